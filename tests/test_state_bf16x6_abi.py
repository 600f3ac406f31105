"""CPU checks of the bf16x6 state-agent work: the new export and its binding, the ABI version, workspace sizes of the other precisions
(the three-plane buffers are carved under bf16x6 only), and the new gradient-grid cases against what tests/test_twin64.py asks of a case."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import _grad_grid as G
import _state_bf16x6_cases as S

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope='module')
def lib():
    return ctypes.CDLL(str(ROOT / 'exorl_amd' / 'libexorl_hip.so'))


def test_library_exports_gemm_planes3(lib):
    assert hasattr(lib, 'exorl_gemm_planes3')
    assert hasattr(lib, 'exorl_gemm_planes') and hasattr(lib, 'exorl_gemm')


def test_binding_matches_the_header():
    from exorl_amd import _lib as L
    header = (ROOT / 'include' / 'exorl_hip.h').read_text()
    m = re.search(r'int exorl_gemm_planes3\((.*?)\);', header, re.S)
    assert m, 'exorl_gemm_planes3 is not declared in include/exorl_hip.h'
    n_header = len([a for a in m.group(1).split(',') if a.strip()])
    res, args = L.PROTOTYPES['exorl_gemm_planes3']
    assert res is ctypes.c_int and len(args) == n_header == 18
    two = re.search(r'int exorl_gemm_planes\((.*?)\);', header, re.S)
    assert len(args) == len([a for a in two.group(1).split(',') if a.strip()]) + 2 == len(L.PROTOTYPES['exorl_gemm_planes'][1]) + 2


def test_abi_version_is_unchanged(lib):
    lib.exorl_abi_version.restype = ctypes.c_int
    assert lib.exorl_abi_version() == 13


# (kind, O, A, H, B, precision) -> exorl_agent_workspace_bytes computed on the parent commit
WORKSPACE_BYTES = [
    ((0, 24, 6, 1024, 1024, 0), 178780160),      # td3_bc, fp32
    ((0, 24, 6, 1024, 1024, 1), 216987648),      # td3_bc, bf16
    ((0, 24, 6, 1024, 1024, 2), 255064064),      # td3_bc, bf16x3
    ((5, 24, 6, 128, 128, 0), 11627520),         # cql, fp32
    ((4, 24, 6, 128, 128, 2), 7326464),          # crr, bf16x3
    ((3, 24, 6, 384, 1024, 1), 54670848),        # ddpg, bf16
    # every kind in every precision, on and off the plane routes; a seventh entry is sf_dim (APS)
    ((0, 24, 6, 128, 128, 3), 4638976),          # td3_bc, bf16x6 on the plane route
    ((3, 24, 6, 128, 128, 3), 3975424),          # ddpg, bf16x6 on the plane route
    ((2, 24, 6, 128, 128, 3), 1538816),          # bc, bf16x6 on the plane route
    ((4, 24, 6, 128, 128, 3), 9390848),          # crr, bf16x6 on the plane route
    ((5, 24, 6, 128, 128, 3), 16542720),         # cql, bf16x6 on the plane route
    ((1, 24, 6, 128, 128, 3), 4638976),          # td3, bf16x6 on the plane route
    ((0, 24, 6, 192, 72, 3), 4316416),           # td3_bc, bf16x6 off it
    ((5, 24, 6, 128, 64, 2), 9103360),           # cql, bf16x3 on the plane pipeline
    ((4, 24, 6, 128, 64, 2), 4537344),           # crr, bf16x3 on the plane pipeline
    ((2, 24, 6, 128, 64, 2), 1047296),           # bc, bf16x3 on the plane pipeline
    ((1, 24, 6, 128, 64, 2), 3144448),           # td3, bf16x3 on the plane pipeline
    ((3, 24, 6, 192, 72, 2), 3830528),           # ddpg, bf16x3 off it
    ((1, 24, 6, 192, 72, 1), 5130496),           # td3, bf16
    ((2, 24, 6, 256, 256, 1), 4950784),          # bc, bf16
    ((4, 24, 6, 256, 256, 1), 22636032),         # crr, bf16
    ((5, 24, 6, 256, 256, 1), 54419712),         # cql, bf16
    ((1, 24, 6, 100, 7, 0), 993792),             # td3, fp32
    ((2, 24, 6, 100, 7, 0), 330752),             # bc, fp32
    ((4, 24, 6, 100, 8, 0), 1141248),            # crr, fp32
    ((3, 24, 6, 320, 1000, 0), 36042752),        # ddpg, fp32
    ((6, 34, 6, 128, 128, 0, 10), 3298048),      # aps, fp32
    ((6, 34, 6, 128, 128, 1, 10), 3855104),      # aps, bf16
    ((6, 34, 6, 128, 128, 2, 10), 4395776),      # aps, bf16x3 on the plane pipeline
    ((6, 34, 6, 128, 128, 3, 10), 4477696),      # aps, bf16x6 on the plane route
]


@pytest.mark.parametrize('cfg,want', WORKSPACE_BYTES)
def test_workspace_bytes_of_the_other_precisions_are_unchanged(lib, cfg, want):
    from exorl_amd import _lib as L
    lib.exorl_agent_workspace_bytes.restype = ctypes.c_size_t
    kind, O, A, H, B, prec, *sf_dim = cfg
    c = L.AgentCfg(kind, O, A, H, B, prec, 1, sf_dim[0] if sf_dim else 0, 1e-4, 0.01, 2.5, 0.3, 0, 10, 1, 3, 0, 5.0, 0)
    assert lib.exorl_agent_workspace_bytes(ctypes.byref(c)) == want


def test_bf16x6_workspace_holds_the_plane_buffers_only_on_the_plane_route(lib):
    """bf16x6 is accepted on states; on the plane route its workspace is fp32 mode's plus the plane images, elsewhere exactly fp32 mode's."""
    from exorl_amd import _lib as L
    lib.exorl_agent_workspace_bytes.restype = ctypes.c_size_t
    ws = lambda H, B, p: lib.exorl_agent_workspace_bytes(ctypes.byref(L.AgentCfg(0, 24, 6, H, B, p, 1, 0, 1e-4, 0.01, 2.5, 0.3, 0, 10, 1, 3, 0, 5.0, 0)))
    assert ws(128, 128, 3) > ws(128, 128, 0) > 0
    assert ws(192, 72, 3) == ws(192, 72, 0) > 0
    assert ws(128, 64, 3) == ws(128, 64, 0) > 0


def _near_kink(res, delta):
    return {s: int(sum((r['z'].abs() < delta * r['z'].abs().max()).sum() for r in relus)) for s, relus in res.relus.items()}


@pytest.mark.parametrize('c', [pytest.param(c, id=G.case_id(c)) for c in S.NEW_PLANE_CASES])
def test_new_case_qualifies(c):
    """What tests/test_twin64.py::test_case_qualifies asks of a table case, for the new seeds (re-checked, not searched): twin32 and twin64
    agree on every discrete decision, each with float64 margin >= 1e-4; at most 64 near-kink elements at delta = 2^-18."""
    r64, r32 = G.run_twin(c, torch.float64), G.run_twin(c, torch.float32)
    assert r64.decisions.keys() == r32.decisions.keys()
    for k, (d, margin) in r64.decisions.items():
        assert np.array_equal(d, r32.decisions[k][0]), f'{k}: {int((d != r32.decisions[k][0]).sum())} rows decided differently in float32'
        assert margin.size == 0 or margin.min() >= G.MARGIN, f'{k}: margin {margin.min():.2e}'
    k18 = _near_kink(r64, S.KINK_DELTA)
    print(f'[case] {G.case_id(c)}: |K(2^-18)| {k18}')
    assert S.KINK_DELTA == 2.0 ** -18 and max(k18.values()) <= G.KINK_CAP == 64, k18
    assert c.bar == 'tight' and S.on_plane_route(c)


def test_case_lists():
    assert all(S.on_plane_route(c) for c in S.PLANE_CASES) and not any(S.on_plane_route(c) for c in S.GENERIC_CASES)
    assert [(c.kind, c.H, c.B) for c in S.GENERIC_CASES] == [('td3_bc', 100, 7), ('td3', 4, 1), ('ddpg', 192, 72), ('td3_bc', 320, 1000), ('cql', 100, 50)]
    assert {G.base_kind(c) for c in S.PLANE_CASES} == {'td3', 'ddpg', 'td3_bc', 'bc', 'crr', 'cql'}
    assert any(G.base_kind(c) == 'cql' and (3 * c.n + 1) * c.B >= 8192 for c in S.PLANE_CASES)
    assert len({G.case_id(c) for c in S.CASES}) == len(S.CASES)
