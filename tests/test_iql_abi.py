"""CPU checks of the IQL kind's C ABI: header and ctypes constants agree, the version and exorl_agent_cfg are what they were, the step's plan,
kind 7 still refused, exorl_agent_set_iql's value refusals, and the workspace of existing-kind configurations byte for byte what the build
before IQL gave. No GPU is touched. (exorl_agent_set_iql's refusals that need a handle — another kind, a captured graph — are in
tests/test_gpu_iql.py: a handle needs a device.)"""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]

# (kind, O, A, H, B, n, precision, exorl_agent_workspace_bytes) — the first case of every (kind, precision) in tests/_grad_grid.CASES, sizes recorded
# from the library built at the commit before the IQL kind
PARENT_WORKSPACE = [
    ('td3_bc', 5, 1, 100, 7, 0, 'fp32', 771584),
    ('td3', 4, 2, 4, 1, 0, 'fp32', 18944),
    ('ddpg', 24, 9, 192, 72, 0, 'fp32', 3892992),
    ('bc', 24, 6, 100, 7, 0, 'fp32', 330752),
    ('crr', 11, 3, 100, 50, 7, 'fp32', 1896192),
    ('cql', 5, 3, 32, 7, 3, 'fp32', 249344),
    ('td3_bc', 24, 6, 128, 64, 0, 'bf16x3', 3144448),
    ('td3', 17, 6, 128, 128, 0, 'bf16x3', 4402688),
    ('ddpg', 24, 9, 256, 64, 0, 'bf16x3', 7996928),
    ('bc', 24, 6, 128, 64, 0, 'bf16x3', 1047296),
    ('crr', 24, 6, 128, 64, 7, 'bf16x3', 4119552),
    ('cql', 24, 6, 128, 64, 3, 'bf16x3', 9103360),
    ('td3_bc', 24, 6, 256, 1024, 0, 'bf16', 42061824),
    ('td3', 17, 6, 192, 1000, 0, 'bf16', 29580544),
    ('ddpg', 24, 6, 384, 1024, 0, 'bf16', 54670848),
    ('bc', 24, 6, 128, 1024, 0, 'bf16', 7559936),
    ('cql', 24, 6, 128, 256, 3, 'bf16', 26531072),
]


@pytest.fixture(scope='module')
def lib():
    from exorl_amd import _lib as L
    return L.load()


def _cfg(kind, O=24, A=6, H=128, B=64, prec=0, ws=1, n=0):
    from exorl_amd import _lib as L
    return L.AgentCfg(kind, O, A, H, B, prec, ws, 0, 1e-4, 0.01, 2.5, 0.3, 0, n or 10, 0, n or 3, 0, 5.0, 0)


def test_constants_match_the_header():
    from exorl_amd import _lib as L
    header = (ROOT / 'include' / 'exorl_hip.h').read_text()
    d = {k: int(v) for k, v in re.findall(r'#define EXORL_([A-Z0-9_]+)\s+(\d+)', header)}
    assert d['ABI_VERSION'] == 13 and d['N_METRICS'] == L.N_METRICS == 16
    assert d['AGENT_IQL'] == L.AGENT_IQL == 8 and d['NET_VALUE'] == L.NET_VALUE == 3 and d['AGENT_XCHG_VALUE_GRAD'] == L.AGENT_XCHG_VALUE_GRAD == 3
    assert 7 not in [v for k, v in d.items() if k.startswith('AGENT_') and not k.startswith('AGENT_XCHG')]
    for k in ('M_VALUE_LOSS', 'M_VALUE', 'M_ADV', 'M_ACTOR_WEIGHT'):
        assert d[k] == getattr(L, k)
    assert [d[k] for k in ('M_VALUE_LOSS', 'M_VALUE', 'M_ADV', 'M_ACTOR_WEIGHT')] == [10, 11, 12, 13]
    assert re.search(r'int exorl_agent_set_iql\(exorl_agent_t\* a, float expectile, float temperature, float max_weight\);', header)
    assert 'exorl_agent_set_iql' in L.PROTOTYPES and 'exorl_iql_rows' in L.PROTOTYPES


def test_version_and_cfg_layout(lib):
    from exorl_amd import _lib as L
    assert lib.exorl_abi_version() == 13
    assert ctypes.sizeof(L.AgentCfg) == 80          # 8 int32, 4 float, uint64, 4 int32, float, int32: what it was before the IQL kind


@pytest.mark.parametrize('ws,want', [(1, [-1, -1, -1, -1]), (2, [3, 0, 2, -1])])
def test_plan_is_four_phases_with_three_gradient_exchanges(lib, ws, want):
    from exorl_amd import _lib as L
    ph, x, n = (ctypes.c_int32 * 8)(), (ctypes.c_int32 * 8)(), ctypes.c_int32()
    L.check(lib.exorl_agent_update_plan(ctypes.byref(_cfg(L.AGENT_IQL, ws=ws)), ph, x, 8, ctypes.byref(n)))
    assert n.value == 4 and list(ph[:4]) == [6, 7, 8, 9] and list(x[:4]) == want
    assert lib.exorl_agent_workspace_bytes(ctypes.byref(_cfg(L.AGENT_IQL))) > 0


def test_kind_7_is_still_refused(lib):
    assert lib.exorl_agent_workspace_bytes(ctypes.byref(_cfg(7))) == 0
    assert b'unknown kind 7' in lib.exorl_last_error()
    ph, x, n = (ctypes.c_int32 * 8)(), (ctypes.c_int32 * 8)(), ctypes.c_int32()
    assert lib.exorl_agent_update_plan(ctypes.byref(_cfg(7)), ph, x, 8, ctypes.byref(n)) != 0


@pytest.mark.parametrize('triple', [(0.0, 3.0, 100.0), (1.0, 3.0, 100.0), (-0.1, 3.0, 100.0), (float('nan'), 3.0, 100.0), (0.7, -1.0, 100.0),
                                    (0.7, 3.0, 0.0), (0.7, 3.0, -5.0)])
def test_set_iql_refuses_bad_values_before_it_looks_at_the_handle(lib, triple):
    assert lib.exorl_agent_set_iql(None, *triple) != 0
    assert b'needs 0 < expectile < 1' in lib.exorl_last_error()


def test_set_iql_refuses_a_null_handle(lib):
    assert lib.exorl_agent_set_iql(None, 0.7, 3.0, 100.0) != 0
    assert b'null handle' in lib.exorl_last_error()


@pytest.mark.parametrize('row', PARENT_WORKSPACE, ids=lambda r: f'{r[0]}-{r[6]}')
def test_existing_workspaces_keep_their_size(lib, row):
    from exorl_amd.engine import KIND, PRECISION
    kind, O, A, H, B, n, prec, want = row
    assert lib.exorl_agent_workspace_bytes(ctypes.byref(_cfg(KIND[kind], O, A, H, B, PRECISION[prec], 1, n))) == want
