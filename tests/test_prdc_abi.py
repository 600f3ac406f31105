"""CPU checks of the PRDC kind: header and ctypes constants agree, the version, counts and exorl_agent_cfg are what they were, the new
exports are declared, which kind ids are accepted, the step's plan, the refusal of world_size > 1 wherever a configuration is judged, and
the workspace: TD3+BC's layout with the search's buffers behind it, every other kind's size untouched. No GPU is touched."""
import ctypes
import re
from pathlib import Path

import pytest

from test_fqe_abi import PARENT_IQL_WORKSPACE
from test_iql_abi import PARENT_WORKSPACE

ROOT = Path(__file__).resolve().parents[1]
NN_MAX_SPLITS = 256          # kernels.h


@pytest.fixture(scope='module')
def lib():
    from exorl_amd import _lib as L
    return L.load()


def _cfg(kind, O=24, A=6, H=128, B=64, prec=0, ws=1, n=0):
    from exorl_amd import _lib as L
    return L.AgentCfg(kind, O, A, H, B, prec, ws, 0, 1e-4, 0.01, 2.5, 0.3, 0, n or 10, 0, n or 3, 0, 5.0, 0)


def _plan(lib, cfg):
    from exorl_amd import _lib as L
    ph, x, n = (ctypes.c_int32 * 8)(), (ctypes.c_int32 * 8)(), ctypes.c_int32()
    L.check(lib.exorl_agent_update_plan(ctypes.byref(cfg), ph, x, 8, ctypes.byref(n)))
    return list(ph[:n.value]), list(x[:n.value])


def test_constants_match_the_header(lib):
    from exorl_amd import _lib as L
    from exorl_amd.engine import KIND, KIND_BEYOND_REFERENCE, kind_id
    header = (ROOT / 'include' / 'exorl_hip.h').read_text()
    d = {k: int(v) for k, v in re.findall(r'#define EXORL_([A-Z0-9_]+)\s+(\d+)', header)}
    assert d['ABI_VERSION'] == 13 == lib.exorl_abi_version() and d['N_METRICS'] == L.N_METRICS == 16
    assert ctypes.sizeof(L.AgentCfg) == 80
    assert d['AGENT_PRDC'] == L.AGENT_PRDC == kind_id('prdc') and 'prdc' in KIND_BEYOND_REFERENCE and 'prdc' not in KIND
    assert d['M_NN_DIST'] == L.M_NN_DIST == 10
    kinds = sorted(v for k, v in d.items() if k.startswith('AGENT_') and not k.startswith('AGENT_XCHG'))
    assert kinds == [0, 1, 2, 3, 4, 5, 6, 8, 9, L.AGENT_PRDC]
    for fn in ('exorl_replay_build_keys', 'exorl_replay_keys', 'exorl_replay_keys_read', 'exorl_nn_search', 'exorl_agent_set_prdc',
               'exorl_agent_nn_result'):
        assert fn in L.PROTOTYPES and re.search(rf'\b{fn}\(', header), fn


def test_prdc_is_accepted_and_unassigned_kinds_are_refused(lib):
    from exorl_amd import _lib as L
    assert lib.exorl_agent_workspace_bytes(ctypes.byref(_cfg(L.AGENT_PRDC))) > 0
    for kind in (7, 10, 12):
        assert lib.exorl_agent_workspace_bytes(ctypes.byref(_cfg(kind))) == 0 and f'unknown kind {kind}'.encode() in lib.exorl_last_error()


def test_plan_is_td3bcs_with_the_search_behind_phase_0(lib):
    from exorl_amd import _lib as L
    assert _plan(lib, _cfg(L.AGENT_PRDC)) == ([0, 12, 1, 2, 3], [-1] * 5)
    assert _plan(lib, _cfg(L.AGENT_TD3_BC)) == ([0, 1, 2, 3], [-1] * 4)


def test_no_other_kind_plans_phase_12(lib):
    from exorl_amd import _lib as L
    from exorl_amd.engine import KIND
    for kind in list(KIND.values()) + [L.AGENT_IQL, L.AGENT_FQE]:
        for ws in (1, 2):
            cfg = _cfg(kind, ws=ws)
            if kind == L.AGENT_APS:
                cfg.sf_dim = 4
            assert 12 not in _plan(lib, cfg)[0], kind


def test_world_size_2_is_refused_wherever_a_configuration_is_judged(lib):
    from exorl_amd import _lib as L
    cfg = _cfg(L.AGENT_PRDC, ws=2)
    assert lib.exorl_agent_workspace_bytes(ctypes.byref(cfg)) == 0 and b'world_size=2' in lib.exorl_last_error()
    ph, x, n = (ctypes.c_int32 * 8)(), (ctypes.c_int32 * 8)(), ctypes.c_int32()
    assert lib.exorl_agent_update_plan(ctypes.byref(cfg), ph, x, 8, ctypes.byref(n)) != 0 and b"rank's shard" in lib.exorl_last_error()
    assert lib.exorl_agent_metric_window_bytes(ctypes.byref(cfg)) == 0
    # exorl_agent_create judges the configuration before it touches the device
    h = ctypes.c_void_p()
    assert lib.exorl_agent_create(ctypes.byref(cfg), None, 0, ctypes.byref(h)) != 0 and b'world_size=2' in lib.exorl_last_error() and not h.value


def test_prdc_workspace_is_td3bcs_plus_the_search_buffers(lib):
    """The kind carves TD3+BC's layout and, behind it, six 64-float-padded runs: the queries (B, round_up(O + A, 4)), the partial minima
    and their indices (NN_MAX_SPLITS, B) each, idx (B), d2 (B) and a_nn (B, A)."""
    from exorl_amd import _lib as L
    pad = lambda n: -(-n // 64) * 64
    for O, A, H, B, prec in [(5, 1, 100, 7, 0), (24, 6, 128, 64, 2), (24, 6, 128, 128, 3), (24, 6, 256, 1024, 1), (27, 6, 64, 1000, 0),
                             (240, 16, 128, 64, 0)]:
        td = lib.exorl_agent_workspace_bytes(ctypes.byref(_cfg(L.AGENT_TD3_BC, O, A, H, B, prec)))
        pr = lib.exorl_agent_workspace_bytes(ctypes.byref(_cfg(L.AGENT_PRDC, O, A, H, B, prec)))
        pitch = -(-(O + A) // 4) * 4
        extra = pad(B * pitch) + 2 * pad(NN_MAX_SPLITS * B) + 2 * pad(B) + pad(B * A)
        assert td > 0 and pr == td + 4 * extra, (O, A, H, B, prec, td, pr, extra)


@pytest.mark.parametrize('row', PARENT_WORKSPACE, ids=lambda r: f'{r[0]}-{r[6]}')
def test_existing_workspaces_keep_their_size(lib, row):
    from exorl_amd.engine import KIND, PRECISION
    kind, O, A, H, B, n, prec, want = row
    assert lib.exorl_agent_workspace_bytes(ctypes.byref(_cfg(KIND[kind], O, A, H, B, PRECISION[prec], 1, n))) == want


@pytest.mark.parametrize('row', PARENT_IQL_WORKSPACE, ids=lambda r: f'iql-{r[4]}')
def test_iql_and_fqe_workspaces_keep_their_size(lib, row):
    from exorl_amd import _lib as L
    from exorl_amd.engine import PRECISION
    O, A, H, B, prec, want = row
    assert lib.exorl_agent_workspace_bytes(ctypes.byref(_cfg(L.AGENT_IQL, O, A, H, B, PRECISION[prec]))) == want
    td3 = lib.exorl_agent_workspace_bytes(ctypes.byref(_cfg(L.AGENT_TD3, O, A, H, B, PRECISION[prec])))
    fqe = lib.exorl_agent_workspace_bytes(ctypes.byref(_cfg(L.AGENT_FQE, O, A, H, B, PRECISION[prec])))
    assert fqe == td3 + 4 * (-(-(6 * -(-B // 256)) // 64) * 64)


def test_null_handles_are_refused(lib):
    assert lib.exorl_agent_set_prdc(None, None, 2.0) != 0 and b'null argument' in lib.exorl_last_error()
    assert lib.exorl_replay_build_keys(None, 2.0, 1, None) != 0 and b'null handle' in lib.exorl_last_error()
    assert lib.exorl_nn_search(None, 1, 4, 3, None, 4, 1, 0, None, None, None) != 0 and b'null argument' in lib.exorl_last_error()


def test_bind_dataset_refusals_need_no_device():
    """bind_dataset judges the iterator before it touches the engine: no arena, several shards, pixels."""
    import numpy as np
    from types import SimpleNamespace
    from exorl_amd.agents import PRDCAgent
    ag = object.__new__(PRDCAgent)
    ag.beta = 2.0
    with pytest.raises(ValueError, match='HBM arena'):
        ag.bind_dataset(iter([]))
    arena = lambda dt, shape, k=1: SimpleNamespace(obs_dtype=np.dtype(dt), obs_shape=shape, frame_stack=k)
    with pytest.raises(ValueError, match='2 shards'):
        ag.bind_dataset(SimpleNamespace(_arenas=lambda: [arena(np.float32, (24,)), arena(np.float32, (24,))]))
    with pytest.raises(ValueError, match='not pixels'):
        ag.bind_dataset(SimpleNamespace(_arenas=lambda: [arena(np.uint8, (9, 84, 84), 3)]))
    with pytest.raises(ValueError, match='not pixels'):
        ag.bind_dataset(SimpleNamespace(_arenas=lambda: [arena(np.uint8, (24,))]))
    assert ag.nn_table_rows == 0 and PRDCAgent.METRIC_WINDOW is False and PRDCAgent._EVALUATES is False
