"""CPU checks of Cal-QL's interface: header and ctypes agree on the new exports and on metric slot 15; the version, exorl_agent_cfg,
exorl_batch_out, the metric count and the list of kind ids are what they were; exorl_agent_calql_bytes is the padded layout and refuses every
other kind and every configuration exorl_agent_create refuses; CQL's workspaces and plans did not move; the refusals that need no device;
the class facts. No GPU is touched."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
NEW = ('exorl_replay_build_returns', 'exorl_replay_returns', 'exorl_replay_returns_read', 'exorl_replay_sample_mc', 'exorl_agent_calql_bytes',
       'exorl_agent_set_calql', 'exorl_cql_dq_rows')


@pytest.fixture(scope='module')
def lib():
    from exorl_amd import _lib as L
    return L.load()


def _cfg(kind, O=24, A=6, H=128, B=64, prec=0, ws=1, lagrange=0):
    from exorl_amd import _lib as L
    return L.AgentCfg(kind, O, A, H, B, prec, ws, 0, 1e-4, 0.01, 0.01, 0.3, 0, 10, 0, 3, lagrange, 5.0, 0)


def test_constants_match_the_header(lib):
    from exorl_amd import _lib as L
    header = (ROOT / 'include' / 'exorl_hip.h').read_text()
    d = {k: int(v) for k, v in re.findall(r'#define EXORL_([A-Z0-9_]+)\s+(\d+)', header)}
    assert d['ABI_VERSION'] == 13 == lib.exorl_abi_version() and d['N_METRICS'] == L.N_METRICS == 16
    assert ctypes.sizeof(L.AgentCfg) == 80 and ctypes.sizeof(L.BatchOut) == 104
    assert d['M_CALQL_BOUND'] == L.M_CALQL_BOUND == 15
    assert d['M_ACTOR_ENT'] == L.M_ACTOR_ENT == 14 and d['M_CRITIC_CQL'] == L.M_CRITIC_CQL == 10          # CQL's other slots stay
    kinds = sorted(v for k, v in d.items() if k.startswith('AGENT_') and not k.startswith('AGENT_XCHG'))
    assert kinds == [0, 1, 2, 3, 4, 5, 6, 8, 9, 11]          # the setting adds no kind id
    for fn in NEW:
        assert fn in L.PROTOTYPES and re.search(rf'\b{fn}\(', header), fn
        assert getattr(lib, fn) is not None
    # the prototypes' arities are the header's
    for fn in NEW:
        args = re.search(rf'^(?:int|size_t) {fn}\(([^;]*)\);', header, re.M).group(1)
        assert len(L.PROTOTYPES[fn][1]) == args.count(',') + 1, fn


@pytest.mark.parametrize('B', [7, 257, 1024])
def test_calql_bytes_is_the_padded_layout(lib, B):
    """One run, mc_return (B), padded to 64 floats; the same at every precision and world size, with and without the multiplier."""
    from exorl_amd import _lib as L
    want = 4 * (-(-B // 64) * 64)
    for prec in (0, 2, 3):
        for ws in (1, 2):
            for lag in (0, 1):
                assert lib.exorl_agent_calql_bytes(ctypes.byref(_cfg(L.AGENT_CQL, B=B, prec=prec, ws=ws, lagrange=lag))) == want, (prec, ws, lag)
    assert want % 256 == 0
    if B % 8 == 0:
        assert lib.exorl_agent_calql_bytes(ctypes.byref(_cfg(L.AGENT_CQL, B=B, prec=1))) == want


def test_calql_bytes_refuses_other_kinds_and_bad_configurations(lib):
    from exorl_amd import _lib as L
    for kind in range(13):
        if kind == L.AGENT_CQL:
            continue
        cfg = _cfg(kind)
        if kind == L.AGENT_APS:
            cfg.sf_dim = 4
        assert lib.exorl_agent_calql_bytes(ctypes.byref(cfg)) == 0, kind
        err = lib.exorl_last_error()
        known = lib.exorl_agent_workspace_bytes(ctypes.byref(cfg)) > 0
        assert (b'kind %d is not CQL' % kind if known else b'unknown kind %d' % kind) in err, (kind, err)
    k = L.AGENT_CQL
    zero_n = _cfg(k)
    zero_n.n_samples = 0
    bad = [(_cfg(k, A=17), b'action_dim <= 16'), (zero_n, b'n_samples'), (_cfg(k, H=6), b'unsupported dims'), (_cfg(k, B=0), b'unsupported dims'),
           (_cfg(k, O=0), b'unsupported dims'), (_cfg(k, prec=9), b'unknown precision'), (_cfg(k, ws=0), b'world_size'),
           (_cfg(k, B=7, prec=1), b'multiples of 8')]
    for cfg, text in bad:          # the first failing check names the error, the same one for both queries
        assert lib.exorl_agent_calql_bytes(ctypes.byref(cfg)) == 0 and text in lib.exorl_last_error(), text
        mine = lib.exorl_last_error()
        assert lib.exorl_agent_workspace_bytes(ctypes.byref(cfg)) == 0 and lib.exorl_last_error() == mine, text
    assert lib.exorl_agent_calql_bytes(None) == 0 and b'null cfg' in lib.exorl_last_error()


def test_cql_workspaces_and_plans_are_unchanged(lib):
    """The setting lives in the caller's buffer: exorl_agent_workspace_bytes and exorl_agent_update_plan take the configuration alone, and
    give what the parent gave (the recorded sizes of tests/test_iql_abi.py; CQL's four plans)."""
    from exorl_amd import _lib as L
    from exorl_amd.engine import KIND, PRECISION
    from test_iql_abi import PARENT_WORKSPACE
    rows = [r for r in PARENT_WORKSPACE if r[0] == 'cql']
    assert len(rows) == 3
    for kind, O, A, H, B, n, prec, want in rows:
        cfg = L.AgentCfg(KIND[kind], O, A, H, B, PRECISION[prec], 1, 0, 1e-4, 0.01, 2.5, 0.3, 0, n or 10, 0, n or 3, 0, 5.0, 0)
        assert lib.exorl_agent_workspace_bytes(ctypes.byref(cfg)) == want, (kind, prec)
    C, S, G = L.AGENT_XCHG_CRITIC_GRAD, L.AGENT_XCHG_STATS, L.AGENT_XCHG_ACTOR_GRAD
    want = {(0, 1): ([0, 1, 2, 3], [-1] * 4), (0, 2): ([0, 1, 2, 3], [C, S, G, -1]), (1, 1): ([0, 1, 2, 3], [-1] * 4),
            (1, 2): ([4, 5, 1, 2, 3], [S, C, S, G, -1])}
    for (lag, ws), (phases, xchg) in want.items():
        ph, x, n = (ctypes.c_int32 * 8)(), (ctypes.c_int32 * 8)(), ctypes.c_int32()
        L.check(lib.exorl_agent_update_plan(ctypes.byref(_cfg(L.AGENT_CQL, ws=ws, lagrange=lag)), ph, x, 8, ctypes.byref(n)))
        assert (list(ph[:n.value]), list(x[:n.value])) == (phases, xchg), (lag, ws)


def test_null_handles_and_bad_rows_are_refused(lib):
    assert lib.exorl_agent_set_calql(None, None, 0) != 0 and b'null handle' in lib.exorl_last_error()
    assert lib.exorl_replay_build_returns(None, 0.99, None) != 0 and b'null handle' in lib.exorl_last_error()
    assert lib.exorl_replay_returns(None, None, None, None, None) != 0 and b'null handle' in lib.exorl_last_error()
    buf = np.zeros(4, np.float32)
    assert lib.exorl_replay_returns_read(None, buf.ctypes.data, 4, None) != 0 and b'null argument' in lib.exorl_last_error()
    assert lib.exorl_replay_sample_mc(None, 4, 1, 0.99, 2, None, None, None, None, None) != 0 and b'null argument' in lib.exorl_last_error()
    assert lib.exorl_cql_dq_rows(None, None, None, None, None, 4, 1, 0.01, 0.25, None, None, None) != 0 and b'bad arguments' in lib.exorl_last_error()


def test_class_facts_need_no_device():
    from exorl_amd import _lib as L
    from exorl_amd import agents
    from exorl_amd.calql import CalQLAgent
    assert agents.CalQLAgent is CalQLAgent and CalQLAgent.__mro__[1] is agents.CQLAgent
    assert CalQLAgent.KIND == 'cql' and CalQLAgent.METRIC_WINDOW is False and CalQLAgent._EVALUATES is False
    assert CalQLAgent.METRICS[:-1] == list(agents.CQLAgent.METRICS) and CalQLAgent.METRICS[-1] == (L.M_CALQL_BOUND, 'calql_bound_rate')
    assert inspect.signature(CalQLAgent.__init__) == inspect.signature(agents.CQLAgent.__init__)
    assert type('Sub', (CalQLAgent,), {})._EVALUATES is False
    assert agents.CQLAgent._EVALUATES is True and agents.CQLAgent.METRIC_WINDOW is True          # the parent's stay
    five = tuple(np.zeros((4, n), np.float32) for n in (3, 2, 1, 1, 3))
    ag = object.__new__(CalQLAgent)
    ag.engine = None
    with pytest.raises(ValueError, match='CalQLAgent.*no mc_return'):
        ag._load_batch(iter([five]))
    with pytest.raises(NotImplementedError):
        ag.evaluate(iter([five]))
    with pytest.raises(AttributeError):
        agents.NoSuchAgent
    # the iterators take the destination as a keyword that defaults to None, and HoldoutIterator inherits ArenaIterator's
    from exorl_amd import replay_buffer as rb
    from exorl_amd.engine import AgentEngine, ReplayEngine
    for fn in (rb.ArenaIterator.sample_into, rb.DeviceReplayIterator.sample_into, ReplayEngine.sample_into):
        assert inspect.signature(fn).parameters['mc_return'].default is None
    assert 'sample_into' not in vars(rb.HoldoutIterator)
    for name in ('calql_bytes', 'set_calql', 'set_mc_return'):
        assert callable(getattr(AgentEngine, name))
    for name in ('build_returns', 'returns_to_go'):
        assert callable(getattr(ReplayEngine, name))
