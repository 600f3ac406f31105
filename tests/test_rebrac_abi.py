"""CPU checks of ReBRAC, a setting of the TD3+BC kind: header and ctypes constants agree, the version, exorl_agent_cfg and the list of kind
ids are what they were, the new exports are declared, exorl_agent_rebrac_bytes is the padded layout and refuses every other kind and every
configuration exorl_agent_create refuses, TD3+BC's workspace and plan did not move, and the refusals that need no device. No GPU is touched."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CHUNK_ROWS = 256             # kernels.h IQL_CHUNK_ROWS


@pytest.fixture(scope='module')
def lib():
    from exorl_amd import _lib as L
    return L.load()


def _cfg(kind, O=24, A=6, H=128, B=64, prec=0, ws=1):
    from exorl_amd import _lib as L
    return L.AgentCfg(kind, O, A, H, B, prec, ws, 0, 1e-4, 0.01, 2.5, 0.3, 0, 10, 0, 3, 0, 5.0, 0)


def test_constants_match_the_header(lib):
    from exorl_amd import _lib as L
    header = (ROOT / 'include' / 'exorl_hip.h').read_text()
    d = {k: int(v) for k, v in re.findall(r'#define EXORL_([A-Z0-9_]+)\s+(\d+)', header)}
    assert d['ABI_VERSION'] == 13 == lib.exorl_abi_version() and d['N_METRICS'] == L.N_METRICS == 16
    assert ctypes.sizeof(L.AgentCfg) == 80 and ctypes.sizeof(L.BatchOut) == 104
    assert d['M_REBRAC_PENALTY'] == L.M_REBRAC_PENALTY == 10 and d['M_REBRAC_VALID'] == L.M_REBRAC_VALID == 11
    kinds = sorted(v for k, v in d.items() if k.startswith('AGENT_') and not k.startswith('AGENT_XCHG'))
    assert kinds == [0, 1, 2, 3, 4, 5, 6, 8, 9, 11]          # ReBRAC adds no kind id
    for fn in ('exorl_agent_rebrac_bytes', 'exorl_agent_set_rebrac', 'exorl_rebrac_rows'):
        assert fn in L.PROTOTYPES and re.search(rf'\b{fn}\(', header), fn
    assert 'no agent kind reads the next action yet' not in header
    kernels = (ROOT / 'exorl_amd' / 'csrc' / 'kernels.h').read_text()
    parts = re.search(r'enum \{ REBRAC_P_PENALTY, REBRAC_P_VALID, REBRAC_P_REWARD, REBRAC_PARTS \};', kernels)
    assert parts and L.REBRAC_PARTS == 3


@pytest.mark.parametrize('O,A,H,B', [(5, 1, 8, 7), (24, 6, 128, 257), (24, 16, 128, 1024)])
def test_rebrac_bytes_is_the_padded_layout(lib, O, A, H, B):
    """Four runs, each padded to 64 floats: next_action (B, A), next_valid (B), r~ (B), the per-chunk sums [chunks(B)][REBRAC_PARTS]. The
    size does not depend on the precision or on world_size."""
    from exorl_amd import _lib as L
    pad = lambda n: -(-n // 64) * 64
    want = 4 * (pad(B * A) + 2 * pad(B) + pad(-(-B // CHUNK_ROWS) * L.REBRAC_PARTS))
    for prec in (0, 2, 3):
        for ws in (1, 2):
            assert lib.exorl_agent_rebrac_bytes(ctypes.byref(_cfg(L.AGENT_TD3_BC, O, A, H, B, prec, ws))) == want, (prec, ws)
    assert want % 256 == 0 and lib.exorl_rebrac_rows is not None and lib.exorl_iql_rows_chunks(B) == -(-B // CHUNK_ROWS)


def test_rebrac_bytes_refuses_other_kinds_and_bad_configurations(lib):
    from exorl_amd import _lib as L
    for kind in range(13):
        if kind == L.AGENT_TD3_BC:
            continue
        cfg = _cfg(kind)
        if kind == L.AGENT_APS:
            cfg.sf_dim = 4
        assert lib.exorl_agent_rebrac_bytes(ctypes.byref(cfg)) == 0, kind
        err = lib.exorl_last_error()
        known = lib.exorl_agent_workspace_bytes(ctypes.byref(cfg)) > 0
        assert (b'kind %d is not TD3+BC' % kind if known else b'unknown kind %d' % kind) in err, (kind, err)
    # what exorl_agent_create refuses, with its own text: dimensions, precision, world_size, plain bf16's multiples of 8, a CQL option
    bad = [(_cfg(L.AGENT_TD3_BC, A=17), b'unsupported dims'), (_cfg(L.AGENT_TD3_BC, H=6), b'unsupported dims'),
           (_cfg(L.AGENT_TD3_BC, B=0), b'unsupported dims'), (_cfg(L.AGENT_TD3_BC, prec=9), b'unknown precision'),
           (_cfg(L.AGENT_TD3_BC, ws=0), b'world_size'), (_cfg(L.AGENT_TD3_BC, B=7, prec=1), b'multiples of 8')]
    lagrange = _cfg(L.AGENT_TD3_BC)
    lagrange.use_critic_lagrange = 1
    bad.append((lagrange, b'CQL option'))
    for cfg, text in bad:
        assert lib.exorl_agent_rebrac_bytes(ctypes.byref(cfg)) == 0 and text in lib.exorl_last_error(), text
        assert lib.exorl_agent_workspace_bytes(ctypes.byref(cfg)) == 0 and text in lib.exorl_last_error(), text
    assert lib.exorl_agent_rebrac_bytes(None) == 0 and b'null cfg' in lib.exorl_last_error()


def test_td3bc_workspace_and_plan_are_unchanged(lib):
    from exorl_amd import _lib as L
    from test_iql_abi import PARENT_WORKSPACE
    from exorl_amd.engine import KIND, PRECISION
    rows = [r for r in PARENT_WORKSPACE if r[0] == 'td3_bc']
    assert rows
    for kind, O, A, H, B, n, prec, want in rows:
        cfg = L.AgentCfg(KIND[kind], O, A, H, B, PRECISION[prec], 1, 0, 1e-4, 0.01, 2.5, 0.3, 0, n or 10, 0, n or 3, 0, 5.0, 0)
        assert lib.exorl_agent_workspace_bytes(ctypes.byref(cfg)) == want
    for ws, xchg in ((1, [-1, -1, -1, -1]), (2, [L.AGENT_XCHG_CRITIC_GRAD, L.AGENT_XCHG_STATS, L.AGENT_XCHG_ACTOR_GRAD, -1])):
        ph, x, n = (ctypes.c_int32 * 8)(), (ctypes.c_int32 * 8)(), ctypes.c_int32()
        L.check(lib.exorl_agent_update_plan(ctypes.byref(_cfg(L.AGENT_TD3_BC, ws=ws)), ph, x, 8, ctypes.byref(n)))
        assert (list(ph[:n.value]), list(x[:n.value])) == ([0, 1, 2, 3], xchg)


def test_null_handle_and_bad_rows_are_refused(lib):
    assert lib.exorl_agent_set_rebrac(None, None, 0, 1.0) != 0 and b'null handle' in lib.exorl_last_error()
    assert lib.exorl_rebrac_rows(None, 7, None, 1, None, None, None, 4, 1, 1.0, 0.25, None, None, None, None) != 0
    assert b'bad arguments' in lib.exorl_last_error()


def test_python_refusals_need_no_device():
    """A plain iterator of 5-tuples has no next action: ValueError naming the class, before the engine is touched. Coefficients are judged
    before anything is built."""
    import numpy as np
    from exorl_amd import agents
    from exorl_amd.rebrac import ReBRACAgent
    assert agents.ReBRACAgent is ReBRACAgent and issubclass(ReBRACAgent, agents.TD3BCAgent)
    assert ReBRACAgent.KIND == 'td3_bc' and ReBRACAgent.METRIC_WINDOW is False and ReBRACAgent._EVALUATES is False
    assert agents.TD3BCAgent._EVALUATES is True and agents.TD3BCAgent.METRIC_WINDOW is True
    sub = type('Sub', (ReBRACAgent,), {})                                 # a subclass keeps the class's own declaration ...
    assert sub._EVALUATES is False and type('SubSub', (sub,), {})._EVALUATES is False
    assert type('Other', (sub,), {'KIND': 'td3'})._EVALUATES is True      # ... until it names a kind of its own
    assert agents.TD3Agent._EVALUATES is True and agents.IQLAgent._EVALUATES is False and type('T', (agents.TD3BCAgent,), {})._EVALUATES is True
    from exorl_amd import _lib as L
    assert ReBRACAgent.METRICS[:6] == agents.TD3BCAgent.METRICS and [s for s, _ in ReBRACAgent.METRICS[6:]] == [L.M_REBRAC_PENALTY, L.M_REBRAC_VALID]
    ag = object.__new__(ReBRACAgent)
    five = tuple(np.zeros((4, n), np.float32) for n in (3, 2, 1, 1, 3))
    with pytest.raises(ValueError, match='ReBRACAgent.*no next_action'):
        ag._load_batch(iter([five]))
    args = ('rebrac', (5,), (2,), 'cuda', 1e-4, 8, 0.01, 0.2, 1, 8, 0.3, False)
    for kw, text in ((dict(actor_bc_coef=-1.0), 'actor_bc_coef'), (dict(actor_bc_coef=0.0), 'actor_bc_coef'),
                     (dict(critic_bc_coef=-0.5), 'critic_bc_coef'), (dict(critic_bc_coef=float('nan')), 'critic_bc_coef')):
        with pytest.raises(ValueError, match=text):
            ReBRACAgent(*args, **kw)
    with pytest.raises(NotImplementedError):
        ag.evaluate(iter([five]))
