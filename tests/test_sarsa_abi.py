"""CPU checks of the SARSA setting of the TD3+BC, TD3, CRR and FQE kinds: header and ctypes constants agree, the version, exorl_agent_cfg,
exorl_batch_out and the list of kind ids are what they were, the new exports are declared, exorl_agent_sarsa_bytes is the padded layout and
refuses every other kind and every configuration exorl_agent_create refuses, the four kinds' workspaces and plans did not move, the
refusals that need no device, the class facts, and the float64 twin on hand-computed rows. No GPU is touched."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
CHUNK_ROWS = 256             # kernels.h IQL_CHUNK_ROWS
SARSA_KINDS = ('TD3_BC', 'TD3', 'CRR', 'FQE')


@pytest.fixture(scope='module')
def lib():
    from exorl_amd import _lib as L
    return L.load()


def _cfg(kind, O=24, A=6, H=128, B=64, prec=0, ws=1):
    from exorl_amd import _lib as L
    return L.AgentCfg(kind, O, A, H, B, prec, ws, 0, 1e-4, 0.01, 2.5, 0.3, 0, 10, 0, 3, 0, 5.0, 0)


def _kinds():
    from exorl_amd import _lib as L
    return [getattr(L, f'AGENT_{k}') for k in SARSA_KINDS]


def test_constants_match_the_header(lib):
    from exorl_amd import _lib as L
    header = (ROOT / 'include' / 'exorl_hip.h').read_text()
    d = {k: int(v) for k, v in re.findall(r'#define EXORL_([A-Z0-9_]+)\s+(\d+)', header)}
    assert d['ABI_VERSION'] == 13 == lib.exorl_abi_version() and d['N_METRICS'] == L.N_METRICS == 16
    assert ctypes.sizeof(L.AgentCfg) == 80 and ctypes.sizeof(L.BatchOut) == 104
    assert d['M_SARSA_VALID'] == L.M_SARSA_VALID == 11
    assert d['M_REBRAC_PENALTY'] == L.M_REBRAC_PENALTY == 10 and d['M_REBRAC_VALID'] == L.M_REBRAC_VALID == 11
    kinds = sorted(v for k, v in d.items() if k.startswith('AGENT_') and not k.startswith('AGENT_XCHG'))
    assert kinds == [0, 1, 2, 3, 4, 5, 6, 8, 9, 11]          # the setting adds no kind id
    for fn in ('exorl_agent_sarsa_bytes', 'exorl_agent_set_sarsa', 'exorl_next_action_rows'):
        assert fn in L.PROTOTYPES and re.search(rf'\b{fn}\(', header), fn
        assert getattr(lib, fn) is not None
    kernels = (ROOT / 'exorl_amd' / 'csrc' / 'kernels.h').read_text()
    assert re.search(r'enum \{ SARSA_P_VALID, SARSA_PARTS \};', kernels) and L.SARSA_PARTS == 1


@pytest.mark.parametrize('O,A,H,B', [(5, 1, 8, 7), (24, 6, 128, 257), (24, 16, 128, 1024)])
def test_sarsa_bytes_is_the_padded_layout(lib, O, A, H, B):
    """Three runs, each padded to 64 floats: next_action (B, A), next_valid (B), the per-chunk sums [chunks(B)][1]. The size does not depend
    on the kind, the precision or world_size."""
    from exorl_amd import _lib as L
    pad = lambda n: -(-n // 64) * 64
    want = 4 * (pad(B * A) + pad(B) + pad(-(-B // CHUNK_ROWS) * L.SARSA_PARTS))
    for kind in _kinds():
        for prec in (0, 2, 3):
            for ws in (1, 2):
                assert lib.exorl_agent_sarsa_bytes(ctypes.byref(_cfg(kind, O, A, H, B, prec, ws))) == want, (kind, prec, ws)
    assert want % 256 == 0 and lib.exorl_iql_rows_chunks(B) == -(-B // CHUNK_ROWS)


def test_sarsa_bytes_refuses_other_kinds_and_bad_configurations(lib):
    from exorl_amd import _lib as L
    ok = _kinds()
    for kind in range(13):
        if kind in ok:
            continue
        cfg = _cfg(kind)
        if kind == L.AGENT_APS:
            cfg.sf_dim = 4
        assert lib.exorl_agent_sarsa_bytes(ctypes.byref(cfg)) == 0, kind
        err = lib.exorl_last_error()
        known = lib.exorl_agent_workspace_bytes(ctypes.byref(cfg)) > 0
        assert (b'kind %d is not ' % kind if known else b'unknown kind %d' % kind) in err, (kind, err)
    for kind in ok:
        bad = [(_cfg(kind, A=17), b'unsupported dims'), (_cfg(kind, H=6), b'unsupported dims'), (_cfg(kind, B=0), b'unsupported dims'),
               (_cfg(kind, prec=9), b'unknown precision'), (_cfg(kind, ws=0), b'world_size'), (_cfg(kind, B=7, prec=1), b'multiples of 8')]
        lagrange = _cfg(kind)
        lagrange.use_critic_lagrange = 1
        bad.append((lagrange, b'CQL option'))
        for cfg, text in bad:
            assert lib.exorl_agent_sarsa_bytes(ctypes.byref(cfg)) == 0 and text in lib.exorl_last_error(), (kind, text)
            assert lib.exorl_agent_workspace_bytes(ctypes.byref(cfg)) == 0 and text in lib.exorl_last_error(), (kind, text)
    assert lib.exorl_agent_sarsa_bytes(None) == 0 and b'null cfg' in lib.exorl_last_error()
    # ReBRAC's own query is where it was
    assert lib.exorl_agent_rebrac_bytes(ctypes.byref(_cfg(L.AGENT_TD3))) == 0 and b'is not TD3+BC' in lib.exorl_last_error()


def test_workspaces_and_plans_of_the_four_kinds_are_unchanged(lib):
    from exorl_amd import _lib as L
    from exorl_amd.engine import KIND, PRECISION
    from test_iql_abi import PARENT_WORKSPACE
    rows = [r for r in PARENT_WORKSPACE if r[0] in ('td3_bc', 'td3', 'crr')]
    assert {r[0] for r in rows} == {'td3_bc', 'td3', 'crr'}
    for kind, O, A, H, B, n, prec, want in rows:
        cfg = L.AgentCfg(KIND[kind], O, A, H, B, PRECISION[prec], 1, 0, 1e-4, 0.01, 2.5, 0.3, 0, n or 10, 0, n or 3, 0, 5.0, 0)
        assert lib.exorl_agent_workspace_bytes(ctypes.byref(cfg)) == want, (kind, prec)
    for O, A, H, B, prec in ((5, 1, 100, 7, 0), (24, 6, 128, 64, 2), (24, 6, 256, 1024, 1)):       # FQE's is TD3's plus its row partials
        td3 = lib.exorl_agent_workspace_bytes(ctypes.byref(_cfg(L.AGENT_TD3, O, A, H, B, prec)))
        fqe = lib.exorl_agent_workspace_bytes(ctypes.byref(_cfg(L.AGENT_FQE, O, A, H, B, prec)))
        assert td3 > 0 and fqe == td3 + 4 * (-(-(6 * -(-B // CHUNK_ROWS)) // 64) * 64)
    C, S, G = L.AGENT_XCHG_CRITIC_GRAD, L.AGENT_XCHG_STATS, L.AGENT_XCHG_ACTOR_GRAD
    want = {'TD3_BC': ([0, 1, 2, 3], [C, S, G, -1]), 'TD3': ([0, 1, 2, 3], [C, -1, G, -1]), 'CRR': ([0, 1, 2, 3], [C, -1, G, -1]),
            'FQE': ([10, 11], [C, -1])}
    for name, (phases, xchg) in want.items():
        for ws in (1, 2):
            ph, x, n = (ctypes.c_int32 * 8)(), (ctypes.c_int32 * 8)(), ctypes.c_int32()
            L.check(lib.exorl_agent_update_plan(ctypes.byref(_cfg(getattr(L, f'AGENT_{name}'), ws=ws)), ph, x, 8, ctypes.byref(n)))
            assert (list(ph[:n.value]), list(x[:n.value])) == (phases, xchg if ws == 2 else [-1] * len(phases)), (name, ws)


def test_null_handle_and_bad_rows_are_refused(lib):
    assert lib.exorl_agent_set_sarsa(None, None, 0) != 0 and b'null handle' in lib.exorl_last_error()
    assert lib.exorl_next_action_rows(None, 1, None, 4, 1, 0.25, None, 7, None, None, None) != 0
    assert b'bad arguments' in lib.exorl_last_error()


def test_python_refusals_and_class_facts_need_no_device():
    """A plain iterator of 5-tuples has no next action: ValueError naming the class, before the engine is touched. The classes' declared
    facts; ReBRACAgent's stay what tests/test_rebrac_abi.py pins."""
    from exorl_amd import _lib as L
    from exorl_amd import agents, fqe, onestep
    from exorl_amd.rebrac import ReBRACAgent
    five = tuple(np.zeros((4, n), np.float32) for n in (3, 2, 1, 1, 3))
    for name, cls, parent in (('OneStepTD3BCAgent', onestep.OneStepTD3BCAgent, agents.TD3BCAgent),
                              ('OneStepCRRAgent', onestep.OneStepCRRAgent, agents.CRRAgent), ('BehaviorQAgent', fqe.BehaviorQAgent, agents.FQEAgent)):
        assert getattr(agents, name) is cls and issubclass(cls, parent) and issubclass(cls, agents._NextActionBatch)
        assert cls.KIND == parent.KIND and cls.METRIC_WINDOW is False and cls._EVALUATES is False
        assert cls.METRICS[:-1] == list(parent.METRICS) and cls.METRICS[-1] == (L.M_SARSA_VALID, 'next_valid')
        assert inspect.signature(cls.__init__) == inspect.signature(parent.__init__)
        assert type('Sub', (cls,), {})._EVALUATES is False
        ag = object.__new__(cls)
        with pytest.raises(ValueError, match=f'{name}.*no next_action'):
            ag._load_batch(iter([five]))
        with pytest.raises(NotImplementedError):
            ag.evaluate(iter([five]))
    assert agents.TD3BCAgent._EVALUATES is True and agents.CRRAgent._EVALUATES is True and agents.TD3BCAgent.METRIC_WINDOW is True
    assert issubclass(ReBRACAgent, agents._NextActionBatch) and '_load_batch' not in vars(ReBRACAgent) and '_load_batch' not in vars(onestep.OneStepCRRAgent)
    assert ReBRACAgent.KIND == 'td3_bc' and ReBRACAgent._EVALUATES is False and [s for s, _ in ReBRACAgent.METRICS[6:]] == [10, 11]
    with pytest.raises(ValueError, match='ReBRACAgent.*no next_action'):
        object.__new__(ReBRACAgent)._load_batch(iter([five]))
    with pytest.raises(AttributeError):
        agents.NoSuchAgent
    # the drivers: FQE keeps its nstep = 1 refusal, behaviour Q has none and asks for shapes when there is no policy to take them from
    it3 = type('It', (), {'nstep': 3, 'batch_size': 8})()
    with pytest.raises(ValueError, match='nstep=3'):
        fqe.fitted_q_evaluation(None, it3, 1)
    with pytest.raises(ValueError, match='obs_shape and action_shape'):
        fqe.behavior_q_evaluation(it3, 1)
    assert list(inspect.signature(fqe.behavior_q_evaluation).parameters)[:3] == ['replay_iter', 'num_grad_steps', 'policy']
    assert inspect.signature(fqe.behavior_q_evaluation).parameters['policy'].kind is inspect.Parameter.KEYWORD_ONLY


def test_value_keys_follow_fqe_values_arithmetic():
    from exorl_amd import _lib as L
    from exorl_amd.agents import FQEAgent, fqe_values
    from exorl_amd.fqe import BehaviorQAgent
    sums = np.zeros(L.N_FQE_VALUE)
    sums[[L.FQE_V_Q1, L.FQE_V_Q2, L.FQE_V_MEAN_SQ, L.FQE_V_DIFF_SQ]] = 6.0, 2.0, 5.0, 8.0
    seen = {}

    def base_value(self, replay_iter, gather=None):
        seen['args'] = (replay_iter, gather)
        return fqe_values(sums, 4, 10.0, 4)
    real, FQEAgent.value = FQEAgent.value, base_value
    try:
        v = BehaviorQAgent.value(object.__new__(BehaviorQAgent), 'it')
    finally:
        FQEAgent.value = real
    assert seen['args'] == ('it', None)
    assert list(v) == ['behavior_q', 'behavior_q_q1', 'behavior_q_q2', 'behavior_q_stderr', 'behavior_q_twin_rms', 'behavior_value', 'episodes']
    assert (v['behavior_q'], v['behavior_q_q1'], v['behavior_q_q2'], v['behavior_value'], v['episodes']) == (1.0, 1.5, 0.5, 2.5, 4)
    assert v['behavior_q_twin_rms'] == np.sqrt(2.0) and abs(v['behavior_q_stderr'] - np.sqrt((5.0 - 4.0) / 3 / 4)) < 1e-15


# ---- the float64 twin on hand-computed rows --------------------------------------------------------------------------------------------------
def _lin_params(O, A, H):
    """Seeded parameters in the reference's order (oracle.agents.param_shapes), as the GPU cases build theirs."""
    import _synth
    from oracle.agents import param_shapes
    ash, csh = param_shapes('td3_bc', O, A, H)
    return [np.asarray(v, np.float64) for v in _synth.synth_params(ash, 11).values()], [np.asarray(v, np.float64) for v in _synth.synth_params(csh, 12).values()]


def test_twin64_takes_the_datasets_action_exactly_where_valid():
    """Three rows, v = (1, 0, 1). The twin's critic target, recomputed by hand from its own nets: rows 0 and 2 at the dataset's a', row 1 at
    the base step's clipped sample; with v = 0 everywhere the step is oracle.twin64.Twin's to the last bit, with v = 1 everywhere the
    critic's gradients do not depend on the actor; the FQE twin likewise, each net on its own target."""
    import _sarsa_twin as S
    from _fqe_twin import FQETwin
    from oracle.twin64 import Twin
    O, A, H, B = 4, 2, 8, 3
    rs = np.random.RandomState(0)
    pa, pc = _lin_params(O, A, H)
    pa2 = [p + 0.05 for p in pa]
    b5 = tuple(rs.uniform(-1, 1, s) for s in ((B, O), (B, A), (B, 1), (B, 1), (B, O)))
    a_next = rs.uniform(-1, 1, (B, A))
    z = [rs.standard_normal((B, A)), rs.standard_normal((B, A))]
    valid = np.array([1.0, 0.0, 1.0])
    for kind in ('td3_bc', 'td3'):
        tw = S.SarsaTwin(kind, pa, pc)
        with torch.no_grad():           # by hand, before the step moves anything
            t = lambda x: torch.as_tensor(x, dtype=torch.float64)
            mu = torch.tanh(tw._actor_raw(tw.actor, t(b5[4])))
            sample = Twin._sample(tw, mu, t(z[0]), None, 'target')
            fed = sample.clone()
            fed[0], fed[2] = t(a_next[0]), t(a_next[2])
            tq1, tq2 = tw._critic(tw.critic_target, t(b5[4]), fed)
            y = t(b5[2]) + t(b5[3]) * torch.min(tq1, tq2)
            q1, q2 = tw._critic(tw.critic, t(b5[0]), t(b5[1]))
            loss = ((q1 - y) ** 2).mean() + ((q2 - y) ** 2).mean()
        r = tw.update(b5 + (a_next, valid), 0, *z)
        assert abs(r.metrics['critic_target_q'] - y.mean().item()) <= 1e-15 and abs(r.metrics['critic_loss'] - loss.item()) <= 1e-14
        assert r.metrics['next_valid'] == 2.0 / 3.0
        # v = 0 everywhere: the base twin, bit for bit
        r0 = S.SarsaTwin(kind, pa, pc).update(b5 + (a_next, np.zeros(B)), 0, *z)
        rb = Twin(kind, pa, pc).update(b5, 0, *z)
        assert all(np.array_equal(g, h) for g, h in zip(r0.critic_grads, rb.critic_grads)) and all(np.array_equal(g, h) for g, h in zip(r0.actor_grads, rb.actor_grads))
        assert {k: v for k, v in r0.metrics.items() if k != 'next_valid'} == rb.metrics and r0.metrics['next_valid'] == 0.0
        # v = 1 everywhere (absent): the critic step does not see the actor; with v = 0 on a row it does
        g1 = S.SarsaTwin(kind, pa, pc).update(b5 + (a_next,), 0, *z).critic_grads
        g2 = S.SarsaTwin(kind, pa2, pc).update(b5 + (a_next,), 0, *z).critic_grads
        assert all(np.array_equal(g, h) for g, h in zip(g1, g2))
        g3 = S.SarsaTwin(kind, pa2, pc).update(b5 + (a_next, valid), 0, *z).critic_grads
        assert not all(np.array_equal(g, h) for g, h in zip(r.critic_grads, g3))
    ft = S.SarsaFQETwin(pa, pc)
    with torch.no_grad():
        t = ft._t
        fed = ft.mu(t(b5[4])).clone()
        fed[0], fed[2] = t(a_next[0]), t(a_next[2])
        t1, t2 = ft._critic(ft.critic_target, torch.cat([t(b5[4]), fed], -1))
        y = 0.5 * ((t(b5[2]) + t(b5[3]) * t1) + (t(b5[2]) + t(b5[3]) * t2))
    r = ft.update(b5 + (a_next, valid))
    assert abs(r.metrics['critic_target_q'] - y.mean().item()) <= 1e-15 and r.metrics['next_valid'] == 2.0 / 3.0
    r0, rb = S.SarsaFQETwin(pa, pc).update(b5 + (a_next, np.zeros(B))), FQETwin(pa, pc).update(b5)
    assert all(np.array_equal(g, h) for g, h in zip(r0.critic_grads, rb.critic_grads))
    g1, g2 = S.SarsaFQETwin(pa, pc).update(b5 + (a_next,)).critic_grads, S.SarsaFQETwin(pa2, pc).update(b5 + (a_next,)).critic_grads
    assert all(np.array_equal(g, h) for g, h in zip(g1, g2))
    q1, q2 = ft.q_rows(b5[0], b5[1])
    assert q1.shape == q2.shape == (B,)


def test_the_cases_are_rebracs_and_qualify():
    """The tables are tests/_rebrac_twin.py's objects; the small cases qualify on this twin too (same decisions in float32 and float64 with
    margins >= MARGIN on the rows that use them, near-kink sets within the cap)."""
    import _rebrac_twin as R
    import _sarsa_twin as S
    assert S.CASES is R.CASES and S.TRAJ_CASES is R.TRAJ_CASES and S.TRAJ_STEPS == 3
    for c in S.CASES:
        if c.B <= 257:
            assert S.qualify(c) == [], (S.case_id(c), S.qualify(c))
