"""Windowed metrics (agent.enable_metric_window / pop_metrics): the step's metrics are formed on the device — on the fused scalar-head path
for TD3+BC, TD3 and DDPG — and accumulated there; the host reads the window once per logging interval.
  1  step-0 metrics of the window path and of the use_tb=True path against the float64 twin (oracle/twin64.py), on the cases of
     tests/_grad_grid.py at which the new kernels can go wrong
  2  the same steps on poisoned scratch and a window buffer of 0xFF bytes: bit-identical
  3  the update itself is unchanged: parameters equal to the use_tb=False agent's (fused kinds), the use_tb=True agent's (the others)
  4  window semantics through the captured graph   5  a moving stddev schedule   6  the reference's recorded trajectories   7  refusals"""
import numpy as np
import pytest
import torch

import _grad_grid as G
import _synth

pytestmark = pytest.mark.gpu

# (kind, O, A, H, B, precision) of the _grad_grid cases used here, and what each one exercises in the new code
WINDOW_CASES = [
    (('td3', 4, 2, 4, 1, 'fp32'), 'one lane, one row'),
    (('td3_bc', 5, 1, 100, 7, 'fp32'), 'head_bwd<1>, no fused sampling, ragged last chunk of 3, H/4 = 25 lanes'),
    (('td3_bc', 24, 8, 32, 50, 'fp32'), 'ragged chunk of 2, last width of head_bwd<8>'),
    (('ddpg', 24, 9, 192, 72, 'fp32'), 'head_bwd<16>, shared trunk, actor_logprob'),
    (('td3', 19, 16, 1024, 64, 'fp32'), 'all 256 lanes'),
    (('td3', 6, 2, 32, 8200, 'fp32'), '2050 chunks: the sub-sum-of-32 path'),
    (('td3_bc', 24, 6, 320, 1000, 'fp32'), '250 chunks'),
    (('td3_bc', 24, 6, 128, 64, 'bf16x3'), 'plane route: folded target heads'),
    (('td3', 17, 6, 128, 128, 'bf16x3'), 'plane route: folded target heads'),
    (('ddpg', 24, 9, 256, 64, 'bf16x3'), 'plane route: folded target heads, shared trunk'),
    (('td3_bc', 5, 1, 100, 7, 'bf16x3'), 'in-GEMM split'),
    (('td3_bc', 24, 6, 256, 1024, 'bf16'), 'plain bf16: held at 3e-2'),
]


def _case(key):
    found = [c for c in G.CASES if (c.kind, c.O, c.A, c.H, c.B, c.precision) == key]
    assert len(found) == 1, key
    return found[0]


CASE_PARAMS = [pytest.param(_case(k), id=G.case_id(_case(k))) for k, _ in WINDOW_CASES]


def make(kind, O, A, H, B, use_tb, precision='fp32', stddev=0.2):
    from exorl_amd import agents
    if kind == 'td3_bc':
        return agents.TD3BCAgent('td3_bc', (O,), (A,), 'cuda', 1e-4, H, 0.01, stddev, 1, B, 0.3, use_tb, 2.5, precision=precision)
    if kind == 'td3':
        return agents.TD3Agent('td3', (O,), (A,), 'cuda', 1e-4, H, 0.01, stddev, 1, B, 0.3, use_tb, precision=precision)
    if kind == 'crr':
        return agents.CRRAgent('crr', (O,), (A,), 'cuda', 1e-4, H, 0.01, 10, 'indicator', stddev, 1, B, 0.3, use_tb, precision=precision)
    if kind == 'cql':
        return agents.CQLAgent('cql', (O,), (A,), 'cuda', 1e-4, H, 0.01, 1, B, use_tb, 0.01, 3, 5.0, False, precision=precision)
    if kind == 'bc':
        return agents.BCAgent('bc', (O,), (A,), 'cuda', 1e-4, H, B, stddev, use_tb, precision=precision)
    return agents.DDPGAgent('ddpg', True, 'states', (O,), (A,), 'cuda', 1e-4, 50, H, 0.01, 2000, 2, stddev, 3, B, 0.3, True, use_tb, False,
                            precision=precision)


def nets_of(ag):
    return [('actor', ag.actor)] + ([('critic', ag.critic), ('critic_target', ag.critic_target)] if hasattr(ag, 'critic') else [])


def params_of(ag):
    return {f'{n}.{i}': p.detach().clone() for n, net in nets_of(ag) for i, p in enumerate(net.parameters())}


def named(ag, raw):
    """The raw metric block as the dict update() returns with use_tb=True."""
    from exorl_amd import _lib as L
    m = {name: float(raw[slot]) for slot, name in ag.METRICS}
    m.setdefault('actor_ent', float(raw[L.M_ACTOR_ENT]))
    return m


def _arena(seed, B=64):
    from exorl_amd.engine import ReplayEngine
    from exorl_amd.replay_buffer import ArenaIterator
    O, A = 24, 6
    eng = ReplayEngine((O,), np.float32, A, 0, 4096, 64)
    eng.set_order([eng.append_episode(ep) for ep in _synth.synth_episodes(seed, [200, 300, 250], O, A)])
    eng.seed_philox(77)
    return eng, ArenaIterator(eng, B, 1, 0.99, 'philox')


# ---- 1, 2: one step of a grid case -------------------------------------------------------------------------------------------------
def run_case(c, window, poison=False):
    """One update() from the case's seeded parameters, batch and recorded noise. window: use_tb=False with the metric window (the fused
    path); else use_tb=True (today's metrics path). poison: scratch filled with NaN patterns, the window buffer with 0xFF bytes.
    Returns (agent, the step's metrics by name)."""
    torch.manual_seed(0)
    ag = make(c.kind, c.O, c.A, c.H, c.B, not window, c.precision)
    _, _, pa, pc = G.params(c)
    ag.actor.load_state_dict({k: torch.from_numpy(v) for k, v in pa.items()})
    ag.critic.load_state_dict({k: torch.from_numpy(v) for k, v in pc.items()})
    ag.critic_target.load_state_dict(ag.critic.state_dict())
    blocks = iter(G.noise(c))
    ag.noise_hook = lambda shape: next(blocks)
    if window:
        assert ag.enable_metric_window() is True
    if poison:
        ag.engine.poison_scratch()
        if window:
            buf = torch.full((ag.engine.metric_window_bytes(),), 0xFF, dtype=torch.uint8, device='cuda')
            ag.engine.set_metric_window(buf)
    m = ag.update(iter([G.batch(c)]), 0)
    if window:
        assert m == {}
        raw = ag.engine.metrics_raw()
        m = named(ag, raw)
        pop = ag.pop_metrics()
        assert pop.pop('metric_steps') == 1 and pop == m, (pop, m)        # a window of one step holds that step's fp32 values exactly
        assert ag.pop_metrics() == {}
    torch.cuda.synchronize()
    return ag, m


@pytest.mark.parametrize('c', CASE_PARAMS)
def test_step0_metrics_vs_twin64(c):
    """e(x) = |x - m64| / S per metric, S = max |m64| over the case's metrics; m64 from the float64 twin taking its actor step from the
    critic the run produced. Bars (the project's gradient bar, tests/test_gpu_grad_grid.py):
      fp32     e(window) <= 8 max(e(metrics path), 2^-23)
      bf16x3   e(window) <= 8 e(metrics path) + 4 * 2^-16
      bf16     e(window) <= 3e-2, the project's plain-bf16 bar"""
    runs = {}
    for mode in ('window', 'metrics'):
        ag, m = run_case(c, mode == 'window')
        after = [p.cpu().numpy() for p in ag.critic.parameters()]
        same = 'window' in runs and all(np.array_equal(a, b) for a, b in zip(after, runs['window'][2]))
        m64 = runs['window'][1] if same else G.run_twin(c, torch.float64, critic_after=after).metrics
        runs[mode] = (m, m64, after)
    (mw, w64, _), (mm, m64, _) = runs['window'], runs['metrics']
    assert sorted(mw) == sorted(mm) == sorted(m64), (sorted(mw), sorted(mm), sorted(m64))
    worst, lines = 0.0, []
    for k in sorted(m64):
        ew = abs(mw[k] - w64[k]) / max(abs(v) for v in w64.values())
        em = abs(mm[k] - m64[k]) / max(abs(v) for v in m64.values())
        bar = {'fp32': 8.0 * max(em, 2.0 ** -23), 'bf16x3': 8.0 * em + 4.0 * 2.0 ** -16, 'bf16': 3e-2}[c.precision]
        worst = max(worst, ew / bar)
        lines.append(f'[metric window] {G.case_id(c):34s} {k:16s} e(window) {ew:.2e}  e(metrics path) {em:.2e}  bar {bar:.2e}  e(window)/bar {ew / bar:.3f}')
    print('\n'.join(lines))
    assert worst <= 1.0, f'{G.case_id(c)}: e(window) is {worst:.2f} x its bar\n' + '\n'.join(lines)


@pytest.mark.parametrize('c', CASE_PARAMS)
def test_poisoned_scratch_and_window_buffer(c):
    """The window step again on NaN-poisoned scratch and a window buffer of 0xFF bytes: metrics and parameters bit-identical."""
    clean, m0 = run_case(c, True)
    dirty, m1 = run_case(c, True, poison=True)
    assert m0 == m1, (m0, m1)                                   # a NaN compares unequal to itself: this also rules them out
    p0, p1 = params_of(clean), params_of(dirty)
    for k in p0:
        assert torch.equal(p0[k], p1[k]), f'{G.case_id(c)}: {k} differs after the poisoned step'
    assert np.array_equal(clean.engine.metrics_raw(), dirty.engine.metrics_raw())


# ---- 3: the update itself is unchanged ----------------------------------------------------------------------------------------------
def _three_steps(kind, precision, use_tb, window, graph):
    torch.manual_seed(3)
    ag = make(kind, 24, 6, 256, 64, use_tb, precision)
    e, it = _arena(9)
    if window:
        assert ag.enable_metric_window() is True
    if graph:
        assert ag.enable_graph(it)
    for s in ([0, 2, 4] if kind == 'ddpg' else [0, 1, 2]):
        assert (ag.update(it, s) == {}) == (window or not use_tb)
    torch.cuda.synchronize()
    return ag, (e, it)


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3', 'bf16x6'])
@pytest.mark.parametrize('kind', ['td3_bc', 'td3', 'ddpg'])
def test_window_leaves_the_fused_update_unchanged(kind, precision):
    """Three steps at H=256, B=64 (the set-up of test_no_metrics_fast_path_matches_metrics_path): every parameter in window mode equals
    the use_tb=False agent's, eager and through the captured graph."""
    ref, _k0 = _three_steps(kind, precision, False, False, False)
    want = params_of(ref)
    for graph in (False, True):
        ag, _k = _three_steps(kind, precision, False, True, graph)
        got = params_of(ag)
        for k in want:
            assert torch.equal(got[k], want[k]), (kind, precision, 'graph' if graph else 'eager', k)
        assert ag.pop_metrics()['metric_steps'] == 3


@pytest.mark.parametrize('kind', ['td3_bc', 'ddpg'])
def test_window_on_an_agent_built_with_use_tb(kind):
    """An agent built with use_tb=True that enables the window: update() returns {} and the step is the fused one, parameters equal to the
    use_tb=False agent's, eager and through the captured graph."""
    ref, _k0 = _three_steps(kind, 'fp32', False, False, False)
    want = params_of(ref)
    for graph in (False, True):
        ag, _k = _three_steps(kind, 'fp32', True, True, graph)         # _three_steps asserts update() == {}
        got = params_of(ag)
        for k in want:
            assert torch.equal(got[k], want[k]), (kind, 'graph' if graph else 'eager', k)
        assert ag.pop_metrics()['metric_steps'] == 3


@pytest.mark.parametrize('kind', ['bc', 'crr', 'cql'])
def test_window_leaves_the_metrics_path_update_unchanged(kind):
    """The kinds off the fused path run the kernels use_tb=True runs: parameters equal to the use_tb=True agent's."""
    ref, _k0 = _three_steps(kind, 'fp32', True, False, False)
    want = params_of(ref)
    for graph in (False, True):
        ag, _k = _three_steps(kind, 'fp32', False, True, graph)
        got = params_of(ag)
        for k in want:
            assert torch.equal(got[k], want[k]), (kind, 'graph' if graph else 'eager', k)
        pop = ag.pop_metrics()
        assert pop['metric_steps'] == 3 and sorted(pop) == sorted([n for _, n in ag.METRICS] + ['metric_steps'] + ([] if kind == 'cql' else ['actor_ent']))


# ---- 4: window semantics through the graph -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['td3_bc', 'ddpg', 'crr'])
def test_window_through_the_captured_graph(kind):
    """Twin agents on twin arenas, both in window mode: one steps eagerly and reads every step's metric block, the other replays the
    captured graph and reads the window once. Sums of twelve fp32 numbers are exact in double, so the means agree to rounding of the
    division."""
    twins = []
    for graph in (False, True):
        torch.manual_seed(3)
        ag = make(kind, 24, 6, 128, 64, False)
        e, it = _arena(9)
        assert ag.enable_metric_window() is True
        if graph:
            assert ag.enable_graph(it)
        twins.append((ag, e, it))
    (eager, _, it_e), (fast, _, it_g) = twins
    step = 0
    for n in (12, 5):
        rows = []
        for _ in range(n):
            assert eager.update(it_e, step) == {} and fast.update(it_g, step) == {}
            rows.append(named(eager, eager.engine.metrics_raw()))
            step += 2 if kind == 'ddpg' else 1
        pop = fast.pop_metrics()
        assert pop.pop('metric_steps') == n
        assert sorted(pop) == sorted(rows[0])
        for k in pop:
            want = float(np.mean(np.array([r[k] for r in rows], np.float64)))
            assert abs(pop[k] - want) <= 1e-12 * abs(want), (kind, n, k, pop[k], want)
        assert fast.pop_metrics() == {}
        assert eager.pop_metrics()['metric_steps'] == n         # the eager twin's window saw the same steps


# ---- 5: a moving schedule -------------------------------------------------------------------------------------------------------------
def test_window_averages_a_moving_stddev_schedule():
    """actor_ent is formed from the device-resident std of each step: over ten graph replays of linear(1.0,0.1,20) the window's mean is the
    mean of the ten host-formula entropies (fp32 log on the device against numpy's)."""
    from exorl_amd import utils
    sched, A = 'linear(1.0,0.1,20)', 6
    torch.manual_seed(3)
    ag = make('td3_bc', 24, A, 128, 64, False, stddev=sched)
    e, it = _arena(9)
    assert ag.enable_metric_window() is True
    assert ag.enable_graph(it)
    for s in range(10):
        assert ag.update(it, s) == {}
    assert ag.engine.graph_captures == 1
    want = np.mean([float(np.float32(0.5 + 0.5 * np.log(2 * np.pi) + np.log(utils.schedule(sched, s))) * A) for s in range(10)])
    pop = ag.pop_metrics()
    assert pop['metric_steps'] == 10
    assert abs(pop['actor_ent'] - want) <= 1e-6 * abs(want), (pop['actor_ent'], want)


# ---- 6: reference trajectories --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['td3_bc', 'td3', 'ddpg'])
def test_window_tiny_trajectory_vs_reference(gold, kind):
    """Five steps of the reference's recorded run (tests/golden/tiny_*.npz) in window mode, fp32: every step's metric block at the
    tolerances test_tiny_trajectory_vs_reference applies to the metrics path, and the window against the mean of the five rows."""
    z = np.load(gold / f'tiny_{kind}.npz')
    torch.manual_seed(21)
    ag = make(kind, 5, 3, 32, 8, False)
    for nm, net in nets_of(ag):
        net.load_state_dict({k: torch.from_numpy(z[f'init/{nm}/{k}']) for k in net.state_dict()})
    noise = iter([z[f'noise/{i}'] for i in range(len([k for k in z.files if k.startswith('noise/')]))])
    ag.noise_hook = lambda shape: next(noise)
    assert ag.enable_metric_window() is True
    keys = [str(k) for k in z['metric_keys']]
    for i in range(5):
        batch = tuple(z[f'batch/{i}/{j}'] for j in range(5))
        assert ag.update(iter([batch]), 2 * i if kind == 'ddpg' else i) == {}
        m = named(ag, ag.engine.metrics_raw())
        assert sorted(m) == keys
        np.testing.assert_allclose(np.array([m[k] for k in keys]), z['metrics'][i], rtol=1e-4, atol=2e-6, err_msg=f'{kind} step {i} {keys}')
    pop = ag.pop_metrics()
    assert pop.pop('metric_steps') == 5 and sorted(pop) == keys
    np.testing.assert_allclose(np.array([pop[k] for k in keys]), np.asarray(z['metrics'][:5], np.float64).mean(0), rtol=1e-4, atol=2e-6,
                               err_msg=f'{kind} window {keys}')


# ---- 7: refusals ------------------------------------------------------------------------------------------------------------------------
def test_window_refusals(gold):
    from exorl_amd import _lib as L
    from exorl_amd import agents
    from exorl_amd.engine import AgentEngine
    ag = make('td3_bc', 24, 6, 128, 64, False)
    e, it = _arena(9)
    assert ag.enable_graph(it)
    with pytest.raises(RuntimeError, match='before enable_graph'):
        ag.enable_metric_window()
    with pytest.raises(L.ExorlError, match='captured graph'):
        ag.engine.set_metric_window()
    assert ag.update(it, 0) == {}                               # nothing changed: still the plain use_tb=False step
    with pytest.raises(RuntimeError, match='enable_metric_window'):
        ag.pop_metrics()
    C_, HW, A, F, H, B, _ = [int(v) for v in np.load(gold / 'pixel_ddpg.npz')['dims']]
    pix = agents.DDPGAgent('ddpg', True, 'pixels', (C_, HW, HW), (A,), 'cuda', 1e-4, F, H, 0.01, 2000, 2, 0.2, 3, B, 0.3, True, True, False)
    assert pix.enable_metric_window() is False
    rnd = agents.RNDAgent(rnd_rep_dim=16, update_encoder=True, rnd_scale=1.0, name='rnd', reward_free=True, obs_type='states', obs_shape=(24,),
                          action_shape=(6,), device='cuda', lr=1e-4, feature_dim=50, hidden_dim=64, critic_target_tau=0.01, num_expl_steps=2000,
                          update_every_steps=2, stddev_schedule=0.2, nstep=3, batch_size=16, stddev_clip=0.3, init_critic=True, use_tb=True,
                          use_wandb=False)
    assert rnd.enable_metric_window() is False
    eng = AgentEngine('td3_bc', 24, 6, 64, 16, world_size=2)
    with pytest.raises(L.ExorlError, match='world_size=2'):
        eng.set_metric_window()
    import pickle
    win = make('td3_bc', 24, 6, 64, 16, True)
    assert win.enable_metric_window() is True
    back = pickle.loads(pickle.dumps(win))
    with pytest.raises(RuntimeError, match='enable_metric_window'):
        back.pop_metrics()


def test_window_attach_read_reset_detach():
    """The metric window through its whole life at batch 259, and the buffers exorl_agent_set_metric_window refuses (tests/_windows.py)."""
    import _windows as W
    eng = W.engine('td3_bc')
    W.check_window(eng, 'metric_window', lambda: eng.update(0.2), 1, 'no metric window')
