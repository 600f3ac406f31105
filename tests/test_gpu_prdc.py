"""PRDCAgent on the GPU: one step of every case of tests/_prdc_cases.py against the float64 twin at the bars of tests/test_gpu_iql.py
(neighbours equal for every row), the step against TD3BCAgent bit for bit when every row's neighbour is the row itself, a five-step
trajectory, graph = eager and poisoned scratch bit for bit, rebinding, pickling and snapshots, train_offline through the normaliser,
and the refusals."""
import ctypes
import pickle

import numpy as np
import pytest
import torch

import _grad_grid as G
import _prdc_cases as P
import _synth

pytestmark = pytest.mark.gpu

NETS = ('actor', 'critic', 'critic_target')


def state_of(ag, metrics=True):
    out = {}
    for nm in NETS:
        net = getattr(ag, nm)
        for i, p in enumerate(net.parameters()):
            out[f'{nm}.param{i}'] = p.detach().clone()
        if nm != 'critic_target':
            for i, g in enumerate(net.grads()):
                out[f'{nm}.grad{i}'] = g.detach().clone()
    for nm, net in (('actor', L().NET_ACTOR), ('critic', L().NET_CRITIC)):
        for w, tag in ((L().T_ADAM_M, 'm'), (L().T_ADAM_V, 'v')):
            out[f'{nm}.adam_{tag}'] = ag.engine.flat(net, w).detach().clone()
    if metrics:
        out['metrics'] = torch.from_numpy(ag.engine.metrics_raw())
    return out


def L():
    from exorl_amd import _lib
    return _lib


def assert_same_bits(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        assert not bool(torch.isnan(b[k]).any()), f'{tag}: NaN in {k}'
        assert torch.equal(a[k], b[k]), f'{tag}: {k} differs (max |d| = {float((a[k] - b[k]).abs().max()):.3e})'


def hooked(ag, blocks):
    it = iter(blocks)
    ag.noise_hook = lambda shape: next(it)
    return ag


# ---- one step against the float64 twin ------------------------------------------------------------------------------------------------
def run(c, route, poison=False):
    torch.manual_seed(0)
    ag = P.load_params(P.make_agent(c, route != 'fast'), c)
    keep = P.bind(ag, c)
    hooked(ag, P.noise(c))
    if poison:
        ag.engine.poison_scratch()
    m = ag.update(iter([P.batch(c)]), 0)
    torch.cuda.synchronize()
    return ag, m, keep


@pytest.mark.parametrize('route', ['metrics', 'fast'])
@pytest.mark.parametrize('c', [pytest.param(c, id=P.case_id(c)) for c in P.CASES])
def test_gradients_vs_twin64(c, route):
    """tests/test_gpu_iql.py's bars per gradient tensor, e(x) = max|x - g64| / max|g64| after the ReLU flips the near-kink set allows:
    fp32 e(gpu) <= 8 max(e(twin32), 2^-23); bf16x3 8 e(twin32) + 4 * 2^-16; bf16x6 8 max(e(twin32), 2^-23) + 4 * 3 * 2^-24; plain bf16
    cosine >= 0.999. Metrics (nn_dist among them): fp32 / bf16x6 2e-5 relative + 1e-6, bf16x3 1e-4, bf16 3e-2. Both twins take their
    actor step from the critic this run's optimiser step produced (tests/test_gpu_grad_grid.py). The engine's neighbour equals the
    twin's for every row. The same step on NaN-filled scratch: same bits."""
    ag, m, keep = run(c, route)
    after = [p.cpu().numpy() for p in ag.critic.parameters()]
    r64 = P.run_twin(c, torch.float64, None if c.bar == 'coarse' else P.KINK_DELTA[c.precision], critic_after=after)
    r32 = P.run_twin(c, torch.float32, critic_after=after)
    tag = f'{P.case_id(c)} {route}'
    prec = c.precision
    idx, d2, a_nn, splits = ag.engine.nn_result()
    assert np.array_equal(idx.cpu().numpy(), r64.nn_idx.astype(np.int32)), (tag, np.flatnonzero(idx.cpu().numpy() != r64.nn_idx)[:8])
    assert np.array_equal(a_nn.cpu().numpy(), P.table(c)[r64.nn_idx, c.O:c.O + c.A])
    rel = {'fp32': 2e-5, 'bf16x6': 2e-5, 'bf16x3': 1e-4, 'bf16': 3e-2}[prec]
    worst_m = 0.0
    if route == 'metrics':
        assert sorted(m) == sorted(r64.metrics), (sorted(m), sorted(r64.metrics))
        worst_m = max(abs(m[k] - v) / (abs(v) + 1e-6 / rel) for k, v in r64.metrics.items())
    else:
        assert m == {}
    ratio_w = e_gpu_w = e_32_w = 0.0
    cos_w, worst_at, flips = 1.0, '', 0
    floor = G.KINK_FLOOR['bf16x3' if prec == 'bf16x3' else 'fp32']
    for step, want in P.steps_of(r64):
        got = [g.cpu().numpy().reshape(w.shape) for g, w in zip(getattr(ag, step).grads(), want)]
        assert len(got) == len(want) and all(np.all(np.isfinite(g)) for g in got), f'{tag}: {step} gradients'
        if c.bar == 'coarse':
            for i, (g, w) in enumerate(zip(got, want)):
                cos = G.tensor_cosines([g], [w])[0]
                cos_w = min(cos_w, cos)
                e_gpu_w = max(e_gpu_w, float(np.abs(g - w).max() / np.abs(w).max()))
                assert cos >= 0.999, (tag, step, i, cos)
            continue
        kinks = r64.kinks[step]
        assert kinks is not None, f'{tag}: |K| = {r64.n_kinks[step]} exceeds the cap of a tight case'
        d_gpu, f_gpu = G.explain_kinks(got, want, kinks, floor, f'{tag} {step} gpu')
        d_32, _ = G.explain_kinks(getattr(r32, f'{step}_grads'), want, kinks, floor, f'{tag} {step} twin32')
        flips += f_gpu
        for i, (eg, e3) in enumerate(zip(G.tensor_errors(d_gpu, want), G.tensor_errors(d_32, want))):
            bar = {'fp32': 8.0 * max(e3, 2.0 ** -23), 'bf16x6': 8.0 * max(e3, 2.0 ** -23) + 12.0 * 2.0 ** -24, 'bf16x3': 8.0 * e3 + 4.0 * 2.0 ** -16}[prec]
            if eg / bar > ratio_w:
                ratio_w, worst_at = eg / bar, f'{step}[{i}]'
            e_gpu_w, e_32_w = max(e_gpu_w, eg), max(e_32_w, e3)
    K = ' '.join(f'|K_{s}|={n}' for s, n in r64.n_kinks.items())
    if c.bar == 'coarse':
        print(f'[prdc grid] {tag}: coarse e(gpu) {e_gpu_w:.2e} worst cosine {cos_w:.6f} (bar 0.999); worst metric error {worst_m:.2e} (bar {rel:g}); '
              f'{splits} key ranges')
    else:
        print(f'[prdc grid] {tag}: tight e(gpu) {e_gpu_w:.2e} e(twin32) {e_32_w:.2e} worst e(gpu)/bar {ratio_w:.3f} at {worst_at or "-"} {K} '
              f'flips gpu {flips}; worst metric error {worst_m:.2e} (bar {rel:g}); {splits} key ranges')
    if route == 'metrics':
        for k, v in r64.metrics.items():
            assert abs(m[k] - v) <= rel * abs(v) + 1e-6 * (3e4 if prec == 'bf16' else 1), (tag, k, m[k], v)
    assert ratio_w <= 1.0, f'{tag}: e(gpu) is {ratio_w:.2f} x its bar at {worst_at} (e(gpu) {e_gpu_w:.2e}, e(twin32) {e_32_w:.2e})'
    dirty, m1, keep1 = run(c, route, poison=True)
    assert_same_bits(state_of(ag), state_of(dirty), f'{tag} poisoned')
    assert m == m1


# ---- TD3+BC, bit for bit ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('use_tb', [True, False])
@pytest.mark.parametrize('precision,H,B', [('fp32', 100, 7), ('bf16x3', 128, 64), ('fp32', 64, 200)])
def test_step_is_td3bcs_when_every_neighbour_is_the_row_itself(use_tb, precision, H, B):
    """The table is built from one episode whose B transitions are the batch itself, distinct states, beta = 1e3: another row is at least
    1e6 |s - s'|^2 away, the row itself at |mu - a|^2 <= 4 A. idx is then 0 .. B - 1 and a_nn the batch's action, so one update() leaves
    parameters, gradients, Adam moments, target, counters and the common metrics with TD3BCAgent's bytes."""
    from exorl_amd import agents
    O, A = 24, 6
    b = _synth.synth_batch(7, 0, B, O, A)
    ep = dict(observation=np.concatenate([b[0], b[0][:1]]), action=np.concatenate([b[1][:1], b[1]]),
              reward=np.zeros((B + 1, 1), np.float32), discount=np.ones((B + 1, 1), np.float32))
    ns = _synth.NoiseStream(4)
    blocks = [ns.draw((B, A)), ns.draw((B, A))]
    torch.manual_seed(1)
    pr = agents.PRDCAgent('prdc', (O,), (A,), 'cuda', 1e-4, H, 0.01, 0.2, 1, B, 0.3, use_tb, 2.5, beta=1e3, precision=precision)
    td = agents.TD3BCAgent('td3_bc', (O,), (A,), 'cuda', 1e-4, H, 0.01, 0.2, 1, B, 0.3, use_tb, 2.5, precision=precision)
    for nm in ('actor', 'critic', 'critic_target'):
        getattr(td, nm).load_state_dict(getattr(pr, nm).state_dict())
    keep = P.arena_of([ep], O, A)
    assert pr.bind_dataset(keep[1]) == B == pr.nn_table_rows
    mp = hooked(pr, blocks).update(iter([b]), 0)
    mt = hooked(td, blocks).update(iter([b]), 0)
    torch.cuda.synchronize()
    idx, d2, a_nn, _ = pr.engine.nn_result()
    assert idx.cpu().tolist() == list(range(B))
    assert torch.equal(a_nn.cpu(), torch.from_numpy(b[1]))
    assert_same_bits(state_of(td, metrics=False), state_of(pr, metrics=False), f'{precision} use_tb={use_tb}')
    assert pr.engine.opt_steps() == td.engine.opt_steps() == (1, 1) and pr.engine.noise_counter() == td.engine.noise_counter()
    assert {k: v for k, v in mp.items() if k != 'nn_dist'} == mt
    if use_tb:
        raw_p, raw_t = pr.engine.metrics_raw(), td.engine.metrics_raw()
        assert raw_p[:10].tobytes() == raw_t[:10].tobytes()
        mu_a = np.sqrt(d2.cpu().numpy().astype(np.float64)).mean()
        assert abs(mp['nn_dist'] - mu_a) <= 2e-6 * mu_a


# ---- five steps ----------------------------------------------------------------------------------------------------------------------
def test_five_steps_vs_twin64():
    c = P.TRAJ
    ag = P.load_params(P.make_agent(c), c)
    keep = P.bind(ag, c)
    tw = P.make_twin(c, torch.float64)
    ns = _synth.NoiseStream(c.seed + 3)
    for step in range(5):
        b = _synth.synth_batch(c.seed + 2, step, c.B, c.O, c.A)
        z = [ns.draw((c.B, c.A)), ns.draw((c.B, c.A))]
        m = hooked(ag, z).update(iter([b]), step)
        r = tw.update(b, step, *z)
        assert ag.engine.nn_result()[0].cpu().tolist() == r.nn_idx.tolist(), step
        assert sorted(m) == sorted(r.metrics)
        for k, v in r.metrics.items():
            assert abs(m[k] - v) <= 2e-5 * abs(v) + 1e-6, (step, k, m[k], v)
        for nm in NETS:
            for i, (p, q) in enumerate(zip(getattr(ag, nm).parameters(), getattr(tw, nm))):
                q = q.detach().numpy()
                err = float(np.abs(p.cpu().numpy().reshape(q.shape) - q).max())
                assert err <= P.traj_bar(q, step), (step, nm, i, err, P.traj_bar(q, step))
    assert ag.engine.opt_steps() == (5, 5)


# ---- graph, poison, rebinding -----------------------------------------------------------------------------------------------------------
SHAPE = P.Case(24, 6, 128, 64, 'fp32', 0, 0, 'tight', 'random', '')


def _arena(seed, B=64, lengths=(200, 300, 250)):
    from exorl_amd.engine import ReplayEngine
    from exorl_amd.replay_buffer import ArenaIterator
    eng = ReplayEngine((24,), np.float32, 6, 0, 4096, 64)
    eng.set_order([eng.append_episode(ep) for ep in _synth.synth_episodes(seed, list(lengths), 24, 6)])
    eng.seed_philox(77)
    return eng, ArenaIterator(eng, B, 1, 0.99, 'philox')


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
def test_graph_equals_eager_and_poisoned_scratch(precision):
    """Three agents from one seed over three equal arenas, three steps: a captured graph, eager launches, and eager launches with the
    scratch refilled with NaN before every step (use_tb=False: the fused path, device sampler, device noise). Parameters, gradients, Adam
    moments, targets and the search's results bit for bit."""
    c = SHAPE._replace(precision=precision)
    runs = []
    for mode in ('graph', 'eager', 'poison'):
        torch.manual_seed(3)
        ag = P.make_agent(c, False)
        keep = _arena(9)
        assert ag.bind_dataset(keep[1]) == 750
        if mode == 'graph':
            assert ag.enable_graph(keep[1])
        for s in range(3):
            if mode == 'poison':
                ag.engine.poison_scratch()
            assert ag.update(keep[1], s) == {}
        torch.cuda.synchronize()
        runs.append((ag, keep, [t.clone() if torch.is_tensor(t) else t for t in ag.engine.nn_result()]))
    for ag, _, nn in runs[1:]:
        assert_same_bits(state_of(runs[0][0], metrics=False), state_of(ag, metrics=False), f'{precision}')
        for x, y in zip(runs[0][2][:3], nn[:3]):
            assert torch.equal(x, y)
    assert runs[0][0].engine.opt_steps() == runs[1][0].engine.opt_steps() == (3, 3)
    # the sampled rows are table rows: every row's own key is at d2 = |mu - a|^2 and no other state is as near
    g, keep, nn = runs[0]
    with pytest.raises(L().ExorlError, match='captured graph'):
        g.engine.set_prdc(keep[0], P.BETA)
    # the arena changes under the captured graph: the step is refused, nothing is launched
    steps = g.engine.opt_steps()
    slot = keep[0].append_episode(_synth.synth_episodes(1, [5], 24, 6)[0])
    with pytest.raises(L().ExorlError, match='stale'):
        g.update(keep[1], 3)
    assert g.engine.opt_steps() == steps
    # a new table after disable_graph: bind, capture and step again
    g.disable_graph()
    keep[0].set_order([0, 1, 2, slot])
    assert g.bind_dataset(keep[1], key_every=2) == -(-755 // 2)
    assert g.enable_graph(keep[1])
    g.update(keep[1], 3)
    torch.cuda.synchronize()
    assert g.engine.opt_steps() == (4, 4) and int(g.engine.nn_result()[0].max()) < 378


def test_pickle_and_snapshot_round_trip():
    from exorl_amd import snapshot
    c = SHAPE
    torch.manual_seed(5)
    a = P.make_agent(c, beta=3.0)
    keep = _arena(11)
    a.bind_dataset(keep[1])
    batches = [_synth.synth_batch(11, s, c.B, c.O, c.A) for s in range(4)]
    ns = _synth.NoiseStream(2)
    z = [ns.draw((c.B, c.A)) for _ in range(8)]
    for s in range(2):
        hooked(a, z[2 * s:2 * s + 2]).update(iter([batches[s]]), s)
    b = pickle.loads(pickle.dumps(a))
    assert b.beta == 3.0 and b.engine.opt_steps() == (2, 2) and b.nn_table_rows == 0
    with pytest.raises(L().ExorlError, match='no key table bound'):
        b.update(iter([batches[2]]), 2)
    assert b.engine.opt_steps() == (2, 2)
    keep_b = _arena(11)             # an equal arena of its own: a second build on `keep` would replace the table `a` is bound to
    assert b.bind_dataset(keep_b[1]) == 750
    for s in range(2, 4):
        assert hooked(a, z[2 * s:2 * s + 2]).update(iter([batches[s]]), s) == hooked(b, z[2 * s:2 * s + 2]).update(iter([batches[s]]), s)
    assert_same_bits(state_of(a), state_of(b), 'pickle')
    sd = snapshot.state_dicts(a)
    torch.manual_seed(6)
    fresh = P.make_agent(c, beta=3.0)
    snapshot.load_state_dicts(fresh, dict(sd))
    for nm in NETS:
        for p, q in zip(getattr(a, nm).parameters(), getattr(fresh, nm).parameters()):
            assert torch.equal(p, q), nm
    fresh.bind_dataset(keep_b[1])
    hooked(fresh, z[:2]).update(iter([batches[0]]), 0)


def test_act_equals_td3bc_act():
    from exorl_amd import agents
    c = P.CASES[1]
    ag = P.load_params(P.make_agent(c), c)
    td = agents.TD3BCAgent('td3_bc', (c.O,), (c.A,), 'cuda', 1e-4, c.H, 0.01, 0.2, 1, c.B, 0.3, True, 2.5)
    td.actor.load_state_dict(ag.actor.state_dict())
    obs = np.random.RandomState(1).standard_normal(c.O).astype(np.float32)
    mean, inv = np.full(c.O, 0.25, np.float32), np.full(c.O, 2.0, np.float32)
    for a in (ag, td):
        a.num_expl_steps = 0
        a.set_obs_normalizer(mean, inv)
    assert np.array_equal(ag.act(obs, 0, True), td.act(obs, 0, True))


# ---- train_offline ------------------------------------------------------------------------------------------------------------------
def test_train_offline_binds_through_the_normaliser(tmp_path):
    """Two directories of synthetic episode files, normalize_obs=True, 20 steps through the captured graph: the keys are built from the
    normalised rows, so a sampled row queried with its own action is at distance exactly 0 from its key."""
    from exorl_amd.replay_buffer import save_episode
    from exorl_amd.train_offline import train_offline
    O, A, B = 24, 6, 64
    dirs = []
    for d, seed in (('a', 1), ('b', 2)):
        (tmp_path / d).mkdir()
        for i, ep in enumerate(_synth.synth_episodes(seed, [40, 50, 60], O, A)):
            ep = dict(ep, observation=(3.0 + 2.0 * ep['observation']).astype(np.float32))
            save_episode(ep, tmp_path / d / f'episode_{i}_{len(ep["reward"]) - 1}.npz')
        dirs.append(tmp_path / d)
    torch.manual_seed(0)
    ag = P.make_agent(SHAPE)
    rows = train_offline(ag, dirs, 20, B, 0.99, log_every_steps=10, normalize_obs=True, mix=[0.5, 0.5])
    torch.cuda.synchronize()
    assert ag.nn_table_rows == 300 and ag.engine.opt_steps() == (20, 20) and ag._graph_iter is not None
    assert len(rows) == 2 and all(np.isfinite(r['nn_dist']) and r['nn_dist'] > 0 for _, r in rows)
    it = ag._graph_iter
    eng = it.engine
    res = eng.sample(8, 1, 0.99, sampler=L().SAMPLER_PHILOX)
    assert abs(float(res[0].mean())) < 0.5                       # normalised: the stored rows have mean 3
    keys = eng.keys()
    q = torch.zeros(8, keys.shape[1], device='cuda')
    q[:, :O] = np.float32(P.BETA) * res[0]
    q[:, O:O + A] = res[1]
    idx = torch.zeros(8, dtype=torch.int32, device='cuda')
    d2 = torch.ones(8, device='cuda')
    L().check(L().load().exorl_nn_search(keys.data_ptr(), keys.shape[0], keys.shape[1], O + A, q.data_ptr(), keys.shape[1], 8, 0, idx.data_ptr(),
                                         d2.data_ptr(), L().current_stream()))
    torch.cuda.synchronize()
    assert d2.cpu().tolist() == [0.0] * 8


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from exorl_amd import agents
    from exorl_amd.engine import AgentEngine, ReplayEngine
    c = P.CASES[0]
    ag = P.make_agent(c)
    b = P.batch(c)
    with pytest.raises(L().ExorlError, match='no key table bound'):
        ag.update(iter([b]), 0)
    with pytest.raises(L().ExorlError, match='no key table bound'):
        ag.engine.update_phase(12, 0.2)
    assert ag.engine.opt_steps() == (0, 0)
    eng, it = P.arena_of([P.episode(c)], c.O, c.A)
    eng.build_keys(2.0)
    td = agents.TD3BCAgent('td3_bc', (c.O,), (c.A,), 'cuda', 1e-4, c.H, 0.01, 0.2, 1, c.B, 0.3, True, 2.5)
    with pytest.raises(L().ExorlError, match='not PRDC'):
        td.engine.set_prdc(eng, 2.0)
    with pytest.raises(L().ExorlError):
        td.engine.update_phase(12, 0.2)                     # phase 12 is PRDC's
    with pytest.raises(L().ExorlError, match='beta=2, not 3'):
        ag.engine.set_prdc(eng, 3.0)
    other = P.arena_of(_synth.synth_episodes(1, [9], c.O + 1, c.A), c.O + 1, c.A)[0]
    other.build_keys(2.0)
    with pytest.raises(L().ExorlError, match='observation'):
        ag.engine.set_prdc(other, 2.0)
    with pytest.raises(L().ExorlError, match='world_size=2'):
        AgentEngine('prdc', c.O, c.A, c.H, c.B, world_size=2)
    stacked = ReplayEngine((4, 8, 8), np.uint8, c.A, 0, 64, 4, frame_stack=2)
    from exorl_amd.replay_buffer import ArenaIterator
    with pytest.raises(ValueError, match='not pixels'):
        ag.bind_dataset(ArenaIterator(stacked, c.B, 1, 0.99, 'philox'))
    assert ag.enable_metric_window() is False
    with pytest.raises(L().ExorlError, match='no metric window'):
        ag.engine.set_metric_window()
    with pytest.raises(NotImplementedError):
        ag.evaluate(iter([b]))
    with pytest.raises(L().ExorlError):
        ag.engine.set_eval()
    with pytest.raises(ValueError, match='beta'):
        P.make_agent(c, beta=-1.0)
    assert ctypes.sizeof(L().AgentCfg) == 80
    ag.bind_dataset(it)
    ag.update(iter([b]), 0)
    assert ag.engine.opt_steps() == (1, 1)
