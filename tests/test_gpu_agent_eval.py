"""Held-out validation on the GPU: agent.evaluate() against the float64 twin over the forward dispatch grid (tests/_eval_twin.py), its
read-only contract around eager and captured steps, its independence of scratch, the window's arithmetic, the H2D fallback, the hold-out
split of the offline loader, and train_offline with validation switched on."""
import numpy as np
import pytest
import torch

import _eval_twin as E
import _grad_grid as G
import _obs_norm as N
import _synth
from test_gpu_grad_grid import assert_bit_identical, make, state_of
from test_gpu_train_offline import write_dataset

pytestmark = pytest.mark.gpu

CASE_PARAMS = [pytest.param(c, id=G.case_id(c)) for c in E.CASES]


def route_of(c):
    """The precision route of a case: what csrc/agent.hip's route_of / planes_ok / planes3_ok decide from the shape."""
    if c.precision == 'bf16x3':
        return 'bf16x3-planes' if c.H % 128 == 0 and c.B % 64 == 0 else 'bf16x3-split'
    if c.precision == 'bf16x6':
        return 'bf16x6-planes' if c.H % 128 == 0 and c.B % 128 == 0 else 'bf16x6-split'
    return c.precision


def _one_per_kind_and_route():
    seen, out = set(), []
    for c in E.CASES:
        k = (G.base_kind(c), route_of(c))
        if k not in seen and c.B <= 1024 and c.H <= 320:
            seen.add(k)
            out.append(pytest.param(c, id=G.case_id(c)))
    return out


ROUTE_PARAMS = _one_per_kind_and_route()


def fresh(c, use_tb=False):
    """An agent of the case's kind and shape with the case's seeded parameters; the target equals the critic."""
    torch.manual_seed(0)
    ag = make(c, use_tb)
    _, _, pa, pc = G.params(c)
    ag.actor.load_state_dict({k: torch.from_numpy(v) for k, v in pa.items()})
    if pc:
        ag.critic.load_state_dict({k: torch.from_numpy(v) for k, v in pc.items()})
        ag.critic_target.load_state_dict(ag.critic.state_dict())
    return ag


def other_batch(c, step):
    return _synth.synth_batch(c.seed + 7, step, c.B, c.O, c.A)


def sums_of(ag, batch):
    """The window after one forward-only pass on `batch`, read and emptied."""
    if getattr(ag.engine, '_eval', None) is None:
        ag.engine.set_eval()
    ag._load_batch(iter([batch]))
    ag.engine.evaluate()
    return ag.engine.eval_read(reset=True)


# ---- values over the forward dispatch grid -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', CASE_PARAMS)
def test_values_vs_twin64(c):
    """Every returned value against the float64 twin at the project's metric bars (E.BARS): fp32 and bf16x6 2e-5 |v| + 1e-6, bf16x3
    1e-4 |v| + 1e-6, plain bf16 3e-2 |v| + 3e-2. val_q_gap is the difference of the two checked values."""
    ag = fresh(c)
    got = ag.evaluate(iter([G.batch(c)]))
    want = E.twin_values(c, torch.float64)
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    assert got['val_rows'] == c.B
    keys = [k for k in E.VALUE_KEYS if k in want]
    ratios = {k: abs(got[k] - want[k]) / E.bar(c.precision, want[k]) for k in keys}
    worst = max(ratios, key=ratios.get)
    print(f'[agent eval] {G.case_id(c)}: worst error / bar = {ratios[worst]:.3f} at {worst} ' + ' '.join(f'{k}={got[k]:.6g}' for k in keys))
    for k in keys:
        assert np.isfinite(got[k]) and abs(got[k] - want[k]) <= E.bar(c.precision, want[k]), (G.case_id(c), k, got[k], want[k])
    if 'val_q_gap' in want:
        assert got['val_q_gap'] == got['val_q_pi'] - got['val_q_data']


# ---- read-only ---------------------------------------------------------------------------------------------------------------------
def full_state(ag):
    """state_of plus what else a step leaves behind: the metric window, the optimiser step counts and the noise counter."""
    torch.cuda.synchronize()
    out = state_of(ag)
    sums, steps = ag.engine.metric_window_read(reset=False)
    out['window_sums'] = torch.from_numpy(np.append(sums, float(steps)))
    out['opt_steps'] = torch.tensor(ag.engine.opt_steps())
    out['noise_counter'] = torch.tensor([ag.engine.noise_counter()], dtype=torch.int64)
    return out


@pytest.mark.parametrize('c', ROUTE_PARAMS)
def test_evaluate_leaves_eager_updates_bit_identical(c):
    """Three update()s (device noise, windowed metrics) with evaluate() before, between and after them on other batches, against three
    update()s alone: parameters, targets, gradients, the metric block, the metric window, step counts, noise counter, CQL's scalars."""
    states = []
    for with_eval in (False, True):
        ag = fresh(c)
        assert ag.enable_metric_window()
        for step in range(3):
            if with_eval and step < 2:
                v = ag.evaluate(iter([other_batch(c, 10 + step)]))
                assert v['val_rows'] == c.B and all(np.isfinite(x) for x in v.values())
            ag.update(iter([_synth.synth_batch(c.seed + 2, step, c.B, c.O, c.A)]), step)
        if with_eval:
            ag.evaluate(iter([other_batch(c, 12), other_batch(c, 13)]), num_batches=2)
        states.append(full_state(ag))
    assert states[0]['opt_steps'].tolist() == ([3, 3] if G.base_kind(c) != 'bc' else [3, 0])
    assert_bit_identical(states[0], states[1], f'{G.case_id(c)} eager')


def _arena(seed, lengths, B, philox_seed):
    from exorl_amd.engine import ReplayEngine
    from exorl_amd.replay_buffer import ArenaIterator
    O, A = 24, 6
    eng = ReplayEngine((O,), np.float32, A, 0, 4096, 64)
    eng.set_order([eng.append_episode(ep) for ep in _synth.synth_episodes(seed, lengths, O, A)])
    eng.seed_philox(philox_seed)
    return eng, ArenaIterator(eng, B, 1, 0.99, 'philox')


@pytest.mark.parametrize('precision,H,B', [pytest.param('fp32', 128, 64, id='fp32'), pytest.param('bf16x3', 128, 64, id='bf16x3-planes')])
def test_evaluate_leaves_the_captured_graph_bit_identical(precision, H, B):
    """train_offline's pairing: TD3+BC, the Philox sampler and the update captured as one graph, windowed metrics; evaluate() on a
    hold-out arena before, between and after the graph launches. The bound iterator stays bound and the fast path is kept."""
    c = G.Case('td3_bc', 24, 6, H, B, 0, precision, 0, 'tight', '')
    states, keep = [], []
    for with_eval in (False, True):
        torch.manual_seed(3)
        ag = make(c, False)
        e, it = _arena(9, [200, 300, 250], B, 77)
        he, hit = _arena(19, [120, 90], B, 78)
        assert ag.enable_metric_window() and ag.enable_graph(it)
        captures = ag.engine.graph_captures
        for step in range(3):
            if with_eval:
                v = ag.evaluate(hit, 2)
                assert v['val_rows'] == 2 * B
            ag.update(it, step)
        if with_eval:
            ag.evaluate(hit)
        assert ag._graph_iter is it and ag.engine.graph_captures == captures
        states.append(full_state(ag))
        keep.append((ag, e, he))
    assert states[0]['opt_steps'].tolist() == [3, 3]
    assert_bit_identical(states[0], states[1], f'graph {precision}')


# ---- scratch independence --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', ROUTE_PARAMS)
def test_poisoned_scratch_is_not_read(c):
    """Scratch filled with NaN bit patterns immediately before evaluate(): the same sums, bit for bit, and no NaN; once on a fresh
    workspace and once on the leftovers of a step."""
    ag = fresh(c)
    b = other_batch(c, 20)
    clean, rows = sums_of(ag, b)
    for after_update in (False, True):
        if after_update:
            ag.update(iter([G.batch(c)]), 0)
            clean, rows = sums_of(ag, b)
        ag._load_batch(iter([b]))
        ag.engine.poison_scratch()
        ag.engine.evaluate()
        dirty, rows2 = ag.engine.eval_read(reset=True)
        assert rows == rows2 == c.B and not np.isnan(dirty).any(), (G.case_id(c), dirty)
        assert np.array_equal(clean, dirty), (G.case_id(c), after_update, clean, dirty)


# ---- window arithmetic -----------------------------------------------------------------------------------------------------------------
WINDOW_CASES = [c for c in E.CASES if (G.base_kind(c), c.H, c.B, c.precision) in (('td3_bc', 32, 50, 'fp32'), ('cql', 128, 64, 'bf16x3'),
                                                                                ('bc', 192, 1000, 'fp32'), ('crr', 128, 128, 'bf16x6'))]


@pytest.mark.parametrize('c', [pytest.param(c, id=G.case_id(c)) for c in WINDOW_CASES])
def test_window_arithmetic(c):
    """K batches in one window == the float64 sum, in order, of the K single-batch windows, bit for bit; reset empties the window;
    val_rows == K B; a second agent gives identical bits."""
    from exorl_amd import _lib as L, agents
    assert len(WINDOW_CASES) == 4
    K = 3
    batches = [other_batch(c, 30 + k) for k in range(K)]
    runs = []
    for _ in range(2):
        ag = fresh(c)
        singles = [sums_of(ag, b) for b in batches]
        for b in batches:
            ag._load_batch(iter([b]))
            ag.engine.evaluate()
        peek, peek_rows = ag.engine.eval_read(reset=False)
        window, rows = ag.engine.eval_read(reset=True)
        empty, empty_rows = ag.engine.eval_read(reset=True)
        want = np.zeros(L.N_EVAL)
        for s, r in singles:
            assert r == c.B and s[L.E_ROWS] == c.B
            want = want + s
        assert rows == peek_rows == K * c.B and np.array_equal(window, want) and np.array_equal(peek, window)
        assert empty_rows == 0 and not empty.any()
        v = ag.evaluate(iter(batches), num_batches=K)
        assert v == agents.eval_values(window, rows, c.A, G.base_kind(c) != 'bc') and v['val_rows'] == K * c.B
        runs.append((singles, window))
    for (s0, _), (s1, _) in zip(*[r[0] for r in runs]):
        assert np.array_equal(s0, s1)
    assert np.array_equal(runs[0][1], runs[1][1])


def test_eval_calls_are_refused_without_a_buffer_and_for_other_kinds():
    from exorl_amd import _lib as L
    ag = fresh(G.Case('td3_bc', 24, 6, 32, 8, 0, 'fp32', 0, 'tight', ''))
    with pytest.raises(L.ExorlError, match='agent_evaluate: no eval buffer'):
        ag.engine.evaluate()
    with pytest.raises(L.ExorlError, match='agent_eval_read: no eval buffer'):
        ag.engine.eval_read()
    ag.engine.set_eval()
    ag.engine.set_eval(None)
    with pytest.raises(L.ExorlError, match='agent_evaluate: no eval buffer'):
        ag.engine.evaluate()
    with pytest.raises(L.ExorlError, match='agent_set_eval: buffer'):
        ag.engine.set_eval(torch.empty(256, dtype=torch.uint8, device='cuda'))
    ddpg = make(G.Case('ddpg', 24, 6, 32, 8, 0, 'fp32', 0, 'tight', ''), False)
    with pytest.raises(L.ExorlError, match='no forward-only evaluation'):
        ddpg.engine.set_eval()
    with pytest.raises(NotImplementedError, match='TD3BCAgent'):
        ddpg.evaluate(iter([]))


def test_the_eval_buffer_is_not_pickled():
    import pickle
    c = G.Case('td3_bc', 24, 6, 32, 8, 0, 'fp32', 0, 'tight', '')
    ag = fresh(c)
    b = other_batch(c, 1)
    v = ag.evaluate(iter([b]))
    blob = pickle.dumps(ag)
    assert getattr(ag.engine, '_eval', None) is not None
    ag2 = pickle.loads(blob)
    assert getattr(ag2.engine, '_eval', None) is None and ag2.evaluate(iter([b])) == v


# ---- H2D fallback ---------------------------------------------------------------------------------------------------------------------
def test_h2d_fallback_equals_the_zero_copy_path():
    """The same rows through sample_into (zero copy) and through an iterator of 5-tuples (next() + set_batch): the same values."""
    c = G.Case('td3_bc', 24, 6, 64, 72, 0, 'fp32', 0, 'tight', '')
    ag = fresh(c)
    _, it = _arena(5, [80, 40, 130], c.B, 11)
    _, it2 = _arena(5, [80, 40, 130], c.B, 11)
    zero_copy = ag.evaluate(it, 3)
    tuples = (tuple(t.cpu().numpy() for t in next(it2)) for _ in range(3))
    assert not hasattr(tuples, 'sample_into')
    assert ag.evaluate(tuples, 3) == zero_copy and zero_copy['val_rows'] == 3 * c.B


# ---- the hold-out loader -----------------------------------------------------------------------------------------------------------------
O, A = 5, 2


def write_indexed(path, lengths, first_index=0, seed=0, offset_held=None):
    """Episodes whose observation column 0 is their index; with offset_held=k every k-th (the ones a holdout_every=k split holds out)
    has 50 added to column 1, so moments that include them are far from the training episodes' alone."""
    rs = np.random.RandomState(seed)
    path.mkdir(parents=True, exist_ok=True)
    eps = []
    for i, n in enumerate(lengths):
        obs = rs.standard_normal((n + 1, O)).astype(np.float32)
        obs[:, 0] = first_index + i
        if offset_held and (i + 1) % offset_held == 0:
            obs[:, 1] += 50.0
        ep = dict(observation=obs, action=rs.uniform(-1, 1, (n + 1, A)).astype(np.float32),
                  reward=rs.uniform(0, 1, (n + 1, 1)).astype(np.float32), discount=np.ones((n + 1, 1), np.float32))
        np.savez_compressed(path / f'20240101T0000{i:02d}_{first_index + i}_{n}.npz', **ep)
        eps.append(ep)
    return eps


def _indices(it, batches):
    seen = []
    for _ in range(batches):
        b = next(it)
        assert torch.equal(b[0][:, 0], b[4][:, 0])        # obs and next_obs of one episode
        seen.append(b[0][:, 0].cpu().numpy())
    return np.concatenate(seen).round().astype(int)


def test_holdout_split_separates_the_episodes(tmp_path):
    from exorl_amd.replay_buffer import make_offline_replay_loader
    lengths = [20, 35, 12, 40, 9, 27, 31, 16, 22, 14, 38]
    write_indexed(tmp_path / 'd', lengths)
    it = iter(make_offline_replay_loader(None, tmp_path / 'd', 10**6, 64, 1, 0.99, sampler='philox', seed=5, holdout_every=4))
    held = {3, 7}
    train = _indices(it, 40)
    hold = _indices(it.holdout, 20)
    assert set(train) == set(range(11)) - held and set(hold) == held
    assert it.holdout is it.holdout and (it.holdout.nstep, it.holdout.discount, it.holdout.batch_size) == (1, 0.99, 64)
    # transition-uniform on the hold-out side: episode 3 (40 transitions) against episode 7 (16)
    share = float((hold == 3).mean())
    assert abs(share - 40 / 56) <= 5 * np.sqrt(40 / 56 * 16 / 56 / len(hold)), share
    # a distinct stream: the hold-out arena's seed is derived from the loader's, not equal to it
    it2 = iter(make_offline_replay_loader(None, tmp_path / 'd', 10**6, 64, 1, 0.99, sampler='philox', seed=5, holdout_every=4))
    assert np.array_equal(_indices(it2.holdout, 20), hold) and np.array_equal(_indices(it2, 40), train)
    # sample_into into an agent's slots, as evaluate() pulls it
    assert hasattr(it.holdout, 'sample_into')
    # without the keyword nothing is held out
    plain = iter(make_offline_replay_loader(None, tmp_path / 'd', 10**6, 64, 1, 0.99, sampler='philox', seed=5))
    assert plain.holdout is None and set(_indices(plain, 40)) == set(range(11))


def test_holdout_with_nothing_to_sample_raises(tmp_path):
    from exorl_amd.replay_buffer import make_offline_replay_loader
    write_indexed(tmp_path / 'd', [20, 35, 12])
    it = iter(make_offline_replay_loader(None, tmp_path / 'd', 10**6, 8, 1, 0.99, sampler='philox', seed=5, holdout_every=4))
    with pytest.raises(ValueError, match='no held-out episode'):
        it.holdout
    assert set(_indices(it, 10)) == {0, 1, 2}


def test_holdout_normaliser_is_the_training_episodes_alone(tmp_path):
    from exorl_amd.replay_buffer import make_offline_replay_loader
    lengths = [20, 35, 12, 40, 9, 27, 31, 16, 22]
    eps = write_indexed(tmp_path / 'd', lengths, offset_held=3)
    it = iter(make_offline_replay_loader(None, tmp_path / 'd', 10**6, 64, 1, 0.99, sampler='philox', seed=5, holdout_every=3,
                                         normalize_obs=True))
    train_eps = [ep for i, ep in enumerate(eps) if (i + 1) % 3]
    mean32, inv32 = it.obs_normalizer
    ref_mean, ref_inv = N.normalizer(*N.moments_of(train_eps))
    all_mean, _ = N.normalizer(*N.moments_of(eps))
    assert abs(all_mean[1] - ref_mean[1]) > 10.0                # the held-out episodes would have moved it
    np.testing.assert_allclose(mean32, ref_mean, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(inv32, ref_inv, rtol=1e-6)
    # both arenas apply the pair: column 0 of a sampled row is its episode's index, normalised
    for side, want in ((it, {0, 1, 3, 4, 6, 7}), (it.holdout, {2, 5, 8})):
        b = next(side)
        col = b[0][:, 0].cpu().numpy()
        index = np.rint(col.astype(np.float64) / float(inv32[0]) + float(mean32[0])).astype(int)
        assert set(index) <= want and len(col) == 64
        assert np.array_equal(col, N.normalize(index.astype(np.float32), mean32[0], inv32[0]))
    col1 = next(it.holdout)[0][:, 1].cpu().numpy()
    assert float(col1.mean()) > 10.0                            # held-out rows are far from the training mean: they had no vote


def test_mix_and_weighting_see_the_training_side_only(tmp_path):
    """mix=[0.75, 0.25] with weighting='transitions' over two directories and holdout_every=3: the existing expectation (a fraction
    mix[d] of the samples from dataset d, every transition of d equally likely) with the held-out episodes removed."""
    from exorl_amd.replay_buffer import make_offline_replay_loader
    la, lb = [30, 10, 25, 40, 15, 20, 35], [12, 18, 50, 22]
    write_indexed(tmp_path / 'a', la, 0, seed=1)
    write_indexed(tmp_path / 'b', lb, 100, seed=2)
    it = iter(make_offline_replay_loader(None, [tmp_path / 'a', tmp_path / 'b'], 10**6, 256, 1, 0.99, sampler='philox', seed=9,
                                         holdout_every=3, mix=[0.75, 0.25], weighting='transitions'))
    idx = _indices(it, 80)
    n = len(idx)
    train_a = {i: la[i] for i in range(7) if (i + 1) % 3}
    train_b = {100 + i: lb[i] for i in range(4) if (i + 1) % 3}
    assert set(idx) == set(train_a) | set(train_b)
    z = lambda count, p: (count - n * p) / np.sqrt(n * p * (1 - p))
    assert abs(z(int((idx < 100).sum()), 0.75)) <= 5
    for group, f in ((train_a, 0.75), (train_b, 0.25)):
        total = sum(group.values())
        for i, length in group.items():
            assert abs(z(int((idx == i).sum()), f * length / total)) <= 5, (i, length)
    assert set(_indices(it.holdout, 10)) == {2, 5, 102}


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_train_offline_with_validation(tmp_path):
    """holdout_every=4, val_batches=2, eval_every_steps=5 on a synthetic directory: val_* rows at steps 0, 5, 10, before eval_fn; the other
    rows and the final parameters bit-identical to the same run without validation."""
    from exorl_amd import agents
    from exorl_amd.train_offline import train_offline
    OO, AA, H, B = 11, 3, 128, 64
    write_dataset(tmp_path / 'buffer')
    out = []
    for val_batches in (0, 2):
        torch.manual_seed(0)
        np.random.seed(3)
        ag = agents.TD3BCAgent('td3_bc', (OO,), (AA,), 'cuda', 1e-4, H, 0.01, '0.2', 1, B, 0.3, False, 2.5)
        order = []
        rows = train_offline(ag, tmp_path / 'buffer', 12, B, 0.99, log_every_steps=3, eval_every_steps=5, metric_window=True,
                             holdout_every=4, val_batches=val_batches, eval_fn=lambda s, a: order.append(('eval_fn', s)),
                             log_fn=lambda s, r: order.append(('val' if 'val_rows' in r else 'row', s)))
        torch.cuda.synchronize()
        assert ag._graph_iter is not None and ag.engine.opt_steps() == (12, 12)
        out.append((rows, order, [p.clone() for p in list(ag.actor.parameters()) + list(ag.critic.parameters()) + list(ag.critic_target.parameters())]))
    (rows0, order0, p0), (rows1, order1, p1) = out
    val = [(s, r) for s, r in rows1 if 'val_rows' in r]
    assert [s for s, _ in val] == [0, 5, 10] and not any('val_rows' in r for _, r in rows0)
    for s, r in val:
        assert r['step'] == s and r['val_rows'] == 2 * B and sorted(r) == sorted(['val_bc_mse', 'val_q_data', 'val_q_pi', 'val_q_gap', 'val_critic_loss',
                                                                                 'val_critic_target_q', 'val_rows', 'step'])
        assert all(np.isfinite(v) for v in r.values())
    assert [x for x in order1 if x[1] in (0, 5, 10) and x[0] != 'row'] == [(k, s) for s in (0, 5, 10) for k in ('val', 'eval_fn')]
    strip = lambda rows: [(s, {k: v for k, v in r.items() if k not in ('fps', 'total_time')}) for s, r in rows if 'val_rows' not in r]
    assert strip(rows0) == strip(rows1) and [s for s, _ in strip(rows0)] == [0, 3, 6, 9]
    assert all(torch.equal(a, b) for a, b in zip(p0, p1))
    assert val[0][1]['val_bc_mse'] > 0


def test_window_attach_read_reset_detach():
    """The evaluation's window through its whole life at batch 259, and the buffers exorl_agent_set_eval refuses (tests/_windows.py)."""
    import _windows as W
    eng = W.engine('td3_bc')
    W.check_window(eng, 'eval', eng.evaluate, W.B, 'no eval buffer')
