"""Offline state agents on goal-conditioned batches: update() fed zero-copy by a goal ArenaIterator equals the same agent fed host tuples
that tests/_goal_ref.py builds from the read-back picks, the captured step (exorl_agent_enable_graph_goal) equals the eager one, a pickled
agent continues identically, a later set_goal makes the graph stale, and train_offline(goal=...) runs with a hold-out split."""
import pickle

import numpy as np
import pytest
import torch

import _goal_ref as G
import _synth

pytestmark = pytest.mark.gpu

O, A, H, B = 24, 6, 128, 64
COLS = [0, 1]
W = O + len(COLS)
LENS = [200, 300, 7, 250]
SEED, GAMMA = 77, 0.99
NETS = ('actor', 'critic', 'critic_target', 'value')


def make(kind, precision):
    from exorl_amd import agents
    torch.manual_seed(3)
    if kind == 'td3_bc':
        return agents.TD3BCAgent('td3_bc', (W,), (A,), 'cuda', 1e-4, H, 0.01, '0.2', 1, B, 0.3, True, 2.5, precision=precision)
    if kind == 'iql':
        return agents.IQLAgent('iql', (W,), (A,), 'cuda', 1e-4, H, 0.01, '0.2', 1, B, True, precision=precision)
    return agents.BCAgent('bc', (W,), (A,), 'cuda', 1e-4, H, B, '0.2', True, precision=precision)


def goal_rule(reward='neg'):
    from exorl_amd.replay_buffer import GoalRelabel
    return GoalRelabel(COLS, reward=reward)


@pytest.fixture(scope='module')
def episodes():
    eps = _synth.synth_episodes(9, LENS, O, A)
    flat = {k: np.concatenate([ep[k] for ep in eps]) for k in ('observation', 'action', 'reward', 'discount')}
    row0 = np.concatenate([[0], np.cumsum(np.asarray(LENS) + 1)[:-1]]).astype(np.int64)
    return eps, flat, row0


def goal_iterator(eps, rule=None):
    from exorl_amd.engine import ReplayEngine
    from exorl_amd.replay_buffer import ArenaIterator
    eng = ReplayEngine((O,), np.float32, A, 0, 1024, 8)
    eng.set_order([eng.append_episode(ep) for ep in eps])
    eng.seed_philox(SEED)
    return ArenaIterator(eng, B, 1, GAMMA, 'philox', goal=rule or goal_rule())


def state_of(ag):
    out = {}
    for nm in NETS:
        net = getattr(ag, nm, None)
        if net is not None:
            for i, p in enumerate(net.parameters()):
                out[f'{nm}.param{i}'] = p.detach().clone()
    out['metrics'] = torch.from_numpy(ag.engine.metrics_raw())
    return out


def assert_same_bits(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        assert not bool(torch.isnan(b[k]).any()), f'{tag}: NaN in {k}'
        assert torch.equal(a[k], b[k]), f'{tag}: {k} differs (max |d| = {float((a[k] - b[k]).abs().max()):.3e})'


def hooked(ag, draws):
    """`ag` with its next exploration-noise draws supplied from the host, in order."""
    src = iter(draws)
    ag.noise_hook = lambda shape: next(src)
    return ag


def host_batch(it, flat, row0, counter):
    """The batch the iterator's last launch produced, rebuilt by the reference from the read-back picks (which are checked on the way)."""
    pairs, goals = it.engine.last_pairs(B), it.engine.last_goals(B)
    want_pairs = G.draw_pairs(SEED, counter, B, LENS, 1)
    want_goals, _ = G.draw_goals(SEED, counter, want_pairs, LENS, 1, 0.2, 0.5, 0.99)
    assert np.array_equal(pairs, want_pairs) and np.array_equal(goals, want_goals)
    o, a, R, D, no, g, _ = G.relabel(flat['observation'], flat['action'], flat['reward'], flat['discount'], row0, pairs, goals, 1, GAMMA, COLS, 'neg')
    return tuple(torch.from_numpy(np.ascontiguousarray(x)) for x in (np.concatenate([o, g], 1), a, R, D, np.concatenate([no, g], 1)))


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('kind', ['td3_bc', 'iql', 'bc'])
def test_zero_copy_graph_and_pickle_agree_bit_for_bit(kind, precision, episodes):
    eps, flat, row0 = episodes
    # 1. zero copy against host tuples built by the reference
    zero, it = make(kind, precision), goal_iterator(eps)
    batches, ms = [], []
    for s in range(3):
        ms.append(zero.update(it, s))
        batches.append(host_batch(it, flat, row0, s))
    host = make(kind, precision)
    assert [host.update(iter([b]), s) for s, b in enumerate(batches)] == ms
    assert_same_bits(state_of(zero), state_of(host), 'host tuples')
    assert all(np.isfinite(v) for m in ms for v in m.values()) and ms[0]
    # 2. the captured goal step against the eager one
    graph, it_g = make(kind, precision), goal_iterator(eps)
    assert graph.enable_graph(it_g) and graph._graph_iter is it_g
    assert [graph.update(it_g, s) for s in range(3)] == ms
    torch.cuda.synchronize()
    assert_same_bits(state_of(zero), state_of(graph), 'graph')
    assert np.array_equal(it_g.engine.last_goals(B), it.engine.last_goals(B))
    # 3. a pickled agent continues identically: the original on its iterator, the copy on the reference's host tuples. The device noise
    # counter is not part of a pickle, so both take their exploration noise from the same host draws, as the other pickle tests do
    copy = pickle.loads(pickle.dumps(zero))
    ns = _synth.NoiseStream(2)
    for s in range(3, 5):
        zs = [ns.draw((B, A)) for _ in range(2)]
        m = hooked(zero, zs).update(it, s)
        assert hooked(copy, zs).update(iter([host_batch(it, flat, row0, s)]), s) == m
    assert_same_bits(state_of(zero), state_of(copy), 'pickle')


def test_set_goal_after_the_capture_makes_the_graph_stale(episodes):
    from exorl_amd import _lib as L
    eps, _, _ = episodes
    ag, it = make('td3_bc', 'fp32'), goal_iterator(eps)
    assert ag.enable_graph(it)
    ag.update(it, 0)
    it.engine.set_goal(goal_rule('sparse'))
    with pytest.raises(L.ExorlError, match='exorl_replay_set_goal was called after the capture'):
        ag.update(it, 1)
    assert ag.enable_graph(it)
    ag.update(it, 1)
    torch.cuda.synchronize()
    assert ag.engine.opt_steps() == (2, 2)
    from exorl_amd.replay_buffer import GoalRelabel
    narrow, narrow_it = make('td3_bc', 'fp32'), goal_iterator(eps, GoalRelabel([0, 1, 2]))          # O + 3 columns for an agent of O + 2
    with pytest.raises(L.ExorlError, match='do not fill the agent'):
        narrow.enable_graph(narrow_it)
    with pytest.raises(ValueError, match='obs_shape'):
        narrow.update(narrow_it, 0)


def write_dataset(path, n_eps=12, ep_len=60, seed=0):
    rs = np.random.RandomState(seed)
    path.mkdir(parents=True, exist_ok=True)
    for e in range(n_eps):
        rows = ep_len + 1
        ep = dict(observation=rs.standard_normal((rows, O)).astype(np.float32), action=rs.uniform(-1, 1, (rows, A)).astype(np.float32),
                  reward=rs.uniform(0, 1, (rows, 1)).astype(np.float32), discount=np.ones((rows, 1), np.float32))
        np.savez_compressed(path / f'20240101T000000_{e}_{ep_len}.npz', **ep)


def test_train_offline_with_goals_and_a_holdout_split(tmp_path):
    from exorl_amd.train_offline import train_offline
    write_dataset(tmp_path / 'buffer')
    ag = make('td3_bc', 'bf16x3')
    rows = train_offline(ag, tmp_path / 'buffer', 20, B, GAMMA, eval_every_steps=10, log_every_steps=5, goal=goal_rule(), normalize_obs=True,
                         holdout_every=4, val_batches=2)
    torch.cuda.synchronize()
    assert ag._graph_iter is not None and ag._graph_iter.goal is not None and ag.engine.opt_steps() == (20, 20)
    logged = [r for _, r in rows if 'fps' in r]
    vals = [r for _, r in rows if 'val_rows' in r]
    assert len(logged) == 4 and len(vals) == 2 and vals[0]['val_rows'] == 2 * B
    for r in logged + vals:
        assert all(np.isfinite(v) for v in r.values()), r
    assert logged[-1]['batch_reward'] <= 0.0 and logged[-1]['batch_reward'] >= -1.0        # the relabelled reward: 0 or -1 per row
    mean, inv = ag._graph_iter.obs_normalizer
    assert mean.shape == inv.shape == (W,) and np.array_equal(mean[O:], mean[COLS]) and np.array_equal(inv[O:], inv[COLS])
    obs = ag._graph_iter.goal_obs(np.zeros(O, np.float32), np.ones(O, np.float32))
    assert obs.shape == (W,) and ag.act(obs, 20, True).shape == (A,)
