"""The goal path of the HBM gather against tests/_goal_ref.py: under Philox the drawn pairs and goals integer for integer and every output bit
for bit at the edges of the gather (the 4-byte and the 16-byte copy path, one and several goal columns and the whole state, a partial last
workgroup, episodes of exactly nstep transitions, the normaliser, a weighted arena, the three reward modes, both horizons); the same for
hand-written goals under the GIVEN sampler; the sample itself unchanged by the goal destinations; and nothing written beyond O + G columns."""
import numpy as np
import pytest
import torch

import _goal_ref as G
import _synth
from _next_action_rule import next_action_rule

pytestmark = pytest.mark.gpu

SEED, GAMMA = 0x5EED0001, 0.99
NAN = float('nan')


def L():
    from exorl_amd import _lib
    return _lib


def relabel_of(cols, mix=(0.2, 0.5, 0.3), gamma_h=0.99, reward='neg'):
    from exorl_amd.replay_buffer import GoalRelabel
    return GoalRelabel(cols, *mix, horizon_discount=gamma_h, reward=reward)


def arena(lens, O, A=2, seed=3):
    from exorl_amd.engine import ReplayEngine
    eps = _synth.synth_episodes(seed, lens, O, A)
    eng = ReplayEngine((O,), np.float32, A, 0, sum(lens) + len(lens) + 8, len(lens) + 2)
    eng.set_order([eng.append_episode(ep) for ep in eps])
    flat = {k: np.concatenate([ep[k] for ep in eps]) for k in ('observation', 'action', 'reward', 'discount')}
    row0 = np.concatenate([[0], np.cumsum(np.asarray(lens) + 1)[:-1]]).astype(np.int64)
    return eng, flat, row0


def normaliser(O, seed=9):
    rs = np.random.RandomState(seed)
    return rs.standard_normal(O).astype(np.float32), rs.uniform(0.5, 2.0, O).astype(np.float32)


class Wide:
    """[obs | g] destinations of B x (O + G) floats, each the head of a NaN-filled buffer with 16 floats of tail, plus the next-action fields."""

    def __init__(self, eng, B, G_):
        self.B, self.O, self.W, A = B, eng.obs_bytes // 4, eng.obs_bytes // 4 + G_, eng.act_dim
        new = lambda n: torch.full((n + 16,), NAN, device=eng.device)
        self.bufs = {k: new(B * n) for k, n in (('obs', self.W), ('next_obs', self.W), ('action', A), ('reward', 1), ('discount', 1),
                                                ('next_action', A), ('next_valid', 1))}
        p = {k: v.data_ptr() for k, v in self.bufs.items()}
        self.out = L().BatchOut(p['obs'], 4 * self.W, p['action'], A, p['reward'], p['discount'], p['next_obs'], 4 * self.W, None, 0,
                                p['next_action'], A, p['next_valid'])
        self.width = dict(obs=self.W, next_obs=self.W, action=A, reward=1, discount=1, next_action=A, next_valid=1)

    def read(self):
        torch.cuda.synchronize()
        res = {}
        for k, buf in self.bufs.items():
            host = buf.cpu().numpy()
            n = self.B * self.width[k]
            assert np.isnan(host[n:]).all(), f'{k}: written past its {n} floats'
            res[k] = host[:n].reshape(self.B, self.width[k])
        return res


def same(got, want, what):
    want = np.ascontiguousarray(want, np.float32).reshape(got.shape)
    assert got.tobytes() == want.tobytes(), (what, got[:4], want[:4])


def check_against_reference(got, flat, row0, lens, pairs, goals, nstep, cols, mode, norm):
    O = flat['observation'].shape[1]
    o, a, R, D, no, g, hit = G.relabel(flat['observation'], flat['action'], flat['reward'], flat['discount'], row0, pairs, goals, nstep, GAMMA,
                                       cols, mode, norm)
    same(got['obs'][:, :O], o, 'obs')
    same(got['obs'][:, O:], g, 'goal behind obs')
    same(got['next_obs'][:, :O], no, 'next_obs')
    same(got['next_obs'][:, O:], g, 'goal behind next_obs')
    same(got['action'], a, 'action')
    same(got['reward'], R, 'reward')
    same(got['discount'], D, 'discount')
    na, nv = next_action_rule(flat['action'], lens, pairs, nstep)
    same(got['next_action'], na, 'next_action')
    same(got['next_valid'], nv, 'next_valid')
    return hit


# (O, cols, B, lens, nstep, normalised, (weighting, weights) or None, reward, horizon_discount)
PHILOX_CASES = [
    (3, [2], 1, [1, 2, 7, 1000], 1, False, None, 'neg', 0.99),
    (3, [0, 2], 5, [3, 7, 1000], 3, True, None, 'sparse', None),
    (3, [2, 1, 0], 257, [1, 2, 7, 1000], 1, True, ('transitions', [1.0, 0.0, 2.0, 1.0]), 'keep', 0.99),
    (8, [5], 257, [3, 2, 7, 1000], 3, False, ('episodes', [1.0, 3.0, 0.0, 2.0]), 'neg', None),
    (8, list(range(8)), 5, [1, 2, 7, 1000], 1, True, None, 'neg', 0.99),                 # rows of 64 bytes: the 16-byte copy path
    (8, [1, 6], 1, [3, 7, 1000], 3, False, None, 'keep', 0.9),
    (24, [0, 23], 257, [1, 2, 7, 1000], 1, False, None, 'sparse', None),
    (24, list(range(23, -1, -1)), 5, [3, 7, 1000], 3, True, ('transitions', None), 'neg', 0.99),      # 192-byte rows: the 16-byte path
    (24, [7], 1, [1, 2, 7, 1000], 1, True, ('episodes', [0.0, 1.0, 1.0, 5.0]), 'sparse', 0.5),
    (8, [0, 1], 5, [3, 3], 3, False, None, 'neg', None),                                 # len == nstep: every TRAJ goal is forced onto T
    (3, [1], 257, [1, 1, 1], 1, False, None, 'sparse', 0.99),
]


@pytest.mark.parametrize('O,cols,B,lens,nstep,normed,weighted,reward,gamma_h', PHILOX_CASES)
def test_philox_picks_and_outputs_equal_the_reference(O, cols, B, lens, nstep, normed, weighted, reward, gamma_h):
    from exorl_amd.engine import quantise_weights
    eng, flat, row0 = arena(lens, O)
    norm = normaliser(O) if normed else None
    if normed:
        eng.set_obs_normalizer(*norm)
    cum = None
    if weighted is not None:
        eng.set_weights(*weighted)
        cum = G.episode_cum(lens, nstep, None if weighted[1] is None else quantise_weights(weighted[1]), weighted[0])
    forced = all(n == nstep for n in lens)
    mix = (0.0, 1.0, 0.0) if forced else (0.2, 0.5, 0.3)
    eng.set_goal(relabel_of(cols, mix, gamma_h, reward))
    eng.seed_philox(SEED)
    hits = 0
    for counter in range(2):                       # two batches: the counter moves the goal blocks with the sample's own
        dst = Wide(eng, B, len(cols))
        eng.sample_into(dst.out, B, nstep, GAMMA, L().SAMPLER_PHILOX, goal=True)
        got = dst.read()
        pairs = G.draw_pairs(SEED, counter, B, lens, nstep, cum)
        goals, src = G.draw_goals(SEED, counter, pairs, lens, nstep, mix[0], mix[1], gamma_h, cum)
        assert np.array_equal(eng.last_pairs(B), pairs)
        assert np.array_equal(eng.last_goals(B), goals)
        hit = check_against_reference(got, flat, row0, lens, pairs, goals, nstep, cols, reward, norm)
        hits += int(hit.sum())
        if forced:
            assert (goals[:, 1] == np.asarray(lens)[pairs[:, 0]]).all() and hit.all()
    assert B < 257 or hits > 0                     # a large batch holds reached and unreached samples


@pytest.mark.parametrize('normed', [False, True])
@pytest.mark.parametrize('reward', ['neg', 'sparse', 'keep'])
@pytest.mark.parametrize('nstep', [1, 3])
def test_given_goals_equal_the_reference(nstep, reward, normed):
    O, cols, lens = 8, [6, 2], [4, 7, 3]
    eng, flat, row0 = arena(lens, O, A=6)
    norm = normaliser(O) if normed else None
    if normed:
        eng.set_obs_normalizer(*norm)
    eng.set_goal(relabel_of(cols, reward=reward))
    n = nstep
    #            reached           same time, other episode   time 0 of another      reached at T                earlier in its own episode
    picks = [((0, 1), (0, n)), ((0, 2), (1, 1 + n)), ((1, 3), (2, 0)), ((2, 4 - n), (2, 3)), ((1, 5), (1, 0)), ((1, 8 - n), (0, 4))]
    pairs, goals = (np.array([p[i] for p in picks], np.int32) for i in (0, 1))
    dst = Wide(eng, len(picks), len(cols))
    eng.sample_into(dst.out, len(picks), nstep, GAMMA, L().SAMPLER_GIVEN, pairs, goal=True, goals=goals)
    got = dst.read()
    assert np.array_equal(eng.last_goals(len(picks)), goals) and np.array_equal(eng.last_pairs(len(picks)), pairs)
    hit = check_against_reference(got, flat, row0, lens, pairs, goals, nstep, cols, reward, norm)
    assert hit.tolist() == [True, False, False, True, False, False]
    if reward == 'neg':
        assert (got['discount'][hit] == 0).all() and (got['discount'][~hit] != 0).all()


def test_given_goals_are_range_checked_on_the_host():
    eng, _, _ = arena([4, 7], 3)
    eng.set_goal(relabel_of([0]))
    pairs = np.array([[0, 1], [1, 1]], np.int32)
    dst = Wide(eng, 2, 1)
    for bad, msg in (([[0, 5], [1, 0]], 'time 5 out of range'), ([[0, 0], [2, 0]], 'position 2 out of range'), ([[0, -1], [1, 0]], 'out of range')):
        with pytest.raises(L().ExorlError, match=msg):
            eng.sample_into(dst.out, 2, 1, GAMMA, L().SAMPLER_GIVEN, pairs, goal=True, goals=np.array(bad, np.int32))
    with pytest.raises(L().ExorlError, match='need goals_host'):
        eng.sample_into(dst.out, 2, 1, GAMMA, L().SAMPLER_GIVEN, pairs, goal=True)
    assert all(np.isnan(v).all() for v in dst.read().values())          # a refused call launches nothing


@pytest.mark.parametrize('reward', ['keep', 'neg'])
@pytest.mark.parametrize('normed', [False, True])
def test_the_sample_does_not_depend_on_the_goal_destinations(reward, normed):
    """The drawn (pos, idx) and every plain output are what the gather without goals gives for the same seed and counter; under 'neg' all
    but reward and discount."""
    O, B, nstep, cols = 24, 257, 3, [3, 4]
    eng, flat, row0 = arena([3, 7, 1000, 40], O, A=6)
    if normed:
        eng.set_obs_normalizer(*normaliser(O))
    eng.seed_philox(SEED)
    plain = [t.cpu().numpy() for t in eng.sample(B, nstep, GAMMA, L().SAMPLER_PHILOX)]
    plain_pairs = eng.last_pairs(B)
    eng.set_goal(relabel_of(cols, reward=reward))
    eng.seed_philox(SEED)
    dst = Wide(eng, B, len(cols))
    eng.sample_into(dst.out, B, nstep, GAMMA, L().SAMPLER_PHILOX, goal=True)
    got = dst.read()
    assert np.array_equal(eng.last_pairs(B), plain_pairs)
    same(got['obs'][:, :O], plain[0], 'obs')
    same(got['action'], plain[1], 'action')
    same(got['next_obs'][:, :O], plain[4], 'next_obs')
    if reward == 'keep':
        same(got['reward'], plain[2], 'reward')
        same(got['discount'], plain[3], 'discount')
    # and with the rule still set, a call without goal destinations is the plain gather
    eng.seed_philox(SEED)
    again = [t.cpu().numpy() for t in eng.sample(B, nstep, GAMMA, L().SAMPLER_PHILOX)]
    for x, y in zip(plain, again):
        assert x.tobytes() == y.tobytes()
    eng.set_goal(None)
    with pytest.raises(ValueError, match='needs a goal rule'):
        eng.sample_into(dst.out, B, nstep, GAMMA, L().SAMPLER_PHILOX, goal=True)


def test_separate_destinations_leave_the_columns_beyond_them_untouched():
    """obs rows of O + 2 floats and goal rows of G + 3: the gather writes O and G of them; the 16-byte copy path (O = 8, 16-byte aligned)."""
    O, cols, B, nstep = 8, [7], 5, 1
    eng, flat, row0 = arena([1, 2, 7, 1000], O)
    eng.set_goal(relabel_of(cols, reward='sparse'))
    eng.seed_philox(SEED)
    res, out = eng.alloc_batch(B)
    g, ng = (torch.full((B, len(cols) + 3), NAN, device=eng.device) for _ in range(2))
    eng.sample_into(out, B, nstep, GAMMA, L().SAMPLER_PHILOX, goal=(g, ng))
    torch.cuda.synchronize()
    pairs = G.draw_pairs(SEED, 0, B, [1, 2, 7, 1000], nstep)
    goals, _ = G.draw_goals(SEED, 0, pairs, [1, 2, 7, 1000], nstep, 0.2, 0.5, 0.99)
    assert np.array_equal(eng.last_goals(B), goals)
    o, a, R, D, no, want, _ = G.relabel(flat['observation'], flat['action'], flat['reward'], flat['discount'], row0, pairs, goals, nstep, GAMMA,
                                        cols, 'sparse')
    for t, w in zip(res, (o, a, R, D, no)):
        same(t.cpu().numpy(), w, 'plain output')
    for t in (g, ng):
        host = t.cpu().numpy()
        same(host[:, :1], want, 'goal')
        assert np.isnan(host[:, 1:]).all()


def test_mc_return_goes_with_the_kept_reward_only():
    eng, _, _ = arena([4, 7, 40], 3)
    eng.build_returns(GAMMA)
    B = 5
    mc = torch.full((B,), NAN, device=eng.device)
    eng.set_goal(relabel_of([0], reward='neg'))
    dst = Wide(eng, B, 1)
    with pytest.raises(L().ExorlError, match='mc_return destination with a relabelled reward'):
        eng.sample_into(dst.out, B, 1, GAMMA, L().SAMPLER_PHILOX, mc_return=mc, goal=True)
    eng.set_goal(relabel_of([0], reward='keep'))
    eng.seed_philox(SEED)
    eng.sample_into(dst.out, B, 1, GAMMA, L().SAMPLER_PHILOX, mc_return=mc, goal=True)
    torch.cuda.synchronize()
    pairs = eng.last_pairs(B)
    rtg = eng.returns_to_go()
    assert mc.cpu().numpy().tolist() == [float(rtg[p][i - 1]) for p, i in pairs.tolist()]


def test_arena_iterator_yields_and_fills_goal_rows():
    from exorl_amd.replay_buffer import ArenaIterator
    O, cols, B = 8, [0, 3, 5], 5
    lens = [2, 7, 1000]
    eng, flat, row0 = arena(lens, O)
    eng.seed_philox(SEED)
    it = ArenaIterator(eng, B, 1, GAMMA, 'philox', goal=relabel_of(cols))
    obs_g, action, reward, discount, next_obs_g = next(it)
    assert obs_g.shape == next_obs_g.shape == (B, O + len(cols)) and action.shape == (B, 2) and reward.shape == discount.shape == (B, 1)
    pairs = G.draw_pairs(SEED, 0, B, lens, 1)
    goals, _ = G.draw_goals(SEED, 0, pairs, lens, 1, 0.2, 0.5, 0.99)
    o, a, R, D, no, g, _ = G.relabel(flat['observation'], flat['action'], flat['reward'], flat['discount'], row0, pairs, goals, 1, GAMMA, cols, 'neg')
    same(obs_g.cpu().numpy(), np.concatenate([o, g], 1), 'obs_g')
    same(next_obs_g.cpu().numpy(), np.concatenate([no, g], 1), 'next_obs_g')
    same(reward.cpu().numpy(), R, 'reward')
    same(discount.cpu().numpy(), D, 'discount')
    _, narrow = eng.alloc_batch(B)
    with pytest.raises(ValueError, match=r'expected 44\).*obs_shape=\(11,\)'):
        it.sample_into(narrow, B)
    assert it.goal_obs(np.zeros(O, np.float32), np.arange(O, dtype=np.float32)).tolist() == [0] * O + [0, 3, 5]
