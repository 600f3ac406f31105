"""The goal relabelling rule as tests/_goal_ref.py restates it, on the reference alone: every pick obeys its constraints, the degenerate
mixes do what they say, and the source shares and the geometric offsets have the distribution the rule promises. The GPU tests then hold
the kernel to this reference exactly, so they have no statistical bar of their own."""
import math

import numpy as np
import pytest

import _goal_ref as G

SEED = 0x1234ABCD5
N = 65536
LENS = [1, 2, 7, 1000, 40, 3]


def draw(lens, nstep, p_cur, p_traj, gamma_h, n=N, cum=None, counter=5):
    pairs = G.draw_pairs(SEED, counter, n, lens, nstep, cum)
    goals, src = G.draw_goals(SEED, counter, pairs, lens, nstep, p_cur, p_traj, gamma_h, cum)
    return pairs, goals, src


@pytest.fixture(scope='module')
def mixed():
    """One large batch of the default mix with the geometric horizon, shared (and left unchanged) by the tests below."""
    return draw(LENS, 1, 0.2, 0.5, 0.99)


@pytest.mark.parametrize('nstep,lens,gamma_h', [(1, LENS, None), (1, LENS, 0.99), (3, [3, 7, 1000, 40], None), (3, [3, 7, 1000, 40], 0.9)])
def test_every_pick_obeys_its_constraints(nstep, lens, gamma_h):
    pairs, goals, src = draw(lens, nstep, 0.2, 0.5, gamma_h, n=4096)
    L = np.asarray(lens)
    t = pairs[:, 1] - 1
    assert (pairs[:, 1] >= 1).all() and (t + nstep <= L[pairs[:, 0]]).all()
    own = src != G.RAND
    assert (goals[own, 0] == pairs[own, 0]).all()                                     # CUR and TRAJ stay in the episode
    assert (goals[own, 1] >= t[own] + nstep).all() and (goals[own, 1] <= L[pairs[own, 0]]).all()
    assert (goals[src == G.CUR, 1] == t[src == G.CUR] + nstep).all()
    rnd = src == G.RAND
    assert (goals[rnd, 0] >= 0).all() and (goals[rnd, 0] < len(lens)).all()
    assert (goals[rnd, 1] >= 0).all() and (goals[rnd, 1] <= L[goals[rnd, 0]]).all()
    assert {G.CUR, G.TRAJ, G.RAND} <= set(src.tolist())


def test_p_cur_1_is_next_obs_and_reached_everywhere():
    nstep, lens = 3, [3, 7, 40]
    rs = np.random.RandomState(0)
    rows = sum(lens) + len(lens)
    obs, act = rs.standard_normal((rows, 5)).astype(np.float32), rs.standard_normal((rows, 2)).astype(np.float32)
    rew, disc = rs.uniform(size=(rows, 1)).astype(np.float32), np.ones((rows, 1), np.float32)
    row0 = np.concatenate([[0], np.cumsum(np.asarray(lens) + 1)[:-1]])
    pairs, goals, src = draw(lens, nstep, 1.0, 0.0, None, n=512)
    assert (src == G.CUR).all()
    cols = [4, 0]
    for mode in ('neg', 'sparse'):
        o, a, R, D, no, g, hit = G.relabel(obs, act, rew, disc, row0, pairs, goals, nstep, 0.99, cols, mode)
        assert hit.all() and np.array_equal(g, no[:, cols]) and (D == 0.0).all()
    _, _, R, _, _, _, _ = G.relabel(obs, act, rew, disc, row0, pairs, goals, nstep, 0.99, cols, 'neg')
    g32 = np.float32(0.99)
    assert (R == np.float32(np.float32(-1.0) + np.float32(-g32))).all()              # -1 - gamma, the reaching third step adds 0
    _, _, R, _, _, _, _ = G.relabel(obs, act, rew, disc, row0, pairs, goals, nstep, 0.99, cols, 'sparse')
    assert (R == np.float32(g32 * g32)).all()                                         # gamma^2 on the reaching third step
    keep = G.relabel(obs, act, rew, disc, row0, pairs, goals, nstep, 0.99, cols, 'keep')
    plain = G.gather_nstep_batch(obs, act, rew, disc, row0[pairs[:, 0]], pairs[:, 1].astype(np.int64), nstep, 0.99)
    for x, y in zip(keep[:5], plain):
        assert x.tobytes() == y.tobytes()


def test_unreached_samples_get_the_plain_not_reached_values():
    pairs = np.array([[0, 1], [0, 2]], np.int32)
    goals = np.array([[0, 5], [1, 2]], np.int32)                                      # a later state; the same time in ANOTHER episode
    z = np.zeros((20, 1), np.float32)
    for mode, want_r in (('neg', -1.0), ('sparse', 0.0)):
        _, _, R, D, _, _, hit = G.relabel(np.zeros((20, 3), np.float32), z, z, z, [0, 10], pairs, goals, 1, 0.99, [0], mode)
        assert not hit.any() and (R == want_r).all() and (D == np.float32(0.99)).all()


def test_p_rand_1_on_a_weighted_table_never_picks_a_zero_weight_episode():
    lens = [5, 9, 2, 30, 4]
    q = [3, 0, 1, 0, 7]
    for mode in ('episodes', 'transitions'):
        cum = G.episode_cum(lens, 1, q, mode)
        pairs, goals, src = draw(lens, 1, 0.0, 0.0, None, n=8192, cum=cum)
        assert (src == G.RAND).all()
        assert set(goals[:, 0].tolist()) == {0, 2, 4} and set(pairs[:, 0].tolist()) == {0, 2, 4}


def test_source_shares_lie_within_4_sigma(mixed):
    _, _, src = mixed
    for tag, p in ((G.CUR, 0.2), (G.TRAJ, 0.5), (G.RAND, 0.3)):
        sigma = math.sqrt(p * (1 - p) / N)
        assert abs(np.mean(src == tag) - p) <= 4 * sigma, (tag, np.mean(src == tag), p, sigma)


def test_geometric_offsets_have_the_tables_truncated_mean():
    """All samples TRAJ in one long episode: d = min(K, room) with K drawn from the table. Per sample the mean and variance of min(K, room)
    follow from the table's own probabilities; the batch mean must lie within 4 standard errors of the mean of those means."""
    lens, gamma_h, n = [1000], 0.99, N
    pairs, goals, src = draw(lens, 1, 0.0, 1.0, gamma_h, n=n)
    assert (src == G.TRAJ).all()
    d = goals[:, 1] - pairs[:, 1]                                                     # tau - (t + n), n = 1
    room = lens[0] - pairs[:, 1]
    assert (d >= 0).all() and (d <= room).all()
    tab = G.horizon_table(gamma_h).astype(np.float64)
    assert len(tab) < G.TAB_MAX and (np.diff(tab) >= 0).all()
    edges = np.concatenate([[0.0], tab, [4294967296.0]])
    pk = np.diff(edges) / 4294967296.0                                                # P(K = k), k = 0 .. len(tab): K = #{tab <= x}
    assert abs(pk.sum() - 1.0) < 1e-12
    ks = np.arange(len(pk), dtype=np.float64)
    mean, var = np.zeros(lens[0] + 1), np.zeros(lens[0] + 1)
    for r in range(lens[0] + 1):
        v = np.minimum(ks, r)
        mean[r] = (pk * v).sum()
        var[r] = (pk * v * v).sum() - mean[r] ** 2
    want = mean[room].mean()
    se = math.sqrt(var[room].sum()) / n
    assert abs(d.mean() - want) <= 4 * se, (d.mean(), want, se)


def test_draws_are_a_pure_function_of_seed_counter_and_sample(mixed):
    pairs, goals, _ = mixed
    again = draw(LENS, 1, 0.2, 0.5, 0.99, n=64)
    assert np.array_equal(again[0], pairs[:64]) and np.array_equal(again[1], goals[:64])
    other = draw(LENS, 1, 0.2, 0.5, 0.99, n=64, counter=6)
    assert not np.array_equal(other[1], goals[:64])
    # the sample's own pair does not depend on the goal mix: block 0 is left alone
    assert np.array_equal(draw(LENS, 1, 1.0, 0.0, None, n=64)[0], pairs[:64])
