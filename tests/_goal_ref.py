"""Numpy restatement of the replay's goal relabelling rule (include/exorl_hip.h at exorl_replay_set_goal), built on the
oracle's Philox and n-step gather. Test infrastructure: the GPU is held to this integer for integer and bit for bit.

Sample b is the pair (pos, idx): obs at time t = idx - 1 of episode pos, next_obs at t + n (n = nstep), T = len[pos] >= t + n. A goal is a
pair (pos_g, tau), arena row row0[pos_g] + tau, and g = o_goal[cols] (through the normaliser's two roundings when one is set).
  x = philox4x32_10((b, ctr_lo, ctr_hi, 1), seed); t_cur = floor(p_cur 2^32), t_traj = floor((p_cur + p_traj) 2^32)
  x[0] < t_cur   CUR   pos_g = pos, tau = t + n
  x[0] < t_traj  TRAJ  pos_g = pos, room = T - (t + n), tau = t + n + d; uniform: d = (x[1] (room + 1)) >> 32; geometric:
                       d = min(#{k : tab[k] <= x[1]}, room), tab[k] = floor(2^32 (1 - p_k)), p_0 = gamma_h, p_(k+1) = p_k gamma_h in double,
                       the table cut before its first entry >= 2^32 - 1 or after 4096 entries
  else           RAND  y = philox4x32_10((b, ctr_lo, ctr_hi, 2), seed); pos_g = the sampler's own episode choice on y (y[0] scaled onto
                       the episode count; on a weighted arena the 64 bits y[2], y[3] scaled onto the total mass and searched in the prefix
                       sums); tau = (y[1] (len[pos_g] + 1)) >> 32
reached = (pos_g == pos and tau == t + n). Reward and discount: the oracle's recurrence on per-step inputs (rho_i, c_i): 'keep' the arena's;
'neg' (0, 0) on the reaching step else (-1, 1); 'sparse' (1, 0) on the reaching step else (0, 1); only step n - 1 can be the reaching one."""
import bisect
import math

import numpy as np

from oracle.replay import gather_nstep_batch, philox4x32_10

CUR, TRAJ, RAND = 0, 1, 2
TAB_MAX = 4096


def thresholds(p_cur, p_traj):
    return int(math.floor(float(p_cur) * 4294967296.0)), int(math.floor((float(p_cur) + float(p_traj)) * 4294967296.0))


def horizon_table(gamma_h):
    """tab[k] = floor(2^32 (1 - gamma_h^(k+1))), the power by repeated multiplication in double."""
    tab, g = [], float(gamma_h)
    p = g
    for _ in range(TAB_MAX):
        e = math.floor(4294967296.0 * (1.0 - p))
        if e >= 4294967295:
            break
        tab.append(int(e))
        p *= g
    return np.array(tab, np.uint32)


def episode_cum(lens, nstep, weights=None, mode='episodes'):
    """Prefix sums of the episode masses of a weighted arena (TRANSITIONS: q span, EPISODES: q where span > 0), span = max(len - n + 1, 0);
    None for the unweighted sampler (no weights, mode 'episodes')."""
    if weights is None and mode == 'episodes':
        return None
    q = np.ones(len(lens), np.int64) if weights is None else np.asarray(weights, np.int64)
    span = np.maximum(np.asarray(lens, np.int64) - nstep + 1, 0)
    mass = q * span if mode == 'transitions' else np.where(span > 0, q, 0)
    return [0] + [int(v) for v in np.cumsum(mass)]


def pick_episode(y, n_episodes, cum):
    if cum is None:
        return (y[0] * n_episodes) >> 32
    u = (y[2] << 32) | y[3]
    g = (u * cum[-1]) >> 64
    return bisect.bisect_right(cum, g) - 1      # the episode whose [cum[p], cum[p+1]) holds g: zero-mass episodes own an empty interval


def _block(seed, counter, b, k):
    return philox4x32_10((b, counter & 0xFFFFFFFF, counter >> 32, k), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def draw_pairs(seed, counter, batch, lens, nstep, cum=None):
    """The (pos, idx) of every sample of Philox batch `counter`: block (b, counter, 0), the sampler's own draw."""
    out = np.zeros((batch, 2), np.int32)
    for b in range(batch):
        x = _block(seed, counter, b, 0)
        pos = pick_episode(x, len(lens), cum)
        out[b] = pos, ((x[1] * (int(lens[pos]) - nstep + 1)) >> 32) + 1
    return out


def draw_goals(seed, counter, pairs, lens, nstep, p_cur, p_traj, gamma_h=None, cum=None):
    """((batch, 2) int32 goals (pos_g, tau), (batch,) source tags) of Philox batch `counter` for the samples `pairs`."""
    t_cur, t_traj = thresholds(p_cur, p_traj)
    tab = None if gamma_h is None else horizon_table(gamma_h)
    goals, src = np.zeros((len(pairs), 2), np.int32), np.zeros(len(pairs), np.int32)
    for b, (pos, idx) in enumerate(np.asarray(pairs).tolist()):
        x = _block(seed, counter, b, 1)
        tn = idx - 1 + nstep
        if x[0] < t_cur:
            goals[b], src[b] = (pos, tn), CUR
        elif x[0] < t_traj:
            room = int(lens[pos]) - tn
            d = (x[1] * (room + 1)) >> 32 if tab is None else min(int(np.searchsorted(tab, np.uint32(x[1]), side='right')), room)
            goals[b], src[b] = (pos, tn + d), TRAJ
        else:
            y = _block(seed, counter, b, 2)
            pg = pick_episode(y, len(lens), cum)
            goals[b], src[b] = (pg, (y[1] * (int(lens[pg]) + 1)) >> 32), RAND
    return goals, src


def reached(pairs, goals, nstep):
    pairs, goals = np.asarray(pairs), np.asarray(goals)
    return (goals[:, 0] == pairs[:, 0]) & (goals[:, 1] == pairs[:, 1] - 1 + nstep)


def normalise(x, mean32, inv32, cols=None):
    """norm_row's two roundings, in float32: the subtraction, then the product."""
    m, w = (np.asarray(a, np.float32) if cols is None else np.asarray(a, np.float32)[list(cols)] for a in (mean32, inv32))
    return ((x.astype(np.float32) - m).astype(np.float32) * w).astype(np.float32)


def relabel(obs, act, rew, disc, row0, pairs, goals, nstep, gamma, cols, mode, norm=None):
    """(obs, action, reward (B, 1), discount (B, 1), next_obs, g (B, G), reached (B,)) at the picks `pairs` / `goals` over a flat row arena
    (obs (rows, O), act (rows, A), rew / disc (rows, 1); row0: the arena row of every episode's dummy first row, by position)."""
    pairs, goals, row0 = np.asarray(pairs, np.int64), np.asarray(goals, np.int64), np.asarray(row0, np.int64)
    B, n = len(pairs), nstep
    o, a, R, D, no = gather_nstep_batch(obs, act, rew, disc, row0[pairs[:, 0]], pairs[:, 1], n, gamma)
    hit = reached(pairs, goals, n)
    if mode != 'keep':
        rho = np.full((B, n), -1.0 if mode == 'neg' else 0.0, np.float32)
        c = np.ones((B, n), np.float32)
        rho[hit, n - 1] = 0.0 if mode == 'neg' else 1.0
        c[hit, n - 1] = 0.0
        dummy = np.zeros((B * n + 1, 1), np.float32)
        _, _, R, D, _ = gather_nstep_batch(dummy, dummy, rho.reshape(-1, 1), c.reshape(-1, 1), np.arange(B, dtype=np.int64) * n,
                                           np.zeros(B, np.int64), n, gamma)
    g = obs[row0[goals[:, 0]] + goals[:, 1]][:, list(cols)]
    if norm is not None:
        o, no, g = normalise(o, *norm), normalise(no, *norm), normalise(g, *norm, cols=cols)
    return o, a, R, D, no, g, hit
