"""CPU restatement of the weighted Philox draw of the HBM replay (exorl_replay_set_weights), in Python ints.

    span_e = max(len_e - nstep + 1, 0)
    mass_e = q_e * span_e                 ('transitions')
             q_e if span_e > 0 else 0     ('episodes')
    cum    = prefix sum of the masses in table order, cum[0] = 0
    x      = philox4x32_10((sample, batch_lo, batch_hi, 0), (seed_lo, seed_hi))          — the unweighted sampler's call
    g      = ((x2 << 32 | x3) * cum[n]) >> 64
    pos    = the index with cum[pos] <= g < cum[pos + 1]
    start  = ((x1 * span_pos) >> 32) + 1

Shared by tests/test_replay_weights_abi.py (CPU) and tests/test_gpu_replay_weights.py (device stream == this, pair for pair).
"""
import numpy as np

from oracle.replay import philox4x32_10


def quantise(w):
    """What exorl_amd.engine.quantise_weights is specified to return, restated: rint(w / max * 2^24) in float64, positives floored at 1."""
    w = np.asarray(w, np.float64)
    q = np.rint(w / w.max() * float(1 << 24))
    q[(w > 0) & (q < 1)] = 1
    return [int(v) for v in q]


def cum_table(lengths, q, nstep, weighting):
    q = [1] * len(lengths) if q is None else [int(v) for v in q]
    cum = [0]
    for n, w in zip(lengths, q):
        span = max(int(n) - nstep + 1, 0)
        cum.append(cum[-1] + (w * span if weighting == 'transitions' else (w if span > 0 else 0)))
    return cum


def search(cum, g):
    """Binary search: the largest pos with cum[pos] <= g (g < cum[-1]); zero-mass entries own an empty interval and are never returned."""
    lo, hi = 0, len(cum) - 1
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if cum[mid] <= g:
            lo = mid
        else:
            hi = mid
    return lo


def search_scan(cum, g):
    """Brute force: the first interval [cum[i], cum[i+1]) that holds g."""
    for i in range(len(cum) - 1):
        if cum[i] <= g < cum[i + 1]:
            return i
    raise AssertionError((g, cum[-1]))


def weighted_draw(seed, batch_counter, sample, cum, lengths, nstep):
    x = philox4x32_10((sample, batch_counter & 0xFFFFFFFF, batch_counter >> 32, 0), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    g = (((x[2] << 32) | x[3]) * cum[-1]) >> 64
    pos = search(cum, g)
    span = int(lengths[pos]) - nstep + 1
    assert span > 0, (pos, lengths[pos], nstep)
    return pos, ((x[1] * span) >> 32) + 1


def weighted_pairs(seed, batch_counter, batch, lengths, nstep, weighting, q=None):
    """(batch, 2) int32 array of (position, start) for one batch: what exorl_replay_last_pairs must return."""
    cum = cum_table(lengths, q, nstep, weighting)
    assert 0 < cum[-1] < 1 << 63
    return np.array([weighted_draw(seed, batch_counter, b, cum, lengths, nstep) for b in range(batch)], np.int32).reshape(batch, 2)


def mix_q(lengths_per_dataset, mix, weighting, nstep=1):
    """Integer weights, one per episode in dataset order, of a mix: f_d / M_d quantised; M_d = total span ('transitions') or the number
    of sampleable episodes ('episodes')."""
    w = []
    for f, lens in zip(mix, lengths_per_dataset):
        spans = [max(n - nstep + 1, 0) for n in lens]
        m = sum(spans) if weighting == 'transitions' else sum(1 for s in spans if s > 0)
        w += [f / m] * len(lens)
    return quantise(w)
