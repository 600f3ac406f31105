"""References for observation normalisation in the HBM replay, independent of exorl_amd: two-pass float64 column moments, the three host
definitions restated (Chan's merge, the normaliser, the two-operation formula), and the synthetic episodes of the tests.

The data (norm_episodes): column 0 = 1000 + 0.01 N(0,1) (mean 1e5 times the spread: sum x^2 in float64 is already off by 1e-6 relative
there), column 2 (where it exists) the constant 0.37, every other column N(0,1).

The bounds (MEAN_REL, M2_REL) are those of the issue that asked for the feature: a Welford + Chan restatement of this data in float64
stays within 3e-12 relative on M2 and 2e-16 on the mean at every column count used, a sum x / sum x^2 formulation lands at 3e-7 .. 8e-6;
1e-10 passes the right algorithm with about 30x room and fails the wrong one by more than 1000x."""
import numpy as np

MEAN_REL = 1e-13        # |mean - ref| <= MEAN_REL * max(|ref mean|, ref std)
M2_REL = 1e-10          # |M2 - ref| <= M2_REL * ref M2; a constant column: M2 == 0.0 exactly
LENGTHS = [1, 2, 5, 63, 64, 65, 300]


def norm_episodes(seed, lengths, O, A, meta_dim=0):
    rs = np.random.RandomState(seed)
    eps = []
    for n in lengths:
        rows = n + 1
        obs = rs.standard_normal((rows, O))
        obs[:, 0] = 1000.0 + 0.01 * obs[:, 0]
        if O > 2:
            obs[:, 2] = 0.37
        ep = dict(observation=obs.astype(np.float32), action=rs.uniform(-1, 1, (rows, A)).astype(np.float32),
                  reward=rs.uniform(0, 1, (rows, 1)).astype(np.float32), discount=rs.choice([0.0, 0.5, 1.0], (rows, 1)).astype(np.float32))
        if meta_dim:
            ep['skill'] = rs.standard_normal((rows, meta_dim)).astype(np.float32)
        eps.append(ep)
    return eps


def two_pass(rows):
    """(count, mean, M2) of the columns of `rows` in float64: the mean first, then the squared deviations from it."""
    x = np.asarray(rows, np.float64).reshape(len(rows), -1)
    mean = x.sum(0) / len(x)
    return len(x), mean, ((x - mean) ** 2).sum(0)


def moments_of(episodes):
    return two_pass(np.concatenate([ep['observation'] for ep in episodes]))


def check_moments(got, ref, where=''):
    """The issue's bounds; prints every figure before asserting."""
    (n, mean, m2), (rn, rmean, rm2) = got, ref
    mean, m2 = np.asarray(mean, np.float64).reshape(-1), np.asarray(m2, np.float64).reshape(-1)
    rstd = np.sqrt(rm2 / rn)
    emean = np.abs(mean - rmean) / np.maximum(np.abs(rmean), rstd)
    const = rm2 == 0.0
    em2 = np.abs(m2[~const] - rm2[~const]) / rm2[~const]
    print(f'{where}: count {n} (ref {rn}); mean err max {emean.max():.3e} (bound {MEAN_REL:g}); M2 rel err max '
          f'{em2.max() if em2.size else 0.0:.3e} (bound {M2_REL:g}); constant columns {np.flatnonzero(const).tolist()} M2 {m2[const].tolist()}')
    assert n == rn
    assert np.all(emean <= MEAN_REL), emean
    assert np.all(em2 <= M2_REL), em2
    assert np.all(m2[const] == 0.0)


def chan(parts):
    """Chan's pairwise update over [(count, mean, M2), ...] in list order, float64; empty parts skipped."""
    acc = None
    for n, mean, m2 in parts:
        if n == 0:
            continue
        mean, m2 = np.asarray(mean, np.float64), np.asarray(m2, np.float64)
        if acc is None:
            acc = (n, mean, m2)
            continue
        na, ma, sa = acc
        d = mean - ma
        acc = (na + n, ma + d * (n / (na + n)), sa + m2 + d * d * (na * n / (na + n)))
    return acc


def normalizer(count, mean, m2, eps=1e-3):
    """float32(mean), float32(1 / (population std + eps)): the reciprocal in float64, rounded once."""
    std = np.sqrt(np.asarray(m2, np.float64) / count)
    return np.asarray(mean, np.float64).astype(np.float32), (1.0 / (std + eps)).astype(np.float32)


def normalize(x, mean32, inv32):
    """Two float32 operations, each rounded: the subtraction, then the product."""
    d = np.subtract(np.asarray(x, np.float32), mean32, dtype=np.float32)
    return np.multiply(d, inv32, dtype=np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)
