"""TEST INFRASTRUCTURE: the return-to-go column's definition in numpy (exorl_replay_build_returns, include/exorl_hip.h).

For an episode of length L (rows 1 .. L behind the dummy row 0), gamma the caller's float32 widened to float64:
    G_L = r_L,    G_i = r_i + (gamma d_i) G_{i+1},
every operation in float64. returns_to_go64 is that recurrence and nothing else; the kernel's scan reassociates it."""
import numpy as np


def returns_to_go64(ep, gamma):
    """float64 array (L,): G_1 .. G_L of one episode dict (reward / discount of len + 1 rows, dummy first)."""
    r, d = ep['reward'].reshape(-1).astype(np.float64), ep['discount'].reshape(-1).astype(np.float64)
    g = np.float64(np.float32(gamma))
    G = np.zeros(len(r), np.float64)
    acc = 0.0
    for i in range(len(r) - 1, 0, -1):
        acc = r[i] + (g * d[i]) * acc
        G[i] = acc
    return G[1:]


def forward_return64(ep, gamma, idx, nstep):
    """sample_tail's recurrence (exorl_amd/csrc/replay.hip; replay_buffer.py:229-234) in float64 from step idx over nstep steps:
    (R, sum_t |D_t r_t|)."""
    r, d = ep['reward'].reshape(-1).astype(np.float64), ep['discount'].reshape(-1).astype(np.float64)
    g = np.float64(np.float32(gamma))
    R, D, mass = 0.0, 1.0, 0.0
    for i in range(nstep):
        R += D * r[idx + i]
        mass += abs(D * r[idx + i])
        D *= d[idx + i] * g
    return R, mass


def lookup(columns, pairs):
    """The float32 values a gather writes for (position, idx) pairs from returns_to_go()'s list of per-episode arrays."""
    return np.array([columns[p][i - 1] for p, i in np.asarray(pairs).reshape(-1, 2)], np.float32)
