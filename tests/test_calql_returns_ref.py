"""CPU checks of the return-to-go column's definition (tests/_calql_returns_ref.py): the backward recurrence is the gather's n-step
recurrence carried to the episode's end, in float64 and against the float32 oracle gather, and G_1 is the episode return that
exorl_replay_episode_returns is held to (tests/test_gpu_fqe.py). No GPU is touched."""
import numpy as np
import pytest

import _synth
from _calql_returns_ref import forward_return64, lookup, returns_to_go64
from oracle.replay import gather_nstep

LENGTHS = [1, 2, 3, 17, 40]


def _episodes(ones):
    eps = _synth.synth_episodes(17, LENGTHS, 3, 2)
    if ones:
        for ep in eps:
            ep['discount'] = np.ones_like(ep['discount'])
    return eps


@pytest.mark.parametrize('gamma', [0.99, 1.0])
@pytest.mark.parametrize('ones', [False, True], ids=['sprinkled', 'ones'])
def test_backward_recurrence_is_sample_tails_carried_to_the_end(ones, gamma):
    """G_idx against the forward recurrence from idx over the L - idx + 1 remaining steps, both float64: 1e-12 of sum |D_t r_t| (at most 40
    reassociated terms cost 40 * 2^-53 = 4.4e-15 of it). G_L = r_L exactly, and a zero discount cuts the tail exactly."""
    for ep in _episodes(ones):
        L = len(ep['reward']) - 1
        G = returns_to_go64(ep, gamma)
        assert G.shape == (L,) and G[L - 1] == np.float64(ep['reward'][L, 0])
        for idx in range(1, L + 1):
            R, mass = forward_return64(ep, gamma, idx, L - idx + 1)
            assert abs(G[idx - 1] - R) <= 1e-12 * mass, (L, idx, G[idx - 1], R)
            if ep['discount'][idx, 0] == 0.0:
                assert G[idx - 1] == np.float64(ep['reward'][idx, 0])


@pytest.mark.parametrize('gamma', [0.99, 1.0])
def test_nstep_sample_to_the_end_is_the_return_to_go(gamma):
    """The float32 oracle gather with n = L - idx + 1 against G_idx. Over n steps the float32 recurrence rounds D twice a step (relative
    error <= 2 t 2^-24 at step t), each product once and each sum once: |R32 - G| <= (3 n + 2) 2^-24 sum |D_t r_t|."""
    worst = 0.0
    for ep in _episodes(False):
        L = len(ep['reward']) - 1
        G = returns_to_go64(ep, gamma)
        for idx in range(1, L + 1):
            n = L - idx + 1
            R32 = float(gather_nstep(ep, idx, n, gamma)[2][0])
            _, mass = forward_return64(ep, gamma, idx, n)
            bar = (3 * n + 2) * 2.0 ** -24 * mass
            worst = max(worst, abs(R32 - G[idx - 1]) / bar) if bar else worst
            assert abs(R32 - G[idx - 1]) <= bar, (L, idx, R32, G[idx - 1])
    print(f'[calql returns] gamma {gamma}: worst |R32 - G| / bar = {worst:.3f}')


def test_first_entry_is_the_episode_return():
    """G_1 against the sequential float64 episode return tests/test_gpu_fqe.py holds exorl_replay_episode_returns to, at its tolerance."""
    for ep in _episodes(False):
        L = len(ep['reward']) - 1
        R, mass = forward_return64(ep, 0.99, 1, L)
        assert abs(returns_to_go64(ep, 0.99)[0] - R) <= 1e-12 * mass


def test_lookup_indexes_by_position_and_start():
    cols = [np.array([1.0, 2.0], np.float32), np.array([5.0], np.float32)]
    assert lookup(cols, [[0, 2], [1, 1], [0, 1]]).tolist() == [2.0, 5.0, 1.0]
