"""TEST INFRASTRUCTURE: the numpy restatement of the replay's next-action column (exorl_batch_out.next_action / next_valid), shared by
tests/test_replay_next_action_abi.py (hand-built episodes, no device) and tests/test_gpu_replay_next_action.py."""
import numpy as np


def next_action_rule(actions, lengths, pairs, nstep):
    """actions: (rows, A) float32, the arena's action rows, episode e (len_e + 1 rows, row 0 the dummy step) starting at row0_e = sum of
    (len + 1) of the episodes before it; pairs: (B, 2) of (position, start idx >= 1). Returns (next_action (B, A), next_valid (B,)):
    action[row0 + idx + nstep] and 1.0 where idx + nstep <= len, else zeros and 0.0 — and in that case the arena row is not looked at."""
    actions = np.asarray(actions, np.float32)
    lengths = np.asarray(lengths, np.int64)
    row0 = np.concatenate([[0], np.cumsum(lengths + 1)[:-1]])
    out = np.zeros((len(pairs), actions.shape[1]), np.float32)
    valid = np.zeros(len(pairs), np.float32)
    for b, (pos, idx) in enumerate(np.asarray(pairs, np.int64)):
        if idx + nstep <= lengths[pos]:
            out[b] = actions[row0[pos] + idx + nstep]
            valid[b] = 1.0
    return out, valid
