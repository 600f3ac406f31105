"""CPU checks of the replay's next-action column: the numpy rule (tests/_next_action_rule.py) against hand-built episodes, and the abi facts
that need no device: the three fields trail exorl_batch_out in the header and in ctypes, a BatchOut built from ten values leaves them
NULL, nothing else of the interface moved, and DeviceReplayIterator's per-segment BatchOut carries them with the segment's offset."""
import ctypes
import re
from pathlib import Path

import numpy as np

from _next_action_rule import next_action_rule

ROOT = Path(__file__).resolve().parents[1]


def test_next_action_rule_on_hand_built_episodes():
    """Three episodes of lengths 1, 3 and 2 (2, 4 and 3 arena rows, row 0 of each the dummy step). Action rows are numbered 10 e + t."""
    lengths = [1, 3, 2]
    act = np.concatenate([[[10.0 * e + t, -(10.0 * e + t)] for t in range(n + 1)] for e, n in enumerate(lengths)]).astype(np.float32)
    pairs = [(0, 1), (1, 1), (1, 2), (1, 3), (2, 1), (2, 2)]
    na, v = next_action_rule(act, lengths, pairs, 1)
    assert v.tolist() == [0, 1, 1, 0, 1, 0]
    assert na[:, 0].tolist() == [0, 12, 13, 0, 22, 0] and na[:, 1].tolist() == [0, -12, -13, 0, -22, 0]
    na, v = next_action_rule(act, lengths, [(1, 1), (2, 1)], 2)         # nstep = 2: idx + 2 <= len
    assert v.tolist() == [1, 0] and na[:, 0].tolist() == [13, 0]
    na, v = next_action_rule(act, lengths, [(1, 1)], 3)                 # the last start of the longest episode at nstep = 3
    assert v.tolist() == [0] and not na.any()
    # an invalid sample never looks at the arena: behind the last episode's last transition there is no row (index 9 of 9 rows)
    assert len(act) == 9
    na, v = next_action_rule(act, lengths, [(2, 2)], 1)
    assert v.tolist() == [0] and not na.any()


def test_fields_trail_the_struct_and_default_to_null():
    from exorl_amd import _lib as L
    header = (ROOT / 'include' / 'exorl_hip.h').read_text()
    d = {k: int(v) for k, v in re.findall(r'#define EXORL_([A-Z0-9_]+)\s+(\d+)', header)}
    assert d['ABI_VERSION'] == 13 == L.load().exorl_abi_version()
    assert ctypes.sizeof(L.BatchOut) == 80 + 24 and ctypes.sizeof(L.AgentCfg) == 80
    names = [f[0] for f in L.BatchOut._fields_]
    assert names == ['obs', 'obs_stride', 'action', 'action_stride', 'reward', 'discount', 'next_obs', 'next_obs_stride', 'meta', 'meta_stride',
                     'next_action', 'next_action_stride', 'next_valid']
    ten = L.BatchOut(1, 2, 3, 4, 5, 6, 7, 8, 9, 10)           # how every caller from before builds one: the rest is zero
    assert (ten.next_action, ten.next_action_stride, ten.next_valid) == (None, 0, None)
    body = re.search(r'typedef struct \{[^}]*?\} exorl_batch_out;', header, re.S).group(0)
    fields = re.findall(r'^\s*(?:void|float)\*\s+(\w+);(?:\s+int64_t (\w+);)?', body, re.M)
    assert [n for pair in fields for n in pair if n] == names


def test_segments_carry_the_fields_with_their_offset():
    """DeviceReplayIterator.sample_into on a stand-in shard: fetch_every = 5 cuts a batch of 12 into segments of 5, 5 and 2 rows; each
    segment's BatchOut points next_action / next_valid at its own rows, and a BatchOut without them stays without them."""
    from types import SimpleNamespace
    from exorl_amd import _lib as L
    from exorl_amd.replay_buffer import DeviceReplayIterator
    A, B = 3, 12
    seen = []
    engine = SimpleNamespace(sample_into=lambda seg, n, nstep, gamma, sampler: seen.append(
        (n, seg.action, seg.next_action, seg.next_action_stride, seg.next_valid)))
    shard = SimpleNamespace(fns=['x'], frozen=False, since_fetch=0, try_fetch=lambda: setattr(shard, 'since_fetch', 0), engine=engine)
    it = object.__new__(DeviceReplayIterator)
    it.loader = SimpleNamespace(batch_size=B, fetch_every=5, nstep=1, discount=0.99, sampler=L.SAMPLER_PHILOX)
    it.shards, it.turn = [shard], 0
    it._ensure_normalizer = lambda: None
    it._load_shard = lambda shard: None
    out = L.BatchOut(1 << 20, 24, 2 << 20, A, 3 << 20, 4 << 20, 5 << 20, 24, None, 0, 6 << 20, A, 7 << 20)
    it.sample_into(out, B)
    assert [s[0] for s in seen] == [5, 5, 2]
    starts = [0, 5, 10]
    assert [s[1] for s in seen] == [(2 << 20) + 4 * A * r for r in starts]
    assert [s[2] for s in seen] == [(6 << 20) + 4 * A * r for r in starts] and all(s[3] == A for s in seen)
    assert [s[4] for s in seen] == [(7 << 20) + 4 * r for r in starts]
    seen.clear()
    it.sample_into(L.BatchOut(1 << 20, 24, 2 << 20, A, 3 << 20, 4 << 20, 5 << 20, 24, None, 0), B)
    assert [(s[2], s[3], s[4]) for s in seen] == [(None, 0, None)] * 3
