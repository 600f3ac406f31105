"""The replay's next-action column (exorl_batch_out.next_action / next_valid) on the GPU: the numpy rule of tests/_next_action_rule.py bit for
bit over GIVEN pairs that include every last valid start, zeros on the invalid rows, and the ordinary outputs unchanged against the same
call with the fields NULL — on plain, frame-stacked and normalised arenas, after an eviction and a new order, through
DeviceReplayIterator across a segment boundary, under Philox, and for the arena's last episode with the arena filled to capacity."""
import random

import numpy as np
import pytest
import torch

import _synth
from _next_action_rule import next_action_rule

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 40]


def L():
    from exorl_amd import _lib
    return _lib


def all_starts(lengths, nstep):
    """Every (position, idx) a sample call accepts: idx = 1 .. len - nstep + 1, the last valid start of every episode among them."""
    return np.array([[p, idx] for p, n in enumerate(lengths) for idx in range(1, n - nstep + 2)], np.int32).reshape(-1, 2)


def with_next(eng, batch):
    """alloc_batch's tensors and BatchOut, then NaN-filled next_action (B, A) / next_valid (B) tensors wired into the BatchOut."""
    res, out = eng.alloc_batch(batch)
    na = torch.full((batch, eng.act_dim), float('nan'), device=eng.device)
    nv = torch.full((batch,), float('nan'), device=eng.device)
    out.next_action, out.next_action_stride, out.next_valid = na.data_ptr(), eng.act_dim, nv.data_ptr()
    return res, out, na, nv


def same_bits(xs, ys):
    assert len(xs) == len(ys)
    for x, y in zip(xs, ys):
        assert torch.equal(x.view(torch.uint8) if x.dtype != torch.uint8 else x, y.view(torch.uint8) if y.dtype != torch.uint8 else y)


def check(eng, eps, pairs, nstep, sampler=None):
    """One call with the fields and one without on the same pairs: the column against the rule, the rest against each other."""
    sampler = L().SAMPLER_GIVEN if sampler is None else sampler
    B = len(pairs)
    plain = eng.sample(B, nstep, 0.99, sampler, pairs=pairs)
    res, out, na, nv = with_next(eng, B)
    eng.sample_into(out, B, nstep, 0.99, sampler, pairs)
    torch.cuda.synchronize()
    same_bits(plain, res)
    want_a, want_v = next_action_rule(np.concatenate([ep['action'] for ep in eps]), [len(ep['action']) - 1 for ep in eps], pairs, nstep)
    got_a, got_v = na.cpu().numpy(), nv.cpu().numpy()
    assert got_v.tobytes() == want_v.tobytes(), (got_v, want_v)
    assert got_a.tobytes() == want_a.tobytes()
    assert not got_a[got_v == 0].any() and set(np.unique(got_v)) <= {0.0, 1.0}
    return got_v


@pytest.mark.parametrize('A', [1, 6, 65])
@pytest.mark.parametrize('nstep', [1, 3])
def test_column_equals_the_rule_on_every_start(A, nstep):
    from exorl_amd.engine import ReplayEngine
    eps = _synth.synth_episodes(3, LENGTHS, 5, A, meta_dim=2)
    eng = ReplayEngine((5,), np.float32, A, 2, 64, 8)
    eng.set_order([eng.append_episode(ep, meta_keys=('skill',)) for ep in eps])
    pairs = all_starts(LENGTHS, nstep)
    assert len(pairs) == sum(max(n - nstep + 1, 0) for n in LENGTHS)
    v = check(eng, eps, pairs, nstep)               # six ordinary outputs: the arena has meta columns
    last = [i for i, (p, idx) in enumerate(pairs) if idx + nstep > LENGTHS[p]]
    assert len(last) == sum(n >= nstep for n in LENGTHS) and not v[last].any() and v.sum() == len(pairs) - len(last)


def test_one_null_field_is_refused():
    from exorl_amd.engine import ReplayEngine
    eps = _synth.synth_episodes(3, [4], 5, 2)
    eng = ReplayEngine((5,), np.float32, 2, 0, 16, 2)
    eng.set_order([eng.append_episode(eps[0])])
    res, out, na, nv = with_next(eng, 2)
    out.next_valid = None
    with pytest.raises(L().ExorlError, match='go together'):
        eng.sample_into(out, 2, 1, 0.99, L().SAMPLER_GIVEN, np.array([[0, 1], [0, 2]], np.int32))
    torch.cuda.synchronize()
    assert torch.isnan(na).all()


def test_frame_stacked_arena():
    from exorl_amd.engine import ReplayEngine
    A, k = 6, 2
    eps = _synth.synth_episodes(4, LENGTHS, 2 * 8 * 8, A, obs_u8=True)
    eng = ReplayEngine((2 * k, 8, 8), np.uint8, A, 0, 64, 8, frame_stack=k)
    eng.set_order([eng.append_episode(ep) for ep in eps])
    for nstep in (1, 3):
        check(eng, eps, all_starts(LENGTHS, nstep), nstep)


def test_normalised_arena_copies_the_action_as_it_is():
    from exorl_amd.engine import ReplayEngine
    O, A = 8, 6
    eps = _synth.synth_episodes(5, LENGTHS, O, A)
    eng = ReplayEngine((O,), np.float32, A, 0, 64, 8)
    eng.set_order([eng.append_episode(ep) for ep in eps])
    pairs = all_starts(LENGTHS, 1)
    raw = eng.sample(len(pairs), 1, 0.99, L().SAMPLER_GIVEN, pairs=pairs)
    eng.set_obs_normalizer(np.full(O, 0.25, np.float32), np.full(O, 2.0, np.float32))
    check(eng, eps, pairs, 1)
    normed = eng.sample(len(pairs), 1, 0.99, L().SAMPLER_GIVEN, pairs=pairs)
    assert not torch.equal(raw[0], normed[0]) and torch.equal(raw[1], normed[1])


def test_after_eviction_and_a_new_order():
    from exorl_amd.engine import ReplayEngine
    A = 6
    lengths = [3, 5, 1, 40, 2]
    eps = _synth.synth_episodes(6, lengths, 5, A)
    eng = ReplayEngine((5,), np.float32, A, 0, 80, 8)
    slots = [eng.append_episode(ep) for ep in eps]
    eng.evict(slots[1])
    order = [4, 0, 3, 2]                              # positions now name these episodes; the hole of episode 1 lies between them
    eng.set_order([slots[i] for i in order])
    live = [eps[i] for i in order]
    for nstep in (1, 3):
        pairs = all_starts([lengths[i] for i in order], nstep)
        B = len(pairs)
        plain = eng.sample(B, nstep, 0.99, L().SAMPLER_GIVEN, pairs=pairs)
        res, out, na, nv = with_next(eng, B)
        eng.sample_into(out, B, nstep, 0.99, L().SAMPLER_GIVEN, pairs)
        torch.cuda.synchronize()
        same_bits(plain, res)
        for b, (p, idx) in enumerate(pairs):          # per episode: the arena's rows are no longer in order-table order
            ep, ok = live[p], idx + nstep <= len(live[p]['action']) - 1
            assert float(nv[b]) == float(ok)
            assert np.array_equal(na[b].cpu().numpy(), ep['action'][idx + nstep] if ok else np.zeros(A, np.float32))


def test_last_episode_at_its_last_transition_with_the_arena_full():
    """Behind the sampled transition there is no arena row at all. That the row is not read is a matter of reading sample_tail; what shows
    here is next_valid = 0 and the zeros."""
    from exorl_amd.engine import ReplayEngine
    A = 6
    lengths = [3, 7]
    eps = _synth.synth_episodes(7, lengths, 5, A)
    rows = sum(n + 1 for n in lengths)
    eng = ReplayEngine((5,), np.float32, A, 0, rows, 2)
    eng.set_order([eng.append_episode(ep) for ep in eps])
    assert eng.num_rows() == (rows, rows)
    for nstep in (1, 3):
        pairs = np.array([[1, lengths[1] - nstep + 1], [1, lengths[1] - nstep], [0, lengths[0] - nstep + 1]], np.int32)
        v = check(eng, eps, pairs, nstep)
        assert v.tolist() == [0.0, 1.0, 0.0]


def test_under_philox():
    from exorl_amd.engine import ReplayEngine
    A, B = 6, 96
    eps = _synth.synth_episodes(8, LENGTHS, 5, A)
    engs = []
    for _ in range(2):
        eng = ReplayEngine((5,), np.float32, A, 0, 64, 8)
        eng.set_order([eng.append_episode(ep) for ep in eps])
        eng.seed_philox(11)
        engs.append(eng)
    acts, lens = np.concatenate([ep['action'] for ep in eps]), LENGTHS
    seen = set()
    for _ in range(3):
        plain = engs[0].sample(B, 1, 0.99, L().SAMPLER_PHILOX)
        res, out, na, nv = with_next(engs[1], B)
        engs[1].sample_into(out, B, 1, 0.99, L().SAMPLER_PHILOX)
        torch.cuda.synchronize()
        same_bits(plain, res)
        pairs = engs[1].last_pairs(B)
        assert np.array_equal(pairs, engs[0].last_pairs(B))
        want_a, want_v = next_action_rule(acts, lens, pairs, 1)
        assert na.cpu().numpy().tobytes() == want_a.tobytes() and nv.cpu().numpy().tobytes() == want_v.tobytes()
        seen |= set(want_v.tolist())
    assert seen == {0.0, 1.0}


def test_device_replay_iterator_carries_the_fields_across_segments(tmp_path):
    """fetch_every = 5 and B = 16: four segments per batch, each with the fields moved by its offset. The action rows name their episode and
    step (1000 e + t in every column), so the sampled action says which next action the rule asks for, whichever sampler drew the pair."""
    from exorl_amd.replay_buffer import ReplayBufferStorage, make_replay_loader
    O, A, B, nstep = 6, 3, 16, 2
    lengths = [2, 3, 9, 14]
    eps = _synth.synth_episodes(21, lengths, O, A)
    for e, ep in enumerate(eps):
        ep['action'] = np.tile((1000.0 * (e + 1) + np.arange(len(ep['action'])))[:, None], (1, A)).astype(np.float32)
    its = []
    for name in ('a', 'b'):
        st = ReplayBufferStorage((), (), tmp_path / name)
        for ep in eps:
            st._store_episode(ep)
        random.seed(4)
        np.random.seed(4)
        its.append(iter(make_replay_loader(st, 10 ** 6, B, 0, True, nstep, 0.99, fetch_every=5)))
    for x, y in zip(next(its[0]), next(its[1])):
        assert torch.equal(x, y)
    seen = set()
    for _ in range(4):
        plain = next(its[0])
        eng = its[1].shards[0].engine
        res, out, na, nv = with_next(eng, B)
        its[1].sample_into(out, B)
        torch.cuda.synchronize()
        same_bits(plain, res)
        act, got_a, got_v = res[1].cpu().numpy(), na.cpu().numpy(), nv.cpu().numpy()
        for b in range(B):
            e, idx = int(act[b, 0]) // 1000 - 1, int(act[b, 0]) % 1000
            ok = idx + nstep <= lengths[e]
            assert got_v[b] == float(ok), (b, e, idx)
            assert np.array_equal(got_a[b], np.full(A, 1000.0 * (e + 1) + idx + nstep if ok else 0.0, np.float32))
            seen.add(ok)
    assert seen == {True, False}
