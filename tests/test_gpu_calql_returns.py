"""The replay's return-to-go column on the GPU (exorl_replay_build_returns / _returns / _returns_read / _sample_mc): the scan kernel against the
float64 recurrence of tests/_calql_returns_ref.py at one float32 ulp, the same bits wherever an episode sits and whatever the column held,
staleness and the refusals, and the gather's extra destination bit for bit beside outputs that do not move."""
import ctypes

import numpy as np
import pytest
import torch

import _synth
from _calql_returns_ref import lookup, returns_to_go64

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 255, 256, 257, 1000, 1025)      # run = 1, the 256 boundary, run = 5 with a ragged last run, threads past the end
ROWS = sum(LENGTHS) + len(LENGTHS)
SPARE = 40


def L():
    from exorl_amd import _lib
    return _lib


def episodes(ones, lengths=LENGTHS, O=3, A=2, seed=31):
    eps = _synth.synth_episodes(seed, list(lengths), O, A)
    if ones:
        for ep in eps:
            ep['discount'] = np.ones_like(ep['discount'])
    return eps


def arena(eps, order=None, spare=SPARE, O=3, A=2):
    """The episodes appended in `order` (positions of eps; the table keeps eps' own order)."""
    from exorl_amd.engine import ReplayEngine
    rows = sum(len(ep['reward']) for ep in eps)
    eng = ReplayEngine((O,), np.float32, A, 0, rows + spare, len(eps) + 4)
    slots = {}
    for i in (order if order is not None else range(len(eps))):
        slots[i] = eng.append_episode(eps[i])
    eng.set_order([slots[i] for i in range(len(eps))])
    return eng, slots


def column(eng, rows, write=None):
    """The whole column (`rows` floats from its first arena row) read back, or overwritten with `write`, through the HIP runtime the library
    links (the column is the library's own allocation: no tensor owns it)."""
    lib = L().load()
    ptr = eng.returns_info()[0]
    assert ptr
    torch.cuda.synchronize()
    cpy = lib.hipMemcpy
    cpy.restype, cpy.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    if write is not None:
        src = np.ascontiguousarray(write, np.float32)
        assert src.size == rows and cpy(ptr, src.ctypes.data, rows * 4, 1) == 0        # hipMemcpyHostToDevice
        return None
    out = np.zeros(rows, np.float32)
    assert cpy(out.ctypes.data, ptr, rows * 4, 2) == 0                                  # hipMemcpyDeviceToHost
    return out


@pytest.mark.parametrize('gamma', [0.99, 1.0])
@pytest.mark.parametrize('ones', [False, True], ids=['sprinkled', 'ones'])
def test_column_vs_float64_recurrence(ones, gamma):
    """|G - G64| <= 2^-23 |G64| element by element, one float32 ulp: rewards are >= 0, so nothing cancels, the scan's float64 reassociation
    costs about 1e-13 and the one rounding to float32 half an ulp. At least 99 % of the values are the correctly rounded float32 (a kernel
    that is off by a constant ulp fails this). G_1 against exorl_replay_episode_returns: 1e-12 relative, after rounding both to float32. The
    same bits on a second build and on a column that held NaN; the dummy rows are 0 and the rows outside the table keep what they held."""
    eps = episodes(ones)
    eng, _ = arena(eps)
    eng.build_returns(gamma)
    got = eng.returns_to_go()
    assert [g.shape for g in got] == [(n,) for n in LENGTHS] and all(g.dtype == np.float32 for g in got)
    worst, exact, total = 0.0, 0, 0
    for ep, g in zip(eps, got):
        want = returns_to_go64(ep, gamma)
        err = np.abs(g.astype(np.float64) - want)
        worst = max(worst, float((err / np.abs(want)).max()))
        exact += int((g == want.astype(np.float32)).sum())
        total += g.size
        assert np.all(err <= 2.0 ** -23 * np.abs(want)), (len(g), int(np.argmax(err / np.abs(want))))
    print(f'[calql returns] ones={ones} gamma={gamma}: worst |G - G64| / |G64| = {worst:.3e} (bar {2.0 ** -23:.3e}), correctly rounded {exact} of {total}')
    assert exact >= 0.99 * total
    er = eng.episode_returns(gamma)
    for e, g in enumerate(got):
        assert abs(float(g[0]) - float(np.float32(er[e]))) <= 1e-12 * abs(er[e]), (e, g[0], er[e])
    ptr, g32, epoch, valid = eng.returns_info()
    assert valid and np.float32(g32) == np.float32(gamma)
    # a second build: same bits, same pointer
    eng.build_returns(gamma)
    again = eng.returns_to_go()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    assert eng.returns_info()[0] == ptr and eng.returns_info()[2] > epoch
    # a column that held NaN everywhere: same bits, dummy rows 0, the rows behind the table untouched
    cap = ROWS + SPARE
    column(eng, cap, np.full(cap, np.nan, np.float32))
    eng.build_returns(gamma)
    col = column(eng, cap)
    row = 0
    for g in got:
        assert col[row] == 0.0 and not np.signbit(col[row])
        assert col[row + 1:row + 1 + g.size].tobytes() == g.tobytes()
        row += g.size + 1
    assert row == ROWS and np.isnan(col[ROWS:]).all()


def test_same_bits_wherever_the_episode_sits():
    """The episodes appended in another order (other arena rows, other neighbours), an episode evicted and the table shortened: every
    episode's values keep their bits, and the rows of an episode outside the table are not written."""
    eps = episodes(False)
    eng, _ = arena(eps)
    eng.build_returns(0.99)
    want = eng.returns_to_go()
    perm = [4, 0, 6, 2, 5, 1, 3]
    other, slots = arena(eps, perm)
    other.build_returns(0.99)
    got = other.returns_to_go()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(want, got))
    # out of the table: episode 5 (appended fifth in `perm`) keeps the poison, its neighbours are rebuilt
    cap = ROWS + SPARE
    column(other, cap, np.full(cap, np.nan, np.float32))
    keep = [i for i in range(len(eps)) if i != 5]
    other.set_order([slots[i] for i in keep])
    other.build_returns(0.99)
    got = other.returns_to_go()
    assert all(want[i].tobytes() == g.tobytes() for i, g in zip(keep, got))
    col = column(other, cap)
    row = 0
    for i in perm:
        n = LENGTHS[i]
        if i == 5:
            assert np.isnan(col[row:row + n + 1]).all()
        else:
            assert col[row] == 0.0 and col[row + 1:row + 1 + n].tobytes() == want[i].tobytes()
        row += n + 1


def _sample(eng, pairs, nstep=1, gamma=0.99, sampler=None, want_next=False, with_mc=True):
    """One sample call into fresh NaN-filled tensors, through exorl_replay_sample_mc with a destination or through exorl_replay_sample:
    (the ordinary outputs, mc_return or None, the recorded pairs)."""
    B = len(pairs) if pairs is not None else 64
    res, out = eng.alloc_batch(B)
    extra = ()
    if want_next:
        na = torch.full((B, eng.act_dim), float('nan'), device=eng.device)
        nv = torch.full((B,), float('nan'), device=eng.device)
        out.next_action, out.next_action_stride, out.next_valid = na.data_ptr(), eng.act_dim, nv.data_ptr()
        extra = (na, nv)
    mc = torch.full((B,), float('nan'), device=eng.device) if with_mc else None
    eng.sample_into(out, B, nstep, gamma, L().SAMPLER_GIVEN if sampler is None else sampler, pairs, mc_return=mc)
    torch.cuda.synchronize()
    return res + extra, (mc.cpu().numpy() if with_mc else None), eng.last_pairs(B)


def same_bits(xs, ys):
    assert len(xs) == len(ys)
    for x, y in zip(xs, ys):
        assert torch.equal(x.view(torch.uint8) if x.dtype != torch.uint8 else x, y.view(torch.uint8) if y.dtype != torch.uint8 else y)


MC_LENGTHS = (1, 2, 40, 300)


def _pairs(B, nstep, lengths=MC_LENGTHS):
    """B (position, idx) pairs that begin with idx = 1 and idx = last valid start of every episode that holds nstep steps."""
    edge = [[p, i] for p, n in enumerate(lengths) if n >= nstep for i in (1, n - nstep + 1)]
    rs = np.random.RandomState(B)
    ok = [p for p, n in enumerate(lengths) if n >= nstep]
    rest = [[p, int(rs.randint(1, lengths[p] - nstep + 2))] for p in rs.choice(ok, max(B - len(edge), 0))]
    return np.array((edge + rest)[:B], np.int32).reshape(-1, 2)


def _check_mc(eng, cols, nstep, want_next=False):
    for B in (1, 5, 257):
        pairs = _pairs(B, nstep)
        got, mc, rec = _sample(eng, pairs, nstep, want_next=want_next)
        ref, _, rec0 = _sample(eng, pairs, nstep, want_next=want_next, with_mc=False)
        assert mc.tobytes() == lookup(cols, pairs).tobytes(), (B, nstep)
        same_bits(got, ref)
        assert np.array_equal(np.asarray(rec), np.asarray(rec0)) and np.array_equal(np.asarray(rec).reshape(-1, 2), pairs)


@pytest.mark.parametrize('nstep', [1, 3])
def test_sample_mc_on_plain_normalised_and_next_action_gathers(nstep):
    """Pairs with idx = 1, idx = L (nstep 1) and an episode of length 1: mc_return is the column's value at the sample's own row, bit for
    bit, whatever nstep is; every other output and the recorded pairs equal exorl_replay_sample's: on a plain arena, with the next action
    requested, and with the normaliser on."""
    O, A = 8, 3
    eps = episodes(False, MC_LENGTHS, O, A, seed=7)
    eng, _ = arena(eps, O=O, A=A)
    eng.build_returns(0.99)
    cols = eng.returns_to_go()
    for ep, g in zip(eps, cols):
        assert np.allclose(g, returns_to_go64(ep, 0.99), rtol=2.0 ** -23, atol=0)
    _check_mc(eng, cols, nstep)
    _check_mc(eng, cols, nstep, want_next=True)
    eng.set_obs_normalizer(np.full(O, 0.25, np.float32), np.full(O, 2.0, np.float32))       # the normaliser leaves the column valid
    assert eng.returns_info()[3]
    _check_mc(eng, cols, nstep)
    eng.set_weights('transitions')                                                          # so do the weights
    assert eng.returns_info()[3]


def test_sample_mc_on_a_frame_stacked_arena():
    from exorl_amd.engine import ReplayEngine
    A, k = 3, 3
    eps = _synth.synth_episodes(4, list(MC_LENGTHS), 2 * 8 * 8, A, obs_u8=True)
    eng = ReplayEngine((2 * k, 8, 8), np.uint8, A, 0, sum(MC_LENGTHS) + len(MC_LENGTHS) + 8, 8, frame_stack=k)
    eng.set_order([eng.append_episode(ep) for ep in eps])
    eng.build_returns(0.99)
    cols = eng.returns_to_go()
    for ep, g in zip(eps, cols):
        assert np.allclose(g, returns_to_go64(ep, 0.99), rtol=2.0 ** -23, atol=0)
    for nstep in (1, 3):
        _check_mc(eng, cols, nstep)


def test_philox_draws_do_not_depend_on_the_destination():
    """Two arenas of one seed, one sampled with the destination and one without, three batches each: the same pairs, the same outputs,
    and mc_return is the lookup for the pairs drawn."""
    eps = episodes(False, MC_LENGTHS, 8, 3, seed=7)
    a, _ = arena(eps, O=8, A=3)
    b, _ = arena(eps, O=8, A=3)
    for e in (a, b):
        e.seed_philox(77)
    a.build_returns(0.99)
    cols = a.returns_to_go()
    for _ in range(3):
        got, mc, rec = _sample(a, None, 1, sampler=L().SAMPLER_PHILOX)
        ref, _, rec0 = _sample(b, None, 1, sampler=L().SAMPLER_PHILOX, with_mc=False)
        same_bits(got, ref)
        assert np.array_equal(np.asarray(rec), np.asarray(rec0))
        assert mc.tobytes() == lookup(cols, np.asarray(rec).reshape(-1, 2)).tobytes()


def test_stale_column_and_other_gamma_are_refused():
    """append_episode, evict and set_order each make exorl_replay_sample_mc and exorl_replay_returns_read refuse, launching nothing (the
    destination keeps its NaN); a rebuild heals them. A gamma whose bits differ from the build's is refused; a NULL destination is
    exorl_replay_sample and never refused. An empty order table refuses the build."""
    eps = episodes(False, MC_LENGTHS, 8, 3, seed=7)
    eng, slots = arena(eps, O=8, A=3, spare=64)
    pairs = np.array([[0, 1], [2, 5]], np.int32)
    ExorlError = L().ExorlError
    with pytest.raises(ExorlError, match='no return-to-go column'):
        eng.returns_to_go()
    assert eng.returns_info()[0] is None and not eng.returns_info()[3]

    def refused():
        res, out = eng.alloc_batch(2)
        mc = torch.full((2,), float('nan'), device=eng.device)
        with pytest.raises(ExorlError, match='stale'):
            eng.sample_into(out, 2, 1, 0.99, L().SAMPLER_GIVEN, pairs, mc_return=mc)
        with pytest.raises(ExorlError, match='stale'):
            eng.returns_to_go()
        torch.cuda.synchronize()
        assert torch.isnan(mc).all() and not eng.returns_info()[3]
        eng.sample_into(out, 2, 1, 0.99, L().SAMPLER_GIVEN, pairs)          # without the destination: exorl_replay_sample, as ever

    def healed():
        eng.build_returns(0.99)
        cols = eng.returns_to_go()
        _, mc, _ = _sample(eng, pairs)
        assert mc.tobytes() == lookup(cols, pairs).tobytes()

    refused()
    healed()
    extra = eng.append_episode(_synth.synth_episodes(8, [5], 8, 3)[0])
    refused()
    healed()
    eng.evict(extra)
    refused()
    healed()
    eng.set_order([slots[i] for i in (0, 1, 2, 3)])                          # the same order: still a new table
    refused()
    healed()
    res, out = eng.alloc_batch(2)
    mc = torch.full((2,), float('nan'), device=eng.device)
    for gamma in (float(np.nextafter(np.float32(0.99), np.float32(1.0))), 1.0):
        with pytest.raises(ExorlError, match='the column was built with'):
            eng.sample_into(out, 2, 1, gamma, L().SAMPLER_GIVEN, pairs, mc_return=mc)
    torch.cuda.synchronize()
    assert torch.isnan(mc).all()
    flat = np.zeros(7, np.float32)
    assert L().load().exorl_replay_returns_read(eng.h, flat.ctypes.data, 7, None) != 0 and b'transitions' in L().load().exorl_last_error()
    eng.set_order([])
    with pytest.raises(ExorlError, match='no resident episode'):
        eng.build_returns(0.99)


def test_iterators_build_the_column_on_demand():
    """ArenaIterator.sample_into(mc_return=) builds the column with its own discount on the first request and again once it is stale;
    next() yields what it yielded before."""
    from exorl_amd.replay_buffer import ArenaIterator
    eps = episodes(False, MC_LENGTHS, 8, 3, seed=7)
    eng, _ = arena(eps, O=8, A=3, spare=64)
    eng.seed_philox(5)
    it = ArenaIterator(eng, 16, 1, 0.97, 'philox')
    assert len(next(it)) == 5 and not eng.returns_info()[3]
    res, out = eng.alloc_batch(16)
    mc = torch.full((16,), float('nan'), device=eng.device)
    it.sample_into(out, mc_return=mc)
    torch.cuda.synchronize()
    _, g32, epoch, valid = eng.returns_info()
    assert valid and np.float32(g32) == np.float32(0.97)
    cols = eng.returns_to_go()
    assert all(np.allclose(g, returns_to_go64(ep, 0.97), rtol=2.0 ** -23, atol=0) for ep, g in zip(eps, cols))
    assert mc.cpu().numpy().tobytes() == lookup(cols, np.asarray(eng.last_pairs(16)).reshape(-1, 2)).tobytes()
    it.sample_into(out, mc_return=mc)
    assert eng.returns_info()[2] == epoch                                    # standing: not rebuilt
    slot = eng.append_episode(_synth.synth_episodes(8, [5], 8, 3)[0])
    assert not eng.returns_info()[3]
    it.sample_into(out, mc_return=mc)
    torch.cuda.synchronize()
    assert eng.returns_info()[3] and eng.returns_info()[2] > epoch
    assert mc.cpu().numpy().tobytes() == lookup(eng.returns_to_go(), np.asarray(eng.last_pairs(16)).reshape(-1, 2)).tobytes()
    del slot


def test_device_replay_iterator_carries_the_destination_across_segments(tmp_path):
    """fetch_every = 5 and B = 16: four segments per batch, each writing its slice of mc_return; the shard's column is built on the first
    request with the loader's discount. The action rows name their episode and step (1000 e + t in every column), so the sampled action
    says which value the column holds for the row, whichever sampler drew the pair; the other outputs are next()'s."""
    import random

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
    eng = its[1].shards[0].engine
    assert not eng.returns_info()[3]
    for _ in range(3):
        plain = next(its[0])
        res, out = eng.alloc_batch(B)
        mc = torch.full((B,), float('nan'), device=eng.device)
        its[1].sample_into(out, B, mc_return=mc)
        torch.cuda.synchronize()
        same_bits(plain, res)
        assert eng.returns_info()[3] and np.float32(eng.returns_info()[1]) == np.float32(0.99)
        by_len = {len(g): g for g in eng.returns_to_go()}
        act, got = res[1].cpu().numpy(), mc.cpu().numpy()
        for b in range(B):
            e, idx = int(act[b, 0]) // 1000 - 1, int(act[b, 0]) % 1000
            assert got[b] == by_len[lengths[e]][idx - 1], (b, e, idx)
            assert abs(float(got[b]) - returns_to_go64(eps[e], 0.99)[idx - 1]) <= 2.0 ** -23 * returns_to_go64(eps[e], 0.99)[idx - 1]
