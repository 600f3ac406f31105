"""Frame-stacked replay arena (ReplayEngine(..., frame_stack=k): one frame per row, gather_frames_kernel assembles the stacks) against the
two yardsticks it must equal byte for byte: a plain arena fed the stacked episodes (gather_nstep_kernel) and oracle.replay.gather_nstep on
the stacked episode dicts."""
import numpy as np
import pytest
import torch

from oracle.replay import gather_nstep

pytestmark = pytest.mark.gpu
LENGTHS = [1, 2, 3, 7, 12]            # transitions per episode: lengths below k exercise every clamp depth
SHAPES = {'192B': (3, 8, 8), '36B': (1, 6, 6)}      # one frame: a multiple of 16 bytes (uint4 path) and one that is not (dword path)
A, META = 3, 2


def make_episodes(frame, k, lengths=LENGTHS, seed=0):
    """[(single-frame episode, stacked episode)]: distinct random bytes per frame, a 2-column meta, some terminal discounts."""
    from exorl_amd.replay_buffer import stack_frames
    rs = np.random.RandomState(1000 * seed + 10 * k + frame[1])
    out = []
    for n in lengths:
        rows = n + 1
        ep = dict(observation=rs.randint(0, 256, (rows,) + frame).astype(np.uint8),
                  action=rs.uniform(-1, 1, (rows, A)).astype(np.float32), reward=rs.uniform(0, 1, (rows, 1)).astype(np.float32),
                  discount=(rs.uniform(size=(rows, 1)) > 0.1).astype(np.float32), skill=rs.standard_normal((rows, META)).astype(np.float32))
        out.append((ep, dict(ep, observation=stack_frames(ep['observation'], k))))
    return out


def make_arenas(frame, k, eps, capacity=256, use=None):
    """(frame arena, plain arena over the stacked episodes), the episodes `use` (default all) appended and ordered alike."""
    from exorl_amd.engine import ReplayEngine
    shape = (k * frame[0],) + frame[1:]
    fr = ReplayEngine(shape, np.uint8, A, META, capacity, 16, frame_stack=k)
    pl = ReplayEngine(shape, np.uint8, A, META, capacity, 16)
    assert fr.frame_bytes * k == fr.obs_bytes == pl.obs_bytes and pl.frame_bytes == pl.obs_bytes
    use = range(len(eps)) if use is None else use
    fr.set_order([fr.append_episode(eps[i][0], ('skill',)) for i in use])
    pl.set_order([pl.append_episode(eps[i][1], ('skill',)) for i in use])
    return fr, pl


def same_bytes(got, want, what=''):
    assert len(got) == len(want) == 6
    for name, g, w in zip(('obs', 'action', 'reward', 'discount', 'next_obs', 'meta'), got, want):
        g = g.cpu().numpy() if torch.is_tensor(g) else np.asarray(g)
        w = w.cpu().numpy() if torch.is_tensor(w) else np.asarray(w)
        assert g.dtype == w.dtype and g.size == w.size, (what, name, g.shape, w.shape)
        assert np.array_equal(np.ascontiguousarray(g).reshape(-1).view(np.uint8), np.ascontiguousarray(w).reshape(-1).view(np.uint8)), (what, name)


# ---- 1. every valid pair ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nstep', [1, 3])
@pytest.mark.parametrize('k', [2, 3, 4])
@pytest.mark.parametrize('size', list(SHAPES))
def test_every_valid_pair_is_bit_exact(size, k, nstep):
    from exorl_amd import _lib as L
    frame = SHAPES[size]
    eps = make_episodes(frame, k)
    fr, pl = make_arenas(frame, k, eps)
    pairs = np.array([[p, idx] for p, n in enumerate(LENGTHS) for idx in range(1, n - nstep + 2)], np.int32)
    assert len(pairs) == sum(max(n - nstep + 1, 0) for n in LENGTHS) and len(pairs) > 4       # more than one block of four waves
    got = fr.sample(len(pairs), nstep, 0.99, L.SAMPLER_GIVEN, pairs=pairs)
    same_bytes(got, pl.sample(len(pairs), nstep, 0.99, L.SAMPLER_GIVEN, pairs=pairs), 'plain arena')
    cols = [gather_nstep(eps[p][1], idx, nstep, 0.99, ('skill',)) for p, idx in pairs]
    same_bytes(got, [np.stack([c[j] for c in cols]) for j in range(6)], 'oracle')
    assert got[0].shape == (len(pairs), k * frame[0]) + frame[1:]


# ---- 2. / 3. the samplers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nstep', [1, 3])
@pytest.mark.parametrize('size', list(SHAPES))
@pytest.mark.parametrize('mode', ['philox', 'philox_weighted', 'mt19937'])
def test_samplers_draw_and_gather_alike(mode, size, nstep):
    from exorl_amd import _lib as L
    frame, k, B = SHAPES[size], 3, 64
    eps = make_episodes(frame, k)
    weighted = mode == 'philox_weighted'
    use = list(range(len(LENGTHS))) if weighted else [i for i, n in enumerate(LENGTHS) if n >= nstep]      # weighted: short episodes have mass 0
    fr, pl = make_arenas(frame, k, eps, use=use)
    sampler = L.SAMPLER_MT19937 if mode == 'mt19937' else L.SAMPLER_PHILOX
    for eng in (fr, pl):
        if weighted:
            eng.set_weights('transitions', [3.0, 0.5, 1.0, 2.0, 0.25])
        eng.seed_mt_ints(5, 5) if mode == 'mt19937' else eng.seed_philox(20241)
    seen = set()
    for batch in range(4):
        got, want = fr.sample(B, nstep, 0.99, sampler), pl.sample(B, nstep, 0.99, sampler)
        pf, pp = fr.last_pairs(B), pl.last_pairs(B)
        assert np.array_equal(pf, pp), batch
        same_bytes(got, want, batch)
        cols = [gather_nstep(eps[use[p]][1], idx, nstep, 0.99, ('skill',)) for p, idx in pf]
        same_bytes(got, [np.stack([c[j] for c in cols]) for j in range(6)], ('oracle', batch))
        seen |= {int(p) for p in pf[:, 0]}
    assert len(seen) == sum(1 for i in use if LENGTHS[i] >= nstep)         # every sampleable episode came up


# ---- 4. strided outputs -------------------------------------------------------------------------------------------------------------------
def _strided_out(L, B, obs_stride, dev='cuda'):
    bufs = dict(obs=torch.full((B, obs_stride), 0xA5, dtype=torch.uint8, device=dev), nobs=torch.full((B, obs_stride), 0xA5, dtype=torch.uint8, device=dev),
                act=torch.zeros(B, A, device=dev), rew=torch.zeros(B, 1, device=dev), disc=torch.zeros(B, 1, device=dev), meta=torch.zeros(B, META, device=dev))
    out = L.BatchOut(bufs['obs'].data_ptr(), obs_stride, bufs['act'].data_ptr(), A, bufs['rew'].data_ptr(), bufs['disc'].data_ptr(),
                     bufs['nobs'].data_ptr(), obs_stride, bufs['meta'].data_ptr(), META)
    return bufs, out


@pytest.mark.parametrize('size', list(SHAPES))
def test_strided_outputs_and_the_stride_check(size):
    from exorl_amd import _lib as L
    frame, k, nstep = SHAPES[size], 3, 3
    eps = make_episodes(frame, k)
    fr, pl = make_arenas(frame, k, eps)
    pairs = np.array([[p, idx] for p, n in enumerate(LENGTHS) for idx in range(1, n - nstep + 2)], np.int32)
    B, ob = len(pairs), fr.obs_bytes
    want = pl.sample(B, nstep, 0.99, L.SAMPLER_GIVEN, pairs=pairs)
    bufs, out = _strided_out(L, B, ob + 64)
    fr.sample_into(out, B, nstep, 0.99, L.SAMPLER_GIVEN, pairs=pairs)
    for got, ref in ((bufs['obs'], want[0]), (bufs['nobs'], want[4])):
        got = got.cpu().numpy()
        assert np.array_equal(got[:, :ob], ref.cpu().numpy().reshape(B, ob))
        assert np.all(got[:, ob:] == 0xA5)                                   # the 64 padding bytes of every sample are untouched
    same_bytes([want[0], bufs['act'], bufs['rew'], bufs['disc'], want[4], bufs['meta']], want)
    for short_obs, short_next in ((ob - 4, ob), (ob, ob - 4), (fr.frame_bytes, fr.frame_bytes)):
        bufs, out = _strided_out(L, B, ob)
        out.obs_stride, out.next_obs_stride = short_obs, short_next
        with pytest.raises(L.ExorlError, match='stride'):
            fr.sample_into(out, B, nstep, 0.99, L.SAMPLER_GIVEN, pairs=pairs)
        torch.cuda.synchronize()
        assert bool((bufs['obs'] == 0xA5).all()) and bool((bufs['nobs'] == 0xA5).all()) and not bool(bufs['act'].any())      # nothing was launched


# ---- 5. compaction ------------------------------------------------------------------------------------------------------------------------
def test_compaction_moves_frame_rows_like_whole_rows():
    from exorl_amd import _lib as L
    from exorl_amd.engine import ReplayEngine
    frame, k, nstep = SHAPES['192B'], 3, 2
    lengths = [9, 5, 7, 6, 8, 4]
    eps = make_episodes(frame, k, lengths, seed=2)
    engines = [ReplayEngine((9, 8, 8), np.uint8, A, META, 40, 8, frame_stack=k), ReplayEngine((9, 8, 8), np.uint8, A, META, 40, 8)]
    live = [0, 3, 4, 5]
    pairs = np.array([[p, 1 + (j % (lengths[live[p]] - 1))] for j in range(16) for p in range(4)], np.int32)
    outs = []
    for which, eng in enumerate(engines):                      # 45 rows needed in total in 40: eviction, then an append that compacts
        slots = [eng.append_episode(eps[i][which], ('skill',)) for i in range(4)]       # 10 + 6 + 8 + 7 = 31 rows
        eng.evict(slots[1]); eng.evict(slots[2])
        slots.append(eng.append_episode(eps[4][which], ('skill',)))                      # 9 rows -> 40 used
        slots.append(eng.append_episode(eps[5][which], ('skill',)))                      # 5 rows: does not fit -> compaction
        assert eng.num_rows() == (31, 31)
        eng.set_order([slots[0], slots[3], slots[4], slots[5]])
        outs.append(eng.sample(len(pairs), nstep, 0.99, L.SAMPLER_GIVEN, pairs=pairs))
    same_bytes(outs[0], outs[1])
    cols = [gather_nstep(eps[live[p]][1], idx, nstep, 0.99, ('skill',)) for p, idx in pairs]
    same_bytes(outs[0], [np.stack([c[j] for c in cols]) for j in range(6)], 'oracle')


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from exorl_amd import _lib as L
    from exorl_amd.engine import AgentEngine, ReplayEngine
    frame, k = SHAPES['36B'], 2
    eps = make_episodes(frame, k)
    eng = ReplayEngine((2, 6, 6), np.uint8, A, META, 64, 8)
    for bad in (0, 17, -1):
        with pytest.raises(L.ExorlError, match='frames='):
            eng.set_frame_stack(bad)
    eng.set_frame_stack(16)
    eng.set_frame_stack(1)                                   # allowed any number of times while the arena is untouched
    slot = eng.append_episode(eps[3][1], ('skill',))
    with pytest.raises(L.ExorlError, match='slots already'):
        eng.set_frame_stack(2)
    eng.evict(slot)
    with pytest.raises(L.ExorlError, match='slots already'):      # "has ever been handed out": an emptied arena stays refused
        eng.set_frame_stack(2)
    # a state agent's captured step reads whole arena rows: refused even when the sampled bytes fit its observation
    O, H, B = 12, 256, 128
    rs = np.random.RandomState(0)
    st = ReplayEngine((2, 2, 3), np.float32, A, 0, 64, 8, frame_stack=2)
    assert st.obs_bytes == O * 4 and st.frame_bytes == O * 2
    ep = dict(observation=rs.standard_normal((9, 1, 2, 3)).astype(np.float32), action=rs.uniform(-1, 1, (9, A)).astype(np.float32),
              reward=np.ones((9, 1), np.float32), discount=np.ones((9, 1), np.float32))
    st.set_order([st.append_episode(ep)])
    st.seed_philox(1)
    agent = AgentEngine('td3_bc', O, A, H, B)
    with pytest.raises(L.ExorlError, match='frames per observation'):
        agent.enable_graph(st, 1, 0.99, 0.2)
    obs = st.sample(B, 1, 0.99, L.SAMPLER_PHILOX)[0]         # the eager path serves the same arena
    assert obs.shape == (B, 2, 2, 3)


# ---- 7. loaders ---------------------------------------------------------------------------------------------------------------------------
def test_loaders_dedup_files_and_hand_off_alike(tmp_path):
    from exorl_amd.replay_buffer import ReplayBufferStorage, make_offline_replay_loader, make_replay_loader, save_episode
    lengths, B, nstep = [5, 9, 3, 12, 7, 4], 16, 3
    eps = [{key: v for key, v in stacked.items() if key != 'skill'} for _, stacked in make_episodes((3, 16, 16), 3, lengths, 7)]
    assert eps[0]['observation'].shape == (6, 9, 16, 16)
    its = {}
    for name, fs in (('frames', dict(frame_stack=3)), ('plain', {})):
        live = ReplayBufferStorage((), (), tmp_path / name)
        for ep in eps:
            live._store_episode(ep)                            # on disk in the reference's stacked format, and in storage._fresh
        cold = ReplayBufferStorage((), (), tmp_path / name)    # another process' view: files only
        assert len(live._fresh) == len(eps) and len(cold._fresh) == 0
        for path, st in (('hand-off', live), ('files', cold)):
            its[name, path] = iter(make_replay_loader(st, 10 ** 6, B, 0, True, nstep, 0.99, sampler='mt19937', seed=4, **fs))
    for batch in range(20):
        got = {key: next(it) for key, it in its.items()}
        for key in (('frames', 'files'), ('plain', 'hand-off'), ('plain', 'files')):
            for x, y in zip(got['frames', 'hand-off'], got[key]):
                assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), (batch, key)
    assert got['frames', 'files'][0].shape == (B, 9, 16, 16)
    for (name, path), it in its.items():
        eng = it.shards[0].engine
        assert eng.obs_bytes == 9 * 16 * 16 and eng.frame_bytes * (3 if name == 'frames' else 1) == eng.obs_bytes
    offline = [iter(make_offline_replay_loader(None, tmp_path / 'frames', 10 ** 6, B, 1, 0.99, sampler='mt19937', seed=4, **fs))
               for fs in (dict(frame_stack=3), {})]
    for batch in range(5):
        for x, y in zip(next(offline[0]), next(offline[1])):
            assert x.shape == y.shape and torch.equal(x, y), batch
    eng = offline[0].shards[0].engine
    assert eng.frame_bytes * 3 == eng.obs_bytes and offline[1].shards[0].engine.frame_bytes == eng.obs_bytes
    # an episode that is no sliding window cannot be stored one frame per row: refused at ingest, not guessed at
    d = tmp_path / 'spliced'
    d.mkdir()
    bad = dict(eps[1], observation=eps[1]['observation'].copy())
    bad['observation'][4, 0] ^= 1
    save_episode(bad, d / 'episode_0_9.npz')
    for make in (lambda: make_replay_loader(ReplayBufferStorage((), (), d), 10 ** 6, B, 0, True, nstep, 0.99, frame_stack=3),
                 lambda: make_offline_replay_loader(None, d, 10 ** 6, B, 1, 0.99, frame_stack=3)):
        with pytest.raises(ValueError, match='row 4 does not continue row 3'):
            next(iter(make()))


# ---- 8. 64-bit offsets --------------------------------------------------------------------------------------------------------------------
def test_frame_arena_past_4_gib_is_addressed_with_64_bit_offsets():
    """The arena of test_pixel_arena_past_4_gib_is_addressed_with_64_bit_offsets (4.7 GB of (3, 84, 84) frames whose bytes are a function of
    their global row), read as k = 3 stacks: pairs in the episodes past the 2^31- and 2^32-byte marks, and one pair whose three frames
    lie before, across and after byte offset 2^32, against stacks built on the host from the same formula."""
    from exorl_amd import _lib as L
    from exorl_amd.engine import ReplayEngine
    OB, T, E, nstep, k = 3 * 84 * 84, 250, 880, 3, 3
    rows = E * (T + 1)
    assert rows * OB > (1 << 32) + (1 << 28)
    eng = ReplayEngine((9, 84, 84), np.uint8, 2, 0, rows + 8, E + 4, frame_stack=k)
    assert eng.frame_bytes == OB
    base = (np.arange(OB) % 251).astype(np.uint8)

    def frames(r):           # frames of the global rows r: base + (37 r + (r >> 8)) mod 256
        r = np.asarray(r, np.int64)
        off = ((37 * r + (r >> 8)) & 255).astype(np.uint8)
        return (base[None, :] + off[:, None]).reshape(len(r), 3, 84, 84)
    slots = []
    one = np.ones((T + 1, 1), np.float32)
    for e in range(E):
        slots.append(eng.append_episode(dict(observation=frames(np.arange(e * (T + 1), (e + 1) * (T + 1))), action=np.tile(np.float32([e, 0.5]), (T + 1, 1)),
                                             reward=one, discount=one)))
    eng.set_order(slots)
    cut = (1 << 32) // OB                                    # the global row that holds byte 2^32
    e_cut, t_cut = divmod(cut, T + 1)
    assert cut * OB < (1 << 32) < (cut + 1) * OB and 1 <= t_cut and t_cut + 1 + nstep <= T
    picks = [0, (1 << 31) // (OB * (T + 1)) + 1, (1 << 32) // (OB * (T + 1)) + 1, E - 1]
    pairs = np.array([[e, idx] for e in picks for idx in (1, 2, 17, T - nstep + 1)] + [[e_cut, t_cut + 2], [e_cut, t_cut + 2 - nstep]], np.int32)
    obs, act, rew, disc, nobs = eng.sample(len(pairs), nstep, 0.99, L.SAMPLER_GIVEN, pairs=pairs)
    for b, (e, idx) in enumerate(pairs):
        for got, t in ((obs, idx - 1), (nobs, idx + nstep - 1)):
            want = frames(e * (T + 1) + np.maximum(t - (k - 1) + np.arange(k), 0)).reshape(9, 84, 84)
            assert np.array_equal(got[b].cpu().numpy(), want), (e, idx, t)
        assert float(act[b, 0]) == e


# ---- 9. end to end ------------------------------------------------------------------------------------------------------------------------
def test_pixel_ddpg_trains_alike_from_either_arena():
    """Two DDPG agents on (9, 64, 64) pixels, one fed by the frame arena and one by the stacked arena through the zero-copy batch slots,
    same Philox seed, same augmentation and noise draws: three updates leave identical metrics and identical weights."""
    import _synth
    from exorl_amd.engine import ReplayEngine
    from exorl_amd.replay_buffer import ArenaIterator, stack_frames
    from test_gpu_pixels import load_pixel_params, make_pixel_agent
    C_, HW, Ad, F, H, B, k, nstep = 9, 64, 4, 50, 256, 16, 3, 3
    rs = np.random.RandomState(11)
    eps = []
    for n in (6, 9, 4):
        ep = dict(observation=rs.randint(0, 256, (n + 1, 3, HW, HW)).astype(np.uint8), action=rs.uniform(-1, 1, (n + 1, Ad)).astype(np.float32),
                  reward=rs.uniform(0, 1, (n + 1, 1)).astype(np.float32), discount=np.ones((n + 1, 1), np.float32))
        eps.append((ep, dict(ep, observation=stack_frames(ep['observation'], k))))
    shifts = [rs.randint(0, 9, (B, 2)).astype(np.int32) for _ in range(6)]
    results = []
    for which in (0, 1):
        eng = ReplayEngine((C_, HW, HW), np.uint8, Ad, 0, 64, 8, **(dict(frame_stack=k) if which == 0 else {}))
        eng.set_order([eng.append_episode(ep[which]) for ep in eps])
        eng.seed_philox(77)
        ag = make_pixel_agent(C_, HW, Ad, F, H, B)
        load_pixel_params(ag, C_, Ad, F, H, 32 * ((HW - 3) // 2 + 1 - 6) ** 2)
        ag.noise_hook = _synth.NoiseStream(4).draw
        todo = list(shifts)
        ag.shift_hook = lambda n: todo.pop(0)
        it = ArenaIterator(eng, B, nstep, 0.99, 'philox')
        metrics = [ag.update(it, 2 * i) for i in range(3)]
        params = [p.detach().cpu().numpy().copy() for net in (ag.actor, ag.critic, ag.encoder) for p in net.parameters()]
        results.append((metrics, params, eng.last_pairs(B)))
        assert not todo
    (m0, p0, pairs0), (m1, p1, pairs1) = results
    assert np.array_equal(pairs0, pairs1)
    assert m0 == m1 and all(len(m) > 0 for m in m0)
    assert len(p0) == len(p1) and all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(p0, p1))
