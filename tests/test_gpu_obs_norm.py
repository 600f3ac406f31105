"""GPU checks of observation normalisation in the HBM replay: the two-launch column moments against float64 two-pass numpy (bounds and
data: tests/_obs_norm.py), the normalising gather bit for bit against normalize_obs of the raw gather, the reference's recorded offline
batches through make_replay_loader(normalize_obs=True), shards and injected rank partials, the captured step on a normalised arena
against a pre-normalised one, act(), pickling and train_offline(normalize_obs=True)."""
import ctypes as C
import pickle
import random

import numpy as np
import pytest
import torch

import _obs_norm as N

pytestmark = pytest.mark.gpu


def fill(eps, O, A, meta_dim=0, spare_rows=64, max_episodes=32):
    from exorl_amd.engine import ReplayEngine
    eng = ReplayEngine((O,), np.float32, A, meta_dim, sum(len(ep['observation']) for ep in eps) + spare_rows, max_episodes)
    slots = [eng.append_episode(ep, ('skill',) if meta_dim else ()) for ep in eps]
    eng.set_order(slots)
    return eng, slots


# ---- 1. moments -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('O', [1, 3, 24, 65, 78, 300])      # 300: more than one 256-column tile per workgroup
def test_moments_against_float64_two_pass(O):
    eps = N.norm_episodes(100 + O, N.LENGTHS, O, 2)
    eng, slots = fill(eps, O, 2, spare_rows=20)
    first = eng.obs_moments()
    N.check_moments(first, N.moments_of(eps), f'O={O} full')
    assert first[1].shape == (O,) and first[1].dtype == np.float64 and first[0] == eng.num_rows()[0]
    eng.evict(slots[3])                                         # a hole in the middle of the arena: its rows are not read
    live = eps[:3] + eps[4:]
    holed = eng.obs_moments()
    N.check_moments(holed, N.moments_of(live), f'O={O} hole')
    assert eng.num_rows() == (sum(N.LENGTHS) + 7 - 64, sum(N.LENGTHS) + 7)
    new = N.norm_episodes(200 + O, [29], O, 2)[0]
    slots[3] = eng.append_episode(new)                          # 30 rows into 20 spare ones: the arena compacts first
    assert eng.num_rows()[0] == eng.num_rows()[1]
    eng.set_order(slots)
    got = eng.obs_moments()
    N.check_moments(got, N.moments_of(eps[:3] + [new] + eps[4:]), f'O={O} compacted')
    assert got[0] == eng.num_rows()[0]
    again = eng.obs_moments()                                   # no atomics, a fixed merge order: the same bits
    assert again[0] == got[0] and np.array_equal(N.bits(again[1]), N.bits(got[1])) and np.array_equal(N.bits(again[2]), N.bits(got[2]))
    eng.set_order(slots[:2])                                    # the order table, not the arena, says which episodes count
    N.check_moments(eng.obs_moments(), N.moments_of(eps[:2]), f'O={O} two episodes')


def test_moments_with_several_items_per_workgroup():
    """More than 1024 work items of 64 rows: a workgroup owns several, and its range runs across episode boundaries."""
    lengths = [99, 130, 64] * 240                                # 2 + 3 + 2 items per triple: 1680 items, two per workgroup
    eps = N.norm_episodes(300, lengths, 3, 2)
    eng, _ = fill(eps, 3, 2, max_episodes=len(eps) + 8)
    got = eng.obs_moments()
    N.check_moments(got, N.moments_of(eps), 'O=3, 1680 items')
    again = eng.obs_moments()
    assert np.array_equal(N.bits(again[1]), N.bits(got[1])) and np.array_equal(N.bits(again[2]), N.bits(got[2]))


def test_moments_refusals():
    from exorl_amd import _lib as L
    from exorl_amd.engine import ReplayEngine
    lib = L.load()
    eng, _ = fill(N.norm_episodes(1, [5, 9], 3, 2), 3, 2)
    cnt, mean, m2 = C.c_int64(-7), np.full(8, 5.0), np.full(8, 5.0)
    for n in (2, 4, 0, -3):                                     # n_cols * 4 != obs_bytes
        assert lib.exorl_replay_obs_moments(eng.h, n, C.byref(cnt), mean.ctypes.data, m2.ctypes.data, None) != 0
        assert b'n_cols' in lib.exorl_last_error()
    assert cnt.value == -7 and np.all(mean == 5.0) and np.all(m2 == 5.0)
    empty = ReplayEngine((3,), np.float32, 2, 0, 64, 8)
    with pytest.raises(L.ExorlError, match='no resident episode'):
        empty.obs_moments()
    eng.set_order([])                                           # resident rows, none of them in the table
    with pytest.raises(L.ExorlError, match='no resident episode'):
        eng.obs_moments()
    stacked = ReplayEngine((6, 4, 4), np.float32, 2, 0, 64, 8, frame_stack=3)
    with pytest.raises(L.ExorlError, match='frame'):
        stacked.obs_moments()
    with pytest.raises(L.ExorlError, match='frame'):
        stacked.set_obs_normalizer(np.zeros(96, np.float32), np.ones(96, np.float32))
    with pytest.raises(ValueError, match='float32'):
        ReplayEngine((9, 8, 8), np.uint8, 2, 0, 64, 8).obs_moments()
    with pytest.raises(ValueError, match='columns'):
        eng.set_obs_normalizer(np.zeros(4, np.float32), np.ones(4, np.float32))
    assert lib.exorl_replay_set_obs_norm(eng.h, 2, mean.ctypes.data, mean.ctypes.data, None) != 0 and b'n_cols' in lib.exorl_last_error()


# ---- 2. the gather, bit for bit -------------------------------------------------------------------------------------------------------
def edge_pairs(lengths, nstep, B, seed):
    """The first and the last valid start of every episode that holds nstep transitions, then random valid pairs up to B."""
    ok = [i for i, n in enumerate(lengths) if n >= nstep]
    pairs = [(i, s) for i in ok for s in (1, lengths[i] - nstep + 1)]
    rs = np.random.RandomState(seed)
    while len(pairs) < B:
        i = ok[int(rs.randint(len(ok)))]
        pairs.append((i, int(rs.randint(1, lengths[i] - nstep + 2))))
    return np.array(pairs[:B], np.int32)


def sample_strided(eng, B, nstep, pairs, O, A, M, pad):
    """eng.sample with obs / next_obs rows `pad` floats wider than an observation: tensors prefilled with a sentinel."""
    from exorl_amd import _lib as L
    dev = eng.device
    obs, nobs = (torch.full((B, O + pad), -77.0, dtype=torch.float32, device=dev) for _ in range(2))
    act = torch.empty(B, A, dtype=torch.float32, device=dev)
    rew, disc = (torch.empty(B, 1, dtype=torch.float32, device=dev) for _ in range(2))
    meta = torch.empty(B, M, dtype=torch.float32, device=dev) if M else None
    out = L.BatchOut(obs.data_ptr(), (O + pad) * 4, act.data_ptr(), A, rew.data_ptr(), disc.data_ptr(), nobs.data_ptr(), (O + pad) * 4,
                     L.ptr(meta), M)
    eng.sample_into(out, B, nstep, 0.99, L.SAMPLER_GIVEN, pairs)
    if pad:
        assert bool((obs[:, O:] == -77.0).all()) and bool((nobs[:, O:] == -77.0).all())
    return (obs[:, :O].contiguous(), act, rew, disc, nobs[:, :O].contiguous()) + ((meta,) if M else ())


@pytest.mark.parametrize('O,nstep,meta_dim,pad', [(1, 1, 0, 0), (1, 3, 0, 0), (24, 1, 0, 0), (24, 3, 2, 0), (24, 1, 0, 4), (65, 1, 2, 0),
                                                 (65, 3, 0, 0), (65, 3, 0, 3)])
def test_gather_equals_normalize_obs_of_the_raw_gather(O, nstep, meta_dim, pad):
    """O = 24 with 16-byte strides takes the 16-byte path, O = 1 and 65 the 4-byte one; pad: output rows wider than an observation."""
    A, B = 2, 13
    lengths = [nstep, 5, 64, 17, 1]                             # an episode of exactly nstep transitions; one too short for nstep = 3
    eps = N.norm_episodes(7 * O + nstep, lengths, O, A, meta_dim)
    eng, _ = fill(eps, O, A, meta_dim)
    pairs = edge_pairs(lengths, nstep, B, O)
    draw = lambda: [t.cpu().numpy() for t in sample_strided(eng, B, nstep, pairs, O, A, meta_dim, pad)]
    raw = draw()
    rows0 = np.cumsum([0] + [n + 1 for n in lengths])
    cat = np.concatenate([ep['observation'] for ep in eps])
    at = rows0[pairs[:, 0]] + pairs[:, 1]
    assert np.array_equal(raw[0], cat[at - 1]) and np.array_equal(raw[4], cat[at + nstep - 1])
    mean32, inv32 = N.normalizer(*N.moments_of(eps))
    eng.set_obs_normalizer(mean32, inv32)
    got = draw()
    for ti in (0, 4):
        assert np.array_equal(N.bits(got[ti]), N.bits(N.normalize(raw[ti], mean32, inv32))), ti
        assert not np.array_equal(got[ti], raw[ti])
    for ti in [1, 2, 3] + ([5] if meta_dim else []):            # action, reward, discount, meta: untouched
        assert np.array_equal(N.bits(got[ti]), N.bits(raw[ti])), ti
    assert np.array_equal(eng.last_pairs(B), pairs)
    m2, w2 = (mean32 * np.float32(0.5) + np.float32(0.125)), (inv32 * np.float32(3.0))
    eng.set_obs_normalizer(m2, w2)                              # new values, in place
    got = draw()
    for ti in (0, 4):
        assert np.array_equal(N.bits(got[ti]), N.bits(N.normalize(raw[ti], m2, w2))), ti
    eng.clear_obs_normalizer()
    back = draw()
    for a, b in zip(back, raw):
        assert np.array_equal(N.bits(a), N.bits(b))


@pytest.mark.parametrize('O', [24, 65])
def test_philox_batch_is_normalize_obs_at_the_recorded_pairs(O):
    from exorl_amd import _lib as L
    A, B, nstep = 2, 13, 3
    lengths = [3, 5, 64, 17]
    eps = N.norm_episodes(O, lengths, O, A)
    eng, _ = fill(eps, O, A)
    mean32, inv32 = N.normalizer(*N.moments_of(eps))
    eng.set_obs_normalizer(mean32, inv32)
    eng.seed_philox(12)
    got = [t.cpu().numpy() for t in eng.sample(B, nstep, 0.99, L.SAMPLER_PHILOX)]
    pairs = eng.last_pairs(B)
    eng.clear_obs_normalizer()
    raw = [t.cpu().numpy() for t in eng.sample(B, nstep, 0.99, L.SAMPLER_GIVEN, pairs=pairs)]
    for ti in (0, 4):
        assert np.array_equal(N.bits(got[ti]), N.bits(N.normalize(raw[ti], mean32, inv32)))
    for ti in (1, 2, 3):
        assert np.array_equal(N.bits(got[ti]), N.bits(raw[ti]))
    eng.seed_philox(12)                                         # the draw itself does not depend on the normaliser
    eng.sample(B, nstep, 0.99, L.SAMPLER_PHILOX)
    assert np.array_equal(eng.last_pairs(B), pairs)


# ---- 3. the reference's recorded offline batches ------------------------------------------------------------------------------------------
def test_reference_offline_batches_normalised(gold, tmp_path):
    from exorl_amd.replay_buffer import make_replay_loader, save_episode
    from test_oracle_replay import offline_episodes
    z = np.load(gold / 'replay_offline_a.npz')
    O, A, P, max_size, B, NB, seed, relabel = [int(x) for x in z['dims']]
    eps, lengths = offline_episodes(z)
    d = tmp_path / 'buffer'
    d.mkdir()
    for i, ep in enumerate(eps):
        save_episode(ep, d / f'episode_{i}_{lengths[i]}.npz')
    loader = make_replay_loader(None, d, max_size, B, 0, 0.99, relabel=False, sampler='mt19937', normalize_obs=True)
    random.seed(seed)
    np.random.seed(seed)
    it = iter(loader)
    batches = [[t.cpu().numpy() for t in next(it)] for _ in range(NB)]
    resident = [eps[int(fn.stem.split('_')[1])] for fn in it.shards[0].fns]
    assert [int(fn.stem.split('_')[1]) for fn in it.shards[0].fns] == list(z['resident'])
    mean32, inv32 = N.normalizer(*N.moments_of(resident))
    assert np.array_equal(N.bits(it.obs_normalizer[0]), N.bits(mean32)) and np.array_equal(N.bits(it.obs_normalizer[1]), N.bits(inv32))
    for bi, batch in enumerate(batches):
        assert len(batch) == 5
        for ti in (0, 4):
            assert np.array_equal(N.bits(batch[ti]), N.bits(N.normalize(z[f'batch{bi}_{ti}'], mean32, inv32))), (bi, ti)
        for ti in (1, 2, 3):
            assert np.array_equal(N.bits(batch[ti]), N.bits(z[f'batch{bi}_{ti}'])), (bi, ti)


# ---- 4. shards and ranks ------------------------------------------------------------------------------------------------------------------
def write_dir(d, eps, first=0):
    from exorl_amd.replay_buffer import save_episode
    d.mkdir()
    for i, ep in enumerate(eps):
        save_episode({k: v for k, v in ep.items()}, d / f'episode_{first + i}_{len(ep["observation"]) - 1}.npz')
    return d


def shard_raw_and_sampled(shard, B):
    """One GIVEN batch of a shard's arena as it is configured, and the same pairs with the normaliser off (then put back)."""
    from exorl_amd import _lib as L
    n = len(shard.fns)
    pairs = np.array([(i % n, 1) for i in range(B)], np.int32)
    got = shard.engine.sample(B, 1, 0.99, L.SAMPLER_GIVEN, pairs=pairs)[0].cpu().numpy()
    eps = [shard.loader_eps[int(fn.stem.split('_')[1])] for fn in shard.fns]
    return got, np.stack([eps[i]['observation'][0] for i, _ in pairs])


def test_two_shards_in_one_process_share_one_normaliser(tmp_path):
    from exorl_amd.replay_buffer import make_offline_replay_loader
    O, A, B = 24, 2, 8
    eps = N.norm_episodes(31, [9, 4, 12, 7, 5], O, A)
    d = write_dir(tmp_path / 'buffer', eps)
    it = iter(make_offline_replay_loader(None, d, 10 ** 6, B, 2, 0.99, sampler='philox', seed=3, normalize_obs=True))
    mean32, inv32 = it.obs_normalizer
    want = N.normalizer(*N.moments_of(eps))
    assert np.array_equal(N.bits(mean32), N.bits(want[0])) and np.array_equal(N.bits(inv32), N.bits(want[1]))
    assert len(it.shards) == 2 and [len(s.fns) for s in it.shards] == [3, 2]
    for shard in it.shards:                                     # both arenas carry the statistic of ALL episodes, not of their own
        shard.loader_eps = eps
        got, raw = shard_raw_and_sampled(shard, B)
        assert np.array_equal(N.bits(got), N.bits(N.normalize(raw, mean32, inv32)))
    batch = next(it)                                            # and the iterator's own batches come out normalised
    assert batch[0].shape == (B, O) and abs(float(batch[0][:, 0].mean())) < 10.0       # column 0 is 1000 + 0.01 N(0,1) raw


def test_injected_rank_partials_give_the_normaliser_of_the_union(tmp_path):
    from exorl_amd.replay_buffer import make_offline_replay_loader
    O, A, B = 24, 2, 8
    eps = N.norm_episodes(32, [9, 4, 12, 7, 5, 30], O, A)
    own_eps, other_eps = eps[:4], eps[4:]
    for e in other_eps:
        e['observation'][:, 1] += np.float32(3.0)               # the other rank's data has another mean
    d = write_dir(tmp_path / 'buffer', own_eps)
    seen = []

    def gather(own):
        seen.append(own)
        return [own, [N.moments_of(other_eps[:1]), N.moments_of(other_eps[1:])]]

    it = iter(make_offline_replay_loader(None, d, 10 ** 6, B, 1, 0.99, sampler='philox', seed=3, normalize_obs=True, gather=gather))
    mean32, inv32 = it.obs_normalizer
    assert len(seen) == 1 and len(seen[0]) == 1 and seen[0][0][0] == sum(len(e['observation']) for e in own_eps)
    want = N.normalizer(*N.moments_of(eps))
    assert np.array_equal(N.bits(mean32), N.bits(want[0])) and np.array_equal(N.bits(inv32), N.bits(want[1]))
    own_only = N.normalizer(*N.moments_of(own_eps))
    assert not np.array_equal(mean32, own_only[0])
    it.shards[0].loader_eps = own_eps
    got, raw = shard_raw_and_sampled(it.shards[0], B)
    assert np.array_equal(N.bits(got), N.bits(N.normalize(raw, mean32, inv32)))
    assert it.engine is it.shards[0].engine                      # what enable_graph is handed already carries it


# ---- 5. the captured step ---------------------------------------------------------------------------------------------------------------
O5, A5, H5, B5 = 5, 2, 32, 8


def make_agent(kind, seed=3):
    from exorl_amd import agents
    torch.manual_seed(seed)
    if kind == 'td3_bc':
        return agents.TD3BCAgent('td3_bc', (O5,), (A5,), 'cuda', 1e-4, H5, 0.01, 0.2, 1, B5, 0.3, False, 2.5, precision='fp32')
    if kind == 'bc':
        return agents.BCAgent('bc', (O5,), (A5,), 'cuda', 1e-4, H5, B5, 0.2, False, precision='fp32')
    return agents.CQLAgent('cql', (O5,), (A5,), 'cuda', 1e-4, H5, 0.01, 1, B5, False, 0.01, 3, 5.0, False, precision='fp32')


def arena_iter(eps, norm=None):
    from exorl_amd.replay_buffer import ArenaIterator
    eng, _ = fill(eps, O5, A5)
    eng.seed_philox(77)
    if norm is not None:
        eng.set_obs_normalizer(*norm)
    return eng, ArenaIterator(eng, B5, 1, 0.99, 'philox')


def state_of(ag):
    from exorl_amd import _lib as L
    eng = ag.engine
    out = []
    for net in [L.NET_ACTOR] + ([L.NET_CRITIC, L.NET_CRITIC_TARGET] if eng.has_critic else []):
        for what in ([L.T_PARAM] if net == L.NET_CRITIC_TARGET else [L.T_PARAM, L.T_ADAM_M, L.T_ADAM_V]):
            out.append(((net, what), eng.flat(net, what).clone()))
    return out


def assert_same_state(a, b):
    for (ka, ta), (kb, tb) in zip(state_of(a), state_of(b)):
        assert ka == kb and torch.equal(ta, tb), ka


@pytest.mark.parametrize('kind', ['td3_bc', 'bc'])
def test_captured_step_on_a_normalised_arena(kind):
    """Graph on the normalised arena N == graph on the host-normalised arena P == eager on N, every parameter, Adam and target buffer
    bit for bit (graph == eager is asserted with torch.equal for both agents by test_gpu_agent.py::test_hip_graph_step_equals_eager)."""
    from exorl_amd import _lib as L
    eps = N.norm_episodes(55, [40, 25, 33], O5, A5)
    norm = N.normalizer(*N.moments_of(eps))
    pre = [dict(ep, observation=N.normalize(ep['observation'], *norm)) for ep in eps]
    aN, aP, aE = make_agent(kind), make_agent(kind), make_agent(kind)
    engN, itN = arena_iter(eps, norm)
    engP, itP = arena_iter(pre)
    engE, itE = arena_iter(eps, norm)
    assert aN.enable_graph(itN) and aP.enable_graph(itP)
    before = state_of(aN)
    for step in range(3):
        aN.update(itN, step), aP.update(itP, step), aE.update(itE, step)
    assert_same_state(aN, aP)
    assert_same_state(aN, aE)
    assert not torch.equal(before[0][1], state_of(aN)[0][1])
    assert np.array_equal(engN.last_pairs(B5), engP.last_pairs(B5))
    norm2 = (norm[0] + np.float32(0.25), norm[1] * np.float32(0.5))
    engN.set_obs_normalizer(*norm2)                              # new values in place: the captured graph reads them, no re-capture
    engE.set_obs_normalizer(*norm2)
    captures = aN.engine.graph_captures
    for step in range(3, 5):
        aN.update(itN, step), aE.update(itE, step), aP.update(itP, step)
    assert aN.engine.graph_captures == captures
    assert_same_state(aN, aE)
    assert any(not torch.equal(x[1], y[1]) for x, y in zip(state_of(aN), state_of(aP)))      # P kept the first normaliser's data
    engN.clear_obs_normalizer()                                  # off: the graph holds the normalising kernel
    with pytest.raises(L.ExorlError, match='normaliser'):
        aN.update(itN, 5)
    engP.set_obs_normalizer(*norm)                               # on: the graph holds the copying kernel
    with pytest.raises(L.ExorlError, match='normaliser'):
        aP.update(itP, 5)
    engN.set_obs_normalizer(*norm2)
    assert aN.enable_graph(itN)                                  # a new capture in the new state runs
    aN.update(itN, 5)
    torch.cuda.synchronize()


def test_enable_graph_intr_refuses_a_normalised_arena():
    from exorl_amd import _lib as L
    eps = N.norm_episodes(56, [40, 25], O5, A5)
    ag = make_agent('td3_bc')
    eng, it = arena_iter(eps, N.normalizer(*N.moments_of(eps)))
    with pytest.raises(L.ExorlError, match='normaliser'):
        ag.engine.enable_graph_intr(eng, 1, 0.99, 0.2)
    eng.clear_obs_normalizer()
    ag.engine.enable_graph_intr(eng, 1, 0.99, 0.2)               # the same call on the plain arena is accepted
    ag.engine.disable_graph()


# ---- 6. act() and pickling ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['td3_bc', 'cql'])             # td3_bc: the act_host fast path; cql: the generic path
def test_act_normalises_and_the_normaliser_is_pickled(kind):
    eps = N.norm_episodes(57, [40], O5, A5)
    norm = N.normalizer(*N.moments_of(eps))
    a, twin = make_agent(kind), make_agent(kind)
    a.set_obs_normalizer(*norm)
    obs = eps[0]['observation'][7]
    got = a.act(obs, 0, eval_mode=True)
    want = twin.act(N.normalize(obs, *norm), 0, eval_mode=True)
    assert got.shape == (A5,) and np.array_equal(N.bits(got), N.bits(want))
    assert not np.array_equal(got, twin.act(obs, 0, eval_mode=True))
    assert np.array_equal(a.act(obs.astype(np.float64).tolist(), 0, eval_mode=True), got)      # what an environment hands over
    b = pickle.loads(pickle.dumps(a))
    assert np.array_equal(N.bits(b.obs_norm_mean), N.bits(norm[0])) and np.array_equal(N.bits(b.obs_norm_inv), N.bits(norm[1]))
    assert np.array_equal(N.bits(b.act(obs, 0, eval_mode=True)), N.bits(got))
    a.clear_obs_normalizer()
    assert np.array_equal(N.bits(a.act(obs, 0, eval_mode=True)), N.bits(twin.act(obs, 0, eval_mode=True)))
    assert pickle.loads(pickle.dumps(a)).obs_norm_mean is None
    with pytest.raises(ValueError, match='columns'):
        a.set_obs_normalizer(np.zeros(O5 + 1, np.float32), np.ones(O5 + 1, np.float32))


def test_reward_free_agent_normalises_the_observation_part_only():
    from exorl_amd import agents
    S = 3
    mk = lambda: (torch.manual_seed(4), agents.DDPGAgent('ddpg', True, 'states', (O5,), (A5,), 'cuda', 1e-4, 50, H5, 0.01, 0, 2, 0.2, 3, B5, 0.3,
                                                         True, False, False, meta_dim=S, precision='fp32'))[1]
    a, twin = mk(), mk()
    eps = N.norm_episodes(58, [20], O5, A5, S)
    norm = N.normalizer(*N.moments_of(eps))
    a.set_obs_normalizer(*norm)
    obs, meta = eps[0]['observation'][4], {'skill': eps[0]['skill'][4]}
    got = a.act(obs, meta, 0, eval_mode=True)
    assert np.array_equal(N.bits(got), N.bits(twin.act(N.normalize(obs, *norm), meta, 0, eval_mode=True)))


# ---- 7. train_offline(normalize_obs=True) ---------------------------------------------------------------------------------------------------
def test_train_offline_normalize_obs_equals_the_manual_sequence(tmp_path):
    from exorl_amd.replay_buffer import make_replay_loader
    from exorl_amd.train_offline import train_offline
    eps = N.norm_episodes(59, [10, 8, 12, 9, 11, 10], O5, A5)
    d = write_dir(tmp_path / 'buffer', eps)
    a1, a2 = make_agent('td3_bc'), make_agent('td3_bc')
    seen = []
    np.random.seed(9)                                           # the loader's Philox seed comes from the global NumPy state
    train_offline(a1, d, 5, B5, 0.99, eval_fn=lambda step, agent: seen.append(agent.obs_norm_mean.copy()), normalize_obs=True)
    np.random.seed(9)
    it = iter(make_replay_loader(None, d, 10 ** 7, B5, 0, 0.99, sampler='philox', normalize_obs=True))
    want = N.normalizer(*N.moments_of(eps))
    assert np.array_equal(N.bits(it.obs_normalizer[0]), N.bits(want[0])) and np.array_equal(N.bits(it.obs_normalizer[1]), N.bits(want[1]))
    assert np.array_equal(N.bits(a1.obs_norm_mean), N.bits(want[0])) and np.array_equal(N.bits(a1.obs_norm_inv), N.bits(want[1]))
    assert len(seen) == 1 and np.array_equal(seen[0], want[0])  # eval_fn's agent already carries it
    a2.set_obs_normalizer(*it.obs_normalizer)
    assert a2.enable_graph(it, 0)
    for step in range(5):
        a2.update(it, step)
    assert_same_state(a1, a2)
    assert a1.engine.opt_steps() == (5, 5)
