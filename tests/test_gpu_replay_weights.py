"""GPU checks of weighted sampling in the HBM replay (exorl_replay_set_weights): the device index stream equals the restatement in
tests/_replay_weights.py pair for pair over three consecutive batches, the gathered batch equals EXORL_SAMPLER_GIVEN's on the same pairs bit
for bit, slot reuse, the host-side refusals, the captured step graph, and the loaders (mix of directories, episode_weight callable)."""
import numpy as np
import pytest
import torch

import _replay_weights as RW
import _synth
from oracle.replay import philox_draw

pytestmark = pytest.mark.gpu
SEED = 4242


def arena(lengths, O=4, A=2, seed=0, meta_dim=0, u8=False, obs_shape=None, max_episodes=None):
    from exorl_amd.engine import ReplayEngine
    eps = _synth.synth_episodes(seed, lengths, O, A, meta_dim, u8)
    shape = obs_shape or (O,)
    for ep in eps:
        ep['observation'] = ep['observation'].reshape((-1,) + tuple(shape))
    eng = ReplayEngine(shape, np.uint8 if u8 else np.float32, A, meta_dim, sum(lengths) + len(lengths) + 64,
                       max_episodes or len(lengths) + 8)
    slots = [eng.append_episode(ep, ('skill',) if meta_dim else ()) for ep in eps]
    eng.set_order(slots)
    eng.seed_philox(SEED)
    return eng, slots, eps


def check_stream(eng, lengths, nstep, weighting, q, B, first_counter=0, batches=3):
    """Three consecutive batches: every pair equals the restatement (the batch counter advances by one per sample call)."""
    from exorl_amd import _lib as L
    for c in range(first_counter, first_counter + batches):
        eng.sample(B, nstep, 0.99, L.SAMPLER_PHILOX)
        got = eng.last_pairs(B)
        want = RW.weighted_pairs(SEED, c, B, lengths, nstep, weighting, q)
        assert np.array_equal(got, want), (weighting, nstep, B, c, got[:8].tolist(), want[:8].tolist())
        spans = np.asarray(lengths)[got[:, 0]] - nstep + 1
        assert np.all(spans >= 1) and np.all(got[:, 1] >= 1) and np.all(got[:, 1] <= spans)
    return first_counter + batches


def check_unweighted(eng, lengths, nstep, B, first_counter):
    from exorl_amd import _lib as L
    for c in range(first_counter, first_counter + 3):
        eng.sample(B, nstep, 0.99, L.SAMPLER_PHILOX)
        want = np.array([philox_draw(SEED, c, b, len(lengths), lengths, nstep) for b in range(B)], np.int32)
        assert np.array_equal(eng.last_pairs(B), want), c
    return first_counter + 3


# ---- 1. transition-uniform stream -------------------------------------------------------------------------------------------------------
RANDOM_LENGTHS = [int(x) for x in np.random.RandomState(8).randint(1, 51, 1000)]


@pytest.mark.parametrize('lengths,nsteps', [([1, 2, 3, 5, 40, 2, 17], (1, 3)), ([9], (1, 3)), ([1, 1, 1], (1,)), (RANDOM_LENGTHS, (1, 3))],
                         ids=['seven', 'single', 'ones', 'thousand'])
@pytest.mark.parametrize('B', [5, 4096])
def test_transition_uniform_stream(lengths, nsteps, B):
    """weights=None in 'transitions' mode. At nstep 3 the episodes shorter than 3 have mass 0 and are never drawn (check_stream asserts
    every span >= 1); with lengths [1, 1, 1] every g is a table boundary."""
    eng, _, _ = arena(lengths)
    eng.set_weights('transitions')
    counter = 0
    for nstep in nsteps:
        counter = check_stream(eng, lengths, nstep, 'transitions', None, B, counter)


# ---- 2. integer weights -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('weighting', ['episodes', 'transitions'])
def test_integer_weights_stream(weighting):
    lengths = [1, 2, 3, 5, 40, 2, 17]
    w = [3.0, 1.0, 0.0, 2.0, 5.0, 1.0, 0.0]                      # a zero weight in the middle and one at the end
    eng, _, _ = arena(lengths)
    eng.set_weights(weighting, w)
    q = RW.quantise(w)
    counter = check_stream(eng, lengths, 1, weighting, q, 512)
    counter = check_stream(eng, lengths, 3, weighting, q, 512, counter)
    from exorl_amd import _lib as L
    eng.sample(4096, 1, 0.99, L.SAMPLER_PHILOX)
    counter += 1
    assert not np.isin(eng.last_pairs(4096)[:, 0], [2, 6]).any()   # zero weight: never drawn
    # back to the default: the unweighted stream again, continuing at the same counter
    eng.set_weights('episodes', None)
    check_unweighted(eng, lengths, 1, 512, counter)


def test_total_mass_above_2_pow_32():
    lengths = [300, 400]
    eng, _, _ = arena(lengths)
    eng.set_weights('transitions', [1.0, 0.5])
    q = RW.quantise([1.0, 0.5])
    assert q == [1 << 24, 1 << 23] and RW.cum_table(lengths, q, 1, 'transitions')[-1] > 1 << 32
    check_stream(eng, lengths, 1, 'transitions', q, 4096)


def test_a_replay_that_never_saw_set_weights_is_the_unweighted_sampler():
    lengths = [6, 9, 4, 12, 7]
    eng, _, _ = arena(lengths)
    c = check_unweighted(eng, lengths, 1, 512, 0)
    check_unweighted(eng, lengths, 3, 512, c)


# ---- 3. batch contents ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', ['f32x5', 'f32x8', 'u8_3x8x8'])
@pytest.mark.parametrize('meta_dim', [0, 3])
def test_weighted_batch_equals_given_pairs_batch(layout, meta_dim):
    """The 4-byte row copy (5 fp32 columns), the 16-byte one (8 columns) and uint8 frames; nstep 3; with and without meta columns."""
    from exorl_amd import _lib as L
    lengths = [4, 2, 30, 11, 3, 25]
    O, u8, shape = {'f32x5': (5, False, None), 'f32x8': (8, False, None), 'u8_3x8x8': (192, True, (3, 8, 8))}[layout]
    eng, _, _ = arena(lengths, O=O, A=3, seed=3, meta_dim=meta_dim, u8=u8, obs_shape=shape)
    w = [1.0, 9.0, 0.5, 2.0, 1.0, 0.25]
    eng.set_weights('transitions', w)
    B = 257
    for c in range(3):
        got = eng.sample(B, 3, 0.99, L.SAMPLER_PHILOX)
        pairs = eng.last_pairs(B)
        assert np.array_equal(pairs, RW.weighted_pairs(SEED, c, B, lengths, 3, 'transitions', RW.quantise(w)))
        want = eng.sample(B, 3, 0.99, L.SAMPLER_GIVEN, pairs=pairs)
        assert len(got) == len(want) == (6 if meta_dim else 5)
        for i, (g, r) in enumerate(zip(got, want)):
            assert g.dtype == r.dtype and torch.equal(g, r), (layout, meta_dim, c, i)


# ---- 4. eviction and slot reuse ---------------------------------------------------------------------------------------------------------
def test_eviction_and_slot_reuse():
    lengths = [6, 9, 4, 12, 7]
    w = [1.0, 2.0, 3.0, 4.0, 5.0]
    eng, slots, _ = arena(lengths)
    eng.set_weights('transitions', w)
    counter = check_stream(eng, lengths, 2, 'transitions', RW.quantise(w), 512)
    eng.evict(slots[2])
    new = eng.append_episode(_synth.synth_episodes(9, [10], 4, 2)[0])
    assert new == slots[2]                                       # the freed slot is reused ...
    order = [3, 0, 2, 4, 1]
    eng.set_order([slots[i] for i in order])
    q = RW.quantise(w)
    q[2] = 1                                                     # ... and is back at weight 1, whatever its predecessor had
    lens2 = [12, 6, 10, 7, 9]
    check_stream(eng, lens2, 2, 'transitions', [q[i] for i in order], 512, counter)


# ---- 5. errors --------------------------------------------------------------------------------------------------------------------------
def test_all_zero_mass_is_refused():
    from exorl_amd import _lib as L
    eng, _, _ = arena([2, 2])
    eng.set_weights('transitions')
    with pytest.raises(L.ExorlError, match='total sampling mass is 0'):
        eng.sample(8, 3, 0.99, L.SAMPLER_PHILOX)
    eng.set_weights('episodes', [1.0, 1.0])
    with pytest.raises(L.ExorlError, match='total sampling mass is 0'):
        eng.sample(8, 3, 0.99, L.SAMPLER_PHILOX)
    check_stream(eng, [2, 2], 1, 'episodes', RW.quantise([1.0, 1.0]), 8)      # the refused calls spent no batch counter


def test_weights_with_the_mt_sampler_are_refused():
    from exorl_amd import _lib as L
    lengths = [6, 9, 4]
    eng, _, _ = arena(lengths)
    eng.seed_mt_ints(1, 1)
    eng.set_weights('transitions')
    with pytest.raises(L.ExorlError, match='weighted sampling needs EXORL_SAMPLER_PHILOX'):
        eng.sample(8, 1, 0.99, L.SAMPLER_MT19937)
    check_stream(eng, lengths, 1, 'transitions', None, 8)
    pairs = np.array([[2, 4], [0, 1]], np.int32)                   # GIVEN ignores the weights
    out = eng.sample(2, 1, 0.99, L.SAMPLER_GIVEN, pairs=pairs, want_pairs=True)
    assert np.array_equal(out[1], pairs)
    eng.set_weights('episodes', None)
    eng.sample(8, 1, 0.99, L.SAMPLER_MT19937)                      # weighting off: the reference stream is served again


def test_total_mass_of_2_pow_63_is_refused():
    """One episode of 2^19 transitions listed 2^20 + 1 times at weight 2^24: 2^24 * 2^19 * (2^20 + 1) > 2^63."""
    from exorl_amd import _lib as L
    from exorl_amd.engine import ReplayEngine
    T, N = 1 << 19, (1 << 20) + 1
    eng = ReplayEngine((1,), np.float32, 1, 0, T + 64, N + 8)
    rows = T + 1
    ep = dict(observation=np.arange(rows, dtype=np.float32).reshape(rows, 1), action=np.zeros((rows, 1), np.float32),
              reward=np.ones((rows, 1), np.float32), discount=np.ones((rows, 1), np.float32))
    s = eng.append_episode(ep)
    eng.seed_philox(SEED)
    eng.set_order(np.full(N, s, np.int32))
    eng.set_weights('transitions', [1.0])
    assert RW.cum_table([T] * N, [1 << 24] * N, 1, 'transitions')[-1] >= 1 << 63
    with pytest.raises(L.ExorlError, match=r'reaches 2\^63'):
        eng.sample(8, 1, 0.99, L.SAMPLER_PHILOX)
    eng.set_order([s, s])
    check_stream(eng, [T, T], 1, 'transitions', [1 << 24] * 2, 64)


def test_short_episodes_unweighted_refused_weighted_skipped():
    from exorl_amd import _lib as L
    lengths = [5, 2, 7]
    eng, _, _ = arena(lengths)
    with pytest.raises(L.ExorlError, match='shorter than nstep'):
        eng.sample(8, 3, 0.99, L.SAMPLER_PHILOX)
    eng.set_weights('episodes', [1.0, 1.0, 1.0])
    c = check_stream(eng, lengths, 3, 'episodes', RW.quantise([1.0, 1.0, 1.0]), 512)
    eng.set_weights('transitions')
    c = check_stream(eng, lengths, 3, 'transitions', None, 512, c)
    eng.set_weights('episodes', None)
    with pytest.raises(L.ExorlError, match='shorter than nstep'):
        eng.sample(8, 3, 0.99, L.SAMPLER_PHILOX)


# ---- 6. captured graph ------------------------------------------------------------------------------------------------------------------
def test_captured_graph_on_a_weighted_arena():
    """TD3+BC through the captured sample+update graph and through eager launches, each on its own copy of one weighted arena: the same
    pairs as the restatement at every step and identical parameters after 5 steps. nstep 3 with a 2-step episode resident: the capture
    goes through the weighted path's checks (mass 0) instead of the shortest-episode refusal."""
    from exorl_amd import agents
    from exorl_amd.replay_buffer import ArenaIterator
    O, A, H, B, nstep = 24, 6, 32, 64, 3
    lengths = [200, 30, 2, 250, 5, 120]
    w = [1.0, 2.0, 7.0, 0.5, 1.0, 3.0]
    q = RW.quantise(w)
    ags, engs, its = [], [], []
    for _ in range(2):
        torch.manual_seed(3)
        ags.append(agents.TD3BCAgent('td3_bc', (O,), (A,), 'cuda', 1e-4, H, 0.01, 0.2, 1, B, 0.3, True, 2.5))
        eng, _, eps = arena(lengths, O=O, A=A, seed=9)
        engs.append(eng)
        its.append(ArenaIterator(eng, B, nstep, 0.99, 'philox', weighting='transitions', episode_weight=lambda ep: ep['w'],
                                 episodes=[dict(ep, w=x) for ep, x in zip(eps, w)]))
    assert ags[0].enable_graph(its[0])                            # the capture spends no batch counter
    for step in range(5):
        m0, m1 = ags[0].update(its[0], step), ags[1].update(its[1], step)
        assert m0 == m1, step
        want = RW.weighted_pairs(SEED, step, B, lengths, nstep, 'transitions', q)
        for eng in engs:
            assert np.array_equal(eng.last_pairs(B), want), step
    for net in ('actor', 'critic', 'critic_target'):
        for p, r in zip(getattr(ags[0], net).parameters(), getattr(ags[1], net).parameters()):
            assert torch.equal(p, r), net
    # weights changed after the capture: the graph would sample the table it was captured with, so the step is refused, not run
    from exorl_amd import _lib as L
    for eng in engs:
        eng.set_weights('transitions')
    with pytest.raises(L.ExorlError, match='exorl_agent_enable_graph again'):
        ags[0].update(its[0], 5)
    assert ags[0].enable_graph(its[0], 5)
    m0, m1 = ags[0].update(its[0], 5), ags[1].update(its[1], 5)
    assert m0 == m1
    want = RW.weighted_pairs(SEED, 5, B, lengths, nstep, 'transitions', None)
    for eng in engs:
        assert np.array_equal(eng.last_pairs(B), want)


# ---- 7. loaders -------------------------------------------------------------------------------------------------------------------------
def _write(d, lengths, O, A, seed):
    from exorl_amd.replay_buffer import save_episode
    d.mkdir()
    eps = _synth.synth_episodes(seed, lengths, O, A)
    for i, (ep, n) in enumerate(zip(eps, lengths)):
        save_episode(ep, d / f'episode_{i}_{n}.npz')
    return eps


def test_offline_mix_of_two_directories(tmp_path):
    from exorl_amd import agents
    from exorl_amd.replay_buffer import make_offline_replay_loader
    from exorl_amd.train_offline import train_offline
    O, A, B = 11, 3, 64
    sets = [[7, 9, 30, 4], [12, 5, 50]]
    d1, d2 = tmp_path / 'reward', tmp_path / 'constraint'
    _write(d1, sets[0], O, A, 1)
    _write(d2, sets[1], O, A, 2)
    it = iter(make_offline_replay_loader(None, [d1, d2], 10 ** 6, B, 1, 0.99, mix=[0.25, 0.75], weighting='transitions',
                                         sampler='philox', seed=99))
    # the table the loader must have built, from the file names alone: ascending within a directory, directories in the order given
    names = [sorted(p.name for p in d.glob('*.npz')) for d in (d1, d2)]
    lens = [[int(n[:-4].split('_')[2]) for n in ns] for ns in names]
    assert lens == sets
    flat, q = lens[0] + lens[1], RW.mix_q(lens, [0.25, 0.75], 'transitions')
    cum = RW.cum_table(flat, q, 1, 'transitions')
    for c in range(3):
        batch = next(it)
        assert len(batch) == 5 and batch[0].shape == (B, O)
        pairs = it.shards[0].engine.last_pairs(B)
        want = np.array([RW.weighted_draw(99, c, b, cum, flat, 1) for b in range(B)], np.int32)
        assert np.array_equal(pairs, want), c
    assert [fn.parent for fn in it.shards[0].fns] == [d1] * 4 + [d2] * 3
    torch.manual_seed(0)
    ag = agents.TD3BCAgent('td3_bc', (O,), (A,), 'cuda', 1e-4, 32, 0.01, '0.2', 1, B, 0.3, False, 2.5)
    rows = train_offline(ag, [d1, d2], 3, B, 0.99, log_every_steps=1, mix=[0.25, 0.75], weighting='transitions')
    assert ag._graph_iter is not None and ag.engine.opt_steps() == (3, 3) and len(rows) == 3
    eng = ag._graph_iter.engine                                   # seeded from NumPy's global state: the table is what can be checked
    eng.seed_philox(99)
    eng.sample(B, 1, 0.99, 1)
    assert np.array_equal(eng.last_pairs(B), np.array([RW.weighted_draw(99, 0, b, cum, flat, 1) for b in range(B)], np.int32))


class Spec:
    def __init__(self, shape, dtype, name):
        self.shape, self.dtype, self.name = tuple(shape), np.dtype(dtype), name


def test_online_loader_with_an_episode_weight_callable(tmp_path):
    """weighting='transitions' with a callable on a `constraint` meta key; the stream is exact across a fetch that adds episodes (and,
    with the size limit reached, evicts the first one): the weights follow the slots."""
    from exorl_amd.replay_buffer import ReplayBufferStorage, make_replay_loader
    O, A, B, nstep = 6, 2, 128, 2
    lengths = [9, 14, 7, 11, 8, 12]
    hit = [0, 1, 0, 0, 1, 1]
    eps = _synth.synth_episodes(21, lengths, O, A)
    for ep, h in zip(eps, hit):
        c = np.zeros((len(ep['reward']), 1), np.float32)
        c[3:5] = h
        ep['constraint'] = c
    st = ReplayBufferStorage((), (Spec((1,), np.float32, 'constraint'),), tmp_path / 'buffer')
    for ep in eps[:4]:
        st._store_episode(ep)
    weight = lambda ep: 4.0 if ep['constraint'].any() else 1.0
    it = iter(make_replay_loader(st, 55, B, 0, True, nstep, 0.99, fetch_every=B, sampler='philox', seed=5, weighting='transitions',
                                 episode_weight=weight))

    def check(counter, resident):
        batch = next(it)
        assert len(batch) == 6 and batch[5].shape == (B, 1)
        shard = it.shards[0]
        assert [int(fn.stem.split('_')[1]) for fn in shard.fns] == resident
        q = RW.quantise([4.0 if hit[i] else 1.0 for i in resident])
        want = RW.weighted_pairs(5, counter, B, [lengths[i] for i in resident], nstep, 'transitions', q)
        pairs = shard.engine.last_pairs(B)
        assert np.array_equal(pairs, want), counter
        flag = np.array([eps[resident[p]]['constraint'][i - 1, 0] for p, i in pairs], np.float32)
        assert np.array_equal(batch[5].cpu().numpy().reshape(-1), flag)              # the meta column of the sampled rows

    check(0, [0, 1, 2, 3])
    for ep in eps[4:]:
        st._store_episode(ep)                                     # 41 + 8 + 12 > 55: episode 0 is evicted, its slot is reused
    check(1, [1, 2, 3, 4, 5])
    check(2, [1, 2, 3, 4, 5])
