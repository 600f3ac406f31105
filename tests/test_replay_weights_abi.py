"""CPU checks of weighted replay sampling: the export, its declaration and binding, the ABI version, quantise_weights, the restatement of
the draw in tests/_replay_weights.py (search == brute force, distribution within 5 binomial sigma on fixed seeds), the multi-directory
selection from file names and the mix -> weights arithmetic, and the keyword plumbing of the loaders and train_offline."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import _replay_weights as RW

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope='module')
def lib():
    return ctypes.CDLL(str(ROOT / 'exorl_amd' / 'libexorl_hip.so'))


def test_symbol_declared_exported_and_bound(lib):
    from exorl_amd import _lib as L
    header = (ROOT / 'include' / 'exorl_hip.h').read_text()
    m = re.search(r'int exorl_replay_set_weights\((.*?)\);', header, re.S)
    assert m, 'exorl_replay_set_weights is not declared in include/exorl_hip.h'
    assert len([a for a in m.group(1).split(',') if a.strip()]) == 4
    assert re.search(r'#define EXORL_WEIGHT_EPISODES\s+0\b', header) and re.search(r'#define EXORL_WEIGHT_TRANSITIONS\s+1\b', header)
    assert hasattr(lib, 'exorl_replay_set_weights'), 'exorl_replay_set_weights is not exported'
    res, args = L.PROTOTYPES['exorl_replay_set_weights']
    assert res is ctypes.c_int and len(args) == 4
    assert (L.WEIGHT_EPISODES, L.WEIGHT_TRANSITIONS) == (0, 1)


def test_abi_version_is_unchanged(lib):
    header = (ROOT / 'include' / 'exorl_hip.h').read_text()
    lib.exorl_abi_version.restype = ctypes.c_int
    assert lib.exorl_abi_version() == 13
    assert re.search(r'#define EXORL_ABI_VERSION 13\b', header)
    comment = header[header.index('#define EXORL_ABI_VERSION'):header.index('const char* exorl_last_error')]
    assert 'exorl_replay_set_weights' in comment          # the version-12 comment names the additive export


def test_null_handle_is_an_error_not_a_crash(lib):
    lib.exorl_replay_set_weights.restype = ctypes.c_int
    lib.exorl_replay_set_weights.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32]
    lib.exorl_last_error.restype = ctypes.c_char_p
    assert lib.exorl_replay_set_weights(None, 0, None, 0) != 0
    assert b'replay_set_weights' in lib.exorl_last_error()


# ---- quantise_weights -----------------------------------------------------------------------------------------------------------------
def test_quantise_weights():
    from exorl_amd.engine import quantise_weights
    q = quantise_weights([0.5, 2.0, 0.0, 1.0, 1e-30, 2.0])
    assert q.dtype == np.uint32
    assert q.tolist() == [1 << 22, 1 << 24, 0, 1 << 23, 1, 1 << 24]       # largest -> 2^24, zero kept, a tiny positive floored at 1
    assert quantise_weights([7.0]).tolist() == [1 << 24]
    assert quantise_weights(np.float32([3, 1])).tolist() == [1 << 24, int(np.rint(float(1 << 24) / 3))]     # float64 arithmetic
    rs = np.random.RandomState(0)
    w = rs.uniform(0, 1, 1000) ** 8
    w[::7] = 0
    q = quantise_weights(w)
    assert q.max() == 1 << 24 and np.all((q == 0) == (w == 0))
    assert q.tolist() == RW.quantise(w)
    for bad in ([], [0.0, 0.0], [1.0, -1.0], [1.0, np.nan], [np.inf, 1.0]):
        with pytest.raises(ValueError):
            quantise_weights(bad)


def test_engine_set_weights_refuses_an_unknown_mode():
    from exorl_amd.engine import ReplayEngine
    eng = object.__new__(ReplayEngine)            # no device needed: the mode is checked before the library is touched
    with pytest.raises(ValueError, match='weighting'):
        ReplayEngine.set_weights(eng, 'uniform')


# ---- the restatement: search --------------------------------------------------------------------------------------------------------
def _boundary_probes(cum):
    total = cum[-1]
    return sorted({g for c in cum for g in (c - 1, c, c + 1) if 0 <= g < total} | {0, total - 1})


@pytest.mark.parametrize('masses', [[5], [1, 1, 1], [0, 0, 3, 1], [2, 0, 0, 0, 7, 1], [4, 9, 0, 0], [0, 1, 0, 1, 0], [0, 0, 1],
                                    [1 << 40, 0, (1 << 62) - (1 << 40) - 1, 1]])
def test_search_equals_scan_on_edge_tables(masses):
    cum = [0]
    for m in masses:
        cum.append(cum[-1] + m)
    for g in _boundary_probes(cum):
        pos = RW.search(cum, g)
        assert pos == RW.search_scan(cum, g) and masses[pos] > 0 and cum[pos] <= g < cum[pos + 1]


def test_search_equals_scan_on_random_tables():
    rs = np.random.RandomState(5)
    for trial in range(200):
        n = int(rs.randint(1, 40))
        masses = [int(m) for m in rs.randint(0, 50, n) * (rs.uniform(size=n) < 0.6)]
        if trial % 3 == 0:                                  # zero-mass runs at the front, in the middle and at the end
            k = max(1, n // 4)
            masses[:k] = [0] * k
            masses[-k:] = [0] * k
            masses[n // 2:n // 2 + k] = [0] * len(masses[n // 2:n // 2 + k])
        if sum(masses) == 0:
            masses[int(rs.randint(n))] = 3
        cum = [0]
        for m in masses:
            cum.append(cum[-1] + m)
        probes = _boundary_probes(cum) + [int(g) for g in rs.randint(0, cum[-1], 20)]
        for g in probes:
            assert RW.search(cum, g) == RW.search_scan(cum, g), (masses, g)


def test_cum_table_modes():
    lens = [1, 2, 3, 5, 40, 2, 17]
    assert RW.cum_table(lens, None, 1, 'transitions') == [0, 1, 3, 6, 11, 51, 53, 70]
    assert RW.cum_table(lens, None, 3, 'transitions') == [0, 0, 0, 1, 4, 42, 42, 57]
    assert RW.cum_table(lens, None, 3, 'episodes') == [0, 0, 0, 1, 2, 3, 3, 4]
    assert RW.cum_table(lens, [2, 2, 0, 3, 1, 9, 0], 3, 'episodes') == [0, 0, 0, 0, 3, 4, 4, 4]
    assert RW.cum_table([300, 400], [1 << 24, 1 << 23], 1, 'transitions')[-1] == 300 * (1 << 24) + 400 * (1 << 23) > 1 << 32


# ---- the restatement: distribution (deterministic for fixed seeds; bound = 5 binomial sigma) ----------------------------------------
def _z(count, n, p):
    return (count - n * p) / np.sqrt(n * p * (1 - p))


def _draws(seed, batches, lengths, nstep, weighting, q=None):
    return np.concatenate([RW.weighted_pairs(seed, c, 4096, lengths, nstep, weighting, q) for c in range(batches)])


def test_distribution_transitions_long_and_short_episodes():
    lens = [1000] + [10] * 9
    p = _draws(12345, 16, lens, 1, 'transitions')
    z = _z(int((p[:, 0] == 0).sum()), len(p), 1000 / 1090)
    print('case a: z =', z)
    assert abs(z) <= 5
    assert p[:, 1].min() >= 1 and np.all(p[:, 1] <= np.asarray(lens)[p[:, 0]])


def test_distribution_every_start_equally_likely():
    lens = [3, 5, 2]
    p = _draws(777, 10, lens, 1, 'transitions')
    flat = np.asarray([0, 3, 8])[p[:, 0]] + p[:, 1] - 1
    counts = np.bincount(flat, minlength=10)
    zs = [_z(int(c), len(p), 0.1) for c in counts]
    print('case b: z =', zs)
    assert len(counts) == 10 and max(abs(z) for z in zs) <= 5


def test_distribution_mix_of_two_datasets():
    sets = [[7, 9, 30, 4], [12, 5, 50]]
    lens = sets[0] + sets[1]
    for weighting in ('transitions', 'episodes'):
        p = _draws(99, 8, lens, 1, weighting, RW.mix_q(sets, [0.25, 0.75], weighting))
        z = _z(int((p[:, 0] >= 4).sum()), len(p), 0.75)
        print('case c', weighting, ': z =', z)
        assert abs(z) <= 5


# ---- host logic: selection from names, mix arithmetic, keyword plumbing ---------------------------------------------------------------
def _touch(d, items):
    d.mkdir()
    for idx, n in items:
        (d / f'episode_{idx}_{n}.npz').touch()
    return d


def test_multi_directory_selection_from_names(tmp_path):
    from exorl_amd.replay_buffer import _OfflineShard
    d1 = _touch(tmp_path / 'a', [(0, 7), (1, 9), (2, 30), (3, 4)])
    d2 = _touch(tmp_path / 'b', [(0, 12), (1, 5), (2, 50), (10, 8)])
    picks = _OfflineShard.select_many([d1, d2], 10 ** 6, 1, 0)
    names = [[fn.name for fn in t] for t, _ in picks]
    assert names == [['episode_0_7.npz', 'episode_1_9.npz', 'episode_2_30.npz', 'episode_3_4.npz'],
                     ['episode_0_12.npz', 'episode_10_8.npz', 'episode_1_5.npz', 'episode_2_50.npz']]      # ascending by NAME per directory
    assert [n for _, n in picks] == [50, 75]
    assert [fn.parent for t, _ in picks for fn in t] == [d1] * 4 + [d2] * 4
    # every directory is cut by the same max_size on its own: the episode that takes the size past it is the last one kept
    picks = _OfflineShard.select_many([d1, d2], 15, 1, 0)
    assert [[fn.name for fn in t] for t, _ in picks] == [['episode_0_7.npz', 'episode_1_9.npz'], ['episode_0_12.npz', 'episode_10_8.npz']]
    # worker modulo, per directory
    picks = _OfflineShard.select_many([d1, d2], 10 ** 6, 2, 1)
    assert [[fn.name for fn in t] for t, _ in picks] == [['episode_1_9.npz', 'episode_3_4.npz'], ['episode_1_5.npz']]
    assert _OfflineShard.select_many([d1], 10 ** 6, 1, 0)[0] == _OfflineShard.select(d1, 10 ** 6, 1, 0)


def test_mix_weights_arithmetic():
    from exorl_amd.engine import quantise_weights
    from exorl_amd.replay_buffer import mix_weights
    sets = [[7, 9, 30, 4], [12, 5, 50]]
    assert mix_weights(sets, [0.25, 0.75], 'transitions', 1) == [0.25 / 50, 0.75 / 67]
    assert mix_weights(sets, [0.25, 0.75], 'episodes', 1) == [0.25 / 4, 0.75 / 3]
    assert mix_weights(sets, [0.25, 0.75], 'transitions', 6) == [0.25 / (2 + 4 + 25), 0.75 / (7 + 45)]      # spans len - 5, short episodes 0
    assert mix_weights(sets, [0.25, 0.75], 'episodes', 6) == [0.25 / 3, 0.75 / 2]
    for weighting in ('transitions', 'episodes'):
        per = mix_weights(sets, [0.25, 0.75], weighting, 1)
        w = [per[0]] * 4 + [per[1]] * 3
        assert quantise_weights(w).tolist() == RW.mix_q(sets, [0.25, 0.75], weighting)
        cum = RW.cum_table(sets[0] + sets[1], quantise_weights(w), 1, weighting)
        assert abs((cum[-1] - cum[4]) / cum[-1] - 0.75) < 1e-6                                            # the second dataset's share of the mass
    with pytest.raises(ValueError):
        mix_weights(sets, [0.5], 'episodes', 1)
    with pytest.raises(ValueError):
        mix_weights(sets, [0.5, -0.5], 'episodes', 1)
    with pytest.raises(ValueError):
        mix_weights([[3, 4], [9]], [0.5, 0.5], 'transitions', 5)          # dataset 0 holds no 5-step window


def test_loaders_refuse_weighting_with_the_mt_sampler(tmp_path):
    from exorl_amd.replay_buffer import ArenaIterator, make_offline_replay_loader, make_replay_loader
    d1, d2 = _touch(tmp_path / 'a', [(0, 7)]), _touch(tmp_path / 'b', [(0, 12)])
    for kw in (dict(weighting='transitions'), dict(episode_weight=lambda ep: 1.0), dict(mix=[0.5, 0.5])):
        with pytest.raises(ValueError, match='philox'):
            make_offline_replay_loader(None, [d1, d2], 100, 8, 1, 0.99, sampler='mt19937', **kw)
        with pytest.raises(ValueError, match='philox'):
            make_offline_replay_loader(None, [d1, d2], 100, 8, 1, 0.99, **kw)                  # the loader's default sampler is mt19937
    with pytest.raises(ValueError, match='philox'):
        ArenaIterator(None, 8, 1, 0.99, 'mt19937', weighting='transitions')
    with pytest.raises(ValueError, match='weighting'):
        make_offline_replay_loader(None, d1, 100, 8, 1, 0.99, sampler='philox', weighting='uniform')
    with pytest.raises(ValueError, match='mix'):
        make_offline_replay_loader(None, d1, 100, 8, 1, 0.99, sampler='philox', mix=[1.0])       # mix without a list of directories
    with pytest.raises(ValueError, match='mix'):
        make_offline_replay_loader(None, [d1, d2], 100, 8, 1, 0.99, sampler='philox', mix=[1.0])
    ld = make_replay_loader(None, [d1, d2], 100, 8, 1, 0.99, sampler='philox', mix=[1, 3], weighting='transitions')     # the 6-argument shape
    assert ld.offline and ld.mix == [1.0, 3.0] and ld.weighting == 'transitions' and ld.storage._replay_dirs == [d1, d2]
    ld = make_offline_replay_loader(None, d1, 100, 8, 1, 0.99)
    assert ld.weighting is None and ld.mix is None and ld.storage._replay_dirs == [d1] and ld.storage._replay_dir == d1


def test_train_offline_forwards_mix_and_weighting(monkeypatch):
    import torch
    from exorl_amd import train_offline as T
    seen = {}

    def fake_loader(*a, **k):
        seen['a'], seen['k'] = a, k
        return [None]

    class Agent:
        def update(self, it, step):
            return {}

    monkeypatch.setattr(T, 'make_replay_loader', fake_loader)
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)
    T.train_offline(Agent(), ['d1', 'd2'], 2, 8, 0.99, mix=[0.25, 0.75], weighting='transitions')
    assert seen['a'][1] == ['d1', 'd2'] and seen['k'] == dict(sampler='philox', mix=[0.25, 0.75], weighting='transitions')
    T.train_offline(Agent(), 'd1', 2, 8, 0.99)
    assert seen['k'] == dict(sampler='philox')            # nothing new reaches the loader by default


def test_duplicate_directories_are_refused(tmp_path):
    from exorl_amd.replay_buffer import make_offline_replay_loader
    d1 = _touch(tmp_path / 'a', [(0, 7)])
    with pytest.raises(ValueError, match='listed twice'):
        make_offline_replay_loader(None, [d1, tmp_path / 'a' / '..' / 'a'], 100, 8, 1, 0.99, sampler='philox', mix=[0.5, 0.5])


def test_reorder_gives_empty_slots_weight_zero():
    """Slots that no resident episode holds (one store evicted several episodes, one slot was reused) must not set the scale of the
    quantisation: they get 0, so the largest RESIDENT weight maps to 2^24 and small weights keep their ratios."""
    from exorl_amd.engine import quantise_weights
    from exorl_amd.replay_buffer import _Shard

    class Engine:
        def set_order(self, slots):
            self.order = list(slots)

        def set_weights(self, weighting, w):
            self.weighting, self.w = weighting, None if w is None else np.array(w, np.float64)

    class Loader:
        fetch_every, weighting = 1000, 'transitions'

    sh = _Shard(Loader(), 0)
    sh.engine = Engine()
    sh.fns = ['b', 'c', 'f']
    sh.slot = {'b': 4, 'c': 0, 'f': 2}                          # slots 1 and 3 are holes
    sh.weight = {'b': 1e-9, 'c': 3e-9, 'f': 2e-9}
    sh._reorder()
    assert sh.engine.order == [4, 0, 2] and sh.engine.weighting == 'transitions'
    assert sh.engine.w.tolist() == [3e-9, 0.0, 2e-9, 0.0, 1e-9]
    q = quantise_weights(sh.engine.w).tolist()
    assert q == [1 << 24, 0, int(np.rint(2 / 3 * (1 << 24))), 0, int(np.rint(1 / 3 * (1 << 24)))] == RW.quantise(sh.engine.w)
    sh.weight = {}                                              # no per-episode weights: unit weights, the mode alone
    sh._reorder()
    assert sh.engine.w is None
    Loader.weighting = None                                     # nothing asked for: set_weights is never called
    sh.engine.weighting = 'untouched'
    sh._reorder()
    assert sh.engine.weighting == 'untouched'
