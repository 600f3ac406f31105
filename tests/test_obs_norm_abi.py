"""CPU checks of observation normalisation in the HBM replay: the two exports, their declaration and binding, the unchanged ABI version and
replay configuration, the three host definitions (combine_moments, obs_normalizer, normalize_obs) against the references in
tests/_obs_norm.py, and the keyword plumbing and refusals of the loaders and train_offline."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import _obs_norm as N

ROOT = Path(__file__).resolve().parents[1]
NAMES = {'exorl_replay_obs_moments': 6, 'exorl_replay_set_obs_norm': 5}


@pytest.fixture(scope='module')
def lib():
    return ctypes.CDLL(str(ROOT / 'exorl_amd' / 'libexorl_hip.so'))


def test_symbols_declared_exported_and_bound(lib):
    from exorl_amd import _lib as L
    header = (ROOT / 'include' / 'exorl_hip.h').read_text()
    for name, nargs in NAMES.items():
        m = re.search(r'int %s\((.*?)\);' % name, header, re.S)
        assert m, f'{name} is not declared in include/exorl_hip.h'
        declared = [a for a in m.group(1).split(',') if a.strip()]
        assert len(declared) == nargs
        assert hasattr(lib, name), f'{name} is not exported'
        res, args = L.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == len(declared)          # one ctypes entry per declared parameter


def test_abi_version_and_replay_cfg_are_unchanged(lib):
    from exorl_amd import _lib as L
    header = (ROOT / 'include' / 'exorl_hip.h').read_text()
    lib.exorl_abi_version.restype = ctypes.c_int
    assert lib.exorl_abi_version() == 13
    assert re.search(r'#define EXORL_ABI_VERSION 13\b', header)
    comment = header[header.index('#define EXORL_ABI_VERSION'):header.index('const char* exorl_last_error')]
    for name in NAMES:
        assert name in comment                       # the version-12 comment names the additive exports
    assert ctypes.sizeof(L.ReplayCfg) == 24
    assert [f[0] for f in L.ReplayCfg._fields_] == ['obs_bytes', 'act_dim', 'meta_dim', 'max_episodes', 'capacity_rows']


def test_null_handle_is_an_error_not_a_crash(lib):
    lib.exorl_last_error.restype = ctypes.c_char_p
    for name, nargs in NAMES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32] + [ctypes.c_void_p] * (nargs - 2)
        assert fn(None, 3, *([None] * (nargs - 2))) != 0
        assert name[len('exorl_'):].encode() in lib.exorl_last_error()


# ---- combine_moments ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('O', [1, 3, 24, 65, 78])
def test_combine_moments_on_random_partitions(O):
    from exorl_amd.utils import combine_moments
    x = np.concatenate([ep['observation'] for ep in N.norm_episodes(11, N.LENGTHS, O, 2)]).astype(np.float64)
    ref = N.two_pass(x)
    rs = np.random.RandomState(O)
    for trial in range(6):
        cuts = np.sort(rs.choice(np.arange(1, len(x)), size=[1, 4, 9, 40, 200, 3][trial], replace=False)).tolist()
        if trial == 5:
            cuts = [1, 2, len(x) - 1]                # single-row parts at both ends
        edges = [0] + cuts + [len(x)]
        parts = [N.two_pass(x[a:b]) for a, b in zip(edges[:-1], edges[1:])]
        empty = (0, np.zeros(O), np.zeros(O))
        parts = [empty] + parts[:2] + [empty, empty] + parts[2:] + [empty]
        got = combine_moments(parts)
        N.check_moments(got, ref, f'O={O} trial {trial}')
        want = N.chan([(n, m, s) for n, m, s in parts])
        assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])       # the restated merge, bit for bit
        assert got[1].dtype == np.float64 and got[2].dtype == np.float64


def test_combine_moments_skips_empty_parts_and_keeps_list_order():
    from exorl_amd.utils import combine_moments
    a, b = (3, np.float64([1.0, 2.0]), np.float64([0.5, 0.0])), (5, np.float64([2.0, 2.0]), np.float64([1.5, 0.0]))
    z = (0, np.float64([9e9, 9e9]), np.float64([9e9, 9e9]))              # an empty part's arrays are never read into the result
    n, mean, m2 = combine_moments([z, a, z, b])
    assert n == 8 and mean.tolist() == [1.0 + 1.0 * (5 / 8), 2.0] and m2.tolist() == [0.5 + 1.5 + 1.0 * (3 * 5 / 8), 0.0]
    assert combine_moments([a])[1].tolist() == [1.0, 2.0]
    assert combine_moments([z, z])[0] == 0 and combine_moments([])[0] == 0


# ---- obs_normalizer / normalize_obs ---------------------------------------------------------------------------------------------------
def test_obs_normalizer_is_the_rounded_float64_reciprocal():
    from exorl_amd.utils import obs_normalizer
    n, mean, m2 = N.moments_of(N.norm_episodes(5, N.LENGTHS, 24, 2))
    for eps in (1e-3, 1e-6, 0.25):
        mean32, inv32 = obs_normalizer(n, mean, m2, eps)
        assert mean32.dtype == np.float32 and inv32.dtype == np.float32
        assert np.array_equal(mean32, mean.astype(np.float32))
        assert np.array_equal(inv32, (1.0 / (np.sqrt(m2 / n) + eps)).astype(np.float32))       # population std, one rounding
        rm, ri = N.normalizer(n, mean, m2, eps)
        assert np.array_equal(N.bits(mean32), N.bits(rm)) and np.array_equal(N.bits(inv32), N.bits(ri))
    assert obs_normalizer(n, mean, m2)[1][2] == np.float32(1.0 / 1e-3)                          # the constant column: std 0, default eps 1e-3
    assert inspect.signature(obs_normalizer).parameters['eps'].default == 1e-3


def test_normalize_obs_is_the_two_operation_formula():
    from exorl_amd.utils import normalize_obs, obs_normalizer
    eps = N.norm_episodes(6, [40, 7], 24, 2)
    mean32, inv32 = obs_normalizer(*N.moments_of(eps))
    x = eps[0]['observation']
    got = normalize_obs(x, mean32, inv32)
    assert got.dtype == np.float32 and got.shape == x.shape
    d = (x - mean32).astype(np.float32)
    assert np.array_equal(N.bits(got), N.bits((d * inv32).astype(np.float32)))
    assert np.array_equal(N.bits(got), N.bits(N.normalize(x, mean32, inv32)))
    want = np.array([[np.float32(np.float32(a) - m) * w for a, m, w in zip(row, mean32, inv32)] for row in x[:5]], np.float32)
    assert np.array_equal(N.bits(got[:5]), N.bits(want))                                      # element by element in scalar float32
    assert np.array_equal(normalize_obs(x.astype(np.float64)[3], mean32, inv32), got[3])       # a float64 row from an environment is rounded first


# ---- keyword plumbing and refusals ------------------------------------------------------------------------------------------------------
def test_loader_refusals_and_defaults(tmp_path):
    from exorl_amd.replay_buffer import DeviceReplayLoader, make_offline_replay_loader, make_replay_loader
    from exorl_amd.train_offline import train_offline
    sig = inspect.signature(DeviceReplayLoader.__init__).parameters
    assert sig['normalize_obs'].default is False and sig['norm_eps'].default == 1e-3 and sig['gather'].default is None
    assert inspect.signature(train_offline).parameters['normalize_obs'].default is False
    d = tmp_path / 'a'
    d.mkdir()
    (d / 'episode_0_7.npz').touch()

    class Storage:
        _replay_dir, _meta_specs = d, ()

    with pytest.raises(ValueError, match='offline'):
        make_replay_loader(Storage(), 100, 8, 1, True, 1, 0.99, normalize_obs=True)            # an online, growing buffer
    with pytest.raises(ValueError, match='offline'):
        DeviceReplayLoader(Storage(), 100, 8, 1, True, 1, 0.99, normalize_obs=True)
    with pytest.raises(ValueError, match='frame_stack'):
        make_offline_replay_loader(None, d, 100, 8, 1, 0.99, normalize_obs=True, frame_stack=3)
    ld = make_replay_loader(None, d, 100, 8, 1, 0.99, normalize_obs=True, norm_eps=0.5, frame_stack=1)      # the 6-argument offline shape
    assert ld.offline and ld.normalize_obs is True and ld.norm_eps == 0.5
    ld = make_offline_replay_loader(None, d, 100, 8, 1, 0.99)
    assert ld.normalize_obs is False and ld.norm_eps == 1e-3 and iter(ld).obs_normalizer is None


def test_train_offline_forwards_normalize_obs_and_hands_the_pair_to_the_agent(monkeypatch):
    import torch
    from exorl_amd import train_offline as T
    seen, calls = {}, []

    class Iter:
        obs_normalizer = ('mean32', 'inv32')

        def __iter__(self):
            return self

        def __next__(self):
            raise StopIteration

    def fake_loader(*a, **k):
        seen['k'] = k
        return Iter()

    class Agent:
        def set_obs_normalizer(self, mean32, inv32):
            calls.append(('norm', mean32, inv32))

        def enable_graph(self, it, step):
            calls.append(('graph',))

        def update(self, it, step):
            return {}

    monkeypatch.setattr(T, 'make_replay_loader', fake_loader)
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)
    T.train_offline(Agent(), 'd1', 2, 8, 0.99, normalize_obs=True)
    assert seen['k'] == dict(sampler='philox', normalize_obs=True)
    assert calls == [('norm', 'mean32', 'inv32'), ('graph',)]                   # the normaliser first: the capture sees it
    calls.clear()
    T.train_offline(Agent(), 'd1', 2, 8, 0.99)
    assert seen['k'] == dict(sampler='philox') and calls == [('graph',)]


def test_engine_refuses_a_uint8_arena():
    from exorl_amd.engine import ReplayEngine
    eng = object.__new__(ReplayEngine)            # no device needed: the dtype is checked before the library is touched
    eng.obs_dtype, eng.obs_bytes = np.dtype(np.uint8), 9 * 84 * 84
    for call in (lambda: ReplayEngine.obs_moments(eng), lambda: ReplayEngine.set_obs_normalizer(eng, [0.0], [1.0]),
                 lambda: ReplayEngine.clear_obs_normalizer(eng)):
        with pytest.raises(ValueError, match='float32'):
            call()


def test_pixel_agents_refuse_a_normaliser():
    from exorl_amd import agents
    ag = object.__new__(agents.DDPGAgent)
    ag.obs_type = 'pixels'
    with pytest.raises(ValueError, match='pixel'):
        ag.set_obs_normalizer(np.zeros(3, np.float32), np.ones(3, np.float32))
