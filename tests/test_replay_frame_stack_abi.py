"""CPU checks of the frame-stacked replay arena: the export, its declaration and binding, stack_frames against the wrapper's deque and
unstack_frames as its inverse (and its refusal of episodes that are no sliding window), and the shape checks of the engine and the loader."""
import ctypes
import re
from collections import deque
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope='module')
def lib():
    return ctypes.CDLL(str(ROOT / 'exorl_amd' / 'libexorl_hip.so'))


def test_symbol_declared_exported_and_bound(lib):
    from exorl_amd import _lib as L
    header = (ROOT / 'include' / 'exorl_hip.h').read_text()
    m = re.search(r'int exorl_replay_set_frame_stack\((.*?)\);', header, re.S)
    assert m, 'exorl_replay_set_frame_stack is not declared in include/exorl_hip.h'
    args = [a.strip() for a in m.group(1).split(',')]
    assert len(args) == 2 and args[0].startswith('exorl_replay_t*') and args[1].startswith('int32_t')
    assert hasattr(lib, 'exorl_replay_set_frame_stack'), 'exorl_replay_set_frame_stack is not exported'
    res, argtypes = L.PROTOTYPES['exorl_replay_set_frame_stack']
    assert res is ctypes.c_int and argtypes == [ctypes.c_void_p, ctypes.c_int32]


def test_abi_version_and_cfg_layout_are_unchanged(lib):
    from exorl_amd import _lib as L
    header = (ROOT / 'include' / 'exorl_hip.h').read_text()
    lib.exorl_abi_version.restype = ctypes.c_int
    assert lib.exorl_abi_version() == 13 and re.search(r'#define EXORL_ABI_VERSION 13\b', header)
    comment = header[header.index('#define EXORL_ABI_VERSION'):header.index('const char* exorl_last_error')]
    assert 'exorl_replay_set_frame_stack' in comment          # the version-12 comment names the additive export
    assert [f[0] for f in L.ReplayCfg._fields_] == ['obs_bytes', 'act_dim', 'meta_dim', 'max_episodes', 'capacity_rows']
    assert ctypes.sizeof(L.ReplayCfg) == 24


def test_null_handle_is_an_error_not_a_crash(lib):
    lib.exorl_replay_set_frame_stack.restype = ctypes.c_int
    lib.exorl_replay_set_frame_stack.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    lib.exorl_last_error.restype = ctypes.c_char_p
    assert lib.exorl_replay_set_frame_stack(None, 3) != 0
    assert b'replay_set_frame_stack' in lib.exorl_last_error()


def _frames(rs, rows, c0=2, hw=3):
    return rs.randint(0, 256, (rows, c0, hw, hw)).astype(np.uint8)


@pytest.mark.parametrize('k', [1, 2, 3, 4])
@pytest.mark.parametrize('transitions', [1, 2, 7])
def test_stack_is_the_wrappers_deque_and_unstack_inverts_it(k, transitions):
    from exorl_amd.replay_buffer import stack_frames, unstack_frames
    f = _frames(np.random.RandomState(10 * k + transitions), transitions + 1)
    d = deque([f[0]] * k, maxlen=k)                       # reset: the deque is filled with the first frame
    want = [np.concatenate(list(d), axis=0)]
    for t in range(1, len(f)):
        d.append(f[t])                                    # step: one frame in, the oldest out
        want.append(np.concatenate(list(d), axis=0))
    s = stack_frames(f, k)
    assert s.shape == (transitions + 1, 2 * k, 3, 3) and s.dtype == f.dtype and np.array_equal(s, np.stack(want))
    back = unstack_frames(s, k)
    assert back.shape == f.shape and np.array_equal(back, f)


def test_unstack_refuses_what_is_not_a_window():
    from exorl_amd.replay_buffer import stack_frames, unstack_frames
    f = _frames(np.random.RandomState(3), 8)
    s = stack_frames(f, 3)
    bad = s.copy()
    bad[5, 1, 2, 0] ^= 1                                  # one byte of the OLDEST frame of row 5: its newest frames are untouched
    with pytest.raises(ValueError, match=r'row 5 does not continue row 4'):
        unstack_frames(bad, 3)
    bad = s.copy()
    bad[0, 0, 0, 0] ^= 1
    with pytest.raises(ValueError, match=r'row 0 is not 3 copies'):
        unstack_frames(bad, 3)
    with pytest.raises(ValueError, match='divide'):
        unstack_frames(s[:, :5], 3)
    bad = s.copy()
    bad[6, -1, 0, 0] ^= 1                                 # a changed NEWEST frame is a different frame sequence: row 7 no longer continues it
    with pytest.raises(ValueError, match=r'row 7 does not continue row 6'):
        unstack_frames(bad, 3)


def test_engine_and_loader_refuse_shapes_that_hold_no_stack(tmp_path):
    """Checked before a device or the library is touched."""
    from exorl_amd.engine import ReplayEngine, frame_shape
    from exorl_amd.replay_buffer import _Shard, make_offline_replay_loader, make_replay_loader
    assert frame_shape((9, 84, 84), 3) == (3, 84, 84) and frame_shape((24,), 1) == (24,) and frame_shape((4, 6, 6), 4) == (1, 6, 6)
    with pytest.raises(ValueError, match='does not divide'):
        ReplayEngine((8, 16, 16), np.uint8, 2, 0, 64, 4, frame_stack=3)
    with pytest.raises(ValueError, match=r'\(channels, H, W\)'):
        ReplayEngine((24,), np.float32, 2, 0, 64, 4, frame_stack=2)
    for k in (0, 17):
        with pytest.raises(ValueError, match='frame_stack'):
            ReplayEngine((9, 16, 16), np.uint8, 2, 0, 64, 4, frame_stack=k)
        with pytest.raises(ValueError, match='frame_stack'):
            make_offline_replay_loader(None, tmp_path, 100, 8, 1, 0.99, frame_stack=k)
    ld = make_replay_loader(None, tmp_path, 100, 8, 1, 0.99, frame_stack=3)            # the 6-argument shape reaches the offline loader
    assert ld.offline and ld.frame_stack == 3
    assert make_offline_replay_loader(None, tmp_path, 100, 8, 1, 0.99).frame_stack is None
    ld = make_replay_loader(None, 1000, 8, 1, True, 3, 0.99, frame_stack=3)
    assert ld.frame_stack == 3 and not ld.offline
    act, one = np.zeros((5, 2), np.float32), np.zeros((5, 1), np.float32)
    for obs in (np.zeros((5, 8, 16, 16), np.uint8), np.zeros((5, 24), np.float32)):     # what the shard does with the first episode it sees
        with pytest.raises(ValueError, match='frame_stack=3'):
            _Shard(ld, 0)._ensure_engine(dict(observation=obs, action=act, reward=one, discount=one))
