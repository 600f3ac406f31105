"""CPU checks of the weight-image export (exorl_debug_agent_weight_images) and of the reference the GPU test compares the images with
(tests/_weight_images.py): the symbol, its declaration and binding, the struct, the ABI version, the NULL-argument refusals, the plane
arithmetic on hard values, the layout rules on a small net, and the rows of the header's carve table that show in the workspace size.

Two items need a created agent, which needs a device, and live in tests/test_gpu_weight_images.py: the refusal of a net the agent does not
have, and the carve table held pointer by pointer (which images are NULL) for every case."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import _weight_images as W

ROOT = Path(__file__).resolve().parents[1]
NAME = 'exorl_debug_agent_weight_images'


@pytest.fixture(scope='module')
def lib():
    from exorl_amd import _lib as L
    return L.load()


def test_symbol_declared_exported_and_bound(lib):
    from exorl_amd import _lib as L
    header = (ROOT / 'include' / 'exorl_hip.h').read_text()
    m = re.search(r'int %s\((.*?)\);' % NAME, header, re.S)
    assert m, f'{NAME} is not declared in include/exorl_hip.h'
    assert len(m.group(1).split(',')) == 3
    assert hasattr(ctypes.CDLL(str(ROOT / 'exorl_amd' / 'libexorl_hip.so')), NAME), f'{NAME} is not exported'
    res, args = L.PROTOTYPES[NAME]
    assert res is ctypes.c_int and len(args) == 3
    from exorl_amd.engine import AgentEngine
    assert callable(AgentEngine.weight_images)


def test_struct_matches_the_header():
    from exorl_amd import _lib as L
    header = (ROOT / 'include' / 'exorl_hip.h').read_text()
    body = re.search(r'typedef struct \{([^}]*)\} exorl_weight_images;', header).group(1)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            typ, names = decl.split(None, 1)
            fields += [(n.strip().lstrip('*'), typ.rstrip('*'), '*' in decl) for n in names.split(',')]
    assert [f[0] for f in fields] == [n for n, _ in L.WeightImages._fields_]
    for (name, typ, is_ptr), (_, ctype) in zip(fields, L.WeightImages._fields_):
        assert ctype is (ctypes.c_void_p if is_ptr else ctypes.c_int32), name
        assert is_ptr or typ == 'int32_t', name
    assert ctypes.sizeof(L.WeightImages) == 4 * 4 + 6 * 8


def test_abi_version_is_unchanged(lib):
    header = (ROOT / 'include' / 'exorl_hip.h').read_text()
    assert lib.exorl_abi_version() == 13
    m = re.search(r'#define EXORL_ABI_VERSION 13\b.*?\*/', header, re.S)
    assert m and NAME in m.group(0).split('no version change')[1]


def test_null_arguments_are_refused_with_a_message(lib):
    from exorl_amd import _lib as L
    out = L.WeightImages()
    assert lib.exorl_debug_agent_weight_images(None, L.NET_ACTOR, ctypes.byref(out)) != 0
    assert 'debug_agent_weight_images: null argument' in lib.exorl_last_error().decode()
    # a non-NULL handle with a NULL out: refused before the handle is looked at
    dummy = ctypes.create_string_buffer(64)
    assert lib.exorl_debug_agent_weight_images(ctypes.cast(dummy, ctypes.c_void_p), L.NET_ACTOR, None) != 0
    assert 'debug_agent_weight_images: null argument' in lib.exorl_last_error().decode()


def hard_values():
    """Seeded significands over the exponents at which all three planes are normal or exactly representable bf16 values (the lowest bit
    of x, 2^(e - 23), has to stay above bf16's smallest subnormal 2^-133), both signs; +-0; the largest finite bf16 and its float32
    neighbours on both sides that still round to a finite bf16; values that round up to the next binade."""
    rs = np.random.RandomState(11)
    e = np.repeat(np.arange(-100, 127), 8)
    x = np.ldexp(rs.uniform(1.0, 2.0, e.size), e).astype(np.float32)
    x = np.concatenate([x, -x])
    edge = np.array([0x00000000, 0x80000000, 0x7f7f0000, 0x7f7effff, 0x7f7f0001, 0x7f7f7fff, 0xff7f0000, 0xff7f7fff,
                     0x3f7fffff, 0x3f7f8000, 0x3f808000, 0x3f818000, 0x3f80ffff, 0x3fffffff, 0x00800000, 0x3f800001], np.uint32).view(np.float32)
    return np.concatenate([x, edge])


def test_planes_of_hard_values():
    x = hard_values()
    x64 = x.astype(np.float64)
    hi, mid, lo3 = (W.bf16_value(p).astype(np.float64) for p in W.planes(x, 3))
    assert np.all(np.isfinite(hi))
    assert np.array_equal(hi + mid + lo3, x64), 'hi + mid + lo is not x'
    h2, l2 = (W.bf16_value(p).astype(np.float64) for p in W.planes(x, 2))
    assert np.array_equal(h2, hi) and np.array_equal(l2, mid)       # the two-plane lo is the three-plane mid
    assert np.all(np.abs(x64 - h2 - l2) <= 2.0 ** -16 * np.abs(x64))
    assert np.all(np.abs(x64 - hi) <= 2.0 ** -8 * np.abs(x64))
    # round to nearest EVEN at exact ties, and the sign of zero kept
    bits = lambda *u: W.bf16_bits(np.array(u, np.uint32).view(np.float32)).tolist()
    assert bits(0x3f808000, 0x3f818000, 0x3f808001, 0x3f807fff) == [0x3f80, 0x3f82, 0x3f81, 0x3f80]
    assert bits(0x80000000, 0x00000000) == [0x8000, 0x0000]
    # against the float path: numpy has no bf16, but a bf16 is a float32 with 16 zero bits, so rounding x to 8 significand bits in float64
    # arithmetic gives the same value
    m, e = np.frexp(x64)
    want = np.ldexp(np.rint(m * 256.0), e - 8)         # np.rint rounds half to even
    assert np.array_equal(hi, want)


def test_expected_images_layout():
    """A twin net and a shared-trunk net of recognisable integers: transposition, K padding with zeros and the per-trunk / per-head order."""
    H, I = 4, 3

    def net(n_trunks, n_heads):
        val = iter(range(1, 10 ** 6))
        arr = lambda *shape: np.array([next(val) for _ in range(int(np.prod(shape)))], np.float32).reshape(shape)
        tr = lambda: [arr(H, I), arr(H), arr(H), arr(H)]
        hd = lambda: [arr(H, H), arr(H), arr(1, H), arr(1)]
        return tr() + hd() + tr() + hd() if n_trunks == 2 else tr() + hd() + hd()
    for nt in (2, 1):
        t = net(nt, 2)
        w0 = [t[0], t[8]] if nt == 2 else [t[0]]
        w1 = [t[4], t[12]] if nt == 2 else [t[4], t[8]]
        im = W.expected_images(t, (nt, 2), (2, 3))
        assert im['w0t'].shape == (nt, I, H) and im['w0_hi'].shape == (nt, H, 32) and im['w1_mid'].shape == (2, H, H)
        for k in range(nt):
            assert np.array_equal(im['w0t'][k], w0[k].T)
            assert np.array_equal(W.bf16_value(im['w0_hi'][k, :, :I]) + W.bf16_value(im['w0_lo'][k, :, :I]), w0[k])
            assert not im['w0_hi'][k, :, I:].any() and not im['w0_lo'][k, :, I:].any()
        for k in range(2):
            assert np.array_equal(sum(W.bf16_value(im[n][k]) for n in ('w1_hi', 'w1_mid', 'w1_lo')), w1[k])
    im = W.expected_images(net(1, 2), (1, 2), (0, 0))
    assert [k for k in W.IMAGES if im[k] is not None] == ['w0t']
    im = W.expected_images(net(2, 2), (2, 2), (1, 1))
    assert [k for k in W.IMAGES if im[k] is not None] == ['w0t', 'w0_hi', 'w1_hi']
    other = dict(im, w1_hi=im['w1_hi'].copy())
    other['w1_hi'][1, 2, 3] ^= 1
    assert W.differing(other, im) == ['w1_hi'] and W.differing(im, im) == []
    assert '1 of 32 elements differ, first at (1, 2, 3)' in W.first_difference(other, im, 'w1_hi')


# one configuration per row of the carve table in include/exorl_hip.h: (precision, kind, O, A, H, B, planes of W0, planes of W1)
CARVE_ROWS = [('bf16', 0, 24, 8, 128, 8, 1, 1), ('bf16x3', 0, 24, 6, 128, 64, 2, 2), ('bf16x6', 0, 24, 6, 128, 128, 0, 3),
              ('fp32', 0, 5, 1, 100, 7, 0, 0), ('bf16x3', 0, 5, 1, 100, 7, 0, 0), ('bf16x3', 0, 24, 6, 64, 64, 0, 0), ('bf16x3', 0, 24, 6, 128, 72, 0, 0),
              ('bf16x6', 1, 24, 6, 64, 128, 0, 0), ('bf16x6', 0, 24, 6, 128, 64, 0, 0)]


@pytest.mark.parametrize('row', CARVE_ROWS, ids=lambda r: f'{r[0]}-H{r[4]}B{r[5]}')
def test_carve_table_in_the_workspace_size(lib, row):
    """planes_for restates the header's table; the library's own carve is visible without a device in exorl_agent_workspace_bytes: a
    configuration the table gives no bf16 image has exactly fp32 mode's workspace (same buffers, same order), one it gives images a larger
    one. (Which pointer is NULL is held on the GPU, where an agent can be created.)"""
    from exorl_amd import _lib as L
    from exorl_amd.engine import PRECISION
    precision, kind, O, A, H, B, p0, p1 = row
    assert W.planes_for(precision, H, B) == (p0, p1)
    cfg = lambda prec: L.AgentCfg(kind, O, A, H, B, PRECISION[prec], 1, 0, 1e-4, 0.01, 2.5, 0.3, 0, 10, 1, 3, 0, 5.0, 0)
    size, base = lib.exorl_agent_workspace_bytes(ctypes.byref(cfg(precision))), lib.exorl_agent_workspace_bytes(ctypes.byref(cfg('fp32')))
    assert base > 0
    if (p0, p1) == (0, 0):
        assert size == base
    else:
        assert size > base
