"""The float64 convolution reference of the per-layer kernel tests (tests/_conv_ref.py) against the reference's own outputs
(tests/golden/pixels_g5.npz), against the oracle, and the known properties of its bf16 plane emulation. CPU only."""
import numpy as np
import pytest
import torch

import _conv_ref as R
from oracle import pixels

ENC_KEYS = [f'convnet.{i}.{w}' for i in (0, 2, 4, 6) for w in ('weight', 'bias')]


@pytest.mark.parametrize('tag', ['c3', 'c9'])
def test_reference_chained_end_to_end_matches_golden(gold, tag):
    """The helper's layers chained in float64 reproduce the reference encoder's features and every parameter gradient (the golden file's dh:
    RandomState(7), as tests/test_oracle_pixels.py). The reference ran in fp32, so the bars are the oracle's."""
    z = np.load(gold / 'pixels_g5.npz')
    p = [torch.from_numpy(z[f'enc_{tag}_param/{k}']) for k in ENC_KEYS]
    x = torch.from_numpy(z[f'enc_{tag}_x'])
    dh = torch.from_numpy(np.random.RandomState(7).standard_normal((2, 39200)).astype(np.float32))
    h, grads = R.encoder(p, x, dh)
    h = h.numpy()
    np.testing.assert_allclose(h[:, ::97], z[f'enc_{tag}_h_sample'], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose([h.sum(), (h ** 2).sum()], z[f'enc_{tag}_h_sums'], rtol=1e-5)
    for k, g in zip(ENC_KEYS, grads):
        want = z[f'enc_{tag}_grad/{k}']
        np.testing.assert_allclose(g.numpy(), want, rtol=2e-4, atol=2e-5 * np.abs(want).max(), err_msg=k)


@pytest.mark.parametrize('c,stride,hw', [(3, 2, 23), (9, 2, 20), (32, 1, 13)])
def test_layer_functions_match_the_oracle(c, stride, hw):
    """Forward, dgrad, weight and bias gradients of one layer against oracle/pixels.py (fp32 im2col) on the same operands, to fp32 rounding of
    the oracle relative to the element-wise scale."""
    rs = np.random.RandomState(c + hw)
    n = 3
    W = (rs.standard_normal((32, c, 3, 3)) / np.sqrt(9 * c)).astype(np.float32)
    b = (0.1 * rs.standard_normal(32)).astype(np.float32)
    if stride == 2:
        xu = rs.randint(0, 256, (n, c, hw, hw)).astype(np.uint8)
        x = R.pixel_scale(torch.from_numpy(xu))
        np.testing.assert_array_equal(x.numpy(), xu.astype(np.float32) / np.float32(255) - np.float32(0.5))
        ref = R.first_layer_fwd(torch.from_numpy(xu), torch.from_numpy(W), torch.from_numpy(b))
    else:
        x = torch.from_numpy(np.maximum(rs.standard_normal((n, c, hw, hw)), 0).astype(np.float32))
        ref = R.conv_fwd(x, torch.from_numpy(W), torch.from_numpy(b), stride)
    scale = R.conv_fwd(x, torch.from_numpy(W), torch.from_numpy(b), stride, absolute=True)
    y, cols = pixels.conv_fwd(x.numpy(), W, b, stride)
    assert (np.abs(y - ref.numpy()) / scale.numpy()).max() < 1e-6
    dy = rs.standard_normal(y.shape).astype(np.float32)
    dW, db, dx = pixels.conv_bwd(x.shape, cols, W, dy, stride, need_dx=stride == 1)
    gw, gb = R.conv_wgrad(torch.from_numpy(dy), x, stride)
    sw, sb = R.conv_wgrad(torch.from_numpy(dy), x, stride, absolute=True)
    assert (np.abs(dW - gw.numpy()) / sw.numpy()).max() < 1e-6
    assert (np.abs(db - gb.numpy()) / sb.numpy()).max() < 1e-6
    if stride == 1:
        mask = torch.from_numpy(rs.standard_normal(x.shape).astype(np.float32))
        d = R.conv_dgrad(torch.from_numpy(dy), torch.from_numpy(W), mask)
        sd = R.conv_dgrad(torch.from_numpy(dy), torch.from_numpy(W), mask, absolute=True)
        want = dx * (mask.numpy() > 0)
        assert (np.abs(want - d.numpy()) / np.maximum(sd.numpy(), 1e-30)).max() < 1e-6
        assert (d.numpy()[mask.numpy() <= 0] == 0).all()


def test_plane_split_is_round_to_nearest_even_and_exact():
    """hi = bf16(x) rounds to nearest even; the residual planes are bf16 of the exact fp32 residuals; three planes hold every fp32 value."""
    one = 1.0
    x = torch.tensor([one + 2 ** -8, one + 3 * 2 ** -8, -(one + 2 ** -8), one + 2 ** -8 + 2 ** -20], dtype=torch.float32)
    p = R.planes(x, 3)
    assert p[0].tolist() == [1.0, 1.0 + 2 ** -6, -1.0, 1.0 + 2 ** -7]         # ties to even; a value above the tie rounds up
    assert p[1].tolist() == [2 ** -8, -2 ** -8, -2 ** -8, -2 ** -8]            # bf16(2^-20 - 2^-8) = -2^-8: the rest goes to the third plane
    assert p[2].tolist() == [0.0, 0.0, 0.0, 2 ** -20]
    rs = np.random.RandomState(0)
    v = torch.from_numpy((rs.standard_normal(200000) * np.exp(rs.uniform(-20, 20, 200000))).astype(np.float32))
    p = R.planes(v, 3)
    assert torch.equal(p[0] + p[1] + p[2], v.double())
    for q in p:
        assert torch.equal(q, q.float().to(torch.bfloat16).double())             # every plane is a bf16 value
    assert (p[1].abs() <= 2 ** -8 * p[0].abs()).all() and (p[2].abs() <= 2 ** -8 * p[1].abs()).all()


def _products(x, y, mode):
    return R.emulate(lambda a, b: a * b, x, y, mode)


def test_plane_products_error_bounds():
    """Element-wise products against the exact ones. A bf16 rounding moves a value by up to 2^-8 of it (half a unit of 8 significant bits just
    above a power of two), so each plane is at most 2^-8 of the one before it. The two-plane (BF16X3) product misses hi*e_y + e_x*hi + lo*lo, each
    up to 2^-16 of |x y|: bound 3 * 2^-16 (measured 1.7 * 2^-16 here — above 3 * 2^-18, which is NOT a bound). The three-plane (BF16X6) product
    misses only lo*l3 + l3*lo + l3*l3 (three planes hold an fp32 value exactly): the header's 3 * 2^-24. Plain bf16: (1 + 2^-8)^2 - 1."""
    rs = np.random.RandomState(1)
    x = torch.from_numpy((rs.standard_normal(500000) * np.exp(rs.uniform(-8, 8, 500000))).astype(np.float32))
    y = torch.from_numpy((rs.standard_normal(500000) * np.exp(rs.uniform(-8, 8, 500000))).astype(np.float32))
    exact = x.double() * y.double()
    rel = {m: float(((_products(x, y, m) - exact).abs() / exact.abs()).max()) for m in (R.BF16, R.BF16X3, R.BF16X6)}
    print('worst relative product error per mode:', rel)
    assert 3 * 2 ** -18 < rel[R.BF16X3] <= 3 * 2 ** -16
    assert 2 ** -26 < rel[R.BF16X6] <= 3 * 2 ** -24
    assert 2 ** -8 < rel[R.BF16] <= 2 ** -7 + 2 ** -16
    assert torch.equal(_products(x, y, R.EXACT), exact)


def test_three_planes_are_exact_on_integers():
    """Integers up to 2^11 in magnitude take at most two planes, so the three-plane product set (which includes lo * lo) is exact on them;
    the two-plane set (no lo * lo) is not."""
    k = torch.arange(-2 ** 11, 2 ** 11 + 1, dtype=torch.float32)
    x, y = k.repeat_interleave(41), k[torch.randperm(k.numel(), generator=torch.Generator().manual_seed(0))].repeat(41)[:k.numel() * 41]
    exact = x.double() * y.double()
    assert torch.equal(_products(x, y, R.BF16X6), exact)
    assert not torch.equal(_products(x, y, R.BF16X3), exact)


def test_emulation_forms_the_documented_products():
    """emulate() on an element-wise product against the products written out by hand, for every mode, a dropped pair and both groupings."""
    rs = np.random.RandomState(2)
    x = torch.from_numpy(rs.standard_normal(1000).astype(np.float32))
    y = torch.from_numpy(rs.standard_normal(1000).astype(np.float32))
    a, b = R.planes(x, 3), R.planes(y, 3)
    want = {R.BF16: a[0] * b[0],
            R.BF16X3: a[0] * b[0] + a[0] * b[1] + a[1] * b[0],
            R.BF16X6: a[0] * b[0] + a[0] * b[1] + a[1] * b[0] + a[0] * b[2] + a[2] * b[0] + a[1] * b[1]}
    for m, w in want.items():
        for g in ('a', 'b'):
            assert torch.allclose(R.emulate(lambda u, v: u * v, x, y, m, group=g), w, rtol=1e-15, atol=0)
    dropped = R.emulate(lambda u, v: u * v, x, y, R.BF16X6, drop=(1, 0))
    assert torch.allclose(dropped, want[R.BF16X6] - a[1] * b[0], rtol=1e-15, atol=0)
    for i, j in R.PAIRS[R.BF16X6]:
        assert torch.equal(R.plane_term(lambda u, v: u * v, x, y, (i, j)), a[i] * b[j])
    db = R.conv_wgrad(torch.from_numpy(rs.standard_normal((2, 32, 5, 5)).astype(np.float32)), torch.zeros(2, 32, 7, 7), 1, R.BF16X3)[1]
    assert db.dtype == torch.float64 and db.shape == (32,)
