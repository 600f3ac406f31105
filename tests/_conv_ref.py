"""Float64 reference of the pixel encoder's convolutions (ddpg.Encoder: 4 x [Conv2d 3x3 + ReLU], stride 2 then 1), for testing each HIP
convolution kernel on its own inputs. Plain torch ops only (F.unfold + matmul), on whichever device the tensors live; no project code.

The operands are split into bf16 planes the way the kernels split them (pixels.hip, conv_weight_shadow_kernel and the staging code of every
MFMA convolution): hi = bf16(x), second = bf16(x - hi), third = bf16((x - hi) - second), round to nearest even, residuals exact in fp32.
A precision mode then forms exactly the kernels' plane products (pixels.hip, conv1_wgrad_mfma_kernel "plane products by magnitude class"):
  BF16    p0*p0
  BF16X3  p0*p0 + p0*p1 + p1*p0
  BF16X6  the three above + p0*p2 + p2*p0 + p1*p1
  EXACT   the exact product of the fp32 operands (the fp32 FMA kernels)
Products of planes are exact in float64 and so are the sums here (to 2^-53 of the scale), so a kernel result differs from these only by its
fp32 accumulation order. `absolute=True` evaluates the same operation on |operands| (exact values): the element-wise scale errors are
measured against, as the GEMM tests use |A| @ |B| + 1.
"""
import numpy as np
import torch
import torch.nn.functional as F

EXACT, BF16, BF16X3, BF16X6 = 0, 1, 2, 3          # the EXORL_PREC_* values (EXACT = EXORL_PREC_F32: exact fp32 products)
NPLANES = {BF16: 1, BF16X3: 2, BF16X6: 3}
PAIRS = {BF16: ((0, 0),),
         BF16X3: ((0, 0), (0, 1), (1, 0)),
         BF16X6: ((0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1))}


def planes(x, k):
    """fp32 tensor -> its first k bf16 planes, as float64 tensors."""
    r = x.float()
    out = []
    for _ in range(k):
        h = r.to(torch.bfloat16).float()           # round to nearest even
        out.append(h.double())
        r = r - h                                  # exact: h carries the leading bits of r
    return out


def emulate(op, a, b, mode, drop=None, group='a'):
    """op: bilinear in (a, b), evaluated in float64. a, b: fp32 tensors. The sum of the mode's plane products, leaving out the pair `drop`
    (a plane index of a, one of b) if given. group: the operand whose planes each call of op takes alone ('a' or 'b'); the other operand's
    planes of that call are summed first (exactly: bf16 planes of one fp32 value add up without rounding in float64), op being linear."""
    if mode == EXACT:
        assert drop is None
        return op(a.double(), b.double())
    k = NPLANES[mode]
    pa, pb = planes(a, k), planes(b, k)
    pairs = [p for p in PAIRS[mode] if p != drop]
    out = None
    for g in range(k):
        if group == 'a':
            mates = [j for i, j in pairs if i == g]
            term = op(pa[g], sum(pb[j] for j in mates)) if mates else None
        else:
            mates = [i for i, j in pairs if j == g]
            term = op(sum(pa[i] for i in mates), pb[g]) if mates else None
        if term is not None:
            out = term if out is None else out + term
    return out


def plane_term(op, a, b, pair):
    """One plane product alone, float64: op(plane i of a, plane j of b) for pair = (i, j)."""
    i, j = pair
    k = max(i, j) + 1
    return op(planes(a, k)[i], planes(b, k)[j])


def pixel_scale(x):
    """Encoder.forward's x / 255 - 0.5 in fp32 (a true division, as the kernels compute it) for pixel values 0..255 of any dtype."""
    lut = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255.0) - np.float32(0.5)).to(x.device)
    return lut[x.long()]


def _corr(x, w, stride, pad):
    """Cross-correlation (nn.Conv2d without bias): x (n, ci, h, w), w (co, ci, 3, 3), both float64."""
    n, _, h, wd = x.shape
    oh, ow = (h + 2 * pad - 3) // stride + 1, (wd + 2 * pad - 3) // stride + 1
    cols = F.unfold(x, 3, padding=pad, stride=stride)                     # (n, ci * 9, oh * ow)
    return (w.reshape(w.shape[0], -1) @ cols).reshape(n, w.shape[0], oh, ow)


def _flip(w):
    """The dgrad kernel of w (co, ci, 3, 3): (ci, co, 3, 3), taps reversed — d(in) = full correlation of d(out) with it (pad 2)."""
    return w.flip(2, 3).transpose(0, 1)


def conv_fwd(x, w, b, stride, mode=EXACT, drop=None, absolute=False, term=None):
    """Pre-activation of a layer, float64: x (n, ci, h, w) fp32 input of the layer, w (32, ci, 3, 3), b (32,). term = (i, j): that plane
    product's share of it alone (no bias)."""
    if term is not None:
        return plane_term(lambda a, v: _corr(a, v, stride, 0), x, w, term)
    if absolute:
        return _corr(x.double().abs(), w.double().abs(), stride, 0) + b.double().abs()[:, None, None]
    return emulate(lambda a, v: _corr(a, v, stride, 0), x, w, mode, drop) + b.double()[:, None, None]


def first_layer_fwd(x, w, b, mode=EXACT, drop=None, absolute=False):
    """The stride-2 first layer on pixel values x (n, c, hw, hw), scaled to x / 255 - 0.5."""
    return conv_fwd(pixel_scale(x), w, b, 2, mode, drop, absolute)


def conv_dgrad(dy, w, mask, mode=EXACT, drop=None, absolute=False, term=None):
    """d(in) of a stride-1 layer, float64: full correlation (pad 2) of dy (n, 32, oh, ow) with the flipped kernel, times (mask > 0) — the
    ReLU of the layer below, mask = its activation (n, ci, oh + 2, ow + 2). term = (i, j): that plane product's share alone."""
    if term is not None:
        out = plane_term(lambda d, v: _corr(d, _flip(v), 1, 2), dy, w, term)
    elif absolute:
        out = _corr(dy.double().abs(), _flip(w.double().abs()), 1, 2)
    else:
        out = emulate(lambda d, v: _corr(d, _flip(v), 1, 2), dy, w, mode, drop)
    return out * (mask > 0)


def _wgrad_op(stride):
    def op(d, x):
        n, co = d.shape[:2]
        cols = F.unfold(x, 3, stride=stride)                               # (n, ci * 9, oh * ow)
        return torch.bmm(d.reshape(n, co, -1), cols.transpose(1, 2)).sum(0).reshape(co, x.shape[1], 3, 3)
    return op


def _bias_op(d, one):
    return (d * one).sum((0, 2, 3))


def conv_wgrad_sq(dy, x, stride):
    """The weight and bias gradient sums on squared operands (sum of squared terms), float64: their square roots are the root-sum-square scale
    of these long reductions, which sums over whole images and batches."""
    d = dy.double() ** 2
    return _wgrad_op(stride)(d, x.double() ** 2), d.sum((0, 2, 3))


def conv_wgrad_term(dy, x, stride, pair):
    """One plane product's share of the weight gradient alone (plane i of dy, plane j of x), float64."""
    return plane_term(_wgrad_op(stride), dy, x, pair)


def conv_wgrad(dy, x, stride, mode=EXACT, bias_mode=None, drop=None, absolute=False):
    """Weight and bias gradients summed over the batch, float64: dy (n, 32, oh, ow) = d(pre-activation), x (n, ci, h, w) fp32 input of the
    layer. bias_mode (default: mode): the bias gradient as the product of dy with a ones operand in that mode — its planes summed (the tile and
    first-layer kernels), or EXACT for plain fp32 sums of dy (the weight-gradient kernel's producer waves)."""
    bias_mode = mode if bias_mode is None else bias_mode
    if absolute:
        d = dy.double().abs()
        return _wgrad_op(stride)(d, x.double().abs()), d.sum((0, 2, 3))
    dw = emulate(_wgrad_op(stride), dy, x, mode, drop, group='b')
    ones = torch.ones_like(dy)
    db = emulate(_bias_op, dy, ones, bias_mode, drop if bias_mode != EXACT and drop in PAIRS[bias_mode] and drop[1] == 0 else None)
    return dw, db


def encoder(params, x, dh):
    """End to end in float64 and exact products: params [W0, b0, .., W3, b3], x (n, c, hw, hw) pixel values, dh (n, 32 e e) the gradient at the
    flattened features. Returns the features (n, 32 e e) and the eight parameter gradients, all float64."""
    p = [q.double() for q in params]
    a = pixel_scale(x).double()
    acts = [a]
    for l in range(4):
        a = _corr(a, p[2 * l], 2 if l == 0 else 1, 0) + p[2 * l + 1][:, None, None]
        a = a.clamp_min(0)
        acts.append(a)
    d = dh.double().reshape(a.shape) * (a > 0)
    grads = [None] * 8
    for l in range(3, -1, -1):
        grads[2 * l] = _wgrad_op(2 if l == 0 else 1)(d, acts[l])
        grads[2 * l + 1] = d.sum((0, 2, 3))
        if l > 0:
            d = _corr(d, _flip(p[2 * l]), 1, 2) * (acts[l] > 0)
    return a.reshape(a.shape[0], -1), grads
