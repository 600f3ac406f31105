"""Every convolution kernel of the pixel encoder, layer by layer, against a float64 reference computed from the inputs the GPU itself produced
(tests/_conv_ref.py), at the batch sizes and geometries where the kernels change form.

Forward and backward run through the ABI (exorl_encoder_forward_prec / exorl_encoder_backward_prec); the intermediate maps are read out of the
workspace (act[1..4], then d(act)[1..3], each rounded up to 64 floats, as enc_carve lays them out). Then, per layer l:
  forward        act[l + 1]  against relu(ref(act[l]))                     (act[0] = the pixels, scaled x / 255 - 0.5)
  top mask       d[4]        bit for bit where(act[4] > 0, dh, 0)
  dgrad          d[l]        against (act[l] > 0) * ref(d[l + 1])           (l = 1..3)
  weight / bias  dW[l], db[l] against ref(d[l + 1], act[l]) summed over all images
The ReLU masks come from the GPU's own activations, so no ReLU can flip between kernel and reference, and no error carries over from one layer
to the next: what separates kernel and reference is the kernel's fp32 accumulation order, and any plane product the kernel does not form
(below: the coefficients). The reference forms the mode's plane products exactly (EXACT for
EXORL_PREC_F32 and for the first layer's forward, which is the fp32 strip kernel in every mode). The error of an element is |got - ref| over
the element-wise scale (the same operation on |operands|, + |bias|): finer than a per-image normalisation, so an error confined to one image
of one persistent workgroup is not diluted by the rest of the batch. Where that scale is 0 the kernel must return exactly 0.

Bars. 2e-6 against the element-wise scale for every output, weight and bias gradients included (the GEMM tests' bar; measured worst on an
MI355X: 4.5e-7 forward / dgrad in fp32, 3.3e-7 in the split modes, 2.2e-7 weight gradients). The weight and bias gradients sum whole images and
the batch, and against the sum of |terms| a dropped product of random sign shrinks like 1 / sqrt(terms): at batch 1024 it is no longer 10x above
any bar that fp32 accumulation could meet. So they are also held to 1e-5 against their root-sum-square scale sqrt(sum of squared terms),
under which a dropped lo-plane product stays at ~2^-9. That bound is derived from the accumulation order: a sequential fp32 sum of k terms
errs by a random walk of ~2^-24 sqrt(k / 2) of that scale; the longest chain is the fp32 weight-gradient kernel's (one thread walks an image's
1521 pixels of a 39 x 39 map: 1.7e-6 per standard deviation; the column sum over images adds 32-term chains); MFMA chains are 16x shorter.
Measured worst: 3.7e-6 fp32, 2.0e-6 plain bf16, 1.4e-6 split modes.

Sensitivity, on the same data: each bar is at least 10x smaller than (a) the difference the reference shows when the largest cross-plane
product (lo plane of the first operand x hi plane of the second) is dropped, in the split modes (forward / dgrad: on the first chunk of
images, a lower bound); (b) the weight-gradient reference with the batch's last image left out. The smallest class of the three-plane mode
(hi*l3, l3*hi, lo*lo: ~2^-16 of a product) moves a result by about as much as fp32 accumulation does, so no bar on the worst error can see
it. Every cross product of the split modes is therefore also tested by regression: the coefficient of the kernel's error (got - ref) on
delta = (reference without that product) - reference, over the layer's outputs (forward / dgrad: the first chunk; weight gradients: the
whole batch). A kernel that forms the product gives a coefficient near 0 (fp32 rounding is uncorrelated with a plane product), one that
leaves it out gives 1; the bar is |coefficient| <= 0.1. Every case prints its worst error per layer, the margin (x bar / error), both ratios
(x difference / bar) and the largest |coefficient| with its product (@ij: plane i of the first operand, plane j of the second).

Operand splits read off the kernels: every MFMA convolution stages hi / second / third planes exactly as conv_weight_shadow_kernel splits the
weights (conv3x3_mfma_kernel, conv3x3_ws_kernel and conv_wgrad_ws_kernel producers, conv_wgrad_mfma_kernel's pack, conv1_wgrad_mfma_kernel's
in-register planes), and forms the products of its mode. Two deviations from "every product on planes": the first layer's forward is the
fp32 strip kernel in every mode (exact products), and conv_wgrad_ws_kernel's producer waves sum the bias gradient from fp32 dy (exact), where
the tile and first-layer kernels multiply dy's planes by a ones operand — in plain-bf16 mode the two paths' bias gradients differ by bf16
rounding of dy. conv_wgrad_ws_kernel in the three-plane mode also gathers all five cross products in one accumulator (order only).

Paths (pixels.hip): n <= 8 gives the one-pass-per-workgroup launch of the forward / dgrad kernels, 9 <= n <= #CUs the persistent
conv3x3_ws_kernel with one image per workgroup, n > #CUs several images per workgroup — except the three-plane dgrad, which never takes the
persistent form (!(npl == 3 && mask) in conv3x3_mfma: one image per workgroup at every n > 8); the 32 -> 32 weight gradients take conv_wgrad_ws_kernel
where it fits (maps of >= 384 pixels) and conv_wgrad_mfma_kernel elsewhere; the first layer is conv1_strip_kernel forward and
conv1_wgrad_mfma_kernel (modes 1-3) or conv_wgrad_kernel (fp32); fp32 mode runs conv3x3_kernel / conv_wgrad_kernel for the other layers.
exorl_gemm_tune selects the reference paths (strip forward / dgrad, tile weight gradients, per-image ws)."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import _conv_ref as R

pytestmark = pytest.mark.gpu

BAR = 2e-6
WBAR = 1e-5                 # weight / bias gradients against their root-sum-square scale (derived in the module docstring)
TUNE_STRIP, TUNE_WGRAD_TILE, TUNE_PER_IMAGE = 1073741824, 64, 8388608
CHUNK = 128                 # images per reference chunk (float64 im2col of a 41 x 41 map: 3.5 MB per image)
DROP = (1, 0)               # the cross-plane product left out for sensitivity (a): lo plane of the first operand x hi plane of the second
BETA_BAR = 0.1              # |coefficient of the error on a plane product| (module docstring): 1 when the kernel leaves that product out


@pytest.fixture(scope='module')
def lib():
    from exorl_amd import _lib as L
    return L.load()


@pytest.fixture(scope='module')
def ncu(lib):
    from exorl_amd import _lib as L
    v = C.c_int(0)
    L.check(lib.exorl_device_info(None, 0, C.byref(v), None))
    assert v.value > 0
    return v.value


def edges(hw):
    e1 = (hw - 3) // 2 + 1
    return [hw, e1, e1 - 2, e1 - 4, e1 - 6]


def ru64(k):
    return (k + 63) // 64 * 64


def wgrad_ws(oh, tune):
    """Mirrors conv_wgrad_ws_fits (pixels.hip; if the dispatch changes, change this too — plain-bf16 mode then fails on the bias gradient):
    conv_wgrad_ws_kernel takes the 32 -> 32 weight gradients of maps of >= 3 passes (384 pixels); its other conditions (width 16..46, rows
    per pass, LDS, 32-bit offsets) hold at every geometry here. Its bias gradient is a plain fp32 sum of dy (producer waves), not a product."""
    return not (tune & TUNE_WGRAD_TILE) and oh * oh >= 384


def make_inputs(seed, n, c, hw, kind, device='cuda'):
    """He-scaled weights, small biases, random pixels, dh ~ N(0, 1). kind 'edge': image 0 all 0, image n - 1 all 255, and four channels of
    the second layer dead (bias -50: act[2] is 0 there for every image). kind 'zero_dh': dh = 0 (every gradient exactly 0)."""
    rs = np.random.RandomState(seed)
    p = []
    for l in range(4):
        ci = c if l == 0 else 32
        p += [(rs.standard_normal((32, ci, 3, 3)) * np.sqrt(2.0 / (ci * 9))).astype(np.float32), (0.1 * rs.standard_normal(32)).astype(np.float32)]
    x = rs.randint(0, 256, (n, c, hw, hw)).astype(np.uint8)
    e4 = edges(hw)[4]
    dh = rs.standard_normal((n, 32 * e4 * e4)).astype(np.float32)
    if kind == 'edge':
        x[0] = 0
        x[-1] = 255
        p[3][:4] = -50.0
    if kind == 'zero_dh':
        dh[:] = 0
    return [torch.from_numpy(q).to(device) for q in p], torch.from_numpy(x).to(device), torch.from_numpy(dh).to(device)


def run_encoder(lib, params, x, dh, mode, tune):
    """Forward + backward through the ABI on a NaN-filled workspace; returns the maps the kernels wrote (views into the workspace) and grads."""
    from exorl_amd import _lib as L
    n, c, hw, _ = x.shape
    e = edges(hw)
    flat = torch.zeros(lib.exorl_encoder_param_floats(c, hw), device='cuda')
    offs, off = [], 0
    for q in params:
        flat[off:off + q.numel()] = q.reshape(-1)
        offs.append(off)
        off += (q.numel() + 3) // 4 * 4
    X = x.float().contiguous()
    ws = torch.full((lib.exorl_encoder_workspace_floats(n, c, hw),), float('nan'), device='cuda')
    DH = dh.clone()
    G = torch.full_like(flat, float('nan'))
    hp = C.c_void_p()
    if tune:
        lib.exorl_gemm_tune(tune)
    try:
        L.check(lib.exorl_encoder_forward_prec(flat.data_ptr(), c, hw, X.data_ptr(), n, ws.data_ptr(), C.byref(hp), mode, None))
        L.check(lib.exorl_encoder_backward_prec(flat.data_ptr(), c, hw, X.data_ptr(), n, ws.data_ptr(), DH.data_ptr(), G.data_ptr(), mode, None))
        torch.cuda.synchronize()
    finally:
        lib.exorl_gemm_tune(-1)
    act, dact, o = {}, {}, 0                                    # enc_carve: act[1..4], then d(act)[1..3]
    for l in range(1, 5):
        act[l] = ws[o:o + n * 32 * e[l] ** 2].view(n, 32, e[l], e[l])
        o += ru64(n * 32 * e[l] ** 2)
    for l in range(1, 4):
        dact[l] = ws[o:o + n * 32 * e[l] ** 2].view(n, 32, e[l], e[l])
        o += ru64(n * 32 * e[l] ** 2)
    assert hp.value == act[4].data_ptr(), 'the mirrored act[4] offset is not h_out'
    grads = [G[q:q + p.numel()].view(p.shape) for q, p in zip(offs, params)]
    return act, dact, DH.view(n, 32, e[4], e[4]), grads


def rel_err(got, ref, scale):
    """max |got - ref| / scale; exact equality required where the scale is 0. A NaN (an unwritten element) counts as an infinite error, so
    that Python's max() over chunks and tensors cannot drop it."""
    e = (got.double() - ref).abs() / scale.clamp_min(1e-300)
    return float(torch.where(torch.isnan(e), torch.full_like(e, float('inf')), e).max())


def coef(err, delta):
    """Least-squares coefficient of the kernel's error on delta = (reference without one plane product) - reference: ~0 when the kernel forms
    that product, 1 when it leaves it out. None where delta is 0 everywhere (no gradient to test)."""
    den = float((delta * delta).sum())
    return float((err * delta).sum()) / den if den > 0 else None


def check_layers(params, x, dh, mode, tune, maps):
    """Measures every layer of one run (maps: what run_encoder returned) against the reference. Returns {name: {'err': worst error, 'bar': its
    bar, 'drop': sensitivity (a), 'last': sensitivity (b), 'beta': {cross product: coefficient}}} (absent entries: not applicable)."""
    n, dv = x.shape[0], x.device
    act, dact, d4, grads = maps
    named = [(f'act{l}', act[l]) for l in act] + [(f'dact{l}', dact[l]) for l in dact] + [('d4', d4)] + [(f'grad{i}', g) for i, g in enumerate(grads)]
    for k, t in named:                                          # the workspace starts as NaN: every map read back was written
        assert bool(torch.isfinite(t).all()), f'{k}: non-finite elements'
    res = {}
    assert torch.equal(d4, torch.where(act[4] > 0, dh.view_as(d4), torch.zeros_like(d4))), 'top ReLU mask'
    res['mask4'] = {'err': 0.0, 'bar': 0.0}
    W, B = params[0::2], params[1::2]
    cross = R.PAIRS[mode][1:] if mode in (R.BF16X3, R.BF16X6) else ()
    d = {4: d4, 3: dact[3], 2: dact[2], 1: dact[1]}
    xs = R.pixel_scale(x)                                       # act[0] as the kernels form it
    for l in range(4):
        lm = R.EXACT if (l == 0 or mode == 0) else mode         # the first layer's forward is the fp32 strip kernel in every mode
        r = res[f'fwd{l}'] = {'err': 0.0, 'bar': BAR}
        stride = 2 if l == 0 else 1
        for s in range(0, n, CHUNK):
            a, got = (xs if l == 0 else act[l])[s:s + CHUNK], act[l + 1][s:s + CHUNK]
            ref = R.conv_fwd(a, W[l], B[l], stride, lm)
            scale = R.conv_fwd(a, W[l], B[l], stride, absolute=True)
            r['err'] = max(r['err'], rel_err(got, ref.clamp_min(0), scale))
            if s == 0 and lm != R.EXACT and cross:              # on the first chunk of images (for (a): a lower bound of the batch's)
                r['beta'] = {}
                for pq in cross:
                    delta = (ref - R.conv_fwd(a, W[l], B[l], stride, term=pq)).clamp_min(0) - ref.clamp_min(0)
                    r['beta'][pq] = coef(got.double() - ref.clamp_min(0), delta)
                    if pq == DROP:
                        r['drop'] = rel_err(delta, torch.zeros_like(delta), scale)
            del ref, scale
    for l in range(3, 0, -1):
        r = res[f'dgrad{l}'] = {'err': 0.0, 'bar': BAR}
        for s in range(0, n, CHUNK):
            dy, m, got = d[l + 1][s:s + CHUNK], act[l][s:s + CHUNK], d[l][s:s + CHUNK]
            ref = R.conv_dgrad(dy, W[l], m, mode)
            scale = R.conv_dgrad(dy, W[l], m, absolute=True)
            r['err'] = max(r['err'], rel_err(got, ref, scale))
            if s == 0 and cross:
                r['beta'] = {}
                for pq in cross:
                    delta = -R.conv_dgrad(dy, W[l], m, term=pq)
                    r['beta'][pq] = coef(got.double() - ref, delta)
                    if pq == DROP:
                        r['drop'] = rel_err(delta, torch.zeros_like(delta), scale)
            del ref, scale
    for l in range(4):
        stride = 2 if l == 0 else 1
        bmode = mode if (l == 0 or mode == 0 or not wgrad_ws(edges(x.shape[2])[l + 1], tune)) else R.EXACT
        zero = lambda: [torch.zeros(W[l].shape, dtype=torch.float64, device=dv), torch.zeros(32, dtype=torch.float64, device=dv)]
        ref, l1, sq = zero(), zero(), zero()
        terms = {pq: torch.zeros_like(ref[0]) for pq in cross}
        for s in range(0, n, CHUNK):
            dy, a = d[l + 1][s:s + CHUNK], (xs if l == 0 else act[l])[s:s + CHUNK]
            for acc, v in ((ref, R.conv_wgrad(dy, a, stride, mode, bmode)), (l1, R.conv_wgrad(dy, a, stride, absolute=True)),
                           (sq, R.conv_wgrad_sq(dy, a, stride))):
                acc[0] += v[0]
                acc[1] += v[1]
            for pq in cross:
                terms[pq] += R.conv_wgrad_term(dy, a, stride, pq)
        rss = [v.sqrt() for v in sq]
        last = R.conv_wgrad(d[l + 1][n - 1:], (xs if l == 0 else act[l])[n - 1:], stride, mode, bmode)
        res[f'wgrad{l}'] = {'err': max(rel_err(grads[2 * l], ref[0], l1[0]), rel_err(grads[2 * l + 1], ref[1], l1[1])), 'bar': BAR}
        r = res[f'wgrad{l}-rss'] = {'err': max(rel_err(grads[2 * l], ref[0], rss[0]), rel_err(grads[2 * l + 1], ref[1], rss[1])), 'bar': WBAR,
                                    'last': max(rel_err(last[0], 0 * last[0], rss[0]), rel_err(last[1], 0 * last[1], rss[1]))}
        if cross:
            r['beta'] = {pq: coef(grads[2 * l].double() - ref[0], -t) for pq, t in terms.items()}
            r['drop'] = rel_err(terms[DROP], 0 * terms[DROP], rss[0])
    return res


def report_and_assert(tag, res, zero_grads=False):
    """Prints every entry (error and margin = bar / error; sensitivities as difference / bar; the largest |coefficient| and its product) and
    asserts all of them. zero_grads: dh = 0, so there is no gradient to be sensitive to."""
    lines, bad = [], []
    for k, r in res.items():
        err, bar = r['err'], r['bar']
        s = f'{k} {err:.1e} (x{bar / err:.0f})' if err > 0 else f'{k} exact'
        if 'drop' in r:
            s += f' drop x{r["drop"] / bar:.0f}'
        if 'last' in r:
            s += f' last x{r["last"] / bar:.0f}'
        if not err <= bar:
            bad.append((k, 'error', err))
        if 'beta' in r:
            known = {pq: b for pq, b in r['beta'].items() if b is not None}
            if known:
                pq, b = max(known.items(), key=lambda kv: abs(kv[1]))
                s += f' beta {b:+.3f}@{pq[0]}{pq[1]}'
                bad += [(k, f'coefficient on product {pq}', b) for pq, b in known.items() if not abs(b) <= BETA_BAR]
            if not zero_grads and len(known) < len(r['beta']):
                bad.append((k, 'no data for a coefficient', r['beta']))
        if not zero_grads:
            if 'drop' in r and not r['drop'] >= 10 * bar:
                bad.append((k, 'sensitivity (a)', r['drop']))
            if 'last' in r and not r['last'] >= 10 * bar:
                bad.append((k, 'sensitivity (b)', r['last']))
        lines.append(s)
    print(f'\n{tag}: ' + ' | '.join(lines))
    assert not bad, (tag, bad)


def cases():
    """(c, hw, n as a function of the CU count, modes, exorl_gemm_tune bits, inputs). Kernels per case, modes 1-3 (mode 0 runs
    conv1_strip_kernel, conv3x3_kernel and conv_wgrad_kernel everywhere; the first layer is conv1_strip_kernel forward and
    conv1_wgrad_mfma_kernel<NPL, 1> (c = 3) or <NPL, 3> (c = 9) in every case):
      n = 1, 8          conv3x3_ws_kernel one pass per workgroup (forward, dgrad); conv_wgrad_ws_kernel (maps 39^2, 37^2, 35^2)
      n = 9, #CUs       conv3x3_ws_kernel persistent, one image per workgroup (bf16x6 dgrad: per image); conv_wgrad_ws_kernel
      n = #CUs+1, 4#CUs persistent, several images on some / all workgroups (bf16x6 dgrad: per image); conv_wgrad_ws_kernel
      hw 64, n = 2      one pass per workgroup on maps 31 / 29 / 27 / 25 (ragged last pass); conv_wgrad_ws_kernel
      hw 64, n = 1000   persistent with a ragged tail (1000 images over #CUs workgroups); conv_wgrad_ws_kernel
      c 9, n = 3 / #CUs+1  9-channel strip forward and NT = 3 first-layer weight gradients; one pass / persistent forward and dgrad
      hw 48, n = 300    persistent on maps 21 / 19 / 17; weight gradients: conv_wgrad_ws_kernel (21^2), conv_wgrad_mfma_kernel (19^2, 17^2)
      tune strip | tile conv3x3_mfma_kernel (forward, dgrad) and conv_wgrad_mfma_kernel, n = #CUs+1
      tune per image    conv3x3_ws_kernel one image per workgroup (forward, dgrad), n = #CUs+1
      edge, zero_dh     the product path of n = #CUs+1 / n = 9 on constant images and dead channels / a zero dh"""
    out = []
    for n in ('1', '8', '9', 'ncu', 'ncu+1', '4ncu'):
        out.append((3, 84, n, (0, 1, 2, 3), 0, 'rand'))
    out.append((3, 64, '2', (0, 1, 2, 3), 0, 'rand'))
    out.append((3, 64, '1000', (1, 2, 3), 0, 'rand'))
    out.append((9, 84, '3', (0, 1, 2, 3), 0, 'rand'))
    out.append((9, 84, 'ncu+1', (1, 2, 3), 0, 'rand'))
    out.append((3, 48, '300', (2, 3), 0, 'rand'))
    out.append((3, 84, 'ncu+1', (1, 2, 3), TUNE_STRIP | TUNE_WGRAD_TILE, 'rand'))
    out.append((3, 84, 'ncu+1', (1, 2, 3), TUNE_PER_IMAGE, 'rand'))
    out.append((3, 84, 'ncu+1', (2, 3), 0, 'edge'))
    out.append((3, 84, '9', (0, 2, 3), 0, 'zero_dh'))
    return [pytest.param(*cs, id=f'c{cs[0]}-hw{cs[1]}-n{cs[2]}-t{cs[4]}-{cs[5]}') for cs in out]


def batch(spec, ncu):
    return {'ncu': ncu, 'ncu+1': ncu + 1, '4ncu': 4 * ncu}.get(spec) or int(spec)


@pytest.mark.parametrize('c,hw,nspec,modes,tune,kind', cases())
def test_conv_layers_vs_float64(lib, ncu, c, hw, nspec, modes, tune, kind):
    n = batch(nspec, ncu)
    t0 = time.time()
    params, x, dh = make_inputs(1000 * c + hw + n, n, c, hw, kind)
    for mode in modes:
        maps = run_encoder(lib, params, x, dh, mode, tune)
        res = check_layers(params, x, dh, mode, tune, maps)
        report_and_assert(f'c={c} hw={hw} n={n} ({nspec}, {ncu} CUs) mode={mode} tune={tune} {kind}', res, zero_grads=kind == 'zero_dh')
        act, dact, d4, grads = maps
        if kind == 'zero_dh':               # (the bars above already demand exact zeros where the scale is 0; stated outright)
            assert all(bool((g == 0).all()) for g in grads) and all(bool((dact[l] == 0).all()) for l in (1, 2, 3)), mode
        if kind == 'edge':                  # the dead channels are dead, the others are not
            assert bool((act[2][:, :4] == 0).all()) and bool((act[2][:, 4:] > 0).any())
    print(f'  [{time.time() - t0:.1f} s]')


def test_reference_on_the_gpu_matches_the_cpu_path(lib):
    """The reference runs on the GPU (torch's float64 kernels) for time: the same layer references on the CPU, from the same GPU maps, agree
    with it to float64 rounding."""
    params, x, dh = make_inputs(5, 2, 3, 64, 'rand')
    act, dact, d4, grads = run_encoder(lib, params, x, dh, R.BF16X6, 0)

    def refs(dev):
        t = lambda v: v.to(dev)
        out = [R.conv_fwd(t(act[1]), t(params[2]), t(params[3]), 1, R.BF16X6),
               R.first_layer_fwd(t(x), t(params[0]), t(params[1])),
               R.conv_dgrad(t(d4), t(params[6]), t(act[3]), R.BF16X6),
               *R.conv_wgrad(t(dact[2]), t(act[1]), 1, R.BF16X6, R.EXACT),
               *R.conv_wgrad(t(dact[1]), R.pixel_scale(t(x)), 2, R.BF16X6)]
        return [v.cuda() for v in out]
    for a, b in zip(refs('cuda'), refs('cpu')):
        assert a.dtype == torch.float64 and a.shape == b.shape
        assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())
