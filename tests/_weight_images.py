"""The derived weight images of a state agent's net (include/exorl_hip.h, exorl_weight_images) rebuilt on the host from the fp32 parameters,
with integer arithmetic on their bit patterns. numpy only; tests/test_weight_images_abi.py checks the arithmetic without a GPU,
tests/test_gpu_weight_images.py holds the library's images to it bit for bit.

The parameters come as the net's tensors in the reference's parameters() order — per trunk W0 (H, in), b0, LayerNorm gain, LayerNorm bias;
per head W1 (H, H), b1, W2, b2; a net with as many trunks as heads lists [trunk i, head i] pairs, a shared trunk lists [trunk, head 0,
head 1] — which is what AgentEngine.tensor(net, i) hands out. Nothing here knows an offset inside the library's flat buffers."""
import numpy as np

IMAGES = ('w0t', 'w0_hi', 'w0_lo', 'w1_hi', 'w1_mid', 'w1_lo')


def bf16_bits(x):
    """bf16(x), round to nearest even, as uint16 bit patterns (finite x)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    """The float32 value of bf16 bit patterns."""
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def planes(x, n):
    """The first n of (hi, mid, lo) for n = 3, (hi, lo) for n = 2, (hi,) for n = 1: every plane is the bf16 of what the planes before it
    leave of x, the residue formed in float32 (where it is exact)."""
    r = np.ascontiguousarray(x, np.float32)
    out = []
    for _ in range(n):
        b = bf16_bits(r)
        out.append(b)
        r = r - bf16_value(b)
    return out


def planes_for(precision, H, B):
    """(planes of W0, planes of W1) a configuration has: the table in include/exorl_hip.h."""
    if precision == 'bf16':
        return 1, 1
    if precision == 'bf16x3' and H % 128 == 0 and B % 64 == 0:
        return 2, 2
    if precision == 'bf16x6' and H % 128 == 0 and B % 128 == 0:
        return 0, 3
    return 0, 0


def split_tensors(tensors, n_trunks, n_heads):
    """([W0 per trunk], [W1 per head]) of a net's tensors in the reference's order."""
    assert len(tensors) == 4 * (n_trunks + n_heads), (len(tensors), n_trunks, n_heads)
    if n_trunks == n_heads:
        w0 = [tensors[8 * i] for i in range(n_trunks)]
        w1 = [tensors[8 * i + 4] for i in range(n_heads)]
    else:
        assert n_trunks == 1
        w0 = [tensors[0]]
        w1 = [tensors[4 + 4 * i] for i in range(n_heads)]
    H, I = w0[0].shape
    assert all(w.shape == (H, I) for w in w0) and all(w.shape == (H, H) for w in w1), ([w.shape for w in w0], [w.shape for w in w1])
    return w0, w1


def expected_images(tensors, layout, precision_planes):
    """tensors: the net's fp32 arrays in the reference's order; layout: (n_trunks, n_heads); precision_planes: (planes of W0, planes of
    W1) as planes_for gives them. Returns name -> array for the six images (None for an image the configuration does not have): w0t
    float32 (n_trunks, in, H), the planes uint16, W0's K-padded with zero columns to a multiple of 32."""
    n_trunks, n_heads = layout
    p0, p1 = precision_planes
    assert p0 in (0, 1, 2) and p1 in (0, 1, 2, 3)
    w0, w1 = split_tensors([np.asarray(t, np.float32) for t in tensors], n_trunks, n_heads)
    H, I = w0[0].shape
    kp = (I + 31) // 32 * 32
    out = dict.fromkeys(IMAGES)
    out['w0t'] = np.stack([np.ascontiguousarray(w.T) for w in w0])
    padded = np.zeros((n_trunks, H, kp), np.float32)
    padded[:, :, :I] = np.stack(w0)
    for name, plane in zip(('w0_hi', 'w0_lo'), planes(padded, p0)):
        out[name] = plane
    names = {1: ('w1_hi',), 2: ('w1_hi', 'w1_lo'), 3: ('w1_hi', 'w1_mid', 'w1_lo')}.get(p1, ())
    for name, plane in zip(names, planes(np.stack(w1), p1)):
        out[name] = plane
    return out


def differing(got, want):
    """Names of the images that are not bit-identical (or exist on one side only). got: name -> array or None; float images are
    compared on their bit patterns."""
    bad = []
    for name in IMAGES:
        g, w = got.get(name), want.get(name)
        if g is None or w is None:
            if (g is None) != (w is None):
                bad.append(name)
            continue
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        bits = np.uint32 if w.dtype == np.float32 else np.uint16
        assert g.dtype.itemsize == w.dtype.itemsize, (name, g.dtype, w.dtype)
        if g.shape != w.shape or not np.array_equal(g.view(bits), w.view(bits)):
            bad.append(name)
    return bad


def first_difference(got, want, name):
    """'index got want' of the first differing element of one image, as hex bit patterns."""
    g, w = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
    if g.shape != w.shape:
        return f'shape {g.shape} != {w.shape}'
    bits = np.uint32 if w.dtype == np.float32 else np.uint16
    g, w = g.view(bits), w.view(bits)
    idx = np.argwhere(g != w)
    i = tuple(int(v) for v in idx[0])
    return f'{len(idx)} of {g.size} elements differ, first at {i}: got {int(g[i]):#x}, want {int(w[i]):#x}'
