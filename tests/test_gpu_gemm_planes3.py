"""The three-plane grouped GEMM (exorl_gemm_planes3: gemm16p on hi / mid / lo bf16 planes, what the state agents launch in bf16x6 precision),
called through the C ABI: against the float64 product of the same planes minus the three terms the kernel drops, exactly on operands whose
products it holds exactly, in the first launch of a fresh process, and on the shapes and alignments it has to refuse."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
FORMS = [(0, 0), (0, 1), (1, 1)]           # (A layout, B layout): forward, dgrad, wgrad of nn.Linear


@pytest.fixture(scope='module')
def lib():
    from exorl_amd import _lib
    return _lib.load()


def split3(x):
    """hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid): the planes to_planes3_kernel writes."""
    hi = x.to(torch.bfloat16)
    r = x - hi.float()
    mid = r.to(torch.bfloat16)
    return hi, mid, (r - mid.float()).to(torch.bfloat16)


def arr(xs):
    return (C.c_void_p * len(xs))(*[x if isinstance(x, int) else x.data_ptr() for x in xs])


def planes3(lib, a_layouts, bl, M, N, K, As, Bs, cptrs, ldc, relu=0):
    """As / Bs: per problem (hi, mid, lo). Returns the C status."""
    count = len(As)
    lda, ldb = (K if a_layouts[0] == 0 else M), (K if bl == 0 else N)
    return lib.exorl_gemm_planes3(count, (C.c_int32 * count)(*a_layouts), bl, M, N, K, arr([a[0] for a in As]), arr([a[1] for a in As]),
                                  arr([a[2] for a in As]), lda, arr([b[0] for b in Bs]), arr([b[1] for b in Bs]), arr([b[2] for b in Bs]), ldb,
                                  arr(cptrs), ldc, relu, torch.cuda.current_stream().cuda_stream)


def reference(a3, b3, al, bl):
    """float64 product of (hi + mid + lo) minus the dropped mid*lo, lo*mid, lo*lo."""
    A = [(p.double() if al == 0 else p.double().t()) for p in a3]
    B = [(p.double().t() if bl == 0 else p.double()) for p in b3]
    return (A[0] + A[1] + A[2]) @ (B[0] + B[1] + B[2]) - A[1] @ B[2] - A[2] @ B[1] - A[2] @ B[2]


SHAPES = [
    (1, [0], 0, 128, 64, 128),                   # one tile, one pass of the stage ring
    (1, [0], 1, 128, 64, 128),                   # B as a k image
    (1, [1], 1, 128, 64, 256),                   # k-image A and B, two passes
    (2, [0, 0], 0, 128, 128, 128),               # two problems
    (1, [0], 1, 256, 192, 384),                  # N = 3 x 64, 12 stages
    (4, [0, 0, 0, 0], 0, 512, 512, 256),         # four problems through xcd_tile()
    (2, [1, 1], 1, 1024, 1024, 1024),            # 256 workgroups
    (4, [0, 0, 0, 0], 0, 1024, 1024, 1024),      # 256 workgroups per problem pair
    (2, [0, 0], 0, 10240, 1024, 1024),           # CQL's row count
]


@pytest.mark.parametrize('count,a_layouts,bl,M,N,K', SHAPES)
def test_planes3_shapes(lib, count, a_layouts, bl, M, N, K):
    """Real mid and lo planes split from torch.randn. error / max|ref| < 2e-6 (the project's bar for fp32 accumulation order) against the
    float64 product of the planes minus the dropped terms; with the output rows packed (pitch N) and with four floats of padding behind each
    row, whatever is not C[:, :N] keeps its guard value; 6 repeated launches are bit-identical (a stage-ring race shows as a result that moves)."""
    from exorl_amd import _lib as L
    g = torch.Generator(device='cuda').manual_seed(M + N + K + count + bl)
    As, Bs, refs = [], [], []
    for i in range(count):
        A = torch.randn((M, K) if a_layouts[i] == 0 else (K, M), device='cuda', generator=g)
        B = torch.randn((N, K) if bl == 0 else (K, N), device='cuda', generator=g)
        As.append(split3(A))
        Bs.append(split3(B))
        refs.append(reference(As[-1], Bs[-1], a_layouts[i], bl))
    GUARD = -123.0
    worst = 0.0
    for ldc in (N, N + 4):
        bufs = [torch.full((M * ldc + 8,), GUARD, device='cuda') for _ in range(count)]
        assert all(t.data_ptr() % 16 == 0 for t in bufs)
        inside = torch.zeros(M * ldc + 8, dtype=torch.bool, device='cuda')
        inside[:M * ldc].view(M, ldc)[:, :N] = True

        def launch():
            for t in bufs:
                t.fill_(GUARD)
            L.check(planes3(lib, a_layouts, bl, M, N, K, As, Bs, bufs, ldc))
            torch.cuda.synchronize()
            return [t.clone() for t in bufs]
        first = launch()
        for i, ref in enumerate(refs):
            err = float((first[i][inside].view(M, N).double() - ref).abs().max() / ref.abs().max())
            worst = max(worst, err)
            assert err < 2e-6, (i, ldc, err)
            assert bool((first[i][~inside] == GUARD).all()), (i, ldc)
        for _ in range(6 if ldc == N else 1):
            again = launch()
            for x, y in zip(first, again):
                assert torch.equal(x, y), ldc
    print(f'[planes3] {count} x {M}x{N}x{K} layouts {a_layouts[0]},{bl}: worst error / max|ref| = {worst:.2e} (bar 2e-6)')


def test_planes3_relu_epilogue(lib):
    """The one epilogue flag the export carries."""
    from exorl_amd import _lib as L
    g = torch.Generator(device='cuda').manual_seed(5)
    M, N, K = 128, 128, 128
    a3, b3 = split3(torch.randn(M, K, device='cuda', generator=g)), split3(torch.randn(N, K, device='cuda', generator=g))
    c = torch.full((M, N), float('nan'), device='cuda')
    L.check(planes3(lib, [0], 0, M, N, K, [a3], [b3], [c], N, relu=1))
    torch.cuda.synchronize()
    ref = reference(a3, b3, 0, 0).clamp_min(0)
    assert float((c.double() - ref).abs().max() / ref.abs().max()) < 2e-6


@pytest.mark.parametrize('al,bl', FORMS)
@pytest.mark.parametrize('M,N,K', [(128, 64, 128), (256, 128, 512)])
def test_planes3_exact_on_sparse_integers(lib, al, bl, M, N, K):
    """A has exactly four nonzero integers per row, |a| <= 2047, at random k positions (they span k16 groups and stages); B is dense integers,
    |b| <= 2047. Every such value is hi + mid exactly with lo = 0, and every partial sum is an integer of magnitude <= 4 * 2048^2 = 2^24, so C
    must equal the integer product bit for bit in any summation order. The same operands through the two-plane kernel, mid passed as its lo
    plane, must NOT be equal: it drops mid*mid."""
    from exorl_amd import _lib as L
    rs = np.random.RandomState(M + K + 2 * al + bl)
    A = np.zeros((M, K), np.float32)
    for m in range(M):
        A[m, rs.choice(K, 4, replace=False)] = rs.randint(1, 2048, 4) * rs.choice([-1, 1], 4)
    B = (rs.randint(1, 2048, (K, N)) * rs.choice([-1, 1], (K, N))).astype(np.float32)
    want = (A.astype(np.int64) @ B.astype(np.int64))
    assert np.abs(want).max() <= 2 ** 24
    a3 = split3(torch.from_numpy(A if al == 0 else np.ascontiguousarray(A.T)).cuda())
    b3 = split3(torch.from_numpy(np.ascontiguousarray(B.T) if bl == 0 else B).cuda())
    assert not bool(a3[2].float().any()) and not bool(b3[2].float().any()) and bool(a3[1].float().any()) and bool(b3[1].float().any())
    c = torch.full((M, N), float('nan'), device='cuda')
    L.check(planes3(lib, [al], bl, M, N, K, [a3], [b3], [c], N))
    torch.cuda.synchronize()
    assert np.array_equal(c.cpu().numpy().astype(np.int64), want) and np.array_equal(c.cpu().numpy(), want.astype(np.float32))
    c2 = torch.full((M, N), float('nan'), device='cuda')
    L.check(lib.exorl_gemm_planes(1, (C.c_int32 * 1)(al), bl, M, N, K, arr([a3[0]]), arr([a3[1]]), K if al == 0 else M, arr([b3[0]]), arr([b3[1]]),
                                  K if bl == 0 else N, arr([c2]), N, 0, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    d = np.abs(c2.cpu().numpy().astype(np.float64) - want).max()
    print(f'[planes3] sparse integers {M}x{N}x{K} layouts {al},{bl}: two-plane kernel max error {d:.0f}')
    assert d > 0


def test_planes3_first_launch_of_a_fresh_process():
    """One fresh interpreter per form makes exactly one launch (cold instruction cache: the waves of a workgroup drift apart, the LDS returns
    late — where a missing fence of the asm-issued transposed reads showed first) at 128 x 128 x 256 and compares it with float64."""
    code = r"""
import sys, ctypes as C
import torch
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from exorl_amd import _lib as L
import test_gpu_gemm_planes3 as T
lib = L.load()
al, bl = int(sys.argv[1]), int(sys.argv[2])
M, N, K = 128, 128, 256
g = torch.Generator(device='cuda').manual_seed(1)
a3 = T.split3(torch.randn((M, K) if al == 0 else (K, M), device='cuda', generator=g))
b3 = T.split3(torch.randn((N, K) if bl == 0 else (K, N), device='cuda', generator=g))
c = torch.full((M, N), float('nan'), device='cuda')
L.check(T.planes3(lib, [al], bl, M, N, K, [a3], [b3], [c], N))
torch.cuda.synchronize()
ref = T.reference(a3, b3, al, bl)
err = float((c.double() - ref).abs().max() / ref.abs().max())
print('ERR', err)
sys.exit(0 if err < 2e-6 else 3)
""" % (str(ROOT), str(ROOT / 'tests'))
    for al, bl in FORMS:
        r = subprocess.run([sys.executable, '-c', code, str(al), str(bl)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert r.returncode == 0, (al, bl, r.stdout[-2000:])


@pytest.mark.parametrize('what', ['M=64', 'N=32', 'K=64', 'K=192', 'ldc=N+1', 'C+4B', 'A_mid+2B', 'B_lo+2B', 'mixed layouts', 'null mid'])
def test_planes3_rejections(lib, what):
    """A shape or alignment the kernel cannot take is an error with a message; nothing is launched (the output keeps its guard value)."""
    M, N, K = 128, 64, 128
    if what in ('M=64', 'N=32', 'K=64', 'K=192'):
        M, N, K = {'M=64': (64, N, K), 'N=32': (M, 32, K), 'K=64': (M, N, 64), 'K=192': (M, N, 192)}[what]
    pad = 8                                     # elements behind every plane, so that a shifted pointer stays inside its allocation
    mk = lambda r, c: tuple(torch.zeros(r * c + pad, dtype=torch.bfloat16, device='cuda') for _ in range(3))
    count = 2 if what == 'mixed layouts' else 1
    As, Bs = [mk(M, K) for _ in range(count)], [mk(K, N) for _ in range(count)]
    ldc = N + 1 if what == 'ldc=N+1' else N
    bufs = [torch.full((M * ldc + 8,), -123.0, device='cuda') for _ in range(count)]
    cptrs = [t.data_ptr() + (4 if what == 'C+4B' else 0) for t in bufs]
    Ap = [[p.data_ptr() for p in a] for a in As]
    Bp = [[p.data_ptr() for p in b] for b in Bs]
    if what == 'A_mid+2B':
        Ap[0][1] += 2
    if what == 'B_lo+2B':
        Bp[0][2] += 2
    if what == 'null mid':
        Ap[0][1] = 0
    lay = [0, 1] if what == 'mixed layouts' else [0] * count
    rc = planes3(lib, lay, 1, M, N, K, Ap, Bp, cptrs, ldc)
    torch.cuda.synchronize()
    assert rc != 0, what
    msg = lib.exorl_last_error().decode()
    assert msg and ('planes3' in msg or 'three-plane' in msg), (what, msg)
    assert all(bool((t == -123.0).all()) for t in bufs), what
