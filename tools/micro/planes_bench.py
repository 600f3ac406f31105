"""Grouped GEMM on bf16 hi/lo planes (exorl_gemm_planes) at the agent's launch shapes: correctness against a float64 product of the
SAME planes, and time per launch.   python tools/micro/planes_bench.py [check]
python tools/micro/planes_bench.py planes3: the three-plane kernel (exorl_gemm_planes3) against gemm_kernel<EXORL_PREC_BF16X6> (exorl_gemm,
precision 3) on the same fp32 operands, alternating, HIP-event time per launch; plus the to_planes3 conversion passes, read off a profiled
bf16x6 TD3+BC update (the conversion kernel has no export of its own)."""
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from exorl_amd import _lib as L

lib = L.load()
C = L.C


def split(x):
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return hi, lo


def make(count, a_layouts, bl, M, N, K, x3, seed=0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    ps = []
    for i in range(count):
        A = torch.randn((M, K) if a_layouts[i] == 0 else (K, M), device='cuda', generator=g)
        B = torch.randn((N, K) if bl == 0 else (K, N), device='cuda', generator=g)
        ps.append((split(A), split(B), torch.zeros(M, N, device='cuda')))
    return ps


def launch(ps, a_layouts, bl, M, N, K, x3, relu=0):
    n = len(ps)
    arr = lambda xs: (C.c_void_p * n)(*[x.data_ptr() for x in xs])
    ah, al = arr([p[0][0] for p in ps]), arr([p[0][1] for p in ps])
    bh, bl_ = arr([p[1][0] for p in ps]), arr([p[1][1] for p in ps])
    cs = arr([p[2] for p in ps])
    lay = (C.c_int32 * n)(*a_layouts)
    lda = K if a_layouts[0] == 0 else M
    ldb = K if bl == 0 else N
    L.check(lib.exorl_gemm_planes(n, lay, bl, M, N, K, ah, al if x3 else None, lda, bh, bl_ if x3 else None, ldb, cs, N, relu,
                                  torch.cuda.current_stream().cuda_stream))


def reference(p, al, bl, x3):
    (ah, alo), (bh, blo), _ = p
    A = ah.double() + (alo.double() if x3 else 0)
    B = bh.double() + (blo.double() if x3 else 0)
    A = A if al == 0 else A.t()
    B = B.t() if bl == 0 else B
    full = A @ B
    if x3:      # the kernel drops lo*lo
        full = full - (alo.double() if al == 0 else alo.double().t()) @ (blo.double().t() if bl == 0 else blo.double())
    return full


def timed(ps, a_layouts, bl, M, N, K, x3, iters=40):
    for _ in range(5):
        launch(ps, a_layouts, bl, M, N, K, x3)
    torch.cuda.synchronize()
    L.check(lib.exorl_profile_gemm(1))
    for _ in range(iters):
        launch(ps, a_layouts, bl, M, N, K, x3)
    cap = 4096
    fl, ms, n = np.zeros(cap, np.float64), np.zeros(cap, np.float32), C.c_int32()
    L.check(lib.exorl_profile_gemm_read(fl.ctypes.data, ms.ctypes.data, cap, C.byref(n)))
    L.check(lib.exorl_profile_gemm(0))
    return float(np.median(ms[:n.value])) * 1e3


H = 1024
SHAPES = [  # (tag, count, a_layouts, b_layout, M, N, K)
    ('critic+target fwd (4)', 4, [0, 0, 0, 0], 0, 1024, H, H),
    ('wgrad+dgrad (2+2)', 4, [1, 1, 0, 0], 1, 1024, H, 1024),
    ('critic fwd (2)', 2, [0, 0], 0, 1024, H, H),
    ('critic dgrad (2)', 2, [0, 0], 1, 1024, H, H),
    ('actor wgrad+dgrad (1+1)', 2, [1, 0], 1, 1024, H, 1024),
    ('actor fwd 2B (1)', 1, [0], 0, 2048, H, H),
]

def split3(x):
    hi = x.to(torch.bfloat16)
    r = x - hi.float()
    mid = r.to(torch.bfloat16)
    return hi, mid, (r - mid.float()).to(torch.bfloat16)


def profiled(fn, iters):
    """(flops, us) of every launch fn() records, `iters` calls."""
    L.check(lib.exorl_profile_gemm(1))
    for _ in range(iters):
        fn()
    cap = 8192
    fl, ms, n = np.zeros(cap, np.float64), np.zeros(cap, np.float32), C.c_int32()
    L.check(lib.exorl_profile_gemm_read(fl.ctypes.data, ms.ctypes.data, cap, C.byref(n)))
    L.check(lib.exorl_profile_gemm(0))
    return fl[:n.value], ms[:n.value] * 1e3


def conversion_times(H=1024, B=1024, iters=20):
    """Median us of to_planes3 on 2 x B x H elements (h1 / dz2 of a twin net, W1 of two heads) and on B x H (the actor's dz2 and W1), from eager
    bf16x6 TD3+BC updates under exorl_profile_gemm: the records with 0 FLOPs, told apart by their duration rank within a step."""
    from exorl_amd.engine import AgentEngine
    eng = AgentEngine('td3_bc', 24, 6, H, B, precision='bf16x6')
    g = torch.Generator(device='cuda').manual_seed(0)
    for net in (0, 1):
        eng.flat(net).copy_(0.05 * torch.randn(eng.flat(net).numel(), device='cuda', generator=g))
    eng.params_changed(sync_target=True)
    r = lambda *sh: torch.randn(*sh, device='cuda', generator=g)
    eng.set_batch(r(B, 24), r(B, 6).tanh(), r(B), torch.full((B,), 0.99, device='cuda'), r(B, 24))
    for _ in range(3):
        eng.update(0.2)
    torch.cuda.synchronize()
    fl, us = profiled(lambda: eng.update(0.2), iters)
    conv = us[fl == 0].reshape(iters, -1)
    per_step = conv.shape[1]
    # 2BH-element passes: actor h1 (2B rows), target h1, critic h1 (twice), critic dz2 (twice), both W1 pairs; BH: actor dz2, actor W1
    med = np.median(conv, 0)
    small = np.sort(med)[:2]
    big = np.sort(med)[2:]
    return float(np.median(big)), float(np.median(small)), per_step, float(conv.sum(1).mean())


def planes3_table(iters=30):
    M = N = K = 1024
    t2, t1, per_step, conv_step = conversion_times()
    print(f'# to_planes3 (from {per_step} conversion launches per eager bf16x6 TD3+BC update, H = B = 1024): {t2:.2f} us per 2 x 1024 x 1024 elements, '
          f'{t1:.2f} us per 1024 x 1024; {conv_step:.1f} us of conversions per update')
    print('# form count | three-plane GEMM us | + conversions of both operands us | gemm_kernel<3> us (count launches summed) | ratio incl. conversions | TF/s incl.')
    rows = []
    for count in (2, 4):
        for tag, al, bl in (('fwd', 0, 0), ('dgrad', 0, 1), ('wgrad', 1, 1)):
            g = torch.Generator(device='cuda').manual_seed(count + 2 * al + bl)
            A = [torch.randn(1024, 1024, device='cuda', generator=g) for _ in range(count)]       # square: the stored shape is the same in both layouts
            B = [torch.randn(1024, 1024, device='cuda', generator=g) for _ in range(count)]
            a3, b3 = [split3(x) for x in A], [split3(x) for x in B]
            c3 = [torch.zeros(M, N, device='cuda') for _ in range(count)]
            cg = [torch.zeros(M, N, device='cuda') for _ in range(count)]
            arr = lambda xs: (C.c_void_p * count)(*[x.data_ptr() for x in xs])
            lay = (C.c_int32 * count)(*([al] * count))
            stream = torch.cuda.current_stream().cuda_stream

            def three():
                L.check(lib.exorl_gemm_planes3(count, lay, bl, M, N, K, arr([p[0] for p in a3]), arr([p[1] for p in a3]), arr([p[2] for p in a3]), 1024,
                                               arr([p[0] for p in b3]), arr([p[1] for p in b3]), arr([p[2] for p in b3]), 1024, arr(c3), N, 0, stream))

            def generic():
                for i in range(count):
                    L.check(lib.exorl_gemm(3, al, bl, M, N, K, A[i].data_ptr(), 1024, B[i].data_ptr(), 1024, cg[i].data_ptr(), N, None, 0, 0, stream))

            def both():
                three()
                generic()
            for _ in range(5):
                both()
            torch.cuda.synchronize()
            err = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(c3, cg))
            assert err < 2e-6, (tag, count, err)
            fl, us = profiled(both, iters)                      # per call: 1 three-plane launch, then `count` generic ones
            us = us.reshape(iters, 1 + count)
            t3, tg = float(np.median(us[:, 0])), float(np.median(us[:, 1:].sum(1)))
            conv = (count // 2) * 2 * t2                        # A and B of every problem, two problems per 2 x 1024 x 1024 pass
            flops = 2.0 * M * N * K * count
            rows.append((tag, count, t3, t3 + conv, tg))
            print(f'{tag:6s} {count} | {t3:7.2f} | {t3 + conv:7.2f} | {tg:7.2f} | {tg / (t3 + conv):5.2f} x | {flops / (t3 + conv) / 1e6:5.0f} (kernel alone {flops / t3 / 1e6:5.0f}, '
                  f'gemm_kernel<3> {flops / tg / 1e6:5.0f})', flush=True)
    return rows


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == 'planes3':
        planes3_table()
        sys.exit(0)
    check_only = len(sys.argv) > 1 and sys.argv[1] == 'check'
    for x3 in (True, False):
        for tag, count, lay, bl, M, N, K in SHAPES:
            ps = make(count, lay, bl, M, N, K, x3)
            for p in ps:
                p[2].zero_()
            launch(ps, lay, bl, M, N, K, x3)
            torch.cuda.synchronize()
            worst = 0.0
            for i, p in enumerate(ps):
                ref = reference(p, lay[i], bl, x3)
                err = float((p[2].double() - ref).abs().max() / ref.abs().max())
                worst = max(worst, err)
            assert worst < 2e-6, (tag, x3, worst)
            if check_only:
                print(f'{"x3" if x3 else "bf16":5s} {tag:26s} ok (max rel err {worst:.1e})', flush=True)
                continue
            t = timed(ps, lay, bl, M, N, K, x3)
            fl = 2.0 * M * N * K * count
            print(f'{"x3" if x3 else "bf16":5s} {tag:26s} {t:6.2f} us ({fl / t / 1e6:6.0f} TF/s)   (err {worst:.1e})', flush=True)
