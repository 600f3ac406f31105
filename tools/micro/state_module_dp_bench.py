"""Per-rank compute of the sharded module step of the reward-free agents on STATE observations on one MI355X: the phases of
exorl_intr_update_phase back to back, with no collective between them, for all eight kinds at the shipped widths (O=24, A=6, hidden 1024,
the configs' rep dims) in bf16x3 and fp32, at a per-rank batch of 1024 rows for world sizes 1, 2, 4 and 8. Beside each figure stands the
replicated module on world x 1024 rows — the default step, which every rank runs on the gathered batch. ICM-APT and APS could not be built
at more than 4096 rows before the chunked kNN selection: those cells say so, with the time the replicated step takes now.

Then the kNN path past 4096 targets: exorl_knn_topk at 1024 x 8192 x 512, k = 12, against eight times the LDS path's time at
1024 x 1024 x 512 in the same process — the ratio of the work in pair distances.

    python tools/micro/state_module_dp_bench.py [steps=20] [warmup=3]

One GPU, no collective: N > 1 on real GPUs is unmeasured. The numbers go to profiles/state_module_dp_per_rank.txt and DESIGN.md §5."""
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from exorl_amd import _lib as L
from exorl_amd.engine import IntrEngine

O, A, H, B = 24, 6, 1024, 1024
STEPS = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 20
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 3
# configs/agent/*.yaml: rnd_rep_dim 512, icm_rep_dim 512, skill_dim 16, sf_dim 10, z_dim 4; PBE knn_k 12; proto: pred 128, proj 512, 512 protos
KINDS = {'rnd': dict(rep_dim=512), 'icm': {}, 'icm_apt': dict(rep_dim=512, knn_k=12), 'disagreement': dict(n_models=5), 'diayn': dict(rep_dim=16),
         'aps': dict(rep_dim=10, knn_k=12), 'smm': dict(rep_dim=4),
         'proto': dict(rep_dim=128, knn_k=3, num_protos=512, queue_size=2048, tau=0.1, target_tau=0.05)}
META = {'diayn': 16, 'aps': 10, 'smm': 4}


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(STEPS)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def module_step_ms(kind, rows, world, precision):
    m = IntrEngine(kind, O, A, 512 if kind == 'proto' else H, rows, lr=1e-4, precision=precision, world_size=world, rank=0, **KINDS[kind])
    dev = m.device
    g = torch.Generator(device='cpu').manual_seed(0)
    p = m.flat()
    p.copy_((torch.randn(p.numel(), generator=g) * 0.01).to(dev))
    M = META.get(kind, 0)
    W = O + M
    obs, nxt = torch.randn(rows, W, device=dev), torch.randn(rows, W, device=dev)
    if M:
        obs[:, O:] = torch.eye(M, device=dev)[torch.randint(0, M, (rows,), device=dev)]
    act, rew = torch.rand(rows, A, device=dev) * 2 - 1, torch.zeros(rows, device=dev)
    o, n, a, r = obs.data_ptr(), nxt.data_ptr(), act.data_ptr(), rew.data_ptr()
    if kind in ('diayn', 'aps'):
        args, kw = (o, None, n, r, r, True), dict(skill=o + 4 * O, obs_ld=W, next_obs_ld=W, skill_ld=W)
    elif kind == 'smm':
        args, kw = (o, None, None, r, r, True), dict(skill=o + 4 * O, obs_ld=W, skill_ld=W)
    elif kind == 'proto':
        args, kw = (o, None, n, r, r, True), {}
    else:
        args, kw = (o, a, n, r, r, True), {}

    def step():
        if world == 1:
            return m.update(*args, **kw)
        ph = 0
        while m.update_phase(ph, *args, **kw) >= 0:        # the gather slots of the other ranks stay as they are: zeros
            ph += 1
    ms = timed(step)
    del m
    torch.cuda.empty_cache()
    return ms


def knn_ms(ns, nt, dim, k):
    lib = L.load()
    src, tgt, out = torch.randn(ns, dim, device='cuda'), torch.randn(nt, dim, device='cuda'), torch.empty(ns, k, device='cuda')
    return timed(lambda: L.check(lib.exorl_knn_topk(src.data_ptr(), ns, tgt.data_ptr(), nt, dim, k, out.data_ptr(), L.current_stream())))


def main():
    name = torch.cuda.get_device_name(0)
    print(f'# {name}: module step on state rows, phases back to back without collectives, median of {STEPS} steps after {WARMUP} warm-up')
    print('# sharded: one rank\'s step on its 1024 rows with world_size = world; replicated: one engine on world x 1024 rows (the default step,')
    print('# run by every rank). One GPU, no collective: N > 1 on real GPUs unmeasured.')
    print(f"{'precision':>9} {'kind':>12} {'world':>5} {'sharded ms':>10} {'replicated ms':>28}")
    rows = []
    for precision in ('bf16x3', 'fp32'):
        for kind in KINDS:
            for world in (1, 2, 4, 8):
                sharded = module_step_ms(kind, B, world, precision)
                replicated = sharded if world == 1 else module_step_ms(kind, B * world, 1, precision)
                refused = kind in ('icm_apt', 'aps') and B * world > 4096
                cell = f'refused before (now {replicated:.3f})' if refused else f'{replicated:.3f}'
                rows.append(dict(precision=precision, kind=kind, world=world, sharded_ms=sharded, replicated_ms=replicated,
                                 replicated_refused_before=refused))
                print(f'{precision:>9} {kind:>12} {world:>5} {sharded:>10.3f} {cell:>28}', flush=True)
    chunked, lds = knn_ms(1024, 8192, 512, 12), knn_ms(1024, 1024, 512, 12)
    print(f'# kNN 1024 x 8192 x 512, k=12 (chunked selection): {chunked:.3f} ms; 8 x (1024 x 1024 x 512, LDS selection: {lds:.3f} ms) = '
          f'{8 * lds:.3f} ms; ratio {chunked / (8 * lds):.2f}')
    print(json.dumps({'device': name, 'rows': rows, 'knn_8192_ms': chunked, 'knn_1024_ms': lds, 'knn_ratio': chunked / (8 * lds)}))


if __name__ == '__main__':
    main()
