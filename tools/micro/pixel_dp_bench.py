"""Per-rank compute floor of a data-parallel DDPG pixel step on one MI355X: the three phases of exorl_pixel_agent_update_phase at config-4
shapes (3x84x84 uint8, A=9, feature_dim 50, hidden 1024) for per-rank batches of 1024, 512, 256 and 128, with no collective between them,
and the bytes of the two exchange buffers an N-rank step all-reduces (exchange 0: critic + encoder gradients, exchange 1: actor gradients).

    python tools/micro/pixel_dp_bench.py [steps=30] [warmup=5]

The engines are built with world_size = 1024 / batch (a global batch of 1024), which changes only the scale of the means. The numbers go to
DESIGN.md §5."""
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from exorl_amd.engine import PixelEngine

C_, HW, A, F, H, GLOBAL = 3, 84, 9, 50, 1024, 1024
STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 30
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 5


def run(B, precision):
    e = PixelEngine((C_, HW, HW), A, F, H, B, precision=precision, world_size=GLOBAL // B)
    rs = np.random.RandomState(0)
    for net in range(3):                  # small random weights: the timing does not depend on the values
        for i in range(e.num_tensors(net)):
            t = e.tensor(net, i)
            t.copy_(torch.from_numpy(rs.standard_normal(tuple(t.shape)).astype(np.float32) * 0.02))
    e.sync_target()
    e.set_batch(rs.randint(0, 256, (B, C_, HW, HW)).astype(np.uint8), rs.uniform(-1, 1, (B, A)).astype(np.float32),
                rs.uniform(0, 1, B).astype(np.float32), np.full(B, 0.99, np.float32), rs.randint(0, 256, (B, C_, HW, HW)).astype(np.uint8))
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(STEPS)]
    for _ in range(WARMUP):
        for ph in range(3):
            e.update_phase(ph, 0.2)
    torch.cuda.synchronize()
    for k in range(STEPS):
        ev[k][0].record()
        for ph in range(3):
            e.update_phase(ph, 0.2)
            ev[k][ph + 1].record()
    torch.cuda.synchronize()
    ph_ms = np.array([[ev[k][p].elapsed_time(ev[k][p + 1]) for p in range(3)] for k in range(STEPS)])
    step = ph_ms.sum(1)
    return {'batch': B, 'precision': precision, 'step_ms_median': float(np.median(step)), 'step_ms_min': float(step.min()),
            'phase_ms_median': [round(float(v), 4) for v in np.median(ph_ms, 0)],
            'exchange0_bytes': int(e.grad_buffer(0).numel() * 4), 'exchange1_bytes': int(e.grad_buffer(1).numel() * 4)}


def main():
    name = torch.cuda.get_device_name(0)
    print(f'# {name}: DDPG pixel step, per-rank phases 0+1+2 without collectives, {STEPS} timed steps after {WARMUP} warm-up')
    print(f"{'precision':>9} {'B/rank':>6} {'ranks@1024':>10} {'step ms':>8} {'min ms':>7} {'ph0 ms':>7} {'ph1 ms':>7} {'ph2 ms':>7} {'ex0 MB':>7} {'ex1 MB':>7}")
    rows = []
    for precision in ('fp32', 'bf16x6'):
        for B in (1024, 512, 256, 128):
            r = run(B, precision)
            rows.append(r)
            p = r['phase_ms_median']
            print(f"{precision:>9} {B:>6} {GLOBAL // B:>10} {r['step_ms_median']:>8.3f} {r['step_ms_min']:>7.3f} {p[0]:>7.3f} {p[1]:>7.3f} {p[2]:>7.3f} "
                  f"{r['exchange0_bytes'] / 1e6:>7.2f} {r['exchange1_bytes'] / 1e6:>7.2f}", flush=True)
            torch.cuda.empty_cache()
    print(json.dumps({'device': name, 'rows': rows}))


if __name__ == '__main__':
    main()
