"""Per-rank compute floor of the data-parallel module step of the pixel pretraining agents on one MI355X: the phases of
exorl_intr_update_phase for RND, ICM, ICM-APT, Disagreement, DIAYN, APS and SMM in bf16x6 at config-4 shapes (encodings of 3x84x84 frames,
repr_dim 39200, A=9, hidden 1024) for per-rank batches of 1024, 512, 256 and 128, with no collective between them, and the bytes of every
exchange an N-rank step runs (what one rank contributes; a gather moves world_size times that).

    python tools/micro/pixel_module_dp_bench.py [steps=20] [warmup=3]

The engines are built with world_size = 1024 / batch (a global batch of 1024) and rank 0. RND's step is the pixel agent's pair of calls:
the optimiser step (train=2) and the reward pass on re-encoded frames (train=0). The numbers go to DESIGN.md §5."""
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from exorl_amd import _lib as L
from exorl_amd.engine import IntrEngine

O, A, H, GLOBAL = 32 * 35 * 35, 9, 1024, 1024
STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 3
# configs/agent/*.yaml: rnd_rep_dim 512, icm_rep_dim 512, skill_dim 16, sf_dim 10, z_dim 4; PBE knn_k 12
KINDS = {'rnd': dict(rep_dim=512, encoded=True), 'icm': {}, 'icm_apt': dict(rep_dim=512, knn_k=12), 'disagreement': dict(n_models=5),
         'diayn': dict(rep_dim=16), 'aps': dict(rep_dim=10, knn_k=12), 'smm': dict(rep_dim=4, encoded=True)}
XNAMES = {L.INTR_XCHG_GRAD: 'grad', L.INTR_XCHG_REP: 'rep', L.INTR_XCHG_MOMENTS: 'moments'}


def run(kind, B):
    ws = GLOBAL // B
    m = IntrEngine(kind, O, A, H, B, lr=1e-4, precision='bf16x6', world_size=ws, rank=0, **KINDS[kind])
    dev = m.device
    g = torch.Generator(device='cpu').manual_seed(0)
    p = m.flat()
    p.copy_((torch.randn(p.numel(), generator=g) * 0.01).to(dev))
    R = KINDS[kind].get('rep_dim', 0)
    meta = R if kind in ('diayn', 'aps', 'smm') else 0
    obs = torch.randn(B, O + meta, device=dev) * 0.1
    nxt = torch.randn(B, O + meta, device=dev) * 0.1
    act = torch.rand(B, A, device=dev) * 2 - 1
    rew = torch.zeros(B, device=dev)
    dobs = torch.empty(B, O + meta, device=dev)
    if meta:
        obs[:, O:] = torch.eye(meta, device=dev)[torch.randint(0, meta, (B,))]
    W = O + meta
    calls = {'rnd': [((obs.data_ptr(), None, nxt.data_ptr(), rew.data_ptr(), rew.data_ptr(), 2), dict(dobs_out=dobs.data_ptr())),
                     ((obs.data_ptr(), None, nxt.data_ptr(), rew.data_ptr(), rew.data_ptr(), False), {})],
             'diayn': [((obs.data_ptr(), None, nxt.data_ptr(), rew.data_ptr(), rew.data_ptr(), True),
                        dict(skill=obs.data_ptr() + 4 * O, obs_ld=W, next_obs_ld=W, skill_ld=W, dobs_out=dobs.data_ptr()))],
             'smm': [((obs.data_ptr(), None, None, rew.data_ptr(), rew.data_ptr(), True),
                      dict(skill=obs.data_ptr() + 4 * O, obs_ld=W, skill_ld=W, dobs_out=dobs.data_ptr()))]}
    calls['aps'] = calls['diayn']
    step_calls = calls.get(kind, [((obs.data_ptr(), act.data_ptr(), nxt.data_ptr(), rew.data_ptr(), rew.data_ptr(), True),
                                   dict(dobs_out=dobs.data_ptr()))])
    exchanges = []

    def step(record=False):
        for a, k in step_calls:
            ph = 0
            while True:
                x = m.update_phase(ph, *a, **k)
                if x < 0:
                    break
                if record:
                    buf, op = m.exchange(x)
                    exchanges.append((XNAMES[x], int(buf[0].numel() * buf.element_size()) if op == L.XCHG_GATHER else int(buf.numel() * buf.element_size())))
                ph += 1
    step(record=True)
    for _ in range(WARMUP):
        step()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(STEPS)]
    for a, b in ev:
        a.record()
        step()
        b.record()
    torch.cuda.synchronize()
    ms = np.array([a.elapsed_time(b) for a, b in ev])
    del m
    return {'kind': kind, 'batch': B, 'ranks': ws, 'step_ms_median': float(np.median(ms)), 'step_ms_min': float(ms.min()),
            'exchanges': exchanges, 'exchange_bytes': int(sum(n for _, n in exchanges))}


def main():
    name = torch.cuda.get_device_name(0)
    print(f'# {name}: pixel module step (bf16x6), per-rank phases without collectives, {STEPS} timed steps after {WARMUP} warm-up')
    print(f"{'kind':>12} {'B/rank':>6} {'ranks@1024':>10} {'step ms':>8} {'min ms':>7} {'exchanged MB/rank':>17}  exchanges (bytes per rank)")
    rows = []
    for kind in KINDS:
        for B in (1024, 512, 256, 128):
            r = run(kind, B)
            rows.append(r)
            xs = ' '.join(f'{n}:{b}' for n, b in r['exchanges'])
            print(f"{kind:>12} {B:>6} {r['ranks']:>10} {r['step_ms_median']:>8.3f} {r['step_ms_min']:>7.3f} {r['exchange_bytes'] / 1e6:>17.2f}  {xs}",
                  flush=True)
            torch.cuda.empty_cache()
    print(json.dumps({'device': name, 'rows': rows}))


if __name__ == '__main__':
    main()
