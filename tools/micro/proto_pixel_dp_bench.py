"""Per-rank compute floor of Proto's data-parallel pixel pretraining update on one MI355X, at config-4 shapes (3x84x84 frames, repr_dim
39200, A=9, feature_dim 50, hidden 1024, pred_dim 128, proj_dim 512, 512 prototypes, queue 2048, topk 3), for per-rank batches of 1024,
512, 256 and 128 in bf16x6 and fp32, with no collective between the phases; plus the bytes of every exchange an N-rank update runs (what
one rank contributes; a gather moves world_size times that).

    python tools/micro/proto_pixel_dp_bench.py [steps=20] [warmup=3]

One update is what ProtoAgent._update_pixels runs with shard_pretraining: augment, encode obs and next_obs (target encoder), the module's
step phases (train=2), the encoder step's two phases, encode next_obs, the module's reward phases (train=0), encode obs, the DDPG pixel
step's three phases and encoder_target's Polyak step. The engines are built with world_size = 1024 / batch (a global batch of 1024) and
rank 0. The second table times the two phases that run over the gathered global batch, at Bg = 1024 and 8192 rows: the step's phase 1
(the targets' scores, Sinkhorn over Bg rows, the loss and its backward pass on this rank's 1024 rows) and the reward's phase 1 (scores of
Bg rows, the candidate draw over them, kNN of this rank's rows); these run on state-width inputs (obs_dim 64) so that the predictor's
share is small. The numbers go to DESIGN.md §5."""
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from exorl_amd import _lib as L
from exorl_amd.engine import IntrEngine, PixelEngine

C_, HW, A, F, H, PD, PJ, NP, Q, GLOBAL = 3, 84, 9, 50, 1024, 128, 512, 512, 2048, 1024
STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 3
XNAMES = {L.INTR_XCHG_GRAD: 'grad', L.INTR_XCHG_REP: 'rep', L.INTR_XCHG_MOMENTS: 'moments'}


def _nbytes(buf, op):
    return int(buf[0].numel() * buf.element_size()) if op == L.XCHG_GATHER else int(buf.numel() * buf.element_size())


def _timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(STEPS)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(b) for a, b in ev])


def _module(O, B, ws, precision):
    m = IntrEngine('proto', O, A, PJ, B, rep_dim=PD, lr=1e-4, knn_k=3, num_protos=NP, queue_size=Q, tau=0.1, target_tau=0.05,
                   precision=precision, world_size=ws, rank=0)
    g = torch.Generator(device='cpu').manual_seed(0)
    p = m.flat()
    p.copy_((torch.randn(p.numel(), generator=g) * 0.01).to(m.device))
    return m


def _phases(m, args, kw, exchanges=None):
    ph = 0
    while True:
        x = m.update_phase(ph, *args, **kw)
        if x < 0:
            return
        if exchanges is not None:
            exchanges.append((XNAMES[x], _nbytes(*m.exchange(x))))
        ph += 1


def run_update(B, precision):
    ws = GLOBAL // B
    pix = PixelEngine((C_, HW, HW), A, F, H, B, precision=precision, world_size=ws)
    pix.encoder_target(init=True)
    O = pix.lib.exorl_encoder_out_dim(HW)
    m = _module(O, B, ws, precision)
    rs = np.random.RandomState(0)
    pix.set_batch(rs.randint(0, 256, (B, C_, HW, HW)).astype(np.uint8), rs.uniform(-1, 1, (B, A)).astype(np.float32),
                  rs.uniform(0, 1, B).astype(np.float32), np.full(B, 0.99, np.float32), rs.randint(0, 256, (B, C_, HW, HW)).astype(np.uint8))
    s = pix.batch_slots()
    dobs = torch.zeros(B, O, device=pix.device)
    exchanges = []

    def update(record=False):
        xs = exchanges if record else None
        pix.augment()
        fo, ft = pix.encode(0), pix.encode(1, target=True)
        _phases(m, (fo, None, ft, None, s.reward, 2), dict(next_obs_target=ft, dobs_out=dobs.data_ptr()), xs)
        pix.encoder_step_phase(0, 0, dobs.data_ptr(), 1)
        if record:
            exchanges.append(('encoder grad', int(pix.grad_buffer(2).numel() * 4)))
        pix.encoder_step_phase(1, 0, dobs.data_ptr(), 1)
        fn = pix.encode(1)
        _phases(m, (fo, None, fn, s.reward, s.reward, False), {}, xs)
        pix.encode(0)
        pix.set_train_encoder(False)
        pix.update_phase(0, 0.2, keep_encoded=True)
        pix.update_phase(1, 0.2)
        pix.update_phase(2, 0.2)
        if record:
            exchanges.extend([('ddpg critic+encoder grad', int(pix.grad_buffer(0).numel() * 4)), ('ddpg actor grad', int(pix.grad_buffer(1).numel() * 4))])
        pix.encoder_target(0.05)
    update(record=True)
    ms = _timed(update)
    del m, pix
    return {'precision': precision, 'batch': B, 'ranks': ws, 'update_ms_median': float(np.median(ms)), 'update_ms_min': float(ms.min()),
            'exchanges': exchanges, 'exchange_bytes': int(sum(n for _, n in exchanges))}


def run_global(Bg, precision, O=64, B=1024):
    ws = Bg // B
    m = _module(O, B, ws, precision)
    dev = m.device
    obs, nxt = torch.randn(B, O, device=dev), torch.randn(B, O, device=dev)
    rew, dobs = torch.zeros(B, device=dev), torch.zeros(B, O, device=dev)
    step = (obs.data_ptr(), None, nxt.data_ptr(), None, rew.data_ptr(), 2), dict(dobs_out=dobs.data_ptr())
    reward = (obs.data_ptr(), None, nxt.data_ptr(), rew.data_ptr(), rew.data_ptr(), False), {}
    out = {'precision': precision, 'Bg': Bg, 'ranks': ws}
    for name, (a, k) in (('sinkhorn_phase', step), ('draw_phase', reward)):
        if ws == 1:           # one rank: phase 0 runs the gathered phase's work too; time the whole call
            ms = _timed(lambda: m.update_phase(0, *a, **k))
        else:
            m.update_phase(0, *a, **k)
            ms = _timed(lambda: m.update_phase(1, *a, **k))
        out[name + '_ms_median'] = float(np.median(ms))
    del m
    return out


def main():
    name = torch.cuda.get_device_name(0)
    print(f'# {name}: Proto pixel pretraining update, per-rank phases without collectives, {STEPS} timed updates after {WARMUP} warm-up')
    print(f"{'precision':>9} {'B/rank':>6} {'ranks@1024':>10} {'update ms':>9} {'min ms':>7} {'exchanged MB/rank':>17}  exchanges (bytes per rank)")
    rows, grows = [], []
    for precision in ('bf16x6', 'fp32'):
        for B in (1024, 512, 256, 128):
            r = run_update(B, precision)
            rows.append(r)
            xs = ' '.join(f'{n.replace(" ", "_")}:{b}' for n, b in r['exchanges'])
            print(f"{precision:>9} {B:>6} {r['ranks']:>10} {r['update_ms_median']:>9.3f} {r['update_ms_min']:>7.3f} {r['exchange_bytes'] / 1e6:>17.2f}  {xs}",
                  flush=True)
            torch.cuda.empty_cache()
    print('# phases over the gathered global batch (obs_dim 64, 1024 rows per rank; Bg 1024: one rank, the whole one-rank call)')
    print(f"{'precision':>9} {'Bg':>6} {'ranks':>5} {'sinkhorn phase ms':>17} {'draw phase ms':>13}")
    for precision in ('bf16x6', 'fp32'):
        for Bg in (1024, 8192):
            r = run_global(Bg, precision)
            grows.append(r)
            print(f"{precision:>9} {Bg:>6} {r['ranks']:>5} {r['sinkhorn_phase_ms_median']:>17.3f} {r['draw_phase_ms_median']:>13.3f}", flush=True)
    print(json.dumps({'device': name, 'rows': rows, 'global': grows}))


if __name__ == '__main__':
    main()
