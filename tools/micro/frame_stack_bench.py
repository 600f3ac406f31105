"""Frame-stacked replay arena against stacked rows at jaco shapes: observation (9, 84, 84) uint8 = frame_stack 3 of (3, 84, 84) frames,
A=9, B=1024, nstep 3, 40 episodes x 250 steps, Philox sampler, on one MI355X.

    python tools/micro/frame_stack_bench.py [gather] [update] [--procs 3] [--launches 200] [--episodes 40]

Variants: `stacked` = a plain arena fed the stacked episodes (gather_nstep_kernel, one wave per sample); `frames` = ReplayEngine(...,
frame_stack=3), one frame per row (gather_frames_kernel, one wave per output frame). Both write the same 2 x B x 63,504 bytes per batch.
Every measurement is a fresh process, --procs per variant, the variants alternating; a child that fails ends the run (exit 3; exit 1: a
requirement was missed).
  gather: the sample launch alone between HIP events, 20 warm-up launches, then --launches timed one by one (median reported) and the same
          number back to back between one event pair (mean); GB/s = (bytes read + bytes written) / the median.
  update: DDPG update()/s at these shapes with the batch sampled straight into the agent's slots (tools/micro/pixel_bench.py's loop).
--episodes sizes the arena (160: 850 MB of frames, past the 256 MiB Infinity Cache in both variants).
Requirement printed at the end: median(frames) <= median(stacked) + (max - min of stacked's processes), per measurement."""
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
C0, HW, K, A, B, NSTEP, EPISODES, EP_LEN = 3, 84, 3, 9, 1024, 3, 40, 250
FRAME_BYTES = C0 * HW * HW
HBM_PEAK_TBS = 8.0            # HBM3E spec peak of one MI355X (about 6.3 TB/s achievable)


def build_arena(variant):
    from exorl_amd.engine import ReplayEngine
    from exorl_amd.replay_buffer import stack_frames
    eng = ReplayEngine((K * C0, HW, HW), np.uint8, A, 0, EPISODES * (EP_LEN + 1) + 64, EPISODES + 8, 'cuda',
                       **(dict(frame_stack=K) if variant == 'frames' else {}))
    rs = np.random.RandomState(0)
    slots = []
    for _ in range(EPISODES):
        rows = EP_LEN + 1
        obs = rs.randint(0, 256, (rows, C0, HW, HW)).astype(np.uint8)
        slots.append(eng.append_episode(dict(observation=obs if variant == 'frames' else stack_frames(obs, K),
                                             action=rs.uniform(-1, 1, (rows, A)).astype(np.float32),
                                             reward=rs.uniform(0, 1, (rows, 1)).astype(np.float32), discount=np.ones((rows, 1), np.float32))))
    eng.set_order(slots)
    eng.seed_philox(1)
    return eng


def child_gather(variant, launches):
    import torch
    from exorl_amd import _lib as L
    eng = build_arena(variant)
    obs = torch.empty((B, K * C0, HW, HW), dtype=torch.uint8, device='cuda')
    nobs = torch.empty_like(obs)
    act, rew, disc = torch.empty(B, A, device='cuda'), torch.empty(B, 1, device='cuda'), torch.empty(B, 1, device='cuda')
    out = L.BatchOut(obs.data_ptr(), eng.obs_bytes, act.data_ptr(), A, rew.data_ptr(), disc.data_ptr(), nobs.data_ptr(), eng.obs_bytes, None, 0)
    for _ in range(20):
        eng.sample_into(out, B, NSTEP, 0.99, L.SAMPLER_PHILOX)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in ev:
        a.record()
        eng.sample_into(out, B, NSTEP, 0.99, L.SAMPLER_PHILOX)
        b.record()
    torch.cuda.synchronize()
    each = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])           # us
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        eng.sample_into(out, B, NSTEP, 0.99, L.SAMPLER_PHILOX)
    b.record()
    torch.cuda.synchronize()
    digest = int(obs.view(torch.int32).sum(dtype=torch.int64).item()) ^ int(nobs.view(torch.int32).sum(dtype=torch.int64).item())
    live, _ = eng.num_rows()
    return dict(median_us=float(np.median(each)), min_us=float(each.min()), p90_us=float(np.percentile(each, 90)),
                back_to_back_us=a.elapsed_time(b) * 1e3 / launches, arena_obs_bytes=live * eng.frame_bytes, last_batch_digest=digest)


def child_update(variant, steps):
    import torch
    from exorl_amd import agents
    from exorl_amd.replay_buffer import ArenaIterator
    eng = build_arena(variant)
    it = ArenaIterator(eng, B, NSTEP, 0.99, 'philox')
    torch.manual_seed(1)
    ag = agents.DDPGAgent(name='ddpg', reward_free=True, obs_type='pixels', obs_shape=(K * C0, HW, HW), action_shape=(A,), device='cuda', lr=1e-4,
                          feature_dim=50, hidden_dim=1024, critic_target_tau=0.01, num_expl_steps=2000, update_every_steps=2, stddev_schedule=0.2,
                          nstep=NSTEP, batch_size=B, stddev_clip=0.3, init_critic=True, use_tb=False, use_wandb=False, precision='fp32')
    for i in range(5):
        ag.update(it, 2 * i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        ag.update(it, 2 * (i + 5))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dict(updates_per_s=steps / dt, ms_per_update=1e3 * dt / steps)


def run_children(what, procs, arg):
    res = {'stacked': [], 'frames': []}
    for _ in range(procs):
        for variant in ('stacked', 'frames'):
            r = subprocess.run([sys.executable, __file__, '--child', what, variant, str(arg), str(EPISODES)], capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                print(f'{what} {variant}: child exited {r.returncode}\n{r.stdout}\n{r.stderr}', flush=True)
                sys.exit(3)                               # nothing more is started on the device after a failed child
            res[variant].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(f'{what:7s} {variant:8s} {res[variant][-1]}', flush=True)
    return res


def verdict(name, stacked, frames, lower_is_better):
    ms, mf, spread = float(np.median(stacked)), float(np.median(frames)), max(stacked) - min(stacked)
    ok = mf <= ms + spread if lower_is_better else mf >= ms - spread
    print(f'{name}: stacked median {ms:.2f} (runs {[round(x, 2) for x in stacked]}, max-min {spread:.2f}); frames median {mf:.2f} '
          f'(runs {[round(x, 2) for x in frames]}); frames/stacked = {mf / ms:.3f}; requirement {"met" if ok else "MISSED"}', flush=True)
    return ok


def main():
    global EPISODES
    args = sys.argv[1:]
    if args[:1] == ['--child']:
        EPISODES = int(args[4])
        sys.path.insert(0, str(ROOT))
        print(json.dumps((child_gather if args[1] == 'gather' else child_update)(args[2], int(args[3]))))
        return
    procs = int(args[args.index('--procs') + 1]) if '--procs' in args else 3
    launches = int(args[args.index('--launches') + 1]) if '--launches' in args else 200
    EPISODES = int(args[args.index('--episodes') + 1]) if '--episodes' in args else EPISODES
    what = [w for w in ('gather', 'update') if w in args] or ['gather', 'update']
    rows = EPISODES * (EP_LEN + 1)
    traffic = 2 * (2 * B * K * FRAME_BYTES)                 # obs + next_obs, each read once and written once
    print(f'shapes: obs ({K * C0},{HW},{HW}) u8 = {K} x {FRAME_BYTES} B, A={A}, B={B}, nstep={NSTEP}, {EPISODES} episodes x {EP_LEN} steps = {rows} rows; '
          f'arena observation bytes: stacked {rows * K * FRAME_BYTES / 1e6:.1f} MB, frames {rows * FRAME_BYTES / 1e6:.1f} MB; '
          f'bytes per batch: {traffic / 2e6:.1f} MB read + {traffic / 2e6:.1f} MB written', flush=True)
    ok = True
    if 'gather' in what:
        res = run_children('gather', procs, launches)
        assert len({r['last_batch_digest'] for v in res.values() for r in v}) == 1, 'the variants sampled different batches'
        ok &= verdict('gather launch, median of one-by-one launches, us', [r['median_us'] for r in res['stacked']], [r['median_us'] for r in res['frames']], True)
        verdict('gather launch, back to back, us', [r['back_to_back_us'] for r in res['stacked']], [r['back_to_back_us'] for r in res['frames']], True)
        for variant in ('stacked', 'frames'):
            us = float(np.median([r['median_us'] for r in res[variant]]))
            print(f'{variant}: {traffic / us / 1e3:.0f} GB/s achieved (bytes read + written over the median launch) of {HBM_PEAK_TBS * 1e3:.0f} GB/s HBM peak '
                  f'({100 * traffic / us / 1e6 / HBM_PEAK_TBS:.1f} %); arena observation bytes resident {res[variant][0]["arena_obs_bytes"] / 1e6:.1f} MB', flush=True)
    if 'update' in what:
        res = run_children('update', procs, 30)
        ok &= verdict('DDPG pixels update()/s', [r['updates_per_s'] for r in res['stacked']], [r['updates_per_s'] for r in res['frames']], False)
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
