"""Observation normalisation in the HBM replay on one MI355X: what the normalising gather costs, and the two moments launches.

    python tools/micro/obs_norm_bench.py [gather] [moments] [--parent DIR] [--procs 3] [--launches 200]
    python tools/micro/obs_norm_bench.py child gather off|on|parent [--parent DIR]      one measurement, e.g. under a kernel tracer
    python tools/micro/obs_norm_bench.py child moments ROWS_K COLS

gather: walker shapes, O=24, A=6, B=1024, nstep 1, Philox sampler, 1000 episodes x 1000 steps. Variants: `off` = this tree, no normaliser
(gather_nstep_kernel<false>); `on` = this tree with ReplayEngine.set_obs_normalizer (gather_nstep_kernel<true>); `parent` = the same loop
on another built checkout (--parent DIR, e.g. the parent commit), which has the untemplated kernel. Every measurement is a fresh process,
--procs per variant, the variants alternating; 20 warm-up launches, then --launches timed one by one between HIP events (median) and the
same number back to back inside one event pair (mean).
moments: ReplayEngine.obs_moments() on 1 M x 24 and 5 M x 78 rows (1000-step episodes): HIP events around the whole call (table upload,
both launches, the read-back) and bytes = live rows x O x 4 over that time; kernel times come from a kernel trace of the child.
A child that fails ends the run (exit 3)."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
O, A, B, EPISODES, EP_LEN = 24, 6, 1024, 1000, 1000
HBM_PEAK_TBS = 8.0            # HBM3E spec peak of one MI355X (about 6.3 TB/s achievable)


def build_arena(cols, episodes):
    from exorl_amd.engine import ReplayEngine
    eng = ReplayEngine((cols,), np.float32, A, 0, episodes * (EP_LEN + 1) + 64, episodes + 8, 'cuda')
    rs = np.random.RandomState(0)
    rows = EP_LEN + 1
    pool = [dict(observation=rs.standard_normal((rows, cols)).astype(np.float32), action=rs.uniform(-1, 1, (rows, A)).astype(np.float32),
                 reward=rs.uniform(0, 1, (rows, 1)).astype(np.float32), discount=np.ones((rows, 1), np.float32)) for _ in range(16)]
    eng.set_order([eng.append_episode(pool[i % 16]) for i in range(episodes)])
    eng.seed_philox(1)
    return eng


def child_gather(variant, launches):
    import torch
    from exorl_amd import _lib as L
    eng = build_arena(O, EPISODES)
    if variant == 'on':
        cnt, mean, m2 = eng.obs_moments()
        from exorl_amd.utils import obs_normalizer
        eng.set_obs_normalizer(*obs_normalizer(cnt, mean, m2))
    obs = torch.empty((B, O), dtype=torch.float32, device='cuda')
    nobs = torch.empty_like(obs)
    act, rew, disc = torch.empty(B, A, device='cuda'), torch.empty(B, 1, device='cuda'), torch.empty(B, 1, device='cuda')
    out = L.BatchOut(obs.data_ptr(), eng.obs_bytes, act.data_ptr(), A, rew.data_ptr(), disc.data_ptr(), nobs.data_ptr(), eng.obs_bytes, None, 0)
    for _ in range(20):
        eng.sample_into(out, B, 1, 0.99, L.SAMPLER_PHILOX)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in ev:
        a.record()
        eng.sample_into(out, B, 1, 0.99, L.SAMPLER_PHILOX)
        b.record()
    torch.cuda.synchronize()
    us = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        eng.sample_into(out, B, 1, 0.99, L.SAMPLER_PHILOX)
    b.record()
    torch.cuda.synchronize()
    print(json.dumps(dict(variant=variant, median_us=float(np.median(us)), min_us=float(us.min()), p90_us=float(np.percentile(us, 90)),
                          back_to_back_us=a.elapsed_time(b) * 1e3 / launches, obs_mean_abs=float(obs.abs().mean()))))


def child_moments(rows_k, cols):
    import torch
    episodes = rows_k * 1000 // EP_LEN
    eng = build_arena(cols, episodes)
    first = eng.obs_moments()                   # allocates the slab
    times = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        got = eng.obs_moments()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
        assert got[0] == first[0] and np.array_equal(got[1], first[1]) and np.array_equal(got[2], first[2])
    nbytes = first[0] * cols * 4
    us = float(np.median(times))
    print(json.dumps(dict(rows=first[0], cols=cols, bytes=nbytes, call_us_median=us, call_us_min=float(min(times)), gbs=nbytes / us * 1e-3,
                          share_of_hbm_peak=nbytes / us * 1e-6 / HBM_PEAK_TBS)))


def run_child(args, tree):
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), 'child', *args, '--tree', str(tree)], stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        print('child failed:', args, file=sys.stderr)
        sys.exit(3)
    row = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(row), flush=True)
    return row


def opt(argv, name, default):
    return argv[argv.index(name) + 1] if name in argv else default


if __name__ == '__main__':
    argv = sys.argv[1:]
    sys.path.insert(0, str(Path(opt(argv, '--tree', ROOT)).resolve()))
    parent, procs, launches = opt(argv, '--parent', None), int(opt(argv, '--procs', 3)), int(opt(argv, '--launches', 200))
    if argv[:1] == ['child']:
        if argv[1] == 'gather':
            child_gather(argv[2], launches)
        else:
            child_moments(int(argv[2]), int(argv[3]))
        sys.exit(0)
    if 'gather' in argv or not {'gather', 'moments'} & set(argv):
        variants = (['parent'] if parent else []) + ['off', 'on']
        rows = [run_child(['gather', v, '--launches', str(launches)], parent if v == 'parent' else ROOT) for _ in range(procs) for v in variants]
        for v in variants:
            med = [r['median_us'] for r in rows if r['variant'] == v]
            print(f'{v}: median of process medians {np.median(med):.2f} us, max-min {max(med) - min(med):.2f} us')
    if 'moments' in argv or not {'gather', 'moments'} & set(argv):
        for rows_k, cols in ((1000, 24), (5000, 78)):
            run_child(['moments', str(rows_k), str(cols)], ROOT)
