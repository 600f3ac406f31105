"""Timings for profiles/prdc_search.txt and profiles/prdc_step.txt: device events around enqueued work, warmed up, one process."""
import ctypes, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / 'tests'))
import numpy as np
import torch
from exorl_amd import _lib as L, agents
from exorl_amd.engine import ReplayEngine
from exorl_amd.replay_buffer import ArenaIterator

lib = L.load()
name = ctypes.create_string_buffer(128); cus = ctypes.c_int(); hbm = ctypes.c_int64()
L.check(lib.exorl_device_info(name, 128, ctypes.byref(cus), ctypes.byref(hbm)))
print('device', name.value.decode(), 'CUs', cus.value, flush=True)


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


D, PITCH, B = 30, 32, 1024
PEAK_LANE_OPS = 157.3e12 / 2          # the vector peak counts an FMA as two operations
for N in (100_000, 1_000_000):
    g = torch.Generator(device='cuda').manual_seed(N)
    keys = torch.randn(N, PITCH, device='cuda', generator=g)
    keys[:, D:] = 0
    q = torch.randn(B, PITCH, device='cuda', generator=g)
    idx = torch.zeros(B, dtype=torch.int32, device='cuda'); d2 = torch.zeros(B, device='cuda')
    for splits in (0, 16, 64, 256):
        fn = lambda: L.check(lib.exorl_nn_search(keys.data_ptr(), N, PITCH, D, q.data_ptr(), PITCH, B, splits, idx.data_ptr(), d2.data_ptr(), L.current_stream()))
        reps = []
        for _ in range(3):
            reps.append(timed(fn, 3, 20))
        ms = min(reps)
        q_tiles = B // 64
        S = splits or min(-(-4 * cus.value // q_tiles), 256)
        lane_ops = 2.0 * B * N * 32          # a subtraction and a multiply-add per pair and column, the padded 32 columns
        reread = q_tiles * N * PITCH * 4
        print(f'search N={N} D={D} B={B} splits_arg={splits} (S={S}, query tile 64): {ms:.3f} ms (three runs of 20: {", ".join(f"{r:.3f}" for r in reps)}); '
              f'{lane_ops / ms / 1e9:.1f} T lane-ops/s = {100 * lane_ops / (ms * 1e-3) / PEAK_LANE_OPS:.1f} % of the vector peak; '
              f'table bytes read by the workgroups {reread / 1e9:.2f} GB per search = {reread / (ms * 1e-3) / 1e12:.2f} TB/s', flush=True)

# ---- the step at walker shapes, captured graph
O, A, H = 24, 6, 1024
EP, LEN = 1000, 1000
rs = np.random.RandomState(0)
eng = ReplayEngine((O,), np.float32, A, 0, EP * (LEN + 1) + 64, EP + 4)
slots = []
for e in range(EP):
    ep = dict(observation=rs.standard_normal((LEN + 1, O)).astype(np.float32), action=rs.uniform(-1, 1, (LEN + 1, A)).astype(np.float32),
              reward=rs.uniform(0, 1, (LEN + 1, 1)).astype(np.float32), discount=np.ones((LEN + 1, 1), np.float32))
    slots.append(eng.append_episode(ep))
eng.set_order(slots)
eng.seed_philox(1)
for precision in ('bf16x3', 'fp32'):
    for cls in ('TD3BCAgent', 'PRDCAgent'):
        torch.manual_seed(0)
        ag = getattr(agents, cls)(cls, (O,), (A,), 'cuda', 1e-4, H, 0.01, 0.2, 1, B, 0.3, False, 2.5, precision=precision)
        it = ArenaIterator(eng, B, 1, 0.99, 'philox')
        if cls == 'PRDCAgent':
            t = time.time(); rows = ag.bind_dataset(it); torch.cuda.synchronize()
            print(f'bind_dataset: {rows} rows in {time.time() - t:.3f} s (host wall, allocation included), {ag.engine.nn_result()[3]} key ranges', flush=True)
        assert ag.enable_graph(it)
        step = [0]
        def fn():
            ag.update(it, step[0]); step[0] += 1
        reps = [timed(fn, 20, 200) for _ in range(3)]
        print(f'{cls} {precision} H={H} B={B} captured graph: {min(reps):.4f} ms per update = {1e3 / min(reps):.0f} update()/s (three runs of 200: '
              f'{", ".join(f"{r:.4f}" for r in reps)})', flush=True)
        if cls == 'PRDCAgent':
            idx, d2, _, _ = ag.engine.nn_result()
            print(f'  last step: mean nn distance {float(d2.sqrt().mean()):.4f}, distinct neighbours {len(set(idx.cpu().tolist()))} of {B}', flush=True)
        ag.disable_graph()
        del ag
