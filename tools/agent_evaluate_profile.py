"""agent.evaluate() at the benchmark's shapes (TD3+BC, walker_walk: O=24, A=6, H=1024, B=1024) next to update() from the same library.

    python tools/agent_evaluate_profile.py time <precision>          HIP-event times of evaluate(), the eager update() and the captured step
    python tools/agent_evaluate_profile.py launches <precision> <n>  2 warm-up + n evaluate() calls and nothing else, for a kernel trace
                                                                     (rocprofv3 --kernel-trace -- python ...): the difference of two runs
                                                                     with different n is the launch list of one call
    python tools/agent_evaluate_profile.py list <trace n1> <trace n2> <n1> <n2>      that difference, from the two kernel-trace CSVs
"""
import csv
import sys
from collections import Counter
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / 'tests')]
O, A, H, B = 24, 6, 1024, 1024


def setup(precision):
    import numpy as np
    import torch
    import _synth
    from exorl_amd import agents
    from exorl_amd.engine import ReplayEngine
    from exorl_amd.replay_buffer import ArenaIterator
    torch.manual_seed(0)
    ag = agents.TD3BCAgent('td3_bc', (O,), (A,), 'cuda', 1e-4, H, 0.01, '0.2', 1, B, 0.3, False, 2.5, precision=precision)
    its = []
    for seed in (1, 2):
        eng = ReplayEngine((O,), np.float32, A, 0, 1 << 16, 64)
        eng.set_order([eng.append_episode(ep) for ep in _synth.synth_episodes(seed, [1000] * 8, O, A)])
        eng.seed_philox(seed)
        its.append(ArenaIterator(eng, B, 1, 0.99, 'philox'))
    return ag, its[0], its[1]


def timed(fn, n):
    import torch
    for _ in range(20):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / n


def main():
    mode = sys.argv[1]
    if mode == 'list':
        def names(path):
            return Counter(r['Kernel_Name'].split('(')[0].replace('void ', '').replace('exorl::', '') for r in csv.DictReader(open(path)))
        a, b, n1, n2 = names(sys.argv[2]), names(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
        total = 0
        for k in sorted(set(a) | set(b)):
            per = (b[k] - a[k]) / (n2 - n1)
            if per:
                total += per
                print(f'   {k[:70]:70s} {per:5.1f}')
        print(f'   launches per evaluate(): {total:.1f}')
        return
    precision = sys.argv[2]
    ag, train, held = setup(precision)
    import torch
    if mode == 'launches':
        ag.engine.set_eval()
        for _ in range(2 + int(sys.argv[3])):
            ag._load_batch(held)
            ag.engine.evaluate()
        torch.cuda.synchronize()
        return
    ag.engine.set_eval()
    ag._load_batch(held)
    step = [0]

    def update():
        ag.update(train, step[0])
        step[0] += 1
    t_fwd = timed(ag.engine.evaluate, 500)
    t_eval = timed(lambda: ag.evaluate(held, 1), 200)
    t_eval8 = timed(lambda: ag.evaluate(held, 8), 50) / 8
    t_eager = timed(update, 500)
    assert ag.enable_graph(train)
    t_graph = timed(update, 500)
    print(f'{precision}: exorl_agent_evaluate alone {t_fwd:.1f} us; agent.evaluate(held, 1) with its sample and read {t_eval:.1f} us; '
          f'per batch of agent.evaluate(held, 8) {t_eval8:.1f} us; eager update() with its sample {t_eager:.1f} us; captured step {t_graph:.1f} us; '
          f'evaluate / captured step = {t_fwd / t_graph:.2f}')


if __name__ == '__main__':
    main()
