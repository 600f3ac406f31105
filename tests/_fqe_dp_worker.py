"""One data-parallel rank of FQEAgent, run as a fresh child process by tests/test_gpu_fqe_dp.py: both ranks sit on cuda:0 and talk gloo, so
AgentEngine.update_steps drives the plan's two phases with a torch.distributed all-reduce of the critic gradients between them. Each rank
takes its half of the global batches the parent replays whole."""
import json
import os
import sys
from pathlib import Path

import numpy as np
import torch
import torch.distributed as dist

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tests'))

O, A, H, B_GLOBAL, STEPS = 24, 6, 128, 128, 3
PRECISIONS = ('fp32', 'bf16x3')
NETS = ('actor', 'critic', 'critic_target')


def case(precision, batch):
    import _fqe_cases as F
    return F.Case(O, A, H, batch, precision, 21, 'tight', 'data parallel')


def build_agent(precision, batch):
    """Same parameters in every process, whatever the batch size."""
    import _fqe_cases as F
    c = case(precision, batch)
    return F.load_params(F.make_agent(c), c)


def global_batch(step):
    import _synth
    return _synth.synth_batch(23, step, B_GLOBAL, O, A)


def flat(net):
    return torch.cat([p.reshape(-1) for p in net.parameters()]).cpu().numpy()


def main():
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    out_dir = Path(sys.argv[1])
    dist.init_process_group('gloo', init_method=f"tcp://127.0.0.1:{os.environ['MASTER_PORT']}", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    Br = B_GLOBAL // world
    sl = slice(rank * Br, (rank + 1) * Br)
    result = {}
    for precision in PRECISIONS:
        ag = build_agent(precision, Br)
        assert ag.world_size == world and ag.engine.comm is None
        metrics = []
        for step in range(STEPS):
            b = tuple(np.ascontiguousarray(x[sl]) for x in global_batch(step))
            metrics.append({k: float(v) for k, v in ag.update(iter([b]), step).items()})
        torch.cuda.synchronize()
        np.savez(out_dir / f'fqe_{precision}_rank{rank}.npz', **{n: flat(getattr(ag, n)) for n in NETS})
        result[precision] = metrics
        del ag
    json.dump(result, open(out_dir / f'metrics_rank{rank}.json', 'w'))
    dist.barrier()
    dist.destroy_process_group()
    print(f'rank {rank} done')


if __name__ == '__main__':
    main()
