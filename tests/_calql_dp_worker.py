"""One data-parallel rank of CalQLAgent, run as a fresh child process by tests/test_gpu_calql_dp.py: both ranks sit on cuda:0 and talk gloo, so
AgentEngine.update_steps drives CQL's phases with torch.distributed all-reduces between them (with use_critic_lagrange phase 0 runs as
phases 4 and 5 around the sum-all-reduce of the penalty sums, which are sums of bounded terms; the bound is per row and adds no exchange).
Each rank takes its half of the global batches, bounds and noise blocks the parent replays whole."""
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

O, A, H, B_GLOBAL, N, STEPS = 24, 6, 128, 128, 3, 3
KINDS = ('cql', 'cql-lagrange')
NETS = ('actor', 'critic', 'critic_target')


def case(kind, batch):
    import _grad_grid as G
    return G.Case(kind, O, A, H, batch, N, 'fp32', 21, 'tight', 'data parallel')


def build_agent(kind, batch):
    """Same parameters in every process, whatever the batch size."""
    import _calql_cases as K
    c = case(kind, batch)
    return K.load_params(K.make_agent(c), c)


def global_batch(step):
    """The 6-tuple of the global batch. The bound: -inf on the first half of the rows (nothing bounded there), and on the second half
    10 on every other row (above every value of the fresh critic: everything bounded) and a value inside the critic's range on the rest: a
    rank's own bound rate is not the global one."""
    import _calql_cases as K
    b = K.batch_at(case('cql', B_GLOBAL), step)
    rs = np.random.RandomState(500 + step)
    m = rs.uniform(-0.2, 0.2, B_GLOBAL).astype(np.float32)
    m[:B_GLOBAL // 2] = -np.inf
    m[B_GLOBAL // 2::2] = 10.0
    return b + (m,)


def global_noise(step):
    import _calql_cases as K
    import _synth
    return K.noise_at(case('cql', B_GLOBAL), _synth.NoiseStream(900 + step))


def slice_noise(z, sl):
    """A rank's rows of the five blocks: (B, A) blocks by row, CQL's (n, B, A) blocks along their middle axis."""
    return [np.ascontiguousarray(x[sl] if x.ndim == 2 else x[:, sl]) for x in z]


def hooked(ag, blocks):
    it = iter(blocks)
    ag.noise_hook = lambda shape, kind='normal': next(it)
    return ag


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
    for kind in KINDS:
        ag = build_agent(kind, Br)
        assert ag.world_size == world and ag.engine.comm is None
        metrics = []
        for step in range(STEPS):
            b = tuple(np.ascontiguousarray(x[sl]) for x in global_batch(step))
            z = slice_noise(global_noise(step), sl)
            metrics.append({k: float(v) for k, v in hooked(ag, z).update(iter([b]), step).items()})
        torch.cuda.synchronize()
        np.savez(out_dir / f'calql_{kind}_rank{rank}.npz', cql_scalars=np.asarray(ag.engine.cql_alpha_state(), np.float64),
                 **{n: flat(getattr(ag, n)) for n in NETS})
        result[kind] = metrics
        del ag
    json.dump(result, open(out_dir / f'metrics_rank{rank}.json', 'w'))
    dist.barrier()
    dist.destroy_process_group()
    print(f'rank {rank} done')


if __name__ == '__main__':
    main()
