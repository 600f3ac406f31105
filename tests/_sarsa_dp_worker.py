"""One data-parallel rank of OneStepTD3BCAgent, run as a fresh child process by tests/test_gpu_sarsa_dp.py: both ranks sit on cuda:0 and talk
gloo, so AgentEngine.update_steps drives TD3+BC's four phases with torch.distributed all-reduces between them (the SARSA rule is per row and
adds no exchange). Each rank takes its half of the global batches, next actions and noise blocks the parent replays whole."""
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
    import _rebrac_twin as R
    return R.Case(O, A, H, batch, precision, 21, 'tight', 'data parallel')


def build_agent(precision, batch):
    """Same parameters in every process, whatever the batch size."""
    import _rebrac_twin as R
    import _sarsa_twin as S
    c = case(precision, batch)
    return R.load_params(S.make_agent(c), c)


def global_batch(step):
    """The 7-tuple of the global batch: the first half of the rows has valid next actions three times in four, the second half one in four,
    so a rank's own mean of next_valid is not the global one."""
    import _rebrac_twin as R
    b = R.batch(case('fp32', B_GLOBAL), step)
    rs = np.random.RandomState(500 + step)
    valid = (rs.uniform(size=B_GLOBAL) < np.where(np.arange(B_GLOBAL) < B_GLOBAL // 2, 0.75, 0.25)).astype(np.float32)
    a_next = (rs.uniform(-1.0, 1.0, (B_GLOBAL, A)) * valid[:, None]).astype(np.float32)
    return b[:5] + (a_next, valid)


def global_noise(step):
    import _synth
    ns = _synth.NoiseStream(900 + step)
    return [ns.draw((B_GLOBAL, A)), ns.draw((B_GLOBAL, A))]


def hooked(ag, blocks):
    it = iter(blocks)
    ag.noise_hook = lambda shape: next(it)
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
    for precision in PRECISIONS:
        ag = build_agent(precision, Br)
        assert ag.world_size == world and ag.engine.comm is None
        metrics = []
        for step in range(STEPS):
            b = tuple(np.ascontiguousarray(x[sl]) for x in global_batch(step))
            z = [np.ascontiguousarray(x[sl]) for x in global_noise(step)]
            metrics.append({k: float(v) for k, v in hooked(ag, z).update(iter([b]), step).items()})
        torch.cuda.synchronize()
        np.savez(out_dir / f'sarsa_{precision}_rank{rank}.npz', **{n: flat(getattr(ag, n)) for n in NETS})
        result[precision] = metrics
        del ag
    json.dump(result, open(out_dir / f'metrics_rank{rank}.json', 'w'))
    dist.barrier()
    dist.destroy_process_group()
    print(f'rank {rank} done')


if __name__ == '__main__':
    main()
