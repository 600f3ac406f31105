"""What the two-process pixel workers share (_pixel_dp_worker.py, _pixel_module_dp_worker.py, _proto_pixel_dp_worker.py): the gloo process
group of ranks that all sit on cuda:0, the hooks and frames drawn for the GLOBAL batch with each rank keeping its rows, and the files a
rank leaves for the parent test."""
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


def init_ranks():
    """(rank, world) of this process, its process group up."""
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    return rank, world


def finish_ranks():
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


def rank_rows(b_global, rank, world):
    """(rows per rank, this rank's slice of the global batch)."""
    br = b_global // world
    return br, slice(rank * br, (rank + 1) * br)


def hooks(ag, rows, b_global, eps=True):
    """Shifts, noise and (SMM) the VAE's epsilon drawn for the GLOBAL batch in every process (one stream each), each rank keeping its rows."""
    import _synth
    rs, ns, es = np.random.RandomState(11), _synth.NoiseStream(9), np.random.RandomState(13)
    ag.shift_hook = lambda n: np.ascontiguousarray(rs.randint(0, 9, (b_global, 2)).astype(np.int32)[rows])
    ag.noise_hook = lambda shape: np.ascontiguousarray(ns.draw((b_global, shape[1]))[rows])
    if eps and hasattr(ag, 'eps_hook'):
        ag.eps_hook = lambda shape: np.ascontiguousarray(es.standard_normal((b_global, shape[1])).astype(np.float32)[rows])


def batch(step, rows, b_global, c, hw, act_dim, meta=None):
    """`rows` of step's global batch of random frames; meta(rs) -> the skill / task rows drawn after them, or None."""
    rs = np.random.RandomState(700 + step)
    obs = rs.randint(0, 256, (b_global, c, hw, hw)).astype(np.uint8)
    nxt = rs.randint(0, 256, (b_global, c, hw, hw)).astype(np.uint8)
    b = [obs, rs.uniform(-1, 1, (b_global, act_dim)).astype(np.float32), rs.uniform(0, 1, b_global).astype(np.float32),
         np.full(b_global, 0.99, np.float32), nxt]
    m = meta(rs) if meta else None
    if m is not None:
        b.append(m)
    return tuple(np.ascontiguousarray(x[rows]) for x in b)


def flat(view):
    from exorl_amd import _lib as L
    if hasattr(view, 'flat'):                       # the module engine: every parameter, frozen ones included
        return view.flat(L.T_PARAM).cpu().numpy()
    return torch.cat([p.reshape(-1) for p in view.parameters()]).cpu().numpy()


def run_updates(ag, batches, step_of=lambda i: i):
    """ag.update on each batch in turn; the metrics of every call as plain floats."""
    return [{k: float(v) for k, v in ag.update(iter([b]), step_of(i)).items()} for i, b in enumerate(batches)]


def save(out, name, rank, arrays, metrics):
    torch.cuda.synchronize()
    np.savez(out / f'{name}_rank{rank}.npz', **arrays)
    json.dump(metrics, open(out / f'metrics_{name}_rank{rank}.json', 'w'))
