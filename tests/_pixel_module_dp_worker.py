"""One data-parallel rank of the pixel pretraining path (reward_free=True), run as a fresh child process (tests/test_gpu_pixel_module_dp.py
starts two of them). Both ranks sit on cuda:0 and talk gloo, so the module phases and their exchanges, the encoder-step phases, RND's
BatchNorm2d exchanges, the sharded DDPG pixel step and the metric all-reduces execute for real on a one-GPU box."""
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

C_, HW, A, F, H, B_GLOBAL, STEPS = 3, 64, 6, 32, 128, 64, 3
KINDS = ['rnd', 'icm', 'icm_apt', 'disagreement', 'diayn', 'aps', 'smm']
META = {'diayn': 8, 'aps': 5, 'smm': 4}


def _kw(kind, batch):
    return dict(name=kind, reward_free=True, obs_type='pixels', obs_shape=(C_, HW, HW), action_shape=(A,), device='cuda:0', lr=1e-4,
                feature_dim=F, hidden_dim=H, critic_target_tau=0.01, num_expl_steps=0, update_every_steps=1, stddev_schedule=0.2, nstep=3,
                batch_size=batch, stddev_clip=0.3, init_critic=True, use_tb=True, use_wandb=False)


def build(kind, batch):
    """Same seed -> same initial weights in every process (the constructors' RNG consumption does not depend on the batch size)."""
    from exorl_amd import agents
    torch.manual_seed(33)
    kw = _kw(kind, batch)
    if kind == 'rnd':
        return agents.RNDAgent(rnd_rep_dim=32, update_encoder=True, rnd_scale=1.0, **kw)
    if kind == 'icm':
        return agents.ICMAgent(icm_scale=1.0, update_encoder=True, **kw)
    if kind == 'icm_apt':
        return agents.ICMAPTAgent(icm_scale=1.0, knn_rms=True, knn_k=12, knn_avg=True, knn_clip=0.0, update_encoder=True, icm_rep_dim=32, **kw)
    if kind == 'disagreement':
        return agents.DisagreementAgent(update_encoder=True, **kw)
    if kind == 'diayn':
        return agents.DIAYNAgent(update_skill_every_step=50, skill_dim=META['diayn'], diayn_scale=1.0, update_encoder=True, skill_type='uniform', **kw)
    if kind == 'aps':
        return agents.APSAgent(update_task_every_step=50, sf_dim=META['aps'], knn_rms=True, knn_k=12, knn_avg=True, knn_clip=0.0, num_init_steps=0,
                               lstsq_batch_size=64, update_encoder=True, **kw)
    return agents.SMMAgent(z_dim=META['smm'], sp_lr=1e-3, vae_lr=1e-2, vae_beta=0.5, state_ent_coef=1.0, latent_ent_coef=1.0,
                           latent_cond_ent_coef=1.0, update_encoder=True, **kw)


def hooks(ag, rows, eps=True):
    """Shifts, noise and (SMM) the VAE's epsilon drawn for the GLOBAL batch in every process (one stream each), each rank keeping its rows."""
    import _synth
    rs, ns, es = np.random.RandomState(11), _synth.NoiseStream(9), np.random.RandomState(13)
    ag.shift_hook = lambda n: np.ascontiguousarray(rs.randint(0, 9, (B_GLOBAL, 2)).astype(np.int32)[rows])
    ag.noise_hook = lambda shape: np.ascontiguousarray(ns.draw((B_GLOBAL, shape[1]))[rows])
    if eps and hasattr(ag, 'eps_hook'):
        ag.eps_hook = lambda shape: np.ascontiguousarray(es.standard_normal((B_GLOBAL, shape[1])).astype(np.float32)[rows])


def batch(kind, step, rows=slice(None)):
    rs = np.random.RandomState(700 + step)
    obs = rs.randint(0, 256, (B_GLOBAL, C_, HW, HW)).astype(np.uint8)
    nxt = rs.randint(0, 256, (B_GLOBAL, C_, HW, HW)).astype(np.uint8)
    b = [obs, rs.uniform(-1, 1, (B_GLOBAL, A)).astype(np.float32), rs.uniform(0, 1, B_GLOBAL).astype(np.float32),
         np.full(B_GLOBAL, 0.99, np.float32), nxt]
    if kind in ('diayn', 'smm'):
        b.append(np.eye(META[kind], dtype=np.float32)[rs.randint(0, META[kind], B_GLOBAL)])
    elif kind == 'aps':
        t = rs.standard_normal((B_GLOBAL, META[kind])).astype(np.float32)
        b.append(t / np.linalg.norm(t, axis=1, keepdims=True))
    return tuple(np.ascontiguousarray(x[rows]) for x in b)


def views(ag):
    return [('encoder', ag.encoder), ('actor', ag.actor), ('critic', ag.critic), ('module', ag.intr)]


def flat(view):
    from exorl_amd import _lib as L
    if hasattr(view, 'flat'):                       # the module engine: every parameter, frozen ones included
        return view.flat(L.T_PARAM).cpu().numpy()
    return torch.cat([p.reshape(-1) for p in view.parameters()]).cpu().numpy()


def _run(kind, rank, world, out, name, eps=True):
    Br = B_GLOBAL // world
    rows = slice(rank * Br, (rank + 1) * Br)
    ag = build(kind, Br)
    assert ag.world_size == world and ag.engine.batch == Br and ag.intr.batch == Br and ag.intr.world_size == world
    hooks(ag, rows, eps)
    metrics = []
    for step in range(STEPS):
        m = ag.update(iter([batch(kind, step, rows)]), step)
        metrics.append({k: float(v) for k, v in m.items()})
    torch.cuda.synchronize()
    arrays = {n: flat(v) for n, v in views(ag)}
    arrays['rms'] = ag.intr._rms.cpu().numpy()
    arrays['bn2d'] = ag.engine.bn2d().cpu().numpy()
    np.savez(out / f'{name}_rank{rank}.npz', **arrays)
    json.dump(metrics, open(out / f'metrics_{name}_rank{rank}.json', 'w'))
    del ag


def main(out):
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    for kind in KINDS:
        _run(kind, rank, world, out, kind)
    _run('smm', rank, world, out, 'smm_unhooked', eps=False)          # the device's epsilon: each rank draws its rows of the global draw
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main(Path(sys.argv[1]))
