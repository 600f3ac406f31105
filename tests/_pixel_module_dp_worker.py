"""One data-parallel rank of the pixel pretraining path (reward_free=True), run as a fresh child process (tests/test_gpu_pixel_module_dp.py
starts two of them). Both ranks sit on cuda:0 and talk gloo, so the module phases and their exchanges, the encoder-step phases, RND's
BatchNorm2d exchanges, the sharded DDPG pixel step and the metric all-reduces execute for real on a one-GPU box."""
import sys
from pathlib import Path

import numpy as np
import torch

import _pixel_dp_common as common
from _pixel_dp_common import flat  # noqa: F401 — the parent test's W.flat

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
    common.hooks(ag, rows, B_GLOBAL, eps)


def batch(kind, step, rows=slice(None)):
    def meta(rs):
        if kind in ('diayn', 'smm'):
            return np.eye(META[kind], dtype=np.float32)[rs.randint(0, META[kind], B_GLOBAL)]
        if kind == 'aps':
            t = rs.standard_normal((B_GLOBAL, META[kind])).astype(np.float32)
            return t / np.linalg.norm(t, axis=1, keepdims=True)
    return common.batch(step, rows, B_GLOBAL, C_, HW, A, meta)


def views(ag):
    return [('encoder', ag.encoder), ('actor', ag.actor), ('critic', ag.critic), ('module', ag.intr)]


def _run(kind, rank, world, out, name, eps=True):
    Br, rows = common.rank_rows(B_GLOBAL, rank, world)
    ag = build(kind, Br)
    assert ag.world_size == world and ag.engine.batch == Br and ag.intr.batch == Br and ag.intr.world_size == world
    hooks(ag, rows, eps)
    metrics = common.run_updates(ag, (batch(kind, step, rows) for step in range(STEPS)))
    arrays = {n: flat(v) for n, v in views(ag)}
    arrays['rms'] = ag.intr._rms.cpu().numpy()
    arrays['bn2d'] = ag.engine.bn2d().cpu().numpy()
    common.save(out, name, rank, arrays, metrics)
    del ag


def main(out):
    rank, world = common.init_ranks()
    for kind in KINDS:
        _run(kind, rank, world, out, kind)
    _run('smm', rank, world, out, 'smm_unhooked', eps=False)          # the device's epsilon: each rank draws its rows of the global draw
    common.finish_ranks()


if __name__ == '__main__':
    main(Path(sys.argv[1]))
