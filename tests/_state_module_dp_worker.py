"""One data-parallel rank of the reward-free agents on state observations with shard_pretraining=True, run as a fresh child process
(tests/test_gpu_state_module_dp.py starts two of them). Both ranks sit on cuda:0 and talk gloo, so the module's phases and their exchanges
(gradients, BatchNorm1d moments, RMS moments, kNN rows, Proto's rows, SMM's moments of log p*), the sharded actor / critic step and the
metric all-reduces execute for real on a one-GPU box. ICM runs a second time without the flag: the gathered, replicated module."""
import sys
from pathlib import Path

import numpy as np
import torch

import _pixel_dp_common as common
from _pixel_dp_common import flat  # noqa: F401 — the parent test's W.flat

O, A, H, B_GLOBAL, STEPS = 12, 4, 64, 64, 3
KINDS = ['rnd', 'icm', 'icm_apt', 'disagreement', 'diayn', 'aps', 'smm', 'proto']
META = {'diayn': 6, 'aps': 5, 'smm': 4}


def _kw(kind, batch):
    return dict(name=kind, reward_free=True, obs_type='states', obs_shape=(O,), action_shape=(A,), device='cuda:0', lr=1e-4, feature_dim=50,
                hidden_dim=H, critic_target_tau=0.01, num_expl_steps=0, update_every_steps=1, stddev_schedule=0.2, nstep=3, batch_size=batch,
                stddev_clip=0.3, init_critic=True, use_tb=True, use_wandb=False)


def build(kind, batch, shard=True):
    """Same seed -> same initial weights in every process (the constructors' RNG consumption does not depend on the batch size)."""
    from exorl_amd import agents
    torch.manual_seed(33)
    kw = dict(_kw(kind, batch), shard_pretraining=shard)
    if kind == 'rnd':
        return agents.RNDAgent(rnd_rep_dim=16, update_encoder=True, rnd_scale=1.0, **kw)
    if kind == 'icm':
        return agents.ICMAgent(icm_scale=1.0, update_encoder=True, **kw)
    if kind == 'icm_apt':
        return agents.ICMAPTAgent(icm_scale=1.0, knn_rms=True, knn_k=12, knn_avg=True, knn_clip=0.0, update_encoder=True, icm_rep_dim=16, **kw)
    if kind == 'disagreement':
        return agents.DisagreementAgent(update_encoder=True, **kw)
    if kind == 'diayn':
        return agents.DIAYNAgent(update_skill_every_step=50, skill_dim=META['diayn'], diayn_scale=1.0, update_encoder=True, skill_type='uniform', **kw)
    if kind == 'aps':
        return agents.APSAgent(update_task_every_step=50, sf_dim=META['aps'], knn_rms=True, knn_k=12, knn_avg=True, knn_clip=0.0, num_init_steps=0,
                               lstsq_batch_size=64, update_encoder=True, **kw)
    if kind == 'smm':
        return agents.SMMAgent(z_dim=META['smm'], sp_lr=1e-3, vae_lr=1e-2, vae_beta=0.5, state_ent_coef=1.0, latent_ent_coef=1.0,
                               latent_cond_ent_coef=1.0, update_encoder=True, **kw)
    return agents.ProtoAgent(pred_dim=16, proj_dim=32, queue_size=256, num_protos=16, tau=0.1, encoder_target_tau=0.05, topk=3,
                             update_encoder=True, **kw)


def hooks(ag, rows):
    """The actor / critic noise and SMM's epsilon are drawn for the GLOBAL batch in every process, each rank keeping its rows; Proto's
    Categorical uniforms are per prototype, the same on every rank."""
    import _synth
    ns, es, us = _synth.NoiseStream(9), np.random.RandomState(13), np.random.RandomState(17)
    ag.noise_hook = lambda shape: np.ascontiguousarray(ns.draw((B_GLOBAL, shape[1]))[rows])
    if hasattr(ag, 'eps_hook'):
        ag.eps_hook = lambda shape: np.ascontiguousarray(es.standard_normal((B_GLOBAL, shape[1])).astype(np.float32)[rows])
    if hasattr(ag, 'cat_hook'):
        ag.cat_hook = lambda n: us.uniform(0, 1, n).astype(np.float32)


def batch(kind, step, rows=slice(None)):
    """`rows` of step's global batch (+ the meta rows of DIAYN / APS / SMM)."""
    import _synth
    b = list(_synth.synth_batch(43, step, B_GLOBAL, O, A))
    if kind in META:
        rs = np.random.RandomState(600 + step)
        Z = META[kind]
        if kind == 'aps':
            m = rs.standard_normal((B_GLOBAL, Z)).astype(np.float32)
            m /= np.linalg.norm(m, axis=1, keepdims=True)
        else:
            m = np.eye(Z, dtype=np.float32)[rs.randint(0, Z, B_GLOBAL)]
        b.append(m)
    return tuple(np.ascontiguousarray(x[rows]) for x in b)


def views(ag):
    return [('actor', ag.actor), ('critic', ag.critic), ('module', ag.intr)]


def _run(kind, rank, world, out, name, shard=True):
    Br, rows = common.rank_rows(B_GLOBAL, rank, world)
    ag = build(kind, Br, shard)
    assert ag.world_size == world and ag.engine.batch == Br and ag.shard_pretraining is shard
    if shard:               # this rank's rows, no gathered batch
        assert ag.intr.batch == Br and ag.intr.world_size == world and ag.intr.rank == rank
    else:                   # the default: the replicated module on the gathered global batch
        assert ag.intr.batch == world * Br and ag.intr.world_size == 1
    hooks(ag, rows)
    metrics, rewards = [], []
    for step in range(STEPS):
        m = ag.update(iter([batch(kind, step, rows)]), step)
        metrics.append({k: float(v) for k, v in m.items()})
        rewards.append(ag.engine._view(ag.engine.batch_slots().reward, Br).cpu().numpy().copy())
    assert getattr(ag, '_dp', None) is None or not shard          # the sharded step allocates no gather buffers
    arrays = {n: flat(v) for n, v in views(ag)}
    arrays['rms'] = ag.intr._rms.cpu().numpy()
    if ag.intr.bn is not None:
        arrays['bn'] = ag.intr.bn.cpu().numpy()
    if ag.intr.queue is not None:
        arrays['queue'] = ag.intr.queue.cpu().numpy()
        arrays['queue_state'] = np.array([ag.intr.queue_ptr(), ag.intr.counter()], np.int64)
    arrays['module_shape'] = np.array([ag.intr.batch, ag.intr.world_size], np.int64)
    if kind == 'rnd' and shard:            # a snapshot taken inside a sharded run keeps the flag and the module state
        import pickle
        clone = pickle.loads(pickle.dumps(ag))
        assert clone.shard_pretraining is True and clone.intr.world_size == world and clone.intr.batch == Br
        assert torch.equal(clone.intr.flat(), ag.intr.flat()) and torch.equal(clone.intr.bn, ag.intr.bn)
        del clone
    common.save(out, name, rank, arrays, metrics)
    np.save(out / f'reward_{name}_rank{rank}.npy', np.stack(rewards))
    del ag


def main(out):
    rank, world = common.init_ranks()
    for kind in KINDS:
        _run(kind, rank, world, out, kind)
    _run('icm', rank, world, out, 'icm_default', shard=False)
    common.finish_ranks()


if __name__ == '__main__':
    main(Path(sys.argv[1]))
