"""One data-parallel rank of Proto's pixel pretraining path (ProtoAgent(..., shard_pretraining=True), reward_free=True), run as a fresh child
process (tests/test_gpu_proto_pixel_dp.py starts two of them). Both ranks sit on cuda:0 and talk gloo, so the module phases and their
gathers and gradient sums, the encoder step's exchange, the sharded DDPG pixel step and the metric all-reduces run for real on one GPU.

Two workloads, each on its golden fixture with every rank holding its rows of the global batch: the miniature of
tests/golden/pixel_proto.npz (2 ranks x 2 rows) and config 4 (tests/golden/config4_proto_b1024.npz, 2 ranks x 512 rows) in fp32 and bf16x6."""
import sys
from pathlib import Path

import numpy as np
import torch

import _pixel_dp_common as common

GOLD = common.ROOT / 'tests' / 'golden'
CONFIG4_PRECISIONS = ('fp32', 'bf16x6')


def proto_agent(z, batch, precision='fp32', shard=True):
    from exorl_amd import agents
    C_, HW, A, F, H, B, N, PD, PJ, Q, NP = [int(v) for v in z['dims']]
    return agents.ProtoAgent(pred_dim=PD, proj_dim=PJ, queue_size=Q, num_protos=NP, tau=0.1, encoder_target_tau=0.05, topk=3, update_encoder=True,
                             shard_pretraining=shard, name='proto', reward_free=True, obs_type='pixels', obs_shape=(C_, HW, HW), action_shape=(A,),
                             device='cuda:0', lr=1e-4, feature_dim=F, hidden_dim=H, critic_target_tau=0.01, num_expl_steps=2000,
                             update_every_steps=2, stddev_schedule=0.2, nstep=3, batch_size=batch, stddev_clip=0.3, init_critic=True,
                             use_tb=True, use_wandb=False, precision=precision)


def load_fixture_params(ag, z):
    """test_gpu_pixels.py::test_pixel_proto_vs_reference's weights."""
    import _synth
    from oracle import pixels
    C_, HW, A, F, H, B, N, PD, PJ, Q, NP = [int(v) for v in z['dims']]
    esh, ash, csh = pixels.pixel_param_shapes(C_, A, F, H, 39200)
    for i, (view, sh) in enumerate(zip((ag.encoder, ag.actor, ag.critic), (esh, ash, csh))):
        view.load_state_dict({k: torch.from_numpy(v) for k, v in _synth.synth_params(sh, 50 + i).items()})
    ag.engine.sync_target()
    psh = [[('weight', (PD, 39200)), ('bias', (PD,))], [('trunk.0.weight', (PJ, PD)), ('trunk.0.bias', (PJ,)), ('trunk.2.weight', (PD, PJ)),
                                                        ('trunk.2.bias', (PD,))], [('weight', (NP, PD))]]
    for i, (view, sh) in enumerate(zip((ag.predictor, ag.projector, ag.protos), psh)):
        view.load_state_dict({k: torch.from_numpy(v) for k, v in _synth.synth_params(sh, 53 + i).items()})
    for p, t in zip(ag.predictor.parameters(), ag.predictor_target.parameters()):
        t.copy_(p)
    ag.engine.encoder_target(init=True)


def load_config4_params(ag, z):
    """test_gpu_pixels.py::_config4_agent's weights."""
    import _synth
    C_, HW, A, F, H, B, N, PD, PJ, Q, NP = [int(v) for v in z['dims']]
    ps = _synth.config4_params(C_, A, F, H, PD, PJ, NP)
    for nm in ('encoder', 'actor', 'critic', 'predictor', 'projector', 'protos'):
        view = getattr(ag, nm)
        sd = view.state_dict()
        view.load_state_dict({k: torch.from_numpy(v).reshape(sd[k].shape) for k, v in ps[nm].items()})
    ag.engine.sync_target()
    for p, t in zip(ag.predictor.parameters(), ag.predictor_target.parameters()):
        t.copy_(p)
    ag.engine.encoder_target(init=True)


def run_fixture(ag, z, rows):
    """The three update() calls of test_pixel_proto_vs_reference; shifts and noise are drawn for the global batch, each rank keeps `rows`."""
    import _synth
    B, N = int(z['dims'][5]), int(z['dims'][6])
    noise = _synth.NoiseStream(21)
    shifts, us = iter(z['shifts']), iter(z['cat_uniform'])
    ag.noise_hook = lambda shape: np.ascontiguousarray(noise.draw((B, shape[1]))[rows])
    ag.shift_hook = lambda n: np.ascontiguousarray(np.asarray(next(shifts))[rows])
    ag.cat_hook = lambda n: next(us)
    ms = []
    for i in range(N):
        batch = tuple(np.ascontiguousarray(z[f'batch/{i}/{k}'][rows]) for k in ('obs', 'action', 'reward', 'discount', 'next_obs'))
        ms.append({k: float(v) for k, v in ag.update(iter([batch]), 2 * i).items()})
    return ms


def run_config4(ag, z, rows):
    """The three update() calls of test_config4_proto_pixels_b1024_vs_reference, each rank on `rows` of the 1024-row batch."""
    import _synth
    C_, HW, A, F, H, B, N, PD, PJ, Q, NP = [int(v) for v in z['dims']]
    ns = _synth.NoiseStream(22)
    ag.noise_hook = lambda shape: np.ascontiguousarray(ns.draw((B, shape[1]))[rows])
    ms = []
    for i in range(N):
        obs, nobs, act, rew, disc, so, sn, u = _synth.config4_inputs(i, B, C_, HW, A, NP)
        sh = [np.ascontiguousarray(so[rows]), np.ascontiguousarray(sn[rows])]
        ag.shift_hook = lambda n: sh.pop(0)
        ag.cat_hook = lambda n: u
        batch = tuple(np.ascontiguousarray(x[rows]) for x in (obs, act, rew, disc, nobs))
        ms.append({k: float(v) for k, v in ag.update(iter([batch]), 2 * i).items()})
    return ms


def state(ag, sample=False):
    """Every view's state_dict (config 4: every 997th element of the large tensors), the queue and its pointer, the module's counter."""
    out = {}
    for nm in ('encoder', 'encoder_target', 'actor', 'critic', 'predictor', 'projector', 'protos', 'predictor_target'):
        for k, t in getattr(ag, nm).state_dict().items():
            v = t.detach().cpu().numpy().reshape(-1)
            out[f'{nm}/{k}'] = v[::997] if (sample and v.size > 4096) else v
    out['queue'] = ag.queue.cpu().numpy()
    out['queue_ptr'] = np.array(ag.queue_ptr)
    out['counter'] = np.array(ag.intr.counter(), np.uint64)
    return out


def main(out):
    rank, world = common.init_ranks()
    z = np.load(GOLD / 'pixel_proto.npz')
    Br, rows = common.rank_rows(int(z['dims'][5]), rank, world)
    ag = proto_agent(z, Br)
    assert ag.world_size == world and ag.intr.world_size == world and ag.intr.batch == Br
    load_fixture_params(ag, z)
    ms = run_fixture(ag, z, rows)
    common.save(out, 'fixture', rank, state(ag), ms)
    del ag
    z = np.load(GOLD / 'config4_proto_b1024.npz')
    Br, rows = common.rank_rows(int(z['dims'][5]), rank, world)
    for precision in CONFIG4_PRECISIONS:
        ag = proto_agent(z, Br, precision)
        load_config4_params(ag, z)
        ms = run_config4(ag, z, rows)
        common.save(out, f'config4_{precision}', rank, state(ag, sample=True), ms)
        del ag
    common.finish_ranks()


if __name__ == '__main__':
    main(Path(sys.argv[1]))
