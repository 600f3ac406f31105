"""Qualifies oracle/intr64.py (the float64 reference of tests/test_gpu_intr_grid.py) and the case table of tests/_intr_grid.py, on the CPU:
  * the twin in float32 reproduces step 0 of the reference's recorded module trajectories (tests/golden/tiny_*.npz);
  * the twin in float32 agrees with the numpy oracle's hand-derived gradients, tensor by tensor;
  * every row of the table meets the conditions its seed was searched for (re-checked, not searched)."""
import numpy as np
import pytest
import torch

import _intr_grid as IG
from _grad_grid import KINK_CAP, MARGIN
from oracle import intr64
from oracle.intr import OracleAPS, OracleDIAYN, OracleDisagreement, OracleICM, OracleICMAPT, OracleRND, OracleSMM
from oracle.proto import PROTO_KEYS, OracleProto, uniform_from_normal
from oracle.intr64 import IntrTwin

GOLD_KINDS = ['rnd', 'icm', 'icm_apt', 'icm_apt-kth', 'disagreement', 'diayn', 'aps', 'smm', 'proto']
MODULE = {'rnd': 'rnd', 'icm': 'icm', 'icm_apt': 'icm', 'disagreement': 'disagreement', 'diayn': 'diayn', 'aps': 'aps', 'smm': 'smm'}
LOSS_KEY = {'rnd': 'rnd_loss', 'icm': 'icm_loss', 'icm_apt': 'icm_loss', 'disagreement': 'disagreement_loss', 'diayn': 'diayn_loss', 'aps': 'aps_loss', 'smm': 'loss_vae', 'proto': 'repr_loss'}
SLOT_KEY = {intr64.IM_INTR_REWARD: 'intr_reward', intr64.IM_EXTR_REWARD: 'extr_reward', intr64.IM_ACC: 'diayn_acc',
            intr64.IM_ENT_REWARD: 'intr_ent_reward', intr64.IM_SF_REWARD: 'intr_sf_reward'}
# the measured worst max|g32 - g_oracle| / max|g_oracle| over the tiny shapes below (test_twin32_gradients_vs_numpy_oracle prints it per kind);
# the assertion is 4 x this
ORACLE_WORST = 5.9e-7


def _gold_case(gold, kind):
    z = np.load(gold / f'tiny_{kind}.npz')
    base = kind.partition('-')[0]
    if base == 'proto':                  # O5 pred8 proj16 protos6 queue24 topk3; noise/0 is the normal draw behind the Categorical's uniforms
        p = [z['init/' + k.replace('.', '/', 1)] for k in PROTO_KEYS]
        b = dict(obs=z['batch/0/0'], next_obs=z['batch/0/4'], extr=z['batch/0/2'].reshape(-1), u=uniform_from_normal(z['noise/0']))
        return z, base, p, dict(num_protos=6, queue_size=24, knn_k=3), b
    mod = MODULE[base]
    keys = [k[len(f'init/{mod}/'):] for k in z.files if k.startswith(f'init/{mod}/') and 'normalize_obs' not in k]
    p = [z[f'init/{mod}/{k}'] for k in keys]
    kw = {}
    if base == 'icm_apt':
        kw = dict(knn_k=3, knn_avg=True, knn_rms=True, knn_clip=0.0)
        if kind.endswith('kth'):
            kw.update(knn_avg=False, knn_clip=0.0005)
    if base == 'aps':
        kw = dict(knn_k=3, knn_avg=True, knn_rms=True, knn_clip=0.0001)
    bt = [z[f'batch/0/{j}'] for j in range(6 if base in ('diayn', 'aps', 'smm') else 5)]
    b = dict(obs=bt[0], action=bt[1], next_obs=bt[4], extr=bt[2].reshape(-1), skill=bt[5] if len(bt) > 5 else None)
    if base == 'smm':                    # noise/0 is the VAE's epsilon of step 0
        b['eps'] = z['noise/0']
    return z, base, p, kw, b


@pytest.mark.parametrize('kind', GOLD_KINDS)
def test_twin32_reproduces_step0_of_the_recorded_reference(gold, kind):
    z, base, p, kw, b = _gold_case(gold, kind)
    tw = IntrTwin(base, p, dtype=torch.float32, **kw)
    res = tw.update(b)
    r, m, _ = tw.reward(b, params_after=tw.adam_first_step(res.grads))
    atol = 3e-6 if base == 'smm' else 2e-6
    if 'intr_reward' in z.files:         # SMM's file records the metrics alone
        np.testing.assert_allclose(r.reshape(-1, 1), z['intr_reward'][0], rtol=1e-4, atol=atol, err_msg=f'{kind} intr reward')
    keys = [str(k) for k in z['metric_keys']]
    want = dict(zip(keys, z['metrics'][0]))
    got = {LOSS_KEY[base]: res.metrics[intr64.IM_LOSS]}
    got.update({SLOT_KEY[s]: v for s, v in {**res.metrics, **m}.items() if s in SLOT_KEY and (base != 'smm' or s < 3)})      # SMM reuses the slots from 3 on
    if base == 'rnd':
        got.update(pred_error_mean=m[intr64.IM_RMS_MEAN], pred_error_std=m[intr64.IM_RMS_STD])
    if base == 'smm':
        got.update(log_p_star=m[3], pred_log_ratios=m[4], loss_pred=m[5], latent_cond_ent_coef=m[6], latent_ent_coef=float(np.log(4.0)))
    for k, v in got.items():
        assert k in want, (k, keys)
        np.testing.assert_allclose(v, want[k], rtol=1e-4, atol=atol, err_msg=f'{kind} {k}')


ORACLE_SHAPES = [('rnd', 5, 3, 32, 16, 8, {}), ('rnd', 9, 2, 50, 5, 7, {}), ('icm', 5, 3, 32, 0, 8, {}), ('icm', 9, 2, 50, 0, 7, {}),
                 ('icm_apt', 5, 3, 32, 16, 8, dict(knn_k=3)), ('icm_apt', 9, 2, 50, 5, 7, dict(knn_k=3)),
                 ('disagreement', 5, 3, 32, 0, 8, {}), ('disagreement', 9, 2, 50, 0, 7, dict(n_models=2)),
                 ('diayn', 5, 3, 32, 4, 8, {}), ('diayn', 9, 2, 50, 5, 7, {}), ('aps', 5, 3, 32, 4, 8, dict(knn_k=3)), ('aps', 9, 2, 50, 5, 7, dict(knn_k=3)),
                 ('smm', 5, 3, 32, 4, 8, {}), ('smm', 9, 2, 50, 5, 7, {}),
                 ('proto', 5, 3, 16, 8, 8, dict(num_protos=6, queue_size=24, knn_k=3)), ('proto', 9, 2, 36, 20, 7, dict(num_protos=10, queue_size=40, knn_k=3))]


@pytest.mark.parametrize('kind,O,A,H,R,B,opts', ORACLE_SHAPES, ids=[f'{s[0]}-O{s[1]}H{s[3]}B{s[5]}' for s in ORACLE_SHAPES])
def test_twin32_gradients_vs_numpy_oracle(kind, O, A, H, R, B, opts):
    c = IG.Case(kind, O, A, H, R, B, 'fp32', 7, opts, '')
    p, b = IG.params(c), IG.batch(c)
    if kind == 'rnd':
        om = OracleRND(p)
        om.update(b['obs'])
    elif kind == 'icm':
        om = OracleICM(p)
        om.update(b['obs'], b['action'], b['next_obs'])
    elif kind == 'icm_apt':
        om = OracleICMAPT(p, **opts)
        om.update(b['obs'], b['action'], b['next_obs'])
    elif kind == 'disagreement':
        om = OracleDisagreement(p, n_models=IG.n_models(c))
        om.update(b['obs'], b['action'], b['next_obs'])
    elif kind == 'diayn':
        om = OracleDIAYN(p)
        om.update(b['skill'], b['next_obs'])
    elif kind == 'aps':
        om = OracleAPS(p, **opts)
        om.update(b['skill'], b['next_obs'])
    elif kind == 'smm':
        om = OracleSMM(p)
        om.update_vae(np.concatenate([b['obs'], b['skill']], 1), b['eps'])
        om.update_pred(b['obs'], b['skill'])
        om.last_grads = om.last_pred_grads + om.last_vae_grads
    else:
        om = OracleProto(p, queue_size=opts['queue_size'])
        om.update(b['obs'], b['next_obs'])
        om.last_grads = om.last_grads + [om.last_dobs]
    res = IG.make_twin(c, torch.float32).update(IG.twin_batch(c))
    worst = 0.0
    for i, want in enumerate(om.last_grads):
        e = float(np.abs(res.grads[i].reshape(want.shape) - want).max() / np.abs(want).max())
        worst = max(worst, e)
    print(f'[intr64] {kind} O{O} H{H} B{B}: worst max|g32 - g_oracle| / max|g_oracle| = {worst:.2e}')
    assert worst <= 4 * ORACLE_WORST, (kind, worst)


@pytest.mark.parametrize('c', [pytest.param(c, id=IG.case_id(c)) for c in IG.CASES])
def test_the_table_row_meets_its_conditions(c):
    """twin32 and twin64 take identical discrete decisions, every margin >= MARGIN, |K| <= KINK_CAP at the precision's delta: conditions the
    seed was searched for, so that no case of the GPU grid falls back to a coarse bar."""
    assert IG.qualifies(c) is None, (IG.case_id(c), IG.qualifies(c))


def test_the_table_is_well_formed():
    ids = [IG.case_id(c) for c in IG.CASES]
    assert len(set(ids)) == len(ids)
    assert all(c.why and c.kind in intr64.KINDS and c.precision in IG.KINK_DELTA for c in IG.CASES)
    assert KINK_CAP == 64 and MARGIN == 1e-4
