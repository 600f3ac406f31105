"""The module grid: the cases tests/test_intr64.py qualifies on the CPU and tests/test_gpu_intr_grid.py runs on the GPU, and what the two
share (inputs from seeds, the float64 / float32 twins of oracle/intr64.py). The kink treatment and the per-tensor error are those of
tests/_grad_grid.py, unchanged.

One case = one step of one IntrEngine at world_size 1 from seeded parameters and rows. Columns of CASES:
  kind       rnd | icm | icm_apt | disagreement | diayn | aps | smm | proto
  O A H R B  observation width, action width, hidden width, rep_dim / skill_dim / sf_dim / z_dim, batch; Proto: R = pred_dim, H = proj_dim
  precision  fp32 | bf16x6 | bf16x3
  seed       parameters synth_params(seed), rows synth_batch(seed + 2, 0), skill / task / z rows RandomState(seed + 3), SMM's epsilon NoiseStream(seed + 4), Proto's
             uniforms RandomState(seed + 4). Searched once on the CPU:
             smallest seed >= the row's base for which the float32 and float64 twins take identical discrete decisions, every decision has
             a float64 margin >= MARGIN and the near-kink set is within KINK_CAP; the tests re-check, they do not search
  opts       what the row changes of the module's configuration (IntrEngine / IntrTwin keywords; Proto: num_protos, queue_size, knn_k = topk), and
               layout='skill_cols'  the rows are [obs | skill] with row stride O + R, the skill read in place (DIAYN / APS / SMM, whose VAE reads
                                    the whole row)
               layout='misaligned'  next_obs starts one float past a 16-byte boundary with row stride O + 1
               u='mid_bin'          Proto's uniforms are not drawn: with B rows a pick's share of the CDF is about 1 / B, so from B = 963 on no
                                    draw of 18 uniforms keeps every pick MARGIN away from a boundary. Each u_p is put at the middle of a bin
                                    of twin64's own table (after its own Adam step) that is at least 3 MARGIN wide, the bin chosen by the seed
                                    among those: picks all over the batch, every chunk of the blocked walk included
  why        the edge the row is there for
L (bf16x3's bar) is the number of chained matrix products on the longest forward-plus-backward path of the kind's loss: L_OF."""
from collections import namedtuple
import numpy as np
import torch

import _synth
from _grad_grid import KINK_CAP, MARGIN
from oracle.intr import intr_param_shapes, smm_param_shapes
from oracle.proto import proto_param_shapes
from oracle.intr64 import IntrTwin

Case = namedtuple('Case', 'kind O A H R B precision seed opts why')

KINK_DELTA = {'fp32': 2.0 ** -18, 'bf16x6': 2.0 ** -18, 'bf16x3': 2.0 ** -14}
KINK_FLOOR = {'fp32': 2.0 ** -22, 'bf16x6': 2.0 ** -22, 'bf16x3': 2.0 ** -16}
# rnd / diayn / aps: three layers forward, two dgrads and a wgrad back. icm / disagreement: two forward, dgrad + wgrad (or the dgrad to the
# input rows) back. icm_apt: the trunk in front of icm's two and behind its backward pass
# proto: predictor, two projector layers and the scores forward, their three dgrads and the predictor's wgrad back. smm: the VAE's encoder (2),
# head, decoder (3) forward and as many back
L_OF = {'rnd': 6, 'diayn': 6, 'aps': 6, 'icm': 4, 'disagreement': 4, 'icm_apt': 6, 'proto': 8, 'smm': 12}
TRAIN0 = ('rnd', 'icm', 'icm_apt', 'disagreement', 'diayn', 'aps', 'proto')      # SMM's reward is made of its step's losses: no reward-only entry

CASES = [
    Case('rnd', 9, 2, 50, 5, 7, 'fp32', 100, {}, 'H % 4 != 0: scalar-load GEMM, colsum_kernel, separate relu_bwd_kernel; R < 64; B % 4 != 0 in the wave-per-row kernels'),
    Case('rnd', 24, 2, 64, 64, 300, 'fp32', 200, {}, 'R = one full lane pass; B > 256: second pass of bn_clamp_kernel ragged; colsum4 128-row loop with a 44-row tail'),
    Case('rnd', 12, 2, 32, 130, 1100, 'fp32', 308, dict(clip_val=1.0), 'three lane passes ragged; B > 1024 in the single-block reward / moments kernels; clamp active on many elements'),
    Case('rnd', 40, 2, 32, 16, 7, 'fp32', 400, dict(encoded=True), 'RND on encodings, dobs_out: the route the pixel agent drives (train 1, and train 2 for the step alone)'),
    Case('icm', 9, 2, 50, 0, 7, 'fp32', 500, {}, 'narrow icm_err_kernel, odd D; H % 4 != 0'),
    Case('icm', 2048, 6, 32, 0, 6, 'fp32', 600, {}, 'first width of icm_err_wide_kernel: two full float4 passes'),
    Case('icm', 2052, 3, 32, 0, 5, 'fp32', 700, {}, 'wide, ragged last float4 pass (513)'),
    Case('icm', 2050, 3, 32, 0, 5, 'fp32', 800, {}, 'D >= 2048 but D % 4 != 0: narrow kernel, 33 lane passes'),
    Case('icm', 2048, 3, 32, 0, 5, 'fp32', 900, dict(layout='misaligned'), 'next_obs one float off a 16-byte boundary, ld 2049: alignment fall-back to the narrow kernel'),
    Case('icm_apt', 9, 2, 50, 5, 7, 'fp32', 1000, dict(knn_k=7, knn_avg=True, knn_rms=True, knn_clip=0.0), 'k = n_tgt with 57 padded +inf columns'),
    Case('icm_apt', 17, 6, 64, 64, 130, 'fp32', 1100, dict(knn_k=1, knn_avg=False, knn_rms=False, knn_clip=5e-4), 'k = 1, knn_avg=False, no RMS, clip active'),
    Case('icm_apt', 24, 6, 32, 130, 1100, 'fp32', 1200, dict(knn_k=12, knn_avg=True, knn_rms=True, knn_clip=0.0), '13200 values through block_moments; B > 1024 in pbe_reward_kernel'),
    Case('icm_apt', 12, 4, 32, 16, 100, 'fp32', 1300, dict(knn_k=64, knn_avg=True, knn_rms=True, knn_clip=0.0), 'KNN_MAX_K'),
    Case('disagreement', 9, 2, 50, 0, 7, 'fp32', 1400, dict(n_models=2), 'smallest ensemble with a defined variance'),
    Case('disagreement', 24, 6, 64, 0, 130, 'fp32', 1500, dict(n_models=0), 'n_models 0 -> 5, the default'),
    Case('disagreement', 2048, 2, 16, 0, 5, 'fp32', 1600, dict(n_models=8), 'wide reward kernel, EXORL_MAX_ENSEMBLE fully unrolled'),
    Case('disagreement', 2052, 2, 16, 0, 5, 'fp32', 1700, dict(n_models=3), 'wide, ragged last float4 pass'),
    Case('disagreement', 2050, 2, 16, 0, 5, 'fp32', 1800, dict(n_models=3), 'narrow kernels above 2048'),
    Case('diayn', 9, 2, 50, 5, 7, 'fp32', 1900, dict(layout='skill_cols'), 'rows [obs | skill], ld O + S: strided skill columns'),
    Case('diayn', 12, 2, 32, 64, 130, 'fp32', 2000, dict(layout='skill_cols'), 'S = 64: one full lane pass of diayn_kernel'),
    Case('diayn', 12, 2, 32, 65, 130, 'fp32', 2100, dict(layout='skill_cols'), 'S = 65: second lane pass with one live lane'),
    Case('diayn', 12, 2, 32, 130, 1100, 'fp32', 2203, dict(layout='skill_cols'), 'S = 130: three lane passes ragged; B = 1100'),
    Case('aps', 9, 2, 50, 5, 7, 'fp32', 2300, dict(knn_k=3, knn_clip=1e-4, layout='skill_cols'), 'sf 5 < 64 in aps_loss_kernel; B = 7'),
    Case('aps', 12, 2, 64, 10, 130, 'fp32', 2400, dict(knn_k=12, knn_clip=1e-4, layout='skill_cols'), 'the shipped sf_dim 10 and k 12'),
    Case('aps', 12, 2, 32, 70, 1100, 'fp32', 2500, dict(knn_k=12, knn_clip=1e-4, layout='skill_cols'), 'sf 70: D across 64; stride loop of aps_sf_reward_kernel past 1024 rows'),
    Case('smm', 9, 2, 50, 5, 7, 'fp32', 4000, dict(layout='skill_cols'), 'narrow vae_out_kernel; fixed 150 / 128 VAE widths beside H % 4 != 0'),
    Case('smm', 24, 2, 64, 4, 130, 'fp32', 4100, dict(layout='skill_cols'), 'the shipped z_dim 4; B = 130'),
    Case('smm', 2044, 2, 32, 4, 5, 'fp32', 4200, dict(layout='skill_cols'), 'W = 2048, obs_ld 2048: first width of vae_out_wide_kernel'),
    Case('smm', 2046, 2, 32, 4, 5, 'fp32', 4300, dict(layout='skill_cols'), 'W = 2050: narrow kernel above 2048'),
    Case('smm', 2044, 2, 32, 4, 5, 'fp32', 4400, dict(layout='skill_cols', encoded=True), 'encodings, W = 2048: the reward branch without the goal prior'),
    Case('proto', 9, 2, 36, 20, 7, 'fp32', 5000, dict(num_protos=10, queue_size=40, knn_k=3), 'protos not a multiple of 16 (live masking); D < 64'),
    Case('proto', 12, 2, 36, 130, 130, 'fp32', 5100, dict(num_protos=70, queue_size=140, knn_k=3), 'P and D across 64 in the Sinkhorn, loss and l2norm kernels'),
    Case('proto', 6, 2, 8, 8, 963, 'fp32', 5200, dict(num_protos=18, queue_size=36, knn_k=3, u='mid_bin'), 'last batch of proto_candidates_kernel<16>: 65484 B of dynamic LDS beside its static arrays; partial last workgroup'),
    Case('proto', 6, 2, 8, 8, 964, 'fp32', 5300, dict(num_protos=18, queue_size=36, knn_k=3, u='mid_bin'), 'first batch of proto_candidates_kernel<8>'),
    Case('proto', 6, 2, 8, 8, 1820, 'fp32', 5400, dict(num_protos=18, queue_size=36, knn_k=3, u='mid_bin'), 'last batch of proto_candidates_kernel<8>'),
    Case('proto', 6, 2, 8, 8, 1821, 'fp32', 5500, dict(num_protos=18, queue_size=36, knn_k=3, u='mid_bin'), 'first batch of proto_candidates_kernel<4>'),
    Case('proto', 6, 2, 8, 8, 3276, 'fp32', 5600, dict(num_protos=18, queue_size=36, knn_k=3, u='mid_bin'), 'last batch of proto_candidates_kernel<4>, the last of the LDS form'),
    Case('proto', 6, 2, 8, 8, 64, 'fp32', 5700, dict(num_protos=16, queue_size=4096, knn_k=3), 'last target count of the LDS knn_select_kernel (64 KB dynamic)'),
    # ---- the in-GEMM bf16 split under the module bars
    Case('rnd', 24, 2, 64, 64, 130, 'bf16x6', 3000, {}, 'bf16x6: three-plane split inside the generic GEMM'),
    Case('rnd', 24, 2, 64, 64, 130, 'bf16x3', 3100, {}, 'bf16x3: hi/lo split inside the generic GEMM'),
    Case('icm_apt', 17, 6, 64, 64, 130, 'bf16x6', 3200, dict(knn_k=12, knn_avg=True, knn_rms=True, knn_clip=0.0), 'bf16x6, LayerNorm trunk in front'),
    Case('icm_apt', 17, 6, 64, 64, 130, 'bf16x3', 3300, dict(knn_k=12, knn_avg=True, knn_rms=True, knn_clip=0.0), 'bf16x3, LayerNorm trunk in front'),
    Case('proto', 12, 2, 36, 130, 130, 'bf16x6', 3403, dict(num_protos=70, queue_size=140, knn_k=3), 'bf16x6, Proto'),
    Case('proto', 12, 2, 36, 130, 130, 'bf16x3', 3501, dict(num_protos=70, queue_size=140, knn_k=3), 'bf16x3, Proto'),
]


def case_id(c):
    o = '-'.join(f'{k}{v}' for k, v in sorted(c.opts.items()))
    return f'{c.kind}-O{c.O}A{c.A}H{c.H}R{c.R}B{c.B}' + (f'-{o}' if o else '') + f'-{c.precision}'


def n_models(c):
    return c.opts.get('n_models') or 5


def shapes(c):
    if c.kind == 'disagreement':
        return [(f'ensemble.{m}.{i}.{w}', s) for m in range(n_models(c))
                for (i, w), s in zip(((0, 'weight'), (0, 'bias'), (2, 'weight'), (2, 'bias')), ((c.H, c.O + c.A), (c.H,), (c.O, c.H), (c.O,)))]
    if c.kind == 'smm':
        return smm_param_shapes(c.O, c.R, c.H)
    if c.kind == 'proto':
        return proto_param_shapes(c.O, c.R, c.H, c.opts['num_protos'])
    return intr_param_shapes(c.kind, c.O, c.A, c.H, c.R)


def params(c):
    return list(_synth.synth_params(shapes(c), c.seed).values())


def batch(c):
    """dict of float32 arrays: obs, action, next_obs, extr, skill (DIAYN / SMM: one-hot; APS: unit task vectors), eps (SMM), u (Proto)."""
    obs, action, reward, _, next_obs = _synth.synth_batch(c.seed + 2, 0, c.B, c.O, c.A)
    b = dict(obs=obs, action=action, next_obs=next_obs, extr=reward.reshape(-1), skill=None)
    rs = np.random.RandomState(c.seed + 3)
    if c.kind in ('diayn', 'smm'):
        b['skill'] = np.eye(c.R, dtype=np.float32)[rs.randint(0, c.R, c.B)]
    if c.kind == 'aps':
        t = rs.standard_normal((c.B, c.R))
        b['skill'] = (t / np.linalg.norm(t, axis=1, keepdims=True)).astype(np.float32)
    if c.kind == 'smm':
        b['eps'] = _synth.NoiseStream(c.seed + 4).draw((c.B, 128))
    if c.kind == 'proto':
        b['u'] = np.random.RandomState(c.seed + 4).uniform(0, 1, c.opts['num_protos']).astype(np.float32)
        if c.opts.get('u') == 'mid_bin':
            b['u'] = _mid_bin_uniforms(c, b)
    return b


_MID_BIN = {}


def _mid_bin_uniforms(c, b):
    if case_id(c) + str(c.seed) not in _MID_BIN:
        tw = make_twin(c, torch.float64)
        res = tw.update({k: v for k, v in b.items() if k != 'u'})
        after = [tw._t(w) for w in tw.adam_first_step(res.grads)]
        cdf = tw.proto_cdf(after, tw._t(b['next_obs']))[2].numpy()
        rs = np.random.RandomState(c.seed + 4)
        u = np.zeros(cdf.shape[0])
        for p, row in enumerate(cdf):
            lo = np.concatenate([[0.0], row[:-1]])
            wide = np.nonzero(row - lo >= 3 * MARGIN * row[-1])[0]
            j = wide[rs.randint(len(wide))]
            u[p] = 0.5 * (lo[j] + row[j]) / row[-1]
        _MID_BIN[case_id(c) + str(c.seed)] = u.astype(np.float32)
    return _MID_BIN[case_id(c) + str(c.seed)]


def twin_kw(c):
    kw = {k: v for k, v in c.opts.items() if k not in ('layout', 'u')}
    if c.kind == 'disagreement':
        kw['n_models'] = n_models(c)
    return kw


def make_twin(c, dtype):
    return IntrTwin(c.kind, params(c), dtype=dtype, **twin_kw(c))


def twin_batch(c):
    return {k: v for k, v in batch(c).items()}


def run_twin(c, dtype, kink_delta=None, params_after=None):
    """(update Result, reward rows, reward metrics, reward decisions, the twin): one step, then the reward under params_after (the twin's
    own first Adam step when None)."""
    tw = make_twin(c, dtype)
    res = tw.update(twin_batch(c), kink_delta=kink_delta, kink_cap=KINK_CAP)
    after = tw.adam_first_step(res.grads) if params_after is None else params_after
    r, m, dec = tw.reward(twin_batch(c), params_after=after)
    return res, r, m, dec, tw


def run_twin_reward_only(c, dtype):
    tw = make_twin(c, dtype)
    r, m, dec = tw.reward(twin_batch(c))
    return r, m, dec, tw


def qualifies(c):
    """None when the case's seed meets the conditions of the table, else what fails."""
    r64, _, _, d64, _ = run_twin(c, torch.float64, KINK_DELTA[c.precision])
    r32, _, _, d32, _ = run_twin(c, torch.float32)
    for a, b in ((r64.decisions, r32.decisions), (d64, d32)):
        for name, (choice, margin) in a.items():
            if not np.array_equal(choice, b[name][0]):
                return f'{name}: twin32 and twin64 decide differently'
            if margin.size and float(margin.min()) < MARGIN:
                return f'{name}: margin {float(margin.min()):.2e} < {MARGIN}'
    if r64.n_kinks['module'] > KINK_CAP:
        return f'|K| = {r64.n_kinks["module"]} > {KINK_CAP}'
    return None
