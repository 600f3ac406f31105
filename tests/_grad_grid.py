"""The gradient grid: the cases tests/test_twin64.py qualifies on the CPU and tests/test_gpu_grad_grid.py runs on the GPU, and the
arithmetic the two share (inputs from seeds, the float64 / float32 twins, the treatment of ReLU kinks, the per-tensor error).

One case = one update() of a state agent from seeded parameters, batch and noise. Columns of CASES:
  kind       td3_bc | td3 | ddpg | bc | crr | crr-exp | crr-identity | cql | cql-lagrange
  O A H B    observation width, action width, hidden width, batch
  n          CRR's num_value_samples / CQL's n_samples (ignored by the others)
  precision  fp32 | bf16x3 | bf16
  seed       parameters synth_params(seed) / (seed + 1), batch synth_batch(seed + 2, 0), noise NoiseStream(seed + 3). Searched once on
             the CPU (smallest seed >= the case's round base for which the float32 and float64 twins take identical discrete
             decisions, every decision has a float64 margin >= 1e-4, the near-kink sets are within the cap and, for plain bf16, the
             bf16-operand twin keeps BF16_FLOOR); the tests do not search
  bar        'tight': per-tensor max-norm bar against twin64 after the kink treatment; 'coarse': per-tensor cosine / norm ratio
             (plain bf16, and bf16x3 cases whose near-kink set exceeds KINK_CAP)
What each case is there for is in its `why`.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np
import torch

import _synth
from oracle.agents import param_shapes, uniform_from_normal
from oracle.twin64 import Twin

Case = namedtuple('Case', 'kind O A H B n precision seed bar why')

KINK_CAP = 64
KINK_DELTA = {'fp32': 2.0 ** -18, 'bf16x3': 2.0 ** -14, 'bf16': 2.0 ** -14}
MARGIN = 1e-4
BF16_FLOOR = 0.9995          # cosine the bf16-operand twin has to keep on every tensor of a plain-bf16 case (half the bar's 1 - 0.999)
KINK_FLOOR = {'fp32': 2.0 ** -22, 'bf16x3': 2.0 ** -16}      # see explain_kinks

CASES = [
    # ---- fp32 mode: dispatch edges
    Case('td3_bc', 5, 1, 100, 7, 0, 'fp32', 100, 'tight', 'A=1: head_bwd<1> with the actor loss gradient, no fused sampling; H=100 (multiple of 4 only); B=7; O+A=6'),
    Case('td3', 4, 2, 4, 1, 0, 'fp32', 200, 'tight', 'H=4 and B=1: the smallest supported net; A=2'),
    Case('td3_bc', 24, 8, 32, 50, 0, 'fp32', 300, 'tight', 'A=8: last width of head_bwd<8>; O+A=32 fills the bf16 K padding exactly; B=50'),
    Case('ddpg', 24, 9, 192, 72, 0, 'fp32', 400, 'tight', 'A=9: head_bwd<16> for a TD3-family actor; O+A=33 crosses the 32-column padding; H=192 (64 | H, 128 does not); B=72; shared trunk'),
    Case('td3', 19, 16, 1024, 64, 0, 'fp32', 501, 'tight', 'A=16: last width of head_bwd<16>; O+A=35 at H=1024: last first layer trunk_fwd stages in one pass'),
    Case('td3_bc', 30, 6, 1024, 72, 0, 'fp32', 600, 'tight', 'O+A=36 at H=1024: first first layer past the W0T staging limit of trunk_fwd'),
    Case('td3', 78, 12, 1024, 50, 0, 'fp32', 700, 'tight', 'O+A=90 at H=1024: three staging passes of trunk_fwd outside CQL; B=50'),
    Case('td3_bc', 240, 16, 128, 64, 0, 'fp32', 800, 'tight', 'O+A=256: the supported limit'),
    Case('td3', 6, 2, 32, 8200, 0, 'fp32', 952, 'tight', 'rows >= 8192 with a ragged tail: 4 passes per workgroup in ln_bwd / outer_reduce, last workgroup has sub-blocks wholly past the end'),
    Case('td3_bc', 24, 6, 320, 1000, 0, 'fp32', 1002, 'tight', 'H=320 (64 | H, 128 does not); B=1000 (not a multiple of 16 or 32: every row-chunked kernel masks its last chunk)'),
    Case('ddpg', 24, 6, 384, 1024, 0, 'fp32', 1105, 'tight', 'H=384 (3 x 128); B=1024'),
    Case('bc', 24, 6, 100, 7, 0, 'fp32', 1200, 'tight', 'BC: the only forward of the step at B=7, H=100'),
    Case('bc', 11, 3, 192, 1000, 0, 'fp32', 1300, 'tight', 'BC at B=1000, H=192'),
    Case('crr', 11, 3, 100, 50, 7, 'fp32', 1400, 'tight', 'CRR indicator, num_value_samples=7 divides no chunk size'),
    Case('crr-exp', 24, 6, 64, 72, 10, 'fp32', 1500, 'tight', 'CRR exp weights, num_value_samples=10, B=72'),
    Case('crr-identity', 5, 1, 32, 7, 3, 'fp32', 1600, 'tight', 'CRR identity weights with A=1: head_bwd<1> with the weighted log-likelihood gradient'),
    Case('cql', 5, 3, 32, 7, 3, 'fp32', 1700, 'tight', 'CQL A=3: 2A=6 outputs, head_bwd<8> with the tanh-Gaussian gradient; B=7'),
    Case('cql', 24, 5, 100, 50, 3, 'fp32', 1800, 'tight', 'CQL A=5: 2A=10 outputs, head_bwd<16>; H=100; B=50'),
    Case('cql', 24, 8, 192, 64, 2, 'fp32', 1900, 'tight', 'CQL A=8: 2A=16, last width of head_bwd<16>; O+A=32; n_samples=2'),
    Case('cql', 24, 9, 128, 72, 3, 'fp32', 2000, 'tight', 'CQL A=9: 2A=18, first width of head_bwd_wide; O+A=33'),
    Case('cql-lagrange', 17, 16, 64, 50, 3, 'fp32', 2100, 'tight', 'CQL A=16: 2A=32, widest head_bwd_wide; Lagrange weight on the penalty'),
    Case('cql', 78, 12, 64, 1000, 3, 'fp32', 2201, 'tight', 'CQL B=1000, n=3: 10000 critic rows, rows >= 8192 with a ragged tail; O+A=90'),
    Case('cql', 78, 12, 64, 1024, 3, 'fp32', 2300, 'tight', 'CQL B=1024, n=3: 10240 critic rows, the even control of the case above'),
    # ---- bf16x3 on the hi/lo-plane pipeline (planes_ok: 128 | H, 64 | B)
    Case('td3_bc', 24, 6, 128, 64, 0, 'bf16x3', 3000, 'tight', 'planes pipeline at the shape of test_gradients_vs_oracle_td3_bc'),
    Case('td3', 17, 6, 128, 128, 0, 'bf16x3', 3101, 'tight', 'planes pipeline, B.H = 16384'),
    Case('ddpg', 24, 9, 256, 64, 0, 'bf16x3', 3202, 'tight', 'planes pipeline, shared trunk, A=9, O+A=33 crosses the K padding of the bf16 first layer'),
    Case('bc', 24, 6, 128, 64, 0, 'bf16x3', 3300, 'tight', 'planes pipeline, BC'),
    Case('crr', 24, 6, 128, 64, 7, 'bf16x3', 3400, 'tight', 'planes pipeline, CRR with 7 value samples (448 rows)'),
    Case('cql', 24, 6, 128, 64, 3, 'bf16x3', 3500, 'tight', 'planes pipeline, CQL: 640 critic rows'),
    Case('td3_bc', 24, 6, 384, 1024, 0, 'bf16x3', 3610, 'coarse', 'planes pipeline at H=384, B=1024: near-kink set above the cap'),
    Case('cql', 78, 12, 128, 1024, 3, 'bf16x3', 3701, 'coarse', 'planes pipeline, 10240 critic rows (4 passes per workgroup on bf16 planes)'),
    # ---- bf16x3 with the operands split inside the GEMM (planes_ok does not hold)
    Case('td3_bc', 5, 1, 100, 7, 0, 'bf16x3', 4000, 'tight', 'in-GEMM split: H=100, B=7, A=1'),
    Case('td3', 24, 8, 192, 72, 0, 'bf16x3', 4100, 'tight', 'in-GEMM split: H=192 is a multiple of 64 but not of 128; O+A=32'),
    Case('cql', 24, 5, 100, 50, 3, 'bf16x3', 4200, 'tight', 'in-GEMM split, CQL A=5'),
    Case('crr-exp', 11, 3, 64, 50, 7, 'bf16x3', 4300, 'tight', 'in-GEMM split: H=64 tiles by 64 but trunk_fwd16 needs 128'),
    Case('td3_bc', 24, 6, 320, 1000, 0, 'bf16x3', 4403, 'coarse', 'in-GEMM split at H=320, B=1000: near-kink set above the cap'),
    Case('cql', 78, 12, 64, 1000, 3, 'bf16x3', 4500, 'coarse', 'in-GEMM split, 10000 critic rows with a ragged tail'),
    # ---- plain bf16 (8 | H, 8 | B): direction only. Sizes at which the format itself leaves room under the bar: with bf16-rounded operands
    # in the twin (Twin(bf16_operands=True)) every tensor keeps cosine >= BF16_FLOOR against twin64 (tests/test_twin64.py). At small batches
    # it does not (TD3+BC, H=128, B=64: 0.9986 on the actor's first layer; CRR's actor step: 0.9978 to 0.9994 from B=8 to B=1024, which is
    # why CRR has no plain-bf16 case): bf16 forward error flips about 1 % of the ReLU derivatives, each a whole row's share of a gradient
    Case('td3_bc', 24, 6, 256, 1024, 0, 'bf16', 5004, 'coarse', 'plain bf16 on the MFMA trunk (128 | H), B=1024'),
    Case('td3', 17, 6, 192, 1000, 0, 'bf16', 5110, 'coarse', 'plain bf16, H=192: trunk_fwd writes the bf16 activations; B=1000 (multiple of 8 only)'),
    Case('ddpg', 24, 6, 384, 1024, 0, 'bf16', 5225, 'coarse', 'plain bf16, shared trunk, H=384'),
    Case('bc', 24, 6, 128, 1024, 0, 'bf16', 5300, 'coarse', 'plain bf16, BC'),
    Case('cql', 24, 6, 128, 256, 3, 'bf16', 5408, 'coarse', 'plain bf16, CQL: 2560 critic rows'),
]


def case_id(c):
    return f'{c.kind}-O{c.O}A{c.A}H{c.H}B{c.B}' + (f'n{c.n}' if c.n else '') + f'-{c.precision}'


def base_kind(c):
    return 'crr' if c.kind.startswith('crr') else 'cql' if c.kind.startswith('cql') else c.kind


def params(c):
    """(actor arrays, critic arrays or None, actor dict, critic dict or None) in the reference's parameter order."""
    ash, csh = param_shapes(base_kind(c), c.O, c.A, c.H)
    pa = _synth.synth_params(ash, c.seed)
    pc = _synth.synth_params(csh, c.seed + 1) if csh else None
    return list(pa.values()), (list(pc.values()) if pc else None), pa, pc


def batch(c):
    return _synth.synth_batch(c.seed + 2, 0, c.B, c.O, c.A)


def noise(c):
    """The noise blocks of the step in the reference's draw order (standard normal; CQL's second block becomes U(-1,1))."""
    ns = _synth.NoiseStream(c.seed + 3)
    k, B, A = base_kind(c), c.B, c.A
    if k == 'bc':
        return []
    if k == 'crr':
        return [ns.draw((B, A)), ns.draw((B * c.n, A))]
    if k == 'cql':
        return [ns.draw((B, A)), uniform_from_normal(ns.draw((c.n, B, A))), ns.draw((c.n, B, A)), ns.draw((c.n, B, A)), ns.draw((B, A))]
    return [ns.draw((B, A)), ns.draw((B, A))]


def make_twin(c, dtype, bf16_operands=False):
    pa, pc, _, _ = params(c)
    return Twin(base_kind(c), pa, pc, dtype=dtype, bf16_operands=bf16_operands, num_value_samples=c.n or 10, weight_func=c.kind.partition('-')[2] or 'indicator',
                n_samples=c.n or 3, use_critic_lagrange=c.kind == 'cql-lagrange')


def run_twin(c, dtype, kink_delta=None, critic_after=None, bf16_operands=False):
    return make_twin(c, dtype, bf16_operands).update(batch(c), 0, *noise(c), rand_is_uniform=True, kink_delta=kink_delta, kink_cap=KINK_CAP,
                                      critic_after=critic_after)


@lru_cache(maxsize=4)
def twin_pair(c):
    """(twin64 result with the near-kink directions at the case's delta, twin32 result)."""
    return run_twin(c, torch.float64, KINK_DELTA[c.precision]), run_twin(c, torch.float32)


def steps_of(res):
    """[(step name, gradient list)] of the nets the step differentiates."""
    return [(s, g) for s, g in (('critic', res.critic_grads), ('actor', res.actor_grads)) if g is not None]


# ---- ReLU kinks -----------------------------------------------------------------------------------------------------------------
# The backward pass is linear in the ReLU masks: flipping the derivative of one element k changes the step's gradient by exactly D_k
# (Twin._step). An element whose pre-activation is within rounding of 0 may be on in one arithmetic and off in another; only the
# elements twin64 itself puts within delta * max|z| of the kink (K) may be explained that way, each by a fitted flip state s_k that has
# to come out as 0 or 1.
def explain_kinks(got, want, kinks, floor, tag=''):
    """got, want: the gradient tensors of one step (lists of arrays, same shapes); kinks: Result.kinks of that step. Returns
    (got - want with the accepted flips taken out, number of flips accepted). Raises AssertionError when a fitted flip state is not
    within 0.05 of 0 or 1.

    The flip states are the least-squares solution of  got - want = sum_k s_k D_k  over the WHOLE gradient vector of the step, every
    tensor divided by its max|want| so that the rounding noise of all of them weighs alike. Reading s_k off the one bias entry
    D_k[b1, unit] = +- d loss / d relu_k alone uses a single number whose signal is one row's share of that bias gradient: over 10000
    critic rows (CQL, B = 1000) the float32 noise of the entry is 0.13 of it (measured), while W1's row of that unit, and every trunk
    tensor below it, carry the same flip over hundreds of entries."""
    diff = [np.asarray(g, np.float64).reshape(w.shape) - w for g, w in zip(got, want)]
    if not kinks:
        return diff, 0
    scale = [max(float(np.abs(w).max()), 1e-300) for w in want]
    # only flips that matter are fitted: one that moves no tensor by `floor` of its largest element stays in the difference and counts
    # against the bar like any other error (floor = a quarter of the smallest bar the caller applies: 8 * 2^-23 in fp32 mode,
    # 4 * 2^-16 for bf16x3). Below that the fit has nothing to hold on to: the flip is smaller than the arithmetic's own rounding
    vis = [k for k in kinks if max(float(np.abs(d).max()) / s for d, s in zip(k['D'], scale) if d is not None) >= floor]
    if not vis:
        return diff, 0
    gram, rhs = np.zeros((len(vis), len(vis))), np.zeros(len(vis))
    for t, (d, sc) in enumerate(zip(diff, scale)):
        M = np.stack([(np.zeros(d.size) if k['D'][t] is None else k['D'][t].reshape(-1)) / sc for k in vis], 1)
        gram += M.T @ M
        rhs += M.T @ (d.reshape(-1) / sc)
    s = np.linalg.lstsq(gram, rhs, rcond=None)[0]
    flips = 0
    for k, sk in zip(vis, s):
        r = round(float(sk))
        assert r in (0, 1) and abs(sk - r) <= 0.05, (f'{tag}: flip state {sk:.4f} of {k["name"]}[{k["row"]},{k["unit"]}] (z = {k["z"]:.3e}) '
                                                     f'is neither 0 nor 1')
        if r:
            flips += 1
            for t, d in enumerate(k['D']):
                if d is not None:
                    diff[t] -= d.reshape(diff[t].shape)
    return diff, flips


def tensor_cosines(got, want):
    """cosine per tensor (1.0 for a tensor both sides leave at exactly 0)."""
    out = []
    for g, w in zip(got, want):
        g, w = np.asarray(g, np.float64).reshape(-1), w.reshape(-1)
        n = np.linalg.norm(g) * np.linalg.norm(w)
        out.append(float(g @ w / n) if n > 0 else (1.0 if not np.any(g) and not np.any(w) else 0.0))
    return out


def tensor_errors(diff, want):
    """e per tensor: max|diff| / max|want| (a tensor the reference leaves at exactly 0 must be exactly 0: inf otherwise)."""
    out = []
    for d, w in zip(diff, want):
        m = float(np.abs(w).max())
        out.append(float(np.abs(d).max()) / m if m > 0 else (0.0 if not np.any(d) else float('inf')))
    return out
