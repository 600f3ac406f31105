"""IQL's gradient cases: what tests/test_iql_twin.py qualifies on the CPU and tests/test_gpu_iql.py runs on the GPU, built like
tests/_grad_grid.py (whose kink treatment, error measures and constants are used as they are).

One case = one update() of IQLAgent from seeded parameters and batch. Columns of CASES:
  O A H B      observation width, action width, hidden width, batch
  precision    fp32 | bf16x3 | bf16x6 | bf16
  seed         actor / critic / value parameters synth_params(seed) / (seed + 1) / (seed + 4), batch synth_batch(seed + 2, 0). Searched once on
               the CPU (smallest seed >= the case's base for which qualify() holds); the tests do not search
  bar          'tight' | 'coarse', as in _grad_grid
  hyper        (expectile, temperature, max_weight)
  clamp        the case must have at least one row clamped at max_weight and at least one not
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np
import torch

import _synth
from _grad_grid import KINK_CAP, KINK_DELTA, MARGIN
from _iql_twin import IQLTwin
from oracle.agents import param_shapes

Case = namedtuple('Case', 'O A H B precision seed bar hyper clamp why')
DEFAULT = (0.7, 3.0, 100.0)
KINK_DELTA = dict(KINK_DELTA, bf16x6=KINK_DELTA['fp32'])       # bf16x6 is fp32-grade: fp32's delta and fp32's bar

CASES = [
    Case(5, 1, 100, 7, 'fp32', 101, 'tight', DEFAULT, False, 'A=1, H=100 (multiple of 4 only), B=7'),
    Case(24, 6, 128, 64, 'fp32', 200, 'tight', DEFAULT, False, 'the shape of the other agents\' gradient tests'),
    Case(240, 16, 128, 64, 'fp32', 300, 'tight', DEFAULT, False, 'O+A=256: the supported limit'),
    Case(78, 12, 64, 1000, 'fp32', 400, 'tight', DEFAULT, False, 'B=1000: every row-chunked kernel masks its last chunk; four chunks of the row kernel'),
    Case(6, 2, 32, 8200, 'fp32', 500, 'tight', DEFAULT, False, 'rows >= 8192 with a ragged tail: the row kernel\'s workgroups take a second chunk'),
    Case(24, 6, 64, 72, 'fp32', 600, 'tight', (0.9, 10.0, 100.0), True, 'clamp: weights on both sides of max_weight'),
    Case(24, 6, 128, 64, 'bf16x3', 700, 'tight', DEFAULT, False, 'planes pipeline'),
    Case(11, 3, 64, 50, 'bf16x3', 800, 'tight', DEFAULT, False, 'in-GEMM split'),
    Case(24, 6, 128, 128, 'bf16x6', 900, 'tight', DEFAULT, False, 'three-plane route (128 | H, 128 | B)'),
    Case(24, 6, 256, 1024, 'bf16', 1000, 'coarse', DEFAULT, False, 'plain bf16: direction only'),
]
VALUE_KEYS = [f'net.{i}.{w}' for i in (0, 1, 3, 5) for w in ('weight', 'bias')]


def case_id(c):
    return f'iql-O{c.O}A{c.A}H{c.H}B{c.B}-{c.precision}' + ('-clamp' if c.clamp else '')


def value_shapes(O, H):
    return list(zip(VALUE_KEYS, [(H, O), (H,), (H,), (H,), (H, H), (H,), (1, H), (1,)]))


def params(c):
    """(actor, critic, value) dicts key -> float32 array, in parameters() order."""
    ash, csh = param_shapes('td3_bc', c.O, c.A, c.H)
    return _synth.synth_params(ash, c.seed), _synth.synth_params(csh, c.seed + 1), _synth.synth_params(value_shapes(c.O, c.H), c.seed + 4)


def batch(c):
    return _synth.synth_batch(c.seed + 2, 0, c.B, c.O, c.A)


def make_twin(c, dtype, stddev=0.2, **kw):
    pa, pc, pv = params(c)
    e, t, mw = c.hyper
    return IQLTwin(list(pa.values()), list(pc.values()), list(pv.values()), dtype=dtype, stddev=stddev,
                   **dict(dict(expectile=e, temperature=t, max_weight=mw), **kw))


def run_twin(c, dtype, kink_delta=None):
    return make_twin(c, dtype).update(batch(c), kink_delta=kink_delta, kink_cap=KINK_CAP)


@lru_cache(maxsize=4)
def twin_pair(c):
    """(twin64 result with the near-kink directions at the case's delta — none for a coarse case —, twin32 result)."""
    return run_twin(c, torch.float64, None if c.bar == 'coarse' else KINK_DELTA[c.precision]), run_twin(c, torch.float32)


STEPS = ('value', 'critic', 'actor')


def steps_of(res):
    return [(s, getattr(res, f'{s}_grads')) for s in STEPS]


def qualify(c):
    """The list of reasons the case does not qualify (empty: it does): the float32 and float64 twins take the same discrete decisions, every
    decision has a float64 margin >= MARGIN, both signs of u occur, a clamp case has rows on both sides of max_weight, and (tight cases) the
    near-kink set of every step is within KINK_CAP and the two twins' ReLU masks agree outside it."""
    r64, r32 = twin_pair(c)
    bad = []
    for name, (choice, margin) in r64.decisions.items():
        if not np.array_equal(choice, r32.decisions[name][0]):
            bad.append(f'{name}: twin32 decides differently')
        if float(margin.min()) < MARGIN:
            bad.append(f'{name}: margin {float(margin.min()):.2e}')
    neg = r64.decisions['u_negative'][0]
    if not (neg.any() and (1 - neg).any()):
        bad.append('u has one sign only')
    cl = r64.decisions['weight_clamped'][0]
    if c.clamp and not (cl.any() and (1 - cl).any()):
        bad.append(f'clamp case with {int(cl.sum())} of {cl.size} rows clamped')
    if c.bar == 'tight':
        for step in STEPS:
            if r64.kinks[step] is None:
                bad.append(f'{step}: |K| = {r64.n_kinks[step]} > {KINK_CAP}')
                continue
            for a, b in zip(r64.relus[step], r32.relus[step]):
                z = a['z']
                far = z.abs() >= KINK_DELTA[c.precision] * z.abs().max()
                if bool((((z > 0) != (b['z'] > 0)) & far).any()):
                    bad.append(f'{step}/{a["name"]}: ReLU masks differ outside the near-kink set')
    return bad


# ---- the five-step trajectory of tests/test_gpu_iql.py (batches synth_batch(seed + 2, step)); its seed qualifies in tests/test_iql_twin.py
TRAJ = Case(5, 2, 32, 8, 'fp32', 40, 'tight', DEFAULT, False, 'five steps')


def traj_bar(p64, step):
    """Per step an Adam update moves a parameter by lr m^ / (sqrt(v^) + eps): a relative error of 1e-3 in that ratio (gradients within the fp32
    bar, far from zero) is 1e-3 lr; storing the parameter rounds it once, 2^-24 max|p|. Both add up over the steps."""
    return (step + 1) * (2.0 ** -23 * max(float(np.abs(p64).max()), 1.0) + 1e-3 * 1e-4)


# ---- the agent under test, for the GPU tests and their child processes
def make_agent(c, use_tb=True, **kw):
    """IQLAgent of the case's shape, precision and hyper-parameters on the GPU (kw overrides constructor keywords)."""
    from exorl_amd import agents
    e, t, mw = c.hyper
    args = dict(expectile=e, temperature=t, max_weight=mw, precision=c.precision)
    args.update(kw)
    return agents.IQLAgent('iql', (c.O,), (c.A,), 'cuda', 1e-4, c.H, 0.01, 0.2, 1, c.B, use_tb, **args)


def load_params(ag, c):
    """The case's seeded parameters into the agent's four nets."""
    pa, pc, pv = params(c)
    for net, p in ((ag.actor, pa), (ag.critic, pc), (ag.value, pv)):
        net.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
    ag.critic_target.load_state_dict(ag.critic.state_dict())
    return ag
