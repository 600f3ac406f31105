"""FQE's gradient cases: what tests/test_fqe_twin.py qualifies on the CPU and tests/test_gpu_fqe.py runs on the GPU, built like
tests/_iql_cases.py (tests/_grad_grid.py's kink treatment, error measures and constants are used as they are).

One case = one update() of FQEAgent from seeded parameters and batch. Columns of CASES:
  O A H B      observation width, action width, hidden width, batch
  precision    fp32 | bf16x3 | bf16x6 | bf16
  seed         actor / critic parameters synth_params(seed) / (seed + 1), batch synth_batch(seed + 2, 0). Searched once on the CPU (smallest
               seed >= the case's base for which qualify() holds); the tests do not search
  bar          'tight' | 'coarse', as in _grad_grid
The step has no min, no clamp and no sign test: its only discrete decisions are the critic's ReLU masks.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np
import torch

import _synth
from _fqe_twin import FQETwin
from _grad_grid import KINK_CAP, KINK_DELTA, MARGIN
from oracle.agents import param_shapes

Case = namedtuple('Case', 'O A H B precision seed bar why')
KINK_DELTA = dict(KINK_DELTA, bf16x6=KINK_DELTA['fp32'])       # bf16x6 is fp32-grade: fp32's delta and fp32's bar

CASES = [
    Case(5, 1, 100, 7, 'fp32', 101, 'tight', 'A=1, H=100 (multiple of 4 only), B=7'),
    Case(24, 6, 128, 64, 'fp32', 200, 'tight', 'the shape of the other agents\' gradient tests'),
    Case(240, 16, 128, 64, 'fp32', 300, 'tight', 'O+A=256: the supported limit'),
    Case(78, 12, 64, 1000, 'fp32', 400, 'tight', 'B=1000: every row-chunked kernel masks its last chunk; four chunks of the row kernel'),
    Case(6, 2, 32, 8200, 'fp32', 500, 'tight', 'rows >= 8192 with a ragged tail: the row kernel\'s workgroups take a second chunk'),
    Case(24, 6, 128, 64, 'bf16x3', 700, 'tight', 'planes pipeline'),
    Case(11, 3, 64, 50, 'bf16x3', 800, 'tight', 'in-GEMM split'),
    Case(24, 6, 128, 128, 'bf16x6', 900, 'tight', 'three-plane route (128 | H, 128 | B)'),
    Case(24, 6, 256, 1024, 'bf16', 1000, 'coarse', 'plain bf16: direction only'),
]


def case_id(c):
    return f'fqe-O{c.O}A{c.A}H{c.H}B{c.B}-{c.precision}'


def params(c):
    """(actor, critic) dicts key -> float32 array, in parameters() order."""
    ash, csh = param_shapes('td3_bc', c.O, c.A, c.H)
    return _synth.synth_params(ash, c.seed), _synth.synth_params(csh, c.seed + 1)


def batch(c, step=0):
    return _synth.synth_batch(c.seed + 2, step, c.B, c.O, c.A)


def make_twin(c, dtype):
    pa, pc = params(c)
    return FQETwin(list(pa.values()), list(pc.values()), dtype=dtype)


def run_twin(c, dtype, kink_delta=None):
    return make_twin(c, dtype).update(batch(c), kink_delta=kink_delta, kink_cap=KINK_CAP)


@lru_cache(maxsize=4)
def twin_pair(c):
    """(twin64 result with the near-kink directions at the case's delta — none for a coarse case —, twin32 result)."""
    return run_twin(c, torch.float64, None if c.bar == 'coarse' else KINK_DELTA[c.precision]), run_twin(c, torch.float32)


def qualify(c):
    """The list of reasons the case does not qualify (empty: it does): there is no discrete decision besides the ReLU masks (any the twin
    reports must agree between float32 and float64 with a margin >= MARGIN), and (tight cases) the near-kink set is within KINK_CAP and the
    two twins' ReLU masks agree outside it."""
    r64, r32 = twin_pair(c)
    bad = []
    for name, (choice, margin) in r64.decisions.items():
        if not np.array_equal(choice, r32.decisions[name][0]):
            bad.append(f'{name}: twin32 decides differently')
        if float(margin.min()) < MARGIN:
            bad.append(f'{name}: margin {float(margin.min()):.2e}')
    if c.bar == 'tight':
        if r64.kinks['critic'] is None:
            bad.append(f'critic: |K| = {r64.n_kinks["critic"]} > {KINK_CAP}')
        else:
            for a, b in zip(r64.relus['critic'], r32.relus['critic']):
                z = a['z']
                far = z.abs() >= KINK_DELTA[c.precision] * z.abs().max()
                if bool((((z > 0) != (b['z'] > 0)) & far).any()):
                    bad.append(f'critic/{a["name"]}: ReLU masks differ outside the near-kink set')
    return bad


# ---- the five-step trajectory of tests/test_gpu_fqe.py (batches synth_batch(seed + 2, step)); its seed qualifies in tests/test_fqe_twin.py
TRAJ = Case(5, 2, 32, 8, 'fp32', 40, 'tight', 'five steps')


# ---- the agent under test, for the GPU tests and their child processes
def make_agent(c, use_tb=True, **kw):
    """FQEAgent of the case's shape and precision on the GPU (kw overrides constructor keywords)."""
    from exorl_amd import agents
    args = dict(precision=c.precision)
    args.update(kw)
    return agents.FQEAgent('fqe', (c.O,), (c.A,), 'cuda', 1e-4, c.H, 0.01, 1, c.B, use_tb, **args)


def load_params(ag, c):
    """The case's seeded parameters into the agent's nets."""
    pa, pc = params(c)
    for net, p in ((ag.actor, pa), (ag.critic, pc)):
        net.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
    ag.critic_target.load_state_dict(ag.critic.state_dict())
    return ag
