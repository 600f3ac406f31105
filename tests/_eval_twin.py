"""The forward-only validation pass (agent.evaluate): the cases tests/test_agent_eval_abi.py qualifies on the CPU and
tests/test_gpu_agent_eval.py runs on the GPU, and the twin the two share: plain MLP forwards in float64 or float32 from parameters in the
reference's order (oracle.agents.param_shapes), the six sums of the window formed from them, and the values evaluate() returns.

CASES are rows of tests/_grad_grid.py's table (same seeds, parameters and batch), the five kinds evaluate() supports over the forward
dispatch edges: H in {4, 100, 128, 192, 320, 1024}, B in {1, 7, 50, 64, 72, 1000, 8200}, O + A at 32 / 33 / 36 / 90 / 256, A in {1, 9, 16},
CQL's 2A-wide heads, both bf16x3 routes, plain bf16, and bf16x6 on the three-plane route (tests/_state_bf16x6_cases.py). Nothing is
searched here or on the GPU: the CPU test holds the float32 twin to half of each bar on every case, so the seeds are known to leave room."""
import numpy as np
import torch
import torch.nn.functional as F

import _grad_grid as G
import _state_bf16x6_cases as S
from oracle.twin64 import LN_EPS

KINDS = ('td3_bc', 'td3', 'crr', 'cql', 'bc')
# (kind, H, B, precision) of the rows taken from _grad_grid.CASES
_PICK = [
    ('td3_bc', 100, 7, 'fp32'), ('td3', 4, 1, 'fp32'), ('td3_bc', 32, 50, 'fp32'), ('td3', 1024, 64, 'fp32'), ('td3_bc', 1024, 72, 'fp32'),
    ('td3', 1024, 50, 'fp32'), ('td3_bc', 128, 64, 'fp32'), ('td3', 32, 8200, 'fp32'), ('td3_bc', 320, 1000, 'fp32'),
    ('bc', 100, 7, 'fp32'), ('bc', 192, 1000, 'fp32'), ('crr', 100, 50, 'fp32'), ('crr-exp', 64, 72, 'fp32'),
    ('cql', 32, 7, 'fp32'), ('cql', 128, 72, 'fp32'), ('cql-lagrange', 64, 50, 'fp32'),
    ('td3_bc', 128, 64, 'bf16x3'), ('bc', 128, 64, 'bf16x3'), ('crr', 128, 64, 'bf16x3'), ('cql', 128, 64, 'bf16x3'),       # planes pipeline
    ('td3_bc', 100, 7, 'bf16x3'), ('td3', 192, 72, 'bf16x3'), ('cql', 100, 50, 'bf16x3'), ('crr-exp', 64, 50, 'bf16x3'),    # in-GEMM split
    ('td3_bc', 256, 1024, 'bf16'), ('td3', 192, 1000, 'bf16'), ('bc', 128, 1024, 'bf16'), ('cql', 128, 256, 'bf16'),
]
CASES = [next(c for c in G.CASES if (c.kind, c.H, c.B, c.precision) == k) for k in _PICK]
# bf16x6: the three-plane route (128 | H, 128 | B) for a twin-critic kind, BC and CQL, and the in-GEMM split at a shape that does not tile
CASES += [c for c in S.NEW_PLANE_CASES if c.B == 128] + [c for c in S.GENERIC_CASES if (c.kind, c.H) == ('td3_bc', 100)]

# the project's metric bars (tests/test_gpu_grad_grid.py, tests/test_gpu_state_bf16x6.py): |got - v| <= REL |v| + ABS
BARS = {'fp32': (2e-5, 1e-6), 'bf16x6': (2e-5, 1e-6), 'bf16x3': (1e-4, 1e-6), 'bf16': (3e-2, 3e-2)}
VALUE_KEYS = ('val_bc_mse', 'val_q_data', 'val_q_pi', 'val_critic_loss', 'val_critic_target_q')
SUM_SLOTS = ('bc_sq', 'q_data', 'q_pi', 'q1_err', 'q2_err', 'target_q')       # the window's slots, in EXORL_E_* order


def bar(precision, v):
    rel, ab = BARS[precision]
    return rel * abs(v) + ab


def mlp(p, x):
    """[Linear LayerNorm Tanh] [Linear ReLU Linear] from the 8 tensors W0 b0 gain beta W1 b1 W2 b2."""
    h = torch.tanh(F.layer_norm(F.linear(x, p[0], p[1]), (p[0].shape[0],), p[2], p[3], LN_EPS))
    return F.linear(torch.relu(F.linear(h, p[4], p[5])), p[6], p[7])


def twin_sums(c, dtype, batch=None, actor=None, critic=None, target=None):
    """The six sums over the rows of `batch` (default: the case's), as float64 numbers computed in `dtype`; parameters default to the
    case's seeded ones, the target to the critic (a fresh agent's). BC has the first only."""
    pa, pc, _, _ = G.params(c)
    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=dtype)
    actor = [t(w) for w in (actor if actor is not None else pa)]
    obs, action, reward, discount, next_obs = (t(x) for x in (batch if batch is not None else G.batch(c)))
    A = c.A
    mu = lambda o: torch.tanh(mlp(actor, o)[:, :A])          # CQL: the first A of its 2A outputs
    out = {'bc_sq': float(((mu(obs) - action) ** 2).sum().double())}
    if G.base_kind(c) == 'bc':
        return out
    critic = [t(w) for w in (critic if critic is not None else pc)]
    target = [t(w) for w in target] if target is not None else critic
    q = lambda p, o, a: tuple(mlp(p[8 * i:8 * i + 8], torch.cat([o, a], -1)) for i in range(2))
    q1, q2 = q(critic, obs, action)
    p1, p2 = q(critic, obs, mu(obs))
    t1, t2 = q(target, next_obs, mu(next_obs))
    y = reward + discount * torch.min(t1, t2)
    for k, v in (('q_data', torch.min(q1, q2)), ('q_pi', torch.min(p1, p2)), ('q1_err', (q1 - y) ** 2), ('q2_err', (q2 - y) ** 2), ('target_q', y)):
        out[k] = float(v.sum().double())
    return out


def values_of(sums, rows, A):
    """evaluate()'s dict from the twin's sums (the definitions of agents.eval_values, restated)."""
    out = {'val_bc_mse': sums['bc_sq'] / (rows * A)}
    if 'q_data' in sums:
        out.update(val_q_data=sums['q_data'] / rows, val_q_pi=sums['q_pi'] / rows, val_critic_loss=(sums['q1_err'] + sums['q2_err']) / rows,
                   val_critic_target_q=sums['target_q'] / rows)
        out['val_q_gap'] = out['val_q_pi'] - out['val_q_data']
    out['val_rows'] = rows
    return out


def twin_values(c, dtype, **kw):
    return values_of(twin_sums(c, dtype, **kw), c.B, c.A)
