"""PRDC's gradient cases: what tests/test_prdc_twin.py qualifies on the CPU and tests/test_gpu_prdc.py runs on the GPU, built like
tests/_iql_cases.py on tests/_grad_grid.py (whose kink treatment, error measures and constants are used as they are).

One case = one update() of PRDCAgent from seeded parameters, batch, noise and table. Columns of CASES:
  O A H B      observation width, action width, hidden width, batch
  precision    fp32 | bf16x3 | bf16x6 | bf16
  N            transitions of the one episode the table is built from (key_every = 1: N table rows)
  seed         actor / critic parameters synth_params(seed) / (seed + 1), batch synth_batch(seed + 2, 0), noise NoiseStream(seed + 3), the
               episode synth_episodes(seed + 5, [N]). Searched once on the CPU (smallest seed >= the case's base for which qualify()
               holds); the tests do not search
  bar          'tight' | 'coarse', as in _grad_grid
  rows         'random': the batch's observations are synth_batch's, independent of the table: the neighbour is a matter of the whole key.
               'table': batch row b is the table's transition b (observation and action; B <= N), what a sampled batch is in training. The
               nearest key is then the row itself at d2 = |mu - a|^2 of a few tenths, the runner-up a different state at about
               2 beta^2 O: the gap is 0.86 at the least (BF16_GAP asks for 0.5) and survives plain bf16's 3e-2 error in mu, which a random batch's gaps (a few per cent at
               best, some row of 1024 always below 1e-3) do not
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np
import torch

import _synth
from _grad_grid import KINK_CAP, KINK_DELTA, MARGIN
from _prdc_twin import PRDCTwin
from oracle.agents import param_shapes

Case = namedtuple('Case', 'O A H B precision N seed bar rows why')
BETA = 2.0
KINK_DELTA = dict(KINK_DELTA, bf16x6=KINK_DELTA['fp32'])       # bf16x6 is fp32-grade: fp32's delta and fp32's bar
BF16_GAP = 0.5                                                 # what the plain-bf16 case's smallest gap has to exceed

CASES = [
    Case(5, 1, 100, 7, 'fp32', 63, 100, 'tight', 'random', 'A=1, H=100 (multiple of 4 only), B=7; D=6 (pitch 8); 63 keys: one ragged key tile'),
    Case(24, 6, 128, 64, 'fp32', 1000, 201, 'tight', 'random', 'the shape of the other agents\' gradient tests; D=30 (pitch 32)'),
    Case(240, 16, 128, 64, 'fp32', 65, 302, 'tight', 'random', 'O+A=256: the supported limit, eight column chunks; 65 keys: a second tile of one key'),
    Case(27, 6, 64, 1000, 'fp32', 5000, 400, 'tight', 'random', 'D=33: pitch 36, a second column chunk that is all pad but one; B=1000: a ragged query tile'),
    Case(24, 6, 128, 64, 'bf16x3', 1000, 700, 'tight', 'random', 'planes pipeline'),
    Case(11, 3, 64, 50, 'bf16x3', 300, 800, 'tight', 'random', 'in-GEMM split'),
    Case(24, 6, 128, 128, 'bf16x6', 1000, 900, 'tight', 'random', 'three-plane route (128 | H, 128 | B)'),
    Case(24, 6, 256, 1024, 'bf16', 2000, 1002, 'coarse', 'table', 'plain bf16: direction only; the batch is table rows, smallest gap 0.86'),
]


def case_id(c):
    return f'prdc-O{c.O}A{c.A}H{c.H}B{c.B}N{c.N}-{c.precision}'


def params(c):
    """(actor, critic) dicts key -> float32 array, in parameters() order."""
    ash, csh = param_shapes('td3_bc', c.O, c.A, c.H)
    return _synth.synth_params(ash, c.seed), _synth.synth_params(csh, c.seed + 1)


def episode(c):
    return _synth.synth_episodes(c.seed + 5, [c.N], c.O, c.A)[0]


def keys_of(ep, beta, O, A, mean=None, inv=None, every=1):
    """The key rows of one episode as exorl_replay_build_keys forms them, in numpy float32: [beta * s | a | 0-pad], s = obs[t - 1]
    (normalised in two float32 operations when mean / inv are given), a = action[t], t = 1 .. len; every `every`-th kept."""
    obs, act = np.asarray(ep['observation'], np.float32), np.asarray(ep['action'], np.float32)
    s = obs[:-1]
    if mean is not None:
        s = ((s - np.asarray(mean, np.float32)).astype(np.float32) * np.asarray(inv, np.float32)).astype(np.float32)
    out = np.zeros((len(s), -(-(O + A) // 4) * 4), np.float32)
    out[:, :O] = (np.float32(beta) * s).astype(np.float32)
    out[:, O:O + A] = act[1:]
    return out[::every]


def table(c):
    return keys_of(episode(c), BETA, c.O, c.A)


def batch(c):
    b = _synth.synth_batch(c.seed + 2, 0, c.B, c.O, c.A)
    if c.rows == 'table':
        ep = episode(c)
        b = (np.ascontiguousarray(ep['observation'][:c.B]), np.ascontiguousarray(ep['action'][1:c.B + 1])) + b[2:]
    return b


def noise(c):
    ns = _synth.NoiseStream(c.seed + 3)
    return [ns.draw((c.B, c.A)), ns.draw((c.B, c.A))]


def make_twin(c, dtype, **kw):
    pa, pc = params(c)
    return PRDCTwin(list(pa.values()), list(pc.values()), table(c), c.O, BETA, dtype=dtype, **kw)


def run_twin(c, dtype, kink_delta=None, critic_after=None):
    return make_twin(c, dtype).update(batch(c), 0, *noise(c), kink_delta=kink_delta, kink_cap=KINK_CAP, critic_after=critic_after)


@lru_cache(maxsize=4)
def twin_pair(c):
    """(twin64 result with the near-kink directions at the case's delta — none for a coarse case —, twin32 result)."""
    return run_twin(c, torch.float64, None if c.bar == 'coarse' else KINK_DELTA[c.precision]), run_twin(c, torch.float32)


STEPS = ('critic', 'actor')


def steps_of(res):
    return [(s, getattr(res, f'{s}_grads')) for s in STEPS]


def qualify(c):
    """The list of reasons the case does not qualify (empty: it does): the float32 and float64 twins take the same discrete decisions, the
    neighbour of EVERY row among them; every decision has a float64 margin >= MARGIN (the neighbour's: the relative gap to the runner-up;
    the plain-bf16 case's gap exceeds BF16_GAP); and (tight cases) the near-kink set of every step is within KINK_CAP and the two twins'
    ReLU masks agree outside it."""
    r64, r32 = twin_pair(c)
    bad = []
    for name, (choice, margin) in r64.decisions.items():
        if not np.array_equal(choice, r32.decisions[name][0]):
            bad.append(f'{name}: twin32 decides differently')
        if float(margin.min()) < MARGIN:
            bad.append(f'{name}: margin {float(margin.min()):.2e}')
    if c.precision == 'bf16' and float(r64.decisions['nn'][1].min()) < BF16_GAP:
        bad.append(f'nn: plain-bf16 gap {float(r64.decisions["nn"][1].min()):.2e}')
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


# ---- the stand-alone search's grid (tests/test_gpu_nn_search.py): (N keys, D columns, query rows, seed). Keys and queries are
# NoiseStream(seed).draw((N, D)) then .draw((rows, D)); the seed is the smallest >= 1 for which every row's gap is >= MARGIN (searched
# once on the CPU, checked in tests/test_prdc_twin.py). Edges: one key; a ragged, a full and a just-started second key tile (63, 64, 65);
# D = 3 (no vector loads: pitch 3), 30, 33 (a second column chunk of one column), 256 (eight chunks); 1, 7, 64, 72 (a ragged second query
# tile) and 1000 query rows; 20000 keys: more tiles than key ranges.
SEARCH_GRID = [
    (1, 3, 1, 1), (1, 30, 7, 1), (63, 3, 7, 1), (63, 256, 64, 1), (64, 30, 64, 2), (65, 33, 72, 1), (65, 256, 1, 1), (1000, 3, 72, 1),
    (1000, 30, 64, 1), (1000, 33, 1000, 2), (1000, 256, 72, 2), (20000, 3, 64, 1), (20000, 256, 7, 1), (20000, 30, 1000, 16),
]


def search_inputs(N, D, rows, seed):
    ns = _synth.NoiseStream(seed)
    return ns.draw((N, D)), ns.draw((rows, D))


def search_reference(keys, q):
    """(idx, d2, relative gap) of the float64 brute force on the float32 inputs, widened."""
    from _prdc_twin import brute_force_nn
    idx, d2, gap = brute_force_nn(torch.from_numpy(q.astype(np.float64)), torch.from_numpy(keys.astype(np.float64)))
    return idx.numpy(), d2.numpy(), gap.numpy()


# ---- the five-step trajectory of tests/test_gpu_prdc.py (batches synth_batch(seed + 2, step), noise NoiseStream(seed + 3) in step order)
TRAJ = Case(5, 2, 32, 8, 'fp32', 200, 40, 'tight', 'random', 'five steps')


def traj_bar(p64, step):
    """tests/_iql_cases.py's: an Adam update moves a parameter by lr m^ / (sqrt(v^) + eps); a relative error of 1e-3 in that ratio is
    1e-3 lr, storing the parameter rounds it once; both add up over the steps."""
    return (step + 1) * (2.0 ** -23 * max(float(np.abs(p64).max()), 1.0) + 1e-3 * 1e-4)


# ---- the agent under test
def make_agent(c, use_tb=True, **kw):
    from exorl_amd import agents
    args = dict(precision=c.precision, beta=BETA)
    args.update(kw)
    return agents.PRDCAgent('prdc', (c.O,), (c.A,), 'cuda', 1e-4, c.H, 0.01, 0.2, 1, c.B, 0.3, use_tb, 2.5, **args)


def load_params(ag, c):
    pa, pc = params(c)
    ag.actor.load_state_dict({k: torch.from_numpy(v) for k, v in pa.items()})
    ag.critic.load_state_dict({k: torch.from_numpy(v) for k, v in pc.items()})
    ag.critic_target.load_state_dict(ag.critic.state_dict())
    return ag


def arena_of(eps, O, A):
    """(ReplayEngine holding the episodes in order, an ArenaIterator over it)."""
    from exorl_amd.engine import ReplayEngine
    from exorl_amd.replay_buffer import ArenaIterator
    rows = sum(len(ep['observation']) for ep in eps)
    eng = ReplayEngine((O,), np.float32, A, 0, rows + 64, len(eps) + 4)
    eng.set_order([eng.append_episode(ep) for ep in eps])
    eng.seed_philox(77)
    return eng, ArenaIterator(eng, 1, 1, 0.99, 'philox')


def bind(ag, c):
    """The case's table built from its episode in an arena and bound; returns what must stay alive."""
    eng, it = arena_of([episode(c)], c.O, c.A)
    assert ag.bind_dataset(it) == c.N
    return eng, it
