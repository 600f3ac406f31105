"""CPU tests of the float64 twin (oracle/twin64.py) and of the gradient grid's case table (tests/_grad_grid.py): the twin against the
reference's recorded float64 runs and, in float32, against the oracle; and for every table case the conditions that make a tight
comparison on the GPU meaningful (identical discrete decisions in float32 and float64 with margins, a small near-kink set)."""
import json

import numpy as np
import pytest
import torch

import _grad_grid as G
import _synth
from oracle.agents import OracleAgent, OracleCQL, param_shapes
from oracle.twin64 import Twin

FULL = ['td3_bc', 'td3', 'ddpg', 'bc', 'crr', 'cql', 'td3_b4096']


def _noise(kind, ns, B, A, n):
    if kind == 'bc':
        return []
    if kind == 'crr':
        return [ns.draw((B, A)), ns.draw((B * n, A))]
    if kind == 'cql':
        return [ns.draw((B, A)), ns.draw((n, B, A)), ns.draw((n, B, A)), ns.draw((n, B, A)), ns.draw((B, A))]
    return [ns.draw((B, A)), ns.draw((B, A))]


@pytest.mark.parametrize('name', FULL)
def test_twin64_matches_recorded_float64_runs(gold, name):
    """First two steps of the reference's own float64 runs at full size (tests/golden/full_*.json["fp64"]), every metric to rtol 1e-9:
    both sides are float64 torch-CPU runs of the same operations, and float64 epsilon times about 1e4 accumulated terms leaves three
    decades of margin."""
    g = json.load(open(gold / f'full_{name}.json'))
    O, A, H, B = g['dims']
    kind = 'td3' if name == 'td3_b4096' else name
    ash, csh = param_shapes(kind, O, A, H)
    pa = list(_synth.synth_params(ash, g['param_seed']).values())
    pc = list(_synth.synth_params(csh, g['param_seed'] + 1).values()) if csh else None
    tw = Twin(kind, pa, pc)
    ns = _synth.NoiseStream(g['noise_seed'])
    worst = 0.0
    for i in range(2):
        step = 2 * i if kind == 'ddpg' else i
        r = tw.update(_synth.synth_batch(g['batch_seed'], i, B, O, A), step, *_noise(kind, ns, B, A, 10 if kind == 'crr' else 3))
        want = g['fp64']['metrics'][i]
        assert sorted(r.metrics) == sorted(want)
        for k, v in want.items():
            worst = max(worst, abs(r.metrics[k] - v) / abs(v) if v else abs(r.metrics[k]))
            assert abs(r.metrics[k] - v) <= 1e-9 * abs(v), (name, i, k, r.metrics[k], v)
    print(f'[twin64 vs recorded fp64] {name}: worst relative metric difference over 2 steps = {worst:.2e} (bar 1e-9)')


TINY = ['td3_bc', 'td3', 'ddpg', 'bc', 'crr', 'crr-exp', 'crr-identity', 'cql', 'cql-lagrange']


@pytest.mark.parametrize('kind', TINY)
def test_twin32_matches_oracle(kind):
    """The float32 twin (autograd) against the oracle's hand-derived float32 backward at the tiny-fixture shape, two steps: every
    gradient tensor within 4e-6 max|g| (the worst float32-against-float32 agreement measured between the two on TD3+BC over three
    shapes, not rounded down), metrics within 2e-5 relative + 1e-6 (test_gradients_vs_oracle_td3_bc's bar)."""
    O, A, H, B, n = 5, 3, 32, 8, 3
    base = 'crr' if kind.startswith('crr') else 'cql' if kind.startswith('cql') else kind
    wf = kind.partition('-')[2] or 'indicator'
    ash, csh = param_shapes(base, O, A, H)
    pa = list(_synth.synth_params(ash, 7).values())
    pc = list(_synth.synth_params(csh, 8).values()) if csh else None
    tw = Twin(base, pa, pc, dtype=torch.float32, num_value_samples=n, weight_func=wf, n_samples=n, use_critic_lagrange=kind == 'cql-lagrange')
    if base == 'cql':
        orc = OracleCQL(pa, pc, n_samples=n, use_critic_lagrange=kind == 'cql-lagrange')
    else:
        orc = OracleAgent(base, pa, pc, num_value_samples=n, weight_func=wf)
    ns = _synth.NoiseStream(9)
    worst = 0.0
    for i in range(2):
        step = 2 * i if base == 'ddpg' else i
        batch = _synth.synth_batch(10, i, B, O, A)
        z = _noise(base, ns, B, A, n)
        r = tw.update(batch, step, *z)
        m = orc.update(batch, step, *z)
        assert sorted(m) == sorted(r.metrics)
        for k, v in m.items():
            assert abs(r.metrics[k] - v) <= 2e-5 * abs(v) + 1e-6, (kind, i, k, r.metrics[k], v)
        for nm, got, want in (('critic', r.critic_grads, getattr(orc, 'last_critic_grads', None)), ('actor', r.actor_grads, orc.last_actor_grads)):
            if got is None:
                continue
            for t, (a, b) in enumerate(zip(got, want)):
                scale = float(np.abs(b).max())
                err = float(np.abs(a.reshape(b.shape) - b).max())
                worst = max(worst, err / scale)
                assert err <= 4e-6 * scale, (kind, i, nm, t, err / scale)
    print(f'[twin32 vs oracle] {kind}: worst max|g32 - g_oracle| / max|g| = {worst:.2e} (bar 4e-6)')


def _near_kink(res, delta):
    """|K(delta)| per step: pre-ReLU elements of the step's graph within delta * max|z| (per ReLU) of the kink."""
    return {s: int(sum((r['z'].abs() < delta * r['z'].abs().max()).sum() for r in relus)) for s, relus in res.relus.items()}


@pytest.mark.parametrize('c', [pytest.param(c, id=G.case_id(c)) for c in G.CASES])
def test_case_qualifies(c):
    """What the GPU comparison of this case rests on, from the twins alone (the seeds were searched once; nothing is searched here):
      * twin32 and twin64 take identical discrete decisions — zero disagreeing rows;
      * each decision's float64 margin is at least 1e-4 relative to the quantities compared (the project's parity bar on forward
        quantities): a kernel within that bar takes the same decisions;
      * the near-kink set of each loss has at most 64 elements at the fp32-mode width 2^-18 max|z| (about 6 times the reference's own
        float32 forward error), for every case; a bf16x3 case is 'tight' exactly when it also has at most 64 at 2^-14 max|z| (4 times
        the 2^-16 split-bf16 product bound);
      * a plain-bf16 case is one where bf16 operands alone leave every tensor's cosine at BF16_FLOOR or better."""
    r64, r32 = G.run_twin(c, torch.float64), G.run_twin(c, torch.float32)
    assert r64.decisions.keys() == r32.decisions.keys()
    for k, (d, margin) in r64.decisions.items():
        assert np.array_equal(d, r32.decisions[k][0]), f'{k}: {int((d != r32.decisions[k][0]).sum())} rows decided differently in float32'
        assert margin.size == 0 or margin.min() >= G.MARGIN, f'{k}: margin {margin.min():.2e}'
    k32, k16 = _near_kink(r64, G.KINK_DELTA['fp32']), _near_kink(r64, G.KINK_DELTA['bf16x3'])
    print(f'[case] {G.case_id(c)}: |K(2^-18)| {k32}, |K(2^-14)| {k16}, smallest margin '
          f'{min([m.min() for _, m in r64.decisions.values() if m.size] or [float("nan")]):.2e}')
    assert max(k32.values()) <= G.KINK_CAP, k32
    if c.precision == 'fp32':
        assert c.bar == 'tight'
    elif c.precision == 'bf16x3':
        assert (c.bar == 'tight') == (max(k16.values()) <= G.KINK_CAP), (c.bar, k16)
    else:
        assert c.bar == 'coarse'
        rb = G.run_twin(c, torch.float32, bf16_operands=True)
        for s, want in G.steps_of(r64):
            cos = G.tensor_cosines(dict(critic=rb.critic_grads, actor=rb.actor_grads)[s], want)
            assert min(cos) >= G.BF16_FLOOR, (s, int(np.argmin(cos)), min(cos))


def test_grid_reaches_the_dispatch_edges():
    """The table covers what it was written to cover."""
    fam = [c for c in G.CASES if c.kind in ('td3_bc', 'td3', 'ddpg')]
    cql = [c for c in G.CASES if c.kind.startswith('cql')]
    assert {1, 2, 8, 9, 16} <= {c.A for c in fam}
    assert {3, 5, 8, 9, 16} <= {c.A for c in cql}
    assert {6, 32, 33, 35, 36, 90, 256} <= {c.O + c.A for c in G.CASES}
    assert {35, 36, 90} <= {c.O + c.A for c in fam if c.H == 1024 and c.precision == 'fp32'}
    assert {4, 32, 100, 128, 192, 320, 384, 1024} <= {c.H for c in G.CASES}
    assert {1, 7, 50, 64, 72, 1000, 1024} <= {c.B for c in G.CASES}
    assert any(c.kind == 'td3' and c.B == 8200 for c in G.CASES)
    assert {1000, 1024} <= {c.B for c in cql if c.n == 3 and (3 * c.n + 1) * c.B >= 8192 and c.precision == 'fp32'}
    assert any(c.kind.startswith('crr') and all(k % c.n for k in (4, 8, 16, 32)) for c in G.CASES)
    planes = lambda c: c.H % 128 == 0 and c.B % 64 == 0
    x3 = [c for c in G.CASES if c.precision == 'bf16x3']
    assert any(planes(c) for c in x3) and any(not planes(c) for c in x3)
    assert all(c.H % 8 == 0 and c.B % 8 == 0 for c in G.CASES if c.precision == 'bf16') and any(c.precision == 'bf16' for c in G.CASES)
    assert 2 * sum(c.bar == 'tight' for c in x3) >= len(x3)
    assert all(c.bar == 'tight' for c in x3 if c.B * c.H <= 16384)
    assert len({G.case_id(c) for c in G.CASES}) == len(G.CASES)
