"""CPU checks of the Cal-QL twin (tests/_calql_twin.py) and of its case table (tests/_calql_cases.py): with m = -inf the twin is
oracle.twin64.Twin('cql') to the last bit; the bound's rule and gradient on hand-computed rows, an exact tie among them; and for every
recorded case the conditions that make the GPU comparison meaningful. No GPU is touched, nothing is searched."""
import math

import numpy as np
import pytest
import torch

import _calql_cases as K
import _grad_grid as G
from _calql_twin import CalQLTwin, bound_rows
from oracle.twin64 import Twin


@pytest.mark.parametrize('lagrange', [False, True])
def test_minus_infinity_is_the_cql_twin(lagrange):
    """Two steps, float64 and float32: every gradient, metric and parameter of CalQLTwin fed m = -inf equals Twin('cql')'s exactly, and
    nothing is bounded."""
    c = G.Case('cql-lagrange' if lagrange else 'cql', 5, 3, 32, 7, 3, 'fp32', 11, 'tight', '')
    pa, pc, _, _ = G.params(c)
    for dtype in (torch.float64, torch.float32):
        base = Twin('cql', pa, pc, dtype=dtype, n_samples=c.n, use_critic_lagrange=lagrange)
        cal = CalQLTwin(pa, pc, dtype=dtype, n_samples=c.n, use_critic_lagrange=lagrange)
        z = G.noise(c)
        for step in range(2):
            b = K.batch_at(c, step)
            rb = base.update(b, step, *z, rand_is_uniform=True)
            rc = cal.update(b + (np.full(c.B, -np.inf, np.float32),), step, *z, rand_is_uniform=True)
            assert rc.metrics.pop('calql_bound_rate') == 0.0 and rc.metrics == rb.metrics
            for got, want in ((rc.critic_grads, rb.critic_grads), (rc.actor_grads, rb.actor_grads)):
                assert all(np.array_equal(g, w) for g, w in zip(got, want))
            for net in ('actor', 'critic', 'critic_target'):
                assert all(torch.equal(p, q) for p, q in zip(getattr(cal, net), getattr(base, net)))
            assert torch.equal(cal.log_critic_alpha, base.log_critic_alpha) and torch.equal(cal.log_actor_alpha, base.log_actor_alpha)


def test_bound_on_hand_computed_rows():
    """B = 2, n = 1: four entries a row (random, pi(s), pi(s'), data). Row 0, m = 1: q = (0, 1, 2, 0.5): the tie at 1 keeps q and its
    gradient, nothing is bounded. Row 1, m = 0: q = (0, -1, 3, 0.5): the entry -1 becomes 0 and gets no gradient. The gradient of the
    mean over b of logsumexp is the softmax over the bounded row, over B, with 0 on the bounded entry."""
    B, n = 2, 1
    rows = np.array([[0.0, 1.0, 2.0, 0.5], [0.0, -1.0, 3.0, 0.5]])
    q = torch.tensor(rows.T.reshape(-1, 1), dtype=torch.float64, requires_grad=True)        # row k B + b
    m = torch.tensor([1.0, 0.0], dtype=torch.float64)
    qh, bounded = bound_rows(q, m, n, B)
    assert qh.detach().reshape(4, B).T.tolist() == [[0.0, 1.0, 2.0, 0.5], [0.0, 0.0, 3.0, 0.5]]
    assert bounded.reshape(2 * n, B).T.tolist() == [[False, False], [True, False]]
    torch.logsumexp(qh.reshape(3 * n + 1, B, 1), 0).mean().backward()
    got = q.grad.reshape(4, B).T.numpy()
    for b, hat in enumerate(([0.0, 1.0, 2.0, 0.5], [0.0, 0.0, 3.0, 0.5])):
        se = sum(math.exp(v) for v in hat)
        want = [math.exp(v) / se / B for v in hat]
        if b == 1:
            want[1] = 0.0
            assert got[b, 1] == 0.0
        assert np.allclose(got[b], want, rtol=1e-15, atol=0), (b, got[b], want)
    assert got[0, 1] > 0.0          # the tie keeps its gradient
    # the rows outside blocks 1 and 2 are never bounded, whatever m is
    qh, bounded = bound_rows(q.detach(), torch.tensor([1e30, 1e30], dtype=torch.float64), n, B)
    assert bool(bounded.all()) and qh.reshape(4, B)[0].tolist() == [0.0, 0.0] and qh.reshape(4, B)[3].tolist() == [0.5, 0.5]
    assert qh.reshape(4, B)[1:3].eq(1e30).all()


def test_the_twin_steps_from_the_bounded_penalty():
    """One step of the smallest case by hand from the twin's own nets: the penalty and the critic loss are CQL's formulas on the bounded
    rows, the mse and the target are untouched, and the bound rate is the share of policy-action entries below m."""
    c = K.CASES[0]
    tw = K.make_twin(c, torch.float64)
    b, z = K.batch(c), G.noise(c)
    r = tw.update(b, 0, *z, rand_is_uniform=True)
    q = tw.policy_q.numpy()                                    # (2, 2n, B), the pre-step critic
    m = np.asarray(b[5], np.float64)
    assert r.metrics['calql_bound_rate'] == float((q < m[None, None]).mean())
    base = Twin('cql', *G.params(c)[:2], n_samples=c.n).update(b[:5], 0, *z, rand_is_uniform=True)
    for k in ('critic_target_q', 'critic_q1', 'critic_q2', 'batch_reward'):
        assert r.metrics[k] == base.metrics[k]
    assert r.metrics['critic_cql_logsum'] > base.metrics['critic_cql_logsum']          # max(q, m) >= q, strictly on the bounded entries
    assert r.metrics['critic_cql'] - r.metrics['critic_cql_logsum'] == base.metrics['critic_cql'] - base.metrics['critic_cql_logsum']


@pytest.mark.parametrize('c', [pytest.param(c, id=K.case_id(c)) for c in K.CASES])
def test_case_qualifies(c):
    """The recorded seed qualifies (tests/_calql_cases.py, qualify): the bounded share lies in [1/4, 3/4], the float32 and float64 twins
    take identical decisions (the bound's 4 n B among them) with float64 margins >= 1e-4, the near-kink sets are within the cap."""
    bad = K.qualify(c)
    r = K.run_twin(c, torch.float64)
    choice, margin = r.decisions['calql_bound']
    print(f'[calql case] {K.case_id(c)}: bounded share {r.metrics["calql_bound_rate"]:.3f}, smallest bound margin {margin.min():.2e}')
    assert choice.size == 4 * c.n * c.B and bad == [], bad
    assert K.bound(c).dtype == np.float32 and K.bound(c).shape == (c.B,)


def test_table_covers_the_issues_shapes():
    got = {(c.O, c.A, c.H, c.B, c.n, c.precision, c.kind == 'cql-lagrange') for c in K.CASES}
    assert got == {(5, 3, 32, 7, 3, 'fp32', False), (24, 5, 100, 50, 3, 'fp32', False), (24, 5, 100, 50, 3, 'bf16x3', False),
                   (17, 16, 64, 50, 3, 'fp32', True), (24, 6, 128, 64, 3, 'bf16x3', False), (24, 6, 128, 64, 3, 'bf16x6', False),
                   (24, 8, 192, 257, 2, 'fp32', False), (24, 6, 128, 256, 3, 'bf16', False)}
    assert all((c.bar == 'coarse') == (c.precision == 'bf16') for c in K.CASES)
    for c in K.TRAJ_CASES:
        rates = [m['calql_bound_rate'] for m, _, _ in K.run_traj(c, torch.float64)]
        assert len(rates) == K.TRAJ_STEPS and all(0.25 <= x <= 0.75 for x in rates), rates
