"""CPU checks of the ReBRAC twin (tests/_rebrac_twin.py) and its cases: critic_beta = 0 is oracle.twin64's TD3+BC twin exactly, nothing
flows back through the penalty, the actor-loss rescaling identity at float64, the penalty against a hand computation, every case qualifies
at its recorded seed, and the float32 twin keeps the trajectory's bars with room to spare."""
import numpy as np
import pytest
import torch

import _rebrac_twin as R
from oracle.twin64 import Twin


def _same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('c', [pytest.param(c, id=R.case_id(c)) for c in R.CASES[:2]])
def test_beta_zero_is_the_td3bc_twin_exactly(c):
    pa, pc = R.params(c)
    for dtype in (torch.float64, torch.float32):
        re = R.make_twin(c, dtype, critic_beta=0.0)
        td = Twin('td3_bc', list(pa.values()), list(pc.values()), dtype=dtype, alpha=R.alpha_of(c.A))
        for step in range(2):
            z = R.noise(c._replace(seed=c.seed + step))
            b = R.batch(c, step)
            r, t = re.update(b, step, *z), td.update(b[:5], step, *z)
            assert _same(r.critic_grads, t.critic_grads) and _same(r.actor_grads, t.actor_grads)
            assert {k: v for k, v in r.metrics.items() if k not in ('critic_penalty', 'next_valid')} == t.metrics
            assert r.metrics['critic_penalty'] > 0 and 0 < r.metrics['next_valid'] < 1
        for net in ('actor', 'critic', 'critic_target'):
            assert all(torch.equal(p, q) for p, q in zip(getattr(re, net), getattr(td, net))), net


def test_all_invalid_rows_are_the_td3bc_twin_exactly():
    c = R.CASES[0]
    pa, pc = R.params(c)
    b = R.batch(c)
    b = b[:5] + (np.zeros_like(b[5]), np.zeros_like(b[6]))
    r = R.make_twin(c, torch.float64, critic_beta=5.0).update(b, 0, *R.noise(c))
    t = Twin('td3_bc', list(pa.values()), list(pc.values()), dtype=torch.float64, alpha=R.alpha_of(c.A)).update(b[:5], 0, *R.noise(c))
    assert _same(r.critic_grads, t.critic_grads) and _same(r.actor_grads, t.actor_grads)
    assert r.metrics['critic_penalty'] == 0.0 and r.metrics['next_valid'] == 0.0 and r.metrics['critic_loss'] == t.metrics['critic_loss']


def test_nothing_flows_back_through_the_penalty():
    """y is formed under no_grad: the critic loss's backward leaves every actor parameter without a gradient, and the penalty moves the
    critic's gradient only through y's value."""
    c = R.CASES[1]
    r1 = R.run_twin(c, torch.float64)
    assert r1.actor_grads_after_critic and all(g is None for g in r1.actor_grads_after_critic)
    r0 = R.make_twin(c, torch.float64, critic_beta=0.0).update(R.batch(c), 0, *R.noise(c))
    assert not _same(r1.critic_grads, r0.critic_grads) and r1.metrics['critic_target_q'] < r0.metrics['critic_target_q']
    assert r1.metrics['batch_reward'] == r0.metrics['batch_reward']


def test_penalty_against_a_hand_computation():
    """Two rows, A = 2, a net whose output is known: compare y's mean with r + D (min Q' - beta v sum (a~' - a')^2) formed by hand from the
    twin's own next-action sample."""
    c = R.Case(3, 2, 8, 2, 'fp32', 11, 'tight', '')
    b = R.batch(c)
    z = R.noise(c)
    tw = R.make_twin(c, torch.float64, critic_beta=0.75)
    t = lambda x: torch.as_tensor(np.asarray(x)).double()
    with torch.no_grad():
        a_s = tw._sample(torch.tanh(tw._actor_raw(tw.actor, t(b[4]))), t(z[0]), None, 'target')
        q1, q2 = tw._critic(tw.critic_target, t(b[4]), a_s)
    pen = b[6].astype(np.float64) * ((a_s.numpy() - b[5].astype(np.float64)) ** 2).sum(1)
    y = b[2][:, 0].astype(np.float64) + b[3][:, 0].astype(np.float64) * (torch.min(q1, q2)[:, 0].numpy() - 0.75 * pen)
    r = tw.update(b, 0, *z)
    assert b[6].tolist() == [1.0, 0.0] and pen[1] == 0.0 and pen[0] > 0
    assert abs(r.metrics['critic_target_q'] - y.mean()) <= 1e-15 * abs(y.mean()) + 1e-15
    assert abs(r.metrics['critic_penalty'] - pen.mean()) <= 1e-15


@pytest.mark.parametrize('actor_bc,A', [(1.0, 1), (0.4, 6), (2.5, 16)])
def test_actor_loss_rescaling_identity(actor_bc, A):
    """beta_a sum_j (mu - a)_j^2 - Q / mean|Q|  ==  (beta_a A) (mse(mu, a) - (alpha / mean|Q|) mean Q) with alpha = 1 / (beta_a A): values and
    gradients, float64, to a few ulp."""
    g = torch.Generator().manual_seed(3)
    B = 33
    mu = torch.randn(B, A, generator=g, dtype=torch.float64, requires_grad=True)
    q = (torch.randn(B, 1, generator=g, dtype=torch.float64) * 7 + 2).requires_grad_()
    a = torch.rand(B, A, generator=g, dtype=torch.float64) * 2 - 1
    lr = R.rebrac_actor_loss(mu, a, q, actor_bc)
    lt = R.td3bc_actor_loss(mu, a, q, R.alpha_of(A, actor_bc))
    k = actor_bc * A
    assert abs(lr.item() - k * lt.item()) <= 1e-14 * abs(lr.item())
    gr = torch.autograd.grad(lr, [mu, q])
    gt = torch.autograd.grad(lt, [mu, q])
    for x, y in zip(gr, gt):
        assert float((x - k * y).abs().max()) <= 1e-14 * float(x.abs().max())


@pytest.mark.parametrize('c', [pytest.param(c, id=R.case_id(c)) for c in R.CASES])
def test_cases_qualify(c):
    assert R.qualify(c) == []


def test_plain_bf16_case_leaves_room_under_the_direction_bar():
    """tests/_grad_grid.py's condition on a plain-bf16 case: with bf16-rounded operands in the twin every gradient tensor keeps cosine >=
    BF16_FLOOR against twin64, so the format itself leaves half of the 1 - 0.999 bar."""
    from _grad_grid import BF16_FLOOR, tensor_cosines
    c = R.CASES[-1]
    assert c.precision == 'bf16'
    r64 = R.twin_pair(c)[0]
    rb = R.make_twin(c, torch.float64, bf16_operands=True).update(R.batch(c), 0, *R.noise(c))
    for step, want in R.steps_of(r64):
        assert min(tensor_cosines(getattr(rb, f'{step}_grads'), want)) >= BF16_FLOOR, step


def test_float32_twin_keeps_the_trajectory_bars_with_room():
    """The reference's own float32 error over the three steps is within half of traj_bar on every parameter and half of the metric bar."""
    t64, t32 = R.run_traj(R.TRAJ, torch.float64), R.run_traj(R.TRAJ, torch.float32)
    for step, ((m64, p64), (m32, p32)) in enumerate(zip(t64, t32)):
        for n64, n32 in zip(p64, p32):
            for a, b in zip(n64, n32):
                assert float(np.abs(a - b).max()) <= 0.5 * R.traj_bar(a, step)
        for k, v in m64.items():
            assert abs(m32[k] - v) <= 0.5 * (2e-5 * abs(v) + 1e-6), (step, k)


@pytest.mark.parametrize('shape', sorted(R.TRAJ_E32))
def test_recorded_float32_trajectory_errors_are_the_measured_ones(shape):
    """TRAJ_E32, the figures behind the fp32-grade trajectories' measured bar (twice the float32 CPU twin's own error against the float64
    twin, profiles/rebrac_step.txt), are what the twins give on the case. A float32 matrix product's summation order is the host
    library's, so another host's figure may differ in its digits: within a factor of 1.5 either way."""
    c = next(c for c in R.TRAJ_CASES if (c.O, c.A, c.H, c.B) == shape)
    got = R.traj_e32(c)
    assert len(got) == R.TRAJ_STEPS
    for g, want in zip(got, R.TRAJ_E32[shape]):
        assert want / 1.5 <= g <= 1.5 * want, (shape, got, R.TRAJ_E32[shape])


def test_recorded_bf16_format_cosines_are_the_measured_ones():
    """TRAJ_BF16_COS, what the plain-bf16 format alone costs the direction of the three-step parameter change, is what the bf16-operand
    twin gives on the case: 1 - cosine within a factor of 1.5 either way (the host library's summation order moves the digits)."""
    c = R.TRAJ_CASES[-1]
    assert c.precision == 'bf16'
    got = R.traj_bf16_cos(c)
    for row, want in zip(got, R.TRAJ_BF16_COS):
        for g, w in zip(row, want):
            assert (1.0 - w) / 1.5 <= 1.0 - g <= 1.5 * (1.0 - w), (got, R.TRAJ_BF16_COS)


def test_trajectory_cases_cover_both_shapes_and_every_precision():
    seen = {((c.O, c.A, c.H, c.B), c.precision) for c in R.TRAJ_CASES}
    for shape in ((5, 1, 8, 7), (24, 6, 128, 257)):
        assert {p for s, p in seen if s == shape} == {'fp32', 'bf16x6', 'bf16x3'}
    assert ((24, 6, 256, 1024), 'bf16') in seen          # plain bf16 needs 8 | H and 8 | B: the library refuses the two shapes above
