"""The IQL twin (tests/_iql_twin.py) held to its own definition in float64, and the qualification of the case table (tests/_iql_cases.py). CPU."""
import numpy as np
import pytest
import torch

import _iql_cases as I
from _iql_twin import IQLTwin
from oracle.twin64 import Twin

SMALL = I.Case(5, 2, 16, 9, 'fp32', 7, 'tight', I.DEFAULT, False, 'small enough for finite differences')


def test_value_gradient_equals_central_differences_of_its_own_loss():
    tw = I.make_twin(SMALL, torch.float64)
    b = I.batch(SMALL)
    lv = tw.losses(b)[0]
    grads = torch.autograd.grad(lv, tw.value)
    rs = np.random.RandomState(0)
    for p, g in zip(tw.value, grads):
        flat = p.detach().view(-1)
        for i in rs.choice(flat.numel(), min(6, flat.numel()), replace=False):
            old, h = float(flat[i]), 1e-6
            with torch.no_grad():
                flat[i] = old + h
                up = float(tw.losses(b)[0])
                flat[i] = old - h
                dn = float(tw.losses(b)[0])
                flat[i] = old
            fd = (up - dn) / (2 * h)
            assert abs(fd - float(g.view(-1)[i])) <= 1e-6 * max(1.0, abs(fd)) + 1e-9, (i, fd, float(g.view(-1)[i]))


def test_expectile_half_is_half_the_mse():
    tw = I.make_twin(SMALL, torch.float64, expectile=0.5)
    b = I.batch(SMALL)
    lv = tw.losses(b)[0]
    g = torch.autograd.grad(lv, tw.value)
    t = lambda x: torch.as_tensor(np.asarray(x)).double()
    with torch.no_grad():
        qt = torch.min(*tw._critic(tw.critic_target, torch.cat([t(b[0]), t(b[1])], -1)))
    mse = ((qt - tw._value(t(b[0]))) ** 2).mean()
    gm = torch.autograd.grad(mse, tw.value)
    assert abs(lv.item() - 0.5 * mse.item()) <= 1e-15 * abs(mse.item())
    for a, c in zip(g, gm):
        assert torch.allclose(a, 0.5 * c, rtol=1e-13, atol=1e-300)


def test_temperature_zero_gives_bc_actor_gradients():
    tw = I.make_twin(SMALL, torch.float64, temperature=0.0)
    b = I.batch(SMALL)
    res = tw.update(b)
    assert np.all(res.decisions['weight_clamped'][0] == 0)
    pa, _, _ = I.params(SMALL)
    bc = Twin('bc', list(pa.values()), dtype=torch.float64, stddev=0.2).update(b, 0)
    for g, w in zip(res.actor_grads, bc.actor_grads):
        np.testing.assert_allclose(g, w, rtol=1e-13, atol=1e-300)


@pytest.mark.parametrize('c', [pytest.param(c, id=I.case_id(c)) for c in I.CASES])
def test_case_qualifies(c):
    assert I.qualify(c) == []


def test_trajectory_case_qualifies():
    """The float32 twin stays within half of traj_bar of the float64 twin over the five steps: the bar leaves the GPU as much room again."""
    import _synth
    c = I.TRAJ
    t64, t32 = I.make_twin(c, torch.float64), I.make_twin(c, torch.float32)
    for step in range(5):
        b = _synth.synth_batch(c.seed + 2, step, c.B, c.O, c.A)
        t64.update(b), t32.update(b)
        for nm in ('actor', 'critic', 'critic_target', 'value'):
            for p, q in zip(getattr(t32, nm), getattr(t64, nm)):
                q = q.detach().numpy()
                assert float(np.abs(p.detach().double().numpy() - q).max()) <= 0.5 * I.traj_bar(q, step), (step, nm)
