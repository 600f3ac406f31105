"""The FQE twin (tests/_fqe_twin.py) held to its own definition in float64, and the qualification of the case table (tests/_fqe_cases.py). CPU."""
import numpy as np
import pytest
import torch

import _fqe_cases as F
from _iql_cases import traj_bar
from oracle.twin64 import Twin

SMALL = F.Case(5, 2, 16, 9, 'fp32', 7, 'tight', 'small enough for finite differences')


def test_critic_gradient_equals_central_differences_of_its_own_loss():
    tw = F.make_twin(SMALL, torch.float64)
    b = F.batch(SMALL)
    grads = torch.autograd.grad(tw.loss(b)[0], tw.critic)
    rs = np.random.RandomState(0)
    for p, g in zip(tw.critic, grads):
        flat = p.detach().view(-1)
        for i in rs.choice(flat.numel(), min(4, flat.numel()), replace=False):
            old, h = float(flat[i]), 1e-6
            with torch.no_grad():
                flat[i] = old + h
                up = float(tw.loss(b)[0])
                flat[i] = old - h
                dn = float(tw.loss(b)[0])
                flat[i] = old
            fd = (up - dn) / (2 * h)
            assert abs(fd - float(g.view(-1)[i])) <= 1e-6 * max(1.0, abs(fd)) + 1e-9, (i, fd, float(g.view(-1)[i]))


def test_each_net_has_its_own_target_and_the_actor_is_frozen():
    """With the target's second net replaced by its first, y_2 = y_1 and net 1's gradients do not move: no min couples the twins. The
    actor's tensors are the same objects with the same values after the step, and none of them is part of a graph."""
    tw = F.make_twin(SMALL, torch.float64)
    b = F.batch(SMALL)
    before = [a.clone() for a in tw.actor]
    g = torch.autograd.grad(tw.loss(b)[0], tw.critic)
    other = F.make_twin(SMALL, torch.float64)
    for i in range(8):
        other.critic_target[8 + i] = other.critic_target[i].clone()
    g2 = torch.autograd.grad(other.loss(b)[0], other.critic)
    for a, c in zip(g[:8], g2[:8]):
        assert torch.equal(a, c)
    assert any(not torch.equal(a, c) for a, c in zip(g[8:], g2[8:]))
    tw.update(b)
    assert all(torch.equal(a, c) and not a.requires_grad for a, c in zip(tw.actor, before))


def test_target_is_td3s_without_noise_and_without_the_min():
    """Against oracle.twin64's TD3 twin with zero noise on a batch whose rows all have Q'_1 <= Q'_2: there min(Q'_1, Q'_2) = Q'_1, so net 1's
    gradients coincide with TD3's and net 2's do not (TD3 regresses it on Q'_1 too)."""
    pa, pc = F.params(SMALL)
    tw = F.make_twin(SMALL, torch.float64)
    obs, action, reward, discount, next_obs = F.batch(SMALL)
    with torch.no_grad():
        no = tw._t(next_obs)
        t1, t2 = tw._critic(tw.critic_target, torch.cat([no, tw.mu(no)], -1))
    keep = (t1 <= t2).reshape(-1).numpy()
    assert 2 <= keep.sum() < len(keep)
    sub = tuple(np.ascontiguousarray(x[keep]) for x in (obs, action, reward, discount, next_obs))
    g = torch.autograd.grad(tw.loss(sub)[0], tw.critic)
    zeros = np.zeros((int(keep.sum()), SMALL.A))
    td3 = Twin('td3', list(pa.values()), list(pc.values()), dtype=torch.float64, stddev=0.2).update(sub, 0, zeros, zeros)
    for a, w in zip(g[:8], td3.critic_grads[:8]):
        np.testing.assert_allclose(a.numpy(), w, rtol=1e-12, atol=1e-300)
    assert any(not np.allclose(a.numpy(), w, rtol=1e-6, atol=0) for a, w in zip(g[8:], td3.critic_grads[8:]))


@pytest.mark.parametrize('c', [pytest.param(c, id=F.case_id(c)) for c in F.CASES])
def test_case_qualifies(c):
    assert F.qualify(c) == []
    assert F.twin_pair(c)[0].decisions == {}          # nothing discrete but the ReLU masks


def test_trajectory_case_qualifies():
    """The float32 twin stays within half of _iql_cases.traj_bar of the float64 twin over the five steps: the bar leaves the GPU as much room
    again."""
    c = F.TRAJ
    t64, t32 = F.make_twin(c, torch.float64), F.make_twin(c, torch.float32)
    for step in range(5):
        b = F.batch(c, step)
        t64.update(b), t32.update(b)
        for nm in ('critic', 'critic_target'):
            for p, q in zip(getattr(t32, nm), getattr(t64, nm)):
                q = q.detach().numpy()
                assert float(np.abs(p.detach().double().numpy() - q).max()) <= 0.5 * traj_bar(q, step), (step, nm)
