"""torch-autograd twin of IQLAgent.update(), dtype selectable (test infrastructure only). IQL has no reference file: this restates the
specification in exorl_amd.agents.IQLAgent's docstring. Built from oracle/twin64.py's helpers, which it does not change.

One update() on (s, a, r, D, s'), every forward on the parameters from before the step:
    q_t = min(Q'_1(s,a), Q'_2(s,a))            target critic, no gradient
    v = V(s), v' = V(s');  u = q_t - v;  k = (u < 0) ? 1 - expectile : expectile
    L_V  = mean(k u^2)
    y    = r + D v'  (no gradient);  L_Q = mse(Q_1(s,a), y) + mse(Q_2(s,a), y)
    w    = min(exp(temperature u), max_weight)  (no gradient)
    L_pi = -mean(w sum_a log N(a; tanh-mean mu(s), std))
then Adam on value, critic, actor and the soft update of the target. Result carries value_grads next to critic_grads / actor_grads and the
decisions target_min, u_negative, weight_clamped with their float64-meaningful relative margins."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle.twin64 import Result, _head, _normal_log_prob, _trunk, backward_with_kinks


def _margin(a, b):
    return ((a - b).abs() / torch.maximum(a.abs(), b.abs()).clamp_min(1e-300)).reshape(-1).double().numpy()


class IQLTwin:
    def __init__(self, actor_params, critic_params, value_params, dtype=torch.float64, lr=1e-4, tau=0.01, stddev=0.2, expectile=0.7,
                 temperature=3.0, max_weight=100.0):
        leaf = lambda w: torch.tensor(np.asarray(w, np.float64), dtype=dtype, requires_grad=True)
        self.dtype = dtype
        self.actor, self.critic, self.value = ([leaf(w) for w in ps] for ps in (actor_params, critic_params, value_params))
        self.critic_target = [p.detach().clone() for p in self.critic]
        self.opts = {n: torch.optim.Adam(getattr(self, n), lr=lr) for n in ('value', 'critic', 'actor')}
        self.tau, self.std, self.expectile, self.temperature, self.max_weight = tau, stddev, expectile, temperature, max_weight

    def _critic(self, p, x, tape=None):
        return tuple(_head(p[8 * i + 4:8 * i + 8], _trunk(p[8 * i:8 * i + 4], x), tape, 'critic', f'q{i + 1}', 8 * i + 4) for i in range(2))

    def _value(self, obs, tape=None):
        return _head(self.value[4:8], _trunk(self.value[0:4], obs), tape, 'value', 'value', 4)

    def losses(self, batch, res=None, tapes=None):
        """(L_V, L_Q, L_pi, metrics dict of tensors) on the current parameters; fills res.decisions when given."""
        t = lambda x: torch.as_tensor(np.asarray(x)).to(self.dtype)
        obs, action, reward, discount, next_obs = (t(x) for x in batch[:5])
        tapes = tapes or {'value': None, 'critic': None, 'actor': None}
        x = torch.cat([obs, action], -1)
        with torch.no_grad():
            tq1, tq2 = self._critic(self.critic_target, x)
            qt = torch.min(tq1, tq2)
            v_next = self._value(next_obs)
        v = self._value(obs, tapes['value'])
        u = qt - v
        k = torch.where(u < 0, 1.0 - self.expectile, self.expectile).to(self.dtype).detach()
        value_loss = (k * u * u).mean()
        y = reward + discount * v_next
        q1, q2 = self._critic(self.critic, x, tapes['critic'])
        critic_loss = F.mse_loss(q1, y) + F.mse_loss(q2, y)
        ud = u.detach()
        e = torch.exp(self.temperature * ud)
        w = e.clamp(max=self.max_weight)
        mu = torch.tanh(_head(self.actor[4:8], _trunk(self.actor[0:4], obs), tapes['actor'], 'actor', 'actor', 4))
        actor_loss = -(_normal_log_prob(action, mu, self.std).sum(-1, keepdim=True) * w).mean()
        if res is not None:
            res.decisions['target_min'] = ((tq2 < tq1).reshape(-1).long().numpy(), _margin(tq1, tq2))
            res.decisions['u_negative'] = ((ud < 0).reshape(-1).long().numpy(), _margin(qt, v.detach()))
            res.decisions['weight_clamped'] = ((e > self.max_weight).reshape(-1).long().numpy(),
                                               ((e - self.max_weight).abs() / self.max_weight).reshape(-1).double().numpy())
        m = dict(batch_reward=reward.mean(), critic_target_q=y.mean(), critic_q1=q1.mean(), critic_q2=q2.mean(), critic_loss=critic_loss,
                 actor_loss=actor_loss, value_loss=value_loss, value=v.mean(), adv=u.mean(), actor_weight=w.mean())
        return value_loss, critic_loss, actor_loss, m

    def update(self, batch, kink_delta=None, kink_cap=64):
        res = Result()
        tapes = {'value': [], 'critic': [], 'actor': []}
        lv, lq, lp, m = self.losses(batch, res, tapes)
        res.metrics = {k: v.item() for k, v in m.items()}
        res.metrics['actor_ent'] = (0.5 + 0.5 * math.log(2 * math.pi) + math.log(self.std)) * np.asarray(batch[1]).shape[1]
        every = self.value + self.critic + self.actor
        for step, loss in (('value', lv), ('critic', lq), ('actor', lp)):
            params = getattr(self, step)
            grads = backward_with_kinks(res, step, loss, every, params, tapes[step], kink_delta, kink_cap)
            setattr(res, f'{step}_grads', grads)
            self.opts[step].step()          # each net is in its own loss's graph only: stepping it leaves the other graphs intact
        with torch.no_grad():
            for p, tg in zip(self.critic, self.critic_target):
                tg.copy_(self.tau * p + (1 - self.tau) * tg)
        return res
