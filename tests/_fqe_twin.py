"""torch-autograd twin of FQEAgent.update() and of its value pass, dtype selectable (test infrastructure only). FQE has no reference file:
this restates the specification in exorl_amd.agents.FQEAgent's docstring. Built from oracle/twin64.py's helpers, which it does not change.

One update() on (s, a, r, D, s'), every forward on the parameters from before the step, the actor frozen:
    a'  = tanh-mean mu(s')                                  no gradient, the actor never steps
    y_i = r + D Q'_i(s', a')   per net, its own target      no gradient, NO min over the twins
    L   = mse(Q_1(s, a), y_1) + mse(Q_2(s, a), y_2)
then Adam on the critic and the soft update of the target. The only discrete decisions are the ReLU masks: Result.decisions stays empty."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.twin64 import Result, _head, _trunk, backward_with_kinks


class FQETwin:
    def __init__(self, actor_params, critic_params, dtype=torch.float64, lr=1e-4, tau=0.01):
        leaf = lambda w: torch.tensor(np.asarray(w, np.float64), dtype=dtype, requires_grad=True)
        self.dtype = dtype
        self.actor = [torch.tensor(np.asarray(w, np.float64), dtype=dtype) for w in actor_params]          # frozen: not a leaf of any graph
        self.critic = [leaf(w) for w in critic_params]
        self.critic_target = [p.detach().clone() for p in self.critic]
        self.opt = torch.optim.Adam(self.critic, lr=lr)
        self.tau = tau

    def _t(self, x):
        return torch.as_tensor(np.asarray(x)).to(self.dtype)

    def _critic(self, p, x, tape=None):
        return tuple(_head(p[8 * i + 4:8 * i + 8], _trunk(p[8 * i:8 * i + 4], x), tape, 'critic', f'q{i + 1}', 8 * i + 4) for i in range(2))

    def mu(self, obs):
        return torch.tanh(_head(self.actor[4:8], _trunk(self.actor[0:4], obs), None, 'actor', 'actor', 4))

    def loss(self, batch, tape=None):
        """(L, metrics dict of tensors) on the current parameters."""
        obs, action, reward, discount, next_obs = (self._t(x) for x in batch[:5])
        with torch.no_grad():
            t1, t2 = self._critic(self.critic_target, torch.cat([next_obs, self.mu(next_obs)], -1))
            y1, y2 = reward + discount * t1, reward + discount * t2
        q1, q2 = self._critic(self.critic, torch.cat([obs, action], -1), tape)
        loss = F.mse_loss(q1, y1) + F.mse_loss(q2, y2)
        m = dict(batch_reward=reward.mean(), critic_target_q=(0.5 * (y1 + y2)).mean(), critic_q1=q1.mean(), critic_q2=q2.mean(), critic_loss=loss)
        return loss, m

    def update(self, batch, kink_delta=None, kink_cap=64):
        res = Result()
        tape = []
        loss, m = self.loss(batch, tape)
        res.metrics = {k: v.item() for k, v in m.items()}
        res.critic_grads = backward_with_kinks(res, 'critic', loss, self.critic, self.critic, tape, kink_delta, kink_cap)
        self.opt.step()
        with torch.no_grad():
            for p, tg in zip(self.critic, self.critic_target):
                tg.copy_(self.tau * p + (1 - self.tau) * tg)
        return res

    def value_rows(self, obs):
        """(Q_1, Q_2) at (s, mu(s)) for the rows of obs, float64 numpy arrays: what the value pass reduces."""
        with torch.no_grad():
            o = self._t(obs)
            q1, q2 = self._critic(self.critic, torch.cat([o, self.mu(o)], -1))
        return q1.reshape(-1).double().numpy(), q2.reshape(-1).double().numpy()


def value_dict(q1, q2, returns):
    """FQEAgent.value()'s dict from per-episode float64 Q_1, Q_2 and episode returns (the definitions of agents.fqe_values, restated)."""
    n = len(q1)
    mean = 0.5 * (q1 + q2)
    return {'fqe_value': float(mean.mean()), 'fqe_value_q1': float(q1.mean()), 'fqe_value_q2': float(q2.mean()),
            'fqe_value_stderr': float(mean.std(ddof=1) / np.sqrt(n)) if n > 1 else 0.0, 'fqe_twin_rms': float(np.sqrt(((q1 - q2) ** 2).mean())),
            'behavior_value': float(np.mean(returns)), 'episodes': n}
