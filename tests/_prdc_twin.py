"""TEST INFRASTRUCTURE: the float64 / float32 autograd twin of PRDCAgent.update(), a restatement of oracle.twin64.Twin's TD3+BC step
(oracle/twin64.py, Twin._update, kind 'td3_bc') with F.mse_loss(mu, action) replaced by F.mse_loss(mu, a_nn): a_nn is the action of the
table row nearest to [beta * obs | mu(obs)], found by brute force over the case's table in the twin's dtype, and a constant of the actor
step. Everything else (nets, critic step, noise, lambda, soft update, the kink bookkeeping) is the base class's.

The table (N, pitch) holds float32 values [beta * s | a | 0-pad] (tests/_prdc_cases.py builds it as the engine does). The query's
observation part is the float32 product float32(beta) * obs, the engine's own operation, widened; mu and the distances are in the twin's
dtype, d2 = sum_c (q_c - k_c)^2 in the difference form. Besides Twin's results one update() returns
  res.nn_idx    the neighbour of every batch row (int64)
  res.nn_d2     its squared distance (float64 numpy)
  res.decisions['nn']   (nn_idx, relative gap (d2_2nd - d2_1st) / d2_2nd per row; 1.0 where the table has one row)
  res.metrics['nn_dist']  mean sqrt(d2)"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle.twin64 import Result, Twin, _margin_min


def brute_force_nn(q, keys):
    """(idx, d2 of the nearest, relative gap to the second nearest) of every row of q (B, D) among keys (N, D), torch tensors of one dtype;
    ties go to the lowest index."""
    d2 = ((q[:, None, :] - keys[None, :, :]) ** 2).sum(-1) if q.shape[0] * keys.shape[0] * q.shape[1] <= 2 ** 24 else \
        torch.stack([((row[None, :] - keys) ** 2).sum(-1) for row in q])
    best = d2.min(1).values
    idx = (d2 == best[:, None]).long().argmax(1)                 # the first index that attains the minimum
    if keys.shape[0] == 1:
        return idx, best, torch.ones_like(best)
    rest = d2.clone()
    rest[torch.arange(q.shape[0]), idx] = float('inf')
    second = rest.min(1).values
    return idx, best, (second - best) / second.clamp_min(1e-300)


class PRDCTwin(Twin):
    def __init__(self, actor_params, critic_params, keys, obs_dim, beta, **kw):
        super().__init__('td3_bc', actor_params, critic_params, **kw)
        self.keys = np.asarray(keys, np.float32)
        self.O, self.beta = int(obs_dim), np.float32(beta)

    def _update(self, batch, step, noise, rand_is_uniform, kink_delta, kink_cap):
        t = lambda x: torch.as_tensor(np.asarray(x)).to(self.dtype)
        obs32 = np.asarray(batch[0], np.float32)
        obs, action, reward, discount, next_obs = (t(x) for x in batch[:5])
        A = action.shape[1]
        res = Result()
        res.metrics['batch_reward'] = reward.mean().item()
        kw = dict(kink_delta=kink_delta, kink_cap=kink_cap)
        ent = (0.5 + 0.5 * math.log(2 * math.pi) + math.log(self.std)) * A
        zc, za = t(noise[0]), t(noise[1])
        # ---- critic: Twin._update's, the dataset action (td3_bc.py:119-143)
        with torch.no_grad():
            next_action = self._sample(torch.tanh(self._actor_raw(self.actor, next_obs)), zc, res, 'target')
            tq1, tq2 = self._critic(self.critic_target, next_obs, next_action)
            res.decisions['target_min'] = ((tq2 < tq1).reshape(-1).long().numpy(), _margin_min(tq1, tq2).double().numpy())
            target_q = reward + discount * torch.min(tq1, tq2)
        tape = []
        q1, q2 = self._critic(self.critic, obs, action, tape)
        critic_loss = F.mse_loss(q1, target_q) + F.mse_loss(q2, target_q)
        res.critic_grads = self._step(res, 'critic', critic_loss, self.critic, self.critic_opt, tape, **kw)
        res.metrics.update(critic_target_q=target_q.mean().item(), critic_q1=q1.mean().item(), critic_q2=q2.mean().item(),
                           critic_loss=critic_loss.item())
        # ---- actor, against the updated critic; the BC target is the nearest table row's action
        tape = []
        mu = torch.tanh(self._actor_raw(self.actor, obs, tape))
        with torch.no_grad():
            keys = t(self.keys[:, :self.O + A])
            query = torch.cat([t(self.beta * obs32), mu.detach()], 1)
            idx, d2, gap = brute_force_nn(query, keys)
            a_nn = keys[idx, self.O:]
        res.nn_idx, res.nn_d2 = idx.numpy(), d2.double().numpy()
        res.decisions['nn'] = (idx.numpy(), gap.double().numpy())
        pi = self._sample(mu, za, res, 'actor')
        p1, p2 = self._critic(self.critic, obs, pi, tape)
        res.decisions['actor_min'] = ((p2 < p1).reshape(-1).long().numpy(), _margin_min(p1.detach(), p2.detach()).double().numpy())
        q = torch.min(p1, p2)
        actor_loss = -(self.alpha / q.abs().mean().detach()) * q.mean() + F.mse_loss(mu, a_nn)
        res.actor_grads = self._step(res, 'actor', actor_loss, self.actor, self.actor_opt, tape, **kw)
        res.metrics.update(actor_loss=actor_loss.item(), actor_ent=ent, nn_dist=d2.clamp_min(0).sqrt().mean().item())
        self._soft_update()
        return res
