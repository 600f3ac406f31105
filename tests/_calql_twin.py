"""TEST INFRASTRUCTURE: the float64 / float32 autograd twin of a CQL step with Cal-QL set (exorl_agent_set_calql).

CalQLTwin restates oracle.twin64.Twin's CQL step (oracle/twin64.py, Twin._update_cql) with one change: in the critic's (3n + 1) B
re-evaluated rows the policy-action blocks 1 and 2, rows [n B, 3n B) (the actions of pi(s) and pi(s') evaluated at s), enter the
conservative penalty as torch.where(q >= m, q, m), m the row's bound batch[5] (the dataset's return-to-go). It enters through
Twin._critic, on the one call of the step that evaluates (3n + 1) B rows, so the nets, the target, the mse, the Lagrange multiplier, the
actor step, the noise, the soft update and the kink bookkeeping are the base class's, untouched. A bounded entry is a constant of the
critic: torch.where routes it no gradient. An exact tie q == m keeps q and its gradient. Besides the base's results one update() returns
  res.metrics['calql_bound_rate']   bounded entries of both nets / (4 n B)
  res.decisions['calql_bound']      per entry (net, block row, b): 1 where bounded, and the relative margin |q - m| / max(|q|, |m|)
and leaves the pre-bound values of the two blocks in self.policy_q, (2, 2n, B), and the critic loss's gradient with respect to the
(3n + 1) B values of each net in self.dq, two ((3n + 1) B,) arrays (their sums are the gradients of the two heads' last biases)."""
import numpy as np
import torch

from oracle.twin64 import Twin


def bound_rows(q, m, n, B):
    """q ((3n + 1) B, 1), rows k B + b; m (B,). Returns (q with rows [n B, 3n B) replaced by where(q >= m, q, m), the bounded mask of
    those rows (2n B, 1))."""
    lo, hi = n * B, 3 * n * B
    mid, mm = q[lo:hi], m.reshape(1, B).repeat(2 * n, 1).reshape(-1, 1)
    keep = mid >= mm
    return torch.cat([q[:lo], torch.where(keep, mid, mm), q[hi:]], 0), ~keep


class CalQLTwin(Twin):
    def __init__(self, actor_params, critic_params, **kw):
        super().__init__('cql', actor_params, critic_params, **kw)
        self.policy_q = None

    def _update(self, batch, step, noise, rand_is_uniform, kink_delta, kink_cap):
        self._m = torch.as_tensor(np.asarray(batch[5])).to(self.dtype).reshape(-1)
        self._bound = None
        res = super()._update(batch[:5], step, noise, rand_is_uniform, kink_delta, kink_cap)
        choice, margin = self._bound
        res.decisions['calql_bound'] = (choice, margin)
        res.metrics['calql_bound_rate'] = float(choice.mean())
        return res

    def _critic(self, p, obs, action, tape=None):
        q1, q2 = super()._critic(p, obs, action, tape)
        B, n = self._m.shape[0], self.n
        if p is not self.critic or obs.shape[0] != (3 * n + 1) * B:
            return q1, q2
        out, masks, margins = [], [], []
        mm = self._m.reshape(1, B).repeat(2 * n, 1).reshape(-1)
        for q in (q1, q2):
            qh, bounded = bound_rows(q, self._m, n, B)
            mid = q[n * B:3 * n * B].detach().reshape(-1)
            rel = (mid - mm).abs() / torch.maximum(mid.abs(), mm.abs()).clamp_min(1e-300)
            out.append(qh)
            masks.append(bounded.reshape(-1).long().numpy())
            margins.append(torch.where(torch.isinf(mm), torch.full_like(rel, float('inf')), rel).double().numpy())
        self.policy_q = torch.stack([q[n * B:3 * n * B].detach().reshape(2 * n, B) for q in (q1, q2)])
        self.dq = [None, None]
        if q1.requires_grad:
            for i, q in enumerate((q1, q2)):
                q.register_hook(lambda g, i=i: self.dq.__setitem__(i, g.detach().double().reshape(-1).numpy().copy()))
        self._bound = (np.concatenate(masks), np.concatenate(margins))
        return tuple(out)
