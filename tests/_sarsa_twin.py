"""TEST INFRASTRUCTURE: the float64 / float32 autograd twins of a step with the SARSA setting on (exorl_agent_set_sarsa), and the cases the
tests run them on.

SarsaTwin restates oracle.twin64.Twin's step (oracle/twin64.py, Twin._update, kinds 'td3_bc', 'td3', 'crr') with one change: the action the
target critic is fed at s' is the dataset's a' on the rows with next_valid v != 0 and the base step's clipped sample a~' on the others
(batch[5], batch[6]; v all ones when absent). It enters through Twin._sample's 'target' draw, the one place the base forms a~', so the
nets, the actor step, the noise, lambda, the soft update and the kink bookkeeping are the base class's, untouched. SarsaFQETwin does the
same to tests/_fqe_twin.py's FQETwin: a' over mu(s') where v != 0, each net on its own target. Besides the base's results one update()
returns res.metrics['next_valid'], the mean of v.

The cases are tests/_rebrac_twin.py's tables, CASES and TRAJ_CASES, as they stand: shapes, precisions, seeds, batches (batch(c, step): five
tensors, the next action with zeros on invalid rows, next_valid with about one row in four invalid), noise and bars."""
import numpy as np
import torch
import torch.nn.functional as F

import _rebrac_twin as R
import _synth
from _fqe_twin import FQETwin
from _grad_grid import KINK_CAP, MARGIN
from oracle.twin64 import Twin

CASES, TRAJ_CASES, TRAJ_STEPS = R.CASES, R.TRAJ_CASES, R.TRAJ_STEPS
KINK_DELTA = R.KINK_DELTA


def mix(valid, a_next, own):
    """The rule: a' where v != 0, the kind's own target action elsewhere."""
    return torch.where(valid != 0, a_next, own)


class SarsaTwin(Twin):
    def _update(self, batch, step, noise, rand_is_uniform, kink_delta, kink_cap):
        t = lambda x: torch.as_tensor(np.asarray(x)).to(self.dtype)
        self._a_next = t(batch[5])
        self._valid = t(batch[6]).reshape(-1, 1) if len(batch) > 6 else torch.ones(self._a_next.shape[0], 1, dtype=self.dtype)
        res = super()._update(batch[:5], step, noise, rand_is_uniform, kink_delta, kink_cap)
        res.metrics['next_valid'] = self._valid.mean().item()
        return res

    def _sample(self, mu, z, res, tag):
        x = super()._sample(mu, z, res, tag)
        return mix(self._valid, self._a_next, x) if tag == 'target' else x


class SarsaFQETwin(FQETwin):
    def loss(self, batch, tape=None):
        obs, action, reward, discount, next_obs, a_next = (self._t(x) for x in batch[:6])
        valid = self._t(batch[6]).reshape(-1, 1) if len(batch) > 6 else torch.ones_like(reward)
        with torch.no_grad():
            t1, t2 = self._critic(self.critic_target, torch.cat([next_obs, mix(valid, a_next, self.mu(next_obs))], -1))
            y1, y2 = reward + discount * t1, reward + discount * t2
        q1, q2 = self._critic(self.critic, torch.cat([obs, action], -1), tape)
        loss = F.mse_loss(q1, y1) + F.mse_loss(q2, y2)
        m = dict(batch_reward=reward.mean(), critic_target_q=(0.5 * (y1 + y2)).mean(), critic_q1=q1.mean(), critic_q2=q2.mean(), critic_loss=loss,
                 next_valid=valid.mean())
        return loss, m

    def q_rows(self, obs, action):
        """(Q_1, Q_2) at (s, a), float64 numpy arrays: what BehaviorQAgent's value pass reduces."""
        with torch.no_grad():
            q1, q2 = self._critic(self.critic, torch.cat([self._t(obs), self._t(action)], -1))
        return q1.reshape(-1).double().numpy(), q2.reshape(-1).double().numpy()


# ---- the TD3+BC cases: ReBRAC's, with its alpha = 1 / A ---------------------------------------------------------------------------------
def case_id(c):
    return f'sarsa-O{c.O}A{c.A}H{c.H}B{c.B}-{c.precision}'


def make_twin(c, dtype, kind='td3_bc', **kw):
    pa, pc = R.params(c)
    return SarsaTwin(kind, list(pa.values()), list(pc.values()), dtype=dtype, alpha=R.alpha_of(c.A), **kw)


def run_twin(c, dtype, kink_delta=None, critic_after=None):
    return make_twin(c, dtype).update(R.batch(c), 0, *R.noise(c), kink_delta=kink_delta, kink_cap=KINK_CAP, critic_after=critic_after)


def qualify(c):
    """tests/_rebrac_twin.py's qualify on this twin: the reasons the case does not qualify (empty: it does)."""
    r64 = run_twin(c, torch.float64, None if c.bar == 'coarse' else KINK_DELTA[c.precision])
    r32 = run_twin(c, torch.float32)
    bad = []
    for name, (choice, margin) in r64.decisions.items():
        if name.startswith('target_noise') or name.startswith('target_action'):      # decided on every row, used on the v = 0 rows alone
            keep = np.repeat(np.asarray(R.batch(c)[6]) == 0, c.A)
            choice, other, margin = choice[keep], r32.decisions[name][0][keep], margin[keep]
        else:
            other = r32.decisions[name][0]
        if not np.array_equal(choice, other):
            bad.append(f'{name}: twin32 decides differently')
        if margin.size and float(margin.min()) < MARGIN:
            bad.append(f'{name}: margin {float(margin.min()):.2e}')
    if c.bar == 'tight':
        for step in R.STEPS:
            if r64.kinks[step] is None:
                bad.append(f'{step}: |K| = {r64.n_kinks[step]} > {KINK_CAP}')
                continue
            for a, b in zip(r64.relus[step], r32.relus[step]):
                z = a['z']
                far = z.abs() >= KINK_DELTA[c.precision] * z.abs().max()
                if bool((((z > 0) != (b['z'] > 0)) & far).any()):
                    bad.append(f'{step}/{a["name"]}: ReLU masks differ outside the near-kink set')
    return bad


def run_traj(c, dtype):
    """[(metrics, [actor, critic, critic_target parameter arrays]) per step] of the twin over TRAJ_STEPS steps."""
    tw = make_twin(c, dtype)
    ns = _synth.NoiseStream(c.seed + 3)
    out = []
    for step in range(TRAJ_STEPS):
        r = tw.update(R.batch(c, step), step, *R.noise(c, ns))
        out.append((dict(r.metrics), [[p.detach().double().numpy().copy() for p in net] for net in (tw.actor, tw.critic, tw.critic_target)]))
    return out


# ---- the agents under test ---------------------------------------------------------------------------------------------------------------
def make_agent(c, use_tb=True, **kw):
    """OneStepTD3BCAgent of the case's shape and precision with ReBRAC's alpha."""
    from exorl_amd import agents
    args = dict(precision=c.precision)
    args.update(kw)
    return agents.OneStepTD3BCAgent('onestep', (c.O,), (c.A,), 'cuda', 1e-4, c.H, 0.01, 0.2, 1, c.B, 0.3, use_tb, R.alpha_of(c.A), **args)


def make_kind(kind, sarsa, O, A, H, B, use_tb=True, precision='fp32', alpha=2.5):
    """The agent of `kind` ('td3_bc' | 'td3' | 'crr' | 'fqe'): with the setting on (the one-step classes and BehaviorQAgent; TD3 has no class
    of its own: a TD3Agent with the buffer set on its engine, batches through set_next_action or the slots) or the base class."""
    from exorl_amd import agents
    from exorl_amd.agents import _NextActionBatch
    common = dict(precision=precision)
    if kind == 'td3_bc':
        cls = agents.OneStepTD3BCAgent if sarsa else agents.TD3BCAgent
        return cls(kind, (O,), (A,), 'cuda', 1e-4, H, 0.01, 0.2, 1, B, 0.3, use_tb, alpha, **common)
    if kind == 'td3':
        ag = agents.TD3Agent(kind, (O,), (A,), 'cuda', 1e-4, H, 0.01, 0.2, 1, B, 0.3, use_tb, **common)
        if sarsa:
            _NextActionBatch._attach_sarsa(ag)
        return ag
    if kind == 'crr':
        cls = agents.OneStepCRRAgent if sarsa else agents.CRRAgent
        return cls(kind, (O,), (A,), 'cuda', 1e-4, H, 0.01, 4, 'exp', 0.2, 1, B, 0.3, use_tb, **common)
    cls = agents.BehaviorQAgent if sarsa else agents.FQEAgent
    return cls(kind, (O,), (A,), 'cuda', 1e-4, H, 0.01, 1, B, use_tb, **common)
