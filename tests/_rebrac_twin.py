"""TEST INFRASTRUCTURE: the float64 / float32 autograd twin of ReBRACAgent.update() and the cases the tests run it on.

The twin restates oracle.twin64.Twin's TD3+BC step (oracle/twin64.py, Twin._update, kind 'td3_bc') with one term more in the critic target,
    y = r + D (min_i Q'_i(s', a~') - critic_beta v sum_j (a~'_j - a'_j)^2),
a~' the clipped target-policy sample the base step draws, a' the dataset's next action and v its validity (batch[5], batch[6]); y is formed
under no_grad, as the base's. Everything else (nets, actor step, noise, lambda, soft update, the kink bookkeeping) is the base class's.
Besides Twin's results one update() returns
  res.metrics['critic_penalty']   mean of p = v sum_j (a~' - a')_j^2      res.metrics['next_valid']   mean of v
  res.actor_grads_after_critic    the .grad of every actor parameter right after the critic loss's backward (all None: y is detached)

One case = one update() from seeded parameters, batch, next action and noise; columns of CASES as in tests/_prdc_cases.py. The shapes are
two, (O, A, H, B) = (5, 1, 8, 7) (A = 1: the un-fused sampling path) and (24, 6, 128, 257) (a second, one-row chunk of the row
kernel; no tiling by 64 or 128, so bf16x3 and bf16x6 split inside the GEMM), at fp32, bf16x3 and bf16x6. Plain bf16 needs 8 | H and 8 | B
(the library refuses both shapes) and a batch at which the format itself keeps the direction bar (tests/_grad_grid.py): its case is the
grid's plain-bf16 TD3+BC shape, (24, 6, 256, 1024), coarse."""
from collections import namedtuple
from functools import lru_cache

import numpy as np
import torch
import torch.nn.functional as F

import _synth
from _grad_grid import KINK_CAP, KINK_DELTA, MARGIN
from oracle.agents import param_shapes
from oracle.twin64 import Result, Twin, _margin_min


class ReBRACTwin(Twin):
    def __init__(self, actor_params, critic_params, critic_beta, **kw):
        super().__init__('td3_bc', actor_params, critic_params, **kw)
        self.critic_beta = float(critic_beta)

    def _step(self, res, step, loss, params, opt, tape, kink_delta, kink_cap):
        grads = super()._step(res, step, loss, params, opt, tape, kink_delta, kink_cap)
        if step == 'critic':          # backward_with_kinks cleared every .grad before loss.backward(): what the actor holds now came through y
            res.actor_grads_after_critic = [p.grad for p in self.actor]
        return grads

    def _update(self, batch, step, noise, rand_is_uniform, kink_delta, kink_cap):
        t = lambda x: torch.as_tensor(np.asarray(x)).to(self.dtype)
        obs, action, reward, discount, next_obs, a_next = (t(x) for x in batch[:6])
        valid = t(batch[6]).reshape(-1, 1) if len(batch) > 6 else torch.ones_like(reward)
        A = action.shape[1]
        res = Result()
        res.metrics['batch_reward'] = reward.mean().item()
        kw = dict(kink_delta=kink_delta, kink_cap=kink_cap)
        ent = (0.5 + 0.5 * np.log(2 * np.pi) + np.log(self.std)) * A
        zc, za = t(noise[0]), t(noise[1])
        # ---- critic: Twin._update's with the penalty in the target
        with torch.no_grad():
            next_action = self._sample(torch.tanh(self._actor_raw(self.actor, next_obs)), zc, res, 'target')
            tq1, tq2 = self._critic(self.critic_target, next_obs, next_action)
            res.decisions['target_min'] = ((tq2 < tq1).reshape(-1).long().numpy(), _margin_min(tq1, tq2).double().numpy())
            pen = valid * ((next_action - a_next) ** 2).sum(-1, keepdim=True)
            target_q = reward + discount * (torch.min(tq1, tq2) - self.critic_beta * pen)
        tape = []
        q1, q2 = self._critic(self.critic, obs, action, tape)
        critic_loss = F.mse_loss(q1, target_q) + F.mse_loss(q2, target_q)
        res.critic_grads = self._step(res, 'critic', critic_loss, self.critic, self.critic_opt, tape, **kw)
        res.metrics.update(critic_target_q=target_q.mean().item(), critic_q1=q1.mean().item(), critic_q2=q2.mean().item(),
                           critic_loss=critic_loss.item(), critic_penalty=pen.mean().item(), next_valid=valid.mean().item())
        # ---- actor, against the updated critic: the base's
        tape = []
        mu = torch.tanh(self._actor_raw(self.actor, obs, tape))
        pi = self._sample(mu, za, res, 'actor')
        p1, p2 = self._critic(self.critic, obs, pi, tape)
        res.decisions['actor_min'] = ((p2 < p1).reshape(-1).long().numpy(), _margin_min(p1.detach(), p2.detach()).double().numpy())
        q = torch.min(p1, p2)
        actor_loss = -(self.alpha / q.abs().mean().detach()) * q.mean() + F.mse_loss(mu, action)
        res.actor_grads = self._step(res, 'actor', actor_loss, self.actor, self.actor_opt, tape, **kw)
        res.metrics.update(actor_loss=actor_loss.item(), actor_ent=ent)
        self._soft_update()
        return res


def rebrac_actor_loss(mu, action, q, actor_bc_coef):
    """ReBRAC's actor loss as the paper writes it: beta_a sum_j (pi(s) - a)_j^2 - Q / mean|Q|, means over the batch."""
    return (actor_bc_coef * ((mu - action) ** 2).sum(-1, keepdim=True) - q / q.abs().mean().detach()).mean()


def td3bc_actor_loss(mu, action, q, alpha):
    """TD3+BC's, as Twin._update forms it (td3_bc.py:152-156)."""
    return -(alpha / q.abs().mean().detach()) * q.mean() + F.mse_loss(mu, action)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
Case = namedtuple('Case', 'O A H B precision seed bar why')
ACTOR_BC, CRITIC_BC = 1.0, 1.0
KINK_DELTA = dict(KINK_DELTA, bf16x6=KINK_DELTA['fp32'])       # bf16x6 is fp32-grade: fp32's delta and fp32's bar (tests/_prdc_cases.py)

CASES = [
    Case(5, 1, 8, 7, 'fp32', 100, 'tight', 'A=1: sample_actions2 writes the sample the row kernel reads; one ragged chunk of 7 rows'),
    Case(24, 6, 128, 257, 'fp32', 200, 'tight', 'A=6: the fused sampling epilogue; 257 rows: a second chunk of one row'),
    Case(5, 1, 8, 7, 'bf16x3', 300, 'tight', 'in-GEMM split'),
    Case(24, 6, 128, 257, 'bf16x3', 400, 'tight', 'in-GEMM split (257 does not tile by 64)'),
    Case(5, 1, 8, 7, 'bf16x6', 500, 'tight', 'in-GEMM split'),
    Case(24, 6, 128, 257, 'bf16x6', 600, 'tight', 'in-GEMM split (257 does not tile by 128)'),
    Case(24, 6, 256, 1024, 'bf16', 704, 'coarse', 'plain bf16: direction only, at the gradient grid\'s plain-bf16 TD3+BC shape'),
]


def case_id(c):
    return f'rebrac-O{c.O}A{c.A}H{c.H}B{c.B}-{c.precision}'


def alpha_of(A, actor_bc=ACTOR_BC):
    return 1.0 / (actor_bc * A)


def params(c):
    ash, csh = param_shapes('td3_bc', c.O, c.A, c.H)
    return _synth.synth_params(ash, c.seed), _synth.synth_params(csh, c.seed + 1)


def batch(c, step=0):
    """synth_batch's five tensors, then the dataset's next action (uniform in [-1, 1), zeros on invalid rows as the gather writes them) and
    next_valid: about one row in four invalid, the first always valid and the last always invalid where there are two."""
    b = _synth.synth_batch(c.seed + 2, step, c.B, c.O, c.A)
    rs = np.random.RandomState((c.seed + 4) * 100003 + step)
    valid = (rs.uniform(size=c.B) >= 0.25).astype(np.float32)
    valid[0] = 1.0
    if c.B > 1:
        valid[-1] = 0.0
    a_next = (rs.uniform(-1.0, 1.0, (c.B, c.A)) * valid[:, None]).astype(np.float32)
    return b + (a_next, valid)


def noise(c, ns=None):
    ns = ns or _synth.NoiseStream(c.seed + 3)
    return [ns.draw((c.B, c.A)), ns.draw((c.B, c.A))]


def make_twin(c, dtype, critic_beta=CRITIC_BC, **kw):
    pa, pc = params(c)
    return ReBRACTwin(list(pa.values()), list(pc.values()), critic_beta, dtype=dtype, alpha=alpha_of(c.A), **kw)


def run_twin(c, dtype, kink_delta=None, critic_after=None):
    return make_twin(c, dtype).update(batch(c), 0, *noise(c), kink_delta=kink_delta, kink_cap=KINK_CAP, critic_after=critic_after)


@lru_cache(maxsize=4)
def twin_pair(c):
    return run_twin(c, torch.float64, None if c.bar == 'coarse' else KINK_DELTA[c.precision]), run_twin(c, torch.float32)


STEPS = ('critic', 'actor')


def steps_of(res):
    return [(s, getattr(res, f'{s}_grads')) for s in STEPS]


def qualify(c):
    """tests/_prdc_cases.py's: the reasons the case does not qualify (empty: it does). The float32 and float64 twins take the same discrete
    decisions, each with a float64 margin >= MARGIN, and (tight cases) the near-kink set of every step is within KINK_CAP with the two
    twins' ReLU masks agreeing outside it."""
    r64, r32 = twin_pair(c)
    bad = []
    for name, (choice, margin) in r64.decisions.items():
        if not np.array_equal(choice, r32.decisions[name][0]):
            bad.append(f'{name}: twin32 decides differently')
        if float(margin.min()) < MARGIN:
            bad.append(f'{name}: margin {float(margin.min()):.2e}')
    if c.bar == 'tight':
        for step in STEPS:
            if r64.kinks[step] is None:
                bad.append(f'{step}: |K| = {r64.n_kinks[step]} > {KINK_CAP}')
                continue
            for a, b in zip(r64.relus[step], r32.relus[step]):
                z = a['z']
                far = z.abs() >= KINK_DELTA[c.precision] * z.abs().max()
                if bool((((z > 0) != (b['z'] > 0)) & far).any()):
                    bad.append(f'{step}/{a["name"]}: ReLU masks differ outside the near-kink set')
    return bad


# ---- the three-step trajectories (tests/test_gpu_rebrac.py): batches batch(c, step), noise NoiseStream(seed + 3) in step order, parameters
# after every step against the float64 twin, at both shapes and every precision (plain bf16 at its own shape, as above). The bars:
#   fp32, bf16x6   element by element, max(traj_bar, 2 E32): E32 = the float32 CPU twin's largest parameter error at that step (traj_e32;
#                  measured on the case itself, recorded in TRAJ_E32 and profiles/rebrac_step.txt). At (5, 1, 8, 7) the float32 twin uses a
#                  third of traj_bar, at (24, 6, 128, 257) 0.94 of it at the first step: that case needs the measured bar.
#   bf16x3         per net, tests/test_gpu_dp.py's bf16x3 rule for three steps (tests/test_gpu_iql_dp.py, tests/test_gpu_rebrac_dp.py): at
#                  most 0.5 % of the elements further than 2e-6 + 1e-4 |p| from the twin's, none further than 6.5e-4 after the third step
#                  (a third and two thirds of that after the first and second). Adam divides the gradient by its own magnitude, so an
#                  element whose gradient is rounding noise moves by +-lr either way: 2 lr a step, 6e-4 over three, is the largest honest
#                  difference, and no element-wise bar below it can be derived for this precision.
#   bf16           per net and step, the direction of the parameter change since the start: 1 - cosine <= twice what the number format
#                  alone costs, measured with the float64 CPU twin on bf16-rounded operands (Twin(bf16_operands=True), no kernel involved;
#                  traj_bf16_cos, recorded in TRAJ_BF16_COS and profiles/rebrac_step.txt), and the same ceiling. Adam's first step is
#                  sign(g) lr: every element whose gradient is smaller than the format's error (2.5e-2 of the tensor's largest, one-step
#                  cases above) may change sign, and the format alone leaves cosine 0.986 on the actor after one step, 0.9973 after three.
#                  The 0.999 that tests/test_gpu_agent.py and smoke() ask of plain bf16 is a bar for H = B = 1024 over more steps: it was
#                  tried here first and neither the engine (0.985905 on the actor after the first step) nor the format-only CPU twin
#                  (0.986026) meets it, to the same digits, so it says nothing about the kernels at this shape and step count.
# Metrics at every step at the precision's one-step tolerance (tests/test_gpu_grad_grid.py).
TRAJ = Case(5, 1, 8, 7, 'fp32', 40, 'tight', 'three steps')
TRAJ_STEPS = 3
TRAJ_CASES = [TRAJ._replace(precision=p) for p in ('fp32', 'bf16x6', 'bf16x3')] + \
             [Case(24, 6, 128, 257, p, 41, 'tight', 'three steps') for p in ('fp32', 'bf16x6', 'bf16x3')] + \
             [Case(24, 6, 256, 1024, 'bf16', 42, 'coarse', 'three steps')]
TRAJ_E32 = {(5, 1, 8, 7): (7.29e-08, 1.26e-07, 1.34e-07), (24, 6, 128, 257): (2.05e-07, 2.07e-07, 2.27e-07)}      # traj_e32, per step
# traj_bf16_cos of the plain-bf16 case: [step][actor, critic, critic_target] cosine of the bf16-operand twin's parameter change with twin64's
TRAJ_BF16_COS = ((0.986026, 0.993267, 0.993267), (0.994924, 0.997704, 0.996443), (0.997315, 0.998827, 0.997780))
TRAJ_METRIC_REL ={'fp32': 2e-5, 'bf16x6': 2e-5, 'bf16x3': 1e-4, 'bf16': 3e-2}
DP_RULE = dict(rel=1e-4, abs=2e-6, share=5e-3, ceiling=6.5e-4)


def traj_bar(p64, step):
    """tests/_prdc_cases.py's: an Adam update moves a parameter by lr m^ / (sqrt(v^) + eps); a relative error of 1e-3 in that ratio is
    1e-3 lr, storing the parameter rounds it once; both add up over the steps."""
    return (step + 1) * (2.0 ** -23 * max(float(np.abs(p64).max()), 1.0) + 1e-3 * 1e-4)


def run_traj(c, dtype):
    """[(metrics, [actor, critic, critic_target parameter arrays]) per step] of the twin over TRAJ_STEPS steps."""
    tw = make_twin(c, dtype)
    ns = _synth.NoiseStream(c.seed + 3)
    out = []
    for step in range(TRAJ_STEPS):
        r = tw.update(batch(c, step), step, *noise(c, ns))
        out.append((dict(r.metrics), [[p.detach().double().numpy().copy() for p in net] for net in (tw.actor, tw.critic, tw.critic_target)]))
    return out


def traj_bf16_cos(c):
    """[step][actor, critic, critic_target]: cosine between the parameter change since the start of the float64 twin on bf16-rounded
    operands and of the float64 twin, after each step of the case's trajectory: what the plain-bf16 format alone does to the direction."""
    flat = lambda ts: np.concatenate([t.detach().double().numpy().reshape(-1) for t in ts])
    t64, tb = make_twin(c, torch.float64), make_twin(c, torch.float64, bf16_operands=True)
    nets = ('actor', 'critic', 'critic_target')
    start = {nm: flat(getattr(t64, nm)) for nm in nets}
    ns = _synth.NoiseStream(c.seed + 3)
    out = []
    for step in range(TRAJ_STEPS):
        b, z = batch(c, step), noise(c, ns)
        t64.update(b, step, *z)
        tb.update(b, step, *z)
        row = []
        for nm in nets:
            dg, dw = flat(getattr(tb, nm)) - start[nm], flat(getattr(t64, nm)) - start[nm]
            row.append(float(dg @ dw / (np.linalg.norm(dg) * np.linalg.norm(dw))))
        out.append(tuple(row))
    return tuple(out)


def traj_e32(c):
    """The float32 CPU twin's largest parameter error against the float64 twin after each step of the case's trajectory."""
    c = c._replace(precision='fp32')
    return tuple(max(float(np.abs(a - b).max()) for n64, n32 in zip(p64, p32) for a, b in zip(n64, n32))
                 for (_, p64), (_, p32) in zip(run_traj(c, torch.float64), run_traj(c, torch.float32)))


# ---- the agent under test
def make_agent(c, use_tb=True, critic_bc_coef=CRITIC_BC, **kw):
    from exorl_amd import agents
    args = dict(precision=c.precision)
    args.update(kw)
    return agents.ReBRACAgent('rebrac', (c.O,), (c.A,), 'cuda', 1e-4, c.H, 0.01, 0.2, 1, c.B, 0.3, use_tb, ACTOR_BC, critic_bc_coef, **args)


def load_params(ag, c):
    pa, pc = params(c)
    ag.actor.load_state_dict({k: torch.from_numpy(v) for k, v in pa.items()})
    ag.critic.load_state_dict({k: torch.from_numpy(v) for k, v in pc.items()})
    ag.critic_target.load_state_dict(ag.critic.state_dict())
    return ag
