"""ORACLE (test infrastructure only — never imported by the product path).

torch-autograd twins of the offline state agents' update(), dtype selectable: td3_bc, td3, ddpg (states), bc, crr (identity /
indicator / exp) and cql (with or without the Lagrange weight). Same step as oracle/agents.py (numpy float32, hand-derived
backward) and as the reference's agent.update() (td3_bc.py:119-189, td3.py:117-186, ddpg.py:240-328, bc.py:78-110,
crr.py:121-196, cql.py:152-263), but with the gradients left to autograd and the arithmetic in float64 when asked: the reference
the gradient-grid tests hold the kernels to. Pinned by tests/test_twin64.py against the reference's recorded float64 runs
(tests/golden/full_*.json) and, in float32, against the oracle.

Besides the metrics one update() returns what a tight comparison of gradients needs:
  * the critic step's and the actor step's gradients separately (the reference leaves the actor step's backward accumulated in the
    critic's .grad; the engine keeps the critic step's gradient);
  * the step's discrete decisions with the margin each was taken by (which net is the min, clipped noise, clamped actions, CRR's
    indicator / exp clip, CQL's clamps);
  * every pre-ReLU tensor in each loss's graph with d loss / d (ReLU output), and — for the elements within kink_delta * max|z| of
    the kink — the exact change of the step's gradient if that one element's ReLU derivative flipped.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

LN_EPS = 1e-5
CLAMP = 1.0 - 1e-6            # TruncatedNormal._clamp (utils.py:132-138)
KINDS = ('td3_bc', 'td3', 'ddpg', 'bc', 'crr', 'cql')


def uniform_from_normal64(z):
    """U(-1,1) from the normal noise stream by the probability integral transform, in float64 (tools/gen_golden.py routes
    Tensor.uniform_ this way; oracle.agents.uniform_from_normal is this rounded to float32)."""
    u = 0.5 * (1.0 + np.vectorize(math.erf)(np.asarray(z, np.float64) / math.sqrt(2.0)))
    return -1.0 + 2.0 * u


def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


class _LinearBf16(torch.autograd.Function):
    """nn.Linear with every matrix product taken on operands rounded to bf16 (8 significant bits), forward, dgrad and wgrad: what
    the plain-bf16 mode's number format alone does to a step, whatever the kernel. Products accumulate in the twin's dtype."""

    @staticmethod
    def forward(ctx, x, W, b):
        ctx.save_for_backward(x, W)
        return _bf16(x) @ _bf16(W).T + b

    @staticmethod
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        return _bf16(dy) @ _bf16(W), _bf16(dy).T @ _bf16(x), dy.sum(0)


_EMULATE_BF16 = [False]          # set by Twin(bf16_operands=True) around its update()


def _linear(x, W, b):
    return _LinearBf16.apply(x, W, b) if _EMULATE_BF16[0] else F.linear(x, W, b)


def _trunk(p, x):
    return torch.tanh(F.layer_norm(_linear(x, p[0], p[1]), (p[0].shape[0],), p[2], p[3], LN_EPS))


def _head(p, h, tape, net, name, first):
    """Linear ReLU Linear; `first` = index of W1 in the net's parameter list (b1 = first + 1)."""
    z = _linear(h, p[0], p[1])
    a = torch.relu(z)
    if tape is not None and a.requires_grad:
        a.retain_grad()
        tape.append(dict(net=net, name=name, w1=first, b1=first + 1, z=z, a=a))
    return F.linear(a, p[2], p[3])


def _normal_log_prob(x, mu, std):
    var = std * std
    log_std = torch.log(std) if torch.is_tensor(std) else math.log(std)
    return -((x - mu) ** 2) / (2 * var) - log_std - math.log(math.sqrt(2 * math.pi))


def _margin_min(q1, q2):
    return ((q1 - q2).abs() / torch.maximum(q1.abs(), q2.abs()).clamp_min(1e-300)).reshape(-1)


def backward_with_kinks(res, step, loss, all_params, params, tape, kink_delta, kink_cap):
    """loss.backward() with the bookkeeping a tight comparison needs, shared by every twin (this file, oracle/intr64.py). Clears the
    .grad of all_params, returns the gradients of `params` (float64 numpy, None where a tensor gets none) and fills res.relus[step],
    res.n_kinks[step] and res.kinks[step] from the tape of pre-ReLU tensors: dict(net, name, w1, b1, z, a) with `a` retaining its grad."""
    for p in all_params:
        p.grad = None
    loss.backward(retain_graph=kink_delta is not None)
    grads = [None if p.grad is None else p.grad.detach().double().numpy().copy() for p in params]
    res.relus[step] = [dict(net=r['net'], name=r['name'], w1=r['w1'], b1=r['b1'], z=r['z'].detach(),
                            da=r['a'].grad.detach() if r['a'].grad is not None else torch.zeros_like(r['z'])) for r in tape]
    if kink_delta is not None:
        found = []
        for r, rec in zip(tape, res.relus[step]):
            z = rec['z']
            idx = (z.abs() < kink_delta * z.abs().max()).nonzero()
            found += [(r, rec, int(m), int(c)) for m, c in idx.tolist()]
        res.n_kinks[step] = len(found)
        res.kinks[step] = None
        if len(found) <= kink_cap:
            res.kinks[step] = []
            for r, rec, m, c in found:
                gz = torch.autograd.grad(r['z'][m, c], params, retain_graph=True, allow_unused=True)
                # on in this arithmetic (z > 0): a flip removes the element's path; off: a flip adds it
                f = -1.0 if float(rec['z'][m, c]) > 0 else 1.0
                da = float(rec['da'][m, c])
                D = [None if g is None else (f * da * g.detach().double()).numpy() for g in gz]
                res.kinks[step].append(dict(net=rec['net'], name=rec['name'], w1=rec['w1'], b1=rec['b1'], row=m, unit=c,
                                            z=float(rec['z'][m, c]), D=D))
    return grads


class Result:
    """metrics: dict of floats. critic_grads / actor_grads: lists of float64 numpy arrays in parameters() order (None for a net the
    step has no gradient for). decisions: name -> (int64 numpy array of the choices, float64 numpy array of relative margins).
    relus: step ('critic' | 'actor') -> list of dict(net, name, w1, b1, z, da) with z the pre-ReLU tensor and da = d loss / d relu(z).
    kinks: step -> list of dict(net, name, w1, b1, row, unit, z, D) for the elements of K(kink_delta), D = the change of the step's
    gradient tensors (list of float64 numpy arrays, None where a tensor gets none) if that element's derivative flipped; None when
    |K| exceeds kink_cap. n_kinks: step -> |K|."""

    def __init__(self):
        self.metrics, self.critic_grads, self.actor_grads = {}, None, None
        self.decisions, self.relus, self.kinks, self.n_kinks = {}, {}, {}, {}


class Twin:
    def __init__(self, kind, actor_params, critic_params=None, dtype=torch.float64, lr=1e-4, tau=0.01, stddev=0.2, stddev_clip=0.3,
                 alpha=None, num_value_samples=10, weight_func='indicator', n_samples=3, use_critic_lagrange=False,
                 target_cql_penalty=5.0, bf16_operands=False):
        """actor_params / critic_params: lists of arrays in the reference's parameters() order (oracle.agents.param_shapes).
        alpha: TD3+BC's 2.5 / CQL's 0.01 when None. bf16_operands: the first-layer and hidden-layer products (the ones the plain-bf16
        mode runs on bf16 MFMA operands) take bf16-rounded operands (_LinearBf16) — the format's own error, for choosing the sizes at
        which a direction bar on plain-bf16 gradients means something."""
        assert kind in KINDS, kind
        self.kind, self.dtype, self.bf16_operands = kind, dtype, bf16_operands
        leaf = lambda w: torch.tensor(np.asarray(w, np.float64), dtype=dtype, requires_grad=True)
        self.actor = [leaf(w) for w in actor_params]
        self.actor_opt = torch.optim.Adam(self.actor, lr=lr)
        self.critic = None
        if kind != 'bc':
            self.critic = [leaf(w) for w in critic_params]
            self.critic_target = [p.detach().clone() for p in self.critic]
            self.critic_opt = torch.optim.Adam(self.critic, lr=lr)
        self.tau, self.std, self.clip = tau, stddev, stddev_clip
        self.alpha = alpha if alpha is not None else (0.01 if kind == 'cql' else 2.5)
        self.n_value, self.weight_func, self.n = num_value_samples, weight_func, n_samples
        self.lagrange, self.target_penalty = use_critic_lagrange, target_cql_penalty
        if kind == 'cql':
            self.log_actor_alpha = torch.zeros(1, dtype=dtype, requires_grad=True)
            self.actor_alpha_opt = torch.optim.Adam([self.log_actor_alpha], lr=lr)
            self.log_critic_alpha = torch.zeros(1, dtype=dtype, requires_grad=True)
            self.critic_alpha_opt = torch.optim.Adam([self.log_critic_alpha], lr=lr)

    # ---- nets -------------------------------------------------------------------------------------------------------------
    def _actor_raw(self, p, obs, tape=None):
        return _head(p[4:8], _trunk(p[0:4], obs), tape, 'actor', 'actor', 4)

    def _critic(self, p, obs, action, tape=None):
        x = torch.cat([obs, action], -1)
        if self.kind == 'ddpg':                 # shared trunk, heads Q1 / Q2 (ddpg.py:79-123)
            h = _trunk(p[0:4], x)
            return _head(p[4:8], h, tape, 'critic', 'q1', 4), _head(p[8:12], h, tape, 'critic', 'q2', 8)
        return tuple(_head(p[8 * i + 4:8 * i + 8], _trunk(p[8 * i:8 * i + 4], x), tape, 'critic', f'q{i + 1}', 8 * i + 4) for i in range(2))

    def _sample(self, mu, z, res, tag):
        """TruncatedNormal(mu, std).sample(clip): clipped noise, value clamped to +-(1 - 1e-6), gradient straight through."""
        eps = z * self.std
        if self.clip is not None:
            if res is not None:
                res.decisions[f'{tag}_noise_clipped'] = ((eps.abs() > self.clip).reshape(-1).long().numpy(),
                                                         ((eps.abs() - self.clip).abs() / self.clip).reshape(-1).double().numpy())
            eps = eps.clamp(-self.clip, self.clip)
        x = mu + eps
        xd = x.detach()
        if res is not None:
            res.decisions[f'{tag}_action_clamped'] = ((xd.abs() > CLAMP).reshape(-1).long().numpy(),
                                                      (xd.abs() - CLAMP).abs().reshape(-1).double().numpy())
        return x - xd + xd.clamp(-CLAMP, CLAMP)

    # ---- one optimiser step with the bookkeeping -----------------------------------------------------------------------------
    def _step(self, res, step, loss, params, opt, tape, kink_delta, kink_cap):
        grads = backward_with_kinks(res, step, loss, self.actor + (self.critic or []), params, tape, kink_delta, kink_cap)
        opt.step()
        if step == 'critic' and self._critic_after is not None:
            with torch.no_grad():
                for p, w in zip(self.critic, self._critic_after):
                    p.copy_(torch.as_tensor(np.asarray(w, np.float64)).to(self.dtype).reshape(p.shape))
        return grads

    def _soft_update(self):
        with torch.no_grad():
            for p, t in zip(self.critic, self.critic_target):
                t.copy_(self.tau * p + (1 - self.tau) * t)

    def update(self, batch, step, *noise, rand_is_uniform=False, kink_delta=None, kink_cap=64, critic_after=None):
        """noise: (noise_critic, noise_actor) — CRR's second block is (B * num_value_samples, A); none for BC; for CQL the five blocks
        (z_next, z_rand, z_cur, z_nxt, z_actor) of OracleCQL.update, z_rand standard normal unless rand_is_uniform.
        critic_after: critic parameters to continue with after the critic's optimiser step instead of this twin's own. The actor step
        differentiates through the UPDATED critic, and Adam's first step moves every weight by +-lr according to the sign of its
        gradient alone: an implementation whose critic gradient differs in the sign of rounding-noise entries (or by one accepted ReLU
        flip, which moves a whole W1 row) hands its actor step a critic that differs by 2 lr there. To compare the actor step's
        gradients tightly the twin has to take that step from the same critic."""
        self._critic_after = critic_after
        _EMULATE_BF16[0] = self.bf16_operands
        try:
            return self._update(batch, step, noise, rand_is_uniform, kink_delta, kink_cap)
        finally:
            _EMULATE_BF16[0] = False

    def _update(self, batch, step, noise, rand_is_uniform, kink_delta, kink_cap):
        t = lambda x: torch.as_tensor(np.asarray(x)).to(self.dtype)
        obs, action, reward, discount, next_obs = (t(x) for x in batch[:5])
        res = Result()
        res.metrics['batch_reward'] = reward.mean().item()
        kw = dict(kink_delta=kink_delta, kink_cap=kink_cap)
        if self.kind == 'cql':
            return self._update_cql(res, obs, action, reward, discount, next_obs, noise, rand_is_uniform, kw)
        A = action.shape[1]
        ent = (0.5 + 0.5 * math.log(2 * math.pi) + math.log(self.std)) * A
        if self.kind == 'bc':                                                                        # bc.py:78-95
            tape = []
            mu = torch.tanh(self._actor_raw(self.actor, obs, tape))
            loss = -_normal_log_prob(action, mu, self.std).sum(-1, keepdim=True).mean()
            res.actor_grads = self._step(res, 'actor', loss, self.actor, self.actor_opt, tape, **kw)
            res.metrics.update(actor_loss=loss.item(), actor_ent=ent)
            return res
        zc, za = t(noise[0]), t(noise[1])
        # ---- critic (td3_bc.py:119-143 / td3.py:117-141 / ddpg.py:240-268 / crr.py:144-168)
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
        # ---- actor, against the updated critic
        tape = []
        mu = torch.tanh(self._actor_raw(self.actor, obs, tape))
        if self.kind == 'crr':                                                                       # crr.py:121-142,170-196
            n, B = self.n_value, obs.shape[0]
            with torch.no_grad():
                acts = self._sample(mu.detach().repeat_interleave(n, 0), za, res, 'value')           # 'b x -> (b n) x'
                v1, v2 = self._critic(self.critic, obs.repeat_interleave(n, 0), acts)
                V = torch.min(v1, v2).view(B, n, 1).mean(1)
                d1, d2 = self._critic(self.critic, obs, action)
                qd = torch.min(d1, d2)
                adv = qd - V
                rel = (adv.abs() / torch.maximum(qd.abs(), V.abs()).clamp_min(1e-300)).reshape(-1).double().numpy()
                if self.weight_func == 'identity':
                    w = adv
                elif self.weight_func == 'indicator':
                    w = torch.sign(torch.relu(adv))
                    res.decisions['crr_indicator'] = ((adv > 0).reshape(-1).long().numpy(), rel)
                else:
                    e = torch.exp(adv)
                    w = e.clamp(0.0, 20.0)
                    res.decisions['crr_exp_clipped'] = ((e > 20.0).reshape(-1).long().numpy(), ((e - 20.0).abs() / 20.0).reshape(-1).double().numpy())
            actor_loss = -(_normal_log_prob(action, mu, self.std).sum(-1, keepdim=True) * w).mean()
        else:
            pi = self._sample(mu, za, res, 'actor')
            p1, p2 = self._critic(self.critic, obs, pi, tape)
            res.decisions['actor_min'] = ((p2 < p1).reshape(-1).long().numpy(), _margin_min(p1.detach(), p2.detach()).double().numpy())
            q = torch.min(p1, p2)
            if self.kind == 'td3_bc':                                                                # td3_bc.py:152-156
                actor_loss = -(self.alpha / q.abs().mean().detach()) * q.mean() + F.mse_loss(mu, action)
            else:
                actor_loss = -q.mean()
            if self.kind == 'ddpg':                                                                  # ddpg.py:276,289
                res.metrics['actor_logprob'] = _normal_log_prob(pi.detach(), mu.detach(), self.std).sum(-1, keepdim=True).mean().item()
        res.actor_grads = self._step(res, 'actor', actor_loss, self.actor, self.actor_opt, tape, **kw)
        res.metrics.update(actor_loss=actor_loss.item(), actor_ent=ent)
        self._soft_update()
        return res

    # ---- CQL (cql.py:152-263): tanh-Gaussian actor with 2A outputs, TD loss + conservative penalty over 3n re-evaluations ----------
    def _policy(self, obs, tape=None):
        raw = self._actor_raw(self.actor, obs, tape)
        A = raw.shape[1] // 2
        ls = raw[:, A:]
        return torch.tanh(raw[:, :A]), torch.exp(ls.clamp(-10.0, 2.0)), ls

    def _update_cql(self, res, obs, action, reward, discount, next_obs, noise, rand_is_uniform, kw):
        t = lambda x: torch.as_tensor(np.asarray(x)).to(self.dtype)
        z_next, z_rand, z_cur, z_nxt, z_actor = noise
        B, A = action.shape
        n = self.n
        rand = t(z_rand if rand_is_uniform else uniform_from_normal64(z_rand))
        z_next, z_cur, z_nxt, z_actor = t(z_next), t(z_cur).reshape(n, B, A), t(z_nxt).reshape(n, B, A), t(z_actor)
        with torch.no_grad():
            mu_n, std_n, _ = self._policy(next_obs)
            mu_c, std_c, _ = self._policy(obs)
            tq1, tq2 = self._critic(self.critic_target, next_obs, torch.tanh(mu_n + std_n * z_next))
            res.decisions['target_min'] = ((tq2 < tq1).reshape(-1).long().numpy(), _margin_min(tq1, tq2).double().numpy())
            y = reward + discount * torch.min(tq1, tq2)
            acts = torch.cat([rand.reshape(n * B, A), torch.tanh(mu_c[None] + std_c[None] * z_cur).reshape(n * B, A),
                              torch.tanh(mu_n[None] + std_n[None] * z_nxt).reshape(n * B, A), action], 0)
            obs_all = torch.cat([obs.repeat(3 * n, 1), obs], 0)                                      # sample-major rows
        tape = []
        q1a, q2a = self._critic(self.critic, obs_all, acts, tape)
        q1, q2 = q1a[3 * n * B:], q2a[3 * n * B:]
        lse = sum(torch.logsumexp(qa.reshape(3 * n + 1, B, 1), 0).mean() for qa in (q1a, q2a))
        penalty = lse - q1.mean() - q2.mean()
        alpha_c = self.alpha
        if self.lagrange:                                                                            # cql.py:201-213
            ea = torch.exp(self.log_critic_alpha)
            res.decisions['critic_alpha_clamped'] = (((ea < 0.0) | (ea > 1e6)).long().numpy(), ((ea - 1e6).abs() / 1e6).detach().double().numpy())
            self.critic_alpha_opt.zero_grad(set_to_none=True)
            (-0.5 * ea.clamp(0.0, 1e6) * (penalty.detach() - self.target_penalty)).sum().backward()
            self.critic_alpha_opt.step()
            alpha_c = torch.exp(self.log_critic_alpha).clamp(0.0, 1e6).detach()[0]
        mse = F.mse_loss(q1, y) + F.mse_loss(q2, y)
        critic_loss = mse + alpha_c * penalty
        res.critic_grads = self._step(res, 'critic', critic_loss, self.critic, self.critic_opt, tape, **kw)
        res.metrics.update(critic_target_q=y.mean().item(), critic_q1=q1.mean().item(), critic_q2=q2.mean().item(),
                           critic_loss=critic_loss.item(), critic_cql=penalty.item(), critic_cql_logsum=lse.item())
        # ---- actor (cql.py:234-263), against the updated critic
        tape = []
        mu, std, ls = self._policy(obs, tape)
        lsd = ls.detach()
        res.decisions['log_std_clamped'] = (((lsd < -10.0) | (lsd > 2.0)).reshape(-1).long().numpy(),
                                            torch.minimum((lsd + 10.0).abs() / 10.0, (lsd - 2.0).abs() / 2.0).reshape(-1).double().numpy())
        x = mu + std * z_actor
        yact = torch.tanh(x)
        log_pi = _normal_log_prob(x, mu, std) - 2.0 * (math.log(2.0) - x - F.softplus(-2.0 * x))     # TanhTransform, utils.py:152-196
        mean_lp = log_pi.mean()
        alpha_loss = -(self.log_actor_alpha * (mean_lp.detach() - A)).sum()                          # target entropy -A
        self.actor_alpha_opt.zero_grad(set_to_none=True)
        alpha_loss.backward()
        self.actor_alpha_opt.step()
        alpha = torch.exp(self.log_actor_alpha).detach()[0]
        p1, p2 = self._critic(self.critic, obs, yact, tape)
        res.decisions['actor_min'] = ((p2 < p1).reshape(-1).long().numpy(), _margin_min(p1.detach(), p2.detach()).double().numpy())
        actor_loss = alpha * mean_lp - torch.min(p1, p2).mean()
        res.actor_grads = self._step(res, 'actor', actor_loss, self.actor, self.actor_opt, tape, **kw)
        res.metrics.update(actor_loss=actor_loss.item(), actor_ent=-mean_lp.item(), actor_alpha=alpha.item(), actor_alpha_loss=alpha_loss.item())
        self._soft_update()
        return res
