"""ORACLE (test infrastructure only — never imported by the product path).

torch-autograd twins of the eight reward-free modules' step, dtype selectable: rnd (state rows and encodings), icm, icm_apt, disagreement,
diayn, aps, smm and proto. Same step as oracle/intr.py and oracle/proto.py (numpy float32, hand-derived backward) and as the reference's
update_<module> / compute_intr_reward (rnd.py:79-108, icm.py:64-92, icm_apt.py:86-110, disagreement.py:64-90, diayn.py:78-127,
aps.py:147-175, smm.py:27-112,173-246, proto.py:14-157; utils.RMS / utils.PBE utils.py:257-319), with the gradients left to autograd and
the arithmetic in float64 when asked: the reference tests/test_gpu_intr_grid.py holds the module kernels to. Pinned by
tests/test_intr64.py against the reference's recorded trajectories (tests/golden/tiny_*.npz) and, in float32, against the oracle's
gradients. The randomness fed from outside (Proto's Categorical uniforms, SMM's epsilon) is an input: batch['u'], batch['eps'].

One update() is one optimiser step (train = 1) from parameters in parameters() order (oracle.intr.intr_param_shapes; Disagreement:
4 tensors per model) and returns a Result (oracle/twin64.py) whose
  grads      trainable gradient tensors, float64 numpy, then d loss / d (input rows) where the module hands one back (`dobs`): the tensors
             a ReLU flip's direction D_k spans (backward_with_kinks), in this order
  dobs       what exorl_intr_batch.dobs_out receives: d/d obs (icm, icm_apt, disagreement, rnd on encodings), d/d next_obs (diayn, aps)
  state      what the step leaves outside the parameters: RND's BatchNorm running mean / var / count
  decisions  name -> (choices, float64 margins): RND's clamp, the DIAYN / SMM arg-max hit, SMM's dist > 1 branch
SMM's reward is made of the losses of the step itself (smm.py:217-246), so its update() computes it and reward() hands it back. Proto's
reward() also returns the picks (with the distance of u * total from the nearest CDF boundary, relative to total, as margin) and leaves
queue / queue_ptr; proto_target_after() is predictor_target's Polyak step.
reward(batch, params_after=) is compute_intr_reward under the updated module: it takes the parameters the run under test produced (as
Twin.update(critic_after=) does, and for the same reason: Adam's first step moves every weight by +-lr on the sign of its gradient
alone). It returns (reward rows, metrics in the EXORL_IM_* slots, decisions) and steps the RMS. reward(batch) alone from the initial
parameters is the train = 0 entry."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from .twin64 import Result, backward_with_kinks

KINDS = ('rnd', 'icm', 'icm_apt', 'disagreement', 'diayn', 'aps', 'smm', 'proto')
IM_LOSS, IM_INTR_REWARD, IM_EXTR_REWARD, IM_RMS_MEAN, IM_RMS_STD, IM_ACC, IM_ENT_REWARD, IM_SF_REWARD = range(8)      # EXORL_IM_*
BN_EPS, LN_EPS = 1e-5, 1e-5


class IntrTwin:
    def __init__(self, kind, params, dtype=torch.float64, lr=1e-4, scale=1.0, clip_val=5.0, n_models=5, knn_k=12, knn_avg=True, knn_rms=True,
                 knn_clip=0.0, encoded=False, num_protos=0, queue_size=0, tau=0.1, target_tau=0.05, sp_lr=1e-3, vae_lr=1e-2, vae_beta=0.5,
                 state_ent_coef=1.0, latent_ent_coef=1.0, latent_cond_ent_coef=1.0, goal=(150.0, 75.0)):
        assert kind in KINDS, kind
        self.kind, self.dtype, self.lr, self.scale, self.clip, self.n_models, self.encoded = kind, dtype, lr, scale, clip_val, n_models, encoded
        self.knn = dict(k=knn_k, avg=knn_avg, rms=knn_rms, clip=knn_clip)
        self.p = [self._leaf(w) for w in params]
        self.n_train = 6 if kind == 'rnd' else len(self.p)                  # RND's target is frozen (rnd.py:41-42)
        self.lrs = [lr] * self.n_train
        if kind == 'smm':                                                   # two optimisers: z_pred_net, then the VAE (smm.py:114-121)
            self.lrs = [sp_lr] * 6 + [vae_lr] * 14
            self.beta, self.coefs, self.goal = vae_beta, (state_ent_coef, latent_ent_coef, latent_cond_ent_coef), goal
        if kind == 'proto':                                                 # p: predictor, projector, protos; predictor_target is a copy
            self.tau, self.ttau = tau, target_tau
            self.pt = [self.p[0].detach().clone(), self.p[1].detach().clone()]
            self.queue = torch.zeros(queue_size, self.p[0].shape[0], dtype=dtype)
            self.queue_ptr = 0
        self.M, self.S, self.n = self._t(0.0), self._t(1.0), 1e-4           # utils.RMS
        self.bn = None                                                       # BatchNorm1d(affine=False): running mean, var, batches
        self.decisions = {}

    def _t(self, x):
        return torch.as_tensor(np.asarray(x, np.float64)).to(self.dtype)

    def _leaf(self, w):
        return torch.tensor(np.asarray(w, np.float64), dtype=self.dtype, requires_grad=True)

    # ---- nets ---------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _mlp(p, x, tape, name, first, final_tanh=False, relu_last=False):
        """Linear (ReLU Linear)* [Tanh]; p = [W, b] * L; `first` = index of p[0] in the module's parameter list. relu_last: p ends with
        a (None, None) pair standing for the missing last Linear, i.e. every Linear is followed by a ReLU (the VAE's encoder)."""
        n = len(p) // 2
        for l in range(n):
            if p[2 * l] is None:
                break
            z = F.linear(x, p[2 * l], p[2 * l + 1])
            if l < n - 1:
                x = torch.relu(z)
                if tape is not None:
                    x.retain_grad()
                    tape.append(dict(net='module', name=f'{name}.{l}', w1=first + 2 * l, b1=first + 2 * l + 1, z=z, a=x))
            else:
                x = torch.tanh(z) if final_tanh else z
        return x

    def _bn_clamp(self, obs):
        """BatchNorm1d in training mode (rnd.py:24-26,49-50), stepping the running statistics, then clamp(+-clip)."""
        B, O = obs.shape
        mean, var = obs.mean(0), obs.var(0, unbiased=False)
        if self.bn is None:
            self.bn = [torch.zeros(O, dtype=self.dtype), torch.ones(O, dtype=self.dtype), 0]
        self.bn[0] = 0.9 * self.bn[0] + 0.1 * mean
        self.bn[1] = 0.9 * self.bn[1] + 0.1 * var * (B / max(B - 1, 1))
        self.bn[2] += 1
        x = (obs - mean) / torch.sqrt(var + BN_EPS)
        self.decisions['rnd_clamped'] = ((x.abs() > self.clip).reshape(-1).long().numpy(),
                                         ((x.abs() - self.clip).abs() / self.clip).reshape(-1).double().numpy())
        return x.clamp(-self.clip, self.clip)

    def _rnd_err(self, p, obs, next_obs, tape):
        if self.encoded:                 # rnd.py:26-27,35-39: the predictor on the agent's encoding, the frozen target on the frozen encoder's
            xp, xt = obs, next_obs
        else:
            xp = xt = self._bn_clamp(obs.detach())
        pred = self._mlp(p[:6], xp, tape, 'predictor', 0)
        with torch.no_grad():
            targ = self._mlp(p[6:], xt, None, 'target', 6)
        return ((targ - pred) ** 2).mean(-1, keepdim=True)

    def _apt_trunk(self, p, x):
        return torch.tanh(F.layer_norm(F.linear(x, p[0], p[1]), (p[0].shape[0],), p[2], p[3], LN_EPS))

    def _icm_errors(self, p, o, action, n_tgt, tape):
        """forward error ||n_tgt - f([o | a])|| and inverse error ||a - tanh(g([o | n_tgt]))|| per row (icm.py:28-45)."""
        nhat = self._mlp(p[0:4], torch.cat([o, action], -1), tape, 'forward_net', self._first)
        fe = torch.norm(n_tgt - nhat, dim=-1, p=2, keepdim=True)
        if tape is None:
            return fe, None
        ahat = self._mlp(p[4:8], torch.cat([o, n_tgt], -1), tape, 'backward_net', self._first + 4, final_tanh=True)
        return fe, torch.norm(action - ahat, dim=-1, p=2, keepdim=True)

    # ---- SMM (smm.py:27-112,173-246) ---------------------------------------------------------------------------------------------
    def _smm_losses(self, b, res, tape):
        """update_vae on [obs | z] and update_pred on obs; the reward is made of their per-row losses. Returns (the obs leaf, loss)."""
        p, zp, v = self.p, self.p[:6], self.p[6:]
        leaf = b['obs'].requires_grad_()
        z = b['skill']
        x = torch.cat([leaf, z], 1)
        B, W = x.shape
        h = self._mlp(v[0:4] + [None, None], x, tape, 'vae.enc', 6, relu_last=True)
        mu, lv = F.linear(h, v[4], v[5]), F.linear(h, v[6], v[7])
        code = b['eps'] * torch.exp(0.5 * lv) + mu
        out = self._mlp(v[8:14], code, tape, 'vae.dec', 14)
        sq = (x - out) ** 2
        kle = (-0.5 * (1 + lv - mu ** 2 - torch.exp(lv)).sum(1)).mean()
        loss_vae = self.beta * kle + sq.mean()
        h_s_z = sq.sum(1).detach()
        logits = self._mlp(zp, leaf.detach(), tape, 'z_pred_net', 0)
        lab = z.argmax(1)
        h_z_s = F.cross_entropy(logits, lab, reduction='none')
        loss_pred = h_z_s.mean()
        ld = logits.detach()
        if ld.shape[1] > 1:
            top = ld.topk(2, dim=1).values
            res.decisions['smm_hit'] = ((ld.argmax(1) == lab).long().numpy(), ((top[:, 0] - top[:, 1]) / ld.abs().amax(1).clamp_min(1e-300)).double().numpy())
        sec, lec, lcec = self.coefs
        m = {IM_LOSS: loss_vae.item(), 5: loss_pred.item(), 4: (sec * h_s_z).mean().item(), 6: (lcec * h_z_s.detach()).mean().item()}
        r = sec * h_s_z + lec * math.log(z.shape[1]) + lcec * h_z_s.detach()
        m[3] = m[7] = 0.0
        if not self.encoded:             # the 1-D log p* broadcasts to (B, B): per sample its batch mean, its variance in each critic's loss
            o = leaf.detach()
            dist = torch.sqrt((o[:, 0] - self.goal[0]) ** 2 + (o[:, 1] - self.goal[1]) ** 2)
            res.decisions['smm_dist_gt_1'] = ((dist > 1.0).long().numpy(), (dist - 1.0).abs().double().numpy())
            lps = torch.log(torch.where(dist > 1.0, 1.0 / dist, torch.ones_like(dist)))
            m[3], m[7] = lps.mean().item(), lps.var(unbiased=False).item()
            r = r + lps.mean()
        m[IM_INTR_REWARD] = r.mean().item()
        if 'extr' in b:
            m[IM_EXTR_REWARD] = b['extr'].mean().item()
        self._smm_reward = (r.double().numpy().reshape(-1), m, {})
        return leaf, loss_vae + loss_pred

    # ---- Proto (proto.py:14-157) ---------------------------------------------------------------------------------------------------
    @staticmethod
    def _sinkhorn(S):
        """proto.py:14-31 on S = scores / tau, (B, P) -> (B, P)."""
        Q = torch.exp(S - S.max()).T
        Q = Q / Q.sum()
        r, c = 1.0 / Q.shape[0], 1.0 / Q.shape[1]
        for _ in range(3):
            Q = Q * (r / Q.sum(1))[:, None]
            Q = Q * (c / Q.sum(0))[None, :]
        return (Q / Q.sum(0, keepdim=True)).T

    def _proto_loss(self, b, tape):
        p = self.p
        with torch.no_grad():            # normalize_protos (proto.py:98-101): in place, in front of the step
            p[6].copy_(F.normalize(p[6], dim=1, p=2))
        leaf = b['obs'].requires_grad_()
        s = self._mlp(p[2:6], F.linear(leaf, p[0], p[1]), tape, 'projector', 2)
        logp = F.log_softmax(F.normalize(s, dim=1, p=2) @ p[6].T / self.tau, dim=1)
        with torch.no_grad():
            t = F.normalize(F.linear(b['next_obs'], self.pt[0], self.pt[1]), dim=1, p=2)
            q = self._sinkhorn(t @ p[6].T / self.tau)
        return leaf, -(q * logp).sum(1).mean()

    def _proto_reward(self, p, b, dec):
        """compute_intr_reward (proto.py:103-124): the candidates drawn by inverse CDF over the batch (serial in float64, as
        torch.multinomial's cumulative table), written into the queue; the reward is the k-th smallest distance to the queue's rows."""
        C, z, cdf = self.proto_cdf(p, b['next_obs'])
        thr = b['u'].double().reshape(-1, 1) * cdf[:, -1:]
        cand = (cdf <= thr).sum(1).clamp_max(cdf.shape[1] - 1)
        dec['proto_picks'] = (cand.numpy().copy(), ((cdf - thr).abs().min(1).values / cdf[:, -1]).numpy())
        P = C.shape[0]
        self.queue[self.queue_ptr:self.queue_ptr + P] = z[cand]
        self.queue_ptr = (self.queue_ptr + P) % self.queue.shape[0]
        self.last_z = z.double().numpy()
        d = torch.norm(z[:, None, :] - self.queue[None, :, :], dim=-1, p=2)
        return d.topk(self.knn['k'], dim=1, largest=False, sorted=True).values[:, -1:]

    @torch.no_grad()
    def proto_cdf(self, p, next_obs):
        """(normalised protos, z = l2norm(predictor(next_obs)), the (P, B) cumulative table of softmax over the batch, float64)."""
        C = F.normalize(p[6], dim=1, p=2)
        z = F.normalize(F.linear(next_obs, p[0], p[1]), dim=1, p=2)
        return C, z, torch.cumsum(torch.softmax((z @ C.T).T, dim=1).double(), 1)

    def proto_target_after(self, predictor_after):
        """predictor_target after its Polyak step towards the updated predictor (proto.py:202-203), float64."""
        return [self.ttau * np.asarray(a, np.float64).reshape(t.shape) + (1 - self.ttau) * t.double().numpy() for a, t in zip(predictor_after, self.pt)]

    # ---- one optimiser step ---------------------------------------------------------------------------------------------------
    def update(self, batch, kink_delta=None, kink_cap=64):
        """batch: dict of arrays obs, action, next_obs, skill (the ones the kind reads)."""
        k, p = self.kind, self.p
        b = {n: self._t(v) for n, v in batch.items() if v is not None}
        res, tape, leaf = Result(), [], None
        self.decisions = res.decisions
        if k == 'rnd':
            if self.encoded:
                leaf = b['obs'].requires_grad_()
            loss = self._rnd_err(p, b['obs'], b.get('next_obs'), tape).mean()
        elif k in ('icm', 'icm_apt'):
            leaf = b['obs'].requires_grad_()
            self._first = 0
            o, n_tgt = leaf, b['next_obs']
            if k == 'icm_apt':           # the same trunk on both; next_obs's representation is also the forward model's target (icm_apt.py:33-50)
                self._first = 4
                o, n_tgt = self._apt_trunk(p[:4], leaf), self._apt_trunk(p[:4], b['next_obs'])
            fe, be = self._icm_errors(p[self._first:], o, b['action'], n_tgt, tape)
            loss = fe.mean() + be.mean()
        elif k == 'disagreement':
            leaf = b['obs'].requires_grad_()
            x = torch.cat([leaf, b['action']], -1)
            errs = [torch.norm(b['next_obs'] - self._mlp(p[4 * m:4 * m + 4], x, tape, f'ensemble.{m}', 4 * m), dim=-1, p=2) for m in range(self.n_models)]
            loss = torch.stack(errs, 1).mean()
        elif k == 'diayn':
            leaf = b['next_obs'].requires_grad_()
            logits = self._mlp(p, leaf, tape, 'skill_pred_net', 0)
            lab = b['skill'].argmax(1)
            loss = F.cross_entropy(logits, lab)
            top = logits.detach().topk(2, dim=1).values if logits.shape[1] > 1 else None
            hit = logits.detach().argmax(1) == lab
            if top is not None:
                res.decisions['diayn_hit'] = (hit.long().numpy(), ((top[:, 0] - top[:, 1]) / logits.detach().abs().amax(1).clamp_min(1e-300)).double().numpy())
            res.metrics[IM_ACC] = float(hit.sum()) / logits.shape[0]
        elif k == 'smm':
            leaf, loss = self._smm_losses(b, res, tape)
        elif k == 'proto':
            leaf, loss = self._proto_loss(b, tape)
        else:                            # aps.py:147-159
            leaf = b['next_obs'].requires_grad_()
            f = self._mlp(p, leaf, tape, 'state_feat_net', 0)
            loss = -(b['skill'] * F.normalize(f, dim=1)).sum(1).mean()
        params = p[:self.n_train] + ([leaf] if leaf is not None else [])
        grads = backward_with_kinks(res, 'module', loss, params + p[self.n_train:], params, tape, kink_delta, kink_cap)
        res.grads, res.dobs = grads, (grads[-1] if leaf is not None else None)
        res.metrics[IM_LOSS] = loss.item()
        if k == 'smm':                   # slot 0 is loss_vae alone; the step's other slots are the reward's
            res.metrics.update(self._smm_reward[1])
        res.state = {}
        if self.bn is not None:
            res.state['bn'] = (self.bn[0].double().numpy().copy(), self.bn[1].double().numpy().copy(), self.bn[2])
        return res

    # ---- compute_intr_reward ----------------------------------------------------------------------------------------------------
    def _rms(self, x):
        """utils.RMS.__call__ (utils.py:264-276): Chan update with the batch mean and unbiased variance."""
        bs = x.shape[0]
        delta = x.mean(0) - self.M
        var = x.var(0, unbiased=True) if bs > 1 else torch.zeros_like(delta)
        self.S = (self.S * self.n + var * bs + delta ** 2 * self.n * bs / (self.n + bs)) / (self.n + bs)
        self.M = self.M + delta * bs / (self.n + bs)
        self.n += bs
        return self.M, self.S

    def _pbe(self, rep, dec):
        """utils.PBE.__call__ (utils.py:279-319) with source = target = rep."""
        kn = self.knn
        d = torch.norm(rep[:, None, :] - rep[None, :, :], dim=-1, p=2)
        r = d.topk(kn['k'], dim=1, largest=False, sorted=True).values
        r = r.reshape(-1, 1) if kn['avg'] else r[:, -1:].reshape(-1, 1)
        if kn['rms']:
            r = r / self._rms(r)[0]
        if kn['clip'] >= 0.0:
            v = r - kn['clip']
            # a row's distance to itself is exactly 0 in every arithmetic (difference form) and clips to 0 whatever the clip: no decision
            margin = torch.where(r == 0, torch.full_like(v, float('inf')), v.abs() / r.abs().max().clamp_min(1e-300))
            dec['pbe_clipped'] = ((v < 0).reshape(-1).long().numpy(), margin.reshape(-1).double().numpy())
            r = v.clamp_min(0.0)
        if kn['avg']:
            r = r.reshape(rep.shape[0], kn['k']).mean(1, keepdim=True)
        return torch.log(r + 1.0)

    @torch.no_grad()
    def reward(self, batch, params_after=None):
        k = self.kind
        p = self.p if params_after is None else [self._t(w).reshape(q.shape) for w, q in zip(params_after, self.p)]
        b = {n: self._t(v) for n, v in batch.items() if v is not None}
        m, dec = {}, {}
        self.decisions = dec
        if k == 'smm':
            return self._smm_reward
        if k == 'proto':
            r = self._proto_reward(p, b, dec)
        elif k == 'rnd':                                                                           # rnd.py:98-103
            err = self._rnd_err(p, b['obs'], b.get('next_obs'), None)
            _, var = self._rms(err)
            r = self.scale * err / (torch.sqrt(var) + 1e-8)
        elif k == 'icm':                                                                         # icm.py:86-92
            self._first = 0
            r = torch.log(self._icm_errors(p, b['obs'], b['action'], b['next_obs'], None)[0] * self.scale + 1.0)
        elif k == 'icm_apt':                                                                     # icm_apt.py:106-110
            r = self._pbe(self._apt_trunk(p[:4], b['obs']), dec)
        elif k == 'disagreement':                                                                # disagreement.py:35-47
            x = torch.cat([b['obs'], b['action']], -1)
            preds = torch.stack([self._mlp(p[4 * i:4 * i + 4], x, None, '', 0) for i in range(self.n_models)], 0)
            r = preds.var(0, unbiased=True).mean(-1, keepdim=True)
        elif k == 'diayn':                                                                       # diayn.py:94-105
            lsm = F.log_softmax(self._mlp(p, b['next_obs'], None, '', 0), dim=1)
            S = b['skill'].shape[1]
            r = (lsm.gather(1, b['skill'].argmax(1, keepdim=True)) - math.log(1 / S)) * self.scale
        else:                                                                                    # aps.py:161-168
            rep = self._mlp(p, b['next_obs'], None, '', 0)
            ent = self._pbe(rep, dec)
            sf = (b['skill'] * (rep / torch.norm(rep, dim=1, keepdim=True))).sum(1, keepdim=True)
            m[IM_ENT_REWARD], m[IM_SF_REWARD] = ent.mean().item(), sf.mean().item()
            r = ent + sf
        m[IM_INTR_REWARD] = r.mean().item()
        if 'extr' in b:
            m[IM_EXTR_REWARD] = b['extr'].mean().item()
        if k in ('rnd', 'icm_apt', 'aps'):
            m[IM_RMS_MEAN], m[IM_RMS_STD] = float(self.M), math.sqrt(float(self.S))
        self.decisions = {}
        return r.double().numpy().reshape(-1), m, dec

    def adam_first_step(self, grads):
        """The parameters after Adam's first step from zero moments (m_hat = g, v_hat = g^2), in this twin's dtype."""
        out = [q.detach().clone() for q in self.p]
        for q, g, lr in zip(out, grads[:self.n_train], self.lrs):
            g = self._t(g)
            q -= lr * g / (g.abs() + 1e-8)
        return [q.double().numpy() for q in out]

    def rms_state(self):
        return float(self.M), float(self.S), float(self.n)

    def bn_state(self):
        return None if self.bn is None else (self.bn[0].double().numpy().copy(), self.bn[1].double().numpy().copy(), self.bn[2])
