"""Thin object wrappers over the C ABI handles (exorl_agent_t, exorl_replay_t).

torch is used here only as plumbing: it owns the device workspace (so parameters can be exposed as
torch tensors for state_dict / pickling / torch.distributed all-reduce) and provides the stream.
All arithmetic happens in libexorl_hip.so.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L

KIND = {'td3_bc': L.AGENT_TD3_BC, 'td3': L.AGENT_TD3, 'bc': L.AGENT_BC, 'ddpg': L.AGENT_DDPG, 'crr': L.AGENT_CRR, 'cql': L.AGENT_CQL,
        'aps': L.AGENT_APS}
KIND_BEYOND_REFERENCE = {'iql': L.AGENT_IQL, 'fqe': L.AGENT_FQE, 'prdc': L.AGENT_PRDC}        # kinds the reference does not have; KIND stays the reference's seven
PRECISION = {'fp32': L.PREC_F32, 'f32': L.PREC_F32, 'bf16': L.PREC_BF16, 'bf16x3': L.PREC_BF16X3, 'bf16x6': L.PREC_BF16X6}
METRIC_KEYS = {L.M_BATCH_REWARD: 'batch_reward', L.M_CRITIC_TARGET_Q: 'critic_target_q', L.M_CRITIC_Q1: 'critic_q1',
               L.M_CRITIC_Q2: 'critic_q2', L.M_CRITIC_LOSS: 'critic_loss', L.M_ACTOR_LOSS: 'actor_loss',
               L.M_ACTOR_LOGPROB: 'actor_logprob'}


def kind_id(name):
    """EXORL_AGENT_* of an agent kind by name: the one lookup, over the reference's kinds and the ones beyond it."""
    return KIND[name] if name in KIND else KIND_BEYOND_REFERENCE[name]


def _require_gpu(device):
    if not torch.cuda.is_available():
        raise L.ExorlError('exorl_amd needs a HIP device (torch.cuda.is_available() is False); there is no CPU path')
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise L.ExorlError(f"exorl_amd agents run on the GPU only; got device={device!r}")
    return dev


class _Phased:
    """What the engines with phased calls share: the library handle over a torch-owned workspace with its tensor views (exorl_<prefix>_*
    for prefix agent / intr / pixel_agent), and the choice between a call's one-call form and its phases under torch.distributed."""
    world_size, rank, comm = 1, None, None

    def _create(self, prefix, cfg):
        """self.h = exorl_<prefix>_create(cfg) on a zeroed workspace of exorl_<prefix>_workspace_bytes(cfg), aligned to 256 bytes; the
        workspace is a torch tensor so that parameters can be exposed as tensors (state_dict, pickling, all-reduce)."""
        self.lib, self.cfg, self._prefix = L.load(), cfg, prefix
        nbytes = self._fn('workspace_bytes')(C.byref(cfg))
        if nbytes == 0:
            raise L.ExorlError(self.lib.exorl_last_error().decode())
        with torch.cuda.device(self.device):
            self.workspace = torch.zeros(nbytes + 256, dtype=torch.uint8, device=self.device)
            base = self.workspace.data_ptr()
            off = (-base) % 256
            handle = C.c_void_p()
            L.check(self._fn('create')(C.byref(cfg), base + off, nbytes, C.byref(handle)))
        self.h = handle
        self._f32 = self.workspace[off:off + nbytes].view(torch.float32)

    def _fn(self, name):
        return getattr(self.lib, f'exorl_{self._prefix}_{name}')

    def __del__(self):
        h, self.h = getattr(self, 'h', None), None
        if h:
            self._fn('destroy')(h)

    # ---- views of library-laid-out memory as torch tensors ------------------------------------------
    def _view(self, ptr, numel):
        off = (ptr - self._f32.data_ptr()) // 4
        return self._f32[off:off + numel]

    def _net(self, net):
        return () if net is None else (net,)        # the module engine has one net and its calls take no net argument

    def num_tensors(self, net=None):
        n = C.c_int32()
        L.check(self._fn('num_tensors')(self.h, *self._net(net), C.byref(n)))
        return n.value

    def tensor(self, net, index, what=L.T_PARAM):
        p, r, c = C.c_void_p(), C.c_int64(), C.c_int64()
        L.check(self._fn('tensor')(self.h, *self._net(net), index, what, C.byref(p), C.byref(r), C.byref(c)))
        v = self._view(p.value, r.value * c.value)
        return v.view(r.value, c.value) if c.value > 1 else v

    def exchange(self, xid):
        """(device tensor, op) of exchange `xid` (exorl_intr_exchange, exorl_pixel_agent_exchange): op L.XCHG_SUM -> sum-all-reduce the
        tensor in place; L.XCHG_GATHER -> the tensor is (world_size, count), rank r's row being its slot, all-gathered in rank order."""
        p, n, dt, op = C.c_void_p(), C.c_int64(), C.c_int32(), C.c_int32()
        L.check(self._fn('exchange')(self.h, xid, C.byref(p), C.byref(n), C.byref(dt), C.byref(op)))
        slots = self.world_size if op.value == L.XCHG_GATHER else 1
        words = 2 if dt.value == L.XCHG_F64 else 1
        t = self._view(p.value, slots * n.value * words)
        if dt.value == L.XCHG_F64:
            t = t.view(torch.float64)
        return (t.view(slots, n.value) if op.value == L.XCHG_GATHER else t), op.value

    def _run(self, one_call, steps, *a, **k):
        """one_call(*a, **k) on one rank, else its phases steps(*a, **k) with the exchanges run over torch.distributed."""
        if self.world_size == 1:
            return one_call(*a, **k)
        return run_steps(steps(*a, **k), self.rank)


class AgentEngine(_Phased):
    def __init__(self, kind, obs_dim, act_dim, hidden_dim, batch, lr=1e-4, tau=0.01, alpha=2.5, stddev_clip=0.3,
                 precision='fp32', world_size=1, seed=0, device='cuda', num_value_samples=10, weight_func='indicator',
                 n_samples=3, use_critic_lagrange=False, target_cql_penalty=5.0, sf_dim=0):
        self.device = _require_gpu(device)
        self.kind = kind
        cfg = L.AgentCfg(kind_id(kind), obs_dim, act_dim, hidden_dim, batch, PRECISION[precision], world_size, sf_dim,
                              lr, tau, alpha, stddev_clip if stddev_clip is not None else 0.0, seed, num_value_samples,
                              L.CRR_WEIGHT[weight_func], n_samples, int(bool(use_critic_lagrange)), target_cql_penalty, 0)
        self.obs_dim, self.act_dim, self.hidden_dim, self.batch = obs_dim, act_dim, hidden_dim, batch
        self.world_size = world_size
        self._create('agent', cfg)
        self.has_critic = kind != 'bc'
        self.has_value = kind == 'iql'
        self.has_alpha = kind == 'cql'
        self._eval = self._fqe_value = None       # the evaluation and value windows (set_eval, set_fqe_value): attached on first use
        self._rebrac = None                       # the ReBRAC buffer (set_rebrac): the caller's, kept alive here while set
        self._sarsa = None                        # the SARSA buffer (set_sarsa), likewise; never both
        self._calql = None                        # Cal-QL's buffer (set_calql), likewise

    # -- pickling support, as PixelEngine's: everything that defines the training state, as CPU data
    def export_state(self):
        nets = [L.NET_ACTOR] + ([L.NET_CRITIC, L.NET_CRITIC_TARGET] if self.has_critic else []) + ([L.NET_VALUE] if self.has_value else [])
        whats = lambda net: [L.T_PARAM] if net == L.NET_CRITIC_TARGET else [L.T_PARAM, L.T_ADAM_M, L.T_ADAM_V]
        st = {'flat': {net: {w: self.flat(net, w).cpu() for w in whats(net)} for net in nets}, 'opt_steps': self.opt_steps()}
        if self.has_alpha:
            st['cql_alpha'] = self.cql_alpha_state().tolist()
        return st

    def import_state(self, st):
        for net, bufs in st['flat'].items():
            for w, t in bufs.items():
                self.flat(net, w).copy_(t)
        self.set_opt_steps(*st['opt_steps'])
        if 'cql_alpha' in st:
            self.set_cql_alpha_state(*st['cql_alpha'])
        self.params_changed(sync_target=False)

    def flat(self, net, what=L.T_PARAM):
        p, n = C.c_void_p(), C.c_int64()
        L.check(self.lib.exorl_agent_flat(self.h, net, what, C.byref(p), C.byref(n)))
        return self._view(p.value, n.value)

    def stats(self):
        p, n = C.c_void_p(), C.c_int64()
        L.check(self.lib.exorl_agent_stats_buffer(self.h, C.byref(p), C.byref(n)))
        return self._view(p.value, n.value)

    def batch_slots(self):
        out = L.BatchOut()
        L.check(self.lib.exorl_agent_batch_slots(self.h, C.byref(out)))
        return out

    # ---- operations ----------------------------------------------------------------------------------
    def params_changed(self, sync_target=False):
        L.check(self.lib.exorl_agent_params_changed(self.h, int(sync_target), L.current_stream()))

    def set_batch(self, obs, action, reward, discount, next_obs):
        ts = [self._dev(x) for x in (obs, action, reward, discount, next_obs)]
        B = self.batch
        for t, n in zip(ts, (B * self.obs_dim, B * self.act_dim, B, B, B * self.obs_dim)):
            if t.numel() != n:
                raise L.ExorlError(f'batch tensor has {t.numel()} elements, expected {n}')
        L.check(self.lib.exorl_agent_set_batch(self.h, *[t.data_ptr() for t in ts], L.current_stream()))
        self._keep = ts

    def _dev(self, x):
        t = torch.as_tensor(x)
        if t.dtype != torch.float32:
            t = t.float()
        return t.to(self.device, non_blocking=True).contiguous()

    def update(self, stddev, noise_critic=None, noise_actor=None):
        nc = self._dev(noise_critic) if noise_critic is not None else None
        na = self._dev(noise_actor) if noise_actor is not None else None
        L.check(self.lib.exorl_agent_update(self.h, stddev, L.ptr(nc), L.ptr(na), L.current_stream()))
        self._keep_noise = (nc, na)

    def update_phase(self, phase, stddev, noise_critic=None, noise_actor=None):
        nc = self._dev(noise_critic) if noise_critic is not None else None
        na = self._dev(noise_actor) if noise_actor is not None else None
        L.check(self.lib.exorl_agent_update_phase(self.h, phase, stddev, L.ptr(nc), L.ptr(na), L.current_stream()))
        self._keep_noise = (nc, na)

    def exchange(self, xid):
        """The buffer of exchange `xid` (L.AGENT_XCHG_*); every one is sum-all-reduced in place."""
        if xid == L.AGENT_XCHG_STATS:
            return self.stats()
        return self.flat({L.AGENT_XCHG_CRITIC_GRAD: L.NET_CRITIC, L.AGENT_XCHG_ACTOR_GRAD: L.NET_ACTOR, L.AGENT_XCHG_VALUE_GRAD: L.NET_VALUE}[xid],
                         L.T_GRAD)

    def update_steps(self, stddev, noise_critic=None, noise_actor=None):
        """update() as its phases, for run_steps: yields the (buffer, op) to exchange across the ranks before the next phase. The library
        names the phases and the exchange behind each (exorl_agent_update_plan): the critic's gradients, the batch statistic of the
        kinds that have one (TD3+BC's lambda; CQL's sum of log_pi for the entropy temperature and, with the Lagrange weight, the penalty
        sums between phases 4 and 5), the actor's gradients; for IQL the value net's, the critic's and the actor's gradients; for FQE the
        critic's alone."""
        phases, xids, n = (C.c_int32 * 8)(), (C.c_int32 * 8)(), C.c_int32()
        L.check(self.lib.exorl_agent_update_plan(C.byref(self.cfg), phases, xids, 8, C.byref(n)))
        for phase, xid in zip(phases[:n.value], xids[:n.value]):
            self.update_phase(phase, stddev, noise_critic, noise_actor)
            if xid >= 0:
                yield self.exchange(xid), L.XCHG_SUM

    def run_update(self, *a, **k):
        """One gradient step on any world size: update() — one host call; with a communicator the library all-reduces between its
        phases — or, with the collectives left to torch.distributed (gloo / EXORL_DP_COMM=torch), update_steps()."""
        if self.comm is not None:
            return self.update(*a, **k)
        self._run(self.update, self.update_steps, *a, **k)

    def act(self, obs, stddev, eval_mode, noise=None):
        o = self._dev(obs).view(-1, self.obs_dim)
        n = o.shape[0]
        out = torch.empty(n, self.act_dim, dtype=torch.float32, device=self.device)
        nz = self._dev(noise) if noise is not None else None
        L.check(self.lib.exorl_agent_act(self.h, o.data_ptr(), n, stddev, int(eval_mode), L.ptr(nz), out.data_ptr(),
                                         L.current_stream()))
        return out

    def act_host(self, obs, stddev, eval_mode, noise=None):
        """act() for ONE observation in one kernel launch (exorl_agent_act_host): the row and the optional noise row travel as kernel
        arguments, the action lands in a pinned host slot. Returns a numpy (act_dim,) array, or None when the fused kernel does not apply
        (CQL's tanh-Gaussian policy, hidden_dim % 4 != 0) and the caller should take act()."""
        if self.kind == 'cql' or self.hidden_dim % 4 != 0 or self.obs_dim > 256:
            return None
        slot = getattr(self, '_act_slot', None)
        if slot is None:
            slot = self._act_slot = torch.zeros(64, dtype=torch.float32).pin_memory()
        o = np.ascontiguousarray(np.asarray(obs, np.float32).reshape(-1))
        assert o.size == self.obs_dim, (o.size, self.obs_dim)
        nz = None if noise is None else np.ascontiguousarray(np.asarray(noise, np.float32).reshape(-1))
        stream = L.current_stream()
        L.check(self.lib.exorl_agent_act_host(self.h, o.ctypes.data, 1, float(stddev), int(eval_mode), nz.ctypes.data if nz is not None else None,
                                              slot.data_ptr(), stream))
        torch.cuda.current_stream(self.device).synchronize()
        return slot[:self.act_dim].numpy().copy()

    def set_comm(self, comm):
        """Attach an exorl_amd.comm.Comm of cfg.world_size ranks: update() then runs the data-parallel step in one call."""
        L.check(self.lib.exorl_agent_set_comm(self.h, comm.h if comm is not None else None))
        self.comm = comm

    def enable_graph(self, replay_engine, nstep, gamma, stddev):
        L.check(self.lib.exorl_agent_enable_graph(self.h, replay_engine.h, nstep, gamma, stddev, L.current_stream()))
        self.graph_captures = getattr(self, 'graph_captures', 0) + 1

    def enable_graph_goal(self, replay_engine, nstep, gamma, stddev):
        """enable_graph on an arena with a goal rule (ReplayEngine.set_goal): the captured gather relabels and writes [obs | g] rows into the
        batch slots (exorl_agent_enable_graph_goal); needs the arena's O + G == obs_dim. A later set_goal makes the graph stale."""
        L.check(self.lib.exorl_agent_enable_graph_goal(self.h, replay_engine.h, nstep, gamma, stddev, L.current_stream()))
        self.graph_captures = getattr(self, 'graph_captures', 0) + 1

    def enable_graph_intr(self, replay_engine, nstep, gamma, stddev, intr=None, batch=None, meta_dim=0):
        """enable_graph with a reward-free agent's module step in front of the agent's (exorl_agent_enable_graph_intr): `batch` is the
        module's L.IntrBatch over this engine's batch slots; meta_dim > 0 for [obs | meta] rows. intr=None: the agent's step alone."""
        L.check(self.lib.exorl_agent_enable_graph_intr(self.h, intr.h if intr is not None else None, C.byref(batch) if batch is not None else None,
                                                       meta_dim, replay_engine.h, nstep, gamma, stddev, L.current_stream()))
        self._graph_keep = (intr, batch)          # the graph holds the module's buffers
        self.graph_captures = getattr(self, 'graph_captures', 0) + 1

    def disable_graph(self):
        L.check(self.lib.exorl_agent_disable_graph(self.h))
        self._graph_keep = None

    def step_graph(self, stddev):
        L.check(self.lib.exorl_agent_step_graph(self.h, stddev, L.current_stream()))

    def noise_counter(self):
        """Philox draw counter of the update noise AFTER the steps enqueued so far (synchronises): step k of a DDPG-family agent
        drew its critic-target noise at counter 2k+2 and its actor noise at 2k+3 (the counter is advanced at the step's start)."""
        c = C.c_uint64()
        L.check(self.lib.exorl_agent_noise_counter(self.h, C.byref(c), L.current_stream()))
        return int(c.value)

    def philox_normal(self, seed, counter, shape):
        """The standard-normal block the update kernels draw for (seed, counter): element e = row * A + column (test hook)."""
        out = torch.empty(tuple(shape), dtype=torch.float32, device=self.device)
        L.check(self.lib.exorl_debug_philox_normal(seed, counter, out.numel(), out.data_ptr(), L.current_stream()))
        return out

    def poison_scratch(self):
        """Fills the scratch a step writes before it reads, and the padding between all sub-buffers, with NaN bit patterns (test hook:
        the next step must not notice)."""
        L.check(self.lib.exorl_debug_agent_poison_scratch(self.h, L.current_stream()))

    def weight_images(self, net):
        """The derived weight copies of `net` (exorl_debug_agent_weight_images) as views of this engine's workspace: 'w0t' float32
        (n_trunks, in, H); 'w0_hi' / 'w0_lo' (n_trunks, H, round_up(in, 32)) and 'w1_hi' / 'w1_mid' / 'w1_lo' (n_heads, H, H), bf16 bit
        patterns as int16. An image the configuration does not have is None. Launches nothing (test hook)."""
        w = L.WeightImages()
        L.check(self.lib.exorl_debug_agent_weight_images(self.h, net, C.byref(w)))
        H, kp = w.hidden_dim, (w.in_dim + 31) // 32 * 32

        def planes(ptr, shape):
            if not ptr:
                return None
            n = int(np.prod(shape))
            return self._view(ptr, (n + 1) // 2).view(torch.int16)[:n].view(*shape)
        out = {'w0t': self._view(w.w0t, w.n_trunks * w.in_dim * H).view(w.n_trunks, w.in_dim, H)}
        for k in ('w0_hi', 'w0_lo'):
            out[k] = planes(getattr(w, k), (w.n_trunks, H, kp))
        for k in ('w1_hi', 'w1_mid', 'w1_lo'):
            out[k] = planes(getattr(w, k), (w.n_heads, H, H))
        return out

    def set_parallel_branches(self, enable):
        L.check(self.lib.exorl_agent_set_parallel_branches(self.h, int(bool(enable))))

    def set_metrics(self, enable):
        L.check(self.lib.exorl_agent_set_metrics(self.h, int(bool(enable))))

    # ---- the three sum windows (metric window, evaluation, FQE's value pass): exorl_agent_<name>_bytes / set_<name> / <name>_read ------
    def _window_bytes(self, name):
        return int(getattr(self.lib, f'exorl_agent_{name}_bytes')(C.byref(self.cfg)))

    def _set_window(self, name, keep, buf):
        """Attach a torch-owned buffer: True allocates one of the window's size, a uint8 tensor of at least that size is taken as it is
        (its contents do not matter), None detaches. The tensor is kept on the engine as `keep`."""
        fn = getattr(self.lib, f'exorl_agent_set_{name}')
        if buf is None:
            L.check(fn(self.h, None, 0))
            setattr(self, keep, None)
            return
        if buf is True:
            buf = torch.empty(self._window_bytes(name), dtype=torch.uint8, device=self.device)
        torch.cuda.current_stream(self.device).synchronize()      # the call clears the window's sums itself, behind whatever wrote `buf`
        L.check(fn(self.h, buf.data_ptr(), buf.numel()))
        setattr(self, keep, buf)

    def _read_window(self, name, n, reset):
        """(sums, count) of the window: n float64 sums and the steps or rows in them; reset empties the window."""
        sums, count = np.zeros(n, np.float64), C.c_int64()
        L.check(getattr(self.lib, f'exorl_agent_{name}_read')(self.h, sums.ctypes.data, C.byref(count), int(bool(reset)), L.current_stream()))
        return sums, int(count.value)

    def metric_window_bytes(self):
        return self._window_bytes('metric_window')

    def set_metric_window(self, buf=True):
        """Windowed metrics (exorl_agent_set_metric_window); None switches the mode off."""
        self._set_window('metric_window', '_window', buf)

    def metric_window_read(self, reset=True):
        """(sums, steps): float64 sums per metric slot and the number of steps in them."""
        return self._read_window('metric_window', L.N_METRICS, reset)

    def eval_bytes(self):
        return self._window_bytes('eval')

    def set_eval(self, buf=True):
        """The forward-only evaluation's window (exorl_agent_set_eval)."""
        self._set_window('eval', '_eval', buf)

    def evaluate(self):
        """One forward-only pass on the rows in the batch slots, added to the window (exorl_agent_evaluate): no step state moves."""
        L.check(self.lib.exorl_agent_evaluate(self.h, L.current_stream()))

    def eval_read(self, reset=True):
        """(sums, rows): float64 sums per L.E_* slot and the rows in them."""
        return self._read_window('eval', L.N_EVAL, reset)

    def fqe_value_bytes(self):
        return self._window_bytes('fqe_value')

    def set_fqe_value(self, buf=True):
        """The value pass's window (exorl_agent_set_fqe_value)."""
        self._set_window('fqe_value', '_fqe_value', buf)

    def fqe_value(self, rows):
        """One forward-only pass of Q(s, mu(s)) on the first `rows` obs rows in the batch slots, added to the window (exorl_agent_fqe_value)."""
        L.check(self.lib.exorl_agent_fqe_value(self.h, int(rows), L.current_stream()))

    def fqe_value_read(self, reset=True):
        """(sums, rows): float64 sums per L.FQE_V_* slot and the rows in them."""
        return self._read_window('fqe_value', L.N_FQE_VALUE, reset)

    def cql_alpha_state(self):
        host = np.zeros(6, np.float32)
        L.check(self.lib.exorl_agent_cql_alpha(self.h, host.ctypes.data, 0))
        return host            # log_actor_alpha, Adam m, Adam v [, log_critic_alpha, m, v with use_critic_lagrange]

    def set_cql_alpha_state(self, log_alpha, m=0.0, v=0.0, log_critic_alpha=0.0, cm=0.0, cv=0.0):
        host = np.array([log_alpha, m, v, log_critic_alpha, cm, cv], np.float32)
        L.check(self.lib.exorl_agent_cql_alpha(self.h, host.ctypes.data, 1))

    def set_iql(self, expectile, temperature, max_weight):
        """IQL's hyper-parameters (exorl_agent_set_iql); refused while a graph is captured."""
        L.check(self.lib.exorl_agent_set_iql(self.h, expectile, temperature, max_weight))

    def set_prdc(self, replay_engine, beta):
        """PRDC: bind the key table `replay_engine.build_keys(beta)` made (exorl_agent_set_prdc). Refused while a graph is captured, for
        another kind, for a stale table and for one built with another beta or another observation / action split."""
        L.check(self.lib.exorl_agent_set_prdc(self.h, replay_engine.h, float(beta)))
        self._prdc_keep = replay_engine             # the step reads the replay's table

    def rebrac_bytes(self):
        """Bytes of the ReBRAC buffer for this configuration (exorl_agent_rebrac_bytes); raises for a kind other than TD3+BC."""
        n = int(self.lib.exorl_agent_rebrac_bytes(C.byref(self.cfg)))
        if n == 0:
            raise L.ExorlError(self.lib.exorl_last_error().decode())
        return n

    def set_rebrac(self, buf, critic_beta):
        """ReBRAC on a TD3+BC engine (exorl_agent_set_rebrac): `buf` a uint8 device tensor of at least rebrac_bytes(), 256-byte aligned,
        kept alive here; None detaches and the engine is TD3+BC again. Refused while a graph is captured and while a metric window or an
        eval window is attached. Batch slots handed out before the call are stale: ask batch_slots() again."""
        torch.cuda.current_stream(self.device).synchronize()      # a step in flight may still read the buffer this call replaces or lets go
        if buf is None:
            L.check(self.lib.exorl_agent_set_rebrac(self.h, None, 0, float(critic_beta)))
            self._rebrac = None
            return
        L.check(self.lib.exorl_agent_set_rebrac(self.h, buf.data_ptr(), buf.numel(), float(critic_beta)))
        self._rebrac = buf

    def sarsa_bytes(self):
        """Bytes of the SARSA buffer for this configuration (exorl_agent_sarsa_bytes); raises for a kind other than TD3+BC, TD3, CRR and FQE."""
        n = int(self.lib.exorl_agent_sarsa_bytes(C.byref(self.cfg)))
        if n == 0:
            raise L.ExorlError(self.lib.exorl_last_error().decode())
        return n

    def set_sarsa(self, buf):
        """The SARSA target on a TD3+BC, TD3, CRR or FQE engine (exorl_agent_set_sarsa): `buf` a uint8 device tensor of at least
        sarsa_bytes(), 256-byte aligned, kept alive here; None detaches and the engine is the base kind again. Refused while a graph is
        captured, while ReBRAC is set and while a metric window or an eval window is attached. Batch slots handed out before the call are
        stale: ask batch_slots() again."""
        torch.cuda.current_stream(self.device).synchronize()      # a step in flight may still read the buffer this call replaces or lets go
        if buf is None:
            L.check(self.lib.exorl_agent_set_sarsa(self.h, None, 0))
            self._sarsa = None
            return
        L.check(self.lib.exorl_agent_set_sarsa(self.h, buf.data_ptr(), buf.numel()))
        self._sarsa = buf

    def set_next_action(self, next_action, next_valid=None):
        """The dataset's action at next_obs, (B, A), and whether the episode holds it, (B) of 1.0 / 0.0 (None: every row valid), into the
        ReBRAC or the SARSA buffer, whichever is set: what the HBM sampler writes there itself, for batches that come from a plain iterator
        (set_batch). A row with next_valid 0 is stored as zeros whatever the caller's row holds, as the gather stores it."""
        buf = self._rebrac if self._rebrac is not None else self._sarsa
        if buf is None:
            raise L.ExorlError('set_next_action: no ReBRAC buffer is set (set_rebrac) and no SARSA buffer (set_sarsa)')
        B, A = self.batch, self.act_dim
        na = self._dev(next_action)
        nv = torch.ones(B, dtype=torch.float32, device=self.device) if next_valid is None else self._dev(next_valid)
        if na.numel() != B * A or nv.numel() != B:
            raise L.ExorlError(f'next_action has {na.numel()} elements and next_valid {nv.numel()}, expected {B * A} and {B}')
        na = torch.where(nv.reshape(B, 1) != 0, na.reshape(B, A), torch.zeros((), device=self.device))      # the gather's rule: zeros where invalid
        slots, f32 = self.batch_slots(), buf[:buf.numel() // 4 * 4].view(torch.float32)     # the library says where the two runs lie
        for ptr, src in ((slots.next_action, na), (slots.next_valid, nv)):
            o = (ptr - buf.data_ptr()) // 4
            f32[o:o + src.numel()].copy_(src.reshape(-1))

    def calql_bytes(self):
        """Bytes of Cal-QL's buffer for this configuration (exorl_agent_calql_bytes); raises for a kind other than CQL."""
        n = int(self.lib.exorl_agent_calql_bytes(C.byref(self.cfg)))
        if n == 0:
            raise L.ExorlError(self.lib.exorl_last_error().decode())
        return n

    def set_calql(self, buf):
        """Cal-QL on a CQL engine (exorl_agent_set_calql): `buf` a uint8 device tensor of at least calql_bytes(), 256-byte aligned, kept
        alive here; None detaches and the engine is CQL again. Refused while a graph is captured and while a metric window or an eval window
        is attached."""
        torch.cuda.current_stream(self.device).synchronize()      # a step in flight may still read the buffer this call replaces or lets go
        if buf is None:
            L.check(self.lib.exorl_agent_set_calql(self.h, None, 0))
            self._calql = None
            return
        L.check(self.lib.exorl_agent_set_calql(self.h, buf.data_ptr(), buf.numel()))
        self._calql = buf

    def mc_return_view(self):
        """The (B,) float32 view of Cal-QL's buffer the critic step reads: where the HBM sampler writes the rows' return-to-go."""
        if self._calql is None:
            raise L.ExorlError('mc_return_view: no Cal-QL buffer is set (set_calql)')
        return self._calql[:self.batch * 4].view(torch.float32)

    def set_mc_return(self, mc_return):
        """The dataset's return-to-go of each row of the batch, (B), into Cal-QL's buffer: what the HBM sampler writes there itself, for
        batches that come from a plain iterator (set_batch)."""
        m = self._dev(mc_return)
        if m.numel() != self.batch:
            raise L.ExorlError(f'mc_return has {m.numel()} elements, expected {self.batch}')
        self.mc_return_view().copy_(m.reshape(-1))

    def nn_result(self):
        """PRDC: (idx int32 (B,), d2 float32 (B,), a_nn float32 (B, A)) views of the last search's results, and the bound table's key
        ranges (0: nothing bound)."""
        i, d, a, s = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int32()
        L.check(self.lib.exorl_agent_nn_result(self.h, C.byref(i), C.byref(d), C.byref(a), C.byref(s)))
        B, A = self.batch, self.act_dim
        return self._view(i.value, B).view(torch.int32), self._view(d.value, B), self._view(a.value, B * A).view(B, A), s.value

    def metrics_raw(self):
        host = np.zeros(L.N_METRICS, np.float32)
        L.check(self.lib.exorl_agent_metrics(self.h, host.ctypes.data, L.current_stream()))
        return host

    def opt_steps(self):
        a, c = C.c_int64(), C.c_int64()
        L.check(self.lib.exorl_agent_opt_steps(self.h, C.byref(a), C.byref(c)))
        return a.value, c.value

    def set_opt_steps(self, actor_steps, critic_steps):
        L.check(self.lib.exorl_agent_set_opt_steps(self.h, actor_steps, critic_steps))


class IntrEngine(_Phased):
    """Intrinsic-reward module (exorl_intr_t): RND / ICM / ICM-APT. Parameters live in a torch-owned workspace so they
    can be exposed as tensors (state_dict, snapshots)."""
    KINDS = {'rnd': L.INTR_RND, 'icm': L.INTR_ICM, 'icm_apt': L.INTR_ICM_APT, 'disagreement': L.INTR_DISAGREEMENT, 'diayn': L.INTR_DIAYN,
             'proto': L.INTR_PROTO, 'aps': L.INTR_APS, 'smm': L.INTR_SMM}

    def __init__(self, kind, obs_dim, act_dim, hidden_dim, batch, rep_dim=0, lr=1e-4, scale=1.0, knn_k=12, knn_avg=True,
                 knn_rms=True, knn_clip=0.0, clip_val=5.0, n_models=0, num_protos=0, queue_size=0, tau=0.1, target_tau=0.05, sp_lr=1e-3, vae_lr=1e-2,
                 vae_beta=0.5, state_ent_coef=1.0, latent_ent_coef=1.0, latent_cond_ent_coef=1.0, goal=(150.0, 75.0), precision='fp32',
                 device='cuda', encoded=False, world_size=1, rank=0):
        self.device = _require_gpu(device)
        self.kind, self.batch, self.obs_dim, self.act_dim = kind, batch, obs_dim, act_dim
        self.world_size, self.rank = world_size, rank
        cfg = L.IntrCfg(self.KINDS[kind], obs_dim, act_dim, hidden_dim, rep_dim, batch, PRECISION[precision], knn_k, int(bool(knn_avg)),
                             int(bool(knn_rms)), n_models, 1 if encoded else 0, lr, scale, knn_clip, clip_val, num_protos, queue_size, tau, target_tau,
                             sp_lr, vae_lr, vae_beta, state_ent_coef, latent_ent_coef, latent_cond_ent_coef, goal[0], goal[1], world_size, rank)
        self._create('intr', cfg)
        rms, bn, nbn = C.c_void_p(), C.c_void_p(), C.c_int64()
        L.check(self.lib.exorl_intr_state(self.h, C.byref(rms), C.byref(bn), C.byref(nbn)))
        self._rms = self._view(rms.value, 4)                       # {float M, float S, double n}
        self.bn = self._view(bn.value, nbn.value) if bn.value else None
        self.queue = None
        if kind == 'proto':
            q, r, c, ptr = C.c_void_p(), C.c_int64(), C.c_int64(), C.c_int64()
            L.check(self.lib.exorl_intr_queue(self.h, C.byref(q), C.byref(r), C.byref(c), C.byref(ptr), 0))
            self.queue = self._view(q.value, r.value * c.value).view(r.value, c.value)

    def queue_ptr(self, set_to=None):
        q, r, c = C.c_void_p(), C.c_int64(), C.c_int64()
        ptr = C.c_int64(0 if set_to is None else int(set_to))
        L.check(self.lib.exorl_intr_queue(self.h, C.byref(q), C.byref(r), C.byref(c), C.byref(ptr), int(set_to is not None)))
        return ptr.value

    def flat(self, what=L.T_PARAM):
        p, n = C.c_void_p(), C.c_int64()
        L.check(self.lib.exorl_intr_flat(self.h, what, C.byref(p), C.byref(n)))
        return self._view(p.value, n.value)

    def rms_state(self):
        """(M, S, n) of the module's utils.RMS."""
        raw = self._rms.cpu().numpy()
        return float(raw[0]), float(raw[1]), float(raw[2:4].view(np.float64)[0])

    def set_rms_state(self, M, S, n):
        raw = np.zeros(4, np.float32)
        raw[0], raw[1] = M, S
        raw[2:4] = np.array([n], np.float64).view(np.float32)
        self._rms.copy_(torch.from_numpy(raw))

    def _batch(self, obs, action, next_obs, extr_reward, reward_out, skill=None, obs_ld=None, action_ld=None, next_obs_ld=None, skill_ld=0,
               cat_uniform=None, next_obs_target=None, dobs_out=None):
        return L.IntrBatch(obs, obs_ld or self.obs_dim, action, action_ld or self.act_dim, next_obs, next_obs_ld or self.obs_dim,
                           skill, skill_ld, extr_reward, reward_out, next_obs_target, self.obs_dim, dobs_out, cat_uniform)

    def update(self, obs, action, next_obs, extr_reward, reward_out, train=True, **kw):
        """Device pointers (ints) + row strides in floats; see exorl_intr_batch. train: True/1, False/0, or 2 (optimiser step only)."""
        b = self._batch(obs, action, next_obs, extr_reward, reward_out, **kw)
        L.check(self.lib.exorl_intr_update(self.h, C.byref(b), 2 if train == 2 else int(bool(train)), L.current_stream()))

    def update_phase(self, phase, obs, action, next_obs, extr_reward, reward_out, train=True, **kw):
        """One phase of the data-parallel module step (exorl_intr_update_phase); returns the exchange to run before the next phase
        (L.INTR_XCHG_*) or -1 when the step is complete."""
        b = self._batch(obs, action, next_obs, extr_reward, reward_out, **kw)
        nxt = C.c_int32()
        L.check(self.lib.exorl_intr_update_phase(self.h, C.byref(b), 2 if train == 2 else int(bool(train)), phase, C.byref(nxt), L.current_stream()))
        return nxt.value

    def update_steps(self, *a, **k):
        """update() as its phases, for run_steps: the library names the exchange that follows each phase."""
        return phase_steps(lambda phase: self.update_phase(phase, *a, **k), self.exchange)

    def run_update(self, *a, **k):
        """update(), or for a sharded module its phases with the exchanges each one names."""
        self._run(self.update, self.update_steps, *a, **k)

    def metrics_raw(self):
        host = np.zeros(L.N_INTR_METRICS, np.float32)
        L.check(self.lib.exorl_intr_metrics(self.h, host.ctypes.data, L.current_stream()))
        return host

    def opt_steps(self):
        n = C.c_int64()
        L.check(self.lib.exorl_intr_opt_steps(self.h, C.byref(n), 0))
        return n.value

    def set_opt_steps(self, n):
        v = C.c_int64(n)
        L.check(self.lib.exorl_intr_opt_steps(self.h, C.byref(v), 1))

    def counter(self, set_to=None):
        c = C.c_uint64(0 if set_to is None else int(set_to))
        L.check(self.lib.exorl_intr_counter(self.h, C.byref(c), 0 if set_to is None else 1))
        return int(c.value)

    # -- pickling support, as PixelEngine's
    def export_state(self):
        return {'flat': {w: self.flat(w).cpu() for w in (L.T_PARAM, L.T_ADAM_M, L.T_ADAM_V)}, 'rms': self.rms_state(),
                'bn': self.bn.cpu() if self.bn is not None else None, 'opt_steps': self.opt_steps(),
                'queue': (self.queue.cpu(), self.queue_ptr()) if self.queue is not None else None, 'counter': self.counter()}

    def import_state(self, st):
        for w, t in st['flat'].items():
            self.flat(w).copy_(t)
        self.set_rms_state(*st['rms'])
        if st['bn'] is not None:
            self.bn.copy_(st['bn'])
        self.set_opt_steps(st['opt_steps'])
        if st.get('queue') is not None:         # pickles from before the queue and the counter were saved lack these keys
            self.queue.copy_(st['queue'][0])
            self.queue_ptr(st['queue'][1])
        if 'counter' in st:
            self.counter(st['counter'])


def run_exchange(buf, op, rank=None, dist=None):
    """One exchange of a phased call under torch.distributed: sum all-reduce in place, or all-gather of the (world_size, count) slots in
    rank order (into views of the slots: gloo has no all_gather_into_tensor)."""
    dist = dist or torch.distributed
    if op == L.XCHG_SUM:
        dist.all_reduce(buf)
    else:
        slots = list(buf.unbind(0))
        dist.all_gather(slots, slots[rank].clone())


def phase_steps(phase_fn, exchange_fn):
    """The steps of a call whose phases name their own exchange: phase_fn(0), phase_fn(1), ... each return the exchange id to run before
    the next phase (-1: done), or (id, value), and exchange_fn(id) -> (buffer, op) names its buffer. Returns the last phase's value."""
    phase = 0
    while True:
        out = phase_fn(phase)
        xid, value = out if isinstance(out, tuple) else (out, None)
        if xid < 0:
            return value
        yield exchange_fn(xid)
        phase += 1


def run_steps(steps, rank=None, dist=None):
    """The one loop behind every phased engine call: runs a *_steps generator to completion, exchanging every (buffer, op) it yields across
    the ranks before it resumes with its next phase. `rank` is this rank's slot in a gather. Returns what the call returns."""
    while True:
        try:
            buf, op = next(steps)
        except StopIteration as done:
            return done.value
        run_exchange(buf, op, rank, dist)


def drive_phases(phase_fn, exchange_fn, rank, dist=None):
    """run_steps for a caller that holds the phase function itself (see phase_steps)."""
    run_steps(phase_steps(phase_fn, exchange_fn), rank, dist)


def global_means(engine, keep=None):
    """engine.metrics_raw() as means over the global batch: a sharded engine's partial means summed over the ranks. `keep` slices the
    slots that hold the same value on every rank already (the RMS state) and are not summed."""
    raw = engine.metrics_raw()
    if engine.world_size == 1:
        return raw
    t = torch.from_numpy(raw.copy()).to(engine.device)
    run_exchange(t, L.XCHG_SUM)
    out = t.cpu().numpy()
    if keep is not None:
        out[keep] = raw[keep]
    return out


class PixelEngine(_Phased):
    """DDPG on pixel observations (exorl_pixel_agent_t): augmentation, conv encoder, pixel actor/critic and their update."""
    NETS = {'encoder': 0, 'actor': 1, 'critic': 2, 'critic_target': 3}

    def __init__(self, obs_shape, act_dim, feature_dim, hidden_dim, batch, lr=1e-4, tau=0.01, stddev_clip=0.3, precision='fp32', seed=0,
                 device='cuda', meta_dim=0, sf_dim=0, world_size=1):
        self.device = _require_gpu(device)
        self.world_size = world_size
        c, h, w = obs_shape
        if h != w:
            raise L.ExorlError(f'pixel observations must be square, got {obs_shape}')
        self.obs_shape, self.act_dim, self.batch, self.meta_dim = tuple(obs_shape), act_dim, batch, meta_dim
        cfg = L.PixelCfg(c, h, act_dim, feature_dim, hidden_dim, batch, PRECISION[precision], meta_dim, lr, tau,
                              stddev_clip if stddev_clip is not None else 0.0, sf_dim, seed, world_size)
        self._create('pixel_agent', cfg)

    def sync_target(self):
        L.check(self.lib.exorl_pixel_agent_sync_target(self.h, L.current_stream()))

    def batch_slots(self):
        out = L.BatchOut()
        L.check(self.lib.exorl_pixel_agent_batch_slots(self.h, C.byref(out)))
        return out

    def _u8(self, x):
        t = torch.as_tensor(x)
        if t.dtype != torch.uint8:
            raise L.ExorlError(f'pixel observations must be uint8 (got {t.dtype}), as the replay buffer stores them')
        return t.to(self.device, non_blocking=True).contiguous()

    def _f(self, x):
        return torch.as_tensor(x).to(self.device, torch.float32, non_blocking=True).contiguous()

    def set_batch(self, obs, action, reward, discount, next_obs):
        ts = [self._u8(obs), self._f(action), self._f(reward), self._f(discount), self._u8(next_obs)]
        L.check(self.lib.exorl_pixel_agent_set_batch(self.h, *[t.data_ptr() for t in ts], L.current_stream()))
        self._keep = ts

    def _i32(self, x):
        return None if x is None else torch.as_tensor(np.ascontiguousarray(x, np.int32)).to(self.device)

    def _update_args(self, stddev, shifts_obs, shifts_next, noise_critic, noise_actor, keep_augmented, keep_encoded):
        """The call's exorl_pixel_step: keep_augmented reuses the images augment() made, keep_encoded also the encodings of the last
        encode(0) / encode(1); a keep flag leaves the shifts out (they are read by a fresh augmentation only)."""
        images = L.PIXEL_IMAGES_ENCODED if keep_encoded else L.PIXEL_IMAGES_AUGMENTED if keep_augmented else L.PIXEL_IMAGES_FRESH
        f32 = lambda x: None if x is None else self._f(x)
        shifts = [self._i32(shifts_obs), self._i32(shifts_next)] if images == L.PIXEL_IMAGES_FRESH else [None, None]
        self._keep_u = ts = shifts + [f32(noise_critic), f32(noise_actor)]
        return C.byref(L.PixelStep(stddev, images, *[L.ptr(t) for t in ts]))

    def update(self, stddev, shifts_obs=None, shifts_next=None, noise_critic=None, noise_actor=None, keep_augmented=False, keep_encoded=False):
        step = self._update_args(stddev, shifts_obs, shifts_next, noise_critic, noise_actor, keep_augmented, keep_encoded)
        L.check(self.lib.exorl_pixel_agent_update(self.h, step, L.current_stream()))

    def update_phase(self, phase, stddev, shifts_obs=None, shifts_next=None, noise_critic=None, noise_actor=None, keep_augmented=False,
                     keep_encoded=False):
        """One of the three phases of update() (exorl_pixel_agent_update_phase); returns the exchange to run before the next phase
        (L.PIXEL_XCHG_*) or -1 when the step is complete."""
        step = self._update_args(stddev, shifts_obs, shifts_next, noise_critic, noise_actor, keep_augmented, keep_encoded)
        nxt = C.c_int32()
        L.check(self.lib.exorl_pixel_agent_update_phase(self.h, phase, step, C.byref(nxt), L.current_stream()))
        return nxt.value

    def update_steps(self, stddev, shifts_obs=None, shifts_next=None, noise_critic=None, noise_actor=None, keep_augmented=False,
                     keep_encoded=False):
        """update() as its phases, for run_steps. Each rank runs the step on its rows and every mean in it is over the global batch, so
        the gradients are sum-all-reduced between the phases: the critic's (+ the encoder's), then the actor's."""
        a = (stddev, shifts_obs, shifts_next, noise_critic, noise_actor, keep_augmented, keep_encoded)
        return phase_steps(lambda phase: self.update_phase(phase, *a), self.exchange)

    def run_update(self, *a, **k):
        """The DDPG pixel step on any world size, as AgentEngine.run_update."""
        if self.comm is not None:
            return self.update(*a, **k)
        self._run(self.update, self.update_steps, *a, **k)

    def grad_buffer(self, exchange):
        """Device view of what a data-parallel step sum-all-reduces: 0 critic (+ encoder) gradients, 1 actor gradients, 2 the encoder's
        gradients of encoder_step."""
        return self.exchange(exchange)[0]

    def set_comm(self, comm):
        """Attach an exorl_amd.comm.Comm of world_size ranks: update() then runs the data-parallel step in one call."""
        L.check(self.lib.exorl_pixel_agent_set_comm(self.h, comm.h if comm is not None else None))
        self.comm = comm

    def augment(self, shifts_obs=None, shifts_next=None):
        ts = [self._i32(shifts_obs), self._i32(shifts_next)]
        L.check(self.lib.exorl_pixel_agent_augment(self.h, L.ptr(ts[0]), L.ptr(ts[1]), L.current_stream()))
        self._keep_s = ts

    def encode(self, which, target=False):
        """Device pointer of the (batch, repr_dim) features of the augmented obs (which=0) / next_obs (1)."""
        p = C.c_void_p()
        L.check(self.lib.exorl_pixel_agent_encode(self.h, which, int(bool(target)), C.byref(p), L.current_stream()))
        return p.value

    def encoder_step(self, which, dfeat_ptr, opt):
        L.check(self.lib.exorl_pixel_agent_encoder_step(self.h, which, dfeat_ptr, opt, L.current_stream()))

    def encoder_step_phase(self, phase, which, dfeat_ptr, opt):
        """encoder_step in two phases: 0 the backward pass, 1 the optimiser step(s); returns the exchange to run before the next phase
        (the encoder's gradients) or -1."""
        nxt = C.c_int32()
        L.check(self.lib.exorl_pixel_agent_encoder_step_phase(self.h, which, dfeat_ptr, opt, phase, C.byref(nxt), L.current_stream()))
        return nxt.value

    def encoder_step_steps(self, which, dfeat_ptr, opt):
        """encoder_step() as its phases, for run_steps."""
        return phase_steps(lambda phase: self.encoder_step_phase(phase, which, dfeat_ptr, opt), self.exchange)

    def run_encoder_step(self, *a):
        self._run(self.encoder_step, self.encoder_step_steps, *a)

    def encoder_target(self, tau=0.0, init=False):
        L.check(self.lib.exorl_pixel_agent_encoder_target(self.h, tau, int(bool(init)), L.current_stream()))

    def encoder_target_tensors(self, shapes):
        p = C.c_void_p()
        L.check(self.lib.exorl_pixel_agent_encoder_target_ptr(self.h, C.byref(p)))
        out, off = [], 0
        for shp in shapes:
            n = int(np.prod(shp))
            out.append(self._view(p.value + 4 * off, n).view(*shp))
            off += (n + 3) // 4 * 4
        return out

    def set_train_encoder(self, enable):
        L.check(self.lib.exorl_pixel_agent_set_train_encoder(self.h, int(bool(enable))))

    # -- pickling support: everything that defines the training state, as CPU data
    def export_state(self):
        torch.cuda.synchronize()
        steps, ctr = np.zeros(3, np.int64), np.zeros(4, np.uint64)
        L.check(self.lib.exorl_pixel_agent_state(self.h, steps.ctypes.data, ctr.ctypes.data))
        st = {'steps': steps, 'counters': ctr, 'tensors': {}, 'bn2d': self.bn2d().cpu()}
        for net in range(4):
            for what in ((L.T_PARAM,) if net == 3 else (L.T_PARAM, L.T_ADAM_M, L.T_ADAM_V)):
                st['tensors'][(net, what)] = [self.tensor(net, i, what).cpu() for i in range(self.num_tensors(net))]
        m, v, n, p = C.c_void_p(), C.c_void_p(), C.c_int64(), C.c_void_p()
        L.check(self.lib.exorl_pixel_agent_encoder_opt2(self.h, C.byref(m), C.byref(v), C.byref(n)))
        L.check(self.lib.exorl_pixel_agent_encoder_target_ptr(self.h, C.byref(p)))
        st['enc_extra'] = [self._view(q.value, n.value).cpu() for q in (m, v, p)]
        return st

    def import_state(self, st):
        for (net, what), ts in st['tensors'].items():
            for i, t in enumerate(ts):
                self.tensor(net, i, what).copy_(t.reshape(self.tensor(net, i, what).shape))
        m, v, n, p = C.c_void_p(), C.c_void_p(), C.c_int64(), C.c_void_p()
        L.check(self.lib.exorl_pixel_agent_encoder_opt2(self.h, C.byref(m), C.byref(v), C.byref(n)))
        L.check(self.lib.exorl_pixel_agent_encoder_target_ptr(self.h, C.byref(p)))
        for q, t in zip((m, v, p), st['enc_extra']):
            self._view(q.value, n.value).copy_(t)
        steps, ctr = np.ascontiguousarray(st['steps'], np.int64), np.ascontiguousarray(st['counters'], np.uint64)
        if steps.size == 2:                 # ABI-6 pickles: encoder_opt stepped with the other optimisers
            steps = np.array([steps[0], steps[1], steps[0]], np.int64)
        if ctr.size == 3:
            ctr = np.concatenate([ctr, np.zeros(1, np.uint64)])
        if 'bn2d' in st:
            self.bn2d().copy_(st['bn2d'])
        L.check(self.lib.exorl_pixel_agent_set_state(self.h, steps.ctypes.data, ctr.ctypes.data))
        torch.cuda.synchronize()

    def metrics_raw(self):
        host = np.zeros(L.N_METRICS, np.float32)
        L.check(self.lib.exorl_pixel_agent_metrics(self.h, host.ctypes.data, L.current_stream()))
        return host

    def act(self, obs, stddev, eval_mode, noise=None, meta=None):
        o = self._u8(obs)
        out = torch.empty(self.act_dim, dtype=torch.float32, device=self.device)
        nz = self._f(noise) if noise is not None else None
        mt = self._f(meta) if meta is not None else None
        L.check(self.lib.exorl_pixel_agent_act(self.h, o.data_ptr(), L.ptr(mt), stddev, int(eval_mode), L.ptr(nz), out.data_ptr(), L.current_stream()))
        return out

    def bn2d(self):
        """RND's BatchNorm2d buffers: running_mean[c], running_var[c], num_batches_tracked (float) as one device view."""
        p, n = C.c_void_p(), C.c_int64()
        L.check(self.lib.exorl_pixel_agent_bn_state(self.h, C.byref(p), C.byref(n)))
        return self._view(p.value, n.value)

    def rnd_features(self, shifts=None, clip_val=5.0):
        """(predictor-side, target-side) encodings of clamp(BatchNorm2d(aug(obs))) as device pointers (rnd.py:47-53)."""
        sh = self._i32(shifts)
        fp, ft = C.c_void_p(), C.c_void_p()
        L.check(self.lib.exorl_pixel_agent_rnd_features(self.h, L.ptr(sh), clip_val, C.byref(fp), C.byref(ft), L.current_stream()))
        self._keep_r = sh
        return fp.value, ft.value

    def _rnd_features_phase(self, phase, shifts=None, clip_val=5.0):
        """(exchange to run before the next phase or -1, the two feature pointers once phase 2 has run)"""
        fp, ft, nxt = C.c_void_p(), C.c_void_p(), C.c_int32()
        if phase == 0:
            self._keep_r = self._i32(shifts)
        L.check(self.lib.exorl_pixel_agent_rnd_features_phase(self.h, phase, L.ptr(self._keep_r) if phase == 0 else None, clip_val,
                                                              C.byref(fp), C.byref(ft), C.byref(nxt), L.current_stream()))
        return nxt.value, ((fp.value, ft.value) if phase == 2 else None)

    def rnd_features_phase(self, phase, shifts=None, clip_val=5.0):
        """rnd_features in three phases: sum-all-reduce bn_partials() after phases 0 and 1; phase 2 returns the two feature pointers."""
        return self._rnd_features_phase(phase, shifts, clip_val)[1]

    def rnd_features_steps(self, shifts=None, clip_val=5.0):
        """rnd_features() as its phases, for run_steps: the BatchNorm2d statistics are over every rank's frames."""
        return phase_steps(lambda phase: self._rnd_features_phase(phase, shifts, clip_val), self.exchange)

    def run_rnd_features(self, *a):
        return self._run(self.rnd_features, self.rnd_features_steps, *a)

    def bn_partials(self):
        """(c_in * chunks,) float64 device view of the BatchNorm2d partial sums the ranks add up between the rnd_features phases."""
        return self.exchange(L.PIXEL_XCHG_BN)[0]

    def meta_rows(self):
        """(batch, meta_dim) device view of the skill / task rows the trunks read (filled by the sampler or by the caller)."""
        out = self.batch_slots()
        return self._view(out.meta, self.batch * self.meta_dim).view(self.batch, self.meta_dim)

    def feature_view(self, ptr):
        """(batch, repr_dim) tensor over the device pointer encode() returned."""
        n = self.lib.exorl_encoder_out_dim(self.obs_shape[1])
        return self._view(ptr, self.batch * n).view(self.batch, n)


WEIGHTING = {'episodes': L.WEIGHT_EPISODES, 'transitions': L.WEIGHT_TRANSITIONS}


def quantise_weights(w):
    """Float episode weights -> the uint32 weights the device sampler sums: q = rint(w / max(w) * 2^24), computed in float64. The largest
    weight maps to 2^24, a positive weight never maps to 0 (floor at 1: a ratio below 2^-25 is rounded up, not dropped), zero stays zero
    (the episode is never drawn). Negative, non-finite or all-zero weights raise ValueError."""
    w = np.asarray(w, np.float64).reshape(-1)
    if w.size == 0 or not np.all(np.isfinite(w)) or np.any(w < 0) or not np.any(w > 0):
        raise ValueError('episode weights must be finite, non-negative and not all zero')
    q = np.rint(w / w.max() * float(1 << 24))
    q[(w > 0) & (q < 1)] = 1
    return q.astype(np.uint32)


def frame_shape(obs_shape, frame_stack):
    """(c0, H, W) of one frame of a (k * c0, H, W) observation stacked along the channel axis; ValueError for what cannot be one."""
    k, shape = int(frame_stack), tuple(int(d) for d in obs_shape)
    if not 1 <= k <= 16:
        raise ValueError(f'frame_stack={frame_stack}: expected 1 .. 16')
    if k > 1 and len(shape) != 3:
        raise ValueError(f'frame_stack={k} needs a (channels, H, W) observation, got shape {shape}')
    if k > 1 and shape[0] % k:
        raise ValueError(f'frame_stack={k} does not divide the {shape[0]} channels of an observation of shape {shape}')
    return ((shape[0] // k,) + shape[1:]) if k > 1 else shape


class ReplayEngine:
    """HBM-resident episodic arena (exorl_replay_t).

    frame_stack=k > 1: obs_shape is still the sampled (k * c0, H, W) observation, but an arena row holds one (c0, H, W) frame
    (frame_bytes = obs_bytes / k) and the gather assembles every sampled observation from the k rows max(t - k + 1, 0) .. t of its
    episode: byte for byte what an arena of the stacked episodes returns, at 1/k of its memory and upload."""

    def __init__(self, obs_shape, obs_dtype, act_dim, meta_dim, capacity_rows, max_episodes, device='cuda', frame_stack=1):
        self.obs_shape = tuple(obs_shape)
        self.obs_dtype = np.dtype(obs_dtype)
        self.frame_stack = int(frame_stack)
        self.frame_shape = frame_shape(self.obs_shape, frame_stack)
        self.lib = L.load()
        self.device = _require_gpu(device)
        self.obs_bytes = int(np.prod(self.obs_shape)) * self.obs_dtype.itemsize
        self.frame_bytes = self.obs_bytes // self.frame_stack
        self.act_dim, self.meta_dim = act_dim, meta_dim
        cfg = L.ReplayCfg(self.frame_bytes, act_dim, meta_dim, max_episodes, capacity_rows)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            L.check(self.lib.exorl_replay_create(C.byref(cfg), C.byref(h)))
        self.h = h
        self._slot_len, self._order = {}, []      # the length of every resident slot and the order table: how returns_to_go() splits the column
        self.goal = None                          # the GoalRelabel in force (set_goal)
        if self.frame_stack > 1:
            self.set_frame_stack(self.frame_stack)

    def __del__(self):
        h, self.h = getattr(self, 'h', None), None
        if h:
            self.lib.exorl_replay_destroy(h)

    def set_frame_stack(self, frames):
        """exorl_replay_set_frame_stack: refused once an episode has been appended. The constructor's frame_stack= is the way in; this is
        the raw call, which leaves obs_shape / frame_bytes as they are."""
        L.check(self.lib.exorl_replay_set_frame_stack(self.h, frames))

    def append_episode(self, ep, meta_keys=()):
        obs = np.ascontiguousarray(ep['observation'])
        rows = obs.shape[0]
        if self.frame_stack > 1 and obs.shape[1:] == self.obs_shape:      # the stacked episode as the reference stores it: keep the newest frames
            from .replay_buffer import unstack_frames
            obs = np.ascontiguousarray(unstack_frames(obs, self.frame_stack))
        assert obs.dtype == self.obs_dtype and obs.reshape(rows, -1).shape[1] * obs.itemsize == self.frame_bytes
        act = np.ascontiguousarray(ep['action'], np.float32).reshape(rows, -1)
        rew = np.ascontiguousarray(ep['reward'], np.float32).reshape(rows)
        disc = np.ascontiguousarray(ep['discount'], np.float32).reshape(rows)
        meta = None
        if self.meta_dim:
            meta = np.ascontiguousarray(np.concatenate([np.asarray(ep[k], np.float32).reshape(rows, -1) for k in meta_keys], 1))
            assert meta.shape[1] == self.meta_dim
        slot = C.c_int32()
        L.check(self.lib.exorl_replay_append_episode(self.h, obs.ctypes.data, act.ctypes.data, rew.ctypes.data,
                                                     disc.ctypes.data, L.ptr(meta), rows, C.byref(slot)))
        self._slot_len[slot.value] = rows - 1
        return slot.value

    def evict(self, slot):
        L.check(self.lib.exorl_replay_evict(self.h, slot))
        self._slot_len.pop(slot, None)
        if slot in self._order:
            self._order.remove(slot)

    def num_rows(self):
        """(live rows, used rows) of the arena; a row is one time-step, an episode holds len+1."""
        live, used = C.c_int64(), C.c_int64()
        L.check(self.lib.exorl_replay_num_rows(self.h, C.byref(live), C.byref(used)))
        return live.value, used.value

    def set_order(self, slots):
        arr = np.ascontiguousarray(slots, np.int32)
        L.check(self.lib.exorl_replay_set_order(self.h, arr.ctypes.data, len(arr)))
        self._order = [int(x) for x in arr]

    def set_weights(self, weighting='episodes', weights=None):
        """Weighted sampling for the Philox sampler. weighting='episodes': an episode is drawn with probability proportional to its
        weight, then a start uniformly inside it (weights=None: the unweighted sampler, the default). weighting='transitions': an
        episode is drawn with probability proportional to weight x (len - nstep + 1), i.e. weights=None is uniform over transitions
        whatever the episode lengths. `weights`: one float per slot id (as returned by append_episode), quantised by
        quantise_weights(); slots past the end of the array, and slots reused by a later append_episode, have weight 1. Episodes
        shorter than nstep are skipped rather than refused. The MT19937 sampler refuses a weighted arena. A captured step graph
        (agent.enable_graph) samples from the table of its capture: after changing weights, mode or resident episodes call
        enable_graph again (a graph step after a later set_weights raises ExorlError instead of sampling the stale table)."""
        if weighting not in WEIGHTING:
            raise ValueError(f"weighting={weighting!r}: expected 'episodes' or 'transitions'")
        q = None if weights is None else np.ascontiguousarray(quantise_weights(weights))
        L.check(self.lib.exorl_replay_set_weights(self.h, WEIGHTING[weighting], L.ptr(q), 0 if q is None else len(q)))

    def _state_cols(self, what):
        if self.obs_dtype != np.float32:
            raise ValueError(f'{what}: the arena holds {self.obs_dtype} observations; only float32 state arenas are normalised (the pixel '
                             'encoder does its own /255 - 0.5)')
        return self.obs_bytes // 4

    def obs_moments(self):
        """(count, mean, M2) of the float32 observation columns over every row (len + 1 per episode, the reset row included) of the
        episodes in the order table: count an int, mean and M2 = sum (x - mean)^2 float64 arrays of obs_shape. One pass over the arena in
        HBM, bitwise reproducible (exorl_replay_obs_moments). A set-up call: it synchronises the current stream."""
        n = self._state_cols('obs_moments')
        cnt, mean, m2 = C.c_int64(), np.zeros(n, np.float64), np.zeros(n, np.float64)
        L.check(self.lib.exorl_replay_obs_moments(self.h, n, C.byref(cnt), mean.ctypes.data, m2.ctypes.data, L.current_stream()))
        return cnt.value, mean.reshape(self.obs_shape), m2.reshape(self.obs_shape)

    def build_keys(self, beta, key_every=1):
        """The key table of PRDC's nearest-neighbour search (exorl_replay_build_keys): one row [beta * s | a | 0-pad] per resident
        transition, s as the gather emits it (normalised when a normaliser is set), every key_every-th transition kept. A snapshot:
        append_episode, evict, set_order and set_obs_normalizer / clear_obs_normalizer make it stale. float32 state arenas only. A set-up
        call: it allocates and synchronises. Returns the number of rows."""
        self._state_cols('build_keys')
        if self.frame_stack > 1:
            raise ValueError('build_keys: a frame-stacked arena holds pixels; keys are built from float32 state rows')
        L.check(self.lib.exorl_replay_build_keys(self.h, float(beta), int(key_every), L.current_stream()))
        return self.keys_info()[1]

    def keys_info(self):
        """(device pointer, rows, pitch, epoch) of the key table as last built (exorl_replay_keys); ExorlError when there is none or it
        is stale."""
        p, n, pitch, epoch = C.c_void_p(), C.c_int64(), C.c_int32(), C.c_uint64()
        L.check(self.lib.exorl_replay_keys(self.h, C.byref(p), C.byref(n), C.byref(pitch), C.byref(epoch)))
        return p.value, n.value, pitch.value, epoch.value

    def keys(self):
        """A copy of the key table as last built: a (rows, pitch) float32 device tensor, pitch = round_up(O + A, 4). ExorlError when
        there is none or it is stale."""
        _, n, pitch, _ = self.keys_info()
        out = torch.empty(n, pitch, dtype=torch.float32, device=self.device)
        L.check(self.lib.exorl_replay_keys_read(self.h, out.data_ptr(), out.numel() * 4, L.current_stream()))
        return out

    def num_episodes(self):
        """Episodes in the order table: the positions a SAMPLER_GIVEN pair may name."""
        n = C.c_int32()
        L.check(self.lib.exorl_replay_num_episodes(self.h, C.byref(n)))
        return n.value

    def episode_returns(self, gamma):
        """float64 array, one entry per episode of the order table: its discounted return sum_t r[t] prod_{k<t} (gamma d[k]) from the first
        step, gamma rounded to float32 as the gather does (exorl_replay_episode_returns). Bitwise reproducible. A set-up call: it
        synchronises the current stream."""
        out = np.zeros(self.num_episodes(), np.float64)
        L.check(self.lib.exorl_replay_episode_returns(self.h, float(gamma), out.ctypes.data, out.size, L.current_stream()))
        return out

    def build_returns(self, gamma):
        """Builds the return-to-go column with one launch over the order table (exorl_replay_build_returns): per transition
        G_i = r_i + (gamma d_i) G_{i+1} to the episode's end, in float64, stored as float32; gamma rounded to float32 as the gather does. An
        episode cut by a time limit (d = 1 on its last step) gets the return of its recorded remainder and no bootstrap: a lower bound on the
        true return only where rewards are >= 0. Appending or evicting an episode and set_order make the column stale. A set-up call: it
        synchronises the current stream."""
        L.check(self.lib.exorl_replay_build_returns(self.h, float(gamma), L.current_stream()))

    def returns_info(self):
        """(device pointer or None, the build's gamma, epoch, valid) of the return-to-go column (exorl_replay_returns)."""
        p, g, e, v = C.c_void_p(), C.c_float(), C.c_uint64(), C.c_int32()
        L.check(self.lib.exorl_replay_returns(self.h, C.byref(p), C.byref(g), C.byref(e), C.byref(v)))
        return p.value, g.value, e.value, bool(v.value)

    def returns_to_go(self):
        """A list of float32 arrays, one per episode of the order table: G_1 .. G_L of the column as last built
        (exorl_replay_returns_read). ExorlError when there is none or it is stale."""
        lens = [self._slot_len[s] for s in self._order]
        flat = np.zeros(sum(lens), np.float32)
        L.check(self.lib.exorl_replay_returns_read(self.h, flat.ctypes.data, flat.size, L.current_stream()))
        return np.split(flat, np.cumsum(lens)[:-1]) if lens else []

    def set_obs_normalizer(self, mean32, inv32):
        """Every obs / next_obs element sampled from now on is (x - mean32[j]) * inv32[j] (utils.normalize_obs), in the captured step's
        staged gather too; action, reward, discount and meta are untouched. Calling it again replaces the values in place: a captured
        graph uses them from its next step. Switching the normaliser on or off changes the captured kernel: call enable_graph again (a
        graph step across the switch raises ExorlError)."""
        n = self._state_cols('set_obs_normalizer')
        m, w = (np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1)) for a in (mean32, inv32))
        if m.size != n or w.size != n:
            raise ValueError(f'set_obs_normalizer: {m.size} means and {w.size} scales for {n} observation columns')
        L.check(self.lib.exorl_replay_set_obs_norm(self.h, n, m.ctypes.data, w.ctypes.data, L.current_stream()))

    def clear_obs_normalizer(self):
        """Back to the copying gather: samples are the arena's raw rows again."""
        self._state_cols('clear_obs_normalizer')
        L.check(self.lib.exorl_replay_set_obs_norm(self.h, 0, None, None, L.current_stream()))

    GOAL_REWARD = {'keep': L.GOAL_KEEP, 'neg': L.GOAL_NEG, 'sparse': L.GOAL_SPARSE}

    def set_goal(self, goal):
        """Hindsight relabelling in the gather (exorl_replay_set_goal). `goal`: a replay_buffer.GoalRelabel (cols, p_cur, p_traj, p_rand,
        horizon_discount, reward), or None to clear the rule. From then on sample_into(..., goal=...) draws a goal per sample (the state the
        trajectory reaches at next_obs, a later state of it, or any state of the arena), emits its columns behind obs and next_obs and, for
        reward 'neg' / 'sparse', a reached / not-reached reward and discount. float32 state arenas without meta columns only. A set-up
        call: it synchronises the device; a graph captured on the arena's goal path must be captured again afterwards."""
        if goal is None:
            L.check(self.lib.exorl_replay_set_goal(self.h, None, 0, 0.0, 0.0, 0.0, 0.0, 0))
            self.goal = None
            return
        n = self._state_cols('set_goal')
        if self.frame_stack > 1 or len(self.obs_shape) != 1:
            raise ValueError(f'set_goal: the arena holds observations of shape {self.obs_shape} (frame_stack={self.frame_stack}); goals are '
                             'columns of float32 state rows, not pixels')
        if self.meta_dim:
            raise ValueError(f'set_goal: the arena has {self.meta_dim} meta columns: the goal takes the place behind the observation that '
                             '[obs | meta] rows give them')
        cols = np.ascontiguousarray(goal.cols, np.int32)
        if cols.size and (cols.min() < 0 or cols.max() >= n):
            raise ValueError(f'set_goal: goal columns {cols.tolist()} outside the arena\'s {n} observation columns')
        L.check(self.lib.exorl_replay_set_goal(self.h, cols.ctypes.data, cols.size, goal.p_cur, goal.p_traj, goal.p_rand,
                                               0.0 if goal.horizon_discount is None else float(goal.horizon_discount),
                                               self.GOAL_REWARD[goal.reward]))
        self.goal = goal

    def last_goals(self, batch):
        """(batch, 2) int32: the (pos_g, tau) goal of every sample of the last goal launch, as last_pairs gives the pairs."""
        out = np.zeros((batch, 2), np.int32)
        L.check(self.lib.exorl_replay_last_goals(self.h, batch, out.ctypes.data, L.current_stream()))
        return out

    def seed_mt_from_globals(self):
        """Adopts the CURRENT state of Python's `random` and NumPy's legacy global generator — the two
        streams replay_buffer.py:169,222 draw from — so the index stream continues exactly where the
        reference's would (valid for num_workers=0; workers reseed unreproducibly, replay_buffer.py:241-244)."""
        import random
        st = random.getstate()[1]
        py_key, py_pos = np.array(st[:-1], np.uint32), int(st[-1])
        ns = np.random.get_state()
        np_key, np_pos = np.ascontiguousarray(ns[1], np.uint32), int(ns[2])
        L.check(self.lib.exorl_replay_seed_mt(self.h, py_key.ctypes.data, py_pos, np_key.ctypes.data, np_pos))

    def seed_mt_ints(self, py_seed, np_seed):
        L.check(self.lib.exorl_replay_seed_mt_ints(self.h, py_seed, np_seed))

    def seed_philox(self, seed):
        L.check(self.lib.exorl_replay_seed_philox(self.h, seed))

    def sample_into(self, out, batch, nstep, gamma, sampler, pairs=None, want_pairs=False, mc_return=None, goal=None, goals=None):
        """mc_return: a (batch,) float32 device tensor that takes each sample's return-to-go from the column of build_returns, written by
        the same gather launch (exorl_replay_sample_mc); None: exorl_replay_sample.
        goal (needs set_goal): True writes the goal's G columns at column O of the rows of out.obs and out.next_obs, which must be
        4 * (O + G) bytes apart; a pair (goal, next_goal) of 2-D float32 device tensors with unit column stride and at least G columns takes
        them instead. goals: the (batch, 2) int32 (pos_g, tau) of every sample for the GIVEN and MT19937 samplers; Philox draws them in the
        kernel (last_goals reads them back). None: the gather without goals, bit for bit what it was."""
        pin = np.ascontiguousarray(pairs, np.int32) if pairs is not None else None
        pout = np.zeros((batch, 2), np.int32) if want_pairs else None
        if mc_return is not None and (mc_return.dtype != torch.float32 or mc_return.numel() < batch or not mc_return.is_contiguous()):
            raise L.ExorlError(f'sample_into: mc_return must be a contiguous float32 tensor of at least {batch} elements')
        if goal is not None and goal is not False:
            if self.goal is None:
                raise ValueError('sample_into: goal= needs a goal rule (set_goal)')
            O, G = self.obs_bytes // 4, len(self.goal.cols)
            if goal is True:
                if out.obs_stride != 4 * (O + G) or out.next_obs_stride != 4 * (O + G):
                    raise ValueError(f'sample_into: goal=True writes [obs | g] rows of {O} + {G} floats: obs_stride={out.obs_stride} and '
                                     f'next_obs_stride={out.next_obs_stride} must both be {4 * (O + G)} bytes')
                dst = (out.obs + 4 * O, O + G, out.next_obs + 4 * O, O + G)
            else:
                g, ng = goal
                for t in (g, ng):
                    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] < batch or t.shape[1] < G or t.stride(1) != 1:
                        raise ValueError(f'sample_into: goal destinations must be 2-D float32 tensors of at least {batch} x {G} with unit '
                                         'column stride')
                dst = (g.data_ptr(), g.stride(0), ng.data_ptr(), ng.stride(0))
            gin = np.ascontiguousarray(goals, np.int32) if goals is not None else None
            if gin is not None and gin.shape != (batch, 2):
                raise ValueError(f'sample_into: goals must be ({batch}, 2) (pos_g, tau) pairs, got {gin.shape}')
            L.check(self.lib.exorl_replay_sample_goal(self.h, batch, nstep, gamma, sampler, L.ptr(pin), L.ptr(gin), C.byref(out), dst[0], dst[1],
                                                      dst[2], dst[3], L.ptr(mc_return), L.ptr(pout), L.current_stream()))
            return pout
        if mc_return is None:
            L.check(self.lib.exorl_replay_sample(self.h, batch, nstep, gamma, sampler, L.ptr(pin), C.byref(out), L.ptr(pout),
                                                 L.current_stream()))
            return pout
        L.check(self.lib.exorl_replay_sample_mc(self.h, batch, nstep, gamma, sampler, L.ptr(pin), C.byref(out), mc_return.data_ptr(), L.ptr(pout),
                                                L.current_stream()))
        return pout

    def last_pairs(self, batch):
        out = np.zeros((batch, 2), np.int32)
        L.check(self.lib.exorl_replay_last_pairs(self.h, batch, out.ctypes.data, L.current_stream()))
        return out

    def alloc_batch(self, batch, goal_cols=0):
        """Fresh output tensors (B,*obs_shape) (B,A) (B,1) (B,1) (B,*obs_shape) [(B,meta)] and the BatchOut that points at them.
        goal_cols=G > 0 (a state arena with a goal rule): obs and next_obs are (B, O + G), the [obs | g] rows of sample_into(goal=True)."""
        tdt = torch.uint8 if self.obs_dtype == np.uint8 else torch.float32
        dev = self.device
        if goal_cols:
            W = self.obs_bytes // 4 + int(goal_cols)
            obs = torch.empty(batch, W, dtype=torch.float32, device=dev)
            nobs = torch.empty_like(obs)
            act = torch.empty(batch, self.act_dim, dtype=torch.float32, device=dev)
            rew = torch.empty(batch, 1, dtype=torch.float32, device=dev)
            disc = torch.empty(batch, 1, dtype=torch.float32, device=dev)
            out = L.BatchOut(obs.data_ptr(), 4 * W, act.data_ptr(), self.act_dim, rew.data_ptr(), disc.data_ptr(), nobs.data_ptr(), 4 * W, None, 0)
            return (obs, act, rew, disc, nobs), out
        obs = torch.empty((batch,) + self.obs_shape, dtype=tdt, device=dev)
        nobs = torch.empty_like(obs)
        act = torch.empty(batch, self.act_dim, dtype=torch.float32, device=dev)
        rew = torch.empty(batch, 1, dtype=torch.float32, device=dev)
        disc = torch.empty(batch, 1, dtype=torch.float32, device=dev)
        meta = torch.empty(batch, self.meta_dim, dtype=torch.float32, device=dev) if self.meta_dim else None
        out = L.BatchOut(obs.data_ptr(), self.obs_bytes, act.data_ptr(), self.act_dim, rew.data_ptr(), disc.data_ptr(),
                         nobs.data_ptr(), self.obs_bytes, L.ptr(meta), self.meta_dim)
        return (obs, act, rew, disc, nobs) + ((meta,) if meta is not None else ()), out

    def sample(self, batch, nstep, gamma, sampler=L.SAMPLER_MT19937, pairs=None, want_pairs=False):
        """One batch into fresh tensors (alloc_batch); with want_pairs also the (episode position, start idx) pairs drawn."""
        res, out = self.alloc_batch(batch)
        p = self.sample_into(out, batch, nstep, gamma, sampler, pairs, want_pairs)
        return (res, p) if want_pairs else res
