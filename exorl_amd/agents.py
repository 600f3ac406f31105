"""Agent classes with the reference's constructor kwargs and act()/update() signatures, running on
libexorl_hip.so. Hydra drop-in: `agent._target_=exorl_amd.agents.TD3BCAgent`.

Reference classes mirrored (file:line in /root/reference):
  TD3BCAgent  agents/offline_learning/td3_bc.py:59-189      TD3Agent  agents/offline_learning/td3.py:59-186
  BCAgent     agents/offline_learning/bc.py:34-110           DDPGAgent agents/unsupervised_learning/ddpg.py:126-328 (states)
  CRRAgent    agents/offline_learning/crr.py:59-219          CQLAgent  agents/offline_learning/cql.py:59-286
  RNDAgent    agents/unsupervised_learning/rnd.py:63-159     ICMAgent  agents/unsupervised_learning/icm.py:48-139
  ICMAPTAgent agents/unsupervised_learning/icm_apt.py:60-158 DisagreementAgent agents/unsupervised_learning/disagreement.py:50-136
  DIAYNAgent  agents/unsupervised_learning/diayn.py:32-176     ProtoAgent agents/unsupervised_learning/proto.py:46-207 (states)
  DDPGAgent with obs_type='pixels': Encoder ddpg.py:12-39, pixel Actor/Critic :42-123, update :213-328 (RandomShiftsAug utils.py:222-254)
  APSAgent    agents/unsupervised_learning/aps.py:82-320       SMMAgent   agents/unsupervised_learning/smm.py:115-281 (states)
  IQLAgent    no reference file: implicit Q-learning on the offline nets (the class's docstring is its definition)
  FQEAgent    no reference file: fitted Q evaluation of a frozen policy (the class's docstring is its definition)
  PRDCAgent   no reference file: TD3+BC regularised to the nearest dataset point; defined in exorl_amd/prdc.py, reachable as agents.PRDCAgent
  ReBRACAgent no reference file: TD3+BC with a critic penalty on the dataset's next action; defined in exorl_amd/rebrac.py, agents.ReBRACAgent
  OneStepTD3BCAgent, OneStepCRRAgent   no reference file: one-step RL, the parent's step with a SARSA critic target; exorl_amd/onestep.py
  BehaviorQAgent   no reference file: FQE's machinery on the dataset's next action, Q^beta; exorl_amd/fqe.py
  CalQLAgent  no reference file: CQL bounded below by the dataset's return-to-go (Cal-QL); defined in exorl_amd/calql.py, agents.CalQLAgent

Python here is orchestration only: it builds the initial weights with torch's CPU RNG in the reference's
construction order (so a given torch.manual_seed yields the reference's initial parameters), hands batches
to the engine and — under torch.distributed — all-reduces the flat gradient buffers between update phases.
"""
import functools
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import utils
from .comm import all_ranks, native_comm
from .engine import PRECISION, AgentEngine, IntrEngine, PixelEngine, global_means

_OFFLINE_ACTOR_KEYS = ['policy.0.weight', 'policy.0.bias', 'policy.1.weight', 'policy.1.bias',
                       'policy.3.weight', 'policy.3.bias', 'policy.5.weight', 'policy.5.bias']
_OFFLINE_CRITIC_KEYS = [f'{q}.{i}.{w}' for q in ('q1_net', 'q2_net') for i in (0, 1, 3, 5) for w in ('weight', 'bias')]
_VALUE_KEYS = [f'net.{i}.{w}' for i in (0, 1, 3, 5) for w in ('weight', 'bias')]
_DDPG_ACTOR_KEYS = ['trunk.0.weight', 'trunk.0.bias', 'trunk.1.weight', 'trunk.1.bias',
                    'policy.0.weight', 'policy.0.bias', 'policy.2.weight', 'policy.2.bias']
_DDPG_CRITIC_KEYS = (['trunk.0.weight', 'trunk.0.bias', 'trunk.1.weight', 'trunk.1.bias'] +
                     [f'{q}.{i}.{w}' for q in ('Q1', 'Q2') for i in (0, 2) for w in ('weight', 'bias')])


def _mlp_init(in_dim, hidden, out_dim, n_trunks, n_heads):
    """Initial tensors of one net, drawn from torch's CPU generator in the order the reference's constructors
    consume it: every nn.Linear is default-initialised at construction, then `apply(utils.weight_init)`
    re-draws each Linear weight orthogonally and zeroes its bias (utils.py:59-69)."""
    mods = []
    if n_trunks == n_heads:                       # [trunk_i, head_i] per net (offline Actor/Critic, DDPG Actor)
        for _ in range(n_trunks):
            mods.append([nn.Linear(in_dim, hidden), nn.LayerNorm(hidden), nn.Linear(hidden, hidden), nn.Linear(hidden, out_dim)])
    else:                                         # DDPG Critic: trunk, then Q1, Q2 (ddpg.py:91-111)
        mods.append([nn.Linear(in_dim, hidden), nn.LayerNorm(hidden)])
        for _ in range(n_heads):
            mods.append([nn.Linear(hidden, hidden), nn.Linear(hidden, out_dim)])
    out = []
    for group in mods:
        for m in group:
            if isinstance(m, nn.Linear):
                nn.init.orthogonal_(m.weight.data)
                m.bias.data.fill_(0.0)
            out += [m.weight.data, m.bias.data]
    return out


class NetView:
    """Stands where the reference has an nn.Module (agent.actor / .critic / .critic_target): parameters(),
    state_dict(), load_state_dict(), train() over torch views of the engine's device buffers."""

    def __init__(self, keys, params, grads=None, on_change=None):
        """keys[i] names the tensor params[i]; grads() -> their gradient tensors (None: a copy nothing differentiates, such as a Polyak
        target outside the engine's net table); on_change() runs after the parameters were written (see _AgentBase.params_changed)."""
        self._keys, self._params, self._grads, self._on_change = list(keys), list(params), grads, on_change
        assert len(self._keys) == len(self._params), (len(self._keys), len(self._params))
        self.training = True

    def parameters(self):
        return list(self._params)

    def named_parameters(self):
        return list(zip(self._keys, self._params))

    def grads(self):
        return self._grads()

    def state_dict(self):
        return OrderedDict((k, p.detach().clone()) for k, p in zip(self._keys, self._params))

    def load_state_dict(self, sd, strict=True):
        missing = [k for k in self._keys if k not in sd]
        if strict and (missing or len(sd) != len(self._keys)):
            raise KeyError(f'state_dict mismatch: missing {missing}, unexpected {[k for k in sd if k not in self._keys]}')
        for k, p in zip(self._keys, self._params):
            if k in sd:
                p.copy_(torch.as_tensor(sd[k]).to(p.device, torch.float32).reshape(p.shape))
        if self._on_change:
            self._on_change()

    def train(self, mode=True):
        self.training = mode
        return self

    def eval(self):
        return self.train(False)


def _engine_tensors(engine, net, indices, shapes=None):
    """NetView's (params, grads) over the tensors `indices` of an engine's net; `shapes` re-views the parameters (conv weights)."""
    params = [engine.tensor(net, i, L.T_PARAM) for i in indices]
    if shapes:
        params = [p.view(*s) for p, s in zip(params, shapes)]
    return params, lambda: [engine.tensor(net, i, L.T_GRAD) for i in indices]


def _net_view(engine, net, keys, on_change=None, indices=None, shapes=None):
    """A NetView over an engine's net: all of its tensors, or the subset `indices` (agent.predictor / .projector / .protos /
    .predictor_target share Proto's module engine); a pixel engine's conv weights are exposed in torch's (co, ci, 3, 3) `shapes`."""
    if indices is None:
        n = engine.num_tensors(net)
        assert n == len(keys), (n, len(keys))
        indices = range(n)
    return NetView(keys, *_engine_tensors(engine, net, indices, shapes), on_change)


def _load(view, tensors):
    """Writes a net's initial tensors (drawn on the CPU) into its device views."""
    for p, t in zip(view.parameters(), tensors):
        p.copy_(t.reshape(p.shape))


def _conv_shapes(c):
    """torch's shapes of the Encoder's four Conv2d weights and biases (ddpg.py:12-39), c input channels."""
    return [s for l in range(4) for s in ((32, c if l == 0 else 32, 3, 3), (32,))]


def _world_size():
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        return torch.distributed.get_world_size()
    return 1


EVAL_KINDS = ('td3_bc', 'td3', 'crr', 'cql', 'bc')      # what exorl_agent_evaluate accepts: evaluate() applies to these classes (_EVALUATES)


class _AgentBase:
    KIND = None
    _evaluates_declared = False         # True on a class whose body sets _EVALUATES itself, and on its subclasses that keep its KIND

    # -- pickling (pretrain.py:293-300 torch.save's the whole agent; finetune.py:222-252 loads it back) ---------------
    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        # a class may say so itself (ReBRACAgent: TD3+BC's kind with the evaluation refused), and its subclasses inherit that unless they
        # declare a KIND of their own; every other class gets its KIND's answer
        if '_EVALUATES' in vars(cls):
            cls._evaluates_declared = True
        elif 'KIND' in vars(cls) or not cls._evaluates_declared:
            cls._EVALUATES, cls._evaluates_declared = cls.KIND in EVAL_KINDS, False
        orig = cls.__dict__.get('__init__')
        if orig is None:
            return

        @functools.wraps(orig)
        def init(self, *a, **k):
            if not hasattr(self, '_ctor'):          # outermost constructor call: remember how this agent was built
                self._ctor = (a, dict(k))
            orig(self, *a, **k)
        cls.__init__ = init

    # Per-class facts, declared next to KIND / METRICS: _build, _run_update, evaluate() and train() read these and never ask what `self` is.
    _ACTOR_KEYS, _CRITIC_KEYS = _OFFLINE_ACTOR_KEYS, _OFFLINE_CRITIC_KEYS      # the reference's state_dict names of the two nets
    _ACTOR_OUT = 1               # actor outputs per action dimension (CQL: mean and log-std)
    _CRITIC_TRUNKS = 2           # trunks under the critic's two heads: one each offline, one shared in DDPG's Critic, 0 for no critic (BC)
    _VALUE_NET = False           # IQL's V(s)
    _DRAWS_NOISE = True          # the step draws the critic target's and the actor's noise (False: noise_hook is never called)
    # defaults of what only some classes or some runs set on the instance
    training, world_size = True, 1
    _pix_meta_dim = _meta_dim = 0       # DDPG on pixels: width of the 6th batch tensor; _MetaObsMixin: meta columns appended to obs
    _second_noise_rows = None           # CRR: rows of the actor's draw
    _dp = None                          # _IntrAgent._dp_buffers, allocated on first use

    @property
    def _pixels(self):          # obs_type is an instance attribute of the DDPG family alone: the offline classes have no such public name
        return vars(self).get('obs_type') == 'pixels'

    @property
    def _logs(self):
        return bool(self.use_tb)

    # One record of the device-backed members (engines, views over their buffers, device tensors), made where each is created. The
    # constructor rebuilds them, so __getstate__ leaves them out of attrs; train() walks those with the role _TRAINS, snapshot.py those
    # with the role _NET, in the order they were recorded.
    _NET, _TRAINS = 'net', 'trains'

    def _own(self, name, member, *roles):
        vars(self).setdefault('_members', {})[name] = roles
        setattr(self, name, member)
        return member

    def _members_with(self, role):
        return [name for name, roles in self._members.items() if role in roles]

    # What else __getstate__ leaves out of attrs: the test hooks (any name ending in _hook), the buffers kept alive across a launch
    # (_keep*) and this transient step state.
    _TRANSIENT = {'_members', '_ctor', '_slots', '_graph_iter', '_graph_stddev', '_metric_window', '_dp'}
    _STATE_KEYS = ('ctor', 'flat', 'opt_steps', 'pixel', 'training', 'cql_alpha', 'intr', 'attrs')     # the pickled dict's keys, in its order

    def __getstate__(self):
        """Constructor arguments + each engine's training state (export_state: parameters, Adam moments and step counts, running
        statistics, as CPU tensors) + the host attributes that are plain data + the training flag."""
        torch.cuda.synchronize()
        st = {'pixel': self.engine.export_state()} if self._pixels else self.engine.export_state()
        if 'intr' in self._members:
            st['intr'] = self.intr.export_state()
        st.update(ctor=self._ctor, training=self.training,
                  attrs={k: v for k, v in vars(self).items()
                         if k not in self._members and k not in self._TRANSIENT and not k.endswith('_hook') and not k.startswith('_keep')})
        return {k: st[k] for k in self._STATE_KEYS if k in st}

    def __setstate__(self, st):
        a, k = st['ctor']
        rng = torch.get_rng_state()                 # construction draws initial weights; loading must not disturb the caller's stream
        self._ctor = (a, dict(k))
        type(self).__init__(self, *a, **k)
        torch.set_rng_state(rng)
        self.engine.import_state(st['pixel'] if 'pixel' in st else st)
        if 'intr' in st:
            self.intr.import_state(st['intr'])
        vars(self).update(st['attrs'])
        self.train(st['training'])

    def _build(self, obs_dim, action_dim, hidden_dim, batch_size, lr, tau, device, precision, seed, alpha=0.0, stddev_clip=0.0, **engine_kw):
        # initial weights first (CPU RNG order: actor, critic, critic_target — td3_bc.py:86-93)
        actor0 = _mlp_init(obs_dim, hidden_dim, self._ACTOR_OUT * action_dim, 1, 1)
        critic0 = value0 = None
        if self._CRITIC_TRUNKS:
            # scalar heads; with sf_dim, APSAgent builds DDPG's scalar critics first, then replaces both with CriticSF (aps.py:94-104)
            for out in (1, engine_kw['sf_dim']) if engine_kw.get('sf_dim') else (1,):
                critic0 = _mlp_init(obs_dim + action_dim, hidden_dim, out, self._CRITIC_TRUNKS, 2)
                _mlp_init(obs_dim + action_dim, hidden_dim, out, self._CRITIC_TRUNKS, 2)       # critic_target's draws, overwritten by the copy
        if self._VALUE_NET:
            value0 = _mlp_init(obs_dim, hidden_dim, 1, 1, 1)      # drawn last: actor, critic, critic_target, value
        self._dp_engine(seed, lambda ws, seed: AgentEngine(self.KIND, obs_dim, action_dim, hidden_dim, batch_size, lr=lr, tau=tau, alpha=alpha,
                                                           stddev_clip=stddev_clip, precision=precision, world_size=ws, seed=seed,
                                                           device=device, **engine_kw))
        nets = [('actor', L.NET_ACTOR, self._ACTOR_KEYS, actor0, True)]
        if critic0 is not None:
            nets += [('critic', L.NET_CRITIC, self._CRITIC_KEYS, critic0, True), ('critic_target', L.NET_CRITIC_TARGET, self._CRITIC_KEYS, None, False)]
        if value0 is not None:
            nets += [('value', L.NET_VALUE, _VALUE_KEYS, value0, True)]
        for name, net, keys, init, trains in nets:
            view = self._own(name, _net_view(self.engine, net, keys, self.params_changed), self._NET, *([self._TRAINS] if trains else []))
            if init is not None:
                _load(view, init)
        self.engine.params_changed(sync_target=True)                   # critic_target.load_state_dict(critic.state_dict())
        self.engine.set_metrics(self._logs)

    def _offline(self, obs_shape, action_shape, device, lr, hidden_dim, batch_size, use_tb, precision, seed, tau, engine=(), **hyper):
        """The head the offline constructors share: the common host attributes, then the class's own hyper-parameters `hyper` as
        attributes (plain data that rides in __getstate__'s attrs), then the engine and its views; `engine` names the hyper-parameters
        that AgentEngine takes too."""
        self.action_dim, self.hidden_dim, self.lr, self.device = action_shape[0], hidden_dim, lr, device
        self.critic_target_tau, self.use_tb = tau, use_tb
        vars(self).update(hyper)
        self._build(obs_shape[0], action_shape[0], hidden_dim, batch_size, lr, tau, device, precision, seed, **{k: hyper[k] for k in engine})

    def _train_all(self):
        """The last step of every constructor (td3_bc.py:95-96)."""
        self.train()
        if self._CRITIC_TRUNKS:
            self.critic_target.train()

    def _dp_engine(self, seed, make):
        """self.engine = make(world_size, seed) for this process, on states and on pixels: under torch.distributed the rank is folded into
        the seed and the native communicator, where there is one, is attached."""
        ws = self.world_size = _world_size()
        if ws > 1:
            # every rank draws its own rows of the global batch's shifts and noise: without this all ranks share one Philox stream and the
            # global batch repeats each noise block world_size times (the reference's single process draws B x A iid normals)
            seed = (seed + 0x9E3779B1 * torch.distributed.get_rank()) & 0x7FFFFFFFFFFFFFFF
        self._own('engine', make(ws, seed))
        if ws > 1:
            comm = native_comm(self.engine.device)          # RCCL inside the library when torch.distributed runs on nccl
            if comm is not None:
                self.engine.set_comm(comm)
        self._slots = None
        self._graph_iter = None
        self._graph_stddev = None
        self._metric_window = False
        self.noise_hook = None      # tests: callable(shape) -> np.ndarray standing in for _standard_normal (TruncatedNormal's draws)

    def params_changed(self):
        """Call after writing parameter tensors in place (copy_ on .parameters(), dist.broadcast, ...): the kernels
        read derived copies (transposed first-layer weights, bf16 hidden weights) that must be rebuilt.
        load_state_dict / init_from / utils.hard_update_params do it themselves."""
        self.engine.params_changed(sync_target=False)

    # -- nn.Module-ish surface used by utils.eval_mode and the training scripts
    def train(self, training=True):
        self.training = training
        for name in self._members_with(self._TRAINS):
            vars(self)[name].train(training)

    def _stddev(self, step):
        return utils.schedule(self.stddev_schedule, step)

    # -- hipGraph fast path: sampler + whole update captured once, replayed with one launch per step
    def enable_graph(self, replay_iter, step=0):
        """Binds `replay_iter` (an ArenaIterator with the Philox sampler) and captures sample+update.
        Returns False (and stays eager) when the iterator cannot be captured. A data-parallel step is captured too when its all-reduces
        are the library's own (RCCL, `engine.comm`): they are enqueued on the capture stream between the phases like any kernel."""
        eng = getattr(replay_iter, 'engine', None)
        if eng is None or getattr(replay_iter, 'sampler', None) != L.SAMPLER_PHILOX:
            return False
        if self.world_size != 1 and self.engine.comm is None:       # collectives in Python between the phases: nothing to capture
            return False
        self._graph_stddev = self._stddev(step)
        ok = True
        goal = getattr(replay_iter, 'goal', None) is not None      # a goal iterator: the capture takes the gather's goal path, [obs | g] rows
        try:
            (self.engine.enable_graph_goal if goal else self.engine.enable_graph)(eng, replay_iter.nstep, replay_iter.discount, self._graph_stddev)
        except L.ExorlError:
            if self.world_size == 1:
                raise
            ok = False
        if self.world_size != 1 and not all_ranks(ok, self.engine.device):      # a capture refused on one rank sends EVERY rank down the eager path
            if ok:
                self.engine.disable_graph()
            return False
        self._graph_iter = replay_iter
        return True

    # -- windowed metrics: the step's metrics accumulate in device memory and are read once per logging interval
    METRIC_WINDOW = True        # False on the classes whose update() reports more than the engine's metric block (the module agents)

    def enable_metric_window(self):
        """Collects update()'s metrics in a window on the device: update() then returns {} with no device-to-host read (whatever use_tb
        says) and pop_metrics() returns their means over the steps since the last pop. TD3+BC, TD3 and DDPG keep the fused fast path.
        Returns False, and changes nothing, for pixel agents, the module agents and under data parallelism. Call it before enable_graph
        (the capture holds the window's kernels); with a graph captured it raises. Not pickled: an unpickled agent has no window."""
        if not self.METRIC_WINDOW or self._pixels or self.world_size != 1:
            return False
        if self._graph_iter is not None:
            raise RuntimeError('enable_metric_window() must be called before enable_graph(): the captured step has no window kernels')
        self.engine.set_metric_window()
        self._metric_window = True
        return True

    def pop_metrics(self):
        """Means over the window of the keys update() returns with use_tb=True, plus metric_steps; {} when no step ran since the last
        pop. Resets the window. One small device-to-host copy: the only one of the logging interval."""
        if not self._metric_window:
            raise RuntimeError('pop_metrics() needs enable_metric_window()')
        sums, steps = self.engine.metric_window_read(reset=True)
        if steps == 0:
            return {}
        m = {name: float(sums[idx] / steps) for idx, name in self.METRICS}
        m.setdefault('actor_ent', float(sums[L.M_ACTOR_ENT] / steps))
        m['metric_steps'] = steps
        return m

    # -- held-out validation: forward-only passes over batches the agent does not train on
    def evaluate(self, replay_iter, num_batches=1, gather=None):
        """Validation without an environment: `num_batches` batches are pulled from `replay_iter` the way update() pulls its own
        (sample_into of an HBM iterator such as iter(loader).holdout, else next() of any iterator of 5-tuples) and each goes through one
        forward-only pass (AgentEngine.evaluate): no parameter, optimiser state, counter or noise draw moves, a captured graph and its bound
        iterator are not disturbed, and update() continues bit for bit as if evaluate() had not run. One device-to-host copy, at the end.
        Returns means over the rows seen, with mu the policy's mean action and y = r + discount * min_i Q'_i(s', mu(s')):
          val_bc_mse            mean over rows and action columns of (mu(s) - a)^2: does the policy still fit actions it has not trained on
          val_q_data, val_q_pi  mean min_i Q_i(s, a) and mean min_i Q_i(s, mu(s))
          val_q_gap             val_q_pi - val_q_data: is the critic's value of the policy's actions running away from the data's
          val_critic_loss       mse(Q_1(s, a), y) + mse(Q_2(s, a), y): the training key's definition with a noise-free target
          val_critic_target_q   mean y
          val_rows              rows behind the means
        BC returns val_bc_mse and val_rows only. Under an initialised torch.distributed every rank evaluates its own batches and the
        sums and row counts are added over the ranks before dividing (all_gather_object of a handful of doubles; `gather`, a callable own
        (sums, rows) -> [(sums, rows) of rank 0, of rank 1, ...], replaces that exchange). Not between the phases of a step."""
        if not self._EVALUATES or self._pixels:
            raise NotImplementedError(f'{type(self).__name__}.evaluate(): the forward-only validation pass covers TD3BCAgent, TD3Agent, '
                                      'CRRAgent, CQLAgent and BCAgent on state observations')
        eng = self.engine
        if eng._eval is None:      # the window is the engine's own torch buffer: nothing of it is pickled
            eng.set_eval()
        for _ in range(int(num_batches)):
            self._load_batch(replay_iter)
            eng.evaluate()
        own = eng.eval_read(reset=True)
        if gather is None and self.world_size != 1:
            def gather(part):
                out = [None] * torch.distributed.get_world_size()
                torch.distributed.all_gather_object(out, part)
                return out
        sums, rows = merge_eval_sums([own] if gather is None else gather(own))
        return eval_values(sums, rows, self.action_dim, self._CRITIC_TRUNKS > 0)

    def disable_graph(self):
        if self._graph_iter is not None:
            self.engine.disable_graph()
        self._graph_iter = None

    def _step(self, replay_iter, stddev):
        if replay_iter is self._graph_iter and self.noise_hook is None:
            self.engine.step_graph(stddev)            # the std lives in device memory: a moving schedule needs no re-capture
            return
        self._load_batch(replay_iter)
        self._run_update(stddev)

    def _batch_slots(self):
        if self._slots is None:
            self._slots = self.engine.batch_slots()
        return self._slots

    def _load_batch(self, replay_iter):
        """The next batch into the engine's slots, on states and on pixels (_MetaObsMixin: the [obs | meta] rows on states)."""
        eng = self.engine
        if hasattr(replay_iter, 'sample_into'):                                         # HBM sampler: replay -> update, zero copy
            replay_iter.sample_into(self._batch_slots(), eng.batch)
        else:
            batch = next(replay_iter)                                                   # any iterator of 5-tuples
            eng.set_batch(*batch[:5])
            M = self._pix_meta_dim
            if M:                                                                       # pixels: the skill / task rows, a 6th tensor
                eng.meta_rows().copy_(torch.as_tensor(batch[5]).to(eng.device, torch.float32).reshape(eng.batch, M))

    def _noise(self, rows=None):
        if self.noise_hook is None:
            return None
        return self.noise_hook((rows or self.engine.batch, self.action_dim))

    def _run_update(self, stddev):
        """One gradient step on the loaded batch."""
        nc = na = None
        if self._DRAWS_NOISE:        # reference draw order: critic target, then actor; CRR's second draw is (B*n, A) (crr.py:125)
            nc, na = self._noise(), self._noise(self._second_noise_rows)
        self.engine.run_update(stddev, nc, na)

    def _metrics(self, keys, stddev):
        raw = global_means(self.engine)
        m = {}
        for idx, name in keys:
            m[name] = float(raw[idx])
        # TruncatedNormal inherits Normal.entropy: 0.5 + 0.5 log(2 pi) + log(std), summed over action dims
        m['actor_ent'] = float(np.float32(0.5 + 0.5 * np.log(2 * np.pi) + np.log(stddev)) * self.action_dim)
        return m

    METRICS = ()                # per class: (slot, name) pairs of the engine's metrics that update() reports

    def _update_metrics(self, stddev):
        """update()'s return value on both observation types: the class's table of engine metrics, then what its module adds."""
        metrics = dict()
        if self._metric_window:         # collected on the device: pop_metrics()
            return metrics
        if self._logs:
            metrics.update(self._metrics(self.METRICS, stddev))
            self._module_metrics(metrics)
        return metrics

    def _module_metrics(self, metrics):
        pass

    # -- observation normalisation: the HBM sampler normalises what update() trains on, act() what the environment hands it
    obs_norm_mean = obs_norm_inv = None          # plain host arrays once set: they ride in __getstate__'s attrs

    def set_obs_normalizer(self, mean32, inv32):
        """act() from now on feeds the policy utils.normalize_obs(obs, mean32, inv32): the pair of a normalize_obs=True loader
        (replay_iter.obs_normalizer), whose HBM gather applies the same formula to every sampled batch. States only; for the reward-free
        agents the observation part, before meta is appended. update() on a plain iterator of 5-tuples (the H2D fallback) is NOT
        normalised: normalisation lives in the HBM sampler, such batches are trained on as they come."""
        if self._pixels:
            raise ValueError('set_obs_normalizer: pixel agents are not normalised (the encoder does its own /255 - 0.5)')
        m, w = (np.array(a, np.float32).reshape(-1) for a in (mean32, inv32))
        O = self._norm_columns()
        if m.size != O or w.size != O:
            raise ValueError(f'set_obs_normalizer: {m.size} means and {w.size} scales for {O} observation columns')
        self.obs_norm_mean, self.obs_norm_inv = m, w

    def _norm_columns(self):
        return self.engine.obs_dim

    def clear_obs_normalizer(self):
        self.obs_norm_mean = self.obs_norm_inv = None

    def _norm_obs(self, obs):
        obs = np.asarray(obs, np.float32)
        return obs if self.obs_norm_mean is None else utils.normalize_obs(obs.reshape(-1), self.obs_norm_mean, self.obs_norm_inv)

    def act(self, obs, step, eval_mode):
        return self._act(self._norm_obs(obs), step, eval_mode)

    def update(self, replay_iter, step):
        stddev = self._stddev(step)
        self._step(replay_iter, stddev)
        return self._update_metrics(stddev)

    def _act(self, obs_vec, step, eval_mode):
        stddev = self._stddev(step)
        noise = self.noise_hook((1, self.action_dim)) if (self.noise_hook and not eval_mode) else None
        explore = (not eval_mode) and step < self.num_expl_steps
        if not explore and isinstance(obs_vec, np.ndarray):
            a = self.engine.act_host(obs_vec, stddev, eval_mode, noise)      # one kernel launch, result in a pinned host slot
            if a is not None:
                return a
        if eval_mode:
            a = self.engine.act(obs_vec, stddev, True)
        else:
            a = self.engine.act(obs_vec, stddev, False, noise)
            if explore:
                a.uniform_(-1.0, 1.0)
        return a.cpu().numpy()[0]


def merge_eval_sums(parts):
    """[(sums, rows) per rank] -> (sums, rows) of all of them: float64 adds in rank order, so every rank forms the same bits."""
    total, rows = np.zeros(L.N_EVAL, np.float64), 0
    for s, r in parts:
        total = total + np.asarray(s, np.float64)
        rows += int(r)
    return total, rows


def eval_values(sums, rows, action_dim, has_critic=True):
    """evaluate()'s dict from the window's sums (L.E_*) over `rows` rows."""
    n = max(int(rows), 1)
    out = {'val_bc_mse': float(sums[L.E_BC_SQ] / (n * action_dim))}
    if has_critic:
        q_data, q_pi = float(sums[L.E_Q_DATA] / n), float(sums[L.E_Q_PI] / n)
        out.update(val_q_data=q_data, val_q_pi=q_pi, val_q_gap=q_pi - q_data,
                   val_critic_loss=float(sums[L.E_Q1_ERR] / n + sums[L.E_Q2_ERR] / n), val_critic_target_q=float(sums[L.E_TARGET_Q] / n))
    out['val_rows'] = int(rows)
    return out


class _NextActionBatch:
    """For the classes whose step reads the dataset's action at next_obs from a buffer set on the engine (ReBRACAgent: set_rebrac; the
    one-step agents and BehaviorQAgent: set_sarsa), in front of an _AgentBase class in the bases. An HBM iterator (iter(loader),
    ArenaIterator) writes next_action / next_valid into the buffer in its gather launch; a plain iterator yields
    (obs, action, reward, discount, next_obs, next_action[, next_valid]), next_valid all ones when absent."""

    def _load_batch(self, replay_iter):
        if hasattr(replay_iter, 'sample_into'):          # HBM sampler: the gather writes the next action into the slots
            return super()._load_batch(replay_iter)
        batch = next(replay_iter)
        if len(batch) < 6:
            raise ValueError(f'{type(self).__name__}: a batch of {len(batch)} tensors has no next_action: the iterator must yield (obs, action, '
                             'reward, discount, next_obs, next_action[, next_valid]), as a has_next_action=True loader does')
        self.engine.set_batch(*batch[:5])
        self.engine.set_next_action(batch[5], batch[6] if len(batch) > 6 else None)

    def _attach_sarsa(self):
        """The SARSA buffer, allocated and set on the fresh engine (AgentEngine.set_sarsa): the last step of a constructor, and so of
        unpickling. Zeros: a plain iterator's first batch may bring no next_valid."""
        eng = self.engine
        eng.set_sarsa(torch.zeros(eng.sarsa_bytes(), dtype=torch.uint8, device=eng.device))
        self._slots = None          # the slots now carry next_action / next_valid


_CRITIC_METRICS = [(L.M_BATCH_REWARD, 'batch_reward'), (L.M_CRITIC_TARGET_Q, 'critic_target_q'), (L.M_CRITIC_Q1, 'critic_q1'),
                   (L.M_CRITIC_Q2, 'critic_q2'), (L.M_CRITIC_LOSS, 'critic_loss'), (L.M_ACTOR_LOSS, 'actor_loss')]


class TD3BCAgent(_AgentBase):
    KIND = 'td3_bc'
    METRICS = _CRITIC_METRICS

    def __init__(self, name, obs_shape, action_shape, device, lr, hidden_dim, critic_target_tau, stddev_schedule, nstep,
                 batch_size, stddev_clip, use_tb, alpha, has_next_action=False, *, precision='fp32', seed=0):
        self._offline(obs_shape, action_shape, device, lr, hidden_dim, batch_size, use_tb, precision, seed, critic_target_tau,
                      ('alpha', 'stddev_clip'), stddev_schedule=stddev_schedule, stddev_clip=stddev_clip, alpha=alpha)
        self._train_all()


class TD3Agent(TD3BCAgent):
    KIND = 'td3'

    def __init__(self, name, obs_shape, action_shape, device, lr, hidden_dim, critic_target_tau, stddev_schedule, nstep,
                 batch_size, stddev_clip, use_tb, has_next_action=False, *, precision='fp32', seed=0):
        super().__init__(name, obs_shape, action_shape, device, lr, hidden_dim, critic_target_tau, stddev_schedule, nstep,
                         batch_size, stddev_clip, use_tb, 0.0, has_next_action, precision=precision, seed=seed)


class CRRAgent(_AgentBase):
    """agents/offline_learning/crr.py:59-219."""
    KIND = 'crr'
    METRICS = _CRITIC_METRICS

    def __init__(self, name, obs_shape, action_shape, device, lr, hidden_dim, critic_target_tau, num_value_samples, weight_func,
                 stddev_schedule, nstep, batch_size, stddev_clip, use_tb, has_next_action=False, *, precision='fp32', seed=0):
        assert weight_func in ['identity', 'indicator', 'exp']
        self._offline(obs_shape, action_shape, device, lr, hidden_dim, batch_size, use_tb, precision, seed, critic_target_tau,
                      ('stddev_clip', 'num_value_samples', 'weight_func'),
                      stddev_schedule=stddev_schedule, stddev_clip=stddev_clip, num_value_samples=num_value_samples, weight_func=weight_func)
        self._second_noise_rows = batch_size * num_value_samples
        self._train_all()


class IQLAgent(_AgentBase):
    """Implicit Q-learning on the offline Actor and twin Critic plus a value net V(s) (`.value`: one Q-net without the action columns, keys
    net.{0,1,3,5}.{weight,bias}). One update() on (s, a, r, D, s'), D the sampler's discount, every forward on the parameters from before the step:
        u = min(Q'_1, Q'_2)(s, a) - V(s);   L_V = mean(|expectile - 1[u < 0]| u^2)
        y = r + D V(s');                    L_Q = mse(Q_1(s, a), y) + mse(Q_2(s, a), y)
        w = min(exp(temperature u), max_weight);   L_pi = -mean(w sum_a log N(a; mu(s), std))      (CRR's actor loss with this w)
    then Adam on value, critic and actor (all at lr) and the soft update of critic_target. Nothing is sampled: the noise counter does not
    move and noise_hook is never called. No evaluate() and no metric window for this class."""
    KIND = 'iql'
    _VALUE_NET = True
    _DRAWS_NOISE = False
    METRIC_WINDOW = False
    METRICS = _CRITIC_METRICS + [(L.M_VALUE_LOSS, 'value_loss'), (L.M_VALUE, 'value'), (L.M_ADV, 'adv'), (L.M_ACTOR_WEIGHT, 'actor_weight')]

    def __init__(self, name, obs_shape, action_shape, device, lr, hidden_dim, critic_target_tau, stddev_schedule, nstep, batch_size, use_tb,
                 expectile=0.7, temperature=3.0, max_weight=100.0, has_next_action=False, *, precision='fp32', seed=0):
        self._offline(obs_shape, action_shape, device, lr, hidden_dim, batch_size, use_tb, precision, seed, critic_target_tau,
                      stddev_schedule=stddev_schedule, expectile=expectile, temperature=temperature, max_weight=max_weight)
        self.engine.set_iql(expectile, temperature, max_weight)
        self._train_all()


class _UnitStd:
    """For the classes whose step takes no exploration std from a schedule (FQE draws nothing; CQL's std is the policy's own output): the
    step's std argument is 1.0 and update() reports the class's table alone, without the base's entropy of N(mu, std)."""

    def _stddev(self, step):
        return 1.0

    def _metrics(self, keys, stddev):
        raw = global_means(self.engine)
        return {name: float(raw[idx]) for idx, name in keys}


def merge_fqe_sums(parts):
    """[(sums, rows, return_sum, return_count) per rank] -> the same four over all of them: float64 adds in rank order, as merge_eval_sums,
    so every rank forms the same bits."""
    total, rows, g_sum, g_n = np.zeros(L.N_FQE_VALUE, np.float64), 0, np.float64(0.0), 0
    for s, r, g, n in parts:
        total = total + np.asarray(s, np.float64)
        rows += int(r)
        g_sum = g_sum + np.float64(g)
        g_n += int(n)
    return total, rows, float(g_sum), g_n


def fqe_values(sums, rows, return_sum, return_count):
    """FQEAgent.value()'s dict from the value window's sums (L.FQE_V_*) over `rows` episodes and the sum of `return_count` episode returns."""
    n = max(int(rows), 1)
    q1, q2 = float(sums[L.FQE_V_Q1] / n), float(sums[L.FQE_V_Q2] / n)
    mean = float((sums[L.FQE_V_Q1] + sums[L.FQE_V_Q2]) / (2 * n))
    # sample variance of the per-episode (Q_1 + Q_2) / 2 from its sum of squares (float64 from the rows on); one episode has no spread
    var = max(float(sums[L.FQE_V_MEAN_SQ] - n * mean * mean) / (n - 1), 0.0) if n > 1 else 0.0
    return {'fqe_value': mean, 'fqe_value_q1': q1, 'fqe_value_q2': q2, 'fqe_value_stderr': float(np.sqrt(var / n)),
            'fqe_twin_rms': float(np.sqrt(max(float(sums[L.FQE_V_DIFF_SQ]), 0.0) / n)),
            'behavior_value': float(return_sum / max(int(return_count), 1)), 'episodes': int(rows)}


class FQEAgent(_UnitStd, _AgentBase):
    """Fitted Q evaluation: scores a FROZEN policy from the dataset alone. The actor is the policy (set_policy / for_policy) and is never
    stepped: no gradient, no Adam pass, its weight images are not rewritten. A fresh twin critic with its Polyak target, in TD3's offline
    layout, is regressed on the policy's own Bellman target. One update() on (s, a, r, D, s'), D the sampler's discount, every forward on the
    parameters from before the step, mu the actor's mean action:
        y_i = r + D Q'_i(s', mu(s'))    per net, with its OWN target: no min over the twins. FQE is an estimate, not a pessimistic bound;
                                        the two nets are a two-member ensemble and their disagreement is reported (fqe_twin_rms)
        L = mse(Q_1(s, a), y_1) + mse(Q_2(s, a), y_2);   Adam on the critic, soft update of critic_target
    Nothing is sampled: the noise counter does not move and noise_hook is never called. value() reads the estimate. The replay must run
    nstep = 1 (the offline loaders do): an n-step target follows the BEHAVIOUR policy's actions for n - 1 steps and biases the estimate
    towards the behaviour value. No evaluate() and no metric window for this class."""
    KIND = 'fqe'
    _DRAWS_NOISE = False
    METRIC_WINDOW = False
    METRICS = _CRITIC_METRICS[:5]
    POLICY_CLASSES = ('TD3BCAgent', 'TD3Agent', 'BCAgent', 'CRRAgent', 'IQLAgent')

    def __init__(self, name, obs_shape, action_shape, device, lr, hidden_dim, critic_target_tau, nstep, batch_size, use_tb, *,
                 precision='fp32', seed=0):
        self.obs_shape = tuple(obs_shape)
        self._offline(obs_shape, action_shape, device, lr, hidden_dim, batch_size, use_tb, precision, seed, critic_target_tau, nstep=nstep)
        self._train_all()

    @staticmethod
    def _check_policy(agent, dims=None, who='FQEAgent'):
        """ValueError unless `agent` is one of POLICY_CLASSES and, with dims = the evaluator's (obs_dim, action_dim, hidden_dim), of that shape.
        who: the class the caller used, for the message."""
        if type(agent).__name__ not in FQEAgent.POLICY_CLASSES or not isinstance(agent, _AgentBase):
            raise ValueError(f'{who}: cannot evaluate a {type(agent).__name__}: the frozen actor is the offline tanh-mean Actor of '
                             'TD3BCAgent, TD3Agent, BCAgent, CRRAgent or IQLAgent. CQLAgent (a 2A-wide tanh-Gaussian head) and the DDPG '
                             'family (a trunk / policy layout) are out of scope')
        theirs = (agent.engine.obs_dim, agent.engine.act_dim, agent.engine.hidden_dim)
        if dims is not None and tuple(dims) != theirs:
            raise ValueError(f'{who}.set_policy: (obs_dim, action_dim, hidden_dim) = {theirs} of the policy, {tuple(dims)} of the evaluator')

    def set_policy(self, agent):
        """Copies `agent`'s actor (the policy to score) and its observation normaliser. ValueError for a class other than TD3BCAgent,
        TD3Agent, BCAgent, CRRAgent and IQLAgent (CQLAgent's 2A-wide head and the DDPG family's trunk layout are out of scope) or when
        obs_dim, action_dim or hidden_dim differ."""
        self._check_policy(agent, (self.engine.obs_dim, self.engine.act_dim, self.engine.hidden_dim), type(self).__name__)
        self.actor.load_state_dict(agent.actor.state_dict())
        if agent.obs_norm_mean is not None:
            self.set_obs_normalizer(agent.obs_norm_mean, agent.obs_norm_inv)
        else:
            self.clear_obs_normalizer()
        return self

    @classmethod
    def for_policy(cls, agent, **overrides):
        """An evaluator shaped after `agent` with its actor copied in: obs / action / hidden sizes, device, batch size and precision are the
        policy's, lr and critic_target_tau its own where it has them (else 1e-4 and 0.01); `overrides` replaces any constructor argument."""
        cls._check_policy(agent, who=cls.__name__)
        eng = agent.engine
        prec = {v: k for k, v in reversed(list(PRECISION.items()))}[eng.cfg.precision]
        kw = dict(name='fqe', obs_shape=(eng.obs_dim,), action_shape=(eng.act_dim,), device=agent.device, lr=getattr(agent, 'lr', 1e-4),
                  hidden_dim=eng.hidden_dim, critic_target_tau=getattr(agent, 'critic_target_tau', 0.01), nstep=1, batch_size=eng.batch,
                  use_tb=False, precision=prec, seed=0)
        kw.update(overrides)
        return cls(**kw).set_policy(agent)

    def act(self, obs, step=0, eval_mode=True):
        """The frozen policy's mean action, whatever eval_mode says."""
        return self._act(self._norm_obs(obs), step, True)

    def value(self, replay_iter, gather=None):
        """The policy's value from the critic as it stands: Q(s_0, mu(s_0)) over the first observation of EVERY resident episode of every
        arena `replay_iter` samples from (its episode_starts(): an ArenaIterator, a loader's iterator or its .holdout), each once, through
        forward-only passes (AgentEngine.fqe_value) that move no parameter, optimiser state or counter; the iterator's Philox stream and a
        captured graph bound to it are not disturbed, and update() continues bit for bit. Returns
          fqe_value                      mean over episodes of (Q_1 + Q_2) / 2 at (s_0, mu(s_0))
          fqe_value_q1, fqe_value_q2     the two nets' means separately
          fqe_value_stderr               standard error of fqe_value over episodes
          fqe_twin_rms                   root-mean-square of Q_1 - Q_2
          behavior_value                 mean discounted return of the episodes themselves (episode_returns()): the anchor to read against
          episodes                       episodes behind the means
        Under an initialised torch.distributed every rank covers its own arenas and the sums and counts are added in rank order before
        dividing (all_gather_object; `gather`, a callable own part -> [part of rank 0, of rank 1, ...], replaces that exchange)."""
        if not hasattr(replay_iter, 'episode_starts'):
            raise ValueError('FQEAgent.value(): needs an HBM iterator (ArenaIterator, iter(loader) or its .holdout): it enumerates the '
                             'episodes resident in the arena')
        eng = self.engine
        if eng._fqe_value is None:      # the window is the engine's own torch buffer: nothing of it is pickled
            eng.set_fqe_value()
        for _, rows in replay_iter.episode_starts(eng.batch, self._batch_slots()):
            eng.fqe_value(rows)
        sums, rows = eng.fqe_value_read(reset=True)
        g = replay_iter.episode_returns()
        own = (sums, rows, float(np.sum(g, dtype=np.float64)), int(g.size))
        if gather is None and self.world_size != 1:
            def gather(part):
                out = [None] * torch.distributed.get_world_size()
                torch.distributed.all_gather_object(out, part)
                return out
        return fqe_values(*merge_fqe_sums([own] if gather is None else gather(own)))


class CQLAgent(_UnitStd, _AgentBase):
    """agents/offline_learning/cql.py:59-286 (both the shipped cql.yaml and use_critic_lagrange=True; under torch.distributed the latter splits
    phase 0 around a sum-all-reduce of the penalty, _run_update)."""
    KIND = 'cql'
    _ACTOR_OUT = 2               # a tanh-Gaussian head: mean and log-std per action
    METRICS = _CRITIC_METRICS + [(L.M_CRITIC_CQL, 'critic_cql'), (L.M_CRITIC_CQL_LOGSUM, 'critic_cql_logsum'), (L.M_ACTOR_ENT, 'actor_ent'),
                                 (L.M_ACTOR_ALPHA, 'actor_alpha'), (L.M_ACTOR_ALPHA_LOSS, 'actor_alpha_loss')]

    def __init__(self, name, obs_shape, action_shape, device, lr, hidden_dim, critic_target_tau, nstep, batch_size, use_tb, alpha,
                 n_samples, target_cql_penalty, use_critic_lagrange, has_next_action=False, *, precision='fp32', seed=0):
        # stddev_schedule: unused by CQL (state-dependent std); keeps the shared plumbing uniform
        self._offline(obs_shape, action_shape, device, lr, hidden_dim, batch_size, use_tb, precision, seed, critic_target_tau,
                      ('alpha', 'n_samples', 'use_critic_lagrange', 'target_cql_penalty'),
                      use_critic_lagrange=use_critic_lagrange, target_cql_penalty=target_cql_penalty, alpha=alpha, n_samples=n_samples,
                      target_entropy=-action_shape[0], stddev_schedule='1.0')
        self._train_all()

    @property
    def log_actor_alpha(self):
        return torch.tensor([self.engine.cql_alpha_state()[0]])

    @property
    def log_critic_alpha(self):
        return torch.tensor([self.engine.cql_alpha_state()[3]])

    def _noise(self, rows=None):
        raise RuntimeError('CQL draws five noise tensors; see _run_update')

    def _run_update(self, stddev):
        B, A, n = self.engine.batch, self.action_dim, self.n_samples
        if self.noise_hook is None:
            nc = na = None
        else:       # draw order cql.py:159,170-176,238; the hook returns N(0,1) except for the uniform(-1,1) random actions
            z_next = self.noise_hook((B, A))
            u_rand = self.noise_hook((n, B, A), 'uniform')
            z_cur, z_nxt = self.noise_hook((n, B, A)), self.noise_hook((n, B, A))
            nc = np.concatenate([np.asarray(x, np.float32).reshape(-1) for x in (z_next, u_rand, z_cur, z_nxt)])
            na = np.asarray(self.noise_hook((B, A)), np.float32)
        self.engine.run_update(stddev, nc, na)


class BCAgent(_AgentBase):
    KIND = 'bc'
    _CRITIC_TRUNKS = 0
    _DRAWS_NOISE = False
    METRICS = [(L.M_BATCH_REWARD, 'batch_reward'), (L.M_ACTOR_LOSS, 'actor_loss')]

    def __init__(self, name, obs_shape, action_shape, device, lr, hidden_dim, batch_size, stddev_schedule, use_tb,
                 has_next_action=False, *, precision='fp32', seed=0):
        self.lr = lr
        self.action_dim = action_shape[0]
        self.hidden_dim = hidden_dim
        self.device = device
        self.stddev_schedule = stddev_schedule
        self.use_tb = use_tb
        self._build(obs_shape[0], action_shape[0], hidden_dim, batch_size, lr, 0.0, device, precision, seed)
        self._train_all()


class DDPGAgent(_AgentBase):
    KIND = 'ddpg'
    _ACTOR_KEYS, _CRITIC_KEYS, _CRITIC_TRUNKS = _DDPG_ACTOR_KEYS, _DDPG_CRITIC_KEYS, 1
    METRICS = _CRITIC_METRICS + [(L.M_ACTOR_LOGPROB, 'actor_logprob')]

    def __init__(self, name, reward_free, obs_type, obs_shape, action_shape, device, lr, feature_dim, hidden_dim,
                 critic_target_tau, num_expl_steps, update_every_steps, stddev_schedule, nstep, batch_size, stddev_clip,
                 init_critic, use_tb, use_wandb, meta_dim=0, skill_type='uniform', *, precision='fp32', seed=0):
        pixels = obs_type == 'pixels'
        if pixels and not self._PIXELS_OK:
            raise NotImplementedError(f"exorl_amd: obs_type='pixels' is not built for {type(self).__name__} yet (DDPG, Proto, ICM, ICM-APT, "
                                      "Disagreement, DIAYN, APS, SMM and RND are)")
        if obs_type not in ('pixels', 'states'):
            raise NotImplementedError(f"exorl_amd DDPGAgent: unknown obs_type {obs_type!r}")
        if (pixels and reward_free and isinstance(self, ProtoAgent) and not self.shard_pretraining and
                _world_size() > 1):
            raise NotImplementedError(f"exorl_amd: {type(self).__name__}(obs_type='pixels', reward_free=True) is single-GPU by default: Proto is the "
                                      "one pixel agent whose sharded pretraining step is opt-in (its candidate queue draws rows from the global "
                                      "batch's softmax and its Sinkhorn runs over the batch; every rank gathers the rows and runs both "
                                      "redundantly). Pass shard_pretraining=True (Hydra: +agent.shard_pretraining=true) to shard it. Under data "
                                      "parallelism the pixel path runs every agent with reward_free=False (fine-tuning: the DDPG pixel step) and "
                                      "every other agent's pretraining step")
        self.reward_free = reward_free
        self.obs_type = obs_type
        self.action_dim = action_shape[0]
        self.hidden_dim = hidden_dim
        self.lr = lr
        self.device = device
        self.critic_target_tau = critic_target_tau
        self.update_every_steps = update_every_steps
        self.use_tb = use_tb
        self.use_wandb = use_wandb
        self.num_expl_steps = num_expl_steps
        self.stddev_schedule = stddev_schedule
        self.stddev_clip = stddev_clip
        self.init_critic = init_critic
        self.feature_dim = feature_dim
        self.solved_meta = None
        self._precision = precision
        if pixels:
            self.obs_shape, self._pix_meta_dim = tuple(obs_shape), meta_dim
            self._init_pixels(obs_shape, batch_size, seed, meta_dim)
        else:
            self.obs_shape = obs_shape
            self.obs_dim = obs_shape[0] + meta_dim
            self._own('encoder', self._own('aug', _Identity()), self._TRAINS)
            self.encoder_opt = None
            self._build(self.obs_dim, action_shape[0], hidden_dim, batch_size, lr, critic_target_tau, device, precision, seed,
                        stddev_clip=stddev_clip, **self._engine_kw())
        self._train_all()

    _PIXELS_OK = True           # obs_type='pixels' is built for this class (False on _IntrAgent: every module class states it)

    @property
    def _logs(self):
        return bool(self.use_tb or self.use_wandb)

    def _norm_columns(self):
        return self.obs_shape[0]                # without the reward-free agents' meta columns

    def _engine_kw(self):
        return {}

    # ---- obs_type == 'pixels' (ddpg.py:12-39 Encoder, :42-123 pixel Actor/Critic, :213-328) -----------------------------------------
    def _init_pixels(self, obs_shape, batch_size, seed, meta_dim):
        c = obs_shape[0]
        sf_dim = self._engine_kw().get('sf_dim', 0)         # APS: CriticSF heads (aps.py:94-104)
        w = _pixel_init(c, obs_shape[1], self.action_dim, self.feature_dim, self.hidden_dim, meta_dim, sf_dim)
        self._dp_engine(seed, lambda ws, seed: PixelEngine(obs_shape, self.action_dim, self.feature_dim, self.hidden_dim, batch_size, lr=self.lr,
                                                           tau=self.critic_target_tau, stddev_clip=self.stddev_clip,
                                                           precision=self._precision, seed=seed, device=self.device, meta_dim=meta_dim,
                                                           sf_dim=sf_dim, world_size=ws))
        self.obs_dim = w['repr_dim'] + meta_dim          # ddpg.py:176 obs_dim = encoder.repr_dim + meta_dim
        self._own('encoder', _net_view(self.engine, 0, _ENC_KEYS, shapes=_conv_shapes(c)), self._NET, self._TRAINS)
        self._own('actor', _net_view(self.engine, 1, _PIX_ACTOR_KEYS), self._NET, self._TRAINS)
        self._own('critic', _net_view(self.engine, 2, _PIX_CRITIC_KEYS), self._NET, self._TRAINS)
        self._own('critic_target', _net_view(self.engine, 3, _PIX_CRITIC_KEYS), self._NET)
        for view, ts in ((self.encoder, w['encoder']), (self.actor, w['actor']), (self.critic, w['critic'])):
            _load(view, ts)
        self.engine.sync_target()
        self._own('aug', _Identity())
        self.encoder_opt = True            # the reference's `if self.encoder_opt is not None` checks hold for pixels
        self.shift_hook = None             # tests: callable(batch) -> (batch, 2) RandomShiftsAug draws

    def _shifts(self):
        """One RandomShiftsAug draw for the batch (None: the engine draws its own)."""
        return self.shift_hook(self.engine.batch) if self.shift_hook else None

    def _pix_before_step(self):
        """What a class does on the loaded frames before the DDPG step; returns how engine.run_update takes its images: fresh shifts
        (here), or keep_augmented / keep_encoded for those a module agent has augmented or encoded already."""
        return dict(shifts_obs=self._shifts(), shifts_next=self._shifts())

    def _pix_after_step(self):
        pass

    def _update_pixels(self, replay_iter, step):
        self._load_batch(replay_iter)
        images = self._pix_before_step()
        stddev = self._stddev(step)
        # reference draw order: the augmentations, then the critic target's noise, then the actor's
        self.engine.run_update(stddev, noise_critic=self._noise(), noise_actor=self._noise(), **images)
        self._pix_after_step()
        return self._update_metrics(stddev)

    def init_from(self, other):
        if self.obs_type == 'pixels':
            utils.hard_update_params(other.encoder, self.encoder)
        utils.hard_update_params(other.actor, self.actor)
        if self.init_critic:          # critic.trunk = first 4 tensors (ddpg.py:209-210)
            for p, t in zip(other.critic.parameters()[:4], self.critic.parameters()[:4]):
                t.copy_(p)
        self.params_changed()

    def get_meta_specs(self):
        return tuple()

    def init_meta(self):
        return OrderedDict()

    def update_meta(self, meta, global_step, time_step, finetune=False):
        return meta

    def act(self, obs, meta, step, eval_mode):
        if self.obs_type == 'pixels':
            stddev = self._stddev(step)
            noise = self.noise_hook((1, self.action_dim)) if (self.noise_hook and not eval_mode) else None
            mv = np.concatenate([np.asarray(v, np.float32).reshape(-1) for v in meta.values()]) if self._pix_meta_dim else None
            a = self.engine.act(np.ascontiguousarray(obs), stddev, eval_mode, noise, mv)
            if not eval_mode and step < self.num_expl_steps:
                a.uniform_(-1.0, 1.0)
            return a.cpu().numpy()
        parts = [self._norm_obs(obs).reshape(-1)] + [np.asarray(v, np.float32).reshape(-1) for v in meta.values()]
        return self._act(np.concatenate(parts), step, eval_mode)

    def update(self, replay_iter, step):
        if step % self.update_every_steps != 0:      # ddpg.py:302-303 — no batch is consumed
            return dict()
        if self.obs_type == 'pixels':
            return self._update_pixels(replay_iter, step)
        return super().update(replay_iter, step)


def _seq_init(spec):
    """Initial tensors of an nn.Sequential-style module: spec = [('lin', in, out) | ('ln', dim)]. Same RNG consumption as the
    reference constructors: all Linears default-initialised at construction, then apply(utils.weight_init) in order."""
    mods = [nn.Linear(s[1], s[2]) if s[0] == 'lin' else nn.LayerNorm(s[1]) for s in spec]
    out = []
    for m in mods:
        if isinstance(m, nn.Linear):
            nn.init.orthogonal_(m.weight.data)
            m.bias.data.fill_(0.0)
        out += [m.weight.data, m.bias.data]
    return out


_RND_KEYS = [f'{n}.{i}.{w}' for n in ('predictor', 'target') for i in (1, 3, 5) for w in ('weight', 'bias')]
_ICM_KEYS = [f'{n}.{i}.{w}' for n in ('forward_net', 'backward_net') for i in (0, 2) for w in ('weight', 'bias')]
_APT_KEYS = ['trunk.0.weight', 'trunk.0.bias', 'trunk.1.weight', 'trunk.1.bias'] + _ICM_KEYS


class _RndView(NetView):
    """agent.rnd: the parameters plus BatchNorm1d's buffers under the reference's state_dict keys (rnd.py:24-27)."""

    def __init__(self, intr):
        super().__init__(_RND_KEYS, *_engine_tensors(intr, None, range(len(_RND_KEYS))))
        self._intr = intr

    def _bn(self):
        O = self._intr.obs_dim
        bn = self._intr.bn
        return bn[:O], bn[O:2 * O], bn[2 * O:]

    def state_dict(self):
        mean, var, cnt = self._bn()
        sd = OrderedDict([('normalize_obs.running_mean', mean.clone()), ('normalize_obs.running_var', var.clone()),
                          ('normalize_obs.num_batches_tracked', cnt.clone().long().reshape(()))])
        sd.update(super().state_dict())
        return sd

    def load_state_dict(self, sd, strict=True):
        sd = dict(sd)
        mean, var, cnt = self._bn()
        for k, dst in (('normalize_obs.running_mean', mean), ('normalize_obs.running_var', var), ('normalize_obs.num_batches_tracked', cnt)):
            if k in sd:
                dst.copy_(torch.as_tensor(sd.pop(k)).to(dst.device, torch.float32).reshape(dst.shape))
            elif strict:
                raise KeyError(f'state_dict mismatch: missing {k}')
        super().load_state_dict(sd, strict)


class _RmsView:
    """Stands where the reference has a utils.RMS object (agent.intrinsic_reward_rms / agent.pbe.rms): .M, .S, .n."""

    def __init__(self, engine):
        self._engine = engine

    M = property(lambda self: torch.tensor([self._engine.rms_state()[0]]))
    S = property(lambda self: torch.tensor([self._engine.rms_state()[1]]))
    n = property(lambda self: self._engine.rms_state()[2])


class _IntrAgent(DDPGAgent):
    """Shared update() of the reward-free agents (rnd.py:110-159, icm.py:94-139, icm_apt.py:112-158): module step and
    intrinsic reward on the sampled batch (libexorl_hip: exorl_intr_update), then the DDPG update on that reward."""
    METRIC_WINDOW = False       # the modules' metrics live in their own engines
    MODULE_METRICS = ()         # per class: (slot, name) pairs of the module's metrics reported while reward_free (_module_table)
    STATE_METRICS = ()          # ... and those reported on state observations only
    _HOOKS = ('noise_hook', 'cat_hook', 'eps_hook')      # the test hooks of the state step, each on the classes that draw it
    _PIXELS_OK = False

    def __init__(self, shard_pretraining=False, **kwargs):
        self.shard_pretraining = bool(shard_pretraining)        # before the base constructor: Proto's pixel refusal reads it
        super().__init__(**kwargs)

    def _module(self, kind, obs_dim, hidden_dim, keys, tensors, dp=None, name=None, **kw):
        """The tail of every subclass constructor: builds the module engine self.intr from the shared arguments plus the kind's own
        keywords and allocates the pixel path's gradient buffer. With `keys`, the module's tensors under the reference's state_dict names
        become the view self.<name> (default: the kind) and take the initial `tensors`; None: the subclass wraps them itself."""
        self._own('intr', IntrEngine(kind, obs_dim, self.action_dim, hidden_dim, **(self._intr_dp() if dp is None else dp), lr=self.lr,
                                     precision=self._precision, device=self.device, **kw))
        if keys is not None:
            _load(self._own(name or kind, _net_view(self.intr, None, keys), self._NET), tensors)
        if self.obs_type == 'pixels':       # d(module loss)/d(encoding), see _pix_module
            self._own('_dobs', torch.zeros(self.engine.batch, self.obs_dim - self._pix_meta_dim, dtype=torch.float32, device=self.engine.device))

    def _intr_args(self):
        """The module's view of the batch slots on states: IntrEngine.update's five pointers and its stride keywords."""
        s = self._batch_slots()
        return (s.obs, s.action, s.next_obs, s.reward, s.reward), {}

    def _intr_hooks(self):
        """Host-supplied draws of the module step (tests): IntrEngine.update keywords; empty when no hook is set."""
        return {}

    def _intr_step(self):
        a, k = self._intr_args()
        self.intr.run_update(*a, True, **k, **self._intr_hooks())

    def _hooked(self):
        return any(vars(self).get(h) is not None for h in self._HOOKS)

    def _refuse_goal(self, replay_iter):
        if getattr(replay_iter, 'goal', None) is not None:
            raise ValueError(f'{type(self).__name__}: a goal iterator (goal=GoalRelabel) relabels the reward and fills [obs | g] rows; the '
                             'reward-free agents train on their own intrinsic reward with the skill behind the observation: goal '
                             'conditioning covers the offline state agents')

    def enable_graph(self, replay_iter, step=0):
        """One hipGraph per update on state observations in one process: sample -> module step and intrinsic reward -> DDPG step
        (reward_free), or sample -> DDPG step (fine-tuning: the module is not stepped). Returns False and stays eager on pixels, under
        torch.distributed (the replicated and the sharded module step run their collectives in Python), for an iterator without the
        Philox HBM sampler, and while a test hook supplies draws from the host. A hook set later sends that step down the eager path."""
        self._refuse_goal(replay_iter)
        eng = getattr(replay_iter, 'engine', None)
        if (self.obs_type != 'states' or self.world_size != 1 or eng is None or getattr(replay_iter, 'sampler', None) != L.SAMPLER_PHILOX or
                self._hooked()):
            return False
        self._graph_stddev = self._stddev(step)
        intr = batch = None
        if self.reward_free:
            a, k = self._intr_args()
            intr, batch = self.intr, self.intr._batch(*a, **k)
        self.engine.enable_graph_intr(eng, replay_iter.nstep, replay_iter.discount, self._graph_stddev, intr, batch, self._meta_dim)
        self._graph_iter = replay_iter
        return True

    # ---- data parallel (last row) ----------------------------------------------------------------------------------------
    # What these modules compute is batch-global: BatchNorm statistics and the running RMS of the rewards (rnd.py:24,47-60,
    # utils.py:257-276), kNN particle entropy over the batch (utils.py:279-319), Sinkhorn normalisation and the candidate queue
    # (proto.py:114-157), SMM's mean_j log p*(s_j), and each steps its own optimiser on a batch mean. Under torch.distributed every rank
    # therefore all-gathers the sampled rows (one collective of B x (2 obs + act + 1) floats, <= 0.3 MB per rank at the shipped widths)
    # and runs the module step on the GLOBAL batch: the kernels are deterministic, so the replicas of the module stay bit-identical
    # without a gradient exchange, every statistic is the single-process one, and each rank keeps its own rows of the reward. The
    # actor / critic step — the 1024-wide layers, 35 of the step's ~45 GFLOP — runs sharded like the offline agents' (_run_update).
    # That replicated step is the default (its replicas equal the single process bit for bit). With shard_pretraining=True the module step
    # is sharded on states as it is on pixels: each rank runs the module on its own rows through IntrEngine.run_update, the gradients are
    # summed, and the batch-global statistics travel as small exchanges — RND's BatchNorm1d moments, the RMS moments, the kNN targets of
    # ICM-APT and APS, Proto's target and reward rows, SMM's moments of log p*. No rows are gathered and each rank's rewards land in its
    # own reward slot. The gradient sum's order differs from the single process's, so the replicas agree with it to rounding only.
    shard_pretraining = False

    @property
    def _module_batch(self):
        return self.engine.batch * self.world_size

    def _intr_dp(self):
        """IntrEngine's batch arguments. Under torch.distributed the module is sharded on pixels, and on states where shard_pretraining asks
        for it: this rank's rows, with world_size and rank (exorl_intr_update_phase and its exchanges). Otherwise it stays replicated on
        the gathered global batch (_intr_step_dp)."""
        if self.world_size > 1 and (self.obs_type == 'pixels' or self._sharded_states):
            return dict(batch=self.engine.batch, world_size=self.world_size, rank=torch.distributed.get_rank())
        return dict(batch=self._module_batch)

    @property
    def _sharded_states(self):
        return self.obs_type == 'states' and self.shard_pretraining and self.reward_free and self.world_size > 1

    def _dp_buffers(self):
        if self._dp is None:
            eng, ws = self.engine, self.world_size
            B, W, A = eng.batch, self.obs_dim, self.action_dim
            dev = eng.device
            pack = torch.empty(B, 2 * W + A + 1, device=dev)
            gpack = torch.empty(ws * B, 2 * W + A + 1, device=dev)
            g = dict(obs=torch.empty(ws * B, W, device=dev), action=torch.empty(ws * B, A, device=dev),
                     next_obs=torch.empty(ws * B, W, device=dev), reward=torch.empty(ws * B, device=dev))
            O = W - self._meta_dim
            slots = L.BatchOut(g['obs'].data_ptr(), W, g['action'].data_ptr(), A, g['reward'].data_ptr(), None, g['next_obs'].data_ptr(), W,
                               g['obs'].data_ptr() + 4 * O, W)
            self._dp = (pack, gpack, g, slots)
        return self._dp

    def _intr_step_dp(self):
        dist = torch.distributed
        eng, ws, rank = self.engine, self.world_size, torch.distributed.get_rank()
        B, W, A = eng.batch, self.obs_dim, self.action_dim
        local = self._batch_slots()
        pack, gpack, g, gslots = self._dp_buffers()
        view = lambda ptr, cols: eng._view(ptr, B * cols).view(B, cols)
        pack[:, :W].copy_(view(local.obs, W))
        pack[:, W:2 * W].copy_(view(local.next_obs, W))
        pack[:, 2 * W:2 * W + A].copy_(view(local.action, A))
        pack[:, 2 * W + A].copy_(eng._view(local.reward, B))
        dist.all_gather(list(gpack.split(B)), pack)              # rows in rank order = the single-process batch of the equivalence test
        g['obs'].copy_(gpack[:, :W])
        g['next_obs'].copy_(gpack[:, W:2 * W])
        g['action'].copy_(gpack[:, 2 * W:2 * W + A])
        g['reward'].copy_(gpack[:, 2 * W + A])
        self._slots = gslots
        try:
            self._intr_step()                                    # module optimiser step + rewards of all ws * B rows, identical on every rank
        finally:
            self._slots = local
        eng._view(local.reward, B).copy_(g['reward'][rank * B:(rank + 1) * B])

    # ---- obs_type == 'pixels' ---------------------------------------------------------------------------------------------------
    # Every one of these agents augments and encodes obs and next_obs ONCE (icm.py:97-99, icm_apt.py:113-118, disagreement.py:98-100,
    # diayn.py:137-138), steps its module AND the encoder on the module's loss (encoder_opt.step() inside update_<module>), takes the
    # intrinsic reward from the updated module on the encodings computed before that step, and hands the critic and the actor those same
    # encodings detached (`update_critic(obs.detach(), ...)`): after the module step nothing else moves the encoder, and encoder_opt's
    # second .step() inside update_critic finds no gradients (Adam skips parameters whose .grad is None, step counts included).
    _PIX_GRAD = 0                        # which encoding carries the graph into the module's loss: 0 obs, 1 next_obs

    # Under torch.distributed every rank runs the module step, the encoder step and BatchNorm2d on its own rows: each loss is a mean over
    # the global batch, so the gradients are partial sums the ranks add up (one exchange each), and the batch-global quantities — RND's
    # BatchNorm2d statistics, the running RMS's batch moments, the kNN targets of ICM-APT and APS — are small exchanges of their own.
    # The engines' run_* calls (engine.py) take the phased forms in that case.
    def _intr_metrics(self):
        """The module's metrics as global means; the RMS state (slots 3, 4 of RND, ICM-APT and APS) and SMM's mean and variance of log p*
        on states (slots 3, 7) are the same on every rank and are not summed."""
        keep = None
        if self.intr.kind in ('rnd', 'icm_apt', 'aps'):
            keep = slice(L.IM_RMS_MEAN, L.IM_RMS_STD + 1)
        elif self.intr.kind == 'smm' and self.obs_type == 'states':
            keep = [3, 7]
        return global_means(self.intr, keep)

    def _pix_module(self, fo, fn, s):
        """Module step + intrinsic reward on the encodings (device pointers); d(loss)/d(encoding) lands in self._dobs."""
        self.intr.run_update(fo, s.action, fn, s.reward, s.reward, True, dobs_out=self._dobs.data_ptr())

    def _pix_before_step(self):
        eng = self.engine
        eng.augment(self._shifts(), self._shifts())         # drawn in fine-tuning too
        fo, fn = eng.encode(0), eng.encode(1)
        if self.reward_free:
            self._pix_module(fo, fn, self._batch_slots())
            eng.run_encoder_step(self._PIX_GRAD, self._dobs.data_ptr(), 0)
        eng.set_train_encoder(False)
        return dict(keep_encoded=True)

    def _module_metrics(self, metrics):
        if self.reward_free:
            raw = self._intr_metrics()              # a replicated module's engine has world_size 1: its own metrics
            table = self.MODULE_METRICS + (self.STATE_METRICS if self.obs_type == 'states' else ())
            metrics.update((name, float(raw[slot])) for slot, name in table)
        else:
            metrics['extr_reward'] = metrics['batch_reward']

    def _step(self, replay_iter, stddev):
        self._refuse_goal(replay_iter)
        if replay_iter is self._graph_iter and not self._hooked():
            self.engine.step_graph(stddev)            # the module's counters and the std live in device memory: no re-capture
            return
        self._load_batch(replay_iter)
        if self.reward_free:
            if self.world_size != 1 and not self._sharded_states:
                self._intr_step_dp()
            else:
                self._intr_step()
        self._run_update(stddev)


def _module_table(loss_key, *more):
    """A class's MODULE_METRICS: the three every module reports, its loss under the reference's name, then its own."""
    return ((L.IM_LOSS, loss_key), (L.IM_INTR_REWARD, 'intr_reward'), (L.IM_EXTR_REWARD, 'extr_reward')) + more


class _RndPixelView(_RndView):
    """agent.rnd on pixels (rnd.py:13-45): normalize_obs is a BatchNorm2d over the frames (buffers in the pixel engine), predictor.0 IS the
    agent's encoder, target.0 its frozen copy (the pixel engine's encoder_target slot); the six Linear layers live in the module engine."""

    def __init__(self, intr, pixel, encoder_view, target_view):
        super().__init__(intr)
        self._pixel, self._enc, self._tgt = pixel, encoder_view, target_view

    def _bn(self):
        b = self._pixel.bn2d()
        c = (b.numel() - 1) // 2
        return b[:c], b[c:2 * c], b[2 * c:]

    def state_dict(self):
        sd = super().state_dict()
        for pre, view in (('predictor.0.', self._enc), ('target.0.', self._tgt)):
            sd.update({pre + k: v for k, v in view.state_dict().items()})
        return sd

    def load_state_dict(self, sd, strict=True):
        sd = dict(sd)
        for pre, view in (('predictor.0.', self._enc), ('target.0.', self._tgt)):
            sub = {k[len(pre):]: sd.pop(k) for k in list(sd) if k.startswith(pre)}
            if sub or strict:
                view.load_state_dict(sub, strict)
        super().load_state_dict(sd, strict)


class RNDAgent(_IntrAgent):
    """agents/unsupervised_learning/rnd.py:63-159 (configs/agent/rnd.yaml)."""
    MODULE_METRICS = _module_table('rnd_loss')
    STATE_METRICS = ((L.IM_RMS_MEAN, 'pred_error_mean'), (L.IM_RMS_STD, 'pred_error_std'))
    _PIXELS_OK = True

    def __init__(self, rnd_rep_dim, update_encoder, rnd_scale=1., shard_pretraining=False, **kwargs):
        super().__init__(shard_pretraining, **kwargs)
        self.rnd_scale = rnd_scale
        self.update_encoder = update_encoder
        O, H = self.obs_dim, self.hidden_dim
        pixels = self.obs_type == 'pixels'
        if pixels:      # RND(...) construction order (rnd.py:28-45): the six Linears, then weight_init over predictor (the shared encoder's
            # convolutions are drawn AGAIN, then its Linears) and target (the copied encoder's convolutions get draws of their own)
            lins = [nn.Linear(*d) for d in ((O, H), (H, H), (H, rnd_rep_dim)) * 2]
            conv_shapes = _conv_shapes(self.obs_shape[0])
            w, convs = [], []
            for half in range(2):
                cw = [nn.init.orthogonal_(torch.empty(sh), nn.init.calculate_gain('relu')) for sh in conv_shapes[0::2]]
                convs.append([t for cv in cw for t in (cv, torch.zeros(32))])
                for m in lins[3 * half:3 * half + 3]:
                    nn.init.orthogonal_(m.weight.data)
                    m.bias.data.fill_(0.0)
                    w += [m.weight.data, m.bias.data]
            _load(self.encoder, convs[0])
        else:
            w = _seq_init([('lin', O, H), ('lin', H, H), ('lin', H, rnd_rep_dim)] * 2)      # predictor then target (rnd.py:28-43)
        self._module('rnd', O, H, None, None, rep_dim=rnd_rep_dim, scale=rnd_scale, encoded=pixels)
        if pixels:
            self._own('rnd_target_encoder', NetView(_ENC_KEYS, self.engine.encoder_target_tensors(conv_shapes)))
            _load(self.rnd_target_encoder, convs[1])
            self._own('rnd', _RndPixelView(self.intr, self.engine, self.encoder, self.rnd_target_encoder), self._NET)
        else:
            self._own('rnd', _RndView(self.intr), self._NET)
        _load(self.rnd, w)
        self._own('intrinsic_reward_rms', _RmsView(self.intr))

    def _pix_before_step(self):
        """rnd.py:110-159 on pixels. RND.forward augments the raw frames itself, normalises them with a BatchNorm2d and runs the agent's
        encoder inside its predictor (and a frozen copy inside its target): update_rnd steps that encoder twice on the same gradients
        (rnd_opt, then encoder_opt), compute_intr_reward draws another augmentation and runs the moved encoder, and only then are obs and
        next_obs augmented and encoded for the critic and the actor (detached)."""
        eng = self.engine
        if self.reward_free:
            s = self._batch_slots()
            fp, ft = eng.run_rnd_features(self._shifts())
            self.intr.run_update(fp, None, ft, s.reward, s.reward, 2, dobs_out=self._dobs.data_ptr())
            eng.run_encoder_step(0, self._dobs.data_ptr(), 2)
            fp, ft = eng.run_rnd_features(self._shifts())
            self.intr.run_update(fp, None, ft, s.reward, s.reward, False)
        eng.set_train_encoder(False)
        return dict(shifts_obs=self._shifts(), shifts_next=self._shifts())

    def _module_metrics(self, metrics):
        super()._module_metrics(metrics)
        if self.obs_type == 'pixels':           # the running RMS itself, in fine-tuning too
            M, S_, _n = self.intr.rms_state()
            metrics['pred_error_mean'] = float(M)
            metrics['pred_error_std'] = float(np.sqrt(np.float32(S_)))


class ICMAgent(_IntrAgent):
    """agents/unsupervised_learning/icm.py:48-139 (configs/agent/icm.yaml)."""
    MODULE_METRICS = _module_table('icm_loss')
    _PIXELS_OK = True

    def __init__(self, icm_scale, update_encoder, shard_pretraining=False, **kwargs):
        super().__init__(shard_pretraining, **kwargs)
        self.icm_scale = icm_scale
        self.update_encoder = update_encoder
        O, A, H = self.obs_dim, self.action_dim, self.hidden_dim
        w = _seq_init([('lin', O + A, H), ('lin', H, O), ('lin', 2 * O, H), ('lin', H, A)])
        self._module('icm', O, H, _ICM_KEYS, w, scale=icm_scale)


class _PbeView:
    def __init__(self, engine):
        self.rms = _RmsView(engine)


class ICMAPTAgent(_IntrAgent):
    """agents/unsupervised_learning/icm_apt.py:60-158 (configs/agent/icm_apt.yaml)."""
    MODULE_METRICS = _module_table('icm_loss')
    _PIXELS_OK = True

    def __init__(self, icm_scale, knn_rms, knn_k, knn_avg, knn_clip, update_encoder, icm_rep_dim, shard_pretraining=False, **kwargs):
        super().__init__(shard_pretraining, **kwargs)
        self.icm_scale = icm_scale
        self.update_encoder = update_encoder
        O, A, H, R = self.obs_dim, self.action_dim, self.hidden_dim, icm_rep_dim
        w = _seq_init([('lin', O, R), ('ln', R), ('lin', R + A, H), ('lin', H, R), ('lin', 2 * R, H), ('lin', H, A)])
        self._module('icm_apt', O, H, _APT_KEYS, w, name='icm', rep_dim=R, scale=icm_scale, knn_k=knn_k, knn_avg=knn_avg, knn_rms=knn_rms,
                     knn_clip=knn_clip)
        self._own('pbe', _PbeView(self.intr))


_DIS_KEYS = [f'ensemble.{m}.{i}.{w}' for m in range(5) for i in (0, 2) for w in ('weight', 'bias')]
_DIAYN_KEYS = [f'skill_pred_net.{i}.{w}' for i in (0, 2, 4) for w in ('weight', 'bias')]


class DisagreementAgent(_IntrAgent):
    """agents/unsupervised_learning/disagreement.py:50-136 (configs/agent/disagreement.yaml)."""
    MODULE_METRICS = _module_table('disagreement_loss')
    _PIXELS_OK = True

    def __init__(self, update_encoder, shard_pretraining=False, **kwargs):
        super().__init__(shard_pretraining, **kwargs)
        self.update_encoder = update_encoder
        O, A, H = self.obs_dim, self.action_dim, self.hidden_dim
        # the ensemble keeps nn.Linear's default initialisation: Disagreement never applies utils.weight_init (disagreement.py:12-18)
        w = []
        for _ in range(5):
            for m in (nn.Linear(O + A, H), nn.Linear(H, O)):
                w += [m.weight.data, m.bias.data]
        self._module('disagreement', O, H, _DIS_KEYS, w, n_models=5)


class _Spec:
    """Stand-in for dm_env.specs.Array as the replay storage reads it (name, shape, dtype)."""

    def __init__(self, shape, dtype, name):
        self.shape, self.dtype, self.name = tuple(shape), np.dtype(dtype), name


class _MetaObsMixin:
    """Agents whose batch carries a 6th tensor (DIAYN's skill, APS's task) that is appended to obs / next_obs for the actor and
    critic (diayn.py:162-164, aps.py:236-238) while the module sees the raw observation: the agent's batch slots hold
    [obs | meta] rows, the module gets strided views of them."""
    def _views(self):
        s = self._batch_slots()
        B, W = self.engine.batch, self.obs_dim
        return s, self.engine._view(s.obs, B * W).view(B, W), self.engine._view(s.next_obs, B * W).view(B, W)

    def _load_batch(self, replay_iter):
        if self.obs_type == 'pixels':                # the frames and the meta rows have slots of their own
            return super()._load_batch(replay_iter)
        O, S = self.obs_dim - self._meta_dim, self._meta_dim
        s, obs_v, next_v = self._views()
        if hasattr(replay_iter, 'sample_into'):      # HBM sampler: obs and the meta columns land in the [obs | meta] rows
            out = L.BatchOut(s.obs, s.obs_stride, s.action, s.action_stride, s.reward, s.discount, s.next_obs, s.next_obs_stride,
                             s.obs + 4 * O, O + S)
            replay_iter.sample_into(out, self.engine.batch)
            next_v[:, O:].copy_(obs_v[:, O:])
            return
        obs, action, reward, discount, next_obs, meta = [torch.as_tensor(x).to(self.engine.device, torch.float32) for x in next(replay_iter)[:6]]
        self.engine.set_batch(torch.cat([obs, meta], 1), action, reward, discount, torch.cat([next_obs, meta], 1))

    def _intr_args(self):
        O, W = self.obs_dim - self._meta_dim, self.obs_dim
        s = self._batch_slots()
        return (s.obs, None, s.next_obs, s.reward, s.reward), dict(skill=s.obs + 4 * O, obs_ld=W, next_obs_ld=W, skill_ld=W)


class DIAYNAgent(_MetaObsMixin, _IntrAgent):
    """agents/unsupervised_learning/diayn.py:32-176 (configs/agent/diayn.yaml): the skill rides in the batch as a 6th tensor and
    is appended to obs / next_obs for the actor and critic; the discriminator sees the raw next_obs."""
    MODULE_METRICS = _module_table('diayn_loss', (L.IM_ACC, 'diayn_acc'))
    _PIXELS_OK = True
    _PIX_GRAD = 1

    def __init__(self, update_skill_every_step, skill_dim, diayn_scale, update_encoder, shard_pretraining=False, **kwargs):
        self.skill_dim = self._meta_dim = skill_dim
        self.update_skill_every_step = update_skill_every_step
        self.diayn_scale = diayn_scale
        self.update_encoder = update_encoder
        kwargs['meta_dim'] = self.skill_dim
        self.skill_type = kwargs['skill_type']
        super().__init__(shard_pretraining, **kwargs)
        O, H = self.obs_dim - self.skill_dim, self.hidden_dim
        w = _seq_init([('lin', O, H), ('lin', H, H), ('lin', H, skill_dim)])
        self._module('diayn', O, H, _DIAYN_KEYS, w, rep_dim=skill_dim, scale=diayn_scale)

    def _pix_module(self, fo, fn, s):          # the discriminator reads the next frame's encoding (diayn.py:141-147)
        self.intr.run_update(fo, None, fn, s.reward, s.reward, True, skill=s.meta, skill_ld=self.skill_dim, dobs_out=self._dobs.data_ptr())

    def get_meta_specs(self):
        return (_Spec((self.skill_dim,), np.float32, 'skill'),)

    def init_meta(self):
        if self.skill_type == 'uniform':
            skill = np.random.uniform(0, 1, self.skill_dim).astype(np.float32)
        else:
            skill = np.zeros(self.skill_dim, dtype=np.float32)
            skill[np.random.choice(self.skill_dim)] = 1.0
        meta = OrderedDict()
        meta['skill'] = skill
        return meta

    def update_meta(self, meta, global_step, time_step, finetune=False):
        if global_step % self.update_skill_every_step == 0:
            return self.init_meta()
        return meta


_APS_KEYS = [f'state_feat_net.{i}.{w}' for i in (0, 2, 4) for w in ('weight', 'bias')]


class APSAgent(_MetaObsMixin, _IntrAgent):
    """agents/unsupervised_learning/aps.py:82-320 (configs/agent/aps.yaml): DDPG whose critic emits sf_dim successor features per
    head, Q = task . features (CriticSF, aps.py:12-60); the task vector rides in the batch and in the trailing columns of obs."""
    KIND = 'aps'
    MODULE_METRICS = _module_table('aps_loss', (L.IM_ENT_REWARD, 'intr_ent_reward'), (L.IM_SF_REWARD, 'intr_sf_reward'))
    _PIXELS_OK = True
    _PIX_GRAD = 1                        # update_aps reaches the encoder through next_obs (aps.py:147-159,203-204)

    def _pix_module(self, fo, fn, s):
        self.intr.run_update(fo, None, fn, s.reward, s.reward, True, skill=s.meta, skill_ld=self.sf_dim, dobs_out=self._dobs.data_ptr())

    def __init__(self, update_task_every_step, sf_dim, knn_rms, knn_k, knn_avg, knn_clip, num_init_steps, lstsq_batch_size, update_encoder,
                 shard_pretraining=False, **kwargs):
        self.sf_dim = self._meta_dim = sf_dim
        self.update_task_every_step = update_task_every_step
        self.num_init_steps = num_init_steps
        self.lstsq_batch_size = lstsq_batch_size
        self.update_encoder = update_encoder
        kwargs['meta_dim'] = self.sf_dim
        super().__init__(shard_pretraining, **kwargs)
        O, H = self.obs_dim - self.sf_dim, self.hidden_dim
        w = _seq_init([('lin', O, H), ('lin', H, H), ('lin', H, sf_dim)])
        self._module('aps', O, H, _APS_KEYS, w, rep_dim=sf_dim, knn_k=knn_k, knn_avg=knn_avg, knn_rms=knn_rms, knn_clip=knn_clip)
        self._own('pbe', _PbeView(self.intr))

    def _engine_kw(self):
        return {'sf_dim': self.sf_dim}

    def get_meta_specs(self):
        return (_Spec((self.sf_dim,), np.float32, 'task'),)

    def init_meta(self):
        if self.solved_meta is not None:
            return self.solved_meta
        task = torch.randn(self.sf_dim)
        task = task / torch.norm(task)
        meta = OrderedDict()
        meta['task'] = task.cpu().numpy()
        return meta

    def update_meta(self, meta, global_step, time_step, finetune=False):
        if global_step % self.update_task_every_step == 0:
            return self.init_meta()
        return meta

    @torch.no_grad()
    def regress_meta(self, replay_iter, step):
        """aps.py:247-266: least-squares task from (reward, phi(obs)) pairs at the start of fine-tuning. Host-side, once per run;
        the features come from the module's forward pass (reward-only call on zero tasks), the solve is torch.linalg.lstsq."""
        obs, reward = [], []
        n = 0
        while n < self.lstsq_batch_size:
            batch = next(replay_iter)
            r = torch.as_tensor(batch[2]).to(self.device, torch.float32)
            if self.obs_type == 'pixels':          # aug_and_encode (aps.py:262) through the engine, one batch of frames at a time
                eng = self.engine
                eng.set_batch(*batch[:5])
                eng.augment(self._shifts(), self._shifts())
                o = eng.feature_view(eng.encode(0)).clone()
            else:
                o = torch.as_tensor(batch[0]).to(self.device, torch.float32)
            obs.append(o)
            reward.append(r.reshape(-1, 1))
            n += o.shape[0]
        obs, reward = torch.cat(obs, 0), torch.cat(reward, 0)
        rep = self._features(obs)
        task = torch.linalg.lstsq(reward, rep)[0][:rep.size(1), :][0]
        task = task / torch.norm(task)
        meta = OrderedDict()
        meta['task'] = task.cpu().numpy()
        self.solved_meta = meta
        return meta

    def _features(self, obs):
        """F.normalize(state_feat_net(obs)) for arbitrary row counts: three Linear layers on the module's own parameter views
        (inference outside the update path; torch GEMMs are plumbing here, not the hot path)."""
        p = self.aps.parameters()
        h = torch.relu(obs @ p[0].t() + p[1])
        h = torch.relu(h @ p[2].t() + p[3])
        return torch.nn.functional.normalize(h @ p[4].t() + p[5], dim=-1)


_SMM_KEYS = ([f'z_pred_net.{i}.{w}' for i in (0, 2, 4) for w in ('weight', 'bias')] +
             [f'vae.{n}.{w}' for n in ('enc.0', 'enc.2', 'enc_mu', 'enc_logvar', 'dec.0', 'dec.2', 'dec.4') for w in ('weight', 'bias')])


def _smm_init(O, Z, H, code_dim=128, vae_hidden=150):
    """SMM.__init__ (smm.py:89-104): z_pred_net, then VAE (which applies weight_init to itself), then weight_init over everything —
    the VAE's Linear layers are re-drawn a second time."""
    def orth(ms):
        for m in ms:
            nn.init.orthogonal_(m.weight.data)
            m.bias.data.fill_(0.0)
    W = O + Z
    zp = [nn.Linear(O, H), nn.Linear(H, H), nn.Linear(H, Z)]
    vae = [nn.Linear(W, vae_hidden), nn.Linear(vae_hidden, vae_hidden), nn.Linear(vae_hidden, code_dim), nn.Linear(vae_hidden, code_dim),
           nn.Linear(code_dim, vae_hidden), nn.Linear(vae_hidden, vae_hidden), nn.Linear(vae_hidden, W)]
    orth(vae)
    orth(zp)
    orth(vae)
    return [t for m in zp + vae for t in (m.weight.data, m.bias.data)]


class SMMAgent(_MetaObsMixin, _IntrAgent):
    """agents/unsupervised_learning/smm.py:115-281 (configs/agent/smm.yaml) on state observations.

    Bug-compatible with the reference in one documented place: smm.py adds the 1-D `log_p_star` (B,) to (B,1) terms, so its reward and
    TD target are (B,B) matrices and `mse_loss` averages over all pairs. Per sample that is the TD loss against
    rest_i + mean_j log_p_star_j, plus var_j(log_p_star_j) in each critic's loss value; the module writes exactly that reward and
    `critic_loss` carries the variance term (tests/golden/tiny_smm.npz reproduces the reference's numbers)."""
    MODULE_METRICS = _module_table('loss_vae')
    _PIXELS_OK = True                    # smm.py:264-331 with obs_type == 'pixels': the VAE and the skill predictor read the encoding, p*(s) is dropped
    _PIX_GRAD = 0

    def __init__(self, z_dim, sp_lr, vae_lr, vae_beta, state_ent_coef, latent_ent_coef, latent_cond_ent_coef, update_encoder,
                 shard_pretraining=False, **kwargs):
        self.z_dim = self._meta_dim = z_dim
        self.state_ent_coef = state_ent_coef
        self.latent_ent_coef = latent_ent_coef
        self.latent_cond_ent_coef = latent_cond_ent_coef
        self.update_encoder = update_encoder
        kwargs['meta_dim'] = self.z_dim
        super().__init__(shard_pretraining, **kwargs)
        O, H = self.obs_dim - z_dim, self.hidden_dim
        self.goal = (150, 75)
        w = _smm_init(O, z_dim, H)
        self._module('smm', O, H, _SMM_KEYS, w, rep_dim=z_dim, sp_lr=sp_lr, vae_lr=vae_lr, vae_beta=vae_beta,
                     state_ent_coef=state_ent_coef, latent_ent_coef=latent_ent_coef, latent_cond_ent_coef=latent_cond_ent_coef,
                     goal=self.goal, encoded=self.obs_type == 'pixels')
        self.ft_returns = np.zeros(z_dim, dtype=np.float32)
        self.ft_not_finished = [True for _ in range(z_dim)]
        self.eps_hook = None            # tests: callable(shape) -> the VAE's epsilon (torch.randn in smm.py:62)

    def _eps(self):
        if self.eps_hook is None:
            return None
        return torch.as_tensor(np.asarray(self.eps_hook((self.engine.batch, 128)), np.float32), device=self.engine.device).contiguous()

    def _pix_module(self, fo, fn, s):
        """update_vae on obs_z = [encoding | z] (the encoder steps on the VAE's loss, smm.py:173-185), update_pred on the detached encoding."""
        eng = self.engine
        xz = torch.cat([eng.feature_view(fo), eng.meta_rows()], 1).contiguous()
        e = self._eps()
        self.intr.run_update(xz.data_ptr(), None, None, s.reward, s.reward, True, skill=s.meta, obs_ld=xz.shape[1], skill_ld=self.z_dim,
                       cat_uniform=e.data_ptr() if e is not None else None, dobs_out=self._dobs.data_ptr())
        self._keep_eps = (e, xz)

    def get_meta_specs(self):
        return (_Spec((self.z_dim,), np.float32, 'z'),)

    def init_meta(self):
        z = np.zeros(self.z_dim, dtype=np.float32)
        z[np.random.choice(self.z_dim)] = 1.0
        meta = OrderedDict()
        meta['z'] = z
        return meta

    def update_meta(self, meta, global_step, time_step, finetune=False):
        if self.reward_free:                             # smm.py:154-160 (sic: the fine-tuning rule is keyed on reward_free)
            return self.update_meta_ft(meta, global_step, time_step)
        if time_step.last():
            return self.init_meta()
        return meta

    def update_meta_ft(self, meta, global_step, time_step):
        z_ind = meta['z'].argmax()
        if any(self.ft_not_finished):
            self.ft_returns[z_ind] += time_step.reward
            if time_step.last():
                if not any(self.ft_not_finished):
                    new_z_ind = self.ft_returns.argmax()
                else:
                    self.ft_not_finished[z_ind] = False
                    not_tried_z = sum(self.ft_not_finished)
                    for i in range(self.z_dim):
                        if self.ft_not_finished[i]:
                            if np.random.random() < 1 / not_tried_z:
                                new_z_ind = i
                                break
                            not_tried_z -= 1
                new_z = np.zeros(self.z_dim, dtype=np.float32)
                new_z[new_z_ind] = 1.0
                meta['z'] = new_z
        return meta

    def _intr_args(self):
        O, W = self.obs_dim - self._meta_dim, self.obs_dim
        s = self._batch_slots()
        return (s.obs, None, None, s.reward, s.reward), dict(skill=s.obs + 4 * O, obs_ld=W, skill_ld=W)

    def _intr_hooks(self):
        e = None
        if self.eps_hook is not None:
            e = torch.as_tensor(np.asarray(self.eps_hook((self.intr.batch, 128)), np.float32), device=self.engine.device).contiguous()
        self._keep_eps = e
        return dict(cat_uniform=e.data_ptr()) if e is not None else {}

    def update(self, replay_iter, step):
        if step % self.update_every_steps != 0:
            return dict()
        metrics = super().update(replay_iter, step)
        if self.obs_type == 'pixels':                    # smm.py:260-265: loss_vae / loss_pred ride with use_tb, nothing else is added
            if self.reward_free and (self.use_tb or self.use_wandb):
                metrics['loss_pred'] = float(self._intr_metrics()[5])
            return metrics
        if self.reward_free:                             # smm.py:249-258: these are reported whatever use_tb says
            raw = self._intr_metrics()
            for k in ('icm_loss', 'loss_vae'):
                metrics.pop(k, None)
            metrics.update(intr_reward=float(raw[1]), log_p_star=float(raw[3]), pred_log_ratios=float(raw[4]),
                           latent_ent_coef=float(np.float32(self.latent_ent_coef) * np.float32(np.log(self.z_dim))),
                           latent_cond_ent_coef=float(raw[6]), loss_vae=float(raw[0]), loss_pred=float(raw[5]))
            if 'critic_loss' in metrics:
                metrics['critic_loss'] += 2.0 * float(raw[7])
        return metrics


def _proto_init(O, pred_dim, proj_dim, num_protos):
    """proto.py:55-67: predictor (Linear + weight_init), projector (Projector applies weight_init itself, then the agent applies it
    again), protos (bias-free Linear + weight_init) — the same RNG consumption, tensor by tensor."""
    def orth(m):
        nn.init.orthogonal_(m.weight.data)
        if m.bias is not None:
            m.bias.data.fill_(0.0)
    pred = nn.Linear(O, pred_dim)
    orth(pred)
    p0, p2 = nn.Linear(pred_dim, proj_dim), nn.Linear(proj_dim, pred_dim)
    for _ in range(2):
        orth(p0)
        orth(p2)
    protos = nn.Linear(pred_dim, num_protos, bias=False)
    orth(protos)
    return [pred.weight.data, pred.bias.data, p0.weight.data, p0.bias.data, p2.weight.data, p2.bias.data, protos.weight.data]


class ProtoAgent(_IntrAgent):
    """agents/unsupervised_learning/proto.py:46-207 (configs/agent/proto.yaml) on state observations: the encoder is the identity,
    so encoder_target and the encoder's share of proto_opt vanish; the intrinsic reward is computed on next_obs (proto.py:175-177)."""
    MODULE_METRICS = _module_table('repr_loss')
    _PIXELS_OK = True

    def __init__(self, pred_dim, proj_dim, queue_size, num_protos, tau, encoder_target_tau, topk, update_encoder, shard_pretraining=False,
                 **kwargs):
        # shard_pretraining: under torch.distributed, run the reward-free module step data-parallel (each rank's rows, the target and reward
        # rows all-gathered, Sinkhorn and the candidate draw run identically on every rank). Off by default: on pixels
        # DDPGAgent.__init__ refuses that case without it, so _IntrAgent sets the flag before the base constructor runs; on states the default
        # is the replicated module on the gathered batch. No effect at world size 1.
        super().__init__(shard_pretraining, **kwargs)
        self.tau = tau
        self.encoder_target_tau = encoder_target_tau
        self.topk = topk
        self.num_protos = num_protos
        self.update_encoder = update_encoder
        if self.obs_type == 'pixels':            # encoder_target = deepcopy(encoder) (proto.py:55): no RNG draws
            self.engine.encoder_target(init=True)
        O = self.obs_dim
        w = _proto_init(O, pred_dim, proj_dim, num_protos)
        dp = self._intr_dp() if self.shard_pretraining else dict(batch=self._module_batch)
        self._module('proto', O, proj_dim, None, None, dp=dp, rep_dim=pred_dim, knn_k=topk, num_protos=num_protos, queue_size=queue_size,
                     tau=tau, target_tau=encoder_target_tau)
        for name, keys, indices, ts in (('predictor', ['weight', 'bias'], [0, 1], w[0:2]), ('predictor_target', ['weight', 'bias'], [7, 8], w[0:2]),
                                        ('projector', ['trunk.0.weight', 'trunk.0.bias', 'trunk.2.weight', 'trunk.2.bias'], [2, 3, 4, 5], w[2:6]),
                                        ('protos', ['weight'], [6], w[6:7])):
            _load(self._own(name, _net_view(self.intr, None, keys, indices=indices), self._NET), ts)
        if self.obs_type == 'pixels':
            self._own('encoder_target', NetView(_ENC_KEYS, self.engine.encoder_target_tensors(_conv_shapes(self.obs_shape[0]))), self._NET)
        else:
            self._own('encoder_target', _Identity())
        self._own('queue', self.intr.queue)
        self.cat_hook = None            # tests: callable(num_protos) -> uniforms standing in for Categorical(prob).sample()

    queue_ptr = property(lambda self: self.intr.queue_ptr(), lambda self, v: self.intr.queue_ptr(v))

    def init_from(self, other):         # proto.py:87-96
        if self.obs_type == 'pixels':
            utils.hard_update_params(other.encoder, self.encoder)
        utils.hard_update_params(other.actor, self.actor)
        utils.hard_update_params(other.predictor, self.predictor)
        utils.hard_update_params(other.projector, self.projector)
        utils.hard_update_params(other.protos, self.protos)
        if self.init_critic:
            utils.hard_update_params(other.critic, self.critic)
        if self.obs_type != 'pixels':
            self.params_changed()

    def _cat_u(self):
        if self.cat_hook is None:
            return None
        return torch.as_tensor(np.asarray(self.cat_hook(self.num_protos), np.float32), device=self.engine.device)

    def _intr_args(self):
        s = self._batch_slots()
        return (s.obs, None, s.next_obs, s.reward, s.reward), {}

    def _intr_hooks(self):
        u = self._keep_u = self._cat_u()
        return dict(cat_uniform=u.data_ptr()) if u is not None else {}

    def _pix_before_step(self):
        """proto.py:159-207 on pixels: augment once; the proto step reaches the encoder through proto_opt; reward from the re-encoded
        next_obs; DDPG step with the encoding detached in update_critic; Polyak updates (_pix_after_step)."""
        eng = self.engine
        eng.augment(self._shifts(), self._shifts())         # drawn in fine-tuning too
        if self.reward_free:
            s = self._batch_slots()
            fo = eng.encode(0)
            ft = eng.encode(1, target=True)
            # under torch.distributed (shard_pretraining): the module's phases with their exchanges, and the encoder's share of proto_opt
            # summed across the ranks; with one process these are the one-call forms
            self.intr.run_update(fo, None, ft, None, s.reward, 2, next_obs_target=ft, dobs_out=self._dobs.data_ptr())
            eng.run_encoder_step(0, self._dobs.data_ptr(), 1)
            fn = eng.encode(1)
            u = self._cat_u()
            self.intr.run_update(fo, None, fn, s.reward, s.reward, False, cat_uniform=u.data_ptr() if u is not None else None)
            self._keep_u = u
            # proto.py:190-191 encodes obs and next_obs again for the actor / critic: next_obs with the weights and the input of the reward
            # pass above — the same values, kept — and obs with the stepped encoder, the one pass left to make (4 of the update's 20
            # forward convolutions gone)
            eng.encode(0)
        eng.set_train_encoder(False)
        return dict(keep_augmented=not self.reward_free, keep_encoded=self.reward_free)

    def _pix_after_step(self):
        self.engine.encoder_target(self.encoder_target_tau)

    def _module_metrics(self, metrics):
        if self.reward_free or self.obs_type == 'states':       # on pixels, fine-tuning reports no extr_reward
            super()._module_metrics(metrics)


_ENC_KEYS = [f'convnet.{i}.{w}' for i in (0, 2, 4, 6) for w in ('weight', 'bias')]
_PIX_ACTOR_KEYS = ['trunk.0.weight', 'trunk.0.bias', 'trunk.1.weight', 'trunk.1.bias'] + [f'policy.{i}.{w}' for i in (0, 2, 4) for w in ('weight', 'bias')]
_PIX_CRITIC_KEYS = (['trunk.0.weight', 'trunk.0.bias', 'trunk.1.weight', 'trunk.1.bias'] +
                    [f'{q}.{i}.{w}' for q in ('Q1', 'Q2') for i in (0, 2, 4) for w in ('weight', 'bias')])


def _pixel_init(c_in, hw, A, F, H, meta_dim=0, sf_dim=0):
    """Initial tensors of Encoder, pixel Actor, pixel Critic (and the critic_target's discarded draws) in the reference's RNG order
    (ddpg.py:165-181): every module default-initialised at construction, then weight_init — orthogonal with the ReLU gain for
    Conv2d, gain 1 for Linear, zero biases (utils.py:59-69)."""
    def orth(m, gain=1.0):
        nn.init.orthogonal_(m.weight.data, gain)
        if m.bias is not None:
            m.bias.data.fill_(0.0)
    convs = [nn.Conv2d(c_in, 32, 3, stride=2)] + [nn.Conv2d(32, 32, 3, stride=1) for _ in range(3)]
    for m in convs:
        orth(m, nn.init.calculate_gain('relu'))
    e = (hw - 3) // 2 + 1 - 6
    R = 32 * e * e

    def net(head_in, out, n_heads):
        mods = [nn.Linear(R + meta_dim, F), nn.LayerNorm(F)]
        for _ in range(n_heads):
            mods += [nn.Linear(head_in, H), nn.Linear(H, H), nn.Linear(H, out)]
        for m in mods:
            if isinstance(m, nn.Linear):
                orth(m)
        return [t for m in mods for t in (m.weight.data, m.bias.data)]
    actor = net(F, A, 1)
    critic = net(F + A, 1, 2)
    net(F + A, 1, 2)                      # critic_target's draws, overwritten by load_state_dict
    if sf_dim:                            # APSAgent replaces both with CriticSF after DDPG's constructor ran (aps.py:94-104)
        critic = net(F + A, sf_dim, 2)
        net(F + A, sf_dim, 2)
    return {'encoder': [t for m in convs for t in (m.weight.data, m.bias.data)], 'actor': actor, 'critic': critic, 'repr_dim': R}


class _Identity:
    training = True

    def train(self, mode=True):
        self.training = mode
        return self

    def parameters(self):
        return []

    def __call__(self, x):
        return x


def __getattr__(name):
    """agents.PRDCAgent (Hydra: `_target_: exorl_amd.agents.PRDCAgent`) resolves to exorl_amd.prdc.PRDCAgent on first use: the class is
    defined beside its dataset binding, as exorl_amd.fqe holds FQE's driver, and is not one of this module's own names."""
    if name == 'PRDCAgent':
        from .prdc import PRDCAgent
        return PRDCAgent
    if name == 'ReBRACAgent':          # likewise: exorl_amd.rebrac.ReBRACAgent, defined beside its buffer and batch handling
        from .rebrac import ReBRACAgent
        return ReBRACAgent
    if name in ('OneStepTD3BCAgent', 'OneStepCRRAgent'):      # exorl_amd.onestep: the SARSA-critic agents
        from . import onestep
        return getattr(onestep, name)
    if name == 'CalQLAgent':           # exorl_amd.calql.CalQLAgent, defined beside its buffer and batch handling
        from .calql import CalQLAgent
        return CalQLAgent
    if name == 'BehaviorQAgent':       # exorl_amd.fqe.BehaviorQAgent, beside its driver
        from .fqe import BehaviorQAgent
        return BehaviorQAgent
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')
