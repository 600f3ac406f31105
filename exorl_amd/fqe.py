"""Fitted Q evaluation as one call: how good is a trained policy, from the dataset alone.

    from exorl_amd.fqe import fitted_q_evaluation
    result = fitted_q_evaluation(agent, iter(loader), 100_000)
    print(result['fqe_value'], '+-', result['fqe_value_stderr'], 'against the data at', result['behavior_value'])

The replay must run nstep = 1 (make_offline_replay_loader does): an n-step target follows the behaviour policy's actions for n - 1 steps and
biases the estimate towards the behaviour value. fitted_q_evaluation refuses an iterator with another nstep.

Behaviour Q evaluation is the same machinery with the dataset's own next action in place of mu(s'): Q^beta, the value of the policy that
collected the data, to read next to the Monte-Carlo behavior_value. Any nstep: the n-step return follows the behaviour policy and so does the
target.

    from exorl_amd.fqe import behavior_q_evaluation
    result = behavior_q_evaluation(iter(loader), 100_000, policy=bc_agent)
    print(result['behavior_q'], '+-', result['behavior_q_stderr'], 'against the returns', result['behavior_value'])
"""
from . import _lib as L
from .agents import FQEAgent, _NextActionBatch


def fitted_q_evaluation(agent, replay_iter, num_grad_steps, *, lr=None, critic_target_tau=None, seed=0, use_graph=True, value_every=None):
    """Builds an FQEAgent around `agent`'s frozen actor (FQEAgent.for_policy: the policy's shapes, batch size, precision and observation
    normaliser; lr / critic_target_tau replace the policy's own, seed seeds the evaluator), trains it for `num_grad_steps` update()s on
    `replay_iter` (captured into one hipGraph per step when use_graph and the iterator allows it, FQEAgent.enable_graph) and returns the
    final FQEAgent.value(replay_iter) dict. With value_every=k it returns (dict, curve) instead, curve a list of (step, value dict) taken
    after every k-th step and after the last; value() between steps does not disturb the training (FQEAgent.value).

    The initial critic is drawn from torch's CPU generator, as every agent's is: call torch.manual_seed before this for a reproducible run."""
    if getattr(replay_iter, 'nstep', 1) != 1:
        raise ValueError(f'fitted_q_evaluation: the replay runs nstep={replay_iter.nstep}; FQE needs nstep=1 (an n-step target follows the '
                         "behaviour policy's actions and biases the estimate)")
    overrides = {'seed': seed}
    if lr is not None:
        overrides['lr'] = lr
    if critic_target_tau is not None:
        overrides['critic_target_tau'] = critic_target_tau
    ev = FQEAgent.for_policy(agent, **overrides)
    if use_graph:
        ev.enable_graph(replay_iter)
    curve = []
    n = int(num_grad_steps)
    for step in range(n):
        ev.update(replay_iter, step)
        if value_every and (step + 1) % int(value_every) == 0 and step + 1 < n:
            curve.append((step + 1, ev.value(replay_iter)))
    result = ev.value(replay_iter)
    if value_every:
        curve.append((n, result))
        return result, curve
    return result


class BehaviorQAgent(_NextActionBatch, FQEAgent):
    """Behaviour Q evaluation: FQEAgent's twin critic, Polyak target and step with the SARSA setting on the engine (AgentEngine.set_sarsa).
    With v = 1 where the episode holds the action a' the dataset took at s' and 0 where the sample's n steps end the episode,
        y_i = r + D Q'_i(s', a')        where v = 1
        y_i = r + D Q'_i(s', mu(s'))    where v = 0: FQE's own target, mu the frozen actor's mean action
    One row kernel copies a' over mu(s') in the target critic's input on the v = 1 rows; nothing else of FQE's step changes, and a batch
    with v = 0 everywhere is FQEAgent's step bit for bit. Unlike FQE the estimate is unbiased at any nstep: the n-step return follows the
    behaviour policy and so does the target, so the replay may run any nstep.
    The actor matters on the v = 0 rows alone: the starts n steps before an episode's end, one start per episode, 1 / (len - nstep + 1) of a
    uniform draw (0.1 % at 1000-step episodes and nstep = 1). set_policy / for_policy give it a policy to fall back on there (a BC clone of
    the data is the consistent choice); without one it is the untrained initial actor.
    Batches: as ReBRACAgent's. An HBM iterator writes next_action / next_valid in its gather launch; a plain iterator yields
    (obs, action, reward, discount, next_obs, next_action[, next_valid]). enable_graph, pickling (the buffer is attached again by the
    constructor), snapshots and torch.distributed are FQEAgent's. update() reports FQE's keys plus next_valid (mean of v).
    value() reads Q(s_0, a_0), the critic at the episode's first observation AND first action, with no actor forward."""
    KIND = 'fqe'
    METRICS = FQEAgent.METRICS + [(L.M_SARSA_VALID, 'next_valid')]
    _VALUE_KEYS = (('fqe_value', 'behavior_q'), ('fqe_value_q1', 'behavior_q_q1'), ('fqe_value_q2', 'behavior_q_q2'),
                   ('fqe_value_stderr', 'behavior_q_stderr'), ('fqe_twin_rms', 'behavior_q_twin_rms'))

    def __init__(self, name, obs_shape, action_shape, device, lr, hidden_dim, critic_target_tau, nstep, batch_size, use_tb, *,
                 precision='fp32', seed=0):
        super().__init__(name, obs_shape, action_shape, device, lr, hidden_dim, critic_target_tau, nstep, batch_size, use_tb,
                         precision=precision, seed=seed)
        self._attach_sarsa()

    def value(self, replay_iter, gather=None):
        """The behaviour policy's value from the critic as it stands: Q(s_0, a_0) over the first observation and the first action of EVERY
        resident episode, enumerated, reduced and exchanged as FQEAgent.value() does it (the same passes and fqe_values' arithmetic; no
        actor forward runs, and update() continues bit for bit). Returns
          behavior_q                       mean over episodes of (Q_1 + Q_2) / 2 at (s_0, a_0)
          behavior_q_q1, behavior_q_q2     the two nets' means separately
          behavior_q_stderr                standard error of behavior_q over episodes
          behavior_q_twin_rms              root-mean-square of Q_1 - Q_2
          behavior_value                   mean discounted return of the episodes themselves: what behavior_q estimates
          episodes                         episodes behind the means"""
        v = super().value(replay_iter, gather)
        for old, new in self._VALUE_KEYS:
            v[new] = v.pop(old)
        return {k: v[k] for k in [new for _, new in self._VALUE_KEYS] + ['behavior_value', 'episodes']}


def behavior_q_evaluation(replay_iter, num_grad_steps, *, policy=None, obs_shape=None, action_shape=None, device='cuda', hidden_dim=1024,
                          batch_size=None, lr=None, critic_target_tau=None, precision='fp32', seed=0, use_graph=True, value_every=None):
    """Trains a BehaviorQAgent for `num_grad_steps` update()s on `replay_iter` (any nstep; captured into one hipGraph per step when
    use_graph and the iterator allows it) and returns the final BehaviorQAgent.value(replay_iter) dict; with value_every=k, (dict, curve) as
    fitted_q_evaluation does.
    `policy` (one of FQEAgent.POLICY_CLASSES, a BC clone of the data say) shapes the evaluator (BehaviorQAgent.for_policy: its sizes, batch
    size, precision and observation normaliser; lr / critic_target_tau replace the policy's own) and supplies the fallback action mu(s') on
    the rows whose episode holds no next action. Without one the evaluator is built from obs_shape, action_shape, device, hidden_dim,
    batch_size (default: the iterator's), lr (1e-4), critic_target_tau (0.01) and precision, and the fallback actor is the untrained
    initial one: it is read on one start per episode, 1 / (len - nstep + 1) of a uniform draw, and never by value().

    The initial critic is drawn from torch's CPU generator, as every agent's is: call torch.manual_seed before this for a reproducible run."""
    nstep = int(getattr(replay_iter, 'nstep', 1))
    if policy is not None:
        overrides = {'name': 'behavior_q', 'nstep': nstep, 'seed': seed}
        if lr is not None:
            overrides['lr'] = lr
        if critic_target_tau is not None:
            overrides['critic_target_tau'] = critic_target_tau
        ev = BehaviorQAgent.for_policy(policy, **overrides)
    else:
        if obs_shape is None or action_shape is None:
            raise ValueError('behavior_q_evaluation: without a policy to shape the evaluator after, pass obs_shape and action_shape')
        batch = int(batch_size or replay_iter.batch_size)
        ev = BehaviorQAgent('behavior_q', tuple(obs_shape), tuple(action_shape), device, 1e-4 if lr is None else lr, hidden_dim,
                            0.01 if critic_target_tau is None else critic_target_tau, nstep, batch, False, precision=precision, seed=seed)
    if use_graph:
        ev.enable_graph(replay_iter)
    curve = []
    n = int(num_grad_steps)
    for step in range(n):
        ev.update(replay_iter, step)
        if value_every and (step + 1) % int(value_every) == 0 and step + 1 < n:
            curve.append((step + 1, ev.value(replay_iter)))
    result = ev.value(replay_iter)
    if value_every:
        curve.append((n, result))
        return result, curve
    return result
