"""Fitted Q evaluation as one call: how good is a trained policy, from the dataset alone.

    from exorl_amd.fqe import fitted_q_evaluation
    result = fitted_q_evaluation(agent, iter(loader), 100_000)
    print(result['fqe_value'], '+-', result['fqe_value_stderr'], 'against the data at', result['behavior_value'])

The replay must run nstep = 1 (make_offline_replay_loader does): an n-step target follows the behaviour policy's actions for n - 1 steps and
biases the estimate towards the behaviour value. fitted_q_evaluation refuses an iterator with another nstep.
"""
from .agents import FQEAgent


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
