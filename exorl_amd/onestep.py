"""One-step RL (Brandfonbrener et al., NeurIPS 2021): the critic learns Q^beta, the behaviour policy's value, by SARSA on the dataset's own
(s, a, r, s', a'), and the policy takes its improvement step against that critic. The critic never evaluates an out-of-distribution action.
The next action a' comes from the HBM replay's gather launch. Also reachable as exorl_amd.agents.OneStepTD3BCAgent / OneStepCRRAgent.

    agent = OneStepTD3BCAgent('onestep', obs_shape, action_shape, 'cuda', 1e-4, 1024, 0.01, 0.2, 1, 1024, 0.3, use_tb, 2.5)
    replay_iter = iter(loader)              # the HBM sampler fills next_action / next_valid itself
    agent.update(replay_iter, step)

The behaviour-value evaluator on the same setting is exorl_amd.fqe.BehaviorQAgent. TD3, the fourth kind that takes the setting, has no class
here: on a TD3Agent it is reached through the engine alone (agent.engine.sarsa_bytes() / set_sarsa(buf) / set_next_action).
"""
from . import _lib as L
from .agents import CRRAgent, TD3BCAgent, _NextActionBatch

_SARSA_DOC = """The engine runs the parent's kind with one setting (AgentEngine.set_sarsa): with v = 1 where the episode holds the action a' the
    dataset took at s' and 0 where the sample's n steps end the episode,
        y = r + D min_i Q'_i(s', a')      where v = 1
        y = r + D min_i Q'_i(s', a~')     where v = 0: the parent's own target, a~' its clipped target-policy sample
    One row kernel copies a' over a~' in the target critic's input on the v = 1 rows, a launch of its own behind the actor head's (whose
    fused sample epilogue, and with it the parent's step, keeps its bits); nothing else of the step changes, the actor step is the parent's.
    A batch with v = 0 everywhere is the parent's step bit for bit; with v = 1 everywhere the critic's trajectory does not depend on the
    actor. The v = 0 rows are the starts n steps before an episode's end, one start per episode: 1 / (len - nstep + 1) of a uniform draw;
    they are not masked out of the loss.
    Batches: an HBM iterator (iter(loader), ArenaIterator) writes next_action / next_valid into the agent's buffer in its gather launch; a
    plain iterator yields (obs, action, reward, discount, next_obs, next_action[, next_valid]), next_valid all ones when absent. act(),
    set_obs_normalizer, enable_graph, pickling (the buffer is allocated and attached again by the constructor before the first update) and
    snapshots are the parent's, and the class runs under torch.distributed: the rule is per row and needs no exchange. update() reports the
    parent's keys plus next_valid (mean of v). No evaluate() and no metric window for this class."""


class OneStepTD3BCAgent(_NextActionBatch, TD3BCAgent):
    __doc__ = 'One-step RL on TD3+BC: the twin critic is regressed on the SARSA target and the actor takes TD3+BC\'s step against it.\n    ' + _SARSA_DOC
    KIND = 'td3_bc'
    METRIC_WINDOW = False
    _EVALUATES = False
    METRICS = TD3BCAgent.METRICS + [(L.M_SARSA_VALID, 'next_valid')]

    def __init__(self, name, obs_shape, action_shape, device, lr, hidden_dim, critic_target_tau, stddev_schedule, nstep,
                 batch_size, stddev_clip, use_tb, alpha, has_next_action=False, *, precision='fp32', seed=0):
        super().__init__(name, obs_shape, action_shape, device, lr, hidden_dim, critic_target_tau, stddev_schedule, nstep,
                         batch_size, stddev_clip, use_tb, alpha, has_next_action, precision=precision, seed=seed)
        self._attach_sarsa()


class OneStepCRRAgent(_NextActionBatch, CRRAgent):
    __doc__ = ('One-step RL on CRR: the twin critic is regressed on the SARSA target and the actor takes CRR\'s advantage-weighted step against '
               'it.\n    ' + _SARSA_DOC)
    KIND = 'crr'
    METRIC_WINDOW = False
    _EVALUATES = False
    METRICS = CRRAgent.METRICS + [(L.M_SARSA_VALID, 'next_valid')]

    def __init__(self, name, obs_shape, action_shape, device, lr, hidden_dim, critic_target_tau, num_value_samples, weight_func,
                 stddev_schedule, nstep, batch_size, stddev_clip, use_tb, has_next_action=False, *, precision='fp32', seed=0):
        super().__init__(name, obs_shape, action_shape, device, lr, hidden_dim, critic_target_tau, num_value_samples, weight_func,
                         stddev_schedule, nstep, batch_size, stddev_clip, use_tb, has_next_action, precision=precision, seed=seed)
        self._attach_sarsa()
