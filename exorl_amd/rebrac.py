"""ReBRACAgent: TD3+BC with decoupled penalties (Tarasov et al., NeurIPS 2023), the critic's on the action the dataset took at next_obs,
which the HBM replay emits from its gather launch. Also reachable as exorl_amd.agents.ReBRACAgent.

    agent = ReBRACAgent('rebrac', obs_shape, action_shape, 'cuda', 1e-4, 1024, 0.01, 0.2, 1, 1024, 0.3, use_tb,
                        actor_bc_coef=1.0, critic_bc_coef=1.0)
    replay_iter = iter(loader)              # the HBM sampler fills next_action / next_valid itself
    agent.update(replay_iter, step)
"""
import torch

from . import _lib as L
from .agents import _CRITIC_METRICS, TD3BCAgent, _NextActionBatch


class ReBRACAgent(_NextActionBatch, TD3BCAgent):
    """ReBRAC on TD3+BC's nets (the critics have LayerNorm already) and step. With a~' the clipped target-policy sample TD3+BC draws, a' the
    action the dataset took at s' and v = 1 where the episode holds it (0 where the sample's n steps end the episode: no penalty there),
        y    = r + D (min_i Q'_i(s', a~') - critic_bc_coef v sum_j (a~'_j - a'_j)^2)
        L_pi = actor_bc_coef sum_j (pi(s) - a)_j^2 - Q(s, pi(s)) / mean|Q|,    means over the batch.
    The engine runs the TD3+BC kind with one setting (AgentEngine.set_rebrac): one row kernel folds the penalty into the reward the critic
    step reads, r~ = r - D (critic_bc_coef p), and nothing else of the step changes; critic_bc_coef = 0 is TD3BCAgent bit for bit.
    The actor loss is TD3+BC's mse(pi(s), a) - (alpha / mean|Q|) Q with alpha = 1 / (actor_bc_coef A), A the action dimension, times the
    positive constant actor_bc_coef A (mse is a mean over A columns, ReBRAC's term their sum). That is what the engine minimises and what
    actor_loss reports: ReBRAC's loss divided by actor_bc_coef A. The gradient is scaled by the same constant, which Adam divides out
    again; Adam's epsilon (1e-8 beside sqrt(v)) is the only place the rescaling shows. actor_bc_coef must be > 0 for that reason
    (without a BC term use TD3Agent) and critic_bc_coef >= 0.
    Batches: an HBM iterator (iter(loader), ArenaIterator) writes next_action / next_valid into the agent's buffer in its gather launch; a
    plain iterator yields (obs, action, reward, discount, next_obs, next_action[, next_valid]), next_valid all ones when absent. act(),
    set_obs_normalizer, enable_graph, pickling (the coefficients ride in the attributes, the buffer is allocated and attached again by the
    constructor before the first update) and snapshots are TD3BCAgent's, and the class runs under torch.distributed: the penalty is per
    row and needs no exchange. update() reports TD3+BC's keys, with critic_target_q the penalised y and batch_reward the dataset's r, plus
    critic_penalty (mean of v sum_j (a~' - a')_j^2, before the coefficient) and next_valid (mean of v). No evaluate() and no metric window
    for this class."""
    KIND = 'td3_bc'
    METRIC_WINDOW = False
    _EVALUATES = False
    METRICS = _CRITIC_METRICS + [(L.M_REBRAC_PENALTY, 'critic_penalty'), (L.M_REBRAC_VALID, 'next_valid')]

    def __init__(self, name, obs_shape, action_shape, device, lr, hidden_dim, critic_target_tau, stddev_schedule, nstep,
                 batch_size, stddev_clip, use_tb, actor_bc_coef=1.0, critic_bc_coef=1.0, has_next_action=True, *, precision='fp32', seed=0):
        if not float(actor_bc_coef) > 0.0:
            raise ValueError(f'ReBRACAgent: actor_bc_coef={actor_bc_coef!r} must be > 0 (the actor loss is TD3+BC\'s with alpha = '
                             '1 / (actor_bc_coef * action_dim); without a BC term use TD3Agent)')
        if not float(critic_bc_coef) >= 0.0:
            raise ValueError(f'ReBRACAgent: critic_bc_coef={critic_bc_coef!r} must be >= 0')
        alpha = 1.0 / (float(actor_bc_coef) * action_shape[0])
        super().__init__(name, obs_shape, action_shape, device, lr, hidden_dim, critic_target_tau, stddev_schedule, nstep,
                         batch_size, stddev_clip, use_tb, alpha, has_next_action, precision=precision, seed=seed)
        self.actor_bc_coef, self.critic_bc_coef = float(actor_bc_coef), float(critic_bc_coef)
        eng = self.engine
        buf = torch.zeros(eng.rebrac_bytes(), dtype=torch.uint8, device=eng.device)      # zeros: a plain iterator's first batch may bring no next_valid
        eng.set_rebrac(buf, self.critic_bc_coef)
        self._slots = None          # the slots now carry next_action / next_valid
