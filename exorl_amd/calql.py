"""CalQLAgent: CQL calibrated from below by the dataset's own returns (Cal-QL, Nakamoto et al., NeurIPS 2023), the Monte-Carlo return-to-go
of every transition being a column the HBM replay builds once and emits from its gather launch. Also reachable as
exorl_amd.agents.CalQLAgent.

    agent = CalQLAgent('calql', obs_shape, action_shape, 'cuda', 1e-4, 1024, 0.01, 1, 1024, use_tb, 0.01, 3, 5.0, False)
    replay_iter = iter(loader)              # the HBM sampler fills mc_return itself
    agent.update(replay_iter, step)
"""
import torch

from . import _lib as L
from .agents import CQLAgent
from .replay_buffer import _ensure_returns


class CalQLAgent(CQLAgent):
    """Cal-QL on CQL's nets and step. In CQL's conservative penalty the critic's value on the policy's actions, Q(s, a) for a ~ pi(s) and
    a ~ pi(s'), is replaced by max(Q(s, a), G(s, a_data)), G the discounted return the dataset's own trajectory achieved from that
    transition: the critic is never pushed below it, which is what keeps offline-to-online fine-tuning from unlearning. The random actions,
    the data action, the TD target, the Lagrange multiplier and the actor step are CQL's. The engine runs the CQL kind with one setting
    (AgentEngine.set_calql): the critic's loss-gradient kernel bounds those entries, no launch is added, and with G = -inf everywhere the
    step is CQLAgent's bit for bit. Both the shipped alpha and use_critic_lagrange=True are supported, and the class runs under
    torch.distributed as CQLAgent does (the bound is per row and needs no exchange).
    G is the return of the episode's recorded remainder: an episode cut by a time limit gets no bootstrap behind its last step, which is a
    lower bound on the true return only where rewards are >= 0, as the DMC tasks' are.
    Batches: an HBM iterator (iter(loader), ArenaIterator) builds its return-to-go column on the first request, and again when a fetch made
    it stale, and writes each row's G into the agent's buffer in its gather launch; a plain iterator yields
    (obs, action, reward, discount, next_obs, mc_return). act(), set_obs_normalizer, pickling (the buffer is allocated and attached again
    by the constructor before the first update) and snapshots are CQLAgent's; enable_graph builds the column before the capture. update()
    reports CQL's keys plus calql_bound_rate, the share of the policy-action entries that the return held up. No evaluate() and no metric
    window for this class."""
    KIND = 'cql'
    METRIC_WINDOW = False
    _EVALUATES = False
    METRICS = CQLAgent.METRICS + [(L.M_CALQL_BOUND, 'calql_bound_rate')]

    def __init__(self, name, obs_shape, action_shape, device, lr, hidden_dim, critic_target_tau, nstep, batch_size, use_tb, alpha,
                 n_samples, target_cql_penalty, use_critic_lagrange, has_next_action=False, *, precision='fp32', seed=0):
        super().__init__(name, obs_shape, action_shape, device, lr, hidden_dim, critic_target_tau, nstep, batch_size, use_tb, alpha,
                         n_samples, target_cql_penalty, use_critic_lagrange, has_next_action, precision=precision, seed=seed)
        eng = self.engine
        eng.set_calql(torch.zeros(eng.calql_bytes(), dtype=torch.uint8, device=eng.device))       # last: unpickling attaches it again

    def _refuse_goal(self, replay_iter):
        goal = getattr(replay_iter, 'goal', None)
        if goal is not None and goal.reward != 'keep':
            raise ValueError(f"{type(self).__name__}: the goal iterator relabels the reward (reward={goal.reward!r}) and the return-to-go column "
                             "that bounds the critic is the arena reward's: use GoalRelabel(reward='keep'), or CQLAgent")

    def _load_batch(self, replay_iter):
        self._refuse_goal(replay_iter)
        eng = self.engine
        if hasattr(replay_iter, 'sample_into'):          # HBM sampler: the gather writes the return-to-go into the buffer
            replay_iter.sample_into(self._batch_slots(), eng.batch, mc_return=eng.mc_return_view())
            return
        batch = next(replay_iter)
        if len(batch) < 6:
            raise ValueError(f'{type(self).__name__}: a batch of {len(batch)} tensors has no mc_return: the iterator must yield (obs, action, '
                             'reward, discount, next_obs, mc_return), mc_return the discounted return-to-go of each row')
        eng.set_batch(*batch[:5])
        eng.set_mc_return(batch[5])

    def enable_graph(self, replay_iter, step=0):
        self._refuse_goal(replay_iter)
        eng = getattr(replay_iter, 'engine', None)
        if eng is not None and getattr(replay_iter, 'sampler', None) == L.SAMPLER_PHILOX:
            _ensure_returns(eng, replay_iter.discount)      # the captured gather reads the column: it stands before the capture
        return super().enable_graph(replay_iter, step)
