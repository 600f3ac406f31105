"""PRDCAgent: TD3+BC with the policy regularised to the nearest dataset point (Ran et al., ICML 2023), the whole dataset searched in HBM on
every step. Also reachable as exorl_amd.agents.PRDCAgent.

    agent = PRDCAgent('prdc', obs_shape, action_shape, 'cuda', 1e-4, 1024, 0.01, 0.2, 1, 1024, 0.3, use_tb, 2.5, beta=2.0)
    replay_iter = iter(loader)
    agent.bind_dataset(replay_iter)         # after the loader's normaliser is set, before enable_graph(); train_offline does it
    agent.update(replay_iter, step)
"""
import numpy as np

from . import _lib as L
from .agents import _CRITIC_METRICS, TD3BCAgent, _world_size


class PRDCAgent(TD3BCAgent):
    """Policy regularisation with dataset constraint (Ran et al., ICML 2023) on TD3+BC's nets and step: the BC target of the actor loss is
    not the sampled row's own action but the action of the dataset point nearest to (beta * s, mu(s)),
        L_pi = -lambda mean(min Q(s, pi(s))) + mse(mu(s), a_nn),   lambda = alpha / mean|Q|,   a_nn a constant of the step,
    found by an exact search over the whole dataset in HBM on every step (AgentEngine.set_prdc, ReplayEngine.build_keys). The critic step,
    the noise, act(), set_obs_normalizer, pickling and snapshots are TD3BCAgent's. bind_dataset() must run before the first update(), and
    again after unpickling: the table is the arena's, not the agent's. update() reports TD3+BC's keys plus nn_dist, the batch mean of the
    distance to the nearest key. One process only; no evaluate() and no metric window for this class."""
    KIND = 'prdc'
    METRIC_WINDOW = False
    METRICS = _CRITIC_METRICS + [(L.M_NN_DIST, 'nn_dist')]

    def __init__(self, name, obs_shape, action_shape, device, lr, hidden_dim, critic_target_tau, stddev_schedule, nstep,
                 batch_size, stddev_clip, use_tb, alpha, has_next_action=False, beta=2.0, *, precision='fp32', seed=0):
        if _world_size() != 1:
            raise ValueError(f'PRDCAgent: the search runs over the whole dataset and a rank holds a shard of it: not built under '
                             f'torch.distributed with {_world_size()} ranks')
        if not float(beta) >= 0.0:
            raise ValueError(f'PRDCAgent: beta={beta!r} must be >= 0')
        super().__init__(name, obs_shape, action_shape, device, lr, hidden_dim, critic_target_tau, stddev_schedule, nstep,
                         batch_size, stddev_clip, use_tb, alpha, has_next_action, precision=precision, seed=seed)
        self.beta = float(beta)

    nn_table_rows = 0           # rows of the bound table (0: none bound); not pickled as a binding: an unpickled agent binds again

    def bind_dataset(self, replay_iter, key_every=1):
        """Builds the key table from `replay_iter`'s arena (after the loader's normaliser is in place, so the keys are what the gather
        emits) and binds it; every key_every-th transition is kept. Call it before enable_graph (with a graph captured the engine
        refuses) and again whenever the arena, its order or its normaliser changed. Returns the number of rows."""
        if getattr(replay_iter, 'goal', None) is not None:
            raise ValueError('PRDCAgent.bind_dataset: a goal iterator (goal=GoalRelabel) fills [obs | g] rows with a goal drawn per sample; '
                             'the key table holds [beta s | a] rows of the arena and has no goal to match: goal-conditioned PRDC is not built')
        arenas = getattr(replay_iter, '_arenas', None)
        if arenas is None:
            raise ValueError('PRDCAgent.bind_dataset: needs an iterator over an HBM arena (iter(loader) or an ArenaIterator); a plain '
                             'iterator of batches has no dataset to search')
        if _world_size() != 1:
            raise ValueError(f'PRDCAgent.bind_dataset: torch.distributed runs {_world_size()} ranks and each holds a shard: the search needs '
                             'the whole dataset in one arena')
        arenas = arenas()
        if len(arenas) != 1:
            raise ValueError(f'PRDCAgent.bind_dataset: the loader keeps its episodes in {len(arenas)} shards (num_workers); the search runs '
                             'over one arena: load with one worker')
        eng = arenas[0]
        if eng.obs_dtype != np.float32 or eng.frame_stack > 1 or len(eng.obs_shape) != 1:
            raise ValueError(f'PRDCAgent.bind_dataset: the arena holds {eng.obs_dtype} observations of shape {eng.obs_shape}; keys are built from '
                             'float32 state rows, not pixels')
        rows = eng.build_keys(self.beta, key_every)
        self.engine.set_prdc(eng, self.beta)
        self.nn_table_rows = rows
        return rows

    def __getstate__(self):
        st = super().__getstate__()
        st['attrs'].pop('nn_table_rows', None)
        return st
