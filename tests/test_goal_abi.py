"""What of the goal-conditioned batches needs no device: the header declares the new entry points under ABI version 13 with
exorl_batch_out still 104 bytes, _lib binds them, GoalRelabel validates its arguments and builds act()'s input and the widened normaliser,
and every refusal is raised with its message before the library is touched."""
import ctypes
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
NEW = ('exorl_replay_set_goal', 'exorl_replay_sample_goal', 'exorl_replay_last_goals', 'exorl_agent_enable_graph_goal')


def test_header_declares_the_entry_points_and_nothing_moved():
    from exorl_amd import _lib as L
    header = (ROOT / 'include' / 'exorl_hip.h').read_text()
    d = {k: int(v) for k, v in re.findall(r'#define EXORL_([A-Z0-9_]+)\s+(\d+)', header)}
    assert d['ABI_VERSION'] == 13 == L.load().exorl_abi_version()
    assert (d['GOAL_KEEP'], d['GOAL_NEG'], d['GOAL_SPARSE']) == (L.GOAL_KEEP, L.GOAL_NEG, L.GOAL_SPARSE) == (0, 1, 2)
    assert ctypes.sizeof(L.BatchOut) == 104
    body = re.search(r'typedef struct \{[^}]*?\} exorl_batch_out;', header, re.S).group(0)
    assert len(re.findall(r'\b(?:void|float)\*\s+\w+;', body)) + len(re.findall(r'\bint64_t \w+;', body)) == 13      # 13 eight-byte fields
    for name in NEW:
        assert re.search(r'^int %s\(' % name, header, re.M), name
        assert name in L.PROTOTYPES and hasattr(L.load(), name)
    note = re.search(r'#define EXORL_ABI_VERSION 13.*?\*/', header, re.S).group(0)
    assert all(name in note for name in NEW)                  # listed under "added since, no version change"
    sig = re.search(r'^int exorl_agent_enable_graph\(([^)]*)\);', header, re.M).group(1)
    assert sig == 'exorl_agent_t* a, exorl_replay_t* r, int32_t nstep, float gamma, float stddev, void* stream'
    # the destinations are arguments of the sample call, as mc_return is
    args = re.search(r'^int exorl_replay_sample_goal\((.*?)\);', header, re.M | re.S).group(1)
    for a in ('goals_host', 'goal_dev', 'goal_stride', 'next_goal_dev', 'next_goal_stride', 'mc_return_dev'):
        assert a in args
    assert len(L.PROTOTYPES['exorl_replay_sample_goal'][1]) == len(args.split(','))
    assert len(L.PROTOTYPES['exorl_replay_set_goal'][1]) == 8


def test_goal_relabel_validates_its_arguments():
    from exorl_amd.replay_buffer import GoalRelabel
    g = GoalRelabel([0, 1])
    assert (g.cols, g.p_cur, g.p_traj, g.p_rand, g.horizon_discount, g.reward) == ((0, 1), 0.2, 0.5, 0.3, 0.99, 'neg')
    assert GoalRelabel(range(3), horizon_discount=None, reward='keep').horizon_discount is None
    assert GoalRelabel(2).cols == (2,)
    for bad, msg in ((dict(cols=[]), 'cols is empty'), (dict(cols=[-1]), 'non-negative integer'), (dict(cols=[0.5]), 'non-negative integer'),
                     (dict(cols=[0], p_cur=0.5), 'sum to 1'), (dict(cols=[0], p_cur=-0.2, p_traj=0.9), 'sum to 1'),
                     (dict(cols=[0], horizon_discount=1.0), r'in \(0, 1\)'), (dict(cols=[0], horizon_discount=0.0), r'in \(0, 1\)'),
                     (dict(cols=[0], reward='dense'), "'neg', 'sparse' or 'keep'")):
        with pytest.raises(ValueError, match=msg):
            GoalRelabel(**bad)


def test_goal_obs_and_the_widened_normaliser():
    import torch
    from exorl_amd.replay_buffer import ArenaIterator, DeviceReplayLoader, GoalRelabel
    g = GoalRelabel([3, 0])
    obs, goal = np.arange(4, dtype=np.float32), 10 + np.arange(4, dtype=np.float32)
    assert g.goal_obs(obs, goal).tolist() == [0, 1, 2, 3, 13, 10] and g.goal_obs(obs, goal).dtype == np.float32
    both = g.goal_obs(torch.from_numpy(np.stack([obs, obs])), np.stack([goal, goal + 1]))
    assert both.tolist() == [[0, 1, 2, 3, 13, 10], [0, 1, 2, 3, 14, 11]]
    mean, inv = g.widen_normalizer(np.array([1, 2, 3, 4], np.float32), np.array([5, 6, 7, 8], np.float32))
    assert mean.tolist() == [1, 2, 3, 4, 4, 1] and inv.tolist() == [5, 6, 7, 8, 8, 5] and mean.dtype == np.float32

    class Storage:
        _replay_dir, _meta_specs = Path('.'), ()
    ld = DeviceReplayLoader(Storage(), 100, 8, 1, True, 1, 0.99, sampler='philox', goal=g)
    assert ld.goal is g and ld.goal_obs(obs, goal).tolist() == [0, 1, 2, 3, 13, 10]
    with pytest.raises(ValueError, match='without goal='):
        DeviceReplayLoader(Storage(), 100, 8, 1, True, 1, 0.99).goal_obs(obs, goal)
    it = object.__new__(ArenaIterator)
    assert it.goal is None                                     # an iterator made without goal= says so without an __init__
    it.goal = g
    assert it.goal_obs(obs, goal).tolist() == [0, 1, 2, 3, 13, 10]


def test_loaders_refuse_what_the_goal_path_cannot_honour():
    from exorl_amd.replay_buffer import ArenaIterator, DeviceReplayLoader, GoalRelabel
    g = GoalRelabel([0])

    class Storage:
        _replay_dir, _meta_specs = Path('.'), ()

    class SkillStorage(Storage):
        _meta_specs = (SimpleNamespace(name='skill', shape=(4,)),)
    with pytest.raises(ValueError, match="needs sampler='philox'"):
        DeviceReplayLoader(Storage(), 100, 8, 1, True, 1, 0.99, goal=g)
    with pytest.raises(ValueError, match="needs sampler='philox'"):
        ArenaIterator(None, 8, 1, 0.99, 'mt19937', goal=g)
    with pytest.raises(ValueError, match='float32 state rows, not pixels'):
        DeviceReplayLoader(Storage(), 100, 8, 1, True, 1, 0.99, sampler='philox', frame_stack=3, goal=g)
    with pytest.raises(ValueError, match='meta specs'):
        DeviceReplayLoader(SkillStorage(), 100, 8, 1, True, 1, 0.99, sampler='philox', goal=g)
    with pytest.raises(ValueError, match='expected a GoalRelabel'):
        DeviceReplayLoader(Storage(), 100, 8, 1, True, 1, 0.99, sampler='philox', goal=[0])


def test_pixel_and_meta_arenas_are_refused_before_the_library_is_touched():
    from exorl_amd.engine import ReplayEngine
    from exorl_amd.replay_buffer import GoalRelabel
    g = GoalRelabel([0])
    eng = object.__new__(ReplayEngine)
    eng.obs_dtype, eng.obs_shape, eng.obs_bytes, eng.frame_stack, eng.meta_dim, eng.goal = np.dtype(np.uint8), (9, 84, 84), 9 * 84 * 84, 1, 0, None
    with pytest.raises(ValueError, match='uint8 observations'):
        eng.set_goal(g)
    eng.obs_dtype, eng.obs_shape, eng.obs_bytes = np.dtype(np.float32), (3, 8, 8), 768
    with pytest.raises(ValueError, match='not pixels'):
        eng.set_goal(g)
    eng.obs_shape, eng.obs_bytes, eng.meta_dim = (6,), 24, 4
    with pytest.raises(ValueError, match='4 meta columns'):
        eng.set_goal(g)
    eng.meta_dim = 0
    with pytest.raises(ValueError, match='outside the arena'):
        eng.set_goal(GoalRelabel([6]))
    out = SimpleNamespace(obs_stride=24, next_obs_stride=24)
    with pytest.raises(ValueError, match='needs a goal rule'):
        eng.sample_into(out, 4, 1, 0.99, 1, goal=True)
    eng.goal = GoalRelabel([0, 5])
    with pytest.raises(ValueError, match=r'must both be 32 bytes'):
        eng.sample_into(out, 4, 1, 0.99, 1, goal=True)


def test_a_goal_iterator_checks_the_width_of_the_rows_it_fills():
    from exorl_amd import _lib as L
    from exorl_amd.replay_buffer import ArenaIterator, GoalRelabel
    it = object.__new__(ArenaIterator)
    it.engine, it.goal = SimpleNamespace(obs_bytes=24), GoalRelabel([0, 1])
    it.batch_size, it.nstep, it.discount, it.sampler = 4, 1, 0.99, L.SAMPLER_PHILOX
    out = L.BatchOut(1 << 20, 24, 2 << 20, 3, 3 << 20, 4 << 20, 5 << 20, 24, None, 0)
    with pytest.raises(ValueError, match=r'obs_stride=24 / next_obs_stride=24 bytes \(expected 32\).*obs_shape=\(8,\)'):
        it.sample_into(out, 4)


def test_agents_refuse_goal_iterators_they_cannot_train_on():
    from exorl_amd import agents
    from exorl_amd.calql import CalQLAgent
    from exorl_amd.prdc import PRDCAgent
    from exorl_amd.replay_buffer import GoalRelabel
    neg = SimpleNamespace(goal=GoalRelabel([0]), sample_into=None, engine=None)
    keep = SimpleNamespace(goal=GoalRelabel([0], reward='keep'))
    ag = object.__new__(CalQLAgent)
    with pytest.raises(ValueError, match="CalQLAgent: the goal iterator relabels the reward \\(reward='neg'\\).*reward='keep'"):
        ag._load_batch(neg)
    with pytest.raises(ValueError, match='relabels the reward'):
        ag.enable_graph(neg)
    ag._refuse_goal(keep)                                       # 'keep' leaves the arena's reward: the return-to-go column applies
    with pytest.raises(ValueError, match='PRDCAgent.bind_dataset: a goal iterator'):
        object.__new__(PRDCAgent).bind_dataset(keep)
    for cls in (agents.RNDAgent, agents.DIAYNAgent, agents.APSAgent, agents.ProtoAgent):
        m = object.__new__(cls)
        with pytest.raises(ValueError, match=f'{cls.__name__}: a goal iterator .* reward-free agents'):
            m._step(keep, 0.2)
        with pytest.raises(ValueError, match='reward-free agents'):
            m.enable_graph(keep)
