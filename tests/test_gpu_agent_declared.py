"""The agent classes' declared state: what a pickle holds, which members are device-backed, what a snapshot names and what the public
surface is, for one agent of every class (states; pixels where the class has them), against tests/golden/agent_declared_state.json —
describe() of every case as the commit before the registry (exorl_amd/agents.py _own) computed it. Then the engines' own
export_state / import_state pairs. Smallest shapes the agents accept: fp32, obs 12, act 4, hidden 64, batch 64 (the reward-free shapes of
tests/_dp_worker.py); on pixels 3 x 84 x 84 frames, feature 50, hidden 64, batch 8 (tests/test_gpu_pixels.py's pickle round trip)."""
import inspect
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import _synth

pytestmark = pytest.mark.gpu

O, A, H, B, META = 12, 4, 64, 64, 4
PIX = dict(C_=3, HW=84, A=4, F=50, H=64, B=8)
MODULES = {'RNDAgent': 'rnd', 'ICMAgent': 'icm', 'ICMAPTAgent': 'icm_apt', 'DisagreementAgent': 'disagreement', 'DIAYNAgent': 'diayn',
           'APSAgent': 'aps', 'SMMAgent': 'smm'}
OFFLINE = ('TD3BCAgent', 'TD3Agent', 'CRRAgent', 'IQLAgent', 'FQEAgent', 'CQLAgent', 'CQLAgent/lagrange', 'BCAgent')
CASES = OFFLINE + tuple(f'{c}/{t}' for t in ('states', 'pixels') for c in ('DDPGAgent', *MODULES, 'ProtoAgent'))
TABLE = json.loads((Path(__file__).parent / 'golden' / 'agent_declared_state.json').read_text())


def build(case, use_tb=True):
    """One agent of `case`: a class name, '/lagrange' for CQL's second form, '/states' or '/pixels' for the DDPG family."""
    import test_gpu_intr as TI
    import test_gpu_pixels as TP
    from exorl_amd import agents
    cls, _, variant = case.partition('/')
    a = (cls, (O,), (A,), 'cuda:0', 1e-4, H)
    if cls in ('TD3BCAgent', 'TD3Agent'):
        return getattr(agents, cls)(*a, 0.01, '0.2', 1, B, 0.3, use_tb, *([2.5] if cls == 'TD3BCAgent' else []))
    if cls == 'CRRAgent':
        return agents.CRRAgent(*a, 0.01, 4, 'exp', '0.2', 1, B, 0.3, use_tb)
    if cls == 'IQLAgent':
        return agents.IQLAgent(*a, 0.01, '0.2', 1, B, use_tb)
    if cls == 'FQEAgent':
        return agents.FQEAgent(*a, 0.01, 1, B, use_tb)
    if cls == 'CQLAgent':
        return agents.CQLAgent(*a, 0.01, 1, B, use_tb, 0.01, 3, 5.0, variant == 'lagrange')
    if cls == 'BCAgent':
        return agents.BCAgent(*a, B, '0.2', use_tb)
    if variant == 'pixels':
        if cls == 'DDPGAgent':
            return TP.make_pixel_agent(PIX['C_'], PIX['HW'], PIX['A'], PIX['F'], PIX['H'], PIX['B'], use_tb)
        if cls == 'ProtoAgent':
            kw = dict(name='proto', reward_free=True, obs_type='pixels', obs_shape=(PIX['C_'], PIX['HW'], PIX['HW']), action_shape=(PIX['A'],),
                      device='cuda', lr=1e-4, feature_dim=PIX['F'], hidden_dim=PIX['H'], critic_target_tau=0.01, num_expl_steps=2000,
                      update_every_steps=2, stddev_schedule=0.2, nstep=3, batch_size=PIX['B'], stddev_clip=0.3, init_critic=True, use_tb=use_tb,
                      use_wandb=False)
            return agents.ProtoAgent(pred_dim=16, proj_dim=32, queue_size=32, num_protos=8, tau=0.1, encoder_target_tau=0.05, topk=3,
                                     update_encoder=True, **kw)
        return TP._pixel_intr_agent(MODULES[cls], PIX['C_'], PIX['HW'], PIX['A'], PIX['F'], PIX['H'], PIX['B'], META)[0]
    if cls == 'DDPGAgent':
        return agents.DDPGAgent(**TI.ddpg_kw('ddpg', O, A, H, B, use_tb))
    if cls == 'ProtoAgent':
        return TI.make_proto(O, A, H, B, 16, 32, 16, 256, use_tb)
    if cls == 'SMMAgent':
        return TI.make_smm(O, A, H, B, META, use_tb)
    return TI.make(MODULES[cls], O, A, H, B, META if cls in ('DIAYNAgent', 'APSAgent') else 16, use_tb)


def describe(ag):
    """What the table records per case. Uses only what agents from before the registry have too."""
    from exorl_amd import snapshot
    st = ag.__getstate__()
    return {'top': list(st), 'intr': sorted(st['intr']) if 'intr' in st else None, 'attrs': sorted(st['attrs']),
            'snapshot': list(snapshot.state_dicts(ag)), 'public': [n for n in dir(ag) if not n.startswith('_') and hasattr(ag, n)]}


@pytest.fixture(scope='module')
def zoo():
    torch.manual_seed(11)
    return {case: build(case) for case in CASES}


def test_every_class_has_a_case():
    from exorl_amd import agents
    classes = [c for c in vars(agents).values() if inspect.isclass(c) and issubclass(c, agents._AgentBase) and not c.__name__.startswith('_')]
    assert len(classes) == 16
    for c in classes:
        names = [case for case in CASES if case.partition('/')[0] == c.__name__]
        assert names and all(n in TABLE for n in names), f'{c.__name__}: no case in CASES or no entry in agent_declared_state.json'
        if issubclass(c, agents.DDPGAgent):
            assert {n.partition('/')[2] for n in names} == {'states', 'pixels'}, c.__name__


@pytest.mark.parametrize('case', CASES)
def test_pickle_layout_snapshot_names_and_public_surface(zoo, case):
    """Key sets of __getstate__() at the top level (in order), under intr and of attrs; list(snapshot.state_dicts(agent)); the sorted
    public names for which hasattr is true."""
    assert case in TABLE, f'{case}: missing from agent_declared_state.json'
    got = describe(zoo[case])
    for what, want in TABLE[case].items():
        assert got[what] == want, (case, what, sorted(set(map(str, got[what] or [])) ^ set(map(str, want or []))))


@pytest.mark.parametrize('case', CASES)
def test_device_backed_members_are_registered(zoo, case):
    from exorl_amd import agents, engine
    ag = zoo[case]
    device_backed = (agents.NetView, agents._RmsView, agents._PbeView, agents._Identity, engine._Phased)
    for k, v in vars(ag).items():
        if isinstance(v, device_backed) or (torch.is_tensor(v) and v.is_cuda):
            assert k in ag._members, (case, k)
    attrs = ag.__getstate__()['attrs']
    assert not set(ag._members) & set(attrs), (case, sorted(set(ag._members) & set(attrs)))
    assert all(getattr(ag, name) is not None for name in ag._members)


def test_value_is_a_net_on_iql_and_a_method_on_fqe(zoo):
    from exorl_amd import agents, snapshot
    fqe, iql = zoo['FQEAgent'], zoo['IQLAgent']
    assert 'value' not in fqe._members and 'value' not in snapshot.state_dicts(fqe) and inspect.ismethod(fqe.value)
    assert fqe.value.__func__ is agents.FQEAgent.value
    assert 'value' in iql._members and 'value' in snapshot.state_dicts(iql) and isinstance(iql.value, agents.NetView)
    for ag in (fqe, iql):           # train() walks the record: the nets an optimiser steps, not the Polyak target
        ag.train(False)
        assert [ag.actor.training, ag.critic.training, ag.critic_target.training] == [False, False, True]
        ag.train(True)
    assert iql.value.training is True


# ---- AgentEngine / IntrEngine export_state -> import_state -------------------------------------------------------------------------
def _batch(step):
    return tuple(_synth.synth_batch(41, step, B, O, A))


def _hooks(ag, seed):
    rs = np.random.RandomState(seed)
    normal = lambda shape: rs.standard_normal(tuple(shape)).astype(np.float32)
    ag.noise_hook = lambda shape, dist='normal': np.tanh(normal(shape)) if dist == 'uniform' else normal(shape)
    if hasattr(ag, 'cat_hook'):
        ag.cat_hook = lambda n: rs.uniform(size=n).astype(np.float32)


def round_trip(case):
    """(source, target) agents of `case` after: two updates on the source; export_state -> import_state into the engines of a target
    fresh from its constructor; one more update on both, same batch and same host-supplied draws."""
    torch.manual_seed(3)
    src = build(case)
    torch.manual_seed(4)            # other initial weights: everything equal afterwards came through import_state
    dst = build(case)
    _hooks(src, 50)
    for i in range(2):
        src.update(iter([_batch(i)]), 2 * i)
    dst.engine.import_state(src.engine.export_state())
    if 'intr' in src._members:
        dst.intr.import_state(src.intr.export_state())
    for ag in (src, dst):
        _hooks(ag, 70)
        ag.update(iter([_batch(2)]), 4)
    torch.cuda.synchronize()
    return src, dst


def differing_words(a, b):
    """Indices of the 32-bit words in which two engines' workspaces (the library's aligned part) differ."""
    return torch.nonzero(a._f32.view(torch.int32) != b._f32.view(torch.int32)).reshape(-1).tolist()


@pytest.mark.parametrize('case', ['TD3BCAgent', 'CQLAgent/lagrange', 'IQLAgent', 'RNDAgent/states', 'ProtoAgent/states'])
def test_engine_state_round_trip_continues_bit_identically(case):
    """After the next update the module engine's whole workspace is bit-equal, and the agent engine's apart from one 64-bit word: the
    Philox counter of the update noise lives in that workspace and is no part of the saved state (a pickled agent restarts that stream;
    the draws here come from noise_hook), so on a target fresh from its constructor it, and nothing else, differs (noise_counter() 6
    against 2 after these steps). IQL draws nothing: its workspace is equal whole."""
    src, dst = round_trip(case)
    assert src.engine.opt_steps() == dst.engine.opt_steps() == (3, 3)
    words = differing_words(src.engine, dst.engine)
    if src.engine.noise_counter() == dst.engine.noise_counter():
        assert words == [], (case, words[:8])
    else:
        assert len({w // 2 for w in words}) == 1, (case, words[:8])
    if 'intr' in src._members:
        assert src.intr.opt_steps() == dst.intr.opt_steps() == 3 and src.intr.counter() == dst.intr.counter()
        if src.intr.queue is not None:
            assert src.intr.queue_ptr() == dst.intr.queue_ptr()
        assert differing_words(src.intr, dst.intr) == [], case
