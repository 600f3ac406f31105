"""The reward-free agents' update on states as one captured hipGraph (sample -> module step -> intrinsic reward -> DDPG step) against the
eager launches, bit for bit: twin agents built from one torch seed on two identical arenas, one captured and one eager."""
import numpy as np
import pytest
import torch

import _synth
from test_gpu_intr import make, make_proto, make_smm

pytestmark = pytest.mark.gpu

O, A, H, B, R = 24, 6, 128, 64, 16
NSTEP = 3
PROTOS = 16
# Proto writes PROTOS candidate rows per update: after five updates the pointer has moved 80 rows, so 80 (a multiple of PROTOS) is the
# largest queue whose pointer still wraps within them
QUEUE = 5 * PROTOS
KINDS = ['rnd', 'icm', 'icm_apt', 'disagreement', 'diayn', 'aps', 'smm', 'proto']
META = {'diayn': 'skill', 'aps': 'task', 'smm': 'z'}


def build(kind, precision, reward_free=True, H=H, B=B):
    if kind == 'proto':
        ag = make_proto(O, A, H, B, R, H, PROTOS, QUEUE, precision=precision)
    elif kind == 'smm':
        ag = make_smm(O, A, H, B, R, precision=precision)
    else:
        ag = make(kind, O, A, H, B, R, precision=precision)
    ag.reward_free = reward_free
    return ag


def arena(kind, seed=5, B=B):
    """tests/test_gpu_agent.py::_arena with the agent's meta columns (DIAYN's skill, APS's task, SMM's z) and the agents' nstep."""
    from exorl_amd.engine import ReplayEngine
    from exorl_amd.replay_buffer import ArenaIterator
    name = META.get(kind)
    eng = ReplayEngine((O,), np.float32, A, R if name else 0, 4096, 64)
    rs = np.random.RandomState(seed + 100)
    slots = []
    for ep in _synth.synth_episodes(seed, [200, 300, 250], O, A):
        rows = ep['observation'].shape[0]
        if name == 'task':
            v = rs.standard_normal((rows, R)).astype(np.float32)
            ep[name] = v / np.linalg.norm(v, axis=1, keepdims=True)
        elif name:
            ep[name] = np.eye(R, dtype=np.float32)[rs.randint(0, R, rows)]
        slots.append(eng.append_episode(ep, (name,) if name else ()))
    eng.set_order(slots)
    eng.seed_philox(77)
    return eng, ArenaIterator(eng, B, NSTEP, 0.99, 'philox')


def twins(kind, precision, reward_free=True, H=H, B=B, **attrs):
    out = []
    for _ in range(2):
        torch.manual_seed(3)
        ag = build(kind, precision, reward_free, H, B)
        for k, v in attrs.items():
            setattr(ag, k, v)
        out.append((ag, arena(kind, B=B)))
    return out


def state_of(ag):
    """Everything a step moves, as CPU values that compare with torch.equal / ==."""
    from exorl_amd import _lib as L
    eng, it = ag.engine, ag.intr
    torch.cuda.synchronize()
    st = {}
    for net in (L.NET_ACTOR, L.NET_CRITIC, L.NET_CRITIC_TARGET):
        for w in ((L.T_PARAM,) if net == L.NET_CRITIC_TARGET else (L.T_PARAM, L.T_ADAM_M, L.T_ADAM_V)):
            st[f'agent.{net}.{w}'] = eng.flat(net, w).cpu()
    for name, view in (('actor', ag.actor), ('critic', ag.critic), ('critic_target', ag.critic_target)):
        for i, p in enumerate(view.parameters()):
            st[f'{name}.{i}'] = p.cpu()
    for w in (L.T_PARAM, L.T_ADAM_M, L.T_ADAM_V):
        st[f'intr.{w}'] = it.flat(w).cpu()
    st['rms'] = it.rms_state()
    if it.bn is not None:
        st['bn'] = it.bn.cpu()
    if it.queue is not None:
        st['queue'] = it.queue.cpu()
        st['queue_ptr'] = it.queue_ptr()
    st['intr_opt_steps'] = it.opt_steps()
    st['intr_counter'] = it.counter()
    st['opt_steps'] = eng.opt_steps()
    st['reward'] = eng._view(ag._batch_slots().reward, eng.batch).cpu()
    return st


def assert_same(a, b, where=''):
    sa, sb = state_of(a), state_of(b)
    assert sa.keys() == sb.keys()
    for k in sa:
        if torch.is_tensor(sa[k]):
            assert torch.equal(sa[k], sb[k]), (where, k, (sa[k] - sb[k]).abs().max().item())
        else:
            assert sa[k] == sb[k], (where, k, sa[k], sb[k])


def run(pair, steps, where=''):
    (a, (_, ia)), (b, (_, ib)) = pair
    for step in steps:
        ma, mb = a.update(ia, step), b.update(ib, step)
        assert ma == mb, (where, step, ma, mb)
        assert ma, 'use_tb agents report metrics on every update'
    assert_same(a, b, where)


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('kind', KINDS)
def test_captured_step_equals_eager(kind, precision):
    pair = twins(kind, precision)
    (a, (_, ia)), (b, _) = pair
    assert a.enable_graph(ia)
    assert a._graph_iter is ia and b._graph_iter is None
    ptrs = []
    for step in (0, 2, 4, 6, 8):
        run(pair, [step], 'captured')
        if kind == 'proto':
            ptrs.append(a.intr.queue_ptr())
    assert a.engine.graph_captures == 1
    assert a.intr.opt_steps() == 5 and a.engine.opt_steps() == (5, 5)
    if kind == 'proto':
        assert ptrs == [(PROTOS * (i + 1)) % QUEUE for i in range(5)]
        assert any(q < p for p, q in zip(ptrs, ptrs[1:])), ptrs            # the pointer wrapped inside a captured step
        assert a.intr.counter() == 5
    if kind == 'smm':
        assert a.intr.counter() == 5
    assert a.update(ia, 9) == {}                                            # off the update cadence: nothing is launched, no batch drawn
    a.disable_graph()
    assert a._graph_iter is None
    run(pair, [10], 'after disable_graph')


def test_captured_step_takes_the_eager_steps_plane_kernels():
    """bf16x3 with a GEMM of M, N, K >= 256 (RND's H x H layer at hidden 256, batch 256): the eager step converts the operands to bf16
    planes in a library-owned scratch arena; the capture sizes that arena first and takes the same kernels."""
    pair = twins('rnd', 'bf16x3', H=256, B=256)
    (a, (_, ia)), _ = pair
    assert a.enable_graph(ia)                   # before any eager step of this shape: the arena is sized by the capture itself
    run(pair, (0, 2, 4), 'plane kernels')


@pytest.mark.parametrize('kind', ['diayn', 'icm'])
def test_fine_tuning_captures_the_ddpg_step_alone(kind):
    pair = twins(kind, 'fp32', reward_free=False)
    (a, (_, ia)), (b, _) = pair
    before = a.intr.flat().clone()
    assert a.enable_graph(ia)
    run(pair, (0, 2, 4, 6, 8), 'fine-tuning')
    assert torch.equal(a.intr.flat(), before) and a.intr.opt_steps() == 0
    assert a.engine.opt_steps() == (5, 5)


def test_a_moving_schedule_needs_no_recapture():
    pair = twins('rnd', 'fp32', stddev_schedule='linear(1.0,0.1,10)')
    (a, (_, ia)), _ = pair
    assert a.enable_graph(ia)
    run(pair, (0, 2, 4, 6, 8), 'schedule')
    assert a.engine.graph_captures == 1


def test_refusals():
    from exorl_amd.replay_buffer import ArenaIterator
    ag = build('icm', 'fp32')
    eng, it = arena('icm')
    assert ag.enable_graph(iter([])) is False                               # a generic Python iterator
    assert ag.enable_graph(ArenaIterator(eng, B, NSTEP, 0.99, 'mt19937')) is False
    ag.obs_type = 'pixels'
    assert ag.enable_graph(it) is False
    ag.obs_type = 'states'
    ag.noise_hook = _synth.NoiseStream(1).draw
    assert ag.enable_graph(it) is False
    ag.noise_hook = None
    assert ag.enable_graph(it) is True


@pytest.mark.parametrize('kind, hook', [('proto', 'cat_hook'), ('smm', 'eps_hook')])
def test_a_hook_set_after_capture_sends_the_step_down_the_eager_path(kind, hook):
    """Captured, then hooked (eager), then captured again: the counters the eager steps moved reach the graph's device copies."""
    pair = twins(kind, 'fp32')
    (a, (_, ia)), (b, _) = pair
    assert a.enable_graph(ia)
    run(pair, (0, 2), 'captured')
    for ag in (a, b):
        rs = np.random.RandomState(11)
        setattr(ag, hook, (lambda n, rs=rs: rs.uniform(0, 1, n).astype(np.float32)) if hook == 'cat_hook' else
                (lambda shape, rs=rs: rs.standard_normal(shape).astype(np.float32)))
    run(pair, (4, 6), 'hooked')
    assert a.engine.graph_captures == 1 and a._graph_iter is ia
    for ag in (a, b):
        setattr(ag, hook, None)
    run(pair, (8, 10), 'captured again')


@pytest.mark.parametrize('kind', ['rnd', 'smm'])
def test_state_setters_reach_a_bound_graph(kind):
    pair = twins(kind, 'fp32')
    (a, (_, ia)), (b, _) = pair
    assert a.enable_graph(ia)
    run(pair, [0], 'before')
    for ag in (a, b):
        ag.intr.set_opt_steps(100)
        if kind == 'smm':
            ag.intr.counter(40)
    run(pair, (2, 4), 'after the setters')
    assert a.intr.opt_steps() == 102
