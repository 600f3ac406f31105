"""FQEAgent's data-parallel step driven by the LIBRARY (exorl_agent_set_comm), modelled on tests/test_gpu_iql_comm.py: a 1-rank RCCL
communicator on the box's one GPU makes the all-reduce an identity, so whole_step_body's plan loop (phases 10 and 11 with the critic gradient
all-reduce on the step's stream, gradients finalised into the flat buffer, unfused Adam) must equal the same phases called one by one, bit for
bit, and the fused one-GPU step to rounding; and the same step captured as one hipGraph must equal eager launches bit for bit. The frozen
actor does not move in any of them."""
import numpy as np
import pytest
import torch

import _fqe_cases as F
import _synth

pytestmark = pytest.mark.gpu
NETS = ('actor', 'critic', 'critic_target')
SHAPE = F.Case(24, 6, 128, 64, 'fp32', 31, 'tight', 'library communicator')


def _flat(ag, nm):
    return torch.cat([p.reshape(-1) for p in getattr(ag, nm).parameters()])


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
def test_native_comm_single_rank_runs_the_fqe_step(precision):
    from exorl_amd.comm import Comm
    c = SHAPE._replace(precision=precision)
    comm = Comm(0, 1, Comm.unique_id())
    native, hand, native_fast, fused = (F.load_params(F.make_agent(c, use_tb=tb), c) for tb in (True, True, False, False))
    start = {nm: _flat(native, nm).clone() for nm in NETS}
    native.engine.set_comm(comm)
    native_fast.engine.set_comm(comm)
    hand.engine.run_update = lambda stddev, nc=None, na=None: [hand.engine.update_phase(ph, stddev) for ph in (10, 11)]
    for step in range(3):
        b = F.batch(c, step)
        ms = [ag.update(iter([b]), step) for ag in (native, hand, native_fast, fused)]
        assert ms[0] == ms[1] and ms[2] == ms[3] == {}
        assert np.array_equal(native.engine.metrics_raw(), hand.engine.metrics_raw())
    for ag in (native, hand, native_fast, fused):
        assert torch.equal(_flat(ag, 'actor'), start['actor'])
    for nm in NETS[1:]:
        assert torch.equal(_flat(native, nm), _flat(hand, nm)), nm
        assert not torch.equal(_flat(native, nm), start[nm]), nm          # the net was stepped
        # the fused optimiser launch sums the gradient partials itself, in another order than finalize_grads: test_gpu_dp.py's rule for that pair
        d = (_flat(native_fast, nm) - _flat(fused, nm)).abs()
        tol = 2e-6 + 1e-5 * _flat(fused, nm).abs()
        assert float((d > tol).float().mean()) <= 5e-3 and float(d.max()) <= 6.5e-4, (nm, float(d.max()))
    for g, h in zip(native.critic.grads(), hand.critic.grads()):
        assert torch.equal(g, h)
    assert native.engine.opt_steps() == hand.engine.opt_steps() == (3, 3)
    for ag in (native, native_fast):
        ag.engine.set_comm(None)


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
def test_fqe_dp_step_with_the_library_communicator_is_capturable(precision):
    from exorl_amd.comm import Comm
    from exorl_amd.engine import ReplayEngine
    from exorl_amd.replay_buffer import ArenaIterator
    c = SHAPE._replace(precision=precision)
    comm = Comm(0, 1, Comm.unique_id())

    def side():
        eng = ReplayEngine((c.O,), np.float32, c.A, 0, 4096, 64)
        eng.set_order([eng.append_episode(ep) for ep in _synth.synth_episodes(9, [200, 300, 250], c.O, c.A)])
        eng.seed_philox(7)
        torch.manual_seed(3)
        ag = F.make_agent(c, use_tb=False)
        ag.engine.set_comm(comm)
        return ag, ArenaIterator(eng, c.B, 1, 0.99, 'philox')
    (g, git), (e, eit) = side(), side()
    assert g.enable_graph(git) and g.engine.graph_captures == 1
    for step in range(4):
        assert g.update(git, step) == {} and e.update(eit, step) == {}
    for nm in NETS:
        assert torch.equal(_flat(g, nm), _flat(e, nm)), nm
    assert g.engine.opt_steps() == e.engine.opt_steps() == (4, 4)
    g.disable_graph()
    g.engine.set_comm(None)
    e.engine.set_comm(None)
