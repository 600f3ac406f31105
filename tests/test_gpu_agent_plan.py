"""AgentEngine.update_steps against the library's plan (exorl_agent_update_plan): in one process, with no process group, an engine built for
world_size = 2 is walked through its phases without exchanging anything; what it yields must be the buffers of the exchanges the plan names,
in the plan's order, and the walk must be one whole optimiser step."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

O, A, H, B = 5, 2, 8, 8
# one case per row of the plan's table (tests/test_agent_plan_abi.py holds the table itself)
ROWS = [('td3_bc', False), ('td3', False), ('ddpg', False), ('crr', False), ('aps', False), ('bc', False), ('cql', False), ('cql', True)]


@pytest.mark.parametrize('kind, lagrange', ROWS)
def test_update_steps_yields_the_plans_exchanges(kind, lagrange):
    from exorl_amd import _lib as L
    from exorl_amd.engine import AgentEngine
    eng = AgentEngine(kind, O, A, H, B, precision='fp32', world_size=2, use_critic_lagrange=lagrange, sf_dim=2 if kind == 'aps' else 0,
                      alpha=0.01 if kind == 'cql' else 2.5, num_value_samples=2)
    gen = torch.Generator().manual_seed(3)
    for net in [L.NET_ACTOR] + ([L.NET_CRITIC] if kind != 'bc' else []):
        flat = eng.flat(net)
        flat.copy_(0.3 * torch.randn(flat.numel(), generator=gen))
    eng.params_changed(sync_target=True)
    eng.set_batch(*[torch.randn(n, generator=gen) for n in (B * O, B * A, B, B, B * O)])

    ph, xc, n = (C.c_int32 * 8)(), (C.c_int32 * 8)(), C.c_int32()
    L.check(eng.lib.exorl_agent_update_plan(C.byref(eng.cfg), ph, xc, 8, C.byref(n)))
    buffers = {L.AGENT_XCHG_CRITIC_GRAD: lambda: eng.flat(L.NET_CRITIC, L.T_GRAD), L.AGENT_XCHG_STATS: eng.stats,
               L.AGENT_XCHG_ACTOR_GRAD: lambda: eng.flat(L.NET_ACTOR, L.T_GRAD)}
    want = [(buffers[x]().data_ptr(), buffers[x]().numel(), L.XCHG_SUM) for x in xc[:n.value] if x >= 0]
    assert len(want) == {'bc': 1, 'td3_bc': 3, 'cql': 4 if lagrange else 3}.get(kind, 2)

    before = eng.opt_steps()
    got = [(buf.data_ptr(), buf.numel(), op) for buf, op in eng.update_steps(0.2)]
    torch.cuda.synchronize()
    assert got == want
    after = eng.opt_steps()
    assert after == (before[0] + 1, before[1] + (kind != 'bc')), (before, after)
