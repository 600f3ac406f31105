"""What a live handle of every agent kind accepts and refuses, against tests/golden/agent_kinds_gpu.json: return code and exorl_last_error()
text of the calls that ask what the kind is, recorded from the library of the commit before the kinds became one table of rows (6ed6eac).

One fp32 handle per kind at (O, A, H, B) = (5, 3, 8, 8), world_size 1. In this order:
  exorl_agent_set_metric_window, _set_eval and _set_fqe_value, each with a buffer of the size the library names (detached again);
  exorl_agent_set_iql(0.7, 3, 100);  exorl_agent_set_prdc with a bound table of a dozen rows;
  exorl_agent_update_phase for phase ids 0 .. 13 (PRDC: with its table bound);  exorl_agent_update with stddev = 0;
  exorl_agent_evaluate with no buffer attached.
Accepted phases run for real on the 8-row batch and return 0. Every refusal is an argument check in front of any launch.

Recording, from a checkout of that commit with its library built (the Python files of the two trees are the same):
    python tests/test_gpu_agent_kinds.py PATH/TO/THAT/CHECKOUT OUT.json
"""
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / 'tests' / 'golden' / 'agent_kinds_gpu.json'
KINDS = ['td3_bc', 'td3', 'bc', 'ddpg', 'crr', 'cql', 'aps', 'iql', 'fqe', 'prdc']
O, A, H, B = 5, 3, 8, 8
BETA = 2.0
# kind -> the phase ids it accepts (its phase table); written out so that the test says which calls have to have run
ACCEPTED = {'cql': range(0, 6), 'iql': range(6, 10), 'fqe': (10, 11), 'prdc': (0, 1, 2, 3, 12)}


def record():
    """kind -> call -> [return code, error text ('' for 0)]"""
    import torch
    import _synth
    from exorl_amd import _lib as L
    from exorl_amd.engine import AgentEngine, ReplayEngine
    lib = L.load()
    # the table: one episode of 12 transitions
    arena = ReplayEngine((O,), np.float32, A, 0, 13 + 64, 4)
    arena.set_order([arena.append_episode(_synth.synth_episodes(3, [12], O, A)[0])])
    assert arena.build_keys(BETA) == 12
    table = {}
    for kind in KINDS:
        torch.manual_seed(11)
        eng = AgentEngine(kind, O, A, H, B, num_value_samples=4, sf_dim=2 if kind == 'aps' else 0)
        for net in [L.NET_ACTOR] + ([L.NET_CRITIC] if eng.has_critic else []) + ([L.NET_VALUE] if eng.has_value else []):
            eng.flat(net).normal_(0.0, 0.3)
        eng.params_changed(sync_target=True)
        eng.set_batch(*_synth.synth_batch(5, 0, B, O, A))
        row = {}

        def call(name, rc):
            row[name] = [rc, '' if rc == 0 else lib.exorl_last_error().decode()]
            return rc
        for name in ('metric_window', 'eval', 'fqe_value'):
            fn = getattr(lib, f'exorl_agent_set_{name}')
            buf = torch.empty(max(getattr(lib, f'exorl_agent_{name}_bytes')(C.byref(eng.cfg)), 256), dtype=torch.uint8, device='cuda')
            if call(f'set_{name}', fn(eng.h, buf.data_ptr(), buf.numel())) == 0:
                torch.cuda.synchronize()
                assert fn(eng.h, None, 0) == 0
        call('set_iql', lib.exorl_agent_set_iql(eng.h, 0.7, 3.0, 100.0))
        call('set_prdc', lib.exorl_agent_set_prdc(eng.h, arena.h, BETA))
        for phase in range(14):
            call(f'update_phase{phase}', lib.exorl_agent_update_phase(eng.h, phase, 0.2, None, None, L.current_stream()))
        call('update_stddev0', lib.exorl_agent_update(eng.h, 0.0, None, None, L.current_stream()))
        call('evaluate_no_buffer', lib.exorl_agent_evaluate(eng.h, L.current_stream()))
        torch.cuda.synchronize()
        table[kind] = row
        del eng
    return table


@pytest.fixture(scope='module')
def tables():
    return json.loads(GOLDEN.read_text()), record()


@pytest.mark.parametrize('kind', KINDS)
def test_return_codes_and_messages_are_the_recorded_ones(tables, kind):
    want, got = tables
    assert list(got[kind]) == list(want[kind])
    for name in want[kind]:
        print(kind, name, got[kind][name])
        assert got[kind][name] == want[kind][name], (kind, name)


@pytest.mark.parametrize('kind', KINDS)
def test_accepted_phases_ran(tables, kind):
    _, got = tables
    for phase in range(14):
        rc, err = got[kind][f'update_phase{phase}']
        if phase in ACCEPTED.get(kind, range(4)):
            assert rc == 0, (kind, phase, err)
        else:
            assert rc == 2 and err.startswith(f'agent_update_phase: phase {phase} out of range for kind '), (kind, phase, err)


if __name__ == '__main__':
    sys.path[:0] = [sys.argv[1], str(ROOT / 'tests')]
    Path(sys.argv[2]).write_text(json.dumps(record(), indent=1) + '\n')
    print(sys.argv[2], Path(sys.argv[2]).stat().st_size, 'bytes')
