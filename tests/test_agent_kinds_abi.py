"""CPU checks that what the library says about an agent kind from the configuration alone is what it was before the kinds became one table of
rows: exorl_agent_workspace_bytes, _metric_window_bytes, _eval_bytes, _fqe_value_bytes and the output of exorl_agent_update_plan over

    every kind id 0 .. 12 (7, 10 and 12 are refused)  x  fp32 / bf16 / bf16x3 / bf16x6  x  world_size 1, 2  x  CQL with and without
    use_critic_lagrange  x  (O, A, H, B) = (5, 3, 8, 8), the smallest the checks accept, and (24, 6, 128, 128), where the plane routes add
    their images

against tests/golden/agent_kinds_abi.json. For a refused configuration the table holds the zero or the return code and the whole
exorl_last_error() text. No GPU is touched.

The table was recorded by record() below from the library of the commit before the rows (6ed6eac), built in a checkout of its own:
    python tests/test_agent_kinds_abi.py PATH/TO/THAT/exorl_amd/libexorl_hip.so
"""
import ctypes as C
import json
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / 'tests' / 'golden' / 'agent_kinds_abi.json'
PRECISIONS = {'fp32': 0, 'bf16': 1, 'bf16x3': 2, 'bf16x6': 3}
SHAPES = [(5, 3, 8, 8), (24, 6, 128, 128)]
CQL = 5


def cases():
    """key -> AgentCfg constructor arguments. Every kind gets the options the kinds that read them accept (sf_dim, CRR's and CQL's counts)."""
    out = {}
    for kind in range(13):
        for lagrange in ((0, 1) if kind == CQL else (0,)):
            for pname, prec in PRECISIONS.items():
                for world in (1, 2):
                    for O, A, H, B in SHAPES:
                        out[f'kind{kind}/lagrange{lagrange}/{pname}/world{world}/O{O}A{A}H{H}B{B}'] = (
                            kind, O, A, H, B, prec, world, 2, 1e-4, 0.01, 2.5, 0.3, 1, 4, 1, 3, lagrange, 5.0, 0)
    return out


def declare(lib):
    lib.exorl_last_error.restype = C.c_char_p
    for name in ('exorl_agent_workspace_bytes', 'exorl_agent_metric_window_bytes', 'exorl_agent_eval_bytes', 'exorl_agent_fqe_value_bytes'):
        getattr(lib, name).restype = C.c_size_t
        getattr(lib, name).argtypes = [C.c_void_p]
    lib.exorl_agent_update_plan.restype = C.c_int
    lib.exorl_agent_update_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    return lib


def record(lib):
    """key -> what the five calls answer. An error text is kept where the call itself has just refused (a zero of exorl_agent_fqe_value_bytes for
    an accepted configuration of another kind sets none)."""
    from exorl_amd._lib import AgentCfg
    err = lambda: (lib.exorl_last_error() or b'').decode()
    table = {}
    for key, args in cases().items():
        cfg = AgentCfg(*args)
        row = {}
        for name in ('workspace', 'metric_window', 'eval', 'fqe_value'):
            n = getattr(lib, f'exorl_agent_{name}_bytes')(C.byref(cfg))
            row[name] = n
            if n == 0 and (name != 'fqe_value' or row['workspace'] == 0):
                row[name + '_error'] = err()
        ph, xc, n = (C.c_int32 * 8)(*[-77] * 8), (C.c_int32 * 8)(*[-77] * 8), C.c_int32(-77)
        row['plan_rc'] = lib.exorl_agent_update_plan(C.byref(cfg), ph, xc, 8, C.byref(n))
        if row['plan_rc'] != 0:
            row['plan_error'] = err()
        row['plan_n'], row['phases'], row['exchanges'] = n.value, list(ph), list(xc)      # whole arrays: nothing behind the plan is touched
        table[key] = row
    return table


@pytest.fixture(scope='module')
def tables():
    from exorl_amd import _lib
    return json.loads(GOLDEN.read_text()), record(declare(_lib.load()))


def test_the_grid_is_the_recorded_one(tables):
    want, got = tables
    assert list(want) == list(cases()) and list(got) == list(cases())
    assert len(want) == (13 + 1) * 4 * 2 * 2


@pytest.mark.parametrize('kind', range(13))
def test_sizes_plans_and_refusals_are_the_recorded_ones(tables, kind):
    want, got = tables
    keys = [k for k in want if k.startswith(f'kind{kind}/')]
    assert len(keys) == (32 if kind == CQL else 16)
    for k in keys:
        assert got[k] == want[k], k


def test_the_refused_ids_are_refused_by_name(tables):
    want, _ = tables
    for k, row in want.items():
        kind = int(k.split('/')[0][4:])
        if kind in (7, 10, 12):
            assert row['workspace'] == 0 and row['plan_rc'] != 0 and row['plan_error'] == f'agent: unknown kind {kind}', k
            assert row['workspace_error'] == row['metric_window_error'] == row['eval_error'] == row['fqe_value_error'] == row['plan_error']
        elif kind == 11 and '/world2/' in k:
            assert row['workspace'] == 0 and 'world_size=2 is not supported for this kind' in row['plan_error'], k
        else:
            assert row['workspace'] > 0 and row['plan_rc'] == 0 and (row['fqe_value'] > 0) == (kind == 9), k


if __name__ == '__main__':
    sys.path.insert(0, str(ROOT))
    GOLDEN.write_text(json.dumps(record(declare(C.CDLL(sys.argv[1]))), indent=0, separators=(',', ':')) + '\n')
    print(GOLDEN, GOLDEN.stat().st_size, 'bytes')
