"""CPU checks of exorl_agent_update_plan: the state agent's step as (phase, exchange that follows it or -1) pairs, for every kind, with and
without CQL's Lagrange weight, at world_size 1 and 2, against the table written out below; and what the call refuses. No GPU is touched."""
import ctypes as C
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CRITIC_GRAD, STATS, ACTOR_GRAD = 0, 1, 2         # EXORL_AGENT_XCHG_*
KINDS = {'td3_bc': 0, 'td3': 1, 'bc': 2, 'ddpg': 3, 'crr': 4, 'cql': 5, 'aps': 6}
# (kind, use_critic_lagrange) -> the phased plan at world_size > 1
PLAN = {
    ('td3_bc', 0): [(0, CRITIC_GRAD), (1, STATS), (2, ACTOR_GRAD), (3, -1)],
    ('td3', 0): [(0, CRITIC_GRAD), (1, -1), (2, ACTOR_GRAD), (3, -1)],
    ('ddpg', 0): [(0, CRITIC_GRAD), (1, -1), (2, ACTOR_GRAD), (3, -1)],
    ('crr', 0): [(0, CRITIC_GRAD), (1, -1), (2, ACTOR_GRAD), (3, -1)],
    ('aps', 0): [(0, CRITIC_GRAD), (1, -1), (2, ACTOR_GRAD), (3, -1)],
    ('bc', 0): [(0, -1), (1, -1), (2, ACTOR_GRAD), (3, -1)],
    ('cql', 0): [(0, CRITIC_GRAD), (1, STATS), (2, ACTOR_GRAD), (3, -1)],
    ('cql', 1): [(4, STATS), (5, CRITIC_GRAD), (1, STATS), (2, ACTOR_GRAD), (3, -1)],
}
ONE_RANK = [(0, -1), (1, -1), (2, -1), (3, -1)]


def _cfg(kind, lagrange=0, world=1, hidden=64):
    from exorl_amd import _lib as L
    return L.AgentCfg(KINDS[kind], 24 + (10 if kind == 'aps' else 0), 6, hidden, 32, 0, world, 10 if kind == 'aps' else 0, 1e-4, 0.01, 2.5, 0.3,
                      1, 4, 1, 3, lagrange, 5.0, 0)


def _plan(cfg, capacity=8, fill=-77):
    """(return code, [(phase, exchange)] written, n, both arrays whole, message)"""
    from exorl_amd import _lib as L
    lib = L.load()
    ph, xc, n = (C.c_int32 * 8)(*[fill] * 8), (C.c_int32 * 8)(*[fill] * 8), C.c_int32(fill)
    rc = lib.exorl_agent_update_plan(C.byref(cfg) if cfg is not None else None, ph, xc, capacity, C.byref(n))
    err = (lib.exorl_last_error() or b'').decode()
    k = n.value if rc == 0 else 0
    return rc, list(zip(ph[:k], xc[:k])), n.value, list(ph) + list(xc), err


@pytest.mark.parametrize('kind, lagrange', sorted(PLAN))
def test_plan_is_the_table(kind, lagrange):
    rc, plan, n, raw, err = _plan(_cfg(kind, lagrange, 2))
    assert rc == 0, err
    assert plan == PLAN[kind, lagrange]
    assert raw[n:8] == [-77] * (8 - n) and raw[8 + n:] == [-77] * (8 - n)        # nothing behind the plan is touched
    rc, plan, _, _, err = _plan(_cfg(kind, lagrange, 1))
    assert rc == 0, err
    assert plan == ONE_RANK


def test_every_kind_is_in_the_table():
    assert {k for k, _ in PLAN} == set(KINDS)
    from exorl_amd.engine import KIND
    assert KIND == KINDS


def test_exact_capacity_is_enough():
    for (kind, lagrange), want in PLAN.items():
        rc, plan, _, _, err = _plan(_cfg(kind, lagrange, 2), capacity=len(want))
        assert rc == 0 and plan == want, err


@pytest.mark.parametrize('kind, lagrange', [('td3_bc', 0), ('cql', 1)])
def test_small_capacity_is_refused_and_nothing_is_written(kind, lagrange):
    rc, _, n, raw, err = _plan(_cfg(kind, lagrange, 2), capacity=len(PLAN[kind, lagrange]) - 1)
    assert rc != 0 and 'capacity' in err, err
    assert n == -77 and raw == [-77] * 16


def test_null_arguments_are_refused():
    from exorl_amd import _lib as L
    lib = L.load()
    rc, _, n, raw, err = _plan(None)
    assert rc != 0 and 'null' in err, err
    assert n == -77 and raw == [-77] * 16
    cfg = _cfg('td3_bc', 0, 2)
    ph, xc, n = (C.c_int32 * 8)(), (C.c_int32 * 8)(), C.c_int32(-77)
    for args in ((None, xc, 8, C.byref(n)), (ph, None, 8, C.byref(n)), (ph, xc, 8, None)):
        assert lib.exorl_agent_update_plan(C.byref(cfg), *args) != 0
        assert 'null' in lib.exorl_last_error().decode()
        assert n.value == -77 and list(ph) == [0] * 8 and list(xc) == [0] * 8


@pytest.mark.parametrize('bad', ['kind', 'world', 'hidden', 'lagrange'])
def test_invalid_cfg_is_refused_and_nothing_is_written(bad):
    cfg = _cfg('td3_bc', 0, 2)
    if bad == 'kind':
        cfg.kind = 7
    elif bad == 'world':
        cfg.world_size = 0
    elif bad == 'hidden':
        cfg.hidden_dim = 6
    else:
        cfg.use_critic_lagrange = 1          # a CQL option
    rc, _, n, raw, err = _plan(cfg)
    assert rc != 0 and err.startswith('agent:'), err
    assert n == -77 and raw == [-77] * 16


def test_constants_and_declaration_match_the_header():
    from exorl_amd import _lib
    h = (ROOT / 'include' / 'exorl_hip.h').read_text()
    ids = {name: int(re.search(rf'#define EXORL_AGENT_XCHG_{name}\s+(\d+)', h).group(1)) for name in ('CRITIC_GRAD', 'STATS', 'ACTOR_GRAD')}
    assert ids == {'CRITIC_GRAD': _lib.AGENT_XCHG_CRITIC_GRAD, 'STATS': _lib.AGENT_XCHG_STATS, 'ACTOR_GRAD': _lib.AGENT_XCHG_ACTOR_GRAD}
    assert ids == {'CRITIC_GRAD': CRITIC_GRAD, 'STATS': STATS, 'ACTOR_GRAD': ACTOR_GRAD}
    assert 'int exorl_agent_update_plan(const exorl_agent_cfg* cfg, int32_t* phases, int32_t* exchanges, int32_t capacity, int32_t* n);' in h
    assert re.search(r'#define EXORL_ABI_VERSION 13\b', h) and 'exorl_agent_update_plan' in h.split('const char* exorl_last_error')[0]
