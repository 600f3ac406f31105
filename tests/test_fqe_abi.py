"""CPU checks of the FQE kind: header and ctypes constants agree, the version, counts and exorl_agent_cfg are what they were, the step's
plan, which kinds refuse phases 10 / 11 (read from the plan: running a phase needs a handle, tests/test_gpu_fqe.py), the value window's
size, the workspace of existing-kind configurations byte for byte what the build before FQE gave, the pure start-pair batching and the
value dict's arithmetic with its merge over ranks. No GPU is touched."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from test_iql_abi import PARENT_WORKSPACE

ROOT = Path(__file__).resolve().parents[1]
# exorl_agent_workspace_bytes of IQL configurations at the commit before the FQE kind (the first fp32 / bf16x3 / bf16 rows of tests/_iql_cases.py)
PARENT_IQL_WORKSPACE = [(5, 1, 100, 7, 'fp32', 977920), (24, 6, 128, 64, 'bf16x3', 4035072), (24, 6, 256, 1024, 'bf16', 55895296)]


@pytest.fixture(scope='module')
def lib():
    from exorl_amd import _lib as L
    return L.load()


def _cfg(kind, O=24, A=6, H=128, B=64, prec=0, ws=1, n=0):
    from exorl_amd import _lib as L
    return L.AgentCfg(kind, O, A, H, B, prec, ws, 0, 1e-4, 0.01, 2.5, 0.3, 0, n or 10, 0, n or 3, 0, 5.0, 0)


def _plan(lib, cfg):
    from exorl_amd import _lib as L
    ph, x, n = (ctypes.c_int32 * 8)(), (ctypes.c_int32 * 8)(), ctypes.c_int32()
    L.check(lib.exorl_agent_update_plan(ctypes.byref(cfg), ph, x, 8, ctypes.byref(n)))
    return list(ph[:n.value]), list(x[:n.value])


def test_constants_match_the_header(lib):
    from exorl_amd import _lib as L
    header = (ROOT / 'include' / 'exorl_hip.h').read_text()
    d = {k: int(v) for k, v in re.findall(r'#define EXORL_([A-Z0-9_]+)\s+(\d+)', header)}
    assert d['ABI_VERSION'] == 13 == lib.exorl_abi_version() and d['N_METRICS'] == L.N_METRICS == 16 and d['N_EVAL'] == L.N_EVAL == 7
    assert ctypes.sizeof(L.AgentCfg) == 80
    assert d['AGENT_FQE'] == L.AGENT_FQE == 9
    assert 7 not in [v for k, v in d.items() if k.startswith('AGENT_') and not k.startswith('AGENT_XCHG')]
    names = ['FQE_V_Q1', 'FQE_V_Q2', 'FQE_V_MEAN_SQ', 'FQE_V_DIFF_SQ', 'FQE_V_ROWS']
    assert [d[k] for k in names] == [getattr(L, k) for k in names] == list(range(5)) and d['N_FQE_VALUE'] == L.N_FQE_VALUE == 5
    assert sorted(k for k in d if k.startswith('E_')) == sorted(['E_BC_SQ', 'E_Q_DATA', 'E_Q_PI', 'E_Q1_ERR', 'E_Q2_ERR', 'E_TARGET_Q', 'E_ROWS'])
    for fn in ('exorl_agent_fqe_value_bytes', 'exorl_agent_set_fqe_value', 'exorl_agent_fqe_value', 'exorl_agent_fqe_value_read', 'exorl_fqe_rows',
               'exorl_fqe_rows_chunks', 'exorl_replay_episode_returns', 'exorl_replay_num_episodes'):
        assert fn in L.PROTOTYPES and re.search(rf'\b{fn}\(', header), fn


@pytest.mark.parametrize('ws,want', [(1, [-1, -1]), (2, [0, -1])])
def test_plan_is_two_phases_with_the_critic_exchange(lib, ws, want):
    from exorl_amd import _lib as L
    assert L.AGENT_XCHG_CRITIC_GRAD == 0
    assert _plan(lib, _cfg(L.AGENT_FQE, ws=ws)) == ([10, 11], want)
    assert lib.exorl_agent_workspace_bytes(ctypes.byref(_cfg(L.AGENT_FQE))) > 0


def test_no_other_kind_plans_phases_10_and_11(lib):
    from exorl_amd import _lib as L
    from exorl_amd.engine import KIND
    for kind in list(KIND.values()) + [L.AGENT_IQL]:
        for ws in (1, 2):
            cfg = _cfg(kind, ws=ws)
            if kind == L.AGENT_APS:
                cfg.sf_dim = 4
            phases, _ = _plan(lib, cfg)
            assert not {10, 11} & set(phases), (kind, phases)
    assert lib.exorl_agent_workspace_bytes(ctypes.byref(_cfg(7))) == 0 and b'unknown kind 7' in lib.exorl_last_error()
    assert lib.exorl_agent_workspace_bytes(ctypes.byref(_cfg(10))) == 0 and b'unknown kind 10' in lib.exorl_last_error()


def test_fqe_workspace_is_td3s_plus_the_row_partials(lib):
    """The kind carves TD3's layout and, behind it, one 64-float-padded run of per-chunk partials."""
    from exorl_amd import _lib as L
    for O, A, H, B, prec in [(5, 1, 100, 7, 0), (24, 6, 128, 64, 2), (24, 6, 128, 128, 3), (24, 6, 256, 1024, 1), (6, 2, 32, 8200, 0)]:
        td3 = lib.exorl_agent_workspace_bytes(ctypes.byref(_cfg(L.AGENT_TD3, O, A, H, B, prec)))
        fqe = lib.exorl_agent_workspace_bytes(ctypes.byref(_cfg(L.AGENT_FQE, O, A, H, B, prec)))
        chunks = -(-B // 256)
        assert td3 > 0 and fqe == td3 + 4 * (-(-(6 * chunks) // 64) * 64), (O, A, H, B, prec, td3, fqe)


def test_value_window_bytes(lib):
    from exorl_amd import _lib as L
    assert lib.exorl_agent_fqe_value_bytes(ctypes.byref(_cfg(L.AGENT_FQE, B=64))) == 256 + 8 * 32
    assert lib.exorl_agent_fqe_value_bytes(ctypes.byref(_cfg(L.AGENT_FQE, B=8200, H=32))) == 256 + 8 * 160       # 33 chunks x 4, padded to 32
    assert lib.exorl_agent_fqe_value_bytes(ctypes.byref(_cfg(L.AGENT_TD3))) == 0
    assert lib.exorl_agent_set_fqe_value(None, None, 0) != 0 and b'null handle' in lib.exorl_last_error()
    assert lib.exorl_agent_fqe_value(None, 1, None) != 0 and b'null handle' in lib.exorl_last_error()


@pytest.mark.parametrize('row', PARENT_WORKSPACE, ids=lambda r: f'{r[0]}-{r[6]}')
def test_existing_workspaces_keep_their_size(lib, row):
    from exorl_amd.engine import KIND, PRECISION
    kind, O, A, H, B, n, prec, want = row
    assert lib.exorl_agent_workspace_bytes(ctypes.byref(_cfg(KIND[kind], O, A, H, B, PRECISION[prec], 1, n))) == want


@pytest.mark.parametrize('row', PARENT_IQL_WORKSPACE, ids=lambda r: f'iql-{r[4]}')
def test_iql_workspaces_keep_their_size(lib, row):
    from exorl_amd import _lib as L
    from exorl_amd.engine import PRECISION
    O, A, H, B, prec, want = row
    assert lib.exorl_agent_workspace_bytes(ctypes.byref(_cfg(L.AGENT_IQL, O, A, H, B, PRECISION[prec]))) == want


# ---- the pure pieces of FQEAgent.value() ---------------------------------------------------------------------------------------------
B = 64


@pytest.mark.parametrize('n', [1, B - 1, B, B + 1, 2 * B + 22])
def test_start_pair_batches(n):
    from exorl_amd.replay_buffer import start_pair_batches
    got = list(start_pair_batches(n, B))
    assert len(got) == -(-n // B)
    seen = []
    for i, (pairs, valid) in enumerate(got):
        assert pairs.dtype == np.int32 and pairs.shape == (B, 2) and pairs.flags['C_CONTIGUOUS']
        assert valid == (B if i < len(got) - 1 else n - B * (len(got) - 1)) and 1 <= valid <= B
        assert np.all(pairs[:, 1] == 1)                         # idx 1: obs is the episode's row 0
        assert np.all(pairs[valid:, 0] == 0)                    # padding: a pair the sampler accepts
        seen += pairs[:valid, 0].tolist()
    assert seen == list(range(n))                               # every episode once, in table order
    assert list(start_pair_batches(0, B)) == []
    with pytest.raises(ValueError):
        list(start_pair_batches(3, 0))


def test_episode_starts_walks_every_arena_without_a_device():
    """The iterator mixin over stand-in arenas: arena after arena, no batch straddles two, the gather is asked for nstep 1 with GIVEN pairs."""
    from exorl_amd import _lib as L
    from exorl_amd.replay_buffer import _EpisodeStarts

    class Arena:
        def __init__(self, n, g):
            self.n, self.g, self.calls = n, g, []

        def num_episodes(self):
            return self.n

        def sample_into(self, out, batch, nstep, gamma, sampler, pairs):
            self.calls.append((out, batch, nstep, gamma, sampler, pairs.copy()))

        def episode_returns(self, gamma):
            return np.full(self.n, self.g * gamma)

    class It(_EpisodeStarts):
        batch_size, discount = 4, 0.5

        def __init__(self, arenas):
            self.arenas = arenas

        def _arenas(self):
            return self.arenas

    a, b = Arena(5, 1.0), Arena(3, 2.0)
    it = It([a, b])
    got = [(p[:v, 0].tolist(), v) for p, v in it.episode_starts(out='slots')]
    assert got == [([0, 1, 2, 3], 4), ([4], 1), ([0, 1, 2], 3)]
    assert [c[:5] for c in a.calls] == [('slots', 4, 1, 0.5, L.SAMPLER_GIVEN)] * 2 and len(b.calls) == 1
    assert [v for _, v in it.episode_starts(8)] == [5, 3] and len(a.calls) == 2          # no `out`: nothing is gathered
    assert it.episode_returns().tolist() == [0.5] * 5 + [1.0] * 3


def test_value_dict_arithmetic_and_rank_merge():
    from exorl_amd import _lib as L
    from exorl_amd.agents import fqe_values, merge_fqe_sums
    from _fqe_twin import value_dict
    rs = np.random.RandomState(0)
    q1, q2, g = 100.0 + 0.01 * rs.standard_normal(150), 100.0 + 0.01 * rs.standard_normal(150), rs.standard_normal(150)

    def part(sl):
        s = np.zeros(L.N_FQE_VALUE)
        s[L.FQE_V_Q1], s[L.FQE_V_Q2] = q1[sl].sum(), q2[sl].sum()
        s[L.FQE_V_MEAN_SQ], s[L.FQE_V_DIFF_SQ] = ((0.5 * (q1[sl] + q2[sl])) ** 2).sum(), ((q1[sl] - q2[sl]) ** 2).sum()
        s[L.FQE_V_ROWS] = len(q1[sl])
        return s, len(q1[sl]), float(g[sl].sum()), len(g[sl])
    want = value_dict(q1, q2, g)
    whole = fqe_values(*merge_fqe_sums([part(slice(None))]))
    split = fqe_values(*merge_fqe_sums([part(slice(0, 64)), part(slice(64, 150))]))
    assert list(whole) == ['fqe_value', 'fqe_value_q1', 'fqe_value_q2', 'fqe_value_stderr', 'fqe_twin_rms', 'behavior_value', 'episodes']
    for got in (whole, split):
        assert got['episodes'] == 150
        for k in ('fqe_value', 'fqe_value_q1', 'fqe_value_q2', 'fqe_twin_rms', 'behavior_value'):
            assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (k, got[k], want[k])
        # the variance comes from a float64 sum of squares: at mean 100 and spread 0.01 the cancellation costs 8 of 16 digits
        assert abs(got['fqe_value_stderr'] - want['fqe_value_stderr']) <= 1e-6 * want['fqe_value_stderr']
    a, b = merge_fqe_sums([part(slice(0, 64)), part(slice(64, 150))]), merge_fqe_sums([part(slice(0, 64)), part(slice(64, 150))])
    assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:]          # rank order: the same bits on every rank
    one = fqe_values(*merge_fqe_sums([part(slice(0, 1))]))
    assert one['episodes'] == 1 and one['fqe_value_stderr'] == 0.0 and one['fqe_value'] == 0.5 * (q1[0] + q2[0])


def test_set_policy_refusals_need_no_device():
    """_check_policy is what set_policy and for_policy call first: the wrong class is refused before anything is built."""
    from exorl_amd.agents import FQEAgent

    class CQLAgent:
        pass
    with pytest.raises(ValueError, match='CQLAgent.*2A-wide'):
        FQEAgent._check_policy(CQLAgent())
    with pytest.raises(ValueError, match='out of scope'):
        FQEAgent.for_policy(object())
    from types import SimpleNamespace
    from exorl_amd.agents import _AgentBase

    class TD3Agent(_AgentBase):           # the class name and base set_policy accepts, over a stand-in engine
        engine = SimpleNamespace(obs_dim=24, act_dim=6, hidden_dim=128)

    class DDPGAgent(TD3Agent):
        pass
    FQEAgent._check_policy(TD3Agent(), (24, 6, 128))
    for dims in ((25, 6, 128), (24, 5, 128), (24, 6, 256)):
        with pytest.raises(ValueError, match=r'\(24, 6, 128\) of the policy'):
            FQEAgent._check_policy(TD3Agent(), dims)
    with pytest.raises(ValueError, match='out of scope'):
        FQEAgent._check_policy(DDPGAgent(), (24, 6, 128))
