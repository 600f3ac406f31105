"""CPU checks of held-out validation: the four forward-only exports (declared, exported, bound; the ABI version and the agent workspace
stay what they were), the eval buffer's size, the hold-out split rule on file names, the keyword plumbing and refusals of the loader and of
train_offline, the rank merge of the window's sums, and the float32 twin against the float64 twin at half of every bar the GPU test applies
(tests/_eval_twin.py). No GPU is touched."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import _eval_twin as E
import _grad_grid as G
from test_intr_graph_abi import A, AGENT_BYTES, O

ROOT = Path(__file__).resolve().parents[1]
SYMBOLS = {'exorl_agent_eval_bytes': 1, 'exorl_agent_set_eval': 3, 'exorl_agent_evaluate': 2, 'exorl_agent_eval_read': 5}


@pytest.fixture(scope='module')
def lib():
    return ctypes.CDLL(str(ROOT / 'exorl_amd' / 'libexorl_hip.so'))


def test_symbols_declared_exported_and_bound(lib):
    from exorl_amd import _lib as L
    header = (ROOT / 'include' / 'exorl_hip.h').read_text()
    for name, nargs in SYMBOLS.items():
        m = re.search(r'(size_t|int) %s\((.*?)\);' % name, header, re.S)
        assert m, f'{name} is not declared in include/exorl_hip.h'
        assert len([a for a in m.group(2).split(',') if a.strip()]) == nargs
        assert hasattr(lib, name), f'{name} is not exported'
        res, args = L.PROTOTYPES[name]
        assert len(args) == nargs and res is (ctypes.c_size_t if m.group(1) == 'size_t' else ctypes.c_int)
    slots = dict(re.findall(r'#define EXORL_(E_[A-Z0-9_]+|N_EVAL)\s+(\d+)', header))
    assert int(slots['N_EVAL']) == L.N_EVAL == 7 and sorted(int(v) for k, v in slots.items() if k != 'N_EVAL') == list(range(7))
    for k, v in slots.items():
        assert getattr(L, k) == int(v), k
    assert 'between the phases' in header[header.index('int exorl_agent_evaluate') - 1500:header.index('int exorl_agent_evaluate')]


def test_abi_version_is_unchanged(lib):
    lib.exorl_abi_version.restype = ctypes.c_int
    assert lib.exorl_abi_version() == 13
    assert re.search(r'#define EXORL_ABI_VERSION 13\b', (ROOT / 'include' / 'exorl_hip.h').read_text())


def _agent_cfg(key):
    from exorl_amd import _lib as L
    from exorl_amd.engine import KIND
    kind, obs, H, B, prec, sf = key
    return L.AgentCfg(KIND[kind], obs, A, H, B, prec, 1, sf, 1e-4, 0.01, 0.0, 0.3, 0, 10, 0, 3, 0, 5.0, 0)


@pytest.mark.parametrize('key', sorted(AGENT_BYTES))
def test_eval_bytes_is_positive_and_aligned_and_outside_the_workspace(lib, key):
    """256 bytes of sums, then 6 floats per chunk of 256 rows padded to 64 floats; the agent workspace is what it was."""
    from exorl_amd import _lib as L
    fn = lib.exorl_agent_eval_bytes
    fn.restype, fn.argtypes = L.PROTOTYPES['exorl_agent_eval_bytes']
    cfg = _agent_cfg(key)
    n = fn(ctypes.byref(cfg))
    chunks = -(-key[3] // 256)
    assert n > 0 and n % 256 == 0 and n == 256 + 4 * (-(-6 * chunks // 64) * 64)
    assert L.load().exorl_agent_workspace_bytes(ctypes.byref(cfg)) == AGENT_BYTES[key]


def test_eval_bytes_of_a_refused_configuration_is_zero(lib):
    from exorl_amd import _lib as L
    fn = lib.exorl_agent_eval_bytes
    fn.restype, fn.argtypes = L.PROTOTYPES['exorl_agent_eval_bytes']
    assert fn(ctypes.byref(L.AgentCfg(0, 24, 6, 6, 64, 0, 1, 0, 1e-4, 0.01, 2.5, 0.3, 0, 10, 1, 3, 0, 5.0, 0))) == 0
    assert fn(ctypes.byref(L.AgentCfg(0, 24, 6, 64, 8200, 0, 1, 0, 1e-4, 0.01, 2.5, 0.3, 0, 10, 1, 3, 0, 5.0, 0))) == 256 + 4 * 256      # 33 chunks


def test_null_arguments_are_refused_without_a_device(lib):
    from exorl_amd import _lib as L
    lib.exorl_last_error.restype = ctypes.c_char_p
    for name, args in (('exorl_agent_set_eval', (None, None, 0)), ('exorl_agent_evaluate', (None, None)),
                       ('exorl_agent_eval_read', (None, None, None, 0, None))):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = L.PROTOTYPES[name]
        assert fn(*args) != 0
        assert name[len('exorl_'):].encode() in lib.exorl_last_error()


# ---- keyword plumbing and refusals ------------------------------------------------------------------------------------------------
def test_defaults():
    from exorl_amd import agents, replay_buffer as R, train_offline as T
    assert inspect.signature(T.train_offline).parameters['holdout_every'].default is None
    assert inspect.signature(T.train_offline).parameters['val_batches'].default == 0
    assert inspect.signature(R.DeviceReplayLoader.__init__).parameters['holdout_every'].default is None
    sig = inspect.signature(agents._AgentBase.evaluate).parameters
    assert list(sig) == ['self', 'replay_iter', 'num_batches', 'gather'] and sig['num_batches'].default == 1 and sig['gather'].default is None
    for cls in (agents.TD3BCAgent, agents.TD3Agent, agents.CRRAgent, agents.CQLAgent, agents.BCAgent):
        assert cls.evaluate is agents._AgentBase.evaluate and cls.KIND in agents.EVAL_KINDS and cls._EVALUATES
    for cls in (agents.IQLAgent, agents.FQEAgent, agents.DDPGAgent, agents.RNDAgent, agents.APSAgent, agents.ProtoAgent):
        assert not cls._EVALUATES and cls.KIND not in agents.EVAL_KINDS


def test_holdout_every_is_refused_online_and_below_two(tmp_path):
    from exorl_amd import replay_buffer as R
    with pytest.raises(ValueError, match='offline'):
        R.make_replay_loader(R._DirStorage(tmp_path), 1000, 8, 1, False, 1, 0.99, holdout_every=4)
    for k in (1, 0, -3, 2.5, True):
        with pytest.raises(ValueError, match='holdout_every'):
            R.make_offline_replay_loader(None, tmp_path, 1000, 8, 1, 0.99, holdout_every=k)
    ld = R.make_offline_replay_loader(None, tmp_path, 1000, 8, 1, 0.99, holdout_every=2)
    assert ld.holdout_every == 2 and ld.offline
    assert R.make_offline_replay_loader(None, tmp_path, 1000, 8, 1, 0.99).holdout_every is None
    assert iter(R.make_offline_replay_loader(None, tmp_path, 1000, 8, 1, 0.99)).holdout is None


def test_unsupported_agents_raise_and_name_the_supported_classes():
    from exorl_amd import agents

    def stub(cls, **kw):
        ag = cls.__new__(cls)
        ag.__dict__.update(kw)
        return ag
    for ag in (stub(agents.DDPGAgent), stub(agents.TD3BCAgent, obs_type='pixels'), stub(agents.RNDAgent), stub(agents.APSAgent)):
        with pytest.raises(NotImplementedError, match='TD3BCAgent, TD3Agent, CRRAgent, CQLAgent and BCAgent'):
            ag.evaluate(iter([]))


class _StubIter:
    holdout = 'the hold-out iterator'

    def __iter__(self):
        return self

    def __next__(self):
        return None


class _StubAgent:
    def __init__(self):
        self.calls = []

    def update(self, replay_iter, step):
        self.calls.append(('update', step))
        return {'critic_loss': float(step)}

    def evaluate(self, replay_iter, num_batches=1):
        self.calls.append(('evaluate', replay_iter, num_batches))
        return {'val_bc_mse': 0.5, 'val_rows': 8 * num_batches}


@pytest.fixture
def offline(monkeypatch):
    from exorl_amd import train_offline as T
    seen = {}

    class Loader:
        def __iter__(self):
            return _StubIter()

    def make(*a, **k):
        seen.update(k)
        return Loader()
    monkeypatch.setattr(T, 'make_replay_loader', make)
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)
    return T.train_offline, seen


def test_train_offline_forwards_the_keywords_and_emits_the_val_rows(offline):
    train, seen = offline
    ag, logged, order = _StubAgent(), [], []
    rows = train(ag, 'unused', 11, 8, 0.99, log_every_steps=4, eval_every_steps=5, holdout_every=4, val_batches=2,
                 log_fn=lambda s, r: logged.append((s, r)), eval_fn=lambda s, a: order.append(('eval_fn', s, len(logged))))
    assert seen['holdout_every'] == 4
    val = [(s, r) for s, r in rows if 'val_rows' in r]
    assert val == [(s, {'val_bc_mse': 0.5, 'val_rows': 16, 'step': s}) for s in (0, 5, 10)]
    assert [c for c in ag.calls if c[0] == 'evaluate'] == [('evaluate', _StubIter.holdout, 2)] * 3
    assert [(s, r['critic_loss']) for s, r in rows if 'val_rows' not in r] == [(0, 0.0), (4, 4.0), (8, 8.0)]
    assert [s for s, r in logged if 'val_rows' in r] == [0, 5, 10] and logged == rows
    # the val row of a boundary is logged before eval_fn runs there
    assert [(s, n) for _, s, n in order] == [(0, 1), (5, 4), (10, 6)]


@pytest.mark.parametrize('kw', [{}, {'holdout_every': 4}, {'val_batches': 3}])
def test_train_offline_without_both_keywords_evaluates_nothing(offline, kw):
    train, seen = offline
    ag = _StubAgent()
    rows = train(ag, 'unused', 6, 8, 0.99, log_every_steps=4, eval_every_steps=5, **kw)
    assert all(c[0] == 'update' for c in ag.calls) and [(s, r['critic_loss']) for s, r in rows] == [(0, 0.0), (4, 4.0)]
    assert seen.get('holdout_every') == kw.get('holdout_every') and ('holdout_every' in seen) == ('holdout_every' in kw)


# ---- the split rule, on file names alone ----------------------------------------------------------------------------------------------
def _touch(d, n, length=5):
    d.mkdir(parents=True, exist_ok=True)
    for e in range(n):
        (d / f'20240101T0000{e:02d}_{e}_{length}.npz').touch()


@pytest.mark.parametrize('k', [2, 3, 4, 7])
def test_split_positions_per_directory(tmp_path, k):
    from exorl_amd.replay_buffer import _OfflineShard as S
    sizes = [13, 4, 1]
    dirs = [tmp_path / f'd{i}' for i in range(3)]
    for d, n in zip(dirs, sizes):
        _touch(d, n)
    for (files, _), n in zip(S.select_many(dirs, 10**6, 1, 0), sizes):
        assert len(files) == n and files == sorted(files)
        train, held = S.split_holdout(files, k)
        assert held == [files[i] for i in range(k - 1, n, k)]                   # positions k - 1, 2k - 1, ... counted from 0
        assert sorted(train + held) == files and not set(train) & set(held)      # every selected file in exactly one of the two
        assert train == [f for f in files if f not in held]                      # the training side keeps its ascending order
    with pytest.raises(ValueError):
        S.split_holdout([], 1)


def test_split_follows_select_under_a_worker_modulo_and_a_size_limit(tmp_path):
    from exorl_amd.replay_buffer import _OfflineShard as S
    _touch(tmp_path / 'd', 20, length=10)
    files, size = S.select(tmp_path / 'd', 55, 2, 1)            # odd indices, until the running size exceeds 55: 6 files
    assert [int(f.stem.split('_')[1]) for f in files] == [1, 3, 5, 7, 9, 11] and size == 60
    train, held = S.split_holdout(files, 3)
    assert [int(f.stem.split('_')[1]) for f in held] == [5, 11] and [int(f.stem.split('_')[1]) for f in train] == [1, 3, 7, 9]


# ---- the rank merge ---------------------------------------------------------------------------------------------------------------------
def test_rank_merge_of_sums_through_a_fake_gather():
    from exorl_amd import _lib as L, agents
    rs = np.random.RandomState(0)
    parts = [(rs.standard_normal(L.N_EVAL) * 100, r) for r in (64, 64, 8)]
    for s, r in parts:
        s[L.E_ROWS] = r
    sums, rows = agents.merge_eval_sums(parts)
    want = (parts[0][0] + parts[1][0]) + parts[2][0]                             # rank order
    assert rows == 136 and np.array_equal(sums, want)
    v = agents.eval_values(sums, rows, 6)
    assert v['val_rows'] == 136 and v['val_bc_mse'] == want[L.E_BC_SQ] / (136 * 6) and v['val_q_data'] == want[L.E_Q_DATA] / 136
    assert v['val_q_gap'] == v['val_q_pi'] - v['val_q_data'] and v['val_critic_target_q'] == want[L.E_TARGET_Q] / 136
    assert v['val_critic_loss'] == want[L.E_Q1_ERR] / 136 + want[L.E_Q2_ERR] / 136
    assert sorted(agents.eval_values(sums, rows, 6, has_critic=False)) == ['val_bc_mse', 'val_rows']
    # evaluate() itself hands its own part to `gather` and divides what comes back

    class Eng:
        _eval = object()
        batch = 64
        n = 0

        def evaluate(self):
            self.n += 1

        def eval_read(self, reset=True):
            assert reset
            return parts[1]

        def set_batch(self, *b):
            pass
    ag = agents.TD3BCAgent.__new__(agents.TD3BCAgent)
    ag.__dict__.update(engine=Eng(), world_size=2, action_dim=6)
    seen = []

    def gather(own):
        seen.append(own)
        return [parts[0], own, parts[2]]
    got = ag.evaluate(iter([(None,) * 5] * 3), num_batches=3, gather=gather)
    assert ag.engine.n == 3 and seen == [parts[1]] and got == v


# ---- the twin: float32 against float64 at half of every bar the GPU test applies -------------------------------------------------------
def test_the_cases_cover_the_dispatch_grid():
    cs = E.CASES
    assert {G.base_kind(c) for c in cs} == set(E.KINDS)
    assert {c.H for c in cs} >= {4, 100, 128, 192, 320, 1024} and {c.B for c in cs} >= {1, 7, 50, 64, 72, 1000, 8200}
    assert {c.O + c.A for c in cs} >= {32, 33, 36, 90, 256} and {c.A for c in cs} >= {1, 9, 16}
    assert any(G.base_kind(c) == 'cql' and 2 * c.A > 16 for c in cs)
    x3 = [c for c in cs if c.precision == 'bf16x3']
    planes = lambda c: c.H % 128 == 0 and c.B % 64 == 0
    assert any(planes(c) for c in x3) and any(not planes(c) for c in x3) and any(c.precision == 'bf16' for c in cs)
    assert any(c.precision == 'bf16x6' and c.H % 128 == 0 and c.B % 128 == 0 for c in cs)
    assert len({G.case_id(c) for c in cs}) == len(cs)


@pytest.mark.parametrize('c', [pytest.param(c, id=G.case_id(c)) for c in E.CASES])
def test_float32_twin_keeps_half_of_every_bar(c):
    v64, v32 = E.twin_values(c, torch.float64), E.twin_values(c, torch.float32)
    assert sorted(v64) == sorted(v32) and (sorted(v64) == ['val_bc_mse', 'val_rows'] if G.base_kind(c) == 'bc' else len(v64) == 7)
    worst = max(abs(v32[k] - v64[k]) / E.bar(c.precision, v64[k]) for k in E.VALUE_KEYS if k in v64)
    print(f'[eval twin] {G.case_id(c)}: worst |twin32 - twin64| / bar = {worst:.3f}')
    for k in E.VALUE_KEYS:
        if k in v64:
            assert np.isfinite(v64[k]) and abs(v32[k] - v64[k]) <= 0.5 * E.bar(c.precision, v64[k]), (k, v32[k], v64[k])
