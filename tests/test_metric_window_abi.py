"""CPU checks of the windowed metrics: the three exports, their declarations and bindings, the ABI version, the window buffer's size, and
train_offline(metric_window=True) with a stub agent (enable before the capture, pop at the logging steps, per-step fall-back)."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
SYMBOLS = {'exorl_agent_metric_window_bytes': 1, 'exorl_agent_set_metric_window': 3, 'exorl_agent_metric_window_read': 5}


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


def test_abi_version_is_unchanged(lib):
    lib.exorl_abi_version.restype = ctypes.c_int
    assert lib.exorl_abi_version() == 13
    assert re.search(r'#define EXORL_ABI_VERSION 13\b', (ROOT / 'include' / 'exorl_hip.h').read_text())


def test_window_bytes(lib):
    """256 bytes of sums and step count, then 6 floats per chunk of 4 rows and one per chunk of 8 rows, padded to 64 floats."""
    from exorl_amd import _lib as L
    fn = lib.exorl_agent_metric_window_bytes
    fn.restype, fn.argtypes = L.PROTOTYPES['exorl_agent_metric_window_bytes']
    cfg = lambda kind, B, H=64: L.AgentCfg(kind, 24, 6, H, B, 0, 1, 0, 1e-4, 0.01, 2.5, 0.3, 0, 10, 1, 3, 0, 5.0, 0)
    assert fn(ctypes.byref(cfg(0, 1024))) == 256 + 4 * (6 * 256 + 128)
    assert fn(ctypes.byref(cfg(0, 7))) == 256 + 4 * 64                       # 2 chunks of 4 rows, 1 of 8: 13 floats
    assert fn(ctypes.byref(cfg(2, 8200))) == 256 + 4 * 13376                 # 6 * 2050 + 1025 = 13325
    assert fn(ctypes.byref(cfg(0, 64, H=6))) == 0                            # a configuration exorl_agent_create refuses


class _StubAgent:
    def __init__(self, has_window):
        self.has_window, self.calls, self.window, self.steps_in_window = has_window, [], False, 0

    def enable_metric_window(self):
        self.calls.append('enable_metric_window')
        self.window = self.has_window
        return self.has_window

    def enable_graph(self, replay_iter, step=0):
        self.calls.append('enable_graph')
        return True

    def update(self, replay_iter, step):
        self.steps_in_window += 1
        return {} if self.window else {'critic_loss': float(step)}

    def pop_metrics(self):
        self.calls.append('pop_metrics')
        n, self.steps_in_window = self.steps_in_window, 0
        return {'critic_loss': -1.0, 'metric_steps': n} if n else {}


@pytest.fixture
def offline(monkeypatch):
    import torch
    from exorl_amd import train_offline as T
    monkeypatch.setattr(T, 'make_replay_loader', lambda *a, **k: [None])
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)
    return T.train_offline


def test_train_offline_pops_the_window_at_the_logging_steps(offline):
    ag = _StubAgent(True)
    rows = offline(ag, 'unused', 10, 8, 0.99, log_every_steps=4, metric_window=True)
    assert ag.calls[:2] == ['enable_metric_window', 'enable_graph']           # the capture has to hold the window's kernels
    assert [s for s, _ in rows] == [0, 4, 8]
    assert [r['metric_steps'] for _, r in rows] == [1, 4, 4] and all(r['critic_loss'] == -1.0 and 'fps' in r for _, r in rows)
    assert ag.calls.count('pop_metrics') == 3


def test_train_offline_falls_back_to_per_step_metrics(offline):
    ag = _StubAgent(False)
    rows = offline(ag, 'unused', 10, 8, 0.99, log_every_steps=4, metric_window=True)
    assert ag.calls == ['enable_metric_window', 'enable_graph']
    assert [(s, r['critic_loss']) for s, r in rows] == [(0, 0.0), (4, 4.0), (8, 8.0)] and all('metric_steps' not in r for _, r in rows)


def test_train_offline_default_is_unchanged(offline):
    ag = _StubAgent(True)
    rows = offline(ag, 'unused', 5, 8, 0.99, log_every_steps=4)
    assert ag.calls == ['enable_graph'] and [(s, r['critic_loss']) for s, r in rows] == [(0, 0.0), (4, 4.0)]
