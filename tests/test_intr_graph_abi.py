"""CPU checks of the joint module + agent graph in the C ABI and the agents' Python surface: exorl_agent_enable_graph_intr is exported,
declared in the header and in the ctypes table, the ABI version stays 12, the device step state does not come out of the caller's workspaces
(exorl_intr_workspace_bytes and exorl_agent_workspace_bytes are what they were), and enable_graph of the reward-free classes is no longer the
constant-False stub. No GPU is touched."""
import ctypes
import inspect
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
O, A = 24, 6
# exorl_intr_workspace_bytes(kind, hidden_dim, rep_dim, batch, precision) with 16 prototypes, an 80-row queue, knn_k 3, world_size 1,
# computed with the library of the commit before the joint graph went in
INTR_BYTES = {('aps', 128, 16, 64, 0): 506624, ('aps', 1024, 16, 1024, 2): 38589952, ('diayn', 128, 16, 64, 0): 489472,
              ('diayn', 1024, 16, 1024, 2): 34383360, ('disagreement', 128, 16, 64, 0): 971776, ('disagreement', 1024, 16, 1024, 2): 47704576,
              ('icm', 128, 16, 64, 0): 413696, ('icm', 1024, 16, 1024, 2): 19473920, ('icm_apt', 128, 16, 64, 0): 409856,
              ('icm_apt', 1024, 16, 1024, 2): 23761408, ('proto', 128, 16, 64, 0): 228096, ('proto', 1024, 16, 1024, 2): 10160896,
              ('rnd', 128, 16, 64, 0): 652800, ('rnd', 1024, 16, 1024, 2): 47302656, ('smm', 128, 16, 64, 0): 2905600,
              ('smm', 1024, 16, 1024, 2): 45316608}
# the same at world_size 2, as (kind, hidden_dim, rep_dim, batch, precision, flags, knn_rms): every kind, EXORL_INTR_ENCODED (flags 1) where the
# kind accepts it, and ICM-APT / APS without the RMS; computed with the library of the commit before the module steps became plans
INTR_BYTES_DP = {('aps', 128, 16, 64, 0, 0, 1): 531456, ('aps', 128, 16, 64, 0, 0, 0): 531456, ('aps', 1024, 16, 1024, 2, 0, 1): 42915584,
                 ('aps', 1024, 16, 1024, 2, 0, 0): 42915584, ('diayn', 128, 16, 64, 0, 0, 1): 489472, ('diayn', 1024, 16, 1024, 2, 0, 1): 34383360,
                 ('disagreement', 128, 16, 64, 0, 0, 1): 971776, ('disagreement', 1024, 16, 1024, 2, 0, 1): 47704576,
                 ('icm', 128, 16, 64, 0, 0, 1): 413696, ('icm', 1024, 16, 1024, 2, 0, 1): 19473920, ('icm_apt', 128, 16, 64, 0, 0, 1): 434688,
                 ('icm_apt', 128, 16, 64, 0, 0, 0): 434688, ('icm_apt', 1024, 16, 1024, 2, 0, 1): 28087040,
                 ('icm_apt', 1024, 16, 1024, 2, 0, 0): 28087040, ('proto', 128, 16, 64, 0, 0, 1): 244992, ('proto', 1024, 16, 1024, 2, 0, 1): 10431232,
                 ('rnd', 128, 16, 64, 0, 0, 1): 654336, ('rnd', 128, 16, 64, 0, 1, 1): 646656, ('rnd', 1024, 16, 1024, 2, 0, 1): 47304192,
                 ('rnd', 1024, 16, 1024, 2, 1, 1): 47204352, ('smm', 128, 16, 64, 0, 0, 1): 2905856, ('smm', 128, 16, 64, 0, 1, 1): 2905600,
                 ('smm', 1024, 16, 1024, 2, 0, 1): 45316864, ('smm', 1024, 16, 1024, 2, 1, 1): 45316608}
# exorl_agent_workspace_bytes(kind, obs_dim, hidden_dim, batch, precision, sf_dim), the same way
AGENT_BYTES = {('ddpg', 24, 128, 64, 0, 0): 2001408, ('ddpg', 40, 128, 64, 2, 0): 2935296, ('aps', 40, 128, 64, 0, 16): 2504192,
               ('ddpg', 24, 1024, 1024, 2, 0): 218986496, ('aps', 34, 1024, 1024, 2, 10): 242188800}
NAME = 'exorl_agent_enable_graph_intr'


def test_the_export_is_in_the_library_the_header_and_the_ctypes_table():
    from exorl_amd import _lib, build
    lib = ctypes.CDLL(str(build.build(force=False, verbose=False)))
    assert hasattr(lib, NAME)
    header = (ROOT / 'include' / 'exorl_hip.h').read_text()
    decl = re.search(rf'int {NAME}\(([^;]*)\);', header)
    assert decl, 'not declared in exorl_hip.h'
    assert NAME in _lib.PROTOTYPES
    res, args = _lib.PROTOTYPES[NAME]
    assert res is ctypes.c_int
    assert len(args) == len(decl.group(1).split(','))           # one ctypes entry per declared parameter
    assert args[2] is ctypes.POINTER(_lib.IntrBatch)
    # exorl_agent_enable_graph keeps its signature
    assert re.search(r'int exorl_agent_enable_graph\(exorl_agent_t\* a, exorl_replay_t\* r, int32_t nstep, float gamma, float stddev, void\* stream\);',
                     header)
    assert len(_lib.PROTOTYPES['exorl_agent_enable_graph'][1]) == 6


def test_abi_version_is_unchanged_and_the_header_names_the_export():
    from exorl_amd import _lib
    assert _lib.load().exorl_abi_version() == 13
    header = (ROOT / 'include' / 'exorl_hip.h').read_text()
    version = re.search(r'#define EXORL_ABI_VERSION 13\s+/\*(.*?)\*/', header, re.S)
    assert version and NAME in version.group(1)


@pytest.mark.parametrize('key', sorted(INTR_BYTES) + sorted(INTR_BYTES_DP))
def test_the_module_workspace_is_what_it_was(key):
    from exorl_amd import _lib as L
    from exorl_amd.engine import IntrEngine
    kind, H, R, B, prec, flags, knn_rms, world = key + ((0, 1, 1) if len(key) == 5 else (2,))
    cfg = L.IntrCfg(IntrEngine.KINDS[kind], O, A, H, R, B, prec, 3, 1, knn_rms, 0, flags, 1e-4, 1.0, 0.0, 5.0, 16, 80, 0.1, 0.05, 1e-3, 1e-2, 0.5,
                    1.0, 1.0, 1.0, 150.0, 75.0, world, 0)
    assert L.load().exorl_intr_workspace_bytes(ctypes.byref(cfg)) == {**INTR_BYTES, **INTR_BYTES_DP}[key]


@pytest.mark.parametrize('key', sorted(AGENT_BYTES))
def test_the_agent_workspace_is_what_it_was(key):
    from exorl_amd import _lib as L
    from exorl_amd.engine import KIND
    kind, obs, H, B, prec, sf = key
    cfg = L.AgentCfg(KIND[kind], obs, A, H, B, prec, 1, sf, 1e-4, 0.01, 0.0, 0.3, 0, 10, 0, 3, 0, 5.0, 0)
    assert L.load().exorl_agent_workspace_bytes(ctypes.byref(cfg)) == AGENT_BYTES[key]


def test_enable_graph_of_the_reward_free_classes_is_no_stub():
    from exorl_amd import agents
    fn = agents._IntrAgent.enable_graph
    src = inspect.getsource(fn)
    assert 'enable_graph_intr' in src and 'return True' in src
    assert fn is not agents._AgentBase.enable_graph
    for cls in (agents.RNDAgent, agents.ICMAgent, agents.ICMAPTAgent, agents.DisagreementAgent, agents.DIAYNAgent, agents.APSAgent,
                agents.SMMAgent, agents.ProtoAgent):
        assert cls.enable_graph is fn, cls.__name__
        assert cls._step is agents._IntrAgent._step, cls.__name__
    # the captured route of the step: taken for the bound iterator while no hook supplies draws from the host
    step = inspect.getsource(agents._IntrAgent._step)
    assert 'step_graph' in step and '_hooked' in step


def test_a_capture_is_refused_off_the_single_process_state_path():
    """The refusals that need no device: pixels, more than one process, a plain Python iterator, a hook."""
    from exorl_amd import _lib as L, agents

    class Iter:
        engine, sampler, nstep, discount = object(), L.SAMPLER_PHILOX, 3, 0.99

    def agent(**kw):
        ag = agents._IntrAgent.__new__(agents._IntrAgent)
        ag.__dict__.update(dict(obs_type='states', world_size=1, noise_hook=None, reward_free=True), **kw)
        return ag

    assert agent(obs_type='pixels').enable_graph(Iter()) is False
    assert agent(world_size=2).enable_graph(Iter()) is False
    assert agent().enable_graph(iter([])) is False
    assert agent(cat_hook=lambda n: None).enable_graph(Iter()) is False
    assert agent(eps_hook=lambda s: None).enable_graph(Iter()) is False
    assert agent(noise_hook=lambda s: None).enable_graph(Iter()) is False
