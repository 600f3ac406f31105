"""CPU checks of the sharded module step on state rows in the C ABI and the agents' constructors: exorl_intr_workspace_bytes accepts RND and
SMM on un-encoded rows with world_size > 1 and carves their gather slots, ICM-APT and APS take a global batch of up to 8192 rows, the
world-1 workspace of every kind is what it was before, the BatchNorm1d exchange constant matches the header, and all eight reward-free agent
classes take shard_pretraining. No GPU is touched."""
import ctypes
import inspect
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
O, A = 24, 6
# kind -> (hidden_dim, rep_dim): the shipped widths (configs/agent/*.yaml); Proto: proj_dim, pred_dim, 512 prototypes, a 2048-row queue
SHAPES = {'rnd': (1024, 512), 'icm': (1024, 0), 'icm_apt': (1024, 512), 'disagreement': (1024, 0), 'diayn': (1024, 16), 'proto': (512, 128),
          'aps': (1024, 10), 'smm': (1024, 4)}
# exorl_intr_workspace_bytes of the configurations below at world_size 1, batch 1024 and 4096, recorded from the commit before the chunked
# kNN selection and the state-row exchanges went in
WORLD1_BYTES = {'rnd': (63564544, 158255872), 'icm': (19473920, 72484352), 'icm_apt': (93095424, 320669184),
                'disagreement': (47704576, 177293824), 'diayn': (34383360, 85132800), 'proto': (26885376, 94825728),
                'aps': (38479360, 152143360), 'smm': (44816896, 122083840)}


def _cfg(kind, batch, world=1, rank=0, flags=0):
    from exorl_amd import _lib as L
    from exorl_amd.engine import IntrEngine
    H, R = SHAPES[kind]
    return L.IntrCfg(IntrEngine.KINDS[kind], O, A, H, R, batch, 0, 12, 1, 1, 0, flags, 1e-4, 1.0, 0.0, 5.0, 512, 2048, 0.1, 0.05,
                     1e-3, 1e-2, 0.5, 1.0, 1.0, 1.0, 150.0, 75.0, world, rank)


def _bytes(cfg):
    from exorl_amd import _lib as L
    lib = L.load()
    n = lib.exorl_intr_workspace_bytes(ctypes.byref(cfg))
    return n, (lib.exorl_last_error() or b'').decode()


@pytest.mark.parametrize('world', [2, 8])
@pytest.mark.parametrize('kind', ['rnd', 'smm'])
def test_rnd_and_smm_on_state_rows_accept_world_size(kind, world):
    one, _ = _bytes(_cfg(kind, 1024))
    many, err = _bytes(_cfg(kind, 1024, world, world - 1))
    assert one > 0
    assert many > one, err
    # the gather slots alone: (n, mean, M2) doubles per rank — per feature for RND's BatchNorm1d, plus the RMS moments; SMM's log p* moments
    slots = world * 3 * 8 * ((O + 1) if kind == 'rnd' else 1)
    assert many - one >= slots


@pytest.mark.parametrize('batch, world', [(1024, 8), (4096, 2), (8192, 1)])
@pytest.mark.parametrize('kind', ['icm_apt', 'aps'])
def test_knn_kinds_accept_a_global_batch_of_8192_rows(kind, batch, world):
    for flags in (0, 1):                                 # state rows and EXORL_INTR_ENCODED
        n, err = _bytes(_cfg(kind, batch, world, 0, flags))
        assert n > 0, err


@pytest.mark.parametrize('batch, world', [(1025, 8), (4097, 2)])
@pytest.mark.parametrize('kind, name', [('icm_apt', 'ICM-APT'), ('aps', 'APS')])
def test_knn_kinds_refuse_more_than_8192_rows(kind, name, batch, world):
    n, err = _bytes(_cfg(kind, batch, world, 0))
    assert n == 0
    assert name in err and '8192' in err, err


def test_one_engine_at_8192_rows_blocks_its_distance_scratch():
    """8192 x 8192 distances would be 256 MB; the scratch is blocked by 1024 source rows (32 MB)."""
    for kind in ('icm_apt', 'aps'):
        big, err = _bytes(_cfg(kind, 8192))
        half, _ = _bytes(_cfg(kind, 4096))
        assert big > 0, err
        assert big - 2 * half < 0, (kind, big, half)      # 4096 x 4096 floats (64 MB) is already more than the blocked scratch


@pytest.mark.parametrize('kind', sorted(SHAPES))
def test_world_one_workspace_is_byte_for_byte_what_it_was(kind):
    for batch, want in zip((1024, 4096), WORLD1_BYTES[kind]):
        for world in (0, 1):
            n, err = _bytes(_cfg(kind, batch, world))
            assert n == want, (kind, batch, world, n, want, err)


def test_bn_exchange_constant_matches_the_header():
    from exorl_amd import _lib
    h = (ROOT / 'include' / 'exorl_hip.h').read_text()
    ids = {name: int(re.search(rf'#define EXORL_INTR_XCHG_{name}\s+(\d+)', h).group(1)) for name in ('GRAD', 'REP', 'MOMENTS', 'BN')}
    assert ids['BN'] == _lib.INTR_XCHG_BN == 3
    assert sorted(ids.values()) == [0, 1, 2, 3]           # the next free id


def test_all_reward_free_agents_take_shard_pretraining():
    from exorl_amd import agents
    for cls in (agents.RNDAgent, agents.ICMAgent, agents.ICMAPTAgent, agents.DisagreementAgent, agents.DIAYNAgent, agents.APSAgent,
                agents.SMMAgent, agents.ProtoAgent):
        sig = inspect.signature(cls.__init__)
        assert 'shard_pretraining' in sig.parameters, cls.__name__
        assert sig.parameters['shard_pretraining'].default is False, cls.__name__


def test_abi_version_is_unchanged():
    from exorl_amd import build
    lib = ctypes.CDLL(str(build.build(force=False, verbose=False)))
    lib.exorl_abi_version.restype = ctypes.c_int
    assert lib.exorl_abi_version() == 13
