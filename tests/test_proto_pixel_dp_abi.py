"""CPU checks of Proto's sharded pretraining step in the C ABI and the agent's constructor: exorl_intr_workspace_bytes accepts a Proto
configuration with world_size > 1 up to a global batch of 8192 rows and carves its gather buffer and global-batch Sinkhorn scratch only
then; the Proto parameter check still names Proto; ProtoAgent takes shard_pretraining. No GPU is touched."""
import inspect

import pytest

O, A, PD, PJ, NP, Q = 39200, 9, 128, 512, 512, 2048        # config 4: pixel features, jaco actions, proto.yaml widths


def _cfg(batch, world, rank=0, num_protos=NP):
    from exorl_amd import _lib as L
    return L.IntrCfg(L.INTR_PROTO, O, A, PJ, PD, batch, 0, 3, 1, 1, 0, 0, 1e-4, 1.0, 0.0, 5.0, num_protos, Q, 0.1, 0.05,
                     1e-3, 1e-2, 0.5, 1.0, 1.0, 1.0, 150.0, 75.0, world, rank)


def _bytes(cfg):
    import ctypes
    from exorl_amd import _lib as L
    lib = L.load()
    n = lib.exorl_intr_workspace_bytes(ctypes.byref(cfg))
    return n, (lib.exorl_last_error() or b'').decode()


@pytest.mark.parametrize('world', [2, 4])
def test_sharded_proto_workspace_is_accepted_and_larger(world):
    one, _ = _bytes(_cfg(1024, 1))
    many, err = _bytes(_cfg(1024, world, world - 1))
    assert one > 0
    assert many > one, err
    # the gather buffer alone: world slots of batch x pred_dim floats
    assert many - one >= world * 1024 * PD * 4


def test_world_one_workspace_is_unchanged_by_the_rank_fields():
    a, _ = _bytes(_cfg(512, 0))
    b, _ = _bytes(_cfg(512, 1))
    assert a == b > 0


@pytest.mark.parametrize('batch, world', [(4096, 2), (1024, 8), (8192, 1)])
def test_global_batch_up_to_8192_rows(batch, world):
    n, err = _bytes(_cfg(batch, world, 0))
    assert n > 0, err


@pytest.mark.parametrize('batch, world', [(4097, 2), (1025, 8), (2048, 5)])
def test_global_batch_above_8192_rows_is_refused(batch, world):
    n, err = _bytes(_cfg(batch, world, 0))
    assert n == 0
    assert '8192' in err and 'Proto' in err, err


@pytest.mark.parametrize('world', [1, 2])
def test_proto_parameter_check_still_names_proto(world):
    n, err = _bytes(_cfg(64, world, 0, num_protos=0))
    assert n == 0
    assert 'Proto' in err, err


def test_proto_agent_accepts_shard_pretraining():
    from exorl_amd import agents
    sig = inspect.signature(agents.ProtoAgent.__init__)
    assert 'shard_pretraining' in sig.parameters
    assert sig.parameters['shard_pretraining'].default is False
