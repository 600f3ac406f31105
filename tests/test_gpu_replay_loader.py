"""What the replay iterator's single load path guarantees: a shard is scanned, sized and seeded the same way whichever of the
iterator's entry points is touched first."""
import numpy as np
import pytest
import torch

import _synth

pytestmark = pytest.mark.gpu
LENGTHS = [5, 9, 3, 12, 7, 4]
O, A, B = 24, 6, 16
FIRST = ['next', 'sample_into', 'engine', 'obs_normalizer', 'holdout']


@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
    from exorl_amd.replay_buffer import save_episode
    d = tmp_path_factory.mktemp('replay_loader') / 'buffer'
    d.mkdir()
    for i, ep in enumerate(_synth.synth_episodes(22, LENGTHS, O, A)):
        save_episode(ep, d / f'episode_{i}_{LENGTHS[i]}.npz')
    return d


def raw(tensors):
    return [t.cpu().numpy().tobytes() for t in tensors]


def touch_first(it, first):
    """The first thing done to a fresh iterator; returns the training batches it produced (one or none)."""
    from exorl_amd import _lib as L
    if first == 'next':
        return [raw(next(it))]
    if first == 'sample_into':
        obs, nobs = torch.empty(B, O, device='cuda:0'), torch.empty(B, O, device='cuda:0')
        act, rew, disc = torch.empty(B, A, device='cuda:0'), torch.empty(B, 1, device='cuda:0'), torch.empty(B, 1, device='cuda:0')
        it.sample_into(L.BatchOut(obs.data_ptr(), 4 * O, act.data_ptr(), A, rew.data_ptr(), disc.data_ptr(), nobs.data_ptr(), 4 * O, None, 0))
        torch.cuda.synchronize()
        return [raw((obs, act, rew, disc, nobs))]
    assert getattr(it, first) is not None
    return []


def test_first_touch_does_not_change_what_is_sampled(dataset):
    """Offline, Philox, one shard, normalize_obs and a hold-out split: the first three training batches, the first hold-out batch and the
    normaliser are byte-equal whether next(), sample_into(), .engine, .obs_normalizer or .holdout comes first."""
    from exorl_amd.replay_buffer import make_offline_replay_loader
    seen = {}
    for first in FIRST:
        it = iter(make_offline_replay_loader(None, dataset, 10**6, B, 1, 0.99, sampler='philox', seed=4, normalize_obs=True, holdout_every=2))
        batches = touch_first(it, first)
        while len(batches) < 3:
            batches.append(raw(next(it)))
        seen[first] = (batches, raw(next(it.holdout)), [np.asarray(x).tobytes() for x in it.obs_normalizer])
        assert len(it.shards) == 1 and it.shards[0].seeded and it.engine is it.shards[0].engine
    for first in FIRST[1:]:
        for what, got, want in zip(('training batches', 'hold-out batch', 'obs_normalizer'), seen[first], seen[FIRST[0]]):
            assert got == want, (first, what)
    batches = seen[FIRST[0]][0]
    assert batches[0] != batches[1] != batches[2]            # the stream moves: equal digests are not three copies of one batch


def test_each_shard_is_sized_from_its_own_files(dataset):
    """Two shards on one loader (no .engine): each holds exactly what _OfflineShard.select gives its worker, in an arena of its own size."""
    from exorl_amd.replay_buffer import _OfflineShard, make_offline_replay_loader
    it = iter(make_offline_replay_loader(None, dataset, 10**6, B, 2, 0.99, sampler='philox', seed=4))
    assert it.engine is None
    for _ in range(2):
        assert len(next(it)) == 5
    want = [_OfflineShard.select(dataset, 10**6 // 2, 2, w) for w in range(2)]
    assert [n for _, n in want] == [5 + 3 + 7, 9 + 12 + 4]
    assert sum(len(s.fns) for s in it.shards) == sum(len(fns) for fns, _ in want) == len(LENGTHS)
    for shard, (fns, size) in zip(it.shards, want):
        assert shard.fns == fns and shard.size == size
        live, used = shard.engine.num_rows()
        assert live == used == size + len(fns)               # len + 1 rows per episode, nothing from the other shard's files
