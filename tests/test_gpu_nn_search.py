"""The nearest-neighbour search and the key table on the GPU: exorl_nn_search against a float64 brute force on the same float32 inputs over
the grid of tests/_prdc_cases.py (indices equal for every row, distances within the fp32 difference form's bound), ties and exact zeros,
the same bits on every call and for every number of key ranges, and exorl_replay_build_keys against its numpy restatement bit for bit."""
import numpy as np
import pytest
import torch

import _prdc_cases as P
import _synth

pytestmark = pytest.mark.gpu


def search(keys, q, splits=0, dim=None, poison=True):
    """(idx int32, d2 float32) numpy arrays of exorl_nn_search on float32 arrays keys (N, pitch) and q (rows, q_ld)."""
    from exorl_amd import _lib as L
    lib = L.load()
    k, x = torch.from_numpy(np.ascontiguousarray(keys)).cuda(), torch.from_numpy(np.ascontiguousarray(q)).cuda()
    rows = q.shape[0]
    idx = torch.full((rows,), -7, dtype=torch.int32, device='cuda')
    d2 = torch.full((rows,), float('nan'), device='cuda')
    L.check(lib.exorl_nn_search(k.data_ptr(), keys.shape[0], keys.shape[1], dim or keys.shape[1], x.data_ptr(), q.shape[1], rows, splits,
                                idx.data_ptr(), d2.data_ptr(), L.current_stream()))
    torch.cuda.synchronize()
    return idx.cpu().numpy(), d2.cpu().numpy()


@pytest.mark.parametrize('g', [pytest.param(g, id='N{}-D{}-rows{}'.format(*g[:3])) for g in P.SEARCH_GRID])
def test_search_vs_float64_brute_force(g):
    N, D, rows, seed = g
    keys, q = P.search_inputs(N, D, rows, seed)
    want_idx, want_d2, gap = P.search_reference(keys, q)
    idx, d2 = search(keys, q)
    err = float(np.max(np.abs(d2.astype(np.float64) - want_d2) / want_d2))
    print(f'[nn search] N={N} D={D} rows={rows}: worst relative d2 error {err:.2e} (bar {(D + 3) * 2.0 ** -24:.2e}), smallest gap {gap.min():.2e}')
    assert np.array_equal(idx, want_idx.astype(np.int32)), np.flatnonzero(idx != want_idx)[:8]
    assert np.all(np.abs(d2.astype(np.float64) - want_d2) <= (D + 3) * 2.0 ** -24 * want_d2)


def test_ties_go_to_the_lowest_index_and_self_queries_are_exact_zeros():
    """Rows 100 .. 199 of the table repeat rows 0 .. 99, and so do rows 1900 .. 1999 (a later key tile, and with three ranges a later
    range); the queries are rows 0 .. 99 themselves, then rows 250 .. 259 (unique)."""
    rs = np.random.RandomState(5)
    keys = rs.standard_normal((2000, 30)).astype(np.float32)
    keys[100:200] = keys[:100]
    keys[1900:2000] = keys[:100]
    q = np.concatenate([keys[:100], keys[250:260]])
    for splits in (0, 1, 3):
        idx, d2 = search(keys, q, splits)
        assert idx.tolist() == list(range(100)) + list(range(250, 260)), splits
        assert d2.tobytes() == np.zeros(110, np.float32).tobytes(), splits


@pytest.mark.parametrize('N,D,rows', [(1000, 33, 72), (20000, 30, 200), (65, 256, 7)])
def test_same_bits_on_every_call_and_for_every_split(N, D, rows):
    keys, q = P.search_inputs(N, D, rows, 3)
    base = search(keys, q, 0)
    for splits in (0, 1, 3, 256):
        got = search(keys, q, splits)
        assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes(), splits


def test_pitch_pad_and_query_stride_do_not_count():
    """Keys at pitch 36 with the pad columns 33 .. 35 holding NaN, queries at a stride of 40 with NaN behind column 33: dim = 33 alone is
    read as data."""
    keys, q = P.search_inputs(500, 33, 70, 9)
    kp = np.full((500, 36), np.nan, np.float32)
    kp[:, :33] = keys
    qp = np.full((70, 40), np.nan, np.float32)
    qp[:, :33] = q
    a, b = search(keys, q), search(kp, qp, dim=33)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_bad_arguments_are_refused():
    from exorl_amd import _lib as L
    keys, q = P.search_inputs(10, 4, 2, 1)
    with pytest.raises(L.ExorlError, match='unsupported sizes'):
        search(keys, q, dim=5)
    with pytest.raises(L.ExorlError, match='unsupported sizes'):
        search(keys, q, splits=-1)


# ---- the key table ------------------------------------------------------------------------------------------------------------------
LENGTHS = [1, 5, 64, 130, 7]
O, A = 11, 3


def _table_arena():
    """Five episodes; the 7-step one is evicted and the rest put in a permuted order."""
    from exorl_amd.engine import ReplayEngine
    eps = _synth.synth_episodes(21, LENGTHS, O, A)
    eng = ReplayEngine((O,), np.float32, A, 0, 512, 16)
    slots = [eng.append_episode(ep) for ep in eps]
    eng.set_order(slots)
    eng.evict(slots[4])
    order = [3, 0, 2, 1]
    eng.set_order([slots[i] for i in order])
    return eng, [eps[i] for i in order]


@pytest.mark.parametrize('norm', [False, True])
@pytest.mark.parametrize('beta', [0.0, 2.0, 5.0])
@pytest.mark.parametrize('every', [1, 3])
def test_build_keys_is_the_numpy_restatement_bit_for_bit(norm, beta, every):
    eng, eps = _table_arena()
    mean = inv = None
    if norm:
        rs = np.random.RandomState(2)
        mean, inv = rs.standard_normal(O).astype(np.float32), rs.uniform(0.5, 2.0, O).astype(np.float32)
        eng.set_obs_normalizer(mean, inv)
    rows = eng.build_keys(beta, every)
    want = np.concatenate([P.keys_of(ep, beta, O, A, mean, inv) for ep in eps])[::every]
    got = eng.keys().cpu().numpy()
    assert rows == len(want) == -(-sum(LENGTHS[:4]) // every) and got.shape == want.shape == (rows, 16)
    assert got.tobytes() == want.tobytes()
    assert not got[:, O + A:].any()
    # a sampled row queried with its own action is at distance exactly 0 from its key
    res, pairs = eng.sample(8, 1, 0.99, sampler=2, pairs=np.array([[1, 1], [1, 1], [0, 130], [2, 64], [3, 5], [0, 1], [2, 7], [3, 1]], np.int32),
                            want_pairs=True)
    q = np.zeros((8, 16), np.float32)
    q[:, :O] = (np.float32(beta) * res[0].cpu().numpy()).astype(np.float32)
    q[:, O:O + A] = res[1].cpu().numpy()
    idx, d2 = search(got, q, dim=O + A)
    first = np.cumsum([0] + [len(ep['observation']) - 1 for ep in eps])
    if every == 1 and beta > 0:
        assert idx.tolist() == [int(first[p] + i - 1) for p, i in pairs.tolist()]
        assert d2.tobytes() == np.zeros(8, np.float32).tobytes()


def test_table_goes_stale_and_refusals():
    from exorl_amd import _lib as L
    from exorl_amd import agents
    from exorl_amd.engine import ReplayEngine
    eng, eps = _table_arena()
    with pytest.raises(L.ExorlError, match='no key table'):
        eng.keys()
    ag = agents.PRDCAgent('prdc', (O,), (A,), 'cuda', 1e-4, 32, 0.01, 0.2, 1, 8, 0.3, True, 2.5, beta=2.0)
    stale = [lambda: eng.append_episode(_synth.synth_episodes(3, [4], O, A)[0]), lambda: eng.evict(0),
             lambda: eng.set_order([1, 2]), lambda: eng.set_obs_normalizer(np.zeros(O, np.float32), np.ones(O, np.float32)),
             lambda: eng.clear_obs_normalizer()]
    for change in stale:
        eng.build_keys(2.0)
        epoch = eng.keys_info()[3]
        ag.engine.set_prdc(eng, 2.0)
        change()
        with pytest.raises(L.ExorlError, match='stale'):
            eng.keys()
        with pytest.raises(L.ExorlError, match='stale'):
            ag.engine.set_prdc(eng, 2.0)
        with pytest.raises(L.ExorlError, match='stale'):
            ag.engine.update(0.2)
        assert eng.build_keys(2.0) > 0 and eng.keys_info()[3] > epoch
    with pytest.raises(L.ExorlError, match='beta >= 0'):
        eng.build_keys(-1.0)
    with pytest.raises(L.ExorlError, match='key_every >= 1'):
        eng.build_keys(2.0, 0)
    empty = ReplayEngine((O,), np.float32, A, 0, 64, 4)
    with pytest.raises(L.ExorlError, match='no resident episode'):
        empty.build_keys(2.0)
    stacked = ReplayEngine((4, 8, 8), np.uint8, A, 0, 64, 4, frame_stack=2)
    with pytest.raises(ValueError):
        stacked.build_keys(2.0)
    assert stacked.lib.exorl_replay_build_keys(stacked.h, 2.0, 1, None) != 0 and b'stacks 2 frames' in stacked.lib.exorl_last_error()
