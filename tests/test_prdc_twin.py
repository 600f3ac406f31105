"""CPU tests of PRDC's twin (tests/_prdc_twin.py) and of its case tables (tests/_prdc_cases.py): the restated step is oracle.twin64.Twin's
TD3+BC step bit for bit when every row's neighbour is the row itself; every gradient case qualifies (identical decisions in float32 and
float64, the neighbour of every row among them, with margins, a small near-kink set); every row of the stand-alone search's grid has the
gap the GPU test's equality of indices rests on. Nothing is searched here."""
import numpy as np
import pytest
import torch

import _grad_grid as G
import _prdc_cases as P
import _synth
from _prdc_twin import PRDCTwin, brute_force_nn
from oracle.twin64 import Twin


def test_brute_force_ties_zeros_and_gap():
    keys = torch.tensor([[0., 0.], [3., 4.], [3., 4.], [1., 0.]], dtype=torch.float64)
    q = torch.tensor([[3., 4.], [0.4, 0.], [10., 10.]], dtype=torch.float64)
    idx, d2, gap = brute_force_nn(q, keys)
    assert idx.tolist() == [1, 0, 1] and d2[0] == 0.0            # the first of two equal rows; an exact zero
    assert abs(float(gap[1]) - (0.36 - 0.16) / 0.36) < 1e-15 and float(gap[0]) == 0.0       # a tie has no gap
    one = brute_force_nn(q, keys[:1])
    assert one[0].tolist() == [0, 0, 0] and one[2].tolist() == [1.0, 1.0, 1.0]


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_restated_step_is_twin64s_when_the_neighbour_is_the_row_itself(dtype):
    """The table is the batch itself (distinct states, beta = 1e3: another row is at least 1e6 |s - s'|^2 away, the row itself at
    |mu - a|^2 <= 4 A): a_nn is the batch's action and every metric and gradient equals Twin('td3_bc')'s in every bit."""
    c = P.CASES[1]._replace(B=16)
    pa, pc = P.params(c)
    b = _synth.synth_batch(7, 0, c.B, c.O, c.A)
    ep = dict(observation=np.concatenate([b[0], b[0][:1]]), action=np.concatenate([b[1][:1], b[1]]))
    keys = P.keys_of(ep, 1e3, c.O, c.A)
    nz = P.noise(c)
    nz = [z[:c.B] for z in nz]
    r = PRDCTwin(list(pa.values()), list(pc.values()), keys, c.O, 1e3, dtype=dtype).update(b, 0, *nz)
    w = Twin('td3_bc', list(pa.values()), list(pc.values()), dtype=dtype).update(b, 0, *nz)
    assert r.nn_idx.tolist() == list(range(c.B))
    assert {k: v for k, v in r.metrics.items() if k != 'nn_dist'} == w.metrics
    for got, want in zip(r.critic_grads + r.actor_grads, w.critic_grads + w.actor_grads):
        assert got.tobytes() == want.tobytes()
    mu_err = np.sqrt(r.nn_d2)
    assert abs(r.metrics['nn_dist'] - float(mu_err.mean())) < 1e-6


@pytest.mark.parametrize('c', [pytest.param(c, id=P.case_id(c)) for c in P.CASES + [P.TRAJ]])
def test_case_qualifies(c):
    bad = P.qualify(c)
    r64, _ = P.twin_pair(c)
    gap = r64.decisions['nn'][1]
    print(f'[prdc case] {P.case_id(c)}: smallest neighbour gap {float(gap.min()):.3e}, distinct neighbours {len(set(r64.nn_idx.tolist()))} of {c.B} rows, '
          + ' '.join(f'|K_{s}|={n}' for s, n in r64.n_kinks.items()))
    assert not bad, bad
    assert float(gap.min()) >= G.MARGIN
    if c.rows == 'table':
        assert r64.nn_idx.tolist() == list(range(c.B))
    assert P.table(c).shape == (c.N, -(-(c.O + c.A) // 4) * 4) and not P.table(c)[:, c.O + c.A:].any()


@pytest.mark.parametrize('g', [pytest.param(g, id='N{}-D{}-rows{}'.format(*g[:3])) for g in P.SEARCH_GRID])
def test_search_grid_rows_have_the_gap(g):
    """The fp32 difference form errs by at most about (D + 3) 2^-24 relative per distance, 1.6e-5 at D = 256; MARGIN = 1e-4 leaves 3 x over
    two such errors, so a search within that bound returns the float64 neighbour for every row."""
    N, D, rows, seed = g
    keys, q = P.search_inputs(N, D, rows, seed)
    idx, d2, gap = P.search_reference(keys, q)
    assert keys.shape == (N, D) and q.shape == (rows, D) and keys.dtype == q.dtype == np.float32
    assert float(gap.min()) >= G.MARGIN, float(gap.min())
    assert 2 * (D + 3) * 2.0 ** -24 * 3 <= G.MARGIN
