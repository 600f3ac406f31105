"""CalQLAgent's data-parallel step executed for real, in the pattern of tests/test_gpu_rebrac_dp.py and at the bars
tests/test_gpu_dp.py holds CQL's two-process step to: two fresh child processes (tests/_calql_dp_worker.py), both on cuda:0 over gloo, each
with half of every 128-row global batch, bounds and noise included, with and without the Lagrange multiplier; the replicas end
bit-identical and equal one process on the whole batch (metrics 5e-5 relative + 2e-6; parameters rtol 5e-5, atol 5e-7, and 1e-5 with the
multiplier; the scalars' state rtol 5e-5). calql_bound_rate is a mean over the global batch: the halves' own rates are 0 and above 1/2."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
CHILD_LIMIT = 240       # seconds, per process


@pytest.fixture(scope='module')
def dp_out(tmp_path_factory):
    out = tmp_path_factory.mktemp('calql_dp')
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        log = out / f'rank{rank}.log'
        procs.append((subprocess.Popen([sys.executable, str(ROOT / 'tests' / '_calql_dp_worker.py'), str(out)], env=env,
                                       stdout=open(log, 'w'), stderr=subprocess.STDOUT), log))
    try:
        for p, log in procs:
            rc = p.wait(timeout=CHILD_LIMIT)
            assert rc == 0, open(log).read()[-3000:]
    finally:
        for p, _ in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    return out


@pytest.mark.parametrize('kind', ['cql', 'cql-lagrange'])
def test_two_ranks_equal_one_process(dp_out, kind):
    import _calql_dp_worker as W
    r0, r1 = (np.load(dp_out / f'calql_{kind}_rank{r}.npz') for r in (0, 1))
    for k in r0.files:
        assert np.array_equal(r0[k], r1[k]), (kind, k)                      # replicas stay bit-identical
    m0, m1 = (json.load(open(dp_out / f'metrics_rank{r}.json'))[kind] for r in (0, 1))
    assert m0 == m1 and len(m0) == W.STEPS                                  # every rank reports the global means
    ag = W.build_agent(kind, W.B_GLOBAL)
    start = {n: W.flat(getattr(ag, n)) for n in W.NETS}
    for step in range(W.STEPS):
        m = W.hooked(ag, W.global_noise(step)).update(iter([W.global_batch(step)]), step)
        assert set(m) == set(m0[step]) and 'calql_bound_rate' in m
        for k, v in m.items():
            assert abs(m0[step][k] - v) <= 5e-5 * abs(v) + 2e-6, (kind, step, k, m0[step][k], v)
        # the first half's own rate is 0 and the second half's is above 1/2: the global mean is neither
        assert 0.25 < m0[step]['calql_bound_rate'] < 0.5, m0[step]['calql_bound_rate']
    for n in W.NETS:
        want = W.flat(getattr(ag, n))
        assert not np.array_equal(want, start[n]), n                        # the net was stepped
        np.testing.assert_allclose(r0[n], want, rtol=5e-5, atol=1e-5 if kind == 'cql-lagrange' else 5e-7, err_msg=f'{kind} {n}')
    want = np.asarray(ag.engine.cql_alpha_state(), np.float64)
    np.testing.assert_allclose(r0['cql_scalars'], want, rtol=5e-5, atol=1e-9, err_msg=f'{kind} temperature / multiplier state')
    if kind == 'cql-lagrange':
        assert abs(want[3]) > 1e-5          # log_critic_alpha has moved off its initial 0
