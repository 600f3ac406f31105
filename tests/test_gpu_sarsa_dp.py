"""OneStepTD3BCAgent's data-parallel step executed for real, in the pattern and at the bars of tests/test_gpu_iql_dp.py: two fresh child processes
(tests/_sarsa_dp_worker.py), both on cuda:0 over gloo, each with half of every 128-row global batch, next actions and noise included; the
replicas end bit-identical and equal one process on the whole batch (metrics 5e-5 relative + 2e-6; parameters rtol 5e-5, atol 5e-7 in fp32,
and for bf16x3 that file's rule), tests/test_gpu_rebrac_dp.py's rule unchanged. next_valid is a mean over the global batch: the halves' own
means differ, and so do the shares of rows on which each rank's critic target is at the dataset's next action."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
CHILD_LIMIT = 240       # seconds, per process


@pytest.fixture(scope='module')
def dp_out(tmp_path_factory):
    out = tmp_path_factory.mktemp('sarsa_dp')
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        log = out / f'rank{rank}.log'
        procs.append((subprocess.Popen([sys.executable, str(ROOT / 'tests' / '_sarsa_dp_worker.py'), str(out)], env=env,
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


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
def test_two_ranks_equal_one_process(dp_out, precision):
    import _sarsa_dp_worker as W
    r0, r1 = (np.load(dp_out / f'sarsa_{precision}_rank{r}.npz') for r in (0, 1))
    for k in W.NETS:
        assert np.array_equal(r0[k], r1[k]), (precision, k)                 # replicas stay bit-identical
    m0, m1 = (json.load(open(dp_out / f'metrics_rank{r}.json'))[precision] for r in (0, 1))
    assert m0 == m1 and len(m0) == W.STEPS                                  # every rank reports the global means
    ag = W.build_agent(precision, W.B_GLOBAL)
    start = {n: W.flat(getattr(ag, n)) for n in W.NETS}
    half = W.B_GLOBAL // 2
    for step in range(W.STEPS):
        b = W.global_batch(step)
        m = W.hooked(ag, W.global_noise(step)).update(iter([b]), step)
        assert set(m) == set(m0[step]) and 'next_valid' in m and 'critic_penalty' not in m
        for k, v in m.items():
            assert abs(m0[step][k] - v) <= 5e-5 * abs(v) + 2e-6, (precision, step, k, m0[step][k], v)
        # the global mean of next_valid, exactly representable (a count over 128), and not either half's own
        valid = b[6]
        assert m0[step]['next_valid'] == float(valid.mean()) and valid[:half].mean() != valid[half:].mean()
        assert abs(m0[step]['next_valid'] - float(valid[:half].mean())) > 0.1
        assert abs(m0[step]['batch_reward'] - float(b[2].astype(np.float64).mean())) <= 5e-5
    for n in W.NETS:
        want = W.flat(getattr(ag, n))
        assert not np.array_equal(want, start[n]), n                        # the net was stepped
        if precision == 'fp32':
            np.testing.assert_allclose(r0[n], want, rtol=5e-5, atol=5e-7, err_msg=f'{precision} {n}')
        else:       # Adam moves rounding-noise gradients by +-lr either way (tests/test_gpu_dp.py's bf16x3 rule)
            d = np.abs(r0[n] - want)
            assert np.mean(d > 2e-6 + 1e-4 * np.abs(want)) <= 5e-3 and d.max() <= 6.5e-4, (precision, n, d.max())
