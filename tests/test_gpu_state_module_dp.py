"""Sharded module step of the eight reward-free agents on STATE observations (shard_pretraining=True): kNN against more than 4096 targets,
RND's BatchNorm1d over the global batch (EXORL_INTR_XCHG_BN), SMM's mean and variance of log p* over it (EXORL_INTR_XCHG_MOMENTS), and
the phases the other six kinds already had, reached from the agents through IntrEngine.run_update.

Each module loss is a mean over the batch, so R module engines built with world_size=R, each on its B/R rows, whose gradient exchanges are
summed and whose batch-global statistics are gathered, make the single-engine step of the global batch. The virtual-rank tests run R
engines in this process and perform the exchanges themselves in rank order; the last tests run the product path in two processes over
gloo. The bars are those of tests/test_gpu_pixel_module_dp.py."""
import json
import os
import socket
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
KINDS = ['rnd', 'icm', 'icm_apt', 'disagreement', 'diayn', 'aps', 'smm', 'proto']
META = {'diayn': 6, 'aps': 5, 'smm': 4}          # skill / task / z columns behind the observation
SMALL = dict(O=12, A=4, H=64, R=16)
SHIPPED = dict(O=24, A=6, H=1024, R=512)         # configs/agent/{rnd,icm_apt}.yaml widths
LR = 1e-4


# ---------------------------------------------------------------------------------------------------- 1. kNN past 4096 targets
def _knn(lib, src, n_src, tgt, n_tgt, dim, k):
    from exorl_amd import _lib as L
    out = torch.empty(n_src, k, device='cuda')
    L.check(lib.exorl_knn_topk(src.data_ptr(), n_src, tgt.data_ptr(), n_tgt, dim, k, out.data_ptr(), None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize('same', [False, True])
@pytest.mark.parametrize('ns,nt,dim,k', [(1024, 8192, 512, 12), (1024, 8192, 10, 12), (1000, 5000, 70, 5), (64, 4097, 8, 3)])
def test_knn_topk_past_4096_targets(ns, nt, dim, k, same):
    from exorl_amd import _lib as L
    from oracle import knn
    lib = L.load()
    rs = np.random.RandomState(ns + nt + dim)
    tgt = rs.standard_normal((nt, dim)).astype(np.float32)
    src = tgt[:ns] if same else rs.standard_normal((ns, dim)).astype(np.float32)      # src is tgt: the rows' own distances are in the row
    td = torch.from_numpy(tgt).cuda()
    sd = td if same else torch.from_numpy(src).cuda()
    got = _knn(lib, sd, ns, td, nt, dim, k)
    rows = 64 if nt == 8192 else ns                      # every row of the small shapes, the first 64 of the large ones
    want = np.concatenate([knn.topk_smallest(knn.pairwise_l2(src[i:i + 8], tgt), k) for i in range(0, rows, 8)])      # (8, nt, dim) temporaries
    np.testing.assert_allclose(got[:rows], want, rtol=2e-5, atol=1e-6)
    assert np.all(np.diff(got, axis=1) >= 0)
    if same:
        assert np.all(got[:, 0] == 0.0)                  # self-distance is an exact zero (PBE relies on it)
    # the same pair distances, so the same k smallest: bit-equal to the merge of the top-k over the target halves (the LDS kernels)
    half = (nt + 1) // 2
    assert half <= 4096 and nt - half >= k
    lo = _knn(lib, sd, ns, td, half, dim, k)
    hi = _knn(lib, sd, ns, td[half:], nt - half, dim, k)
    merged = np.sort(np.concatenate([lo, hi], axis=1), axis=1)[:, :k]
    assert np.array_equal(got, merged)


def test_knn_topk_refuses_more_than_8192_targets():
    from exorl_amd import _lib as L
    x = torch.zeros(8256, 4, device='cuda')
    out = torch.empty(8, 3, device='cuda')
    assert L.load().exorl_knn_topk(x.data_ptr(), 8, x.data_ptr(), 8193, 4, 3, out.data_ptr(), None) != 0


# ---------------------------------------------------------------------------------------------------- module engines on state rows
def _intr(kind, shp, B, ws, rank, precision):
    from exorl_amd.engine import IntrEngine
    O, A, H, R = shp['O'], shp['A'], shp['H'], shp['R']
    kw = dict(lr=LR, precision=precision, world_size=ws, rank=rank)
    if kind in ('rnd', 'icm_apt'):
        kw['rep_dim'] = R
    if kind in META:
        kw['rep_dim'] = META[kind]
    if kind in ('icm_apt', 'aps'):
        kw.update(knn_k=12, knn_avg=True, knn_rms=True, knn_clip=0.0)
    if kind == 'disagreement':
        kw['n_models'] = 5
    if kind == 'proto':
        kw.update(rep_dim=R, knn_k=3, num_protos=16, queue_size=256, tau=0.1, target_tau=0.05)
        H = 2 * R
    m = IntrEngine(kind, O, A, H, B, **kw)
    g = torch.Generator(device='cpu').manual_seed(17)
    p = m.flat()
    p.copy_((torch.randn(p.numel(), generator=g) * 0.05).to(p.device))
    return m


def _global_batch(kind, shp, B, step):
    """The global batch of one update as the agents lay it out: [obs | meta] rows, actions, extrinsic rewards, the module's own draws."""
    O, A, M = shp['O'], shp['A'], META.get(kind, 0)
    rs = np.random.RandomState(900 + step)
    b = dict(obs=rs.standard_normal((B, O)).astype(np.float32), next_obs=rs.standard_normal((B, O)).astype(np.float32),
             action=rs.uniform(-1, 1, (B, A)).astype(np.float32), reward=rs.uniform(0, 1, B).astype(np.float32),
             eps=rs.standard_normal((B, 128)).astype(np.float32), u=rs.uniform(0, 1, 16).astype(np.float32))
    if M:
        meta = rs.standard_normal((B, M)).astype(np.float32) if kind == 'aps' else np.eye(M, dtype=np.float32)[rs.randint(0, M, B)]
        if kind == 'aps':
            meta /= np.linalg.norm(meta, axis=1, keepdims=True)
        b['obs'], b['next_obs'] = np.concatenate([b['obs'], meta], 1), np.concatenate([b['next_obs'], meta], 1)
    return b


class _Rank:
    """One module engine and the device rows an agent's batch slots would hold."""

    def __init__(self, kind, shp, B, ws, rank, precision):
        self.kind, self.B, self.O, self.M = kind, B, shp['O'], META.get(kind, 0)
        self.intr = _intr(kind, shp, B, ws, rank, precision)

    def set_batch(self, b, rows):
        self.t = {k: torch.from_numpy(np.ascontiguousarray(v[rows] if k != 'u' else v)).cuda() for k, v in b.items()}

    def args(self):
        t, k, W = self.t, self.kind, self.O + self.M
        p = {n: v.data_ptr() for n, v in t.items()}
        if k in ('rnd', 'icm', 'icm_apt', 'disagreement'):
            return (p['obs'], p['action'], p['next_obs'], p['reward'], p['reward'], True), {}
        if k == 'proto':
            return (p['obs'], None, p['next_obs'], p['reward'], p['reward'], True), dict(cat_uniform=p['u'])
        skill = p['obs'] + 4 * self.O
        if k == 'smm':
            return (p['obs'], None, None, p['reward'], p['reward'], True), dict(skill=skill, obs_ld=W, skill_ld=W, cat_uniform=p['eps'])
        return (p['obs'], None, p['next_obs'], p['reward'], p['reward'], True), dict(skill=skill, obs_ld=W, next_obs_ld=W, skill_ld=W)

    def reward(self):
        return self.t['reward'].cpu().numpy()

    def state(self):
        """Everything outside the activations that defines the module."""
        from exorl_amd import _lib as L
        st = {f'flat{w}': self.intr.flat(w).cpu().numpy() for w in (L.T_PARAM, L.T_ADAM_M, L.T_ADAM_V)}
        st['rms'] = self.intr._rms.cpu().numpy()
        if self.intr.bn is not None:
            st['bn'] = self.intr.bn.cpu().numpy()
        if self.intr.queue is not None:
            st['queue'] = self.intr.queue.cpu().numpy()
            st['queue_state'] = np.array([self.intr.queue_ptr(), self.intr.counter()], np.int64)
        st['opt_steps'] = np.array([self.intr.opt_steps()])
        return st


def _exchange(ranks, xid):
    """What the collective does across R GPUs, in this process and in rank order."""
    from exorl_amd import _lib as L
    bufs = [r.intr.exchange(xid) for r in ranks]
    ops = {op for _, op in bufs}
    assert len(ops) == 1
    if ops.pop() == L.XCHG_SUM:
        tot = bufs[0][0].clone()
        for b, _ in bufs[1:]:
            tot += b
        for b, _ in bufs:
            b.copy_(tot)
    else:
        for src, (b, _) in enumerate(bufs):
            for dst, _ in bufs:
                dst[src].copy_(b[src])


def _module_phases(ranks):
    seen, phase = [], 0
    per_rank = [r.args() for r in ranks]
    while True:
        nxt = {r.intr.update_phase(phase, *a, **k) for r, (a, k) in zip(ranks, per_rank)}
        assert len(nxt) == 1, nxt
        x = nxt.pop()
        seen.append(x)
        if x < 0:
            return seen
        _exchange(ranks, x)
        phase += 1


def _check_close(got, want, init, steps, what):
    d, moved = np.abs(got - want), np.abs(want - init)
    assert d.max() <= 2 * steps * LR, (what, float(d.max()))
    assert np.mean(d > 1e-6 + 1e-3 * moved) <= 1e-3, (what, float(np.mean(d > 1e-6 + 1e-3 * moved)))


# ---------------------------------------------------------------------------------------------------- 2. world_size 1: phases = one call
class _NoDist:
    """One rank: a sum all-reduce and an all-gather are the identity."""

    def all_reduce(self, t):
        pass

    def all_gather(self, out, t):
        out[0].copy_(t)


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('kind', KINDS)
def test_state_module_phases_equal_the_one_call_step_bit_for_bit(kind, precision):
    from exorl_amd import _lib as L
    from exorl_amd.engine import drive_phases
    B = 64
    one, ph = (_Rank(kind, SMALL, B, 1, 0, precision) for _ in range(2))
    for step in range(2):
        b = _global_batch(kind, SMALL, B, step)
        for r in (one, ph):
            r.set_batch(b, slice(None))
        a, k = one.args()
        one.intr.update(*a, **k)
        a, k = ph.args()
        seen = []

        def phase(p):
            seen.append(ph.intr.update_phase(p, *a, **k))
            return seen[-1]
        drive_phases(phase, ph.intr.exchange, 0, dist=_NoDist())
        assert seen == [L.INTR_XCHG_GRAD, -1], (kind, seen)         # one rank: no other exchange is named
        torch.cuda.synchronize()
        assert np.array_equal(one.reward(), ph.reward()), (kind, step)
        assert np.array_equal(one.intr.metrics_raw(), ph.intr.metrics_raw()), (kind, step)
        sa, sb = one.state(), ph.state()
        assert sa.keys() == sb.keys()
        for key in sa:
            assert np.array_equal(sa[key], sb[key]), (kind, step, key)


# ---------------------------------------------------------------------------------------------------- 3. virtual ranks
def _virtual_vs_single(kind, shp, B, R, precision, steps=3, params=True):
    from exorl_amd import _lib as L
    Br = B // R
    rows = [slice(i * Br, (i + 1) * Br) for i in range(R)]
    ranks = [_Rank(kind, shp, Br, R, i, precision) for i in range(R)]
    single = _Rank(kind, shp, B, 1, 0, precision)
    init = single.intr.flat().cpu().numpy()
    rms_kind = kind in ('rnd', 'icm_apt', 'aps')
    same = [L.IM_RMS_MEAN, L.IM_RMS_STD] if rms_kind else ([3, 7] if kind == 'smm' else [])      # global values on every rank
    for step in range(steps):
        b = _global_batch(kind, shp, B, step)
        for r, rw in zip(ranks, rows):
            r.set_batch(b, rw)
        single.set_batch(b, slice(None))
        seen = _module_phases(ranks)
        if kind == 'rnd':
            assert seen == [L.INTR_XCHG_BN, L.INTR_XCHG_GRAD, L.INTR_XCHG_MOMENTS, -1]
        if kind == 'smm':
            assert seen == [L.INTR_XCHG_GRAD, L.INTR_XCHG_MOMENTS, -1]
        a, k = single.args()
        single.intr.update(*a, **k)
        torch.cuda.synchronize()
        got_r, want_r = np.concatenate([r.reward() for r in ranks]), single.reward()
        # step 0 runs on identical parameters: every row to 1e-4 relative. Later steps run on parameters that differ within the Adam bars
        # below, and a row whose reward is a near-cancelling sum gets a floor of 1e-5 of the batch's scale
        floor = 1e-6 if step == 0 else 1e-6 + 1e-5 * float(np.abs(want_r).max())
        assert np.all(np.abs(got_r - want_r) <= 1e-4 * np.abs(want_r) + floor), (kind, step, float(np.abs(got_r - want_r).max()))
        mets = [r.intr.metrics_raw() for r in ranks]
        got_m = np.sum(mets, axis=0)
        for m in mets[1:]:
            assert np.array_equal(m[same], mets[0][same]), (kind, step)
        got_m[same] = mets[0][same]
        want_m = single.intr.metrics_raw()
        assert np.all(np.abs(got_m - want_m) <= 1e-4 * np.abs(want_m) + 1e-6), (kind, step, got_m, want_m)
        reps = [r.state() for r in ranks]
        for rep in reps[1:]:
            for key in rep:
                assert np.array_equal(rep[key], reps[0][key]), (kind, step, key)      # the replicas stay bit-identical
        if rms_kind:
            assert np.allclose(reps[0]['rms'][:2], single.intr._rms.cpu().numpy()[:2], rtol=1e-4, atol=1e-6), kind
        if kind == 'rnd':
            bn = single.intr.bn.cpu().numpy()
            assert np.allclose(reps[0]['bn'], bn, rtol=1e-5, atol=1e-6), (kind, step)
            assert reps[0]['bn'][-1] == bn[-1] == 2 * (step + 1)      # num_batches_tracked: the step and the reward pass
        if kind == 'proto':
            assert np.array_equal(reps[0]['queue_state'], single.state()['queue_state'])
    if params:
        _check_close(ranks[0].intr.flat().cpu().numpy(), single.intr.flat().cpu().numpy(), init, steps, (kind, precision))


@pytest.mark.parametrize('R', [2, 4])
@pytest.mark.parametrize('kind', KINDS)
def test_virtual_ranks_on_state_rows_equal_one_engine(kind, R):
    _virtual_vs_single(kind, SMALL, 64, R, 'fp32')


# ---------------------------------------------------------------------------------------------------- 4. shipped widths
@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('kind', ['rnd', 'icm_apt'])
def test_shipped_widths_two_ranks_equal_one_engine(kind, precision):
    _virtual_vs_single(kind, SHIPPED, 1024, 2, precision)


@pytest.mark.parametrize('kind', ['icm_apt', 'aps'])
def test_eight_ranks_of_1024_rows_equal_one_engine_at_8192(kind):
    """The node shape: the kNN reward of each rank's 1024 rows against the gathered 8192, and one engine's 8192 against themselves."""
    _virtual_vs_single(kind, SHIPPED, 8192, 8, 'fp32', steps=1, params=False)


# ---------------------------------------------------------------------------------------------------- 5. the product path in two processes
@pytest.fixture(scope='module')
def state_dp_run():
    """Two fresh rank processes (tests/_state_module_dp_worker.py) on cuda:0 over gloo; one wait with a hard limit, no retry."""
    tmp = Path(tempfile.mkdtemp(prefix='exorl_state_module_dp_'))
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        log = tmp / f'rank{rank}.log'
        procs.append((subprocess.Popen([sys.executable, str(ROOT / 'tests' / '_state_module_dp_worker.py'), str(tmp)], env=env,
                                       stdout=open(log, 'w'), stderr=subprocess.STDOUT), log))
    try:
        for p, log in procs:
            try:
                rc = p.wait(timeout=600)
            except subprocess.TimeoutExpired:
                pytest.fail(f'state module data-parallel rank timed out:\n{open(log).read()[-3000:]}')
            assert rc == 0, open(log).read()[-3000:]
    finally:
        for p, _ in procs:
            if p.poll() is None:
                p.kill()
                p.wait(timeout=30)
    return tmp


def _single_process(kind):
    import _state_module_dp_worker as W
    ag = W.build(kind, W.B_GLOBAL)
    assert ag.intr.world_size == 1 and ag.intr.batch == W.B_GLOBAL          # the flag is a no-op at world size 1
    W.hooks(ag, slice(None))
    init = {n: W.flat(v) for n, v in W.views(ag)}
    ms = [ag.update(iter([W.batch(kind, step)]), step) for step in range(W.STEPS)]
    return ag, init, ms


@pytest.mark.parametrize('kind', KINDS)
def test_two_process_sharded_state_agents_equal_single_process(state_dp_run, kind):
    import _state_module_dp_worker as W
    out = state_dp_run
    r0, r1 = np.load(out / f'{kind}_rank0.npz'), np.load(out / f'{kind}_rank1.npz')
    assert sorted(r0.files) == sorted(r1.files)
    for k in r0.files:
        assert np.array_equal(r0[k], r1[k]), (kind, k)              # replicas stay bit-identical
    assert list(r0['module_shape']) == [W.B_GLOBAL // 2, 2]         # no rows were gathered
    m0, m1 = (json.load(open(out / f'metrics_{kind}_rank{r}.json')) for r in (0, 1))
    assert m0 == m1 and len(m0) == W.STEPS                          # every rank reports the global means
    ag, init, ms = _single_process(kind)
    for step, m in enumerate(ms):
        assert m.keys() == m0[step].keys()
        for k, v in m.items():
            assert abs(m0[step][k] - v) <= 1e-4 * abs(v) + 1e-6, (kind, step, k, m0[step][k], v)
    for n, v in W.views(ag):
        _check_close(r0[n], W.flat(v), init[n], W.STEPS, (kind, n))


def test_two_process_default_still_gathers_the_rows(state_dp_run):
    """Without the flag ICM takes the replicated path: one module engine on the 2 * B/2 gathered rows, world_size 1."""
    import _state_module_dp_worker as W
    r0, r1 = (np.load(state_dp_run / f'icm_default_rank{r}.npz') for r in (0, 1))
    assert list(r0['module_shape']) == list(r1['module_shape']) == [W.B_GLOBAL, 1]
    assert np.array_equal(r0['module'], r1['module'])
