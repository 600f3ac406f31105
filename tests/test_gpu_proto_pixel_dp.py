"""Data-parallel pretraining step of Proto on pixels (exorl_intr_update_phase for Proto, ProtoAgent(..., shard_pretraining=True)) and the
multi-workgroup candidate draw that lets the global batch reach 8192 rows.

Each rank runs the online branch and the loss on its own rows; the target rows (for Sinkhorn) and the reward rows (for the candidate draw)
are all-gathered, and Sinkhorn and the draw run over all of them on every rank, deterministically, so the replicas hold bit-identical
queues. The virtual-rank tests run R engine pairs in this process and perform the exchanges themselves, in rank order; the last tests
run the product path in two processes over gloo against the reference's fixtures."""
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

import test_gpu_pixel_module_dp as MD

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
STDDEV = MD.STDDEV
SMALL = MD.SMALL                     # c, hw, A, feature_dim, hidden_dim, module hidden_dim (proj_dim)
PD, NP, Q, TOPK = 16, 16, 64, 3      # pred_dim, prototypes, queue, topk of the small shapes


def _proto(O, B, ws, rank, precision, H=SMALL[5], pd=PD, num_protos=NP, queue=Q):
    from exorl_amd.engine import IntrEngine
    m = IntrEngine('proto', O, SMALL[2], H, B, rep_dim=pd, lr=1e-4, knn_k=TOPK, num_protos=num_protos, queue_size=queue, tau=0.1,
                   target_tau=0.05, precision=precision, world_size=ws, rank=rank)
    g = torch.Generator(device='cpu').manual_seed(17)
    p = m.flat()
    p.copy_((torch.randn(p.numel(), generator=g) * 0.05).to(p.device))
    return m


class _Rank:
    """One (pixel engine, Proto engine) pair and the buffers ProtoAgent keeps."""

    def __init__(self, B, ws, rank, precision):
        C_, HW, A, F, H, HM = SMALL
        self.B = B
        self.pix = MD._pixel(C_, HW, A, F, H, B, ws, precision, 0, 0)
        self.O = self.pix.lib.exorl_encoder_out_dim(HW)
        self.intr = _proto(self.O, B, ws, rank, precision)
        self.dobs = torch.zeros(B, self.O, device=self.pix.device)

    def set_batch(self, b, rows):
        self.pix.set_batch(*[np.ascontiguousarray(x[rows]) for x in b])

    def step_args(self, fo, ft):
        s = self.pix.batch_slots()
        return (fo, None, ft, None, s.reward, 2), dict(next_obs_target=ft, dobs_out=self.dobs.data_ptr())

    def reward_args(self, fo, fn, u):
        s = self.pix.batch_slots()
        return (fo, None, fn, s.reward, s.reward, False), dict(cat_uniform=u.data_ptr() if u is not None else None)

    def reward(self):
        return self.pix._view(self.pix.batch_slots().reward, self.B).cpu().numpy()


def _uniforms(step):
    return torch.from_numpy(np.random.RandomState(50 + step).uniform(size=NP).astype(np.float32)).cuda()


def _step_sharded(ranks, rows, d, u):
    """One pretraining update of R virtual ranks: what ProtoAgent._update_pixels does under torch.distributed with shard_pretraining."""
    args = []
    for r, rw in zip(ranks, rows):
        r.pix.augment(d['so'][rw], d['sn'][rw])
        fo, ft = r.pix.encode(0), r.pix.encode(1, target=True)
        r.fo = fo
        args.append(r.step_args(fo, ft))
    MD._module_phases(ranks, args)
    for r in ranks:
        r.pix.encoder_step_phase(0, 0, r.dobs.data_ptr(), 1)
    MD._sum_into([r.pix.grad_buffer(2) for r in ranks])
    for r in ranks:
        r.pix.encoder_step_phase(1, 0, r.dobs.data_ptr(), 1)
    MD._module_phases(ranks, [r.reward_args(r.fo, r.pix.encode(1), u) for r in ranks])
    for r in ranks:
        r.pix.encode(0)
        r.pix.set_train_encoder(False)
    MD._pix_dp_step(ranks, rows, d, kept=True)
    for r in ranks:
        r.pix.encoder_target(0.05)


def _step_single(r, d, u):
    """The same update on one engine pair through the one-call forms (the world_size 1 product path)."""
    r.pix.augment(d['so'], d['sn'])
    fo, ft = r.pix.encode(0), r.pix.encode(1, target=True)
    a, k = r.step_args(fo, ft)
    r.intr.update(*a, **k)
    r.pix.encoder_step(0, r.dobs.data_ptr(), 1)
    a, k = r.reward_args(fo, r.pix.encode(1), u)
    r.intr.update(*a, **k)
    r.pix.encode(0)
    r.pix.set_train_encoder(False)
    r.pix.update(STDDEV, None, None, d['nc'], d['na'], keep_encoded=True)
    r.pix.encoder_target(0.05)


def _params(r):
    from exorl_amd import _lib as L
    out = {'module': r.intr.flat(L.T_PARAM).cpu().numpy()}
    for net, name in ((0, 'encoder'), (1, 'actor'), (2, 'critic')):
        out[name] = torch.cat([r.pix.tensor(net, i).reshape(-1) for i in range(r.pix.num_tensors(net))]).cpu().numpy()
    return out


def _replicated(r):
    return {'module': r.intr.flat().cpu().numpy(), 'queue': r.intr.queue.cpu().numpy(), 'queue_ptr': np.array(r.intr.queue_ptr()),
            'counter': np.array(r.intr.counter()),
            'encoder': torch.cat([r.pix.tensor(0, i).reshape(-1) for i in range(r.pix.num_tensors(0))]).cpu().numpy(),
            'encoder_target': torch.cat([t.reshape(-1) for t in r.pix.encoder_target_tensors(
                [s for l in range(4) for s in ((32, SMALL[0] if l == 0 else 32, 3, 3), (32,))])]).cpu().numpy()}


# ---------------------------------------------------------------------------------------------------- 1. world_size 1: phases = one call
@pytest.mark.parametrize('precision', ['fp32', 'bf16x6'])
def test_proto_phases_equal_the_one_call_step_bit_for_bit(precision):
    from exorl_amd import _lib as L
    from exorl_amd.engine import drive_phases
    B = 64
    one, ph = (_Rank(B, 1, 0, precision) for _ in range(2))
    for step, d in enumerate(MD._draws(B, SMALL[2], 3, 0)):
        b, _ = MD._batch(step, B, SMALL[0], SMALL[1], SMALL[2], 0)
        u = _uniforms(step) if step != 1 else None              # step 1: the module's own Philox draw
        for r in (one, ph):
            r.set_batch(b, slice(None))
        for train in (2, 0, 1):
            outs = []
            for r in (one, ph):
                r.pix.augment(d['so'], d['sn'])
                fo, ft, fn = r.pix.encode(0), r.pix.encode(1, target=True), r.pix.encode(1)
                s = r.pix.batch_slots()
                outs.append(((fo, None, fn, s.reward, s.reward, train),
                             dict(next_obs_target=ft, dobs_out=r.dobs.data_ptr(), cat_uniform=u.data_ptr() if u is not None else None)))
            one.intr.update(*outs[0][0], **outs[0][1])
            seen = []

            def phase(p):
                nxt = ph.intr.update_phase(p, *outs[1][0], **outs[1][1])
                seen.append(nxt)
                return nxt
            drive_phases(phase, ph.intr.exchange, 0, dist=MD._NoDist())
            # one rank names no gather: only the gradient exchange of a training call (a sum over one rank)
            assert seen == ([L.INTR_XCHG_GRAD, -1] if train else [-1]), (train, seen)
            torch.cuda.synchronize()
            assert np.array_equal(one.reward(), ph.reward()), (step, train)
            assert np.array_equal(one.intr.metrics_raw(), ph.intr.metrics_raw()), (step, train)
            assert np.array_equal(one.dobs.cpu().numpy(), ph.dobs.cpu().numpy()), (step, train)
            for what in (L.T_PARAM, L.T_ADAM_M, L.T_ADAM_V):
                assert np.array_equal(one.intr.flat(what).cpu().numpy(), ph.intr.flat(what).cpu().numpy()), (step, train, what)
            assert np.array_equal(one.intr.queue.cpu().numpy(), ph.intr.queue.cpu().numpy()), (step, train)
            assert one.intr.queue_ptr() == ph.intr.queue_ptr() and one.intr.counter() == ph.intr.counter()
            assert one.intr.opt_steps() == ph.intr.opt_steps()


# ---------------------------------------------------------------------------------------------------- 2. the candidate draw at 8192 rows
def _chunked_kth(z, queue, k):
    from oracle.knn import pairwise_l2, topk_smallest
    return np.concatenate([topk_smallest(pairwise_l2(z[i:i + 512], queue), k)[:, -1] for i in range(0, len(z), 512)])


@pytest.mark.parametrize('B', [4096, 8192])
def test_candidate_draw_beyond_the_lds_form_matches_the_oracle(B):
    """One engine on state widths at a batch whose (B, PC_P + 1) slab does not fit in LDS: the multi-workgroup draw against
    OracleProto.reward, which picks by searchsorted in a float64 cumulative table."""
    from oracle.nets import linear_fwd
    from oracle.proto import OracleProto, l2_normalize
    O, H, pd, P, Qs = 24, 32, 16, 32, 96
    m = _proto(O, B, 1, 0, 'fp32', H=H, pd=pd, num_protos=P, queue=Qs)
    rs = np.random.RandomState(8 + B)
    params = [m.tensor(None, i).cpu().numpy() for i in range(7)]
    orc = OracleProto(params, queue_size=Qs, tau=0.1, topk=TOPK)
    total_near = 0
    for step in range(2):
        nobs = rs.standard_normal((B, O)).astype(np.float32)
        u = rs.uniform(size=P).astype(np.float32)
        nd, ud = torch.from_numpy(nobs).cuda(), torch.from_numpy(u).cuda()
        rew = torch.zeros(B, device='cuda')
        ptr0 = m.queue_ptr()
        m.update(nd.data_ptr(), None, nd.data_ptr(), None, rew.data_ptr(), False, cat_uniform=ud.data_ptr())
        want_r = orc.reward(nobs, u)[:, 0]
        torch.cuda.synchronize()
        assert m.queue_ptr() == orc.queue_ptr
        # the oracle's table, to tell a CDF-boundary case from a wrong pick
        C = orc.p[6]
        z = l2_normalize(linear_fwd(nobs, orc.p[0], orc.p[1]))[0]
        sc = (z @ C.T).astype(np.float32).T
        e = np.exp(sc - sc.max(1, keepdims=True)).astype(np.float32)
        cdf = np.cumsum((e / e.sum(1, keepdims=True, dtype=np.float32)).astype(np.float32).astype(np.float64), 1)
        thr = u.astype(np.float64) * cdf[:, -1]
        near = np.min(np.abs(cdf - thr[:, None]), axis=1) <= 1e-5 * cdf[:, -1]
        total_near += int(near.sum())
        q = m.queue.cpu().numpy()[ptr0:ptr0 + P]
        zd = z.astype(np.float64)
        picks = np.array([int(np.argmin(((zd - row) ** 2).sum(1))) for row in q.astype(np.float64)])
        cand = orc.last_candidates
        bad = np.nonzero(picks != cand)[0]
        print(f'[proto draw B={B}] step {step}: {int(near.sum())} of {P} prototypes within 1e-5 of a CDF boundary, '
              f'{len(bad)} picks differ from the oracle')
        assert all(near[p] for p in bad), [(int(p), int(picks[p]), int(cand[p])) for p in bad]
        # a boundary case keeps the device's row in both the queue and the rewards the oracle is checked against
        want_q = orc.queue.copy()
        for p in bad:
            want_q[ptr0 + p] = z[picks[p]]
        if len(bad):
            want_r = _chunked_kth(z, want_q, TOPK)
        np.testing.assert_allclose(m.queue.cpu().numpy(), want_q, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(rew.cpu().numpy(), want_r, rtol=1e-4, atol=2e-6)
        orc.queue = want_q
    print(f'[proto draw B={B}] {total_near} boundary prototypes in all')


# ---------------------------------------------------------------------------------------------------- 3. virtual ranks, small shapes
@pytest.mark.parametrize('R', [2, 4])
def test_virtual_ranks_equal_one_engine(R):
    from exorl_amd import _lib as L
    B, steps = 64, 3
    Br = B // R
    rows = [slice(i * Br, (i + 1) * Br) for i in range(R)]
    ranks = [_Rank(Br, R, i, 'fp32') for i in range(R)]
    single = _Rank(B, 1, 0, 'fp32')
    init = _params(single)
    for step, d in enumerate(MD._draws(B, SMALL[2], steps, 0)):
        b, _ = MD._batch(step, B, SMALL[0], SMALL[1], SMALL[2], 0)
        for r, rw in zip(ranks, rows):
            r.set_batch(b, rw)
        single.set_batch(b, slice(None))
        u = _uniforms(step)
        ptr0 = single.intr.queue_ptr()
        _step_sharded(ranks, rows, d, u)
        _step_single(single, d, u)
        torch.cuda.synchronize()
        reps = [_replicated(r) for r in ranks]
        for rep in reps[1:]:
            for k in rep:
                assert np.array_equal(rep[k], reps[0][k]), (R, step, k)      # the replicas stay bit-identical
        got_r, want_r = np.concatenate([r.reward() for r in ranks]), single.reward()
        floor = 1e-6 if step == 0 else 1e-6 + 1e-5 * float(np.abs(want_r).max())
        assert np.all(np.abs(got_r - want_r) <= 1e-4 * np.abs(want_r) + floor), (R, step, float(np.abs(got_r - want_r).max()))
        got_m, want_m = np.sum([r.intr.metrics_raw() for r in ranks], axis=0), single.intr.metrics_raw()
        assert np.all(np.abs(got_m - want_m) <= 1e-4 * np.abs(want_m) + 1e-6), (R, step, got_m, want_m)
        assert reps[0]['queue_ptr'] == single.intr.queue_ptr() and reps[0]['counter'] == single.intr.counter()
        # this step's queue rows: equal within 1e-4, or a Categorical pick that moved to the adjacent row of the gathered batch
        gat = ranks[0].intr.exchange(L.INTR_XCHG_REP)[0].reshape(B, PD).cpu().numpy().astype(np.float64)
        qs, qr = single.intr.queue.cpu().numpy()[ptr0:ptr0 + NP], reps[0]['queue'][ptr0:ptr0 + NP]
        flips = 0
        for p in range(NP):
            if np.abs(qs[p] - qr[p]).max() <= 1e-4:
                continue
            ks, kr = (int(np.argmin(((gat - row) ** 2).sum(1))) for row in (qs[p].astype(np.float64), qr[p].astype(np.float64)))
            assert abs(ks - kr) == 1, (R, step, p, ks, kr)
            flips += 1
        print(f'[proto virtual R={R}] step {step}: {flips} adjacent-row boundary flips in the queue')
    got, want = _params(ranks[0]), _params(single)
    for k in want:
        MD._check_close(got[k], want[k], init[k], steps, ('proto', R, k))


def test_sharded_proto_refuses_the_one_call_form():
    from exorl_amd import _lib as L
    r = _Rank(32, 2, 1, 'fp32')
    b, _ = MD._batch(0, 32, *SMALL[:3], 0)
    r.set_batch(b, slice(None))
    r.pix.augment()
    a, k = r.step_args(r.pix.encode(0), r.pix.encode(1, target=True))
    with pytest.raises(L.ExorlError, match='exorl_intr_update_phase'):
        r.intr.update(*a, **k)


# ---------------------------------------------------------------------------------------------------- 4, 5. the product path in two processes
@pytest.fixture(scope='module')
def proto_dp_run():
    """Two fresh rank processes (tests/_proto_pixel_dp_worker.py) on cuda:0 over gloo; one wait with a hard limit, no retry."""
    tmp = Path(tempfile.mkdtemp(prefix='exorl_proto_dp_'))
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        log = tmp / f'rank{rank}.log'
        procs.append((subprocess.Popen([sys.executable, str(ROOT / 'tests' / '_proto_pixel_dp_worker.py'), str(tmp)], env=env,
                                       stdout=open(log, 'w'), stderr=subprocess.STDOUT), log))
    try:
        for p, log in procs:
            try:
                rc = p.wait(timeout=900)
            except subprocess.TimeoutExpired:
                pytest.fail(f'Proto data-parallel rank timed out:\n{open(log).read()[-3000:]}')
            assert rc == 0, open(log).read()[-3000:]
    finally:
        for p, _ in procs:
            if p.poll() is None:
                p.kill()
                p.wait(timeout=30)
    return tmp


def _ranks_agree(out, name):
    r0, r1 = np.load(out / f'{name}_rank0.npz'), np.load(out / f'{name}_rank1.npz')
    for k in r0.files:
        assert np.array_equal(r0[k], r1[k]), (name, k)              # replicas stay bit-identical
    m0, m1 = (json.load(open(out / f'metrics_{name}_rank{r}.json')) for r in (0, 1))
    assert m0 == m1                                                 # every rank reports the global means
    return r0, m0


def test_two_process_sharded_proto_matches_the_reference_fixture(proto_dp_run, gold):
    """test_pixel_proto_vs_reference's run and bars, on 2 ranks x 2 rows."""
    z = np.load(gold / 'pixel_proto.npz')
    st, ms = _ranks_agree(proto_dp_run, 'fixture')
    keys = [str(k) for k in z['metric_keys']]
    assert len(ms) == int(z['dims'][6])
    for i, m in enumerate(ms):
        assert sorted(m.keys()) == keys
        np.testing.assert_allclose(np.array([m[k] for k in keys]), z['metrics'][i], rtol=2e-4, atol=3e-6, err_msg=f'step {i} {keys}')
    for nm in ('encoder', 'encoder_target', 'critic', 'protos', 'projector', 'predictor_target'):
        for key in [k for k in st.files if k.startswith(nm + '/')]:
            k = key.split('/', 1)[1]
            if f'final/{nm}/{k}' in z.files:
                np.testing.assert_allclose(st[key], z[f'final/{nm}/{k}'].reshape(-1), rtol=1e-4, atol=2e-6, err_msg=key)
            else:
                np.testing.assert_allclose(st[key][::997], z[f'final_sample/{nm}/{k}'], rtol=1e-4, atol=2e-6, err_msg=key)
    np.testing.assert_allclose(st['queue'], z['final/queue'], rtol=1e-4, atol=1e-6)
    assert int(st['queue_ptr']) == int(z['final/queue_ptr'])


@pytest.mark.parametrize('precision', ['fp32', 'bf16x6'])
def test_two_process_config4_proto_matches_the_reference(proto_dp_run, gold, precision):
    """test_config4_proto_pixels_b1024_vs_reference's bars (see its docstring) with the 1024-row batch sharded 2 x 512."""
    z = np.load(gold / 'config4_proto_b1024.npz')
    st, ms = _ranks_agree(proto_dp_run, f'config4_{precision}')
    keys = [str(k) for k in z['metric_keys']]
    ref = z['metrics_fp64']
    band = np.max([np.abs(z[nm] - ref) for nm in ('metrics', 'metrics_1thread', 'metrics_no_onednn')], axis=0)
    band[1:] = band[1:].max(axis=0)
    for i, m in enumerate(ms):
        assert sorted(m.keys()) == sorted(keys)
        rel = {k: abs(m[k] - v) / (abs(v) + 1e-12) for k, v in zip(keys, ref[i])}
        print(f'[config 4 sharded 2x512, {precision}] update {i}: ' + ' '.join(f'{k}={e:.1e}' for k, e in rel.items()))
        for j, (k, v) in enumerate(zip(keys, ref[i])):
            assert abs(m[k] - v) <= max(1e-4 * abs(v) + 1e-6, 2.0 * band[i][j]), (precision, i, k, m[k], v, band[i][j])
        if i == 0:
            for k, v in zip(keys, ref[i]):
                assert abs(m[k] - v) <= 1e-4 * abs(v) + 1e-6, (i, k, m[k], v)
    worst = 0.0
    for nm in ('encoder', 'actor', 'critic', 'predictor', 'projector', 'protos'):
        for key in [k for k in st.files if k.startswith(nm + '/')]:
            k = key.split('/', 1)[1]
            got = st[key].astype(np.float64)
            init, r64, r32 = (z[f'{tag}/{nm}/{k}'].reshape(-1).astype(np.float64) for tag in ('init_sample', 'final_sample_fp64', 'final_sample'))
            d, d64, d32 = got - init, r64 - init, r32 - init
            if np.linalg.norm(d64) < 1e-12:
                continue
            cos = float(d @ d64 / (np.linalg.norm(d) * np.linalg.norm(d64) + 1e-30))
            cos32 = float(d32 @ d64 / (np.linalg.norm(d32) * np.linalg.norm(d64) + 1e-30))
            assert cos >= min(0.999, cos32 - 2e-3), (precision, nm, k, cos, cos32)
            worst = max(worst, 1 - cos)
    print(f'[config 4 sharded 2x512, {precision}] parameter steps vs the reference fp64 run: worst 1 - cos = {worst:.2e}')


# ---------------------------------------------------------------------------------------------------- 6. the flag without peers
def test_shard_pretraining_without_peers_changes_nothing(gold):
    import _proto_pixel_dp_worker as W
    z = np.load(gold / 'pixel_proto.npz')
    runs = []
    for shard in (False, True):
        ag = W.proto_agent(z, int(z['dims'][5]), shard=shard)
        assert ag.shard_pretraining is shard and ag.world_size == 1 and ag.intr.world_size == 1
        W.load_fixture_params(ag, z)
        ms = W.run_fixture(ag, z, slice(None))
        torch.cuda.synchronize()
        runs.append((ms, W.state(ag)))
        del ag
    (m0, s0), (m1, s1) = runs
    assert m0 == m1
    assert s0.keys() == s1.keys()
    for k in s0:
        assert np.array_equal(s0[k], s1[k]), k
