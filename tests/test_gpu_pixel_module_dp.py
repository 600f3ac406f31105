"""Data-parallel pretraining step of the pixel module agents (exorl_intr_update_phase / _exchange, exorl_intr_cfg.world_size / rank,
exorl_pixel_agent_encoder_step_phase, exorl_pixel_agent_rnd_features_phase / _bn_partials).

Each module loss is a mean over the batch, so R module engines built with world_size=R, each on its B/R rows, whose gradient exchanges are
summed, make the single-process step of the global batch; the batch-global quantities (BatchNorm2d partial sums, the RMS moments, the kNN
targets) are exchanged too. The virtual-rank tests below run R engines in this process and perform the exchanges themselves in rank order
(sums, or copies of every rank's slot into every rank's buffer); the last tests run the product path in two processes over gloo."""
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
STDDEV = 0.2
KINDS = ['rnd', 'icm', 'icm_apt', 'disagreement', 'diayn', 'aps', 'smm']
META = {'diayn': 8, 'aps': 5, 'smm': 4}          # skill / task / z columns
REP = {'rnd': 32, 'icm_apt': 32, 'diayn': 8, 'aps': 5, 'smm': 4}


def _pixel(C_, HW, A, F, H, B, ws, precision, M, S):
    from exorl_amd import agents
    from exorl_amd.engine import PixelEngine
    torch.manual_seed(5)
    w = agents._pixel_init(C_, HW, A, F, H, M, S)
    e = PixelEngine((C_, HW, HW), A, F, H, B, precision=precision, meta_dim=M, sf_dim=S, world_size=ws)
    for net, ts in ((0, w['encoder']), (1, w['actor']), (2, w['critic'])):
        for i, t in enumerate(ts):
            dst = e.tensor(net, i)
            dst.copy_(torch.as_tensor(np.asarray(t)).reshape(dst.shape))
    e.sync_target()
    e.encoder_target(init=True)                  # RND's frozen encoder copy: any fixed weights, the same in every engine
    return e


def _intr(kind, O, A, H, B, ws, rank, precision):
    from exorl_amd.engine import IntrEngine
    kw = dict(rep_dim=REP.get(kind, 0), lr=1e-4, precision=precision, world_size=ws, rank=rank)
    if kind in ('icm_apt', 'aps'):
        kw.update(knn_k=12, knn_avg=True, knn_rms=True, knn_clip=0.0)
    if kind == 'disagreement':
        kw['n_models'] = 5
    if kind in ('rnd', 'smm'):
        kw['encoded'] = True
    m = IntrEngine(kind, O, A, H, B, **kw)
    g = torch.Generator(device='cpu').manual_seed(17)
    p = m.flat()
    p.copy_((torch.randn(p.numel(), generator=g) * 0.05).to(p.device))
    return m


def _draws(B, A, steps, M, seed=3):
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(steps):
        out.append(dict(so=rs.randint(0, 9, (B, 2)).astype(np.int32), sn=rs.randint(0, 9, (B, 2)).astype(np.int32),
                        sr=rs.randint(0, 9, (B, 2)).astype(np.int32), sr2=rs.randint(0, 9, (B, 2)).astype(np.int32),
                        nc=rs.standard_normal((B, A)).astype(np.float32), na=rs.standard_normal((B, A)).astype(np.float32),
                        eps=rs.standard_normal((B, 128)).astype(np.float32)))
    return out


def _batch(step, B, C_, HW, A, M):
    rs = np.random.RandomState(900 + step)
    obs = rs.randint(0, 256, (B, C_, HW, HW)).astype(np.uint8)
    nxt = rs.randint(0, 256, (B, C_, HW, HW)).astype(np.uint8)
    b = [obs, rs.uniform(-1, 1, (B, A)).astype(np.float32), rs.uniform(0, 1, B).astype(np.float32), np.full(B, 0.99, np.float32), nxt]
    meta = None
    if M:
        meta = np.eye(M, dtype=np.float32)[rs.randint(0, M, B)] if M != 5 else rs.standard_normal((B, M)).astype(np.float32)
    return b, meta


class _Rank:
    """One (pixel engine, module engine) pair and the device buffers an agent keeps."""

    def __init__(self, kind, shapes, B, ws, rank, precision):
        C_, HW, A, F, H, HM = shapes
        M = META.get(kind, 0)
        S = M if kind == 'aps' else 0
        self.kind, self.B, self.M = kind, B, M
        self.pix = _pixel(C_, HW, A, F, H, B, ws, precision, M, S)
        self.O = self.pix.lib.exorl_encoder_out_dim(HW)
        self.intr = _intr(kind, self.O, A, HM, B, ws, rank, precision)
        self.dobs = torch.zeros(B, self.O, device=self.pix.device)

    def set_batch(self, b, meta, rows):
        self.pix.set_batch(*[np.ascontiguousarray(x[rows]) for x in b])
        if meta is not None:
            self.pix.meta_rows().copy_(torch.from_numpy(np.ascontiguousarray(meta[rows])))

    def module_args(self, d, rows, fo=None, fn=None, train=True):
        s, k = self.pix.batch_slots(), self.kind
        dob = self.dobs.data_ptr()
        if k == 'rnd':
            return (fo, None, fn, s.reward, s.reward, train), (dict(dobs_out=dob) if train == 2 else {})
        if k in ('icm', 'icm_apt', 'disagreement'):
            return (fo, s.action, fn, s.reward, s.reward, True), dict(dobs_out=dob)
        if k in ('diayn', 'aps'):
            return (fo, None, fn, s.reward, s.reward, True), dict(skill=s.meta, skill_ld=self.M, dobs_out=dob)
        self.xz = torch.cat([self.pix.feature_view(fo), self.pix.meta_rows()], 1).contiguous()
        self.eps = torch.from_numpy(np.ascontiguousarray(d['eps'][rows])).to(self.pix.device)
        return (self.xz.data_ptr(), None, None, s.reward, s.reward, True), dict(skill=s.meta, obs_ld=self.xz.shape[1], skill_ld=self.M,
                                                                               cat_uniform=self.eps.data_ptr(), dobs_out=dob)

    def reward(self):
        return self.pix._view(self.pix.batch_slots().reward, self.B).cpu().numpy()


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


def _module_phases(ranks, per_rank_args):
    phase = 0
    while True:
        nxt = {r.intr.update_phase(phase, *a, **k) for r, (a, k) in zip(ranks, per_rank_args)}
        assert len(nxt) == 1, nxt
        x = nxt.pop()
        if x < 0:
            return
        _exchange(ranks, x)
        phase += 1


def _sum_into(bufs):
    tot = bufs[0].clone()
    for b in bufs[1:]:
        tot += b
    for b in bufs:
        b.copy_(tot)


def _pix_dp_step(ranks, rows, d, kept):
    for r, rw in zip(ranks, rows):
        if kept:
            r.pix.update_phase(0, STDDEV, noise_critic=d['nc'][rw], keep_encoded=True)
        else:
            r.pix.update_phase(0, STDDEV, d['so'][rw], d['sn'][rw], d['nc'][rw])
    _sum_into([r.pix.grad_buffer(0) for r in ranks])
    for r, rw in zip(ranks, rows):
        r.pix.update_phase(1, STDDEV, noise_actor=d['na'][rw])
    _sum_into([r.pix.grad_buffer(1) for r in ranks])
    for r in ranks:
        r.pix.update_phase(2, STDDEV)


def _step_sharded(ranks, rows, d):
    """One pretraining update of R virtual ranks (what _IntrAgent._update_pixels / RNDAgent._update_pixels do under torch.distributed)."""
    kind = ranks[0].kind
    if kind == 'rnd':
        def feats(key):
            for ph in range(2):
                for r, rw in zip(ranks, rows):
                    r.pix.rnd_features_phase(ph, d[key][rw] if ph == 0 else None)
                _sum_into([r.pix.bn_partials() for r in ranks])
            return [r.pix.rnd_features_phase(2) for r in ranks]
        f = feats('sr')
        _module_phases(ranks, [r.module_args(d, rw, fp, ft, 2) for r, rw, (fp, ft) in zip(ranks, rows, f)])
        for r in ranks:
            r.pix.encoder_step_phase(0, 0, r.dobs.data_ptr(), 2)
        _sum_into([r.pix.grad_buffer(2) for r in ranks])
        for r in ranks:
            r.pix.encoder_step_phase(1, 0, r.dobs.data_ptr(), 2)
        f = feats('sr2')
        _module_phases(ranks, [r.module_args(d, rw, fp, ft, False) for r, rw, (fp, ft) in zip(ranks, rows, f)])
        for r in ranks:
            r.pix.set_train_encoder(False)
        _pix_dp_step(ranks, rows, d, kept=False)
        return
    grad = 1 if kind in ('diayn', 'aps') else 0
    args = []
    for r, rw in zip(ranks, rows):
        r.pix.augment(d['so'][rw], d['sn'][rw])
        fo, fn = r.pix.encode(0), r.pix.encode(1)
        args.append(r.module_args(d, rw, fo, fn))
    _module_phases(ranks, args)
    for r in ranks:
        r.pix.encoder_step_phase(0, grad, r.dobs.data_ptr(), 0)
    _sum_into([r.pix.grad_buffer(2) for r in ranks])
    for r in ranks:
        r.pix.encoder_step_phase(1, grad, r.dobs.data_ptr(), 0)
        r.pix.set_train_encoder(False)
    _pix_dp_step(ranks, rows, d, kept=True)


def _step_single(r, d):
    """The same update on one engine pair through the one-call forms (the world_size 1 product path)."""
    all_ = slice(None)
    if r.kind == 'rnd':
        fp, ft = r.pix.rnd_features(d['sr'])
        a, k = r.module_args(d, all_, fp, ft, 2)
        r.intr.update(*a, **k)
        r.pix.encoder_step(0, r.dobs.data_ptr(), 2)
        fp, ft = r.pix.rnd_features(d['sr2'])
        a, k = r.module_args(d, all_, fp, ft, False)
        r.intr.update(*a, **k)
        r.pix.set_train_encoder(False)
        r.pix.update(STDDEV, d['so'], d['sn'], d['nc'], d['na'])
        return
    r.pix.augment(d['so'], d['sn'])
    fo, fn = r.pix.encode(0), r.pix.encode(1)
    a, k = r.module_args(d, all_, fo, fn)
    r.intr.update(*a, **k)
    r.pix.encoder_step(1 if r.kind in ('diayn', 'aps') else 0, r.dobs.data_ptr(), 0)
    r.pix.set_train_encoder(False)
    r.pix.update(STDDEV, None, None, d['nc'], d['na'], keep_encoded=True)


def _params(r):
    from exorl_amd import _lib as L
    out = {'module': r.intr.flat(L.T_PARAM).cpu().numpy()}
    for net, name in ((0, 'encoder'), (1, 'actor'), (2, 'critic')):
        out[name] = torch.cat([r.pix.tensor(net, i).reshape(-1) for i in range(r.pix.num_tensors(net))]).cpu().numpy()
    return out


def _replicated(r):
    return {'module': r.intr.flat().cpu().numpy(), 'rms': r.intr._rms.cpu().numpy(), 'bn2d': r.pix.bn2d().cpu().numpy(),
            'encoder': torch.cat([r.pix.tensor(0, i).reshape(-1) for i in range(r.pix.num_tensors(0))]).cpu().numpy()}


def _check_close(got, want, init, steps, what):
    d, moved = np.abs(got - want), np.abs(want - init)
    assert d.max() <= 2 * steps * 1e-4, (what, float(d.max()))
    assert np.mean(d > 1e-6 + 1e-3 * moved) <= 1e-3, (what, float(np.mean(d > 1e-6 + 1e-3 * moved)))


def _virtual_vs_single(kind, shapes, B, R, precision, steps=3):
    from exorl_amd import _lib as L
    C_, HW, A = shapes[0], shapes[1], shapes[2]
    M = META.get(kind, 0)
    Br = B // R
    rows = [slice(i * Br, (i + 1) * Br) for i in range(R)]
    ranks = [_Rank(kind, shapes, Br, R, i, precision) for i in range(R)]
    single = _Rank(kind, shapes, B, 1, 0, precision)
    init = _params(single)
    draws = _draws(B, A, steps, M)
    for step, d in enumerate(draws):
        b, meta = _batch(step, B, C_, HW, A, M)
        for r, rw in zip(ranks, rows):
            r.set_batch(b, meta, rw)
        single.set_batch(b, meta, slice(None))
        _step_sharded(ranks, rows, d)
        _step_single(single, d)
        torch.cuda.synchronize()
        got_r, want_r = np.concatenate([r.reward() for r in ranks]), single.reward()
        # step 0 runs on identical parameters: every row to 1e-4 relative. Later steps run on parameters that differ within the Adam bars
        # below, and a row whose reward is a near-cancelling sum (APS: log(1 + kNN) + task . phi) gets a floor of 1e-5 of the batch's scale
        floor = 1e-6 if step == 0 else 1e-6 + 1e-5 * float(np.abs(want_r).max())
        assert np.all(np.abs(got_r - want_r) <= 1e-4 * np.abs(want_r) + floor), (kind, step, float(np.abs(got_r - want_r).max()))
        mets = [r.intr.metrics_raw() for r in ranks]
        got_m = np.sum(mets, axis=0)
        if kind in ('rnd', 'icm_apt', 'aps'):
            for m in mets[1:]:
                assert np.array_equal(m[L.IM_RMS_MEAN:L.IM_RMS_STD + 1], mets[0][L.IM_RMS_MEAN:L.IM_RMS_STD + 1])
            got_m[L.IM_RMS_MEAN:L.IM_RMS_STD + 1] = mets[0][L.IM_RMS_MEAN:L.IM_RMS_STD + 1]
        want_m = single.intr.metrics_raw()
        assert np.all(np.abs(got_m - want_m) <= 1e-4 * np.abs(want_m) + 1e-6), (kind, step, got_m, want_m)
        reps = [_replicated(r) for r in ranks]
        for rep in reps[1:]:
            for k in rep:
                assert np.array_equal(rep[k], reps[0][k]), (kind, step, k)      # the replicas stay bit-identical
        if kind in ('rnd', 'icm_apt', 'aps'):
            assert np.allclose(reps[0]['rms'][:2], single.intr._rms.cpu().numpy()[:2], rtol=1e-4, atol=1e-6), kind
        if kind == 'rnd':
            assert np.allclose(reps[0]['bn2d'], single.pix.bn2d().cpu().numpy(), rtol=1e-5, atol=1e-6)
    got, want = _params(ranks[0]), _params(single)
    for k in want:
        _check_close(got[k], want[k], init[k], steps, (kind, precision, k))


SMALL = (3, 64, 6, 32, 128, 64)            # c, hw, A, feature_dim, hidden_dim, module hidden_dim


# ---------------------------------------------------------------------------------------------------- 1. world_size 1: phases = one call
@pytest.mark.parametrize('precision', ['fp32', 'bf16x6'])
@pytest.mark.parametrize('kind', KINDS)
def test_module_phases_equal_the_one_call_step_bit_for_bit(kind, precision):
    from exorl_amd import _lib as L
    from exorl_amd.engine import drive_phases
    B = 64
    one, ph = (_Rank(kind, SMALL, B, 1, 0, precision) for _ in range(2))
    for step, d in enumerate(_draws(B, SMALL[2], 2, META.get(kind, 0))):
        b, meta = _batch(step, B, SMALL[0], SMALL[1], SMALL[2], META.get(kind, 0))
        for r in (one, ph):
            r.set_batch(b, meta, slice(None))
        trains = (2, False) if kind == 'rnd' else (True,)
        for train in trains:
            outs = []
            for r in (one, ph):
                if kind == 'rnd':
                    fp, ft = r.pix.rnd_features(d['sr'])
                    a, k = r.module_args(d, slice(None), fp, ft, train)
                else:
                    r.pix.augment(d['so'], d['sn'])
                    a, k = r.module_args(d, slice(None), r.pix.encode(0), r.pix.encode(1))
                outs.append((a, k))
            one.intr.update(*outs[0][0], **outs[0][1])
            seen = []

            def phase(p):
                nxt = ph.intr.update_phase(p, *outs[1][0], **outs[1][1])
                seen.append(nxt)
                return nxt
            drive_phases(phase, ph.intr.exchange, 0, dist=_NoDist())
            assert seen[-1] == -1 and all(x == L.INTR_XCHG_GRAD for x in seen[:-1])
        torch.cuda.synchronize()
        assert np.array_equal(one.reward(), ph.reward())
        assert np.array_equal(one.intr.metrics_raw(), ph.intr.metrics_raw())
        assert np.array_equal(one.dobs.cpu().numpy(), ph.dobs.cpu().numpy())
        for what in (L.T_PARAM, L.T_ADAM_M, L.T_ADAM_V):
            assert np.array_equal(one.intr.flat(what).cpu().numpy(), ph.intr.flat(what).cpu().numpy()), (kind, step, what)
        assert np.array_equal(one.intr._rms.cpu().numpy(), ph.intr._rms.cpu().numpy())


class _NoDist:
    """One rank: a sum all-reduce and an all-gather are the identity."""

    def all_reduce(self, t):
        pass

    def all_gather(self, out, t):
        out[0].copy_(t)


@pytest.mark.parametrize('opt', [0, 2])
@pytest.mark.parametrize('precision', ['fp32', 'bf16x6'])
def test_encoder_step_phases_equal_the_one_call_form(opt, precision):
    B = 64
    one, ph = (_Rank('icm', SMALL, B, 1, 0, precision) for _ in range(2))
    b, _ = _batch(0, B, *SMALL[:3], 0)
    g = torch.Generator(device='cpu').manual_seed(4)
    dfeat = (torch.randn(B, one.O, generator=g) * 1e-3).to(one.pix.device)
    for r in (one, ph):
        r.set_batch(b, None, slice(None))
        r.pix.augment(np.zeros((B, 2), np.int32), np.zeros((B, 2), np.int32))
        r.pix.encode(0)
        r.dobs.copy_(dfeat)
    one.pix.encoder_step(0, one.dobs.data_ptr(), opt)
    ph.pix.encoder_step_phase(0, 0, ph.dobs.data_ptr(), opt)
    ph.pix.encoder_step_phase(1, 0, ph.dobs.data_ptr(), opt)
    torch.cuda.synchronize()
    sa, sb = one.pix.export_state(), ph.pix.export_state()
    assert np.array_equal(sa['steps'], sb['steps'])
    for key in sa['tensors']:
        for x, y in zip(sa['tensors'][key], sb['tensors'][key]):
            assert torch.equal(x, y), key
    for x, y in zip(sa['enc_extra'], sb['enc_extra']):
        assert torch.equal(x, y)


@pytest.mark.parametrize('precision', ['fp32', 'bf16x6'])
def test_rnd_features_phases_equal_the_one_call_form(precision):
    B = 64
    one, ph = (_Rank('rnd', SMALL, B, 1, 0, precision) for _ in range(2))
    b, _ = _batch(0, B, *SMALL[:3], 0)
    sh = np.random.RandomState(2).randint(0, 9, (B, 2)).astype(np.int32)
    for r in (one, ph):
        r.set_batch(b, None, slice(None))
    for _ in range(2):
        fa = one.pix.rnd_features(sh)
        ph.pix.rnd_features_phase(0, sh)
        ph.pix.rnd_features_phase(1)
        fb = ph.pix.rnd_features_phase(2)
        torch.cuda.synchronize()
        for pa, pb in zip(fa, fb):
            assert torch.equal(one.pix.feature_view(pa), ph.pix.feature_view(pb))
        assert torch.equal(one.pix.bn2d(), ph.pix.bn2d())


def test_sharded_engines_refuse_the_one_call_forms():
    from exorl_amd import _lib as L
    r = _Rank('icm', SMALL, 32, 2, 0, 'fp32')
    b, _ = _batch(0, 32, *SMALL[:3], 0)
    r.set_batch(b, None, slice(None))
    r.pix.augment()
    a, k = r.module_args(None, slice(None), r.pix.encode(0), r.pix.encode(1))
    with pytest.raises(L.ExorlError, match='exorl_intr_update_phase'):
        r.intr.update(*a, **k)
    with pytest.raises(L.ExorlError, match='encoder_step_phase'):
        r.pix.encoder_step(0, r.dobs.data_ptr(), 0)
    with pytest.raises(L.ExorlError, match='rnd_features_phase'):
        r.pix.rnd_features()
    with pytest.raises(L.ExorlError, match='Proto'):
        _intr('proto', 64, 6, 32, 32, 2, 0, 'fp32')


# ---------------------------------------------------------------------------------------------------- 2. virtual ranks, small shapes
@pytest.mark.parametrize('R', [2, 4])
@pytest.mark.parametrize('kind', KINDS)
def test_virtual_ranks_equal_one_engine(kind, R):
    _virtual_vs_single(kind, SMALL, 64, R, 'fp32')


# ---------------------------------------------------------------------------------------------------- 3. config-4 size
@pytest.mark.parametrize('case', ['icm_bf16x6', 'icm_fp32', 'rnd_bf16x6', 'aps_bf16x6'])
def test_config4_two_ranks_equal_one_engine(case):
    kind, precision = case.split('_')
    _virtual_vs_single(kind, (3, 84, 9, 50, 1024, 1024), 1024, 2, precision)


# ---------------------------------------------------------------------------------------------------- 4. the product path in two processes
@pytest.fixture(scope='module')
def module_dp_run():
    """Two fresh rank processes (tests/_pixel_module_dp_worker.py) on cuda:0 over gloo; one wait with a hard limit, no retry."""
    tmp = Path(tempfile.mkdtemp(prefix='exorl_module_dp_'))
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        log = tmp / f'rank{rank}.log'
        procs.append((subprocess.Popen([sys.executable, str(ROOT / 'tests' / '_pixel_module_dp_worker.py'), str(tmp)], env=env,
                                       stdout=open(log, 'w'), stderr=subprocess.STDOUT), log))
    try:
        for p, log in procs:
            try:
                rc = p.wait(timeout=600)
            except subprocess.TimeoutExpired:
                pytest.fail(f'module data-parallel rank timed out:\n{open(log).read()[-3000:]}')
            assert rc == 0, open(log).read()[-3000:]
    finally:
        for p, _ in procs:
            if p.poll() is None:
                p.kill()
                p.wait(timeout=30)
    return tmp


def _single_process(kind, hooked_eps=True):
    import _pixel_module_dp_worker as W
    ag = W.build(kind, W.B_GLOBAL)
    W.hooks(ag, slice(None), eps=hooked_eps)
    init = {n: W.flat(v) for n, v in W.views(ag)}
    ms = [ag.update(iter([W.batch(kind, step)]), step) for step in range(W.STEPS)]
    return ag, init, ms


@pytest.mark.parametrize('kind', KINDS)
def test_two_process_module_dp_equals_single_process(module_dp_run, kind):
    import _pixel_module_dp_worker as W
    out = module_dp_run
    r0, r1 = np.load(out / f'{kind}_rank0.npz'), np.load(out / f'{kind}_rank1.npz')
    for k in r0.files:
        assert np.array_equal(r0[k], r1[k]), (kind, k)              # replicas stay bit-identical
    m0, m1 = (json.load(open(out / f'metrics_{kind}_rank{r}.json')) for r in (0, 1))
    assert m0 == m1 and len(m0) == W.STEPS                          # every rank reports the global means
    ag, init, ms = _single_process(kind)
    for step, m in enumerate(ms):
        assert m.keys() == m0[step].keys()
        for k, v in m.items():
            assert abs(m0[step][k] - v) <= 1e-4 * abs(v) + 1e-6, (kind, step, k, m0[step][k], v)
    for n, v in W.views(ag):
        _check_close(r0[n], W.flat(v), init[n], W.STEPS, (kind, n))


def test_two_process_unhooked_smm_draws_the_single_process_epsilon(module_dp_run):
    import _pixel_module_dp_worker as W
    r0, r1 = (np.load(module_dp_run / f'smm_unhooked_rank{r}.npz') for r in (0, 1))
    m0 = json.load(open(module_dp_run / 'metrics_smm_unhooked_rank0.json'))
    ag, init, ms = _single_process('smm', hooked_eps=False)
    for step, m in enumerate(ms):
        assert abs(m0[step]['loss_vae'] - m['loss_vae']) <= 1e-4 * abs(m['loss_vae']) + 1e-6, (step, m0[step]['loss_vae'], m['loss_vae'])
    for n, v in W.views(ag):
        assert np.array_equal(r0[n], r1[n]), n
        _check_close(r0[n], W.flat(v), init[n], W.STEPS, ('smm unhooked', n))
