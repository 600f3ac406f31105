"""Data-parallel DDPG pixel step (exorl_pixel_agent_update_phase / _grad_buffer / _set_comm, PixelCfg.world_size).

Within the DDPG pixel step the only cross-row quantities are means over the batch, so R engines built with world_size=R, each on its B/R rows,
whose exchange buffers are summed between the phases, make the single-process update of the global batch. The virtual-rank tests below do the
summing in this process in rank order (what the all-reduce does across GPUs); the last test runs the product path in two processes over gloo."""
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


def _engine(C_, HW, A, F, H, B, ws=1, precision='fp32', meta_dim=0, sf_dim=0, init_seed=5):
    from exorl_amd import agents
    from exorl_amd.engine import PixelEngine
    torch.manual_seed(init_seed)
    w = agents._pixel_init(C_, HW, A, F, H, meta_dim, sf_dim)
    e = PixelEngine((C_, HW, HW), A, F, H, B, precision=precision, meta_dim=meta_dim, sf_dim=sf_dim, world_size=ws)
    _load(e, w['encoder'], w['actor'], w['critic'])
    return e


def _load(e, enc, actor, critic):
    for net, ts in ((0, enc), (1, actor), (2, critic)):
        for i, t in enumerate(ts):
            dst = e.tensor(net, i)
            dst.copy_(torch.as_tensor(np.asarray(t)).reshape(dst.shape))
    e.sync_target()


def _state(e):
    """Everything that defines the training state (parameters, Adam moments, target, step counts, Philox counters) as flat numpy arrays."""
    st = e.export_state()
    out = {'steps': st['steps'], 'counters': st['counters']}
    for (net, what), ts in st['tensors'].items():
        out[f'{net}/{what}'] = torch.cat([t.reshape(-1) for t in ts]).numpy()
    for k, t in zip(('enc_m2', 'enc_v2', 'enc_target'), st['enc_extra']):
        out[k] = t.numpy()
    return out


def _assert_states_equal(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


def _frames(rs, B, C_, HW):
    return rs.randint(0, 256, (B, C_, HW, HW)).astype(np.uint8)


def _batch(seed, B, C_, HW, A, M=0):
    rs = np.random.RandomState(seed)
    obs, nxt = _frames(rs, B, C_, HW), _frames(rs, B, C_, HW)
    act = rs.uniform(-1, 1, (B, A)).astype(np.float32)
    rew = rs.uniform(0, 1, B).astype(np.float32)
    disc = np.full(B, 0.99, np.float32)
    meta = np.eye(M, dtype=np.float32)[rs.randint(0, M, B)] if M else None
    return obs, act, rew, disc, nxt, meta


def _set(e, b, rows=slice(None)):
    e.set_batch(*[np.ascontiguousarray(x[rows]) for x in b[:5]])
    if b[5] is not None:
        e.meta_rows().copy_(torch.from_numpy(np.ascontiguousarray(b[5][rows])))


def _encode_kept(e, so, sn):
    """The module agents' prologue with reward_free=False: augment and encode once, then the DDPG step on the kept (detached) encodings."""
    e.augment(so, sn)
    e.encode(0)
    e.encode(1)
    e.set_train_encoder(False)


def _phases(ranks, rows, so, sn, nc, na, kept):
    """One update of R virtual ranks; the exchanges are summed in rank order and written back to every rank."""
    def allreduce(ex):
        bufs = [e.grad_buffer(ex) for e in ranks]
        tot = bufs[0].clone()
        for b in bufs[1:]:
            tot += b
        for b in bufs:
            b.copy_(tot)
    for e, r in zip(ranks, rows):
        if kept:
            _encode_kept(e, so[r], sn[r])
            e.update_phase(0, STDDEV, noise_critic=nc[r], keep_encoded=True)
        else:
            e.update_phase(0, STDDEV, so[r], sn[r], nc[r])
    allreduce(0)
    for e, r in zip(ranks, rows):
        e.update_phase(1, STDDEV, noise_actor=na[r])
    allreduce(1)
    for e in ranks:
        e.update_phase(2, STDDEV)


def _shifts(rs, B):
    return rs.randint(0, 9, (B, 2)).astype(np.int32)


# ---------------------------------------------------------------------------------------------------- 1. phases = the fused update
@pytest.mark.parametrize('case', ['ddpg_fp32', 'ddpg_bf16x6', 'diayn_kept_fp32'])
def test_phases_equal_the_fused_update_bit_for_bit(case):
    kind, precision = case.split('_', 1)[0], case.rsplit('_', 1)[1]
    kept = kind == 'diayn'
    C_, HW, A, F, H, B, M = 3, 84, 6, 50, 256, 64, (16 if kept else 0)
    fused, phased = (_engine(C_, HW, A, F, H, B, precision=precision, meta_dim=M) for _ in range(2))
    for step in range(3):
        b = _batch(100 + step, B, C_, HW, A, M)
        for e in (fused, phased):
            _set(e, b)
        if kept:                             # Philox shifts and noise: the two engines' counters must advance alike
            for e in (fused, phased):
                _encode_kept(e, None, None)
            fused.update(STDDEV, keep_encoded=True)
            phased.update_phase(0, STDDEV, keep_encoded=True)
        else:
            fused.update(STDDEV)
            phased.update_phase(0, STDDEV)
        phased.update_phase(1, STDDEV)
        phased.update_phase(2, STDDEV)
        assert np.array_equal(fused.metrics_raw(), phased.metrics_raw()), (case, step)
    _assert_states_equal(_state(fused), _state(phased), case)


def test_world_size_above_one_needs_a_communicator_for_the_fused_update():
    from exorl_amd import _lib as L
    e = _engine(3, 84, 6, 50, 64, 8, ws=2)
    _set(e, _batch(1, 8, 3, 84, 6))
    with pytest.raises(L.ExorlError, match='exorl_pixel_agent_update_phase'):
        e.update(STDDEV)


# ---------------------------------------------------------------------------------------------------- 2. virtual ranks vs the reference
def test_two_virtual_ranks_vs_reference(gold):
    """tests/golden/pixel_ddpg.npz (the reference's DDPGAgent(obs_type='pixels'), B=4, 3 updates) as 2 ranks x 2 rows."""
    import _synth
    from oracle import pixels
    from exorl_amd import _lib as L
    from exorl_amd.engine import METRIC_KEYS
    z = np.load(gold / 'pixel_ddpg.npz')
    C_, HW, A, F, H, B, N = [int(v) for v in z['dims']]
    R, Br = 2, B // 2
    esh, ash, csh = pixels.pixel_param_shapes(C_, A, F, H, 39200)
    ps = [list(_synth.synth_params(sh, 50 + i).values()) for i, sh in enumerate((esh, ash, csh))]
    from exorl_amd.engine import PixelEngine
    ranks = []
    for _ in range(R):
        e = PixelEngine((C_, HW, HW), A, F, H, Br, world_size=R)
        _load(e, *ps)
        ranks.append(e)
    rows = [slice(r * Br, (r + 1) * Br) for r in range(R)]
    noise = _synth.NoiseStream(21)
    shifts = iter(z['shifts'])
    keys = [str(k) for k in z['metric_keys']]
    by_name = {v: k for k, v in METRIC_KEYS.items()}
    for i in range(N):
        b = (z[f'batch/{i}/obs'], z[f'batch/{i}/action'], z[f'batch/{i}/reward'], z[f'batch/{i}/discount'], z[f'batch/{i}/next_obs'], None)
        for e, r in zip(ranks, rows):
            _set(e, b, r)
        so, sn = next(shifts), next(shifts)
        nc, na = noise.draw((B, A)), noise.draw((B, A))
        _phases(ranks, rows, so, sn, nc, na, False)
        raw = sum(e.metrics_raw() for e in ranks)           # partial means add up to the global means
        m = {k: float(raw[by_name[k]]) for k in keys if k != 'actor_ent'}
        m['actor_ent'] = float(np.float32(0.5 + 0.5 * np.log(2 * np.pi) + np.log(STDDEV)) * A)
        np.testing.assert_allclose(np.array([m[k] for k in keys]), z['metrics'][i], rtol=1e-4, atol=3e-6, err_msg=f'step {i} {keys}')
    _assert_states_equal(_state(ranks[0]), _state(ranks[1]), 'replicas')
    names = (('encoder', 0, [k for k, _ in esh]), ('actor', 1, [k for k, _ in ash]), ('critic', 2, [k for k, _ in csh]),
             ('critic_target', 3, [k for k, _ in csh]))
    for nm, net, ks in names:
        for idx, k in enumerate(ks):
            v = ranks[0].tensor(net, idx, L.T_PARAM).cpu().numpy()
            if f'final/{nm}/{k}' in z.files:
                want = z[f'final/{nm}/{k}']
                np.testing.assert_allclose(v.reshape(want.shape), want, rtol=1e-4, atol=2e-6, err_msg=f'{nm}.{k}')
            else:
                np.testing.assert_allclose(v.reshape(-1)[::997], z[f'final_sample/{nm}/{k}'], rtol=1e-4, atol=2e-6, err_msg=f'{nm}.{k}')


# ---------------------------------------------------------------------------------------------------- 3. virtual ranks at config-4 size
def _virtual_vs_single(C_, HW, A, F, H, B, R, precision, M=0, S=0, kept=False, steps=2, check_params=True):
    Br = B // R
    single = _engine(C_, HW, A, F, H, B, precision=precision, meta_dim=M, sf_dim=S)
    ranks = [_engine(C_, HW, A, F, H, Br, ws=R, precision=precision, meta_dim=M, sf_dim=S) for _ in range(R)]
    init = _state(single)
    rows = [slice(r * Br, (r + 1) * Br) for r in range(R)]
    rs = np.random.RandomState(7)
    for step in range(steps):
        b = _batch(200 + step, B, C_, HW, A, M)
        if S:                                 # APS: the task rows are unit vectors (aps.py:236-238)
            t = rs.standard_normal((B, M)).astype(np.float32)
            b = b[:5] + (t / np.linalg.norm(t, axis=1, keepdims=True),)
        so, sn = _shifts(rs, B), _shifts(rs, B)
        nc, na = rs.standard_normal((B, A)).astype(np.float32), rs.standard_normal((B, A)).astype(np.float32)
        _set(single, b)
        for e, r in zip(ranks, rows):
            _set(e, b, r)
        if kept:
            _encode_kept(single, so, sn)
            single.update(STDDEV, noise_critic=nc, noise_actor=na, keep_encoded=True)
        else:
            single.update(STDDEV, so, sn, nc, na)
        _phases(ranks, rows, so, sn, nc, na, kept)
        want, got = single.metrics_raw(), sum(e.metrics_raw() for e in ranks)
        for idx in range(7):
            assert abs(got[idx] - want[idx]) <= 1e-4 * abs(want[idx]) + 1e-6, (precision, R, step, idx, got[idx], want[idx])
    st = [_state(e) for e in ranks]
    for s in st[1:]:
        _assert_states_equal(st[0], s, f'replicas R={R} {precision}')
    if check_params:
        want = _state(single)
        for k in ('0/0', '1/0', '2/0', '3/0'):
            d = np.abs(st[0][k] - want[k])
            moved = np.abs(want[k] - init[k])
            # summation order only: Adam turns rounding-level gradient differences into at most ~lr per step on elements whose gradient
            # is itself at rounding level; everything else agrees to float precision
            assert d.max() <= 2 * steps * 1e-4, (k, d.max())
            assert np.mean(d > 1e-6 + 1e-3 * moved) <= 1e-3, (k, np.mean(d > 1e-6 + 1e-3 * moved))


@pytest.mark.parametrize('precision', ['fp32', 'bf16x6'])
@pytest.mark.parametrize('R', [2, 4])
def test_config4_virtual_ranks_equal_one_engine(R, precision):
    """Config 4's shapes (3x84x84, A=9, F=50, H=1024), global batch 1024 as R x 1024/R: the persistent convolution form at 512 and 256 images."""
    _virtual_vs_single(3, 84, 9, 50, 1024, 1024, R, precision, check_params=precision == 'fp32')


@pytest.mark.parametrize('kind', ['aps', 'smm'])
def test_meta_agents_virtual_ranks_equal_one_engine(kind):
    """Fine-tuning shapes of APS (CriticSF heads, sf_dim = meta_dim) and SMM (skill columns) on the kept-encodings path."""
    M, S = (5, 5) if kind == 'aps' else (4, 0)
    _virtual_vs_single(3, 84, 6, 50, 256, 128, 2, 'fp32', M=M, S=S, kept=True)


# ---------------------------------------------------------------------------------------------------- 4. one-rank library communicator
@pytest.mark.parametrize('precision', ['fp32', 'bf16x6'])
def test_native_comm_single_rank_equals_the_phases(precision):
    """A 1-rank RCCL communicator makes every all-reduce an identity: the library-driven step (critic gradients reduced on the side stream
    while the encoder's backward pass runs, then the encoder's, then the actor's) must equal the hand-driven phases bit for bit."""
    from exorl_amd.comm import Comm
    comm = Comm(0, 1, Comm.unique_id())
    C_, HW, A, F, H, B = 3, 84, 6, 50, 256, 128
    native, hand = (_engine(C_, HW, A, F, H, B, precision=precision) for _ in range(2))
    native.set_comm(comm)
    for step in range(3):
        b = _batch(300 + step, B, C_, HW, A)
        for e in (native, hand):
            _set(e, b)
        native.update(STDDEV)
        for ph in range(3):
            hand.update_phase(ph, STDDEV)
        assert np.array_equal(native.metrics_raw(), hand.metrics_raw()), step
    torch.cuda.synchronize()
    _assert_states_equal(_state(native), _state(hand), precision)
    native.set_comm(None)
    del comm


# ---------------------------------------------------------------------------------------------------- 5. the product path in two processes
@pytest.fixture(scope='module')
def pixel_dp_run():
    """Two fresh rank processes (tests/_pixel_dp_worker.py) on cuda:0 over gloo; one wait with a hard limit, no retry."""
    tmp = Path(tempfile.mkdtemp(prefix='exorl_pixel_dp_'))
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        log = tmp / f'rank{rank}.log'
        procs.append((subprocess.Popen([sys.executable, str(ROOT / 'tests' / '_pixel_dp_worker.py'), str(tmp)], env=env,
                                       stdout=open(log, 'w'), stderr=subprocess.STDOUT), log))
    try:
        for p, log in procs:
            try:
                rc = p.wait(timeout=600)
            except subprocess.TimeoutExpired:
                pytest.fail(f'pixel data-parallel rank timed out:\n{open(log).read()[-3000:]}')
            assert rc == 0, open(log).read()[-3000:]
    finally:
        for p, _ in procs:
            if p.poll() is None:
                p.kill()
                p.wait(timeout=30)
    return tmp


@pytest.mark.parametrize('kind', ['ddpg', 'diayn'])
def test_two_process_pixel_dp_equals_single_process(pixel_dp_run, kind):
    import _pixel_dp_worker as W
    out = pixel_dp_run
    r0, r1 = np.load(out / f'{kind}_rank0.npz'), np.load(out / f'{kind}_rank1.npz')
    for k in r0.files:
        assert np.array_equal(r0[k], r1[k]), (kind, k)              # replicas stay bit-identical
    m0, m1 = (json.load(open(out / f'metrics_{kind}_rank{r}.json')) for r in (0, 1))
    assert m0 == m1 and len(m0) == W.STEPS                          # every rank reports the global means
    ag = W.build(kind, W.B_GLOBAL)
    W.hooks(ag, slice(None))
    init = {n: W.flat(v) for n, v in W.views(ag)}
    for step in range(W.STEPS):
        m = ag.update(iter([W.batch(kind, step)]), step)
        assert m.keys() == m0[step].keys()
        for k, v in m.items():
            assert abs(m0[step][k] - v) <= 1e-4 * abs(v) + 1e-6, (kind, step, k, m0[step][k], v)
    for n, v in W.views(ag):
        want, got = W.flat(v), r0[n]
        d, moved = np.abs(got - want), np.abs(want - init[n])
        assert d.max() <= 2 * W.STEPS * 1e-4, (kind, n, d.max())
        assert np.mean(d > 1e-6 + 1e-3 * moved) <= 1e-3, (kind, n)


def test_two_process_ranks_draw_different_shifts_and_noise(pixel_dp_run):
    """Without hooks each rank's device Philox streams differ (the rank is folded into the seed): different shifts of identical frames,
    different TruncatedNormal noise."""
    a, b = (np.load(pixel_dp_run / f'unhooked_rank{r}.npz') for r in (0, 1))
    assert int(a['seed']) != int(b['seed'])
    assert not np.array_equal(a['feat'], b['feat'])
    assert not np.array_equal(a['noise'], b['noise'])
    assert abs(float(np.corrcoef(a['noise'].reshape(-1), b['noise'].reshape(-1))[0, 1])) < 0.2


def test_two_process_reward_free_module_agent_still_refuses(pixel_dp_run):
    msgs = [json.load(open(pixel_dp_run / f'refusal_rank{r}.json')) for r in (0, 1)]
    for m in msgs:
        assert m['type'] == 'NotImplementedError' and 'reward_free=False' in m['msg'], m
