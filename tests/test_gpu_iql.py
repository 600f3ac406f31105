"""IQLAgent on the GPU: the row kernel on crafted rows against float64, one step of every case of tests/_iql_cases.py against the float64
twin at the bars of tests/test_gpu_grad_grid.py, a five-step trajectory, graph = eager and poisoned scratch bit for bit, pickling and
snapshots, the temperature = 0 step against BCAgent, act() against TD3BCAgent, and the refusals that need a handle."""
import ctypes
import pickle

import numpy as np
import pytest
import torch

import _grad_grid as G
import _iql_cases as I
import _synth

pytestmark = pytest.mark.gpu

NETS = ('actor', 'critic', 'critic_target', 'value')


make, load = I.make_agent, I.load_params


def state_of(ag):
    out = {}
    for nm in NETS:
        net = getattr(ag, nm)
        for i, p in enumerate(net.parameters()):
            out[f'{nm}.param{i}'] = p.detach().clone()
        if nm != 'critic_target':
            for i, g in enumerate(net.grads()):
                out[f'{nm}.grad{i}'] = g.detach().clone()
    out['metrics'] = torch.from_numpy(ag.engine.metrics_raw())
    return out


def assert_same_bits(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        assert not bool(torch.isnan(b[k]).any()), f'{tag}: NaN in {k}'
        assert torch.equal(a[k], b[k]), f'{tag}: {k} differs (max |d| = {float((a[k] - b[k]).abs().max()):.3e})'


# ---- 4. the row kernel ------------------------------------------------------------------------------------------------------------
CHUNK, MAX_WG = 256, 32      # kernels.h: IQL_CHUNK_ROWS, IQL_MAX_WG


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def _chunk_ordered_sums(part, parts):
    """The sums kernel's order on the host: one float32 accumulator per quantity over the per-chunk partials, first chunk first (up to 1024
    chunks chunk_sum adds them one by one)."""
    part = part.reshape(-1, parts)
    assert len(part) <= 1024
    acc = np.zeros(parts, np.float32)
    for row in part:
        acc = (acc + row).astype(np.float32)
    return acc


@pytest.mark.parametrize('rows', [1, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK * MAX_WG + 1, CHUNK * MAX_WG + CHUNK + 37])
def test_row_kernel_vs_float64(rows):
    """exorl_iql_rows on random rows in (-0.5, 0.5) with temperature 0.5 (|temperature u| <= 0.5) and three crafted ones:
      row 0   v = min(tq) exactly: u = 0, dv = 0 and w = 1 (u = 0 takes the `expectile` branch; with u = 0 both branches give dv = 0)
      row 1   u = 200: temperature u = 100 > 88.8 overflows expf, w = max_weight exactly
      row 2   D = 0: y = r
    dv, dq and w each to 4 ulp of fp32 of its own float64 value. Count of roundings: dv 4 (u, k, k u, inv_bg); dq 2 (the kernel forms
    Q - (r + D v') in double and rounds once, since the difference cancels where Q is close to y, then inv_bg); w 1 (temperature u, worth
    |x| 2^-23 relative = at most one ulp at |x| <= 0.5) plus expf's 1 to 2 ulp. Row 3 has Q_1 within 1e-6 of y: dq there is held to its own
    ulp like every other row. The ten sums: bitwise equal on a second run, equal to the float32 sum of the per-chunk partials in chunk order
    (8193 rows: 33 chunks on 32 workgroups, so the first workgroup's second chunk is the last partial), and within 1e-5 of sum |term| of the
    float64 sums."""
    from exorl_amd import _lib as L
    lib = L.load()
    rs = np.random.RandomState(rows)
    f = lambda *s: rs.uniform(-0.5, 0.5, s).astype(np.float32)
    tq, q, v, vn, r = f(2, rows), f(2, rows), f(rows), f(rows), f(rows)
    D = rs.uniform(0.9, 0.99, rows).astype(np.float32)
    v[0] = min(tq[0, 0], tq[1, 0])
    if rows > 2:
        tq[:, 1], v[1] = 120.0, -80.0
        D[2] = 0.0
    if rows > 3:
        q[0, 3] = np.float32(np.float64(r[3]) + np.float64(D[3]) * np.float64(vn[3])) + np.float32(1e-6)
    e, t, mw = np.float32(0.7), np.float32(0.5), np.float32(100.0)
    inv_bg = np.float32(1.0 / rows)
    dev = lambda x: torch.from_numpy(x).cuda()
    d = [dev(x) for x in (tq, q, v, vn, r, D)]
    chunks = lib.exorl_iql_rows_chunks(rows)
    assert chunks == -(-rows // CHUNK)
    outs = []
    for _ in range(2):
        dv, dq, w = (torch.full((n,), float('nan'), device='cuda') for n in (rows, 2 * rows, rows))
        part, sums = torch.full((chunks * 10,), float('nan'), device='cuda'), torch.full((10,), float('nan'), device='cuda')
        L.check(lib.exorl_iql_rows(*[x.data_ptr() for x in d], rows, inv_bg, e, t, mw, dv.data_ptr(), dq.data_ptr(), w.data_ptr(),
                                   part.data_ptr(), sums.data_ptr(), None))
        torch.cuda.synchronize()
        outs.append([x.cpu().numpy() for x in (dv, dq, w, sums, part)])
    dv, dq, w, sums, part = outs[0]
    assert sums.tobytes() == _chunk_ordered_sums(part, 10).tobytes(), 'the sums are not the chunk-ordered float32 sums of the partials'
    assert sums.tobytes() == outs[1][3].tobytes(), 'the sums differ between two runs'
    for a, b in zip(outs[0][:3], outs[1][:3]):
        assert a.tobytes() == b.tobytes()
    x = lambda a: a.astype(np.float64)
    u = np.minimum(x(tq)[0], x(tq)[1]) - x(v)
    k = np.where(u < 0, 1.0 - float(e), float(e))
    dv64 = -2.0 * k * u * float(inv_bg)
    y = x(r) + x(D) * x(vn)
    dq64 = 2.0 * (x(q) - y[None]) * float(inv_bg)
    with np.errstate(over='ignore'):
        w64 = np.minimum(np.exp(float(t) * u), float(mw))
    worst = lambda got, want, ulp: float(np.max(np.abs(x(got) - want) / ulp))
    e_dv, e_w = worst(dv, dv64, _ulp(dv64)), worst(w, w64, _ulp(w64))
    e_dq = worst(dq.reshape(2, rows), dq64, _ulp(dq64))
    print(f'[iql rows] rows={rows}: dv {e_dv:.2f} ulp, dq {e_dq:.2f} ulp, w {e_w:.2f} ulp (bar 4)')
    assert dv[0] == 0.0 and w[0] == 1.0
    if rows > 2:
        assert w[1] == mw and dq[2] == np.float32(2.0) * (q[0, 2] - r[2]) * inv_bg
    assert e_dv <= 4.0 and e_dq <= 4.0 and e_w <= 4.0, (e_dv, e_dq, e_w)
    terms = [x(r), y, x(q)[0], x(q)[1], (x(q)[0] - y) ** 2, (x(q)[1] - y) ** 2, k * u * u, x(v), u, w64]
    for i, tm in enumerate(terms):
        assert abs(float(sums[i]) - tm.sum()) <= 1e-5 * np.abs(tm).sum() + 1e-30, (i, float(sums[i]), tm.sum())


# ---- 5. one step against the float64 twin ---------------------------------------------------------------------------------------------
def run(c, poison=False, use_tb=True):
    torch.manual_seed(0)
    ag = load(make(c, use_tb), c)
    if poison:
        ag.engine.poison_scratch()
    m = ag.update(iter([I.batch(c)]), 0)
    torch.cuda.synchronize()
    return ag, m


@pytest.mark.parametrize('c', [pytest.param(c, id=I.case_id(c)) for c in I.CASES])
def test_gradients_vs_twin64(c):
    """test_gpu_grad_grid's bars per gradient tensor, e(x) = max|x - g64| / max|g64| after the ReLU flips the near-kink set allows:
    fp32 e(gpu) <= 8 max(e(twin32), 2^-23); bf16x3 8 e(twin32) + 4 * 2^-16; bf16x6 (test_gpu_state_bf16x6) 8 max(e(twin32), 2^-23) + 4 * 3 * 2^-24;
    plain bf16 cosine >= 0.999. Metrics: fp32 / bf16x6 2e-5 relative + 1e-6, bf16x3 1e-4, bf16 3e-2. All three nets' forwards read the
    parameters from before the step, so the twins need no hand-over of stepped parameters. The same step on NaN-filled scratch: same bits."""
    ag, m = run(c)
    r64, r32 = I.twin_pair(c)
    tag = I.case_id(c)
    prec = c.precision
    rel = {'fp32': 2e-5, 'bf16x6': 2e-5, 'bf16x3': 1e-4, 'bf16': 3e-2}[prec]
    assert sorted(m) == sorted(r64.metrics), (sorted(m), sorted(r64.metrics))
    worst_m = max(abs(m[k] - v) / (abs(v) + 1e-6 / rel) for k, v in r64.metrics.items())
    ratio_w = e_gpu_w = e_32_w = 0.0
    cos_w, worst_at, flips = 1.0, '', 0
    floor = G.KINK_FLOOR['bf16x3' if prec == 'bf16x3' else 'fp32']
    for step, want in I.steps_of(r64):
        got = [g.cpu().numpy().reshape(w.shape) for g, w in zip(getattr(ag, step).grads(), want)]
        assert len(got) == len(want) and all(np.all(np.isfinite(g)) for g in got), f'{tag}: {step} gradients'
        if c.bar == 'coarse':
            for i, (g, w) in enumerate(zip(got, want)):
                cos = G.tensor_cosines([g], [w])[0]
                cos_w = min(cos_w, cos)
                e_gpu_w = max(e_gpu_w, float(np.abs(g - w).max() / np.abs(w).max()))
                assert cos >= 0.999, (tag, step, i, cos)
            continue
        kinks = r64.kinks[step]
        d_gpu, f_gpu = G.explain_kinks(got, want, kinks, floor, f'{tag} {step} gpu')
        d_32, _ = G.explain_kinks(getattr(r32, f'{step}_grads'), want, kinks, floor, f'{tag} {step} twin32')
        flips += f_gpu
        for i, (eg, e3) in enumerate(zip(G.tensor_errors(d_gpu, want), G.tensor_errors(d_32, want))):
            bar = {'fp32': 8.0 * max(e3, 2.0 ** -23), 'bf16x6': 8.0 * max(e3, 2.0 ** -23) + 12.0 * 2.0 ** -24, 'bf16x3': 8.0 * e3 + 4.0 * 2.0 ** -16}[prec]
            if eg / bar > ratio_w:
                ratio_w, worst_at = eg / bar, f'{step}[{i}]'
            e_gpu_w, e_32_w = max(e_gpu_w, eg), max(e_32_w, e3)
    K = ' '.join(f'|K_{s}|={n}' for s, n in r64.n_kinks.items())
    if c.bar == 'coarse':
        print(f'[iql grid] {tag}: coarse e(gpu) {e_gpu_w:.2e} worst cosine {cos_w:.6f} (bar 0.999); worst metric error {worst_m:.2e} (bar {rel:g})')
    else:
        print(f'[iql grid] {tag}: tight e(gpu) {e_gpu_w:.2e} e(twin32) {e_32_w:.2e} worst e(gpu)/bar {ratio_w:.3f} at {worst_at or "-"} {K} '
              f'flips gpu {flips}; worst metric error {worst_m:.2e} (bar {rel:g})')
    for k, v in r64.metrics.items():
        assert abs(m[k] - v) <= rel * abs(v) + 1e-6 * (3e4 if prec == 'bf16' else 1), (tag, k, m[k], v)
    assert ratio_w <= 1.0, f'{tag}: e(gpu) is {ratio_w:.2f} x its bar at {worst_at} (e(gpu) {e_gpu_w:.2e}, e(twin32) {e_32_w:.2e})'
    dirty, m1 = run(c, poison=True)
    assert_same_bits(state_of(ag), state_of(dirty), f'{tag} poisoned')
    assert m == m1


# ---- 6. five steps -------------------------------------------------------------------------------------------------------------------
TRAJ, traj_bar = I.TRAJ, I.traj_bar


def test_five_steps_vs_twin64():
    ag = load(make(TRAJ), TRAJ)
    tw = I.make_twin(TRAJ, torch.float64)
    for step in range(5):
        b = _synth.synth_batch(TRAJ.seed + 2, step, TRAJ.B, TRAJ.O, TRAJ.A)
        m = ag.update(iter([b]), step)
        r = tw.update(b)
        assert sorted(m) == sorted(r.metrics)
        for k, v in r.metrics.items():
            assert abs(m[k] - v) <= 2e-5 * abs(v) + 1e-6, (step, k, m[k], v)
        for nm in NETS:
            for i, (p, q) in enumerate(zip(getattr(ag, nm).parameters(), getattr(tw, nm))):
                q = q.detach().numpy()
                err = float(np.abs(p.cpu().numpy().reshape(q.shape) - q).max())
                assert err <= traj_bar(q, step), (step, nm, i, err, traj_bar(q, step))
    assert ag.engine.opt_steps() == (5, 5)


# ---- 7. graph, poison, counter, pickle, snapshot -------------------------------------------------------------------------------------------
SHAPE = I.Case(24, 6, 128, 64, 'fp32', 0, 'tight', I.DEFAULT, False, '')


def _arena(seed, B=64):
    from exorl_amd.engine import ReplayEngine
    from exorl_amd.replay_buffer import ArenaIterator
    eng = ReplayEngine((24,), np.float32, 6, 0, 4096, 64)
    eng.set_order([eng.append_episode(ep) for ep in _synth.synth_episodes(seed, [200, 300, 250], 24, 6)])
    eng.seed_philox(77)
    return eng, ArenaIterator(eng, B, 1, 0.99, 'philox')


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
def test_graph_equals_eager_and_poisoned_scratch(precision):
    """Three agents from one seed over three equal arenas, four steps: a captured graph, eager launches, and eager launches with the scratch
    refilled with NaN before every step. Parameters, gradients, targets and metrics bit for bit; update() leaves the noise counter alone."""
    c = SHAPE._replace(precision=precision)
    runs = []
    for mode in ('graph', 'eager', 'poison'):
        torch.manual_seed(3)
        ag = make(c)
        keep = _arena(9)
        if mode == 'graph':
            assert ag.enable_graph(keep[1])
        n0 = ag.engine.noise_counter()
        ms = []
        for s in range(4):
            if mode == 'poison':
                ag.engine.poison_scratch()
            ms.append(ag.update(keep[1], s))
        torch.cuda.synchronize()
        assert ag.engine.noise_counter() == n0, mode
        runs.append((ag, ms, keep))
    for ag, ms, _ in runs[1:]:
        assert ms == runs[0][1]
        assert_same_bits(state_of(runs[0][0]), state_of(ag), precision)
    assert runs[0][0].engine.opt_steps() == runs[1][0].engine.opt_steps() == (4, 4)
    from exorl_amd import _lib as L
    with pytest.raises(L.ExorlError, match='captured graph'):
        runs[0][0].engine.set_iql(0.7, 3.0, 100.0)


def test_pickle_and_snapshot_round_trip():
    from exorl_amd import snapshot
    c = SHAPE._replace(hyper=(0.8, 2.0, 50.0))
    torch.manual_seed(5)
    a = make(c)
    batches = [_synth.synth_batch(11, s, c.B, c.O, c.A) for s in range(4)]
    for s in range(2):
        a.update(iter([batches[s]]), s)
    b = pickle.loads(pickle.dumps(a))
    assert (b.expectile, b.temperature, b.max_weight) == (0.8, 2.0, 50.0) and b.engine.opt_steps() == (2, 2)
    for s in range(2, 4):
        assert a.update(iter([batches[s]]), s) == b.update(iter([batches[s]]), s)
    assert_same_bits(state_of(a), state_of(b), 'pickle')
    sd = snapshot.state_dicts(a)
    assert list(sd['value']) == I.VALUE_KEYS
    torch.manual_seed(6)
    fresh = make(c)
    snapshot.load_state_dicts(fresh, dict(sd))
    for nm in NETS:
        for p, q in zip(getattr(a, nm).parameters(), getattr(fresh, nm).parameters()):
            assert torch.equal(p, q), nm


# ---- 8. temperature 0 is behaviour cloning; act() is the offline actor's -------------------------------------------------------------------
def test_temperature_zero_actor_gradient_is_bc_bit_for_bit():
    """w = min(expf(0 * u), max_weight) = 1.0f exactly and the weighted path forms -w (a - mu) / std^2 / Bg, a multiplication by exactly 1.0f:
    the actor gradient equals BCAgent's on the same actor, batch and std in every bit (fp32)."""
    from exorl_amd import agents
    c = I.CASES[1]
    ag = load(make(c, temperature=0.0), c)
    bc = agents.BCAgent('bc', (c.O,), (c.A,), 'cuda', 1e-4, c.H, c.B, 0.2, True)
    bc.actor.load_state_dict(ag.actor.state_dict())
    b = I.batch(c)
    m, mb = ag.update(iter([b]), 0), bc.update(iter([b]), 0)
    assert m['actor_weight'] == 1.0 and m['actor_loss'] == mb['actor_loss']
    for i, (g, w) in enumerate(zip(ag.actor.grads(), bc.actor.grads())):
        assert torch.equal(g, w), i
    for p, q in zip(ag.actor.parameters(), bc.actor.parameters()):
        assert torch.equal(p, q)


def test_act_equals_td3bc_act():
    from exorl_amd import agents
    c = I.CASES[1]
    ag = load(make(c), c)
    td = agents.TD3BCAgent('td3_bc', (c.O,), (c.A,), 'cuda', 1e-4, c.H, 0.01, 0.2, 1, c.B, 0.3, True, 2.5)
    td.actor.load_state_dict(ag.actor.state_dict())
    obs = np.random.RandomState(1).standard_normal(c.O).astype(np.float32)
    z = np.random.RandomState(2).standard_normal((1, c.A)).astype(np.float32)
    for a in (ag, td):
        a.num_expl_steps = 0
        a.noise_hook = lambda shape: z
    assert np.array_equal(ag.act(obs, 0, True), td.act(obs, 0, True))
    assert np.array_equal(ag.act(obs, 0, False), td.act(obs, 0, False))
    many = torch.from_numpy(np.random.RandomState(3).standard_normal((70, c.O)).astype(np.float32)).cuda()
    assert torch.equal(ag.engine.act(many, 0.2, True), td.engine.act(many, 0.2, True))


def test_refusals_that_need_a_handle():
    from exorl_amd import _lib as L
    from exorl_amd import agents
    c = I.CASES[0]
    ag = make(c)
    bc = agents.BCAgent('bc', (c.O,), (c.A,), 'cuda', 1e-4, c.H, c.B, 0.2, True)
    with pytest.raises(L.ExorlError, match='not IQL'):
        bc.engine.set_iql(0.7, 3.0, 100.0)
    with pytest.raises(L.ExorlError, match='needs 0 < expectile < 1'):
        ag.engine.set_iql(1.5, 3.0, 100.0)
    with pytest.raises(L.ExorlError):
        ag.engine.update_phase(0, 0.2)              # IQL's phases are 6..9
    with pytest.raises(L.ExorlError):
        bc.engine.update_phase(6, 0.2)
    assert ag.enable_metric_window() is False
    with pytest.raises(NotImplementedError):
        ag.evaluate(iter([I.batch(c)]))
    with pytest.raises(L.ExorlError):
        ag.engine.set_eval()
    assert ctypes.sizeof(L.AgentCfg) == 80
