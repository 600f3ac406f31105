"""ReBRACAgent on the GPU: the row kernel alone against numpy in its stated fp32 order, critic_beta = 0 (and a dataset without valid next
actions) against TD3BCAgent bit for bit, one step of every case of tests/_rebrac_twin.py and a three-step trajectory against the float64
twin, update = per-phase = captured graph bit for bit and on a poisoned buffer, the replay's next-action column as the step sees it,
pickling, snapshots and the refusals."""
import pickle

import numpy as np
import pytest
import torch

import _grad_grid as G
import _rebrac_twin as R
import _synth
from _next_action_rule import next_action_rule

pytestmark = pytest.mark.gpu

NETS = ('actor', 'critic', 'critic_target')


def L():
    from exorl_amd import _lib
    return _lib


def state_of(ag, metrics=True):
    out = {}
    for nm in NETS:
        net = getattr(ag, nm)
        for i, p in enumerate(net.parameters()):
            out[f'{nm}.param{i}'] = p.detach().clone()
    for nm, net in (('actor', L().NET_ACTOR), ('critic', L().NET_CRITIC)):
        for w, tag in ((L().T_GRAD, 'grad'), (L().T_ADAM_M, 'adam_m'), (L().T_ADAM_V, 'adam_v')):
            out[f'{nm}.{tag}'] = ag.engine.flat(net, w).detach().clone()
    if metrics:
        out['metrics'] = torch.from_numpy(ag.engine.metrics_raw())
    return out


def assert_same_bits(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        assert not bool(torch.isnan(b[k]).any()), f'{tag}: NaN in {k}'
        assert torch.equal(a[k], b[k]), f'{tag}: {k} differs (max |d| = {float((a[k] - b[k]).abs().max()):.3e})'


def hooked(ag, blocks):
    it = iter(blocks)
    ag.noise_hook = lambda shape: next(it)
    return ag


def phased(ag):
    """update() through exorl_agent_update_phase 0..3, as under torch.distributed."""
    eng = ag.engine
    eng.run_update = lambda stddev, nc=None, na=None: [eng.update_phase(ph, stddev, nc, na) for ph in range(4)]
    return ag


def poison_buffer(ag):
    """NaN into the ReBRAC buffer's two scratch runs (r~ and the per-chunk sums); next_action / next_valid are inputs and stay."""
    eng = ag.engine
    B, A = eng.batch, eng.act_dim
    pad = lambda n: -(-n // 64) * 64
    f32 = eng._rebrac.view(torch.float32)
    f32[pad(B * A) + pad(B):] = float('nan')


MIXED = (200, 3, 300, 5, 250, 4)         # episodes are drawn uniformly: half of the rows come from the short ones, one in eight ends its episode


def _arena(seed, B, lengths=MIXED, nstep=1, O=24, A=6):
    from exorl_amd.engine import ReplayEngine
    from exorl_amd.replay_buffer import ArenaIterator
    eps = _synth.synth_episodes(seed, list(lengths), O, A)
    eng = ReplayEngine((O,), np.float32, A, 0, sum(lengths) + len(lengths) + 64, len(lengths) + 4)
    eng.set_order([eng.append_episode(ep) for ep in eps])
    eng.seed_philox(77)
    return eng, ArenaIterator(eng, B, nstep, 0.99, 'philox'), eps


# ---- 1. the row kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('valid', ['ones', 'zeros', 'mixed'])
@pytest.mark.parametrize('A', [1, 6, 16])
@pytest.mark.parametrize('rows', [1, 7, 256, 257, 1000])
def test_row_kernel_vs_numpy(rows, A, valid):
    """exorl_rebrac_rows against numpy float32 in the header's order: s over j ascending of the squared fp32 difference, p = v s,
    t = beta p, r~ = r - D t, every operation rounded on its own. r~ bit for bit; the three sums (p, v, r) to 1e-6 relative of float64
    (all terms are >= 0: no cancellation), equal to the chunk-ordered float32 sum of the partials and the same bits on NaN-filled
    outputs. The sample sits at a pitch larger than A, inside rows of 5 + A floats whose other columns are NaN."""
    lib = L().load()
    rs = np.random.RandomState(1000 * rows + 10 * A + len(valid))
    ld = A + 5
    x = np.full((rows, ld), np.nan, np.float32)
    x[:, 5:] = rs.uniform(-1, 1, (rows, A)).astype(np.float32)
    v = {'ones': np.ones(rows), 'zeros': np.zeros(rows), 'mixed': (rs.uniform(size=rows) < 0.6)}[valid].astype(np.float32)
    y = (rs.uniform(-1, 1, (rows, A)) * v[:, None]).astype(np.float32)         # the gather writes zeros into invalid rows
    r = rs.uniform(0, 1, rows).astype(np.float32)
    D = rs.uniform(0.5, 0.99, rows).astype(np.float32)
    if rows > 2:
        D[2] = 0.0
    beta = np.float32(0.7)
    s = np.zeros(rows, np.float32)
    for j in range(A):
        d = (x[:, 5 + j] - y[:, j]).astype(np.float32)
        s = (s + (d * d).astype(np.float32)).astype(np.float32)
    p = (v * s).astype(np.float32)
    t = (beta * p).astype(np.float32)
    want = (r - (D * t).astype(np.float32)).astype(np.float32)
    dev = lambda a: torch.from_numpy(a).cuda()
    xd, yd, vd, rd, Dd = dev(x), dev(y), dev(v), dev(r), dev(D)
    chunks = lib.exorl_iql_rows_chunks(rows)
    outs = []
    for fill in (0.0, float('nan')):
        out, part, sums = (torch.full((n,), fill, device='cuda') for n in (rows, chunks * 3, 3))
        L().check(lib.exorl_rebrac_rows(xd.data_ptr() + 20, ld, yd.data_ptr(), A, vd.data_ptr(), rd.data_ptr(), Dd.data_ptr(), rows, A, beta,
                                        np.float32(1.0 / rows), out.data_ptr(), part.data_ptr(), sums.data_ptr(), None))
        torch.cuda.synchronize()
        outs.append([a.cpu().numpy() for a in (out, part, sums)])
    got, part, sums = outs[0]
    assert got.tobytes() == want.tobytes(), f'r~ differs in {int((got != want).sum())} of {rows} rows'
    for a, b in zip(outs[0], outs[1]):
        assert a.tobytes() == b.tobytes(), 'NaN-filled outputs changed the result: something is read before it is written'
    acc = np.zeros(3, np.float32)
    for row in part.reshape(-1, 3):
        acc = (acc + row).astype(np.float32)
    assert sums.tobytes() == acc.tobytes()
    want64 = np.array([p.astype(np.float64).sum(), v.astype(np.float64).sum(), r.astype(np.float64).sum()])
    assert np.all(np.abs(sums - want64) <= 1e-6 * np.abs(want64)), (sums, want64)
    if valid == 'zeros':
        assert got.tobytes() == r.tobytes() and sums[0] == 0.0 and sums[1] == 0.0
    if rows > 2:
        assert got[2] == r[2]
    # critic_beta = 0: the reward, bit for bit
    out, part, sums = (torch.full((n,), float('nan'), device='cuda') for n in (rows, chunks * 3, 3))
    L().check(lib.exorl_rebrac_rows(xd.data_ptr() + 20, ld, yd.data_ptr(), A, vd.data_ptr(), rd.data_ptr(), Dd.data_ptr(), rows, A, 0.0,
                                    np.float32(1.0 / rows), out.data_ptr(), part.data_ptr(), sums.data_ptr(), None))
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == r.tobytes()


# ---- 2. critic_beta = 0 and a dataset without next actions: TD3BCAgent, bit for bit -----------------------------------------------------
def _pair(precision, use_tb, critic_bc, H=128, B=64):
    from exorl_amd import agents
    torch.manual_seed(1)
    c = R.Case(24, 6, H, B, precision, 0, 'tight', '')
    re = R.make_agent(c, use_tb, critic_bc)
    td = agents.TD3BCAgent('td3_bc', (24,), (6,), 'cuda', 1e-4, H, 0.01, 0.2, 1, B, 0.3, use_tb, R.alpha_of(6), precision=precision)
    for nm in NETS:
        getattr(td, nm).load_state_dict(getattr(re, nm).state_dict())
    return re, td


@pytest.mark.parametrize('mode', ['eager', 'phased', 'graph'])
@pytest.mark.parametrize('precision', ['fp32', 'bf16x3', 'bf16x6', 'bf16'])
@pytest.mark.parametrize('dataset', ['beta0', 'length1'])
def test_without_a_penalty_the_step_is_td3bcs(dataset, precision, mode):
    """Three steps of a ReBRACAgent and a TD3BCAgent of one seed over equal arenas (device sampler, device noise): parameters, gradients,
    Adam moments, the target, the counters and TD3+BC's ten metric slots bit for bit. beta0: critic_bc_coef = 0 on ordinary episodes (valid
    and invalid rows mixed). length1: critic_bc_coef = 5 on episodes of length 1 at nstep = 1, where every sample ends its episode: v = 0
    on every row. eager and phased report metrics (the unfused kernels), graph runs the fused path bench.py times."""
    use_tb = mode != 'graph'
    re, td = _pair(precision, use_tb, 0.0 if dataset == 'beta0' else 5.0)
    lengths = MIXED if dataset == 'beta0' else (1,) * 96
    keeps = [_arena(9, 64, lengths), _arena(9, 64, lengths)]
    for ag, keep in zip((re, td), keeps):
        if mode == 'phased':
            phased(ag)
        if mode == 'graph':
            assert ag.enable_graph(keep[1])
    for s in range(3):
        mr, mt = re.update(keeps[0][1], s), td.update(keeps[1][1], s)
        assert {k: v for k, v in mr.items() if k not in ('critic_penalty', 'next_valid')} == mt
        if use_tb and dataset == 'length1':
            assert mr['critic_penalty'] == 0.0 and mr['next_valid'] == 0.0
        if use_tb and dataset == 'beta0':
            assert mr['critic_penalty'] > 0.0 and 0.0 < mr['next_valid'] < 1.0
    torch.cuda.synchronize()
    assert_same_bits(state_of(td, metrics=False), state_of(re, metrics=False), f'{dataset} {precision} {mode}')
    assert re.engine.opt_steps() == td.engine.opt_steps() == (3, 3) and re.engine.noise_counter() == td.engine.noise_counter()
    if use_tb:
        assert re.engine.metrics_raw()[:10].tobytes() == td.engine.metrics_raw()[:10].tobytes()


# ---- 3. against the float64 twin ------------------------------------------------------------------------------------------------------
def run(c, route, poison=False):
    torch.manual_seed(0)
    ag = R.load_params(R.make_agent(c, route != 'fast'), c)
    if route == 'phased':
        phased(ag)
    hooked(ag, R.noise(c))
    if poison:
        ag.engine.poison_scratch()
        poison_buffer(ag)
    m = ag.update(iter([R.batch(c)]), 0)
    torch.cuda.synchronize()
    return ag, m


@pytest.mark.parametrize('route', ['metrics', 'fast', 'phased'])
@pytest.mark.parametrize('c', [pytest.param(c, id=R.case_id(c)) for c in R.CASES])
def test_gradients_vs_twin64(c, route):
    """critic_bc_coef = 1, fixed noise. The bars of tests/test_gpu_grad_grid.py (and tests/test_gpu_prdc.py for bf16x6) per gradient
    tensor, e(x) = max|x - g64| / max|g64| after the ReLU flips the near-kink set allows: fp32 e(gpu) <= 8 max(e(twin32), 2^-23); bf16x3
    8 e(twin32) + 4 * 2^-16; bf16x6 8 max(e(twin32), 2^-23) + 4 * 3 * 2^-24; plain bf16 cosine >= 0.999. Metrics (critic_penalty, next_valid,
    the penalised critic_target_q and the dataset's batch_reward among them): fp32 / bf16x6 2e-5 relative + 1e-6, bf16x3 1e-4, bf16 3e-2.
    Both twins take their actor step from the critic this run's optimiser step produced. The new term adds one fp32 row operation in
    front of the same kernels: no bar is widened for it. The same step on NaN-filled scratch and a NaN-filled r~: same bits."""
    ag, m = run(c, route)
    after = [p.cpu().numpy() for p in ag.critic.parameters()]
    r64 = R.run_twin(c, torch.float64, None if c.bar == 'coarse' else R.KINK_DELTA[c.precision], critic_after=after)
    r32 = R.run_twin(c, torch.float32, critic_after=after)
    tag = f'{R.case_id(c)} {route}'
    prec = c.precision
    rel = {'fp32': 2e-5, 'bf16x6': 2e-5, 'bf16x3': 1e-4, 'bf16': 3e-2}[prec]
    worst_m = 0.0
    if route != 'fast':
        assert sorted(m) == sorted(r64.metrics), (sorted(m), sorted(r64.metrics))
        worst_m = max(abs(m[k] - v) / (abs(v) + 1e-6 / rel) for k, v in r64.metrics.items())
        b = R.batch(c)
        assert abs(m['batch_reward'] - float(b[2].astype(np.float64).mean())) <= 2e-6        # the dataset's r, never r~
        assert abs(m['next_valid'] - float(b[6].mean())) <= 1e-6
    else:
        assert m == {}
    ratio_w = e_gpu_w = e_32_w = 0.0
    cos_w, worst_at, flips = 1.0, '', 0
    floor = G.KINK_FLOOR['bf16x3' if prec == 'bf16x3' else 'fp32']
    for step, want in R.steps_of(r64):
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
        assert kinks is not None, f'{tag}: |K| = {r64.n_kinks[step]} exceeds the cap of a tight case'
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
        print(f'[rebrac grid] {tag}: coarse e(gpu) {e_gpu_w:.2e} worst cosine {cos_w:.6f} (bar 0.999); worst metric error {worst_m:.2e} (bar {rel:g})')
    else:
        print(f'[rebrac grid] {tag}: tight e(gpu) {e_gpu_w:.2e} e(twin32) {e_32_w:.2e} worst e(gpu)/bar {ratio_w:.3f} at {worst_at or "-"} {K} '
              f'flips gpu {flips}; worst metric error {worst_m:.2e} (bar {rel:g})')
    if route != 'fast':
        for k, v in r64.metrics.items():
            assert abs(m[k] - v) <= rel * abs(v) + 1e-6 * (3e4 if prec == 'bf16' else 1), (tag, k, m[k], v)
    assert ratio_w <= 1.0, f'{tag}: e(gpu) is {ratio_w:.2f} x its bar at {worst_at} (e(gpu) {e_gpu_w:.2e}, e(twin32) {e_32_w:.2e})'
    dirty, m1 = run(c, route, poison=True)
    assert_same_bits(state_of(ag), state_of(dirty), f'{tag} poisoned')
    assert m == m1


@pytest.mark.parametrize('c', [pytest.param(c, id=R.case_id(c)) for c in R.TRAJ_CASES])
def test_three_steps_vs_twin64(c):
    """Parameters after each of three steps against the float64 twin, both shapes at fp32, bf16x6 and bf16x3 and plain bf16 at its own;
    the bars and where each comes from are in tests/_rebrac_twin.py (TRAJ_CASES): fp32-grade element by element within max(traj_bar, twice
    the float32 CPU twin's recorded error), bf16x3 per net by tests/test_gpu_dp.py's three-step rule, plain bf16 by the direction of the
    parameter change within twice the loss the number format alone causes (the bf16-operand CPU twin; measured on the GPU: the engine's
    cosines equal that twin's to three digits, 0.985905 against 0.986026 on the actor after the first step). The metrics of every step at the precision's one-step tolerance. Every figure is printed before anything is asserted."""
    prec = c.precision
    ag = R.load_params(R.make_agent(c), c)
    tw = R.make_twin(c, torch.float64)
    start = {nm: [p.detach().double().cpu().numpy().copy() for p in getattr(ag, nm).parameters()] for nm in NETS}
    ns = _synth.NoiseStream(c.seed + 3)
    rel = R.TRAJ_METRIC_REL[prec]
    flat = lambda ts: np.concatenate([np.asarray(t, np.float64).reshape(-1) for t in ts])
    bad, worst, worst_m = [], 0.0, 0.0
    for step in range(R.TRAJ_STEPS):
        b, z = R.batch(c, step), R.noise(c, ns)
        m = hooked(ag, z).update(iter([b]), step)
        r = tw.update(b, step, *z)
        assert sorted(m) == sorted(r.metrics)
        for k, v in r.metrics.items():
            tol = rel * abs(v) + 1e-6 * (3e4 if prec == 'bf16' else 1)
            worst_m = max(worst_m, abs(m[k] - v) / tol)
            if abs(m[k] - v) > tol:
                bad.append(f'step {step} metric {k}: {m[k]!r} against {v!r}')
        for nm in NETS:
            got = [p.detach().double().cpu().numpy().reshape(q.shape) for p, q in zip(getattr(ag, nm).parameters(), getattr(tw, nm))]
            want = [q.detach().numpy() for q in getattr(tw, nm)]
            if prec in ('fp32', 'bf16x6'):
                e32 = R.TRAJ_E32[(c.O, c.A, c.H, c.B)][step]
                for i, (g, w) in enumerate(zip(got, want)):
                    bar = max(R.traj_bar(w, step), 2.0 * e32)
                    err = float(np.abs(g - w).max())
                    worst = max(worst, err / bar)
                    if err > bar:
                        bad.append(f'step {step} {nm}[{i}]: error {err:.3e} over the bar {bar:.3e}')
                continue
            g, w = flat(got), flat(want)
            d = np.abs(g - w)
            ceiling = R.DP_RULE['ceiling'] * (step + 1) / R.TRAJ_STEPS          # 2 lr a step, and the rule's 5e-5 of slack shared out
            share = float(np.mean(d > R.DP_RULE['abs'] + R.DP_RULE['rel'] * np.abs(w)))
            dg, dw = g - flat(start[nm]), w - flat(start[nm])
            cos = float(dg @ dw / (np.linalg.norm(dg) * np.linalg.norm(dw)))
            print(f'[rebrac traj] {R.case_id(c)} step {step} {nm}: max |d| {d.max():.2e} (ceiling {ceiling:.2e}), share outside 2e-6 + 1e-4 |p| '
                  f'{share:.2e}, cosine of the change {cos:.6f}')
            if d.max() > ceiling:
                bad.append(f'step {step} {nm}: max |d| {d.max():.3e} over {ceiling:.3e}')
            if prec == 'bf16x3' and share > R.DP_RULE['share']:
                bad.append(f'step {step} {nm}: {share:.3e} of the elements outside the rule')
            if prec == 'bf16':          # twice what the number format alone costs the direction (the bf16-operand CPU twin, recorded)
                floor = 1.0 - 2.0 * (1.0 - R.TRAJ_BF16_COS[step][NETS.index(nm)])
                if cos < floor:
                    bad.append(f'step {step} {nm}: cosine {cos:.6f} under {floor:.6f}')
    print(f'[rebrac traj] {R.case_id(c)}: worst element error / bar {worst:.3f}, worst metric error / tolerance {worst_m:.3f}')
    assert not bad, bad
    assert ag.engine.opt_steps() == (3, 3)


# ---- 4. update = per-phase = captured graph; the poisoned buffer; the refusals -----------------------------------------------------------
@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
def test_update_phases_and_graph_agree_bit_for_bit(precision):
    """critic_bc_coef = 1. Four agents of one seed over four equal arenas, three steps, use_tb=True (every driver then runs the same
    kernels: the unfused heads and critic_loss): exorl_agent_update, the four phases one by one, the captured graph, and exorl_agent_update
    with the workspace's scratch and the buffer's r~ and sums refilled with NaN before every step. Parameters, gradients, Adam moments,
    targets and metrics bit for bit. Then use_tb=False, the fused path: graph = eager = eager on poisoned scratch."""
    c = R.Case(24, 6, 128, 64, precision, 0, 'tight', '')
    for use_tb, modes in ((True, ('eager', 'phased', 'graph', 'poison')), (False, ('eager', 'graph', 'poison'))):
        runs = []
        for mode in modes:
            torch.manual_seed(3)
            ag = R.make_agent(c, use_tb)
            keep = _arena(9, 64)
            if mode == 'phased':
                phased(ag)
            if mode == 'graph':
                assert ag.enable_graph(keep[1])
            ms = []
            for s in range(3):
                if mode == 'poison':
                    ag.engine.poison_scratch()
                    poison_buffer(ag)
                ms.append(ag.update(keep[1], s))
            torch.cuda.synchronize()
            runs.append((ag, keep, ms))
        for (ag, _, ms), mode in zip(runs[1:], modes[1:]):
            assert_same_bits(state_of(runs[0][0], metrics=use_tb), state_of(ag, metrics=use_tb), f'{precision} use_tb={use_tb} {mode}')
            assert ms == runs[0][2], mode
        if use_tb:
            assert all(m['critic_penalty'] > 0 and 0 < m['next_valid'] < 1 for m in runs[0][2])
    g, keep, _ = runs[modes.index('graph')]
    with pytest.raises(L().ExorlError, match='captured graph'):
        g.engine.set_rebrac(g.engine._rebrac, 2.0)
    with pytest.raises(L().ExorlError, match='captured graph'):
        g.engine.set_rebrac(None, 0.0)
    g.update(keep[1], 3)
    torch.cuda.synchronize()
    assert g.engine.opt_steps() == (4, 4)


def test_refusals_and_detaching():
    from exorl_amd import agents
    c = R.CASES[0]
    ag = R.load_params(R.make_agent(c), c)
    eng = ag.engine
    b, z = R.batch(c), R.noise(c)
    assert ag.enable_metric_window() is False
    with pytest.raises(L().ExorlError, match='ReBRAC has no metric window'):
        eng.set_metric_window()
    with pytest.raises(NotImplementedError):
        ag.evaluate(iter([b]))
    with pytest.raises(L().ExorlError, match='ReBRAC has no forward-only evaluation'):
        eng.set_eval()
    with pytest.raises(L().ExorlError, match='ReBRAC has no forward-only evaluation'):
        eng.evaluate()
    buf = eng._rebrac
    for beta in (-1.0, float('nan')):
        with pytest.raises(L().ExorlError, match='critic_beta'):
            eng.set_rebrac(buf, beta)
    with pytest.raises(L().ExorlError, match='need'):
        eng.set_rebrac(buf[:buf.numel() - 256], 1.0)
    with pytest.raises(L().ExorlError, match='256-byte aligned'):
        eng.set_rebrac(torch.zeros(buf.numel() + 64, dtype=torch.uint8, device='cuda')[4:], 1.0)
    td3 = agents.TD3Agent('td3', (c.O,), (c.A,), 'cuda', 1e-4, c.H, 0.01, 0.2, 1, c.B, 0.3, True)
    with pytest.raises(L().ExorlError, match='not TD3\\+BC'):
        td3.engine.set_rebrac(buf, 1.0)
    with pytest.raises(L().ExorlError, match='not TD3\\+BC'):
        td3.engine.rebrac_bytes()
    assert eng.opt_steps() == (0, 0)
    slots = eng.batch_slots()
    assert slots.next_action == buf.data_ptr() and slots.next_action_stride == c.A and slots.next_valid > slots.next_action
    # the refused calls changed nothing: the step is the penalised one
    m1 = hooked(ag, z).update(iter([b]), 0)
    assert m1['critic_penalty'] > 0 and eng.opt_steps() == (1, 1)
    # detached: TD3+BC again. NULL slots; the evaluation and the window attach, and while one is attached ReBRAC is refused
    other = R.load_params(R.make_agent(c), c)
    eng, buf = other.engine, other.engine._rebrac
    eng.set_rebrac(None, float('nan'))          # a detach looks at neither the size nor the coefficient
    slots = eng.batch_slots()
    assert (slots.next_action, slots.next_action_stride, slots.next_valid) == (None, 0, None)
    eng.set_eval()
    eng.set_batch(*b[:5])
    eng.evaluate()
    sums, rows = eng.eval_read()
    assert rows == c.B and np.all(np.isfinite(sums))
    eng.set_metric_window()
    with pytest.raises(L().ExorlError, match='detach the metric window'):
        eng.set_rebrac(buf, 1.0)
    eng.set_metric_window(None)
    with pytest.raises(L().ExorlError, match='detach the eval buffer'):
        eng.set_rebrac(buf, 1.0)
    eng.set_eval(None)
    # attached again: the penalised step, bit for bit the one `ag` took
    eng.set_rebrac(buf, R.CRITIC_BC)
    other._slots = None
    assert hooked(other, z).update(iter([b]), 0) == m1
    torch.cuda.synchronize()
    assert_same_bits(state_of(ag), state_of(other), 'detached and attached again')
    # a detached engine's step is TD3BCAgent's
    td = R.load_params(agents.TD3BCAgent('td3_bc', (c.O,), (c.A,), 'cuda', 1e-4, c.H, 0.01, 0.2, 1, c.B, 0.3, True, R.alpha_of(c.A)), c)
    ref = R.load_params(R.make_agent(c), c)
    ref.engine.set_rebrac(None, 0.0)
    hooked(td, z).update(iter([b[:5]]), 0)
    ref.engine.set_batch(*b[:5])
    ref.engine.run_update(0.2, *z)
    torch.cuda.synchronize()
    assert_same_bits(state_of(td), state_of(ref), 'detached')


# ---- 5. through the replay ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nstep', [1, 3])
def test_slots_hold_the_replays_next_action(nstep):
    """iter-style sampling from a synthetic arena into the agent's slots: what the step read as a' and v equals the numpy rule of
    tests/_next_action_rule.py on the pairs the sampler drew, and the step's next_valid metric is their mean."""
    c = R.Case(24, 6, 128, 64, 'fp32', 0, 'tight', '')
    lengths = (5, 3, 40, 4, 9, 3)
    ag = R.make_agent(c)
    eng, it, eps = _arena(5, c.B, lengths, nstep)
    acts = np.concatenate([ep['action'] for ep in eps])
    slots = ag.engine.batch_slots()
    f32 = ag.engine._rebrac.view(torch.float32)
    o_na, o_nv = ((p - ag.engine._rebrac.data_ptr()) // 4 for p in (slots.next_action, slots.next_valid))
    seen = 0
    for s in range(3):
        m = ag.update(it, s)
        torch.cuda.synchronize()
        pairs = eng.last_pairs(c.B)
        pairs = pairs.cpu().numpy() if torch.is_tensor(pairs) else np.asarray(pairs)
        na, nv = next_action_rule(acts, lengths, pairs.reshape(-1, 2), nstep)
        assert np.array_equal(f32[o_na:o_na + c.B * c.A].cpu().numpy().reshape(c.B, c.A), na)
        assert np.array_equal(f32[o_nv:o_nv + c.B].cpu().numpy(), nv)
        assert m['next_valid'] == float(nv.mean())
        seen += int((nv == 0).sum())
    assert 0 < seen < 3 * c.B


def test_pickle_and_snapshot_round_trip():
    """A pickled agent continues bit for bit (the constructor allocates and attaches a fresh buffer; the coefficients ride in the
    attributes), on an HBM iterator and on a plain iterator of 6- and 7-tuples; a snapshot's three nets restore into a fresh agent."""
    from exorl_amd import agents, snapshot
    c = R.Case(24, 6, 128, 64, 'fp32', 7, 'tight', '')
    torch.manual_seed(5)
    a = agents.ReBRACAgent('rebrac', (c.O,), (c.A,), 'cuda', 1e-4, c.H, 0.01, 0.2, 1, c.B, 0.3, True, actor_bc_coef=2.0, critic_bc_coef=0.5)
    assert a.alpha == 1.0 / (2.0 * c.A)
    ns = _synth.NoiseStream(2)
    z = [ns.draw((c.B, c.A)) for _ in range(8)]
    for s in range(2):
        hooked(a, z[2 * s:2 * s + 2]).update(iter([R.batch(c, s)]), s)
    b = pickle.loads(pickle.dumps(a))
    assert (b.actor_bc_coef, b.critic_bc_coef, b.alpha) == (2.0, 0.5, a.alpha) and b.engine.opt_steps() == (2, 2)
    assert b.engine._rebrac is not None and b.engine._rebrac.data_ptr() != a.engine._rebrac.data_ptr()
    six = R.batch(c, 2)[:6]                          # no next_valid: every row valid
    assert hooked(a, z[4:6]).update(iter([six]), 2) == hooked(b, z[4:6]).update(iter([six]), 2)
    assert a.engine.metrics_raw()[L().M_REBRAC_VALID] == 1.0
    assert hooked(a, z[6:8]).update(iter([R.batch(c, 3)]), 3) == hooked(b, z[6:8]).update(iter([R.batch(c, 3)]), 3)
    assert_same_bits(state_of(a), state_of(b), 'pickle')
    # through the replay: the two go on over equal arenas, whose gather fills each agent's own buffer
    keep_a, keep_b = _arena(11, c.B), _arena(11, c.B)
    for s in range(4, 6):
        zs = [ns.draw((c.B, c.A)) for _ in range(2)]
        ma, mb = hooked(a, zs).update(keep_a[1], s), hooked(b, zs).update(keep_b[1], s)
        assert ma == mb and 0 < ma['next_valid'] < 1 and ma['critic_penalty'] > 0
    torch.cuda.synchronize()
    assert_same_bits(state_of(a), state_of(b), 'pickle, through the replay')
    assert a.engine.opt_steps() == b.engine.opt_steps() == (6, 6)
    sd = snapshot.state_dicts(a)
    assert list(sd) == list(NETS)
    torch.manual_seed(6)
    fresh = agents.ReBRACAgent('rebrac', (c.O,), (c.A,), 'cuda', 1e-4, c.H, 0.01, 0.2, 1, c.B, 0.3, True, actor_bc_coef=2.0, critic_bc_coef=0.5)
    snapshot.load_state_dicts(fresh, dict(sd))
    for nm in NETS:
        for p, q in zip(getattr(a, nm).parameters(), getattr(fresh, nm).parameters()):
            assert torch.equal(p, q), nm
    m = fresh.update(keep_a[1], 0)
    assert np.isfinite(m['critic_loss']) and m['critic_penalty'] > 0
    with pytest.raises(ValueError, match='ReBRACAgent'):
        fresh.update(iter([R.batch(c, 0)[:5]]), 1)
