"""The SARSA setting on the GPU (exorl_agent_set_sarsa; OneStepTD3BCAgent, OneStepCRRAgent, BehaviorQAgent): the row kernel alone against numpy
bit for bit, a dataset without valid next actions against the base kind bit for bit (four kinds, four precisions, three drivers), a
dataset where every next action is valid and the critic no longer sees the actor, one step of every case of tests/_rebrac_twin.py and its
three-step trajectories against the float64 twin of tests/_sarsa_twin.py at ReBRAC's bars, update = per-phase = captured graph, the
replay's next-action column as the step sees it, the refusals and detaching, pickling and snapshots, and BehaviorQAgent.value()."""
import pickle

import numpy as np
import pytest
import torch

import _grad_grid as G
import _rebrac_twin as R
import _sarsa_twin as S
import _synth
from _eval_twin import BARS
from _fqe_twin import value_dict
from _next_action_rule import next_action_rule

pytestmark = pytest.mark.gpu

NETS = ('actor', 'critic', 'critic_target')
PHASES = {'td3_bc': (0, 1, 2, 3), 'td3': (0, 1, 2, 3), 'crr': (0, 1, 2, 3), 'fqe': (10, 11)}
MIXED = (200, 3, 300, 5, 250, 4)         # episodes are drawn uniformly: half of the rows come from the short ones, one in eight ends its episode


def L():
    from exorl_amd import _lib
    return _lib


def state_of(ag, metrics=True, nets=NETS):
    out = {}
    for nm in nets:
        for i, p in enumerate(getattr(ag, nm).parameters()):
            out[f'{nm}.param{i}'] = p.detach().clone()
    for nm, net in (('actor', L().NET_ACTOR), ('critic', L().NET_CRITIC)):
        if nm in nets:
            for w, tag in ((L().T_GRAD, 'grad'), (L().T_ADAM_M, 'adam_m'), (L().T_ADAM_V, 'adam_v')):
                out[f'{nm}.{tag}'] = ag.engine.flat(net, w).detach().clone()
    if metrics:
        out['metrics'] = torch.from_numpy(ag.engine.metrics_raw()[:10].copy())
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
    """update() through exorl_agent_update_phase over the kind's plan, as under torch.distributed."""
    eng = ag.engine
    eng.run_update = lambda stddev, nc=None, na=None: [eng.update_phase(ph, stddev, nc, na) for ph in PHASES[ag.KIND]]
    return ag


def poison_part(ag):
    """NaN into the SARSA buffer's scratch run (the per-chunk sums); next_action / next_valid are inputs and stay."""
    eng = ag.engine
    pad = lambda n: -(-n // 64) * 64
    eng._sarsa.view(torch.float32)[pad(eng.batch * eng.act_dim) + pad(eng.batch):] = float('nan')


def _arena(seed, B, lengths=MIXED, nstep=1, O=24, A=6):
    from exorl_amd.engine import ReplayEngine
    from exorl_amd.replay_buffer import ArenaIterator
    eps = _synth.synth_episodes(seed, list(lengths), O, A)
    eng = ReplayEngine((O,), np.float32, A, 0, sum(lengths) + len(lengths) + 64, len(lengths) + 4)
    eng.set_order([eng.append_episode(ep) for ep in eps])
    eng.seed_philox(77)
    return eng, ArenaIterator(eng, B, nstep, 0.99, 'philox'), eps


def _same_nets(dst, src):
    for nm in NETS:
        getattr(dst, nm).load_state_dict(getattr(src, nm).state_dict())
    return dst


# ---- 1. the row kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('valid', ['ones', 'zeros', 'mixed'])
@pytest.mark.parametrize('A', [1, 6, 16])
@pytest.mark.parametrize('rows', [1, 7, 256, 257, 1000])
def test_row_kernel_vs_numpy(rows, A, valid):
    """exorl_next_action_rows against numpy: the destination's A action columns take the next action's row where v != 0 and keep their own
    bits elsewhere; into a contiguous destination and into rows of 5 + A floats (the step's O + A) whose other columns keep theirs. The
    invalid rows of the source hold NaN: nothing of them arrives. The sum of v is exact (a count) and equals the chunk-ordered float32 sum
    of the per-chunk partials, the same on NaN-filled partials."""
    lib = L().load()
    rs = np.random.RandomState(1000 * rows + 10 * A + len(valid))
    v = {'ones': np.ones(rows), 'zeros': np.zeros(rows), 'mixed': (rs.uniform(size=rows) < 0.6)}[valid].astype(np.float32)
    y = rs.uniform(-1, 1, (rows, A)).astype(np.float32)
    y[v == 0] = np.nan
    chunks = lib.exorl_iql_rows_chunks(rows)
    dev = lambda a: torch.from_numpy(a).cuda()
    yd, vd = dev(y), dev(v)
    for off in (0, 5):
        ld = A + off
        x = rs.uniform(-1, 1, (rows, ld)).astype(np.float32)
        want = x.copy()
        want[v != 0, off:] = y[v != 0]
        outs = []
        for fill in (0.0, float('nan')):
            xd = dev(x)
            part, sums = (torch.full((n,), fill, device='cuda') for n in (chunks, 1))
            L().check(lib.exorl_next_action_rows(yd.data_ptr(), A, vd.data_ptr(), rows, A, np.float32(1.0 / rows), xd.data_ptr() + 4 * off, ld,
                                                 part.data_ptr(), sums.data_ptr(), None))
            torch.cuda.synchronize()
            outs.append([a.cpu().numpy() for a in (xd, part, sums)])
        got, part, sums = outs[0]
        assert got.tobytes() == want.tobytes(), f'ld={ld}: {int((got != want).sum())} elements differ'
        for a, b in zip(outs[0], outs[1]):
            assert a.tobytes() == b.tobytes(), 'NaN-filled partials changed the result: something is read before it is written'
        acc = np.float32(0.0)
        for p in part:
            acc = np.float32(acc + p)
        assert sums[0] == acc == np.float32(v.sum()) and part.size == -(-rows // 256)
        if valid == 'zeros':
            assert got.tobytes() == x.tobytes()


# ---- 2. v = 0 on every row: the base kind, bit for bit ----------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['eager', 'phased', 'graph'])
@pytest.mark.parametrize('precision', ['fp32', 'bf16x3', 'bf16x6', 'bf16'])
@pytest.mark.parametrize('kind', ['td3_bc', 'td3', 'crr', 'fqe'])
def test_without_valid_next_actions_the_step_is_the_base_kinds(kind, precision, mode):
    """Three steps of the kind with the setting on and of its base class, one seed, over equal arenas of length-1 episodes at nstep = 1 (every
    sample ends its episode: v = 0 on every row; device sampler, device noise): parameters, gradients, Adam moments, the target, the
    counters and the base's metric slots bit for bit. eager and phased report metrics (the unfused kernels), graph runs the fused path."""
    use_tb = mode != 'graph'
    torch.manual_seed(1)
    on = S.make_kind(kind, True, 24, 6, 128, 64, use_tb, precision)
    off = _same_nets(S.make_kind(kind, False, 24, 6, 128, 64, use_tb, precision), on)
    assert on.engine._sarsa is not None and off.engine._sarsa is None
    keeps = [_arena(9, 64, (1,) * 96), _arena(9, 64, (1,) * 96)]
    for ag, keep in zip((on, off), keeps):
        if mode == 'phased':
            phased(ag)
        if mode == 'graph':
            assert ag.enable_graph(keep[1])
    for s in range(3):
        m1, m0 = on.update(keeps[0][1], s), off.update(keeps[1][1], s)
        assert {k: v for k, v in m1.items() if k != 'next_valid'} == m0
        if use_tb:
            assert m0 and on.engine.metrics_raw()[L().M_SARSA_VALID] == 0.0
            assert m1.get('next_valid', 0.0) == 0.0 and ('next_valid' in m1) == (kind != 'td3')
    torch.cuda.synchronize()
    assert_same_bits(state_of(off, metrics=use_tb), state_of(on, metrics=use_tb), f'{kind} {precision} {mode}')
    assert on.engine.opt_steps() == off.engine.opt_steps() == (3, 3) and on.engine.noise_counter() == off.engine.noise_counter()


class _LastStarts:
    """An HBM iterator that hands the GIVEN sampler each episode's last start (idx = len at nstep = 1: the next step ends the episode)."""

    def __init__(self, eng, lengths, B):
        self.engine, self.B = eng, B
        self.pairs = np.array([(i % len(lengths), lengths[i % len(lengths)]) for i in range(B)], np.int32)

    def sample_into(self, out, batch=None):
        self.engine.sample_into(out, batch or self.B, 1, 0.99, L().SAMPLER_GIVEN, self.pairs)


@pytest.mark.parametrize('kind', ['td3_bc', 'td3', 'crr', 'fqe'])
def test_given_last_starts_are_the_base_kinds_step(kind):
    """Ordinary episodes, GIVEN pairs at each episode's last start: v = 0 on every row, the gather's next-action rows are zeros, and three
    steps are the base class's bit for bit, metrics included."""
    torch.manual_seed(2)
    on = S.make_kind(kind, True, 24, 6, 128, 64)
    off = _same_nets(S.make_kind(kind, False, 24, 6, 128, 64), on)
    its = [_LastStarts(_arena(9, 64)[0], MIXED, 64) for _ in range(2)]
    for s in range(3):
        m1, m0 = on.update(its[0], s), off.update(its[1], s)
        assert m1.pop('next_valid', 0.0) == 0.0 and m1 == m0 and on.engine.metrics_raw()[L().M_SARSA_VALID] == 0.0
    torch.cuda.synchronize()
    assert float(on.engine._sarsa.view(torch.float32)[:64 * 6 + 64].abs().max()) == 0.0
    assert_same_bits(state_of(off), state_of(on), kind)


# ---- 3. v = 1 on every row: the critic does not see the actor -----------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('kind', ['td3_bc', 'crr'])
def test_with_every_next_action_valid_the_critic_ignores_the_actor(kind, precision):
    """Two agents that differ in the actor's weights alone, three steps on 6-tuples (no next_valid: every row valid): critic, critic target
    and the critic's gradient and Adam moments end bit-identical. The same pair with the setting off (the base classes on the 5-tuples)
    ends with different critics: the comparison is not vacuous."""
    O, A, H, B = 24, 6, 128, 64
    c = R.Case(O, A, H, B, precision, 50, 'tight', '')
    for sarsa in (True, False):
        torch.manual_seed(4)
        a = S.make_kind(kind, sarsa, O, A, H, B, True, precision)
        b = _same_nets(S.make_kind(kind, sarsa, O, A, H, B, True, precision), a)
        b.actor.load_state_dict({k: v + 0.05 * (i + 1) for i, (k, v) in enumerate(a.actor.state_dict().items())})
        assert not torch.equal(next(iter(a.actor.parameters())), next(iter(b.actor.parameters())))
        for s in range(3):
            batch = R.batch(c, s)[:6 if sarsa else 5]
            ma, mb = a.update(iter([batch]), s), b.update(iter([batch]), s)
            if sarsa:
                assert ma['next_valid'] == mb['next_valid'] == 1.0
                assert all(ma[k] == mb[k] for k in ('critic_loss', 'critic_target_q', 'critic_q1', 'critic_q2', 'batch_reward'))
        torch.cuda.synchronize()
        sa, sb = (state_of(x, metrics=False, nets=('critic', 'critic_target')) for x in (a, b))
        if sarsa:
            assert_same_bits(sa, sb, f'{kind} {precision}')
        else:
            assert not torch.equal(sa['critic.param0'], sb['critic.param0']) and not torch.equal(sa['critic.adam_m'], sb['critic.adam_m'])


# ---- 4. against the float64 twin --------------------------------------------------------------------------------------------------------
def run(c, route, poison=False):
    torch.manual_seed(0)
    ag = R.load_params(S.make_agent(c, route != 'fast'), c)
    hooked(ag, R.noise(c))
    if poison:
        ag.engine.poison_scratch()
        poison_part(ag)
    m = ag.update(iter([R.batch(c)]), 0)
    torch.cuda.synchronize()
    return ag, m


@pytest.mark.parametrize('route', ['metrics', 'fast'])
@pytest.mark.parametrize('c', [pytest.param(c, id=S.case_id(c)) for c in S.CASES])
def test_gradients_vs_twin64(c, route):
    """OneStepTD3BCAgent on ReBRAC's cases (mixed v, fixed noise), tests/test_gpu_rebrac.py's comparison and bars unchanged: per gradient
    tensor, e(x) = max|x - g64| / max|g64| after the ReLU flips the near-kink set allows: fp32 e(gpu) <= 8 max(e(twin32), 2^-23); bf16x3
    8 e(twin32) + 4 * 2^-16; bf16x6 8 max(e(twin32), 2^-23) + 4 * 3 * 2^-24; plain bf16 cosine >= 0.999. Metrics (next_valid among them):
    fp32 / bf16x6 2e-5 relative + 1e-6, bf16x3 1e-4, bf16 3e-2. Both twins take their actor step from the critic this run's optimiser
    step produced. The setting is a bit-exact copy in front of the same kernels: no bar is widened for it. The same step on NaN-filled
    scratch and NaN-filled per-chunk sums: same bits. Every figure is printed before it is asserted."""
    ag, m = run(c, route)
    after = [p.cpu().numpy() for p in ag.critic.parameters()]
    r64 = S.run_twin(c, torch.float64, None if c.bar == 'coarse' else S.KINK_DELTA[c.precision], critic_after=after)
    r32 = S.run_twin(c, torch.float32, critic_after=after)
    tag = f'{S.case_id(c)} {route}'
    prec = c.precision
    rel = {'fp32': 2e-5, 'bf16x6': 2e-5, 'bf16x3': 1e-4, 'bf16': 3e-2}[prec]
    worst_m = 0.0
    if route != 'fast':
        assert sorted(m) == sorted(r64.metrics), (sorted(m), sorted(r64.metrics))
        worst_m = max(abs(m[k] - v) / (abs(v) + 1e-6 / rel) for k, v in r64.metrics.items())
        assert abs(m['next_valid'] - float(R.batch(c)[6].mean())) <= 1e-6
    else:
        assert m == {}
    ratio_w = e_gpu_w = e_32_w = 0.0
    cos_w, worst_at, flips = 1.0, '', 0
    floor = G.KINK_FLOOR['bf16x3' if prec == 'bf16x3' else 'fp32']
    failures = []
    for step, want in R.steps_of(r64):
        got = [g.cpu().numpy().reshape(w.shape) for g, w in zip(getattr(ag, step).grads(), want)]
        assert len(got) == len(want) and all(np.all(np.isfinite(g)) for g in got), f'{tag}: {step} gradients'
        if c.bar == 'coarse':
            for i, (g, w) in enumerate(zip(got, want)):
                cos = G.tensor_cosines([g], [w])[0]
                cos_w = min(cos_w, cos)
                e_gpu_w = max(e_gpu_w, float(np.abs(g - w).max() / np.abs(w).max()))
                if cos < 0.999:
                    failures.append((step, i, cos))
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
        print(f'[sarsa grid] {tag}: coarse e(gpu) {e_gpu_w:.2e} worst cosine {cos_w:.6f} (bar 0.999); worst metric error {worst_m:.2e} (bar {rel:g})')
    else:
        print(f'[sarsa grid] {tag}: tight e(gpu) {e_gpu_w:.2e} e(twin32) {e_32_w:.2e} worst e(gpu)/bar {ratio_w:.3f} at {worst_at or "-"} {K} '
              f'flips gpu {flips}; worst metric error {worst_m:.2e} (bar {rel:g})')
    assert not failures, (tag, failures)
    if route != 'fast':
        for k, v in r64.metrics.items():
            assert abs(m[k] - v) <= rel * abs(v) + 1e-6 * (3e4 if prec == 'bf16' else 1), (tag, k, m[k], v)
    assert ratio_w <= 1.0, f'{tag}: e(gpu) is {ratio_w:.2f} x its bar at {worst_at} (e(gpu) {e_gpu_w:.2e}, e(twin32) {e_32_w:.2e})'
    dirty, m1 = run(c, route, poison=True)
    assert_same_bits(state_of(ag), state_of(dirty), f'{tag} poisoned')
    assert m == m1


@pytest.mark.parametrize('c', [pytest.param(c, id=S.case_id(c)) for c in S.TRAJ_CASES])
def test_three_steps_vs_twin64(c):
    """Parameters after each of three steps against the float64 twin on ReBRAC's trajectory cases, by tests/test_gpu_rebrac.py's rules with
    its recorded figures (tests/_rebrac_twin.py: TRAJ_E32, TRAJ_BF16_COS, DP_RULE), unchanged: fp32-grade element by element within
    max(traj_bar, twice the float32 CPU twin's recorded error), bf16x3 per net by the three-step rule, plain bf16 by the direction of the
    parameter change. The metrics of every step at the precision's one-step tolerance. Every figure is printed before anything is asserted."""
    prec = c.precision
    ag = R.load_params(S.make_agent(c), c)
    tw = S.make_twin(c, torch.float64)
    start = {nm: [p.detach().double().cpu().numpy().copy() for p in getattr(ag, nm).parameters()] for nm in NETS}
    ns = _synth.NoiseStream(c.seed + 3)
    rel = R.TRAJ_METRIC_REL[prec]
    flat = lambda ts: np.concatenate([np.asarray(t, np.float64).reshape(-1) for t in ts])
    bad, worst, worst_m = [], 0.0, 0.0
    for step in range(S.TRAJ_STEPS):
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
            ceiling = R.DP_RULE['ceiling'] * (step + 1) / S.TRAJ_STEPS
            share = float(np.mean(d > R.DP_RULE['abs'] + R.DP_RULE['rel'] * np.abs(w)))
            dg, dw = g - flat(start[nm]), w - flat(start[nm])
            cos = float(dg @ dw / (np.linalg.norm(dg) * np.linalg.norm(dw)))
            print(f'[sarsa traj] {S.case_id(c)} step {step} {nm}: max |d| {d.max():.2e} (ceiling {ceiling:.2e}), share outside 2e-6 + 1e-4 |p| '
                  f'{share:.2e}, cosine of the change {cos:.6f}')
            if d.max() > ceiling:
                bad.append(f'step {step} {nm}: max |d| {d.max():.3e} over {ceiling:.3e}')
            if prec == 'bf16x3' and share > R.DP_RULE['share']:
                bad.append(f'step {step} {nm}: {share:.3e} of the elements outside the rule')
            if prec == 'bf16':
                floor = 1.0 - 2.0 * (1.0 - R.TRAJ_BF16_COS[step][NETS.index(nm)])
                if cos < floor:
                    bad.append(f'step {step} {nm}: cosine {cos:.6f} under {floor:.6f}')
    print(f'[sarsa traj] {S.case_id(c)}: worst element error / bar {worst:.3f}, worst metric error / tolerance {worst_m:.3f}')
    assert not bad, bad
    assert ag.engine.opt_steps() == (3, 3)


# ---- 5. update = per-phase = captured graph ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('kind', ['td3_bc', 'crr', 'fqe'])
def test_update_phases_and_graph_agree_bit_for_bit(kind, precision):
    """Agents of one seed over equal arenas (mixed v), three steps. use_tb=True (every driver runs the same kernels): exorl_agent_update, the
    kind's phases one by one, the captured graph, and exorl_agent_update with the workspace's scratch and the buffer's sums refilled with
    NaN before every step: parameters, gradients, Adam moments, targets and metrics bit for bit. Then use_tb=False, the fused path: graph =
    eager = eager on poisoned scratch. The captured graph holds the buffer's pointers: set_sarsa refuses until it is released."""
    for use_tb, modes in ((True, ('eager', 'phased', 'graph', 'poison')), (False, ('eager', 'graph', 'poison'))):
        runs = []
        for mode in modes:
            torch.manual_seed(3)
            ag = S.make_kind(kind, True, 24, 6, 128, 64, use_tb, precision)
            keep = _arena(9, 64)
            if mode == 'phased':
                phased(ag)
            if mode == 'graph':
                assert ag.enable_graph(keep[1])
            ms = []
            for s in range(3):
                if mode == 'poison':
                    ag.engine.poison_scratch()
                    poison_part(ag)
                ms.append(ag.update(keep[1], s))
            torch.cuda.synchronize()
            runs.append((ag, keep, ms))
        for (ag, _, ms), mode in zip(runs[1:], modes[1:]):
            assert_same_bits(state_of(runs[0][0], metrics=use_tb), state_of(ag, metrics=use_tb), f'{kind} {precision} use_tb={use_tb} {mode}')
            assert ms == runs[0][2], mode
            if use_tb:
                assert ag.engine.metrics_raw()[L().M_SARSA_VALID] == runs[0][0].engine.metrics_raw()[L().M_SARSA_VALID]
        if use_tb:
            assert all(0 < m['next_valid'] < 1 for m in runs[0][2])
    g, keep, _ = runs[modes.index('graph')]
    with pytest.raises(L().ExorlError, match='captured graph'):
        g.engine.set_sarsa(g.engine._sarsa)
    with pytest.raises(L().ExorlError, match='captured graph'):
        g.engine.set_sarsa(None)
    g.update(keep[1], 3)
    torch.cuda.synchronize()
    assert g.engine.opt_steps() == (4, 4)


# ---- 6. through the replay ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nstep', [1, 3])
def test_slots_hold_the_replays_next_action(nstep):
    """iter-style sampling from a synthetic arena into the agent's slots: what the step read as a' and v equals the numpy rule of
    tests/_next_action_rule.py on the pairs the sampler drew, and the step's next_valid metric is their mean."""
    c = R.Case(24, 6, 128, 64, 'fp32', 0, 'tight', '')
    lengths = (5, 3, 40, 4, 9, 3)
    ag = S.make_agent(c)
    eng, it, eps = _arena(5, c.B, lengths, nstep)
    acts = np.concatenate([ep['action'] for ep in eps])
    slots = ag.engine.batch_slots()
    buf = ag.engine._sarsa
    f32 = buf.view(torch.float32)
    assert slots.next_action == buf.data_ptr() and slots.next_action_stride == c.A
    o_na, o_nv = ((p - buf.data_ptr()) // 4 for p in (slots.next_action, slots.next_valid))
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


# ---- 7. refusals and detaching ---------------------------------------------------------------------------------------------------------------
def test_refusals_and_detaching():
    from exorl_amd import agents
    c = R.CASES[0]
    ag = R.load_params(S.make_agent(c), c)
    eng = ag.engine
    b, z = R.batch(c), R.noise(c)
    assert ag.enable_metric_window() is False
    with pytest.raises(L().ExorlError, match='SARSA setting has no metric window'):
        eng.set_metric_window()
    with pytest.raises(NotImplementedError):
        ag.evaluate(iter([b]))
    with pytest.raises(L().ExorlError, match='SARSA setting has no forward-only evaluation'):
        eng.set_eval()
    with pytest.raises(L().ExorlError, match='SARSA setting has no forward-only evaluation'):
        eng.evaluate()
    buf = eng._sarsa
    with pytest.raises(L().ExorlError, match='need'):
        eng.set_sarsa(buf[:buf.numel() - 256])
    with pytest.raises(L().ExorlError, match='256-byte aligned'):
        eng.set_sarsa(torch.zeros(buf.numel() + 64, dtype=torch.uint8, device='cuda')[4:])
    # mutually exclusive with ReBRAC, both ways
    rbuf = torch.zeros(eng.rebrac_bytes(), dtype=torch.uint8, device='cuda')
    with pytest.raises(L().ExorlError, match='SARSA setting is on'):
        eng.set_rebrac(rbuf, 1.0)
    re = R.make_agent(c)
    with pytest.raises(L().ExorlError, match='ReBRAC is set'):
        re.engine.set_sarsa(torch.zeros(re.engine.sarsa_bytes(), dtype=torch.uint8, device='cuda'))
    assert re.engine._sarsa is None and re.engine.batch_slots().next_action == re.engine._rebrac.data_ptr()
    bc = agents.BCAgent('bc', (c.O,), (c.A,), 'cuda', 1e-4, c.H, c.B, 0.2, True)
    with pytest.raises(L().ExorlError, match='is not TD3\\+BC, TD3, CRR or FQE'):
        bc.engine.set_sarsa(buf)
    with pytest.raises(L().ExorlError, match='is not TD3\\+BC, TD3, CRR or FQE'):
        bc.engine.sarsa_bytes()
    with pytest.raises(L().ExorlError, match='no ReBRAC buffer is set'):
        bc.engine.set_next_action(b[5])
    assert eng.opt_steps() == (0, 0)
    slots = eng.batch_slots()
    assert slots.next_action == buf.data_ptr() and slots.next_action_stride == c.A and slots.next_valid > slots.next_action
    # the refused calls changed nothing: the step is the SARSA one
    m1 = hooked(ag, z).update(iter([b]), 0)
    # 6 of 7 rows: the sum (exact) times fl(1 / 7), two roundings, against numpy's one
    assert abs(m1['next_valid'] - float(b[6].mean())) <= 2.0 ** -22 and eng.opt_steps() == (1, 1)
    # detached: the base kind again. NULL slots; the evaluation and the window attach, and while one is attached the setting is refused
    other = R.load_params(S.make_agent(c), c)
    eng, buf = other.engine, other.engine._sarsa
    eng.set_sarsa(None)
    slots = eng.batch_slots()
    assert (slots.next_action, slots.next_action_stride, slots.next_valid) == (None, 0, None)
    eng.set_eval()
    eng.set_batch(*b[:5])
    eng.evaluate()
    sums, rows = eng.eval_read()
    assert rows == c.B and np.all(np.isfinite(sums))
    eng.set_metric_window()
    with pytest.raises(L().ExorlError, match='detach the metric window'):
        eng.set_sarsa(buf)
    eng.set_metric_window(None)
    with pytest.raises(L().ExorlError, match='detach the eval buffer'):
        eng.set_sarsa(buf)
    eng.set_eval(None)
    # ReBRAC attaches on the detached handle and goes again; then the setting is attached again: the step `ag` took, bit for bit
    eng.set_rebrac(rbuf, 1.0)
    eng.set_rebrac(None, 0.0)
    eng.set_sarsa(buf)
    other._slots = None
    assert hooked(other, z).update(iter([b]), 0) == m1
    torch.cuda.synchronize()
    assert_same_bits(state_of(ag), state_of(other), 'detached and attached again')
    # a detached engine's step is TD3BCAgent's
    td = R.load_params(agents.TD3BCAgent('td3_bc', (c.O,), (c.A,), 'cuda', 1e-4, c.H, 0.01, 0.2, 1, c.B, 0.3, True, R.alpha_of(c.A)), c)
    ref = R.load_params(S.make_agent(c), c)
    ref.engine.set_sarsa(None)
    hooked(td, z).update(iter([b[:5]]), 0)
    ref.engine.set_batch(*b[:5])
    ref.engine.run_update(0.2, *z)
    torch.cuda.synchronize()
    assert_same_bits(state_of(td), state_of(ref), 'detached')


# ---- 8. pickle and snapshot ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['td3_bc', 'crr', 'fqe'])
def test_pickle_and_snapshot_round_trip(kind):
    """A pickled agent continues bit for bit (the constructor allocates and attaches a fresh buffer), on a plain iterator of 6- and 7-tuples
    and on an HBM iterator; a snapshot's three nets restore into a fresh agent; a 5-tuple is refused by name."""
    from exorl_amd import snapshot
    c = R.Case(24, 6, 128, 64, 'fp32', 7, 'tight', '')
    torch.manual_seed(5)
    a = S.make_kind(kind, True, c.O, c.A, c.H, c.B)
    ns = _synth.NoiseStream(2)
    # the step's two noise blocks, fixed: the device's noise counter is no part of a pickle (CRR's second is (B * num_value_samples, A); FQE draws none)
    z = lambda: [ns.draw((c.B, c.A)), ns.draw((c.B * (4 if kind == 'crr' else 1), c.A))]
    both = lambda batch, s, zs: (hooked(a, zs).update(batch(), s), hooked(b, zs).update(batch(), s))
    for s in range(2):
        hooked(a, z()).update(iter([R.batch(c, s)]), s)
    b = pickle.loads(pickle.dumps(a))
    assert type(b) is type(a) and b.engine.opt_steps() == (2, 2)
    assert b.engine._sarsa is not None and b.engine._sarsa.data_ptr() != a.engine._sarsa.data_ptr()
    six = R.batch(c, 2)[:6]                          # no next_valid: every row valid
    ma, mb = both(lambda: iter([six]), 2, z())
    assert ma == mb and a.engine.metrics_raw()[L().M_SARSA_VALID] == 1.0
    ma, mb = both(lambda: iter([R.batch(c, 3)]), 3, z())
    assert ma == mb
    keep_a, keep_b = _arena(11, c.B), _arena(11, c.B)
    for s in range(4, 6):
        zs = z()
        ma, mb = hooked(a, zs).update(keep_a[1], s), hooked(b, zs).update(keep_b[1], s)
        assert ma == mb and 0 < ma['next_valid'] < 1
    torch.cuda.synchronize()
    assert_same_bits(state_of(a), state_of(b), f'{kind} pickle')
    assert a.engine.opt_steps() == b.engine.opt_steps() == (6, 6)
    sd = snapshot.state_dicts(a)
    assert list(sd) == list(NETS)
    torch.manual_seed(6)
    fresh = S.make_kind(kind, True, c.O, c.A, c.H, c.B)
    snapshot.load_state_dicts(fresh, dict(sd))
    for nm in NETS:
        for p, q in zip(getattr(a, nm).parameters(), getattr(fresh, nm).parameters()):
            assert torch.equal(p, q), nm
    m = fresh.update(keep_a[1], 0)
    assert np.isfinite(m['critic_loss']) and 0 < m['next_valid'] <= 1
    with pytest.raises(ValueError, match=type(a).__name__):
        fresh.update(iter([R.batch(c, 0)[:5]]), 1)


# ---- 9. BehaviorQAgent.value() -----------------------------------------------------------------------------------------------------------
VB = 64


def _value_setup(precision, n_episodes):
    from exorl_amd.engine import ReplayEngine
    from exorl_amd.replay_buffer import ArenaIterator
    c = R.Case(24, 6, 128, VB, precision, 61, 'tight', 'value pass')
    lengths = ([1, 2, 3, 1, 17] + [4 + (7 * i) % 23 for i in range(n_episodes)])[:n_episodes]
    eps = _synth.synth_episodes(17, lengths, c.O, c.A)
    eng = ReplayEngine((c.O,), np.float32, c.A, 0, sum(lengths) + n_episodes + 64, n_episodes + 4)
    eng.set_order([eng.append_episode(ep) for ep in eps])
    eng.seed_philox(5)
    torch.manual_seed(1)
    ag = R.load_params(S.make_kind('fqe', True, c.O, c.A, c.H, c.B, False, precision), c)
    return c, eps, eng, ArenaIterator(eng, VB, 1, 0.99, 'philox'), ag


def _returns64(eps, gamma):
    g32 = np.float64(np.float32(gamma))
    out = []
    for ep in eps:
        r, d = ep['reward'].reshape(-1).astype(np.float64), ep['discount'].reshape(-1).astype(np.float64)
        ret, D = 0.0, 1.0
        for t in range(1, len(r)):
            ret += D * r[t]
            D *= g32 * d[t]
        out.append(ret)
    return np.array(out)


@pytest.mark.parametrize('n_episodes', [1, 2, VB + 1])
@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
def test_value_is_the_critic_at_the_first_observation_and_action(precision, n_episodes):
    """Over 1, 2 and batch + 1 episodes (a second pass with one valid row): every mean of the dict against the float64 forward of the twin's
    critic at (s_0, a_0), the episode's first observation and the action stored with the step after it, at tests/_eval_twin.BARS of the
    precision as tests/test_gpu_fqe.py's value test has it (the two that are not means at the same bar on the root-mean-square scale);
    behavior_value against the float64 recurrence. No actor forward runs: the same bits with the actor's weights overwritten in between."""
    c, eps, eng, it, ag = _value_setup(precision, n_episodes)
    got = ag.value(it)
    pa, pc = R.params(c)
    tw = S.SarsaFQETwin(list(pa.values()), list(pc.values()))
    q1, q2 = tw.q_rows(np.stack([ep['observation'][0] for ep in eps]), np.stack([ep['action'][1] for ep in eps]))
    want = value_dict(q1, q2, _returns64(eps, 0.99))
    names = {'fqe_value': 'behavior_q', 'fqe_value_q1': 'behavior_q_q1', 'fqe_value_q2': 'behavior_q_q2', 'fqe_value_stderr': 'behavior_q_stderr',
             'fqe_twin_rms': 'behavior_q_twin_rms'}
    want = {names.get(k, k): v for k, v in want.items()}
    rel, ab = BARS[precision]
    print(f'[behavior q] {precision} {n_episodes} episodes: ' + ' '.join(f'{k} {got[k]:.6g} (want {want[k]:.6g})' for k in want))
    assert list(got) == list(want) and got['episodes'] == n_episodes == want['episodes']
    for k in ('behavior_q', 'behavior_q_q1', 'behavior_q_q2'):
        assert abs(got[k] - want[k]) <= rel * abs(want[k]) + ab, (k, got[k], want[k])
    scale = float(np.sqrt(np.mean((0.5 * (q1 + q2)) ** 2)))
    assert abs(got['behavior_q_twin_rms'] - want['behavior_q_twin_rms']) <= rel * scale + ab
    assert abs(got['behavior_q_stderr'] - want['behavior_q_stderr']) <= rel * scale + ab
    assert abs(got['behavior_value'] - want['behavior_value']) <= 1e-12 * abs(want['behavior_value'])
    ag.actor.load_state_dict({k: torch.full_like(v, float('nan')) for k, v in ag.actor.state_dict().items()})
    assert ag.value(it) == got


@pytest.mark.parametrize('mode', ['eager', 'graph'])
def test_update_after_value_continues_bit_for_bit(mode):
    c = R.Case(24, 6, 128, 64, 'fp32', 0, 'tight', '')
    runs = []
    for with_value in (True, False):
        torch.manual_seed(3)
        ag = S.make_kind('fqe', True, c.O, c.A, c.H, c.B)
        eng, it, _ = _arena(9, c.B, (5, 1, 200, 300, 2, 250))
        if mode == 'graph':
            assert ag.enable_graph(it)
        ms = [ag.update(it, 0), ag.update(it, 1)]
        if with_value:
            v = ag.value(it)
            assert v['episodes'] == 6 and np.isfinite(v['behavior_q'])
        ms += [ag.update(it, 2), ag.update(it, 3)]
        torch.cuda.synchronize()
        runs.append((ag, ms, eng.last_pairs(c.B), (eng, it)))
    assert runs[0][1] == runs[1][1] and np.array_equal(runs[0][2], runs[1][2])
    assert_same_bits(state_of(runs[0][0]), state_of(runs[1][0]), mode)
    assert runs[0][0].engine.opt_steps() == runs[1][0].engine.opt_steps() == (4, 4)


def test_policy_refusals_name_the_class_that_was_called():
    from exorl_amd import agents
    cql = agents.CQLAgent('cql', (24,), (6,), 'cuda', 1e-4, 128, 0.01, 1, 64, True, 1.0, 3, 5.0, False)
    bc = agents.BCAgent('bc', (24,), (6,), 'cuda', 1e-4, 256, 64, 0.2, True)
    ev = S.make_kind('fqe', True, 24, 6, 128, 64)
    with pytest.raises(ValueError, match='^BehaviorQAgent: cannot evaluate a CQLAgent.*out of scope'):
        agents.BehaviorQAgent.for_policy(cql)
    with pytest.raises(ValueError, match='^BehaviorQAgent.set_policy.*of the evaluator'):
        ev.set_policy(bc)
    with pytest.raises(ValueError, match='^FQEAgent: cannot evaluate a CQLAgent'):
        agents.FQEAgent.for_policy(cql)


def test_behavior_q_evaluation_runs_at_nstep_3_with_and_without_a_policy():
    """The driver end to end at nstep = 3 (fitted_q_evaluation refuses that iterator): with a BC policy to shape the evaluator and fall back
    on, and without one from the shapes; the result is BehaviorQAgent.value()'s dict."""
    from exorl_amd import agents
    from exorl_amd.fqe import behavior_q_evaluation, fitted_q_evaluation
    eng, it, eps = _arena(9, 64, MIXED, nstep=3)
    bc = agents.BCAgent('bc', (24,), (6,), 'cuda', 1e-4, 128, 64, 0.2, False)
    with pytest.raises(ValueError, match='nstep=3'):
        fitted_q_evaluation(bc, it, 1)
    torch.manual_seed(0)
    r1, curve = behavior_q_evaluation(it, 4, policy=bc, value_every=2)
    torch.manual_seed(0)
    r2 = behavior_q_evaluation(it, 4, obs_shape=(24,), action_shape=(6,), hidden_dim=128, use_graph=False)
    for r in (r1, r2):
        assert list(r)[0] == 'behavior_q' and r['episodes'] == len(MIXED) and np.isfinite(r['behavior_q'])
        assert abs(r['behavior_value'] - float(np.mean(_returns64(eps, 0.99)))) <= 1e-9
    assert [s for s, _ in curve] == [2, 4] and curve[-1][1] == r1
