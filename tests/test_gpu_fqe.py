"""FQEAgent on the GPU: the row kernel on crafted rows against float64, one step of every case of tests/_fqe_cases.py against the float64
twin at the bars of tests/test_gpu_grad_grid.py, the frozen actor, a five-step trajectory, graph = eager and poisoned scratch bit for bit,
pickling, the value pass against the twin's float64 forward, the arena's episode returns, fitted_q_evaluation end to end, and the refusals
that need a handle."""
import ctypes
import pickle

import numpy as np
import pytest
import torch

import _fqe_cases as F
import _grad_grid as G
import _synth
from _eval_twin import BARS
from _fqe_twin import value_dict
from _iql_cases import traj_bar

pytestmark = pytest.mark.gpu

NETS = ('actor', 'critic', 'critic_target')
make, load = F.make_agent, F.load_params


def state_of(ag):
    out = {}
    for nm in NETS:
        net = getattr(ag, nm)
        for i, p in enumerate(net.parameters()):
            out[f'{nm}.param{i}'] = p.detach().clone()
    for i, g in enumerate(ag.critic.grads()):
        out[f'critic.grad{i}'] = g.detach().clone()
    out['metrics'] = torch.from_numpy(ag.engine.metrics_raw())
    return out


def actor_state(ag):
    """Everything of the actor a step could touch: parameters, Adam moments, and every derived weight image the configuration has."""
    from exorl_amd import _lib as L
    out = {f'flat{w}': ag.engine.flat(L.NET_ACTOR, w).clone() for w in (L.T_PARAM, L.T_ADAM_M, L.T_ADAM_V)}
    out.update({k: v.clone() for k, v in ag.engine.weight_images(L.NET_ACTOR).items() if v is not None})
    return out


def assert_same_bits(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        assert not bool(torch.isnan(b[k].float()).any()), f'{tag}: NaN in {k}'
        assert torch.equal(a[k], b[k]), f'{tag}: {k} differs'


# ---- 1. the row kernel ------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize('rows', [1, 7, 255, 256, 257, 1000, 8193, 8200])
def test_row_kernel_vs_float64(rows):
    """exorl_fqe_rows on random rows in (-0.5, 0.5) and two crafted ones: row 2 has D = 0 (y = r for both nets) and row 3 has Q_1 within 1e-6
    of y_1. dq against the float64 value of 2 (Q_i - y_i) inv_bg, in ulp of fp32 at that value. Count of roundings: 2. The kernel forms
    Q_i - (r + D Q'_i) in double (the products of two fp32 are exact there) and rounds it once to fp32, at most 0.5 ulp of the difference,
    which is a relative 2^-24 and so at most 1 ulp of the product it is carried into; 2 e is exact; the product with inv_bg rounds once more,
    0.5 ulp. 1.5 ulp in all: the bar is 2 ulp, half of the 4 ulp tests/test_gpu_iql.py holds iql_rows' dq to. Row 3 is held to its own
    (tiny) ulp like every other row: its cancellation happens in double. The six sums: bitwise equal on a second run, equal to the float32
    sum of the per-chunk partials in chunk order (8193 rows: 33 chunks on 32 workgroups), and within 1e-5 of sum |term| of the float64 sums."""
    from exorl_amd import _lib as L
    lib = L.load()
    rs = np.random.RandomState(rows)
    f = lambda *s: rs.uniform(-0.5, 0.5, s).astype(np.float32)
    tq, q, r = f(2, rows), f(2, rows), f(rows)
    D = rs.uniform(0.9, 0.99, rows).astype(np.float32)
    if rows > 3:
        D[2] = 0.0
        q[0, 3] = np.float32(np.float64(r[3]) + np.float64(D[3]) * np.float64(tq[0, 3])) + np.float32(1e-6)
    inv_bg = np.float32(1.0 / rows)
    d = [torch.from_numpy(x).cuda() for x in (tq, q, r, D)]
    chunks = lib.exorl_fqe_rows_chunks(rows)
    assert chunks == -(-rows // 256)
    outs = []
    for _ in range(2):
        dq = torch.full((2 * rows,), float('nan'), device='cuda')
        part, sums = torch.full((chunks * 6,), float('nan'), device='cuda'), torch.full((6,), float('nan'), device='cuda')
        L.check(lib.exorl_fqe_rows(*[x.data_ptr() for x in d], rows, inv_bg, dq.data_ptr(), part.data_ptr(), sums.data_ptr(), None))
        torch.cuda.synchronize()
        outs.append([x.cpu().numpy() for x in (dq, sums, part)])
    dq, sums, part = outs[0]
    assert sums.tobytes() == _chunk_ordered_sums(part, 6).tobytes(), 'the sums are not the chunk-ordered float32 sums of the partials'
    assert sums.tobytes() == outs[1][1].tobytes(), 'the sums differ between two runs'
    assert dq.tobytes() == outs[1][0].tobytes()
    x = lambda a: a.astype(np.float64)
    y = x(r)[None] + x(D)[None] * x(tq)                         # (2, rows): a target per net
    dq64 = 2.0 * (x(q) - y) * float(inv_bg)
    err = np.abs(x(dq.reshape(2, rows)) - dq64) / _ulp(dq64)
    print(f'[fqe rows] rows={rows}: dq {float(err.max()):.2f} ulp (bar 2)' + (f', the near-cancelling row {float(err[0, 3]):.2f} ulp of {dq64[0, 3]:.3e}' if rows > 3 else ''))
    assert np.all(np.isfinite(dq)) and float(err.max()) <= 2.0, float(err.max())
    if rows > 3:
        assert dq[2] == np.float32(2.0) * (q[0, 2] - r[2]) * inv_bg and 0.0 < abs(x(q)[0, 3] - y[0, 3]) < 2e-6
    terms = [x(r), 0.5 * (y[0] + y[1]), x(q)[0], x(q)[1], (x(q)[0] - y[0]) ** 2, (x(q)[1] - y[1]) ** 2]
    for i, tm in enumerate(terms):
        assert abs(float(sums[i]) - tm.sum()) <= 1e-5 * np.abs(tm).sum() + 1e-30, (i, float(sums[i]), tm.sum())


# ---- 2. one step against the float64 twin ---------------------------------------------------------------------------------------------
def run(c, poison=False, use_tb=True):
    torch.manual_seed(0)
    ag = load(make(c, use_tb), c)
    if poison:
        ag.engine.poison_scratch()
    m = ag.update(iter([F.batch(c)]), 0)
    torch.cuda.synchronize()
    return ag, m


@pytest.mark.parametrize('c', [pytest.param(c, id=F.case_id(c)) for c in F.CASES])
def test_gradients_vs_twin64(c):
    """test_gpu_grad_grid's bars per gradient tensor, e(x) = max|x - g64| / max|g64| after the ReLU flips the near-kink set allows:
    fp32 e(gpu) <= 8 max(e(twin32), 2^-23); bf16x3 8 e(twin32) + 4 * 2^-16; bf16x6 (test_gpu_state_bf16x6) 8 max(e(twin32), 2^-23) + 4 * 3 * 2^-24;
    plain bf16 cosine >= 0.999. Metrics (exactly update()'s five keys): fp32 / bf16x6 2e-5 relative + 1e-6, bf16x3 1e-4, bf16 3e-2. The same
    step on NaN-filled scratch: same bits."""
    ag, m = run(c)
    r64, r32 = F.twin_pair(c)
    tag = F.case_id(c)
    prec = c.precision
    rel = {'fp32': 2e-5, 'bf16x6': 2e-5, 'bf16x3': 1e-4, 'bf16': 3e-2}[prec]
    assert list(m) == ['batch_reward', 'critic_target_q', 'critic_q1', 'critic_q2', 'critic_loss'] and sorted(m) == sorted(r64.metrics)
    worst_m = max(abs(m[k] - v) / (abs(v) + 1e-6 / rel) for k, v in r64.metrics.items())
    ratio_w = e_gpu_w = e_32_w = 0.0
    cos_w, worst_at = 1.0, ''
    floor = G.KINK_FLOOR['bf16x3' if prec == 'bf16x3' else 'fp32']
    want = r64.critic_grads
    got = [g.cpu().numpy().reshape(w.shape) for g, w in zip(ag.critic.grads(), want)]
    assert len(got) == len(want) and all(np.all(np.isfinite(g)) for g in got), f'{tag}: critic gradients'
    assert all(float(g.abs().max()) == 0.0 for g in ag.actor.grads()), f'{tag}: the frozen actor got a gradient'
    flips = 0
    if c.bar == 'coarse':
        for i, (g, w) in enumerate(zip(got, want)):
            cos = G.tensor_cosines([g], [w])[0]
            cos_w = min(cos_w, cos)
            e_gpu_w = max(e_gpu_w, float(np.abs(g - w).max() / np.abs(w).max()))
            assert cos >= 0.999, (tag, i, cos)
        print(f'[fqe grid] {tag}: coarse e(gpu) {e_gpu_w:.2e} worst cosine {cos_w:.6f} (bar 0.999); worst metric error {worst_m:.2e} (bar {rel:g})')
    else:
        kinks = r64.kinks['critic']
        d_gpu, flips = G.explain_kinks(got, want, kinks, floor, f'{tag} critic gpu')
        d_32, _ = G.explain_kinks(r32.critic_grads, want, kinks, floor, f'{tag} critic twin32')
        for i, (eg, e3) in enumerate(zip(G.tensor_errors(d_gpu, want), G.tensor_errors(d_32, want))):
            bar = {'fp32': 8.0 * max(e3, 2.0 ** -23), 'bf16x6': 8.0 * max(e3, 2.0 ** -23) + 12.0 * 2.0 ** -24, 'bf16x3': 8.0 * e3 + 4.0 * 2.0 ** -16}[prec]
            if eg / bar > ratio_w:
                ratio_w, worst_at = eg / bar, f'critic[{i}]'
            e_gpu_w, e_32_w = max(e_gpu_w, eg), max(e_32_w, e3)
        print(f'[fqe grid] {tag}: tight e(gpu) {e_gpu_w:.2e} e(twin32) {e_32_w:.2e} worst e(gpu)/bar {ratio_w:.3f} at {worst_at or "-"} '
              f'|K|={r64.n_kinks["critic"]} flips gpu {flips}; worst metric error {worst_m:.2e} (bar {rel:g})')
    for k, v in r64.metrics.items():
        assert abs(m[k] - v) <= rel * abs(v) + 1e-6 * (3e4 if prec == 'bf16' else 1), (tag, k, m[k], v)
    assert ratio_w <= 1.0, f'{tag}: e(gpu) is {ratio_w:.2f} x its bar at {worst_at} (e(gpu) {e_gpu_w:.2e}, e(twin32) {e_32_w:.2e})'
    dirty, m1 = run(c, poison=True)
    assert_same_bits(state_of(ag), state_of(dirty), f'{tag} poisoned')
    assert m == m1


# ---- 3. five steps: the trajectory and the frozen actor ---------------------------------------------------------------------------------
def test_five_steps_vs_twin64():
    c = F.TRAJ
    ag = load(make(c), c)
    tw = F.make_twin(c, torch.float64)
    n0 = ag.engine.noise_counter()
    for step in range(5):
        b = F.batch(c, step)
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
    assert ag.engine.opt_steps() == (5, 5) and ag.engine.noise_counter() == n0


SHAPE = F.Case(24, 6, 128, 64, 'fp32', 0, 'tight', '')


@pytest.mark.parametrize('precision,B', [('fp32', 64), ('bf16x3', 64), ('bf16x6', 128), ('bf16', 64)])
def test_actor_is_bit_identical_after_five_steps(precision, B):
    """Parameters, Adam moments and every weight image of the actor (the transposed W0, the bf16 planes of the precision's route) before and
    after five steps; the critic and its target did move."""
    c = SHAPE._replace(precision=precision, B=B, seed=33)
    ag = load(make(c, use_tb=False), c)
    before, crit = actor_state(ag), state_of(ag)
    for step in range(5):
        ag.update(iter([F.batch(c, step)]), step)
    torch.cuda.synchronize()
    after = actor_state(ag)
    assert before.keys() == after.keys() and len(before) >= 4
    for k in before:
        assert torch.equal(before[k], after[k]), (precision, k)
    assert float(after['flat2'].abs().max()) == 0.0 and float(after['flat3'].abs().max()) == 0.0          # Adam never ran on it
    now = state_of(ag)
    assert not torch.equal(crit['critic.param0'], now['critic.param0']) and not torch.equal(crit['critic_target.param0'], now['critic_target.param0'])


# ---- 4. graph, poison, pickle ---------------------------------------------------------------------------------------------------------------
def _arena(seed, B=64, lengths=(200, 300, 250)):
    from exorl_amd.engine import ReplayEngine
    from exorl_amd.replay_buffer import ArenaIterator
    eng = ReplayEngine((24,), np.float32, 6, 0, 4096, 256)
    eng.set_order([eng.append_episode(ep) for ep in _synth.synth_episodes(seed, list(lengths), 24, 6)])
    eng.seed_philox(77)
    return eng, ArenaIterator(eng, B, 1, 0.99, 'philox')


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
def test_graph_equals_eager_and_poisoned_scratch(precision):
    """Three agents from one seed over three equal arenas, four steps: a captured graph, eager launches, and eager launches with the scratch
    refilled with NaN before every step. Parameters, gradients, targets and metrics bit for bit; update() leaves the noise counter alone; the
    replay's Philox counter ends in the same place (the captured step advances it from the critic's optimiser pass, its last kernel)."""
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
        runs.append((ag, ms, keep, keep[0].last_pairs(c.B)))
    for ag, ms, _, pairs in runs[1:]:
        assert ms == runs[0][1] and np.array_equal(pairs, runs[0][3])
        assert_same_bits(state_of(runs[0][0]), state_of(ag), precision)
    assert runs[0][0].engine.opt_steps() == runs[1][0].engine.opt_steps() == (4, 4)


def test_pickle_round_trip():
    c = SHAPE
    torch.manual_seed(5)
    a = make(c)
    a.set_obs_normalizer(np.full(c.O, 0.25, np.float32), np.full(c.O, 2.0, np.float32))
    batches = [_synth.synth_batch(11, s, c.B, c.O, c.A) for s in range(4)]
    for s in range(2):
        a.update(iter([batches[s]]), s)
    b = pickle.loads(pickle.dumps(a))
    assert b.engine.opt_steps() == (2, 2) and np.array_equal(b.obs_norm_mean, a.obs_norm_mean) and np.array_equal(b.obs_norm_inv, a.obs_norm_inv)
    for s in range(2, 4):
        assert a.update(iter([batches[s]]), s) == b.update(iter([batches[s]]), s)
    assert_same_bits(state_of(a), state_of(b), 'pickle')
    assert_same_bits(actor_state(a), actor_state(b), 'pickle actor')


# ---- 5. set_policy, act, refusals ------------------------------------------------------------------------------------------------------------
def test_set_policy_for_policy_act_and_refusals():
    from exorl_amd import _lib as L
    from exorl_amd import agents
    c = F.CASES[1]
    td = agents.TD3BCAgent('td3_bc', (c.O,), (c.A,), 'cuda', 3e-4, c.H, 0.02, 0.2, 1, c.B, 0.3, True, 2.5, precision='bf16x3')
    td.set_obs_normalizer(np.linspace(-1, 1, c.O).astype(np.float32), np.linspace(0.5, 2, c.O).astype(np.float32))
    ev = agents.FQEAgent.for_policy(td, use_tb=True)
    assert (ev.engine.obs_dim, ev.engine.act_dim, ev.engine.hidden_dim, ev.engine.batch) == (c.O, c.A, c.H, c.B)
    assert ev.lr == 3e-4 and ev.critic_target_tau == 0.02 and ev.engine.cfg.precision == td.engine.cfg.precision
    for p, q in zip(ev.actor.parameters(), td.actor.parameters()):
        assert torch.equal(p, q)
    assert np.array_equal(ev.obs_norm_mean, td.obs_norm_mean) and np.array_equal(ev.obs_norm_inv, td.obs_norm_inv)
    obs = np.random.RandomState(1).standard_normal(c.O).astype(np.float32)
    assert np.array_equal(ev.act(obs, 0, True), td.act(obs, 0, True)) and np.array_equal(ev.act(obs, 0, False), td.act(obs, 0, True))
    for other in (agents.BCAgent('bc', (c.O,), (c.A,), 'cuda', 1e-4, c.H, c.B, 0.2, True),
                  agents.IQLAgent('iql', (c.O,), (c.A,), 'cuda', 1e-4, c.H, 0.01, 0.2, 1, c.B, True)):
        ev.set_policy(other)
        assert all(torch.equal(p, q) for p, q in zip(ev.actor.parameters(), other.actor.parameters())) and ev.obs_norm_mean is None
    cql = agents.CQLAgent('cql', (c.O,), (c.A,), 'cuda', 1e-4, c.H, 0.01, 1, c.B, True, 1.0, 3, 5.0, False)
    with pytest.raises(ValueError, match='out of scope'):
        ev.set_policy(cql)
    with pytest.raises(ValueError, match='of the evaluator'):
        ev.set_policy(agents.BCAgent('bc', (c.O,), (c.A,), 'cuda', 1e-4, 2 * c.H, c.B, 0.2, True))
    assert ev.enable_metric_window() is False
    with pytest.raises(NotImplementedError):
        ev.evaluate(iter([F.batch(c)]))
    with pytest.raises(L.ExorlError):
        ev.engine.set_eval()
    with pytest.raises(L.ExorlError, match='no metric window'):
        ev.engine.set_metric_window()
    with pytest.raises(L.ExorlError, match="not one of FQE's"):
        ev.engine.update_phase(0, 1.0)
    with pytest.raises(L.ExorlError, match="is FQE's"):
        td.engine.update_phase(10, 0.2)
    with pytest.raises(L.ExorlError, match="is FQE's"):
        cql.engine.update_phase(11, 0.2)
    with pytest.raises(L.ExorlError, match='not FQE'):
        td.engine.fqe_value(1)
    with pytest.raises(L.ExorlError, match='no value window'):
        ev.engine.fqe_value(1)
    ev.engine.set_fqe_value()
    for rows in (0, c.B + 1):
        with pytest.raises(L.ExorlError, match='outside'):
            ev.engine.fqe_value(rows)
    assert ctypes.sizeof(L.AgentCfg) == 80


# ---- 6. value() ------------------------------------------------------------------------------------------------------------------------
VB, VEPISODES = 64, 150
VLENGTHS = [1, 2, 3, 1, 17] + [4 + (7 * i) % 23 for i in range(VEPISODES - 5)]           # 150 episodes, lengths 1 .. 26: batches of 64, 64, 22


def _value_setup(precision, episodes=None, normalizer=None):
    from exorl_amd.engine import ReplayEngine
    from exorl_amd.replay_buffer import ArenaIterator
    c = F.Case(24, 6, 128, VB, precision, 61, 'tight', 'value pass')
    eps = episodes if episodes is not None else _synth.synth_episodes(17, VLENGTHS, c.O, c.A)
    eng = ReplayEngine((c.O,), np.float32, c.A, 0, sum(VLENGTHS) + VEPISODES + 64, 256)
    eng.set_order([eng.append_episode(ep) for ep in eps])
    eng.seed_philox(5)
    if normalizer is not None:
        eng.set_obs_normalizer(*normalizer)
    torch.manual_seed(1)
    ag = load(make(c, use_tb=False), c)
    return c, eps, eng, ArenaIterator(eng, VB, 1, 0.99, 'philox'), ag


def _returns64(eps, gamma):
    g32 = np.float64(np.float32(gamma))
    out = []
    for ep in eps:
        r, d = ep['reward'].reshape(-1).astype(np.float64), ep['discount'].reshape(-1).astype(np.float64)
        R, D = 0.0, 1.0
        for t in range(1, len(r)):
            R += D * r[t]
            D *= g32 * d[t]
        out.append(R)
    return np.array(out)


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3', 'bf16x6', 'bf16'])
def test_value_vs_twin64(precision):
    """150 episodes, lengths from 1 up, B = 64: three batches, the last with 22 valid rows. Every mean of the dict against the twin's float64
    forward at tests/_eval_twin.BARS of the precision (fqe_twin_rms and fqe_value_stderr, which are not means, at the same bar on the
    root-mean-square scale); behavior_value against the float64 recurrence; the same dict, bit for bit, when the padding rows of the last
    batch hold NaN observations; and from a second call."""
    c, eps, eng, it, ag = _value_setup(precision)
    got = ag.value(it)
    tw = F.make_twin(c, torch.float64)
    q1, q2 = tw.value_rows(np.stack([ep['observation'][0] for ep in eps]))
    want = value_dict(q1, q2, _returns64(eps, 0.99))
    rel, ab = BARS[precision]
    print(f'[fqe value] {precision}: ' + ' '.join(f'{k} {got[k]:.6g} (want {want[k]:.6g})' for k in want))
    assert list(got) == list(want) and got['episodes'] == VEPISODES == want['episodes']
    for k in ('fqe_value', 'fqe_value_q1', 'fqe_value_q2'):
        assert abs(got[k] - want[k]) <= rel * abs(want[k]) + ab, (k, got[k], want[k])
    scale = float(np.sqrt(np.mean((0.5 * (q1 + q2)) ** 2)))
    assert abs(got['fqe_twin_rms'] - want['fqe_twin_rms']) <= rel * scale + ab
    assert abs(got['fqe_value_stderr'] - want['fqe_value_stderr']) <= (rel * scale + ab)
    assert abs(got['behavior_value'] - want['behavior_value']) <= 1e-12 * abs(want['behavior_value'])
    assert ag.value(it) == got

    class Poisoned(type(it)):
        """The same batches with NaN observations written over the padding rows of the agent's obs slot before each pass."""
        def episode_starts(self, batch=None, out=None):
            for pairs, valid in super().episode_starts(batch, out):
                rows = ag.engine._view(out.obs, batch * c.O).view(batch, c.O)
                rows[valid:] = float('nan')
                yield pairs, valid
    it.__class__ = Poisoned
    assert ag.value(it) == got


@pytest.mark.parametrize('mode', ['eager', 'graph'])
def test_update_after_value_continues_bit_for_bit(mode):
    runs = []
    for with_value in (True, False):
        torch.manual_seed(3)
        ag = make(SHAPE)
        eng, it = _arena(9, lengths=[5, 1, 200, 300, 2, 250])
        if mode == 'graph':
            assert ag.enable_graph(it)
        ms = [ag.update(it, 0), ag.update(it, 1)]
        if with_value:
            v = ag.value(it)
            assert v['episodes'] == 6 and np.isfinite(v['fqe_value'])
        ms += [ag.update(it, 2), ag.update(it, 3)]
        torch.cuda.synchronize()
        runs.append((ag, ms, eng.last_pairs(SHAPE.B), (eng, it)))
    assert runs[0][1] == runs[1][1] and np.array_equal(runs[0][2], runs[1][2])
    assert_same_bits(state_of(runs[0][0]), state_of(runs[1][0]), mode)
    assert_same_bits(actor_state(runs[0][0]), actor_state(runs[1][0]), mode)
    assert runs[0][0].engine.opt_steps() == runs[1][0].engine.opt_steps() == (4, 4)


def test_value_through_a_normalising_loader_equals_a_hand_normalised_dataset(tmp_path):
    """make_offline_replay_loader(normalize_obs=True) over a directory, against a plain arena fed the same episodes normalised on the host with
    the loader's own (mean32, inv32) and utils.normalize_obs: the gather applies the same two fp32 operations, so the dicts are equal."""
    from exorl_amd import utils
    from exorl_amd.replay_buffer import make_offline_replay_loader, save_episode
    c = F.Case(24, 6, 128, VB, 'fp32', 61, 'tight', 'value pass')
    eps = _synth.synth_episodes(17, VLENGTHS, c.O, c.A)
    for i, ep in enumerate(eps):
        save_episode(ep, tmp_path / f'episode_{i:06d}_{len(ep["reward"]) - 1}.npz')
    it = iter(make_offline_replay_loader(None, tmp_path, 10 ** 6, VB, 1, 0.99, sampler='philox', seed=4, normalize_obs=True))
    torch.manual_seed(1)
    ag = load(make(c, use_tb=False), c)
    got = ag.value(it)
    mean32, inv32 = it.obs_normalizer
    hand = [dict(ep, observation=utils.normalize_obs(ep['observation'], mean32, inv32)) for ep in eps]
    _, _, _, it2, ag2 = _value_setup('fp32', episodes=hand)
    want = ag2.value(it2)
    assert got == want and got['episodes'] == VEPISODES
    plain = _value_setup('fp32')
    assert plain[4].value(plain[3])['fqe_value'] != got['fqe_value']          # the normaliser was applied


def test_value_covers_every_shard_and_the_holdout_split(tmp_path):
    """Two shards with a hold-out split: value(iter(loader)) walks both training arenas, value(.holdout) both hold-out arenas, no episode twice
    and none left out: weighted by their episode counts the two dicts add up to the value over one arena holding all the episodes (the
    per-row Q are the same numbers; only the order of the float64 adds differs)."""
    from exorl_amd.engine import ReplayEngine
    from exorl_amd.replay_buffer import ArenaIterator, make_offline_replay_loader, save_episode
    c = F.Case(24, 6, 128, VB, 'fp32', 61, 'tight', 'value pass')
    lengths = [3, 1, 9, 4, 12, 7, 5, 2, 8, 6, 11, 10]
    eps = _synth.synth_episodes(19, lengths, c.O, c.A)
    for i, ep in enumerate(eps):
        save_episode(ep, tmp_path / f'episode_{i:06d}_{lengths[i]}.npz')
    it = iter(make_offline_replay_loader(None, tmp_path, 10 ** 6, VB, 2, 0.99, sampler='philox', seed=4, holdout_every=3))
    ag = load(make(c, use_tb=False), c)
    train, held = ag.value(it), ag.value(it.holdout)
    assert (train['episodes'], held['episodes']) == (8, 4)
    eng = ReplayEngine((c.O,), np.float32, c.A, 0, sum(lengths) + 64, 32)
    eng.set_order([eng.append_episode(ep) for ep in eps])
    whole = ag.value(ArenaIterator(eng, VB, 1, 0.99, 'philox'))
    assert whole['episodes'] == 12
    for k in ('fqe_value', 'fqe_value_q1', 'fqe_value_q2', 'behavior_value'):
        both = (8 * train[k] + 4 * held[k]) / 12
        assert abs(both - whole[k]) <= 1e-12 * max(abs(whole[k]), 1.0), (k, both, whole[k])
    assert train['fqe_value'] != held['fqe_value']


# ---- 7. episode returns -------------------------------------------------------------------------------------------------------------------
RLENGTHS = [1, 2, 63, 64, 65, 255, 256, 257, 1000]


def _check_returns(eng, eps, gamma, tag):
    got = eng.episode_returns(gamma)
    assert got.dtype == np.float64 and got.shape == (len(eps),)
    g32 = np.float64(np.float32(gamma))
    for e, ep in enumerate(eps):
        r, d = ep['reward'].reshape(-1).astype(np.float64), ep['discount'].reshape(-1).astype(np.float64)
        R, D, mass = 0.0, 1.0, 0.0
        for t in range(1, len(r)):
            R += D * r[t]
            mass += abs(D * r[t])
            D *= g32 * d[t]
        assert abs(got[e] - R) <= 1e-12 * mass, (tag, e, len(r) - 1, got[e], R)
    assert eng.episode_returns(gamma).tobytes() == got.tobytes(), f'{tag}: two calls differ'
    return got


def test_episode_returns_vs_sequential_float64():
    """|got - want| <= 1e-12 sum_t |D_t r_t| against the sequential float64 recurrence: reassociating <= 1000 fp64 terms costs at most about
    1000 * 2^-53 = 1.1e-13 of that sum, and in practice (a tree of depth 8 over runs of <= 4) three orders less. Episodes of every length around
    the 64-lane and 256-thread edges, random rewards in (-1, 1), all-ones discounts except one episode with a zero discount mid-way (the
    steps behind it must not count); before and after an eviction, a compaction and a reorder."""
    from exorl_amd.engine import ReplayEngine
    rs = np.random.RandomState(3)
    eps = _synth.synth_episodes(21, RLENGTHS, 3, 2)
    for ep in eps:
        ep['reward'] = rs.uniform(-1, 1, ep['reward'].shape).astype(np.float32)
        ep['discount'] = np.ones_like(ep['discount'])
    eps[5]['discount'][100] = 0.0
    eps[5]['reward'][101:] = 1e6                               # behind the zero discount: any leak would be seen
    rows = sum(RLENGTHS) + len(RLENGTHS)
    eng = ReplayEngine((3,), np.float32, 2, 0, rows + 40, 16)
    slots = [eng.append_episode(ep) for ep in eps]
    eng.set_order(slots)
    assert eng.num_episodes() == len(eps)
    got = _check_returns(eng, eps, 0.99, 'full')
    assert abs(got[5]) < 101.0
    eng.evict(slots[3])                                         # a hole: its rows are not read, the table has one episode fewer
    assert eng.num_episodes() == len(eps) - 1
    _check_returns(eng, eps[:3] + eps[4:], 0.99, 'hole')
    new = _synth.synth_episodes(22, [70], 3, 2)[0]
    slots[3] = eng.append_episode(new)                          # 71 rows into 40 spare ones: the arena compacts first
    order = [slots[i] for i in (8, 3, 0, 7, 1, 6, 2, 5, 4)]
    eng.set_order(order)
    live = eps[:3] + [new] + eps[4:]
    _check_returns(eng, [live[i] for i in (8, 3, 0, 7, 1, 6, 2, 5, 4)], 0.99, 'compacted and reordered')
    _check_returns(eng, [live[i] for i in (8, 3, 0, 7, 1, 6, 2, 5, 4)], 1.0, 'gamma 1')
    from exorl_amd import _lib as L
    buf = np.zeros(4)
    assert L.load().exorl_replay_episode_returns(eng.h, 0.99, buf.ctypes.data, 4, None) != 0          # n is the table's count, nothing else
    eng.set_order([])
    with pytest.raises(L.ExorlError, match='no resident episode'):
        eng.episode_returns(0.99)


# ---- 8. fitted_q_evaluation --------------------------------------------------------------------------------------------------------------
def test_fitted_q_evaluation_equals_driving_the_agent_by_hand(tmp_path):
    from exorl_amd import agents
    from exorl_amd.fqe import fitted_q_evaluation
    from exorl_amd.replay_buffer import make_offline_replay_loader, save_episode
    O, A, H, B, STEPS = 24, 6, 32, 64, 300
    for i, ep in enumerate(_synth.synth_episodes(31, [40, 1, 55, 38, 60, 47], O, A)):
        save_episode(ep, tmp_path / f'episode_{i:06d}_{len(ep["reward"]) - 1}.npz')
    torch.manual_seed(2)
    policy = agents.TD3BCAgent('td3_bc', (O,), (A,), 'cuda', 1e-4, H, 0.01, 0.2, 1, B, 0.3, False, 2.5, precision='bf16x3')
    loader = lambda: iter(make_offline_replay_loader(None, tmp_path, 10 ** 6, B, 1, 0.99, sampler='philox', seed=4))
    torch.manual_seed(7)
    got, curve = fitted_q_evaluation(policy, loader(), STEPS, lr=3e-4, critic_target_tau=0.05, seed=9, value_every=100)
    torch.manual_seed(7)
    it = loader()
    ev = agents.FQEAgent.for_policy(policy, lr=3e-4, critic_target_tau=0.05, seed=9)
    assert ev.enable_graph(it)
    mid = None
    for step in range(STEPS):
        ev.update(it, step)
        if step + 1 == 200:
            mid = ev.value(it)
    want = ev.value(it)
    assert got == want and got['episodes'] == 6 and ev.engine.opt_steps() == (STEPS, STEPS)
    assert [s for s, _ in curve] == [100, 200, 300] and curve[1][1] == mid and curve[2][1] == got
    assert curve[0][1]['fqe_value'] != got['fqe_value']          # the critic moved
    assert fitted_q_evaluation(policy, loader(), 3, use_graph=False)['episodes'] == 6
    from exorl_amd.replay_buffer import ArenaIterator
    with pytest.raises(ValueError, match='nstep=1'):
        fitted_q_evaluation(policy, ArenaIterator(_arena(9)[0], B, 3, 0.99, 'philox'), 1)


def test_value_window_attach_read_reset_detach():
    """FQE's value window through its whole life at batch 259, and the buffers exorl_agent_set_fqe_value refuses (tests/_windows.py)."""
    import _windows as W
    eng = W.engine('fqe')
    W.check_window(eng, 'fqe_value', lambda: eng.fqe_value(W.B), W.B, 'no value window')
