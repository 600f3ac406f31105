"""State agents in bf16x6 precision (fp32 mode's pipeline with the H x H products in three bf16 planes): gradients against the float64 twin
on both routes — the three-plane GEMM (128 | hidden_dim, 128 | batch) and the generic kernel's in-GEMM split —, NaN-filled scratch,
trajectories against the reference's recordings at fp32 mode's bars, the captured graph, and act().
Every gradient test prints its worst e(gpu) / bar as the grid does ("[grad grid bf16x6] ...")."""
import functools
import json

import numpy as np
import pytest
import torch

import _grad_grid as G
import _state_bf16x6_cases as S
import _synth
import test_gpu_agent as TA
import test_gpu_intr as TI
from test_gpu_grad_grid import ROUTES, _arena, assert_bit_identical, make, run, state_of

pytestmark = pytest.mark.gpu

CASE_PARAMS = [pytest.param(c, id=G.case_id(c)) for c in S.CASES]
PRODUCT_BOUND = 3.0 * 2.0 ** -24      # include/exorl_hip.h, EXORL_PREC_BF16X6: the three dropped terms per product


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('c', CASE_PARAMS)
def test_gradients_vs_twin64(c, route):
    """Per gradient tensor, e(x) = max|x - g64| / max|g64| after the ReLU flips K allows are taken out (fp32 mode's delta 2^-18, floor 2^-22):
        e(gpu) <= 8 max(e(twin32), 2^-23) + 4 * 3 * 2^-24
    the grid's bf16x3 bar, 8 e(twin32) + 4 * 2^-16 (four chained products of forward and backward), with the split-bf16 product bound 2^-16
    replaced by the three-plane bound 3 * 2^-24 of the header, kept over fp32 mode's floor. Metrics: fp32 mode's 2e-5 relative + 1e-6."""
    ag, m = run(c, route, False)
    after = [p.cpu().numpy() for p in ag.critic.parameters()] if hasattr(ag, 'critic') else None
    r64 = G.run_twin(c, torch.float64, S.KINK_DELTA, critic_after=after)
    r32 = G.run_twin(c, torch.float32, critic_after=after)
    tag = f'{G.case_id(c)} {route}'
    if route != 'fast':
        rel = 2e-5
        assert sorted(m) == sorted(r64.metrics), (sorted(m), sorted(r64.metrics))
        worst_m = max(abs(m[k] - v) / (abs(v) + 1e-6 / rel) for k, v in r64.metrics.items())
        print(f'[grad grid bf16x6] {tag}: worst metric error / (|v| + {1e-6 / rel:.0e}) = {worst_m:.2e} (bar {rel:g})')
        for k, v in r64.metrics.items():
            assert abs(m[k] - v) <= rel * abs(v) + 1e-6, (tag, k, m[k], v)
    else:
        assert m == {}
    nets = {'actor': ag.actor, 'critic': getattr(ag, 'critic', None)}
    e_gpu_w = e_32_w = ratio_w = 0.0
    flips_gpu = flips_32 = 0
    worst_at = ''
    for step, want in G.steps_of(r64):
        got = [g.cpu().numpy().reshape(w.shape) for g, w in zip(nets[step].grads(), want)]
        assert len(got) == len(want)
        for i, g in enumerate(got):
            assert np.all(np.isfinite(g)), f'{tag}: non-finite {step} gradient {i}'
        kinks = r64.kinks[step]
        assert kinks is not None, f'{tag}: |K| = {r64.n_kinks[step]} exceeds the cap of a tight case'
        d_gpu, f_gpu = G.explain_kinks(got, want, kinks, S.KINK_FLOOR, f'{tag} {step} gpu')
        d_32, f_32 = G.explain_kinks(dict(critic=r32.critic_grads, actor=r32.actor_grads)[step], want, kinks, S.KINK_FLOOR, f'{tag} {step} twin32')
        flips_gpu, flips_32 = flips_gpu + f_gpu, flips_32 + f_32
        for i, (eg, e3) in enumerate(zip(G.tensor_errors(d_gpu, want), G.tensor_errors(d_32, want))):
            bar = 8.0 * max(e3, 2.0 ** -23) + 4.0 * PRODUCT_BOUND
            if eg / bar > ratio_w:
                ratio_w, worst_at = eg / bar, f'{step}[{i}]'
            e_gpu_w, e_32_w = max(e_gpu_w, eg), max(e_32_w, e3)
    K = ' '.join(f'|K_{s}|={n}' for s, n in r64.n_kinks.items())
    print(f'[grad grid bf16x6] {tag} ({"planes" if S.on_plane_route(c) else "generic"}): tight e(gpu) {e_gpu_w:.2e} e(twin32) {e_32_w:.2e} '
          f'worst e(gpu)/bar {ratio_w:.3f} at {worst_at or "-"} {K} flips gpu {flips_gpu} twin32 {flips_32}')
    assert ratio_w <= 1.0, f'{tag}: e(gpu) is {ratio_w:.2f} x its bar at {worst_at} (e(gpu) {e_gpu_w:.2e}, e(twin32) {e_32_w:.2e})'


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('c', CASE_PARAMS)
def test_poisoned_scratch_is_not_read(c, route):
    """The same update with the scratch (the h1 / dz2 plane images among it) and all padding holding NaN bit patterns: bit-identical."""
    clean, m0 = run(c, route, False)
    dirty, m1 = run(c, route, True)
    tag = f'{G.case_id(c)} {route}'
    assert_bit_identical(state_of(clean), state_of(dirty), tag)
    assert m0.keys() == m1.keys() and all(m0[k] == m1[k] for k in m0), (tag, m0, m1)


@pytest.mark.parametrize('kind', ['td3_bc', 'td3', 'bc', 'ddpg', 'crr'])
def test_full_size_vs_reference(gold, kind):
    """tests/test_gpu_agent.py::test_full_size_vs_reference_fp32's body in bf16x6 at the bars it holds fp32 mode to (H = 1024, B = 1024 / BC 256:
    the plane route): per-step losses within 1e-4 of the reference's fp32 run over 10 steps, final parameter checksums and update directions."""
    g = json.load(open(gold / f'full_{kind}.json'))
    O, A, H, B = g['dims']
    ag = TA.make(kind, O, A, H, B, precision='bf16x6')
    TA.load_synth(ag, kind, O, A, H, g['param_seed'])
    ag.noise_hook = _synth.NoiseStream(g['noise_seed']).draw
    worst = 0.0
    for i in range(g['nsteps']):
        step = 2 * i if kind == 'ddpg' else i
        m = ag.update(iter([_synth.synth_batch(g['batch_seed'], i, B, O, A)]), step)
        for k, v in g['fp32']['metrics'][i].items():
            assert abs(m[k] - v) <= 1e-4 * abs(v) + 1e-6, (kind, i, k, m[k], v, g['fp64']['metrics'][i][k])
            worst = max(worst, abs(m[k] - v) / (abs(v) + 1e-2))
    print(f'[parity margin] {kind} bf16x6: worst relative metric error over {g["nsteps"]} steps = {worst:.2e} (bar 1e-4)')
    init = TA._init_samples(kind, O, A, H, g['param_seed'], g['sample_stride'])
    for nm, net in TA.nets_of(ag):
        flat = torch.cat([p.double().reshape(-1) for p in net.parameters()])
        s, s2, mx = g['fp32']['checksums'][nm]
        assert abs(float((flat * flat).sum()) - s2) <= 1e-5 * s2, nm
        assert abs(float(flat.sum()) - s) <= 1e-4 * max(1.0, abs(s)) + 2e-2, nm
        assert abs(float(flat.abs().max()) - mx) <= 1e-4 * mx, nm
        cos, out = TA._delta_report(f'metrics path {kind} bf16x6 {nm}', flat[::g['sample_stride']].cpu().numpy(),
                                    np.array(g['fp32']['param_sample'][nm]), init[nm], 1e-4)
        assert cos >= 0.9999 and out <= (0.08 if kind == 'td3' else 0.02), (kind, nm, cos, out)


def test_cql_full_size_vs_reference(gold):
    """tests/test_gpu_agent.py::test_cql_full_size_vs_reference_fp32's body in bf16x6 (its bars do not depend on the precision): 10240 critic rows."""
    TA.test_cql_full_size_vs_reference_fp32(gold, 'bf16x6')


def test_tiny_trajectory_ddpg(gold):
    """H = 32, B = 8: the generic route, five steps against the reference's recorded metrics and weights."""
    TA.test_tiny_trajectory_vs_reference(gold, 'ddpg', 'bf16x6')


def test_tiny_trajectory_rnd_end_to_end(gold, monkeypatch):
    """A reward-free agent on states with precision='bf16x6' end to end: backbone and intrinsic module in the same mode."""
    monkeypatch.setattr(TI, 'make', functools.partial(TI.make, precision='bf16x6'))
    TI.test_tiny_trajectory_vs_reference(gold, 'rnd')


@pytest.mark.parametrize('kind', ['td3_bc', 'ddpg'])
def test_hip_graph_step_equals_eager(kind):
    """tests/test_gpu_agent.py::test_hip_graph_step_equals_eager's body at H = 128, B = 128 in bf16x6: the captured sample + update graph (plane
    conversions and three-plane launches among its nodes) replays exactly what the eager launches do."""
    O, A, H, B = 24, 6, 128, 128
    torch.manual_seed(3)
    a1 = TA.make(kind, O, A, H, B, precision='bf16x6')
    torch.manual_seed(3)
    a2 = TA.make(kind, O, A, H, B, precision='bf16x6')
    e1, it1 = _arena(9, 128)
    e2, it2 = _arena(9, 128)
    assert a1.enable_graph(it1)
    steps = [0, 2, 4, 6] if kind == 'ddpg' else [0, 1, 2, 3]
    for s in steps:
        m1, m2 = a1.update(it1, s), a2.update(it2, s)
        assert m1.keys() == m2.keys()
        for k in m1:
            assert m1[k] == m2[k], (kind, s, k, m1[k], m2[k])
    for (n1, net1), (n2, net2) in zip(TA.nets_of(a1), TA.nets_of(a2)):
        for p, q in zip(net1.parameters(), net2.parameters()):
            assert torch.equal(p, q), n1
    assert a1.engine.opt_steps() == a2.engine.opt_steps()
    a1.disable_graph()
    m1, m2 = a1.update(it1, 8), a2.update(it2, 8)
    assert m1 == m2


def test_poisoned_scratch_is_not_read_through_the_captured_graph():
    """The grid's graph-poison test at H = 128, B = 128 in bf16x6: scratch poisoned before the capture and again between two replays."""
    c = G.Case('td3_bc', 24, 6, 128, 128, 0, 'bf16x6', 0, 'tight', '')
    agents_ = []
    for poison in (False, True):
        torch.manual_seed(3)
        ag = make(c, False)
        e, it = _arena(9, 128)
        if poison:
            ag.engine.poison_scratch()
        assert ag.enable_graph(it)
        for s in range(3):
            ag.update(it, s)
            if poison and s == 0:
                torch.cuda.synchronize()
                ag.engine.poison_scratch()
        torch.cuda.synchronize()
        agents_.append((ag, e, it))
    assert_bit_identical(state_of(agents_[0][0]), state_of(agents_[1][0]), 'graph bf16x6 H=128 B=128')


@pytest.mark.parametrize('H', [128, 1024])
def test_act_agrees_with_fp32(H):
    """One observation, same weights: the bf16x6 agent's action against the fp32 agent's to 2e-5 (the project's fused-vs-generic bar), through
    act() (one fused launch) and through the engine's batched path at 3 rows (the generic GEMM in the agent's precision)."""
    O, A, B = 24, 6, 128
    ags = {}
    for p in ('fp32', 'bf16x6'):
        ags[p] = TA.make('td3_bc', O, A, H, B, precision=p)
        TA.load_synth(ags[p], 'td3_bc', O, A, H, 5)
    obs = np.random.RandomState(0).standard_normal((3, O)).astype(np.float32)
    a32, a6 = (ags[p].act(obs[0], 0, eval_mode=True) for p in ('fp32', 'bf16x6'))
    assert a32.shape == (A,) and np.abs(a32 - a6).max() <= 2e-5, np.abs(a32 - a6).max()
    b32, b6 = (ags[p].engine.act(obs, 0.2, True).cpu().numpy() for p in ('fp32', 'bf16x6'))
    assert np.abs(b32 - b6).max() <= 2e-5, np.abs(b32 - b6).max()
    assert np.abs(b32[0] - a32).max() <= 2e-5
