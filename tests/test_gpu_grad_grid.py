"""One update() of every state agent over the kernel dispatch grid (tests/_grad_grid.py): every gradient tensor and the metrics against
the float64 autograd twin (oracle/twin64.py), and the same step again on scratch memory filled with NaN, which must not change one bit.
Three routes through the library:
  metrics   use_tb=True, one whole-step call: critic_loss / actor_stats / head_bwd, partials reduced inside the optimiser launch
  fast      use_tb=False, one whole-step call: qhead, folded target heads, finalize_adam (what bench.py times)
  phased    use_tb=True, the four phases called one by one as under torch.distributed: finalize_grads + the plain Adam launch"""
import numpy as np
import pytest
import torch

import _grad_grid as G
import _synth

pytestmark = pytest.mark.gpu

ROUTES = ['metrics', 'fast', 'phased']
CASE_PARAMS = [pytest.param(c, id=G.case_id(c)) for c in G.CASES]


def make(c, use_tb):
    from exorl_amd import agents
    O, A, H, B, p = c.O, c.A, c.H, c.B, c.precision
    k = G.base_kind(c)
    if k == 'td3_bc':
        return agents.TD3BCAgent('td3_bc', (O,), (A,), 'cuda', 1e-4, H, 0.01, 0.2, 1, B, 0.3, use_tb, 2.5, precision=p)
    if k == 'td3':
        return agents.TD3Agent('td3', (O,), (A,), 'cuda', 1e-4, H, 0.01, 0.2, 1, B, 0.3, use_tb, precision=p)
    if k == 'crr':
        return agents.CRRAgent('crr', (O,), (A,), 'cuda', 1e-4, H, 0.01, c.n, c.kind.partition('-')[2] or 'indicator', 0.2, 1, B, 0.3, use_tb, precision=p)
    if k == 'cql':
        return agents.CQLAgent('cql', (O,), (A,), 'cuda', 1e-4, H, 0.01, 1, B, use_tb, 0.01, c.n, 5.0, c.kind == 'cql-lagrange', precision=p)
    if k == 'bc':
        return agents.BCAgent('bc', (O,), (A,), 'cuda', 1e-4, H, B, 0.2, use_tb, precision=p)
    return agents.DDPGAgent('ddpg', True, 'states', (O,), (A,), 'cuda', 1e-4, 50, H, 0.01, 2000, 2, 0.2, 3, B, 0.3, True, use_tb, False, precision=p)


def nets_of(ag):
    return [('actor', ag.actor)] + ([('critic', ag.critic), ('critic_target', ag.critic_target)] if hasattr(ag, 'critic') else [])


def run(c, route, poison):
    """One update() from the case's seeded parameters, batch and noise; poison: scratch filled with NaN just before the step."""
    torch.manual_seed(0)
    ag = make(c, route != 'fast')
    if route == 'phased':
        eng = ag.engine
        eng.run_update = lambda stddev, nc=None, na=None: [eng.update_phase(ph, stddev, nc, na) for ph in range(4)]
    _, _, pa, pc = G.params(c)
    ag.actor.load_state_dict({k: torch.from_numpy(v) for k, v in pa.items()})
    if pc:
        ag.critic.load_state_dict({k: torch.from_numpy(v) for k, v in pc.items()})
        ag.critic_target.load_state_dict(ag.critic.state_dict())
    blocks = iter(G.noise(c))

    def hook(shape, kind='normal'):
        z = next(blocks)
        assert z.size == int(np.prod(shape)), (z.shape, shape)
        return z
    ag.noise_hook = hook
    if poison:
        ag.engine.poison_scratch()
    m = ag.update(iter([G.batch(c)]), 0)
    torch.cuda.synchronize()
    return ag, m


def state_of(ag):
    """Everything a step leaves behind: parameters, gradients, target parameters, the raw metric block, CQL's scalars."""
    out = {}
    for nm, net in nets_of(ag):
        for i, p in enumerate(net.parameters()):
            out[f'{nm}.param{i}'] = p.detach().clone()
        if nm != 'critic_target':
            for i, g in enumerate(net.grads()):
                out[f'{nm}.grad{i}'] = g.detach().clone()
    out['metrics'] = torch.from_numpy(ag.engine.metrics_raw())
    if ag.KIND == 'cql':
        out['cql_scalars'] = torch.from_numpy(ag.engine.cql_alpha_state())
    return out


def assert_bit_identical(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        assert not bool(torch.isnan(y).any()), f'{tag}: NaN in {k} after the poisoned step'
        assert torch.equal(x, y), f'{tag}: {k} differs after the poisoned step (max |d| = {float((x - y).abs().max()):.3e})'


def _cos_ratio(g, w):
    g, w = np.asarray(g, np.float64).reshape(-1), w.reshape(-1)
    ng, nw = np.linalg.norm(g), np.linalg.norm(w)
    return float(g @ w / (ng * nw)), float(ng / nw)


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('c', CASE_PARAMS)
def test_gradients_vs_twin64(c, route):
    """Bars (per gradient tensor t, e(x) = max|x - g64| / max|g64| after the ReLU flips K allows are taken out, see _grad_grid):
      fp32            e(gpu) <= 8 max(e(twin32), 2^-23): the reference's own float32 error on the same case sets the scale; 8 covers a
                      different summation order over reductions of up to 1024 terms (about sqrt(n) ulp)
      bf16x3 tight    e(gpu) <= 8 e(twin32) + 4 * 2^-16: four chained products of forward and backward, each within the 2^-16 split-bf16
                      product bound of kernels.h, norm-wise
      coarse          per-tensor cosine >= 0.9995 and |norm ratio - 1| <= 2e-2 (bf16x3), cosine >= 0.999 (plain bf16)
    Metrics (routes with use_tb=True): fp32 2e-5 relative + 1e-6; bf16x3 1e-4 relative + 1e-6; plain bf16 3e-2 (its documented drift)."""
    ag, m = run(c, route, False)
    # both twins take their actor step from the critic this run's optimiser step produced (Twin.update, critic_after)
    after = [p.cpu().numpy() for p in ag.critic.parameters()] if hasattr(ag, 'critic') else None
    r64 = G.run_twin(c, torch.float64, G.KINK_DELTA[c.precision], critic_after=after)
    r32 = G.run_twin(c, torch.float32, critic_after=after)
    tag = f'{G.case_id(c)} {route}'
    if route != 'fast':
        rel = {'fp32': 2e-5, 'bf16x3': 1e-4, 'bf16': 3e-2}[c.precision]
        assert sorted(m) == sorted(r64.metrics), (sorted(m), sorted(r64.metrics))
        worst_m = max(abs(m[k] - v) / (abs(v) + 1e-6 / rel) for k, v in r64.metrics.items())
        print(f'[grad grid] {tag}: worst metric error / (|v| + {1e-6 / rel:.0e}) = {worst_m:.2e} (bar {rel:g})')
        for k, v in r64.metrics.items():
            assert abs(m[k] - v) <= rel * abs(v) + 1e-6 * (3e4 if c.precision == 'bf16' else 1), (tag, k, m[k], v)
    else:
        assert m == {}
    nets = {'actor': ag.actor, 'critic': getattr(ag, 'critic', None)}
    e_gpu_w = e_32_w = ratio_w = 0.0
    flips_gpu = flips_32 = 0
    cos_w, norm_w = 1.0, 0.0
    worst_at = ''
    for step, want in G.steps_of(r64):
        got = [g.cpu().numpy().reshape(w.shape) for g, w in zip(nets[step].grads(), want)]
        assert len(got) == len(want)
        for i, g in enumerate(got):
            assert np.all(np.isfinite(g)), f'{tag}: non-finite {step} gradient {i}'
        if c.bar == 'coarse':
            for i, (g, w) in enumerate(zip(got, want)):
                if not np.any(w):
                    assert not np.any(g), (tag, step, i)
                    continue
                cos, ratio = _cos_ratio(g, w)
                cos_w, norm_w = min(cos_w, cos), max(norm_w, abs(ratio - 1.0))
                e_gpu_w = max(e_gpu_w, float(np.abs(g - w).max() / np.abs(w).max()))
                if c.precision == 'bf16x3':
                    assert cos >= 0.9995 and abs(ratio - 1.0) <= 2e-2, (tag, step, i, cos, ratio)
                else:
                    assert cos >= 0.999, (tag, step, i, cos, ratio)
            continue
        kinks = r64.kinks[step]
        assert kinks is not None, f'{tag}: |K| = {r64.n_kinks[step]} exceeds the cap of a tight case'
        d_gpu, f_gpu = G.explain_kinks(got, want, kinks, G.KINK_FLOOR[c.precision], f'{tag} {step} gpu')
        d_32, f_32 = G.explain_kinks(dict(critic=r32.critic_grads, actor=r32.actor_grads)[step], want, kinks, G.KINK_FLOOR[c.precision], f'{tag} {step} twin32')
        flips_gpu, flips_32 = flips_gpu + f_gpu, flips_32 + f_32
        for i, (eg, e3) in enumerate(zip(G.tensor_errors(d_gpu, want), G.tensor_errors(d_32, want))):
            bar = 8.0 * max(e3, 2.0 ** -23) if c.precision == 'fp32' else 8.0 * e3 + 4.0 * 2.0 ** -16
            if eg / bar > ratio_w:
                ratio_w, worst_at = eg / bar, f'{step}[{i}]'
            e_gpu_w, e_32_w = max(e_gpu_w, eg), max(e_32_w, e3)
    K = ' '.join(f'|K_{s}|={n}' for s, n in r64.n_kinks.items())
    if c.bar == 'coarse':
        print(f'[grad grid] {tag}: coarse e(gpu) {e_gpu_w:.2e} worst cosine {cos_w:.6f} worst |norm ratio - 1| {norm_w:.2e} {K}')
    else:
        print(f'[grad grid] {tag}: tight e(gpu) {e_gpu_w:.2e} e(twin32) {e_32_w:.2e} worst e(gpu)/bar {ratio_w:.3f} at {worst_at or "-"} {K} '
              f'flips gpu {flips_gpu} twin32 {flips_32}')
    assert ratio_w <= 1.0, f'{tag}: e(gpu) is {ratio_w:.2f} x its bar at {worst_at} (e(gpu) {e_gpu_w:.2e}, e(twin32) {e_32_w:.2e})'


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('c', CASE_PARAMS)
def test_poisoned_scratch_is_not_read(c, route):
    """The same update on a second agent whose scratch (everything a step writes before it reads, and the padding between all
    sub-buffers) holds NaN bit patterns: parameters, gradients, target parameters and metrics bit-identical to the clean run. The
    workspace is zeroed at creation, so without this a read of scratch the step never wrote, or past the end of a buffer, returns
    0 or a stale finite value and goes unnoticed."""
    clean, m0 = run(c, route, False)
    dirty, m1 = run(c, route, True)
    tag = f'{G.case_id(c)} {route}'
    assert_bit_identical(state_of(clean), state_of(dirty), tag)
    assert m0.keys() == m1.keys() and all(m0[k] == m1[k] for k in m0), (tag, m0, m1)


def _arena(seed, B):
    from exorl_amd.engine import ReplayEngine
    from exorl_amd.replay_buffer import ArenaIterator
    O, A = 24, 6
    eng = ReplayEngine((O,), np.float32, A, 0, 4096, 64)
    eng.set_order([eng.append_episode(ep) for ep in _synth.synth_episodes(seed, [200, 300, 250], O, A)])
    eng.seed_philox(77)
    return eng, ArenaIterator(eng, B, 1, 0.99, 'philox')


@pytest.mark.parametrize('H,B', [pytest.param(128, 64, id='planes'), pytest.param(192, 72, id='in-gemm-split')])
def test_poisoned_scratch_is_not_read_through_the_captured_graph(H, B):
    """bf16x3 TD3+BC, sample + update replayed as one captured graph (use_tb=False, device sampler and device noise): scratch poisoned
    before the capture and again between two replays, against an agent that is never poisoned."""
    c = G.Case('td3_bc', 24, 6, H, B, 0, 'bf16x3', 0, 'tight', '')
    agents_ = []
    for poison in (False, True):
        torch.manual_seed(3)
        ag = make(c, False)
        e, it = _arena(9, B)
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
    assert_bit_identical(state_of(agents_[0][0]), state_of(agents_[1][0]), f'graph H={H} B={B}')
