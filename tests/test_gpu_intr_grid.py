"""One step of every reward-free module over the kernel dispatch grid of tests/_intr_grid.py, one IntrEngine per case at world_size 1,
against the float64 autograd twin (oracle/intr64.py): every gradient tensor, dobs_out, the reward row by row under the parameters the
engine's own step produced, the metrics, the state the step leaves (BatchNorm running statistics, RMS, Proto's queue rows, queue pointer,
picks and predictor_target) and the optimiser's wiring.
Three routes through the library:
  update    exorl_intr_update(train = 1)
  phased    the same step as its exorl_intr_update_phase phases: bit-identical to the single call
  train0    exorl_intr_update(train = 0) from the seeded parameters: the reward alone, parameters bit-unchanged (every kind but SMM, whose
            reward is made of its step's losses; Proto's prototypes come back normalised, as compute_intr_reward leaves them)
Bars (per tensor t, e(x) = max|x - x64| / max|x64| after the ReLU flips K allows are taken out, tests/_grad_grid.py):
  fp32, bf16x6   e(gpu) <= 8 max(e(twin32), 2^-23), for gradients, dobs_out and the reward column alike; a tensor the twin leaves exactly
                 0 must be exactly 0
  bf16x3         e(gpu) <= 8 e(twin32) + L 2^-16, L chained matrix products (_intr_grid.L_OF): kernels.h's per-product bound
  metrics        2e-5 relative + 1e-6 (fp32, bf16x6); 1e-4 relative + 1e-6 (bf16x3)
Each test prints one '[intr grid]' line; profiles/intr_grid.txt holds a run's."""
import numpy as np
import pytest
import torch

import _grad_grid as G
import _intr_grid as IG
from oracle import intr64

pytestmark = pytest.mark.gpu

CASE_PARAMS = [pytest.param(c, id=IG.case_id(c)) for c in IG.CASES]
LR = 1e-4
DOBS = {'icm': 'obs', 'icm_apt': 'obs', 'disagreement': 'obs', 'diayn': 'next_obs', 'aps': 'next_obs', 'smm': 'obs', 'proto': 'obs'}      # rnd: obs, on encodings only
N_TRAIN = {'rnd': 6, 'proto': 7}              # tensors Adam owns, where not all: RND's target and Proto's predictor_target follow them


def engine_of(c):
    from exorl_amd.engine import IntrEngine
    kw = {k: v for k, v in c.opts.items() if k not in ('layout', 'u')}
    m = IntrEngine(c.kind, c.O, c.A, c.H, c.B, rep_dim=c.R, lr=LR, precision=c.precision, **kw)
    p = IG.params(c)
    if c.kind == 'proto':                         # predictor_target starts as a copy of the predictor (proto.py:59)
        p = p + p[:2]
    assert m.num_tensors() == len(p), (m.num_tensors(), len(p))
    for i, w in enumerate(p):
        t = m.tensor(None, i)
        t.copy_(torch.from_numpy(w).reshape(t.shape))
    return m


def device_rows(c):
    """The case's rows on the device in the layout its row asks for: (tensors kept alive, positional arguments, keyword arguments)."""
    b = IG.batch(c)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t = dict(action=dev(b['action']), extr=dev(b['extr']), reward=torch.full((c.B,), float('nan'), device='cuda'))
    layout = c.opts.get('layout')
    kw = {}
    if layout == 'skill_cols':                    # [obs | skill] rows, the skill read in place
        t['obs'] = dev(np.concatenate([b['obs'], b['skill']], 1))
        t['next_obs'] = dev(np.concatenate([b['next_obs'], b['skill']], 1))
        kw.update(obs_ld=c.O + c.R, next_obs_ld=c.O + c.R, skill=t['next_obs'].data_ptr() + 4 * c.O, skill_ld=c.O + c.R)
        ptr = {k: t[k].data_ptr() for k in ('obs', 'next_obs')}
    elif layout == 'misaligned':                  # next_obs one float past a 16-byte boundary, row stride O + 1
        t['obs'] = dev(b['obs'])
        buf = torch.zeros(c.B * (c.O + 1) + 8, device='cuda')
        off = 1 + (-(buf.data_ptr() // 4)) % 4
        view = buf[off:off + c.B * (c.O + 1)].view(c.B, c.O + 1)
        view[:, :c.O] = dev(b['next_obs'])
        t['next_obs'] = buf
        ptr = dict(obs=t['obs'].data_ptr(), next_obs=view.data_ptr())
        assert ptr['next_obs'] % 16 == 4
        kw.update(next_obs_ld=c.O + 1)
    else:
        t['obs'], t['next_obs'] = dev(b['obs']), dev(b['next_obs'])
        ptr = {k: t[k].data_ptr() for k in ('obs', 'next_obs')}
        if b['skill'] is not None:
            t['skill'] = dev(b['skill'])
            kw.update(skill=t['skill'].data_ptr(), skill_ld=c.R)
    for k in ('eps', 'u'):                        # the randomness fed from outside: SMM's epsilon, Proto's Categorical uniforms
        if b.get(k) is not None:
            t[k] = dev(b[k])
            kw['cat_uniform'] = t[k].data_ptr()
    if c.kind in DOBS or c.opts.get('encoded'):
        t['dobs'] = torch.full((c.B, c.O), float('nan'), device='cuda')
        kw['dobs_out'] = t['dobs'].data_ptr()
    return t, (ptr['obs'], t['action'].data_ptr(), ptr['next_obs'], t['extr'].data_ptr(), t['reward'].data_ptr()), kw


def run(c, route, train=1):
    m = engine_of(c)
    t, a, kw = device_rows(c)
    before = m.flat().clone()
    if route == 'phased':
        phase = 0
        while m.update_phase(phase, *a, train, **kw) >= 0:
            phase += 1
    else:
        m.update(*a, train, **kw)
    torch.cuda.synchronize()
    n = m.num_tensors()
    n_train = N_TRAIN.get(c.kind, n)
    out = dict(flat_before=before, flat_after=m.flat().clone(),
               params=[m.tensor(None, i).cpu().numpy().astype(np.float64) for i in range(n)],
               grads=[m.tensor(None, i, 1).cpu().numpy().astype(np.float64) for i in range(n_train)],
               flat_grad=m.flat(1).clone(), reward=t['reward'].cpu().numpy().astype(np.float64), metrics=m.metrics_raw().astype(np.float64),
               rms=m.rms_state(), bn=None if m.bn is None else m.bn.cpu().numpy().astype(np.float64),
               dobs=t['dobs'].cpu().numpy().astype(np.float64) if 'dobs' in t else None, n_train=n_train)
    if c.kind == 'proto':
        out.update(queue=m.queue.cpu().numpy().astype(np.float64), queue_ptr=m.queue_ptr())
    return out


def rel_err(x, x64):
    d = float(np.abs(np.asarray(x, np.float64) - x64).max())
    s = float(np.abs(x64).max())
    return d / s if s > 0 else (0.0 if d == 0 else float('inf'))


def bar_of(c, e32):
    if c.precision == 'bf16x3':
        return 8.0 * e32 + IG.L_OF[c.kind] * 2.0 ** -16
    return 8.0 * max(e32, 2.0 ** -23)


class Worst:
    def __init__(self):
        self.e_gpu = self.e_32 = self.ratio = 0.0
        self.at = '-'

    def add(self, c, name, eg, e3):
        r = eg / bar_of(c, e3)
        if r > self.ratio:
            self.ratio, self.at = r, name
        self.e_gpu, self.e_32 = max(self.e_gpu, eg), max(self.e_32, e3)


def check_metrics(c, tag, got, want):
    rel = 1e-4 if c.precision == 'bf16x3' else 2e-5
    for slot, v in want.items():
        assert abs(got[slot] - v) <= rel * abs(v) + 1e-6, (tag, f'metric slot {slot}', got[slot], v)


def check_reward_and_state(c, tag, run_, tw64, tw32, r64, r32, m64, w, dec64=None):
    assert np.all(np.isfinite(run_['reward'])), f'{tag}: non-finite reward'
    w.add(c, 'reward', rel_err(run_['reward'], r64), rel_err(r32, r64))
    check_metrics(c, tag, run_['metrics'], m64)
    if c.kind in ('rnd', 'icm_apt', 'aps'):
        M, S, n = tw64.rms_state()
        M3, S3, _ = tw32.rms_state()
        gM, gS, gn = run_['rms']
        assert gn == n, (tag, 'rms n', gn, n)
        for name, g, x3, x in (('rms.M', gM, M3, M), ('rms.S', gS, S3, S)):
            w.add(c, name, rel_err([g], np.array([x])), rel_err([x3], np.array([x])))
    if c.kind == 'proto':
        P = c.opts['num_protos']
        assert run_['queue_ptr'] == tw64.queue_ptr, (tag, 'queue_ptr', run_['queue_ptr'], tw64.queue_ptr)
        q64 = tw64.queue.double().numpy()
        w.add(c, 'queue', rel_err(run_['queue'], q64), rel_err(tw32.queue.double().numpy(), q64))
        picks, margin = dec64['proto_picks']
        rows = run_['queue'][(tw64.queue_ptr - P) % q64.shape[0]:][:P]           # the rows this pass wrote: the engine's picks, read off them
        got = np.array([int(np.argmin(np.linalg.norm(tw64.last_z - r, axis=1))) for r in rows])
        sure = margin >= 1e-12               # below that the blocked double-precision walk may round across the boundary
        assert np.array_equal(got[sure], picks[sure]), (tag, 'picks', got, picks)
    if tw64.bn is not None:
        O = c.O
        mean, var, count = tw64.bn_state()
        mean3, var3, _ = tw32.bn_state()
        assert run_['bn'][2 * O] == count, (tag, 'num_batches_tracked', run_['bn'][2 * O], count)
        w.add(c, 'bn.running_mean', rel_err(run_['bn'][:O], mean), rel_err(mean3, mean))
        w.add(c, 'bn.running_var', rel_err(run_['bn'][O:2 * O], var), rel_err(var3, var))


def check_optimiser(c, tag, run_, tw):
    """Adam's first step, m_hat = g and v_hat = g^2: every trainable element moved by -lr g / (|g| + 1e-8), computed in float64 from the
    engine's own gradient, within lr 1e-4 + 2^-23 |p| (one float32 rounding of the stored parameter); everything else bit-unchanged."""
    p0 = IG.params(c)
    lrs = tw.lrs
    if c.kind == 'proto':
        # predictor_target is not Adam's: after the step it is its Polyak step towards the UPDATED predictor and nothing else (one fused
        # multiply-add pair in float32 on the stored value: 2 ulp)
        for after, want in zip(run_['params'][7:9], tw.proto_target_after(run_['params'][0:2])):
            assert np.all(np.abs(after - want.reshape(after.shape)) <= 2.0 ** -22 * np.abs(want.reshape(after.shape)) + 1e-12), f'{tag}: predictor_target is not its Polyak step'
        p0 = p0 + p0[:2]
    unit = lambda x: x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)
    for i, (after, w0) in enumerate(zip(run_['params'], p0)):
        w0 = np.asarray(w0, np.float64).reshape(after.shape)
        if i >= run_['n_train']:
            assert c.kind == 'proto' or np.array_equal(after, w0), f'{tag}: frozen tensor {i} moved'
            continue
        g, ulps = run_['grads'][i], 1.0
        if c.kind == 'proto' and i == 6:
            # normalize_protos rewrites the prototypes in place in front of the step and again in front of the reward pass: Adam moved the
            # normalised rows, and what is read back is normalised once more. Each normalisation is a float32 sum, sqrt and divide on
            # the stored value: 4 ulp for the two instead of the 1 of a stored parameter
            want, ulps = unit(unit(w0) - LR * g / (np.abs(g) + 1e-8)), 4.0
        else:
            want = w0 - lrs[i] * g / (np.abs(g) + 1e-8)
        bad = np.abs(after - want) > lrs[i] * 1e-4 + ulps * 2.0 ** -23 * np.abs(want)
        assert not bad.any(), f'{tag}: Adam moved {int(bad.sum())} elements of tensor {i} off -lr g / (|g| + eps) (worst {np.abs(after - want).max():.3e})'


@pytest.mark.parametrize('c', CASE_PARAMS)
def test_step_vs_twin64(c):
    tag = f'{IG.case_id(c)} update'
    got = run(c, 'update')
    r64, rew64, m64, dec64, tw64 = IG.run_twin(c, torch.float64, IG.KINK_DELTA[c.precision], params_after=got['params'])
    r32, rew32, _, _, tw32 = IG.run_twin(c, torch.float32, params_after=got['params'])
    kinks = r64.kinks['module']
    assert kinks is not None, f'{tag}: |K| = {r64.n_kinks["module"]} exceeds the cap'
    g_gpu = got['grads'] + ([got['dobs']] if got['dobs'] is not None else [])
    assert len(g_gpu) == len(r64.grads), (len(g_gpu), len(r64.grads))
    g_gpu = [g.reshape(w_.shape) for g, w_ in zip(g_gpu, r64.grads)]
    for i, g in enumerate(g_gpu):
        assert np.all(np.isfinite(g)), f'{tag}: non-finite gradient tensor {i}'
    d_gpu, f_gpu = G.explain_kinks(g_gpu, r64.grads, kinks, IG.KINK_FLOOR[c.precision], f'{tag} gpu')
    d_32, f_32 = G.explain_kinks(r32.grads, r64.grads, kinks, IG.KINK_FLOOR[c.precision], f'{tag} twin32')
    w = Worst()
    names = [f'grad[{i}]' for i in range(got['n_train'])] + (['dobs_out'] if got['dobs'] is not None else [])
    for name, eg, e3 in zip(names, G.tensor_errors(d_gpu, r64.grads), G.tensor_errors(d_32, r64.grads)):
        w.add(c, name, eg, e3)
    check_reward_and_state(c, tag, got, tw64, tw32, rew64, rew32, {**r64.metrics, **m64}, w, dec64)
    print(f'[intr grid] {tag}: e(gpu) {w.e_gpu:.2e} e(twin32) {w.e_32:.2e} worst e/bar {w.ratio:.3f} at {w.at} |K| {r64.n_kinks["module"]} '
          f'flips gpu {f_gpu} twin32 {f_32}')
    check_optimiser(c, tag, got, tw64)
    assert w.ratio <= 1.0, f'{tag}: e(gpu) is {w.ratio:.2f} x its bar at {w.at} (e(gpu) {w.e_gpu:.2e}, e(twin32) {w.e_32:.2e})'


@pytest.mark.parametrize('c', CASE_PARAMS)
def test_phases_are_the_single_call_bit_for_bit(c):
    a, b = run(c, 'update'), run(c, 'phased')
    tag = f'{IG.case_id(c)} phased'
    for k in ('flat_after', 'flat_grad'):
        assert torch.equal(a[k], b[k]), f'{tag}: {k} differs (max |d| = {float((a[k] - b[k]).abs().max()):.3e})'
    for k in ('reward', 'metrics'):
        assert np.array_equal(a[k], b[k]), f'{tag}: {k} differs'
    assert a['rms'] == b['rms'], tag
    for k in ('bn', 'dobs', 'queue', 'queue_ptr'):
        assert (a.get(k) is None and b.get(k) is None) or np.array_equal(a[k], b[k]), f'{tag}: {k} differs'
    print(f'[intr grid] {tag}: bit-identical to the single call')


@pytest.mark.parametrize('c', [p for p in CASE_PARAMS if p.values[0].kind in IG.TRAIN0])
def test_reward_only_vs_twin64(c):
    tag = f'{IG.case_id(c)} train0'
    got = run(c, 'update', train=0)
    if c.kind == 'proto':                 # normalize_protos is part of compute_intr_reward (proto.py:103-107): the prototypes are rewritten, normalised
        probe = engine_of(c)
        lo = (probe.tensor(None, 6).data_ptr() - probe.flat().data_ptr()) // 4
        hi = lo + probe.tensor(None, 6).numel()
        keep = torch.ones_like(got['flat_before'], dtype=torch.bool)
        keep[lo:hi] = False
        assert torch.equal(got['flat_before'][keep], got['flat_after'][keep]), f'{tag}: train = 0 changed parameters other than the prototypes'
        w0 = np.asarray(IG.params(c)[6], np.float64)
        want = w0 / np.linalg.norm(w0, axis=1, keepdims=True)
        assert np.all(np.abs(got['params'][6] - want) <= 2.0 ** -22 * np.abs(want)), f'{tag}: the prototypes are not their normalised rows'
    else:
        assert torch.equal(got['flat_before'], got['flat_after']), f'{tag}: train = 0 changed the parameters'
    r64, m64, dec64, tw64 = IG.run_twin_reward_only(c, torch.float64)
    r32, _, _, tw32 = IG.run_twin_reward_only(c, torch.float32)
    w = Worst()
    check_reward_and_state(c, tag, got, tw64, tw32, r64, r32, m64, w, dec64)
    print(f'[intr grid] {tag}: e(gpu) {w.e_gpu:.2e} e(twin32) {w.e_32:.2e} worst e/bar {w.ratio:.3f} at {w.at}')
    assert w.ratio <= 1.0, f'{tag}: e(gpu) is {w.ratio:.2f} x its bar at {w.at} (e(gpu) {w.e_gpu:.2e}, e(twin32) {w.e_32:.2e})'


def test_rnd_on_encodings_step_only():
    """train = 2 (the pixel agent's first run_update call): the optimiser step alone. Gradients, dobs_out and parameters are those of the
    train = 1 call bit for bit; the reward slot and the RMS are not touched."""
    c = next(c for c in IG.CASES if c.opts.get('encoded'))
    one, two = run(c, 'update', train=1), run(c, 'update', train=2)
    for k in ('flat_after', 'flat_grad'):
        assert torch.equal(one[k], two[k]), k
    assert np.array_equal(one['dobs'], two['dobs'])
    assert np.all(np.isnan(two['reward'])) and two['rms'] == (0.0, 1.0, 1e-4)
