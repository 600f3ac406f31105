"""Every derived weight image of a state agent (include/exorl_hip.h, exorl_weight_images: W0 transposed, W0 and W1 as one, two or three bf16
planes; of actor, critic and Polyak target) equals the image of its current fp32 source, bit for bit, after every writer has written it:
exorl_agent_params_changed (check A), then three optimiser steps on each route through the library (check B: the plain Adam launch, the
fused finalize + Adam launch eager and replayed from a captured graph, the three-plane conversion pass behind either, and the target halves
of each), then exorl_agent_params_changed over what the steps left, which must not change one byte of the workspace (check C). The
reference (tests/_weight_images.py) is built from the parameter tensors the engine hands out in the reference's order with integer
arithmetic; all comparisons are equality of bit patterns.

The engines are built directly (AgentEngine with the arguments the agent classes of tests/test_gpu_grad_grid.py::make pass) so that one
driver serves every kind, APS's successor-feature critic included, and the routes are the library's own entry points."""
import numpy as np
import pytest
import torch

import _grad_grid as G
import _state_bf16x6_cases as S
import _synth
import _weight_images as W

pytestmark = pytest.mark.gpu

ROUTES = ['metrics', 'fast', 'phased', 'graph', 'window', 'mixed']
# metrics  whole-step call, metrics on: partials reduced inside the optimiser launch (finalize_adam), metric kernels in the step
# fast     whole-step call, metrics off: the fused scalar-head path where the kind has one, finalize_adam
# phased   the four phases called one by one at world_size 1: finalize_grads + the plain Adam launch with its shadow writes
# graph    sample + whole step captured once and replayed three times
# window   the fast path with the metric window's kernels in the step
# mixed    one eager fast step, one phased step, one replayed step on ONE agent: each writer takes the images over from the last
WINDOW_KINDS = ('td3_bc', 'td3', 'ddpg')                           # the kinds exorl_agent_set_metric_window keeps on the fused path
GRAPH_KINDS = ('td3_bc', 'td3', 'ddpg', 'bc', 'crr', 'cql', 'aps')  # every kind's step is captured by exorl_agent_enable_graph
SF_DIM = {'aps': 5}
STEPS = 3


def _grid(table, kind, H, B, precision):
    return next(c for c in table if (c.kind, c.H, c.B, c.precision) == (kind, H, B, precision))


def _new(kind, O, A, H, B, n, precision, seed, why):
    return G.Case(kind, O, A, H, B, n, precision, seed, '', why)


CASES = [
    # ---- fp32: w0t is the only image; the index rules of its writers
    _grid(G.CASES, 'td3', 4, 1, 'fp32')._replace(why='smallest net; two trunks, two heads'),
    _grid(G.CASES, 'td3_bc', 100, 7, 'fp32')._replace(why='odd in_dim (5 and 6): W0 rows straddle the float4 groups of the Adam launch; A = 1 head tensors are no multiples of 4'),
    _grid(G.CASES, 'ddpg', 192, 72, 'fp32')._replace(why='shared trunk (n_trunks 1, n_heads 2); in_dim 33'),
    _grid(G.CASES, 'cql', 128, 72, 'fp32')._replace(why='actor nout = 18 > 16: the 32-slot bias block of finalize_adam_kernel in front of the W0 elements'),
    _new('bc', 11, 3, 192, 8, 0, 'fp32', 7000, 'no critic, no target: the writers without their target halves'),
    _grid(G.CASES, 'crr', 100, 50, 'fp32')._replace(why="CRR's step order"),
    _new('aps', 14, 2, 136, 8, 0, 'fp32', 7100, 'critic out_dim = sf_dim 5 (observation 9 + task 5): wide head tensors in front of the second head'),
    # ---- plain bf16: one plane of W0 and W1
    _new('td3', 17, 6, 192, 8, 0, 'bf16', 7200, 'hi planes written; H = 192 keeps the trunk off the MFMA kernel; in_dim 17 and 23: 15 and 9 padding columns'),
    _new('td3_bc', 24, 8, 128, 8, 0, 'bf16', 7300, 'critic in_dim 32: no K padding; actor in_dim 24: 8 padding columns'),
    _new('ddpg', 24, 9, 256, 64, 0, 'bf16', 7400, 'in_dim 33 -> 64 columns: 31 padding columns per row'),
    # ---- bf16x3 on the plane pipeline: hi + lo of W1, W0 and the target's, W1's leaving as packed 16-byte stores
    _grid(G.CASES, 'td3_bc', 128, 64, 'bf16x3')._replace(why='hi + lo, twin critic'),
    _grid(G.CASES, 'ddpg', 256, 64, 'bf16x3')._replace(why='hi + lo, shared trunk, in_dim 33 -> 64'),
    _grid(G.CASES, 'cql', 128, 64, 'bf16x3')._replace(why='hi + lo, CQL: 12-wide actor head'),
    _grid(G.CASES, 'crr', 128, 64, 'bf16x3')._replace(why="hi + lo, CRR's step order"),
    _grid(G.CASES, 'bc', 128, 64, 'bf16x3')._replace(why='hi + lo, no critic'),
    _grid(G.CASES, 'td3_bc', 100, 7, 'bf16x3')._replace(why='in-GEMM split: w0t only, every plane pointer NULL'),
    # ---- bf16x6: three planes of W1 from the conversion pass behind the optimiser, for actor, critic AND target; no W0 planes
    _grid(S.CASES, 'td3_bc', 128, 128, 'bf16x6')._replace(why='hi + mid + lo of W1, twin critic'),
    _new('ddpg', 24, 6, 128, 128, 0, 'bf16x6', 7500, 'hi + mid + lo of W1, shared trunk'),
    _new('td3', 24, 6, 64, 128, 0, 'bf16x6', 7600, 'H = 64: off the plane route, w0t only'),
]
# the case that also runs the teeth check (on route `fast`), one per precision
TEETH = {'fp32': 'td3_bc-O5A1H100B7-fp32', 'bf16': 'td3_bc-O24A8H128B8-bf16', 'bf16x3': 'td3_bc-O24A6H128B64-bf16x3',
         'bf16x6': 'td3_bc-O24A6H128B128-bf16x6'}
assert all(sum(G.case_id(c) == v for c in CASES) == 1 for v in TEETH.values())


def runs(c, route):
    """The explicit table of what does not run: the metric window belongs to three kinds; a kind without a captured step has no graph."""
    k = G.base_kind(c)
    if route == 'window':
        return k in WINDOW_KINDS
    if route in ('graph', 'mixed'):
        return k in GRAPH_KINDS
    return True


PARAMS = [pytest.param(c, r, id=f'{G.case_id(c)}-{r}') for c in CASES for r in ROUTES if runs(c, r)]


def make_engine(c):
    from exorl_amd.engine import AgentEngine
    k = G.base_kind(c)
    return AgentEngine(k, c.O, c.A, c.H, c.B, lr=1e-4, tau=0.01, alpha=0.01 if k == 'cql' else 2.5, stddev_clip=0.0 if k == 'cql' else 0.3, precision=c.precision,
                       num_value_samples=c.n or 10, weight_func='indicator', n_samples=c.n or 3, sf_dim=SF_DIM.get(k, 0))


def seeded_params(c):
    from oracle.agents import param_shapes
    k = G.base_kind(c)
    ash, csh = param_shapes(k, c.O, c.A, c.H, SF_DIM.get(k))
    pa = list(_synth.synth_params(ash, c.seed).values())
    pc = list(_synth.synth_params(csh, c.seed + 1).values()) if csh else None
    return pa, pc


def nets_of(eng):
    from exorl_amd import _lib as L
    return [('actor', L.NET_ACTOR)] + ([('critic', L.NET_CRITIC), ('critic_target', L.NET_CRITIC_TARGET)] if eng.has_critic else [])


def load(eng, net, arrays):
    assert eng.num_tensors(net) == len(arrays)
    for i, w in enumerate(arrays):
        t = eng.tensor(net, i)
        t.copy_(torch.from_numpy(w).reshape(t.shape))


def read_params(eng, net):
    return [eng.tensor(net, i).cpu().numpy() for i in range(eng.num_tensors(net))]


def read_images(eng, net):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in eng.weight_images(net).items()}


def compare(eng, c, sources=None):
    """{net name: [names of the images that differ from the image of the net's fp32 source]} with a description of the first difference
    of each; sources: {net name: arrays} to compare against instead of the engine's current parameters. Also holds the carve table:
    which images exist follows from precision, hidden_dim and batch alone."""
    torch.cuda.synchronize()
    p0, p1 = W.planes_for(c.precision, c.H, c.B)
    bad, detail = {}, []
    for name, net in nets_of(eng):
        got = read_images(eng, net)
        have = sorted(k for k, v in got.items() if v is not None)
        want_have = sorted(['w0t'] + ['w0_hi', 'w0_lo'][:p0] + {0: [], 1: ['w1_hi'], 2: ['w1_hi', 'w1_lo'], 3: ['w1_hi', 'w1_mid', 'w1_lo']}[p1])
        assert have == want_have, f'{name}: the configuration carves {have}, the header says {want_have}'
        tensors = sources[name] if sources else read_params(eng, net)
        nt, nh = got['w0t'].shape[0], (2 if name != 'actor' else 1)
        want = W.expected_images(tensors, (nt, nh), (p0, p1))
        in_dim = got['w0t'].shape[1]
        for k in ('w0_hi', 'w0_lo'):
            if got[k] is not None:
                assert not got[k][:, :, in_dim:].any(), f'{name}.{k}: a K-padding column is not zero'
        bad[name] = W.differing(got, want)
        detail += [f'{name}.{k}: {W.first_difference(got, want, k)}' for k in bad[name]]
    return bad, detail


def assert_images(eng, c, tag, sources=None):
    bad, detail = compare(eng, c, sources)
    assert not any(bad.values()), f'{tag}: ' + '; '.join(detail)


_arena_eps = {}


def arena(c):
    from exorl_amd.engine import ReplayEngine
    eps = _arena_eps.setdefault((c.O, c.A), _synth.synth_episodes(9, [200, 300, 250], c.O, c.A))
    r = ReplayEngine((c.O,), np.float32, c.A, 0, 4096, 64)
    r.set_order([r.append_episode(ep) for ep in eps])
    r.seed_philox(77)
    return r


class Driver:
    """The steps of one route on one engine; noise comes from the device's Philox stream."""

    def __init__(self, eng, c):
        self.eng, self.c, self.i, self.replay = eng, c, 0, None
        self.stddev = 1.0 if G.base_kind(c) == 'cql' else 0.2

    def _batch(self):
        c = self.c
        self.eng.set_batch(*_synth.synth_batch(c.seed + 2, self.i, c.B, c.O, c.A))
        self.i += 1

    def whole(self, metrics):
        self.eng.set_metrics(metrics)
        self._batch()
        self.eng.update(self.stddev)

    def phased(self):
        self.eng.set_metrics(True)
        self._batch()
        for ph in range(4):
            self.eng.update_phase(ph, self.stddev)

    def capture(self):
        self.eng.set_metrics(False)
        self.replay = arena(self.c)
        self.eng.enable_graph(self.replay, 1, 0.99, self.stddev)

    def replayed(self):
        self.eng.step_graph(self.stddev)
        self.i += 1

    def run(self, route):
        if route in ('metrics', 'fast'):
            for _ in range(STEPS):
                self.whole(route == 'metrics')
        elif route == 'phased':
            for _ in range(STEPS):
                self.phased()
        elif route == 'window':
            self.eng.set_metric_window()
            for _ in range(STEPS):
                self.whole(False)
        elif route == 'graph':
            self.capture()
            for _ in range(STEPS):
                self.replayed()
        else:
            assert route == 'mixed'
            self.whole(False)
            self.phased()
            self.capture()
            self.replayed()
        torch.cuda.synchronize()
        steps = self.eng.opt_steps()
        assert steps == (STEPS, STEPS if self.eng.has_critic else 0), steps


def flip(t, index):
    """Writes, at `index` of the parameter view `t`, a value whose hi, mid and lo planes all differ from the old value's."""
    old = np.float32(t[index].item())
    for v in (1.2345678, -0.7654321, 0.3141592):
        v = np.float32(v)
        if all(a != b for a, b in zip(W.planes(np.array([old]), 3), W.planes(np.array([v]), 3))):
            t[index] = float(v)
            return
    raise AssertionError(old)


def teeth(eng, c, tag):
    """One element each of critic W0, target W1 and actor W1 written through the parameter views WITHOUT params_changed: the comparator
    has to name exactly the images of those three tensors that the configuration has; after params_changed it passes again."""
    from exorl_amd import _lib as L
    H = c.H
    flip(eng.tensor(L.NET_CRITIC, 0), (H - 1, 2))                  # critic trunk 0, W0
    flip(eng.tensor(L.NET_CRITIC_TARGET, 12), (1, H - 2))          # target head 1, W1 (twin critic: [trunk 0, head 0, trunk 1, head 1])
    flip(eng.tensor(L.NET_ACTOR, 4), (H // 2, 3))                  # actor W1
    p0, p1 = W.planes_for(c.precision, c.H, c.B)
    w1 = {0: [], 1: ['w1_hi'], 2: ['w1_hi', 'w1_lo'], 3: ['w1_hi', 'w1_mid', 'w1_lo']}[p1]
    stale = {n: read_images(eng, net) for n, net in nets_of(eng)}
    want = {'critic': ['w0t'] + ['w0_hi', 'w0_lo'][:p0], 'critic_target': w1, 'actor': w1}
    got = {n: W.differing(stale[n], W.expected_images(read_params(eng, net), (stale[n]['w0t'].shape[0], 1 if n == 'actor' else 2), (p0, p1)))
           for n, net in nets_of(eng)}
    assert got == want, f'{tag}: the comparator reports {got} for three stale tensors, expected {want}'
    eng.params_changed(sync_target=False)
    assert_images(eng, c, f'{tag} after the teeth check')


@pytest.mark.parametrize('c,route', PARAMS)
def test_weight_images_equal_their_source(c, route):
    tag = f'{G.case_id(c)} {route}'
    eng = make_engine(c)
    pa, pc = seeded_params(c)
    from exorl_amd import _lib as L
    load(eng, L.NET_ACTOR, pa)
    if pc:
        load(eng, L.NET_CRITIC, pc)
    eng.params_changed(sync_target=True)
    # A: the refresh kernels, from the arrays just loaded (the target's source is the critic's arrays)
    assert_images(eng, c, f'{tag} check A', {'actor': pa, 'critic': pc, 'critic_target': pc})
    # B: whatever the route's optimiser launches left, against the parameters they left
    Driver(eng, c).run(route)
    if pc:
        moved = [bool((torch.from_numpy(w).reshape(-1) != eng.tensor(L.NET_CRITIC_TARGET, i).cpu().reshape(-1)).any()) for i, w in enumerate(pc)]
        assert moved[0] and moved[4], f'{tag}: the Polyak target did not move'
    assert_images(eng, c, f'{tag} check B')
    # C: a refresh over the same parameters rewrites every image with the bytes it already holds
    before = eng.workspace.clone()
    eng.params_changed(sync_target=False)
    torch.cuda.synchronize()
    same = torch.equal(before, eng.workspace)
    assert same, f'{tag} check C: params_changed changed {int((before != eng.workspace).sum())} bytes, first at {int((before != eng.workspace).nonzero()[0])}'
    if route == 'fast' and TEETH[c.precision] == G.case_id(c):
        teeth(eng, c, tag)


def test_export_refuses_a_net_the_agent_lacks():
    """The argument checks that need a created agent (the NULL checks are in tests/test_weight_images_abi.py)."""
    from exorl_amd import _lib as L
    eng = make_engine(next(c for c in CASES if c.kind == 'bc'))
    for net in (L.NET_CRITIC, L.NET_CRITIC_TARGET, 3, -1):
        with pytest.raises(L.ExorlError, match=f'debug_agent_weight_images: agent has no net {net}'):
            eng.weight_images(net)
    assert sorted(eng.weight_images(L.NET_ACTOR)) == sorted(W.IMAGES)
