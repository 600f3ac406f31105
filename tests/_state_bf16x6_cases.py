"""The gradient-grid cases of the state agents in bf16x6 precision (tests/test_gpu_state_bf16x6.py runs them on the GPU,
tests/test_state_bf16x6_abi.py qualifies the new ones on the CPU). Same columns as tests/_grad_grid.py's CASES.

Plane route (planes3_ok in csrc/agent.hip: 128 | H, 128 | B): the smallest shapes that reach the three-plane GEMM. Two reuse the data of
existing table cases; the seeds of the other five were searched once on the CPU exactly as _grad_grid.CASES' were (smallest seed >= the
round base 6000, 6100, ... for which twin32 and twin64 take identical discrete decisions with float64 margin >= 1e-4 and the near-kink set
at 2^-18 max|z| has at most 64 elements); the tests do not search.
Generic route (every other shape: gemm_kernel<EXORL_PREC_BF16X6>): five of the existing fp32 tight cases, run in bf16x6."""
import _grad_grid as G

NEW_PLANE_CASES = [
    G.Case('td3_bc', 24, 6, 128, 128, 0, 'bf16x6', 6000, 'tight', 'three-plane kernel, TD3+BC: one 128-row tile per problem'),
    G.Case('bc', 24, 6, 128, 128, 0, 'bf16x6', 6100, 'tight', 'three-plane kernel, BC: the only forward of the step on the offset half of the actor buffers'),
    G.Case('crr', 24, 6, 128, 128, 7, 'bf16x6', 6201, 'tight', 'three-plane kernel, CRR with 7 value samples: 896 rows of value forward'),
    G.Case('cql', 24, 6, 128, 128, 3, 'bf16x6', 6300, 'tight', 'three-plane kernel, CQL: 1280 critic rows'),
    G.Case('cql', 78, 12, 128, 1024, 3, 'bf16x6', 6400, 'tight', 'three-plane kernel, CQL: 10240 critic rows, the wgrad in accumulated 1024-row slabs'),
]
PLANE_CASES = [
    G.Case('td3', 17, 6, 128, 128, 0, 'bf16x6', 3101, 'tight', 'three-plane kernel on the data of the bf16x3 planes case of seed 3101'),
    G.Case('ddpg', 24, 6, 384, 1024, 0, 'bf16x6', 1105, 'tight', 'three-plane kernel, shared trunk (per-head dgrad launches, the second accumulating), H = 3 x 128, B = 1024'),
] + NEW_PLANE_CASES
_GENERIC = [('td3_bc', 100, 7), ('td3', 4, 1), ('ddpg', 192, 72), ('td3_bc', 320, 1000), ('cql', 100, 50)]
GENERIC_CASES = [next(c for c in G.CASES if c.precision == 'fp32' and (c.kind, c.H, c.B) == k)._replace(precision='bf16x6') for k in _GENERIC]
CASES = PLANE_CASES + GENERIC_CASES

# bf16x6 is held to fp32 mode's kink treatment
KINK_DELTA = G.KINK_DELTA['fp32']
KINK_FLOOR = G.KINK_FLOOR['fp32']


def on_plane_route(c):
    return c.H % 128 == 0 and c.B % 128 == 0
