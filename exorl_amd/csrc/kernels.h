// Internal C++ interface between the kernel translation units of libexorl_hip.so.
#pragma once
#include <vector>

#include "numerics.h"

namespace exorl {

struct TensorDesc { int64_t off, rows, cols; };      // one parameter tensor inside a flat buffer (floats), torch shape rows x cols

// Lays sub-buffers out in one workspace, each padded to 64 floats; base == nullptr -> sizing pass.
struct SimpleCarver {
    float* base; int64_t off = 0;
    explicit SimpleCarver(float* b) : base(b) {}
    float* take(int64_t n) { float* p = base ? base + off : nullptr; off += round_up(n, 64); return p; }
};

// The bf16 images of one fp32 buffer, same shape and pitch: hi = bf16(x) alone (plain bf16), hi + lo with lo = bf16(x - hi) (bf16x3 on the
// plane pipeline), or hi + mid + lo = the 24 significand bits of x (bf16x6 on the plane route). A plane the precision does not use is null.
struct Planes {
    unsigned short *hi = nullptr, *mid = nullptr, *lo = nullptr;
    __host__ __device__ Planes at(int64_t off) const { return Planes{hi ? hi + off : nullptr, mid ? mid + off : nullptr, lo ? lo + off : nullptr}; }
    __host__ __device__ explicit operator bool() const { return hi != nullptr; }
};

struct GemmProblem {
    const float* A;
    const float* B;
    float* C;
    const float* bias;
    int M, N, K;
    int64_t lda, ldb, ldc;
};
int gemm_grouped(int precision, int a_layout, int b_layout, const GemmProblem* probs, int count, bool relu,
                 bool accumulate, hipStream_t s);
// bf16x3's plane adapter inside a stream capture (off by default: such launches take the generic kernel). allow: launches captured from now on
// take the adapter where its scratch arena is large enough already; probe (optional) receives the largest arena size they ask for.
// gemm_planes_reserve grows the arena to `bytes` (synchronises; never while capturing).
void gemm_planes_capture(bool allow, size_t* probe);
int gemm_planes_reserve(size_t bytes);

struct Gemm16Problem {
    const unsigned short* A;
    const unsigned short* B;
    float* C;
    const float* bias;
    int M, N, K;
    int64_t lda, ldb, ldc;
    // split-bf16 ("bf16x3") operands: x = hi + lo with hi = bf16(x), lo = bf16(x - hi); the product is formed as
    // hi*hi + hi*lo + lo*hi in fp32 accumulators (relative error ~2^-16: per-step losses stay within 1e-4 of the fp32 reference)
    const unsigned short* A_lo = nullptr;
    const unsigned short* B_lo = nullptr;
    // Scalar head folded into the epilogue (the 128 x TN "p" kernels only; forward launches with relu): instead of storing C the workgroup leaves,
    // per output row, the dot of relu(acc + bias) with head_w over each wave's column block: head_part[row][column block] (N / (TN / 2) floats per
    // row, gemm16_head_slots() says how many). For a net whose hidden activations nobody reads again — the Polyak target critic of a TD step.
    const float* head_w = nullptr;
    float* head_part = nullptr;
    // > 0 (the 128 x TN "p" kernels only; a multiple of 4): only columns [0, n_store) of C exist — N is the padded width of the operand planes.
    // The planes adapter uses it for outputs whose width is not a multiple of the tile (39200-wide module layers) instead of a padded C + copy.
    int n_store = 0;
    // three-plane split-bf16 ("bf16x6") operands: x = hi + mid + lo with hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid), i.e. the 24
    // significand bits of an fp32 value (a Planes with all three set). A problem with mid planes carries A_lo / B_lo as its third planes —
    // Planes::lo is the last plane of a two-plane and of a three-plane image alike; the product is formed as hi*hi,
    // hi*mid + mid*hi, hi*lo + lo*hi + mid*mid in three fp32 accumulators summed small-first (mid*lo, lo*mid, lo*lo are dropped: relative error
    // <= 3 * 2^-24 of |a||b|). One kernel takes such a launch (gemm16p, TN = 64): M % 128, N % 64, K % 128 = 0, 16-byte aligned planes, C and bias.
    const unsigned short* A_mid = nullptr;
    const unsigned short* B_mid = nullptr;
};
// fp32 (rows x cols, pitch ld) -> three bf16 planes of rows_p x cols_p (>= rows x cols, cols_p % 8 = 0; the padding is written as zeros), for
// `nb` images `src_stride` floats / `dst_stride` bf16 apart (the heads of a net share a launch). gemm.hip, to_planes3_kernel.
int to_planes3(const float* src, int64_t ld, int rows, int cols, unsigned short* hi, unsigned short* mid, unsigned short* lo, int rows_p, int cols_p,
               int nb, int64_t src_stride, int64_t dst_stride, hipStream_t s);
// slots per row the "p" kernels would write for these problems' head_part (N / wave column block), or 0 when the launch would not take them
int gemm16_head_slots(const Gemm16Problem* probs, int count);
// operands stored as bf16 in memory (fast mode); same layout conventions as gemm_grouped
int gemm16_grouped(int a_layout, int b_layout, const Gemm16Problem* probs, int count, bool relu, bool accumulate, hipStream_t s);
// wgrad (a_layout 1) and dgrad (a_layout 0) problems of one backward pass in a single launch; b_layout 1, plain store
int gemm16_grouped_mixed(const int* a_layouts, const Gemm16Problem* probs, int count, hipStream_t s);

// ---- row-wise / column-wise layer kernels (rowops.hip). `nets` independent nets are processed by one
// launch (blockIdx.y); a* strides are in floats between nets for activations, p* for parameters.
int ln_tanh_fwd(const float* z, const float* gain, const float* beta, float* h, float* xhat, float* rstd,
                int rows, int H, int nets, int64_t astride, int64_t pstride, hipStream_t s);
int ln_tanh_bwd(const float* dh, const float* h, const float* xhat, const float* rstd, const float* gain, float* dz,
                int rows, int H, int nets, int64_t astride, int64_t pstride, hipStream_t s);
int ln_param_grad(const float* dh, const float* h, const float* xhat, float* dgain, float* dbeta,
                  int rows, int H, int nets, int64_t astride, int64_t pstride, hipStream_t s);
int colsum(const float* x, float* out, int rows, int cols, int nets, int64_t astride, int64_t pstride, hipStream_t s);
// fused ReLU backward + column sum (0 = done; 1 = shapes need relu_bwd + colsum separately)
int relu_bwd_colsum(float* x, const float* act, float* out, int rows, int cols, hipStream_t s);
// out = x W^T + b with the reduction cut into `splits` slabs in one grouped launch (scratch: splits x rows x F floats), summed in slab order
int linear_splitk(int prec, const float* x, int64_t ldx, const float* W, const float* b, float* out, int rows, int F, int K, float* scratch,
                  int splits, hipStream_t s);
int head_fwd(const float* a, const float* W, const float* b, float* out, int rows, int H, int nout, int tanh_out,
             int nets, int64_t astride, int64_t pstride, int64_t ostride, hipStream_t s);

// ---- fused layer kernels (fused.hip)
int trunk_fwd(const float* x, int64_t ldx, const float* W0T, const float* b0, const float* gain, const float* beta,
              float* h, float* xhat, float* rstd, unsigned short* h_bf16, unsigned short* xhat_bf16, int rows, int in_dim,
              int H, int nets, int64_t astride, int64_t pstride, int64_t tstride, hipStream_t s);
// per-net operands of one trunk / scalar head, so that nets whose parameters live in different buffers (critic and its Polyak
// target) share a launch
// W0l / hl / xhl: lo planes of the split-bf16 mode (x = hi + lo); null in plain bf16 mode
struct TrunkItem { const float* x; const unsigned short* W0b; const float *b0, *gain, *beta; float* rstd; unsigned short *hb, *xhb;
                   const unsigned short* W0l; unsigned short *hl, *xhl; };
struct TrunkBatch { TrunkItem it[4]; };
int trunk_fwd16_batch(const TrunkBatch& tb, int count, int64_t ldx, int rows, int in_dim, int H, hipStream_t s);
struct HeadItem { const float* a; const float* W; const float* b; float* out; };
struct HeadBatch { HeadItem it[4]; };
int head_fwd1_batch(const HeadBatch& hb, int count, int rows, int H, hipStream_t s);
// MFMA variant for the bf16 fast mode (H % 128 == 0): W0b = bf16 shadow [nets][H][round_up(in_dim, 32)], zero padded
bool trunk_fwd16_supported(int H);
// W0q, hq, xhatq: hi planes, and lo planes in split-bf16 mode (x = hi + lo); xhatq empty -> h only (nobody runs a backward pass over it)
int trunk_fwd16(const float* x, int64_t ldx, const Planes& W0q, const float* b0, const float* gain, const float* beta, float* rstd,
                const Planes& hq, const Planes& xhatq, int rows, int in_dim, int H, int nets, int64_t astride, int64_t pstride, hipStream_t s);
// hq, xhatq: both empty -> reads the fp32 h / xhat; otherwise the bf16 images (hi, or hi + lo) in their place
int ln_bwd(float* dh, const float* h, const float* xhat, const Planes& hq, const Planes& xhatq, const float* rstd, const float* gain, float* P,
           int rows, int H, int nets, int64_t astride, int64_t pstride, int want_params, hipStream_t s, const float* w0t, int64_t tstride,
           float* dx, int dx_cols, const float* beta);
int trunk_chunks(int rows);
// k smallest L2 distances of every src row to the tgt rows (at most 8192), ascending (knn.hip); d2 = scratch of knn_scratch_floats(n_src, n_tgt)
// floats: n_src x round_up(n_tgt, 64) up to 4096 targets, at most 1024 such rows above
int64_t knn_scratch_floats(int n_src, int n_tgt);
int knn_topk(const float* src, int n_src, const float* tgt, int n_tgt, int dim, int k, float* out, float* d2, hipStream_t s);
int outer_reduce(const float* u, int64_t ldu, int J, const float* v, float* P, int rows, int H, int nets, int64_t vstride,
                 hipStream_t s);
int outer_chunks(int rows);
// Optional epilogue of the actor head on the stacked [next_obs; obs] batch: the two TruncatedNormal draws of a DDPG-family
// step (rows < B -> next_action into dst_next, rows >= B -> pi(obs) sample into dst_pi), td3_bc.py:125,151 — saves the
// separate sampling kernel. noise_* null -> Philox(seed, *counter_ptr + half).
struct SampleSpec {
    const float* stddev_ptr;   // device-resident exploration std (StepState::stddev); null -> the `stddev` value below
    const float *noise_c, *noise_a;
    uint64_t seed;
    const uint64_t* counter_ptr;
    float stddev, clip;
    float *dst_next, *dst_pi;
    int64_t dst_ld;
    int B;
};
int head_fwd4(const float* a, const float* W, const float* b, float* out, int rows, int H, int nout, int tanh_out,
              int nets, int64_t astride, int64_t pstride, int64_t ostride, hipStream_t s, const SampleSpec* sample = nullptr);
// Where head_bwd takes d(loss)/d(head output) from: a buffer, or computed on the fly from the loss definition so that
// the (B,1)/(B,A)-sized loss kernels need not sit between the forward and the backward pass.
#define EXORL_DOUT_BUFFER   0
#define EXORL_DOUT_TD       1   /* 2 (q_net - (r + D min(tq1,tq2))) * inv_bg                    td3_bc.py:127-131 */
#define EXORL_DOUT_ACTOR_Q  2   /* -lambda * inv_bg * [q_net is the min] (0.5 on ties)            td3_bc.py:152-155 */
#define EXORL_DOUT_CQL_ACTOR 4  /* tanh-Gaussian actor, 2A outputs: reparameterised (alpha*log_pi - Q).mean()   cql.py:236-255 */
#define EXORL_DOUT_ACTOR_MU 3   /* (sum_t da_t + bc term) * (1 - mu^2)  /  BC: -(a-mu)/std^2*inv_bg td3_bc.py:155, bc.py:83 */
// The form of the actor's loss, which is all head_bwd, actor_dmu and metrics_window ask of an agent kind. The values are those of the agent kinds
// the kernels compared against before the form had a name of its own (TD3+BC 0, TD3 1, BC 2, CRR 4), so the device code is what it was,
// instruction for instruction; a kernel parameter that carries a form stays `int`, which keeps the kernel's symbol.
enum ActorLoss : int {
    ACTOR_LOSS_Q_BC = 0,     // -lambda Q(s, mu) + (mu - a)^2                            td3_bc.py:152-155
    ACTOR_LOSS_Q = 1,        // -Q(s, mu)                                                td3.py, ddpg.py
    ACTOR_LOSS_BC = 2,       // -log N(a; mu, std)                                       bc.py:83
    ACTOR_LOSS_WLL = 4,      // -w log N(a; mu, std), w per row: CRR's and IQL's         crr.py:185-186
};
struct DoutSpec {
    int mode;
    union {
        const float* buf;    // BUFFER: (nets, rows, nout)
        // `buf` must stay null in ACTOR_MU mode: there a non-null value is bc_part and selects head_bwd's metrics variant (net_backward),
        // which writes through it
        float* bc_part;      // ACTOR_MU, TD3+BC, metrics variant (head_bwd's `metrics`): per-chunk sum (mu - a_data)^2 out, head_chunks(rows) floats
    };
    const float *q, *tq, *reward, *discount;   // TD / ACTOR_Q: q, tq are (2, rows)
    const float* stats;      // ACTOR_Q: stats[0] = sum |Q| over the global batch
    const float *da, *mu, *a_data;             // ACTOR_MU: da (da_nets, rows, nout), mu / a_data (rows, nout)
    const float* w;          // ACTOR_MU, CRR: per-sample advantage weight (rows)
    const float *raw, *z;    // CQL_ACTOR: actor head outputs (rows, 2A) [mu_raw | log_std_raw]; rsample noise (rows, A) or null
    const float* alpha_ptr;  // CQL_ACTOR: exp(log_actor_alpha) after its optimiser step (device scalar)
    uint64_t seed, counter; const uint64_t* counter_ptr;   // Philox identity of z when z == nullptr
    const float* task;       // TD / ACTOR_Q with a successor-feature critic (aps.py:50-58): dQ/d(feature j) = task[m][j]
    int64_t task_ld;
    const float* lam_parts;  // ACTOR_MU after qhead(ACTOR): per-chunk [sum |min Q|, sum min Q]; lambda = alpha / mean|Q| is applied here
    int lam_chunks;          //   (the critic backward is linear in its output gradient, so it ran with lambda = 1)
    int da_nets;
    ActorLoss form;          // ACTOR_MU: which terms d L / d mu has
    int use_lambda;
    float inv_bg, alpha, stddev;
    const float* stddev_ptr;   // BC / CRR: device-resident std (StepState::stddev); null -> `stddev`
};
// dz (fp32) and / or dzq (hi, or hi + lo) receive the gradient at the hidden layer: whichever is non-null
// metrics: ACTOR_MU of TD3+BC also leaves per-chunk sums of (mu - a_data)^2 in dspec.bc_part (one net)
int head_bwd(const DoutSpec& dspec, const float* W, const float* a, float* dz, const Planes& dzq, float* P, int rows,
             int H, int nout, int nets, int64_t astride, int64_t pstride, int want_params, hipStream_t s, bool metrics = false);
int head_chunks(int rows);
int tune_variant();      // exorl_gemm_tune's bits (0 = defaults): the reference paths below, each read at one decision point
constexpr int TUNE_CONV_WGRAD_TILE = 64;             // 32 -> 32 conv weight gradient on the tile kernel, not conv_wgrad_ws_kernel
constexpr int TUNE_ACT_GENERIC = 256;                // act() on the generic multi-launch path
constexpr int TUNE_CONV_PER_IMAGE = 8388608;         // wave-specialised conv forward / dgrad: one image per workgroup, not the persistent form
constexpr int TUNE_ADAPTER_PADDED = 134217728;       // planes adapter: ragged widths through the padded copy
constexpr int TUNE_CONV_STRIP = 1073741824;          // 32 -> 32 conv forward / dgrad on the strip kernel, not conv3x3_ws_kernel
int prec_override_mask();    // exorl_debug_precision_override's bits (0 = none; diagnostic)
// Scalar critic heads, forward and backward in one kernel (single-GPU whole-step path, no metrics): Q1,Q2 (and the target's
// Q1',Q2') row dots, the loss gradient at the head output, dz2 = dQ * W2 * [h2 > 0] and the per-chunk parameter partials.
//   mode 0 (critic step, td3_bc.py:126-131): dQ_n = 2 (Q_n - (r + D min(Q1',Q2'))) * inv_bg
//   mode 1 (actor step, td3_bc.py:152-155):  dQ_n = -inv_bg * [Q_n is the min] (0.5 on ties); per-chunk sum|min Q|, sum min Q -> abs_part
struct QHeadArgs {
    const float* a[4];       // h2 rows of critic net 0, 1 and (mode 0) target net 0, 1
    const float* W[4];
    const float* b[4];
    float *q, *tq;           // (2, rows) outputs
    const float *reward, *discount;
    float* dz; unsigned short* dzb; unsigned short* dzl; int64_t act;     // dzl: lo plane (split-bf16) or null
    float* P;                // head partials [net][chunk][(1+1)H + 16] or null
    float* abs_part;         // mode 1: [chunk][2]; mode 0 with `metrics`: [chunk][6] = sum r, y, q1, q2, (q1 - y)^2, (q2 - y)^2 (y = r + D min(Q1', Q2'))
    const float* tpart[2];   // mode 0, folded target heads: per row `tslots` partial dots of target net 0 / 1 (gemm16 head_part) instead of a[2], a[3]
    int tslots;
    int rows, H, mode;
    float inv_bg;
};
// metrics (windowed metrics on the fused path): mode 0 also leaves the critic metrics' per-chunk sums in abs_part
int qhead(const QHeadArgs& q, hipStream_t s, bool metrics = false);
int qhead_chunks(int rows);     // partial rows qhead writes per net (finer than head_chunks)
// Per-chunk partials are summed in chunk order by one thread per element (finalize_grads, finalize_adam, metrics_window).
// sum of n partials spaced `stride` apart, 16 loads in flight
__device__ __forceinline__ float chunk_sum(const float* __restrict__ p, int n, int64_t stride) {
    float acc = 0.f;
    int ch = 0;
    if (n > 1024) {          // thousands of partials (8192 rows and more): sub-sums of 32 added to a second accumulator. One running float32 sum
        for (; ch + 32 <= n; ch += 32) {        // of n terms drifts by about sqrt(n) ulp of the total: 2050 qhead partials at B = 8200 left
            float t[32], sub = 0.f;             // a bias gradient 1.1e-6 off its float64 value, where the float32 reference is 4e-8 off
#pragma unroll
            for (int q = 0; q < 32; ++q) t[q] = p[(int64_t)(ch + q) * stride];
#pragma unroll
            for (int q = 0; q < 32; ++q) sub += t[q];
            acc += sub;
        }
    }
    for (; ch + 32 <= n; ch += 32) {            // 32 in flight: the 256 qhead chunks are 8 dependent rounds instead of 16 (same order of adds)
        float t[32];
#pragma unroll
        for (int q = 0; q < 32; ++q) t[q] = p[(int64_t)(ch + q) * stride];
#pragma unroll
        for (int q = 0; q < 32; ++q) acc += t[q];
    }
    for (; ch + 16 <= n; ch += 16) {
        float t[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) t[q] = p[(int64_t)(ch + q) * stride];
#pragma unroll
        for (int q = 0; q < 16; ++q) acc += t[q];
    }
    for (; ch < n; ++ch) acc += p[(int64_t)ch * stride];
    return acc;
}

struct FinalizeArgs {
    const float* Ph; int head_chunks; int n_heads; int64_t head_stride;    // head partials; stride between heads in G
    int64_t gW2, gb1, gb2;                                                 // offsets of head 0's tensors in G
    const float* Pt; int trunk_chunks; int n_trunks; int64_t trunk_stride; // LN/bias column-sum partials
    const float* Pw; int w_chunks;                                         // first-layer weight partials [k][c]
    int64_t gW0, gb0, gg, gbeta;
    int H, nout, in_dim;
    float* G;
};
int finalize_grads(const FinalizeArgs& f, hipStream_t s);

// Products and sums are rounded separately (no FMA contraction): the op order of torch's CPU kernels.
__device__ __forceinline__ float polyak(float p, float t, float tau, float one_minus_tau) {
#pragma clang fp contract(off)
    const float a = tau * p;
    const float b = one_minus_tau * t;
    return a + b;
}
struct AdamConst;
// One launch for "sum the per-workgroup gradient partials" and the optimiser step (single-GPU steps: nothing has to be
// exchanged between the two): the first blocks reduce the partials of every tensor except the H x H weights and step those
// elements in place (Adam, Polyak target, derived copies), the remaining blocks stream the H x H weights' Adam update.
struct FusedAdamArgs {
    float *p, *g, *m, *v, *target;
    const AdamConst* c;                // device
    int n_heads; int64_t w1_off[2];    // flat offsets of the H x H weights
    unsigned long long* bump;
};
struct ShadowSpec;
int finalize_adam(const FinalizeArgs& f, const FusedAdamArgs& a, const ShadowSpec& sh, hipStream_t s);

// The derived images of one net's weights, which the kernels read in place of the fp32 parameters (exorl_hip.h, exorl_weight_images, defines
// them): W0 transposed, fp32, per trunk (coalesced first-layer reads); W1 per head and W0 per trunk, K-padded with zeros, as bf16 planes
// (MFMA operands; W0 has hi and lo at most). The functions below are the one statement of where an element sits and how large an image is.
struct WeightImages { float* w0t = nullptr; Planes w1, w0; };
__host__ __device__ inline int64_t w0_kp(int64_t in_dim) { return (in_dim + 31) / 32 * 32; }      // row pitch of a W0 plane
// sizes per trunk / per head, in elements
__host__ __device__ inline int64_t w0t_size(int64_t in_dim, int64_t H) { return in_dim * H; }
__host__ __device__ inline int64_t w0_plane_size(int64_t in_dim, int64_t H) { return H * w0_kp(in_dim); }
__host__ __device__ inline int64_t w1_plane_size(int64_t H) { return H * H; }
// W0[c][k] of a trunk: in W0T [trunk][k][c], in a W0 plane [trunk][c][Kp]. (W1[r][c] of a head sits at head * w1_plane_size(H) + r * H + c.)
__host__ __device__ inline int64_t w0t_index(int64_t trunk, int64_t k, int64_t c, int64_t in_dim, int64_t H) { return trunk * w0t_size(in_dim, H) + k * H + c; }
__host__ __device__ inline int64_t w0_plane_index(int64_t trunk, int64_t c, int64_t k, int64_t in_dim, int64_t H) {
    return trunk * w0_plane_size(in_dim, H) + c * w0_kp(in_dim) + k;
}
// What the optimiser kernels need to keep the images of a net (and of its Polyak target, if any: empty otherwise) current.
struct ShadowSpec {
    int n_trunks, n_heads, in_dim, H;
    int64_t w0_off[2], w1_off[2];      // flat offsets of W0 (per trunk) and W1 (per head)
    WeightImages own, target;
};
int refresh_shadows(const float* p, int64_t n, const ShadowSpec& sh, bool target, hipStream_t s);

// ---- loss / sampling kernels (loss.hip)
struct NoiseSpec {           // where TruncatedNormal noise comes from
    const float* buf;        // (B,A) standard normal draws, or nullptr -> Philox(seed, counter)
    uint64_t seed;
    uint64_t counter;              // draw id = counter + (counter_ptr ? *counter_ptr : 0)
    const uint64_t* counter_ptr;   // device-resident base (advanced by step_begin_device) so a captured graph replays fresh draws
};

struct AdamConst {           // fp32 scalars of one torch.optim.Adam step (bias corrections folded in)
    float one_minus_b1, b2, one_minus_b2, bc2_sqrt, eps, neg_step_size, tau, one_minus_tau;
};

__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamConst& c) {
#pragma clang fp contract(off)
    // exp_avg.lerp_(g, 1-b1); exp_avg_sq.mul_(b2).addcmul_(g, g, 1-b2); p.addcdiv_(m, sqrt(v)/bc2_sqrt + eps, -lr/bc1)
    m = m + c.one_minus_b1 * (g - m);
    v = v * c.b2 + (c.one_minus_b2 * g) * g;
    const float denom = sqrtf(v) / c.bc2_sqrt + c.eps;
    p = p + (c.neg_step_size * m) / denom;
}

// Device-resident per-agent step state: everything that changes from one update() to the next, so the whole
// step can be captured once in a hipGraph and replayed with no host-side argument patching.
struct StepState {
    uint64_t replay_counter;     // Philox batch counter of the sampler bound to the graph
    uint64_t noise_counter;      // Philox draw counter for action noise (2 draws per step)
    long long t_actor, t_critic; // Adam step counts
    double b1t, b2t_actor_unused, b1t_c, b2t_c;   // running beta^t products: [actor b1^t, (pad), critic b1^t, critic b2^t]
    double b2t;                  // actor b2^t
    AdamConst actor, critic;
    double lr, b1, b2, eps, tau;  // the Python-float hyper-parameters torch.optim.Adam holds (dec7() of the fp32 ABI values)
    int has_critic;
    float stddev;                // exploration std of the step (utils.schedule value): read through a pointer, so a schedule
                                 // that moves every step needs no re-capture of the hipGraph
    int no_noise;                // 1: the kind's update() draws nothing and the noise counter stays put (IQL, FQE); 0 keeps the bytes every other kind has
};

// The same for an intrinsic-reward module (intr.hip): what changes from one exorl_intr_update to the next. The host keeps the truth
// (exorl_intr::t, cat_counter, queue_ptr) and pushes it here before a graph launch whenever an eager step or a setter moved it; a captured
// module step starts with intr_step_begin, which advances everything for the step and leaves the values the step's kernels read.
struct IntrStepState {
    uint64_t counter;            // Philox draw counter after this step's draw
    uint64_t draw_counter;       // ... and the one this step's draw uses (vae_code_kernel, Proto's candidate draw)
    long long t;                 // Adam step count
    long long queue_ptr;         // Proto: the queue's write pointer after this step
    long long qrow0;             // ... and the first row this step's candidates are written to
    int queue_size, num_protos;  // 0, 0 for the other kinds
    int draws;                   // Philox draws per step (SMM and Proto: 1)
    double b1t, b2t;             // running beta^t products, as StepState keeps them
    double b1, b2, eps;
    double lr[3];                // the optimisers of the kind: [0] cfg.lr; SMM: [1] sp_lr, [2] vae_lr
    AdamConst c[3];
};
// act() for up to ACT_FAST_ROWS observation rows in one launch (loss.hip, act_fast_kernel): trunk + LayerNorm + tanh + Linear(H,H) + ReLU +
// head + tanh + TruncatedNormal draw. x_host / noise_host (host pointers) travel as kernel arguments; `out` may be pinned host memory.
constexpr int ACT_FAST_ROWS = 2;            // x 256 floats of embedded observation: the kernel-argument block stays under 4 KB
struct ActFast {
    const float *x_dev, *x_host;            // one of the two
    const float *w0t, *P;
    int64_t b0, g, beta, W1, b1, W2, b2;
    float* part; unsigned int* ticket;      // scratch: cdiv(H, 4) * rows * nout floats; one zero-initialised word
    const float *noise_dev, *noise_host;    // at most one; both null -> Philox(seed, counter)
    uint64_t seed, counter;
    float* out;
    float stddev;
    int rows, in_dim, H, nout, eval_mode;
    int first_relu = 0; int64_t W0 = 0;     // pixel policy: the first layer is Linear(in_dim, H) + ReLU with torch-layout weights at offset W0 of P
                                            // (no W0T shadow, no LayerNorm); b0 is its bias
};
bool act_fast_supported(int rows, int in_dim, int H, int nout);
int act_fast(const ActFast& f, hipStream_t s);
// pixel act(): tanh(LayerNorm([x | meta] W^T + b)) for one encoding, split over 256 workgroups with an in-launch combine (loss.hip)
int trunk_one(const float* x, const float* meta, const float* W, const float* b, const float* gain, const float* beta, float* part, unsigned int* ticket,
              float* out, int R, int M, int F, hipStream_t s);
// out[0] = sum_i parts[2i], out[1] = sum_i parts[2i+1] in a fixed order (qhead's per-chunk [sum |min Q|, sum min Q] -> the 4-float
// statistics buffer that is all-reduced under data parallelism)
int reduce_pairs(const float* parts, int chunks, float* out, hipStream_t s);
// End-of-step kernel of the windowed metrics (loss.hip, metrics_window_kernel)
struct MetricsWindowArgs {
    const float *crit_part, *abs_part, *bc_part;   // fused: qhead mode 0's [chunk][6], mode 1's [chunk][2], head_bwd's [chunk] (TD3+BC)
    int q_chunks, bc_chunks;                       // qhead_chunks(B); head_chunks(B), or 0 when the kind has no BC term
    int fused;                                     // 1: form the step's metrics from the partials; 0: the step's metric kernels wrote them
    ActorLoss form; int act_dim, ent_from_std;
    float inv_bg, alpha;
    const float* stddev;                           // StepState::stddev
    float* metrics;                                // EXORL_N_METRICS slots (EXORL_M_*)
    double* sums; long long* steps;                // the window: EXORL_N_METRICS sums, one step count
};
int metrics_window(const MetricsWindowArgs& w, hipStream_t s);
// Forward-only evaluation (exorl_agent_evaluate; loss.hip). eval_mean_actions: the policy's mean action of the stacked actor forward, rows
// 0..B-1 of mu2 (next_obs) into dst_next, rows B..2B-1 (obs) into dst_pi, the action columns of the critic's inputs; raw: mu2 holds CQL's raw
// (mu | log_std) head, tanh of its first A columns is taken here. No draw, no counter.
int eval_mean_actions(const float* mu2, int64_t mu_ld, int raw, float* dst_next, float* dst_pi, int64_t dst_ld, int B, int A, hipStream_t s);
// eval_partials: one thread per row, per chunk of EVAL_CHUNK_ROWS rows the EXORL_N_EVAL - 1 sums of the header's EXORL_E_* slots, y = r + D min Q'.
// eval_window: thread i adds slot i's partials in chunk order as doubles to sums[i], thread EXORL_E_ROWS adds the rows.
constexpr int EVAL_CHUNK_ROWS = 256;
constexpr int EVAL_PARTS = EXORL_N_EVAL - 1;
inline int eval_chunks(int rows) { return cdiv(rows, EVAL_CHUNK_ROWS); }
struct EvalArgs {
    const float* mu; int64_t mu_ld; int raw;       // mu(s): the obs rows of the actor's output (raw: CQL's head before tanh)
    const float* a_data; int A;
    const float *q_data, *q_pi, *tq;               // (2, rows) each; all null without a critic (BC)
    const float *reward, *discount;
    float* part;                                   // [eval_chunks(rows)][EVAL_PARTS]
    double* sums;                                  // EXORL_N_EVAL
    int rows;
};
int eval_reduce(const EvalArgs& e, hipStream_t s);
int set_device_float(float* dst, float value, hipStream_t s);
int set_device_u64(uint64_t* dst, uint64_t value, hipStream_t s);

__host__ __device__ inline void fill_adam_const(AdamConst& c, double b1t, double b2t, double lr, double b1, double b2, double eps, double tau) {
    // double-precision scalar math, as torch's _single_tensor_adam does in Python floats; beta^t comes from a running
    // product kept in the step state (one multiply per step instead of two software pow() calls on the critical path)
    const double bc1 = 1.0 - b1t;
    const double bc2 = 1.0 - b2t;
    c.one_minus_b1 = (float)(1.0 - b1);
    c.b2 = (float)b2;
    c.one_minus_b2 = (float)(1.0 - b2);
    c.bc2_sqrt = (float)sqrt(bc2);
    c.eps = (float)eps;
    c.neg_step_size = (float)(-(lr / bc1));
    c.tau = (float)tau;
    c.one_minus_tau = (float)(1.0 - tau);
}

// One thread: advance the counters and pre-compute both optimisers' scalars for this step.
__device__ inline void step_begin_device(StepState* st, int advance_replay) {
    if (advance_replay) st->replay_counter += 1;
    if (!st->no_noise) st->noise_counter += 2;
    st->t_actor += 1;
    st->b1t *= st->b1;
    st->b2t *= st->b2;
    fill_adam_const(st->actor, st->b1t, st->b2t, st->lr, st->b1, st->b2, st->eps, 0.0);
    if (st->has_critic) {
        st->t_critic += 1;
        st->b1t_c *= st->b1;
        st->b2t_c *= st->b2;
        fill_adam_const(st->critic, st->b1t_c, st->b2t_c, st->lr, st->b1, st->b2, st->eps, st->tau);
    }
}


// One thread: advance the module's counters and pre-compute its optimisers' scalars for this step.
__device__ inline void intr_step_begin_device(IntrStepState* st) {
    st->t += 1;
    st->b1t *= st->b1;
    st->b2t *= st->b2;
    for (int i = 0; i < 3; ++i) fill_adam_const(st->c[i], st->b1t, st->b2t, st->lr[i], st->b1, st->b2, st->eps, 0.0);
    st->draw_counter = st->counter;
    st->counter += (uint64_t)st->draws;
    st->qrow0 = st->queue_ptr;
    if (st->queue_size > 0) st->queue_ptr = (st->queue_ptr + st->num_protos) % st->queue_size;
}

int prepare_inputs(const float* obs, const float* action, const float* next_obs, float* xa, float* xc_cur,
                   float* xc_next, float* xc_pi, int B, int O, int A, int has_critic, StepState* st, int advance_replay,
                   hipStream_t s);
// both TruncatedNormal draws of a DDPG-family step in one launch: rows 0..B-1 of mu2 -> next_action (draw 0),
// rows B..2B-1 -> pi(obs) sample (draw 1)
int sample_actions2(const float* mu2, const float* noise_c, const float* noise_a, uint64_t seed, const uint64_t* counter_ptr,
                    float stddev, float clip, float* dst_next, float* dst_pi, int64_t dst_ld, int B, int A, hipStream_t s,
                    const float* stddev_ptr = nullptr);
int sample_action(const float* mu, NoiseSpec noise, float stddev, float clip, int use_clip, float* dst, int64_t dst_ld,
                  int B, int A, float* logprob_sum, hipStream_t s, const float* stddev_ptr = nullptr, int world_size = 1);
// ---- CQL (cql.py:152-263)
struct CqlNoise {            // the five draws of one CQL update; null buffers -> Philox(seed, *counter_ptr + k)
    const float *z_next, *u_rand, *z_cur, *z_nxt, *z_actor;
    uint64_t seed;
    const uint64_t* counter_ptr;
};
struct CqlScalars {          // device-resident entropy-temperature state (cql.py:96-101,241-247)
    float log_alpha, m, v, alpha;
};
// raw2: actor head outputs on [next_obs; obs] (2B, 2A). Writes next_action into xc_next[:, O:] and the (3n+1)B critic
// rows x_all = [obs | rand] (nB) ; [obs | pi(obs) samples] (nB) ; [obs | pi(next_obs) samples] (nB) ; [obs | a_data] (B)
int cql_build_inputs(const float* obs, const float* action, const float* raw2, CqlNoise nz, float* xc_next, float* x_all, int B,
                     int O, int A, int n, hipStream_t s);
// per-row d(critic_loss)/dQ over the (3n+1)B rows of both nets + metrics (TD loss, logsumexp penalty)
// lag != nullptr: the penalty weight is exp(log_critic_alpha), stepped by Adam inside the kernel before it is used (cql.py:201-213)
int cql_critic_dq(const float* q_all, const float* tq, const float* reward, const float* discount, float* dq_all, float* metrics,
                  int B, int n, float cql_alpha, float inv_bg, hipStream_t s, CqlScalars* lag = nullptr, const AdamConst* c_dev = nullptr,
                  float target_penalty = 0.f,
                  int mode = 0, float* gsum = nullptr, const float* mc = nullptr);      // mc: Cal-QL's per-row lower bound (B), null: CQL
// rsample of pi(obs): y = tanh(mu + std z) -> xc_pi[:, O:]; stats[0] = sum log_pi (per element, cql.py:239)
int cql_actor_sample(const float* raw_obs, CqlNoise nz, float* xc_pi, int64_t ld, float* stats, int B, int O, int A, hipStream_t s);
// scalar Adam step on log_actor_alpha from the (all-reduced) sum of log_pi; writes alpha = exp(log_alpha) and metrics
int cql_alpha_step(CqlScalars* sc, const float* stats, const AdamConst* c_dev, float* metrics, int B, int A, float inv_bg, const float* q,
                   hipStream_t s);
// policy output for act(): tanh(mu) (eval) or tanh(mu + std z)
int cql_act(const float* raw, const float* noise, uint64_t seed, uint64_t counter, int eval_mode, float* out, int rows, int A, hipStream_t s);
int head_bwd_wide(const DoutSpec& dspec, const float* W, const float* a, float* dz, const Planes& dzq, float* P, int rows, int H,
                  int nout, int64_t astride, int64_t pstride, int want_params, hipStream_t s);

// CRR (crr.py:121-142): xc_rep[(b*n+i)] = [obs_b | TruncatedNormal(mu_b).sample(clip)] for i < n
int repeat_sample(const float* obs, const float* mu, const float* noise, uint64_t seed, const uint64_t* counter_ptr, uint64_t counter,
                  float stddev, float clip, float* xc_rep, int B, int O, int A, int n, hipStream_t s, const float* stddev_ptr = nullptr);
// w_b = f(min(Q1,Q2)(s_b, a_b) - mean_i min(Q1,Q2)(s_b, a_bi))
int crr_weights(const float* q_rep, const float* q_data, float* w, int B, int n, int weight_func, hipStream_t s);
// IQL's row kernel (loss.hip, chunk_rows_kernel<IqlRow>): from the target heads tq (2, rows), the critic heads q (2, rows), v = V(s), vn = V(s'), reward and
// discount, in one pass: dv (rows) = d L_V / d v, dq (2, rows) = d L_Q / d Q_j, w (rows) = the actor step's advantage weights, and per chunk of
// IQL_CHUNK_ROWS rows the IQL_PARTS sums below. iql_sums adds them in chunk order: into sums (raw, IQL_P_* order) and / or as partial means over
// the global batch into metrics' EXORL_M_* slots; either may be null.
constexpr int IQL_CHUNK_ROWS = 256;
constexpr int IQL_MAX_WG = 32;               // above 32 chunks (8192 rows) a workgroup takes a second chunk
enum { IQL_P_REWARD, IQL_P_TARGET, IQL_P_Q1, IQL_P_Q2, IQL_P_ERR1, IQL_P_ERR2, IQL_P_VLOSS, IQL_P_V, IQL_P_ADV, IQL_P_W, IQL_PARTS };
__host__ __device__ inline int iql_chunks(int rows) { return (rows + IQL_CHUNK_ROWS - 1) / IQL_CHUNK_ROWS; }
struct IqlRowsArgs {
    const float *tq, *q, *v, *vn, *reward, *discount;
    float *dv, *dq, *w, *part;               // part: [iql_chunks(rows)][IQL_PARTS]
    int rows;
    float inv_bg, expectile, temperature, max_weight;
};
int iql_rows(const IqlRowsArgs& a, hipStream_t s);
int iql_sums(const float* part, int rows, float inv_bg, float* sums, float* metrics, hipStream_t s);
// FQE's row kernel (loss.hip, chunk_rows_kernel<FqeRow>), on iql_rows' chunking: from the target heads tq (2, rows), the critic heads q (2, rows), reward
// and discount: dq (2, rows) = d L / d Q_i with each net regressed on its OWN target y_i = r + D Q'_i (no min), and per chunk the FQE_PARTS sums
// below. fqe_sums adds them in chunk order: into sums (raw, FQE_P_* order) and / or as partial means over the global batch into metrics' slots.
enum { FQE_P_REWARD, FQE_P_TARGET, FQE_P_Q1, FQE_P_Q2, FQE_P_ERR1, FQE_P_ERR2, FQE_PARTS };
struct FqeRowsArgs {
    const float *tq, *q, *reward, *discount;
    float *dq, *part;                        // part: [iql_chunks(rows)][FQE_PARTS]
    int rows;
    float inv_bg;
};
int fqe_rows(const FqeRowsArgs& a, hipStream_t s);
int fqe_sums(const float* part, int rows, float inv_bg, float* sums, float* metrics, hipStream_t s);
// ReBRAC's row kernel (loss.hip, chunk_rows_kernel<RebracRow>), on iql_rows' chunking: the critic target's penalty as a per-row correction of the
// reward. From the clipped target-policy sample a~' (rows, A at ld sample_ld), the dataset's next action a' (rows, A at next_ld) with its validity
// v (rows), reward and discount, in fp32 and in this order (nothing contracted):
//   s = sum over j ascending of (a~'_j - a'_j)^2;   p = v s;   t = critic_beta p;   r~ = r - D t        (steps 2 and 3: rebrac_reward)
// so that y = r~ + D min Q' = r + D (min Q' - critic_beta p). critic_beta = 0 and v = 0 leave r~ = r bit for bit. Per chunk the REBRAC_PARTS sums
// below (the reward's is the dataset's r, not r~). rebrac_sums adds them in chunk order: into sums (raw, REBRAC_P_* order) and / or as partial
// means over the global batch into EXORL_M_REBRAC_PENALTY, EXORL_M_REBRAC_VALID and EXORL_M_BATCH_REWARD.
enum { REBRAC_P_PENALTY, REBRAC_P_VALID, REBRAC_P_REWARD, REBRAC_PARTS };
struct RebracRowsArgs {
    const float* sample; int64_t sample_ld;
    const float* next_action; int64_t next_ld;
    const float *next_valid, *reward, *discount;
    float *reward_out, *part;                // part: [iql_chunks(rows)][REBRAC_PARTS]
    int rows, act_dim;
    float critic_beta;
};
int rebrac_rows(const RebracRowsArgs& a, hipStream_t s);
int rebrac_sums(const float* part, int rows, float inv_bg, float* sums, float* metrics, hipStream_t s);
// The SARSA setting's row kernel (loss.hip, chunk_rows_kernel<NextActionRow>), on the same chunking: the dataset's next action a' (rows, A at
// next_ld) over the action columns the kind's own launch left in the target critic's input (dst: rows, A at dst_ld = O + A), on the rows whose
// validity v (rows) is not 0. A masked copy, bit-exact; a row with v = 0 is not written and the columns outside the A are never touched. Per
// chunk the one sum of v. next_action_sums adds them in chunk order: into sums[0] (raw) and / or as the partial mean over the global batch
// into EXORL_M_SARSA_VALID.
enum { SARSA_P_VALID, SARSA_PARTS };
struct NextActionRowsArgs {
    const float* next_action; int64_t next_ld;
    const float* next_valid;
    float* dst; int64_t dst_ld;
    float* part;                             // [iql_chunks(rows)][SARSA_PARTS]
    int rows, act_dim;
};
int next_action_rows(const NextActionRowsArgs& a, hipStream_t s);
int next_action_sums(const float* part, int rows, float inv_bg, float* sums, float* metrics, hipStream_t s);
// mu (rows, A) of a tanh-mean actor forward into the action columns of a critic input (ld = dst_ld): FQE's a' = mu(s') and the value pass's mu(s)
int fqe_mean_actions(const float* mu, float* dst, int64_t dst_ld, int rows, int A, hipStream_t s);
// FQE's value pass: q (2, ld) at (s, mu(s)); rows < `rows` -> per-chunk fp64 partials [iql_chunks(rows)][FQE_VALUE_PARTS], added in chunk order to
// sums[EXORL_N_FQE_VALUE] (the last slot counts the rows)
constexpr int FQE_VALUE_PARTS = EXORL_N_FQE_VALUE - 1;
int fqe_value_reduce(const float* q, int ld, int rows, double* part, double* sums, hipStream_t s);
int critic_loss(const float* q, const float* tq, const float* reward, const float* discount, float* dq,
                float* metrics, int B, float inv_bg, hipStream_t s);
int actor_stats(const float* q, float* stats, int B, hipStream_t s);
// successor-feature critic: q[net][m] = sum_j task[m][j] * feat[net][m][j]   (aps.py:55-58)
int sf_q(const float* feat, const float* task, int64_t task_ld, float* q, int B, int sf, int nets, hipStream_t s);
int actor_dq(const float* q, const float* stats, float* dq, int B, float inv_bg, float alpha, int use_lambda,
             hipStream_t s);
int actor_dmu(const float* da, int64_t da_ld, int da_nets, int64_t da_net_stride, const float* mu, const float* a_data, const float* reward, const float* w, float* dpre, float* stats,
              float* metrics, int B, int A, float inv_bg, float alpha, ActorLoss form, float stddev, hipStream_t s, const float* stddev_ptr = nullptr);

// ---- optimiser (optim.hip)
int adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps,
              int64_t t, float* target, float tau, hipStream_t s);
int soft_update(const float* p, float* target, int64_t n, float tau, hipStream_t s);
// Adam with the scalars read from device memory (StepState), for graph-replayable steps.
// bump != nullptr: block 0 also increments *bump (the replay counter of a captured step: nothing later in the step reads it)
int adam_step_dev(float* p, const float* g, float* m, float* v, int64_t n, const AdamConst* c_dev, float* target,
                  const ShadowSpec* shadows, hipStream_t s, uint64_t* bump = nullptr);

// ---- plain Linear/ReLU stacks on the generic grouped GEMM (intr.hip); shared by the intrinsic modules and the pixel agent
struct Lin { int in, out; int64_t W, b; };           // offsets into a flat parameter buffer, torch layout W[out][in]
struct Mlp {                                         // Linear-ReLU-...-Linear; the last layer's output is raw unless relu_last
    std::vector<Lin> L;
    bool relu_last = false;
    std::vector<float*> act, dact;                   // per layer: (rows, out) activations and their gradients
};
int mlp_forward(const Mlp& m, const float* P, const float* x, int64_t ldx, int rows, int prec, hipStream_t s);
// dact[last] holds d(loss)/d(output); writes parameter gradients into G and, if dx, d(loss)/d(input) (rows, in0)
int mlp_backward(const Mlp& m, const float* P, float* G, const float* x, int64_t ldx, int rows, float* dx, int prec, hipStream_t s);
// n nets of identical shapes (twin Q heads, Disagreement's ensemble) layer by layer in shared launches; dx (rows, in0) receives the SUM of the nets' d/d(input)
int mlp_forward_many(const Mlp* nets, int n, const float* P, const float* x, int64_t ldx, int rows, int prec, hipStream_t s);
int mlp_backward_many(const Mlp* nets, int n, const float* P, float* G, const float* x, int64_t ldx, int rows, int prec, hipStream_t s, float* dx);
int launch_concat(const float* a, int64_t lda, int ca, const float* b, int64_t ldb, int cb, float* dst, int rows, hipStream_t s);

// ---- the module's side of the joint graph (intr.hip), used by exorl_agent_enable_graph_intr
// intr_graph_prepare: outside a capture — checks the batch, allocates the device step state on first use, sizes the bf16x3 plane arena for
// the step's GEMMs (a throw-away capture on `capture`) and pushes the host's counters. intr_graph_capture: the launches of
// exorl_intr_update(train = 1) on `b`, reading the device step state; enqueues nothing that runs now and leaves the host's counters alone.
// intr_graph_before_launch: re-pushes the counters on `s` if an eager step or a setter moved them; intr_graph_after_launch: advances the
// host mirrors by one step.
int intr_graph_prepare(exorl_intr* it, const exorl_intr_batch* b, hipStream_t capture);
int intr_graph_capture(exorl_intr* it, const exorl_intr_batch* b, hipStream_t capture);
int intr_graph_before_launch(exorl_intr* it, hipStream_t s);
void intr_graph_after_launch(exorl_intr* it);
void intr_graph_release(exorl_intr* it);
// meta agents: next_obs[:, O:O+M] = obs[:, O:O+M] on [obs | meta] rows of `ld` floats (the replay gather fills the obs rows' meta columns)
int copy_meta_columns(const float* obs, float* next_obs, int64_t ld, int rows, int O, int M, hipStream_t s);

// ---- exact 1-nearest-neighbour search against a key table in HBM (nn.hip): PRDC's BC target
constexpr int NN_MAX_SPLITS = 256;        // key ranges of one search: what a workspace sizes its partials for
constexpr int NN_MAX_DIM = 512;           // columns of a key: a 64-query tile of whole rows stays in LDS
// The table's build from the arena: one work item per (episode of the order table, 64-transition chunk), item0 / trans0 the item and
// transition prefix per episode (n_episodes + 1 entries). mean / inv null: the observations are taken as they are stored.
struct NnKeyBuild {
    const float *obs, *act;
    const int64_t* row0; const int32_t* len; const int32_t* item0; const int64_t* trans0;
    int n_episodes, n_items, O, A, pitch;
    const float *mean, *inv;
    float beta; int every;
    float* keys;
};
int nn_build_keys(const NnKeyBuild& b, hipStream_t s);
// q (rows, pitch) = [beta obs | mu | 0-pad]
int nn_query(const float* obs, const float* mu, float beta, int rows, int O, int A, int pitch, float* q, hipStream_t s);
struct NnPlan { int splits, tiles_per_split, q_tiles; };
NnPlan nn_plan(int n, int rows, int want_splits, int cus);       // want_splits 0: chosen from n, rows and the CU count
int nn_device_cus(int* cus);
// part_d2 / part_idx: plan.splits x rows scratch. a_nn (rows, act_dim), may be null: columns act_col0.. of each winning key row.
struct NnSearch {
    const float* keys; int n, pitch, dim;
    const float* q; int64_t q_ld; int rows;
    NnPlan plan;
    float* part_d2; int* part_idx;
    int* idx_out; float* d2_out;
    float* a_nn; int act_col0, act_dim;
};
int nn_search(const NnSearch& a, hipStream_t s);
int nn_dist(const float* d2, int rows, float inv_bg, float* out, hipStream_t s);      // *out = inv_bg sum sqrt(d2), a fixed order
// the replay's key table as exorl_replay_build_keys left it (replay.hip); valid = false once the arena, its order or its normaliser changed
struct ReplayKeys { const float* ptr; int64_t n; int pitch, obs_cols, act_dim; float beta; uint64_t epoch; bool valid; };
ReplayKeys replay_keys(exorl_replay* r);

// ---- replay (replay.hip) internal entry points used by the agent's graph capture
// Optional fan-out of the sampled rows into the agent's staged network inputs (what prepare_inputs would do in a second
// kernel): xa = [next_obs ; obs], xc_cur = [obs | action], xc_next[:, :O] = next_obs, xc_pi[:, :O] = obs. fp32 state
// observations only. st != nullptr: thread 0 also runs step_begin_device(st, 0).
struct StageOut {
    float *xa, *xc_cur, *xc_next, *xc_pi;
    int O, A, B, has_critic;
    StepState* st;
};
// The goal path of the gather (exorl_replay_set_goal): goals_host is the (pos_g, tau) per sample of the GIVEN / MT19937 samplers (Philox draws
// them in the kernel), goal / next_goal take the goal's columns behind obs and behind next_obs, strides in floats. Un-staged only.
struct GoalOut {
    const int32_t* goals_host;
    float* goal; int64_t goal_stride;
    float* next_goal; int64_t next_goal_stride;
};
int replay_sample_impl(exorl_replay* r, int32_t batch, int32_t nstep, float gamma, int32_t sampler,
                       const int32_t* pairs_host, const exorl_batch_out* out, int32_t* pairs_out_host, hipStream_t s,
                       const uint64_t* dev_counter, const StageOut* stage = nullptr, float* mc_return = nullptr, const GoalOut* goal = nullptr);
int replay_goal_cols(exorl_replay* r);           // G of the goal rule in force, 0: none (exorl_replay_set_goal)
uint64_t replay_goal_epoch(exorl_replay* r);     // number of exorl_replay_set_goal calls: a captured goal graph is bound to one value
// the return-to-go column as exorl_replay_build_returns left it; valid = false once an episode was appended or evicted or the order was set.
// ptr never moves once allocated.
struct ReplayReturns { const float* ptr; float gamma; uint64_t epoch; bool valid; };
ReplayReturns replay_returns(exorl_replay* r);
int replay_obs_bytes(exorl_replay* r);        // bytes of one SAMPLED observation (frames x the arena's row on a frame-stacked arena)
int replay_frame_stack(exorl_replay* r);      // frames per sampled observation (exorl_replay_set_frame_stack; 1: none)
void replay_dims(exorl_replay* r, int* act_dim, int* meta_dim);
// comm.cpp (exorl_comm is the C ABI's opaque struct, declared at global scope in exorl_hip.h)
int comm_allreduce_sum(exorl_comm* c, float* buf, int64_t n, hipStream_t s);
int comm_nranks(const exorl_comm* c);

uint64_t replay_philox_counter(exorl_replay* r);
uint64_t replay_weights_epoch(exorl_replay* r);      // number of exorl_replay_set_weights calls: a captured graph is bound to one value
bool replay_norm_on(exorl_replay* r);                // exorl_replay_set_obs_norm: the normalising gather is launched; a captured graph holds one of the two
// what a sample call does before its launch, without drawing: episode table upload, pair buffer, nstep vs the shortest episode
int replay_prepare(exorl_replay* r, int32_t batch, int32_t nstep, hipStream_t s);
void replay_advance_philox(exorl_replay* r, uint64_t n);

}  // namespace exorl
