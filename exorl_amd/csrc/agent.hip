// Agent update orchestration: TD3+BC, TD3, BC and the DDPG (states) backbone as one stream-ordered chain of
// the kernels in gemm.hip / rowops.hip / loss.hip / optim.hip.
// Replaces (file:line in the reference repo):
//   td3_bc.py:119-189 update_critic/update_actor/update    td3.py:117-186    bc.py:78-110
//   unsupervised_learning/ddpg.py:240-328
// Structure exploited (what the reference's autograd graph hides):
//   * the actor is evaluated on next_obs (critic target, td3_bc.py:124) and on obs (actor loss, :149) with the
//     SAME weights -> one stacked 2B-row forward;
//   * the twin critics / twin heads are independent nets -> every layer is a 2-problem grouped GEMM;
//   * the actor step needs only the critic's dgrad, and of dX only the action columns (the reference also
//     computes and discards the critic wgrad there — SURVEY 8d);
//   * Polyak averaging of the target is fused into the critic's Adam pass.
// Data parallel: the step is split in 4 phases at the three points where a global batch quantity is needed
// (critic grads, sum|Q| for lambda (td3_bc.py:154), actor grads); the caller all-reduces between phases.
#include <cmath>
#include <cstring>
#include <vector>

#include "kernels.h"

namespace exorl {

// A net = n_trunks x [Linear(in,H) LN Tanh] feeding n_heads x [Linear(H,H) ReLU Linear(H,out)].
// twin critic: 2 trunks, 2 heads (head i on trunk i); shared critic: 1 trunk, 2 heads; actor: 1, 1.
struct NetDesc {
    int in_dim = 0, out_dim = 0, H = 0, n_trunks = 0, n_heads = 0;
    int64_t W0 = 0, b0 = 0, g = 0, beta = 0, trunk_stride = 0;   // offsets of trunk 0's tensors; stride to trunk 1
    int64_t W1 = 0, b1 = 0, W2 = 0, b2 = 0, head_stride = 0;     // offsets of head 0's tensors; stride to head 1
    int64_t total = 0;                                           // padded flat size (floats)
    std::vector<TensorDesc> tensors;                             // reference parameters() order
};

static int64_t pad4(int64_t n) { return round_up(n, 4); }

static NetDesc make_net(int in_dim, int out_dim, int H, int n_trunks, int n_heads) {
    NetDesc d;
    d.in_dim = in_dim; d.out_dim = out_dim; d.H = H; d.n_trunks = n_trunks; d.n_heads = n_heads;
    int64_t off = 0;
    auto add = [&](int64_t rows, int64_t cols) { const int64_t o = off; d.tensors.push_back({o, rows, cols}); off += pad4(rows * cols); return o; };
    auto add_trunk = [&](bool first) {
        const int64_t w = add(H, in_dim), b = add(H, 1), gg = add(H, 1), be = add(H, 1);
        if (first) { d.W0 = w; d.b0 = b; d.g = gg; d.beta = be; }
        return w;
    };
    auto add_head = [&](bool first) {
        const int64_t w1 = add(H, H), bb1 = add(H, 1), w2 = add(out_dim, H), bb2 = add(out_dim, 1);
        if (first) { d.W1 = w1; d.b1 = bb1; d.W2 = w2; d.b2 = bb2; }
        return w1;
    };
    if (n_trunks == n_heads) {             // [trunk0 head0][trunk1 head1]
        int64_t t0 = 0, h0 = 0;
        for (int i = 0; i < n_trunks; ++i) {
            const int64_t t = add_trunk(i == 0);
            const int64_t h = add_head(i == 0);
            if (i == 0) { t0 = t; h0 = h; }
            if (i == 1) { d.trunk_stride = t - t0; d.head_stride = h - h0; }
        }
    } else {                               // [trunk][head0][head1]
        add_trunk(true);
        int64_t h0 = 0;
        for (int i = 0; i < n_heads; ++i) {
            const int64_t h = add_head(i == 0);
            if (i == 0) h0 = h;
            if (i == 1) d.head_stride = h - h0;
        }
    }
    d.total = round_up(off, 64);
    return d;
}

// Second stream for independent branches of the step (target forward || critic forward, wgrad || dgrad chain).
// Used while capturing: the hipGraph then has parallel branches, so kernels that fill only part of the 256 CUs
// (64x64-tile GEMMs, row kernels) overlap instead of queueing behind each other.
struct ForkStreams {                           // lives on the handle; whether a call forks is the call's (Step::fk)
    hipStream_t aux = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
};
struct Fork : ForkStreams {
    bool on = false;
    Fork() = default;
    Fork(const ForkStreams& st, bool enabled) : ForkStreams(st), on(enabled) {}
    int fork(hipStream_t s) const {            // aux continues after everything enqueued on s so far
        if (!on) return 0;
        EXORL_CHECK_HIP(hipEventRecord(ev_fork, s));
        EXORL_CHECK_HIP(hipStreamWaitEvent(aux, ev_fork, 0));
        return 0;
    }
    int join(hipStream_t s) const {            // s waits for everything enqueued on aux
        if (!on) return 0;
        EXORL_CHECK_HIP(hipEventRecord(ev_join, aux));
        EXORL_CHECK_HIP(hipStreamWaitEvent(s, ev_join, 0));
        return 0;
    }
    hipStream_t side(hipStream_t s) const { return on ? aux : s; }
};

// The bf16 images (Planes, kernels.h) sit beside the fp32 buffer they mirror; carve() fills the planes the agent's precision reads. h1's are written
// by the trunk kernels (bf16 routes) or by to_planes3 behind the trunk (three-plane route), dz2's by the head kernels or by to_planes3 behind
// them, W1's and W0's by the optimiser kernel (ShadowSpec) or, three planes, by refresh_w1_planes. One image serves every layout its buffer is read in.
struct FwdBufs {
    float *h1, *xhat, *rstd, *h2, *out;
    Planes h1q, xhatq;
    // rows row0.. of a one-trunk, one-head net's buffers (the obs half of the actor's stacked forward)
    FwdBufs rows_from(int64_t row0, int64_t H, int64_t out_cols) const {
        return FwdBufs{h1 + row0 * H, xhat + row0 * H, rstd + row0, h2 + row0 * H, out + row0 * out_cols, h1q.at(row0 * H), xhatq.at(row0 * H)};
    }
};
struct BwdBufs { float *dz2, *dh1; Planes dz2q; };

// Which operands the H x H products of a net read.
enum class Route {
    F32,       // fp32 buffers through gemm_grouped(prec): fp32 mode, and bf16x3 / bf16x6 at shapes that do not tile (the split happens inside the GEMM)
    Planes,    // bf16 activation pipeline through gemm16_grouped: hi planes (plain bf16) or hi + lo (bf16x3; H, batch multiples of 64: see planes_ok)
    Planes3,   // fp32 activation pipeline with hi + mid + lo images of the products' operands (bf16x6; carve: planes3_ok), gemm16_grouped
};
// bf16x3 takes the plane pipeline only when the shadow has lo planes (act() hides them: its rows do not tile by 64). bf16x6 takes the three-plane
// kernel when activation and weight images exist and the rows tile by 128 (act()'s 64-row chunks do not).
static Route route_of(int prec, const Planes& act, const Planes& w1, int rows) {
    if (prec == EXORL_PREC_BF16 || (prec == EXORL_PREC_BF16X3 && w1.lo)) return Route::Planes;
    if (prec == EXORL_PREC_BF16X6 && act && w1 && rows % 128 == 0) return Route::Planes3;
    return Route::F32;
}
// One GEMM operand in both forms, each at its own offset (W1 is strided by head_stride in the parameters and by H * H in its images).
struct Operand {
    const float* f; Planes q;
    Operand() : f(nullptr) {}
    Operand(const float* f32, int64_t foff, const Planes& planes, int64_t qoff) : f(f32 ? f32 + foff : nullptr), q(planes.at(qoff)) {}
};
struct Product { Operand A, B; float* C; const float* bias; int M, N, K; };      // every pitch is H
// A problem carries mid planes only when both operands have them, and likewise lo planes. (act()'s buffers have a hi plane at most: a plain-bf16
// act() multiplies hi planes, and a bf16x3 act() never comes here — route_of sends it to Route::F32.)
static Gemm16Problem g16(const Planes& A, const Planes& B, float* C, const float* bias, int M, int N, int K, int64_t ld) {
    Gemm16Problem p{A.hi, B.hi, C, bias, M, N, K, ld, ld, ld};
    if (A.mid && B.mid) { p.A_mid = A.mid; p.B_mid = B.mid; }
    if (A.lo && B.lo) { p.A_lo = A.lo; p.B_lo = B.lo; }
    return p;
}
static Gemm16Problem g16(const Product& p, int64_t ld) { return g16(p.A.q, p.B.q, p.C, p.bias, p.M, p.N, p.K, ld); }
// `count` (<= 4) products of one shape class in one grouped launch on the route's GEMM
static int products(Route rt, int prec, int a_layout, int b_layout, const Product* p, int count, int64_t ld, bool relu, bool accumulate, hipStream_t s) {
    if (rt == Route::F32) {
        GemmProblem g[4];
        for (int i = 0; i < count; ++i) g[i] = GemmProblem{p[i].A.f, p[i].B.f, p[i].C, p[i].bias, p[i].M, p[i].N, p[i].K, ld, ld, ld};
        return gemm_grouped(prec, a_layout, b_layout, g, count, relu, accumulate, s);
    }
    Gemm16Problem q[4];
    for (int i = 0; i < count; ++i) q[i] = g16(p[i], ld);
    return gemm16_grouped(a_layout, b_layout, q, count, relu, accumulate, s);
}
// W1 of every head -> its three plane images, one launch. Once per optimiser step (and per exorl_agent_params_changed) rather than once per use:
// a TD3+BC step reads the critic's W1 in five launches and the actor's in two.
static int refresh_w1_planes(const NetDesc& d, const float* P, const WeightImages& sh, hipStream_t s) {
    if (!sh.w1.mid) return 0;
    return to_planes3(P + d.W1, d.H, d.H, d.H, sh.w1.hi, sh.w1.mid, sh.w1.lo, d.H, d.H, d.n_heads, d.head_stride, w1_plane_size(d.H), s);
}
struct Partials { float *Ph, *Pt, *Pw; };                  // per-chunk partial gradients (fused.hip)

static ShadowSpec shadow_spec(const NetDesc& d, const WeightImages& sh, const WeightImages* target) {
    ShadowSpec s{};
    s.n_trunks = d.n_trunks; s.n_heads = d.n_heads; s.in_dim = d.in_dim; s.H = d.H;
    for (int t = 0; t < d.n_trunks; ++t) s.w0_off[t] = d.W0 + t * d.trunk_stride;
    for (int i = 0; i < d.n_heads; ++i) s.w1_off[i] = d.W1 + i * d.head_stride;
    s.own = sh;
    if (target) s.target = *target;
    // the optimiser kernel keeps the one- and two-plane images current; three-plane images are refresh_w1_planes' and stay out of its sight
    if (sh.w1.mid) s.own.w1 = s.target.w1 = Planes{};
    return s;
}

static int net_forward(const NetDesc& d, const float* P, const WeightImages& sh, const float* x, int64_t ldx, int rows,
                       const FwdBufs& f, bool save, bool tanh_out, int prec, hipStream_t s, const SampleSpec* sample = nullptr,
                       bool no_head = false) {
    const int H = d.H;
    const int64_t act = (int64_t)rows * H;
    const Route rt = route_of(prec, f.h1q, sh.w1, rows);
    const bool bf = rt == Route::Planes;
    // fast mode keeps the trunk activations as bf16 only (MFMA operand + LN backward input): 4 B/elem written instead of 10. The MFMA trunk needs
    // W0's image and H % 128 == 0; plain bf16 at other widths (H = 192) takes the fp32 trunk kernel with bf16 outputs.
    if (bf && sh.w0 && trunk_fwd16_supported(H))
        EXORL_TRY(trunk_fwd16(x, ldx, sh.w0, P + d.b0, P + d.g, P + d.beta, save ? f.rstd : nullptr, f.h1q, save ? f.xhatq : Planes{}, rows,
                              d.in_dim, H, d.n_trunks, act, d.trunk_stride, s));
    else
        EXORL_TRY(trunk_fwd(x, ldx, sh.w0t, P + d.b0, P + d.g, P + d.beta, bf ? nullptr : f.h1, (save && !bf) ? f.xhat : nullptr,
                            save ? f.rstd : nullptr, bf ? f.h1q.hi : nullptr, (bf && save) ? f.xhatq.hi : nullptr, rows, d.in_dim, H,
                            d.n_trunks, act, d.trunk_stride, (int64_t)d.in_dim * H, s));
    if (rt == Route::Planes3) EXORL_TRY(to_planes3(f.h1, H, d.n_trunks * rows, H, f.h1q.hi, f.h1q.mid, f.h1q.lo, d.n_trunks * rows, H, 1, 0, 0, s));
    Product p[2];
    for (int i = 0; i < d.n_heads; ++i) {        // h2_i = relu(h1 W1_i^T + b1_i), head i on trunk i (paired) or on the one trunk (shared)
        const int64_t t = (d.n_trunks == d.n_heads ? i : 0) * act;
        p[i] = Product{Operand(f.h1, t, f.h1q, t), Operand(P + d.W1, i * d.head_stride, sh.w1, i * w1_plane_size(H)), f.h2 + i * act,
                       P + d.b1 + i * d.head_stride, rows, H, H};
    }
    EXORL_TRY(products(rt, prec, 0, 0, p, d.n_heads, H, true, false, s));
    if (no_head) return 0;                       // the caller runs the fused head forward+backward (qhead)
    if (H % 4 == 0)
        EXORL_TRY(head_fwd4(f.h2, P + d.W2, P + d.b2, f.out, rows, H, d.out_dim, tanh_out ? 1 : 0, d.n_heads, act, d.head_stride,
                            (int64_t)rows * d.out_dim, s, sample));
    else
        EXORL_TRY(head_fwd(f.h2, P + d.W2, P + d.b2, f.out, rows, H, d.out_dim, tanh_out ? 1 : 0, d.n_heads, act, d.head_stride,
                           (int64_t)rows * d.out_dim, s));
    return 0;
}

// The critic on (obs, a_data) and its Polyak target on (next_obs, next_action) in shared launches (bf16 mode): the two forward
// chains are independent, same shapes, different weights -> 3 launches instead of 6, each filling the chip twice as deep.
static bool forward2_supported(const NetDesc& d, int prec, const WeightImages& sa, const FwdBufs& fa, const WeightImages& sb, const FwdBufs& fb, int rows) {
    const bool planes = route_of(prec, fa.h1q, sa.w1, rows) == Route::Planes && route_of(prec, fb.h1q, sb.w1, rows) == Route::Planes;
    return planes && sa.w0 && sb.w0 && trunk_fwd16_supported(d.H) && d.out_dim == 1 && d.n_heads == 2 && d.H % 4 == 0;
}
// fold_a (with no_head): net A's scalar heads are folded into the GEMM epilogue (Gemm16Problem::head_part) when the launch takes the 128 x TN
// kernels — A's h2 buffer then holds, per head, rows x *slots_a partial dots instead of hidden activations (qhead sums them)
static int net_forward2(const NetDesc& d, const float* Pa, const WeightImages& sa, const float* xa, const FwdBufs& fa, bool save_a,
                        const float* Pb, const WeightImages& sb, const float* xb, const FwdBufs& fb, bool save_b, int64_t ldx, int rows,
                        hipStream_t s, bool no_head = false, bool fold_a = false, int* slots_a = nullptr) {
    const int H = d.H;
    const int64_t act = (int64_t)rows * H, wst = w0_plane_size(d.in_dim, H);
    const float* P[2] = {Pa, Pb};
    const WeightImages* sh[2] = {&sa, &sb};
    const float* x[2] = {xa, xb};
    const FwdBufs* f[2] = {&fa, &fb};
    const bool save[2] = {save_a, save_b};
    TrunkBatch tb{};
    int nt = 0;
    for (int k = 0; k < 2; ++k)
        for (int t = 0; t < d.n_trunks; ++t) {
            const Planes w = sh[k]->w0.at(t * wst), h = f[k]->h1q.at(t * act), xh = save[k] ? f[k]->xhatq.at(t * act) : Planes{};
            tb.it[nt++] = TrunkItem{x[k], w.hi, P[k] + d.b0 + t * d.trunk_stride, P[k] + d.g + t * d.trunk_stride, P[k] + d.beta + t * d.trunk_stride,
                                    save[k] ? f[k]->rstd + (int64_t)t * rows : nullptr, h.hi, xh.hi, w.lo, h.lo, xh.lo};
        }
    EXORL_TRY(trunk_fwd16_batch(tb, nt, ldx, rows, d.in_dim, H, s));
    Gemm16Problem q[4];
    HeadBatch hb{};
    int nq = 0;
    for (int k = 0; k < 2; ++k)
        for (int i = 0; i < d.n_heads; ++i) {
            q[nq] = g16(f[k]->h1q.at((d.n_trunks == d.n_heads ? i : 0) * act), sh[k]->w1.at(i * w1_plane_size(H)), f[k]->h2 + i * act,
                        P[k] + d.b1 + i * d.head_stride, rows, H, H, H);
            hb.it[nq] = HeadItem{f[k]->h2 + i * act, P[k] + d.W2 + i * d.head_stride, P[k] + d.b2 + i * d.head_stride, f[k]->out + (int64_t)i * rows};
            ++nq;
        }
    if (slots_a) *slots_a = 0;
    if (no_head && fold_a && slots_a) {
        const int slots = gemm16_head_slots(q, nq);
        if (slots > 0 && (int64_t)slots <= H) {
            for (int i = 0; i < d.n_heads; ++i) {
                q[i].head_w = P[0] + d.W2 + i * d.head_stride;
                q[i].head_part = f[0]->h2 + i * act;
            }
            *slots_a = slots;
        }
    }
    EXORL_TRY(gemm16_grouped(0, 0, q, nq, true, false, s));
    if (no_head) return 0;
    return head_fwd1_batch(hb, nq, rows, H, s);
}

// G == nullptr: dgrad only (no parameter gradients). dx (n_trunks x rows x dx_cols, one slab per trunk — the
// consumer adds them) receives d/dx[:, col0:col0+dx_cols].
static int net_backward(const NetDesc& d, const float* P, const WeightImages& sh, float* G, const Partials& pt, const float* x,
                        int64_t ldx, int rows, const FwdBufs& f, const DoutSpec& dout, const BwdBufs& b, float* dx, int dx_col0,
                        int dx_cols, int prec, hipStream_t s, const Fork& fk, FinalizeArgs* defer = nullptr, bool have_dz2 = false) {
    const int H = d.H;
    const int64_t act = (int64_t)rows * H;
    const bool paired = d.n_trunks == d.n_heads;
    Route rt = route_of(prec, f.h1q, sh.w1, rows);
    if (rt == Route::Planes3 && !b.dz2q) rt = Route::F32;      // the three-plane kernel wants dz2's images too
    const bool bf = rt == Route::Planes;
    // the bf16 route's row kernels read and write the images in place of the fp32 buffers; on the other routes they see no image
    const Planes none{};
    const Planes &dz2q = bf ? b.dz2q : none, &h1q = bf ? f.h1q : none, &xhatq = bf ? f.xhatq : none;
    if (have_dz2) {
        // dz2 and the head partials were produced by qhead
    } else if (d.out_dim > 16) {
        EXORL_REQUIRE(d.n_heads == 1, "net_backward: wide heads are single-net only");
        EXORL_TRY(head_bwd_wide(dout, P + d.W2, f.h2, bf ? nullptr : b.dz2, dz2q, G ? pt.Ph : nullptr, rows, H, d.out_dim, act, d.head_stride,
                                G ? 1 : 0, s));
    } else {
        EXORL_TRY(head_bwd(dout, P + d.W2, f.h2, bf ? nullptr : b.dz2, dz2q, G ? pt.Ph : nullptr, rows, H, d.out_dim, d.n_heads, act,
                           d.head_stride, G ? 1 : 0, s, dout.mode == EXORL_DOUT_ACTOR_MU && dout.bc_part));
    }
    // dz2 converted once for the wgrad and the dgrad; h1's images are the forward pass's
    if (rt == Route::Planes3) EXORL_TRY(to_planes3(b.dz2, H, d.n_heads * rows, H, b.dz2q.hi, b.dz2q.mid, b.dz2q.lo, d.n_heads * rows, H, 1, 0, 0, s));
    auto trunk_of = [&](int i) { return (paired ? i : 0) * act; };
    auto wgrad = [&](int i, int r0, int kr) {      // dW1_i[n][k] = sum_{m in r0 .. r0 + kr} dz2_i[m][n] h1[m][k]
        const int64_t o = (int64_t)r0 * H;
        return Product{Operand(b.dz2, i * act + o, b.dz2q, i * act + o), Operand(f.h1, trunk_of(i) + o, f.h1q, trunk_of(i) + o),
                       G + d.W1 + i * d.head_stride, nullptr, H, H, kr};
    };
    auto dgrad = [&](int i) {                      // dh1[m][k] = sum_n dz2_i[m][n] W1_i[n][k]
        return Product{Operand(b.dz2, i * act, b.dz2q, i * act), Operand(P + d.W1, i * d.head_stride, sh.w1, i * w1_plane_size(H)),
                       b.dh1 + trunk_of(i), nullptr, rows, H, H};
    };
    Product p[2];
    int dgrads_done = 0;
    if (bf && G && !fk.on) {
        // bf16 route only, no side stream: wgrad + dgrad in one launch (independent readers of dz2). With a shared trunk the heads' dgrads add into
        // one dh1, so only the first joins the launch; the others follow below as accumulating launches.
        Gemm16Problem q[4];
        int at[4], nq = 0;
        for (int i = 0; i < d.n_heads; ++i) { at[nq] = 1; q[nq++] = g16(wgrad(i, 0, rows), H); }
        dgrads_done = paired ? d.n_heads : 1;
        for (int i = 0; i < dgrads_done; ++i) { at[nq] = 0; q[nq++] = g16(dgrad(i), H); }
        EXORL_TRY(gemm16_grouped_mixed(at, q, nq, s));
    } else if (G) {
        EXORL_TRY(fk.fork(s));                     // wgrad only feeds the optimiser: off the dgrad -> LN-backward chain
        // F32 and Planes3 routes: the wgrad sums over the rows in one float32 accumulator per element; from 8192 rows on (the row kernels' own
        // threshold) it runs as slabs of 1024 rows accumulated into G, so that no running sum is longer than 1024 terms (one pass over 8200 rows
        // left dW1 1.6e-6 of its largest element off the float64 value, 13 times the float32 reference's own error). The bf16 route (bf16-grade
        // operands) keeps one pass.
        const int slab = (!bf && rows >= 8192) ? 1024 : rows;
        for (int r0 = 0; r0 < rows; r0 += slab) {
            for (int i = 0; i < d.n_heads; ++i) p[i] = wgrad(i, r0, rows - r0 < slab ? rows - r0 : slab);
            EXORL_TRY(products(rt, prec, 1, 1, p, d.n_heads, H, false, r0 > 0, fk.side(s)));
        }
    }
    for (int i = 0; i < d.n_heads; ++i) p[i] = dgrad(i);
    if (!paired) {                                 // shared trunk: one launch per head, accumulating into the one dh1
        for (int i = dgrads_done; i < d.n_heads; ++i) EXORL_TRY(products(rt, prec, 0, 1, p + i, 1, H, false, i > 0, s));
    } else if (dgrads_done == 0) {                 // paired: one grouped launch
        EXORL_TRY(products(rt, prec, 0, 1, p, d.n_heads, H, false, false, s));
    }
    const bool dx_fused = dx && !G;              // dgrad-only pass: d/d(input columns) in the LayerNorm-backward kernel itself
    // beta: with the MFMA trunk's images (bf16 route, trunk_fwd16_supported) the kernel rebuilds the LayerNorm input from h
    EXORL_TRY(ln_bwd(b.dh1, f.h1, f.xhat, h1q, xhatq, f.rstd, P + d.g, pt.Pt, rows, H, d.n_trunks, act, d.trunk_stride, G ? 1 : 0, s,
                     dx_fused ? sh.w0t + (int64_t)dx_col0 * H : nullptr, (int64_t)d.in_dim * H, dx_fused ? dx : nullptr, dx_cols,
                     (bf && trunk_fwd16_supported(H)) ? P + d.beta : nullptr));
    if (dx && !dx_fused)       // dx[m][j] = sum_c dz0[m][c] W0[c][col0+j]: a row-dot against rows col0.. of the transposed shadow
        EXORL_TRY(head_fwd4(b.dh1, sh.w0t + (int64_t)dx_col0 * H, nullptr, dx, rows, H, dx_cols, 0, d.n_trunks, act,
                            (int64_t)d.in_dim * H, (int64_t)rows * dx_cols, s));
    if (G) {
        EXORL_TRY(outer_reduce(x, ldx, d.in_dim, b.dh1, pt.Pw, rows, H, d.n_trunks, act, s));
        EXORL_TRY(fk.join(s));                     // wgrad branch done before the gradients are finalised
        FinalizeArgs fa{};
        fa.Ph = pt.Ph; fa.head_chunks = have_dz2 ? qhead_chunks(rows) : head_chunks(rows); fa.n_heads = d.n_heads; fa.head_stride = d.head_stride;
        fa.gW2 = d.W2; fa.gb1 = d.b1; fa.gb2 = d.b2;
        fa.Pt = pt.Pt; fa.trunk_chunks = trunk_chunks(rows); fa.n_trunks = d.n_trunks; fa.trunk_stride = d.trunk_stride;
        fa.Pw = pt.Pw; fa.w_chunks = outer_chunks(rows);
        fa.gW0 = d.W0; fa.gb0 = d.b0; fa.gg = d.g; fa.gbeta = d.beta;
        fa.H = H; fa.nout = d.out_dim; fa.in_dim = d.in_dim; fa.G = G;
        if (defer) *defer = fa;                    // the optimiser launch sums the partials itself (finalize_adam)
        else EXORL_TRY(finalize_grads(fa, s));
    }
    return 0;
}

struct Carver : SimpleCarver {
    // exorl_debug_agent_poison_scratch: carve() marks the takes a step writes before it reads (scratch = true); `fill` collects those whole,
    // and of every other take only the alignment padding behind it, as (offset, floats) runs
    bool scratch = false;
    std::vector<std::pair<int64_t, int64_t>>* fill = nullptr;
    using SimpleCarver::SimpleCarver;
    float* take(int64_t n) {
        if (fill) {
            const int64_t padded = round_up(n, 64), o = scratch ? off : off + n, len = scratch ? padded : padded - n;
            if (len > 0) {
                if (!fill->empty() && fill->back().first + fill->back().second == o) fill->back().second += len;
                else fill->push_back({o, len});
            }
        }
        return SimpleCarver::take(n);
    }
};

constexpr int ACT_ROWS = 64;

// What an agent kind is, as one row of data (KINDS, behind the phase tables): every fact that more than one kind answers is read from here, so
// a new kind is one row, its phases and its block in carve(). A direct comparison against EXORL_AGENT_* is right only where the code reaches
// for that kind's own machinery (CQL's sample rows and scalars, APS's sf_q, CRR's value samples, PRDC's binding, the kind-only setters).
struct PhaseTable;
struct KindTraits {
    int kind;                      // EXORL_AGENT_*
    const char* name;
    int critic_trunks;             // 0: no critic (and no target); 1: two heads on a shared trunk; 2: twin nets
    int actor_outs;                // actor outputs per action dimension (2: CQL's mean and log-std)
    bool sf_heads;                 // the critic's heads emit cfg.sf_dim successor features, not a scalar
    bool value_net;                // V(s) beside the critic
    bool draws_noise;              // update() draws (StepState::no_noise is its negation)
    bool uses_stddev;              // a tanh-mean policy explored with the caller's stddev; false: a squashed normal with a std of its own
    ActorLoss actor_loss;          // the form handed to the actor-step kernels
    bool bc_nearest;               // the BC term pulls towards the searched a_nn, not the batch's action
    bool qfuse;                    // the fused scalar-head path may run (make_step decides per call)
    bool logs_logprob;             // phase 1 writes the log-prob of the pi(obs) sample among the metrics (ddpg.py:276,289)
    bool evaluates;                // forward-only evaluation (exorl_agent_evaluate)
    bool metric_window;            // exorl_agent_set_metric_window
    const char* one_process_why;   // non-null: world_size > 1 is refused, for this reason
    const PhaseTable* plan;
    int (*check)(const exorl_agent_cfg&);      // the kind's own configuration checks
    bool has_critic() const { return critic_trunks > 0; }
    bool uses_lambda() const { return actor_loss == ACTOR_LOSS_Q_BC; }      // lambda = alpha / mean |Q| scales the Q term beside a BC term
};
static const KindTraits* traits_of(int kind);      // nullptr: no such kind

}  // namespace exorl

using namespace exorl;

struct exorl_agent {
    exorl_agent_cfg cfg;
    const KindTraits* traits = nullptr;       // cfg.kind's row (describe)
    NetDesc actor, critic, value;             // value: IQL's V(s), one Q-net without the action columns
    bool has_critic = false, has_value = false;
    bool owns_ws = false;
    float* ws = nullptr;
    size_t ws_bytes = 0;
    // flat parameter state: [net][what]
    float* flat[4][4] = {{nullptr}};
    // batch slots
    float *obs = nullptr, *action = nullptr, *reward = nullptr, *discount = nullptr, *next_obs = nullptr;
    // staged inputs
    float *xa = nullptr, *xc_cur = nullptr, *xc_next = nullptr, *xc_pi = nullptr;
    FwdBufs fa{}, ft{}, fc{};    // actor (2B rows), target critic, critic
    BwdBufs bc{}, ba{};
    float *dq = nullptr, *da = nullptr, *dpre = nullptr, *abs_part = nullptr;
    float* row_w = nullptr;      // per-row weight of the weighted log-likelihood actor step (B): CRR's weights kernel and IQL's row kernel write it
    // ---- what one kind alone has
    struct {
        float *sfq = nullptr, *sftq = nullptr;       // scalar Q = task . successor features of critic / target (2, B)
    } aps;
    struct {
        float *x_all = nullptr, *dq_all = nullptr;   // (3n+1)B critic rows and their per-row loss gradients
        CqlScalars* sc = nullptr;                    // log_actor_alpha + Adam moments + alpha (device)
    } cql;
    struct {
        float* xc_rep = nullptr;                     // repeated (obs, sampled action) inputs
        FwdBufs fr{};                                // critic forward on B*num_value_samples rows (no grad)
    } crr;
    struct {      // the value net on the stacked [next_obs; obs] rows (2B forward, B backward: the actor's arrangement), the row kernel's outputs
        FwdBufs fv{}; BwdBufs bv{};
        WeightImages sh{}; ShadowSpec spec{}; Partials pv{};
        float *dv = nullptr, *part = nullptr;        // d L_V / d v (B); per-chunk metric sums [iql_chunks(B)][IQL_PARTS]; w goes to row_w
        float expectile = 0.7f, temperature = 3.0f, max_weight = 100.0f;      // exorl_agent_set_iql
    } iql;
    struct {
        float* part = nullptr;                       // per-chunk metric sums [iql_chunks(B)][FQE_PARTS]
        // the value pass (exorl_agent_set_fqe_value): views of the caller's buffer, [EXORL_N_FQE_VALUE double sums | pad to 256 B][iql_chunks(B) x
        // FQE_VALUE_PARTS double partials]
        double *value_sums = nullptr, *value_part = nullptr;
    } fqe;
    // the query rows [beta obs | mu(obs) | 0-pad], the search's partial minima and its results; a_nn stands where TD3+BC's actor phase reads
    // the batch's action. The table is the replay's (exorl_agent_set_prdc): pointer, rows and key ranges are fixed while it is bound.
    struct {
        float *q = nullptr, *d2 = nullptr, *a_nn = nullptr, *part_d2 = nullptr;
        int *idx = nullptr, *part_idx = nullptr;
        exorl_replay* replay = nullptr;
        ReplayKeys keys{};
        NnPlan plan{};
    } prdc;
    // ReBRAC, a setting of the TD3+BC kind (exorl_agent_set_rebrac; `on` is the mode): views of the caller's buffer, laid out by rebrac_carve.
    // The sampler writes next_action / next_valid (exorl_agent_batch_slots); the row kernel writes reward (r~) and part on every step before
    // anything reads them.
    struct {
        float *next_action = nullptr, *next_valid = nullptr, *reward = nullptr, *part = nullptr;
        float beta = 0.f;
        bool on = false;
    } rebrac;
    // The SARSA setting of the TD3+BC, TD3, CRR and FQE kinds (exorl_agent_set_sarsa; `on` is the mode): views of the caller's buffer, laid out by
    // sarsa_carve. The sampler writes next_action / next_valid (exorl_agent_batch_slots); the row kernel writes part on every step before
    // anything reads it. Never on together with rebrac.
    struct {
        float *next_action = nullptr, *next_valid = nullptr, *part = nullptr;
        bool on = false;
    } sarsa;
    // Cal-QL, a setting of the CQL kind (exorl_agent_set_calql; `on` is the mode): the caller's buffer holds mc_return (B), the dataset's
    // return-to-go of each row, written by the sampler (exorl_replay_sample_mc; the captured gather) or by the caller before every step.
    struct {
        float* mc_return = nullptr;
        bool on = false;
    } calql;
    WeightImages sh_actor{}, sh_critic{}, sh_target{};
    ShadowSpec spec_actor{}, spec_critic{};
    Partials pa{}, pc{};
    float *stats = nullptr, *metrics = nullptr;      // contiguous: stats[4] then metrics[EXORL_N_METRICS]
    float *act_x = nullptr, *act_noise = nullptr;
    float* act_part = nullptr; unsigned int* act_ticket = nullptr;      // one-launch act(): head shares per workgroup, arrival ticket
    FwdBufs fact{};
    StepState* state = nullptr;  // device-resident counters + Adam scalars (graph-replayable)
    int64_t actor_t = 0, critic_t = 0;       // host mirrors of state->t_*
    uint64_t act_noise_counter = 0;
    float inv_bg = 0.f;
    float dev_stddev = -1.f;     // host mirror of state->stddev (the last value enqueued for it)
    // captured step (sample + update) — exorl_agent_enable_graph
    hipGraphExec_t graph_exec = nullptr;
    hipGraph_t graph = nullptr;
    hipStream_t capture_stream = nullptr;
    exorl_replay* graph_replay = nullptr;
    uint64_t graph_weights_epoch = 0;        // the replay's exorl_replay_set_weights count at capture: the graph samples that table
    bool graph_goal = false;                 // captured by exorl_agent_enable_graph_goal: the gather relabels with the rule of ...
    uint64_t graph_goal_epoch = 0;           // ... this exorl_replay_set_goal count
    float graph_gamma = 0.f;                 // the capture's gamma: Cal-QL's gather reads a return-to-go column built with the same bits
    bool graph_norm_on = false;              // the replay's normaliser at capture, on or off: the graph holds the normalising or the copying gather
    uint64_t graph_replay_ctr = 0;           // host mirror of state->replay_counter: eager samples drawn between two launches move the replay's own
    exorl_intr* graph_intr = nullptr;        // joint graph (exorl_agent_enable_graph_intr): the module whose step rides in front of the agent's
    ForkStreams fk{};            // parallel-branch plumbing (a captured step forks when parallel_branches is set)
    bool parallel_branches = false;  // measured slower than one chain on MI355X (2987 vs 3259 steps/s): opt-in
    // data parallel: RCCL communicator attached by exorl_agent_set_comm; the library enqueues the all-reduces between the phases
    exorl_comm* comm = nullptr;
    hipStream_t comm_stream = nullptr;           // the 16-byte statistic travels here while the critic's backward pass runs
    hipEvent_t ev_stats_ready = nullptr, ev_stats_done = nullptr;
    FinalizeArgs pend_c{}, pend_a{}, pend_v{};           // fused optimiser launch: the partials a gradient phase left for the optimiser phase behind it
    bool want_metrics = true;    // the (B,1)-sized metric reductions are skipped when the caller never reads them (use_tb=False)
    // windowed metrics (exorl_agent_set_metric_window; win_sums != nullptr is the mode): views of the caller's buffer, laid out as
    // [EXORL_N_METRICS double sums | int64 steps | pad to 256 B][qhead_chunks(B) x 6 critic partials][head_chunks(B) BC partials]
    double* win_sums = nullptr; long long* win_steps = nullptr;
    float *win_crit = nullptr, *win_bc = nullptr;
    // forward-only evaluation (exorl_agent_set_eval): views of the caller's buffer, [EXORL_N_EVAL double sums | pad to 256 B][eval_chunks(B) x
    // EVAL_PARTS partials]
    double* eval_sums = nullptr;
    float* eval_part = nullptr;
};

namespace exorl {

// split-bf16 mode runs the bf16 activation pipeline on hi/lo planes when every H x H GEMM tiles by 64 (the LDS-DMA kernel has no
// edge handling); other shapes take the fp32 activation pipeline with the operands split inside the GEMM (gemm_kernel<BF16X3>)
static bool planes_ok(const exorl_agent_cfg& cfg) {
    return cfg.precision == EXORL_PREC_BF16X3 && cfg.hidden_dim % 64 == 0 && cfg.batch % 64 == 0 && trunk_fwd16_supported(cfg.hidden_dim);
}

// bf16x6 mode runs fp32 mode's pipeline with the H x H products on the three-plane kernel when every one of them tiles by 128 (the kernel has no
// edge handling): hidden_dim and every row count of the step — B, 2B, CQL's (3n + 1) B, CRR's B num_value_samples, all multiples of B. Other
// shapes keep the operands fp32 and split them inside the GEMM (gemm_kernel<BF16X6>). The choice is made from the shape alone.
static bool planes3_ok(const exorl_agent_cfg& cfg) {
    return cfg.precision == EXORL_PREC_BF16X6 && cfg.hidden_dim % 128 == 0 && cfg.batch % 128 == 0;
}

static const float* bc_target(const exorl_agent* a) { return a->traits->bc_nearest ? a->prdc.a_nn : a->action; }
static int prdc_pitch(const exorl_agent_cfg& cfg) { return (int)round_up(cfg.obs_dim + cfg.act_dim, 4); }

static void carve(exorl_agent* a, Carver& c) {
    const auto& cfg = a->cfg;
    const int64_t B = cfg.batch, O = cfg.obs_dim, A = cfg.act_dim, H = cfg.hidden_dim, W = O + A;
    const int64_t AO = a->actor.out_dim;                                     // actor head width (2A for CQL)
    const int64_t RC = cfg.kind == EXORL_AGENT_CQL ? (3 * cfg.n_samples + 1) * B : B;   // rows of the critic's gradient pass
    for (int w = 0; w < 4; ++w) a->flat[EXORL_NET_ACTOR][w] = c.take(a->actor.total);
    if (a->has_critic) {
        for (int w = 0; w < 4; ++w) a->flat[EXORL_NET_CRITIC][w] = c.take(a->critic.total);
        a->flat[EXORL_NET_CRITIC_TARGET][EXORL_T_PARAM] = c.take(a->critic.total);
    }
    a->obs = c.take(B * O); a->action = c.take(B * A); a->reward = c.take(B); a->discount = c.take(B); a->next_obs = c.take(B * O);
    // Images per buffer: 1 plain bf16, 2 bf16x3 on the plane pipeline, 3 bf16x6 on the plane route, 0 otherwise (planes_ok and planes3_ok exclude
    // each other by precision). The one- and two-plane images follow their struct's fp32 buffers, hi planes first; the three-plane images
    // (three_planes below, no-ops otherwise) follow their group of structs. The order is part of the contract: exorl_debug_agent_poison_scratch
    // and the whole-workspace digests of tools/agent_digests.py see it.
    const int np = cfg.precision == EXORL_PREC_BF16 ? 1 : planes_ok(cfg) ? 2 : planes3_ok(cfg) ? 3 : 0;
    const int nb = np == 3 ? 0 : np;                // images the row kernels write: the bf16 routes' only
    auto take_u16 = [&](int64_t n) { return reinterpret_cast<unsigned short*>(c.take((n + 1) / 2)); };
    auto take_hi_lo = [&](Planes& x, int64_t nx, Planes* y, int64_t ny, int planes) {
        if (planes >= 1) { x.hi = take_u16(nx); if (y) y->hi = take_u16(ny); }
        if (planes >= 2) { x.lo = take_u16(nx); if (y) y->lo = take_u16(ny); }
    };
    auto three_planes = [&](Planes& x, int64_t n) { if (np == 3) { x.hi = take_u16(n); x.mid = take_u16(n); x.lo = take_u16(n); } };
    // saved: xhat and rstd are kept for a backward pass. f32_h1 = false: nobody reads h1 as fp32 (CRR's value samples on the bf16 routes).
    auto take_fwd = [&](int64_t trunk_rows, int64_t head_rows, int64_t out_cols, bool saved, bool f32_h1, int planes) {
        FwdBufs f{};
        if (f32_h1) f.h1 = c.take(trunk_rows * H);
        if (saved) { f.xhat = c.take(trunk_rows * H); f.rstd = c.take(trunk_rows); }
        f.h2 = c.take(head_rows * H); f.out = c.take(head_rows * out_cols);
        take_hi_lo(f.h1q, trunk_rows * H, saved ? &f.xhatq : nullptr, trunk_rows * H, planes);
        return f;
    };
    auto take_bwd = [&](int64_t head_rows, int64_t trunk_rows) {
        BwdBufs b{c.take(head_rows * H), c.take(trunk_rows * H), {}};
        take_hi_lo(b.dz2q, head_rows * H, nullptr, 0, nb);
        return b;
    };
    auto take_shadow = [&](int64_t n_trunks, int64_t n_heads, int64_t in_dim) {      // W0 has no three-plane image: the trunk kernels read fp32
        WeightImages sh{c.take(n_trunks * w0t_size(in_dim, H)), {}, {}};
        take_hi_lo(sh.w1, n_heads * w1_plane_size(H), &sh.w0, n_trunks * w0_plane_size(in_dim, H), nb);
        return sh;
    };
    c.scratch = true;       // from here on: c.scratch says whether a step writes the sub-buffer before it reads it (see Carver)
    a->xa = c.take(2 * B * O);
    a->fa = take_fwd(2 * B, 2 * B, AO, true, true, nb);
    a->ba = take_bwd(B, B);
    three_planes(a->fa.h1q, 2 * B * H);
    three_planes(a->ba.dz2q, B * H);
    c.scratch = false;
    a->sh_actor = take_shadow(1, 1, O);
    three_planes(a->sh_actor.w1, w1_plane_size(H));
    c.scratch = true;
    a->pa = Partials{c.take((int64_t)head_chunks(B) * ((AO + 1) * H + 32)), c.take((int64_t)trunk_chunks(B) * 3 * H),
                     c.take((int64_t)outer_chunks(B) * O * H)};
    a->dpre = c.take(B * AO);
    c.scratch = false;      // statistics, metrics, step state, act()'s own scratch and ticket
    a->stats = c.take(4 + EXORL_N_METRICS);
    a->metrics = a->stats ? a->stats + 4 : nullptr;
    a->state = reinterpret_cast<StepState*>(c.take((sizeof(StepState) + 3) / 4));
    a->act_x = c.take(ACT_ROWS * O);
    a->act_noise = c.take(ACT_ROWS * A);
    a->act_part = c.take((int64_t)cdiv(H, 4) * ACT_FAST_ROWS * 16);
    a->act_ticket = reinterpret_cast<unsigned int*>(c.take(4));
    a->fact = take_fwd(ACT_ROWS, ACT_ROWS, AO, false, true, nb ? 1 : 0);      // act(): a hi plane at most (see g16)
    if (a->has_critic) {
        const int64_t nt = a->critic.n_trunks;
        c.scratch = true;
        a->xc_cur = c.take(B * W); a->xc_next = c.take(B * W); a->xc_pi = c.take(B * W);
        const int64_t od = a->critic.out_dim;
        a->ft = take_fwd(nt * B, 2 * B, od, false, true, nb);
        a->fc = take_fwd(nt * RC, 2 * RC, od, true, true, nb);
        a->bc = take_bwd(2 * RC, nt * RC);
        three_planes(a->ft.h1q, nt * B * H);
        three_planes(a->fc.h1q, nt * RC * H);
        three_planes(a->bc.dz2q, 2 * RC * H);
        if (cfg.kind == EXORL_AGENT_CQL) {
            a->cql.x_all = c.take(RC * W);
            a->cql.dq_all = c.take(2 * RC);
            c.scratch = false;
            a->cql.sc = reinterpret_cast<CqlScalars*>(c.take(16));
            c.scratch = true;
        }
        a->dq = c.take(2 * B);
        if (cfg.kind == EXORL_AGENT_APS) { a->aps.sfq = c.take(2 * B); a->aps.sftq = c.take(2 * B); }
        a->abs_part = c.take(2 * (int64_t)qhead_chunks(B));
        a->da = c.take(nt * B * A);
        if (cfg.kind == EXORL_AGENT_CRR) {
            const int64_t R = B * cfg.num_value_samples;
            a->crr.xc_rep = c.take(R * W);
            a->row_w = c.take(B);
            a->crr.fr = take_fwd(nt * R, 2 * R, 1, false, nb == 0, nb);
            three_planes(a->crr.fr.h1q, nt * R * H);
        }
        c.scratch = false;
        a->sh_critic = take_shadow(nt, 2, W);
        a->sh_target = take_shadow(nt, 2, W);
        three_planes(a->sh_critic.w1, 2 * w1_plane_size(H));
        three_planes(a->sh_target.w1, 2 * w1_plane_size(H));
        c.scratch = true;
        a->pc = Partials{c.take(2 * (int64_t)qhead_chunks(RC) * ((od + 1) * H + 32)), c.take(nt * (int64_t)trunk_chunks(RC) * 3 * H),
                         c.take(nt * (int64_t)outer_chunks(RC) * W * H)};
    }
    c.scratch = false;
    if (cfg.kind == EXORL_AGENT_IQL) {          // behind everything the other kinds take: their layouts stay as they are
        for (int w = 0; w < 4; ++w) a->flat[EXORL_NET_VALUE][w] = c.take(a->value.total);
        c.scratch = true;
        a->iql.fv = take_fwd(2 * B, 2 * B, 1, true, true, nb);
        a->iql.bv = take_bwd(B, B);
        three_planes(a->iql.fv.h1q, 2 * B * H);
        three_planes(a->iql.bv.dz2q, B * H);
        c.scratch = false;
        a->iql.sh = take_shadow(1, 1, O);
        three_planes(a->iql.sh.w1, w1_plane_size(H));
        c.scratch = true;
        a->iql.pv = Partials{c.take((int64_t)head_chunks(B) * (2 * H + 32)), c.take((int64_t)trunk_chunks(B) * 3 * H),
                         c.take((int64_t)outer_chunks(B) * O * H)};
        a->iql.dv = c.take(B);
        a->row_w = c.take(B);
        a->iql.part = c.take((int64_t)iql_chunks(B) * IQL_PARTS);
        c.scratch = false;
    }
    if (cfg.kind == EXORL_AGENT_FQE) {          // TD3's layout with the row kernel's partials behind it
        c.scratch = true;
        a->fqe.part = c.take((int64_t)iql_chunks(B) * FQE_PARTS);
        c.scratch = false;
    }
    if (cfg.kind == EXORL_AGENT_PRDC) {         // TD3+BC's layout with the search's buffers behind it: all written before they are read
        c.scratch = true;
        a->prdc.q = c.take(B * prdc_pitch(cfg));
        a->prdc.part_d2 = c.take((int64_t)NN_MAX_SPLITS * B);
        a->prdc.part_idx = reinterpret_cast<int*>(c.take((int64_t)NN_MAX_SPLITS * B));
        a->prdc.idx = reinterpret_cast<int*>(c.take(B));
        a->prdc.d2 = c.take(B);
        a->prdc.a_nn = c.take(B * A);
        c.scratch = false;
    }
}

// Whether the library accepts a configuration, from the configuration alone: the kind's row, the row's own checks, then what every kind asks
// of the dimensions and the precision. The order of the refusals is the library's interface (the first failing check names the error).
static int check_cfg(const exorl_agent_cfg* cfg) {
    EXORL_REQUIRE(cfg, "agent: null cfg");
    const KindTraits* t = traits_of(cfg->kind);
    EXORL_REQUIRE(t, "agent: unknown kind %d", cfg->kind);
    EXORL_REQUIRE(!t->one_process_why || cfg->world_size == 1, "agent: %s: world_size=%d is not supported for this kind", t->one_process_why,
                  cfg->world_size);
    EXORL_TRY(t->check(*cfg));
    EXORL_REQUIRE(cfg->obs_dim > 0 && cfg->act_dim > 0 && cfg->act_dim <= 16 && cfg->hidden_dim >= 4 && cfg->hidden_dim <= 1024 && cfg->hidden_dim % 4 == 0 &&
                  cfg->obs_dim + cfg->act_dim <= 256 &&
                  cfg->batch > 0, "agent: unsupported dims O=%d A=%d (<=16) H=%d (multiple of 4, <=1024) B=%d; O+A <= 256", cfg->obs_dim, cfg->act_dim,
                  cfg->hidden_dim, cfg->batch);
    EXORL_REQUIRE(cfg->precision == EXORL_PREC_F32 || cfg->precision == EXORL_PREC_BF16 || cfg->precision == EXORL_PREC_BF16X3 ||
                  cfg->precision == EXORL_PREC_BF16X6, "agent: unknown precision %d", cfg->precision);
    EXORL_REQUIRE(cfg->world_size >= 1, "agent: world_size must be >= 1");
    EXORL_REQUIRE(cfg->precision != EXORL_PREC_BF16 || (cfg->hidden_dim % 8 == 0 && cfg->batch % 8 == 0),
                  "agent: bf16 precision needs hidden_dim and batch to be multiples of 8 (got H=%d B=%d)", cfg->hidden_dim, cfg->batch);
    return 0;
}

// Everything the handle derives from an accepted configuration: the row and the nets. carve() and every reader start from this.
static int describe(exorl_agent* a, const exorl_agent_cfg* cfg) {
    EXORL_TRY(check_cfg(cfg));
    const KindTraits& t = *traits_of(cfg->kind);
    a->cfg = *cfg;
    a->traits = &t;
    a->has_critic = t.has_critic();
    a->actor = make_net(cfg->obs_dim, t.actor_outs * cfg->act_dim, cfg->hidden_dim, 1, 1);
    if (a->has_critic) a->critic = make_net(cfg->obs_dim + cfg->act_dim, t.sf_heads ? cfg->sf_dim : 1, cfg->hidden_dim, t.critic_trunks, 2);
    a->has_value = t.value_net;
    if (a->has_value) a->value = make_net(cfg->obs_dim, 1, cfg->hidden_dim, 1, 1);
    a->inv_bg = 1.0f / ((float)cfg->batch * (float)cfg->world_size);
    return 0;
}

// update(): draw `which` (0 = critic target, 1 = actor) of this step, counter base lives in StepState
static NoiseSpec noise_spec(exorl_agent* a, const float* buf, int which) {
    return NoiseSpec{buf, a->cfg.seed, (uint64_t)which, buf ? nullptr : &a->state->noise_counter};
}
// act(): separate counter space (top bit set) so exploration draws never collide with update draws
static NoiseSpec act_noise_spec(exorl_agent* a, const float* buf) {
    NoiseSpec n{buf, a->cfg.seed, 0, nullptr};
    if (!buf) n.counter = (1ull << 63) | a->act_noise_counter++;
    return n;
}

static int push_opt_steps(exorl_agent* a) {
    long long t[2] = {a->actor_t, a->critic_t};
    EXORL_CHECK_HIP(hipMemcpy(&a->state->t_actor, t, sizeof(t), hipMemcpyHostToDevice));
    // beta^t as the device forms it (a running product, one multiply per step) so that a restored agent continues bit-identically
    auto prod = [](double b, long long t) { double r = 1.0; for (long long i = 0; i < t; ++i) r *= b; return r; };
    const double p[4] = {prod(0.9, a->actor_t), 0.0, prod(0.9, a->critic_t), prod(0.999, a->critic_t)};
    const double p2 = prod(0.999, a->actor_t);
    EXORL_CHECK_HIP(hipMemcpy(&a->state->b1t, p, sizeof(p), hipMemcpyHostToDevice));
    EXORL_CHECK_HIP(hipMemcpy(&a->state->b2t, &p2, sizeof(p2), hipMemcpyHostToDevice));
    return 0;
}

// Everything the handle keeps for one net (EXORL_NET_*), by reference: what a forward, a backward or an optimiser launch of that net is given.
// The critic's Polyak target has parameters and weight images of its own and borrows the rest from the critic.
struct NetView {
    const NetDesc& d;
    float* const* flat;                  // [EXORL_T_*]: parameters, gradients, Adam moments
    const WeightImages& sh;
    const Partials& pt;
    const BwdBufs& b;
    FinalizeArgs& pend;                  // the partials a gradient phase left for the optimiser phase behind it (fused optimiser launch)
    const ShadowSpec& spec;
    float* P() const { return flat[EXORL_T_PARAM]; }
    float* G() const { return flat[EXORL_T_GRAD]; }
};
static bool has_net(const exorl_agent* a, int net) {
    if (net == EXORL_NET_ACTOR) return true;
    if (net == EXORL_NET_CRITIC || net == EXORL_NET_CRITIC_TARGET) return a->has_critic;
    return net == EXORL_NET_VALUE && a->has_value;
}
static NetView net_view(exorl_agent* a, int net) {
    switch (net) {
        case EXORL_NET_ACTOR: return NetView{a->actor, a->flat[net], a->sh_actor, a->pa, a->ba, a->pend_a, a->spec_actor};
        case EXORL_NET_VALUE: return NetView{a->value, a->flat[net], a->iql.sh, a->iql.pv, a->iql.bv, a->pend_v, a->iql.spec};
        case EXORL_NET_CRITIC_TARGET: return NetView{a->critic, a->flat[net], a->sh_target, a->pc, a->bc, a->pend_c, a->spec_critic};
        default: return NetView{a->critic, a->flat[net], a->sh_critic, a->pc, a->bc, a->pend_c, a->spec_critic};
    }
}
// How one driver call runs the step. Each driver builds one (make_step) before its first launch and hands it to every phase, so a step's launch
// decisions are taken once, from the call's arguments and the handle's settings, and nothing of one call carries over to the next.
//   exorl_agent_update_phase   one phase:                   whole = capture = staged = fork = false
//   exorl_agent_update         all phases:                  whole
//   enable_graph_impl          all phases under capture:    whole, capture; staged and fork as the replay and parallel_branches say
struct Step {
    hipStream_t s;
    float stddev;
    const float *noise_c, *noise_a;      // caller-supplied noise (parity tests), nullptr: device Philox
    bool whole;                          // this call drives every phase: the fused scalar-head kernels may run
    bool capture;                        // the launches are captured with the sampler in front: the step advances the replay counter itself
    bool staged;                         // the sampler's gather kernel wrote the staged inputs and advanced the step state
    Fork fk;                             // fk.on: independent branches go to the side stream
    // derived once
    bool fuse_opt;                       // one GPU, one chain: the optimiser launches reduce the gradient partials themselves
    bool qfuse;                          // fused scalar-head path: whole-step call on one GPU, twin scalar heads, and nobody reads the step's metrics
                                         // or they are collected in a window (the kernels' metrics variants then leave per-chunk sums for metrics_window)
    bool metric_kernels;                 // critic_loss, actor_dmu run: always in window mode off the fused path, else when the caller reads the metrics
    bool stats_in_phase2;                // TD3+BC on the fused path with a communicator: phase 2 reduces sum |Q| itself, on the side stream
};
static Step make_step(const exorl_agent* a, hipStream_t s, float stddev, const float* noise_c, const float* noise_a, bool whole, bool capture,
                      bool staged, bool fork) {
    const KindTraits& k = *a->traits;
    Step st{s, stddev, noise_c, noise_a, whole, capture, staged, Fork(a->fk, fork)};
    st.fuse_opt = whole && !a->comm && !fork;
    st.qfuse = whole && !fork && (!a->want_metrics || a->win_sums) && k.qfuse && a->critic.n_heads == 2 && a->critic.out_dim == 1 &&
               a->cfg.hidden_dim % 4 == 0;
    st.metric_kernels = a->win_sums ? !st.qfuse : a->want_metrics;
    st.stats_in_phase2 = st.qfuse && a->comm && k.uses_lambda();
    return st;
}

// Adam on net n with the step scalars c. target: the Polyak target stepped in the same pass (the critic's), or nullptr. bump: the replay counter a
// staged capture's last kernel advances, or nullptr.
static int opt_step(const Step& st, const NetView& n, const AdamConst* c, const NetView* target, uint64_t* bump) {
    float* const* f = n.flat;
    float* tp = target ? target->P() : nullptr;
    hipStream_t s = st.s;
    if (st.fuse_opt)
        EXORL_TRY(finalize_adam(n.pend, FusedAdamArgs{f[EXORL_T_PARAM], f[EXORL_T_GRAD], f[EXORL_T_ADAM_M], f[EXORL_T_ADAM_V], tp, c, n.d.n_heads,
                                                      {n.d.W1, n.d.W1 + n.d.head_stride}, reinterpret_cast<unsigned long long*>(bump)}, n.spec, s));
    else EXORL_TRY(adam_step_dev(f[EXORL_T_PARAM], f[EXORL_T_GRAD], f[EXORL_T_ADAM_M], f[EXORL_T_ADAM_V], n.d.total, c, tp, &n.spec, s, bump));
    // bf16x6 on the plane kernel: the stepped W1 (and the Polyak target's) as three planes for the next step's launches
    EXORL_TRY(refresh_w1_planes(n.d, n.P(), n.sh, s));
    if (target) EXORL_TRY(refresh_w1_planes(n.d, tp, target->sh, s));
    return 0;
}
static int opt_step_critic(exorl_agent* a, const Step& st, uint64_t* bump = nullptr) {
    const NetView target = net_view(a, EXORL_NET_CRITIC_TARGET);
    return opt_step(st, net_view(a, EXORL_NET_CRITIC), &a->state->critic, &target, bump);
}

// ---- the blocks every kind's step is made of --------------------------------------------------------
// Opens a step: stages the inputs and (thread 0 of the kernel) advances the device-side step state — counters, this step's Adam scalars — with the
// host's mirrors of the counters. A staged capture's gather kernel has done the device side already. st == nullptr: a forward-only pass
// (exorl_agent_evaluate, exorl_agent_fqe_value): the inputs are staged and nothing advances.
static int open_step(exorl_agent* a, const Step* st, hipStream_t s) {
    const auto& cfg = a->cfg;
    if (!st || !st->staged)
        EXORL_TRY(prepare_inputs(a->obs, a->action, a->next_obs, a->xa, a->xc_cur, a->xc_next, a->xc_pi, cfg.batch, cfg.obs_dim, cfg.act_dim,
                                 a->has_critic ? 1 : 0, st ? a->state : nullptr, st && st->capture ? 1 : 0, s));
    if (!st) return 0;
    a->actor_t += 1;                            // the step state counts steps for both nets (step_begin_device), whichever of them steps
    if (a->has_critic) a->critic_t += 1;
    return 0;
}

// The Polyak target on x_target (into ft, nothing saved) and the critic on (obs, a_data) (into fc): independent chains of one shape, so one set
// of shared launches where forward2 applies, else two chains, the target's on the side stream when the call forks. save: the critic keeps what a
// backward pass needs. fused_heads: the scalar heads are left to qhead (no_head), the target's folded into its GEMM where the launch allows
// (*tq_slots, see net_forward2).
static int twin_forward(exorl_agent* a, hipStream_t s, const Fork& fk, const float* x_target, bool save, bool fused_heads = false,
                        int* tq_slots = nullptr) {
    const NetView c = net_view(a, EXORL_NET_CRITIC), t = net_view(a, EXORL_NET_CRITIC_TARGET);
    const int B = a->cfg.batch, W = c.d.in_dim, prec = a->cfg.precision;
    if (!fk.on && forward2_supported(c.d, prec, t.sh, a->ft, c.sh, a->fc, B))
        return net_forward2(c.d, t.P(), t.sh, x_target, a->ft, false, c.P(), c.sh, a->xc_cur, a->fc, save, W, B, s, fused_heads, fused_heads, tq_slots);
    EXORL_TRY(fk.fork(s));
    EXORL_TRY(net_forward(c.d, t.P(), t.sh, x_target, W, B, a->ft, false, false, prec, fk.side(s), nullptr, fused_heads));
    EXORL_TRY(net_forward(c.d, c.P(), c.sh, a->xc_cur, W, B, a->fc, save, false, prec, s, nullptr, fused_heads));
    return fk.join(s);
}

// Parameter gradients of net n from dout: finalised into its flat gradients, or left as partials where the optimiser launch sums them itself.
static int net_grads(const exorl_agent* a, const Step& st, const NetView& n, const float* x, int rows, const FwdBufs& f, const DoutSpec& dout,
                     bool have_dz2 = false) {
    return net_backward(n.d, n.P(), n.sh, n.G(), n.pt, x, n.d.in_dim, rows, f, dout, n.b, nullptr, 0, 0, a->cfg.precision, st.s, st.fk,
                        st.fuse_opt ? &n.pend : nullptr, have_dz2);
}
// ... from a buffer that holds d L / d out, row by row (a row kernel wrote it)
static int net_grads_from(const exorl_agent* a, const Step& st, const NetView& n, const float* x, int rows, const FwdBufs& f, const float* buf) {
    DoutSpec d{};
    d.mode = EXORL_DOUT_BUFFER; d.buf = buf;
    return net_grads(a, st, n, x, rows, f, d);
}

// The actor's gradients on the obs half (rows B..2B of the stacked buffers) from d L / d mu: the forward where the step has not run it, the
// actor_loss metric kernel, the backward pass. form: the loss's (Q + BC, BC, weighted log-likelihood, else the critic's da
// alone); da_nets: how many slabs of a->da add up. dm: the caller's additions (phase 2's fused path); the common fields are set here.
static int actor_mu_step(exorl_agent* a, const Step& st, bool forward, ActorLoss form, int da_nets, const float* reward, DoutSpec dm) {
    const auto& cfg = a->cfg;
    const int B = cfg.batch, O = cfg.obs_dim, A = cfg.act_dim;
    const NetView n = net_view(a, EXORL_NET_ACTOR);
    const float* x = a->xa + (int64_t)B * O;
    const FwdBufs f = a->fa.rows_from(B, cfg.hidden_dim, A);
    if (forward) EXORL_TRY(net_forward(n.d, n.P(), n.sh, x, O, B, f, true, true, cfg.precision, st.s));
    if (st.metric_kernels)                      // actor_loss / batch_reward(BC) metrics only (the gradient is formed in head_bwd)
        EXORL_TRY(actor_dmu(a->da, A, da_nets, (int64_t)B * A, f.out, bc_target(a), reward, a->row_w, a->dpre, a->stats, a->metrics, B, A,
                            a->inv_bg, cfg.alpha, form, st.stddev, st.s, &a->state->stddev));
    dm.mode = EXORL_DOUT_ACTOR_MU; dm.da = da_nets ? a->da : nullptr; dm.da_nets = da_nets; dm.mu = f.out; dm.a_data = bc_target(a);
    dm.form = form; dm.inv_bg = a->inv_bg; dm.stddev = st.stddev; dm.stddev_ptr = &a->state->stddev; dm.w = a->row_w;
    return net_grads(a, st, n, x, B, f, dm);
}

constexpr size_t WIN_HEAD_BYTES = 256;       // the window's sums and step count
static_assert(EXORL_N_METRICS * sizeof(double) + sizeof(long long) <= WIN_HEAD_BYTES, "the window's sums and step count fit its head");
static size_t window_bytes(const exorl_agent_cfg& cfg) {
    return WIN_HEAD_BYTES + sizeof(float) * (size_t)round_up(6 * (int64_t)qhead_chunks(cfg.batch) + head_chunks(cfg.batch), 64);
}
static int run_metrics_window(exorl_agent* a, const Step& st) {
    const int B = a->cfg.batch;
    MetricsWindowArgs w{};
    w.fused = st.qfuse ? 1 : 0;
    w.crit_part = a->win_crit; w.abs_part = a->abs_part; w.bc_part = a->win_bc;
    w.q_chunks = qhead_chunks(B); w.bc_chunks = a->traits->uses_lambda() ? head_chunks(B) : 0;
    w.form = a->traits->actor_loss; w.act_dim = a->cfg.act_dim; w.ent_from_std = a->traits->uses_stddev;
    w.inv_bg = a->inv_bg; w.alpha = a->cfg.alpha; w.stddev = &a->state->stddev;
    w.metrics = a->metrics; w.sums = a->win_sums; w.steps = a->win_steps;
    return metrics_window(w, st.s);
}
// tq_slots > 0 (mode 0): this step's target critic left per-row partial head dots in ft.h2 (folded into the forward GEMM, net_forward2)
static int run_qhead(exorl_agent* a, const Step& st, int mode, int tq_slots, const float* reward) {
    const NetDesc& d = a->critic;
    const int B = a->cfg.batch, H = d.H;
    const int64_t act = (int64_t)B * H;
    const float* Pc = a->flat[EXORL_NET_CRITIC][EXORL_T_PARAM];
    const float* Pt = a->flat[EXORL_NET_CRITIC_TARGET][EXORL_T_PARAM];
    const bool bf = route_of(a->cfg.precision, a->fc.h1q, a->sh_critic.w1, B) == Route::Planes;       // as net_backward decides it
    QHeadArgs q{};
    for (int i = 0; i < 2; ++i) {
        q.a[i] = a->fc.h2 + i * act; q.W[i] = Pc + d.W2 + i * d.head_stride; q.b[i] = Pc + d.b2 + i * d.head_stride;
        q.a[2 + i] = a->ft.h2 + i * act; q.W[2 + i] = Pt + d.W2 + i * d.head_stride; q.b[2 + i] = Pt + d.b2 + i * d.head_stride;
    }
    q.q = a->fc.out; q.tq = a->ft.out; q.reward = reward; q.discount = a->discount;
    q.tpart[0] = q.tpart[1] = nullptr; q.tslots = 0;
    if (mode == 0 && tq_slots > 0) { q.tpart[0] = a->ft.h2; q.tpart[1] = a->ft.h2 + act; q.tslots = tq_slots; }
    q.dz = bf ? nullptr : a->bc.dz2; q.dzb = bf ? a->bc.dz2q.hi : nullptr; q.dzl = bf ? a->bc.dz2q.lo : nullptr; q.act = act;
    q.P = mode == 0 ? a->pc.Ph : nullptr;
    const bool met = mode == 0 && a->win_sums;       // the critic metrics' per-chunk sums ride in mode 0's otherwise unused abs_part
    q.abs_part = met ? a->win_crit : a->abs_part;
    q.rows = B; q.H = H; q.mode = mode; q.inv_bg = a->inv_bg;
    return qhead(q, st.s, met);
}

// The SARSA setting (exorl_agent_set_sarsa), off: nothing. Behind the launch that wrote the kind's own target action into xc_next's action columns
// and ahead of the target critic's forward: the dataset's a' over it on the rows with next_valid != 0, a masked copy in a launch of its own (the
// actor head's sample epilogue, which writes those columns for TD3+BC, keeps its bits and the base kind its launch count).
static int sarsa_rows(exorl_agent* a, hipStream_t s) {
    if (!a->sarsa.on) return 0;
    const int B = a->cfg.batch, O = a->cfg.obs_dim, A = a->cfg.act_dim;
    return next_action_rows(NextActionRowsArgs{a->sarsa.next_action, A, a->sarsa.next_valid, a->xc_next + O, O + A, a->sarsa.part, B, A}, s);
}
// ... and its metric, the partial mean of next_valid over the global batch, where the step's other metrics are written
static int sarsa_sums(exorl_agent* a, hipStream_t s) {
    if (!a->sarsa.on) return 0;
    return next_action_sums(a->sarsa.part, a->cfg.batch, a->inv_bg, nullptr, a->metrics, s);
}

// -- phase 0: everything up to the critic gradients -------------------------------------------------
static int phase0(exorl_agent* a, const Step& st) {
    const auto& cfg = a->cfg;
    hipStream_t s = st.s;
    const float stddev = st.stddev, *noise_c = st.noise_c;
    const int B = cfg.batch, O = cfg.obs_dim, A = cfg.act_dim, W = O + A, prec = cfg.precision;
    EXORL_TRY(open_step(a, &st, s));
    if (!a->has_critic) return 0;
    const float* Pa = a->flat[EXORL_NET_ACTOR][EXORL_T_PARAM];
    // actor on [next_obs; obs] in one pass (td3_bc.py:124 and :149 use the same weights)
    // next_action = dist.sample(clip) (td3_bc.py:125) and the actor-step sample pi(obs) (:151, it does not depend on the
    // critic update) straight into the two critic input buffers, as the epilogue of the actor head
    const bool fused_sample = cfg.hidden_dim % 4 == 0 && A > 1;
    SampleSpec sp{&a->state->stddev, noise_c, cfg.kind == EXORL_AGENT_CRR ? nullptr : st.noise_a, cfg.seed, &a->state->noise_counter, stddev, cfg.stddev_clip,
                  a->xc_next + O, a->xc_pi + O, W, B};
    EXORL_TRY(net_forward(a->actor, Pa, a->sh_actor, a->xa, O, 2 * B, a->fa, true, true, prec, s, fused_sample ? &sp : nullptr));
    if (!fused_sample)
        EXORL_TRY(sample_actions2(a->fa.out, noise_c, cfg.kind == EXORL_AGENT_CRR ? nullptr : st.noise_a, cfg.seed,
                                  &a->state->noise_counter, stddev, cfg.stddev_clip, a->xc_next + O, a->xc_pi + O, W, B, A, s, &a->state->stddev));
    // ReBRAC: the critic target's penalty on (a~' - a')^2 as a correction of the reward, r~ = r - D (beta p), from the sample the launch above
    // left in xc_next's action columns; every reader of the reward below takes r~ (y = r~ + D min Q' = r + D (min Q' - beta p))
    const float* reward = a->reward;
    if (a->rebrac.on) {
        EXORL_TRY(rebrac_rows(RebracRowsArgs{a->xc_next + O, W, a->rebrac.next_action, A, a->rebrac.next_valid, a->reward, a->discount,
                                             a->rebrac.reward, a->rebrac.part, B, A, a->rebrac.beta}, s));
        reward = a->rebrac.reward;
    }
    EXORL_TRY(sarsa_rows(a, s));                // the SARSA setting: the dataset's a' over a~' where the episode holds it
    const bool qf = st.qfuse;
    int tq_slots = 0;
    EXORL_TRY(twin_forward(a, s, st.fk, a->xc_next, true, qf, &tq_slots));      // target critic (td3_bc.py:126) and critic (td3_bc.py:130)
    if (qf) EXORL_TRY(run_qhead(a, st, 0, tq_slots, reward));      // Q, Q', TD gradient, dz2 and head partials in one kernel
    const bool aps = cfg.kind == EXORL_AGENT_APS;
    const float* task = aps ? a->obs + (O - cfg.sf_dim) : nullptr;          // obs rows are [observation | task] (aps.py:236-238)
    const float *qv = a->fc.out, *tqv = a->ft.out;
    if (aps) {                                  // Q = task . successor features (aps.py:55-58)
        EXORL_TRY(sf_q(a->ft.out, task, O, a->aps.sftq, B, cfg.sf_dim, 2, s));
        EXORL_TRY(sf_q(a->fc.out, task, O, a->aps.sfq, B, cfg.sf_dim, 2, s));
        qv = a->aps.sfq; tqv = a->aps.sftq;
    }
    if (st.metric_kernels)
        EXORL_TRY(critic_loss(qv, tqv, reward, a->discount, a->dq, a->metrics, B, a->inv_bg, s));   // :133-137
    // behind critic_loss, which reported the mean of r~ as batch_reward: the row kernel's sums put the dataset's r there, and the penalty's slots
    if (a->rebrac.on && st.metric_kernels) EXORL_TRY(rebrac_sums(a->rebrac.part, B, a->inv_bg, nullptr, a->metrics, s));
    if (st.metric_kernels) EXORL_TRY(sarsa_sums(a, s));
    DoutSpec td{};                              // d(2 x MSE)/dQ computed where it is consumed (:127-131)
    td.mode = EXORL_DOUT_TD; td.q = qv; td.tq = tqv; td.reward = reward; td.discount = a->discount; td.inv_bg = a->inv_bg;
    td.task = task; td.task_ld = O;
    return net_grads(a, st, net_view(a, EXORL_NET_CRITIC), a->xc_cur, B, a->fc, td, qf);                                       // :141
}

// -- phase 1: critic optimiser step (+ fused soft update), critic re-evaluated at pi(obs) -------------
static int phase1(exorl_agent* a, const Step& st) {
    if (!a->has_critic) return 0;
    const auto& cfg = a->cfg;
    hipStream_t s = st.s;
    const float stddev = st.stddev, *noise_a = st.noise_a;
    const int B = cfg.batch, O = cfg.obs_dim, A = cfg.act_dim, W = O + A, prec = cfg.precision;
    EXORL_TRY(opt_step_critic(a, st));
    if (cfg.kind == EXORL_AGENT_CRR) {          // crr.py:170-179 with the updated critic, no gradients
        const int n = cfg.num_value_samples;
        const float* Pc = a->flat[EXORL_NET_CRITIC][EXORL_T_PARAM];
        EXORL_TRY(repeat_sample(a->obs, a->fa.out + (int64_t)B * A, noise_a, cfg.seed, noise_a ? nullptr : &a->state->noise_counter, 1,
                                stddev, cfg.stddev_clip, a->crr.xc_rep, B, O, A, n, s, &a->state->stddev));
        EXORL_TRY(net_forward(a->critic, Pc, a->sh_critic, a->crr.xc_rep, W, B * n, a->crr.fr, false, false, prec, s));      // compute_value
        EXORL_TRY(net_forward(a->critic, Pc, a->sh_critic, a->xc_cur, W, B, a->fc, false, false, prec, s));          // Q(s, a_data)
        EXORL_TRY(crr_weights(a->crr.fr.out, a->fc.out, a->row_w, B, n, cfg.weight_func, s));
        return 0;
    }
    // pi(obs) sample already sits in xc_pi (phase 0); DDPG logs its log-prob (ddpg.py:276,289)
    if (a->traits->logs_logprob && (a->want_metrics || a->win_sums))
        EXORL_TRY(sample_action(a->fa.out + (int64_t)B * A, noise_spec(a, noise_a, 1), stddev, cfg.stddev_clip, 1, a->xc_pi + O, W, B, A,
                                a->metrics + EXORL_M_ACTOR_LOGPROB, s, &a->state->stddev, cfg.world_size));
    const bool qf = st.qfuse;
    EXORL_TRY(net_forward(a->critic, a->flat[EXORL_NET_CRITIC][EXORL_T_PARAM], a->sh_critic, a->xc_pi, W, B, a->fc, true, false, prec, s,
                          nullptr, qf));
    if (cfg.kind == EXORL_AGENT_APS) {
        EXORL_TRY(sf_q(a->fc.out, a->obs + (O - cfg.sf_dim), O, a->aps.sfq, B, cfg.sf_dim, 2, s));
        EXORL_TRY(actor_stats(a->aps.sfq, a->stats, B, s));
    } else if (!qf) {
        EXORL_TRY(actor_stats(a->fc.out, a->stats, B, s));
    }
    return 0;
}

// -- phase 2: actor gradients -----------------------------------------------------------------------
static int phase2(exorl_agent* a, const Step& st) {
    const auto& cfg = a->cfg;
    hipStream_t s = st.s;
    const bool qf = st.qfuse;
    const int B = cfg.batch, O = cfg.obs_dim, A = cfg.act_dim, W = O + A, prec = cfg.precision;
    if (a->has_critic && cfg.kind != EXORL_AGENT_CRR) {
        DoutSpec dq{};                          // -lambda/Bg routed to the smaller Q (td3_bc.py:152-155)
        dq.mode = EXORL_DOUT_ACTOR_Q; dq.q = a->fc.out; dq.stats = a->stats; dq.inv_bg = a->inv_bg; dq.alpha = cfg.alpha;
        if (cfg.kind == EXORL_AGENT_APS) { dq.q = a->aps.sfq; dq.task = a->obs + (O - cfg.sf_dim); dq.task_ld = O; }
        dq.use_lambda = a->traits->uses_lambda();
        if (qf) EXORL_TRY(run_qhead(a, st, 1, 0, a->reward));   // Q(s, pi(s)), its min-routing gradient (lambda applied later), dz2, sum|Q| partials
        if (st.stats_in_phase2) {                // lambda needs sum|Q| over the GLOBAL batch (td3_bc.py:154): reduce it while the critic's
            EXORL_TRY(reduce_pairs(a->abs_part, qhead_chunks(B), a->stats, s));          // backward pass runs (it does not depend on lambda)
            EXORL_CHECK_HIP(hipEventRecord(a->ev_stats_ready, s));
            EXORL_CHECK_HIP(hipStreamWaitEvent(a->comm_stream, a->ev_stats_ready, 0));
            EXORL_TRY(comm_allreduce_sum(a->comm, a->stats, 4, a->comm_stream));
            EXORL_CHECK_HIP(hipEventRecord(a->ev_stats_done, a->comm_stream));
        }
        EXORL_TRY(net_backward(a->critic, a->flat[EXORL_NET_CRITIC][EXORL_T_PARAM], a->sh_critic, nullptr, a->pc, a->xc_pi, W, B, a->fc,
                               dq, a->bc, a->da, O, A, prec, s, st.fk, nullptr, qf));
    }
    DoutSpec dm{};
    if (qf) {                                   // lambda = alpha / mean|Q| from the per-chunk sums qhead left behind
        dm.lam_parts = a->abs_part; dm.lam_chunks = qhead_chunks(B); dm.use_lambda = a->traits->uses_lambda(); dm.alpha = cfg.alpha;
        if (st.stats_in_phase2) {                // the all-reduced statistic (one 'chunk': stats[0] = global sum |Q|)
            EXORL_CHECK_HIP(hipStreamWaitEvent(s, a->ev_stats_done, 0));
            dm.lam_parts = a->stats; dm.lam_chunks = 1;
        }
        if (a->win_sums && a->traits->uses_lambda()) dm.bc_part = a->win_bc;       // head_bwd's metrics variant: actor_loss's (mu - a)^2 term
    }
    // BC (bc.py:82) runs its only forward here; the other kinds' is the obs half of phase 0's stacked pass
    return actor_mu_step(a, st, !a->has_critic, a->traits->actor_loss, a->has_critic ? a->critic.n_trunks : 0, a->has_critic ? nullptr : a->reward, dm);
}

static int phase3(exorl_agent* a, const Step& st) {
    return opt_step(st, net_view(a, EXORL_NET_ACTOR), &a->state->actor, nullptr, st.staged ? &a->state->replay_counter : nullptr);
}

// ---- CQL (cql.py:152-263) ---------------------------------------------------------------------------
static CqlNoise cql_noise(exorl_agent* a, const Step& st) {
    const int64_t BA = (int64_t)a->cfg.batch * a->cfg.act_dim, n = a->cfg.n_samples;
    const float* nc = st.noise_c;
    CqlNoise z{};
    z.z_next = nc; z.u_rand = nc ? nc + BA : nullptr; z.z_cur = nc ? nc + (1 + n) * BA : nullptr;
    z.z_nxt = nc ? nc + (1 + 2 * n) * BA : nullptr; z.z_actor = st.noise_a;
    z.seed = a->cfg.seed; z.counter_ptr = &a->state->noise_counter;
    return z;
}

// Phase 0 in two halves. One GPU (and data parallel without the Lagrange multiplier) runs them back to back. With use_critic_lagrange under
// torch.distributed the host drives them as phases 4 and 5 and sum-all-reduces the statistics block in between (cql.hip, cql_critic_dq_kernel).
static int cql_phase0a(exorl_agent* a, const Step& st, bool split) {
    const auto& cfg = a->cfg;
    hipStream_t s = st.s;
    const int B = cfg.batch, O = cfg.obs_dim, A = cfg.act_dim, W = O + A, n = cfg.n_samples, prec = cfg.precision;
    const int R = (3 * n + 1) * B;
    EXORL_TRY(open_step(a, &st, s));
    const float* Pa = a->flat[EXORL_NET_ACTOR][EXORL_T_PARAM];
    const float* Pc = a->flat[EXORL_NET_CRITIC][EXORL_T_PARAM];
    EXORL_TRY(net_forward(a->actor, Pa, a->sh_actor, a->xa, O, 2 * B, a->fa, true, false, prec, s));      // raw (mu | log_std) on [next_obs; obs]
    EXORL_TRY(cql_build_inputs(a->obs, a->action, a->fa.out, cql_noise(a, st), a->xc_next, a->cql.x_all, B, O, A, n, s));
    EXORL_TRY(net_forward(a->critic, a->flat[EXORL_NET_CRITIC_TARGET][EXORL_T_PARAM], a->sh_target, a->xc_next, W, B, a->ft, false, false,
                          prec, s));                                                                     // cql.py:160
    EXORL_TRY(net_forward(a->critic, Pc, a->sh_critic, a->cql.x_all, W, R, a->fc, true, false, prec, s));     // cql.py:166,179-184 in one pass
    if (split)      // this rank's penalty sums into stats[2], stats[3]
        EXORL_TRY(cql_critic_dq(a->fc.out, a->ft.out, a->reward, a->discount, a->cql.dq_all, a->metrics, B, n, cfg.alpha, a->inv_bg, s,
                                a->cql.sc + 1, &a->state->critic, cfg.target_cql_penalty, 1, a->stats + 2, a->calql.mc_return));
    return 0;
}

static int cql_phase0b(exorl_agent* a, const Step& st, bool split) {
    const auto& cfg = a->cfg;
    hipStream_t s = st.s;
    const int B = cfg.batch, n = cfg.n_samples;
    EXORL_TRY(cql_critic_dq(a->fc.out, a->ft.out, a->reward, a->discount, a->cql.dq_all, a->metrics, B, n, cfg.alpha, a->inv_bg, s,
                            cfg.use_critic_lagrange ? a->cql.sc + 1 : nullptr, &a->state->critic, cfg.target_cql_penalty, split ? 2 : 0, a->stats + 2,
                            a->calql.mc_return));
    return net_grads_from(a, st, net_view(a, EXORL_NET_CRITIC), a->cql.x_all, (3 * n + 1) * B, a->fc, a->cql.dq_all);
}

static int cql_phase0(exorl_agent* a, const Step& st) {
    EXORL_REQUIRE(!(a->cfg.use_critic_lagrange && a->cfg.world_size > 1), "agent_update_phase: CQL with use_critic_lagrange under data parallelism "
                  "runs phase 0 as phases 4 and 5 with a sum-all-reduce of exorl_agent_stats in between");
    EXORL_TRY(cql_phase0a(a, st, false));
    return cql_phase0b(a, st, false);
}
// use_critic_lagrange under data parallelism: phase 0 up to the penalty sums, and from the global penalty on
static int cql_phase4(exorl_agent* a, const Step& st) { return cql_phase0a(a, st, true); }
static int cql_phase5(exorl_agent* a, const Step& st) { return cql_phase0b(a, st, true); }

static int cql_phase1(exorl_agent* a, const Step& st) {
    const auto& cfg = a->cfg;
    hipStream_t s = st.s;
    const int B = cfg.batch, O = cfg.obs_dim, A = cfg.act_dim, W = O + A, prec = cfg.precision;
    EXORL_TRY(opt_step_critic(a, st));
    EXORL_TRY(cql_actor_sample(a->fa.out + (int64_t)B * 2 * A, cql_noise(a, st), a->xc_pi, W, a->stats, B, O, A, s));    // cql.py:237-239
    EXORL_TRY(net_forward(a->critic, a->flat[EXORL_NET_CRITIC][EXORL_T_PARAM], a->sh_critic, a->xc_pi, W, B, a->fc, true, false, prec, s));
    return 0;
}

static int cql_phase2(exorl_agent* a, const Step& st) {
    const auto& cfg = a->cfg;
    hipStream_t s = st.s;
    const int B = cfg.batch, O = cfg.obs_dim, A = cfg.act_dim, W = O + A, H = cfg.hidden_dim, prec = cfg.precision;
    EXORL_TRY(cql_alpha_step(a->cql.sc, a->stats, &a->state->actor, a->metrics, B, A, a->inv_bg, a->fc.out, s));    // cql.py:241-247
    DoutSpec dq{};
    dq.mode = EXORL_DOUT_ACTOR_Q; dq.q = a->fc.out; dq.stats = a->stats; dq.inv_bg = a->inv_bg; dq.use_lambda = 0;
    EXORL_TRY(net_backward(a->critic, a->flat[EXORL_NET_CRITIC][EXORL_T_PARAM], a->sh_critic, nullptr, a->pc, a->xc_pi, W, B, a->fc, dq,
                           a->bc, a->da, O, A, prec, s, st.fk));
    const FwdBufs f = a->fa.rows_from(B, H, 2 * A);
    DoutSpec dm{};
    dm.mode = EXORL_DOUT_CQL_ACTOR; dm.da = a->da; dm.da_nets = a->critic.n_trunks; dm.raw = f.out; dm.z = st.noise_a;
    dm.alpha_ptr = &a->cql.sc->alpha; dm.inv_bg = a->inv_bg; dm.seed = cfg.seed; dm.counter = 4; dm.counter_ptr = &a->state->noise_counter;
    return net_grads(a, st, net_view(a, EXORL_NET_ACTOR), a->xa + (int64_t)B * O, B, f, dm);
}

// ---- IQL: expectile value net, V-target critic, advantage-weighted actor --------------------------------
// Every forward of the step reads the parameters as they were before it, so the four passes are independent of each other and of the three
// optimiser steps, which all come last. Nothing is drawn. Phases 6..9:
//   6  Q'(s, a), Q(s, a), V on [s'; s] (one 2B-row pass), the row kernel (dv, dq, w, metric partials), value backward on the s rows -> value grads
//   7  critic backward from dq -> critic grads
//   8  actor forward on s and the weighted log-likelihood backward (w from the row kernel) -> actor grads
//   9  Adam on value, critic (Polyak target fused into its pass) and actor
static int iql_phase6(exorl_agent* a, const Step& st) {
    const auto& cfg = a->cfg;
    hipStream_t s = st.s;
    const int B = cfg.batch, O = cfg.obs_dim, H = cfg.hidden_dim;
    EXORL_TRY(open_step(a, &st, s));
    const NetView v = net_view(a, EXORL_NET_VALUE);
    EXORL_TRY(twin_forward(a, s, st.fk, a->xc_cur, true));      // the target's and the critic's forwards on (s, a)
    EXORL_TRY(net_forward(v.d, v.P(), v.sh, a->xa, O, 2 * B, a->iql.fv, true, false, cfg.precision, s));      // rows 0..B-1: V(s'), B..2B-1: V(s)
    IqlRowsArgs r{a->ft.out, a->fc.out, a->iql.fv.out + B, a->iql.fv.out, a->reward, a->discount, a->iql.dv, a->dq, a->row_w, a->iql.part, B,
                  a->inv_bg, a->iql.expectile, a->iql.temperature, a->iql.max_weight};
    EXORL_TRY(iql_rows(r, s));
    if (st.metric_kernels) EXORL_TRY(iql_sums(a->iql.part, B, a->inv_bg, nullptr, a->metrics, s));
    return net_grads_from(a, st, v, a->xa + (int64_t)B * O, B, a->iql.fv.rows_from(B, H, 1), a->iql.dv);
}

static int iql_phase7(exorl_agent* a, const Step& st) {
    return net_grads_from(a, st, net_view(a, EXORL_NET_CRITIC), a->xc_cur, a->cfg.batch, a->fc, a->dq);
}

// the obs half, as BC runs it: the only actor forward of the step. actor_loss = -(w * log N(a; mu, std)).mean(): the weighted
// log-likelihood form with IQL's weights (the row kernel left them in row_w)
static int iql_phase8(exorl_agent* a, const Step& st) { return actor_mu_step(a, st, true, a->traits->actor_loss, 0, nullptr, DoutSpec{}); }

static int iql_phase9(exorl_agent* a, const Step& st) {
    // the value net steps with the critic (one step count, exorl_agent_opt_steps): it reads the critic's Adam scalars and has no target
    EXORL_TRY(opt_step(st, net_view(a, EXORL_NET_VALUE), &a->state->critic, nullptr, nullptr));
    EXORL_TRY(opt_step_critic(a, st));
    return phase3(a, st);
}

// ---- FQE: a frozen actor, each critic regressed on its own target ----------------------------------------
// TD3's critic step with the mean action in place of the draw, a target per net in place of the min, and no actor step at all: the actor is read
// (one B-row forward on the next_obs rows, nothing saved for a backward pass) and never written. Nothing is drawn. Phases 10 and 11:
//   10  mu(s') into the target critic's action columns, Q'(s', mu(s')), Q(s, a), the row kernel (dq, metric partials), critic backward -> critic grads
//   11  Adam on the critic with the Polyak target fused into its pass; under a staged capture this last kernel of the step advances the replay counter
static int fqe_phase10(exorl_agent* a, const Step& st) {
    const auto& cfg = a->cfg;
    hipStream_t s = st.s;
    const int B = cfg.batch, O = cfg.obs_dim, A = cfg.act_dim, W = O + A;
    EXORL_TRY(open_step(a, &st, s));            // the actor's step count moves with the critic's; its Adam never runs
    // rows 0..B-1 of the stacked input are next_obs: the actor runs on those alone
    EXORL_TRY(net_forward(a->actor, a->flat[EXORL_NET_ACTOR][EXORL_T_PARAM], a->sh_actor, a->xa, O, B, a->fa, false, true, cfg.precision, s));
    EXORL_TRY(fqe_mean_actions(a->fa.out, a->xc_next + O, W, B, A, s));
    EXORL_TRY(sarsa_rows(a, s));                // the SARSA setting: the dataset's a' over mu(s') where the episode holds it (behaviour Q)
    EXORL_TRY(twin_forward(a, s, st.fk, a->xc_next, true));      // the target's forward on (s', mu(s')) and the critic's on (s, a)
    FqeRowsArgs r{a->ft.out, a->fc.out, a->reward, a->discount, a->dq, a->fqe.part, B, a->inv_bg};
    EXORL_TRY(fqe_rows(r, s));
    if (st.metric_kernels) EXORL_TRY(fqe_sums(a->fqe.part, B, a->inv_bg, nullptr, a->metrics, s));
    if (st.metric_kernels) EXORL_TRY(sarsa_sums(a, s));
    return net_grads_from(a, st, net_view(a, EXORL_NET_CRITIC), a->xc_cur, B, a->fc, a->dq);
}

static int fqe_phase11(exorl_agent* a, const Step& st) { return opt_step_critic(a, st, st.staged ? &a->state->replay_counter : nullptr); }

// ---- PRDC: the BC target is the action of the dataset point nearest to (beta s, mu(s)) ----------------------
// Phase 12, between phases 0 and 1: the query rows from the obs slot and the obs half of phase 0's stacked actor forward (the mu the actor
// step differentiates), the search over the bound table (nn.hip: partial minima per key range, then the merge that also gathers a_nn), and
// nn_dist where the step's metrics are read. a_nn is a constant of the actor step: nothing flows back through the search.
static int prdc_bound(const exorl_agent* a, const char* who) {
    if (a->cfg.kind != EXORL_AGENT_PRDC) return 0;
    EXORL_REQUIRE(a->prdc.replay, "%s: no key table bound (exorl_replay_build_keys, then exorl_agent_set_prdc)", who);
    const ReplayKeys k = replay_keys(a->prdc.replay);
    EXORL_REQUIRE(k.valid && k.epoch == a->prdc.keys.epoch, "%s: the bound key table is stale: the arena, its order or its normaliser changed, or "
                  "the table was rebuilt (exorl_replay_build_keys and exorl_agent_set_prdc again)", who);
    return 0;
}
static int prdc_phase12(exorl_agent* a, const Step& st) {
    const auto& cfg = a->cfg;
    const int B = cfg.batch, O = cfg.obs_dim, A = cfg.act_dim, pitch = prdc_pitch(cfg);      // every driver has checked the binding (prdc_bound)
    EXORL_TRY(nn_query(a->obs, a->fa.out + (int64_t)B * A, a->prdc.keys.beta, B, O, A, pitch, a->prdc.q, st.s));
    NnSearch n{};
    n.keys = a->prdc.keys.ptr; n.n = (int)a->prdc.keys.n; n.pitch = pitch; n.dim = O + A;
    n.q = a->prdc.q; n.q_ld = pitch; n.rows = B; n.plan = a->prdc.plan;
    n.part_d2 = a->prdc.part_d2; n.part_idx = a->prdc.part_idx; n.idx_out = a->prdc.idx; n.d2_out = a->prdc.d2;
    n.a_nn = a->prdc.a_nn; n.act_col0 = O; n.act_dim = A;
    EXORL_TRY(nn_search(n, st.s));
    if (st.metric_kernels) EXORL_TRY(nn_dist(a->prdc.d2, B, a->inv_bg, a->metrics + EXORL_M_NN_DIST, st.s));
    return 0;
}

// ---- the step as a plan -----------------------------------------------------------------------------
// One update is the ordered list of its phases; where the data-parallel step (dp) needs a global batch quantity before the next phase, the plan
// names the exchange that follows (EXORL_AGENT_XCHG_*, each a sum all-reduce), else -1. Both drivers read it: whole_step_body, which runs the
// exchanges on the library's communicator, and through exorl_agent_update_plan the caller that runs them itself (AgentEngine.update_steps).
//   critic gradients   after phase 0, every kind with a critic
//   statistics         after phase 1: TD3+BC's sum |Q| behind lambda (td3_bc.py:154), unless phase 2 reduces it itself on the side stream
//                      (stats_in_phase2); CQL's sum of log pi for the entropy temperature (cql.py:242-243)
//   actor gradients    after phase 2
//   IQL                value, critic and actor gradients after phases 6, 7 and 8; phase 9 steps all three nets
//   FQE                critic gradients after phase 10; phase 11 steps the critic (the actor is frozen)
// CQL's Lagrange multiplier steps on the penalty of the GLOBAL batch inside phase 0 (cql.py:199-213): data parallel, phases 4 and 5 stand for
// phase 0 with the statistics (this rank's penalty sums) exchanged in between.
// All of that is one table per kind: a row is a phase id, the function it means, the exchange behind it and the rule both hang on. agent_plan
// walks the kind's table in order (the rows the configuration runs are the step); run_phase looks an id up in it (a kind accepts exactly its
// table's ids, whether or not this configuration's plan runs them).
using PhaseFn = int (*)(exorl_agent*, const Step&);
enum PhaseRule {
    EVERY_STEP,        // runs in every plan; under dp its exchange follows
    IF_CRITIC,         // ... its exchange only for a kind with a critic (BC's phase 0 leaves no critic gradients)
    IF_LAMBDA,         // ... its exchange only for TD3+BC, and not where phase 2 reduces the statistic itself (stats_in_phase2)
    IF_SPLIT,          // runs only where CQL's phase 0 is split (use_critic_lagrange under dp); its exchange follows
    UNLESS_SPLIT,      // runs where it is not; under dp its exchange follows
};
struct PhaseRow { int id; PhaseFn fn; int xchg; PhaseRule rule; };
struct PhaseTable { const char* owner; const char* ids; const PhaseRow* rows; int n; };
static const PhaseRow DDPG_ROWS[] = {         // TD3+BC, TD3, BC, DDPG, CRR, APS (BC's phase 1 is a no-op)
    {0, phase0, EXORL_AGENT_XCHG_CRITIC_GRAD, IF_CRITIC},
    {1, phase1, EXORL_AGENT_XCHG_STATS, IF_LAMBDA},
    {2, phase2, EXORL_AGENT_XCHG_ACTOR_GRAD, EVERY_STEP},
    {3, phase3, -1, EVERY_STEP},
};
static const PhaseRow CQL_ROWS[] = {
    {4, cql_phase4, EXORL_AGENT_XCHG_STATS, IF_SPLIT},
    {5, cql_phase5, EXORL_AGENT_XCHG_CRITIC_GRAD, IF_SPLIT},
    {0, cql_phase0, EXORL_AGENT_XCHG_CRITIC_GRAD, UNLESS_SPLIT},
    {1, cql_phase1, EXORL_AGENT_XCHG_STATS, EVERY_STEP},
    {2, cql_phase2, EXORL_AGENT_XCHG_ACTOR_GRAD, EVERY_STEP},
    {3, phase3, -1, EVERY_STEP},
};
static const PhaseRow IQL_ROWS[] = {          // three gradient sums and no batch statistic
    {6, iql_phase6, EXORL_AGENT_XCHG_VALUE_GRAD, EVERY_STEP},
    {7, iql_phase7, EXORL_AGENT_XCHG_CRITIC_GRAD, EVERY_STEP},
    {8, iql_phase8, EXORL_AGENT_XCHG_ACTOR_GRAD, EVERY_STEP},
    {9, iql_phase9, -1, EVERY_STEP},
};
static const PhaseRow FQE_ROWS[] = {
    {10, fqe_phase10, EXORL_AGENT_XCHG_CRITIC_GRAD, EVERY_STEP},
    {11, fqe_phase11, -1, EVERY_STEP},
};
static const PhaseRow PRDC_ROWS[] = {         // TD3+BC's with the search behind phase 0; one process only, so no exchange is ever named
    {0, phase0, EXORL_AGENT_XCHG_CRITIC_GRAD, IF_CRITIC},
    {12, prdc_phase12, -1, EVERY_STEP},
    {1, phase1, EXORL_AGENT_XCHG_STATS, IF_LAMBDA},
    {2, phase2, EXORL_AGENT_XCHG_ACTOR_GRAD, EVERY_STEP},
    {3, phase3, -1, EVERY_STEP},
};
template <int N>
static constexpr PhaseTable phase_rows(const char* owner, const char* ids, const PhaseRow (&rows)[N]) { return PhaseTable{owner, ids, rows, N}; }
static const PhaseTable DDPG_PLAN = phase_rows("the DDPG family", "0..3", DDPG_ROWS), CQL_PLAN = phase_rows("CQL", "0..5", CQL_ROWS),
                        IQL_PLAN = phase_rows("IQL", "6..9", IQL_ROWS), FQE_PLAN = phase_rows("FQE", "10, 11", FQE_ROWS),
                        PRDC_PLAN = phase_rows("PRDC", "0..3, 12", PRDC_ROWS);

// ---- the kinds ----------------------------------------------------------------------------------------
// A kind's own configuration checks (KindTraits::check). use_critic_lagrange is refused for every kind but CQL; it sits in these functions, not
// in check_cfg, because its place among a kind's refusals is part of the interface: behind APS's check, in front of CRR's.
static int check_plain(const exorl_agent_cfg& c) {
    EXORL_REQUIRE(!c.use_critic_lagrange, "agent: use_critic_lagrange is a CQL option");
    return 0;
}
static int check_aps(const exorl_agent_cfg& c) {
    EXORL_REQUIRE(c.sf_dim >= 1 && c.sf_dim <= 16 && c.sf_dim < c.obs_dim,
                  "agent: APS needs 1 <= sf_dim <= 16 and obs_dim = observation + sf_dim (got sf_dim=%d obs_dim=%d)", c.sf_dim, c.obs_dim);
    return check_plain(c);
}
static int check_cql(const exorl_agent_cfg& c) {
    EXORL_REQUIRE(c.n_samples >= 1 && c.n_samples <= 16 && c.act_dim <= 16, "agent: CQL needs 1 <= n_samples <= 16 and action_dim <= 16 (got %d, %d)",
                  c.n_samples, c.act_dim);
    return 0;
}
static int check_crr(const exorl_agent_cfg& c) {
    EXORL_TRY(check_plain(c));
    EXORL_REQUIRE(c.num_value_samples >= 1 && c.num_value_samples <= 64 && c.weight_func >= EXORL_CRR_IDENTITY && c.weight_func <= EXORL_CRR_EXP,
                  "agent: CRR needs 1 <= num_value_samples <= 64 and a valid weight_func (got %d, %d)", c.num_value_samples, c.weight_func);
    return 0;
}
constexpr ActorLoss Q_BC = ACTOR_LOSS_Q_BC, Q = ACTOR_LOSS_Q, BC = ACTOR_LOSS_BC, WLL = ACTOR_LOSS_WLL;
static const char PRDC_ONE_PROCESS[] = "PRDC searches the whole dataset on every step and a rank's shard is not the dataset";
// Columns as KindTraits declares them. FQE's actor is frozen: its loss form is never read. Ids 7 and 10 are not agents of this library.
static const KindTraits KINDS[] = {
    //                             critic actor sf     value  draws  uses          bc             logs           metric one
    // kind              name      trunks outs  heads  net    noise  stddev loss   nearest qfuse  logprob eval   window process           plan        check
    {EXORL_AGENT_TD3_BC, "TD3+BC", 2,     1,    false, false, true,  true,  Q_BC,  false,  true,  false,  true,  true,  nullptr,          &DDPG_PLAN, check_plain},
    {EXORL_AGENT_TD3,    "TD3",    2,     1,    false, false, true,  true,  Q,     false,  true,  false,  true,  true,  nullptr,          &DDPG_PLAN, check_plain},
    {EXORL_AGENT_BC,     "BC",     0,     1,    false, false, true,  true,  BC,    false,  false, false,  true,  true,  nullptr,          &DDPG_PLAN, check_plain},
    {EXORL_AGENT_DDPG,   "DDPG",   1,     1,    false, false, true,  true,  Q,     false,  true,  true,   false, true,  nullptr,          &DDPG_PLAN, check_plain},
    {EXORL_AGENT_CRR,    "CRR",    2,     1,    false, false, true,  true,  WLL,   false,  false, false,  true,  true,  nullptr,          &DDPG_PLAN, check_crr},
    {EXORL_AGENT_CQL,    "CQL",    2,     2,    false, false, true,  false, Q,     false,  false, false,  true,  true,  nullptr,          &CQL_PLAN,  check_cql},
    {EXORL_AGENT_APS,    "APS",    1,     1,    true,  false, true,  true,  Q,     false,  false, true,   false, true,  nullptr,          &DDPG_PLAN, check_aps},
    {EXORL_AGENT_IQL,    "IQL",    2,     1,    false, true,  false, true,  WLL,   false,  false, false,  false, false, nullptr,          &IQL_PLAN,  check_plain},
    {EXORL_AGENT_FQE,    "FQE",    2,     1,    false, false, false, true,  Q,     false,  false, false,  false, false, nullptr,          &FQE_PLAN,  check_plain},
    {EXORL_AGENT_PRDC,   "PRDC",   2,     1,    false, false, true,  true,  Q_BC,  true,   true,  false,  false, false, PRDC_ONE_PROCESS, &PRDC_PLAN, check_plain},
};
static const KindTraits* traits_of(int kind) {
    for (const KindTraits& k : KINDS)
        if (k.kind == kind) return &k;
    return nullptr;
}
static const PhaseRow* find_phase(const PhaseTable& t, int id) {
    for (int i = 0; i < t.n; ++i)
        if (t.rows[i].id == id) return &t.rows[i];
    return nullptr;
}

struct AgentPlan {
    int n = 0;
    int phase[6], xchg[6];         // xchg: the exchange that follows the phase, or -1
};
static AgentPlan agent_plan(const exorl_agent_cfg& c, bool dp, bool stats_in_phase2) {
    const KindTraits& k = *traits_of(c.kind);
    const bool split = dp && c.use_critic_lagrange;      // a CQL option (check_cfg): the only table with IF_SPLIT rows
    const PhaseTable& t = *k.plan;
    AgentPlan p;
    for (int i = 0; i < t.n; ++i) {
        const PhaseRow& r = t.rows[i];
        if (r.rule == (split ? UNLESS_SPLIT : IF_SPLIT)) continue;
        const bool on = r.rule == IF_CRITIC ? k.has_critic() : r.rule == IF_LAMBDA ? k.uses_lambda() && !stats_in_phase2 : true;
        p.phase[p.n] = r.id;
        p.xchg[p.n++] = dp && on ? r.xchg : -1;
    }
    return p;
}

static int run_phase(exorl_agent* a, const Step& st, int phase) {
    const PhaseTable& t = *a->traits->plan;
    if (const PhaseRow* r = find_phase(t, phase)) return r->fn(a, st);
    const PhaseTable* owner = nullptr;       // whose phase it is, if anybody's: the first table in kind order that has it
    for (const KindTraits& k : KINDS)
        if (!owner && find_phase(*k.plan, phase)) owner = k.plan;
    if (owner)
        set_error("agent_update_phase: phase %d out of range for kind %d: it is not one of %s's (%s, exorl_agent_update_plan); phase %d is %s's",
                  phase, a->cfg.kind, t.owner, t.ids, phase, owner->owner);
    else
        set_error("agent_update_phase: phase %d out of range for kind %d: it is not one of %s's (%s, exorl_agent_update_plan)", phase,
                  a->cfg.kind, t.owner, t.ids);
    return 2;
}

// What exchange `xid` (EXORL_AGENT_XCHG_*) sum-all-reduces: the statistics block, or a net's flat gradients.
struct Exchange { float* ptr; int64_t count; };
static Exchange exchange_of(exorl_agent* a, int xid) {
    static const int net[] = {EXORL_NET_CRITIC, -1, EXORL_NET_ACTOR, EXORL_NET_VALUE};      // by EXORL_AGENT_XCHG_*; -1: the statistics
    static_assert(EXORL_AGENT_XCHG_CRITIC_GRAD == 0 && EXORL_AGENT_XCHG_STATS == 1 && EXORL_AGENT_XCHG_ACTOR_GRAD == 2 &&
                  EXORL_AGENT_XCHG_VALUE_GRAD == 3, "exchange_of: the table is indexed by exchange id");
    if (net[xid] < 0) return Exchange{a->stats, 4};
    const NetView n = net_view(a, net[xid]);
    return Exchange{n.G(), n.d.total};
}

// the kernels read the exploration std from the device step state; enqueue a new value only when the schedule moved (a captured graph is
// std-agnostic: exorl_agent_step_graph writes it before the launch)
static int push_stddev(exorl_agent* a, const char* who, float stddev, hipStream_t s) {
    EXORL_REQUIRE(stddev > 0.f || !a->traits->uses_stddev, "%s: stddev must be > 0", who);
    if (a->traits->uses_stddev && stddev != a->dev_stddev) {
        EXORL_TRY(set_device_float(&a->state->stddev, stddev, s));
        a->dev_stddev = stddev;
    }
    return 0;
}

// One whole update, eager (exorl_agent_update) or under capture: the plan's phases, each followed by its exchange on the library's communicator.
// one GPU: nothing is exchanged between the phases, the optimiser launches reduce the gradient partials themselves.
// data parallel: gradients are finalised into the flat buffers, sum-all-reduced over RCCL on this stream, then stepped.
static int whole_step_body(exorl_agent* a, const Step& st) {
    const AgentPlan p = agent_plan(a->cfg, a->comm != nullptr, st.stats_in_phase2);
    for (int i = 0; i < p.n; ++i) {
        EXORL_TRY(run_phase(a, st, p.phase[i]));
        if (p.xchg[i] < 0) continue;
        const Exchange x = exchange_of(a, p.xchg[i]);
        EXORL_TRY(comm_allreduce_sum(a->comm, x.ptr, x.count, st.s));
    }
    if (a->win_sums) EXORL_TRY(run_metrics_window(a, st));      // the step's metrics into the window (and, on the fused path, into a->metrics)
    return 0;
}

// A sum window is a caller's device buffer: [double sums (and, the metric window, an int64 count behind them) | pad to WIN_HEAD_BYTES][per-chunk
// partials]. The metric window, the evaluation's and FQE's value pass each have one; attaching and reading is the same for all three.
// attach_window: `need` bytes, 256-byte aligned, refused in `who`'s name; clears the head (an empty window: the partials behind it are written
// before they are read) and hands out the two parts. buf_dev == nullptr detaches; a refused buffer leaves the window as it was.
template <typename Part>
static int attach_window(const char* who, void* buf_dev, size_t bytes, size_t need, double** sums, Part** part) {
    if (!buf_dev) { *sums = nullptr; *part = nullptr; return 0; }
    EXORL_REQUIRE(bytes >= need && (uintptr_t)buf_dev % 256 == 0, "%s: buffer %zu B (need %zu B, 256-byte aligned)", who, bytes, need);
    EXORL_CHECK_HIP(hipMemset(buf_dev, 0, WIN_HEAD_BYTES));
    *sums = static_cast<double*>(buf_dev);
    *part = reinterpret_cast<Part*>(static_cast<char*>(buf_dev) + WIN_HEAD_BYTES);
    return 0;
}
// read_window: the n sums and, where count_host is given, the int64 behind them; reset empties what was read. Synchronises the stream.
static int read_window(const double* sums_dev, int n, double* sums_host, int64_t* count_host, int reset, hipStream_t s) {
    struct { double sums[WIN_HEAD_BYTES / sizeof(double) - 1]; long long count; } host;
    const size_t bytes = n * sizeof(double) + (count_host ? sizeof(long long) : 0);
    EXORL_CHECK_HIP(hipMemcpyAsync(&host, sums_dev, bytes, hipMemcpyDeviceToHost, s));
    if (reset) EXORL_CHECK_HIP(hipMemsetAsync(const_cast<double*>(sums_dev), 0, bytes, s));
    EXORL_CHECK_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < n; ++i) sums_host[i] = host.sums[i];
    if (count_host) memcpy(count_host, &host.sums[n], sizeof(long long));
    return 0;
}

static int release_graph(exorl_agent* a) {
    if (a->graph_exec) { EXORL_CHECK_HIP(hipGraphExecDestroy(a->graph_exec)); a->graph_exec = nullptr; }
    if (a->graph) { EXORL_CHECK_HIP(hipGraphDestroy(a->graph)); a->graph = nullptr; }
    a->graph_replay = nullptr;
    a->graph_intr = nullptr;
    return 0;
}

}  // namespace exorl

extern "C" {

size_t exorl_agent_workspace_bytes(const exorl_agent_cfg* cfg) {
    exorl_agent tmp;
    if (describe(&tmp, cfg) != 0) return 0;
    Carver c(nullptr);
    carve(&tmp, c);
    return (size_t)c.off * sizeof(float);
}

int exorl_agent_create(const exorl_agent_cfg* cfg, void* workspace, size_t workspace_bytes, exorl_agent_t** out) {
    EXORL_REQUIRE(out, "agent_create: null out");
    auto* a = new exorl_agent();
    if (int rc = describe(a, cfg)) { delete a; return rc; }
    Carver sizing(nullptr);
    carve(a, sizing);
    const size_t need = (size_t)sizing.off * sizeof(float);
    if (workspace) {
        if (workspace_bytes < need || (uintptr_t)workspace % 256 != 0) {
            set_error("agent_create: workspace %zu B (need %zu B, 256-byte aligned)", workspace_bytes, need);
            delete a;
            return 2;
        }
        a->ws = static_cast<float*>(workspace);
    } else {
        hipError_t e = hipMalloc((void**)&a->ws, need);
        if (e != hipSuccess) { set_error("agent_create: hipMalloc(%zu) -> %s", need, hipGetErrorString(e)); delete a; return 1; }
        a->owns_ws = true;
    }
    a->ws_bytes = need;
    hipError_t e = hipMemset(a->ws, 0, need);
    if (e != hipSuccess) { set_error("agent_create: hipMemset -> %s", hipGetErrorString(e)); if (a->owns_ws) (void)hipFree(a->ws); delete a; return 1; }
    Carver c(a->ws);
    carve(a, c);
    a->spec_actor = shadow_spec(a->actor, a->sh_actor, nullptr);
    if (a->has_critic) a->spec_critic = shadow_spec(a->critic, a->sh_critic, &a->sh_target);
    if (a->has_value) a->iql.spec = shadow_spec(a->value, a->iql.sh, nullptr);
    StepState st{};
    st.lr = dec7(cfg->lr); st.b1 = 0.9; st.b2 = 0.999; st.eps = 1e-8; st.tau = dec7(cfg->tau);      // torch.optim.Adam defaults
    st.has_critic = a->has_critic ? 1 : 0;
    st.no_noise = a->traits->draws_noise ? 0 : 1;
    st.b1t = st.b2t = st.b1t_c = st.b2t_c = 1.0;
    if (a->cql.sc) { CqlScalars sc{0.f, 0.f, 0.f, 1.0f}; (void)hipMemcpy(a->cql.sc, &sc, sizeof(sc), hipMemcpyHostToDevice); }
    e = hipMemcpy(a->state, &st, sizeof(st), hipMemcpyHostToDevice);
    if (e != hipSuccess) { set_error("agent_create: state upload -> %s", hipGetErrorString(e)); if (a->owns_ws) (void)hipFree(a->ws); delete a; return 1; }
    *out = a;
    return 0;
}

int exorl_agent_destroy(exorl_agent_t* a) {
    if (!a) return 0;
    (void)release_graph(a);
    if (a->capture_stream) (void)hipStreamDestroy(a->capture_stream);
    if (a->comm_stream) { (void)hipStreamDestroy(a->comm_stream); (void)hipEventDestroy(a->ev_stats_ready); (void)hipEventDestroy(a->ev_stats_done); }
    if (a->fk.aux) { (void)hipStreamDestroy(a->fk.aux); (void)hipEventDestroy(a->fk.ev_fork); (void)hipEventDestroy(a->fk.ev_join); }
    if (a->owns_ws) (void)hipFree(a->ws);
    delete a;
    return 0;
}

static const NetDesc* net_of(exorl_agent_t* a, int32_t net) { return has_net(a, net) ? &net_view(a, net).d : nullptr; }

int exorl_agent_num_tensors(exorl_agent_t* a, int32_t net, int32_t* n) {
    EXORL_REQUIRE(a && n, "agent_num_tensors: null argument");
    const NetDesc* d = net_of(a, net);
    EXORL_REQUIRE(d, "agent_num_tensors: agent has no net %d", net);
    *n = (int32_t)d->tensors.size();
    return 0;
}

int exorl_agent_tensor(exorl_agent_t* a, int32_t net, int32_t index, int32_t what, void** ptr, int64_t* rows, int64_t* cols) {
    EXORL_REQUIRE(a && ptr && rows && cols, "agent_tensor: null argument");
    const NetDesc* d = net_of(a, net);
    EXORL_REQUIRE(d, "agent_tensor: agent has no net %d", net);
    EXORL_REQUIRE(index >= 0 && index < (int)d->tensors.size(), "agent_tensor: index %d out of range", index);
    EXORL_REQUIRE(what >= 0 && what < 4 && a->flat[net][what], "agent_tensor: net %d has no buffer kind %d", net, what);
    *ptr = a->flat[net][what] + d->tensors[index].off;
    *rows = d->tensors[index].rows;
    *cols = d->tensors[index].cols;
    return 0;
}

int exorl_agent_flat(exorl_agent_t* a, int32_t net, int32_t what, void** ptr, int64_t* numel) {
    EXORL_REQUIRE(a && ptr && numel, "agent_flat: null argument");
    const NetDesc* d = net_of(a, net);
    EXORL_REQUIRE(d && what >= 0 && what < 4 && a->flat[net][what], "agent_flat: no buffer net=%d what=%d", net, what);
    *ptr = a->flat[net][what];
    *numel = d->total;
    return 0;
}

int exorl_agent_params_changed(exorl_agent_t* a, int32_t sync_target, void* stream) {
    EXORL_REQUIRE(a, "agent_params_changed: null handle");
    hipStream_t s = as_stream(stream);
    if (sync_target && a->has_critic)
        EXORL_CHECK_HIP(hipMemcpyAsync(a->flat[EXORL_NET_CRITIC_TARGET][EXORL_T_PARAM], a->flat[EXORL_NET_CRITIC][EXORL_T_PARAM],
                                       a->critic.total * sizeof(float), hipMemcpyDeviceToDevice, s));
    EXORL_TRY(refresh_shadows(a->flat[EXORL_NET_ACTOR][EXORL_T_PARAM], a->actor.total, a->spec_actor, false, s));
    if (a->has_critic) {
        EXORL_TRY(refresh_shadows(a->flat[EXORL_NET_CRITIC][EXORL_T_PARAM], a->critic.total, a->spec_critic, false, s));
        EXORL_TRY(refresh_shadows(a->flat[EXORL_NET_CRITIC_TARGET][EXORL_T_PARAM], a->critic.total, a->spec_critic, true, s));
        EXORL_TRY(refresh_w1_planes(a->critic, a->flat[EXORL_NET_CRITIC][EXORL_T_PARAM], a->sh_critic, s));
        EXORL_TRY(refresh_w1_planes(a->critic, a->flat[EXORL_NET_CRITIC_TARGET][EXORL_T_PARAM], a->sh_target, s));
    }
    EXORL_TRY(refresh_w1_planes(a->actor, a->flat[EXORL_NET_ACTOR][EXORL_T_PARAM], a->sh_actor, s));
    if (a->has_value) {
        EXORL_TRY(refresh_shadows(a->flat[EXORL_NET_VALUE][EXORL_T_PARAM], a->value.total, a->iql.spec, false, s));
        EXORL_TRY(refresh_w1_planes(a->value, a->flat[EXORL_NET_VALUE][EXORL_T_PARAM], a->iql.sh, s));
    }
    return 0;
}

int exorl_agent_batch_slots(exorl_agent_t* a, exorl_batch_out* out) {
    EXORL_REQUIRE(a && out, "agent_batch_slots: null argument");
    const int64_t O = a->cfg.obs_dim, A = a->cfg.act_dim;
    out->obs = a->obs; out->obs_stride = O * 4;
    out->action = a->action; out->action_stride = A;
    out->reward = a->reward; out->discount = a->discount;
    out->next_obs = a->next_obs; out->next_obs_stride = O * 4;
    out->meta = nullptr; out->meta_stride = 0;
    // ReBRAC and the SARSA setting read the column (never both on one handle): while one is set the sampler fills the caller's buffer, otherwise
    // the gather writes neither field
    float* const na = a->rebrac.on ? a->rebrac.next_action : a->sarsa.on ? a->sarsa.next_action : nullptr;
    out->next_action = na;
    out->next_action_stride = na ? A : 0;
    out->next_valid = a->rebrac.on ? a->rebrac.next_valid : a->sarsa.on ? a->sarsa.next_valid : nullptr;
    return 0;
}

int exorl_agent_set_batch(exorl_agent_t* a, const float* obs, const float* action, const float* reward, const float* discount,
                          const float* next_obs, void* stream) {
    EXORL_REQUIRE(a && obs && action && reward && discount && next_obs, "agent_set_batch: null argument");
    hipStream_t s = as_stream(stream);
    const size_t B = a->cfg.batch, O = a->cfg.obs_dim, A = a->cfg.act_dim;
    EXORL_CHECK_HIP(hipMemcpyAsync(a->obs, obs, B * O * 4, hipMemcpyDeviceToDevice, s));
    EXORL_CHECK_HIP(hipMemcpyAsync(a->action, action, B * A * 4, hipMemcpyDeviceToDevice, s));
    EXORL_CHECK_HIP(hipMemcpyAsync(a->reward, reward, B * 4, hipMemcpyDeviceToDevice, s));
    EXORL_CHECK_HIP(hipMemcpyAsync(a->discount, discount, B * 4, hipMemcpyDeviceToDevice, s));
    EXORL_CHECK_HIP(hipMemcpyAsync(a->next_obs, next_obs, B * O * 4, hipMemcpyDeviceToDevice, s));
    return 0;
}

int exorl_agent_update_phase(exorl_agent_t* a, int32_t phase, float stddev, const float* noise_c, const float* noise_a, void* stream) {
    EXORL_REQUIRE(a, "agent_update_phase: null handle");
    EXORL_TRY(prdc_bound(a, "agent_update_phase"));
    hipStream_t s = as_stream(stream);
    EXORL_TRY(push_stddev(a, "agent_update_phase", stddev, s));
    return run_phase(a, make_step(a, s, stddev, noise_c, noise_a, false, false, false, false), phase);
}

int exorl_agent_update(exorl_agent_t* a, float stddev, const float* noise_c, const float* noise_a, void* stream) {
    EXORL_REQUIRE(a, "agent_update: null handle");
    EXORL_REQUIRE(a->cfg.world_size == 1 || a->comm, "agent_update: world_size=%d needs a communicator (exorl_agent_set_comm), or drive "
                  "exorl_agent_update_phase and all-reduce between the phases yourself", a->cfg.world_size);
    EXORL_TRY(prdc_bound(a, "agent_update"));
    hipStream_t s = as_stream(stream);
    EXORL_TRY(push_stddev(a, "agent_update_phase", stddev, s));      // the phased call's prefix: the refusal's text is part of the interface as it is
    return whole_step_body(a, make_step(a, s, stddev, noise_c, noise_a, true, false, false, false));
}

int exorl_agent_update_plan(const exorl_agent_cfg* cfg, int32_t* phases, int32_t* exchanges, int32_t capacity, int32_t* n) {
    EXORL_REQUIRE(cfg && phases && exchanges && n, "agent_update_plan: null argument");
    EXORL_TRY(check_cfg(cfg));
    const AgentPlan p = agent_plan(*cfg, cfg->world_size > 1, false);
    EXORL_REQUIRE(capacity >= p.n, "agent_update_plan: capacity %d, the plan has %d phases", capacity, p.n);
    for (int i = 0; i < p.n; ++i) { phases[i] = p.phase[i]; exchanges[i] = p.xchg[i]; }
    *n = p.n;
    return 0;
}

int exorl_agent_set_comm(exorl_agent_t* a, exorl_comm_t* c) {
    EXORL_REQUIRE(a, "agent_set_comm: null handle");
    EXORL_REQUIRE(!a->graph_exec, "agent_set_comm: disable the captured graph first");
    EXORL_REQUIRE(!c || comm_nranks(c) == a->cfg.world_size, "agent_set_comm: communicator has %d ranks, the agent was built for world_size=%d "
                  "(its means are over batch * world_size)", comm_nranks(c), a->cfg.world_size);
    if (c && !a->comm_stream) {
        EXORL_CHECK_HIP(hipStreamCreateWithFlags(&a->comm_stream, hipStreamNonBlocking));
        EXORL_CHECK_HIP(hipEventCreateWithFlags(&a->ev_stats_ready, hipEventDisableTiming));
        EXORL_CHECK_HIP(hipEventCreateWithFlags(&a->ev_stats_done, hipEventDisableTiming));
    }
    a->comm = c;
    return 0;
}

int exorl_agent_stats_buffer(exorl_agent_t* a, void** ptr, int64_t* numel) {
    EXORL_REQUIRE(a && ptr && numel, "agent_stats_buffer: null argument");
    *ptr = a->stats;
    *numel = 4;
    return 0;
}

// one launch for <= ACT_FAST_ROWS rows of a tanh-mean policy (every agent kind but CQL's tanh-Gaussian); obs / noise on the device or on the host
static bool act_fast_ok(const exorl_agent* a, int n) {
    return a->traits->uses_stddev && act_fast_supported(n, a->cfg.obs_dim, a->cfg.hidden_dim, a->actor.out_dim) && !(tune_variant() & TUNE_ACT_GENERIC);
}
static int act_fast_launch(exorl_agent* a, const float* obs_dev, const float* obs_host, int n, float stddev, int eval_mode, const float* noise_dev,
                           const float* noise_host, float* out, hipStream_t s) {
    EXORL_REQUIRE(eval_mode || stddev > 0.f, "agent_act: stddev must be > 0 in sampling mode");
    const NetDesc& d = a->actor;
    ActFast f{};
    f.x_dev = obs_dev; f.x_host = obs_host; f.w0t = a->sh_actor.w0t; f.P = a->flat[EXORL_NET_ACTOR][EXORL_T_PARAM];
    f.b0 = d.b0; f.g = d.g; f.beta = d.beta; f.W1 = d.W1; f.b1 = d.b1; f.W2 = d.W2; f.b2 = d.b2;
    f.part = a->act_part; f.ticket = a->act_ticket; f.noise_dev = noise_dev; f.noise_host = noise_host;
    f.seed = a->cfg.seed;
    f.counter = (eval_mode || noise_dev || noise_host) ? 0ull : ((1ull << 63) | a->act_noise_counter++);      // act_noise_spec's counter space
    f.out = out; f.stddev = stddev; f.rows = n; f.in_dim = a->cfg.obs_dim; f.H = a->cfg.hidden_dim; f.nout = d.out_dim; f.eval_mode = eval_mode;
    return act_fast(f, s);
}

int exorl_agent_act_host(exorl_agent_t* a, const float* obs_host, int32_t n, float stddev, int32_t eval_mode, const float* noise_host,
                         float* action_out, void* stream) {
    EXORL_REQUIRE(a && obs_host && action_out && n > 0, "agent_act_host: bad arguments");
    EXORL_REQUIRE(act_fast_ok(a, n), "agent_act_host: needs <= %d rows, a tanh-mean policy (not CQL), obs_dim <= 256 and hidden_dim %% 4 == 0; use exorl_agent_act",
                  ACT_FAST_ROWS);
    return act_fast_launch(a, nullptr, obs_host, n, stddev, eval_mode, nullptr, noise_host, action_out, as_stream(stream));
}

int exorl_agent_act(exorl_agent_t* a, const float* obs, int32_t n, float stddev, int32_t eval_mode, const float* noise,
                    float* out, void* stream) {
    EXORL_REQUIRE(a && obs && out && n > 0, "agent_act: bad arguments");
    hipStream_t s = as_stream(stream);
    const int O = a->cfg.obs_dim, A = a->cfg.act_dim;
    if (act_fast_ok(a, n)) return act_fast_launch(a, obs, nullptr, n, stddev, eval_mode, noise, nullptr, out, s);
    for (int r0 = 0; r0 < n; r0 += ACT_ROWS) {
        const int rows = n - r0 < ACT_ROWS ? n - r0 : ACT_ROWS;
        WeightImages sh = a->sh_actor;              // act() rows do not tile by 64: split-bf16 takes the in-GEMM split here
        sh.w1.lo = sh.w0.lo = nullptr;
        EXORL_TRY(net_forward(a->actor, a->flat[EXORL_NET_ACTOR][EXORL_T_PARAM], sh, obs + (int64_t)r0 * O, O, rows, a->fact, false,
                              a->traits->uses_stddev, a->cfg.precision, s));
        if (!a->traits->uses_stddev) {               // SquashedNormal: mean = tanh(loc), sample = tanh(loc + std z)  (cql.py:122-131)
            EXORL_TRY(cql_act(a->fact.out, noise ? noise + (int64_t)r0 * A : nullptr, a->cfg.seed, (1ull << 63) | a->act_noise_counter++,
                              eval_mode, out + (int64_t)r0 * A, rows, A, s));
        } else if (eval_mode) {
            EXORL_CHECK_HIP(hipMemcpyAsync(out + (int64_t)r0 * A, a->fact.out, (size_t)rows * A * 4, hipMemcpyDeviceToDevice, s));
        } else {
            EXORL_REQUIRE(stddev > 0.f, "agent_act: stddev must be > 0 in sampling mode");
            EXORL_TRY(sample_action(a->fact.out, act_noise_spec(a, noise ? noise + (int64_t)r0 * A : nullptr), stddev, 0.f, 0,
                                    out + (int64_t)r0 * A, A, rows, A, nullptr, s));
        }
    }
    return 0;
}

int exorl_agent_metrics(exorl_agent_t* a, float* host, void* stream) {
    EXORL_REQUIRE(a && host, "agent_metrics: null argument");
    hipStream_t s = as_stream(stream);
    EXORL_CHECK_HIP(hipMemcpyAsync(host, a->metrics, EXORL_N_METRICS * sizeof(float), hipMemcpyDeviceToHost, s));
    EXORL_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}

int exorl_agent_opt_steps(exorl_agent_t* a, int64_t* actor_steps, int64_t* critic_steps) {
    EXORL_REQUIRE(a, "agent_opt_steps: null handle");
    if (actor_steps) *actor_steps = a->actor_t;
    if (critic_steps) *critic_steps = a->critic_t;
    return 0;
}

int exorl_agent_set_opt_steps(exorl_agent_t* a, int64_t actor_steps, int64_t critic_steps) {
    EXORL_REQUIRE(a && actor_steps >= 0 && critic_steps >= 0, "agent_set_opt_steps: bad arguments");
    a->actor_t = actor_steps;
    a->critic_t = critic_steps;
    return push_opt_steps(a);
}

// sample -> [meta columns into the next_obs rows] -> [module step + intrinsic reward] -> the agent's step, captured once
// goal: the gather is the replay's goal path (exorl_replay_set_goal) into [obs | g] slots, the step un-staged on them
static int enable_graph_impl(exorl_agent_t* a, exorl_intr_t* it, const exorl_intr_batch* ib, int32_t meta_dim, exorl_replay_t* r, int32_t nstep,
                             float gamma, float stddev, void* stream, bool goal = false) {
    EXORL_REQUIRE(a && r, "agent_enable_graph: null argument");
    if (goal) {
        const int G = replay_goal_cols(r), O = replay_obs_bytes(r) / 4;
        EXORL_REQUIRE(G > 0, "agent_enable_graph_goal: the replay has no goal rule (exorl_replay_set_goal)");
        EXORL_REQUIRE(O + G == a->cfg.obs_dim, "agent_enable_graph_goal: the replay's %d observation + %d goal columns do not fill the agent's rows "
                      "of obs_dim=%d", O, G, a->cfg.obs_dim);
    }
    // a previous step (eager or a graph launch) may still be running on the caller's stream and reads the buffers the new graph is
    // built over; releasing a graph exec that is executing is not allowed either. Setup call: a full stream sync is fine here.
    EXORL_CHECK_HIP(hipStreamSynchronize(as_stream(stream)));
    EXORL_REQUIRE(a->cfg.world_size == 1 || a->comm, "agent_enable_graph: a data-parallel step needs the library's communicator (exorl_agent_set_comm) to be captured; "
                  "steps whose collectives run in the caller's code are enqueued eagerly");
    EXORL_REQUIRE(stddev > 0.f && nstep >= 1, "agent_enable_graph: bad stddev/nstep");
    EXORL_TRY(prdc_bound(a, "agent_enable_graph"));
    EXORL_REQUIRE(replay_frame_stack(r) == 1, "agent_enable_graph: the arena stacks %d frames per observation (exorl_replay_set_frame_stack): the "
                  "captured step stages its inputs from whole arena rows; sample a frame-stacked arena eagerly", replay_frame_stack(r));
    if (a->calql.on) {      // the captured gather reads the replay's return-to-go column: it must stand, built with this gamma
        const ReplayReturns g = replay_returns(r);
        EXORL_REQUIRE(g.valid && memcmp(&g.gamma, &gamma, sizeof(float)) == 0, "agent_enable_graph: Cal-QL is set (exorl_agent_set_calql) and the replay "
                      "has %s (exorl_replay_build_returns)", g.valid ? "a return-to-go column built with another gamma" : "no return-to-go column, or a stale one");
    }
    EXORL_TRY(release_graph(a));
    if (!a->capture_stream) EXORL_CHECK_HIP(hipStreamCreateWithFlags(&a->capture_stream, hipStreamNonBlocking));
    exorl_batch_out slots;
    EXORL_TRY(exorl_agent_batch_slots(a, &slots));
    const int O_raw = a->cfg.obs_dim - meta_dim;
    if (meta_dim > 0) {          // [obs | meta] rows: the gather fills the obs rows' meta columns, a second kernel the next_obs rows'
        int r_act = 0, r_meta = 0;
        replay_dims(r, &r_act, &r_meta);
        EXORL_REQUIRE(O_raw > 0 && replay_obs_bytes(r) == O_raw * 4 && r_act == a->cfg.act_dim && r_meta == meta_dim,
                      "agent_enable_graph_intr: the replay's rows (%d obs bytes, %d action, %d meta columns) do not fill [obs | meta] rows of "
                      "%d + %d floats and %d actions", replay_obs_bytes(r), r_act, r_meta, O_raw, meta_dim, a->cfg.act_dim);
        slots.meta = a->obs + O_raw;
        slots.meta_stride = a->cfg.obs_dim;
    }
    if (it) {
        EXORL_REQUIRE(ib && ib->reward_out == a->reward && (!ib->extr_reward || ib->extr_reward == a->reward),
                      "agent_enable_graph_intr: the module writes its reward into the agent's reward slot");
        EXORL_TRY(intr_graph_prepare(it, ib, a->capture_stream));
    }
    // what a sample call would do on the host side (episode table upload, pair buffer, nstep vs episode lengths) — no draw is spent
    EXORL_TRY(replay_prepare(r, a->cfg.batch, nstep, a->capture_stream));
    const uint64_t ctr = replay_philox_counter(r);
    EXORL_CHECK_HIP(hipMemcpyAsync(&a->state->replay_counter, &ctr, sizeof(ctr), hipMemcpyHostToDevice, a->capture_stream));
    EXORL_TRY(set_device_float(&a->state->stddev, stddev, a->capture_stream));
    a->dev_stddev = stddev;
    EXORL_CHECK_HIP(hipStreamSynchronize(a->capture_stream));
    const int64_t t_a = a->actor_t, t_c = a->critic_t;
    if (!a->fk.aux) {
        EXORL_CHECK_HIP(hipStreamCreateWithFlags(&a->fk.aux, hipStreamNonBlocking));
        EXORL_CHECK_HIP(hipEventCreateWithFlags(&a->fk.ev_fork, hipEventDisableTiming));
        EXORL_CHECK_HIP(hipEventCreateWithFlags(&a->fk.ev_join, hipEventDisableTiming));
    }
    EXORL_CHECK_HIP(hipStreamBeginCapture(a->capture_stream, hipStreamCaptureModeThreadLocal));
    // fp32 state observations: the gather kernel writes the networks' staged inputs itself and runs step_begin_device (one kernel
    // boundary less per step); the replay counter is then advanced by the step's last kernel (the actor's optimiser pass)
    StageOut stage{a->xa, a->xc_cur, a->xc_next, a->xc_pi, a->cfg.obs_dim, a->cfg.act_dim, a->cfg.batch, a->has_critic ? 1 : 0, a->state};
    const bool staged = replay_obs_bytes(r) == a->cfg.obs_dim * 4;
    const int O_goal = replay_obs_bytes(r) / 4;
    const GoalOut go{nullptr, a->obs + O_goal, a->cfg.obs_dim, a->next_obs + O_goal, a->cfg.obs_dim};
    int rc = replay_sample_impl(r, a->cfg.batch, nstep, gamma, EXORL_SAMPLER_PHILOX, nullptr, &slots, nullptr, a->capture_stream,
                                &a->state->replay_counter, staged ? &stage : nullptr, a->calql.mc_return, goal ? &go : nullptr);
    if (rc == 0 && meta_dim > 0) rc = copy_meta_columns(a->obs, a->next_obs, a->cfg.obs_dim, a->cfg.batch, O_raw, meta_dim, a->capture_stream);
    // the module reads the batch slots and writes the reward slot only: what the sampler staged for the networks (observations and actions)
    // stays valid, and the agent's step reads the reward from its slot after this
    if (rc == 0 && it) rc = intr_graph_capture(it, ib, a->capture_stream);
    // RCCL's all-reduces are captured with the kernels around them
    if (rc == 0) rc = whole_step_body(a, make_step(a, a->capture_stream, stddev, nullptr, nullptr, true, true, staged, a->parallel_branches));
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(a->capture_stream, &g);
    a->actor_t = t_a; a->critic_t = t_c;             // capture enqueued nothing: undo the host-side bookkeeping
    replay_advance_philox(r, (uint64_t)-1);
    if (rc != 0) { if (g) (void)hipGraphDestroy(g); return rc; }
    if (e != hipSuccess) { set_error("agent_enable_graph: hipStreamEndCapture -> %s", hipGetErrorString(e)); return 1; }
    a->graph = g;
    EXORL_CHECK_HIP(hipGraphInstantiate(&a->graph_exec, g, nullptr, nullptr, 0));
    a->graph_replay = r;
    a->graph_weights_epoch = replay_weights_epoch(r);
    a->graph_norm_on = replay_norm_on(r);
    a->graph_goal = goal;
    a->graph_goal_epoch = replay_goal_epoch(r);
    a->graph_gamma = gamma;
    a->graph_replay_ctr = ctr;
    a->graph_intr = it;
    return 0;
}

int exorl_agent_enable_graph(exorl_agent_t* a, exorl_replay_t* r, int32_t nstep, float gamma, float stddev, void* stream) {
    return enable_graph_impl(a, nullptr, nullptr, 0, r, nstep, gamma, stddev, stream);
}

int exorl_agent_enable_graph_goal(exorl_agent_t* a, exorl_replay_t* r, int32_t nstep, float gamma, float stddev, void* stream) {
    return enable_graph_impl(a, nullptr, nullptr, 0, r, nstep, gamma, stddev, stream, true);
}

int exorl_agent_enable_graph_intr(exorl_agent_t* a, exorl_intr_t* intr, const exorl_intr_batch* batch, int32_t meta_dim, exorl_replay_t* r,
                                  int32_t nstep, float gamma, float stddev, void* stream) {
    EXORL_REQUIRE(a, "agent_enable_graph_intr: null argument");
    EXORL_REQUIRE(meta_dim >= 0 && meta_dim < a->cfg.obs_dim, "agent_enable_graph_intr: meta_dim=%d out of range", meta_dim);
    EXORL_REQUIRE(!intr || a->cfg.world_size == 1, "agent_enable_graph_intr: the joint graph is the one-process step");
    EXORL_REQUIRE(!r || !replay_norm_on(r), "agent_enable_graph_intr: the arena has an observation normaliser (exorl_replay_set_obs_norm): the "
                  "reward-free [obs | meta] step trains on raw observations; turn it off (n_cols = 0) first");
    return enable_graph_impl(a, intr, batch, meta_dim, r, nstep, gamma, stddev, stream);
}

int exorl_agent_noise_counter(exorl_agent_t* a, uint64_t* counter_out, void* stream) {
    EXORL_REQUIRE(a && counter_out, "agent_noise_counter: null argument");
    hipStream_t s = as_stream(stream);
    EXORL_CHECK_HIP(hipMemcpyAsync(counter_out, &a->state->noise_counter, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    EXORL_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}

int exorl_debug_agent_poison_scratch(exorl_agent_t* a, void* stream) {
    EXORL_REQUIRE(a, "debug_agent_poison_scratch: null handle");
    hipStream_t s = as_stream(stream);
    exorl_agent layout;              // a second carve over the same configuration: same offsets, nothing of `a` is touched
    EXORL_TRY(describe(&layout, &a->cfg));
    std::vector<std::pair<int64_t, int64_t>> runs;
    Carver c(nullptr);
    c.fill = &runs;
    carve(&layout, c);
    EXORL_REQUIRE((size_t)c.off * sizeof(float) == a->ws_bytes, "debug_agent_poison_scratch: layout mismatch");
    for (const auto& r : runs) EXORL_CHECK_HIP(hipMemsetAsync(a->ws + r.first, 0xFF, (size_t)r.second * sizeof(float), s));
    return 0;
}

int exorl_debug_agent_weight_images(exorl_agent_t* a, int32_t net, exorl_weight_images* out) {
    EXORL_REQUIRE(a && out, "debug_agent_weight_images: null argument");
    const NetDesc* d = net_of(a, net);
    EXORL_REQUIRE(d, "debug_agent_weight_images: agent has no net %d", net);
    const WeightImages& sh = net_view(a, net).sh;
    *out = exorl_weight_images{d->n_trunks, d->n_heads, d->in_dim, d->H, sh.w0t, sh.w0.hi, sh.w0.lo, sh.w1.hi, sh.w1.mid, sh.w1.lo};
    return 0;
}

int exorl_agent_cql_alpha(exorl_agent_t* a, float* host, int32_t set) {
    EXORL_REQUIRE(a && host && a->cql.sc, "agent_cql_alpha: not a CQL agent / null argument");
    const int nsc = a->cfg.use_critic_lagrange ? 2 : 1;      // [1] = log_critic_alpha (cql.py:103-105)
    for (int i = 0; i < nsc; ++i) {
        float* h = host + 3 * i;
        if (set) {
            CqlScalars sc{h[0], h[1], h[2], expf(h[0])};
            EXORL_CHECK_HIP(hipMemcpy(a->cql.sc + i, &sc, sizeof(sc), hipMemcpyHostToDevice));
        } else {
            CqlScalars sc;
            EXORL_CHECK_HIP(hipMemcpy(&sc, a->cql.sc + i, sizeof(sc), hipMemcpyDeviceToHost));
            h[0] = sc.log_alpha; h[1] = sc.m; h[2] = sc.v;
        }
    }
    return 0;
}

int exorl_agent_set_iql(exorl_agent_t* a, float expectile, float temperature, float max_weight) {
    // the values first: a bad triple is refused whatever the handle is (NaN fails every comparison)
    EXORL_REQUIRE(expectile > 0.f && expectile < 1.f && temperature >= 0.f && max_weight > 0.f,
                  "agent_set_iql: needs 0 < expectile < 1, temperature >= 0 and max_weight > 0 (got %g, %g, %g)", expectile, temperature, max_weight);
    EXORL_REQUIRE(a, "agent_set_iql: null handle");
    EXORL_REQUIRE(a->cfg.kind == EXORL_AGENT_IQL, "agent_set_iql: kind %d is not IQL", a->cfg.kind);
    EXORL_REQUIRE(!a->graph_exec, "agent_set_iql: disable the captured graph first (it holds the values as kernel arguments)");
    a->iql.expectile = expectile; a->iql.temperature = temperature; a->iql.max_weight = max_weight;
    return 0;
}

int exorl_agent_set_prdc(exorl_agent_t* a, exorl_replay_t* r, float beta) {
    EXORL_REQUIRE(a && r, "agent_set_prdc: null argument");
    EXORL_REQUIRE(a->cfg.kind == EXORL_AGENT_PRDC, "agent_set_prdc: kind %d is not PRDC", a->cfg.kind);
    EXORL_REQUIRE(!a->graph_exec, "agent_set_prdc: disable the captured graph first (it holds the table's pointer, row count and key ranges)");
    const ReplayKeys k = replay_keys(r);
    EXORL_REQUIRE(k.valid, "agent_set_prdc: the replay has no key table, or a stale one: the arena, its order or its normaliser changed since "
                  "exorl_replay_build_keys (call it again)");
    EXORL_REQUIRE(k.obs_cols == a->cfg.obs_dim && k.act_dim == a->cfg.act_dim, "agent_set_prdc: the table's keys are %d observation + %d action "
                  "columns, the agent's %d + %d", k.obs_cols, k.act_dim, a->cfg.obs_dim, a->cfg.act_dim);
    EXORL_REQUIRE(k.beta == beta, "agent_set_prdc: the table was built with beta=%g, not %g", k.beta, beta);
    int cus = 0;
    EXORL_TRY(nn_device_cus(&cus));
    a->prdc.replay = r;
    a->prdc.keys = k;
    a->prdc.plan = nn_plan((int)k.n, a->cfg.batch, 0, cus);      // fixed here, not per call: a captured graph replays the same launches
    return 0;
}

int exorl_agent_nn_result(exorl_agent_t* a, void** idx_dev, void** d2_dev, void** a_nn_dev, int32_t* splits) {
    EXORL_REQUIRE(a && idx_dev && d2_dev && a_nn_dev, "agent_nn_result: null argument");
    EXORL_REQUIRE(a->cfg.kind == EXORL_AGENT_PRDC, "agent_nn_result: kind %d is not PRDC", a->cfg.kind);
    *idx_dev = a->prdc.idx; *d2_dev = a->prdc.d2; *a_nn_dev = a->prdc.a_nn;
    if (splits) *splits = a->prdc.replay ? a->prdc.plan.splits : 0;
    return 0;
}

// The ReBRAC buffer's four runs, each padded to 64 floats as every take is: what exorl_agent_rebrac_bytes sizes and exorl_agent_set_rebrac views.
struct RebracViews { float *next_action, *next_valid, *reward, *part; };
static RebracViews rebrac_carve(const exorl_agent_cfg& cfg, SimpleCarver& c) {
    const int64_t B = cfg.batch, A = cfg.act_dim;
    RebracViews v{};
    v.next_action = c.take(B * A); v.next_valid = c.take(B); v.reward = c.take(B); v.part = c.take((int64_t)iql_chunks(cfg.batch) * REBRAC_PARTS);
    return v;
}
static int rebrac_cfg_ok(const exorl_agent_cfg* cfg, const char* who) {
    EXORL_TRY(check_cfg(cfg));
    EXORL_REQUIRE(cfg->kind == EXORL_AGENT_TD3_BC, "%s: kind %d is not TD3+BC (ReBRAC is a setting of that kind)", who, cfg->kind);
    return 0;
}

size_t exorl_agent_rebrac_bytes(const exorl_agent_cfg* cfg) {
    if (rebrac_cfg_ok(cfg, "agent_rebrac_bytes") != 0) return 0;
    SimpleCarver c(nullptr);
    rebrac_carve(*cfg, c);
    return (size_t)c.off * sizeof(float);
}

int exorl_agent_set_rebrac(exorl_agent_t* a, void* buf_dev, size_t bytes, float critic_beta) {
    EXORL_REQUIRE(a, "agent_set_rebrac: null handle");
    EXORL_TRY(rebrac_cfg_ok(&a->cfg, "agent_set_rebrac"));
    EXORL_REQUIRE(!a->graph_exec, "agent_set_rebrac: disable the captured graph first (it holds critic_beta and the buffer's pointers)");
    if (!buf_dev) { a->rebrac = {}; return 0; }      // detach: bytes and critic_beta are not looked at
    EXORL_REQUIRE(critic_beta >= 0.f, "agent_set_rebrac: critic_beta must be >= 0 (got %g)", critic_beta);      // NaN fails the comparison
    EXORL_REQUIRE(!a->sarsa.on, "agent_set_rebrac: the SARSA setting is on (detach it first: exorl_agent_set_sarsa with a null buffer)");
    EXORL_REQUIRE(!a->win_sums && !a->eval_sums, "agent_set_rebrac: ReBRAC has no metric window and no forward-only evaluation: detach the %s first",
                  a->win_sums ? "metric window (exorl_agent_set_metric_window)" : "eval buffer (exorl_agent_set_eval)");
    SimpleCarver c(static_cast<float*>(buf_dev));
    const RebracViews v = rebrac_carve(a->cfg, c);
    const size_t need = (size_t)c.off * sizeof(float);
    EXORL_REQUIRE(bytes >= need && (uintptr_t)buf_dev % 256 == 0, "agent_set_rebrac: buffer %zu B (need %zu B, 256-byte aligned)", bytes, need);
    a->rebrac.next_action = v.next_action; a->rebrac.next_valid = v.next_valid; a->rebrac.reward = v.reward; a->rebrac.part = v.part;
    a->rebrac.beta = critic_beta; a->rebrac.on = true;
    return 0;
}

// The SARSA buffer's three runs, each padded to 64 floats as every take is: what exorl_agent_sarsa_bytes sizes and exorl_agent_set_sarsa views.
struct SarsaViews { float *next_action, *next_valid, *part; };
static SarsaViews sarsa_carve(const exorl_agent_cfg& cfg, SimpleCarver& c) {
    const int64_t B = cfg.batch, A = cfg.act_dim;
    SarsaViews v{};
    v.next_action = c.take(B * A); v.next_valid = c.take(B); v.part = c.take((int64_t)iql_chunks(cfg.batch) * SARSA_PARTS);
    return v;
}
// the kinds whose critic step feeds the target critic one action per row that the setting can replace: phase0's three and FQE
static int sarsa_cfg_ok(const exorl_agent_cfg* cfg, const char* who) {
    EXORL_TRY(check_cfg(cfg));
    const int k = cfg->kind;
    EXORL_REQUIRE(k == EXORL_AGENT_TD3_BC || k == EXORL_AGENT_TD3 || k == EXORL_AGENT_CRR || k == EXORL_AGENT_FQE,
                  "%s: kind %d is not TD3+BC, TD3, CRR or FQE (the SARSA target is a setting of those kinds)", who, k);
    return 0;
}

size_t exorl_agent_sarsa_bytes(const exorl_agent_cfg* cfg) {
    if (sarsa_cfg_ok(cfg, "agent_sarsa_bytes") != 0) return 0;
    SimpleCarver c(nullptr);
    sarsa_carve(*cfg, c);
    return (size_t)c.off * sizeof(float);
}

int exorl_agent_set_sarsa(exorl_agent_t* a, void* buf_dev, size_t bytes) {
    EXORL_REQUIRE(a, "agent_set_sarsa: null handle");
    EXORL_TRY(sarsa_cfg_ok(&a->cfg, "agent_set_sarsa"));
    EXORL_REQUIRE(!a->graph_exec, "agent_set_sarsa: disable the captured graph first (it holds the buffer's pointers)");
    if (!buf_dev) { a->sarsa = {}; return 0; }      // detach: bytes is not looked at
    EXORL_REQUIRE(!a->rebrac.on, "agent_set_sarsa: ReBRAC is set on this handle (detach it first: exorl_agent_set_rebrac with a null buffer)");
    EXORL_REQUIRE(!a->win_sums && !a->eval_sums, "agent_set_sarsa: the SARSA setting has no metric window and no forward-only evaluation: detach the %s first",
                  a->win_sums ? "metric window (exorl_agent_set_metric_window)" : "eval buffer (exorl_agent_set_eval)");
    SimpleCarver c(static_cast<float*>(buf_dev));
    const SarsaViews v = sarsa_carve(a->cfg, c);
    const size_t need = (size_t)c.off * sizeof(float);
    EXORL_REQUIRE(bytes >= need && (uintptr_t)buf_dev % 256 == 0, "agent_set_sarsa: buffer %zu B (need %zu B, 256-byte aligned)", bytes, need);
    a->sarsa.next_action = v.next_action; a->sarsa.next_valid = v.next_valid; a->sarsa.part = v.part;
    a->sarsa.on = true;
    return 0;
}

// Cal-QL's buffer: one run, mc_return (B), padded to 64 floats as every take is.
static int calql_cfg_ok(const exorl_agent_cfg* cfg, const char* who) {
    EXORL_TRY(check_cfg(cfg));
    EXORL_REQUIRE(cfg->kind == EXORL_AGENT_CQL, "%s: kind %d is not CQL (Cal-QL is a setting of that kind)", who, cfg->kind);
    return 0;
}

size_t exorl_agent_calql_bytes(const exorl_agent_cfg* cfg) {
    if (calql_cfg_ok(cfg, "agent_calql_bytes") != 0) return 0;
    SimpleCarver c(nullptr);
    c.take(cfg->batch);
    return (size_t)c.off * sizeof(float);
}

int exorl_agent_set_calql(exorl_agent_t* a, void* buf_dev, size_t bytes) {
    EXORL_REQUIRE(a, "agent_set_calql: null handle");
    EXORL_TRY(calql_cfg_ok(&a->cfg, "agent_set_calql"));
    EXORL_REQUIRE(!a->graph_exec, "agent_set_calql: disable the captured graph first (it holds the buffer's pointer)");
    if (!buf_dev) { a->calql = {}; return 0; }      // detach: bytes is not looked at
    EXORL_REQUIRE(!a->win_sums && !a->eval_sums, "agent_set_calql: Cal-QL has no metric window and no forward-only evaluation: detach the %s first",
                  a->win_sums ? "metric window (exorl_agent_set_metric_window)" : "eval buffer (exorl_agent_set_eval)");
    SimpleCarver c(static_cast<float*>(buf_dev));
    float* const mc = c.take(a->cfg.batch);
    const size_t need = (size_t)c.off * sizeof(float);
    EXORL_REQUIRE(bytes >= need && (uintptr_t)buf_dev % 256 == 0, "agent_set_calql: buffer %zu B (need %zu B, 256-byte aligned)", bytes, need);
    a->calql.mc_return = mc;
    a->calql.on = true;
    return 0;
}

int exorl_agent_set_parallel_branches(exorl_agent_t* a, int32_t enable) {
    EXORL_REQUIRE(a, "agent_set_parallel_branches: null handle");
    EXORL_REQUIRE(!a->graph_exec, "agent_set_parallel_branches: disable the captured graph first");
    a->parallel_branches = enable != 0;
    return 0;
}

int exorl_agent_set_metrics(exorl_agent_t* a, int32_t enable) {
    EXORL_REQUIRE(a, "agent_set_metrics: null handle");
    EXORL_REQUIRE(!a->graph_exec, "agent_set_metrics: disable the captured graph first");
    a->want_metrics = enable != 0;
    return 0;
}

size_t exorl_agent_metric_window_bytes(const exorl_agent_cfg* cfg) {
    if (check_cfg(cfg) != 0) return 0;
    return window_bytes(*cfg);
}

int exorl_agent_set_metric_window(exorl_agent_t* a, void* buf_dev, size_t bytes) {
    EXORL_REQUIRE(a, "agent_set_metric_window: null handle");
    EXORL_REQUIRE(!a->graph_exec, "agent_set_metric_window: disable the captured graph first");
    if (!buf_dev) {
        a->win_steps = nullptr; a->win_bc = nullptr;
        return attach_window("agent_set_metric_window", nullptr, 0, 0, &a->win_sums, &a->win_crit);
    }
    EXORL_REQUIRE(a->traits->metric_window, "agent_set_metric_window: %s has no metric window", a->traits->name);
    EXORL_REQUIRE(!a->rebrac.on, "agent_set_metric_window: ReBRAC has no metric window (detach it first: exorl_agent_set_rebrac with a null buffer)");
    EXORL_REQUIRE(!a->sarsa.on, "agent_set_metric_window: the SARSA setting has no metric window (detach it first: exorl_agent_set_sarsa with a null buffer)");
    EXORL_REQUIRE(!a->calql.on, "agent_set_metric_window: Cal-QL has no metric window (detach it first: exorl_agent_set_calql with a null buffer)");
    EXORL_REQUIRE(a->cfg.world_size == 1, "agent_set_metric_window: the metric window belongs to the one-process step; this agent was built for "
                  "world_size=%d (its metrics are partial means that the caller all-reduces)", a->cfg.world_size);
    EXORL_TRY(attach_window("agent_set_metric_window", buf_dev, bytes, window_bytes(a->cfg), &a->win_sums, &a->win_crit));
    a->win_steps = reinterpret_cast<long long*>(a->win_sums + EXORL_N_METRICS);
    a->win_bc = a->win_crit + 6 * (int64_t)qhead_chunks(a->cfg.batch);
    return 0;
}

int exorl_agent_metric_window_read(exorl_agent_t* a, double* sums_host, int64_t* steps_host, int32_t reset, void* stream) {
    EXORL_REQUIRE(a && sums_host && steps_host, "agent_metric_window_read: null argument");
    EXORL_REQUIRE(a->win_sums, "agent_metric_window_read: no metric window (exorl_agent_set_metric_window)");
    return read_window(a->win_sums, EXORL_N_METRICS, sums_host, steps_host, reset, as_stream(stream));
}

static_assert(EXORL_N_EVAL * sizeof(double) <= WIN_HEAD_BYTES && EXORL_E_ROWS == EVAL_PARTS, "the eval window's sums fit its head; the row count follows the partials");
static size_t eval_bytes(const exorl_agent_cfg& cfg) {
    return WIN_HEAD_BYTES + sizeof(float) * (size_t)round_up((int64_t)EVAL_PARTS * eval_chunks(cfg.batch), 64);
}

size_t exorl_agent_eval_bytes(const exorl_agent_cfg* cfg) {
    if (check_cfg(cfg) != 0) return 0;
    return eval_bytes(*cfg);
}

int exorl_agent_set_eval(exorl_agent_t* a, void* buf_dev, size_t bytes) {
    EXORL_REQUIRE(a, "agent_set_eval: null handle");
    if (!buf_dev) return attach_window("agent_set_eval", nullptr, 0, 0, &a->eval_sums, &a->eval_part);
    EXORL_REQUIRE(a->traits->evaluates, "agent_set_eval: kind %d has no forward-only evaluation (TD3+BC, TD3, CRR, CQL and BC have)", a->cfg.kind);
    EXORL_REQUIRE(!a->rebrac.on, "agent_set_eval: ReBRAC has no forward-only evaluation (detach it first: exorl_agent_set_rebrac with a null buffer)");
    EXORL_REQUIRE(!a->sarsa.on, "agent_set_eval: the SARSA setting has no forward-only evaluation (detach it first: exorl_agent_set_sarsa with a null buffer)");
    EXORL_REQUIRE(!a->calql.on, "agent_set_eval: Cal-QL has no forward-only evaluation (detach it first: exorl_agent_set_calql with a null buffer)");
    return attach_window("agent_set_eval", buf_dev, bytes, eval_bytes(a->cfg), &a->eval_sums, &a->eval_part);
}

// The forwards of phases 0 and 1 with the mean action in place of the draws and nothing saved for a backward pass: same kernels, same routes.
// Writes the staged inputs, forward scratch (fa, ft, fc, dq: takes carve() marks as scratch) and the eval buffer; reads everything else.
int exorl_agent_evaluate(exorl_agent_t* a, void* stream) {
    EXORL_REQUIRE(a, "agent_evaluate: null handle");
    EXORL_REQUIRE(a->traits->evaluates, "agent_evaluate: kind %d has no forward-only evaluation (TD3+BC, TD3, CRR, CQL and BC have)", a->cfg.kind);
    EXORL_REQUIRE(!a->rebrac.on, "agent_evaluate: ReBRAC has no forward-only evaluation (detach it first: exorl_agent_set_rebrac with a null buffer)");
    EXORL_REQUIRE(!a->sarsa.on, "agent_evaluate: the SARSA setting has no forward-only evaluation (detach it first: exorl_agent_set_sarsa with a null buffer)");
    EXORL_REQUIRE(!a->calql.on, "agent_evaluate: Cal-QL has no forward-only evaluation (detach it first: exorl_agent_set_calql with a null buffer)");
    EXORL_REQUIRE(a->eval_sums, "agent_evaluate: no eval buffer (exorl_agent_set_eval)");
    hipStream_t s = as_stream(stream);
    const auto& cfg = a->cfg;
    const int B = cfg.batch, O = cfg.obs_dim, A = cfg.act_dim, W = O + A, H = cfg.hidden_dim, prec = cfg.precision;
    const bool raw = !a->traits->uses_stddev;      // the head holds (mu | log_std) before the tanh
    const int AO = a->actor.out_dim;
    const float* Pa = a->flat[EXORL_NET_ACTOR][EXORL_T_PARAM];
    EXORL_TRY(open_step(a, nullptr, s));         // no step: the inputs are staged, the step state stays where it is
    EvalArgs e{};
    e.mu = a->fa.out + (int64_t)B * AO; e.mu_ld = AO; e.raw = raw ? 1 : 0;
    e.a_data = a->action; e.A = A; e.reward = a->reward; e.discount = a->discount;
    e.part = a->eval_part; e.sums = a->eval_sums; e.rows = B;
    if (!a->has_critic) {          // BC: the obs half alone, as its step runs it (phase 2)
        EXORL_TRY(net_forward(a->actor, Pa, a->sh_actor, a->xa + (int64_t)B * O, O, B, a->fa.rows_from(B, H, AO), false, true, prec, s));
        return eval_reduce(e, s);
    }
    const float* Pc = a->flat[EXORL_NET_CRITIC][EXORL_T_PARAM];
    EXORL_TRY(net_forward(a->actor, Pa, a->sh_actor, a->xa, O, 2 * B, a->fa, false, !raw, prec, s));
    EXORL_TRY(eval_mean_actions(a->fa.out, AO, raw ? 1 : 0, a->xc_next + O, a->xc_pi + O, W, B, A, s));
    // Q'(s', mu(s')) and Q(s, a) as phase 0 launches them; then Q(s, mu(s)) as phase 1 does, its two columns into dq (fc.out holds Q(s, a))
    EXORL_TRY(twin_forward(a, s, Fork{}, a->xc_next, false));
    FwdBufs fpi = a->fc;
    fpi.out = a->dq;
    EXORL_TRY(net_forward(a->critic, Pc, a->sh_critic, a->xc_pi, W, B, fpi, false, false, prec, s));
    e.q_data = a->fc.out; e.q_pi = a->dq; e.tq = a->ft.out;
    return eval_reduce(e, s);
}

int exorl_agent_eval_read(exorl_agent_t* a, double* sums_host, int64_t* rows_host, int32_t reset, void* stream) {
    EXORL_REQUIRE(a && sums_host && rows_host, "agent_eval_read: null argument");
    EXORL_REQUIRE(a->eval_sums, "agent_eval_read: no eval buffer (exorl_agent_set_eval)");
    EXORL_TRY(read_window(a->eval_sums, EXORL_N_EVAL, sums_host, nullptr, reset, as_stream(stream)));
    *rows_host = (int64_t)sums_host[EXORL_E_ROWS];
    return 0;
}

static size_t fqe_value_bytes(const exorl_agent_cfg& cfg) {
    return WIN_HEAD_BYTES + sizeof(double) * (size_t)round_up((int64_t)FQE_VALUE_PARTS * iql_chunks(cfg.batch), 32);
}
static_assert(EXORL_N_FQE_VALUE * sizeof(double) <= WIN_HEAD_BYTES && EXORL_FQE_V_ROWS == FQE_VALUE_PARTS, "the value window's sums fit its head; the row count follows the partials");

size_t exorl_agent_fqe_value_bytes(const exorl_agent_cfg* cfg) {
    if (check_cfg(cfg) != 0 || cfg->kind != EXORL_AGENT_FQE) return 0;
    return fqe_value_bytes(*cfg);
}

int exorl_agent_set_fqe_value(exorl_agent_t* a, void* buf_dev, size_t bytes) {
    EXORL_REQUIRE(a, "agent_set_fqe_value: null handle");
    if (!buf_dev) return attach_window("agent_set_fqe_value", nullptr, 0, 0, &a->fqe.value_sums, &a->fqe.value_part);
    EXORL_REQUIRE(a->cfg.kind == EXORL_AGENT_FQE, "agent_set_fqe_value: kind %d is not FQE", a->cfg.kind);
    return attach_window("agent_set_fqe_value", buf_dev, bytes, fqe_value_bytes(a->cfg), &a->fqe.value_sums, &a->fqe.value_part);
}

// Forward-only, as exorl_agent_evaluate: the inputs are staged with the step state left where it is, the actor runs on the obs rows (the half of
// the stacked buffers BC's step uses), mu(s) goes into xc_pi's action columns and the critic runs on (s, mu(s)) with nothing saved. All B rows
// go through the nets (their kernels are row-wise: a padding row cannot reach another row's output); only rows < `rows` are reduced.
int exorl_agent_fqe_value(exorl_agent_t* a, int32_t rows, void* stream) {
    EXORL_REQUIRE(a, "agent_fqe_value: null handle");
    EXORL_REQUIRE(a->cfg.kind == EXORL_AGENT_FQE, "agent_fqe_value: kind %d is not FQE", a->cfg.kind);
    EXORL_REQUIRE(a->fqe.value_sums, "agent_fqe_value: no value window (exorl_agent_set_fqe_value)");
    EXORL_REQUIRE(rows >= 1 && rows <= a->cfg.batch, "agent_fqe_value: rows=%d outside [1, batch=%d]", rows, a->cfg.batch);
    hipStream_t s = as_stream(stream);
    const auto& cfg = a->cfg;
    const int B = cfg.batch, O = cfg.obs_dim, A = cfg.act_dim, W = O + A, H = cfg.hidden_dim, prec = cfg.precision;
    EXORL_TRY(open_step(a, nullptr, s));
    if (a->sarsa.on) {      // behaviour Q: the critic at the staged (s, a) of the obs and action slots, Q^beta(s0, a0) on episode starts; no actor forward
        EXORL_TRY(net_forward(a->critic, a->flat[EXORL_NET_CRITIC][EXORL_T_PARAM], a->sh_critic, a->xc_cur, W, B, a->fc, false, false, prec, s));
        return fqe_value_reduce(a->fc.out, B, rows, a->fqe.value_part, a->fqe.value_sums, s);
    }
    const FwdBufs f = a->fa.rows_from(B, H, A);
    EXORL_TRY(net_forward(a->actor, a->flat[EXORL_NET_ACTOR][EXORL_T_PARAM], a->sh_actor, a->xa + (int64_t)B * O, O, B, f, false, true, prec, s));
    EXORL_TRY(fqe_mean_actions(f.out, a->xc_pi + O, W, B, A, s));
    EXORL_TRY(net_forward(a->critic, a->flat[EXORL_NET_CRITIC][EXORL_T_PARAM], a->sh_critic, a->xc_pi, W, B, a->fc, false, false, prec, s));
    return fqe_value_reduce(a->fc.out, B, rows, a->fqe.value_part, a->fqe.value_sums, s);
}

int exorl_agent_fqe_value_read(exorl_agent_t* a, double* sums_host, int64_t* rows_host, int32_t reset, void* stream) {
    EXORL_REQUIRE(a && sums_host && rows_host, "agent_fqe_value_read: null argument");
    EXORL_REQUIRE(a->fqe.value_sums, "agent_fqe_value_read: no value window (exorl_agent_set_fqe_value)");
    EXORL_TRY(read_window(a->fqe.value_sums, EXORL_N_FQE_VALUE, sums_host, nullptr, reset, as_stream(stream)));
    *rows_host = (int64_t)sums_host[EXORL_FQE_V_ROWS];
    return 0;
}

int exorl_agent_disable_graph(exorl_agent_t* a) {
    EXORL_REQUIRE(a, "agent_disable_graph: null handle");
    if (a->graph_intr) intr_graph_release(a->graph_intr);
    return release_graph(a);
}

// One captured step: replay sample (Philox) + the kind's whole update plan, one hipGraphLaunch.
int exorl_agent_step_graph(exorl_agent_t* a, float stddev, void* stream) {
    EXORL_REQUIRE(a && a->graph_exec, "agent_step_graph: no captured graph (call exorl_agent_enable_graph)");
    EXORL_TRY(prdc_bound(a, "agent_step_graph"));      // the graph holds the table's pointer, row count and key ranges
    EXORL_TRY(push_stddev(a, "agent_step_graph", stddev, as_stream(stream)));      // schedule moved: one scalar write ahead of the launch, same stream
    EXORL_REQUIRE(replay_weights_epoch(a->graph_replay) == a->graph_weights_epoch, "agent_step_graph: exorl_replay_set_weights was called after "
                  "the capture: the graph samples the table it was captured with (call exorl_agent_enable_graph again)");
    EXORL_REQUIRE(replay_norm_on(a->graph_replay) == a->graph_norm_on, "agent_step_graph: exorl_replay_set_obs_norm switched the "
                  "normaliser %s after the capture: the graph holds the other gather kernel (call exorl_agent_enable_graph again)",
                  a->graph_norm_on ? "off" : "on");
    EXORL_REQUIRE(!a->graph_goal || replay_goal_epoch(a->graph_replay) == a->graph_goal_epoch, "agent_step_graph: exorl_replay_set_goal was called "
                  "after the capture: the graph relabels with the rule it was captured with (call exorl_agent_enable_graph_goal again)");
    if (a->calql.on) {
        const ReplayReturns g = replay_returns(a->graph_replay);
        EXORL_REQUIRE(g.valid && memcmp(&g.gamma, &a->graph_gamma, sizeof(float)) == 0, "agent_step_graph: the replay's return-to-go column is stale "
                      "or was rebuilt with another gamma after the capture: Cal-QL's gather reads it (call exorl_replay_build_returns with the capture's gamma)");
    }
    const uint64_t ctr = replay_philox_counter(a->graph_replay);
    if (ctr != a->graph_replay_ctr) EXORL_TRY(set_device_u64(&a->state->replay_counter, ctr, as_stream(stream)));      // eager batches were drawn in between
    a->graph_replay_ctr = ctr + 1;
    if (a->graph_intr) EXORL_TRY(intr_graph_before_launch(a->graph_intr, as_stream(stream)));      // counters an eager step or a setter moved
    EXORL_CHECK_HIP(hipGraphLaunch(a->graph_exec, as_stream(stream)));
    a->actor_t += 1;
    if (a->has_critic) a->critic_t += 1;
    replay_advance_philox(a->graph_replay, 1);
    if (a->graph_intr) intr_graph_after_launch(a->graph_intr);
    return 0;
}

}  // extern "C"
