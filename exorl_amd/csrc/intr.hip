// Intrinsic-reward modules of the reward-free DDPG-backbone agents (states observations): one optimiser step of
// the module on the sampled batch, then the intrinsic reward of that batch under the updated module, written
// where the DDPG critic update reads its reward. Replaces (file:line in the reference repo):
//   RND      agents/unsupervised_learning/rnd.py:13-60 (module), :79-108 (update_rnd, compute_intr_reward)
//   ICM      agents/unsupervised_learning/icm.py:12-45, :64-92
//   ICM-APT  agents/unsupervised_learning/icm_apt.py:13-57, :86-110; utils.PBE / utils.RMS utils/utils.py:257-319
//   Disagreement agents/unsupervised_learning/disagreement.py:11-47, :64-90
//   DIAYN    agents/unsupervised_learning/diayn.py:15-29, :78-127
//   APS      agents/unsupervised_learning/aps.py:63-79, :147-175 (successor-feature net; PBE + task . phi reward)
//   SMM      agents/unsupervised_learning/smm.py:27-112 (VAE, discriminator), :173-246 (updates, reward)
//   Proto    agents/unsupervised_learning/proto.py:14-157 (sinkhorn_knopp, prototypes, candidate queue, kNN reward)
// The modules are plain Linear/ReLU stacks of arbitrary widths (obs_dim, hidden_dim, rep_dim), so the layers run on
// the generic fp32-source grouped GEMM (gemm.hip) with small row/column kernels around it; what the reference's
// autograd graph hides and this file exploits:
//   * RND's target net is frozen and BatchNorm of the same batch is identical in the reward pass, so the target
//     forward runs once per update instead of twice;
//   * the L2-norm losses' gradients are formed in the same kernel that computes the errors (no separate loss pass);
//   * APT's reward is a top-k over pairwise distances (knn.hip) instead of a (B,B,rep) broadcast temporary.
#include <cmath>
#include <vector>

#include "kernels.h"

namespace exorl {

struct RmsState { float M, S; double n; };          // utils.RMS: running mean / variance / count (n starts at 1e-4)

__device__ __forceinline__ float block_sum(float v, float* red) {      // all threads get the total; red: >= 17 floats
    v = wave_sum(v);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int i = 0; i < nw; ++i) s += red[i];
        red[16] = s;
    }
    __syncthreads();
    return red[16];
}

// nn.BatchNorm1d(affine=False) in training mode, then clamp(+-clip) (rnd.py:24-26,49-50): one block per feature.
__global__ __launch_bounds__(256) void bn_clamp_kernel(const float* __restrict__ x, int64_t ldx, float* __restrict__ out, int rows, int O,
                                                       float clip, float* __restrict__ running /* mean[O] var[O] count */) {
    __shared__ float red[17];
    const int c = blockIdx.x;
    float s = 0.f;
    for (int r = threadIdx.x; r < rows; r += blockDim.x) s += x[(int64_t)r * ldx + c];
    const float mean = block_sum(s, red) / (float)rows;
    float q = 0.f;
    for (int r = threadIdx.x; r < rows; r += blockDim.x) { const float d = x[(int64_t)r * ldx + c] - mean; q += d * d; }
    const float var = block_sum(q, red) / (float)rows;
    const float rstd = 1.0f / sqrtf(var + 1e-5f);
    for (int r = threadIdx.x; r < rows; r += blockDim.x) {
        const float v = (x[(int64_t)r * ldx + c] - mean) * rstd;
        out[(int64_t)r * O + c] = fminf(fmaxf(v, -clip), clip);
    }
    if (threadIdx.x == 0) {                          // momentum 0.1; running_var takes the unbiased estimate
        running[c] = 0.9f * running[c] + 0.1f * mean;
        running[O + c] = 0.9f * running[O + c] + 0.1f * var * ((float)rows / (float)(rows > 1 ? rows - 1 : 1));
        if (c == 0) running[2 * O] += 1.0f;
    }
}

// ---- the same BatchNorm1d over the global batch of a data-parallel step ----------------------------------------------------------------
// Each rank reduces its rows to per-feature (n, mean, M2) — the two passes of bn_clamp_kernel — and the ranks' moments are all-gathered
// (EXORL_INTR_XCHG_BN). Every rank then merges them in rank order in double (Chan et al., as rms_combine_update), so the normalisation and
// the running statistics are the same bits on every rank. mom: [rank][feature][3] doubles.
__global__ __launch_bounds__(256) void bn_moments_kernel(const float* __restrict__ x, int64_t ldx, int rows, int O, double* __restrict__ mom) {
    __shared__ float red[17];
    const int c = blockIdx.x;
    float s = 0.f;
    for (int r = threadIdx.x; r < rows; r += blockDim.x) s += x[(int64_t)r * ldx + c];
    const float mean = block_sum(s, red) / (float)rows;
    float q = 0.f;
    for (int r = threadIdx.x; r < rows; r += blockDim.x) { const float d = x[(int64_t)r * ldx + c] - mean; q += d * d; }
    q = block_sum(q, red);
    if (threadIdx.x == 0) { mom[3 * c] = (double)rows; mom[3 * c + 1] = (double)mean; mom[3 * c + 2] = (double)q; }
}
// normalise this rank's rows with the merged statistics, clamp, and step the running statistics (momentum 0.1, unbiased variance over the
// global batch's rows); every thread merges the `world` triples of its feature itself (a few dozen double operations)
__global__ __launch_bounds__(256) void bn_merged_clamp_kernel(const float* __restrict__ x, int64_t ldx, float* __restrict__ out, int rows, int O,
                                                              float clip, float* __restrict__ running, const double* __restrict__ mom, int world) {
    const int c = blockIdx.x;
    double n = mom[3 * c], dmean = mom[3 * c + 1], m2 = mom[3 * c + 2];
    for (int r = 1; r < world; ++r) {
        const double* m = mom + 3 * ((int64_t)r * O + c);
        const double nr = m[0], d = m[1] - dmean, tot = n + nr;
        dmean += d * nr / tot;
        m2 += m[2] + d * d * n * nr / tot;
        n = tot;
    }
    const float mean = (float)dmean, var = (float)(m2 / n);
    const float rstd = 1.0f / sqrtf(var + 1e-5f);
    for (int r = threadIdx.x; r < rows; r += blockDim.x) {
        const float v = (x[(int64_t)r * ldx + c] - mean) * rstd;
        out[(int64_t)r * O + c] = fminf(fmaxf(v, -clip), clip);
    }
    if (threadIdx.x == 0) {
        running[c] = 0.9f * running[c] + 0.1f * mean;
        running[O + c] = 0.9f * running[O + c] + 0.1f * (float)(m2 / (n > 1.0 ? n - 1.0 : 1.0));
        if (c == 0) running[2 * O] += 1.0f;
    }
}

// dst[r] = [a[r, 0:ca] | b[r, 0:cb]]
__global__ __launch_bounds__(256) void concat2_kernel(const float* __restrict__ a, int64_t lda, int ca, const float* __restrict__ b, int64_t ldb,
                                                      int cb, float* __restrict__ dst, int rows) {
    const int w = ca + cb;
    const int64_t n = (int64_t)rows * w;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / w;
        const int c = (int)(i - r * w);
        dst[i] = c < ca ? a[r * lda + c] : b[r * ldb + (c - ca)];
    }
}

__global__ __launch_bounds__(256) void relu_bwd_kernel(float* __restrict__ d, const float* __restrict__ a, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        d[i] = a[i] > 0.f ? d[i] : 0.f;
}

// err[b] = mean_j (t - p)^2 (rnd.py:54-56); dpred = d(mean_b err)/dp = -2 (t - p) / R / B. One wave per row. grows: the rows the
// loss mean is over (batch * world_size; the gradients are then partial sums the ranks add up)
__global__ __launch_bounds__(256) void rnd_err_kernel(const float* __restrict__ pred, const float* __restrict__ targ, float* __restrict__ err,
                                                      float* __restrict__ dpred, int rows, int R, int grows) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float invR = 1.0f / (float)R, invB = 1.0f / (float)grows;
    float s = 0.f;
    for (int j = lane; j < R; j += 64) {
        const float d = targ[(int64_t)row * R + j] - pred[(int64_t)row * R + j];
        s += d * d;
        if (dpred) dpred[(int64_t)row * R + j] = (-2.0f * d * invR) * invB;
    }
    s = wave_sum(s);
    if (lane == 0) err[row] = s * invR;
}

// out[idx] (+)= sum(x) * scale — single block
__global__ __launch_bounds__(1024) void mean_kernel(const float* __restrict__ x, int n, float scale, float* __restrict__ out, int accumulate) {
    __shared__ float red[17];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) s += x[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) *out = (accumulate ? *out : 0.f) + s * scale;
}

// utils.RMS.__call__ (utils.py:264-276) on n values with batch mean `mean` and unbiased variance `var`; fp32 tensor math
// with the Python-float scalars rounded to fp32 where torch does
__device__ inline void rms_update(RmsState* st, float mean, float var, int bs) {
    const float n = (float)st->n, nb = (float)(st->n + (double)bs), fbs = (float)bs;
    const float delta = mean - st->M;
    const float newM = st->M + delta * fbs / nb;
    const float newS = (st->S * n + var * fbs + delta * delta * n * fbs / nb) / nb;
    st->M = newM; st->S = newS; st->n += (double)bs;
}

// The moments utils.RMS takes of a batch, as every thread of the block gets them: the fp32 mean of val(0..n-1), then the fp32 sum of the
// squared distances from it
template <class V>
__device__ __forceinline__ void block_moments(V val, int n, float* red, float& mean, float& q) {
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) s += val(i);
    mean = block_sum(s, red) / (float)n;
    q = 0.f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) { const float d = val(i) - mean; q += d * d; }
    q = block_sum(q, red);
}

// ---- utils.RMS over the global batch of a data-parallel step (rnd.py:98-103, utils.py:264-276,301-319) -----------------------
// Each rank reduces its own values to (n, mean, M2) with block_moments and the ranks' moments are all-gathered. The combine merges them
// in rank order in double (Chan et al.), so every rank computes the same RMS update bit for bit. Values: RND's per-row error (k = 1,
// avg = 0), or PBE's top-k distances (all B*k with avg, else the k-th of each row).
__global__ __launch_bounds__(1024) void rms_moments_kernel(const float* __restrict__ x, int B, int k, int avg, double* __restrict__ mom) {
    __shared__ float red[17];
    const int n = avg ? B * k : B;
    float mean, q;
    block_moments([&](int i) { return avg ? x[i] : x[(int64_t)i * k + (k - 1)]; }, n, red, mean, q);
    if (threadIdx.x == 0) { mom[0] = (double)n; mom[1] = (double)mean; mom[2] = (double)q; }
}
// merge `world` (n, mean, M2) triples in rank order, then utils.RMS.__call__ with the merged batch mean and unbiased variance
__device__ void rms_combine_update(RmsState* st, const double* __restrict__ mom, int world) {
    double n = mom[0], mean = mom[1], m2 = mom[2];
    for (int r = 1; r < world; ++r) {
        const double nr = mom[3 * r], d = mom[3 * r + 1] - mean, tot = n + nr;
        mean += d * nr / tot;
        m2 += mom[3 * r + 2] + d * d * n * nr / tot;
        n = tot;
    }
    rms_update(st, (float)mean, (float)(m2 / (n > 1.0 ? n - 1.0 : 1.0)), (int)n);
}

// compute_intr_reward (rnd.py:98-103) + the update()'s reward bookkeeping (:131-137) on this rank's B rows of the Bg-row batch: single
// block. mom: the `world` ranks' gathered moments of err, or null with one rank (the kernel takes them itself); metrics are partial
// means over Bg rows
__global__ __launch_bounds__(1024) void rnd_reward_kernel(const float* __restrict__ err, const float* extr, float* reward, int B, int Bg, float scale,
                                                          RmsState* st, const double* __restrict__ mom, int world, float* __restrict__ metrics) {
    __shared__ float red[17];
    __shared__ float sh_S;
    float e = 0.f, mean = 0.f, q = 0.f;
    for (int i = threadIdx.x; i < B; i += blockDim.x) e += extr ? extr[i] : 0.f;
    e = block_sum(e, red);
    if (!mom) block_moments([&](int i) { return err[i]; }, B, red, mean, q);
    if (threadIdx.x == 0) {
        if (mom) rms_combine_update(st, mom, world);
        else rms_update(st, mean, q / (float)(B > 1 ? B - 1 : 1), B);
        sh_S = st->S;
        metrics[EXORL_IM_EXTR_REWARD] = e / (float)Bg;
        metrics[EXORL_IM_RMS_MEAN] = st->M;
        metrics[EXORL_IM_RMS_STD] = sqrtf(st->S);
    }
    __syncthreads();
    const float denom = sqrtf(sh_S) + 1e-8f;
    float rs = 0.f;
    for (int i = threadIdx.x; i < B; i += blockDim.x) {
        const float r = scale * err[i] / denom;
        reward[i] = r;
        rs += r;
    }
    rs = block_sum(rs, red);
    if (threadIdx.x == 0) metrics[EXORL_IM_INTR_REWARD] = rs / (float)Bg;
}

// ICM errors (icm.py:28-45): fe = ||tgt - pred||_2, be = ||a - tanh(apre)||_2 per row, and the gradients of
// mean(fe) + mean(be) w.r.t. pred / apre. One wave per row. apre == nullptr: forward error only (reward pass).
__global__ __launch_bounds__(256) void icm_err_kernel(const float* __restrict__ pred, int D, const float* __restrict__ tgt, int64_t ldt,
                                                      const float* __restrict__ apre, const float* __restrict__ action, int A,
                                                      float* __restrict__ fe, float* __restrict__ be, float* __restrict__ dpred,
                                                      float* __restrict__ dapre, int rows, float invB) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float s = 0.f;
    for (int j = lane; j < D; j += 64) { const float d = tgt[(int64_t)row * ldt + j] - pred[(int64_t)row * D + j]; s += d * d; }
    const float nf = sqrtf(wave_sum(s));
    if (lane == 0) fe[row] = nf;
    if (dpred)
        for (int j = lane; j < D; j += 64) {
            const float d = tgt[(int64_t)row * ldt + j] - pred[(int64_t)row * D + j];
            dpred[(int64_t)row * D + j] = nf > 0.f ? -(d / nf) * invB : 0.f;
        }
    if (!apre) return;
    float ah = 0.f, d = 0.f;
    if (lane < A) { ah = tanhf(apre[(int64_t)row * A + lane]); d = action[(int64_t)row * A + lane] - ah; }
    const float nb = sqrtf(wave_sum(d * d));
    if (lane == 0) be[row] = nb;
    if (dapre && lane < A) dapre[(int64_t)row * A + lane] = nb > 0.f ? (-(d / nb) * invB) * (1.0f - ah * ah) : 0.f;
}

// The same errors for wide rows (pixel encodings: D = 39200): one WORKGROUP per row and 16-byte accesses. With one wave per row a batch of
// 1024 rows is 1024 waves — four per CU — each walking 157 KB twice in 4-byte steps: 440-610 us per call where the 480 MB it moves cost ~100
// (0.9 ms of an ICM update on pixels, 3.1 ms of a Disagreement update). The second pass re-reads the row from L2.
__global__ __launch_bounds__(256) void icm_err_wide_kernel(const float* __restrict__ pred, int D, const float* __restrict__ tgt, int64_t ldt,
                                                           const float* __restrict__ apre, const float* __restrict__ action, int A,
                                                           float* __restrict__ fe, float* __restrict__ be, float* __restrict__ dpred,
                                                           float* __restrict__ dapre, float invB) {
    __shared__ float red[17];
    const int row = blockIdx.x, lane = threadIdx.x & 63, n4 = D >> 2;
    const float4* p4 = reinterpret_cast<const float4*>(pred + (int64_t)row * D);
    const float4* t4 = reinterpret_cast<const float4*>(tgt + (int64_t)row * ldt);
    float s = 0.f;
    for (int j = threadIdx.x; j < n4; j += 256) {
        const float4 t = t4[j], p = p4[j];
        const float dx = t.x - p.x, dy = t.y - p.y, dz = t.z - p.z, dw = t.w - p.w;
        s += (dx * dx + dy * dy) + (dz * dz + dw * dw);
    }
    const float nf = sqrtf(block_sum(s, red));
    if (threadIdx.x == 0) fe[row] = nf;
    if (dpred) {
        float4* g4 = reinterpret_cast<float4*>(dpred + (int64_t)row * D);
        for (int j = threadIdx.x; j < n4; j += 256) {
            const float4 t = t4[j], p = p4[j];
            float4 g;
            g.x = nf > 0.f ? -((t.x - p.x) / nf) * invB : 0.f; g.y = nf > 0.f ? -((t.y - p.y) / nf) * invB : 0.f;
            g.z = nf > 0.f ? -((t.z - p.z) / nf) * invB : 0.f; g.w = nf > 0.f ? -((t.w - p.w) / nf) * invB : 0.f;
            g4[j] = g;
        }
    }
    if (!apre || threadIdx.x >= 64) return;
    float ah = 0.f, d = 0.f;
    if (lane < A) { ah = tanhf(apre[(int64_t)row * A + lane]); d = action[(int64_t)row * A + lane] - ah; }
    const float nb = sqrtf(wave_sum(d * d));
    if (lane == 0) be[row] = nb;
    if (dapre && lane < A) dapre[(int64_t)row * A + lane] = nb > 0.f ? (-(d / nb) * invB) * (1.0f - ah * ah) : 0.f;
}
// one launch of the ICM errors: wide rows take the workgroup-per-row kernel (16-byte alignment of every row of pred / tgt / dpred required)
static void launch_icm_err(const float* pred, int D, const float* tgt, int64_t ldt, const float* apre, const float* action, int A, float* fe, float* be,
                           float* dpred, float* dapre, int rows, float invB, hipStream_t s) {
    const bool wide = D >= 2048 && D % 4 == 0 && ldt % 4 == 0 && reinterpret_cast<uintptr_t>(pred) % 16 == 0 && reinterpret_cast<uintptr_t>(tgt) % 16 == 0 &&
                      (!dpred || reinterpret_cast<uintptr_t>(dpred) % 16 == 0);
    if (wide) hipLaunchKernelGGL(icm_err_wide_kernel, dim3(rows), dim3(256), 0, s, pred, D, tgt, ldt, apre, action, A, fe, be, dpred, dapre, invB);
    else hipLaunchKernelGGL(icm_err_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, s, pred, D, tgt, ldt, apre, action, A, fe, be, dpred, dapre, rows, invB);
}

// reward = log(fe * scale + 1) (icm.py:86-92) + reward bookkeeping; single block
__global__ __launch_bounds__(1024) void icm_reward_kernel(const float* __restrict__ fe, const float* extr, float* reward, int B, float scale,
                                                          float* __restrict__ metrics, int Bg) {
    __shared__ float red[17];
    float e = 0.f;
    for (int i = threadIdx.x; i < B; i += blockDim.x) e += extr ? extr[i] : 0.f;
    e = block_sum(e, red);
    float rs = 0.f;
    for (int i = threadIdx.x; i < B; i += blockDim.x) {
        const float r = logf(fe[i] * scale + 1.0f);
        reward[i] = r;
        rs += r;
    }
    rs = block_sum(rs, red);
    if (threadIdx.x == 0) { metrics[EXORL_IM_EXTR_REWARD] = e / (float)Bg; metrics[EXORL_IM_INTR_REWARD] = rs / (float)Bg; }
}

// utils.PBE.__call__ after the top-k (utils.py:301-319) on this rank's B rows of the Bg-row batch: topk (B,k) ascending, against the whole
// batch; single block. mom as in rnd_reward_kernel (read only with use_rms)
__global__ __launch_bounds__(1024) void pbe_reward_kernel(const float* __restrict__ topk, const float* extr, float* reward, int B, int Bg, int k,
                                                          int avg, int use_rms, float clip, RmsState* st, const double* __restrict__ mom, int world,
                                                          float* __restrict__ metrics) {
    __shared__ float red[17];
    __shared__ float sh_M;
    float e = 0.f;
    for (int i = threadIdx.x; i < B; i += blockDim.x) e += extr ? extr[i] : 0.f;
    e = block_sum(e, red);
    float M = 1.0f;
    if (use_rms) {
        const int n = avg ? B * k : B;
        float mean = 0.f, q = 0.f;
        if (!mom) block_moments([&](int i) { return avg ? topk[i] : topk[(int64_t)i * k + (k - 1)]; }, n, red, mean, q);
        if (threadIdx.x == 0) {
            if (mom) rms_combine_update(st, mom, world);
            else rms_update(st, mean, q / (float)(n > 1 ? n - 1 : 1), n);
            sh_M = st->M;
        }
        __syncthreads();
        M = sh_M;
    }
    float rs = 0.f;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        float r;
        if (avg) {
            float acc = 0.f;
            for (int j = 0; j < k; ++j) {
                float v = topk[(int64_t)b * k + j];
                if (use_rms) v = v / M;
                if (clip >= 0.f) v = fmaxf(v - clip, 0.f);
                acc += v;
            }
            r = acc / (float)k;
        } else {
            r = topk[(int64_t)b * k + (k - 1)];
            if (use_rms) r = r / M;
            if (clip >= 0.f) r = fmaxf(r - clip, 0.f);
        }
        r = logf(r + 1.0f);
        reward[b] = r;
        rs += r;
    }
    rs = block_sum(rs, red);
    if (threadIdx.x == 0) {
        metrics[EXORL_IM_EXTR_REWARD] = e / (float)Bg;
        metrics[EXORL_IM_INTR_REWARD] = rs / (float)Bg;
        metrics[EXORL_IM_RMS_MEAN] = st->M;
        metrics[EXORL_IM_RMS_STD] = sqrtf(st->S);
    }
}

// gradient reaching the trunk output of [obs; next_obs] (icm_apt.py:36-39): rows 0..B-1 from both nets' inputs,
// rows B..2B-1 from the inverse model's input and from being the forward model's regression target (= -dnhat)
__global__ __launch_bounds__(256) void apt_drep_kernel(const float* __restrict__ dxf, int64_t ldf, const float* __restrict__ dxb, int64_t ldb,
                                                       const float* __restrict__ dnhat, float* __restrict__ drep, int B, int R) {
    const int64_t n = (int64_t)B * R;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / R;
        const int c = (int)(i - r * R);
        drep[i] = dxf[r * ldf + c] + dxb[r * ldb + c];
        drep[n + i] = dxb[r * ldb + R + c] - dnhat[i];
    }
}

// d(loss)/d(obs) of plain ICM (icm.py:27-45): obs feeds the forward model's and the inverse model's input; dst is dense (B, O)
__global__ __launch_bounds__(256) void icm_dobs_kernel(const float* __restrict__ dxf, int64_t ldf, const float* __restrict__ dxb, int64_t ldb,
                                                       float* __restrict__ dst, int B, int O) {
    const int64_t n = (int64_t)B * O;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / O;
        const int c = (int)(i - r * O);
        dst[i] = dxf[r * ldf + c] + dxb[r * ldb + c];
    }
}

// SMM: d(loss_vae)/d(obs) = d/d(encoder input) - d/d(decoder output) over the observation columns (the reconstruction target is the
// input itself, F.mse_loss(obs_z, out), smm.py:66)
__global__ __launch_bounds__(256) void smm_dobs_kernel(const float* __restrict__ dx, const float* __restrict__ dout, int64_t ld, float* __restrict__ dst,
                                                       int B, int O) {
    const int64_t n = (int64_t)B * O;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / O;
        const int c = (int)(i - r * O);
        dst[i] = dx[r * ld + c] - dout[r * ld + c];
    }
}

// Disagreement reward (disagreement.py:35-47): unbiased variance over the ensemble's predictions, mean over features
struct PredSet { const float* p[EXORL_MAX_ENSEMBLE]; };
__global__ __launch_bounds__(256) void disagreement_reward_kernel(PredSet ps, int n, float* __restrict__ reward, int rows, int D) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float acc = 0.f;
    for (int j = lane; j < D; j += 64) {
        float mean = 0.f;
        for (int m = 0; m < n; ++m) mean += ps.p[m][(int64_t)row * D + j];
        mean /= (float)n;
        float q = 0.f;
        for (int m = 0; m < n; ++m) { const float d = ps.p[m][(int64_t)row * D + j] - mean; q += d * d; }
        acc += q / (float)(n > 1 ? n - 1 : 1);
    }
    acc = wave_sum(acc);
    if (lane == 0) reward[row] = acc / (float)D;
}

// wide rows (pixel encodings): one workgroup per row, 16-byte accesses, the ensemble loop unrolled over the kernel-argument pointers — the
// wave-per-row kernel above took 2.0 ms on five (1024, 39200) predictions (800 MB: ~160 us of HBM time)
__global__ __launch_bounds__(256) void disagreement_reward_wide_kernel(PredSet ps, int n, float* __restrict__ reward, int D) {
    __shared__ float red[17];
    const int row = blockIdx.x, n4 = D >> 2;
    const float inv_n = (float)n, inv_n1 = (float)(n > 1 ? n - 1 : 1);
    float acc = 0.f;
    for (int j = threadIdx.x; j < n4; j += 256) {
        float4 v[EXORL_MAX_ENSEMBLE];
#pragma unroll
        for (int m = 0; m < EXORL_MAX_ENSEMBLE; ++m)
            if (m < n) v[m] = reinterpret_cast<const float4*>(ps.p[m] + (int64_t)row * D)[j];
        float mx = 0.f, my = 0.f, mz = 0.f, mw = 0.f;
#pragma unroll
        for (int m = 0; m < EXORL_MAX_ENSEMBLE; ++m)
            if (m < n) { mx += v[m].x; my += v[m].y; mz += v[m].z; mw += v[m].w; }
        mx /= inv_n; my /= inv_n; mz /= inv_n; mw /= inv_n;
        float qx = 0.f, qy = 0.f, qz = 0.f, qw = 0.f;
#pragma unroll
        for (int m = 0; m < EXORL_MAX_ENSEMBLE; ++m)
            if (m < n) {
                const float dx = v[m].x - mx, dy = v[m].y - my, dz = v[m].z - mz, dw = v[m].w - mw;
                qx += dx * dx; qy += dy * dy; qz += dz * dz; qw += dw * dw;
            }
        acc += (qx / inv_n1 + qy / inv_n1) + (qz / inv_n1 + qw / inv_n1);
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) reward[row] = acc / (float)D;
}

// DIAYN (diayn.py:94-127): z = argmax(skill), log-softmax of the discriminator logits; nll = -lsm[z], hit = [argmax lsm == z],
// dlogits = (softmax - onehot(z)) / B (CrossEntropyLoss, mean), reward = (lsm[z] - log(1/S)) * scale. One wave per row.
__global__ __launch_bounds__(256) void diayn_kernel(const float* __restrict__ logits, const float* __restrict__ skill, int64_t lds_, int S,
                                                    float* __restrict__ nll, float* __restrict__ hit, float* __restrict__ dlogits,
                                                    float* reward, float scale, int rows, int grows) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float mx = -INFINITY, smx = -INFINITY;
    int amx = 0x7fffffff, asx = 0x7fffffff;
    for (int j = lane; j < S; j += 64) {
        const float v = logits[(int64_t)row * S + j], k = skill[(int64_t)row * lds_ + j];
        if (v > mx) { mx = v; amx = j; }
        if (k > smx) { smx = k; asx = j; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {            // first-occurrence arg-max, as torch.argmax / torch.max
        const float ov = __shfl_xor(mx, off, 64), ok = __shfl_xor(smx, off, 64);
        const int oi = __shfl_xor(amx, off, 64), oj = __shfl_xor(asx, off, 64);
        if (ov > mx || (ov == mx && oi < amx)) { mx = ov; amx = oi; }
        if (ok > smx || (ok == smx && oj < asx)) { smx = ok; asx = oj; }
    }
    float se = 0.f;
    for (int j = lane; j < S; j += 64) se += expf(logits[(int64_t)row * S + j] - mx);
    const float lse = mx + logf(wave_sum(se));
    const float lz = logits[(int64_t)row * S + asx] - lse;
    if (lane == 0) {
        if (nll) { nll[row] = -lz; hit[row] = amx == asx ? 1.f : 0.f; }
        if (reward) reward[row] = (lz - logf(1.0f / (float)S)) * scale;
    }
    if (dlogits) {
        const float invB = 1.0f / (float)grows;
        for (int j = lane; j < S; j += 64)
            dlogits[(int64_t)row * S + j] = (expf(logits[(int64_t)row * S + j] - lse) - (j == asx ? 1.f : 0.f)) * invB;
    }
}

// ---- Proto (proto.py) -------------------------------------------------------------------------------
// F.normalize(x, dim=1): y = x / max(||x||, 1e-12), one wave per row; in place allowed; nrm optional
__global__ __launch_bounds__(256) void l2norm_fwd_kernel(const float* x, float* y, float* __restrict__ nrm, int rows, int D) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float s = 0.f;
    for (int j = lane; j < D; j += 64) { const float v = x[(int64_t)row * D + j]; s += v * v; }
    const float n = fmaxf(sqrtf(wave_sum(s)), 1e-12f);
    for (int j = lane; j < D; j += 64) y[(int64_t)row * D + j] = x[(int64_t)row * D + j] / n;
    if (nrm && lane == 0) nrm[row] = n;
}
// dx = (dy - y (y . dy)) / ||x||
__global__ __launch_bounds__(256) void l2norm_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ nrm,
                                                         float* __restrict__ dx, int rows, int D) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float s = 0.f;
    for (int j = lane; j < D; j += 64) s += y[(int64_t)row * D + j] * dy[(int64_t)row * D + j];
    s = wave_sum(s);
    const float n = nrm[row];
    for (int j = lane; j < D; j += 64) dx[(int64_t)row * D + j] = (dy[(int64_t)row * D + j] - y[(int64_t)row * D + j] * s) / n;
}
// Sinkhorn-Knopp on S = scores / tau in the (B, P) layout of the scores (the reference works on the transpose). The global
// max (Q -= Q.max(), proto.py:16) and the global sum (Q /= Q.sum(), :18) are formed from per-row values, a wave per row:
//   sk_rowmax: rowred[b] = max_p S[b,p]
//   sk_exp   : mx = max_b rowred[b] (every wave re-reduces the B values, fixed order); E = exp(S/tau - mx/tau); rowred[B+b] = sum_p E
//   sk_row(first): total = sum_b rowred[B+b] (again per wave), E /= total
__device__ __forceinline__ float sk_reduce_all(const float* __restrict__ v, int n, int lane, bool is_max) {
    float r = is_max ? -INFINITY : 0.f;
    for (int i = lane; i < n; i += 64) r = is_max ? fmaxf(r, v[i]) : r + v[i];
    return is_max ? wave_max(r) : wave_sum(r);
}
__global__ __launch_bounds__(256) void sk_rowmax_kernel(const float* __restrict__ S, int rows, int P, float* __restrict__ rowred) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float m = -INFINITY;
    for (int j = lane; j < P; j += 64) m = fmaxf(m, S[(int64_t)row * P + j]);
    m = wave_max(m);
    if (lane == 0) rowred[row] = m;
}
__global__ __launch_bounds__(256) void sk_exp_kernel(const float* __restrict__ S, float* __restrict__ E, int rows, int P, float inv_tau,
                                                     float* __restrict__ rowred) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float mx = sk_reduce_all(rowred, rows, lane, true) * inv_tau;
    float s = 0.f;
    for (int j = lane; j < P; j += 64) { const float e = expf(S[(int64_t)row * P + j] * inv_tau - mx); E[(int64_t)row * P + j] = e; s += e; }
    s = wave_sum(s);
    if (lane == 0) rowred[rows + row] = s;
}
// one Sinkhorn half-iteration pair, wave per row b: E[b,p] *= colscale_p, then the row is rescaled to sum `target`
// (1/B inside the loop, 1 for the final normalisation). first != 0: colscale_p = 1/total (the Q /= Q.sum() of proto.py:18).
__global__ __launch_bounds__(256) void sk_row_kernel(float* __restrict__ E, const float* __restrict__ colsum, const float* __restrict__ rowred,
                                                     int rows, int P, int first, float rP, float target) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float total = first ? sk_reduce_all(rowred + rows, rows, lane, false) : 1.0f;
    float s = 0.f;
    for (int j = lane; j < P; j += 64) {
        const float v = E[(int64_t)row * P + j] * (first ? 1.0f / total : rP / colsum[j]);
        E[(int64_t)row * P + j] = v;
        s += v;
    }
    if (first) return;
    s = wave_sum(s);
    for (int j = lane; j < P; j += 64) E[(int64_t)row * P + j] = E[(int64_t)row * P + j] * (target / s);
}
// loss_b = -sum_p q log_softmax(scores/tau); dscores = (softmax * sum_p q - q) / (grows tau), grows the global batch's rows. One wave per row.
__global__ __launch_bounds__(256) void proto_loss_kernel(const float* __restrict__ scores, const float* __restrict__ q, float* __restrict__ dscores,
                                                         float* __restrict__ loss_row, int rows, int P, float inv_tau, int grows) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float mx = -INFINITY, qs = 0.f;
    for (int j = lane; j < P; j += 64) { mx = fmaxf(mx, scores[(int64_t)row * P + j] * inv_tau); qs += q[(int64_t)row * P + j]; }
    mx = wave_max(mx); qs = wave_sum(qs);
    float se = 0.f;
    for (int j = lane; j < P; j += 64) se += expf(scores[(int64_t)row * P + j] * inv_tau - mx);
    const float lse = mx + logf(wave_sum(se));
    float l = 0.f;
    const float sc = inv_tau / (float)grows;
    for (int j = lane; j < P; j += 64) {
        const float lp = scores[(int64_t)row * P + j] * inv_tau - lse, qq = q[(int64_t)row * P + j];
        l -= qq * lp;
        dscores[(int64_t)row * P + j] = (expf(lp) * qs - qq) * sc;
    }
    l = wave_sum(l);
    if (lane == 0) loss_row[row] = l;
}
// Categorical(softmax over the batch of scores[:, p]).sample() by inverse CDF (proto.py:109-112); the chosen z row goes straight
// into the candidate queue (proto.py:115-117). A workgroup owns 16 prototypes: the (B, 16) slab of scores is read as 64-byte row
// segments (a column per workgroup reads B separate cache lines), exp'd into LDS, and 16 lanes run the 16 serial double-precision
// prefix walks side by side (serial in double, as the oracle / torch.multinomial's cumulative table).
template <int PC_P>
__global__ __launch_bounds__(256) void proto_candidates_kernel(const float* __restrict__ scores, const float* __restrict__ z,
                                                               const float* __restrict__ u_in, uint64_t seed, uint64_t counter,
                                                               float* __restrict__ queue, int64_t qrow0, int B, int P, int D,
                                                               int* __restrict__ cand_out, const IntrStepState* __restrict__ st) {
    if (st) { counter = st->draw_counter; qrow0 = st->qrow0; }      // captured step: this step's values live in device memory
    extern __shared__ float pr[];               // [B][PC_P + 1] unnormalised probabilities
    __shared__ float cmax[256 / PC_P][PC_P];
    __shared__ double csum[256 / PC_P][PC_P];
    __shared__ int pick[PC_P];
    const int p0 = blockIdx.x * PC_P;
    constexpr int NBL = 256 / PC_P;
    const int pl = threadIdx.x % PC_P, bl = threadIdx.x / PC_P;      // prototype lane, row lane
    const bool live = p0 + pl < P;
    float mx = -INFINITY;
    for (int b = bl; b < B; b += NBL) {
        const float v = live ? scores[(int64_t)b * P + p0 + pl] : 0.f;
        pr[b * (PC_P + 1) + pl] = v;
        mx = fmaxf(mx, v);
    }
    cmax[bl][pl] = mx;
    __syncthreads();
    mx = cmax[0][pl];
    for (int i = 1; i < NBL; ++i) mx = fmaxf(mx, cmax[i][pl]);
    for (int b = bl; b < B; b += NBL) pr[b * (PC_P + 1) + pl] = expf(pr[b * (PC_P + 1) + pl] - mx);
    __syncthreads();
    // inverse CDF in double, blocked: the NBL row lanes of a prototype each sum a contiguous chunk of rows in row order, one lane
    // chains the chunk totals in chunk order, and the walk to the first row with run > u * total restarts from the prefix of the
    // chunk that contains it. Same sequence of partial sums as one serial walk up to the association of double additions
    // (~1e-16 relative: the pick can differ only if u * total falls that close to a boundary).
    const int chunk = (B + NBL - 1) / NBL;
    {
        double c = 0.0;
        const int b0 = bl * chunk, b1 = b0 + chunk < B ? b0 + chunk : B;
        for (int b = b0; b < b1; ++b) c += (double)pr[b * (PC_P + 1) + pl];
        csum[bl][pl] = c;
    }
    __syncthreads();
    if (threadIdx.x < PC_P && live) {
        const int p = p0 + pl;
        double acc = 0.0;
        for (int i = 0; i < NBL; ++i) acc += csum[i][pl];
        float u;
        if (u_in) u = u_in[p];
        else u = philox_uniform(seed, counter, (uint32_t)p, PHILOX_PROTO_CATEGORICAL);
        const double thr = (double)u * acc;
        double run = 0.0;
        int j = 0;
        while (j < NBL - 1 && !(run + csum[j][pl] > thr)) { run += csum[j][pl]; ++j; }
        const int b1 = (j + 1) * chunk < B ? (j + 1) * chunk : B;
        int k = b1 < B - 1 ? b1 : B - 1;          // reached only if rounding keeps the chunk's own walk at or below thr
        for (int b = j * chunk; b < b1; ++b) { run += (double)pr[b * (PC_P + 1) + pl]; if (run > thr) { k = b; break; } }
        pick[pl] = k;
        if (cand_out) cand_out[p] = k;
    }
    __syncthreads();
    for (int q = 0; q < PC_P && p0 + q < P; ++q) {
        const int k = pick[q];
        for (int j = threadIdx.x; j < D; j += blockDim.x) queue[(qrow0 + p0 + q) * D + j] = z[(int64_t)k * D + j];
    }
}
// Multi-workgroup form of the draw above, for batches whose (B, PC_P + 1) slab does not fit in LDS (B > 3276). The rows fall into
// chunks of PCM_CHUNK rows and each chunk into 16 blocks of 16 rows; both sizes are constants, so every sum below is associated by B
// alone, whatever the grid, the rank or the device. Three launches, the kernel boundaries being the only hand-offs:
//   proto_cand_max : (chunk, 16-prototype group): the chunk's column maxima                                      -> cmax[chunk][p]
//   proto_cand_sum : (chunk, group): mx_p = max over the chunks (exact in any order); each block's sum of exp(S - mx_p) in double in
//                    row order, then the 16 block sums in order                                                      -> csum[chunk][p]
//   proto_cand_pick: (group): a lane per prototype walks the chunk totals in chunk order to the chunk that crosses u * total, the
//                    workgroup recomputes that chunk's 16 block sums (the same code, so the same values), the lane walks them and then
//                    the rows of the chosen block; the chosen z rows go into the queue.
// The probabilities are the LDS kernel's (expf of the same float differences); the sums' association differs from its blocking, so the
// two forms can pick differently only where u * total lies within double rounding of a CDF boundary.
constexpr int PCM_CHUNK = 256, PCM_G = 16, PCM_BLK = 16;
static_assert(PCM_CHUNK == PCM_BLK * (256 / PCM_G), "a 256-thread workgroup covers one chunk of a 16-prototype group");
__global__ __launch_bounds__(256) void proto_cand_max_kernel(const float* __restrict__ S, int B, int P, float* __restrict__ cmax) {
    __shared__ float red[256 / PCM_G][PCM_G];
    const int pl = threadIdx.x % PCM_G, bl = threadIdx.x / PCM_G, p = blockIdx.y * PCM_G + pl, c = blockIdx.x;
    float m = -INFINITY;
    if (p < P)
        for (int i = 0; i < PCM_BLK; ++i) {
            const int b = c * PCM_CHUNK + bl * PCM_BLK + i;
            if (b < B) m = fmaxf(m, S[(int64_t)b * P + p]);
        }
    red[bl][pl] = m;
    __syncthreads();
    if (threadIdx.x < PCM_G && p < P) {
        for (int i = 1; i < 256 / PCM_G; ++i) m = fmaxf(m, red[i][pl]);
        cmax[(int64_t)c * P + p] = m;
    }
}
__device__ __forceinline__ float pcm_colmax(const float* __restrict__ cmax, int nch, int P, int p) {
    float mx = cmax[p];
    for (int c = 1; c < nch; ++c) mx = fmaxf(mx, cmax[(int64_t)c * P + p]);
    return mx;
}
// sum over the rows [b0, b0 + PCM_BLK) below B of exp(S[b, p] - mx), in double, in row order
__device__ __forceinline__ double pcm_block_sum(const float* __restrict__ S, int B, int P, int p, int b0, float mx) {
    double acc = 0.0;
    for (int i = 0; i < PCM_BLK; ++i) {
        const int b = b0 + i;
        if (b < B) acc += (double)expf(S[(int64_t)b * P + p] - mx);
    }
    return acc;
}
__global__ __launch_bounds__(256) void proto_cand_sum_kernel(const float* __restrict__ S, int B, int P, int nch, const float* __restrict__ cmax,
                                                             double* __restrict__ csum) {
    __shared__ double bs[256 / PCM_G][PCM_G];
    const int pl = threadIdx.x % PCM_G, bl = threadIdx.x / PCM_G, p = blockIdx.y * PCM_G + pl, c = blockIdx.x;
    if (p < P) bs[bl][pl] = pcm_block_sum(S, B, P, p, c * PCM_CHUNK + bl * PCM_BLK, pcm_colmax(cmax, nch, P, p));
    __syncthreads();
    if (threadIdx.x < PCM_G && p < P) {
        double acc = 0.0;
        for (int i = 0; i < 256 / PCM_G; ++i) acc += bs[i][pl];
        csum[(int64_t)c * P + p] = acc;
    }
}
__global__ __launch_bounds__(256) void proto_cand_pick_kernel(const float* __restrict__ S, const float* __restrict__ z, const float* __restrict__ cmax,
                                                              const double* __restrict__ csum, int nch, const float* __restrict__ u_in, uint64_t seed,
                                                              uint64_t counter, float* __restrict__ queue, int64_t qrow0, int B, int P, int D,
                                                              const IntrStepState* __restrict__ st) {
    if (st) { counter = st->draw_counter; qrow0 = st->qrow0; }
    __shared__ double bs[256 / PCM_G][PCM_G];
    __shared__ double run_s[PCM_G], thr_s[PCM_G];
    __shared__ float mx_s[PCM_G];
    __shared__ int ch_s[PCM_G], pick[PCM_G];
    const int p0 = blockIdx.x * PCM_G, pl = threadIdx.x % PCM_G, bl = threadIdx.x / PCM_G, p = p0 + pl;
    if (threadIdx.x < PCM_G && p < P) {
        double total = 0.0;
        for (int c = 0; c < nch; ++c) total += csum[(int64_t)c * P + p];
        float u;
        if (u_in) u = u_in[p];
        else u = philox_uniform(seed, counter, (uint32_t)p, PHILOX_PROTO_CATEGORICAL);
        const double thr = (double)u * total;
        double run = 0.0;
        int j = 0;
        while (j < nch - 1 && !(run + csum[(int64_t)j * P + p] > thr)) { run += csum[(int64_t)j * P + p]; ++j; }
        run_s[pl] = run; thr_s[pl] = thr; ch_s[pl] = j; mx_s[pl] = pcm_colmax(cmax, nch, P, p);
    }
    __syncthreads();
    if (p < P) bs[bl][pl] = pcm_block_sum(S, B, P, p, ch_s[pl] * PCM_CHUNK + bl * PCM_BLK, mx_s[pl]);
    __syncthreads();
    if (threadIdx.x < PCM_G && p < P) {
        const double thr = thr_s[pl];
        const float mx = mx_s[pl];
        double run = run_s[pl];
        int j = 0;
        while (j < 256 / PCM_G - 1 && !(run + bs[j][pl] > thr)) { run += bs[j][pl]; ++j; }
        const int b0 = ch_s[pl] * PCM_CHUNK + j * PCM_BLK, b1 = b0 + PCM_BLK < B ? b0 + PCM_BLK : B;
        int k = b1 < B - 1 ? b1 : B - 1;          // reached only if rounding keeps the block's own walk at or below thr
        for (int b = b0; b < b1; ++b) { run += (double)expf(S[(int64_t)b * P + p] - mx); if (run > thr) { k = b; break; } }
        pick[pl] = k;
    }
    __syncthreads();
    for (int q = 0; q < PCM_G && p0 + q < P; ++q) {
        const int k = pick[q];
        for (int j = threadIdx.x; j < D; j += blockDim.x) queue[(qrow0 + p0 + q) * D + j] = z[(int64_t)k * D + j];
    }
}
// reward = topk-th smallest distance (proto.py:119-124) + reward bookkeeping; single block. The metrics are this rank's partial means over
// the global batch's Bg rows
__global__ __launch_bounds__(1024) void kth_reward_kernel(const float* __restrict__ topk, const float* extr, float* reward, int B, int k,
                                                          float* __restrict__ metrics, int Bg) {
    __shared__ float red[17];
    float e = 0.f;
    for (int i = threadIdx.x; i < B; i += blockDim.x) e += extr ? extr[i] : 0.f;
    e = block_sum(e, red);
    float rs = 0.f;
    for (int i = threadIdx.x; i < B; i += blockDim.x) { const float r = topk[(int64_t)i * k + (k - 1)]; reward[i] = r; rs += r; }
    rs = block_sum(rs, red);
    if (threadIdx.x == 0) { metrics[EXORL_IM_EXTR_REWARD] = e / (float)Bg; metrics[EXORL_IM_INTR_REWARD] = rs / (float)Bg; }
}

// ---- APS (aps.py:147-175) ---------------------------------------------------------------------------
// loss_b = -task . fn with fn = F.normalize(f); df = (dfn - fn (fn . dfn)) / max(||f||, 1e-12), dfn = -task / B. One wave per row.
__global__ __launch_bounds__(256) void aps_loss_kernel(const float* __restrict__ f, const float* __restrict__ task, int64_t ldt,
                                                       float* __restrict__ df, float* __restrict__ loss_row, int rows, int D, int grows) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float s = 0.f, tf = 0.f;
    for (int j = lane; j < D; j += 64) { const float v = f[(int64_t)row * D + j]; s += v * v; tf += v * task[(int64_t)row * ldt + j]; }
    const float n = fmaxf(sqrtf(wave_sum(s)), 1e-12f);
    const float tfn = wave_sum(tf) / n;                 // task . fn
    const float invB = 1.0f / (float)grows;
    for (int j = lane; j < D; j += 64) {
        const float fn = f[(int64_t)row * D + j] / n, dfn = -task[(int64_t)row * ldt + j] * invB;
        df[(int64_t)row * D + j] = (dfn - fn * (-tfn * invB)) / n;
    }
    if (lane == 0) loss_row[row] = -tfn;
}
// reward += task . rep / ||rep|| (aps.py:164-168), metrics split into the two parts; single block
__global__ __launch_bounds__(1024) void aps_sf_reward_kernel(const float* __restrict__ rep, const float* __restrict__ task, int64_t ldt,
                                                             float* reward, int B, int D, float* __restrict__ metrics, int Bg) {
    __shared__ float red[17];
    float ss = 0.f;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        float n2 = 0.f, tr = 0.f;
        for (int j = 0; j < D; ++j) { const float v = rep[(int64_t)b * D + j]; n2 += v * v; tr += v * task[(int64_t)b * ldt + j]; }
        const float sf = tr / sqrtf(n2);
        reward[b] += sf;
        ss += sf;
    }
    ss = block_sum(ss, red);
    if (threadIdx.x == 0) {
        metrics[EXORL_IM_ENT_REWARD] = metrics[EXORL_IM_INTR_REWARD];
        metrics[EXORL_IM_SF_REWARD] = ss / (float)Bg;
        metrics[EXORL_IM_INTR_REWARD] += ss / (float)Bg;
    }
}

// ---- SMM (smm.py) -----------------------------------------------------------------------------------
constexpr int SMM_VAE_HIDDEN = 150, SMM_CODE_DIM = 128;      // smm.py:38-45,98-101: fixed by the reference
// code = eps * exp(0.5 logvar) + mu (smm.py:54-58); eps kept for the backward pass. elem0: element index of this rank's first row in the
// global batch, so that each rank draws the single-process epsilon of its rows
__global__ __launch_bounds__(256) void vae_code_kernel(const float* __restrict__ mu, const float* __restrict__ lv, const float* __restrict__ eps_in,
                                                       uint64_t seed, uint64_t counter, float* __restrict__ eps, float* __restrict__ code, int64_t n,
                                                       int64_t elem0, const IntrStepState* __restrict__ st) {
    if (st) counter = st->draw_counter;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float e = eps_in ? eps_in[i] : philox_normal(seed, counter, (uint32_t)(elem0 + i), PHILOX_SMM_EPSILON);
        eps[i] = e;
        code[i] = e * expf(0.5f * lv[i]) + mu[i];
    }
}
// per row: h_s_z = sum_j (x - out)^2 (smm.py:66-70), d(mean squared error)/d out
__global__ __launch_bounds__(256) void vae_out_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ out, float* __restrict__ dout,
                                                      float* __restrict__ hsz, int rows, int W, int grows) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float sc = -2.0f / ((float)grows * (float)W);
    float s = 0.f;
    for (int j = lane; j < W; j += 64) {
        const float d = x[(int64_t)row * ldx + j] - out[(int64_t)row * W + j];
        s += d * d;
        dout[(int64_t)row * W + j] = sc * d;
    }
    s = wave_sum(s);
    if (lane == 0) hsz[row] = s;
}
// wide rows (pixel encodings, W = 39200): one workgroup per row, 16-byte accesses (the wave-per-row kernel took 309 us for 480 MB)
__global__ __launch_bounds__(256) void vae_out_wide_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ out, float* __restrict__ dout,
                                                           float* __restrict__ hsz, int rows, int W, int grows) {
    __shared__ float red[17];
    const int row = blockIdx.x, n4 = W >> 2;
    const float sc = -2.0f / ((float)grows * (float)W);
    (void)rows;
    const float4* x4 = reinterpret_cast<const float4*>(x + (int64_t)row * ldx);
    const float4* o4 = reinterpret_cast<const float4*>(out + (int64_t)row * W);
    float4* g4 = reinterpret_cast<float4*>(dout + (int64_t)row * W);
    float s = 0.f;
    for (int j = threadIdx.x; j < n4; j += 256) {
        const float4 a = x4[j], b = o4[j];
        const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z, dw = a.w - b.w;
        s += (dx * dx + dy * dy) + (dz * dz + dw * dw);
        g4[j] = make_float4(sc * dx, sc * dy, sc * dz, sc * dw);
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) hsz[row] = s;
}
// gradients at (mu, logvar) of beta * KL + reconstruction, given d/d code; kle_row = -0.5 sum (1 + lv - mu^2 - e^lv)
__global__ __launch_bounds__(256) void vae_latent_kernel(const float* __restrict__ dcode, const float* __restrict__ mu, const float* __restrict__ lv,
                                                         const float* __restrict__ eps, float* __restrict__ dmu, float* __restrict__ dlv,
                                                         float* __restrict__ kle_row, int rows, int C, float beta, int grows) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float invB = 1.0f / (float)grows;
    float k = 0.f;
    for (int j = lane; j < C; j += 64) {
        const int64_t i = (int64_t)row * C + j;
        const float m = mu[i], l = lv[i], el = expf(l), sd = expf(0.5f * l), dc = dcode[i];
        dmu[i] = dc + beta * m * invB;
        dlv[i] = dc * eps[i] * 0.5f * sd + beta * -0.5f * (1.0f - el) * invB;
        k += 1.0f + l - m * m - el;
    }
    k = wave_sum(k);
    if (lane == 0) kle_row[row] = -0.5f * k;
}
__device__ __forceinline__ float smm_log_p_star(const float* __restrict__ obs, int64_t ld, int b, float gx, float gy) {
    const float dx = obs[(int64_t)b * ld] - gx, dy = obs[(int64_t)b * ld + 1] - gy;
    const float dist = sqrtf(dx * dx + dy * dy);
    return logf(dist > 1.0f ? 1.0f / dist : 1.0f);
}
// this rank's (n, mean, M2) of log p*(s_j) for the data-parallel step: the ranks' triples are gathered and merged in rank order in double
__global__ __launch_bounds__(1024) void smm_logp_moments_kernel(const float* __restrict__ obs, int64_t ld, int B, float gx, float gy,
                                                                double* __restrict__ mom) {
    __shared__ float red[17];
    float mean, q;
    block_moments([&](int i) { return smm_log_p_star(obs, ld, i, gx, gy); }, B, red, mean, q);
    if (threadIdx.x == 0) { mom[0] = (double)B; mom[1] = (double)mean; mom[2] = (double)q; }
}
// reward and bookkeeping (smm.py:229-258); single block. mom: the `world` ranks' gathered moments of log p* (states, world > 1: slots 3
// and 7 then hold the global mean and variance on every rank, the other slots this rank's partial means over Bg), else null. The
// reference's 1-D log_p_star broadcasts its reward to (B,B): per sample that is rest_i + mean_j log_p_star_j for the TD gradient, plus
// var_j(log_p_star_j) in each critic's loss value.
__global__ __launch_bounds__(1024) void smm_reward_kernel(const float* __restrict__ obs, int64_t ld, const float* __restrict__ hsz,
                                                          const float* __restrict__ hzs, const float* extr, float* reward, int B, int Z,
                                                          float sec, float lec, float lcec, float gx, float gy, float* __restrict__ metrics, int encoded,
                                                          int Bg, const double* __restrict__ mom, int world) {
    __shared__ float red[17];
    float e = 0.f, sl = 0.f, s1 = 0.f, s2 = 0.f;
    if (encoded) {                 // pixels: p*(s) is ignored (smm.py:232-235), the reward is a plain (B, 1) column
        float rs = 0.f;
        const float hz = lec * logf((float)Z);
        for (int b = threadIdx.x; b < B; b += blockDim.x) {
            e += extr ? extr[b] : 0.f;
            s1 += sec * hsz[b];
            s2 += lcec * hzs[b];
            const float r = sec * hsz[b] + hz + lcec * hzs[b];
            reward[b] = r;
            rs += r;
        }
        e = block_sum(e, red); s1 = block_sum(s1, red); s2 = block_sum(s2, red); rs = block_sum(rs, red);
        if (threadIdx.x == 0) {
            metrics[1] = rs / (float)Bg; metrics[2] = e / (float)Bg; metrics[3] = 0.f; metrics[4] = s1 / (float)Bg; metrics[6] = s2 / (float)Bg; metrics[7] = 0.f;
        }
        return;
    }
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        e += extr ? extr[b] : 0.f;
        const float dx = obs[(int64_t)b * ld] - gx, dy = obs[(int64_t)b * ld + 1] - gy;
        const float dist = sqrtf(dx * dx + dy * dy);
        sl += logf(dist > 1.0f ? 1.0f / dist : 1.0f);
        s1 += sec * hsz[b];
        s2 += lcec * hzs[b];
    }
    e = block_sum(e, red);
    float lm = block_sum(sl, red) / (float)B, gvar = 0.f;
    if (mom) {                     // every thread merges the same few triples
        double n = mom[0], mean = mom[1], m2 = mom[2];
        for (int r = 1; r < world; ++r) {
            const double nr = mom[3 * r], d = mom[3 * r + 1] - mean, tot = n + nr;
            mean += d * nr / tot;
            m2 += mom[3 * r + 2] + d * d * n * nr / tot;
            n = tot;
        }
        lm = (float)mean; gvar = (float)(m2 / n);
    }
    s1 = block_sum(s1, red); s2 = block_sum(s2, red);
    float var = 0.f, rs = 0.f;
    const float hz = lec * logf((float)Z);
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const float dx = obs[(int64_t)b * ld] - gx, dy = obs[(int64_t)b * ld + 1] - gy;
        const float dist = sqrtf(dx * dx + dy * dy);
        const float l = logf(dist > 1.0f ? 1.0f / dist : 1.0f) - lm;
        var += l * l;
        const float r = lm + sec * hsz[b] + hz + lcec * hzs[b];
        reward[b] = r;
        rs += r;
    }
    var = block_sum(var, red); rs = block_sum(rs, red);
    if (threadIdx.x == 0) {          // one rank: Bg == B
        metrics[1] = rs / (float)Bg; metrics[2] = e / (float)Bg; metrics[3] = lm; metrics[4] = s1 / (float)Bg; metrics[6] = s2 / (float)Bg;
        metrics[7] = mom ? gvar : var / (float)B;
    }
}

static int grid_for(int64_t n) { const int64_t b = (n + 255) / 256; return (int)(b > 2048 ? 2048 : (b < 1 ? 1 : b)); }

// n nets of identical shape on the same input (an ensemble): each layer's GEMMs of all nets share one grouped launch
int mlp_forward_many(const Mlp* nets, int n, const float* P, const float* x, int64_t ldx, int rows, int prec, hipStream_t s) {
    EXORL_REQUIRE(n >= 1 && n <= 16, "mlp_forward_many: %d nets", n);
    const int nl = (int)nets[0].L.size();
    for (int l = 0; l < nl; ++l) {
        GemmProblem p[16];
        for (int m = 0; m < n; ++m) {
            const Lin& L = nets[m].L[l];
            p[m] = GemmProblem{l ? nets[m].act[l - 1] : x, P + L.W, nets[m].act[l], P + L.b, rows, L.out, L.in, l ? (int64_t)L.in : ldx, L.in, L.out};
        }
        EXORL_TRY(gemm_grouped(prec, 0, 0, p, n, l < nl - 1 || nets[0].relu_last, false, s));
    }
    return 0;
}
// backward of the same ensemble: masks + bias gradients per net, weight gradients and hidden dgrads grouped; dx (rows, in0) or null
int mlp_backward_many(const Mlp* nets, int n, const float* P, float* G, const float* x, int64_t ldx, int rows, int prec, hipStream_t s, float* dx) {
    EXORL_REQUIRE(n >= 1 && n <= 16, "mlp_backward_many: %d nets", n);
    const int nl = (int)nets[0].L.size();
    for (int l = nl - 1; l >= 0; --l) {
        GemmProblem w[16], g[16];
        for (int m = 0; m < n; ++m) {
            const Lin& L = nets[m].L[l];
            float* d = nets[m].dact[l];
            bool summed = false;
            if (l < nl - 1 || nets[m].relu_last) {
                summed = relu_bwd_colsum(d, nets[m].act[l], G + L.b, rows, L.out, s) == 0;      // mask and bias gradient in one pass over dZ
                if (!summed) {
                    const int64_t cnt = (int64_t)rows * L.out;
                    hipLaunchKernelGGL(relu_bwd_kernel, dim3(grid_for(cnt)), dim3(256), 0, s, d, nets[m].act[l], cnt);
                    EXORL_LAUNCH_CHECK();
                }
            }
            if (!summed) EXORL_TRY(colsum(d, G + L.b, rows, L.out, 1, 0, 0, s));
            w[m] = GemmProblem{d, l ? nets[m].act[l - 1] : x, G + L.W, nullptr, L.out, L.in, rows, L.out, l ? (int64_t)L.in : ldx, L.in};      // dW[o][i] = sum_r d[r][o] in[r][i]
            if (l) g[m] = GemmProblem{d, P + L.W, nets[m].dact[l - 1], nullptr, rows, L.in, L.out, L.out, L.in, L.in};      // din[r][i] = sum_o d[r][o] W[o][i]
        }
        EXORL_TRY(gemm_grouped(prec, 1, 1, w, n, false, false, s));
        if (l) EXORL_TRY(gemm_grouped(prec, 0, 1, g, n, false, false, s));
        else if (dx)                               // d/d(input) summed over the nets in net order (one accumulating launch per net)
            for (int m = 0; m < n; ++m) {
                const Lin& L = nets[m].L[0];
                GemmProblem gx{nets[m].dact[0], P + L.W, dx, nullptr, rows, L.in, L.out, L.out, L.in, L.in};
                EXORL_TRY(gemm_grouped(prec, 0, 1, &gx, 1, false, m > 0, s));
            }
    }
    return 0;
}

// the single net is the ensemble of one: the same launches with the same arguments (dact[last] holds d(loss)/d(output))
int mlp_forward(const Mlp& m, const float* P, const float* x, int64_t ldx, int rows, int prec, hipStream_t s) {
    return mlp_forward_many(&m, 1, P, x, ldx, rows, prec, s);
}
int mlp_backward(const Mlp& m, const float* P, float* G, const float* x, int64_t ldx, int rows, float* dx, int prec, hipStream_t s) {
    return mlp_backward_many(&m, 1, P, G, x, ldx, rows, prec, s, dx);
}

}  // namespace exorl

using namespace exorl;

struct exorl_intr {
    exorl_intr_cfg cfg;
    std::vector<TensorDesc> tensors;          // module.parameters() order
    int64_t total = 0, trainable = 0;      // flat sizes (floats): all parameters / the prefix the optimiser steps
    float* ws = nullptr;
    bool owns_ws = false;
    float* flat[4] = {nullptr, nullptr, nullptr, nullptr};
    Mlp net[EXORL_MAX_ENSEMBLE];           // RND: predictor, target; ICM(-APT): forward_net, backward_net; Disagreement: the ensemble; DIAYN: [0]
    int n_nets = 0;
    Lin trunk{};                           // APT: Linear(O, R) of the trunk; LayerNorm gain/beta offsets below
    int64_t ln_g = 0, ln_b = 0;
    float *xn = nullptr, *xf = nullptr, *xb = nullptr, *dxf = nullptr, *dxb = nullptr;
    float *x2 = nullptr, *z = nullptr, *rep = nullptr, *xhat = nullptr, *rstd = nullptr, *drep = nullptr, *dz = nullptr, *topk = nullptr, *d2 = nullptr, *skr = nullptr, *splitk = nullptr;    // d2: squared-distance scratch of the kNN (B x n_tgt)
    float *fe = nullptr, *be = nullptr, *metrics = nullptr, *bn = nullptr;
    RmsState* rms = nullptr;
    // Proto: predictor (Linear) in front of net[0] = projector; prototypes C; frozen predictor_target; candidate queue
    Lin pred{}, pred_t{};
    int64_t protos = 0;
    float *z1 = nullptr, *dz1 = nullptr, *sn = nullptr, *nrm = nullptr, *tn = nullptr, *scores_s = nullptr, *scores_t = nullptr,
          *dscores = nullptr, *dsn = nullptr, *colsum_p = nullptr, *scal = nullptr, *queue = nullptr;
    float* pcm_max = nullptr;              // candidate draw over more rows than the LDS form holds: chunk maxima (float), chunk sums (double)
    double* pcm_sum = nullptr;
    int64_t queue_ptr = 0;
    uint64_t cat_counter = 0;
    // SMM: net[0] = z_pred_net, net[1] = vae.enc (ReLU after both layers), net[2] = vae.dec; the two heads; sub-range of the vae
    Lin enc_mu{}, enc_lv{};
    int64_t vae_off = 0;
    float *mu = nullptr, *lv = nullptr, *eps = nullptr, *code = nullptr, *dcode = nullptr, *dmu = nullptr, *dlv = nullptr, *hsz = nullptr, *hzs = nullptr;
    int64_t t = 0;                         // optimiser steps taken
    // joint graph with the agent (exorl_agent_enable_graph_intr): t, cat_counter and queue_ptr above stay the truth; `dev` is their
    // device copy, library-allocated on first capture, which the captured step advances itself (intr_step_begin_kernel)
    IntrStepState* dev = nullptr;
    bool dev_stale = true;                 // an eager step or a setter moved the host values since the last push
    bool capturing = false;                // the stages enqueue the forms that read `dev`
    const IntrStepState* st() const { return capturing ? dev : nullptr; }
    // data parallel (cfg.world_size > 1): this rank's batch rows are rows [rank * batch, (rank + 1) * batch) of the global batch
    int world = 1, rank = 0;
    float* gat = nullptr;                  // ICM-APT / APS / Proto: the gathered representation rows (world slots of batch x rep_dim, rank order)
    double* mom = nullptr;                 // RND / ICM-APT / APS: the gathered RMS moments, (n, mean, M2) per rank; SMM on states: those of log p*
    double* bnmom = nullptr;               // RND on states: the gathered BatchNorm1d moments, (n, mean, M2) per feature per rank
    bool bn_dp() const { return cfg.kind == EXORL_INTR_RND && world > 1 && !(cfg.flags & EXORL_INTR_ENCODED); }
    int Bg() const { return cfg.batch * world; }
};

namespace exorl {

static bool proto_cand_lds_fits(int64_t rows) { return (size_t)rows * 5 * sizeof(float) <= 64 * 1024; }     // proto_candidates_kernel<4>

static int n_models_of(const exorl_intr_cfg& c) { return c.n_models > 0 ? c.n_models : 5; }     // disagreement.py:12 default

static void describe_intr(exorl_intr* it) {
    const auto& c = it->cfg;
    const int O = c.obs_dim, A = c.act_dim, H = c.hidden_dim, R = c.rep_dim;
    int64_t off = 0;
    auto add = [&](int64_t rows, int64_t cols) { const int64_t o = off; it->tensors.push_back({o, rows, cols}); off += round_up(rows * cols, 4); return o; };
    auto lin = [&](int in, int out) { Lin l{in, out, 0, 0}; l.W = add(out, in); l.b = add(out, 1); return l; };
    it->tensors.clear();
    for (auto& n : it->net) n.L.clear();
    it->n_nets = 2;
    if (c.kind == EXORL_INTR_RND) {
        for (int n = 0; n < 2; ++n) {
            it->net[n].L = {lin(O, H), lin(H, H), lin(H, R)};
            if (n == 0) it->trainable = round_up(off, 64);
            off = round_up(off, 64);
        }
    } else if (c.kind == EXORL_INTR_DISAGREEMENT) {
        it->n_nets = n_models_of(c);
        for (int n = 0; n < it->n_nets; ++n) it->net[n].L = {lin(O + A, H), lin(H, O)};
        it->trainable = round_up(off, 64);
    } else if (c.kind == EXORL_INTR_DIAYN || c.kind == EXORL_INTR_APS) {
        it->n_nets = 1;
        it->net[0].L = {lin(O, H), lin(H, H), lin(H, R)};             // R = skill_dim
        it->trainable = round_up(off, 64);
    } else if (c.kind == EXORL_INTR_SMM) {                            // R = z_dim
        const int W = O + R, V = SMM_VAE_HIDDEN, C = SMM_CODE_DIM;
        it->n_nets = 3;
        it->net[0].L = {lin(O, H), lin(H, H), lin(H, R)};
        off = round_up(off, 64);
        it->vae_off = off;
        it->net[1].L = {lin(W, V), lin(V, V)};
        it->net[1].relu_last = true;
        it->enc_mu = lin(V, C);
        it->enc_lv = lin(V, C);
        it->net[2].L = {lin(C, V), lin(V, V), lin(V, W)};
        it->trainable = round_up(off, 64);
    } else if (c.kind == EXORL_INTR_PROTO) {                          // R = pred_dim, H = proj_dim
        it->n_nets = 1;
        it->pred = lin(O, R);
        it->net[0].L = {lin(R, H), lin(H, R)};
        it->protos = add(c.num_protos, R);
        it->trainable = round_up(off, 64);
        off = it->trainable;
        it->pred_t = lin(O, R);                                       // predictor_target: same padded layout as predictor
    } else {
        int in_f = O + A, in_b = 2 * O, out_f = O;
        if (c.kind == EXORL_INTR_ICM_APT) {
            it->trunk = lin(O, R);
            it->ln_g = add(R, 1); it->ln_b = add(R, 1);
            in_f = R + A; in_b = 2 * R; out_f = R;
        }
        it->net[0].L = {lin(in_f, H), lin(H, out_f)};
        it->net[1].L = {lin(in_b, H), lin(H, A)};
        it->trainable = round_up(off, 64);
    }
    it->total = round_up(off, 64);
}

static bool intr_exchanges(const exorl_intr_cfg& c, int xchg);      // asks the plan (below)

static void carve_intr(exorl_intr* it, SimpleCarver& c) {
    const auto& g = it->cfg;
    const int64_t B = g.batch, O = g.obs_dim, R = g.rep_dim, W = g.world_size > 1 ? g.world_size : 1;
    it->flat[EXORL_T_PARAM] = c.take(it->total);
    for (int w = 1; w < 4; ++w) it->flat[w] = c.take(it->trainable);
    for (int n = 0; n < it->n_nets; ++n) {
        Mlp& m = it->net[n];
        m.act.clear(); m.dact.clear();
        for (const Lin& l : m.L) {
            m.act.push_back(c.take(B * l.out));
            m.dact.push_back((g.kind == EXORL_INTR_RND && n == 1) ? nullptr : c.take(B * l.out));
        }
    }
    it->fe = c.take(B * (g.kind == EXORL_INTR_DISAGREEMENT ? it->n_nets : 1)); it->be = c.take(B);
    it->metrics = c.take(EXORL_N_INTR_METRICS);
    it->rms = reinterpret_cast<RmsState*>(c.take(4));
    // ICM-APT / APS: the slot is in the layout whether or not knn_rms is on, so for them the kind decides and not the plan
    if (intr_exchanges(g, EXORL_INTR_XCHG_MOMENTS) || (W > 1 && (g.kind == EXORL_INTR_ICM_APT || g.kind == EXORL_INTR_APS)))
        it->mom = reinterpret_cast<double*>(c.take(2 * 3 * W));
    if (g.kind == EXORL_INTR_RND) {
        if (!(g.flags & EXORL_INTR_ENCODED)) {     // encoded rows arrive normalised (BatchNorm2d ran on the frames)
            it->xn = c.take(B * O);
            it->bn = c.take(2 * O + 1);
            if (intr_exchanges(g, EXORL_INTR_XCHG_BN)) it->bnmom = reinterpret_cast<double*>(c.take(2 * 3 * O * W));
        }
    } else if (g.kind == EXORL_INTR_APS) {
        it->topk = c.take(B * g.knn_k);
        it->d2 = c.take(knn_scratch_floats((int)B, (int)(B * W)));
        if (intr_exchanges(g, EXORL_INTR_XCHG_REP)) it->gat = c.take(W * B * R);
    } else if (g.kind == EXORL_INTR_SMM) {
        const int64_t C = SMM_CODE_DIM;
        it->mu = c.take(B * C); it->lv = c.take(B * C); it->eps = c.take(B * C); it->code = c.take(B * C); it->dcode = c.take(B * C);
        it->dmu = c.take(B * C); it->dlv = c.take(B * C); it->hsz = c.take(B); it->hzs = c.take(B);
        it->dxf = c.take(B * (O + R));                           // d/d(obs_z) of the VAE encoder (dobs_out)
    } else if (g.kind == EXORL_INTR_PROTO) {
        const int64_t P = g.num_protos, Bg = B * W;                // Sinkhorn and the candidate draw run over the global batch's rows
        it->z1 = c.take(B * R); it->dz1 = c.take(B * R); it->sn = c.take(B * R); it->nrm = c.take(B); it->tn = c.take(B * R);
        it->scores_s = c.take(Bg * P); it->scores_t = c.take(Bg * P); it->dscores = c.take(B * P); it->dsn = c.take(B * R);
        it->colsum_p = c.take(P); it->scal = c.take(4); it->skr = c.take(2 * Bg);
        if (intr_exchanges(g, EXORL_INTR_XCHG_REP)) it->gat = c.take(W * B * R);
        if (!proto_cand_lds_fits(Bg)) {
            it->pcm_max = c.take(cdiv(Bg, PCM_CHUNK) * P);
            it->pcm_sum = reinterpret_cast<double*>(c.take(2 * cdiv(Bg, PCM_CHUNK) * P));
        }
        if (O >= 4096) it->splitk = c.take(16 * B * R);              // pixel features: split-K scratch of the predictor
        it->queue = c.take((int64_t)g.queue_size * R);
        it->topk = c.take(B * g.knn_k);
        it->d2 = c.take(B * round_up(g.queue_size, 64));
    } else if (g.kind == EXORL_INTR_DISAGREEMENT) {
        it->xf = c.take(B * it->net[0].L[0].in);
        it->dxf = c.take(B * it->net[0].L[0].in);
    } else if (g.kind != EXORL_INTR_DIAYN) {
        const int64_t in_f = it->net[0].L[0].in, in_b = it->net[1].L[0].in;
        it->xf = c.take(B * in_f); it->xb = c.take(B * in_b);
        it->dxf = c.take(B * in_f); it->dxb = c.take(B * in_b);
        if (g.kind == EXORL_INTR_ICM_APT) {
            it->x2 = c.take(2 * B * O); it->z = c.take(2 * B * R); it->rep = c.take(2 * B * R); it->xhat = c.take(2 * B * R);
            it->rstd = c.take(2 * B); it->drep = c.take(2 * B * R); it->dz = c.take(2 * B * R);
            it->topk = c.take(B * g.knn_k);
            it->d2 = c.take(knn_scratch_floats((int)B, (int)(B * W)));
            if (intr_exchanges(g, EXORL_INTR_XCHG_REP)) it->gat = c.take(W * B * R);
        }
    }
}

static int intr_reset_state(exorl_intr* it) {
    const RmsState r0{0.f, 1.f, 1e-4};                    // utils.RMS.__init__ (utils.py:259-262)
    EXORL_CHECK_HIP(hipMemcpy(it->rms, &r0, sizeof(r0), hipMemcpyHostToDevice));
    if (it->bn) {                                         // BatchNorm1d buffers: running_mean 0, running_var 1, num_batches_tracked 0
        std::vector<float> b(2 * it->cfg.obs_dim + 1, 0.f);
        for (int i = 0; i < it->cfg.obs_dim; ++i) b[it->cfg.obs_dim + i] = 1.f;
        EXORL_CHECK_HIP(hipMemcpy(it->bn, b.data(), b.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    return 0;
}

static int launch_mean(const float* x, int n, float scale, float* out, int accumulate, hipStream_t s) {
    hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(1024), 0, s, x, n, scale, out, accumulate);
    EXORL_LAUNCH_CHECK();
    return 0;
}

static int intr_adam(exorl_intr* it, hipStream_t s) {
    it->t += 1;
    if (it->capturing)
        return adam_step_dev(it->flat[EXORL_T_PARAM], it->flat[EXORL_T_GRAD], it->flat[EXORL_T_ADAM_M], it->flat[EXORL_T_ADAM_V], it->trainable,
                             &it->dev->c[0], nullptr, nullptr, s);
    return adam_step(it->flat[EXORL_T_PARAM], it->flat[EXORL_T_GRAD], it->flat[EXORL_T_ADAM_M], it->flat[EXORL_T_ADAM_V], it->trainable,
                     it->cfg.lr, 0.9f, 0.999f, 1e-8f, it->t, nullptr, 0.f, s);
}

int launch_concat(const float* a, int64_t lda, int ca, const float* b, int64_t ldb, int cb, float* dst, int rows, hipStream_t s) {
    hipLaunchKernelGGL(concat2_kernel, dim3(grid_for((int64_t)rows * (ca + cb))), dim3(256), 0, s, a, lda, ca, b, ldb, cb, dst, rows);
    EXORL_LAUNCH_CHECK();
    return 0;
}

// ---- staged module steps ------------------------------------------------------------------------------
// A module's step is a flat list of steps, its plan. A step is a fixed piece of work (xxx_step runs exactly one); where the data-parallel
// step needs an exchange across the ranks after it, the plan names the exchange (EXORL_INTR_XCHG_*). Which steps there are and what
// follows them depends on the configuration and on `train` alone, so intr_plan knows it before the first launch, and carve_intr asks the
// same plan which exchange buffers a configuration needs. A phase (exorl_intr_update_phase) runs steps until one is followed by an
// exchange; the one-rank step (exorl_intr_update, the joint graph) runs the phases back to back. The gradient exchange is named at one
// rank too, where a sum over one rank is the identity; no other exchange is named there.
// train: 0 reward only, 1 step + reward on the same rows, 2 step only (RND on encodings and Proto: the pixel reward pass draws a new
// augmentation and runs the encoder the step has just moved, rnd.py:98-103, so the caller encodes again in between).
// "-> X": exchange X follows; [..]: the step exists only then; dp: world_size > 1.
//   RND                         [dp, states] BN_MOMENTS -> BN | [train] LOSS -> GRAD | [train] ADAM | then unless train == 2:
//                               FORWARD (the errors the reward reads) | [dp] MOMENTS -> MOMENTS | REWARD
//   ICM, Disagreement, DIAYN    [train] LOSS -> GRAD | [train] ADAM | REWARD (forward pass and reward)
//   ICM-APT, APS                [train] LOSS -> GRAD | [train] ADAM | FORWARD (the representation rows) | [dp] ROWS (into this rank's slot)
//                               -> REP | KNN (own rows at one rank, the gathered rows otherwise) | [dp, knn_rms] MOMENTS -> MOMENTS | REWARD
//   SMM (train is required)     LOSS (vae + pred) -> GRAD | ADAM (both ranges) | [dp, states] MOMENTS (of log p*) -> MOMENTS | REWARD
//   Proto                       see proto_step
enum { ST_BN_MOMENTS, ST_LOSS, ST_ADAM, ST_FORWARD, ST_ROWS, ST_KNN, ST_MOMENTS, ST_REWARD };

struct IntrPlan {
    int n = 0;
    int step[8], xchg[8];          // xchg: the exchange that follows the step, or -1
    void add(bool on, int st, int x = -1) { if (on) { step[n] = st; xchg[n++] = x; } }
};

static IntrPlan intr_plan(const exorl_intr_cfg& c, int train) {
    const bool dp = c.world_size > 1, states = !(c.flags & EXORL_INTR_ENCODED), reward = train != 2;
    const int rep = dp ? EXORL_INTR_XCHG_REP : -1;
    IntrPlan p;
    switch (c.kind) {
        case EXORL_INTR_RND:
            p.add(dp && states, ST_BN_MOMENTS, EXORL_INTR_XCHG_BN);
            p.add(train, ST_LOSS, EXORL_INTR_XCHG_GRAD);
            p.add(train, ST_ADAM);
            p.add(reward, ST_FORWARD);
            p.add(reward && dp, ST_MOMENTS, EXORL_INTR_XCHG_MOMENTS);
            p.add(reward, ST_REWARD);
            break;
        case EXORL_INTR_ICM_APT: case EXORL_INTR_APS:
            p.add(train, ST_LOSS, EXORL_INTR_XCHG_GRAD);
            p.add(train, ST_ADAM);
            p.add(true, ST_FORWARD);
            p.add(dp, ST_ROWS, EXORL_INTR_XCHG_REP);
            p.add(true, ST_KNN);
            p.add(dp && c.knn_rms, ST_MOMENTS, EXORL_INTR_XCHG_MOMENTS);
            p.add(true, ST_REWARD);
            break;
        case EXORL_INTR_SMM:               // train is required: smm_step refuses without
            p.add(true, ST_LOSS, EXORL_INTR_XCHG_GRAD);
            p.add(true, ST_ADAM);
            p.add(dp && states, ST_MOMENTS, EXORL_INTR_XCHG_MOMENTS);
            p.add(true, ST_REWARD);
            break;
        case EXORL_INTR_PROTO:
            p.add(train, ST_FORWARD, rep);
            p.add(train, ST_LOSS, EXORL_INTR_XCHG_GRAD);
            p.add(train, ST_ADAM);
            p.add(reward, ST_ROWS, rep);
            p.add(reward, ST_REWARD);
            break;
        default:                           // ICM, Disagreement, DIAYN
            p.add(train, ST_LOSS, EXORL_INTR_XCHG_GRAD);
            p.add(train, ST_ADAM);
            p.add(true, ST_REWARD);
    }
    return p;
}

static bool intr_exchanges(const exorl_intr_cfg& c, int xchg) {      // does this configuration's full step (train = 1) name the exchange?
    const IntrPlan p = intr_plan(c, 1);
    for (int i = 0; i < p.n; ++i)
        if (p.xchg[i] == xchg) return true;
    return false;
}

// ---- RND -------------------------------------------------------------------------------------------
static int rnd_forward(exorl_intr* it, const exorl_intr_batch& b, bool with_target, float* dpred, hipStream_t s) {
    const auto& c = it->cfg;
    const int B = c.batch, O = c.obs_dim, R = c.rep_dim;
    const float* P = it->flat[EXORL_T_PARAM];
    if (c.flags & EXORL_INTR_ENCODED) {
        // pixels (rnd.py:26-27,35-39,47-53): BatchNorm2d + clamp ran on the frames, in front of the two encoders; obs is the agent's encoder
        // on them (the predictor's first stage), next_obs the frozen encoder copy's output (the target's first stage)
        EXORL_REQUIRE(b.next_obs, "intr_update: RND on encodings reads the frozen encoder's output from next_obs");
        EXORL_TRY(mlp_forward(it->net[0], P, b.obs, b.obs_ld, B, c.precision, s));
        EXORL_TRY(mlp_forward(it->net[1], P, b.next_obs, b.next_obs_ld, B, c.precision, s));
    } else {
        if (it->bn_dp()) hipLaunchKernelGGL(bn_merged_clamp_kernel, dim3(O), dim3(256), 0, s, b.obs, b.obs_ld, it->xn, B, O, c.clip_val, it->bn,
                                            (const double*)it->bnmom, it->world);
        else hipLaunchKernelGGL(bn_clamp_kernel, dim3(O), dim3(256), 0, s, b.obs, b.obs_ld, it->xn, B, O, c.clip_val, it->bn);
        EXORL_LAUNCH_CHECK();
        if (with_target) EXORL_TRY(mlp_forward_many(it->net, 2, P, it->xn, O, B, c.precision, s));      // predictor and frozen target: same input, same shapes
        else EXORL_TRY(mlp_forward(it->net[0], P, it->xn, O, B, c.precision, s));
    }
    hipLaunchKernelGGL(rnd_err_kernel, dim3(cdiv(B, 4)), dim3(256), 0, s, it->net[0].act[2], it->net[1].act[2], it->fe, dpred, B, R, it->Bg());
    EXORL_LAUNCH_CHECK();
    return 0;
}

// On state rows with world_size > 1 each rank's BatchNorm1d moments are gathered before anything reads the normalised rows. The reward pass
// normalises the same rows in training mode again (rnd.py:98-100): the merged moments are still in place, so rnd_forward steps the running
// statistics a second time without an exchange.
static int rnd_step(exorl_intr* it, const exorl_intr_batch& b, int train, int step, hipStream_t s) {
    const auto& c = it->cfg;
    const int B = c.batch;
    const bool enc = (c.flags & EXORL_INTR_ENCODED) != 0;
    EXORL_REQUIRE(enc || train != 2, "intr_update: RND's step-only call belongs to the encoded (pixel) variant");
    if (step == ST_BN_MOMENTS) {
        hipLaunchKernelGGL(bn_moments_kernel, dim3(c.obs_dim), dim3(256), 0, s, b.obs, b.obs_ld, B, c.obs_dim, it->bnmom + (int64_t)3 * c.obs_dim * it->rank);
        EXORL_LAUNCH_CHECK();
        return 0;
    }
    if (step == ST_LOSS) {                                                                           // rnd.py:79-96
        EXORL_TRY(rnd_forward(it, b, true, it->net[0].dact[2], s));
        EXORL_TRY(launch_mean(it->fe, B, 1.0f / (float)it->Bg(), it->metrics + EXORL_IM_LOSS, 0, s));
        return mlp_backward(it->net[0], it->flat[EXORL_T_PARAM], it->flat[EXORL_T_GRAD], enc ? b.obs : it->xn, enc ? b.obs_ld : (int64_t)c.obs_dim, B,
                            enc ? b.dobs_out : nullptr, c.precision, s);
    }
    if (step == ST_ADAM) return intr_adam(it, s);
    // compute_intr_reward (rnd.py:98-103); states: same batch -> same BatchNorm output and frozen target, only the predictor moved
    if (step == ST_FORWARD) return rnd_forward(it, b, !train, nullptr, s);
    if (step == ST_MOMENTS) {                       // the batch moments of the error
        hipLaunchKernelGGL(rms_moments_kernel, dim3(1), dim3(1024), 0, s, it->fe, B, 1, 0, it->mom + 3 * it->rank);
        EXORL_LAUNCH_CHECK();
        return 0;
    }
    hipLaunchKernelGGL(rnd_reward_kernel, dim3(1), dim3(1024), 0, s, it->fe, b.extr_reward, b.reward_out, B, it->Bg(), c.scale, it->rms,
                       it->world > 1 ? (const double*)it->mom : nullptr, it->world, it->metrics);
    EXORL_LAUNCH_CHECK();
    return 0;
}

// ---- ICM / ICM-APT ---------------------------------------------------------------------------------
static int icm_errors(exorl_intr* it, const float* tgt, int64_t ldt, const float* action, int64_t lda, bool grads, bool inverse, hipStream_t s) {
    const auto& c = it->cfg;
    const int D = it->net[0].L[1].out;
    EXORL_REQUIRE(!inverse || lda == c.act_dim, "intr: ICM needs a dense action matrix (ld == action_dim)");
    launch_icm_err(it->net[0].act[1], D, tgt, ldt, inverse ? it->net[1].act[1] : nullptr, action, c.act_dim, it->fe, it->be,
                   grads ? it->net[0].dact[1] : nullptr, grads ? it->net[1].dact[1] : nullptr, c.batch, 1.0f / (float)it->Bg(), s);
    EXORL_LAUNCH_CHECK();
    return 0;
}

static int icm_step(exorl_intr* it, const exorl_intr_batch& b, int train, int step, hipStream_t s) {
    const auto& c = it->cfg;
    const int B = c.batch, O = c.obs_dim, A = c.act_dim, prec = c.precision;
    const float invBg = 1.0f / (float)it->Bg();
    const float* P = it->flat[EXORL_T_PARAM];
    float* G = it->flat[EXORL_T_GRAD];
    if (step == ST_LOSS) {                                                                           // icm.py:64-84
        EXORL_TRY(launch_concat(b.obs, b.obs_ld, O, b.action, b.action_ld, A, it->xf, B, s));
        EXORL_TRY(launch_concat(b.obs, b.obs_ld, O, b.next_obs, b.next_obs_ld, O, it->xb, B, s));
        EXORL_TRY(mlp_forward(it->net[0], P, it->xf, O + A, B, prec, s));
        EXORL_TRY(mlp_forward(it->net[1], P, it->xb, 2 * O, B, prec, s));
        EXORL_TRY(icm_errors(it, b.next_obs, b.next_obs_ld, b.action, b.action_ld, true, true, s));
        EXORL_TRY(launch_mean(it->fe, B, invBg, it->metrics + EXORL_IM_LOSS, 0, s));
        EXORL_TRY(launch_mean(it->be, B, invBg, it->metrics + EXORL_IM_LOSS, 1, s));
        EXORL_TRY(mlp_backward(it->net[0], P, G, it->xf, O + A, B, b.dobs_out ? it->dxf : nullptr, prec, s));
        EXORL_TRY(mlp_backward(it->net[1], P, G, it->xb, 2 * O, B, b.dobs_out ? it->dxb : nullptr, prec, s));
        if (b.dobs_out) {                          // obs is an encoding: the caller's encoder continues the backward pass (icm.py:64-78)
            hipLaunchKernelGGL(icm_dobs_kernel, dim3(grid_for((int64_t)B * O)), dim3(256), 0, s, it->dxf, (int64_t)(O + A), it->dxb, (int64_t)(2 * O), b.dobs_out, B, O);
            EXORL_LAUNCH_CHECK();
        }
        return 0;
    }
    if (step == ST_ADAM) return intr_adam(it, s);
    if (!train) EXORL_TRY(launch_concat(b.obs, b.obs_ld, O, b.action, b.action_ld, A, it->xf, B, s));      // after LOSS xf is in place
    EXORL_TRY(mlp_forward(it->net[0], P, it->xf, O + A, B, prec, s));                                // icm.py:86-92
    EXORL_TRY(icm_errors(it, b.next_obs, b.next_obs_ld, b.action, b.action_ld, false, false, s));
    hipLaunchKernelGGL(icm_reward_kernel, dim3(1), dim3(1024), 0, s, it->fe, b.extr_reward, b.reward_out, B, c.scale, it->metrics, it->Bg());
    EXORL_LAUNCH_CHECK();
    return 0;
}

static int apt_trunk(exorl_intr* it, const float* x, int64_t ldx, int rows, hipStream_t s) {    // Linear -> LayerNorm -> Tanh (icm_apt.py:21-22)
    const auto& c = it->cfg;
    const float* P = it->flat[EXORL_T_PARAM];
    GemmProblem p{x, P + it->trunk.W, it->z, P + it->trunk.b, rows, c.rep_dim, c.obs_dim, ldx, c.obs_dim, c.rep_dim};
    EXORL_TRY(gemm_grouped(c.precision, 0, 0, &p, 1, false, false, s));
    return ln_tanh_fwd(it->z, P + it->ln_g, P + it->ln_b, it->rep, it->xhat, it->rstd, rows, c.rep_dim, 1, 0, 0, s);
}

// utils.PBE on the representation rows `rep` (batch x rep_dim) of ICM-APT / APS: the steps after FORWARD, which made rep
static int pbe_step(exorl_intr* it, const exorl_intr_batch& b, const float* rep, int step, hipStream_t s) {
    const auto& c = it->cfg;
    const int B = c.batch, R = c.rep_dim;
    if (step == ST_ROWS) {                              // gather the rows: the neighbours are sought in the global batch
        EXORL_CHECK_HIP(hipMemcpyAsync(it->gat + (int64_t)it->rank * B * R, rep, sizeof(float) * B * R, hipMemcpyDeviceToDevice, s));
        return 0;
    }
    if (step == ST_KNN) return knn_topk(rep, B, it->world > 1 ? it->gat : rep, it->Bg(), R, c.knn_k, it->topk, it->d2, s);
    if (step == ST_MOMENTS) {
        hipLaunchKernelGGL(rms_moments_kernel, dim3(1), dim3(1024), 0, s, it->topk, B, c.knn_k, c.knn_avg, it->mom + 3 * it->rank);
        EXORL_LAUNCH_CHECK();
        return 0;
    }
    hipLaunchKernelGGL(pbe_reward_kernel, dim3(1), dim3(1024), 0, s, it->topk, b.extr_reward, b.reward_out, B, it->Bg(), c.knn_k, c.knn_avg, c.knn_rms,
                       c.knn_clip, it->rms, it->world > 1 ? (const double*)it->mom : nullptr, it->world, it->metrics);
    EXORL_LAUNCH_CHECK();
    return 0;
}

static int apt_step(exorl_intr* it, const exorl_intr_batch& b, int train, int step, hipStream_t s) {
    const auto& c = it->cfg;
    const int B = c.batch, O = c.obs_dim, A = c.act_dim, R = c.rep_dim, prec = c.precision;
    const float invBg = 1.0f / (float)it->Bg();
    const float* P = it->flat[EXORL_T_PARAM];
    float* G = it->flat[EXORL_T_GRAD];
    if (step == ST_LOSS) {                                                                           // icm_apt.py:33-50,86-104
        EXORL_TRY(launch_concat(b.obs, b.obs_ld, O, nullptr, 0, 0, it->x2, B, s));                   // x2 = [obs; next_obs] stacked by rows
        EXORL_TRY(launch_concat(b.next_obs, b.next_obs_ld, O, nullptr, 0, 0, it->x2 + (int64_t)B * O, B, s));
        EXORL_TRY(apt_trunk(it, it->x2, O, 2 * B, s));
        const float* rn = it->rep + (int64_t)B * R;
        EXORL_TRY(launch_concat(it->rep, R, R, b.action, b.action_ld, A, it->xf, B, s));
        EXORL_TRY(launch_concat(it->rep, R, R, rn, R, R, it->xb, B, s));
        EXORL_TRY(mlp_forward(it->net[0], P, it->xf, R + A, B, prec, s));
        EXORL_TRY(mlp_forward(it->net[1], P, it->xb, 2 * R, B, prec, s));
        EXORL_TRY(icm_errors(it, rn, R, b.action, b.action_ld, true, true, s));
        EXORL_TRY(launch_mean(it->fe, B, invBg, it->metrics + EXORL_IM_LOSS, 0, s));
        EXORL_TRY(launch_mean(it->be, B, invBg, it->metrics + EXORL_IM_LOSS, 1, s));
        EXORL_TRY(mlp_backward(it->net[0], P, G, it->xf, R + A, B, it->dxf, prec, s));
        EXORL_TRY(mlp_backward(it->net[1], P, G, it->xb, 2 * R, B, it->dxb, prec, s));
        hipLaunchKernelGGL(apt_drep_kernel, dim3(grid_for((int64_t)B * R)), dim3(256), 0, s, it->dxf, (int64_t)(R + A), it->dxb,
                           (int64_t)(2 * R), it->net[0].dact[1], it->drep, B, R);
        EXORL_LAUNCH_CHECK();
        EXORL_TRY(ln_param_grad(it->drep, it->rep, it->xhat, G + it->ln_g, G + it->ln_b, 2 * B, R, 1, 0, 0, s));
        EXORL_TRY(ln_tanh_bwd(it->drep, it->rep, it->xhat, it->rstd, P + it->ln_g, it->dz, 2 * B, R, 1, 0, 0, s));
        EXORL_TRY(colsum(it->dz, G + it->trunk.b, 2 * B, R, 1, 0, 0, s));
        GemmProblem w{it->dz, it->x2, G + it->trunk.W, nullptr, R, O, 2 * B, R, O, O};
        EXORL_TRY(gemm_grouped(prec, 1, 1, &w, 1, false, false, s));
        if (b.dobs_out) {                          // d(loss)/d(obs rows) = dz[:B] W_trunk (next_obs was encoded without a graph, icm_apt.py:116-118)
            GemmProblem gx{it->dz, P + it->trunk.W, b.dobs_out, nullptr, B, O, R, R, O, O};
            EXORL_TRY(gemm_grouped(prec, 0, 1, &gx, 1, false, false, s));
        }
        return 0;
    }
    if (step == ST_ADAM) return intr_adam(it, s);
    if (step == ST_FORWARD) return apt_trunk(it, b.obs, b.obs_ld, B, s);                             // icm_apt.py:106-110
    return pbe_step(it, b, it->rep, step, s);
}

// ---- Disagreement ----------------------------------------------------------------------------------
static int disagreement_step(exorl_intr* it, const exorl_intr_batch& b, int train, int step, hipStream_t s) {
    const auto& c = it->cfg;
    const int B = c.batch, O = c.obs_dim, A = c.act_dim, prec = c.precision, n = it->n_nets;
    const float invBg = 1.0f / (float)it->Bg();
    const float* P = it->flat[EXORL_T_PARAM];
    float* G = it->flat[EXORL_T_GRAD];
    if (step == ST_LOSS) {                                                                           // disagreement.py:19-33,64-80
        EXORL_TRY(launch_concat(b.obs, b.obs_ld, O, b.action, b.action_ld, A, it->xf, B, s));
        EXORL_TRY(mlp_forward_many(it->net, n, P, it->xf, O + A, B, prec, s));          // the 5 models' layers share launches
        for (int m = 0; m < n; ++m) {
            launch_icm_err(it->net[m].act[1], O, b.next_obs, b.next_obs_ld, nullptr, nullptr, A, it->fe + (int64_t)m * B, nullptr, it->net[m].dact[1],
                           nullptr, B, 1.0f / ((float)it->Bg() * (float)n), s);
            EXORL_LAUNCH_CHECK();
        }
        EXORL_TRY(mlp_backward_many(it->net, n, P, G, it->xf, O + A, B, prec, s, b.dobs_out ? it->dxf : nullptr));
        if (b.dobs_out) EXORL_TRY(launch_concat(it->dxf, O + A, O, nullptr, 0, 0, b.dobs_out, B, s));
        return launch_mean(it->fe, B * n, 1.0f / ((float)it->Bg() * (float)n), it->metrics + EXORL_IM_LOSS, 0, s);
    }
    if (step == ST_ADAM) return intr_adam(it, s);
    if (!train) EXORL_TRY(launch_concat(b.obs, b.obs_ld, O, b.action, b.action_ld, A, it->xf, B, s));      // after LOSS xf is in place
    PredSet ps{};
    EXORL_TRY(mlp_forward_many(it->net, n, P, it->xf, O + A, B, prec, s));                           // disagreement.py:35-47
    for (int m = 0; m < n; ++m) ps.p[m] = it->net[m].act[1];
    if (b.extr_reward) EXORL_TRY(launch_mean(b.extr_reward, B, invBg, it->metrics + EXORL_IM_EXTR_REWARD, 0, s));
    bool wide = O >= 2048 && O % 4 == 0;
    for (int m = 0; m < n; ++m) wide = wide && reinterpret_cast<uintptr_t>(ps.p[m]) % 16 == 0;
    if (wide) hipLaunchKernelGGL(disagreement_reward_wide_kernel, dim3(B), dim3(256), 0, s, ps, n, b.reward_out, O);
    else hipLaunchKernelGGL(disagreement_reward_kernel, dim3(cdiv(B, 4)), dim3(256), 0, s, ps, n, b.reward_out, B, O);
    EXORL_LAUNCH_CHECK();
    return launch_mean(b.reward_out, B, invBg, it->metrics + EXORL_IM_INTR_REWARD, 0, s);
}

// ---- DIAYN -----------------------------------------------------------------------------------------
static int diayn_step(exorl_intr* it, const exorl_intr_batch& b, int step, hipStream_t s) {
    const auto& c = it->cfg;
    const int B = c.batch, S = c.rep_dim, prec = c.precision, Bg = it->Bg();
    const float invBg = 1.0f / (float)Bg;
    const float* P = it->flat[EXORL_T_PARAM];
    if (step == ST_LOSS) {                                                                           // diayn.py:78-92,107-127
        EXORL_TRY(mlp_forward(it->net[0], P, b.next_obs, b.next_obs_ld, B, prec, s));
        hipLaunchKernelGGL(diayn_kernel, dim3(cdiv(B, 4)), dim3(256), 0, s, it->net[0].act[2], b.skill, b.skill_ld, S, it->fe, it->be,
                           it->net[0].dact[2], (float*)nullptr, c.scale, B, Bg);
        EXORL_LAUNCH_CHECK();
        EXORL_TRY(launch_mean(it->fe, B, invBg, it->metrics + EXORL_IM_LOSS, 0, s));
        EXORL_TRY(launch_mean(it->be, B, invBg, it->metrics + EXORL_IM_ACC, 0, s));
        return mlp_backward(it->net[0], P, it->flat[EXORL_T_GRAD], b.next_obs, b.next_obs_ld, B, b.dobs_out, prec, s);      // dobs_out: d/d(next_obs)
    }
    if (step == ST_ADAM) return intr_adam(it, s);
    EXORL_TRY(mlp_forward(it->net[0], P, b.next_obs, b.next_obs_ld, B, prec, s));                    // diayn.py:94-105
    if (b.extr_reward) EXORL_TRY(launch_mean(b.extr_reward, B, invBg, it->metrics + EXORL_IM_EXTR_REWARD, 0, s));
    hipLaunchKernelGGL(diayn_kernel, dim3(cdiv(B, 4)), dim3(256), 0, s, it->net[0].act[2], b.skill, b.skill_ld, S, (float*)nullptr,
                       (float*)nullptr, (float*)nullptr, b.reward_out, c.scale, B, Bg);
    EXORL_LAUNCH_CHECK();
    return launch_mean(b.reward_out, B, invBg, it->metrics + EXORL_IM_INTR_REWARD, 0, s);
}

// ---- SMM --------------------------------------------------------------------------------------------
static int adam_range(exorl_intr* it, int64_t off, int64_t n, float lr, int opt, hipStream_t s) {      // opt: IntrStepState::lr's slot of `lr`
    if (it->capturing)
        return adam_step_dev(it->flat[EXORL_T_PARAM] + off, it->flat[EXORL_T_GRAD] + off, it->flat[EXORL_T_ADAM_M] + off, it->flat[EXORL_T_ADAM_V] + off, n,
                             &it->dev->c[opt], nullptr, nullptr, s);
    return adam_step(it->flat[EXORL_T_PARAM] + off, it->flat[EXORL_T_GRAD] + off, it->flat[EXORL_T_ADAM_M] + off, it->flat[EXORL_T_ADAM_V] + off, n,
                     lr, 0.9f, 0.999f, 1e-8f, it->t, nullptr, 0.f, s);
}

// Both optimisers' gradients (vae_opt's and pred_opt's ranges) are ready after LOSS: one exchange, then the two Adam steps. update_pred
// neither reads the VAE's parameters nor writes its range, so running its passes before vae_opt.step() changes nothing.
static int smm_step(exorl_intr* it, const exorl_intr_batch& b, int train, int step, hipStream_t s) {
    const auto& c = it->cfg;
    const int B = c.batch, O = c.obs_dim, Z = c.rep_dim, W = O + Z, V = SMM_VAE_HIDDEN, C = SMM_CODE_DIM, prec = c.precision, Bg = it->Bg();
    EXORL_REQUIRE(b.obs_ld >= W, "intr_update: SMM reads [obs | z] rows (obs_ld >= obs_dim + z_dim)");
    EXORL_REQUIRE(train, "intr_update: SMM's reward is defined by the losses of its own update step (smm.py:226-241); train must be set");
    const float* P = it->flat[EXORL_T_PARAM];
    float* G = it->flat[EXORL_T_GRAD];
    Mlp &zp = it->net[0], &enc = it->net[1], &dec = it->net[2];
    if (step == ST_ADAM) {
        EXORL_TRY(adam_range(it, it->vae_off, it->trainable - it->vae_off, c.vae_lr, 2, s));
        return adam_range(it, 0, it->vae_off, c.sp_lr, 1, s);
    }
    if (step == ST_MOMENTS) {                      // mean_j and var_j of log p*(s_j) are over the global batch
        hipLaunchKernelGGL(smm_logp_moments_kernel, dim3(1), dim3(1024), 0, s, b.obs, b.obs_ld, B, c.goal_x, c.goal_y, it->mom + 3 * it->rank);
        EXORL_LAUNCH_CHECK();
        return 0;
    }
    if (step == ST_REWARD) {                       // smm.py:229-246
        const bool merged = it->world > 1 && !(c.flags & EXORL_INTR_ENCODED);
        hipLaunchKernelGGL(smm_reward_kernel, dim3(1), dim3(1024), 0, s, b.obs, b.obs_ld, it->hsz, it->hzs, b.extr_reward, b.reward_out, B, Z,
                           c.state_ent_coef, c.latent_ent_coef, c.latent_cond_ent_coef, c.goal_x, c.goal_y, it->metrics, (c.flags & EXORL_INTR_ENCODED) ? 1 : 0, Bg,
                           merged ? (const double*)it->mom : nullptr, it->world);
        EXORL_LAUNCH_CHECK();
        return 0;
    }
    it->t += 1;                                    // LOSS: both updates' passes; the ADAM step reads the t of this step
    // ---- update_vae (smm.py:173-185, VAE.loss :61-70) on obs_z
    EXORL_TRY(mlp_forward(enc, P, b.obs, b.obs_ld, B, prec, s));
    GemmProblem hd[2] = {{enc.act[1], P + it->enc_mu.W, it->mu, P + it->enc_mu.b, B, C, V, V, V, C},
                         {enc.act[1], P + it->enc_lv.W, it->lv, P + it->enc_lv.b, B, C, V, V, V, C}};
    EXORL_TRY(gemm_grouped(prec, 0, 0, hd, 2, false, false, s));
    hipLaunchKernelGGL(vae_code_kernel, dim3(grid_for((int64_t)B * C)), dim3(256), 0, s, it->mu, it->lv, b.cat_uniform, 0x736d6dull, it->cat_counter++,
                       it->eps, it->code, (int64_t)B * C, (int64_t)it->rank * B * C, it->st());
    EXORL_LAUNCH_CHECK();
    EXORL_TRY(mlp_forward(dec, P, it->code, C, B, prec, s));
    if (W >= 2048 && W % 4 == 0 && b.obs_ld % 4 == 0 && reinterpret_cast<uintptr_t>(b.obs) % 16 == 0 && reinterpret_cast<uintptr_t>(dec.act[2]) % 16 == 0 &&
        reinterpret_cast<uintptr_t>(dec.dact[2]) % 16 == 0)
        hipLaunchKernelGGL(vae_out_wide_kernel, dim3(B), dim3(256), 0, s, b.obs, b.obs_ld, dec.act[2], dec.dact[2], it->hsz, B, W, Bg);
    else hipLaunchKernelGGL(vae_out_kernel, dim3(cdiv(B, 4)), dim3(256), 0, s, b.obs, b.obs_ld, dec.act[2], dec.dact[2], it->hsz, B, W, Bg);
    EXORL_LAUNCH_CHECK();
    EXORL_TRY(mlp_backward(dec, P, G, it->code, C, B, it->dcode, prec, s));
    hipLaunchKernelGGL(vae_latent_kernel, dim3(cdiv(B, 4)), dim3(256), 0, s, it->dcode, it->mu, it->lv, it->eps, it->dmu, it->dlv, it->fe, B, C, c.vae_beta, Bg);
    EXORL_LAUNCH_CHECK();
    EXORL_TRY(launch_mean(it->fe, B, c.vae_beta / (float)Bg, it->metrics + EXORL_IM_LOSS, 0, s));            // beta * kle
    EXORL_TRY(launch_mean(it->hsz, B, 1.0f / ((float)Bg * (float)W), it->metrics + EXORL_IM_LOSS, 1, s));    // + mse.mean()
    EXORL_TRY(colsum(it->dmu, G + it->enc_mu.b, B, C, 1, 0, 0, s));
    EXORL_TRY(colsum(it->dlv, G + it->enc_lv.b, B, C, 1, 0, 0, s));
    GemmProblem wg[2] = {{it->dmu, enc.act[1], G + it->enc_mu.W, nullptr, C, V, B, C, V, V}, {it->dlv, enc.act[1], G + it->enc_lv.W, nullptr, C, V, B, C, V, V}};
    EXORL_TRY(gemm_grouped(prec, 1, 1, wg, 2, false, false, s));
    GemmProblem d1{it->dmu, P + it->enc_mu.W, enc.dact[1], nullptr, B, V, C, C, V, V}, d2{it->dlv, P + it->enc_lv.W, enc.dact[1], nullptr, B, V, C, C, V, V};
    EXORL_TRY(gemm_grouped(prec, 0, 1, &d1, 1, false, false, s));
    EXORL_TRY(gemm_grouped(prec, 0, 1, &d2, 1, false, true, s));
    EXORL_TRY(mlp_backward(enc, P, G, b.obs, b.obs_ld, B, b.dobs_out ? it->dxf : nullptr, prec, s));
    if (b.dobs_out) {
        hipLaunchKernelGGL(smm_dobs_kernel, dim3(grid_for((int64_t)B * O)), dim3(256), 0, s, it->dxf, dec.dact[2], (int64_t)W, b.dobs_out, B, O);
        EXORL_LAUNCH_CHECK();
    }
    // ---- update_pred (smm.py:187-200): skill discriminator on the raw observation columns
    EXORL_TRY(mlp_forward(zp, P, b.obs, b.obs_ld, B, prec, s));
    hipLaunchKernelGGL(diayn_kernel, dim3(cdiv(B, 4)), dim3(256), 0, s, zp.act[2], b.skill, b.skill_ld, Z, it->hzs, it->be, zp.dact[2], (float*)nullptr, 1.0f, B, Bg);
    EXORL_LAUNCH_CHECK();
    EXORL_TRY(launch_mean(it->hzs, B, 1.0f / (float)Bg, it->metrics + 5, 0, s));
    return mlp_backward(zp, P, G, b.obs, b.obs_ld, B, nullptr, prec, s);
}

// ---- APS -------------------------------------------------------------------------------------------
static int aps_step(exorl_intr* it, const exorl_intr_batch& b, int step, hipStream_t s) {
    const auto& c = it->cfg;
    const int B = c.batch, D = c.rep_dim, prec = c.precision, Bg = it->Bg();
    const float* P = it->flat[EXORL_T_PARAM];
    const float* rep = it->net[0].act[2];
    if (step == ST_LOSS) {                                                                           // aps.py:147-159,170-175
        EXORL_TRY(mlp_forward(it->net[0], P, b.next_obs, b.next_obs_ld, B, prec, s));
        hipLaunchKernelGGL(aps_loss_kernel, dim3(cdiv(B, 4)), dim3(256), 0, s, it->net[0].act[2], b.skill, b.skill_ld, it->net[0].dact[2], it->fe, B, D, Bg);
        EXORL_LAUNCH_CHECK();
        EXORL_TRY(launch_mean(it->fe, B, 1.0f / (float)Bg, it->metrics + EXORL_IM_LOSS, 0, s));
        return mlp_backward(it->net[0], P, it->flat[EXORL_T_GRAD], b.next_obs, b.next_obs_ld, B, b.dobs_out, prec, s);      // dobs_out: d/d(next_obs)
    }
    if (step == ST_ADAM) return intr_adam(it, s);
    if (step == ST_FORWARD) return mlp_forward(it->net[0], P, b.next_obs, b.next_obs_ld, B, prec, s);      // aps.py:161-168
    EXORL_TRY(pbe_step(it, b, rep, step, s));
    if (step != ST_REWARD) return 0;
    hipLaunchKernelGGL(aps_sf_reward_kernel, dim3(1), dim3(1024), 0, s, rep, b.skill, b.skill_ld, b.reward_out, B, D, it->metrics, Bg);
    EXORL_LAUNCH_CHECK();
    return 0;
}

// ---- Proto ------------------------------------------------------------------------------------------
static int launch_l2norm(const float* x, float* y, float* nrm, int rows, int D, hipStream_t s) {
    hipLaunchKernelGGL(l2norm_fwd_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, s, x, y, nrm, rows, D);
    EXORL_LAUNCH_CHECK();
    return 0;
}

// predictor Linear(obs_dim, pred_dim): on pixel features (obs_dim = 39200) a (B, 128) output is 32 tiles of a 39200-long reduction,
// so it runs as a 16-way split-K there
static int proto_predict(exorl_intr* it, const float* x, int64_t ldx, const float* W, const float* bias, float* out, hipStream_t s) {
    const auto& c = it->cfg;
    if (it->splitk) return linear_splitk(c.precision, x, ldx, W, bias, out, c.batch, c.rep_dim, c.obs_dim, it->splitk, 16, s);
    GemmProblem p{x, W, out, bias, c.batch, c.rep_dim, c.obs_dim, ldx, c.obs_dim, c.rep_dim};
    return gemm_grouped(c.precision, 0, 0, &p, 1, false, false, s);
}

// Categorical(softmax over the rows of scores[:, p]).sample() for every prototype (proto.py:109-112), the chosen rows of z written into
// the queue at queue_ptr (proto.py:115-117). Every rank draws from the same gathered rows with the same seed and counter, so every
// rank writes the same queue rows.
static int proto_candidates(exorl_intr* it, const float* scores, const float* z, const float* u, int rows, hipStream_t s) {
    const int P = it->cfg.num_protos, D = it->cfg.rep_dim;
    const uint64_t seed = 0x70726f746full, ctr = it->cat_counter++;
    if (proto_cand_lds_fits(rows)) {
#define EXORL_PCAND(PP) hipLaunchKernelGGL(proto_candidates_kernel<PP>, dim3(cdiv(P, PP)), dim3(256), (size_t)rows * (PP + 1) * sizeof(float), s, scores, \
                                            z, u, seed, ctr, it->queue, it->queue_ptr, rows, P, D, (int*)nullptr, it->st())
        if ((size_t)rows * 17 * sizeof(float) <= 64 * 1024) EXORL_PCAND(16);
        else if ((size_t)rows * 9 * sizeof(float) <= 64 * 1024) EXORL_PCAND(8);
        else EXORL_PCAND(4);
#undef EXORL_PCAND
    } else {
        EXORL_REQUIRE(it->pcm_max && it->pcm_sum, "intr: Proto candidate sampling over %d rows without its scratch", rows);
        const int nch = cdiv(rows, PCM_CHUNK);
        hipLaunchKernelGGL(proto_cand_max_kernel, dim3(nch, cdiv(P, PCM_G)), dim3(256), 0, s, scores, rows, P, it->pcm_max);
        hipLaunchKernelGGL(proto_cand_sum_kernel, dim3(nch, cdiv(P, PCM_G)), dim3(256), 0, s, scores, rows, P, nch, it->pcm_max, it->pcm_sum);
        hipLaunchKernelGGL(proto_cand_pick_kernel, dim3(cdiv(P, PCM_G)), dim3(256), 0, s, scores, z, it->pcm_max, it->pcm_sum, nch, u, seed, ctr,
                           it->queue, it->queue_ptr, rows, P, D, it->st());
    }
    EXORL_LAUNCH_CHECK();
    it->queue_ptr = (it->queue_ptr + P) % it->cfg.queue_size;
    return 0;
}

// Proto's steps (proto.py:103-157); train 2 plans FORWARD to ADAM, train 1 all five, train 0 ROWS and REWARD:
//   FORWARD  normalize_protos; the online branch on this rank's rows (scores_s); the target branch's normalised rows, written into this
//            rank's slot of the gather buffer                                                                -> REP (world > 1)
//   LOSS     the targets' scores and Sinkhorn-Knopp over all Bg gathered rows (every rank the same, in the same order); loss and dscores of
//            this rank's rows against its rows of the assignment, as means over Bg; backward into the gradients and dobs_out -> GRAD
//   ADAM     Adam; predictor_target's Polyak step
//   ROWS     the reward pass: normalize_protos; z = l2norm(predictor(next_obs)) of this rank's rows into its slot -> REP (world > 1)
//   REWARD   scores of all Bg rows; the candidate draw over them (same seed and counter on every rank: the same queue rows, queue_ptr and
//            counter); kNN of this rank's rows against the queue; the k-th-distance reward; the metrics as partial means over Bg
static int proto_step(exorl_intr* it, const exorl_intr_batch& b, int step, hipStream_t s) {
    const auto& c = it->cfg;
    const int B = c.batch, O = c.obs_dim, D = c.rep_dim, P = c.num_protos, prec = c.precision, Bg = it->Bg();
    float* Pm = it->flat[EXORL_T_PARAM];
    float* G = it->flat[EXORL_T_GRAD];
    float* C = Pm + it->protos;
    const float inv_tau = 1.0f / c.tau;
    float* mine = it->world > 1 ? it->gat + (int64_t)it->rank * B * D : nullptr;      // this rank's slot of the gathered rows
    if (step == ST_FORWARD) {                                                                        // proto.py:126-157
        EXORL_TRY(launch_l2norm(C, C, nullptr, P, D, s));                                            // normalize_protos
        EXORL_TRY(proto_predict(it, b.obs, b.obs_ld, Pm + it->pred.W, Pm + it->pred.b, it->z1, s));
        EXORL_TRY(mlp_forward(it->net[0], Pm, it->z1, D, B, prec, s));
        EXORL_TRY(launch_l2norm(it->net[0].act[1], it->sn, it->nrm, B, D, s));
        GemmProblem ps{it->sn, C, it->scores_s, nullptr, B, P, D, D, D, P};
        EXORL_TRY(gemm_grouped(prec, 0, 0, &ps, 1, false, false, s));
        // target branch (no gradient): predictor_target on next_obs, Sinkhorn assignment
        const float* nt = b.next_obs_target ? b.next_obs_target : b.next_obs;
        const int64_t nt_ld = b.next_obs_target ? b.next_obs_target_ld : b.next_obs_ld;
        EXORL_TRY(proto_predict(it, nt, nt_ld, Pm + it->pred_t.W, Pm + it->pred_t.b, it->tn, s));
        return launch_l2norm(it->tn, mine ? mine : it->tn, nullptr, B, D, s);
    }
    if (step == ST_LOSS) {
        const float* t = it->world > 1 ? it->gat : it->tn;
        GemmProblem pq{t, C, it->scores_t, nullptr, Bg, P, D, D, D, P};
        EXORL_TRY(gemm_grouped(prec, 0, 0, &pq, 1, false, false, s));
        hipLaunchKernelGGL(sk_rowmax_kernel, dim3(cdiv(Bg, 4)), dim3(256), 0, s, it->scores_t, Bg, P, it->skr);
        hipLaunchKernelGGL(sk_exp_kernel, dim3(cdiv(Bg, 4)), dim3(256), 0, s, it->scores_t, it->scores_t, Bg, P, inv_tau, it->skr);
        hipLaunchKernelGGL(sk_row_kernel, dim3(cdiv(Bg, 4)), dim3(256), 0, s, it->scores_t, it->colsum_p, it->skr, Bg, P, 1, 0.f, 0.f);
        EXORL_LAUNCH_CHECK();
        for (int iter = 0; iter < 3; ++iter) {     // u = r / Q.sum(1); Q *= u; Q *= c / Q.sum(0)   (+ the final Q / Q.sum(0) folded into the last pass)
            EXORL_TRY(colsum(it->scores_t, it->colsum_p, Bg, P, 1, 0, 0, s));
            hipLaunchKernelGGL(sk_row_kernel, dim3(cdiv(Bg, 4)), dim3(256), 0, s, it->scores_t, it->colsum_p, it->skr, Bg, P, 0, 1.0f / (float)P,
                               iter == 2 ? 1.0f : 1.0f / (float)Bg);
            EXORL_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(proto_loss_kernel, dim3(cdiv(B, 4)), dim3(256), 0, s, it->scores_s, it->scores_t + (int64_t)it->rank * B * P, it->dscores,
                           it->fe, B, P, inv_tau, Bg);
        EXORL_LAUNCH_CHECK();
        EXORL_TRY(launch_mean(it->fe, B, 1.0f / (float)Bg, it->metrics + EXORL_IM_LOSS, 0, s));
        GemmProblem gc{it->dscores, it->sn, G + it->protos, nullptr, P, D, B, P, D, D};              // dC = dscores^T sn
        EXORL_TRY(gemm_grouped(prec, 1, 1, &gc, 1, false, false, s));
        GemmProblem gs{it->dscores, C, it->dsn, nullptr, B, D, P, P, D, D};                          // dsn = dscores C
        EXORL_TRY(gemm_grouped(prec, 0, 1, &gs, 1, false, false, s));
        hipLaunchKernelGGL(l2norm_bwd_kernel, dim3(cdiv(B, 4)), dim3(256), 0, s, it->dsn, it->sn, it->nrm, it->net[0].dact[1], B, D);
        EXORL_LAUNCH_CHECK();
        EXORL_TRY(mlp_backward(it->net[0], Pm, G, it->z1, D, B, it->dz1, prec, s));
        EXORL_TRY(colsum(it->dz1, G + it->pred.b, B, D, 1, 0, 0, s));
        GemmProblem gw{it->dz1, b.obs, G + it->pred.W, nullptr, D, O, B, D, b.obs_ld, O};
        EXORL_TRY(gemm_grouped(prec, 1, 1, &gw, 1, false, false, s));
        if (b.dobs_out) {                      // d(loss)/d(obs) = dz1 Wp, before Wp moves: the caller's encoder continues the backward pass
            GemmProblem gx{it->dz1, Pm + it->pred.W, b.dobs_out, nullptr, B, O, D, D, O, O};
            EXORL_TRY(gemm_grouped(prec, 0, 1, &gx, 1, false, false, s));
        }
        return 0;
    }
    if (step == ST_ADAM) {
        EXORL_TRY(intr_adam(it, s));
        // utils.soft_update_params(predictor, predictor_target, encoder_target_tau) (proto.py:202-203): nothing reads the target before the next update
        return soft_update(Pm + it->pred.W, Pm + it->pred_t.W, it->pred_t.b + round_up(c.rep_dim, 4) - it->pred_t.W, c.target_tau, s);
    }
    if (step == ST_ROWS) {                                                                           // compute_intr_reward(next_obs) (proto.py:103-124)
        EXORL_TRY(launch_l2norm(C, C, nullptr, P, D, s));
        EXORL_TRY(proto_predict(it, b.next_obs, b.next_obs_ld, Pm + it->pred.W, Pm + it->pred.b, it->sn, s));
        return launch_l2norm(it->sn, mine ? mine : it->sn, nullptr, B, D, s);
    }
    const float* z = it->world > 1 ? it->gat : it->sn;
    GemmProblem pc{z, C, it->scores_s, nullptr, Bg, P, D, D, D, P};
    EXORL_TRY(gemm_grouped(prec, 0, 0, &pc, 1, false, false, s));
    EXORL_TRY(proto_candidates(it, it->scores_s, z, b.cat_uniform, Bg, s));
    EXORL_TRY(knn_topk(mine ? mine : it->sn, B, it->queue, c.queue_size, D, c.knn_k, it->topk, it->d2, s));
    hipLaunchKernelGGL(kth_reward_kernel, dim3(1), dim3(1024), 0, s, it->topk, b.extr_reward, b.reward_out, B, c.knn_k, it->metrics, Bg);
    EXORL_LAUNCH_CHECK();
    return 0;
}

// one phase of the step: the steps of the phases before it are skipped, then steps run until one is followed by an exchange
static int intr_phase(exorl_intr* it, const exorl_intr_batch& b, int train, int phase, int* next, hipStream_t s) {
    const IntrPlan p = intr_plan(it->cfg, train);
    int i = 0;
    for (int ph = 0; ph < phase && i < p.n; ++ph) {
        while (i < p.n - 1 && p.xchg[i] < 0) ++i;
        ++i;
    }
    EXORL_REQUIRE(phase >= 0 && i < p.n, "intr_update_phase: phase %d out of range", phase);
    for (*next = -1; i < p.n && *next < 0; ++i) {
        switch (it->cfg.kind) {
            case EXORL_INTR_RND: EXORL_TRY(rnd_step(it, b, train, p.step[i], s)); break;
            case EXORL_INTR_ICM: EXORL_TRY(icm_step(it, b, train, p.step[i], s)); break;
            case EXORL_INTR_ICM_APT: EXORL_TRY(apt_step(it, b, train, p.step[i], s)); break;
            case EXORL_INTR_DISAGREEMENT: EXORL_TRY(disagreement_step(it, b, train, p.step[i], s)); break;
            case EXORL_INTR_APS: EXORL_TRY(aps_step(it, b, p.step[i], s)); break;
            case EXORL_INTR_SMM: EXORL_TRY(smm_step(it, b, train, p.step[i], s)); break;
            case EXORL_INTR_PROTO: EXORL_TRY(proto_step(it, b, p.step[i], s)); break;
            default: EXORL_TRY(diayn_step(it, b, p.step[i], s));
        }
        *next = p.xchg[i];
    }
    return 0;
}

// ---- the module's side of the joint graph ---------------------------------------------------------------
__global__ void intr_step_begin_kernel(IntrStepState* st) {
    if (threadIdx.x == 0 && blockIdx.x == 0) intr_step_begin_device(st);
}
// stream-ordered upload of the host's counters (kernel argument: no host buffer whose lifetime would matter)
__global__ void intr_state_set_kernel(IntrStepState* st, IntrStepState v) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *st = v;
}
__global__ __launch_bounds__(256) void copy_meta_columns_kernel(const float* __restrict__ obs, float* __restrict__ next_obs, int64_t ld, int rows,
                                                                int O, int M) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (int64_t)rows * M; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / M, j = O + i % M;
        next_obs[r * ld + j] = obs[r * ld + j];
    }
}
int copy_meta_columns(const float* obs, float* next_obs, int64_t ld, int rows, int O, int M, hipStream_t s) {
    EXORL_REQUIRE(obs && next_obs && rows > 0 && O > 0 && M > 0 && ld >= O + M, "copy_meta_columns: bad arguments");
    hipLaunchKernelGGL(copy_meta_columns_kernel, dim3(grid_for((int64_t)rows * M)), dim3(256), 0, s, obs, next_obs, ld, rows, O, M);
    EXORL_LAUNCH_CHECK();
    return 0;
}

// the device step state that the host's counters imply: beta^t by pow(), as adam_step computes it for an eager step
static IntrStepState intr_host_state(const exorl_intr* it) {
    const auto& c = it->cfg;
    IntrStepState v{};
    v.counter = v.draw_counter = it->cat_counter;
    v.t = it->t;
    v.queue_ptr = v.qrow0 = it->queue_ptr;
    const bool proto = c.kind == EXORL_INTR_PROTO;
    v.queue_size = proto ? c.queue_size : 0;
    v.num_protos = proto ? c.num_protos : 0;
    v.draws = (proto || c.kind == EXORL_INTR_SMM) ? 1 : 0;
    v.b1 = dec7(0.9f); v.b2 = dec7(0.999f); v.eps = dec7(1e-8f);
    v.b1t = pow(v.b1, (double)it->t); v.b2t = pow(v.b2, (double)it->t);
    v.lr[0] = dec7(c.lr); v.lr[1] = dec7(c.sp_lr); v.lr[2] = dec7(c.vae_lr);
    return v;
}

static int intr_push_state(exorl_intr* it, hipStream_t s) {
    hipLaunchKernelGGL(intr_state_set_kernel, dim3(1), dim3(64), 0, s, it->dev, intr_host_state(it));
    EXORL_LAUNCH_CHECK();
    it->dev_stale = false;
    return 0;
}

static int check_intr_batch(exorl_intr* it, const exorl_intr_batch* b);
static int intr_run_stages(exorl_intr* it, const exorl_intr_batch& b, int train, hipStream_t s);

// the step's launches in their captured form; the host's counters are put back afterwards (nothing ran)
static int intr_capture_body(exorl_intr* it, const exorl_intr_batch* b, hipStream_t s) {
    const int64_t t = it->t, qp = it->queue_ptr;
    const uint64_t ctr = it->cat_counter;
    it->capturing = true;
    hipLaunchKernelGGL(intr_step_begin_kernel, dim3(1), dim3(64), 0, s, it->dev);
    int rc = hipGetLastError() == hipSuccess ? 0 : 1;
    if (rc != 0) set_error("intr_graph_capture: intr_step_begin_kernel failed to launch");
    if (rc == 0) rc = intr_run_stages(it, *b, 1, s);
    it->capturing = false;
    it->t = t; it->queue_ptr = qp; it->cat_counter = ctr;
    return rc;
}

int intr_graph_prepare(exorl_intr* it, const exorl_intr_batch* b, hipStream_t capture) {
    EXORL_TRY(check_intr_batch(it, b));
    EXORL_REQUIRE(it->world == 1, "agent_enable_graph_intr: a module with world_size=%d steps in phases with exchanges between them; "
                  "only the one-rank step is captured", it->world);
    EXORL_REQUIRE(!b->cat_uniform && !b->dobs_out, "agent_enable_graph_intr: a captured step draws from Philox (cat_uniform) and has no "
                  "encoder behind it (dobs_out): both must be null");
    if (!it->dev) EXORL_CHECK_HIP(hipMalloc((void**)&it->dev, sizeof(IntrStepState)));
    if (it->cfg.precision == EXORL_PREC_BF16X3) {
        // what the step's GEMMs ask of the plane arena: a throw-away capture of the same launches (nothing runs), then the arena is grown
        // outside any capture, so that the graph proper takes the kernels the eager step takes
        size_t need = 0;
        EXORL_CHECK_HIP(hipStreamBeginCapture(capture, hipStreamCaptureModeThreadLocal));
        gemm_planes_capture(true, &need);
        const int rc = intr_capture_body(it, b, capture);
        gemm_planes_capture(false, nullptr);
        hipGraph_t g = nullptr;
        const hipError_t e = hipStreamEndCapture(capture, &g);
        if (g) (void)hipGraphDestroy(g);
        if (rc != 0) return rc;
        if (e != hipSuccess) { set_error("agent_enable_graph_intr: sizing capture -> %s", hipGetErrorString(e)); return 1; }
        EXORL_TRY(gemm_planes_reserve(need));
    }
    EXORL_TRY(intr_push_state(it, capture));
    return 0;
}

int intr_graph_capture(exorl_intr* it, const exorl_intr_batch* b, hipStream_t capture) {
    EXORL_REQUIRE(it && it->dev, "intr_graph_capture: intr_graph_prepare first");
    gemm_planes_capture(true, nullptr);
    const int rc = intr_capture_body(it, b, capture);
    gemm_planes_capture(false, nullptr);
    return rc;
}

int intr_graph_before_launch(exorl_intr* it, hipStream_t s) {
    if (it->dev_stale) EXORL_TRY(intr_push_state(it, s));
    return 0;
}

void intr_graph_after_launch(exorl_intr* it) {      // what one exorl_intr_update(train = 1) does to the host's counters
    const auto& c = it->cfg;
    it->t += 1;
    if (c.kind == EXORL_INTR_PROTO || c.kind == EXORL_INTR_SMM) it->cat_counter += 1;
    if (c.kind == EXORL_INTR_PROTO) it->queue_ptr = (it->queue_ptr + c.num_protos) % c.queue_size;
}

void intr_graph_release(exorl_intr* it) { it->dev_stale = true; }

}  // namespace exorl

extern "C" {

static int check_intr_cfg(const exorl_intr_cfg* cfg) {
    EXORL_REQUIRE(cfg, "intr: null cfg");
    EXORL_REQUIRE(cfg->kind >= EXORL_INTR_RND && cfg->kind <= EXORL_INTR_SMM, "intr: unknown kind %d", cfg->kind);
    EXORL_REQUIRE(cfg->kind != EXORL_INTR_SMM || (cfg->rep_dim >= 1 && cfg->rep_dim <= 1024 && cfg->obs_dim >= 2 && cfg->sp_lr > 0.f && cfg->vae_lr > 0.f),
                  "intr: SMM needs z_dim in [1, 1024], obs_dim >= 2 (p* reads obs[:, :2]) and positive sp_lr / vae_lr");
    EXORL_REQUIRE(cfg->world_size >= 0 && cfg->rank >= 0 && cfg->rank < (cfg->world_size > 1 ? cfg->world_size : 1),
                  "intr: world_size=%d / rank=%d out of range (world_size 0 and 1: one rank)", cfg->world_size, cfg->rank);
    const int world = cfg->world_size > 1 ? cfg->world_size : 1, Bg = cfg->batch * world;     // kNN rows: this rank's against the gathered batch
    EXORL_REQUIRE(cfg->kind != EXORL_INTR_PROTO || (int64_t)cfg->batch * world <= 8192, "intr: Proto supports batch * world_size <= 8192 (its "
                  "Sinkhorn and candidate draw run over the global batch; got %d x %d)", cfg->batch, world);
    EXORL_REQUIRE(cfg->kind != EXORL_INTR_APS || (cfg->knn_k >= 1 && cfg->knn_k <= 64 && cfg->knn_k <= Bg && (int64_t)cfg->batch * world <= 8192),
                  "intr: APS needs 1 <= knn_k <= min(64, batch * world_size) and batch * world_size <= 8192 (got k=%d, %d x %d)", cfg->knn_k,
                  cfg->batch, world);
    EXORL_REQUIRE(cfg->kind != EXORL_INTR_PROTO || (cfg->num_protos >= 1 && cfg->queue_size >= cfg->num_protos && cfg->queue_size % cfg->num_protos == 0 &&
                  cfg->queue_size <= 4096 && cfg->knn_k >= 1 && cfg->knn_k <= 64 && cfg->knn_k <= cfg->queue_size && cfg->tau > 0.f && cfg->batch <= 8192),
                  "intr: Proto needs num_protos >= 1, queue_size a multiple of num_protos and <= 4096, 1 <= topk <= 64, tau > 0 (got %d, %d, %d, %g)",
                  cfg->num_protos, cfg->queue_size, cfg->knn_k, (double)cfg->tau);
    EXORL_REQUIRE(cfg->n_models >= 0 && cfg->n_models <= EXORL_MAX_ENSEMBLE, "intr: n_models=%d out of range (<= %d)", cfg->n_models, EXORL_MAX_ENSEMBLE);
    EXORL_REQUIRE(cfg->obs_dim > 0 && cfg->act_dim > 0 && cfg->act_dim <= 64 && cfg->hidden_dim > 0 && cfg->batch > 0,
                  "intr: unsupported dims O=%d A=%d (<=64) H=%d B=%d", cfg->obs_dim, cfg->act_dim, cfg->hidden_dim, cfg->batch);
    EXORL_REQUIRE(cfg->kind == EXORL_INTR_ICM || cfg->kind == EXORL_INTR_DISAGREEMENT || (cfg->rep_dim > 0 && (cfg->kind != EXORL_INTR_ICM_APT || cfg->rep_dim <= 1024)),
                  "intr: rep_dim=%d out of range (ICM-APT trunk: <= 1024)", cfg->rep_dim);
    EXORL_REQUIRE(cfg->kind != EXORL_INTR_ICM_APT || (cfg->knn_k >= 1 && cfg->knn_k <= 64 && cfg->knn_k <= Bg && (int64_t)cfg->batch * world <= 8192),
                  "intr: ICM-APT needs 1 <= knn_k <= min(64, batch * world_size) and batch * world_size <= 8192 (got k=%d, %d x %d)", cfg->knn_k,
                  cfg->batch, world);
    EXORL_REQUIRE(cfg->precision >= EXORL_PREC_F32 && cfg->precision <= EXORL_PREC_BF16X6, "intr: unknown precision %d", cfg->precision);
    return 0;
}

size_t exorl_intr_workspace_bytes(const exorl_intr_cfg* cfg) {
    if (check_intr_cfg(cfg) != 0) return 0;
    exorl_intr tmp;
    tmp.cfg = *cfg;
    describe_intr(&tmp);
    SimpleCarver sizing(nullptr);
    carve_intr(&tmp, sizing);
    return (size_t)sizing.off * sizeof(float);
}

int exorl_intr_create(const exorl_intr_cfg* cfg, void* workspace, size_t workspace_bytes, exorl_intr_t** out) {
    EXORL_REQUIRE(out, "intr_create: null argument");
    EXORL_TRY(check_intr_cfg(cfg));
    const size_t bytes = exorl_intr_workspace_bytes(cfg);
    EXORL_REQUIRE(!workspace || (workspace_bytes >= bytes && (reinterpret_cast<uintptr_t>(workspace) & 255) == 0),
                  "intr_create: workspace of %zu bytes (need %zu, 256-byte aligned)", workspace_bytes, bytes);
    auto* it = new exorl_intr();
    it->cfg = *cfg;
    it->world = cfg->world_size > 1 ? cfg->world_size : 1;
    it->rank = cfg->rank;
    describe_intr(it);
    if (workspace) {
        it->ws = static_cast<float*>(workspace);
    } else {
        if (hipMalloc(&it->ws, bytes) != hipSuccess) {
            set_error("intr_create: hipMalloc(%zu) failed", bytes);
            delete it;
            return 1;
        }
        it->owns_ws = true;
    }
    SimpleCarver c(it->ws);
    carve_intr(it, c);
    int rc = hipMemset(it->ws, 0, bytes) == hipSuccess ? 0 : 1;
    if (rc != 0) set_error("intr_create: hipMemset failed");
    if (rc == 0) rc = intr_reset_state(it);
    if (rc != 0) { if (it->owns_ws) (void)hipFree(it->ws); delete it; return rc; }
    *out = it;
    return 0;
}

int exorl_intr_destroy(exorl_intr_t* it) {
    if (!it) return 0;
    (void)hipDeviceSynchronize();
    if (it->dev) (void)hipFree(it->dev);
    if (it->owns_ws) (void)hipFree(it->ws);
    delete it;
    return 0;
}

int exorl_intr_num_tensors(exorl_intr_t* it, int32_t* n) {
    EXORL_REQUIRE(it && n, "intr_num_tensors: null argument");
    *n = (int32_t)it->tensors.size();
    return 0;
}

int exorl_intr_tensor(exorl_intr_t* it, int32_t index, int32_t what, void** ptr, int64_t* rows, int64_t* cols) {
    EXORL_REQUIRE(it && ptr && rows && cols, "intr_tensor: null argument");
    EXORL_REQUIRE(index >= 0 && index < (int32_t)it->tensors.size(), "intr_tensor: index %d out of range", index);
    EXORL_REQUIRE(what >= EXORL_T_PARAM && what <= EXORL_T_ADAM_V, "intr_tensor: unknown buffer %d", what);
    const TensorDesc& t = it->tensors[index];
    EXORL_REQUIRE(what == EXORL_T_PARAM || t.off < it->trainable, "intr_tensor: tensor %d is frozen (no gradient / optimiser state)", index);
    *ptr = it->flat[what] + t.off; *rows = t.rows; *cols = t.cols;
    return 0;
}

int exorl_intr_flat(exorl_intr_t* it, int32_t what, void** ptr, int64_t* numel) {
    EXORL_REQUIRE(it && ptr && numel, "intr_flat: null argument");
    EXORL_REQUIRE(what >= EXORL_T_PARAM && what <= EXORL_T_ADAM_V, "intr_flat: unknown buffer %d", what);
    *ptr = it->flat[what];
    *numel = what == EXORL_T_PARAM ? it->total : it->trainable;
    return 0;
}

int exorl_intr_state(exorl_intr_t* it, void** rms_dev, void** bn_dev, int64_t* bn_numel) {
    EXORL_REQUIRE(it && rms_dev && bn_dev && bn_numel, "intr_state: null argument");
    *rms_dev = it->rms; *bn_dev = it->bn; *bn_numel = it->bn ? 2 * it->cfg.obs_dim + 1 : 0;
    return 0;
}

}  // extern "C"

namespace exorl {
static int check_intr_batch(exorl_intr* it, const exorl_intr_batch* b) {
    EXORL_REQUIRE(it && b && b->obs && b->reward_out, "intr_update: null argument");
    const int k = it->cfg.kind;
    EXORL_REQUIRE(k == EXORL_INTR_RND || k == EXORL_INTR_SMM || b->next_obs, "intr_update: this module needs next_obs");
    EXORL_REQUIRE(k == EXORL_INTR_RND || k == EXORL_INTR_DIAYN || k == EXORL_INTR_PROTO || k == EXORL_INTR_APS || k == EXORL_INTR_SMM || b->action, "intr_update: this module needs action");
    EXORL_REQUIRE((k != EXORL_INTR_DIAYN && k != EXORL_INTR_APS && k != EXORL_INTR_SMM) || b->skill, "intr_update: DIAYN / APS / SMM need the skill / task matrix");
    EXORL_REQUIRE(b->obs_ld >= it->cfg.obs_dim && (!b->next_obs || b->next_obs_ld >= it->cfg.obs_dim) && (!b->action || b->action_ld >= it->cfg.act_dim) &&
                  (!b->skill || (k != EXORL_INTR_DIAYN && k != EXORL_INTR_APS && k != EXORL_INTR_SMM) || b->skill_ld >= it->cfg.rep_dim), "intr_update: a leading dimension is smaller than its row width");
    return 0;
}

// the one-rank step: its phases back to back (the gradient exchange between them is the identity)
static int intr_run_stages(exorl_intr* it, const exorl_intr_batch& b, int train, hipStream_t s) {
    int next = 0;
    for (int phase = 0; next >= 0; ++phase) EXORL_TRY(intr_phase(it, b, train, phase, &next, s));
    return 0;
}
}  // namespace exorl

extern "C" {

int exorl_intr_update(exorl_intr_t* it, const exorl_intr_batch* b, int32_t train, void* stream) {
    EXORL_TRY(check_intr_batch(it, b));
    EXORL_REQUIRE(it->world == 1, "intr_update: world_size=%d: drive exorl_intr_update_phase and run the exchange each phase names "
                  "(exorl_intr_exchange) across the ranks in between", it->world);
    it->dev_stale = true;                              // a joint graph re-reads the host's counters before its next launch
    return intr_run_stages(it, *b, train, as_stream(stream));
}

int exorl_intr_update_phase(exorl_intr_t* it, const exorl_intr_batch* b, int32_t train, int32_t phase, int32_t* next_exchange, void* stream) {
    EXORL_REQUIRE(next_exchange, "intr_update_phase: null next_exchange");
    *next_exchange = -1;
    EXORL_TRY(check_intr_batch(it, b));
    it->dev_stale = true;
    return intr_phase(it, *b, train, phase, next_exchange, as_stream(stream));
}

int exorl_intr_exchange(exorl_intr_t* it, int32_t id, void** ptr_dev, int64_t* count, int32_t* dtype, int32_t* op) {
    EXORL_REQUIRE(it && ptr_dev && count && dtype && op, "intr_exchange: null argument");
    if (id == EXORL_INTR_XCHG_GRAD) {
        *ptr_dev = it->flat[EXORL_T_GRAD]; *count = it->trainable; *dtype = EXORL_XCHG_F32; *op = EXORL_XCHG_SUM;
    } else if (id == EXORL_INTR_XCHG_REP) {
        EXORL_REQUIRE(it->gat, "intr_exchange: exchange %d belongs to ICM-APT / APS / Proto with world_size > 1", id);
        *ptr_dev = it->gat; *count = (int64_t)it->cfg.batch * it->cfg.rep_dim; *dtype = EXORL_XCHG_F32; *op = EXORL_XCHG_GATHER;
    } else if (id == EXORL_INTR_XCHG_MOMENTS) {
        EXORL_REQUIRE(it->mom, "intr_exchange: exchange %d belongs to RND / ICM-APT / APS / SMM on states with world_size > 1", id);
        *ptr_dev = it->mom; *count = 3; *dtype = EXORL_XCHG_F64; *op = EXORL_XCHG_GATHER;
    } else if (id == EXORL_INTR_XCHG_BN) {
        EXORL_REQUIRE(it->bnmom, "intr_exchange: exchange %d belongs to RND on state rows with world_size > 1", id);
        *ptr_dev = it->bnmom; *count = (int64_t)3 * it->cfg.obs_dim; *dtype = EXORL_XCHG_F64; *op = EXORL_XCHG_GATHER;
    } else {
        EXORL_REQUIRE(false, "intr_exchange: unknown exchange %d", id);
    }
    return 0;
}

int exorl_intr_queue(exorl_intr_t* it, void** queue_dev, int64_t* rows, int64_t* cols, int64_t* ptr_inout, int32_t set) {
    EXORL_REQUIRE(it && queue_dev && rows && cols && ptr_inout && it->queue, "intr_queue: not a Proto module / null argument");
    *queue_dev = it->queue; *rows = it->cfg.queue_size; *cols = it->cfg.rep_dim;
    if (set) {
        EXORL_REQUIRE(*ptr_inout >= 0 && *ptr_inout < it->cfg.queue_size && *ptr_inout % it->cfg.num_protos == 0, "intr_queue: bad write pointer");
        it->queue_ptr = *ptr_inout;
        it->dev_stale = true;
    } else {
        *ptr_inout = it->queue_ptr;
    }
    return 0;
}

int exorl_intr_metrics(exorl_intr_t* it, float* host, void* stream) {
    EXORL_REQUIRE(it && host, "intr_metrics: null argument");
    EXORL_CHECK_HIP(hipMemcpyAsync(host, it->metrics, sizeof(float) * EXORL_N_INTR_METRICS, hipMemcpyDeviceToHost, as_stream(stream)));
    EXORL_CHECK_HIP(hipStreamSynchronize(as_stream(stream)));
    return 0;
}

int exorl_intr_opt_steps(exorl_intr_t* it, int64_t* steps, int32_t set) {
    EXORL_REQUIRE(it && steps, "intr_opt_steps: null argument");
    if (set) { EXORL_REQUIRE(*steps >= 0, "intr_opt_steps: negative step count"); it->t = *steps; it->dev_stale = true; }
    else *steps = it->t;
    return 0;
}

int exorl_intr_counter(exorl_intr_t* m, uint64_t* counter_inout, int32_t set) {
    EXORL_REQUIRE(m && counter_inout, "intr_counter: null argument");
    if (set) { m->cat_counter = *counter_inout; m->dev_stale = true; }
    else *counter_inout = m->cat_counter;
    return 0;
}

}  // extern "C"
