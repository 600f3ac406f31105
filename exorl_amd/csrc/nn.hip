// Exact 1-nearest-neighbour search of a batch of queries against a key table resident in HBM, and the table's build from the replay arena:
// the hot path of the PRDC agent (policy regularisation with dataset constraint, Ran et al., ICML 2023: the BC target of TD3+BC's actor step
// becomes the action of the dataset point nearest to (beta s, mu(s)); the authors search a CPU KD-tree, here the whole table is streamed).
// knn.hip stops at 8192 targets and writes the distance matrix; this search never writes a distance.
//   nn_build_keys_kernel  one workgroup per (episode of the order table, 64-transition chunk), as obs_moments_partial_kernel walks the arena:
//     key row i / key_every for the running transition index i = [beta (x - mean) inv_scale | action | 0-pad], the observation columns with
//     the gather's own two uncontracted fp32 operations and one further product.
//   nn_query_kernel       q = [beta obs | mu(obs) | 0-pad] per batch row, the same product.
//   nn_partial_kernel     a workgroup owns 64 queries (held in LDS for the whole launch) and one of S contiguous key ranges; it streams its
//     range in 64-key tiles of 32 columns through LDS (pairdist2_kernel's layout: row stride 36 floats, ds_read_b128 along the columns,
//     conflict-free over 16 consecutive rows; the next tile's global loads are in flight while this one is computed) and a thread keeps a
//     4 x 4 block of squared distances in the difference form, sum_c (q_c - k_c)^2 with c ascending in one accumulator per pair. After a
//     tile's last column chunk a thread folds its 16 distances into a running (d2, index) per query it owns, keys in ascending order with a
//     strict <, so a tie keeps the lower index; the 16 threads of a query combine by the lexicographic (d2, index) minimum (associative and
//     commutative: the shuffle order does not matter) and leave one pair per (query, range).
//   nn_merge_kernel       one thread per query: the S pairs in range order by the same minimum; writes idx, d2 and gathers the action
//     columns of the winning key row.
// The bits of d2 of a pair depend on the pair alone (column order and the code that adds them are fixed), never on S, the tile or the
// thread; the minimum is exact, so idx and d2 are the same bits for every split. No atomics.
// Grid order: workgroups that read the same key range are given linear ids equal modulo 8, 8 apart, so that under the round-robin
// placement of workgroups over the 8 XCDs they run together on one XCD and the range comes out of that XCD's L2 for all but the first of
// them. Placement is a matter of speed only.
#include "kernels.h"

namespace exorl {

constexpr int NN_T = 64, NN_K = 32, NN_LD = NN_K + 4;

__global__ __launch_bounds__(256) void nn_build_keys_kernel(NnKeyBuild b) {
#pragma clang fp contract(off)
    const int it = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int e = 0;                                    // the episode of item `it`: item0[e] <= it < item0[e + 1]
    for (int hi = b.n_episodes; hi - e > 1;) {
        const int mid = (e + hi) >> 1;
        if (b.item0[mid] <= it) e = mid; else hi = mid;
    }
    const int t0 = (it - b.item0[e]) * NN_T, t1 = min(t0 + NN_T, b.len[e]);      // transitions t0 + 1 .. t1 of the episode
    const int64_t row0 = b.row0[e], i0 = b.trans0[e];
    for (int tt = t0 + wave; tt < t1; tt += 4) {
        const int64_t i = i0 + tt;
        if (i % b.every) continue;
        float* k = b.keys + (i / b.every) * b.pitch;
        const float* x = b.obs + (row0 + tt) * b.O;           // obs[t - 1], t = tt + 1
        const float* a = b.act + (row0 + tt + 1) * b.A;       // action[t]
        for (int j = lane; j < b.pitch; j += 64) {
            float v = 0.f;
            if (j < b.O) {
                v = x[j];
                if (b.mean) { v = v - b.mean[j]; v = v * b.inv[j]; }
                v = b.beta * v;
            } else if (j < b.O + b.A) {
                v = a[j - b.O];
            }
            k[j] = v;
        }
    }
}

int nn_build_keys(const NnKeyBuild& b, hipStream_t s) {
    hipLaunchKernelGGL(nn_build_keys_kernel, dim3(b.n_items), dim3(256), 0, s, b);
    EXORL_LAUNCH_CHECK();
    return 0;
}

__global__ __launch_bounds__(256) void nn_query_kernel(const float* __restrict__ obs, const float* __restrict__ mu, float beta, int rows, int O,
                                                       int A, int pitch, float* __restrict__ q) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)rows * pitch) return;
    const int b = (int)(i / pitch), j = (int)(i % pitch);
    q[i] = j < O ? beta * obs[(int64_t)b * O + j] : j < O + A ? mu[(int64_t)b * A + j - O] : 0.f;
}

int nn_query(const float* obs, const float* mu, float beta, int rows, int O, int A, int pitch, float* q, hipStream_t s) {
    hipLaunchKernelGGL(nn_query_kernel, dim3(cdiv((int64_t)rows * pitch, 256)), dim3(256), 0, s, obs, mu, beta, rows, O, A, pitch, q);
    EXORL_LAUNCH_CHECK();
    return 0;
}

__device__ __forceinline__ void nn_take_min(float& best, int& bi, float ob, int oi) {
    if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
}

__global__ __launch_bounds__(256) void nn_partial_kernel(const float* __restrict__ keys, int n, int pitch, int dim, int vec,
                                                         const float* __restrict__ q, int64_t q_ld, int rows, int q_tiles, int splits,
                                                         int tiles_per_split, float* __restrict__ part_d2, int* __restrict__ part_idx) {
    extern __shared__ __attribute__((aligned(16))) float nn_smem[];
    const int dpad = (dim + NN_K - 1) / NN_K * NN_K, qld = dpad + 4, nch = dpad / NN_K;
    float* Q = nn_smem;                       // [NN_T][qld]: the query tile, whole rows
    float* K = nn_smem + NN_T * qld;          // [NN_T][NN_LD]: one column chunk of one key tile
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    // linear id -> (key range r, query tile t): ids r % 8 + 8 t + 8 q_tiles (r / 8), see the header
    const int per = 8 * q_tiles, w = blockIdx.x % per;
    const int t = w >> 3, r = (blockIdx.x / per) * 8 + (w & 7);
    if (r >= splits) return;                  // the whole workgroup, ahead of every barrier
    const int s0 = t * NN_T;
    const int tiles = (n + NN_T - 1) / NN_T;
    const int tile_lo = r * tiles_per_split, tile_hi = min(tile_lo + tiles_per_split, tiles);      // not empty: nn_plan leaves no empty range
    for (int i = tid; i < NN_T * dpad; i += 256) {
        const int rr = i / dpad, c = i - rr * dpad;
        Q[rr * qld + c] = (s0 + rr < rows && c < dim) ? q[(int64_t)(s0 + rr) * q_ld + c] : 0.f;
    }
    float4 pre[2];
    auto fetch = [&](int step) {
        const int tile = tile_lo + step / nch, c0 = (step % nch) * NN_K;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int idx = tid + 256 * u, rr = idx >> 3, c = c0 + 4 * (idx & 7);
            const int row = tile * NN_T + rr;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (row < n) {
                const float* p = keys + (int64_t)row * pitch + c;
                if (vec && c + 4 <= pitch) {
                    const float4 f = *reinterpret_cast<const float4*>(p);
                    v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (c + k < pitch) v[k] = p[k];
                }
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c + k >= dim) v[k] = 0.f;          // columns past `dim` (the table's pad) never count
            }
            pre[u] = make_float4(v[0], v[1], v[2], v[3]);
        }
    };
    float best[4];
    int bi[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { best[i] = INFINITY; bi[i] = tile_lo * NN_T; }      // a valid index whatever the distances are
    float acc[4][4];
    const int total = (tile_hi - tile_lo) * nch;
    fetch(0);
    for (int step = 0; step < total; ++step) {
        __syncthreads();                      // the previous chunk has been read (first pass: nothing); Q is written before the second barrier
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int idx = tid + 256 * u;
            *reinterpret_cast<float4*>(K + (idx >> 3) * NN_LD + 4 * (idx & 7)) = pre[u];
        }
        __syncthreads();
        if (step + 1 < total) fetch(step + 1);
        const int ch = step % nch;
        if (ch == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
        }
        const float* Qc = Q + ch * NN_K;
#pragma unroll 2
        for (int c = 0; c < NN_K; c += 4) {
            float4 sv[4], tv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                sv[i] = *reinterpret_cast<const float4*>(Qc + (ty + 16 * i) * qld + c);
                tv[i] = *reinterpret_cast<const float4*>(K + (tx + 16 * i) * NN_LD + c);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float d = sv[i].x - tv[j].x; acc[i][j] += d * d;
                    d = sv[i].y - tv[j].y; acc[i][j] += d * d;
                    d = sv[i].z - tv[j].z; acc[i][j] += d * d;
                    d = sv[i].w - tv[j].w; acc[i][j] += d * d;
                }
        }
        if (ch == nch - 1) {
            const int k0 = (tile_lo + step / nch) * NN_T + tx;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {           // this thread's keys in ascending order: a tie keeps the earlier one
                    const int key = k0 + 16 * j;
                    if (key < n && acc[i][j] < best[i]) { best[i] = acc[i][j]; bi[i] = key; }
                }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) {         // the 16 threads of a query are 16 consecutive lanes
            const float ob = __shfl_xor(best[i], off, 64);
            const int oi = __shfl_xor(bi[i], off, 64);
            nn_take_min(best[i], bi[i], ob, oi);
        }
        const int row = s0 + ty + 16 * i;
        if (tx == 0 && row < rows) {
            part_d2[(int64_t)r * rows + row] = best[i];
            part_idx[(int64_t)r * rows + row] = bi[i];
        }
    }
}

__global__ __launch_bounds__(256) void nn_merge_kernel(const float* __restrict__ part_d2, const int* __restrict__ part_idx, int splits, int rows,
                                                       const float* __restrict__ keys, int pitch, int act_col0, int act_dim,
                                                       int* __restrict__ idx_out, float* __restrict__ d2_out, float* __restrict__ a_nn) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= rows) return;
    float best = part_d2[b];
    int bi = part_idx[b];
    for (int s = 1; s < splits; ++s) nn_take_min(best, bi, part_d2[(int64_t)s * rows + b], part_idx[(int64_t)s * rows + b]);
    idx_out[b] = bi;
    d2_out[b] = best;
    if (a_nn)
        for (int k = 0; k < act_dim; ++k) a_nn[(int64_t)b * act_dim + k] = keys[(int64_t)bi * pitch + act_col0 + k];
}

// metrics slot = inv_bg * sum_b sqrt(d2[b]): thread t adds rows t, t + 256, ... in that order, then a fixed tree
__global__ __launch_bounds__(256) void nn_dist_kernel(const float* __restrict__ d2, int rows, float inv_bg, float* __restrict__ out) {
    __shared__ float s[256];
    float acc = 0.f;
    for (int b = threadIdx.x; b < rows; b += 256) acc += sqrtf(d2[b]);
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if (threadIdx.x < half) s[threadIdx.x] += s[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = s[0] * inv_bg;
}

int nn_dist(const float* d2, int rows, float inv_bg, float* out, hipStream_t s) {
    hipLaunchKernelGGL(nn_dist_kernel, dim3(1), dim3(256), 0, s, d2, rows, inv_bg, out);
    EXORL_LAUNCH_CHECK();
    return 0;
}

// The key ranges of a search over n keys: `want` of them (0: the library's choice, about four workgroups per CU over the query tiles),
// at most NN_MAX_SPLITS and never an empty one.
NnPlan nn_plan(int n, int rows, int want, int cus) {
    const int tiles = cdiv(n, NN_T), q_tiles = cdiv(rows, NN_T);
    int S = want > 0 ? want : cdiv(4 * (int64_t)(cus > 0 ? cus : 256), q_tiles);
    S = S < 1 ? 1 : S > NN_MAX_SPLITS ? NN_MAX_SPLITS : S;
    if (S > tiles) S = tiles;
    NnPlan p;
    p.tiles_per_split = cdiv(tiles, S);
    p.splits = cdiv(tiles, p.tiles_per_split);
    p.q_tiles = q_tiles;
    return p;
}

int nn_device_cus(int* cus) {
    static int cached = 0;
    if (!cached) {
        int dev = 0;
        EXORL_CHECK_HIP(hipGetDevice(&dev));
        hipDeviceProp_t prop;
        EXORL_CHECK_HIP(hipGetDeviceProperties(&prop, dev));
        cached = prop.multiProcessorCount;
    }
    *cus = cached;
    return 0;
}

int nn_search(const NnSearch& a, hipStream_t s) {
    EXORL_REQUIRE(a.n > 0 && a.rows > 0 && a.dim > 0 && a.pitch >= a.dim && a.q_ld >= a.dim, "nn_search: bad sizes n=%d rows=%d dim=%d pitch=%d q_ld=%lld",
                  a.n, a.rows, a.dim, a.pitch, (long long)a.q_ld);
    EXORL_REQUIRE(a.dim <= NN_MAX_DIM, "nn_search: dim=%d (max %d)", a.dim, NN_MAX_DIM);
    EXORL_REQUIRE(a.plan.splits >= 1 && a.plan.splits <= NN_MAX_SPLITS && (int64_t)a.plan.splits * a.plan.tiles_per_split >= cdiv(a.n, NN_T) &&
                  (int64_t)(a.plan.splits - 1) * a.plan.tiles_per_split < cdiv(a.n, NN_T) && a.plan.q_tiles == cdiv(a.rows, NN_T),
                  "nn_search: the plan (%d ranges of %d tiles, %d query tiles) does not cover n=%d, rows=%d", a.plan.splits, a.plan.tiles_per_split,
                  a.plan.q_tiles, a.n, a.rows);
    static bool attr = false;
    if (!attr) {
        EXORL_CHECK_HIP(hipFuncSetAttribute((const void*)nn_partial_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr = true;
    }
    const int dpad = (int)round_up(a.dim, NN_K);
    const size_t lds = sizeof(float) * ((size_t)NN_T * (dpad + 4) + (size_t)NN_T * NN_LD);
    const int vec = (a.pitch % 4 == 0 && reinterpret_cast<uintptr_t>(a.keys) % 16 == 0) ? 1 : 0;
    const int groups = cdiv(a.plan.splits, 8);
    hipLaunchKernelGGL(nn_partial_kernel, dim3(groups * 8 * a.plan.q_tiles), dim3(256), lds, s, a.keys, a.n, a.pitch, a.dim, vec, a.q, a.q_ld,
                       a.rows, a.plan.q_tiles, a.plan.splits, a.plan.tiles_per_split, a.part_d2, a.part_idx);
    EXORL_LAUNCH_CHECK();
    hipLaunchKernelGGL(nn_merge_kernel, dim3(cdiv(a.rows, 256)), dim3(256), 0, s, a.part_d2, a.part_idx, a.plan.splits, a.rows, a.keys, a.pitch,
                       a.act_col0, a.act_dim, a.idx_out, a.d2_out, a.a_nn);
    EXORL_LAUNCH_CHECK();
    return 0;
}

}  // namespace exorl

extern "C" int exorl_nn_search(const float* keys, int64_t n, int32_t pitch, int32_t dim, const float* queries, int64_t q_ld, int32_t rows,
                               int32_t splits, int32_t* idx_out, float* d2_out, void* stream) {
    using namespace exorl;
    EXORL_REQUIRE(keys && queries && idx_out && d2_out, "nn_search: null argument");
    EXORL_REQUIRE(n > 0 && n <= INT32_MAX - NN_T && rows > 0 && dim > 0 && dim <= NN_MAX_DIM && pitch >= dim && q_ld >= dim && splits >= 0,
                  "nn_search: unsupported sizes n=%lld rows=%d dim=%d (max %d) pitch=%d q_ld=%lld splits=%d", (long long)n, rows, dim, NN_MAX_DIM,
                  pitch, (long long)q_ld, splits);
    hipStream_t s = as_stream(stream);
    int cus = 0;
    EXORL_TRY(nn_device_cus(&cus));
    NnSearch a{};
    a.keys = keys; a.n = (int)n; a.pitch = pitch; a.dim = dim; a.q = queries; a.q_ld = q_ld; a.rows = rows;
    a.plan = nn_plan((int)n, rows, splits, cus);
    // stand-alone entry (tests, callers without a workspace): library-owned scratch, grown on demand outside graph capture
    static float* scratch = nullptr;
    static size_t scratch_floats = 0;
    const size_t need = 2 * (size_t)a.plan.splits * rows;
    if (need > scratch_floats) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        EXORL_CHECK_HIP(hipStreamIsCapturing(s, &cs));
        EXORL_REQUIRE(cs == hipStreamCaptureStatusNone, "nn_search: the stand-alone entry sizes its scratch on first use; call it once before capturing");
        EXORL_CHECK_HIP(hipDeviceSynchronize());
        if (scratch) EXORL_CHECK_HIP(hipFree(scratch));
        scratch = nullptr; scratch_floats = 0;
        EXORL_CHECK_HIP(hipMalloc(&scratch, need * sizeof(float)));
        scratch_floats = need;
    }
    a.part_d2 = scratch; a.part_idx = reinterpret_cast<int*>(scratch + (size_t)a.plan.splits * rows);
    a.idx_out = idx_out; a.d2_out = d2_out;
    return nn_search(a, s);
}
