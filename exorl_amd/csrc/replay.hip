// HBM-resident episodic replay buffer with a gather + n-step-return relabel kernel.
// Replaces /root/reference/utils/replay_buffer.py:153-239 (ReplayBuffer._store_episode/_sample) and the
// DataLoader collate at :260-277: one launch emits a whole coalesced (s, a, R, D, s') minibatch.
//
// Layout: a row arena (SoA) — obs[rows][obs_bytes], action[rows][A], reward[rows], discount[rows],
// meta[rows][Mt] — episodes are len+1 consecutive rows (row 0 = dummy reset step, replay_buffer.py:13-15);
// an episode table (row0, len) in the reference's sorted `_episode_fns` order lives beside it.
// Kernel: one wave per sample; lanes stream the obs / next_obs rows as 16-byte (or 4-byte) words, lane 0
// runs the n-step recurrence with products and sums rounded separately (no FMA contraction) so values are
// bit-identical to NumPy's fp32 arithmetic (replay_buffer.py:229-234). HBM-bound, ~2*(2*obs_bytes+4A+8) B/sample.
//
// Index streams: EXORL_SAMPLER_MT19937 reproduces the reference's two MT19937 streams on the host
// (CPython random.choice -> _randbelow_with_getrandbits; NumPy legacy randint masked rejection) and ships the
// B index pairs with one async copy; EXORL_SAMPLER_PHILOX draws them in the kernel (Philox4x32-10).
//
// Weighted sampling (exorl_replay_set_weights, Philox only): every slot carries an integer weight q_e and the table gains a uint64
// prefix sum `cum` of the episode masses (TRANSITIONS: q_e * span_e, EPISODES: q_e where span_e > 0; span_e = len_e - nstep + 1
// clamped at 0). The kernel scales 64 Philox bits onto [0, cum[n]) and binary-searches the episode; zero-mass episodes own an empty
// interval and are never drawn. With unit weights TRANSITIONS mode is uniform over transitions.
//
// Frame stacking (exorl_replay_set_frame_stack(k), k > 1): an obs row holds the ONE frame the env produced at that step (obs_bytes = one
// frame) and a sampled observation is k of them, oldest first: the stack at step t is rows max(t - k + 1, 0) .. t of the episode, what the
// wrapper's deque(maxlen=k), filled with the reset frame, held (utils/env_constructor.py:144-188). gather_frames_kernel gives one wave to
// each of the 2 k frames of a sample; gather_nstep_kernel, its arguments and its launch are those of an arena without stacking.
//
// Observation normalisation (fp32 state arenas): exorl_replay_obs_moments reduces the resident rows to fp64 column moments in two launches
// (obs_moments_partial_kernel: Welford per thread, Chan between threads, one partial per workgroup in a slab; obs_moments_combine_kernel: the
// slab in slab order), and exorl_replay_set_obs_norm makes gather_nstep_kernel<true> write y = (x - mean[j]) * inv_scale[j] wherever the plain
// instantiation copies an observation element, the staged network inputs included.
//
// Return-to-go column (exorl_replay_build_returns): one float per arena row, G_i = r_i + (gamma d_i) G_{i+1} carried to the episode's end in fp64
// (returns_to_go_kernel, one launch over the order table). The gather writes G[row0 + idx] beside reward and discount when
// exorl_replay_sample_mc names a destination: Cal-QL's lower bound on the critic. Stale once an episode is appended or evicted or the order changes.
//
// Goal relabelling (exorl_replay_set_goal, exorl_replay_sample_goal; fp32 state arenas): every sample also gets a goal, a pair (pos_g, tau)
// naming arena row row0[pos_g] + tau: the state its own trajectory reaches at next_obs (CUR) or later (TRAJ), or any state of the arena (RAND),
// drawn from Philox blocks 1 and 2 of the sample's counter (block 0, the sample's own pair, keeps its bits) or shipped by the caller. The same
// gather launch writes the goal's columns g = o[cols] (through the normaliser when it is on) behind obs and behind next_obs, and in the 'neg' and
// 'sparse' modes feeds sample_tail's recurrence "reached / not reached" per-step inputs instead of the arena's reward and discount. The goal
// path is gather_nstep_kernel<NORM, GoalView>, chosen on the host; the instantiations without a goal take no further argument and are unchanged.
#include <algorithm>
#include <vector>

#include "kernels.h"

namespace exorl {

// ---- MT19937 (host) ----------------------------------------------------------------------------
struct MT19937 {
    uint32_t mt[624];
    int pos = 624;
    void init_genrand(uint32_t s) {
        mt[0] = s;
        for (int i = 1; i < 624; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
        pos = 624;
    }
    void init_by_array(const uint32_t* key, int klen) {
        init_genrand(19650218u);
        int i = 1, j = 0;
        for (int k = (624 > klen ? 624 : klen); k; --k) {
            mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1664525u)) + key[j] + (uint32_t)j;
            ++i; ++j;
            if (i >= 624) { mt[0] = mt[623]; i = 1; }
            if (j >= klen) j = 0;
        }
        for (int k = 623; k; --k) {
            mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1566083941u)) - (uint32_t)i;
            ++i;
            if (i >= 624) { mt[0] = mt[623]; i = 1; }
        }
        mt[0] = 0x80000000u;
        pos = 624;
    }
    void twist() {
        for (int k = 0; k < 624; ++k) {
            const uint32_t y = (mt[k] & 0x80000000u) | (mt[(k + 1) % 624] & 0x7FFFFFFFu);
            uint32_t v = mt[(k + 397) % 624] ^ (y >> 1);
            if (y & 1u) v ^= 0x9908B0DFu;
            mt[k] = v;
        }
        pos = 0;
    }
    uint32_t next() {
        if (pos >= 624) twist();
        uint32_t y = mt[pos++];
        y ^= y >> 11;
        y ^= (y << 7) & 0x9D2C5680u;
        y ^= (y << 15) & 0xEFC60000u;
        y ^= y >> 18;
        return y;
    }
    // CPython random._randbelow_with_getrandbits(n), 0 < n < 2^32
    uint32_t py_randbelow(uint32_t n) {
        int k = 32 - __builtin_clz(n);
        uint32_t r = next() >> (32 - k);
        while (r >= n) r = next() >> (32 - k);
        return r;
    }
    // NumPy legacy RandomState.randint(0, hi), hi >= 1
    uint32_t np_randint0(uint32_t hi) {
        const uint32_t rng = hi - 1;
        if (rng == 0) return 0;
        uint32_t mask = rng;
        mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
        uint32_t v = next() & mask;
        while (v > rng) v = next() & mask;
        return v;
    }
};

struct Slot {
    int64_t row0;
    int32_t rows;
    bool live;
};

}  // namespace exorl

using namespace exorl;

struct exorl_replay {
    exorl_replay_cfg cfg;
    unsigned char* obs = nullptr;
    float *act = nullptr, *rew = nullptr, *disc = nullptr, *meta = nullptr;
    int64_t used_rows = 0, live_rows = 0;
    std::vector<Slot> slots;
    std::vector<int32_t> order;
    int64_t* d_row0 = nullptr;
    int32_t* d_len = nullptr;
    int32_t* d_pairs = nullptr;
    int pairs_cap = 0;
    bool table_dirty = true;
    int32_t min_len = 0;
    MT19937 py, np;
    bool mt_seeded = false;
    uint64_t philox_seed = 0, philox_counter = 0;
    std::vector<int32_t> h_pairs;
    std::vector<int64_t> h_row0;
    std::vector<int32_t> h_len;
    // weighted sampling: q per slot, the mode, and the prefix sum of the masses in table order for `cum_nstep`
    std::vector<uint32_t> weight;
    int32_t weight_mode = EXORL_WEIGHT_EPISODES;
    bool weighted = false;            // false: the unweighted sampler, no cum table
    uint64_t* d_cum = nullptr;        // max_episodes + 1 entries, allocated at create: its address is stable across graph replays
    std::vector<uint64_t> h_cum;
    int32_t cum_nstep = -1;           // -1: stale
    // cut-point table over the top guide_bits bits of the 64 random bits: guide[k] = the episode of the smallest g of bucket k, so the
    // search of a draw in bucket k runs over [guide[k], guide[k + 1]] only (>= 2 buckets per episode: O(1) expected loads)
    int32_t* d_guide = nullptr;       // guide_cap + 1 entries, allocated at create
    std::vector<int32_t> h_guide;
    int32_t guide_cap = 0, guide_bits = 0;
    uint64_t weights_epoch = 0;       // counts exorl_replay_set_weights calls (a captured step graph refuses to replay across one)
    int32_t frames = 1;               // frames per sampled observation (exorl_replay_set_frame_stack); 1: a row is the whole observation
    // observation normaliser: mean[obs_bytes / 4] then inv_scale[obs_bytes / 4], allocated at create (its address is stable across graph replays)
    float* d_norm = nullptr;
    std::vector<float> h_norm;
    bool norm_on = false;             // which gather_nstep_kernel is launched (a captured step graph holds the kernel of its capture)
    // exorl_replay_obs_moments' scratch, allocated on first use: the item prefix per episode and the slab of workgroup partials + the result
    int32_t* d_item0 = nullptr;
    double* d_slab = nullptr;
    std::vector<int32_t> h_item0;
    std::vector<double> h_moments;
    double* d_returns = nullptr;      // exorl_replay_episode_returns' output, max_episodes doubles, allocated on first use
    // exorl_replay_build_keys' table (nn.hip): a snapshot of the resident transitions, stale once the arena, its order or its normaliser moves
    float* d_keys = nullptr;
    size_t keys_cap = 0;              // floats allocated
    int64_t keys_n = 0;
    float keys_beta = 0.f;
    int32_t keys_every = 1;
    bool keys_valid = false;
    uint64_t keys_epoch = 0;          // counts builds and invalidations: an agent bound to the table holds the value of its build
    int32_t* d_kitem0 = nullptr;      // the build's item and transition prefix per episode, max_episodes + 1 entries each, allocated on first use
    int64_t* d_ktrans0 = nullptr;
    std::vector<int32_t> h_kitem0;
    std::vector<int64_t> h_ktrans0;
    void keys_stale() { if (keys_valid) { keys_valid = false; keys_epoch += 1; } }
    // exorl_replay_build_returns' column: capacity_rows floats, allocated at the first build and never moved (a captured graph holds the
    // pointer); stale once an episode is appended or evicted or the order table is set. Weights, the normaliser and the frame stack leave it.
    float* d_rtg = nullptr;
    float rtg_gamma = 0.f;
    bool rtg_valid = false;
    uint64_t rtg_epoch = 0;           // counts builds and invalidations
    std::vector<float> h_rtg;         // exorl_replay_returns_read's bounce buffer
    void returns_stale() { if (rtg_valid) { rtg_valid = false; rtg_epoch += 1; } }
    // exorl_replay_set_goal: the goal columns and the geometric horizon's table, allocated at the first call and never moved (a captured graph
    // holds the pointers; every other value below is a kernel argument, so a graph is bound to the goal_epoch of its capture)
    int32_t* d_goal_cols = nullptr;   // obs_bytes / 4 entries, the first goal_n in use
    uint32_t* d_goal_tab = nullptr;   // GOAL_TAB_MAX entries, the first goal_tab_n in use
    int32_t goal_n = 0;               // 0: no goal rule set
    int32_t goal_tab_n = 0;           // 0: the uniform horizon
    uint64_t goal_t_cur = 0, goal_t_traj = 0;
    int32_t goal_mode = EXORL_GOAL_KEEP;
    uint64_t goal_epoch = 0;          // counts exorl_replay_set_goal calls
    int32_t* d_goals = nullptr;       // the (pos_g, tau) pairs of the last goal launch, goals_cap of them
    int goals_cap = 0;
    std::vector<int32_t> h_goals;
};

namespace exorl {

struct ReplayView {
    const unsigned char* obs;
    const float *act, *rew, *disc, *meta;
    const int64_t* row0;
    const int32_t* len;
    int32_t obs_bytes, act_dim, meta_dim, n_episodes;
    const uint64_t* cum;      // null: unweighted; else n_episodes + 1 prefix sums of the episode masses, cum[n_episodes] the total
    const int32_t* guide;     // (1 << guide_bits) + 1 cut points into cum, indexed by the top guide_bits bits of the draw
    int32_t guide_bits;
    const float *norm_mean, *norm_inv;      // null: observations are copied; else obs_bytes / 4 floats each, y = (x - mean[j]) * inv[j]
    const float* rtg;         // the return-to-go column, one float per arena row; read only where the launch has a destination for it
};

constexpr int GOAL_TAB_MAX = 4096;

// What the goal path of the gather reads beside the ReplayView: the rule of exorl_replay_set_goal and the destinations of this launch.
struct GoalView {
    const int32_t* cols;      // n_cols observation column indices: g[j] = o[cols[j]]
    int32_t n_cols;
    uint64_t t_cur, t_traj;   // the source thresholds on x[0]: floor(p_cur 2^32), floor((p_cur + p_traj) 2^32)
    const uint32_t* tab;      // the geometric horizon's table, tab[k] = floor(2^32 (1 - gamma_h^(k+1))), ascending; n_tab == 0: uniform
    int32_t n_tab;
    int32_t reward_mode;      // EXORL_GOAL_KEEP / _NEG / _SPARSE
    int32_t* goals;           // batch (pos_g, tau) pairs: written by a Philox launch, read by the others
    float *goal, *next_goal;  // destinations, strides in floats
    int64_t goal_stride, next_goal_stride;
};

__device__ __forceinline__ void copy_row(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                         int bytes, int lane, bool vec16) {
    if (vec16) {
        const uint4* s = reinterpret_cast<const uint4*>(src);
        uint4* d = reinterpret_cast<uint4*>(dst);
        for (int i = lane; i < bytes / 16; i += 64) d[i] = s[i];
    } else {
        const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
        uint32_t* d = reinterpret_cast<uint32_t*>(dst);
        for (int i = lane; i < bytes / 4; i += 64) d[i] = s[i];
    }
}

// copy_row of an fp32 row through the normaliser: two roundings per element, the subtraction then the product.
__device__ __forceinline__ void norm_row(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int bytes, int lane, bool vec16,
                                         const float* __restrict__ mean, const float* __restrict__ inv) {
#pragma clang fp contract(off)
    if (vec16) {
        const float4* s = reinterpret_cast<const float4*>(src);
        const float4* m = reinterpret_cast<const float4*>(mean);
        const float4* w = reinterpret_cast<const float4*>(inv);
        float4* d = reinterpret_cast<float4*>(dst);
        for (int i = lane; i < bytes / 16; i += 64) {
            const float4 x = s[i], mu = m[i], sc = w[i];
            float4 y;
            y.x = (x.x - mu.x) * sc.x; y.y = (x.y - mu.y) * sc.y; y.z = (x.z - mu.z) * sc.z; y.w = (x.w - mu.w) * sc.w;
            d[i] = y;
        }
    } else {
        const float* s = reinterpret_cast<const float*>(src);
        float* d = reinterpret_cast<float*>(dst);
        for (int i = lane; i < bytes / 4; i += 64) d[i] = (s[i] - mean[i]) * inv[i];
    }
}

// The episode a Philox block picks, wave-uniform: on a weighted arena 64 of its bits scaled onto [0, total) and searched in cum through the
// guide table (pos = the episode whose interval [cum[pos], cum[pos+1]) holds g), else word 0 scaled onto the episode count.
__device__ __forceinline__ void pick_episode(const ReplayView& v, const uint32_t (&c)[4], int& pos) {
    if (v.cum) {
        const uint64_t u = ((uint64_t)c[2] << 32) | c[3];
        const uint64_t g = __umul64hi(u, v.cum[v.n_episodes]);
        const uint32_t k = (uint32_t)(u >> (64 - v.guide_bits));
        int lo = v.guide[k], hi = v.guide[k + 1] + 1;      // g is monotone in u: the answer lies between the buckets' first episodes
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (v.cum[mid] <= g) lo = mid; else hi = mid;
        }
        pos = lo;
    } else {
        pos = (int)(((uint64_t)c[0] * (uint64_t)v.n_episodes) >> 32);
    }
}

// The (episode position, start idx) pair of sample b, the same in every wave that asks for it: a Philox counter block (the cum / guide
// search on a weighted arena), or the pair the host sampler shipped. Lane 0 of a `writer` wave records a drawn pair in pairs_out.
__device__ __forceinline__ void draw_pair(const ReplayView& v, const int32_t* pairs_in, int32_t* pairs_out, int b, int nstep, int sampler,
                                          uint64_t seed, uint64_t counter, int lane, bool writer, int& pos, int& idx) {
    if (sampler == EXORL_SAMPLER_PHILOX) {
        uint32_t c[4] = {(uint32_t)b, (uint32_t)counter, (uint32_t)(counter >> 32), 0u};
        Philox::gen(c, seed);
        pick_episode(v, c, pos);
        const int span = v.len[pos] - nstep + 1;
        idx = (int)(((uint64_t)c[1] * (uint64_t)span) >> 32) + 1;
        if (writer && lane == 0) { pairs_out[2 * b] = pos; pairs_out[2 * b + 1] = idx; }
    } else {
        pos = pairs_in[2 * b];
        idx = pairs_in[2 * b + 1];
    }
}

// The goal (pos_g, tau) of sample b, whose own pair is (pos, idx): obs at time t = idx - 1, next_obs at t + nstep <= len[pos]. Philox: block
// (b, counter, 1) gives the source on x[0] and the offset on x[1]; CUR is next_obs itself, TRAJ a state d steps behind it in the same episode
// (uniform over what is left of it, or geometric from the table, the mass past the episode's end on its last state), RAND an episode from
// block (b, counter, 2) through pick_episode and a time uniform over its len + 1 rows. Lane 0 records the drawn goal. Other samplers: the
// goal the host shipped (range-checked there).
__device__ __forceinline__ void draw_goal(const ReplayView& v, const GoalView& g, int b, int nstep, int sampler, uint64_t seed, uint64_t counter,
                                          int lane, int pos, int idx, int& pos_g, int& tau) {
    if (sampler == EXORL_SAMPLER_PHILOX) {
        uint32_t x[4] = {(uint32_t)b, (uint32_t)counter, (uint32_t)(counter >> 32), 1u};
        Philox::gen(x, seed);
        const int tn = idx - 1 + nstep;
        pos_g = pos;
        if (x[0] < g.t_cur) {
            tau = tn;
        } else if (x[0] < g.t_traj) {
            const int room = v.len[pos] - tn;
            int d;
            if (g.n_tab) {                     // d = #{k : tab[k] <= x[1]}, capped at the episode's end
                int lo = 0, hi = g.n_tab;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (g.tab[mid] <= x[1]) lo = mid + 1; else hi = mid;
                }
                d = lo < room ? lo : room;
            } else {
                d = (int)(((uint64_t)x[1] * (uint64_t)(room + 1)) >> 32);
            }
            tau = tn + d;
        } else {
            uint32_t y[4] = {(uint32_t)b, (uint32_t)counter, (uint32_t)(counter >> 32), 2u};
            Philox::gen(y, seed);
            pick_episode(v, y, pos_g);
            tau = (int)(((uint64_t)y[1] * (uint64_t)(v.len[pos_g] + 1)) >> 32);
        }
        if (lane == 0) { g.goals[2 * b] = pos_g; g.goals[2 * b + 1] = tau; }
    } else {
        pos_g = g.goals[2 * b];
        tau = g.goals[2 * b + 1];
    }
}

// What one wave writes per sample, whatever the shape of the observation gather: the action of arena row `row` (= row0 + idx), the meta
// row of the step before it, and the n-step return and discount in the reference's operation order. fp contract is off INSIDE this body
// (the pragma is lexically scoped): an FMA in the recurrence would stop matching NumPy.
// next_ok (idx + nstep <= len[pos], the caller has both): the episode holds the action taken at next_obs, arena row `row + nstep`. Where
// it does not, that row is the next episode's dummy row or lies past the arena's end and is not read: the sample gets zeros.
// mc (null: not written): the sample's Monte-Carlo return-to-go, the column's value at `row`, a plain copy.
// RELABEL (the goal path) with a mode other than EXORL_GOAL_KEEP: the recurrence runs on "reached / not reached" inputs instead of the arena's,
// rho_i = (NEG: 0 on the reaching step, else -1; SPARSE: 1 on it, else 0), c_i = 0 on it, else 1; only step nstep - 1 can be the reaching one.
template <bool RELABEL = false>
__device__ __forceinline__ void sample_tail(const ReplayView& v, const exorl_batch_out& out, int b, int64_t row, int nstep, float gamma,
                                            int lane, bool next_ok, float* mc, int mode = EXORL_GOAL_KEEP, bool reached = false) {
#pragma clang fp contract(off)
    for (int j = lane; j < v.act_dim; j += 64) out.action[(int64_t)b * out.action_stride + j] = v.act[row * v.act_dim + j];
    if (out.next_action) {                           // wave-uniform, as next_ok is
        float* dst = out.next_action + (int64_t)b * out.next_action_stride;
        if (next_ok) {
            const float* src = v.act + (row + nstep) * v.act_dim;
            for (int j = lane; j < v.act_dim; j += 64) dst[j] = src[j];
        } else {
            for (int j = lane; j < v.act_dim; j += 64) dst[j] = 0.0f;
        }
        if (lane == 0) out.next_valid[b] = next_ok ? 1.0f : 0.0f;
    }
    if (out.meta)
        for (int j = lane; j < v.meta_dim; j += 64) out.meta[(int64_t)b * out.meta_stride + j] = v.meta[(row - 1) * v.meta_dim + j];
    if (lane == 0) {
        float R = 0.0f, D = 1.0f;
        for (int i = 0; i < nstep; ++i) {
            float rho, c;
            if (RELABEL && mode != EXORL_GOAL_KEEP) {
                const bool hit = reached && i == nstep - 1;
                rho = mode == EXORL_GOAL_NEG ? (hit ? 0.0f : -1.0f) : (hit ? 1.0f : 0.0f);
                c = hit ? 0.0f : 1.0f;
            } else {
                rho = v.rew[row + i];
                c = v.disc[row + i];
            }
            const float t = D * rho;                   // replay_buffer.py:233  reward += discount * step_reward
            R = R + t;
            const float u = c * gamma;                 // replay_buffer.py:234  discount *= ep_discount * gamma
            D = D * u;
        }
        out.reward[b] = R;
        out.discount[b] = D;
        if (mc) mc[b] = v.rtg[row];
    }
}

template <typename T>
__device__ __forceinline__ const T& only(const T& x) { return x; }

// NORM = false is the copying gather; NORM = true (exorl_replay_set_obs_norm) differs only where an observation element is written.
// Goal is empty (the kernel as it always was, argument for argument) or one GoalView: the goal path, which also draws the sample's goal,
// writes its columns behind obs and next_obs and hands sample_tail the reward mode and whether next_obs IS the goal.
template <bool NORM, typename... Goal>
__global__ __launch_bounds__(256) void gather_nstep_kernel(ReplayView v, const int32_t* pairs_in,
                                                           int32_t* pairs_out, exorl_batch_out out,
                                                           int batch, int nstep, float gamma, int sampler,
                                                           uint64_t seed, uint64_t counter_val,
                                                           const uint64_t* counter_ptr, int vec16, StageOut stage, float* mc, Goal... goal) {
#pragma clang fp contract(off)
    if (stage.st && blockIdx.x == 0 && threadIdx.x == 0) step_begin_device(stage.st, 0);   // noise counter, Adam scalars of this step
    const uint64_t counter = counter_ptr ? *counter_ptr : counter_val;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (b >= batch) return;
    int pos, idx;
    draw_pair(v, pairs_in, pairs_out, b, nstep, sampler, seed, counter, lane, true, pos, idx);
    const int64_t row = v.row0[pos] + idx;
    if constexpr (NORM) {
        norm_row(v.obs + (row - 1) * v.obs_bytes, static_cast<unsigned char*>(out.obs) + (int64_t)b * out.obs_stride,
                 v.obs_bytes, lane, vec16, v.norm_mean, v.norm_inv);
        norm_row(v.obs + (row + nstep - 1) * v.obs_bytes,
                 static_cast<unsigned char*>(out.next_obs) + (int64_t)b * out.next_obs_stride, v.obs_bytes, lane, vec16, v.norm_mean, v.norm_inv);
    } else {
        copy_row(v.obs + (row - 1) * v.obs_bytes, static_cast<unsigned char*>(out.obs) + (int64_t)b * out.obs_stride,
                 v.obs_bytes, lane, vec16);
        copy_row(v.obs + (row + nstep - 1) * v.obs_bytes,
                 static_cast<unsigned char*>(out.next_obs) + (int64_t)b * out.next_obs_stride, v.obs_bytes, lane, vec16);
    }
    if (stage.xa) {                                  // the agent's staged network inputs, straight from the arena rows
        const int O = stage.O, A = stage.A, W = O + A;
        const float* so = reinterpret_cast<const float*>(v.obs + (row - 1) * v.obs_bytes);
        const float* sn = reinterpret_cast<const float*>(v.obs + (row + nstep - 1) * v.obs_bytes);
        for (int j = lane; j < O; j += 64) {
            float o = so[j], no = sn[j];
            if constexpr (NORM) {
                const float mu = v.norm_mean[j], sc = v.norm_inv[j];
                o = (o - mu) * sc;
                no = (no - mu) * sc;
            }
            stage.xa[(int64_t)b * O + j] = no;
            stage.xa[(int64_t)(stage.B + b) * O + j] = o;
            if (stage.has_critic) {
                stage.xc_cur[(int64_t)b * W + j] = o;
                stage.xc_next[(int64_t)b * W + j] = no;
                stage.xc_pi[(int64_t)b * W + j] = o;
            }
        }
        if (stage.has_critic)
            for (int j = lane; j < A; j += 64) stage.xc_cur[(int64_t)b * W + O + j] = v.act[row * v.act_dim + j];
    }
    if constexpr (sizeof...(Goal) > 0) {
        const GoalView& gv = only(goal...);
        int pos_g, tau;
        draw_goal(v, gv, b, nstep, sampler, seed, counter, lane, pos, idx, pos_g, tau);
        const float* gs = reinterpret_cast<const float*>(v.obs + (v.row0[pos_g] + tau) * v.obs_bytes);
        for (int j = lane; j < gv.n_cols; j += 64) {
            const int c = gv.cols[j];
            float x = gs[c];
            if constexpr (NORM) x = (x - v.norm_mean[c]) * v.norm_inv[c];      // norm_row's two roundings
            gv.goal[(int64_t)b * gv.goal_stride + j] = x;
            gv.next_goal[(int64_t)b * gv.next_goal_stride + j] = x;
        }
        sample_tail<true>(v, out, b, row, nstep, gamma, lane, idx + nstep <= v.len[pos], mc, gv.reward_mode,
                          pos_g == pos && tau == idx - 1 + nstep);
    } else {
        sample_tail(v, out, b, row, nstep, gamma, lane, idx + nstep <= v.len[pos], mc);
    }
}

// copy_row with four loads of a lane in flight before the first store (the compiler keeps copy_row's loop at one load, one wait, one store):
// a frame is 21 KB at (3, 84, 84), 21 wave-wide 16-byte passes, and a wave that waits out every miss by itself leaves HBM idle.
template <typename W>
__device__ __forceinline__ void stream_words(const W* __restrict__ s, W* __restrict__ d, int n, int lane) {
    int i = lane;
    for (; i + 192 < n; i += 256) {
        const W a = s[i], b = s[i + 64], c = s[i + 128], e = s[i + 192];
        d[i] = a; d[i + 64] = b; d[i + 128] = c; d[i + 192] = e;
    }
    for (; i < n; i += 64) d[i] = s[i];
}

// Frame-stacked arenas: one wave per output frame, 2 * frames * batch of them. Wave (b, which, j) streams frame j (0 = oldest) of sample b's
// obs (which = 0, the stack at t = idx - 1) or next_obs (which = 1, t = idx + nstep - 1) from episode row max(t - (frames - 1 - j), 0): steps
// before the reset repeat the reset frame. The first wave of a sample also writes what is per sample: sample_tail and the drawn pair.
__global__ __launch_bounds__(256) void gather_frames_kernel(ReplayView v, const int32_t* pairs_in, int32_t* pairs_out, exorl_batch_out out,
                                                            int batch, int nstep, float gamma, int sampler, uint64_t seed,
                                                            uint64_t counter_val, const uint64_t* counter_ptr, int frames, float* mc) {
    const uint64_t counter = counter_ptr ? *counter_ptr : counter_val;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int b = w / (2 * frames), part = w % (2 * frames);
    if (b >= batch) return;
    const int which = part / frames, j = part % frames;
    const bool first = part == 0;
    int pos, idx;
    draw_pair(v, pairs_in, pairs_out, b, nstep, sampler, seed, counter, lane, first, pos, idx);
    const int64_t row0 = v.row0[pos];
    const int t = idx - 1 + (which ? nstep : 0);
    const int f = t - (frames - 1 - j);
    const unsigned char* src = v.obs + (row0 + (f > 0 ? f : 0)) * v.obs_bytes;
    unsigned char* dst = static_cast<unsigned char*>(which ? out.next_obs : out.obs) +
                         (int64_t)b * (which ? out.next_obs_stride : out.obs_stride) + (int64_t)j * v.obs_bytes;
    // wave-uniform; the arena rows are 16-byte aligned whenever a frame is a multiple of 16 bytes, the destination need not be
    const bool vec16 = v.obs_bytes % 16 == 0 && (reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) % 16 == 0;
    if (vec16) stream_words(reinterpret_cast<const uint4*>(src), reinterpret_cast<uint4*>(dst), v.obs_bytes / 16, lane);
    else stream_words(reinterpret_cast<const uint32_t*>(src), reinterpret_cast<uint32_t*>(dst), v.obs_bytes / 4, lane);
    if (!first) return;
    sample_tail(v, out, b, row0 + idx, nstep, gamma, lane, idx + nstep <= v.len[pos], mc);
}

// ---- column moments of the resident observations (exorl_replay_obs_moments) -----------------------------------------------------------
// (count, mean, M2 = sum (x - mean)^2) of one column over some rows, in fp64. A value is added with Welford's update, two such triples are
// merged with Chan's; neither forms sum x^2, so a column of mean 1000 and spread 0.01 keeps its M2, and a constant column keeps M2 == 0
// exactly (every delta is 0).
struct Moments {
    double n, mean, m2;
};

__device__ __forceinline__ void moments_add(Moments& a, double x) {
    a.n += 1.0;
    const double d = x - a.mean;
    a.mean += d / a.n;
    a.m2 += d * (x - a.mean);
}

__device__ __forceinline__ Moments moments_merge(const Moments& a, const Moments& b) {
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    const double n = a.n + b.n, d = b.mean - a.mean;
    return Moments{n, a.mean + d * (b.n / n), a.m2 + b.m2 + d * d * (a.n * b.n / n)};
}

constexpr int MOMENTS_CHUNK = 64;          // rows of one work item: an episode of `rows` rows is cdiv(rows, 64) items
constexpr int MOMENTS_MAX_GROUPS = 1024;   // workgroups of the first launch = partials in the slab

// Launch 1. Work item i is a run of <= 64 consecutive rows of one episode (item0[e] = the first item of the episode at table position e);
// workgroup g owns items [g * items_per_group, (g + 1) * items_per_group), a fixed assignment. The 256 threads tile rows x columns: with
// ct = min(n_cols, 256) columns per tile and rp = 256 / ct rows per pass, thread (tr, tc) keeps column cb + tc and walks rows tr, tr + rp, ...
// of every item, so a pass reads rp whole rows, contiguous in the arena. Per column tile the rp threads of a column are merged through LDS
// in a fixed tree and the workgroup stores one partial: slab = count[G] | mean[G][n_cols] | m2[G][n_cols].
__global__ __launch_bounds__(256) void obs_moments_partial_kernel(const float* __restrict__ obs, const int64_t* __restrict__ row0,
                                                                  const int32_t* __restrict__ len, const int32_t* __restrict__ item0,
                                                                  int n_episodes, int n_cols, int items_per_group, int n_items,
                                                                  double* __restrict__ slab) {
    __shared__ double s_n[256], s_mean[256], s_m2[256];
    const int g = blockIdx.x, G = gridDim.x, t = threadIdx.x;
    const int ct = n_cols < 256 ? n_cols : 256, rp = 256 / ct;
    const int tc = t % ct, tr = t / ct;
    const int i0 = g * items_per_group, i1 = min(i0 + items_per_group, n_items);
    int e0 = 0;                                   // the episode of item i0: item0[e0] <= i0 < item0[e0 + 1]
    for (int hi = n_episodes; hi - e0 > 1;) {
        const int mid = (e0 + hi) >> 1;
        if (item0[mid] <= i0) e0 = mid; else hi = mid;
    }
    for (int cb = 0; cb < n_cols; cb += ct) {
        const int j = cb + tc;
        Moments acc{0.0, 0.0, 0.0};
        if (tr < rp && j < n_cols) {
            int e = e0;
            for (int it = i0; it < i1; ++it) {
                while (item0[e + 1] <= it) ++e;
                const int r0 = (it - item0[e]) * MOMENTS_CHUNK;
                const int nr = min(len[e] + 1 - r0, MOMENTS_CHUNK);
                const float* x = obs + (row0[e] + r0) * (int64_t)n_cols + j;
                int r = tr;
                for (; r + 3 * rp < nr; r += 4 * rp) {          // four loads in flight ahead of the dependent updates
                    const float a = x[(int64_t)r * n_cols], b = x[(int64_t)(r + rp) * n_cols], c = x[(int64_t)(r + 2 * rp) * n_cols],
                                d = x[(int64_t)(r + 3 * rp) * n_cols];
                    moments_add(acc, a); moments_add(acc, b); moments_add(acc, c); moments_add(acc, d);
                }
                for (; r < nr; r += rp) moments_add(acc, x[(int64_t)r * n_cols]);
            }
        }
        s_n[t] = acc.n; s_mean[t] = acc.mean; s_m2[t] = acc.m2;
        __syncthreads();
        int half = 1;
        while (half < rp) half <<= 1;
        for (half >>= 1; half >= 1; half >>= 1) {               // row slots tr and tr + half of one column, the same pairs every run
            if (tr < half && tr + half < rp) {
                const int u = t + half * ct;
                const Moments m = moments_merge(Moments{s_n[t], s_mean[t], s_m2[t]}, Moments{s_n[u], s_mean[u], s_m2[u]});
                s_n[t] = m.n; s_mean[t] = m.mean; s_m2[t] = m.m2;
            }
            __syncthreads();
        }
        if (tr == 0 && j < n_cols) {
            if (j == 0) slab[g] = s_n[t];
            slab[G + (int64_t)g * n_cols + j] = s_mean[t];
            slab[G + (int64_t)G * n_cols + (int64_t)g * n_cols + j] = s_m2[t];
        }
        __syncthreads();
    }
}

// Launch 2. One wave per column, four columns per workgroup: lane l merges its run of cdiv(G, 64) consecutive partials in slab order, then
// neighbouring runs are merged pairwise through LDS, the earlier run on the left: the slab in slab order, as a fixed tree.
// result = count | mean[n_cols] | m2[n_cols].
__global__ __launch_bounds__(256) void obs_moments_combine_kernel(const double* __restrict__ slab, int G, int n_cols, double* __restrict__ result) {
    __shared__ double s_n[256], s_mean[256], s_m2[256];
    const int t = threadIdx.x, lane = t & 63, j = blockIdx.x * 4 + (t >> 6);
    const int run = (G + 63) / 64;
    Moments acc{0.0, 0.0, 0.0};
    if (j < n_cols)
        for (int g = lane * run; g < min((lane + 1) * run, G); ++g)
            acc = moments_merge(acc, Moments{slab[g], slab[G + (int64_t)g * n_cols + j], slab[G + (int64_t)G * n_cols + (int64_t)g * n_cols + j]});
    s_n[t] = acc.n; s_mean[t] = acc.mean; s_m2[t] = acc.m2;
    __syncthreads();
    for (int step = 1; step < 64; step <<= 1) {
        if (lane % (2 * step) == 0) {
            const Moments m = moments_merge(Moments{s_n[t], s_mean[t], s_m2[t]}, Moments{s_n[t + step], s_mean[t + step], s_m2[t + step]});
            s_n[t] = m.n; s_mean[t] = m.mean; s_m2[t] = m.m2;
        }
        __syncthreads();
    }
    if (lane == 0 && j < n_cols) {
        if (j == 0) result[0] = s_n[t];
        result[1 + j] = s_mean[t];
        result[1 + n_cols + j] = s_m2[t];
    }
}

// ---- discounted return of every resident episode (exorl_replay_episode_returns) --------------------------------------------------------
// The gather's n-step recurrence (sample_tail) from idx 1 over the whole episode, in fp64: a run of steps is the pair (R, D) = (its return
// discounted to its first step, the product of its gamma d), and two adjacent runs combine as (R1 + D1 R2, D1 D2). The operation is
// associative, not commutative: the earlier run is always the left operand. One workgroup per episode (table position blockIdx.x); thread t
// folds steps [t run + 1, (t + 1) run] sequentially, run = cdiv(len, 256), then the 256 pairs combine through LDS in a fixed tree, neighbours
// first. A thread past the end holds the identity (0, 1). Reads rows row0 + 1 .. row0 + len of the episode only.
__global__ __launch_bounds__(256) void episode_returns_kernel(const float* __restrict__ rew, const float* __restrict__ disc,
                                                              const int64_t* __restrict__ row0, const int32_t* __restrict__ len, double gamma,
                                                              double* __restrict__ out) {
    __shared__ double s_r[256], s_d[256];
    const int e = blockIdx.x, t = threadIdx.x;
    const int n = len[e];
    const int64_t base = row0[e];
    const int run = (n + 255) / 256;
    const int t0 = t * run + 1, t1 = min(t0 + run - 1, n);
    double R = 0.0, D = 1.0;
    for (int i = t0; i <= t1; ++i) {
        R += D * (double)rew[base + i];
        D *= gamma * (double)disc[base + i];
    }
    s_r[t] = R; s_d[t] = D;
    __syncthreads();
    for (int step = 1; step < 256; step <<= 1) {
        if (t % (2 * step) == 0) {
            s_r[t] = s_r[t] + s_d[t] * s_r[t + step];
            s_d[t] = s_d[t] * s_d[t + step];
        }
        __syncthreads();
    }
    if (t == 0) out[e] = s_r[0];
}

// ---- return-to-go of every resident transition (exorl_replay_build_returns) ------------------------------------------------------------
// episode_returns_kernel's recurrence carried to the episode's end and kept per step: G_len = r_len, G_i = r_i + (gamma d_i) G_{i+1}, in fp64,
// stored as float (round to nearest) at arena row row0 + i; the dummy row gets 0. An episode cut by a time limit (d = 1 on its last step) gets
// the return of its recorded remainder and no bootstrap: a lower bound on the true return only where rewards are >= 0.
// One workgroup per episode of the order table. Thread t folds its run of cdiv(len, 256) steps backwards into the pair (R, D) of
// episode_returns_kernel (a step is the pair (r_i, gamma d_i), the earlier run the left operand of (R1 + D1 R2, D1 D2)); the 256 pairs go
// through an inclusive suffix scan in LDS, 8 rounds of doubling distance, every round reading before any thread writes; a thread past the end
// holds the identity (0, 1). The return behind thread t's run is the R of thread t + 1's suffix; from it the thread walks its run backwards a
// second time and stores. No atomics, nothing read but rew and disc of rows row0 + 1 .. row0 + len: an episode's bits depend on nothing else.
__global__ __launch_bounds__(256) void returns_to_go_kernel(const float* __restrict__ rew, const float* __restrict__ disc,
                                                            const int64_t* __restrict__ row0, const int32_t* __restrict__ len, double gamma,
                                                            float* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double s_r[256], s_d[256];
    const int e = blockIdx.x, t = threadIdx.x;
    const int n = len[e];
    const int64_t base = row0[e];
    const int run = (n + 255) / 256;
    const int t0 = t * run + 1, t1 = min(t0 + run - 1, n);
    double R = 0.0, D = 1.0;
    for (int i = t1; i >= t0; --i) {
        const double c = gamma * (double)disc[base + i];
        R = (double)rew[base + i] + c * R;
        D = c * D;
    }
    s_r[t] = R; s_d[t] = D;
    __syncthreads();
    for (int step = 1; step < 256; step <<= 1) {
        const bool has = t + step < 256;
        const double r2 = has ? s_r[t + step] : 0.0, d2 = has ? s_d[t + step] : 1.0;
        __syncthreads();
        if (has) {
            R = R + D * r2;
            D = D * d2;
            s_r[t] = R; s_d[t] = D;
        }
        __syncthreads();
    }
    double G = t + 1 < 256 ? s_r[t + 1] : 0.0;
    for (int i = t1; i >= t0; --i) {
        G = (double)rew[base + i] + (gamma * (double)disc[base + i]) * G;
        out[base + i] = (float)G;
    }
    if (t == 0) out[base] = 0.0f;
}

// Prefix sum of the episode masses for `nstep`, checked on the host before anything is enqueued.
static int build_cum(exorl_replay* r, int32_t nstep) {
    const int n = (int)r->order.size();
    r->h_cum.resize((size_t)n + 1);
    uint64_t total = 0;
    r->h_cum[0] = 0;
    for (int i = 0; i < n; ++i) {
        const int slot = r->order[i];
        const int64_t span = std::max<int64_t>((int64_t)r->slots[slot].rows - 1 - nstep + 1, 0);
        const uint64_t q = r->weight[slot];
        const uint64_t mass = r->weight_mode == EXORL_WEIGHT_TRANSITIONS ? q * (uint64_t)span : (span > 0 ? q : 0);   // < 2^32 * 2^31
        EXORL_REQUIRE(mass < (1ull << 63) - total, "replay_sample: total sampling mass reaches 2^63 at position %d of %d: use smaller "
                      "weights", i, n);
        total += mass;
        r->h_cum[i + 1] = total;
    }
    EXORL_REQUIRE(total > 0, "replay_sample: total sampling mass is 0: no episode with a positive weight holds nstep=%d transitions", nstep);
    int bits = 1;
    while ((1 << bits) < 2 * n && (2 << bits) <= r->guide_cap) ++bits;
    const int G = 1 << bits;
    r->guide_bits = bits;
    r->h_guide.resize((size_t)G + 1);
    int p = 0;
    for (int k = 0; k <= G; ++k) {       // bucket k starts at u = k << (64 - bits); entry G: the last drawable g
        const uint64_t g = k < G ? (uint64_t)(((unsigned __int128)((uint64_t)k << (64 - bits)) * total) >> 64) : total - 1;
        while (r->h_cum[p + 1] <= g) ++p;
        r->h_guide[k] = p;
    }
    return 0;
}

// nstep: the Philox sampler's (the cum table depends on it); 0 for the host-side samplers, which read no cum table.
static int upload_table(exorl_replay* r, int32_t nstep, hipStream_t s) {
    const bool want_cum = r->weighted && nstep > 0;
    if (want_cum && (r->table_dirty || r->cum_nstep != nstep)) {
        r->cum_nstep = -1;
        EXORL_TRY(build_cum(r, nstep));
        EXORL_CHECK_HIP(hipMemcpyAsync(r->d_cum, r->h_cum.data(), r->h_cum.size() * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        EXORL_CHECK_HIP(hipMemcpyAsync(r->d_guide, r->h_guide.data(), r->h_guide.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        r->cum_nstep = nstep;
    }
    if (!r->table_dirty) return 0;
    if (!want_cum) r->cum_nstep = -1;      // the table moved under a cum built earlier
    const int n = (int)r->order.size();
    r->h_row0.resize(n);
    r->h_len.resize(n);
    int32_t mn = INT32_MAX;
    for (int i = 0; i < n; ++i) {
        const Slot& sl = r->slots[r->order[i]];
        r->h_row0[i] = sl.row0;
        r->h_len[i] = sl.rows - 1;
        mn = sl.rows - 1 < mn ? sl.rows - 1 : mn;
    }
    r->min_len = n ? mn : 0;
    if (n) {
        EXORL_CHECK_HIP(hipMemcpyAsync(r->d_row0, r->h_row0.data(), n * sizeof(int64_t), hipMemcpyHostToDevice, s));
        EXORL_CHECK_HIP(hipMemcpyAsync(r->d_len, r->h_len.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, s));
        // pageable sources: the runtime stages them before returning, so the vectors may be reused
    }
    r->table_dirty = false;
    return 0;
}

// Moves live episodes down over evicted holes (bounce buffer handles overlapping ranges).
static int compact(exorl_replay* r) {
    EXORL_CHECK_HIP(hipDeviceSynchronize());
    std::vector<int> live;
    for (int i = 0; i < (int)r->slots.size(); ++i)
        if (r->slots[i].live) live.push_back(i);
    std::sort(live.begin(), live.end(), [&](int a, int b) { return r->slots[a].row0 < r->slots[b].row0; });
    const int64_t chunk_rows_cap = 4096;
    const int64_t widest = std::max<int64_t>(r->cfg.obs_bytes, std::max<int64_t>(r->cfg.act_dim, r->cfg.meta_dim) * 4);
    void* tmp = nullptr;
    EXORL_CHECK_HIP(hipMalloc(&tmp, chunk_rows_cap * std::max<int64_t>(widest, 4)));
    int64_t dst = 0;
    auto move = [&](unsigned char* base, int64_t rowbytes, int64_t from, int64_t to, int64_t rows) -> int {
        if (!base || rowbytes == 0 || from == to) return 0;
        for (int64_t done = 0; done < rows; done += chunk_rows_cap) {
            const int64_t n = std::min(chunk_rows_cap, rows - done);
            EXORL_CHECK_HIP(hipMemcpy(tmp, base + (from + done) * rowbytes, n * rowbytes, hipMemcpyDeviceToDevice));
            EXORL_CHECK_HIP(hipMemcpy(base + (to + done) * rowbytes, tmp, n * rowbytes, hipMemcpyDeviceToDevice));
        }
        return 0;
    };
    for (int i : live) {
        Slot& sl = r->slots[i];
        EXORL_TRY(move(r->obs, r->cfg.obs_bytes, sl.row0, dst, sl.rows));
        EXORL_TRY(move((unsigned char*)r->act, r->cfg.act_dim * 4, sl.row0, dst, sl.rows));
        EXORL_TRY(move((unsigned char*)r->rew, 4, sl.row0, dst, sl.rows));
        EXORL_TRY(move((unsigned char*)r->disc, 4, sl.row0, dst, sl.rows));
        EXORL_TRY(move((unsigned char*)r->meta, r->cfg.meta_dim * 4, sl.row0, dst, sl.rows));
        sl.row0 = dst;
        dst += sl.rows;
    }
    EXORL_CHECK_HIP(hipFree(tmp));
    r->used_rows = dst;
    r->table_dirty = true;
    return 0;
}

}  // namespace exorl

extern "C" {

int exorl_replay_create(const exorl_replay_cfg* cfg, exorl_replay_t** out) {
    EXORL_REQUIRE(cfg && out, "replay_create: null argument");
    EXORL_REQUIRE(cfg->obs_bytes > 0 && cfg->obs_bytes % 4 == 0, "replay_create: obs_bytes=%d must be a positive multiple of 4",
                  cfg->obs_bytes);
    EXORL_REQUIRE(cfg->act_dim > 0 && cfg->meta_dim >= 0 && cfg->capacity_rows > 0 && cfg->max_episodes > 0,
                  "replay_create: bad dims");
    auto* r = new exorl_replay();
    r->cfg = *cfg;
    const int64_t rows = cfg->capacity_rows;
    EXORL_CHECK_HIP(hipMalloc((void**)&r->obs, rows * cfg->obs_bytes));
    EXORL_CHECK_HIP(hipMalloc((void**)&r->act, rows * cfg->act_dim * 4));
    EXORL_CHECK_HIP(hipMalloc((void**)&r->rew, rows * 4));
    EXORL_CHECK_HIP(hipMalloc((void**)&r->disc, rows * 4));
    if (cfg->meta_dim) EXORL_CHECK_HIP(hipMalloc((void**)&r->meta, rows * cfg->meta_dim * 4));
    EXORL_CHECK_HIP(hipMalloc((void**)&r->d_row0, (size_t)cfg->max_episodes * sizeof(int64_t)));
    EXORL_CHECK_HIP(hipMalloc((void**)&r->d_len, (size_t)cfg->max_episodes * sizeof(int32_t)));
    EXORL_CHECK_HIP(hipMalloc((void**)&r->d_cum, ((size_t)cfg->max_episodes + 1) * sizeof(uint64_t)));
    r->guide_cap = 2;
    while (r->guide_cap < 2 * (int64_t)cfg->max_episodes && r->guide_cap < (1 << 28)) r->guide_cap <<= 1;
    EXORL_CHECK_HIP(hipMalloc((void**)&r->d_guide, ((size_t)r->guide_cap + 1) * sizeof(int32_t)));
    EXORL_CHECK_HIP(hipMalloc((void**)&r->d_norm, 2 * (size_t)(cfg->obs_bytes / 4) * sizeof(float)));
    *out = r;
    return 0;
}

int exorl_replay_destroy(exorl_replay_t* r) {
    if (!r) return 0;
    (void)hipFree(r->obs); (void)hipFree(r->act); (void)hipFree(r->rew); (void)hipFree(r->disc);
    if (r->meta) (void)hipFree(r->meta);
    (void)hipFree(r->d_row0); (void)hipFree(r->d_len); (void)hipFree(r->d_cum); (void)hipFree(r->d_guide);
    if (r->d_pairs) (void)hipFree(r->d_pairs);
    (void)hipFree(r->d_norm);
    if (r->d_item0) (void)hipFree(r->d_item0);
    if (r->d_slab) (void)hipFree(r->d_slab);
    if (r->d_returns) (void)hipFree(r->d_returns);
    if (r->d_rtg) (void)hipFree(r->d_rtg);
    if (r->d_goal_cols) (void)hipFree(r->d_goal_cols);
    if (r->d_goal_tab) (void)hipFree(r->d_goal_tab);
    if (r->d_goals) (void)hipFree(r->d_goals);
    if (r->d_keys) (void)hipFree(r->d_keys);
    if (r->d_kitem0) (void)hipFree(r->d_kitem0);
    if (r->d_ktrans0) (void)hipFree(r->d_ktrans0);
    delete r;
    return 0;
}

int exorl_replay_append_episode(exorl_replay_t* r, const void* obs, const float* act, const float* rew,
                                const float* disc, const float* meta, int32_t rows, int32_t* slot_out) {
    EXORL_REQUIRE(r && obs && act && rew && disc && slot_out, "replay_append_episode: null argument");
    EXORL_REQUIRE(rows >= 2, "replay_append_episode: rows=%d (an episode is a dummy row + >=1 transition)", rows);
    EXORL_REQUIRE((r->cfg.meta_dim == 0) == (meta == nullptr), "replay_append_episode: meta pointer/meta_dim mismatch");
    r->keys_stale();
    r->returns_stale();
    if (r->used_rows + rows > r->cfg.capacity_rows) {
        EXORL_REQUIRE(r->live_rows + rows <= r->cfg.capacity_rows,
                      "replay_append_episode: arena full (%lld live + %d > capacity %lld rows)", (long long)r->live_rows, rows,
                      (long long)r->cfg.capacity_rows);
        EXORL_TRY(compact(r));
    }
    int slot = -1;
    for (int i = 0; i < (int)r->slots.size(); ++i)
        if (!r->slots[i].live) { slot = i; break; }
    if (slot < 0) {
        EXORL_REQUIRE((int)r->slots.size() < r->cfg.max_episodes, "replay_append_episode: more than max_episodes=%d resident",
                      r->cfg.max_episodes);
        r->slots.push_back(Slot{0, 0, false});
        r->weight.push_back(1u);
        slot = (int)r->slots.size() - 1;
    }
    const int64_t row0 = r->used_rows;
    EXORL_CHECK_HIP(hipMemcpy(r->obs + row0 * r->cfg.obs_bytes, obs, (size_t)rows * r->cfg.obs_bytes, hipMemcpyHostToDevice));
    EXORL_CHECK_HIP(hipMemcpy(r->act + row0 * r->cfg.act_dim, act, (size_t)rows * r->cfg.act_dim * 4, hipMemcpyHostToDevice));
    EXORL_CHECK_HIP(hipMemcpy(r->rew + row0, rew, (size_t)rows * 4, hipMemcpyHostToDevice));
    EXORL_CHECK_HIP(hipMemcpy(r->disc + row0, disc, (size_t)rows * 4, hipMemcpyHostToDevice));
    if (meta) EXORL_CHECK_HIP(hipMemcpy(r->meta + row0 * r->cfg.meta_dim, meta, (size_t)rows * r->cfg.meta_dim * 4, hipMemcpyHostToDevice));
    r->slots[slot] = Slot{row0, rows, true};
    r->weight[slot] = 1u;                           // a reused slot does not inherit the evicted episode's weight
    r->used_rows += rows;
    r->live_rows += rows;
    *slot_out = slot;
    return 0;
}

int exorl_replay_evict(exorl_replay_t* r, int32_t slot) {
    EXORL_REQUIRE(r && slot >= 0 && slot < (int)r->slots.size() && r->slots[slot].live, "replay_evict: slot %d not resident", slot);
    r->keys_stale();
    r->returns_stale();
    r->slots[slot].live = false;
    r->live_rows -= r->slots[slot].rows;
    for (size_t i = 0; i < r->order.size(); ++i)
        if (r->order[i] == slot) { r->order.erase(r->order.begin() + i); break; }
    r->table_dirty = true;
    return 0;
}

int exorl_replay_set_order(exorl_replay_t* r, const int32_t* slots, int32_t n) {
    EXORL_REQUIRE(r && (slots || n == 0) && n >= 0 && n <= r->cfg.max_episodes, "replay_set_order: bad arguments");
    for (int i = 0; i < n; ++i)
        EXORL_REQUIRE(slots[i] >= 0 && slots[i] < (int)r->slots.size() && r->slots[slots[i]].live,
                      "replay_set_order: slot %d (position %d) not resident", slots[i], i);
    r->keys_stale();
    r->returns_stale();
    r->order.assign(slots, slots + n);
    r->table_dirty = true;
    return 0;
}

int exorl_replay_set_weights(exorl_replay_t* r, int32_t mode, const uint32_t* q_per_slot, int32_t n_slots) {
    EXORL_REQUIRE(r, "replay_set_weights: null handle");
    EXORL_REQUIRE(mode == EXORL_WEIGHT_EPISODES || mode == EXORL_WEIGHT_TRANSITIONS, "replay_set_weights: unknown mode %d", mode);
    EXORL_REQUIRE(!q_per_slot || (n_slots >= 0 && n_slots <= (int)r->slots.size()),
                  "replay_set_weights: %d weights for %d slots", n_slots, (int)r->slots.size());
    for (size_t i = 0; i < r->weight.size(); ++i) r->weight[i] = q_per_slot && (int)i < n_slots ? q_per_slot[i] : 1u;
    r->weight_mode = mode;
    r->weighted = q_per_slot != nullptr || mode == EXORL_WEIGHT_TRANSITIONS;
    r->cum_nstep = -1;
    r->weights_epoch += 1;
    return 0;
}

int exorl_replay_set_frame_stack(exorl_replay_t* r, int32_t frames) {
    EXORL_REQUIRE(r, "replay_set_frame_stack: null handle");
    EXORL_REQUIRE(frames >= 1 && frames <= 16, "replay_set_frame_stack: frames=%d outside [1, 16]", frames);
    EXORL_REQUIRE(r->slots.empty(), "replay_set_frame_stack: the arena has handed out %d slots already: rows stored as whole observations "
                  "cannot be re-read as single frames", (int)r->slots.size());
    EXORL_REQUIRE((int64_t)frames * r->cfg.obs_bytes <= INT32_MAX, "replay_set_frame_stack: %d frames of %d bytes overflow an observation's "
                  "32-bit size", frames, r->cfg.obs_bytes);
    EXORL_REQUIRE(frames == 1 || !r->norm_on, "replay_set_frame_stack: the arena has an observation normaliser (exorl_replay_set_obs_norm), which "
                  "reads a row as one fp32 observation");
    r->frames = frames;
    return 0;
}

int exorl_replay_obs_moments(exorl_replay_t* r, int32_t n_cols, int64_t* count_host, double* mean_host, double* m2_host, void* stream) {
    EXORL_REQUIRE(r && count_host && mean_host && m2_host, "replay_obs_moments: null argument");
    EXORL_REQUIRE(r->frames == 1, "replay_obs_moments: the arena stacks %d frames per observation (exorl_replay_set_frame_stack): column moments "
                  "are defined for fp32 state rows", r->frames);
    EXORL_REQUIRE(n_cols > 0 && (int64_t)n_cols * 4 == r->cfg.obs_bytes, "replay_obs_moments: n_cols=%d fp32 columns do not fill a row of %d bytes",
                  n_cols, r->cfg.obs_bytes);
    EXORL_REQUIRE(!r->order.empty(), "replay_obs_moments: no resident episode in the order table");
    hipStream_t s = as_stream(stream);
    const int n = (int)r->order.size();
    r->h_item0.resize((size_t)n + 1);
    int64_t items = 0, rows = 0;
    for (int i = 0; i < n; ++i) {
        r->h_item0[i] = (int32_t)items;
        items += cdiv(r->slots[r->order[i]].rows, MOMENTS_CHUNK);
        rows += r->slots[r->order[i]].rows;
        EXORL_REQUIRE(items < INT32_MAX, "replay_obs_moments: more than 2^31 work items of %d rows", MOMENTS_CHUNK);
    }
    r->h_item0[n] = (int32_t)items;
    const size_t res = 1 + 2 * (size_t)n_cols, slab = MOMENTS_MAX_GROUPS * res;
    if (!r->d_item0) EXORL_CHECK_HIP(hipMalloc((void**)&r->d_item0, ((size_t)r->cfg.max_episodes + 1) * sizeof(int32_t)));
    if (!r->d_slab) EXORL_CHECK_HIP(hipMalloc((void**)&r->d_slab, (slab + res) * sizeof(double)));
    EXORL_TRY(upload_table(r, 0, s));
    EXORL_CHECK_HIP(hipMemcpyAsync(r->d_item0, r->h_item0.data(), ((size_t)n + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
    const int per = (int)cdiv(items, (int64_t)MOMENTS_MAX_GROUPS), G = (int)cdiv(items, (int64_t)per);      // no workgroup without an item
    hipLaunchKernelGGL(obs_moments_partial_kernel, dim3(G), dim3(256), 0, s, reinterpret_cast<const float*>(r->obs), r->d_row0, r->d_len,
                       r->d_item0, n, n_cols, per, (int)items, r->d_slab);
    EXORL_LAUNCH_CHECK();
    hipLaunchKernelGGL(obs_moments_combine_kernel, dim3(cdiv(n_cols, 4)), dim3(256), 0, s, r->d_slab, G, n_cols, r->d_slab + slab);
    EXORL_LAUNCH_CHECK();
    r->h_moments.resize(res);
    EXORL_CHECK_HIP(hipMemcpyAsync(r->h_moments.data(), r->d_slab + slab, res * sizeof(double), hipMemcpyDeviceToHost, s));
    EXORL_CHECK_HIP(hipStreamSynchronize(s));
    EXORL_REQUIRE((int64_t)r->h_moments[0] == rows, "replay_obs_moments: the kernels counted %lld rows, the table holds %lld",
                  (long long)r->h_moments[0], (long long)rows);
    *count_host = rows;
    memcpy(mean_host, r->h_moments.data() + 1, (size_t)n_cols * sizeof(double));
    memcpy(m2_host, r->h_moments.data() + 1 + n_cols, (size_t)n_cols * sizeof(double));
    return 0;
}

int exorl_replay_episode_returns(exorl_replay_t* r, float gamma, double* returns_host, int32_t n, void* stream) {
    EXORL_REQUIRE(r && returns_host, "replay_episode_returns: null argument");
    EXORL_REQUIRE(!r->order.empty(), "replay_episode_returns: no resident episode in the order table");
    EXORL_REQUIRE(n == (int)r->order.size(), "replay_episode_returns: n=%d, the order table holds %d episodes", n, (int)r->order.size());
    hipStream_t s = as_stream(stream);
    if (!r->d_returns) EXORL_CHECK_HIP(hipMalloc((void**)&r->d_returns, (size_t)r->cfg.max_episodes * sizeof(double)));
    EXORL_TRY(upload_table(r, 0, s));
    hipLaunchKernelGGL(episode_returns_kernel, dim3(n), dim3(256), 0, s, r->rew, r->disc, r->d_row0, r->d_len, (double)gamma, r->d_returns);
    EXORL_LAUNCH_CHECK();
    EXORL_CHECK_HIP(hipMemcpyAsync(returns_host, r->d_returns, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    EXORL_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}

int exorl_replay_build_returns(exorl_replay_t* r, float gamma, void* stream) {
    EXORL_REQUIRE(r, "replay_build_returns: null handle");
    EXORL_REQUIRE(!r->order.empty(), "replay_build_returns: no resident episode in the order table");
    hipStream_t s = as_stream(stream);
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    EXORL_CHECK_HIP(hipStreamIsCapturing(s, &cs));
    EXORL_REQUIRE(cs == hipStreamCaptureStatusNone, "replay_build_returns: a set-up call (it allocates and synchronises): not inside a capture");
    r->returns_stale();
    if (!r->d_rtg) {
        EXORL_CHECK_HIP(hipMalloc((void**)&r->d_rtg, (size_t)r->cfg.capacity_rows * sizeof(float)));
        EXORL_CHECK_HIP(hipMemsetAsync(r->d_rtg, 0, (size_t)r->cfg.capacity_rows * sizeof(float), s));
    }
    EXORL_TRY(upload_table(r, 0, s));
    hipLaunchKernelGGL(returns_to_go_kernel, dim3((int)r->order.size()), dim3(256), 0, s, r->rew, r->disc, r->d_row0, r->d_len, (double)gamma,
                       r->d_rtg);
    EXORL_LAUNCH_CHECK();
    EXORL_CHECK_HIP(hipStreamSynchronize(s));
    r->rtg_gamma = gamma;
    r->rtg_valid = true;
    r->rtg_epoch += 1;
    return 0;
}

int exorl_replay_returns(exorl_replay_t* r, float** ptr_dev, float* gamma, uint64_t* epoch, int32_t* valid) {
    EXORL_REQUIRE(r, "replay_returns: null handle");
    if (ptr_dev) *ptr_dev = r->d_rtg;
    if (gamma) *gamma = r->rtg_gamma;
    if (epoch) *epoch = r->rtg_epoch;
    if (valid) *valid = r->rtg_valid ? 1 : 0;
    return 0;
}

int exorl_replay_returns_read(exorl_replay_t* r, float* dst_host, int64_t n, void* stream) {
    EXORL_REQUIRE(r && dst_host, "replay_returns_read: null argument");
    EXORL_REQUIRE(r->rtg_valid, "replay_returns_read: no return-to-go column, or a stale one: an episode was appended or evicted or the order was "
                  "set since exorl_replay_build_returns (call it again)");
    int64_t total = 0;
    for (int slot : r->order) total += r->slots[slot].rows - 1;
    EXORL_REQUIRE(n == total, "replay_returns_read: n=%lld, the order table holds %lld transitions", (long long)n, (long long)total);
    hipStream_t s = as_stream(stream);
    r->h_rtg.resize((size_t)r->used_rows);
    EXORL_CHECK_HIP(hipMemcpyAsync(r->h_rtg.data(), r->d_rtg, (size_t)r->used_rows * sizeof(float), hipMemcpyDeviceToHost, s));
    EXORL_CHECK_HIP(hipStreamSynchronize(s));
    for (int slot : r->order) {
        const Slot& sl = r->slots[slot];
        memcpy(dst_host, r->h_rtg.data() + sl.row0 + 1, (size_t)(sl.rows - 1) * sizeof(float));
        dst_host += sl.rows - 1;
    }
    return 0;
}

int exorl_replay_set_obs_norm(exorl_replay_t* r, int32_t n_cols, const float* mean_host, const float* inv_scale_host, void* stream) {
    EXORL_REQUIRE(r, "replay_set_obs_norm: null handle");
    r->keys_stale();
    if (n_cols == 0) {
        r->norm_on = false;
        return 0;
    }
    EXORL_REQUIRE(mean_host && inv_scale_host, "replay_set_obs_norm: null argument");
    EXORL_REQUIRE(r->frames == 1, "replay_set_obs_norm: the arena stacks %d frames per observation (exorl_replay_set_frame_stack): only fp32 "
                  "state rows are normalised", r->frames);
    EXORL_REQUIRE(n_cols > 0 && (int64_t)n_cols * 4 == r->cfg.obs_bytes, "replay_set_obs_norm: n_cols=%d fp32 columns do not fill a row of %d bytes",
                  n_cols, r->cfg.obs_bytes);
    r->h_norm.resize(2 * (size_t)n_cols);
    memcpy(r->h_norm.data(), mean_host, (size_t)n_cols * sizeof(float));
    memcpy(r->h_norm.data() + n_cols, inv_scale_host, (size_t)n_cols * sizeof(float));
    // a pageable source: the runtime stages it before returning, so the vector may be rewritten by the next call
    EXORL_CHECK_HIP(hipMemcpyAsync(r->d_norm, r->h_norm.data(), r->h_norm.size() * sizeof(float), hipMemcpyHostToDevice, as_stream(stream)));
    r->norm_on = true;
    return 0;
}

int exorl_replay_set_goal(exorl_replay_t* r, const int32_t* cols_host, int32_t n_cols, double p_cur, double p_traj, double p_rand,
                          double horizon_gamma, int32_t reward_mode) {
    EXORL_REQUIRE(r, "replay_set_goal: null handle");
    if (n_cols == 0) {
        r->goal_n = 0;
        r->goal_epoch += 1;
        return 0;
    }
    const int O = r->cfg.obs_bytes / 4;
    EXORL_REQUIRE(r->frames == 1, "replay_set_goal: the arena stacks %d frames per observation (exorl_replay_set_frame_stack): goals are columns "
                  "of fp32 state rows", r->frames);
    EXORL_REQUIRE(r->cfg.meta_dim == 0, "replay_set_goal: the arena has %d meta columns: the goal takes the place behind the observation that "
                  "[obs | meta] rows give them", r->cfg.meta_dim);
    EXORL_REQUIRE(cols_host && n_cols >= 1 && n_cols <= O, "replay_set_goal: n_cols=%d goal columns of %d fp32 observation columns", n_cols, O);
    for (int j = 0; j < n_cols; ++j)
        EXORL_REQUIRE(cols_host[j] >= 0 && cols_host[j] < O, "replay_set_goal: cols[%d]=%d outside [0, %d)", j, cols_host[j], O);
    EXORL_REQUIRE(p_cur >= 0.0 && p_traj >= 0.0 && p_rand >= 0.0 && fabs(p_cur + p_traj + p_rand - 1.0) <= 1e-6,
                  "replay_set_goal: p_cur=%g p_traj=%g p_rand=%g must be non-negative and sum to 1", p_cur, p_traj, p_rand);
    EXORL_REQUIRE(horizon_gamma < 1.0, "replay_set_goal: horizon_gamma=%g must be below 1 (<= 0: the uniform horizon)", horizon_gamma);
    EXORL_REQUIRE(reward_mode == EXORL_GOAL_KEEP || reward_mode == EXORL_GOAL_NEG || reward_mode == EXORL_GOAL_SPARSE,
                  "replay_set_goal: unknown reward_mode %d", reward_mode);
    // tab[k] = floor(2^32 (1 - gamma_h^(k+1))), the power by repeated multiplication in double (no libm: a reference restates it to the bit);
    // cut at the first entry >= 2^32 - 1, which is left out, or at GOAL_TAB_MAX entries
    std::vector<uint32_t> tab;
    if (horizon_gamma > 0.0) {
        double p = horizon_gamma;
        for (int k = 0; k < GOAL_TAB_MAX; ++k, p *= horizon_gamma) {
            const double e = floor(4294967296.0 * (1.0 - p));
            if (e >= 4294967295.0) break;
            tab.push_back((uint32_t)e);
        }
    }
    EXORL_CHECK_HIP(hipDeviceSynchronize());      // a gather enqueued earlier may still read the columns and the table that are replaced
    if (!r->d_goal_cols) EXORL_CHECK_HIP(hipMalloc((void**)&r->d_goal_cols, (size_t)O * sizeof(int32_t)));
    if (!r->d_goal_tab) EXORL_CHECK_HIP(hipMalloc((void**)&r->d_goal_tab, (size_t)GOAL_TAB_MAX * sizeof(uint32_t)));
    EXORL_CHECK_HIP(hipMemcpy(r->d_goal_cols, cols_host, (size_t)n_cols * sizeof(int32_t), hipMemcpyHostToDevice));
    if (!tab.empty()) EXORL_CHECK_HIP(hipMemcpy(r->d_goal_tab, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    r->goal_n = n_cols;
    r->goal_tab_n = (int32_t)tab.size();
    r->goal_t_cur = (uint64_t)floor(p_cur * 4294967296.0);
    r->goal_t_traj = (uint64_t)floor((p_cur + p_traj) * 4294967296.0);
    r->goal_mode = reward_mode;
    r->goal_epoch += 1;
    return 0;
}

int exorl_replay_build_keys(exorl_replay_t* r, float beta, int32_t key_every, void* stream) {
    EXORL_REQUIRE(r, "replay_build_keys: null handle");
    EXORL_REQUIRE(beta >= 0.f && key_every >= 1, "replay_build_keys: needs beta >= 0 and key_every >= 1 (got %g, %d)", beta, key_every);
    EXORL_REQUIRE(r->frames == 1, "replay_build_keys: the arena stacks %d frames per observation (exorl_replay_set_frame_stack): keys are built "
                  "from fp32 state rows", r->frames);
    EXORL_REQUIRE(!r->order.empty(), "replay_build_keys: no resident episode in the order table");
    hipStream_t s = as_stream(stream);
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    EXORL_CHECK_HIP(hipStreamIsCapturing(s, &cs));
    EXORL_REQUIRE(cs == hipStreamCaptureStatusNone, "replay_build_keys: a set-up call (it allocates and synchronises): not inside a capture");
    const int n = (int)r->order.size(), O = r->cfg.obs_bytes / 4, A = r->cfg.act_dim;
    const int pitch = (int)round_up(O + A, 4);
    EXORL_REQUIRE(O + A <= NN_MAX_DIM, "replay_build_keys: %d observation + %d action columns (max %d)", O, A, NN_MAX_DIM);
    r->h_kitem0.resize((size_t)n + 1);
    r->h_ktrans0.resize((size_t)n + 1);
    int64_t items = 0, trans = 0;
    for (int i = 0; i < n; ++i) {
        const int len = r->slots[r->order[i]].rows - 1;
        r->h_kitem0[i] = (int32_t)items;
        r->h_ktrans0[i] = trans;
        items += cdiv(len, 64);
        trans += len;
        EXORL_REQUIRE(items < INT32_MAX, "replay_build_keys: more than 2^31 work items of 64 transitions");
    }
    r->h_kitem0[n] = (int32_t)items;
    r->h_ktrans0[n] = trans;
    const int64_t rows = (trans + key_every - 1) / key_every;
    EXORL_REQUIRE(rows < INT32_MAX - 64, "replay_build_keys: %lld key rows (the search indexes them with 32 bits)", (long long)rows);
    r->keys_stale();
    EXORL_CHECK_HIP(hipDeviceSynchronize());      // a search enqueued earlier may still read the table that is replaced
    const size_t need = (size_t)rows * pitch;
    if (need > r->keys_cap) {
        if (r->d_keys) EXORL_CHECK_HIP(hipFree(r->d_keys));
        r->d_keys = nullptr; r->keys_cap = 0;
        EXORL_CHECK_HIP(hipMalloc((void**)&r->d_keys, need * sizeof(float)));
        r->keys_cap = need;
    }
    if (!r->d_kitem0) EXORL_CHECK_HIP(hipMalloc((void**)&r->d_kitem0, ((size_t)r->cfg.max_episodes + 1) * sizeof(int32_t)));
    if (!r->d_ktrans0) EXORL_CHECK_HIP(hipMalloc((void**)&r->d_ktrans0, ((size_t)r->cfg.max_episodes + 1) * sizeof(int64_t)));
    EXORL_TRY(upload_table(r, 0, s));
    EXORL_CHECK_HIP(hipMemcpyAsync(r->d_kitem0, r->h_kitem0.data(), ((size_t)n + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
    EXORL_CHECK_HIP(hipMemcpyAsync(r->d_ktrans0, r->h_ktrans0.data(), ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    NnKeyBuild b{reinterpret_cast<const float*>(r->obs), r->act, r->d_row0, r->d_len, r->d_kitem0, r->d_ktrans0, n, (int)items, O, A, pitch,
                 r->norm_on ? r->d_norm : nullptr, r->norm_on ? r->d_norm + O : nullptr, beta, key_every, r->d_keys};
    EXORL_TRY(nn_build_keys(b, s));
    EXORL_CHECK_HIP(hipStreamSynchronize(s));
    r->keys_n = rows; r->keys_beta = beta; r->keys_every = key_every;
    r->keys_valid = true;
    r->keys_epoch += 1;
    return 0;
}

int exorl_replay_keys(exorl_replay_t* r, void** ptr_dev, int64_t* n, int32_t* pitch, uint64_t* epoch) {
    EXORL_REQUIRE(r && ptr_dev && n && pitch && epoch, "replay_keys: null argument");
    EXORL_REQUIRE(r->keys_valid, "replay_keys: no key table, or a stale one: the arena, its order or its normaliser changed since "
                  "exorl_replay_build_keys (call it again)");
    const ReplayKeys k = replay_keys(r);
    *ptr_dev = const_cast<float*>(k.ptr); *n = k.n; *pitch = k.pitch; *epoch = k.epoch;
    return 0;
}

int exorl_replay_keys_read(exorl_replay_t* r, void* dst_dev, size_t bytes, void* stream) {
    EXORL_REQUIRE(r && dst_dev, "replay_keys_read: null argument");
    EXORL_REQUIRE(r->keys_valid, "replay_keys_read: no key table, or a stale one (exorl_replay_build_keys)");
    const ReplayKeys k = replay_keys(r);
    EXORL_REQUIRE(bytes == (size_t)k.n * k.pitch * sizeof(float), "replay_keys_read: buffer of %zu bytes, the table has %lld rows of %d floats",
                  bytes, (long long)k.n, k.pitch);
    EXORL_CHECK_HIP(hipMemcpyAsync(dst_dev, k.ptr, bytes, hipMemcpyDeviceToDevice, as_stream(stream)));
    return 0;
}

int exorl_replay_num_rows(exorl_replay_t* r, int64_t* live_rows, int64_t* used_rows) {
    EXORL_REQUIRE(r, "replay_num_rows: null handle");
    if (live_rows) *live_rows = r->live_rows;
    if (used_rows) *used_rows = r->used_rows;
    return 0;
}

int exorl_replay_num_episodes(exorl_replay_t* r, int32_t* n) {
    EXORL_REQUIRE(r && n, "replay_num_episodes: null argument");
    *n = (int32_t)r->order.size();
    return 0;
}

int exorl_replay_seed_mt(exorl_replay_t* r, const uint32_t* py_key, int32_t py_pos, const uint32_t* np_key, int32_t np_pos) {
    EXORL_REQUIRE(r && py_key && np_key, "replay_seed_mt: null argument");
    EXORL_REQUIRE(py_pos >= 0 && py_pos <= 624 && np_pos >= 0 && np_pos <= 624, "replay_seed_mt: bad position");
    memcpy(r->py.mt, py_key, sizeof(r->py.mt)); r->py.pos = py_pos;
    memcpy(r->np.mt, np_key, sizeof(r->np.mt)); r->np.pos = np_pos;
    r->mt_seeded = true;
    return 0;
}

int exorl_replay_seed_mt_ints(exorl_replay_t* r, uint64_t py_seed, uint32_t np_seed) {
    EXORL_REQUIRE(r, "replay_seed_mt_ints: null handle");
    uint32_t key[2] = {(uint32_t)py_seed, (uint32_t)(py_seed >> 32)};
    r->py.init_by_array(key, key[1] ? 2 : 1);      // random.seed(int): 32-bit limbs of abs(seed)
    r->np.init_genrand(np_seed);                   // np.random.seed(int)
    r->mt_seeded = true;
    return 0;
}

int exorl_replay_get_mt(exorl_replay_t* r, uint32_t* py_key, int32_t* py_pos, uint32_t* np_key, int32_t* np_pos) {
    EXORL_REQUIRE(r && py_key && np_key && py_pos && np_pos, "replay_get_mt: null argument");
    memcpy(py_key, r->py.mt, sizeof(r->py.mt)); *py_pos = r->py.pos;
    memcpy(np_key, r->np.mt, sizeof(r->np.mt)); *np_pos = r->np.pos;
    return 0;
}

int exorl_replay_seed_philox(exorl_replay_t* r, uint64_t seed) {
    EXORL_REQUIRE(r, "replay_seed_philox: null handle");
    r->philox_seed = seed;
    r->philox_counter = 0;
    return 0;
}

}  // extern "C"

namespace exorl {
int replay_prepare(exorl_replay* r, int32_t batch, int32_t nstep, hipStream_t s) {
    EXORL_REQUIRE(r && batch > 0, "replay_prepare: bad arguments");
    EXORL_REQUIRE(!r->order.empty(), "replay_sample: no resident episodes (IndexError in random.choice, replay_buffer.py:169)");
    EXORL_TRY(upload_table(r, nstep, s));
    if (batch > r->pairs_cap) {
        if (r->d_pairs) EXORL_CHECK_HIP(hipFree(r->d_pairs));
        EXORL_CHECK_HIP(hipMalloc((void**)&r->d_pairs, (size_t)batch * 2 * sizeof(int32_t)));
        r->pairs_cap = batch;
    }
    if (r->goal_n && batch > r->goals_cap) {
        if (r->d_goals) EXORL_CHECK_HIP(hipFree(r->d_goals));
        r->d_goals = nullptr; r->goals_cap = 0;
        EXORL_CHECK_HIP(hipMalloc((void**)&r->d_goals, (size_t)batch * 2 * sizeof(int32_t)));
        r->goals_cap = batch;
    }
    if (nstep > 0 && !r->weighted)      // unweighted Philox draws a start inside every episode: all of them must hold nstep transitions
        EXORL_REQUIRE(r->min_len - nstep + 1 >= 1, "replay_sample: shortest episode (%d) shorter than nstep=%d", r->min_len, nstep);
    return 0;
}

// dev_counter != nullptr: Philox batch counter is read from device memory (graph-replayable); the host copy is
// still advanced so eager sampling continues the stream afterwards.
int replay_sample_impl(exorl_replay* r, int32_t batch, int32_t nstep, float gamma, int32_t sampler,
                       const int32_t* pairs_host, const exorl_batch_out* out, int32_t* pairs_out_host, hipStream_t s,
                       const uint64_t* dev_counter, const StageOut* stage, float* mc_return, const GoalOut* goal) {
    EXORL_REQUIRE(r && out, "replay_sample: null argument");
    if (goal) {
        EXORL_REQUIRE(r->goal_n > 0, "replay_sample_goal: no goal rule is set (exorl_replay_set_goal)");
        EXORL_REQUIRE(r->frames == 1 && !stage, "replay_sample_goal: goals are gathered from fp32 state rows into the caller's rows, un-staged");
        EXORL_REQUIRE(goal->goal && goal->next_goal && goal->goal_stride >= r->goal_n && goal->next_goal_stride >= r->goal_n,
                      "replay_sample_goal: goal / next_goal destinations of %d floats per row (strides %lld / %lld)", r->goal_n,
                      (long long)goal->goal_stride, (long long)goal->next_goal_stride);
        EXORL_REQUIRE(!mc_return || r->goal_mode == EXORL_GOAL_KEEP, "replay_sample_goal: an mc_return destination with a relabelled reward: the "
                      "return-to-go column is the arena reward's, which only reward_mode keep emits");
        EXORL_REQUIRE(sampler == EXORL_SAMPLER_PHILOX || goal->goals_host, "replay_sample_goal: EXORL_SAMPLER_GIVEN and EXORL_SAMPLER_MT19937 need "
                      "goals_host, the (pos_g, tau) of every sample");
    }
    if (mc_return) {
        EXORL_REQUIRE(r->rtg_valid, "replay_sample_mc: no return-to-go column, or a stale one: an episode was appended or evicted or the order was "
                      "set since exorl_replay_build_returns (call it again)");
        EXORL_REQUIRE(memcmp(&gamma, &r->rtg_gamma, sizeof(float)) == 0, "replay_sample_mc: gamma=%.9g, the column was built with %.9g", gamma,
                      r->rtg_gamma);
    }
    EXORL_REQUIRE(!stage || (r->frames == 1 && r->cfg.obs_bytes == stage->O * 4 && r->cfg.act_dim == stage->A && stage->B == batch),
                  "replay_sample: staged outputs need fp32 state observations of the agent's dimensions");
    EXORL_REQUIRE(batch > 0 && nstep >= 1, "replay_sample: batch=%d nstep=%d", batch, nstep);
    EXORL_REQUIRE(out->obs && out->action && out->reward && out->discount && out->next_obs, "replay_sample: null output");
    EXORL_REQUIRE((r->cfg.meta_dim > 0) || out->meta == nullptr, "replay_sample: meta output without meta columns");
    EXORL_REQUIRE((out->next_action == nullptr) == (out->next_valid == nullptr), "replay_sample: next_action and next_valid go together");
    if (r->frames > 1) {
        const int64_t need = (int64_t)r->frames * r->cfg.obs_bytes;
        EXORL_REQUIRE(out->obs_stride >= need && out->next_obs_stride >= need, "replay_sample: obs_stride=%lld / next_obs_stride=%lld cannot "
                      "hold an observation of %d frames x %d bytes", (long long)out->obs_stride, (long long)out->next_obs_stride, r->frames,
                      r->cfg.obs_bytes);
        EXORL_REQUIRE(2ll * r->frames * batch <= INT32_MAX, "replay_sample: batch=%d x %d frames: too many output frames", batch, r->frames);
    }
    const int n = (int)r->order.size();
    EXORL_REQUIRE(!(r->weighted && sampler == EXORL_SAMPLER_MT19937), "replay_sample: weighted sampling needs EXORL_SAMPLER_PHILOX: the MT19937 "
                  "sampler reproduces the reference's unweighted index stream (exorl_replay_set_weights(EPISODES, NULL) turns weighting off)");
    EXORL_TRY(replay_prepare(r, batch, sampler == EXORL_SAMPLER_PHILOX ? nstep : 0, s));
    if (sampler == EXORL_SAMPLER_MT19937 || sampler == EXORL_SAMPLER_GIVEN) {
        r->h_pairs.resize((size_t)batch * 2);
        if (sampler == EXORL_SAMPLER_MT19937) {
            EXORL_REQUIRE(r->mt_seeded, "replay_sample: MT19937 streams not seeded (exorl_replay_seed_mt)");
            for (int b = 0; b < batch; ++b) {
                const int pos = (int)r->py.py_randbelow((uint32_t)n);
                const int len = r->slots[r->order[pos]].rows - 1;
                EXORL_REQUIRE(len - nstep + 1 >= 1, "replay_sample: episode of length %d shorter than nstep=%d (ValueError in "
                              "np.random.randint, replay_buffer.py:222)", len, nstep);
                r->h_pairs[2 * b] = pos;
                r->h_pairs[2 * b + 1] = (int)r->np.np_randint0((uint32_t)(len - nstep + 1)) + 1;
            }
        } else {
            EXORL_REQUIRE(pairs_host, "replay_sample: EXORL_SAMPLER_GIVEN needs pairs_host");
            for (int b = 0; b < batch; ++b) {
                const int pos = pairs_host[2 * b], idx = pairs_host[2 * b + 1];
                EXORL_REQUIRE(pos >= 0 && pos < n, "replay_sample: pair %d: position %d out of range [0,%d)", b, pos, n);
                const int len = r->slots[r->order[pos]].rows - 1;
                EXORL_REQUIRE(idx >= 1 && idx + nstep - 1 <= len, "replay_sample: pair %d: idx %d out of range for len %d nstep %d",
                              b, idx, len, nstep);
                r->h_pairs[2 * b] = pos;
                r->h_pairs[2 * b + 1] = idx;
            }
        }
        EXORL_CHECK_HIP(hipMemcpyAsync(r->d_pairs, r->h_pairs.data(), (size_t)batch * 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
        if (pairs_out_host) memcpy(pairs_out_host, r->h_pairs.data(), (size_t)batch * 2 * sizeof(int32_t));
    } else if (sampler != EXORL_SAMPLER_PHILOX) {
        set_error("replay_sample: unknown sampler %d", sampler);
        return 2;
    }
    if (goal && sampler != EXORL_SAMPLER_PHILOX) {
        r->h_goals.resize((size_t)batch * 2);
        for (int b = 0; b < batch; ++b) {
            const int pos = goal->goals_host[2 * b], tau = goal->goals_host[2 * b + 1];
            EXORL_REQUIRE(pos >= 0 && pos < n, "replay_sample_goal: goal %d: position %d out of range [0,%d)", b, pos, n);
            const int len = r->slots[r->order[pos]].rows - 1;
            EXORL_REQUIRE(tau >= 0 && tau <= len, "replay_sample_goal: goal %d: time %d out of range [0,%d]", b, tau, len);
            r->h_goals[2 * b] = pos;
            r->h_goals[2 * b + 1] = tau;
        }
        EXORL_CHECK_HIP(hipMemcpyAsync(r->d_goals, r->h_goals.data(), (size_t)batch * 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    }
    ReplayView v{r->obs, r->act, r->rew, r->disc, r->meta, r->d_row0, r->d_len, r->cfg.obs_bytes, r->cfg.act_dim, r->cfg.meta_dim, n,
                 r->weighted && sampler == EXORL_SAMPLER_PHILOX ? r->d_cum : nullptr, r->d_guide, r->guide_bits,
                 r->norm_on ? r->d_norm : nullptr, r->norm_on ? r->d_norm + r->cfg.obs_bytes / 4 : nullptr, r->d_rtg};
    if (r->frames > 1) {
        hipLaunchKernelGGL(gather_frames_kernel, dim3(cdiv(2 * r->frames * batch, 4)), dim3(256), 0, s, v, r->d_pairs, r->d_pairs, *out, batch,
                           nstep, gamma, sampler, r->philox_seed, r->philox_counter, dev_counter, r->frames, mc_return);
    } else {
        const int vec16 = (r->cfg.obs_bytes % 16 == 0) && (out->obs_stride % 16 == 0) && (out->next_obs_stride % 16 == 0) &&
                          ((uintptr_t)out->obs % 16 == 0) && ((uintptr_t)out->next_obs % 16 == 0);
        if (goal) {
            const GoalView gv{r->d_goal_cols, r->goal_n, r->goal_t_cur, r->goal_t_traj, r->d_goal_tab, r->goal_tab_n, r->goal_mode, r->d_goals,
                              goal->goal, goal->next_goal, goal->goal_stride, goal->next_goal_stride};
            const auto kernel = r->norm_on ? gather_nstep_kernel<true, GoalView> : gather_nstep_kernel<false, GoalView>;
            hipLaunchKernelGGL(kernel, dim3(cdiv(batch, 4)), dim3(256), 0, s, v, r->d_pairs, r->d_pairs, *out, batch, nstep, gamma, sampler,
                               r->philox_seed, r->philox_counter, dev_counter, vec16, StageOut{}, mc_return, gv);
        } else {
            hipLaunchKernelGGL(r->norm_on ? gather_nstep_kernel<true> : gather_nstep_kernel<false>, dim3(cdiv(batch, 4)), dim3(256), 0, s, v,
                               r->d_pairs, r->d_pairs, *out, batch, nstep, gamma, sampler, r->philox_seed, r->philox_counter, dev_counter, vec16,
                               stage ? *stage : StageOut{}, mc_return);
        }
    }
    EXORL_LAUNCH_CHECK();
    if (sampler == EXORL_SAMPLER_PHILOX) r->philox_counter += 1;
    return 0;
}

uint64_t replay_philox_counter(exorl_replay* r) { return r->philox_counter; }
uint64_t replay_weights_epoch(exorl_replay* r) { return r->weights_epoch; }
bool replay_norm_on(exorl_replay* r) { return r->norm_on; }
int replay_obs_bytes(exorl_replay* r) { return r->frames * r->cfg.obs_bytes; }      // of one SAMPLED observation
int replay_frame_stack(exorl_replay* r) { return r->frames; }
ReplayKeys replay_keys(exorl_replay* r) {
    return ReplayKeys{r->d_keys, r->keys_n, (int)round_up(r->cfg.obs_bytes / 4 + r->cfg.act_dim, 4), r->cfg.obs_bytes / 4, r->cfg.act_dim, r->keys_beta,
                      r->keys_epoch, r->keys_valid};
}
void replay_dims(exorl_replay* r, int* act_dim, int* meta_dim) { *act_dim = r->cfg.act_dim; *meta_dim = r->cfg.meta_dim; }
void replay_advance_philox(exorl_replay* r, uint64_t n) { r->philox_counter += n; }
ReplayReturns replay_returns(exorl_replay* r) { return ReplayReturns{r->d_rtg, r->rtg_gamma, r->rtg_epoch, r->rtg_valid}; }
int replay_goal_cols(exorl_replay* r) { return r->goal_n; }
uint64_t replay_goal_epoch(exorl_replay* r) { return r->goal_epoch; }
}  // namespace exorl

extern "C" {

int exorl_replay_sample(exorl_replay_t* r, int32_t batch, int32_t nstep, float gamma, int32_t sampler,
                        const int32_t* pairs_host, const exorl_batch_out* out, int32_t* pairs_out_host, void* stream) {
    return replay_sample_impl(r, batch, nstep, gamma, sampler, pairs_host, out, pairs_out_host, as_stream(stream), nullptr);
}

int exorl_replay_sample_mc(exorl_replay_t* r, int32_t batch, int32_t nstep, float gamma, int32_t sampler, const int32_t* pairs_host,
                           const exorl_batch_out* out, float* mc_return_dev, int32_t* pairs_out_host, void* stream) {
    return replay_sample_impl(r, batch, nstep, gamma, sampler, pairs_host, out, pairs_out_host, as_stream(stream), nullptr, nullptr, mc_return_dev);
}

int exorl_replay_sample_goal(exorl_replay_t* r, int32_t batch, int32_t nstep, float gamma, int32_t sampler, const int32_t* pairs_host,
                             const int32_t* goals_host, const exorl_batch_out* out, float* goal_dev, int64_t goal_stride, float* next_goal_dev,
                             int64_t next_goal_stride, float* mc_return_dev, int32_t* pairs_out_host, void* stream) {
    const GoalOut g{goals_host, goal_dev, goal_stride, next_goal_dev, next_goal_stride};
    return replay_sample_impl(r, batch, nstep, gamma, sampler, pairs_host, out, pairs_out_host, as_stream(stream), nullptr, nullptr, mc_return_dev, &g);
}

int exorl_replay_last_goals(exorl_replay_t* r, int32_t batch, int32_t* goals_host, void* stream) {
    EXORL_REQUIRE(r && goals_host && batch > 0 && batch <= r->goals_cap, "replay_last_goals: bad arguments (no goal launch of that batch yet?)");
    hipStream_t s = as_stream(stream);
    EXORL_CHECK_HIP(hipMemcpyAsync(goals_host, r->d_goals, (size_t)batch * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    EXORL_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}

int exorl_replay_last_pairs(exorl_replay_t* r, int32_t batch, int32_t* pairs_host, void* stream) {
    EXORL_REQUIRE(r && pairs_host && batch > 0 && batch <= r->pairs_cap, "replay_last_pairs: bad arguments");
    hipStream_t s = as_stream(stream);
    EXORL_CHECK_HIP(hipMemcpyAsync(pairs_host, r->d_pairs, (size_t)batch * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    EXORL_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}

}  // extern "C"
