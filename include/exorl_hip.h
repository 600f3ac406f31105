/*
 * exorl_hip.h — C ABI of libexorl_hip.so, the MI355X (gfx950) backend for the exorl RL-update hot path.
 *
 * Drop-in boundary. Each entry point names the reference interface it replaces
 * (paths relative to the reference repo AOS55/exorl):
 *
 *   exorl_replay_*          utils/replay_buffer.py:153-239  ReplayBuffer (_store_episode, eviction,
 *                           _sample: episode pick + start index + gather + n-step return) and
 *                           :241-277 make_replay_loader / DataLoader collate (batched output)
 *   exorl_agent_create      agents/offline_learning/td3_bc.py:59-100 (and td3.py, bc.py,
 *                           agents/unsupervised_learning/ddpg.py:126-197) constructors
 *   exorl_agent_update*     td3_bc.py:119-189, td3.py:117-186, bc.py:78-110, ddpg.py:240-328
 *                           (update_critic / update_actor / soft_update_params / update)
 *   exorl_agent_act         td3_bc.py:107-117, ddpg.py:221-238
 *   exorl_adam_step         torch.optim.Adam.step as used at td3_bc.py:96-97,142,160
 *   exorl_soft_update       utils/utils.py:44-47
 *   exorl_knn_*             utils/utils.py:279-319 (PBE) and unsupervised_learning/proto.py:114-119
 *
 * Conventions: plain pointers and sizes only (no torch types). Every function returns 0 on success,
 * non-zero on error; exorl_last_error() returns the message of the calling thread's last error.
 * All device work is enqueued on the `stream` argument (a hipStream_t passed as void*; NULL = the
 * default stream) and is asynchronous unless stated. Pointers named *_dev are device pointers,
 * *_host host pointers. One host thread per GPU; handles are not thread-safe.
 */
#ifndef EXORL_HIP_H
#define EXORL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EXORL_ABI_VERSION 13     /* 8 (round 3): EXORL_PREC_BF16X6, exorl_agent_act_host, exorl_debug_precision_override
                                    9: exorl_debug_gemm_stamps and exorl_debug_conv_stamps removed; exorl_gemm_tune keeps five bits
                                    10: exorl_pixel_cfg.world_size; exorl_pixel_agent_update_phase / _grad_buffer / _set_comm
                                    11: exorl_intr_cfg.world_size / rank; exorl_intr_update_phase / _exchange; exorl_pixel_agent_encoder_step_phase /
                                        _rnd_features_phase / _bn_partials; exorl_pixel_agent_grad_buffer exchange 2
                                    12: exorl_debug_agent_poison_scratch; (added since, no version change: exorl_gemm_planes3, EXORL_PREC_BF16X6 for
                                        exorl_agent_cfg.precision, exorl_agent_enable_graph_intr, exorl_debug_agent_weight_images, exorl_replay_set_weights,
                                        exorl_replay_set_frame_stack, exorl_agent_update_plan, exorl_replay_obs_moments, exorl_replay_set_obs_norm)                                    13: exorl_pixel_step replaces the loose arguments of exorl_pixel_agent_update / _update_phase; the three phased pixel
                                        calls return next_exchange; exorl_pixel_agent_exchange replaces _grad_buffer and _bn_partials; (added since, no version change:
                                        exorl_agent_eval_bytes / _set_eval / _evaluate / _eval_read; EXORL_AGENT_IQL, exorl_agent_set_iql;
                                        EXORL_AGENT_FQE, exorl_agent_fqe_value_bytes / _set_fqe_value / _fqe_value / _fqe_value_read,
                                        exorl_replay_episode_returns, exorl_replay_num_episodes; EXORL_AGENT_PRDC, exorl_replay_build_keys,
                                        exorl_replay_keys, exorl_replay_keys_read, exorl_nn_search, exorl_agent_set_prdc, exorl_agent_nn_result;
                                        exorl_batch_out.next_action / next_action_stride / next_valid (trailing);
                                        exorl_agent_rebrac_bytes, exorl_agent_set_rebrac, exorl_rebrac_rows;
                                        exorl_agent_sarsa_bytes, exorl_agent_set_sarsa, exorl_next_action_rows;
                                        exorl_replay_build_returns, exorl_replay_returns, exorl_replay_returns_read, exorl_replay_sample_mc,
                                        exorl_agent_calql_bytes, exorl_agent_set_calql, exorl_cql_dq_rows, EXORL_M_CALQL_BOUND;
                                        exorl_replay_set_goal, exorl_replay_sample_goal, exorl_replay_last_goals, exorl_agent_enable_graph_goal,
                                        EXORL_GOAL_KEEP / _NEG / _SPARSE) */

const char* exorl_last_error(void);
int exorl_abi_version(void);
/* device name / CU count of the current HIP device (fails if none). */
int exorl_device_info(char* name_out, int name_len, int* num_cus, int64_t* hbm_bytes);

/* ------------------------------------------------------------------------------------------------
 * Replay: episodic buffer resident in HBM.
 * Arena layout (SoA, row = one time-step; episode = len+1 consecutive rows, row 0 the dummy reset step):
 *   obs[rows][obs_bytes]  action[rows][act_dim] f32  reward[rows] f32  discount[rows] f32  meta[rows][meta_dim] f32
 * ---------------------------------------------------------------------------------------------- */
typedef struct exorl_replay exorl_replay_t;

typedef struct {
    int32_t obs_bytes;      /* bytes per observation row: O*4 (f32 states) or C*H*W (u8 pixels); multiple of 4 */
    int32_t act_dim;
    int32_t meta_dim;       /* total width of the concatenated meta columns (0 = none) */
    int32_t max_episodes;
    int64_t capacity_rows;  /* arena rows = transitions + one dummy row per episode */
} exorl_replay_cfg;

typedef struct {            /* where one sampled minibatch is written (device memory, caller-owned) */
    void*   obs;       int64_t obs_stride;       /* bytes between consecutive samples */
    float*  action;    int64_t action_stride;    /* floats between consecutive samples */
    float*  reward;                              /* (B) contiguous */
    float*  discount;                            /* (B) contiguous */
    void*   next_obs;  int64_t next_obs_stride;  /* bytes */
    float*  meta;      int64_t meta_stride;      /* floats; may be NULL when meta_dim == 0 */
    /* Trailing and optional (a caller that zero-fills the struct gets neither): the action taken at next_obs, action[idx + nstep], and whether
     * the episode holds it (idx + nstep <= len). An invalid sample gets next_valid = 0 and a row of zeros; the arena row behind the episode's last
     * (the next episode's dummy row, or past the arena's end) is never read. A plain copy: bit-exact, untouched by exorl_replay_set_obs_norm.
     * Written by the same gather launch; with next_action NULL every other output keeps its bits. Read by the TD3+BC step while ReBRAC is
     * set on the handle (exorl_agent_set_rebrac): the critic target's penalty on (a~' - a')^2; and by the critic step of TD3+BC, TD3, CRR and FQE
     * while the SARSA setting is on (exorl_agent_set_sarsa): the action the target critic is fed at s'. */
    float*  next_action;  int64_t next_action_stride;   /* floats between samples; NULL: not written */
    float*  next_valid;                                 /* (B) contiguous, 1.0f or 0.0f; NULL iff next_action is NULL */
} exorl_batch_out;

#define EXORL_SAMPLER_MT19937 0   /* reference-exact index stream (CPython random + NumPy legacy RandomState) */
#define EXORL_SAMPLER_PHILOX  1   /* device-side counter-based stream, same distribution */
#define EXORL_SAMPLER_GIVEN   2   /* (episode position, start idx) pairs supplied by the caller */

int exorl_replay_create(const exorl_replay_cfg* cfg, exorl_replay_t** out);
int exorl_replay_destroy(exorl_replay_t* r);
/* Copies one episode (rows = len+1 host rows per array) into the arena; returns its slot id. */
int exorl_replay_append_episode(exorl_replay_t* r, const void* obs_host, const float* act_host,
                                const float* rew_host, const float* disc_host, const float* meta_host,
                                int32_t rows, int32_t* slot_out);
int exorl_replay_evict(exorl_replay_t* r, int32_t slot);
/* Sampling order of resident episodes = the reference's sorted `_episode_fns` list (replay_buffer.py:184). */
int exorl_replay_set_order(exorl_replay_t* r, const int32_t* slots_host, int32_t n);
int exorl_replay_num_rows(exorl_replay_t* r, int64_t* live_rows, int64_t* used_rows);
/* Weighted sampling for EXORL_SAMPLER_PHILOX. q_per_slot_host: one integer weight per slot id (n_slots <= slots handed out so far; the
 * rest, and NULL, mean 1); a slot reused by exorl_replay_append_episode goes back to 1. With span_e = max(len_e - nstep + 1, 0):
 *   EXORL_WEIGHT_EPISODES     P(episode e) ~ q_e where span_e > 0, then a uniform start        (NULL weights: the unweighted sampler)
 *   EXORL_WEIGHT_TRANSITIONS  P(episode e) ~ q_e * span_e, then a uniform start                (NULL weights: uniform over transitions)
 * Draw: x = philox(sample, batch counter) as unweighted; g = mulhi64(x2 << 32 | x3, total mass); the episode is the one whose interval
 * of the running mass sum holds g; start = mulhi32(x1, span_e) + 1. Episodes shorter than nstep have mass 0 and are skipped instead of
 * refused. A sample call fails, launching nothing, when the total mass is 0 or reaches 2^63, or when the sampler is
 * EXORL_SAMPLER_MT19937 (the reference's stream stays unweighted); EXORL_SAMPLER_GIVEN ignores the weights. A captured graph
 * (exorl_agent_enable_graph) holds the table of its capture: re-capture after changing weights, mode or resident episodes;
 * exorl_agent_step_graph refuses to replay a graph captured before the latest exorl_replay_set_weights call. */
#define EXORL_WEIGHT_EPISODES    0
#define EXORL_WEIGHT_TRANSITIONS 1
int exorl_replay_set_weights(exorl_replay_t* r, int32_t mode, const uint32_t* q_per_slot_host, int32_t n_slots);
/* Frame stacking, frames in [1, 16] (1, the default: none), allowed only before the first exorl_replay_append_episode. With frames = k > 1
 * cfg.obs_bytes is ONE frame (c0*H*W of the k*c0 stacked channels) and row t of an episode holds the single frame the env produced at
 * step t; a sampled observation is frames * obs_bytes bytes, the frames of steps max(t-k+1, 0) .. t oldest first (t = idx-1 for obs,
 * idx+nstep-1 for next_obs): what a frame-stack wrapper's deque, filled with the reset frame, held at step t. Samples are byte-identical
 * to those of an arena without stacking that was fed the stacked episodes, for every sampler, weighting, eviction and compaction, at
 * 1/k of the arena's observation bytes. exorl_replay_sample fails, launching nothing, unless out->obs_stride and out->next_obs_stride
 * are >= frames * obs_bytes. exorl_agent_enable_graph / _intr refuse such an arena (the captured step reads whole arena rows). */
int exorl_replay_set_frame_stack(exorl_replay_t* r, int32_t frames);
/* Column moments of the fp32 observations, in fp64: over ALL rows (len + 1 each, the reset row included: every observation the sampler can
 * return as obs or next_obs) of the episodes in the current order table, *count_host = the number of rows, mean_host[j] the mean of column
 * j and m2_host[j] = sum (x - mean_j)^2. Evicted slots and holes awaiting compaction are not read. Two launches: fixed ranges of
 * (episode, 64-row chunk) items per workgroup, Welford per thread, Chan's pairwise update between threads and workgroups, one fp64
 * partial per workgroup in a slab the replay owns; then the slab combined in slab order. No atomics: two calls on the same arena return
 * the same bits, and a constant column returns m2 == 0. Fails, launching nothing, unless n_cols * 4 == obs_bytes, the arena is not
 * frame-stacked and at least one episode is resident. A set-up call: it synchronises `stream`; never call it inside a capture. */
int exorl_replay_obs_moments(exorl_replay_t* r, int32_t n_cols, int64_t* count_host, double* mean_host, double* m2_host, void* stream);
/* Discounted return of every episode of the current order table, in fp64: returns_host[e] = sum_{t=1..len} r[t] prod_{k<t} (gamma d[k]) for
 * the episode at table position e, gamma the float32 the gather uses widened to double, r and d the stored float32 values widened: the
 * gather's n-step recurrence started at idx 1 with nstep = len. n must equal the number of episodes in the table. One workgroup per episode:
 * a thread folds a contiguous run of steps into a pair (R, D), pairs combine in step order with (R1, D1) o (R2, D2) = (R1 + D1 R2, D1 D2)
 * in a fixed tree. No atomics: two calls return the same bits. Evicted slots and holes are not read. A set-up call: it synchronises `stream`;
 * never call it inside a capture. */
int exorl_replay_episode_returns(exorl_replay_t* r, float gamma, double* returns_host, int32_t n, void* stream);
/* The Monte-Carlo return-to-go of every transition of the order table, one float per arena row, built by one launch. For an episode of
 * length L at rows row0 + 1 .. row0 + L, with gamma widened to double: G_L = r_L, G_i = r_i + (gamma d_i) G_{i+1}, all in fp64, stored as
 * float (round to nearest) at row row0 + i; the dummy row gets 0. This is the gather's n-step recurrence carried to the episode's end: G_1 is
 * what exorl_replay_episode_returns reports. An episode cut by a time limit (d = 1 on its last step) gets the return of its recorded
 * remainder and no bootstrap, which is a lower bound on the true return only where rewards are >= 0 (as the DMC tasks' are).
 * One workgroup per episode: a thread folds its run of steps backwards into episode_returns' (R, D) pair, the pairs go through a suffix scan
 * in a fixed order (the earlier run is always the left operand), and the thread walks its run a second time to store. No atomics; the kernel
 * reads reward and discount of the episode's own rows only, so an episode's bits do not depend on where it sits or on what else is resident.
 * The column (capacity_rows floats) is allocated at the first build and never moves; a rebuild is one launch over the current order table.
 * exorl_replay_append_episode, _evict and _set_order make it stale; weights, the normaliser and the frame stack do not.
 * A set-up call (it synchronises `stream`). Refuses, launching nothing: a null handle, an empty order table, a stream that is being captured. */
int exorl_replay_build_returns(exorl_replay_t* r, float gamma, void* stream);
/* The column as the last build left it: its device pointer (NULL before the first build), the build's gamma, a count of builds and
 * invalidations, and whether it stands (1) or is stale or absent (0). Any output may be NULL. */
int exorl_replay_returns(exorl_replay_t* r, float** ptr_dev, float* gamma, uint64_t* epoch, int32_t* valid);
/* G_1 .. G_L of every order-table episode, concatenated in table order, into n host floats. Synchronous. Refuses a stale or absent column and
 * an n other than the table's transition count. */
int exorl_replay_returns_read(exorl_replay_t* r, float* dst_host, int64_t n, void* stream);
/* Episodes in the current order table: the positions EXORL_SAMPLER_GIVEN accepts are [0, *n). */
int exorl_replay_num_episodes(exorl_replay_t* r, int32_t* n);
/* Observation normaliser of the gather: with n_cols = obs_bytes / 4 values each in mean_host and inv_scale_host, every obs and next_obs
 * element exorl_replay_sample (and the captured step's staged gather) writes is y = (x - mean[j]) * inv_scale[j], two fp32 operations in
 * that order, never contracted; action, reward, discount, meta and the pairs are untouched. n_cols = 0 turns it off (the default: the
 * gather copies the rows). The values live in a device buffer allocated at create; calling again with new values writes them in place
 * on `stream` and later launches, graph replays included, use them. Switching between off and on changes the captured kernel:
 * exorl_agent_step_graph refuses a graph captured in the other state. Fails for n_cols * 4 != obs_bytes and on a frame-stacked arena;
 * exorl_agent_enable_graph_intr refuses a normalised arena. */
int exorl_replay_set_obs_norm(exorl_replay_t* r, int32_t n_cols, const float* mean_host, const float* inv_scale_host, void* stream);
/* The key table of the nearest-neighbour search (EXORL_AGENT_PRDC): one row per resident transition, episodes in order-table order and
 * t = 1 .. len inside each, row = [beta * s | a | 0-pad] with s = obs[t - 1] as the gather would emit it (with a normaliser set,
 * (x - mean) * inv_scale in the same two uncontracted fp32 operations), beta * s one further fp32 product, a = action[t]; the pitch is
 * round_up(obs_bytes / 4 + act_dim, 4) floats. key_every = m >= 1 keeps the transitions whose running index i has i % m == 0, as row i / m.
 * One launch over (episode, 64-transition chunk) items into a device buffer the replay owns; evicted slots and holes are not read. Fails,
 * launching nothing, on a frame-stacked arena, with no resident episode, for beta < 0 and inside a capture. The arena must hold fp32 state
 * rows (the C side cannot tell: a u8 arena is refused by the caller that knows the type). A set-up call: it allocates and synchronises.
 * The table is a snapshot: exorl_replay_append_episode, exorl_replay_evict, exorl_replay_set_order and exorl_replay_set_obs_norm all mark
 * it stale, and a new build replaces it. */
int exorl_replay_build_keys(exorl_replay_t* r, float beta, int32_t key_every, void* stream);
/* The table as last built: device pointer, rows, pitch in floats and the epoch of this build (it moves with every build and every
 * invalidation). Fails when there is no table or it is stale. */
int exorl_replay_keys(exorl_replay_t* r, void** ptr_dev, int64_t* n, int32_t* pitch, uint64_t* epoch);
/* Copies the table (n * pitch floats, `bytes` must be exactly that) into the caller's device buffer, on `stream`. Same refusals. */
int exorl_replay_keys_read(exorl_replay_t* r, void* dst_dev, size_t bytes, void* stream);
/* MT19937 states as exposed by random.getstate()[1] / np.random.get_state()[1:3]. */
int exorl_replay_seed_mt(exorl_replay_t* r, const uint32_t* py_key624, int32_t py_pos,
                         const uint32_t* np_key624, int32_t np_pos);
/* Convenience for callers without a Python interpreter: random.seed(py_seed); np.random.seed(np_seed). */
int exorl_replay_seed_mt_ints(exorl_replay_t* r, uint64_t py_seed, uint32_t np_seed);
int exorl_replay_get_mt(exorl_replay_t* r, uint32_t* py_key624, int32_t* py_pos,
                        uint32_t* np_key624, int32_t* np_pos);
int exorl_replay_seed_philox(exorl_replay_t* r, uint64_t seed);
/* One minibatch: B x (obs[idx-1], action[idx], n-step reward, n-step discount, obs[idx+n-1], meta[idx-1]) and, where out->next_action is set,
 * (action[idx+n] or zeros, next_valid). Fails, launching nothing, when exactly one of out->next_action and out->next_valid is NULL.
 * pairs_host: for EXORL_SAMPLER_GIVEN, B x {position in order, start idx >= 1};
 * pairs_out_host: if non-NULL receives the pairs drawn (MT19937 mode only; host-generated). */
int exorl_replay_sample(exorl_replay_t* r, int32_t batch, int32_t nstep, float gamma, int32_t sampler,
                        const int32_t* pairs_host, const exorl_batch_out* out, int32_t* pairs_out_host,
                        void* stream);

/* exorl_replay_sample with one more destination: mc_return_dev[b] = G[row0[pos] + idx], the sample's return-to-go from the column of
 * exorl_replay_build_returns, a plain copy written by the same gather launch (both gather kernels: the lane that writes reward and discount
 * writes it). With mc_return_dev NULL this is exorl_replay_sample: same bits, same launch. With a destination it refuses, launching nothing,
 * a missing or stale column and a gamma whose bits differ from the build's. (The destination is an argument because exorl_batch_out
 * keeps its size.) */
int exorl_replay_sample_mc(exorl_replay_t* r, int32_t batch, int32_t nstep, float gamma, int32_t sampler,
                           const int32_t* pairs_host, const exorl_batch_out* out, float* mc_return_dev, int32_t* pairs_out_host,
                           void* stream);

/* Synchronous: the (position, start idx) pairs of the last sample call, read back from the device. */
int exorl_replay_last_pairs(exorl_replay_t* r, int32_t batch, int32_t* pairs_host, void* stream);

/* Goal relabelling in the gather (fp32 state arenas). Sample b is the pair (pos, idx): obs at time t = idx - 1, next_obs at t + n, n = nstep,
 * T = len[pos] >= t + n. Its goal is a pair (pos_g, tau), arena row row0[pos_g] + tau, and g[j] = o_goal[cols[j]] for the n_cols column indices
 * of cols_host, with a normaliser set (x - mean[cols[j]]) * inv_scale[cols[j]] in the gather's two uncontracted operations: bit for bit the
 * normalised observation's columns. The same g is written behind obs and behind next_obs.
 * EXORL_SAMPLER_PHILOX draws the goal in the kernel; block (b, counter_lo, counter_hi, 0), the sample's own pair, keeps its bits.
 *   x = philox4x32_10((b, counter_lo, counter_hi, 1), seed); t_cur = floor(p_cur 2^32), t_traj = floor((p_cur + p_traj) 2^32) as uint64
 *   x[0] < t_cur   CUR   pos_g = pos, tau = t + n
 *   x[0] < t_traj  TRAJ  pos_g = pos, room = T - (t + n), tau = t + n + d;
 *                        horizon_gamma <= 0 (uniform):  d = (x[1] (room + 1)) >> 32
 *                        0 < horizon_gamma < 1:         d = min(#{k : tab[k] <= x[1]}, room), tab[k] = floor(2^32 (1 - p_k)), p_0 = horizon_gamma,
 *                                                       p_(k+1) = p_k horizon_gamma in double on the host; the table ends before its first entry
 *                                                       >= 2^32 - 1, or after 4096 entries; mass past the episode's end piles on its last state
 *   else           RAND  y = philox4x32_10((b, counter_lo, counter_hi, 2), seed); pos_g = the sampler's own episode choice on y (y[0] scaled
 *                        onto the episode count, or the cum / guide search on y[2], y[3] of a weighted arena: a zero-mass episode is never a
 *                        goal); tau = (y[1] (len[pos_g] + 1)) >> 32, any of the episode's len + 1 states
 * The other samplers take the goals from the caller (exorl_replay_sample_goal's goals_host).
 * reached = (pos_g == pos && tau == t + n), an equality of indices whatever the source. Reward and discount run through the n-step recurrence
 * of exorl_replay_sample in its operation order (t = D rho_i; R += t; u = c_i gamma; D *= u), only its per-step inputs substituted; only step
 * i = n - 1 can reach the goal:
 *   EXORL_GOAL_KEEP    rho_i = the arena's reward, c_i = the arena's discount (the goal is context only)
 *   EXORL_GOAL_NEG     rho_i = 0 on the reaching step, else -1;  c_i = 0 on the reaching step, else 1
 *   EXORL_GOAL_SPARSE  rho_i = 1 on the reaching step, else 0;   c_i = 0 on the reaching step, else 1
 * p_cur + p_traj + p_rand must be 1 within 1e-6. n_cols = 0 clears the rule. Refused on a frame-stacked arena and on one with meta columns; the
 * arena must hold fp32 state rows (the C side cannot tell: a u8 arena is refused by the caller that knows the type). A set-up call: it
 * synchronises the device. A graph captured by exorl_agent_enable_graph_goal is bound to the rule of its capture. */
#define EXORL_GOAL_KEEP   0
#define EXORL_GOAL_NEG    1
#define EXORL_GOAL_SPARSE 2
int exorl_replay_set_goal(exorl_replay_t* r, const int32_t* cols_host, int32_t n_cols, double p_cur, double p_traj, double p_rand,
                          double horizon_gamma /* <= 0: uniform */, int32_t reward_mode);
/* exorl_replay_sample_mc under the rule of exorl_replay_set_goal, the same single gather launch: goal_dev[b * goal_stride + j] and
 * next_goal_dev[b * next_goal_stride + j], j < n_cols, take g (strides in floats; [obs | g] rows: out->obs + 4 * O with stride
 * out->obs_stride / 4). goals_host: B x {pos_g, tau in [0, len[pos_g]]} for EXORL_SAMPLER_GIVEN and EXORL_SAMPLER_MT19937, range-checked on the
 * host as the pairs are; ignored by EXORL_SAMPLER_PHILOX. out->next_action / next_valid work as in exorl_replay_sample. mc_return_dev is
 * refused unless the reward mode is EXORL_GOAL_KEEP. The drawn (pos, idx) and every output of exorl_replay_sample other than reward and
 * discount are what exorl_replay_sample gives for the same seed and counter. (The destinations are arguments because exorl_batch_out keeps
 * its size.) */
int exorl_replay_sample_goal(exorl_replay_t* r, int32_t batch, int32_t nstep, float gamma, int32_t sampler, const int32_t* pairs_host,
                             const int32_t* goals_host, const exorl_batch_out* out, float* goal_dev, int64_t goal_stride, float* next_goal_dev,
                             int64_t next_goal_stride, float* mc_return_dev, int32_t* pairs_out_host, void* stream);
/* Synchronous: the (pos_g, tau) goals of the last exorl_replay_sample_goal call (or captured goal step), read back from the device. */
int exorl_replay_last_goals(exorl_replay_t* r, int32_t batch, int32_t* goals_host, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Data-parallel communicator: RCCL over xGMI, one per process / GPU. The reference has no distributed path; these
 * are the exchanges its single-process update implies when the batch is sharded: critic gradients before critic_opt.step()
 * (td3_bc.py:140-142), the batch-global sum |Q| behind lambda (:154), actor gradients before actor_opt.step() (:158-160).
 * ---------------------------------------------------------------------------------------------- */
typedef struct exorl_comm exorl_comm_t;
#define EXORL_COMM_ID_BYTES 128
/* Rank 0 makes the id and hands the bytes to the other ranks by any channel (torch.distributed broadcast, MPI, a file). */
int exorl_comm_unique_id(void* id_out_host /* EXORL_COMM_ID_BYTES */);
/* Collective over all ranks, on the caller's current HIP device. */
int exorl_comm_init(int32_t rank, int32_t nranks, const void* id_host, exorl_comm_t** out);
int exorl_comm_destroy(exorl_comm_t* c);
/* In-place float32 sum all-reduce, enqueued on `stream`. */
int exorl_comm_allreduce(exorl_comm_t* c, float* buf_dev, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Agents
 * ---------------------------------------------------------------------------------------------- */
typedef struct exorl_agent exorl_agent_t;

#define EXORL_AGENT_TD3_BC 0
#define EXORL_AGENT_TD3    1
#define EXORL_AGENT_BC     2
#define EXORL_AGENT_DDPG   3   /* states; shared-trunk critic (ddpg.py:79-123) */
#define EXORL_AGENT_CRR    4   /* agents/offline_learning/crr.py:59-219 */
#define EXORL_AGENT_CQL    5   /* agents/offline_learning/cql.py:59-286 */
#define EXORL_AGENT_APS    6   /* agents/unsupervised_learning/aps.py:12-60,268-320: DDPG with the successor-feature critic
                                  (heads emit sf_dim features, Q = task . features; the task is the last sf_dim columns of obs) */
/* kind 7 is unassigned and refused */
#define EXORL_AGENT_IQL    8   /* implicit Q-learning, no reference file: a value net V(s) regressed on min Q'(s, a) by expectile regression,
                                  critics regressed on r + D V(s'), actor by the advantage-weighted log-likelihood (CRR's actor step with
                                  w = min(exp(temperature (min Q' - V)), max_weight)). Hyper-parameters: exorl_agent_set_iql. update() draws no
                                  noise: the noise arguments are ignored and the Philox counter stays where it is. */
#define EXORL_AGENT_FQE    9   /* fitted Q evaluation, no reference file: a FROZEN actor (no gradient, no Adam pass, its weight images never
                                  rewritten) and a twin critic with its Polyak target in TD3's offline layout. One update regresses each net on
                                  its own target, y_i = r + D Q'_i(s', mu(s')), mu the actor's mean action: no min over the twins (an estimate,
                                  not a pessimistic bound; the two nets are a two-member ensemble). update() draws no noise, as IQL's. The
                                  policy's value is read with exorl_agent_fqe_value. */

/* kind 10 is unassigned and refused, as 7 is */
#define EXORL_AGENT_PRDC   11  /* policy regularisation with dataset constraint (Ran et al., ICML 2023), no reference file: TD3+BC with the BC target
                                  replaced by the action of the dataset point nearest to (beta s, mu(s)), searched exactly over the replay's key
                                  table on every step (exorl_replay_build_keys, exorl_agent_set_prdc):
                                  actor loss = -lambda mean(min Q(s, pi(s))) + mse(mu(s), a_nn), lambda = alpha / mean|Q|, a_nn a constant.
                                  Nets, critic step, noise and soft update are TD3+BC's. One process only: world_size > 1 is refused. */

#define EXORL_CRR_IDENTITY  0   /* crr.py:132-142 adv_transform */
#define EXORL_CRR_INDICATOR 1
#define EXORL_CRR_EXP       2

#define EXORL_PREC_F32  0      /* v_mfma_f32_32x32x2_f32: exact fp32 products, parity mode */
#define EXORL_PREC_BF16 1      /* v_mfma_f32_32x32x16_bf16: bf16 operands, fp32 accumulate, fp32 master weights */
#define EXORL_PREC_BF16X3 2    /* split-bf16: every GEMM operand x = hi + lo (two bf16), product = hi*hi + hi*lo + lo*hi on the bf16 MFMA,
                                  fp32 accumulate; everything else as EXORL_PREC_F32. ~2^-16 relative product error: per-step losses stay
                                  within the 1e-4 parity bar of the fp32 reference (tests/test_gpu_agent.py) at about twice fp32 mode's rate */
#define EXORL_PREC_BF16X6 3    /* three-plane split-bf16: x = hi + mid + lo, three bf16 planes = the 24 significand bits of fp32 held exactly;
                                  product = hi*hi + (hi*mid + mid*hi) + (hi*lo + lo*hi + mid*mid) on the bf16 MFMA, fp32 accumulate, the three
                                  dropped terms <= 3 * 2^-24 per product — fp32-grade products at 6 / 16 of the fp32 MFMA's cycles.
                                  Pixel agents and intrinsic modules: generic GEMMs and the 32-channel convolutions (forward, dgrad); the
                                  convolution weight gradients and the first layer run as in EXORL_PREC_F32.
                                  State agents (every kind): the pipeline of EXORL_PREC_F32 with the H x H products (forward, dgrad, wgrad) in
                                  three planes — on the 128 x 64 plane kernel (exorl_gemm_planes3's) when hidden_dim and batch are multiples
                                  of 128, else split inside the generic GEMM; first layer, LayerNorm, heads, losses and Adam are fp32 mode's. */

#define EXORL_NET_ACTOR         0
#define EXORL_NET_CRITIC        1
#define EXORL_NET_CRITIC_TARGET 2
#define EXORL_NET_VALUE         3   /* IQL only: Linear(O,H) LayerNorm Tanh Linear(H,H) ReLU Linear(H,1), keys net.{0,1,3,5}.{weight,bias} */

#define EXORL_T_PARAM 0
#define EXORL_T_GRAD  1
#define EXORL_T_ADAM_M 2
#define EXORL_T_ADAM_V 3

/* metrics[] layout written by exorl_agent_metrics (same keys as the reference's metrics dict) */
#define EXORL_M_BATCH_REWARD    0
#define EXORL_M_CRITIC_TARGET_Q 1
#define EXORL_M_CRITIC_Q1       2
#define EXORL_M_CRITIC_Q2       3
#define EXORL_M_CRITIC_LOSS     4
#define EXORL_M_ACTOR_LOSS      5
#define EXORL_M_ACTOR_LOGPROB   6
#define EXORL_M_Q_ABS_SUM       7   /* local sum |Q| (DP scalar all-reduce operand) */
#define EXORL_M_Q_SUM           8   /* local sum  Q  */
#define EXORL_M_BC_SUM          9   /* local sum (mu-a)^2 */
#define EXORL_M_CRITIC_CQL        10
#define EXORL_M_CRITIC_CQL_LOGSUM 11
#define EXORL_M_ACTOR_ALPHA       12
#define EXORL_M_ACTOR_ALPHA_LOSS  13
#define EXORL_M_ACTOR_ENT         14
/* EXORL_AGENT_IQL only: slots 10..13 carry IQL's own quantities (the four names above are CQL's and mean nothing for IQL). Slots 0..5 keep
 * their meaning, with critic_target_q = mean of y = r + D V(s'). */
#define EXORL_M_VALUE_LOSS   10   /* (1/Bg) sum k u^2, u = min Q'(s, a) - V(s), k = u < 0 ? 1 - expectile : expectile */
#define EXORL_M_VALUE        11   /* mean V(s) */
#define EXORL_M_ADV          12   /* mean u */
#define EXORL_M_ACTOR_WEIGHT 13   /* mean w */
/* EXORL_AGENT_PRDC only: slot 10 (CQL's and IQL's names above mean nothing for PRDC); slots 0..9 are TD3+BC's. */
#define EXORL_M_NN_DIST      10   /* mean over the batch of sqrt(d2) to the nearest key */
/* EXORL_AGENT_TD3_BC while ReBRAC is set (exorl_agent_set_rebrac) only: slots 10 and 11. Slots 0..9 are TD3+BC's, with critic_target_q the mean
 * of the penalised y and batch_reward the mean of the dataset's r (never of the corrected reward). */
#define EXORL_M_REBRAC_PENALTY 10 /* mean over the global batch of p = v sum_j (a~'_j - a'_j)^2, before critic_beta */
#define EXORL_M_REBRAC_VALID   11 /* mean of v, the share of rows whose episode holds the next action */
/* EXORL_AGENT_TD3_BC, _TD3, _CRR and _FQE while the SARSA setting is on (exorl_agent_set_sarsa) only: slot 11; the other slots are the kind's. */
#define EXORL_M_SARSA_VALID    11 /* mean over the global batch of v = next_valid, the share of rows whose target is at the dataset's a' */
/* EXORL_AGENT_CQL: slot 15. 0 unless Cal-QL is set on the handle (exorl_agent_set_calql). */
#define EXORL_M_CALQL_BOUND    15 /* mean over the global batch of (bounded policy-action entries of row b, both nets) / (4 n_samples) */
#define EXORL_N_METRICS        16

typedef struct {
    int32_t kind;
    int32_t obs_dim, act_dim, hidden_dim;
    int32_t batch;            /* rows per update on THIS rank */
    int32_t precision;        /* EXORL_PREC_* */
    int32_t world_size;       /* data-parallel ranks; losses are means over batch*world_size */
    int32_t sf_dim;           /* APS: successor-feature width (aps.yaml: 10); obs_dim includes it */
    float   lr, tau, alpha, stddev_clip;
    uint64_t seed;            /* Philox stream for action noise when no noise buffer is given */
    int32_t num_value_samples; /* CRR: actions sampled per state for V(s) (crr.yaml: 10) */
    int32_t weight_func;       /* CRR: EXORL_CRR_* */
    int32_t n_samples;         /* CQL: action samples per source (cql.yaml: 3); `alpha` is then the CQL penalty weight */
    int32_t use_critic_lagrange; /* CQL: learn the penalty weight (cql.py:201-213); data parallel through exorl_agent_update_phase 4 / 5 (exorl_agent_update does that itself when a communicator is set) */
    float   target_cql_penalty;  /* CQL Lagrange target (cql.yaml: 5.0) */
    int32_t reserved3;
} exorl_agent_cfg;

size_t exorl_agent_workspace_bytes(const exorl_agent_cfg* cfg);
/* workspace_dev: caller-allocated device memory of at least exorl_agent_workspace_bytes (e.g. a torch
 * tensor's data_ptr) or NULL to let the library hipMalloc it. Contents are zero-initialised. */
int exorl_agent_create(const exorl_agent_cfg* cfg, void* workspace_dev, size_t workspace_bytes,
                       exorl_agent_t** out);
int exorl_agent_destroy(exorl_agent_t* a);
/* Number of parameter tensors of a net, in the reference's nn.Module.parameters() order. */
int exorl_agent_num_tensors(exorl_agent_t* a, int32_t net, int32_t* n);
/* Device pointer + logical shape (rows x cols; cols = 1 for vectors) of one tensor. */
int exorl_agent_tensor(exorl_agent_t* a, int32_t net, int32_t index, int32_t what,
                       void** ptr_dev, int64_t* rows, int64_t* cols);
/* The flat (padded) buffer that holds all tensors of a net back to back: all-reduce operand. */
int exorl_agent_flat(exorl_agent_t* a, int32_t net, int32_t what, void** ptr_dev, int64_t* numel);
/* Must be called after parameters were written from outside (load_state_dict, init): refreshes derived
 * copies (bf16 shadows) and, if sync_target != 0, copies critic -> critic_target (td3_bc.py:93). */
int exorl_agent_params_changed(exorl_agent_t* a, int32_t sync_target, void* stream);
/* Where the sampler should write this agent's minibatch (zero-copy hand-off replay -> update). Every field is written: next_action /
 * next_valid point into the ReBRAC buffer or the SARSA buffer (next_action_stride = act_dim) while one is set (exorl_agent_set_rebrac,
 * exorl_agent_set_sarsa: the column's readers, never both on one handle), and are NULL otherwise. */
int exorl_agent_batch_slots(exorl_agent_t* a, exorl_batch_out* out);
/* Copies a caller-provided device batch (contiguous f32 (B,O) (B,A) (B) (B) (B,O)) into the batch slots. */
int exorl_agent_set_batch(exorl_agent_t* a, const float* obs_dev, const float* action_dev,
                          const float* reward_dev, const float* discount_dev, const float* next_obs_dev,
                          void* stream);
/* One gradient step on the batch currently in the batch slots.
 * noise_critic_dev / noise_actor_dev: (B,A) standard-normal draws (reference order; for CRR the second
 * draw is (B*num_value_samples, A), crr.py:125) or NULL for device Philox.
 * CQL (draw order cql.py:159,170-176,238): noise_critic_dev = [z_next (B,A) | u_rand (n,B,A) uniform(-1,1) | z_cur (n,B,A) |
 * z_nxt (n,B,A)] back to back, noise_actor_dev = z_actor (B,A). Runs phases 0..3 back to back (world_size 1). */
int exorl_agent_update(exorl_agent_t* a, float stddev, const float* noise_critic_dev,
                       const float* noise_actor_dev, void* stream);
/* One phase of the step, for the caller that runs the data-parallel exchanges itself. What each phase leaves ready:
 *   phase 0 -> critic grads             (BC: the staged inputs only, and phase 1 does nothing)
 *   phase 1 -> critic Adam + soft update done, actor-side Q statistics in the 4-float stats buffer
 *   phase 2 -> actor grads
 *   phase 3 -> actor Adam done
 *   phase 4 -> CQL, phase 0's first half: forwards done, this rank's penalty sums in the stats buffer
 *   phase 5 -> CQL, phase 0's second half: multiplier stepped from the global penalty (cql.py:199-213), critic grads
 *   phase 6 -> IQL: Q'(s,a), Q(s,a), V on [s'; s], the row kernel (dv, dq, w, metric sums), value grads
 *   phase 7 -> IQL: critic grads          phase 8 -> IQL: actor forward on s, actor grads
 *   phase 9 -> IQL: Adam on value, critic (+ soft update) and actor. IQL runs phases 6..9 only; the other kinds refuse them.
 *   phase 10 -> FQE: mu(s') on the next_obs rows, Q'(s', mu(s')), Q(s, a), the row kernel (dq, metric sums), critic grads
 *   phase 11 -> FQE: critic Adam (+ soft update). FQE runs phases 10 and 11 only; the other kinds refuse them.
 *   phase 12 -> PRDC, between phases 0 and 1: the queries [beta obs | mu(obs)], the search, a_nn gathered. PRDC's plan is 0, 12, 1, 2, 3.
 * Which phases a configuration's step runs, in which order, and which exchange follows each: exorl_agent_update_plan. Phase 0 is refused for
 * CQL with use_critic_lagrange and world_size > 1 (phases 4 and 5 stand for it). */
int exorl_agent_update_phase(exorl_agent_t* a, int32_t phase, float stddev, const float* noise_critic_dev,
                             const float* noise_actor_dev, void* stream);
/* The step as its phases: phases[i] is the i-th exorl_agent_update_phase id and exchanges[i] the sum all-reduce over the ranks that must
 * follow it before the next phase, or -1. Exchanges are named only for world_size > 1. Needs no device. Writes *n (<= 5) entries; fails,
 * writing nothing, when capacity is smaller. */
#define EXORL_AGENT_XCHG_CRITIC_GRAD 0   /* exorl_agent_flat(EXORL_NET_CRITIC, EXORL_T_GRAD) */
#define EXORL_AGENT_XCHG_STATS       1   /* exorl_agent_stats_buffer */
#define EXORL_AGENT_XCHG_ACTOR_GRAD  2   /* exorl_agent_flat(EXORL_NET_ACTOR, EXORL_T_GRAD) */
#define EXORL_AGENT_XCHG_VALUE_GRAD  3   /* exorl_agent_flat(EXORL_NET_VALUE, EXORL_T_GRAD): IQL, after phase 6 */
int exorl_agent_update_plan(const exorl_agent_cfg* cfg, int32_t* phases, int32_t* exchanges, int32_t capacity, int32_t* n);
int exorl_agent_stats_buffer(exorl_agent_t* a, void** ptr_dev, int64_t* numel);
/* Attach a communicator of cfg.world_size ranks (NULL detaches): exorl_agent_update then runs the four phases AND the all-reduces
 * between them on `stream` — no host round trip inside a step. The 16-byte statistic is reduced on a second stream while the critic's
 * backward pass runs (lambda enters only at the actor head: the critic backward is linear in its output gradient). */
int exorl_agent_set_comm(exorl_agent_t* a, exorl_comm_t* c);
/* CQL: entropy temperature state (log_actor_alpha and its Adam moments), host <-> device: host[0..2]; with
 * use_critic_lagrange also host[3..5] = log_critic_alpha and its Adam moments (pass a 6-float array). */
int exorl_agent_cql_alpha(exorl_agent_t* a, float* log_alpha_host, int32_t set);
/* IQL's hyper-parameters (at creation: expectile 0.7, temperature 3.0, max_weight 100.0). Refuses, in this order: expectile outside (0, 1),
 * temperature < 0 or max_weight <= 0 (or NaN); a null handle; a kind other than EXORL_AGENT_IQL; a handle with a captured graph (the graph
 * holds the values: disable it, set, capture again). */
int exorl_agent_set_iql(exorl_agent_t* a, float expectile, float temperature, float max_weight);
/* EXORL_AGENT_PRDC: bind the key table of `r`, built with this beta. Refuses another kind, a handle with a captured graph (the graph holds
 * the table's pointer, row count and key ranges), a replay without a valid table, a table whose observation / action split is not the
 * agent's and a table built with another beta. The number of key ranges is chosen here, from the table's rows, the batch and the CU count.
 * exorl_agent_update, exorl_agent_update_phase, exorl_agent_enable_graph and exorl_agent_step_graph refuse, launching nothing, while no
 * table is bound or the bound one is stale or was rebuilt; `r` must outlive the binding. */
int exorl_agent_set_prdc(exorl_agent_t* a, exorl_replay_t* r, float beta);
/* EXORL_AGENT_PRDC: the last search's results in the workspace, idx (batch) int32, d2 (batch) and a_nn (batch, act_dim) float32, and the
 * number of key ranges of the bound table (0: none bound). */
int exorl_agent_nn_result(exorl_agent_t* a, void** idx_dev, void** d2_dev, void** a_nn_dev, int32_t* splits);
/* ReBRAC (Tarasov et al., NeurIPS 2023) as a per-handle setting of EXORL_AGENT_TD3_BC: the critic target gains a penalty on the distance
 * between the clipped target-policy sample a~' and the action a' the dataset took at s',
 *   y = r + D (min_i Q'_i(s', a~') - critic_beta p),   p = v sum_j (a~'_j - a'_j)^2,   v = next_valid,
 * formed as a per-row correction of the reward, r~ = r - D (critic_beta p) in fp32 in that order (p = v s with s summed over j ascending),
 * which every reader of the reward in the critic step then reads: one more row kernel per step, the plan stays 0, 1, 2, 3 and no exchange
 * is added under data parallelism. critic_beta = 0, and v = 0 on a row, leave that row's step TD3+BC's bit for bit. The actor loss
 * beta_a sum_j (pi(s) - a)^2 - Q / mean|Q| is TD3+BC's times beta_a act_dim with cfg.alpha = 1 / (beta_a act_dim).
 * The buffer is the caller's device memory, exorl_agent_rebrac_bytes(cfg) bytes, 256-byte aligned, alive while set: four runs, each padded
 * to 64 floats, next_action (batch, act_dim), next_valid (batch), r~ (batch) and the row kernel's per-chunk sums
 * [exorl_iql_rows_chunks(batch)][3]; r~ and the sums are written before they are read on every step. exorl_agent_rebrac_bytes needs no
 * device and returns 0, with exorl_last_error set, for another kind and for every configuration exorl_agent_create refuses.
 * exorl_agent_set_rebrac refuses, launching nothing: a null handle; another kind; a handle with a captured graph (the graph holds
 * critic_beta and the pointers); and, attaching, critic_beta < 0 or NaN; a handle with a metric window or an eval window attached; a buffer
 * too small or misaligned. buf_dev NULL detaches, whatever bytes and critic_beta are: the handle is TD3+BC again. While set, exorl_agent_batch_slots hands out the buffer's next_action / next_valid,
 * exorl_agent_set_batch leaves them to the caller, and exorl_agent_set_metric_window, exorl_agent_set_eval and exorl_agent_evaluate refuse. */
size_t exorl_agent_rebrac_bytes(const exorl_agent_cfg* cfg);
int exorl_agent_set_rebrac(exorl_agent_t* a, void* buf_dev, size_t bytes, float critic_beta);
/* The SARSA target as a per-handle setting of EXORL_AGENT_TD3_BC, _TD3, _CRR (critic step in phase 0) and _FQE (phase 10): the critic learns
 * Q^beta, the behaviour policy's value, from the dataset's own (s, a, r, s', a'). One-step RL (Brandfonbrener et al., NeurIPS 2021) is this
 * critic under the kind's unchanged actor step; on FQE it is behaviour Q evaluation. With v = next_valid, the action fed to the target critic
 * at s' is the dataset's a' where v != 0 and the kind's own target action where v = 0 (the sample's n steps end the episode there and the
 * dataset holds no a'): TD3's clipped sample a~', FQE's mu(s'). One row kernel, launched behind the launch that writes the kind's own action
 * and ahead of the critics' forward, copies a' over the action columns of the target critic's input on the rows with v != 0: a bit-exact
 * masked copy, one more launch per step (and one single-wave sums launch on a step whose metrics are read), no other kernel changes, the plan
 * stays the kind's and data parallelism needs no new exchange (the rule is per row). A row with v = 0 is the base kind's row bit for bit and
 * a batch of them its step; with v = 1 on every row the critic's trajectory does not depend on the actor. The copy is a launch of its own and
 * not part of the actor head's sample epilogue, which TD3+BC's step keeps as it is, bits and launch count.
 * The buffer is the caller's device memory, exorl_agent_sarsa_bytes(cfg) bytes (the same at every precision and world_size), 256-byte
 * aligned, alive while set: three runs, each padded to 64 floats, next_action (batch, act_dim), next_valid (batch) and the row kernel's
 * per-chunk sums [exorl_iql_rows_chunks(batch)][1], written before they are read on every step. exorl_agent_sarsa_bytes needs no device and
 * returns 0, with exorl_last_error set, for another kind and for every configuration exorl_agent_create refuses.
 * exorl_agent_set_sarsa refuses, launching nothing: a null handle; another kind; a handle with a captured graph (the graph holds the
 * pointers); and, attaching, a handle with ReBRAC set, a metric window or an eval window attached; a buffer too small or misaligned. buf_dev
 * NULL detaches, whatever bytes is: the handle is the base kind again. While set, exorl_agent_batch_slots hands out the buffer's next_action /
 * next_valid, exorl_agent_set_batch leaves them to the caller, exorl_agent_set_rebrac, exorl_agent_set_metric_window, exorl_agent_set_eval and
 * exorl_agent_evaluate refuse, and exorl_agent_fqe_value reads Q(s, a) at the obs and action slots (the critic on its own input rows, no actor
 * forward): Q^beta(s0, a0) when the slots hold episode starts. */
size_t exorl_agent_sarsa_bytes(const exorl_agent_cfg* cfg);
int exorl_agent_set_sarsa(exorl_agent_t* a, void* buf_dev, size_t bytes);
/* Cal-QL (Nakamoto et al., NeurIPS 2023) as a per-handle setting of EXORL_AGENT_CQL: in the conservative penalty the critic's value on the
 * policy actions, entries k in [n, 3n) of a row (the actions of pi(s) and pi(s') evaluated at s), enters as q^ = (q >= m_b) ? q : m_b with
 * m_b = mc_return[b], the dataset's Monte-Carlo return-to-go of the row (exorl_replay_build_returns, exorl_replay_sample_mc). The row
 * maximum, the exponent sum, lse and the penalty use q^; dq of a bounded entry is +0, every other dq keeps its formula with q^ inside the
 * softmax; the random entries, the data entry, y, the mse and the Lagrange step are CQL's, in all three modes of the critic kernel (under
 * data parallelism the mode-1 sums are sums of q^ terms; the bound is per row and needs no exchange). No launch is added: the plan and the
 * dispatch count are CQL's. With the setting off, or on with m = -inf everywhere, the step is CQL's bit for bit. m is a lower bound on the
 * value of the behaviour only where an episode's recorded remainder is one (see exorl_replay_build_returns).
 * The buffer is the caller's device memory, exorl_agent_calql_bytes(cfg) bytes (4 * batch rounded up to 64 floats, the same at every
 * precision and world_size), 256-byte aligned: mc_return (batch), which the sampler or the caller writes before every step.
 * exorl_agent_calql_bytes needs no device and returns 0 (exorl_last_error set) for another kind or a configuration exorl_agent_create
 * refuses. exorl_agent_set_calql refuses, launching nothing: a null handle; another kind; a handle with a captured graph (the graph holds the
 * pointer); when attaching, a metric window or eval buffer already attached; a buffer too small or misaligned. A NULL buffer detaches.
 * While set, exorl_agent_set_metric_window, exorl_agent_set_eval and exorl_agent_evaluate refuse; exorl_agent_enable_graph hands the buffer to
 * the captured gather and refuses a replay without a valid column at its gamma; exorl_agent_step_graph refuses once the column is stale. */
size_t exorl_agent_calql_bytes(const exorl_agent_cfg* cfg);
int exorl_agent_set_calql(exorl_agent_t* a, void* buf_dev, size_t bytes);
/* Policy inference for n rows: out = mean (eval) or TruncatedNormal sample (clip=None). */
int exorl_agent_act(exorl_agent_t* a, const float* obs_dev, int32_t n, float stddev, int32_t eval_mode,
                    const float* noise_dev, float* action_out_dev, void* stream);
/* The same for the online loop's one observation per environment step (pretrain.py:271-283 -> ddpg.py:221-238 / td3_bc.py:107-117): obs_host
 * (n <= 2 rows) and noise_host (or NULL -> device Philox) are HOST pointers copied into the kernel arguments, `action_out` is any
 * device-accessible address — pinned host memory makes the result visible after a stream synchronise with no copy. One kernel launch, no other
 * device work. Not for CQL's tanh-Gaussian policy (exorl_agent_act handles it). */
int exorl_agent_act_host(exorl_agent_t* a, const float* obs_host, int32_t n, float stddev, int32_t eval_mode,
                         const float* noise_host, float* action_out, void* stream);
/* Synchronous: copies the metric block of the last update to host. */
int exorl_agent_metrics(exorl_agent_t* a, float* metrics_host, void* stream);
/* The reference computes its metrics dict only under use_tb (td3_bc.py:133,162,175); enable = 0 skips the metric
 * reductions of the step (default: enabled). */
int exorl_agent_set_metrics(exorl_agent_t* a, int32_t enable);
/* Windowed metrics: every whole step (exorl_agent_update, exorl_agent_step_graph) ends in one kernel that writes the step's metrics to the
 * EXORL_M_* slots (exorl_agent_metrics still returns the last step's) and adds each slot to a window of double sums with an int64 step count,
 * all in device memory: nothing is copied to the host until the window is read. TD3+BC, TD3 and DDPG then stay on the fused scalar-head path,
 * whose kernels leave the metrics' per-chunk sums behind; the other kinds run the metric kernels they run under exorl_agent_set_metrics(1).
 * The buffer is the caller's: exorl_agent_metric_window_bytes(cfg) bytes of device memory, 256-byte aligned, alive while it is set; NULL
 * switches the mode off. Refused while a graph is captured (set the window first: the capture then holds its kernels) and for
 * world_size > 1. */
size_t exorl_agent_metric_window_bytes(const exorl_agent_cfg* cfg);
int exorl_agent_set_metric_window(exorl_agent_t* a, void* buf_dev, size_t bytes);
/* Synchronous: sums_host[EXORL_N_METRICS] and *steps_host = the window since the last reset (mean of slot i = sums_host[i] / *steps_host).
 * One copy and, with reset != 0, one hipMemsetAsync, both enqueued on `stream`: they order against the graph replays on it. */
int exorl_agent_metric_window_read(exorl_agent_t* a, double* sums_host, int64_t* steps_host, int32_t reset, void* stream);
/* Held-out validation: a forward-only pass over the networks, for TD3+BC, TD3, CRR, CQL and BC (every other kind is refused). Nothing is
 * sampled, no Philox draw is made and no counter moves; mu is the policy's mean action (tanh of the head; CQL: tanh of the first act_dim of
 * its 2 act_dim outputs), y = reward + discount * min_i Q'_i(s', mu(s')) the noise-free target. One call adds, over the rows of the batch,
 * to a window of double sums: */
#define EXORL_E_BC_SQ     0   /* sum over rows and action columns of (mu(s) - a)^2 */
#define EXORL_E_Q_DATA    1   /* sum of min_i Q_i(s, a) */
#define EXORL_E_Q_PI      2   /* sum of min_i Q_i(s, mu(s)) */
#define EXORL_E_Q1_ERR    3   /* sum of (Q_1(s, a) - y)^2 */
#define EXORL_E_Q2_ERR    4   /* sum of (Q_2(s, a) - y)^2 */
#define EXORL_E_TARGET_Q  5   /* sum of y */
#define EXORL_E_ROWS      6   /* rows in the window */
#define EXORL_N_EVAL      7
/* Bytes of the window and its per-chunk partials for a configuration (0 for one exorl_agent_create refuses). Needs no device. */
size_t exorl_agent_eval_bytes(const exorl_agent_cfg* cfg);
/* Attach the window: exorl_agent_eval_bytes(cfg) bytes of the caller's device memory, 256-byte aligned, alive while it is set; the call
 * empties it. NULL detaches. The buffer is the caller's, as the metric window is: the agent workspace keeps its size and layout. */
int exorl_agent_set_eval(exorl_agent_t* a, void* buf_dev, size_t bytes);
/* One forward-only pass on the cfg.batch rows currently in the batch slots (exorl_agent_batch_slots / exorl_agent_set_batch), through the
 * step's own forward kernels in the agent's precision, then one row kernel and a one-wave kernel that adds the per-chunk partials to the window
 * in chunk order (the sums are bitwise reproducible). BC runs the actor alone and adds to EXORL_E_BC_SQ and EXORL_E_ROWS only.
 * Read-only towards everything a step leaves behind or reads: parameters, targets, weight images, gradients, Adam moments, the step state,
 * the metrics and their window, the statistics, CQL's scalars and exorl_agent_act's buffers. It writes the staged network inputs, the
 * scratch a whole step writes before it reads (what exorl_debug_agent_poison_scratch fills) and its own window. Eager launches on `stream`:
 * it may run between exorl_agent_update or exorl_agent_step_graph calls on that stream, and must NOT be called between the phases of a step
 * driven through exorl_agent_update_phase (the phases hand their activations to each other in that scratch). */
int exorl_agent_evaluate(exorl_agent_t* a, void* stream);
/* Synchronous: sums_host[EXORL_N_EVAL] and *rows_host = the window since the last reset (val mean of slot i = sums_host[i] / *rows_host).
 * One copy and, with reset != 0, one hipMemsetAsync, both enqueued on `stream`. */
int exorl_agent_eval_read(exorl_agent_t* a, double* sums_host, int64_t* rows_host, int32_t reset, void* stream);
/* EXORL_AGENT_FQE only: the value pass. Forward-only on the first `rows` (1 <= rows <= cfg.batch) of the obs rows in the batch slots: the actor's
 * mean action mu(s), then both critics at (s, mu(s)), through the step's own forward kernels; then a row kernel and a one-wave kernel add, in
 * chunk order (bitwise reproducible, no atomics, fp64 from the rows on), to a window of double sums: */
#define EXORL_FQE_V_Q1       0   /* sum of Q_1(s, mu(s)) */
#define EXORL_FQE_V_Q2       1   /* sum of Q_2(s, mu(s)) */
#define EXORL_FQE_V_MEAN_SQ  2   /* sum of ((Q_1 + Q_2) / 2)^2 */
#define EXORL_FQE_V_DIFF_SQ  3   /* sum of (Q_1 - Q_2)^2 */
#define EXORL_FQE_V_ROWS     4   /* rows in the window */
#define EXORL_N_FQE_VALUE    5
/* The window is the caller's, as the eval window is: exorl_agent_fqe_value_bytes(cfg) bytes of device memory (0 for a configuration that is
 * refused or not FQE), 256-byte aligned, alive while it is set; setting empties it, NULL detaches. The pass reads the action, reward, discount and
 * next_obs slots only to stage them (rows >= `rows` and those slots may hold anything, NaN included: nothing of them reaches the sums) and is
 * read-only towards parameters, targets, weight images, gradients, Adam moments, the step state and the metrics: exorl_agent_update or
 * exorl_agent_step_graph afterwards continue bit for bit. Not between the phases of a step driven through exorl_agent_update_phase.
 * While the SARSA setting is on (exorl_agent_set_sarsa) the pass runs no actor forward: both critics at (s, a) of the obs AND action slots,
 * rows < `rows` of both then being read, into the same sums (Q_i(s, a) for Q_i(s, mu(s))). */
size_t exorl_agent_fqe_value_bytes(const exorl_agent_cfg* cfg);
int exorl_agent_set_fqe_value(exorl_agent_t* a, void* buf_dev, size_t bytes);
int exorl_agent_fqe_value(exorl_agent_t* a, int32_t rows, void* stream);
/* Synchronous: sums_host[EXORL_N_FQE_VALUE] and *rows_host = the window since the last reset; with reset != 0 one hipMemsetAsync on `stream`. */
int exorl_agent_fqe_value_read(exorl_agent_t* a, double* sums_host, int64_t* rows_host, int32_t reset, void* stream);
/* Captured graphs run independent parts of the step (target || critic forward, wgrad || dgrad chain) as parallel
 * branches on a second stream (default: off — one chain measured faster on MI355X). */
int exorl_agent_set_parallel_branches(exorl_agent_t* a, int32_t enable);
/* IQL's value net always steps with the critic: critic_steps is its Adam step count too. */
int exorl_agent_opt_steps(exorl_agent_t* a, int64_t* actor_steps, int64_t* critic_steps);
int exorl_agent_set_opt_steps(exorl_agent_t* a, int64_t actor_steps, int64_t critic_steps);
/* Captures exorl_replay_sample(PHILOX) into the agent's batch slots + exorl_agent_update into one hipGraph;
 * exorl_agent_step_graph replays it (all per-step counters, Adam scalars and the exploration std live in device memory, so a
 * stddev schedule — utils.schedule, td3_bc.py:169 — that moves every step costs one scalar write, not a re-capture).
 * enable_graph synchronises `stream` (the caller's stream, where earlier steps may still run) before touching anything and does not
 * consume a Philox batch. step_graph launches on `stream`; stddev is the schedule's value for this step. */
int exorl_agent_enable_graph(exorl_agent_t* a, exorl_replay_t* r, int32_t nstep, float gamma, float stddev, void* stream);
/* exorl_agent_enable_graph on a replay with a goal rule (exorl_replay_set_goal): captures exorl_replay_sample_goal(PHILOX) into the agent's
 * [obs | g] batch slots (g at column O of the obs and next_obs rows), then the step on those rows. Requires the replay's O + n_cols ==
 * cfg.obs_dim. exorl_agent_step_graph refuses to replay the graph once exorl_replay_set_goal was called after the capture. */
int exorl_agent_enable_graph_goal(exorl_agent_t* a, exorl_replay_t* r, int32_t nstep, float gamma, float stddev, void* stream);
int exorl_agent_step_graph(exorl_agent_t* a, float stddev, void* stream);
int exorl_agent_disable_graph(exorl_agent_t* a);
/* Test hooks for the device-side noise stream (synchronous): the Philox draw counter after the steps enqueued so far, and the
 * standard-normal block the update kernels generate for (seed, counter) — out[e], e = row * act_dim + column. With these a test
 * can replay a captured-graph trajectory (device sampler + device noise) through the CPU oracle. */
int exorl_agent_noise_counter(exorl_agent_t* a, uint64_t* counter_out, void* stream);
int exorl_debug_philox_normal(uint64_t seed, uint64_t counter, int64_t n, float* out_dev, void* stream);
/* Diagnostic only: fills with 0xFF bytes (NaN as fp32 and as bf16) every workspace sub-buffer that a step writes before it reads — the
 * staged inputs, activations, backward buffers, per-chunk partials, per-row loss gradients and weights — and the alignment padding
 * behind every sub-buffer. Parameters, gradients, optimiser state, weight shadows, step state, CQL scalars, batch slots, statistics,
 * metrics and act()'s scratch keep their contents. A step after this call must give bit-identical results: anything else is a read of
 * memory the step did not write. Enqueued on `stream`. */
int exorl_debug_agent_poison_scratch(exorl_agent_t* a, void* stream);
/* The derived weight images of one net. The kernels do not read the first-layer weight W0 ([H][in] per trunk) and the H x H weight W1 (per
 * head) from the fp32 parameters but from copies of them in the workspace, which every writer of the parameters keeps equal, bit for bit,
 * to the image of the current fp32 value x:
 *   w0t                     W0 transposed, fp32 [n_trunks][in][H]: the value itself
 *   hi                      bf16(x), round to nearest even
 *   lo  (two-plane image)   bf16(x - hi)
 *   mid, lo (three planes)  mid = bf16(x - hi), lo = bf16(x - hi - mid); the differences are formed in fp32, where they are exact
 *   w0_hi / w0_lo           [n_trunks][H][round_up(in, 32)]: columns in .. round_up(in, 32) - 1 of every row are zero
 *   w1_hi / w1_mid / w1_lo  [n_heads][H][H]
 * Which images a configuration has (a pointer is NULL where it has none; w0t always exists):
 *   EXORL_PREC_BF16                                                                   w0_hi, w1_hi
 *   EXORL_PREC_BF16X3, hidden_dim % 128 == 0 and batch % 64 == 0 (the plane pipeline)  w0_hi, w0_lo, w1_hi, w1_lo
 *   EXORL_PREC_BF16X6, hidden_dim % 128 == 0 and batch % 128 == 0 (the plane route)    w1_hi, w1_mid, w1_lo; none of W0
 *   everything else (fp32; bf16x3 / bf16x6 at other shapes: the GEMM splits fp32)     none
 * Written by exorl_agent_params_changed, by the optimiser launch of every step route (for the critic also the Polyak target's) and, three
 * planes, by a conversion pass behind it. Inside the library this layout is stated once, by the index and size functions next to
 * WeightImages in exorl_amd/csrc/kernels.h, and the planes' values by bf16_bits / bf16_lo_bits / bf16_residual in csrc/numerics.h. */
typedef struct {
    int32_t n_trunks, n_heads, in_dim, hidden_dim;
    float* w0t;
    uint16_t *w0_hi, *w0_lo;
    uint16_t *w1_hi, *w1_mid, *w1_lo;
} exorl_weight_images;
/* Diagnostic only: the derived weight copies of one net (EXORL_NET_*), device pointers into the workspace, NULL where the configuration
 * carves none. Launches nothing and synchronises nothing: the caller orders its reads behind the steps it enqueued. */
int exorl_debug_agent_weight_images(exorl_agent_t* a, int32_t net, exorl_weight_images* out);

/* ------------------------------------------------------------------------------------------------
 * Stand-alone operators (used by the agents above; exported for tests and for callers' own nets)
 * ---------------------------------------------------------------------------------------------- */
/* C[M,N] = op(A) * op(B) (+bias[N]) (ReLU) (C +=), fp32 in memory.
 * a_layout: 0 = A stored [M][K] (lda >= K), 1 = A stored [K][M] (lda >= M)
 * b_layout: 0 = B stored [N][K] (ldb >= K)  (nn.Linear weight), 1 = B stored [K][N] (ldb >= N) */
int exorl_gemm(int32_t precision, int32_t a_layout, int32_t b_layout, int32_t M, int32_t N, int32_t K,
               const float* A_dev, int64_t lda, const float* B_dev, int64_t ldb, float* C_dev, int64_t ldc,
               const float* bias_dev, int32_t relu, int32_t accumulate, void* stream);
/* Same with A and B stored as bf16 in memory (the fast mode's operand format); fp32 accumulate and output. */
int exorl_gemm_bf16(int32_t a_layout, int32_t b_layout, int32_t M, int32_t N, int32_t K, const uint16_t* A_dev, int64_t lda,
                    const uint16_t* B_dev, int64_t ldb, float* C_dev, int64_t ldc, const float* bias_dev, int32_t relu,
                    int32_t accumulate, void* stream);
/* Grouped form on bf16 planes, as the agents launch it: up to 4 problems of one shape in ONE launch, each operand given as a hi plane and
 * (split-bf16) a lo plane with x = hi + lo, or lo == NULL for plain bf16. a_layouts[i] selects problem i's A layout (a Linear's wgrad
 * and dgrad share a launch with different A layouts); b_layout is common. No bias. Pointer arrays are host arrays of device pointers. */
int exorl_gemm_planes(int32_t count, const int32_t* a_layouts, int32_t b_layout, int32_t M, int32_t N, int32_t K,
                      const uint16_t* const* A_hi_dev, const uint16_t* const* A_lo_dev, int64_t lda,
                      const uint16_t* const* B_hi_dev, const uint16_t* const* B_lo_dev, int64_t ldb,
                      float* const* C_dev, int64_t ldc, int32_t relu, void* stream);
/* The same on three planes per operand (EXORL_PREC_BF16X6's arithmetic): x = hi + mid + lo with hi = bf16(x), mid = bf16(x - hi),
 * lo = bf16(x - hi - mid); C = hi*hi + (hi*mid + mid*hi) + (hi*lo + lo*hi + mid*mid), three fp32 accumulators summed small-first. One kernel
 * (128 x 64 tiles): M % 128 = 0, N % 64 = 0, K % 128 = 0, 16-byte aligned planes and C, lda and ldb multiples of 8, ldc a multiple of 4; every
 * problem of a launch has the same A layout (there is no mixed wgrad + dgrad form); anything else is an error, nothing is launched. */
int exorl_gemm_planes3(int32_t count, const int32_t* a_layouts, int32_t b_layout, int32_t M, int32_t N, int32_t K,
                       const uint16_t* const* A_hi_dev, const uint16_t* const* A_mid_dev, const uint16_t* const* A_lo_dev, int64_t lda,
                       const uint16_t* const* B_hi_dev, const uint16_t* const* B_mid_dev, const uint16_t* const* B_lo_dev, int64_t ldb,
                       float* const* C_dev, int64_t ldc, int32_t relu, void* stream);
/* Reference-path switches for tests and A/B runs; -1 or 0 = defaults. Bits (any combination):
 *   64          32 -> 32 convolution weight gradient on the tile kernel instead of the wave-specialised one
 *   256         act() on the generic multi-launch path
 *   8388608     wave-specialised convolution forward / dgrad: one image per workgroup instead of the persistent form
 *   134217728   planes adapter: ragged output widths through the padded copy
 *   1073741824  32 -> 32 convolution forward / dgrad on the strip kernel instead of the wave-specialised one */
int exorl_gemm_tune(int32_t variant);
/* Diagnostic only (tools/debug/config4_ablation.py): in EXORL_PREC_BF16X3 mode, run the selected product families with exact fp32 products.
 * bits 1/2 forward GEMM narrow/wide, 4/8 wgrad, 16/32 dgrad ("wide": a dimension >= 8192), 64/128/256 convolution forward/dgrad/wgrad.
 * No reference counterpart; the product never calls it. */
int exorl_debug_precision_override(int32_t mask);
/* Measurement hook (bench.py roofline leg): time every GEMM launch with HIP events on its own stream. */
int exorl_profile_gemm(int32_t enable);
int exorl_profile_gemm_read(double* flops_out_host, float* ms_out_host, int32_t cap, int32_t* n_out);
int exorl_profile_event_overhead(float* ms_out_host, void* stream);
int exorl_adam_step(float* p_dev, const float* g_dev, float* m_dev, float* v_dev, int64_t n, float lr,
                    float beta1, float beta2, float eps, int64_t t, float* target_dev, float tau, void* stream);
int exorl_soft_update(const float* p_dev, float* target_dev, int64_t n, float tau, void* stream);
int exorl_ln_tanh_fwd(const float* z_dev, const float* gain_dev, const float* beta_dev, float* h_dev,
                      float* xhat_dev, float* rstd_dev, int32_t rows, int32_t H, void* stream);
/* kNN particle-entropy building block: out[i][j] = j-th smallest L2 distance from src row i to the tgt rows (sorted). n_tgt <= 8192,
 * k <= 64; up to 4096 targets a wave holds a row of distances in LDS, above it walks the row in fixed chunks with a running top-k. */
int exorl_knn_topk(const float* src_dev, int32_t n_src, const float* tgt_dev, int32_t n_tgt, int32_t dim,
                   int32_t k, float* out_dev, void* stream);
/* Exact nearest neighbour of every query row among n key rows (PRDC's search on caller-made rows): keys (n, pitch) and queries (rows, q_ld)
 * float32, the first `dim` columns of each count (dim <= 512; key columns past dim are not read as data). idx_out[i] (int32) = argmin_j d2(i, j),
 * d2_out[i] = that minimum, d2 = sum_c (q_c - k_c)^2 in the difference form, fp32, columns ascending in one accumulator per pair: its bits do
 * not depend on how the work is split. Ties go to the lowest key index; a query equal to a key row returns exactly 0.0. The keys are cut
 * into `splits` contiguous ranges (0: the library's choice from n, rows and the CU count; at most 256, never an empty one), a first launch
 * leaves one (d2, index) per (query, range) and a second merges them in range order: the results are the same bits for every value of
 * `splits`, and no atomics are used. Library-owned scratch, grown outside captures. */
int exorl_nn_search(const float* keys_dev, int64_t n, int32_t pitch, int32_t dim, const float* queries_dev, int64_t q_ld, int32_t rows,
                    int32_t splits, int32_t* idx_out_dev, float* d2_out_dev, void* stream);
/* IQL's row kernel on caller-made rows (unit test hook): tq, q (2, rows) target and critic heads, v = V(s), v_next = V(s'), reward, discount
 * (rows) in; dv (rows), dq (2, rows), w (rows) out as the step forms them (EXORL_AGENT_IQL above), and sums[10] = the sums over the rows of
 * r, y, Q_1, Q_2, (Q_1 - y)^2, (Q_2 - y)^2, k u^2, v, u, w, added per chunk in chunk order with no atomics (the same bits on every run).
 * part: scratch of 10 * exorl_iql_rows_chunks(rows) floats. */
int32_t exorl_iql_rows_chunks(int32_t rows);
/* FQE's row kernel on caller-made rows (unit test hook): tq, q (2, rows) target and critic heads, reward, discount (rows) in; dq (2, rows) =
 * 2 inv_bg (Q_i - y_i), y_i = r + D Q'_i, out as the step forms them (EXORL_AGENT_FQE above), and sums[6] = the sums over the rows of r,
 * (y_1 + y_2) / 2, Q_1, Q_2, (Q_1 - y_1)^2, (Q_2 - y_2)^2, added per chunk in chunk order with no atomics (the same bits on every run).
 * part: scratch of 6 * exorl_fqe_rows_chunks(rows) floats. */
int32_t exorl_fqe_rows_chunks(int32_t rows);
int exorl_fqe_rows(const float* tq_dev, const float* q_dev, const float* reward_dev, const float* discount_dev, int32_t rows, float inv_bg,
                   float* dq_dev, float* part_dev, float* sums_dev, void* stream);
int exorl_iql_rows(const float* tq_dev, const float* q_dev, const float* v_dev, const float* v_next_dev, const float* reward_dev,
                   const float* discount_dev, int32_t rows, float inv_bg, float expectile, float temperature, float max_weight,
                   float* dv_dev, float* dq_dev, float* w_dev, float* part_dev, float* sums_dev, void* stream);
/* ReBRAC's row kernel on caller-made rows (unit test hook): sample (rows, act_dim at pitch sample_ld) the clipped target-policy sample,
 * next_action (rows, act_dim at pitch next_action_stride), next_valid, reward, discount (rows) in; reward_out (rows) = r - D (critic_beta p),
 * p = next_valid sum_j (sample_j - next_action_j)^2, as the step forms it (exorl_agent_set_rebrac above), and sums[3] = the sums over the rows
 * of p, next_valid and r, added per chunk in chunk order with no atomics (the same bits on every run). 1 <= act_dim <= 16; inv_bg is unused by
 * the raw sums. part: scratch of 3 * exorl_iql_rows_chunks(rows) floats. */
int exorl_rebrac_rows(const float* sample_dev, int64_t sample_ld, const float* next_action_dev, int64_t next_action_stride,
                      const float* next_valid_dev, const float* reward_dev, const float* discount_dev, int32_t rows, int32_t act_dim,
                      float critic_beta, float inv_bg, float* reward_out_dev, float* part_dev, float* sums_dev, void* stream);
/* The SARSA setting's row kernel on caller-made rows (unit test hook): next_action (rows, act_dim at pitch next_action_stride) and next_valid
 * (rows) in; dst (rows, act_dim at pitch dst_ld) takes next_action's row where next_valid != 0 and keeps its own elsewhere, bit for bit, and
 * nothing of dst outside those act_dim columns is written (dst_ld = obs_dim + act_dim with dst at the action columns in the step); sums[1] =
 * the sum of next_valid, added per chunk in chunk order with no atomics. 1 <= act_dim <= 16; inv_bg is unused by the raw sum. part: scratch of
 * exorl_iql_rows_chunks(rows) floats. */
int exorl_next_action_rows(const float* next_action_dev, int64_t next_action_stride, const float* next_valid_dev, int32_t rows, int32_t act_dim,
                           float inv_bg, float* dst_dev, int64_t dst_ld, float* part_dev, float* sums_dev, void* stream);
/* CQL's critic loss-gradient kernel on caller-made rows, one process, a fixed alpha and no multiplier (unit test hook). q_all (2, (3n + 1) B):
 * per net the entries k = 0 .. 3n of sample b at [k B + b], k < n random actions, n <= k < 3n policy actions, k = 3n the data action; tq (2, B)
 * the target critics at s'; reward, discount (B); mc_or_null (B) Cal-QL's bound or NULL for CQL. Writes dq_all_out (the shape of q_all, every
 * element) and metrics_out (EXORL_N_METRICS floats: the slots the critic kernel owns). Per row and net, in this order: mx = the maximum over
 * the data entry then k ascending; se = exp(q_data - mx) + sum over k ascending of exp(q^_k - mx); lse = log(se) + mx. */
int exorl_cql_dq_rows(const float* q_all_dev, const float* tq_dev, const float* reward_dev, const float* discount_dev, const float* mc_or_null_dev,
                      int32_t B, int32_t n, float alpha, float inv_bg, float* dq_all_out_dev, float* metrics_out_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Intrinsic-reward modules of the reward-free DDPG-backbone agents (states observations).
 * Replaces, per update() of the reference agent: the module's optimiser step and compute_intr_reward
 *   RND      agents/unsupervised_learning/rnd.py:79-108   (module rnd.py:13-60)
 *   ICM      agents/unsupervised_learning/icm.py:64-92    (module icm.py:12-45)
 *   ICM-APT  agents/unsupervised_learning/icm_apt.py:86-110 (module icm_apt.py:13-57; utils.PBE/RMS utils/utils.py:257-319)
 * The DDPG critic/actor update that follows is exorl_agent_update on the same batch with reward_out as its reward.
 * ------------------------------------------------------------------------------------------- */
#define EXORL_INTR_RND     0
#define EXORL_INTR_ICM     1
#define EXORL_INTR_ICM_APT 2
#define EXORL_INTR_DISAGREEMENT 3   /* agents/unsupervised_learning/disagreement.py:11-90 */
#define EXORL_INTR_DIAYN   4        /* agents/unsupervised_learning/diayn.py:15-127 */
#define EXORL_INTR_PROTO   5        /* agents/unsupervised_learning/proto.py:14-207 (state observations) */
#define EXORL_INTR_APS     6        /* agents/unsupervised_learning/aps.py:63-79,147-175 (the task rides in `skill`) */
#define EXORL_INTR_SMM     7        /* agents/unsupervised_learning/smm.py:27-112,173-246 (states; obs rows are [obs | z], z also in `skill`) */
#define EXORL_MAX_ENSEMBLE 8
#define EXORL_INTR_ENCODED 1       /* exorl_intr_cfg.flags */

typedef struct exorl_intr_cfg {
    int32_t kind;         /* EXORL_INTR_* */
    int32_t obs_dim, act_dim, hidden_dim;
    int32_t rep_dim;      /* rnd_rep_dim / icm_rep_dim / DIAYN skill_dim / APS sf_dim (unused by plain ICM and Disagreement) */
    int32_t batch;
    int32_t precision;    /* EXORL_PREC_* (MFMA operand type of the module's GEMMs) */
    int32_t knn_k, knn_avg, knn_rms;   /* ICM-APT: utils.PBE arguments (configs/agent/icm_apt.yaml) */
    int32_t n_models;     /* Disagreement ensemble size (0 -> 5, disagreement.py:12) */
    int32_t flags;        /* EXORL_INTR_ENCODED: the observation rows are encodings of pixel frames (obs_type == 'pixels') — SMM drops the goal prior
                             p*(s) from its reward (smm.py:232-235); RND takes the rows as already normalised (BatchNorm2d ran on the frames,
                             rnd.py:26-27,47-50) and feeds its frozen target net from next_obs, the frozen encoder copy's output (rnd.py:35-39) */
    float lr;             /* Adam, betas (0.9, 0.999), eps 1e-8 */
    float scale;          /* rnd_scale / icm_scale */
    float knn_clip;
    float clip_val;       /* RND: clamp of the BatchNorm-normalised observation (rnd.py:22, 5.0) */
    /* Proto (configs/agent/proto.yaml): rep_dim = pred_dim, hidden_dim = proj_dim, knn_k = topk */
    int32_t num_protos, queue_size;
    float tau;            /* softmax / Sinkhorn temperature */
    float target_tau;     /* encoder_target_tau: Polyak rate of predictor_target */
    /* SMM (configs/agent/smm.yaml, pretrain.yaml): rep_dim = z_dim; lr is unused, the two optimisers have their own rates */
    float sp_lr, vae_lr, vae_beta;
    float state_ent_coef, latent_ent_coef, latent_cond_ent_coef;
    float goal_x, goal_y; /* smm.py:139 self.goal = (150, 75): p*(s) is 1/dist of obs[:, :2] to it beyond distance 1 */
    int32_t world_size;   /* data-parallel ranks (0 and 1: one): every loss mean, loss gradient and metric is over batch * world_size rows
                             (the gradients and the metrics are then this rank's partial sums / means); Proto, ICM-APT and APS with
                             batch * world_size <= 8192 (Proto's Sinkhorn and candidate draw run over the gathered global batch, redundantly
                             and identically on every rank; the kNN reward of the other two seeks its neighbours in it) */
    int32_t rank;         /* this rank's batch rows are rows [rank * batch, (rank + 1) * batch) of the global batch (SMM's epsilon draws) */
} exorl_intr_cfg;

typedef struct exorl_intr exorl_intr_t;

/* metric slots of exorl_intr_metrics */
#define EXORL_IM_LOSS        0   /* rnd_loss / icm_loss */
#define EXORL_IM_INTR_REWARD 1   /* mean intrinsic reward of the batch */
#define EXORL_IM_EXTR_REWARD 2   /* mean of the extrinsic reward passed in (0 if none) */
#define EXORL_IM_RMS_MEAN    3   /* running mean of the RMS (RND: pred_error_mean) */
#define EXORL_IM_RMS_STD     4   /* sqrt of its running variance (RND: pred_error_std) */
#define EXORL_IM_ACC         5   /* DIAYN: discriminator accuracy (diayn_acc) */
#define EXORL_IM_ENT_REWARD  6   /* APS: mean particle-entropy part of the reward (intr_ent_reward) */
#define EXORL_IM_SF_REWARD   7   /* APS: mean successor-feature part (intr_sf_reward) */
/* SMM reuses the slots: 0 loss_vae, 1 intr_reward, 2 extr_reward, 3 log_p_star (batch mean), 4 pred_log_ratios, 5 loss_pred,
 * 6 latent_cond_ent_coef term, 7 var_j(log_p_star_j) — the constant the reference's (B,B) reward broadcast adds to each critic's loss */
#define EXORL_N_INTR_METRICS 8

/* workspace: device memory of exorl_intr_workspace_bytes(cfg) bytes, 256-byte aligned, owned by the caller (so that the
 * parameters can be exposed as the caller's own tensors), or null to let the library allocate. */
size_t exorl_intr_workspace_bytes(const exorl_intr_cfg* cfg);
int exorl_intr_create(const exorl_intr_cfg* cfg, void* workspace, size_t workspace_bytes, exorl_intr_t** out);
int exorl_intr_destroy(exorl_intr_t* m);
/* Parameter tensors in the module's parameters() order (RND: predictor.{1,3,5}, target.{1,3,5}; ICM: forward_net.{0,2},
 * backward_net.{0,2}; ICM-APT: trunk.0, trunk.1 (LayerNorm), forward_net, backward_net; Disagreement: ensemble.{m}.{0,2};
 * DIAYN: skill_pred_net.{0,2,4}; APS: state_feat_net.{0,2,4}; SMM: z_pred_net.{0,2,4}, vae.enc.{0,2}, vae.enc_mu, vae.enc_logvar,
 * vae.dec.{0,2,4}; Proto: predictor, projector.trunk.{0,2}, protos (no bias), then the frozen predictor_target),
 * each weight then bias.
 * what = EXORL_T_*; RND's frozen target tensors have parameters only. */
int exorl_intr_num_tensors(exorl_intr_t* m, int32_t* n);
int exorl_intr_tensor(exorl_intr_t* m, int32_t index, int32_t what, void** ptr, int64_t* rows, int64_t* cols);
int exorl_intr_flat(exorl_intr_t* m, int32_t what, void** ptr, int64_t* numel);
/* Device state outside the parameters: rms = {float M, float S, double n} (utils.RMS); bn = running_mean[obs_dim],
 * running_var[obs_dim], num_batches_tracked (as float) of RND's BatchNorm1d, or null. */
int exorl_intr_state(exorl_intr_t* m, void** rms_dev, void** bn_dev, int64_t* bn_numel);
/* Proto's candidate queue (queue_size x pred_dim, device) and its write pointer (get: set == 0; restore: set != 0). */
int exorl_intr_queue(exorl_intr_t* m, void** queue_dev, int64_t* rows, int64_t* cols, int64_t* ptr_inout, int32_t set);
/* One sampled batch as device pointers with row strides in floats (so that columns of a wider matrix can be passed in place:
 * DIAYN's skill lives in the last columns of the agent's [obs | skill] rows). action / next_obs / skill / extr_reward may be
 * null where the module does not read them; reward_out (batch,) may alias extr_reward (the agent's reward slot). */
typedef struct exorl_intr_batch {
    const float* obs;      int64_t obs_ld;
    const float* action;   int64_t action_ld;
    const float* next_obs; int64_t next_obs_ld;
    const float* skill;    int64_t skill_ld;
    const float* extr_reward;
    float* reward_out;
    const float* next_obs_target; int64_t next_obs_target_ld;   /* Proto on pixels: encoder_target(next_obs) for the Sinkhorn branch
                                                                   (proto.py:144-148); null -> next_obs */
    float* dobs_out;            /* if set (train != 0): receives the loss gradient at the encoding the module's loss reaches the caller's encoder
                                   through, dense (batch, obs_dim), so that the caller continues the backward pass: d/d(obs rows) for Proto
                                   (proto_opt owns the encoder too, proto.py:75-78), ICM, ICM-APT and Disagreement (next_obs is encoded without a
                                   graph there, icm.py:97-99), SMM (through the VAE's input and its reconstruction target, smm.py:61-70) and RND with
                                   EXORL_INTR_ENCODED (the predictor's input); d/d(next_obs rows) for DIAYN and APS (diayn.py:78-92, aps.py:147-159) */
    const float* cat_uniform;   /* Proto: num_protos uniforms in [0,1) for Categorical(prob).sample() (proto.py:112); SMM: the VAE's
                                   epsilon, (batch, 128) standard normals (smm.py:62); null -> Philox */
} exorl_intr_batch;
/* train != 0: the module's optimiser step (update_rnd / update_icm / update_disagreement / update_diayn) then
 * compute_intr_reward under the updated module (rnd.py:121-124, icm.py:106-110, icm_apt.py:123-127, disagreement.py:106-112,
 * diayn.py:143-147); train == 0: compute_intr_reward only; train == 2 (Proto): the optimiser step only — with an encoder in front
 * the reward is computed from features re-encoded after that step (proto.py:173-177). */
int exorl_intr_update(exorl_intr_t* m, const exorl_intr_batch* batch, int32_t train, void* stream);
/* The same step in phases, for data parallelism (world_size > 1: exorl_intr_update then refuses). Call phase 0, 1, ... with the
 * same arguments; each returns in *next_exchange the exchange the ranks run before the next phase, or -1 when the step is complete:
 *   EXORL_INTR_XCHG_GRAD     the module's flat gradients (every kind that trains; SMM's two optimisers share the range): sum all-reduce
 *   EXORL_INTR_XCHG_REP      ICM-APT / APS: the representation rows the kNN reward reads (ICM-APT: trunk(obs); APS: features of next_obs);
 *                            Proto: l2norm(predictor_target(next_obs_target)) for the Sinkhorn assignment (the step) and
 *                            l2norm(predictor(next_obs)) for the candidate draw (the reward), batch x pred_dim per rank
 *   EXORL_INTR_XCHG_MOMENTS  RND / ICM-APT / APS (knn_rms): each rank's (n, mean, M2) of the RMS input, merged in rank order in double;
 *                            SMM on state rows: those of log p*(s_j) (metric slots 3 and 7 are then the global values on every rank)
 *   EXORL_INTR_XCHG_BN       RND on state rows: each rank's per-feature (n, mean, M2) of BatchNorm1d's input, 3 * obs_dim doubles, merged
 *                            the same way; it is the first exchange of the step, and running_var takes the unbiased estimate over
 *                            batch * world_size rows
 * With world_size 1 the phases back to back are exorl_intr_update bit for bit (only the gradient exchange is named: a sum over one rank). */
#define EXORL_INTR_XCHG_GRAD    0
#define EXORL_INTR_XCHG_REP     1
#define EXORL_INTR_XCHG_MOMENTS 2
#define EXORL_INTR_XCHG_BN      3
#define EXORL_XCHG_F32    0
#define EXORL_XCHG_F64    1
#define EXORL_XCHG_SUM    0      /* sum all-reduce of count elements in place */
#define EXORL_XCHG_GATHER 1      /* all-gather: rank r's count elements sit at slot r (ptr + r * count) of world_size slots, rank order */
int exorl_intr_update_phase(exorl_intr_t* m, const exorl_intr_batch* batch, int32_t train, int32_t phase, int32_t* next_exchange, void* stream);
int exorl_intr_exchange(exorl_intr_t* m, int32_t id, void** ptr_dev, int64_t* count, int32_t* dtype /* EXORL_XCHG_F32 / _F64 */,
                        int32_t* op /* EXORL_XCHG_SUM / _GATHER */);
int exorl_intr_metrics(exorl_intr_t* m, float* host_out /* EXORL_N_INTR_METRICS */, void* stream);
/* exorl_agent_enable_graph with a reward-free agent's module in front of the agent's step: one hipGraph of
 *   replay sample (PHILOX) into the agent's batch slots -> the meta columns into the next_obs rows (meta_dim > 0) ->
 *   exorl_intr_update(intr, batch, train = 1) -> exorl_agent_update.
 * batch: the module's view of the agent's batch slots (exorl_agent_batch_slots), fixed for the graph's life; reward_out (and extr_reward,
 *   if set) is the agent's reward slot; cat_uniform and dobs_out are null (a captured step draws from Philox and has no encoder behind it).
 * meta_dim > 0: the agent's rows are [obs | meta] (DIAYN's skill, APS's task, SMM's z): the replay's obs_bytes is (obs_dim - meta_dim) * 4
 *   and its meta columns are meta_dim wide; the gather writes them behind the obs rows and one more kernel copies them behind the next_obs rows.
 * intr == NULL (batch ignored): the agent's step alone, with the meta columns where meta_dim > 0 (fine-tuning); with meta_dim 0 that is
 *   exorl_agent_enable_graph.
 * What moves from one module step to the next — the Adam step count and the scalars of its optimisers, the Philox draw counter, Proto's
 * queue pointer — lives in a device struct the library allocates on first capture; the captured step advances it itself.
 * exorl_agent_step_graph advances the module's host counters with the agent's, so exorl_intr_opt_steps / _counter / _queue keep answering
 * without a read-back; their setters and eager exorl_intr_update calls in between are pushed to the device before the next launch.
 * One process only (world_size 1 on both handles). exorl_agent_step_graph / exorl_agent_disable_graph serve this graph too; the module
 * must outlive it. */
int exorl_agent_enable_graph_intr(exorl_agent_t* a, exorl_intr_t* intr, const exorl_intr_batch* batch, int32_t meta_dim, exorl_replay_t* r,
                                  int32_t nstep, float gamma, float stddev, void* stream);
/* optimiser step count of the module's Adam: set == 0 reads into *steps, else writes it (snapshot restore) */
int exorl_intr_opt_steps(exorl_intr_t* m, int64_t* steps, int32_t set);
/* Philox counter of the module's own random draws (Proto's categorical candidate picks, SMM's VAE epsilon): part of the pickled state */
int exorl_intr_counter(exorl_intr_t* m, uint64_t* counter_inout, int32_t set);

/* ---------------------------------------------------------------------------------------------
 * Pixel front end (building blocks; the pixel actor/critic heads are not wired into exorl_agent_* yet).
 *   utils.RandomShiftsAug  utils/utils.py:222-254      ddpg.Encoder  agents/unsupervised_learning/ddpg.py:12-39
 * ------------------------------------------------------------------------------------------- */
/* out (n, c, h, h) fp32 pixel values = RandomShiftsAug(pad)(x) for x (n, c, h, h) uint8. shifts_dev: (n, 2) int32 (x shift, y shift)
 * in [0, 2 pad] — what torch.randint draws at utils.py:244-248 — or null for Philox(seed, counter). */
int exorl_aug_shift(const unsigned char* x_dev, int32_t n, int32_t c, int32_t h, int32_t pad, const int32_t* shifts_dev, uint64_t seed,
                    uint64_t counter, float* out_dev, void* stream);
/* Encoder parameters live in one flat fp32 buffer in torch order convnet.{0,2,4,6}.{weight,bias} (each tensor padded to 4 floats). */
int64_t exorl_encoder_param_floats(int32_t c_in, int32_t hw);
int64_t exorl_encoder_out_dim(int32_t hw);                         /* repr_dim: 32*35*35 for 84x84, 32*25*25 for 64x64 */
int64_t exorl_encoder_workspace_floats(int32_t n, int32_t c_in, int32_t hw);
/* Encoder.forward on x (n, c_in, hw, hw) fp32 pixel values; *h_out_dev = the flattened features (n, repr_dim) inside ws_dev. */
int exorl_encoder_forward(const float* params_dev, int32_t c_in, int32_t hw, const float* x_dev, int32_t n, float* ws_dev, float** h_out_dev,
                          void* stream);
/* Backward after exorl_encoder_forward with the same x / ws: dh_dev (n, repr_dim) is overwritten; parameter gradients go to
 * grads_dev (flat layout of the parameters). */
int exorl_encoder_backward(const float* params_dev, int32_t c_in, int32_t hw, const float* x_dev, int32_t n, float* ws_dev, float* dh_dev,
                           float* grads_dev, void* stream);
/* The same with the 32-channel stride-1 layers (forward and dgrad) on the matrix cores: precision = EXORL_PREC_BF16 / _BF16X3 runs them
 * as an implicit GEMM on v_mfma_f32_32x32x16_bf16 (split mode: hi*hi + hi*lo + lo*hi); EXORL_PREC_F32 = the two calls above. The first
 * layer (3 or 9 input channels, stride 2, uint8 scaling) and the weight gradients stay fp32 FMA. */
int exorl_encoder_forward_prec(const float* params_dev, int32_t c_in, int32_t hw, const float* x_dev, int32_t n, float* ws_dev, float** h_out_dev,
                               int32_t precision, void* stream);
int exorl_encoder_backward_prec(const float* params_dev, int32_t c_in, int32_t hw, const float* x_dev, int32_t n, float* ws_dev, float* dh_dev,
                                float* grads_dev, int32_t precision, void* stream);
int exorl_u8_to_f32(const unsigned char* x_dev, int64_t n, float* out_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * DDPG on pixel observations (agents/unsupervised_learning/ddpg.py with obs_type == 'pixels'): augmentation + encoder +
 * pixel Actor (:42-76) / Critic (:79-123) and update (:240-328; the encoder steps with the critic's loss).
 * ------------------------------------------------------------------------------------------- */
typedef struct exorl_pixel_cfg {
    int32_t c_in, hw;          /* obs_shape = (c_in, hw, hw), hw in {84, 64}, uint8 */
    int32_t act_dim, feature_dim, hidden_dim, batch;
    int32_t precision;         /* EXORL_PREC_*: Linear layers' GEMMs and (bf16 modes) the 32-channel convolutions on MFMA; fp32: fp32 FMA convolutions */
    int32_t meta_dim;          /* skill / task columns concatenated after the encoding in front of the actor's and the critic's trunk (ddpg.py:294-299,305-312) */
    float lr, tau, stddev_clip;
    int32_t sf_dim;            /* > 0: CriticSF (aps.py:17-60) — each Q head emits sf_dim successor features, Q = task . features, the task being the meta row */
    uint64_t seed;
    int32_t world_size;        /* data-parallel ranks (0 and 1: one): every mean over the batch is over batch * world_size rows, metrics are partial means */
} exorl_pixel_cfg;
typedef struct exorl_pixel_agent exorl_pixel_agent_t;
#define EXORL_PNET_ENCODER 0
#define EXORL_PNET_ACTOR   1
#define EXORL_PNET_CRITIC  2
#define EXORL_PNET_CRITIC_TARGET 3
size_t exorl_pixel_agent_workspace_bytes(const exorl_pixel_cfg* cfg);
int exorl_pixel_agent_create(const exorl_pixel_cfg* cfg, void* workspace_dev, size_t workspace_bytes, exorl_pixel_agent_t** out);
int exorl_pixel_agent_destroy(exorl_pixel_agent_t* a);
/* tensors in parameters() order: encoder convnet.{0,2,4,6}.{weight,bias} (weights as (32, ci*9)); actor trunk.0, trunk.1,
 * policy.{0,2,4}; critic trunk.0, trunk.1, Q1.{0,2,4}, Q2.{0,2,4}. what = EXORL_T_*; the target has parameters only. */
int exorl_pixel_agent_num_tensors(exorl_pixel_agent_t* a, int32_t net, int32_t* n);
int exorl_pixel_agent_tensor(exorl_pixel_agent_t* a, int32_t net, int32_t index, int32_t what, void** ptr_dev, int64_t* rows, int64_t* cols);
int exorl_pixel_agent_sync_target(exorl_pixel_agent_t* a, void* stream);       /* critic_target.load_state_dict(critic.state_dict()) */
int exorl_pixel_agent_batch_slots(exorl_pixel_agent_t* a, exorl_batch_out* out);   /* uint8 obs / next_obs rows for the HBM sampler */
int exorl_pixel_agent_set_batch(exorl_pixel_agent_t* a, const unsigned char* obs_dev, const float* action_dev, const float* reward_dev,
                                const float* discount_dev, const unsigned char* next_obs_dev, void* stream);
/* One update() on the batch in the slots. `images` says what the handle's image buffers hold when the call starts; shifts_*: (batch, 2)
 * int32 RandomShiftsAug draws for obs / next_obs or null -> Philox (EXORL_PIXEL_IMAGES_FRESH only: the other two refuse shifts);
 * noise_*: (batch, act_dim) standard normals for the TruncatedNormal draws (critic target first, actor second) or null -> Philox. */
#define EXORL_PIXEL_IMAGES_FRESH     0  /* augment with shifts_* (null: Philox), then encode */
#define EXORL_PIXEL_IMAGES_AUGMENTED 1  /* the images exorl_pixel_agent_augment left; shifts_* must be null */
#define EXORL_PIXEL_IMAGES_ENCODED   2  /* also the encodings of encode(0,0)/(1,0); needs set_train_encoder(0); shifts_* must be null */
typedef struct exorl_pixel_step {
    float stddev; int32_t images;
    const int32_t *shifts_obs_dev, *shifts_next_dev;
    const float *noise_critic_dev, *noise_actor_dev;
} exorl_pixel_step;
int exorl_pixel_agent_update(exorl_pixel_agent_t* a, const exorl_pixel_step* step, void* stream);
/* The phased calls, for data parallelism (world_size > 1: exorl_pixel_agent_update refuses without a communicator, the other two one-call
 * forms refuse). Call phase 0, 1, ... with the same arguments; each returns in *next_exchange the exchange (EXORL_PIXEL_XCHG_*) the ranks
 * run before the next phase, or -1 when the call is complete. With world_size 1 the phases back to back are the one-call form bit for bit.
 *   call                 phase  work                                                                                   next_exchange
 *   _update_phase        0      augmentation and encoding as `images` says, critic forward + backward, encoder        CRITIC_GRAD
 *                               backward when it trains (reads shifts_*, noise_critic)
 *                        1      critic Adam, encoder Adam, actor forward + backward on the stepped critic             ACTOR_GRAD
 *                               (reads noise_actor)
 *                        2      actor Adam, critic soft update                                                         -1
 *   _encoder_step_phase  0      encoder backward from dfeat_dev                                                        ENCODER_GRAD
 *                        1      the optimiser step(s) `opt` chooses (dfeat_dev unused)                                 -1
 *   _rnd_features_phase  0      augmentation (reads shifts_dev), per-channel sums of the BatchNorm2d input             BN
 *                        1      mean, per-channel sums of the centred squares                                          BN
 *                        2      normalisation over batch * world_size images, running statistics, both encodings      -1
 *                               (fills the feature pointers)
 * exorl_pixel_agent_exchange names the buffer of an exchange; every one is a sum all-reduce in place (*op = EXORL_XCHG_SUM):
 *   CRITIC_GRAD   the critic's gradients, then (set_train_encoder(1)) the encoder's: one contiguous range            EXORL_XCHG_F32
 *   ACTOR_GRAD    the actor's gradients                                                                               EXORL_XCHG_F32
 *   ENCODER_GRAD  the encoder's gradients alone                                                                       EXORL_XCHG_F32
 *   BN            c_in * 128 partial sums of the BatchNorm2d statistics                                               EXORL_XCHG_F64
 * *count in elements (padding of the gradient ranges included: it stays zero). */
#define EXORL_PIXEL_XCHG_CRITIC_GRAD  0
#define EXORL_PIXEL_XCHG_ACTOR_GRAD   1
#define EXORL_PIXEL_XCHG_ENCODER_GRAD 2
#define EXORL_PIXEL_XCHG_BN           3
int exorl_pixel_agent_update_phase(exorl_pixel_agent_t* a, int32_t phase, const exorl_pixel_step* step, int32_t* next_exchange, void* stream);
int exorl_pixel_agent_exchange(exorl_pixel_agent_t* a, int32_t id, void** ptr_dev, int64_t* count, int32_t* dtype /* EXORL_XCHG_F32 / _F64 */,
                               int32_t* op /* EXORL_XCHG_SUM */);
/* Attach a communicator of world_size ranks (NULL detaches): exorl_pixel_agent_update then all-reduces both exchanges between its phases on
 * `stream`. The critic's part of exchange 0 is reduced on a second stream while the encoder's backward pass runs. */
int exorl_pixel_agent_set_comm(exorl_pixel_agent_t* a, exorl_comm_t* c);
int exorl_pixel_agent_metrics(exorl_pixel_agent_t* a, float* host_out /* EXORL_N_METRICS */, void* stream);
/* Primitives for agents that put a module between augmentation and the DDPG step (Proto on pixels, proto.py:159-207): augment once,
 * encode with the online or the target encoder, push a feature gradient back through the encoder with a chosen optimiser state,
 * maintain encoder_target; exorl_pixel_agent_update with images = EXORL_PIXEL_IMAGES_AUGMENTED then reuses the augmented batch, and with
 * EXORL_PIXEL_IMAGES_ENCODED also the encodings the last exorl_pixel_agent_encode(0, 0) / (1, 0) calls left (what the agents that step the
 * encoder through their own module hand the critic: computed before that step, detached — icm.py:97-131, diayn.py:137-170; needs
 * set_train_encoder(0)). */
int exorl_pixel_agent_augment(exorl_pixel_agent_t* a, const int32_t* shifts_obs_dev, const int32_t* shifts_next_dev, void* stream);
int exorl_pixel_agent_encode(exorl_pixel_agent_t* a, int32_t which, int32_t target, float** feat_out_dev, void* stream);
int exorl_pixel_agent_encoder_step(exorl_pixel_agent_t* a, int32_t which, float* dfeat_dev, int32_t opt /* 0 encoder_opt, 1 second state, 2 both */, void* stream);
/* The same in two phases (the table above). */
int exorl_pixel_agent_encoder_step_phase(exorl_pixel_agent_t* a, int32_t which, float* dfeat_dev, int32_t opt, int32_t phase, int32_t* next_exchange,
                                         void* stream);
int exorl_pixel_agent_encoder_target(exorl_pixel_agent_t* a, float tau, int32_t init, void* stream);
/* RND on pixels (rnd.py:26-27,35-39,47-53): x = clamp(BatchNorm2d(RandomShiftsAug(obs)), +-clip_val), then the agent's encoder on x
 * (*feat_pred_dev; exorl_pixel_agent_encoder_step(0, dfeat, 2) continues its backward pass and steps the encoder with rnd_opt's state and
 * then encoder_opt's, rnd.py:86-89) and the frozen encoder copy kept in the encoder_target slot (*feat_target_dev). Every call draws a new
 * augmentation and updates the BatchNorm running statistics, as RND.forward does. */
int exorl_pixel_agent_rnd_features(exorl_pixel_agent_t* a, const int32_t* shifts_dev, float clip_val, float** feat_pred_dev, float** feat_target_dev,
                                   void* stream);
/* The same in three phases (the table above). */
int exorl_pixel_agent_rnd_features_phase(exorl_pixel_agent_t* a, int32_t phase, const int32_t* shifts_dev, float clip_val, float** feat_pred_dev,
                                         float** feat_target_dev, int32_t* next_exchange, void* stream);
int exorl_pixel_agent_bn_state(exorl_pixel_agent_t* a, void** ptr_dev, int64_t* n_floats);   /* running_mean[c] running_var[c] num_batches_tracked */
int exorl_pixel_agent_encoder_target_ptr(exorl_pixel_agent_t* a, void** ptr_dev);
/* Whole-agent pickling (pretrain.py:293-300): steps3 = {Adam step count of critic_opt/actor_opt, of proto_opt's encoder state, of encoder_opt},
 * counters4 = Philox counters of the update-noise, augmentation, act() and RND-augmentation streams; encoder_opt2 = proto_opt's Adam moments for the
 * encoder (n floats each, same layout as the encoder's flat parameters, which encoder_target_ptr also uses). */
int exorl_pixel_agent_state(exorl_pixel_agent_t* a, int64_t* steps3_out, uint64_t* counters4_out);
int exorl_pixel_agent_set_state(exorl_pixel_agent_t* a, const int64_t* steps3, const uint64_t* counters4);
int exorl_pixel_agent_encoder_opt2(exorl_pixel_agent_t* a, void** m_dev, void** v_dev, int64_t* n_floats);
/* enable == 0: update() treats the encoding as detached in update_critic (what the reward-free agents pass, proto.py:190-193):
 * no encoder backward, encoder_opt does not step. Default 1 (plain DDPG, ddpg.py:316-319). */
int exorl_pixel_agent_set_train_encoder(exorl_pixel_agent_t* a, int32_t enable);
int exorl_pixel_agent_act(exorl_pixel_agent_t* a, const unsigned char* obs_dev, const float* meta_dev /* (meta_dim,) or null */, float stddev, int32_t eval_mode, const float* noise_dev,
                          float* action_out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EXORL_HIP_H */
