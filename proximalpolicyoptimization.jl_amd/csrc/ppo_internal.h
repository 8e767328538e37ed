// ppo_internal.h -- shared internals of libppo_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include <map>
#include "../../include/ppo_hip.h"

#define PPO_OUT 4   // actions per half-edge (test/quad_game_utilities.jl:39,95)
#define PPO_TPL 36  // template rows; F = 72
#define PPO_PACK_PAD (16 * 64 * 4)   // floats of zero tail padding behind each packed weight stream (prefetch over-read)
// bytes of zero tail padding behind the split-fp32 (bf16x6) piece streams.  W2 (w2x: backward, w2fx: train forward): the last
// round of an operand ring re-issues a ring's depth of 1 KiB pieces past the last wave's stream (static_asserts at the rings).
// W1 (w1x): layer 1's ring stops at the stream's end; the padding is slack
#define PPO_X6_W2_PAD_BYTES 16384
#define PPO_X6_W1_PAD_BYTES 8192

// ---------------------------------------------------------------- host-side error plumbing
void ppo_set_error(const std::string& msg);
hipStream_t ppo_stream();
int ppo_hip_fail(hipError_t e, const char* what, const char* file, int line);

#define HIP_TRY(expr)                                                        \
    do {                                                                     \
        hipError_t _e = (expr);                                              \
        if (_e != hipSuccess) return ppo_hip_fail(_e, #expr, __FILE__, __LINE__); \
    } while (0)
#define ARG_CHECK(cond, msg)                                                 \
    do {                                                                     \
        if (!(cond)) { ppo_set_error(std::string("AssertionError: ") + msg + " [" #cond "]"); return PPO_ERR_ARG; } \
    } while (0)
#define PPO_TRY(expr)                                                        \
    do { int32_t _s = (expr); if (_s != PPO_OK) return _s; } while (0)

// host <-> device copies on the engine's stream, complete on return
template <typename T>
inline int32_t h2d(T* dst, const T* src, size_t n) {
    if (n == 0) return PPO_OK;
    HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyHostToDevice, ppo_stream()));
    HIP_TRY(hipStreamSynchronize(ppo_stream()));
    return PPO_OK;
}
template <typename T>
inline int32_t d2h(T* dst, const T* src, size_t n) {
    if (n == 0) return PPO_OK;
    HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, ppo_stream()));
    HIP_TRY(hipStreamSynchronize(ppo_stream()));
    return PPO_OK;
}

// kernel timing registry (bench roofline leg)
struct ProfScope {
    const char* name; hipEvent_t e0, e1; bool on;
    ProfScope(const char* n);
    ~ProfScope();
};

// ---------------------------------------------------------------- device buffers
template <typename T>
struct DevBuf {
    T* p = nullptr; size_t n = 0;
    int32_t alloc(size_t count) {
        if (count <= n && p) return PPO_OK;
        release();
        if (count == 0) return PPO_OK;
        HIP_TRY(hipMalloc((void**)&p, count * sizeof(T)));
        n = count;
        return PPO_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
    ~DevBuf() { release(); }
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
};

// ---------------------------------------------------------------- handles
struct ppo_env_s {
    int32_t kind, Q, H, A, V, F, max_actions;
    int32_t strict_sampling = 0;       // 1: a CDF residue landing on a masked action is an error (reference @assert)
    float no_action_reward;
    int64_t N, global_offset;
    uint64_t seed;
    DevBuf<int8_t> score, degree;      // [N][V]
    DevBuf<uint32_t> active;           // [N]
    DevBuf<int32_t> steps;             // [N]
    DevBuf<float> reward;              // [N]
    DevBuf<uint8_t> done;              // [N]
    DevBuf<uint32_t> episode, tick;    // [N]
    DevBuf<int32_t> err;               // [1] OR of error flags
    DevBuf<int32_t> actions_tmp;       // [N]
    DevBuf<int8_t> obs_tmp;            // [N][H][F]
    DevBuf<int32_t> episodes_left;     // [N] (episodes mode)
    DevBuf<int8_t> tmpl;               // [H][36] template vertex ids (env_template), -1 = missing: looked up by k_env_observe
};

// k-slot order of the packed W2^T fragments (backward: dH1^T = W2^T dZ2^T).  Row form: component e of fragment group g,
// lane half hh <-> contraction feature 8g + 4hh + e, so the B operands of four MFMAs are ONE 16-byte LDS read of a
// row-major dZ2 tile; else feature 8g + 2e + hh against a feature-major tile, one ds_read_b32 per MFMA (round-1 form).
// Measured (gpurun_out/r2x, alternating): HID = 128 backward 0.1170 -> 0.1156 ms with the row form; at HID = 256 it is
// 0.3 % SLOWER (0.3423 -> 0.3432: LDS instructions beside an fp32 MFMA are not what that kernel waits for, and phase C
// then needs four 4-byte reads per A operand), so the row form is used up to HID = 128 only.  Shared by ppo_optim.hip
// (packing), ppo_policy_bwd.hip, ppo_policy_bwd_small.hip and ppo_policy_train_tile.hip.
#define PPO_BWD_Z2ROW_AT(HID) ((HID) <= 128)

struct ppo_policy_s {
    int32_t F, HID, L, OUT;            // HID: the width the kernels run (128 or 256); L = hidden layers (test/policy.jl:9-19):
                                       // Dense(F,HID) + (L-1) x Dense(HID,HID) + Dense(HID,OUT).  L == 2 runs the fused
                                       // kernels; L in {1, 3, 4} the layer-looped ("deep") forms of the same kernels
    int32_t hid_user = 0;              // hidden_channels the caller asked for (<= HID): the missing units are zero-padded
    int64_t np_user = 0;               // parameter count of the caller's Policy (what crosses the ABI)
    int64_t np;                        // parameter count at width HID (device buffers, all-reduce)
    // canonical flat parameters (Flux order) + packed MFMA-fragment copies
    DevBuf<float> params;              // [np]
    DevBuf<float> w1p, w2p, w2tp;      // A-operand fragment order; w2p / w2tp: the L-1 hidden->hidden layers back to back (HID*HID each)
    DevBuf<float> b1p, b2p, w3p, b3;   // accumulator-init / VALU packs; b2p: L-1 x HID
    // bf16 compute mode (ppo_policy_set_dtype): bf16 fragment streams of the same parameters, rewritten by k_adam
    int32_t dtype = 0;                 // PPO_DTYPE_F32 / PPO_DTYPE_BF16
    DevBuf<uint16_t> w1b, w2b, w2tb;   // [HID/32][KS][64][8] A-operand fragments of v_mfma_f32_32x32x16_bf16
    DevBuf<uint16_t> w3c, w3tb;        // layer 3 forward (compact rows 0..3) / backward ([HID][4])
    // split-fp32 backward (ppo_policy_bwd_x6.hip): W2 as three bf16 pieces, B-operand fragments of dH1 = dZ2 W2,
    // [in-feature tile][k-step][piece: lo, mid, hi][64 lanes][8]; L == 2, F == 72 only; rewritten by k_adam
    DevBuf<uint16_t> w2x;
    // split-fp32 train forward (ppo_policy_fwd_x6.hip): A-operand piece fragments [feature tile][k-step][piece][64][8] of
    // layer 1 (5 k-steps of natural input order, zero padded from 72 to 80) and layer 2 (k order of packed accumulators)
    DevBuf<uint16_t> w1x, w2fx;
    DevBuf<float> grad;                // [np + 2]  (+ ppo sum, entropy sum)
    // training workspace
    DevBuf<float> act1, act2;          // saved activations, D-fragment order [tiles][HID/32][4][64] float4: the FIRST and the LAST hidden layer
    DevBuf<float> actm;                // L > 2: the L-2 hidden layers in between, [L-2][tiles]... back to back
    DevBuf<float> dz2f, dz1f;          // three-product backward: dZ of the last / first hidden layer in fragment order (like act2 / act1)
    DevBuf<float> dzm;                 // L > 2: dZ of the layers in between, like actm
    DevBuf<float> dY;                  // [tiles][32][4]
    DevBuf<double> loss_terms;         // [tiles][2]
    DevBuf<float> slabs;               // [nwg][slab]
    DevBuf<int32_t> idx;               // gathered transition ids of the minibatch
    DevBuf<int8_t> xs;                 // [tiles][32][F] state rows of the minibatch re-derived by the forward (compact rollouts)
    DevBuf<float> adv_col;             // batch_advantage scratch column [T*N] (PPO_ADV_RETURNS_NORMALISED)
    DevBuf<int32_t> err;               // device error flag
    int64_t cap_tiles = 0;
    int32_t nwg_bwd = 0;               // slabs holding weight-gradient partials of the last backward
    int32_t nwg_small = 0;             // slabs holding its small-gradient tails (0: the same slabs)
    int64_t last_B = 0;
    double last_entropy_weight = 0.0;
    // probability ratios p_new(a|s) / p_old(a|s) of the train forward (ppo_policy_tail.h) and what ppo_train makes of them
    DevBuf<float> ratio;               // [cap_tiles] one minibatch (ppo_forward_backward / ppo_step_batch), minibatch order
    DevBuf<float> ratio_col;           // [len] one epoch of ppo_train: the minibatch at dataset position `start` writes at start
    float* ratio_out = nullptr;        // where the next train forward stores them (train_pass_dev sets it)
    const float* ratio_last = nullptr; // what ppo_debug_train_ratios reads: the latest forward's, or the latest epoch's column
    int64_t ratio_last_n = 0;          // floats readable there
    DevBuf<double> stats_part;         // block partials of the two reductions, then their results (ppo_stats.hip)
    double target_kl = 0.0;            // ppo_policy_set_target_kl: 0 off
    int32_t stats_stopped = 0;         // the latest ppo_train: ended by target_kl before num_epochs
    std::vector<double> stats_kl, stats_old_kl, stats_clip;   // ... and its per-epoch statistics (epochs that ran)
    // KL anchor (ppo_policy_set_kl_anchor): a penalty anchor_coef * KL(q || pi) in the policy's PPO objective, q
    // the rollout buffer's target rows of anchor_source (PPO_TARGETS_COLUMN / PPO_TARGETS_RECORDED; PPO_ANCHOR_OFF: none)
    double anchor_coef = 0.0;          // >= 0, finite; adapted by ppo_train's epoch loop while anchor_target > 0
    int32_t anchor_source = PPO_ANCHOR_OFF;
    double anchor_target = 0.0;        // 0: fixed coefficient; d > 0: PPO's adaptive rule around d
    DevBuf<float> anchor;              // [cap_tiles] the divergence per state of one minibatch (ppo_forward_backward / ppo_step_batch)
    DevBuf<float> anchor_col;          // [len] one epoch of ppo_train, like ratio_col
    const float* anchor_last = nullptr; int64_t anchor_last_n = 0;   // what ppo_debug_anchor_kl reads, like ratio_last
    std::vector<double> astats_kl, astats_coef;   // the latest ppo_train, per epoch: mean anchor KL, the coefficient it ran with
    // critic: PPO's clipped value loss (ppo_policy_set_value_clip) and what ppo_value_train makes of V - vold
    double value_clip = 0.0;           // 0 off; > 0 on; +inf: record the statistics, never clip
    DevBuf<float> vdelta_col;          // [len] one epoch of ppo_value_train: the minibatch at dataset position `start` writes at start
    int64_t vdelta_n = 0;              // floats ppo_debug_value_deltas may read there (the latest epoch's), 0: none
    std::vector<double> vstats_clip, vstats_msq;   // the latest ppo_value_train, per epoch: clip_fraction, mean_sq_change
    // action selection of the calls that APPLY the policy (ppo_policy_set_selection); the collectors, the
    // forward and the training calls never read it
    int32_t select_rule = PPO_SELECT_SAMPLE;
    double select_temperature = 1.0;   // finite, > 0
    // truncation of the tempered distribution the "sample" rule draws from (ppo_policy_set_truncation): the top_k
    // likeliest actions (0: all) and the likeliest set whose mass in front of an action stays below top_p (1: all).  Read where
    // the selection is read, and by the same calls only
    int32_t trunc_top_k = 0;           // >= 0
    double trunc_top_p = 1.0;          // in (0, 1]
};
inline bool default_selection(const ppo_policy_s* p) { return p->select_rule == PPO_SELECT_SAMPLE && p->select_temperature == 1.0; }
inline bool default_truncation(const ppo_policy_s* p) { return p->trunc_top_k == 0 && p->trunc_top_p == 1.0; }

// one member of a Flux.Optimiser chain: its hyper row of ppo_optimiser_create and its state
struct OptMember {
    int32_t kind = 0;                  // PPO_OPT_*
    double eta = 0.0, h1 = 0.0, h2 = 0.0, h3 = 0.0, h4 = 0.0;   // the hyper row (eta in front; the members without eta keep
                                       // thresh / wd / gamma in its place): Adam eta, beta1, beta2, eps
    int64_t count = 0;                 // ExpDecay / InvDecay: update! calls seen
    DevBuf<float> s, s1;               // Adam m, v; Momentum / Nesterov velocity and RMSProp acc (s alone)
    double beta_pow[2] = {0.0, 0.0};   // Adam: beta1^t, beta2^t of the next step
};

inline bool has_eta(int32_t kind) { return kind >= PPO_OPT_ADAM && kind <= PPO_OPT_RMSPROP; }   // ClipValue .. InvDecay have none

// every optimiser handle is a chain: ppo_adam_create makes the chain of Adam alone that ppo_optimiser_create makes
struct ppo_adam_s {
    ppo_policy_s* pol;
    int64_t epochs_done = 0;           // epochs trained through ppo_train: keys the minibatch permutation with the seed
    // nmem = 1..4 members in chain order.  A chain of Adam alone runs the Adam kernels (k_reduce_adam / k_adam); every
    // other chain the chain kernels (k_reduce_chain / k_chain_update)
    int32_t nmem = 0;
    OptMember mem[4];
    // ClipNorm member: the update splits in two launches around it (ppo_optim.hip): D of the members before it, and
    // double-double partial sums of D^2, one per 32 consecutive elements of the first launch
    DevBuf<float> clip_d;              // [np]
    DevBuf<double> clip_part;          // [clip_slots][2]
    int64_t clip_slots = 0;
    bool adam_only() const { return nmem == 1 && mem[0].kind == PPO_OPT_ADAM; }
    double lr() const;                 // left-to-right product of the members' etas (get_optimizer_learning_rate)
};

struct DiskSink;   // ppo_disk.hip

struct ppo_rollouts_s {
    int64_t N, capT, T;    // T = steps currently held
    int32_t H, F, A;
    int64_t len;           // valid transitions
    // state storage, one of two forms (ppo_set_rollout_compact):
    //   expanded: the observation rows themselves, 2304 B per transition for Q = 8 (host-supplied rollouts always)
    //   compact:  the env snapshot the rows are derived from (score[V] then degree[V], int8: 64 B for Q = 8) -- the
    //             train forward re-derives the rows like the persistent rollout does (k_policy_fwd's FwdMode::TrainSnap)
    bool compact = false;
    int32_t V = 0;             // vertices per env (4Q)
    DevBuf<int8_t> states;     // [T][N][H][F]        (expanded form)
    DevBuf<int8_t> cstate;     // [T][N][2V]          (compact form)
    DevBuf<int8_t> tmpl;       // [H][36] template vertex ids of the env the buffer was created for
    DevBuf<int8_t> expand_tmp; // getters of the compact form: expanded observations, built on demand
    DevBuf<uint32_t> active;   // [T][N]
    DevBuf<int32_t> actions;   // [T][N]
    DevBuf<float> p_sel;       // [T][N]
    DevBuf<float> rewards;     // [T][N] raw
    DevBuf<float> returns;     // [T][N]
    DevBuf<uint8_t> done;      // [T][N]
    DevBuf<uint8_t> valid;     // [T][N]
    DevBuf<int32_t> index;     // [len] transition ids in dataset order
    DevBuf<float> full_probs;  // [T][N][A] optional
    DevBuf<float> values;      // [T+1][N] state values: host-supplied (ppo_rollouts_compute_gae) or a device critic's (ppo_rollouts_compute_values)
    DevBuf<float> adv;         // [T][N] GAE(gamma, lambda) advantages (PPO_ADV_GAE*)
    DevBuf<float> lam_ret;     // [T][N] lambda-returns adv + V
    int64_t adv_T = -1;        // T the adv column was computed for (-1: none)
    int64_t values_T = -1;     // T the values were computed for (-1: none)
    // time-limit bootstrap (ppo_gae_boot.hip): which done transitions were truncations, and what the critic makes of the
    // states they cut the episodes in
    DevBuf<uint8_t> truncated; // [T][N] 1: done && valid and the optimum not reached
    DevBuf<int32_t> trunc_ids; // [K] their transition ids, ascending
    DevBuf<int32_t> trunc_counts;  // compaction workspace: block counts / offsets, then the 8-byte total
    DevBuf<int8_t> boot_cstate;    // [K][2V] post-step env snapshots of those transitions
    DevBuf<uint32_t> boot_active;  // [K]
    DevBuf<float> boot_vals;   // [K] the critic's values of them
    DevBuf<float> boot;        // [T][N] boot_vals scattered to their transitions (or host-supplied), 0 elsewhere
    int64_t boot_T = -1;       // T the boot column was computed for (-1: none)
    DevBuf<double> stats_part; // workspace and result of k_value_moments (ppo_stats.hip)
    // policy distillation: a target distribution per transition, in full_probs' layout; allocated on first use
    DevBuf<float> targets;     // [T][N][A] filled by ppo_rollouts_fill_targets (a teacher's probabilities) or ppo_rollouts_set_targets
    int64_t targets_T = -1;    // T the targets were filled for (-1: none)
    int64_t probs_T = -1;      // T full_probs was recorded for (-1: the buffer's contents were collected without record_probs)
    bool all_valid = true;
    DiskSink* sink = nullptr;  // optional out-of-core store (ppo_rollouts_attach_disk)
    ~ppo_rollouts_s();
};

// rollout buffer internals and argument checks of ppo_api.hip, shared with the disk loader and ppo_play.hip
extern "C" int32_t rollouts_reserve(ppo_rollouts_s* r, int64_t T, bool compact);
extern "C" int32_t set_index_all(ppo_rollouts_s* r);
extern "C" int32_t check_shapes(ppo_rollouts_s* ro, ppo_env_s* env, ppo_policy_s* pol);
extern "C" bool want_compact(const ppo_rollouts_s* ro, int64_t T);
extern "C" int32_t check_internal_host(int32_t Q, int64_t count, const int8_t* score, const int8_t* degree, const uint32_t* active);
// the buffer now holds T steps, or (scratch_used) row 0 served a call as scratch and nothing is held: every column cached
// for the previous contents is stale
// (a collector that recorded the whole distributions sets probs_T behind this call)
inline void rollouts_filled(ppo_rollouts_s* ro, int64_t T) {
    ro->T = T; ro->adv_T = -1; ro->values_T = -1; ro->boot_T = -1; ro->targets_T = -1; ro->probs_T = -1;
}
inline void rollouts_scratch_used(ppo_rollouts_s* ro) { rollouts_filled(ro, 0); ro->len = 0; }

// out-of-core store hooks used by ppo_collect_rollouts (ppo_disk.hip)
int32_t disk_sink_begin(ppo_rollouts_s* ro, int64_t T);
int disk_sink_slots(const ppo_rollouts_s* ro);                // pinned records in the ring (0: no sink)
int disk_sink_chunk(const ppo_rollouts_s* ro);                // steps per persistent launch of a streamed collection
int32_t disk_sink_step(ppo_rollouts_s* ro, int64_t t);       // after the kernels of step t were enqueued
int32_t disk_sink_finish(ppo_rollouts_s* ro);                // after the return scan: appends returns, flushes
bool disk_sink_destroy(DiskSink* s);                           // false: an unreported deferred-finish failure (ppo_last_error set)
int32_t disk_sink_settle_previous(ppo_rollouts_s* ro);         // waits for a deferred finish; its failure is reported here

// ---------------------------------------------------------------- packed layout sizes
// one gradient slab: [dW of the L-1 hidden->hidden layers][dW1, input padded to 32][db1][db of the L-1 layers][dW3][db3 + pad]
// (L == 2: exactly the round-1 layout W2, W1, b1, b2, W3, b3)
static inline size_t slab_elems(int F, int HID, int L = 2) {    // without the padding: what the slab reduction walks
    const int FP = ((F + 31) / 32) * 32;
    return (size_t)(L - 1) * HID * HID + (size_t)HID * FP + (size_t)HID * L + (size_t)HID * PPO_OUT + 4;
}
static inline size_t slab_floats(int F, int HID, int L = 2) { return slab_elems(F, HID, L) + 60; }

// ---------------------------------------------------------------- kernel launchers (defined in the .hip files)
int32_t launch_returns_tn(const float* r, const uint8_t* done, float* out, int64_t T, int64_t N,
                          double discount, int f32mode);
int32_t launch_returns_flat(const float* r, const uint8_t* term, float* out, int64_t n, double discount, int f32mode);
int32_t launch_gae_tn(const float* r, const uint8_t* done, const float* values, float* adv, float* ret,
                      int64_t T, int64_t N, double gamma, double lambda);

int32_t launch_gae_boot_tn(const float* r, const uint8_t* done, const float* values, const float* boot, float* adv,
                           float* ret, int64_t T, int64_t N, double gamma, double lambda);
// ppo_gae_boot.hip: the buffer's truncated flags, their ascending ids and their count (the one host crossing); the
// post-step snapshots of those K transitions; vals[k] -> boot[ids[k]] over a zeroed column
int32_t launch_truncated(ppo_rollouts_s* ro, int64_t* K_out);
int32_t launch_truncated_states(ppo_rollouts_s* ro, int64_t K, int8_t* cstate_out, uint32_t* active_out);
int32_t launch_boot_scatter(ppo_rollouts_s* ro, const float* vals, int64_t K, float* boot);

int32_t launch_env_reset(ppo_env_s* e, int only_done);
// evaluator bookkeeping folded into the env step of the episodes mode (test/quad_game_utilities.jl:280-307,369-387,
// src/evaluate.jl:1-25): per-env running values of the episode in flight, one result per finished episode
struct EvalView {
    int32_t kind = 0;              // 0 off, 1 return (sum of rewards), 2 best return (initial score - lowest score seen),
                                   // 3 normalised best return (best / (initial score - optimum score); 1.0 when that is 0)
    double* ep_ret = nullptr;      // [N] reward sum of the episode in flight
    int32_t* ep_init = nullptr;    // [N] score at its reset
    int32_t* ep_min = nullptr;     // [N] lowest score seen so far
    int32_t* ep_maxret = nullptr;  // [N] initial score - optimum score
    int32_t* ep_count = nullptr;   // [N] episodes this env has finished
    double* out = nullptr;         // [num_traj] results, env-major (env n's episodes are consecutive)
    int64_t num_traj = 0;
};
int32_t launch_env_step(ppo_env_s* e, const int32_t* actions_dev, float* reward_out, uint8_t* done_out,
                        uint8_t* valid_out, int auto_reset, int episodes_mode, const EvalView* ev = nullptr);
// best-state bookkeeping folded into the env step of the episodes mode (best_state_in_rollout, single_trajectory_scores
// test/quad_game_utilities.jl:309-323,341-358; count_non_flips test/random_quad.jl:9-27): k_env_step_track, a sibling of
// k_env_step on the same env_step_ref.  The record of the trajectory in flight lives in its own output slot (the slot is
// known from its first step on), so finishing a trajectory copies nothing: gap = current_score - opt_score.
struct TrackView {
    int32_t* t_in = nullptr;       // [N] steps the trajectory in flight has played (0: its first step! is still to come)
    int32_t* ep_init = nullptr;    // [N] score at its start
    int32_t* ep_count = nullptr;   // [N] trajectories this env has finished
    int8_t* best_state = nullptr;  // [num_traj][2V] score[V] then degree[V] of the best state so far (k_env_snapshot's layout)
    uint32_t* best_active = nullptr;   // [num_traj]
    int32_t* best_gap = nullptr;   // [num_traj] its gap
    int32_t* best_step = nullptr;  // [num_traj] steps played when it was reached (0: the start; argmin's first minimum)
    int32_t* length = nullptr;     // [num_traj] steps of the whole trajectory (written on done)
    int32_t* initial_gap = nullptr;    // [num_traj]
    int32_t* trace = nullptr;      // [num_traj][max_actions] initial score - score behind step t, optional
    int32_t* type_counts = nullptr;    // [num_traj][4] actions played by type a % 4, optional (zeroed by the caller)
    int16_t* actions = nullptr;    // [num_traj][max_actions] the 0-based action played at step t in entry t - 1, optional (an
                                   // action index is below 16 Q <= 512).  In a record of results (`out` of the searches): the
                                   // path to the best state, best_step entries and -1 behind them
    int64_t num_traj = 0;          // slots, env-major like EvalView::out
};
int32_t launch_env_step_track(ppo_env_s* e, const int32_t* actions_dev, float* reward_out, uint8_t* done_out,
                              uint8_t* valid_out, const TrackView& tv);
// best-of-K search: start s of the round (snapshot start[s], active[s]) into envs s*K .. s*K + K - 1 as reset! would leave
// them (steps, reward, done = 0) with one episode to play; every env from busy on idles (episodes_left = 0)
int32_t launch_env_load_starts(ppo_env_s* e, const int8_t* start_state, const uint32_t* start_active, int64_t busy, int64_t K,
                               int32_t* t_in);
// ... and its reduction: winner of the K clones of each of S starts (lowest gap, then lowest clone) from the per-env
// records of `tv` (slot = env) into record out_base + s of `out`; clone_gaps (optional): [..][K] every clone's best gap.
// out.actions set (tv.actions then too): the winner's first best_step actions to row out_base + s, -1 behind them
int32_t launch_search_argmin(const TrackView& tv, int32_t V, int64_t S, int64_t K, const TrackView& out, int32_t* best_clone,
                             int32_t* clone_gaps, int64_t out_base, int32_t max_actions);
// resampling search, one launch for the S starts of a round: fold the K per-env records of every start into
// record out_base + s of `out` (flags & 1: the round's first fold takes the winner as it is, later ones only a strictly
// lower gap), then -- unless flags & 2, the fold behind a round's last step -- rank the live clones by (cur_gap, clone) and
// overwrite every clone of rank >= m = min(survivors, live) with state, record and t_in of the clone of rank (rank - m) % m.
// donors (optional): [..][E][K] log, row `event`; clone_gaps (optional): [..][K] every clone's record gap.  K above
// PPO_RESAMPLE_MAX_K (the keys are staged in LDS): PPO_ERR_UNSUPPORTED.
// out.actions set (tv.actions then too): the action history travels with the record -- a fold that takes a
// winner's record writes the first best_step entries of its history to row out_base + s of out.actions and -1 behind them,
// a copy takes the donor's entries 0 .. t_in - 1.  played: loop steps of the round so far (an upper bound of every t_in)
// values set: [N] floats, one per env, written before this launch; a live clone ranks by
// fmaf(-value_weight, values[env], (float)cur_gap) (a value that is not finite counting as 0) instead of cur_gap.
// event_values (optional): [..][E][K] log of the values read, row `event`, NaN for a terminal clone
constexpr int64_t PPO_RESAMPLE_MAX_K = 4096;
int32_t launch_search_resample(ppo_env_s* e, const TrackView& tv, int64_t S, int64_t K, int64_t survivors, int flags,
                               const TrackView& out, int32_t* best_clone, int64_t out_base, int32_t* donors, int64_t E,
                               int64_t event, int32_t* clone_gaps, int64_t played, const float* values = nullptr,
                               float* event_values = nullptr, float value_weight = 0.0f);
// beam search: what its kernels share.  Start s of a round owns envs s*K .. s*K + K - 1, its slots
constexpr int PPO_BEAM_MAX_K = 256;    // one thread per slot in k_beam_select's rank and k_beam_expand's step; the chosen keys
                                       // (16 B each) and the weights (12 B each) are staged in static LDS
struct BeamView {
    double* wm = nullptr;              // [N] a slot's weight: mantissa in [0.5, 1)
    int32_t* we = nullptr;             // [N] ... and exponent
    uint8_t* live = nullptr;           // [N]
    int32_t* sel_parent = nullptr;     // [N] what k_beam_select chose for slot j of the step: its parent slot (-1: dead)
    int32_t* sel_action = nullptr;     // [N] ... and 0-based action
    uint32_t* tick_scratch = nullptr;  // [N] the tick env_step_ref bumps in place of the env's own
    int32_t* fin = nullptr;            // [S] the start of the round has finished
    // results, one record per start of the call
    int8_t* best_state = nullptr; uint32_t* best_active = nullptr;
    int32_t* best_gap = nullptr; int32_t* best_beam = nullptr; int32_t* best_step = nullptr; int32_t* initial_gap = nullptr;
    double* best_mant = nullptr; int32_t* best_exp = nullptr;
    // back-pointer log [num_starts][max_actions][K], each on request: parent and action (both or neither), the weights
    int16_t* log_parent = nullptr; int16_t* log_action = nullptr; double* log_mant = nullptr; int32_t* log_exp = nullptr;
};
// load (behind launch_env_load_starts): slot 0 of every start live with weight (0.5, 1), the others dead; record out_base + s
// = the start's state at step 0
int32_t launch_beam_init(ppo_env_s* e, const BeamView& bv, int64_t S, int64_t K, const int8_t* start_state,
                         const uint32_t* start_active, int64_t out_base);
// step t of the S starts of a round: the exact top min(K, #candidates) of the scored candidates (probs: [N][A] of the states
// the envs hold) into sel_*, the weights and row t of the log; then gather of the parents' states, env step, fold, finish
int32_t launch_beam_select(ppo_env_s* e, const float* probs, const BeamView& bv, int64_t S, int64_t K, int64_t out_base, int64_t t);
int32_t launch_beam_expand(ppo_env_s* e, const BeamView& bv, int64_t S, int64_t K, int64_t out_base, int64_t t);
// the distinct beam: the parents stay in the env arrays through a step and the accepted children collect here
constexpr int PPO_BEAM_WINDOW = 256;   // candidates per round: k_beam_children runs one thread per window entry
constexpr int PPO_BEAM_MAX_ROUNDS = 16;
struct BeamChildView {
    // per slot [N]: the accepted children of the step
    int8_t* state = nullptr;           // [N][2V] score, then degree
    uint32_t* active = nullptr; int32_t* steps = nullptr; int32_t* gap = nullptr;
    double* wm = nullptr; int32_t* we = nullptr;
    int32_t* parent = nullptr; int32_t* action = nullptr; int32_t* rank = nullptr;
    unsigned long long* hash = nullptr;
    // per start [S]
    int32_t* n = nullptr;              // accepted so far in this step
    int32_t* examined = nullptr;       // candidates the walk has looked at
    int32_t* exhausted = nullptr;      // the select found fewer than a full window: no candidate is left below the ceiling
    int32_t* win_count = nullptr;      // entries of the window k_beam_children has not yet read
    unsigned long long* ceil = nullptr;  // [S][2] beam_key's two words: the window takes keys strictly below it
    // the window [S][PPO_BEAM_WINDOW], in rank order
    uint32_t* win_idx = nullptr;       // parent * A + action
    double* win_m = nullptr; int32_t* win_e = nullptr;
    // logs [num_starts][max_actions][K] and [num_starts][max_actions], each on request
    int32_t* log_rank = nullptr; int32_t* log_examined = nullptr;
};
// step t of the distinct beam: up to `rounds` times window + children, then one commit.  mode 1: "children", 2: "parents"
int32_t launch_beam_select_window(ppo_env_s* e, const float* probs, const BeamView& bv, const BeamChildView& cv, int64_t S, int64_t K);
int32_t launch_beam_children(ppo_env_s* e, const BeamView& bv, const BeamChildView& cv, int64_t S, int64_t K, int32_t mode);
int32_t launch_beam_commit(ppo_env_s* e, const BeamView& bv, const BeamChildView& cv, int64_t S, int64_t K, int64_t out_base, int64_t t);
// the refusals every value entry point shares: a bf16-dtype critic, an input width other than F (ppo_train.hip)
extern "C" int32_t value_checks(const char* who, ppo_policy_s* critic, int32_t F);
// teacher-forced replay: path m ([count][stride] 0-based actions, < 0 ends a path) from snapshot m (score[V]
// then degree[V]) as reset! leaves an env, until the path ends or the state is terminal; out_state / out_active / out_gap /
// applied per path, trace (optional) [count][stride].  work: [4][count] int32 scratch; err: one word, OR of the step's flags
int32_t launch_env_apply_paths(ppo_env_s* e, int64_t count, const int8_t* start_state, const uint32_t* start_active,
                               const int16_t* paths, int32_t stride, int8_t* out_state, uint32_t* out_active, int32_t* out_gap,
                               int32_t* applied, int32_t* trace_or_null, int32_t* work, int32_t* err);
// teacher-forced collection, loop step t.  Feed: actions_out[n] = paths[n][t] (0-based; [M][stride], lens[n] =
// the path's declared length <= stride), or -1 for an idle env: n >= M, t >= lens[n], or the env is terminal.  Forced forward:
// launch_policy_forced below.  Forced step: every env with an action >= 0 steps (env_step_ref), done = its own done or
// t + 1 == lens[n], valid = 0 for an action on an inactive quad; an idle env records valid 0, reward 0, done 1 and is not
// touched.  err: one word of the caller's, OR of the step's flags and the forward's bit 64
int32_t launch_paths_feed(ppo_env_s* e, const int16_t* paths, const int32_t* lens, int64_t M, int64_t stride, int64_t t,
                          int32_t* actions_out);
int32_t launch_env_step_forced(ppo_env_s* e, const int32_t* actions_dev, const int32_t* lens, int64_t t, float* reward_out,
                               uint8_t* done_out, uint8_t* valid_out, int32_t* err);
int32_t launch_env_observe(ppo_env_s* e, int8_t* obs_out, uint32_t* active_out);
// compact rollout storage: env snapshot of every env (score[V] then degree[V]) -> cstate_out [N][2V]
int32_t launch_env_snapshot(ppo_env_s* e, int8_t* cstate_out);
// snapshots -> observations (the same arithmetic as state(env)): count records of 2V bytes -> [count][H][F]
// idx (optional): output record n = transition idx[n] (a gathered minibatch) instead of record n
int32_t launch_expand_states(const int8_t* cstate, const uint32_t* active, const int8_t* tmpl, int64_t count, int32_t Q,
                             int8_t* obs_out, const int32_t* idx = nullptr);

int32_t launch_pack_params(ppo_policy_s* p);
int32_t launch_policy_probs(ppo_policy_s* p, const int8_t* states_dev, const uint32_t* active_dev, int64_t B,
                            int32_t H, float* probs_dev);
int32_t launch_policy_rollout(ppo_policy_s* p, ppo_env_s* e, const int8_t* states_dev, const uint32_t* active_dev,
                              int32_t* actions_out, float* psel_out, float* full_probs_or_null);
// one step under the policy's selection: launch_policy_rollout for the default ("sample", 1), otherwise k_policy_fwd's FwdMode::Tempered
// (tempered sampling) / Greedy / Truncated (tempered sampling from the truncated distribution: rule "sample" with a non-default
// truncation, at any temperature), same outputs.  A bf16-dtype policy with a non-default selection or truncation:
// PPO_ERR_UNSUPPORTED
int32_t launch_policy_select(ppo_policy_s* p, ppo_env_s* e, const int8_t* states_dev, const uint32_t* active_dev,
                             int32_t* actions_out, float* psel_out, float* full_probs_or_null);
// one teacher-forced step (k_policy_fwd's FwdMode::Forced): actions_io[n] = env n's given action (kept; < 0 idles), psel_out[n] = its
// probability under the policy, 0 for an idle env or an inactive quad (bit 64 of *err).  A bf16-dtype policy: PPO_ERR_UNSUPPORTED
int32_t launch_policy_forced(ppo_policy_s* p, ppo_env_s* e, const int8_t* states_dev, const uint32_t* active_dev,
                             int32_t* actions_io, float* psel_out, float* full_probs_or_null, int32_t* err);
// adv_col: the advantage column indexed by transition id (ro->returns for PPO_ADV_RETURNS)
int32_t launch_policy_rollout_persistent(ppo_policy_s* p, ppo_env_s* e, ppo_rollouts_s* ro, int64_t T, int record_probs,
                                         int64_t t0 = 0);
int32_t launch_adv_normalise(const float* returns, const int32_t* idx_dev, int64_t B, float* adv_col);

// ---------------------------------------------------------------- kernel selection (ppo_route.hip)
// Every kernel-selection knob of the policy, process-wide (include/ppo_hip.h): read from its environment variable once at
// load, changed by the ppo_set_* setters; a setter's -1 restores the value read at load.
struct PpoKnobs {
    // training pass                          environment variable
    int32_t bwd_split = 1;                    // PPO_BWD_SPLIT_BF16: split-fp32 train forward and fused backward
    int64_t train_tile_max_tiles = 0;         // PPO_TRAIN_TILE_MAX_TILES: one-tile training pass up to this many tiles
    int64_t bwd_small_max_tiles = 384;        // PPO_BWD_SMALL_MAX_TILES: three-product backward up to this many tiles,
    int64_t bwd_small_max_tiles_split = 0;    // PPO_BWD_SMALL_MAX_TILES_SPLIT: ... or this many while the split backward covers
    int64_t fwd_split_max_states = 512;       // PPO_FWD_SPLIT_MAX_STATES: 2 or 4 waves per state up to this many states
    int64_t fwd_x6_max_states = 1 << 30;      // PPO_FWD_SPLIT_MAX_TILES: split-fp32 train forward up to this many STATES
    // its two-tile form from this many tiles on (0 = never): [0] HID = 128, PPO_FWD_SPLIT_T2_MIN_TILES_128 (measured: train
    // forward 0.0570 -> 0.0548 ms at 4096 states); [1] HID = 256, PPO_FWD_SPLIT_T2_MIN_TILES
    int64_t fwd_x6_t2_min_tiles[2] = {1024, 1536};
    int32_t fuse_reduce_adam = 1;             // PPO_FUSE_REDUCE_ADAM: single-rank Adam in the slab-reduction launch
    // rollout
    int32_t rollout_persistent = -1;          // PPO_ROLLOUT_PERSISTENT: 0 / 1, -1 = one launch for Q = 8
    int32_t rollout_compact = -1;             // PPO_ROLLOUT_COMPACT: 0 / 1, -1 = compact above compact_auto_bytes or with a sink
    double compact_auto_bytes = 32.0 * 1024 * 1024 * 1024;   // PPO_COMPACT_AUTO_BYTES
    int64_t rollout_split_max_envs = 512;     // PPO_ROLLOUT_SPLIT_MAX_ENVS: 2 or 4 waves per env up to this many envs
};
const PpoKnobs& ppo_knobs();

// What one training pass minimises: the policy's clipped PPO loss with its entropy bonus, or a critic's (a ppo_policy_t
// read as a state value) Flux.mse against a target column, or the policy's cross-entropy on the buffer's actions (behaviour
// cloning), or its cross-entropy against a target distribution per state (policy distillation).
// TrainObjective: the loss inputs of one pass
// PolicyAnchored: Policy plus a coefficient times Distill's cross-entropy, while the handle has a KL anchor.
enum class Objective { Policy, Value, Imitate, Distill, PolicyAnchored };
struct TrainObjective {
    Objective kind;
    // Policy
    double eps = 0.0, entropy_weight = 0.0;
    int32_t adv_mode = PPO_ADV_RETURNS;
    float* ratio_dst = nullptr;        // where the pass stores its probability ratios while a target_kl is set (nullptr: the
                                       // policy's minibatch buffer)
    // Value
    const float* target_col = nullptr; // regression target indexed by transition id
    const float* vold_col = nullptr;   // clipped value loss: the values the critic had before the update, by transition id
                                       // (train_pass_dev fills it and vclip from the critic handle and the buffer)
    float vclip = 0.0f;                // ... and the clip range
    float* vdelta_dst = nullptr;       // where the pass stores V - vold per state while the clip is set (nullptr: nowhere)
    // Imitate (entropy_weight and adv_mode as for Policy; adv_mode names the weights' column, read in the weighted form only)
    int32_t weight_mode = PPO_IMITATE_UNIFORM;
    // Distill (entropy_weight, adv_mode and weight_mode as for Imitate): the target rows [T*N][A] by transition id
    const float* distill_targets = nullptr;
    // PolicyAnchored (eps, entropy_weight, adv_mode and ratio_dst as for Policy): the target rows, the coefficient of this pass
    // and where it stores the divergence per state (nullptr: the policy's minibatch buffer)
    const float* anchor_targets = nullptr;
    double anchor_coef = 0.0;
    float* anchor_dst = nullptr;
};

// The kernels that run one training minibatch.  TrainTile runs forward, loss and backward-data in one launch and is
// always followed by Wgrad (k_policy_wgrad<TR = true>).  Objective::Value: the forward is always Fwd -- k_policy_fwd in a
// value-train mode, the only forward with one -- followed by the backward the policy would take at that shape and size; where
// that is the one-tile pass, whose weight-gradient kernel only runs from inside it, the three-product Small backward.
// Objective::Imitate: likewise, k_policy_fwd in an imitation mode (12 / 13).  Objective::Distill: likewise, modes 17 / 18.
// Objective::PolicyAnchored: likewise, modes 20 / 21.
enum class TrainFwd { None, TrainTile, X6S, X6T, X6, Split, Fwd, Bf16 };
enum class TrainBwd { None, Wgrad, Small, X6, Fused, Bf16 };
struct TrainRoute { TrainFwd fwd; TrainBwd bwd; const char* err; };      // err: why fwd is None
// dtype: PPO_DTYPE_*; HID: kernel width (128 / 256); H: rows per state (32 / 128); states: minibatch size
TrainRoute train_route(int32_t dtype, int F, int HID, int L, int H, bool compact, int64_t states, const PpoKnobs& k, Objective obj);

// k_policy_fwd's MODE (k_policy_fwd_bf16 has the first five).  The numbers are what kernel traces, the route strings and DESIGN.md
// print.  A mode is two independent choices, where the state comes from and what runs behind the logits: fwd_traits is the table.
// The clipped value loss, the forced step, imitation, distillation and the selection rules are modes of their own rather than
// runtime tests in a tail because every such test moved the register allocation of the instantiations next to it, measurably
// (DESIGN.md 7k .. 7n, 7q)
enum class FwdMode : int {
    Probs = 0, Sample = 1, Train = 2, Persistent = 3, TrainSnap = 4, ValuePredict = 5, ValueTrain = 6, ValuePredictSnap = 7,
    ValueTrainSnap = 8, ValueTrainClip = 9, ValueTrainClipSnap = 10, Forced = 11, Imitate = 12, ImitateSnap = 13, Tempered = 14,
    Greedy = 15, Truncated = 16, Distill = 17, DistillSnap = 18, ProbsSnap = 19, TrainAnchored = 20, TrainAnchoredSnap = 21
};
enum class FwdSource {
    Rows,       // observation rows [B][H][F] in storage order
    RowsIdx,    // ... gathered through idx (a minibatch)
    EnvSlots,   // the env slots of the persistent rollout, in the wave's LDS
    Snap,       // one env snapshot [2V] per state in storage order, the rows re-derived from it
    SnapIdx     // ... fetched through idx, the rows left in xs_out (minibatch order) for the backward
};
enum class FwdTail {      // policy_tail, or value_tail for the three Value*
    Probs, Sample, SamplePersistent, Train, Forced, Imitate, Tempered, Greedy, Truncated, ValuePredict, ValueTrain, ValueTrainClip,
    Distill, TrainAnchored
};
struct FwdTraits { FwdSource src; FwdTail tail; };
constexpr FwdTraits fwd_traits(FwdMode m) {
    switch (m) {
    case FwdMode::Probs:              return {FwdSource::Rows, FwdTail::Probs};
    case FwdMode::Sample:             return {FwdSource::Rows, FwdTail::Sample};
    case FwdMode::Train:              return {FwdSource::RowsIdx, FwdTail::Train};
    case FwdMode::Persistent:         return {FwdSource::EnvSlots, FwdTail::SamplePersistent};
    case FwdMode::TrainSnap:          return {FwdSource::SnapIdx, FwdTail::Train};
    case FwdMode::ValuePredict:       return {FwdSource::Rows, FwdTail::ValuePredict};
    case FwdMode::ValueTrain:         return {FwdSource::RowsIdx, FwdTail::ValueTrain};
    case FwdMode::ValuePredictSnap:   return {FwdSource::Snap, FwdTail::ValuePredict};
    case FwdMode::ValueTrainSnap:     return {FwdSource::SnapIdx, FwdTail::ValueTrain};
    case FwdMode::ValueTrainClip:     return {FwdSource::RowsIdx, FwdTail::ValueTrainClip};
    case FwdMode::ValueTrainClipSnap: return {FwdSource::SnapIdx, FwdTail::ValueTrainClip};
    case FwdMode::Forced:             return {FwdSource::Rows, FwdTail::Forced};
    case FwdMode::Imitate:            return {FwdSource::RowsIdx, FwdTail::Imitate};
    case FwdMode::ImitateSnap:        return {FwdSource::SnapIdx, FwdTail::Imitate};
    case FwdMode::Tempered:           return {FwdSource::Rows, FwdTail::Tempered};
    case FwdMode::Greedy:             return {FwdSource::Rows, FwdTail::Greedy};
    case FwdMode::Truncated:          return {FwdSource::Rows, FwdTail::Truncated};
    case FwdMode::Distill:            return {FwdSource::RowsIdx, FwdTail::Distill};
    case FwdMode::DistillSnap:        return {FwdSource::SnapIdx, FwdTail::Distill};
    case FwdMode::ProbsSnap:          return {FwdSource::Snap, FwdTail::Probs};
    case FwdMode::TrainAnchored:      return {FwdSource::RowsIdx, FwdTail::TrainAnchored};
    case FwdMode::TrainAnchoredSnap:  return {FwdSource::SnapIdx, FwdTail::TrainAnchored};
    }
    return {FwdSource::Rows, FwdTail::Probs};
}
constexpr bool src_snapshot(FwdSource s) { return s == FwdSource::Snap || s == FwdSource::SnapIdx; }
constexpr bool tail_value(FwdTail t) { return t == FwdTail::ValuePredict || t == FwdTail::ValueTrain || t == FwdTail::ValueTrainClip; }
// train forward: saves the activations, writes dY and the loss terms
constexpr bool tail_trains(FwdTail t) {
    return t == FwdTail::Train || t == FwdTail::Imitate || t == FwdTail::Distill || t == FwdTail::TrainAnchored || t == FwdTail::ValueTrain ||
           t == FwdTail::ValueTrainClip;
}
// logits times 1 / temperature in front of the softmax
constexpr bool tail_tempers(FwdTail t) { return t == FwdTail::Tempered || t == FwdTail::Greedy || t == FwdTail::Truncated; }
// rand(Categorical): the Philox uniform and the CDF walk
constexpr bool tail_samples(FwdTail t) { return t == FwdTail::Sample || t == FwdTail::SamplePersistent || t == FwdTail::Tempered || t == FwdTail::Truncated; }
// one rollout step: an action, its probability and (on request) the whole distribution go to the output columns
constexpr bool tail_steps(FwdTail t) { return tail_samples(t) || t == FwdTail::Greedy || t == FwdTail::Forced; }
// the train mode the launchers run for an objective (clipped: the critic's clipped value loss), and the one the route strings
// name: the clip is chosen at launch, while a value clip is set, and the routes keep naming 6 / 8
constexpr FwdMode fwd_train_mode(Objective obj, bool compact, bool clipped = false) {
    switch (obj) {
    case Objective::Value:
        if (clipped) return compact ? FwdMode::ValueTrainClipSnap : FwdMode::ValueTrainClip;
        return compact ? FwdMode::ValueTrainSnap : FwdMode::ValueTrain;
    case Objective::Imitate: return compact ? FwdMode::ImitateSnap : FwdMode::Imitate;
    case Objective::Distill: return compact ? FwdMode::DistillSnap : FwdMode::Distill;
    case Objective::PolicyAnchored: return compact ? FwdMode::TrainAnchoredSnap : FwdMode::TrainAnchored;
    default: return compact ? FwdMode::TrainSnap : FwdMode::Train;
    }
}
constexpr FwdMode fwd_route_mode(Objective obj, bool compact) { return fwd_train_mode(obj, compact, false); }

// train-pass launchers: each launches what train_route chose and checks nothing else
int32_t launch_policy_train_fwd(ppo_policy_s* p, ppo_rollouts_s* ro, const int32_t* idx_dev, int64_t B,
                                int64_t B_global, double eps, double entropy_weight, const float* adv_col, TrainFwd form);
int32_t launch_policy_bwd(ppo_policy_s* p, ppo_rollouts_s* ro, const int32_t* idx_dev, int64_t B);
// critic (ppo_policy_fwd.hip value modes): state values of B stored states (rows, or snapshots when cstate_dev is given), and
// the value-train forward of a minibatch against target_col (indexed by transition id); vold_col (likewise indexed, optional):
// the clipped value loss with range vclip, V - vold of every state to vdelta_dst (optional, minibatch order)
int32_t launch_value_predict(ppo_policy_s* p, const int8_t* states_dev, const int8_t* cstate_dev, const uint32_t* active_dev,
                             const int8_t* tmpl_dev, int32_t V, int64_t B, int32_t H, float* values_dev);
int32_t launch_value_train_fwd(ppo_policy_s* p, ppo_rollouts_s* ro, const int32_t* idx_dev, int64_t B, int64_t B_global,
                               const float* target_col, const float* vold_col, float vclip, float* vdelta_dst);
// imitation train forward (k_policy_fwd's FwdMode::Imitate / ImitateSnap): cross-entropy of the buffer's actions, weighted by
// max(weight_col[transition], 0) (nullptr: uniform weights), plus the policy's entropy term
int32_t launch_imitate_train_fwd(ppo_policy_s* p, ppo_rollouts_s* ro, const int32_t* idx_dev, int64_t B, int64_t B_global,
                                 double entropy_weight, const float* weight_col);
// distillation train forward (k_policy_fwd's FwdMode::Distill / DistillSnap): cross-entropy against the target row
// target_ptr[transition][A] (full_probs' layout), weighted like imitation's, plus the policy's entropy term
int32_t launch_distill_train_fwd(ppo_policy_s* p, ppo_rollouts_s* ro, const int32_t* idx_dev, int64_t B, int64_t B_global,
                                 double entropy_weight, const float* weight_col, const float* target_ptr);
// KL-anchored train forward (k_policy_fwd's FwdMode::TrainAnchored / TrainAnchoredSnap): launch_policy_train_fwd's
// surrogate and entropy term plus beta times the cross-entropy against target_ptr[transition][A]; the ratios go where
// p->ratio_out points, the divergence per state to anchor_dst (minibatch order)
int32_t launch_anchored_train_fwd(ppo_policy_s* p, ppo_rollouts_s* ro, const int32_t* idx_dev, int64_t B, int64_t B_global,
                                  double eps, double entropy_weight, const float* adv_col, const float* target_ptr, double beta,
                                  float* anchor_dst);
// launch_policy_probs from env snapshots [B][2V] in storage order (k_policy_fwd's FwdMode::ProbsSnap; fp32 policies, F = 72)
int32_t launch_policy_probs_snap(ppo_policy_s* p, const int8_t* cstate_dev, const uint32_t* active_dev, const int8_t* tmpl_dev,
                                 int32_t V, int64_t B, int32_t H, float* probs_dev);
// the same fused backward with its row contractions (dW2, dW1) as split-fp32 products on the bf16 matrix pipe
// (ppo_policy_bwd_x6.hip)
int32_t launch_policy_bwd_x6(ppo_policy_s* p, ppo_rollouts_s* ro, const int32_t* idx_dev, int64_t B);
// three-product backward of an fp32 policy (ppo_policy_bwd_small.hip); dz1f (dz2f, dzm where the layers exist) allocated.
// tr_tail_wg > 0: only its weight-gradient kernel, on the operand-layout tiles k_policy_train_tile left in act1 / dz2f /
// dz1f from that many workgroups (the slabs holding the small-gradient tails)
int32_t launch_policy_bwd_small(ppo_policy_s* p, ppo_rollouts_s* ro, const int32_t* idx_dev, int64_t B, int tr_tail_wg = 0);
// forward + loss + backward-data of a tile in one workgroup, then the weight-gradient kernel (ppo_policy_train_tile.hip)
int32_t launch_policy_train_tile(ppo_policy_s* p, ppo_rollouts_s* ro, const int32_t* idx_dev, int64_t B, int64_t B_global,
                                 double eps, double entropy_weight, const float* adv_col);
// bf16 compute mode (ppo_policy_bf16.hip): k_policy_fwd's modes Probs, Sample, Train and TrainSnap
struct FwdArgs;
// one-launch rollout with 2 or 4 waves per env for few envs, bit-identical results (ppo_policy_rollout_split.hip)
int32_t launch_rollout_split(ppo_policy_s* p, FwdArgs& a, int64_t N, int tps, int V, int env);
// train forward with 2 or 4 waves per state for small minibatches (ppo_policy_fwd_split.hip)
int32_t launch_policy_train_fwd_split(ppo_policy_s* p, FwdArgs& a, int64_t B, bool compact);
// train forward with its Dense products as split-fp32 MFMAs (ppo_policy_fwd_x6.hip); form: X6S, X6T or X6
int32_t launch_policy_train_fwd_x6(ppo_policy_s* p, FwdArgs& a, int64_t B, TrainFwd form, bool compact);
int32_t launch_policy_fwd_bf16(ppo_policy_s* p, FwdArgs& args, FwdMode mode, int64_t B, int tps);
int32_t launch_policy_rollout_persistent_bf16(ppo_policy_s* p, FwdArgs& args, int64_t N, int tps, int V);
int32_t launch_policy_bwd_bf16(ppo_policy_s* p, ppo_rollouts_s* ro, const int32_t* idx_dev, int64_t B);
static inline int bf16_ks1(int F) { return (F + 15) / 16; }     // layer-1 k-steps of 16 (zero padded)
// fuse (optional): apply the optimiser (Adam, or a chain: k_reduce_chain) + re-pack in the same launch (single-rank training); hist2: the per-batch loss pair of that step
int32_t launch_grad_reduce(ppo_policy_s* p, int64_t B, int64_t B_global, double entropy_weight, ppo_adam_s* fuse = nullptr, float* hist2 = nullptr);
int64_t clip_slot_count(const ppo_policy_s* p);                     // ClipNorm partial-sum slots either launch pair writes
int32_t launch_adam(ppo_adam_s* o, float* hist2_or_null);           // any handle: a chain other than Adam alone -> k_chain_update
int32_t launch_categorical(const float* probs, const float* u, int64_t B, int64_t A, int32_t* actions, float* psel,
                           int32_t* err);
// ppo_stats.hip -- fixed-order fp64 reductions; part: workspace of stats_part_doubles() doubles, the results land in its
// first 4 (ratio statistics: sum(-log r), sum((r - 1) - log r), count(|r - 1| > eps), n) resp. 5 (value moments) doubles
size_t stats_part_doubles();
int32_t launch_ratio_stats(const float* ratio, int64_t n, double eps, double* part);
// (sum x, n) of a column of n floats in the first 2 doubles
int32_t launch_sum_stats(const float* col, int64_t n, double* part);
// value-clip statistics over n deltas V - vold: count(|delta| > c), sum delta^2, n in the first 3 doubles
int32_t launch_value_clip_stats(const float* delta, int64_t n, float c, double* part);
// over the transitions with valid[i] != 0 of [0, n): n, sum x, sum x^2, sum y, sum y^2 with x = t - t[i0], y = (t - v) - (t - v)[i0],
// i0 = first_id[0] (a valid transition: the first of the dataset)
int32_t launch_value_moments(const float* target, const float* values, const uint8_t* valid, const int32_t* first_id,
                             int64_t n, double* part);
int32_t launch_feistel_index(const int32_t* index_dev, int64_t len, uint64_t seed, uint32_t epoch, int32_t* out_dev);
