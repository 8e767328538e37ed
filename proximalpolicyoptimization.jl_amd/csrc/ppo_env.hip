// ppo_env.hip -- K1: batched synthetic rand-poly-shaped env (plugin contract
// src/ProximalPolicyOptimization.jl:16-20; tensor shapes test/quad_game_utilities.jl:39-59,95-110).
// QuadMeshGame's dynamics are not in the reference tree, so this is an honest synthetic stand-in
// with exactly specified integer dynamics (DESIGN.md "Synthetic env"): SoA state in HBM, one
// thread per env for the integer update, one thread per output dword for the observation.
#include <algorithm>
#include "ppo_env_device.h"

struct EnvView {
    int8_t* score; int8_t* degree; uint32_t* active; int32_t* steps; float* reward; uint8_t* done;
    uint32_t* episode; uint32_t* tick; int32_t* err; int32_t* episodes_left; const int8_t* tmpl;
    int32_t Q, V, max_actions; float no_action_reward; int64_t N, global_offset; uint32_t k0, k1;
};

static EnvView view_of(ppo_env_s* e) {
    EnvView v;
    v.score = e->score.p; v.degree = e->degree.p; v.active = e->active.p; v.steps = e->steps.p;
    v.reward = e->reward.p; v.done = e->done.p; v.episode = e->episode.p; v.tick = e->tick.p; v.err = e->err.p;
    v.episodes_left = e->episodes_left.p; v.tmpl = e->tmpl.p;
    v.Q = e->Q; v.V = e->V; v.max_actions = e->max_actions; v.no_action_reward = e->no_action_reward;
    v.N = e->N; v.global_offset = e->global_offset; v.k0 = (uint32_t)e->seed; v.k1 = (uint32_t)(e->seed >> 32);
    return v;
}

static __device__ __forceinline__ EnvConst const_of(const EnvView& e) {
    EnvConst c;
    c.Q = e.Q; c.V = e.V; c.max_actions = e.max_actions; c.no_action_reward = e.no_action_reward; c.k0 = e.k0; c.k1 = e.k1;
    return c;
}
static __device__ __forceinline__ EnvRef ref_of(const EnvView& e, int64_t n) {
    EnvRef r;
    r.sc = e.score + n * e.V; r.dg = e.degree + n * e.V; r.active = e.active + n; r.steps = e.steps + n;
    r.reward = e.reward + n; r.done = e.done + n; r.episode = e.episode + n; r.tick = e.tick + n;
    return r;
}
__device__ __forceinline__ void env_reset_one(const EnvView& e, int64_t n) {
    env_reset_ref(const_of(e), ref_of(e, n), (uint32_t)(e.global_offset + n));
}

__global__ void k_env_reset(EnvView e, int only_done) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= e.N) return;
    if (only_done && !e.done[n]) return;
    env_reset_one(e, n);
}

// step!(env, a) for every env + record reward/is_terminal + optional auto-reset
// (call order src/collect_rollouts.jl:9-12; reset before the next episode src/rollout_buffer.jl:75).
// ev.kind != 0 (episodes mode only): the evaluator variants' per-episode values are tracked here, one thread per env --
// best_single_trajectory_return / single_trajectory_normalized_return (test/quad_game_utilities.jl:280-296,369-378) and
// single_trajectory_return (src/evaluate.jl:1-16).  env.current_score = sum |vertex score| over the active quads,
// env.opt_score = |sum of vertex scores| (the synthetic env's termination test uses the same two numbers).
__global__ void k_env_step(EnvView e, const int32_t* __restrict__ actions, float* __restrict__ reward_out,
                           uint8_t* __restrict__ done_out, uint8_t* __restrict__ valid_out, int auto_reset,
                           int episodes_mode, EvalView ev) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= e.N) return;
    if (episodes_mode && e.episodes_left[n] <= 0) {          // this env already played its episodes
        if (valid_out) valid_out[n] = 0;
        if (reward_out) reward_out[n] = 0.0f;
        if (done_out) done_out[n] = 1;
        return;
    }
    const EnvRef er = ref_of(e, n);
    int64_t slot = 0;
    if (ev.kind) {
        const int64_t q = ev.num_traj / e.N, rem = ev.num_traj % e.N;
        slot = n * q + (n < rem ? n : rem) + ev.ep_count[n];          // env n's episodes are consecutive in `out`
        if (*er.steps == 0) {                                        // first step! of an episode: the values at reset!
            const uint32_t act = *er.active;
            const int cur = env_total_abs(er.sc, act, e.Q), sum = env_total_sum(er.sc, act, e.Q);
            const int mr = cur - (sum < 0 ? -sum : sum);
            if (ev.kind == 3 && mr == 0) {
                // single_trajectory_normalized_return: maxreturn == 0 -> 1.0 and the episode is not played (:372-373).
                // The action sampled for this state is dropped; the next step sees the env's next episode.
                ev.out[slot] = 1.0;
                ev.ep_count[n] += 1;
                const int left = e.episodes_left[n] - 1;
                e.episodes_left[n] = left;
                if (left > 0) env_reset_one(e, n);
                if (valid_out) valid_out[n] = 0;
                if (reward_out) reward_out[n] = 0.0f;
                if (done_out) done_out[n] = 1;
                return;
            }
            ev.ep_ret[n] = 0.0; ev.ep_init[n] = cur; ev.ep_min[n] = cur; ev.ep_maxret[n] = mr;
        }
    }
    float rew; uint8_t dn;
    int score_after = 0;
    const int errf = env_step_ref(const_of(e), er, actions[n], rew, dn, &score_after);
    if (errf) atomicOr(e.err, errf);
    if (errf & 4) return;                          // step! on a terminated env: nothing recorded (as before)
    if (reward_out) reward_out[n] = rew;
    if (done_out) done_out[n] = dn;
    if (valid_out) valid_out[n] = 1;
    if (ev.kind) {
        const double ret = ev.ep_ret[n] + (double)rew;               // ret += reward(env)   src/evaluate.jl:13
        const int mn = min(ev.ep_min[n], score_after);               // minscore = min(minscore, env.current_score)
        ev.ep_ret[n] = ret; ev.ep_min[n] = mn;
        if (dn) {
            const int best = ev.ep_init[n] - mn;                     // initial_score - minscore
            ev.out[slot] = ev.kind == 1 ? ret : (ev.kind == 2 ? (double)best : (double)best / (double)ev.ep_maxret[n]);
            ev.ep_count[n] += 1;
        }
    }
    if (dn) {
        if (episodes_mode) {
            const int left = e.episodes_left[n] - 1;
            e.episodes_left[n] = left;
            if (left > 0) env_reset_one(e, n);
        } else if (auto_reset) {
            env_reset_one(e, n);
        }
    }
}

// The episodes-mode step with the bookkeeping of best_state_in_rollout (test/quad_game_utilities.jl:341-358): the reference
// keeps a copy of the wrapper behind every step and returns the one at argmin(current_score - opt_score); here the env's
// thread keeps the best state so far in the trajectory's output slot and replaces it only on a STRICTLY lower gap (argmin
// returns the first minimum; the start state is candidate 0).  Also single_trajectory_scores (:309-323: initial_score -
// current_score behind every step), the action types count_non_flips counts (test/random_quad.jl:9-27) and, optionally, the
// action history: the action played at step t in entry t - 1 of the slot's row.  Same idle
// branch, env_step_ref call, outputs and reset-on-done as k_env_step's episodes mode; the snapshot copies are dword copies
// (V % 4 == 0, rows start dword aligned).
__global__ void k_env_step_track(EnvView e, const int32_t* __restrict__ actions, float* __restrict__ reward_out,
                                 uint8_t* __restrict__ done_out, uint8_t* __restrict__ valid_out, TrackView tv) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= e.N) return;
    const int64_t q = tv.num_traj / e.N, rem = tv.num_traj % e.N;
    const int64_t slot = n * q + (n < rem ? n : rem) + tv.ep_count[n];   // env n's trajectories are consecutive
    if (e.episodes_left[n] <= 0 || slot >= tv.num_traj) {                // this env already played its trajectories
        if (valid_out) valid_out[n] = 0;
        if (reward_out) reward_out[n] = 0.0f;
        if (done_out) done_out[n] = 1;
        return;
    }
    const EnvRef er = ref_of(e, n);
    const int dv = e.V / 4;
    uint32_t* __restrict__ bs = reinterpret_cast<uint32_t*>(tv.best_state + slot * 2 * e.V);
    const uint32_t* sc4 = reinterpret_cast<const uint32_t*>(er.sc);
    const uint32_t* dg4 = reinterpret_cast<const uint32_t*>(er.dg);
    int t = tv.t_in[n];
    int best_gap;
    if (t == 0) {                                                        // first step! of a trajectory: the start state
        const uint32_t act = *er.active;
        const int cur = env_total_abs(er.sc, act, e.Q), sum = env_total_sum(er.sc, act, e.Q);
        best_gap = cur - (sum < 0 ? -sum : sum);
        for (int d = 0; d < dv; ++d) { bs[d] = sc4[d]; bs[dv + d] = dg4[d]; }
        tv.best_active[slot] = act; tv.best_gap[slot] = best_gap; tv.best_step[slot] = 0; tv.initial_gap[slot] = best_gap;
        tv.ep_init[n] = cur;
    } else {
        best_gap = tv.best_gap[slot];
    }
    const int a = actions[n];
    float rew; uint8_t dn;
    int score_after = 0;
    const int errf = env_step_ref(const_of(e), er, a, rew, dn, &score_after);
    if (errf) atomicOr(e.err, errf);
    if (errf & 4) return;                          // step! on a terminated env: nothing recorded
    if (reward_out) reward_out[n] = rew;
    if (done_out) done_out[n] = dn;
    if (valid_out) valid_out[n] = 1;
    t += 1;
    const uint32_t act = *er.active;
    const int sum = env_total_sum(er.sc, act, e.Q);
    const int gap = score_after - (sum < 0 ? -sum : sum);
    if (gap < best_gap) {
        for (int d = 0; d < dv; ++d) { bs[d] = sc4[d]; bs[dv + d] = dg4[d]; }
        tv.best_active[slot] = act; tv.best_gap[slot] = gap; tv.best_step[slot] = t;
    }
    if (tv.trace && t <= e.max_actions) tv.trace[slot * e.max_actions + (t - 1)] = tv.ep_init[n] - score_after;
    if (tv.type_counts) tv.type_counts[slot * 4 + ((a < 0 || a >= 16 * e.Q) ? 0 : (a & 3))] += 1;
    if (tv.actions && t <= e.max_actions) tv.actions[slot * e.max_actions + (t - 1)] = (int16_t)a;   // the action history
    if (dn) {
        tv.length[slot] = t;
        tv.ep_count[n] += 1;
        tv.t_in[n] = 0;
        const int left = e.episodes_left[n] - 1;
        e.episodes_left[n] = left;
        if (left > 0) env_reset_one(e, n);
    } else {
        tv.t_in[n] = t;
    }
}

// best-of-K search, load: one thread per dword of every env's state.  Env n < busy takes start n / K (clone n % K) and is
// left as reset! leaves an env, with one episode to play; the others idle
__global__ void k_env_load_starts(EnvView e, const uint32_t* __restrict__ start_state, const uint32_t* __restrict__ start_active,
                                  int64_t busy, int64_t K, int32_t* __restrict__ t_in) {
    const int dv = e.V / 4;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = gid / (2 * dv);
    if (n >= e.N) return;
    const int d = (int)(gid - n * 2 * dv);
    if (n >= busy) {
        if (d == 0) e.episodes_left[n] = 0;
        return;
    }
    const int64_t s = n / K;
    int8_t* dst = (d < dv) ? (e.score + n * e.V) : (e.degree + n * e.V);
    reinterpret_cast<uint32_t*>(dst)[d < dv ? d : d - dv] = start_state[s * 2 * dv + d];
    if (d == 0) {
        e.active[n] = start_active[s]; e.steps[n] = 0; e.reward[n] = 0.0f; e.done[n] = 0;
        e.episodes_left[n] = 1; t_in[n] = 0;
    }
}

// best-of-K search, reduction: one workgroup per start.  Threads stride over the K clones (envs s*K ..) holding
// min(gap << 32 | clone) -- a gap is sum|s| - |sum s| >= 0, so the unsigned order is the order of (gap, clone) and ties go to
// the lowest clone -- then a wave reduction by shuffles, one LDS exchange across the four waves, and the whole workgroup
// copies the winner's record -- and, where out.actions is set, the path to it: the first best_step entries of the winner's
// action history (tv.actions, rows of M = max_actions entries), -1 behind them
__global__ __launch_bounds__(256) void k_search_argmin(TrackView tv, int V, int64_t K, TrackView out,
                                                       int32_t* __restrict__ best_clone, int32_t* __restrict__ clone_gaps,
                                                       int64_t out_base, int M) {
    __shared__ unsigned long long wave_min[4];
    const int tid = threadIdx.x;
    const int64_t s = blockIdx.x, o = out_base + s;
    unsigned long long best = ~0ull;
    for (int64_t c = tid; c < K; c += 256) {
        const int g = tv.best_gap[s * K + c];
        if (clone_gaps) clone_gaps[o * K + c] = g;
        const unsigned long long key = ((unsigned long long)(uint32_t)g << 32) | (unsigned long long)(uint32_t)c;
        best = key < best ? key : best;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t hi = __shfl_xor((uint32_t)(best >> 32), off), lo = __shfl_xor((uint32_t)best, off);
        const unsigned long long other = ((unsigned long long)hi << 32) | lo;
        best = other < best ? other : best;
    }
    if ((tid & 63) == 0) wave_min[tid >> 6] = best;
    __syncthreads();
    best = wave_min[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) best = wave_min[w] < best ? wave_min[w] : best;
    const int64_t clone = (int64_t)(uint32_t)best, env = s * K + clone;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(tv.best_state + env * 2 * V);
    uint32_t* dst = reinterpret_cast<uint32_t*>(out.best_state + o * 2 * V);
    for (int d = tid; d < V / 2; d += 256) dst[d] = src[d];
    if (out.actions) {
        const int len = tv.best_step[env];
        const int16_t* hist = tv.actions + env * M;
        int16_t* path = out.actions + o * M;
        for (int i = tid; i < M; i += 256) path[i] = i < len ? hist[i] : (int16_t)-1;
    }
    if (tid == 0) {
        out.best_active[o] = tv.best_active[env]; out.best_gap[o] = tv.best_gap[env]; out.best_step[o] = tv.best_step[env];
        out.initial_gap[o] = tv.initial_gap[env]; best_clone[o] = (int32_t)clone;
    }
}

// resampling search, one event: one workgroup per start, fold -> rank -> copy.
//   fold   k_search_argmin's reduction over the K records of the start (terminal clones included); the winner's record goes
//          to the start's output record on the round's first fold (flags & 1), afterwards only on a STRICTLY lower gap.  A
//          barrier separates it from the copies, which overwrite receivers' records.  flags & 2: the fold is all that runs.
//   rank   live clones (done == 0) by (cur_gap, clone), cur_gap recomputed from the env's score bytes; the keys
//          cur_gap << 32 | clone sit in LDS (~0 for a terminal clone) and a clone's rank is the number of lower keys: every
//          lane of a wave reads the same LDS address, a broadcast.  Ranks below m = min(survivors, live) keep their state.
//   copy   the clone of rank rho >= m takes state, record and t_in of the clone of rank (rho - m) % m: scalars by one thread
//          per clone, score / degree / best_state as dwords across the workgroup.  Donors are never receivers: in place.
// Dynamic LDS, 48 + 12 * Kp bytes (Kp = K rounded up to 8): wave_min [4], live count, keys [Kp], by_rank [Kp], rank_of [Kp];
// every carve offset is a multiple of 16.
// PATH: the action history (tv.actions, rows of M = max_actions entries) belongs to the lineage.  A fold that
// takes the winner's record also writes the first best_step entries of the winner's history to the start's output path
// (out.actions) and -1 behind them -- read, like the snapshot, before the barrier that releases the copies, since the winner
// may be a receiver of this event.  A copy takes the donor's entries 0 .. t_in - 1 with its t_in (at most `played`, the loop
// steps of the round so far).  PATH = false compiles to the event without any of it.
// VALUE: the rank key of a live clone is ord(s) << 32 | clone with s = fmaf(-w, v, (float)cur_gap) in fp32,
// v = values[env] (0.0f where that is not finite) and ord the monotone map of fp32 bits to uint32 (all bits flipped under a
// set sign bit, else the sign bit set).  s is never NaN (w, v and cur_gap are finite), so no live key is ~0.  `values` is
// a buffer of its own, written before the launch from the states the clones hold and touched by no copy; it is read here,
// in front of the barrier that releases the copies.  event_values (optional): [..][E][K] log, row `event`: the raw
// values[env] of a live clone, a quiet NaN for a terminal one.  Fold, ranks, copy and LDS are the event's own; VALUE = false
// compiles to the event without any of it.
extern __shared__ __attribute__((aligned(16))) unsigned char resample_lds[];
template <bool PATH, bool VALUE>
__global__ __launch_bounds__(256) void k_search_resample(EnvView e, TrackView tv, int K, int survivors, int flags,
                                                         TrackView out, int32_t* __restrict__ best_clone, int64_t out_base,
                                                         int32_t* __restrict__ donors, int64_t E, int64_t event,
                                                         int32_t* __restrict__ clone_gaps, int M, int played,
                                                         const float* __restrict__ values, float* __restrict__ event_values,
                                                         float value_weight) {
    unsigned long long* wave_min = reinterpret_cast<unsigned long long*>(resample_lds);
    int* live_count = reinterpret_cast<int*>(resample_lds + 32);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(resample_lds + 48);
    const int Kp = (K + 7) & ~7;
    uint16_t* by_rank = reinterpret_cast<uint16_t*>(keys + Kp);
    uint16_t* rank_of = by_rank + Kp;
    const int tid = threadIdx.x, V = e.V, dv = V / 4;
    const int64_t s = blockIdx.x, o = out_base + s, env0 = s * K;
    // ---- fold
    const int out_gap = (flags & 1) ? 0 : out.best_gap[o];               // read by everyone before the barrier below
    if (tid == 0) *live_count = 0;
    unsigned long long best = ~0ull;
    for (int c = tid; c < K; c += 256) {
        const int g = tv.best_gap[env0 + c];
        if (clone_gaps) clone_gaps[o * K + c] = g;
        const unsigned long long key = ((unsigned long long)(uint32_t)g << 32) | (unsigned long long)(uint32_t)c;
        best = key < best ? key : best;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t hi = __shfl_xor((uint32_t)(best >> 32), off), lo = __shfl_xor((uint32_t)best, off);
        const unsigned long long other = ((unsigned long long)hi << 32) | lo;
        best = other < best ? other : best;
    }
    if ((tid & 63) == 0) wave_min[tid >> 6] = best;
    __syncthreads();
    best = wave_min[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) best = wave_min[w] < best ? wave_min[w] : best;
    if ((flags & 1) || (int)(uint32_t)(best >> 32) < out_gap) {
        const int64_t wenv = env0 + (int64_t)(uint32_t)best;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(tv.best_state + wenv * 2 * V);
        uint32_t* dst = reinterpret_cast<uint32_t*>(out.best_state + o * 2 * V);
        for (int d = tid; d < 2 * dv; d += 256) dst[d] = src[d];
        if (PATH) {
            const int len = tv.best_step[wenv];
            const int16_t* hist = tv.actions + wenv * M;
            int16_t* path = out.actions + o * M;
            for (int i = tid; i < M; i += 256) path[i] = i < len ? hist[i] : (int16_t)-1;
        }
        if (tid == 0) {
            out.best_active[o] = tv.best_active[wenv]; out.best_gap[o] = tv.best_gap[wenv];
            out.best_step[o] = tv.best_step[wenv]; out.initial_gap[o] = tv.initial_gap[wenv];
            best_clone[o] = (int32_t)(uint32_t)best;
        }
    }
    if (flags & 2) return;
    // ---- rank
    for (int c = tid; c < K; c += 256) {
        const int64_t n = env0 + c;
        unsigned long long key = ~0ull;
        if (!e.done[n]) {
            const uint32_t act = e.active[n];
            const int8_t* sc = e.score + n * V;
            const int cur = env_total_abs(sc, act, e.Q), sum = env_total_sum(sc, act, e.Q);
            uint32_t hi = (uint32_t)(cur - (sum < 0 ? -sum : sum));
            if (VALUE) {
                const float raw = values[n];
                if (event_values) event_values[(o * E + event) * K + c] = raw;
                const float v = (__float_as_uint(raw) & 0x7F800000u) == 0x7F800000u ? 0.0f : raw;      // inf / NaN rank as 0
                const uint32_t b = __float_as_uint(fmaf(-value_weight, v, (float)(int)hi));
                hi = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
            }
            key = ((unsigned long long)hi << 32) | (unsigned long long)(uint32_t)c;
            atomicAdd(live_count, 1);
        } else if (VALUE && event_values) {
            event_values[(o * E + event) * K + c] = __uint_as_float(0x7FC00000u);
        }
        keys[c] = key;
    }
    __syncthreads();                              // the keys are staged; the winner's record is read (the copies may start)
    const int live = *live_count, m = survivors < live ? survivors : live;
    for (int c = tid; c < K; c += 256) {
        const unsigned long long key = keys[c];
        int r = 0xFFFF;                           // terminal
        if (key != ~0ull) {
            r = 0;
            for (int j = 0; j < K; ++j) r += keys[j] < key ? 1 : 0;
            if (r < m) by_rank[r] = (uint16_t)c;
        }
        rank_of[c] = (uint16_t)r;
    }
    __syncthreads();
    // ---- copy
    for (int c = tid; c < K; c += 256) {
        const int r = rank_of[c];
        int donor = r == 0xFFFF ? -2 : -1;
        if (r != 0xFFFF && r >= m) {
            donor = by_rank[(r - m) % m];
            const int64_t n = env0 + c, d = env0 + donor;
            e.active[n] = e.active[d]; e.steps[n] = e.steps[d]; e.reward[n] = e.reward[d];
            tv.best_active[n] = tv.best_active[d]; tv.best_gap[n] = tv.best_gap[d]; tv.best_step[n] = tv.best_step[d];
            tv.initial_gap[n] = tv.initial_gap[d]; tv.t_in[n] = tv.t_in[d];
        }
        if (donors) donors[(o * E + event) * K + c] = donor;
    }
    for (int i = tid; i < K * V; i += 256) {      // V dwords per clone: score [dv], degree [dv], best_state [2 dv]
        const int c = i / V, d = i - c * V;
        const int r = rank_of[c];
        if (r == 0xFFFF || r < m) continue;
        const int64_t n = env0 + c, dn = env0 + by_rank[(r - m) % m];
        if (d < dv) reinterpret_cast<uint32_t*>(e.score + n * V)[d] = reinterpret_cast<const uint32_t*>(e.score + dn * V)[d];
        else if (d < 2 * dv) reinterpret_cast<uint32_t*>(e.degree + n * V)[d - dv] = reinterpret_cast<const uint32_t*>(e.degree + dn * V)[d - dv];
        else reinterpret_cast<uint32_t*>(tv.best_state + n * 2 * V)[d - 2 * dv] = reinterpret_cast<const uint32_t*>(tv.best_state + dn * 2 * V)[d - 2 * dv];
    }
    if (PATH) {                                   // the donor's played prefix: t_in[donor] <= played <= M entries per receiver
        const int P = played < M ? played : M;    // 0 (the last fold passes it, and returns above): no entry, no i / P
        for (int i = tid; P > 0 && i < K * P; i += 256) {
            const int c = i / P, d = i - c * P;
            const int r = rank_of[c];
            if (r == 0xFFFF || r < m) continue;
            const int64_t n = env0 + c, dn = env0 + by_rank[(r - m) % m];
            if (d < tv.t_in[dn]) tv.actions[n * M + d] = tv.actions[dn * M + d];
        }
    }
}

// ================================================================ beam search
// The candidate key of the rule, in two words.  x = m * (double)p is ONE fp64 multiply (the file is compiled without
// contraction); p >= 2^-149 and m >= 0.5 make x a normal double, so frexp is a read of its fields: mantissa m' = 0.5 + the
// 52 fraction bits / 2^53, exponent d = biased exponent - 1022, e' = e + d.  The order "e' descending, m' descending, index
// ascending" is the descending order of the 108-bit number
//     [e' ^ 0x80000000 : 32][fraction : 52][0xFFFFFF - index : 24]
// (m' has a fixed exponent field, so its fraction orders it), held as w0 = its top 64 bits and w1 = the other 44, shifted up
// to 48 so that both words split into whole 8-bit digits: 8 digits of w0, then 6 of w1.  Keys of one start are distinct
__device__ __forceinline__ void beam_key(float p, double m, int e, uint32_t idx, unsigned long long& w0, unsigned long long& w1) {
    const double x = m * (double)p;
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    const int d = (int)((b >> 52) & 0x7FFull) - 1022;
    const unsigned long long frac = b & 0xFFFFFFFFFFFFFull;
    const uint32_t eb = (uint32_t)(e + d) ^ 0x80000000u;
    w0 = ((unsigned long long)eb << 32) | (frac >> 20);
    w1 = (((frac & 0xFFFFFull) << 24) | (unsigned long long)(0xFFFFFFu - idx)) << 4;
}
constexpr int BEAM_DIGITS = 14;
__device__ __forceinline__ uint32_t beam_digit(unsigned long long w0, unsigned long long w1, int d) {
    return d < 8 ? (uint32_t)(w0 >> (56 - 8 * d)) & 0xFFu : (uint32_t)(w1 >> (40 - 8 * (d - 8))) & 0xFFu;
}
// do the first d digits of (w0, w1) equal those of (t0, t1)?
__device__ __forceinline__ bool beam_prefix_eq(unsigned long long w0, unsigned long long w1, unsigned long long t0,
                                               unsigned long long t1, int d) {
    if (d == 0) return true;
    if (d <= 8) return ((w0 ^ t0) >> (64 - 8 * d)) == 0;
    return w0 == t0 && ((w1 ^ t1) >> (48 - 8 * (d - 8))) == 0;
}

// One pass of an NT-thread workgroup over the candidates of a start: f(p, m, e, index) for every (k, a) with slot k live (m != 0)
// and p[k][a] > 0, index = k*A + a.  A thread takes four float4 of probabilities per round, all four loads issued before the
// first is used: the pass is bound by the latency of its loads, not by their bytes (one workgroup per start is few waves per
// CU).  A = 16 Q, so a float4 never straddles two slots and the rows start 16-byte aligned
template <int NT, typename Fn>
__device__ __forceinline__ void beam_for_each(const float* __restrict__ p0, int total_c, int A, const double* s_m, const int* s_e,
                                              int tid, Fn&& f) {
    const float4* __restrict__ p4 = reinterpret_cast<const float4*>(p0);
    const int nv = total_c / 4;
    for (int v0 = tid; v0 < nv; v0 += 4 * NT) {
        float4 q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int v = v0 + u * NT;
            q[u] = v < nv ? p4[v] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = 4 * (v0 + u * NT);
            if (c >= total_c) continue;
            const int k = c / A;
            const double m = s_m[k];
            if (m == 0.0) continue;
            const int e = s_e[k];
            if (q[u].x > 0.0f) f(q[u].x, m, e, (uint32_t)c);
            if (q[u].y > 0.0f) f(q[u].y, m, e, (uint32_t)c + 1u);
            if (q[u].z > 0.0f) f(q[u].z, m, e, (uint32_t)c + 2u);
            if (q[u].w > 0.0f) f(q[u].w, m, e, (uint32_t)c + 3u);
        }
    }
}

// load: the weights and the result of every start of a round, behind k_env_load_starts.  Slot 0 live with (0.5, 1), the
// others dead; the result is the load state at step 0, slot 0
__global__ __launch_bounds__(256) void k_beam_init(EnvView e, BeamView bv, int K, const uint32_t* __restrict__ start_state,
                                                   const uint32_t* __restrict__ start_active, int64_t out_base) {
    const int tid = threadIdx.x, V = e.V, dv = V / 4;
    const int64_t s = blockIdx.x, o = out_base + s, env0 = s * K;
    for (int k = tid; k < K; k += 256) {
        bv.wm[env0 + k] = 0.5; bv.we[env0 + k] = 1; bv.live[env0 + k] = k == 0 ? 1 : 0;
        bv.sel_parent[env0 + k] = -1; bv.sel_action[env0 + k] = -1;
    }
    uint32_t* dst = reinterpret_cast<uint32_t*>(bv.best_state + o * 2 * V);
    for (int d = tid; d < 2 * dv; d += 256) dst[d] = start_state[o * 2 * dv + d];
    if (tid == 0) {
        const uint32_t act = start_active[o];
        const int8_t* sc = reinterpret_cast<const int8_t*>(start_state + o * 2 * dv);
        const int cur = env_total_abs(sc, act, e.Q), sum = env_total_sum(sc, act, e.Q);
        const int gap = cur - (sum < 0 ? -sum : sum);
        bv.best_active[o] = act; bv.best_gap[o] = gap; bv.initial_gap[o] = gap; bv.best_step[o] = 0; bv.best_beam[o] = 0;
        bv.best_mant[o] = 0.5; bv.best_exp[o] = 1;
        bv.fin[s] = 0;
    }
}

// select, one workgroup of 1024 threads per start: the exact top n = min(K, #candidates) of the keys above, by a most-significant-digit radix
// select.  A pass streams the K * A probabilities of the start (a dead slot's row is skipped), forms every candidate's key
// again -- one multiply and a few shifts, cheaper than keeping 131,072 keys -- and counts digit d of the keys that share the d
// digits found so far in a 256-bin LDS histogram; the bin in which the count from the top reaches `need` is digit d of the
// n-th key T, and `need` drops by what lies above it.  Keys are distinct, so some pass ends with exactly `need` keys in T's
// bin: every key >= (T's digits, zeros behind) is chosen, and that is n keys.  Index ties need no case of their own: the
// index is the key's last 24 bits.  A thread counts runs of equal digits in registers and adds a run at once: in the
// first passes every key has the same digit, and one LDS atomic per key would serialise the wave on one bin.
// The chosen keys (n <= 256) go to LDS in any order; thread i then ranks key i by counting the keys above it (every lane reads
// the same LDS word: a broadcast) and writes slot `rank`: parent, action, weight, and the log row of step t.  The weights of
// the step are read into LDS behind the first barrier and written from the keys behind the last one, so no slot's new weight
// is read as an old one
// WINDOW is the same select over the keys STRICTLY BELOW the start's ceiling: the top min(256, remaining) of
// them go, in rank order, into the start's window instead of the slots, and the lowest chosen key becomes the new ceiling.
// Keys are distinct, so the ceiling is exact: no candidate enters two windows and none is skipped
constexpr int BEAM_SELECT_THREADS = 1024;
template <bool WINDOW>
__device__ __forceinline__ void beam_select_body(const float* __restrict__ probs, const BeamView& bv, const BeamChildView& cv, int K, int A,
                                                 int64_t out_base, int M, int t) {
    __shared__ double s_m[PPO_BEAM_MAX_K];
    __shared__ int s_e[PPO_BEAM_MAX_K];
    __shared__ unsigned long long s_k0[PPO_BEAM_MAX_K], s_k1[PPO_BEAM_MAX_K];
    __shared__ uint32_t hist[256], wave_tot[4], ctrl[3], nsel;
    const int tid = threadIdx.x;
    const int64_t s = blockIdx.x, o = out_base + s, env0 = s * K;
    if (bv.fin[s]) return;                                               // the start has finished: its slots idle
    unsigned long long c0 = 0, c1 = 0;
    if (WINDOW) {
        if (cv.n[s] >= K || cv.exhausted[s]) return;                     // the step's beam is full, or no candidate is left
        c0 = cv.ceil[2 * s]; c1 = cv.ceil[2 * s + 1];
    }
    const int limit = WINDOW ? PPO_BEAM_WINDOW : K;
    if (tid < K) {
        const bool lv = bv.live[env0 + tid] != 0;
        s_m[tid] = lv ? bv.wm[env0 + tid] : 0.0;                         // 0: dead (a live mantissa is >= 0.5)
        s_e[tid] = bv.we[env0 + tid];
    }
    if (tid == 0) nsel = 0;
    const float* p0 = probs + env0 * A;
    const int total_c = K * A;
    unsigned long long t0 = 0, t1 = 0;                                   // the digits of T found so far, zeros behind them
    uint32_t need = (uint32_t)limit;
    int n = 0;
    for (int d = 0; d < BEAM_DIGITS; ++d) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();                                                 // (first pass: the weights are staged)
        uint32_t run_digit = 0, run = 0;
        beam_for_each<BEAM_SELECT_THREADS>(p0, total_c, A, s_m, s_e, tid, [&](float p, double m, int e, uint32_t c) {
            unsigned long long w0, w1;
            beam_key(p, m, e, c, w0, w1);
            if (WINDOW && !(w0 < c0 || (w0 == c0 && w1 < c1))) return;
            if (!beam_prefix_eq(w0, w1, t0, t1, d)) return;
            const uint32_t g = beam_digit(w0, w1, d);
            if (g != run_digit) {
                if (run) atomicAdd(&hist[run_digit], run);
                run_digit = g; run = 0;
            }
            ++run;
        });
        if (run) atomicAdd(&hist[run_digit], run);
        __syncthreads();
        // keys in the bins above this thread's (threads 0 .. 255 hold a bin each): a suffix sum across the wave by shuffles,
        // across the four waves through LDS
        const uint32_t h = tid < 256 ? hist[tid] : 0u;
        uint32_t inc = h;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t up = __shfl_down(inc, off);
            if ((tid & 63) + off < 64) inc += up;
        }
        if ((tid & 63) == 0 && tid < 256) wave_tot[tid >> 6] = inc;
        __syncthreads();
        uint32_t above = inc - h, all = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t wt = wave_tot[w];
            all += wt;
            if (w > (tid >> 6)) above += wt;
        }
        if (d == 0) {
            n = (int)(all < (uint32_t)limit ? all : (uint32_t)limit);
            need = (uint32_t)n;
            if (n == 0) break;                                           // no candidate: every slot dies
        }
        if (tid < 256 && above < need && above + h >= need) { ctrl[0] = (uint32_t)tid; ctrl[1] = need - above; ctrl[2] = h; }
        __syncthreads();
        const unsigned long long g = ctrl[0];
        need = ctrl[1];
        if (d < 8) t0 |= g << (56 - 8 * d);
        else t1 |= g << (40 - 8 * (d - 8));
        if (ctrl[2] == need) break;                                      // T's bin holds exactly what is still to choose
    }
    if (n > 0) {
        beam_for_each<BEAM_SELECT_THREADS>(p0, total_c, A, s_m, s_e, tid, [&](float p, double m, int e, uint32_t c) {
            unsigned long long w0, w1;
            beam_key(p, m, e, c, w0, w1);
            if (WINDOW && !(w0 < c0 || (w0 == c0 && w1 < c1))) return;
            if (w0 > t0 || (w0 == t0 && w1 >= t1)) {
                const uint32_t pos = atomicAdd(&nsel, 1u);
                if (pos < (uint32_t)PPO_BEAM_MAX_K) { s_k0[pos] = w0; s_k1[pos] = w1; }
            }
        });
    }
    __syncthreads();
    if (WINDOW && tid == 0) {
        cv.win_count[s] = n;
        if (n < PPO_BEAM_WINDOW) cv.exhausted[s] = 1;
    }
    if (tid < n) {
        const unsigned long long w0 = s_k0[tid], w1 = s_k1[tid];
        int r = 0;
        for (int j = 0; j < n; ++j) {
            const unsigned long long u0 = s_k0[j], u1 = s_k1[j];
            r += (u0 > w0 || (u0 == w0 && u1 > w1)) ? 1 : 0;
        }
        const uint32_t idx = 0xFFFFFFu - (uint32_t)((w1 >> 4) & 0xFFFFFFull);
        const int parent = (int)(idx / (uint32_t)A), action = (int)(idx % (uint32_t)A);
        const unsigned long long frac = ((w0 & 0xFFFFFFFFull) << 20) | (w1 >> 28);
        const double mant = __longlong_as_double((long long)(0x3FE0000000000000ull | frac));
        const int ex = (int)((uint32_t)(w0 >> 32) ^ 0x80000000u);
        if (WINDOW) {                                                    // the slots keep the parents' weights until the commit
            const int64_t wi = s * PPO_BEAM_WINDOW + r;
            cv.win_idx[wi] = idx; cv.win_m[wi] = mant; cv.win_e[wi] = ex;
            if (r == n - 1) { cv.ceil[2 * s] = w0; cv.ceil[2 * s + 1] = w1; }
            return;
        }
        bv.wm[env0 + r] = mant; bv.we[env0 + r] = ex; bv.live[env0 + r] = 1;
        bv.sel_parent[env0 + r] = parent; bv.sel_action[env0 + r] = action;
        const int64_t li = (o * M + t) * K + r;
        if (bv.log_parent) { bv.log_parent[li] = (int16_t)parent; bv.log_action[li] = (int16_t)action; }
        if (bv.log_mant) bv.log_mant[li] = mant;
        if (bv.log_exp) bv.log_exp[li] = ex;
    } else if (!WINDOW && tid < K) {
        bv.live[env0 + tid] = 0; bv.sel_parent[env0 + tid] = -1; bv.sel_action[env0 + tid] = -1;
    }
}
__global__ __launch_bounds__(BEAM_SELECT_THREADS) void k_beam_select(const float* __restrict__ probs, BeamView bv, int K, int A, int64_t out_base,
                                                     int M, int t) {
    beam_select_body<false>(probs, bv, BeamChildView(), K, A, out_base, M, t);
}
__global__ __launch_bounds__(BEAM_SELECT_THREADS) void k_beam_select_window(const float* __restrict__ probs, BeamView bv, BeamChildView cv,
                                                                            int K, int A) {
    beam_select_body<true>(probs, bv, cv, K, A, 0, 0, 0);
}

// expand, one workgroup per start: gather -> step -> fold -> finish.
//   gather  slot j takes score, degree, active and steps of its parent.  Every slot is a receiver and most parents are read
//           several times, so nothing can be copied in place: the whole workgroup first stages the K states of the start in LDS
//           (dynamic, K * (2V + 8) bytes), a barrier, and every write of a child reads LDS only.  One workgroup owns the K
//           envs of a start and no other touches them, so that barrier is all the ordering there is to keep.
//   step    one thread per live slot plays its action with env_step_ref (behind a second barrier: the thread reads bytes
//           other threads gathered).  The tick the step bumps is a scratch word: the envs' own ticks stay.
//   fold    the lowest (gap, slot) of the live slots, k_search_argmin's reduction; the start's result takes it on a STRICTLY
//           lower gap, with step t + 1 and the slot's weight.
//   finish  result gap 0, or t + 1 == max_actions: the start's flag is set and its K envs are left terminal.
extern __shared__ __attribute__((aligned(16))) unsigned char beam_lds[];
__global__ __launch_bounds__(256) void k_beam_expand(EnvView e, BeamView bv, int K, int64_t out_base, int t) {
    __shared__ unsigned long long wave_min[4];
    const int tid = threadIdx.x, V = e.V, dv = V / 4, row = 2 * dv;
    const int64_t s = blockIdx.x, o = out_base + s, env0 = s * K;
    if (bv.fin[s]) return;
    uint32_t* st = reinterpret_cast<uint32_t*>(beam_lds);                // [K][row]
    uint32_t* l_act = st + K * row;                                      // [K]
    int32_t* l_steps = reinterpret_cast<int32_t*>(l_act + K);            // [K]
    // ---- gather
    for (int i = tid; i < K * row; i += 256) {
        const int k = i / row, d = i - k * row;
        st[i] = d < dv ? reinterpret_cast<const uint32_t*>(e.score + (env0 + k) * V)[d]
                       : reinterpret_cast<const uint32_t*>(e.degree + (env0 + k) * V)[d - dv];
    }
    if (tid < K) { l_act[tid] = e.active[env0 + tid]; l_steps[tid] = e.steps[env0 + tid]; }
    const int best_gap = bv.best_gap[o];                                 // read by everyone before the barriers below
    __syncthreads();
    for (int i = tid; i < K * row; i += 256) {
        const int j = i / row, d = i - j * row;
        const int par = bv.sel_parent[env0 + j];
        if (par < 0) continue;
        const uint32_t w = st[par * row + d];
        if (d < dv) reinterpret_cast<uint32_t*>(e.score + (env0 + j) * V)[d] = w;
        else reinterpret_cast<uint32_t*>(e.degree + (env0 + j) * V)[d - dv] = w;
    }
    const int my_par = tid < K ? bv.sel_parent[env0 + tid] : -1;
    if (my_par >= 0) { e.active[env0 + tid] = l_act[my_par]; e.steps[env0 + tid] = l_steps[my_par]; }
    __syncthreads();
    // ---- step
    unsigned long long best = ~0ull;
    if (my_par >= 0) {
        const int64_t nn = env0 + tid;
        EnvRef er = ref_of(e, nn);
        er.tick = bv.tick_scratch + nn;
        float rew; uint8_t dn;
        int score_after = 0;
        const int errf = env_step_ref(const_of(e), er, bv.sel_action[nn], rew, dn, &score_after);
        if (errf) atomicOr(e.err, errf);
        const int sum = env_total_sum(er.sc, *er.active, e.Q);
        const int gap = score_after - (sum < 0 ? -sum : sum);
        best = ((unsigned long long)(uint32_t)gap << 32) | (unsigned long long)(uint32_t)tid;
    }
    // ---- fold
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t hi = __shfl_xor((uint32_t)(best >> 32), off), lo = __shfl_xor((uint32_t)best, off);
        const unsigned long long other = ((unsigned long long)hi << 32) | lo;
        best = other < best ? other : best;
    }
    if ((tid & 63) == 0) wave_min[tid >> 6] = best;
    __syncthreads();                                                     // ... and the stepped states are written
    best = wave_min[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) best = wave_min[w] < best ? wave_min[w] : best;
    int result_gap = best_gap;
    if (best != ~0ull && (int)(uint32_t)(best >> 32) < best_gap) {
        const int slot = (int)(uint32_t)best;
        const int64_t wenv = env0 + slot;
        result_gap = (int)(uint32_t)(best >> 32);
        uint32_t* dst = reinterpret_cast<uint32_t*>(bv.best_state + o * 2 * V);
        for (int d = tid; d < row; d += 256)
            dst[d] = d < dv ? reinterpret_cast<const uint32_t*>(e.score + wenv * V)[d]
                            : reinterpret_cast<const uint32_t*>(e.degree + wenv * V)[d - dv];
        if (tid == 0) {
            bv.best_active[o] = e.active[wenv]; bv.best_gap[o] = result_gap; bv.best_step[o] = t + 1; bv.best_beam[o] = slot;
            bv.best_mant[o] = bv.wm[wenv]; bv.best_exp[o] = bv.we[wenv];
        }
    }
    // ---- finish
    if (result_gap == 0 || t + 1 >= e.max_actions) {
        if (tid < K) { e.done[env0 + tid] = 1; e.episodes_left[env0 + tid] = 0; }
        if (tid == 0) bv.fin[s] = 1;
    }
}

// ================================================================ the distinct beam
// A 64-bit hash of a state's identity: `words` dwords (score, degree, then the active word).  It only filters: equal states
// hash equally, and a full compare decides whether equal hashes are equal states
__device__ __forceinline__ unsigned long long beam_hash_step(unsigned long long h, uint32_t w) {
    h = (h ^ w) * 0x9E3779B97F4A7C15ull;
    return h ^ (h >> 29);
}

// children, one workgroup of 256 threads per start: thread i forms the child of window entry i and decides whether the
// sequential walk would accept it.
//   gather   the window's parents (score, degree, active, steps) from the env arrays into row i of dynamic LDS,
//            256 * (2V + 8) bytes.  The env arrays are only read: the parents stay there until the commit
//   step     env_step_ref on the row (reward, done and tick are LDS scratch words), then the hash of the row's identity
//   compare  behind a barrier, entry i is new iff no window entry j < i, no child accepted in an earlier round and -- mode 2
//            -- no live parent holds the same state.  Comparing against EVERY earlier entry, accepted or not, is the
//            sequential walk without its dependency chain: equality is transitive, so an entry that equals a rejected one
//            equals whatever that one was rejected for.  Everything compared is written in front of the barrier or by an
//            earlier launch, and nothing of it is written behind the barrier
//   place    slot = accepted before the round + new entries before i (ballot and popcount in the wave, wave totals through
//            LDS); slots < K go to the child buffer
extern __shared__ __attribute__((aligned(16))) unsigned char beam_child_lds[];
__global__ __launch_bounds__(256) void k_beam_children(EnvView e, BeamView bv, BeamChildView cv, int K, int mode) {
    __shared__ unsigned long long s_hw[PPO_BEAM_WINDOW], s_ha[PPO_BEAM_MAX_K], s_hp[PPO_BEAM_MAX_K];
    __shared__ uint32_t s_idx[PPO_BEAM_WINDOW], s_tick[PPO_BEAM_WINDOW], s_wt[4];
    __shared__ float s_rew[PPO_BEAM_WINDOW];
    __shared__ uint8_t s_done[PPO_BEAM_WINDOW], s_pl[PPO_BEAM_MAX_K];
    const int tid = threadIdx.x, V = e.V, dv = V / 4, row = 2 * dv + 2, A = 16 * e.Q;
    const int64_t s = blockIdx.x, env0 = s * K;
    if (bv.fin[s]) return;
    const int n_prev = cv.n[s], cnt = cv.win_count[s], ex_prev = cv.examined[s];
    if (n_prev >= K || cnt <= 0) return;                                 // full, or no window that has not been read
    uint32_t* rows = reinterpret_cast<uint32_t*>(beam_child_lds);        // [256][row]: score dv, degree dv, active, steps
    if (tid < cnt) s_idx[tid] = cv.win_idx[s * PPO_BEAM_WINDOW + tid];
    if (tid < n_prev) s_ha[tid] = cv.hash[env0 + tid];
    if (tid < K) {
        const bool lv = mode == 2 && bv.live[env0 + tid] != 0;
        s_pl[tid] = lv ? 1 : 0;
        if (lv) {
            unsigned long long h = 0;
            for (int d = 0; d < dv; ++d) h = beam_hash_step(h, reinterpret_cast<const uint32_t*>(e.score + (env0 + tid) * V)[d]);
            for (int d = 0; d < dv; ++d) h = beam_hash_step(h, reinterpret_cast<const uint32_t*>(e.degree + (env0 + tid) * V)[d]);
            s_hp[tid] = beam_hash_step(h, e.active[env0 + tid]);
        }
    }
    __syncthreads();
    // ---- gather
    for (int i = tid; i < cnt * row; i += 256) {
        const int c = i / row, d = i - c * row;
        const int64_t pn = env0 + (int)(s_idx[c] / (uint32_t)A);
        rows[i] = d < dv ? reinterpret_cast<const uint32_t*>(e.score + pn * V)[d]
                : d < 2 * dv ? reinterpret_cast<const uint32_t*>(e.degree + pn * V)[d - dv]
                : d == 2 * dv ? e.active[pn] : (uint32_t)e.steps[pn];
    }
    __syncthreads();
    // ---- step
    uint32_t* mine = rows + tid * row;
    unsigned long long h = 0;
    int gap = 0;
    if (tid < cnt) {
        s_rew[tid] = 0.0f; s_done[tid] = 0; s_tick[tid] = 0;
        EnvRefLds er;
        er.sc = (PPO_LDS int8_t*)mine; er.dg = (PPO_LDS int8_t*)(mine + dv);
        er.active = (PPO_LDS uint32_t*)(mine + 2 * dv); er.steps = (PPO_LDS int32_t*)(mine + 2 * dv + 1);
        er.reward = (PPO_LDS float*)&s_rew[tid]; er.done = (PPO_LDS uint8_t*)&s_done[tid];
        er.episode = (PPO_LDS uint32_t*)&s_tick[tid]; er.tick = (PPO_LDS uint32_t*)&s_tick[tid];
        float rew; uint8_t dn;
        int score_after = 0;
        const int errf = env_step_ref(const_of(e), er, (int)(s_idx[tid] % (uint32_t)A), rew, dn, &score_after);
        if (errf) atomicOr(e.err, errf);
        const int sum = env_total_sum(er.sc, *er.active, e.Q);
        gap = score_after - (sum < 0 ? -sum : sum);
        for (int d = 0; d <= 2 * dv; ++d) h = beam_hash_step(h, mine[d]);
        s_hw[tid] = h;
    }
    __syncthreads();
    // ---- compare: the hash filters, the bytes decide
    bool is_new = tid < cnt;
    if (is_new) {
        for (int j = 0; j < tid && is_new; ++j) {
            if (s_hw[j] != h) continue;
            const uint32_t* other = rows + j * row;
            bool eq = true;
            for (int d = 0; d <= 2 * dv && eq; ++d) eq = other[d] == mine[d];
            if (eq) is_new = false;
        }
        for (int j = 0; j < n_prev && is_new; ++j) {
            if (s_ha[j] != h) continue;
            const uint32_t* other = reinterpret_cast<const uint32_t*>(cv.state + (env0 + j) * 2 * V);
            bool eq = cv.active[env0 + j] == mine[2 * dv];
            for (int d = 0; d < 2 * dv && eq; ++d) eq = other[d] == mine[d];
            if (eq) is_new = false;
        }
        for (int k = 0; k < K && is_new; ++k) {
            if (!s_pl[k] || s_hp[k] != h) continue;
            const uint32_t* osc = reinterpret_cast<const uint32_t*>(e.score + (env0 + k) * V);
            const uint32_t* odg = reinterpret_cast<const uint32_t*>(e.degree + (env0 + k) * V);
            bool eq = e.active[env0 + k] == mine[2 * dv];
            for (int d = 0; d < dv && eq; ++d) eq = osc[d] == mine[d] && odg[d] == mine[dv + d];
            if (eq) is_new = false;
        }
    }
    // ---- place
    const unsigned long long ballot = __ballot(is_new);
    const int lane = tid & 63, wave = tid >> 6;
    if (lane == 0) s_wt[wave] = (uint32_t)__popcll(ballot);
    __syncthreads();
    int before = __popcll(ballot & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int wt = (int)s_wt[w];
        total += wt;
        if (w < wave) before += wt;
    }
    const int slot = n_prev + before;
    if (is_new && slot < K) {
        const int64_t cn = env0 + slot;
        uint32_t* dst = reinterpret_cast<uint32_t*>(cv.state + cn * 2 * V);
        for (int d = 0; d < 2 * dv; ++d) dst[d] = mine[d];
        cv.active[cn] = mine[2 * dv]; cv.steps[cn] = (int32_t)mine[2 * dv + 1]; cv.gap[cn] = gap; cv.hash[cn] = h;
        cv.wm[cn] = cv.win_m[s * PPO_BEAM_WINDOW + tid]; cv.we[cn] = cv.win_e[s * PPO_BEAM_WINDOW + tid];
        cv.parent[cn] = (int32_t)(s_idx[tid] / (uint32_t)A); cv.action[cn] = (int32_t)(s_idx[tid] % (uint32_t)A);
        cv.rank[cn] = ex_prev + tid;
        if (slot == K - 1) cv.examined[s] = ex_prev + tid + 1;           // the walk stops at K accepted
    }
    if (tid == 0) {
        const int n_now = n_prev + total;
        cv.n[s] = n_now < K ? n_now : K;
        if (n_now < K) cv.examined[s] = ex_prev + cnt;
        cv.win_count[s] = 0;
    }
}

// commit, one workgroup per start, behind the last round of a step: the n accepted children become slots 0 .. n-1 (state,
// active, steps, weight, live), slots n .. K-1 die, row t of the logs is written, then k_beam_expand's fold and finish -- the
// finish also when nothing was accepted.  Last, the start's walk state is cleared for the next step.  The child buffer is
// only read here and the env arrays are only written, so the copy needs no staging
__global__ __launch_bounds__(256) void k_beam_commit(EnvView e, BeamView bv, BeamChildView cv, int K, int64_t out_base, int M, int t) {
    __shared__ unsigned long long wave_min[4];
    const int tid = threadIdx.x, V = e.V, dv = V / 4, row = 2 * dv;
    const int64_t s = blockIdx.x, o = out_base + s, env0 = s * K;
    if (bv.fin[s]) return;
    const int n = cv.n[s], examined = cv.examined[s];
    const int best_gap = bv.best_gap[o];                                 // read by everyone before the barrier below
    for (int i = tid; i < n * row; i += 256) {
        const int j = i / row, d = i - j * row;
        const uint32_t w = reinterpret_cast<const uint32_t*>(cv.state + (env0 + j) * 2 * V)[d];
        if (d < dv) reinterpret_cast<uint32_t*>(e.score + (env0 + j) * V)[d] = w;
        else reinterpret_cast<uint32_t*>(e.degree + (env0 + j) * V)[d - dv] = w;
    }
    unsigned long long best = ~0ull;
    if (tid < n) {
        const int64_t nn = env0 + tid;
        e.active[nn] = cv.active[nn]; e.steps[nn] = cv.steps[nn];
        bv.wm[nn] = cv.wm[nn]; bv.we[nn] = cv.we[nn]; bv.live[nn] = 1;
        const int64_t li = (o * M + t) * K + tid;
        if (bv.log_parent) { bv.log_parent[li] = (int16_t)cv.parent[nn]; bv.log_action[li] = (int16_t)cv.action[nn]; }
        if (bv.log_mant) bv.log_mant[li] = cv.wm[nn];
        if (bv.log_exp) bv.log_exp[li] = cv.we[nn];
        if (cv.log_rank) cv.log_rank[li] = cv.rank[nn];
        best = ((unsigned long long)(uint32_t)cv.gap[nn] << 32) | (unsigned long long)(uint32_t)tid;
    } else if (tid < K) {
        bv.live[env0 + tid] = 0;
    }
    if (tid == 0 && cv.log_examined) cv.log_examined[o * M + t] = examined;
    // ---- fold
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t hi = __shfl_xor((uint32_t)(best >> 32), off), lo = __shfl_xor((uint32_t)best, off);
        const unsigned long long other = ((unsigned long long)hi << 32) | lo;
        best = other < best ? other : best;
    }
    if ((tid & 63) == 0) wave_min[tid >> 6] = best;
    __syncthreads();
    best = wave_min[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) best = wave_min[w] < best ? wave_min[w] : best;
    int result_gap = best_gap;
    if (best != ~0ull && (int)(uint32_t)(best >> 32) < best_gap) {
        const int slot = (int)(uint32_t)best;
        const int64_t wenv = env0 + slot;
        result_gap = (int)(uint32_t)(best >> 32);
        uint32_t* dst = reinterpret_cast<uint32_t*>(bv.best_state + o * 2 * V);
        const uint32_t* src = reinterpret_cast<const uint32_t*>(cv.state + wenv * 2 * V);
        for (int d = tid; d < row; d += 256) dst[d] = src[d];
        if (tid == 0) {
            bv.best_active[o] = cv.active[wenv]; bv.best_gap[o] = result_gap; bv.best_step[o] = t + 1; bv.best_beam[o] = slot;
            bv.best_mant[o] = cv.wm[wenv]; bv.best_exp[o] = cv.we[wenv];
        }
    }
    // ---- finish
    if (result_gap == 0 || t + 1 >= e.max_actions || n == 0) {
        if (tid < K) { e.done[env0 + tid] = 1; e.episodes_left[env0 + tid] = 0; }
        if (tid == 0) bv.fin[s] = 1;
    }
    if (tid == 0) {
        cv.n[s] = 0; cv.examined[s] = 0; cv.exhausted[s] = 0; cv.win_count[s] = 0;
        cv.ceil[2 * s] = ~0ull; cv.ceil[2 * s + 1] = ~0ull;
    }
}

// Teacher-forced replay of action paths: one thread per path, no policy, no resident env.  Path m starts
// from snapshot m (score[V] then degree[V], k_env_snapshot's layout) as reset! leaves an env -- steps 0, not terminal -- and
// plays paths[m][0 ..] with env_step_ref until an entry < 0, `stride` entries, or a terminal state.  The thread's env IS
// its output record (out_state row m, out_active[m]); steps / reward / done / tick live in `work` [4][count] and are
// thrown away.  trace (optional): initial score - score behind every step, INT32_MIN behind `applied`.  Error flags of
// env_step_ref (an action on an inactive quad) are OR-ed into *err, a word of the call, not of the env handle.
__global__ void k_env_apply_paths(EnvConst c, int64_t count, const uint32_t* __restrict__ start_state,
                                  const uint32_t* __restrict__ start_active, const int16_t* __restrict__ paths, int stride,
                                  int8_t* __restrict__ out_state, uint32_t* __restrict__ out_active, int32_t* __restrict__ out_gap,
                                  int32_t* __restrict__ applied, int32_t* __restrict__ trace, int32_t* __restrict__ work,
                                  int32_t* __restrict__ err) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= count) return;
    const int dv = c.V / 4;
    uint32_t* st = reinterpret_cast<uint32_t*>(out_state + m * 2 * c.V);
    for (int d = 0; d < 2 * dv; ++d) st[d] = start_state[m * 2 * dv + d];
    EnvRef er;
    er.sc = out_state + m * 2 * c.V; er.dg = er.sc + c.V; er.active = out_active + m;
    er.steps = work + m; er.reward = reinterpret_cast<float*>(work + count + m);
    er.tick = reinterpret_cast<uint32_t*>(work + 2 * count + m);
    er.done = reinterpret_cast<uint8_t*>(work + 3 * count) + m;
    er.episode = er.tick;                         // step! never reads the episode counter
    *er.active = start_active[m]; *er.steps = 0; *er.reward = 0.0f; *er.tick = 0u; *er.done = 0;
    const int init = env_total_abs(er.sc, *er.active, c.Q);
    int n = 0;
    while (n < stride && !*er.done) {
        const int a = paths[m * stride + n];
        if (a < 0) break;
        float rew; uint8_t dn;
        int score_after = 0;
        const int errf = env_step_ref(c, er, a, rew, dn, &score_after);
        if (errf) atomicOr(err, errf);
        if (trace) trace[m * stride + n] = init - score_after;
        ++n;
    }
    if (trace) for (int i = n; i < stride; ++i) trace[m * stride + i] = INT32_MIN;
    const uint32_t act = *er.active;
    const int cur = env_total_abs(er.sc, act, c.Q), sum = env_total_sum(er.sc, act, c.Q);
    out_gap[m] = cur - (sum < 0 ? -sum : sum);
    applied[m] = n;
}

// Teacher-forced collection, feed: the action env n is given at loop step t, into the rollout buffer's action
// column.  THE definition of "idle": env n plays paths[n][t] unless n >= M, t is at or behind the path's declared length
// (lens[n] = index of its first negative entry, at most stride: worked out by the host, which needs it for T anyway) or the
// env is terminal; an idle env gets -1.  The forced forward and the forced step both read this column and nothing else
__global__ void k_paths_feed(EnvView e, const int16_t* __restrict__ paths, const int32_t* __restrict__ lens, int64_t M,
                             int64_t stride, int64_t t, int32_t* __restrict__ actions_out) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= e.N) return;
    int a = -1;
    if (n < M && t < (int64_t)lens[n] && !e.done[n]) a = paths[n * stride + t];
    actions_out[n] = a;
}

// ... and the step beside k_env_step: one thread per env.  An idle env (action < 0) records valid = 0, reward = 0, done = 1
// like the idle branch of the episodes mode and its state, tick included, stays.  Every other env (then n < M) steps with
// env_step_ref; done_out = the env's own done OR "this was the path's last entry" (t + 1 == lens[n]), so that a path is a
// whole episode for the return scan, GAE and the truncation detector.  An action on an inactive quad is played and
// penalised as step! does and recorded with valid = 0: it never enters the dataset.  No reset, no episode bookkeeping;
// flags go to *err, a word of the call
__global__ void k_env_step_forced(EnvView e, const int32_t* __restrict__ actions, const int32_t* __restrict__ lens, int64_t t,
                                  float* __restrict__ reward_out, uint8_t* __restrict__ done_out,
                                  uint8_t* __restrict__ valid_out, int32_t* __restrict__ err) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= e.N) return;
    const int a = actions[n];
    if (a < 0) {
        valid_out[n] = 0; reward_out[n] = 0.0f; done_out[n] = 1;
        return;
    }
    float rew; uint8_t dn;
    const int errf = env_step_ref(const_of(e), ref_of(e, n), a, rew, dn);
    if (errf) atomicOr(err, errf);
    reward_out[n] = rew;
    done_out[n] = (uint8_t)(dn || t + 1 >= (int64_t)lens[n]);
    valid_out[n] = (errf & 1) ? 0 : 1;
}

// state(env): obs[n][h][f] int8, f<36 template scores, f>=36 template degrees, 0 where the
// template entry is missing or its quad is inactive (test/quad_game_utilities.jl:35-37,46-59).
// One thread per output dword (4 features): coalesced 4-byte stores.
__global__ void k_env_observe(EnvView e, int8_t* __restrict__ obs, uint32_t* __restrict__ active_out) {
    const int H = 4 * e.Q, F = 2 * PPO_TPL, V = e.V;
    const int dw_per_env = H * F / 4;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = gid / dw_per_env;
    if (n >= e.N) return;
    const int rem = (int)(gid - n * dw_per_env);
    const int h = rem / (F / 4), f0 = (rem % (F / 4)) * 4;
    const uint32_t act = e.active[n];
    if (rem == 0 && active_out) active_out[n] = act;
    const int8_t* src = (f0 < PPO_TPL) ? (e.score + n * V) : (e.degree + n * V);
    const int t0 = (f0 < PPO_TPL) ? f0 : f0 - PPO_TPL;
    const bool own = (act >> (h >> 2)) & 1u;
    // four template vertex ids at once from the [H][36] table (36 % 4 == 0, t0 % 4 == 0: one aligned dword)
    const uint32_t ids = *reinterpret_cast<const uint32_t*>(e.tmpl + h * PPO_TPL + t0);
    uint32_t packed = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int v = (int)(int8_t)(ids >> (8 * i));
        const bool ok = own && v >= 0 && ((act >> (v >> 2)) & 1u);
        const int8_t val = ok ? src[v] : (int8_t)0;
        packed |= ((uint32_t)(uint8_t)val) << (8 * i);
    }
    reinterpret_cast<uint32_t*>(obs)[gid] = packed;
}

// compact rollout storage: record [2V] = score[V] then degree[V] of every env (one thread per dword)
__global__ void k_env_snapshot(EnvView e, uint32_t* __restrict__ out) {
    const int dv = e.V / 4;                                    // dwords per array
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = gid / (2 * dv);
    if (n >= e.N) return;
    const int d = (int)(gid - n * 2 * dv);
    const int8_t* src = (d < dv) ? (e.score + n * e.V) : (e.degree + n * e.V);
    out[gid] = reinterpret_cast<const uint32_t*>(src)[d < dv ? d : d - dv];
}

// state(env) from stored snapshots (getters / exporter of the compact form): same arithmetic as k_env_observe with the
// score / degree bytes taken from record n of `cstate` instead of the live env arrays
// idx (optional): record n of the output is transition idx[n] (a minibatch in minibatch order) instead of record n
__global__ void k_expand_states(const int8_t* __restrict__ cstate, const uint32_t* __restrict__ active,
                                const int8_t* __restrict__ tmpl, int64_t count, int Q, int8_t* __restrict__ obs,
                                const int32_t* __restrict__ idx) {
    const int H = 4 * Q, F = 2 * PPO_TPL, V = 4 * Q;
    const int dw_per_env = H * F / 4;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = gid / dw_per_env;
    if (n >= count) return;
    const int rem = (int)(gid - n * dw_per_env);
    const int h = rem / (F / 4), f0 = (rem % (F / 4)) * 4;
    const int64_t rec = idx ? (int64_t)idx[n] : n;
    const uint32_t act = active[rec];
    const int8_t* src = cstate + rec * 2 * V + ((f0 < PPO_TPL) ? 0 : V);
    const int t0 = (f0 < PPO_TPL) ? f0 : f0 - PPO_TPL;
    const bool own = (act >> (h >> 2)) & 1u;
    const uint32_t ids = *reinterpret_cast<const uint32_t*>(tmpl + h * PPO_TPL + t0);
    uint32_t packed = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int v = (int)(int8_t)(ids >> (8 * i));
        const bool ok = own && v >= 0 && ((act >> (v >> 2)) & 1u);
        const int8_t val = ok ? src[v] : (int8_t)0;
        packed |= ((uint32_t)(uint8_t)val) << (8 * i);
    }
    reinterpret_cast<uint32_t*>(obs)[gid] = packed;
}

int32_t launch_env_snapshot(ppo_env_s* e, int8_t* cstate_out) {
    const int64_t total = e->N * (int64_t)(e->V / 2);
    hipLaunchKernelGGL(k_env_snapshot, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ppo_stream(), view_of(e),
                       reinterpret_cast<uint32_t*>(cstate_out));
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

int32_t launch_expand_states(const int8_t* cstate, const uint32_t* active, const int8_t* tmpl, int64_t count, int32_t Q,
                             int8_t* obs_out, const int32_t* idx) {
    if (count <= 0) return PPO_OK;
    const int64_t total = count * (int64_t)(4 * Q * 2 * PPO_TPL / 4);
    hipLaunchKernelGGL(k_expand_states, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ppo_stream(), cstate, active,
                       tmpl, count, (int)Q, obs_out, idx);
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

int32_t launch_env_reset(ppo_env_s* e, int only_done) {
    dim3 grid((unsigned)((e->N + 255) / 256));
    hipLaunchKernelGGL(k_env_reset, grid, dim3(256), 0, ppo_stream(), view_of(e), only_done);
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

int32_t launch_env_step(ppo_env_s* e, const int32_t* actions_dev, float* reward_out, uint8_t* done_out,
                        uint8_t* valid_out, int auto_reset, int episodes_mode, const EvalView* ev) {
    ProfScope ps("k_env_step");
    dim3 grid((unsigned)((e->N + 63) / 64));
    hipLaunchKernelGGL(k_env_step, grid, dim3(64), 0, ppo_stream(), view_of(e), actions_dev, reward_out, done_out,
                       valid_out, auto_reset, episodes_mode, (ev && episodes_mode) ? *ev : EvalView());
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

int32_t launch_env_step_track(ppo_env_s* e, const int32_t* actions_dev, float* reward_out, uint8_t* done_out,
                              uint8_t* valid_out, const TrackView& tv) {
    ProfScope ps("k_env_step");
    dim3 grid((unsigned)((e->N + 63) / 64));
    hipLaunchKernelGGL(k_env_step_track, grid, dim3(64), 0, ppo_stream(), view_of(e), actions_dev, reward_out, done_out,
                       valid_out, tv);
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

int32_t launch_env_load_starts(ppo_env_s* e, const int8_t* start_state, const uint32_t* start_active, int64_t busy, int64_t K,
                               int32_t* t_in) {
    const int64_t total = e->N * (int64_t)(e->V / 2);
    hipLaunchKernelGGL(k_env_load_starts, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ppo_stream(), view_of(e),
                       reinterpret_cast<const uint32_t*>(start_state), start_active, busy, K, t_in);
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

int32_t launch_search_argmin(const TrackView& tv, int32_t V, int64_t S, int64_t K, const TrackView& out, int32_t* best_clone,
                             int32_t* clone_gaps, int64_t out_base, int32_t max_actions) {
    if (out.actions && !tv.actions) {
        ppo_set_error("search_argmin: a path is asked for and no action history was kept");
        return PPO_ERR_ARG;
    }
    hipLaunchKernelGGL(k_search_argmin, dim3((unsigned)S), dim3(256), 0, ppo_stream(), tv, (int)V, K, out, best_clone,
                       clone_gaps, out_base, (int)max_actions);
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

int32_t launch_search_resample(ppo_env_s* e, const TrackView& tv, int64_t S, int64_t K, int64_t survivors, int flags,
                               const TrackView& out, int32_t* best_clone, int64_t out_base, int32_t* donors, int64_t E,
                               int64_t event, int32_t* clone_gaps, int64_t played, const float* values, float* event_values,
                               float value_weight) {
    if (K < 1 || K > PPO_RESAMPLE_MAX_K || S < 1 || S * K > e->N || e->V % 4 != 0) {
        ppo_set_error("search_resample: unsupported shape");
        return PPO_ERR_UNSUPPORTED;
    }
    const bool path = out.actions != nullptr;
    if (path && (!tv.actions || played < 0)) {
        ppo_set_error("search_resample: a path is asked for and no action history was kept");
        return PPO_ERR_ARG;
    }
    ProfScope ps((flags & 2) ? "k_search_fold" : "k_search_resample");
    const size_t lds = 48 + 12 * (size_t)((K + 7) & ~(int64_t)7);
    const int M = e->max_actions, P = (int)std::min<int64_t>(played, M);
    const bool value = values != nullptr && !(flags & 2);               // the last fold ranks nothing
#define LAUNCH_EVENT(PP, VV)                                                                                                  \
    hipLaunchKernelGGL((k_search_resample<PP, VV>), dim3((unsigned)S), dim3(256), lds, ppo_stream(), view_of(e), tv, (int)K, \
                       (int)survivors, flags, out, best_clone, out_base, donors, E, event, clone_gaps, M, P, values,          \
                       event_values, value_weight)
    if (path && value) LAUNCH_EVENT(true, true);
    else if (path) LAUNCH_EVENT(true, false);
    else if (value) LAUNCH_EVENT(false, true);
    else LAUNCH_EVENT(false, false);
#undef LAUNCH_EVENT
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

int32_t launch_beam_init(ppo_env_s* e, const BeamView& bv, int64_t S, int64_t K, const int8_t* start_state,
                         const uint32_t* start_active, int64_t out_base) {
    hipLaunchKernelGGL(k_beam_init, dim3((unsigned)S), dim3(256), 0, ppo_stream(), view_of(e), bv, (int)K,
                       reinterpret_cast<const uint32_t*>(start_state), start_active, out_base);
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

// k_beam_expand's dynamic LDS: the K parent states (score, degree: 2V bytes), active words and step counts of a start.  V = 4 Q
// is at most 128 (Q = 32): 256 * (2 * 128 + 8) = 67,584 bytes is the most a call can ask for
constexpr int BEAM_EXPAND_MAX_V = 128;
static constexpr size_t beam_expand_lds(int64_t K, int64_t V) { return (size_t)K * (2 * (size_t)V + 8); }

static int32_t beam_shape_ok(ppo_env_s* e, int64_t S, int64_t K) {
    if (K < 1 || K > PPO_BEAM_MAX_K || S < 1 || S * K > e->N || e->V % 4 != 0 || K * (int64_t)e->A > 0xFFFFFF) {
        ppo_set_error("beam_search: unsupported shape");
        return PPO_ERR_UNSUPPORTED;
    }
    return PPO_OK;
}

int32_t launch_beam_select(ppo_env_s* e, const float* probs, const BeamView& bv, int64_t S, int64_t K, int64_t out_base, int64_t t) {
    PPO_TRY(beam_shape_ok(e, S, K));
    ProfScope ps("k_beam_select");
    hipLaunchKernelGGL(k_beam_select, dim3((unsigned)S), dim3(BEAM_SELECT_THREADS), 0, ppo_stream(), probs, bv, (int)K, (int)e->A, out_base,
                       (int)e->max_actions, (int)t);
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

int32_t launch_beam_expand(ppo_env_s* e, const BeamView& bv, int64_t S, int64_t K, int64_t out_base, int64_t t) {
    PPO_TRY(beam_shape_ok(e, S, K));
    if (e->V > BEAM_EXPAND_MAX_V) {
        ppo_set_error("beam_search: unsupported shape");
        return PPO_ERR_UNSUPPORTED;
    }
    const size_t lds = beam_expand_lds(K, e->V);
    // per engine: an engine is one host thread with its own device
    static thread_local bool attr_set = false;
    if (!attr_set) {
        HIP_TRY(hipFuncSetAttribute((const void*)k_beam_expand, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)beam_expand_lds(PPO_BEAM_MAX_K, BEAM_EXPAND_MAX_V)));
        attr_set = true;
    }
    ProfScope ps("k_beam_expand");
    hipLaunchKernelGGL(k_beam_expand, dim3((unsigned)S), dim3(256), lds, ppo_stream(), view_of(e), bv, (int)K, out_base, (int)t);
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

int32_t launch_beam_select_window(ppo_env_s* e, const float* probs, const BeamView& bv, const BeamChildView& cv, int64_t S, int64_t K) {
    PPO_TRY(beam_shape_ok(e, S, K));
    ProfScope ps("k_beam_select_window");
    hipLaunchKernelGGL(k_beam_select_window, dim3((unsigned)S), dim3(BEAM_SELECT_THREADS), 0, ppo_stream(), probs, bv, cv, (int)K,
                       (int)e->A);
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

int32_t launch_beam_children(ppo_env_s* e, const BeamView& bv, const BeamChildView& cv, int64_t S, int64_t K, int32_t mode) {
    PPO_TRY(beam_shape_ok(e, S, K));
    if (e->V > BEAM_EXPAND_MAX_V || (mode != 1 && mode != 2)) {
        ppo_set_error("beam_search: unsupported shape");
        return PPO_ERR_UNSUPPORTED;
    }
    // a row per window entry, whatever K is: k_beam_expand's budget at K = 256
    const size_t lds = beam_expand_lds(PPO_BEAM_WINDOW, e->V);
    static thread_local bool attr_set = false;
    if (!attr_set) {
        HIP_TRY(hipFuncSetAttribute((const void*)k_beam_children, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)beam_expand_lds(PPO_BEAM_WINDOW, BEAM_EXPAND_MAX_V)));
        attr_set = true;
    }
    ProfScope ps("k_beam_children");
    hipLaunchKernelGGL(k_beam_children, dim3((unsigned)S), dim3(256), lds, ppo_stream(), view_of(e), bv, cv, (int)K, (int)mode);
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

int32_t launch_beam_commit(ppo_env_s* e, const BeamView& bv, const BeamChildView& cv, int64_t S, int64_t K, int64_t out_base, int64_t t) {
    PPO_TRY(beam_shape_ok(e, S, K));
    ProfScope ps("k_beam_commit");
    hipLaunchKernelGGL(k_beam_commit, dim3((unsigned)S), dim3(256), 0, ppo_stream(), view_of(e), bv, cv, (int)K, out_base,
                       (int)e->max_actions, (int)t);
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

int32_t launch_env_apply_paths(ppo_env_s* e, int64_t count, const int8_t* start_state, const uint32_t* start_active,
                               const int16_t* paths, int32_t stride, int8_t* out_state, uint32_t* out_active, int32_t* out_gap,
                               int32_t* applied, int32_t* trace_or_null, int32_t* work, int32_t* err) {
    if (count <= 0) return PPO_OK;
    if (stride < 1 || e->V % 4 != 0) {
        ppo_set_error("env_apply_paths: unsupported shape");
        return PPO_ERR_UNSUPPORTED;
    }
    EnvConst c;
    c.Q = e->Q; c.V = e->V; c.max_actions = e->max_actions; c.no_action_reward = e->no_action_reward; c.k0 = 0; c.k1 = 0;
    hipLaunchKernelGGL(k_env_apply_paths, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, ppo_stream(), c, count,
                       reinterpret_cast<const uint32_t*>(start_state), start_active, paths, (int)stride, out_state, out_active,
                       out_gap, applied, trace_or_null, work, err);
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

int32_t launch_paths_feed(ppo_env_s* e, const int16_t* paths, const int32_t* lens, int64_t M, int64_t stride, int64_t t,
                          int32_t* actions_out) {
    hipLaunchKernelGGL(k_paths_feed, dim3((unsigned)((e->N + 255) / 256)), dim3(256), 0, ppo_stream(), view_of(e), paths, lens, M,
                       stride, t, actions_out);
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

int32_t launch_env_step_forced(ppo_env_s* e, const int32_t* actions_dev, const int32_t* lens, int64_t t, float* reward_out,
                               uint8_t* done_out, uint8_t* valid_out, int32_t* err) {
    ProfScope ps("k_env_step_forced");
    hipLaunchKernelGGL(k_env_step_forced, dim3((unsigned)((e->N + 63) / 64)), dim3(64), 0, ppo_stream(), view_of(e), actions_dev,
                       lens, t, reward_out, done_out, valid_out, err);
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

int32_t launch_env_observe(ppo_env_s* e, int8_t* obs_out, uint32_t* active_out) {
    ProfScope ps("k_env_observe");
    const int64_t total = e->N * (int64_t)(e->H * e->F / 4);
    dim3 grid((unsigned)((total + 255) / 256));
    hipLaunchKernelGGL(k_env_observe, grid, dim3(256), 0, ppo_stream(), view_of(e), obs_out, active_out);
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}
