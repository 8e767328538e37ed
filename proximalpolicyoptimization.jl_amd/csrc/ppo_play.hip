// ppo_play.hip -- the calls that play the resident envs step by step from the host (launch order only; all math is in the
// kernels): the episodes-mode collector, the evaluators, best-state tracking, the best-of-K and resampling searches, beam
// search, the teacher-forced replay and collection, and the host helpers they share.  The step-mode collector (ppo_collect_rollouts) and
// the handles these calls work on are in ppo_api.hip.
#include "ppo_internal.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <limits>

// ---------------------------------------------------------------- shared host helpers
// episode e of the call is played by env e mod N: env n plays episodes n, n + N, n + 2N, ... below num_episodes
__global__ void k_episode_quota(int32_t* left, int64_t N, int64_t num_episodes) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n < N) left[n] = n < num_episodes ? (int32_t)((num_episodes - n + N - 1) / N) : 0;
}
static void launch_episode_quota(ppo_env_s* env, int64_t count) {
    const int64_t N = env->N;
    hipLaunchKernelGGL(k_episode_quota, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ppo_stream(), env->episodes_left.p, N, count);
}

// has every env used up its episodes_left?  One device-to-host copy: the step loops poll it every 8 steps
static bool poll_due(int64_t t, int64_t Tmax) { return (t & 7) == 7 || t + 1 == Tmax; }
static int32_t quotas_used_up(ppo_env_s* env, std::vector<int32_t>& left, bool* all) {
    left.resize((size_t)env->N);
    PPO_TRY(d2h(left.data(), env->episodes_left.p, left.size()));
    *all = std::all_of(left.begin(), left.end(), [](int32_t l) { return l <= 0; });
    return PPO_OK;
}

// dataset order = env-major concatenation of whole episodes, valid transitions only (the reference's flat buffer)
static int32_t set_index_env_major(ppo_rollouts_s* ro, int64_t T) {
    const int64_t N = ro->N;
    std::vector<uint8_t> valid((size_t)T * N);
    PPO_TRY(d2h(valid.data(), ro->valid.p, (size_t)T * N));
    std::vector<int32_t> index;
    index.reserve((size_t)T * N);
    for (int64_t n = 0; n < N; ++n)
        for (int64_t t = 0; t < T; ++t)
            if (valid[(size_t)t * N + n]) index.push_back((int32_t)(t * N + n));
    ro->len = (int64_t)index.size();
    ro->all_valid = false;
    return h2d(ro->index.p, index.data(), index.size());
}

// caller-supplied start states on the device (check_internal_host first): [count] snapshots in k_env_snapshot's layout,
// score[V] then degree[V], and their active-quad words
struct StartBufs {
    DevBuf<int8_t> d_start; DevBuf<uint32_t> d_act;
    int32_t upload(int32_t V, int64_t count, const int8_t* score, const int8_t* degree, const uint32_t* active) {
        std::vector<int8_t> snap((size_t)count * 2 * V);
        for (int64_t m = 0; m < count; ++m) {
            std::memcpy(&snap[(size_t)m * 2 * V], score + m * V, (size_t)V);
            std::memcpy(&snap[(size_t)m * 2 * V + V], degree + m * V, (size_t)V);
        }
        PPO_TRY(d_start.alloc(snap.size())); PPO_TRY(d_act.alloc((size_t)count));
        PPO_TRY(h2d(d_start.p, snap.data(), snap.size()));
        return h2d(d_act.p, active, (size_t)count);
    }
};

static void mean_std(const std::vector<double>& x, double* mean, double* std) {
    double m = 0.0;
    for (double v : x) m += v;
    m /= (double)x.size();
    double s = 0.0;
    for (double v : x) s += (v - m) * (v - m);
    *mean = m;
    *std = x.size() > 1 ? std::sqrt(s / (double)(x.size() - 1)) : NAN;   // Flux.std: corrected (n-1)
}

extern "C" {

// ================================================================ whole-episode collection
int32_t ppo_collect_rollouts_episodes(ppo_rollouts_t ro, ppo_env_t env, ppo_policy_t pol, int64_t num_episodes,
                                      double discount, int32_t discount_is_f32) {
    PPO_TRY(check_shapes(ro, env, pol));
    ARG_CHECK(num_episodes >= 1, "collect_rollouts!: num_episodes must be >= 1");
    const int64_t N = env->N;
    const int64_t episodes_per_env = (num_episodes + N - 1) / N;       // the busiest env (env 0)
    const int64_t Tmax = episodes_per_env * env->max_actions;
    const bool compact = want_compact(ro, Tmax);
    PPO_TRY(rollouts_reserve(ro, Tmax, compact));
    const size_t srow = (size_t)N * env->H * env->F, crow = (size_t)N * 2 * env->V;
    if (compact) PPO_TRY(env->obs_tmp.alloc(srow));
    launch_episode_quota(env, num_episodes);
    PPO_TRY(launch_env_reset(env, 0));                                  // reset!(env) before the first episode
    std::vector<int32_t> left;
    int64_t T = 0;
    for (int64_t t = 0; t < Tmax; ++t) {
        int8_t* st = compact ? env->obs_tmp.p : ro->states.p + (size_t)t * srow;
        uint32_t* am = ro->active.p + (size_t)t * N;
        PPO_TRY(launch_env_observe(env, st, am));
        if (compact) PPO_TRY(launch_env_snapshot(env, ro->cstate.p + (size_t)t * crow));
        PPO_TRY(launch_policy_rollout(pol, env, st, am, ro->actions.p + t * N, ro->p_sel.p + t * N, nullptr));
        PPO_TRY(launch_env_step(env, ro->actions.p + t * N, ro->rewards.p + t * N, ro->done.p + t * N,
                                ro->valid.p + t * N, 0, 1));
        T = t + 1;
        if (poll_due(t, Tmax)) {
            bool all = false;
            PPO_TRY(quotas_used_up(env, left, &all));
            if (all) break;
        }
    }
    rollouts_filled(ro, T);
    PPO_TRY(set_index_env_major(ro, T));
    PPO_TRY(launch_returns_tn(ro->rewards.p, ro->done.p, ro->returns.p, T, N, discount, discount_is_f32));
    return ppo_env_check_errors(env, nullptr);
}

// ================================================================ evaluators
// The step loop of the evaluators and of the best-state search: observe, policy forward + sample, env step with the
// bookkeeping of `ev` (k_env_step) or `tv` (k_env_step_track), until every env has used up its episodes_left (polled every
// 8 steps) or Tmax steps have run.  Row 0 of `scratch` is the only rollout storage touched.
// The action is chosen under the policy's selection (ppo_policy_set_selection; the default is the sampled rollout step).
// after_step (optional) runs behind the env step of loop step t, before the poll (the resampling search's events).
static int32_t play_quotas(ppo_policy_s* pol, ppo_env_s* env, ppo_rollouts_s* scratch, int64_t Tmax, const EvalView* ev,
                           const TrackView* tv, bool* all_done, const std::function<int32_t(int64_t)>* after_step = nullptr) {
    std::vector<int32_t> left;
    bool all = false;
    for (int64_t t = 0; t < Tmax && !all; ++t) {
        PPO_TRY(launch_env_observe(env, scratch->states.p, scratch->active.p));
        PPO_TRY(launch_policy_select(pol, env, scratch->states.p, scratch->active.p, scratch->actions.p, scratch->p_sel.p, nullptr));
        if (tv) PPO_TRY(launch_env_step_track(env, scratch->actions.p, scratch->rewards.p, scratch->done.p, scratch->valid.p, *tv));
        else PPO_TRY(launch_env_step(env, scratch->actions.p, scratch->rewards.p, scratch->done.p, scratch->valid.p, 0, 1, ev));
        if (after_step) PPO_TRY((*after_step)(t));
        if (poll_due(t, Tmax)) PPO_TRY(quotas_used_up(env, left, &all));
    }
    *all_done = all;
    return PPO_OK;
}

// Evaluator variants on the device (test/quad_game_utilities.jl:280-307,369-387; kind 1 = src/evaluate.jl:1-16): exactly
// num_trajectories whole episodes, trajectory e on resident env e mod N like ppo_collect_rollouts_episodes; the
// per-episode value is tracked inside the env step (k_env_step, EvalView), nothing but one value per trajectory
// comes back.  Row 0 of `scratch` is the only rollout storage touched.  values: [num_trajectories], env-major.
static int32_t evaluate_impl(ppo_policy_s* pol, ppo_env_s* env, ppo_rollouts_s* scratch, int64_t num_traj, int32_t kind,
                             std::vector<double>& values) {
    PPO_TRY(check_shapes(scratch, env, pol));
    ARG_CHECK(num_traj >= 1, "evaluator: num_trajectories must be >= 1");
    ARG_CHECK(kind >= 1 && kind <= 3, "evaluator: kind must be 1 (return), 2 (best return) or 3 (normalised best return)");
    const int64_t N = env->N;
    const int64_t per_env = (num_traj + N - 1) / N;
    const int64_t Tmax = per_env * ((int64_t)env->max_actions + 1);      // + 1: a skipped (maxreturn == 0) episode costs one step
    PPO_TRY(rollouts_reserve(scratch, 1, false));
    DevBuf<double> ep_ret, out; DevBuf<int32_t> ep_i;
    PPO_TRY(ep_ret.alloc((size_t)N)); PPO_TRY(out.alloc((size_t)num_traj)); PPO_TRY(ep_i.alloc((size_t)4 * N));
    HIP_TRY(hipMemsetAsync(ep_ret.p, 0, (size_t)N * 8, ppo_stream()));
    HIP_TRY(hipMemsetAsync(ep_i.p, 0, (size_t)4 * N * 4, ppo_stream()));
    HIP_TRY(hipMemsetAsync(out.p, 0, (size_t)num_traj * 8, ppo_stream()));
    EvalView ev;
    ev.kind = kind; ev.ep_ret = ep_ret.p; ev.ep_init = ep_i.p; ev.ep_min = ep_i.p + N; ev.ep_maxret = ep_i.p + 2 * N;
    ev.ep_count = ep_i.p + 3 * N; ev.out = out.p; ev.num_traj = num_traj;
    launch_episode_quota(env, num_traj);
    PPO_TRY(launch_env_reset(env, 0));                                  // reset!(env) before the first trajectory
    bool all = false;
    PPO_TRY(play_quotas(pol, env, scratch, Tmax, &ev, nullptr, &all));
    ARG_CHECK(all, "evaluator: the episodes did not finish within max_actions steps each");
    rollouts_scratch_used(scratch);
    values.resize((size_t)num_traj);
    PPO_TRY(d2h(values.data(), out.p, (size_t)num_traj));
    return ppo_env_check_errors(env, nullptr);
}

// average_returns (src/evaluate.jl:18-25): undiscounted return of each whole episode, then Flux.mean / Flux.std
int32_t ppo_average_returns(ppo_policy_t pol, ppo_env_t env, ppo_rollouts_t scratch, int64_t num_trajectories,
                            double* mean, double* std) {
    ARG_CHECK(pol && env && scratch && mean && std && num_trajectories >= 1, "average_returns: bad argument");
    std::vector<double> rets;
    if (!default_selection(pol) || !default_truncation(pol)) {     // the collectors never read the selection or the truncation: kind 1 of the evaluators is the same statistic
        PPO_TRY(evaluate_impl(pol, env, scratch, num_trajectories, 1, rets));
        mean_std(rets, mean, std);
        return PPO_OK;
    }
    const int64_t N = env->N;
    const int64_t per_env = (num_trajectories + N - 1) / N;
    PPO_TRY(ppo_collect_rollouts_episodes(scratch, env, pol, num_trajectories, 1.0, 0));   // exactly num_trajectories (:19-22)
    const int64_t T = scratch->T;
    std::vector<float> r((size_t)T * N);
    std::vector<uint8_t> dn((size_t)T * N), va((size_t)T * N);
    PPO_TRY(d2h(r.data(), scratch->rewards.p, r.size()));
    PPO_TRY(d2h(dn.data(), scratch->done.p, dn.size()));
    PPO_TRY(d2h(va.data(), scratch->valid.p, va.size()));
    rets.reserve((size_t)per_env * N);
    for (int64_t n = 0; n < N; ++n) {
        double acc = 0.0;
        for (int64_t t = 0; t < T; ++t) {
            const size_t i = (size_t)t * N + n;
            if (!va[i]) continue;
            acc += (double)r[i];                         // ret += reward(env)   src/evaluate.jl:13
            if (dn[i]) { rets.push_back(acc); acc = 0.0; }
        }
    }
    ARG_CHECK(!rets.empty(), "average_returns: no complete episode");
    mean_std(rets, mean, std);
    return PPO_OK;
}

// diagnostic for the tests (not part of include/ppo_hip.h), like ppo_debug_train_ratios: what one step of play_quotas would
// choose for every env from the state and tick it holds -- observe, launch_policy_select -- WITHOUT the env step: actions [N]
// (0-based) and p_sel [N], which no call behind play_quotas returns.  The envs keep state, tick and counters; their flag word
// takes the tail's bits
int32_t ppo_debug_select_step(ppo_policy_t pol, ppo_env_t env, ppo_rollouts_t scratch, int32_t* actions, float* p_sel) {
    ARG_CHECK(pol && env && scratch && actions && p_sel, "ppo_debug_select_step: null argument");
    PPO_TRY(check_shapes(scratch, env, pol));
    PPO_TRY(rollouts_reserve(scratch, 1, false));
    PPO_TRY(launch_env_observe(env, scratch->states.p, scratch->active.p));
    PPO_TRY(launch_policy_select(pol, env, scratch->states.p, scratch->active.p, scratch->actions.p, scratch->p_sel.p, nullptr));
    rollouts_scratch_used(scratch);
    PPO_TRY(d2h(actions, scratch->actions.p, (size_t)env->N));
    return d2h(p_sel, scratch->p_sel.p, (size_t)env->N);
}

int32_t ppo_evaluate_trajectories(ppo_policy_t pol, ppo_env_t env, ppo_rollouts_t scratch, int64_t num_trajectories,
                                  int32_t kind, double* values) {
    ARG_CHECK(pol && env && scratch && values, "evaluator: null argument");
    std::vector<double> v;
    PPO_TRY(evaluate_impl(pol, env, scratch, num_trajectories, kind, v));
    std::memcpy(values, v.data(), v.size() * sizeof(double));
    return PPO_OK;
}

// average_best_returns(wrapper, policy, num_trajectories)         test/quad_game_utilities.jl:299-307
int32_t ppo_average_best_returns(ppo_policy_t pol, ppo_env_t env, ppo_rollouts_t scratch, int64_t num_trajectories,
                                 double* mean, double* std) {
    ARG_CHECK(pol && env && scratch && mean && std, "average_best_returns: null argument");
    std::vector<double> v;
    PPO_TRY(evaluate_impl(pol, env, scratch, num_trajectories, 2, v));
    mean_std(v, mean, std);
    return PPO_OK;
}

// average_normalized_returns(wrapper, policy, num_trajectories)   test/quad_game_utilities.jl:380-387
int32_t ppo_average_normalized_returns(ppo_policy_t pol, ppo_env_t env, ppo_rollouts_t scratch, int64_t num_trajectories,
                                       double* mean, double* std) {
    ARG_CHECK(pol && env && scratch && mean && std, "average_normalized_returns: null argument");
    std::vector<double> v;
    PPO_TRY(evaluate_impl(pol, env, scratch, num_trajectories, 3, v));
    mean_std(v, mean, std);
    return PPO_OK;
}

// ================================================================ best state of a rollout, best-of-K search
// device storage of TrackView records: `slots` output records and the per-env running values
struct TrackBufs {
    DevBuf<int32_t> per_env, ints, trace, types; DevBuf<int8_t> state; DevBuf<uint32_t> active; DevBuf<int16_t> acts;
    TrackView tv;
    int32_t alloc(int64_t N, int64_t slots, int32_t V, int32_t max_actions, bool want_trace, bool want_types,
                  bool want_actions = false) {
        const size_t S = (size_t)slots;
        hipStream_t stream = ppo_stream();
        PPO_TRY(per_env.alloc((size_t)3 * N)); PPO_TRY(ints.alloc(4 * S)); PPO_TRY(state.alloc(S * 2 * V)); PPO_TRY(active.alloc(S));
        HIP_TRY(hipMemsetAsync(per_env.p, 0, (size_t)3 * N * 4, stream));
        HIP_TRY(hipMemsetAsync(ints.p, 0, 4 * S * 4, stream));
        HIP_TRY(hipMemsetAsync(state.p, 0, S * 2 * V, stream));
        HIP_TRY(hipMemsetAsync(active.p, 0, S * 4, stream));
        tv.t_in = per_env.p; tv.ep_init = per_env.p + N; tv.ep_count = per_env.p + 2 * N;
        tv.best_state = state.p; tv.best_active = active.p;
        tv.best_gap = ints.p; tv.best_step = ints.p + S; tv.length = ints.p + 2 * S; tv.initial_gap = ints.p + 3 * S;
        tv.num_traj = slots;
        if (want_trace) {
            PPO_TRY(trace.alloc(S * max_actions));
            HIP_TRY(hipMemsetAsync(trace.p, 0, S * max_actions * 4, stream));
            tv.trace = trace.p;
        }
        if (want_types) {
            PPO_TRY(types.alloc(S * 4));
            HIP_TRY(hipMemsetAsync(types.p, 0, S * 4 * 4, stream));
            tv.type_counts = types.p;
        }
        if (want_actions) {                                               // -1 everywhere: what stays behind a trajectory's end
            PPO_TRY(acts.alloc(S * max_actions));
            HIP_TRY(hipMemsetAsync(acts.p, 0xFF, S * max_actions * sizeof(int16_t), stream));
            tv.actions = acts.p;
        }
        return PPO_OK;
    }
};

// best_state_in_rollout (test/quad_game_utilities.jl:341-358) for num_trajectories trajectories, with
// single_trajectory_scores (:309-323) and the action-type counts behind count_non_flips (test/random_quad.jl:9-27)
static int32_t best_states_impl(ppo_policy_t pol, ppo_env_t env, ppo_rollouts_t scratch, int64_t num_trajectories,
                                int32_t reset_first, int8_t* best_state, uint32_t* best_active, int32_t* best_gap,
                                int32_t* best_step, int32_t* length, int32_t* initial_gap, int32_t* trace_or_null,
                                int32_t* type_counts_or_null, int16_t* actions_or_null) {
    ARG_CHECK(best_state && best_active && best_gap && best_step && length && initial_gap, "best_states: null argument");
    PPO_TRY(check_shapes(scratch, env, pol));
    const int64_t N = env->N, nt = num_trajectories;
    ARG_CHECK(nt >= 1, "best_states: num_trajectories must be >= 1");
    if (!reset_first) {
        ARG_CHECK(nt <= N, "best_states: without reset! every env plays at most one trajectory (num_trajectories <= N)");
        std::vector<uint8_t> dn((size_t)N);
        PPO_TRY(d2h(dn.data(), env->done.p, (size_t)N));
        for (int64_t n = 0; n < nt; ++n) ARG_CHECK(!dn[n], "best_states: an env that is to play is already terminal");
    }
    const int64_t per_env = (nt + N - 1) / N;
    const int32_t M = env->max_actions, V = env->V;
    PPO_TRY(rollouts_reserve(scratch, 1, false));
    TrackBufs b;
    PPO_TRY(b.alloc(N, nt, V, M, trace_or_null != nullptr, type_counts_or_null != nullptr, actions_or_null != nullptr));
    launch_episode_quota(env, nt);
    if (reset_first) PPO_TRY(launch_env_reset(env, 0));                 // reset!(env) before the first trajectory
    bool all = false;
    PPO_TRY(play_quotas(pol, env, scratch, per_env * M, nullptr, &b.tv, &all));
    ARG_CHECK(all, "best_states: the trajectories did not finish within max_actions steps each");
    rollouts_scratch_used(scratch);
    const size_t S = (size_t)nt;
    PPO_TRY(d2h(best_state, b.state.p, S * 2 * V)); PPO_TRY(d2h(best_active, b.active.p, S));
    PPO_TRY(d2h(best_gap, b.tv.best_gap, S)); PPO_TRY(d2h(best_step, b.tv.best_step, S));
    PPO_TRY(d2h(length, b.tv.length, S)); PPO_TRY(d2h(initial_gap, b.tv.initial_gap, S));
    if (trace_or_null) {
        PPO_TRY(d2h(trace_or_null, b.trace.p, S * M));
        for (size_t s = 0; s < S; ++s)                                    // entries behind the trajectory's end
            for (int32_t t = std::max(length[s], 0); t < M; ++t) trace_or_null[s * M + t] = INT32_MIN;
    }
    if (type_counts_or_null) PPO_TRY(d2h(type_counts_or_null, b.types.p, S * 4));
    if (actions_or_null) PPO_TRY(d2h(actions_or_null, b.acts.p, S * M));
    return ppo_env_check_errors(env, nullptr);
}

int32_t ppo_best_states(ppo_policy_t pol, ppo_env_t env, ppo_rollouts_t scratch, int64_t num_trajectories,
                        int32_t reset_first, int8_t* best_state, uint32_t* best_active, int32_t* best_gap,
                        int32_t* best_step, int32_t* length, int32_t* initial_gap, int32_t* trace_or_null,
                        int32_t* type_counts_or_null) {
    return best_states_impl(pol, env, scratch, num_trajectories, reset_first, best_state, best_active, best_gap, best_step,
                            length, initial_gap, trace_or_null, type_counts_or_null, nullptr);
}

// ... with every trajectory's 0-based actions: row [max_actions], -1 behind `length`; its first best_step
// entries are the path to the best state
int32_t ppo_best_states_actions(ppo_policy_t pol, ppo_env_t env, ppo_rollouts_t scratch, int64_t num_trajectories,
                                int32_t reset_first, int8_t* best_state, uint32_t* best_active, int32_t* best_gap,
                                int32_t* best_step, int32_t* length, int32_t* initial_gap, int32_t* trace_or_null,
                                int32_t* type_counts_or_null, int16_t* actions) {
    ARG_CHECK(actions, "best_states_actions: null argument");
    return best_states_impl(pol, env, scratch, num_trajectories, reset_first, best_state, best_active, best_gap, best_step,
                            length, initial_gap, trace_or_null, type_counts_or_null, actions);
}

// What both searches take and return: the starts ([num_starts][V] score and degree, [num_starts] active-quad words) and one
// result row per start
struct SearchIO {
    int64_t num_starts, K;
    const int8_t* score; const int8_t* degree; const uint32_t* active;
    int8_t* best_state; uint32_t* best_active; int32_t* best_gap; int32_t* best_clone; int32_t* best_step; int32_t* initial_gap;
    int32_t* clone_gaps_or_null; int16_t* path_or_null;
};
// What the resampling search adds to best-of-K: a resample event (k_search_resample: fold, rank, copy) behind
// every interval-th step of a round.  critic (optional): an event ranks the live clones by cur_gap -
// value_weight * V(state held now) instead of cur_gap.  donors, event_values (optional): [num_starts][E][K] logs of the events
struct ResampleArgs {
    int64_t interval, survivors;
    int32_t* donors_or_null;
    ppo_policy_s* critic; double value_weight; float* event_values_or_null;
};

// The driver of both searches from caller-supplied start states.  Sampling is keyed on (global env id, tick), so K resident
// envs loaded with one state play K different trajectories: rounds of S = N / K starts, each a load (k_env_load_starts), the
// tracked step loop and one fold of the K per-env records of every start into its result.  No reset! runs: the episode
// counters stay, ticks advance by the steps played.
// Best-of-K (rs == nullptr): the fold is one reduction (k_search_argmin).
// Resampling (rs): events ride in play_quotas' loop, which polls completion every 8 steps as for every other caller -- an
// event costs a launch, no copy -- and one more fold (k_search_resample, flags & 2) runs behind the round's last step.  With a
// critic the envs are observed into row 0 of `scratch` in front of an event (the next loop step overwrites it anyway) and
// the critic's forward turns the rows into one value per env, all on the device; the last fold ranks nothing and needs neither
static int32_t search_impl(const std::string& who, ppo_policy_t pol, ppo_env_t env, ppo_rollouts_t scratch, const SearchIO& io,
                           const ResampleArgs* rs) {
    ARG_CHECK(io.score && io.degree && io.active && io.best_state && io.best_active && io.best_gap && io.best_clone &&
              io.best_step && io.initial_gap, who + ": null argument");
    PPO_TRY(check_shapes(scratch, env, pol));
    const int64_t N = env->N, Mst = io.num_starts, K = io.K;
    ARG_CHECK(Mst >= 1 && K >= 1 && K <= N, who + ": need num_starts >= 1 and 1 <= K <= N");
    if (rs) {
        ARG_CHECK(rs->interval >= 1, who + ": interval must be >= 1");
        ARG_CHECK(rs->survivors >= 1 && rs->survivors <= K, who + ": need 1 <= survivors <= K");
        ARG_CHECK(rs->critic || !rs->event_values_or_null, who + ": a log of values needs a critic");
    }
    ppo_policy_s* critic = rs ? rs->critic : nullptr;
    if (critic) {
        PPO_TRY(value_checks(who.c_str(), critic, env->F));
        if (env->H != 32 && env->H != 128) {
            ppo_set_error(who + ": the critic needs H = 32 (Q=8) or 128 (Q=32) half-edges in this build");
            return PPO_ERR_UNSUPPORTED;
        }
        ARG_CHECK(std::isfinite(rs->value_weight) && rs->value_weight >= 0.0 && std::isfinite((float)rs->value_weight),
                  who + ": value_weight must be finite and >= 0");
    }
    PPO_TRY(check_internal_host(env->Q, Mst, io.score, io.degree, io.active));
    if (rs && K > PPO_RESAMPLE_MAX_K) {
        ppo_set_error(who + ": K above 4096 clones is not supported (the rank keys are staged in LDS)");
        return PPO_ERR_UNSUPPORTED;
    }
    const int32_t V = env->V, M = env->max_actions;
    const int64_t S = N / K, E = rs ? (M - 1) / rs->interval : 0;
    PPO_TRY(rollouts_reserve(scratch, 1, false));
    StartBufs start;
    PPO_TRY(start.upload(V, Mst, io.score, io.degree, io.active));
    DevBuf<int32_t> d_clone, d_gaps, d_donors;
    PPO_TRY(d_clone.alloc((size_t)Mst));
    if (io.clone_gaps_or_null) PPO_TRY(d_gaps.alloc((size_t)Mst * K));
    int32_t* const gaps = io.clone_gaps_or_null ? d_gaps.p : nullptr;
    const size_t log_len = (size_t)Mst * (size_t)E * (size_t)K;
    const bool want_log = rs && rs->donors_or_null && log_len > 0;
    if (want_log) {                                                      // an event that never runs: every clone had terminated
        std::fill(rs->donors_or_null, rs->donors_or_null + log_len, -2);
        PPO_TRY(d_donors.alloc(log_len));
        PPO_TRY(h2d(d_donors.p, rs->donors_or_null, log_len));
    }
    DevBuf<float> d_values, d_vlog;                                      // the critic's value of every env; the log of them
    const bool want_vlog = rs && rs->event_values_or_null && log_len > 0;
    if (critic) PPO_TRY(d_values.alloc((size_t)N));
    if (want_vlog) {                                                     // an event that never runs leaves NaN
        std::fill(rs->event_values_or_null, rs->event_values_or_null + log_len, std::numeric_limits<float>::quiet_NaN());
        PPO_TRY(d_vlog.alloc(log_len));
        PPO_TRY(h2d(d_vlog.p, rs->event_values_or_null, log_len));
    }
    TrackBufs rec, out;                                                  // per-env records of a round (slot = env); the results
    PPO_TRY(rec.alloc(N, N, V, M, false, false, io.path_or_null != nullptr));
    PPO_TRY(out.alloc(1, Mst, V, M, false, false, io.path_or_null != nullptr));
    for (int64_t base = 0; base < Mst; base += S) {
        const int64_t Sr = std::min(S, Mst - base);
        HIP_TRY(hipMemsetAsync(rec.tv.ep_count, 0, (size_t)N * 4, ppo_stream()));
        PPO_TRY(launch_env_load_starts(env, start.d_start.p + (size_t)base * 2 * V, start.d_act.p + base, Sr * K, K, rec.tv.t_in));
        int first = 1;
        const std::function<int32_t(int64_t)> event = [&](int64_t t) -> int32_t {
            const int64_t played = t + 1;                                // loop steps since the round's load
            if (played % rs->interval != 0 || played >= M) return PPO_OK;
            if (critic) {                                                // V of the state every env holds behind the step
                PPO_TRY(launch_env_observe(env, scratch->states.p, scratch->active.p));
                PPO_TRY(launch_value_predict(critic, scratch->states.p, nullptr, scratch->active.p, nullptr, 0, N, env->H,
                                             d_values.p));
            }
            PPO_TRY(launch_search_resample(env, rec.tv, Sr, K, rs->survivors, first, out.tv, d_clone.p, base,
                                           want_log ? d_donors.p : nullptr, E, played / rs->interval - 1, nullptr, played,
                                           critic ? d_values.p : nullptr, want_vlog ? d_vlog.p : nullptr, (float)rs->value_weight));
            first = 0;
            return PPO_OK;
        };
        bool all = false;
        PPO_TRY(play_quotas(pol, env, scratch, M, nullptr, &rec.tv, &all, rs ? &event : nullptr));
        ARG_CHECK(all, who + ": the trajectories did not finish within max_actions steps");
        if (rs) PPO_TRY(launch_search_resample(env, rec.tv, Sr, K, rs->survivors, first | 2, out.tv, d_clone.p, base, nullptr, E, 0, gaps, 0));
        else PPO_TRY(launch_search_argmin(rec.tv, V, Sr, K, out.tv, d_clone.p, gaps, base, M));
    }
    rollouts_scratch_used(scratch);
    const size_t Ms = (size_t)Mst;
    PPO_TRY(d2h(io.best_state, out.state.p, Ms * 2 * V)); PPO_TRY(d2h(io.best_active, out.active.p, Ms));
    PPO_TRY(d2h(io.best_gap, out.tv.best_gap, Ms)); PPO_TRY(d2h(io.best_step, out.tv.best_step, Ms));
    PPO_TRY(d2h(io.initial_gap, out.tv.initial_gap, Ms)); PPO_TRY(d2h(io.best_clone, d_clone.p, Ms));
    if (gaps) PPO_TRY(d2h(io.clone_gaps_or_null, gaps, Ms * (size_t)K));
    if (want_log) PPO_TRY(d2h(rs->donors_or_null, d_donors.p, log_len));
    if (want_vlog) PPO_TRY(d2h(rs->event_values_or_null, d_vlog.p, log_len));
    if (io.path_or_null) PPO_TRY(d2h(io.path_or_null, out.acts.p, Ms * (size_t)M));
    return ppo_env_check_errors(env, nullptr);
}

int32_t ppo_search_best_states(ppo_policy_t pol, ppo_env_t env, ppo_rollouts_t scratch, int64_t num_starts, int64_t K,
                               const int8_t* score, const int8_t* degree, const uint32_t* active, int8_t* best_state,
                               uint32_t* best_active, int32_t* best_gap, int32_t* best_clone, int32_t* best_step,
                               int32_t* initial_gap, int32_t* clone_gaps_or_null) {
    return search_impl("search_best_states", pol, env, scratch, {num_starts, K, score, degree, active, best_state, best_active,
                       best_gap, best_clone, best_step, initial_gap, clone_gaps_or_null, nullptr}, nullptr);
}

// ... with the path to every start's result: the winner's first best_step 0-based actions, -1 behind them
int32_t ppo_search_best_states_path(ppo_policy_t pol, ppo_env_t env, ppo_rollouts_t scratch, int64_t num_starts, int64_t K,
                                    const int8_t* score, const int8_t* degree, const uint32_t* active, int8_t* best_state,
                                    uint32_t* best_active, int32_t* best_gap, int32_t* best_clone, int32_t* best_step,
                                    int32_t* initial_gap, int32_t* clone_gaps_or_null, int16_t* path) {
    ARG_CHECK(path, "search_best_states_path: null argument");
    return search_impl("search_best_states", pol, env, scratch, {num_starts, K, score, degree, active, best_state, best_active,
                       best_gap, best_clone, best_step, initial_gap, clone_gaps_or_null, path}, nullptr);
}

// Resampling search: ppo_search_best_states' schedule with a resample event behind every interval-th step of
// a round, and one more fold behind the round's last step
int32_t ppo_search_resample_states(ppo_policy_t pol, ppo_env_t env, ppo_rollouts_t scratch, int64_t num_starts, int64_t K,
                                   const int8_t* score, const int8_t* degree, const uint32_t* active, int8_t* best_state,
                                   uint32_t* best_active, int32_t* best_gap, int32_t* best_clone, int32_t* best_step,
                                   int32_t* initial_gap, int32_t* clone_gaps_or_null, int64_t interval, int64_t survivors,
                                   int32_t* donors_or_null) {
    const ResampleArgs rs = {interval, survivors, donors_or_null, nullptr, 0.0, nullptr};
    return search_impl("search_resample_states", pol, env, scratch, {num_starts, K, score, degree, active, best_state,
                       best_active, best_gap, best_clone, best_step, initial_gap, clone_gaps_or_null, nullptr}, &rs);
}

// ... with the path to every start's result.  The action history belongs to the lineage: a copy carries the
// donor's played prefix with its record, and every fold that takes a winner's record takes the first best_step entries of
// that winner's history with it -- before the event's copies can overwrite them
int32_t ppo_search_resample_states_path(ppo_policy_t pol, ppo_env_t env, ppo_rollouts_t scratch, int64_t num_starts, int64_t K,
                                        const int8_t* score, const int8_t* degree, const uint32_t* active, int8_t* best_state,
                                        uint32_t* best_active, int32_t* best_gap, int32_t* best_clone, int32_t* best_step,
                                        int32_t* initial_gap, int32_t* clone_gaps_or_null, int64_t interval, int64_t survivors,
                                        int32_t* donors_or_null, int16_t* path) {
    ARG_CHECK(path, "search_resample_states_path: null argument");
    const ResampleArgs rs = {interval, survivors, donors_or_null, nullptr, 0.0, nullptr};
    return search_impl("search_resample_states", pol, env, scratch, {num_starts, K, score, degree, active, best_state,
                       best_active, best_gap, best_clone, best_step, initial_gap, clone_gaps_or_null, path}, &rs);
}

// ... ranking a start's live clones by where the critic expects them to end: cur_gap - value_weight * V(s)
// in place of cur_gap.  The fold, the ranks, the copy and the path are the plain call's
int32_t ppo_search_resample_states_value(ppo_policy_t pol, ppo_policy_t critic, ppo_env_t env, ppo_rollouts_t scratch,
                                         int64_t num_starts, int64_t K, const int8_t* score, const int8_t* degree,
                                         const uint32_t* active, int8_t* best_state, uint32_t* best_active, int32_t* best_gap,
                                         int32_t* best_clone, int32_t* best_step, int32_t* initial_gap,
                                         int32_t* clone_gaps_or_null, int64_t interval, int64_t survivors, double value_weight,
                                         int32_t* donors_or_null, float* event_values_or_null, int16_t* path_or_null) {
    ARG_CHECK(critic, "search_resample_states_value: null argument");
    const ResampleArgs rs = {interval, survivors, donors_or_null, critic, value_weight, event_values_or_null};
    return search_impl("search_resample_states", pol, env, scratch, {num_starts, K, score, degree, active, best_state,
                       best_active, best_gap, best_clone, best_step, initial_gap, clone_gaps_or_null, path_or_null}, &rs);
}

// ================================================================ beam search
// Beam search: the K likeliest action sequences from every start, deterministic and seed-free.  search_impl's
// rounds of S = N / K starts; a step is observe, the probabilities forward (ppo_policy_forward's launcher over the N envs),
// k_beam_select and k_beam_expand.  A finished start's workgroups return at once; the host reads the round's finish flags
// every 8 steps, play_quotas' poll, and nothing else crosses in the loop.  No reset! runs, nothing is sampled, the envs' ticks
// and episode counters stay (the step bumps a scratch tick).  The path is walked on the host from the back-pointer log, which
// comes back in one copy behind the last round
//
// The distinct beam (distinct_mode 1 "children", 2 "parents") replaces select and expand by up to `rounds` rounds
// of k_beam_select_window + k_beam_children and one k_beam_commit: the parents stay in the env arrays through the step and the
// accepted children collect in a child buffer of the call.  The rounds of a step are enqueued without a look at the device: a
// start that is full or has run out of candidates costs workgroups that return at once
static int32_t beam_impl(ppo_policy_t pol, ppo_env_t env, ppo_rollouts_t scratch, int64_t num_starts, int64_t K,
                         const int8_t* score, const int8_t* degree, const uint32_t* active, int8_t* best_state,
                         uint32_t* best_active, int32_t* best_gap, int32_t* best_beam, int32_t* best_step,
                         int32_t* initial_gap, double* best_mant, int32_t* best_exp, int16_t* path_or_null,
                         int16_t* log_parent_or_null, int16_t* log_action_or_null, double* log_mant_or_null,
                         int32_t* log_exp_or_null, int32_t distinct_mode, int32_t rounds, int32_t* log_rank_or_null,
                         int32_t* examined_or_null) {
    const std::string who = "beam_search_states";
    ARG_CHECK(score && degree && active && best_state && best_active && best_gap && best_beam && best_step && initial_gap &&
              best_mant && best_exp, who + ": null argument");
    ARG_CHECK(distinct_mode >= 0 && distinct_mode <= 2, who + ": distinct must be 0 (off), 1 (children) or 2 (parents)");
    ARG_CHECK(distinct_mode == 0 || (rounds >= 1 && rounds <= PPO_BEAM_MAX_ROUNDS), who + ": need 1 <= rounds <= 16");
    ARG_CHECK(distinct_mode != 0 || (!log_rank_or_null && !examined_or_null), who + ": rank and examined are logs of a distinct call");
    PPO_TRY(check_shapes(scratch, env, pol));
    const int64_t N = env->N, Mst = num_starts;
    ARG_CHECK(Mst >= 1 && K >= 1 && K <= N, who + ": need num_starts >= 1 and 1 <= K <= N");
    if (pol->dtype != PPO_DTYPE_F32) {
        ppo_set_error(who + ": a bf16-dtype policy is not supported (the weights are defined on the fp32-MFMA forward's probabilities)");
        return PPO_ERR_UNSUPPORTED;
    }
    if (env->H != 32 && env->H != 128) {
        ppo_set_error(who + ": H must be 32 (Q=8) or 128 (Q=32) half-edges in this build");
        return PPO_ERR_UNSUPPORTED;
    }
    PPO_TRY(check_internal_host(env->Q, Mst, score, degree, active));
    if (K > PPO_BEAM_MAX_K) {
        ppo_set_error(who + ": K above 256 slots is not supported (the chosen keys and the weights are staged in LDS, one thread per slot)");
        return PPO_ERR_UNSUPPORTED;
    }
    const int32_t V = env->V, M = env->max_actions, A = env->A;
    const int64_t S = N / K;
    const size_t Ms = (size_t)Mst, log_len = Ms * (size_t)M * (size_t)K;
    PPO_TRY(rollouts_reserve(scratch, 1, false));
    StartBufs start;
    PPO_TRY(start.upload(V, Mst, score, degree, active));
    DevBuf<float> d_probs; DevBuf<double> d_wm, d_bmant, d_lmant; DevBuf<int32_t> d_ints, d_res, d_lexp; DevBuf<uint8_t> d_live;
    DevBuf<uint32_t> d_tick, d_bact; DevBuf<int8_t> d_state; DevBuf<int16_t> d_log;
    PPO_TRY(d_probs.alloc((size_t)N * A)); PPO_TRY(d_wm.alloc((size_t)N)); PPO_TRY(d_live.alloc((size_t)N));
    PPO_TRY(d_ints.alloc((size_t)4 * N + S));                            // we, sel_parent, sel_action, the load's step counters [N]; fin [S]
    PPO_TRY(d_tick.alloc((size_t)N));
    PPO_TRY(d_state.alloc(Ms * 2 * V)); PPO_TRY(d_bact.alloc(Ms)); PPO_TRY(d_bmant.alloc(Ms));
    PPO_TRY(d_res.alloc(5 * Ms));                                        // gap, beam, step, initial_gap, exp
    // the back-pointer log (parent, action: -1 = a dead slot, a step that did not run) is kept only where an output is made of it
    const bool want_log = path_or_null || log_parent_or_null || log_action_or_null;
    hipStream_t stream = ppo_stream();
    if (want_log) {
        PPO_TRY(d_log.alloc(2 * log_len));
        HIP_TRY(hipMemsetAsync(d_log.p, 0xFF, 2 * log_len * sizeof(int16_t), stream));
    }
    HIP_TRY(hipMemsetAsync(d_tick.p, 0, (size_t)N * 4, stream));
    BeamView bv;
    bv.wm = d_wm.p; bv.we = d_ints.p; bv.sel_parent = d_ints.p + N; bv.sel_action = d_ints.p + 2 * N; bv.fin = d_ints.p + 4 * N;
    int32_t* const load_t_in = d_ints.p + 3 * N;                         // k_env_load_starts zeroes a step counter per env; unread here
    bv.live = d_live.p; bv.tick_scratch = d_tick.p;
    bv.best_state = d_state.p; bv.best_active = d_bact.p; bv.best_mant = d_bmant.p;
    bv.best_gap = d_res.p; bv.best_beam = d_res.p + Ms; bv.best_step = d_res.p + 2 * Ms; bv.initial_gap = d_res.p + 3 * Ms;
    bv.best_exp = d_res.p + 4 * Ms;
    if (want_log) { bv.log_parent = d_log.p; bv.log_action = d_log.p + log_len; }
    if (log_mant_or_null) {                                              // weights of a dead slot or of a step that did not run: 0
        PPO_TRY(d_lmant.alloc(log_len));
        HIP_TRY(hipMemsetAsync(d_lmant.p, 0, log_len * 8, stream));
        bv.log_mant = d_lmant.p;
    }
    if (log_exp_or_null) {
        PPO_TRY(d_lexp.alloc(log_len));
        HIP_TRY(hipMemsetAsync(d_lexp.p, 0, log_len * 4, stream));
        bv.log_exp = d_lexp.p;
    }
    // the distinct beam's child buffer, walk state and window
    BeamChildView cv;
    DevBuf<int8_t> c_state; DevBuf<double> c_dbl; DevBuf<int32_t> c_ints, c_lrank, c_lex; DevBuf<uint32_t> c_u32;
    DevBuf<unsigned long long> c_u64;
    const size_t Ns = (size_t)N, Ss = (size_t)S, Ws = Ss * PPO_BEAM_WINDOW;
    if (distinct_mode) {
        PPO_TRY(c_state.alloc(Ns * 2 * V)); PPO_TRY(c_dbl.alloc(Ns + Ws)); PPO_TRY(c_u32.alloc(Ns + Ws));
        PPO_TRY(c_ints.alloc(6 * Ns + 4 * Ss + Ws)); PPO_TRY(c_u64.alloc(Ns + 2 * Ss));
        cv.state = c_state.p; cv.wm = c_dbl.p; cv.win_m = c_dbl.p + Ns; cv.active = c_u32.p; cv.win_idx = c_u32.p + Ns;
        cv.steps = c_ints.p; cv.gap = c_ints.p + Ns; cv.we = c_ints.p + 2 * Ns; cv.parent = c_ints.p + 3 * Ns;
        cv.action = c_ints.p + 4 * Ns; cv.rank = c_ints.p + 5 * Ns;
        cv.n = c_ints.p + 6 * Ns; cv.examined = cv.n + Ss; cv.exhausted = cv.n + 2 * Ss; cv.win_count = cv.n + 3 * Ss;
        cv.win_e = cv.n + 4 * Ss;
        cv.hash = c_u64.p; cv.ceil = c_u64.p + Ns;
        if (log_rank_or_null) {                                          // -1: a dead slot, a step that did not run
            PPO_TRY(c_lrank.alloc(log_len));
            HIP_TRY(hipMemsetAsync(c_lrank.p, 0xFF, log_len * 4, stream));
            cv.log_rank = c_lrank.p;
        }
        if (examined_or_null) {
            PPO_TRY(c_lex.alloc(Ms * (size_t)M));
            HIP_TRY(hipMemsetAsync(c_lex.p, 0xFF, Ms * (size_t)M * 4, stream));
            cv.log_examined = c_lex.p;
        }
    }
    std::vector<int32_t> fin;
    for (int64_t base = 0; base < Mst; base += S) {
        const int64_t Sr = std::min(S, Mst - base);
        PPO_TRY(launch_env_load_starts(env, start.d_start.p + (size_t)base * 2 * V, start.d_act.p + base, Sr * K, K, load_t_in));
        PPO_TRY(launch_beam_init(env, bv, Sr, K, start.d_start.p, start.d_act.p, base));
        if (distinct_mode) {                                             // an empty walk and the highest ceiling; the commit restores them
            HIP_TRY(hipMemsetAsync(cv.n, 0, 4 * Ss * sizeof(int32_t), stream));
            HIP_TRY(hipMemsetAsync(cv.ceil, 0xFF, 2 * Ss * sizeof(unsigned long long), stream));
        }
        bool all = false;
        for (int64_t t = 0; t < M && !all; ++t) {
            PPO_TRY(launch_env_observe(env, scratch->states.p, scratch->active.p));
            PPO_TRY(launch_policy_probs(pol, scratch->states.p, scratch->active.p, N, env->H, d_probs.p));
            if (distinct_mode) {
                for (int32_t r = 0; r < rounds; ++r) {
                    PPO_TRY(launch_beam_select_window(env, d_probs.p, bv, cv, Sr, K));
                    PPO_TRY(launch_beam_children(env, bv, cv, Sr, K, distinct_mode));
                }
                PPO_TRY(launch_beam_commit(env, bv, cv, Sr, K, base, t));
            } else {
                PPO_TRY(launch_beam_select(env, d_probs.p, bv, Sr, K, base, t));
                PPO_TRY(launch_beam_expand(env, bv, Sr, K, base, t));
            }
            if (poll_due(t, M)) {
                fin.resize((size_t)Sr);
                PPO_TRY(d2h(fin.data(), bv.fin, (size_t)Sr));
                all = std::all_of(fin.begin(), fin.end(), [](int32_t f) { return f != 0; });
            }
        }
        ARG_CHECK(all, who + ": the starts did not finish within max_actions steps");
    }
    rollouts_scratch_used(scratch);
    PPO_TRY(d2h(best_state, d_state.p, Ms * 2 * V)); PPO_TRY(d2h(best_active, d_bact.p, Ms));
    PPO_TRY(d2h(best_gap, bv.best_gap, Ms)); PPO_TRY(d2h(best_beam, bv.best_beam, Ms)); PPO_TRY(d2h(best_step, bv.best_step, Ms));
    PPO_TRY(d2h(initial_gap, bv.initial_gap, Ms)); PPO_TRY(d2h(best_mant, d_bmant.p, Ms)); PPO_TRY(d2h(best_exp, bv.best_exp, Ms));
    if (log_mant_or_null) PPO_TRY(d2h(log_mant_or_null, d_lmant.p, log_len));
    if (log_exp_or_null) PPO_TRY(d2h(log_exp_or_null, d_lexp.p, log_len));
    if (log_rank_or_null) PPO_TRY(d2h(log_rank_or_null, c_lrank.p, log_len));
    if (examined_or_null) PPO_TRY(d2h(examined_or_null, c_lex.p, Ms * (size_t)M));
    if (path_or_null || log_parent_or_null || log_action_or_null) {
        std::vector<int16_t> log(2 * log_len);
        PPO_TRY(d2h(log.data(), d_log.p, 2 * log_len));
        if (log_parent_or_null) std::memcpy(log_parent_or_null, log.data(), log_len * sizeof(int16_t));
        if (log_action_or_null) std::memcpy(log_action_or_null, log.data() + log_len, log_len * sizeof(int16_t));
        if (path_or_null) {                                              // walk the back-pointers from (best_step, best_beam)
            std::fill(path_or_null, path_or_null + Ms * (size_t)M, (int16_t)-1);
            for (size_t m = 0; m < Ms; ++m) {
                int slot = best_beam[m];
                for (int t = best_step[m] - 1; t >= 0; --t) {
                    const size_t li = (m * (size_t)M + (size_t)t) * (size_t)K + (size_t)slot;
                    ARG_CHECK(slot >= 0 && slot < K && log[li] >= 0, who + ": the back-pointer log does not lead to the result");
                    path_or_null[m * (size_t)M + (size_t)t] = log[log_len + li];
                    slot = log[li];
                }
            }
        }
    }
    return ppo_env_check_errors(env, nullptr);
}

int32_t ppo_beam_search_states(ppo_policy_t pol, ppo_env_t env, ppo_rollouts_t scratch, int64_t num_starts, int64_t K,
                               const int8_t* score, const int8_t* degree, const uint32_t* active, int8_t* best_state,
                               uint32_t* best_active, int32_t* best_gap, int32_t* best_beam, int32_t* best_step,
                               int32_t* initial_gap, double* best_mant, int32_t* best_exp, int16_t* path_or_null,
                               int16_t* log_parent_or_null, int16_t* log_action_or_null, double* log_mant_or_null,
                               int32_t* log_exp_or_null) {
    return beam_impl(pol, env, scratch, num_starts, K, score, degree, active, best_state, best_active, best_gap, best_beam,
                     best_step, initial_gap, best_mant, best_exp, path_or_null, log_parent_or_null, log_action_or_null,
                     log_mant_or_null, log_exp_or_null, 0, 0, nullptr, nullptr);
}

int32_t ppo_beam_search_states_distinct(ppo_policy_t pol, ppo_env_t env, ppo_rollouts_t scratch, int64_t num_starts, int64_t K,
                                        const int8_t* score, const int8_t* degree, const uint32_t* active, int8_t* best_state,
                                        uint32_t* best_active, int32_t* best_gap, int32_t* best_beam, int32_t* best_step,
                                        int32_t* initial_gap, double* best_mant, int32_t* best_exp, int16_t* path_or_null,
                                        int16_t* log_parent_or_null, int16_t* log_action_or_null, double* log_mant_or_null,
                                        int32_t* log_exp_or_null, int32_t distinct_mode, int32_t rounds,
                                        int32_t* log_rank_or_null, int32_t* examined_or_null) {
    return beam_impl(pol, env, scratch, num_starts, K, score, degree, active, best_state, best_active, best_gap, best_beam,
                     best_step, initial_gap, best_mant, best_exp, path_or_null, log_parent_or_null, log_action_or_null,
                     log_mant_or_null, log_exp_or_null, distinct_mode, rounds, log_rank_or_null, examined_or_null);
}

// ================================================================ teacher-forced replay and collection
// Teacher-forced replay of action paths on caller-supplied states, without a policy: what checks a returned
// path on the device.  The env handle supplies Q, max_actions and no_action_reward only: the resident envs, their ticks,
// episode counters and error flag are untouched.  Everything is validated on the host before anything is uploaded
int32_t ppo_env_apply_paths(ppo_env_t env, int64_t M, const int8_t* score, const int8_t* degree, const uint32_t* active,
                            const int16_t* paths, int64_t stride, int8_t* out_state, uint32_t* out_active, int32_t* out_gap,
                            int32_t* applied, int32_t* trace_or_null) {
    ARG_CHECK(env && score && degree && active && paths && out_state && out_active && out_gap && applied,
              "env_apply_paths: null argument");
    ARG_CHECK(M >= 1, "env_apply_paths: need at least one path");
    ARG_CHECK(stride >= 1 && stride <= INT32_MAX, "env_apply_paths: stride must be >= 1");
    PPO_TRY(check_internal_host(env->Q, M, score, degree, active));
    const int32_t V = env->V, A = 16 * env->Q;
    const size_t Ms = (size_t)M, cells = Ms * (size_t)stride;
    for (size_t i = 0; i < cells; ++i) ARG_CHECK(paths[i] < A, "env_apply_paths: action index out of range");
    StartBufs start;
    PPO_TRY(start.upload(V, M, score, degree, active));
    DevBuf<int8_t> d_state; DevBuf<uint32_t> d_oact; DevBuf<int16_t> d_paths; DevBuf<int32_t> d_ints, d_trace;
    PPO_TRY(d_state.alloc(Ms * 2 * V)); PPO_TRY(d_oact.alloc(Ms));
    PPO_TRY(d_paths.alloc(cells)); PPO_TRY(d_ints.alloc(6 * Ms + 1));     // gap, applied, work [4][M], the flag word
    if (trace_or_null) PPO_TRY(d_trace.alloc(cells));
    PPO_TRY(h2d(d_paths.p, paths, cells));
    HIP_TRY(hipMemsetAsync(d_ints.p, 0, (6 * Ms + 1) * 4, ppo_stream()));
    int32_t* d_err = d_ints.p + 6 * Ms;
    PPO_TRY(launch_env_apply_paths(env, M, start.d_start.p, start.d_act.p, d_paths.p, (int32_t)stride, d_state.p, d_oact.p, d_ints.p,
                                   d_ints.p + Ms, trace_or_null ? d_trace.p : nullptr, d_ints.p + 2 * Ms, d_err));
    PPO_TRY(d2h(out_state, d_state.p, Ms * 2 * V)); PPO_TRY(d2h(out_active, d_oact.p, Ms));
    PPO_TRY(d2h(out_gap, d_ints.p, Ms)); PPO_TRY(d2h(applied, d_ints.p + Ms, Ms));
    if (trace_or_null) PPO_TRY(d2h(trace_or_null, d_trace.p, cells));
    int32_t f = 0;
    PPO_TRY(d2h(&f, d_err, 1));
    if (f) {
        ppo_set_error("AssertionError (device flag): env_apply_paths: a path holds an action on an inactive quad");
        return PPO_ERR_DEVICE_FLAG;
    }
    return PPO_OK;
}

// Teacher-forced collection: envs 0 .. M - 1 are loaded with the starts and play the given paths instead of
// sampled actions, and what they pass through is left in `ro` as an ordinary rollout buffer.  The loop is the episodes
// mode's -- observe, snapshot when compact, forward, step -- with the forced forward and the forced step; the host knows every
// path's declared length, so T is known in front of the loop and nothing is polled.  The flag word is the call's own: a
// path with an action on an inactive quad does not leave the env handle flagged
int32_t ppo_collect_paths(ppo_rollouts_t ro, ppo_env_t env, ppo_policy_t pol, int64_t M, const int8_t* score, const int8_t* degree,
                          const uint32_t* active, const int16_t* paths, int64_t stride, double discount, int32_t discount_is_f32,
                          int32_t record_probs) {
    PPO_TRY(check_shapes(ro, env, pol));
    ARG_CHECK(score && degree && active && paths, "collect_paths!: null argument");
    const int64_t N = env->N;
    ARG_CHECK(M >= 1 && M <= N, "collect_paths!: need 1 <= M <= N paths (one resident env plays one path)");
    ARG_CHECK(stride >= 1 && stride <= INT32_MAX, "collect_paths!: stride must be >= 1");
    PPO_TRY(check_internal_host(env->Q, M, score, degree, active));
    const int32_t V = env->V, A = 16 * env->Q;
    const size_t Ms = (size_t)M, cells = Ms * (size_t)stride;
    std::vector<int32_t> lens(Ms);                                       // declared length: the index of the first negative entry
    int64_t T = 1;
    for (size_t m = 0; m < Ms; ++m) {
        int64_t len = stride;
        for (int64_t i = 0; i < stride; ++i) {
            const int16_t a = paths[m * (size_t)stride + i];
            ARG_CHECK(a < A, "collect_paths!: action index out of range");
            if (a < 0 && i < len) len = i;
        }
        lens[m] = (int32_t)len;
        T = std::max(T, len);
    }
    if (pol->dtype != PPO_DTYPE_F32) {
        ppo_set_error("collect_paths!: a bf16-dtype policy is not supported (the teacher-forced mode exists in the fp32-MFMA forward only)");
        return PPO_ERR_UNSUPPORTED;
    }
    if (ro->sink) {
        ppo_set_error("collect_paths!: a buffer with a disk sink attached is not supported");
        return PPO_ERR_UNSUPPORTED;
    }
    const bool compact = want_compact(ro, T);
    PPO_TRY(rollouts_reserve(ro, T, compact));
    const size_t srow = (size_t)N * env->H * env->F, crow = (size_t)N * 2 * V;
    if (compact) PPO_TRY(env->obs_tmp.alloc(srow));
    if (record_probs) PPO_TRY(ro->full_probs.alloc((size_t)T * N * env->A));
    StartBufs start;
    PPO_TRY(start.upload(V, M, score, degree, active));
    DevBuf<int16_t> d_paths; DevBuf<int32_t> d_ints;
    PPO_TRY(d_paths.alloc(cells));
    PPO_TRY(d_ints.alloc(Ms + (size_t)N + 1));                           // lens [M], the load's step counters [N], the flag word
    PPO_TRY(h2d(d_paths.p, paths, cells));
    PPO_TRY(h2d(d_ints.p, lens.data(), Ms));
    int32_t* d_err = d_ints.p + Ms + N;
    HIP_TRY(hipMemsetAsync(d_err, 0, 4, ppo_stream()));
    // envs 0 .. M - 1 as reset! leaves an env, one start each; the envs behind them keep what they hold and idle
    PPO_TRY(launch_env_load_starts(env, start.d_start.p, start.d_act.p, M, 1, d_ints.p + Ms));
    for (int64_t t = 0; t < T; ++t) {
        int8_t* st = compact ? env->obs_tmp.p : ro->states.p + (size_t)t * srow;
        uint32_t* am = ro->active.p + (size_t)t * N;
        int32_t* ac = ro->actions.p + t * N;
        PPO_TRY(launch_env_observe(env, st, am));
        if (compact) PPO_TRY(launch_env_snapshot(env, ro->cstate.p + (size_t)t * crow));
        PPO_TRY(launch_paths_feed(env, d_paths.p, d_ints.p, M, stride, t, ac));
        PPO_TRY(launch_policy_forced(pol, env, st, am, ac, ro->p_sel.p + t * N,
                                     record_probs ? ro->full_probs.p + (size_t)t * N * env->A : nullptr, d_err));
        PPO_TRY(launch_env_step_forced(env, ac, d_ints.p, t, ro->rewards.p + t * N, ro->done.p + t * N, ro->valid.p + t * N, d_err));
    }
    rollouts_filled(ro, T);
    if (record_probs) ro->probs_T = T;
    PPO_TRY(set_index_env_major(ro, T));          // env-major concatenation of the paths: the episodes mode's order
    PPO_TRY(launch_returns_tn(ro->rewards.p, ro->done.p, ro->returns.p, T, N, discount, discount_is_f32));
    int32_t f = 0;
    PPO_TRY(d2h(&f, d_err, 1));
    if (f) {
        ppo_set_error("AssertionError (device flag): collect_paths!: a path holds an action on an inactive quad (its transition is recorded with valid = 0 and probability 0)");
        return PPO_ERR_DEVICE_FLAG;
    }
    return PPO_OK;
}

}  // extern "C"
