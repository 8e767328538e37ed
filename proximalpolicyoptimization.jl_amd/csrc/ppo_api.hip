// ppo_api.hip -- extern "C" surface of libppo_hip.so (include/ppo_hip.h): engine state, handle management (env, policy,
// optimiser, rollout buffer) and the host-side orchestration of the step-mode collect_rollouts! (launch order only; all math
// is in the kernels); the calls that play whole episodes, evaluate and search are in ppo_play.hip, training and the critic
// in ppo_train.hip.  There is NO CPU fallback: every entry point runs on the GPU or fails.
#include "ppo_internal.h"
#include "ppo_device.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>


// ---------------------------------------------------------------- engine state: ONE ENGINE PER HOST THREAD
// Everything that makes up an engine instance -- the HIP device (hipSetDevice is per thread), the stream every kernel of
// that engine is enqueued on, the kernel-timing tables, the RCCL communicator (ppo_rccl.hip), the last error text -- is
// thread_local: a process may run several engines, one per host thread (e.g. one per GPU), each with its own stream and
// communicator, and handles belong to the thread that created them ("one stream per engine handle").  What
// stays process-wide are the tuning knobs (ppo_set_*) and the pinned-record pool of the disk sink (mutex-protected).
static thread_local std::string g_err;
static thread_local hipStream_t g_stream = nullptr;
static thread_local bool g_own_stream = false;
static thread_local bool g_init = false;
static thread_local bool g_prof = false;
struct ProfRec { hipEvent_t e0, e1; };
static thread_local std::map<std::string, std::vector<ProfRec>> g_prof_pending;
static thread_local std::map<std::string, std::pair<double, int64_t>> g_prof_done;

void ppo_set_error(const std::string& msg) { g_err = msg; }
hipStream_t ppo_stream() { return g_stream; }
int ppo_hip_fail(hipError_t e, const char* what, const char* file, int line) {
    g_err = std::string("HIP error: ") + hipGetErrorString(e) + " in " + what + " at " + file + ":" + std::to_string(line);
    return PPO_ERR_HIP;
}

ProfScope::ProfScope(const char* n) : name(n), e0(nullptr), e1(nullptr), on(g_prof) {
    if (on) {
        (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
        (void)hipEventRecord(e0, g_stream);
    }
}
ProfScope::~ProfScope() {
    if (on) {
        (void)hipEventRecord(e1, g_stream);
        g_prof_pending[name].push_back({e0, e1});
    }
}

static int32_t ensure_init() {
    if (g_init) return PPO_OK;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        ppo_set_error("no HIP device available: libppo_hip has no CPU fallback");
        return PPO_ERR_HIP;
    }
    HIP_TRY(hipStreamCreate(&g_stream));
    g_own_stream = true;
    g_init = true;
    return PPO_OK;
}

extern "C" {

int32_t ppo_version(void) { return 200; }

int32_t ppo_last_error(char* buf, int64_t cap) {
    if (!buf || cap <= 0) return PPO_ERR_ARG;
    std::strncpy(buf, g_err.c_str(), (size_t)cap - 1);
    buf[cap - 1] = 0;
    return PPO_OK;
}

int32_t ppo_device_count(int32_t* out) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) n = 0;
    if (out) *out = n;
    return PPO_OK;
}

int32_t ppo_device_init(int32_t device_ordinal) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) { ppo_set_error("no HIP device available: libppo_hip has no CPU fallback"); return PPO_ERR_HIP; }
    ARG_CHECK(device_ordinal >= 0 && device_ordinal < n, "device ordinal out of range");
    HIP_TRY(hipSetDevice(device_ordinal));
    if (!g_init) {
        HIP_TRY(hipStreamCreate(&g_stream));
        g_own_stream = true;
        g_init = true;
    }
    return PPO_OK;
}

int32_t ppo_set_stream(void* hip_stream) {
    PPO_TRY(ensure_init());
    if (g_own_stream && g_stream) { (void)hipStreamSynchronize(g_stream); (void)hipStreamDestroy(g_stream); }
    g_stream = (hipStream_t)hip_stream;
    g_own_stream = false;
    return PPO_OK;
}

int32_t ppo_device_synchronize(void) {
    PPO_TRY(ensure_init());
    HIP_TRY(hipStreamSynchronize(g_stream));
    return PPO_OK;
}

int32_t ppo_profile_enable(int32_t on) {
    g_prof = on != 0;
    if (on) { g_prof_pending.clear(); g_prof_done.clear(); }
    return PPO_OK;
}

int32_t ppo_profile_get(const char* kernel_name, double* total_ms, int64_t* launches) {
    PPO_TRY(ensure_init());
    HIP_TRY(hipStreamSynchronize(g_stream));
    for (auto& kv : g_prof_pending) {
        auto& acc = g_prof_done[kv.first];
        for (auto& r : kv.second) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) { acc.first += ms; acc.second += 1; }
            (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1);
        }
        kv.second.clear();
    }
    auto it = g_prof_done.find(kernel_name ? kernel_name : "");
    if (total_ms) *total_ms = it == g_prof_done.end() ? 0.0 : it->second.first;
    if (launches) *launches = it == g_prof_done.end() ? 0 : it->second.second;
    return PPO_OK;
}

int32_t ppo_profile_returns(int64_t T, int64_t N, double discount, int32_t iters, double* avg_ms) {
    PPO_TRY(ensure_init());
    ARG_CHECK(T >= 1 && N >= 1 && iters >= 1 && avg_ms, "profile_returns: bad argument");
    const size_t n = (size_t)T * N;
    DevBuf<float> r, o; DevBuf<uint8_t> d;
    PPO_TRY(r.alloc(n)); PPO_TRY(o.alloc(n)); PPO_TRY(d.alloc(n));
    HIP_TRY(hipMemsetAsync(r.p, 0x3c, n * 4, g_stream));          // ~0.0115 everywhere
    HIP_TRY(hipMemsetAsync(d.p, 0, n, g_stream));
    PPO_TRY(launch_returns_tn(r.p, d.p, o.p, T, N, discount, 0)); // warm-up
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1));
    HIP_TRY(hipEventRecord(e0, g_stream));
    for (int i = 0; i < iters; ++i) PPO_TRY(launch_returns_tn(r.p, d.p, o.p, T, N, discount, 0));
    HIP_TRY(hipEventRecord(e1, g_stream));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *avg_ms = (double)ms / iters;
    return PPO_OK;
}

int32_t ppo_profile_gae(int64_t T, int64_t N, double gamma, double lambda, int32_t iters, double* avg_ms) {
    PPO_TRY(ensure_init());
    ARG_CHECK(T >= 1 && N >= 1 && iters >= 1 && avg_ms, "profile_gae: bad argument");
    const size_t n = (size_t)T * N;
    DevBuf<float> r, v, a, o; DevBuf<uint8_t> d;
    PPO_TRY(r.alloc(n)); PPO_TRY(v.alloc(n + N)); PPO_TRY(a.alloc(n)); PPO_TRY(o.alloc(n)); PPO_TRY(d.alloc(n));
    HIP_TRY(hipMemsetAsync(r.p, 0x3c, n * 4, g_stream));          // ~0.0115 everywhere
    HIP_TRY(hipMemsetAsync(v.p, 0x3c, (n + N) * 4, g_stream));
    HIP_TRY(hipMemsetAsync(d.p, 0, n, g_stream));
    PPO_TRY(launch_gae_tn(r.p, d.p, v.p, a.p, o.p, T, N, gamma, lambda));   // warm-up
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1));
    HIP_TRY(hipEventRecord(e0, g_stream));
    for (int i = 0; i < iters; ++i) PPO_TRY(launch_gae_tn(r.p, d.p, v.p, a.p, o.p, T, N, gamma, lambda));
    HIP_TRY(hipEventRecord(e1, g_stream));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *avg_ms = (double)ms / iters;
    return PPO_OK;
}

// ================================================================ standalone ops
int32_t ppo_compute_returns(const float* rewards, const uint8_t* terminal, int64_t n, double discount,
                            int32_t discount_is_f32, float* out) {
    PPO_TRY(ensure_init());
    ARG_CHECK(n >= 0 && (n == 0 || (rewards && terminal && out)), "compute_returns: null buffer");
    if (n == 0) return PPO_OK;
    DevBuf<float> r, o; DevBuf<uint8_t> t;
    PPO_TRY(r.alloc(n)); PPO_TRY(o.alloc(n)); PPO_TRY(t.alloc(n));
    PPO_TRY(h2d(r.p, rewards, n)); PPO_TRY(h2d(t.p, terminal, n));
    PPO_TRY(launch_returns_flat(r.p, t.p, o.p, n, discount, discount_is_f32));
    return d2h(out, o.p, n);
}

int32_t ppo_compute_returns_tn(const float* rewards, const uint8_t* done, int64_t T, int64_t N, double discount,
                               int32_t discount_is_f32, float* out) {
    PPO_TRY(ensure_init());
    ARG_CHECK(T >= 0 && N >= 0, "compute_returns_tn: negative size");
    const size_t n = (size_t)T * N;
    if (n == 0) return PPO_OK;
    ARG_CHECK(rewards && done && out, "compute_returns_tn: null buffer");
    DevBuf<float> r, o; DevBuf<uint8_t> t;
    PPO_TRY(r.alloc(n)); PPO_TRY(o.alloc(n)); PPO_TRY(t.alloc(n));
    PPO_TRY(h2d(r.p, rewards, n)); PPO_TRY(h2d(t.p, done, n));
    PPO_TRY(launch_returns_tn(r.p, t.p, o.p, T, N, discount, discount_is_f32));
    return d2h(out, o.p, n);
}

int32_t ppo_gae_tn(const float* rewards, const uint8_t* done, const float* values, int64_t T, int64_t N, double gamma,
                   double lambda, float* adv_out, float* ret_out) {
    PPO_TRY(ensure_init());
    const size_t n = (size_t)T * N;
    if (n == 0) return PPO_OK;
    ARG_CHECK(rewards && done && values && adv_out && ret_out, "gae_tn: null buffer");
    DevBuf<float> r, v, a, o; DevBuf<uint8_t> t;
    PPO_TRY(r.alloc(n)); PPO_TRY(v.alloc(n + N)); PPO_TRY(a.alloc(n)); PPO_TRY(o.alloc(n)); PPO_TRY(t.alloc(n));
    PPO_TRY(h2d(r.p, rewards, n)); PPO_TRY(h2d(t.p, done, n)); PPO_TRY(h2d(v.p, values, n + N));
    PPO_TRY(launch_gae_tn(r.p, t.p, v.p, a.p, o.p, T, N, gamma, lambda));
    PPO_TRY(d2h(adv_out, a.p, n));
    return d2h(ret_out, o.p, n);
}

int32_t ppo_gae_boot_tn(const float* rewards, const uint8_t* done, const float* values, const float* boot, int64_t T, int64_t N,
                        double gamma, double lambda, float* adv_out, float* ret_out) {
    ARG_CHECK(T >= 0 && N >= 0, "gae_boot_tn: negative size");
    const size_t n = (size_t)T * N;
    if (n == 0) return PPO_OK;
    ARG_CHECK(rewards && done && values && boot && adv_out && ret_out, "gae_boot_tn: null buffer");
    PPO_TRY(ensure_init());
    DevBuf<float> r, v, b, a, o; DevBuf<uint8_t> t;
    PPO_TRY(r.alloc(n)); PPO_TRY(v.alloc(n + N)); PPO_TRY(b.alloc(n)); PPO_TRY(a.alloc(n)); PPO_TRY(o.alloc(n)); PPO_TRY(t.alloc(n));
    PPO_TRY(h2d(r.p, rewards, n)); PPO_TRY(h2d(t.p, done, n)); PPO_TRY(h2d(v.p, values, n + N)); PPO_TRY(h2d(b.p, boot, n));
    PPO_TRY(launch_gae_boot_tn(r.p, t.p, v.p, b.p, a.p, o.p, T, N, gamma, lambda));
    PPO_TRY(d2h(adv_out, a.p, n));
    return d2h(ret_out, o.p, n);
}

int32_t ppo_categorical_sample(const float* probs, const float* u, int64_t B, int64_t A, int32_t* actions,
                               float* p_sel, int32_t* err) {
    PPO_TRY(ensure_init());
    ARG_CHECK(B >= 0 && A >= 1, "categorical_sample: bad shape");
    if (B == 0) return PPO_OK;
    DevBuf<float> p, uu, ps; DevBuf<int32_t> ac, er;
    PPO_TRY(p.alloc((size_t)B * A)); PPO_TRY(uu.alloc(B)); PPO_TRY(ps.alloc(B)); PPO_TRY(ac.alloc(B)); PPO_TRY(er.alloc(B));
    PPO_TRY(h2d(p.p, probs, (size_t)B * A)); PPO_TRY(h2d(uu.p, u, B));
    PPO_TRY(launch_categorical(p.p, uu.p, B, A, ac.p, ps.p, er.p));
    PPO_TRY(d2h(actions, ac.p, B)); PPO_TRY(d2h(p_sel, ps.p, B));
    return d2h(err, er.p, B);
}

int32_t ppo_linear_action_index(const int64_t* actions1, int64_t B, int64_t A, int64_t* out) {
    // src/train.jl:48-52: selected_actions + range(0, step=A, length=B).  Pure index arithmetic on
    // the host side of the ABI (it is fused into the loss kernel on the device path).
    ARG_CHECK(B >= 0 && A >= 1, "linear_action_index: bad shape");
    for (int64_t b = 0; b < B; ++b) out[b] = actions1[b] + b * A;
    return PPO_OK;
}

// ================================================================ env
int32_t ppo_env_create(int32_t kind, int64_t num_envs, int64_t global_env_offset, int32_t Q, int32_t max_actions,
                       float no_action_reward, uint64_t seed, ppo_env_t* out) {
    PPO_TRY(ensure_init());
    ARG_CHECK(out, "env_create: null out");
    ARG_CHECK(kind == 0, "env_create: only kind 0 (synthetic rand-poly-shaped env) is built in");
    ARG_CHECK(num_envs >= 1 && Q >= 2 && Q <= 32 && max_actions >= 1, "env_create: bad sizes");
    ppo_env_s* e = new ppo_env_s();
    e->kind = kind; e->Q = Q; e->H = 4 * Q; e->A = 16 * Q; e->V = 4 * Q; e->F = 2 * PPO_TPL;
    e->max_actions = max_actions; e->no_action_reward = no_action_reward; e->N = num_envs;
    e->global_offset = global_env_offset; e->seed = seed;
    const size_t N = (size_t)num_envs;
    int32_t s = PPO_OK;
    if ((s = e->score.alloc(N * e->V)) || (s = e->degree.alloc(N * e->V)) || (s = e->active.alloc(N)) ||
        (s = e->steps.alloc(N)) || (s = e->reward.alloc(N)) || (s = e->done.alloc(N)) || (s = e->episode.alloc(N)) ||
        (s = e->tick.alloc(N)) || (s = e->err.alloc(1)) || (s = e->actions_tmp.alloc(N)) ||
        (s = e->episodes_left.alloc(N)) || (s = e->tmpl.alloc((size_t)e->H * PPO_TPL))) { delete e; return s; }
    {   // the observation template depends on (half-edge, template row) only: tabulated once (1-4.5 KB, cache resident)
        std::vector<int8_t> t((size_t)e->H * PPO_TPL);
        for (int h = 0; h < e->H; ++h)
            for (int k = 0; k < PPO_TPL; ++k) t[(size_t)h * PPO_TPL + k] = (int8_t)env_template(Q, h, k);
        s = h2d(e->tmpl.p, t.data(), t.size());
        if (s) { delete e; return s; }
    }
    (void)hipMemsetAsync(e->episode.p, 0, N * 4, g_stream);
    (void)hipMemsetAsync(e->tick.p, 0, N * 4, g_stream);
    (void)hipMemsetAsync(e->err.p, 0, 4, g_stream);
    (void)hipMemsetAsync(e->done.p, 0, N, g_stream);
    (void)hipMemsetAsync(e->episodes_left.p, 0, N * 4, g_stream);
    s = launch_env_reset(e, 0);
    if (s) { delete e; return s; }
    *out = e;
    return PPO_OK;
}

int32_t ppo_env_destroy(ppo_env_t env) { if (env) { (void)hipStreamSynchronize(g_stream); delete env; } return PPO_OK; }

int32_t ppo_env_dims(ppo_env_t env, int64_t* N, int32_t* H, int32_t* F, int32_t* A) {
    ARG_CHECK(env, "env_dims: null env");
    if (N) *N = env->N; if (H) *H = env->H; if (F) *F = env->F; if (A) *A = env->A;
    return PPO_OK;
}

// state storage of engine-collected rollouts: automatic (rollout_compact = -1): compact env snapshots when the expanded
// observations of the requested rollout would exceed PPO_COMPACT_AUTO_BYTES -- default 32 GiB: re-deriving the rows costs
// the train forward 3 % in fp32 and 17 % in bf16 mode, so below that the 288 GB of HBM are spent on speed -- or when a disk
// sink is attached: the stream then carries 64 + 4 instead of 2304 + 4 state bytes per env-step for Q = 8
bool want_compact(const ppo_rollouts_s* ro, int64_t T) {
    const PpoKnobs& k = ppo_knobs();
    if (ro->V == 0) return false;                             // created by shape: no env snapshot form
    if (k.rollout_compact >= 0) return k.rollout_compact == 1;
    if (ro->sink) return true;
    return (double)T * (double)ro->N * ro->H * ro->F > k.compact_auto_bytes;
}

int32_t ppo_env_set_strict_sampling(ppo_env_t env, int32_t strict) { ARG_CHECK(env, "null env"); env->strict_sampling = strict ? 1 : 0; return PPO_OK; }

int32_t ppo_env_reset(ppo_env_t env) { ARG_CHECK(env, "reset!: null env"); return launch_env_reset(env, 0); }

int32_t ppo_env_check_errors(ppo_env_t env, int32_t* flags_or_null) {
    ARG_CHECK(env, "null env");
    int32_t f = 0;
    PPO_TRY(d2h(&f, env->err.p, 1));
    if (flags_or_null) *flags_or_null = f;
    if (f & ~(env->strict_sampling ? 0 : 32)) {     // bit 32 is informational unless strict: a CDF rounding residue went to the last unmasked action
        std::string m = "AssertionError (device flag):";
        if (f & 1) m += " action on inactive quad;";
        if (f & 2) m += " action index out of range;";
        if (f & 4) m += " step! on a terminated env;";
        if (f & 8) m += " sampled action has probability 0 (ap[a] > 0.0 failed, src/collect_rollouts.jl:7);";
        if (f & 32) m += " the CDF walk ended on a masked action (ap[a] > 0.0 would fail in the reference; strict sampling);";
        ppo_set_error(m);
        return PPO_ERR_DEVICE_FLAG;
    }
    return PPO_OK;
}

int32_t ppo_env_step(ppo_env_t env, const int32_t* actions0) {
    ARG_CHECK(env && actions0, "step!: null argument");
    PPO_TRY(h2d(env->actions_tmp.p, actions0, (size_t)env->N));
    PPO_TRY(launch_env_step(env, env->actions_tmp.p, nullptr, nullptr, nullptr, 0, 0));
    return ppo_env_check_errors(env, nullptr);
}

int32_t ppo_env_get_state(ppo_env_t env, int8_t* obs, uint32_t* active) {
    ARG_CHECK(env && obs, "state: null argument");
    const size_t n = (size_t)env->N * env->H * env->F;
    PPO_TRY(env->obs_tmp.alloc(n));
    PPO_TRY(launch_env_observe(env, env->obs_tmp.p, nullptr));
    PPO_TRY(d2h(obs, env->obs_tmp.p, n));
    if (active) PPO_TRY(d2h(active, env->active.p, (size_t)env->N));
    return PPO_OK;
}

int32_t ppo_env_get_reward(ppo_env_t env, float* out) { ARG_CHECK(env && out, "reward: null"); return d2h(out, env->reward.p, (size_t)env->N); }
int32_t ppo_env_get_terminal(ppo_env_t env, uint8_t* out) { ARG_CHECK(env && out, "is_terminal: null"); return d2h(out, env->done.p, (size_t)env->N); }

int32_t ppo_env_get_internal(ppo_env_t env, int8_t* score, int8_t* degree, int32_t* steps, uint32_t* episode,
                             uint32_t* tick) {
    ARG_CHECK(env, "null env");
    const size_t N = (size_t)env->N;
    if (score) PPO_TRY(d2h(score, env->score.p, N * env->V));
    if (degree) PPO_TRY(d2h(degree, env->degree.p, N * env->V));
    if (steps) PPO_TRY(d2h(steps, env->steps.p, N));
    if (episode) PPO_TRY(d2h(episode, env->episode.p, N));
    if (tick) PPO_TRY(d2h(tick, env->tick.p, N));
    return PPO_OK;
}

// what ppo_env_set_internal and ppo_search_best_states require of caller-supplied env states ([count][V] each, [count]
// active-quad words): a state reset! or step! could have left.  Checked on the host before anything is uploaded
int32_t check_internal_host(int32_t Q, int64_t count, const int8_t* score, const int8_t* degree, const uint32_t* active) {
    const int V = 4 * Q;
    for (int64_t n = 0; n < count; ++n) {
        const uint32_t act = active[n];
        ARG_CHECK(act != 0, "env state: no active quad");
        ARG_CHECK(Q >= 32 || (act >> Q) == 0, "env state: active bit at or above Q");
        for (int v = 0; v < V; ++v)
            if (!((act >> (v >> 2)) & 1u))
                ARG_CHECK(score[n * V + v] == 0 && degree[n * V + v] == 0, "env state: nonzero entry of an inactive quad");
    }
    return PPO_OK;
}

int32_t ppo_env_set_internal(ppo_env_t env, const int8_t* score, const int8_t* degree, const uint32_t* active) {
    ARG_CHECK(env && score && degree && active, "env_set_internal: null argument");
    PPO_TRY(check_internal_host(env->Q, env->N, score, degree, active));
    const size_t N = (size_t)env->N;
    PPO_TRY(h2d(env->score.p, score, N * env->V));
    PPO_TRY(h2d(env->degree.p, degree, N * env->V));
    PPO_TRY(h2d(env->active.p, active, N));
    HIP_TRY(hipMemsetAsync(env->steps.p, 0, N * 4, g_stream));         // as reset! leaves them; episode and tick stay
    HIP_TRY(hipMemsetAsync(env->reward.p, 0, N * 4, g_stream));
    HIP_TRY(hipMemsetAsync(env->done.p, 0, N, g_stream));
    HIP_TRY(hipStreamSynchronize(g_stream));
    return PPO_OK;
}

int32_t ppo_env_get_active(ppo_env_t env, uint32_t* active) {
    ARG_CHECK(env && active, "env_get_active: null argument");
    return d2h(active, env->active.p, (size_t)env->N);
}

// ================================================================ policy
// Hidden widths other than 128 / 256 run on the next wider kernel with ZERO-PADDED hidden units.  That is exact, not an
// approximation: a padded unit has zero input weights and zero bias, so its activation is leakyrelu(0) = 0; its outgoing
// weights are zero, so it adds fmaf(0, 0, acc) = acc to every sum it enters; and every gradient that touches it carries
// one of those zeros as a factor (dZ2[pad] = (W3^T dY)[pad] = 0, H1[pad] = 0, dH1[pad] = (W2^T dZ2)[pad] = 0), so Adam
// (m = v = 0 -> update 0 / (sqrt(0) + eps) = 0) never moves it.  The caller sees its own Policy(F, hidden, 2, 4): the flat
// Flux-order vectors that cross the ABI (parameters, gradient, Adam moments) have the caller's layout.
static __host__ __device__ inline int64_t np_of(int64_t F, int64_t hid, int64_t L = 2) {
    return hid * F + hid + (L - 1) * (hid * hid + hid) + (int64_t)PPO_OUT * hid + PPO_OUT;
}

// index of the caller's flat element i (width hu, L hidden layers) in the flat vector at width hp
__device__ __forceinline__ int64_t pad_index(int64_t i, int F, int hu, int hp, int L) {
    const int64_t uW2 = (int64_t)hu * F + hu, uper = (int64_t)hu * hu + hu, uW3 = uW2 + (L - 1) * uper;
    const int64_t pW2 = (int64_t)hp * F + hp, pper = (int64_t)hp * hp + hp, pW3 = pW2 + (L - 1) * pper;
    if (i < (int64_t)hu * F) return (i % hu) + (int64_t)hp * (i / hu);                  // W1[o][k]
    if (i < uW2) return (int64_t)hp * F + (i - (int64_t)hu * F);                        // b1
    if (i < uW3) {                                                                     // hidden->hidden layer: W[o][k], then b
        const int64_t lay = (i - uW2) / uper, e = (i - uW2) - lay * uper;
        if (e < (int64_t)hu * hu) return pW2 + lay * pper + (e % hu) + (int64_t)hp * (e / hu);
        return pW2 + lay * pper + (int64_t)hp * hp + (e - (int64_t)hu * hu);
    }
    return pW3 + (i - uW3);                                                            // W3[4][k] (k < hu), b3: b3 follows W3
}
__global__ void k_pad_copy(float* __restrict__ user, float* __restrict__ padded, int64_t n_user, int F, int hu, int hp, int L, int to_user) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_user) return;
    // b3 sits behind W3 in both layouts, but W3 is [4][hid]: the last 4 elements are b3
    const int64_t pi = (i >= n_user - PPO_OUT) ? (np_of(F, hp, L) - (n_user - i)) : pad_index(i, F, hu, hp, L);
    if (to_user) user[i] = padded[pi]; else padded[pi] = user[i];
}
// host flat vector (caller's layout) <-> device flat vector at the kernels' width
static int32_t flat_to_device(ppo_policy_s* p, const float* host, float* dev_padded) {
    if (p->hid_user == p->HID) return h2d(dev_padded, host, (size_t)p->np);
    DevBuf<float> tmp;
    PPO_TRY(tmp.alloc((size_t)p->np_user));
    PPO_TRY(h2d(tmp.p, host, (size_t)p->np_user));
    HIP_TRY(hipMemsetAsync(dev_padded, 0, (size_t)p->np * sizeof(float), g_stream));
    hipLaunchKernelGGL(k_pad_copy, dim3((unsigned)((p->np_user + 255) / 256)), dim3(256), 0, g_stream, tmp.p, dev_padded,
                       p->np_user, p->F, p->hid_user, p->HID, p->L, 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g_stream));
    return PPO_OK;
}
static int32_t flat_to_host(ppo_policy_s* p, float* host, const float* dev_padded) {
    if (p->hid_user == p->HID) return d2h(host, dev_padded, (size_t)p->np);
    DevBuf<float> tmp;
    PPO_TRY(tmp.alloc((size_t)p->np_user));
    hipLaunchKernelGGL(k_pad_copy, dim3((unsigned)((p->np_user + 255) / 256)), dim3(256), 0, g_stream, tmp.p,
                       const_cast<float*>(dev_padded), p->np_user, p->F, p->hid_user, p->HID, p->L, 1);
    HIP_TRY(hipGetLastError());
    return d2h(host, tmp.p, (size_t)p->np_user);
}

int32_t ppo_policy_create(int32_t F, int32_t hidden_user, int32_t num_hidden_layers, int32_t out_per_edge,
                          ppo_policy_t* out) {
    PPO_TRY(ensure_init());
    ARG_CHECK(out, "policy_create: null out");
    const int32_t hidden = hidden_user <= 128 ? 128 : 256;                  // width of the kernels that run it
    if (num_hidden_layers < 1 || num_hidden_layers > 4 || out_per_edge != PPO_OUT || hidden_user < 1 || hidden_user > 256 ||
        !(F == 72 || F == 216)) {
        ppo_set_error("policy_create: the gfx950 kernels cover Policy(F, hidden, num_hidden_layers, 4) with F in {72, 216}, "
                      "hidden in 1..256 and num_hidden_layers in 1..4 (test/policy.jl:9-19, test/test_square_mesh.jl:29, "
                      "test/output/*.bson, BASELINE config 2); hidden widths other than 128 / 256 run zero-padded on the "
                      "next wider kernel; out must be the quad game's 4 actions per edge (test/quad_game_utilities.jl:95)");
        return PPO_ERR_UNSUPPORTED;
    }
    const int32_t NL2 = num_hidden_layers - 1;
    ppo_policy_s* p = new ppo_policy_s();
    p->F = F; p->HID = hidden; p->L = num_hidden_layers; p->OUT = out_per_edge;
    p->hid_user = hidden_user; p->np_user = np_of(F, hidden_user, num_hidden_layers);
    p->np = np_of(F, hidden, num_hidden_layers);
    int32_t s = PPO_OK;
    if ((s = p->params.alloc(p->np)) || (s = p->w1p.alloc((size_t)hidden * F + PPO_PACK_PAD)) ||
        (s = p->w2p.alloc((size_t)NL2 * hidden * hidden + PPO_PACK_PAD)) ||
        (s = p->w2tp.alloc((size_t)NL2 * hidden * hidden + PPO_PACK_PAD)) || (s = p->b1p.alloc(hidden)) ||
        (s = p->b2p.alloc((size_t)(NL2 > 0 ? NL2 : 1) * hidden)) ||
        (s = p->w3p.alloc((size_t)hidden * PPO_OUT)) || (s = p->b3.alloc(PPO_OUT)) || (s = p->grad.alloc(p->np + 2)) ||
        (s = p->err.alloc(1))) { delete p; return s; }
    if (num_hidden_layers == 2 && F == 72) {             // zero padding: the operand rings of the last k-steps read ahead (bf16 elements here)
        if ((s = p->w2x.alloc((size_t)3 * hidden * hidden + PPO_X6_W2_PAD_BYTES / 2))) { delete p; return s; }
        (void)hipMemsetAsync(p->w2x.p, 0, p->w2x.n * 2, g_stream);
        if ((s = p->w2fx.alloc((size_t)3 * hidden * hidden + PPO_X6_W2_PAD_BYTES / 2)) ||
            (s = p->w1x.alloc((size_t)(hidden / 32) * 5 * 3 * 512 + PPO_X6_W1_PAD_BYTES / 2))) { delete p; return s; }
        (void)hipMemsetAsync(p->w2fx.p, 0, p->w2fx.n * 2, g_stream);
        (void)hipMemsetAsync(p->w1x.p, 0, p->w1x.n * 2, g_stream);       // inputs 72 .. 79 of the last k-step stay zero
    }
    (void)hipMemsetAsync(p->params.p, 0, p->np * 4, g_stream);
    (void)hipMemsetAsync(p->w1p.p, 0, p->w1p.n * 4, g_stream);
    (void)hipMemsetAsync(p->w2p.p, 0, p->w2p.n * 4, g_stream);
    (void)hipMemsetAsync(p->w2tp.p, 0, p->w2tp.n * 4, g_stream);
    (void)hipMemsetAsync(p->grad.p, 0, (p->np + 2) * 4, g_stream);
    (void)hipMemsetAsync(p->err.p, 0, 4, g_stream);
    s = launch_pack_params(p);
    if (s) { delete p; return s; }
    *out = p;
    return PPO_OK;
}

int32_t ppo_policy_set_dtype(ppo_policy_t pol, int32_t dtype) {
    ARG_CHECK(pol, "policy_set_dtype: null policy");
    ARG_CHECK(dtype == PPO_DTYPE_F32 || dtype == PPO_DTYPE_BF16, "policy_set_dtype: dtype must be PPO_DTYPE_F32 or PPO_DTYPE_BF16");
    if (dtype == PPO_DTYPE_BF16 && (pol->L != 2 || pol->F != 72)) {
        ppo_set_error("policy_set_dtype: the bf16 kernels cover Policy(72, hidden, 2, 4) only");
        return PPO_ERR_UNSUPPORTED;
    }
    if (dtype == PPO_DTYPE_BF16 && !pol->w1b.p) {
        const size_t HID = pol->HID, KS1 = bf16_ks1(pol->F);
        PPO_TRY(pol->w1b.alloc(HID * KS1 * 16)); PPO_TRY(pol->w2b.alloc(HID * HID)); PPO_TRY(pol->w2tb.alloc(HID * HID));
        PPO_TRY(pol->w3c.alloc(HID * PPO_OUT)); PPO_TRY(pol->w3tb.alloc(HID * PPO_OUT));
        HIP_TRY(hipMemsetAsync(pol->w1b.p, 0, pol->w1b.n * 2, g_stream));      // k-slots >= F stay zero
    }
    pol->dtype = dtype;
    return launch_pack_params(pol);
}
int32_t ppo_policy_get_dtype(ppo_policy_t pol, int32_t* dtype) { ARG_CHECK(pol && dtype, "null"); *dtype = pol->dtype; return PPO_OK; }

int32_t ppo_policy_destroy(ppo_policy_t pol) { if (pol) { (void)hipStreamSynchronize(g_stream); delete pol; } return PPO_OK; }
int32_t ppo_policy_num_params(ppo_policy_t pol, int64_t* n) { ARG_CHECK(pol && n, "null"); *n = pol->np_user; return PPO_OK; }

int32_t ppo_policy_set_params(ppo_policy_t pol, const float* flat) {
    ARG_CHECK(pol && flat, "set_params: null");
    PPO_TRY(flat_to_device(pol, flat, pol->params.p));
    return launch_pack_params(pol);
}
int32_t ppo_policy_get_params(ppo_policy_t pol, float* flat) { ARG_CHECK(pol && flat, "get_params: null"); return flat_to_host(pol, flat, pol->params.p); }
int32_t ppo_policy_get_grad(ppo_policy_t pol, float* flat) { ARG_CHECK(pol && flat, "get_grad: null"); return flat_to_host(pol, flat, pol->grad.p); }
int32_t ppo_policy_grad_buffer_dev(ppo_policy_t pol, void** dev_ptr, int64_t* n_floats) {
    ARG_CHECK(pol && dev_ptr && n_floats, "grad_buffer_dev: null");
    *dev_ptr = pol->grad.p; *n_floats = pol->np + 2;
    return PPO_OK;
}

int32_t ppo_policy_forward(ppo_policy_t pol, const int8_t* states, const uint32_t* active, int64_t B, int32_t H,
                           float* probs) {
    ARG_CHECK(pol && states && active && probs, "batch_action_probabilities: null argument");
    ARG_CHECK(B >= 1, "batch_action_probabilities: empty batch");
    if (H != 32 && H != 128) { ppo_set_error("policy_forward: H must be 32 (Q=8) or 128 (Q=32) half-edges in this build"); return PPO_ERR_UNSUPPORTED; }
    DevBuf<int8_t> s; DevBuf<uint32_t> a; DevBuf<float> p;
    const size_t ns = (size_t)B * H * pol->F;
    PPO_TRY(s.alloc(ns)); PPO_TRY(a.alloc(B)); PPO_TRY(p.alloc((size_t)B * H * 4));
    PPO_TRY(h2d(s.p, states, ns)); PPO_TRY(h2d(a.p, active, (size_t)B));
    PPO_TRY(launch_policy_probs(pol, s.p, a.p, B, H, p.p));
    return d2h(probs, p.p, (size_t)B * H * 4);
}

// ---- action selection of the calls behind play_quotas (ppo_play.hip; no reference op): a property of the
// policy handle
int32_t ppo_policy_set_selection(ppo_policy_t pol, int32_t rule, double temperature) {
    ARG_CHECK(rule == PPO_SELECT_SAMPLE || rule == PPO_SELECT_GREEDY, "policy_set_selection: rule must be 0 (sample) or 1 (greedy)");
    ARG_CHECK(std::isfinite(temperature) && temperature > 0.0, "policy_set_selection: temperature must be finite and > 0");
    ARG_CHECK(pol, "policy_set_selection: null policy");
    pol->select_rule = rule;
    pol->select_temperature = temperature;
    return PPO_OK;
}
int32_t ppo_policy_get_selection(ppo_policy_t pol, int32_t* rule, double* temperature) {
    ARG_CHECK(pol && rule && temperature, "policy_get_selection: null argument");
    *rule = pol->select_rule;
    *temperature = pol->select_temperature;
    return PPO_OK;
}
// ---- truncation of the distribution the "sample" rule draws from (no reference op), read where the selection is
int32_t ppo_policy_set_truncation(ppo_policy_t pol, int32_t top_k, double top_p) {
    ARG_CHECK(top_k >= 0, "policy_set_truncation: top_k must be >= 0 (0: no limit)");
    ARG_CHECK(top_p > 0.0 && top_p <= 1.0, "policy_set_truncation: top_p must be in (0, 1] (1: no limit)");     // NaN fails both
    ARG_CHECK(pol, "policy_set_truncation: null policy");
    pol->trunc_top_k = top_k;
    pol->trunc_top_p = top_p;
    return PPO_OK;
}
int32_t ppo_policy_get_truncation(ppo_policy_t pol, int32_t* top_k, double* top_p) {
    ARG_CHECK(pol && top_k && top_p, "policy_get_truncation: null argument");
    *top_k = pol->trunc_top_k;
    *top_p = pol->trunc_top_p;
    return PPO_OK;
}

// ================================================================ optimiser
// every handle is a Flux.Optimiser chain (include/ppo_hip.h); ppo_adam_* are the chain of Adam alone
int32_t ppo_adam_create(ppo_policy_t pol, double eta, double beta1, double beta2, double eps, ppo_adam_t* out) {
    const int32_t kind = PPO_OPT_ADAM;
    const double hyper[5] = {eta, beta1, beta2, eps, 0.0};
    return ppo_optimiser_create(pol, 1, &kind, hyper, out);
}
int32_t ppo_adam_destroy(ppo_adam_t opt) { if (opt) { (void)hipStreamSynchronize(g_stream); delete opt; } return PPO_OK; }
int32_t ppo_adam_get_lr(ppo_adam_t opt, double* eta) { ARG_CHECK(opt && eta, "null"); *eta = opt->lr(); return PPO_OK; }
int32_t ppo_adam_set_lr(ppo_adam_t opt, double eta) {
    ARG_CHECK(opt && opt->adam_only(), "adam_set_lr: null, or a chain (ppo_optimiser_set_eta)");
    return ppo_optimiser_set_eta(opt, 0, eta);
}
int32_t ppo_adam_get_state(ppo_adam_t opt, float* m, float* v, double* bp) {
    ARG_CHECK(opt && opt->adam_only(), "adam_get_state: null, or a chain (ppo_optimiser_get_state)");
    return ppo_optimiser_get_state(opt, 0, m, v, bp, nullptr);
}
int32_t ppo_adam_set_state(ppo_adam_t opt, const float* m, const float* v, const double* bp) {
    ARG_CHECK(opt && opt->adam_only(), "adam_set_state: null, or a chain (ppo_optimiser_set_state)");
    return ppo_optimiser_set_state(opt, 0, m, v, bp, nullptr);
}

int32_t ppo_adam_get_epoch_count(ppo_adam_t opt, int64_t* epochs) { ARG_CHECK(opt && epochs, "null"); *epochs = opt->epochs_done; return PPO_OK; }
int32_t ppo_adam_set_epoch_count(ppo_adam_t opt, int64_t epochs) { ARG_CHECK(opt && epochs >= 0, "bad epoch count"); opt->epochs_done = epochs; return PPO_OK; }

double ppo_adam_s::lr() const {
    double p = 1.0;                                     // get_optimizer_learning_rate: prod(opt.eta for opt in optimizer)
    for (int j = 0; j < nmem; ++j)                      // the members without eta are skipped (the reference would fail)
        if (has_eta(mem[j].kind)) p *= mem[j].eta;
    return p;
}

// a member's hyper row (include/ppo_hip.h): PPO_OK, or PPO_ERR_ARG with the reason
static int32_t check_hyper(int32_t kind, const double* h) {
    if (kind == PPO_OPT_EXPDECAY)
        ARG_CHECK(h[2] >= 1 && h[2] == std::floor(h[2]) && h[4] == std::floor(h[4]), "ExpDecay: integer decay_step >= 1 and start");
    if (kind == PPO_OPT_CLIPVALUE || kind == PPO_OPT_CLIPNORM)
        ARG_CHECK(h[0] >= 0, std::string(kind == PPO_OPT_CLIPNORM ? "ClipNorm" : "ClipValue") + ": thresh must be >= 0 (and not NaN)");
    return PPO_OK;
}

static int32_t alloc_zeroed(DevBuf<float>& b, size_t n) {
    PPO_TRY(b.alloc(n));
    (void)hipMemsetAsync(b.p, 0, n * 4, g_stream);
    return PPO_OK;
}

int32_t ppo_optimiser_create(ppo_policy_t pol, int32_t n, const int32_t* kinds, const double* hyper, ppo_adam_t* out) {
    ARG_CHECK(pol && kinds && hyper && out, "optimiser_create: null");
    ARG_CHECK(n >= 1 && n <= 4, "optimiser_create: a chain of 1 to 4 members");
    for (int32_t j = 0; j < n; ++j) {
        if (kinds[j] < PPO_OPT_ADAM || kinds[j] > PPO_OPT_INVDECAY) {
            ppo_set_error("optimiser_create: member " + std::to_string(j) + " has an unknown kind " + std::to_string(kinds[j]));
            return PPO_ERR_UNSUPPORTED;
        }
        for (int32_t k = 0; k < j; ++k) ARG_CHECK(kinds[k] != kinds[j], "optimiser_create: each member kind at most once");
        PPO_TRY(check_hyper(kinds[j], hyper + 5 * (size_t)j));
    }
    ppo_adam_s* o = new ppo_adam_s();
    o->pol = pol; o->nmem = n;
    int32_t s = PPO_OK;
    for (int32_t j = 0; j < n && s == PPO_OK; ++j) {
        const double* h = hyper + 5 * (size_t)j;
        OptMember& e = o->mem[j];
        e.kind = kinds[j];
        e.eta = h[0]; e.h1 = h[1]; e.h2 = h[2]; e.h3 = h[3]; e.h4 = h[4];
        const bool adam = e.kind == PPO_OPT_ADAM;
        if (adam) { e.beta_pow[0] = h[1]; e.beta_pow[1] = h[2]; }
        if (adam || e.kind == PPO_OPT_MOMENTUM || e.kind == PPO_OPT_NESTEROV || e.kind == PPO_OPT_RMSPROP) s = alloc_zeroed(e.s, pol->np);
        if (adam && s == PPO_OK) s = alloc_zeroed(e.s1, pol->np);
        if (e.kind == PPO_OPT_CLIPNORM) {
            o->clip_slots = clip_slot_count(pol);
            if ((s = o->clip_d.alloc(pol->np)) || (s = o->clip_part.alloc(2 * (size_t)o->clip_slots))) break;
        }
    }
    if (s != PPO_OK) { delete o; return s; }
    *out = o;
    return PPO_OK;
}

static int32_t chain_member(ppo_adam_t opt, int32_t member) {
    ARG_CHECK(opt && member >= 0 && member < opt->nmem, "optimiser: null handle or member out of range");
    return PPO_OK;
}

int32_t ppo_optimiser_get_eta(ppo_adam_t opt, int32_t member, double* eta) {
    PPO_TRY(chain_member(opt, member));
    ARG_CHECK(eta, "null");
    ARG_CHECK(has_eta(opt->mem[member].kind), "optimiser_get_eta: the member has no eta (ppo_optimiser_get_hyper)");
    *eta = opt->mem[member].eta;
    return PPO_OK;
}
int32_t ppo_optimiser_set_eta(ppo_adam_t opt, int32_t member, double eta) {
    PPO_TRY(chain_member(opt, member));
    ARG_CHECK(has_eta(opt->mem[member].kind), "optimiser_set_eta: the member has no eta (ppo_optimiser_set_hyper)");
    opt->mem[member].eta = eta;
    return PPO_OK;
}
int32_t ppo_optimiser_get_hyper(ppo_adam_t opt, int32_t member, double* h) {
    PPO_TRY(chain_member(opt, member));
    ARG_CHECK(h, "null");
    const OptMember& e = opt->mem[member];
    h[0] = e.eta; h[1] = e.h1; h[2] = e.h2; h[3] = e.h3; h[4] = e.h4;
    return PPO_OK;
}
int32_t ppo_optimiser_set_hyper(ppo_adam_t opt, int32_t member, const double* h) {
    PPO_TRY(chain_member(opt, member));
    ARG_CHECK(h, "null");
    OptMember& e = opt->mem[member];
    PPO_TRY(check_hyper(e.kind, h));
    e.eta = h[0]; e.h1 = h[1]; e.h2 = h[2]; e.h3 = h[3]; e.h4 = h[4];   // Adam: the beta powers stay
    return PPO_OK;
}
int32_t ppo_optimiser_get_state(ppo_adam_t opt, int32_t member, float* s0, float* s1, double* scalars2, int64_t* count) {
    PPO_TRY(chain_member(opt, member));
    const OptMember& e = opt->mem[member];
    if (s0 && e.s.p) PPO_TRY(flat_to_host(opt->pol, s0, e.s.p));
    if (s1 && e.s1.p) PPO_TRY(flat_to_host(opt->pol, s1, e.s1.p));
    if (scalars2 && e.kind == PPO_OPT_ADAM) { scalars2[0] = e.beta_pow[0]; scalars2[1] = e.beta_pow[1]; }
    if (count) *count = e.count;                        // 0 for every member but ExpDecay / InvDecay
    return PPO_OK;
}
int32_t ppo_optimiser_set_state(ppo_adam_t opt, int32_t member, const float* s0, const float* s1, const double* scalars2,
                                const int64_t* count) {
    PPO_TRY(chain_member(opt, member));
    OptMember& e = opt->mem[member];
    if (s0 && e.s.p) PPO_TRY(flat_to_device(opt->pol, s0, e.s.p));
    if (s1 && e.s1.p) PPO_TRY(flat_to_device(opt->pol, s1, e.s1.p));
    if (scalars2 && e.kind == PPO_OPT_ADAM) { e.beta_pow[0] = scalars2[0]; e.beta_pow[1] = scalars2[1]; }
    if (count && (e.kind == PPO_OPT_EXPDECAY || e.kind == PPO_OPT_INVDECAY)) { ARG_CHECK(*count >= 0, "negative update count"); e.count = *count; }
    return PPO_OK;
}

// ================================================================ rollouts
// capacity for T steps in the requested state-storage form (the other form's buffer is released: the two differ by
// 36x in size and a buffer switches form only when the caller changes ppo_set_rollout_compact between collections)
int32_t rollouts_reserve(ppo_rollouts_s* r, int64_t T, bool compact) {
    const int64_t cap = std::max(T, r->capT);
    const size_t n = (size_t)cap * r->N;
    if (compact) { PPO_TRY(r->cstate.alloc(n * 2 * r->V)); r->states.release(); }
    else { PPO_TRY(r->states.alloc(n * r->H * r->F)); r->cstate.release(); }
    r->compact = compact;
    if (T <= r->capT) return PPO_OK;
    PPO_TRY(r->active.alloc(n)); PPO_TRY(r->actions.alloc(n));
    PPO_TRY(r->p_sel.alloc(n)); PPO_TRY(r->rewards.alloc(n)); PPO_TRY(r->returns.alloc(n)); PPO_TRY(r->done.alloc(n));
    PPO_TRY(r->valid.alloc(n)); PPO_TRY(r->index.alloc(n));
    r->capT = T;
    return PPO_OK;
}

int32_t ppo_rollouts_create(ppo_env_t env, int64_t capacity_T, ppo_rollouts_t* out) {
    PPO_TRY(ensure_init());
    ARG_CHECK(env && out && capacity_T >= 0, "BufferRollouts: bad argument");
    ppo_rollouts_s* r = new ppo_rollouts_s();
    r->N = env->N; r->H = env->H; r->F = env->F; r->A = env->A; r->V = env->V; r->capT = 0; r->T = 0; r->len = 0;
    int32_t s = r->tmpl.alloc((size_t)env->H * PPO_TPL);
    if (!s && hipMemcpyAsync(r->tmpl.p, env->tmpl.p, (size_t)env->H * PPO_TPL, hipMemcpyDeviceToDevice, g_stream) != hipSuccess) s = PPO_ERR_HIP;
    if (!s) s = rollouts_reserve(r, capacity_T, want_compact(r, capacity_T));
    if (s) { delete r; return s; }
    *out = r;
    return PPO_OK;
}
// BufferRollouts for states that do not come from the built-in env: any feature count the policy kernels take (F = 72 or
// 216 int8 features per half-edge row), H = 32 or 128 rows.  Host-supplied columns only (ppo_rollouts_set): the
// expanded storage form, no env template.
int32_t ppo_rollouts_create_shape(int64_t num_envs, int32_t H, int32_t F, int64_t capacity_T, ppo_rollouts_t* out) {
    PPO_TRY(ensure_init());
    ARG_CHECK(out && num_envs >= 1 && capacity_T >= 0, "BufferRollouts: bad argument");
    ARG_CHECK((H == 32 || H == 128) && F >= 8 && F % 8 == 0, "BufferRollouts: H must be 32 or 128 rows, F a multiple of 8");
    ppo_rollouts_s* r = new ppo_rollouts_s();
    r->N = num_envs; r->H = H; r->F = F; r->A = 4 * H; r->V = 0; r->capT = 0; r->T = 0; r->len = 0;
    const int32_t s = rollouts_reserve(r, capacity_T, false);
    if (s) { delete r; return s; }
    *out = r;
    return PPO_OK;
}
int32_t ppo_rollouts_destroy(ppo_rollouts_t ro) { if (ro) { (void)hipStreamSynchronize(g_stream); delete ro; } return PPO_OK; }
int32_t ppo_rollouts_len(ppo_rollouts_t ro, int64_t* n) { ARG_CHECK(ro && n, "length: null"); *n = ro->len; return PPO_OK; }
int32_t ppo_rollouts_dims(ppo_rollouts_t ro, int64_t* T, int64_t* N) {
    ARG_CHECK(ro, "null"); if (T) *T = ro->T; if (N) *N = ro->N; return PPO_OK;
}

__global__ void k_iota(int32_t* p, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = (int32_t)i;
}

int32_t set_index_all(ppo_rollouts_s* r) {
    const int64_t n = r->T * r->N;
    r->len = n; r->all_valid = true;
    if (n == 0) return PPO_OK;
    hipLaunchKernelGGL(k_iota, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, g_stream, r->index.p, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(r->valid.p, 1, (size_t)n, g_stream));
    return PPO_OK;
}

int32_t check_shapes(ppo_rollouts_s* ro, ppo_env_s* env, ppo_policy_s* pol) {
    ARG_CHECK(ro && env && pol, "collect_rollouts!: null argument");
    ARG_CHECK(ro->N == env->N && ro->H == env->H && ro->F == env->F, "collect_rollouts!: rollouts were created for another env shape");
    ARG_CHECK(pol->F == env->F, "collect_rollouts!: policy input width != env feature count");
    if (env->H != 32 && env->H != 128) { ppo_set_error("collect_rollouts!: H must be 32 (Q=8) or 128 (Q=32) half-edges in this build"); return PPO_ERR_UNSUPPORTED; }
    return PPO_OK;
}

int32_t ppo_collect_rollouts(ppo_rollouts_t ro, ppo_env_t env, ppo_policy_t pol, int64_t T, double discount,
                             int32_t discount_is_f32, int32_t record_probs) {
    PPO_TRY(check_shapes(ro, env, pol));
    ARG_CHECK(T >= 1, "collect_rollouts!: T must be >= 1");
    PPO_TRY(disk_sink_settle_previous(ro));        // a failed deferred finish of the previous file: nothing of this call starts
    const bool compact = want_compact(ro, T);
    PPO_TRY(rollouts_reserve(ro, T, compact));
    const int64_t N = env->N;
    const size_t srow = (size_t)N * env->H * env->F, crow = (size_t)N * 2 * env->V;
    if (compact) PPO_TRY(env->obs_tmp.alloc(srow));           // per-step launches: the observation of one step only
    if (record_probs) PPO_TRY(ro->full_probs.alloc((size_t)T * N * env->A));
    // an env left terminal by a previous call starts a fresh episode (reset! before each episode)
    PPO_TRY(launch_env_reset(env, 1));
    // One launch for the whole rollout (every wave walks its envs through all T steps: k_policy_fwd's FwdMode::Persistent).  Default: on
    // for Q = 8, where the env update is wavefront-parallel (312.7 vs 314.6 ms per bench iteration, same box); off for
    // Q = 32, whose update still runs on one lane.  ppo_set_rollout_persistent / PPO_ROLLOUT_PERSISTENT=0|1 override.
    // With a disk sink attached the rollout is a CHAIN of such launches, a few steps each: the finished steps of launch k
    // are copied device -> pinned host on the copy stream while launch k + 1 runs.
    const int32_t persistent = ppo_knobs().rollout_persistent;
    const bool persistent_ok = persistent == 1 || (persistent < 0 && env->Q == 8);
    int32_t ps = PPO_ERR_UNSUPPORTED;
    PPO_TRY(disk_sink_begin(ro, T));
    if (persistent_ok && !ro->sink) ps = launch_policy_rollout_persistent(pol, env, ro, T, record_probs);
    else if (persistent_ok) {
        const int64_t chunk = disk_sink_chunk(ro);                         // half the ring in flight (at most 8 steps), the rest draining
        for (int64_t t0 = 0; t0 < T; t0 += chunk) {
            const int64_t tc = std::min(chunk, T - t0);
            ps = launch_policy_rollout_persistent(pol, env, ro, tc, record_probs, t0);
            if (ps == PPO_ERR_UNSUPPORTED && t0 > 0) {
                // the per-step fallback restarts at t = 0, but the envs have advanced t0 steps and their records are
                // already enqueued to the sink: a shape that stops being covered mid-chain is a hard error
                ppo_set_error("collect_rollouts!: the one-launch rollout became unavailable in the middle of a streamed collection");
                return PPO_ERR_UNSUPPORTED;
            }
            if (ps != PPO_OK) break;                                       // t0 == 0: shape not covered -> per-step launches
            for (int64_t t = t0; t < t0 + tc; ++t) PPO_TRY(disk_sink_step(ro, t));
        }
    }
    if (ps != PPO_OK && ps != PPO_ERR_UNSUPPORTED) return ps;
    if (ps == PPO_ERR_UNSUPPORTED) {
    for (int64_t t = 0; t < T; ++t) {
        int8_t* st = compact ? env->obs_tmp.p : ro->states.p + (size_t)t * srow;
        uint32_t* am = ro->active.p + (size_t)t * N;
        PPO_TRY(launch_env_observe(env, st, am));                                               // state(env)
        if (compact) PPO_TRY(launch_env_snapshot(env, ro->cstate.p + (size_t)t * crow));       // what is kept of it
        PPO_TRY(launch_policy_rollout(pol, env, st, am, ro->actions.p + t * N, ro->p_sel.p + t * N,
                                      record_probs ? ro->full_probs.p + (size_t)t * N * env->A : nullptr));
        PPO_TRY(launch_env_step(env, ro->actions.p + t * N, ro->rewards.p + t * N, ro->done.p + t * N, nullptr, 1, 0));
        PPO_TRY(disk_sink_step(ro, t));                 // out-of-core store: async D2H of step t on the copy stream
    }
    }
    rollouts_filled(ro, T);
    if (record_probs) ro->probs_T = T;
    PPO_TRY(set_index_all(ro));
    // compute_state_value!: returns overwrite the rewards column (src/rollout_buffer.jl:55-64)
    PPO_TRY(launch_returns_tn(ro->rewards.p, ro->done.p, ro->returns.p, T, N, discount, discount_is_f32));
    PPO_TRY(disk_sink_finish(ro));
    return ppo_env_check_errors(env, nullptr);
}

#define RO_GETTER(name, member, type, per)                                                     \
    int32_t name(ppo_rollouts_t ro, type* out) {                                               \
        ARG_CHECK(ro && out, #name ": null");                                                  \
        return d2h(out, ro->member.p, (size_t)ro->T * ro->N * (per));                          \
    }
RO_GETTER(ppo_rollouts_get_actions, actions, int32_t, 1)
RO_GETTER(ppo_rollouts_get_probs, p_sel, float, 1)
RO_GETTER(ppo_rollouts_get_returns, returns, float, 1)
RO_GETTER(ppo_rollouts_get_raw_rewards, rewards, float, 1)
RO_GETTER(ppo_rollouts_get_terminal, done, uint8_t, 1)
RO_GETTER(ppo_rollouts_get_valid, valid, uint8_t, 1)

int32_t ppo_rollouts_get_states(ppo_rollouts_t ro, int8_t* states, uint32_t* active) {
    ARG_CHECK(ro, "null");
    if (states && !ro->compact) PPO_TRY(d2h(states, ro->states.p, (size_t)ro->T * ro->N * ro->H * ro->F));
    if (states && ro->compact) {       // compact form: the observations are re-derived on the device, <= 256 MiB at a time
        const size_t per = (size_t)ro->H * ro->F, total = (size_t)ro->T * ro->N;
        const size_t chunk = std::max<size_t>(1, std::min(total, ((size_t)256 << 20) / per));
        PPO_TRY(ro->expand_tmp.alloc(chunk * per));
        for (size_t o = 0; o < total; o += chunk) {
            const size_t c = std::min(chunk, total - o);
            PPO_TRY(launch_expand_states(ro->cstate.p + o * 2 * ro->V, ro->active.p + o, ro->tmpl.p, (int64_t)c, ro->V / 4, ro->expand_tmp.p));
            PPO_TRY(d2h(states + o * per, ro->expand_tmp.p, c * per));
        }
    }
    if (active) PPO_TRY(d2h(active, ro->active.p, (size_t)ro->T * ro->N));
    return PPO_OK;
}
int32_t ppo_rollouts_get_full_probs(ppo_rollouts_t ro, float* probs) {
    ARG_CHECK(ro && probs, "null");
    ARG_CHECK(ro->full_probs.p && ro->full_probs.n >= (size_t)ro->T * ro->N * ro->A, "full probabilities were not recorded");
    return d2h(probs, ro->full_probs.p, (size_t)ro->T * ro->N * ro->A);
}
int32_t ppo_rollouts_get_index(ppo_rollouts_t ro, int64_t* idx) {
    ARG_CHECK(ro && idx, "null");
    std::vector<int32_t> tmp((size_t)ro->len);
    PPO_TRY(d2h(tmp.data(), ro->index.p, tmp.size()));
    for (size_t i = 0; i < tmp.size(); ++i) idx[i] = tmp[i];
    return PPO_OK;
}

int32_t ppo_rollouts_set(ppo_rollouts_t ro, int64_t T, const int8_t* states, const uint32_t* active,
                         const int32_t* actions0, const float* p_sel, const float* returns, const uint8_t* terminal) {
    ARG_CHECK(ro && T >= 1 && states && active && actions0 && p_sel && returns, "rollouts_set: bad argument");
    PPO_TRY(rollouts_reserve(ro, T, false));                  // host-supplied observations: always the expanded form
    const size_t n = (size_t)T * ro->N;
    PPO_TRY(h2d(ro->states.p, states, n * ro->H * ro->F)); PPO_TRY(h2d(ro->active.p, active, n));
    PPO_TRY(h2d(ro->actions.p, actions0, n)); PPO_TRY(h2d(ro->p_sel.p, p_sel, n)); PPO_TRY(h2d(ro->returns.p, returns, n));
    PPO_TRY(h2d(ro->rewards.p, returns, n));
    if (terminal) PPO_TRY(h2d(ro->done.p, terminal, n));
    rollouts_filled(ro, T);
    return set_index_all(ro);
}

// batch_advantage plugin as GAE(gamma, lambda): the state values come from the host (the reference has no value head;
// a user's critic supplies them), the scan runs on the device over the buffer's raw rewards / terminal flags.
int32_t ppo_rollouts_compute_gae(ppo_rollouts_t ro, const float* values, double gamma, double lambda, float* adv_out,
                                 float* lambda_returns_out) {
    ARG_CHECK(ro && values, "compute_gae: null argument");
    ARG_CHECK(ro->T >= 1, "compute_gae: empty rollout buffer");
    const size_t n = (size_t)ro->T * ro->N;
    PPO_TRY(ro->values.alloc(n + ro->N)); PPO_TRY(ro->adv.alloc((size_t)ro->capT * ro->N)); PPO_TRY(ro->lam_ret.alloc((size_t)ro->capT * ro->N));
    PPO_TRY(h2d(ro->values.p, values, n + ro->N));
    PPO_TRY(launch_gae_tn(ro->rewards.p, ro->done.p, ro->values.p, ro->adv.p, ro->lam_ret.p, ro->T, ro->N, gamma, lambda));
    ro->adv_T = ro->T; ro->values_T = ro->T;
    if (adv_out) PPO_TRY(d2h(adv_out, ro->adv.p, n));
    if (lambda_returns_out) PPO_TRY(d2h(lambda_returns_out, ro->lam_ret.p, n));
    return PPO_OK;
}

// the same with a host-supplied bootstrap column [T][N] (ppo_gae_boot_tn): any buffer, any env
int32_t ppo_rollouts_compute_gae_boot(ppo_rollouts_t ro, const float* values, const float* boot, double gamma, double lambda,
                                      float* adv_out, float* lambda_returns_out) {
    ARG_CHECK(ro && values && boot, "compute_gae_boot: null argument");
    ARG_CHECK(ro->T >= 1, "compute_gae_boot: empty rollout buffer");
    const size_t n = (size_t)ro->T * ro->N;
    PPO_TRY(ro->values.alloc(n + ro->N)); PPO_TRY(ro->adv.alloc((size_t)ro->capT * ro->N)); PPO_TRY(ro->lam_ret.alloc((size_t)ro->capT * ro->N));
    PPO_TRY(ro->boot.alloc((size_t)ro->capT * ro->N));
    PPO_TRY(h2d(ro->values.p, values, n + ro->N)); PPO_TRY(h2d(ro->boot.p, boot, n));
    PPO_TRY(launch_gae_boot_tn(ro->rewards.p, ro->done.p, ro->values.p, ro->boot.p, ro->adv.p, ro->lam_ret.p, ro->T, ro->N, gamma, lambda));
    ro->adv_T = ro->T; ro->values_T = ro->T; ro->boot_T = ro->T;
    if (adv_out) PPO_TRY(d2h(adv_out, ro->adv.p, n));
    if (lambda_returns_out) PPO_TRY(d2h(lambda_returns_out, ro->lam_ret.p, n));
    HIP_TRY(hipStreamSynchronize(g_stream));
    return PPO_OK;
}

int32_t ppo_rollouts_get_boot(ppo_rollouts_t ro, float* boot_out) {
    ARG_CHECK(ro && boot_out, "get_boot: null argument");
    ARG_CHECK(ro->boot.p && ro->boot_T == ro->T && ro->T >= 1, "get_boot: needs ppo_rollouts_compute_gae_boot or ppo_rollouts_compute_gae_critic_boot on these rollouts first");
    return d2h(boot_out, ro->boot.p, (size_t)ro->T * ro->N);
}

}  // extern "C"
