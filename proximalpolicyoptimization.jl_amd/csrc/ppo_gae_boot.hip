// ppo_gae_boot.hip -- time-limit truncations of a rollout buffer and the states they cut the episodes in.
//
// The built-in env ends an episode at its optimum (a real terminal) or after max_actions steps (a time limit) and resets
// itself inside the rollout kernels, so the state an episode was cut in is not stored.  It does not have to be: the env is
// deterministic integer dynamics, so the step is replayed here from what the buffer holds -- the stored state (the env
// snapshot of a compact buffer; in an expanded one, feature 0 / 36 of observation row v is score[v] / degree[v] whenever
// quad v >> 2 is active, since env_template(Q, h, 0) == h, and an inactive quad's vertices are 0 / 0 by construction) and
// the stored action, through the one definition of the dynamics (env_step_ref) on a per-thread LDS slot.
//   terminated = (sum |score| == |sum score|) over the active quads of the post-step state;  truncated = !terminated
// Launch order (launch_truncated): flags -> deterministic compaction of the flagged transition ids (ascending t*N + n, no
// order decided by atomics) -> [one 8-byte count to the host] -> post-step snapshots of the K truncated transitions in the
// layout launch_value_predict's compact form takes.  The second launch replays the K steps again rather than parking
// T*N post-step snapshots between the launches: K is about T*N / max_actions and a replay is a few hundred LDS operations.
#include "ppo_env_device.h"

#define GB_THREADS 64

struct BootView {
    const int8_t* states;      // [n][H][F] observation rows (expanded form) or nullptr
    const int8_t* cstate;      // [n][2V] env snapshots (compact form) or nullptr
    const uint32_t* active;    // [n]
    const int32_t* actions;    // [n]
    int32_t F;
};

// Replay transition i on this thread's LDS slot; returns truncated (1) / terminated (0) and leaves the post-step state there.
// The slots are thread-private: program order and the in-order LDS suffice, no barrier.
template <int Q>
__device__ __forceinline__ int boot_replay(const BootView& b, int64_t i, const EnvRefLds& r) {
    constexpr int V = 4 * Q;
    if (b.cstate) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(b.cstate + i * (2 * V));
        for (int d = 0; d < V / 2; ++d) {
            const uint32_t w = src[d];
#pragma unroll
            for (int k = 0; k < 4; ++k) r.sc[4 * d + k] = (int8_t)(w >> (8 * k));     // sc[V] then dg[V], contiguous
        }
    } else {
        const int8_t* rows = b.states + i * (int64_t)V * b.F;                          // H == V rows of F features
        for (int v = 0; v < V; ++v) {
            r.sc[v] = rows[(int64_t)v * b.F];
            r.dg[v] = rows[(int64_t)v * b.F + PPO_TPL];
        }
    }
    *r.active = b.active[i];
    *r.steps = 0; *r.reward = 0.0f; *(PPO_LDS uint32_t*)r.done = 0u; *r.episode = 0u; *r.tick = 0u;
    EnvConst c;
    c.Q = Q; c.V = V; c.max_actions = 0x7fffffff; c.no_action_reward = 0.0f; c.k0 = 0u; c.k1 = 0u;
    float rew; uint8_t dn;
    (void)env_step_ref(c, r, b.actions[i], rew, dn);
    const uint32_t act = *r.active;
    const int tot = env_total_abs(r.sc, act, Q), sum = env_total_sum(r.sc, act, Q);
    return tot == (sum < 0 ? -sum : sum) ? 0 : 1;
}

template <int Q>
__device__ __forceinline__ EnvRefLds boot_slot(PPO_LDS char* bytes, PPO_LDS uint32_t* words) {
    constexpr int SLOT = 8 * Q + 4;              // 2V state bytes + one pad dword: an odd dword stride between the threads
    EnvRefLds r;
    r.sc = (PPO_LDS int8_t*)(bytes + threadIdx.x * SLOT); r.dg = r.sc + 4 * Q;
    PPO_LDS uint32_t* w = words + threadIdx.x;
    r.active = w; r.steps = (PPO_LDS int32_t*)(w + GB_THREADS); r.reward = (PPO_LDS float*)(w + 2 * GB_THREADS);
    r.done = (PPO_LDS uint8_t*)(w + 3 * GB_THREADS); r.episode = w + 4 * GB_THREADS; r.tick = w + 5 * GB_THREADS;
    return r;
}

// truncated[i] for every transition: 0 unless done && valid, then the replay's verdict
template <int Q>
__global__ __launch_bounds__(GB_THREADS) void k_boot_flags(BootView b, const uint8_t* __restrict__ done,
                                                           const uint8_t* __restrict__ valid, int64_t n,
                                                           uint8_t* __restrict__ truncated) {
    __shared__ __attribute__((aligned(4))) char sBytes[GB_THREADS * (8 * Q + 4)];
    __shared__ uint32_t sWords[6 * GB_THREADS];
    const int64_t i = (int64_t)blockIdx.x * GB_THREADS + threadIdx.x;
    if (i >= n) return;
    int tr = 0;
    if (done[i] && valid[i]) tr = boot_replay<Q>(b, i, boot_slot<Q>((PPO_LDS char*)sBytes, (PPO_LDS uint32_t*)sWords));
    truncated[i] = (uint8_t)tr;
}

// post-step snapshot (score[V] then degree[V]) and active word of truncated transition ids[k], k < K
template <int Q>
__global__ __launch_bounds__(GB_THREADS) void k_boot_states(BootView b, const int32_t* __restrict__ ids, int64_t K,
                                                            int8_t* __restrict__ cstate_out, uint32_t* __restrict__ active_out) {
    __shared__ __attribute__((aligned(4))) char sBytes[GB_THREADS * (8 * Q + 4)];
    __shared__ uint32_t sWords[6 * GB_THREADS];
    const int64_t k = (int64_t)blockIdx.x * GB_THREADS + threadIdx.x;
    if (k >= K) return;
    const EnvRefLds r = boot_slot<Q>((PPO_LDS char*)sBytes, (PPO_LDS uint32_t*)sWords);
    (void)boot_replay<Q>(b, (int64_t)ids[k], r);
    uint32_t* dst = reinterpret_cast<uint32_t*>(cstate_out + k * (8 * Q));
    for (int d = 0; d < 2 * Q; ++d) {
        uint32_t w = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) w |= ((uint32_t)(uint8_t)r.sc[4 * d + j]) << (8 * j);
        dst[d] = w;
    }
    active_out[k] = *r.active;
}

// ---- deterministic compaction of the set flags' positions, ascending: per-block counts, one-block exclusive scan of the
// counts (+ the total), scatter.  A block covers CP_ITEMS consecutive chunks of 256 flags.
#define CP_ITEMS 4
#define CP_BLOCK (256 * CP_ITEMS)

// flags set among the block's threads: the count in every thread, this thread's rank among them in `rank`
__device__ __forceinline__ int block_rank_256(bool f, int* sWave, int& rank) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long m = __ballot(f);
    const int below = __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();                                         // sWave is reused by the caller's next chunk
    if (lane == 0) sWave[w] = __popcll(m);
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { const int c = sWave[j]; if (j < w) base += c; total += c; }
    rank = base + below;
    return total;
}

__global__ __launch_bounds__(256) void k_flag_count(const uint8_t* __restrict__ flags, int64_t n, int32_t* __restrict__ block_counts) {
    __shared__ int sWave[4];
    int total = 0, rank;
    for (int j = 0; j < CP_ITEMS; ++j) {
        const int64_t i = (int64_t)blockIdx.x * CP_BLOCK + j * 256 + threadIdx.x;
        total += block_rank_256(i < n && flags[i] != 0, sWave, rank);
    }
    if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

// in place: counts -> exclusive offsets; count_out = the total.  One block; chunks of 256 counts with a running carry
__global__ __launch_bounds__(256) void k_scan_counts(int32_t* __restrict__ counts, int64_t nb, int64_t* __restrict__ count_out) {
    __shared__ int s[256];
    __shared__ int sCarry;
    if (threadIdx.x == 0) sCarry = 0;
    __syncthreads();
    for (int64_t c0 = 0; c0 < nb; c0 += 256) {
        const int64_t i = c0 + threadIdx.x;
        const int x = i < nb ? counts[i] : 0;
        s[threadIdx.x] = x;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {            // inclusive scan of the chunk
            const int y = (int)threadIdx.x >= off ? s[threadIdx.x - off] : 0;
            __syncthreads();
            s[threadIdx.x] += y;
            __syncthreads();
        }
        const int carry = sCarry;
        if (i < nb) counts[i] = carry + s[threadIdx.x] - x;
        __syncthreads();
        if (threadIdx.x == 255) sCarry = carry + s[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) *count_out = (int64_t)sCarry;
}

__global__ __launch_bounds__(256) void k_flag_scatter(const uint8_t* __restrict__ flags, int64_t n,
                                                      const int32_t* __restrict__ block_offsets, int32_t* __restrict__ ids) {
    __shared__ int sWave[4];
    int at = block_offsets[blockIdx.x], rank;
    for (int j = 0; j < CP_ITEMS; ++j) {
        const int64_t i = (int64_t)blockIdx.x * CP_BLOCK + j * 256 + threadIdx.x;
        const bool f = i < n && flags[i] != 0;
        const int total = block_rank_256(f, sWave, rank);
        if (f) ids[at + rank] = (int32_t)i;                  // at + rank < the total of set flags <= n: inside ids[n]
        at += total;
    }
}

static int64_t compact_blocks(int64_t n) { return (n + CP_BLOCK - 1) / CP_BLOCK; }

// ids[0 .. K) = the positions of the non-zero flags[0 .. n), ascending; *total = K.  counts: compact_blocks(n) words of
// workspace; ids: room for n
static int32_t launch_compact_flags(const uint8_t* flags, int64_t n, int32_t* counts, int32_t* ids, int64_t* total) {
    const int64_t nb = compact_blocks(n);
    hipLaunchKernelGGL(k_flag_count, dim3((unsigned)nb), dim3(256), 0, ppo_stream(), flags, n, counts);
    hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(256), 0, ppo_stream(), counts, nb, total);
    hipLaunchKernelGGL(k_flag_scatter, dim3((unsigned)nb), dim3(256), 0, ppo_stream(), flags, n, counts, ids);
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

// boot[ids[k]] = vals[k] over a column the caller zeroed
__global__ void k_boot_scatter(const int32_t* __restrict__ ids, const float* __restrict__ vals, int64_t K, float* __restrict__ boot) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < K) boot[ids[k]] = vals[k];
}

static BootView view_of(const ppo_rollouts_s* ro) {
    BootView b;
    b.states = ro->compact ? nullptr : ro->states.p; b.cstate = ro->compact ? ro->cstate.p : nullptr;
    b.active = ro->active.p; b.actions = ro->actions.p; b.F = ro->F;
    return b;
}

// ro->truncated [T][N], ro->trunc_ids [K] ascending and *K_out on the host (the one count that crosses).  The caller
// checked: built-in env buffer (V = 32 or 128, F = 72), T >= 1
int32_t launch_truncated(ppo_rollouts_s* ro, int64_t* K_out) {
    const int64_t n = ro->T * ro->N;
    const int64_t nb = compact_blocks(n);
    PPO_TRY(ro->truncated.alloc((size_t)ro->capT * ro->N)); PPO_TRY(ro->trunc_ids.alloc((size_t)ro->capT * ro->N));
    PPO_TRY(ro->trunc_counts.alloc((size_t)nb + 4));         // [nb] block counts, then the 8-byte total (8-byte aligned)
    int64_t* total = reinterpret_cast<int64_t*>(ro->trunc_counts.p + ((nb + 1) & ~(int64_t)1));
    const BootView b = view_of(ro);
    const dim3 g((unsigned)((n + GB_THREADS - 1) / GB_THREADS));
    {
        ProfScope ps("k_boot_flags");
        if (ro->V == 32) hipLaunchKernelGGL(k_boot_flags<8>, g, dim3(GB_THREADS), 0, ppo_stream(), b, ro->done.p, ro->valid.p, n, ro->truncated.p);
        else hipLaunchKernelGGL(k_boot_flags<32>, g, dim3(GB_THREADS), 0, ppo_stream(), b, ro->done.p, ro->valid.p, n, ro->truncated.p);
        HIP_TRY(hipGetLastError());
    }
    PPO_TRY(launch_compact_flags(ro->truncated.p, n, ro->trunc_counts.p, ro->trunc_ids.p, total));
    return d2h(K_out, total, 1);
}

// diagnostic for the tests (not part of include/ppo_hip.h), like ppo_debug_train_ratios: the compaction alone on host flags of
// any length.  ids_out [n]: the ascending positions of the non-zero flags, then -1 (the device buffer is filled with 0xFF
// bytes first, so a write behind the K-th entry shows)
extern "C" int32_t ppo_debug_compact_flags(const uint8_t* flags, int64_t n, int32_t* ids_out, int64_t* K) {
    PPO_TRY(ppo_device_synchronize());
    ARG_CHECK(flags && ids_out && K && n >= 1 && n <= 0x7fffffff, "ppo_debug_compact_flags: null argument or n outside [1, 2^31)");
    const int64_t nb = compact_blocks(n);
    DevBuf<uint8_t> f; DevBuf<int32_t> counts, ids;
    PPO_TRY(f.alloc((size_t)n)); PPO_TRY(ids.alloc((size_t)n)); PPO_TRY(counts.alloc((size_t)nb + 4));
    int64_t* total = reinterpret_cast<int64_t*>(counts.p + ((nb + 1) & ~(int64_t)1));
    PPO_TRY(h2d(f.p, flags, (size_t)n));
    HIP_TRY(hipMemsetAsync(ids.p, 0xFF, (size_t)n * sizeof(int32_t), ppo_stream()));
    PPO_TRY(launch_compact_flags(f.p, n, counts.p, ids.p, total));
    PPO_TRY(d2h(K, total, 1));
    return d2h(ids_out, ids.p, (size_t)n);
}

// post-step snapshots [K][2V] and active words [K] of the transitions launch_truncated listed
int32_t launch_truncated_states(ppo_rollouts_s* ro, int64_t K, int8_t* cstate_out, uint32_t* active_out) {
    if (K <= 0) return PPO_OK;
    ProfScope ps("k_boot_states");
    const BootView b = view_of(ro);
    const dim3 g((unsigned)((K + GB_THREADS - 1) / GB_THREADS));
    if (ro->V == 32) hipLaunchKernelGGL(k_boot_states<8>, g, dim3(GB_THREADS), 0, ppo_stream(), b, ro->trunc_ids.p, K, cstate_out, active_out);
    else hipLaunchKernelGGL(k_boot_states<32>, g, dim3(GB_THREADS), 0, ppo_stream(), b, ro->trunc_ids.p, K, cstate_out, active_out);
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

// boot [T][N]: vals[k] at transition ids[k], exactly 0.0f elsewhere
int32_t launch_boot_scatter(ppo_rollouts_s* ro, const float* vals, int64_t K, float* boot) {
    HIP_TRY(hipMemsetAsync(boot, 0, (size_t)ro->T * ro->N * sizeof(float), ppo_stream()));
    if (K <= 0) return PPO_OK;
    hipLaunchKernelGGL(k_boot_scatter, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, ppo_stream(), ro->trunc_ids.p, vals, K, boot);
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}
