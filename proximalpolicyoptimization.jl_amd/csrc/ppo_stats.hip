// ppo_stats.hip -- what a PPO user reads off an update, reduced on the device (no reference op: the reference reports the
// two losses and the learning rate only):
//   k_ratio_stats    over the probability ratios r = p_new(a|s) / p_old(a|s) the loss tail stored (ppo_policy_tail.h):
//                    sum(-log r), sum((r - 1) - log r), count(|r - 1| > eps), n  ->  old_approx_kl, approx_kl, clip_fraction
//   k_value_clip_stats over the changes delta = V - V_old the critic's loss tail stored while a value clip is set:
//                    count(|delta| > c), sum(delta^2), n  ->  clip_fraction, mean_sq_change
//   k_sum_stats      over a column of floats, e.g. the per-state anchor divergences the anchored loss tail stored: sum x, n
//   k_value_moments  over the valid transitions of a rollout buffer: the five shifted sums behind the critic's explained
//                    variance 1 - Var(t - V) / Var(t)
// All in fp64 with a FIXED summation order that depends on the element count only: every thread walks its 16-byte groups
// in ascending order, a butterfly over the wave, the block's waves in order, the blocks in order (second launch, one wave:
// lane l takes blocks l, l + 64, ... in order, then the butterfly).  No float atomics, so a second run repeats the first
// bit for bit.  Bandwidth-trivial (4 bytes per transition), hence simple rather than tuned.
#include "ppo_internal.h"

#define STATS_THREADS 256
#define STATS_MAX_BLOCKS 1024
#define STATS_PER_BLOCK 4096      // elements per block until STATS_MAX_BLOCKS is reached
#define STATS_RESULT 8            // doubles in front of the block partials that hold the results
#define STATS_MAX_K 5

size_t stats_part_doubles() { return STATS_RESULT + (size_t)STATS_MAX_BLOCKS * STATS_MAX_K; }

static int stats_blocks(int64_t n) {
    const int64_t b = (n + STATS_PER_BLOCK - 1) / STATS_PER_BLOCK;
    return (int)(b < 1 ? 1 : (b > STATS_MAX_BLOCKS ? STATS_MAX_BLOCKS : b));
}

__device__ __forceinline__ double wave64_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off);
    return v;
}

// acc of every thread of the block -> row[K]: wave butterflies, then the waves in order
template <int K>
__device__ __forceinline__ void block_sum_store(double (&acc)[K], double* __restrict__ row) {
    __shared__ double sw[STATS_THREADS / 64][K];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double s = wave64_sum(acc[k]);
        if (lane == 0) sw[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        double s = sw[0][threadIdx.x];
        for (int w = 1; w < STATS_THREADS / 64; ++w) s = s + sw[w][threadIdx.x];
        row[threadIdx.x] = s;
    }
}

// one wave: out[k] = partials[0][k] + ... in the fixed order above
template <int K>
__global__ __launch_bounds__(64) void k_stats_finish(const double* __restrict__ partials, int blocks, double* __restrict__ out) {
    const int lane = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double s = 0.0;
        for (int b = lane; b < blocks; b += 64) s = s + partials[(size_t)b * K + k];
        s = wave64_sum(s);
        if (lane == 0) out[k] = s;
    }
}

__device__ __forceinline__ void ratio_term(const float r, const double eps, double (&acc)[4]) {
    const double rd = (double)r;
    const double lg = log(rd);
    acc[0] = acc[0] + (-lg);
    acc[1] = acc[1] + ((rd - 1.0) - lg);
    acc[2] = acc[2] + (fabs(rd - 1.0) > eps ? 1.0 : 0.0);
    acc[3] = acc[3] + 1.0;
}

// r: 16-byte aligned
__global__ __launch_bounds__(STATS_THREADS) void k_ratio_stats(const float* __restrict__ r, int64_t n, double eps,
                                                               double* __restrict__ partials) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const int64_t n4 = n >> 2, total = (int64_t)gridDim.x * STATS_THREADS;
    const int64_t g = (int64_t)blockIdx.x * STATS_THREADS + threadIdx.x;
    for (int64_t q = g; q < n4; q += total) {
        const float4 v = reinterpret_cast<const float4*>(r)[q];
        ratio_term(v.x, eps, acc); ratio_term(v.y, eps, acc); ratio_term(v.z, eps, acc); ratio_term(v.w, eps, acc);
    }
    const int64_t i = (n4 << 2) + g;                       // the n & 3 elements behind the last whole group
    if (i < n) ratio_term(r[i], eps, acc);
    block_sum_store<4>(acc, partials + (size_t)blockIdx.x * 4);
}

// c: the fp32 clip range the tail compared with, so that the count is the tail's own `inside` decision
__device__ __forceinline__ void vclip_term(const float dl, const float c, double (&acc)[3]) {
    const double dd = (double)dl;
    acc[0] = acc[0] + (fabsf(dl) > c ? 1.0 : 0.0);
    acc[1] = acc[1] + dd * dd;
    acc[2] = acc[2] + 1.0;
}

// delta: 16-byte aligned
__global__ __launch_bounds__(STATS_THREADS) void k_value_clip_stats(const float* __restrict__ delta, int64_t n, float c,
                                                                    double* __restrict__ partials) {
    double acc[3] = {0.0, 0.0, 0.0};
    const int64_t n4 = n >> 2, total = (int64_t)gridDim.x * STATS_THREADS;
    const int64_t g = (int64_t)blockIdx.x * STATS_THREADS + threadIdx.x;
    for (int64_t q = g; q < n4; q += total) {
        const float4 v = reinterpret_cast<const float4*>(delta)[q];
        vclip_term(v.x, c, acc); vclip_term(v.y, c, acc); vclip_term(v.z, c, acc); vclip_term(v.w, c, acc);
    }
    const int64_t i = (n4 << 2) + g;                       // the n & 3 elements behind the last whole group
    if (i < n) vclip_term(delta[i], c, acc);
    block_sum_store<3>(acc, partials + (size_t)blockIdx.x * 3);
}

// x: 16-byte aligned
__global__ __launch_bounds__(STATS_THREADS) void k_sum_stats(const float* __restrict__ x, int64_t n, double* __restrict__ partials) {
    double acc[2] = {0.0, 0.0};
    const int64_t n4 = n >> 2, total = (int64_t)gridDim.x * STATS_THREADS;
    const int64_t g = (int64_t)blockIdx.x * STATS_THREADS + threadIdx.x;
    for (int64_t q = g; q < n4; q += total) {
        const float4 v = reinterpret_cast<const float4*>(x)[q];
        acc[0] = (((acc[0] + (double)v.x) + (double)v.y) + (double)v.z) + (double)v.w;
        acc[1] = acc[1] + 4.0;
    }
    const int64_t i = (n4 << 2) + g;                       // the n & 3 elements behind the last whole group
    if (i < n) { acc[0] = acc[0] + (double)x[i]; acc[1] = acc[1] + 1.0; }
    block_sum_store<2>(acc, partials + (size_t)blockIdx.x * 2);
}

__device__ __forceinline__ void moment_term(const float t, const float v, const uint8_t on, const double st, const double sd,
                                            double (&acc)[5]) {
    if (!on) return;
    const double x = (double)t - st;
    const double y = ((double)t - (double)v) - sd;
    acc[0] = acc[0] + 1.0;
    acc[1] = acc[1] + x; acc[2] = acc[2] + x * x;
    acc[3] = acc[3] + y; acc[4] = acc[4] + y * y;
}

// t, v: 16-byte aligned; valid: 4-byte aligned; first_id[0] in [0, n)
__global__ __launch_bounds__(STATS_THREADS) void k_value_moments(const float* __restrict__ t, const float* __restrict__ v,
                                                                 const uint8_t* __restrict__ valid,
                                                                 const int32_t* __restrict__ first_id, int64_t n,
                                                                 double* __restrict__ partials) {
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const int64_t i0 = first_id[0];
    const double st = (double)t[i0], sd = (double)t[i0] - (double)v[i0];
    const int64_t n4 = n >> 2, total = (int64_t)gridDim.x * STATS_THREADS;
    const int64_t g = (int64_t)blockIdx.x * STATS_THREADS + threadIdx.x;
    for (int64_t q = g; q < n4; q += total) {
        const float4 tv = reinterpret_cast<const float4*>(t)[q];
        const float4 vv = reinterpret_cast<const float4*>(v)[q];
        const uchar4 m = reinterpret_cast<const uchar4*>(valid)[q];
        moment_term(tv.x, vv.x, m.x, st, sd, acc); moment_term(tv.y, vv.y, m.y, st, sd, acc);
        moment_term(tv.z, vv.z, m.z, st, sd, acc); moment_term(tv.w, vv.w, m.w, st, sd, acc);
    }
    const int64_t i = (n4 << 2) + g;
    if (i < n) moment_term(t[i], v[i], valid[i], st, sd, acc);
    block_sum_store<5>(acc, partials + (size_t)blockIdx.x * 5);
}

int32_t launch_ratio_stats(const float* ratio, int64_t n, double eps, double* part) {
    const int blocks = stats_blocks(n);
    ProfScope ps("k_ratio_stats");
    hipLaunchKernelGGL(k_ratio_stats, dim3(blocks), dim3(STATS_THREADS), 0, ppo_stream(), ratio, n, eps, part + STATS_RESULT);
    hipLaunchKernelGGL(k_stats_finish<4>, dim3(1), dim3(64), 0, ppo_stream(), part + STATS_RESULT, blocks, part);
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

int32_t launch_value_clip_stats(const float* delta, int64_t n, float c, double* part) {
    const int blocks = stats_blocks(n);
    ProfScope ps("k_value_clip_stats");
    hipLaunchKernelGGL(k_value_clip_stats, dim3(blocks), dim3(STATS_THREADS), 0, ppo_stream(), delta, n, c, part + STATS_RESULT);
    hipLaunchKernelGGL(k_stats_finish<3>, dim3(1), dim3(64), 0, ppo_stream(), part + STATS_RESULT, blocks, part);
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

int32_t launch_sum_stats(const float* col, int64_t n, double* part) {
    const int blocks = stats_blocks(n);
    ProfScope ps("k_sum_stats");
    hipLaunchKernelGGL(k_sum_stats, dim3(blocks), dim3(STATS_THREADS), 0, ppo_stream(), col, n, part + STATS_RESULT);
    hipLaunchKernelGGL(k_stats_finish<2>, dim3(1), dim3(64), 0, ppo_stream(), part + STATS_RESULT, blocks, part);
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

int32_t launch_value_moments(const float* target, const float* values, const uint8_t* valid, const int32_t* first_id,
                             int64_t n, double* part) {
    const int blocks = stats_blocks(n);
    ProfScope ps("k_value_moments");
    hipLaunchKernelGGL(k_value_moments, dim3(blocks), dim3(STATS_THREADS), 0, ppo_stream(), target, values, valid, first_id, n,
                       part + STATS_RESULT);
    hipLaunchKernelGGL(k_stats_finish<5>, dim3(1), dim3(64), 0, ppo_stream(), part + STATS_RESULT, blocks, part);
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

// ---- diagnostics for the tests (not part of include/ppo_hip.h), like ppo_debug_train_ratios: the three reductions on host
// columns of any length, through the launch functions above and a workspace of the size the product path allocates
static int32_t debug_stats_begin(const char* who, const void* a, const void* out, int64_t n, DevBuf<double>& part) {
    PPO_TRY(ppo_device_synchronize());
    if (!a || !out || n < 1) { ppo_set_error(std::string("AssertionError: ") + who + ": null argument or n < 1"); return PPO_ERR_ARG; }
    return part.alloc(stats_part_doubles());
}

extern "C" int32_t ppo_debug_ratio_stats(const float* r, int64_t n, double eps, double* out4) {
    DevBuf<double> part; DevBuf<float> col;
    PPO_TRY(debug_stats_begin("ppo_debug_ratio_stats", r, out4, n, part));
    PPO_TRY(col.alloc((size_t)n)); PPO_TRY(h2d(col.p, r, (size_t)n));
    PPO_TRY(launch_ratio_stats(col.p, n, eps, part.p));
    return d2h(out4, part.p, 4);
}

extern "C" int32_t ppo_debug_value_clip_stats(const float* delta, int64_t n, float c, double* out3) {
    DevBuf<double> part; DevBuf<float> col;
    PPO_TRY(debug_stats_begin("ppo_debug_value_clip_stats", delta, out3, n, part));
    PPO_TRY(col.alloc((size_t)n)); PPO_TRY(h2d(col.p, delta, (size_t)n));
    PPO_TRY(launch_value_clip_stats(col.p, n, c, part.p));
    return d2h(out3, part.p, 3);
}

extern "C" int32_t ppo_debug_sum_stats(const float* x, int64_t n, double* out2) {
    DevBuf<double> part; DevBuf<float> col;
    PPO_TRY(debug_stats_begin("ppo_debug_sum_stats", x, out2, n, part));
    PPO_TRY(col.alloc((size_t)n)); PPO_TRY(h2d(col.p, x, (size_t)n));
    PPO_TRY(launch_sum_stats(col.p, n, part.p));
    return d2h(out2, part.p, 2);
}

extern "C" int32_t ppo_debug_value_moments(const float* t, const float* v, const uint8_t* valid, int64_t first_id, int64_t n,
                                           double* out5) {
    DevBuf<double> part; DevBuf<float> tc, vc; DevBuf<uint8_t> on; DevBuf<int32_t> first;
    PPO_TRY(debug_stats_begin("ppo_debug_value_moments", t, out5, n, part));
    ARG_CHECK(v && valid && first_id >= 0 && first_id < n && n <= 0x7fffffff, "ppo_debug_value_moments: null argument or first_id outside [0, n)");
    PPO_TRY(tc.alloc((size_t)n)); PPO_TRY(vc.alloc((size_t)n)); PPO_TRY(on.alloc((size_t)n)); PPO_TRY(first.alloc(1));
    const int32_t i0 = (int32_t)first_id;
    PPO_TRY(h2d(tc.p, t, (size_t)n)); PPO_TRY(h2d(vc.p, v, (size_t)n)); PPO_TRY(h2d(on.p, valid, (size_t)n)); PPO_TRY(h2d(first.p, &i0, 1));
    PPO_TRY(launch_value_moments(tc.p, vc.p, on.p, first.p, n, part.p));
    return d2h(out5, part.p, 5);
}
