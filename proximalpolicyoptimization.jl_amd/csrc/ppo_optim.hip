// ppo_optim.hip -- gradient slab reduction, K12 Adam (Flux legacy Adam + Flux.update!,
// src/train.jl:81; semantics SURVEY.md Appendix A) and the re-packing of the updated parameters
// into the MFMA A-operand fragment orders used by the forward/backward kernels; Flux.Optimiser chains (ExpDecay, Descent,
// Momentum, Nesterov, RMSProp, Adam, ClipValue, ClipNorm, WeightDecay, InvDecay; include/ppo_hip.h) through the same
// reduction and re-pack.
#include "ppo_internal.h"
#include "ppo_device.h"
#include <algorithm>
#include <cstring>
#include <type_traits>

// flat Flux-order parameter vector of Policy(F, HID, NL, 4) (test/policy.jl:9-19): W1, b1, then the NL - 1 hidden->hidden
// layers (W, b) back to back -- layer l at offW2 + l * (HID*HID + HID) -- then W3, b3
struct ParamLayout {
    int F, HID, NT, FP, NI, NL2;                // NL2 = hidden->hidden layers (num_hidden_layers - 1)
    int64_t offW1, offb1, offW2, offW3, offb3, np;
};

static ParamLayout layout_of(const ppo_policy_s* p) {
    ParamLayout L;
    L.F = p->F; L.HID = p->HID; L.NT = p->HID / 32; L.FP = ((p->F + 31) / 32) * 32; L.NI = L.FP / 32; L.NL2 = p->L - 1;
    L.offW1 = 0; L.offb1 = (int64_t)p->HID * p->F; L.offW2 = L.offb1 + p->HID;
    L.offW3 = L.offW2 + (int64_t)L.NL2 * ((int64_t)p->HID * p->HID + p->HID);
    L.offb3 = L.offW3 + (int64_t)PPO_OUT * p->HID; L.np = L.offb3 + PPO_OUT;
    return L;
}

// ---------------------------------------------------------------- slab reduce
// One thread per slab element (coalesced reads across slabs); fixed summation order.
__device__ void loss_reduce_block(const double* __restrict__ terms, int64_t B, double inv_Bg, double entropy_weight,
                                  float* __restrict__ grad_tail);

struct PackPtrs {
    float* w1p; float* w2p; float* w2tp; float* b1p; float* b2p; float* w3p; float* b3;
    // bf16 compute mode (null in fp32 mode): A-operand fragments of v_mfma_f32_32x32x16_bf16 (ppo_policy_bf16.hip)
    uint16_t* w1b; uint16_t* w2b; uint16_t* w2tb; uint16_t* w3c; uint16_t* w3tb;
    // split-fp32 backward (null when the policy has none): W2 as three bf16 pieces (ppo_policy_bwd_x6.hip)
    uint16_t* w2x; uint16_t* w1x; uint16_t* w2fx;
};

// Adam fused into the slab reduction (single-rank training: no all-reduce between them): the thread that holds an element's
// gradient sum applies Flux's legacy Adam to that parameter and re-packs it -- one launch and one pass over the gradient less
struct AdamFuse { float* params; float* m; float* v; double eta, beta1, beta2, eps, bp1, bp2; float* hist2; int on; };
__device__ __forceinline__ void pack_one(const ParamLayout& L, const PackPtrs& P, int64_t i, float x);
__device__ __forceinline__ void adam_one(const AdamFuse& A, const ParamLayout& L, const PackPtrs& P, int64_t i, float g);

// Flux.Optimiser chain of 1..4 members (ppo_optimiser_create; arithmetic in include/ppo_hip.h and DESIGN.md section 3):
// passed by value, so the member loop below is unrolled over four constant slots and every branch is wave-uniform.
// c[j]: the member's float64 scalars for this step -- Adam (eta, beta1, beta2, eps, beta1^t, beta2^t), ExpDecay (eta_n:
// the host advanced its counter and decay), Descent (eta), Momentum / Nesterov (eta, rho), RMSProp (eta, rho, epsilon);
// s0 / s1: its float32 state arrays at the kernels' width (Adam m / v, velocity, acc)
struct ChainFuse {
    float* params; float* hist2; int on; int n;
    int kind[4];
    double c[4][6];
    float* s0[4]; float* s1[4];
};
__device__ __forceinline__ void chain_one(const ChainFuse& C, const ParamLayout& L, const PackPtrs& P, int64_t i, float g);
__device__ __forceinline__ void fuse_one(const AdamFuse& A, const ParamLayout& L, const PackPtrs& P, int64_t i, float g) { adam_one(A, L, P, i, g); }
__device__ __forceinline__ void fuse_one(const ChainFuse& C, const ParamLayout& L, const PackPtrs& P, int64_t i, float g) { chain_one(C, L, P, i, g); }

// A chain with a ClipNorm member at position c updates in two launches, because ClipNorm's per-array norm is a reduction
// across workgroups between the gradient and the update.  Phase 1 (k_grad_reduce<ClipFuse> fused with the slab reduction,
// or k_chain_clip1 behind an all-reduce) applies members [0, c), stores their state and D into dbuf, and writes one
// double-double partial sum of D^2 per 32 consecutive elements it walks (a half-wave: every array starts at a multiple of
// 32 in both the slab order and the Flux order, so a half-wave never straddles two arrays).  Phase 2 (k_clip_apply)
// finishes each array's norm from its slot range in a fixed order, scales D, applies members (c, n) and does x -= D.
// No float atomics: a second run repeats the first bit for bit.
struct ClipFuse {
    float* hist2; int on;
    ChainFuse C;                                // members [0, c): C.n = c
    float* dbuf;                                // [np] D after them, Flux order
    double* part;                               // [slots][2] (hi, lo)
};
__device__ __forceinline__ float chain_delta(const ChainFuse& C, int64_t i, float g);
__device__ __forceinline__ void clip_partial(double* __restrict__ part, size_t e, float d);

__device__ __forceinline__ void fuse_one(const ClipFuse&, const ParamLayout&, const PackPtrs&, int64_t, float) {}   // (phase 1 returns earlier)

// Block = 64 consecutive slab elements x 4 slab groups (wave g sums slabs g, g+4, g+8, ... with 8 loads in flight);
// the four partial sums meet in LDS and are added in a fixed order.  4x the waves of a one-thread-per-element
// layout: the 87 MB slab walk needs the memory-level parallelism (341 blocks of one wave per SIMD did 3.3 TB/s).
// nwg_w slabs carry weight-gradient partials, nwg_s slabs the small-gradient tails (equal for the fused backward).
// Fuse: AdamFuse (k_grad_reduce<AdamFuse>, timed as k_grad_reduce / k_reduce_adam), ChainFuse (timed as k_reduce_chain) or
// ClipFuse (k_reduce_clip)
template <typename Fuse>
__global__ __launch_bounds__(256) void k_grad_reduce(const float* __restrict__ slabs, size_t slab_stride, int nwg_w, int nwg_s, ParamLayout L,
                                                     float* __restrict__ grad, const double* __restrict__ terms, int64_t B,
                                                     double inv_Bg, double entropy_weight, Fuse A, PackPtrs P) {
    if (blockIdx.x == gridDim.x - 1) {          // the extra last block reduces the per-sample loss terms
        loss_reduce_block(terms, B, inv_Bg, entropy_weight, grad + L.np);
        if (A.on && A.hist2 && threadIdx.x == 0) { A.hist2[0] = grad[L.np]; A.hist2[1] = grad[L.np + 1]; }   // per-batch loss history (k_opt_update's job otherwise)
        return;
    }
    __shared__ float part[4][64];
    const int el = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const size_t e = (size_t)blockIdx.x * 64 + el;
    const size_t nW2l = (size_t)L.HID * L.HID, nW2 = (size_t)L.NL2 * nW2l, nW1 = (size_t)L.HID * L.FP;
    const size_t total = nW2 + nW1 + (size_t)L.HID * (1 + L.NL2) + (size_t)L.HID * 4 + 4;
    // fixed summation order: 8 interleaved partial sums per slab group, a fixed tree, then the 4 groups in order
    float ps[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int nwg = (e < nW2 + nW1) ? nwg_w : nwg_s;
    // padding columns of the dW1 block (inputs F .. FP-1: a quarter of its last 32-column tile for F = 72) map to no parameter:
    // their slab values are never read (the split-fp32 backward does not write them either, except the ones column it keeps db1 in)
    bool dead = false;
    if (e >= nW2 && e < nW2 + nW1) {
        const size_t e1 = e - nW2;
        const int it = (int)((e1 >> 10) % L.NI);
        dead = 32 * it + (int)(e1 & 31) >= L.F;
    }
    if (e < total && !dead) {
        int g = grp;
        for (; g + 28 < nwg; g += 32) {
#pragma unroll
            for (int u = 0; u < 8; ++u) ps[u] += slabs[(size_t)(g + 4 * u) * slab_stride + e];
        }
        for (int u = 0; g < nwg; g += 4, ++u) ps[u] += slabs[(size_t)g * slab_stride + e];
    }
    part[grp][el] = ((ps[0] + ps[1]) + (ps[2] + ps[3])) + ((ps[4] + ps[5]) + (ps[6] + ps[7]));
    __syncthreads();
    constexpr bool clip = std::is_same<Fuse, ClipFuse>::value;   // ClipNorm phase 1: every lane of wave 0 joins its half-wave's sum
    if (grp != 0 || (e >= total && !clip)) return;
    const float s = (part[0][el] + part[1][el]) + (part[2][el] + part[3][el]);
    int64_t canon = -1;
    if (e < nW2) {
        const int lay = (int)(e / nW2l);
        const size_t el2 = e - (size_t)lay * nW2l;
        const int lane = (int)(el2 & 63), r = (int)((el2 >> 6) & 15);
        const int tile = (int)(el2 >> 10), kt = tile % L.NT, ft = tile / L.NT;
        const int f = dfeat(ft, r, lane >> 5), k = 32 * kt + (lane & 31);
        canon = L.offW2 + (int64_t)lay * ((int64_t)nW2l + L.HID) + f + (int64_t)L.HID * k;
    } else if (e < nW2 + nW1) {
        const size_t e1 = e - nW2;
        const int lane = (int)(e1 & 63), r = (int)((e1 >> 6) & 15);
        const int tile = (int)(e1 >> 10), it = tile % L.NI, ft = tile / L.NI;
        const int ko = dfeat(ft, r, lane >> 5), i = 32 * it + (lane & 31);
        if (i < L.F) canon = L.offW1 + ko + (int64_t)L.HID * i;
    } else {
        size_t e2 = e - nW2 - nW1;
        if (e2 < (size_t)L.HID) canon = L.offb1 + (int64_t)e2;
        else if ((e2 -= L.HID) < (size_t)L.HID * L.NL2)         // bias of hidden->hidden layer e2 / HID, behind its weights
            canon = L.offW2 + (int64_t)(e2 / L.HID) * ((int64_t)nW2l + L.HID) + (int64_t)nW2l + (int64_t)(e2 % L.HID);
        else if ((e2 -= (size_t)L.HID * L.NL2) < (size_t)L.HID * 4) canon = L.offW3 + (int64_t)(e2 & 3) + 4 * (int64_t)(e2 >> 2);
        else canon = L.offb3 + (int64_t)(e2 - (size_t)L.HID * 4);
    }
    if constexpr (clip) {
        float d = 0.f;                          // beyond the end and in dead columns: adds nothing to any norm
        if (e < total && canon >= 0) {
            grad[canon] = s;
            d = chain_delta(A.C, canon, s);
            A.dbuf[canon] = d;
        }
        clip_partial(A.part, e, d);
        return;
    }
    if (canon >= 0) {
        grad[canon] = s;
        if (A.on) fuse_one(A, L, P, canon, s);
    }
}

// loss scalars: grad[np] = -(sum min)/B_global, grad[np+1] = entropy_weight * -(sum H)/B_global.
// One block of 256 threads, fixed order: 8 interleaved fp64 partial sums per thread (loads in flight), a fixed tree
// per thread, then the LDS tree.
__device__ void loss_reduce_block(const double* __restrict__ terms, int64_t B, double inv_Bg, double entropy_weight,
                                  float* __restrict__ grad_tail) {
    __shared__ double s0[256], s1[256];
    const double2* t2 = reinterpret_cast<const double2*>(terms);
    double a[8] = {0, 0, 0, 0, 0, 0, 0, 0}, b[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t i = threadIdx.x;
    for (; i + 7 * 256 < B; i += 8 * 256) {
#pragma unroll
        for (int u = 0; u < 8; ++u) { const double2 v = t2[i + u * 256]; a[u] += v.x; b[u] += v.y; }
    }
    for (int u = 0; i < B; i += 256, ++u) { const double2 v = t2[i]; a[u] += v.x; b[u] += v.y; }
    s0[threadIdx.x] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    s1[threadIdx.x] = ((b[0] + b[1]) + (b[2] + b[3])) + ((b[4] + b[5]) + (b[6] + b[7]));
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) { s0[threadIdx.x] += s0[threadIdx.x + off]; s1[threadIdx.x] += s1[threadIdx.x + off]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        grad_tail[0] = (float)(-(s0[0] * inv_Bg));
        grad_tail[1] = (float)(entropy_weight * (-(s1[0] * inv_Bg)));
    }
}

// ---------------------------------------------------------------- Adam + pack

__device__ __forceinline__ uint16_t to_bf16(float x) { return __builtin_bit_cast(uint16_t, (__bf16)x); }   // RNE
// x = h + m + l: each piece the RNE bf16 of what the previous ones left (the differences are exact in fp32)
__device__ __forceinline__ void split3_bf16(float x, uint16_t& ph, uint16_t& pm, uint16_t& pl) {
    ph = to_bf16(x);
    const float r1 = x - __uint_as_float((uint32_t)ph << 16);
    pm = to_bf16(r1);
    const float r2 = r1 - __uint_as_float((uint32_t)pm << 16);
    pl = to_bf16(r2);
}
// k-slot of contraction index kk (0..31) inside a 32-wide tile when the other operand is a packed accumulator tile:
// k-step s = kk>>4, lane half hh and element jj such that 16s + 8(jj>>2) + 4hh + (jj&3) == kk
__device__ __forceinline__ void acc_kslot(int kk, int& s, int& hh, int& jj) {
    const int q = kk & 15;
    s = kk >> 4; hh = (q >> 2) & 1; jj = 4 * (q >> 3) + (q & 3);
}

__device__ __forceinline__ void pack_one(const ParamLayout& L, const PackPtrs& P, int64_t i, float x) {
    const int HID = L.HID, F = L.F, NT = L.NT;
    if (i < L.offb1) {                                   // W1[io][k]  (layer-1 A operand)
        const int io = (int)(i % HID), k = (int)(i / HID);
        const int hh = k / (F / 2), s = k % (F / 2);
        P.w1p[((size_t)((io >> 5) * (F / 8) + (s >> 2)) * 64 + (io & 31) + 32 * hh) * 4 + (s & 3)] = x;
        if (P.w1x) {                                     // split-fp32 train forward: natural k order, 5 k-steps, three pieces
            uint16_t ph, pm, pl;
            split3_bf16(x, ph, pm, pl);
            uint16_t* base = P.w1x + ((size_t)(io >> 5) * 5 + (k >> 4)) * 3 * 512 + ((size_t)(io & 31) + 32 * ((k >> 3) & 1)) * 8 + (k & 7);
            base[0] = pl; base[512] = pm; base[1024] = ph;
        }
        if (P.w1b) {                                     // natural k order: k = 16*step + 8*half + element
            const int KS1 = (F + 15) / 16;
            P.w1b[((size_t)((io >> 5) * KS1 + (k >> 4)) * 64 + (io & 31) + 32 * ((k >> 3) & 1)) * 8 + (k & 7)] = to_bf16(x);
        }
    } else if (i < L.offW2) {
        const int f = (int)(i - L.offb1), kk = f & 31, hh = (kk >> 2) & 1, r = (kk & 3) + 4 * (kk >> 3);
        P.b1p[((f >> 5) * 2 + hh) * 16 + r] = x;
    } else if (i < L.offW3) {                            // hidden->hidden layer `lay`: W[f][k], then its bias
        const int64_t per = (int64_t)HID * HID + HID;
        const int lay = (int)((i - L.offW2) / per);
        const int64_t e = (i - L.offW2) - (int64_t)lay * per;
        if (e >= (int64_t)HID * HID) {                   // bias: accumulator-init order, like b1
            const int f = (int)(e - (int64_t)HID * HID), kk = f & 31, hh = (kk >> 2) & 1, r = (kk & 3) + 4 * (kk >> 3);
            P.b2p[(size_t)lay * HID + ((f >> 5) * 2 + hh) * 16 + r] = x;
            return;
        }
        const size_t lo = (size_t)lay * HID * HID;       // the layers' fragment streams sit back to back
        const int f = (int)(e % HID), k = (int)(e / HID);
        {   // forward A operand: out f, contraction in the previous layer's accumulator-register order
            const int kk = k & 31, hh = (kk >> 2) & 1, r = (kk & 3) + 4 * (kk >> 3);
            const int s = 16 * (k >> 5) + r;
            P.w2p[lo + ((size_t)((f >> 5) * (HID / 8) + (s >> 2)) * 64 + (f & 31) + 32 * hh) * 4 + (s & 3)] = x;
        }
        {   // backward A operand (W^T): out k, contraction slot (group g, component e, lane half hh) of feature f
            const bool zrow = PPO_BWD_Z2ROW_AT(HID);
            const int g = f >> 3, hh = zrow ? (f >> 2) & 1 : f & 1, e = zrow ? f & 3 : (f >> 1) & 3;   // f = 8g + 4hh + e  |  8g + 2e + hh
            P.w2tp[lo + ((size_t)((k >> 5) * (HID / 8) + g) * 64 + (k & 31) + 32 * hh) * 4 + e] = x;
        }
        if (P.w2x && lay == 0) {
            uint16_t ph, pm, pl;
            split3_bf16(x, ph, pm, pl);
            const int KS = HID / 16;
            int s, hh, jj;
            {   // backward: dH1[row, k] = sum_f dZ2[row, f] W[f][k]: B operand, column k, contraction f in the register order
                // of the packed dZ2 accumulator tile; [in-feature tile][k-step][piece lo, mid, hi][64 lanes][8]
                acc_kslot(f & 31, s, hh, jj);
                uint16_t* base = P.w2x + ((size_t)(k >> 5) * KS + 2 * (f >> 5) + s) * 3 * 512 + ((size_t)(k & 31) + 32 * hh) * 8 + jj;
                base[0] = pl; base[512] = pm; base[1024] = ph;
            }
            {   // train forward: H2^T[f, row] = sum_k W[f][k] H1[row, k]: A operand, row f, contraction k in the register order
                // of the packed H1 accumulator tile
                acc_kslot(k & 31, s, hh, jj);
                uint16_t* base = P.w2fx + ((size_t)(f >> 5) * KS + 2 * (k >> 5) + s) * 3 * 512 + ((size_t)(f & 31) + 32 * hh) * 8 + jj;
                base[0] = pl; base[512] = pm; base[1024] = ph;
            }
        }
        if (P.w2b) {
            const uint16_t xb = to_bf16(x);
            int s, hh, jj;
            acc_kslot(k & 31, s, hh, jj);                // forward: out f, contraction k against packed H1 tiles
            P.w2b[((size_t)((f >> 5) * (HID / 16) + 2 * (k >> 5) + s) * 64 + (f & 31) + 32 * hh) * 8 + jj] = xb;
            // backward (W2^T): out k, contraction f in natural order (k-step f>>4, lane half (f>>3)&1, element f&7): the B
            // operand is read straight from the row-major dZ2 image
            P.w2tb[((size_t)((k >> 5) * (HID / 16) + (f >> 4)) * 64 + (k & 31) + 32 * ((f >> 3) & 1)) * 8 + (f & 7)] = xb;
        }
    } else if (i < L.offb3) {                            // W3[oo][k]
        const int64_t e = i - L.offW3;
        const int oo = (int)(e & 3), k = (int)(e >> 2);
        const int kk = k & 31, hh = (kk >> 2) & 1, r = (kk & 3) + 4 * (kk >> 3);
        P.w3p[((size_t)(hh * NT + (k >> 5)) * 16 + r) * 4 + oo] = x;
        if (P.w3c) {
            const uint16_t xb = to_bf16(x);
            int s, h2, jj;
            acc_kslot(k & 31, s, h2, jj);                // forward: rows 0..3 of the layer-3 A operand, [step][half][o][8]
            P.w3c[((size_t)((2 * (k >> 5) + s) * 2 + h2) * 4 + oo) * 8 + jj] = xb;
            P.w3tb[(size_t)k * 4 + oo] = xb;             // backward: W3^T rows [HID][4]
        }
    } else {
        P.b3[i - L.offb3] = x;
    }
}

// Flux legacy Adam on one element: element arithmetic in Float64 (Float64 hyper-parameters against Float32 arrays), Float32
// stores; the bias-correction powers bp1, bp2 are tracked in Float64 on the host.  Returns D (x -= D is the caller's)
__device__ __forceinline__ float adam_delta(float* m, float* v, int64_t i, float g, double eta, double beta1, double beta2,
                                            double eps, double bp1, double bp2) {
    const double gd = (double)g;
    const float mn = (float)(beta1 * (double)m[i] + (1.0 - beta1) * gd);
    const float vn = (float)(beta2 * (double)v[i] + ((1.0 - beta2) * gd) * gd);
    m[i] = mn; v[i] = vn;
    return (float)((double)mn / (1.0 - bp1) / (sqrt((double)vn / (1.0 - bp2)) + eps) * eta);
}

// Adam on one parameter, then its packed copies.  x is loaded after adam_delta's m, v stores, which the compiler must take to
// alias it: written as one expression the load moves in front of them and k_grad_reduce<AdamFuse> schedules differently
__device__ __forceinline__ void adam_one(const AdamFuse& A, const ParamLayout& L, const PackPtrs& P, int64_t i, float g) {
    const float d = adam_delta(A.m, A.v, i, g, A.eta, A.beta1, A.beta2, A.eps, A.bp1, A.bp2);
    const float x = A.params[i] - d;
    A.params[i] = x;
    pack_one(L, P, i, x);
}

__global__ void k_pack_params(const float* __restrict__ params, ParamLayout L, PackPtrs P) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.np) return;
    pack_one(L, P, i, params[i]);
}

// Flux.update! through a chain on one parameter: D = g, D = apply!(member, x, D) in chain order, each member's D rounded
// to float32; returns the final D (x -= D is the caller's)
__device__ __forceinline__ float chain_delta(const ChainFuse& C, int64_t i, float g) {
    float d = g;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j >= C.n) break;
        const double* c = C.c[j];
        const double dd = (double)d;
        const int kind = C.kind[j];
        if (kind == PPO_OPT_ADAM) {
            d = adam_delta(C.s0[j], C.s1[j], i, d, c[0], c[1], c[2], c[3], c[4], c[5]);
        } else if (kind == PPO_OPT_EXPDECAY || kind == PPO_OPT_DESCENT) {  // D .*= eta
            d = (float)(dd * c[0]);
        } else if (kind == PPO_OPT_MOMENTUM) {                             // v = rho v - eta D; D = -v
            const float vn = (float)(c[1] * (double)C.s0[j][i] - c[0] * dd);
            C.s0[j][i] = vn;
            d = -vn;
        } else if (kind == PPO_OPT_NESTEROV) {                             // d = rho^2 v - (1 + rho) eta D; v = rho v - eta D; D = -d
            const double v0 = (double)C.s0[j][i];
            const double dn = (c[1] * c[1]) * v0 - ((1.0 + c[1]) * c[0]) * dd;
            C.s0[j][i] = (float)(c[1] * v0 - c[0] * dd);
            d = (float)(-dn);
        } else if (kind == PPO_OPT_RMSPROP) {                              // acc = rho acc + (1 - rho) D^2; D .*= eta / (sqrt(acc) + eps)
            const float a = (float)(c[1] * (double)C.s0[j][i] + ((1.0 - c[1]) * dd) * dd);
            C.s0[j][i] = a;
            // sqrt of the Float32 array: the float64 root of a float rounds to the correctly rounded float root (53 >= 2*24 + 2)
            const float ra = (float)sqrt((double)a);
            d = (float)(dd * (c[0] / ((double)ra + c[2])));
        } else if (kind == PPO_OPT_CLIPVALUE) {                            // clamp(D, -thresh, thresh); NaN stays NaN
            d = (float)(dd > c[0] ? c[0] : (dd < -c[0] ? -c[0] : dd));
        } else if (kind == PPO_OPT_WEIGHTDECAY) {                          // D += wd x (x before this step's update)
            d = (float)(dd + c[0] * (double)C.params[i]);
        } else {                                                           // InvDecay: D .*= 1 / (1 + gamma n), host-side
            d = (float)(dd * c[0]);
        }
    }
    return d;
}

// (h, l) += (bh, bl) in double-double: the exact error of the leading sum is kept; an infinite or NaN sum stays one
__device__ __forceinline__ void dd_add(double& h, double& l, double bh, double bl) {
    const double s = h + bh;
    if (!isfinite(s)) { h = s; l = 0.0; return; }
    const double v = s - h;
    double e = (h - (s - v)) + (bh - v);
    e += l + bl;
    h = s + e;
    l = e - (h - s);
}

// one double-double sum of D^2 (exact squares) per 32 consecutive elements e, in a fixed shuffle tree; lane 0 of the
// half-wave stores it in slot e / 32.  All 64 lanes of the wave must call it.
__device__ __forceinline__ void clip_partial(double* __restrict__ part, size_t e, float d) {
    double h = (double)d * (double)d, l = 0.0;
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) {
        const double bh = __shfl_down(h, off, 32), bl = __shfl_down(l, off, 32);
        dd_add(h, l, bh, bl);
    }
    if ((e & 31) == 0) { part[2 * (e >> 5)] = h; part[2 * (e >> 5) + 1] = l; }
}

__device__ __forceinline__ void chain_one(const ChainFuse& C, const ParamLayout& L, const PackPtrs& P, int64_t i, float g) {
    const float x = C.params[i] - chain_delta(C, i, g);
    C.params[i] = x;
    pack_one(L, P, i, x);
}

// standalone update (all-reduce hook path, ppo_step_batch, ppo_adam_apply): k_opt_update<AdamFuse> is timed as k_adam,
// k_opt_update<ChainFuse> as k_chain_update
template <typename Fuse>
__global__ void k_opt_update(const float* __restrict__ grad, ParamLayout L, PackPtrs P, Fuse A) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (A.hist2 && i < 2) A.hist2[i] = grad[L.np + i];   // per-batch loss history (after any all-reduce)
    if (i >= L.np) return;
    fuse_one(A, L, P, i, grad[i]);
}

// ClipNorm phase 1 behind an all-reduce (hook path, ppo_step_batch, ppo_adam_apply): slot = Flux-order index / 32
__global__ __launch_bounds__(256) void k_chain_clip1(const float* __restrict__ grad, ParamLayout L, ClipFuse A) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (A.hist2 && i < 2) A.hist2[i] = grad[L.np + i];   // per-batch loss history (after any all-reduce)
    float d = 0.f;
    if (i < L.np) {
        d = chain_delta(A.C, i, grad[i]);
        A.dbuf[i] = d;
    }
    clip_partial(A.part, (size_t)i, d);
}

// the 2L + 2 arrays of Flux.params: Flux-order start of each (start[na] = np) and the range of partial-sum slots phase 1
// wrote for it
#define PPO_CLIP_MAX_ARRAYS 10
struct ClipMap {
    const float* dbuf; const double* part;
    double thresh;
    int na;
    int64_t start[PPO_CLIP_MAX_ARRAYS + 1];
    int32_t s0[PPO_CLIP_MAX_ARRAYS], s1[PPO_CLIP_MAX_ARRAYS];
};
__device__ __forceinline__ int clip_array(const ClipMap& M, int64_t i) {
    int a = 0;
    while (a + 1 < M.na && i >= M.start[a + 1]) ++a;
    return a;
}

// ClipNorm phase 2: one parameter per thread, 256 per block (many blocks: the re-pack's scattered stores want the CUs).
// The block first finishes the norm of every array its range touches -- each thread a strided double-double sum over the
// array's slots (8 loads in flight), the wave's shuffle tree, the 4 waves in order -- the same fixed order in every block;
// then D = dbuf (scaled when nrm > thresh), members (c, n) of the chain (C), x -= D, re-pack
#define PPO_CLIP_BLOCK 256
__global__ __launch_bounds__(PPO_CLIP_BLOCK) void k_clip_apply(ParamLayout L, PackPtrs P, ChainFuse C, ClipMap M) {
    __shared__ double wsum[PPO_CLIP_BLOCK / 64][2];
    __shared__ float nrm[PPO_CLIP_MAX_ARRAYS];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * PPO_CLIP_BLOCK, i = i0 + t;
    const int a0 = clip_array(M, i0), a1 = clip_array(M, std::min<int64_t>(i0 + PPO_CLIP_BLOCK, L.np) - 1);
    for (int a = a0; a <= a1; ++a) {
        double h = 0.0, l = 0.0;
        for (int s = M.s0[a] + t; s < M.s1[a]; s += 8 * PPO_CLIP_BLOCK) {
            double v[8][2];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int su = s + u * PPO_CLIP_BLOCK;
                v[u][0] = su < M.s1[a] ? M.part[2 * (size_t)su] : 0.0;
                v[u][1] = su < M.s1[a] ? M.part[2 * (size_t)su + 1] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) dd_add(h, l, v[u][0], v[u][1]);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double bh = __shfl_down(h, off, 64), bl = __shfl_down(l, off, 64);
            dd_add(h, l, bh, bl);
        }
        if (lane == 0) { wsum[w][0] = h; wsum[w][1] = l; }
        __syncthreads();
        if (t == 0) {
            double H = wsum[0][0], Lo = wsum[0][1];
            for (int k = 1; k < PPO_CLIP_BLOCK / 64; ++k) dd_add(H, Lo, wsum[k][0], wsum[k][1]);
            nrm[a] = (float)sqrt(H + Lo);                   // S rounded once; nrm = f32(sqrt(S))
        }
        __syncthreads();
    }
    if (i >= L.np) return;
    float d = M.dbuf[i];
    const double nr = (double)nrm[clip_array(M, i)];
    if (nr > M.thresh) d = (float)((double)d * (M.thresh / nr));
    const float x = C.params[i] - chain_delta(C, i, d);
    C.params[i] = x;
    pack_one(L, P, i, x);
}

// dataset order -> minibatch order: out[i] = index[perm_epoch(i)]
__global__ void k_feistel_index(const int32_t* __restrict__ index, int64_t len, uint64_t seed, uint32_t epoch,
                                int32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len) return;
    out[i] = index[feistel_perm(i, len, seed, epoch)];
}

static PackPtrs packs_of(ppo_policy_s* p) {
    PackPtrs P;
    P.w1p = p->w1p.p; P.w2p = p->w2p.p; P.w2tp = p->w2tp.p; P.b1p = p->b1p.p; P.b2p = p->b2p.p; P.w3p = p->w3p.p;
    P.b3 = p->b3.p;
    const bool b = (p->dtype == PPO_DTYPE_BF16);
    P.w1b = b ? p->w1b.p : nullptr; P.w2b = b ? p->w2b.p : nullptr; P.w2tb = b ? p->w2tb.p : nullptr;
    P.w3c = b ? p->w3c.p : nullptr; P.w3tb = b ? p->w3tb.p : nullptr;
    P.w2x = p->w2x.p; P.w1x = p->w1x.p; P.w2fx = p->w2fx.p;
    return P;
}

int32_t launch_pack_params(ppo_policy_s* p) {
    ParamLayout L = layout_of(p);
    hipLaunchKernelGGL(k_pack_params, dim3((unsigned)((L.np + 255) / 256)), dim3(256), 0, ppo_stream(), p->params.p, L,
                       packs_of(p));
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

// one optimiser step of a chain: the members' scalars for this step (ExpDecay advances its counter and, on schedule, its eta
// first: Flux's apply! does it before it scales the first array); the Adam member's beta powers advance after the launch
// (chain_done)
static ChainFuse chain_step(ppo_adam_s* o, float* hist2) {
    ChainFuse C = {};
    C.params = o->pol->params.p; C.hist2 = hist2; C.on = 1; C.n = o->nmem;
    for (int j = 0; j < o->nmem; ++j) {
        OptMember& e = o->mem[j];
        double* c = C.c[j];
        C.kind[j] = e.kind;
        switch (e.kind) {
        case PPO_OPT_EXPDECAY: {   // h1 decay, h2 decay_step, h3 clip, h4 start
            const int64_t n = ++e.count, st = (int64_t)e.h2, start = (int64_t)e.h4;
            // Flux decays when exactly one array's counter is on schedule: once per step for decay_step > 1; with decay_step
            // == 1 only at the first step past `start` (or at step 1, while the other arrays have no counter yet)
            if (n > start && n % st == 0 && (st > 1 || n == start + 1 || n == 1)) e.eta = std::max(e.eta * e.h1, e.h3);
            c[0] = e.eta;
            break;
        }
        case PPO_OPT_INVDECAY: {   // h0 gamma: n counts its update! calls, this one included
            const int64_t n = ++e.count;
            c[0] = 1.0 / (1.0 + e.eta * (double)n);
            break;
        }
        case PPO_OPT_CLIPNORM:     // not a chain_delta member: split_at_clip takes it out (thresh: ClipMap)
            break;
        default:                   // the hyper row as it stands and the state arrays the member has: Adam (with its beta
                                   // powers), Descent, Momentum, Nesterov, RMSProp, ClipValue (thresh), WeightDecay (wd)
            c[0] = e.eta; c[1] = e.h1; c[2] = e.h2; c[3] = e.h3; c[4] = e.beta_pow[0]; c[5] = e.beta_pow[1];
            C.s0[j] = e.s.p; C.s1[j] = e.s1.p;
            break;
        }
    }
    return C;
}

// ---------------------------------------------------------------- ClipNorm: the two-launch update
static int clip_position(const ppo_adam_s* o) {
    for (int j = 0; j < o->nmem; ++j)
        if (o->mem[j].kind == PPO_OPT_CLIPNORM) return j;
    return -1;
}

// slots: k_grad_reduce<ClipFuse> writes two per 64-element block, k_chain_clip1 eight per 256-thread block
int64_t clip_slot_count(const ppo_policy_s* p) {
    const ParamLayout L = layout_of(p);
    return std::max<int64_t>(2 * (int64_t)((slab_elems(p->F, p->HID, p->L) + 63) / 64), 8 * ((L.np + 255) / 256));
}

// the chain of this step (chain_step) split around its ClipNorm at position c: members [0, c) for phase 1, (c, n) for phase 2
static void split_at_clip(const ChainFuse& C, int c, ChainFuse& before, ChainFuse& after) {
    before = C;
    before.n = c;
    after = C;
    after.hist2 = nullptr;
    after.n = C.n - c - 1;
    for (int j = 0; j < after.n; ++j) {
        after.kind[j] = C.kind[c + 1 + j];
        std::memcpy(after.c[j], C.c[c + 1 + j], sizeof(after.c[j]));
        after.s0[j] = C.s0[c + 1 + j]; after.s1[j] = C.s1[c + 1 + j];
    }
}

// Flux.params arrays in order (W1, b1, (W, b) per hidden->hidden layer, W3, b3) with the slots phase 1 wrote for each:
// in the slab order of k_grad_reduce (slab_order) or in the Flux order of k_chain_clip1
static ClipMap clip_map(const ppo_adam_s* o, const ParamLayout& L, bool slab_order) {
    ClipMap M = {};
    M.dbuf = o->clip_d.p; M.part = o->clip_part.p; M.thresh = o->mem[clip_position(o)].eta;
    const int64_t H = L.HID, nW2l = H * H, nW2 = (int64_t)L.NL2 * nW2l, nW1 = H * L.FP, tail = nW2 + nW1;
    auto add = [&](int64_t canon_lo, int64_t canon_hi, int64_t slab_lo, int64_t slab_hi) {
        const int64_t lo = slab_order ? slab_lo : canon_lo, hi = slab_order ? slab_hi : canon_hi;
        M.start[M.na] = canon_lo; M.s0[M.na] = (int32_t)(lo / 32); M.s1[M.na] = (int32_t)((hi + 31) / 32);
        ++M.na;
    };
    add(L.offW1, L.offb1, nW2, nW2 + nW1);                                  // W1 (the slab block also holds the dead columns)
    add(L.offb1, L.offW2, tail, tail + H);                                  // b1
    for (int l = 0; l < L.NL2; ++l) {
        const int64_t w = L.offW2 + l * (nW2l + H);
        add(w, w + nW2l, l * nW2l, (l + 1) * nW2l);                         // W of hidden->hidden layer l
        add(w + nW2l, w + nW2l + H, tail + H * (1 + l), tail + H * (2 + l)); // its b
    }
    const int64_t t3 = tail + H * (1 + L.NL2);
    add(L.offW3, L.offb3, t3, t3 + 4 * H);                                  // W3
    add(L.offb3, L.np, t3 + 4 * H, t3 + 4 * H + 4);                         // b3
    M.start[M.na] = L.np;
    return M;
}

// phase 1 is launched by the caller; this is phase 2
static int32_t launch_clip_apply(ppo_adam_s* o, const ParamLayout& L, const ChainFuse& after, bool slab_order) {
    ppo_policy_s* p = o->pol;
    const ClipMap M = clip_map(o, L, slab_order);
    ProfScope ps("k_clip_apply");
    hipLaunchKernelGGL(k_clip_apply, dim3((unsigned)((L.np + PPO_CLIP_BLOCK - 1) / PPO_CLIP_BLOCK)), dim3(PPO_CLIP_BLOCK), 0,
                       ppo_stream(), L, packs_of(p), after, M);
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

// this step's ClipFuse (members before the ClipNorm) and the members after it
static ClipFuse clip_fuse(ppo_adam_s* o, float* hist2, ChainFuse& after) {
    ClipFuse A = {};
    split_at_clip(chain_step(o, hist2), clip_position(o), A.C, after);
    A.hist2 = hist2; A.on = 1; A.dbuf = o->clip_d.p; A.part = o->clip_part.p;
    return A;
}

// a chain of Adam alone: the Adam kernels' argument
static AdamFuse adam_fuse(const ppo_adam_s* o, float* hist2) {
    const OptMember& e = o->mem[0];
    AdamFuse A = {};
    A.params = o->pol->params.p; A.m = e.s.p; A.v = e.s1.p; A.eta = e.eta; A.beta1 = e.h1; A.beta2 = e.h2; A.eps = e.h3;
    A.bp1 = e.beta_pow[0]; A.bp2 = e.beta_pow[1]; A.hist2 = hist2; A.on = 1;
    return A;
}

// after a step's launches: the Adam member's beta powers for the next step
static void chain_done(ppo_adam_s* o) {
    for (int j = 0; j < o->nmem; ++j)
        if (o->mem[j].kind == PPO_OPT_ADAM) { o->mem[j].beta_pow[0] *= o->mem[j].h1; o->mem[j].beta_pow[1] *= o->mem[j].h2; }
}

template <typename Fuse>
static int32_t reduce_launch(const char* name, ppo_policy_s* p, const ParamLayout& L, int64_t B, int64_t B_global,
                             double entropy_weight, const Fuse& A) {
    ProfScope ps(name);
    hipLaunchKernelGGL(k_grad_reduce<Fuse>, dim3((unsigned)((slab_elems(p->F, p->HID, p->L) + 63) / 64) + 1), dim3(256), 0, ppo_stream(),
                       p->slabs.p, slab_floats(p->F, p->HID, p->L), p->nwg_bwd, p->nwg_small ? p->nwg_small : p->nwg_bwd, L, p->grad.p,
                       p->loss_terms.p, B, 1.0 / (double)B_global, entropy_weight, A, packs_of(p));
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

template <typename Fuse>
static int32_t update_launch(const char* name, ppo_policy_s* p, const ParamLayout& L, const Fuse& A) {
    ProfScope ps(name);
    hipLaunchKernelGGL(k_opt_update<Fuse>, dim3((unsigned)((L.np + 255) / 256)), dim3(256), 0, ppo_stream(), p->grad.p, L, packs_of(p), A);
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

// slab reduction + (one extra block) loss-term reduction in a single launch; with `fuse`, its optimiser step in the same launch
int32_t launch_grad_reduce(ppo_policy_s* p, int64_t B, int64_t B_global, double entropy_weight, ppo_adam_s* fuse, float* hist2) {
    const ParamLayout L = layout_of(p);
    if (!fuse) return reduce_launch("k_grad_reduce", p, L, B, B_global, entropy_weight, AdamFuse{});
    if (clip_position(fuse) >= 0) {
        ChainFuse after;
        PPO_TRY(reduce_launch("k_reduce_clip", p, L, B, B_global, entropy_weight, clip_fuse(fuse, hist2, after)));
        PPO_TRY(launch_clip_apply(fuse, L, after, true));
    } else if (fuse->adam_only()) {
        PPO_TRY(reduce_launch("k_reduce_adam", p, L, B, B_global, entropy_weight, adam_fuse(fuse, hist2)));
    } else {
        PPO_TRY(reduce_launch("k_reduce_chain", p, L, B, B_global, entropy_weight, chain_step(fuse, hist2)));
    }
    chain_done(fuse);
    return PPO_OK;
}

int32_t launch_adam(ppo_adam_s* o, float* hist2) {
    ppo_policy_s* p = o->pol;
    const ParamLayout L = layout_of(p);
    if (clip_position(o) >= 0) {
        ChainFuse after;
        const ClipFuse A = clip_fuse(o, hist2, after);
        {
            ProfScope ps("k_chain_clip1");
            hipLaunchKernelGGL(k_chain_clip1, dim3((unsigned)((L.np + 255) / 256)), dim3(256), 0, ppo_stream(), p->grad.p, L, A);
            HIP_TRY(hipGetLastError());
        }
        PPO_TRY(launch_clip_apply(o, L, after, false));
    } else if (o->adam_only()) {
        PPO_TRY(update_launch("k_adam", p, L, adam_fuse(o, hist2)));
    } else {
        PPO_TRY(update_launch("k_chain_update", p, L, chain_step(o, hist2)));
    }
    chain_done(o);
    return PPO_OK;
}

int32_t launch_feistel_index(const int32_t* index_dev, int64_t len, uint64_t seed, uint32_t epoch, int32_t* out_dev) {
    if (len <= 0) return PPO_OK;
    hipLaunchKernelGGL(k_feistel_index, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, ppo_stream(), index_dev, len,
                       seed, epoch, out_dev);
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

// batch_advantage plugin, PPO_ADV_RETURNS_NORMALISED (src/ProximalPolicyOptimization.jl:29 declares the plugin, the
// reference ships no implementation): adv = (R - mean(R)) / (std(R) + 1e-8) over the minibatch, population std,
// statistics in fp64.  One workgroup: two fixed-order block reductions, then the normalised values are scattered
// into a scratch column at their transition ids so the forward kernel reads them exactly like the returns column.
__global__ __launch_bounds__(1024) void k_adv_normalise(const float* __restrict__ returns, const int32_t* __restrict__ idx,
                                                        int64_t B, float* __restrict__ adv_col) {
    __shared__ double red[1024];
    __shared__ double stat[2];
    const int t = threadIdx.x;
    double s = 0.0;
    for (int64_t i = t; i < B; i += 1024) s += (double)returns[idx[i]];
    red[t] = s;
    __syncthreads();
    for (int off = 512; off >= 1; off >>= 1) { if (t < off) red[t] += red[t + off]; __syncthreads(); }
    if (t == 0) stat[0] = red[0] / (double)B;
    __syncthreads();
    const double mean = stat[0];
    s = 0.0;
    for (int64_t i = t; i < B; i += 1024) { const double d = (double)returns[idx[i]] - mean; s += d * d; }
    __syncthreads();
    red[t] = s;
    __syncthreads();
    for (int off = 512; off >= 1; off >>= 1) { if (t < off) red[t] += red[t + off]; __syncthreads(); }
    if (t == 0) stat[1] = 1.0 / (sqrt(red[0] / (double)B) + 1e-8);
    __syncthreads();
    const double inv = stat[1];
    for (int64_t i = t; i < B; i += 1024) { const int32_t k = idx[i]; adv_col[k] = (float)(((double)returns[k] - mean) * inv); }
}

int32_t launch_adv_normalise(const float* returns, const int32_t* idx_dev, int64_t B, float* adv_col) {
    hipLaunchKernelGGL(k_adv_normalise, dim3(1), dim3(1024), 0, ppo_stream(), returns, idx_dev, B, adv_col);
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}
