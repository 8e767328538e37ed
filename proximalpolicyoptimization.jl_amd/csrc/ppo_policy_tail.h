// ppo_policy_tail.h -- the part of the policy forward that both compute modes (fp32 MFMA, bf16 MFMA) share:
// kernel arguments, and everything behind the 4 logits per lane of a state -- masked softmax
// (test/quad_game_utilities.jl:68-69,76-77), rand(Categorical) + ap[a] > 0 (src/collect_rollouts.jl:6-7), and the
// loss / dlogits of ppo_loss_with_entropy (src/train.jl:21-26,35-46).  All fp32 in both modes.
#pragma once
#include "ppo_internal.h"
#include "ppo_device.h"

struct FwdArgs {
    // inputs
    const int8_t* states;      // FwdSource::Rows: [B][H][F]; RowsIdx: rollout states base (gathered by idx)
    const uint32_t* active;    // same indexing as states
    const int32_t* idx;        // RowsIdx / SnapIdx: transition id per state
    int64_t B;
    unsigned long long* stamps;   // diagnostic build only (-DPPO_FWD_STAMP)
    int unused_wg_sync;        // no kernel reads it (it allowed per-chunk barriers in a build that is gone) and nothing fills it: it
                               // keeps the offsets below, see profiles/build_knobs_code_identity.txt
    const float4* w1p; const float4* w2p; const float4* b1p; const float4* b2p; const float4* w3p; const float* b3;
    // FwdTail::Probs
    float* probs_out;
    // the rollout tails (Sample .. Truncated, Forced)
    const uint32_t* tick; int64_t global_offset; uint32_t k0, k1;
    int32_t* actions_out; float* psel_out; float* full_probs; int32_t* err;
    // the train tails
    float4* act1; float4* act2; float4* dY; double* loss_terms;
    const int32_t* actions; const float* p_old; const float* adv;
    // ... and, in the same storage, what the selection tails (which train nothing) read instead: Tempered / Greedy / Truncated
    // the factor 1 / temperature, Truncated top_k (an integer a double holds exactly) and top_p
    union { double eps; double top_k; };
    union { float c_over_B; float top_p; };
    union { float inv_B; float inv_temperature; };
    // FwdSource::EnvSlots (persistent rollout: T steps of every env in ONE launch; env state lives in the wave's LDS slots)
    int64_t T;                                                   // steps
    int8_t* env_score; int8_t* env_degree; uint32_t* env_active; int32_t* env_steps; float* env_reward;
    uint8_t* env_done; uint32_t* env_episode; uint32_t* env_tick; const int8_t* env_tmpl;
    int32_t envQ, envV, env_max_actions, env_slots; float env_nar;
    int8_t* states_out; uint32_t* active_out; float* rew_out; uint8_t* done_out;      // rollout columns [T][N]
    // compact rollout storage: an env snapshot (score[V] then degree[V], int8) per transition instead of the expanded
    // [H][F] observation.  The persistent rollout writes cstate_out (states_out may then be null); Snap / SnapIdx read cstate,
    // re-deriving the rows like the persistent rollout, SnapIdx leaving them in xs_out (minibatch order) for the backward
    int8_t* cstate_out; const int8_t* cstate; int8_t* xs_out;
    // deep form (num_hidden_layers != 2, k_policy_fwd<.., DEEP = 1>): nl2 = hidden->hidden layers (L - 1: 0, 2 or 3), w2p /
    // b2p hold them back to back; act_mid[l] = saved output of hidden->hidden layer l < nl2 - 1 (the last one goes to act2,
    // with nl2 == 0 only act1 exists); park_off = byte offset of the waves' activation park in dynamic LDS
    int32_t nl2; float4* act_mid[2]; uint32_t park_off;
    // bf16 compute mode (ppo_policy_bf16.hip): bf16 fragment streams and bf16 saved activations
    const uint4* w1b; const uint4* w2b; const uint4* w3c; uint4* act1b; uint4* act2b;
    // critic (k_policy_fwd value modes, value_tail): state values out, indexed like the states (predict); regression target per
    // transition id (train).  Appended last: the offsets of every field above are what the other kernels were built with
    float* values_out; const float* vtarget;
    // FwdTail::Train, optional: ratio_out[state] = p_new(a|s) / p_old(a|s) of every state of the minibatch, the quotient the
    // surrogate forms (per-epoch KL / clip-fraction statistics, ppo_stats.hip).  Appended last, like the two above
    float* ratio_out;
    // value-train, optional (PPO's clipped value loss, value_tail): vold = the values the critic had before the update,
    // indexed by transition id like vtarget (nullptr: plain mse); vclip = the clip range; vdelta_out[state] = V - vold of
    // every state of the minibatch (per-epoch value-clip statistics, ppo_stats.hip; nullptr: not stored).  Appended last
    const float* vold; float vclip; float* vdelta_out;
    // FwdTail::Distill: the target distributions [T*N][A] by transition id, entry 128 ts + 4 j + i of a row as probs_out and
    // full_probs hold it.  Appended last
    const float* targets;
    // FwdTail::TrainAnchored: the coefficient beta of the penalty towards the target rows (a.targets), and,
    // optional, anchor_out[state] = the divergence KL(q' || pi) of every state of the minibatch.  Appended last
    double beta; float* anchor_out;
};
// the aliases move nothing: these are the layout every kernel was built with
static_assert(sizeof(FwdArgs) == 536 && offsetof(FwdArgs, vdelta_out) == 504 && offsetof(FwdArgs, targets) == 512 &&
              offsetof(FwdArgs, beta) == 520, "FwdArgs layout");

// value of lane (lane ^ OFF), OFF < 32.  Same lane mapping as __shfl_xor (which hipcc lowers to ds_bpermute_b32: an
// LDS round trip of ~100+ cycles per step, fully exposed in the one-or-two-waves-per-SIMD kernels here), but as DPP
// moves where the xor is a DPP pattern (1, 2: quad_perm; 8: row_ror:8; 4: row_shl:4 / row_shr:4 on alternate banks)
// and ds_swizzle (no address VGPR) for 16.  Bit-identical results: only the transport changes.
template <int OFF>
__device__ __forceinline__ float xor_lane(float v) {
    static_assert(OFF == 1 || OFF == 2 || OFF == 4 || OFF == 8 || OFF == 16, "the steps of a 32-lane butterfly");
    const int x = __float_as_int(v);
    if (OFF == 1) return __int_as_float(__builtin_amdgcn_update_dpp(x, x, 0xB1, 0xF, 0xF, false));          // quad_perm:[1,0,3,2]
    if (OFF == 2) return __int_as_float(__builtin_amdgcn_update_dpp(x, x, 0x4E, 0xF, 0xF, false));          // quad_perm:[2,3,0,1]
    if (OFF == 4) {
        const int t = __builtin_amdgcn_update_dpp(x, x, 0x104, 0xF, 0x5, false);                            // row_shl:4 -> banks 0, 2
        return __int_as_float(__builtin_amdgcn_update_dpp(t, x, 0x114, 0xF, 0xA, false));                   // row_shr:4 -> banks 1, 3
    }
    if (OFF == 8) return __int_as_float(__builtin_amdgcn_update_dpp(x, x, 0x128, 0xF, 0xF, false));         // row_ror:8
    return __int_as_float(__builtin_amdgcn_ds_swizzle(x, 0x401F));                                           // OFF == 16, bitmode: xor 16
}
__device__ __forceinline__ float wave32_max(float v) {
    v = fmaxf(v, xor_lane<16>(v)); v = fmaxf(v, xor_lane<8>(v)); v = fmaxf(v, xor_lane<4>(v));
    v = fmaxf(v, xor_lane<2>(v)); v = fmaxf(v, xor_lane<1>(v));
    return v;
}
__device__ __forceinline__ float wave32_sum(float v) {
    v = v + xor_lane<16>(v); v = v + xor_lane<8>(v); v = v + xor_lane<4>(v);
    v = v + xor_lane<2>(v); v = v + xor_lane<1>(v);
    return v;
}
__device__ __forceinline__ float readlane_f(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}


// bf16 compute mode hands dL/dlogits to the backward MFMAs as bf16: round once here (RNE), keep the fp32 container
template <bool DYBF16>
__device__ __forceinline__ float dy_round(float x) {
    if (!DYBF16) return x;
    return (float)(__bf16)x;
}

// FwdTail::Train inputs of one transition, when the caller fetched them ahead of its own stores (vmcnt counts loads and stores
// in one in-order queue on gfx9: a load issued behind a store cannot be waited for without waiting for the store)
struct TailPre { int ab; float po; float adv; };

// the entropy term of ppo_loss_with_entropy on the smoothed probabilities sp = p + smooth / A (src/train.jl:22):
// lg = log(sp) per entry; returns sum(sp * lg) over the state
template <int TPS>
__device__ __forceinline__ float smoothed_entropy(const float (&p)[TPS][4], float (&lg)[TPS][4]) {
    const float sA = 1e-8f / (float)(128 * TPS);
    float hl = 0.0f;
#pragma unroll
    for (int ts = 0; ts < TPS; ++ts)
#pragma unroll
        for (int i = 0; i < 4; ++i) { const float sp = p[ts][i] + sA; lg[ts][i] = logf(sp); hl += sp * lg[ts][i]; }
    return wave32_sum(hl);
}

// l[ts][i]: logit of action 128*ts + 4*j + i of the state, present in both lane halves (j = lane & 31).
// Sample / SamplePersistent (rollout): tick_val = the env's tick (Philox counter word), out_index = position of the transition in
// the output columns (state for one step, t*N + state for the persistent rollout); returns the sampled action.
// Forced (teacher-forced step): Sample's outputs for the action in pre->ab instead of a sampled one; returns it.
// Train: the loss and dL/dlogits of ppo_loss_with_entropy, whatever the source of the state.
// Imitate: Train's outputs for the cross-entropy of the action in pre->ab, weighted by max(pre->adv, 0); pre is required.
// Distill: Train's outputs for the cross-entropy against the state's target row, weighted like Imitate; pre (adv)
// and qrow are required: qrow[ts] = entries 128 ts + 4 j .. + 3 of a.targets' row sid, the caller's fetch (registers).
// TrainAnchored: Train's surrogate plus a.beta times Distill's cross-entropy against the target row; pre (ab, po,
// adv) and qrow are required.
// Tempered / Greedy (selection rules): Sample on the logits times a.inv_temperature; Tempered samples like Sample,
// Greedy takes the first maximum of p instead (tick_val unused).  l is scaled in place.
// Truncated: Tempered on the top-k / nucleus truncation of the tempered p, renormalised; a.top_k (0: all),
// a.top_p (1: all).
// dy_copy (Train, TPS == 1, optional): a second destination for the state's 32 dL/dlogits rows, e.g. an LDS tile of the
// calling workgroup (k_policy_train_tile keeps the whole training pass of a tile on the CU).
// (The pick of entry ab and the probs_out store are written out at each site: as helpers they compile to other code.)
template <FwdTail TAIL, int TPS, bool DYBF16>
__device__ __forceinline__ int policy_tail(const FwdArgs& a, const int64_t state, const int64_t sid, const uint32_t act,
                                           float (&l)[TPS][4], const int lane, const int j, const int h,
                                           const uint32_t tick_val = 0u, const int64_t out_index = 0,
                                           const TailPre* pre = nullptr, float4* dy_copy = nullptr,
                                           const float4* qrow = nullptr) {
    static_assert(!tail_value(TAIL), "the critic's tails are value_tail's");
    int sampled = 0;
    constexpr int A = 128 * TPS;
    if (tail_tempers(TAIL)) {
        // selection temperature: l' = l * (float)(1 / temperature), one fp32 multiply per logit in front of the
        // masked max
        const float inv = a.inv_temperature;
#pragma unroll
        for (int ts = 0; ts < TPS; ++ts)
#pragma unroll
            for (int i = 0; i < 4; ++i) l[ts][i] = l[ts][i] * inv;
    }
    // ---- masked softmax over the A = 128*TPS logits of the state (quad of row 32ts+j = 8ts + j/4)
    bool on[TPS];
    float m = -INFINITY;
#pragma unroll
    for (int ts = 0; ts < TPS; ++ts) {
        on[ts] = (act >> (8 * ts + (j >> 2))) & 1u;
        if (on[ts]) m = fmaxf(m, fmaxf(fmaxf(l[ts][0], l[ts][1]), fmaxf(l[ts][2], l[ts][3])));
    }
    m = wave32_max(m);
    float p[TPS][4];
    float ssum = 0.0f;
#pragma unroll
    for (int ts = 0; ts < TPS; ++ts) {
#pragma unroll
        for (int i = 0; i < 4; ++i) p[ts][i] = on[ts] ? exp_dev(l[ts][i] - m) : 0.0f;
        const float st = ((p[ts][0] + p[ts][1]) + p[ts][2]) + p[ts][3];
        ssum = (ts == 0) ? st : ssum + st;                 // tile partials in tile order, then the butterfly
    }
    ssum = wave32_sum(ssum);
#pragma unroll
    for (int ts = 0; ts < TPS; ++ts)
#pragma unroll
        for (int i = 0; i < 4; ++i) p[ts][i] = p[ts][i] / ssum;

    if (TAIL == FwdTail::Truncated) {
        // top-k / nucleus truncation.  b precedes a iff p[b] > p[a] || (p[b] == p[a] && b < a); rank(a) counts the b
        // that precede a, mass(a) adds their p[b] in ascending b (fp32, one rounding per add).  One pass over b = 0 .. A - 1 in
        // ascending order serves every a: p[b] is broadcast by readlane like the walk below broadcasts it, and each lane updates
        // the rank and the mass of its 4 * TPS entries.  b = 128 tb + 4 jb + ib with tb and ib compile-time and the lane jb a
        // rolled loop (v_readlane takes its lane from an SGPR): 32 bodies' worth less code than the full unroll, same order.
        // "b < a" for a = 128 ts + 4 j + i needs no index compare: ts != tb decides it at compile time, ts == tb leaves
        // j > jb, or j >= jb where ib < i.  A state without an active quad has p NaN everywhere: no comparison holds, rank and
        // mass stay 0, everything is kept and NaN stays NaN -- what Tempered leaves for such a state.
        const int top_k = (int)a.top_k;
        const float top_p = a.top_p;
        int rk[TPS][4];
        float ms[TPS][4];
#pragma unroll
        for (int ts = 0; ts < TPS; ++ts)
#pragma unroll
            for (int i = 0; i < 4; ++i) { rk[ts][i] = 0; ms[ts][i] = 0.0f; }
#pragma unroll
        for (int tb = 0; tb < TPS; ++tb) {
#pragma unroll 1
            for (int jb = 0; jb < 32; ++jb) {
                const bool behind = j > jb, at_or_behind = j >= jb;
#pragma unroll
                for (int ib = 0; ib < 4; ++ib) {
                    const float pb = readlane_f(p[tb][ib], jb);
#pragma unroll
                    for (int ts = 0; ts < TPS; ++ts)
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            // where b < a an equal p precedes too: pb >= pa in one compare where the tiles decide it.
                            // (| and & on purpose: || and && become a branch on the exec mask per entry, measured 75 us
                            // per launch of 4096 states at Q = 8 where this form takes 46)
                            const float pa = p[ts][i];
                            bool prec;
                            if (ts > tb) prec = pb >= pa;
                            else if (ts < tb) prec = pb > pa;
                            else prec = (pb > pa) | ((pb == pa) & (ib < i ? at_or_behind : behind));
                            rk[ts][i] = prec ? rk[ts][i] + 1 : rk[ts][i];
                            ms[ts][i] = prec ? ms[ts][i] + pb : ms[ts][i];
                        }
                }
            }
        }
        // keep, renormalise: the sum of the kept p in the softmax's own order, one division per entry.  Any truncation that
        // reaches this mode renormalises, also one that keeps everything
        float ksum = 0.0f;
#pragma unroll
        for (int ts = 0; ts < TPS; ++ts) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bool keep = (top_k == 0 || rk[ts][i] < top_k) && (top_p == 1.0f || ms[ts][i] < top_p);
                p[ts][i] = keep ? p[ts][i] : 0.0f;
            }
            const float st = ((p[ts][0] + p[ts][1]) + p[ts][2]) + p[ts][3];
            ksum = (ts == 0) ? st : ksum + st;
        }
        ksum = wave32_sum(ksum);
#pragma unroll
        for (int ts = 0; ts < TPS; ++ts)
#pragma unroll
            for (int i = 0; i < 4; ++i) p[ts][i] = p[ts][i] / ksum;
    }

    if (TAIL == FwdTail::Probs) {
        if (h == 0) {
#pragma unroll
            for (int ts = 0; ts < TPS; ++ts)
                reinterpret_cast<float4*>(a.probs_out)[((size_t)state * TPS + ts) * 32 + j] =
                    make_float4(p[ts][0], p[ts][1], p[ts][2], p[ts][3]);
        }
    }
    if (tail_samples(TAIL)) {
        // rand(Categorical(p)): sequential fp32 inverse-CDF walk, same uniform as the oracle (Tempered: over the tempered p;
        // Truncated: over its renormalised truncation)
        uint32_t rnd[4];
        philox4x32_10((uint32_t)(a.global_offset + state), tick_val, 0u, 0u, a.k0, a.k1, rnd);
        const float u = u01_from_u32(rnd[0]);
        float cp = readlane_f(p[0][0], 0);
        int ia = 0;
#pragma unroll
        for (int q = 1; q < A; ++q) {
            const float pa = readlane_f(p[q >> 7][q & 3], (q & 127) >> 2);
            const bool take = cp <= u;
            cp = take ? cp + pa : cp;
            ia = take ? q : ia;
        }
        float cand = 0.0f;
#pragma unroll
        for (int ts = 0; ts < TPS; ++ts)
#pragma unroll
            for (int i = 0; i < 4; ++i) cand = ((ia >> 7) == ts && (ia & 3) == i) ? p[ts][i] : cand;
        float psel = __shfl(cand, (ia & 127) >> 2);
        if (!(psel > 0.0f)) {                            // wave-uniform, about 3 in 10^8 samples
            // The walk ran off the end: the sequential fp32 sum of the probabilities fell short of u (u within a few
            // 2^-24 of 1).  Distributions.jl lets the LAST bin absorb that rounding residue; when the last action is
            // masked its probability is 0 and the reference's `@assert ap[a] > 0.0` throws -- at 10^6 samples per
            // iteration that would abort a run every few iterations.  The engine hands the residue to the last action
            // with non-zero probability instead (flag bit 32, informational); a distribution without any positive
            // entry still raises (bit 8).
            int best = -1;
#pragma unroll
            for (int ts = 0; ts < TPS; ++ts)
#pragma unroll
                for (int i = 0; i < 4; ++i) best = (p[ts][i] > 0.0f) ? 128 * ts + 4 * j + i : best;    // ascending: last wins
#pragma unroll
            for (int off = 16; off >= 1; off >>= 1) best = max(best, __shfl_xor(best, off));
            if (best >= 0) {
                ia = best;
                cand = 0.0f;
#pragma unroll
                for (int ts = 0; ts < TPS; ++ts)
#pragma unroll
                    for (int i = 0; i < 4; ++i) cand = ((ia >> 7) == ts && (ia & 3) == i) ? p[ts][i] : cand;
                psel = __shfl(cand, (ia & 127) >> 2);
            }
            if (lane == 0) atomicOr(a.err, best >= 0 ? 32 : 8);
        }
        if (lane == 0) {
            a.actions_out[out_index] = ia;
            a.psel_out[out_index] = psel;
        }
        sampled = ia;
    }
    if (TAIL == FwdTail::Greedy) {
        // greedy: the lowest action index among those with the largest p, Julia's argmax.  No Philox call, no walk.
        // Per lane the first maximum in index order (tile, then i: strictly greater replaces), then a butterfly over the 32 lanes
        // of a half on the pair (p, index) in which equal p keeps the lower index -- both halves hold the same p, so every lane
        // ends with the winner.  p >= 0 or NaN (a state without an active quad: 0 / 0): NaN never replaces, the result is then
        // action 0 with p_sel NaN in every lane and flag bit 8, as the sampled tail leaves such a state
        float bp = -1.0f;
        int bi = 0;
#pragma unroll
        for (int ts = 0; ts < TPS; ++ts)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bool take = p[ts][i] > bp;
                bi = take ? 128 * ts + 4 * j + i : bi;
                bp = take ? p[ts][i] : bp;
            }
#define PPO_ARGMAX_STEP(OFF)                                                                   \
        {                                                                                      \
            const float op = xor_lane<OFF>(bp);                                                \
            const int oi = __float_as_int(xor_lane<OFF>(__int_as_float(bi)));                  \
            const bool take = op > bp || (op == bp && oi < bi);                                \
            bi = take ? oi : bi;                                                               \
            bp = take ? op : bp;                                                               \
        }
        PPO_ARGMAX_STEP(16) PPO_ARGMAX_STEP(8) PPO_ARGMAX_STEP(4) PPO_ARGMAX_STEP(2) PPO_ARGMAX_STEP(1)
#undef PPO_ARGMAX_STEP
        const float psel = (bp >= 0.0f) ? bp : p[0][0];
        if (lane == 0) {
            if (!(psel > 0.0f)) atomicOr(a.err, 8);
            a.actions_out[out_index] = bi;
            a.psel_out[out_index] = psel;
        }
        sampled = bi;
    }
    if (TAIL == FwdTail::Forced) {
        // teacher-forced: the action is given -- pre->ab, the caller's early fetch of a.actions[out_index], 0-based,
        // wave-uniform -- and p[action] is picked like the training tail picks p[ab]: no Philox call, no walk.  ab < 0 (an idle
        // env): probability 0.  An action on an inactive quad: the mask left it exactly 0; it is written as 0 and reported
        // in flag bit 64 (the rollout tail owns 8 and 32, the env step 1, 2 and 4, the minibatch gather 16)
        const int ab = pre->ab;
        const int abc = ab < 0 ? 0 : ab;
        float cand = 0.0f;
#pragma unroll
        for (int ts = 0; ts < TPS; ++ts)
#pragma unroll
            for (int i = 0; i < 4; ++i) cand = ((abc >> 7) == ts && (abc & 3) == i) ? p[ts][i] : cand;
        float psel = __shfl(cand, (abc & 127) >> 2);
        const bool off_quad = ab >= 0 && !((act >> (abc >> 4)) & 1u);
        if (ab < 0 || off_quad) psel = 0.0f;
        if (lane == 0) {
            if (off_quad) atomicOr(a.err, 64);
            a.actions_out[out_index] = ab;
            a.psel_out[out_index] = psel;
        }
        sampled = ab;
    }
    if (tail_steps(TAIL) && a.full_probs && h == 0) {        // every rollout step: the whole distribution, on request
#pragma unroll
        for (int ts = 0; ts < TPS; ++ts)
            reinterpret_cast<float4*>(a.full_probs)[((size_t)out_index * TPS + ts) * 32 + j] =
                make_float4(p[ts][0], p[ts][1], p[ts][2], p[ts][3]);
    }
    if (TAIL == FwdTail::Imitate) {
        // behaviour cloning: cross-entropy of the stored action, -w log pi(a|s), with Train's
        // entropy term.  pre: the caller's early fetch -- ab the 0-based action (on an active quad, Train's precondition), adv
        // the weight column's entry (1 for uniform weights); w = max(adv, 0).  log pi in the log-softmax form (l[a] - m) - log S
        // and dL/dlogit_k = (w / B_global)(p_k - [k == a]) without a division by p[a]: both stay finite where exp(l[a] - m)
        // underflows to 0, the searched action the current policy finds very unlikely.  No p_old, no clip, no ratio
        const int ab = pre->ab;
        const float w = fmaxf(pre->adv, 0.0f);
        float cand = 0.0f;
#pragma unroll
        for (int ts = 0; ts < TPS; ++ts)
#pragma unroll
            for (int i = 0; i < 4; ++i) cand = ((ab >> 7) == ts && (ab & 3) == i) ? l[ts][i] : cand;
        const float la = __shfl(cand, (ab & 127) >> 2);
        const float logp = (la - m) - logf(ssum);
        float lg[TPS][4];
        const float hl = smoothed_entropy(p, lg);
        float dpe[TPS][4], dot = 0.0f;
#pragma unroll
        for (int ts = 0; ts < TPS; ++ts)
#pragma unroll
            for (int i = 0; i < 4; ++i) { dpe[ts][i] = a.c_over_B * (lg[ts][i] + 1.0f); dot += p[ts][i] * dpe[ts][i]; }
        dot = wave32_sum(dot);
        const float wB = w * a.inv_B;
        if (h == 0) {
#pragma unroll
            for (int ts = 0; ts < TPS; ++ts) {
                float dy[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float pd = (128 * ts + 4 * j + i == ab) ? p[ts][i] - 1.0f : p[ts][i];       // p_k - [k == a]
                    dy[i] = dy_round<DYBF16>(wB * pd + p[ts][i] * (dpe[ts][i] - dot));
                }
                a.dY[((size_t)state * TPS + ts) * 32 + j] = make_float4(dy[0], dy[1], dy[2], dy[3]);
            }
        }
        if (lane == 0) { a.loss_terms[state * 2] = (double)(w * logp); a.loss_terms[state * 2 + 1] = (double)(-hl); }
    }
    if (TAIL == FwdTail::Distill) {
        // policy distillation: cross-entropy against a target distribution q over the state's actions,
        // -w sum_k q'_k log pi(k|s), with Train's entropy term.  q' = q on the rows of active quads and 0 elsewhere (mass on an
        // inactive row is ignored); Qs = sum q' in the softmax's own reduction order, used as it is: an unnormalised row, or one
        // that lost mass to the mask, gets the exact gradient of the loss as stated.  log pi in the log-softmax form
        // (l_k - m) - log S, a term with q'_k == 0 contributing exactly 0 (selected, not multiplied), and
        // dL/dlogit_k = (w / B_global)(p_k Qs - q'_k): nothing divides by a probability, so a target on an action whose
        // exp(l - m) underflows keeps a finite loss and gradient.  A one-hot row is Imitate term for term (Qs == 1)
        const float w = fmaxf(pre->adv, 0.0f);
        float q[TPS][4];
        float qs = 0.0f;
#pragma unroll
        for (int ts = 0; ts < TPS; ++ts) {
            const float4 v = qrow[ts];
            q[ts][0] = on[ts] ? v.x : 0.0f; q[ts][1] = on[ts] ? v.y : 0.0f;
            q[ts][2] = on[ts] ? v.z : 0.0f; q[ts][3] = on[ts] ? v.w : 0.0f;
            const float st = ((q[ts][0] + q[ts][1]) + q[ts][2]) + q[ts][3];
            qs = (ts == 0) ? st : qs + st;                   // tile partials in tile order, then the butterfly
        }
        qs = wave32_sum(qs);
        const float ls = logf(ssum);
        float ce = 0.0f;
#pragma unroll
        for (int ts = 0; ts < TPS; ++ts) {
            float t[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) t[i] = (q[ts][i] == 0.0f) ? 0.0f : q[ts][i] * ((l[ts][i] - m) - ls);
            const float st = ((t[0] + t[1]) + t[2]) + t[3];
            ce = (ts == 0) ? st : ce + st;
        }
        ce = wave32_sum(ce);
        float lg[TPS][4];
        const float hl = smoothed_entropy(p, lg);
        float dpe[TPS][4], dot = 0.0f;
#pragma unroll
        for (int ts = 0; ts < TPS; ++ts)
#pragma unroll
            for (int i = 0; i < 4; ++i) { dpe[ts][i] = a.c_over_B * (lg[ts][i] + 1.0f); dot += p[ts][i] * dpe[ts][i]; }
        dot = wave32_sum(dot);
        const float wB = w * a.inv_B;
        if (h == 0) {
#pragma unroll
            for (int ts = 0; ts < TPS; ++ts) {
                float dy[4];
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    dy[i] = dy_round<DYBF16>(wB * (p[ts][i] * qs - q[ts][i]) + p[ts][i] * (dpe[ts][i] - dot));   // p_k Qs - q'_k
                a.dY[((size_t)state * TPS + ts) * 32 + j] = make_float4(dy[0], dy[1], dy[2], dy[3]);
            }
        }
        if (lane == 0) { a.loss_terms[state * 2] = (double)(w * ce); a.loss_terms[state * 2 + 1] = (double)(-hl); }
    }
    if (TAIL == FwdTail::TrainAnchored) {
        // KL-anchored PPO: the clipped surrogate and the entropy term of Train plus beta times Distill's
        // cross-entropy against the state's target row q -- a penalty beta KL(q' || pi) up to the targets' entropy, which has no
        // gradient.  The surrogate (gain, fp64 clip, unclipped, minval, dsel, ratio_out) is Train's term for term; q', Qs and ce
        // are Distill's with its weight w replaced by beta: betaB = (float)beta * inv_B.  Order of dL/dlogit_k:
        //     dy_k = dy_round(betaB * (p_k * Qs - q'_k) + p_k * (dp_k - dot))
        // Distill's expression with Train's second summand (dp carries dsel at k == a, dot is formed from that dp).  With an
        // advantage of 0 dsel is -0 and the line is Distill's at w = beta; with beta == 0 the first summand is a zero and the
        // line is Train's value (an exact -0 of Train's on a row of an inactive quad, where p == 0, comes out as +0).
        // kl = sum over q'_k > 0 of q'_k (log q'_k - ((l_k - m) - log S)) in fp32, the softmax's reduction order.  Nothing
        // divides by a probability: a target on an action whose exp(l - m) underflows keeps loss, gradient and kl finite
        const int ab = pre->ab;
        const float po = pre->po;
        const float adv = pre->adv;
        float cand = 0.0f;
#pragma unroll
        for (int ts = 0; ts < TPS; ++ts)
#pragma unroll
            for (int i = 0; i < 4; ++i) cand = ((ab >> 7) == ts && (ab & 3) == i) ? p[ts][i] : cand;
        const float ps = __shfl(cand, (ab & 127) >> 2);
        const float gain = ps / po * adv;
        // (opaque per-state copies of the two scalar arguments: 1 + eps, 1 - eps, (float)beta and beta / B are then formed here,
        // a handful of operations per state, instead of being hoisted out of the state loop into registers that the tile loop
        // spills -- 36 bytes of scratch per lane in the deep snapshot instantiations, as FwdMode::TrainSnap has them)
        double eps = a.eps, beta = a.beta;
        asm volatile("" : "+s"(eps), "+s"(beta));
        const double clip = adv >= 0.0f ? (1.0 + eps) * (double)adv : (1.0 - eps) * (double)adv;
        const bool unclipped = (double)gain < clip;
        const double minval = unclipped ? (double)gain : clip;
        float q[TPS][4];
        float qs = 0.0f;
#pragma unroll
        for (int ts = 0; ts < TPS; ++ts) {
            const float4 v = qrow[ts];
            q[ts][0] = on[ts] ? v.x : 0.0f; q[ts][1] = on[ts] ? v.y : 0.0f;
            q[ts][2] = on[ts] ? v.z : 0.0f; q[ts][3] = on[ts] ? v.w : 0.0f;
            const float st = ((q[ts][0] + q[ts][1]) + q[ts][2]) + q[ts][3];
            qs = (ts == 0) ? st : qs + st;                   // tile partials in tile order, then the butterfly
        }
        qs = wave32_sum(qs);
        const float ls = logf(ssum);
        float ce = 0.0f, kl = 0.0f;
#pragma unroll
        for (int ts = 0; ts < TPS; ++ts) {
            float t[4], u[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float lp = (l[ts][i] - m) - ls;
                t[i] = (q[ts][i] == 0.0f) ? 0.0f : q[ts][i] * lp;
                u[i] = (q[ts][i] > 0.0f) ? q[ts][i] * (logf(q[ts][i]) - lp) : 0.0f;
            }
            const float st = ((t[0] + t[1]) + t[2]) + t[3];
            const float su = ((u[0] + u[1]) + u[2]) + u[3];
            ce = (ts == 0) ? st : ce + st;
            kl = (ts == 0) ? su : kl + su;
        }
        ce = wave32_sum(ce);
        kl = wave32_sum(kl);
        float lg[TPS][4];
        const float hl = smoothed_entropy(p, lg);
        float dp[TPS][4], dot = 0.0f;
        const float dsel = unclipped ? -(a.inv_B * adv / po) : 0.0f;
#pragma unroll
        for (int ts = 0; ts < TPS; ++ts)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                dp[ts][i] = a.c_over_B * (lg[ts][i] + 1.0f) + ((128 * ts + 4 * j + i == ab) ? dsel : 0.0f);
                dot += p[ts][i] * dp[ts][i];
            }
        dot = wave32_sum(dot);
        const float beta_f = (float)beta;
        const float betaB = beta_f * a.inv_B;
        if (h == 0) {
#pragma unroll
            for (int ts = 0; ts < TPS; ++ts) {
                float dy[4];
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    dy[i] = dy_round<DYBF16>(betaB * (p[ts][i] * qs - q[ts][i]) + p[ts][i] * (dp[ts][i] - dot));
                a.dY[((size_t)state * TPS + ts) * 32 + j] = make_float4(dy[0], dy[1], dy[2], dy[3]);
            }
        }
        if (lane == 0) {
            a.loss_terms[state * 2] = minval + (double)(beta_f * ce); a.loss_terms[state * 2 + 1] = (double)(-hl);
            if (a.ratio_out) a.ratio_out[state] = ps / po;
            if (a.anchor_out) a.anchor_out[state] = kl;
        }
    }
    if (TAIL == FwdTail::Train) {
        const int ab = pre ? pre->ab : a.actions[sid];
        const float po = pre ? pre->po : a.p_old[sid];
        const float adv = pre ? pre->adv : a.adv[sid];
        float cand = 0.0f;
#pragma unroll
        for (int ts = 0; ts < TPS; ++ts)
#pragma unroll
            for (int i = 0; i < 4; ++i) cand = ((ab >> 7) == ts && (ab & 3) == i) ? p[ts][i] : cand;
        const float ps = __shfl(cand, (ab & 127) >> 2);
        const float gain = ps / po * adv;                                    // src/train.jl:39 (Float32)
        const double clip = adv >= 0.0f ? (1.0 + a.eps) * (double)adv : (1.0 - a.eps) * (double)adv;   // :1-7
        const bool unclipped = (double)gain < clip;
        const double minval = unclipped ? (double)gain : clip;
        float lg[TPS][4];
        const float hl = smoothed_entropy(p, lg);
        float dp[TPS][4], dot = 0.0f;
        const float dsel = unclipped ? -(a.inv_B * adv / po) : 0.0f;
#pragma unroll
        for (int ts = 0; ts < TPS; ++ts)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                dp[ts][i] = a.c_over_B * (lg[ts][i] + 1.0f) + ((128 * ts + 4 * j + i == ab) ? dsel : 0.0f);
                dot += p[ts][i] * dp[ts][i];
            }
        dot = wave32_sum(dot);
        if (h == 0) {
#pragma unroll
            for (int ts = 0; ts < TPS; ++ts) {
                const float4 dyv =
                    make_float4(dy_round<DYBF16>(p[ts][0] * (dp[ts][0] - dot)), dy_round<DYBF16>(p[ts][1] * (dp[ts][1] - dot)),
                                dy_round<DYBF16>(p[ts][2] * (dp[ts][2] - dot)), dy_round<DYBF16>(p[ts][3] * (dp[ts][3] - dot)));
                a.dY[((size_t)state * TPS + ts) * 32 + j] = dyv;
                if (TPS == 1 && dy_copy) dy_copy[j] = dyv;
            }
        }
        if (lane == 0) {
            a.loss_terms[state * 2] = minval; a.loss_terms[state * 2 + 1] = (double)(-hl);
            if (a.ratio_out) a.ratio_out[state] = ps / po;                   // the quotient inside `gain`
        }
    }
    return sampled;
}

// ---- critic: the same MLP read as a state value.  V(s) = mean of the 4 outputs of every half-edge row of an ACTIVE quad
// (the rows policy_tail's mask keeps), 0 for a state without one; loss = Flux.mse(V, target) over the global minibatch.
// ValuePredict:     values_out[out_index] = V.
// ValueTrain:       dY = dL/dy = 2 (V - target) / (B_global * n) on the n = 16 * active-quads outputs of active rows, exactly
//                    0.0f on the others; loss_terms[state] = (-(V - target)^2, 0) -- the slab reduction's -(sum)/B_global
//                    then leaves the mse where the policy's ppo loss goes.  target: the caller's early fetch (TailPre rule).
// ValueTrainClip (chosen by the host while a value clip is set): the loss is PPO's clipped value loss
//                    max((V - t)^2, (Vclip - t)^2), Vclip = vold + clamp(V - vold, -c, c), c = a.vclip, vold = the caller's
//                    early fetch of a.vold[transition]: whether V left the range is decided on delta = V - vold itself
//                    (vold + clamp(delta) need not reproduce V in fp32), a tie of the two squares keeps the unclipped one,
//                    and a state whose clipped square is the larger one has dY exactly 0.0f on every row.  c = +inf: every
//                    state is inside, the plain mse bit for bit.  a.vdelta_out (optional): delta per state of the minibatch.
// A handful of adds, one division and the DPP butterfly: no exp / log, so the tail is short serial time for the workgroup.
template <FwdTail TAIL, int TPS>
__device__ __forceinline__ void value_tail(const FwdArgs& a, const int64_t state, const uint32_t act, const float (&l)[TPS][4],
                                           const int lane, const int j, const int h, const int64_t out_index, const float target,
                                           const float vold = 0.0f) {
    static_assert(tail_value(TAIL), "the policy's tails are policy_tail's");
    constexpr bool CLIP = TAIL == FwdTail::ValueTrainClip;
    bool on[TPS];
    float s = 0.0f;
#pragma unroll
    for (int ts = 0; ts < TPS; ++ts) {
        on[ts] = (act >> (8 * ts + (j >> 2))) & 1u;
        const float st = on[ts] ? ((l[ts][0] + l[ts][1]) + l[ts][2]) + l[ts][3] : 0.0f;
        s = (ts == 0) ? st : s + st;                       // tile partials in tile order, then the butterfly
    }
    s = wave32_sum(s);
    const uint32_t quads = (TPS == 4) ? act : (act & ((1u << (8 * TPS)) - 1u));
    const int nq = __builtin_popcount(quads);              // wave-uniform
    const float n = (float)(16 * nq);                      // 4 rows per quad x 4 outputs per row
    const float v = nq ? s / n : 0.0f;
    if (TAIL == FwdTail::ValuePredict) {
        if (lane == 0) a.values_out[out_index] = v;
    } else {
        const float d = v - target;
        float term = d, delta = 0.0f;
        bool keep = true;
        if (CLIP) {
            const float c = a.vclip;
            delta = v - vold;
            const bool inside = fabsf(delta) <= c;
            const float vc = vold + copysignf(c, delta);   // used only when !inside
            const float dc = vc - target;
            keep = inside || fabsf(d) >= fabsf(dc);        // the unclipped square is the larger one; a tie keeps it
            term = keep ? d : dc;
        }
        const float g = (nq && keep) ? ((2.0f * d) * a.inv_B) / n : 0.0f;
        if (h == 0) {
#pragma unroll
            for (int ts = 0; ts < TPS; ++ts) {
                const float gi = on[ts] ? g : 0.0f;
                a.dY[((size_t)state * TPS + ts) * 32 + j] = make_float4(gi, gi, gi, gi);
            }
        }
        if (lane == 0) {
            a.loss_terms[state * 2] = -((double)term * (double)term); a.loss_terms[state * 2 + 1] = 0.0;
            if (CLIP && a.vdelta_out) a.vdelta_out[state] = delta;
        }
    }
}
