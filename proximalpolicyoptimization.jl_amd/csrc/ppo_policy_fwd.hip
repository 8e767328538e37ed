// ppo_policy_fwd.hip -- K2/K3/K4 (rollout) and K8/K9/K10 (train forward + loss + dlogits).
//
// Reference: action_probabilities / batch_action_probabilities (test/quad_game_utilities.jl:65-79)
// over SimplePolicy (test/policy.jl:9-31): per half-edge MLP F -> HID -> HID -> 4 (leakyrelu 0.01),
// vec, + mask, softmax; rand(Categorical) + ap[a] > 0 (src/collect_rollouts.jl:5-7); loss
// src/train.jl:35-46.
//
// gfx950 mapping: one wave owns one state = 32 half-edge rows.  The transposed product
// Y^T = W * X^T puts the rows on the MFMA lane axis (B operand, D columns) and the features on the
// accumulator-register axis, so the 32x32 accumulator tiles of layer 1 ARE the B operands of
// layer 2 with no LDS round trip or lane movement (v_mfma_f32_32x32x2_f32, exact fp32).  Weights
// stream as A operands from HBM/L2 in a pre-packed fragment order (1 KiB contiguous per wave
// load).  The 128 logits of a state live 4-per-lane, so masked softmax and the entropy/loss
// reductions are wave shuffles; the categorical sample is the reference's sequential fp32 CDF walk
// (bit-exact action indices).  Two waves per SIMD (<=256 VGPRs) hide the weight-load latency.
//
// MFMA-bound: 2*(F*HID + HID*HID)*32 flop per state on the matrix pipe; layer 3 (HID x 4) is a VALU
// dot-product epilogue.
#include "ppo_policy_tail.h"
#include "ppo_env_device.h"
#include <cstdlib>

// Non-temporal stores for the 268 MB of activations the train forward saves: they are written once and read once by the
// backward kernel much later, so they should not churn the L2; measured -4 % on the train forward (A/B in one process).
static __device__ __forceinline__ void act_store_nt(float4* p, float4 v) {
    f32x4 t = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(t, reinterpret_cast<f32x4*>(p));
}

// waves per SIMD: the HID=256 / F=216 instantiations need more than 256 VGPRs (128 for the layer-1
// accumulators + operands in flight), so they run one wave per SIMD with the whole 512-entry file.
// HID = 128, F = 72: two waves per SIMD with the deep (16-group) ring in the train forward.  Re-measured in round 2
// (train forward / 128-step rollout): 2 waves + 16 groups 0.0685 ms / 8.34 ms; 2 + 8: 0.0817 / 8.37;
// 3 waves + 4 groups: 0.0717 / 8.87 (the rollout instantiation spills at 168 registers); 3 + 8: 0.0889 / 8.88.
// k_policy_fwd's MODE: FwdMode, and the table fwd_traits from a mode to its state source and its tail (ppo_internal.h)

template <int F, int HID>
struct FwdCfg { static constexpr int WPS = (HID >= 256 || F > 128) ? 1 : 2; };

// FwdTail::Distill: whether an instantiation holds the state's target row (4 * TPS registers) across the tile loop.  Every one
// does without scratch but the deep HID = 128 forward of Q = 32 rows at two waves per SIMD with the 16-group ring (24 bytes per
// lane with the early fetch): that one fetches the row behind the loop.  (Its snapshot sibling runs the 8-group ring and fits.)
constexpr bool distill_row_early(int F, int HID, int TPS, int DEEP, bool SNAP) {
    return !(F == 72 && HID == 128 && TPS == 4 && DEEP && !SNAP);
}

// FwdTail::TrainAnchored: the same question for the anchored train forward, which holds TailPre's three inputs
// beside the row.  DESIGN.md 7r lists which instantiation got which
constexpr bool anchor_row_early(int F, int HID, int TPS, int DEEP, bool SNAP) {
    return distill_row_early(F, HID, TPS, DEEP, SNAP);      // the same one instantiation: 20 bytes per lane with the early fetch
}
// ... and whether TailPre's three inputs are fetched ahead of the activation stores too (else behind the loop, like the row)
constexpr bool anchor_pre_early(int F, int HID, int TPS, int DEEP, bool SNAP) { return anchor_row_early(F, HID, TPS, DEEP, SNAP); }

// TPS = 32-row tiles per state (H = 32*TPS half-edges, A = 128*TPS actions): the wave walks the tiles of its
// state one after the other, keeps the 4*TPS logits per lane, and runs softmax / sampling / loss once per state.
// DEEP = 1: Policy(F, HID, num_hidden_layers != 2, 4) (test/policy.jl:9-19).  The hidden->hidden block becomes a loop over
// a.nl2 layers: the output tiles of every layer but the last are parked in a wave-private LDS region (lane-linear 1 KiB
// rows, no barrier: only the wave itself reads them back) and re-loaded as the next layer's B operands; the last one feeds
// the layer-3 dot epilogue as before (nl2 == 0: the dot runs on the layer-1 tiles).  Every layer walks its contraction in
// the same accumulator-register order as layer 2, so the fp32 chain order per layer is the one the oracle's device-order
// mode mirrors.  DEEP = 0 is the num_hidden_layers == 2 kernel, unchanged.  The persistent rollout has no deep form:
// its env slots and the park would share the LDS; deep policies roll out with the per-step launches.
template <int F, int HID, FwdMode MODE, int TPS, int DEEP = 0>
__global__ __launch_bounds__(256, (FwdCfg<F, HID>::WPS)) void k_policy_fwd(FwdArgs a) {
    constexpr int NT = HID / 32;       // 32-feature tiles
    constexpr int S41 = F / 8;         // float4 groups of layer-1 k-steps
    constexpr int XB = F / 2;          // bytes of the state row held by one lane
    constexpr int XW = XB / 4;
    constexpr int PFW = 16;            // the deep ring of weight-fragment groups: at most the groups of one output tile
    static_assert(PFW <= HID / 8, "the deep ring is one output tile's groups at the most");
    constexpr FwdSource SRC = fwd_traits(MODE).src;
    constexpr FwdTail TAIL = fwd_traits(MODE).tail;
    constexpr bool TRAIN = tail_trains(TAIL);           // train forward: saves activations, loss tail
    constexpr bool VALUE = tail_value(TAIL);            // critic: value_tail
    constexpr bool IMITATE = TAIL == FwdTail::Imitate;
    constexpr bool DISTILL = TAIL == FwdTail::Distill;
    constexpr bool ANCHOR = TAIL == FwdTail::TrainAnchored;
    constexpr bool QROW = DISTILL || ANCHOR;                // the tails that read a target row per state
    constexpr bool GATHER = SRC == FwdSource::RowsIdx;
    constexpr bool SNAP = src_snapshot(SRC), SNAPX = SRC == FwdSource::SnapIdx;
    constexpr bool PERSIST = SRC == FwdSource::EnvSlots;    // persistent rollout: T steps of the wave's envs, their state in LDS slots
    // two waves per SIMD (HID = 128, F = 72): 4 groups cover the L2 latency; the train forward, whose activation stores
    // sit in the same vmcnt queue, wants the deep ring here too (0.072 -> 0.069 ms), the rollout does not (8.3 -> 8.7 ms)
    // (value-train from snapshots keeps half the train ring at two waves per SIMD: with 16 groups next to the row
    // re-derivation it does not fit the 256 registers)
    constexpr int PFV = PFW / 2;
    // (the imitation forward from snapshots likewise: with 16 groups ImitateSnap spills where TrainSnap does, 196 / 60 / 116 bytes per lane)
    // (the distillation forward from snapshots takes the same ring: ImitateSnap's registers plus the target row)
    // (the anchored forward from snapshots likewise: DistillSnap's registers plus TailPre's)
    constexpr int PF = (FwdCfg<F, HID>::WPS == 1) ? PFW : (TRAIN ? (((VALUE || IMITATE || QROW) && SNAP) ? PFV : PFW) : 4);   // weight-fragment groups kept in flight per wave
    // distillation: the state's target row (TPS float4 per lane) is fetched in front of the tile loop, ahead of the activation
    // stores like TailPre, where holding it across the loop costs no scratch; else behind the loop, paying the wait for the
    // stores queued in front of it (vmcnt is one in-order queue).  DESIGN.md 7q lists which instantiation got which
    constexpr bool QPRE = (DISTILL && distill_row_early(F, HID, TPS, DEEP, SNAP)) || (ANCHOR && anchor_row_early(F, HID, TPS, DEEP, SNAP));
    constexpr bool OBS = (PERSIST || SNAP);             // the state rows are re-derived from an env snapshot in LDS
    static_assert(F % 8 == 0 && HID % 32 == 0, "shape");
    static_assert(PF * 64 * 4 <= PPO_PACK_PAD, "the ring reads PF groups past the end of a packed weight stream: padding must cover it");
    const int lane = threadIdx.x & 63;
    const int j = lane & 31;           // half-edge row inside the tile
    const int h = lane >> 5;           // lane half = k parity of the MFMA step
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * 4;

    // W3 fragments and the two bias packs are read once per output tile by every wave: staged in LDS once per
    // workgroup so the per-tile epilogues see an LDS round trip instead of a global (L1/L2) one
    __shared__ __attribute__((aligned(16))) float4 sW3[2 * NT * 16];     // [half][tile][reg]  (HID*4 floats)
    __shared__ __attribute__((aligned(16))) float4 sB1[NT * 2 * 4];      // [tile][half][4]    (HID floats)
    constexpr int NB2L = DEEP ? 3 : 1;                                   // bias packs of up to three hidden->hidden layers
    __shared__ __attribute__((aligned(16))) float4 sB2[NB2L * NT * 2 * 4];
    static_assert(!(DEEP && PERSIST), "no deep persistent rollout");
    for (int i = threadIdx.x; i < 2 * NT * 16; i += 256) sW3[i] = a.w3p[i];
    for (int i = threadIdx.x; i < NT * 8; i += 256) sB1[i] = a.b1p[i];
    for (int i = threadIdx.x; i < NT * 8 * (DEEP ? a.nl2 : 1); i += 256) sB2[i] = a.b2p[i];
    __syncthreads();

    // the rows of the NEXT 32-row tile are fetched while the current one computes (the gather through idx is two
    // dependent HBM round trips that one wave per SIMD cannot hide otherwise)
    constexpr bool PFX = (FwdCfg<F, HID>::WPS == 1) && !OBS;      // with two waves per SIMD the partner wave hides it instead;
                                                                  // OBS: the wave computes the rows itself (no fetch)
    uint32_t xw[XW];
    auto fetch_rows = [&](int64_t state, int ts) {
        const int64_t sidn = GATHER ? (int64_t)a.idx[state] : state;
        const uint32_t* xr = reinterpret_cast<const uint32_t*>(a.states + ((size_t)sidn * TPS + ts) * 32 * F +
                                                               (size_t)j * F + (size_t)h * XB);
#pragma unroll
        for (int k = 0; k < XW; ++k) xw[k] = xr[k];
    };
    if (PFX && wave < a.B) fetch_rows(wave, 0);

#ifdef PPO_FWD_STAMP
    unsigned long long st_sum[6] = {0, 0, 0, 0, 0, 0}, st_t = clock64();
#define FSTAMP(i) do { unsigned long long _n = clock64(); st_sum[i] += _n - st_t; st_t = _n; } while (0)
#else
#define FSTAMP(i) do {} while (0)
#endif
    // ---- PERSIST: persistent rollout.  Envs are independent, so every wave walks ITS envs (state = wave, wave + nwaves,
    // ...) through all T steps without any grid-wide synchronisation: observe -> MLP -> sample -> step!, with the env
    // state (scores, degrees, counters) resident in the wave's LDS slots and written back once at the end.
    extern __shared__ __attribute__((aligned(16))) char env_lds[];
    const int slot_bytes = 2 * a.envV + 32;
    char* const my_slots = env_lds + (size_t)(threadIdx.x >> 6) * a.env_slots * slot_bytes;
    EnvConst ec;
    auto slot_ref = [&](int slot) {                               // LDS-typed pointers: ds_* instead of flat_* accesses
        PPO_LDS char* b = (PPO_LDS char*)(my_slots + (size_t)slot * slot_bytes);
        EnvRefLds r;
        r.sc = (PPO_LDS int8_t*)b; r.dg = r.sc + a.envV;
        PPO_LDS uint32_t* w = (PPO_LDS uint32_t*)(b + 2 * a.envV);
        r.active = w; r.steps = (PPO_LDS int32_t*)(w + 1); r.reward = (PPO_LDS float*)(w + 2);
        r.done = (PPO_LDS uint8_t*)(w + 3); r.episode = w + 4; r.tick = w + 5;
        return r;
    };
    if (PERSIST) {
        ec.Q = a.envQ; ec.V = a.envV; ec.max_actions = a.env_max_actions; ec.no_action_reward = a.env_nar; ec.k0 = a.k0; ec.k1 = a.k1;
        int slot = 0;
        for (int64_t n = wave; n < a.B; n += nwaves, ++slot) {
            const EnvRefLds r = slot_ref(slot);
            for (int v = lane; v < a.envV; v += 64) { r.sc[v] = a.env_score[n * a.envV + v]; r.dg[v] = a.env_degree[n * a.envV + v]; }
            if (lane == 0) {
                *r.active = a.env_active[n]; *r.steps = a.env_steps[n]; *r.reward = a.env_reward[n];
                *(PPO_LDS uint32_t*)r.done = a.env_done[n]; *r.episode = a.env_episode[n]; *r.tick = a.env_tick[n];
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // slots are wave-private: program order + in-order LDS suffice
    }
    uint32_t tmpl_regs[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};       // OBS, TPS == 1: this lane's 36 template vertex ids
    if (OBS && TPS == 1) {
        const uint32_t* tp = reinterpret_cast<const uint32_t*>(a.env_tmpl + j * PPO_TPL);
#pragma unroll
        for (int k = 0; k < 9; ++k) tmpl_regs[k] = tp[k];
    }
    // SNAP: the env snapshot of a state (2V bytes + the active-quad word) is fetched (SNAPX: through idx) one state ahead
    // (two dependent HBM round trips) into registers and parked in the wave's LDS slot at the top of its state
    // (one dword per lane: 2V/4 <= 64 dwords for V <= 128)
    uint32_t cs_next = 0u, act_next = 0u;
    int32_t sid_next = 0;
    auto fetch_snapshot = [&](int64_t state) {
        sid_next = SNAPX ? a.idx[state] : (int32_t)state;
        act_next = a.active[sid_next];
        const int nd = a.envV >> 1;                              // dwords of one snapshot
        cs_next = (lane < nd) ? reinterpret_cast<const uint32_t*>(a.cstate)[(size_t)sid_next * nd + lane] : 0u;
    };
    if (SNAP && wave < a.B) fetch_snapshot(wave);
    const int64_t t_steps = PERSIST ? a.T : 1;
    for (int64_t tt = 0; tt < t_steps; ++tt) {
    int slot = 0;
    for (int64_t state = wave; state < a.B; state += nwaves, ++slot) {
        const int64_t sid = GATHER ? (int64_t)a.idx[state] : (SNAP ? (int64_t)sid_next : state);
        EnvRefLds er = {};
        if (PERSIST) er = slot_ref(slot);
        if (SNAP) {
            er = slot_ref(0);
            if (lane < (a.envV >> 1)) reinterpret_cast<PPO_LDS uint32_t*>(er.sc)[lane] = cs_next;
            if (lane == 0) *er.active = act_next;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // wave-private slot: program order + in-order LDS suffice
        }
        const uint32_t act = PERSIST ? *er.active : (SNAP ? act_next : a.active[sid]);
        // value-train: the target is fetched here, ahead of the activation stores it would otherwise queue behind (vmcnt)
        float vtarget = 0.0f, vold = 0.0f;
        if (VALUE && TRAIN) vtarget = a.vtarget[sid];
        if (TAIL == FwdTail::ValueTrainClip) vold = a.vold[sid];                  // clipped value loss: the old value, likewise
        if (SNAP) fetch_snapshot(state + nwaves < a.B ? state + nwaves : state);      // lands under this state's MFMAs
        const uint32_t tick_val = PERSIST ? *er.tick : (tail_samples(TAIL) ? a.tick[state] : 0u);
        const int64_t out_index = PERSIST ? tt * a.B + state : state;
        // teacher-forced step: the state's given action, fetched here like the tick so that it has landed by the tail
        [[maybe_unused]] TailPre forced = {0, 0.0f, 0.0f};
        if constexpr (TAIL == FwdTail::Forced) forced.ab = a.actions[state];
        // imitation: the stored action and its weight (a.adv == nullptr: uniform), ahead of the activation stores like vtarget
        if constexpr (IMITATE) { forced.ab = a.actions[sid]; forced.adv = a.adv ? a.adv[sid] : 1.0f; }
        // distillation: the weight likewise, and the target row: TPS coalesced float4 loads per lane (both lane halves read the
        // same 512 B of a tile, as both hold the same logits)
        // the anchored train forward: Train's three inputs ahead of the activation stores (TailPre), and the target row likewise
        [[maybe_unused]] float4 qrow[QROW ? TPS : 1];
        [[maybe_unused]] const float4* qsrc = nullptr;
        constexpr bool APRE = ANCHOR && anchor_pre_early(F, HID, TPS, DEEP, SNAP);
        if constexpr (APRE) { forced.ab = a.actions[sid]; forced.po = a.p_old[sid]; forced.adv = a.adv[sid]; }
        if constexpr (DISTILL) forced.adv = a.adv ? a.adv[sid] : 1.0f;
        if constexpr (QROW) {
            qsrc = reinterpret_cast<const float4*>(a.targets) + (size_t)sid * (32 * TPS) + j;
            if constexpr (QPRE) {
#pragma unroll
                for (int ts = 0; ts < TPS; ++ts) qrow[ts] = qsrc[ts * 32];
            }
        }
        float l[TPS][4];
        // multi-tile states: the tile loop stays a real loop (no 4x code blow-up, no cross-tile hoisting that
        // would spill); the 4 logits per lane of each tile are parked in LDS and re-read after the loop
        __shared__ float4 sL[(TPS > 1) ? 4 * TPS * 64 : 1];

#pragma unroll 1
        for (int ts = 0; ts < TPS; ++ts) {
            const int64_t tile = state * TPS + ts;
            // per-tile opaque lane offsets: the weight/bias fragment loads below must be re-issued for every tile
            // (they are L2 hits); without this LICM hoists ~330 loop-invariant float4 loads out of the tile loop
            int lane_o = lane, half_o = h;
            asm volatile("" : "+v"(lane_o), "+v"(half_o));
            // ---- state rows -> B operands of layer 1: lane half 0 holds features [0,F/2), half 1 [F/2,F)
            if (OBS) {
                // state(env): this lane's 36 features of half-edge row 32*ts + j, recorded into the rollout buffer
                // (PERSIST, expanded storage) or into the minibatch-ordered row scratch the backward reads (SNAPX)
                static_assert(!OBS || XW == 9, "the built-in env has F = 72 features");
                uint32_t ob[9], tid[9];
                if (TPS == 1) {
#pragma unroll
                    for (int k = 0; k < 9; ++k) tid[k] = tmpl_regs[k];          // row j's ids, loaded once per kernel
                } else {
                    const uint32_t* tp = reinterpret_cast<const uint32_t*>(a.env_tmpl + (32 * ts + j) * PPO_TPL);
#pragma unroll
                    for (int k = 0; k < 9; ++k) tid[k] = tp[k];
                }
                env_observe_lane(er, tid, 32 * ts + j, h, ob);
#pragma unroll
                for (int k = 0; k < XW; ++k) xw[k] = ob[k < 9 ? k : 0];
                int8_t* const rows_out = SNAPX ? a.xs_out : (PERSIST ? a.states_out : nullptr);
                if (rows_out) {                                  // wave-uniform
                    uint32_t* so = reinterpret_cast<uint32_t*>(rows_out + ((size_t)(SNAPX ? state : out_index) * TPS + ts) * 32 * F +
                                                               (size_t)j * F + (size_t)h * XB);
#pragma unroll
                    for (int k = 0; k < XW; ++k) so[k] = xw[k];
                }
                if (PERSIST && ts == 0 && a.cstate_out && lane < (a.envV >> 1))      // compact storage: the env snapshot itself
                    reinterpret_cast<uint32_t*>(a.cstate_out)[(size_t)out_index * (a.envV >> 1) + lane] =
                        reinterpret_cast<PPO_LDS uint32_t*>(er.sc)[lane];
            } else if (!PFX) fetch_rows(state, ts);
            float xf[XB];
#pragma unroll
            for (int k = 0; k < XW; ++k) {
#pragma unroll
                for (int i = 0; i < 4; ++i) xf[4 * k + i] = (float)(int)(int8_t)(xw[k] >> (8 * i));
            }
            if (PFX) {                                          // unconditional: lands under the MFMA chains below
                if (ts + 1 < TPS) fetch_rows(state, ts + 1);
                else fetch_rows(state + nwaves < a.B ? state + nwaves : state, 0);
            }

            FSTAMP(0);
            // ---- layer 1: H1^T[o-tile] = W1[o-tile,:] * X^T  (accumulator initialised with the bias)
            // The weight stream of a layer is one linear run of 1 KiB fragment groups (4 MFMA k-steps each);
            // a PF-deep register ring keeps PF groups in flight so the single wave of a SIMD never waits on L2.
            f32x16 h1[NT];
            {
                const float4* wp = a.w1p + lane_o;
                float4 ring[PF];
#pragma unroll
                for (int g = 0; g < PF; ++g) ring[g] = wp[(size_t)g * 64];
#pragma unroll
                for (int o = 0; o < NT; ++o) {
                    f32x16 acc;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float4 b = sB1[(o * 2 + half_o) * 4 + q];
                        acc[4 * q + 0] = b.x; acc[4 * q + 1] = b.y; acc[4 * q + 2] = b.z; acc[4 * q + 3] = b.w;
                    }
#pragma unroll
                    for (int s4 = 0; s4 < S41; ++s4) {
                        const int g = o * S41 + s4;
                        const float4 w = ring[g % PF];
                        ring[g % PF] = wp[(size_t)(g + PF) * 64];      // the packed buffers carry tail padding
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, xf[4 * s4 + 0], acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, xf[4 * s4 + 1], acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.z, xf[4 * s4 + 2], acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.w, xf[4 * s4 + 3], acc, 0, 0, 0);
                    }
                    // the epilogue reads the tile with VALU instructions: ask for VGPRs (hipcc otherwise parks the
                    // accumulator in AGPRs and copies it out with 16 v_accvgpr_read per tile)
                    asm volatile("" : "+v"(acc));
                    lrelu16(acc);
                    h1[o] = acc;
                    if (TRAIN) {
                        float4* dst = a.act1 + ((size_t)tile * NT + o) * 4 * 64;
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            act_store_nt(dst + q * 64 + lane, make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]));
                    }
                }
            }

            FSTAMP(1);
            // ---- layer 2 (MFMA, B operands = layer-1 accumulators) + layer 3 (VALU dot epilogue)
            float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
            if constexpr (DEEP) {
                constexpr int S42 = NT * 4;
                static_assert(S42 % PF == 0, "ring depth must divide the groups per tile");
                // this wave's park: [NT tiles][4 quarter-tiles][64 lanes] float4
                float4* const park = reinterpret_cast<float4*>(env_lds + a.park_off) + (size_t)(threadIdx.x >> 6) * NT * 256 + lane;
                const int nl2 = a.nl2;
                auto dot3 = [&](int o, const f32x16& acc) {
                    const float4* w3 = sW3 + (half_o * NT + o) * 16;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float4 w = w3[r];
                        p0 = fmaf(w.x, acc[r], p0); p1 = fmaf(w.y, acc[r], p1);
                        p2 = fmaf(w.z, acc[r], p2); p3 = fmaf(w.w, acc[r], p3);
                    }
                };
#pragma unroll 1
                for (int l = 0; l < nl2; ++l) {
                    const bool last = (l + 1 == nl2);                   // wave-uniform
                    const float4* wp = a.w2p + (size_t)l * (HID * HID / 4) + lane_o;
                    float4* const act_out = last ? a.act2 : a.act_mid[l < 2 ? l : 0];
                    float4 ring[PF];
#pragma unroll
                    for (int g = 0; g < PF; ++g) ring[g] = wp[(size_t)g * 64];
#pragma unroll 1
                    for (int o = 0; o < NT; ++o) {
                        f32x16 acc;
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const float4 b = sB2[((l * NT + o) * 2 + half_o) * 4 + q];
                            acc[4 * q + 0] = b.x; acc[4 * q + 1] = b.y; acc[4 * q + 2] = b.z; acc[4 * q + 3] = b.w;
                        }
                        const float4* wo = wp + (size_t)o * S42 * 64;
#pragma unroll
                        for (int t = 0; t < NT; ++t) {
#pragma unroll
                            for (int r4 = 0; r4 < 4; ++r4) {
                                const int s4 = t * 4 + r4;
                                const float4 w = ring[s4 % PF];
                                ring[s4 % PF] = wo[(size_t)(s4 + PF) * 64];      // the next layer's head / the tail padding
                                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, h1[t][4 * r4 + 0], acc, 0, 0, 0);
                                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, h1[t][4 * r4 + 1], acc, 0, 0, 0);
                                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.z, h1[t][4 * r4 + 2], acc, 0, 0, 0);
                                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.w, h1[t][4 * r4 + 3], acc, 0, 0, 0);
                            }
                        }
                        asm volatile("" : "+v"(acc));
                        lrelu16(acc);
                        if (TRAIN) {
                            float4* dst = act_out + ((size_t)tile * NT + o) * 4 * 64;
#pragma unroll
                            for (int q = 0; q < 4; ++q)
                                act_store_nt(dst + q * 64 + lane, make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]));
                        }
                        if (last) dot3(o, acc);
                        else {
#pragma unroll
                            for (int q = 0; q < 4; ++q)
                                park[(o * 4 + q) * 64] = make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
                        }
                    }
                    if (!last) {                                        // this layer's output becomes the next layer's input
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // wave-private: program order + in-order LDS suffice
#pragma unroll
                        for (int t = 0; t < NT; ++t)
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                const float4 v = park[(t * 4 + q) * 64];
                                h1[t][4 * q + 0] = v.x; h1[t][4 * q + 1] = v.y; h1[t][4 * q + 2] = v.z; h1[t][4 * q + 3] = v.w;
                            }
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // read back before the next layer overwrites the park
                    }
                }
                if (nl2 == 0) {                                         // num_hidden_layers == 1: layer 3 on the layer-1 tiles
#pragma unroll
                    for (int o = 0; o < NT; ++o) dot3(o, h1[o]);
                }
            } else {
                constexpr int S42 = NT * 4;                  // groups per output tile
                static_assert(S42 % PF == 0, "ring depth must divide the groups per tile");
                const float4* wp = a.w2p + lane_o;
                float4 ring[PF];
#pragma unroll
                for (int g = 0; g < PF; ++g) ring[g] = wp[(size_t)g * 64];
#pragma unroll 1
                for (int o = 0; o < NT; ++o) {
                    f32x16 acc;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float4 b = sB2[(o * 2 + half_o) * 4 + q];
                        acc[4 * q + 0] = b.x; acc[4 * q + 1] = b.y; acc[4 * q + 2] = b.z; acc[4 * q + 3] = b.w;
                    }
                    const float4* wo = wp + (size_t)o * S42 * 64;
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
#pragma unroll
                        for (int r4 = 0; r4 < 4; ++r4) {
                            const int s4 = t * 4 + r4;
                            const float4 w = ring[s4 % PF];
                            // next group PF ahead in the linear stream (tail padding covers the last tile's over-read)
                            ring[s4 % PF] = wo[(size_t)(s4 + PF) * 64];
                            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, h1[t][4 * r4 + 0], acc, 0, 0, 0);
                            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, h1[t][4 * r4 + 1], acc, 0, 0, 0);
                            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.z, h1[t][4 * r4 + 2], acc, 0, 0, 0);
                            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.w, h1[t][4 * r4 + 3], acc, 0, 0, 0);
                        }
                    }
                    FSTAMP(2);
                    asm volatile("" : "+v"(acc));
                    lrelu16(acc);
                    if (TRAIN) {
                        float4* dst = a.act2 + ((size_t)tile * NT + o) * 4 * 64;
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            act_store_nt(dst + q * 64 + lane, make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]));
                    }
                    const float4* w3 = sW3 + (half_o * NT + o) * 16;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float4 w = w3[r];
                        p0 = fmaf(w.x, acc[r], p0); p1 = fmaf(w.y, acc[r], p1);
                        p2 = fmaf(w.z, acc[r], p2); p3 = fmaf(w.w, acc[r], p3);
                    }
                    FSTAMP(3);
                }
            }
            const float l0 = (p0 + __shfl_xor(p0, 32)) + a.b3[0];
            const float l1 = (p1 + __shfl_xor(p1, 32)) + a.b3[1];
            const float l2 = (p2 + __shfl_xor(p2, 32)) + a.b3[2];
            const float l3 = (p3 + __shfl_xor(p3, 32)) + a.b3[3];
            if (TPS == 1) { l[0][0] = l0; l[0][1] = l1; l[0][2] = l2; l[0][3] = l3; }
            else sL[((threadIdx.x >> 6) * TPS + ts) * 64 + lane] = make_float4(l0, l1, l2, l3);
        }
        if (TPS > 1) {
#pragma unroll
            for (int ts = 0; ts < TPS; ++ts) {
                const float4 v = sL[((threadIdx.x >> 6) * TPS + ts) * 64 + lane];   // own lane's values: no barrier needed
                l[ts][0] = v.x; l[ts][1] = v.y; l[ts][2] = v.z; l[ts][3] = v.w;
            }
        }

        FSTAMP(4);
        int sampled = 0;
        if constexpr (VALUE) value_tail<TAIL, TPS>(a, state, act, l, lane, j, h, out_index, vtarget, vold);
        else if constexpr (QROW) {
            if constexpr (ANCHOR && !APRE) { forced.ab = a.actions[sid]; forced.po = a.p_old[sid]; forced.adv = a.adv[sid]; }
            if constexpr (!QPRE) {
#pragma unroll
                for (int ts = 0; ts < TPS; ++ts) qrow[ts] = qsrc[ts * 32];
            }
            sampled = policy_tail<TAIL, TPS, false>(a, state, sid, act, l, lane, j, h, 0u, out_index, &forced, nullptr, qrow);
        }
        else if constexpr (TAIL == FwdTail::Forced || IMITATE) sampled = policy_tail<TAIL, TPS, false>(a, state, sid, act, l, lane, j, h, 0u, out_index, &forced);
        else sampled = policy_tail<TAIL, TPS, false>(a, state, sid, act, l, lane, j, h, tick_val, out_index);
        if (PERSIST) {
            // update!: the observed mask, then step!(env, a), reward, is_terminal (src/collect_rollouts.jl:9-14) and the
            // reset! before the next episode (src/rollout_buffer.jl:75) -- one lane, on the LDS slot
            asm volatile("" ::: "memory");
            if (TPS == 1) {                                  // Q == 8: wavefront-parallel env update (one state byte per lane)
                float rew; uint8_t dn;
                // (an opaque copy of the lane id: the env update's lane constants -- vertex, array, quad -- are then
                // recomputed here instead of being hoisted out of the step loop as registers that spill)
                int lane_e = lane;
                asm volatile("" : "+v"(lane_e));
                const int errf = env_step_wave32(ec, er, sampled, lane_e, rew, dn);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (lane == 0) {
                    a.active_out[out_index] = act;
                    if (errf) atomicOr(a.err, errf);
                    a.rew_out[out_index] = rew; a.done_out[out_index] = dn;
                }
                if (dn) env_reset_wave32(ec, er, (uint32_t)(a.global_offset + state), lane_e);
            } else if (lane == 0) {
                a.active_out[out_index] = act;
                float rew; uint8_t dn;
                const int errf = env_step_ref(ec, er, sampled, rew, dn);
                if (errf) atomicOr(a.err, errf);
                a.rew_out[out_index] = rew; a.done_out[out_index] = dn;
                if (dn) env_reset_ref(ec, er, (uint32_t)(a.global_offset + state));
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        FSTAMP(5);
    }
    }
    if (PERSIST) {                                              // env state back to the [N] arrays
        int slot2 = 0;
        for (int64_t n = wave; n < a.B; n += nwaves, ++slot2) {
            const EnvRefLds r = slot_ref(slot2);
            for (int v = lane; v < a.envV; v += 64) { a.env_score[n * a.envV + v] = r.sc[v]; a.env_degree[n * a.envV + v] = r.dg[v]; }
            if (lane == 0) {
                a.env_active[n] = *r.active; a.env_steps[n] = *r.steps; a.env_reward[n] = *r.reward;
                a.env_done[n] = *r.done; a.env_episode[n] = *r.episode; a.env_tick[n] = *r.tick;
            }
        }
    }
#ifdef PPO_FWD_STAMP
    if (a.stamps && lane == 0 && wave < 1024)
        for (int i = 0; i < 6; ++i) a.stamps[wave * 6 + i] = st_sum[i];
#endif
}

// rand(Categorical) on given probabilities (parity entry point, src/collect_rollouts.jl:6-7):
// one thread per row walks the CDF sequentially in fp32.
__global__ void k_categorical(const float* __restrict__ probs, const float* __restrict__ u, int64_t B, int64_t A,
                              int32_t* __restrict__ actions, float* __restrict__ psel, int32_t* __restrict__ err) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float* p = probs + b * A;
    const float uu = u[b];
    float cp = p[0];
    int64_t i = 0;
    while (cp <= uu && i < A - 1) { i += 1; cp = cp + p[i]; }
    actions[b] = (int32_t)i;
    psel[b] = p[i];
    err[b] = !(p[i] > 0.0f);
}

// One launch of k_policy_fwd<F, HID, MODE, tps, DEEP> on persistent waves: 256 CUs x WPS blocks of 4 waves (one per SIMD).
// DEEP = 0 is the entry: num_hidden_layers == 2 launches here, every other depth the layer-looped instantiations (DEEP = 1).
// Dynamic LDS = [snapshot sources: one env-snapshot slot per wave][DEEP: the park, 4 waves x HID/32 tiles x 4 KiB]
template <FwdMode MODE, int DEEP = 0>
static int32_t dispatch_fwd(ppo_policy_s* p, const FwdArgs& args, int64_t B, int tps) {
    if constexpr (!DEEP) {
        if (p->L != 2) return dispatch_fwd<MODE, 1>(p, args, B, tps);
    }
    constexpr bool SNAP = src_snapshot(fwd_traits(MODE).src);
    const int64_t need = (B + 3) / 4;
    FwdArgs a = args;
    size_t snap = SNAP ? (size_t)4 * (2 * a.envV + 32) : 0;
    if (DEEP) {
        snap = (snap + 15) & ~(size_t)15;
        a.nl2 = p->L - 1;
        a.park_off = (uint32_t)snap;
    }
#define LAUNCH(FF, HH, TT)                                                                               \
    do {                                                                                                 \
        const int64_t cap = 256 * FwdCfg<FF, HH>::WPS;                                                   \
        const unsigned grid = (unsigned)(need < cap ? need : cap);                                       \
        if constexpr (SNAP && FF != 72) {                                                                \
            ppo_set_error("compact rollouts need the built-in env's F = 72"); return PPO_ERR_UNSUPPORTED; \
        } else {                                                                                         \
            const size_t dlds = snap + (DEEP ? (size_t)4 * (HH / 32) * 4096 : 0);                        \
            if constexpr (DEEP) {                                                                        \
                static thread_local size_t attr_lds = 0;                                                 \
                if (dlds > attr_lds) {                                                                   \
                    HIP_TRY(hipFuncSetAttribute((const void*)k_policy_fwd<FF, HH, MODE, TT, DEEP>,       \
                                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)dlds)); \
                    attr_lds = dlds;                                                                     \
                }                                                                                        \
            }                                                                                            \
            hipLaunchKernelGGL((k_policy_fwd<FF, HH, MODE, TT, DEEP>), dim3(grid), dim3(256), dlds, ppo_stream(), a); \
        }                                                                                                \
    } while (0)
    if (p->F == 72 && p->HID == 256 && tps == 1) LAUNCH(72, 256, 1);
    else if (p->F == 72 && p->HID == 256 && tps == 4) LAUNCH(72, 256, 4);
    else if (p->F == 72 && p->HID == 128 && tps == 1) LAUNCH(72, 128, 1);
    else if (p->F == 72 && p->HID == 128 && tps == 4) LAUNCH(72, 128, 4);
    else if (p->F == 216 && p->HID == 128 && tps == 1) LAUNCH(216, 128, 1);
    else if (p->F == 216 && p->HID == 256 && tps == 1) LAUNCH(216, 256, 1);
    else { ppo_set_error("unsupported policy/state shape (F,HID,H) for the gfx950 kernels"); return PPO_ERR_UNSUPPORTED; }
#undef LAUNCH
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

#ifdef PPO_FWD_STAMP
static unsigned long long* g_fwd_stamps = nullptr;
extern "C" int32_t ppo_debug_fwd_stamps(unsigned long long* out) {
    if (!g_fwd_stamps) return -1;
    (void)hipDeviceSynchronize();
    return hipMemcpy(out, g_fwd_stamps, 1024 * 6 * 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -2;
}
#endif

static void fill_weights(ppo_policy_s* p, FwdArgs& a) {
    a.stamps = nullptr;
#ifdef PPO_FWD_STAMP
    if (!g_fwd_stamps) (void)hipMalloc((void**)&g_fwd_stamps, 1024 * 6 * 8);
    a.stamps = g_fwd_stamps;
#endif
    a.w1p = (const float4*)p->w1p.p; a.w2p = (const float4*)p->w2p.p; a.b1p = (const float4*)p->b1p.p;
    a.b2p = (const float4*)p->b2p.p; a.w3p = (const float4*)p->w3p.p; a.b3 = p->b3.p;
}

// what the rollout tails take from the env: the Philox counter words and key, and where the step's outputs and flags go
static void fill_rollout(ppo_env_s* e, FwdArgs& a, int32_t* actions_out, float* psel_out, float* full_probs_or_null, int32_t* err) {
    a.tick = e->tick.p; a.global_offset = e->global_offset; a.k0 = (uint32_t)e->seed; a.k1 = (uint32_t)(e->seed >> 32);
    a.actions_out = actions_out; a.psel_out = psel_out; a.full_probs = full_probs_or_null; a.err = err;
}

int32_t launch_policy_probs(ppo_policy_s* p, const int8_t* states_dev, const uint32_t* active_dev, int64_t B,
                            int32_t H, float* probs_dev) {
    if (B <= 0) return PPO_OK;
    FwdArgs a = {};
    fill_weights(p, a);
    a.states = states_dev; a.active = active_dev; a.B = B; a.probs_out = probs_dev;
    ProfScope ps("k_policy_fwd_probs");
    if (p->dtype == PPO_DTYPE_BF16) return launch_policy_fwd_bf16(p, a, FwdMode::Probs, B, H / 32);
    return dispatch_fwd<FwdMode::Probs>(p, a, B, H / 32);
}

int32_t launch_policy_rollout(ppo_policy_s* p, ppo_env_s* e, const int8_t* states_dev, const uint32_t* active_dev,
                              int32_t* actions_out, float* psel_out, float* full_probs_or_null) {
    FwdArgs a = {};
    fill_weights(p, a);
    a.states = states_dev; a.active = active_dev; a.B = e->N;
    fill_rollout(e, a, actions_out, psel_out, full_probs_or_null, e->err.p);
    ProfScope ps("k_policy_fwd_rollout");
    if (p->dtype == PPO_DTYPE_BF16) return launch_policy_fwd_bf16(p, a, FwdMode::Sample, e->N, e->H / 32);
    if (e->N <= ppo_knobs().rollout_split_max_envs) {   // few envs: 2 or 4 waves per env, same bits
        const int32_t rs = launch_rollout_split(p, a, e->N, e->H / 32, e->V, 0);
        if (rs != PPO_ERR_UNSUPPORTED) return rs;
    }
    return dispatch_fwd<FwdMode::Sample>(p, a, e->N, e->H / 32);
}

// One teacher-forced step (FwdMode::Forced): actions_io[n] holds env n's given 0-based action (< 0: the env idles) and keeps it;
// psel_out[n] = the policy's probability of it (0 for an idle env or an action on an inactive quad, the latter also setting
// bit 64 of *err, a word of the caller's).  The per-step launch only: no split-rollout form, no persistent form, no bf16 mode
int32_t launch_policy_forced(ppo_policy_s* p, ppo_env_s* e, const int8_t* states_dev, const uint32_t* active_dev,
                             int32_t* actions_io, float* psel_out, float* full_probs_or_null, int32_t* err) {
    if (p->dtype != PPO_DTYPE_F32) {
        ppo_set_error("collect_paths!: a bf16-dtype policy is not supported (the teacher-forced mode exists in the fp32-MFMA forward only)");
        return PPO_ERR_UNSUPPORTED;
    }
    FwdArgs a = {};
    fill_weights(p, a);
    a.states = states_dev; a.active = active_dev; a.B = e->N;
    fill_rollout(e, a, actions_io, psel_out, full_probs_or_null, err);     // (the tick and the key go unread: nothing is sampled)
    a.actions = actions_io;
    ProfScope ps("k_policy_fwd_forced");
    return dispatch_fwd<FwdMode::Forced>(p, a, e->N, e->H / 32);
}

// One rollout step under the policy's selection, for the callers that APPLY a policy (play_quotas): the default
// ("sample", 1) is launch_policy_rollout itself, with its split and bf16 branches; any other selection launches FwdMode::Tempered
// or Greedy through the per-step dispatch only: no split-rollout form, no persistent form, no bf16.
// Rule "sample" with a non-default truncation launches Truncated instead, at any temperature, 1 included; greedy
// plays the arg-max, which every truncation keeps, and stays Greedy
int32_t launch_policy_select(ppo_policy_s* p, ppo_env_s* e, const int8_t* states_dev, const uint32_t* active_dev,
                             int32_t* actions_out, float* psel_out, float* full_probs_or_null) {
    const bool truncated = !default_truncation(p) && p->select_rule == PPO_SELECT_SAMPLE;
    if (default_selection(p) && !truncated)
        return launch_policy_rollout(p, e, states_dev, active_dev, actions_out, psel_out, full_probs_or_null);
    if (p->dtype != PPO_DTYPE_F32) {
        if (default_selection(p))
            ppo_set_error("truncation: a bf16-dtype policy plays the default truncation (top_k 0, top_p 1) only (the truncated "
                          "sampling mode exists in the fp32-MFMA forward only)");
        else
            ppo_set_error("selection: a bf16-dtype policy plays the default selection (\"sample\", 1) only (the tempered and greedy "
                          "modes exist in the fp32-MFMA forward only)");
        return PPO_ERR_UNSUPPORTED;
    }
    FwdArgs a = {};
    fill_weights(p, a);
    a.states = states_dev; a.active = active_dev; a.B = e->N;
    fill_rollout(e, a, actions_out, psel_out, full_probs_or_null, e->err.p);
    a.inv_temperature = (float)(1.0 / p->select_temperature);
    if (p->select_rule == PPO_SELECT_GREEDY) {
        ProfScope ps("k_policy_fwd_greedy");
        return dispatch_fwd<FwdMode::Greedy>(p, a, e->N, e->H / 32);
    }
    if (truncated) {
        a.top_k = (double)p->trunc_top_k;
        a.top_p = (float)p->trunc_top_p;
        ProfScope ps("k_policy_fwd_truncated");
        return dispatch_fwd<FwdMode::Truncated>(p, a, e->N, e->H / 32);
    }
    ProfScope ps("k_policy_fwd_tempered");
    return dispatch_fwd<FwdMode::Tempered>(p, a, e->N, e->H / 32);
}

// Persistent rollout (FwdMode::Persistent): T steps of all N envs in one launch.  Returns PPO_ERR_UNSUPPORTED (without setting an
// error) when the shape is not covered, so the caller falls back to the per-step launches.
// t0: first row of the rollout columns this launch writes (streaming collects a long rollout as a chain of launches)
int32_t launch_policy_rollout_persistent(ppo_policy_s* p, ppo_env_s* e, ppo_rollouts_s* ro, int64_t T, int record_probs,
                                         int64_t t0) {
    if (p->F != 72 || e->F != 72 || p->L != 2) return PPO_ERR_UNSUPPORTED;
    const int tps = e->H / 32;
    const int64_t N = e->N;
    const int64_t need = (N + 3) / 4;
    const int wps = (p->HID >= 256) ? 1 : 2;                     // FwdCfg<72, HID>::WPS
    const int64_t cap = 256 * wps;
    const unsigned grid = (unsigned)(need < cap ? need : cap);
    const int slots = (int)((N + (int64_t)grid * 4 - 1) / ((int64_t)grid * 4));
    const size_t lds = (size_t)4 * slots * (2 * e->V + 32);
    if (p->dtype == PPO_DTYPE_F32 && lds > 96 * 1024) return PPO_ERR_UNSUPPORTED;
    FwdArgs a = {};
    fill_weights(p, a);
    a.B = N; a.T = T;
    a.global_offset = e->global_offset; a.k0 = (uint32_t)e->seed; a.k1 = (uint32_t)(e->seed >> 32);
    a.env_score = e->score.p; a.env_degree = e->degree.p; a.env_active = e->active.p; a.env_steps = e->steps.p;
    a.env_reward = e->reward.p; a.env_done = e->done.p; a.env_episode = e->episode.p; a.env_tick = e->tick.p;
    a.env_tmpl = e->tmpl.p; a.envQ = e->Q; a.envV = e->V; a.env_max_actions = e->max_actions; a.env_slots = slots;
    a.env_nar = e->no_action_reward; a.err = e->err.p;
    const size_t r0 = (size_t)t0 * N;                                   // transitions in front of this launch's rows
    a.states_out = ro->compact ? nullptr : ro->states.p + r0 * e->H * e->F;
    a.cstate_out = ro->compact ? ro->cstate.p + r0 * 2 * e->V : nullptr;
    a.active_out = ro->active.p + r0; a.actions_out = ro->actions.p + r0; a.psel_out = ro->p_sel.p + r0;
    a.rew_out = ro->rewards.p + r0; a.done_out = ro->done.p + r0;
    a.full_probs = record_probs ? ro->full_probs.p + r0 * e->A : nullptr;
    ProfScope ps("k_rollout_persistent");
    if (p->dtype == PPO_DTYPE_BF16) return launch_policy_rollout_persistent_bf16(p, a, N, tps, e->V);
    if (N <= ppo_knobs().rollout_split_max_envs) {      // few envs: 2 or 4 waves per env, same bits (ppo_policy_rollout_split.hip)
        const int32_t rs = launch_rollout_split(p, a, N, tps, e->V, 1);
        if (rs != PPO_ERR_UNSUPPORTED) return rs;
        a.env_slots = slots;
    }
#define LAUNCH3(HH, TT)                                                                                      \
    do {                                                                                                     \
        static thread_local size_t attr_lds = 0;                                                                          \
        if (lds > attr_lds) {                                                                                \
            HIP_TRY(hipFuncSetAttribute((const void*)k_policy_fwd<72, HH, FwdMode::Persistent, TT>,                            \
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));              \
            attr_lds = lds;                                                                                  \
        }                                                                                                    \
        hipLaunchKernelGGL((k_policy_fwd<72, HH, FwdMode::Persistent, TT>), dim3(grid), dim3(256), lds, ppo_stream(), a);      \
    } while (0)
    if (p->HID == 256 && tps == 1) LAUNCH3(256, 1);
    else if (p->HID == 256 && tps == 4) LAUNCH3(256, 4);
    else if (p->HID == 128 && tps == 1) LAUNCH3(128, 1);
    else if (p->HID == 128 && tps == 4) LAUNCH3(128, 4);
    else return PPO_ERR_UNSUPPORTED;
#undef LAUNCH3
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

// a mode known at run time -> its instantiation (the modes that have a caller here)
static int32_t dispatch_fwd_mode(FwdMode mode, ppo_policy_s* p, const FwdArgs& a, int64_t B, int tps) {
    switch (mode) {
#define MODE_CASE(M) case FwdMode::M: return dispatch_fwd<FwdMode::M>(p, a, B, tps)
    MODE_CASE(TrainSnap); MODE_CASE(Train); MODE_CASE(Imitate); MODE_CASE(ImitateSnap); MODE_CASE(ValuePredict);
    MODE_CASE(ValuePredictSnap); MODE_CASE(ValueTrainClip); MODE_CASE(ValueTrainClipSnap); MODE_CASE(ValueTrain); MODE_CASE(ValueTrainSnap);
    MODE_CASE(Distill); MODE_CASE(DistillSnap); MODE_CASE(ProbsSnap); MODE_CASE(TrainAnchored); MODE_CASE(TrainAnchoredSnap);
#undef MODE_CASE
    default: ppo_set_error("k_policy_fwd: not a mode chosen at run time"); return PPO_ERR_ARG;
    }
}

// what both train forwards take from the workspace: the minibatch through idx, the saved activations, dL/dy and the loss terms
static void fill_train(ppo_policy_s* p, ppo_rollouts_s* ro, const int32_t* idx_dev, int64_t B, int64_t B_global, FwdArgs& a) {
    fill_weights(p, a);
    a.states = ro->states.p; a.active = ro->active.p; a.idx = idx_dev; a.B = B;
    a.act1 = (float4*)p->act1.p; a.act2 = (float4*)p->act2.p; a.dY = (float4*)p->dY.p; a.loss_terms = p->loss_terms.p;
    for (int l = 0; l < 2; ++l)          // deep policies: the hidden layers between the first and the last
        a.act_mid[l] = (p->L > 2 && l < p->L - 2) ? (float4*)p->actm.p + (size_t)l * p->cap_tiles * (p->HID / 32) * 256 : nullptr;
    a.inv_B = (float)(1.0 / (double)B_global);
    if (ro->compact) {      // env snapshots instead of observation rows: the rows are re-derived from them and left in p->xs
                            // (minibatch order) for the backward
        a.states = nullptr; a.cstate = ro->cstate.p; a.xs_out = p->xs.p;
        a.env_tmpl = ro->tmpl.p; a.envV = ro->V; a.envQ = ro->V / 4; a.env_slots = 1;
    }
}

// form: any TrainFwd but None and TrainTile (train_route)
int32_t launch_policy_train_fwd(ppo_policy_s* p, ppo_rollouts_s* ro, const int32_t* idx_dev, int64_t B,
                                int64_t B_global, double eps, double entropy_weight, const float* adv_col, TrainFwd form) {
    FwdArgs a = {};
    fill_train(p, ro, idx_dev, B, B_global, a);
    a.actions = ro->actions.p; a.p_old = ro->p_sel.p; a.adv = adv_col; a.ratio_out = p->ratio_out;
    a.eps = eps; a.c_over_B = (float)(entropy_weight / (double)B_global);
    ProfScope ps("k_policy_fwd_train");
    const FwdMode mode = fwd_train_mode(Objective::Policy, ro->compact);
    switch (form) {         // compact: TrainSnap / the CS form of the split kernel
    case TrainFwd::Split: return launch_policy_train_fwd_split(p, a, B, ro->compact);     // ppo_policy_fwd_split.hip
    case TrainFwd::Bf16: return launch_policy_fwd_bf16(p, a, mode, B, ro->H / 32);
    case TrainFwd::Fwd: return dispatch_fwd_mode(mode, p, a, B, ro->H / 32);
    default: return launch_policy_train_fwd_x6(p, a, B, form, ro->compact);               // ppo_policy_fwd_x6.hip
    }
}

// imitation train forward (FwdMode::Imitate / ImitateSnap): the policy's train forward with the cross-entropy of the buffer's actions as the loss;
// weight_col: the weights' column by transition id, clamped at 0 in the tail (nullptr: uniform weights).  Only this fp32-MFMA
// forward has the mode
int32_t launch_imitate_train_fwd(ppo_policy_s* p, ppo_rollouts_s* ro, const int32_t* idx_dev, int64_t B, int64_t B_global,
                                 double entropy_weight, const float* weight_col) {
    FwdArgs a = {};
    fill_train(p, ro, idx_dev, B, B_global, a);
    a.actions = ro->actions.p; a.adv = weight_col;
    a.c_over_B = (float)(entropy_weight / (double)B_global);
    ProfScope ps("k_policy_fwd_imitate");
    return dispatch_fwd_mode(fwd_train_mode(Objective::Imitate, ro->compact), p, a, B, ro->H / 32);
}

// distillation train forward (FwdMode::Distill / DistillSnap): the imitation forward with a target row per state,
// target_ptr[transition][A], in place of the stored action.  Only this fp32-MFMA forward has the mode
int32_t launch_distill_train_fwd(ppo_policy_s* p, ppo_rollouts_s* ro, const int32_t* idx_dev, int64_t B, int64_t B_global,
                                 double entropy_weight, const float* weight_col, const float* target_ptr) {
    FwdArgs a = {};
    fill_train(p, ro, idx_dev, B, B_global, a);
    a.adv = weight_col; a.targets = target_ptr;
    a.c_over_B = (float)(entropy_weight / (double)B_global);
    ProfScope ps("k_policy_fwd_distill");
    return dispatch_fwd_mode(fwd_train_mode(Objective::Distill, ro->compact), p, a, B, ro->H / 32);
}

// KL-anchored train forward (FwdMode::TrainAnchored / TrainAnchoredSnap): the policy's train forward with beta
// times the cross-entropy against target_ptr[transition][A] added to the surrogate; the divergence per state goes to
// anchor_dst.  Only this fp32-MFMA forward has the mode
int32_t launch_anchored_train_fwd(ppo_policy_s* p, ppo_rollouts_s* ro, const int32_t* idx_dev, int64_t B, int64_t B_global,
                                  double eps, double entropy_weight, const float* adv_col, const float* target_ptr, double beta,
                                  float* anchor_dst) {
    FwdArgs a = {};
    fill_train(p, ro, idx_dev, B, B_global, a);
    a.actions = ro->actions.p; a.p_old = ro->p_sel.p; a.adv = adv_col; a.ratio_out = p->ratio_out;
    a.eps = eps; a.c_over_B = (float)(entropy_weight / (double)B_global);
    a.targets = target_ptr; a.beta = beta; a.anchor_out = anchor_dst;
    ProfScope ps("k_policy_fwd_train_anchored");
    return dispatch_fwd_mode(fwd_train_mode(Objective::PolicyAnchored, ro->compact), p, a, B, ro->H / 32);
}

// probs_dev[b][A] of B states held as env snapshots [B][2V] in storage order (FwdMode::ProbsSnap: what ValuePredictSnap is to
// ValuePredict): launch_policy_probs' bits for the rows the snapshots expand to.  fp32 policies, F = 72
int32_t launch_policy_probs_snap(ppo_policy_s* p, const int8_t* cstate_dev, const uint32_t* active_dev, const int8_t* tmpl_dev,
                                 int32_t V, int64_t B, int32_t H, float* probs_dev) {
    if (B <= 0) return PPO_OK;
    FwdArgs a = {};
    fill_weights(p, a);
    a.active = active_dev; a.B = B; a.probs_out = probs_dev;
    a.cstate = cstate_dev; a.env_tmpl = tmpl_dev; a.envV = V; a.envQ = V / 4; a.env_slots = 1;
    ProfScope ps("k_policy_fwd_probs_snap");
    return dispatch_fwd_mode(FwdMode::ProbsSnap, p, a, B, H / 32);
}

// ---- critic (the Value* modes): only this fp32-MFMA forward has them
// values_dev[b] = V(state b) for B states in storage order: observation rows [B][H][F] (cstate_dev == nullptr), or env
// snapshots [B][2V] with the buffer's template (compact rollouts; F = 72)
int32_t launch_value_predict(ppo_policy_s* p, const int8_t* states_dev, const int8_t* cstate_dev, const uint32_t* active_dev,
                             const int8_t* tmpl_dev, int32_t V, int64_t B, int32_t H, float* values_dev) {
    if (B <= 0) return PPO_OK;
    FwdArgs a = {};
    fill_weights(p, a);
    a.states = states_dev; a.active = active_dev; a.B = B; a.values_out = values_dev;
    ProfScope ps("k_value_fwd_predict");
    if (!cstate_dev) return dispatch_fwd_mode(FwdMode::ValuePredict, p, a, B, H / 32);
    a.states = nullptr; a.cstate = cstate_dev; a.env_tmpl = tmpl_dev; a.envV = V; a.envQ = V / 4; a.env_slots = 1;
    return dispatch_fwd_mode(FwdMode::ValuePredictSnap, p, a, B, H / 32);
}

// value-train forward of a minibatch: saves the activations like the policy's train forward, leaves dL/dy of
// Flux.mse(V, target_col[idx]) in p->dY and the squared errors in p->loss_terms; with vold_col the clipped value loss against
// those old values (range vclip), the per-state V - vold going to vdelta_dst when given
int32_t launch_value_train_fwd(ppo_policy_s* p, ppo_rollouts_s* ro, const int32_t* idx_dev, int64_t B, int64_t B_global,
                               const float* target_col, const float* vold_col, float vclip, float* vdelta_dst) {
    FwdArgs a = {};
    fill_train(p, ro, idx_dev, B, B_global, a);
    a.vtarget = target_col;
    a.vold = vold_col; a.vclip = vclip; a.vdelta_out = vold_col ? vdelta_dst : nullptr;
    ProfScope ps("k_value_fwd_train");
    return dispatch_fwd_mode(fwd_train_mode(Objective::Value, ro->compact, vold_col != nullptr), p, a, B, ro->H / 32);
}

int32_t launch_categorical(const float* probs, const float* u, int64_t B, int64_t A, int32_t* actions, float* psel,
                           int32_t* err) {
    if (B <= 0) return PPO_OK;
    hipLaunchKernelGGL(k_categorical, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, ppo_stream(), probs, u, B, A,
                       actions, psel, err);
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}
