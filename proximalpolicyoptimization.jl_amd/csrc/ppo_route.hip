// ppo_route.hip -- which kernels run a training minibatch, and every kernel-selection knob of the policy (host only).
#include "ppo_internal.h"
#include <cstdlib>

static int64_t env_int(const char* name, int64_t dflt) { const char* v = std::getenv(name); return v ? (int64_t)atoll(v) : dflt; }
static int32_t env_flag(const char* name, int32_t dflt) { const char* v = std::getenv(name); return v ? (atoi(v) != 0) : dflt; }
static int32_t env_mode(const char* name) { const char* v = std::getenv(name); return (v && (v[0] == '0' || v[0] == '1')) ? v[0] - '0' : -1; }

static PpoKnobs knobs_from_env() {
    PpoKnobs k;
    k.bwd_split = env_flag("PPO_BWD_SPLIT_BF16", k.bwd_split);
    k.train_tile_max_tiles = env_int("PPO_TRAIN_TILE_MAX_TILES", k.train_tile_max_tiles);
    k.bwd_small_max_tiles = env_int("PPO_BWD_SMALL_MAX_TILES", k.bwd_small_max_tiles);
    k.bwd_small_max_tiles_split = env_int("PPO_BWD_SMALL_MAX_TILES_SPLIT", k.bwd_small_max_tiles_split);
    k.fwd_split_max_states = env_int("PPO_FWD_SPLIT_MAX_STATES", k.fwd_split_max_states);
    k.fwd_x6_max_states = env_int("PPO_FWD_SPLIT_MAX_TILES", k.fwd_x6_max_states);
    k.fwd_x6_t2_min_tiles[0] = env_int("PPO_FWD_SPLIT_T2_MIN_TILES_128", k.fwd_x6_t2_min_tiles[0]);
    k.fwd_x6_t2_min_tiles[1] = env_int("PPO_FWD_SPLIT_T2_MIN_TILES", k.fwd_x6_t2_min_tiles[1]);
    k.fuse_reduce_adam = env_flag("PPO_FUSE_REDUCE_ADAM", k.fuse_reduce_adam);
    k.rollout_persistent = env_mode("PPO_ROLLOUT_PERSISTENT");
    k.rollout_compact = env_mode("PPO_ROLLOUT_COMPACT");
    if (const char* v = std::getenv("PPO_COMPACT_AUTO_BYTES")) k.compact_auto_bytes = atof(v);
    k.rollout_split_max_envs = env_int("PPO_ROLLOUT_SPLIT_MAX_ENVS", k.rollout_split_max_envs);
    return k;
}

static const PpoKnobs g_start = knobs_from_env();   // what -1 restores
static PpoKnobs g_knobs = g_start;
const PpoKnobs& ppo_knobs() { return g_knobs; }

extern "C" {
int32_t ppo_set_bwd_split_bf16(int32_t mode) { g_knobs.bwd_split = mode < 0 ? g_start.bwd_split : (mode != 0); return PPO_OK; }
int32_t ppo_set_train_tile_max_tiles(int64_t tiles) { g_knobs.train_tile_max_tiles = tiles < 0 ? g_start.train_tile_max_tiles : tiles; return PPO_OK; }
int32_t ppo_set_bwd_small_max_tiles(int64_t tiles) { g_knobs.bwd_small_max_tiles = tiles < 0 ? g_start.bwd_small_max_tiles : tiles; return PPO_OK; }
int32_t ppo_set_fwd_split_max_states(int64_t states) { g_knobs.fwd_split_max_states = states < 0 ? g_start.fwd_split_max_states : states; return PPO_OK; }
int32_t ppo_set_fwd_split_t2_min_tiles(int32_t hid, int64_t tiles) {
    ARG_CHECK(hid == 128 || hid == 256, "set_fwd_split_t2_min_tiles: hid must be 128 or 256");
    g_knobs.fwd_x6_t2_min_tiles[hid == 256] = tiles < 0 ? g_start.fwd_x6_t2_min_tiles[hid == 256] : tiles; return PPO_OK;
}
int32_t ppo_set_rollout_persistent(int32_t mode) { g_knobs.rollout_persistent = mode < 0 ? g_start.rollout_persistent : (mode != 0); return PPO_OK; }
int32_t ppo_set_rollout_compact(int32_t mode) { g_knobs.rollout_compact = mode < 0 ? g_start.rollout_compact : (mode != 0); return PPO_OK; }
int32_t ppo_set_rollout_split_max_envs(int64_t envs) { g_knobs.rollout_split_max_envs = envs < 0 ? g_start.rollout_split_max_envs : envs; return PPO_OK; }
}  // extern "C"

TrainRoute train_route(int32_t dtype, int F, int HID, int L, int H, bool compact, int64_t states, const PpoKnobs& k, Objective obj) {
    // (value: the objectives only the fp32-MFMA forward has a tail for -- a critic's mse, the imitation cross-entropy and the
    // distillation cross-entropy -- and the policy's KL-anchored objective, which takes the same branch)
    const bool f32 = dtype == PPO_DTYPE_F32, value = obj != Objective::Policy;
    const int tps = H / 32;
    const int64_t tiles = states * tps;
    const bool split_images = F == 72 && L == 2;        // the policy holds the split-fp32 weight images (ppo_policy_create)
    if (value) {                                        // what the fp32-MFMA forward refuses, before anything else
        if (!f32 && obj == Objective::Imitate) return {TrainFwd::None, TrainBwd::None, "imitation training of a bf16-dtype policy is not supported: the imitation modes exist in the fp32-MFMA forward only"};
        if (!f32 && obj == Objective::Distill) return {TrainFwd::None, TrainBwd::None, "distillation into a bf16-dtype student is not supported: the distillation modes exist in the fp32-MFMA forward only"};
        if (!f32 && obj == Objective::PolicyAnchored) return {TrainFwd::None, TrainBwd::None, "KL-anchored training of a bf16-dtype policy is not supported: the anchored modes exist in the fp32-MFMA forward only"};
        if (!f32) return {TrainFwd::None, TrainBwd::None, "a bf16-dtype critic is not supported: the value modes exist in the fp32-MFMA forward only"};
        if (F != 72 && tps != 1) return {TrainFwd::None, TrainBwd::None, "unsupported policy/state shape (F,HID,H) for the gfx950 kernels"};
        if (F != 72 && compact) return {TrainFwd::None, TrainBwd::None, "compact rollouts need the built-in env's F = 72"};
    }
    // small minibatches: the whole training pass of a tile on one CU, then the weight gradients
    if (tiles <= k.train_tile_max_tiles && f32 && split_images && H == 32 && !compact)
        return value ? TrainRoute{TrainFwd::Fwd, TrainBwd::Small, nullptr} : TrainRoute{TrainFwd::TrainTile, TrainBwd::Wgrad, nullptr};
    TrainRoute r = {TrainFwd::None, TrainBwd::None, nullptr};
    if (value) {
        r.fwd = TrainFwd::Fwd;
    } else if (k.bwd_split && states <= k.fwd_x6_max_states && f32 && split_images && (tps == 1 || (tps == 4 && HID == 256))) {
        // Dense products as split-fp32 MFMAs: Q = 32 states one workgroup each, Q = 8 from the switch point two tiles per pass
        const int64_t t2 = k.fwd_x6_t2_min_tiles[HID == 256];
        r.fwd = tps == 4 ? TrainFwd::X6S : (t2 > 0 && tiles >= t2) ? TrainFwd::X6T : TrainFwd::X6;
    } else if (states <= k.fwd_split_max_states && f32 && split_images && tps == 1) {
        r.fwd = TrainFwd::Split;                         // small minibatch: 2 or 4 waves per state
    } else if (!f32) {
        if (F != 72) return {TrainFwd::None, TrainBwd::None, "unsupported policy/state shape (F,HID,H) for the gfx950 bf16 kernels"};
        r.fwd = TrainFwd::Bf16;
    } else {
        if (F != 72 && tps != 1) return {TrainFwd::None, TrainBwd::None, "unsupported policy/state shape (F,HID,H) for the gfx950 kernels"};
        if (F != 72 && compact) return {TrainFwd::None, TrainBwd::None, "compact rollouts need the built-in env's F = 72"};
        r.fwd = TrainFwd::Fwd;
    }
    // the fused backward is the L = 2 shape with all its weight gradients resident (F = 216 at HID = 256 does not fit its
    // LDS): every other fp32 policy takes the layer-looped three-product form at any minibatch size.  Against the fp32-MFMA
    // fused kernel the three-product form is 7.6 % faster per PPO iteration at 256 tiles, level at 512 and 6 % slower at 1024
    // (HID = 256), hence 384; against the split-fp32 one it wins at no size (128 / 256 / 384 tiles:
    // 30.3 / 35.6 / 49.4 ms per iteration against 28.4 / 35.5 / 43.8), hence 0
    const bool fused_ok = L == 2 && !(F == 216 && HID == 256);
    const bool split_bwd = k.bwd_split && split_images;
    if (f32 && (!fused_ok || tiles <= (split_bwd ? k.bwd_small_max_tiles_split : k.bwd_small_max_tiles))) r.bwd = TrainBwd::Small;
    else if (!f32) r.bwd = TrainBwd::Bf16;
    else r.bwd = split_bwd ? TrainBwd::X6 : TrainBwd::Fused;
    return r;
}

// diagnostics for the tests (not part of include/ppo_hip.h): the kernels train_route picks for a shape and an objective under
// the current knobs, named as a kernel trace lists them demangled (first kernel of each half).  No HIP call.
static int32_t debug_route(const char* who, Objective obj, int32_t dtype, int32_t F, int32_t hid, int32_t L, int32_t H,
                           int32_t compact, int64_t states, char* fwd, char* bwd, int64_t cap) {
    ARG_CHECK((dtype == PPO_DTYPE_F32 || dtype == PPO_DTYPE_BF16) && (F == 72 || F == 216) && (hid == 128 || hid == 256) && L >= 1 && L <= 4 && (H == 32 || H == 128) && states >= 1,
              std::string(who) + ": shape");
    ARG_CHECK(fwd && bwd && cap >= 64, std::string(who) + ": output buffers");
    const TrainRoute r = train_route(dtype, F, hid, L, H, compact != 0, states, ppo_knobs(), obj);
    const int tps = H / 32, mode = (int)fwd_route_mode(obj, compact != 0);      // the kernels' names print the mode's number
    switch (r.fwd) {
    case TrainFwd::None: snprintf(fwd, cap, "none"); break;
    case TrainFwd::TrainTile: snprintf(fwd, cap, "k_policy_train_tile<72,%d>", hid); break;
    case TrainFwd::X6S: snprintf(fwd, cap, "k_policy_fwd_train_x6s<256,4>"); break;
    case TrainFwd::X6T: snprintf(fwd, cap, "k_policy_fwd_train_x6t<%d,2>", hid); break;
    case TrainFwd::X6: snprintf(fwd, cap, "k_policy_fwd_train_x6<%d>", hid); break;
    // (launch_split: 4 waves per state up to 256 states, 2 above)
    case TrainFwd::Split: snprintf(fwd, cap, "k_policy_fwd_train_split<72,%d,%d,%d>", hid, states <= 256 ? 4 : 2, compact ? 1 : 0); break;
    case TrainFwd::Fwd: snprintf(fwd, cap, "k_policy_fwd<%d,%d,%d,%d,%d>", F, hid, mode, tps, L != 2 ? 1 : 0); break;
    case TrainFwd::Bf16: snprintf(fwd, cap, "k_policy_fwd_bf16<72,%d,%d,%d>", hid, mode, tps); break;
    }
    switch (r.bwd) {
    case TrainBwd::None: snprintf(bwd, cap, "none"); break;
    case TrainBwd::Wgrad: snprintf(bwd, cap, "k_policy_wgrad<72,%d,true>", hid); break;
    case TrainBwd::Small: snprintf(bwd, cap, "k_policy_bwd_data%s<%d,%d>", L == 2 ? "" : "_deep", F, hid); break;
    case TrainBwd::X6: snprintf(bwd, cap, "k_policy_bwd_x6<72,%d>", hid); break;
    case TrainBwd::Fused: snprintf(bwd, cap, "k_policy_bwd<%d,%d>", F, hid); break;
    case TrainBwd::Bf16: snprintf(bwd, cap, "k_policy_bwd_bf16<72,%d>", hid); break;
    }
    if (r.fwd == TrainFwd::None) { ppo_set_error(r.err); return PPO_ERR_UNSUPPORTED; }
    return PPO_OK;
}

extern "C" int32_t ppo_debug_train_route(int32_t dtype, int32_t F, int32_t hid, int32_t L, int32_t H, int32_t compact,
                                         int64_t states, char* fwd, char* bwd, int64_t cap) {
    return debug_route("ppo_debug_train_route", Objective::Policy, dtype, F, hid, L, H, compact, states, fwd, bwd, cap);
}
extern "C" int32_t ppo_debug_value_route(int32_t dtype, int32_t F, int32_t hid, int32_t L, int32_t H, int32_t compact,
                                         int64_t states, char* fwd, char* bwd, int64_t cap) {
    return debug_route("ppo_debug_value_route", Objective::Value, dtype, F, hid, L, H, compact, states, fwd, bwd, cap);
}
extern "C" int32_t ppo_debug_imitate_route(int32_t dtype, int32_t F, int32_t hid, int32_t L, int32_t H, int32_t compact,
                                           int64_t states, char* fwd, char* bwd, int64_t cap) {
    return debug_route("ppo_debug_imitate_route", Objective::Imitate, dtype, F, hid, L, H, compact, states, fwd, bwd, cap);
}
extern "C" int32_t ppo_debug_distill_route(int32_t dtype, int32_t F, int32_t hid, int32_t L, int32_t H, int32_t compact,
                                           int64_t states, char* fwd, char* bwd, int64_t cap) {
    return debug_route("ppo_debug_distill_route", Objective::Distill, dtype, F, hid, L, H, compact, states, fwd, bwd, cap);
}
extern "C" int32_t ppo_debug_anchor_route(int32_t dtype, int32_t F, int32_t hid, int32_t L, int32_t H, int32_t compact,
                                          int64_t states, char* fwd, char* bwd, int64_t cap) {
    return debug_route("ppo_debug_anchor_route", Objective::PolicyAnchored, dtype, F, hid, L, H, compact, states, fwd, bwd, cap);
}
