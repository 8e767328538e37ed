// ppo_train.hip -- the training half of the extern "C" surface (include/ppo_hip.h): one minibatch pass and one epoch loop,
// driven for the policy (step_batch! / ppo_train!), for a critic (value_forward_backward / value_train) and for the policy's
// imitation objective (imitate_forward_backward / imitate_train) and its distillation objective (distill_forward_backward /
// distill_train, with the target column's fill, upload and getter), and the critic's state values and GAE.  Host orchestration only: launch order, all math is in the kernels.
#include "ppo_internal.h"
#include <algorithm>
#include <cmath>

extern "C" {

// ================================================================ training
// B = number of 32-row tiles of the minibatch (states * H/32)
static int32_t train_reserve(ppo_policy_s* p, int64_t B, bool compact = false) {
    if (compact) PPO_TRY(p->xs.alloc((size_t)std::max(B, p->cap_tiles) * 32 * p->F));
    if (B <= p->cap_tiles) return PPO_OK;
    const size_t NT = p->HID / 32;
    PPO_TRY(p->act1.alloc((size_t)B * NT * 1024));
    if (p->L >= 2) PPO_TRY(p->act2.alloc((size_t)B * NT * 1024));
    if (p->L > 2) PPO_TRY(p->actm.alloc((size_t)(p->L - 2) * B * NT * 1024));       // hidden layers between the first and the last
    PPO_TRY(p->dY.alloc((size_t)B * 128)); PPO_TRY(p->loss_terms.alloc((size_t)B * 2));
    // one gradient slab per backward workgroup: 256, or 512 where two workgroups share a CU (fp32 HID = 128, F = 72)
    PPO_TRY(p->slabs.alloc((size_t)((p->HID == 128 && p->F == 72) ? 512 : 256) * slab_floats(p->F, p->HID, p->L)));
    PPO_TRY(p->idx.alloc((size_t)B));
    PPO_TRY(p->ratio.alloc((size_t)B)); p->ratio_last = nullptr; p->ratio_last_n = 0;
    p->cap_tiles = B;
    return PPO_OK;
}

// batch_advantage: the column (by transition id) adv_mode selects for a minibatch -- the PPO surrogate's advantages, and the
// weights of the weighted imitation loss
static int32_t advantage_column(ppo_policy_s* net, ppo_rollouts_s* ro, const int32_t* idx_dev, int64_t B, int32_t adv_mode,
                                const float** col) {
    const float* adv = ro->returns.p;                       // batch_advantage = returns (reference-equivalent)
    if (adv_mode == PPO_ADV_GAE || adv_mode == PPO_ADV_GAE_NORMALISED) {
        ARG_CHECK(ro->adv.p && ro->adv_T == ro->T, "batch_advantage: GAE mode needs ppo_rollouts_compute_gae on these rollouts first");
        adv = ro->adv.p;
    }
    if (adv_mode == PPO_ADV_RETURNS_NORMALISED || adv_mode == PPO_ADV_GAE_NORMALISED) {   // normalised over this rank's minibatch
        PPO_TRY(net->adv_col.alloc((size_t)ro->capT * ro->N));
        PPO_TRY(launch_adv_normalise(adv, idx_dev, B, net->adv_col.p));
        adv = net->adv_col.p;
    }
    *col = adv;
    return PPO_OK;
}

// One minibatch: train forward, backward, slab reduction (+ the optimiser step when fuse_opt is given).
// idx_dev: transition ids (already resolved through the dataset index)
static int32_t train_pass_dev(ppo_policy_s* net, ppo_rollouts_s* ro, const int32_t* idx_dev, int64_t B, int64_t B_global,
                              const TrainObjective& obj, ppo_adam_s* fuse_opt = nullptr, float* fuse_hist2 = nullptr) {
    PPO_TRY(train_reserve(net, B * (ro->H / 32), ro->compact));
    // (the KL-anchored objective is the policy's: advantages and ratios as for Objective::Policy, a forward of its own)
    const bool anchored = obj.kind == Objective::PolicyAnchored;
    const bool policy = obj.kind == Objective::Policy || anchored, imitate = obj.kind == Objective::Imitate, distill = obj.kind == Objective::Distill;
    const float* adv = nullptr;                            // imitation / distillation with uniform weights: no column
    if (policy || ((imitate || distill) && obj.weight_mode == PPO_IMITATE_POSITIVE_ADVANTAGE))
        PPO_TRY(advantage_column(net, ro, idx_dev, B, obj.adv_mode, &adv));
    if (policy) {
        // the tail's probability ratios, stored while a target_kl is set only (measured: the store costs the train forward
        // 0.2 %, more than the run-to-run spread of the benchmark): the caller's slice of an epoch column (train_epochs), else
        // the policy's minibatch buffer.  A critic stores none, whatever its handle's target_kl
        const bool keep_ratio = net->target_kl != 0.0;
        net->ratio_out = !keep_ratio ? nullptr : obj.ratio_dst ? obj.ratio_dst : net->ratio.p;
        if (keep_ratio && !obj.ratio_dst) { net->ratio_last = net->ratio.p; net->ratio_last_n = (int64_t)net->ratio.n; }
    }
    const TrainRoute r = train_route(net->dtype, net->F, net->HID, net->L, ro->H, ro->compact, B, ppo_knobs(), obj.kind);
    if (r.fwd == TrainFwd::None) { ppo_set_error(r.err); return PPO_ERR_UNSUPPORTED; }
    if (r.bwd == TrainBwd::Wgrad || r.bwd == TrainBwd::Small) {
        const size_t frag = (size_t)net->cap_tiles * (net->HID / 32) * 1024;     // dZ in fragment order, like act1 / act2
        PPO_TRY(net->dz1f.alloc(frag));
        if (net->L >= 2) PPO_TRY(net->dz2f.alloc(frag));
        if (net->L > 2) PPO_TRY(net->dzm.alloc((size_t)(net->L - 2) * frag));
    }
    if (imitate) PPO_TRY(launch_imitate_train_fwd(net, ro, idx_dev, B, B_global, obj.entropy_weight, adv));
    else if (distill) PPO_TRY(launch_distill_train_fwd(net, ro, idx_dev, B, B_global, obj.entropy_weight, adv, obj.distill_targets));
    else if (anchored) {
        // the divergence per state: the caller's slice of an epoch column (train_epochs), else the policy's minibatch buffer
        float* kl_dst = obj.anchor_dst;
        if (!kl_dst) {
            PPO_TRY(net->anchor.alloc((size_t)net->cap_tiles));
            kl_dst = net->anchor.p; net->anchor_last = kl_dst; net->anchor_last_n = (int64_t)net->anchor.n;
        }
        PPO_TRY(launch_anchored_train_fwd(net, ro, idx_dev, B, B_global, obj.eps, obj.entropy_weight, adv, obj.anchor_targets,
                                          obj.anchor_coef, kl_dst));
    }
    else if (!policy) {
        // PPO's clipped value loss while the critic handle has a clip range: against the buffer's values of before the update
        // (the callers have checked that they are there), V - vold going to the caller's slice of an epoch column if any
        TrainObjective o = obj;
        if (net->value_clip != 0.0) { o.vold_col = ro->values.p; o.vclip = (float)net->value_clip; }
        else o.vdelta_dst = nullptr;
        PPO_TRY(launch_value_train_fwd(net, ro, idx_dev, B, B_global, o.target_col, o.vold_col, o.vclip, o.vdelta_dst));
    }
    else if (r.fwd == TrainFwd::TrainTile) PPO_TRY(launch_policy_train_tile(net, ro, idx_dev, B, B_global, obj.eps, obj.entropy_weight, adv));
    else PPO_TRY(launch_policy_train_fwd(net, ro, idx_dev, B, B_global, obj.eps, obj.entropy_weight, adv, r.fwd));
    switch (r.bwd) {
    case TrainBwd::Small: PPO_TRY(launch_policy_bwd_small(net, ro, idx_dev, B)); break;
    case TrainBwd::X6: PPO_TRY(launch_policy_bwd_x6(net, ro, idx_dev, B)); break;
    case TrainBwd::Fused: PPO_TRY(launch_policy_bwd(net, ro, idx_dev, B)); break;
    case TrainBwd::Bf16: PPO_TRY(launch_policy_bwd_bf16(net, ro, idx_dev, B)); break;
    default: break;                                         // Wgrad: launched by launch_policy_train_tile
    }
    PPO_TRY(launch_grad_reduce(net, B, B_global, obj.entropy_weight, fuse_opt, fuse_hist2));   // Value: the weight stays 0
    net->last_B = B; net->last_entropy_weight = obj.entropy_weight;
    return PPO_OK;
}

// out[i] = index[pos[i]] for B dataset positions; one outside [0, len) raises the device flag
__global__ void k_gather_index(const int32_t* __restrict__ index, const int64_t* __restrict__ pos, int64_t B,
                               int64_t len, int32_t* __restrict__ out, int32_t* __restrict__ err) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const int64_t p = pos[i];
    if (p < 0 || p >= len) { atomicOr(err, 16); out[i] = index[0]; return; }
    out[i] = index[p];
}

static int32_t launch_gather_index(const ppo_rollouts_s* ro, const int64_t* pos_dev, int64_t n, int32_t* out, int32_t* err) {
    hipLaunchKernelGGL(k_gather_index, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ppo_stream(), ro->index.p, pos_dev, n,
                       ro->len, out, err);
    HIP_TRY(hipGetLastError());
    return PPO_OK;
}

// the caller's minibatch (dataset positions on the host) -> its transition ids in net->idx; pos: the upload, alive until the
// caller has waited for the stream
static int32_t gather_minibatch(ppo_policy_s* net, ppo_rollouts_s* ro, const int64_t* sample_idx, int64_t B, DevBuf<int64_t>& pos) {
    for (int64_t i = 0; i < B; ++i) ARG_CHECK(sample_idx[i] >= 0 && sample_idx[i] < ro->len, "dataset index out of range (src/rollout_buffer.jl:105-106)");
    PPO_TRY(train_reserve(net, B * (ro->H / 32)));
    PPO_TRY(pos.alloc(B));
    PPO_TRY(h2d(pos.p, sample_idx, (size_t)B));
    return launch_gather_index(ro, pos.p, B, net->idx.p, net->err.p);
}

// KL anchor: while the policy handle has one, the policy's pass runs Objective::PolicyAnchored with the handle's
// coefficient against the buffer's rows of the handle's source.  What the distillation entry points refuse is refused here,
// before anything is launched: a source not filled / not recorded for these rollouts, a disk sink, a bf16-dtype policy
static int32_t anchor_objective(const char* who, ppo_policy_s* pol, ppo_rollouts_s* ro, TrainObjective& obj) {
    if (pol->anchor_source == PPO_ANCHOR_OFF) return PPO_OK;
    if (pol->dtype != PPO_DTYPE_F32) {
        ppo_set_error(std::string(who) + ": KL-anchored training of a bf16-dtype policy is not supported: the anchored modes exist in the fp32-MFMA forward only");
        return PPO_ERR_UNSUPPORTED;
    }
    if (ro->sink) {
        ppo_set_error(std::string(who) + ": a KL anchor on a buffer with a disk sink attached is not supported");
        return PPO_ERR_UNSUPPORTED;
    }
    if (pol->anchor_source == PPO_TARGETS_COLUMN) {
        ARG_CHECK(ro->targets.p && ro->targets_T == ro->T && ro->T >= 1, std::string(who) + ": KL anchor: the target column is not filled for these rollouts (ppo_rollouts_fill_targets or ppo_rollouts_set_targets first)");
        obj.anchor_targets = ro->targets.p;
    } else {
        ARG_CHECK(ro->full_probs.p && ro->probs_T == ro->T && ro->T >= 1, std::string(who) + ": KL anchor: no recorded distributions for these rollouts (collect them with record_probs)");
        obj.anchor_targets = ro->full_probs.p;
    }
    obj.kind = Objective::PolicyAnchored;
    obj.anchor_coef = pol->anchor_coef;
    return PPO_OK;
}

int32_t ppo_forward_backward(ppo_policy_t pol, ppo_rollouts_t ro, const int64_t* sample_idx, int64_t B,
                             int64_t B_global, double epsilon, double entropy_weight, int32_t adv_mode) {
    ARG_CHECK(pol && ro && sample_idx, "step_batch!: null argument");
    ARG_CHECK(B >= 1 && B <= ro->len, "step_batch!: 1 <= batch_size <= num_data (src/train.jl:88)");
    ARG_CHECK(B_global >= B, "step_batch!: B_global < B");
    ARG_CHECK(pol->F == ro->F && (ro->H == 32 || ro->H == 128), "step_batch!: shape mismatch");
    if (adv_mode < PPO_ADV_RETURNS || adv_mode > PPO_ADV_GAE_NORMALISED) { ppo_set_error("batch_advantage: unknown advantage mode"); return PPO_ERR_UNSUPPORTED; }
    TrainObjective obj = {Objective::Policy};
    obj.eps = epsilon; obj.entropy_weight = entropy_weight; obj.adv_mode = adv_mode;
    PPO_TRY(anchor_objective("step_batch!", pol, ro, obj));
    DevBuf<int64_t> pos;
    PPO_TRY(gather_minibatch(pol, ro, sample_idx, B, pos));
    PPO_TRY(train_pass_dev(pol, ro, pol->idx.p, B, B_global, obj));
    HIP_TRY(hipStreamSynchronize(ppo_stream()));
    return PPO_OK;
}

int32_t ppo_adam_apply(ppo_adam_t opt, ppo_policy_t pol) {
    ARG_CHECK(opt && pol && opt->pol == pol, "update!: optimiser was created for another policy");
    return launch_adam(opt, nullptr);
}

int32_t ppo_last_losses(ppo_policy_t pol, double* ppoloss, double* entropyloss) {
    ARG_CHECK(pol, "null");
    float t[2];
    PPO_TRY(d2h(t, pol->grad.p + pol->np, 2));
    if (ppoloss) *ppoloss = t[0];
    if (entropyloss) *entropyloss = t[1];
    return PPO_OK;
}

// diagnostic for the tests (not part of include/ppo_hip.h): what the last training forward left per tile of its minibatch, in
// minibatch order -- the dL/dlogits rows [tiles][32][4] and the two loss terms [tiles][2]
int32_t ppo_debug_train_outputs(ppo_policy_t pol, int64_t tiles, float* dY, double* loss_terms) {
    ARG_CHECK(pol && tiles >= 1 && tiles <= pol->cap_tiles, "ppo_debug_train_outputs: tiles out of range");
    if (dY) PPO_TRY(d2h(dY, pol->dY.p, (size_t)tiles * 128));
    if (loss_terms) PPO_TRY(d2h(loss_terms, pol->loss_terms.p, (size_t)tiles * 2));
    return PPO_OK;
}

// likewise: the probability ratios p_new / p_old the loss tail stored, one per state -- of the latest forward in minibatch
// order (n up to the capacity of that buffer: what lies behind the minibatch is whatever an earlier, larger one left), or,
// after ppo_train, of its latest epoch in the order of that epoch's permutation (n up to the dataset length)
int32_t ppo_debug_train_ratios(ppo_policy_t pol, int64_t n, float* out) {
    ARG_CHECK(pol && out, "ppo_debug_train_ratios: null argument");
    ARG_CHECK(pol->ratio_last && n >= 1 && n <= pol->ratio_last_n, "ppo_debug_train_ratios: no ratios stored, or n out of range");
    return d2h(out, pol->ratio_last, (size_t)n);
}

int32_t ppo_step_batch(ppo_policy_t pol, ppo_adam_t opt, ppo_rollouts_t ro, const int64_t* sample_idx, int64_t B,
                       double epsilon, double entropy_weight, int32_t adv_mode, double* ppoloss, double* entropyloss) {
    PPO_TRY(ppo_forward_backward(pol, ro, sample_idx, B, B, epsilon, entropy_weight, adv_mode));
    PPO_TRY(ppo_last_losses(pol, ppoloss, entropyloss));
    return ppo_adam_apply(opt, pol);
}


// Data-parallel shards may differ in length (remainder envs, episode-mode rollouts): every rank learns every
// rank's dataset length once per call -- an all-gather spelled as the hook's sum all-reduce over a one-hot
// [2*world] vector (length split into two exactly representable floats).  lens: [world], this rank's filled in
static int32_t exchange_shard_lengths(std::vector<int64_t>& lens, int32_t rank, ppo_allreduce_fn allreduce, void* allreduce_ctx) {
    const int32_t world = (int32_t)lens.size();
    const int64_t len = lens[(size_t)rank];
    DevBuf<float> xch;
    PPO_TRY(xch.alloc((size_t)2 * world));
    std::vector<float> hx((size_t)2 * world, 0.0f);
    hx[2 * (size_t)rank] = (float)(len >> 12); hx[2 * (size_t)rank + 1] = (float)(len & 4095);
    PPO_TRY(h2d(xch.p, hx.data(), hx.size()));
    if (allreduce(allreduce_ctx, xch.p, 2 * (int64_t)world) != 0) { ppo_set_error("all-reduce hook failed (shard-length exchange)"); return PPO_ERR_ARG; }
    // a rank that fails locally from here on must not leave the others blocked in their next collective: every rank
    // carries its status into ONE more tiny all-reduce and all of them return together
    int32_t local = d2h(hx.data(), xch.p, hx.size());
    if (local == PPO_OK) {
        for (int32_t r = 0; r < world; ++r) lens[(size_t)r] = ((int64_t)hx[2 * (size_t)r] << 12) + (int64_t)hx[2 * (size_t)r + 1];
        if (lens[(size_t)rank] != len) {
            ppo_set_error("AssertionError: ppo_train!: shard-length exchange is inconsistent (two ranks with the same rank id, "
                          "or a hook that does not SUM the buffer it is handed?)");
            local = PPO_ERR_ARG;
        }
    }
    float bad = local == PPO_OK ? 0.0f : 1.0f;
    const int32_t hs = h2d(xch.p, &bad, 1);
    if (allreduce(allreduce_ctx, xch.p, 1) != 0) { ppo_set_error("all-reduce hook failed (status agreement)"); return PPO_ERR_ARG; }
    PPO_TRY(hs);
    PPO_TRY(d2h(&bad, xch.p, 1));
    if (local != PPO_OK) return local;
    if (bad != 0.0f) { ppo_set_error("ppo_train!: another data-parallel rank failed in the shard-length exchange"); return PPO_ERR_ARG; }
    return PPO_OK;
}

// every rank must hold the same per-epoch statistics (and take the same target_kl decision): gather all ranks' k sums EXACTLY
// (a one-hot [world][k][3] vector through the hook's sum, each double as three floats whose sum it is) and add them in rank
// order.  sx: [3 * k * world]; what: the statistics' name for the error text
static int32_t sum_rank_sums(double* st, int k, DevBuf<float>& sx, int32_t rank, int32_t world, ppo_allreduce_fn allreduce,
                             void* allreduce_ctx, const char* what) {
    const size_t row = (size_t)3 * k;
    std::vector<float> hx(row * world, 0.0f);
    for (int q = 0; q < k; ++q) {
        float* d = hx.data() + row * (size_t)rank + 3 * q;
        d[0] = (float)st[q];
        if (std::isfinite(st[q]) && std::isfinite(d[0])) {
            const double r1 = st[q] - (double)d[0];
            d[1] = (float)r1; d[2] = (float)(r1 - (double)d[1]);
        }
    }
    PPO_TRY(h2d(sx.p, hx.data(), hx.size()));
    if (allreduce(allreduce_ctx, sx.p, (int64_t)hx.size()) != 0) { ppo_set_error(std::string("all-reduce hook failed (") + what + ")"); return PPO_ERR_ARG; }
    PPO_TRY(d2h(hx.data(), sx.p, hx.size()));
    for (int q = 0; q < k; ++q) {
        st[q] = 0.0;
        for (int32_t r = 0; r < world; ++r) {
            const float* d = hx.data() + row * (size_t)r + 3 * q;
            st[q] += ((double)d[0] + (double)d[1]) + (double)d[2];
        }
    }
    return PPO_OK;
}

// The epoch loop of ppo_train and ppo_value_train, after their own argument checks: num_epochs passes over a fresh
// permutation of the dataset in minibatches of batch_size, an optimiser step after each.  hist0 / hist1: per-epoch means of
// the two per-batch loss columns (ppo and entropy loss; a critic's mse is column 0).  world > 1: data-parallel, through the
// all-reduce hook.  Objective::Policy adds the per-epoch ratio statistics and the target_kl stop, Objective::Value the per-epoch
// value-clip statistics while the critic handle has a value clip; with world > 1 either kind is summed over the ranks.
// Objective::Imitate and Objective::Distill keep no statistics of either kind, leave the handle's as they are and never stop early.
// Objective::PolicyAnchored is Objective::Policy in all of this and adds the per-epoch mean anchor KL and PPO's coefficient rule
// (DESIGN.md 7r): every minibatch's forward stores its divergences in its slice of one column, one reduction per epoch reads it;
// the coefficient starts from the handle's, is adapted on the host behind every epoch while the handle has an anchor target, and
// the adapted value goes back to the handle.  With world > 1 the rule reads the sums of all ranks, so every rank keeps the same
// coefficient
static int32_t train_epochs(ppo_policy_s* net, ppo_adam_s* opt, ppo_rollouts_s* ro, const TrainObjective& obj, int64_t batch_size,
                            int32_t num_epochs, const int64_t* perm, uint64_t seed, int32_t rank, int32_t world,
                            ppo_allreduce_fn allreduce, void* allreduce_ctx, double* hist0, double* hist1, double* lr_hist) {
    const int64_t len = ro->len;
    // every rank derives from all shard lengths the SAME number of optimiser steps and the exact global minibatch size of
    // each step.  A rank whose shard is exhausted contributes a zero gradient to the remaining steps, so all ranks issue the
    // same collectives.
    std::vector<int64_t> lens((size_t)world, len);
    if (world > 1) PPO_TRY(exchange_shard_lengths(lens, rank, allreduce, allreduce_ctx));
    int64_t nb = 0, min_len = len;
    for (int64_t l : lens) { nb = std::max(nb, (l + batch_size - 1) / batch_size); min_len = std::min(min_len, l); }
    ARG_CHECK(batch_size <= min_len, "1 <= batch_size <= num_data (src/train.jl:88) on every data-parallel shard");
    PPO_TRY(train_reserve(net, batch_size * (ro->H / 32)));
    DevBuf<int32_t> order; DevBuf<int64_t> permd; DevBuf<float> hist;
    PPO_TRY(order.alloc(len));
    if (perm) PPO_TRY(permd.alloc(len));
    PPO_TRY(hist.alloc((size_t)nb * 2));
    std::vector<float> hh((size_t)nb * 2);
    // per-epoch statistics of the policy's probability ratios (ppo_stats.hip), while a target_kl is set: every minibatch's
    // train forward stores its ratios in its slice of one column, one reduction per epoch reads the column, its four sums come
    // back with the loss history.  target_kl == 0: nothing is stored, launched or copied, the statistics are NaN
    const bool anchored = obj.kind == Objective::PolicyAnchored;
    const bool policy = obj.kind == Objective::Policy || anchored;
    // likewise for a critic while a value clip is set: V - vold of every minibatch in its slice of one column, one reduction per
    // epoch (count(|delta| > c), sum delta^2, n).  value_clip == 0: nothing is allocated, stored, launched or copied
    const bool value = obj.kind == Objective::Value;
    const bool vstats = value && net->value_clip != 0.0;
    if (value) {
        if (vstats) {
            if (net->vdelta_col.n < (size_t)len) net->vdelta_n = 0;
            PPO_TRY(net->vdelta_col.alloc((size_t)len));
            PPO_TRY(net->stats_part.alloc(stats_part_doubles()));
        }
        net->vstats_clip.clear(); net->vstats_msq.clear();
    }
    DevBuf<float> sx;                                                  // the ranks' sums, three floats per double
    if (world > 1 && vstats) PPO_TRY(sx.alloc((size_t)9 * world));
    const double target_kl = policy ? net->target_kl : 0.0;
    const bool stats = target_kl != 0.0;
    if (policy) {
        if (stats) {
            if (net->ratio_col.n < (size_t)len) { net->ratio_last = nullptr; net->ratio_last_n = 0; }
            PPO_TRY(net->ratio_col.alloc((size_t)len));
            PPO_TRY(net->stats_part.alloc(stats_part_doubles()));
        }
        net->stats_kl.clear(); net->stats_old_kl.clear(); net->stats_clip.clear(); net->stats_stopped = 0;
        if (world > 1 && target_kl > 0) PPO_TRY(sx.alloc((size_t)12 * world));
        net->astats_kl.clear(); net->astats_coef.clear();
    }
    double coef = obj.anchor_coef;                                     // the coefficient of the epoch at hand
    if (anchored) {
        if (net->anchor_col.n < (size_t)len) { net->anchor_last = nullptr; net->anchor_last_n = 0; }
        PPO_TRY(net->anchor_col.alloc((size_t)len));
        PPO_TRY(net->stats_part.alloc(stats_part_doubles()));
        if (world > 1) PPO_TRY(sx.alloc((size_t)std::max(6, target_kl > 0 ? 12 : 6) * world));
    }
    for (int32_t ep = 0; ep < num_epochs; ++ep) {
        if (perm) {                                                    // randperm(num_data)  src/train.jl:93
            PPO_TRY(h2d(permd.p, perm + (size_t)ep * len, (size_t)len));
            PPO_TRY(launch_gather_index(ro, permd.p, len, order.p, net->err.p));
        } else {
            // keyed by (seed, epochs this optimiser has trained): no process-global state, so the same seed with a
            // fresh optimiser reproduces the run and a restored optimiser (ppo_adam_set_epoch_count) resumes it
            PPO_TRY(launch_feistel_index(ro->index.p, len, seed, (uint32_t)opt->epochs_done, order.p));
        }
        for (int64_t b = 0; b < nb; ++b) {                                          // :95-96 (last batch may be short)
            const int64_t start = b * batch_size;
            const int64_t B = std::max<int64_t>(0, std::min(batch_size, len - start));
            int64_t Bg = 0;
            for (int64_t l : lens) Bg += std::max<int64_t>(0, std::min(batch_size, l - start));
            // single-rank training: Adam and the re-pack ride in the slab-reduction launch (PPO_FUSE_REDUCE_ADAM=0: separate launches)
            const bool fused = ppo_knobs().fuse_reduce_adam && !allreduce && B > 0;
            TrainObjective o = obj;
            o.ratio_dst = stats ? net->ratio_col.p + start : nullptr;
            o.vdelta_dst = vstats ? net->vdelta_col.p + start : nullptr;
            if (anchored) { o.anchor_dst = net->anchor_col.p + start; o.anchor_coef = coef; }
            if (B > 0) PPO_TRY(train_pass_dev(net, ro, order.p + start, B, Bg, o, fused ? opt : nullptr, hist.p + 2 * b));
            else HIP_TRY(hipMemsetAsync(net->grad.p, 0, (size_t)(net->np + 2) * sizeof(float), ppo_stream()));   // shard exhausted
            if (allreduce) {                     // every rank of a data-parallel run; a world of 1 may pass it too
                ProfScope ps("allreduce");
                const int32_t s = allreduce(allreduce_ctx, net->grad.p, net->np + 2);
                if (s != 0) { ppo_set_error("all-reduce hook failed"); return PPO_ERR_ARG; }
            }
            if (!fused) PPO_TRY(launch_adam(opt, hist.p + 2 * b));                  // Flux.update!  :81 (+ loss history)
        }
        opt->epochs_done += 1;
        double st[4] = {NAN, NAN, NAN, 1.0};                                         // sum(-log r), sum((r - 1) - log r), clipped, n
        if (stats) {
            PPO_TRY(launch_ratio_stats(net->ratio_col.p, len, obj.eps, net->stats_part.p));
            net->ratio_last = net->ratio_col.p; net->ratio_last_n = len;
            HIP_TRY(hipMemcpyAsync(st, net->stats_part.p, sizeof(st), hipMemcpyDeviceToHost, ppo_stream()));   // waited for just below
        }
        double vst[3] = {NAN, NAN, 1.0};                                             // count(|delta| > c), sum delta^2, n
        if (vstats) {
            PPO_TRY(launch_value_clip_stats(net->vdelta_col.p, len, (float)net->value_clip, net->stats_part.p));
            net->vdelta_n = len;
            HIP_TRY(hipMemcpyAsync(vst, net->stats_part.p, sizeof(vst), hipMemcpyDeviceToHost, ppo_stream()));  // waited for just below
        }
        double ast[2] = {NAN, 1.0};                                                  // sum of the anchor divergences, n
        if (anchored) {
            PPO_TRY(launch_sum_stats(net->anchor_col.p, len, net->stats_part.p));    // behind the copy above, in stream order
            net->anchor_last = net->anchor_col.p; net->anchor_last_n = len;
            HIP_TRY(hipMemcpyAsync(ast, net->stats_part.p, sizeof(ast), hipMemcpyDeviceToHost, ppo_stream()));  // waited for just below
        }
        PPO_TRY(d2h(hh.data(), hist.p, (size_t)nb * 2));
        double s0 = 0.0, s1 = 0.0;
        for (int64_t i = 0; i < nb; ++i) { s0 += hh[2 * i]; s1 += hh[2 * i + 1]; }
        if (hist0) hist0[ep] = s0 / (double)nb;                                     // unweighted mean over batches :127
        if (hist1) hist1[ep] = s1 / (double)nb;
        if (lr_hist) lr_hist[ep] = opt->lr();                                       // :144,155-158
        if (value) {
            if (world > 1 && vstats) PPO_TRY(sum_rank_sums(vst, 3, sx, rank, world, allreduce, allreduce_ctx, "value-clip statistics"));
            net->vstats_clip.push_back(vst[0] / vst[2]); net->vstats_msq.push_back(vst[1] / vst[2]);
        }
        if (!policy) continue;
        if (anchored) {
            if (world > 1) PPO_TRY(sum_rank_sums(ast, 2, sx, rank, world, allreduce, allreduce_ctx, "anchor statistics"));
            const double akl = ast[0] / ast[1];
            net->astats_kl.push_back(akl); net->astats_coef.push_back(coef);
            // PPO's rule (Schulman et al. 2017, section 4) around the handle's target d: above 1.5 d the coefficient doubles,
            // below d / 1.5 it halves (a NaN mean compares false twice and leaves it)
            const double d = net->anchor_target;
            if (d > 0.0) {
                if (akl > 1.5 * d && std::isfinite(coef * 2.0)) coef *= 2.0;
                else if (akl < d / 1.5) coef /= 2.0;
                net->anchor_coef = coef;
            }
        }
        if (world > 1 && target_kl > 0) PPO_TRY(sum_rank_sums(st, 4, sx, rank, world, allreduce, allreduce_ctx, "ratio statistics"));
        const double kl = st[1] / st[3];
        net->stats_kl.push_back(kl); net->stats_old_kl.push_back(st[0] / st[3]); net->stats_clip.push_back(st[2] / st[3]);
        if (target_kl > 0 && !(kl <= target_kl)) {          // Inf and NaN stop too; this epoch's updates stay applied
            net->stats_stopped = ep + 1 < num_epochs ? 1 : 0;
            break;
        }
    }
    int32_t f = 0;
    PPO_TRY(d2h(&f, net->err.p, 1));
    if (f) { ppo_set_error("AssertionError (device flag): permutation / dataset index out of range"); return PPO_ERR_DEVICE_FLAG; }
    return PPO_OK;
}

int32_t ppo_train(ppo_policy_t pol, ppo_adam_t opt, ppo_rollouts_t ro, double epsilon, int64_t batch_size,
                  int32_t num_epochs, double entropy_weight, int32_t adv_mode, const int64_t* perm, uint64_t seed,
                  int32_t rank, int32_t world, ppo_allreduce_fn allreduce, void* allreduce_ctx, double* ppo_hist,
                  double* entropy_hist, double* lr_hist) {
    ARG_CHECK(pol && opt && ro && opt->pol == pol, "ppo_train!: null/mismatched argument");
    ARG_CHECK(num_epochs >= 0 && world >= 1 && rank >= 0 && rank < world, "ppo_train!: bad epochs/rank/world");
    ARG_CHECK(world == 1 || allreduce, "ppo_train!: world > 1 needs an all-reduce hook");
    ARG_CHECK(pol->F == ro->F && (ro->H == 32 || ro->H == 128), "ppo_train!: shape mismatch");
    ARG_CHECK(batch_size >= 1, "1 <= batch_size <= num_data (src/train.jl:88)");
    if (adv_mode < PPO_ADV_RETURNS || adv_mode > PPO_ADV_GAE_NORMALISED) { ppo_set_error("batch_advantage: unknown advantage mode"); return PPO_ERR_UNSUPPORTED; }
    TrainObjective obj = {Objective::Policy};
    obj.eps = epsilon; obj.entropy_weight = entropy_weight; obj.adv_mode = adv_mode;
    PPO_TRY(anchor_objective("ppo_train!", pol, ro, obj));
    return train_epochs(pol, opt, ro, obj, batch_size, num_epochs, perm, seed, rank, world, allreduce, allreduce_ctx, ppo_hist,
                        entropy_hist, lr_hist);
}


// ---- behaviour cloning (no reference op): the policy's cross-entropy on the buffer's actions
// what both entry points check of their two mode arguments: the weights' column is read in the weighted form only
static int32_t imitate_modes(int32_t weight_mode, int32_t adv_mode) {
    if (weight_mode != PPO_IMITATE_UNIFORM && weight_mode != PPO_IMITATE_POSITIVE_ADVANTAGE) { ppo_set_error("imitation: unknown weight mode"); return PPO_ERR_UNSUPPORTED; }
    if (adv_mode < PPO_ADV_RETURNS || adv_mode > PPO_ADV_GAE_NORMALISED) { ppo_set_error("batch_advantage: unknown advantage mode"); return PPO_ERR_UNSUPPORTED; }
    if (adv_mode == PPO_ADV_RETURNS_NORMALISED || adv_mode == PPO_ADV_GAE_NORMALISED) {
        ppo_set_error("imitation: the weights are max(advantage, 0) of the returns or the GAE column; the normalised advantage modes are not supported");
        return PPO_ERR_UNSUPPORTED;
    }
    return PPO_OK;
}

int32_t ppo_imitate_forward_backward(ppo_policy_t pol, ppo_rollouts_t ro, const int64_t* sample_idx, int64_t B, int64_t B_global,
                                     double entropy_weight, int32_t weight_mode, int32_t adv_mode) {
    ARG_CHECK(pol && ro && sample_idx, "imitate_forward_backward: null argument");
    ARG_CHECK(B >= 1 && B <= ro->len, "imitate_forward_backward: 1 <= batch_size <= num_data (src/train.jl:88)");
    ARG_CHECK(B_global >= B, "imitate_forward_backward: B_global < B");
    ARG_CHECK(pol->F == ro->F && (ro->H == 32 || ro->H == 128), "imitate_forward_backward: shape mismatch");
    PPO_TRY(imitate_modes(weight_mode, adv_mode));
    DevBuf<int64_t> pos;
    PPO_TRY(gather_minibatch(pol, ro, sample_idx, B, pos));
    TrainObjective obj = {Objective::Imitate};
    obj.entropy_weight = entropy_weight; obj.adv_mode = adv_mode; obj.weight_mode = weight_mode;
    PPO_TRY(train_pass_dev(pol, ro, pol->idx.p, B, B_global, obj));
    HIP_TRY(hipStreamSynchronize(ppo_stream()));
    return PPO_OK;
}

int32_t ppo_imitate_train(ppo_policy_t pol, ppo_adam_t opt, ppo_rollouts_t ro, int64_t batch_size, int32_t num_epochs,
                          double entropy_weight, int32_t weight_mode, int32_t adv_mode, const int64_t* perm, uint64_t seed,
                          int32_t rank, int32_t world, ppo_allreduce_fn allreduce, void* allreduce_ctx, double* ce_hist,
                          double* entropy_hist, double* lr_hist) {
    ARG_CHECK(pol && opt && ro && opt->pol == pol, "imitate_train!: null/mismatched argument");
    ARG_CHECK(num_epochs >= 0 && world >= 1 && rank >= 0 && rank < world, "imitate_train!: bad epochs/rank/world");
    ARG_CHECK(world == 1 || allreduce, "imitate_train!: world > 1 needs an all-reduce hook");
    ARG_CHECK(pol->F == ro->F && (ro->H == 32 || ro->H == 128), "imitate_train!: shape mismatch");
    ARG_CHECK(batch_size >= 1, "1 <= batch_size <= num_data (src/train.jl:88)");
    PPO_TRY(imitate_modes(weight_mode, adv_mode));
    TrainObjective obj = {Objective::Imitate};
    obj.entropy_weight = entropy_weight; obj.adv_mode = adv_mode; obj.weight_mode = weight_mode;
    return train_epochs(pol, opt, ro, obj, batch_size, num_epochs, perm, seed, rank, world, allreduce, allreduce_ctx, ce_hist,
                        entropy_hist, lr_hist);
}

// ---- policy distillation (no reference op): the policy's cross-entropy against a target distribution per state
// The target column [T*N][A], full_probs' layout, by transition id; every call that writes new transitions into the buffer
// marks it not filled (rollouts_filled)
static int32_t targets_checks(const char* who, const ppo_rollouts_s* ro) {
    ARG_CHECK(ro->T >= 1, std::string(who) + ": empty rollout buffer");
    if (ro->sink) {
        ppo_set_error(std::string(who) + ": a buffer with a disk sink attached is not supported");
        return PPO_ERR_UNSUPPORTED;
    }
    return PPO_OK;
}

int32_t ppo_rollouts_fill_targets(ppo_policy_t teacher, ppo_rollouts_t ro) {
    ARG_CHECK(teacher && ro, "fill_targets: null argument");
    PPO_TRY(targets_checks("fill_targets", ro));
    ARG_CHECK(ro->H == 32 || ro->H == 128, "fill_targets: shape mismatch");
    ARG_CHECK(teacher->F == ro->F, "fill_targets: the teacher's input width F differs from the buffer's");
    ARG_CHECK(teacher->OUT == PPO_OUT && ro->A == PPO_OUT * ro->H, "fill_targets: the teacher must have 4 outputs per half-edge row");
    if (ro->compact && teacher->dtype != PPO_DTYPE_F32) {
        ppo_set_error("fill_targets: a bf16-dtype teacher on a compact buffer is not supported (the probabilities forward from env "
                      "snapshots exists in the fp32-MFMA forward only); collect with expanded storage");
        return PPO_ERR_UNSUPPORTED;
    }
    const int64_t n = ro->T * ro->N;
    PPO_TRY(ro->targets.alloc((size_t)ro->capT * ro->N * ro->A));
    ro->targets_T = -1;
    if (ro->compact) PPO_TRY(launch_policy_probs_snap(teacher, ro->cstate.p, ro->active.p, ro->tmpl.p, ro->V, n, ro->H, ro->targets.p));
    else PPO_TRY(launch_policy_probs(teacher, ro->states.p, ro->active.p, n, ro->H, ro->targets.p));
    HIP_TRY(hipStreamSynchronize(ppo_stream()));
    ro->targets_T = ro->T;
    return PPO_OK;
}

int32_t ppo_rollouts_set_targets(ppo_rollouts_t ro, const float* targets) {
    ARG_CHECK(ro && targets, "set_targets: null argument");
    PPO_TRY(targets_checks("set_targets", ro));
    const size_t n = (size_t)ro->T * ro->N * ro->A;
    for (size_t i = 0; i < n; ++i) ARG_CHECK(std::isfinite(targets[i]) && targets[i] >= 0.0f, "set_targets: every target entry must be finite and >= 0");
    PPO_TRY(ro->targets.alloc((size_t)ro->capT * ro->N * ro->A));
    ro->targets_T = -1;
    PPO_TRY(h2d(ro->targets.p, targets, n));
    ro->targets_T = ro->T;
    return PPO_OK;
}

int32_t ppo_rollouts_get_targets(ppo_rollouts_t ro, float* targets_out) {
    ARG_CHECK(ro && targets_out, "get_targets: null argument");
    ARG_CHECK(ro->targets.p && ro->targets_T == ro->T && ro->T >= 1, "get_targets: the target column is not filled for these rollouts (ppo_rollouts_fill_targets or ppo_rollouts_set_targets first)");
    return d2h(targets_out, ro->targets.p, (size_t)ro->T * ro->N * ro->A);
}

// what both entry points check of the buffer and their mode arguments -> the target rows
static int32_t distill_targets(ppo_rollouts_s* ro, int32_t weight_mode, int32_t adv_mode, int32_t target_source, const float** col) {
    if (weight_mode != PPO_IMITATE_UNIFORM && weight_mode != PPO_IMITATE_POSITIVE_ADVANTAGE) { ppo_set_error("distill: unknown weight mode"); return PPO_ERR_UNSUPPORTED; }
    if (adv_mode < PPO_ADV_RETURNS || adv_mode > PPO_ADV_GAE_NORMALISED) { ppo_set_error("batch_advantage: unknown advantage mode"); return PPO_ERR_UNSUPPORTED; }
    if (adv_mode == PPO_ADV_RETURNS_NORMALISED || adv_mode == PPO_ADV_GAE_NORMALISED) {
        ppo_set_error("distill: the weights are max(advantage, 0) of the returns or the GAE column; the normalised advantage modes are not supported");
        return PPO_ERR_UNSUPPORTED;
    }
    if (target_source != PPO_TARGETS_COLUMN && target_source != PPO_TARGETS_RECORDED) { ppo_set_error("distill: unknown target source"); return PPO_ERR_UNSUPPORTED; }
    PPO_TRY(targets_checks("distill", ro));
    if (target_source == PPO_TARGETS_COLUMN) {
        ARG_CHECK(ro->targets.p && ro->targets_T == ro->T, "distill: the target column is not filled for these rollouts (ppo_rollouts_fill_targets or ppo_rollouts_set_targets first)");
        *col = ro->targets.p;
    } else {
        ARG_CHECK(ro->full_probs.p && ro->probs_T == ro->T, "distill: no recorded distributions for these rollouts (collect them with record_probs)");
        *col = ro->full_probs.p;
    }
    return PPO_OK;
}

int32_t ppo_distill_forward_backward(ppo_policy_t pol, ppo_rollouts_t ro, const int64_t* sample_idx, int64_t B, int64_t B_global,
                                     double entropy_weight, int32_t weight_mode, int32_t adv_mode, int32_t target_source) {
    ARG_CHECK(pol && ro && sample_idx, "distill_forward_backward: null argument");
    ARG_CHECK(B >= 1 && B <= ro->len, "distill_forward_backward: 1 <= batch_size <= num_data (src/train.jl:88)");
    ARG_CHECK(B_global >= B, "distill_forward_backward: B_global < B");
    ARG_CHECK(pol->F == ro->F && (ro->H == 32 || ro->H == 128), "distill_forward_backward: shape mismatch");
    TrainObjective obj = {Objective::Distill};
    PPO_TRY(distill_targets(ro, weight_mode, adv_mode, target_source, &obj.distill_targets));
    DevBuf<int64_t> pos;
    PPO_TRY(gather_minibatch(pol, ro, sample_idx, B, pos));
    obj.entropy_weight = entropy_weight; obj.adv_mode = adv_mode; obj.weight_mode = weight_mode;
    PPO_TRY(train_pass_dev(pol, ro, pol->idx.p, B, B_global, obj));
    HIP_TRY(hipStreamSynchronize(ppo_stream()));
    return PPO_OK;
}

int32_t ppo_distill_train(ppo_policy_t pol, ppo_adam_t opt, ppo_rollouts_t ro, int64_t batch_size, int32_t num_epochs,
                          double entropy_weight, int32_t weight_mode, int32_t adv_mode, int32_t target_source, const int64_t* perm,
                          uint64_t seed, int32_t rank, int32_t world, ppo_allreduce_fn allreduce, void* allreduce_ctx,
                          double* ce_hist, double* entropy_hist, double* lr_hist) {
    ARG_CHECK(pol && opt && ro && opt->pol == pol, "distill_train!: null/mismatched argument");
    ARG_CHECK(num_epochs >= 0 && world >= 1 && rank >= 0 && rank < world, "distill_train!: bad epochs/rank/world");
    ARG_CHECK(world == 1 || allreduce, "distill_train!: world > 1 needs an all-reduce hook");
    ARG_CHECK(pol->F == ro->F && (ro->H == 32 || ro->H == 128), "distill_train!: shape mismatch");
    ARG_CHECK(batch_size >= 1, "1 <= batch_size <= num_data (src/train.jl:88)");
    TrainObjective obj = {Objective::Distill};
    PPO_TRY(distill_targets(ro, weight_mode, adv_mode, target_source, &obj.distill_targets));
    obj.entropy_weight = entropy_weight; obj.adv_mode = adv_mode; obj.weight_mode = weight_mode;
    return train_epochs(pol, opt, ro, obj, batch_size, num_epochs, perm, seed, rank, world, allreduce, allreduce_ctx, ce_hist,
                        entropy_hist, lr_hist);
}

// ---- per-epoch KL / clip-fraction statistics and target-KL early stopping (no reference op)
int32_t ppo_policy_set_target_kl(ppo_policy_t pol, double target_kl) {
    ARG_CHECK(target_kl >= 0.0, "policy_set_target_kl: target_kl must be 0 (off), positive or +inf");    // NaN fails it too
    ARG_CHECK(pol, "policy_set_target_kl: null policy");
    pol->target_kl = target_kl;
    return PPO_OK;
}
int32_t ppo_policy_get_target_kl(ppo_policy_t pol, double* target_kl) {
    ARG_CHECK(pol && target_kl, "policy_get_target_kl: null argument");
    *target_kl = pol->target_kl;
    return PPO_OK;
}
int32_t ppo_policy_last_train_stats(ppo_policy_t pol, int32_t cap, int32_t* epochs_run, int32_t* stopped_early,
                                    double* approx_kl, double* old_approx_kl, double* clip_fraction) {
    ARG_CHECK(pol && cap >= 0, "policy_last_train_stats: null policy or negative capacity");
    const size_t n = pol->stats_kl.size(), m = std::min(n, (size_t)cap);
    if (epochs_run) *epochs_run = (int32_t)n;
    if (stopped_early) *stopped_early = pol->stats_stopped;
    for (size_t i = 0; i < m; ++i) {
        if (approx_kl) approx_kl[i] = pol->stats_kl[i];
        if (old_approx_kl) old_approx_kl[i] = pol->stats_old_kl[i];
        if (clip_fraction) clip_fraction[i] = pol->stats_clip[i];
    }
    return PPO_OK;
}

// ---- KL anchor (no reference op): a property of the policy handle
int32_t ppo_policy_set_kl_anchor(ppo_policy_t pol, double coef, int32_t source, double target) {
    // (the arguments are judged before the handle, like ppo_policy_set_target_kl's)
    if (source != PPO_ANCHOR_OFF && source != PPO_TARGETS_COLUMN && source != PPO_TARGETS_RECORDED) { ppo_set_error("policy_set_kl_anchor: unknown target source"); return PPO_ERR_UNSUPPORTED; }
    if (source != PPO_ANCHOR_OFF) {
        ARG_CHECK(coef >= 0.0 && std::isfinite(coef), "policy_set_kl_anchor: the coefficient must be finite and >= 0");      // NaN fails it too
        ARG_CHECK(target >= 0.0 && std::isfinite(target), "policy_set_kl_anchor: the target must be 0 (fixed coefficient) or positive and finite");
    }
    ARG_CHECK(pol, "policy_set_kl_anchor: null policy");
    if (source == PPO_ANCHOR_OFF) { pol->anchor_source = PPO_ANCHOR_OFF; pol->anchor_coef = 0.0; pol->anchor_target = 0.0; return PPO_OK; }
    pol->anchor_coef = coef; pol->anchor_source = source; pol->anchor_target = target;
    return PPO_OK;
}
int32_t ppo_policy_get_kl_anchor(ppo_policy_t pol, double* coef, int32_t* source, double* target) {
    ARG_CHECK(pol, "policy_get_kl_anchor: null policy");
    if (coef) *coef = pol->anchor_coef;
    if (source) *source = pol->anchor_source;
    if (target) *target = pol->anchor_target;
    return PPO_OK;
}
int32_t ppo_policy_last_anchor_stats(ppo_policy_t pol, int32_t cap, int32_t* n, double* kl, double* coef) {
    ARG_CHECK(pol && cap >= 0, "policy_last_anchor_stats: null policy or negative capacity");
    const size_t k = pol->astats_kl.size(), m = std::min(k, (size_t)cap);
    if (n) *n = (int32_t)k;
    for (size_t i = 0; i < m; ++i) {
        if (kl) kl[i] = pol->astats_kl[i];
        if (coef) coef[i] = pol->astats_coef[i];
    }
    return PPO_OK;
}

// diagnostic for the tests (not part of include/ppo_hip.h), like ppo_debug_train_ratios: the anchor divergence per state the
// anchored loss tail stored -- of the latest forward in minibatch order, or, after ppo_train, of its latest epoch in the order
// of that epoch's permutation
int32_t ppo_debug_anchor_kl(ppo_policy_t pol, int64_t n, float* out) {
    ARG_CHECK(pol && out, "ppo_debug_anchor_kl: null argument");
    ARG_CHECK(pol->anchor_last && n >= 1 && n <= pol->anchor_last_n, "ppo_debug_anchor_kl: no divergences stored, or n out of range");
    return d2h(out, pol->anchor_last, (size_t)n);
}

// ---- PPO's clipped value loss for a critic (no reference op): the clip range is a property of the handle
int32_t ppo_policy_set_value_clip(ppo_policy_t critic, double clip) {
    ARG_CHECK(clip >= 0.0, "policy_set_value_clip: value_clip must be 0 (off), positive or +inf");        // NaN fails it too
    ARG_CHECK(critic, "policy_set_value_clip: null policy");
    critic->value_clip = clip;
    return PPO_OK;
}
int32_t ppo_policy_get_value_clip(ppo_policy_t critic, double* clip) {
    ARG_CHECK(critic && clip, "policy_get_value_clip: null argument");
    *clip = critic->value_clip;
    return PPO_OK;
}
int32_t ppo_policy_last_value_stats(ppo_policy_t critic, int32_t cap, int32_t* epochs_run, double* clip_fraction,
                                    double* mean_sq_change) {
    ARG_CHECK(critic && cap >= 0, "policy_last_value_stats: null policy or negative capacity");
    const size_t n = critic->vstats_clip.size(), m = std::min(n, (size_t)cap);
    if (epochs_run) *epochs_run = (int32_t)n;
    for (size_t i = 0; i < m; ++i) {
        if (clip_fraction) clip_fraction[i] = critic->vstats_clip[i];
        if (mean_sq_change) mean_sq_change[i] = critic->vstats_msq[i];
    }
    return PPO_OK;
}

// diagnostic for the tests (not part of include/ppo_hip.h), like ppo_debug_train_ratios: V - vold of every state of the latest
// epoch of the latest ppo_value_train that ran with a value clip, in the order of that epoch's permutation (n up to the
// dataset length)
int32_t ppo_debug_value_deltas(ppo_policy_t critic, int64_t n, float* out) {
    ARG_CHECK(critic && out, "ppo_debug_value_deltas: null argument");
    ARG_CHECK(critic->vdelta_n > 0 && n >= 1 && n <= critic->vdelta_n, "ppo_debug_value_deltas: no deltas stored, or n out of range");
    return d2h(out, critic->vdelta_col.p, (size_t)n);
}

// ================================================================ critic
// A critic is a ppo_policy_t read as a state value (include/ppo_hip.h): the refusals every value entry point shares
int32_t value_checks(const char* who, ppo_policy_s* critic, int32_t F) {
    if (critic->dtype != PPO_DTYPE_F32) {
        ppo_set_error(std::string(who) + ": a bf16-dtype critic is not supported (the value modes exist in the fp32-MFMA forward only)");
        return PPO_ERR_UNSUPPORTED;
    }
    if (critic->F != F) {
        ppo_set_error(std::string(who) + ": the critic's input width F = " + std::to_string(critic->F) + " differs from the buffer's F = " + std::to_string(F));
        return PPO_ERR_UNSUPPORTED;
    }
    return PPO_OK;
}

// a value clip needs the values the critic had before the update: the buffer's, of these rollouts
static int32_t value_clip_check(const ppo_policy_s* critic, const ppo_rollouts_s* ro) {
    if (critic->value_clip == 0.0) return PPO_OK;
    ARG_CHECK(ro->values.p && ro->values_T == ro->T, "value clipping needs ppo_rollouts_compute_values or ppo_rollouts_compute_gae on these rollouts first");
    return PPO_OK;
}

int32_t ppo_value_forward(ppo_policy_t critic, const int8_t* states, const uint32_t* active, int64_t B, int32_t H, float* values) {
    ARG_CHECK(critic && states && active && values, "state_values: null argument");
    ARG_CHECK(B >= 1, "state_values: empty batch");
    if (H != 32 && H != 128) { ppo_set_error("value_forward: H must be 32 (Q=8) or 128 (Q=32) half-edges in this build"); return PPO_ERR_UNSUPPORTED; }
    PPO_TRY(value_checks("value_forward", critic, critic->F));
    DevBuf<int8_t> s; DevBuf<uint32_t> a; DevBuf<float> v;
    const size_t ns = (size_t)B * H * critic->F;
    PPO_TRY(s.alloc(ns)); PPO_TRY(a.alloc(B)); PPO_TRY(v.alloc(B));
    PPO_TRY(h2d(s.p, states, ns)); PPO_TRY(h2d(a.p, active, (size_t)B));
    PPO_TRY(launch_value_predict(critic, s.p, nullptr, a.p, nullptr, 0, B, H, v.p));
    return d2h(values, v.p, (size_t)B);
}

// ro->values [T+1][N] on the device: rows 0 .. T-1 from the stored states (one launch, either storage form), row T from the
// envs' current observation (zeros without an env)
static int32_t compute_values_dev(const char* who, ppo_rollouts_s* ro, ppo_env_s* env, ppo_policy_s* critic) {
    ARG_CHECK(ro->T >= 1, "compute_values: empty rollout buffer");
    ARG_CHECK(ro->H == 32 || ro->H == 128, "compute_values: shape mismatch");
    PPO_TRY(value_checks(who, critic, ro->F));
    if (env) ARG_CHECK(ro->N == env->N && ro->H == env->H && ro->F == env->F, "compute_values: rollouts were created for another env shape");
    const size_t n = (size_t)ro->T * ro->N;
    PPO_TRY(ro->values.alloc((size_t)(ro->capT + 1) * ro->N));
    PPO_TRY(launch_value_predict(critic, ro->compact ? nullptr : ro->states.p, ro->compact ? ro->cstate.p : nullptr, ro->active.p,
                                 ro->tmpl.p, ro->V, (int64_t)n, ro->H, ro->values.p));
    if (env) {
        PPO_TRY(env->obs_tmp.alloc((size_t)env->N * env->H * env->F));
        PPO_TRY(launch_env_observe(env, env->obs_tmp.p, nullptr));
        PPO_TRY(launch_value_predict(critic, env->obs_tmp.p, nullptr, env->active.p, nullptr, 0, env->N, env->H, ro->values.p + n));
    } else {
        HIP_TRY(hipMemsetAsync(ro->values.p + n, 0, (size_t)ro->N * sizeof(float), ppo_stream()));
    }
    ro->values_T = ro->T;
    return PPO_OK;
}

int32_t ppo_rollouts_compute_values(ppo_rollouts_t ro, ppo_env_t env, ppo_policy_t critic, float* values_out) {
    ARG_CHECK(ro && critic, "compute_values: null argument");
    PPO_TRY(compute_values_dev("compute_values", ro, env, critic));
    if (values_out) return d2h(values_out, ro->values.p, (size_t)(ro->T + 1) * ro->N);
    HIP_TRY(hipStreamSynchronize(ppo_stream()));
    return PPO_OK;
}

int32_t ppo_rollouts_compute_gae_critic(ppo_rollouts_t ro, ppo_env_t env, ppo_policy_t critic, double gamma, double lambda,
                                        float* adv_out, float* lambda_returns_out) {
    ARG_CHECK(ro && critic, "compute_gae_critic: null argument");
    PPO_TRY(compute_values_dev("compute_gae_critic", ro, env, critic));
    const size_t n = (size_t)ro->T * ro->N;
    PPO_TRY(ro->adv.alloc((size_t)ro->capT * ro->N)); PPO_TRY(ro->lam_ret.alloc((size_t)ro->capT * ro->N));
    PPO_TRY(launch_gae_tn(ro->rewards.p, ro->done.p, ro->values.p, ro->adv.p, ro->lam_ret.p, ro->T, ro->N, gamma, lambda));
    ro->adv_T = ro->T;
    if (adv_out) PPO_TRY(d2h(adv_out, ro->adv.p, n));
    if (lambda_returns_out) PPO_TRY(d2h(lambda_returns_out, ro->lam_ret.p, n));
    HIP_TRY(hipStreamSynchronize(ppo_stream()));
    return PPO_OK;
}

// the replay needs the built-in env's buffer: its template, and the snapshot (or the rows it can be read back from)
static int32_t truncation_checks(const char* who, const ppo_rollouts_s* ro) {
    ARG_CHECK(ro->T >= 1, "truncated: empty rollout buffer");
    if (ro->V == 0 || !ro->tmpl.p) {
        ppo_set_error(std::string(who) + ": the buffer has no env template, so its final states cannot be replayed; pass final values of your own to ppo_rollouts_compute_gae_boot");
        return PPO_ERR_UNSUPPORTED;
    }
    ARG_CHECK((ro->V == 32 || ro->V == 128) && ro->H == ro->V && ro->F == 2 * PPO_TPL, "truncated: shape mismatch");
    ARG_CHECK(ro->compact ? ro->cstate.p != nullptr : ro->states.p != nullptr, "truncated: the buffer holds no states");
    return PPO_OK;
}

// flags, ids and K (the one count that crosses), then the K post-step snapshots in ro->boot_cstate / boot_active
static int32_t truncated_dev(ppo_rollouts_s* ro, int64_t* K) {
    PPO_TRY(launch_truncated(ro, K));
    ARG_CHECK(*K >= 0 && *K <= ro->T * ro->N, "truncated: count out of range");
    PPO_TRY(ro->boot_cstate.alloc((size_t)*K * 2 * ro->V)); PPO_TRY(ro->boot_active.alloc((size_t)*K));
    return launch_truncated_states(ro, *K, ro->boot_cstate.p, ro->boot_active.p);
}

int32_t ppo_rollouts_truncated(ppo_rollouts_t ro, uint8_t* truncated_out, int8_t* final_states_out, uint32_t* final_active_out,
                               int64_t capacity, int64_t* count_out) {
    ARG_CHECK(ro && count_out, "truncated: null argument");
    ARG_CHECK(capacity >= 0, "truncated: negative capacity");
    PPO_TRY(truncation_checks("truncated", ro));
    int64_t K = 0;
    PPO_TRY(truncated_dev(ro, &K));
    *count_out = K;
    if (truncated_out) PPO_TRY(d2h(truncated_out, ro->truncated.p, (size_t)ro->T * ro->N));
    if (final_states_out || final_active_out) ARG_CHECK(capacity >= K, "truncated: capacity is below the number of truncated transitions");
    if (final_states_out && K > 0) {       // observations re-derived from the snapshots on the device, <= 256 MiB at a time
        const size_t per = (size_t)ro->H * ro->F, total = (size_t)K;
        const size_t chunk = std::max<size_t>(1, std::min(total, ((size_t)256 << 20) / per));
        PPO_TRY(ro->expand_tmp.alloc(chunk * per));
        for (size_t o = 0; o < total; o += chunk) {
            const size_t c = std::min(chunk, total - o);
            PPO_TRY(launch_expand_states(ro->boot_cstate.p + o * 2 * ro->V, ro->boot_active.p + o, ro->tmpl.p, (int64_t)c, ro->V / 4, ro->expand_tmp.p));
            PPO_TRY(d2h(final_states_out + o * per, ro->expand_tmp.p, c * per));
        }
    }
    if (final_active_out) PPO_TRY(d2h(final_active_out, ro->boot_active.p, (size_t)K));
    HIP_TRY(hipStreamSynchronize(ppo_stream()));
    return PPO_OK;
}

int32_t ppo_rollouts_compute_gae_critic_boot(ppo_rollouts_t ro, ppo_env_t env, ppo_policy_t critic, double gamma, double lambda,
                                             float* adv_out, float* lambda_returns_out, int64_t* n_truncated_out) {
    ARG_CHECK(ro && critic, "compute_gae_critic_boot: null argument");
    PPO_TRY(truncation_checks("compute_gae_critic_boot", ro));
    PPO_TRY(compute_values_dev("compute_gae_critic_boot", ro, env, critic));
    const size_t n = (size_t)ro->T * ro->N;
    int64_t K = 0;
    PPO_TRY(truncated_dev(ro, &K));
    PPO_TRY(ro->boot_vals.alloc((size_t)K)); PPO_TRY(ro->boot.alloc((size_t)ro->capT * ro->N));
    PPO_TRY(launch_value_predict(critic, nullptr, ro->boot_cstate.p, ro->boot_active.p, ro->tmpl.p, ro->V, K, ro->H, ro->boot_vals.p));
    PPO_TRY(launch_boot_scatter(ro, ro->boot_vals.p, K, ro->boot.p));
    PPO_TRY(ro->adv.alloc((size_t)ro->capT * ro->N)); PPO_TRY(ro->lam_ret.alloc((size_t)ro->capT * ro->N));
    PPO_TRY(launch_gae_boot_tn(ro->rewards.p, ro->done.p, ro->values.p, ro->boot.p, ro->adv.p, ro->lam_ret.p, ro->T, ro->N, gamma, lambda));
    ro->adv_T = ro->T; ro->boot_T = ro->T;
    if (n_truncated_out) *n_truncated_out = K;
    if (adv_out) PPO_TRY(d2h(adv_out, ro->adv.p, n));
    if (lambda_returns_out) PPO_TRY(d2h(lambda_returns_out, ro->lam_ret.p, n));
    HIP_TRY(hipStreamSynchronize(ppo_stream()));
    return PPO_OK;
}

// the regression target column [T][N] of a value-training call
static int32_t value_target(ppo_rollouts_s* ro, int32_t target, const float** col) {
    if (target != PPO_VTARGET_RETURNS && target != PPO_VTARGET_LAMBDA_RETURNS) { ppo_set_error("value target: unknown target"); return PPO_ERR_UNSUPPORTED; }
    if (target == PPO_VTARGET_LAMBDA_RETURNS)
        ARG_CHECK(ro->lam_ret.p && ro->adv_T == ro->T, "value target: lambda-returns mode needs ppo_rollouts_compute_gae on these rollouts first");
    *col = target == PPO_VTARGET_RETURNS ? ro->returns.p : ro->lam_ret.p;
    return PPO_OK;
}

int32_t ppo_rollouts_value_moments(ppo_rollouts_t ro, int32_t target, double* sums5) {
    ARG_CHECK(ro && sums5, "value_moments: null argument");
    ARG_CHECK(ro->T >= 1 && ro->len >= 1, "value_moments: empty rollout buffer");
    ARG_CHECK(ro->values.p && ro->values_T == ro->T, "value_moments: needs ppo_rollouts_compute_values or ppo_rollouts_compute_gae on these rollouts first");
    const float* col = nullptr;
    PPO_TRY(value_target(ro, target, &col));
    PPO_TRY(ro->stats_part.alloc(stats_part_doubles()));
    PPO_TRY(launch_value_moments(col, ro->values.p, ro->valid.p, ro->index.p, ro->T * ro->N, ro->stats_part.p));
    return d2h(sums5, ro->stats_part.p, 5);
}

// the same sums with the two shifts k_value_moments took them relative to, so that shards can be merged: t[i0] and
// t[i0] - V[i0], i0 = the first transition of the dataset, read back as the two floats the kernel read
int32_t ppo_rollouts_value_moments_shifts(ppo_rollouts_t ro, int32_t target, double* sums5, double* shifts2) {
    ARG_CHECK(shifts2, "value_moments: null argument");
    PPO_TRY(ppo_rollouts_value_moments(ro, target, sums5));
    const float* col = nullptr;
    PPO_TRY(value_target(ro, target, &col));
    int32_t i0 = 0;
    float t0 = 0.0f, v0 = 0.0f;
    PPO_TRY(d2h(&i0, ro->index.p, 1));
    ARG_CHECK(i0 >= 0 && (int64_t)i0 < ro->T * ro->N, "value_moments: dataset index out of range");
    PPO_TRY(d2h(&t0, col + i0, 1)); PPO_TRY(d2h(&v0, ro->values.p + i0, 1));
    shifts2[0] = (double)t0; shifts2[1] = (double)t0 - (double)v0;
    return PPO_OK;
}

int32_t ppo_value_forward_backward(ppo_policy_t critic, ppo_rollouts_t ro, const int64_t* sample_idx, int64_t B,
                                   int64_t B_global, int32_t target, double* loss_out) {
    ARG_CHECK(critic && ro && sample_idx, "value_forward_backward: null argument");
    ARG_CHECK(B >= 1 && B <= ro->len, "value_forward_backward: 1 <= batch_size <= num_data");
    ARG_CHECK(B_global >= B, "value_forward_backward: B_global < B");
    ARG_CHECK(ro->H == 32 || ro->H == 128, "value_forward_backward: shape mismatch");
    PPO_TRY(value_checks("value_forward_backward", critic, ro->F));
    TrainObjective obj = {Objective::Value};
    PPO_TRY(value_target(ro, target, &obj.target_col));
    PPO_TRY(value_clip_check(critic, ro));
    DevBuf<int64_t> pos;
    PPO_TRY(gather_minibatch(critic, ro, sample_idx, B, pos));
    PPO_TRY(train_pass_dev(critic, ro, critic->idx.p, B, B_global, obj));
    if (loss_out) {
        float t = 0.0f;
        PPO_TRY(d2h(&t, critic->grad.p + critic->np, 1));
        *loss_out = t;
    }
    HIP_TRY(hipStreamSynchronize(ppo_stream()));
    return PPO_OK;
}

// the epoch loop for a critic, data-parallel like ppo_train: the handle's last_train_stats stay what the policy's ppo_train
// left; its last_value_stats are this call's, summed over the ranks.  The checks that read no handle come first
int32_t ppo_value_train_dp(ppo_policy_t critic, ppo_adam_t opt, ppo_rollouts_t ro, int64_t batch_size, int32_t num_epochs,
                           int32_t target, const int64_t* perm, uint64_t seed, int32_t rank, int32_t world,
                           ppo_allreduce_fn allreduce, void* allreduce_ctx, double* mse_hist, double* lr_hist) {
    ARG_CHECK(num_epochs >= 0 && world >= 1 && rank >= 0 && rank < world, "value_train: bad epochs/rank/world");
    ARG_CHECK(world == 1 || allreduce, "value_train: world > 1 needs an all-reduce hook");
    ARG_CHECK(critic && opt && ro && opt->pol == critic, "value_train: null/mismatched argument");
    ARG_CHECK(ro->H == 32 || ro->H == 128, "value_train: shape mismatch");
    PPO_TRY(value_checks("value_train", critic, ro->F));
    TrainObjective obj = {Objective::Value};
    PPO_TRY(value_target(ro, target, &obj.target_col));
    PPO_TRY(value_clip_check(critic, ro));
    // shards may differ in length: with world > 1 train_epochs holds batch_size against the shortest one, on every rank alike
    ARG_CHECK(batch_size >= 1 && (world > 1 || batch_size <= ro->len), "1 <= batch_size <= num_data (src/train.jl:88)");
    return train_epochs(critic, opt, ro, obj, batch_size, num_epochs, perm, seed, rank, world, allreduce, allreduce_ctx, mse_hist,
                        nullptr, lr_hist);
}

int32_t ppo_value_train(ppo_policy_t critic, ppo_adam_t opt, ppo_rollouts_t ro, int64_t batch_size, int32_t num_epochs,
                        int32_t target, const int64_t* perm, uint64_t seed, double* mse_hist, double* lr_hist) {
    return ppo_value_train_dp(critic, opt, ro, batch_size, num_epochs, target, perm, seed, 0, 1, nullptr, nullptr, mse_hist, lr_hist);
}

}  // extern "C"
