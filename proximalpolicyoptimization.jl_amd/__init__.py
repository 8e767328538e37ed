"""Host-side mirror of module ProximalPolicyOptimization (reference: src/ProximalPolicyOptimization.jl)
over the C ABI of libppo_hip.so (include/ppo_hip.h).

Julia is not available in the build image, so the host language above the C ABI is Python; the
Julia `ccall` shim a maintainer would use is julia/ProximalPolicyOptimizationHIP.jl.
Names, argument order and error behaviour follow the reference:

    Julia                                   here
    ------------------------------------    -------------------------------------------
    PPO.state / reward / is_terminal        state(env) / reward(env) / is_terminal(env)
    PPO.reset!(env) / PPO.step!(env, a)     reset_(env) / step_(env, a)          (a is 1-based)
    PPO.action_probabilities(policy, s)     action_probabilities(policy, s)
    PPO.batch_action_probabilities          batch_action_probabilities(policy, s)
    PPO.batch_state / number_of_actions_per_state / batch_advantage / save_loss   same names
    PPO.BufferRollouts()                    BufferRollouts()
    PPO.collect_rollouts!(r, env, p, n, g)  collect_rollouts_(r, env, p, n, g)
    PPO.compute_returns(r, t, g)            compute_returns(r, t, g)
    PPO.construct_dataset(r)                construct_dataset(r);  len(ds);  ds[i] / ds[[i,...]] (1-based)
    PPO.ppo_train!(...)                     ppo_train_(...)
    PPO.ppo_iterate!(...)                   ppo_iterate_(...)
    Flux.Optimiser(Adam(1e-4))              Optimiser(Adam(1e-4))
    Flux.Optimiser(Adam(), ExpDecay(...))   Optimiser(Adam(), ExpDecay(...))   (also Descent, Momentum, Nesterov, RMSProp)

Plugin functions are generic: calling one on an object that does not overload it raises
`PPOError("Function <name> needs to be overloaded")` like src/ProximalPolicyOptimization.jl:12-14.
Indices that cross this API are 1-based like the reference; the C ABI below is 0-based.
All compute runs in the HIP library; nothing here falls back to the CPU.
"""
import contextlib
import ctypes as C
import functools
import os
import shutil
import sys

import numpy as np

from . import _lib
from . import checkpoint  # noqa: F401
from . import generic  # noqa: F401
from .generic import HostDataset, HostRollouts  # noqa: F401
from ._lib import PPOError, call, lib
from .disk import (DiskDataset, DiskRollouts, bson_decode_state, bson_encode_state, export_reference_layout,  # noqa: F401
                   update_, write_returns_to_disk)

__all__ = [
    "PPOError", "HipVecEnv", "HipPolicy", "Adam", "ExpDecay", "Descent", "Momentum", "Nesterov", "RMSProp", "ClipValue", "ClipNorm", "WeightDecay", "InvDecay", "AdamW", "Optimiser", "StateData", "BufferRollouts", "BufferDataset",
    "state", "reward", "is_terminal", "reset_", "step_", "action_probabilities", "batch_action_probabilities",
    "batch_state", "number_of_actions_per_state", "batch_advantage", "save_loss", "compute_returns",
    "compute_returns_tn", "gae_tn", "gae_boot_tn", "truncated_transitions_", "compute_gae_", "profile_gae", "collect_rollouts_", "collect_rollouts_steps_", "construct_dataset",
    "simplified_ppo_clip", "get_linear_action_index", "ppo_loss_with_entropy", "categorical_sample", "step_batch_",
    "ppo_train_", "ppo_iterate_", "get_optimizer_learning_rate", "index_to_action", "action_mask", "DataParallel",
    "device_count", "average_returns", "average_best_returns", "average_normalized_returns",
    "evaluate_trajectories", "DiskRollouts", "DiskDataset", "update_", "write_returns_to_disk",
    "export_reference_layout", "load_disk_rollouts", "bson_encode_state", "bson_decode_state", "philox4x32_10", "profile_enable", "profile_get", "synchronize",
    "HostRollouts", "HostDataset", "update_rollouts_", "compute_state_value_", "collect_step_data_", "collect_episode_data_",
    "permute_", "shuffle_", "single_trajectory_return", "smoothed_entropy", "clamped_entropy", "ppo_loss", "step_epoch_",
    "save_policy", "load_policy", "forward_backward",
    "HipCritic", "state_values", "batch_state_values", "compute_values_", "compute_gae_critic_", "value_forward_backward",
    "value_train_", "pooled_state_value", "value_loss", "value_loss_clipped",
    "kl_stats", "explained_variance_", "explained_variance_from_sums",
    "check_internal", "best_states_", "best_state_in_rollout", "single_trajectory_scores", "count_non_flips",
    "search_best_states_", "search_resample_states_", "check_resample", "apply_paths_", "check_paths", "beam_search_states_",
    "beam_search_states_distinct_",
    "collect_paths_",
    "imitate_forward_backward", "imitate_train_", "imitation_loss",
    "fill_targets_", "distill_forward_backward", "distill_train_", "distillation_loss",
    "check_selection", "selecting", "SELECT_RULES",
    "check_truncation", "DEFAULT_TRUNCATION",
]


def _p(a, t):
    return a.ctypes.data_as(t)


def _not_implemented(name):
    raise PPOError(-1, "Function %s needs to be overloaded" % name)       # src/ProximalPolicyOptimization.jl:12-14


def _generic(name):
    @functools.singledispatch
    def f(obj, *a, **k):
        _not_implemented(name)
    f.__name__ = name
    return f


# ---- plugin generic functions (src/ProximalPolicyOptimization.jl:16-30)
state = _generic("state")
reward = _generic("reward")
is_terminal = _generic("is_terminal")
reset_ = _generic("reset!")
step_ = _generic("step!")
action_probabilities = _generic("action_probabilities")
batch_action_probabilities = _generic("batch_action_probabilities")
batch_state = _generic("batch_state")
number_of_actions_per_state = _generic("number_of_actions_per_state")
batch_advantage = _generic("batch_advantage")
save_loss = _generic("save_loss")


def device_count():
    return _lib.device_count()


def set_rollout_persistent(on=None):
    """Rollout execution: True = one launch per rollout (each wavefront walks its envs through all T steps) wherever
    covered, False = three launches per step, None = the value at load (PPO_ROLLOUT_PERSISTENT, else automatic: one launch
    for Q = 8 envs).  Bit-identical results either way."""
    call("ppo_set_rollout_persistent", -1 if on is None else int(bool(on)))


def set_rollout_compact(on=None):
    """State storage of engine-collected rollouts: True = compact env snapshots (64 B per transition for Q = 8; the train
    forward re-derives the observation rows), False = expanded observations (2304 B), None = the value at load
    (PPO_ROLLOUT_COMPACT, else automatic: compact above 32 GiB of expanded states or while streaming to disk).
    Bit-identical results either way."""
    call("ppo_set_rollout_compact", -1 if on is None else int(bool(on)))


def set_bwd_small_max_tiles(tiles=None):
    """Minibatches of up to `tiles` 32-row tiles use the three-product backward (no per-workgroup gradient slabs), larger
    ones the fused kernel.  None = the value at load (PPO_BWD_SMALL_MAX_TILES, else 384), 0 = always the fused kernel."""
    call("ppo_set_bwd_small_max_tiles", -1 if tiles is None else int(tiles))


def set_bwd_split_bf16(mode=None):
    """fp32 policies: True = the fused backward's three big products as split-fp32 ("bf16x6") products on the bf16 matrix
    pipe, False = the pure fp32-MFMA kernel, None = the value at load (PPO_BWD_SPLIT_BF16, else on)."""
    call("ppo_set_bwd_split_bf16", -1 if mode is None else int(bool(mode)))


def set_train_tile_max_tiles(tiles=None):
    """Minibatches of up to `tiles` 32-row tiles run forward + loss + backward-data of each tile in one workgroup
    (k_policy_train_tile) followed by the split-K weight-gradient kernel.  None = the value at load
    (PPO_TRAIN_TILE_MAX_TILES, else 0), 0 = never."""
    call("ppo_set_train_tile_max_tiles", -1 if tiles is None else int(tiles))


def set_fwd_split_max_states(states=None):
    """Minibatches of up to `states` states use the train forward that gives each state to 2 or 4 waves.  None = the value
    at load (PPO_FWD_SPLIT_MAX_STATES, else 512), 0 = always one wave per state."""
    call("ppo_set_fwd_split_max_states", -1 if states is None else int(states))


def set_fwd_split_t2_min_tiles(hid, tiles=None):
    """Split-fp32 train forward at kernel width `hid` (128 or 256): minibatches of at least `tiles` 32-row tiles take its
    two-tiles-per-pass form.  None = the value at load (PPO_FWD_SPLIT_T2_MIN_TILES_128 / PPO_FWD_SPLIT_T2_MIN_TILES, else
    1024 / 1536), 0 = never."""
    call("ppo_set_fwd_split_t2_min_tiles", int(hid), -1 if tiles is None else int(tiles))


def set_rollout_split_max_envs(envs=None):
    """One-launch rollouts of up to `envs` envs give every env to 2 or 4 waves (bit-identical results).  None = the value at
    load (PPO_ROLLOUT_SPLIT_MAX_ENVS, else 512), 0 = always one wave per env."""
    call("ppo_set_rollout_split_max_envs", -1 if envs is None else int(envs))


def synchronize():
    call("ppo_device_synchronize")


def profile_enable(on=True):
    call("ppo_profile_enable", int(bool(on)))


def profile_returns(T, N, discount=1.0, iters=20):
    """Average device time (ms) of the return scan on resident [T,N] columns (K6 roofline measurement)."""
    ms = C.c_double(0)
    call("ppo_profile_returns", int(T), int(N), float(discount), int(iters), C.byref(ms))
    return ms.value


def profile_gae(T, N, gamma=0.99, lam=0.95, iters=20):
    """Average device time (ms) of the GAE scan on resident [T,N] columns (17 B/transition roofline measurement)."""
    ms = C.c_double(0)
    call("ppo_profile_gae", int(T), int(N), float(gamma), float(lam), int(iters), C.byref(ms))
    return ms.value


def profile_get(name):
    ms, n = C.c_double(0), C.c_int64(0)
    call("ppo_profile_get", name.encode(), C.byref(ms), C.byref(n))
    return ms.value, n.value


# ------------------------------------------------------------------ state container (test/quad_game_utilities.jl:17-20)
class StateData:
    """vertex_score: int8 [H,F] (single) or [B,H,F] (batched); action_mask: active-quad bit mask(s).

    The reference stores the [F,H] Int matrix and a Float32 {0,-Inf} mask vector; here the same
    information travels as the row-per-half-edge int8 matrix and the active-quad bits the mask is
    built from (action_mask(), test/quad_game_utilities.jl:39-44)."""

    def __init__(self, vertex_score, action_mask):
        self.vertex_score = vertex_score
        self.action_mask = action_mask

    def mask_vector(self, actions_per_edge=4):
        bits = np.atleast_1d(np.asarray(self.action_mask, np.uint32))
        Hh = self.vertex_score.shape[-2]
        q = np.arange(Hh * actions_per_edge) // (4 * actions_per_edge)
        m = np.where((bits[:, None] >> q[None, :]) & 1, np.float32(0), np.float32(-np.inf))
        return m[0] if np.ndim(self.action_mask) == 0 else m


@batch_state.register(list)
def _(states):
    """PPO.batch_state (test/quad_game_utilities.jl:26-33): cat along the batch dimension."""
    if not states or not all(isinstance(x, StateData) for x in states):
        _not_implemented("batch_state")          # the reference dispatches on the element type: no method, no batch
    vs = np.stack([np.asarray(s.vertex_score, np.int8) for s in states])
    am = np.array([np.uint32(s.action_mask) for s in states], np.uint32)
    return StateData(vs, am)


@number_of_actions_per_state.register(StateData)
def _(s):
    return int(s.vertex_score.shape[-2]) * 4          # default: size(mask, 1)  


@batch_advantage.register(StateData)
def _(s, returns):
    return np.asarray(returns, np.float32)             # reference scripts use raw returns as advantage


def index_to_action(index, actions_per_edge=4):
    """test/quad_game_utilities.jl:95-105 (1-based)."""
    apq = 4 * actions_per_edge
    quad = (index - 1) // apq + 1
    qa = (index - 1) % apq
    return quad, qa // actions_per_edge + 1, qa % actions_per_edge + 1


def action_mask(active_quad, actions_per_edge=4):
    """test/quad_game_utilities.jl:39-44."""
    req = np.repeat(~np.asarray(active_quad, bool), 4 * actions_per_edge)
    return np.where(req, -np.inf, 0.0).astype(np.float32)


# ------------------------------------------------------------------ env
class HipVecEnv:
    """N synthetic rand-poly-shaped envs resident on the GPU (ppo_env_*).  Not QuadMeshGame: the
    mesh dynamics are not in the reference tree ('Synthetic env')."""

    def __init__(self, num_envs=1, Q=8, max_actions=128, no_action_reward=-4.0, seed=1234, global_offset=0,
                 strict_sampling=False):
        h = C.c_void_p()
        call("ppo_env_create", 0, int(num_envs), int(global_offset), int(Q), int(max_actions), float(no_action_reward),
             int(seed), C.byref(h))
        self._h = h
        self.N, self.Q, self.H, self.F, self.A = int(num_envs), Q, 4 * Q, 72, 16 * Q
        self.max_actions = max_actions
        if strict_sampling:      # reference behaviour: a CDF walk that ends on a masked action raises (@assert ap[a] > 0.0)
            call("ppo_env_set_strict_sampling", h, 1)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().ppo_env_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def error_flags(self):
        """OR of the device-side flags since creation: 1 action on an inactive quad, 2 index out of range, 4 step! on a
        terminated env, 8 sampled action with probability 0 (the reference's @assert), 32 informational: a CDF
        rounding residue was handed to the last unmasked action (numerics contract)."""
        f = C.c_int32(0)
        lib().ppo_env_check_errors(self._h, C.byref(f))
        return f.value

    def internal(self):
        V = 4 * self.Q
        sc = np.empty((self.N, V), np.int8)
        dg = np.empty((self.N, V), np.int8)
        st = np.empty(self.N, np.int32)
        ep = np.empty(self.N, np.uint32)
        tk = np.empty(self.N, np.uint32)
        call("ppo_env_get_internal", self._h, _p(sc, _lib.c_i8p), _p(dg, _lib.c_i8p), _p(st, _lib.c_i32p),
             _p(ep, _lib.c_u32p), _p(tk, _lib.c_u32p))
        return dict(score=sc, degree=dg, steps=st, episode=ep, tick=tk)

    def set_internal(self, score, degree, active):
        """Load caller-supplied states (check_internal's conditions; one per env): every env is left as reset! would leave
        it (steps 0, reward 0, not terminal) with these arrays in place of the random draw; the episode and tick counters
        are untouched."""
        sc, dg, act = check_internal(score, degree, active, self.Q)
        if sc.shape[0] != self.N:
            raise PPOError(-1, "AssertionError: set_internal expects one state per env")
        call("ppo_env_set_internal", self._h, _p(sc, _lib.c_i8p), _p(dg, _lib.c_i8p), _p(act, _lib.c_u32p))

    def active_quads(self):
        """The active-quad word of every env (uint32 [N])."""
        act = np.empty(self.N, np.uint32)
        call("ppo_env_get_active", self._h, _p(act, _lib.c_u32p))
        return act


@state.register(HipVecEnv)
def _(env):
    obs = np.empty((env.N, env.H, env.F), np.int8)
    act = np.empty(env.N, np.uint32)
    call("ppo_env_get_state", env._h, _p(obs, _lib.c_i8p), _p(act, _lib.c_u32p))
    return StateData(obs[0], act[0]) if env.N == 1 else StateData(obs, act)


@reward.register(HipVecEnv)
def _(env):
    r = np.empty(env.N, np.float32)
    call("ppo_env_get_reward", env._h, _p(r, _lib.c_f32p))
    return float(r[0]) if env.N == 1 else r


@is_terminal.register(HipVecEnv)
def _(env):
    d = np.empty(env.N, np.uint8)
    call("ppo_env_get_terminal", env._h, _p(d, _lib.c_u8p))
    return bool(d[0]) if env.N == 1 else d.astype(bool)


@reset_.register(HipVecEnv)
def _(env):
    call("ppo_env_reset", env._h)


@step_.register(HipVecEnv)
def _(env, action):
    a = np.atleast_1d(np.asarray(action, np.int64))
    if a.size != env.N:
        raise PPOError(-1, "AssertionError: step! expects one action per env")
    if np.any(a < 1) or np.any(a > env.A):
        raise PPOError(-1, "AssertionError: Expected 0 < action_index <= %d" % env.A)   # quad_game_utilities.jl:178
    a0 = (a - 1).astype(np.int32)
    call("ppo_env_step", env._h, _p(a0, _lib.c_i32p))


# ------------------------------------------------------------------ policy
class HipPolicy:
    """SimplePolicy.Policy(in_channels, hidden_channels, num_hidden_layers, num_output) (test/policy.jl:9-19)
    with parameters resident on the GPU.  `params` is the flat Flux.params vector (W [out,in] column-major)."""

    DTYPES = {"f32": 0, "bf16": 1}

    def __init__(self, in_channels, hidden_channels, num_hidden_layers, num_output, seed=0, dtype="f32"):
        """dtype: arithmetic of the MLP's three Dense products -- "f32" (exact fp32 MFMA, the reference's Float32)
        or "bf16" (bf16 MFMA with fp32 accumulation, BASELINE config 5; ppo_policy_set_dtype)."""
        if dtype not in self.DTYPES:
            raise PPOError(-1, "AssertionError: dtype must be 'f32' or 'bf16'")
        h = C.c_void_p()
        call("ppo_policy_create", int(in_channels), int(hidden_channels), int(num_hidden_layers), int(num_output),
             C.byref(h))
        self._h = h
        self.dtype = dtype
        if dtype != "f32":
            call("ppo_policy_set_dtype", h, self.DTYPES[dtype])
        self.in_channels, self.hidden_channels = in_channels, hidden_channels
        self.num_hidden_layers, self.num_output = num_hidden_layers, num_output
        n = C.c_int64(0)
        call("ppo_policy_num_params", h, C.byref(n))
        self.num_params = n.value
        self.params = glorot_uniform_params(in_channels, hidden_channels, num_hidden_layers, num_output, seed)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().ppo_policy_destroy(self._h)
                self._h = None
        except Exception:
            pass

    @property
    def params(self):
        out = np.empty(self.num_params, np.float32)
        call("ppo_policy_get_params", self._h, _p(out, _lib.c_f32p))
        return out

    @params.setter
    def params(self, flat):
        flat = np.ascontiguousarray(flat, np.float32)
        if flat.size != self.num_params:
            raise PPOError(-1, "AssertionError: expected %d parameters, got %d" % (self.num_params, flat.size))
        call("ppo_policy_set_params", self._h, _p(flat, _lib.c_f32p))

    def grad(self):
        out = np.empty(self.num_params, np.float32)
        call("ppo_policy_get_grad", self._h, _p(out, _lib.c_f32p))
        return out

    @property
    def target_kl(self):
        """None (off, the default), or the approx_kl above which ppo_train_ ends after the epoch that reached it
        (float("inf"): record the statistics, never stop).  The statistics are collected while a target is set only (the
        extra store costs the train forward 0.2 %); with a target set, ppo_iterate_ reports them."""
        t = C.c_double(0)
        call("ppo_policy_get_target_kl", self._h, C.byref(t))
        return None if t.value == 0.0 else t.value

    @target_kl.setter
    def target_kl(self, value):
        call("ppo_policy_set_target_kl", self._h, 0.0 if value is None else float(value))

    def last_train_stats(self):
        """Of the latest ppo_train_ on this policy: {"epochs_run", "stopped_early", "approx_kl", "old_approx_kl",
        "clip_fraction"}, the last three one entry per epoch that ran (kl_stats of that epoch's probability ratios; NaN
        when the call ran with target_kl = None)."""
        n, stopped = C.c_int32(0), C.c_int32(0)
        call("ppo_policy_last_train_stats", self._h, 0, C.byref(n), C.byref(stopped), None, None, None)
        kl, okl, cf = (np.zeros(n.value, np.float64) for _ in range(3))
        call("ppo_policy_last_train_stats", self._h, n.value, C.byref(n), C.byref(stopped), _p(kl, _lib.c_f64p),
             _p(okl, _lib.c_f64p), _p(cf, _lib.c_f64p))
        return {"epochs_run": n.value, "stopped_early": bool(stopped.value), "approx_kl": list(kl),
                "old_approx_kl": list(okl), "clip_fraction": list(cf)}

    @property
    def kl_anchor(self):
        """None (off, the default), or (coef, source, target): while set, ppo_train_, forward_backward and step_batch_ on this
        policy minimise the PPO loss plus coef * the soft-target cross-entropy against the rollouts' target rows -- the gradient
        of coef * KL(q || pi).  source: "column" (fill_targets_ / set_action_targets: a frozen cloned or teacher policy) or
        "recorded" (the behaviour policy's distributions of a collection with record_probs=True: PPO's penalty form).  target:
        0.0 for a fixed coefficient, or d > 0 for PPO's rule: behind every epoch of ppo_train_ whose mean anchor KL exceeds 1.5 d
        coef doubles, below d / 1.5 it halves; the adapted coef is what this property then reads.  Set it from (coef, source)
        or (coef, source, target); coef = 0 records the divergence and leaves the gradient alone.  fp32 policies, in-memory
        rollouts."""
        c, s, t = C.c_double(0), C.c_int32(0), C.c_double(0)
        call("ppo_policy_get_kl_anchor", self._h, C.byref(c), C.byref(s), C.byref(t))
        if s.value == ANCHOR_OFF:
            return None
        return (c.value, ANCHOR_SOURCES[s.value], t.value)

    @kl_anchor.setter
    def kl_anchor(self, value):
        if value is None:
            call("ppo_policy_set_kl_anchor", self._h, 0.0, ANCHOR_OFF, 0.0)
            return
        call("ppo_policy_set_kl_anchor", self._h, *check_kl_anchor(value))

    def last_anchor_stats(self):
        """Of the latest ppo_train_ on this policy that ran with kl_anchor set: {"anchor_kl", "anchor_coef"}, one entry per epoch
        that ran: the mean over the dataset of KL(q' || pi), each state with the parameters its own minibatch saw, and the
        coefficient that epoch ran with.  Empty lists after a ppo_train_ without an anchor.  After ppo_train_(..., parallel=):
        over the states of all ranks, the same on every rank."""
        n = C.c_int32(0)
        call("ppo_policy_last_anchor_stats", self._h, 0, C.byref(n), None, None)
        kl, co = np.zeros(n.value, np.float64), np.zeros(n.value, np.float64)
        call("ppo_policy_last_anchor_stats", self._h, n.value, C.byref(n), _p(kl, _lib.c_f64p), _p(co, _lib.c_f64p))
        return {"anchor_kl": list(kl), "anchor_coef": list(co)}

    @property
    def value_clip(self):
        """For a handle that serves as a critic: None (off, the default: Flux.mse), or the range c of PPO's clipped value loss
        max((V - t)^2, (V_old + clamp(V - V_old, -c, c) - t)^2) that value_forward_backward / value_train_ then minimise,
        V_old being the values compute_values_ / compute_gae_critic_ / compute_gae_ left in the rollout buffer
        (float("inf"): record the statistics, never clip).  With a clip set, ppo_iterate_ reports "value_clip_fraction"."""
        c = C.c_double(0)
        call("ppo_policy_get_value_clip", self._h, C.byref(c))
        return None if c.value == 0.0 else c.value

    @value_clip.setter
    def value_clip(self, value):
        c = 0.0 if value is None else float(value)
        if not c >= 0.0:                                                  # NaN fails it too
            raise PPOError(-1, "AssertionError: value_clip must be None (off), positive or float('inf')")
        call("ppo_policy_set_value_clip", self._h, c)

    def last_value_stats(self):
        """Of the latest value_train_ on this handle: {"epochs_run", "clip_fraction", "mean_sq_change"}, the last two one entry
        per epoch: the share of states whose value left [V_old - c, V_old + c] and the mean of (V - V_old)^2, each state with
        the parameters its own minibatch saw (NaN when the call ran with value_clip = None).  After
        value_train_(..., parallel=): over the states of all ranks, the same on every rank."""
        n = C.c_int32(0)
        call("ppo_policy_last_value_stats", self._h, 0, C.byref(n), None, None)
        cf, ms = np.zeros(n.value, np.float64), np.zeros(n.value, np.float64)
        call("ppo_policy_last_value_stats", self._h, n.value, C.byref(n), _p(cf, _lib.c_f64p), _p(ms, _lib.c_f64p))
        return {"epochs_run": n.value, "clip_fraction": list(cf), "mean_sq_change": list(ms)}

    @property
    def selection(self):
        """(rule, temperature): how the calls that APPLY this policy on a HipVecEnv choose an action -- the evaluators
        (average_returns, average_best_returns, average_normalized_returns, evaluate_trajectories), best_states_ /
        best_state_in_rollout and its siblings, search_best_states_ and search_resample_states_.  rule "sample" draws
        rand(Categorical(p)), "greedy" plays argmax(p) (the lowest index among equal maxima); p = softmax(logits / temperature).
        The default ("sample", 1.0) is the reference's rule.  The setter takes "sample", "greedy", (rule, temperature) or None
        (the default).  The collectors, action_probabilities and every training call never read it: a buffer's p_old must be
        the probability under the distribution the training pass differentiates.  fp32 policies only."""
        r, t = C.c_int32(0), C.c_double(0)
        call("ppo_policy_get_selection", self._h, C.byref(r), C.byref(t))
        return SELECT_RULES[r.value], t.value

    @selection.setter
    def selection(self, value):
        if value is None:
            value = ("sample", 1.0)
        elif isinstance(value, str):
            value = (value, 1.0)
        rule, temperature = check_selection(*value)
        call("ppo_policy_set_selection", self._h, SELECT_RULES.index(rule), temperature)

    @property
    def truncation(self):
        """(top_k, top_p): the truncation of the tempered distribution that rule "sample" of `selection` draws from, read by the
        calls that read the selection and by no other.  top_k keeps the k likeliest actions (0: all), top_p the likeliest set
        whose probability mass in front of an action is below top_p (1.0: all); equal probabilities rank by the lower index;
        the kept probabilities are renormalised and p_sel is the renormalised one.  Both compose (an action is kept when both
        keep it) and compose with the temperature.  "greedy" ignores it: the arg-max is always kept.  The default (0, 1.0) is
        no truncation; the setter takes a pair or None (the default).  fp32 policies only."""
        k, p = C.c_int32(0), C.c_double(0)
        call("ppo_policy_get_truncation", self._h, C.byref(k), C.byref(p))
        return k.value, p.value

    @truncation.setter
    def truncation(self, value):
        top_k, top_p = check_truncation(*(DEFAULT_TRUNCATION if value is None else value))
        call("ppo_policy_set_truncation", self._h, top_k, top_p)

    def grad_buffer_dev(self):
        ptr, n = C.c_void_p(), C.c_int64(0)
        call("ppo_policy_grad_buffer_dev", self._h, C.byref(ptr), C.byref(n))
        return ptr.value, n.value

    def layer_shapes(self):
        d = [(self.hidden_channels, self.in_channels)] + [(self.hidden_channels, self.hidden_channels)] * \
            (self.num_hidden_layers - 1) + [(self.num_output, self.hidden_channels)]
        return d


def glorot_uniform_params(F, HID, n_hidden, out, seed=0):
    """Flux default init: Glorot-uniform weights, zero bias; flat Flux order."""
    rng = np.random.default_rng(seed)
    parts = []
    for (o, i) in [(HID, F)] + [(HID, HID)] * (n_hidden - 1) + [(out, HID)]:
        lim = np.sqrt(6.0 / (o + i))
        W = rng.uniform(-lim, lim, size=(o, i)).astype(np.float32)
        parts += [W.ravel(order="F"), np.zeros(o, np.float32)]
    return np.concatenate(parts).astype(np.float32)


def _forward(policy, vs, bits):
    vs = np.ascontiguousarray(vs, np.int8)
    bits = np.ascontiguousarray(bits, np.uint32)
    B, Hh, F = vs.shape
    probs = np.empty((B, Hh * 4), np.float32)
    call("ppo_policy_forward", policy._h, _p(vs, _lib.c_i8p), _p(bits, _lib.c_u32p), B, Hh, _p(probs, _lib.c_f32p))
    return probs


@action_probabilities.register(HipPolicy)
def _(policy, s):
    """test/quad_game_utilities.jl:65-71 -> vector of length A."""
    return _forward(policy, np.asarray(s.vertex_score)[None], np.atleast_1d(np.uint32(s.action_mask)))[0]


@batch_action_probabilities.register(HipPolicy)
def _(policy, s):
    """test/quad_game_utilities.jl:73-79 -> [A,B] (returned as the transposed view of the C-order [B,A])."""
    return _forward(policy, s.vertex_score, s.action_mask).T


# ------------------------------------------------------------------ critic
class HipCritic(HipPolicy):
    """A state-value network of the policy's own shape, Policy(in_channels, hidden_channels, num_hidden_layers, 4), read as
    V(s) = mean of the 4 outputs of every half-edge row of an ACTIVE quad (0 when no quad is active) and trained with
    Flux.mse.  Being a HipPolicy, `params`, `grad`, save_policy / load_policy and every Optimiser chain work unchanged.
    fp32 only."""

    def __init__(self, in_channels, hidden_channels, num_hidden_layers, seed=0):
        super().__init__(in_channels, hidden_channels, num_hidden_layers, 4, seed=seed)


def _value_forward(critic, vs, bits):
    vs = np.ascontiguousarray(vs, np.int8)
    bits = np.ascontiguousarray(bits, np.uint32)
    B, Hh, F = vs.shape
    out = np.empty(B, np.float32)
    call("ppo_value_forward", critic._h, _p(vs, _lib.c_i8p), _p(bits, _lib.c_u32p), B, Hh, _p(out, _lib.c_f32p))
    return out


def state_values(critic, s):
    """V(s) of one StateData -> float."""
    return float(_value_forward(critic, np.asarray(s.vertex_score)[None], np.atleast_1d(np.uint32(s.action_mask)))[0])


def batch_state_values(critic, s):
    """V of a batched StateData ([B,H,F] rows, [B] active-quad masks) -> float32 [B]."""
    return _value_forward(critic, s.vertex_score, s.action_mask)


def pooled_state_value(logits, active):
    """The critic's pooling on given per-half-edge outputs (plain numpy, for users of the generic path): logits [B,H,4]
    (or [H,4]), active = active-quad bit mask(s) -> float32 [B]: mean over the rows of active quads and their 4 outputs,
    0 where no quad is active."""
    y = np.asarray(logits, np.float32)
    single = y.ndim == 2
    y = y[None] if single else y
    bits = np.atleast_1d(np.asarray(active, np.uint32))
    on = ((bits[:, None] >> (np.arange(y.shape[1]) // 4).astype(np.uint32)[None, :]) & 1).astype(bool)     # [B,H]
    n = 4 * on.sum(axis=1)
    tot = np.where(on[:, :, None], y, np.float32(0)).sum(axis=(1, 2), dtype=np.float32)
    v = np.where(n > 0, tot / np.maximum(n, 1).astype(np.float32), np.float32(0)).astype(np.float32)
    return v[0] if single else v


def value_loss(values, targets):
    """Flux.mse(values, targets) in float32 arithmetic -> float."""
    d = np.asarray(values, np.float32) - np.asarray(targets, np.float32)
    return float(np.mean(d * d, dtype=np.float32))


def value_loss_clipped(values, old_values, targets, clip):
    """PPO's clipped value loss in float32 arithmetic, as the device forms it -> float: the mean of
    max((V - t)^2, (Vclip - t)^2) with Vclip = V_old + clamp(V - V_old, -clip, clip); whether V left the range is decided on
    V - V_old itself, and a tie of the two squares keeps the unclipped one.  clip None: value_loss."""
    if clip is None:
        return value_loss(values, targets)
    v, vo, t = (np.asarray(x, np.float32) for x in (values, old_values, targets))
    c = np.float32(clip)
    delta = v - vo
    with np.errstate(invalid="ignore"):
        vc = vo + np.copysign(c, delta)
        d, dc = v - t, vc - t
        keep = (np.abs(delta) <= c) | (np.abs(d) >= np.abs(dc))
    term = np.where(keep, d, dc).astype(np.float32)
    return float(np.mean(term * term, dtype=np.float32))


def imitation_loss(logits, mask, actions, weights=None):
    """The imitation (behaviour-cloning) loss column 0 on given logits, in float32 arithmetic as the device forms it (plain
    numpy host mirror, for users of the generic path) -> float: -mean_i(w_i log pi(a_i | s_i)), log pi the log-softmax over
    the actions of active quads, (l[a] - max l) - log sum exp(l - max l), finite where exp underflows.  logits [B, A]; mask:
    [B, A] bools (True = allowed), or the [B] active-quad bit masks (action k belongs to quad k // 16); actions [B] 0-based,
    each allowed; weights [B] (None: 1), clamped at 0 like the device's max(adv, 0)."""
    l = np.asarray(logits, np.float32)
    B, A = l.shape
    m = np.asarray(mask)
    if m.ndim == 1:
        bits = m.astype(np.uint32)
        m = ((bits[:, None] >> (np.arange(A) // 16).astype(np.uint32)[None, :]) & 1).astype(bool)
    m = m.astype(bool)
    a = np.asarray(actions, np.int64)
    w = np.ones(B, np.float32) if weights is None else np.maximum(np.asarray(weights, np.float32), np.float32(0))
    lm = np.where(m, l, np.float32(-np.inf))
    mx = lm.max(axis=1)
    S = np.where(m, np.exp(l - mx[:, None], dtype=np.float32), np.float32(0)).sum(axis=1, dtype=np.float32)
    logp = (l[np.arange(B), a] - mx) - np.log(S, dtype=np.float32)
    return float(-np.mean(w * logp, dtype=np.float32))


def _bool_mask(mask, A):
    m = np.asarray(mask)
    if m.ndim == 1:
        bits = m.astype(np.uint32)
        m = ((bits[:, None] >> (np.arange(A) // 16).astype(np.uint32)[None, :]) & 1).astype(bool)
    return m.astype(bool)


def distillation_loss(logits, mask, targets, weights=None, floor=False):
    """The distillation (soft-target cross-entropy) loss column 0 on given logits, in float32 arithmetic as the device forms it
    (plain numpy host mirror) -> float: -mean_i(w_i sum_k q'_ik log pi(k | s_i)), q' the target row on the allowed actions and
    0 elsewhere (mass on a masked action is ignored), log pi the log-softmax over the allowed actions, (l - max l) -
    log sum exp(l - max l); a term with q'_k == 0 is exactly 0, so the loss is finite where exp underflows.  logits, targets
    [B, A] (targets finite and >= 0, not necessarily normalised); mask and weights as in imitation_loss.  floor=True: returns
    (loss, floor) with floor = mean_i(w_i * -sum_k q'_ik log q'_ik), the weighted entropy of the kept targets: the value the
    cross-entropy of normalised rows cannot go below (loss - floor is then the weighted KL(q' || pi)); the device does not
    compute it."""
    l = np.asarray(logits, np.float32)
    B, A = l.shape
    m = _bool_mask(mask, A)
    q = np.asarray(targets, np.float32)
    if q.shape != l.shape:
        raise PPOError(-1, "AssertionError: distillation_loss: targets must have the logits' shape")
    if not np.all(np.isfinite(q)) or (q < 0).any():
        raise PPOError(-1, "AssertionError: distillation_loss: every target entry must be finite and >= 0")
    w = np.ones(B, np.float32) if weights is None else np.maximum(np.asarray(weights, np.float32), np.float32(0))
    q = np.where(m, q, np.float32(0))
    mx = np.where(m, l, np.float32(-np.inf)).max(axis=1)
    S = np.where(m, np.exp(np.where(m, l - mx[:, None], np.float32(0)), dtype=np.float32), np.float32(0)).sum(axis=1, dtype=np.float32)
    logp = (l - mx[:, None]) - np.log(S, dtype=np.float32)[:, None]
    ce = np.where(q == 0, np.float32(0), q * np.where(q == 0, np.float32(0), logp)).sum(axis=1, dtype=np.float32)
    loss = float(-np.mean(w * ce, dtype=np.float32))
    if not floor:
        return loss
    with np.errstate(divide="ignore", invalid="ignore"):
        h = -np.where(q == 0, 0.0, q.astype(np.float64) * np.log(q.astype(np.float64))).sum(axis=1)
    return loss, float(np.mean(w.astype(np.float64) * h))


ANCHOR_OFF = -1              # PPO_ANCHOR_OFF
ANCHOR_SOURCES = ("column", "recorded")        # PPO_TARGETS_COLUMN, PPO_TARGETS_RECORDED


def check_kl_anchor(value):
    """A HipPolicy.kl_anchor value -> (coef, source number, target), refused like the library refuses it (no device call)."""
    if not isinstance(value, (tuple, list)) or len(value) not in (2, 3):
        raise PPOError(-1, "AssertionError: kl_anchor must be None, (coef, source) or (coef, source, target)")
    coef, source = float(value[0]), value[1]
    target = float(value[2]) if len(value) == 3 else 0.0
    if source not in ANCHOR_SOURCES:
        raise PPOError(-4, "kl_anchor source must be one of %s" % sorted(ANCHOR_SOURCES))
    if not (coef >= 0.0 and np.isfinite(coef)):                           # NaN fails it too
        raise PPOError(-1, "AssertionError: kl_anchor: the coefficient must be finite and >= 0")
    if not (target >= 0.0 and np.isfinite(target)):
        raise PPOError(-1, "AssertionError: kl_anchor: the target must be 0 (fixed coefficient) or positive and finite")
    return coef, ANCHOR_SOURCES.index(source), target


def adapt_kl_coef(coef, mean_kl, target):
    """The coefficient rule ppo_train_ applies behind every epoch (PPO's penalty form, Schulman et al. 2017, section 4; plain
    host mirror): target 0 keeps coef; a mean anchor KL above 1.5 target doubles it, one below target / 1.5 halves it.  On a
    data-parallel run mean_kl is the mean over the states of ALL ranks, so every rank makes the same move."""
    if target > 0:
        if mean_kl > 1.5 * target and np.isfinite(coef * 2.0):
            return coef * 2.0
        if mean_kl < target / 1.5:
            return coef / 2.0
    return coef


def anchored_ppo_loss(logits, mask, actions, p_old, adv, eps, targets, coef, kl=False):
    """The KL-anchored PPO loss column 0 on given logits, in float32 arithmetic as the device forms it (plain numpy host mirror)
    -> float: -mean_i(min(pi(a_i | s_i) / p_old_i * adv_i, clip_i) + coef * sum_k q'_ik log pi(k | s_i)), the clipped surrogate
    of ppo_loss_with_entropy (clip = (1 + eps) adv for adv >= 0, (1 - eps) adv below) plus coef times distillation_loss's
    cross-entropy.  logits, targets [B, A]; mask as in imitation_loss; actions [B] 0-based, each allowed; p_old, adv [B].
    kl=True: returns (loss, mean_i KL(q'_i || pi_i)), KL_i = sum over q'_ik > 0 of q'_ik (log q'_ik - log pi(k | s_i)), the
    figure last_anchor_stats reports per epoch."""
    l = np.asarray(logits, np.float32)
    B, A = l.shape
    m = _bool_mask(mask, A)
    q = np.asarray(targets, np.float32)
    if q.shape != l.shape:
        raise PPOError(-1, "AssertionError: anchored_ppo_loss: targets must have the logits' shape")
    if not np.all(np.isfinite(q)) or (q < 0).any():
        raise PPOError(-1, "AssertionError: anchored_ppo_loss: every target entry must be finite and >= 0")
    a = np.asarray(actions, np.int64)
    po, ad = np.asarray(p_old, np.float32), np.asarray(adv, np.float32)
    q = np.where(m, q, np.float32(0))
    mx = np.where(m, l, np.float32(-np.inf)).max(axis=1)
    e = np.where(m, np.exp(np.where(m, l - mx[:, None], np.float32(0)), dtype=np.float32), np.float32(0))
    S = e.sum(axis=1, dtype=np.float32)
    ps = (e / S[:, None])[np.arange(B), a]
    gain = (ps / po * ad).astype(np.float64)
    clip = np.where(ad >= 0, (1.0 + float(eps)) * ad.astype(np.float64), (1.0 - float(eps)) * ad.astype(np.float64))
    minval = np.where(gain < clip, gain, clip)
    logp = (l - mx[:, None]) - np.log(S, dtype=np.float32)[:, None]
    ce = np.where(q == 0, np.float32(0), q * np.where(q == 0, np.float32(0), logp)).sum(axis=1, dtype=np.float32)
    loss = float(np.float32(-np.mean(minval + (np.float32(coef) * ce).astype(np.float64))))
    if not kl:
        return loss
    pos = q > 0
    lq = np.log(np.where(pos, q, np.float32(1)), dtype=np.float32)
    d = np.where(pos, q * (lq - np.where(pos, logp, np.float32(0))), np.float32(0)).sum(axis=1, dtype=np.float32)
    return loss, float(np.mean(d, dtype=np.float64))


# ------------------------------------------------------------------ optimiser
class Adam:
    """Flux legacy Adam(eta, beta, epsilon)."""

    def __init__(self, eta=1e-3, beta=(0.9, 0.999), epsilon=1e-8):
        self.eta, self.beta, self.epsilon = float(eta), (float(beta[0]), float(beta[1])), float(epsilon)
        self._h = None
        self._policy = None

    def _bind(self, policy):
        if self._h is None:
            h = C.c_void_p()
            call("ppo_adam_create", policy._h, self.eta, self.beta[0], self.beta[1], self.epsilon, C.byref(h))
            self._h, self._policy = h, policy
        elif self._policy is not policy:
            raise PPOError(-1, "AssertionError: optimiser state belongs to another policy")
        call("ppo_adam_set_lr", self._h, float(self.eta))
        return self._h

    def __del__(self):
        try:
            if self._h:
                lib().ppo_adam_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def get_state(self):
        n = self._policy.num_params
        m, v, bp = np.empty(n, np.float32), np.empty(n, np.float32), np.empty(2, np.float64)
        call("ppo_adam_get_state", self._h, _p(m, _lib.c_f32p), _p(v, _lib.c_f32p), _p(bp, _lib.c_f64p))
        return m, v, bp


class ExpDecay:
    """Flux legacy ExpDecay(eta, decay, decay_step, clip, start): eta = max(eta * decay, clip) every `decay_step`
    update! calls past `start` (field `step` holds decay_step, as in Flux).  Only as a member of an Optimiser."""

    def __init__(self, eta=1e-3, decay=0.1, decay_step=1000, clip=1e-4, start=0):
        self.eta, self.decay, self.step, self.clip, self.start = float(eta), float(decay), int(decay_step), float(clip), int(start)


class Descent:
    """Flux legacy Descent(eta): plain gradient descent."""

    def __init__(self, eta=0.1):
        self.eta = float(eta)


class Momentum:
    """Flux legacy Momentum(eta, rho)."""

    def __init__(self, eta=0.01, rho=0.9):
        self.eta, self.rho = float(eta), float(rho)


class Nesterov:
    """Flux legacy Nesterov(eta, rho)."""

    def __init__(self, eta=1e-3, rho=0.9):
        self.eta, self.rho = float(eta), float(rho)


class RMSProp:
    """Flux legacy RMSProp(eta, rho, epsilon)."""

    def __init__(self, eta=1e-3, rho=0.9, epsilon=1e-8):
        self.eta, self.rho, self.epsilon = float(eta), float(rho), float(epsilon)


class ClipValue:
    """Flux legacy ClipValue(thresh): D = clamp(D, -thresh, thresh).  No eta: get_optimizer_learning_rate fails on a chain
    that holds it, as in the reference."""

    def __init__(self, thresh):
        self.thresh = float(thresh)


class ClipNorm:
    """Flux legacy ClipNorm(thresh): each parameter array's D scaled by thresh / norm(D) when its 2-norm exceeds thresh
    (the norm: float64 sum of the squares, rounded once; include/ppo_hip.h)."""

    def __init__(self, thresh):
        self.thresh = float(thresh)


class WeightDecay:
    """Flux legacy WeightDecay(wd): D += wd * x."""

    def __init__(self, wd=0.0):
        self.wd = float(wd)


class InvDecay:
    """Flux legacy InvDecay(gamma): D *= 1 / (1 + gamma * n) at its n-th update! call."""

    def __init__(self, gamma=0.001):
        self.gamma = float(gamma)


def AdamW(eta=0.001, beta=(0.9, 0.999), decay=0.0):
    """Flux 0.13 AdamW: Optimiser(Adam(1, beta), WeightDecay(decay), Descent(eta))."""
    return Optimiser(Adam(1.0, beta), WeightDecay(decay), Descent(eta))


# PPO_OPT_* kinds of include/ppo_hip.h and each member's hyper row (eta first; thresh / wd / gamma for the members without)
_CHAIN_KINDS = {
    Adam: (1, lambda o: (o.eta, o.beta[0], o.beta[1], o.epsilon, 0.0)),
    ExpDecay: (2, lambda o: (o.eta, o.decay, float(o.step), o.clip, float(o.start))),
    Descent: (3, lambda o: (o.eta, 0.0, 0.0, 0.0, 0.0)),
    Momentum: (4, lambda o: (o.eta, o.rho, 0.0, 0.0, 0.0)),
    Nesterov: (5, lambda o: (o.eta, o.rho, 0.0, 0.0, 0.0)),
    RMSProp: (6, lambda o: (o.eta, o.rho, o.epsilon, 0.0, 0.0)),
    ClipValue: (7, lambda o: (o.thresh, 0.0, 0.0, 0.0, 0.0)),
    ClipNorm: (8, lambda o: (o.thresh, 0.0, 0.0, 0.0, 0.0)),
    WeightDecay: (9, lambda o: (o.wd, 0.0, 0.0, 0.0, 0.0)),
    InvDecay: (10, lambda o: (o.gamma, 0.0, 0.0, 0.0, 0.0)),
}
_STATE_KINDS = (Adam, Momentum, Nesterov, RMSProp)
_NO_ETA = (ClipValue, ClipNorm, WeightDecay, InvDecay)
_HYPER_FIELD = {ClipValue: "thresh", ClipNorm: "thresh", WeightDecay: "wd", InvDecay: "gamma"}


class Optimiser:
    """Flux.Optimiser(...): iterable composite (get_optimizer_learning_rate iterates it, src/train.jl:155-158).
    On the device: 1 to 4 members of Adam, ExpDecay, Descent, Momentum, Nesterov, RMSProp, ClipValue, ClipNorm,
    WeightDecay, InvDecay, each kind at most once, in any order (include/ppo_hip.h, ppo_optimiser_create); AdamW(...) is
    such a chain.  Optimiser(Adam(...)) keeps its Adam handle (members[0])."""

    def __init__(self, *members):
        self.members = list(members)
        self._h = None
        self._policy = None

    def __iter__(self):
        return iter(self.members)

    def _adam(self):
        adams = [m for m in self.members if isinstance(m, Adam)]
        if len(adams) != 1 or len(self.members) != 1:
            raise PPOError(-4, "only Optimiser(Adam(...)) is implemented on the device")
        return adams[0]

    def _adam_only(self):
        return len(self.members) == 1 and type(self.members[0]) is Adam

    def _check(self):
        """The chain's (kinds, hyper) rows, or PPOError(PPO_ERR_UNSUPPORTED / PPO_ERR_ARG) before any device work."""
        if not 1 <= len(self.members) <= 4:
            raise PPOError(-4, "Optimiser: the device runs chains of 1 to 4 members, got %d" % len(self.members))
        kinds, hyper = [], []
        for m in self.members:
            name = type(m).__name__
            if type(m) in _NO_ETA:
                t = getattr(m, "thresh", 0.0)
                if not t >= 0:
                    raise PPOError(-1, "AssertionError: %s: thresh must be >= 0 (and not NaN), got %r" % (name, t))
            elif not hasattr(m, "eta"):
                raise PPOError(-4, "Optimiser member %s has no eta (get_optimizer_learning_rate cannot run it): "
                                   "not supported on the device" % name)
            if type(m) not in _CHAIN_KINDS:
                raise PPOError(-4, "Optimiser member %s is not supported on the device (Adam, ExpDecay, Descent, Momentum, "
                                   "Nesterov, RMSProp)" % name)
            if type(m) in (type(x) for x in self.members[:len(kinds)]):
                raise PPOError(-4, "Optimiser: member %s appears twice; each kind at most once on the device" % name)
            if isinstance(m, ExpDecay) and m.step < 1:
                raise PPOError(-1, "AssertionError: ExpDecay: decay_step >= 1")
            k, row = _CHAIN_KINDS[type(m)]
            kinds.append(k)
            hyper.append(row(m))
        return np.array(kinds, np.int32), np.ascontiguousarray(hyper, np.float64)

    def _handle(self, policy):
        """The ppo_adam_t of this chain for `policy`, created on first use; pushes every member's current eta."""
        if self._adam_only():
            return self._adam()._bind(policy)
        kinds, hyper = self._check()
        if self._h is None:
            h = C.c_void_p()
            call("ppo_optimiser_create", policy._h, len(kinds), _p(kinds, _lib.c_i32p), _p(hyper, _lib.c_f64p), C.byref(h))
            self._h, self._policy = h, policy
        elif self._policy is not policy:
            raise PPOError(-1, "AssertionError: optimiser state belongs to another policy")
        for j, m in enumerate(self.members):
            if type(m) in _NO_ETA:                          # thresh / wd / gamma may change between calls, as in Flux
                call("ppo_optimiser_set_hyper", self._h, j, _p(np.ascontiguousarray(hyper[j]), _lib.c_f64p))
            else:
                call("ppo_optimiser_set_eta", self._h, j, float(m.eta))
        return self._h

    def _pull(self):
        """After training: the etas ExpDecay decayed on the device back into the members."""
        if self._h is None:
            return
        e = C.c_double(0)
        for j, m in enumerate(self.members):
            if isinstance(m, ExpDecay):
                call("ppo_optimiser_get_eta", self._h, j, C.byref(e))
                m.eta = e.value

    def __del__(self):
        try:
            if self._h:
                lib().ppo_adam_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def get_state(self):
        """Checkpoint of a bound chain: {"epochs": epochs trained (keys the device permutation), "members": one dict per
        member in chain order with its eta (or thresh / wd / gamma) and state (Adam m, v, beta_pow; Momentum / Nesterov
        velocity; RMSProp acc; ExpDecay / InvDecay its update count)}."""
        h = self._adam()._h if self._adam_only() else self._h
        if h is None:
            raise PPOError(-1, "AssertionError: get_state: the optimiser has not been bound to a policy yet")
        pol = self._adam()._policy if self._adam_only() else self._policy
        n = pol.num_params
        ep = C.c_int64(0)
        call("ppo_adam_get_epoch_count", h, C.byref(ep))
        out = []
        for j, m in enumerate(self.members):
            eta, cnt = C.c_double(0), C.c_int64(0)
            s0, s1, sc = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(2, np.float64)
            call("ppo_optimiser_get_state", h, j, _p(s0, _lib.c_f32p), _p(s1, _lib.c_f32p), _p(sc, _lib.c_f64p), C.byref(cnt))
            if type(m) in _NO_ETA:
                hy = np.zeros(5, np.float64)
                call("ppo_optimiser_get_hyper", h, j, _p(hy, _lib.c_f64p))
                d = {"kind": type(m).__name__, _HYPER_FIELD[type(m)]: float(hy[0])}
                if isinstance(m, InvDecay):
                    d["count"] = int(cnt.value)
                out.append(d)
                continue
            call("ppo_optimiser_get_eta", h, j, C.byref(eta))
            d = {"kind": type(m).__name__, "eta": eta.value}
            if isinstance(m, Adam):
                d.update(m=s0, v=s1, beta_pow=sc)
            elif isinstance(m, (Momentum, Nesterov)):
                d["velocity"] = s0
            elif isinstance(m, RMSProp):
                d["acc"] = s0
            elif isinstance(m, ExpDecay):
                d["count"] = int(cnt.value)
            out.append(d)
        return {"epochs": int(ep.value), "members": out}

    def set_state(self, policy, state):
        """Resume from get_state(): binds this chain (same member kinds, same order) to `policy` and restores it."""
        ms = state["members"]
        if [d["kind"] for d in ms] != [type(m).__name__ for m in self.members]:
            raise PPOError(-1, "AssertionError: set_state: the checkpoint holds a chain of other members")
        for m, d in zip(self.members, ms):
            if type(m) in _NO_ETA:
                setattr(m, _HYPER_FIELD[type(m)], float(d[_HYPER_FIELD[type(m)]]))
            else:
                m.eta = float(d["eta"])
        h = self._handle(policy)
        keep = []                                          # the arrays handed over live until their call returns
        for j, (m, d) in enumerate(zip(self.members, ms)):
            s0 = s1 = sc = cnt = None
            if isinstance(m, Adam):
                keep += [np.ascontiguousarray(d["m"], np.float32), np.ascontiguousarray(d["v"], np.float32),
                         np.ascontiguousarray(d["beta_pow"], np.float64)]
                s0, s1, sc = _p(keep[-3], _lib.c_f32p), _p(keep[-2], _lib.c_f32p), _p(keep[-1], _lib.c_f64p)
            elif isinstance(m, (Momentum, Nesterov, RMSProp)):
                keep.append(np.ascontiguousarray(d["acc" if isinstance(m, RMSProp) else "velocity"], np.float32))
                s0 = _p(keep[-1], _lib.c_f32p)
            elif isinstance(m, (ExpDecay, InvDecay)):
                cnt = C.byref(C.c_int64(int(d["count"])))
            call("ppo_optimiser_set_state", h, j, s0, s1, sc, cnt)
        call("ppo_adam_set_epoch_count", h, int(state["epochs"]))


def get_optimizer_learning_rate(optimizer):
    lr = 1.0
    for opt in optimizer:          # a bare Adam is not iterable, like the reference
        lr *= opt.eta
    return lr


# ------------------------------------------------------------------ standalone ops
def compute_returns(rewards, terminal, discount):
    """src/collect_rollouts.jl:26-42.  A Python float discount is a Float64 (running value in fp64);
    pass np.float32(discount) for the all-Float32 variant."""
    r = np.ascontiguousarray(rewards, np.float32)
    t = np.ascontiguousarray(terminal, np.uint8)
    if r.shape != t.shape:
        raise PPOError(-1, "AssertionError: rewards and terminal differ in length")
    out = np.empty_like(r)
    call("ppo_compute_returns", _p(r, _lib.c_f32p), _p(t, _lib.c_u8p), r.size, float(discount),
         int(isinstance(discount, np.float32)), _p(out, _lib.c_f32p))
    return out


def compute_returns_tn(rewards, done, discount):
    r = np.ascontiguousarray(rewards, np.float32)
    d = np.ascontiguousarray(done, np.uint8)
    T, N = r.shape
    out = np.empty_like(r)
    call("ppo_compute_returns_tn", _p(r, _lib.c_f32p), _p(d, _lib.c_u8p), T, N, float(discount),
         int(isinstance(discount, np.float32)), _p(out, _lib.c_f32p))
    return out


def gae_tn(rewards, done, values, gamma, lam):
    r = np.ascontiguousarray(rewards, np.float32)
    d = np.ascontiguousarray(done, np.uint8)
    v = np.ascontiguousarray(values, np.float32)
    T, N = r.shape
    adv, ret = np.empty_like(r), np.empty_like(r)
    call("ppo_gae_tn", _p(r, _lib.c_f32p), _p(d, _lib.c_u8p), _p(v, _lib.c_f32p), T, N, float(gamma), float(lam),
         _p(adv, _lib.c_f32p), _p(ret, _lib.c_f32p))
    return adv, ret


def gae_boot_tn(rewards, done, values, boot, gamma, lam):
    """gae_tn with a bootstrap column boot [T,N]: a done row takes V[t+1] := boot[t] instead of 0 (the trace is still cut
    there).  boot = the value of the state a time-limit truncation cut the episode in, 0 at real terminals and elsewhere."""
    r = np.ascontiguousarray(rewards, np.float32)
    d = np.ascontiguousarray(done, np.uint8)
    v = np.ascontiguousarray(values, np.float32)
    b = np.ascontiguousarray(boot, np.float32)
    T, N = r.shape
    if d.shape != (T, N) or b.shape != (T, N) or v.shape != (T + 1, N):
        raise PPOError(-1, "AssertionError: done and boot must be [T, N], values [T+1, N] = [%d, %d]" % (T + 1, N))
    adv, ret = np.empty_like(r), np.empty_like(r)
    call("ppo_gae_boot_tn", _p(r, _lib.c_f32p), _p(d, _lib.c_u8p), _p(v, _lib.c_f32p), _p(b, _lib.c_f32p), T, N, float(gamma),
         float(lam), _p(adv, _lib.c_f32p), _p(ret, _lib.c_f32p))
    return adv, ret


def categorical_sample(probs, u):
    """rand(Categorical(p)) for rows of probs [B,A] with uniforms u[B]; returns 1-based actions,
    selected probabilities and the ap[a] > 0 assertion flags (src/collect_rollouts.jl:6-7)."""
    p = np.ascontiguousarray(probs, np.float32)
    uu = np.ascontiguousarray(u, np.float32)
    B, A = p.shape
    a, ps, err = np.empty(B, np.int32), np.empty(B, np.float32), np.empty(B, np.int32)
    call("ppo_categorical_sample", _p(p, _lib.c_f32p), _p(uu, _lib.c_f32p), B, A, _p(a, _lib.c_i32p),
         _p(ps, _lib.c_f32p), _p(err, _lib.c_i32p))
    return a.astype(np.int64) + 1, ps, err


def simplified_ppo_clip(advantage, epsilon):
    """src/train.jl:1-7 (scalar helper; the device path fuses it into the loss kernel)."""
    return (1.0 + epsilon) * advantage if advantage >= 0 else (1.0 - epsilon) * advantage


def get_linear_action_index(selected_actions, num_actions_per_state):
    """src/train.jl:48-52 (1-based in, 1-based out)."""
    a = np.ascontiguousarray(selected_actions, np.int64)
    out = np.empty_like(a)
    call("ppo_linear_action_index", _p(a, _lib.c_i64p), a.size, int(num_actions_per_state), _p(out, _lib.c_i64p))
    return out


def ppo_loss_with_entropy(probs_AB, linear_action_index, old_action_probabilities, advantage, epsilon):
    """Forward-only loss on given probabilities [A,B] (src/train.jl:35-46) -> (ppoloss, entropyloss)."""
    pr = np.ascontiguousarray(np.asarray(probs_AB, np.float32).T)          # [B,A] C-order == [A,B] column-major
    B, A = pr.shape
    li = np.ascontiguousarray(linear_action_index, np.int64)
    po = np.ascontiguousarray(old_action_probabilities, np.float32)
    ad = np.ascontiguousarray(advantage, np.float32)
    a, b = C.c_double(0), C.c_double(0)
    call("ppo_loss_with_entropy", _p(pr, _lib.c_f32p), _p(li, _lib.c_i64p), _p(po, _lib.c_f32p), _p(ad, _lib.c_f32p),
         B, A, float(epsilon), C.byref(a), C.byref(b))
    return a.value, b.value


def philox4x32_10(ctr, key):
    c = np.ascontiguousarray(ctr, np.uint32).reshape(-1, 4)
    k = np.ascontiguousarray(key, np.uint32)
    out = np.empty_like(c)
    call("ppo_philox4x32_10", _p(c, _lib.c_u32p), _p(k, _lib.c_u32p), c.shape[0], _p(out, _lib.c_u32p))
    return out


# ------------------------------------------------------------------ rollouts / dataset
class _Shape:
    """Stand-in for the env of a rollout buffer created by shape (N columns of [H][F] int8 state rows)."""

    def __init__(self, N, H, F):
        self.N, self.H, self.F, self.A = int(N), int(H), int(F), 4 * int(H)


class BufferRollouts:
    """PPO.BufferRollouts() (src/rollout_buffer.jl:1-22): device-resident SoA columns [T,N]."""

    def __init__(self):
        self._h = None
        self._env = None
        self.n_truncated = None  # time-limit truncations the latest compute_gae_critic_(..., bootstrap_truncated=True) found
        self._host = None        # generic (user-defined env) mode: the reference's own AoS columns (generic.HostRollouts)

    def _ensure(self, env, T):
        if self._h is None:
            h = C.c_void_p()
            if isinstance(env, _Shape):      # states of a user env (any F the policy kernels take): ppo_rollouts_create_shape
                call("ppo_rollouts_create_shape", env.N, env.H, env.F, int(T), C.byref(h))
            else:
                call("ppo_rollouts_create", env._h, int(T), C.byref(h))
            self._h, self._env = h, env
        return self._h

    def __del__(self):
        try:
            if self._h:
                lib().ppo_rollouts_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def __len__(self):                                     # Base.length (src/rollout_buffer.jl:40-48)
        if self._h is None and self._host is not None:
            return len(self._host)
        if self._h is None:
            return 0
        n = C.c_int64(0)
        call("ppo_rollouts_len", self._h, C.byref(n))
        return n.value

    def dims(self):
        T, N = C.c_int64(0), C.c_int64(0)
        call("ppo_rollouts_dims", self._h, C.byref(T), C.byref(N))
        return T.value, N.value

    def _get(self, fn, dtype, ctype, extra=()):
        T, N = self.dims()
        out = np.empty((T, N) + tuple(extra), dtype)
        call(fn, self._h, _p(out, ctype))
        return out

    # columns (time-major [T,N]); names follow the reference struct fields
    @property
    def selected_actions(self):
        return self._get("ppo_rollouts_get_actions", np.int32, _lib.c_i32p).astype(np.int64) + 1

    @property
    def selected_action_probabilities(self):
        return self._get("ppo_rollouts_get_probs", np.float32, _lib.c_f32p)

    @property
    def rewards(self):
        """After collect_rollouts! this column holds the RETURNS (compute_state_value! overwrites it,
        src/rollout_buffer.jl:55-64)."""
        return self._get("ppo_rollouts_get_returns", np.float32, _lib.c_f32p)

    @property
    def raw_rewards(self):
        return self._get("ppo_rollouts_get_raw_rewards", np.float32, _lib.c_f32p)

    @property
    def terminal(self):
        return self._get("ppo_rollouts_get_terminal", np.uint8, _lib.c_u8p).astype(bool)

    @property
    def valid(self):
        return self._get("ppo_rollouts_get_valid", np.uint8, _lib.c_u8p).astype(bool)

    @property
    def boot_values(self):
        """The bootstrap column [T,N] the latest compute_gae_(..., final_values=) / compute_gae_critic_(...,
        bootstrap_truncated=True) on these rollouts left on the device."""
        return self._get("ppo_rollouts_get_boot", np.float32, _lib.c_f32p)

    @property
    def state_data(self):
        T, N = self.dims()
        env = self._env
        st = np.empty((T, N, env.H, env.F), np.int8)
        act = np.empty((T, N), np.uint32)
        call("ppo_rollouts_get_states", self._h, _p(st, _lib.c_i8p), _p(act, _lib.c_u32p))
        return st, act

    def full_probs(self):
        T, N = self.dims()
        out = np.empty((T, N, self._env.A), np.float32)
        call("ppo_rollouts_get_full_probs", self._h, _p(out, _lib.c_f32p))
        return out

    @property
    def action_targets(self):
        """The distillation target column [T,N,A] (fill_targets_ / set_action_targets), in full_probs' layout."""
        T, N = self.dims()
        out = np.empty((T, N, self._env.A), np.float32)
        call("ppo_rollouts_get_targets", self._h, _p(out, _lib.c_f32p))
        return out

    def set_action_targets(self, q):
        """Upload distillation targets q [T,N,A]: one row per stored transition (valid or not), every entry finite and >= 0.
        Rows need not be normalised; mass on the actions of inactive quads is ignored by the loss."""
        if self._h is None:
            raise PPOError(-1, "AssertionError: set_action_targets: empty rollout buffer")
        T, N = self.dims()
        q = np.asarray(q)
        if q.shape != (T, N, self._env.A):
            raise PPOError(-1, "AssertionError: set_action_targets: targets must have shape [T,N,A] = %r, got %r" % ((T, N, self._env.A), q.shape))
        q = np.ascontiguousarray(q, np.float32)
        if not np.all(np.isfinite(q)):
            raise PPOError(-1, "AssertionError: set_action_targets: every target entry must be finite")
        if (q < 0).any():
            raise PPOError(-1, "AssertionError: set_action_targets: every target entry must be >= 0")
        call("ppo_rollouts_set_targets", self._h, _p(q, _lib.c_f32p))

    def index(self):
        """Dataset order: flat transition ids t*N+n of the valid transitions."""
        idx = np.empty(len(self), np.int64)
        call("ppo_rollouts_get_index", self._h, _p(idx, _lib.c_i64p))
        return idx

    def set_columns(self, env, states, active, actions1, p_sel, returns, terminal=None):
        """Load columns from the host (generic host-side envs, tests).  env = None: the buffer takes its shape from
        `states` [T,N,H,F] (a user env whose state rows are not the built-in env's 72 features)."""
        st = np.ascontiguousarray(states, np.int8)
        T = st.shape[0]
        if env is None:
            env = _Shape(st.shape[1], st.shape[2], st.shape[3])
        self._ensure(env, T)
        ac = np.ascontiguousarray(active, np.uint32)
        a0 = np.ascontiguousarray(np.asarray(actions1, np.int64) - 1, np.int32)
        ps = np.ascontiguousarray(p_sel, np.float32)
        rt = np.ascontiguousarray(returns, np.float32)
        tm = None if terminal is None else np.ascontiguousarray(terminal, np.uint8)
        call("ppo_rollouts_set", self._h, T, _p(st, _lib.c_i8p), _p(ac, _lib.c_u32p), _p(a0, _lib.c_i32p),
             _p(ps, _lib.c_f32p), _p(rt, _lib.c_f32p), _p(tm, _lib.c_u8p) if tm is not None else None)


def _discount_args(discount):
    return float(discount), int(isinstance(discount, np.float32))


def collect_rollouts_(rollouts, env, policy, num_episodes, discount):
    """PPO.collect_rollouts!(rollouts, env, policy, num_episodes, discount) (src/rollout_buffer.jl:66-79,
    src/rollouts_to_disk.jl:134-147).  Exactly num_episodes whole episodes enter the buffer: the N resident envs play
    them in parallel, episode e on env e mod N (reset! before each).  A DiskRollouts target additionally gets the
    reference's CSV + BSON layout."""
    if not isinstance(env, HipVecEnv):
        # generic method: the reference's own per-step control flow over the user's plugin methods (an env without a
        # `state` method raises "Function state needs to be overloaded" from inside it, like the reference)
        if isinstance(rollouts, DiskRollouts):
            raise PPOError(-4, "DiskRollouts with a user-defined env: use update_ / write_returns_to_disk (disk.py)")
        if rollouts._host is None:
            rollouts._host = HostRollouts()
        generic.collect_rollouts_host_(_this_module(), rollouts._host, env, policy, num_episodes, discount)
        return
    if not isinstance(policy, HipPolicy):
        _not_implemented("action_probabilities")
    if isinstance(rollouts, DiskRollouts):
        print("\n\nCOLLECTING ROLLOUTS :")                              # src/rollouts_to_disk.jl:141
        dev = BufferRollouts()
        collect_rollouts_(dev, env, policy, num_episodes, discount)
        rollouts._device = dev
        export_reference_layout(rollouts, dev)
        return
    if num_episodes < 1:
        raise PPOError(-1, "AssertionError: num_episodes must be >= 1")
    per_env = -(-int(num_episodes) // env.N)
    h = rollouts._ensure(env, per_env * env.max_actions)
    g, f32 = _discount_args(discount)
    call("ppo_collect_rollouts_episodes", h, env._h, policy._h, int(num_episodes), g, f32)


def collect_rollouts_steps_(rollouts, env, policy, num_steps, discount, record_probs=False, pinned_slots=16):
    """Vectorised fixed-T form: num_steps steps of all N envs with auto-reset (the throughput path).
    With a DiskRollouts target every finished step is streamed device -> pinned host -> <dir>/rollout.bin
    while the next step runs (ppo_rollouts_attach_disk)."""
    if isinstance(rollouts, DiskRollouts):
        dev = BufferRollouts()
        h = dev._ensure(env, 0)          # capacity comes with the collection (its storage form depends on the sink)
        # the constructor already wiped the directory; attach recreates it (same semantics) for the shard
        call("ppo_rollouts_attach_disk", h, rollouts.state_data_directory.encode(), int(pinned_slots))
        g, f32 = _discount_args(discount)
        call("ppo_collect_rollouts", h, env._h, policy._h, int(num_steps), g, f32, 0)
        rollouts._device = dev                       # before detach: a failed detach leaves the columns reachable
        if not _disk_async():
            call("ppo_rollouts_detach_disk", h)      # (deferred finish: disk_sync detaches once the file is complete)
        rollouts.num_samples = len(dev)
        with open(rollouts.trajectory_filename, "w", newline="") as f:          # attach wiped it: keep the header
            f.write(",".join(DiskRollouts.FINAL) + "\n")
        return
    h = rollouts._ensure(env, int(num_steps))
    g, f32 = _discount_args(discount)
    call("ppo_collect_rollouts", h, env._h, policy._h, int(num_steps), g, f32, int(bool(record_probs)))


def collect_paths_(rollouts, env, policy, score, degree, active, paths, discount, record_probs=False):
    """Teacher-forced collection: resident env m < M is loaded with start m (score, degree [M, 4Q], active [M]; M <= N) as
    reset! leaves an env and plays path m (paths [M, stride], 1-based action indices as the searches' path output and
    apply_paths_ speak them, anything <= 0 ends a path) instead of sampled actions.  `rollouts` becomes an ordinary buffer
    of T = max(1, longest path) steps: the state in front of every step (compact or expanded storage, as the collectors
    choose), the path's action, the probability the CURRENT policy gives it, reward, terminal, valid, returns and the
    env-major dataset index -- what construct_dataset, ppo_train_, forward_backward, value_train_, compute_values_ and
    compute_gae_critic_ take unchanged.  An env idles (valid False, action 0) behind its path's end, once it is terminal,
    and from M on.  terminal = is_terminal or "the path's last entry": a path is a whole episode for the returns and GAE, and
    a path cut short of the optimum is a truncation, so compute_gae_critic_(..., bootstrap_truncated=True) bootstraps from the
    critic's value of the state it was cut in.  The data is off-policy: selected_action_probabilities is this policy's
    probability of another sampler's action.  The envs that played keep their final states, ticks advanced by the steps
    played, episode counters unchanged; the others are untouched.  An action on an inactive quad is played and penalised
    as step! does, recorded with valid False and probability 0 (in no dataset), and the call raises
    PPOError(PPO_ERR_DEVICE_FLAG) with the buffer filled.  HipVecEnv and a fp32 HipPolicy only.  Returns nothing."""
    if not isinstance(env, HipVecEnv):
        raise PPOError(-4, "collect_paths_ needs a HipVecEnv")
    if not isinstance(policy, HipPolicy):
        _not_implemented("action_probabilities")
    if isinstance(rollouts, DiskRollouts):
        raise PPOError(-4, "collect_paths_: DiskRollouts are not supported")
    sc, dg, act = check_internal(score, degree, active, env.Q)
    M = sc.shape[0]
    if not 1 <= M <= env.N:
        raise PPOError(-1, "AssertionError: collect_paths!: need 1 <= M <= N paths (one resident env plays one path)")
    pa = check_paths(paths, M, env.Q)
    h = rollouts._ensure(env, pa.shape[1])
    g, f32 = _discount_args(discount)
    call("ppo_collect_paths", h, env._h, policy._h, M, _p(sc, _lib.c_i8p), _p(dg, _lib.c_i8p), _p(act, _lib.c_u32p),
         _p(pa, _lib.c_i16p), pa.shape[1], g, f32, int(bool(record_probs)))


def compute_gae_(rollouts, values, gamma, lam, final_values=None):
    """batch_advantage as GAE(gamma, lambda): `values` [T+1, N] are the caller's state values (row T = bootstrap).  The
    advantage column stays on the device for ppo_train_(..., advantage="gae"); returns (advantages, lambda_returns).
    final_values [T, N] (None: today's call): the caller's value of the state an episode was cut in at every time-limit
    truncation (truncated_transitions_ lists them and their final states), 0 at real terminals and everywhere else; a done
    row then bootstraps from it instead of from 0.  The buffer's returns column is not bootstrapped."""
    T, N = rollouts.dims()
    v = np.ascontiguousarray(values, np.float32)
    if v.shape != (T + 1, N):
        raise PPOError(-1, "AssertionError: values must be [T+1, N] = [%d, %d]" % (T + 1, N))
    adv, ret = np.empty((T, N), np.float32), np.empty((T, N), np.float32)
    if final_values is None:
        call("ppo_rollouts_compute_gae", rollouts._h, _p(v, _lib.c_f32p), float(gamma), float(lam), _p(adv, _lib.c_f32p),
             _p(ret, _lib.c_f32p))
        return adv, ret
    b = np.ascontiguousarray(final_values, np.float32)
    if b.shape != (T, N):
        raise PPOError(-1, "AssertionError: final_values must be [T, N] = [%d, %d]" % (T, N))
    call("ppo_rollouts_compute_gae_boot", rollouts._h, _p(v, _lib.c_f32p), _p(b, _lib.c_f32p), float(gamma), float(lam),
         _p(adv, _lib.c_f32p), _p(ret, _lib.c_f32p))
    return adv, ret


def truncated_transitions_(rollouts, fetch_states=True):
    """Which `done` transitions of a buffer collected from the built-in env were time limits (max_actions) and not the
    optimum, found on the device by replaying the stored action on the stored state.  Returns (flags [T,N] bool, final
    states [K,H,F] int8, final active [K] uint32): the state each of the K truncated episodes was cut in, in ascending
    transition id t*N + n -- what a host critic needs for compute_gae_(..., final_values=).  fetch_states=False: (flags,
    None, None).  A buffer of a user-defined env (no env template) is refused."""
    T, N = rollouts.dims()
    flags = np.empty((T, N), np.uint8)
    k = C.c_int64(0)
    call("ppo_rollouts_truncated", rollouts._h, _p(flags, _lib.c_u8p), None, None, 0, C.byref(k))
    if not fetch_states:
        return flags.astype(bool), None, None
    env = rollouts._env
    st, act = np.empty((k.value, env.H, env.F), np.int8), np.empty(k.value, np.uint32)
    call("ppo_rollouts_truncated", rollouts._h, None, _p(st, _lib.c_i8p), _p(act, _lib.c_u32p), k.value, C.byref(k))
    return flags.astype(bool), st, act


def compute_values_(rollouts, env, critic):
    """State values of the buffer from a device critic -> float32 [T+1, N]: rows 0..T-1 are the stored states, row T the
    state every env is in now (zeros when env is None).  They stay on the device for compute_gae_critic_."""
    T, N = rollouts.dims()
    v = np.empty((T + 1, N), np.float32)
    call("ppo_rollouts_compute_values", rollouts._h, env._h if env is not None else None, critic._h, _p(v, _lib.c_f32p))
    return v


def compute_gae_critic_(rollouts, env, critic, gamma, lam, fetch=True, bootstrap_truncated=False):
    """compute_values_ + the GAE(gamma, lambda) scan without a host trip; the advantage column stays on the device for
    ppo_train_(..., advantage="gae"), the lambda-returns for value_train_(..., target="lambda_returns").
    fetch=True returns (advantages, lambda_returns) [T,N]; fetch=False copies nothing back and returns None.
    bootstrap_truncated=True: an episode the env's time limit cut bootstraps from the critic's value of the state it was cut
    in (replayed on the device, truncated_transitions_) instead of from 0; rollouts.boot_values is that column and
    rollouts.n_truncated the number of truncations.  The returns column (target="returns") is not bootstrapped."""
    T, N = rollouts.dims()
    adv = ret = None
    if fetch:
        adv, ret = np.empty((T, N), np.float32), np.empty((T, N), np.float32)
    if not bootstrap_truncated:
        call("ppo_rollouts_compute_gae_critic", rollouts._h, env._h if env is not None else None, critic._h, float(gamma),
             float(lam), _p(adv, _lib.c_f32p) if fetch else None, _p(ret, _lib.c_f32p) if fetch else None)
        return (adv, ret) if fetch else None
    k = C.c_int64(0)
    call("ppo_rollouts_compute_gae_critic_boot", rollouts._h, env._h if env is not None else None, critic._h, float(gamma),
         float(lam), _p(adv, _lib.c_f32p) if fetch else None, _p(ret, _lib.c_f32p) if fetch else None, C.byref(k))
    rollouts.n_truncated = k.value
    return (adv, ret) if fetch else None


def kl_stats(ratio, epsilon):
    """What ppo_train_ keeps per epoch, from probability ratios r = p_new(a|s) / p_old(a|s) in plain numpy float64:
    {"approx_kl": mean((r - 1) - log r), "old_approx_kl": mean(-log r), "clip_fraction": mean(|r - 1| > epsilon)}.
    For users of the generic path, and the statement the device reduction is tested against."""
    r = np.asarray(ratio).astype(np.float64).reshape(-1)
    lg = np.log(r)
    return {"approx_kl": float(np.sum((r - 1.0) - lg) / r.size), "old_approx_kl": float(np.sum(-lg) / r.size),
            "clip_fraction": float(np.count_nonzero(np.abs(r - 1.0) > float(epsilon)) / r.size)}


def explained_variance_from_sums(sums5):
    """1 - Var(t - V) / Var(t) from (n, sum x, sum x^2, sum y, sum y^2), x and y being t and t - V up to a constant shift
    each (ppo_rollouts_value_moments).  NaN when Var(t) == 0."""
    n, sx, sxx, sy, syy = (float(s) for s in sums5)
    var_t = sxx / n - (sx / n) ** 2
    var_d = syy / n - (sy / n) ** 2
    return float("nan") if var_t == 0.0 else 1.0 - var_d / var_t


def value_moments_row(sums5, shifts2):
    """One shard's (n, mean t, M2 t, mean d, M2 d), d = t - V and M2 = the sum of squared deviations from the mean, in float64
    from its shifted sums and its two shifts (ppo_rollouts_value_moments_shifts).  n == 0 gives a row of zeros."""
    n, sx, sxx, sy, syy = (float(s) for s in sums5)
    if n == 0.0:
        return (0.0, 0.0, 0.0, 0.0, 0.0)
    st, sd = (float(s) for s in shifts2)
    return (n, st + sx / n, sxx - sx * sx / n, sd + sy / n, syy - sy * sy / n)


def explained_variance_from_shards(rows):
    """1 - Var(t - V) / Var(t) over the union of shards, from one value_moments_row per shard: merged in the order given with
    the pairwise formula (Chan et al.), so every caller holding the same rows gets the same float.  A shard with n == 0 is
    skipped; NaN when Var(t) == 0 or every shard is empty."""
    n = mt = m2t = md = m2d = 0.0
    for nb, mtb, m2tb, mdb, m2db in ((float(x) for x in r) for r in rows):
        if nb == 0.0:
            continue
        tot = n + nb
        dt, dd = mtb - mt, mdb - md
        mt, md = mt + dt * (nb / tot), md + dd * (nb / tot)
        m2t, m2d = m2t + m2tb + dt * dt * (n * nb / tot), m2d + m2db + dd * dd * (n * nb / tot)
        n = tot
    return float("nan") if n == 0.0 or m2t == 0.0 else 1.0 - m2d / m2t


def explained_variance_(rollouts, target="lambda_returns", parallel=None):
    """The critic's explained variance over the valid transitions of the buffer, reduced on the device: V = the state
    values compute_values_ / compute_gae_critic_ / compute_gae_ left there, target as in value_train_.
    parallel (a DataParallel with world > 1): over the union of every rank's buffer, collectively -- each rank's
    value_moments_row is gathered exactly (a one-hot [world, 5] float64 tensor through DataParallel.allreduce_) and the rows
    are merged in rank order, so every rank returns the same float."""
    t = _value_target(target)
    s = np.zeros(5, np.float64)
    if parallel is None or parallel.world == 1:
        call("ppo_rollouts_value_moments", rollouts._h, t, _p(s, _lib.c_f64p))
        return explained_variance_from_sums(s)
    import torch
    import torch.distributed as dist
    rows = np.zeros((parallel.world, 5), np.float64)
    if len(rollouts):                                       # an empty shard joins the collective with a row of zeros
        sh = np.zeros(2, np.float64)
        call("ppo_rollouts_value_moments_shifts", rollouts._h, t, _p(s, _lib.c_f64p), _p(sh, _lib.c_f64p))
        rows[parallel.rank] = value_moments_row(s, sh)
    x = torch.from_numpy(rows)
    host = dist.get_backend() == "gloo"                     # "nccl" (= RCCL) reduces device tensors only
    x = parallel.allreduce_(x if host else x.cuda())
    return explained_variance_from_shards(x.cpu().numpy())


class BufferDataset:
    """src/rollout_buffer.jl:95-147.  Non-owning view; indices are 1-based like the reference."""

    def __init__(self, rollouts):
        self.rollouts = rollouts
        self._cache = None

    def __len__(self):
        return len(self.rollouts)

    def _columns(self):
        if self._cache is None:
            r = self.rollouts
            st, act = r.state_data
            idx = r.index()
            self._cache = dict(idx=idx, st=st.reshape(-1, st.shape[2], st.shape[3]), act=act.reshape(-1),
                               a=r.selected_actions.reshape(-1), p=r.selected_action_probabilities.reshape(-1),
                               ret=r.rewards.reshape(-1))
        return self._cache

    def __getitem__(self, idx):
        c = self._columns()
        n = len(self)
        if isinstance(idx, (int, np.integer)):
            if not (1 <= idx <= n):
                raise PPOError(-1, "AssertionError: 1 <= idx <= length(rollouts)")         # :105-106
            t = c["idx"][idx - 1]
            return {"state": StateData(c["st"][t], c["act"][t]), "selected_action": int(c["a"][t]),
                    "selected_action_probability": float(c["p"][t]), "returns": float(c["ret"][t])}
        if isinstance(idx, (list, tuple, np.ndarray)):
            ii = np.asarray(idx, np.int64)
            if ii.size and (ii.min() < 1 or ii.max() > n):
                raise PPOError(-1, "AssertionError: dataset index out of range")
            t = c["idx"][ii - 1]
            return {"state": StateData(c["st"][t], c["act"][t]), "selected_action": c["a"][t],
                    "selected_action_probability": c["p"][t], "returns": c["ret"][t]}
        raise PPOError(-1, "Dataset index should be Int or Array, got %s" % type(idx).__name__)   # :141


def _this_module():
    import sys
    return sys.modules[__name__]


def _upload_host_rollouts(rollouts):
    """HostRollouts of StateData states -> device buffer (ppo_rollouts_set), so ppo_train_ runs the MFMA path."""
    h = rollouts._host
    vs = np.stack([np.asarray(s.vertex_score, np.int8) for s in h.state_data])
    if vs.ndim != 3 or vs.shape[2] != 72 or vs.shape[1] not in (32, 128):
        raise PPOError(-4, "states must be [H,72] int8 with H in {32,128} for the gfx950 kernels")
    carrier = HipVecEnv(num_envs=1, Q=vs.shape[1] // 4, max_actions=max(1, len(h)))
    dev = BufferRollouts()
    dev.set_columns(carrier, vs[:, None], np.array([[np.uint32(s.action_mask)] for s in h.state_data], np.uint32),
                    np.asarray(h.selected_actions, np.int64)[:, None],
                    np.asarray(h.selected_action_probabilities, np.float32)[:, None],
                    np.asarray(h.rewards, np.float32)[:, None], np.asarray(h.terminal, np.uint8)[:, None])
    return dev


def construct_dataset(rollouts):
    """construct_dataset (src/rollout_buffer.jl:145-147, src/rollouts_to_disk.jl:169-171)."""
    if isinstance(rollouts, BufferRollouts) and rollouts._h is None and rollouts._host is not None:
        if len(rollouts._host) and all(isinstance(s, StateData) for s in rollouts._host.state_data):
            rollouts._device = _upload_host_rollouts(rollouts)
            return BufferDataset(rollouts._device)
        return HostDataset(_this_module(), rollouts._host)
    if isinstance(rollouts, DiskRollouts):
        if rollouts._device is not None:
            return BufferDataset(rollouts._device)       # columns are still resident: no reload needed
        return DiskDataset(rollouts.state_data_directory)
    return BufferDataset(rollouts)


def set_disk_async(on=None):
    """Streamed collections (DiskRollouts) return without waiting for the file: the pinned ring holds the whole collection and
    the writer thread finishes rollout.bin while training runs; disk_sync(rollouts) (or the next collection) waits for it.
    None / False = the file is complete when collect_rollouts_ returns (default, the reference's behaviour)."""
    call("ppo_set_disk_async", -1 if on is None else int(bool(on)))


def _disk_async():
    """The library's mode, not a copy of it: PPO_DISK_ASYNC=1 in the environment turns it on without set_disk_async."""
    m = C.c_int32(0)
    call("ppo_get_disk_async", C.byref(m))
    return bool(m.value)


def disk_sync(rollouts):
    """Wait until the rollout file of a streamed collection is complete, then detach the store (only needed after
    set_disk_async(True); a no-op otherwise).  A write of the deferred finish that failed raises PPOError here (or at
    whichever wait point comes first: include/ppo_hip.h); rollout.bin is then gone."""
    dev = getattr(rollouts, "_device", None)
    if dev is None:                                  # (not `or`: a buffer of length 0 is falsy and still has a store)
        dev = rollouts
    if getattr(dev, "_h", None):
        try:
            call("ppo_rollouts_disk_sync", dev._h)
        finally:
            call("ppo_rollouts_detach_disk", dev._h)


def load_disk_rollouts(state_data_dir, env):
    """DiskDataset over the engine's streaming shard: <dir>/rollout.bin -> device rollout buffer."""
    ro = BufferRollouts()
    h = ro._ensure(env, 1)
    call("ppo_rollouts_load_disk", h, state_data_dir.encode())
    return ro


# ------------------------------------------------------------------ training
ADVANTAGE_MODES = {"returns": 0, "returns_normalised": 1, "gae": 2, "gae_normalised": 3}


def _adv_mode(advantage):
    """batch_advantage plugin (src/ProximalPolicyOptimization.jl:29; no implementation in the reference): "returns"
    (identity, what the reference's scripts do), "returns_normalised" ((R - mean) / (std + 1e-8) per minibatch), "gae"
    (the GAE(gamma, lambda) column of compute_gae_) or "gae_normalised"."""
    if advantage not in ADVANTAGE_MODES:
        raise PPOError(-1, "AssertionError: advantage must be one of %s" % sorted(ADVANTAGE_MODES))
    return ADVANTAGE_MODES[advantage]


def step_batch_(policy, optimizer, dataset, batch_indices, epsilon, entropy_weight, advantage="returns"):
    """One optimiser step on dataset[batch_indices] (1-based): gather + batch_advantage (=returns) +
    get_linear_action_index + step_batch! (src/train.jl:98-120, 54-84).  Returns (ppoloss, entropy_weight*entropyloss)."""
    oh = optimizer._handle(policy)
    ii = np.ascontiguousarray(np.asarray(batch_indices, np.int64) - 1)
    a, b = C.c_double(0), C.c_double(0)
    try:
        call("ppo_step_batch", policy._h, oh, dataset.rollouts._h, _p(ii, _lib.c_i64p), ii.size, float(epsilon),
             float(entropy_weight), _adv_mode(advantage), C.byref(a), C.byref(b))
    finally:
        optimizer._pull()
    return a.value, b.value


def forward_backward(policy, dataset, batch_indices, epsilon, entropy_weight, B_global=None, advantage="returns"):
    """Gradient only (no update): leaves the flat gradient in policy.grad(); returns the two losses."""
    ii = np.ascontiguousarray(np.asarray(batch_indices, np.int64) - 1)
    call("ppo_forward_backward", policy._h, dataset.rollouts._h, _p(ii, _lib.c_i64p), ii.size,
         int(B_global or ii.size), float(epsilon), float(entropy_weight), _adv_mode(advantage))
    a, b = C.c_double(0), C.c_double(0)
    call("ppo_last_losses", policy._h, C.byref(a), C.byref(b))
    return a.value, b.value


def _perm0(perm, num_epochs, n):
    """The caller's [num_epochs, n] 1-based permutations as the contiguous 0-based int64 array the library reads (None stays None)."""
    if perm is None:
        return None
    return np.ascontiguousarray(np.asarray(perm, np.int64).reshape(num_epochs, n) - 1)


def _check_batch_size(batch_size, n):
    if not (1 <= batch_size <= n):
        raise PPOError(-1, "AssertionError: 1 <= batch_size <= num_data")                    # src/train.jl:88


def ppo_train_(policy, optimizer, dataset, epsilon, batch_size, num_epochs, entropy_weight, perm=None, seed=0,
               parallel=None, verbose=True, advantage="returns"):
    """PPO.ppo_train!(policy, optimizer, dataset, epsilon, batch_size, num_epochs, entropy_weight)
    (src/train.jl:130-153) -> (ppo_loss_history, entropy_loss_history, lr_history).
    perm: optional [num_epochs, len] 1-based permutations standing in for randperm (:93)."""
    oh = optimizer._handle(policy)
    n = len(dataset)
    pp = _perm0(perm, num_epochs, n)
    ph, eh, lh = (np.zeros(num_epochs, np.float64) for _ in range(3))
    rank, world, fn, keep = 0, 1, _lib.ALLREDUCE_FN(0), None
    if parallel is not None and (parallel.world > 1 or parallel.force_hook):
        rank, world = parallel.rank, parallel.world
        keep = parallel.make_hook(policy)
        fn = keep
    # the data-parallel shards may differ in length: the batch_size assert is then made inside ppo_train on the
    # shortest shard, identically on every rank (a local raise here would leave the other ranks in a collective)
    if world == 1:
        _check_batch_size(batch_size, n)
    try:
        call("ppo_train", policy._h, oh, dataset.rollouts._h, float(epsilon), int(batch_size), int(num_epochs),
             float(entropy_weight), _adv_mode(advantage), _p(pp, _lib.c_i64p) if pp is not None else None, int(seed),
             int(rank), int(world), fn, None,
             _p(ph, _lib.c_f64p), _p(eh, _lib.c_f64p), _p(lh, _lib.c_f64p))
    finally:
        optimizer._pull()                                  # decayed ExpDecay etas: get_optimizer_learning_rate == lr_history
    ran = C.c_int32(0)                                     # fewer than num_epochs when policy.target_kl ended the call
    call("ppo_policy_last_train_stats", policy._h, 0, C.byref(ran), None, None, None, None)
    ph, eh, lh = ph[:ran.value], eh[:ran.value], lh[:ran.value]
    if verbose:
        for e in range(ran.value):                                                          # :146
            print("EPOCH : %d \t PPO LOSS : %1.4f\t ENTROPY LOSS : %1.4f \t LR : %1.1e" % (e + 1, ph[e], eh[e], lh[e]))
    return list(ph), list(eh), list(lh)                     # lr = get_optimizer_learning_rate per epoch (:144)


IMITATION_WEIGHTS = {"uniform": 0, "positive_advantage": 1}


def _imitation_modes(weights, advantage):
    """(weight_mode, adv_mode) of the imitation entry points: an unknown `weights` and the normalised advantage modes
    (the weights are max(advantage, 0) of a buffer column as it is) are refused like the library refuses them."""
    if weights not in IMITATION_WEIGHTS:
        raise PPOError(-4, "imitation weights must be one of %s" % sorted(IMITATION_WEIGHTS))
    a = _adv_mode(advantage)
    if advantage.endswith("_normalised"):
        raise PPOError(-4, "imitation: the normalised advantage modes are not supported")
    return IMITATION_WEIGHTS[weights], a


def imitate_forward_backward(policy, dataset, batch_indices, entropy_weight=0.0, weights="uniform", advantage="returns",
                             B_global=None):
    """Gradient (no update) of the behaviour-cloning loss on dataset[batch_indices] (1-based): the cross-entropy
    -(1 / B_global) sum w log pi(a | s) of the stored actions plus the entropy term of ppo_loss_with_entropy; leaves it in
    policy.grad() and returns (cross_entropy, entropy_weight * entropy loss).  weights: "uniform" (w = 1) or
    "positive_advantage" (w = max(adv, 0), self-imitation), adv the column `advantage` names: "returns", or "gae" after a
    GAE call on these rollouts.  p_old is not read."""
    wm, am = _imitation_modes(weights, advantage)
    ii = np.ascontiguousarray(np.asarray(batch_indices, np.int64) - 1)
    call("ppo_imitate_forward_backward", policy._h, dataset.rollouts._h, _p(ii, _lib.c_i64p), ii.size,
         int(B_global or ii.size), float(entropy_weight), wm, am)
    a, b = C.c_double(0), C.c_double(0)
    call("ppo_last_losses", policy._h, C.byref(a), C.byref(b))
    return a.value, b.value


def imitate_train_(policy, optimizer, dataset, batch_size, num_epochs, entropy_weight=0.0, weights="uniform",
                   advantage="returns", perm=None, seed=0, parallel=None, verbose=True):
    """ppo_train_'s epoch loop on the behaviour-cloning loss (imitate_forward_backward) -> (ce_history, entropy_history,
    lr_history), num_epochs entries each: policy.target_kl is not read, the call never stops early and leaves
    policy.last_train_stats() what the latest ppo_train_ left.  perm, seed and parallel as in ppo_train_."""
    wm, am = _imitation_modes(weights, advantage)
    oh = optimizer._handle(policy)
    n = len(dataset)
    pp = _perm0(perm, num_epochs, n)
    ch, eh, lh = (np.zeros(num_epochs, np.float64) for _ in range(3))
    rank, world, fn, keep = 0, 1, _lib.ALLREDUCE_FN(0), None
    if parallel is not None and (parallel.world > 1 or parallel.force_hook):
        rank, world = parallel.rank, parallel.world
        keep = parallel.make_hook(policy)
        fn = keep
    if world == 1:                                         # else inside the library, on the shortest shard (see ppo_train_)
        _check_batch_size(batch_size, n)
    try:
        call("ppo_imitate_train", policy._h, oh, dataset.rollouts._h, int(batch_size), int(num_epochs), float(entropy_weight),
             wm, am, _p(pp, _lib.c_i64p) if pp is not None else None, int(seed), int(rank), int(world), fn, None,
             _p(ch, _lib.c_f64p), _p(eh, _lib.c_f64p), _p(lh, _lib.c_f64p))
    finally:
        optimizer._pull()
    if verbose:
        for e in range(num_epochs):
            print("EPOCH : %d \t CE LOSS : %1.4f\t ENTROPY LOSS : %1.4f \t LR : %1.1e" % (e + 1, ch[e], eh[e], lh[e]))
    return list(ch), list(eh), list(lh)


DISTILL_TARGETS = {"column": 0, "recorded": 1}


def _distill_modes(weights, advantage, targets):
    """(weight_mode, adv_mode, target_source) of the distillation entry points, refused like the library refuses them."""
    if weights not in IMITATION_WEIGHTS:
        raise PPOError(-4, "distill weights must be one of %s" % sorted(IMITATION_WEIGHTS))
    a = _adv_mode(advantage)
    if advantage.endswith("_normalised"):
        raise PPOError(-4, "distill: the normalised advantage modes are not supported")
    if targets not in DISTILL_TARGETS:
        raise PPOError(-4, "distill targets must be one of %s" % sorted(DISTILL_TARGETS))
    return IMITATION_WEIGHTS[weights], a, DISTILL_TARGETS[targets]


def fill_targets_(rollouts, teacher):
    """Fills the rollouts' distillation target column with `teacher`'s action probabilities of every stored state, on the
    device (no host trip): what batch_action_probabilities(teacher, ...) gives for those states, bit for bit.  Any HipPolicy
    that can read the buffer's states (same F, 4 outputs; any width, depth, dtype) -- on compact storage fp32 teachers only.
    A later collection into the buffer, or set_columns, marks the column not filled.  Returns nothing."""
    if not isinstance(rollouts, BufferRollouts) or rollouts._h is None:
        raise PPOError(-4, "fill_targets_ needs a filled BufferRollouts")
    if not isinstance(teacher, HipPolicy):
        _not_implemented("action_probabilities")
    call("ppo_rollouts_fill_targets", teacher._h, rollouts._h)


def distill_forward_backward(policy, dataset, batch_indices, entropy_weight=0.0, weights="uniform", advantage="returns",
                             targets="column", B_global=None):
    """Gradient (no update) of the distillation loss on dataset[batch_indices] (1-based): the cross-entropy
    -(1 / B_global) sum w sum_k q'_k log pi(k | s) against each state's target row plus the entropy term of
    ppo_loss_with_entropy; leaves it in policy.grad() and returns (cross_entropy, entropy_weight * entropy loss).  targets:
    "column" (fill_targets_ / set_action_targets) or "recorded" (the distributions a collector recorded with
    record_probs=True).  weights and advantage as in imitate_forward_backward."""
    wm, am, ts = _distill_modes(weights, advantage, targets)
    ii = np.ascontiguousarray(np.asarray(batch_indices, np.int64) - 1)
    call("ppo_distill_forward_backward", policy._h, dataset.rollouts._h, _p(ii, _lib.c_i64p), ii.size,
         int(B_global or ii.size), float(entropy_weight), wm, am, ts)
    a, b = C.c_double(0), C.c_double(0)
    call("ppo_last_losses", policy._h, C.byref(a), C.byref(b))
    return a.value, b.value


def distill_train_(policy, optimizer, dataset, batch_size, num_epochs, entropy_weight=0.0, weights="uniform",
                   advantage="returns", targets="column", perm=None, seed=0, parallel=None, verbose=True):
    """imitate_train_'s epoch loop on the distillation loss (distill_forward_backward) -> (ce_history, entropy_history,
    lr_history), num_epochs entries each: never stops early, leaves policy.last_train_stats() and last_value_stats() alone.
    The history is the cross-entropy, whose floor is the targets' entropy (distillation_loss(..., floor=True)), not the KL."""
    wm, am, ts = _distill_modes(weights, advantage, targets)
    oh = optimizer._handle(policy)
    n = len(dataset)
    pp = _perm0(perm, num_epochs, n)
    ch, eh, lh = (np.zeros(num_epochs, np.float64) for _ in range(3))
    rank, world, fn, keep = 0, 1, _lib.ALLREDUCE_FN(0), None
    if parallel is not None and (parallel.world > 1 or parallel.force_hook):
        rank, world = parallel.rank, parallel.world
        keep = parallel.make_hook(policy)
        fn = keep
    if world == 1:                                         # else inside the library, on the shortest shard (see ppo_train_)
        _check_batch_size(batch_size, n)
    try:
        call("ppo_distill_train", policy._h, oh, dataset.rollouts._h, int(batch_size), int(num_epochs), float(entropy_weight),
             wm, am, ts, _p(pp, _lib.c_i64p) if pp is not None else None, int(seed), int(rank), int(world), fn, None,
             _p(ch, _lib.c_f64p), _p(eh, _lib.c_f64p), _p(lh, _lib.c_f64p))
    finally:
        optimizer._pull()
    if verbose:
        for e in range(num_epochs):
            print("EPOCH : %d \t CE LOSS : %1.4f\t ENTROPY LOSS : %1.4f \t LR : %1.1e" % (e + 1, ch[e], eh[e], lh[e]))
    return list(ch), list(eh), list(lh)


VALUE_TARGETS = {"returns": 0, "lambda_returns": 1}


def _value_target(target):
    if target not in VALUE_TARGETS:
        raise PPOError(-4, "value target must be one of %s" % sorted(VALUE_TARGETS))
    return VALUE_TARGETS[target]


def value_forward_backward(critic, dataset, batch_indices, target="returns", B_global=None):
    """Gradient of Flux.mse(V(dataset[batch_indices]), target) (no update): leaves it in critic.grad(); returns the loss.
    target: "returns" (the buffer's returns; never bootstrapped through time-limit truncations) or "lambda_returns" (adv + V of
    the latest GAE call on these rollouts, bootstrapped if that call was)."""
    t = _value_target(target)
    ii = np.ascontiguousarray(np.asarray(batch_indices, np.int64) - 1)
    out = C.c_double(0)
    call("ppo_value_forward_backward", critic._h, dataset.rollouts._h, _p(ii, _lib.c_i64p), ii.size,
         int(B_global or ii.size), t, C.byref(out))
    return out.value


def value_train_(critic, optimizer, dataset, batch_size, num_epochs, target="returns", perm=None, seed=0, verbose=True,
                 parallel=None):
    """ppo_train_'s epoch loop for the critic -> (mse_history, lr_history).  optimizer: any Optimiser chain, bound to the
    critic (not the one that trains the policy).  target as in value_forward_backward: "lambda_returns" follows the latest
    GAE call (bootstrapped through time-limit truncations if that call was), "returns" is the reference's compute_returns
    and is not bootstrapped.
    parallel: as in ppo_train_ -- every rank holds a replica of the critic and of its optimiser and passes its own shard;
    the replicas stay bit-identical, the mse history and critic.last_value_stats() are the global ones.  critic.value_clip
    must be the same on every rank, like policy.target_kl and num_epochs."""
    t = _value_target(target)
    oh = optimizer._handle(critic)
    n = len(dataset)
    pp = _perm0(perm, num_epochs, n)
    rank, world, fn, keep = 0, 1, _lib.ALLREDUCE_FN(0), None
    if parallel is not None and (parallel.world > 1 or parallel.force_hook):
        rank, world = parallel.rank, parallel.world
        keep = parallel.make_hook(critic)
        fn = keep
    if world == 1:                                         # else inside ppo_value_train_dp, on the shortest shard (see ppo_train_)
        _check_batch_size(batch_size, n)
    mh, lh = np.zeros(num_epochs, np.float64), np.zeros(num_epochs, np.float64)
    try:
        call("ppo_value_train_dp", critic._h, oh, dataset.rollouts._h, int(batch_size), int(num_epochs), t,
             _p(pp, _lib.c_i64p) if pp is not None else None, int(seed), int(rank), int(world), fn, None,
             _p(mh, _lib.c_f64p), _p(lh, _lib.c_f64p))
    finally:
        optimizer._pull()
    if verbose:
        for e in range(num_epochs):
            print("EPOCH : %d \t VALUE LOSS : %1.4f \t LR : %1.1e" % (e + 1, mh[e], lh[e]))
    return list(mh), list(lh)


def ppo_iterate_(policy, env, optimizer, episodes_per_iteration, minibatch_size, num_ppo_iterations, evaluator,
                 epochs_per_iteration, discount, epsilon, entropy_weight, state_data_path=None, verbose=True, *,
                 critic=None, critic_optimizer=None, gae_lambda=0.95, value_epochs=None, **options):
    """PPO.ppo_iterate! (src/train.jl:164-249), positional argument order preserved: 11 arguments = in-memory
    method, a 12th `state_data_path` = the disk method (rollouts through DiskRollouts, directory removed at
    the end, :198-201).
    critic (keyword only; None = the reference's loop, advantage = returns): a HipCritic with its own critic_optimizer.
    Each iteration then is collect, GAE(discount, gae_lambda) from the critic as it stands, ppo_train_ on that advantage,
    value_train_ on the lambda-returns for value_epochs (default epochs_per_iteration) epochs; loss gains "value".
    With policy.target_kl set (float("inf") to record without stopping) loss also gains "approx_kl" and "clip_fraction",
    one entry per epoch that ran, and with a critic "explained_variance", one per iteration, of the values the critic
    had before that iteration's update.  With critic.value_clip set, loss gains "value_clip_fraction", one entry per value
    epoch.
    parallel (keyword only; the one name **options takes -- tests/test_value_host.py pins the set of named keywords): a
    DataParallel.  `env` is then this rank's shard (DataParallel.env_shard, global_offset); ppo_train_, value_train_ and
    explained_variance_ run across the ranks, so policy, critic and every list of the loss dict are the same on all of them.
    The GAE and any advantage normalisation stay per rank.  None runs the single-process loop.
    bootstrap_truncated (keyword only, the second name **options takes; without a critic there is no GAE and it does
    nothing): every iteration's GAE bootstraps the episodes the env's time limit cut from the critic's value of the state they
    were cut in
    (compute_gae_critic_(..., bootstrap_truncated=True)), per rank like the GAE itself; loss gains "truncated", the number of
    truncated transitions per iteration (this rank's).  value_train_'s lambda-returns and "explained_variance" are then the
    bootstrapped ones.
    anchor (keyword only, the third name **options takes): a frozen HipPolicy -- a cloned or teacher policy -- that PPO stays
    anchored to.  policy.kl_anchor must be set with source "column" (PPOError otherwise, before anything runs; "recorded" is
    not taken here); every iteration runs fill_targets_(rollouts, anchor) behind its collection, ppo_train_ then minimises the
    PPO loss plus coef * KL(anchor || policy), and loss gains "anchor_kl" and "anchor_coef", one entry per epoch that ran.
    In-memory rollouts only."""
    parallel = options.pop("parallel", None)
    bootstrap = bool(options.pop("bootstrap_truncated", False))
    anchor = options.pop("anchor", None)
    if options:
        raise TypeError("ppo_iterate_() got an unexpected keyword argument %r" % sorted(options)[0])
    loss = {"ppo": [], "entropy": [], "lr": []}
    if anchor is not None:
        set_anchor = getattr(policy, "kl_anchor", None)
        if set_anchor is None:
            raise PPOError(-1, "AssertionError: ppo_iterate_(anchor=...) needs policy.kl_anchor = (coef, \"column\"[, target]) set")
        if set_anchor[1] != "column":
            raise PPOError(-4, "ppo_iterate_(anchor=...) fills the target column: policy.kl_anchor's source must be \"column\"")
        if state_data_path is not None:
            raise PPOError(-4, "an anchor with disk-backed rollouts is not supported")
        loss["anchor_kl"], loss["anchor_coef"] = [], []
    stats = getattr(policy, "target_kl", None) is not None
    if stats:
        loss["approx_kl"], loss["clip_fraction"] = [], []
        if critic is not None:
            loss["explained_variance"] = []
    if critic is not None:
        if critic_optimizer is None:
            raise PPOError(-1, "AssertionError: a critic needs its own critic_optimizer")
        if state_data_path is not None:
            raise PPOError(-4, "a critic with disk-backed rollouts is not supported")
        loss["value"] = []
        if getattr(critic, "value_clip", None) is not None:
            loss["value_clip_fraction"] = []
        if bootstrap:
            loss["truncated"] = []
    for it in range(1, num_ppo_iterations + 1):
        evaluator(policy, env, optimizer)                                                    # :181,226
        if verbose:
            print("\nPPO ITERATION : %d" % it)
        rollouts = BufferRollouts() if state_data_path is None else DiskRollouts(state_data_path)   # :185,230
        collect_rollouts_(rollouts, env, policy, episodes_per_iteration, discount)
        dataset = construct_dataset(rollouts)
        if anchor is not None:
            fill_targets_(dataset.rollouts, anchor)
        if critic is None:
            p, e, lr = ppo_train_(policy, optimizer, dataset, epsilon, minibatch_size, epochs_per_iteration,
                                  entropy_weight, parallel=parallel, verbose=verbose)
        else:
            if bootstrap:
                compute_gae_critic_(dataset.rollouts, env, critic, discount, gae_lambda, fetch=False, bootstrap_truncated=True)
                loss["truncated"].append(dataset.rollouts.n_truncated)
            else:
                compute_gae_critic_(dataset.rollouts, env, critic, discount, gae_lambda, fetch=False)
            p, e, lr = ppo_train_(policy, optimizer, dataset, epsilon, minibatch_size, epochs_per_iteration,
                                  entropy_weight, parallel=parallel, verbose=verbose, advantage="gae")
            if stats:
                loss["explained_variance"].append(explained_variance_(dataset.rollouts, "lambda_returns", parallel=parallel))
            v, _ = value_train_(critic, critic_optimizer, dataset, minibatch_size,
                                epochs_per_iteration if value_epochs is None else value_epochs,
                                target="lambda_returns", verbose=verbose, parallel=parallel)
            loss["value"] += v
            if "value_clip_fraction" in loss:
                loss["value_clip_fraction"] += critic.last_value_stats()["clip_fraction"]
        loss["ppo"] += p
        loss["entropy"] += e
        loss["lr"] += lr
        if stats:
            st = policy.last_train_stats()
            loss["approx_kl"] += st["approx_kl"]
            loss["clip_fraction"] += st["clip_fraction"]
        if anchor is not None:
            ast = policy.last_anchor_stats()
            loss["anchor_kl"] += ast["anchor_kl"]
            loss["anchor_coef"] += ast["anchor_coef"]
        save_loss(evaluator, loss)       # :196,247 -- like the reference, an evaluator without a save_loss method throws
    if state_data_path is not None and os.path.isdir(state_data_path):
        if verbose:
            print("\n\nCLEARING DATA IN ROLLOUTS FOLDER :")                                 # :199
        shutil.rmtree(state_data_path)
    return loss


def average_returns(policy, env, num_trajectories):
    """PPO.average_returns(policy, env, num_trajectories) (src/evaluate.jl:18-25) -> (mean, std) of the
    undiscounted episode return under the stochastic policy (std with the n-1 correction like Flux.std).  On a HipVecEnv
    the actions are chosen under policy.selection; the default is the reference's rule."""
    if not isinstance(env, HipVecEnv):
        return generic.average_returns_host(_this_module(), policy, env, num_trajectories)
    per_env = -(-int(num_trajectories) // env.N)
    return _mean_std("ppo_average_returns", env, policy, num_trajectories, per_env * env.max_actions)


def _evaluator_scratch(env, T=1):
    scratch = BufferRollouts()
    return scratch, scratch._ensure(env, T)


def _mean_std(name, env, policy, num_trajectories, scratch_T=1):
    """(mean, std) of the evaluator export `name` over num_trajectories trajectories, on a scratch buffer of scratch_T steps."""
    scratch, h = _evaluator_scratch(env, scratch_T)
    m, s = C.c_double(0), C.c_double(0)
    call(name, policy._h, env._h, h, int(num_trajectories), C.byref(m), C.byref(s))
    return m.value, s.value


def average_best_returns(env, policy, num_trajectories):
    """average_best_returns(wrapper, policy, num_trajectories) (test/quad_game_utilities.jl:299-307; note the
    reference's argument order: env first) -> (mean, std) of initial_score - lowest score seen on the trajectory."""
    return _mean_std("ppo_average_best_returns", env, policy, num_trajectories)


def average_normalized_returns(env, policy, num_trajectories):
    """average_normalized_returns(wrapper, policy, num_trajectories) (test/quad_game_utilities.jl:380-387) ->
    (mean, std) of best return / (initial_score - opt_score); a trajectory that starts at its optimum counts 1.0."""
    return _mean_std("ppo_average_normalized_returns", env, policy, num_trajectories)


def evaluate_trajectories(env, policy, num_trajectories, kind):
    """Per-trajectory values behind the three evaluators: kind "return" (single_trajectory_return, src/evaluate.jl:1-16),
    "best" (best_single_trajectory_return, test/quad_game_utilities.jl:280-296) or "normalized"
    (single_trajectory_normalized_return, :369-378).  Env-major order: env n's trajectories are consecutive."""
    k = {"return": 1, "best": 2, "normalized": 3}[kind]
    scratch, h = _evaluator_scratch(env)
    out = np.zeros(int(num_trajectories), np.float64)
    call("ppo_evaluate_trajectories", policy._h, env._h, h, int(num_trajectories), k, _p(out, _lib.c_f64p))
    return out


# ------------------------------------------------------------------ best state of a rollout, best-of-K search
def check_internal(score, degree, active, Q):
    """What HipVecEnv.set_internal and search_best_states_ require of caller-supplied env states (ppo_env_set_internal checks
    the same before it uploads anything): score, degree [n, 4Q] int8, active [n] active-quad words with active != 0, no bit
    at or above Q, and every entry of an inactive quad 0 in both arrays.  Returns the three arrays C-contiguous;
    PPOError(PPO_ERR_ARG) otherwise."""
    V = 4 * int(Q)
    sc, dg = np.ascontiguousarray(score, np.int8), np.ascontiguousarray(degree, np.int8)
    act = np.ascontiguousarray(np.atleast_1d(active), np.uint32)
    if sc.ndim != 2 or sc.shape[1] != V or dg.shape != sc.shape or act.shape != (sc.shape[0],):
        raise PPOError(-1, "AssertionError: env state: score and degree must be [n, %d], active [n]" % V)
    if np.any(act == 0):
        raise PPOError(-1, "AssertionError: env state: no active quad")
    if Q < 32 and np.any(act >> np.uint32(Q)):
        raise PPOError(-1, "AssertionError: env state: active bit at or above Q")
    off = ((act[:, None] >> (np.arange(V, dtype=np.uint32) >> 2)[None, :]) & 1) == 0
    if np.any(sc[off]) or np.any(dg[off]):
        raise PPOError(-1, "AssertionError: env state: nonzero entry of an inactive quad")
    return sc, dg, act


def _paths_out(raw):
    """0-based device rows with -1 as padding -> the reference's 1-based action indices with 0 as padding."""
    return (raw + 1).astype(np.int16)


def _best_states(env, policy, num_trajectories, reset_first, scores, action_types, actions=False):
    nt, V = int(num_trajectories), 4 * env.Q
    scratch, h = _evaluator_scratch(env)
    st, act = np.zeros((nt, 2 * V), np.int8), np.zeros(nt, np.uint32)
    gap, step, length, init = (np.zeros(nt, np.int32) for _ in range(4))
    tr = np.zeros((nt, env.max_actions), np.int32) if scores else None
    tc = np.zeros((nt, 4), np.int32) if action_types else None
    args = (policy._h, env._h, h, nt, int(bool(reset_first)), _p(st, _lib.c_i8p), _p(act, _lib.c_u32p),
            _p(gap, _lib.c_i32p), _p(step, _lib.c_i32p), _p(length, _lib.c_i32p), _p(init, _lib.c_i32p),
            None if tr is None else _p(tr, _lib.c_i32p), None if tc is None else _p(tc, _lib.c_i32p))
    if actions:
        ac = np.zeros((nt, env.max_actions), np.int16)
        call("ppo_best_states_actions", *args, _p(ac, _lib.c_i16p))
    else:
        call("ppo_best_states", *args)
    out = dict(best_state=st, best_score=st[:, :V], best_degree=st[:, V:], best_active=act, best_gap=gap, best_step=step,
               length=length, initial_gap=init)
    if scores:
        out["trace"] = tr
    if action_types:
        out["type_counts"] = tc
    if actions:
        out["actions"] = _paths_out(ac)
    return out


def best_states_(env, policy, num_trajectories, scores=False, action_types=False, actions=False):
    """best_state_in_rollout (test/quad_game_utilities.jl:341-358) over num_trajectories trajectories in the
    average_best_returns convention: trajectory e on env e mod N, reset! before each, env-major output.  Returns a dict of
    arrays, one row per trajectory: best_state [2V] (best_score / best_degree are its halves), best_active, best_gap
    (current_score - opt_score of that state), best_step (steps played when it was reached, 0 = the start: the first
    minimum, like argmin), length, initial_gap; scores=True adds trace [max_actions] (single_trajectory_scores:
    initial_score - current_score behind every step, INT32_MIN behind the end), action_types=True adds type_counts [4],
    actions=True adds actions [max_actions] int16: the trajectory's 1-based action indices (as selected_actions and step_
    speak them), 0 behind its end; the first best_step of them lead from the trajectory's start to best_state."""
    return _best_states(env, policy, num_trajectories, True, scores, action_types, actions)


def best_state_in_rollout(env, policy, rng=None):
    """best_state_in_rollout(wrapper, policy) (test/quad_game_utilities.jl:341-358), the reference's argument order: every
    env plays one stochastic trajectory from the state it holds (no reset!, no episode counter consumed) and the state at
    argmin(current_score - opt_score) comes back -- for a HipVecEnv the dict of best_states_ over all N envs, for any other
    env object a deep copy of it in that state."""
    if not isinstance(env, HipVecEnv):
        return generic.best_state_in_rollout(_this_module(), env, policy, rng)
    return _best_states(env, policy, env.N, False, False, False)


def single_trajectory_scores(env, policy, rng=None):
    """single_trajectory_scores(wrapper, policy) (test/quad_game_utilities.jl:309-323): initial_score - current_score behind
    every step of one trajectory from the current state.  HipVecEnv: a list of N int32 arrays, one per env."""
    if not isinstance(env, HipVecEnv):
        return generic.single_trajectory_scores(_this_module(), env, policy, rng)
    r = _best_states(env, policy, env.N, False, True, False)
    return [r["trace"][n, :r["length"][n]].copy() for n in range(env.N)]


def count_non_flips(env, policy, rng=None):
    """count_non_flips(wrapper, policy) (test/random_quad.jl:9-27): how many actions of one trajectory from the current
    state were of type 3 or 4 (1-based; a % 4 >= 2 here).  HipVecEnv: int64 [N]."""
    if not isinstance(env, HipVecEnv):
        return generic.count_non_flips(_this_module(), env, policy, rng)
    r = _best_states(env, policy, env.N, False, False, True)
    return r["type_counts"][:, 2:].sum(axis=1, dtype=np.int64)


def _search_io(env, sc, dg, act, K, clone_gaps):
    """What both searches pass and return: (scratch, args, out, cg) -- the scratch buffer (the caller keeps it alive across the
    call), the exports' common arguments from the env handle to clone_gaps, the result dict over freshly allocated output
    arrays, and the clone_gaps array or None."""
    M, V = sc.shape[0], 4 * env.Q
    scratch, h = _evaluator_scratch(env)
    st, bact = np.zeros((M, 2 * V), np.int8), np.zeros(M, np.uint32)
    gap, clone, step, init = (np.zeros(M, np.int32) for _ in range(4))
    cg = np.zeros((M, K), np.int32) if clone_gaps else None
    args = (env._h, h, M, K, _p(sc, _lib.c_i8p), _p(dg, _lib.c_i8p), _p(act, _lib.c_u32p),
            _p(st, _lib.c_i8p), _p(bact, _lib.c_u32p), _p(gap, _lib.c_i32p), _p(clone, _lib.c_i32p), _p(step, _lib.c_i32p),
            _p(init, _lib.c_i32p), None if cg is None else _p(cg, _lib.c_i32p))
    out = dict(best_state=st, best_score=st[:, :V], best_degree=st[:, V:], best_active=bact, best_gap=gap, best_clone=clone,
               best_step=step, initial_gap=init)
    return scratch, args, out, cg


def search_best_states_(env, policy, score, degree, active, K, clone_gaps=False, path=False):
    """Best of K stochastic trajectories from each caller-supplied start state (score, degree [M, 4Q], active [M]):
    K resident envs are loaded with one start and, sampling being keyed on (global env id, tick), play K different
    trajectories; N // K starts run at a time.  Returns a dict of arrays, one row per start: best_state [2V] (best_score /
    best_degree), best_active, best_gap, best_clone, best_step, initial_gap; clone_gaps=True adds clone_gaps [M, K].  Ties go
    to the lowest clone, then its first minimum.  No reset! runs: episode counters stay, ticks advance by the steps played,
    the envs that played are left terminal.  path=True adds path [M, max_actions] int16: the winner's best_step 1-based
    actions from the start to best_state, 0 behind them (apply_paths_ replays them)."""
    sc, dg, act = check_internal(score, degree, active, env.Q)
    K = int(K)
    if not 1 <= K <= env.N:
        raise PPOError(-1, "AssertionError: search_best_states: 1 <= K <= N")
    scratch, args, out, cg = _search_io(env, sc, dg, act, K, clone_gaps)
    if path:
        pa = np.zeros((sc.shape[0], env.max_actions), np.int16)
        call("ppo_search_best_states_path", policy._h, *args, _p(pa, _lib.c_i16p))
    else:
        call("ppo_search_best_states", policy._h, *args)
    if clone_gaps:
        out["clone_gaps"] = cg
    if path:
        out["path"] = _paths_out(pa)
    return out


RESAMPLE_MAX_K = 4096        # k_search_resample stages one 8-byte rank key per clone in LDS


def check_resample(N, K, interval, survivors):
    """What search_resample_states_ requires of its schedule on N envs (ppo_search_resample_states checks the same):
    interval >= 1 and 1 <= survivors <= K <= N, else PPOError(PPO_ERR_ARG); K above RESAMPLE_MAX_K is
    PPOError(PPO_ERR_UNSUPPORTED).  Returns the three as ints."""
    K, R, m0 = int(K), int(interval), int(survivors)
    if R < 1:
        raise PPOError(-1, "AssertionError: search_resample_states: interval must be >= 1")
    if not 1 <= m0 <= K <= int(N):
        raise PPOError(-1, "AssertionError: search_resample_states: 1 <= survivors <= K <= N")
    if K > RESAMPLE_MAX_K:
        raise PPOError(-4, "search_resample_states: K above %d clones is not supported" % RESAMPLE_MAX_K)
    return K, R, m0


SELECT_RULES = ("sample", "greedy")        # PPO_SELECT_SAMPLE, PPO_SELECT_GREEDY


def check_selection(rule, temperature=1.0):
    """What HipPolicy.selection requires (ppo_policy_set_selection checks the same): rule "sample" or "greedy", temperature
    finite and > 0, else PPOError(PPO_ERR_ARG).  Returns (rule, float(temperature)); touches no library."""
    if not isinstance(rule, str) or rule not in SELECT_RULES:
        raise PPOError(-1, "AssertionError: selection: rule must be 'sample' or 'greedy'")
    try:
        t = float(temperature)
    except (TypeError, ValueError):
        raise PPOError(-1, "AssertionError: selection: temperature must be a number")
    if not (np.isfinite(t) and t > 0.0):
        raise PPOError(-1, "AssertionError: selection: temperature must be finite and > 0")
    return rule, t


DEFAULT_TRUNCATION = (0, 1.0)


def check_truncation(top_k=0, top_p=1.0):
    """What HipPolicy.truncation requires (ppo_policy_set_truncation checks the same): top_k an integer >= 0 that fits an int32
    (0: no limit), top_p a number in (0, 1] (1: no limit), else PPOError(PPO_ERR_ARG).  Returns (int(top_k), float(top_p));
    touches no library."""
    if isinstance(top_k, (bool, np.bool_)) or not isinstance(top_k, (int, np.integer)):
        raise PPOError(-1, "AssertionError: truncation: top_k must be an integer")
    if not 0 <= int(top_k) <= 2 ** 31 - 1:
        raise PPOError(-1, "AssertionError: truncation: top_k must be >= 0 (0: no limit) and fit an int32")
    try:
        p = float(top_p)
    except (TypeError, ValueError):
        raise PPOError(-1, "AssertionError: truncation: top_p must be a number")
    if not (p > 0.0 and p <= 1.0):
        raise PPOError(-1, "AssertionError: truncation: top_p must be in (0, 1] (1: no limit)")
    return int(top_k), p


@contextlib.contextmanager
def selecting(policy, rule="sample", temperature=1.0, top_k=0, top_p=1.0):
    """with selecting(policy, "greedy"): ... -- sets policy.selection and policy.truncation for the block and restores the previous
    ones on exit, e.g. inside an evaluator callback of ppo_iterate_ so that the collectors' policy is scored by its mode, or
    around a search: with selecting(policy, "sample", 2.0, top_p=0.9): search_best_states_(...)."""
    new = check_selection(rule, temperature)
    new_trunc = check_truncation(top_k, top_p)
    old, old_trunc = policy.selection, policy.truncation
    policy.selection = new
    policy.truncation = new_trunc
    try:
        yield policy
    finally:
        policy.selection = old
        policy.truncation = old_trunc


def search_resample_states_(env, policy, score, degree, active, K, interval, survivors, donors=False, clone_gaps=False,
                            path=False, critic=None, value_weight=1.0, values=False):
    """search_best_states_ with resampling: behind every `interval`-th step of a round (t % interval == 0, t < max_actions)
    each start folds its K clones' records into its result (the lowest (best_gap, clone); the first fold as it is, later
    ones only on a strictly lower gap), ranks its live clones by (current_score - opt_score now, clone) and overwrites
    every clone of rank r >= m = min(survivors, live) with state, record and step count of the clone of rank (r - m) % m.
    The copies keep their own ticks, so they diverge at the next step.  One more fold behind the round's last step gives the
    result.  Returns the dict of search_best_states_ (best_step counts steps along the lineage); donors=True adds donors
    [M, E, K] int32 with E = (max_actions - 1) // interval: a receiver's donor clone, -1 a live clone that kept its state, -2
    a terminal clone or an event that no longer ran; clone_gaps=True adds every clone's record gap at the last fold.
    interval >= max_actions runs no event (search_best_states_); survivors == K copies nothing.  path=True adds path
    [M, max_actions] int16: the best_step 1-based actions that lead from the start to best_state along the result's lineage
    (a copy carries the donor's actions with its record), 0 behind them.  HipVecEnv only.
    critic (a HipCritic): the live clones rank by where the critic expects them to end instead of where they
    are -- by the fp32 number fmaf(-value_weight, V(s), cur_gap), V(s) the critic's value of the state the clone holds behind
    the step (0 where it is not finite), computed on the device in front of every event.  The fold, the ranks and the copy
    stay as they are; value_weight = 0 is the call without a critic.  values=True (needs a critic) adds event_values
    [M, E, K] float32: the V(s) every live clone was ranked with, NaN for a terminal clone or an event that no longer ran.
    value_weight must be finite and >= 0.  Without a critic the call is the one it has always been."""
    if not isinstance(env, HipVecEnv):
        raise PPOError(-4, "search_resample_states_ needs a HipVecEnv")
    if critic is None and values:
        raise PPOError(-1, "AssertionError: search_resample_states: values=True needs a critic")
    if critic is not None and not (np.isfinite(np.float32(value_weight)) and float(value_weight) >= 0.0):
        raise PPOError(-1, "AssertionError: search_resample_states: value_weight must be finite and >= 0")
    sc, dg, act = check_internal(score, degree, active, env.Q)
    M = sc.shape[0]
    K, R, m0 = check_resample(env.N, K, interval, survivors)
    scratch, args, out, cg = _search_io(env, sc, dg, act, K, clone_gaps)
    args += (R, m0)
    dn = np.full((M, (env.max_actions - 1) // R, K), -2, np.int32) if donors else None
    ev = np.full((M, (env.max_actions - 1) // R, K), np.nan, np.float32) if values else None
    pa = np.zeros((M, env.max_actions), np.int16) if path else None
    dnp = None if dn is None else _p(dn, _lib.c_i32p)
    if critic is not None:
        call("ppo_search_resample_states_value", policy._h, critic._h, *args, float(value_weight), dnp,
             None if ev is None else _p(ev, _lib.c_f32p), None if pa is None else _p(pa, _lib.c_i16p))
    elif path:
        call("ppo_search_resample_states_path", policy._h, *args, dnp, _p(pa, _lib.c_i16p))
    else:
        call("ppo_search_resample_states", policy._h, *args, dnp)
    if donors:
        out["donors"] = dn
    if clone_gaps:
        out["clone_gaps"] = cg
    if path:
        out["path"] = _paths_out(pa)
    if values:
        out["event_values"] = ev
    return out


BEAM_MAX_K = 256             # k_beam_select stages the chosen keys and the weights in LDS, one thread per slot


BEAM_DISTINCT_MODES = {None: 0, "children": 1, "parents": 2}
BEAM_MAX_ROUNDS = 16         # windows of 256 candidates a step of the distinct beam may examine


def beam_search_states_(env, policy, score, degree, active, K, path=False, log=False):
    """Beam search: the K action sequences from each caller-supplied start (score, degree [M, 4Q], active [M])
    to which the policy gives the highest probability -- deterministic, seed-free, the greedy trajectory at K = 1.  K resident
    envs, the start's slots, are loaded with one start; N // K starts run at a time.  A slot carries a weight (mant, exp), an
    fp64 in [0.5, 1) and an int32 standing for the path probability mant * 2^exp; slot 0 starts live with (0.5, 1), the others
    dead.  Every step scores the candidates (live slot k, action a with p[k][a] > 0) by ONE fp64 multiply mant_k * p[k][a],
    re-normalised by frexp; the first min(K, #candidates) in the order (exp descending, mant descending, k * A + a ascending)
    become slots 0, 1, ..., each taking its parent's state and playing its action.  A start's result is its load state (step
    0) until a live slot's gap is strictly below it, then the lowest (gap, slot) of that step; it finishes at gap 0 or after
    max_actions steps.  policy.selection and policy.truncation are not read.
    Returns a dict of arrays, one row per start: best_state [2V] (best_score / best_degree), best_active, best_gap, best_step,
    initial_gap, best_beam (the slot the result was taken from) and log_prob, float64: log(best_mant) + best_exp * log(2),
    the log of the policy's probability of the path (0.0 at step 0).  path=True adds path [M, max_actions] int16: the
    best_step 1-based actions from the start to best_state, 0 behind them (apply_paths_ replays them).  log=True adds the
    back-pointer log, [M, max_actions, K]: parents and actions (int16, 1-based, 0 for a dead slot or a step that did not run),
    mant (float64) and exp (int32), 0 there.  No reset! runs and nothing is sampled: ticks and episode counters stay, the
    slots' envs are left terminal, envs at and beyond (N // K) * K are untouched.  HipVecEnv and fp32 policies only; K above
    BEAM_MAX_K is PPOError(PPO_ERR_UNSUPPORTED)."""
    return beam_search_states_distinct_(env, policy, score, degree, active, K, path=path, log=log, distinct=None)


def beam_search_states_distinct_(env, policy, score, degree, active, K, path=False, log=False, distinct=None, rounds=4):
    """beam_search_states_ with two more keywords; everything said there holds.
    distinct="children" or "parents"  keeps K DIFFERENT states per step: the candidates are taken in the same
    order, at most 256 * rounds of them (1 <= rounds <= 16); each is played, and a child whose state (score, degree, active)
    equals that of a child accepted before it -- under "parents" also that of a slot live in front of the step -- is rejected;
    the others become slots 0, 1, ... until K are accepted, each with its own weight.  A start also finishes when a step
    accepts nothing.  log=True then adds rank [M, max_actions, K] int32 (the 0-based position of the slot's candidate in the
    step's order, -1 for a dead slot or a step that did not run) and examined [M, max_actions] int32 (the candidates the step
    looked at, -1 for a step that did not run).  distinct=None is the plain beam: rounds is not read."""
    if not isinstance(env, HipVecEnv):
        raise PPOError(-4, "beam_search_states_ needs a HipVecEnv")
    if not (distinct is None or isinstance(distinct, str)) or distinct not in BEAM_DISTINCT_MODES:
        raise PPOError(-1, "AssertionError: beam_search_states: distinct must be None, \"children\" or \"parents\"")
    mode = BEAM_DISTINCT_MODES[distinct]
    if mode and not (isinstance(rounds, (int, np.integer)) and 1 <= int(rounds) <= BEAM_MAX_ROUNDS):
        raise PPOError(-1, "AssertionError: beam_search_states: need 1 <= rounds <= %d" % BEAM_MAX_ROUNDS)
    sc, dg, act = check_internal(score, degree, active, env.Q)
    K = int(K)
    if not 1 <= K <= env.N:
        raise PPOError(-1, "AssertionError: beam_search_states: 1 <= K <= N")
    if K > BEAM_MAX_K:
        raise PPOError(-4, "beam_search_states: K above %d slots is not supported" % BEAM_MAX_K)
    M, V, T = sc.shape[0], 4 * env.Q, env.max_actions
    scratch, h = _evaluator_scratch(env)
    st, bact = np.zeros((M, 2 * V), np.int8), np.zeros(M, np.uint32)
    gap, beam, step, init, bexp = (np.zeros(M, np.int32) for _ in range(5))
    bmant = np.zeros(M, np.float64)
    pa = np.zeros((M, T), np.int16) if path else None
    lp, la = (np.zeros((M, T, K), np.int16) for _ in range(2)) if log else (None, None)
    lm = np.zeros((M, T, K), np.float64) if log else None
    le = np.zeros((M, T, K), np.int32) if log else None
    args = (policy._h, env._h, h, M, K, _p(sc, _lib.c_i8p), _p(dg, _lib.c_i8p), _p(act, _lib.c_u32p),
            _p(st, _lib.c_i8p), _p(bact, _lib.c_u32p), _p(gap, _lib.c_i32p), _p(beam, _lib.c_i32p), _p(step, _lib.c_i32p),
            _p(init, _lib.c_i32p), _p(bmant, _lib.c_f64p), _p(bexp, _lib.c_i32p),
            None if pa is None else _p(pa, _lib.c_i16p), None if lp is None else _p(lp, _lib.c_i16p),
            None if la is None else _p(la, _lib.c_i16p), None if lm is None else _p(lm, _lib.c_f64p),
            None if le is None else _p(le, _lib.c_i32p))
    lr = np.zeros((M, T, K), np.int32) if log and mode else None
    lx = np.zeros((M, T), np.int32) if log and mode else None
    if mode:
        call("ppo_beam_search_states_distinct", *args, mode, int(rounds), None if lr is None else _p(lr, _lib.c_i32p),
             None if lx is None else _p(lx, _lib.c_i32p))
    else:
        call("ppo_beam_search_states", *args)
    out = dict(best_state=st, best_score=st[:, :V], best_degree=st[:, V:], best_active=bact, best_gap=gap, best_step=step,
               initial_gap=init, best_beam=beam, log_prob=np.log(bmant) + bexp.astype(np.float64) * np.log(2.0))
    if path:
        out["path"] = _paths_out(pa)
    if log:
        out.update(parents=_paths_out(lp), actions=_paths_out(la), mant=lm, exp=le)
        if mode:
            out.update(rank=lr, examined=lx)
    return out


def check_paths(paths, M, Q):
    """What apply_paths_ requires of its paths (ppo_env_apply_paths checks the same): an integer array [M, stride] with
    stride >= 1 of 1-based action indices <= 16 Q, anything <= 0 ending a path.  Returns them 0-based, int16, C-contiguous
    (-1 where a path has ended); PPOError(PPO_ERR_ARG) otherwise."""
    pa = np.asarray(paths)
    if pa.ndim != 2 or pa.shape[0] != int(M) or pa.shape[1] < 1 or not np.issubdtype(pa.dtype, np.integer):
        raise PPOError(-1, "AssertionError: env_apply_paths: paths must be an integer array [%d, stride], stride >= 1" % int(M))
    if np.any(pa > 16 * int(Q)):
        raise PPOError(-1, "AssertionError: env_apply_paths: action index out of range")
    return np.ascontiguousarray(np.maximum(pa.astype(np.int64), 0) - 1, np.int16)


def apply_paths_(env, score, degree, active, paths, scores=False):
    """Teacher-forced replay without a policy: path m (paths [M, stride], 1-based action indices as selected_actions, step_
    and the path / actions outputs of the searches speak them, 0 behind a path's end) is applied to start m (score, degree
    [M, 4Q], active [M]), which begins as reset! leaves an env.  A path ends at its first 0, after stride entries or once
    the state is terminal.  Returns a dict of arrays, one row per path: state [2V] (score / degree are its halves), active,
    gap, applied (the actions stepped); scores=True adds trace [stride] (initial_score - current_score behind every step,
    INT32_MIN behind applied).  env supplies Q, max_actions and no_action_reward only: its resident envs, ticks and counters
    are unchanged.  Replaying a search's path from its start gives best_state, best_active, best_gap and applied ==
    best_step.  HipVecEnv only."""
    if not isinstance(env, HipVecEnv):
        raise PPOError(-4, "apply_paths_ needs a HipVecEnv")
    sc, dg, act = check_internal(score, degree, active, env.Q)
    M, V = sc.shape[0], 4 * env.Q
    pa = check_paths(paths, M, env.Q)
    stride = pa.shape[1]
    st, oact = np.zeros((M, 2 * V), np.int8), np.zeros(M, np.uint32)
    gap, applied = np.zeros(M, np.int32), np.zeros(M, np.int32)
    tr = np.zeros((M, stride), np.int32) if scores else None
    call("ppo_env_apply_paths", env._h, M, _p(sc, _lib.c_i8p), _p(dg, _lib.c_i8p), _p(act, _lib.c_u32p), _p(pa, _lib.c_i16p),
         stride, _p(st, _lib.c_i8p), _p(oact, _lib.c_u32p), _p(gap, _lib.c_i32p), _p(applied, _lib.c_i32p),
         None if tr is None else _p(tr, _lib.c_i32p))
    out = dict(state=st, score=st[:, :V], degree=st[:, V:], active=oact, gap=gap, applied=applied)
    if scores:
        out["trace"] = tr
    return out


# ------------------------------------------------------------------ data parallel (one process per GPU)
class _DevArray:
    """Exposes a raw device pointer through __cuda_array_interface__ so torch can alias it."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (ptr, False), "version": 3,
                                         "strides": None}


class DataParallel:
    """Env shards are data-parallel across ranks; the only exchange is one all-reduce (sum) of the flat
    gradient buffer [num_params + 2] per optimiser step, through torch.distributed (backend "nccl" = RCCL
    over xGMI on MI355X; "gloo" for the CPU rehearsal of the host logic)."""

    def __init__(self, rank=0, world=1, force_hook=False):
        self.rank, self.world = int(rank), int(world)
        self.force_hook = bool(force_hook)      # exercise the all-reduce hook even with one rank (tests)
        self.hook_kind = None                   # set by make_hook: "native-rccl" or "torch.distributed/<backend>"

    def env_shard(self, total_envs):
        """Contiguous shard [offset, offset+n) of this rank; RNG uses global env ids."""
        base, rem = divmod(int(total_envs), self.world)
        n = base + (1 if self.rank < rem else 0)
        off = self.rank * base + min(self.rank, rem)
        return off, n

    @staticmethod
    def allreduce_(tensor):
        """Sum all-reduce in place.  "nccl" (= RCCL) reduces the device tensor on the current stream; with the "gloo"
        backend (CPU rehearsal: several ranks sharing one GPU in the tests) a device tensor takes a host round trip."""
        import torch.distributed as dist
        if tensor.is_cuda and dist.get_backend() == "gloo":
            host = tensor.cpu()                       # synchronises with the stream the engine runs on
            dist.all_reduce(host, op=dist.ReduceOp.SUM)
            tensor.copy_(host)
            return tensor
        dist.all_reduce(tensor, op=dist.ReduceOp.SUM)
        return tensor

    def _native_rccl_hook(self):
        global _NATIVE_RCCL_HOOK                   # one in-library communicator per process, created on first use
        if _NATIVE_RCCL_HOOK is False:
            _NATIVE_RCCL_HOOK = _native_rccl_hook_impl(self.rank, self.world)
        return _NATIVE_RCCL_HOOK

    def make_hook(self, policy):
        """The ppo_allreduce_fn handed to ppo_train.  Default: the library's own RCCL all-reduce (ppo_rccl_*), adopted
        only if EVERY rank brought its communicator up and passed the known-answer all-reduce (the decision is itself
        collective, so the ranks can never end up on different collectives); otherwise -- or with PPO_NATIVE_RCCL=0, or
        on the gloo rehearsal backend -- one torch.distributed all-reduce per step on a tensor aliasing the buffer."""
        import torch
        import torch.distributed as dist
        # the engine must run on the stream torch orders its collectives against
        call("ppo_set_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))
        ptr, n = policy.grad_buffer_dev()
        if os.environ.get("PPO_NATIVE_RCCL", "1") != "0" and dist.get_backend() != "gloo":
            native = self._native_rccl_hook()
            if native is not None:
                self.hook_kind = "native-rccl"
                return native
        self.hook_kind = "torch.distributed/" + dist.get_backend()

        views = {}

        def reduce(dev_ptr, n_floats):             # also serves ppo_train's small shard-length exchange
            t = views.get((dev_ptr, n_floats)) if dev_ptr == ptr else None
            if t is None:
                t = torch.as_tensor(_DevArray(dev_ptr, n_floats), device="cuda")
                if dev_ptr == ptr:                 # the gradient buffer lives as long as the policy: keep its view
                    views[(dev_ptr, n_floats)] = t
            self.allreduce_(t)

        def hook(ctx, dev_ptr, n_floats):
            try:
                reduce(dev_ptr, n_floats)
                return 0
            except Exception:                      # noqa: BLE001 -- reported through the status code
                return 1
        return _lib.ALLREDUCE_FN(hook)


_NATIVE_RCCL_HOOK = False                          # False: not tried yet; None: not adopted (torch hook stays)


def _native_rccl_hook_impl(rank, world):
    """ppo_rccl_* (include/ppo_hip.h): the unique id travels over the host's process group, the all-reduce itself is
    one RCCL call made by the library on its own stream.  Every stage is followed by a MIN all-reduce of a success
    flag over the host group, and rank 0 always reaches the broadcast (sending a zero id if it could not make one):
    either all ranks adopt the native communicator or all of them keep the torch.distributed hook."""
    import torch
    import torch.distributed as dist

    def all_ok(ok):
        t = torch.tensor([1 if ok else 0], dtype=torch.int32, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        return bool(t.item())

    why = ""
    uid = np.zeros(128, np.uint8)
    # stage 0: every rank must be able to resolve RCCL before any rank enters the collective ncclCommInitRank
    probe = lib().ppo_rccl_probe() == 0
    if not all_ok(probe):
        sys.stderr.write("rank %d: native RCCL hook not adopted (librccl %s here); every rank uses the torch.distributed hook\n"
                         % (rank, "resolved" if probe else "not found"))
        return None
    if rank == 0:
        try:
            call("ppo_rccl_unique_id", uid.ctypes.data_as(C.c_void_p))
        except Exception as e:                  # noqa: BLE001
            uid[:] = 0
            why = str(e)
    t = torch.from_numpy(uid).cuda()
    dist.broadcast(t, 0)
    uid = np.ascontiguousarray(t.cpu().numpy())
    ok = bool(uid.any())
    if ok:
        try:
            call("ppo_rccl_init", int(rank), int(world), uid.ctypes.data_as(C.c_void_p))
        except Exception as e:                  # noqa: BLE001
            ok, why = False, str(e)
    if all_ok(ok):
        try:                                    # collective known-answer all-reduce on the new communicator
            good = C.c_int32(0)
            call("ppo_rccl_self_test", C.byref(good))
            r_, w_ = C.c_int32(-1), C.c_int32(-1)
            call("ppo_rccl_comm_info", C.byref(r_), C.byref(w_))
            ok = bool(good.value) and r_.value == rank and w_.value == world
            if not ok:
                why = "known-answer all-reduce / communicator size check failed"
        except Exception as e:                  # noqa: BLE001
            ok, why = False, str(e)
        if all_ok(ok):
            return _lib.ALLREDUCE_FN(C.cast(_lib.lib().ppo_rccl_allreduce, C.c_void_p).value)
    try:
        lib().ppo_rccl_finalize()
    except Exception:                           # noqa: BLE001
        pass
    sys.stderr.write("rank %d: native RCCL hook not adopted (%s); every rank uses the torch.distributed hook\n"
                     % (rank, why or "another rank failed"))
    return None


def rccl_finalize():
    """Destroy the library's communicator (if any) and forget the cached native hook, so a later process group can
    build a new one."""
    global _NATIVE_RCCL_HOOK
    _NATIVE_RCCL_HOOK = False
    call("ppo_rccl_finalize")


def rccl_comm_info():
    """(rank, world) as the library's own communicator reports them, or None when the native hook is not in use."""
    r_, w_ = C.c_int32(-1), C.c_int32(-1)
    if lib().ppo_rccl_comm_info(C.byref(r_), C.byref(w_)) != 0:
        return None
    return r_.value, w_.value


# ---------------------------------------------------------------- checkpoints (BSON.@save / BSON.@load of the policy)
def save_policy(path, policy):
    """BSON.@save path policy (examples/triangle/distance_weighted/triangle_utilities.jl:370-373): the document
    BSON.jl writes for SimplePolicy.Policy, readable by the reference."""
    checkpoint.save_policy(path, policy)


def load_policy(path, seed=0, dtype="f32"):
    """BSON.@load path policy -> HipPolicy holding the saved Float32 weights (e.g. the reference's test/output/*.bson)."""
    return checkpoint.load_policy(path, HipPolicy, seed=seed, dtype=dtype)


# ---------------------------------------------------------------- remaining reference entry points (host mirrors)
def update_rollouts_(buffer, state, action_probability, action, reward, terminal):
    """update!(buffer::BufferRollouts, ...) (src/rollout_buffer.jl:24-38) for user-driven collection."""
    if buffer._host is None:
        buffer._host = HostRollouts()
    generic.update_host_(buffer._host, state, action_probability, action, reward, terminal)


def compute_state_value_(rollouts, discount):
    """compute_state_value!(rollouts, discount) (src/rollout_buffer.jl:55-64), generic (host-collected) rollouts."""
    generic.compute_state_value_(_this_module(), rollouts._host, discount)


def collect_step_data_(buffer, env, policy, rng=None):
    """collect_step_data!(buffer, env, policy) (src/collect_rollouts.jl:1-15)."""
    if buffer._host is None:
        buffer._host = HostRollouts()
    generic.collect_step_data_(_this_module(), buffer._host, env, policy, rng or np.random.default_rng())


def collect_episode_data_(buffer, env, policy, rng=None):
    """collect_episode_data!(buffer, env, policy) (src/collect_rollouts.jl:17-24)."""
    if buffer._host is None:
        buffer._host = HostRollouts()
    generic.collect_episode_data_(_this_module(), buffer._host, env, policy, rng or np.random.default_rng())


def permute_(rollouts, idx):
    """permute!(rollouts, idx) (src/rollout_buffer.jl:81-88)."""
    generic.permute_(rollouts._host, idx)


def shuffle_(rollouts, rng=None):
    """shuffle!(rollouts) (src/rollout_buffer.jl:90-93)."""
    generic.shuffle_(rollouts._host, rng)


def single_trajectory_return(policy, env, rng=None):
    """single_trajectory_return(policy, env) (src/evaluate.jl:1-16)."""
    return generic.single_trajectory_return(_this_module(), policy, env, rng)


def smoothed_entropy(probs_AB, smooth=np.float32(1e-8)):
    """smoothed_entropy(probs, smooth) (src/train.jl:21-26) on probs [A,B] -> mean entropy (Float32 arithmetic)."""
    p = np.asarray(probs_AB, np.float32)
    sp = (np.float32(1.0) - np.float32(smooth)) * p + np.float32(smooth) / np.float32(p.shape[0])
    return float(np.mean(-np.sum(sp * np.log(sp), axis=0, dtype=np.float32), dtype=np.float32))


def clamped_entropy(probs_AB, clamp=np.float32(1e-8)):
    """clamped_entropy(probs, clamp) (src/train.jl:28-33; unused by the reference's training loop)."""
    p = np.clip(np.asarray(probs_AB, np.float32), np.float32(clamp), None)
    return float(np.mean(-np.sum(p * np.log(p), axis=0, dtype=np.float32), dtype=np.float32))


def ppo_loss(probs_AB, linear_action_index, old_action_probabilities, advantage, epsilon):
    """ppo_loss (src/train.jl:9-19): the clipped-surrogate term alone (ppo_loss_with_entropy without the entropy)."""
    return ppo_loss_with_entropy(probs_AB, linear_action_index, old_action_probabilities, advantage, epsilon)[0]


def step_epoch_(policy, optimizer, dataset, epsilon, batch_size, entropy_weight, perm=None, seed=0, advantage="returns"):
    """step_epoch!(policy, optimizer, dataset, epsilon, batch_size, entropy_weight) (src/train.jl:86-128):
    one pass over a fresh permutation; returns the unweighted means of the per-batch losses (:127)."""
    p, e, _ = ppo_train_(policy, optimizer, dataset, epsilon, batch_size, 1, entropy_weight,
                         perm=None if perm is None else np.asarray(perm)[None, :], seed=seed, verbose=False,
                         advantage=advantage)
    return p[0], e[0]
