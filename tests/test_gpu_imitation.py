"""Behaviour cloning on the device: the imitation train forward (k_policy_fwd modes 12 / 13, policy_tail mode 12),
the backwards imitate_route pairs it with, and the epoch loop, against the float64 restatement tests/imitation_ref.py.
TEST_RECORD_DIR=<dir>: measured figures go to <dir>/imitation.jsonl.

Bars.  Gradients and dL/dlogits: BAR = 2e-5 relative to the largest reference entry (tests/test_gpu_bench_shapes.py).  The
per-state loss terms and the two loss scalars: LOSS_BAR relative to max(1, largest reference entry).  LOSS_BAR is four times
the largest error of a plain numpy-float32 restatement (forward, log-softmax and entropy in float32: imitation_ref with
dtype=float32) against float64 over the cases of test 1 and 2, measured on a CPU: 1.24e-6 (the entropy terms of the
underflow cases, where logits near 200 carry a float32 ulp of 1.5e-5; 3.0e-7 over the cases of test 1), hence 5e-6.  The
device's own error is recorded beside it and was not used to set the bar."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import imitation_ref as ref
from test_imitation_host import NO_BF16_IMITATE, imitate_route

pytestmark = pytest.mark.gpu

BAR = 2e-5                                   # tests/test_gpu_bench_shapes.py: BAR, the bar of every fp32 gradient test
LOSS_BAR = 5e-6                              # see the module docstring
ETA = 1e-3
# (F, hidden, L): the headline, the 128 kernel, a zero-padded width, a deep policy; every one at H = 32 and H = 128, the wide
# rows at H = 32 (no kernel of the project takes F = 216 at H = 128)
SHAPE_H = [(F, hid, L, H) for (F, hid, L) in [(72, 256, 2), (72, 128, 2), (72, 192, 2), (72, 128, 3)] for H in (32, 128)] + [(216, 128, 2, 32)]
B1 = 21


@pytest.fixture(scope="module")
def P(ppo):
    if ppo.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests must run on the GPU box")
    return ppo


@pytest.fixture()
def knobs(P):
    yield P
    P.set_bwd_split_bf16(None)
    P.set_rollout_compact(None)
    P.set_train_tile_max_tiles(None)


def _record(rec):
    print(json.dumps(rec))
    d = os.environ.get("TEST_RECORD_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "imitation.jsonl"), "a") as f:
            f.write(json.dumps(rec) + "\n")


def _outputs(P, pol, B, H):
    """What the last train forward left: dL/dlogits [B, H, 4] and the loss terms [B, 2]."""
    L = P._lib.lib()
    L.ppo_debug_train_outputs.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.ppo_debug_train_outputs.restype = C.c_int32
    tiles = B * (H // 32)
    dy, lt = np.zeros((tiles, 32, 4), np.float32), np.zeros((tiles, 2), np.float64)
    assert L.ppo_debug_train_outputs(pol._h, tiles, dy.ctypes.data, lt.ctypes.data) == 0, P._lib.last_error()
    return dy.reshape(B, H, 4), lt[:B]                   # the loss terms are per state, the dL/dlogits rows per tile


def params_for(ppo, F, hid, L, rng):
    return (ppo.glorot_uniform_params(F, hid, L, 4, seed=5) + (rng.normal(size=ppo.glorot_uniform_params(F, hid, L, 4).size) * 0.03).astype(np.float32)).astype(np.float32)


def case1(ppo, F, hid, L, H, underflow=False):
    """The inputs of test 1 / 2 (no device needed).  Masks: all quads, only the first, only the last, random.  Given actions:
    on the first and on the last active row, at the arg-max, at the least likely action, and at H = 128 one in each of the
    four tiles (states 4 .. 7, all quads active).  Weights of both signs and zero.  underflow: b3 is shifted so that output 0 of
    every row lies at least 200 above every given action's logit (the given actions then avoid output 0)."""
    rng = np.random.default_rng(5000 + F + hid + L + H + int(underflow))
    Q = H // 4
    params = params_for(ppo, F, hid, L, rng)
    states = rng.integers(-3, 7, size=(B1, H, F)).astype(np.int8)
    active = rng.integers(1, 2 ** Q, size=B1, dtype=np.uint64).astype(np.uint32)
    active[0], active[1], active[2] = 2 ** Q - 1, 1, 1 << (Q - 1)
    active[4:8] = 2 ** Q - 1
    mask = ref.action_mask(active, H)
    logits = ref.logits_np(params, F, hid, L, states)
    lm = np.where(mask, logits, np.nan)
    if underflow:
        lm[:, 0::4] = np.nan                                          # output 0 is where the mass goes
    actions = np.zeros(B1, np.int64)
    for b in range(B1):
        ok = np.flatnonzero(~np.isnan(lm[b]))
        kind = b % 4 if not (H == 128 and 4 <= b < 8) else 4
        if kind == 0:
            actions[b] = ok[0]                                        # first active row
        elif kind == 1:
            actions[b] = ok[-1]                                       # last active row
        elif kind == 2:
            actions[b] = np.nanargmax(lm[b])
        elif kind == 3:
            actions[b] = np.nanargmin(lm[b])
        else:
            tile = ok[(ok // 128) == b - 4]
            actions[b] = tile[rng.integers(len(tile))]
    adv = rng.normal(size=B1).astype(np.float32)
    adv[0], adv[1], adv[2], adv[3] = 0.0, -1.5, 2.0, 0.75
    if underflow:
        la = logits[np.arange(B1), actions]
        shift = np.float32(200.0 + la.max() - logits[:, 0::4].min() + 1.0)
        p = params.copy()
        p[-4] += shift                                                # b3[0]
        params = p
        logits = ref.logits_np(params, F, hid, L, states)
        assert (np.where(mask, logits, np.inf)[:, 0::4].min(axis=1) - logits[np.arange(B1), actions] >= 200).all()
    assert mask[np.arange(B1), actions].all()
    return dict(params=params, states=states, active=active, actions=actions, adv=adv, logits=logits)


def loss_errors(c, F, hid, L, H, w, ew, dtype, logits=None, terms=None, Bg=None):
    """max error of the per-state terms and of the two scalars against float64, each relative to max(1, largest reference
    entry): of a restatement in `dtype`, or of given per-state `terms` [B, 2] summed in float64."""
    t0, t1 = ref.per_state_terms(c["logits"], c["active"], c["actions"], w, H)
    Bg = Bg or len(t0)
    ce, ent = -t0.sum() / Bg, ew * -t1.sum() / Bg
    if terms is None:
        lg = ref.logits_np(c["params"], F, hid, L, c["states"], dtype)
        g0, g1 = ref.per_state_terms(lg, c["active"], c["actions"], w, H, dtype)
        gce, gent = ref.losses_np(lg, c["active"], c["actions"], w, H, ew, Bg, dtype)
    else:
        g0, g1 = terms[:, 0], terms[:, 1]
        gce, gent = -g0.sum() / Bg, ew * -g1.sum() / Bg
    return dict(ce_terms=float(np.abs(g0 - t0).max() / max(1.0, np.abs(t0).max())),
                ent_terms=float(np.abs(g1 - t1).max() / max(1.0, np.abs(t1).max())),
                ce=float(abs(gce - ce) / max(1.0, abs(ce))), ent=float(abs(gent - ent) / max(1.0, abs(ent))))


def _buffer(P, states, active, actions0, returns, T=1):
    B, H, F = states.shape
    N = B // T
    ro = P.BufferRollouts()
    ro.set_columns(None, states.reshape(T, N, H, F), active.reshape(T, N), (actions0 + 1).reshape(T, N), np.ones((T, N), np.float32),
                   np.asarray(returns, np.float32).reshape(T, N), np.zeros((T, N), np.uint8))
    return ro


def _policy(P, F, hid, L, params):
    pol = P.HipPolicy(F, hid, L, 4, seed=1)
    pol.params = params
    return pol


def _check_outputs(P, pol, ds, c, F, hid, L, H, tag):
    """Both weight modes on one dataset: dY exactly 0 on inactive rows and within BAR of the analytic float64 dL/dlogits,
    loss terms and scalars within LOSS_BAR; B_global > B in the weighted run.  The entropy term is on in both."""
    B = len(c["actions"])
    on = ref.row_mask(c["active"], H)
    for weights, w, Bg, ew in (("uniform", np.ones(B, np.float32), B, 0.01), ("positive_advantage", c["adv"], 3 * B, 0.02)):
        ce, ent = P.imitate_forward_backward(pol, ds, np.arange(1, B + 1), ew, weights=weights, B_global=Bg)
        dy, lt = _outputs(P, pol, B, H)
        want = ref.analytic_dy(c["logits"], c["active"], c["actions"], w, H, ew, Bg)
        assert np.all(np.isfinite(dy)) and np.all(np.isfinite(lt)) and np.isfinite(ce) and np.isfinite(ent)
        assert not dy[~on].any(), "rows of inactive quads get exactly 0"
        err_dy = float(np.abs(dy - want).max() / np.abs(want).max())
        dev = loss_errors(c, F, hid, L, H, w, ew, None, terms=lt, Bg=Bg)
        f32 = loss_errors(c, F, hid, L, H, w, ew, np.float32, Bg=Bg)
        t0, t1 = ref.per_state_terms(c["logits"], c["active"], c["actions"], w, H)
        err_ce = abs(ce - -t0.sum() / Bg) / max(1.0, abs(t0.sum() / Bg))
        err_ent = abs(ent - ew * -t1.sum() / Bg) / max(1.0, abs(ew * t1.sum() / Bg))
        _record({"case": tag, "shape": [F, hid, L, H], "weights": weights, "B_global": Bg, "dy_err_over_max": err_dy,
                 "loss_err_device": dev, "loss_err_numpy_f32": f32, "ce_scalar_err": float(err_ce), "ent_scalar_err": float(err_ent),
                 "min_logp": float(ref.per_state_terms(c["logits"], c["active"], c["actions"], np.ones(B), H)[0].min())})
        assert err_dy <= BAR, (tag, weights, err_dy)
        assert max(dev.values()) <= LOSS_BAR, (tag, weights, dev)
        assert err_ce <= LOSS_BAR + 2.0 ** -23 and err_ent <= LOSS_BAR + 2.0 ** -23, "the scalars are stored as floats"
        if weights == "positive_advantage":
            assert (lt[c["adv"] <= 0, 0] == 0.0).all(), "weights at or below 0 clamp to 0"


# ---------------------------------------------------------------- 1. per-state outputs
@pytest.mark.parametrize("F,hid,L,H", SHAPE_H)
def test_per_state_outputs(P, F, hid, L, H):
    c = case1(P, F, hid, L, H)
    pol = _policy(P, F, hid, L, c["params"])
    hk = 128 if hid <= 128 else 256
    assert imitate_route(P, "f32", F, hk, L, H, False, B1)[0] == "k_policy_fwd<%d,%d,12,%d,%d>" % (F, hk, H // 32, int(L != 2))
    ds = P.construct_dataset(_buffer(P, c["states"], c["active"], c["actions"], c["adv"]))
    _check_outputs(P, pol, ds, c, F, hid, L, H, "outputs")
    if H == 128:                                         # the delta term of every tile is there
        dy, _ = _outputs(P, pol, B1, H)
        for b in range(4, 8):
            assert c["actions"][b] // 128 == b - 4


def _compact_case(P, F, hid, L, H, params):
    """Mode 13: a compact buffer collected on the device -- B1 fresh envs each play ONE given action (collect_paths_), chosen
    like case1's from the float64 logits of the env's reset state.  The weights are the buffer's own returns."""
    Q = H // 4
    env = P.HipVecEnv(num_envs=B1, Q=Q, max_actions=5, seed=77)
    it = env.internal()
    starts = (it["score"], it["degree"], env.active_quads())
    st0 = P.state(env)
    states = np.asarray(st0.vertex_score).reshape(B1, H, F)
    active = np.atleast_1d(st0.action_mask).astype(np.uint32)
    logits = ref.logits_np(params, F, hid, L, states)
    lm = np.where(ref.action_mask(active, H), logits, np.nan)
    rng = np.random.default_rng(H)
    actions = np.zeros(B1, np.int64)
    for b in range(B1):
        ok = np.flatnonzero(~np.isnan(lm[b]))
        if H == 128 and 4 <= b < 8 and len(ok[(ok // 128) == b - 4]):
            tile = ok[(ok // 128) == b - 4]
            actions[b] = tile[rng.integers(len(tile))]
        else:
            actions[b] = (ok[0], ok[-1], np.nanargmax(lm[b]), np.nanargmin(lm[b]))[b % 4]
    return env, starts, dict(params=params, states=states, active=active, actions=actions, logits=logits)


@pytest.mark.parametrize("hid,L,H", [(hid, L, H) for (F, hid, L, H) in SHAPE_H if F == 72])
def test_per_state_outputs_from_compact_buffers(knobs, hid, L, H):
    P = knobs
    F = 72
    params = params_for(P, F, hid, L, np.random.default_rng(hid + L + H))
    pol = _policy(P, F, hid, L, params)
    env, starts, c = _compact_case(P, F, hid, L, H, params)
    ro = P.BufferRollouts()
    P.set_rollout_compact(1)
    P.collect_paths_(ro, env, pol, *starts, (c["actions"] + 1).reshape(B1, 1).astype(np.int16), 1.0)
    P.set_rollout_compact(None)
    assert ro.dims() == (1, B1) and len(ro) == B1, "every given action lies on an active quad"
    st, act = ro.state_data
    assert np.array_equal(st.reshape(B1, H, F), c["states"]) and np.array_equal(act.reshape(-1), c["active"])
    assert np.array_equal(ro.selected_actions.reshape(-1) - 1, c["actions"])
    c["adv"] = ro.rewards.reshape(-1).astype(np.float32)
    hk = 128 if hid <= 128 else 256
    assert imitate_route(P, "f32", F, hk, L, H, True, B1)[0] == "k_policy_fwd<72,%d,13,%d,%d>" % (hk, H // 32, int(L != 2))
    ds = P.construct_dataset(ro)
    _check_outputs(P, pol, ds, c, F, hid, L, H, "outputs_compact")
    # ... and the rows mode 13 leaves the backward are mode 12's: the gradient of the expanded form of the same data, bit for bit
    P.imitate_forward_backward(pol, ds, np.arange(1, B1 + 1), 0.01)
    g13 = pol.grad()
    P.imitate_forward_backward(pol, P.construct_dataset(_buffer(P, c["states"], c["active"], c["actions"], c["adv"])), np.arange(1, B1 + 1), 0.01)
    assert g13.tobytes() == pol.grad().tobytes()


# ---------------------------------------------------------------- 2. the underflow case
@pytest.mark.parametrize("F,hid,L,H", [(72, 256, 2, 32), (72, 128, 2, 128), (72, 128, 3, 32)])
def test_underflow_case(P, F, hid, L, H):
    """exp(l[a] - m) underflows to 0 in float32 for every state: softmax gives p[a] = 0, log(p[a]) = -inf and a division by
    p[a] NaN; the log-softmax tail stays finite and within the bounds of test 1.  (forward_backward, the PPO pass, on the same
    buffer is not asserted.)"""
    c = case1(P, F, hid, L, H, underflow=True)
    assert np.exp(np.float32(-200.0)) == 0.0
    pol = _policy(P, F, hid, L, c["params"])
    ds = P.construct_dataset(_buffer(P, c["states"], c["active"], c["actions"], c["adv"]))
    _check_outputs(P, pol, ds, c, F, hid, L, H, "underflow")
    assert np.all(np.isfinite(pol.grad()))


# ---------------------------------------------------------------- 3. the full gradient
def _grad_case(P, F, hid, L, H, B, seed):
    """B random states off leakyrelu's kink, random masks, a uniformly drawn allowed action each, weights ~ N(0.5, 1)."""
    rng = np.random.default_rng(seed)
    params = params_for(P, F, hid, L, rng)
    parts, have = [], 0
    while have < B:
        cand = rng.integers(-3, 7, size=(B - have + B // 8 + 16, H, F)).astype(np.int8)
        cand = cand[ref.off_the_kink(params, F, hid, L, cand)]
        parts.append(cand)
        have += len(cand)
    states = np.ascontiguousarray(np.concatenate(parts)[:B])
    active = rng.integers(1, 2 ** (H // 4), size=B, dtype=np.uint64).astype(np.uint32)
    mask = ref.action_mask(active, H)
    actions = np.array([rng.choice(np.flatnonzero(m)) for m in mask])
    adv = (rng.normal(size=B) + 0.5).astype(np.float32)
    return params, states, active, actions, adv


GRAD_CASES = [  # (F, hid, L, H, B, split knob, backward)
    (72, 256, 2, 32, 48, 0, "k_policy_bwd_data<72,256>"),
    (72, 256, 2, 32, 400, None, "k_policy_bwd_x6<72,256>"),
    (72, 256, 2, 32, 400, 0, "k_policy_bwd<72,256>"),
    (72, 128, 3, 32, 48, None, "k_policy_bwd_data_deep<72,128>"),
    (72, 128, 2, 128, 30, None, "k_policy_bwd_x6<72,128>"),
]


@pytest.mark.parametrize("F,hid,L,H,B,split,bwd", GRAD_CASES)
def test_full_gradient_against_float64(knobs, F, hid, L, H, B, split, bwd):
    """max|g - g64| <= BAR max|g64| through every backward, uniform weights with B_global = B and weighted with
    B_global > B, the entropy term on in the second."""
    P = knobs
    params, states, active, actions, adv = _grad_case(P, F, hid, L, H, B, 300 + hid + L + H + B)
    pol = _policy(P, F, hid, L, params)
    ds = P.construct_dataset(_buffer(P, states, active, actions, adv))
    P.set_bwd_split_bf16(split)
    assert imitate_route(P, "f32", F, hid, L, H, False, B) == ("k_policy_fwd<%d,%d,12,%d,%d>" % (F, hid, H // 32, int(L != 2)), bwd)
    for weights, w, Bg, ew in (("uniform", np.ones(B), B, 0.0), ("positive_advantage", adv, 3 * B, 0.01)):
        ce, ent = P.imitate_forward_backward(pol, ds, np.arange(1, B + 1), ew, weights=weights, B_global=Bg)
        g = pol.grad()
        ce2, _ = P.imitate_forward_backward(pol, ds, np.arange(1, B + 1), ew, weights=weights, B_global=Bg)
        assert g.tobytes() == pol.grad().tobytes() and ce == ce2, "a second call repeats the first bit for bit"
        ce64, ent64, g64, _ = ref.loss_grad(params, F, hid, L, states, active, actions, w, ew, B_global=Bg)
        gmax, err = float(np.abs(g64).max()), float(np.abs(g - g64).max())
        _record({"case": "gradient", "shape": [F, hid, L, H], "B": B, "B_global": Bg, "weights": weights, "bwd": bwd, "max_abs_g64": gmax,
                 "err_over_max": err / gmax, "ce": ce, "ce64": ce64, "ent": ent, "ent64": ent64})
        assert gmax > 1e-4
        assert err <= BAR * gmax, (weights, err, gmax)
        assert abs(ce - ce64) <= (LOSS_BAR + 2.0 ** -23) * max(1.0, abs(ce64)) and abs(ent - ent64) <= (LOSS_BAR + 2.0 ** -23) * max(1.0, abs(ent64))
    assert np.array_equal(pol.params, params), "forward_backward does not touch the parameters"


# ---------------------------------------------------------------- 4. the epoch loop
def schedule_bars(p, p64, hist, h64, steps, eta=ETA):
    """The bars of a replayed Adam schedule.  (tests/test_gpu_value.py holds its schedule to conditions on the loss history
    alone; the parameters are held here too.)  History: 1e-5 (1 + |h64|), the bar of every loss-history comparison of the critic
    tests.  Parameters: Adam's step is eta m_hat / (sqrt(v_hat) + eps), m_hat and v_hat weighted means of g and g^2 with weights
    a_i ~ 0.9^(t-i), b_i ~ 0.999^(t-i); by Cauchy-Schwarz m_hat^2 / v_hat <= (sum a_i^2 / b_i)(sum b_i) / (sum a_i)^2, which is
    1.031 at t = 6 and less before, whatever the gradients -- so a step is at most 1.016 eta and two replicas of any precision
    differ by at most 2.04 eta steps, reached only in components whose gradient is smaller than its own error (the sign of the
    step is then free).  Components whose float64 gradient is well above the gradient bar move alike: the median difference is
    held to 1 % of one step."""
    d = np.abs(np.asarray(p, np.float64) - p64)
    out = dict(max_param_diff=float(d.max()), median_param_diff=float(np.median(d)),
               hist_err=float(np.max(np.abs(np.asarray(hist) - np.asarray(h64)) / (1 + np.abs(h64)))))
    ok = out["max_param_diff"] <= 2.04 * eta * steps and out["median_param_diff"] <= 0.01 * eta and out["hist_err"] <= 1e-5
    return ok, out


def test_epoch_loop_against_the_float64_schedule(P):
    """imitate_train_, 2 epochs of 3 minibatches (40, 40, 20) with given permutations, against imitation_ref.adam_schedule."""
    F, hid, L, H, B = 72, 128, 2, 32, 100
    params, states, active, actions, adv = _grad_case(P, F, hid, L, H, B, 4)
    pol = _policy(P, F, hid, L, params)
    ds = P.construct_dataset(_buffer(P, states, active, actions, adv))
    perms = np.stack([np.random.default_rng(40 + e).permutation(B) for e in range(2)])
    before = pol.last_train_stats()
    ch, eh, lh = P.imitate_train_(pol, P.Optimiser(P.Adam(ETA)), ds, 40, 2, perm=perms + 1, verbose=False)
    h64, p64 = ref.adam_schedule(params, F, hid, L, states, active, actions, np.ones(B), 40, perms, eta=ETA)
    ok, fig = schedule_bars(pol.params, p64, ch, h64, 6)
    _record({"case": "schedule", "device": ch, "float64": h64, **fig})
    assert len(ch) == len(eh) == len(lh) == 2 and lh == [ETA] * 2
    assert eh == [0.0, 0.0], "entropy_weight = 0: the entropy history is exactly 0"
    assert h64[-1] < h64[0], "the float64 restatement must satisfy the condition by itself"
    assert ch[-1] < ch[0]
    assert ok, fig
    after = pol.last_train_stats()
    assert after["epochs_run"] == before["epochs_run"] and after["stopped_early"] == before["stopped_early"]


# ---------------------------------------------------------------- 5. closure on the device
def test_search_collect_clone_collect(P):
    """search_best_states_(path=True) -> collect_paths_ -> imitate_train_ -> collect_paths_ with the same paths: the mean of
    log p_sel over the valid transitions rises (the policy moved towards the searched actions).  Q = 8, 64 starts, K = 8."""
    S, K, T = 64, 8, 12
    pol = P.HipPolicy(72, 128, 2, 4, seed=2)
    search_env = P.HipVecEnv(num_envs=S * K, Q=8, max_actions=T, seed=7)
    env = P.HipVecEnv(num_envs=S, Q=8, max_actions=T, seed=8)
    fresh = P.HipVecEnv(num_envs=S, Q=8, max_actions=T, seed=1000)
    it = fresh.internal()
    starts = (it["score"], it["degree"], fresh.active_quads())
    found = P.search_best_states_(search_env, pol, *starts, K, path=True)
    ro = P.BufferRollouts()
    P.collect_paths_(ro, env, pol, *starts, found["path"], 1.0)
    n = len(ro)
    assert n >= 32, "the search must find something to imitate"
    valid = ro.valid.astype(bool)
    lp0 = float(np.log(ro.selected_action_probabilities[valid].astype(np.float64)).mean())
    ch, _, _ = P.imitate_train_(pol, P.Optimiser(P.Adam(ETA)), P.construct_dataset(ro), min(64, n), 4, seed=3, verbose=False)
    P.collect_paths_(ro, env, pol, *starts, found["path"], 1.0)
    assert np.array_equal(ro.valid.astype(bool), valid)
    lp1 = float(np.log(ro.selected_action_probabilities[valid].astype(np.float64)).mean())
    _record({"case": "closure", "transitions": n, "mean_log_p_before": lp0, "mean_log_p_after": lp1, "ce_history": ch})
    assert lp1 > lp0 and ch[-1] < ch[0]


# ---------------------------------------------------------------- 6. the weighted form
def test_weighted_form_with_gae_from_the_critic(P):
    """positive_advantage with "gae" after compute_gae_critic_(lam = 1, bootstrap_truncated=True): the gradient meets the bar with
    w = max(adv, 0) taken from the column that call returned; weights that are all 0 give an exactly zero gradient."""
    F, hid, L = 72, 128, 2
    env = P.HipVecEnv(num_envs=48, Q=8, max_actions=6, seed=31)
    # an env's all-zero rows have z1 = b1: seed 9 keeps every hidden bias 6e-4 or more from leakyrelu's kink (seed 6: one at 2e-6,
    # and 372 of the 384 states fail off_the_kink)
    pol = _policy(P, F, hid, L, params_for(P, F, hid, L, np.random.default_rng(9)))
    assert min(np.abs(b).min() for _, b in ref.unpack(pol.params, F, hid, L)[:-1]) > 5e-4
    critic = P.HipCritic(F, hid, L, seed=4)
    ro = P.BufferRollouts()
    P.set_rollout_compact(0)
    P.collect_rollouts_steps_(ro, env, pol, 8, 0.99)
    P.set_rollout_compact(None)
    adv, _ = P.compute_gae_critic_(ro, env, critic, 0.99, 1.0, bootstrap_truncated=True)
    st, act = ro.state_data
    states, active = st.reshape(-1, 32, F), act.reshape(-1)
    actions, w = ro.selected_actions.reshape(-1) - 1, adv.reshape(-1)
    params = pol.params
    sel = np.flatnonzero(ref.off_the_kink(params, F, hid, L, states))
    assert len(sel) >= 64 and (w[sel] > 0).any() and (w[sel] < 0).any(), "weights of both signs"
    ds = P.construct_dataset(ro)
    assert np.array_equal(ro.index(), np.arange(len(ds))), "storage order is dataset order here"
    P.imitate_forward_backward(pol, ds, sel + 1, weights="positive_advantage", advantage="gae")
    g = pol.grad()
    _, _, g64, _ = ref.loss_grad(params, F, hid, L, states[sel], active[sel], actions[sel], w[sel])
    gmax, err = float(np.abs(g64).max()), float(np.abs(g - g64).max())
    _record({"case": "weighted_gae", "B": int(len(sel)), "n_truncated": int(ro.n_truncated), "positive": int((w[sel] > 0).sum()), "max_abs_g64": gmax, "err_over_max": err / gmax})
    assert gmax > 1e-4 and err <= BAR * gmax
    # all weights 0: returns at or below 0 in the column "returns" names
    B = 40
    params, states, active, actions, _ = _grad_case(P, F, hid, L, 32, B, 66)
    pol0 = _policy(P, F, hid, L, params)
    ret = -np.abs(np.random.default_rng(1).normal(size=B)).astype(np.float32)
    ret[::5] = 0.0
    ds0 = P.construct_dataset(_buffer(P, states, active, actions, ret))
    ce, ent = P.imitate_forward_backward(pol0, ds0, np.arange(1, B + 1), weights="positive_advantage", advantage="returns")
    assert not pol0.grad().any() and ce == 0.0 and ent == 0.0
    ce, _ = P.imitate_forward_backward(pol0, ds0, np.arange(1, B + 1))
    assert pol0.grad().any() and ce > 0.0


# ---------------------------------------------------------------- 7. refusals
def test_refusals(knobs):
    P = knobs
    env = P.HipVecEnv(num_envs=8, Q=8, max_actions=5, seed=1)
    pol = P.HipPolicy(72, 128, 2, 4, seed=1)
    ro = P.BufferRollouts()
    P.set_rollout_compact(1)
    P.collect_rollouts_steps_(ro, env, pol, 6, 1.0)
    P.set_rollout_compact(None)
    ds = P.construct_dataset(ro)
    idx = np.arange(1, 9)

    def both(policy, **kw):
        return (lambda: P.imitate_forward_backward(policy, ds, idx, **kw),
                lambda: P.imitate_train_(policy, P.Optimiser(P.Adam()), ds, 8, 1, verbose=False, **kw))

    bf = P.HipPolicy(72, 128, 2, 4, seed=1, dtype="bf16")
    for call in both(bf):
        with pytest.raises(P.PPOError, match=NO_BF16_IMITATE) as e:
            call()
        assert e.value.status == -4
    for call in both(pol, weights="positive_advantage", advantage="gae"):
        with pytest.raises(P.PPOError, match="needs ppo_rollouts_compute_gae on these rollouts first") as e:
            call()
        assert e.value.status == -1
    for call in both(pol, advantage="gae_normalised") + both(pol, weights="positive_advantage", advantage="returns_normalised") + both(pol, weights="exp"):
        with pytest.raises(P.PPOError) as e:
            call()
        assert e.value.status == -4
    L = P._lib.lib()                                     # ... and at the C ABI, past the mirror's own check
    i0 = np.zeros(1, np.int64)
    for wm, am, text in ((0, 1, "normalised advantage modes are not supported"), (1, 3, "normalised advantage modes are not supported"),
                         (2, 0, "unknown weight mode"), (0, 9, "unknown advantage mode")):
        assert L.ppo_imitate_forward_backward(pol._h, ro._h, i0.ctypes.data_as(P._lib.c_i64p), 1, 1, 0.0, wm, am) == -4
        assert text in P._lib.last_error()
    # F = 216 with a compact buffer: the buffer is the built-in env's (F = 72), so the entry points' own shape check refuses the
    # pair (PPO_ERR_ARG, as ppo_forward_backward does); the route refuses the shape itself (PPO_ERR_UNSUPPORTED)
    wide = P.HipPolicy(216, 128, 2, 4, seed=1)
    for call in both(wide):
        with pytest.raises(P.PPOError, match="shape mismatch") as e:
            call()
        assert e.value.status == -1
    assert imitate_route(P, "f32", 216, 128, 2, 32, True, 8) == ("none", "compact rollouts need the built-in env's F = 72")
    # a GAE call later, the weighted form runs
    P.compute_gae_critic_(ro, env, P.HipCritic(72, 128, 2, seed=3), 0.99, 1.0, fetch=False)
    ce, _ = P.imitate_forward_backward(pol, ds, idx, weights="positive_advantage", advantage="gae")
    assert np.isfinite(ce)


# ---------------------------------------------------------------- 8. nothing else moved
def test_other_objectives_and_statistics_unchanged(P):
    F, hid, L, H, B = 72, 128, 2, 32, 64
    params, states, active, actions, adv = _grad_case(P, F, hid, L, H, B, 8)
    pol = _policy(P, F, hid, L, params)
    critic = P.HipCritic(F, hid, L, seed=4)
    ro = _buffer(P, states, active, actions, adv)
    ds = P.construct_dataset(ro)
    idx = np.arange(1, B + 1)
    pol.target_kl = float("inf")
    P.ppo_train_(pol, P.Optimiser(P.Adam(1e-4)), ds, 0.05, 32, 2, 0.01, seed=1, verbose=False)
    stats = pol.last_train_stats()
    assert stats["epochs_run"] == 2 and np.all(np.isfinite(stats["approx_kl"]))

    def others():
        l = P.forward_backward(pol, ds, idx, 0.05, 0.01)
        g = pol.grad().tobytes()
        v = P.value_forward_backward(critic, ds, idx)
        return l, g, v, critic.grad().tobytes()

    before = others()
    P.imitate_forward_backward(pol, ds, idx, 0.01)
    P.imitate_forward_backward(critic, ds, idx, 0.01, weights="positive_advantage")
    assert others() == before
    p0 = pol.params
    P.imitate_train_(pol, P.Optimiser(P.Adam(1e-4)), ds, 32, 3, 0.01, seed=2, verbose=False)
    assert not np.array_equal(pol.params, p0)
    after = pol.last_train_stats()
    assert after["epochs_run"] == 2 and after["stopped_early"] == stats["stopped_early"]
    for k in ("approx_kl", "old_approx_kl", "clip_fraction"):
        assert np.array_equal(after[k], stats[k]), k
