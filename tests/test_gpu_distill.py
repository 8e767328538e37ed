"""Policy distillation on the device: the target column and its fill (k_policy_fwd modes 0 / 19), the distillation
train forward (modes 17 / 18, policy_tail's Distill branch), the backwards distill_route pairs it with, and the epoch loop, against
the float64 restatement tests/distill_ref.py.  TEST_RECORD_DIR=<dir>: measured figures go to <dir>/distill.jsonl.

Bars.  Gradients and dL/dlogits: BAR = 2e-5 relative to the largest reference entry (tests/test_gpu_bench_shapes.py).  The
per-state loss terms and the two loss scalars: LOSS_BAR relative to max(1, largest reference entry).  LOSS_BAR is four times the
largest error of a plain numpy-float32 restatement (forward, log-softmax, the sum over up to 512 products q logp and the entropy
in float32: distill_ref with dtype=float32) against float64 over the cases of test 2 -- every shape of SHAPE_H with the "kinds"
and the "teacher" targets (the teacher's probabilities restated in numpy float32 for this measurement) and the three underflow
cases, both weight modes -- measured on a CPU by measure_loss_bar() below: 1.24e-6 (the entropy terms of the underflow cases,
where logits near 200 carry a float32 ulp of 1.5e-5; 2.96e-7 over the other cases; the cross-entropy terms, sums of up to 512
products, 2.66e-7 at the most), and 4 x 1.24e-6 = 4.96e-6 rounds up to 5e-6.  The device's own error is recorded beside it and
was not used to set the bar."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import distill_ref as ref
from test_distill_host import NO_BF16_STUDENT, distill_route, target_kinds
from test_gpu_imitation import (B1, BAR, ETA, GRAD_CASES, SHAPE_H, _buffer, _grad_case, _outputs, _policy, case1, params_for,
                                schedule_bars)

pytestmark = pytest.mark.gpu

LOSS_BAR = 5e-6                              # see the module docstring
UNDERFLOW_SHAPES = [(72, 256, 2, 32), (72, 128, 2, 128), (72, 128, 3, 32)]
WEIGHT_RUNS = (("uniform", None, 1, 0.01), ("positive_advantage", "adv", 3, 0.02))    # (weights, column, B_global / B, entropy_weight)


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
        with open(os.path.join(d, "distill.jsonl"), "a") as f:
            f.write(json.dumps(rec) + "\n")


# ---------------------------------------------------------------- the cases of test 2 (no device needed)
def teacher_shape(F, hid):
    """A teacher of another width than the student's kernel width, same F."""
    return (F, 128 if hid > 128 else 256, 2)


def teacher_probs_np(ppo, F, hid, H, states, active):
    """The teacher's probabilities restated in numpy float32 (what fill_targets_ writes up to float32 rounding)."""
    tF, thid, tL = teacher_shape(F, hid)
    tp = params_for(ppo, tF, thid, tL, np.random.default_rng(77))
    _, p = ref.log_probs_np(ref.logits_np(tp, tF, thid, tL, states, np.float32), ref.action_mask(active, H), np.float32)
    return tp, p.astype(np.float32)


def kinds_targets(c, H):
    """One target row per state of case1: by b % 5 a dense row over ALL actions (mass on inactive rows wherever a quad is
    inactive), one-hot on case1's action, half the mass on an inactive quad, a row summing to 0.5, an all-zero row; at H = 128
    states 4 .. 7 (all quads active) hold their whole mass in tile b - 4."""
    rng = np.random.default_rng(900 + H)
    q = target_kinds(rng, c["active"], H)
    B = len(c["active"])
    for b in range(1, B, 5):
        q[b] = 0
        q[b, c["actions"][b]] = 1.0
    if H == 128:
        for b in range(4, 8):
            e = rng.random(128).astype(np.float32)
            q[b] = 0
            q[b, 128 * (b - 4):128 * (b - 3)] = e / e.sum()
    return q


def underflow_targets(c, H):
    """case1(underflow=True): output 0 of every row lies 200 above the given action's logit.  Half of every state's mass on the
    given action, half spread over the other allowed actions of outputs 1 .. 3: float32 exp(l - m) is 0 on all of them."""
    mask = ref.action_mask(c["active"], H)
    mask[:, 0::4] = False
    B = len(c["active"])
    q = np.zeros(mask.shape, np.float32)
    for b in range(B):
        ok = np.flatnonzero(mask[b])
        q[b, ok] = np.float32(0.5 / len(ok))
        q[b, c["actions"][b]] += np.float32(0.5)
    lm = np.where(ref.action_mask(c["active"], H), c["logits"], -np.inf)
    gap = (lm.max(axis=1, keepdims=True) - c["logits"]).astype(np.float32)
    with np.errstate(under="ignore"):
        assert (np.exp(-gap[q > 0], dtype=np.float32) == 0.0).all(), "the student gives every target action exp = 0"
    return q


def loss_errors(c, q, F, hid, L, H, w, ew, dtype, terms=None, Bg=None):
    """max error of the per-state terms and of the two scalars against float64, each relative to max(1, largest reference
    entry): of a restatement in `dtype`, or of given per-state `terms` [B, 2] summed in float64."""
    t0, t1 = ref.per_state_terms(c["logits"], c["active"], q, w, H)
    Bg = Bg or len(t0)
    ce, ent = -t0.sum() / Bg, ew * -t1.sum() / Bg
    if terms is None:
        lg = ref.logits_np(c["params"], F, hid, L, c["states"], dtype)
        g0, g1 = ref.per_state_terms(lg, c["active"], q, w, H, dtype)
        gce, gent = ref.losses_np(lg, c["active"], q, w, H, ew, Bg, dtype)
    else:
        g0, g1 = terms[:, 0], terms[:, 1]
        gce, gent = -g0.sum() / Bg, ew * -g1.sum() / Bg
    return dict(ce_terms=float(np.abs(g0 - t0).max() / max(1.0, np.abs(t0).max())),
                ent_terms=float(np.abs(g1 - t1).max() / max(1.0, np.abs(t1).max())),
                ce=float(abs(gce - ce) / max(1.0, abs(ce))), ent=float(abs(gent - ent) / max(1.0, abs(ent))))


def _weights(c, col):
    return np.ones(len(c["active"]), np.float32) if col is None else c[col]


def measure_loss_bar(ppo):
    """The figure LOSS_BAR rests on (CPU only): the largest float32-restatement error over the cases of test 2, and the same
    split into the underflow cases and the others."""
    worst = {"underflow": {}, "others": {}}
    for group, shapes in (("others", SHAPE_H), ("underflow", UNDERFLOW_SHAPES)):
        for (F, hid, L, H) in shapes:
            c = case1(ppo, F, hid, L, H, underflow=group == "underflow")
            if group == "underflow":
                qs = [underflow_targets(c, H)]
            else:
                qs = [kinds_targets(c, H), teacher_probs_np(ppo, F, hid, H, c["states"], c["active"])[1]]
            for q in qs:
                for _, col, k, ew in WEIGHT_RUNS:
                    e = loss_errors(c, q, F, hid, L, H, _weights(c, col), ew, np.float32, Bg=k * B1)
                    for key, v in e.items():
                        worst[group][key] = max(worst[group].get(key, 0.0), v)
    return worst


def _check_outputs(P, pol, ds, c, q, F, hid, L, H, tag):
    """Both weight modes on one dataset: dY exactly 0 on inactive rows and within BAR of the analytic float64 dL/dlogits, loss
    terms and scalars within LOSS_BAR; B_global > B in the weighted run.  The entropy term is on in both."""
    B = len(c["active"])
    on = ref.row_mask(c["active"], H)
    for weights, col, k, ew in WEIGHT_RUNS:
        w, Bg = _weights(c, col), k * B
        ce, ent = P.distill_forward_backward(pol, ds, np.arange(1, B + 1), ew, weights=weights, B_global=Bg)
        dy, lt = _outputs(P, pol, B, H)
        want = ref.analytic_dy(c["logits"], c["active"], q, w, H, ew, Bg)
        assert np.all(np.isfinite(dy)) and np.all(np.isfinite(lt)) and np.isfinite(ce) and np.isfinite(ent)
        err_dy = float(np.abs(dy - want).max() / np.abs(want).max())
        dev = loss_errors(c, q, F, hid, L, H, w, ew, None, terms=lt, Bg=Bg)
        f32 = loss_errors(c, q, F, hid, L, H, w, ew, np.float32, Bg=Bg)
        t0, t1 = ref.per_state_terms(c["logits"], c["active"], q, w, H)
        err_ce = abs(ce - -t0.sum() / Bg) / max(1.0, abs(t0.sum() / Bg))
        err_ent = abs(ent - ew * -t1.sum() / Bg) / max(1.0, abs(ew * t1.sum() / Bg))
        _record({"case": tag, "shape": [F, hid, L, H], "weights": weights, "B_global": Bg, "dy_err_over_max": err_dy,
                 "loss_err_device": dev, "loss_err_numpy_f32": f32, "ce_scalar_err": float(err_ce), "ent_scalar_err": float(err_ent)})
        assert not dy[~on].any(), "rows of inactive quads get exactly 0"
        assert err_dy <= BAR, (tag, weights, err_dy)
        assert max(dev.values()) <= LOSS_BAR, (tag, weights, dev)
        assert err_ce <= LOSS_BAR + 2.0 ** -23 and err_ent <= LOSS_BAR + 2.0 ** -23, "the scalars are stored as floats"
        if weights == "positive_advantage":
            assert (lt[c["adv"] <= 0, 0] == 0.0).all(), "weights at or below 0 clamp to 0"


def _dataset(P, c, q=None):
    B, H, _ = c["states"].shape
    ro = _buffer(P, c["states"], c["active"], c["actions"], c["adv"])
    if q is not None:
        ro.set_action_targets(q.reshape(1, B, 4 * H))
    return ro, P.construct_dataset(ro)


def _collect(P, pol, N, T, Q, compact, seed, record_probs=False, max_actions=6):
    env = P.HipVecEnv(num_envs=N, Q=Q, max_actions=max_actions, seed=seed)
    ro = P.BufferRollouts()
    P.set_rollout_compact(int(compact))
    P.collect_rollouts_steps_(ro, env, pol, T, 0.99, record_probs=record_probs)
    P.set_rollout_compact(None)
    return env, ro


# ---------------------------------------------------------------- 1. the fill
FILL_TEACHERS = [(72, 256, 2, "f32"), (72, 128, 3, "f32"), (72, 256, 2, "bf16")]


@pytest.mark.parametrize("Q", [8, 32])
@pytest.mark.parametrize("F,hid,L,dtype", FILL_TEACHERS)
def test_fill_is_the_probabilities_forward(knobs, orc, F, hid, L, dtype, Q):
    """Expanded storage: the column is ppo_policy_forward(teacher, states) bit for bit, and (fp32 teachers) the device-order
    oracle's action_probabilities bit for bit.  Compact storage (fp32 teachers): mode 19 on the same collection gives the
    expanded fill bit for bit.  72 / 12 states: more than one workgroup at Q = 8."""
    P = knobs
    H = 4 * Q
    N, T = (24, 3) if Q == 8 else (6, 2)
    teacher = P.HipPolicy(F, hid, L, 4, seed=11, dtype=dtype)
    teacher.params = params_for(P, F, hid, L, np.random.default_rng(11))
    actor = P.HipPolicy(72, 128, 2, 4, seed=2)
    _, ro = _collect(P, actor, N, T, Q, False, 21)
    st, act = ro.state_data
    states, active = st.reshape(-1, H, F), act.reshape(-1)
    P.fill_targets_(ro, teacher)
    col = ro.action_targets
    assert col.shape == (T, N, 4 * H) and col.dtype == np.float32
    fwd = P._forward(teacher, states, active)
    assert col.reshape(-1, 4 * H).tobytes() == fwd.tobytes(), "the fill is the probabilities forward"
    assert np.all(col.reshape(-1, 4 * H)[~ref.action_mask(active, H)] == 0.0) and abs(float(col.sum(dtype=np.float64)) - T * N) < 1e-2
    if dtype == "f32":
        want = np.stack([orc.action_probabilities(teacher.params, F, hid, states[b], int(active[b]), mode="dev", n_hidden=L)
                         for b in range(len(states))])
        assert col.reshape(-1, 4 * H).tobytes() == want.astype(np.float32).tobytes(), "... and the device-order oracle's word"
        _, roc = _collect(P, actor, N, T, Q, True, 21)
        stc, actc = roc.state_data
        assert np.array_equal(stc, st) and np.array_equal(actc, act), "the same collection in the other storage form"
        P.fill_targets_(roc, teacher)
        assert roc.action_targets.tobytes() == col.tobytes(), "mode 19 from snapshots is mode 0 from rows"
    # the getter returns what the uploader took
    q = np.random.default_rng(1).random(col.shape).astype(np.float32)
    ro.set_action_targets(q)
    assert np.array_equal(ro.action_targets, q)


# ---------------------------------------------------------------- 2. per-state outputs
@pytest.mark.parametrize("F,hid,L,H", SHAPE_H)
def test_per_state_outputs(P, F, hid, L, H):
    """dY and the loss terms for every kind of target row, and for rows a teacher of another width filled on the device."""
    c = case1(P, F, hid, L, H)
    pol = _policy(P, F, hid, L, c["params"])
    hk = 128 if hid <= 128 else 256
    assert distill_route(P, "f32", F, hk, L, H, False, B1)[0] == "k_policy_fwd<%d,%d,17,%d,%d>" % (F, hk, H // 32, int(L != 2))
    q = kinds_targets(c, H)
    ro, ds = _dataset(P, c, q)
    _check_outputs(P, pol, ds, c, q, F, hid, L, H, "outputs_kinds")
    tF, thid, tL = teacher_shape(F, hid)
    tp, _ = teacher_probs_np(P, F, hid, H, c["states"], c["active"])
    teacher = _policy(P, tF, thid, tL, tp)
    P.fill_targets_(ro, teacher)
    qt = ro.action_targets.reshape(B1, 4 * H)
    assert qt.tobytes() == P._forward(teacher, c["states"], c["active"]).tobytes()
    _check_outputs(P, pol, ds, c, qt, F, hid, L, H, "outputs_teacher")


@pytest.mark.parametrize("hid,L,H", [(hid, L, H) for (F, hid, L, H) in SHAPE_H if F == 72])
def test_per_state_outputs_from_compact_buffers(knobs, hid, L, H):
    """Mode 18: a compact buffer collected on the device, its targets filled from snapshots by a teacher of another width
    (mode 19); the weights are the buffer's own returns.  The rows mode 18 leaves the backward are mode 17's: the gradient of
    the expanded form of the same data, bit for bit."""
    P = knobs
    F, Q = 72, H // 4
    params = params_for(P, F, hid, L, np.random.default_rng(hid + L + H))
    pol = _policy(P, F, hid, L, params)
    _, ro = _collect(P, pol, B1, 1, Q, True, 77)
    st, act = ro.state_data
    c = dict(params=params, states=st.reshape(B1, H, F), active=act.reshape(-1), adv=ro.rewards.reshape(-1).astype(np.float32),
             actions=ro.selected_actions.reshape(-1) - 1)
    c["logits"] = ref.logits_np(params, F, hid, L, c["states"])
    tF, thid, tL = teacher_shape(F, hid)
    teacher = _policy(P, tF, thid, tL, params_for(P, tF, thid, tL, np.random.default_rng(78)))
    P.fill_targets_(ro, teacher)
    q = ro.action_targets.reshape(B1, 4 * H)
    assert q.tobytes() == P._forward(teacher, c["states"], c["active"]).tobytes()
    hk = 128 if hid <= 128 else 256
    assert distill_route(P, "f32", F, hk, L, H, True, B1)[0] == "k_policy_fwd<72,%d,18,%d,%d>" % (hk, H // 32, int(L != 2))
    ds = P.construct_dataset(ro)
    _check_outputs(P, pol, ds, c, q, F, hid, L, H, "outputs_compact")
    P.distill_forward_backward(pol, ds, np.arange(1, B1 + 1), 0.01)
    g18 = pol.grad()
    _, dse = _dataset(P, c, q)
    P.distill_forward_backward(pol, dse, np.arange(1, B1 + 1), 0.01)
    assert g18.tobytes() == pol.grad().tobytes()


@pytest.mark.parametrize("F,hid,L,H", UNDERFLOW_SHAPES)
def test_underflow_case(P, F, hid, L, H):
    """The whole target mass where the student's exp(l - m) is 0 in float32: softmax gives p = 0 there, log(p) = -inf and a
    division by p NaN; the log-softmax tail stays finite and within the bounds of test 2."""
    c = case1(P, F, hid, L, H, underflow=True)
    q = underflow_targets(c, H)
    pol = _policy(P, F, hid, L, c["params"])
    _, ds = _dataset(P, c, q)
    _check_outputs(P, pol, ds, c, q, F, hid, L, H, "underflow")
    assert np.all(np.isfinite(pol.grad()))


# ---------------------------------------------------------------- 3. one-hot targets are behaviour cloning
@pytest.mark.parametrize("F,hid,L,H", [(72, 256, 2, 32), (72, 128, 2, 128), (72, 128, 3, 32), (216, 128, 2, 32)])
def test_one_hot_targets_equal_cloning(P, F, hid, L, H):
    c = case1(P, F, hid, L, H)
    q = np.zeros((B1, 4 * H), np.float32)
    q[np.arange(B1), c["actions"]] = 1.0
    pol = _policy(P, F, hid, L, c["params"])
    _, ds = _dataset(P, c, q)
    idx = np.arange(1, B1 + 1)
    for weights, col, k, ew in WEIGHT_RUNS:
        ld = P.distill_forward_backward(pol, ds, idx, ew, weights=weights, B_global=k * B1)
        dyd, ltd = _outputs(P, pol, B1, H)
        gd = pol.grad()
        li = P.imitate_forward_backward(pol, ds, idx, ew, weights=weights, B_global=k * B1)
        dyi, lti = _outputs(P, pol, B1, H)
        gi = pol.grad()
        bitwise = dyd.tobytes() == dyi.tobytes() and ltd.tobytes() == lti.tobytes() and gd.tobytes() == gi.tobytes() and ld == li
        _record({"case": "one_hot", "shape": [F, hid, L, H], "weights": weights, "bitwise_equal": bool(bitwise),
                 "dy_diff_over_max": float(np.abs(dyd - dyi).max() / np.abs(dyi).max()),
                 "grad_diff_over_max": float(np.abs(gd - gi).max() / np.abs(gi).max())})
        assert np.abs(dyd - dyi).max() <= 1e-6 * np.abs(dyi).max()
        assert np.abs(ltd - lti).max() <= 1e-6 * np.abs(lti).max()
        assert np.abs(gd - gi).max() <= 1e-6 * np.abs(gi).max()
        assert abs(ld[0] - li[0]) <= 1e-6 * max(1.0, abs(li[0])) and abs(ld[1] - li[1]) <= 1e-6 * max(1.0, abs(li[1]))


# ---------------------------------------------------------------- 4. self-distillation
@pytest.mark.parametrize("F,hid,L,H", [(72, 128, 2, 32), (72, 256, 2, 128), (72, 128, 3, 32)])
def test_self_distillation_has_no_gradient(P, F, hid, L, H):
    """Teacher = a copy of the student, uniform weights, no entropy term: the tail forms the softmax the probabilities forward
    formed, so p Qs - q has q == p and Qs within a few ulp of 1: every |dY| <= 8 * 2^-24 / B_global.  The loss is the entropy
    of the targets."""
    c = case1(P, F, hid, L, H)
    pol = _policy(P, F, hid, L, c["params"])
    teacher = _policy(P, F, hid, L, c["params"])
    ro, ds = _dataset(P, c)
    P.fill_targets_(ro, teacher)
    q = ro.action_targets.reshape(B1, 4 * H)
    Bg = 2 * B1
    ce, ent = P.distill_forward_backward(pol, ds, np.arange(1, B1 + 1), 0.0, B_global=Bg)
    dy, lt = _outputs(P, pol, B1, H)
    floor = ref.target_entropy(q, c["active"], np.ones(B1), H, B_global=Bg)
    _record({"case": "self", "shape": [F, hid, L, H], "max_abs_dy_times_Bg_over_ulp": float(np.abs(dy).max() * Bg / 2.0 ** -24),
             "ce": ce, "targets_entropy": floor})
    assert np.abs(dy).max() <= 8 * 2.0 ** -24 / Bg
    assert ent == 0.0 and abs(ce - floor) <= (LOSS_BAR + 2.0 ** -23) * max(1.0, floor)
    h = -np.where(q > 0, q.astype(np.float64) * np.log(np.where(q > 0, q, 1).astype(np.float64)), 0).sum(axis=1)
    assert np.abs(-lt[:, 0] - h).max() <= LOSS_BAR * max(1.0, h.max())


# ---------------------------------------------------------------- 5. the full gradient
def _dense_targets(rng, active, H):
    """Rows of every kind but one-hot-only: dense over all actions (some mass on inactive rows), unnormalised, a few all-zero."""
    q = target_kinds(rng, active, H)
    q[5::7] *= np.float32(1.5)
    return q


@pytest.mark.parametrize("F,hid,L,H,B,split,bwd", GRAD_CASES)
def test_full_gradient_against_float64(knobs, F, hid, L, H, B, split, bwd):
    """max|g - g64| <= BAR max|g64| through every backward from expanded storage, uniform weights with B_global = B and
    weighted with B_global > B (entropy term on); a second call repeats the first bit for bit."""
    P = knobs
    params, states, active, actions, adv = _grad_case(P, F, hid, L, H, B, 300 + hid + L + H + B)
    q = _dense_targets(np.random.default_rng(B + H), active, H)
    pol = _policy(P, F, hid, L, params)
    _, ds = _dataset(P, dict(states=states, active=active, actions=actions, adv=adv), q)
    P.set_bwd_split_bf16(split)
    assert distill_route(P, "f32", F, hid, L, H, False, B) == ("k_policy_fwd<%d,%d,17,%d,%d>" % (F, hid, H // 32, int(L != 2)), bwd)
    for weights, w, Bg, ew in (("uniform", np.ones(B), B, 0.0), ("positive_advantage", adv, 3 * B, 0.01)):
        ce, ent = P.distill_forward_backward(pol, ds, np.arange(1, B + 1), ew, weights=weights, B_global=Bg)
        g = pol.grad()
        ce2, _ = P.distill_forward_backward(pol, ds, np.arange(1, B + 1), ew, weights=weights, B_global=Bg)
        assert np.array_equal(g, pol.grad()) and g.tobytes() == pol.grad().tobytes() and ce == ce2, "a second call repeats the first bit for bit"
        ce64, ent64, g64 = ref.loss_grad(params, F, hid, L, states, active, q, w, ew, B_global=Bg)
        gmax, err = float(np.abs(g64).max()), float(np.abs(g - g64).max())
        _record({"case": "gradient", "shape": [F, hid, L, H], "B": B, "B_global": Bg, "weights": weights, "bwd": bwd, "max_abs_g64": gmax,
                 "err_over_max": err / gmax, "ce": ce, "ce64": ce64, "ent": ent, "ent64": ent64})
        assert gmax > 1e-5
        assert err <= BAR * gmax, (weights, err, gmax)
        assert abs(ce - ce64) <= (LOSS_BAR + 2.0 ** -23) * max(1.0, abs(ce64)) and abs(ent - ent64) <= (LOSS_BAR + 2.0 ** -23) * max(1.0, abs(ent64))
    assert np.array_equal(pol.params, params), "forward_backward does not touch the parameters"


def _kink_free_student(P):
    """Policy(72,128,2,4) whose hidden biases stay clear of leakyrelu's kink on an env's all-zero rows (tests/test_gpu_imitation.py,
    test 6: seed 9)."""
    params = params_for(P, 72, 128, 2, np.random.default_rng(9))
    assert min(np.abs(b).min() for _, b in ref.unpack(params, 72, 128, 2)[:-1]) > 5e-4
    return params, _policy(P, 72, 128, 2, params)


@pytest.mark.parametrize("split,bwd", [(None, "k_policy_bwd_x6<72,128>"), (0, "k_policy_bwd_data<72,128>")])
def test_full_gradient_from_compact_storage(knobs, split, bwd):
    """The same bar from a compact buffer collected on the device (mode 18), the targets filled from its snapshots by a
    256-wide teacher, B_global > B; repeated bit for bit."""
    P = knobs
    F, hid, L, H = 72, 128, 2, 32
    params, pol = _kink_free_student(P)
    _, ro = _collect(P, pol, 48, 8, 8, True, 31)
    teacher = _policy(P, 72, 256, 2, params_for(P, 72, 256, 2, np.random.default_rng(12)))
    P.fill_targets_(ro, teacher)
    st, act = ro.state_data
    states, active = st.reshape(-1, H, F), act.reshape(-1)
    q = ro.action_targets.reshape(-1, 4 * H)
    sel = np.flatnonzero(ref.off_the_kink(params, F, hid, L, states))
    assert len(sel) >= 64
    ds = P.construct_dataset(ro)
    assert np.array_equal(ro.index(), np.arange(len(ds))), "storage order is dataset order here"
    P.set_bwd_split_bf16(split)
    B, Bg = len(sel), 3 * len(sel)
    assert distill_route(P, "f32", F, hid, L, H, True, B) == ("k_policy_fwd<72,128,18,1,0>", bwd)
    ce, ent = P.distill_forward_backward(pol, ds, sel + 1, 0.01, B_global=Bg)
    g = pol.grad()
    P.distill_forward_backward(pol, ds, sel + 1, 0.01, B_global=Bg)
    assert np.array_equal(g, pol.grad()) and g.tobytes() == pol.grad().tobytes()
    ce64, ent64, g64 = ref.loss_grad(params, F, hid, L, states[sel], active[sel], q[sel], np.ones(B), 0.01, B_global=Bg)
    gmax, err = float(np.abs(g64).max()), float(np.abs(g - g64).max())
    _record({"case": "gradient_compact", "B": int(B), "B_global": int(Bg), "bwd": bwd, "max_abs_g64": gmax, "err_over_max": err / gmax})
    assert gmax > 1e-5 and err <= BAR * gmax
    assert abs(ce - ce64) <= (LOSS_BAR + 2.0 ** -23) * max(1.0, abs(ce64))


# ---------------------------------------------------------------- 6. the recorded distributions as targets
def test_recorded_targets(knobs):
    """targets="recorded" on a buffer collected with record_probs=True: dY and the gradient within the bar of the restatement
    fed rollouts.full_probs(); without record_probs the call is PPO_ERR_ARG, also on a buffer that recorded them EARLIER."""
    P = knobs
    F, hid, L, H = 72, 128, 2, 32
    params, pol = _kink_free_student(P)
    actor = P.HipPolicy(72, 256, 2, 4, seed=2)
    env, ro = _collect(P, actor, 48, 8, 8, False, 33, record_probs=True)
    st, act = ro.state_data
    states, active = st.reshape(-1, H, F), act.reshape(-1)
    q = ro.full_probs().reshape(-1, 4 * H)
    sel = np.flatnonzero(ref.off_the_kink(params, F, hid, L, states))
    assert len(sel) >= 64
    ds = P.construct_dataset(ro)
    B = len(sel)
    ce, ent = P.distill_forward_backward(pol, ds, sel + 1, 0.0, targets="recorded")
    g = pol.grad()
    dy, _ = _outputs(P, pol, B, H)
    want = ref.analytic_dy(ref.logits_np(params, F, hid, L, states[sel]), active[sel], q[sel], np.ones(B), H)
    ce64, _, g64 = ref.loss_grad(params, F, hid, L, states[sel], active[sel], q[sel], np.ones(B))
    err = float(np.abs(g - g64).max() / np.abs(g64).max())
    _record({"case": "recorded", "B": int(B), "err_over_max": err, "dy_err_over_max": float(np.abs(dy - want).max() / np.abs(want).max())})
    assert np.abs(dy - want).max() <= BAR * np.abs(want).max() and err <= BAR
    assert abs(ce - ce64) <= (LOSS_BAR + 2.0 ** -23) * max(1.0, abs(ce64))
    with pytest.raises(P.PPOError, match="target column is not filled") as e:
        P.distill_forward_backward(pol, ds, sel + 1)
    assert e.value.status == -1
    P.set_rollout_compact(0)
    P.collect_rollouts_steps_(ro, env, actor, 8, 0.99)               # the same buffer again, nothing recorded this time
    P.set_rollout_compact(None)
    for call in (lambda: P.distill_forward_backward(pol, P.construct_dataset(ro), [1, 2], targets="recorded"),
                 lambda: P.distill_train_(pol, P.Optimiser(P.Adam()), P.construct_dataset(ro), 8, 1, targets="recorded", verbose=False)):
        with pytest.raises(P.PPOError, match="no recorded distributions") as e:
            call()
        assert e.value.status == -1


# ---------------------------------------------------------------- 7. the epoch loop
def test_epoch_loop_against_the_float64_schedule(P):
    """distill_train_, 2 epochs of 3 minibatches (40, 40, 20) with given permutations, against distill_ref.adam_schedule, under
    imitation's schedule bars."""
    F, hid, L, H, B = 72, 128, 2, 32, 100
    params, states, active, actions, adv = _grad_case(P, F, hid, L, H, B, 4)
    q = _dense_targets(np.random.default_rng(7), active, H)
    pol = _policy(P, F, hid, L, params)
    _, ds = _dataset(P, dict(states=states, active=active, actions=actions, adv=adv), q)
    perms = np.stack([np.random.default_rng(40 + e).permutation(B) for e in range(2)])
    before, vbefore = pol.last_train_stats(), pol.last_value_stats()
    ch, eh, lh = P.distill_train_(pol, P.Optimiser(P.Adam(ETA)), ds, 40, 2, perm=perms + 1, verbose=False)
    h64, p64 = ref.adam_schedule(params, F, hid, L, states, active, q, np.ones(B), 40, perms, eta=ETA)
    ok, fig = schedule_bars(pol.params, p64, ch, h64, 6)
    _record({"case": "schedule", "device": ch, "float64": h64, **fig})
    assert len(ch) == len(eh) == len(lh) == 2 and lh == [ETA] * 2
    assert eh == [0.0, 0.0], "entropy_weight = 0: the entropy history is exactly 0"
    assert h64[-1] < h64[0], "the float64 restatement must satisfy the condition by itself"
    assert ch[-1] < ch[0]
    assert ok, fig
    after = pol.last_train_stats()
    assert after["epochs_run"] == before["epochs_run"] and after["stopped_early"] == before["stopped_early"]
    assert pol.last_value_stats()["epochs_run"] == vbefore["epochs_run"]


# ---------------------------------------------------------------- 8. closure on the device
def test_distil_a_wide_teacher_into_a_narrow_student(knobs):
    """Q = 8, 64 envs, T = 16: a (72,256,2) teacher of perturbed parameters into a fresh (72,128,2) student, 4 epochs.  The mean
    KL(teacher || student) over the buffer, computed on the host from ppo_policy_forward of both, falls."""
    P = knobs
    teacher = _policy(P, 72, 256, 2, params_for(P, 72, 256, 2, np.random.default_rng(21)))
    student = P.HipPolicy(72, 128, 2, 4, seed=6)
    _, ro = _collect(P, teacher, 64, 16, 8, False, 41, max_actions=16)
    P.fill_targets_(ro, teacher)
    st, act = ro.state_data
    states, active = st.reshape(-1, 32, 72), act.reshape(-1)
    pt = P._forward(teacher, states, active).astype(np.float64)

    def mean_kl():
        ps = P._forward(student, states, active).astype(np.float64)
        keep = pt > 0
        return float((pt[keep] * (np.log(pt[keep]) - np.log(ps[keep]))).sum() / len(pt))

    kl0 = mean_kl()
    ch, _, _ = P.distill_train_(student, P.Optimiser(P.Adam(ETA)), P.construct_dataset(ro), 256, 4, seed=3, verbose=False)
    kl1 = mean_kl()
    _record({"case": "closure", "transitions": len(ro), "mean_kl_before": kl0, "mean_kl_after": kl1, "ce_history": ch})
    assert np.isfinite(kl0) and np.isfinite(kl1) and kl1 < kl0 and ch[-1] < ch[0]


# ---------------------------------------------------------------- 9. invalidation, refusals, nothing else moved
def test_invalidation_and_refusals(knobs, tmp_path):
    P = knobs
    pol = P.HipPolicy(72, 128, 2, 4, seed=1)
    teacher = P.HipPolicy(72, 256, 2, 4, seed=2)
    env, ro = _collect(P, pol, 8, 6, 8, True, 1, max_actions=5)
    idx = np.arange(1, 9)

    def both(policy, rollouts=None, **kw):
        r = rollouts or ro
        return (lambda: P.distill_forward_backward(policy, P.construct_dataset(r), idx, **kw),
                lambda: P.distill_train_(policy, P.Optimiser(P.Adam()), P.construct_dataset(r), 8, 1, verbose=False, **kw))

    def refused(calls, status, text):
        for call in calls:
            with pytest.raises(P.PPOError, match=text or None) as e:
                call()
            assert e.value.status == status, (text, e.value.status)

    # not filled yet; filled; a collect invalidates; the next fill restores; so does set_columns on an expanded buffer
    refused(both(pol), -1, "target column is not filled")
    with pytest.raises(P.PPOError, match="target column is not filled"):
        ro.action_targets
    P.fill_targets_(ro, teacher)
    ce, _ = P.distill_forward_backward(pol, P.construct_dataset(ro), idx)
    assert np.isfinite(ce)
    P.set_rollout_compact(1)
    P.collect_rollouts_steps_(ro, env, pol, 6, 0.99)
    P.set_rollout_compact(None)
    refused(both(pol), -1, "target column is not filled")
    P.fill_targets_(ro, teacher)
    assert np.isfinite(P.distill_forward_backward(pol, P.construct_dataset(ro), idx)[0])
    st, act = ro.state_data
    roe = P.BufferRollouts()
    cols = (st, act, ro.selected_actions, ro.selected_action_probabilities, ro.rewards)
    roe.set_columns(None, *cols)
    roe.set_action_targets(ro.action_targets)
    assert np.isfinite(P.distill_forward_backward(pol, P.construct_dataset(roe), idx)[0])
    roe.set_columns(None, *cols)
    refused(both(pol, roe), -1, "target column is not filled")
    # refusals
    bf = P.HipPolicy(72, 128, 2, 4, seed=1, dtype="bf16")
    refused(both(bf), -4, NO_BF16_STUDENT)
    with pytest.raises(P.PPOError, match="bf16-dtype teacher on a compact buffer") as e:
        P.fill_targets_(ro, P.HipPolicy(72, 256, 2, 4, seed=2, dtype="bf16"))
    assert e.value.status == -4
    refused(both(pol, advantage="gae_normalised") + both(pol, weights="positive_advantage", advantage="returns_normalised")
            + both(pol, targets="search") + both(pol, weights="exp"), -4, "")
    L = P._lib.lib()                                     # ... and at the C ABI, past the mirror's own check
    i0 = np.zeros(1, np.int64)
    for wm, am, ts, text in ((0, 1, 0, "normalised advantage modes are not supported"), (1, 3, 0, "normalised advantage modes are not supported"),
                             (2, 0, 0, "unknown weight mode"), (0, 9, 0, "unknown advantage mode"), (0, 0, 2, "unknown target source")):
        assert L.ppo_distill_forward_backward(pol._h, ro._h, i0.ctypes.data_as(P._lib.c_i64p), 1, 1, 0.0, wm, am, ts) == -4
        assert text in P._lib.last_error()
    with pytest.raises(P.PPOError, match="teacher's input width F differs from the buffer's") as e:
        P.fill_targets_(ro, P.HipPolicy(216, 128, 2, 4, seed=1))
    assert e.value.status == -1
    bad = np.zeros(6 * 8 * 128, np.float32)
    bad[77] = -1.0
    assert L.ppo_rollouts_set_targets(ro._h, bad.ctypes.data_as(P._lib.c_f32p)) == -1 and "finite and >= 0" in P._lib.last_error()
    # a buffer with a disk sink attached
    rod = P.BufferRollouts()
    h = rod._ensure(env, 0)
    P._lib.call("ppo_rollouts_attach_disk", h, str(tmp_path / "sink").encode(), 4)
    P._lib.call("ppo_collect_rollouts", h, env._h, pol._h, 6, 0.99, 0, 0)
    for fn in (lambda: P.fill_targets_(rod, teacher), lambda: rod.set_action_targets(np.zeros((6, 8, 128), np.float32)),
               lambda: P.distill_forward_backward(pol, P.construct_dataset(rod), idx)):
        with pytest.raises(P.PPOError, match="a buffer with a disk sink attached is not supported") as e:
            fn()
        assert e.value.status == -4
    P._lib.call("ppo_rollouts_detach_disk", h)


def test_other_objectives_and_statistics_unchanged(P):
    """Distil calls between them leave the bytes of the PPO, imitation and value gradients and last_train_stats() alone."""
    F, hid, L, H, B = 72, 128, 2, 32, 64
    params, states, active, actions, adv = _grad_case(P, F, hid, L, H, B, 8)
    pol = _policy(P, F, hid, L, params)
    critic = P.HipCritic(F, hid, L, seed=4)
    q = _dense_targets(np.random.default_rng(2), active, H)
    ro, ds = _dataset(P, dict(states=states, active=active, actions=actions, adv=adv), q)
    idx = np.arange(1, B + 1)
    pol.target_kl = float("inf")
    P.ppo_train_(pol, P.Optimiser(P.Adam(1e-4)), ds, 0.05, 32, 2, 0.01, seed=1, verbose=False)
    stats = pol.last_train_stats()
    assert stats["epochs_run"] == 2 and np.all(np.isfinite(stats["approx_kl"]))

    def others():
        l = P.forward_backward(pol, ds, idx, 0.05, 0.01)
        g = pol.grad().tobytes()
        i = P.imitate_forward_backward(pol, ds, idx, 0.01)
        gi = pol.grad().tobytes()
        v = P.value_forward_backward(critic, ds, idx)
        return l, g, i, gi, v, critic.grad().tobytes()

    before = others()
    P.distill_forward_backward(pol, ds, idx, 0.01)
    P.distill_forward_backward(critic, ds, idx, 0.01, weights="positive_advantage")
    assert others() == before
    p0 = pol.params
    P.distill_train_(pol, P.Optimiser(P.Adam(1e-4)), ds, 32, 3, 0.01, seed=2, verbose=False)
    assert not np.array_equal(pol.params, p0)
    after = pol.last_train_stats()
    assert after["epochs_run"] == 2 and after["stopped_early"] == stats["stopped_early"]
    for k in ("approx_kl", "old_approx_kl", "clip_fraction"):
        assert np.array_equal(after[k], stats[k]), k
    assert np.array_equal(ro.action_targets.reshape(B, -1), q), "training reads the column, it does not write it"
