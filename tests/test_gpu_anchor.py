"""KL-anchored PPO on the device: the anchored train forward (k_policy_fwd modes 20 / 21, policy_tail's
TrainAnchored branch), the backwards anchor_route pairs it with, the per-epoch anchor KL and the coefficient rule of the epoch
loop, against the float64 restatement tests/anchor_ref.py.  TEST_RECORD_DIR=<dir>: measured figures go to <dir>/kl_anchor.jsonl.

Bars.  Gradients and dL/dlogits: BAR = 2e-5 relative to the largest reference entry (tests/test_gpu_bench_shapes.py).  The
per-state loss terms, ratios and divergences and the two loss scalars: LOSS_BAR relative to max(1, largest reference entry).
LOSS_BAR is four times the largest error of a plain numpy-float32 restatement (forward, softmax, surrogate, the sums over up to
512 products and the entropy in float32: anchor_ref with dtype=float32) against float64 over the cases of tests 1 and 2 -- every
shape of SHAPE_H with the "kinds" targets and the three underflow cases, both runs of RUNS -- measured on a CPU by
measure_loss_bar() below (tests/test_anchor_host.py runs it and holds LOSS_BAR to it): 2.07e-6 (the ratios p_new / p_old of the
least likely actions, whose float32 probability carries the rounding of a logit difference near 10; the loss terms 4.1e-7, the
divergences 2.1e-7, the entropy terms of the underflow cases 1.24e-6 as in tests/test_gpu_distill.py), and 4 x 2.07e-6 = 8.28e-6
rounds up to 9e-6.  The device's own error is recorded beside it and was not used to set the bar.

Byte identities.  Test 4 (zero advantages are distillation) compares every output byte for byte.  Test 3 (coef = 0 is
FwdMode::Train) compares loss terms, ratios and gradient byte for byte and dL/dlogits value for value: where FwdMode::Train leaves
an exact -0.0 (a row of an inactive quad, p = 0, times a negative factor) the anchored line adds it to the exact zero
beta / B * (p Qs - q') and IEEE addition gives +0.0; the test asserts that every word that differs is such a pair of zeros."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import anchor_ref as ref
from test_anchor_host import NO_BF16_ANCHOR, anchor_route
from test_gpu_distill import UNDERFLOW_SHAPES, kinds_targets, underflow_targets
from test_gpu_imitation import B1, BAR, ETA, GRAD_CASES, SHAPE_H, _grad_case, _outputs, _policy, case1, params_for, schedule_bars
from test_train_route import route

pytestmark = pytest.mark.gpu

LOSS_BAR = 9e-6                              # see the module docstring
EPS = 0.2
RUNS = ((0.75, 1, 0.01), (2.5, 3, 0.02))     # (coef, B_global / B, entropy_weight); both coefficients are float32 numbers
RATIOS = (0.7, 0.95, 1.05, 1.4)              # p_new / p_old by state: well off the clip's 0.8 and 1.2


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
    P.set_fwd_split_max_states(None)


def _record(rec):
    print(json.dumps(rec))
    d = os.environ.get("TEST_RECORD_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "kl_anchor.jsonl"), "a") as f:
            f.write(json.dumps(rec) + "\n")


def _debug_col(P, pol, name, n):
    fn = getattr(P._lib.lib(), name)
    fn.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    fn.restype = C.c_int32
    out = np.zeros(n, np.float32)
    assert fn(pol._h, n, out.ctypes.data) == 0, P._lib.last_error()
    return out


def _ratios(P, pol, n):
    return _debug_col(P, pol, "ppo_debug_train_ratios", n)


def _anchor_kl(P, pol, n):
    return _debug_col(P, pol, "ppo_debug_anchor_kl", n)


# ---------------------------------------------------------------- the cases of tests 1 and 2 (no device needed)
def old_probs(logits, active, actions, H, underflow=False):
    """p_old [B] float32: the float64 probability of the given action divided by RATIOS[b % 4], so that the ratio the surrogate
    forms is that number; underflow (the current policy gives the action exp = 0): 0.05 + 0.01 (b % 5), as a behaviour policy
    that played the action gave it."""
    B = len(actions)
    if underflow:
        return (0.05 + 0.01 * (np.arange(B) % 5)).astype(np.float32)
    _, p = ref.log_probs_np(logits, ref.action_mask(active, H))
    return (p[np.arange(B), actions] / np.array(RATIOS)[np.arange(B) % 4]).astype(np.float32)


def anchor_case(ppo, F, hid, L, H, underflow=False):
    """case1 (tests/test_gpu_imitation.py) with its weights as the advantages (both signs and zero), p_old and a target row
    per state: the "kinds" rows of the distillation tests, or their underflow rows."""
    c = case1(ppo, F, hid, L, H, underflow=underflow)
    c["p_old"] = old_probs(c["logits"], c["active"], c["actions"], H, underflow)
    c["q"] = underflow_targets(c, H) if underflow else kinds_targets(c, H)
    return c


def kinds_present(c, H):
    """What test 1 asserts of its own inputs: every kind of target row and both sides of the clip occur."""
    mask = ref.action_mask(c["active"], H)
    q = c["q"]
    kept = np.where(mask, q, 0).sum(axis=1)
    total = q.sum(axis=1)
    _, p = ref.log_probs_np(c["logits"], mask)
    _, un = ref.surrogate(p[np.arange(len(q)), c["actions"]], c["p_old"], c["adv"], EPS)
    out = dict(dense_with_ignored_mass=bool(((total - kept > 1e-3) & ((q > 0).sum(axis=1) > 4 * H // 2)).any()),
               one_hot=bool((((q > 0).sum(axis=1) == 1) & (np.abs(total - 1) < 1e-6)).any()),
               sub_normalised=bool(((np.abs(total - 0.5) < 1e-3) & (np.abs(kept - 0.5) < 1e-3)).any()),
               all_zero=bool((total == 0).any()), clipped=bool((~un).any()), unclipped=bool(un.any()),
               advantages_of_both_signs=bool((c["adv"] > 0).any() and (c["adv"] < 0).any()))
    if H == 128:
        out["one_tile"] = all(q[b, 128 * (b - 4):128 * (b - 3)].sum() == q[b].sum() > 0 for b in range(4, 8))
    return out


def loss_errors(c, F, hid, L, H, coef, ew, dtype, terms=None, ratio=None, kl=None, Bg=None):
    """max error against float64, each relative to max(1, largest reference entry): of a restatement in `dtype`, or of the
    device's per-state `terms` [B, 2], `ratio` [B] and `kl` [B], the scalars summed in float64."""
    t0, t1, r, k = ref.per_state_terms(c["logits"], c["active"], c["actions"], c["p_old"], c["adv"], EPS, c["q"], coef, H)
    Bg = Bg or len(t0)
    lo, ent = -t0.sum() / Bg, ew * -t1.sum() / Bg
    if terms is None:
        lg = ref.logits_np(c["params"], F, hid, L, c["states"], dtype)
        g0, g1, gr, gk = ref.per_state_terms(lg, c["active"], c["actions"], c["p_old"], c["adv"], EPS, c["q"], coef, H, dtype)
        glo = float(dtype(-(g0.sum() / Bg)))
        gent = float(dtype(ew) * dtype(-(g1.astype(dtype).sum(dtype=dtype) / dtype(Bg))))
    else:
        g0, g1, gr, gk = terms[:, 0], terms[:, 1], ratio, kl
        glo, gent = -g0.sum() / Bg, ew * -g1.sum() / Bg

    def rel(g, t):
        return float(np.abs(np.asarray(g, np.float64) - t).max() / max(1.0, np.abs(t).max()))
    return dict(loss_terms=rel(g0, t0), ent_terms=rel(g1, t1), ratio=rel(gr, r), kl=rel(gk, k),
                loss=float(abs(glo - lo) / max(1.0, abs(lo))), ent=float(abs(gent - ent) / max(1.0, abs(ent))))


def measure_loss_bar(ppo):
    """The figure LOSS_BAR rests on (CPU only): the largest float32-restatement error over the cases of tests 1 and 2, split
    into the underflow cases and the others."""
    worst = {"underflow": {}, "others": {}}
    for group, shapes in (("others", SHAPE_H), ("underflow", UNDERFLOW_SHAPES)):
        for (F, hid, L, H) in shapes:
            c = anchor_case(ppo, F, hid, L, H, underflow=group == "underflow")
            for coef, k, ew in RUNS:
                e = loss_errors(c, F, hid, L, H, coef, ew, np.float32, Bg=k * B1)
                for key, v in e.items():
                    worst[group][key] = max(worst[group].get(key, 0.0), v)
    return worst


def _abuffer(P, c, adv=None, T=1):
    """An expanded buffer of the case's states with its actions, p_old and advantages (the returns column), targets uploaded."""
    B, H, F = c["states"].shape
    N = B // T
    ro = P.BufferRollouts()
    ro.set_columns(None, c["states"].reshape(T, N, H, F), c["active"].reshape(T, N), (c["actions"] + 1).reshape(T, N),
                   np.asarray(c["p_old"], np.float32).reshape(T, N),
                   np.asarray(c["adv"] if adv is None else adv, np.float32).reshape(T, N), np.zeros((T, N), np.uint8))
    if c.get("q") is not None:
        ro.set_action_targets(np.asarray(c["q"], np.float32).reshape(T, N, 4 * H))
    return ro


def _check_outputs(P, pol, ds, c, F, hid, L, H, tag):
    """Both runs on one dataset: dY exactly 0 on inactive rows and within BAR of the analytic float64 dL/dlogits; loss terms,
    ratios, divergences and scalars within LOSS_BAR; B_global > B in the second run."""
    B = len(c["active"])
    on = ref.row_mask(c["active"], H)
    pol.target_kl = float("inf")                           # the ratios are stored while a target is set
    for coef, k, ew in RUNS:
        Bg = k * B
        pol.kl_anchor = (coef, "column")
        lo, ent = P.forward_backward(pol, ds, np.arange(1, B + 1), EPS, ew, B_global=Bg)
        dy, lt = _outputs(P, pol, B, H)
        ratio, kl = _ratios(P, pol, B), _anchor_kl(P, pol, B)
        want = ref.analytic_dy(c["logits"], c["active"], c["actions"], c["p_old"], c["adv"], EPS, c["q"], coef, H, ew, Bg)
        assert np.all(np.isfinite(dy)) and np.all(np.isfinite(lt)) and np.all(np.isfinite(kl)) and np.all(np.isfinite(ratio))
        assert np.isfinite(lo) and np.isfinite(ent)
        err_dy = float(np.abs(dy - want).max() / np.abs(want).max())
        dev = loss_errors(c, F, hid, L, H, coef, ew, None, terms=lt, ratio=ratio, kl=kl, Bg=Bg)
        f32 = loss_errors(c, F, hid, L, H, coef, ew, np.float32, Bg=Bg)
        t0, t1, _, k64 = ref.per_state_terms(c["logits"], c["active"], c["actions"], c["p_old"], c["adv"], EPS, c["q"], coef, H)
        err_lo = abs(lo - -t0.sum() / Bg) / max(1.0, abs(t0.sum() / Bg))
        err_ent = abs(ent - ew * -t1.sum() / Bg) / max(1.0, abs(ew * t1.sum() / Bg))
        _record({"case": tag, "shape": [F, hid, L, H], "coef": coef, "B_global": Bg, "dy_err_over_max": err_dy,
                 "loss_err_device": dev, "loss_err_numpy_f32": f32, "loss_scalar_err": float(err_lo), "ent_scalar_err": float(err_ent),
                 "max_kl": float(k64.max())})
        assert not dy[~on].any(), "rows of inactive quads get exactly 0"
        assert err_dy <= BAR, (tag, coef, err_dy)
        assert max(dev.values()) <= LOSS_BAR, (tag, coef, dev)
        assert err_lo <= LOSS_BAR + 2.0 ** -23 and err_ent <= LOSS_BAR + 2.0 ** -23, "the scalars are stored as floats"
        full = (np.abs(np.where(ref.action_mask(c["active"], H), c["q"], 0).sum(axis=1) - 1) < 1e-5)
        assert (kl[full] >= -LOSS_BAR * max(1.0, k64.max())).all(), "a normalised kept row: a divergence, at least 0"
    pol.kl_anchor = None
    pol.target_kl = None


# ---------------------------------------------------------------- 1. per-state outputs
@pytest.mark.parametrize("F,hid,L,H", SHAPE_H)
def test_per_state_outputs(P, F, hid, L, H):
    """dY, both loss terms, ratio_out and anchor_out for every kind of target row, clipped and unclipped states."""
    c = anchor_case(P, F, hid, L, H)
    have = kinds_present(c, H)
    assert all(have.values()), have
    pol = _policy(P, F, hid, L, c["params"])
    hk = 128 if hid <= 128 else 256
    assert anchor_route(P, "f32", F, hk, L, H, False, B1)[0] == "k_policy_fwd<%d,%d,20,%d,%d>" % (F, hk, H // 32, int(L != 2))
    ds = P.construct_dataset(_abuffer(P, c))
    _check_outputs(P, pol, ds, c, F, hid, L, H, "outputs_kinds")


@pytest.mark.parametrize("hid,L,H", [(hid, L, H) for (F, hid, L, H) in SHAPE_H if F == 72])
def test_per_state_outputs_from_compact_buffers(knobs, hid, L, H):
    """Mode 21: a compact buffer collected on the device, the "kinds" rows uploaded for its states; advantages are the buffer's
    own returns, p_old what the collecting policy gave.  The rows mode 21 leaves the backward are mode 20's: the gradient of
    the expanded form of the same data, bit for bit."""
    P = knobs
    F, Q = 72, H // 4
    params = params_for(P, F, hid, L, np.random.default_rng(hid + L + H))
    pol = _policy(P, F, hid, L, params)
    env = P.HipVecEnv(num_envs=B1, Q=Q, max_actions=6, seed=77)
    ro = P.BufferRollouts()
    P.set_rollout_compact(1)
    P.collect_rollouts_steps_(ro, env, pol, 1, 0.99)
    P.set_rollout_compact(None)
    st, act = ro.state_data
    c = dict(params=params, states=st.reshape(B1, H, F), active=act.reshape(-1), adv=ro.rewards.reshape(-1).astype(np.float32),
             actions=ro.selected_actions.reshape(-1) - 1, p_old=ro.selected_action_probabilities.reshape(-1).astype(np.float32))
    c["logits"] = ref.logits_np(params, F, hid, L, c["states"])
    c["q"] = kinds_targets(c, H)
    ro.set_action_targets(c["q"].reshape(1, B1, 4 * H))
    hk = 128 if hid <= 128 else 256
    assert anchor_route(P, "f32", F, hk, L, H, True, B1)[0] == "k_policy_fwd<72,%d,21,%d,%d>" % (hk, H // 32, int(L != 2))
    ds = P.construct_dataset(ro)
    _check_outputs(P, pol, ds, c, F, hid, L, H, "outputs_compact")
    pol.kl_anchor = (0.75, "column")
    P.forward_backward(pol, ds, np.arange(1, B1 + 1), EPS, 0.01)
    g21 = pol.grad()
    P.forward_backward(pol, P.construct_dataset(_abuffer(P, c)), np.arange(1, B1 + 1), EPS, 0.01)
    assert g21.tobytes() == pol.grad().tobytes()


# ---------------------------------------------------------------- 2. the underflow case
@pytest.mark.parametrize("F,hid,L,H", UNDERFLOW_SHAPES)
def test_underflow_case(P, F, hid, L, H):
    """The whole target mass, and the stored action, where the policy's exp(l - m) is 0 in float32: log(p) is -inf and a
    division by p NaN; the log-softmax tail keeps loss, gradient and divergence finite and within the bars of test 1."""
    c = anchor_case(P, F, hid, L, H, underflow=True)
    pol = _policy(P, F, hid, L, c["params"])
    ds = P.construct_dataset(_abuffer(P, c))
    _check_outputs(P, pol, ds, c, F, hid, L, H, "underflow")
    assert np.all(np.isfinite(pol.grad()))


# ---------------------------------------------------------------- 3. coef = 0 is FwdMode::Train
@pytest.mark.parametrize("F,hid,L,H", [(72, 256, 2, 32), (72, 128, 2, 128), (72, 128, 3, 32), (216, 128, 2, 32)])
def test_zero_coefficient_is_the_plain_train_forward(knobs, F, hid, L, H):
    """The plain objective forced onto k_policy_fwd (mode 2) against the anchored run at coef = 0 (mode 20): loss terms, ratios,
    losses and gradient byte for byte, dL/dlogits value for value with signed zeros as the module docstring states; anchor_out
    is still the divergence."""
    P = knobs
    c = anchor_case(P, F, hid, L, H)
    pol = _policy(P, F, hid, L, c["params"])
    ds = P.construct_dataset(_abuffer(P, c))
    idx = np.arange(1, B1 + 1)
    pol.target_kl = float("inf")
    P.set_bwd_split_bf16(0)
    P.set_train_tile_max_tiles(0)
    P.set_fwd_split_max_states(0)
    assert route(P, "f32", F, hid, L, H, False, B1)[0] == "k_policy_fwd<%d,%d,2,%d,%d>" % (F, hid, H // 32, int(L != 2))
    for k, ew in ((1, 0.01), (3, 0.0)):
        pol.kl_anchor = None
        lt_ = P.forward_backward(pol, ds, idx, EPS, ew, B_global=k * B1)
        dyt, ltt = _outputs(P, pol, B1, H)
        gt, rt = pol.grad(), _ratios(P, pol, B1)
        pol.kl_anchor = (0.0, "column")
        la = P.forward_backward(pol, ds, idx, EPS, ew, B_global=k * B1)
        dya, lta = _outputs(P, pol, B1, H)
        ga, ra, kl = pol.grad(), _ratios(P, pol, B1), _anchor_kl(P, pol, B1)
        differ = dyt.view(np.uint32) != dya.view(np.uint32)
        _record({"case": "zero_coef", "shape": [F, hid, L, H], "entropy_weight": ew, "dy_words_differing": int(differ.sum()),
                 "grad_bitwise": bool(gt.tobytes() == ga.tobytes())})
        assert ltt.tobytes() == lta.tobytes() and rt.tobytes() == ra.tobytes() and lt_ == la
        assert gt.tobytes() == ga.tobytes()
        assert np.array_equal(dyt, dya)
        assert (dyt[differ] == 0).all() and (dya[differ] == 0).all() and not np.signbit(dya[differ]).any()
        assert not differ[ref.row_mask(c["active"], H)].any(), "rows of active quads are byte-identical"
        k64 = ref.state_kl(c["logits"], c["active"], c["q"], H)
        assert np.abs(kl - k64).max() <= LOSS_BAR * max(1.0, k64.max()) and k64.max() > 0.1


# ---------------------------------------------------------------- 4. zero advantages are distillation
@pytest.mark.parametrize("F,hid,L,H", [(72, 256, 2, 32), (72, 128, 2, 128), (72, 128, 3, 32), (216, 128, 2, 32)])
def test_zero_advantages_are_distillation(P, F, hid, L, H):
    """An advantage column of zeros and any p_old: dY, loss terms, losses and gradient equal distill_forward_backward with
    weights="positive_advantage" on a column holding coef, byte for byte; loss column 0 is coef * ce."""
    c = anchor_case(P, F, hid, L, H)
    pol = _policy(P, F, hid, L, c["params"])
    idx = np.arange(1, B1 + 1)
    for coef, k, ew in RUNS + ((0.375, 2, 0.0),):
        dsa = P.construct_dataset(_abuffer(P, c, adv=np.zeros(B1, np.float32)))
        dsd = P.construct_dataset(_abuffer(P, c, adv=np.full(B1, coef, np.float32)))
        pol.kl_anchor = (coef, "column")
        la = P.forward_backward(pol, dsa, idx, EPS, ew, B_global=k * B1)
        dya, lta = _outputs(P, pol, B1, H)
        ga = pol.grad()
        pol.kl_anchor = None
        ld = P.distill_forward_backward(pol, dsd, idx, ew, weights="positive_advantage", B_global=k * B1)
        dyd, ltd = _outputs(P, pol, B1, H)
        gd = pol.grad()
        _record({"case": "zero_adv", "shape": [F, hid, L, H], "coef": coef,
                 "bitwise": [bool(dya.tobytes() == dyd.tobytes()), bool(lta.tobytes() == ltd.tobytes()), bool(ga.tobytes() == gd.tobytes())]})
        assert dya.tobytes() == dyd.tobytes() and lta.tobytes() == ltd.tobytes() and ga.tobytes() == gd.tobytes() and la == ld
        ce64 = ref.per_state_terms(c["logits"], c["active"], c["actions"], c["p_old"], np.zeros(B1), EPS, c["q"], 1.0, H)[0]
        assert abs(la[0] - coef * -ce64.sum() / (k * B1)) <= (LOSS_BAR + 2.0 ** -23) * max(1.0, coef * abs(ce64.sum()) / (k * B1))


# ---------------------------------------------------------------- 5. the full gradient
def _anchor_grad_case(P, F, hid, L, H, B, seed):
    params, states, active, actions, adv = _grad_case(P, F, hid, L, H, B, seed)
    logits = ref.logits_np(params, F, hid, L, states)
    rng = np.random.default_rng(seed + 1)
    e = np.exp(rng.normal(size=(B, 4 * H)) * 2)
    return dict(params=params, states=states, active=active, actions=actions, adv=adv, logits=logits,
                p_old=old_probs(logits, active, actions, H), q=(e / e.sum(axis=1, keepdims=True)).astype(np.float32))


def _check_gradient(P, pol, ds, c, F, hid, L, H, B, tag, bwd):
    for coef, k, ew in RUNS:
        Bg = k * B
        pol.kl_anchor = (coef, "column")
        lo, ent = P.forward_backward(pol, ds, np.arange(1, B + 1), EPS, ew, B_global=Bg)
        g = pol.grad()
        lo2, _ = P.forward_backward(pol, ds, np.arange(1, B + 1), EPS, ew, B_global=Bg)
        assert g.tobytes() == pol.grad().tobytes() and lo == lo2, "a second call repeats the first bit for bit"
        r = ref.loss_grad(c["params"], F, hid, L, c["states"], c["active"], c["actions"], c["p_old"], c["adv"], EPS, c["q"], coef, ew,
                          B_global=Bg)
        gmax, err = float(np.abs(r["grad"]).max()), float(np.abs(g - r["grad"]).max())
        _record({"case": tag, "shape": [F, hid, L, H], "B": B, "B_global": Bg, "coef": coef, "bwd": bwd, "max_abs_g64": gmax,
                 "err_over_max": err / gmax, "loss": lo, "loss64": r["loss"], "ent": ent, "ent64": r["entropy"]})
        assert gmax > 1e-4
        assert err <= BAR * gmax, (coef, err, gmax)
        assert abs(lo - r["loss"]) <= (LOSS_BAR + 2.0 ** -23) * max(1.0, abs(r["loss"]))
        assert abs(ent - r["entropy"]) <= (LOSS_BAR + 2.0 ** -23) * max(1.0, abs(r["entropy"]))
    pol.kl_anchor = None


@pytest.mark.parametrize("F,hid,L,H,B,split,bwd", GRAD_CASES)
def test_full_gradient_against_float64(knobs, F, hid, L, H, B, split, bwd):
    """max|g - g64| <= BAR max|g64| through every backward the route pairs the anchored forward with."""
    P = knobs
    c = _anchor_grad_case(P, F, hid, L, H, B, 700 + hid + L + H + B)
    pol = _policy(P, F, hid, L, c["params"])
    ds = P.construct_dataset(_abuffer(P, c))
    P.set_bwd_split_bf16(split)
    assert anchor_route(P, "f32", F, hid, L, H, False, B) == ("k_policy_fwd<%d,%d,20,%d,%d>" % (F, hid, H // 32, int(L != 2)), bwd)
    _check_gradient(P, pol, ds, c, F, hid, L, H, B, "gradient", bwd)
    assert np.array_equal(pol.params, c["params"]), "forward_backward does not touch the parameters"


def test_full_gradient_from_compact_storage(knobs):
    """Mode 21 with the split-fp32 backward: 12 envs x 8 steps collected into a compact buffer."""
    P = knobs
    F, hid, L, H, N, T = 72, 256, 2, 32, 12, 8
    params = params_for(P, F, hid, L, np.random.default_rng(91))
    pol = _policy(P, F, hid, L, params)
    env = P.HipVecEnv(num_envs=N, Q=8, max_actions=6, seed=13)
    ro = P.BufferRollouts()
    P.set_rollout_compact(1)
    P.collect_rollouts_steps_(ro, env, pol, T, 0.99)
    P.set_rollout_compact(None)
    ds = P.construct_dataset(ro)
    B = len(ds)
    assert B == N * T and np.array_equal(ro.index(), np.arange(B))
    st, act = ro.state_data
    c = dict(params=params, states=st.reshape(B, H, F), active=act.reshape(-1), adv=ro.rewards.reshape(-1).astype(np.float32),
             actions=ro.selected_actions.reshape(-1) - 1, p_old=ro.selected_action_probabilities.reshape(-1).astype(np.float32))
    e = np.exp(np.random.default_rng(92).normal(size=(B, 4 * H)) * 2)
    c["q"] = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    ro.set_action_targets(c["q"].reshape(T, N, 4 * H))
    assert anchor_route(P, "f32", F, hid, L, H, True, B) == ("k_policy_fwd<72,256,21,1,0>", "k_policy_bwd_x6<72,256>")
    _check_gradient(P, pol, ds, c, F, hid, L, H, B, "gradient_compact", "k_policy_bwd_x6<72,256>")


# ---------------------------------------------------------------- 6. the epoch loop
def _loop_case(P):
    F, hid, L, H, B = 72, 128, 2, 32, 100
    c = _anchor_grad_case(P, F, hid, L, H, B, 6)
    # the anchor: the policy's own distribution a little way off (parameters + noise), so that the divergence is small at the
    # start and moves by a multiple of itself within a few Adam steps
    tp = (c["params"] + np.random.default_rng(66).normal(size=c["params"].size).astype(np.float32) * 0.002).astype(np.float32)
    _, q = ref.log_probs_np(ref.logits_np(tp, F, hid, L, c["states"]), ref.action_mask(c["active"], H))
    c["q"] = q.astype(np.float32)
    perms = np.stack([np.random.default_rng(60 + e).permutation(B) for e in range(3)])
    return F, hid, L, H, B, c, perms


def choose_target(F, hid, L, H, c, perms, coef0, batch=40):
    """A target d for which the float64 replay both doubles and halves the coefficient within the run, with every epoch's mean
    divergence at least 10 % away from both thresholds: the first such d of a geometric grid around the replay's own divergences
    at a fixed coefficient.  Returns (d, replay)."""
    base = ref.adam_schedule(c["params"], F, hid, L, c["states"], c["active"], c["actions"], c["p_old"], c["adv"], EPS, c["q"], coef0,
                             batch, perms, eta=ETA)
    lo, hi = min(base["kl"]), max(base["kl"])
    for d in np.geomspace(lo / 2, hi * 2, 25):
        r = ref.adam_schedule(c["params"], F, hid, L, c["states"], c["active"], c["actions"], c["p_old"], c["adv"], EPS, c["q"], coef0,
                              batch, perms, target=float(d), eta=ETA)
        coefs = r["coef"] + [r["final_coef"]]
        moves = [b / a for a, b in zip(coefs, coefs[1:])]
        margin = min(min(abs(np.log(k / (1.5 * d))), abs(np.log(k / (d / 1.5)))) for k in r["kl"])
        if 2.0 in moves and 0.5 in moves and margin > 0.1:
            return float(d), r
    return None, base


def test_epoch_loop_against_the_float64_schedule(P):
    """ppo_train_ with an anchor, 3 epochs of 3 minibatches (40, 40, 20) with given permutations, against
    anchor_ref.adam_schedule: the loss history, the per-epoch anchor KL, the coefficient every epoch ran with and the one left
    on the handle, approx_kl with target_kl recording."""
    F, hid, L, H, B, c, perms = _loop_case(P)
    coef0 = 1.0
    d, r = choose_target(F, hid, L, H, c, perms, coef0)
    assert d is not None, r["kl"]
    coefs = r["coef"] + [r["final_coef"]]
    assert any(b == 2 * a for a, b in zip(coefs, coefs[1:])) and any(b == a / 2 for a, b in zip(coefs, coefs[1:])), coefs
    pol = _policy(P, F, hid, L, c["params"])
    ds = P.construct_dataset(_abuffer(P, c))
    pol.kl_anchor = (coef0, "column", d)
    pol.target_kl = float("inf")
    ph, eh, lh = P.ppo_train_(pol, P.Optimiser(P.Adam(ETA)), ds, EPS, 40, 3, 0.0, perm=perms + 1, verbose=False)
    st, ast = pol.last_train_stats(), pol.last_anchor_stats()
    ok, fig = schedule_bars(pol.params, r["params"], ph, r["hist"], 9)
    _record({"case": "schedule", "target": d, "device": ph, "float64": r["hist"], "anchor_kl": ast["anchor_kl"], "anchor_kl64": r["kl"],
             "anchor_coef": ast["anchor_coef"], "coef64": r["coef"], "final_coef": pol.kl_anchor[0], "approx_kl": st["approx_kl"],
             "approx_kl64": r["approx_kl"], **fig})
    assert len(ph) == 3 and lh == [ETA] * 3 and st["epochs_run"] == 3
    assert ok, fig
    assert ast["anchor_coef"] == r["coef"] and pol.kl_anchor == (r["final_coef"], "column", d)
    for got, want in ((ast["anchor_kl"], r["kl"]), (st["approx_kl"], r["approx_kl"]), (st["old_approx_kl"], r["old_approx_kl"])):
        assert np.max(np.abs(np.asarray(got) - np.asarray(want)) / (1 + np.abs(want))) <= 1e-5, (got, want)
    # the last epoch's column is what the statistics were reduced from; a second call starts from the adapted coefficient
    assert abs(float(_anchor_kl(P, pol, B).astype(np.float64).mean()) - ast["anchor_kl"][-1]) <= 1e-12
    P.ppo_train_(pol, P.Optimiser(P.Adam(ETA)), ds, EPS, 40, 1, 0.0, perm=perms[:1] + 1, verbose=False)
    assert pol.last_anchor_stats()["anchor_coef"] == [r["final_coef"]]
    pol.kl_anchor = None
    P.ppo_train_(pol, P.Optimiser(P.Adam(ETA)), ds, EPS, 40, 1, 0.0, perm=perms[:1] + 1, verbose=False)
    assert pol.last_anchor_stats() == {"anchor_kl": [], "anchor_coef": []}


# ---------------------------------------------------------------- 7. source "recorded"
def test_recorded_distributions_as_the_anchor(knobs):
    """PPO's penalty form: the anchor is the behaviour policy's own distribution, recorded at collection time."""
    P = knobs
    F, hid, L, N, T = 72, 128, 2, 32, 8
    params = params_for(P, F, hid, L, np.random.default_rng(7))
    runs = {}
    for name, anchor in (("anchored", (64.0, "recorded")), ("plain", None)):
        pol = _policy(P, F, hid, L, params)
        env = P.HipVecEnv(num_envs=N, Q=8, max_actions=8, seed=3)
        ro = P.BufferRollouts()
        P.set_rollout_compact(0)
        P.collect_rollouts_steps_(ro, env, pol, T, 0.99, record_probs=True)
        ds = P.construct_dataset(ro)
        n = len(ds)
        perms = np.stack([np.random.default_rng(70 + e).permutation(n) for e in range(4)])
        pol.kl_anchor = anchor
        pol.target_kl = float("inf")
        P.ppo_train_(pol, P.Optimiser(P.Adam(ETA)), ds, EPS, n // 4, 1, 0.0, perm=perms[:1] + 1, verbose=False)
        if anchor:
            first = _anchor_kl(P, pol, n)[:n // 4]       # epoch 1, minibatch 1: the policy is the behaviour policy
            assert np.abs(first).max() <= LOSS_BAR, float(np.abs(first).max())
        pol.params = params
        P.ppo_train_(pol, P.Optimiser(P.Adam(ETA)), ds, EPS, n // 4, 4, 0.0, perm=perms + 1, verbose=False)
        runs[name] = pol.last_train_stats()["old_approx_kl"]
        if anchor:
            runs["anchor_kl"] = pol.last_anchor_stats()["anchor_kl"]
    _record({"case": "recorded", **runs})
    assert runs["anchored"][-1] < runs["plain"][-1]


# ---------------------------------------------------------------- 8. refusals and invalidation
def test_refusals_and_invalidation(knobs):
    P = knobs
    F, hid, L, H = 72, 128, 2, 32
    c = anchor_case(P, F, hid, L, H)
    pol = _policy(P, F, hid, L, c["params"])
    idx = np.arange(1, B1 + 1)
    shape = ("f32", F, hid, L, H, False, 4096)
    before = route(P, *shape)
    q, c["q"] = c["q"], None
    ro = _abuffer(P, c)
    ds = P.construct_dataset(ro)
    assert pol.kl_anchor is None
    pol.kl_anchor = (1.0, "column")
    assert pol.kl_anchor == (1.0, "column", 0.0)
    for fn in (lambda: P.forward_backward(pol, ds, idx, EPS, 0.0), lambda: P.step_batch_(pol, P.Optimiser(P.Adam(ETA)), ds, idx, EPS, 0.0),
               lambda: P.ppo_train_(pol, P.Optimiser(P.Adam(ETA)), ds, EPS, 7, 1, 0.0, verbose=False)):
        with pytest.raises(P.PPOError, match="target column is not filled") as e:
            fn()
        assert e.value.status == -1
    pol.kl_anchor = (1.0, "recorded")
    with pytest.raises(P.PPOError, match="no recorded distributions") as e:
        P.forward_backward(pol, ds, idx, EPS, 0.0)
    assert e.value.status == -1
    pol.kl_anchor = (1.0, "column", 0.01)
    ro.set_action_targets(q.reshape(1, B1, 4 * H))
    P.forward_backward(pol, ds, idx, EPS, 0.0)
    # a new collection into the buffer invalidates the column
    env = P.HipVecEnv(num_envs=B1, Q=8, max_actions=6, seed=4)
    ro2 = P.BufferRollouts()
    P.collect_rollouts_steps_(ro2, env, pol, 1, 0.99)
    ro2.set_action_targets(q.reshape(1, B1, 4 * H))
    ds2 = P.construct_dataset(ro2)
    P.forward_backward(pol, ds2, np.arange(1, len(ds2) + 1), EPS, 0.0)
    P.collect_rollouts_steps_(ro2, env, pol, 1, 0.99)
    ds2 = P.construct_dataset(ro2)
    with pytest.raises(P.PPOError, match="target column is not filled"):
        P.forward_backward(pol, ds2, np.arange(1, len(ds2) + 1), EPS, 0.0)
    # the anchor is a property of the handle: other calls leave it alone
    P._forward(pol, c["states"], c["active"])
    pol.params = c["params"]
    P.imitate_forward_backward(pol, ds, idx)
    assert pol.kl_anchor == (1.0, "column", 0.01)
    # a bf16 policy and disk rollouts
    pb = P.HipPolicy(F, hid, L, 4, seed=1, dtype="bf16")
    pb.kl_anchor = (1.0, "column")
    with pytest.raises(P.PPOError, match="bf16") as e:
        P.forward_backward(pb, ds, idx, EPS, 0.0)
    assert e.value.status == -4
    assert anchor_route(P, "bf16", F, hid, L, H, False, 64) == ("none", NO_BF16_ANCHOR)
    # off again: today's routes, and the plain forward
    pol.kl_anchor = None
    assert pol.kl_anchor is None and route(P, *shape) == before and before[0].startswith("k_policy_fwd_train_x6")
    P.forward_backward(pol, ds2, np.arange(1, len(ds2) + 1), EPS, 0.0)


def test_disk_rollouts_are_refused(knobs, tmp_path):
    """A buffer with a disk sink attached (what the distillation entry points refuse): PPO_ERR_UNSUPPORTED from all three calls;
    without the anchor the same buffer trains."""
    P = knobs
    pol = P.HipPolicy(72, 128, 2, 4, seed=1)
    env = P.HipVecEnv(num_envs=8, Q=8, max_actions=6, seed=4)
    rod = P.BufferRollouts()
    h = rod._ensure(env, 0)
    P._lib.call("ppo_rollouts_attach_disk", h, str(tmp_path / "sink").encode(), 4)
    P._lib.call("ppo_collect_rollouts", h, env._h, pol._h, 6, 0.99, 0, 0)
    ds = P.construct_dataset(rod)
    idx = np.arange(1, 9)
    pol.kl_anchor = (1.0, "column")
    for fn in (lambda: P.ppo_train_(pol, P.Optimiser(P.Adam(ETA)), ds, EPS, 4, 1, 0.0, verbose=False),
               lambda: P.forward_backward(pol, ds, idx, EPS, 0.0), lambda: P.step_batch_(pol, P.Optimiser(P.Adam(ETA)), ds, idx, EPS, 0.0)):
        with pytest.raises(P.PPOError, match="disk sink attached is not supported") as e:
            fn()
        assert e.value.status == -4
    pol.kl_anchor = None
    P.forward_backward(pol, ds, idx, EPS, 0.0)
    P._lib.call("ppo_rollouts_detach_disk", h)


# ---------------------------------------------------------------- 9. the other objectives
def test_other_objectives_unchanged(P):
    """ppo_train_, imitate_train_, distill_train_ and value_train_ give the same bytes and statistics with an anchor set on
    ANOTHER policy handle as with none."""
    F, hid, L, H = 72, 128, 2, 32
    c = anchor_case(P, F, hid, L, H)
    ds = P.construct_dataset(_abuffer(P, c))
    perm = np.stack([np.random.default_rng(9).permutation(B1)]) + 1
    out = []
    for other_anchor in (None, (3.0, "column", 0.01)):
        other = _policy(P, F, hid, L, c["params"])
        other.kl_anchor = other_anchor
        res = []
        for name in ("ppo", "imitate", "distill", "value"):
            pol = _policy(P, F, hid, L, c["params"])
            opt = P.Optimiser(P.Adam(ETA))
            if name == "ppo":
                pol.target_kl = float("inf")
                h = P.ppo_train_(pol, opt, ds, EPS, 8, 1, 0.01, perm=perm, verbose=False)
                res.append(json.dumps(pol.last_train_stats()))
                assert pol.last_anchor_stats() == {"anchor_kl": [], "anchor_coef": []}
            elif name == "imitate":
                h = P.imitate_train_(pol, opt, ds, 8, 1, 0.01, perm=perm, verbose=False)
            elif name == "distill":
                h = P.distill_train_(pol, opt, ds, 8, 1, 0.01, perm=perm, verbose=False)
            else:
                h = P.value_train_(pol, opt, ds, 8, 1, perm=perm, verbose=False)
            res += [json.dumps(h), pol.params.tobytes()]
        out.append(res)
    assert out[0] == out[1]
