"""KL-anchored PPO as far as a machine without a GPU can see it: the float64 restatement (tests/anchor_ref.py) held against
itself and against the distillation restatement, the numpy host mirror anchored_ppo_loss against it, the divergence's sign, the
coefficient rule, the route (csrc/ppo_route.hip through ppo_debug_anchor_route), the entry points declared, bound and exported,
the refusals that need no device, ppo_iterate_'s third option name and the float32-restatement measurement the GPU tests' loss
bar rests on."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import anchor_ref as ref
import distill_ref
from test_distill_host import distill_route, target_kinds
from test_imitation_host import _case
from test_train_route import DTYPE, ERR_UNSUPPORTED, SHAPES, SIZES, route

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREE = ("ppo_policy_set_kl_anchor", "ppo_policy_get_kl_anchor", "ppo_policy_last_anchor_stats")
NO_BF16_ANCHOR = "KL-anchored training of a bf16-dtype policy is not supported: the anchored modes exist in the fp32-MFMA forward only"
EPS = 0.2


def anchor_route(ppo, dtype, F, hid, L, H, compact, states):
    lib = ppo._lib.lib()
    fn = lib.ppo_debug_anchor_route
    fn.argtypes = [C.c_int32] * 6 + [C.c_int64, C.c_char_p, C.c_char_p, C.c_int64]
    fn.restype = C.c_int32
    fwd, bwd = C.create_string_buffer(128), C.create_string_buffer(128)
    s = fn(DTYPE[dtype], F, hid, L, H, int(compact), states, fwd, bwd, 128)
    if s != 0:
        assert s == ERR_UNSUPPORTED and fwd.value == b"none" and bwd.value == b"none", (s, fwd.value, bwd.value)
        return ("none", ppo._lib.last_error())
    return (fwd.value.decode(), bwd.value.decode())


@pytest.fixture()
def knobs(ppo):
    yield ppo
    ppo.set_bwd_split_bf16(None)
    ppo.set_train_tile_max_tiles(None)
    ppo.set_bwd_small_max_tiles(None)


def _anchor_case(rng, B, H, F=72, hid=128, L=2):
    """_case (states, masks, allowed actions, advantages of both signs and zero) with p_old on both sides of the clip and a
    target row of every kind."""
    params, states, active, actions, adv = _case(rng, B, H, F, hid, L)
    logits = ref.logits_np(params, F, hid, L, states)
    _, p = ref.log_probs_np(logits, ref.action_mask(active, H))
    p_old = (p[np.arange(B), actions] / np.array([0.7, 0.95, 1.05, 1.4])[np.arange(B) % 4]).astype(np.float32)
    return dict(params=params, states=states, active=active, actions=actions, adv=adv, logits=logits, p_old=p_old,
                q=target_kinds(rng, active, H))


# ---------------------------------------------------------------- the restatement against itself
@pytest.mark.parametrize("F,hid,L,H", [(72, 128, 2, 32), (72, 64, 3, 32), (216, 128, 2, 32), (72, 128, 1, 128)])
def test_analytic_dy_against_autograd(F, hid, L, H):
    """dL/dlogits = (beta / Bg)(p Qs - q') + p (dp - dot), exactly 0 on inactive rows, for B_global = B and above, with and
    without the entropy term, clipped and unclipped states; column 0 is the sum of the per-state terms."""
    rng = np.random.default_rng(F + hid + L + H)
    B = 12
    c = _anchor_case(rng, B, H, F, hid, L)
    args = (c["active"], c["actions"], c["p_old"], c["adv"], EPS, c["q"])
    for Bg, ew, coef in ((B, 0.0, 0.75), (3 * B, 0.0, 2.5), (B, 0.01, 0.0)):
        r = ref.loss_grad(c["params"], F, hid, L, c["states"], *args, coef, ew, B_global=Bg, chunk=5, want_dy=True)
        ana = ref.analytic_dy(c["logits"], *args, coef, H, ew, Bg)
        assert np.all(np.isfinite(r["grad"])) and np.all(np.isfinite(r["dy"]))
        assert np.abs(r["dy"] - ana).max() <= 1e-13 * max(1.0, np.abs(ana).max())
        assert np.all(r["dy"][~ref.row_mask(c["active"], H)] == 0.0) and np.all(ana[~ref.row_mask(c["active"], H)] == 0.0)
        t0, t1, ratio, kl = ref.per_state_terms(c["logits"], *args, coef, H)
        assert abs(r["loss"] - -t0.sum() / Bg) <= 1e-12 * max(1.0, abs(r["loss"]))
        assert abs(r["entropy"] - ew * -t1.sum() / Bg) <= 1e-12 * max(1.0, abs(r["entropy"]))
        assert np.abs(r["kl"] - kl).max() <= 1e-12 * max(1.0, kl.max()) and np.abs(r["ratio"] - ratio).max() <= 1e-12
    p_sel = ratio * c["p_old"]
    _, un = ref.surrogate(p_sel, c["p_old"], c["adv"], EPS)
    assert un.any() and (~un).any(), "both sides of the clip occur"


def test_the_two_halves_are_the_existing_objectives():
    """coef = 0: the gradient has no anchor part and column 0 is the surrogate.  Zero advantages: loss, dL/dlogits and gradient
    are distill_ref's with every weight equal to coef."""
    rng = np.random.default_rng(11)
    B, H, F, hid, L = 10, 32, 72, 128, 2
    c = _anchor_case(rng, B, H)
    args = (c["active"], c["actions"], c["p_old"])
    r0 = ref.loss_grad(c["params"], F, hid, L, c["states"], *args, c["adv"], EPS, c["q"], 0.0, 0.01)
    rz = ref.loss_grad(c["params"], F, hid, L, c["states"], *args, c["adv"], EPS, np.zeros_like(c["q"]), 5.0, 0.01)
    assert r0["loss"] == r0["surrogate"] and np.abs(r0["grad"] - rz["grad"]).max() <= 1e-15
    zero = np.zeros(B)
    for coef, Bg, ew in ((0.75, B, 0.01), (2.5, 3 * B, 0.0)):
        r = ref.loss_grad(c["params"], F, hid, L, c["states"], *args, zero, EPS, c["q"], coef, ew, B_global=Bg)
        ce, ent, g = distill_ref.loss_grad(c["params"], F, hid, L, c["states"], c["active"], c["q"], np.full(B, coef), ew, B_global=Bg)
        assert abs(r["loss"] - ce) <= 1e-14 * max(1.0, abs(ce)) and abs(r["entropy"] - ent) <= 1e-14 * max(1.0, abs(ent))
        assert np.abs(r["grad"] - g).max() <= 1e-14 * np.abs(g).max() and r["surrogate"] == 0.0
        a = ref.analytic_dy(c["logits"], *args, zero, EPS, c["q"], coef, H, ew, Bg)
        d = distill_ref.analytic_dy(c["logits"], c["active"], c["q"], np.full(B, coef), H, ew, Bg)
        assert np.abs(a - d).max() <= 1e-16


def test_divergence_is_a_divergence():
    """kl >= 0 for normalised rows on fully active states, 0 for q = pi, and the cross-entropy minus the targets' entropy; on
    a row that lost mass to the mask or sums to less than 1 it is the stated sum and may be negative."""
    rng = np.random.default_rng(12)
    B, H = 16, 32
    logits = rng.normal(size=(B, 4 * H)) * 3
    full = np.full(B, 2 ** (H // 4) - 1, np.uint32)
    e = np.exp(rng.normal(size=(B, 4 * H)) * 2)
    q = e / e.sum(axis=1, keepdims=True)
    kl = ref.state_kl(logits, full, q, H)
    assert (kl > 0).all()
    logp, p = ref.log_probs_np(logits, ref.action_mask(full, H))
    assert np.abs(ref.state_kl(logits, full, p, H)).max() <= 1e-14
    assert np.abs(kl - (-(q * logp).sum(axis=1) - -(q * np.log(q)).sum(axis=1))).max() <= 1e-12
    _, _, active, _, _ = _case(rng, B, H)
    qk = target_kinds(rng, active, H)
    k2 = ref.state_kl(logits, active, qk, H)
    assert np.all(np.isfinite(k2)) and k2[4] == 0.0, "an all-zero row has divergence 0"
    onehot = np.flatnonzero((qk > 0).sum(axis=1) == 1)
    lp2, _ = ref.log_probs_np(logits, ref.action_mask(active, H))
    for b in onehot:
        assert abs(k2[b] - -lp2[b, np.argmax(qk[b])]) <= 1e-12, "a one-hot row: -log pi(a)"


# ---------------------------------------------------------------- the host mirror
@pytest.mark.parametrize("H", [32, 128])
def test_anchored_loss_mirror_against_the_reference(ppo, H):
    """anchored_ppo_loss (numpy float32) against the float64 restatement: both mask forms, every kind of row, a row whose mass
    sits where exp(l - m) underflows.  Bound: distillation_loss's 2^-21 max(1, max|logp|) max(1, coef) for the anchor half (see
    tests/test_distill_host.py) plus 2^-21 max|gain| for the surrogate, a quotient and a product of float32 numbers."""
    rng = np.random.default_rng(H)
    B = 15
    c = _anchor_case(rng, B, H)
    logits = (rng.normal(size=(B, 4 * H)) * 3).astype(np.float32)
    mask = ref.action_mask(c["active"], H)
    ok = np.flatnonzero(mask[5])
    logits[5, :] -= 200.0
    logits[5, ok[0]] += 200.0
    c["q"][5] = 0
    c["q"][5, ok[1:]] = 1.0 / len(ok[1:])
    c["actions"][5] = ok[0]
    _, p = ref.log_probs_np(logits, mask)
    p_old = (p[np.arange(B), c["actions"]] / np.array([0.7, 0.95, 1.05, 1.4])[np.arange(B) % 4]).astype(np.float32)
    logp, _ = ref.log_probs_np(logits, mask)
    big = np.abs(np.where(mask, logp, 0)).max()
    assert big > 190
    for coef in (0.0, 0.75, 2.5):
        t0, _, ratio, kl = ref.per_state_terms(logits, c["active"], c["actions"], p_old, c["adv"], EPS, c["q"], coef, H)
        want = -t0.mean()
        bound = 2.0 ** -21 * (max(1.0, big) * max(1.0, coef) + np.abs(ratio * c["adv"]).max())
        got = ppo.anchored_ppo_loss(logits, c["active"], c["actions"], p_old, c["adv"], EPS, c["q"], coef)
        got2, gkl = ppo.anchored_ppo_loss(logits, mask, c["actions"], p_old, c["adv"], EPS, c["q"], coef, kl=True)
        assert np.isfinite(got) and got == got2
        assert abs(got - want) <= bound, (got, want, bound)
        assert abs(gkl - kl.mean()) <= 2.0 ** -21 * max(1.0, big), (gkl, kl.mean())
    # the divergence: at least 0 for normalised rows on fully active states, 0 at pi == q
    full = np.full(B, 2 ** (H // 4) - 1, np.uint32)
    e = np.exp(rng.normal(size=(B, 4 * H)))
    qn = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    a0 = np.zeros(B, np.int64)
    one = np.ones(B, np.float32)
    _, k = ppo.anchored_ppo_loss(logits, full, a0, one, one, EPS, qn, 1.0, kl=True)
    assert k > 0
    _, k = ppo.anchored_ppo_loss(np.log(qn), full, a0, one, one, EPS, qn, 1.0, kl=True)
    assert abs(k) <= 2.0 ** -18
    for bad in (np.full_like(qn, np.nan), -qn, qn[:, :5]):
        with pytest.raises(ppo.PPOError):
            ppo.anchored_ppo_loss(logits, full, a0, one, one, EPS, bad, 1.0)


# ---------------------------------------------------------------- the coefficient rule
def test_coefficient_rule(ppo):
    """Doubling, halving and holding on hand-made sequences, the restatement and the host mirror alike; across ranks the rule
    reads ONE mean, that of the union, so ranks whose own means lie on different sides of the thresholds move together."""
    d = 0.01
    for rule in (ref.adapt_coef, ppo.adapt_kl_coef):
        assert rule(1.0, 0.0151, d) == 2.0 and rule(1.0, 0.015, d) == 1.0            # above 1.5 d, not at it
        assert rule(1.0, 0.0066, d) == 0.5 and rule(1.0, d / 1.5, d) == 1.0          # below d / 1.5, not at it
        assert rule(1.0, 0.01, d) == 1.0 and rule(3.0, 100.0, 0.0) == 3.0            # inside the band; no target: fixed
        assert rule(1.0, float("nan"), d) == 1.0
        coef, seen = 1.0, []
        for kl in (0.05, 0.03, 0.012, 0.004, 0.001, 0.009):
            coef = rule(coef, kl, d)
            seen.append(coef)
        assert seen == [2.0, 4.0, 4.0, 2.0, 1.0, 1.0]
        assert rule(0.0, 1.0, d) == 0.0, "a zero coefficient stays zero"
    # two ranks, 30 and 10 states: sums 0.6 and 0.02 -> the union's mean 0.0155 doubles; per rank 0.02 would double and 0.002 halve
    sums, ns = (0.6, 0.02), (30, 10)
    union = sum(sums) / sum(ns)
    assert ppo.adapt_kl_coef(1.0, union, d) == 2.0
    assert [ppo.adapt_kl_coef(1.0, s / n, d) for s, n in zip(sums, ns)] == [2.0, 0.5]
    assert ppo.adapt_kl_coef(1e308, 1.0, d) == 1e308, "doubling never leaves the finite numbers"


def test_check_kl_anchor(ppo):
    assert ppo.check_kl_anchor((0.5, "column")) == (0.5, 0, 0.0)
    assert ppo.check_kl_anchor([2, "recorded", 0.01]) == (2.0, 1, 0.01)
    assert ppo.check_kl_anchor((0.0, "column", 0.0)) == (0.0, 0, 0.0)
    for bad, status in (((1.0,), -1), ((1.0, "column", 0.0, 1), -1), ("column", -1), ((-1.0, "column"), -1), ((float("nan"), "column"), -1),
                        ((float("inf"), "column"), -1), ((1.0, "column", -0.1), -1), ((1.0, "column", float("inf")), -1),
                        ((1.0, "teacher"), -4), ((1.0, 0), -4)):
        with pytest.raises(ppo.PPOError) as e:
            ppo.check_kl_anchor(bad)
        assert e.value.status == status, bad
    assert ppo.ANCHOR_SOURCES == tuple(sorted(ppo.DISTILL_TARGETS, key=ppo.DISTILL_TARGETS.get))


# ---------------------------------------------------------------- the route
def _check_anchor_routes(ppo):
    seen = set()
    for (dtype, F, hid, L, Q, compact) in SHAPES:
        H = 4 * Q
        for B in SIZES:
            got = anchor_route(ppo, dtype, F, hid, L, H, compact, B)
            if dtype == "bf16":
                assert got == ("none", NO_BF16_ANCHOR), (F, hid, L, Q, compact, B, got)
                continue
            dfwd, dbwd = distill_route(ppo, dtype, F, hid, L, H, compact, B)
            if dfwd == "none":
                assert got == ("none", dbwd), (F, hid, L, Q, compact, B, got)
                continue
            want_fwd = "k_policy_fwd<%d,%d,%d,%d,%d>" % (F, hid, 21 if compact else 20, H // 32, int(L != 2))
            assert got == (want_fwd, dbwd), (F, hid, L, Q, compact, B, got, dbwd)
            seen.add(dbwd.split("<")[0])
    return seen


def test_anchor_route(knobs):
    """Forward: always k_policy_fwd in an anchored mode (20: rows through idx, 21: snapshots through idx), at every minibatch
    size.  Backward: distillation's, i.e. what the policy would take at that shape and size.  A bf16-dtype policy is refused
    with a message of its own.  The plain objective's routes are what they were."""
    P = knobs
    plain = {(s, B): route(P, s[0], s[1], s[2], s[3], 4 * s[4], s[5], B) for s in SHAPES for B in SIZES}
    seen = _check_anchor_routes(P)
    assert {"k_policy_bwd_x6", "k_policy_bwd_data", "k_policy_bwd_data_deep"} <= seen, seen
    assert anchor_route(P, "f32", 72, 256, 2, 32, False, 4096) == ("k_policy_fwd<72,256,20,1,0>", "k_policy_bwd_x6<72,256>")
    P.set_train_tile_max_tiles(512)
    _check_anchor_routes(P)
    assert anchor_route(P, "f32", 72, 128, 2, 32, False, 256) == ("k_policy_fwd<72,128,20,1,0>", "k_policy_bwd_data<72,128>")
    P.set_train_tile_max_tiles(None)
    P.set_bwd_split_bf16(0)
    assert "k_policy_bwd" in _check_anchor_routes(P)
    assert anchor_route(P, "f32", 72, 256, 2, 32, False, 385) == ("k_policy_fwd<72,256,20,1,0>", "k_policy_bwd<72,256>")
    P.set_bwd_split_bf16(None)
    assert anchor_route(P, "f32", 72, 128, 3, 32, True, 64) == ("k_policy_fwd<72,128,21,1,1>", "k_policy_bwd_data_deep<72,128>")
    assert anchor_route(P, "f32", 72, 256, 4, 128, False, 4096) == ("k_policy_fwd<72,256,20,4,1>", "k_policy_bwd_data_deep<72,256>")
    assert plain == {(s, B): route(P, s[0], s[1], s[2], s[3], 4 * s[4], s[5], B) for s in SHAPES for B in SIZES}
    assert route(P, "f32", 72, 256, 2, 32, False, 4096)[0].startswith("k_policy_fwd_train_x6"), "the headline keeps its x6 pair"
    assert distill_route(P, "f32", 72, 256, 2, 32, False, 4096)[0] == "k_policy_fwd<72,256,17,1,0>"


# ---------------------------------------------------------------- the surface
def test_three_functions_declared_bound_exported(ppo):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppo_hip.h")).read(), flags=re.S)
    jl = open(os.path.join(ROOT, "julia", "ProximalPolicyOptimizationHIP.jl")).read()
    L = ppo._lib.lib()
    for name in THREE:
        m = re.search(r"int32_t\s+%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
        assert m, "%s is not declared in include/ppo_hip.h" % name
        assert len(ppo._lib.SIGNATURES[name]) == m.group(1).count(",") + 1, name
        assert hasattr(L, name), "%s is not exported by libppo_hip.so" % name
        assert "(:%s, LIB)" % name in jl, "%s has no ccall in the Julia shim" % name
    assert re.search(r"#define\s+PPO_ANCHOR_OFF\s+\(-1\)", src) and ppo.ANCHOR_OFF == -1
    assert "function set_kl_anchor!" in jl and "function last_anchor_stats" in jl and "function kl_anchor" in jl
    # the signatures the issue froze
    for name, n in (("ppo_train", 17), ("ppo_forward_backward", 8), ("ppo_step_batch", 10), ("ppo_policy_last_train_stats", 7)):
        assert len(ppo._lib.SIGNATURES[name]) == n, name
    assert isinstance(ppo.HipPolicy.kl_anchor, property) and callable(ppo.HipPolicy.last_anchor_stats)


def test_refusals_without_a_device(ppo):
    L = ppo._lib.lib()
    p = ppo._lib
    f64 = np.zeros(1, np.float64)
    i32 = np.zeros(1, np.int32)
    # the arguments are judged before the handle
    for coef, source, target, status, text in ((-1.0, 0, 0.0, -1, "coefficient"), (float("nan"), 0, 0.0, -1, "coefficient"),
                                               (float("inf"), 1, 0.0, -1, "coefficient"), (1.0, 0, -1.0, -1, "target"),
                                               (1.0, 1, float("nan"), -1, "target"), (1.0, 2, 0.0, -4, "unknown target source"),
                                               (1.0, -2, 0.0, -4, "unknown target source"), (1.0, 0, 0.0, -1, "null"),
                                               (0.0, -1, 0.0, -1, "null")):
        assert L.ppo_policy_set_kl_anchor(None, coef, source, target) == status, (coef, source, target)
        assert text in p.last_error(), p.last_error()
    assert L.ppo_policy_get_kl_anchor(None, f64.ctypes.data_as(p.c_f64p), i32.ctypes.data_as(p.c_i32p), f64.ctypes.data_as(p.c_f64p)) == -1
    assert "null" in p.last_error()
    assert L.ppo_policy_last_anchor_stats(None, 0, i32.ctypes.data_as(p.c_i32p), None, None) == -1 and "null" in p.last_error()


class _Evaluator:
    pass


class _Anchored:
    def __init__(self, anchor):
        self.kl_anchor = anchor
        self.target_kl = None


def test_ppo_iterate_takes_anchor_and_nothing_else(ppo):
    args = (None, None, None, 8, 8, 0, _Evaluator(), 1, 0.99, 0.05, 0.01)
    today = ppo.ppo_iterate_(*args, verbose=False)
    assert today == {"ppo": [], "entropy": [], "lr": []}, "policy = None, zero iterations: the three-key dict"
    assert ppo.ppo_iterate_(*args, verbose=False, anchor=None) == today
    assert ppo.ppo_iterate_(*args, verbose=False, parallel=None, bootstrap_truncated=True, anchor=None) == today
    for bad in ({"paralel": None}, {"bootstrap": True}, {"anchors": None}, {"anchor": None, "teacher": None},
                {"bootstrap_truncated": True, "bootstrap_truncate": True}):
        with pytest.raises(TypeError, match="unexpected keyword argument"):
            ppo.ppo_iterate_(*args, verbose=False, **bad)
    teacher = object()
    # before anything runs (zero iterations would run nothing anyway; the evaluator of a first iteration is never called)
    for policy, status, text in ((None, -1, "kl_anchor"), (_Anchored(None), -1, "kl_anchor"), (_Anchored((1.0, "recorded", 0.0)), -4, "column")):
        with pytest.raises(ppo.PPOError, match=text) as e:
            ppo.ppo_iterate_(policy, None, None, 8, 8, 3, None, 1, 0.99, 0.05, 0.01, verbose=False, anchor=teacher)
        assert e.value.status == status
    with pytest.raises(ppo.PPOError, match="disk-backed"):
        ppo.ppo_iterate_(_Anchored((1.0, "column", 0.0)), None, None, 8, 8, 0, None, 1, 0.99, 0.05, 0.01, "/nonexistent", False, anchor=teacher)
    got = ppo.ppo_iterate_(_Anchored((1.0, "column", 0.0)), None, None, 8, 8, 0, _Evaluator(), 1, 0.99, 0.05, 0.01, verbose=False,
                           anchor=teacher)
    assert got == dict(today, anchor_kl=[], anchor_coef=[])


# ---------------------------------------------------------------- the loss bar of the GPU tests
def test_float32_restatement_sets_the_loss_bar(ppo):
    """tests/test_gpu_anchor.py holds loss terms, loss scalars, ratios and per-state divergences to LOSS_BAR: four times the
    largest error of the numpy-float32 restatement over the cases of its tests 1 and 2, rounded up to one digit.  Measured here,
    on the CPU; TEST_RECORD_DIR=<dir> writes the measurement to <dir>/kl_anchor.jsonl beside the device's own errors."""
    import test_gpu_anchor as g
    worst = g.measure_loss_bar(ppo)
    top = max(max(v.values()) for v in worst.values())
    exp = math.floor(math.log10(4 * top))
    bar = math.ceil(4 * top / 10 ** exp - 1e-9) * 10 ** exp
    g._record({"case": "loss_bar_measurement", "numpy_f32_worst": worst, "four_times": 4 * top, "rounded_up": bar, "LOSS_BAR": g.LOSS_BAR})
    # (numpy's float32 exp and log may differ by an ulp between builds: the bar must cover four times the measurement and lie
    # within the step the rounding to one digit takes here, 8.3e-6 -> 9e-6)
    assert 4 * top <= g.LOSS_BAR <= 4.5 * top, (top, bar, g.LOSS_BAR)
