"""The distillation (soft-target cross-entropy) objective as far as a machine without a GPU can see it: the float64
restatement (tests/distill_ref.py) held against itself and against the imitation restatement, the numpy host mirror
distillation_loss against it, set_action_targets' checks, the route (csrc/ppo_route.hip through ppo_debug_distill_route), the
entry points declared, bound and exported, and the refusals that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import distill_ref as ref
import imitation_ref
from test_imitation_host import _case, imitate_route
from test_train_route import DTYPE, ERR_UNSUPPORTED, NO_COMPACT, NO_FP32, SHAPES, SIZES, route

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIVE = ("ppo_rollouts_fill_targets", "ppo_rollouts_set_targets", "ppo_rollouts_get_targets", "ppo_distill_forward_backward",
        "ppo_distill_train")
NO_BF16_STUDENT = "distillation into a bf16-dtype student is not supported: the distillation modes exist in the fp32-MFMA forward only"


def distill_route(ppo, dtype, F, hid, L, H, compact, states):
    lib = ppo._lib.lib()
    fn = lib.ppo_debug_distill_route
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


def target_kinds(rng, active, H):
    """Target rows [B, 4H] of every kind the rule names, by state: 0 a softmax of random scores over ALL actions (so part of the
    mass lies on inactive rows unless every quad is active), 1 one-hot on an allowed action, 2 half the mass on an inactive
    quad where there is one, 3 a row summing to 0.5, 4 an all-zero row; then round again."""
    B, A = len(active), 4 * H
    mask = ref.action_mask(active, H)
    q = np.zeros((B, A), np.float32)
    for b in range(B):
        ok, off = np.flatnonzero(mask[b]), np.flatnonzero(~mask[b])
        kind = b % 5
        if kind == 0:
            e = np.exp(rng.normal(size=A) * 2)
            q[b] = e / e.sum()
        elif kind == 1:
            q[b, rng.choice(ok)] = 1.0
        elif kind == 2:
            e = rng.random(len(ok))
            q[b, ok] = 0.5 * e / e.sum() if len(off) else e / e.sum()
            if len(off):
                q[b, off[:16]] = 0.5 / 16
        elif kind == 3:
            e = rng.random(len(ok))
            q[b, ok] = 0.5 * e / e.sum()
    return q


# ---------------------------------------------------------------- the restatement against itself
@pytest.mark.parametrize("F,hid,L,H", [(72, 128, 2, 32), (72, 64, 3, 32), (216, 128, 2, 32), (72, 128, 1, 128)])
def test_analytic_dy_against_autograd(F, hid, L, H):
    """dL/dlogits = (w / Bg)(p Qs - q') + the entropy part, exactly 0 on inactive rows, for B_global = B and B_global > B, with
    and without the entropy term, over every kind of target row; the loss is the sum of the per-state terms."""
    rng = np.random.default_rng(F + hid + L + H)
    B = 10
    params, states, active, _, w = _case(rng, B, H, F, hid, L)
    q = target_kinds(rng, active, H)
    logits = ref.logits_np(params, F, hid, L, states)
    for Bg, ew, wt in ((B, 0.0, np.ones(B)), (3 * B, 0.0, w), (B, 0.01, w)):
        ce, ent, g, dy = ref.loss_grad(params, F, hid, L, states, active, q, wt, ew, B_global=Bg, chunk=4, want_dy=True)
        ana = ref.analytic_dy(logits, active, q, wt, H, ew, Bg)
        assert np.all(np.isfinite(g)) and np.all(np.isfinite(dy)) and np.isfinite(ce) and np.isfinite(ent)
        assert np.abs(dy - ana).max() <= 1e-13 * max(1.0, np.abs(ana).max())
        assert np.all(dy[~ref.row_mask(active, H)] == 0.0) and np.all(ana[~ref.row_mask(active, H)] == 0.0)
        ce_np, ent_np = ref.losses_np(logits, active, q, wt, H, ew, Bg)
        assert abs(ce - ce_np) <= 1e-12 * max(1.0, abs(ce)) and abs(ent - ent_np) <= 1e-12 * max(1.0, abs(ent))
        assert np.abs(g).max() > 1e-4
    t0, _ = ref.per_state_terms(logits, active, q, w, H)
    assert t0[0] == 0.0 and t0[1] == 0.0 and t0[2] < 0.0, "weights 0 and -1.5 clamp to 0, weight 2 counts"


def test_rule_on_special_rows():
    """Mass on inactive rows is ignored (the same loss and gradient as with that mass removed), Qs is used as it is (a row
    scaled by c scales ce by c and the gradient is (p c Qs - c q'), not c (p - q')), an all-zero row leaves the entropy term
    alone."""
    rng = np.random.default_rng(3)
    B, H = 10, 32
    _, _, active, _, _ = _case(rng, B, H)
    logits = rng.normal(size=(B, 4 * H)) * 2
    mask = ref.action_mask(active, H)
    q = target_kinds(rng, active, H)
    w = np.ones(B)
    ew = 0.01
    # ignored mass
    qk = np.where(mask, q, 0).astype(np.float64)
    assert (q != qk).any()
    assert ref.losses_np(logits, active, q, w, H, ew) == ref.losses_np(logits, active, qk, w, H, ew)
    assert np.array_equal(ref.analytic_dy(logits, active, q, w, H, ew), ref.analytic_dy(logits, active, qk, w, H, ew))
    # unnormalised rows: the exact gradient of the stated loss, which is NOT the normalised row's gradient scaled
    _, p = ref.log_probs_np(logits, mask)
    Qs = qk.sum(axis=1)
    assert abs(Qs[3] - 0.5) < 1e-6 and Qs[4] == 0.0 and abs(Qs[1] - 1.0) < 1e-6
    dy = ref.analytic_dy(logits, active, q, w, H).reshape(B, -1)
    assert np.abs(dy - (p * Qs[:, None] - qk) / B).max() <= 1e-15
    assert np.abs(dy[3] - (p[3] - qk[3]) / B).max() > 1e-4, "assuming Qs == 1 would be another gradient"
    assert np.abs(dy.sum(axis=1)).max() <= 1e-15, "the gradient of a function of the softmax sums to 0 per state"
    # the all-zero row: only the entropy term
    t0, _ = ref.per_state_terms(logits, active, q, w, H)
    assert t0[4] == 0.0 and not dy[4].any()
    dye = ref.analytic_dy(logits, active, q, w, H, ew).reshape(B, -1)
    dy0 = ref.analytic_dy(logits, active, np.zeros_like(q), w, H, ew).reshape(B, -1)
    assert np.array_equal(dye[4], dy0[4]) and dye[4].any()
    # float64 autograd agrees on all of it
    params, states, active2, _, _ = _case(np.random.default_rng(4), B, H)
    q2 = target_kinds(np.random.default_rng(5), active2, H)
    _, _, _, dya = ref.loss_grad(params, 72, 128, 2, states, active2, q2, w, ew, want_dy=True)
    ana = ref.analytic_dy(ref.logits_np(params, 72, 128, 2, states), active2, q2, w, H, ew)
    assert np.abs(dya - ana).max() <= 1e-13 * np.abs(ana).max()


@pytest.mark.parametrize("H", [32, 128])
def test_one_hot_targets_are_behaviour_cloning(ppo, H):
    """A one-hot target row gives imitation's loss, per-state terms, dL/dlogits and gradient: in the float64 restatements to
    rounding, and in the float32 host mirrors bit for bit."""
    rng = np.random.default_rng(10 + H)
    B = 12
    params, states, active, actions, w = _case(rng, B, H)
    q = np.zeros((B, 4 * H), np.float32)
    q[np.arange(B), actions] = 1.0
    logits = ref.logits_np(params, 72, 128, 2, states)
    for wt, ew, Bg in ((np.ones(B), 0.0, B), (w, 0.02, 3 * B)):
        a = ref.per_state_terms(logits, active, q, wt, H)
        b = imitation_ref.per_state_terms(logits, active, actions, wt, H)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.abs(ref.analytic_dy(logits, active, q, wt, H, ew, Bg) - imitation_ref.analytic_dy(logits, active, actions, wt, H, ew, Bg)).max() <= 1e-16
        ce, ent, g = ref.loss_grad(params, 72, 128, 2, states, active, q, wt, ew, B_global=Bg)
        ce_i, ent_i, g_i, _ = imitation_ref.loss_grad(params, 72, 128, 2, states, active, actions, wt, ew, B_global=Bg)
        assert abs(ce - ce_i) <= 1e-14 * max(1.0, abs(ce_i)) and ent == ent_i and np.abs(g - g_i).max() <= 1e-14 * np.abs(g_i).max()
    l32 = logits.astype(np.float32)
    for weights in (None, w):
        assert ppo.distillation_loss(l32, active, q, weights) == ppo.imitation_loss(l32, active, actions, weights)


# ---------------------------------------------------------------- the host mirror
@pytest.mark.parametrize("H", [32, 128])
def test_distillation_loss_mirror_against_the_reference(ppo, H):
    """distillation_loss (numpy float32) against the float64 restatement: both mask forms, weights None / of both signs, every
    kind of row, and a row whose mass sits where exp(l - m) underflows.  Bound: 2^-21 max(1, max|logp|) max(1, max Qs) -- a
    float32 log-softmax entry is a difference of two rounded values of that size plus a rounded log (2^-22 of it, as for
    imitation_loss), and the float32 sum of up to 512 products q logp, sum q <= Qs, adds at most as much again with numpy's
    pairwise order.  The floor it reports is the targets' entropy."""
    rng = np.random.default_rng(H)
    B = 15
    _, _, active, _, w = _case(rng, B, H)
    logits = (rng.normal(size=(B, 4 * H)) * 3).astype(np.float32)
    q = target_kinds(rng, active, H)
    ok = np.flatnonzero(ref.action_mask(active, H)[5])
    logits[5, :] -= 200.0
    logits[5, ok[0]] += 200.0
    q[5] = 0
    q[5, ok[1:]] = 1.0 / len(ok[1:])                                 # all of row 5's mass where the student's exp underflows
    with np.errstate(divide="ignore"):
        assert np.exp(np.float32(-190.0)) == 0.0
    for weights in (None, w):
        w64 = np.ones(B) if weights is None else weights
        want, _ = ref.losses_np(logits, active, q, w64, H)
        logp, _ = ref.log_probs_np(logits, ref.action_mask(active, H))
        big = np.abs(np.where(ref.action_mask(active, H), logp, 0)).max()
        bound = 2.0 ** -21 * max(1.0, big) * max(1.0, np.abs(w64).max())
        got = ppo.distillation_loss(logits, active, q, weights)
        got2, floor = ppo.distillation_loss(logits, ref.action_mask(active, H), q, weights, floor=True)
        assert np.isfinite(got) and got == got2
        assert abs(got - want) <= bound, (got, want, bound)
        assert abs(floor - ref.target_entropy(q, active, w64, H)) <= 1e-12
    assert big > 190
    # normalised rows on fully active states: the cross-entropy is at least the floor, and equal to it at pi == q
    full = np.full(B, 2 ** (H // 4) - 1, np.uint32)
    e = np.exp(rng.normal(size=(B, 4 * H)))
    qn = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    loss, floor = ppo.distillation_loss(logits, full, qn, floor=True)
    assert loss > floor
    same, floor = ppo.distillation_loss(np.log(qn), full, qn, floor=True)
    assert abs(same - floor) <= 2.0 ** -18 * max(1.0, floor)
    for bad in (np.full_like(qn, np.nan), -qn, qn[:, :5]):
        with pytest.raises(ppo.PPOError):
            ppo.distillation_loss(logits, full, bad)


def test_float32_restatement_error_over_the_host_cases():
    """The figure LOSS_BAR rests on is measured by tests/test_gpu_distill.py's loss_errors over its own cases (no device
    needed); here only that the float32 switch of the restatement runs every operation in float32 and stays close."""
    rng = np.random.default_rng(8)
    B, H = 10, 32
    params, states, active, _, w = _case(rng, B, H)
    q = target_kinds(rng, active, H)
    l32 = ref.logits_np(params, 72, 128, 2, states, np.float32)
    t32 = ref.per_state_terms(l32, active, q, w, H, np.float32)
    t64 = ref.per_state_terms(ref.logits_np(params, 72, 128, 2, states), active, q, w, H)
    assert t32[0].dtype == np.float32 and t32[1].dtype == np.float32
    assert np.abs(t32[0] - t64[0]).max() <= 1e-5 * max(1.0, np.abs(t64[0]).max())


# ---------------------------------------------------------------- set_action_targets
def test_set_action_targets_refuses_bad_rows(ppo):
    """Shape, finiteness and sign are checked on the host, before the library is called (the kernel does not check them)."""
    class _Dims(ppo.BufferRollouts):
        def dims(self):
            return 2, 3

    ro = _Dims()
    with pytest.raises(ppo.PPOError, match="empty rollout buffer"):
        ro.set_action_targets(np.zeros((2, 3, 128), np.float32))
    ro._h, ro._env = object(), ppo._Shape(3, 32, 72)              # no handle: anything that reached the library would fail
    good = np.full((2, 3, 128), 1.0 / 128, np.float32)
    for bad, text in ((np.zeros((2, 3, 127), np.float32), "shape"), (np.zeros((6, 128), np.float32), "shape"),
                      (np.where(np.arange(128) == 5, np.nan, good), "finite"), (np.where(np.arange(128) == 7, np.inf, good), "finite"),
                      (np.where(np.arange(128) == 9, -1e-3, good), ">= 0")):
        with pytest.raises(ppo.PPOError, match=text) as e:
            ro.set_action_targets(bad)
        assert e.value.status == -1
    ro._h = None                                                   # nothing to destroy


# ---------------------------------------------------------------- the route
def _check_distill_routes(ppo):
    seen = set()
    for (dtype, F, hid, L, Q, compact) in SHAPES:
        H = 4 * Q
        for B in SIZES:
            got = distill_route(ppo, dtype, F, hid, L, H, compact, B)
            if dtype == "bf16":
                assert got == ("none", NO_BF16_STUDENT), (F, hid, L, Q, compact, B, got)
                continue
            ifwd, ibwd = imitate_route(ppo, dtype, F, hid, L, H, compact, B)
            if ifwd == "none":
                assert ibwd in (NO_FP32, NO_COMPACT) and got == ("none", ibwd), (F, hid, L, Q, compact, B, got)
                continue
            want_fwd = "k_policy_fwd<%d,%d,%d,%d,%d>" % (F, hid, 18 if compact else 17, H // 32, int(L != 2))
            assert got == (want_fwd, ibwd), (F, hid, L, Q, compact, B, got, ibwd)
            seen.add(ibwd.split("<")[0])
    return seen


def test_distill_route(knobs):
    """Forward: always k_policy_fwd in a distillation mode (17: rows through idx, 18: snapshots through idx).  Backward:
    imitation's, i.e. what the policy would take at that shape and size.  A bf16-dtype student is refused with a message of
    its own."""
    P = knobs
    seen = _check_distill_routes(P)
    assert {"k_policy_bwd_x6", "k_policy_bwd_data", "k_policy_bwd_data_deep"} <= seen, seen
    assert distill_route(P, "f32", 72, 256, 2, 32, False, 4096) == ("k_policy_fwd<72,256,17,1,0>", "k_policy_bwd_x6<72,256>")
    P.set_train_tile_max_tiles(512)
    _check_distill_routes(P)
    assert distill_route(P, "f32", 72, 128, 2, 32, False, 256) == ("k_policy_fwd<72,128,17,1,0>", "k_policy_bwd_data<72,128>")
    P.set_train_tile_max_tiles(None)
    P.set_bwd_split_bf16(0)
    assert "k_policy_bwd" in _check_distill_routes(P)
    assert distill_route(P, "f32", 72, 256, 2, 32, False, 385) == ("k_policy_fwd<72,256,17,1,0>", "k_policy_bwd<72,256>")
    assert distill_route(P, "f32", 72, 256, 2, 32, False, 384) == ("k_policy_fwd<72,256,17,1,0>", "k_policy_bwd_data<72,256>")
    P.set_bwd_split_bf16(None)
    assert distill_route(P, "f32", 72, 128, 3, 32, True, 64) == ("k_policy_fwd<72,128,18,1,1>", "k_policy_bwd_data_deep<72,128>")
    assert distill_route(P, "f32", 72, 256, 4, 128, False, 4096) == ("k_policy_fwd<72,256,17,4,1>", "k_policy_bwd_data_deep<72,256>")
    assert distill_route(P, "bf16", 72, 256, 2, 32, False, 4096) == ("none", NO_BF16_STUDENT)
    assert distill_route(P, "f32", 216, 128, 2, 32, True, 64) == ("none", NO_COMPACT)
    # the other objectives' routes are what they were
    assert route(P, "f32", 72, 256, 2, 32, False, 4096)[0].startswith("k_policy_fwd_train_x6")
    assert imitate_route(P, "f32", 72, 256, 2, 32, False, 4096)[0] == "k_policy_fwd<72,256,12,1,0>"


# ---------------------------------------------------------------- the surface
def test_five_functions_declared_bound_exported(ppo):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppo_hip.h")).read(), flags=re.S)
    jl = open(os.path.join(ROOT, "julia", "ProximalPolicyOptimizationHIP.jl")).read()
    L = ppo._lib.lib()
    for name in FIVE:
        m = re.search(r"int32_t\s+%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
        assert m, "%s is not declared in include/ppo_hip.h" % name
        assert len(ppo._lib.SIGNATURES[name]) == m.group(1).count(",") + 1, name
        assert hasattr(L, name), "%s is not exported by libppo_hip.so" % name
    for name in ("ppo_rollouts_fill_targets", "ppo_distill_forward_backward", "ppo_distill_train"):
        assert "(:%s, LIB)" % name in jl, "%s has no ccall in the Julia shim" % name
    assert re.search(r"#define\s+PPO_TARGETS_COLUMN\s+0", src) and re.search(r"#define\s+PPO_TARGETS_RECORDED\s+1", src)
    assert ppo.DISTILL_TARGETS == {"column": 0, "recorded": 1}
    assert "function fill_targets!" in jl and "function distill_train!" in jl and "function distill_forward_backward" in jl
    assert hasattr(ppo.BufferRollouts, "action_targets") and hasattr(ppo.BufferRollouts, "set_action_targets")


def test_refusals_without_a_device(ppo):
    L = ppo._lib.lib()
    p = ppo._lib
    i64 = np.zeros(1, np.int64)
    f32 = np.zeros(1, np.float32)
    f64 = np.zeros(1, np.float64)
    assert L.ppo_rollouts_fill_targets(None, None) == -1 and "null" in p.last_error()
    assert L.ppo_rollouts_set_targets(None, f32.ctypes.data_as(p.c_f32p)) == -1 and "null" in p.last_error()
    assert L.ppo_rollouts_get_targets(None, f32.ctypes.data_as(p.c_f32p)) == -1 and "null" in p.last_error()
    assert L.ppo_distill_forward_backward(None, None, i64.ctypes.data_as(p.c_i64p), 1, 1, 0.0, 0, 0, 0) == -1
    assert "null" in p.last_error()
    assert L.ppo_distill_train(None, None, None, 1, 1, 0.0, 0, 0, 0, None, 0, 0, 1, p.ALLREDUCE_FN(0), None, f64.ctypes.data_as(p.c_f64p),
                               f64.ctypes.data_as(p.c_f64p), f64.ctypes.data_as(p.c_f64p)) == -1
    assert "null" in p.last_error()
    # unknown weights / target sources and the normalised advantage modes never reach the library from the mirror
    for kw in (dict(weights="softmax"), dict(advantage="returns_normalised"), dict(weights="positive_advantage", advantage="gae_normalised"),
               dict(targets="search")):
        for fn in (lambda: ppo.distill_forward_backward(None, None, [1], **kw), lambda: ppo.distill_train_(None, None, None, 1, 1, **kw)):
            with pytest.raises(ppo.PPOError) as e:
                fn()
            assert e.value.status == ERR_UNSUPPORTED, kw
    with pytest.raises(ppo.PPOError, match="advantage must be one of"):
        ppo.distill_forward_backward(None, None, [1], advantage="td0")
    with pytest.raises(ppo.PPOError) as e:
        ppo.fill_targets_(ppo.BufferRollouts(), None)
    assert e.value.status == ERR_UNSUPPORTED
