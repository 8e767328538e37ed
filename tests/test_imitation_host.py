"""The imitation (behaviour-cloning) objective as far as a machine without a GPU can see it: the float64 restatement
(tests/imitation_ref.py) held against itself, the numpy host mirror imitation_loss against it, the route
(csrc/ppo_route.hip through ppo_debug_imitate_route: the imitation forward paired with the backward train_route picks), the
two entry points declared, bound and exported, and the refusals that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import imitation_ref as ref
from test_train_route import DTYPE, ERR_UNSUPPORTED, NO_COMPACT, NO_FP32, SHAPES, SIZES, route

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO = ("ppo_imitate_forward_backward", "ppo_imitate_train")
NO_BF16_IMITATE = "imitation training of a bf16-dtype policy is not supported: the imitation modes exist in the fp32-MFMA forward only"


def imitate_route(ppo, dtype, F, hid, L, H, compact, states):
    lib = ppo._lib.lib()
    fn = lib.ppo_debug_imitate_route
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


def _case(rng, B, H, F=72, hid=128, L=2):
    """States, masks (all quads, only the first, only the last, random), an allowed action per state, weights of both signs."""
    Q = H // 4
    params = (rng.normal(size=F * hid + hid + (L - 1) * (hid * hid + hid) + 4 * hid + 4) * 0.05).astype(np.float32)
    states = rng.integers(-3, 7, size=(B, H, F)).astype(np.int8)
    active = rng.integers(1, 2 ** Q, size=B, dtype=np.uint64).astype(np.uint32)
    active[0], active[1], active[2] = 2 ** Q - 1, 1, 1 << (Q - 1)
    mask = ref.action_mask(active, H)
    actions = np.array([rng.choice(np.flatnonzero(m)) for m in mask])
    w = rng.normal(size=B).astype(np.float32)
    w[0], w[1], w[2] = 0.0, -1.5, 2.0
    return params, states, active, actions, w


# ---------------------------------------------------------------- the restatement against itself
@pytest.mark.parametrize("F,hid,L,H", [(72, 128, 2, 32), (72, 64, 3, 32), (216, 128, 2, 32), (72, 128, 1, 128)])
def test_analytic_dy_against_autograd(F, hid, L, H):
    """dL/dlogits = (w / Bg)(p - onehot) + the entropy part, exactly 0 on inactive rows, for B_global = B and B_global > B,
    with and without the entropy term; the loss is the sum of the per-state terms."""
    rng = np.random.default_rng(F + hid + L + H)
    B = 10
    params, states, active, actions, w = _case(rng, B, H, F, hid, L)
    logits = ref.logits_np(params, F, hid, L, states)
    for Bg, ew in ((B, 0.0), (3 * B, 0.0), (B, 0.01)):
        ce, ent, g, logp, dy = ref.loss_grad(params, F, hid, L, states, active, actions, w, ew, B_global=Bg, chunk=4, want_dy=True)
        ana = ref.analytic_dy(logits, active, actions, w, H, ew, Bg)
        assert np.all(np.isfinite(g)) and np.all(np.isfinite(dy)) and np.isfinite(ce) and np.isfinite(ent)
        assert np.abs(dy - ana).max() <= 1e-13 * max(1.0, np.abs(ana).max())
        assert np.all(dy[~ref.row_mask(active, H)] == 0.0) and np.all(ana[~ref.row_mask(active, H)] == 0.0)
        ce_np, ent_np = ref.losses_np(logits, active, actions, w, H, ew, Bg)
        assert abs(ce - ce_np) <= 1e-12 * max(1.0, abs(ce)) and abs(ent - ent_np) <= 1e-12 * max(1.0, abs(ent))
        t0, _ = ref.per_state_terms(logits, active, actions, w, H)
        assert np.abs(t0 - np.maximum(w.astype(np.float64), 0) * logp).max() <= 1e-12
        assert t0[0] == 0.0 and t0[1] == 0.0 and t0[2] < 0.0, "weights 0 and -1.5 clamp to 0, weight 2 counts"
        assert np.abs(g).max() > 1e-4
    # uniform weights: the plain cross-entropy
    ce1, _, _, logp1 = ref.loss_grad(params, F, hid, L, states, active, actions, np.ones(B), 0.0)
    assert abs(ce1 + logp1.mean()) <= 1e-12 * abs(ce1)


def test_underflow_case_is_finite_in_the_reference():
    """A state whose given action has a logit 200 below the maximum: softmax in fp32 gives p[a] = 0 and log(p[a]) = -inf; the
    log-softmax form gives -200 - log(S), in float64 and in the float32 restatement alike, and a finite dL/dlogits."""
    A, H = 128, 32
    l = np.zeros((1, A), np.float32)
    l[0, 0], l[0, 5] = 200.0, 1.0
    active = np.array([255], np.uint32)
    a = np.array([77])
    with np.errstate(divide="ignore"):
        e = np.exp(l - l.max(), dtype=np.float32)
        naive = np.log((e / e.sum(dtype=np.float32))[0, 77], dtype=np.float32)
    assert naive == -np.inf
    t64, _ = ref.per_state_terms(l, active, a, np.ones(1), H)
    t32, _ = ref.per_state_terms(l, active, a, np.ones(1), H, np.float32)
    want = -200.0 - np.log1p(np.exp(-199.0) + 126 * np.exp(-200.0))
    assert abs(t64[0] - want) <= 1e-12 and abs(float(t32[0]) - want) <= 200 * 2.0 ** -23
    ce, _ = ref.losses_np(l, active, a, np.ones(1), H)
    assert ce == -t64[0] and np.isfinite(ce)
    dy = ref.analytic_dy(l, active, a, np.ones(1), H)
    assert np.all(np.isfinite(dy)) and abs(dy.reshape(-1)[77] + 1.0) <= 1e-12 and abs(dy.reshape(-1)[0] - 1.0) <= 1e-12


# ---------------------------------------------------------------- the host mirror
@pytest.mark.parametrize("H", [32, 128])
def test_imitation_loss_mirror_against_the_reference(ppo, H):
    """imitation_loss (numpy float32) against the float64 restatement: both mask forms, weights None / of both signs, and the
    underflow case.  Bound: 2^-22 max(1, max|logp|) -- a float32 log-softmax is a difference of two rounded values of that
    size plus a rounded log, and the mean of B rounded terms adds at most as much again."""
    rng = np.random.default_rng(H)
    B = 12
    _, _, active, actions, w = _case(rng, B, H)
    logits = (rng.normal(size=(B, 4 * H)) * 3).astype(np.float32)
    logits[3, :] -= 200.0
    first = int(np.flatnonzero(ref.action_mask(active, H)[3])[0])
    logits[3, first] += 200.0
    if actions[3] == first:
        actions[3] = int(np.flatnonzero(ref.action_mask(active, H)[3])[1])
    for weights in (None, w):
        w64 = np.ones(B) if weights is None else weights
        want, _ = ref.losses_np(logits, active, actions, w64, H)
        t0, _ = ref.per_state_terms(logits, active, actions, np.ones(B), H)
        bound = 2.0 ** -22 * max(1.0, np.abs(t0).max()) * max(1.0, np.abs(w64).max())
        got = ppo.imitation_loss(logits, active, actions, weights)
        got2 = ppo.imitation_loss(logits, ref.action_mask(active, H), actions, weights)
        assert np.isfinite(got) and got == got2
        assert abs(got - want) <= bound, (got, want, bound)
    assert np.abs(t0).max() > 190


# ---------------------------------------------------------------- the route
def _check_imitate_routes(ppo):
    seen = set()
    for (dtype, F, hid, L, Q, compact) in SHAPES:
        H = 4 * Q
        for B in SIZES:
            got = imitate_route(ppo, dtype, F, hid, L, H, compact, B)
            if dtype == "bf16":
                assert got == ("none", NO_BF16_IMITATE), (F, hid, L, Q, compact, B, got)
                continue
            tfwd, tbwd = route(ppo, dtype, F, hid, L, H, compact, B)
            if tfwd == "none":                                       # shapes no fp32 forward covers: the same refusal
                assert tbwd in (NO_FP32, NO_COMPACT) and got == ("none", tbwd), (F, hid, L, Q, compact, B, got)
                continue
            want_fwd = "k_policy_fwd<%d,%d,%d,%d,%d>" % (F, hid, 13 if compact else 12, H // 32, int(L != 2))
            want_bwd = "k_policy_bwd_data<72,%d>" % hid if tbwd.startswith("k_policy_wgrad") else tbwd
            assert got == (want_fwd, want_bwd), (F, hid, L, Q, compact, B, got, tbwd)
            seen.add(tbwd.split("<")[0])
    return seen


def test_imitate_route(knobs):
    """Forward: always k_policy_fwd in an imitation mode (12: rows through idx, 13: snapshots through idx).  Backward: what
    ppo_debug_train_route reports for the same shape and size, k_policy_bwd_data where that is the one-tile pass's
    k_policy_wgrad.  A bf16-dtype policy is refused with a message of its own."""
    P = knobs
    seen = _check_imitate_routes(P)
    assert {"k_policy_bwd_x6", "k_policy_bwd_data", "k_policy_bwd_data_deep"} <= seen, seen
    # the headline shape: Fwd + the split-fp32 backward
    assert imitate_route(P, "f32", 72, 256, 2, 32, False, 4096) == ("k_policy_fwd<72,256,12,1,0>", "k_policy_bwd_x6<72,256>")
    # where the policy would take the one-tile pass: Fwd + Small
    P.set_train_tile_max_tiles(512)
    assert "k_policy_wgrad" in _check_imitate_routes(P)
    assert route(P, "f32", 72, 128, 2, 32, False, 256)[0] == "k_policy_train_tile<72,128>"
    assert imitate_route(P, "f32", 72, 128, 2, 32, False, 256) == ("k_policy_fwd<72,128,12,1,0>", "k_policy_bwd_data<72,128>")
    P.set_train_tile_max_tiles(None)
    # the split-fp32 kernels off: Fwd + Fused above 384 tiles, Fwd + Small up to there
    P.set_bwd_split_bf16(0)
    assert "k_policy_bwd" in _check_imitate_routes(P)
    assert imitate_route(P, "f32", 72, 256, 2, 32, False, 385) == ("k_policy_fwd<72,256,12,1,0>", "k_policy_bwd<72,256>")
    assert imitate_route(P, "f32", 72, 256, 2, 32, False, 384) == ("k_policy_fwd<72,256,12,1,0>", "k_policy_bwd_data<72,256>")
    P.set_bwd_split_bf16(None)
    # deep policies, compact storage
    assert imitate_route(P, "f32", 72, 128, 3, 32, True, 64) == ("k_policy_fwd<72,128,13,1,1>", "k_policy_bwd_data_deep<72,128>")
    assert imitate_route(P, "f32", 72, 256, 4, 128, False, 4096) == ("k_policy_fwd<72,256,12,4,1>", "k_policy_bwd_data_deep<72,256>")
    assert imitate_route(P, "bf16", 72, 256, 2, 32, False, 4096) == ("none", NO_BF16_IMITATE)
    assert imitate_route(P, "f32", 216, 128, 2, 32, True, 64) == ("none", NO_COMPACT)
    # the other two objectives' routes are what they were
    assert route(P, "f32", 72, 256, 2, 32, False, 4096)[0].startswith("k_policy_fwd_train_x6")


# ---------------------------------------------------------------- the surface
def test_two_functions_declared_bound_exported(ppo):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppo_hip.h")).read(), flags=re.S)
    jl = open(os.path.join(ROOT, "julia", "ProximalPolicyOptimizationHIP.jl")).read()
    L = ppo._lib.lib()
    for name in TWO:
        m = re.search(r"int32_t\s+%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
        assert m, "%s is not declared in include/ppo_hip.h" % name
        assert len(ppo._lib.SIGNATURES[name]) == m.group(1).count(",") + 1, name
        assert hasattr(L, name), "%s is not exported by libppo_hip.so" % name
        assert "(:%s, LIB)" % name in jl, "%s has no ccall in the Julia shim" % name
    assert re.search(r"#define\s+PPO_IMITATE_UNIFORM\s+0", src) and re.search(r"#define\s+PPO_IMITATE_POSITIVE_ADVANTAGE\s+1", src)
    assert ppo.IMITATION_WEIGHTS == {"uniform": 0, "positive_advantage": 1}
    assert "function imitate_train!" in jl and "function imitate_forward_backward" in jl


def test_refusals_without_a_device(ppo):
    L = ppo._lib.lib()
    p = ppo._lib
    i64 = np.zeros(1, np.int64)
    f64 = np.zeros(1, np.float64)
    assert L.ppo_imitate_forward_backward(None, None, i64.ctypes.data_as(p.c_i64p), 1, 1, 0.0, 0, 0) == -1
    assert "null" in p.last_error()
    assert L.ppo_imitate_train(None, None, None, 1, 1, 0.0, 0, 0, None, 0, 0, 1, p.ALLREDUCE_FN(0), None, f64.ctypes.data_as(p.c_f64p),
                               f64.ctypes.data_as(p.c_f64p), f64.ctypes.data_as(p.c_f64p)) == -1
    assert "null" in p.last_error()
    # unknown weights and the normalised advantage modes never reach the library from the mirror: PPO_ERR_UNSUPPORTED
    for kw in (dict(weights="softmax"), dict(advantage="returns_normalised"), dict(weights="positive_advantage", advantage="gae_normalised")):
        for fn in (lambda: ppo.imitate_forward_backward(None, None, [1], **kw), lambda: ppo.imitate_train_(None, None, None, 1, 1, **kw)):
            with pytest.raises(ppo.PPOError) as e:
                fn()
            assert e.value.status == ERR_UNSUPPORTED, kw
    # an advantage name nobody knows is the policy's own assertion
    with pytest.raises(ppo.PPOError, match="advantage must be one of"):
        ppo.imitate_forward_backward(None, None, [1], advantage="td0")
