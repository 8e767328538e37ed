"""The critic's PPO-clipped value loss, as far as a machine without a GPU can see it: the three entry points (include/ppo_hip.h
"critic: PPO-clipped value loss") are declared, bound, exported and ccall'ed; the float64 restatement (tests/value_clip_ref.py)
holds its analytic dL/dy against its own autograd; the plain-numpy mirror value_loss_clipped against float64; and the argument
checks that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import value_clip_ref
import value_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREE = ("ppo_policy_set_value_clip", "ppo_policy_get_value_clip", "ppo_policy_last_value_stats")


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
    assert hasattr(L, "ppo_debug_value_deltas") and "ppo_debug_value_deltas" not in src
    for fn in ("function set_value_clip!(", "function value_clip(", "function last_value_stats("):
        assert fn in jl, fn
    assert isinstance(ppo.HipPolicy.value_clip, property) and callable(ppo.HipPolicy.last_value_stats)
    assert "value_loss_clipped" in ppo.__all__


def _case(rng, B, H, F=72):
    states = rng.integers(-3, 7, size=(B, H, F)).astype(np.int8)
    active = rng.integers(0, 2 ** (H // 4), size=B, dtype=np.uint64).astype(np.uint32)
    active[0] = 0                                                     # a state with no active quad
    active[1] = 2 ** (H // 4) - 1                                     # and a fully active one
    return states, active


@pytest.mark.parametrize("F,hid,L,H", [(72, 128, 2, 32), (72, 64, 3, 32), (216, 128, 2, 32), (72, 128, 1, 128)])
def test_analytic_dy_against_autograd(ppo, F, hid, L, H):
    """dL/dy of the clipped loss = the mse's 2 (V - t) / (B_global 4 n_rows) on the states that keep the unclipped square and
    exactly 0 on the clipped-away ones, for B_global = B and B_global > B, with every regime present; the loss is the sum of
    the larger squares."""
    rng = np.random.default_rng(F + hid + L + H)
    B, c = 12, 0.5
    params = ppo.glorot_uniform_params(F, hid, L, 4, seed=3) + (rng.normal(size=ppo.glorot_uniform_params(F, hid, L, 4).size) * 0.02).astype(np.float32)
    states, active = _case(rng, B, H, F)
    v64 = value_ref.values_np(params, F, hid, L, states, active)
    v_old, t, regime = value_clip_ref.make_regimes(rng, v64, c)
    b = value_clip_ref.check_margins(v64, v_old, t, c, regime)
    for Bg in (B, 3 * B):
        loss, g, v, dy = value_clip_ref.loss_grad(params, F, hid, L, states, active, t, v_old, c, B_global=Bg, chunk=5, want_dy=True)
        ana = value_clip_ref.analytic_dy(v, active, t, v_old, c, Bg, H)
        assert np.all(np.isfinite(g)) and np.all(np.isfinite(dy)) and np.isfinite(loss)
        assert np.abs(dy - ana).max() <= 1e-14 * max(1.0, np.abs(ana).max())
        assert np.abs(v - v64).max() <= 1e-12
        assert not dy[regime == value_clip_ref.CLIPPED].any() and not dy[0].any()
        live = (regime != value_clip_ref.CLIPPED) & (active != 0)
        assert all(dy[i].any() for i in np.flatnonzero(live))
        assert np.all(dy[~value_ref.row_mask(active, H)] == 0.0)
        assert abs(loss - float((b["term"] ** 2).sum() / Bg)) <= 1e-12 * max(1.0, loss)
        assert abs(loss - float(np.maximum(b["d"] ** 2, b["dc"] ** 2).sum() / Bg)) <= 1e-12 * max(1.0, loss)
        assert np.abs(g).max() > 1e-4
    # a clip nothing reaches is the mse
    l0, g0, _ = value_ref.loss_grad(params, F, hid, L, states, active, t)
    l1, g1, _ = value_clip_ref.loss_grad(params, F, hid, L, states, active, t, v_old, 1e30)
    assert abs(l0 - l1) <= 1e-12 * max(1.0, l0) and np.abs(g0 - g1).max() <= 1e-12 * np.abs(g0).max()


def test_value_loss_clipped_against_float64(ppo):
    rng = np.random.default_rng(7)
    B = 300
    v = (rng.normal(size=B) * 2).astype(np.float32)
    for c in (0.5, float(np.float32(0.2))):
        v_old, t, regime = value_clip_ref.make_regimes(rng, v.astype(np.float64), c)
        b = value_clip_ref.check_margins(v.astype(np.float64), v_old, t, c, regime)
        l64 = float(np.mean(b["term"] ** 2))
        got = ppo.value_loss_clipped(v, v_old, t, c)
        assert abs(got - l64) <= 1e-6 * max(1.0, l64)
        assert got > ppo.value_loss(v, t)                             # some state's clipped square is the larger one
        assert ppo.value_loss_clipped(v, v_old, t, None) == ppo.value_loss(v, t)
        assert ppo.value_loss_clipped(v, v_old, t, float("inf")) == ppo.value_loss(v, t)
        assert ppo.value_loss_clipped(v, v_old, t, 1e30) == ppo.value_loss(v, t)
    # a tie of the two squares keeps the unclipped one; the decision is made on V - V_old, not on a re-formed V
    assert ppo.value_loss_clipped([1.0], [0.0], [0.75], 0.5) == 0.0625
    assert ppo.value_loss_clipped([1.0], [0.0], [1.0], 0.5) == 0.25
    assert ppo.value_loss_clipped([1.0], [0.0], [0.0], 0.5) == 1.0


def test_argument_checks_without_a_device(ppo):
    L = ppo._lib.lib()
    p = ppo._lib
    f64 = np.zeros(1, np.float64)
    i32 = np.zeros(1, np.int32)
    assert L.ppo_policy_set_value_clip(None, 0.2) == -1
    assert "null" in p.last_error()
    assert L.ppo_policy_get_value_clip(None, f64.ctypes.data_as(p.c_f64p)) == -1
    assert "null" in p.last_error()
    assert L.ppo_policy_last_value_stats(None, 1, i32.ctypes.data_as(p.c_i32p), f64.ctypes.data_as(p.c_f64p), f64.ctypes.data_as(p.c_f64p)) == -1
    assert "null" in p.last_error()
    L.ppo_debug_value_deltas.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.ppo_debug_value_deltas.restype = C.c_int32
    assert L.ppo_debug_value_deltas(None, 1, np.zeros(1, np.float32).ctypes.data) == -1
    # the range is checked in front of the handle
    for bad in (-0.1, float("nan"), float("-inf")):
        assert L.ppo_policy_set_value_clip(None, bad) == -1
        assert "value_clip must be 0 (off), positive or +inf" in p.last_error()


def test_setter_refuses_negative_and_nan_through_the_mirror(ppo):
    pol = object.__new__(ppo.HipPolicy)                               # no device: the mirror refuses before the library is asked
    pol._h = None
    for bad in (-1.0, -1e-30, float("nan"), float("-inf")):
        with pytest.raises(ppo.PPOError, match="value_clip must be None"):
            pol.value_clip = bad
