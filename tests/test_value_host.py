"""The device critic, as far as a machine without a GPU can see it: the five entry points (include/ppo_hip.h "critic") are
declared, bound and exported; value_route (csrc/ppo_route.hip) pairs the value-train forward with the backward train_route
picks; the plain-numpy pooling / loss of the host mirror against the float64 restatement (tests/value_ref.py), whose analytic
dL/dy is held against its own autograd; and the argument checks that need no device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import value_ref
from test_train_route import DTYPE, ERR_UNSUPPORTED, NO_COMPACT, NO_FP32, SHAPES, SIZES, route

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIVE = ("ppo_value_forward", "ppo_rollouts_compute_values", "ppo_rollouts_compute_gae_critic", "ppo_value_forward_backward",
        "ppo_value_train")
NO_BF16_CRITIC = "a bf16-dtype critic is not supported: the value modes exist in the fp32-MFMA forward only"


def test_five_functions_declared_bound_exported(ppo):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppo_hip.h")).read(), flags=re.S)
    jl = open(os.path.join(ROOT, "julia", "ProximalPolicyOptimizationHIP.jl")).read()
    L = ppo._lib.lib()
    for name in FIVE:
        m = re.search(r"int32_t\s+%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
        assert m, "%s is not declared in include/ppo_hip.h" % name
        assert len(ppo._lib.SIGNATURES[name]) == m.group(1).count(",") + 1, name
        assert hasattr(L, name), "%s is not exported by libppo_hip.so" % name
        assert "(:%s, LIB)" % name in jl, "%s has no ccall in the Julia shim" % name
    assert re.search(r"#define\s+PPO_VTARGET_RETURNS\s+0", src) and re.search(r"#define\s+PPO_VTARGET_LAMBDA_RETURNS\s+1", src)
    assert ppo.VALUE_TARGETS == {"returns": 0, "lambda_returns": 1}


def value_route(ppo, dtype, F, hid, L, H, compact, states):
    lib = ppo._lib.lib()
    fn = lib.ppo_debug_value_route
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


def _check_value_routes(ppo):
    seen = set()
    for (dtype, F, hid, L, Q, compact) in SHAPES:
        H = 4 * Q
        for B in SIZES:
            got = value_route(ppo, dtype, F, hid, L, H, compact, B)
            if dtype == "bf16":
                assert got == ("none", NO_BF16_CRITIC), (F, hid, L, Q, compact, B, got)
                continue
            tfwd, tbwd = route(ppo, dtype, F, hid, L, H, compact, B)
            if tfwd == "none":                                       # shapes no fp32 forward covers: the same refusal
                assert tbwd in (NO_FP32, NO_COMPACT) and got == ("none", tbwd), (F, hid, L, Q, compact, B, got)
                continue
            want_fwd = "k_policy_fwd<%d,%d,%d,%d,%d>" % (F, hid, 8 if compact else 6, H // 32, int(L != 2))
            want_bwd = "k_policy_bwd_data<72,%d>" % hid if tbwd.startswith("k_policy_wgrad") else tbwd
            assert got == (want_fwd, want_bwd), (F, hid, L, Q, compact, B, got, tbwd)
            seen.add(tbwd.split("<")[0])
    return seen


def test_value_route(knobs):
    """Forward: always k_policy_fwd in a value-train mode (6: rows through idx, 8: snapshots through idx).  Backward: what
    ppo_debug_train_route reports for the same shape and size, k_policy_bwd_data where that is the one-tile pass's
    k_policy_wgrad -- under the default knobs, with the one-tile pass switched on, and with the split-fp32 kernels off."""
    P = knobs
    seen = _check_value_routes(P)
    assert {"k_policy_bwd_x6", "k_policy_bwd_data", "k_policy_bwd_data_deep"} <= seen, seen
    P.set_train_tile_max_tiles(512)
    assert "k_policy_wgrad" in _check_value_routes(P)
    P.set_train_tile_max_tiles(None)
    P.set_bwd_split_bf16(0)
    assert "k_policy_bwd" in _check_value_routes(P)
    # the benchmark's minibatch, spelled out
    P.set_bwd_split_bf16(None)
    assert value_route(P, "f32", 72, 256, 2, 32, False, 4096) == ("k_policy_fwd<72,256,6,1,0>", "k_policy_bwd_x6<72,256>")
    assert value_route(P, "f32", 72, 128, 3, 32, True, 64) == ("k_policy_fwd<72,128,8,1,1>", "k_policy_bwd_data_deep<72,128>")


def _case(rng, B, H, F=72):
    states = rng.integers(-3, 7, size=(B, H, F)).astype(np.int8)
    active = rng.integers(0, 2 ** (H // 4), size=B, dtype=np.uint64).astype(np.uint32)
    active[0] = 0                                                     # a state with no active quad
    active[1] = 2 ** (H // 4) - 1                                     # and a fully active one
    return states, active


@pytest.mark.parametrize("H", [32, 128])
def test_pooling_and_loss_against_float64(ppo, H):
    rng = np.random.default_rng(H)
    B = 12
    y = rng.normal(size=(B, H, 4)).astype(np.float32) * 3
    _, active = _case(rng, B, H)
    v = ppo.pooled_state_value(y, active)
    v64 = value_ref.pool(y, active)
    assert v.dtype == np.float32 and v.shape == (B,)
    assert v[0] == 0.0 and v64[0] == 0.0 and np.all(np.isfinite(v))
    n = 4 * value_ref.row_mask(active, H).sum(axis=1)
    bound = 2.0 ** -24 * (np.maximum(n - 1, 0) * np.abs(y.astype(np.float64) * value_ref.row_mask(active, H)[:, :, None]).sum(axis=(1, 2))
                          / np.maximum(n, 1) + np.abs(v64))
    assert np.all(np.abs(v.astype(np.float64) - v64) <= bound)
    assert ppo.pooled_state_value(y[3], active[3]) == v[3]            # one state: [H, 4] and a scalar mask
    t = rng.normal(size=B).astype(np.float32)
    l64 = float(np.mean((v.astype(np.float64) - t.astype(np.float64)) ** 2))
    assert abs(ppo.value_loss(v, t) - l64) <= 1e-6 * max(1.0, l64)


@pytest.mark.parametrize("F,hid,L,H", [(72, 128, 2, 32), (72, 64, 3, 32), (216, 128, 2, 32), (72, 128, 1, 128)])
def test_analytic_dy_against_autograd(ppo, F, hid, L, H):
    """dL/dy = 2 (V - t) / (B_global 4 n_rows) on active rows and exactly 0 elsewhere, for B_global = B and B_global > B; a
    state without an active quad has V = 0, a zero gradient row block, and no NaN anywhere."""
    rng = np.random.default_rng(F + hid + L + H)
    B = 10
    params = ppo.glorot_uniform_params(F, hid, L, 4, seed=3) + (rng.normal(size=ppo.glorot_uniform_params(F, hid, L, 4).size) * 0.02).astype(np.float32)
    states, active = _case(rng, B, H, F)
    t = (rng.normal(size=B) + 2).astype(np.float32)
    for Bg in (B, 3 * B):
        loss, g, v, dy = value_ref.loss_grad(params, F, hid, L, states, active, t, B_global=Bg, chunk=4, want_dy=True)
        ana = value_ref.analytic_dy(v, active, t, Bg, H)
        assert np.all(np.isfinite(g)) and np.all(np.isfinite(dy)) and np.isfinite(loss)
        assert np.abs(dy - ana).max() <= 1e-14 * max(1.0, np.abs(ana).max())
        assert v[0] == 0.0 and not dy[0].any() and not ana[0].any()
        assert np.all(dy[~value_ref.row_mask(active, H)] == 0.0)
        assert abs(loss - float(((v - t.astype(np.float64)) ** 2).sum() / Bg)) <= 1e-12 * max(1.0, loss)
        # the restatement's own forward in numpy float64 agrees with the torch one
        assert np.abs(value_ref.values_np(params, F, hid, L, states, active) - v).max() <= 1e-12
        assert np.abs(g).max() > 1e-4


def test_argument_checks_without_a_device(ppo):
    L = ppo._lib.lib()
    one = np.zeros(1, np.float32)
    i64 = np.zeros(1, np.int64)
    f64 = np.zeros(1, np.float64)
    p = ppo._lib
    assert L.ppo_value_forward(None, None, None, 1, 32, one.ctypes.data_as(p.c_f32p)) == -1
    assert "null" in p.last_error()
    assert L.ppo_rollouts_compute_values(None, None, None, None) == -1
    assert L.ppo_rollouts_compute_gae_critic(None, None, None, 0.99, 0.95, None, None) == -1
    assert L.ppo_value_forward_backward(None, None, i64.ctypes.data_as(p.c_i64p), 1, 1, 0, f64.ctypes.data_as(p.c_f64p)) == -1
    assert L.ppo_value_train(None, None, None, 1, 1, 0, None, 0, f64.ctypes.data_as(p.c_f64p), f64.ctypes.data_as(p.c_f64p)) == -1
    assert "null" in p.last_error()
    # an unknown target never reaches the library from the mirror
    for fn in (lambda: ppo.value_forward_backward(None, None, [1], target="td0"), lambda: ppo.value_train_(None, None, None, 1, 1, target="td0")):
        with pytest.raises(ppo.PPOError, match="value target must be one of"):
            fn()


def test_ppo_iterate_signature_keeps_its_positionals(ppo):
    ps = list(inspect.signature(ppo.ppo_iterate_).parameters.values())
    assert [p.name for p in ps[:13]] == ["policy", "env", "optimizer", "episodes_per_iteration", "minibatch_size", "num_ppo_iterations",
                                         "evaluator", "epochs_per_iteration", "discount", "epsilon", "entropy_weight", "state_data_path",
                                         "verbose"]
    kw = {p.name: p.default for p in ps if p.kind is inspect.Parameter.KEYWORD_ONLY}
    assert kw == {"critic": None, "critic_optimizer": None, "gae_lambda": 0.95, "value_epochs": None}
    assert issubclass(ppo.HipCritic, ppo.HipPolicy)
