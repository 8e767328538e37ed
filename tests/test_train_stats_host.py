"""Update statistics and target-KL early stopping, the part that needs no device: the four entry points are declared, bound,
exported and ccall'ed and refuse bad arguments; kl_stats and the explained variance against closed forms and numpy; and the
float64 restated run the device's early-stopping test leans on has the property that test needs."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import train_stats_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"ppo_policy_set_target_kl": 2, "ppo_policy_get_target_kl": 2, "ppo_policy_last_train_stats": 7,
       "ppo_rollouts_value_moments": 3}
ERR_ARG = -1


def test_entry_points_are_declared_bound_exported_and_ccalled(ppo):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppo_hip.h")).read(), flags=re.S)
    jl = open(os.path.join(ROOT, "julia", "ProximalPolicyOptimizationHIP.jl")).read()
    L = ppo._lib.lib()
    for name, arity in NEW.items():
        m = re.search(r"int32_t\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m, "%s is not declared in include/ppo_hip.h" % name
        assert m.group(1).count(",") + 1 == arity, name
        assert len(ppo._lib.SIGNATURES[name]) == arity, name
        assert hasattr(L, name), name
        assert "(:%s, LIB)" % name in jl, "%s has no ccall in the Julia shim" % name
    assert hasattr(L, "ppo_debug_train_ratios")
    for fn in ("set_target_kl!", "last_train_stats", "explained_variance"):
        assert "function %s(" % fn in jl, fn
    # every header entry carries its one-line reference citation
    raw = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()
    for name in NEW:
        at = re.search(r"int32_t\s+%s\s*\(" % name, raw).start()
        comment = raw[raw.rfind("/*", 0, at):at]
        assert comment.rstrip().endswith("*/") and "no reference op" in comment, name


def test_null_handles_and_bad_targets_are_refused_without_a_device(ppo):
    L = ppo._lib.lib()
    d, i = C.c_double(0), C.c_int32(0)
    assert L.ppo_policy_set_target_kl(None, 0.01) == ERR_ARG and "null policy" in ppo._lib.last_error()
    assert L.ppo_policy_get_target_kl(None, C.byref(d)) == ERR_ARG
    assert L.ppo_policy_last_train_stats(None, 0, C.byref(i), C.byref(i), None, None, None) == ERR_ARG
    s5 = np.zeros(5)
    assert L.ppo_rollouts_value_moments(None, 0, s5.ctypes.data_as(ppo._lib.c_f64p)) == ERR_ARG
    L.ppo_debug_train_ratios.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.ppo_debug_train_ratios.restype = C.c_int32
    assert L.ppo_debug_train_ratios(None, 1, None) == ERR_ARG
    # the value is judged before the handle: -1 and NaN are refused AS VALUES, 0 / 0.01 / inf pass that check and only then
    # meet the null handle (no policy handle exists without a device; the read-back is in tests/test_gpu_train_stats.py)
    for bad in (-1.0, float("nan"), -0.001, float("-inf")):
        assert L.ppo_policy_set_target_kl(None, bad) == ERR_ARG
        assert "target_kl must be" in ppo._lib.last_error(), bad
    for ok in (0.0, 0.01, float("inf")):
        assert L.ppo_policy_set_target_kl(None, ok) == ERR_ARG
        assert "null policy" in ppo._lib.last_error() and "target_kl must be" not in ppo._lib.last_error(), ok


def test_kl_stats_closed_forms(ppo):
    z = ppo.kl_stats(np.ones(1000, np.float32), 0.2)
    assert z == {"approx_kl": 0.0, "old_approx_kl": 0.0, "clip_fraction": 0.0}
    for d in (0.5, 1.0, 2.0):
        for sgn in (1.0, -1.0):
            r = np.full(2, np.exp(sgn * d))
            s = ppo.kl_stats(r, 0.2)
            # float64 identities: -log(exp(+-d)) = -+d, and (r - 1) - log r = exp(+-d) - 1 -+ d
            assert abs(s["old_approx_kl"] - (-sgn * d)) <= 1e-15 * d, (d, sgn, s)
            want = (np.exp(sgn * d) - 1.0) - sgn * d
            assert abs(s["approx_kl"] - want) <= 1e-15 * abs(want), (d, sgn, s, want)
            assert s["clip_fraction"] == 1.0
    # the clip count: exactly at 1 +- eps is inside (|r - 1| > eps is false), one ulp further is outside; eps exact in binary
    for dt in (np.float32, np.float64):
        eps = 0.25
        hi, lo = dt(1.25), dt(0.75)
        r = np.array([hi, np.nextafter(hi, dt(0)), np.nextafter(hi, dt(2)), lo, np.nextafter(lo, dt(1)), np.nextafter(lo, dt(0))], dt)
        assert ppo.kl_stats(r, eps)["clip_fraction"] == 2 / 6, dt
        assert ppo.kl_stats(r[[0, 1, 3, 4]], eps)["clip_fraction"] == 0.0
        assert ppo.kl_stats(r[[2, 5]], eps)["clip_fraction"] == 1.0
        assert ref.ratio_sums(r, eps)[2] == 2
    # agrees with the helper the device tests use
    rng = np.random.default_rng(0)
    r = np.exp(rng.normal(size=5000) * 0.1).astype(np.float32)
    s1, s3, c, n = ref.ratio_sums(r, 0.05)
    s = ppo.kl_stats(r, 0.05)
    assert (s["old_approx_kl"], s["approx_kl"], s["clip_fraction"]) == (s1 / n, s3 / n, c / n)


def test_explained_variance_from_five_sums(ppo):
    rng = np.random.default_rng(1)
    n = 4000
    t = (rng.normal(size=n) * 3 + 100.0)
    v = t + rng.normal(size=n)                      # a critic that explains most of it
    valid = rng.random(n) < 0.8
    i0 = int(np.flatnonzero(valid)[0])
    sums, _ = ref.value_moments(t, v, valid, i0)
    want = 1.0 - np.var((t - v)[valid]) / np.var(t[valid])
    got = ppo.explained_variance_from_sums(sums)
    # shifted sums: Var from them loses about n * 2^-52 relative to E[x^2], far inside this
    assert abs(got - want) <= 1e-12, (got, want)
    assert 0.8 < got < 1.0
    # an unshifted statement of the same sums agrees too (the shift only changes conditioning)
    x, y = t[valid], (t - v)[valid]
    raw = [x.size, x.sum(), (x * x).sum(), y.sum(), (y * y).sum()]
    assert abs(ppo.explained_variance_from_sums(raw) - want) <= 1e-9
    const, _ = ref.value_moments(np.full(n, 2.5), v, valid, i0)
    assert math.isnan(ppo.explained_variance_from_sums(const))


def test_restated_run_has_a_rising_epoch(ppo, orc):
    """The device's early-stopping test needs an epoch j in 1..4 whose approx_kl exceeds every earlier epoch's.  That is a
    property of the inputs: here on the CPU oracle's rollout of the same seeded setup (the device test asserts it again on
    the rollout it collected)."""
    c = ref.EARLY
    params = ppo.glorot_uniform_params(c["F"], c["HID"], c["L"], 4, c["policy_seed"])
    env = orc.Env(Q=c["Q"], max_actions=c["max_actions"], N=c["N"], seed=c["env_seed"])
    env.reset()
    ro = orc.collect_rollouts_tn(env, params, c["HID"], c["T"], mode_dev=True)
    n = c["N"] * c["T"]
    cols = dict(states=ro["states"].reshape(n, 32, c["F"]), active=ro["active"].reshape(n), a0=ro["actions"].reshape(n),
                p_old=ro["p_sel"].reshape(n), adv=orc.compute_returns_tn(ro["rewards"], ro["done"], c["discount"]).reshape(n),
                Q=c["Q"])
    assert ro["done"].any(), "episodes form inside the rollout"
    k, clips, p = ref.restated_run(params, c["F"], c["HID"], c["L"], cols, ref.early_perms(n), c["batch"], c["eps"], c["ent"],
                                   c["eta"])
    print("restated approx_kl per epoch:", k, "clip fractions:", clips)
    assert len(k) == c["epochs"] and all(np.isfinite(k)) and all(x > 0 for x in k)
    j = ref.first_rise(k)
    assert j is not None, k
    assert not np.array_equal(p, params)
