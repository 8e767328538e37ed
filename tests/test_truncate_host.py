"""Top-k / nucleus truncation (HipPolicy.truncation), the part that needs no device: the reference of
tests/truncate_ref.py is select_ref's at the default truncation and greedy's at top_k = 1; its kept sets have the sizes and the
masses the rule defines; the cases of tests/test_gpu_truncate.py choose other actions than the untruncated sampler, so that the
device comparison is not vacuous; check_truncation; the entry points are declared, bound and ccall'ed and refuse bad values.

TEST_RECORD_DIR=<dir>: the measured shares and kept sizes go to <dir>/truncate.jsonl."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import episodes_ref as ref
import select_ref as S
import truncate_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"ppo_policy_set_truncation": 3, "ppo_policy_get_truncation": 3}
ERR_ARG = -1


def _record(**kw):
    d = os.environ.get("TEST_RECORD_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "truncate.jsonl"), "a") as f:
            f.write(json.dumps(kw) + "\n")


def _fresh(orc, case):
    e = ref._env(orc, ref.env_kw_of(case))
    e.reset()
    return e


# ---------------------------------------------------------------- (a) the construction is sound
@pytest.mark.parametrize("case", (S.SIDE[0], S.SIDE[3]), ids=lambda c: c["name"])
def test_default_truncation_is_the_selection_reference(orc, case):
    """At the default truncation the wrapper returns SelectOracle's bytes, at temperature 1 and at another, sampled and greedy;
    greedy ignores a truncation."""
    params = ref.policy_params(orc, case)
    steps = case["M"] + 3                                               # across the auto-resets
    for sel, trunc in ((("sample", 1.0), T.DEFAULT), (("sample", 0.7), T.DEFAULT), (("greedy", 0.7), T.DEFAULT),
                       (("greedy", 0.7), (2, 0.5))):
        want = S.SelectOracle(orc, *sel).collect_rollouts_tn(_fresh(orc, case), params, case["hid"], steps, n_hidden=case["L"])
        got = T.TruncateOracle(orc, *sel, trunc).collect_rollouts_tn(_fresh(orc, case), params, case["hid"], steps,
                                                                     n_hidden=case["L"])
        assert want["done"].any()
        for k in want:
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (sel, trunc, k)
    assert T.TruncateOracle(orc, "sample", 1.0).glorot_params is orc.glorot_params


@pytest.mark.parametrize("tau", (1.0, 0.7))
@pytest.mark.parametrize("case", (S.SIDE[0], S.SIDE[3]), ids=lambda c: c["name"])
def test_top_k_one_is_greedy_with_p_sel_one(orc, case, tau):
    params = ref.policy_params(orc, case)
    steps = case["M"]
    want = S.SelectOracle(orc, "greedy", tau).collect_rollouts_tn(_fresh(orc, case), params, case["hid"], steps, n_hidden=case["L"])
    got = T.TruncateOracle(orc, "sample", tau, (1, 1.0)).collect_rollouts_tn(_fresh(orc, case), params, case["hid"], steps,
                                                                             n_hidden=case["L"])
    assert np.array_equal(got["actions"], want["actions"])
    assert np.all(got["p_sel"] == np.float32(1.0)) and not np.all(want["p_sel"] == np.float32(1.0))
    for k in ("states", "active", "rewards", "done"):
        assert np.array_equal(got[k], want[k]), k


def _states(orc, case, tau, steps):
    """The tempered p of every (step, env) of an untruncated rollout of `steps` steps, a list of float32 [A]."""
    params = ref.policy_params(orc, case)
    e = _fresh(orc, case)
    out = []
    for t in range(steps):
        for n in range(e.N):
            a, p, _ = S.select_action(orc, e, n, params, case["hid"], case["L"], "sample", tau)
            out.append(p)
            e.step_one(n, a)
    return out


def test_kept_set_sizes_and_masses(orc):
    """top_k alone keeps exactly min(k, A) entries, and they are the k first of the order; top_p alone keeps exactly the
    entries whose mass_before, recomputed here entry by entry with a scalar loop, is below float32(top_p)."""
    for case in (S.SIDE[0], S.SIDE[3]):
        A = 16 * case["Q"]
        for p in _states(orc, case, 1.0, 2)[::5]:
            assert p.size == A
            order = sorted(range(A), key=lambda a: (-float(p[a]), a))          # the rule's strict total order
            rank, mass = T.rank_and_mass(p)
            assert [int(rank[a]) for a in order] == list(range(A))
            for k in (1, 2, 5, A - 1, A, A + 7, 2 ** 31 - 1):
                keep = T.keep_set(p, k, 1.0)
                assert int(keep.sum()) == min(k, A) and set(np.flatnonzero(keep)) == set(order[:k])
            for a in order[:6] + order[-3:] + [0, A - 1]:                       # the sequential mass, ascending b
                m = np.float32(0.0)
                for b in range(A):
                    if p[b] > p[a] or (p[b] == p[a] and b < a):
                        m = np.float32(m + p[b])
                assert m.tobytes() == mass[a].tobytes(), a
            for top_p in (0.5, 0.9, 1e-9, 1.0 - 1e-12):
                keep = T.keep_set(p, 0, top_p)
                tp = np.float32(top_p)
                assert np.array_equal(keep, np.ones(A, bool) if tp == 1 else mass < tp)
                assert keep[order[0]] and (tp == 1 or int(keep.sum()) >= 1)
                if tp != 1:                        # a prefix of the order: mass_before does not fall along it
                    assert set(np.flatnonzero(keep)) == set(order[:int(keep.sum())])
            # both: the intersection; and every non-default truncation renormalises, also one that keeps everything
            assert np.array_equal(T.keep_set(p, 3, 0.8), T.keep_set(p, 3, 1.0) & T.keep_set(p, 0, 0.8))
            full = T.truncate(p, A, 1.0)
            assert np.array_equal(full, p / T.device_order_sum(p)) and np.count_nonzero(full) == np.count_nonzero(p)
            # the device-order sum of p itself is the softmax's own denominator's order: close to 1, and float32
            assert abs(float(T.device_order_sum(p)) - 1.0) < 1e-5


def test_a_state_without_an_active_quad_stays_nan(orc):
    """p NaN everywhere: no comparison holds, everything is kept and NaN stays NaN."""
    p = np.full(128, np.nan, np.float32)
    for trunc in T.TRUNCATIONS:
        assert T.keep_set(p, *trunc).all() and np.isnan(T.truncate(p, *trunc)).all()


# ---------------------------------------------------------------- (b) the cases contain what matters
def test_truncations_leave_the_untruncated_samplers_actions(orc):
    """On SIDE[0] (24 envs, 8 steps) and SIDE[3] (Q = 32, 10 envs, 6 steps) at temperatures 1 and 2: the rollout under each
    truncation chooses another action than the untruncated sampler's rollout at the same (step, env), i.e. the same tick and
    uniform, in at least 40 % of the steps, and the nucleus keeps a set whose mean size along the rollout is recorded."""
    for case in (S.SIDE[0], S.SIDE[3]):
        params = ref.policy_params(orc, case)
        steps = case["N"] * case["M"]
        for tau in (1.0, 2.0):
            base = S.select_rollout_tn(orc, _fresh(orc, case), params, case["hid"], case["M"], "sample", tau, case["L"])
            for tr in T.TRUNCATIONS:
                e = _fresh(orc, case)
                differ = kept = 0
                for t in range(case["M"]):
                    for n in range(e.N):
                        a, pp, _ = T.select_action(orc, e, n, params, case["hid"], case["L"], "sample", tau, tr)
                        differ += a != base["actions"][t, n]
                        kept += int(np.count_nonzero(pp))
                        e.step_one(n, a)
                        if e.done[n]:
                            e.reset_one(n)
                share, size = differ / steps, kept / steps
                print(case["name"], "tau", tau, tr, "other action in %.1f %%" % (100 * share), "mean kept %.1f" % size)
                _record(test="non_vacuity", case=case["name"], Q=case["Q"], tau=tau, top_k=tr[0], top_p=tr[1], steps=steps,
                        share_other_action=share, mean_kept=size)
                assert share >= 0.40, (case["name"], tau, tr, share)
                if tr[0]:
                    assert size <= tr[0]


def test_tie_cases(orc):
    """Logits (0, 1, 1, 0) on every row: top_k = 3 keeps the three lowest-indexed maxima, each with p'' = 1/3 as the reference
    rounds it; at Q = 32 they lie in tiles 1 and 2.  At temperature 2^-7 the minima underflow to 0 and the maxima are uniform,
    1 / n each with n a power of two: the sequential mass of equal terms is exact, mass_before of the maximum number n/2 is 0.5
    exactly, and top_p = 0.5 keeps n/2 of them -- `<=` would keep one more."""
    for Q, masks in ((8, T.TIE_MASKS_Q8), (32, T.TIE_MASKS_Q32)):
        for m in masks:
            p = T.tie_probabilities(orc, m, Q)
            maxima = T.tie_maxima(m, Q)
            assert len(maxima) >= 8 and np.all(p[maxima] == p.max()) and np.count_nonzero(p == p.max()) == len(maxima)
            pp = T.truncate(p, 3, 1.0)
            assert np.flatnonzero(pp).tolist() == maxima[:3]
            assert len(set(pp[maxima[:3]].tolist())) == 1 and abs(float(pp[maxima[0]]) - 1 / 3) < 1e-7
            # uniform maxima
            u = T.tie_probabilities(orc, m, Q, T.TIE_UNIFORM_TAU)
            n = len(maxima)
            assert n & (n - 1) == 0 and np.all(u[maxima] == np.float32(1.0 / n)) and np.count_nonzero(u) == n
            _, mass = T.rank_and_mass(u)
            assert mass[maxima[n // 2]] == np.float32(0.5) and mass[maxima[n // 2 - 1]] < np.float32(0.5)
            uu = T.truncate(u, 0, 0.5)
            assert np.flatnonzero(uu).tolist() == maxima[:n // 2] and np.all(uu[maxima[:n // 2]] == np.float32(2.0 / n))
            assert int((mass[maxima] <= np.float32(0.5)).sum()) == n // 2 + 1
    assert all((m & 0xFF) == 0 and (m >> 24) == 0 for m in T.TIE_MASKS_Q32)


def test_search_cases_differ_from_the_untruncated_search(orc):
    sel, trunc = T.SEARCH_CASE
    base, got = S.search(orc, T.SEARCH_SHAPE, sel), T.search(orc, T.SEARCH_SHAPE, sel, trunc)
    assert not np.array_equal(got["clone_gaps"], base["clone_gaps"])
    assert len(set(got["clone_gaps"][0].tolist())) > 1


# ---------------------------------------------------------------- (c) check_truncation and the entry points
def test_check_truncation(ppo):
    P = ppo
    assert P.check_truncation() == (0, 1.0) == P.DEFAULT_TRUNCATION
    assert P.check_truncation(5, 1) == (5, 1.0) and isinstance(P.check_truncation(5, 1)[1], float)
    assert P.check_truncation(np.int32(3), np.float32(0.5)) == (3, 0.5) and isinstance(P.check_truncation(np.int64(3))[0], int)
    assert P.check_truncation(2 ** 31 - 1, 1e-300) == (2 ** 31 - 1, 1e-300)
    for k, p in ((-1, 1.0), (2 ** 31, 1.0), (1.5, 1.0), ("3", 1.0), (None, 1.0), (True, 1.0), (0, 0.0), (0, -0.5), (0, 1.0000001),
                 (0, float("nan")), (0, float("inf")), (0, float("-inf")), (0, "half"), (0, None)):
        with pytest.raises(P.PPOError) as ei:
            P.check_truncation(k, p)
        assert ei.value.status == ERR_ARG, (k, p)
    assert all(n in P.__all__ for n in ("check_truncation", "selecting"))


def test_entry_points_are_declared_bound_and_ccalled(ppo):
    raw = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    jl = open(os.path.join(ROOT, "julia", "ProximalPolicyOptimizationHIP.jl")).read()
    L = ppo._lib.lib()
    for name, arity in NEW.items():
        m = re.search(r"int32_t\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m and m.group(1).count(",") + 1 == arity, name
        assert len(ppo._lib.SIGNATURES[name]) == arity and hasattr(L, name), name
        assert "(:%s, LIB)" % name in jl, name
    assert "function set_truncation!(" in jl and "function get_truncation(" in jl
    block = raw[raw.index("Truncation of the distribution"):raw.index("int32_t ppo_policy_set_truncation")]
    for word in ("NOT READ by", "ppo_collect_rollouts", "ppo_collect_paths", "ppo_policy_forward", "training call", "ascending b"):
        assert word in block, word
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "`HipPolicy.truncation`" in readme


def test_bad_values_are_refused_without_a_device(ppo):
    """The setter judges top_k and top_p before the handle and makes no device call: this runs without a GPU."""
    L = ppo._lib.lib()
    for k, p, msg in ((-1, 1.0, "top_k must be"), (-2 ** 31, 0.5, "top_k must be"), (0, 0.0, "top_p must be"),
                      (3, -0.5, "top_p must be"), (0, 1.0000001, "top_p must be"), (0, float("nan"), "top_p must be"),
                      (0, float("inf"), "top_p must be")):
        assert L.ppo_policy_set_truncation(None, k, p) == ERR_ARG and msg in ppo._lib.last_error(), (k, p)
    for k, p in ((0, 1.0), (1, 1.0), (0, 0.5), (2 ** 31 - 1, 1e-300)):
        assert L.ppo_policy_set_truncation(None, k, p) == ERR_ARG and "null policy" in ppo._lib.last_error(), (k, p)
    k, d = C.c_int32(0), C.c_double(0)
    assert L.ppo_policy_get_truncation(None, C.byref(k), C.byref(d)) == ERR_ARG


def test_selecting_signature(ppo):
    """selecting(policy, rule, temperature, top_k=0, top_p=1.0): existing calls are unchanged; sets and restores both."""
    import inspect
    sig = inspect.signature(ppo.selecting)
    assert list(sig.parameters) == ["policy", "rule", "temperature", "top_k", "top_p"]
    assert [sig.parameters[n].default for n in ("rule", "temperature", "top_k", "top_p")] == ["sample", 1.0, 0, 1.0]

    class Handle:
        selection, truncation = ("greedy", 0.5), (4, 0.25)
    h = Handle()
    with ppo.selecting(h, "sample", 2.0, top_p=0.9) as got:
        assert got is h and h.selection == ("sample", 2.0) and h.truncation == (0, 0.9)
    assert h.selection == ("greedy", 0.5) and h.truncation == (4, 0.25)
    with ppo.selecting(h, "greedy"):
        assert h.selection == ("greedy", 1.0) and h.truncation == (0, 1.0)
    assert h.selection == ("greedy", 0.5) and h.truncation == (4, 0.25)
    with pytest.raises(ppo.PPOError):
        with ppo.selecting(h, "sample", 1.0, top_k=-1):
            pass
    assert h.selection == ("greedy", 0.5) and h.truncation == (4, 0.25)
