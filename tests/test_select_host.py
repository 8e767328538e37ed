"""Action selection rules (HipPolicy.selection), the part that needs no device: the reference of
tests/select_ref.py reproduces the oracle's own rollout at ("sample", 1); check_selection; the entry points are declared, bound
and ccall'ed and refuse bad values; and the reference cases contain what the device comparison of tests/test_gpu_select.py
leans on, so that it is not vacuous."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import episodes_ref as ref
import select_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"ppo_policy_set_selection": 3, "ppo_policy_get_selection": 3}
ERR_ARG = -1


# ---------------------------------------------------------------- (a) the construction is sound
@pytest.mark.parametrize("Q,hid,L,N,T", [(8, 256, 2, 6, 20), (8, 128, 3, 4, 9), (32, 128, 2, 3, 6)],
                         ids=["q8-h256", "q8-L3", "q32"])
def test_reference_at_temperature_one_is_the_oracles_rollout(orc, Q, hid, L, N, T):
    """select_rollout_tn at ("sample", 1) returns the bytes of orc.collect_rollouts_tn: actions, p_sel and every other column,
    across the auto-resets (max_actions 7 < T)."""
    params = orc.glorot_params(ref.F, hid, L, seed=3)
    envs = []
    for _ in range(2):
        e = orc.Env(Q=Q, max_actions=7, N=N, seed=ref.SEED, global_offset=40)
        e.reset()
        envs.append(e)
    want = orc.collect_rollouts_tn(envs[0], params, hid, T, mode_dev=True, n_hidden=L)
    got = S.select_rollout_tn(orc, envs[1], params, hid, T, "sample", 1.0, L)
    assert want["done"].any() or T <= 7
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert np.array_equal(envs[0].tick, envs[1].tick) and np.array_equal(envs[0].episode, envs[1].episode)
    # the proxy hands every replay of tests/ the same thing
    e = orc.Env(Q=Q, max_actions=7, N=N, seed=ref.SEED, global_offset=40)
    e.reset()
    again = S.SelectOracle(orc, "sample", 1.0).collect_rollouts_tn(e, params, hid, T, mode_dev=True, n_hidden=L)
    assert all(np.array_equal(again[k], want[k]) for k in want)
    assert S.SelectOracle(orc, "greedy", 1.0).glorot_params is orc.glorot_params


# ---------------------------------------------------------------- (b) check_selection
def test_check_selection(ppo):
    P = ppo
    assert P.check_selection("sample", 1.0) == ("sample", 1.0) and P.check_selection("greedy") == ("greedy", 1.0)
    assert P.check_selection("sample", 2) == ("sample", 2.0) and isinstance(P.check_selection("sample", 2)[1], float)
    assert P.check_selection("greedy", np.float32(0.5)) == ("greedy", 0.5)
    assert P.check_selection("sample", 1e-30)[1] == 1e-30 and P.check_selection("sample", 1e30)[1] == 1e30
    for rule, t in (("sample", 0.0), ("sample", -1.0), ("greedy", float("nan")), ("sample", float("inf")),
                    ("sample", float("-inf")), ("sample", "warm"), ("sample", None), ("argmax", 1.0), ("Sample", 1.0),
                    (0, 1.0), (None, 1.0), ("", 1.0)):
        with pytest.raises(P.PPOError) as ei:
            P.check_selection(rule, t)
        assert ei.value.status == ERR_ARG, (rule, t)
    assert P.SELECT_RULES == ("sample", "greedy")
    assert all(n in P.__all__ for n in ("check_selection", "selecting"))


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
    assert re.search(r"#define\s+PPO_SELECT_SAMPLE\s+0\b", hdr) and re.search(r"#define\s+PPO_SELECT_GREEDY\s+1\b", hdr)
    assert "function set_selection!(" in jl and "function get_selection(" in jl
    assert hasattr(L, "ppo_debug_select_step") and "ppo_debug_select_step" not in raw
    # the header and the README say which calls do not read the selection
    block = raw[raw.index("Action selection of the calls"):raw.index("#define PPO_SELECT_SAMPLE")]
    for word in ("NOT READ by", "ppo_collect_rollouts", "ppo_collect_paths", "ppo_policy_forward", "training call"):
        assert word in block, word
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "selection" in readme and "collect_paths_" in readme[readme.index("`HipPolicy.selection`"):][:2500]


def test_bad_values_are_refused_without_a_device(ppo):
    """The setter judges rule and temperature before the handle and makes no device call: this runs without a GPU."""
    L = ppo._lib.lib()
    for rule, t, msg in ((2, 1.0, "rule must be"), (-1, 1.0, "rule must be"), (0, 0.0, "temperature must be"),
                         (0, -0.5, "temperature must be"), (1, float("nan"), "temperature must be"),
                         (0, float("inf"), "temperature must be"), (1, float("-inf"), "temperature must be")):
        assert L.ppo_policy_set_selection(None, rule, t) == ERR_ARG and msg in ppo._lib.last_error(), (rule, t)
    for rule, t in ((0, 1.0), (1, 1.0), (0, 0.25), (1, 0.7), (0, 1e30)):
        assert L.ppo_policy_set_selection(None, rule, t) == ERR_ARG and "null policy" in ppo._lib.last_error(), (rule, t)
    r, d = C.c_int32(0), C.c_double(0)
    assert L.ppo_policy_get_selection(None, C.byref(r), C.byref(d)) == ERR_ARG


# ---------------------------------------------------------------- (c) the cases contain what matters
def test_tempered_cases_leave_the_default_trajectories(orc):
    """Per sampled temperature at least half of the steps of the main case choose another action than ("sample", 1) does at
    the same (env, tick); the first 8 steps of env 0 are printed like the issue records them."""
    base = S.episodes(orc, S.MAIN, S.DEFAULT)
    for tau in S.TEMPERATURES:
        got = S.episodes(orc, S.MAIN, ("sample", tau))
        T = min(base["actions"].shape[0], got["actions"].shape[0])
        both = base["valid"][:T] & got["valid"][:T]
        differ = (base["actions"][:T] != got["actions"][:T]) & both
        first8 = int(differ[:8, 0].sum())
        print("tau", tau, "steps", int(both.sum()), "other action", int(differ.sum()), "first 8 of env 0:", first8)
        assert 2 * int(differ.sum()) >= int(both.sum()), tau
        assert 2 * first8 >= 8, tau
        assert not np.array_equal(base["p_sel"][:T][both], got["p_sel"][:T][both])


def test_inexact_scaling_differs_from_scaling_by_a_rounded_quotient(orc):
    """0.7 and 1.3 are the temperatures whose float32 reciprocal is inexact: l * fl(1 / tau) and l / tau differ in at least one
    logit of the first state, so a device that divided would not reproduce the reference's p_sel."""
    case = S.MAIN
    e = ref._env(orc, ref.env_kw_of(case), 1)
    e.episode[0] = 1
    e.reset()
    l = S.logits(orc, ref.policy_params(orc, case), ref.F, case["hid"], case["L"], e.observe_one(0))
    for tau in (0.7, 1.3):
        assert np.any((l * np.float32(1.0 / tau)).astype(np.float32) != (l / np.float32(tau)).astype(np.float32)), tau
    for tau in (0.5, 2.0, 0.25):
        assert np.array_equal((l * np.float32(1.0 / tau)).astype(np.float32), (l / np.float32(tau)).astype(np.float32)), tau


def test_greedy_cases_move(orc):
    """Greedy paths of the coverage case hold at least 10 distinct actions, and every greedy case at least one accepted move."""
    cov = S.episodes(orc, S.GREEDY_COVERAGE, ("greedy", 1.0))
    distinct = len(set(int(a) for a in cov["actions"][cov["valid"]]))
    changed, total = S.state_changes(orc, S.GREEDY_COVERAGE, cov)
    print("greedy coverage: distinct actions", distinct, "state changed in", changed, "of", total, "steps")
    assert distinct >= 10 and total == 480
    for case in (S.GREEDY_COVERAGE, S.MAIN) + S.SIDE:
        for sel in (("greedy", 1.0), ("greedy", 0.7)):
            if case in S.SIDE and sel not in S.SIDE_SELECTIONS:
                continue
            cols = S.episodes(orc, case, sel)
            changed, total = S.state_changes(orc, case, cols)
            print(case["name"], sel, "state changed in", changed, "of", total)
            assert changed >= 1, (case["name"], sel)
    # greedy at another temperature is greedy on the tempered p: same actions here (a positive factor keeps the order unless
    # rounding merges two logits), other probabilities
    a, b = S.episodes(orc, S.MAIN, ("greedy", 1.0)), S.episodes(orc, S.MAIN, ("greedy", 0.7))
    assert not np.array_equal(a["p_sel"], b["p_sel"])


def test_tie_cases(orc):
    """logits (0, 1, 1, 0) on every row: greedy plays 16 * (lowest active quad) + 1, the first of the tied maxima, at any
    temperature; the Q = 32 masks keep tiles 1 and 2 alone."""
    for Q, masks in ((8, S.TIE_MASKS_Q8), (32, S.TIE_MASKS_Q32)):
        for m in masks:
            for tau in (1.0, 0.7):
                a, p = S.tie_expected(orc, m, Q, tau)
                assert a == 16 * S.lowest_quad(m) + 1, (Q, hex(m), tau)
                assert p > 0 and abs(float(p) - 1.0 / (8 * bin(m).count("1") * (1 + np.exp(-1.0 / tau)))) < 1e-6
    assert S.tie_expected(orc, (1 << 9) | (1 << 20), 32)[0] == 145
    assert all((m & 0xFF) == 0 and (m >> 24) == 0 for m in S.TIE_MASKS_Q32)
    # the tie policy really has those logits on an arbitrary state
    e = orc.Env(Q=8, max_actions=5, N=1, seed=ref.SEED)
    e.reset()
    l = orc.mlp_logits(S.tie_params(orc, 128, 2), ref.F, 128, e.observe_one(0), "dev", 2)
    assert np.array_equal(l, np.tile(np.array([0, 1, 1, 0], np.float32), 32))


def test_search_cases_differ_from_the_default(orc):
    """The search shapes under a selection return other results than the default: the device comparison cannot pass by
    ignoring the setting.  Greedy: all K clones of a start play one trajectory."""
    shape = S.SEARCH_SHAPE
    base = S.search(orc, shape, S.DEFAULT)
    for sel in S.SEARCH_SELECTIONS:
        got = S.search(orc, shape, sel)
        assert not np.array_equal(got["clone_gaps"], base["clone_gaps"]), sel
    g = S.search(orc, shape, ("greedy", 1.0))
    assert np.all(g["clone_gaps"] == g["clone_gaps"][:, :1]) and np.all(g["best_clone"] == 0)
    assert len(set(base["clone_gaps"][0].tolist())) > 1
