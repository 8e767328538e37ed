"""The rule of the distinct beam without a device: tests/beam_distinct_ref.py replayed with the oracle's
device-order probabilities (action_probabilities(mode="dev")).

1. properties of every replay: the accepted children of a step are pairwise different and, in mode "parents", differ from
   every parent; ranks strictly increase with the slot; every rejected candidate equals a state seen before it; `examined`
   obeys its definition; every path replays to best_state;
2. K = 1 in mode "children" is the plain replay in every field: one child cannot duplicate;
3. the shape table holds what can go wrong on the device, asserted as counts so that a changed table fails loudly: results the
   plain beam does not reach, an empty beam, steps the budget cuts short, steps that use several windows, candidates that run
   out below K, all parameters zero;
4. the header, the binding table, the Julia shim and the Python signature carry the feature.

What the data cannot show: in these replays no two examined children share score and active but differ in degree, so a
compare that skipped degree would pass (test_no_children_differ_in_degree_alone states it)."""
import inspect
import os
import re

import numpy as np
import pytest

import beam_distinct_ref as dref
import beam_ref as bref
import path_ref as pref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every replay the assertions below read: (shape, mode, rounds)
REPLAYS = (("q8-k3", "children", 4), ("q8-k3", "parents", 4), ("q8-k3", "parents", 1), ("q8-k8", "children", 4),
           ("q8-k8", "parents", 4), ("q8-k64", "parents", 1), ("q8-k64", "parents", 2), ("q8-k130", "parents", 1),
           ("q8-k130", "parents", 2), ("q8-k130", "parents", 4), ("q32-k5", "children", 4), ("ties", "children", 4),
           ("ties", "parents", 4))


def _rec(orc, name, mode, rounds=4):
    return dref.host_reference(orc, name, mode, rounds)


# ---------------------------------------------------------------- 1. properties
@pytest.mark.parametrize("name,mode,rounds", REPLAYS)
def test_walk_properties(orc, name, mode, rounds):
    r = _rec(orc, name, mode, rounds)
    K, T = bref.SHAPES[name]["K"], bref.SHAPES[name]["T"]
    B = dref.WINDOW * rounds
    kw, st = dref.env_kw(name), dref.starts(orc, name)
    for s, steps in enumerate(r["steps"]):
        for x in steps:
            t, walk, ids = x["t"], x["walk"], x["child_ids"]
            acc = [(w, ids[i]) for i, w in enumerate(walk) if w[3] is not None]
            assert len({cid for _, cid in acc}) == len(acc) == x["n"] <= K, "accepted children are pairwise different"
            if mode == "parents":
                assert not {cid for _, cid in acc} & set(x["parent_ids"]), "... and differ from every parent"
            assert [w[3] for w, _ in acc] == list(range(x["n"])), "slot j = the number accepted so far"
            ranks = [w[0] for w, _ in acc]
            assert all(a < b for a, b in zip(ranks, ranks[1:])) and r["rank"][s, t, :x["n"]].tolist() == ranks
            assert (r["rank"][s, t, x["n"]:] == -1).all() and (r["parents"][s, t, x["n"]:] == -1).all()
            assert [w[0] for w in walk] == list(range(len(walk))), "candidates are examined in order, none twice"
            first = {}
            for i, w in enumerate(walk):
                if w[3] is None:
                    kind, j = w[4]
                    if kind == "parent":
                        assert mode == "parents" and ids[i] == x["parent_ids"][j]
                    else:
                        assert j in first and ids[i] == first[j], "a rejected candidate equals a child accepted before it"
                else:
                    first[w[3]] = ids[i]
            # examined: the last accepted rank + 1 if the walk stopped at K, otherwise min(#candidates, B)
            want = ranks[-1] + 1 if x["n"] == K else min(x["ncand"], B)
            assert x["examined"] == len(walk) == want == r["examined"][s, t]
            assert x["cut"] == (x["n"] < K and x["ncand"] > B)
        assert (r["examined"][s, len(steps):] == -1).all() and (r["rank"][s, len(steps):] == -1).all()
        last = steps[-1]
        assert r["best_gap"][s] == 0 or len(steps) == T or last["n"] == 0, "finish: optimum, the last step, or an empty beam"
        # the path replays to the result
        path = [int(a) for a in r["path"][s] if a >= 0]
        assert len(path) == r["best_step"][s]
        got = pref.apply_path(orc, kw, (st[0][s], st[1][s], int(st[2][s])), path)
        assert np.array_equal(got["state"], r["best_state"][s]) and got["active"] == r["best_active"][s]
        assert got["gap"] == r["best_gap"][s] and got["applied"] == r["best_step"][s]


# ---------------------------------------------------------------- 2. K = 1
def test_k1_children_is_the_plain_beam(orc):
    d, p = _rec(orc, "q8-k1", "children"), _rec(orc, "q8-k1", None)
    for k in ("best_state", "best_active", "best_gap", "best_step", "best_beam", "initial_gap", "best_exp", "path", "parents",
              "actions", "exp"):
        assert np.array_equal(d[k], p[k]), k
    for k in ("best_mant", "mant", "log_prob"):
        assert np.array_equal(np.asarray(d[k]).view(np.uint64), np.asarray(p[k]).view(np.uint64)), k
    assert (d["rank"][d["parents"] >= 0] == 0).all() and (d["examined"][d["examined"] >= 0] == 1).all()


# ---------------------------------------------------------------- 3. what the shapes contain
def test_results_the_plain_beam_does_not_reach(orc):
    res = lambda name, mode, s: dref.result(_rec(orc, name, mode), s)
    assert [res("q8-k3", m, 0) for m in (None, "children", "parents")] == [(20, 0), (16, 1), (14, 2)]
    assert [res("q8-k3", m, 3) for m in (None, "children", "parents")] == [(22, 0), (22, 0), (16, 1)]
    assert [res("q8-k8", m, 2) for m in (None, "children", "parents")] == [(2, 1), (2, 1), (0, 3)]
    assert [res("q8-k8", m, 1) for m in (None, "children", "parents")] == [(22, 0), (22, 0), (20, 1)]
    plain, par = _rec(orc, "q8-k8", None), _rec(orc, "q8-k8", "parents")
    assert len(par["steps"][2]) == 3 < len(plain["steps"][2]), "the distinct beam finishes early where the plain one never does"


def test_an_empty_beam_finishes_the_start(orc):
    for rounds in (1, 4):
        r = _rec(orc, "q8-k3", "parents", rounds)
        steps = r["steps"][2]
        assert [x["n"] for x in steps] == [3, 3, 3, 3, 2, 0], "the candidates run out with nothing accepted at the sixth step"
        assert steps[-1]["examined"] == steps[-1]["ncand"] > 0 and not steps[-1]["cut"]
        assert dref.result(r, 2) == (22, 2) and len(steps) < bref.SHAPES["q8-k3"]["T"]
        assert (r["parents"][2, 5:] == -1).all()


def test_the_budget_cuts_steps_short(orc):
    cuts = lambda name, rounds: [sum(x["cut"] for x in steps) for steps in _rec(orc, name, "parents", rounds)["steps"]]
    assert all(len(steps) == 8 for steps in _rec(orc, "q8-k130", "parents", 1)["steps"])
    assert cuts("q8-k130", 1) == [7, 7, 7]
    assert cuts("q8-k130", 2) == [5, 6, 5]
    assert cuts("q8-k130", 4) == [0, 1, 2]
    assert cuts("q8-k64", 1)[1] == 10 and len(_rec(orc, "q8-k64", "parents", 1)["steps"][1]) == 12
    assert cuts("q8-k64", 2)[1] == 0


def test_more_than_one_window_is_used(orc):
    windows = lambda name, rounds: [[dref.windows_used(x) for x in steps] for steps in _rec(orc, name, "parents", rounds)["steps"]]
    w = windows("q8-k130", 4)
    assert max(max(ws) for ws in w) == 4 and all({2, 3, 4} <= set(ws) for ws in w), "second, third and fourth windows"
    full = [x for steps in _rec(orc, "q8-k130", "parents", 4)["steps"] for x in steps if x["n"] == 130 and x["examined"] > 256]
    assert any(x["examined"] % 256 for x in full), "a walk that stops inside a window that is not the first"
    assert max(windows("q8-k64", 2)[1]) == 2 and max(windows("q8-k64", 1)[1]) == 1


def test_candidates_run_out_below_K(orc):
    for name, rounds in (("q8-k64", 2), ("q8-k130", 4)):
        K = bref.SHAPES[name]["K"]
        for steps in _rec(orc, name, "parents", rounds)["steps"]:
            x = steps[0]
            assert x["n"] < K and x["examined"] == x["ncand"] < 256 and not x["cut"]


def test_all_zero_parameters(orc):
    assert not bref.policy_params(orc, "ties").any()
    r = _rec(orc, "ties", "parents")
    assert [dref.result(r, s) for s in range(2)] == [(12, 3), (14, 7)]
    assert [dref.result(_rec(orc, "ties", None), s) for s in range(2)] == [(20, 0), (22, 0)]
    assert [dref.result(_rec(orc, "ties", "children"), s) for s in range(2)] == [(20, 0), (20, 1)]


def test_rejections_of_both_kinds_occur(orc):
    """A candidate equal to a parent (a no-op, or a step onto a sibling's parent) and one equal to an accepted child."""
    for name, mode, rounds in REPLAYS:
        kinds = {w[4][0] for steps in _rec(orc, name, mode, rounds)["steps"] for x in steps for w in x["walk"] if w[3] is None}
        assert kinds == ({"parent", "child"} if mode == "parents" else {"child"}), (name, mode, rounds, kinds)


def test_no_children_differ_in_degree_alone(orc):
    """The statement of the module docstring: the data cannot catch a compare that skips degree."""
    for name, mode, rounds in REPLAYS:
        V = 4 * bref.SHAPES[name]["Q"]
        for steps in _rec(orc, name, mode, rounds)["steps"]:
            for x in steps:
                ids = set(x["child_ids"]) | (set(x["parent_ids"]) if mode == "parents" else set())
                assert len({i[:V] + i[2 * V:] for i in ids}) == len(ids)


# ---------------------------------------------------------------- 4. the layers
def test_the_layers_carry_the_call(ppo):
    hdr = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()
    assert re.search(r"int32_t\s+ppo_beam_search_states_distinct\s*\(", hdr)
    sig = ppo._lib.SIGNATURES
    assert len(sig["ppo_beam_search_states_distinct"]) == len(sig["ppo_beam_search_states"]) + 4 == 25
    assert sig["ppo_beam_search_states_distinct"][:21] == sig["ppo_beam_search_states"]
    jl = open(os.path.join(ROOT, "julia", "ProximalPolicyOptimizationHIP.jl")).read()
    assert ":ppo_beam_search_states_distinct" in jl and ":ppo_beam_search_states, LIB" in jl
    p = inspect.signature(ppo.beam_search_states_distinct_).parameters
    assert list(p) == list(inspect.signature(ppo.beam_search_states_).parameters) + ["distinct", "rounds"]
    assert p["distinct"].default is None and p["rounds"].default == 4 and "beam_search_states_distinct_" in ppo.__all__
    assert ppo.BEAM_MAX_ROUNDS == 16 and ppo.BEAM_DISTINCT_MODES == {None: 0, "children": 1, "parents": 2}
    assert {c[0] for c in dref.GPU_CASES} <= set(bref.SHAPES)
