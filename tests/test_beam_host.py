"""The rule of beam search without a device: tests/beam_ref.py replayed with the oracle's device-order
probabilities (action_probabilities(mode="dev")).

1. unit properties of the rule: the child weight is one fp64 multiply re-normalised exactly, also at the smallest fp32
   probability; the order is (e' descending, m' descending, index ascending), and m' never decides against e';
2. the shape table of tests/test_gpu_beam.py holds every situation that matters, so that the GPU test cannot pass by luck --
   conditions on the inputs, checked on the reference alone;
3. the replay is consistent with itself: the path replays to the result, the weight of the result is the product along the
   path, K = 1 follows the arg-max;
4. the header, the binding table, the Julia shim and the Python signature carry the feature.

Every situation the issue names holds on the built-in env; none had to be dropped."""
import inspect
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import beam_ref as bref
import path_ref as pref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _within_the_staging_limit(ppo):
    """The table is written for the call as it is built: every beam width lies inside the limit the package names."""
    assert all(c["K"] <= ppo.BEAM_MAX_K for c in bref.SHAPES.values())


# ---------------------------------------------------------------- 1. the rule
def test_child_weight_is_one_exact_renormalised_multiply():
    rng = np.random.default_rng(0)
    tiny = np.float32(2.0 ** -149)
    ps = [tiny, np.float32(1.0), np.float32(0.5), np.float32(1.1754944e-38), np.float32(1e-40)]
    ps += list(rng.random(200).astype(np.float32) + tiny)
    ms = [0.5, float(np.nextafter(1.0, 0.0)), 0.75] + list(0.5 + rng.random(50) / 2)
    for p in ps:
        for m in ms:
            m2, e2 = bref.child_weight(m, -7, p)
            assert 0.5 <= m2 < 1.0
            exact = Fraction(m) * Fraction(float(p))
            got = Fraction(m2) * Fraction(2) ** (e2 + 7)
            assert abs(got - exact) <= exact * Fraction(1, 2 ** 53), "one rounding of an fp64 multiply, frexp exact"
            assert Fraction(float(np.float64(m) * np.float64(p))) == got, "x is normal: re-normalising loses nothing"


def test_order_is_exponent_then_mantissa_then_index():
    # slot 0 (weight 0.75 * 2^0) and slot 1 (weight 0.5 * 2^1 = 1.0): slot 1's candidates have the higher exponent although
    # slot 0 has the higher mantissa
    p = np.array([[0.5, 0.25, 0.25, 0.0], [0.25, 0.25, 0.5, 0.0]], np.float32)
    cand = bref.candidates([0, 1], {0: (0.75, 0), 1: (0.5, 1)}, p)
    assert len(cand) == 6, "p == 0 is no candidate"
    got = [(c[3], c[4]) for c in cand]
    # weights: (1,2) 0.5 = 0.5*2^0 ; (0,0) 0.375 = 0.75*2^-1 ; (1,0),(1,1) 0.25 = 0.5*2^-1 ; (0,1),(0,2) 0.1875 = 0.75*2^-2
    assert got == [(1, 2), (0, 0), (1, 0), (1, 1), (0, 1), (0, 2)]
    assert [(c[5], c[6]) for c in cand] == [(0.5, 0), (0.75, -1), (0.5, -1), (0.5, -1), (0.75, -2), (0.75, -2)]
    wrong = sorted(cand, key=lambda c: (-c[5], c[2]))            # m' compared without e'
    assert [(c[3], c[4]) for c in wrong] != got


# ---------------------------------------------------------------- 2. what the shapes contain
@pytest.fixture(scope="module")
def host_cover(orc):
    return {name: bref.coverage(bref.host_reference(orc, name), bref.SHAPES[name]["K"]) for name in bref.HOST_SHAPES}


def test_shape_table_is_the_issues(orc):
    want = {(8, 1), (8, 3), (8, 8), (8, 64), (8, 130), (32, 5), (32, 256)}
    assert {(bref.SHAPES[n]["Q"], bref.SHAPES[n]["K"]) for n in bref.GPU_SHAPES} == want
    for name in bref.GPU_SHAPES:
        c = bref.SHAPES[name]
        assert 8 <= c["T"] <= 24 and 1 <= c["K"] <= c["N"]
    big, wide = bref.SHAPES["q32-k256"], bref.SHAPES["q8-k130"]
    assert big["K"] * 16 * big["Q"] == 131072 and big["M"] == 1 and big["T"] == 8
    A = 16 * wide["Q"]
    assert wide["K"] > A and wide["K"] * A == 16640 and wide["N"] % wide["K"] != 0
    S = wide["N"] // wide["K"]
    assert S < wide["M"] < 2 * S, "two rounds, the second partial"
    assert any(c["K"] % 8 and c["K"] % 64 for c in (bref.SHAPES[n] for n in bref.GPU_SHAPES))
    assert set(bref.HOST_SHAPES) - {"ties"} <= set(bref.GPU_SHAPES)


def test_dead_slots_are_exercised(host_cover):
    c = host_cover["q8-k130"]
    assert c["fewer_than_K_at_step0"] == bref.SHAPES["q8-k130"]["M"], "one live slot has at most A = 128 candidates"
    assert c["dead_slots"] >= 1


def test_a_start_reaches_the_optimum_early_and_one_never_does(host_cover):
    for name in ("q8-k3", "q8-k8"):
        assert host_cover[name]["reached_optimum_early"] >= 1, name
        assert host_cover[name]["never_optimum"] >= 1, name
        assert host_cover[name]["result_at_start"] >= 1, name


def test_a_result_is_found_off_slot_0(host_cover):
    for name in ("q8-k3", "q8-k8", "q8-k130", "q32-k5"):
        assert host_cover[name]["result_off_slot0"] >= 1, name


def test_a_parent_is_shared_while_a_live_parent_is_childless(host_cover):
    for name in ("q8-k3", "q8-k8", "q8-k130", "q32-k5"):
        assert host_cover[name]["shared_and_childless_parent"] >= 1, name


def test_rounds(host_cover):
    for name in ("q8-k3", "q8-k130", "q32-k5"):
        assert host_cover[name]["rounds"] >= 2 and host_cover[name]["partial_round"] == 1, name


def test_exact_weight_ties_are_decided_by_the_index(orc, host_cover):
    assert host_cover["ties"]["index_decided"] >= 1
    for name in ("q8-k3", "q8-k8", "q8-k130"):
        assert host_cover[name]["index_decided"] >= 1, "no-op actions leave equal states behind: equal rows, equal weights"
    # all parameters zero: at step 0 every candidate ties, so the chosen ones are the lowest indices in index order
    r = bref.host_reference(orc, "ties")
    K = bref.SHAPES["ties"]["K"]
    for s, steps in enumerate(r["steps"]):
        st = steps[0]
        valid = np.flatnonzero(st["probs"][0] > 0)
        assert len(set(st["probs"][0][valid].tolist())) == 1
        assert [a for _, a, _, _ in st["chosen"]] == [int(a) for a in valid[:K]]
        assert len({(m, e) for _, _, m, e in st["chosen"]}) == 1


# ---------------------------------------------------------------- 3. the replay against itself
@pytest.mark.parametrize("name", bref.HOST_SHAPES)
def test_path_replays_to_the_result_and_carries_its_weight(orc, name):
    r = bref.host_reference(orc, name)
    kw, st = bref.env_kw(name), bref.starts(orc, name)
    for s in range(st[2].shape[0]):
        path = [int(a) for a in r["path"][s] if a >= 0]
        assert len(path) == r["best_step"][s]
        got = pref.apply_path(orc, kw, (st[0][s], st[1][s], int(st[2][s])), path)
        assert np.array_equal(got["state"], r["best_state"][s]) and got["active"] == r["best_active"][s]
        assert got["gap"] == r["best_gap"][s] and got["applied"] == r["best_step"][s]
        # the weight: the probabilities along the path, multiplied with one rounding each
        slot, ps = int(r["best_beam"][s]), []
        for t in range(int(r["best_step"][s]) - 1, -1, -1):
            k, a, m2, e2 = r["steps"][s][t]["chosen"][slot]
            ps.append(r["steps"][s][t]["probs"][k][a])
            slot = k
        want = bref.path_log_prob(ps)
        assert abs(r["log_prob"][s] - want) <= (r["best_step"][s] + 2) * 2.0 ** -52 * (1 + abs(r["log_prob"][s]))
        if r["best_step"][s] == 0:
            assert r["log_prob"][s] == 0.0 and r["best_mant"][s] == 0.5 and r["best_exp"][s] == 1


def test_k1_follows_the_argmax(orc):
    r = bref.beam_replay(orc, bref.env_kw("q8-k1"), bref.starts(orc, "q8-k1"), 1, bref.oracle_probs(orc, "q8-k1"))
    for steps in r["steps"]:
        for st in steps:
            assert st["chosen"][0][1] == int(np.argmax(st["probs"][0])), "the lowest index among the largest p"


# ---------------------------------------------------------------- 4. the layers
def test_the_layers_carry_the_call(ppo):
    hdr = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()
    assert re.search(r"int32_t\s+ppo_beam_search_states\s*\(", hdr)
    assert "ppo_beam_search_states" in ppo._lib.SIGNATURES and len(ppo._lib.SIGNATURES["ppo_beam_search_states"]) == 21
    jl = open(os.path.join(ROOT, "julia", "ProximalPolicyOptimizationHIP.jl")).read()
    assert ":ppo_beam_search_states" in jl
    assert "ppo_beam_search_states" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sig = inspect.signature(ppo.beam_search_states_)
    assert list(sig.parameters) == ["env", "policy", "score", "degree", "active", "K", "path", "log"]
    assert sig.parameters["path"].default is False and sig.parameters["log"].default is False
    assert "beam_search_states_" in ppo.__all__ and ppo.BEAM_MAX_K == 256
    assert math.isclose(float(bref.log_prob(0.5, 1)), 0.0, abs_tol=0.0)
