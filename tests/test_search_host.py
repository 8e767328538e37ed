"""What the best-state search can be held to without a device: the binding table, the validation of caller-supplied env
states, the first-argmin bookkeeping, and that the cases tests/test_gpu_search.py runs really contain what it needs (the
reference is tests/search_ref.py)."""
import numpy as np
import pytest

import episodes_ref as ref
import search_ref as sref
from test_abi import _header_prototypes

NEW_SYMBOLS = ("ppo_env_set_internal", "ppo_env_get_active", "ppo_best_states", "ppo_search_best_states")


def test_binding_table_holds_the_new_symbols(ppo):
    protos = _header_prototypes()
    for name in NEW_SYMBOLS:
        assert name in ppo._lib.SIGNATURES and name in protos, name
        assert len(ppo._lib.SIGNATURES[name]) == protos[name], name
    for name in ("best_states_", "best_state_in_rollout", "single_trajectory_scores", "count_non_flips",
                 "search_best_states_", "check_internal"):
        assert callable(getattr(ppo, name)) and name in ppo.__all__, name
    assert callable(ppo.HipVecEnv.set_internal) and callable(ppo.HipVecEnv.active_quads)


def test_check_internal(ppo, orc):
    e = orc.Env(Q=8, max_actions=6, N=5, seed=ref.SEED)
    e.reset()
    sc, dg, act = e.score.copy(), e.degree.copy(), e.active.copy()
    a, b, c = ppo.check_internal(sc, dg, act, 8)
    assert a.dtype == np.int8 and b.dtype == np.int8 and c.dtype == np.uint32
    assert np.array_equal(a, sc) and np.array_equal(b, dg) and np.array_equal(c, act)
    assert (act == 0x3F).all() and not sc[:, 24:].any() and not dg[:, 24:].any(), "a reset state: quads 0..5 active"
    bad = act.copy()
    bad[3] = 0
    with pytest.raises(ppo.PPOError, match="no active quad"):
        ppo.check_internal(sc, dg, bad, 8)
    bad = act.copy()
    bad[1] |= 1 << 8
    with pytest.raises(ppo.PPOError, match="at or above Q"):
        ppo.check_internal(sc, dg, bad, 8)
    for arr in (0, 1):
        s2, d2 = sc.copy(), dg.copy()
        (s2, d2)[arr][4, 27] = 1                           # quad 6 is inactive
        with pytest.raises(ppo.PPOError, match="inactive quad"):
            ppo.check_internal(s2, d2, act, 8)
    with pytest.raises(ppo.PPOError):
        ppo.check_internal(sc[:, :28], dg[:, :28], act, 8)
    # Q = 32: every bit of the word is a quad
    e = orc.Env(Q=32, max_actions=4, N=2, seed=ref.SEED)
    e.reset()
    full = np.full(2, 0xFFFFFFFF, np.uint32)
    ppo.check_internal(np.zeros((2, 128), np.int8), np.full((2, 128), 4, np.int8), full, 32)
    ppo.check_internal(e.score, e.degree, e.active, 32)


@pytest.mark.parametrize("gaps,want", [
    ([4, 2, 2, 3], (2, 1)),              # a tie returns the first
    ([3, 3, 5, 3], (3, 0)),              # the start wins when never improved
    ([5, 6, 4, 1], (1, 3)),              # the last step can win
    ([2, 0, 0, 0], (0, 1)),
    ([0], (0, 0)),
    ([6, 4, 4, 2, 2], (2, 3)),
])
def test_first_argmin_is_julias(gaps, want):
    assert sref.first_argmin(gaps) == want
    assert want == (min(gaps), int(np.argmin(gaps)))       # np.argmin, like Julia's argmin: the first minimum


@pytest.mark.parametrize("name", sref.COVERAGE_CASES)
def test_cases_contain_what_the_device_test_needs(orc, name):
    rec = sref.oracle_record(orc, ref.by_name(name))
    got = sref.coverage(rec)
    print(name, got)
    assert got == sref.COVERAGE[name]
    assert all(x >= 1 for x in got[1:])
    # the records agree with their own gap lists
    for i, g in enumerate(rec["gaps"]):
        assert rec["best_gap"][i] == min(g) and rec["best_step"][i] == int(np.argmin(g))
        assert rec["length"][i] == len(g) - 1 and rec["initial_gap"][i] == g[0] and min(g) >= 0
        assert rec["type_counts"][i].sum() == rec["length"][i]
        assert (rec["trace"][i, rec["length"][i]:] == sref.INT32_MIN).all()


def test_1x3_starts_on_its_optimum(orc):
    rec = sref.oracle_record(orc, ref.by_name("1x3"))
    assert rec["initial_gap"][0] == 0 and rec["best_gap"][0] == 0 and rec["best_step"][0] == 0
    assert len(rec["best_step"]) == 3


def test_search_shapes_hold_a_tie_for_the_best_gap(orc):
    """The lowest-clone rule is only exercised by a start whose best gap is held by two clones; the winner fields follow the
    rule; the rounds leave the ticks the schedule says."""
    tied = 0
    for shape in sref.SEARCH_SHAPES:
        M, K, N = shape
        rec = sref.search_reference(orc, shape)
        ts = sref.tied_starts(rec)
        print(shape, "tied starts", ts, "best gaps", rec["best_gap"].tolist(), "clones", rec["best_clone"].tolist())
        tied += len(ts)
        assert ts or shape != sref.TIED_SHAPE
        for s in range(M):
            assert rec["best_gap"][s] == rec["clone_gaps"][s].min()
            assert rec["best_clone"][s] == int(np.flatnonzero(rec["clone_gaps"][s] == rec["best_gap"][s])[0])
        S = N // K
        assert not rec["tick"][min(S, M) * K:].any(), "the envs behind the busiest round never play"
        assert (rec["tick"][:min(S, M) * K] >= 1).all()
    assert tied >= 1
