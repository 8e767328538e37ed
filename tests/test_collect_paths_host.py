"""The host reference of the teacher-forced collection (tests/collect_paths_ref.py) without a device: that the path sets of
tests/test_gpu_collect_paths.py contain what matters -- a case missing from them fails here instead of going untested --
and that the reference obeys its own rule."""
import numpy as np

import collect_paths_ref as cref
import episodes_ref as ref
import path_ref as pref
import resample_ref as rref
import search_ref as sref


def test_the_path_sets_contain_what_matters(orc):
    exp = cref.reference(orc, "h256-12x9")
    shape = cref.by_name("h256-12x9")
    starts, paths = cref.inputs(orc, shape)
    N, M, T = shape["N"], shape["M"], cref.Q8_MAX_ACTIONS
    lens, played = exp["lengths"], exp["played"]
    print("q8 declared", lens.tolist(), "played", played.tolist(), "end gaps",
          [sref.score_gap(exp["env"]["score"][n], int(exp["env"]["active"][n]))[1] for n in range(M)])
    # an empty path; a path of exactly stride entries without padding; a path of exactly max_actions steps
    assert lens[0] == 0 and played[0] == 0 and not exp["valid"][:, 0].any()
    assert lens[1] == paths.shape[1] == cref.Q8_STRIDE and not (paths[1] < 0).any() and played[1] == T < lens[1]
    assert lens[2] == T == played[2]
    assert exp["T"] == cref.Q8_STRIDE > T and not exp["valid"][T:].any(), "rows behind max_actions: every env idles"
    # a path that reaches the optimum before its entries end: the entries behind that point are never played
    assert lens[3] == played[3] + 3 and exp["gap_after"][played[3] - 1, 3] == 0 and exp["env"]["done"][3]
    assert exp["done"][played[3] - 1, 3] and not exp["valid"][played[3]:, 3].any() and played[3] < T
    # paths cut short of the optimum (truncated in the sense of 7f), by their last entry and by the time limit
    cut = cref.cut_transitions(exp)
    by_entry = [n for n in range(M) if 0 < lens[n] == played[n] < T and cut[lens[n] - 1, n]]
    assert set(by_entry) >= {4, 5, 6} and cut[T - 1, 1] and cut[T - 1, 2] and not cut[:, 3].any()
    assert all(not exp["env"]["done"][n] for n in by_entry), "a path's end is not the env's terminal"
    assert cut.sum() == cut.any(axis=0).sum() >= 5, "at most one cut per path"
    # M < N leaves idle envs; M == N is there too
    assert M < N and not exp["valid"][:, M:].any() and (exp["actions"][:, M:] == -1).all()
    assert any(s["M"] == s["N"] for s in cref.SHAPES)
    # paths taken from path_ref's search references, replayed to the search's own result
    found = pref.resample_reference(orc, "B")
    for row, s in ((3, cref.SOLVED_START), (4, 0), (7, 1), (8, 2)):
        n = int(found["best_step"][s])
        assert n > 0 and np.array_equal(paths[row, :n], found["path"][s, :n]) and played[row] == n
        end = np.concatenate([exp["env"]["score"][row], exp["env"]["degree"][row]])
        assert np.array_equal(end, found["best_state"][s]) and exp["env"]["active"][row] == found["best_active"][s]
    assert found["best_gap"][cref.SOLVED_START] == 0
    # one path with an action on an inactive quad, played in the middle of its path
    off = cref.reference(orc, cref.OFFQUAD_SHAPE["name"])
    r, t = cref.OFFQUAD_ROW, cref.OFFQUAD_STEP
    a = int(off["actions"][t, r])
    assert a >= 0 and not (int(off["active"][t, r]) >> (a >> 4)) & 1
    assert not off["valid"][t, r] and off["p_sel"][t, r] == 0 and off["rewards"][t, r] == cref.NO_ACTION_REWARD
    assert off["valid"][t + 1, r] and off["valid"].sum() == off["played"].sum() - 1 and off["env"]["tick"][r] == 3
    # Q = 32: the same three lengths
    q32 = cref.reference(orc, "q32-6x5")
    assert q32["lengths"].tolist()[:3] == [0, cref.Q32_STRIDE, cref.Q32_MAX_ACTIONS]
    assert q32["played"].tolist()[1:3] == [cref.Q32_MAX_ACTIONS] * 2 and (q32["actions"].max() >= 128), "an action beyond Q = 8's range"


def test_the_reference_obeys_its_rule(orc):
    for shape in cref.SHAPES + [cref.OFFQUAD_SHAPE]:
        exp = cref.reference(orc, shape["name"])
        starts, paths = cref.inputs(orc, shape)
        N, M, T = shape["N"], shape["M"], exp["T"]
        idle = exp["actions"] < 0
        assert not exp["valid"][idle].any() and ((~idle & ~exp["valid"]).sum() == 0 or shape is cref.OFFQUAD_SHAPE)
        assert (exp["p_sel"][idle] == 0).all() and (exp["rewards"][idle] == 0).all() and (exp["done"][idle] == 1).all()
        assert (exp["p_sel"][exp["valid"]] > 0).all()
        assert np.array_equal(exp["index"], ref.env_major_index(exp["valid"])) and len(exp["index"]) == exp["valid"].sum()
        # every path is a whole episode: its last played transition is done, none before it
        for n in range(M):
            ts = np.flatnonzero(~idle[:, n])
            assert np.array_equal(ts, np.arange(exp["played"][n])) and (len(ts) == 0 or exp["done"][ts[-1], n])
            assert not exp["done"][ts[:-1], n].any()
            # the state in front of step t + 1 is the state behind step t: the actions of column n replay on the oracle
            back = pref.apply_path(orc, cref.env_kw(shape), (starts[0][n], starts[1][n], int(starts[2][n])),
                                   exp["actions"][ts, n]) if shape is not cref.OFFQUAD_SHAPE else None
            if back is not None:
                assert back["applied"] == exp["played"][n]
                assert np.array_equal(back["state"], np.concatenate([exp["env"]["score"][n], exp["env"]["degree"][n]]))
        # ticks advance by the steps played, episode counters stay, the envs behind M are untouched
        b, a = exp["env_before"], exp["env"]
        assert np.array_equal(a["tick"][:M].astype(np.int64), b["tick"][:M].astype(np.int64) + exp["played"])
        assert np.array_equal(a["episode"], b["episode"])
        assert all(np.array_equal(a[k][M:], b[k][M:]) for k in a)
        # returns: the scan of orc.compute_returns over each path's own transitions (a path is an episode)
        for n in range(M):
            k = int(exp["played"][n])
            if k:
                want = orc.compute_returns(exp["rewards"][:k, n], exp["done"][:k, n], cref.DISCOUNT)
                assert np.array_equal(exp["returns"][:k, n], want)


def test_reward_identity_on_the_reference(orc):
    """What the closure test on the device relies on: the sum of a path's raw rewards is score(start) - score(end) plus
    no_action_reward per rejected move; it equals initial_gap - end_gap where no move was rejected and opt_score did not move
    -- and NOT in general (moves of types 2 and 3 change the sum of the vertex scores)."""
    exp = cref.reference(orc, "h256-12x9")
    starts, _ = cref.inputs(orc, cref.by_name("h256-12x9"))
    exact, moved = 0, 0
    for n in range(9):
        total, dscore, rejected, opt_moved = cref.reward_identity(exp, starts, n)
        assert total == dscore + cref.NO_ACTION_REWARD * rejected, n
        g0 = sref.score_gap(starts[0][n], int(starts[2][n]))[1]
        g1 = sref.score_gap(exp["env"]["score"][n], int(exp["env"]["active"][n]))[1]
        if rejected == 0 and not opt_moved:
            assert total == g0 - g1
            exact += 1
        moved += int(opt_moved)
    print("paths where the sum of rewards is initial_gap - end_gap:", exact, "of 9; opt_score moved on", moved)
    assert moved >= 1, "initial_gap - end_gap is not the sum of the rewards in general: the device test holds the paths to the general identity"
