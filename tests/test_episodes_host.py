"""tests/episodes_ref.py checked against itself and the oracle, without a device: the two restatements of the episodes form
(orc.collect_rollouts_tn cut at the quota, and the reference's loops step by step) agree, the evaluator values of a played
record are those of the loops, the env-major flat returns are the [T, N] scan's, and the case tables of
tests/test_gpu_episodes_form.py reach the branches they are there for: a case that does not fails here, not silently on
the GPU."""
import numpy as np
import pytest

import episodes_ref as ref


def _all_columns(orc, kw, params, hid, L, ne):
    exp = ref.expected_episodes(orc, kw, params, hid, L, ne)
    T = -(-ne // kw["num_envs"]) * kw["max_actions"]
    return exp, ref.assemble(exp, kw["num_envs"], T, 4 * kw["Q"])


def test_cut_reproduces_the_step_by_step_replay(orc):
    """1 env, 2 episodes of up to 128 steps (tests/test_gpu_parity.py::test_rollout_episodes_mode_plumbing)."""
    kw = dict(num_envs=1, Q=8, max_actions=128, seed=5)
    p = orc.glorot_params(72, 128, 2, seed=2)
    col = ref.expected_episodes(orc, kw, p, 128, 2, 2)[0]
    loop = ref.play_column(orc, kw, 0, p, 128, 2, 2)
    assert col["length"] == sum(loop["lengths"]) and int(col["done"].sum()) == 2 and col["done"][-1]
    for k in ("actions", "p_sel", "rewards", "done"):
        assert col[k].tobytes() == loop[k].tobytes(), k
    assert col["episode_after"] == 3 and col["tick_after"] == col["length"]


@pytest.mark.parametrize("kind", ["return", "best", "normalized"])
def test_evaluator_values_reproduce_the_loops(orc, kind):
    """3 envs, 8 trajectories, global id 107433 first (tests/test_gpu_parity.py::test_evaluator_variants): env 0 starts on
    its optimum, so its "normalized" trajectories are not the ones the rollout plays."""
    kw = dict(num_envs=3, Q=8, max_actions=9, seed=13, global_offset=107433)
    p = orc.glorot_params(72, 128, 2, seed=5)
    exp, cols = _all_columns(orc, kw, p, 128, 2, 8)
    rec = ref.teacher_forced(orc, kw, cols["actions"], 8)
    assert np.array_equal(rec["valid"], cols["valid"])
    quota = ref.quotas(3, 8)
    loops = [ref.play_column(orc, kw, n, p, 128, 2, int(quota[n]), kind) for n in range(3)]
    want = np.concatenate([l["values"] for l in loops])
    tab = ref.skip_table(orc, kw, 8)
    assert tab[0, 0] and tab.sum() == 1
    skip = {0: loops[0]["values"]} if kind == "normalized" else None
    got = ref.evaluator_values(kind, rec, skip)
    assert got.shape == (8,) and np.array_equal(got, want)
    if kind == "normalized":
        assert loops[0]["skipped"] == [True, False, False] and want[0] == 1.0
        # the skip shifts env 0's later trajectories: they start from the same resets one tick count earlier
        played = ref.evaluator_values(kind, rec)
        assert played[0] == 1.0 and np.array_equal(played[3:], want[3:])


def test_flat_returns_are_the_scan_over_the_ragged_buffer(orc):
    case = ref.by_name("70x100")
    kw = ref.env_kw_of(case)
    exp, cols = _all_columns(orc, kw, ref.policy_params(orc, case), case["hid"], case["L"], case["episodes"])
    index = ref.env_major_index(cols["valid"])
    assert index.size == cols["valid"].sum() and np.array_equal(np.sort(index), np.flatnonzero(cols["valid"].reshape(-1)))
    assert index[0] == 0 and index[1] == 70                  # env 0's rows first, in time order
    for g in (1.0, 0.99, np.float32(0.97)):
        tn = orc.compute_returns_tn(cols["rewards"], cols["done"], float(g), isinstance(g, np.float32))
        assert ref.flat_returns(orc, cols["rewards"], cols["done"], index, g).tobytes() == tn.reshape(-1)[index].tobytes()
    # teacher-forcing the oracle's own actions gives the oracle's buffer back
    rec = ref.teacher_forced(orc, kw, cols["actions"], case["episodes"])
    for k in ("states", "active", "rewards", "done", "valid"):
        assert np.array_equal(rec[k], cols[k]), k
    assert np.array_equal(rec["episode"], [exp[n]["episode_after"] for n in range(70)])
    assert np.array_equal(rec["tick"], [exp[n]["tick_after"] for n in range(70)])


@pytest.mark.parametrize("case", ref.ROLLOUT_CASES, ids=lambda c: c["name"])
def test_rollout_cases_hold_ragged_columns(orc, case):
    N, ne, M = case["N"], case["episodes"], case["M"]
    quota = ref.quotas(N, ne)
    assert quota.sum() == ne and quota.max() <= 3 and 4 <= M <= 6 and -(-ne // N) * M <= 18
    if case["Q"] != 8:
        assert not case["short"]                             # no Q = 32 id among the first 20,000 resets onto its optimum
        return
    assert case["short"] and set(case["short"]) <= set(case["special"])
    exp = ref.expected_episodes(orc, ref.env_kw_of(case), ref.policy_params(orc, case), case["hid"], case["L"], ne,
                                case["short"])
    for n in case["short"]:
        assert ref.ON_OPTIMUM[case["goff"] + n] == 1
        ends = np.flatnonzero(exp[n]["done"]) + 1
        assert ends.size == quota[n] >= 1 and ends[0] < M, "the env named short plays a full-length first episode"
        if quota.max() >= 2:                                 # followed by another episode in the same column
            assert quota[n] >= 2 and exp[n]["length"] > ends[0]


def test_evaluator_cases_take_the_skip_in_three_places(orc):
    first_with_more = later_after_played = last = quota3 = 0
    for case in ref.EVAL_CASES:
        tab = ref.skip_table(orc, ref.env_kw_of(case), case["episodes"])
        quota = ref.quotas(case["N"], case["episodes"])
        envs = np.flatnonzero(tab.any(axis=0))
        assert set(envs.tolist()) <= set(case["special"]), (case["name"], envs)
        for n in envs:
            for j in np.flatnonzero(tab[:, n]):
                first_with_more += int(j == 0 and quota[n] > 1)
                later_after_played += int(j > 0 and not tab[:j, n].all())
                last += int(j == quota[n] - 1)
                quota3 += int(quota[n] == 3)
    assert first_with_more >= 1 and later_after_played >= 1 and last >= 1 and quota3 >= 1
    c = ref.by_name("200x400")
    tab = ref.skip_table(orc, ref.env_kw_of(c), 400)
    assert tab[:, 14].tolist() == [False, True] and tab[:, 173].tolist() == [True, False] and tab.sum() == 2
    for name, n, where in (("20x60-last", 7, 2), ("20x60-middle", 5, 1), ("20x60-first", 11, 0)):
        tab = ref.skip_table(orc, ref.env_kw_of(ref.by_name(name)), 60)
        assert np.flatnonzero(tab[:, n]).tolist() == [where] and tab.sum() == 1


@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c["name"])
def test_replayed_columns_cover_the_edges(case):
    N, ne = case["N"], case["episodes"]
    cols = set(ref.replay_columns(case))
    quota = ref.quotas(N, ne)
    assert {0, N - 1} <= cols and set(case["special"]) <= cols
    for m in (64, 256, 512):
        if m < N:
            assert {m - 1, m} <= cols
    for n in range(1, N):                                    # every place where the quota changes, the idle boundary included
        if quota[n] != quota[n - 1]:
            assert {n - 1, n} <= cols, n
    if N <= 70:
        assert cols == set(range(N))


def test_case_tables_are_the_sizes_asked_for():
    sizes = {(c["N"], c["episodes"]) for c in ref.ROLLOUT_CASES}
    assert {(1, 3), (64, 64), (70, 100), (130, 5), (257, 515), (300, 450), (600, 520), (20, 30), (40, 60)} <= sizes
    assert {(c["N"], c["episodes"]) for c in ref.EVAL_CASES} >= {(64, 64), (70, 100), (130, 5), (200, 400), (300, 450),
                                                                 (600, 900), (20, 30), (40, 60)}
    q32 = [c for c in ref.ROLLOUT_CASES if c["Q"] == 32]
    assert {(c["N"], c["episodes"]) for c in q32} == {(20, 30), (70, 100)} and all(c["forms"] == ref.BOTH for c in q32)
    assert ref.by_name("70x100")["forms"] == ref.BOTH and ref.by_name("300x450-h256")["forms"] == ref.BOTH
    assert ref.by_name("300x450-h256")["hid"] == 256 and ref.by_name("L3-40x60")["L"] == 3
    assert ref.quotas(257, 515).tolist() == [3] + [2] * 256 and ref.quotas(600, 520)[519:521].tolist() == [1, 0]
