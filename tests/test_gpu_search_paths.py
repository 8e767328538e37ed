"""The action paths on the device (ppo_best_states_actions, ppo_search_best_states_path, ppo_search_resample_states_path,
ppo_env_apply_paths) against the CPU oracle.  Every comparison is exact equality.  tests/path_ref.py holds the
reference; tests/test_search_paths_host.py checks it without a device and asserts that the shapes contain what matters here:
results taken at an event fold after 4 to 12 copies along the lineage, a path only the fold keeps, empty paths, a path that
ends on a solved state.

1. best_states_(actions=True): the oracle's own actions of the trajectories, every other field as without them;
2. search_best_states_(path=True) against the reference, every other field as without the path;
3. search_resample_states_(path=True) on all eight shapes: the path against the reference; every other field, the donors log,
   ticks, episode counters and done flags against resample_ref.reference and against the device call without the path;
4. apply_paths_ against step_one on ragged paths at Q = 8 and Q = 32, and the refused arguments;
5. closure: apply_paths_(starts, path) gives best_state, best_active, best_gap with applied == best_step for every search
   above (inside 2 and 3) and for one K = 4096 resampling call with 64 survivors, where no CPU replay exists."""
import numpy as np
import pytest

import episodes_ref as ref
import path_ref as pref
import resample_ref as rref
import search_ref as sref

pytestmark = pytest.mark.gpu

RESULT = ("best_state", "best_active", "best_gap", "best_clone", "best_step", "initial_gap")


@pytest.fixture(scope="module")
def P(ppo):
    if ppo.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests must run on the GPU box")
    return ppo


def _policy(P, orc, hid, L, pseed):
    pol = P.HipPolicy(ref.F, hid, L, 4, seed=0)
    pol.params = orc.glorot_params(ref.F, hid, L, seed=pseed)
    return pol


def _mismatches(got, want, fields):
    return {k: int(np.count_nonzero(np.asarray(got[k]) != np.asarray(want[k]))) if np.shape(got[k]) == np.shape(want[k])
            else (np.shape(got[k]), np.shape(want[k])) for k in fields if not np.array_equal(got[k], want[k])}


def _env_state(P, env):
    it = env.internal()
    return dict(tick=it["tick"].copy(), episode=it["episode"].copy(), done=P.is_terminal(env).copy())


def _assert_closes(P, env, starts, got):
    """apply_paths_(starts, path) on the device: best_state, best_active, best_gap, and best_step actions applied."""
    before = _env_state(P, env)
    back = P.apply_paths_(env, *starts, got["path"])
    bad = _mismatches(dict(best_state=back["state"], best_active=back["active"], best_gap=back["gap"], best_step=back["applied"]),
                      got, ("best_state", "best_active", "best_gap", "best_step"))
    assert not bad, bad
    after = _env_state(P, env)
    assert all(np.array_equal(before[k], after[k]) for k in before), "apply_paths_ leaves the resident envs alone"


# ---------------------------------------------------------------- 1. best_states_ with the trajectories' actions
@pytest.mark.parametrize("name", sref.COVERAGE_CASES)
def test_best_states_actions(P, orc, name):
    case = ref.by_name(name)
    kw, nt = ref.env_kw_of(case), case["episodes"]
    pol = _policy(P, orc, case["hid"], case["L"], case["pseed"])
    want, rec = pref.one_based(pref.trajectory_actions(orc, case)), sref.oracle_record(orc, case)
    env = P.HipVecEnv(**kw)
    got = P.best_states_(env, pol, nt, scores=True, action_types=True, actions=True)
    assert env.error_flags() & ~32 == 0
    assert got["actions"].dtype == np.int16 and got["actions"].shape == (nt, case["M"])
    bad = int(np.count_nonzero(got["actions"] != want))
    print(name, "trajectories", nt, "action mismatches", bad)
    assert bad == 0
    assert np.array_equal((got["actions"] > 0).sum(axis=1), got["length"]), "0 behind a trajectory's end, and only there"
    fields = ("best_state", "best_active", "best_gap", "best_step", "length", "initial_gap", "trace", "type_counts")
    assert not _mismatches(got, rec, fields)
    env2 = P.HipVecEnv(**kw)
    plain = P.best_states_(env2, pol, nt, scores=True, action_types=True)
    assert "actions" not in plain and not _mismatches(plain, got, fields)
    assert all(np.array_equal(env.internal()[k], env2.internal()[k]) for k in ("tick", "episode"))
    # closure: the first best_step actions of a trajectory lead from its start to its best state.  Every env's first
    # trajectory starts from the reset with episode counter 1
    N = case["N"]
    first = np.cumsum(np.concatenate([[0], ref.quotas(N, nt)[:-1]]))
    o = ref._env(orc, kw)
    o.episode[:] = 1
    o.reset()
    prefix = got["actions"][first].copy()
    prefix[np.arange(case["M"])[None, :] >= got["best_step"][first][:, None]] = 0
    back = P.apply_paths_(env, o.score, o.degree, o.active.astype(np.uint32), prefix)
    assert np.array_equal(back["state"], got["best_state"][first]) and np.array_equal(back["gap"], got["best_gap"][first])
    assert np.array_equal(back["active"], got["best_active"][first]) and np.array_equal(back["applied"], got["best_step"][first])


# ---------------------------------------------------------------- 2. best-of-K search with the winner's path
@pytest.mark.parametrize("shape", sref.SEARCH_SHAPES, ids=lambda s: "M%d-K%d-N%d" % s)
def test_search_path(P, orc, shape):
    M, K, N = shape
    want = pref.search_reference(orc, shape)
    c = sref.SEARCH_CASE
    pol = _policy(P, orc, c["hid"], c["L"], c["pseed"])
    starts = sref.search_starts(orc, M)
    env, env2 = P.HipVecEnv(**sref.search_env_kw(N)), P.HipVecEnv(**sref.search_env_kw(N))
    got = P.search_best_states_(env, pol, *starts, K, clone_gaps=True, path=True)
    assert env.error_flags() & ~32 == 0
    assert got["path"].dtype == np.int16 and got["path"].shape == (M, c["M"])
    bad = _mismatches(got, dict(want, path=pref.one_based(want["path"])), RESULT + ("path",))
    print(shape, "path lengths", want["best_step"].tolist(), "mismatches", bad)
    assert not bad, (shape, bad)
    plain = P.search_best_states_(env2, pol, *starts, K, clone_gaps=True)
    assert "path" not in plain and not _mismatches(plain, got, RESULT + ("clone_gaps",))
    assert all(np.array_equal(a, b) for a, b in zip(_env_state(P, env).values(), _env_state(P, env2).values()))
    _assert_closes(P, env, starts, got)


# ---------------------------------------------------------------- 3. resampling search with the lineage's path
@pytest.mark.parametrize("name", list(rref.SHAPES))
def test_resample_path(P, orc, name):
    M, K, N, T, R, m0 = rref.SHAPES[name]
    want, old = pref.resample_reference(orc, name), rref.reference(orc, name)
    pol = _policy(P, orc, rref.CASE["hid"], rref.CASE["L"], rref.CASE["pseed"])
    kw = rref.env_kw(rref.SHAPES[name])
    starts = sref.search_starts(orc, M)
    env, env2 = P.HipVecEnv(**kw), P.HipVecEnv(**kw)
    before = _env_state(P, env)
    got = P.search_resample_states_(env, pol, *starts, K, R, m0, donors=True, clone_gaps=True, path=True)
    assert env.error_flags() & ~32 == 0
    assert got["path"].dtype == np.int16 and got["path"].shape == (M, T)
    bad = int(np.count_nonzero(got["path"] != pref.one_based(want["path"])))
    print(name, rref.SHAPES[name], "fold event", want["fold_event"].tolist(), "copies", want["copies"].tolist(), "path lengths",
          want["best_step"].tolist(), "path mismatches", bad)
    assert bad == 0, (name, bad)
    fields = RESULT + ("donors", "clone_gaps")
    assert not _mismatches(got, old, fields), "against resample_ref.reference"
    plain = P.search_resample_states_(env2, pol, *starts, K, R, m0, donors=True, clone_gaps=True)
    assert "path" not in plain and not _mismatches(plain, got, fields), "against the call without the path"
    a, b = _env_state(P, env), _env_state(P, env2)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert np.array_equal(a["episode"], before["episode"]) and np.array_equal(a["tick"].astype(np.int64), old["tick"])
    assert a["done"][old["played"]].all() and np.array_equal(a["done"][~old["played"]], before["done"][~old["played"]])
    _assert_closes(P, env, starts, got)


def test_resample_path_at_the_cap(P, orc):
    """K = 4096, 64 survivors, the shape of test_gpu_resample.test_k_at_the_cap: too many env-steps for the CPU replay, so
    the path is held to the closure alone, and the other fields to the call without the path."""
    K, T, m0 = 4096, 4, 64
    kw = rref.env_kw((1, K, K, T, 1, K))
    pol = _policy(P, orc, rref.CASE["hid"], rref.CASE["L"], rref.CASE["pseed"])
    starts = sref.search_starts(orc, 1)
    env, env2 = P.HipVecEnv(**kw), P.HipVecEnv(**kw)
    got = P.search_resample_states_(env, pol, *starts, K, 1, m0, donors=True, clone_gaps=True, path=True)
    plain = P.search_resample_states_(env2, pol, *starts, K, 1, m0, donors=True, clone_gaps=True)
    assert env.error_flags() & ~32 == 0
    assert not _mismatches(plain, got, RESULT + ("donors", "clone_gaps"))
    assert (got["donors"] >= 0).any(), "copies ran"
    assert int((got["path"][0] > 0).sum()) == got["best_step"][0]
    print("K = 4096: best step", got["best_step"].tolist(), "best gap", got["best_gap"].tolist(), "receivers",
          int((got["donors"] >= 0).sum()))
    _assert_closes(P, env, starts, got)


# ---------------------------------------------------------------- 4. apply_paths_ against step_one
@pytest.mark.parametrize("name", list(pref.APPLY_CASES))
def test_apply_paths_against_oracle(P, orc, name):
    kw, starts, paths = pref.apply_inputs(orc, name)
    N, V = kw["num_envs"], 4 * kw["Q"]
    want = [pref.apply_path(orc, kw, (starts[0][i], starts[1][i], int(starts[2][i])), paths[i]) for i in range(N)]
    env = P.HipVecEnv(**kw)
    before = _env_state(P, env)
    got = P.apply_paths_(env, *starts, pref.one_based(paths), scores=True)
    assert got["state"].shape == (N, 2 * V) and got["trace"].shape == paths.shape
    assert np.array_equal(got["state"], np.stack([w["state"] for w in want]))
    assert np.array_equal(got["score"], got["state"][:, :V]) and np.array_equal(got["degree"], got["state"][:, V:])
    for k in ("active", "gap", "applied"):
        assert np.array_equal(got[k], np.array([w[k] for w in want])), k
    trace = np.full(paths.shape, sref.INT32_MIN, np.int64)
    for i, w in enumerate(want):
        trace[i, :w["applied"]] = w["trace"]
    assert np.array_equal(got["trace"], trace), "INT32_MIN behind applied"
    print(name, "lengths", (paths >= 0).sum(axis=1).tolist(), "applied", got["applied"].tolist())
    # a row without any padding: stride equals the path's length
    for i in (1, 2):
        n = int((paths[i] >= 0).sum())
        one = P.apply_paths_(env, starts[0][i:i + 1], starts[1][i:i + 1], starts[2][i:i + 1], pref.one_based(paths[i:i + 1, :n]))
        assert one["applied"][0] == want[i]["applied"] and np.array_equal(one["state"][0], want[i]["state"])
    assert "trace" not in one
    after = _env_state(P, env)
    assert all(np.array_equal(before[k], after[k]) for k in before), "the resident envs, ticks and counters are unchanged"
    assert env.error_flags() == 0


def test_apply_paths_refuses_bad_arguments(P, orc):
    kw, starts, paths = pref.apply_inputs(orc, "q8")
    env = P.HipVecEnv(**kw)
    ok = pref.one_based(paths)
    big = ok.copy()
    big[3, 0] = 16 * kw["Q"] + 1
    for bad in (big, ok[:-1], ok[:, :0]):
        with pytest.raises(P.PPOError) as err:
            P.apply_paths_(env, *starts, bad)
        assert err.value.status == -1
    with pytest.raises(P.PPOError, match="no active quad"):
        P.apply_paths_(env, starts[0], starts[1], np.zeros_like(starts[2]), ok)
    # the C entry point checks the same itself
    N, V = kw["num_envs"], 4 * kw["Q"]
    L = P._lib
    ptr = lambda a, t: a.ctypes.data_as(t)
    st, act, gap, app = np.zeros((N, 2 * V), np.int8), np.zeros(N, np.uint32), np.zeros(N, np.int32), np.zeros(N, np.int32)
    raw = np.ascontiguousarray(paths)

    def status(active, rows, stride):
        return L.lib().ppo_env_apply_paths(env._h, N, ptr(starts[0], L.c_i8p), ptr(starts[1], L.c_i8p), ptr(active, L.c_u32p),
                                           ptr(rows, L.c_i16p), stride, ptr(st, L.c_i8p), ptr(act, L.c_u32p),
                                           ptr(gap, L.c_i32p), ptr(app, L.c_i32p), None)
    over = raw.copy()
    over[3, 0] = 16 * kw["Q"]
    assert status(starts[2], raw, raw.shape[1]) == 0
    assert status(starts[2], over, raw.shape[1]) == -1 and status(starts[2], raw, 0) == -1
    assert status(np.zeros_like(starts[2]), raw, raw.shape[1]) == -1
    # an action on an inactive quad: the step counts and changes nothing (step! does the same); the call reports the flag
    off = int(np.flatnonzero([not (int(starts[2][4]) >> q) & 1 for q in range(kw["Q"])])[0])
    one = np.full((1, 2), -1, np.int16)
    one[0, 0] = 16 * off
    st1, act1, gap1, app1 = np.zeros((1, 2 * V), np.int8), np.zeros(1, np.uint32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    s = L.lib().ppo_env_apply_paths(env._h, 1, ptr(starts[0][4:5], L.c_i8p), ptr(starts[1][4:5], L.c_i8p),
                                    ptr(starts[2][4:5], L.c_u32p), ptr(one, L.c_i16p), 2, ptr(st1, L.c_i8p), ptr(act1, L.c_u32p),
                                    ptr(gap1, L.c_i32p), ptr(app1, L.c_i32p), None)
    assert s == -3 and app1[0] == 1 and np.array_equal(st1[0], np.concatenate([starts[0][4], starts[1][4]]))
    assert env.error_flags() == 0 and not env.internal()["tick"].any(), "the env handle's own flags and ticks are untouched"
