"""The distinct beam on the device (ppo_beam_search_states_distinct: k_beam_select_window, k_beam_children, k_beam_commit;
DESIGN.md 7p) against tests/beam_distinct_ref.py.  Every comparison is exact equality: the walk rounds nothing that the plain
beam does not.  tests/test_beam_distinct_host.py checks the reference without a device and asserts that the shapes contain
what matters here: results the plain beam does not reach, an empty beam, steps the budget cuts short, steps of up to four
windows, walks that stop inside a later window, candidates that run out below K.

1. exact replay: probs_of is the device's own ppo_policy_forward of the states the replay holds (as tests/test_gpu_beam.py
   closes its loop; that file holds those rows equal to the oracle's); every returned field, the whole log with the mantissas
   bit for bit, rank, examined and the path equal the replay; apply_paths_ closes every path onto best_state; ticks, episode
   counters and the envs at and beyond S*K are untouched, the slots' envs terminal;
2. distinct=None returns byte for byte what beam_search_states_ returns, and the kernel-timing tables then hold
   launches of today's kernels only;
3. two envs of different seeds and prior ticks give identical dicts;
4. the refusals: distinct outside the three values, rounds outside 1 .. 16, and the plain call's refusals in a distinct call."""
import numpy as np
import pytest

import beam_distinct_ref as dref
import beam_ref as bref
import episodes_ref as ref
import path_ref as pref

pytestmark = pytest.mark.gpu

RESULT = ("best_state", "best_active", "best_gap", "best_step", "initial_gap", "best_beam")
LOG = ("parents", "actions", "mant", "exp", "rank", "examined")
NEW_KERNELS = ("k_beam_select_window", "k_beam_children", "k_beam_commit")


@pytest.fixture(scope="module")
def P(ppo):
    if ppo.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests must run on the GPU box")
    return ppo


def _policy(P, orc, name):
    c = bref.SHAPES[name]
    pol = P.HipPolicy(ref.F, c["hid"], c["L"], 4, seed=0)
    pol.params = bref.policy_params(orc, name)
    return pol


def _device_probs(P, pol):
    return lambda states, active: P.batch_action_probabilities(pol, P.StateData(states, active)).T.copy()


def _mismatches(got, want, fields):
    return {k: int(np.count_nonzero(np.asarray(got[k]) != np.asarray(want[k]))) if np.shape(got[k]) == np.shape(want[k])
            else (np.shape(got[k]), np.shape(want[k])) for k in fields if not np.array_equal(got[k], want[k])}


def _env_state(P, env):
    it = env.internal()
    return dict(tick=it["tick"].copy(), episode=it["episode"].copy(), done=P.is_terminal(env).copy(), score=it["score"].copy(),
                degree=it["degree"].copy())


def _expected(want):
    return dict(want, path=pref.one_based(want["path"]), parents=pref.one_based(want["parents"]),
                actions=pref.one_based(want["actions"]))


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


# ---------------------------------------------------------------- 1. the replay, case by case
@pytest.mark.parametrize("name,mode,rounds", dref.GPU_CASES, ids=["%s-%s-r%d" % c for c in dref.GPU_CASES])
def test_distinct_beam_against_replay(P, orc, name, mode, rounds):
    c = bref.SHAPES[name]
    K, M, T = c["K"], c["M"], c["T"]
    kw, starts = bref.env_kw(name), bref.starts(orc, name)
    pol = _policy(P, orc, name)
    env = P.HipVecEnv(**kw)
    P.collect_rollouts_steps_(P.BufferRollouts(), env, pol, 3, 1.0)      # ticks and episode counters off their initial values
    before = _env_state(P, env)
    got = P.beam_search_states_distinct_(env, pol, *starts, K, path=True, log=True, distinct=mode, rounds=rounds)
    assert env.error_flags() & ~32 == 0
    after = _env_state(P, env)
    want = dref.distinct_replay(orc, kw, starts, K, _device_probs(P, pol), mode, rounds)
    bad = _mismatches(got, _expected(want), RESULT + ("path",) + LOG)
    print(name, mode, rounds, "results", [dref.result(want, s) for s in range(M)],
          "accepted", [[x["n"] for x in steps] for steps in want["steps"]],
          "windows", [[dref.windows_used(x) for x in steps] for steps in want["steps"]],
          "cut", [sum(x["cut"] for x in steps) for steps in want["steps"]], "mismatches", bad)
    assert not bad, (name, mode, rounds, bad)
    assert got["rank"].dtype == np.int32 and got["rank"].shape == (M, T, K)
    assert got["examined"].dtype == np.int32 and got["examined"].shape == (M, T)
    assert _bits_equal(got["mant"], want["mant"]), "the mantissas, bit for bit"
    assert _bits_equal(got["log_prob"], want["log_prob"])
    # the optional outputs change nothing else
    plain = P.beam_search_states_distinct_(P.HipVecEnv(**kw), pol, *starts, K, distinct=mode, rounds=rounds)
    assert "path" not in plain and "rank" not in plain and "examined" not in plain
    assert not _mismatches(plain, got, RESULT) and _bits_equal(plain["log_prob"], got["log_prob"])
    # what the call leaves behind
    assert np.array_equal(after["tick"], before["tick"]) and np.array_equal(after["episode"], before["episode"])
    played = want["played"]
    assert after["done"][played].all(), "the slots' envs are left terminal"
    for k in ("done", "score", "degree"):
        assert np.array_equal(after[k][~played], before[k][~played]), "envs beyond S*K are untouched: " + k
    # closure on the device
    back = P.apply_paths_(env, *starts, got["path"])
    bad = _mismatches(dict(best_state=back["state"], best_active=back["active"], best_gap=back["gap"], best_step=back["applied"]),
                      got, ("best_state", "best_active", "best_gap", "best_step"))
    assert not bad, bad


# ---------------------------------------------------------------- 2. distinct=None is today's call
def test_distinct_none_is_the_plain_call(P, orc):
    name = "q8-k8"
    c, kw, starts = bref.SHAPES[name], bref.env_kw(name), bref.starts(orc, name)
    pol = _policy(P, orc, name)
    old = P.beam_search_states_(P.HipVecEnv(**kw), pol, *starts, c["K"], path=True, log=True)
    P.synchronize()
    P.profile_enable(True)
    try:
        new = P.beam_search_states_distinct_(P.HipVecEnv(**kw), pol, *starts, c["K"], path=True, log=True, distinct=None, rounds=99)
        P.synchronize()
        counts = {k: P.profile_get(k)[1] for k in NEW_KERNELS + ("k_beam_select", "k_beam_expand")}
        print("launches of a plain call:", counts)
        assert all(counts[k] == 0 for k in NEW_KERNELS), "a plain call launches today's kernels only"
        assert counts["k_beam_select"] == counts["k_beam_expand"] > 0
        P.beam_search_states_distinct_(P.HipVecEnv(**kw), pol, *starts, c["K"], distinct="parents", rounds=2)
        P.synchronize()
        after = {k: P.profile_get(k)[1] for k in counts}
        print("... and behind a distinct call:", after)
        assert after["k_beam_select"] == counts["k_beam_select"] and after["k_beam_expand"] == counts["k_beam_expand"]
        assert after["k_beam_select_window"] == after["k_beam_children"] == 2 * after["k_beam_commit"] > 0
    finally:
        P.profile_enable(False)
    assert set(old) == set(new) and "rank" not in new
    for k in old:
        assert np.asarray(old[k]).tobytes() == np.asarray(new[k]).tobytes() and old[k].dtype == new[k].dtype, k


# ---------------------------------------------------------------- 3. determinism and independence
def test_result_depends_on_neither_seed_nor_ticks(P, orc):
    name = "q8-k8"
    c, kw, starts = bref.SHAPES[name], bref.env_kw(name), bref.starts(orc, name)
    pol = _policy(P, orc, name)
    env_a = P.HipVecEnv(**kw)
    env_b = P.HipVecEnv(**dict(kw, seed=kw["seed"] + 77, global_offset=1000))
    P.collect_rollouts_steps_(P.BufferRollouts(), env_b, pol, 5, 1.0)
    tick_b = env_b.internal()["tick"].copy()
    assert tick_b.any()
    opts = dict(path=True, log=True, distinct="parents")
    a = P.beam_search_states_distinct_(env_a, pol, *starts, c["K"], **opts)
    b = P.beam_search_states_distinct_(env_b, pol, *starts, c["K"], **opts)
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(env_b.internal()["tick"], tick_b) and not env_a.internal()["tick"].any()
    again = P.beam_search_states_distinct_(env_a, pol, *starts, c["K"], **opts)                  # on envs the first call left terminal
    for k in a:
        assert np.array_equal(a[k], again[k]), k


# ---------------------------------------------------------------- 4. refusals
def test_refusals(P, orc):
    name = "q8-k3"
    c, kw, starts = bref.SHAPES[name], bref.env_kw(name), bref.starts(orc, name)
    pol = _policy(P, orc, name)
    env = P.HipVecEnv(**kw)
    before = _env_state(P, env)
    for bad in ("child", "Parents", "", 1, True, ("parents",)):
        with pytest.raises(P.PPOError, match="distinct") as err:
            P.beam_search_states_distinct_(env, pol, *starts, c["K"], distinct=bad)
        assert err.value.status == -1
    for bad in (0, -1, 17, 2.5, None):
        with pytest.raises(P.PPOError, match="rounds") as err:
            P.beam_search_states_distinct_(env, pol, *starts, c["K"], distinct="parents", rounds=bad)
        assert err.value.status == -1
    # what the plain call refuses, a distinct call refuses as well
    with pytest.raises(P.PPOError, match="1 <= K <= N") as err:
        P.beam_search_states_distinct_(env, pol, *starts, 0, distinct="children")
    assert err.value.status == -1
    wide = P.HipVecEnv(**dict(kw, num_envs=P.BEAM_MAX_K + 4))
    with pytest.raises(P.PPOError, match="K above 256") as err:
        P.beam_search_states_distinct_(wide, pol, *starts, P.BEAM_MAX_K + 1, distinct="parents")
    assert err.value.status == -4
    bf = P.HipPolicy(ref.F, c["hid"], c["L"], 4, seed=0, dtype="bf16")
    with pytest.raises(P.PPOError, match="bf16") as err:
        P.beam_search_states_distinct_(env, bf, *starts, c["K"], distinct="parents")
    assert err.value.status == -4
    with pytest.raises(P.PPOError, match="HipVecEnv"):
        P.beam_search_states_distinct_(object(), pol, *starts, c["K"], distinct="parents")
    # the C entry point refuses the same itself
    L = P._lib
    ptr = lambda a, t: a.ctypes.data_as(t)
    M, V = c["M"], 4 * c["Q"]
    scratch, h = P._evaluator_scratch(env)
    st, act, mant = np.zeros((M, 2 * V), np.int8), np.zeros(M, np.uint32), np.zeros(M, np.float64)
    ints = [np.zeros(M, np.int32) for _ in range(5)]
    rank = np.zeros((M, c["T"], c["K"]), np.int32)

    def status(policy, K, mode, rounds, rank_out=None):
        return L.lib().ppo_beam_search_states_distinct(
            policy._h, env._h, h, M, K, ptr(starts[0], L.c_i8p), ptr(starts[1], L.c_i8p), ptr(starts[2], L.c_u32p),
            ptr(st, L.c_i8p), ptr(act, L.c_u32p), ptr(ints[0], L.c_i32p), ptr(ints[1], L.c_i32p), ptr(ints[2], L.c_i32p),
            ptr(ints[3], L.c_i32p), ptr(mant, L.c_f64p), ptr(ints[4], L.c_i32p), None, None, None, None, None, mode, rounds,
            None if rank_out is None else ptr(rank_out, L.c_i32p), None)
    assert status(pol, c["K"], 3, 4) == -1 and "distinct" in L.last_error()
    assert status(pol, c["K"], -1, 4) == -1
    assert status(pol, c["K"], 2, 0) == -1 and "rounds" in L.last_error()
    assert status(pol, c["K"], 1, 17) == -1
    assert status(pol, c["K"], 0, 4, rank) == -1 and "distinct" in L.last_error()
    assert status(pol, 0, 2, 4) == -1 and "1 <= K <= N" in L.last_error()
    assert status(bf, c["K"], 2, 4) == -4 and "bf16" in L.last_error()
    assert env.error_flags() == 0
    after = _env_state(P, env)
    assert all(np.array_equal(before[k], after[k]) for k in before), "a refused call touches no env"
    assert status(pol, c["K"], 0, 99) == 0, "mode 0 is the plain call: rounds is not read"
