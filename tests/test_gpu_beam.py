"""Beam search on the device (ppo_beam_search_states, k_beam_select, k_beam_expand) against tests/beam_ref.py.
Every comparison but log_prob's is exact equality: the scoring rule is one fp64 multiply and an exact re-normalisation.
tests/test_beam_host.py checks the reference without a device and asserts that the shapes contain what matters here: dead slots,
starts that reach the optimum early and starts that never do, results off slot 0, shared and childless parents in one step,
partial rounds, exact weight ties.

1. exact replay: probs_of is the device's own ppo_policy_forward of the states the replay holds; every returned field, the
   whole log (parents, actions, mant, exp) and the path equal the replay; path=True and log=True change no other output;
   those probabilities also equal oracle.action_probabilities(mode="dev") on the replay's states, as the parity tests hold
   them, so the loop does not close on the device's word alone (every state; in q32-k256 alone a fixed sample of every third
   state, since an oracle forward at Q = 32 costs sixteen times one at Q = 8);
2. path closure: apply_paths_(starts, path) gives best_state, best_active, best_gap and applied == best_step (inside 1);
3. K = 1 is search_best_states_(K = 1) under selecting(policy, "greedy");
4. all parameters zero: every candidate of a live slot ties, the index alone decides; the log equals the replay;
5. determinism and independence: two envs of different seeds and prior ticks return identical dicts; ticks and episode
   counters are unchanged, the slots' envs terminal, the envs beyond them untouched (inside 1 as well);
6. log_prob against sum(log(float64(p))) along the path, tolerance (best_step + 2) * 2^-52 * (1 + |log_prob|): one fp64
   rounding per multiply plus the two host logs (inside 1);
7. refusals: K < 1, K > N, a bf16 policy, K above the staging limit, malformed starts -- code, message, env unflagged."""
import numpy as np
import pytest

import beam_ref as bref
import episodes_ref as ref
import path_ref as pref

pytestmark = pytest.mark.gpu

RESULT = ("best_state", "best_active", "best_gap", "best_step", "initial_gap", "best_beam")
LOG = ("parents", "actions", "mant", "exp")


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


def _one_based_log(want):
    return dict(parents=pref.one_based(want["parents"]), actions=pref.one_based(want["actions"]), mant=want["mant"], exp=want["exp"])


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


# ---------------------------------------------------------------- 1, 2, 5, 6. the replay, shape by shape
@pytest.mark.parametrize("name", bref.GPU_SHAPES)
def test_beam_against_replay(P, orc, name):
    c = bref.SHAPES[name]
    K, M, T = c["K"], c["M"], c["T"]
    kw, starts = bref.env_kw(name), bref.starts(orc, name)
    pol = _policy(P, orc, name)
    env = P.HipVecEnv(**kw)
    ro = P.BufferRollouts()
    P.collect_rollouts_steps_(ro, env, pol, 3, 1.0)              # ticks and episode counters off their initial values
    before = _env_state(P, env)
    got = P.beam_search_states_(env, pol, *starts, K, path=True, log=True)
    assert env.error_flags() & ~32 == 0
    after = _env_state(P, env)
    want = bref.beam_replay(orc, kw, starts, K, _device_probs(P, pol))
    cover = bref.coverage(want, K)
    bad = _mismatches(got, dict(want, path=pref.one_based(want["path"]), **_one_based_log(want)), RESULT + ("path",) + LOG)
    print(name, "coverage", cover, "best_step", want["best_step"].tolist(), "best_beam", want["best_beam"].tolist(), "mismatches", bad)
    assert not bad, (name, bad)
    assert got["path"].dtype == np.int16 and got["path"].shape == (M, T) and got["parents"].shape == (M, T, K)
    assert _bits_equal(got["mant"], want["mant"]), "the mantissas, bit for bit"
    assert _bits_equal(got["log_prob"], want["log_prob"]), "log(best_mant) + best_exp * log(2) of equal weights"
    assert np.array_equal(got["best_score"], got["best_state"][:, :4 * c["Q"]])
    # the optional outputs change nothing else
    for opts in (dict(), dict(path=True), dict(log=True)):
        env2 = P.HipVecEnv(**kw)
        plain = P.beam_search_states_(env2, pol, *starts, K, **opts)
        assert ("path" in plain) == bool(opts.get("path")) and ("parents" in plain) == bool(opts.get("log"))
        assert not _mismatches(plain, got, RESULT + tuple(k for k in ("path",) + LOG if k in plain)), opts
        assert _bits_equal(plain["log_prob"], got["log_prob"])
    # 5. what the call leaves behind
    assert np.array_equal(after["tick"], before["tick"]) and np.array_equal(after["episode"], before["episode"])
    played = want["played"]
    assert after["done"][played].all(), "the slots' envs are left terminal"
    for k in ("done", "score", "degree"):
        assert np.array_equal(after[k][~played], before[k][~played]), "envs beyond S*K are untouched: " + k
    # 2. closure on the device
    back = P.apply_paths_(env, *starts, got["path"])
    bad = _mismatches(dict(best_state=back["state"], best_active=back["active"], best_gap=back["gap"], best_step=back["applied"]),
                      got, ("best_state", "best_active", "best_gap", "best_step"))
    assert not bad, bad
    # 6. log_prob against the probabilities along the path
    for s in range(M):
        slot, ps = int(want["best_beam"][s]), []
        for t in range(int(want["best_step"][s]) - 1, -1, -1):
            k, a, _, _ = want["steps"][s][t]["chosen"][slot]
            ps.append(want["steps"][s][t]["probs"][k][a])
            slot = k
        ref_lp = bref.path_log_prob(ps)
        tol = (want["best_step"][s] + 2) * 2.0 ** -52 * (1 + abs(got["log_prob"][s]))
        print("   start", s, "log_prob", got["log_prob"][s], "sum log p", ref_lp, "tolerance", tol)
        assert abs(got["log_prob"][s] - ref_lp) <= tol
    # 1. the loop does not close on the device's word alone: the device's rows equal the oracle's device-order forward, as the
    # parity tests hold them.  Every state of the replay at Q = 8.  At Q = 32 an oracle forward costs sixteen times as much
    # (four times the rows, four times the actions), so q32-k256 -- some 1400 states -- is a SAMPLE of every third state, fixed
    # by the stride, which keeps the case within a few seconds; the replay equality above covers the states in between
    oracle_of = bref.oracle_probs(orc, name)
    states = np.concatenate([st["states"] for steps in want["steps"] for st in steps])
    active = np.concatenate([st["active"] for steps in want["steps"] for st in steps])
    probs = np.concatenate([st["probs"] for steps in want["steps"] for st in steps])
    stride = max(1, states.shape[0] // 400) if c["Q"] == 32 else 1
    differ = int(np.count_nonzero(oracle_of(states[::stride], active[::stride]).view(np.uint32) != probs[::stride].view(np.uint32)))
    print("   device probabilities that differ from the oracle's:", differ, "of", probs[::stride].size, "(every %d-th state)" % stride)
    assert differ == 0


# ---------------------------------------------------------------- 3. K = 1 is greedy
def test_k1_is_greedy(P, orc):
    name = "q8-k1"
    c, kw, starts = bref.SHAPES[name], bref.env_kw(name), bref.starts(orc, name)
    pol = _policy(P, orc, name)
    env, env2 = P.HipVecEnv(**kw), P.HipVecEnv(**kw)
    got = P.beam_search_states_(env, pol, *starts, 1, path=True)
    with P.selecting(pol, "greedy"):
        want = P.search_best_states_(env2, pol, *starts, 1, path=True)
    assert pol.selection == ("sample", 1.0)
    bad = _mismatches(got, want, ("best_state", "best_active", "best_gap", "best_step", "path"))
    print("K = 1: best_step", got["best_step"].tolist(), "mismatches", bad)
    assert not bad, bad
    assert not got["best_beam"].any()
    assert (got["best_step"] > 0).sum() >= 3 and (got["best_step"] > 1).any(), "the greedy trajectory improves: paths to compare"
    # the selection of the handle is not read
    with P.selecting(pol, "sample", 3.0, top_k=2):
        again = P.beam_search_states_(P.HipVecEnv(**kw), pol, *starts, 1, path=True)
    assert not _mismatches(again, got, RESULT + ("path",))


# ---------------------------------------------------------------- 4. all ties
def test_all_ties_are_decided_by_the_index(P, orc):
    name = "ties"
    c, kw, starts = bref.SHAPES[name], bref.env_kw(name), bref.starts(orc, name)
    K = c["K"]
    pol = _policy(P, orc, name)
    assert not pol.params.any()
    env = P.HipVecEnv(**kw)
    got = P.beam_search_states_(env, pol, *starts, K, path=True, log=True)
    want = bref.beam_replay(orc, kw, starts, K, _device_probs(P, pol))
    for s, steps in enumerate(want["steps"]):
        p0 = steps[0]["probs"][0]
        valid = np.flatnonzero(p0 > 0)
        assert len(set(p0[valid].tolist())) == 1, "every valid action of a state has the same probability"
        assert np.array_equal(got["actions"][s, 0], valid[:K] + 1), "step 0: the lowest indices, in index order"
        assert not (got["parents"][s, 0] != 1).any()
        assert all(st["index_decided"] for st in steps)
    bad = _mismatches(got, dict(want, path=pref.one_based(want["path"]), **_one_based_log(want)), RESULT + ("path",) + LOG)
    assert not bad, bad
    assert _bits_equal(got["mant"], want["mant"])


# ---------------------------------------------------------------- 5. determinism and independence
def test_result_depends_on_neither_seed_nor_ticks(P, orc):
    name = "q8-k8"
    c, kw, starts = bref.SHAPES[name], bref.env_kw(name), bref.starts(orc, name)
    pol = _policy(P, orc, name)
    env_a = P.HipVecEnv(**kw)
    env_b = P.HipVecEnv(**dict(kw, seed=kw["seed"] + 77, global_offset=1000))
    P.collect_rollouts_steps_(P.BufferRollouts(), env_b, pol, 5, 1.0)
    tick_b = env_b.internal()["tick"].copy()
    assert tick_b.any()
    a = P.beam_search_states_(env_a, pol, *starts, c["K"], path=True, log=True)
    b = P.beam_search_states_(env_b, pol, *starts, c["K"], path=True, log=True)
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(env_b.internal()["tick"], tick_b) and not env_a.internal()["tick"].any()
    again = P.beam_search_states_(env_a, pol, *starts, c["K"], path=True, log=True)      # on envs the first call left terminal
    for k in a:
        assert np.array_equal(a[k], again[k]), k


# ---------------------------------------------------------------- 7. refusals
def test_refusals(P, orc):
    name = "q8-k3"
    c, kw, starts = bref.SHAPES[name], bref.env_kw(name), bref.starts(orc, name)
    pol = _policy(P, orc, name)
    env = P.HipVecEnv(**kw)
    before = _env_state(P, env)
    for K in (0, -1, kw["num_envs"] + 1):
        with pytest.raises(P.PPOError, match="1 <= K <= N") as err:
            P.beam_search_states_(env, pol, *starts, K)
        assert err.value.status == -1
    wide = P.HipVecEnv(**dict(kw, num_envs=P.BEAM_MAX_K + 4))
    with pytest.raises(P.PPOError, match="K above 256") as err:
        P.beam_search_states_(wide, pol, *starts, P.BEAM_MAX_K + 1)
    assert err.value.status == -4
    bf = P.HipPolicy(ref.F, c["hid"], c["L"], 4, seed=0, dtype="bf16")
    with pytest.raises(P.PPOError, match="bf16") as err:
        P.beam_search_states_(env, bf, *starts, c["K"])
    assert err.value.status == -4
    with pytest.raises(P.PPOError, match="no active quad"):
        P.beam_search_states_(env, pol, starts[0], starts[1], np.zeros_like(starts[2]), c["K"])
    off = starts[0].copy()
    off[:, -1] = 1                                               # the last quad of a reset state is inactive
    with pytest.raises(P.PPOError, match="inactive quad"):
        P.beam_search_states_(env, pol, off, starts[1], starts[2], c["K"])
    with pytest.raises(P.PPOError):
        P.beam_search_states_(env, pol, starts[0][:-1], starts[1], starts[2], c["K"])
    with pytest.raises(P.PPOError, match="HipVecEnv"):
        P.beam_search_states_(object(), pol, *starts, c["K"])
    # the C entry point refuses the same itself
    L = P._lib
    ptr = lambda a, t: a.ctypes.data_as(t)
    M, V = c["M"], 4 * c["Q"]
    scratch, h = P._evaluator_scratch(env)
    st, act, mant = np.zeros((M, 2 * V), np.int8), np.zeros(M, np.uint32), np.zeros(M, np.float64)
    ints = [np.zeros(M, np.int32) for _ in range(5)]

    def status(e, policy, K, active=starts[2], score=starts[0]):
        return L.lib().ppo_beam_search_states(policy._h, e._h, h, M, K, ptr(score, L.c_i8p), ptr(starts[1], L.c_i8p),
                                              ptr(active, L.c_u32p), ptr(st, L.c_i8p), ptr(act, L.c_u32p), ptr(ints[0], L.c_i32p),
                                              ptr(ints[1], L.c_i32p), ptr(ints[2], L.c_i32p), ptr(ints[3], L.c_i32p),
                                              ptr(mant, L.c_f64p), ptr(ints[4], L.c_i32p), None, None, None, None, None)
    assert status(env, pol, 0) == -1 and "1 <= K <= N" in L.last_error()
    assert status(env, pol, kw["num_envs"] + 1) == -1
    assert status(env, bf, c["K"]) == -4 and "bf16" in L.last_error()
    assert status(env, pol, c["K"], active=np.zeros_like(starts[2])) == -1
    assert status(env, pol, c["K"], score=off) == -1
    wscratch, wh = P._evaluator_scratch(wide)
    h = wh
    assert status(wide, pol, P.BEAM_MAX_K + 1) == -4 and "K above 256" in L.last_error()
    assert env.error_flags() == 0 and wide.error_flags() == 0
    after = _env_state(P, env)
    assert all(np.array_equal(before[k], after[k]) for k in before), "a refused call touches no env"
