"""The resampling search on the device (ppo_search_resample_states, k_search_resample) against the CPU oracle.  Every
comparison is exact integer equality.  tests/resample_ref.py holds the reference and the shape table;
tests/test_resample_host.py checks, without a device, that the shapes contain the situations that matter: a survivor cut
between clones of equal gap, terminal clones at an event, a receiver whose discarded record only the fold keeps, a result the
fold decides.

1. every shape: every returned field, the donors log, and the ticks, episode counters and done flags the call leaves;
2. interval >= max_actions (shape H) and survivors == K (shape G) against the device's own search_best_states_;
3. search_best_states_ behind a resampling call on the same env, from the ticks it left;
4. K at the cap of 4096 clones (the largest LDS request, sixteen passes of the workgroup): too many env-steps for the CPU
   replay, so survivors == K against the device's own search_best_states_, and with survivors = 64 what the log and the
   result must satisfy whatever was played;
5. refused arguments."""
import numpy as np
import pytest

import episodes_ref as ref
import resample_ref as rref
import search_ref as sref

pytestmark = pytest.mark.gpu

FIELDS = ("best_state", "best_active", "best_gap", "best_clone", "best_step", "initial_gap", "donors", "clone_gaps")


@pytest.fixture(scope="module")
def P(ppo):
    if ppo.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests must run on the GPU box")
    return ppo


def _policy(P, orc):
    pol = P.HipPolicy(ref.F, rref.CASE["hid"], rref.CASE["L"], 4, seed=0)
    pol.params = rref.policy_params(orc)
    return pol


def _mismatches(got, want, fields):
    return {k: int(np.count_nonzero(np.asarray(got[k]) != np.asarray(want[k]))) if np.shape(got[k]) == np.shape(want[k])
            else (np.shape(got[k]), np.shape(want[k])) for k in fields if not np.array_equal(got[k], want[k])}


# ---------------------------------------------------------------- 1. every shape against the oracle
@pytest.mark.parametrize("name", list(rref.SHAPES))
def test_resample_against_oracle(P, orc, name):
    M, K, N, T, R, m0 = rref.SHAPES[name]
    want = rref.reference(orc, name)
    pol, env = _policy(P, orc), P.HipVecEnv(**rref.env_kw(rref.SHAPES[name]))
    before = env.internal()
    done_before = P.is_terminal(env).copy()
    assert not before["tick"].any()
    sc, dg, act = sref.search_starts(orc, M)
    got = P.search_resample_states_(env, pol, sc, dg, act, K, R, m0, donors=True, clone_gaps=True)
    assert env.error_flags() & ~32 == 0
    bad = _mismatches(got, want, FIELDS)
    print(name, rref.SHAPES[name], "rounds", -(-M // (N // K)), "events", len(want["events"]), "receivers",
          int((want["donors"] >= 0).sum()), "best", want["best_gap"].tolist(), "mismatches", bad)
    assert not bad, (name, bad)
    assert got["donors"].dtype == np.int32 and got["donors"].shape == (M, (T - 1) // R, K)
    assert np.array_equal(got["best_score"], got["best_state"][:, :4 * rref.CASE["Q"]])
    after = env.internal()
    assert np.array_equal(after["episode"], before["episode"]), "episode counters are unchanged by the call"
    assert np.array_equal(after["tick"].astype(np.int64), want["tick"]), "ticks advance by the steps each env played"
    done = P.is_terminal(env)
    assert done[want["played"]].all(), "the envs that played are left terminal"
    assert np.array_equal(done[~want["played"]], done_before[~want["played"]]), "the idle envs are left alone"
    # without the optional outputs: the same result
    plain = P.search_resample_states_(P.HipVecEnv(**rref.env_kw(rref.SHAPES[name])), pol, sc, dg, act, K, R, m0)
    assert "donors" not in plain and "clone_gaps" not in plain and not _mismatches(plain, want, FIELDS[:6])


# ---------------------------------------------------------------- 2. against the device's own best-of-K search
def test_no_event_is_search_best_states(P, orc):
    M, K, N, T, R, m0 = rref.SHAPES["H"]
    pol, kw = _policy(P, orc), rref.env_kw(rref.SHAPES["H"])
    sc, dg, act = sref.search_starts(orc, M)
    a, b = P.HipVecEnv(**kw), P.HipVecEnv(**kw)
    got = P.search_resample_states_(a, pol, sc, dg, act, K, R, m0, donors=True, clone_gaps=True)
    want = P.search_best_states_(b, pol, sc, dg, act, K, clone_gaps=True)
    assert got["donors"].shape == (M, 0, K)
    assert not _mismatches(got, want, ("best_state", "best_active", "best_gap", "best_clone", "best_step", "initial_gap",
                                       "clone_gaps"))
    assert np.array_equal(a.internal()["tick"], b.internal()["tick"])
    assert np.array_equal(P.is_terminal(a), P.is_terminal(b))


def test_survivors_equal_k_copies_nothing(P, orc):
    M, K, N, T, R, m0 = rref.SHAPES["G"]
    assert m0 == K
    pol, kw = _policy(P, orc), rref.env_kw(rref.SHAPES["G"])
    sc, dg, act = sref.search_starts(orc, M)
    a, b = P.HipVecEnv(**kw), P.HipVecEnv(**kw)
    got = P.search_resample_states_(a, pol, sc, dg, act, K, R, m0, donors=True, clone_gaps=True)
    want = P.search_best_states_(b, pol, sc, dg, act, K, clone_gaps=True)
    assert not (got["donors"] >= 0).any()
    assert not _mismatches(got, want, ("best_gap", "initial_gap", "clone_gaps"))
    assert np.array_equal(a.internal()["tick"], b.internal()["tick"])


# ---------------------------------------------------------------- 3. the env behind a resampling call
def test_search_best_states_behind_a_resampling_call(P, orc):
    """The best-of-K search on the env a resampling call has used: it plays from the ticks left behind."""
    name = "C"
    M, K, N, T, R, m0 = rref.SHAPES[name]
    first = rref.reference(orc, name)
    pol, kw = _policy(P, orc), rref.env_kw(rref.SHAPES[name])
    env = P.HipVecEnv(**kw)
    sc, dg, act = sref.search_starts(orc, M)
    P.search_resample_states_(env, pol, sc, dg, act, K, R, m0)
    assert np.array_equal(env.internal()["tick"].astype(np.int64), first["tick"])
    M2, K2 = 3, 20                                            # another split of the same envs: three starts on 60 of them
    s2 = (sc[:M2], dg[:M2], act[:M2])
    want = sref.search_replay(orc, kw, rref.policy_params(orc), rref.CASE["hid"], rref.CASE["L"], s2, K2, tick0=first["tick"])
    got = P.search_best_states_(env, pol, *s2, K2, clone_gaps=True)
    bad = _mismatches(got, want, ("clone_gaps", "best_state", "best_active", "best_gap", "best_clone", "best_step", "initial_gap"))
    assert not bad, bad
    assert np.array_equal(env.internal()["tick"].astype(np.int64), want["tick"])
    assert env.error_flags() & ~32 == 0


# ---------------------------------------------------------------- 4. K at the cap
def test_k_at_the_cap(P, orc):
    K, T = 4096, 4
    kw = rref.env_kw((1, K, K, T, 1, K))
    pol = _policy(P, orc)
    sc, dg, act = sref.search_starts(orc, 1)
    a, b = P.HipVecEnv(**kw), P.HipVecEnv(**kw)
    got = P.search_resample_states_(a, pol, sc, dg, act, K, 1, K, donors=True, clone_gaps=True)
    want = P.search_best_states_(b, pol, sc, dg, act, K, clone_gaps=True)
    assert not (got["donors"] >= 0).any()
    assert not _mismatches(got, want, ("best_gap", "initial_gap", "clone_gaps"))
    assert np.array_equal(a.internal()["tick"], b.internal()["tick"])
    m0 = 64
    env = P.HipVecEnv(**kw)
    got = P.search_resample_states_(env, pol, sc, dg, act, K, 1, m0, donors=True, clone_gaps=True)
    assert env.error_flags() & ~32 == 0
    V = 4 * rref.CASE["Q"]
    assert sref.score_gap(got["best_state"][0, :V], int(got["best_active"][0]))[1] == got["best_gap"][0]
    assert got["best_gap"][0] <= got["clone_gaps"][0].min() and got["initial_gap"][0] == want["initial_gap"][0]
    assert 0 <= got["best_step"][0] <= T and 0 <= got["best_clone"][0] < K
    for row in got["donors"][0]:
        live = int((row != -2).sum())
        kept = np.flatnonzero(row == -1)
        assert kept.size == min(m0, live), "ranks below m keep their state"
        receivers = np.flatnonzero(row >= 0)
        assert np.isin(row[receivers], kept).all(), "a donor is a survivor, never a receiver"
        if receivers.size:                                    # rank rho >= m takes rank (rho - m) % m: donors are used evenly
            uses = np.bincount(row[receivers], minlength=K)[kept]
            assert uses.max() - uses.min() <= 1


# ---------------------------------------------------------------- 5. refused arguments
def test_resample_refuses_bad_arguments(P, orc):
    pol = _policy(P, orc)
    env = P.HipVecEnv(**rref.env_kw((2, 4, 8, 6, 2, 2)))
    sc, dg, act = sref.search_starts(orc, 2)
    for K, R, m0 in ((4, 0, 2), (4, 2, 0), (4, 2, 5), (0, 2, 1), (9, 2, 2)):
        with pytest.raises(P.PPOError) as err:
            P.search_resample_states_(env, pol, sc, dg, act, K, R, m0)
        assert err.value.status == -1
    with pytest.raises(P.PPOError, match="no active quad"):
        P.search_resample_states_(env, pol, sc, dg, np.zeros(2, np.uint32), 4, 2, 2)
    # the C entry point checks the same itself
    scratch, h = P._evaluator_scratch(env)
    V = 4 * env.Q
    st, bact = np.zeros((2, 2 * V), np.int8), np.zeros(2, np.uint32)
    ints = [np.zeros(2, np.int32) for _ in range(4)]
    p8, pu, pi = P._lib.c_i8p, P._lib.c_u32p, P._lib.c_i32p
    ptr = lambda a, t: a.ctypes.data_as(t)
    fn = P._lib.lib().ppo_search_resample_states
    for K, R, m0, a in ((4, 0, 2, act), (4, 2, 0, act), (4, 2, 5, act), (9, 2, 2, act), (4, 2, 2, np.zeros(2, np.uint32))):
        status = fn(pol._h, env._h, h, 2, K, ptr(sc, p8), ptr(dg, p8), ptr(a, pu), ptr(st, p8), ptr(bact, pu),
                    *(ptr(x, pi) for x in ints), None, R, m0, None)
        assert status == -1, (K, R, m0)
    assert not env.internal()["tick"].any(), "a refused call plays nothing"
    big = P.HipVecEnv(**rref.env_kw((1, 4097, 4100, 6, 2, 2)))     # above the cap: the keys no longer fit the LDS request
    scratch_b, hb = P._evaluator_scratch(big)
    status = fn(pol._h, big._h, hb, 2, 4097, ptr(sc, p8), ptr(dg, p8), ptr(act, pu), ptr(st, p8), ptr(bact, pu),
                *(ptr(x, pi) for x in ints), None, 2, 2, None)
    assert status == -4 and not big.internal()["tick"].any()
    assert env.error_flags() & ~32 == 0
