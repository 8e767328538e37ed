"""Best state of a rollout and best-of-K search on the device (ppo_env_set_internal, ppo_best_states,
ppo_search_best_states) against the CPU oracle.  Every comparison is exact integer equality.  tests/search_ref.py holds the
reference and the tables; tests/test_search_host.py checks both without a device.

1. best_states_ (reset before every trajectory): the trajectories are the ones collect_rollouts_ plays on a fresh identical
   env (as tests/test_gpu_episodes_form.py argues for the evaluators); its actions replayed teacher-forced on the oracle env
   give every field of every trajectory.  Against the parent's evaluator: max(0, max trace) is evaluate_trajectories("best").
   Restated through the gap: best_gap = initial_gap - best wherever opt_score stayed what it was at the start (an action of
   type 2 or 3 changes the sum of the scores, and with it opt_score; then the lowest gap need not sit at the lowest score).
2. set_internal round trip;
3. best_state_in_rollout (no reset) from loaded states against the full CPU replay, then single_trajectory_scores and
   count_non_flips from the same states (at the ticks the envs have reached by then);
4. search_best_states_ against the full CPU replay of the round / clone / tick schedule;
5. an env object of another type: the reference's literal loops, sampling on the engine."""
import numpy as np
import pytest

import episodes_ref as ref
import search_ref as sref

pytestmark = pytest.mark.gpu

FIELDS = ("best_state", "best_active", "best_gap", "best_step", "length", "initial_gap", "trace", "type_counts")


@pytest.fixture(scope="module")
def P(ppo):
    if ppo.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests must run on the GPU box")
    return ppo


def _policy(P, orc, case):
    pol = P.HipPolicy(ref.F, case["hid"], case["L"], 4, seed=0)
    pol.params = ref.policy_params(orc, case)
    return pol


def _mismatches(got, want, fields):
    return {k: int(np.count_nonzero(np.asarray(got[k]) != np.asarray(want[k]))) for k in fields
            if not np.array_equal(got[k], want[k])}


# ---------------------------------------------------------------- 1. best_states_, reset before every trajectory
@pytest.mark.parametrize("name", sref.CASES)
def test_best_states_against_oracle(P, orc, name):
    case = ref.by_name(name)
    kw, nt, N = ref.env_kw_of(case), case["episodes"], case["N"]
    pol = _policy(P, orc, case)
    env, ro = P.HipVecEnv(**kw), P.BufferRollouts()
    P.collect_rollouts_(ro, env, pol, nt, 1.0)
    actions = (ro.selected_actions - 1).astype(np.int32)
    valid = ro.valid
    for n, col in ref.reference(orc, case).items():          # the replayed columns tie the actions to the oracle's own
        assert valid[:, n].sum() == col["length"] and np.array_equal(actions[:col["length"], n], col["actions"]), n
    want = sref.tracked_replay(orc, kw, actions, nt)
    env = P.HipVecEnv(**kw)
    got = P.best_states_(env, pol, nt, scores=True, action_types=True)
    assert env.error_flags() & ~32 == 0
    bad = _mismatches(got, want, FIELDS)
    print(name, "trajectories", nt, "coverage", sref.coverage(want), "mismatches", bad)
    assert not bad, (name, bad)
    it = env.internal()
    assert np.array_equal(it["episode"], want["episode"]) and np.array_equal(it["tick"], want["tick"])
    assert np.array_equal(got["best_score"], got["best_state"][:, :4 * case["Q"]])
    # without the optional outputs: the same records
    env = P.HipVecEnv(**kw)
    plain = P.best_states_(env, pol, nt)
    assert "trace" not in plain and not _mismatches(plain, want, FIELDS[:6])
    # against the evaluator the tracking grew out of
    env = P.HipVecEnv(**kw)
    best = P.evaluate_trajectories(env, pol, nt, "best")
    assert np.array_equal(np.maximum(got["trace"].max(axis=1), 0).astype(np.float64), best)
    const_opt = np.array([t[2] + t[3] == 0 for t in got["type_counts"]])
    assert const_opt.any() or name == "1x3"
    assert np.array_equal(got["best_gap"][const_opt], got["initial_gap"][const_opt] - best[const_opt].astype(np.int64))
    assert env.error_flags() & ~32 == 0


# ---------------------------------------------------------------- 2. set_internal
def test_set_internal_round_trip(P, orc):
    case = ref.by_name("q32-20x30")
    kw, N = ref.env_kw_of(case), case["N"]
    env = P.HipVecEnv(**kw)
    pol, ro = _policy(P, orc, case), P.BufferRollouts()
    P.collect_rollouts_steps_(ro, env, pol, 3, 1.0)           # counters off their initial values, states off a reset
    before = env.internal()
    act0 = env.active_quads()
    assert np.array_equal(act0, P.state(env).action_mask)
    sc, dg, act = np.roll(before["score"], 1, axis=0), np.roll(before["degree"], 1, axis=0), np.roll(act0, 1)
    env.set_internal(sc, dg, act)
    after = env.internal()
    assert np.array_equal(after["score"], sc) and np.array_equal(after["degree"], dg)
    assert np.array_equal(env.active_quads(), act)
    assert not after["steps"].any() and not P.is_terminal(env).any() and not P.reward(env).any()
    assert np.array_equal(after["episode"], before["episode"]) and np.array_equal(after["tick"], before["tick"])
    oenv = ref._env(orc, kw)
    oenv.score[:], oenv.degree[:], oenv.active[:] = sc, dg, act
    st = P.state(env)
    assert np.array_equal(st.vertex_score, oenv.observe_all()) and np.array_equal(st.action_mask, act)
    bad = sc.copy()
    bad[:, -1] = 1                                            # the last quad of a Q = 32 reset state is inactive
    assert not ((act >> 31) & 1).any()
    with pytest.raises(P.PPOError, match="inactive quad"):
        env.set_internal(bad, dg, act)
    with pytest.raises(P.PPOError):
        env.set_internal(sc[:-1], dg[:-1], act[:-1])
    assert np.array_equal(env.internal()["score"], sc), "a refused call uploads nothing"
    assert env.error_flags() & ~32 == 0


# ---------------------------------------------------------------- 3. from the states the envs hold
def test_best_state_in_rollout_from_loaded_states(P, orc):
    case = ref.by_name("70x100")
    kw, N, M = ref.env_kw_of(case), case["N"], case["M"]
    params = ref.policy_params(orc, case)
    pol, env = _policy(P, orc, case), P.HipVecEnv(**kw)
    first = P.best_states_(env, pol, case["episodes"])
    sc, dg, act = first["best_score"][:N].copy(), first["best_degree"][:N].copy(), first["best_active"][:N].copy()
    for call in ("best_state_in_rollout", "single_trajectory_scores", "count_non_flips"):
        env.set_internal(sc, dg, act)
        before = env.internal()                               # the ticks moved on: each call plays other trajectories
        want = sref.stack([sref.play_from(orc, kw, n, params, case["hid"], case["L"], (sc[n], dg[n], int(act[n])),
                                          int(before["tick"][n])) for n in range(N)], M)
        if call == "best_state_in_rollout":
            got = P.best_state_in_rollout(env, pol)
            bad = _mismatches(got, want, FIELDS[:6])
            print("no reset, 70 envs: start already best", int((want["best_step"] == 0).sum()), "mismatches", bad)
            assert not bad, bad
            assert (want["initial_gap"] == first["best_gap"][:N]).all()
        elif call == "single_trajectory_scores":
            got = P.single_trajectory_scores(env, pol)
            assert all(np.array_equal(got[n], want["trace"][n, :want["length"][n]]) for n in range(N))
        else:
            assert np.array_equal(P.count_non_flips(env, pol), want["type_counts"][:, 2:].sum(axis=1))
        after = env.internal()
        assert np.array_equal(after["episode"], before["episode"]), "no reset!: no episode counter is consumed"
        assert np.array_equal(after["tick"].astype(np.int64), before["tick"].astype(np.int64) + want["length"])
        assert P.is_terminal(env).all()
        assert env.error_flags() & ~32 == 0
    with pytest.raises(P.PPOError, match="already terminal"):
        P.best_state_in_rollout(env, pol)


# ---------------------------------------------------------------- 4. best-of-K search
@pytest.mark.parametrize("shape", sref.SEARCH_SHAPES, ids=lambda s: "M%d-K%d-N%d" % s)
def test_search_against_oracle(P, orc, shape):
    M, K, N = shape
    want = sref.search_reference(orc, shape)
    c = dict(sref.SEARCH_CASE)
    pol = P.HipPolicy(ref.F, c["hid"], c["L"], 4, seed=0)
    pol.params = orc.glorot_params(ref.F, c["hid"], c["L"], seed=c["pseed"])
    env = P.HipVecEnv(**sref.search_env_kw(N))
    before = env.internal()
    assert not before["tick"].any()
    sc, dg, act = sref.search_starts(orc, M)
    got = P.search_best_states_(env, pol, sc, dg, act, K, clone_gaps=True)
    assert env.error_flags() & ~32 == 0
    fields = ("clone_gaps", "best_state", "best_active", "best_gap", "best_clone", "best_step", "initial_gap")
    bad = _mismatches(got, want, fields)
    tied = sref.tied_starts(want)
    print(shape, "rounds", -(-M // (N // K)), "tied starts", tied, "mismatches", bad)
    assert not bad, (shape, bad)
    after = env.internal()
    assert np.array_equal(after["episode"], before["episode"]), "episode counters are unchanged by the call"
    assert np.array_equal(after["tick"].astype(np.int64), want["tick"]), "ticks advance by the steps each env played"
    busy = min(N // K, M) * K
    assert P.is_terminal(env)[:busy].all()
    plain = P.search_best_states_(P.HipVecEnv(**sref.search_env_kw(N)), pol, sc, dg, act, K)
    assert "clone_gaps" not in plain and not _mismatches(plain, want, fields[1:])
    if shape == sref.TIED_SHAPE:
        assert tied, "no start with two clones tied for the best gap: the lowest-clone rule is not exercised"


def test_search_refuses_bad_arguments(P, orc):
    c = sref.SEARCH_CASE
    pol = P.HipPolicy(ref.F, c["hid"], c["L"], 4, seed=0)
    env = P.HipVecEnv(**sref.search_env_kw(3))
    sc, dg, act = sref.search_starts(orc, 2)
    for K in (0, 4):
        with pytest.raises(P.PPOError):
            P.search_best_states_(env, pol, sc, dg, act, K)
    with pytest.raises(P.PPOError, match="no active quad"):
        P.search_best_states_(env, pol, sc, dg, np.zeros(2, np.uint32), 1)
    assert env.error_flags() & ~32 == 0


# ---------------------------------------------------------------- 5. any other env object: the reference's literal loops
class WalkGame:
    """wrapper.env of a toy game: the score walks by the sampled action; it logs what it was asked to do."""

    def __init__(self):
        self.initial_score = self.current_score = 7
        self.opt_score = 1
        self.log = []


class WalkEnv:
    def __init__(self, horizon=12):
        self.env, self.horizon = WalkGame(), horizon


class WalkPolicy:
    pass


def test_generic_env_runs_the_reference_loops(P):
    if not getattr(P, "_walkenv_registered", False):
        def step(w, action):                                  # 1-based actions 1..8: types 1..4 twice over
            g = w.env
            g.log.append(action)
            g.current_score = max(g.opt_score, g.current_score + (-1, 1, -2, 0, 2, -1, 0, 1)[action - 1])
        P.state.register(WalkEnv)(lambda w: w.env.current_score)
        P.is_terminal.register(WalkEnv)(lambda w: len(w.env.log) >= w.horizon)
        P.step_.register(WalkEnv)(step)
        P.action_probabilities.register(WalkPolicy)(lambda p, s: np.full(8, 0.125, np.float32))
        P._walkenv_registered = True
    for seed in range(4):
        w = WalkEnv()
        best = P.best_state_in_rollout(w, WalkPolicy(), rng=np.random.default_rng(seed))
        scores = [7]
        for a in w.env.log:
            scores.append(max(1, scores[-1] + (-1, 1, -2, 0, 2, -1, 0, 1)[a - 1]))
        gaps = [s - 1 for s in scores]
        assert len(w.env.log) == 12 and best is not w
        assert best.env.current_score - best.env.opt_score == min(gaps)
        assert len(best.env.log) == int(np.argmin(gaps)), "the copy at the FIRST minimum"
        w = WalkEnv()
        tr = P.single_trajectory_scores(w, WalkPolicy(), rng=np.random.default_rng(seed))
        assert w.env.log == best.env.log + w.env.log[len(best.env.log):] and len(tr) == 12
        assert tr == [7 - s for s in scores[1:]], "the same uniforms: the same trajectory"
        w = WalkEnv()
        assert P.count_non_flips(w, WalkPolicy(), rng=np.random.default_rng(seed)) == sum(1 for a in w.env.log if (a - 1) % 4 >= 2)
