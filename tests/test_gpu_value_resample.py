"""The resampling search that ranks by the critic's value on the device (ppo_search_resample_states_value,
k_search_resample<PATH, VALUE>) against the CPU oracle.

Device values are not bit-predictable on the CPU, so the replay (tests/value_resample_ref.py) is TEACHER-FORCED: it takes the
values of every event from the device's own event_values log and must then reproduce every returned field, the donors log,
the paths, the clone gaps, the ticks, the episode counters and the done flags EXACTLY.  The loop is closed by comparing every
logged value bit for bit with batch_state_values(critic, ...) of the states the replay holds at that event: the value
forward computes a state's value from that state's rows alone (tests/test_gpu_value.py holds a one-state call against its
row of a batch), so a device that leaves the rule shows either a state mismatch or a value mismatch at the first event where
it does.  A value that is not finite is compared by class (NaN / +inf / -inf): the rule ranks every such value as 0, and
nothing in the search reads its payload.  tests/test_value_resample_host.py checks without a device that the inputs hold
the situations that matter.

1. every shape: the teacher-forced equality with and without path=True, the closure of the values, the closure of the paths
   (apply_paths_), and donors that differ from gap ranking in at least one event;
2. value_weight = 0 with a critic is the call without a critic, in every field and in the ticks;
3. interval >= max_actions is search_best_states_;
4. a critic with NaN and inf among its values still follows the rule, and they are logged raw;
5. the refusals."""
import numpy as np
import pytest

import episodes_ref as ref
import value_resample_ref as vref

pytestmark = pytest.mark.gpu

RESULT = ("best_state", "best_active", "best_gap", "best_clone", "best_step", "initial_gap")
FIELDS = RESULT + ("donors", "clone_gaps")


@pytest.fixture(scope="module")
def P(ppo):
    if ppo.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests must run on the GPU box")
    return ppo


def _policy(P, orc):
    pol = P.HipPolicy(ref.F, vref.POLICY["hid"], vref.POLICY["L"], 4, seed=0)
    pol.params = vref.policy_params(orc)
    return pol


def _critic(P, orc, name, params=None):
    hid, L = vref.SHAPES[name]["critic"]
    c = P.HipCritic(ref.F, hid, L, seed=0)
    c.params = vref.critic_params(orc, name) if params is None else params
    return c


def _mismatches(got, want, fields):
    return {k: int(np.count_nonzero(np.asarray(got[k]) != np.asarray(want[k]))) if np.shape(got[k]) == np.shape(want[k])
            else (np.shape(got[k]), np.shape(want[k])) for k in fields if not np.array_equal(got[k], want[k])}


def _env_state(P, env):
    it = env.internal()
    return dict(tick=it["tick"].copy(), episode=it["episode"].copy(), done=P.is_terminal(env).copy())


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _same_values(got, want):
    """Bit for bit where finite; by class (NaN, +inf, -inf) where not."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    fin = np.isfinite(want)
    return (np.array_equal(np.isfinite(got), fin) and _same_bits(got[fin], want[fin])
            and np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.signbit(got[~fin & ~np.isnan(want)]),
                                                                                 np.signbit(want[~fin & ~np.isnan(want)])))


def _teacher_forced(P, orc, name, critic, w=None):
    """The device call with and without the path, the replay on the device's log, every comparison.  Returns (got, want)."""
    M, K, N, T, R, m0 = vref.SHAPES[name]["shape"]
    w = vref.SHAPES[name]["w"] if w is None else w
    pol, kw, starts = _policy(P, orc), vref.env_kw(name), vref.starts(orc, name)
    env, env2 = P.HipVecEnv(**kw), P.HipVecEnv(**kw)
    before = _env_state(P, env)
    assert not before["tick"].any()
    got = P.search_resample_states_(env, pol, *starts, K, R, m0, donors=True, clone_gaps=True, path=True, critic=critic,
                                    value_weight=w, values=True)
    plain = P.search_resample_states_(env2, pol, *starts, K, R, m0, donors=True, clone_gaps=True, critic=critic, value_weight=w,
                                      values=True)
    assert env.error_flags() & ~32 == 0 and env2.error_flags() & ~32 == 0
    log = got["event_values"]
    assert log.dtype == np.float32 and log.shape == (M, (T - 1) // R, K) == got["donors"].shape
    assert got["path"].dtype == np.int16 and got["path"].shape == (M, T)
    # with and without the path: the same search
    assert "path" not in plain and not _mismatches(plain, got, FIELDS) and _same_bits(plain["event_values"], log)
    a, b = _env_state(P, env), _env_state(P, env2)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    # the replay on the device's own values
    want = vref.replay(orc, name, lambda start, ev, states, active, done: log[start, ev], w=w)
    bad = _mismatches(got, want, FIELDS)
    pbad = int(np.count_nonzero(got["path"] != (want["path"] + 1)))
    evs = [e for e in want["events"] if e["order"]]
    differ = sum(vref.differs_from_gap_ranking(e) for e in evs)
    print(name, vref.SHAPES[name], "events with live clones", len(evs), "survivors differ from gap ranking", differ, "receivers",
          int((want["donors"] >= 0).sum()), "fold event", want["fold_event"].tolist(), "best", want["best_gap"].tolist(),
          "mismatches", bad, "path mismatches", pbad)
    assert not bad, (name, bad)
    assert pbad == 0, (name, pbad)
    assert np.array_equal(a["episode"], before["episode"]), "episode counters are unchanged by the call"
    assert np.array_equal(a["tick"].astype(np.int64), want["tick"]), "ticks advance by the steps each env played"
    assert a["done"][want["played"]].all(), "the envs that played are left terminal"
    assert np.array_equal(a["done"][~want["played"]], before["done"][~want["played"]]), "the idle envs are left alone"
    # the log itself: the critic's forward of the states the replay holds, NaN for terminal clones and events that never ran
    seen = np.zeros(log.shape, bool)
    states, active, where = [], [], []
    for e in want["events"]:
        for c in range(K):
            seen[e["start"], e["event"], c] = not e["done"][c]
            if not e["done"][c]:
                states.append(e["states"][c])
                active.append(e["active"][c])
                where.append((e["start"], e["event"], c))
    assert np.isnan(log[~seen]).all(), "NaN for a terminal clone and for an event that did not run"
    direct = P.batch_state_values(critic, P.StateData(np.stack(states), np.asarray(active, np.uint32)))
    logged = np.array([log[i] for i in where], np.float32)
    assert _same_values(logged, direct), ("logged values differ from the critic's forward of the replayed states",
                                          int(np.count_nonzero(logged.view(np.uint32) != direct.view(np.uint32))))
    # closure of the paths on the device
    back = P.apply_paths_(env, *starts, got["path"])
    cbad = _mismatches(dict(best_state=back["state"], best_active=back["active"], best_gap=back["gap"], best_step=back["applied"]),
                       got, ("best_state", "best_active", "best_gap", "best_step"))
    assert not cbad, cbad
    return got, want, differ


# ---------------------------------------------------------------- 1. every shape, teacher-forced
@pytest.mark.parametrize("name", list(vref.SHAPES))
def test_value_resample_teacher_forced(P, orc, name):
    got, want, differ = _teacher_forced(P, orc, name, _critic(P, orc, name))
    assert np.isfinite(got["event_values"][got["donors"] != -2]).all()
    assert differ >= 1, "the donors derived from the device's own log differ from gap ranking in at least one event"


# ---------------------------------------------------------------- 2. weight 0 is the call without a critic
@pytest.mark.parametrize("name", ["A", "E"])
def test_weight_zero_is_the_plain_call(P, orc, name):
    M, K, N, T, R, m0 = vref.SHAPES[name]["shape"]
    pol, kw, starts, critic = _policy(P, orc), vref.env_kw(name), vref.starts(orc, name), _critic(P, orc, name)
    a, b = P.HipVecEnv(**kw), P.HipVecEnv(**kw)
    got = P.search_resample_states_(a, pol, *starts, K, R, m0, donors=True, clone_gaps=True, path=True, critic=critic,
                                    value_weight=0.0, values=True)
    want = P.search_resample_states_(b, pol, *starts, K, R, m0, donors=True, clone_gaps=True, path=True)
    assert "event_values" not in want and not _mismatches(got, want, FIELDS + ("path",))
    sa, sb = _env_state(P, a), _env_state(P, b)
    assert all(np.array_equal(sa[k], sb[k]) for k in sa)
    assert np.array_equal(np.isnan(got["event_values"]), got["donors"] == -2), "the values are logged whatever the weight"
    assert (got["donors"] >= 0).any()


# ---------------------------------------------------------------- 3. no event: the best-of-K search
def test_no_event_is_search_best_states(P, orc):
    name = "C"
    M, K, N, T, R, m0 = vref.SHAPES[name]["shape"]
    pol, kw, starts, critic = _policy(P, orc), vref.env_kw(name), vref.starts(orc, name), _critic(P, orc, name)
    a, b = P.HipVecEnv(**kw), P.HipVecEnv(**kw)
    got = P.search_resample_states_(a, pol, *starts, K, T, m0, donors=True, clone_gaps=True, path=True, critic=critic,
                                    value_weight=vref.SHAPES[name]["w"], values=True)
    want = P.search_best_states_(b, pol, *starts, K, clone_gaps=True, path=True)
    assert got["donors"].shape == (M, 0, K) and got["event_values"].shape == (M, 0, K)
    assert not _mismatches(got, want, RESULT + ("clone_gaps", "path"))
    sa, sb = _env_state(P, a), _env_state(P, b)
    assert all(np.array_equal(sa[k], sb[k]) for k in sa)


# ---------------------------------------------------------------- 4. values that are not finite
def test_non_finite_values_rank_as_zero(P, orc):
    """value_resample_ref.non_finite_critic_params: +inf, NaN and finite values, depending on the state."""
    name = "A"
    hid, L = vref.NON_FINITE["critic"]
    critic = P.HipCritic(ref.F, hid, L, seed=0)
    critic.params = vref.non_finite_critic_params(orc)
    got, want, differ = _teacher_forced(P, orc, name, critic)
    live = got["event_values"][got["donors"] != -2]
    print("live values", live.size, "NaN", int(np.isnan(live).sum()), "inf", int(np.isinf(live).sum()))
    assert (~np.isfinite(live)).any() and np.isfinite(live).any(), "the case holds both kinds of value"
    for e in want["events"]:                                      # ranked as 0: s is the gap itself, exactly
        for c in e["order"]:
            if not np.isfinite(e["values"][c]):
                assert e["s"][c] == e["cur_gap"][c]


# ---------------------------------------------------------------- 5. refused arguments
def test_value_resample_refuses_bad_arguments(P, orc):
    name = "Q32"
    M, K, N, T, R, m0 = vref.SHAPES[name]["shape"]
    pol, kw, starts, critic = _policy(P, orc), vref.env_kw(name), vref.starts(orc, name), _critic(P, orc, name)
    env = P.HipVecEnv(**kw)
    call = lambda **k: P.search_resample_states_(env, pol, *starts, K, R, m0, **k)
    for k, status in ((dict(values=True), -1), (dict(critic=critic, value_weight=-1.0), -1),
                      (dict(critic=critic, value_weight=float("nan")), -1), (dict(critic=critic, value_weight=float("inf")), -1),
                      (dict(critic=P.HipCritic(216, 128, 2, seed=1)), -4)):
        with pytest.raises(P.PPOError) as err:
            call(**k)
        assert err.value.status == status, (k, err.value)
    half = P.HipPolicy(ref.F, 128, 2, 4, seed=1, dtype="bf16")
    with pytest.raises(P.PPOError) as err:
        call(critic=half)
    assert err.value.status == -4
    # the C entry point checks the same itself
    scratch, h = P._evaluator_scratch(env)
    V = 4 * env.Q
    st, bact = np.zeros((M, 2 * V), np.int8), np.zeros(M, np.uint32)
    ints = [np.zeros(M, np.int32) for _ in range(4)]
    p8, pu, pi = P._lib.c_i8p, P._lib.c_u32p, P._lib.c_i32p
    ptr = lambda a, t: a.ctypes.data_as(t)
    fn = P._lib.lib().ppo_search_resample_states_value
    for c, w, status in ((critic._h, -0.5, -1), (critic._h, float("nan"), -1), (critic._h, 1e39, -1), (None, 1.0, -1),
                         (half._h, 1.0, -4)):
        got = fn(pol._h, c, env._h, h, M, K, ptr(starts[0], p8), ptr(starts[1], p8), ptr(starts[2], pu), ptr(st, p8),
                 ptr(bact, pu), *(ptr(x, pi) for x in ints), None, R, m0, w, None, None, None)
        assert got == status, (w, got)
    assert not env.internal()["tick"].any(), "a refused call plays nothing"
    assert env.error_flags() & ~32 == 0
