"""Action selection rules on the device (HipPolicy.selection; k_policy_fwd modes 14 / 15) against the CPU oracle.
Every comparison is exact equality, p_sel bitwise.  tests/select_ref.py holds the reference; tests/test_select_host.py checks it
without a device and asserts that the cases contain what matters here: tempered trajectories that leave the default ones, greedy
trajectories that move, the tie masks.

1. best_states_(actions, scores, action types) in the reset form under every selection on Policy(72,256,2,4), Q = 8, 70 envs,
   100 trajectories, max_actions 20; on the side shapes (hidden 128, three hidden layers, hidden 96, Q = 32) under an inexact
   temperature and greedy, in both reset forms; ticks, episode counters and done flags after each call;
2. the three evaluator kinds and average_returns;
3. search_best_states_(path, clone_gaps) and search_resample_states_(path, donors) with the closure on the device; greedy
   clones of a start all play one trajectory;
4. the action and p_sel of a single step (ppo_debug_select_step: no call behind play_quotas returns p_sel) for 70 envs in
   mid-trajectory states under every selection, and at Q = 32;
5. ties: logits (0, 1, 1, 0) on every row, greedy plays 16 * (lowest active quad) + 1;
6. 1100 envs at hidden 128 and 256 (at 256 a second pass of the forward's grid);
7. unchanged ground: the collectors, action_probabilities and the gradient do not read the selection; None restores the default;
8. refusals."""
import ctypes as C

import numpy as np
import pytest

import episodes_ref as ref
import path_ref as pref
import select_ref as S

pytestmark = pytest.mark.gpu

RECORD = ("best_state", "best_active", "best_gap", "best_step", "length", "initial_gap", "trace", "type_counts")
RESULT = ("best_state", "best_active", "best_gap", "best_clone", "best_step", "initial_gap")


@pytest.fixture(scope="module")
def P(ppo):
    if ppo.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests must run on the GPU box")
    return ppo


def _sid(sel):
    return "%s-%g" % sel


def _policy(P, params, hid, L, sel=None):
    pol = P.HipPolicy(ref.F, hid, L, 4, seed=0)
    pol.params = params
    if sel is not None:
        pol.selection = sel
        assert pol.selection == (sel[0], float(sel[1]))
    return pol


def _case_policy(P, orc, case, sel=None):
    return _policy(P, ref.policy_params(orc, case), case["hid"], case["L"], sel)


def _mismatches(got, want, fields):
    return {k: int(np.count_nonzero(np.asarray(got[k]) != np.asarray(want[k]))) if np.shape(got[k]) == np.shape(want[k])
            else (np.shape(got[k]), np.shape(want[k])) for k in fields if not np.array_equal(got[k], want[k])}


def _env_state(P, env):
    it = env.internal()
    return dict(tick=it["tick"].astype(np.int64), episode=it["episode"].astype(np.int64), done=P.is_terminal(env).copy())


def _debug_step(P, pol, env):
    """(0-based actions [N], p_sel [N]) of one selection step from the states and ticks the envs hold; nothing is stepped."""
    L = P._lib.lib()
    L.ppo_debug_select_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ppo_debug_select_step.restype = C.c_int32
    scratch = P.BufferRollouts()
    h = scratch._ensure(env, 1)
    a, p = np.full(env.N, -7, np.int32), np.full(env.N, -7.0, np.float32)
    assert L.ppo_debug_select_step(pol._h, env._h, h, a.ctypes.data, p.ctypes.data) == 0, P._lib.last_error()
    return a, p


def _check_reset_form(P, orc, case, sel):
    pol = _case_policy(P, orc, case, sel)
    env = P.HipVecEnv(**ref.env_kw_of(case))
    got = P.best_states_(env, pol, case["episodes"], scores=True, action_types=True, actions=True)
    assert env.error_flags() & ~32 == 0
    want, cols = S.best_states(orc, case, sel), S.episodes(orc, case, sel)
    bad = _mismatches(got, dict(want, actions=pref.one_based(want["actions"])), RECORD + ("actions",))
    print(case["name"], sel, "trajectories", case["episodes"], "steps", int(want["length"].sum()), "mismatches", bad)
    assert not bad, (case["name"], sel, bad)
    after = _env_state(P, env)
    assert np.array_equal(after["tick"], cols["tick"]) and np.array_equal(after["episode"], cols["episode"])
    assert after["done"].all()
    return pol


# ---------------------------------------------------------------- 1. best_states_
@pytest.mark.parametrize("sel", S.SELECTIONS, ids=_sid)
def test_best_states_main_shape(P, orc, sel):
    _check_reset_form(P, orc, S.MAIN, sel)


@pytest.mark.parametrize("sel", S.SIDE_SELECTIONS, ids=_sid)
@pytest.mark.parametrize("case", S.SIDE, ids=lambda c: c["name"])
def test_best_states_side_shapes_both_reset_forms(P, orc, case, sel):
    pol = _check_reset_form(P, orc, case, sel)
    # without a reset: every env plays one trajectory from the state a fresh env holds (the reset of episode counter 0)
    N = case["N"]
    env = P.HipVecEnv(**ref.env_kw_of(case))
    before = _env_state(P, env)
    got = P._best_states(env, pol, N, False, True, True, True)
    assert env.error_flags() & ~32 == 0
    want = S.trajectories(orc, case, sel, list(range(N)), 0)
    bad = _mismatches(got, dict(want, actions=pref.one_based(want["actions"])), RECORD + ("actions",))
    assert not bad, (case["name"], sel, bad)
    after = _env_state(P, env)
    assert np.array_equal(after["episode"], before["episode"]) and np.array_equal(after["tick"], want["length"])
    assert after["done"].all()


# ---------------------------------------------------------------- 2. evaluators
@pytest.mark.parametrize("sel", S.SIDE_SELECTIONS, ids=_sid)
def test_evaluators(P, orc, sel):
    case = S.SIDE[0]
    pol = _case_policy(P, orc, case, sel)
    cols = S.episodes(orc, case, sel)
    for kind in ("return", "best", "normalized"):
        env = P.HipVecEnv(**ref.env_kw_of(case))
        got = P.evaluate_trajectories(env, pol, case["episodes"], kind)
        want = S.evaluator_values(orc, case, sel, kind)
        assert got.shape == want.shape and np.array_equal(got, want), (kind, int(np.count_nonzero(got != want)))
        after = _env_state(P, env)
        assert np.array_equal(after["tick"], cols["tick"]) and np.array_equal(after["episode"], cols["episode"]) and after["done"].all()
    # the three averages are mean and sample std of those values; average_returns leaves its collector for them
    for fn, kind, env_first in ((P.average_returns, "return", False), (P.average_best_returns, "best", True),
                                (P.average_normalized_returns, "normalized", True)):
        env = P.HipVecEnv(**ref.env_kw_of(case))
        m, s = fn(env, pol, case["episodes"]) if env_first else fn(pol, env, case["episodes"])
        v = S.evaluator_values(orc, case, sel, kind)
        assert abs(m - v.mean()) <= 1e-12 * (1 + abs(v.mean())) and abs(s - v.std(ddof=1)) <= 1e-12 * (1 + v.std(ddof=1)), kind
        assert np.array_equal(_env_state(P, env)["tick"], cols["tick"])
    # ... and with the default selection it is the collector's figure, as before
    base = S.episodes(orc, case, S.DEFAULT)
    rec = ref.teacher_forced(orc, ref.env_kw_of(case), base["actions"], case["episodes"])
    v = ref.evaluator_values("return", rec)
    pol.selection = None
    m, s = P.average_returns(pol, P.HipVecEnv(**ref.env_kw_of(case)), case["episodes"])
    assert abs(m - v.mean()) <= 1e-12 * (1 + abs(v.mean())) and abs(s - v.std(ddof=1)) <= 1e-12 * (1 + v.std(ddof=1))


# ---------------------------------------------------------------- 3. the searches
def _assert_closes(P, env, starts, got):
    back = P.apply_paths_(env, *starts, got["path"])
    bad = _mismatches(dict(best_state=back["state"], best_active=back["active"], best_gap=back["gap"], best_step=back["applied"]),
                      got, ("best_state", "best_active", "best_gap", "best_step"))
    assert not bad, bad


@pytest.mark.parametrize("sel", S.SEARCH_SELECTIONS, ids=_sid)
def test_search_best_states(P, orc, sel):
    M, K, N, T = S.SEARCH_SHAPE
    want = S.search(orc, S.SEARCH_SHAPE, sel)
    pol = _policy(P, S.rref.policy_params(orc), S.rref.CASE["hid"], S.rref.CASE["L"], sel)
    starts = S.search_starts(orc, M, T)
    env = P.HipVecEnv(**S.search_env_kw(N, T))
    before = _env_state(P, env)
    got = P.search_best_states_(env, pol, *starts, K, clone_gaps=True, path=True)
    assert env.error_flags() & ~32 == 0
    bad = _mismatches(got, dict(want, path=pref.one_based(want["path"])), RESULT + ("clone_gaps", "path"))
    print(sel, "best gaps", want["best_gap"].tolist(), "path lengths", want["best_step"].tolist(), "mismatches", bad)
    assert not bad, (sel, bad)
    after = _env_state(P, env)
    assert np.array_equal(after["tick"], want["tick"]) and np.array_equal(after["episode"], before["episode"])
    assert after["done"][:M * K].all()
    _assert_closes(P, env, starts, got)
    if sel[0] == "greedy":          # K clones of a start play one trajectory: the lowest clone wins every tie
        assert np.all(got["clone_gaps"] == got["clone_gaps"][:, :1]) and np.all(got["best_clone"] == 0)


@pytest.mark.parametrize("sel", S.SEARCH_SELECTIONS, ids=_sid)
@pytest.mark.parametrize("shape", S.RESAMPLE_SHAPES, ids=lambda s: "M%d-K%d-N%d-T%d-R%d-m%d" % s)
def test_search_resample_states(P, orc, shape, sel):
    M, K, N, T, R, m0 = shape
    want = S.resample(orc, shape, sel)
    pol = _policy(P, S.rref.policy_params(orc), S.rref.CASE["hid"], S.rref.CASE["L"], sel)
    starts = S.search_starts(orc, M, T)
    env = P.HipVecEnv(**S.rref.env_kw(shape))
    before = _env_state(P, env)
    got = P.search_resample_states_(env, pol, *starts, K, R, m0, donors=True, clone_gaps=True, path=True)
    assert env.error_flags() & ~32 == 0
    bad = _mismatches(got, dict(want, path=pref.one_based(want["path"])), RESULT + ("donors", "clone_gaps", "path"))
    print(shape, sel, "best gaps", want["best_gap"].tolist(), "fold events", want["fold_event"].tolist(), "mismatches", bad)
    assert not bad, (shape, sel, bad)
    after = _env_state(P, env)
    assert np.array_equal(after["tick"], want["tick"]) and np.array_equal(after["episode"], before["episode"])
    _assert_closes(P, env, starts, got)
    if sel[0] == "greedy":
        assert np.all(got["clone_gaps"] == got["clone_gaps"][:, :1]) and np.all(got["best_clone"] == 0)


# ---------------------------------------------------------------- 4. one step: the action and p_sel
def _step_reference(orc, kw, params, hid, L, warm, sel):
    """Actions, p_sel and flags of one selection step of every env of a fresh env that has played `warm` default steps."""
    o = ref._env(orc, kw)
    o.reset()
    if warm:
        orc.collect_rollouts_tn(o, params, hid, warm, mode_dev=True, n_hidden=L)
    tick = o.tick.copy()
    out = [S.select_action(orc, o, n, params, hid, L, *sel) for n in range(o.N)]
    assert np.array_equal(o.tick, tick)
    return np.array([a for a, _, _ in out], np.int32), np.array([p[a] for a, p, _ in out], np.float32), tick


@pytest.mark.parametrize("sel", S.SELECTIONS, ids=_sid)
@pytest.mark.parametrize("Q,hid,N", [(8, 256, 70), (32, 128, 9)], ids=["q8-h256", "q32-h128"])
def test_single_step_action_and_p_sel(P, orc, Q, hid, N, sel):
    warm = 3
    kw = dict(num_envs=N, Q=Q, max_actions=12, seed=ref.SEED, global_offset=900)
    params = orc.glorot_params(ref.F, hid, 2, seed=3)
    pol = _policy(P, params, hid, 2, sel)
    env = P.HipVecEnv(**kw)
    P.collect_rollouts_steps_(P.BufferRollouts(), env, pol, warm, 1.0)         # a collector: plays the default whatever is set
    want_a, want_p, tick = _step_reference(orc, kw, params, hid, 2, warm, sel)
    before = _env_state(P, env)
    assert np.array_equal(before["tick"], tick)
    got_a, got_p = _debug_step(P, pol, env)
    print(sel, Q, hid, "action mismatches", int((got_a != want_a).sum()), "p_sel mismatches",
          int((got_p.view(np.uint32) != want_p.view(np.uint32)).sum()))
    assert np.array_equal(got_a, want_a)
    assert np.array_equal(got_p.view(np.uint32), want_p.view(np.uint32)), "p_sel bitwise"
    after = _env_state(P, env)
    assert all(np.array_equal(before[k], after[k]) for k in before) and env.error_flags() & ~32 == 0
    # the default selection from the same states and ticks: the sampled step as it always was
    pol.selection = None
    base_a, base_p, _ = _step_reference(orc, kw, params, hid, 2, warm, S.DEFAULT)
    got_a, got_p = _debug_step(P, pol, env)
    assert np.array_equal(got_a, base_a) and np.array_equal(got_p.view(np.uint32), base_p.view(np.uint32))


# ---------------------------------------------------------------- 5. ties
@pytest.mark.parametrize("tau", (1.0, 0.7))
@pytest.mark.parametrize("Q,hid,L", [(8, 128, 2), (8, 256, 2), (32, 128, 2), (32, 256, 3)],
                         ids=["q8-h128", "q8-h256", "q32-h128", "q32-h256-L3"])
def test_greedy_ties_go_to_the_lowest_index(P, orc, Q, hid, L, tau):
    masks = S.TIE_MASKS_Q8 if Q == 8 else S.TIE_MASKS_Q32
    pol = _policy(P, S.tie_params(orc, hid, L), hid, L, ("greedy", tau))
    env = P.HipVecEnv(num_envs=len(masks), Q=Q, max_actions=4, seed=ref.SEED)
    env.set_internal(*S.tie_states(masks, Q))
    got_a, got_p = _debug_step(P, pol, env)
    want = [S.tie_expected(orc, m, Q, tau) for m in masks]
    assert got_a.tolist() == [16 * S.lowest_quad(m) + 1 for m in masks] == [a for a, _ in want]
    assert np.array_equal(got_p.view(np.uint32), np.array([p for _, p in want], np.float32).view(np.uint32))
    assert env.error_flags() == 0
    # through a public call: the first action of every env's trajectory (1-based)
    got = P._best_states(env, pol, len(masks), False, False, False, True)
    assert got["actions"][:, 0].tolist() == [16 * S.lowest_quad(m) + 2 for m in masks]


# ---------------------------------------------------------------- 6. 1100 envs
@pytest.mark.parametrize("sel", (("sample", 0.7), ("greedy", 1.0)), ids=_sid)
@pytest.mark.parametrize("case", S.BIG, ids=lambda c: c["name"])
def test_1100_envs(P, orc, case, sel):
    """The replayed columns (both sides of every multiple of 64, the first and the last env) against the reference; every env
    through the closure: the first best_step actions lead from the env's reset state to best_state."""
    N, M = case["N"], case["M"]
    kw = ref.env_kw_of(case)
    pol = _case_policy(P, orc, case, sel)
    env = P.HipVecEnv(**kw)
    got = P.best_states_(env, pol, N, scores=True, action_types=True, actions=True)
    assert env.error_flags() & ~32 == 0
    cols = S.grid_columns(N)
    want = S.trajectories(orc, case, sel, cols, 1)
    bad = _mismatches({k: got[k][cols] for k in RECORD + ("actions",)}, dict(want, actions=pref.one_based(want["actions"])),
                      RECORD + ("actions",))
    assert not bad, (case["name"], sel, bad)
    assert np.array_equal(_env_state(P, env)["tick"], got["length"]) and np.array_equal((got["actions"] > 0).sum(axis=1), got["length"])
    o = ref._env(orc, kw)
    o.episode[:] = 1
    o.reset()
    prefix = got["actions"].copy()
    prefix[np.arange(M)[None, :] >= got["best_step"][:, None]] = 0
    back = P.apply_paths_(env, o.score, o.degree, o.active.astype(np.uint32), prefix)
    assert np.array_equal(back["state"], got["best_state"]) and np.array_equal(back["gap"], got["best_gap"])
    assert np.array_equal(back["active"], got["best_active"]) and np.array_equal(back["applied"], got["best_step"])


# ---------------------------------------------------------------- 7. unchanged ground
def test_collectors_forward_and_training_do_not_read_the_selection(P, orc):
    kw = dict(num_envs=24, Q=8, max_actions=8, seed=ref.SEED, global_offset=0)
    params = orc.glorot_params(ref.F, 128, 2, seed=3)

    def run(sel):
        pol = _policy(P, params, 128, 2, sel)
        out = {}
        for name, collect in (("episodes", lambda ro, env: P.collect_rollouts_(ro, env, pol, 30, 0.9)),
                              ("steps", lambda ro, env: P.collect_rollouts_steps_(ro, env, pol, 9, 0.9, record_probs=True))):
            env, ro = P.HipVecEnv(**kw), P.BufferRollouts()
            collect(ro, env)
            st, act = ro.state_data
            out[name] = [ro.selected_actions, ro.selected_action_probabilities, ro.rewards, ro.terminal, ro.valid, st, act,
                         env.internal()["tick"]]
            if name == "steps":
                out[name].append(ro.full_probs())
                ds = P.construct_dataset(ro)
                out["loss"] = list(P.forward_backward(pol, ds, np.arange(1, 101), 0.05, 0.01))
                out["grad"] = [pol.grad()]
                out["probs"] = [P.batch_action_probabilities(pol, P.StateData(st[0], act[0]))]
        env, ro = P.HipVecEnv(**kw), P.BufferRollouts()
        it = env.internal()
        rng = np.random.default_rng(2)
        paths = (16 * rng.integers(0, 6, (24, 5)) + 4 * rng.integers(0, 4, (24, 5)) + rng.integers(0, 2, (24, 5)) + 1).astype(np.int16)
        P.collect_paths_(ro, env, pol, it["score"], it["degree"], env.active_quads(), paths, 0.9, record_probs=True)
        out["paths"] = [ro.selected_actions, ro.selected_action_probabilities, ro.rewards, ro.valid, ro.full_probs()]
        return out
    base = run(None)
    for sel in (("greedy", 0.7), ("sample", 2.0)):
        got = run(sel)
        for k in base:
            assert len(got[k]) == len(base[k])
            for a, b in zip(got[k], base[k]):
                assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), (sel, k)


def test_none_restores_the_default(P, orc):
    """selection = None behind a greedy call: the sampled results of a handle that was never set, from the same ticks."""
    case = S.SIDE[0]
    fields = RECORD + ("actions",)

    def greedy_then(default_pol_of):
        pol = _case_policy(P, orc, case, ("greedy", 1.0))
        env = P.HipVecEnv(**ref.env_kw_of(case))
        first = P.best_states_(env, pol, case["episodes"], scores=True, action_types=True, actions=True)
        second = P.best_states_(env, default_pol_of(pol), case["episodes"], scores=True, action_types=True, actions=True)
        return first, second, _env_state(P, env)

    def cleared(pol):
        pol.selection = None
        assert pol.selection == S.DEFAULT
        return pol
    g1, s1, e1 = greedy_then(cleared)
    g2, s2, e2 = greedy_then(lambda pol: _case_policy(P, orc, case))
    assert not _mismatches(g1, g2, fields) and not _mismatches(s1, s2, fields)
    assert all(np.array_equal(e1[k], e2[k]) for k in e1)
    assert _mismatches(s1, g1, ("actions",)), "the sampled call is not the greedy one"
    with P.selecting(_case_policy(P, orc, case, ("sample", 2.0)), "greedy", 0.5) as pol:
        assert pol.selection == ("greedy", 0.5)
    assert pol.selection == ("sample", 2.0)
    for v, want in (("greedy", ("greedy", 1.0)), ("sample", S.DEFAULT), (("greedy", 3), ("greedy", 3.0))):
        pol.selection = v
        assert pol.selection == want


# ---------------------------------------------------------------- 8. refusals
def test_refusals(P, orc):
    pol = P.HipPolicy(ref.F, 128, 2, 4, seed=1)
    pol.selection = ("sample", 0.7)
    for bad in (("sample", 0.0), ("sample", -1.0), ("greedy", float("nan")), ("sample", float("inf")), ("argmax", 1.0), "softmax"):
        with pytest.raises(P.PPOError) as ei:
            pol.selection = bad
        assert ei.value.status == -1, bad
    L = P._lib.lib()
    for rule, t in ((2, 1.0), (0, 0.0), (0, -1.0), (1, float("nan")), (0, float("inf"))):
        assert L.ppo_policy_set_selection(pol._h, rule, t) == -1, (rule, t)
    assert pol.selection == ("sample", 0.7), "a refused value leaves the selection as it was"
    # bf16: the setter makes no device call and accepts; the calls that read the selection refuse
    env = P.HipVecEnv(num_envs=8, Q=8, max_actions=5, seed=ref.SEED)
    b = P.HipPolicy(ref.F, 128, 2, 4, seed=1, dtype="bf16")
    b.selection = "greedy"
    for call in (lambda: P.best_states_(env, b, 8), lambda: P.evaluate_trajectories(env, b, 8, "best"),
                 lambda: P.average_returns(b, env, 8)):
        with pytest.raises(P.PPOError) as ei:
            call()
        assert ei.value.status == -4 and "bf16" in str(ei.value)
    b.selection = None
    assert P.best_states_(env, b, 8)["best_gap"].shape == (8,)
    # a generic (host) env samples at temperature 1: a non-default selection is refused there, the default is not
    class HostEnv:
        pass
    for fn in (lambda p: P.best_state_in_rollout(HostEnv(), p), lambda p: P.single_trajectory_scores(HostEnv(), p),
               lambda p: P.count_non_flips(HostEnv(), p), lambda p: P.average_returns(p, HostEnv(), 2),
               lambda p: P.single_trajectory_return(p, HostEnv())):
        with pytest.raises(NotImplementedError):
            fn(pol)
        pol.selection = None
        with pytest.raises(Exception) as ei:                  # the host loop itself, which finds no plugin method for HostEnv
            fn(pol)
        assert not isinstance(ei.value, NotImplementedError)
        pol.selection = ("sample", 0.7)
