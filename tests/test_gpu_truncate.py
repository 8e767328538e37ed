"""Top-k / nucleus truncation on the device (HipPolicy.truncation; k_policy_fwd mode 16) against the CPU oracle.
Every comparison is exact equality, p_sel bitwise.  tests/truncate_ref.py holds the reference; tests/test_truncate_host.py
checks it without a device and asserts that the cases choose other actions than the untruncated sampler.

1. best_states_(actions, scores, action types) in the reset form on Policy(72,256,2,4), Q = 8, 70 envs, 100 trajectories,
   max_actions 20 under five (selection, truncation) pairs; on the side shapes (hidden 128, three hidden layers, hidden 96,
   Q = 32) under ("sample", 0.7) + (3, 0.8); ticks, episode counters and done flags after each call;
2. the action and p_sel of a single step (ppo_debug_select_step) for 70 envs in mid-trajectory states at hidden 256 and 9 envs
   at Q = 32 under every truncation, then the default again from the same ticks; top_k = 1 is greedy with p_sel 1;
3. ties: logits (0, 1, 1, 0) on every row -- top_k = 3 keeps the three lowest-indexed maxima (p_sel 1/3, the action among
   them over several ticks); top_p = 0.5 on uniform maxima keeps half of them, the strict <;
4. 1100 envs at hidden 256 (a second pass of the forward's grid) and 128;
5. search_best_states_ and search_resample_states_ with the closure on the device;
6. unchanged ground: the collectors, batch_action_probabilities, the gradient and greedy do not read the truncation; None
   restores the default;
7. refusals."""
import ctypes as C

import numpy as np
import pytest

import episodes_ref as ref
import path_ref as pref
import select_ref as S
import truncate_ref as T

pytestmark = pytest.mark.gpu

RECORD = ("best_state", "best_active", "best_gap", "best_step", "length", "initial_gap", "trace", "type_counts")
RESULT = ("best_state", "best_active", "best_gap", "best_clone", "best_step", "initial_gap")


@pytest.fixture(scope="module")
def P(ppo):
    if ppo.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests must run on the GPU box")
    return ppo


def _tid(pair):
    (rule, tau), (k, p) = pair
    return "%s-%g-k%d-p%g" % (rule, tau, k, p)


def _policy(P, params, hid, L, sel=None, trunc=None):
    pol = P.HipPolicy(ref.F, hid, L, 4, seed=0)
    pol.params = params
    if sel is not None:
        pol.selection = sel
    if trunc is not None:
        pol.truncation = trunc                                   # without the feature the file fails here
        assert pol.truncation == (int(trunc[0]), float(trunc[1]))
    return pol


def _case_policy(P, orc, case, sel=None, trunc=None):
    return _policy(P, ref.policy_params(orc, case), case["hid"], case["L"], sel, trunc)


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


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


# ---------------------------------------------------------------- 1. whole trajectories
def _check_reset_form(P, orc, case, sel, trunc):
    pol = _case_policy(P, orc, case, sel, trunc)
    env = P.HipVecEnv(**ref.env_kw_of(case))
    got = P.best_states_(env, pol, case["episodes"], scores=True, action_types=True, actions=True)
    assert env.error_flags() & ~32 == 0
    want, cols = T.best_states(orc, case, sel, trunc), T.episodes(orc, case, sel, trunc)
    bad = _mismatches(got, dict(want, actions=pref.one_based(want["actions"])), RECORD + ("actions",))
    print(case["name"], sel, trunc, "trajectories", case["episodes"], "steps", int(want["length"].sum()), "mismatches", bad)
    assert not bad, (case["name"], sel, trunc, bad)
    after = _env_state(P, env)
    assert np.array_equal(after["tick"], cols["tick"]) and np.array_equal(after["episode"], cols["episode"])
    assert after["done"].all()


@pytest.mark.parametrize("pair", T.MAIN_CASES, ids=_tid)
def test_best_states_main_shape(P, orc, pair):
    _check_reset_form(P, orc, S.MAIN, *pair)


@pytest.mark.parametrize("case", S.SIDE, ids=lambda c: c["name"])
def test_best_states_side_shapes(P, orc, case):
    _check_reset_form(P, orc, case, *T.SIDE_CASE)


# ---------------------------------------------------------------- 2. one step: the action and p_sel
def _warm_env(orc, kw, params, hid, L, warm):
    """A fresh oracle env that has played `warm` default steps (select_action does not step: one env serves every truncation)."""
    o = ref._env(orc, kw)
    o.reset()
    orc.collect_rollouts_tn(o, params, hid, warm, mode_dev=True, n_hidden=L)
    return o


def _step_reference(orc, o, params, hid, L, sel, trunc):
    """Actions and p_sel of one step of every env of `o` from the states and ticks it holds."""
    tick = o.tick.copy()
    out = [T.select_action(orc, o, n, params, hid, L, *sel, trunc) for n in range(o.N)]
    assert np.array_equal(o.tick, tick)
    return np.array([a for a, _, _ in out], np.int32), np.array([p[a] for a, p, _ in out], np.float32)


@pytest.mark.parametrize("sel", (("sample", 0.7), ("sample", 1.0)), ids=lambda s: "%s-%g" % s)
@pytest.mark.parametrize("Q,hid,N", [(8, 256, 70), (32, 128, 9)], ids=["q8-h256", "q32-h128"])
def test_single_step_action_and_p_sel(P, orc, Q, hid, N, sel):
    warm = 3
    kw = dict(num_envs=N, Q=Q, max_actions=12, seed=ref.SEED, global_offset=900)
    params = orc.glorot_params(ref.F, hid, 2, seed=3)
    pol = _policy(P, params, hid, 2, sel)
    env = P.HipVecEnv(**kw)
    P.collect_rollouts_steps_(P.BufferRollouts(), env, pol, warm, 1.0)         # a collector: plays the default whatever is set
    o = _warm_env(orc, kw, params, hid, 2, warm)
    before = _env_state(P, env)
    assert np.array_equal(before["tick"], o.tick)
    greedy_a, _ = _step_reference(orc, o, params, hid, 2, ("greedy", sel[1]), T.DEFAULT)
    for trunc in T.TRUNCATIONS + ((16 * Q, 1.0), (16 * Q + 5, 1.0)):             # the last two keep everything and renormalise
        want_a, want_p = _step_reference(orc, o, params, hid, 2, sel, trunc)
        pol.truncation = trunc
        got_a, got_p = _debug_step(P, pol, env)
        print(sel, trunc, Q, hid, "action mismatches", int((got_a != want_a).sum()), "p_sel mismatches",
              int((_bits(got_p) != _bits(want_p)).sum()))
        assert np.array_equal(got_a, want_a), trunc
        assert np.array_equal(_bits(got_p), _bits(want_p)), ("p_sel bitwise", trunc)
        if trunc == (1, 1.0):
            assert np.array_equal(got_a, greedy_a) and np.all(got_p == np.float32(1.0))
        after = _env_state(P, env)
        assert all(np.array_equal(before[k], after[k]) for k in before) and env.error_flags() & ~32 == 0
    # the default truncation from the same states and ticks: the selection's step as it was
    pol.truncation = None
    base_a, base_p = _step_reference(orc, o, params, hid, 2, sel, T.DEFAULT)
    got_a, got_p = _debug_step(P, pol, env)
    assert np.array_equal(got_a, base_a) and np.array_equal(_bits(got_p), _bits(base_p))


# ---------------------------------------------------------------- 3. ties
@pytest.mark.parametrize("Q,hid,L", [(8, 128, 2), (8, 256, 2), (32, 128, 2), (32, 256, 3)],
                         ids=["q8-h128", "q8-h256", "q32-h128", "q32-h256-L3"])
def test_ties_rank_by_the_lower_index(P, orc, Q, hid, L):
    masks = T.TIE_MASKS_Q8 if Q == 8 else T.TIE_MASKS_Q32
    pol = _policy(P, S.tie_params(orc, hid, L), hid, L, ("sample", 1.0), (3, 1.0))
    env = P.HipVecEnv(num_envs=len(masks), Q=Q, max_actions=3, seed=ref.SEED)
    states = S.tie_states(masks, Q)
    env.set_internal(*states)
    maxima = [T.tie_maxima(m, Q) for m in masks]
    third = [T.truncate(T.tie_probabilities(orc, m, Q), 3, 1.0)[mx[0]] for m, mx in zip(masks, maxima)]
    seen = [set() for _ in masks]
    for _ in range(12):                                   # several ticks: a rejected or accepted move, the mask is set again
        got_a, got_p = _debug_step(P, pol, env)
        for n, mx in enumerate(maxima):
            assert int(got_a[n]) in mx[:3], (hex(masks[n]), int(got_a[n]))
            seen[n].add(int(got_a[n]))
        assert np.array_equal(_bits(got_p), _bits(third)), "p_sel = 1/3 as the reference rounds it"
        P._best_states(env, pol, len(masks), False, False, False, False)        # moves the ticks on
        env.set_internal(*states)
    assert env.error_flags() & ~32 == 0
    assert all(len(s) >= 2 for s in seen), "the ticks reach more than one of the three kept maxima"
    # uniform maxima, 1 / n each with n a power of two: top_p = 0.5 keeps the n / 2 lowest-indexed (mass_before < 0.5, strictly)
    pol.selection = ("sample", T.TIE_UNIFORM_TAU)
    pol.truncation = (0, 0.5)
    for _ in range(6):
        got_a, got_p = _debug_step(P, pol, env)
        for n, mx in enumerate(maxima):
            assert int(got_a[n]) in mx[:len(mx) // 2], (hex(masks[n]), int(got_a[n]))
        assert np.array_equal(_bits(got_p), _bits([2.0 / len(mx) for mx in maxima]))
        P._best_states(env, pol, len(masks), False, False, False, False)
        env.set_internal(*states)


# ---------------------------------------------------------------- 4. 1100 envs
@pytest.mark.parametrize("case", S.BIG, ids=lambda c: c["name"])
def test_1100_envs(P, orc, case):
    """The replayed columns (both sides of every multiple of 64, the first and the last env) against the reference, one
    trajectory each; at hidden 256 envs 1024 .. 1099 are a wave's second state."""
    sel, trunc = T.SIDE_CASE
    N = case["N"]
    pol = _case_policy(P, orc, case, sel, trunc)
    env = P.HipVecEnv(**ref.env_kw_of(case))
    got = P.best_states_(env, pol, N, scores=True, action_types=True, actions=True)
    assert env.error_flags() & ~32 == 0
    cols = S.grid_columns(N)
    assert {1023, 1024, 1099} <= set(cols)
    want = T.trajectories(orc, case, sel, trunc, cols, 1)
    bad = _mismatches({k: got[k][cols] for k in RECORD + ("actions",)}, dict(want, actions=pref.one_based(want["actions"])),
                      RECORD + ("actions",))
    assert not bad, (case["name"], bad)
    assert np.array_equal(_env_state(P, env)["tick"], got["length"])


# ---------------------------------------------------------------- 5. the searches
def _assert_closes(P, env, starts, got):
    back = P.apply_paths_(env, *starts, got["path"])
    bad = _mismatches(dict(best_state=back["state"], best_active=back["active"], best_gap=back["gap"], best_step=back["applied"]),
                      got, ("best_state", "best_active", "best_gap", "best_step"))
    assert not bad, bad


def test_search_best_states(P, orc):
    sel, trunc = T.SEARCH_CASE
    M, K, N, Tm = T.SEARCH_SHAPE
    want = T.search(orc, T.SEARCH_SHAPE, sel, trunc)
    pol = _policy(P, S.rref.policy_params(orc), S.rref.CASE["hid"], S.rref.CASE["L"], sel, trunc)
    starts = S.search_starts(orc, M, Tm)
    env = P.HipVecEnv(**S.search_env_kw(N, Tm))
    before = _env_state(P, env)
    got = P.search_best_states_(env, pol, *starts, K, clone_gaps=True, path=True)
    assert env.error_flags() & ~32 == 0
    bad = _mismatches(got, dict(want, path=pref.one_based(want["path"])), RESULT + ("clone_gaps", "path"))
    print(sel, trunc, "best gaps", want["best_gap"].tolist(), "path lengths", want["best_step"].tolist(), "mismatches", bad)
    assert not bad, bad
    after = _env_state(P, env)
    assert np.array_equal(after["tick"], want["tick"]) and np.array_equal(after["episode"], before["episode"])
    assert after["done"][:M * K].all()
    _assert_closes(P, env, starts, got)


def test_search_resample_states(P, orc):
    sel, trunc = T.SEARCH_CASE
    shape = T.RESAMPLE_SHAPE
    M, K, N, Tm, R, m0 = shape
    want = T.resample(orc, shape, sel, trunc)
    pol = _policy(P, S.rref.policy_params(orc), S.rref.CASE["hid"], S.rref.CASE["L"], sel, trunc)
    starts = S.search_starts(orc, M, Tm)
    env = P.HipVecEnv(**S.rref.env_kw(shape))
    before = _env_state(P, env)
    got = P.search_resample_states_(env, pol, *starts, K, R, m0, donors=True, clone_gaps=True, path=True)
    assert env.error_flags() & ~32 == 0
    bad = _mismatches(got, dict(want, path=pref.one_based(want["path"])), RESULT + ("donors", "clone_gaps", "path"))
    print(shape, sel, trunc, "best gaps", want["best_gap"].tolist(), "mismatches", bad)
    assert not bad, bad
    after = _env_state(P, env)
    assert np.array_equal(after["tick"], want["tick"]) and np.array_equal(after["episode"], before["episode"])
    _assert_closes(P, env, starts, got)


# ---------------------------------------------------------------- 6. unchanged ground
def test_collectors_forward_training_and_greedy_do_not_read_the_truncation(P, orc):
    kw = dict(num_envs=24, Q=8, max_actions=8, seed=ref.SEED, global_offset=0)
    params = orc.glorot_params(ref.F, 128, 2, seed=3)
    fields = RECORD + ("actions",)

    def run(trunc):
        pol = _policy(P, params, 128, 2, None, trunc)
        out = {}
        env, ro = P.HipVecEnv(**kw), P.BufferRollouts()
        P.collect_rollouts_(ro, env, pol, 30, 0.9)
        st, act = ro.state_data
        out["episodes"] = [ro.selected_actions, ro.selected_action_probabilities, ro.rewards, ro.terminal, ro.valid, st, act,
                           env.internal()["tick"]]
        out["probs"] = [P.batch_action_probabilities(pol, P.StateData(st[0], act[0]))]
        ds = P.construct_dataset(ro)
        out["loss"] = list(P.forward_backward(pol, ds, np.arange(1, 101), 0.05, 0.01))
        out["grad"] = [pol.grad()]
        env, ro = P.HipVecEnv(**kw), P.BufferRollouts()
        it = env.internal()
        rng = np.random.default_rng(2)
        paths = (16 * rng.integers(0, 6, (24, 5)) + 4 * rng.integers(0, 4, (24, 5)) + rng.integers(0, 2, (24, 5)) + 1).astype(np.int16)
        P.collect_paths_(ro, env, pol, it["score"], it["degree"], env.active_quads(), paths, 0.9, record_probs=True)
        out["paths"] = [ro.selected_actions, ro.selected_action_probabilities, ro.rewards, ro.valid, ro.full_probs()]
        with P.selecting(pol, "greedy", 1.0, *(trunc or (0, 1.0))):
            assert pol.truncation == (trunc or (0, 1.0))
            g = P.best_states_(P.HipVecEnv(**kw), pol, 30, scores=True, action_types=True, actions=True)
        assert pol.selection == ("sample", 1.0) and pol.truncation == (trunc or (0, 1.0))
        out["greedy"] = [g[k] for k in fields]
        return out, pol
    base, _ = run(None)
    got, pol = run((2, 0.5))
    for k in base:
        assert len(got[k]) == len(base[k])
        for a, b in zip(got[k], base[k]):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), k
    # truncation = None: the default's results from the same ticks as a handle that was never set
    def sampled_after(pol_of):
        p = _policy(P, params, 128, 2, None, (2, 0.5))
        env = P.HipVecEnv(**kw)
        first = P.best_states_(env, p, 30, scores=True, action_types=True, actions=True)
        second = P.best_states_(env, pol_of(p), 30, scores=True, action_types=True, actions=True)
        return first, second, _env_state(P, env)

    def cleared(p):
        p.truncation = None
        assert p.truncation == (0, 1.0)
        return p
    t1, s1, e1 = sampled_after(cleared)
    t2, s2, e2 = sampled_after(lambda p: _policy(P, params, 128, 2))
    assert not _mismatches(t1, t2, fields) and not _mismatches(s1, s2, fields)
    assert all(np.array_equal(e1[k], e2[k]) for k in e1)
    assert _mismatches(t1, s1, ("actions",)), "the truncated call is not the default one"


# ---------------------------------------------------------------- 7. refusals
def test_refusals(P, orc):
    pol = P.HipPolicy(ref.F, 128, 2, 4, seed=1)
    pol.truncation = (3, 0.8)
    assert P.HipPolicy(ref.F, 128, 2, 4, seed=1).truncation == (0, 1.0), "a fresh handle holds the default truncation"
    for bad in ((-1, 1.0), (0, 0.0), (0, -0.5), (0, 1.5), (0, float("nan")), (1.5, 1.0), ("3", 1.0)):
        with pytest.raises(P.PPOError) as ei:
            pol.truncation = bad
        assert ei.value.status == -1, bad
    L = P._lib.lib()
    for k, p in ((-1, 1.0), (0, 0.0), (0, -1.0), (0, float("nan")), (0, 1.0000001), (0, float("inf"))):
        assert L.ppo_policy_set_truncation(pol._h, k, p) == -1, (k, p)
    assert pol.truncation == (3, 0.8), "a refused value leaves the truncation as it was"
    # bf16: the setter makes no device call and accepts; the calls that read the truncation refuse, with their own message
    env = P.HipVecEnv(num_envs=8, Q=8, max_actions=5, seed=ref.SEED)
    b = P.HipPolicy(ref.F, 128, 2, 4, seed=1, dtype="bf16")
    b.truncation = (2, 1.0)
    for call in (lambda: P.best_states_(env, b, 8), lambda: P.evaluate_trajectories(env, b, 8, "best"),
                 lambda: P.average_returns(b, env, 8)):
        with pytest.raises(P.PPOError) as ei:
            call()
        assert ei.value.status == -4 and "bf16" in str(ei.value) and "truncation" in str(ei.value)
    b.truncation = None
    assert P.best_states_(env, b, 8)["best_gap"].shape == (8,)
    # a generic (host) env samples from the whole distribution: a non-default truncation is refused there, the default is not
    class HostEnv:
        pass
    for fn in (lambda p: P.best_state_in_rollout(HostEnv(), p), lambda p: P.single_trajectory_scores(HostEnv(), p),
               lambda p: P.count_non_flips(HostEnv(), p), lambda p: P.average_returns(p, HostEnv(), 2),
               lambda p: P.single_trajectory_return(p, HostEnv())):
        with pytest.raises(NotImplementedError):
            fn(pol)
        pol.truncation = None
        with pytest.raises(Exception) as ei:                  # the host loop itself, which finds no plugin method for HostEnv
            fn(pol)
        assert not isinstance(ei.value, NotImplementedError)
        pol.truncation = (3, 0.8)
