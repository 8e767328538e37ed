"""Teacher-forced collection on the device (ppo_collect_paths) against the CPU oracle.  Every comparison is exact
equality unless stated.  tests/collect_paths_ref.py holds the reference and the path sets; tests/test_collect_paths_host.py
checks both without a device and asserts that the sets contain what matters here: an empty path, a path of stride entries, a
path of max_actions steps, a path solved before its entries end, paths cut short of the optimum, idle envs, searched paths.

1. every column, len, dims, index, returns and the envs afterwards against the reference, in every template family;
2. grid-wide self-consistency at 1100 envs, where no CPU replay is affordable;
3. closure with the resampling search: valid transitions == best_step, and the reward identity that holds;
4. the consumers: forward_backward against the float64 oracle, compute_gae_critic_(bootstrap_truncated=True), ppo_train_,
   value_train_, compute_values_;
5. refused arguments, each with its error class, and the inactive-quad path;
6. a sampled collection after a teacher-forced one on the same handles."""
import numpy as np
import pytest

import collect_paths_ref as cref
import episodes_ref as ref
import path_ref as pref
import resample_ref as rref
import search_ref as sref

pytestmark = pytest.mark.gpu

COLUMNS = ("states", "active", "actions", "p_sel", "rewards", "done", "valid", "returns", "index")


@pytest.fixture(scope="module")
def P(ppo):
    if ppo.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests must run on the GPU box")
    return ppo


def _policy(P, orc, shape, dtype="f32"):
    pol = P.HipPolicy(ref.F, shape["hid"], shape["L"], 4, seed=0, dtype=dtype)
    pol.params = cref.policy_params(orc, shape)
    return pol


def _columns(ro):
    st, act = ro.state_data
    return dict(states=st, active=act, actions=(ro.selected_actions - 1).astype(np.int32), p_sel=ro.selected_action_probabilities,
                rewards=ro.raw_rewards, done=ro.terminal.astype(np.uint8), valid=ro.valid, returns=ro.rewards, index=ro.index())


def _env_state(P, env):
    it = env.internal()
    return dict(score=it["score"], degree=it["degree"], active=env.active_quads(), tick=it["tick"], episode=it["episode"],
                done=P.is_terminal(env).astype(bool), steps=it["steps"])


def _mismatches(got, want, keys):
    out = {}
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.shape != w.shape:
            out[k] = (g.shape, w.shape)
        elif g.dtype == np.float32:                     # bitwise
            if not np.array_equal(g.view(np.uint32), w.astype(np.float32).view(np.uint32)):
                out[k] = int(np.count_nonzero(g.view(np.uint32) != w.astype(np.float32).view(np.uint32)))
        elif not np.array_equal(g, w):
            out[k] = int(np.count_nonzero(g != w))
    return out


def _collect(P, orc, shape, form="expanded", record_probs=False, pol=None):
    starts, paths = cref.inputs(orc, shape)
    env = P.HipVecEnv(**cref.env_kw(shape))
    pol = pol or _policy(P, orc, shape)
    ro = P.BufferRollouts()
    P.set_rollout_compact(form == "compact")
    try:
        P.collect_paths_(ro, env, pol, *starts, pref.one_based(paths), cref.DISCOUNT, record_probs=record_probs)
    finally:
        P.set_rollout_compact(None)
    return env, pol, ro


# ---------------------------------------------------------------- 1. the columns against the reference
@pytest.mark.parametrize("shape,form", cref.RUNS, ids=lambda x: x["name"] if isinstance(x, dict) else x)
def test_columns_against_reference(P, orc, shape, form):
    exp = cref.reference(orc, shape["name"])
    fresh = _env_state(P, P.HipVecEnv(**cref.env_kw(shape)))
    assert not _mismatches(fresh, exp["env_before"], fresh), "the reference starts from the device's fresh env"
    env, pol, ro = _collect(P, orc, shape, form)
    assert ro.dims() == (exp["T"], shape["N"]) and len(ro) == len(exp["index"]) == int(exp["valid"].sum())
    got = _columns(ro)
    bad = _mismatches(got, exp, COLUMNS)
    print(shape["name"], form, "T", exp["T"], "transitions", len(ro), "played", exp["played"].tolist(), "mismatches", bad)
    assert not bad, bad
    assert (got["p_sel"][got["valid"]] > 0).all() and (got["p_sel"][~got["valid"]] == 0).all()
    # the envs: final states of the paths, ticks advanced by the steps played, episode counters and the envs behind M untouched
    after = _env_state(P, env)
    assert not _mismatches(after, exp["env"], after)
    M = shape["M"]
    assert all(np.array_equal(after[k][M:], fresh[k][M:]) for k in after), "envs >= M are as they were"
    assert np.array_equal(after["episode"], fresh["episode"])
    assert np.array_equal(after["tick"][:M].astype(np.int64), exp["played"])
    assert env.error_flags() == 0
    # the same call again on the same handles: the starts are loaded again, only the ticks differ
    starts, paths = cref.inputs(orc, shape)
    P.set_rollout_compact(form == "compact")
    try:
        P.collect_paths_(ro, env, pol, *starts, pref.one_based(paths), cref.DISCOUNT)
    finally:
        P.set_rollout_compact(None)
    assert not _mismatches(_columns(ro), exp, COLUMNS)
    assert np.array_equal(env.internal()["tick"][:M].astype(np.int64), 2 * exp["played"])


# ---------------------------------------------------------------- 2. grid-wide self-consistency
def test_grid_wide_self_consistency(P, orc):
    """1100 envs, Policy(72,256,2,4): 275 workgroups of the forward against a grid of 256 (a second pass for some waves), and
    the env step's last block of 64 is partial.  Paths from the device's own best-of-1 search."""
    N, T = 1100, 6
    kw = dict(num_envs=N, Q=8, max_actions=T, seed=ref.SEED, global_offset=2000)
    shape = dict(hid=256, L=2, pseed=5)
    pol = _policy(P, orc, shape)
    src = P.HipVecEnv(**kw)
    it = src.internal()
    starts = (it["score"], it["degree"], src.active_quads())
    found = P.search_best_states_(src, pol, *starts, 1, path=True)
    lens = (found["path"] > 0).sum(axis=1)
    assert np.array_equal(lens, found["best_step"]) and lens.max() == T and (lens == 0).any()
    env = P.HipVecEnv(**kw)
    ro = P.BufferRollouts()
    P.collect_paths_(ro, env, pol, *starts, found["path"], 1.0, record_probs=True)
    assert ro.dims() == (T, N)
    got = _columns(ro)
    valid = got["valid"]
    print("1100 envs: paths per length", np.bincount(lens, minlength=T + 1).tolist(), "transitions", len(ro))
    assert np.array_equal(valid.sum(axis=0), found["best_step"]) and len(ro) == int(found["best_step"].sum())
    assert np.array_equal(got["actions"], np.where(np.arange(T)[:, None] < lens[None, :], found["path"].T.astype(np.int32) - 1, -1))
    # p_sel == the MODE 0 forward on the buffer's own states at the forced action; full_probs == that forward
    probs = P.batch_action_probabilities(pol, P.StateData(got["states"].reshape(-1, 32, ref.F), got["active"].reshape(-1))).T
    probs = np.ascontiguousarray(probs).reshape(T, N, 128)
    want = np.take_along_axis(probs, np.maximum(got["actions"], 0)[:, :, None], axis=2)[:, :, 0]
    want = np.where(valid, want, np.float32(0)).astype(np.float32)
    assert np.array_equal(got["p_sel"].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(ro.full_probs().view(np.uint32), probs.view(np.uint32))
    # the state behind each path's last step (what the env holds now) == apply_paths_'s == the search's best state
    back = P.apply_paths_(env, *starts, found["path"])
    after = _env_state(P, env)
    state = np.concatenate([after["score"], after["degree"]], axis=1)
    assert np.array_equal(state, back["state"]) and np.array_equal(after["active"], back["active"])
    assert np.array_equal(state, found["best_state"]) and np.array_equal(back["applied"], found["best_step"])
    assert np.array_equal(after["tick"].astype(np.int64), lens) and env.error_flags() == 0
    # every path is one episode: its last valid transition is terminal, none before it
    last = np.zeros((T, N), bool)
    last[lens[lens > 0] - 1, np.flatnonzero(lens > 0)] = True
    assert np.array_equal(got["done"].astype(bool) & valid, last)


# ---------------------------------------------------------------- 3. closure with the resampling search
def test_closure_with_resampling_search(P, orc):
    """search_resample_states_(path=True), then collect_paths_(starts, path).  The number of valid transitions of a path is
    best_step.  The sum of its raw rewards is NOT initial_gap - best_gap in general (tests/test_collect_paths_host.py shows it
    on the CPU reference: moves of types 2 and 3 change opt_score, and a rejected move costs no_action_reward without moving
    the score).  The identity that holds, and is held here:
        sum of rewards == score(start) - score(best_state) + no_action_reward * rejected moves,
    and == initial_gap - best_gap on the paths without a rejected move whose opt_score is the same at both ends."""
    name = "B"
    M, K, N, T, R, m0 = rref.SHAPES[name]
    pol = P.HipPolicy(ref.F, rref.CASE["hid"], rref.CASE["L"], 4, seed=0)
    pol.params = rref.policy_params(orc)
    starts = sref.search_starts(orc, M)
    env = P.HipVecEnv(**rref.env_kw(rref.SHAPES[name]))
    found = P.search_resample_states_(env, pol, *starts, K, R, m0, path=True)
    env2 = P.HipVecEnv(**dict(rref.env_kw(rref.SHAPES[name]), num_envs=M + 2))
    ro = P.BufferRollouts()
    P.collect_paths_(ro, env2, pol, *starts, found["path"], 1.0)
    got = _columns(ro)
    assert np.array_equal(got["valid"].sum(axis=0)[:M], found["best_step"]) and not got["valid"][:, M:].any()
    trace = P.apply_paths_(env2, *starts, found["path"], scores=True)["trace"]
    exact = 0
    for m in range(M):
        k = int(found["best_step"][m])
        rew = got["rewards"][:k, m].astype(np.float64)
        drop = np.diff(np.concatenate([[0], trace[m, :k].astype(np.int64)]))
        rejected = int(((rew == cref.NO_ACTION_REWARD) & (drop == 0)).sum())
        cur0, gap0 = sref.score_gap(starts[0][m], int(starts[2][m]))
        cur1, gap1 = sref.score_gap(found["best_state"][m, :32], int(found["best_active"][m]))
        assert gap0 == found["initial_gap"][m] and gap1 == found["best_gap"][m]
        assert rew.sum() == cur0 - cur1 + cref.NO_ACTION_REWARD * rejected, m
        if rejected == 0 and cur0 - gap0 == cur1 - gap1:
            assert rew.sum() == found["initial_gap"][m] - found["best_gap"][m]
            exact += 1
    print("resample", name, "best_step", found["best_step"].tolist(), "paths with sum == initial_gap - best_gap:", exact)


# ---------------------------------------------------------------- 4. the consumers
@pytest.mark.parametrize("name,form", list(zip(cref.CONSUMER_SHAPES, ("compact", "expanded"))))
def test_consumers(P, orc, name, form):
    shape = cref.by_name(name)
    exp = cref.reference(orc, name)
    env, pol, ro = _collect(P, orc, shape, form)
    got = _columns(ro)
    ds = P.construct_dataset(ro)
    n = len(ds)
    assert n == len(exp["index"])
    idx = got["index"]
    # forward_backward on the whole dataset against the float64 oracle fed with the buffer's own columns: 2e-5 of max|g|
    lp, le = P.forward_backward(pol, ds, np.arange(1, n + 1), 0.05, 0.01)
    g = pol.grad()
    g64, olp, ole = orc.step_batch_grad_f64(cref.policy_params(orc, shape), ref.F, shape["hid"], got["states"].reshape(-1, 32, ref.F)[idx],
                                            got["active"].reshape(-1)[idx], got["actions"].reshape(-1)[idx], got["p_sel"].reshape(-1)[idx],
                                            got["returns"].reshape(-1)[idx], 0.05, 0.01, n_hidden=shape["L"])
    err = float(np.abs(g - g64).max())
    print(name, form, "transitions", n, "grad err", err, "max|g|", float(np.abs(g64).max()))
    assert err <= 2e-5 * np.abs(g64).max()
    assert abs(lp - olp) <= 1e-5 * (1 + abs(olp)) and abs(le - ole) <= 1e-5 * (1 + abs(ole))
    # the critic: values, GAE bootstrapped through the cut paths, value training
    critic = P.HipCritic(ref.F, shape["hid"], shape["L"], seed=1)
    v = P.compute_values_(ro, env, critic)
    assert v.shape == (exp["T"] + 1, shape["N"]) and np.isfinite(v).all()
    adv, lam = P.compute_gae_critic_(ro, env, critic, 0.99, 0.95, bootstrap_truncated=True)
    cut = cref.cut_transitions(exp)
    assert ro.n_truncated == int(cut.sum()) > 0
    boot = ro.boot_values
    assert np.isfinite(adv).all() and np.isfinite(lam).all() and (boot[~cut] == 0).all()
    mh, _ = P.value_train_(critic, P.Optimiser(P.Adam(1e-4)), ds, n, 1, target="lambda_returns", verbose=False)
    assert np.isfinite(mh).all()
    # one epoch of one minibatch: the ratios are 1 before the first update, so nothing is clipped
    pol.target_kl = float("inf")
    ph, eh, _ = P.ppo_train_(pol, P.Optimiser(P.Adam(1e-4)), ds, 0.05, n, 1, 0.01, verbose=False)
    stats = pol.last_train_stats()
    print(name, "ppo loss", ph, "entropy loss", eh, stats)
    assert np.isfinite(ph).all() and np.isfinite(eh).all()
    assert stats["epochs_run"] == 1 and stats["clip_fraction"] == [0.0] and abs(stats["approx_kl"][0]) < 1e-6


# ---------------------------------------------------------------- 5. refused arguments
def test_refused_arguments(P, orc, tmp_path):
    shape = cref.by_name("h128-8x8")
    starts, paths = cref.inputs(orc, shape)
    ok = pref.one_based(paths)
    kw = cref.env_kw(shape)
    env, pol, ro = P.HipVecEnv(**kw), _policy(P, orc, shape), P.BufferRollouts()

    def status(*args, **kwargs):
        with pytest.raises(P.PPOError) as err:
            P.collect_paths_(*args, **kwargs)
        return err.value.status

    small = P.HipVecEnv(**dict(kw, num_envs=shape["M"] - 1))
    assert status(P.BufferRollouts(), small, pol, *starts, ok, 1.0) == -1, "M > N"
    assert status(ro, env, pol, starts[0], starts[1], np.zeros_like(starts[2]), ok, 1.0) == -1, "a start without an active quad"
    dirty = starts[0].copy()
    dirty[2, 4 * 7] = 1                                  # quad 7 is inactive in a reset state
    assert status(ro, env, pol, dirty, starts[1], starts[2], ok, 1.0) == -1, "a nonzero entry of an inactive quad"
    big = ok.copy()
    big[3, 0] = 16 * kw["Q"] + 1
    assert status(ro, env, pol, *starts, big, 1.0) == -1, "an entry beyond 16 Q"
    assert status(ro, env, pol, *starts, ok[:, :0], 1.0) == -1, "stride 0"
    # the C entry point checks the same itself
    L = P._lib
    ptr = lambda a, t: a.ctypes.data_as(t)
    h = ro._ensure(env, 1)
    raw = np.ascontiguousarray(paths)

    def cstatus(e, M, active, rows, stride):
        return L.lib().ppo_collect_paths(h, e._h, pol._h, M, ptr(starts[0], L.c_i8p), ptr(starts[1], L.c_i8p), ptr(active, L.c_u32p),
                                         ptr(rows, L.c_i16p), stride, 1.0, 0, 0)
    over = raw.copy()
    over[3, 0] = 16 * kw["Q"]
    assert cstatus(env, shape["N"] + 1, starts[2], raw, raw.shape[1]) == -1 and cstatus(env, 0, starts[2], raw, raw.shape[1]) == -1
    assert cstatus(env, shape["M"], np.zeros_like(starts[2]), raw, raw.shape[1]) == -1
    assert cstatus(env, shape["M"], starts[2], over, raw.shape[1]) == -1 and cstatus(env, shape["M"], starts[2], raw, 0) == -1
    # unsupported: a bf16 policy, a disk sink attached to the buffer
    assert status(ro, env, _policy(P, orc, shape, dtype="bf16"), *starts, ok, 1.0) == -4
    L.call("ppo_rollouts_attach_disk", h, str(tmp_path / "sink").encode(), 4)
    try:
        assert status(ro, env, pol, *starts, ok, 1.0) == -4
    finally:
        L.call("ppo_rollouts_detach_disk", h)
    # nothing ran: the env is as created
    fresh = _env_state(P, P.HipVecEnv(**kw))
    assert not _mismatches(_env_state(P, env), fresh, fresh) and env.error_flags() == 0
    P.collect_paths_(ro, env, pol, *starts, ok, cref.DISCOUNT)          # and the handles still work
    assert not _mismatches(_columns(ro), cref.reference(orc, shape["name"]), COLUMNS)


def test_action_on_an_inactive_quad(P, orc):
    shape = cref.OFFQUAD_SHAPE
    exp = cref.reference(orc, shape["name"])
    starts, paths = cref.inputs(orc, shape)
    env, pol, ro = P.HipVecEnv(**cref.env_kw(shape)), _policy(P, orc, shape), P.BufferRollouts()
    with pytest.raises(P.PPOError, match="inactive quad") as err:
        P.collect_paths_(ro, env, pol, *starts, pref.one_based(paths), cref.DISCOUNT)
    assert err.value.status == -3
    got = _columns(ro)                                   # the buffer is filled
    assert ro.dims() == (exp["T"], shape["N"]) and len(ro) == len(exp["index"])
    assert not _mismatches(got, exp, COLUMNS)
    r, t = cref.OFFQUAD_ROW, cref.OFFQUAD_STEP
    assert not got["valid"][t, r] and got["p_sel"][t, r] == 0 and got["actions"][t, r] == paths[r, t]
    assert got["rewards"][t, r] == cref.NO_ACTION_REWARD and t * shape["N"] + r not in got["index"]
    assert not _mismatches(_env_state(P, env), exp["env"], exp["env"])
    assert env.error_flags() == 0, "the flag is the call's, the env handle stays clean"
    n = len(ro)
    lp, le = P.forward_backward(pol, P.construct_dataset(ro), np.arange(1, n + 1), 0.05, 0.01)
    assert np.isfinite(lp) and np.isfinite(le) and np.isfinite(pol.grad()).all(), "no ratio divides by 0"


# ---------------------------------------------------------------- 6. nothing else moved
def test_sampled_collection_after_paths(P, orc):
    """collect_rollouts_ after collect_paths_ on the same handles.  The paths advanced the ticks of the envs that played (the
    sampler's Philox counter), so a fresh env cannot give the same columns; what must hold: (a) the buffer handle is as good
    as new -- the same two calls with the sampled collection going into a fresh buffer give the same columns; (b) the env
    handle carries nothing but its counters -- the columns are the oracle's episodes form started from the episode counters
    (unchanged) and ticks (advanced by the steps played) the reference says the call left."""
    shape = cref.by_name("h128-8x8")
    exp = cref.reference(orc, shape["name"])
    kw, N, E = cref.env_kw(shape), shape["N"], shape["N"] + 3
    env, pol, ro = _collect(P, orc, shape)
    P.collect_rollouts_(ro, env, pol, E, cref.DISCOUNT)
    got = _columns(ro)
    env2, _, _ = _collect(P, orc, shape, pol=pol)
    ro2 = P.BufferRollouts()
    P.collect_rollouts_(ro2, env2, pol, E, cref.DISCOUNT)
    assert ro.dims() == ro2.dims() and len(ro) == len(ro2)
    assert not _mismatches(got, _columns(ro2), COLUMNS)
    want = ref.expected_episodes(orc, kw, cref.policy_params(orc, shape), shape["hid"], shape["L"], E,
                                 episode0=exp["env"]["episode"], tick0=exp["env"]["tick"])
    T = ro.dims()[0]
    assert T == max(c["length"] for c in want.values())
    cols = ref.assemble(want, N, T, 32)
    assert np.array_equal(got["valid"], cols["valid"])
    v = cols["valid"]                                    # the rows of an env behind its quota hold no transition
    assert not _mismatches({k: got[k][v] for k in cols}, {k: cols[k][v] for k in cols},
                           ("states", "active", "actions", "p_sel", "rewards", "done"))
    assert env.error_flags() & ~32 == 0
