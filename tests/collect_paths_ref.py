"""Host reference of the teacher-forced collection (collect_paths_): the [T, N] columns the call must leave in
the rollout buffer and the env state it must leave behind.  Everything here comes from the CPU oracle (oracle/oracle.py),
numpy, tests/episodes_ref.py, tests/search_ref.py, tests/resample_ref.py and tests/path_ref.py, never from the device.

The rule.  A fresh device env holds the reset of episode counter 0 (the counter is then 1, the ticks 0).  Envs 0 .. M - 1 are
loaded with the starts as reset! leaves an env (steps 0, not terminal, reward 0); the episode counters and ticks stay.  A
path's declared length is the index of its first negative entry, at most stride; T = max(1, longest declared length).  At
loop step t every env is observed; env n then idles when n >= M, t >= its declared length or it is terminal, and plays
paths[n][t] otherwise:

  idle      action -1, p_sel 0, reward 0, done 1, valid 0; the env is not touched;
  playing   p_sel = action_probabilities(.., mode="dev")[action] of the state in front of the step, step_one, reward =
            the env's reward, done = the env's done OR t + 1 == declared length, valid 1;
  playing an action on an inactive quad: step_one all the same (it counts, penalises and changes nothing else), p_sel 0,
            valid 0.

index = the valid transitions env-major, returns = compute_returns_tn over the raw rewards and done.

Paths here are 0-based and padded with -1, as the C ABI takes them; path_ref.one_based() is what Python takes.
The path sets and the shape table of tests/test_collect_paths_host.py and tests/test_gpu_collect_paths.py live at the end."""
import numpy as np

import episodes_ref as ref
import path_ref as pref
import resample_ref as rref
import search_ref as sref

NO_ACTION_REWARD = -4.0          # the env's default, oracle and device


def declared_lengths(paths):
    neg = paths < 0
    return np.where(neg.any(axis=1), neg.argmax(axis=1), paths.shape[1]).astype(np.int64)


def expected(orc, env_kw, params, hid, L, starts, paths, discount):
    """The buffer and the env collect_paths_ leaves on a FRESH env of env_kw for starts = (score [M, V], degree [M, V], active
    [M]) and paths int16 [M, stride] (0-based).  Returns dict(T, states, active, actions, p_sel, rewards, done, valid, index,
    returns: the columns; gap_after [T, N]: current_score - opt_score behind a played step, -1 elsewhere; lengths [M];
    played [M]: steps each path really played; env: score, degree, active, tick, episode, done, steps as the call leaves
    them; env_before: the same of the fresh env)."""
    N = env_kw["num_envs"]
    M, stride = paths.shape
    assert 1 <= M <= N and stride >= 1 and starts[2].shape == (M,)
    e = ref._env(orc, env_kw)
    e.reset()
    before = _env_state(e)
    for m in range(M):
        e.score[m], e.degree[m], e.active[m] = starts[0][m], starts[1][m], starts[2][m]
        e.steps[m], e.done[m], e.reward[m] = 0, 0, 0.0
    lens = declared_lengths(paths)
    T = max(1, int(lens.max()))
    r = dict(states=np.zeros((T, N, e.H, e.F), np.int8), active=np.zeros((T, N), np.uint32), actions=np.full((T, N), -1, np.int32),
             p_sel=np.zeros((T, N), np.float32), rewards=np.zeros((T, N), np.float32), done=np.ones((T, N), np.uint8),
             valid=np.zeros((T, N), bool), gap_after=np.full((T, N), -1, np.int64), rejected=np.zeros((T, N), bool))
    played = np.zeros(M, np.int64)
    for t in range(T):
        obs = e.observe_all()
        r["states"][t], r["active"][t] = obs, e.active
        for n in range(M):
            if t >= lens[n] or e.done[n]:
                continue
            a, act = int(paths[n, t]), int(e.active[n])
            on = bool((act >> (a >> 4)) & 1)
            p = orc.action_probabilities(params, ref.F, hid, obs[n], act, "dev", n_hidden=L)
            held = sref.state_of(e, n)
            e.step_one(n, a)
            now = sref.state_of(e, n)
            r["rejected"][t, n] = np.array_equal(held[0], now[0]) and np.array_equal(held[1], now[1]) and held[2] == now[2]
            played[n] += 1
            r["actions"][t, n], r["p_sel"][t, n] = a, (p[a] if on else 0.0)
            r["rewards"][t, n] = e.reward[n]
            r["done"][t, n] = int(bool(e.done[n]) or t + 1 == lens[n])
            r["valid"][t, n] = on
            r["gap_after"][t, n] = sref.score_gap(e.score[n], int(e.active[n]))[1]
    r["index"] = ref.env_major_index(r["valid"])
    r["returns"] = orc.compute_returns_tn(r["rewards"], r["done"], float(discount), isinstance(discount, np.float32))
    r.update(T=T, lengths=lens, played=played, env=_env_state(e), env_before=before)
    return r


def _env_state(e):
    return dict(score=e.score.copy(), degree=e.degree.copy(), active=e.active.copy().astype(np.uint32), tick=e.tick.copy(),
                episode=e.episode.copy(), done=e.done.copy().astype(bool), steps=e.steps.copy())


def cut_transitions(exp):
    """Truncations in the sense of DESIGN.md 7f: done && valid with the optimum not reached behind the step -- a path cut
    short of the optimum by its last entry, or by the env's time limit."""
    return exp["done"].astype(bool) & exp["valid"] & (exp["gap_after"] != 0)


# ---------------------------------------------------------------- random legal paths
def reset_starts(orc, Q, max_actions, count, offset):
    """The reset states (episode counter 1) of `count` envs of global ids offset ..: what search_ref.search_starts does."""
    e = orc.Env(Q=Q, max_actions=max_actions, N=count, seed=ref.SEED, global_offset=offset)
    e.episode[:] = 1
    e.reset()
    return e.score.copy(), e.degree.copy(), e.active.copy().astype(np.uint32)


def random_path(orc, rng, Q, max_actions, start, length):
    """`length` 0-based entries, each a move (any type) on a quad that is active when it is played, found by stepping the
    oracle env; the entries behind a terminal state (never played) are moves on the quads active then."""
    e = orc.Env(Q=Q, max_actions=max_actions, N=1, seed=ref.SEED)
    e.score[0], e.degree[0], e.active[0] = start
    e.steps[0], e.done[0], e.reward[0] = 0, 0, 0.0
    out = []
    for _ in range(length):
        quads = np.flatnonzero([(int(e.active[0]) >> q) & 1 for q in range(Q)])
        a = 16 * int(rng.choice(quads)) + int(rng.integers(16))
        out.append(a)
        if not e.done[0]:
            e.step_one(0, a)
    assert int(e.err[0]) == 0
    return out


# ---------------------------------------------------------------- path sets
Q8_MAX_ACTIONS = rref.SHAPES["B"][3]             # 20: the env of the resampling reference the searched paths come from
Q8_STRIDE = Q8_MAX_ACTIONS + 4
Q32_MAX_ACTIONS, Q32_STRIDE = 5, 6
SOLVED_START = 4                                 # start of resample shape B whose result is solved (tests/test_search_paths_host.py)


def q8_set(orc):
    """Nine paths on Q = 8, max_actions 20, stride 24, in the order the smaller cases cut it (the first M rows):
      0  empty;  1  stride entries, no padding (the time limit cuts it with entries to spare);  2  exactly max_actions entries;
      3  the searched path of shape B's solved start with three entries behind the optimum, never played;
      4  the searched path of shape B's start 0, cut short of the optimum;  5 .. 6  random, 1 and 7 entries, cut short;
      7 .. 8  the searched paths of shape B's starts 1 and 2.
    Rows 0 .. 2, 5, 6 start from reset states of their own, the searched rows from the starts of their search."""
    key = ("collect-paths", "q8")
    if key not in ref._CACHE:
        Q, T = rref.CASE["Q"], Q8_MAX_ACTIONS
        found = pref.resample_reference(orc, "B")
        sst = sref.search_starts(orc, rref.SHAPES["B"][0])
        own = reset_starts(orc, Q, T, 5, 700)
        rng = np.random.default_rng(11)
        rows, starts = [], []

        def add(start, path):
            starts.append(start)
            rows.append(list(path))

        def searched(s, extra=()):
            n = int(found["best_step"][s])
            add((sst[0][s], sst[1][s], int(sst[2][s])), [int(a) for a in found["path"][s, :n]] + list(extra))
        for i, length in enumerate((0, Q8_STRIDE, T)):
            st = (own[0][i], own[1][i], int(own[2][i]))
            add(st, random_path(orc, rng, Q, T, st, length))
        searched(SOLVED_START, (0, 1, 2))
        searched(0)
        for i, length in ((3, 1), (4, 7)):
            st = (own[0][i], own[1][i], int(own[2][i]))
            add(st, random_path(orc, rng, Q, T, st, length))
        searched(1)
        searched(2)
        ref._CACHE[key] = (_stack_starts(starts), pref.padded(rows, Q8_STRIDE))
    return ref._CACHE[key]


def q32_set(orc):
    """Five paths on Q = 32, max_actions 5, stride 6: empty, full stride, exactly max_actions, 2 and 4 entries."""
    key = ("collect-paths", "q32")
    if key not in ref._CACHE:
        own = reset_starts(orc, 32, Q32_MAX_ACTIONS, 5, 900)
        rng = np.random.default_rng(12)
        starts = [(own[0][i], own[1][i], int(own[2][i])) for i in range(5)]
        rows = [random_path(orc, rng, 32, Q32_MAX_ACTIONS, starts[i], n) for i, n in enumerate((0, Q32_STRIDE, Q32_MAX_ACTIONS, 2, 4))]
        ref._CACHE[key] = (_stack_starts(starts), pref.padded(rows, Q32_STRIDE))
    return ref._CACHE[key]


OFFQUAD_MAX_ACTIONS, OFFQUAD_STRIDE, OFFQUAD_ROW, OFFQUAD_STEP = 6, 4, 1, 1


def offquad_set(orc):
    """Three paths on Q = 8, max_actions 6, stride 4.  Row 1 is flip, a move on quad 7 (inactive in a reset state and left so
    by flips), flip: the step on the inactive quad is played in the middle of the path.  Rows 0 and 2: three random entries."""
    key = ("collect-paths", "offquad")
    if key not in ref._CACHE:
        own = reset_starts(orc, 8, OFFQUAD_MAX_ACTIONS, 3, 1100)
        rng = np.random.default_rng(13)
        starts = [(own[0][i], own[1][i], int(own[2][i])) for i in range(3)]
        rows = [random_path(orc, rng, 8, OFFQUAD_MAX_ACTIONS, starts[i], 3) for i in range(3)]
        assert not (starts[1][2] >> 7) & 1
        rows[OFFQUAD_ROW] = [16 * 0 + 4 * 1 + 0, 16 * 7 + 5, 16 * 2 + 4 * 3 + 1]
        ref._CACHE[key] = (_stack_starts(starts), pref.padded(rows, OFFQUAD_STRIDE))
    return ref._CACHE[key]


def _stack_starts(starts):
    return (np.stack([s[0] for s in starts]).astype(np.int8), np.stack([s[1] for s in starts]).astype(np.int8),
            np.array([s[2] for s in starts], np.uint32))


SETS = {"q8": q8_set, "q32": q32_set, "offquad": offquad_set}

# ---------------------------------------------------------------- shapes: the smallest that reach every template family
DISCOUNT = 0.9


def _shape(name, pset, N, M, hid, L=2, pseed=3, goff=40, forms=("expanded",)):
    return dict(name=name, set=pset, N=N, M=M, hid=hid, L=L, pseed=pseed, goff=goff, forms=tuple(forms))


SHAPES = [
    _shape("h256-12x9", "q8", 12, 9, 256, forms=ref.BOTH),        # HID = 256, one wave per SIMD; idle envs behind M
    _shape("h128-8x8", "q8", 8, 8, 128),                          # HID = 128, two waves per SIMD; M == N
    _shape("q32-6x5", "q32", 6, 5, 128, forms=ref.BOTH),          # TPS = 4
    _shape("L3-8x6", "q8", 8, 6, 128, L=3),                       # DEEP
    _shape("h96-8x7", "q8", 8, 7, 96),                            # a padded width
]
OFFQUAD_SHAPE = _shape("offquad-4x3", "offquad", 4, 3, 128)
RUNS = [(s, form) for s in SHAPES for form in s["forms"]]
CONSUMER_SHAPES = ("h256-12x9", "h128-8x8")


def by_name(name):
    return next(s for s in SHAPES + [OFFQUAD_SHAPE] if s["name"] == name)


def max_actions_of(pset):
    return {"q8": Q8_MAX_ACTIONS, "q32": Q32_MAX_ACTIONS, "offquad": OFFQUAD_MAX_ACTIONS}[pset]


def env_kw(shape):
    return dict(num_envs=shape["N"], Q=32 if shape["set"] == "q32" else 8, max_actions=max_actions_of(shape["set"]), seed=ref.SEED,
                global_offset=shape["goff"])


def policy_params(orc, shape):
    return orc.glorot_params(ref.F, shape["hid"], shape["L"], seed=shape["pseed"])


def inputs(orc, shape):
    """(starts, paths) of a shape: the first M rows of its path set."""
    starts, paths = SETS[shape["set"]](orc)
    M = shape["M"]
    return tuple(a[:M] for a in starts), paths[:M]


def reference(orc, name):
    """expected() of one shape, once per process and never modified."""
    key = ("collect-paths-ref", name)
    if key not in ref._CACHE:
        shape = by_name(name)
        starts, paths = inputs(orc, shape)
        ref._CACHE[key] = expected(orc, env_kw(shape), policy_params(orc, shape), shape["hid"], shape["L"], starts, paths, DISCOUNT)
    return ref._CACHE[key]


# ---------------------------------------------------------------- the reward identity of a replayed path
def reward_identity(exp, starts, n):
    """For path n of a reference: (sum of its raw rewards, score(start) - score(end), rejected, opt_moved).  step! rewards
    old_total - new_total of an accepted move and no_action_reward of a rejected one, which leaves the state as it was, so
        sum of rewards == score(start) - score(end) + no_action_reward * rejected
    always holds, and sum == initial_gap - end_gap exactly where no move was rejected and opt_score (|sum of the vertex
    scores|, which moves of types 2 and 3 change) is the same at both ends."""
    sc0, act0 = starts[0][n], int(starts[2][n])
    sc1, act1 = exp["env"]["score"][n], int(exp["env"]["active"][n])
    cur0, gap0 = sref.score_gap(sc0, act0)
    cur1, gap1 = sref.score_gap(sc1, act1)
    ts = np.flatnonzero(exp["actions"][:, n] >= 0)
    total = float(exp["rewards"][ts, n].astype(np.float64).sum())
    return total, cur0 - cur1, int(exp["rejected"][:, n].sum()), (cur0 - gap0) != (cur1 - gap1)
