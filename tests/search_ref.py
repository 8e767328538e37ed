"""Host reference of the best-state bookkeeping (best_state_in_rollout, single_trajectory_scores, count_non_flips:
test/quad_game_utilities.jl:309-323,341-358, test/random_quad.jl:9-27) and of the best-of-K search built on it.  Everything
here comes from the CPU oracle (oracle/oracle.py), numpy and tests/episodes_ref.py, never from the device.

The reference keeps a copy of the wrapper behind every step of a trajectory, the start state first, and returns the copy at
argmin(current_score - opt_score): Julia's argmin returns the FIRST minimum.  Traj keeps the same list; record() reads the
answer off it.

Three replays:
  tracked_replay   teacher-forced (the device's actions), every env of an episodes-form call, integer work only;
  play_from        the full replay (oracle forward in "dev" mode + Philox sampling keyed on (global env id, tick)) of ONE
                   trajectory from a supplied state;
  search_replay    play_from over the round / clone / tick schedule of the best-of-K search.

The case and shape tables of tests/test_search_host.py and tests/test_gpu_search.py live at the end of the file."""
import numpy as np

import episodes_ref as ref

INT32_MIN = -2 ** 31


# ---------------------------------------------------------------- one env's state and scores
def state_of(oenv, n):
    return oenv.score[n].copy(), oenv.degree[n].copy(), int(oenv.active[n])


def score_gap(sc, act):
    """(current_score, current_score - opt_score) of one state: sum |vertex score| over the active quads, minus |sum|."""
    on = ((act >> (np.arange(sc.size) >> 2)) & 1).astype(bool)
    s = sc.astype(np.int64)[on]
    cur = int(np.abs(s).sum())
    return cur, cur - abs(int(s.sum()))


def first_argmin(gaps):
    """The bookkeeping the device runs, on a plain gap sequence (start state first): the candidate is replaced on a strictly
    lower gap only.  Returns (best gap, its index)."""
    best, at = gaps[0], 0
    for t in range(1, len(gaps)):
        if gaps[t] < best:
            best, at = gaps[t], t
    return int(best), at


class Traj:
    """The copies and scores best_state_in_rollout keeps while one trajectory runs."""

    def __init__(self, oenv, n):
        st = state_of(oenv, n)
        self.init, gap = score_gap(st[0], st[2])
        self.states, self.gaps, self.trace, self.types = [st], [gap], [], [0, 0, 0, 0]

    def after(self, oenv, n, action):
        st = state_of(oenv, n)
        cur, gap = score_gap(st[0], st[2])
        self.states.append(st)
        self.gaps.append(gap)
        self.trace.append(self.init - cur)            # single_trajectory_scores
        self.types[action % 4] += 1                   # count_non_flips: types 2 and 3

    def record(self):
        gap, at = first_argmin(self.gaps)
        sc, dg, act = self.states[at]
        return dict(best_state=np.concatenate([sc, dg]), best_active=act, best_gap=gap, best_step=at,
                    length=len(self.trace), initial_gap=self.gaps[0], trace=list(self.trace), type_counts=list(self.types),
                    gaps=list(self.gaps))


def stack(records, max_actions):
    """Per-trajectory records -> the arrays best_states_ returns (trace padded with INT32_MIN); `gaps` stays a list."""
    n = len(records)
    out = dict(best_state=np.stack([r["best_state"] for r in records]).astype(np.int8),
               best_active=np.array([r["best_active"] for r in records], np.uint32),
               trace=np.full((n, max_actions), INT32_MIN, np.int64),
               type_counts=np.array([r["type_counts"] for r in records], np.int32).reshape(n, 4),
               gaps=[r["gaps"] for r in records])
    for k in ("best_gap", "best_step", "length", "initial_gap"):
        out[k] = np.array([r[k] for r in records], np.int32)
    for i, r in enumerate(records):
        out["trace"][i, :len(r["trace"])] = r["trace"]
    out["trace"] = out["trace"].astype(np.int32)
    return out


# ---------------------------------------------------------------- teacher-forced, every env
def tracked_replay(orc, env_kw, actions, num_traj, episode0=None, tick0=None):
    """ref.teacher_forced's loop with the bookkeeping: the oracle env of all N columns stepped with the given 0-based actions
    [T, N], reset before the first trajectory and before each further one of an env's quota.  Returns stack() of the
    num_traj records, env-major (env n's trajectories are consecutive), plus episode / tick [N] as the call leaves them."""
    N, M = env_kw["num_envs"], env_kw["max_actions"]
    oenv = ref._env(orc, env_kw)
    oenv.episode[:] = 1 if episode0 is None else episode0
    if tick0 is not None:
        oenv.tick[:] = tick0
    oenv.reset()
    left = ref.quotas(N, num_traj)
    recs, cur = [[] for _ in range(N)], [None] * N
    for t in range(actions.shape[0]):
        busy = np.flatnonzero(left > 0)
        if busy.size == 0:
            break
        for n in (int(x) for x in busy):
            if cur[n] is None:
                cur[n] = Traj(oenv, n)
            a = int(actions[t, n])
            oenv.step_one(n, a)
            cur[n].after(oenv, n, a)
            if oenv.done[n]:
                recs[n].append(cur[n].record())
                cur[n] = None
                left[n] -= 1
                if left[n] > 0:
                    oenv.reset_one(n)
    assert not (left > 0).any(), "the actions do not finish the quotas"
    assert np.all(oenv.err == 0)
    out = stack([r for n in range(N) for r in recs[n]], M)
    out.update(episode=oenv.episode.copy(), tick=oenv.tick.copy())
    return out


# ---------------------------------------------------------------- the full replay from a supplied state
def play_from(orc, env_kw, n, params, hid, L, start, tick0):
    """One trajectory of env n (global id offset + n) from start = (score [V], degree [V], active) at tick tick0, the env left
    as reset! leaves one: the oracle's own rollout (forward in "dev" mode, sampling keyed on (global id, tick)) gives the
    actions up to the first terminal, a second pass from the same state keeps the copies.  Returns Traj.record()."""
    M = env_kw["max_actions"]

    def load():
        e = ref._env(orc, env_kw, 1, n)
        e.score[0], e.degree[0], e.active[0] = start[0], start[1], start[2]
        e.steps[0], e.done[0], e.reward[0], e.tick[0] = 0, 0, 0.0, tick0
        return e
    e = load()
    r = orc.collect_rollouts_tn(e, params, hid, M, mode_dev=True, n_hidden=L)
    length = int(np.flatnonzero(r["done"][:, 0])[0]) + 1
    e = load()
    tr = Traj(e, 0)
    for t in range(length):
        e.step_one(0, int(r["actions"][t, 0]))
        tr.after(e, 0, int(r["actions"][t, 0]))
    assert e.done[0] and int(e.err[0]) == 0 and int(e.tick[0]) == tick0 + length
    return tr.record()


def search_replay(orc, env_kw, params, hid, L, starts, K, tick0=None):
    """The best-of-K search: rounds of S = N // K starts; in a round env n < S_r * K plays start base + n // K as clone n % K
    from the tick it holds, the other envs idle (their ticks do not move).  starts = (score [M, V], degree [M, V], active
    [M]).  The winner of a start: lowest best gap, ties to the lowest clone (np.argmin: the first minimum), then that clone's
    first minimum.  Returns the arrays search_best_states_ returns, plus tick [N] afterwards."""
    N = env_kw["num_envs"]
    M = starts[2].shape[0]
    S = N // K
    tick = np.zeros(N, np.int64) if tick0 is None else np.asarray(tick0, np.int64).copy()
    win, clone_gaps, best_clone = [], np.zeros((M, K), np.int32), np.zeros(M, np.int32)
    for base in range(0, M, S):
        for s in range(base, min(base + S, M)):
            recs = []
            for c in range(K):
                n = (s - base) * K + c
                recs.append(play_from(orc, env_kw, n, params, hid, L, (starts[0][s], starts[1][s], int(starts[2][s])),
                                      int(tick[n])))
                tick[n] += recs[-1]["length"]
            clone_gaps[s] = [r["best_gap"] for r in recs]
            best_clone[s] = int(np.argmin(clone_gaps[s]))
            win.append(recs[best_clone[s]])
    out = stack(win, env_kw["max_actions"])
    out.update(best_clone=best_clone, clone_gaps=clone_gaps, tick=tick)
    return out


# ---------------------------------------------------------------- cases
# best_states_ (reset before every trajectory): cases of tests/episodes_ref.py, so the trajectories are the ones
# collect_rollouts_ plays and tests/test_gpu_episodes_form.py ties to the oracle
CASES = ("1x3", "70x100", "q32-20x30", "L3-40x60", "257x515")
# ... of which these are replayed on the host (every column, from the oracle's own rollout) for what they must contain
COVERAGE_CASES = ("70x100", "q32-20x30", "L3-40x60")
# per case: trajectories, best at the start, at the last step, strictly in between, minimum reached more than once, more
# than one improvement (the oracle at seed 13, policy seed 3)
COVERAGE = {"70x100": (100, 51, 11, 38, 69, 16), "q32-20x30": (30, 16, 5, 9, 21, 8), "L3-40x60": (60, 35, 7, 18, 47, 8)}


def coverage(rec):
    """(trajectories, best at the start, best at the last step, best strictly in between, minimum reached more than once,
    more than one improvement) of a stacked record."""
    step, length = rec["best_step"], rec["length"]
    tied = sum(1 for g in rec["gaps"] if g.count(min(g)) > 1)
    several = sum(1 for g in rec["gaps"] if np.count_nonzero(np.diff(np.minimum.accumulate(g)) < 0) > 1)
    return (len(step), int((step == 0).sum()), int(((step == length) & (step > 0)).sum()),
            int(((step > 0) & (step < length)).sum()), tied, several)


def oracle_record(orc, case):
    """tracked_replay of the case's own oracle rollout (ref.reference, every column): needs N <= 70.  Once per process."""
    key = ("tracked", case["name"])
    if key not in ref._CACHE:
        assert case["N"] <= 70
        exp = ref.reference(orc, case)
        T = max(col["length"] for col in exp.values())
        acts = ref.assemble(exp, case["N"], T, 4 * case["Q"])["actions"]
        ref._CACHE[key] = tracked_replay(orc, ref.env_kw_of(case), acts, case["episodes"])
    return ref._CACHE[key]


# best-of-K search: (M starts, K clones, N envs); Q = 8, max_actions 6, hid 128, two hidden layers
SEARCH_SHAPES = [(3, 1, 3), (5, 13, 70), (7, 64, 130), (2, 65, 130), (1, 257, 300)]
TIED_SHAPE = (5, 13, 70)     # a shape whose replay holds a start with two clones tied for the best gap (the host test asserts it)
SEARCH_CASE = dict(Q=8, M=6, hid=128, L=2, pseed=3, goff=0)
START_OFFSET = 5000          # the starts are the reset states (episode counter 1) of the envs of these global ids on


def search_env_kw(N):
    return dict(num_envs=N, Q=SEARCH_CASE["Q"], max_actions=SEARCH_CASE["M"], seed=ref.SEED, global_offset=SEARCH_CASE["goff"])


def search_starts(orc, M):
    e = orc.Env(Q=SEARCH_CASE["Q"], max_actions=SEARCH_CASE["M"], N=M, seed=ref.SEED, global_offset=START_OFFSET)
    e.episode[:] = 1
    e.reset()
    return e.score.copy(), e.degree.copy(), e.active.copy().astype(np.uint32)


def search_reference(orc, shape):
    """search_replay of one shape on a fresh env (ticks 0), once per process and never modified."""
    key = ("search", shape)
    if key not in ref._CACHE:
        M, K, N = shape
        params = orc.glorot_params(ref.F, SEARCH_CASE["hid"], SEARCH_CASE["L"], seed=SEARCH_CASE["pseed"])
        ref._CACHE[key] = search_replay(orc, search_env_kw(N), params, SEARCH_CASE["hid"], SEARCH_CASE["L"],
                                        search_starts(orc, M), K)
    return ref._CACHE[key]


def tied_starts(rec):
    """Starts whose best gap is held by more than one clone: the lowest-clone rule decides them."""
    return [s for s in range(rec["clone_gaps"].shape[0]) if (rec["clone_gaps"][s] == rec["clone_gaps"][s].min()).sum() > 1]
