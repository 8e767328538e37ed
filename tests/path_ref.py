"""Host reference of the action paths: what best_states_(actions=True), search_best_states_(path=True),
search_resample_states_(path=True) and apply_paths_ must return.  Everything here comes from the CPU oracle (oracle/oracle.py),
numpy, tests/episodes_ref.py, tests/search_ref.py and tests/resample_ref.py, never from the device; none of those is changed.

The rule.  Every clone keeps the list of the actions it has played: its history.  A record update (a strictly lower gap)
stores the history as it is then -- best_step entries -- as the record's path.  A copy gives the receiver the donor's
history with its record.  A fold that takes a winner's record takes its path.  So a result's path has best_step entries, and
replaying it from the start with step_one must give best_state and best_active exactly: apply_path below is that replay.

Paths here are 0-based and padded with -1 behind their end, as the C ABI returns them; one_based() is what Python returns.

  PathRound / resample_paths   the resampling replay of resample_ref with the per-clone history;
  search_paths                 the best-of-K replay of search_ref returning the winner's action prefix;
  trajectory_actions           the actions of the trajectories search_ref.oracle_record replays, one row per trajectory;
  apply_path                   a plain replay on the oracle env."""
import numpy as np

import episodes_ref as ref
import resample_ref as rref
import search_ref as sref


def padded(paths, width):
    """Lists of 0-based actions -> int16 [n, width], -1 behind each path's end."""
    out = np.full((len(paths), width), -1, np.int16)
    for i, p in enumerate(paths):
        out[i, :len(p)] = p
    return out


def one_based(rows):
    """The encoding Python speaks: the reference's 1-based action indices, 0 as padding."""
    return (np.asarray(rows) + 1).astype(np.int16)


# ---------------------------------------------------------------- a plain replay
def apply_path(orc, env_kw, start, path):
    """step_one for every entry of `path` (0-based; an entry < 0 ends it) on a one-env oracle env loaded with start = (score
    [V], degree [V], active) as reset! leaves an env, until the path ends or the state is terminal.  Returns dict(state [2V],
    active, gap, applied, trace)."""
    e = ref._env(orc, env_kw, 1)
    e.score[0], e.degree[0], e.active[0] = start[0], start[1], start[2]
    e.steps[0], e.done[0], e.reward[0], e.tick[0] = 0, 0, 0.0, 0
    init = sref.score_gap(*sref.state_of(e, 0)[::2])[0]
    trace = []
    for a in path:
        if a < 0 or e.done[0]:
            break
        e.step_one(0, int(a))
        sc, dg, act = sref.state_of(e, 0)
        trace.append(init - sref.score_gap(sc, act)[0])
    sc, dg, act = sref.state_of(e, 0)
    assert int(e.err[0]) == 0
    return dict(state=np.concatenate([sc, dg]).astype(np.int8), active=act, gap=sref.score_gap(sc, act)[1], applied=len(trace),
                trace=trace)


# ---------------------------------------------------------------- the resampling search with histories
class PathRound(rref.Round):
    """resample_ref.Round whose clones keep their action history: step appends the action (and a record update stores the
    history so far as the record's path), copy copies the history.  copies[n]: how many copies the lineage clone n holds has
    crossed."""

    def __init__(self, *args):
        super().__init__(*args)
        busy = self.Sr * self.K
        self.hist = [[] for _ in range(busy)]
        self.copies = [0] * busy
        for r in self.recs:
            r.update(path=())

    def step(self):
        e, x = self.env, self.scratch
        x.score[:], x.degree[:], x.active[:], x.tick[:] = e.score, e.degree, e.active, e.tick
        x.steps[:], x.done[:], x.reward[:] = 0, 0, 0.0
        acts = self.orc.collect_rollouts_tn(x, self.params, self.hid, 1, mode_dev=True, n_hidden=self.L)["actions"][0]
        self.t += 1
        for n in (int(i) for i in self.live()):
            a = int(acts[n])
            e.step_one(n, a)
            self.hist[n].append(a)
            sc, dg, act = sref.state_of(e, n)
            gap = sref.score_gap(sc, act)[1]
            if gap < self.recs[n]["best_gap"]:
                self.recs[n].update(best_state=np.concatenate([sc, dg]), best_active=act, best_gap=gap, best_step=self.t,
                                    path=tuple(self.hist[n]))
        assert np.all(e.err == 0)

    def copy(self, s, receiver, donor):
        super().copy(s, receiver, donor)                      # state and record (the path with it)
        r, d = s * self.K + receiver, s * self.K + donor
        self.hist[r] = list(self.hist[d])
        self.copies[r] = self.copies[d] + 1


def resample_paths(orc, env_kw, params, hid, L, starts, K, R, m0):
    """resample_ref.resample_replay's loop on PathRound, fresh ticks.  Returns its result arrays (best_state, best_active,
    best_gap, best_step, initial_gap, best_clone, donors, clone_gaps, tick) plus
      path         int16 [M, max_actions], 0-based, -1 behind best_step entries;
      fold_event   [M] the event whose fold took the result, -1: the last fold;
      copies       [M] the copies the winner's lineage had crossed when that fold took it;
      final_hist   per start the K histories the clones hold at the end."""
    N, T = env_kw["num_envs"], env_kw["max_actions"]
    M = starts[2].shape[0]
    S, E = N // K, (T - 1) // R
    tick = np.zeros(N, np.int64)
    donors = np.full((M, E, K), -2, np.int32)
    clone_gaps = np.zeros((M, K), np.int32)
    results, final_hist = [None] * M, [None] * M

    def fold(rd, s, base, ev):
        old = results[base + s]
        new = rref.fold_into(old, rd.recs[s * K:(s + 1) * K])
        if new is not old:
            new.update(fold_event=ev, copies=rd.copies[s * K + new["best_clone"]])
        results[base + s] = new

    for base in range(0, M, S):
        Sr = min(S, M - base)
        rd = PathRound(orc, env_kw, params, hid, L, starts, base, Sr, K, tick)
        while rd.t < T and rd.live().size:
            rd.step()
            if rd.t % R == 0 and rd.t < T:
                ev = rd.t // R - 1
                for s in range(Sr):
                    fold(rd, s, base, ev)
                    done = [int(x) for x in rd.env.done[s * K:(s + 1) * K]]
                    order, m, donor_of = rref.rank_live(rd.cur_gaps(s), done, m0)
                    for c in range(K):
                        donors[base + s, ev, c] = -2 if done[c] else donor_of.get(c, -1)
                    for c, d in donor_of.items():
                        rd.copy(s, c, d)
        assert not rd.live().size
        for s in range(Sr):
            fold(rd, s, base, -1)
            clone_gaps[base + s] = [r["best_gap"] for r in rd.recs[s * K:(s + 1) * K]]
            final_hist[base + s] = [tuple(h) for h in rd.hist[s * K:(s + 1) * K]]
        tick[:Sr * K] = rd.env.tick
    out = dict(best_state=np.stack([r["best_state"] for r in results]).astype(np.int8),
               best_active=np.array([r["best_active"] for r in results], np.uint32))
    for k in ("best_gap", "best_step", "initial_gap", "best_clone", "fold_event", "copies"):
        out[k] = np.array([r[k] for r in results], np.int32)
    out.update(path=padded([r["path"] for r in results], T), donors=donors, clone_gaps=clone_gaps, tick=tick,
               final_hist=final_hist)
    return out


def resample_reference(orc, name):
    """resample_paths of one shape of resample_ref.SHAPES, once per process and never modified."""
    key = ("resample-paths", name)
    if key not in ref._CACHE:
        M, K, N, T, R, m0 = rref.SHAPES[name]
        ref._CACHE[key] = resample_paths(orc, rref.env_kw(rref.SHAPES[name]), rref.policy_params(orc), rref.CASE["hid"],
                                         rref.CASE["L"], sref.search_starts(orc, M), K, R, m0)
    return ref._CACHE[key]


# ---------------------------------------------------------------- the best-of-K search with the winner's prefix
def play_from_actions(orc, env_kw, n, params, hid, L, start, tick0):
    """search_ref.play_from, returning (record, the trajectory's 0-based actions)."""
    M = env_kw["max_actions"]

    def load():
        e = ref._env(orc, env_kw, 1, n)
        e.score[0], e.degree[0], e.active[0] = start[0], start[1], start[2]
        e.steps[0], e.done[0], e.reward[0], e.tick[0] = 0, 0, 0.0, tick0
        return e
    e = load()
    r = orc.collect_rollouts_tn(e, params, hid, M, mode_dev=True, n_hidden=L)
    length = int(np.flatnonzero(r["done"][:, 0])[0]) + 1
    acts = [int(a) for a in r["actions"][:length, 0]]
    e = load()
    tr = sref.Traj(e, 0)
    for a in acts:
        e.step_one(0, a)
        tr.after(e, 0, a)
    assert e.done[0] and int(e.err[0]) == 0
    return tr.record(), acts


def search_paths(orc, env_kw, params, hid, L, starts, K):
    """search_ref.search_replay's schedule, fresh ticks.  Returns best_state, best_active, best_gap, best_step, initial_gap,
    best_clone and path int16 [M, max_actions]: the winner's first best_step actions, -1 behind them."""
    N, T = env_kw["num_envs"], env_kw["max_actions"]
    M = starts[2].shape[0]
    S = N // K
    tick = np.zeros(N, np.int64)
    win, paths, best_clone = [], [], np.zeros(M, np.int32)
    for base in range(0, M, S):
        for s in range(base, min(base + S, M)):
            recs = []
            for c in range(K):
                n = (s - base) * K + c
                recs.append(play_from_actions(orc, env_kw, n, params, hid, L, (starts[0][s], starts[1][s], int(starts[2][s])),
                                              int(tick[n])))
                tick[n] += recs[-1][0]["length"]
            best_clone[s] = int(np.argmin([r["best_gap"] for r, _ in recs]))
            rec, acts = recs[best_clone[s]]
            win.append(rec)
            paths.append(acts[:rec["best_step"]])
    out = sref.stack(win, T)
    out.update(best_clone=best_clone, path=padded(paths, T))
    return out


def search_reference(orc, shape):
    """search_paths of one shape of search_ref.SEARCH_SHAPES, once per process and never modified."""
    key = ("search-paths", shape)
    if key not in ref._CACHE:
        M, K, N = shape
        c = sref.SEARCH_CASE
        params = orc.glorot_params(ref.F, c["hid"], c["L"], seed=c["pseed"])
        ref._CACHE[key] = search_paths(orc, sref.search_env_kw(N), params, c["hid"], c["L"], sref.search_starts(orc, M), K)
    return ref._CACHE[key]


# ---------------------------------------------------------------- the trajectories of best_states_
def trajectory_actions(orc, case):
    """The oracle's own actions of the trajectories search_ref.oracle_record replays (ref.reference, every column: N <= 70),
    one row per trajectory in env-major order: int16 [num_traj, max_actions], -1 behind each trajectory's end."""
    assert case["N"] <= 70
    exp = ref.reference(orc, case)
    rows = []
    for n in range(case["N"]):
        col = exp[n]
        ends = np.flatnonzero(col["done"]) + 1
        first = 0
        for end in (int(x) for x in ends):
            rows.append([int(a) for a in col["actions"][first:end]])
            first = end
        assert first == col["length"]
    assert len(rows) == case["episodes"]
    return padded(rows, case["M"])


# ---------------------------------------------------------------- apply_paths_: ragged paths on two env sizes
APPLY_CASES = {"q8": dict(Q=8, max_actions=6, N=9), "q32": dict(Q=32, max_actions=5, N=7)}
APPLY_STRIDE = 8                 # above both max_actions: a full row ends by truncation with entries to spare


def apply_env_kw(name):
    c = APPLY_CASES[name]
    return dict(num_envs=c["N"], Q=c["Q"], max_actions=c["max_actions"], seed=ref.SEED, global_offset=300)


def apply_inputs(orc, name):
    """Starts (the reset states of the case's envs) and ragged 0-based paths [N, APPLY_STRIDE] of moves on active quads: row
    0 is empty, row 1 is full (no padding, stride == its length: it ends by truncation at max_actions with entries behind the
    terminal state), row 2 has exactly max_actions entries, the others lengths 1 .. 7 and -1 behind them."""
    kw = apply_env_kw(name)
    e = ref._env(orc, kw)
    e.episode[:] = 1
    e.reset()
    starts = (e.score.copy(), e.degree.copy(), e.active.copy().astype(np.uint32))
    rng = np.random.default_rng(5)
    N, Q = kw["num_envs"], kw["Q"]
    paths = np.full((N, APPLY_STRIDE), -1, np.int16)
    for n in range(N):
        length = (0, APPLY_STRIDE, kw["max_actions"])[n] if n < 3 else 1 + (n * 3) % (APPLY_STRIDE - 1)
        # flips (types 0 and 1) keep the set of active quads, so every entry stays a move on an active quad
        quads = np.flatnonzero([(int(starts[2][n]) >> q) & 1 for q in range(Q)])
        for i in range(length):
            paths[n, i] = 16 * int(rng.choice(quads)) + 4 * int(rng.integers(4)) + int(rng.integers(2))
    return kw, starts, paths
