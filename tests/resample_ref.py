"""Host reference of the resampling search (search_resample_states_).  Everything here comes from the CPU
oracle (oracle/oracle.py), numpy, tests/episodes_ref.py and tests/search_ref.py, never from the device.

The schedule is search_ref.search_replay's: rounds of S = N // K starts, env n < S_r * K plays start base + n // K as clone
n % K from the tick it holds, the other envs idle.  All clones of a round advance one loop step at a time.  The oracle's own
rollout resets an env when it terminates, so it only chooses the actions: a scratch env takes a copy of every state and
tick, orc.collect_rollouts_tn plays ONE step on it (forward in "dev" mode, Philox sampling keyed on (global id, tick)) and
the actions are applied with step_one to the env that is kept -- what search_ref.play_from does, batched over the round.

Behind loop step t (1-based, counted from the round's load) with t % R == 0 and t < max_actions every start of the round
runs a resample event -- fold, rank, copy -- and behind the round's last step one more fold (fold_into / resample_event
below are the rule).  The loop of a round ends once every clone is terminal; an event that would come later finds no live
clone: its fold changes nothing the last fold does not do, its log row stays -2.

resample_replay keeps, next to the result, a second result made WITHOUT the event folds (the last fold alone) and a list of
what every event saw: tests/test_resample_host.py reads the situations the device test depends on off that list.

The shape table of tests/test_resample_host.py and tests/test_gpu_resample.py lives at the end of the file."""
import numpy as np

import episodes_ref as ref
import search_ref as sref

RECORD = ("best_state", "best_active", "best_gap", "best_step", "initial_gap")


# ---------------------------------------------------------------- the rule
def fold_into(result, recs):
    """Fold: the clone with the lowest (record best_gap, clone) of ALL K; its record becomes the start's result on the first
    fold (result is None), afterwards only on a strictly lower best_gap.  Returns the result (a dict with best_clone)."""
    c = min(range(len(recs)), key=lambda i: (recs[i]["best_gap"], i))
    if result is None or recs[c]["best_gap"] < result["best_gap"]:
        result = dict(recs[c], best_clone=c)
    return result


def rank_live(cur_gap, done, m0):
    """Rank: the live clones (done == 0) ascending by (cur_gap, clone).  Returns (order, m, donor_of): order[rho] is the
    clone of rank rho, m = min(m0, live), donor_of {receiver clone: donor clone} for the ranks rho >= m, whose donor is the
    clone of rank (rho - m) % m."""
    order = sorted((c for c in range(len(done)) if not done[c]), key=lambda c: (cur_gap[c], c))
    m = min(m0, len(order))
    return order, m, {order[rho]: order[(rho - m) % m] for rho in range(m, len(order))}


class Round:
    """The clones of one round on the oracle env: envs 0 .. busy - 1 of the call's env, loaded with their starts."""

    def __init__(self, orc, env_kw, params, hid, L, starts, base, Sr, K, tick):
        self.orc, self.params, self.hid, self.L, self.K, self.Sr = orc, params, hid, L, K, Sr
        busy = Sr * K
        self.env = ref._env(orc, env_kw, busy)
        self.scratch = ref._env(orc, env_kw, busy)
        e = self.env
        for n in range(busy):
            s = base + n // K
            e.score[n], e.degree[n], e.active[n] = starts[0][s], starts[1][s], starts[2][s]
        e.steps[:], e.done[:], e.reward[:] = 0, 0, 0.0
        e.tick[:] = tick[:busy]
        self.recs = []
        for n in range(busy):
            sc, dg, act = sref.state_of(e, n)
            gap = sref.score_gap(sc, act)[1]
            self.recs.append(dict(best_state=np.concatenate([sc, dg]), best_active=act, best_gap=gap, best_step=0,
                                  initial_gap=gap))
        self.t = 0

    def live(self):
        return np.flatnonzero(self.env.done == 0)

    def step(self):
        """One loop step: every live clone samples from the state and tick it holds and steps; its record takes the new state
        on a strictly lower gap."""
        e, x = self.env, self.scratch
        x.score[:], x.degree[:], x.active[:], x.tick[:] = e.score, e.degree, e.active, e.tick
        x.steps[:], x.done[:], x.reward[:] = 0, 0, 0.0
        acts = self.orc.collect_rollouts_tn(x, self.params, self.hid, 1, mode_dev=True, n_hidden=self.L)["actions"][0]
        self.t += 1
        for n in (int(i) for i in self.live()):
            e.step_one(n, int(acts[n]))
            sc, dg, act = sref.state_of(e, n)
            gap = sref.score_gap(sc, act)[1]
            if gap < self.recs[n]["best_gap"]:
                self.recs[n].update(best_state=np.concatenate([sc, dg]), best_active=act, best_gap=gap, best_step=self.t)
        assert np.all(e.err == 0)

    def cur_gaps(self, s):
        e = self.env
        return [sref.score_gap(e.score[n], int(e.active[n]))[1] for n in range(s * self.K, (s + 1) * self.K)]

    def copy(self, s, receiver, donor):
        """Copy donor -> receiver: score, degree, active, steps, reward and the whole record (every clone of a round has
        played t steps, so its step count is equal anyway); tick, episode, done stay the receiver's own."""
        e, r, d = self.env, s * self.K + receiver, s * self.K + donor
        e.score[r], e.degree[r], e.active[r], e.steps[r], e.reward[r] = e.score[d], e.degree[d], e.active[d], e.steps[d], e.reward[d]
        self.recs[r] = dict(self.recs[d])


def resample_replay(orc, env_kw, params, hid, L, starts, K, R, m0, tick0=None):
    """The resampling search.  starts = (score [M, V], degree [M, V], active [M]).  Returns the arrays
    search_resample_states_ returns (donors and clone_gaps included) plus tick / done [N] as the call leaves them (done of an
    env that never played is None here: whatever it was), `nofold`: the result arrays of the same play with the last fold
    alone, and `events`: one dict per (start, event) that ran."""
    N, T = env_kw["num_envs"], env_kw["max_actions"]
    M = starts[2].shape[0]
    S, E = N // K, (T - 1) // R
    tick = np.zeros(N, np.int64) if tick0 is None else np.asarray(tick0, np.int64).copy()
    played = np.zeros(N, bool)
    donors = np.full((M, E, K), -2, np.int32)
    clone_gaps = np.zeros((M, K), np.int32)
    results, plain, events = [None] * M, [None] * M, []
    for base in range(0, M, S):
        Sr = min(S, M - base)
        rd = Round(orc, env_kw, params, hid, L, starts, base, Sr, K, tick)
        played[:Sr * K] = True
        while rd.t < T and rd.live().size:
            rd.step()
            if rd.t % R == 0 and rd.t < T:
                ev = rd.t // R - 1
                for s in range(Sr):
                    recs = rd.recs[s * K:(s + 1) * K]
                    results[base + s] = fold_into(results[base + s], recs)
                    done = [int(x) for x in rd.env.done[s * K:(s + 1) * K]]
                    cur = rd.cur_gaps(s)
                    order, m, donor_of = rank_live(cur, done, m0)
                    events.append(dict(start=base + s, event=ev, t=rd.t, cur_gap=cur, done=done, order=order, m=m,
                                       donor_of=dict(donor_of), record_gap=[r["best_gap"] for r in recs]))
                    for c in range(K):
                        donors[base + s, ev, c] = -2 if done[c] else donor_of.get(c, -1)
                    for c, d in donor_of.items():
                        rd.copy(s, c, d)
        assert not rd.live().size
        for s in range(Sr):
            recs = rd.recs[s * K:(s + 1) * K]
            results[base + s] = fold_into(results[base + s], recs)
            plain[base + s] = fold_into(None, recs)
            clone_gaps[base + s] = [r["best_gap"] for r in recs]
        tick[:Sr * K] = rd.env.tick

    def arrays(res):
        out = dict(best_state=np.stack([r["best_state"] for r in res]).astype(np.int8),
                   best_active=np.array([r["best_active"] for r in res], np.uint32))
        for k in ("best_gap", "best_step", "initial_gap", "best_clone"):
            out[k] = np.array([r[k] for r in res], np.int32)
        return out
    out = arrays(results)
    out.update(donors=donors, clone_gaps=clone_gaps, tick=tick, played=played, nofold=arrays(plain), events=events)
    return out


# ---------------------------------------------------------------- what the events of a replay contain
def cut_between_equals(ev):
    """The survivor cut falls between two live clones of equal cur_gap: the clone index decides who survives."""
    o, m = ev["order"], ev["m"]
    return len(o) > m >= 1 and ev["cur_gap"][o[m - 1]] == ev["cur_gap"][o[m]]


def terminal_among_live(ev):
    """A terminal clone among the K of a start that still has live ones."""
    return 0 < len(ev["order"]) < len(ev["done"])


def discarded_record_beats_survivors(ev):
    """A receiver whose own record -- overwritten by the copy -- is strictly better than every survivor's record: only the
    fold keeps it."""
    o, m = ev["order"], ev["m"]
    if not ev["donor_of"]:
        return False
    best_kept = min(ev["record_gap"][c] for c in o[:m])
    return any(ev["record_gap"][c] < best_kept for c in ev["donor_of"])


# ---------------------------------------------------------------- shapes
# (starts, K clones, N envs, max_actions, R interval, survivors); Q = 8, hid 128, two hidden layers, policy seed 3, env seed
# 13, the starts of search_ref.search_starts, fresh ticks
SHAPES = {
    "A": (4, 12, 48, 24, 2, 3),      # the fold decides a result
    "B": (6, 8, 48, 20, 1, 2),       # terminal clones at events, a start solved to gap 0
    "C": (5, 13, 70, 8, 2, 3),       # K not a power of two, five idle envs
    "D": (7, 8, 20, 12, 2, 2),       # four rounds, the last one ragged
    "E": (1, 257, 300, 6, 2, 32),    # K beyond one pass of the workgroup
    "F": (3, 1, 3, 6, 2, 1),         # K = 1
    "G": (4, 16, 64, 10, 3, 16),     # survivors = K: nothing is copied
    "H": (5, 13, 70, 8, 8, 3),       # shape C with R = max_actions: no event, the best-of-K search
}
CASE = dict(Q=8, hid=128, L=2, pseed=3, goff=0)


def env_kw(shape):
    return dict(num_envs=shape[2], Q=CASE["Q"], max_actions=shape[3], seed=ref.SEED, global_offset=CASE["goff"])


def policy_params(orc):
    return orc.glorot_params(ref.F, CASE["hid"], CASE["L"], seed=CASE["pseed"])


def reference(orc, name):
    """resample_replay of one shape on a fresh env (ticks 0), once per process and never modified."""
    key = ("resample", name)
    if key not in ref._CACHE:
        M, K, N, T, R, m0 = SHAPES[name]
        ref._CACHE[key] = resample_replay(orc, env_kw(SHAPES[name]), policy_params(orc), CASE["hid"], CASE["L"],
                                          sref.search_starts(orc, M), K, R, m0)
    return ref._CACHE[key]
