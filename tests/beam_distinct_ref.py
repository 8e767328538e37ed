"""Host reference of the distinct beam (beam_search_states_distinct_).  It takes the candidate
order, the shape table, the starts and the oracle's probabilities from tests/beam_ref.py, which stays as it is; the env is the
CPU oracle's, never the device's.

The rule.  Everything of beam_ref's rule holds but its steps 3 and 4, which become one walk.  Step t of an unfinished start:

  identity   of a state: the bytes of score[V], degree[V] and the active word (steps is equal among the slots of a start;
             done, reward and tick are no part of it);
  seen set   empty in mode "children"; in mode "parents" the states of the slots live in front of the step;
  walk       the candidates in beam_ref's order, at most B = 256 * rounds of them.  Examining (k, a) forms the child: slot k's
             state in front of the step after step_one(a), a no-op included.  A child whose state is in the seen set is
             rejected; otherwise it becomes slot j = the number accepted so far (parent k, action a, weight (m', e')) and its
             state joins the seen set.  The walk stops at K accepted, at the end of the candidates or at B examined; slots
             n .. K-1 are dead.  A survivor keeps its own weight;
  fold       as beam_ref's, over the n accepted slots;
  finish     as beam_ref's, and also when n == 0: the result stands as it is.

Logs: parents, actions, mant, exp per accepted slot as in beam_ref; rank [T, K] (the 0-based position of the slot's candidate
in the step's order; -1 for a dead slot or a step that did not run) and examined [T] (the last accepted rank + 1 if the walk
stopped at K, otherwise min(#candidates, B); -1 for a step that did not run).

Arrays are 0-based with -1 as padding, as the C ABI returns them."""
import numpy as np

import beam_ref as bref
import episodes_ref as ref
import path_ref as pref
import search_ref as sref
from beam_ref import SHAPES, candidates, env_kw, oracle_probs, starts  # noqa: F401  (the tests reach them through this module)

WINDOW = 256                     # candidates per round: k_beam_children's one thread per window entry
MODES = ("children", "parents")
# what the two test files replay: (shape, mode, rounds).  GPU_CASES is the issue's list
GPU_CASES = (("q8-k3", "children", 1), ("q8-k3", "parents", 1), ("q8-k8", "parents", 4), ("q8-k64", "parents", 1),
             ("q8-k64", "parents", 2), ("q8-k130", "parents", 2), ("q8-k130", "parents", 4), ("q32-k5", "children", 4),
             ("q32-k256", "parents", 2), ("ties", "parents", 4))


def identity(score, degree, active):
    return np.asarray(score, np.int8).tobytes() + np.asarray(degree, np.int8).tobytes() + int(active).to_bytes(4, "little")


def distinct_one(orc, env_kw, start, K, probs_of, mode, rounds=4):
    """The rule on a K-env oracle env (slot j = env j) plus a one-env work env on which every examined child is formed.
    Returns beam_ref.beam_one's record plus rank, examined, and per step: ncand, n, examined, cut (n < K with candidates left:
    the budget ended the walk), walk = [(rank, k, a, slot or None, equalled)] for every examined candidate, equalled being
    None for an accepted one, ("parent", k') or ("child", slot') for a rejected one; child_ids (identity of every examined
    child, in walk order) and parent_ids (of the live slots in front of the step)."""
    assert mode in MODES and 1 <= rounds <= 16
    T, B = env_kw["max_actions"], WINDOW * rounds
    e, w = ref._env(orc, env_kw, K), ref._env(orc, env_kw, 1)
    for k in range(K):
        e.score[k], e.degree[k], e.active[k] = start[0], start[1], start[2]
        e.steps[k], e.done[k], e.reward[k], e.tick[k] = 0, 0, 0.0, 0
    gap0 = sref.score_gap(np.asarray(start[0]), int(start[2]))[1]
    res = dict(best_state=np.concatenate([start[0], start[1]]).astype(np.int8), best_active=int(start[2]), best_gap=gap0,
               best_step=0, best_beam=0, best_mant=0.5, best_exp=1, initial_gap=gap0)
    live, weights = [0], {0: (0.5, 1)}
    parents, actions = np.full((T, K), -1, np.int16), np.full((T, K), -1, np.int16)
    mant, exp = np.zeros((T, K), np.float64), np.zeros((T, K), np.int32)
    rank, examined = np.full((T, K), -1, np.int32), np.full(T, -1, np.int32)
    steps = []
    for t in range(T):
        obs = e.observe_all()[live]
        act = np.asarray(e.active).astype(np.uint32)[live].copy()
        p = np.asarray(probs_of(obs, act), np.float32)
        assert p.shape == (len(live), e.A)
        cand = candidates(live, weights, p)
        snap = (e.score.copy(), e.degree.copy(), np.asarray(e.active).copy(), np.asarray(e.steps).copy())
        parent_ids = [identity(snap[0][k], snap[1][k], snap[2][k]) for k in live]
        seen = {pid: ("parent", k) for k, pid in reversed(list(zip(live, parent_ids)))} if mode == "parents" else {}
        accepted, walk, child_ids = [], [], []               # accepted: (candidate, rank, score, degree, active, steps)
        looked = 0
        for r, c in enumerate(cand[:B]):
            if len(accepted) == K:
                break
            looked = r + 1
            k, a = c[3], c[4]
            w.score[0], w.degree[0], w.active[0], w.steps[0] = snap[0][k], snap[1][k], snap[2][k], snap[3][k]
            w.done[0], w.reward[0], w.tick[0] = 0, 0.0, 0
            w.step_one(0, a)
            assert np.all(w.err == 0)
            sc, dg, ac = sref.state_of(w, 0)
            cid = identity(sc, dg, ac)
            child_ids.append(cid)
            if cid in seen:
                walk.append((r, k, a, None, seen[cid]))
                continue
            seen[cid] = ("child", len(accepted))
            walk.append((r, k, a, len(accepted), None))
            accepted.append((c, r, sc, dg, ac, int(w.steps[0])))
        n = len(accepted)
        gaps = []
        for j, (c, r, sc, dg, ac, st) in enumerate(accepted):
            e.score[j], e.degree[j], e.active[j], e.steps[j] = sc, dg, ac, st
            parents[t, j], actions[t, j], mant[t, j], exp[t, j], rank[t, j] = c[3], c[4], c[5], c[6], r
            gaps.append(sref.score_gap(sc, ac)[1])
        examined[t] = looked
        live = list(range(n))
        weights = {j: (a[0][5], a[0][6]) for j, a in enumerate(accepted)}
        steps.append(dict(t=t, ncand=len(cand), n=n, examined=looked, cut=n < K and looked < len(cand), walk=walk,
                          child_ids=child_ids, parent_ids=parent_ids,
                          chosen=[(a[0][3], a[0][4], a[0][5], a[0][6]) for a in accepted], states=obs, active=act, probs=p,
                          gaps=gaps))
        if gaps:
            g, j = min((g, j) for j, g in enumerate(gaps))
            if g < res["best_gap"]:
                res.update(best_state=np.concatenate([accepted[j][2], accepted[j][3]]).astype(np.int8),
                           best_active=accepted[j][4], best_gap=g, best_step=t + 1, best_beam=j, best_mant=weights[j][0],
                           best_exp=weights[j][1])
        if res["best_gap"] == 0 or t + 1 == T or n == 0:
            break
    path, slot = [], res["best_beam"]
    for t in range(res["best_step"] - 1, -1, -1):
        assert parents[t, slot] >= 0
        path.append(int(actions[t, slot]))
        slot = int(parents[t, slot])
    res.update(path=path[::-1], parents=parents, actions=actions, mant=mant, exp=exp, rank=rank, examined=examined, steps=steps)
    return res


def distinct_replay(orc, env_kw, starts, K, probs_of, mode, rounds=4):
    """Every start of a call, as beam_ref.beam_replay returns it, plus rank [M, T, K] and examined [M, T]."""
    N, T = env_kw["num_envs"], env_kw["max_actions"]
    M = starts[2].shape[0]
    S = N // K
    recs = [distinct_one(orc, env_kw, (starts[0][s], starts[1][s], int(starts[2][s])), K, probs_of, mode, rounds)
            for s in range(M)]
    out = dict(best_state=np.stack([r["best_state"] for r in recs]).astype(np.int8),
               best_active=np.array([r["best_active"] for r in recs], np.uint32),
               best_mant=np.array([r["best_mant"] for r in recs], np.float64))
    for k in ("best_gap", "best_step", "best_beam", "initial_gap", "best_exp"):
        out[k] = np.array([r[k] for r in recs], np.int32)
    for k in ("parents", "actions", "mant", "exp", "rank", "examined"):
        out[k] = np.stack([r[k] for r in recs])
    played = np.zeros(N, bool)
    played[:min(S, M) * K] = True
    out.update(log_prob=bref.log_prob(out["best_mant"], out["best_exp"]), path=pref.padded([r["path"] for r in recs], T),
               steps=[r["steps"] for r in recs], played=played)
    return out


def host_reference(orc, name, mode, rounds=4):
    """distinct_replay with the oracle's probabilities, once per process and never modified; mode None: the plain beam."""
    key = ("beam-distinct-host", name, mode, rounds if mode else 0)
    if key not in ref._CACHE:
        if mode is None:
            ref._CACHE[key] = bref.beam_replay(orc, env_kw(name), starts(orc, name), SHAPES[name]["K"], oracle_probs(orc, name))
        else:
            ref._CACHE[key] = distinct_replay(orc, env_kw(name), starts(orc, name), SHAPES[name]["K"],
                                              _cached_probs(orc, name), mode, rounds)
    return ref._CACHE[key]


def _cached_probs(orc, name):
    """oracle_probs with a per-process memo on the state's bytes: the modes and budgets of a shape revisit the same states."""
    memo = ref._CACHE.setdefault(("beam-distinct-probs", name), {})
    inner = oracle_probs(orc, name)

    def probs_of(states, active):
        keys = [states[i].tobytes() + int(active[i]).to_bytes(4, "little") for i in range(states.shape[0])]
        miss = [i for i, k in enumerate(keys) if k not in memo]
        if miss:
            rows = inner(states[miss], active[miss])
            for i, row in zip(miss, rows):
                memo[keys[i]] = row
        return np.stack([memo[k] for k in keys]).astype(np.float32)
    return probs_of


def result(rec, s):
    return int(rec["best_gap"][s]), int(rec["best_step"][s])


def windows_used(step):
    """How many windows of 256 candidates the walk of a step read."""
    return -(-step["examined"] // WINDOW)
