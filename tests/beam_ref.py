"""Host reference of beam search (beam_search_states_).  Everything here comes from the CPU oracle
(oracle/oracle.py), numpy, tests/episodes_ref.py, tests/search_ref.py and tests/path_ref.py, never from the device; none of those
is changed.

The rule.  A call takes M starts and a beam width K, 1 <= K <= N.  S = N // K starts run per round; start s of a round owns
resident envs s*K .. s*K + K - 1, its slots.  Every slot carries a live flag and a weight (m, e), m an fp64 in [0.5, 1) and e an
int, standing for the path probability m * 2^e.  At load all K envs hold the start's state, slot 0 is live with (0.5, 1) and slots
1 .. K-1 are dead.  Step t = 0 .. max_actions - 1 of a start that has not finished:

  1. probabilities   p[slot][a], fp32, of the states the slots hold: they come from outside (`probs_of`), as value_resample_ref
                     takes its values -- the device test feeds the device's own forward and then checks it against the oracle;
  2. candidates      every (k, a) with slot k live and p[k][a] > 0; x = m_k * float64(p[k][a]), one IEEE fp64 multiply;
                     (m', d) = frexp(x), e' = e_k + d.  p >= 2^-149 and m_k >= 0.5, so x is normal, frexp is exact and nothing
                     else rounds;
  3. select          candidates ordered by e' descending, then m' descending, then k*A + a ascending (a Python tuple sort of
                     (-e', -m', k*A + a)); the first n = min(K, #candidates): rank j becomes slot j with parent k, action a and
                     weight (m', e'); slots n .. K-1 become dead;
  4. expand          slot j takes the state (score, degree, active, steps) its parent held in front of this step, then plays
                     its action with step_one, an action the env counts as a no-op included;
  5. fold            the start's result (gap, state, step, slot) is the load state with step 0 (slot 0, weight (0.5, 1)) until
                     some live slot's gap = current_score - opt_score is STRICTLY below it; then the lowest (gap, slot) of the
                     step, with best_step = t + 1 and best_beam = slot;
  6. finish          the result's gap is 0, or t + 1 == max_actions.

Every step writes (parent, action, m', e') per slot into the start's log [max_actions][K]: -1, -1, 0.0, 0 for a dead slot and
for a step that did not run.  The path to the result is the walk back through the log from (best_step, best_beam).  No reset
runs and no random number is drawn: ticks and episode counters stay; the slots' envs are left terminal; envs at and beyond
S*K of a round are untouched.

Arrays here are 0-based with -1 as padding, as the C ABI returns them; path_ref.one_based() is what Python returns.

The shape table of tests/test_beam_host.py and tests/test_gpu_beam.py lives at the end of the file."""
import math

import numpy as np

import episodes_ref as ref
import path_ref as pref
import search_ref as sref


# ---------------------------------------------------------------- the rule
def child_weight(m, e, p):
    """(m', e') of one candidate: one fp64 multiply and an exact frexp."""
    x = np.float64(m) * np.float64(np.float32(p))
    m2, d = np.frexp(x)
    return float(m2), int(e) + int(d)


def candidates(live, weights, p):
    """The sorted candidate list of one step: tuples (-e', -m', k*A + a, k, a, m', e') over the live slots k and the actions
    with p[k][a] > 0.  live: the live slot numbers; weights: {k: (m, e)}; p: [len(live), A] float32, row i of slot live[i]."""
    A = p.shape[1]
    out = []
    for i, k in enumerate(live):
        m, e = weights[k]
        x = np.float64(m) * p[i].astype(np.float64)              # one multiply per candidate
        m2, d = np.frexp(x)
        for a in np.flatnonzero(p[i] > 0):
            out.append((-(e + int(d[a])), -float(m2[a]), k * A + int(a), k, int(a), float(m2[a]), e + int(d[a])))
    out.sort()
    return out


def log_prob(mant, exp):
    """log of the path probability mant * 2^exp, as beam_search_states_ computes it on the host."""
    return np.log(np.asarray(mant, np.float64)) + np.asarray(exp, np.float64) * np.log(2.0)


# ---------------------------------------------------------------- the replay of one start
def beam_one(orc, env_kw, start, K, probs_of):
    """The rule on a K-env oracle env (slot j = env j).  Returns the start's result and log plus `steps`: one dict per step
    that ran with t, ncand, chosen [(k, a, m', e')] in slot order, index_decided (two candidates with equal (e', m'), at least
    one of them chosen), states / active (what probs_of was asked about: the slots live in front of the step, which are slots
    0 .. len - 1), probs (what it answered), gaps (of the new slots)."""
    T = env_kw["max_actions"]
    e = ref._env(orc, env_kw, K)
    V, A = e.V, e.A
    for k in range(K):
        e.score[k], e.degree[k], e.active[k] = start[0], start[1], start[2]
        e.steps[k], e.done[k], e.reward[k], e.tick[k] = 0, 0, 0.0, 0
    gap0 = sref.score_gap(np.asarray(start[0]), int(start[2]))[1]
    res = dict(best_state=np.concatenate([start[0], start[1]]).astype(np.int8), best_active=int(start[2]), best_gap=gap0,
               best_step=0, best_beam=0, best_mant=0.5, best_exp=1, initial_gap=gap0)
    live, weights = [0], {0: (0.5, 1)}
    parents, actions = np.full((T, K), -1, np.int16), np.full((T, K), -1, np.int16)
    mant, exp = np.zeros((T, K), np.float64), np.zeros((T, K), np.int32)
    steps = []
    for t in range(T):
        obs = e.observe_all()[live]
        act = np.asarray(e.active).astype(np.uint32)[live].copy()
        p = np.asarray(probs_of(obs, act), np.float32)
        assert p.shape == (len(live), A)
        cand = candidates(live, weights, p)
        chosen = cand[:K]
        keys = [(c[0], c[1]) for c in cand]
        index_decided = any(keys[i] == keys[i + 1] for i in range(min(len(chosen), len(cand) - 1)))
        # expand: every parent is read from the copy taken in front of the step
        snap = (e.score.copy(), e.degree.copy(), np.asarray(e.active).copy(), np.asarray(e.steps).copy())
        gaps = []
        for j, (_, _, _, k, a, m2, e2) in enumerate(chosen):
            e.score[j], e.degree[j], e.active[j], e.steps[j] = snap[0][k], snap[1][k], snap[2][k], snap[3][k]
            e.done[j] = 0
            e.step_one(j, a)
            parents[t, j], actions[t, j], mant[t, j], exp[t, j] = k, a, m2, e2
            gaps.append(sref.score_gap(*sref.state_of(e, j)[::2])[1])
        assert np.all(e.err == 0)
        live = list(range(len(chosen)))
        weights = {j: (c[5], c[6]) for j, c in enumerate(chosen)}
        steps.append(dict(t=t, ncand=len(cand),
                          chosen=[(c[3], c[4], c[5], c[6]) for c in chosen], index_decided=index_decided, states=obs, active=act,
                          probs=p, gaps=gaps))
        # fold: the lowest (gap, slot), taken on a strictly lower gap only
        if gaps:
            g, j = min((g, j) for j, g in enumerate(gaps))
            if g < res["best_gap"]:
                sc, dg, ac = sref.state_of(e, j)
                res.update(best_state=np.concatenate([sc, dg]).astype(np.int8), best_active=ac, best_gap=g, best_step=t + 1,
                           best_beam=j, best_mant=weights[j][0], best_exp=weights[j][1])
        if res["best_gap"] == 0 or t + 1 == T:
            break
    # the path: walk the back-pointers from (best_step, best_beam)
    path, slot = [], res["best_beam"]
    for t in range(res["best_step"] - 1, -1, -1):
        assert parents[t, slot] >= 0
        path.append(int(actions[t, slot]))
        slot = int(parents[t, slot])
    res.update(path=path[::-1], parents=parents, actions=actions, mant=mant, exp=exp, steps=steps)
    return res


def beam_replay(orc, env_kw, starts, K, probs_of):
    """Every start of a call (a start's search depends on nothing but the start; the rounds decide which resident envs play).
    starts = (score [M, V], degree [M, V], active [M]).  Returns the arrays beam_search_states_ returns, 0-based: best_state,
    best_active, best_gap, best_step, best_beam, initial_gap, best_mant, best_exp, log_prob, path [M, T] int16, parents / actions
    [M, T, K] int16, mant [M, T, K] float64, exp [M, T, K] int32; plus `steps` (per start, beam_one's list), rounds (the starts
    of every round) and played [N] bool: the resident envs a round loaded."""
    N, T = env_kw["num_envs"], env_kw["max_actions"]
    M = starts[2].shape[0]
    S = N // K
    recs = [beam_one(orc, env_kw, (starts[0][s], starts[1][s], int(starts[2][s])), K, probs_of) for s in range(M)]
    out = dict(best_state=np.stack([r["best_state"] for r in recs]).astype(np.int8),
               best_active=np.array([r["best_active"] for r in recs], np.uint32),
               best_mant=np.array([r["best_mant"] for r in recs], np.float64))
    for k in ("best_gap", "best_step", "best_beam", "initial_gap", "best_exp"):
        out[k] = np.array([r[k] for r in recs], np.int32)
    for k in ("parents", "actions", "mant", "exp"):
        out[k] = np.stack([r[k] for r in recs])
    played = np.zeros(N, bool)
    played[:min(S, M) * K] = True
    out.update(log_prob=log_prob(out["best_mant"], out["best_exp"]), path=pref.padded([r["path"] for r in recs], T),
               steps=[r["steps"] for r in recs], rounds=[list(range(b, min(b + S, M))) for b in range(0, M, S)], played=played)
    return out


# ---------------------------------------------------------------- what a replay contains
def coverage(rec, K):
    """The situations of a replay, as counts over (start, step) or over starts."""
    c = dict(fewer_than_K_at_step0=0, dead_slots=0, reached_optimum_early=0, never_optimum=0, result_off_slot0=0,
             shared_and_childless_parent=0, index_decided=0, result_at_start=0)
    T = rec["parents"].shape[1]
    for s, steps in enumerate(rec["steps"]):
        c["fewer_than_K_at_step0"] += steps[0]["ncand"] < K
        c["reached_optimum_early"] += rec["best_gap"][s] == 0 and len(steps) < T
        c["never_optimum"] += rec["best_gap"][s] > 0
        c["result_off_slot0"] += rec["best_step"][s] > 0 and rec["best_beam"][s] != 0
        c["result_at_start"] += rec["best_step"][s] == 0
        nlive = 1
        for st in steps:
            par = [k for k, _, _, _ in st["chosen"]]
            c["dead_slots"] += len(par) < K
            c["index_decided"] += st["index_decided"]
            counts = [par.count(k) for k in range(nlive)]
            c["shared_and_childless_parent"] += max(counts) >= 2 and min(counts) == 0
            nlive = len(par)
    c["rounds"] = len(rec["rounds"])
    c["partial_round"] = int(len(rec["rounds"][-1]) < len(rec["rounds"][0])) if len(rec["rounds"]) > 1 else 0
    return {k: int(v) for k, v in c.items()}


# ---------------------------------------------------------------- shapes
# Q, K, N envs, M starts, T = max_actions, and the policy: hidden width, layers, seed and a scale on the Glorot parameters (a
# scale above 1 sharpens the near-uniform distribution of an untrained policy, so that weights spread over many binades; 0: all
# parameters zero, every valid action of a state equally likely: every candidate of a live slot ties).  Env seed ref.SEED; the
# starts are search_ref's: the reset states of the envs of global ids START_OFFSET on
SHAPES = {
    "q8-k1": dict(Q=8, K=1, N=5, M=5, T=16, hid=128, L=2, pseed=3, scale=1.0,                # the greedy trajectory improves on four
                  ids=(5000, 5006, 5016, 5032, 5037)),
    "q8-k3": dict(Q=8, K=3, N=11, M=4, T=16, hid=128, L=2, pseed=3, scale=4.0,               # two rounds, the second partial
                  ids=(5000, 43993, 5002, 5003)),
    "q8-k8": dict(Q=8, K=8, N=24, M=3, T=24, hid=128, L=2, pseed=3, scale=1.0, ids=(24293, 5001, 731)),
    "q8-k64": dict(Q=8, K=64, N=130, M=2, T=12, hid=128, L=2, pseed=3, scale=4.0, ids=(894, 5001)),
    "q8-k130": dict(Q=8, K=130, N=300, M=3, T=8, hid=128, L=2, pseed=3, scale=1.0),          # K > A; two rounds, one start in the second
    "q32-k5": dict(Q=32, K=5, N=12, M=3, T=10, hid=128, L=2, pseed=3, scale=1.0),
    "q32-k256": dict(Q=32, K=256, N=256, M=1, T=8, hid=128, L=2, pseed=3, scale=4.0),        # 131,072 candidates per step
    "ties": dict(Q=8, K=3, N=7, M=2, T=8, hid=128, L=2, pseed=3, scale=0.0),
}
GPU_SHAPES = ("q8-k1", "q8-k3", "q8-k8", "q8-k64", "q8-k130", "q32-k5", "q32-k256")
HOST_SHAPES = ("q8-k3", "q8-k8", "q8-k130", "q32-k5", "ties")       # replayed with the oracle's probabilities (seconds each)
START_OFFSET = sref.START_OFFSET


def env_kw(name):
    c = SHAPES[name]
    return dict(num_envs=c["N"], Q=c["Q"], max_actions=c["T"], seed=ref.SEED, global_offset=0)


def starts(orc, name):
    """The reset states (episode counter 1) of the envs of global ids START_OFFSET .. START_OFFSET + M - 1, or of the ids the
    shape names (`ids`: among them reset states two or four score points above their optimum, which a beam can reach, and
    states on which the arg-max trajectory improves)."""
    c = SHAPES[name]
    ids = c.get("ids", tuple(range(START_OFFSET, START_OFFSET + c["M"])))
    assert len(ids) == c["M"]
    rows = []
    for g in ids:
        e = orc.Env(Q=c["Q"], max_actions=c["T"], N=1, seed=ref.SEED, global_offset=g)
        e.episode[:] = 1
        e.reset()
        rows.append((e.score[0].copy(), e.degree[0].copy(), np.uint32(e.active[0])))
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.array([r[2] for r in rows], np.uint32)


def policy_params(orc, name):
    c = SHAPES[name]
    return (orc.glorot_params(ref.F, c["hid"], c["L"], seed=c["pseed"]) * np.float32(c["scale"])).astype(np.float32)


def oracle_probs(orc, name):
    """probs_of from the oracle's device-order forward ("dev" mode), one state at a time."""
    c = SHAPES[name]
    params = policy_params(orc, name)

    def probs_of(states, active):
        return np.stack([orc.action_probabilities(params, ref.F, c["hid"], states[i], int(active[i]), "dev", n_hidden=c["L"])
                         for i in range(states.shape[0])]).astype(np.float32)
    return probs_of


def host_reference(orc, name):
    """beam_replay with the oracle's probabilities, once per process and never modified."""
    key = ("beam-host", name)
    if key not in ref._CACHE:
        ref._CACHE[key] = beam_replay(orc, env_kw(name), starts(orc, name), SHAPES[name]["K"], oracle_probs(orc, name))
    return ref._CACHE[key]


def path_log_prob(probs_rows):
    """sum(log(float64(p))) over the probabilities along a path, in path order (math.fsum: no rounding of its own to speak of)."""
    return math.fsum(math.log(float(np.float64(p))) for p in probs_rows)
