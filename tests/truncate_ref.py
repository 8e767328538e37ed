"""Host reference of the top-k / nucleus truncation of tempered sampling (HipPolicy.truncation).  Everything here
comes from the CPU oracle (oracle/oracle.py), numpy float32 and tests/select_ref.py, never from the device; none of those is
changed.

The rule, per step of one env, on p = select_ref.probabilities (the tempered masked softmax in the device's order), A entries:

    b precedes a    iff  p[b] > p[a] or (p[b] == p[a] and b < a)
    rank[a]         =    the number of b that precede a
    mass_before[a]  =    the float32 sum of p[b] over the b that precede a, added one by one in ascending b from 0.0f
    keep[a]         =    (top_k == 0 or rank[a] < top_k) and (float32(top_p) == 1 or mass_before[a] < float32(top_p))
    q               =    keep ? p : 0
    S'              =    the sum of q in the softmax's own order: per lane j and tile ((q0 + q1) + q2) + q3 of the entries
                         128 ts + 4 j + 0..3, tile partials in tile order, then the 16, 8, 4, 2, 1 butterfly over the 32 lanes
    p''             =    q / S'
    a               =    orc.categorical_sample(p'', u) with the uniform and the run-off rule of select_ref.select_action

The default truncation (0, 1.0) is select_ref.select_action itself: no renormalisation.  Any other renormalises, also one
that keeps everything.  "greedy" ignores the truncation.

TruncateOracle is the oracle module with collect_rollouts_tn replaced, like select_ref.SelectOracle, so that episodes_ref,
search_ref, resample_ref and path_ref run unchanged on its actions.  The case tables live at the end of the file."""
import numpy as np

import episodes_ref as ref
import path_ref as pref
import resample_ref as rref
import search_ref as sref
import select_ref as S

DEFAULT = (0, 1.0)


def is_default(trunc):
    return int(trunc[0]) == 0 and float(trunc[1]) == 1.0


def rank_and_mass(p):
    """(rank int32 [A], mass_before float32 [A]) of a float32 vector: one pass over b in ascending order, every a at once."""
    p = np.asarray(p)
    assert p.dtype == np.float32
    idx = np.arange(p.size)
    rank = np.zeros(p.size, np.int32)
    mass = np.zeros(p.size, np.float32)
    with np.errstate(invalid="ignore"):
        for b in range(p.size):
            prec = (p[b] > p) | ((p[b] == p) & (b < idx))
            rank += prec
            added = mass + p[b]                              # float32 + float32: one rounding
            assert added.dtype == np.float32
            mass = np.where(prec, added, mass)
    return rank, mass


def keep_set(p, top_k, top_p):
    """bool [A]: the entries a truncation keeps."""
    rank, mass = rank_and_mass(p)
    tp = np.float32(top_p)
    keep = np.ones(p.size, bool)
    if int(top_k) != 0:
        keep &= rank < int(top_k)
    if tp != np.float32(1.0):
        keep &= mass < tp
    return keep


def device_order_sum(q):
    """The float32 sum of q [128 * TPS] in the order the forward's softmax sums: lane partials, tiles, butterfly."""
    assert q.dtype == np.float32 and q.size % 128 == 0
    t = q.reshape(-1, 32, 4)                                 # [tile][lane][i]
    lane = None
    for ts in range(t.shape[0]):
        st = ((t[ts, :, 0] + t[ts, :, 1]) + t[ts, :, 2]) + t[ts, :, 3]
        lane = st if ts == 0 else lane + st
    for off in (16, 8, 4, 2, 1):
        lane = lane + lane[np.arange(32) ^ off]
    assert lane.dtype == np.float32
    return lane[0]


def truncate(p, top_k, top_p):
    """p'' float32 [A] of a non-default truncation."""
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(keep_set(p, top_k, top_p), p, np.float32(0.0)).astype(np.float32)
        out = q / device_order_sum(q)
    assert out.dtype == np.float32
    return out


_TRUNCATED = {}


def truncated_probabilities(orc, oenv, n, params, hid, L, tau, trunc):
    """p'' of env n's current state (p itself at the default truncation), remembered per (p, truncation): a rejected move
    leaves the state as it was."""
    p = S.probabilities(orc, oenv, n, params, hid, L, tau)
    if is_default(trunc):
        return p
    key = (p.tobytes(), int(trunc[0]), float(np.float32(trunc[1])))
    if key not in _TRUNCATED:
        _TRUNCATED[key] = truncate(p, *trunc)
    return _TRUNCATED[key]


def select_action(orc, oenv, n, params, hid, L, rule, tau, trunc):
    """select_ref.select_action under a truncation: (0-based action, the distribution drawn from, flag).  Does not step."""
    if rule == "greedy" or is_default(trunc):
        return S.select_action(orc, oenv, n, params, hid, L, rule, tau)
    p = truncated_probabilities(orc, oenv, n, params, hid, L, tau, trunc)
    c = oenv.e.contents
    w = orc.philox([(int(c.global_offset) + n) & 0xFFFFFFFF, int(oenv.tick[n]), 0, 0],
                   [int(c.seed) & 0xFFFFFFFF, int(c.seed) >> 32])
    a, err = orc.categorical_sample(p, orc.u01(w[0]))
    if not err:
        return a, p, 0
    pos = np.flatnonzero(p > 0)
    return (int(pos[-1]), p, 32) if pos.size else (a, p, 8)


def truncate_rollout_tn(orc, oenv, params, hid, T, rule, tau, trunc, L=2):
    """select_ref.select_rollout_tn under a truncation: the same dict of [T, N] columns."""
    N = oenv.N
    out = dict(states=np.empty((T, N, oenv.H, oenv.F), np.int8), active=np.empty((T, N), np.uint32),
               p_sel=np.empty((T, N), np.float32), actions=np.empty((T, N), np.int32), rewards=np.empty((T, N), np.float32),
               done=np.empty((T, N), np.uint8))
    for t in range(T):
        for n in range(N):
            out["states"][t, n] = oenv.observe_one(n)
            out["active"][t, n] = oenv.active[n]
            a, p, flag = select_action(orc, oenv, n, params, hid, L, rule, tau, trunc)
            oenv.err[n] |= flag
            oenv.step_one(n, a)
            out["p_sel"][t, n], out["actions"][t, n] = p[a], a
            out["rewards"][t, n], out["done"][t, n] = oenv.reward[n], oenv.done[n]
            if oenv.done[n]:
                oenv.reset_one(n)
    return out


class TruncateOracle:
    """The oracle module with collect_rollouts_tn under a selection and a truncation; every other attribute is the oracle's."""

    def __init__(self, orc, rule, tau, trunc=DEFAULT):
        self._orc, self.rule, self.tau, self.trunc = orc, rule, float(tau), (int(trunc[0]), float(trunc[1]))

    def __getattr__(self, name):
        return getattr(self._orc, name)

    def collect_rollouts_tn(self, env, params, HID, T, mode_dev=True, n_hidden=2):
        assert mode_dev
        return truncate_rollout_tn(self._orc, env, params, HID, T, self.rule, self.tau, self.trunc, n_hidden)


# ---------------------------------------------------------------- the calls (select_ref's, with the truncation in the key)
def episodes(orc, case, sel, trunc):
    """select_ref.episodes under a truncation: the [T, N] columns of an episodes-form call plus episode / tick [N] afterwards."""
    key = ("truncate-episodes", case["name"], sel, trunc)
    if key not in ref._CACHE:
        so = TruncateOracle(orc, *sel, trunc)
        exp = ref.expected_episodes(so, ref.env_kw_of(case), ref.policy_params(orc, case), case["hid"], case["L"],
                                    case["episodes"])
        T = max(col["length"] for col in exp.values())
        cols = ref.assemble(exp, case["N"], T, 4 * case["Q"])
        cols.update(episode=np.array([exp[n]["episode_after"] for n in range(case["N"])], np.int64),
                    tick=np.array([exp[n]["tick_after"] for n in range(case["N"])], np.int64))
        ref._CACHE[key] = cols
    return ref._CACHE[key]


def best_states(orc, case, sel, trunc):
    """best_states_(reset form, scores, action types, actions) under a truncation (select_ref.best_states)."""
    key = ("truncate-best", case["name"], sel, trunc)
    if key not in ref._CACHE:
        cols = episodes(orc, case, sel, trunc)
        rec = sref.tracked_replay(orc, ref.env_kw_of(case), cols["actions"], case["episodes"])
        rows = []
        for n in range(case["N"]):
            t_valid = np.flatnonzero(cols["valid"][:, n])
            first = 0
            for end in (int(x) + 1 for x in np.flatnonzero(cols["done"][t_valid, n])):
                rows.append([int(a) for a in cols["actions"][t_valid[first:end], n]])
                first = end
        assert len(rows) == case["episodes"]
        rec.update(actions=pref.padded(rows, case["M"]))
        ref._CACHE[key] = rec
    return ref._CACHE[key]


def trajectories(orc, case, sel, trunc, columns, episode):
    """select_ref.trajectories under a truncation: one trajectory of each env of `columns`, each on a one-env oracle."""
    key = ("truncate-traj", case["name"], sel, trunc, tuple(columns), episode)
    if key not in ref._CACHE:
        so, kw = TruncateOracle(orc, *sel, trunc), ref.env_kw_of(case)
        params = ref.policy_params(orc, case)
        recs, rows = [], []
        for n in columns:
            e = ref._env(orc, kw, 1, n)
            e.episode[0] = episode
            e.reset()
            rec, acts = pref.play_from_actions(so, kw, n, params, case["hid"], case["L"], sref.state_of(e, 0), 0)
            recs.append(rec)
            rows.append(acts)
        out = sref.stack(recs, case["M"])
        out["actions"] = pref.padded(rows, case["M"])
        ref._CACHE[key] = out
    return ref._CACHE[key]


def search(orc, shape, sel, trunc):
    """search_best_states_(path, clone_gaps) under a truncation on shape (M, K, N, max_actions) (select_ref.search)."""
    key = ("truncate-search", shape, sel, trunc)
    if key not in ref._CACHE:
        M, K, N, T = shape
        so = TruncateOracle(orc, *sel, trunc)
        kw = S.search_env_kw(N, T)
        hid, L = rref.CASE["hid"], rref.CASE["L"]
        params = orc.glorot_params(ref.F, hid, L, seed=rref.CASE["pseed"])
        starts = S.search_starts(orc, M, T)
        out = sref.search_replay(so, kw, params, hid, L, starts, K)
        out["path"] = pref.search_paths(so, kw, params, hid, L, starts, K)["path"]
        ref._CACHE[key] = out
    return ref._CACHE[key]


def resample(orc, shape, sel, trunc):
    """search_resample_states_(path, donors, clone_gaps) under a truncation (select_ref.resample)."""
    key = ("truncate-resample", shape, sel, trunc)
    if key not in ref._CACHE:
        M, K, N, T, R, m0 = shape
        so = TruncateOracle(orc, *sel, trunc)
        ref._CACHE[key] = pref.resample_paths(so, rref.env_kw(shape), rref.policy_params(orc), rref.CASE["hid"], rref.CASE["L"],
                                              S.search_starts(orc, M, T), K, R, m0)
    return ref._CACHE[key]


# ---------------------------------------------------------------- ties
def tie_probabilities(orc, active, Q, tau=1.0):
    """The tempered p of a state with active-quad word `active` under select_ref.tie_params: logits (0, 1, 1, 0) on every row,
    so every active row holds two equal maxima and two equal minima."""
    l = np.tile(np.array([0.0, 1.0, 1.0, 0.0], np.float32), 4 * Q)
    return orc.masked_softmax((l * np.float32(1.0 / tau)).astype(np.float32), int(active), "dev")


def tie_maxima(active, Q):
    """The action indices of the tied maxima in ascending order: entries 1 and 2 of every row of every active quad."""
    return [16 * q + 4 * r + i for q in range(Q) if (int(active) >> q) & 1 for r in range(4) for i in (1, 2)]


# ---------------------------------------------------------------- cases
TRUNCATIONS = ((1, 1.0), (2, 1.0), (5, 1.0), (0, 0.5), (0, 0.9), (3, 0.8))
# the whole-trajectory cases of the main shape: (selection, truncation)
MAIN_CASES = ((("sample", 0.7), (2, 1.0)), (("sample", 0.7), (0, 0.5)), (("sample", 0.7), (3, 0.8)),
              (("sample", 1.0), (5, 1.0)), (("sample", 1.0), (0, 0.9)))
SIDE_CASE = (("sample", 0.7), (3, 0.8))
SEARCH_CASE = (("sample", 2.0), (0, 0.9))
SEARCH_SHAPE = S.SEARCH_SHAPE                   # (4, 12, 48, 24)
RESAMPLE_SHAPE = S.RESAMPLE_SHAPES[0]           # (4, 12, 48, 24, 2, 3)
TIE_MASKS_Q8 = S.TIE_MASKS_Q8
TIE_MASKS_Q32 = S.TIE_MASKS_Q32
# at this temperature the tie policy's scaled logits are (0, 128, 128, 0): exp(-128) is 0 in float32, so the maxima are uniform,
# 1 / n each; every tie mask has a power-of-two number of active quads, so 1 / n and the sequential sums of it are exact
TIE_UNIFORM_TAU = 2.0 ** -7
