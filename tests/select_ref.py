"""Host reference of the action selection rules (HipPolicy.selection): tempered sampling and greedy.  Everything
here comes from the CPU oracle (oracle/oracle.py), numpy and the other reference modules of tests/, never from the device; none
of those is changed.

The rule, per step of one env, restated on the oracle's Python API:

    obs = Env.observe_one(n)
    l   = orc.mlp_logits(params, F, hid, obs, "dev", L)          the device-order logits
    l'  = l * np.float32(1.0 / tau)                               one float32 multiply per logit
    p   = orc.masked_softmax(l', active, "dev")
    "sample":  u = orc.u01(orc.philox([global id, tick, 0, 0], [seed lo, seed hi])[0]);  a = orc.categorical_sample(p, u),
               and when that walk runs off the end (its err), the last index with p > 0
    "greedy":  a = np.argmax(p)                                   the first maximum
    Env.step_one(n, a);  p_sel = p[a]

select_rollout_tn is orc.collect_rollouts_tn's loop (t outer, env inner, auto-reset on done) on that step, and at ("sample", 1)
it returns the bytes orc.collect_rollouts_tn returns (tests/test_select_host.py holds that).  SelectOracle is the oracle module
with collect_rollouts_tn replaced by it: every replay of tests/ that takes its actions from orc.collect_rollouts_tn --
episodes_ref.expected_episodes, search_ref.search_replay, resample_ref.resample_replay, path_ref.search_paths /
resample_paths -- then runs its own round / clone / tick schedule and bookkeeping on the selected actions, unchanged.

The case tables of tests/test_select_host.py and tests/test_gpu_select.py live at the end of the file."""
import numpy as np

import episodes_ref as ref
import path_ref as pref
import resample_ref as rref
import search_ref as sref

DEFAULT = ("sample", 1.0)


_LOGITS = {}


def logits(orc, params, F, hid, L, obs):
    """orc.mlp_logits(.., "dev", L) of one observation, remembered per (parameters, observation): a rejected move leaves the
    state as it was, so a trajectory asks for the same rows again and again (greedy: almost always), and the logits do not
    depend on the selection.  The oracle's device-order forward is the expensive part of every replay here."""
    key = (hash(params.tobytes()), hid, L, obs.tobytes())
    if key not in _LOGITS:
        _LOGITS[key] = orc.mlp_logits(params, F, hid, obs, "dev", L)
    return _LOGITS[key]


def probabilities(orc, oenv, n, params, hid, L, tau):
    """The tempered masked softmax of env n's current state, float32 [A]."""
    l = logits(orc, params, oenv.F, hid, L, oenv.observe_one(n))
    inv = np.float32(1.0 / tau)
    scaled = (l * inv).astype(np.float32)
    assert l.dtype == np.float32 and (l * inv).dtype == np.float32
    return orc.masked_softmax(scaled, int(oenv.active[n]), "dev")


def select_action(orc, oenv, n, params, hid, L, rule, tau):
    """(0-based action, p [A], flag) of env n from the state and tick it holds; flag 32: the walk ran off the end, 8: no
    positive entry (the bits the device sets).  Does not step."""
    p = probabilities(orc, oenv, n, params, hid, L, tau)
    c = oenv.e.contents
    if rule == "greedy":
        a = int(np.argmax(p))
        return a, p, 0 if p[a] > 0 else 8
    assert rule == "sample"
    w = orc.philox([(int(c.global_offset) + n) & 0xFFFFFFFF, int(oenv.tick[n]), 0, 0],
                   [int(c.seed) & 0xFFFFFFFF, int(c.seed) >> 32])
    a, err = orc.categorical_sample(p, orc.u01(w[0]))
    if not err:
        return a, p, 0
    pos = np.flatnonzero(p > 0)
    return (int(pos[-1]), p, 32) if pos.size else (a, p, 8)


def select_rollout_tn(orc, oenv, params, hid, T, rule, tau, L=2):
    """orc.collect_rollouts_tn (T steps of every env, auto-reset on done) under a selection: the same dict of [T, N] columns."""
    N = oenv.N
    out = dict(states=np.empty((T, N, oenv.H, oenv.F), np.int8), active=np.empty((T, N), np.uint32),
               p_sel=np.empty((T, N), np.float32), actions=np.empty((T, N), np.int32), rewards=np.empty((T, N), np.float32),
               done=np.empty((T, N), np.uint8))
    for t in range(T):
        for n in range(N):
            out["states"][t, n] = oenv.observe_one(n)
            out["active"][t, n] = oenv.active[n]
            a, p, flag = select_action(orc, oenv, n, params, hid, L, rule, tau)
            oenv.err[n] |= flag
            oenv.step_one(n, a)
            out["p_sel"][t, n], out["actions"][t, n] = p[a], a
            out["rewards"][t, n], out["done"][t, n] = oenv.reward[n], oenv.done[n]
            if oenv.done[n]:
                oenv.reset_one(n)
    return out


class SelectOracle:
    """The oracle module with collect_rollouts_tn under a selection; every other attribute is the oracle's own."""

    def __init__(self, orc, rule, tau):
        self._orc, self.rule, self.tau = orc, rule, float(tau)

    def __getattr__(self, name):
        return getattr(self._orc, name)

    def collect_rollouts_tn(self, env, params, HID, T, mode_dev=True, n_hidden=2):
        assert mode_dev
        return select_rollout_tn(self._orc, env, params, HID, T, self.rule, self.tau, n_hidden)


# ---------------------------------------------------------------- the calls
def episodes(orc, case, sel):
    """An episodes-form call (best_states_, the evaluators: trajectory e on env e mod N, reset before each) under `sel` on a
    fresh env: the [T, N] columns of ref.assemble plus episode / tick [N] afterwards.  Once per process, never modified."""
    key = ("select-episodes", case["name"], sel)
    if key not in ref._CACHE:
        so = SelectOracle(orc, *sel)
        exp = ref.expected_episodes(so, ref.env_kw_of(case), ref.policy_params(orc, case), case["hid"], case["L"],
                                    case["episodes"])
        T = max(col["length"] for col in exp.values())
        cols = ref.assemble(exp, case["N"], T, 4 * case["Q"])
        cols.update(episode=np.array([exp[n]["episode_after"] for n in range(case["N"])], np.int64),
                    tick=np.array([exp[n]["tick_after"] for n in range(case["N"])], np.int64))
        ref._CACHE[key] = cols
    return ref._CACHE[key]


def best_states(orc, case, sel):
    """best_states_(reset form, scores, action types, actions) under `sel`: search_ref.tracked_replay fed with the selected
    actions, plus actions int16 [num_traj, max_actions] (0-based, -1 behind the end) and p_sel per trajectory (a list)."""
    key = ("select-best", case["name"], sel)
    if key not in ref._CACHE:
        cols = episodes(orc, case, sel)
        rec = sref.tracked_replay(orc, ref.env_kw_of(case), cols["actions"], case["episodes"])
        rows, psel = [], []
        for n in range(case["N"]):
            t_valid = np.flatnonzero(cols["valid"][:, n])
            first = 0
            for end in (int(x) + 1 for x in np.flatnonzero(cols["done"][t_valid, n])):
                rows.append([int(a) for a in cols["actions"][t_valid[first:end], n]])
                psel.append(cols["p_sel"][t_valid[first:end], n].copy())
                first = end
        assert len(rows) == case["episodes"]
        rec.update(actions=pref.padded(rows, case["M"]), p_sel=psel)
        ref._CACHE[key] = rec
    return ref._CACHE[key]


def trajectories(orc, case, sel, columns, episode):
    """One trajectory of each env of `columns` from the reset state of episode counter `episode` at tick 0, under `sel`:
    best_states_ with one trajectory per env (episode = 1: the reset form resets a fresh env once more; 0: the form without a
    reset plays from the state a fresh env holds).  Returns sref.stack of the records plus actions int16 (0-based, -1 padding),
    one row per column.  Each column on a one-env oracle, so a large N costs nothing here."""
    key = ("select-traj", case["name"], sel, tuple(columns), episode)
    if key not in ref._CACHE:
        so, kw = SelectOracle(orc, *sel), ref.env_kw_of(case)
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


def grid_columns(N):
    """Env 0, both sides of every multiple of 64 below N, and N - 1."""
    cols = {0, N - 1}
    for m in range(64, N, 64):
        cols |= {m - 1, m}
    return sorted(cols)


def state_changes(orc, case, cols):
    """(steps that changed score, degree or the active quads; steps) of an episodes-form record, replayed on the oracle env with
    ref.teacher_forced's schedule: a rejected move leaves the state as it was."""
    kw = ref.env_kw_of(case)
    oenv = ref._env(orc, kw)
    oenv.episode[:] = 1
    oenv.reset()
    left = ref.quotas(case["N"], case["episodes"])
    changed = total = 0
    for t in range(cols["actions"].shape[0]):
        for n in (int(x) for x in np.flatnonzero(left > 0)):
            before = sref.state_of(oenv, n)
            oenv.step_one(n, int(cols["actions"][t, n]))
            after = sref.state_of(oenv, n)
            total += 1
            changed += not (np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2] == after[2])
            if oenv.done[n]:
                left[n] -= 1
                if left[n] > 0:
                    oenv.reset_one(n)
    return changed, total


def evaluator_values(orc, case, sel, kind):
    """evaluate_trajectories under `sel` ("return", "best", "normalized").  The case must hold no trajectory that starts on
    its optimum (ref.skip_table: such a trajectory is not played by "normalized", which moves the ticks of what follows)."""
    assert not ref.skip_table(orc, ref.env_kw_of(case), case["episodes"]).any()
    cols = episodes(orc, case, sel)
    rec = ref.teacher_forced(orc, ref.env_kw_of(case), cols["actions"], case["episodes"])
    return ref.evaluator_values(kind, rec)


def search(orc, shape, sel, hid=None, L=None):
    """search_best_states_(path, clone_gaps) under `sel` on shape (M, K, N, max_actions): search_ref.search_replay's records
    and clone gaps with path_ref.search_paths' winner prefix (0-based, -1 padding), ticks afterwards."""
    key = ("select-search", shape, sel, hid, L)
    if key not in ref._CACHE:
        M, K, N, T = shape
        so = SelectOracle(orc, *sel)
        kw = search_env_kw(N, T)
        hid, L = hid or rref.CASE["hid"], L or rref.CASE["L"]
        params = orc.glorot_params(ref.F, hid, L, seed=rref.CASE["pseed"])
        starts = search_starts(orc, M, T)
        out = sref.search_replay(so, kw, params, hid, L, starts, K)
        out["path"] = pref.search_paths(so, kw, params, hid, L, starts, K)["path"]
        ref._CACHE[key] = out
    return ref._CACHE[key]


def resample(orc, shape, sel):
    """search_resample_states_(path, donors, clone_gaps) under `sel` on shape (M, K, N, max_actions, R, survivors):
    path_ref.resample_paths (which holds resample_ref's result arrays, donors, clone gaps and ticks)."""
    key = ("select-resample", shape, sel)
    if key not in ref._CACHE:
        M, K, N, T, R, m0 = shape
        so = SelectOracle(orc, *sel)
        ref._CACHE[key] = pref.resample_paths(so, rref.env_kw(shape), rref.policy_params(orc), rref.CASE["hid"], rref.CASE["L"],
                                              search_starts(orc, M, T), K, R, m0)
    return ref._CACHE[key]


def search_env_kw(N, T):
    return dict(num_envs=N, Q=rref.CASE["Q"], max_actions=T, seed=ref.SEED, global_offset=rref.CASE["goff"])


def search_starts(orc, M, T):
    """search_ref.search_starts' states (the reset states of global ids START_OFFSET ..; the reset does not depend on
    max_actions)."""
    e = orc.Env(Q=rref.CASE["Q"], max_actions=T, N=M, seed=ref.SEED, global_offset=sref.START_OFFSET)
    e.episode[:] = 1
    e.reset()
    return e.score.copy(), e.degree.copy(), e.active.copy().astype(np.uint32)


# ---------------------------------------------------------------- ties
def tie_params(orc, hid, L):
    """A policy whose every row has logits (0, 1, 1, 0): the last layer's weights 0, its bias (0, 1, 1, 0)."""
    p = orc.glorot_params(ref.F, hid, L, seed=3).copy()
    p[-(4 * hid + 4):-4] = 0.0
    p[-4:] = (0.0, 1.0, 1.0, 0.0)
    return p


def tie_expected(orc, active, Q, tau=1.0):
    """(0-based greedy action, p_sel) of a state with active-quad word `active` under tie_params: the probabilities depend on
    the mask alone, so any env of that Q serves as the carrier of the mask."""
    l = np.tile(np.array([0.0, 1.0, 1.0, 0.0], np.float32), 4 * Q)
    p = orc.masked_softmax((l * np.float32(1.0 / tau)).astype(np.float32), int(active), "dev")
    a = int(np.argmax(p))
    return a, p[a]


def lowest_quad(active):
    return (int(active) & -int(active)).bit_length() - 1


def tie_states(masks, Q):
    """Env states (score, degree [n, 4Q], active [n]) with the given active-quad words that set_internal accepts: small
    entries on the active quads, 0 elsewhere.  The tie policy's logits do not depend on them."""
    act = np.array(masks, np.uint32)
    on = ((act[:, None] >> (np.arange(4 * Q, dtype=np.uint32) >> 2)[None, :]) & 1).astype(np.int8)
    rng = np.random.default_rng(11)
    return (rng.integers(-2, 3, on.shape).astype(np.int8) * on, rng.integers(3, 6, on.shape).astype(np.int8) * on, act)


TIE_MASKS_Q8 = (0xFF, 0x01, 0x80, 0x28, 0xF0, 0x06, 0x81)
# tiles 1 and 2 alone (quads 8 .. 23): the arg-max has to cross tiles, and tile 0's masked zeros must not win
TIE_MASKS_Q32 = ((1 << 9) | (1 << 20), 1 << 8, (1 << 15) | (1 << 16), 0x00FFFF00, 1 << 23, 1 << 16)


# ---------------------------------------------------------------- cases
SELECTIONS = (("sample", 0.5), ("sample", 2.0), ("sample", 0.7), ("sample", 1.3), ("sample", 0.25), ("greedy", 1.0),
              ("greedy", 0.7))
TEMPERATURES = (0.5, 2.0, 0.7, 1.3)


def _case(name, N, episodes, Q=8, hid=128, L=2, M=6, goff=0):
    return dict(name="select-" + name, N=N, episodes=episodes, goff=goff, Q=Q, hid=hid, L=L, M=M, pseed=3)


# the main shape under every selection; the others under an inexact temperature and greedy
MAIN = _case("h256", 70, 100, hid=256, M=20)
SIDE = (_case("h128", 24, 30, M=8), _case("L3", 24, 30, L=3, M=8), _case("h96", 24, 30, hid=96, M=8),
        _case("q32", 10, 14, Q=32, M=6))
SIDE_SELECTIONS = (("sample", 0.7), ("greedy", 0.7))
GREEDY_COVERAGE = _case("greedy-coverage", 24, 24, hid=256, M=20)       # the issue's Q = 8, max_actions = 20, N = 24 case
# 1100 envs: at hidden 256 the forward's grid is 256 workgroups of 4 waves, so envs 1024 .. 1099 are a wave's second state; at
# hidden 128 (two workgroups per CU, 512 in the grid) one pass takes them all, the case is the partly filled last workgroups
BIG = (_case("n1100-h128", 1100, 1100, M=6), _case("n1100-h256", 1100, 1100, hid=256, M=6))
SEARCH_SHAPE = (4, 12, 48, 24)
RESAMPLE_SHAPES = ((4, 12, 48, 24, 2, 3), (5, 13, 70, 8, 2, 3))
SEARCH_SELECTIONS = (("sample", 0.7), ("sample", 2.0), ("greedy", 1.0))


def by_name(name):
    return next(c for c in (MAIN, GREEDY_COVERAGE) + BIG + SIDE if c["name"] == "select-" + name)
