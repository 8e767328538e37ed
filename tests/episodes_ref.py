"""Host reference of the whole-episode rollout form (collect_rollouts!(rollouts, env, policy, num_episodes, discount),
src/rollout_buffer.jl:66-79) and of the evaluators built on it (src/evaluate.jl:1-25, test/quad_game_utilities.jl:280-307,
369-387).  Everything here comes from the CPU oracle (oracle/oracle.py) and numpy, never from the device.

Semantics restated: episode e of a call is played by env e mod N, so env n plays len(range(n, num_episodes, N)) episodes
(its quota); every env is reset before the call's first episode (the idle ones too: that consumes one episode counter) and a
busy env again before each further episode of its quota, not after its last.  An env's trajectory depends only on its global
id, its episode counter and its tick (the Philox counters), so one column can be replayed alone on a one-env oracle.

The case tables of tests/test_episodes_host.py and tests/test_gpu_episodes_form.py live at the end of the file."""
import numpy as np

F = 72
SEED = 13                       # the seed the ids below were searched with
# Q = 8, seed 13: global ids whose reset with episode counter c lands on the optimum (policy independent)
ON_OPTIMUM = {107433: 1, 160637: 1, 165273: 1, 167413: 1, 165114: 2, 4624: 3, 51504: 3}


# ---------------------------------------------------------------- small pieces
def quotas(N, num_episodes):
    return np.array([len(range(n, num_episodes, N)) for n in range(N)], np.int64)


def policy_params(orc, case):
    return orc.glorot_params(F, case["hid"], case["L"], seed=case["pseed"])


def env_kw_of(case):
    return dict(num_envs=case["N"], Q=case["Q"], max_actions=case["M"], seed=SEED, global_offset=case["goff"])


def _env(orc, env_kw, N=None, first=0):
    return orc.Env(Q=env_kw["Q"], max_actions=env_kw["max_actions"], N=env_kw["num_envs"] if N is None else N,
                   seed=env_kw["seed"], global_offset=env_kw.get("global_offset", 0) + first)


def scores(oenv):
    """env.current_score (sum |vertex score| over the active quads) and env.opt_score (|sum|) of every env."""
    sc = oenv.score.astype(np.int64).reshape(oenv.N, oenv.V)
    act = np.asarray(oenv.active).astype(np.int64)
    on = ((act[:, None] >> (np.arange(oenv.V) >> 2)[None, :]) & 1).astype(bool)
    return (np.abs(sc) * on).sum(axis=1), np.abs((sc * on).sum(axis=1))


def _start(n, episode0, tick0):
    return (1 if episode0 is None else int(episode0[n])), (0 if tick0 is None else int(tick0[n]))


# ---------------------------------------------------------------- the episodes form, column by column
def expected_episodes(orc, env_kw, params, hid, L, num_episodes, columns=None, episode0=None, tick0=None):
    """Column n of the buffer collect_rollouts!(.., num_episodes, ..) fills, from orc.collect_rollouts_tn (steps and
    auto-resets) on the one-env oracle of global id offset + n, cut at the env's quota-th terminal.  A column is run
    quota * max_actions steps, as far as its own quota can reach.  episode0 / tick0: the [N] counters the envs hold when the
    call starts (a fresh device env: 1 and 0, create consumed episode counter 0).  Returns {n: dict(states, active,
    actions, p_sel, rewards, done, length, episode_after, tick_after)}."""
    N, M = env_kw["num_envs"], env_kw["max_actions"]
    quota = quotas(N, num_episodes)
    out = {}
    for n in (range(N) if columns is None else columns):
        ep, tk = _start(n, episode0, tick0)
        q = int(quota[n])
        e = _env(orc, env_kw, 1, n)
        e.episode[0], e.tick[0] = ep, tk
        e.reset()                                               # reset!(env) before the first episode, idle envs included
        length = 0
        if q:
            r = orc.collect_rollouts_tn(e, params, hid, q * M, mode_dev=True, n_hidden=L)
            assert int(e.err[0]) & ~32 == 0
            length = int(np.flatnonzero(r["done"][:, 0])[q - 1]) + 1
            col = {k: v[:length, 0].copy() for k, v in r.items()}
        else:
            col = dict(states=np.zeros((0, e.H, e.F), np.int8), active=np.zeros(0, np.uint32), p_sel=np.zeros(0, np.float32),
                       actions=np.zeros(0, np.int32), rewards=np.zeros(0, np.float32), done=np.zeros(0, np.uint8))
        col.update(length=length, episode_after=ep + max(q, 1), tick_after=tk + length)
        out[int(n)] = col
    return out


def expected_steps(orc, env_kw, params, hid, L, T, columns, episode, tick, fresh):
    """Column n of the steps form (T steps with auto-reset) that follows an episodes-form call on the same env: an env that
    finished its quota is terminal and is reset (it consumes counter episode[n]); an env that never played (fresh[n]) goes on
    from the state its last reset left, which is the reset of counter episode[n] - 1."""
    out = {}
    for n in columns:
        e = _env(orc, env_kw, 1, n)
        e.episode[0], e.tick[0] = int(episode[n]) - int(bool(fresh[n])), int(tick[n])
        e.reset()
        r = orc.collect_rollouts_tn(e, params, hid, T, mode_dev=True, n_hidden=L)
        out[int(n)] = {k: v[:, 0].copy() for k, v in r.items()}
    return out


def play_column(orc, env_kw, n, params, hid, L, quota, kind="return", episode0=1, tick0=0):
    """The reference's loops written out step by step for one env (the loop of tests/test_gpu_parity.py's
    _oracle_trajectories, over any Q, width and depth): reset!, then sample / step! until terminal, `quota` times.  kind =
    "normalized" takes single_trajectory_normalized_return's early exit: a trajectory that starts at its optimum is not
    played (1.0): it consumes an episode counter and no tick.  Returns dict(actions, p_sel, rewards, done: the played
    transitions in order; values: one per trajectory; skipped: one flag per trajectory; lengths)."""
    seed, goff = int(env_kw["seed"]), int(env_kw.get("global_offset", 0))
    e = _env(orc, env_kw, 1, n)
    e.episode[0], e.tick[0] = episode0, tick0
    acts, psel, rews, dones, values, skipped, lengths = [], [], [], [], [], [], []
    for _ in range(quota):
        e.reset_one(0)
        cur, opt = (int(x[0]) for x in scores(e))
        init, low, maxret, ret, steps = cur, cur, cur - opt, 0.0, 0
        if kind == "normalized" and maxret == 0:
            values.append(1.0)
            skipped.append(True)
            lengths.append(0)
            continue
        while not e.done[0]:
            p = orc.action_probabilities(params, F, hid, e.observe_one(0), e.active[0], "dev", n_hidden=L)
            w = orc.philox([(goff + n) & 0xFFFFFFFF, int(e.tick[0]), 0, 0], [seed & 0xFFFFFFFF, seed >> 32])
            a, err = orc.categorical_sample(p, orc.u01(w[0]))
            if err:                                             # the rounding residue goes to the last unmasked action
                a = int(np.flatnonzero(p > 0)[-1])
            e.step_one(0, a)
            acts.append(a)
            psel.append(p[a])
            rews.append(float(e.reward[0]))
            dones.append(int(e.done[0]))
            ret += float(e.reward[0])
            low = min(low, int(scores(e)[0][0]))
            steps += 1
        best = init - low
        values.append(ret if kind == "return" else (float(best) if kind == "best" else best / maxret))
        skipped.append(False)
        lengths.append(steps)
    assert int(e.err[0]) == 0
    return dict(actions=np.array(acts, np.int32), p_sel=np.array(psel, np.float32), rewards=np.array(rews, np.float32),
                done=np.array(dones, np.uint8), values=values, skipped=skipped, lengths=lengths)


def assemble(exp, N, T, H):
    """[T, N] columns from expected_episodes of every column (host tests: there is no device buffer to take them from)."""
    a = dict(states=np.zeros((T, N, H, F), np.int8), active=np.zeros((T, N), np.uint32), actions=np.zeros((T, N), np.int32),
             p_sel=np.zeros((T, N), np.float32), rewards=np.zeros((T, N), np.float32), done=np.ones((T, N), np.uint8),
             valid=np.zeros((T, N), bool))
    for n, col in exp.items():
        k = col["length"]
        for key in ("states", "active", "actions", "p_sel", "rewards", "done"):
            a[key][:k, n] = col[key]
        a["valid"][:k, n] = True
    return a


# ---------------------------------------------------------------- all columns, teacher-forced
def teacher_forced(orc, env_kw, actions, num_episodes, episode0=None, tick0=None):
    """Replay the oracle env for all N columns with the given 0-based actions [T, N] (the device's).  Only busy envs are
    stepped (quota not used up: rows of the others keep reward 0, done 1, valid 0) and an env is reset on done only while
    episodes of its quota remain.  Integer work only.  Returns states, active, rewards, done, valid [T, ..]; cur_before /
    opt_before / cur_after [T, N] (the scores around each step); episode, tick, fresh [N] as the call leaves them."""
    N = env_kw["num_envs"]
    T = actions.shape[0]
    oenv = _env(orc, env_kw)
    oenv.episode[:] = 1 if episode0 is None else episode0
    if tick0 is not None:
        oenv.tick[:] = tick0
    oenv.reset()
    left = quotas(N, num_episodes)
    fresh = left == 0
    r = dict(states=np.zeros((T, N, oenv.H, oenv.F), np.int8), active=np.zeros((T, N), np.uint32),
             rewards=np.zeros((T, N), np.float32), done=np.ones((T, N), np.uint8), valid=np.zeros((T, N), bool),
             cur_before=np.zeros((T, N), np.int64), opt_before=np.zeros((T, N), np.int64), cur_after=np.zeros((T, N), np.int64))
    for t in range(T):
        busy = left > 0
        if not busy.any():
            break
        r["states"][t][busy] = oenv.observe_all()[busy]
        r["active"][t][busy] = oenv.active[busy]
        r["cur_before"][t], r["opt_before"][t] = scores(oenv)
        for n in np.flatnonzero(busy):
            oenv.step_one(int(n), int(actions[t, n]))
        r["cur_after"][t] = scores(oenv)[0]
        r["rewards"][t][busy] = oenv.reward[busy]
        r["done"][t][busy] = oenv.done[busy]
        r["valid"][t] = busy
        fin = busy & oenv.done.astype(bool)
        left[fin] -= 1
        for n in np.flatnonzero(fin & (left > 0)):
            oenv.reset_one(int(n))
    assert not (left > 0).any(), "the actions do not finish the quotas within T rows"
    assert np.all(oenv.err == 0), "the actions are not moves the oracle env accepts: %s" % np.flatnonzero(oenv.err)[:8]
    r.update(episode=oenv.episode.copy(), tick=oenv.tick.copy(), fresh=fresh)
    return r


def env_major_index(valid):
    """Flat ids t * N + n of the valid transitions in the reference's buffer order: env after env, each in time order."""
    T, N = valid.shape
    ids = (np.arange(T)[None, :] * N + np.arange(N)[:, None])          # [N, T]
    return ids[valid.T]


def flat_returns(orc, rewards, done, index, discount):
    """compute_state_value! over the env-major flat buffer, the reference's own layout (src/rollout_buffer.jl:55-64)."""
    return orc.compute_returns(rewards.reshape(-1)[index], np.asarray(done, np.uint8).reshape(-1)[index], float(discount),
                               isinstance(discount, np.float32))


# ---------------------------------------------------------------- evaluators
def evaluator_values(kind, rec, skip=None):
    """The per-trajectory values of a played record (teacher_forced's), env-major: "return" sums the raw rewards in
    float64, "best" is initial - min(current score), "normalized" is best / (initial - optimum).  skip: {n: values} replaces
    the values of the envs whose "normalized" trajectories are not the played ones (an env that skips one)."""
    T, N = rec["valid"].shape
    out = []
    for n in range(N):
        if skip is not None and n in skip:
            out.extend(skip[n])
            continue
        ret, first = 0.0, True
        for t in np.flatnonzero(rec["valid"][:, n]):
            if first:
                init = low = int(rec["cur_before"][t, n])
                maxret = init - int(rec["opt_before"][t, n])
                first = False
            ret += float(rec["rewards"][t, n])
            low = min(low, int(rec["cur_after"][t, n]))
            if rec["done"][t, n]:
                best = init - low
                out.append(ret if kind == "return" else (float(best) if kind == "best" else
                                                         (1.0 if maxret == 0 else best / maxret)))
                ret, first = 0.0, True
    return np.array(out, np.float64)


def skip_table(orc, env_kw, num_traj):
    """[max quota, N] flags: trajectory j of env n starts at its optimum (the reset of episode counter 1 + j: a skipped
    trajectory consumes a counter like a played one, so this does not depend on the policy)."""
    N = env_kw["num_envs"]
    quota = quotas(N, num_traj)
    tab = np.zeros((int(quota.max()), N), bool)
    oenv = _env(orc, env_kw)
    for j in range(tab.shape[0]):
        oenv.episode[:] = 1 + j
        oenv.reset()
        cur, opt = scores(oenv)
        tab[j] = (cur == opt) & (quota > j)
    return tab


def skipping_envs(orc, case):
    return [int(n) for n in np.flatnonzero(skip_table(orc, env_kw_of(case), case["episodes"]).any(axis=0))]


def normalized_of_skippers(orc, case):
    """{n: values} of the envs that skip a trajectory, from the full oracle replay (policy forward included)."""
    key = ("norm", case["name"])
    if key not in _CACHE:
        kw, quota = env_kw_of(case), quotas(case["N"], case["episodes"])
        _CACHE[key] = {n: play_column(orc, kw, n, policy_params(orc, case), case["hid"], case["L"], int(quota[n]),
                                      "normalized")["values"] for n in skipping_envs(orc, case)}
    return _CACHE[key]


# ---------------------------------------------------------------- which columns get the full oracle forward
def replay_columns(case):
    """env 0; both sides of every multiple of 64 below N (those of 256 among them); the last busy env and the first idle
    one; the last env of the larger quota and the first of the smaller; env N - 1; the envs the case names (a short episode
    or a skip).  Every column up to 70 envs."""
    return list(range(case["N"])) if case["N"] <= 70 else edge_columns(case)


def edge_columns(case):
    """replay_columns without the every-column rule: the columns the calls that follow the first one on the same env
    (a second episodes-form call, then a steps-form call) are replayed at."""
    N, ne = case["N"], case["episodes"]
    cols = {0, N - 1} | set(case["special"])
    for m in range(64, N, 64):
        cols |= {m - 1, m}
    if ne < N:
        cols |= {ne - 1, ne}
    elif ne % N:
        cols |= {ne % N - 1, ne % N}
    return sorted(c for c in cols if 0 <= c < N)


_CACHE = {}


def reference(orc, case):
    """expected_episodes of the case's replayed columns, computed once per process and never modified."""
    key = ("episodes", case["name"])
    if key not in _CACHE:
        _CACHE[key] = expected_episodes(orc, env_kw_of(case), policy_params(orc, case), case["hid"], case["L"],
                                        case["episodes"], replay_columns(case))
    return _CACHE[key]


# ---------------------------------------------------------------- case tables
def _case(name, N, episodes, goff=0, Q=8, hid=128, L=2, M=6, pseed=3, special=(), short=(), forms=("expanded",),
          rollout=True, evaluate=True):
    """goff: global id of env 0.  special: envs that hold a short episode or an evaluator skip.  short: envs whose first
    episode is shorter than max_actions (found with the oracle for this case's policy; the host test re-checks).  forms: the
    storage forms the rollout test runs the case in."""
    return dict(name=name, N=N, episodes=episodes, goff=goff, Q=Q, hid=hid, L=L, M=M, pseed=pseed, special=tuple(special),
                short=tuple(short), forms=tuple(forms), rollout=rollout, evaluate=evaluate)


BOTH = ("expanded", "compact")
# Q = 8 cases put a global id of ON_OPTIMUM (episode counter 1) into the batch: its env plays a short first episode (the
# host test asserts it), in an env of quota >= 2 wherever the case has one (64/64, 130/5 and 600/520 have quotas of 1 only:
# there the short column ends rows before its neighbours).  No Q = 32 id among the first 20,000 resets onto its optimum.
CASES = [
    _case("1x3", 1, 3, goff=107433, special=(0,), short=(0,)),
    _case("64x64", 64, 64, goff=107433 - 37, special=(37,), short=(37,)),
    _case("70x100", 70, 100, goff=107433 - 10, special=(10,), short=(10,), forms=BOTH),
    _case("130x5", 130, 5, goff=107433 - 3, special=(3,), short=(3,)),
    _case("257x515", 257, 515, goff=160637 - 100, special=(100,), short=(100,)),
    _case("300x450-h256", 300, 450, goff=167413 - 120, hid=256, M=4, special=(120,), short=(120,), forms=BOTH),
    _case("600x520", 600, 520, goff=107433 - 515, M=5, special=(515,), short=(515,), evaluate=False),
    _case("q32-20x30", 20, 30, goff=5, Q=32, M=4, forms=BOTH),
    _case("q32-70x100", 70, 100, goff=11, Q=32, M=4, forms=BOTH, evaluate=False),
    _case("L3-40x60", 40, 60, goff=160637 - 7, L=3, M=5, special=(7,), short=(7,)),
    # evaluator only
    _case("200x400", 200, 400, goff=165100, special=(14, 173), rollout=False),     # env 14 skips its second and last
    _case("600x900", 600, 900, goff=107433 - 130, M=5, special=(130,), rollout=False),   # trajectory, env 173 its first of two
    _case("20x60-last", 20, 60, goff=4624 - 7, special=(7,), rollout=False),       # quota 3: env 7 skips its last
    _case("20x60-middle", 20, 60, goff=165114 - 5, special=(5,), rollout=False),   # env 5 skips its second of three
    _case("20x60-first", 20, 60, goff=107433 - 11, special=(11,), rollout=False),  # env 11 skips its first of three
]
ROLLOUT_CASES = [c for c in CASES if c["rollout"]]
ROLLOUT_RUNS = [(c, form) for c in ROLLOUT_CASES for form in c["forms"]]
EVAL_CASES = [c for c in CASES if c["evaluate"]]
BF16_HID = (128, 256)
DOWNSTREAM = "300x450-h256"


def by_name(name):
    return next(c for c in CASES if c["name"] == name)
