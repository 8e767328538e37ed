"""Float64 restatements for the time-limit bootstrap: the GAE recurrence with a bootstrap column in plain
numpy, and the replay of a stored transition on the CPU oracle env -- which `done` transitions were time limits, and the
state each of them cut its episode in."""
import numpy as np


def gae_boot(rewards, done, values, boot, gamma, lam):
    """adv, ret [T,N] float32.  All float64, latest row first, one IEEE operation per statement:
        dn = done[t]; nd = dn ? 0 : 1; v = V[t]
        vnext = dn ? boot[t] : vn
        gvn = gamma * vnext; delta = (r[t] + gvn) - v
        carry = (gamma*lambda * nd) * a; a = delta + carry
        adv[t] = f32(a); ret[t] = f32(a + v); vn = v"""
    r = np.asarray(rewards, np.float32).astype(np.float64)
    d = np.asarray(done).astype(bool)
    V = np.asarray(values, np.float32).astype(np.float64)
    b = np.asarray(boot, np.float32).astype(np.float64)
    T, N = r.shape
    assert d.shape == (T, N) and b.shape == (T, N) and V.shape == (T + 1, N)
    gamma, gl = float(gamma), float(gamma) * float(lam)
    adv, ret = np.empty((T, N), np.float32), np.empty((T, N), np.float32)
    a = np.zeros(N, np.float64)
    vn = V[T].copy()
    for t in range(T - 1, -1, -1):
        nd = np.where(d[t], 0.0, 1.0)
        v = V[t]
        vnext = np.where(d[t], b[t], vn)
        gvn = gamma * vnext
        delta = (r[t] + gvn) - v
        carry = (gl * nd) * a
        a = delta + carry
        adv[t] = a.astype(np.float32)
        ret[t] = (a + v).astype(np.float32)
        vn = v
    return adv, ret


def gae_plain(rewards, done, values, gamma, lam):
    return gae_boot(rewards, done, values, np.zeros(np.shape(rewards), np.float32), gamma, lam)


def state_from_observation(obs, active):
    """(score[V], degree[V]) from observation rows [H, F]: env_template(Q, h, 0) == h, so feature 0 / 36 of row v is
    score[v] / degree[v] whenever quad v >> 2 is active; an inactive quad's vertices are 0 / 0."""
    obs = np.asarray(obs, np.int8)
    V = obs.shape[0]
    on = ((int(active) >> (np.arange(V) >> 2)) & 1).astype(bool)
    return np.where(on, obs[:, 0], 0).astype(np.int8), np.where(on, obs[:, 36], 0).astype(np.int8)


class Replay:
    """One oracle env (slot 0 of an oracle.Env with a time limit that never fires) to replay stored transitions on."""

    def __init__(self, orc, Q):
        self.env = orc.Env(Q=Q, max_actions=2 ** 30, N=1, seed=0)
        self.env.reset()
        self.Q = Q

    def step(self, score, degree, active, action0):
        """-> (truncated, observation [H,F] int8, active word, reward) of the state behind step!(env, action0)."""
        e = self.env
        e.score[0, :] = score
        e.degree[0, :] = degree
        e.active[0] = active
        e.steps[0] = 0
        e.done[0] = 0
        e.step_one(0, int(action0))
        act = int(e.active[0])
        on = ((act >> (np.arange(4 * self.Q) >> 2)) & 1).astype(bool)
        sc = e.score[0].astype(np.int64)[on]
        terminated = int(np.abs(sc).sum()) == abs(int(sc.sum()))
        return (not terminated), e.observe_one(0).copy(), np.uint32(act), float(e.reward[0])


def replay_buffer(orc, Q, states, active, actions0, ends):
    """states [T,N,H,F], active / actions0 / ends [T,N] (ends = done & valid).  -> flags [T,N] bool, final observations [K,H,F]
    and active words [K] of the truncated transitions in ascending transition id."""
    rp = Replay(orc, Q)
    T, N = ends.shape
    flags = np.zeros((T, N), bool)
    obs, act = [], []
    for t in range(T):
        for n in range(N):
            if not ends[t, n]:
                continue
            sc, dg = state_from_observation(states[t, n], active[t, n])
            tr, o, a, _ = rp.step(sc, dg, active[t, n], actions0[t, n])
            flags[t, n] = tr
            if tr:
                obs.append(o)
                act.append(a)
    H, F = states.shape[2], states.shape[3]
    return flags, (np.stack(obs) if obs else np.zeros((0, H, F), np.int8)), np.asarray(act, np.uint32)


def crafted_states(orc, extra):
    """The Q = 8 recipe: active = 0x3F, degree 4 on vertices 0..23, scores 0 but score[0] = score[1] = -1 and score[3] =
    score[4] = +1: action 0 gives reward 4 and reaches the optimum.  extra: score[8] = +1, score[9] = -1 on top, and the
    same action does not.  -> (observation [32,72], active word, score, degree)"""
    sc, dg = np.zeros(32, np.int8), np.zeros(32, np.int8)
    dg[:24] = 4
    sc[0] = sc[1] = -1
    sc[3] = sc[4] = 1
    if extra:
        sc[8], sc[9] = 1, -1
    rp = Replay(orc, 8)
    e = rp.env
    e.score[0, :] = sc
    e.degree[0, :] = dg
    e.active[0] = 0x3F
    return e.observe_one(0).copy(), np.uint32(0x3F), sc, dg
