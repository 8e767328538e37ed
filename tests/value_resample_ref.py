"""Host reference of the resampling search that ranks by the critic's value (search_resample_states_(critic=...), DESIGN.md
7j).  Everything here comes from the CPU oracle (oracle/oracle.py), numpy, tests/episodes_ref.py, tests/search_ref.py,
tests/resample_ref.py and tests/path_ref.py, never from the device; none of those is changed.

The rule.  An event is 7h's fold -> rank -> copy; only the rank key of a live clone changes:

    s = fmaf(-w, v, (float)cur_gap)  in fp32,   w = (float)value_weight,   v = V(state the clone holds), 0.0 if not finite
    key = ord(s) << 32 | clone,      ord(x) = ~bits(x) if the sign bit of x is set, else bits(x) | 0x80000000

ord is the usual monotone map of fp32 bits to uint32; it orders -0.0 before +0.0.  score() computes s with ONE rounding (an
exact rational sum rounded to the nearest fp32, ties to even), which is what fmaf does; no double rounding through float64.

Device values are not bit-predictable on the CPU (the pooling order; tests/test_gpu_value.py bounds them against float64
instead), so a replay that computed its own values could not decide a close ranking.  The replay therefore takes the values
of every event from outside (`values_of`): the device test feeds it the device's own log and then checks the log itself, bit
for bit, against the critic's forward of the states the replay holds at that event (the `events` list keeps them).  The
host test feeds it value_ref.values_np(..., float32) of a stand-in critic.

The shape table of tests/test_value_resample_host.py and tests/test_gpu_value_resample.py lives at the end of the file."""
from fractions import Fraction

import numpy as np

import episodes_ref as ref
import path_ref as pref
import resample_ref as rref

F32_MAX = Fraction(int(np.finfo(np.float32).max))


# ---------------------------------------------------------------- the rule
def ord32(x):
    """The monotone map of fp32 bits to uint32 (array or scalar in, same shape out)."""
    b = np.asarray(x, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def round_f32(q):
    """The fp32 nearest to the rational q, ties to even, overflow to inf; an exact zero is +0.0 (a sum of a product and
    (float)cur_gap >= +0.0 that cancels is +0.0 under round-to-nearest)."""
    if q == 0:
        return np.float32(0.0)
    if abs(q) >= F32_MAX + Fraction(2) ** 103:                   # half an ulp above the largest finite fp32
        return np.float32(np.inf if q > 0 else -np.inf)
    c = np.float32(float(q))                                     # a double rounding at worst one ulp off: look at the neighbours
    cands = [c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))]
    cands = [x for x in cands if np.isfinite(x)]

    def key(x):
        return (abs(Fraction(float(x)) - q), int(np.float32(x).view(np.uint32)) & 1)
    return np.float32(min(cands, key=key))


def score(cur_gap, v, w):
    """s of one live clone: fmaf(-w, v, (float)cur_gap) with one rounding; v not finite counts as 0.0."""
    v = np.float32(v)
    if not np.isfinite(v):
        v = np.float32(0.0)
    w = np.float32(w)
    assert np.isfinite(w) and w >= 0 and 0 <= int(cur_gap) < 2 ** 24
    return round_f32(-Fraction(float(w)) * Fraction(float(v)) + int(cur_gap))


def rank_live_value(cur_gap, values, done, m0, w):
    """rref.rank_live with the key (ord(s), clone).  Returns (order, m, donor_of, s) -- s [K] float32, NaN for a terminal
    clone."""
    K = len(done)
    s = np.full(K, np.nan, np.float32)
    for c in range(K):
        if not done[c]:
            s[c] = score(cur_gap[c], values[c], w)
    o = ord32(s)
    order = sorted((c for c in range(K) if not done[c]), key=lambda c: (int(o[c]), c))
    m = min(m0, len(order))
    return order, m, {order[rho]: order[(rho - m) % m] for rho in range(m, len(order))}, s


# ---------------------------------------------------------------- the replay
def value_resample_replay(orc, env_kw, params, hid, L, starts, K, R, m0, w, values_of):
    """path_ref.resample_paths' loop (fold by the record's real best_gap, histories, fresh ticks) with the rank above.
    values_of(start, event, states [K, H, F] int8, active [K] uint32, done [K]) -> [K] values of that start's clones at that
    event (entries of terminal clones are ignored).  Returns resample_paths' arrays (best_state, best_active, best_gap,
    best_step, initial_gap, best_clone, fold_event, copies, path, donors, clone_gaps, tick) plus played [N] bool and `events`:
    one dict per (start, event) that ran with start, event, cur_gap, done, values (as given), s, order, m, donor_of, states,
    active, and gap_survivors / survivors: the sets (cur_gap, clone) and the rule keep."""
    N, T = env_kw["num_envs"], env_kw["max_actions"]
    M = starts[2].shape[0]
    S, E = N // K, (T - 1) // R
    tick = np.zeros(N, np.int64)
    played = np.zeros(N, bool)
    donors = np.full((M, E, K), -2, np.int32)
    clone_gaps = np.zeros((M, K), np.int32)
    results, events = [None] * M, []

    def fold(rd, s, base, ev):
        old = results[base + s]
        new = rref.fold_into(old, rd.recs[s * K:(s + 1) * K])
        if new is not old:
            new.update(fold_event=ev, copies=rd.copies[s * K + new["best_clone"]])
        results[base + s] = new

    for base in range(0, M, S):
        Sr = min(S, M - base)
        rd = pref.PathRound(orc, env_kw, params, hid, L, starts, base, Sr, K, tick)
        played[:Sr * K] = True
        while rd.t < T and rd.live().size:
            rd.step()
            if rd.t % R == 0 and rd.t < T:
                ev = rd.t // R - 1
                obs = rd.env.observe_all()                       # the states behind the step, before any copy of the event
                act = np.asarray(rd.env.active).astype(np.uint32).copy()
                for s in range(Sr):
                    fold(rd, s, base, ev)
                    sl = slice(s * K, (s + 1) * K)
                    done = [int(x) for x in rd.env.done[sl]]
                    cur = rd.cur_gaps(s)
                    vals = np.asarray(values_of(base + s, ev, obs[sl], act[sl], done), np.float32)
                    order, m, donor_of, sc = rank_live_value(cur, vals, done, m0, w)
                    gap_order, gm, _ = rref.rank_live(cur, done, m0)
                    events.append(dict(start=base + s, event=ev, t=rd.t, cur_gap=cur, done=done, values=vals.copy(), s=sc,
                                       order=order, m=m, donor_of=dict(donor_of), states=obs[sl].copy(), active=act[sl].copy(),
                                       survivors=set(order[:m]), gap_survivors=set(gap_order[:gm])))
                    for c in range(K):
                        donors[base + s, ev, c] = -2 if done[c] else donor_of.get(c, -1)
                    for c, d in donor_of.items():
                        rd.copy(s, c, d)
        assert not rd.live().size
        for s in range(Sr):
            fold(rd, s, base, -1)
            clone_gaps[base + s] = [r["best_gap"] for r in rd.recs[s * K:(s + 1) * K]]
        tick[:Sr * K] = rd.env.tick
    out = dict(best_state=np.stack([r["best_state"] for r in results]).astype(np.int8),
               best_active=np.array([r["best_active"] for r in results], np.uint32))
    for k in ("best_gap", "best_step", "initial_gap", "best_clone", "fold_event", "copies"):
        out[k] = np.array([r[k] for r in results], np.int32)
    out.update(path=pref.padded([r["path"] for r in results], T), donors=donors, clone_gaps=clone_gaps, tick=tick, played=played,
               events=events)
    return out


# ---------------------------------------------------------------- what the events of a replay contain
def differs_from_gap_ranking(ev):
    """The survivor set is not the one (cur_gap, clone) would keep."""
    return ev["survivors"] != ev["gap_survivors"]


def keeps_a_higher_gap(ev):
    """A survivor whose cur_gap is strictly higher than a discarded (live) clone's."""
    o, m = ev["order"], ev["m"]
    return len(o) > m >= 1 and max(ev["cur_gap"][c] for c in o[:m]) > min(ev["cur_gap"][c] for c in o[m:])


def terminal_among_live(ev):
    return rref.terminal_among_live(ev)


# ---------------------------------------------------------------- shapes
# (starts, K clones, N envs, max_actions, R interval, survivors) taken from resample_ref.SHAPES, the env's Q, the critic
# (hidden, layers), its seed and value_weight.  The policy is resample_ref's (hid 128, two hidden layers, seed 3), env seed 13,
# fresh ticks.  A critic of hidden width 64 runs zero-padded on the 128 kernel; Q = 32 is four tiles per state.  The critics are
# untrained (values of a few tenths that differ by hundredths from clone to clone), so a weight of 64 lets the value overrule
# gap differences of one or two; shape B keeps 8, under which the gap still leads clones to the optimum: terminal clones.
SHAPES = {
    "A": dict(shape=(4, 12, 48, 24, 2, 3), Q=8, critic=(64, 2), cseed=11, w=64.0),
    "B": dict(shape=(6, 8, 48, 20, 1, 2), Q=8, critic=(64, 2), cseed=16, w=8.0),          # terminal clones beside live ones
    "C": dict(shape=(5, 13, 70, 8, 2, 3), Q=8, critic=(256, 2), cseed=12, w=64.0),        # five idle envs
    "D": dict(shape=(7, 8, 20, 12, 2, 2), Q=8, critic=(128, 3), cseed=13, w=64.0),        # four rounds, the last one ragged
    "E": dict(shape=(1, 257, 300, 6, 2, 32), Q=8, critic=(256, 2), cseed=14, w=64.0),     # K beyond one pass of the workgroup
    "Q32": dict(shape=(3, 6, 20, 6, 2, 2), Q=32, critic=(64, 2), cseed=15, w=64.0),       # four tiles of the value forward
}
POLICY = dict(hid=rref.CASE["hid"], L=rref.CASE["L"], pseed=rref.CASE["pseed"])
START_OFFSET = 5000              # search_ref.START_OFFSET: the starts are the reset states of the envs of these global ids on


def env_kw(name):
    c = SHAPES[name]
    return dict(num_envs=c["shape"][2], Q=c["Q"], max_actions=c["shape"][3], seed=ref.SEED, global_offset=0)


def starts(orc, name):
    """search_ref.search_starts at the shape's Q: the reset states (episode counter 1) of M envs."""
    c = SHAPES[name]
    e = orc.Env(Q=c["Q"], max_actions=c["shape"][3], N=c["shape"][0], seed=ref.SEED, global_offset=START_OFFSET)
    e.episode[:] = 1
    e.reset()
    return e.score.copy(), e.degree.copy(), e.active.copy().astype(np.uint32)


def policy_params(orc):
    return orc.glorot_params(ref.F, POLICY["hid"], POLICY["L"], seed=POLICY["pseed"])


def _critic_params(orc, hid, L, seed):
    p = orc.glorot_params(ref.F, hid, L, seed=seed).astype(np.float32)
    rng = np.random.default_rng(seed)
    return (p + (rng.normal(size=p.size) * 0.03).astype(np.float32)).astype(np.float32)


def critic_params(orc, name):
    """Glorot weights with small random biases: values of order one that differ from state to state."""
    hid, L = SHAPES[name]["critic"]
    return _critic_params(orc, hid, L, SHAPES[name]["cseed"])


NON_FINITE = dict(critic=(128, 2), cseed=17, inf_feature=51, nan_feature=63, threshold=6)


def non_finite_critic_params(orc):
    """A critic (hidden 128, no zero padding on the device) whose values are +inf, NaN or finite depending on the state.
    Features 51 and 63 are template DEGREES (>= 0); about half the states of shape A have a row where one of them reaches 6
    (the host test asserts that both kinds of state occur).  Unit 0 of layer 1 sees feature 51 alone, times 0.6e38: a
    degree of 6 overflows to +inf, 5 gives 3e38.  Every unit k of layer 2 takes it times 2e-38 sign(W3[0, k]), and the rows
    of W3 share their signs, so a +inf there reaches all four outputs as +inf and the pooled value is +inf; a finite row
    moves by a few units at most.  Unit 1 does the same for feature 63 with alternating signs in layer 2: infinities of both
    signs meet and the value is NaN."""
    import value_ref
    hid, L = NON_FINITE["critic"]
    p = _critic_params(orc, hid, L, NON_FINITE["cseed"])
    (W1, b1), (W2, b2), (W3, b3) = value_ref.unpack(p, ref.F, hid, L)        # views into p
    sgn = np.where(W3[0] < 0, -1.0, 1.0).astype(np.float32)
    W3[:] = np.abs(W3) * sgn[None, :]
    big = np.float32(3.4e38 / (NON_FINITE["threshold"] - 0.4))               # threshold x big overflows, (threshold - 1) x big does not
    for unit, f, signs in ((0, NON_FINITE["inf_feature"], sgn),
                           (1, NON_FINITE["nan_feature"], np.where(np.arange(hid) % 2, -1.0, 1.0).astype(np.float32))):
        W1[unit, :], b1[unit] = 0.0, 0.0
        W1[unit, f] = big
        W2[:, unit] = np.float32(2e-38) * signs
    return p


def replay(orc, name, values_of, w=None):
    c = SHAPES[name]
    M, K, N, T, R, m0 = c["shape"]
    return value_resample_replay(orc, env_kw(name), policy_params(orc), POLICY["hid"], POLICY["L"], starts(orc, name), K, R, m0,
                                 c["w"] if w is None else w, values_of)


def host_values(orc, name):
    """The stand-in critic of the host test: value_ref.values_np in float32 on the shape's critic parameters."""
    import value_ref
    hid, L = SHAPES[name]["critic"]
    p = critic_params(orc, name)
    return lambda start, ev, states, active, done: value_ref.values_np(p, ref.F, hid, L, states, active, np.float32)


def host_reference(orc, name):
    """replay with the stand-in critic, once per process and never modified."""
    key = ("value-resample-host", name)
    if key not in ref._CACHE:
        ref._CACHE[key] = replay(orc, name, host_values(orc, name))
    return ref._CACHE[key]
