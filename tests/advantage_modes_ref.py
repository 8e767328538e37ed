"""Inputs and float64 restatements of the advantage-mode tests (test helper, CPU only).

ppo_train / step_batch take the advantage from one of four columns: "returns", "gae", "returns_normalised" and
"gae_normalised" ((x - mean) / (std + 1e-8) over the minibatch, population std).  tests/test_gpu_advantage_modes.py holds every
train-forward family to them; this module builds that file's inputs without a device, so that
tests/test_advantage_modes_host.py can show on the CPU that the inputs alone have the properties the device cases rest on:

  * the GAE column A and the returns column R differ in sign on at least a quarter of the minibatch (a family that read the
    other column cannot pass), A has both signs on at least a quarter each,
  * the float64 restatement of the probability ratios puts at least B / 20 samples on each side of the clip,
  * in the normaliser cases every sample is clipped, so that the loss term is (1 +- eps) * advantage and the advantage the
    tail consumed can be read back from it.

A is never restated here: ppo_rollouts_compute_gae is held bit for bit to oracle/ppo_oracle.c (test_gpu_parity.py::test_gae),
so the callers pass the oracle's scan (`gae`), and the device test asserts that the device column is that array."""
import functools

import numpy as np

import train_stats_ref as stats_ref
import value_ref
from oracle import np_oracle

EPS, ENT = 0.1, 0.01                  # part 1: ratios lie in 0.8 .. 1.25, so eps = 0.1 clips about a quarter of the samples
GAMMA, LAM = 0.99, 0.95
MARGIN = 0.02                         # no ratio within this of 1 +- eps: no precision decides a sample's side of the clip
NORM_EPS = 0.2                        # part 2: ratios of 2 and 1 / 2, every sample clipped

# family -> knob setup, dtype, F, Q, HID, L, compact storage, states, forward kernel.  The state counts are the smallest that
# select the route and leave a ragged last tile or pass
FAMILIES = {
    "x6-h128": dict(setup={}, dtype="f32", F=72, Q=8, hid=128, L=2, compact=False, B=300, fwd="k_policy_fwd_train_x6<128>"),
    "x6-h256": dict(setup={}, dtype="f32", F=72, Q=8, hid=256, L=2, compact=False, B=300, fwd="k_policy_fwd_train_x6<256>"),
    "x6t-h128": dict(setup={}, dtype="f32", F=72, Q=8, hid=128, L=2, compact=False, B=1025, fwd="k_policy_fwd_train_x6t<128,2>"),
    "x6t-h256": dict(setup={}, dtype="f32", F=72, Q=8, hid=256, L=2, compact=False, B=1537, fwd="k_policy_fwd_train_x6t<256,2>"),
    "x6s": dict(setup={}, dtype="f32", F=72, Q=32, hid=256, L=2, compact=False, B=70, fwd="k_policy_fwd_train_x6s<256,4>"),
    "mode2-q32-h128": dict(setup={}, dtype="f32", F=72, Q=32, hid=128, L=2, compact=False, B=70, fwd="k_policy_fwd<72,128,2,4,0>"),
    "split-4w": dict(setup={"split": 0}, dtype="f32", F=72, Q=8, hid=256, L=2, compact=False, B=256,
                     fwd="k_policy_fwd_train_split<72,256,4,0>"),
    "split-2w": dict(setup={"split": 0}, dtype="f32", F=72, Q=8, hid=256, L=2, compact=False, B=300,
                     fwd="k_policy_fwd_train_split<72,256,2,0>"),
    "mode2": dict(setup={"split": 0}, dtype="f32", F=72, Q=8, hid=256, L=2, compact=False, B=520, fwd="k_policy_fwd<72,256,2,1,0>"),
    "mode2-L3": dict(setup={}, dtype="f32", F=72, Q=8, hid=256, L=3, compact=False, B=300, fwd="k_policy_fwd<72,256,2,1,1>"),
    "mode4": dict(setup={"split": 0, "compact": True}, dtype="f32", F=72, Q=8, hid=256, L=2, compact=True, B=520,
                  fwd="k_policy_fwd<72,256,4,1,0>"),
    # the split-fp32 forward from compact storage: the kernel is named from what ppo_debug_train_route reports
    "x6-compact": dict(setup={"compact": True}, dtype="f32", F=72, Q=8, hid=256, L=2, compact=True, B=300, fwd=None),
    "bf16-h256": dict(setup={}, dtype="bf16", F=72, Q=8, hid=256, L=2, compact=False, B=300, fwd="k_policy_fwd_bf16<72,256,2,1>"),
    "bf16-h128": dict(setup={}, dtype="bf16", F=72, Q=8, hid=128, L=2, compact=False, B=300, fwd="k_policy_fwd_bf16<72,128,2,1>"),
    "tile": dict(setup={"tile": 512}, dtype="f32", F=72, Q=8, hid=256, L=2, compact=False, B=300, fwd="k_policy_train_tile<72,256>"),
    "F216": dict(setup={}, dtype="f32", F=216, Q=8, hid=128, L=2, compact=False, B=100, fwd="k_policy_fwd<216,128,2,1,0>"),
}
# the one engine rollout of the two compact-storage cases (they cannot be loaded through set_columns): Policy(72, 256, 2, 4)
ROLLOUT = dict(N=96, T=8, Q=8, hid=256, max_actions=12, env_seed=8, policy_seed=90, discount=GAMMA, moved=0.01)


def make_params(F, hid, L, seed):
    """Glorot-uniform weights and zero biases in flat Flux order, then moved by N(0, 0.02): no bias is exactly zero."""
    rng = np.random.default_rng(seed)
    parts = []
    for (o, i) in [(hid, F)] + [(hid, hid)] * (L - 1) + [(4, hid)]:
        lim = np.sqrt(6.0 / (o + i))
        parts += [rng.uniform(-lim, lim, size=(o, i)).astype(np.float32).ravel(order="F"), np.zeros(o, np.float32)]
    p = np.concatenate(parts)
    return (p + (rng.normal(size=p.size) * 0.02).astype(np.float32)).astype(np.float32)


def probabilities(params, dtype, F, hid, L, states, active, Q):
    """[B, 16 Q] float64 action probabilities: of the float64 forward, or of the restated bf16 arithmetic for a bf16 policy."""
    if dtype == "bf16":
        return np.concatenate([np_oracle.action_probabilities_bf16(params, F, hid, states[s:s + 512],
                                                                   np_oracle.batch_masks(active[s:s + 512], Q))
                               for s in range(0, len(states), 512)])
    return stats_ref.probabilities(params, F, hid, L, states, active, Q)


def random_states(rng, params, F, hid, L, B, Q, kink=True):
    """B random int8 states [B, 4 Q, F], off leakyrelu's kink where a float64 gradient is compared."""
    parts, have = [], 0
    while have < B:
        cand = rng.integers(-3, 7, size=(B - have + B // 8 + 16, 4 * Q, F)).astype(np.int8)
        if kink:
            cand = cand[value_ref.off_the_kink(params, F, hid, L, cand)]
        parts.append(cand)
        have += len(cand)
    return np.ascontiguousarray(np.concatenate(parts)[:B])


def sample_actions(rng, probs):
    """Inverse CDF on the policy's own probabilities: never a zero-probability action."""
    cdf = np.cumsum(probs, axis=1)
    u = rng.random(len(probs)) * cdf[:, -1]
    a0 = (cdf < u[:, None]).sum(axis=1).astype(np.int32)
    assert np.all(probs[np.arange(len(probs)), a0] > 0)
    return a0


def ratios_off_the_clip(rng, B, eps):
    """B ratios in 0.8 .. 1.25, none within MARGIN of 1 - eps or 1 + eps."""
    r = rng.uniform(0.8, 1.25, B)
    while True:
        bad = (np.abs(r - (1 - eps)) < MARGIN) | (np.abs(r - (1 + eps)) < MARGIN)
        if not bad.any():
            return r
        r[bad] = rng.uniform(0.8, 1.25, int(bad.sum()))


def buffer_shape(B):
    """[2, B / 2], or [1, B] for an odd B."""
    return (2, B // 2) if B % 2 == 0 else (1, B)


def normalise64(x):
    """(x - mean) / (std + 1e-8) in float64, population std, rounded to float32: the minibatch normalisation restated."""
    x = np.asarray(x, np.float32).astype(np.float64)
    return ((x - x.mean()) / (x.std() + 1e-8)).astype(np.float32)


def clip_value(adv, eps):
    """The clip branch of the loss term in float64: (1 + eps) adv for adv >= 0, else (1 - eps) adv."""
    a = np.asarray(adv, np.float32).astype(np.float64)
    return np.where(a >= 0, (1.0 + eps) * a, (1.0 - eps) * a)


def unclipped64(r64, adv, eps):
    return np.asarray(r64, np.float64) * np.asarray(adv, np.float32).astype(np.float64) < clip_value(adv, eps)


def reference_gradient(c, params, cols, adv, eps=EPS, ent=ENT):
    """(gradient, ppo loss, entropy loss) of the minibatch `cols` with the advantages `adv`: float64 autograd, or the restated
    bf16 arithmetic for a bf16 policy.  c: a row of FAMILIES (dtype, F, Q, hid, L)."""
    masks = np_oracle.batch_masks(cols["active"], c["Q"])
    if c["dtype"] == "bf16":
        return np_oracle.step_batch_grad_chunked(np_oracle.step_batch_grad_bf16, params, c["F"], c["hid"], cols["states"], masks,
                                                 cols["a0"], cols["p_old"], adv, eps, ent, chunk=512)
    return np_oracle.step_batch_grad_chunked(np_oracle.step_batch_grad_torch, params, c["F"], c["hid"], cols["states"], masks,
                                             cols["a0"], cols["p_old"], adv, eps, ent, chunk=4096 // c["Q"], n_hidden=c["L"])


# ---------------------------------------------------------------- part 1: one case per train-forward family
@functools.lru_cache(maxsize=None)
def expanded_case(fam):
    """The set_columns dataset of an expanded-storage family, in storage order: parameters, states off the kink, actions drawn
    from the policy's own probabilities, p_old within 0.8 .. 1.25 of them, returns R ~ N(0.3, 1), terminal flags, host state
    values V ~ N(0, 4) for the GAE scan (A is then dominated by V: its sign is nearly independent of R's), and the minibatch
    `sel0`, a permutation of all B states."""
    c = FAMILIES[fam]
    assert not c["compact"]
    seed = 100 + list(FAMILIES).index(fam)
    rng = np.random.default_rng(seed)
    F, Q, hid, L, B = c["F"], c["Q"], c["hid"], c["L"], c["B"]
    params = make_params(F, hid, L, seed)
    states = random_states(rng, params, F, hid, L, B, Q)
    active = rng.integers(1, 2 ** Q, size=B, dtype=np.uint64).astype(np.uint32)
    probs = probabilities(params, c["dtype"], F, hid, L, states, active, Q)
    a0 = sample_actions(rng, probs)
    p_sel = probs[np.arange(B), a0]
    p_old = (p_sel / ratios_off_the_clip(rng, B, EPS)).astype(np.float32)
    T, N = buffer_shape(B)
    return dict(params=params, states=states, active=active, a0=a0, p_old=p_old, p64=p_sel, T=T, N=N,
                R=(0.3 + rng.normal(size=B)).astype(np.float32), terminal=(rng.random((T, N)) < 0.1).astype(np.uint8),
                V=(rng.normal(size=(T + 1, N)) * 2).astype(np.float32), sel0=rng.permutation(B))


def expanded_advantages(d, gae):
    """The GAE column of an expanded_case, flat in storage order.  gae: oracle.gae_tn."""
    return gae(d["R"].reshape(d["T"], d["N"]), d["terminal"], d["V"], GAMMA, LAM)[0].reshape(-1)


def rollout_start():
    """(parameters that collect the engine rollout of the compact-storage families, parameters that train on it)."""
    r = ROLLOUT
    p0 = make_params(72, r["hid"], 2, r["policy_seed"])
    moved = (p0 + (np.random.default_rng(r["policy_seed"] + 1).normal(size=p0.size) * r["moved"]).astype(np.float32)).astype(np.float32)
    return p0, moved


def trainable_pool(c, params, states, active, a0, p_old, eps=EPS):
    """Engine states share many rows and few are off the kink: the positions that are, under the training parameters, and
    whose float64 ratio is not within 1e-3 of 1 +- eps (no precision decides a sample's side of the clip); and the float64
    probability of every state's action."""
    n = len(states)
    p64 = probabilities(params, c["dtype"], c["F"], c["hid"], c["L"], states, active, c["Q"])[np.arange(n), a0]
    r64 = p64 / p_old.astype(np.float64)
    clear = (np.abs(r64 - (1 - eps)) > 1e-3) & (np.abs(r64 - (1 + eps)) > 1e-3)
    pool = np.flatnonzero(value_ref.off_the_kink(params, c["F"], c["hid"], c["L"], states) & clear)
    assert len(pool) >= 64, len(pool)
    return pool, p64


def compact_case(fam, params, states, active, a0, p_old, R):
    """The minibatch of a compact-storage family on an engine rollout (columns flat in transition order): host state values
    for the GAE scan, and B positions drawn from the states that are off the kink under the training parameters (engine
    states share many rows, few are; with replacement if need be)."""
    c = FAMILIES[fam]
    rng = np.random.default_rng(200 + list(FAMILIES).index(fam))
    n = len(states)
    assert n == ROLLOUT["N"] * ROLLOUT["T"] and (c["F"], c["hid"], c["L"], c["Q"]) == (72, ROLLOUT["hid"], 2, ROLLOUT["Q"])
    V = (rng.normal(size=(ROLLOUT["T"] + 1, ROLLOUT["N"])) * 20).astype(np.float32)  # the engine's returns reach -25
    pool, p64 = trainable_pool(c, params, states, active, a0, p_old)
    sel0 = rng.choice(pool, size=c["B"], replace=len(pool) < c["B"])
    return dict(params=params, states=states, active=active, a0=a0, p_old=p_old, R=R, V=V, sel0=sel0, p64=p64)


def minibatch(d):
    """The minibatch columns of a case, in minibatch order, as the references take them."""
    s = d["sel0"]
    return dict(states=d["states"][s], active=d["active"][s], a0=d["a0"][s], p_old=d["p_old"][s])


def family_conditions(d, A, eps=EPS):
    """What a part-1 case rests on, judged on the float64 restatement alone.  A: the GAE column, flat in storage order.
    -> the counts, after asserting them."""
    s = d["sel0"]
    B = len(s)
    a, r = A[s].astype(np.float64), d["R"][s].astype(np.float64)
    r64 = d["p64"][s] / d["p_old"][s].astype(np.float64)
    un = unclipped64(r64, A[s], eps)
    got = dict(B=B, sign_differs=int((a * r < 0).sum()), positive=int((a > 0).sum()), negative=int((a < 0).sum()),
               unclipped=int(un.sum()), clipped=int((~un).sum()))
    assert 4 * got["sign_differs"] >= B, got
    assert 4 * got["positive"] >= B and 4 * got["negative"] >= B, got
    assert 20 * got["unclipped"] >= B and 20 * got["clipped"] >= B, got
    assert np.all(np.abs(r64 - (1 - eps)) > 1e-3) and np.all(np.abs(r64 - (1 + eps)) > 1e-3), got
    return got


# ---------------------------------------------------------------- part 2: the normaliser at every width
NORM_F, NORM_HID, NORM_L, NORM_Q = 72, 128, 2, 8
NORM_KERNEL = "k_policy_fwd_train_x6<128>"
# case -> (states in the dataset, minibatch size, column the mode normalises, contents)
NORMALISER = {
    "B1": (1, 1, "returns", "normal"), "B2": (2, 2, "returns", "normal"), "B1023": (1023, 1023, "returns", "normal"),
    "B1024": (1024, 1024, "returns", "normal"), "B1025": (1025, 1025, "returns", "normal"),
    "B2048": (2048, 2048, "returns", "normal"), "B4096": (4096, 4096, "returns", "normal"),
    "B5000": (5000, 5000, "returns", "normal"),
    "constant-1025": (1025, 1025, "returns", "constant"),
    "large-mean-2048": (2048, 2048, "returns", "large-mean"),
    "repeats-1500": (2000, 1500, "returns", "normal"),           # drawn with replacement from 2000 states (B <= num_data)
    "gae-1025": (1025, 1025, "gae", "normal"), "gae-4096": (4096, 4096, "gae", "normal"),
}


@functools.lru_cache(maxsize=None)
def normaliser_dataset(name):
    """The dataset of a normaliser case but for p_old, which depends on the column the mode normalises (normaliser_case)."""
    n, B, col, contents = NORMALISER[name]
    seed = 300 + list(NORMALISER).index(name)
    rng = np.random.default_rng(seed)
    params = make_params(NORM_F, NORM_HID, NORM_L, 7)
    states = random_states(rng, params, NORM_F, NORM_HID, NORM_L, n, NORM_Q, kink=False)
    active = rng.integers(1, 2 ** NORM_Q, size=n, dtype=np.uint64).astype(np.uint32)
    probs = probabilities(params, "f32", NORM_F, NORM_HID, NORM_L, states, active, NORM_Q)
    a0 = sample_actions(rng, probs)
    if contents == "constant":
        R = np.full(n, 0.7, np.float32)
    elif contents == "large-mean":
        R = (1000 + 0.01 * rng.normal(size=n)).astype(np.float32)
    else:
        R = (0.3 + rng.normal(size=n)).astype(np.float32)
    T, N = buffer_shape(n)
    sel0 = rng.integers(0, n, size=B) if B != n else rng.permutation(n)
    return dict(params=params, states=states, active=active, a0=a0, p64=probs[np.arange(n), a0], R=R, T=T, N=N,
                terminal=(rng.random((T, N)) < 0.1).astype(np.uint8), V=(rng.normal(size=(T + 1, N)) * 2).astype(np.float32),
                sel0=sel0)


def normaliser_case(name, gae=None):
    """A normaliser case complete: p_old = p / 2 where the normalised column lies above the mean of the B gathered entries and
    2 p where it lies below, so that with eps = 0.2 every sample is clipped and the loss term is (1 +- eps) * advantage.
    -> the dataset with p_old, the column x (flat, storage order) and want = normalise64(x[sel0])."""
    d = dict(normaliser_dataset(name))
    x = d["R"] if NORMALISER[name][2] == "returns" else expanded_advantages(d, gae)
    xs = x[d["sel0"]].astype(np.float64)
    mean = xs.mean()
    side = np.ones(len(x))
    side[d["sel0"]] = np.where(xs > mean, 0.5, 2.0)                  # a repeated state gets one value: its x is one value
    d.update(x=x, p_old=(d["p64"] * side).astype(np.float32), want=normalise64(x[d["sel0"]]), mean=mean)
    return d


def all_clipped64(d, eps=NORM_EPS):
    """Number of samples of a normaliser case the float64 restatement leaves UNclipped (the cap is zero)."""
    s = d["sel0"]
    r64 = d["p64"][s] / d["p_old"][s].astype(np.float64)
    return int(unclipped64(r64, d["want"], eps).sum())


def advantage_from_term(term, eps=NORM_EPS):
    """The float32 advantage behind a clipped loss term (1 +- eps) * double(adv), and the term re-formed from it.  The
    quotient is within 2^-52 relative of adv, which is a float32: rounding to float32 returns adv itself."""
    t = np.asarray(term, np.float64)
    adv = np.where(t >= 0, t / (1.0 + eps), t / (1.0 - eps)).astype(np.float32)
    return adv, clip_value(adv, eps)


def ulp_distance(a, b):
    """|a - b| in float32 ulps, through the ordered-integer view of the two arrays."""
    def ordered(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


# ---------------------------------------------------------------- part 3: the epoch loop
LOOP = dict(n=2500, batch=1100, epochs=2, hid=128, eta=1e-3, eps=0.2, ent=0.01, seed=11)


@functools.lru_cache(maxsize=None)
def loop_dataset():
    """2500 states in a [2, 1250] buffer: minibatches of 1100, 1100 and 300 per epoch (the normaliser runs beyond its 1024
    threads, the short last one on another train-forward kernel)."""
    c = LOOP
    rng = np.random.default_rng(400)
    n = c["n"]
    params = make_params(NORM_F, c["hid"], 2, 9)
    states = random_states(rng, params, NORM_F, c["hid"], 2, n, NORM_Q, kink=False)
    active = rng.integers(1, 2 ** NORM_Q, size=n, dtype=np.uint64).astype(np.uint32)
    probs = probabilities(params, "f32", NORM_F, c["hid"], 2, states, active, NORM_Q)
    a0 = sample_actions(rng, probs)
    p_old = (probs[np.arange(n), a0] / rng.uniform(0.8, 1.25, n)).astype(np.float32)
    T, N = buffer_shape(n)
    return dict(params=params, states=states, active=active, a0=a0, p_old=p_old, R=(0.3 + rng.normal(size=n)).astype(np.float32),
                T=T, N=N, terminal=(rng.random((T, N)) < 0.1).astype(np.uint8), V=(rng.normal(size=(T + 1, N)) * 2).astype(np.float32),
                perm=np.stack([rng.permutation(n) for _ in range(c["epochs"])]))
