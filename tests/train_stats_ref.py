"""Float64 restatement of the update statistics (test helper, CPU only).

Per epoch of ppo_train, over the probability ratios r = p_new(a|s) / p_old(a|s) of every transition, each taken with the
parameters its own minibatch saw (before that minibatch's update):

    old_approx_kl = mean(-log r)      approx_kl = mean((r - 1) - log r)      clip_fraction = mean(|r - 1| > eps)

and, for the critic, the five shifted sums behind the explained variance 1 - Var(t - V) / Var(t).  The run itself is restated
with the float64 gradient of oracle/np_oracle.py (torch autograd) and its Adam, the way tests/value_ref.py restates the
critic's schedule."""
import numpy as np

from oracle import np_oracle


def probabilities(params, F, hid, L, states, active, Q, chunk=1024):
    """Masked-softmax action probabilities [B, 16 Q] in float64 (numpy), states [B, H, F] int8, active [B] quad bit sets."""
    layers = np_oracle.unpack_params(params, F, hid, L)
    out = []
    for s in range(0, len(states), chunk):
        a = np.asarray(states[s:s + chunk]).astype(np.float64)
        for (W, b) in layers[:-1]:
            z = a @ W.astype(np.float64).T + b.astype(np.float64)
            a = np.where(z > 0, z, 0.01 * z)
        W, b = layers[-1]
        y = a @ W.astype(np.float64).T + b.astype(np.float64)              # [B, H, 4]
        l = y.reshape(len(y), -1) + np_oracle.batch_masks(active[s:s + chunk], Q).astype(np.float64)
        l = l - l.max(axis=1, keepdims=True)
        e = np.exp(l)
        out.append(e / e.sum(axis=1, keepdims=True))
    return np.concatenate(out)


def logits_max(params, F, hid, L, states, active, Q, chunk=1024):
    """max |logit| over the unmasked actions of every state [B], float64 (the scale of the forward's logit-space bar)."""
    layers = np_oracle.unpack_params(params, F, hid, L)
    out = []
    for s in range(0, len(states), chunk):
        a = np.asarray(states[s:s + chunk]).astype(np.float64)
        for (W, b) in layers[:-1]:
            z = a @ W.astype(np.float64).T + b.astype(np.float64)
            a = np.where(z > 0, z, 0.01 * z)
        W, b = layers[-1]
        y = np.abs(a @ W.astype(np.float64).T + b.astype(np.float64)).reshape(len(a), -1)
        on = np.isfinite(np_oracle.batch_masks(active[s:s + chunk], Q))
        out.append(np.where(on, y, 0.0).max(axis=1))
    return np.concatenate(out)


def ratios(params, F, hid, L, states, active, Q, a0, p_old):
    """float64 p_new(a|s) / p_old(a|s), p_old the recorded float32 probability."""
    p = probabilities(params, F, hid, L, states, active, Q)
    return p[np.arange(len(p)), np.asarray(a0, np.int64)] / np.asarray(p_old, np.float64)


def ratio_sums(r, eps):
    """(sum(-log r), sum((r - 1) - log r), count(|r - 1| > eps), n) in float64."""
    r = np.asarray(r).astype(np.float64).reshape(-1)
    lg = np.log(r)
    return float(np.sum(-lg)), float(np.sum((r - 1.0) - lg)), int(np.count_nonzero(np.abs(r - 1.0) > eps)), r.size


def sum_bound(r):
    """The derived bound of a fixed-order fp64 reduction against numpy's, for the two log sums of `r` (float32 ratios):
    2^-52 * sum(|r_i - 1| + |log r_i|)  (one fp64 log per term, rounded differently by two libraries, and the term's own
    rounding)  +  n * 2^-53 * sum|term_i|  (n additions in any two orders).  Returns (bound for sum(-log r), for sum((r-1)-log r))."""
    r = np.asarray(r).astype(np.float64).reshape(-1)
    lg = np.log(r)
    per_term = 2.0 ** -52 * float(np.sum(np.abs(r - 1.0) + np.abs(lg)))
    n = r.size
    return (per_term + n * 2.0 ** -53 * float(np.sum(np.abs(lg))),
            per_term + n * 2.0 ** -53 * float(np.sum(np.abs((r - 1.0) - lg))))


def restated_run(params, F, hid, L, cols, perms, batch, eps, ent, eta):
    """ppo_train's schedule with Adam(eta) restated: per epoch the permutation perms[ep] (0-based), consecutive slices of
    `batch` (short last one), the float64 gradient of each slice, np_oracle's Adam on it; the ratios of a slice are taken
    in float64 with the parameters the slice saw.  cols: dict of states [n, H, F], active, a0, p_old, adv, Q.
    -> (per-epoch approx_kl, per-epoch clip_fraction, final parameters)."""
    p = np.asarray(params, np.float32).copy()
    m, v, bp = np.zeros_like(p), np.zeros_like(p), np.array([0.9, 0.999])
    Q = cols["Q"]
    kls, clips = [], []
    for perm in perms:
        rs = []
        for s in range(0, len(perm), batch):
            sel = np.asarray(perm[s:s + batch])
            st, ac, a0, po, ad = (cols[k][sel] for k in ("states", "active", "a0", "p_old", "adv"))
            rs.append(ratios(p, F, hid, L, st, ac, Q, a0, po))
            g, _, _ = np_oracle.step_batch_grad_torch(p, F, hid, st, np_oracle.batch_masks(ac, Q), a0, po, ad, eps, ent, n_hidden=L)
            p, m, v, bp = np_oracle.adam_step(p, g, m, v, bp, eta=eta)
        s1, s3, c, n = ratio_sums(np.concatenate(rs), eps)
        kls.append(s3 / n)
        clips.append(c / n)
    return kls, clips, p


def first_rise(k, last=4):
    """The first epoch j in 1..last with k[j] > max(k[:j]), or None."""
    for j in range(1, min(last, len(k) - 1) + 1):
        if k[j] > max(k[:j]):
            return j
    return None


def value_moments(t, v, valid, i0):
    """(n, sum x, sum x^2, sum y, sum y^2) over the valid transitions in float64, x = t - t[i0], y = (t - v) - (t - v)[i0];
    t, v, valid flat in storage order.  Also the per-sum magnitudes sum|x| ... for a summation bound."""
    t, v = np.asarray(t).astype(np.float64).reshape(-1), np.asarray(v).astype(np.float64).reshape(-1)
    on = np.asarray(valid).reshape(-1) != 0
    x = (t - t[i0])[on]
    y = ((t - v) - (t[i0] - v[i0]))[on]
    sums = np.array([x.size, x.sum(), (x * x).sum(), y.sum(), (y * y).sum()], np.float64)
    mags = np.array([0.0, np.abs(x).sum(), (x * x).sum(), np.abs(y).sum(), (y * y).sum()], np.float64)
    return sums, mags


# ---- the one seeded setup of the early-stopping tests (host: restated on the CPU rollout; device: on the one it collected)
# The clip range is wide on purpose.  Adam(3e-4) moves every parameter by about eta per step, so with the usual 0.05 .. 0.2
# the ratios reach the clip range within epoch 0, approx_kl settles near eps^2 / 2 and later epochs only fluctuate around it
# (restated: 0.0020, 0.0016, 0.0015, ... at 0.05; 0.023, 0.022, 0.013, ... at 0.2).  At 0.5 the policy is still moving away
# in the second epoch (0.097 then 0.18), which is what a test of a stop "after the first epoch that exceeds the target" needs.
EARLY = dict(N=512, T=16, Q=8, max_actions=12, env_seed=7, policy_seed=1, F=72, HID=128, L=2, eta=3e-4, batch=1024, epochs=6,
             eps=0.5, ent=0.01, discount=0.99, perm_seed=20)


def early_perms(n, cfg=EARLY):
    """[epochs, n] 0-based permutations of the setup."""
    rng = np.random.default_rng(cfg["perm_seed"])
    return np.stack([rng.permutation(n) for _ in range(cfg["epochs"])])
