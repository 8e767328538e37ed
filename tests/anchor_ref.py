"""Float64 restatement of the KL-anchored PPO objective (test helper, CPU only; does not import the engine).  For a minibatch of
B states of B_global, logits l [B, 4H], the stored action a, its probability p_old at collection time, the advantage adv, the
clip range eps, a target row q [B, 4H] per state and the coefficient beta:

    surrogate term  s    = min(p_a / p_old * adv, clip),  clip = (1 + eps) adv for adv >= 0, (1 - eps) adv below
                           (simplified_ppo_clip; a tie counts as clipped, as the device's `gain < clip` does)
    anchor          ce   = sum_k q'_k logp_k               (distill_ref: q' = q on the rows of active quads, 0 elsewhere;
                                                            logp the log-softmax form; a term with q'_k == 0 is exactly 0)
    per state       t0   = s + beta ce,   t1 = -sum_k sp log sp          (what the device leaves in loss_terms)
    loss column 0        = -(1 / B_global) sum_b t0_b  =  surrogate loss + beta * cross-entropy
    entropy term         = entropy_weight (1 / B_global) sum_b sum_k sp log sp
    divergence      kl   = sum over q'_k > 0 of q'_k (log q'_k - logp_k)  (KL(q' || pi) for a normalised row; no 1 / B_global)
    dL/dlogit_k          = (beta / B_global)(p_k Qs - q'_k) + p_k (dp_k - sum_j p_j dp_j),
                           dp_k = (entropy_weight / B_global)(log sp_k + 1) - [k == a][unclipped] adv / (B_global p_old)

torch float64 autograd gives the gradient and dL/dlogits; the analytic dL/dlogits is restated beside it.  dtype=np.float32 runs
the forward, the softmax, the sums, the entropy and the divergence in float32 (what sets the loss bar).  adapt_coef is the
coefficient rule of the epoch loop."""
import numpy as np

import imitation_ref
import value_ref
from distill_ref import kept_targets
from imitation_ref import SMOOTH, action_mask, log_probs_np, logits_np  # noqa: F401  (re-exported for the tests)
from value_ref import off_the_kink, row_mask, unpack  # noqa: F401


def clip_value(adv, eps):
    adv = np.asarray(adv, np.float64)
    return np.where(adv >= 0, (1.0 + eps) * adv, (1.0 - eps) * adv)


def surrogate(p_sel, p_old, adv, eps, dtype=np.float64):
    """(min(gain, clip) [B] in float64, unclipped [B]): gain = p_sel / p_old * adv formed in `dtype`, the clip and the
    comparison in float64 as the device forms them."""
    gain = (np.asarray(p_sel, dtype) / np.asarray(p_old, dtype) * np.asarray(adv, dtype)).astype(np.float64)
    clip = clip_value(adv, eps)
    un = gain < clip
    return np.where(un, gain, clip), un


def state_kl(logits, active, targets, H, dtype=np.float64):
    """kl [B] in `dtype`: sum over q'_k > 0 of q'_k (log q'_k - logp_k)."""
    logp, _ = log_probs_np(logits, action_mask(active, H), dtype)
    q = kept_targets(targets, active, H, dtype)
    pos = q > 0
    safe_q = np.where(pos, q, dtype(1))
    return np.where(pos, q * (np.log(safe_q) - np.where(pos, logp, dtype(0))), dtype(0)).sum(axis=1, dtype=dtype).astype(dtype)


def per_state_terms(logits, active, actions, p_old, adv, eps, targets, coef, H, dtype=np.float64):
    """What the device leaves per state: (s + beta ce [B], -sum sp log sp [B], ratio p_a / p_old [B], kl [B]); the sum
    s + beta ce in float64 of a float32 product when dtype is float32, as the device forms it."""
    mask = action_mask(active, H)
    logp, p = log_probs_np(logits, mask, dtype)
    B, A = p.shape
    ps = p[np.arange(B), np.asarray(actions)]
    s, _ = surrogate(ps, p_old, adv, eps, dtype)
    q = kept_targets(targets, active, H, dtype)
    ce = np.where(q == 0, dtype(0), q * np.where(q == 0, dtype(0), logp)).sum(axis=1, dtype=dtype)
    sp = p + dtype(SMOOTH) / dtype(A)
    hl = (sp * np.log(sp)).sum(axis=1, dtype=dtype)
    t0 = s + (dtype(coef) * ce).astype(np.float64)
    return t0, (-hl).astype(np.float64), (ps / np.asarray(p_old, dtype)).astype(dtype), state_kl(logits, active, targets, H, dtype)


def analytic_dy(logits, active, actions, p_old, adv, eps, targets, coef, H, entropy_weight=0.0, B_global=None):
    """dL/dlogits [B, H, 4] in float64; exactly 0 on the rows of inactive quads."""
    mask = action_mask(active, H)
    _, p = log_probs_np(logits, mask)
    B, A = p.shape
    Bg = float(B if B_global is None else B_global)
    a = np.asarray(actions)
    _, un = surrogate(p[np.arange(B), a], p_old, adv, eps)
    q = kept_targets(targets, active, H)
    Qs = q.sum(axis=1, keepdims=True)
    dp = (entropy_weight / Bg) * (np.log(p + SMOOTH / A) + 1.0)
    dp[np.arange(B), a] += np.where(un, -(np.asarray(adv, np.float64) / np.asarray(p_old, np.float64)) / Bg, 0.0)
    dot = (p * dp).sum(axis=1, keepdims=True)
    return ((coef / Bg) * (p * Qs - q) + p * (dp - dot)).reshape(B, H, 4)


def loss_grad(params, F, hid, L, states, active, actions, p_old, adv, eps, targets, coef, entropy_weight=0.0, B_global=None,
              chunk=2048, want_dy=False):
    """float64 autograd of the objective over the minibatch, built chunk by chunk -> dict(loss = column 0, surrogate, ce,
    entropy = entropy_weight * entropy loss, grad = flat gradient in Flux order, kl [B], ratio [B]) and, with want_dy,
    dy = dL/dlogits [B, H, 4]."""
    import torch
    B, H = len(states), states.shape[1]
    Bg = float(B if B_global is None else B_global)
    tl = value_ref._torch_layers(params, F, hid, L)
    qall = kept_targets(targets, active, H)
    actions, p_old, adv = np.asarray(actions), np.asarray(p_old, np.float64), np.asarray(adv, np.float64)
    sur, ce, ent, dys, kls, ratios = 0.0, 0.0, 0.0, [], [], []
    zero = torch.zeros((), dtype=torch.float64)
    for s in range(0, B, chunk):
        y = imitation_ref._torch_logits(tl, states[s:s + chunk], keep=want_dy)
        n = y.shape[0]
        mask = torch.tensor(action_mask(active[s:s + chunk], H))
        l = torch.where(mask, y.reshape(n, -1), torch.full((), -float("inf"), dtype=torch.float64))
        logp = torch.log_softmax(l, dim=1)
        prob = torch.softmax(l, dim=1)
        ps = prob[torch.arange(n), torch.tensor(actions[s:s + chunk])]
        ad, po = torch.tensor(adv[s:s + chunk]), torch.tensor(p_old[s:s + chunk])
        gain = ps / po * ad
        clip = torch.tensor(clip_value(adv[s:s + chunk], eps))
        part_sur = -torch.where(gain < clip, gain, clip).sum() / Bg
        q = torch.tensor(qall[s:s + chunk])
        cs = torch.where(q == 0, zero, q * torch.where(q == 0, zero, logp)).sum(dim=1)
        part_ce = -cs.sum() / Bg
        sp = prob + SMOOTH / l.shape[1]
        part_ent = entropy_weight * (sp * torch.log(sp)).sum() / Bg
        (part_sur + coef * part_ce + part_ent).backward()
        sur += float(part_sur.detach())
        ce += float(part_ce.detach())
        ent += float(part_ent.detach())
        one = torch.ones((), dtype=torch.float64)
        kls.append(torch.where(q > 0, q * (torch.log(torch.where(q > 0, q, one)) - torch.where(q > 0, logp, zero)), zero)
                   .sum(dim=1).detach().numpy())
        ratios.append((ps / po).detach().numpy())
        if want_dy:
            dys.append(y.grad.numpy().copy())
    g = []
    for (W, b) in tl:
        g.append(W.grad.numpy().ravel(order="F"))
        g.append(b.grad.numpy())
    out = dict(loss=sur + coef * ce, surrogate=sur, ce=ce, entropy=ent, grad=np.concatenate(g), kl=np.concatenate(kls),
               ratio=np.concatenate(ratios))
    if want_dy:
        out["dy"] = np.concatenate(dys)
    return out


def adapt_coef(coef, mean_kl, target):
    """PPO's rule (Schulman et al. 2017, section 4) behind an epoch: target 0 keeps the coefficient; a mean divergence above
    1.5 target doubles it, one below target / 1.5 halves it."""
    if target > 0:
        if mean_kl > 1.5 * target:
            return coef * 2.0
        if mean_kl < target / 1.5:
            return coef / 2.0
    return coef


def adam_schedule(params, F, hid, L, states, active, actions, p_old, adv, eps, targets, coef, batch, perms, target=0.0,
                  entropy_weight=0.0, eta=1e-3, beta=(0.9, 0.999), adam_eps=1e-8, shards=None):
    """ppo_train_'s schedule with the anchor in float64: per epoch the permutation perms[ep] (0-based), consecutive slices of
    `batch` (short last one), Flux.Adam on each slice's gradient, the coefficient rule behind every epoch ->
    dict(hist = per-epoch mean of the per-batch loss column 0, kl = per-epoch mean divergence (each state under the parameters
    its own minibatch saw), coef = the coefficient every epoch ran with, approx_kl, old_approx_kl = kl_stats of the epoch's
    ratios, params, final_coef).  shards / perms as in distill_ref.adam_schedule: the divergence is then the union's."""
    p = np.asarray(params, np.float64).copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    bp = [beta[0], beta[1]]
    out = dict(hist=[], kl=[], coef=[], approx_kl=[], old_approx_kl=[])
    targets = np.asarray(targets).reshape(len(states), -1)
    for perm in perms:
        losses, kls, ratios = [], [], []
        if shards is None:
            steps = [np.asarray(perm[s:s + batch]) for s in range(0, len(perm), batch)]
        else:
            nb = max(-(-(hi - lo) // batch) for lo, hi in shards)
            steps = [np.concatenate([lo + np.asarray(pr[b * batch:(b + 1) * batch], np.int64) for (lo, hi), pr in zip(shards, perm)])
                     for b in range(nb)]
        for sel in steps:
            r = loss_grad(p, F, hid, L, states[sel], active[sel], actions[sel], p_old[sel], adv[sel], eps, targets[sel], coef,
                          entropy_weight)
            losses.append(r["loss"])
            kls.append(r["kl"])
            ratios.append(r["ratio"])
            g = r["grad"]
            m = beta[0] * m + (1 - beta[0]) * g
            v = beta[1] * v + (1 - beta[1]) * g * g
            p = p - m / (1 - bp[0]) / (np.sqrt(v / (1 - bp[1])) + adam_eps) * eta
            bp = [bp[0] * beta[0], bp[1] * beta[1]]
        mean_kl = float(np.concatenate(kls).mean())
        rr = np.concatenate(ratios)
        out["hist"].append(float(np.mean(losses)))
        out["kl"].append(mean_kl)
        out["coef"].append(coef)
        out["approx_kl"].append(float(((rr - 1.0) - np.log(rr)).mean()))
        out["old_approx_kl"].append(float((-np.log(rr)).mean()))
        coef = adapt_coef(coef, mean_kl, target)
    out["params"], out["final_coef"] = p, coef
    return out
