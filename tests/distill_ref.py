"""Float64 restatement of the distillation (soft-target cross-entropy) objective (test helper, CPU only; does not import the
engine).  For a minibatch of B states of B_global, logits l [B, 4H] of the Policy(F, hidden, L, 4) MLP (action k = 4 * row +
output) and a target row q [B, 4H] per state:

    q'_k   = q_k on the rows of ACTIVE quads, 0 elsewhere            (mass on inactive rows is ignored)
    Qs     = sum_k q'_k                                              (used as it is, not assumed 1)
    logp_k = (l_k - m) - log S,  m and S the masked softmax's         (the log-softmax form, never log(p_k))
    ce     = sum_k q'_k logp_k                                       (a term with q'_k == 0 is exactly 0)
    w      = 1 | max(weight, 0)
    cross-entropy = -(1 / B_global) sum_b w_b ce_b
    entropy term  = entropy_weight (1 / B_global) sum_b sum_k sp log sp,   sp = p + 1e-8 / A  (ppo_loss_with_entropy's)
    dL/dlogit_k   = (w / B_global)(p_k Qs - q'_k) + p_k (dpe_k - sum_j p_j dpe_j),  dpe_k = (entropy_weight / B_global)(log sp_k + 1)

torch float64 autograd gives the gradient and dL/dlogits; the analytic dL/dlogits is restated beside it so a test can hold one
against the other.  dtype=np.float32 runs the forward, the log-softmax, the sums and the entropy in float32 (what sets
LOSS_BAR).  Flat parameters are in Flux order (value_ref.unpack)."""
import numpy as np

import imitation_ref
import value_ref
from imitation_ref import SMOOTH, action_mask, log_probs_np, logits_np  # noqa: F401  (re-exported for the tests)
from value_ref import off_the_kink, row_mask, unpack  # noqa: F401


def kept_targets(targets, active, H, dtype=np.float64):
    """q' [B, 4H]: the target rows with the actions of inactive quads zeroed."""
    q = np.asarray(targets, dtype).reshape(len(active), -1)
    return np.where(action_mask(active, H), q, dtype(0)).astype(dtype)


def per_state_terms(logits, active, targets, weights, H, dtype=np.float64):
    """What the device leaves per state: (w ce [B], -sum_k sp log sp [B]) in `dtype`."""
    mask = action_mask(active, H)
    logp, p = log_probs_np(logits, mask, dtype)
    B, A = p.shape
    q = kept_targets(targets, active, H, dtype)
    w = np.maximum(np.asarray(weights, dtype), dtype(0))
    ce = np.where(q == 0, dtype(0), q * np.where(q == 0, dtype(0), logp)).sum(axis=1, dtype=dtype)
    sp = p + dtype(SMOOTH) / dtype(A)
    hl = (sp * np.log(sp)).sum(axis=1, dtype=dtype)
    return (w * ce).astype(dtype), (-hl).astype(dtype)


def losses_np(logits, active, targets, weights, H, entropy_weight=0.0, B_global=None, dtype=np.float64):
    """(cross-entropy, entropy_weight * entropy loss) with every operation in `dtype`."""
    t0, t1 = per_state_terms(logits, active, targets, weights, H, dtype)
    Bg = dtype(len(t0) if B_global is None else B_global)
    return float(-(t0.sum(dtype=dtype) / Bg)), float(dtype(entropy_weight) * -(t1.sum(dtype=dtype) / Bg))


def target_entropy(targets, active, weights, H, B_global=None):
    """The floor of the cross-entropy of normalised rows: (1 / B_global) sum_b w_b (-sum_k q'_k log q'_k), float64."""
    q = kept_targets(targets, active, H)
    w = np.maximum(np.asarray(weights, np.float64), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        h = -np.where(q == 0, 0.0, q * np.log(q)).sum(axis=1)
    return float((w * h).sum() / (len(q) if B_global is None else B_global))


def analytic_dy(logits, active, targets, weights, H, entropy_weight=0.0, B_global=None):
    """dL/dlogits [B, H, 4] in float64: (w / Bg)(p_k Qs - q'_k) + p_k (dpe_k - sum_j p_j dpe_j); exactly 0 on the rows of
    inactive quads."""
    mask = action_mask(active, H)
    _, p = log_probs_np(logits, mask)
    B, A = p.shape
    Bg = float(B if B_global is None else B_global)
    q = kept_targets(targets, active, H)
    Qs = q.sum(axis=1, keepdims=True)
    w = np.maximum(np.asarray(weights, np.float64), 0.0)
    dpe = (entropy_weight / Bg) * (np.log(p + SMOOTH / A) + 1.0)
    dot = (p * dpe).sum(axis=1, keepdims=True)
    return ((w / Bg)[:, None] * (p * Qs - q) + p * (dpe - dot)).reshape(B, H, 4)


def loss_grad(params, F, hid, L, states, active, targets, weights, entropy_weight=0.0, B_global=None, chunk=2048, want_dy=False):
    """float64 autograd of the objective over the minibatch, built chunk by chunk (it is a sum over states) ->
    (cross-entropy, entropy_weight * entropy loss, flat gradient in Flux order) and, with want_dy, dL/dlogits [B, H, 4]."""
    import torch
    B, H = len(states), states.shape[1]
    Bg = float(B if B_global is None else B_global)
    tl = value_ref._torch_layers(params, F, hid, L)
    qall = kept_targets(targets, active, H)
    ce, ent, dys = 0.0, 0.0, []
    for s in range(0, B, chunk):
        y = imitation_ref._torch_logits(tl, states[s:s + chunk], keep=want_dy)
        n = y.shape[0]
        mask = torch.tensor(action_mask(active[s:s + chunk], H))
        l = torch.where(mask, y.reshape(n, -1), torch.full((), -float("inf"), dtype=torch.float64))
        logp = torch.log_softmax(l, dim=1)
        q = torch.tensor(qall[s:s + chunk])
        w = torch.tensor(np.maximum(np.asarray(weights[s:s + chunk], np.float64), 0.0))
        zero = torch.zeros((), dtype=torch.float64)
        cs = torch.where(q == 0, zero, q * torch.where(q == 0, zero, logp)).sum(dim=1)
        part_ce = -(w * cs).sum() / Bg
        sp = torch.softmax(l, dim=1) + SMOOTH / l.shape[1]
        part_ent = entropy_weight * (sp * torch.log(sp)).sum() / Bg
        (part_ce + part_ent).backward()
        ce += float(part_ce.detach())
        ent += float(part_ent.detach())
        if want_dy:
            dys.append(y.grad.numpy().copy())
    g = []
    for (W, b) in tl:
        g.append(W.grad.numpy().ravel(order="F"))
        g.append(b.grad.numpy())
    out = (ce, ent, np.concatenate(g))
    return out + (np.concatenate(dys),) if want_dy else out


def adam_schedule(params, F, hid, L, states, active, targets, weights, batch, perms, entropy_weight=0.0, eta=1e-3,
                  beta=(0.9, 0.999), eps=1e-8, shards=None):
    """distill_train_'s schedule in float64: per epoch the permutation perms[ep] (0-based), consecutive slices of `batch`
    (short last one), Flux.Adam on each slice's gradient -> (per-epoch mean of the per-batch cross-entropies, final params).
    shards: a list of (lo, hi) index ranges, one per data-parallel rank, perms then a list (per epoch) of one permutation per
    shard: step b takes slice b of every shard (an exhausted shard gives nothing), the gradient is the mean over their union."""
    p = np.asarray(params, np.float64).copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    bp = [beta[0], beta[1]]
    hist = []
    targets = np.asarray(targets).reshape(len(states), -1)
    for perm in perms:
        losses = []
        if shards is None:
            steps = [np.asarray(perm[s:s + batch]) for s in range(0, len(perm), batch)]
        else:
            nb = max(-(-(hi - lo) // batch) for lo, hi in shards)
            steps = [np.concatenate([lo + np.asarray(pr[b * batch:(b + 1) * batch], np.int64) for (lo, hi), pr in zip(shards, perm)])
                     for b in range(nb)]
        for sel in steps:
            ce, _, g = loss_grad(p, F, hid, L, states[sel], active[sel], targets[sel], weights[sel], entropy_weight)
            losses.append(ce)
            m = beta[0] * m + (1 - beta[0]) * g
            v = beta[1] * v + (1 - beta[1]) * g * g
            p = p - m / (1 - bp[0]) / (np.sqrt(v / (1 - bp[1])) + eps) * eta
            bp = [bp[0] * beta[0], bp[1] * beta[1]]
        hist.append(float(np.mean(losses)))
    return hist, p
