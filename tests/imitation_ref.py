"""Float64 restatement of the imitation (behaviour-cloning) objective (test helper, CPU only; does not import the engine):

    logits l [B, 4H] of the Policy(F, hidden, L, 4) MLP (action k = 4 * row + output), masked to the rows of ACTIVE quads,
    logp_b = log_softmax(l_b)[a_b],   w_b = max(weight_b, 0),
    cross-entropy = -(1 / B_global) sum_b w_b logp_b,
    entropy term  = entropy_weight (1 / B_global) sum_b sum_k sp log sp,   sp = p + 1e-8 / A  (ppo_loss_with_entropy's).

torch float64 autograd gives the gradient and dL/dlogits; the analytic dL/dlogits is restated beside it so a test can hold one
against the other.  Flat parameters are in Flux order (value_ref.unpack)."""
import numpy as np

import value_ref
from value_ref import off_the_kink, row_mask, unpack  # noqa: F401  (re-exported for the tests)

SMOOTH = 1e-8


def action_mask(active, H):
    """[B, 4H] bool: action k lies on row k // 4."""
    return np.repeat(row_mask(active, H), 4, axis=1)


def logits_np(params, F, hid, L, states, dtype=np.float64):
    """Plain numpy forward in `dtype` -> logits [B, 4H]."""
    y = value_ref.forward_np(params, F, hid, L, states, dtype)
    return y.reshape(y.shape[0], -1)


def log_probs_np(logits, mask, dtype=np.float64):
    """Masked log-softmax in `dtype`, the log-softmax form (l - m) - log(sum exp(l - m)) -> (logp [B, A] with -inf on masked
    actions, p [B, A] with 0 there)."""
    l = np.asarray(logits, dtype)
    m = np.where(mask, l, dtype(-np.inf)).max(axis=1, keepdims=True)
    e = np.where(mask, np.exp(np.where(mask, l - m, dtype(0))), dtype(0)).astype(dtype)
    S = e.sum(axis=1, keepdims=True, dtype=dtype)
    logp = np.where(mask, (l - m) - np.log(S), dtype(-np.inf)).astype(dtype)
    return logp, (e / S).astype(dtype)


def per_state_terms(logits, active, actions, weights, H, dtype=np.float64):
    """What the device leaves per state: (w logp [B], -sum_k sp log sp [B]) in `dtype`."""
    mask = action_mask(active, H)
    logp, p = log_probs_np(logits, mask, dtype)
    B, A = p.shape
    w = np.maximum(np.asarray(weights, dtype), dtype(0))
    sp = p + dtype(SMOOTH) / dtype(A)
    hl = (sp * np.log(sp)).sum(axis=1, dtype=dtype)
    return (w * logp[np.arange(B), np.asarray(actions)]).astype(dtype), (-hl).astype(dtype)


def losses_np(logits, active, actions, weights, H, entropy_weight=0.0, B_global=None, dtype=np.float64):
    """(cross-entropy, entropy_weight * entropy loss) with every operation in `dtype`."""
    t0, t1 = per_state_terms(logits, active, actions, weights, H, dtype)
    Bg = dtype(len(t0) if B_global is None else B_global)
    return float(-(t0.sum(dtype=dtype) / Bg)), float(dtype(entropy_weight) * -(t1.sum(dtype=dtype) / Bg))


def analytic_dy(logits, active, actions, weights, H, entropy_weight=0.0, B_global=None):
    """dL/dlogits [B, H, 4] in float64: (w / Bg)(p_k - [k == a]) + p_k (dpe_k - sum_j p_j dpe_j), dpe_k = (ew / Bg)(log sp_k + 1);
    exactly 0 on the rows of inactive quads."""
    mask = action_mask(active, H)
    _, p = log_probs_np(logits, mask)
    B, A = p.shape
    Bg = float(B if B_global is None else B_global)
    w = np.maximum(np.asarray(weights, np.float64), 0.0)
    onehot = np.zeros_like(p)
    onehot[np.arange(B), np.asarray(actions)] = 1.0
    dpe = (entropy_weight / Bg) * (np.log(p + SMOOTH / A) + 1.0)
    dot = (p * dpe).sum(axis=1, keepdims=True)
    return ((w / Bg)[:, None] * (p - onehot) + p * (dpe - dot)).reshape(B, H, 4)


def _torch_logits(tl, states, keep=False):
    import torch
    a = torch.tensor(np.asarray(states), dtype=torch.float64)
    for (W, b) in tl[:-1]:
        a = torch.nn.functional.leaky_relu(a @ W.T + b, 0.01)
    W, b = tl[-1]
    y = a @ W.T + b                                                     # [B, H, 4]
    if keep:
        y.retain_grad()
    return y


def loss_grad(params, F, hid, L, states, active, actions, weights, entropy_weight=0.0, B_global=None, chunk=2048, want_dy=False):
    """float64 autograd of the objective over the minibatch, built chunk by chunk (it is a sum over states) ->
    (cross-entropy, entropy_weight * entropy loss, flat gradient in Flux order, logp [B]) and, with want_dy, dL/dlogits [B, H, 4]."""
    import torch
    B, H = len(states), states.shape[1]
    Bg = float(B if B_global is None else B_global)
    tl = value_ref._torch_layers(params, F, hid, L)
    ce, ent, lps, dys = 0.0, 0.0, [], []
    for s in range(0, B, chunk):
        y = _torch_logits(tl, states[s:s + chunk], keep=want_dy)
        n = y.shape[0]
        mask = torch.tensor(action_mask(active[s:s + chunk], H))
        l = torch.where(mask, y.reshape(n, -1), torch.full((), -float("inf"), dtype=torch.float64))
        logp = torch.log_softmax(l, dim=1)
        lp = logp[torch.arange(n), torch.tensor(np.asarray(actions[s:s + chunk], np.int64))]
        w = torch.tensor(np.maximum(np.asarray(weights[s:s + chunk], np.float64), 0.0))
        part_ce = -(w * lp).sum() / Bg
        sp = torch.softmax(l, dim=1) + SMOOTH / l.shape[1]
        part_ent = entropy_weight * (sp * torch.log(sp)).sum() / Bg
        (part_ce + part_ent).backward()
        ce += float(part_ce.detach())
        ent += float(part_ent.detach())
        lps.append(lp.detach().numpy())
        if want_dy:
            dys.append(y.grad.numpy().copy())
    g = []
    for (W, b) in tl:
        g.append(W.grad.numpy().ravel(order="F"))
        g.append(b.grad.numpy())
    out = (ce, ent, np.concatenate(g), np.concatenate(lps))
    return out + (np.concatenate(dys),) if want_dy else out


def adam_schedule(params, F, hid, L, states, active, actions, weights, batch, perms, entropy_weight=0.0, eta=1e-3,
                  beta=(0.9, 0.999), eps=1e-8):
    """imitate_train_'s schedule in float64: per epoch the permutation perms[ep] (0-based), consecutive slices of `batch`
    (short last one), Flux.Adam on each slice's gradient -> (per-epoch mean of the per-batch cross-entropies, final params)."""
    p = np.asarray(params, np.float64).copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    bp = [beta[0], beta[1]]
    hist = []
    for perm in perms:
        losses = []
        for s in range(0, len(perm), batch):
            sel = np.asarray(perm[s:s + batch])
            ce, _, g, _ = loss_grad(p, F, hid, L, states[sel], active[sel], actions[sel], weights[sel], entropy_weight)
            losses.append(ce)
            m = beta[0] * m + (1 - beta[0]) * g
            v = beta[1] * v + (1 - beta[1]) * g * g
            p = p - m / (1 - bp[0]) / (np.sqrt(v / (1 - bp[1])) + eps) * eta
            bp = [bp[0] * beta[0], bp[1] * beta[1]]
        hist.append(float(np.mean(losses)))
    return hist, p
