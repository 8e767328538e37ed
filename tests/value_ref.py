"""Float64 restatement of the critic (test helper, CPU only): the Policy(F, hidden, L, 4) MLP read as a state value,

    V(s) = (sum over rows r of ACTIVE quads, outputs i = 0..3, of y[r][i]) / (4 * number of active rows),   0 without one,

trained with Flux.mse(V, target) = sum_b (V_b - target_b)^2 / B_global.  torch float64 autograd gives the gradient; the
analytic dL/dy is restated beside it so a test can hold one against the other.  Flat parameters are in Flux order
(W [out, in] column-major, then b, per layer)."""
import numpy as np


def unpack(params, F, hid, L):
    p = np.asarray(params)
    out, o = [], 0
    for (no, ni) in [(hid, F)] + [(hid, hid)] * (L - 1) + [(4, hid)]:
        W = p[o:o + no * ni].reshape((no, ni), order="F")
        o += no * ni
        out.append((W, p[o:o + no]))
        o += no
    assert o == p.size
    return out


def row_mask(active, H):
    """[B, H] bool: row r belongs to quad r // 4, active when bit r // 4 of the state's mask is set."""
    bits = np.atleast_1d(np.asarray(active, np.uint32)).astype(np.uint64)
    return ((bits[:, None] >> (np.arange(H, dtype=np.uint64) // 4)[None, :]) & 1).astype(bool)


def pool(y, active):
    """numpy float64 pooling of outputs y [B, H, 4] -> V [B]."""
    y = np.asarray(y, np.float64)
    on = row_mask(active, y.shape[1])
    n = 4 * on.sum(axis=1)
    tot = (y * on[:, :, None]).sum(axis=(1, 2))
    return np.where(n > 0, tot / np.maximum(n, 1), 0.0)


def forward_np(params, F, hid, L, states, dtype=np.float64):
    """Plain numpy forward in `dtype` -> outputs [B, H, 4] (float32: what a host-side critic without the engine computes)."""
    a = np.asarray(states).astype(dtype)
    layers = unpack(params, F, hid, L)
    for (W, b) in layers[:-1]:
        z = a @ W.astype(dtype).T + b.astype(dtype)
        a = np.where(z > 0, z, dtype(0.01) * z)
    W, b = layers[-1]
    return a @ W.astype(dtype).T + b.astype(dtype)


def values_np(params, F, hid, L, states, active, dtype=np.float64, chunk=1024):
    """V [B] with forward and pooling in `dtype`."""
    out = []
    for s in range(0, len(states), chunk):
        y = forward_np(params, F, hid, L, states[s:s + chunk], dtype)
        on = row_mask(active[s:s + chunk], y.shape[1])
        n = 4 * on.sum(axis=1)
        tot = np.where(on[:, :, None], y, dtype(0)).sum(axis=(1, 2), dtype=dtype)
        out.append(np.where(n > 0, tot / np.maximum(n, 1).astype(dtype), dtype(0)).astype(dtype))
    return np.concatenate(out)


def analytic_dy(values, active, targets, B_global, H):
    """dL/dy [B, H, 4] of the mse: 2 (V - target) / (B_global * 4 * n_active_rows) on active rows, 0 elsewhere."""
    on = row_mask(active, H)
    n = 4.0 * on.sum(axis=1)
    g = np.where(n > 0, 2.0 * (np.asarray(values, np.float64) - np.asarray(targets, np.float64)) / (B_global * np.maximum(n, 1)), 0.0)
    return np.broadcast_to((g[:, None] * on)[:, :, None], on.shape + (4,)).copy()


def _torch_layers(params, F, hid, L):
    import torch
    return [(torch.tensor(np.asarray(W, np.float64), requires_grad=True), torch.tensor(np.asarray(b, np.float64), requires_grad=True))
            for (W, b) in unpack(params, F, hid, L)]


def _torch_values(tl, states, active, keep_y=False):
    import torch
    a = torch.tensor(np.asarray(states), dtype=torch.float64)
    for (W, b) in tl[:-1]:
        a = torch.nn.functional.leaky_relu(a @ W.T + b, 0.01)
    W, b = tl[-1]
    y = a @ W.T + b                                                     # [B, H, 4]
    if keep_y:
        y.retain_grad()
    on = torch.tensor(row_mask(active, y.shape[1]))
    n = 4 * on.sum(dim=1)
    tot = (y * on[:, :, None]).sum(dim=(1, 2))
    v = torch.where(n > 0, tot / torch.clamp(n, min=1), torch.zeros_like(tot))
    return v, y


def loss_grad(params, F, hid, L, states, active, targets, B_global=None, chunk=2048, want_dy=False):
    """float64 autograd of sum_b (V_b - t_b)^2 / B_global over the minibatch, built chunk by chunk (the loss is a sum over
    states) -> (loss, flat gradient in Flux order, V [B]) and, with want_dy, dL/dy [B, H, 4] from autograd."""
    import torch
    B = len(states)
    Bg = float(B if B_global is None else B_global)
    tl = _torch_layers(params, F, hid, L)
    loss, vals, dys = 0.0, [], []
    for s in range(0, B, chunk):
        v, y = _torch_values(tl, states[s:s + chunk], active[s:s + chunk], keep_y=want_dy)
        t = torch.tensor(np.asarray(targets[s:s + chunk], np.float64))
        part = ((v - t) ** 2).sum() / Bg
        part.backward()
        loss += float(part.detach())
        vals.append(v.detach().numpy())
        if want_dy:
            dys.append(y.grad.numpy().copy())
    g = []
    for (W, b) in tl:
        g.append(W.grad.numpy().ravel(order="F"))
        g.append(b.grad.numpy())
    out = (loss, np.concatenate(g), np.concatenate(vals))
    return out + (np.concatenate(dys),) if want_dy else out


def off_the_kink(params, F, hid, L, states, delta=1e-5):
    """True per state when no hidden pre-activation of any row lies within `delta` of leakyrelu's kink: there fp32 and
    float64 can disagree about the sign, the derivative jumps 100x, and ANY two precisions differ in a whole gradient row."""
    B, H = states.shape[:2]
    ok = np.ones(B, bool)
    layers = unpack(params, F, hid, L)[:-1]
    for s in range(0, B, 256):
        a = states[s:s + 256].reshape(-1, F).astype(np.float64)
        n = a.shape[0] // H
        for (W, b) in layers:
            z = a @ W.astype(np.float64).T + b.astype(np.float64)
            ok[s:s + n] &= np.abs(z).min(axis=1).reshape(n, H).min(axis=1) >= delta
            a = np.where(z > 0, z, 0.01 * z)
    return ok


def adam_schedule(params, F, hid, L, states, active, targets, batch, perms, eta=1e-3, beta=(0.9, 0.999), eps=1e-8):
    """value_train_'s schedule in float64: per epoch the permutation perms[ep] (0-based), consecutive slices of `batch`
    (short last one), Flux.Adam on each slice's mse gradient -> (per-epoch mean of the per-batch losses, final params)."""
    p = np.asarray(params, np.float64).copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    bp = [beta[0], beta[1]]
    hist = []
    for perm in perms:
        losses = []
        for s in range(0, len(perm), batch):
            sel = np.asarray(perm[s:s + batch])
            loss, g, _ = loss_grad(p, F, hid, L, states[sel], active[sel], targets[sel])
            losses.append(loss)
            m = beta[0] * m + (1 - beta[0]) * g
            v = beta[1] * v + (1 - beta[1]) * g * g
            p = p - m / (1 - bp[0]) / (np.sqrt(v / (1 - bp[1])) + eps) * eta
            bp = [bp[0] * beta[0], bp[1] * beta[1]]
        hist.append(float(np.mean(losses)))
    return hist, p
