"""Float64 restatement of the critic's PPO-clipped value loss (test helper, CPU only), on top of tests/value_ref.py:

    L = sum_b max((V_b - t_b)^2, (Vclip_b - t_b)^2) / B_global,    Vclip = V_old + clamp(V - V_old, -c, c)

(no factor 1/2: it continues Flux.mse).  torch float64 autograd gives the gradient; the analytic dL/dy -- the mse's on the
states that keep their unclipped square, exactly 0 on the ones whose clipped square is the larger -- is restated beside it.
make_regimes builds old values and targets that keep every state away from both decision boundaries (|V - V_old| = c, and
the tie of the two squares), so that fp32 and float64 cannot disagree about the branch."""
import numpy as np

import value_ref

INSIDE, KEPT, CLIPPED = 0, 1, 2                 # |delta| <= c; outside and the unclipped square wins; outside and it loses


def branches(v, v_old, t, c):
    """numpy float64 -> dict of delta, inside, vclip, d, dc, keep, term (the difference whose square enters the loss)."""
    v, v_old, t = (np.asarray(x, np.float64) for x in (v, v_old, t))
    c = float(c)
    delta = v - v_old
    inside = np.abs(delta) <= c
    vclip = np.where(inside, v, v_old + np.copysign(c, delta))
    d, dc = v - t, vclip - t
    keep = inside | (np.abs(d) >= np.abs(dc))
    return {"delta": delta, "inside": inside, "vclip": vclip, "d": d, "dc": dc, "keep": keep, "term": np.where(keep, d, dc)}


def analytic_dy(values, active, targets, v_old, c, B_global, H):
    """dL/dy [B, H, 4]: value_ref.analytic_dy on the states that keep the unclipped square, 0 on the others."""
    keep = branches(values, v_old, targets, c)["keep"]
    return value_ref.analytic_dy(values, active, targets, B_global, H) * keep[:, None, None]


def loss_grad(params, F, hid, L, states, active, targets, v_old, c, B_global=None, chunk=2048, want_dy=False):
    """float64 autograd of the clipped loss, chunk by chunk like value_ref.loss_grad -> (loss, flat gradient in Flux order,
    V [B]) and, with want_dy, dL/dy [B, H, 4] from autograd."""
    import torch
    B = len(states)
    Bg = float(B if B_global is None else B_global)
    c = float(c)
    tl = value_ref._torch_layers(params, F, hid, L)
    loss, vals, dys = 0.0, [], []
    for s in range(0, B, chunk):
        v, y = value_ref._torch_values(tl, states[s:s + chunk], active[s:s + chunk], keep_y=want_dy)
        t = torch.tensor(np.asarray(targets[s:s + chunk], np.float64))
        vo = torch.tensor(np.asarray(v_old[s:s + chunk], np.float64))
        vclip = vo + torch.clamp(v - vo, -c, c)
        part = torch.maximum((v - t) ** 2, (vclip - t) ** 2).sum() / Bg
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


def make_regimes(rng, v64, c):
    """Old values and targets (float32, what the buffer stores) for states whose float64 value is v64, a third of the states
    in each regime:  V_old = V64 - s m c with s = +-1 and m in [0.25, 0.75] (INSIDE) or [1.5, 3] (outside); for outside states
    t lies outside the interval between Vclip and V64 by u c, u in [0.25, 1.5]: beyond V64 for CLIPPED (the clipped square is
    then the larger one: the state loses its gradient), beyond Vclip for KEPT.  INSIDE states get |V64 - t| in [0.5, 2].
    -> (v_old, t, regime)"""
    v64 = np.asarray(v64, np.float64)
    B = len(v64)
    c = float(c)
    regime = rng.permutation(np.arange(B) % 3)
    s = rng.choice([-1.0, 1.0], size=B)
    m = np.where(regime == INSIDE, rng.uniform(0.25, 0.75, size=B), rng.uniform(1.5, 3.0, size=B))
    v_old = v64 - s * m * c
    vclip = v_old + s * c                                             # outside states: delta = s m c, |delta| > c
    u = rng.uniform(0.25, 1.5, size=B)
    t = np.where(regime == CLIPPED, v64 + s * u * c, vclip - s * u * c)
    t = np.where(regime == INSIDE, v64 + rng.choice([-1.0, 1.0], size=B) * rng.uniform(0.5, 2.0, size=B), t)
    return v_old.astype(np.float32), t.astype(np.float32), regime


def check_margins(v64, v_old, t, c, regime):
    """The float64 preconditions of the GPU tests: every state at least 0.2 c from |delta| = c, every outside state at least
    0.4 c from the tie of the two squares, every regime at least 20 % of the states, and the regimes what branches() says."""
    c = float(c)
    b = branches(v64, v_old, t, c)
    assert np.all(np.abs(np.abs(b["delta"]) - c) >= 0.2 * c)
    out = ~b["inside"]
    assert np.all(np.abs(np.abs(b["d"]) - np.abs(b["dc"]))[out] >= 0.4 * c)
    assert np.array_equal(b["inside"], regime == INSIDE) and np.array_equal(b["keep"], regime != CLIPPED)
    for r in (INSIDE, KEPT, CLIPPED):
        assert np.count_nonzero(regime == r) >= 0.2 * len(regime)
    return b
