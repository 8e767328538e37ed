"""A gradient bar per parameter block, set by the block's own fp32 floor (test helper, CPU only).

The bar of every fp32 gradient test here is one maximum over the flat gradient, max|g - g64| <= 2e-5 max|g64|.  It is blind
to the blocks that are small next to the largest one (with trained weights b2 is 1 % of W1), and on peaked policies it lies
below what plain fp32 arithmetic delivers.  This module resolves the comparison per block and takes the bar from the
reference alone:

  blocks(F, hid_user, HID, L)  the flat gradient cut into W1, b1, ..., W_L, b_L and the output layer as one block
  tiles(F, hid_user, HID, L)   every W cut again into 32-unit feature tiles, the granularity at which the kernels assign work
  grad64 / grad32              the step_batch! loss of np_oracle.step_batch_grad_torch differentiated in float64 / float32
  floor(block)                 || grad32[block] - grad64[block] ||_2, absolute (some blocks are exact cancellations)
  the bar                      || g[block] - g64[block] ||_2 <= M floor(block); for a tile
                               M max(floor(tile), floor(parent block) sqrt(n_tile / n_block))

M = 4 is the factor tests/test_gpu_split_backward.py grants a second fp32-grade chain over the first (e1 <= 4 e0): about 2
for the amount by which one block's floor moves between two env seeds, 2 for the ordering of the kernels' sums.  It is fixed
from the reference, not from what the kernels deliver.

The cases are built here without a device (engine rollouts by the oracle, which the device matches bit for bit), so that
tests/test_grad_blocks_host.py can assert on the CPU what the device cases rest on."""
import os

import numpy as np

import advantage_modes_ref as am
import value_ref
from oracle import np_oracle

M = 4.0
EPS, ENT = am.EPS, am.ENT
KINK = 2e-6                          # states with a hidden pre-activation this close to leakyrelu's kink are left out
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------------------------------------------------------- the cuts
def blocks(F, hid_user, HID, L):
    """name -> slice of the flat gradient in np_oracle.unpack_params order (the caller's width hid_user, run at HID):
    W1, b1, ..., W_L, b_L, then "out" = the output layer's weights and its four biases together (the lone bias moves by
    about 4x between two accumulation orders: too noisy to stand alone)."""
    assert 1 <= hid_user <= HID and HID % 32 == 0 and 1 <= L <= 4
    out, o = {}, 0
    for l, (no, ni) in enumerate([(hid_user, F)] + [(hid_user, hid_user)] * (L - 1), 1):
        out["W%d" % l] = slice(o, o + no * ni)
        o += no * ni
        out["b%d" % l] = slice(o, o + no)
        o += no
    out["out"] = slice(o, o + 4 * hid_user + 4)
    return out


def num_params(F, hid_user, L):
    return hid_user * F + hid_user + (L - 1) * (hid_user * hid_user + hid_user) + 4 * hid_user + 4


def tiles(F, hid_user, HID, L):
    """name -> (parent block, flat indices): W1 in row tiles of 32 output units, every hidden-to-hidden W in 32 x 32 tiles.
    W is stored column-major (Flux): element (o, i) of a [no, ni] matrix lies at o + i no.  A padded width has a ragged last
    tile; the padding units of the HID-wide kernels do not cross the ABI."""
    nt = -(-hid_user // 32)
    assert nt <= HID // 32
    cut = [np.arange(32 * t, min(32 * t + 32, hid_user)) for t in range(nt)]
    bl = blocks(F, hid_user, HID, L)
    out = {}
    for t in range(nt):
        out["W1[%d]" % t] = ("W1", (bl["W1"].start + cut[t][:, None] + np.arange(F)[None, :] * hid_user).ravel())
    for l in range(2, L + 1):
        for to in range(nt):
            for ti in range(nt):
                idx = bl["W%d" % l].start + cut[to][:, None] + cut[ti][None, :] * hid_user
                out["W%d[%d,%d]" % (l, to, ti)] = ("W%d" % l, idx.ravel())
    return out


# ---------------------------------------------------------------- the two references
def _forward(dtype, params, F, hid_user, states, masks, actions0, p_old, adv, eps, entropy_weight, n_hidden, B_global):
    """The loss of np_oracle.step_batch_grad_torch in `dtype`, every operation in that type.
    -> (leaf tensors [(W, b)], total loss, ppo loss, entropy loss, hidden activations, pre-activations)."""
    import torch
    tl = [(torch.tensor(W.copy(), dtype=dtype, requires_grad=True), torch.tensor(b.copy(), dtype=dtype, requires_grad=True))
          for (W, b) in np_oracle.unpack_params(params, F, hid_user, n_hidden)]
    x = torch.tensor(np.asarray(states), dtype=dtype)
    B, H, _ = x.shape
    a, acts, pre = x, [x], []
    for (W, b) in tl[:-1]:
        z = a @ W.T + b
        z.retain_grad()
        a = torch.nn.functional.leaky_relu(z, 0.01)
        pre.append(z)
        acts.append(a)
    W, b = tl[-1]
    logits = (a @ W.T + b).reshape(B, H * 4) + torch.tensor(np.asarray(masks), dtype=dtype)
    probs = torch.softmax(logits, dim=1)
    sel = probs[torch.arange(B), torch.tensor(np.asarray(actions0), dtype=torch.long)]
    advt = torch.tensor(np.asarray(adv), dtype=dtype)
    gain = sel / torch.tensor(np.asarray(p_old), dtype=dtype) * advt
    clip = torch.where(advt >= 0, (1.0 + eps) * advt, (1.0 - eps) * advt)
    mean = torch.mean if B_global is None else (lambda t: t.sum() / B_global)
    ppoloss = -mean(torch.minimum(gain, clip))
    s = float(np.float32(1e-8))
    sp = (1.0 - s) * probs + s / (H * 4)
    entloss = -mean(-(sp * torch.log(sp)).sum(dim=1)) * entropy_weight
    return tl, ppoloss + entloss, ppoloss, entloss, acts, pre


def _flat(pairs):
    return np.concatenate([np.concatenate([W.astype(np.float64).ravel(order="F"), b.astype(np.float64)]) for (W, b) in pairs])


def _grad(dtype, params, F, HID, states, masks, actions0, p_old, adv, eps, entropy_weight, n_hidden=2, B_global=None):
    tl, loss, lp, le, _, _ = _forward(dtype, params, F, HID, states, masks, actions0, p_old, adv, eps, entropy_weight, n_hidden,
                                      B_global)
    loss.backward()
    return _flat([(W.grad.numpy(), b.grad.numpy()) for (W, b) in tl]), float(lp.detach()), float(le.detach())


def grad64(params, F, HID, states, masks, actions0, p_old, adv, eps, entropy_weight, n_hidden=2, B_global=None):
    """(flat gradient, ppo loss, entropy loss) by torch autograd in float64; the arguments of step_batch_grad_torch
    (HID: the caller's width).  Agrees with oracle.step_batch_grad_f64 to 1e-12 of max|g| (test_grad_blocks_host.py)."""
    import torch
    return _grad(torch.float64, params, F, HID, states, masks, actions0, p_old, adv, eps, entropy_weight, n_hidden, B_global)


def grad32(params, F, HID, states, masks, actions0, p_old, adv, eps, entropy_weight, n_hidden=2, B_global=None):
    """The same loss and its gradient in plain float32, as float64 values: its distance from grad64 is the floor."""
    import torch
    return _grad(torch.float32, params, F, HID, states, masks, actions0, p_old, adv, eps, entropy_weight, n_hidden, B_global)


def bf16_top_two(t):
    """hi + mid of the split-fp32 form of a float32 tensor: what is left of it when the low bf16 piece is dropped."""
    import torch
    hi = t.to(torch.bfloat16).to(torch.float32)
    return hi + (t - hi).to(torch.bfloat16).to(torch.float32)


def grad32_low_piece_dropped(which, params, F, HID, states, masks, actions0, p_old, adv, eps, entropy_weight):
    """grad32 of a two-hidden-layer policy with the low bf16 piece of one operand of one backward product dropped:
    which = "H1 in dW2": dW2 = dZ2^T (hi + mid)(H1);  which = "W2 in dH1": dH1 = dZ2 (hi + mid)(W2), and dW1, db1 from it."""
    import torch
    tl, loss, _, _, acts, pre = _forward(torch.float32, params, F, HID, states, masks, actions0, p_old, adv, eps, entropy_weight,
                                         2, None)
    loss.backward()
    g = [[W.grad.clone(), b.grad.clone()] for (W, b) in tl]
    with torch.no_grad():
        dZ2 = pre[1].grad.reshape(-1, HID)
        H1 = acts[1].reshape(-1, HID)
        if which == "H1 in dW2":
            g[1][0] = dZ2.T @ bf16_top_two(H1)
        else:
            assert which == "W2 in dH1"
            dZ1 = (dZ2 @ bf16_top_two(tl[1][0].detach())) * torch.where(pre[0].detach().reshape(-1, HID) > 0, 1.0, 0.01)
            g[0][0] = dZ1.T @ acts[0].reshape(-1, F)
            g[0][1] = dZ1.sum(dim=0)
    return _flat([(W.numpy(), b.numpy()) for (W, b) in g])


# ---------------------------------------------------------------- floors and bars
def floors(g32, g64, bl, tl):
    """(block -> floor, tile -> the tile's bar floor max(floor(tile), floor(parent) sqrt(n_tile / n_block)))."""
    d = np.asarray(g32, np.float64) - g64
    fb = {k: float(np.linalg.norm(d[s])) for k, s in bl.items()}
    ft = {k: max(float(np.linalg.norm(d[idx])), fb[par] * np.sqrt(len(idx) / (bl[par].stop - bl[par].start)))
          for k, (par, idx) in tl.items()}
    return fb, ft


def multiples(g, g64, fb, ft, bl, tl):
    """(block -> ||g - g64|| / floor, (worst tile, its multiple of its bar floor), the old metric max|g - g64| / max|g64|)."""
    d = np.asarray(g, np.float64) - g64
    mb = {k: float(np.linalg.norm(d[s]) / fb[k]) for k, s in bl.items()}
    mt = {k: float(np.linalg.norm(d[idx]) / ft[k]) for k, (par, idx) in tl.items()}
    worst = max(mt, key=mt.get)
    return mb, (worst, mt[worst]), float(np.abs(d).max() / np.abs(g64).max())


# ---------------------------------------------------------------- the cases
# Beyond am.FAMILIES: backwards the family table does not pin (knobs as tests/test_gpu_split_backward.py and
# tests/test_gpu_bench_shapes.py set them), depths 1 and 4, a padded width, and peaked policies on the default route.
# kind "random": random states off the kink through set_columns; "rollout": a 32 x 12 engine rollout with golden weights.
X6_128 = ("k_policy_fwd_train_x6<128>", "k_policy_bwd_x6<72,128>")
EXTRA = {
    "three-product-37": dict(kind="random", hid=128, L=2, B=37, knobs=dict(split=0, small=4096),
                             route=("k_policy_fwd_train_split<72,128,4,0>", "k_policy_bwd_data<72,128>")),
    "three-product-385": dict(kind="random", hid=256, L=2, B=385, knobs=dict(split=0, small=4096),
                              route=("k_policy_fwd_train_split<72,256,2,0>", "k_policy_bwd_data<72,256>")),
    "fused-fp32-37": dict(kind="random", hid=128, L=2, B=37, knobs=dict(split=0, small=0),
                          route=("k_policy_fwd_train_split<72,128,4,0>", "k_policy_bwd<72,128>")),
    "fused-fp32-385": dict(kind="random", hid=256, L=2, B=385, knobs=dict(split=0, small=0),
                           route=("k_policy_fwd_train_split<72,256,2,0>", "k_policy_bwd<72,256>")),
    "L1-37": dict(kind="random", hid=128, L=1, B=37, knobs={}, route=("k_policy_fwd<72,128,2,1,1>", "k_policy_bwd_data_deep<72,128>")),
    "L4-37": dict(kind="random", hid=128, L=4, B=37, knobs={}, route=("k_policy_fwd<72,128,2,1,1>", "k_policy_bwd_data_deep<72,128>")),
    "width-50": dict(kind="random", hid=50, L=2, B=100, knobs={}, route=X6_128),
    "poly-30-seed17": dict(kind="rollout", weights="poly-30-policy", env_seed=17, hid=128, L=2, B=200, knobs={}, route=X6_128),
    "poly-30-seed21": dict(kind="rollout", weights="poly-30-policy", env_seed=21, hid=128, L=2, B=200, knobs={}, route=X6_128),
    "catmull-clark-seed17": dict(kind="rollout", weights="catmull-clark-policy", env_seed=17, hid=128, L=2, B=200, knobs={},
                                 route=X6_128),
    "catmull-clark-seed21": dict(kind="rollout", weights="catmull-clark-policy", env_seed=21, hid=128, L=2, B=200, knobs={},
                                 route=X6_128),
    "peaked-out-x8": dict(kind="random", hid=256, L=2, B=200, out_scale=8.0, knobs={},
                          route=("k_policy_fwd_train_x6<256>", "k_policy_bwd_x6<72,256>")),
}
ROLLOUT_N, ROLLOUT_T, ROLLOUT_MAX_ACTIONS = 32, 12, 12
F32_FAMILIES = [f for f, c in am.FAMILIES.items() if c["dtype"] == "f32"]
BF16_FAMILIES = [f for f, c in am.FAMILIES.items() if c["dtype"] == "bf16"]
F32_CASES = F32_FAMILIES + list(EXTRA)


def kernel_width(hid_user):
    return 128 if hid_user <= 128 else 256


def shape_of(name):
    """dict(F, Q, hid, HID, L, dtype) of a case: hid is the caller's width, HID the width the kernels run."""
    c = am.FAMILIES[name] if name in am.FAMILIES else dict(EXTRA[name], F=72, Q=8, dtype="f32")
    return dict(F=c["F"], Q=c["Q"], hid=c["hid"], HID=kernel_width(c["hid"]), L=c["L"], dtype=c["dtype"])


def pool(c, params, states, active, a0, p_old, eps=EPS):
    """am.trainable_pool with this module's kink distance: the positions of an engine rollout that are off the kink under
    `params` and whose float64 ratio is not within 1e-3 of 1 +- eps."""
    n = len(states)
    p64 = am.probabilities(params, c["dtype"], c["F"], c["hid"], c["L"], states, active, c["Q"])[np.arange(n), a0]
    r64 = p64 / p_old.astype(np.float64)
    clear = (np.abs(r64 - (1 - eps)) > 1e-3) & (np.abs(r64 - (1 + eps)) > 1e-3)
    return np.flatnonzero(value_ref.off_the_kink(params, c["F"], c["hid"], c["L"], states, delta=KINK) & clear), p64


def _random_case(name):
    """As am.expanded_case: states off the kink, actions from the policy's own probabilities, ratios off the clip, returns
    ~ N(0.3, 1).  `kept`: the share of candidate states the kink filter passed, of ratios the clip margin passed."""
    c = EXTRA[name]
    seed = 500 + list(EXTRA).index(name)
    rng = np.random.default_rng(seed)
    F, Q, hid, L, B = 72, 8, c["hid"], c["L"], c["B"]
    params = am.make_params(F, hid, L, seed)
    if "out_scale" in c:
        params[blocks(F, hid, kernel_width(hid), L)["out"]] *= np.float32(c["out_scale"])
    cand = rng.integers(-3, 7, size=(2 * B, 4 * Q, F)).astype(np.int8)
    ok = value_ref.off_the_kink(params, F, hid, L, cand, delta=KINK)
    assert ok.sum() >= B, (name, int(ok.sum()))
    states = np.ascontiguousarray(cand[ok][:B])
    active = rng.integers(1, 2 ** Q, size=B, dtype=np.uint64).astype(np.uint32)
    probs = am.probabilities(params, "f32", F, hid, L, states, active, Q)
    a0 = am.sample_actions(rng, probs)
    raw = rng.uniform(0.8, 1.25, 4096)
    off = (np.abs(raw - (1 - EPS)) >= am.MARGIN) & (np.abs(raw - (1 + EPS)) >= am.MARGIN)
    p_old = (probs[np.arange(B), a0] / am.ratios_off_the_clip(rng, B, EPS)).astype(np.float32)
    T, N = am.buffer_shape(B)
    return dict(params=params, states=states, active=active, a0=a0, p_old=p_old, T=T, N=N,
                R=(0.3 + rng.normal(size=B)).astype(np.float32), sel0=rng.permutation(B),
                kept=float(ok.mean()) * float(off.mean()))


def _rollout_case(name, orc):
    """A 32 x 12 rollout of the built-in game under reference-trained weights (tests/test_gpu_parity.py::
    test_gradient_with_reference_trained_weights), collected by the oracle in device order: the device's rollout bit for bit.
    The minibatch is 200 of its states that are off the kink, p_old moved off the clip, the advantage the returns."""
    c = EXTRA[name]
    rng = np.random.default_rng(600 + list(EXTRA).index(name))
    params = np.load(os.path.join(GOLDEN, c["weights"] + ".npz"))["params"].astype(np.float32)
    env = orc.Env(Q=8, max_actions=ROLLOUT_MAX_ACTIONS, N=ROLLOUT_N, seed=c["env_seed"])
    env.reset()
    ro = orc.collect_rollouts_tn(env, params, c["hid"], ROLLOUT_T, mode_dev=True)
    n = ROLLOUT_N * ROLLOUT_T
    states, active = ro["states"].reshape(n, 32, 72), ro["active"].reshape(n)
    a0 = ro["actions"].reshape(n).astype(np.int32)
    R = orc.compute_returns_tn(ro["rewards"], ro["done"], 1.0).reshape(n)
    sh = shape_of(name)
    p64 = am.probabilities(params, "f32", 72, c["hid"], c["L"], states, active, 8)[np.arange(n), a0]
    p_old = (p64 / am.ratios_off_the_clip(rng, n, EPS)).astype(np.float32)
    keep, _ = pool(sh, params, states, active, a0, p_old)
    sel0 = rng.choice(keep, size=c["B"], replace=len(keep) < c["B"])
    T, N = ROLLOUT_T, ROLLOUT_N
    return dict(params=params, states=states, active=active, a0=a0, p_old=p_old, T=T, N=N, R=R, sel0=sel0,
                kept=len(keep) / n)


def _compact_case(name, orc):
    """A compact-storage family: the engine rollout am.ROLLOUT collected by the oracle (the device's bit for bit), trained on
    by the moved parameters; the minibatch is drawn from the states that are off the kink under those."""
    c, r = am.FAMILIES[name], am.ROLLOUT
    rng = np.random.default_rng(700 + list(am.FAMILIES).index(name))
    p0, moved = am.rollout_start()
    if "compact-rollout" not in _CACHE:                     # the two compact families share the one rollout
        env = orc.Env(Q=r["Q"], max_actions=r["max_actions"], N=r["N"], seed=r["env_seed"])
        env.reset()
        _CACHE["compact-rollout"] = orc.collect_rollouts_tn(env, p0, r["hid"], r["T"], mode_dev=True)
    ro = _CACHE["compact-rollout"]
    n = r["N"] * r["T"]
    states, active = ro["states"].reshape(n, 32, 72), ro["active"].reshape(n)
    a0, p_old = ro["actions"].reshape(n).astype(np.int32), ro["p_sel"].reshape(n)
    R = orc.compute_returns_tn(ro["rewards"], ro["done"], r["discount"]).reshape(n)
    keep, _ = pool(c, moved, states, active, a0, p_old)
    sel0 = rng.choice(keep, size=c["B"], replace=len(keep) < c["B"])
    return dict(params=moved, collect_params=p0, states=states, active=active, a0=a0, p_old=p_old, T=r["T"], N=r["N"], R=R,
                sel0=sel0, kept=len(keep) / n)


_CACHE = {}


def case(name, orc=None):
    """The dataset of a case in storage order with its minibatch sel0 and the advantage column R (mode "returns").
    orc: the oracle module, needed by the rollout cases."""
    if name not in _CACHE:
        if name in am.FAMILIES and am.FAMILIES[name]["compact"]:
            d = _compact_case(name, orc)
        elif name in am.FAMILIES:
            d = dict(am.expanded_case(name))
            d["kept"] = kink_pass_rate(name, d["params"]) * _CLIP_PASS
        elif EXTRA[name]["kind"] == "random":
            d = _random_case(name)
        else:
            d = _rollout_case(name, orc)
        _CACHE[name] = d
    return _CACHE[name]


_CLIP_PASS = 1.0 - 2 * (2 * am.MARGIN) / (1.25 - 0.8)      # the share of uniform(0.8, 1.25) ratios am.ratios_off_the_clip keeps


def kink_pass_rate(name, params, n=256):
    """The share of am.random_states' candidates (its distribution, a fresh draw) that its kink filter keeps under `params`."""
    c = am.FAMILIES[name]
    cand = np.random.default_rng(7).integers(-3, 7, size=(n // (c["Q"] // 8), 4 * c["Q"], c["F"])).astype(np.int8)
    return float(value_ref.off_the_kink(params, c["F"], c["hid"], c["L"], cand).mean())


def minibatch(d):
    s = d["sel0"]
    return dict(states=d["states"][s], active=d["active"][s], a0=d["a0"][s], p_old=d["p_old"][s], adv=d["R"][s])


def reference(sh, params, mb, eps=EPS, ent=ENT):
    """dict(g64, g32, lp, le: the float64 losses, fb: block floors, ft: tile bar floors, blocks, tiles) of a minibatch()."""
    masks = np_oracle.batch_masks(mb["active"], sh["Q"])
    args = (params, sh["F"], sh["hid"], mb["states"], masks, mb["a0"], mb["p_old"], mb["adv"], eps, ent)
    g64, lp, le = grad64(*args, n_hidden=sh["L"])
    g32, _, _ = grad32(*args, n_hidden=sh["L"])
    bl, tl = blocks(sh["F"], sh["hid"], sh["HID"], sh["L"]), tiles(sh["F"], sh["hid"], sh["HID"], sh["L"])
    fb, ft = floors(g32, g64, bl, tl)
    return dict(g64=g64, g32=g32, lp=lp, le=le, fb=fb, ft=ft, blocks=bl, tiles=tl)
