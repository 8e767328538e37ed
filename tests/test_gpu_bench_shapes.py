"""The training pass at the minibatch sizes bench.py launches, with the library's DEFAULT kernel selection (no kernel-selection
environment variables, no tile-count setters): the 4096-state headline minibatch (HID = 256 and 128), the switch points of
the split train forward (1536 tiles at HID = 256, 1024 at HID = 128) and one state on either side, the config-4 action space
(Q = 32) up to 8192 states, the layer-looped policies (--layers 1 / 3), and the 65536-state bf16 minibatch of config 5.

(a) float64 parity: every case against the torch float64 gradient (oracle/np_oracle.py, built chunk by chunk), at the bar
    of every gradient test here (2e-5 of max|g|), bitwise reproducible.  At these sizes one state moves the mean gradient by
    only about the bar (measured and recorded per case, see the note in the test), so (a) alone cannot see a lost tile.
(b) additivity, device against device, for every shape of (a) and the 65536-state bf16 minibatch: one launch over B states
    against the sum of launches over chunks with B_global = B, to a derived fp32-reordering tolerance that each case shows to
    be 10x below one sampled state's effect.  The bf16 mode cannot see a lost tile through a float64 comparison either (its
    bar is 1 % of max|g|).
(c) the optimiser step the benchmark takes (one 4096-state minibatch per step, Adam and the re-pack of every weight image in
    the slab-reduction launch at world 1): parameters, Adam moments and loss history bit for bit against the oracle's Adam on
    forward_backward's gradient, on the fused and on the unfused (all-reduce hook) path; then a fresh policy given the trained
    parameters through set_params must compute the same probabilities and gradients bit for bit (pins the re-pack).
Every launch also asserts the kernels the library picks for it (ppo_debug_train_route, see tests/test_train_route.py).

TEST_RECORD_DIR=<dir>: append the measured errors / tolerances of every case to <dir>/bench_shapes.jsonl."""
import json
import os

import numpy as np
import pytest

from oracle import np_oracle
from test_train_route import DEFAULT, expected, route

pytestmark = pytest.mark.gpu

F, EPS, ENT = 72, 0.05, 0.01          # bench.py: eps 0.05, entropy weight 0.01
BAR = 2e-5                            # max|g - g64| <= BAR * max|g64|: the bar of every fp32 gradient test
U32 = 2.0 ** -24                      # fp32 unit roundoff (round to nearest)


@pytest.fixture(scope="module")
def P(ppo):
    if ppo.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests must run on the GPU box")
    return ppo


@pytest.fixture()
def knobs(P):
    """The two knobs a test here may switch, restored to the library defaults whatever happens."""
    yield P
    P.set_bwd_split_bf16(None)
    P.set_rollout_compact(None)


def _assert_route(P, dtype, split, Q, hid, L, B, compact=False, want=None):
    """The library's route for this launch is the restated table's (and `want`, where the case names its kernels)."""
    got = route(P, dtype, F, hid, L, 4 * Q, compact, B)
    assert got == expected(dtype, F, hid, L, 4 * Q, compact, B, dict(DEFAULT, split=split)), got
    assert want is None or got == want, (got, want)


def _record(rec):
    d = os.environ.get("TEST_RECORD_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "bench_shapes.jsonl"), "a") as f:
            f.write(json.dumps(rec) + "\n")


def _policy(P, hid, L, rng, dtype="f32", seed=1):
    pol = P.HipPolicy(F, hid, L, 4, seed=seed, dtype=dtype)
    pol.params = (pol.params + (rng.normal(size=pol.num_params) * 0.02).astype(np.float32)).astype(np.float32)
    return pol


def _off_the_kink(params, hid, L, states, delta=1e-5):
    """True per state when no hidden unit's pre-activation, at any of the H rows, lies within `delta` of leakyrelu's kink.
    There fp32 and float64 can disagree about the sign (fp32 error of a 72..256-term dot product ~1e-6), the derivative jumps
    100x and a whole gradient row differs by O(1e-3 max|g|) between ANY two precisions (see test_gpu_deep_policy.py).
    Any H (32 rows for Q = 8, 128 for Q = 32); evaluated 256 states at a time to keep the float64 activations small."""
    B, H = states.shape[:2]
    ok = np.ones(B, bool)
    layers = np_oracle.unpack_params(params, F, hid, L)[:-1]
    for s in range(0, B, 256):
        a = states[s:s + 256].reshape(-1, F).astype(np.float64).T
        n = a.shape[1] // H
        for (W, b) in layers:
            z = W.astype(np.float64) @ a + b.astype(np.float64)[:, None]
            ok[s:s + n] &= np.abs(z).min(axis=0).reshape(n, H).min(axis=1) >= delta
            a = np.where(z > 0, z, 0.01 * z)
    return ok


class Cols:
    """One minibatch's columns as the references take them (0-based actions, Q quads -> H = 4 Q rows)."""

    def __init__(self, states, active, a0, p_old, adv, Q):
        self.states, self.active, self.a0, self.p_old, self.adv, self.Q = states, active, a0, p_old, adv, Q

    def take(self, sel0):
        return Cols(self.states[sel0], self.active[sel0], self.a0[sel0], self.p_old[sel0], self.adv[sel0], self.Q)


def _by_shape(P, pol, rng, B, Q, kink=True, ratio=(0.8, 1.25)):
    """A minibatch of B random states at Q quads loaded through set_columns: states off the kink (when the test compares
    with float64), actions sampled from the policy's own probabilities, p_old near them (ratios 0.8..1.25, the regime
    step_batch! runs in), advantages of both signs.  ratio = (1, 1): p_old = p, no sample clipped, |advantage| in [1, 4]
    (every state carries a PPO gradient of its own).  Returns (dataset, Cols) in dataset order."""
    H = 4 * Q
    parts, have = [], 0
    while have < B:
        cand = rng.integers(-3, 7, size=(B - have + B // 8 + 16, H, F)).astype(np.int8)
        if kink:
            cand = cand[_off_the_kink(pol.params, pol.hidden_channels, pol.num_hidden_layers, cand)]
        parts.append(cand)
        have += len(cand)
    states = np.ascontiguousarray(np.concatenate(parts)[:B])
    active = rng.integers(1, 2 ** Q, size=B, dtype=np.uint64).astype(np.uint32)
    probs = P.batch_action_probabilities(pol, P.StateData(states, active)).T.astype(np.float64)     # [B, A]
    cdf = np.cumsum(probs, axis=1)
    u = rng.random(B) * cdf[:, -1]
    a0 = (cdf < u[:, None]).sum(axis=1).astype(np.int32)                 # inverse CDF: never a zero-probability action
    assert np.all(probs[np.arange(B), a0] > 0)
    p_old = (probs[np.arange(B), a0] * rng.uniform(ratio[0], ratio[1], B)).astype(np.float32)
    if ratio == (1, 1):
        adv = (rng.choice([-1.0, 1.0], size=B) * rng.uniform(1, 4, B)).astype(np.float32)
    else:
        adv = (rng.normal(size=B) * 3).astype(np.float32)
    ro = P.BufferRollouts()
    ro.set_columns(None, states[None], active[None], a0[None].astype(np.int64) + 1, p_old[None], adv[None])
    return P.construct_dataset(ro), Cols(states, active, a0, p_old, adv, Q)


def _from_rollout(P, pol, N, T, Q=8):
    """A dataset from an engine rollout (the storage form set by set_rollout_compact), with its columns read back."""
    env = P.HipVecEnv(num_envs=N, Q=Q, max_actions=16, seed=N + T)
    ro = P.BufferRollouts()
    P.collect_rollouts_steps_(ro, env, pol, T, 1.0)
    st, act = ro.state_data
    cols = Cols(st.reshape(-1, 4 * Q, F), act.reshape(-1), (ro.selected_actions.reshape(-1) - 1).astype(np.int32),
                ro.selected_action_probabilities.reshape(-1), ro.rewards.reshape(-1), Q)
    return P.construct_dataset(ro), cols


def _ref64(params, hid, L, c, B_global=None):
    """float64 gradient (torch autograd) as a sum of chunks of at most 32768 rows."""
    masks = np_oracle.batch_masks(c.active, c.Q)
    return np_oracle.step_batch_grad_chunked(np_oracle.step_batch_grad_torch, params, F, hid, c.states, masks, c.a0, c.p_old,
                                             c.adv, EPS, ENT, chunk=32768 // (4 * c.Q), B_global=B_global, n_hidden=L)


def _teeth64(params, hid, L, c, rng, g64):
    """min over 8 sampled states s of max|c_s| / (BAR max|g64|), c_s = the float64 contribution of state s to the mean
    gradient (a one-state reference with B_global = B): dropping or doubling s moves the gradient by c_s."""
    B = len(c.states)
    worst = np.inf
    for s in rng.choice(B, size=8, replace=False):
        cs, _, _ = _ref64(params, hid, L, c.take([s]), B_global=B)
        worst = min(worst, np.abs(cs).max() / (BAR * np.abs(g64).max()))
    return worst


# ---------------------------------------------------------------- (a) float64 parity at the bench shapes
# (Q, HID, L, states, source): "shape" = random states through set_columns, "compact" = an engine rollout in compact storage
PARITY = [
    (8, 256, 2, 4096, "shape"),      # headline minibatch: two-tile split forward, 16 tiles per backward workgroup
    (8, 256, 2, 4096, "compact"),    # headline minibatch from compact rollout storage (the train forward re-derives the rows)
    (8, 128, 2, 4096, "shape"),      # --hid 128
    (8, 256, 2, 1535, "shape"),      # HID = 256 split train forward: one-tile form below 1536 tiles,
    (8, 256, 2, 1536, "shape"),      # the two-tile form from 1536 on,
    (8, 256, 2, 1537, "shape"),      # with an odd last pass
    (8, 128, 2, 1023, "shape"),      # HID = 128: the same switch at 1024 tiles
    (8, 128, 2, 1024, "shape"),
    (8, 128, 2, 1025, "shape"),
    (32, 256, 2, 1024, "shape"),     # config-4 action space (H = 128 rows: 4 tiles per state)
    (32, 256, 2, 8192, "shape"),     # config-4 shape: 32768 tiles, 128 per backward workgroup
    (32, 128, 2, 1024, "shape"),     # Q = 32 at HID = 128: fp32-MFMA forward, split backward
    (8, 256, 3, 4096, "shape"),      # --layers 3: layer-looped kernels
    (8, 256, 1, 4096, "shape"),      # --layers 1
]
# the kernels each case of PARITY runs with the default knobs (split-fp32 on)
X6T, X6, X6S, BX6 = "k_policy_fwd_train_x6t<%d,2>", "k_policy_fwd_train_x6<%d>", "k_policy_fwd_train_x6s<256,4>", "k_policy_bwd_x6<72,%d>"
PARITY_ROUTE = {
    (8, 256, 2, 4096): (X6T % 256, BX6 % 256), (8, 128, 2, 4096): (X6T % 128, BX6 % 128),
    (8, 256, 2, 1535): (X6 % 256, BX6 % 256), (8, 256, 2, 1536): (X6T % 256, BX6 % 256), (8, 256, 2, 1537): (X6T % 256, BX6 % 256),
    (8, 128, 2, 1023): (X6 % 128, BX6 % 128), (8, 128, 2, 1024): (X6T % 128, BX6 % 128), (8, 128, 2, 1025): (X6T % 128, BX6 % 128),
    (32, 256, 2, 1024): (X6S, BX6 % 256), (32, 256, 2, 8192): (X6S, BX6 % 256),
    (32, 128, 2, 1024): ("k_policy_fwd<72,128,2,4,0>", BX6 % 128),
    (8, 256, 3, 4096): ("k_policy_fwd<72,256,2,1,1>", "k_policy_bwd_data_deep<72,256>"),
    (8, 256, 1, 4096): ("k_policy_fwd<72,256,2,1,1>", "k_policy_bwd_data_deep<72,256>"),
}


@pytest.mark.parametrize("Q,hid,L,B,source", PARITY, ids=["Q%d-h%d-L%d-%d-%s" % c for c in PARITY])
def test_bench_shape_gradient_vs_f64(P, knobs, Q, hid, L, B, source):
    rng = np.random.default_rng(Q * 100000 + hid * 100 + L * 10 + B)
    pol = _policy(P, hid, L, rng, seed=B % 7 + 1)
    if source == "compact":
        P.set_rollout_compact(True)
        ds, allc = _from_rollout(P, pol, 512, 12)
        # engine states share many rows (inactive quads, repeated meshes): few of them are off the kink, so the minibatch
        # draws with replacement from those that are (a minibatch may repeat samples; the kernels see 4096 tiles either way)
        pool = np.flatnonzero(_off_the_kink(pol.params, hid, L, allc.states))
        assert len(pool) >= 64
        sel0 = rng.choice(pool, size=B, replace=len(pool) < B)
    else:
        ds, allc = _by_shape(P, pol, rng, B, Q)
        sel0 = rng.permutation(B)
    c = allc.take(sel0)
    g64, olp, ole = _ref64(pol.params, hid, L, c)
    scale = np.abs(g64).max()
    assert scale > 0
    rec = dict(case="parity", Q=Q, HID=hid, L=L, B=B, source=source)
    modes = (1, 0) if L == 2 else (None,)                     # L = 2: the default split backward, then the fp32-MFMA one
    out = {}
    for mode in modes:
        if mode is not None:
            P.set_bwd_split_bf16(mode)
        _assert_route(P, "f32", 1 if mode is None else mode, Q, hid, L, B, source == "compact",
                      PARITY_ROUTE[(Q, hid, L, B)] if mode != 0 else None)
        lp, le = P.forward_backward(pol, ds, sel0 + 1, EPS, ENT)
        g = pol.grad()
        err = np.abs(g - g64).max() / scale
        rec["err_split" if mode == 1 else "err_fp32_mfma" if mode == 0 else "err"] = float(err)
        assert err <= BAR, rec
        assert abs(lp - olp) <= 1e-5 * (1 + abs(olp)) and abs(le - ole) <= 1e-5 * (1 + abs(ole)), (lp, olp, le, ole)
        P.forward_backward(pol, ds, sel0 + 1, EPS, ENT)
        assert np.array_equal(g, pol.grad()), "fixed-order reductions: a second identical launch is bitwise equal"
        out[mode] = g
    P.set_bwd_split_bf16(None)
    if L == 2:
        rec["diff"] = float(np.abs(out[1] - out[0]).max() / scale)
        assert rec["diff"] <= 4e-6, rec
    # teeth, measured and recorded but not asserted: min over 8 sampled states of (the state's float64 contribution to the
    # mean, max over elements) / (the bar).  At these sizes it is of order 1, not above 10: the largest gradient elements
    # (W3 / b3) are sums of terms of one sign over all B states (the entropy term pulls every state's logits the same way),
    # while a state with a small |advantage| contributes far less than 1/B of them.  So a lost or doubled tile is not
    # guaranteed to cross the 2e-5 bar here; every shape of this list has a device-against-device case in
    # test_bench_shape_additivity, which asserts its own teeth.
    rec["teeth"] = float(_teeth64(pol.params, hid, L, c, rng, g64))
    _record(rec)


# ---------------------------------------------------------------- (b) additivity at the largest launches
def _tau(d1, slices, n_chunks, B, m_s, M):
    """Tolerance of max|g_full - sum_c g_c| / max|g_full|, derived.  Both sides sum the SAME per-row fp32 products: every
    per-sample value (probabilities, dY, dZ) depends on that sample and B_global only, so it is rounded identically on both
    sides, also in bf16 mode.  Only the grouping of the fp32 additions differs: which backward workgroup (slab) accumulates
    which tiles, how the slabs combine, and the fp32 rounding of each chunk's result (the host adds the chunks in float64).
    Every rounding error is at most U32 times the partial sum it rounds, and the errors are independent with mean zero, so
    they add in quadrature.  Partial sums of an element are bounded by R M, R = max(1, sqrt(B) m_s / M): per-state terms of
    size m_s with independent signs stay within sqrt(B) m_s, terms of one sign within the final value M.
      stage 1: a chain of d1 additions per slab, its partials at most R M / slices, over `slices` independent slabs:
               U32 R M sqrt(d1 / slices)
      stage 2: the fixed 8-way-interleaved slab tree (log2(slices) + 4 additions reach the top partials) and the rounding of
               the n_chunks chunk results: U32 R M sqrt(log2(slices) + 4 + n_chunks)
    6 standard deviations on each of the two sides keep the ~10^5 elements clear of a false alarm (P(|z| > 6) = 2e-9)."""
    R = max(1.0, np.sqrt(B) * m_s / M)
    sigma = U32 * R * (np.sqrt(d1 / slices) + np.sqrt(np.log2(slices) + 4 + n_chunks))
    return 2 * 6 * sigma


def _chain(mode, hid, L, tiles):
    """(d1, slices) of _tau.  The fused backward (L = 2) gives each of its 256 (HID = 256) or 512 (HID = 128) workgroups a
    contiguous share of the tiles and keeps a slab per workgroup (256 is taken for both: fewer slabs, longer chains); the
    layer-looped weight gradients (L = 1, 3) split the rows over 512 / blocks K-slices (ppo_policy_bwd_small.hip).  A row
    adds one product per element, the split-fp32 form up to six bf16 piece products."""
    if L == 2:
        slices, per_row = 256, (6 if mode in ("split", "compact") else 1)
    else:
        nt = hid // 32
        slices, per_row = max(1, 512 // ((L - 1) * (nt // 2) ** 2 + nt)), 1
    return 32 * per_row * -(-tiles // slices), slices


# (mode, Q, HID, L, states, chunkings): a chunking is the list of chunk lengths.  512 x 8 at 4096 states are exactly the 8-way
# strong-scaling shard launches; 1535 + 1537 + 1024 and 1023 + 1025 + 2 x 1024 put chunks on both sides of the split train
# forward's switch; every float64-parity shape of part (a) has its additivity case here (see the teeth note there).
ADDITIVITY = [
    ("split", 8, 256, 2, 4096, ([512] * 8, [1024] * 4, [1535, 1537, 1024])),
    ("compact", 8, 256, 2, 4096, ([512] * 8,)),
    ("split", 8, 128, 2, 4096, ([512] * 8, [1023, 1025, 1024, 1024])),
    ("split", 32, 256, 2, 8192, ([1024] * 8,)),
    ("split", 32, 128, 2, 1024, ([256] * 4,)),
    ("split", 8, 256, 3, 4096, ([512] * 8,)),
    ("split", 8, 256, 1, 4096, ([512] * 8,)),
    ("bf16", 8, 256, 2, 65536, ([4096] * 16,)),
]


@pytest.mark.parametrize("mode,Q,hid,L,B,chunkings", ADDITIVITY, ids=["%s-Q%d-h%d-L%d-%d" % c[:5] for c in ADDITIVITY])
def test_bench_shape_additivity(P, knobs, mode, Q, hid, L, B, chunkings):
    """forward_backward over all B states against the sum of forward_backward over chunks with B_global = B.  Plus, in bf16
    mode, one 4096-state chunk against the float64 restatement of the bf16 arithmetic at the bf16 bars."""
    rng = np.random.default_rng(B + Q + hid + L)
    if mode == "bf16":
        # the config-5 dataset: 65536 envs of the built-in game under a bf16 policy (test_bf16_config5_size_properties)
        pol = P.HipPolicy(F, hid, 2, 4, seed=1, dtype="bf16")
        ds, allc = _from_rollout(P, pol, 65536, 2)
        sel0 = rng.choice(len(ds), size=B, replace=False)
    elif mode == "compact":
        P.set_rollout_compact(True)
        pol = _policy(P, hid, L, rng, seed=3)
        ds, allc = _from_rollout(P, pol, 512, 12)
        sel0 = rng.choice(len(ds), size=B, replace=False)
    else:
        pol = _policy(P, hid, L, rng, seed=3)
        ds, allc = _by_shape(P, pol, rng, B, Q, kink=False, ratio=(1, 1))      # device against device: the kink does not matter
        sel0 = rng.permutation(B)
    dtype, compact = ("bf16" if mode == "bf16" else "f32"), mode == "compact"
    for n in {B, 1} | {n for c in chunkings for n in c}:
        _assert_route(P, dtype, 1, Q, hid, L, n, compact)
    lp, le = P.forward_backward(pol, ds, sel0 + 1, EPS, ENT)
    g_full = pol.grad().astype(np.float64)
    M = np.abs(g_full).max()
    # one-state launches with B_global = B: what dropping / doubling that state's tile changes
    m = []
    for s in rng.choice(B, size=8, replace=False):
        P.forward_backward(pol, ds, [sel0[s] + 1], EPS, ENT, B_global=B)
        m.append(np.abs(pol.grad()).max())
    m_min, m_mean = float(min(m)), float(np.mean(m))
    d1, slices = _chain(mode, hid, L, B * Q // 8)
    tau = _tau(d1, slices, max(len(c) for c in chunkings), B, m_mean, M)
    rec = dict(case="additivity", mode=mode, Q=Q, HID=hid, L=L, B=B, tau=tau, min_single_state=m_min / M)
    # teeth: losing or doubling any one sampled state's tile moves the gradient by >= 10 tau max|g_full|
    assert tau * M <= 0.1 * m_min, rec
    for chunks in chunkings:
        assert sum(chunks) == B
        g_sum = np.zeros_like(g_full)
        l_sum = [0.0, 0.0]
        l_abs = abs(lp) + abs(le)
        s = 0
        for n in chunks:
            l1, l2 = P.forward_backward(pol, ds, sel0[s:s + n] + 1, EPS, ENT, B_global=B)
            g_sum += pol.grad()
            l_sum[0] += l1
            l_sum[1] += l2
            l_abs += abs(l1) + abs(l2)
            if mode == "bf16" and s == 0 and chunks is chunkings[0]:
                gc = pol.grad()
                c = allc.take(sel0[:n])
                g16, olp, ole = np_oracle.step_batch_grad_bf16(pol.params, F, hid, c.states, np_oracle.batch_masks(c.active, Q),
                                                                c.a0, c.p_old, c.adv, EPS, ENT, B_global=B)
                sc = np.abs(g16).max()
                rec["chunk_err_bf16"] = float(np.abs(gc - g16).max() / sc)
                rec["chunk_l2_bf16"] = float(np.linalg.norm(gc - g16) / np.linalg.norm(g16))
                # the bars of tests/test_gpu_bf16.py: 1 % of max|g| per element, 0.3 % in the 2-norm, losses 2e-3
                assert rec["chunk_err_bf16"] <= 1e-2 and rec["chunk_l2_bf16"] <= 3e-3, rec
                assert abs(l1 - olp) <= 2e-3 * (1 + abs(olp)) and abs(l2 - ole) <= 2e-3 * (1 + abs(ole)), (l1, olp, l2, ole)
            s += n
        err = float(np.abs(g_sum - g_full).max() / M)
        rec["err_%s" % "+".join(map(str, sorted(set(chunks))))] = err
        _record(rec)
        assert err <= tau, rec
        # losses: per-sample terms are float64 and identical on both sides, summed in float64; each of the 1 + len(chunks)
        # values is then rounded to fp32 once (at most U32 / 2 of itself): the difference is within U32 / 2 of their magnitudes
        assert abs(l_sum[0] - lp) <= 0.5 * U32 * l_abs + 1e-12 and abs(l_sum[1] - le) <= 0.5 * U32 * l_abs + 1e-12, \
            (l_sum, lp, le)


# ---------------------------------------------------------------- (c) the optimiser step of the benchmark
@pytest.fixture(scope="module")
def world1(P):
    """A one-rank process group: ppo_train then takes the unfused path (slab reduction, all-reduce hook, k_adam)."""
    import socket
    import torch.distributed as dist
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
    try:
        yield lambda: P.DataParallel(0, 1, force_hook=True)
    finally:
        P.rccl_finalize()
        dist.destroy_process_group()


STEP = [(256, "f32", 1), (128, "f32", 1), (256, "f32", 0), (256, "bf16", None)]


def _bench_step(P, orc, hid, dtype, parallel, split):
    rng = np.random.default_rng(hid + (dtype == "bf16"))
    B = 4096
    pol = _policy(P, hid, 2, rng, dtype=dtype, seed=5)
    p0 = pol.params.copy()
    ds, c = _by_shape(P, pol, rng, B, 8, kink=False)
    assert len(ds) == B
    perm = (rng.permutation(B) + 1)[None]
    _assert_route(P, dtype, 1 if split is None else split, 8, hid, 2, B)
    # the reference: forward_backward on an identical copy of the pre-step policy, the oracle's Adam on its gradient
    ref = P.HipPolicy(F, hid, 2, 4, dtype=dtype)
    ref.params = p0
    lp, le = P.forward_backward(ref, ds, perm[0], EPS, ENT)
    g = ref.grad()
    pp, mm, vv, bp = p0.copy(), np.zeros_like(p0), np.zeros_like(p0), np.array([0.9, 0.999])
    orc.adam_step(pp, g, mm, vv, bp, 1e-4)
    opt = P.Optimiser(P.Adam(1e-4))
    ph, eh, _ = P.ppo_train_(pol, opt, ds, EPS, B, 1, ENT, perm=perm, parallel=parallel, verbose=False)
    if parallel is not None:
        import torch
        torch.cuda.synchronize()
        assert parallel.hook_kind is not None, "the unfused path ran through the all-reduce hook"
    trained = pol.params
    assert not np.array_equal(trained, p0)
    assert np.array_equal(trained, pp), "parameters after one ppo_train! step == oracle Adam on forward_backward's gradient"
    m, v, bpd = opt.members[0].get_state()
    assert np.array_equal(m, mm) and np.array_equal(v, vv) and np.array_equal(bpd, bp), "Adam moments"
    assert ph == [lp] and eh == [le], "loss history == the losses forward_backward returned"
    # re-pack pin: a fresh policy packed by set_params from the trained parameters runs the same forward and backward
    fresh = P.HipPolicy(F, hid, 2, 4, dtype=dtype)
    fresh.params = trained
    probe = P.StateData(c.states[:256], c.active[:256])
    assert np.array_equal(P.batch_action_probabilities(pol, probe), P.batch_action_probabilities(fresh, probe)), \
        "rollout forward packs after the step == packs written by set_params"
    P.forward_backward(pol, ds, perm[0], EPS, ENT)
    g1 = pol.grad()
    P.forward_backward(fresh, ds, perm[0], EPS, ENT)
    assert np.array_equal(g1, fresh.grad()), "train forward / backward packs after the step == packs written by set_params"


@pytest.mark.parametrize("hid,dtype,split", STEP, ids=["h%d-%s-split%s" % s for s in STEP])
def test_bench_optimiser_step_fused(P, orc, knobs, hid, dtype, split):
    """World 1: the gradient reduction, Adam and the re-pack in one launch (k_reduce_adam).  The fused launch reduces the
    slabs in the same order as forward_backward's own reduction (it is the same kernel, with Adam switched on), so the
    gradient it steps with is forward_backward's bit for bit."""
    if split is not None:
        P.set_bwd_split_bf16(split)
    _bench_step(P, orc, hid, dtype, None, split)


@pytest.mark.parametrize("hid,dtype,split", STEP, ids=["h%d-%s-split%s" % s for s in STEP])
def test_bench_optimiser_step_unfused(P, orc, knobs, world1, hid, dtype, split):
    """The same step through the all-reduce hook (one rank: the sum is the identity), then a separate k_adam launch."""
    if split is not None:
        P.set_bwd_split_bf16(split)
    _bench_step(P, orc, hid, dtype, world1(), split)
