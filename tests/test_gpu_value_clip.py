"""The critic's PPO-clipped value loss on the GPU: the value-train tail's clipped form (csrc/ppo_policy_tail.h) in every
value-train instantiation, the per-epoch value-clip statistics (k_value_clip_stats), the handle property and the refusals.
Reference: the float64 restatement tests/value_clip_ref.py.  The host puts the old values into the buffer with compute_gae_ and
the targets with set_columns, so every state is, by construction, at least 0.2 c away from |V - V_old| = c and every outside
state at least 0.4 c from the tie of the two squares: fp32 and float64 cannot disagree about a branch.
TEST_RECORD_DIR=<dir>: measured figures go to <dir>/value_clip.jsonl."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import value_clip_ref
import value_ref
from test_value_host import value_route

pytestmark = pytest.mark.gpu

BAR = 2e-5                                   # the bar of every fp32 gradient test of the project
CLIP = 0.5
# (F, hidden, L, H): the 128 kernel, the headline width, a deep critic, the wide rows, four tiles per state
SHAPES = [(72, 128, 2, 32), (72, 256, 2, 32), (72, 128, 3, 32), (216, 128, 2, 32), (72, 128, 2, 128)]
KEYS = ["entropy", "lr", "ppo", "value"]


@pytest.fixture(scope="module")
def P(ppo):
    if ppo.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests must run on the GPU box")
    return ppo


@pytest.fixture()
def knobs(P):
    yield P
    P.set_rollout_compact(None)
    P.set_bwd_split_bf16(None)


def _record(rec):
    print(json.dumps(rec))
    d = os.environ.get("TEST_RECORD_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "value_clip.jsonl"), "a") as f:
            f.write(json.dumps(rec) + "\n")


def _debug(P):
    L = P._lib.lib()
    L.ppo_debug_train_outputs.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.ppo_debug_train_outputs.restype = C.c_int32
    L.ppo_debug_value_deltas.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.ppo_debug_value_deltas.restype = C.c_int32
    return L


# ---------------------------------------------------------------- inputs and references, computed once per (shape, size, clip)
@functools.lru_cache(maxsize=None)
def _case(F, hid, L, H, B, c):
    """Parameters, B states off leakyrelu's kink (one without an active quad, one fully active), and old values / targets in
    the three regimes around the float64 values -- with the float64 preconditions asserted before any device call."""
    import ppo_amd as ppo
    rng = np.random.default_rng(9000 + F + hid + L + H + B)
    params = (ppo.glorot_uniform_params(F, hid, L, 4, seed=5) + (rng.normal(size=ppo.glorot_uniform_params(F, hid, L, 4).size) * 0.03).astype(np.float32)).astype(np.float32)
    parts, have = [], 0
    while have < B:
        cand = rng.integers(-3, 7, size=(B - have + B // 8 + 16, H, F)).astype(np.int8)
        cand = cand[value_ref.off_the_kink(params, F, hid, L, cand)]
        parts.append(cand)
        have += len(cand)
    states = np.ascontiguousarray(np.concatenate(parts)[:B])
    active = rng.integers(0, 2 ** (H // 4), size=B, dtype=np.uint64).astype(np.uint32)
    active[:3] = (0, 1, 2 ** (H // 4) - 1)
    v64 = value_ref.values_np(params, F, hid, L, states, active)
    v_old, t, regime = value_clip_ref.make_regimes(rng, v64, c)
    b = value_clip_ref.check_margins(v64, v_old, t, c, regime)
    case = dict(F=F, hid=hid, L=L, H=H, B=B, c=c, params=params, states=states, active=active, v64=v64, v_old=v_old, t=t,
                regime=regime, branches=b)
    for a in (params, states, active, v64, v_old, t, regime):
        a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def _ref(F, hid, L, H, B, c, Bg):
    k = _case(F, hid, L, H, B, c)
    loss, g, v = value_clip_ref.loss_grad(k["params"], F, hid, L, k["states"], k["active"], k["t"], k["v_old"], c, B_global=Bg)
    assert float(np.abs(g).max()) > 1e-4
    g.setflags(write=False)
    return loss, g


def _device(P, k):
    """critic + dataset of a case: states in a [2, B/2] buffer, the targets as its returns column, the old values through
    compute_gae_ (row T of the values is the bootstrap row: zeros)."""
    critic = P.HipCritic(k["F"], k["hid"], k["L"], seed=5)
    critic.params = k["params"]
    B, H, F = k["B"], k["H"], k["F"]
    T, N = 2, B // 2
    ro = P.BufferRollouts()
    ro.set_columns(None, k["states"].reshape(T, N, H, F), k["active"].reshape(T, N), np.ones((T, N), np.int64), np.ones((T, N), np.float32),
                   k["t"].reshape(T, N), np.zeros((T, N), np.uint8))
    values = np.concatenate([k["v_old"].reshape(T, N), np.zeros((1, N), np.float32)])
    P.compute_gae_(ro, values, 0.99, 0.95)
    return critic, ro, P.construct_dataset(ro)


# ---------------------------------------------------------------- 1. per-state tail output
@pytest.mark.parametrize("B", [64, 1000])
@pytest.mark.parametrize("F,hid,L,H", SHAPES)
def test_tail_output_per_state(P, F, hid, L, H, B):
    """After value_forward_backward with the clip set: the states whose dY rows are all exactly 0.0f are the reference's
    clipped-away states plus the ones without an active quad (no state on the wrong branch); the other dY is within
    2e-5 max|dY64|; every loss term is within 1e-5 relative; rows of inactive quads are exactly zero."""
    k = _case(F, hid, L, H, B, CLIP)
    critic, ro, ds = _device(P, k)
    critic.value_clip = CLIP
    assert critic.value_clip == CLIP
    P.value_forward_backward(critic, ds, np.arange(1, B + 1))
    tiles = B * (H // 32)
    dy, lt = np.zeros((tiles, 32, 4), np.float32), np.zeros((tiles, 2), np.float64)
    assert _debug(P).ppo_debug_train_outputs(critic._h, tiles, dy.ctypes.data, lt.ctypes.data) == 0, P._lib.last_error()
    dy = dy.reshape(B, H, 4)
    lt = lt.reshape(-1)[:2 * B].reshape(B, 2)                          # one pair per STATE, in front of the buffer
    dy64 = value_clip_ref.analytic_dy(k["v64"], k["active"], k["t"], k["v_old"], CLIP, B, H)
    zero_dev = ~dy.reshape(B, -1).any(axis=1)
    zero_ref = (k["regime"] == value_clip_ref.CLIPPED) | (k["active"] == 0)
    assert np.array_equal(zero_dev, zero_ref), np.flatnonzero(zero_dev != zero_ref)
    assert not np.signbit(dy[zero_dev]).any(), "exactly 0.0f"
    dmax = float(np.abs(dy64).max())
    err = float(np.abs(dy - dy64).max())
    lt64 = -(k["branches"]["term"] ** 2)
    lerr = float((np.abs(lt[:, 0] - lt64) / np.abs(lt64)).max())
    _record({"case": "tail", "shape": [F, hid, L, H], "B": B, "dy_err_over_max": err / dmax, "loss_term_rel_err": lerr})
    assert err <= BAR * dmax
    assert lerr <= 1e-5
    assert not lt[:, 1].any()
    assert np.all(dy[~value_ref.row_mask(k["active"], H)] == 0.0)


# ---------------------------------------------------------------- 2. gradient against float64
def _gradient_check(P, k, critic, ds, sel, c, Bg, label):
    F, hid, L, H, B = k["F"], k["hid"], k["L"], k["H"], k["B"]
    loss = P.value_forward_backward(critic, ds, sel, B_global=Bg)
    g = critic.grad()
    loss2 = P.value_forward_backward(critic, ds, sel, B_global=Bg)
    assert g.tobytes() == critic.grad().tobytes() and loss == loss2, "a second call repeats the first bit for bit"
    l64, g64 = _ref(F, hid, L, H, B, c, Bg)
    gmax = float(np.abs(g64).max())
    err = float(np.abs(g - g64).max())
    _record({"case": "gradient", "shape": [F, hid, L, H], "B": B, "B_global": Bg, "clip": c, "knobs": label, "max_abs_g64": gmax,
             "err_over_max": err / gmax, "loss": loss, "loss64": l64})
    assert gmax > 1e-4
    assert err <= BAR * gmax + 1e-9, (label, err, gmax)
    assert abs(loss - l64) <= 1e-5 * max(1.0, abs(l64))


@pytest.mark.parametrize("F,hid,L,H", SHAPES)
def test_clipped_gradient_against_float64(knobs, F, hid, L, H):
    """max|g - g64| <= 2e-5 max|g64| + 1e-9 and the loss within 1e-5 max(1, |l64|): 64 states under the default knobs and with
    the split-fp32 kernels off (three-product backward), 1000 states under the default knobs, B_global = 3B once, the clip
    np.float32(0.2) once; a second call repeats the first bit for bit; the route is the one ppo_debug_value_route names (its
    forward in the clipped form: k_policy_fwd mode 9 for 6)."""
    P = knobs
    hk = 128 if hid <= 128 else 256
    for B, split, Bg_mul, c in ((64, None, 1, CLIP), (64, 0, 3, CLIP), (1000, None, 1, CLIP), (64, None, 1, float(np.float32(0.2)))):
        k = _case(F, hid, L, H, B, c)
        critic, ro, ds = _device(P, k)
        critic.value_clip = np.float32(c)
        assert critic.value_clip == c
        P.set_bwd_split_bf16(split)
        fwd, bwd = value_route(P, "f32", F, hk, L, H, False, B)
        assert fwd == "k_policy_fwd<%d,%d,6,%d,%d>" % (F, hk, H // 32, int(L != 2)), fwd
        assert split is None or bwd.startswith("k_policy_bwd_data"), bwd
        _gradient_check(P, k, critic, ds, np.arange(1, B + 1), c, Bg_mul * B, "%s/%s" % (split, bwd))
        P.set_bwd_split_bf16(None)
        assert np.array_equal(critic.params, k["params"]), "forward_backward does not touch the parameters"


# ---------------------------------------------------------------- 3. off means off
def test_off_means_off(P):
    """One minibatch: gradient and loss are byte-identical between value_clip = None, 1e30 and inf; and for 1e-3 right after
    compute_values_ with the same, unmodified critic (V - V_old is then zero or rounding-sized)."""
    k = _case(72, 128, 2, 32, 1000, CLIP)
    critic, ro, ds = _device(P, k)
    sel = np.random.default_rng(3).permutation(1000)[:700] + 1
    out = []
    for c in (None, 1e30, float("inf"), None):
        critic.value_clip = c
        assert critic.value_clip == c
        loss = P.value_forward_backward(critic, ds, sel)
        out.append((loss, critic.grad().tobytes()))
    assert out[0] == out[1] == out[2] == out[3]
    assert np.abs(critic.grad()).max() > 1e-4
    critic.value_clip = CLIP                                           # the clip does bite on these inputs
    assert P.value_forward_backward(critic, ds, sel) != out[0][0] and critic.grad().tobytes() != out[0][1]
    P.compute_values_(ro, None, critic)
    critic.value_clip = 1e-3
    assert (P.value_forward_backward(critic, ds, sel), critic.grad().tobytes()) == out[0]


# ---------------------------------------------------------------- 4. storage forms
def test_clipped_gradient_from_both_storage_forms(knobs):
    """Rollouts collected in the expanded and in the compact form (value-train modes 6 and 8, clipped: 9 and 10), values from a critic whose
    parameters are then perturbed, c = 0.05: the clipped gradients of the two forms agree bit for bit, differ from the
    unclipped one, and some state is clipped."""
    P = knobs
    for hid, L in ((128, 2), (256, 2), (128, 3)):
        rng = np.random.default_rng(hid + L)
        critic = P.HipCritic(72, hid, L, seed=5)
        p0 = (critic.params + (rng.normal(size=critic.num_params) * 0.03).astype(np.float32)).astype(np.float32)
        p1 = (p0 + (rng.normal(size=p0.size) * 0.01).astype(np.float32)).astype(np.float32)
        grads, plain = [], []
        for compact in (0, 1):
            P.set_rollout_compact(compact)
            env = P.HipVecEnv(num_envs=64, Q=8, max_actions=9, seed=12)
            pol = P.HipPolicy(72, 128, 2, 4, seed=4)
            ro = P.BufferRollouts()
            P.collect_rollouts_steps_(ro, env, pol, 24, 0.99)
            ds = P.construct_dataset(ro)
            sel = np.random.default_rng(1).permutation(len(ds))[:700]
            assert value_route(P, "f32", 72, hid, L, 32, bool(compact), 700)[0] == "k_policy_fwd<72,%d,%d,1,%d>" % (hid, 8 if compact else 6, int(L != 2))
            critic.params = p0
            critic.value_clip = None
            v_old = P.compute_values_(ro, env, critic)
            critic.params = p1
            P.value_forward_backward(critic, ds, sel + 1)
            plain.append(critic.grad())
            critic.value_clip = 0.05
            P.value_forward_backward(critic, ds, sel + 1)
            grads.append(critic.grad())
        assert grads[0].tobytes() == grads[1].tobytes() and plain[0].tobytes() == plain[1].tobytes()
        assert grads[0].tobytes() != plain[0].tobytes() and np.all(np.isfinite(grads[0])) and np.abs(grads[0]).max() > 0


# ---------------------------------------------------------------- 5. statistics
def _adam_state(opt):
    m = opt.get_state()["members"][0]
    return (m["m"].tobytes(), m["v"].tobytes(), m["beta_pow"].tobytes())


def test_value_clip_statistics(P):
    """value_train_ with Descent(0.0), one epoch, 1000 states in minibatches of 256 (short last slice), seeded order:
    clip_fraction is the reference's count over 1000 exactly; mean_sq_change is the float64 sum of the squares of the device's
    own deltas (ppo_debug_value_deltas) to 1e-12 relative; those deltas are within 1e-5 max(1, |V64|) of V64 - V_old (section
    7a of DESIGN.md measured 4.4e-7 for fp32 values against a float64 forward: a factor of twenty).  Then four epochs of
    Adam(3e-4): two runs from one start are bit-identical in parameters, moments and statistics; inf equals None byte for byte
    in parameters and moments and has finite statistics; None reports NaN statistics and epochs_run == 4."""
    k = _case(72, 128, 2, 32, 1000, CLIP)
    B = 1000
    critic, ro, ds = _device(P, k)
    critic.value_clip = CLIP
    perm = np.random.default_rng(55).permutation(B)
    P.value_train_(critic, P.Optimiser(P.Descent(0.0)), ds, 256, 1, perm=perm[None] + 1, verbose=False)
    assert np.array_equal(critic.params, k["params"])
    st = critic.last_value_stats()
    assert st["epochs_run"] == 1 and len(st["clip_fraction"]) == 1 and len(st["mean_sq_change"]) == 1
    outside = int(np.count_nonzero(k["regime"] != value_clip_ref.INSIDE))
    want = outside / B
    assert st["clip_fraction"][0] == want, (st, want)
    d = np.zeros(B, np.float32)
    assert _debug(P).ppo_debug_value_deltas(critic._h, B, d.ctypes.data) == 0, P._lib.last_error()
    msq = float(np.sum(d.astype(np.float64) ** 2)) / B
    assert abs(st["mean_sq_change"][0] - msq) <= 1e-12 * msq
    d64 = (k["v64"] - k["v_old"].astype(np.float64))[perm]
    derr = np.abs(d - d64) / np.maximum(1.0, np.abs(k["v64"][perm]))
    _record({"case": "statistics", "clip_fraction": st["clip_fraction"][0], "mean_sq_change": st["mean_sq_change"][0],
             "max_delta_err": float(derr.max())})
    assert np.all(derr <= 1e-5)
    assert np.count_nonzero(np.abs(d) > np.float32(CLIP)) == outside
    assert _debug(P).ppo_debug_value_deltas(critic._h, B + 1, d.ctypes.data) == -1

    perms = np.stack([np.random.default_rng(60 + e).permutation(B) for e in range(4)]) + 1
    runs = {}
    for name, c in (("a", CLIP), ("b", CLIP), ("inf", float("inf")), ("none", None)):
        critic.params = k["params"]
        critic.value_clip = c
        opt = P.Optimiser(P.Adam(3e-4))
        hist, _ = P.value_train_(critic, opt, ds, 256, 4, perm=perms, verbose=False)
        runs[name] = (critic.params.tobytes(), _adam_state(opt), critic.last_value_stats(), hist)
    assert runs["a"] == runs["b"]
    assert runs["a"][2]["epochs_run"] == 4 and np.all(np.isfinite(runs["a"][2]["clip_fraction"])) and np.all(np.isfinite(runs["a"][2]["mean_sq_change"]))
    assert runs["a"][0] != runs["none"][0] and all(0.0 < x < 1.0 for x in runs["a"][2]["clip_fraction"])
    assert runs["inf"][:2] == runs["none"][:2] and runs["inf"][3] == runs["none"][3]
    si, sn = runs["inf"][2], runs["none"][2]
    assert si["epochs_run"] == 4 and np.all(np.isfinite(si["clip_fraction"])) and np.all(np.isfinite(si["mean_sq_change"]))
    assert si["clip_fraction"] == [0.0] * 4 and min(si["mean_sq_change"]) > 0
    assert sn["epochs_run"] == 4 and np.all(np.isnan(sn["clip_fraction"])) and np.all(np.isnan(sn["mean_sq_change"]))


# ---------------------------------------------------------------- 6. refusals
def test_refusals(P):
    needs = "value clipping needs ppo_rollouts_compute_values or ppo_rollouts_compute_gae on these rollouts first"
    env = P.HipVecEnv(num_envs=8, Q=8, max_actions=5, seed=1)
    pol = P.HipPolicy(72, 128, 2, 4, seed=1)
    ro = P.BufferRollouts()
    P.collect_rollouts_steps_(ro, env, pol, 6, 1.0)
    ds = P.construct_dataset(ro)
    idx = np.arange(1, 9)
    critic = P.HipCritic(72, 128, 2, seed=3)
    assert critic.value_clip is None
    P.value_forward_backward(critic, ds, idx)
    g0 = critic.grad()
    assert np.abs(g0).max() > 0
    critic.value_clip = 0.2
    calls = (lambda: P.value_forward_backward(critic, ds, idx), lambda: P.value_train_(critic, P.Optimiser(P.Adam()), ds, 8, 1, verbose=False))
    for call in calls:                                     # no values yet
        with pytest.raises(P.PPOError, match=needs):
            call()
        assert critic.grad().tobytes() == g0.tobytes()
    P.compute_values_(ro, env, critic)
    assert np.isfinite(P.value_forward_backward(critic, ds, idx))
    P.collect_rollouts_steps_(ro, env, pol, 6, 1.0)        # a new collection into the same buffer: the values are stale
    ds = P.construct_dataset(ro)
    g1 = critic.grad()
    for call in calls:
        with pytest.raises(P.PPOError, match=needs):
            call()
        assert critic.grad().tobytes() == g1.tobytes()
    P.compute_gae_critic_(ro, env, critic, 0.99, 0.95, fetch=False)
    assert np.isfinite(P.value_forward_backward(critic, ds, idx))
    for bad in (-0.5, float("nan")):
        with pytest.raises(P.PPOError, match="value_clip must be"):
            critic.value_clip = bad
        assert P._lib.lib().ppo_policy_set_value_clip(critic._h, bad) == -1
        assert critic.value_clip == 0.2
    critic.value_clip = None
    assert critic.value_clip is None
    bf = P.HipPolicy(72, 128, 2, 4, seed=1, dtype="bf16")  # a bf16 critic stays refused with today's text, clip or not
    bf.value_clip = 0.2
    with pytest.raises(P.PPOError, match="a bf16-dtype critic is not supported"):
        P.value_forward_backward(bf, ds, idx)


# ---------------------------------------------------------------- 7. ppo_iterate_
class _Evaluator:
    def __init__(self):
        self.calls = 0

    def __call__(self, policy, env, optimizer):
        self.calls += 1


def test_ppo_iterate_reports_the_clip_fraction(P):
    P.save_loss.register(_Evaluator)(lambda ev, loss: None)
    for clip in (0.2, None):
        env = P.HipVecEnv(num_envs=64, Q=8, max_actions=8, seed=21)
        pol, opt = P.HipPolicy(72, 128, 2, 4, seed=3), P.Optimiser(P.Adam(3e-4))
        critic, copt = P.HipCritic(72, 128, 2, seed=4), P.Optimiser(P.Adam(1e-3))
        critic.value_clip = clip
        loss = P.ppo_iterate_(pol, env, opt, 64, 64, 2, _Evaluator(), 2, 0.99, 0.05, 0.01, verbose=False, critic=critic,
                              critic_optimizer=copt, value_epochs=3)
        if clip is None:
            assert sorted(loss) == KEYS
            continue
        assert sorted(loss) == sorted(KEYS + ["value_clip_fraction"])
        cf = loss["value_clip_fraction"]
        assert len(cf) == 2 * 3 and len(loss["value"]) == 6 and all(0.0 <= x <= 1.0 for x in cf)
        assert np.all(np.isfinite(loss["value"]))
        # the latest value_train_'s own deltas: what its last epoch reported is their count
        n = critic.last_value_stats()
        assert n["epochs_run"] == 3 and n["clip_fraction"] == cf[3:]
