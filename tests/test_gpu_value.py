"""The device critic on the GPU: a Policy(F, hidden, L, 4) read as a state value (mean of the outputs of the active quads'
rows, 0 without one), its values feeding GAE without a host trip, and its training pass (k_policy_fwd value-train mode, then
the backward value_route picks).  References: the device-order oracle's logits (bit for bit the device's) pooled in float64,
and the float64 restatement tests/value_ref.py.  TEST_RECORD_DIR=<dir>: measured figures go to <dir>/value.jsonl."""
import json
import os

import numpy as np
import pytest

import value_ref
from test_value_host import value_route

pytestmark = pytest.mark.gpu

BAR = 2e-5                                   # tests/test_gpu_bench_shapes.py: BAR, the bar of every fp32 gradient test
U32 = 2.0 ** -24
# (F, hidden, L): the headline, the 128 kernel, a zero-padded width, the wide rows, a deep critic
SHAPES = [(72, 256, 2), (72, 128, 2), (72, 192, 2), (216, 128, 2), (72, 128, 3)]
# every shape at H = 32; H = 128 (four tiles per state) exists for F = 72 only (no kernel of the project takes F = 216 there)
SHAPE_H = [(F, hid, L, H) for (F, hid, L) in SHAPES for H in (32, 128) if not (F == 216 and H == 128)]


@pytest.fixture(scope="module")
def P(ppo):
    if ppo.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests must run on the GPU box")
    return ppo


@pytest.fixture()
def knobs(P):
    yield P
    P.set_rollout_compact(None)


def _record(rec):
    print(json.dumps(rec))
    d = os.environ.get("TEST_RECORD_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "value.jsonl"), "a") as f:
            f.write(json.dumps(rec) + "\n")


def _critic(P, F, hid, L, rng, seed=5):
    c = P.HipCritic(F, hid, L, seed=seed)
    c.params = (c.params + (rng.normal(size=c.num_params) * 0.03).astype(np.float32)).astype(np.float32)
    return c


def _masks(rng, B, H):
    """fully active, one quad, none, then random masks"""
    Q = H // 4
    m = rng.integers(0, 2 ** Q, size=B, dtype=np.uint64).astype(np.uint32)
    m[0], m[1], m[2], m[3] = 2 ** Q - 1, 1, 0, 1 << (Q - 1)
    return m


# ---------------------------------------------------------------- 5. values against the device-order logits
@pytest.mark.parametrize("F,hid,L,H", SHAPE_H)
def test_values_against_device_order_logits(P, orc, F, hid, L, H):
    """|V_dev - V_ref| <= 2^-24 ((n - 1) sum|y| / n + |V_ref|), n = 4 * active rows: the worst case of an n-term fp32 sum in
    any order divided by n, plus the rounding of the division -- V_ref pools the device-order oracle's fp32 logits (the
    device's own, bit for bit) in float64.  A state without an active quad returns exactly 0.0."""
    rng = np.random.default_rng(1000 + F + hid + L + H)
    c = _critic(P, F, hid, L, rng)
    p0 = c.params
    B = 21
    states = rng.integers(-3, 7, size=(B, H, F)).astype(np.int8)
    active = _masks(rng, B, H)
    v = P.batch_state_values(c, P.StateData(states, active))
    assert v.dtype == np.float32 and v.shape == (B,) and np.all(np.isfinite(v))
    on = value_ref.row_mask(active, H)
    worst = 0.0
    for b in range(B):
        y = orc.mlp_logits(p0, F, hid, states[b], "dev", L).astype(np.float64).reshape(H, 4)
        n = 4 * int(on[b].sum())
        if n == 0:
            assert v[b] == 0.0 and not np.signbit(v[b])
            continue
        ya = y[on[b]]
        vref = ya.sum() / n
        bound = U32 * ((n - 1) * np.abs(ya).sum() / n + abs(vref))
        worst = max(worst, abs(float(v[b]) - vref) / bound)
        assert abs(float(v[b]) - vref) <= bound, (b, n, float(v[b]), vref, bound)
    assert P.state_values(c, P.StateData(states[4], active[4])) == float(v[4])
    # the numbers nobody had measured: fp32 device values, and a plain numpy float32 forward, against float64
    v64 = value_ref.values_np(p0, F, hid, L, states, active)
    vnp = value_ref.values_np(p0, F, hid, L, states, active, np.float32)
    _record({"case": "values", "shape": [F, hid, L, H], "worst_fraction_of_bound": worst,
             "max_abs_dev_minus_f64": float(np.abs(v - v64).max()), "max_abs_numpy_f32_minus_f64": float(np.abs(vnp - v64).max()),
             "max_abs_value": float(np.abs(v64).max())})


# ---------------------------------------------------------------- 6 / 7. buffer values and GAE without the host
def _buffer_checks(P, ro, env, critic):
    T, N = ro.dims()
    v = P.compute_values_(ro, env, critic)
    st, act = ro.state_data
    H, F = st.shape[2], st.shape[3]
    ref = P.batch_state_values(critic, P.StateData(st.reshape(-1, H, F), act.reshape(-1))).reshape(T, N)
    assert v.shape == (T + 1, N)
    assert np.array_equal(v[:T].view(np.uint32), ref.view(np.uint32)), "rows 0..T-1: the stored states"
    now = P.state(env)
    last = P.batch_state_values(critic, P.StateData(np.asarray(now.vertex_score).reshape(N, H, F), np.atleast_1d(now.action_mask)))
    assert np.array_equal(v[T].view(np.uint32), last.view(np.uint32)), "row T: the state every env is in now"
    adv, ret = P.compute_gae_critic_(ro, env, critic, 0.99, 0.95)
    adv2, ret2 = P.compute_gae_(ro, v, 0.99, 0.95)
    assert adv.tobytes() == adv2.tobytes() and ret.tobytes() == ret2.tobytes()
    assert np.all(np.isfinite(adv)) and np.abs(adv).max() > 0
    assert P.compute_gae_critic_(ro, env, critic, 0.99, 0.95, fetch=False) is None
    return v


@pytest.mark.parametrize("hid,L", [(128, 2), (256, 2), (128, 3)])
@pytest.mark.parametrize("compact", [0, 1], ids=["expanded", "compact"])
def test_buffer_values_and_gae_steps(knobs, compact, hid, L):
    P = knobs
    P.set_rollout_compact(compact)
    rng = np.random.default_rng(60 + hid + L)
    env = P.HipVecEnv(num_envs=48, Q=8, max_actions=7, seed=31)
    pol = P.HipPolicy(72, hid, L, 4, seed=2)
    critic = _critic(P, 72, hid, L, rng)
    ro = P.BufferRollouts()
    P.collect_rollouts_steps_(ro, env, pol, 13, 0.99)
    _buffer_checks(P, ro, env, critic)


def test_buffer_values_and_gae_q32_and_episodes(knobs):
    P = knobs
    rng = np.random.default_rng(77)
    for compact in (0, 1):                               # four tiles per state, both storage forms
        P.set_rollout_compact(compact)
        env = P.HipVecEnv(num_envs=20, Q=32, max_actions=6, seed=5)
        pol = P.HipPolicy(72, 128, 2, 4, seed=2)
        ro = P.BufferRollouts()
        P.collect_rollouts_steps_(ro, env, pol, 5, 1.0)
        _buffer_checks(P, ro, env, _critic(P, 72, 128, 2, rng))
    P.set_rollout_compact(None)
    env = P.HipVecEnv(num_envs=16, Q=8, max_actions=6, seed=9)  # episodes form: whole episodes, idle envs, terminal envs at the end
    pol = P.HipPolicy(72, 128, 2, 4, seed=2)
    ro = P.BufferRollouts()
    P.collect_rollouts_(ro, env, pol, 40, 1.0)
    _buffer_checks(P, ro, env, _critic(P, 72, 128, 2, rng))


def test_values_without_env_bootstrap_from_zero(P):
    rng = np.random.default_rng(3)
    c = _critic(P, 216, 128, 2, rng)
    T, N = 3, 10
    st = rng.integers(-3, 7, size=(T, N, 32, 216)).astype(np.int8)
    act = rng.integers(1, 256, size=(T, N)).astype(np.uint32)
    ro = P.BufferRollouts()
    ro.set_columns(None, st, act, np.ones((T, N), np.int64), np.ones((T, N), np.float32), rng.normal(size=(T, N)).astype(np.float32),
                   np.zeros((T, N), np.uint8))
    v = P.compute_values_(ro, None, c)
    assert np.array_equal(v[:T].reshape(-1), P.batch_state_values(c, P.StateData(st.reshape(-1, 32, 216), act.reshape(-1))))
    assert not v[T].any()


# ---------------------------------------------------------------- 8. gradient against float64
def _value_dataset(P, critic, rng, B, F, hid, L, H):
    """B random states off leakyrelu's kink in a [2, B/2] buffer, returns ~ N(2, 1) (a target mean far from the critic's
    values keeps max|g64| away from zero), and a GAE call on host values so that the lambda-returns exist."""
    parts, have = [], 0
    while have < B:
        cand = rng.integers(-3, 7, size=(B - have + B // 8 + 16, H, F)).astype(np.int8)
        cand = cand[value_ref.off_the_kink(critic.params, F, hid, L, cand)]
        parts.append(cand)
        have += len(cand)
    states = np.ascontiguousarray(np.concatenate(parts)[:B])
    active = rng.integers(0, 2 ** (H // 4), size=B, dtype=np.uint64).astype(np.uint32)
    active[:3] = (0, 1, 2 ** (H // 4) - 1)
    returns = (rng.normal(size=B) + 2).astype(np.float32)
    T, N = 2, B // 2
    ro = P.BufferRollouts()
    ro.set_columns(None, states.reshape(T, N, H, F), active.reshape(T, N), np.ones((T, N), np.int64), np.ones((T, N), np.float32),
                   returns.reshape(T, N), np.zeros((T, N), np.uint8))
    _, lam = P.compute_gae_(ro, (rng.normal(size=(T + 1, N)) - 1).astype(np.float32), 0.99, 0.95)
    return P.construct_dataset(ro), states, active, {"returns": returns, "lambda_returns": lam.reshape(-1)}


@pytest.mark.parametrize("F,hid,L,H", SHAPE_H)
def test_value_gradient_against_float64(P, F, hid, L, H):
    """max|g - g64| <= 2e-5 max|g64| + 1e-9 at minibatches of 64 (default route and three-product backward), 4096 and 16384 states, both
    targets, B_global > B once per shape; the float64 gradient alone has max|g64| > 1e-4; a second call repeats the first bit
    for bit; the kernels are the ones value_route names."""
    rng = np.random.default_rng(8000 + F + hid + L + H)
    critic = _critic(P, F, hid, L, rng)
    p0 = critic.params
    ds, states, active, targets = _value_dataset(P, critic, rng, 16384, F, hid, L, H)
    order = rng.permutation(16384)
    hk = 128 if hid <= 128 else 256
    # 64 states twice: under the default knobs (an L = 2, F = 72 critic goes to the split-fp32 backward at every size) and with
    # the split kernels off, where 64 states take the three-product ("small") backward whatever the shape
    for B, split in ((64, None), (64, 0), (4096, None), (16384, None)):
        sel = np.sort(order[:B]) if B < 16384 else order
        P.set_bwd_split_bf16(split)
        try:
            fwd, bwd = value_route(P, "f32", F, hk, L, H, False, B)
            assert fwd == "k_policy_fwd<%d,%d,6,%d,%d>" % (F, hk, H // 32, int(L != 2)), fwd
            assert split is None or bwd.startswith("k_policy_bwd_data"), bwd
            for target in ("returns", "lambda_returns"):
                Bg = 3 * B if (B == 4096 and target == "returns") else B
                loss = P.value_forward_backward(critic, ds, sel + 1, target=target, B_global=Bg)
                g = critic.grad()
                loss2 = P.value_forward_backward(critic, ds, sel + 1, target=target, B_global=Bg)
                assert g.tobytes() == critic.grad().tobytes() and loss == loss2, "a second call repeats the first bit for bit"
                l64, g64, _ = value_ref.loss_grad(p0, F, hid, L, states[sel], active[sel], targets[target][sel], B_global=Bg)
                gmax = float(np.abs(g64).max())
                err = float(np.abs(g - g64).max())
                _record({"case": "gradient", "shape": [F, hid, L, H], "B": B, "B_global": Bg, "target": target, "bwd": bwd,
                         "max_abs_g64": gmax, "err_over_max": err / gmax, "loss": loss, "loss64": l64})
                assert gmax > 1e-4
                assert err <= BAR * gmax + 1e-9, (B, target, err, gmax)
                assert abs(loss - l64) <= 1e-5 * max(1.0, abs(l64))
        finally:
            P.set_bwd_split_bf16(None)
    assert np.array_equal(critic.params, p0), "forward_backward does not touch the parameters"


def test_value_gradient_from_compact_rollouts(knobs):
    """The value-train forward from env snapshots (mode 8) leaves the backward the same rows: gradients of the two storage
    forms of one rollout agree bit for bit, and with float64."""
    P = knobs
    rng = np.random.default_rng(88)
    grads = []
    for hid, L in ((128, 2), (256, 2), (128, 3)):
        critic = _critic(P, 72, hid, L, np.random.default_rng(hid + L))
        for compact in (0, 1):
            P.set_rollout_compact(compact)
            env = P.HipVecEnv(num_envs=64, Q=8, max_actions=9, seed=12)
            pol = P.HipPolicy(72, 128, 2, 4, seed=4)
            ro = P.BufferRollouts()
            P.collect_rollouts_steps_(ro, env, pol, 24, 0.99)
            ds = P.construct_dataset(ro)
            sel = np.random.default_rng(1).permutation(len(ds))[:700]
            assert value_route(P, "f32", 72, hid, L, 32, bool(compact), 700)[0] == "k_policy_fwd<72,%d,%d,1,%d>" % (hid, 8 if compact else 6, int(L != 2))
            P.value_forward_backward(critic, ds, sel + 1)
            grads.append(critic.grad())
        assert grads[-1].tobytes() == grads[-2].tobytes()
        st, act = ro.state_data
        ok = value_ref.off_the_kink(critic.params, 72, hid, L, st.reshape(-1, 32, 72)[sel])
        P.value_forward_backward(critic, ds, sel[ok] + 1)
        _, g64, _ = value_ref.loss_grad(critic.params, 72, hid, L, st.reshape(-1, 32, 72)[sel[ok]], act.reshape(-1)[sel[ok]], ro.rewards.reshape(-1)[sel[ok]])
        assert np.abs(critic.grad() - g64).max() <= BAR * np.abs(g64).max() + 1e-9


# ---------------------------------------------------------------- 9. one step is the gradient
@pytest.mark.parametrize("F,hid,L", [(72, 256, 2), (72, 192, 2), (72, 128, 3)])
def test_one_descent_step_is_the_gradient(P, F, hid, L):
    """value_train_ with Optimiser(Descent(eta)), one epoch, batch = the whole dataset in dataset order: the new parameters are
    Flux's Float32 update old - f32(eta * grad) (Descent: D = f32(f64(g) eta), then x -= D in float32) bit for bit, with grad
    from value_forward_backward on the same minibatch."""
    rng = np.random.default_rng(90 + hid + L)
    critic = _critic(P, F, hid, L, rng)
    ds, *_ = _value_dataset(P, critic, rng, 512, F, hid, L, 32)
    n = len(ds)
    old = critic.params
    loss = P.value_forward_backward(critic, ds, np.arange(1, n + 1))
    g = critic.grad()
    eta = 0.05
    hist, lr = P.value_train_(critic, P.Optimiser(P.Descent(eta)), ds, n, 1, perm=np.arange(1, n + 1)[None], verbose=False)
    want = (old - (g.astype(np.float64) * eta).astype(np.float32)).astype(np.float32)
    assert np.array_equal(critic.params.view(np.uint32), want.view(np.uint32))
    assert hist == [float(np.float32(loss))] and lr == [eta]


# ---------------------------------------------------------------- 10. it learns, and it leaves the policy alone
def _fixed_rollouts(rng, B=1024):
    """Seeded states whose target is a smooth function of what the critic sees (mean score over the active rows)."""
    states = rng.integers(-3, 7, size=(B, 32, 72)).astype(np.int8)
    active = rng.integers(1, 256, size=B).astype(np.uint32)
    on = value_ref.row_mask(active, 32)
    t = (states[:, :, :36].astype(np.float64).mean(axis=2) * on).sum(axis=1) / on.sum(axis=1)
    return states, active, (t - 1.0).astype(np.float32)


def _policy_snapshot(pol, opt):
    st = opt.get_state()
    m = st["members"][0]
    assert m["kind"] == "Adam" and np.abs(m["m"]).max() > 0
    return (pol.params.tobytes(), st["epochs"], m["eta"], m["m"].tobytes(), m["v"].tobytes(), m["beta_pow"].tobytes())


def test_value_training_learns_and_leaves_the_policy_alone(P):
    """8 epochs of value_train_ with Adam(1e-3) on fixed rollouts (seed 2024, 1024 states, minibatch 256): the last epoch's mse
    is below the first's.  The float64 restatement of the same schedule satisfies that by itself (checked on the CPU when the
    seeds were chosen: 0.1139 -> 0.0203; asserted again here).  The policy's parameters and optimiser state do not change."""
    rng = np.random.default_rng(2024)
    states, active, t = _fixed_rollouts(rng)
    B = len(t)
    ro = P.BufferRollouts()
    ro.set_columns(None, states[None], active[None], np.ones((1, B), np.int64), np.full((1, B), 1 / 128, np.float32), t[None], np.zeros((1, B), np.uint8))
    ds = P.construct_dataset(ro)
    pol = P.HipPolicy(72, 128, 2, 4, seed=1)
    popt = P.Optimiser(P.Adam(3e-4))
    P.ppo_train_(pol, popt, ds, 0.05, 256, 1, 0.01, seed=1, verbose=False)         # so that the policy's Adam state is not all zeros
    before = _policy_snapshot(pol, popt)
    critic = P.HipCritic(72, 128, 2, seed=11)
    p0 = critic.params
    perms = np.stack([rng.permutation(B) for _ in range(8)])
    hist, lr = P.value_train_(critic, P.Optimiser(P.Adam(1e-3)), ds, 256, 8, perm=perms + 1, verbose=False)
    h64, _ = value_ref.adam_schedule(p0, 72, 128, 2, states, active, t, 256, perms)
    _record({"case": "learns", "device": hist, "float64": h64})
    assert h64[-1] < h64[0], "the float64 restatement must satisfy the condition by itself"
    assert len(hist) == 8 and np.all(np.isfinite(hist)) and hist[-1] < hist[0]
    assert lr == [1e-3] * 8
    assert _policy_snapshot(pol, popt) == before
    assert not np.array_equal(critic.params, p0)


# ---------------------------------------------------------------- 11. end to end
class _Evaluator:
    def __init__(self):
        self.calls, self.loss = 0, None

    def __call__(self, policy, env, optimizer):
        self.calls += 1


def test_ppo_iterate_with_and_without_a_critic(P):
    P.save_loss.register(_Evaluator)(lambda ev, loss: setattr(ev, "loss", {k: list(v) for k, v in loss.items()}))
    args = dict(episodes=256, mb=256, iters=3, epochs=2, discount=0.99, eps=0.05, ew=0.01)

    def fresh():
        return (P.HipVecEnv(num_envs=256, Q=8, max_actions=8, seed=21), P.HipPolicy(72, 128, 2, 4, seed=3), P.Optimiser(P.Adam(3e-4)))

    # with a critic: finite histories of the right lengths
    env, pol, opt = fresh()
    critic, copt, ev = P.HipCritic(72, 128, 2, seed=4), P.Optimiser(P.Adam(1e-3)), _Evaluator()
    c0 = critic.params
    loss = P.ppo_iterate_(pol, env, opt, args["episodes"], args["mb"], args["iters"], ev, args["epochs"], args["discount"], args["eps"],
                          args["ew"], verbose=False, critic=critic, critic_optimizer=copt, gae_lambda=0.9, value_epochs=3)
    assert sorted(loss) == ["entropy", "lr", "ppo", "value"] and ev.calls == 3 and ev.loss == loss
    assert [len(loss[k]) for k in ("ppo", "entropy", "lr", "value")] == [6, 6, 6, 9]
    assert all(np.all(np.isfinite(v)) for v in loss.values())
    assert not np.array_equal(critic.params, c0)
    # without: exactly the statements ppo_iterate_ has always run, spelled out by hand on an identical second setup
    env, pol, opt = fresh()
    ev = _Evaluator()
    got = P.ppo_iterate_(pol, env, opt, args["episodes"], args["mb"], args["iters"], ev, args["epochs"], args["discount"], args["eps"],
                         args["ew"], verbose=False, critic=None)
    env2, pol2, opt2 = fresh()
    want = {"ppo": [], "entropy": [], "lr": []}
    for _ in range(args["iters"]):
        ro = P.BufferRollouts()
        P.collect_rollouts_(ro, env2, pol2, args["episodes"], args["discount"])
        p, e, lr = P.ppo_train_(pol2, opt2, P.construct_dataset(ro), args["eps"], args["mb"], args["epochs"], args["ew"], verbose=False)
        want["ppo"] += p
        want["entropy"] += e
        want["lr"] += lr
    assert got == want and sorted(got) == ["entropy", "lr", "ppo"]
    assert pol.params.tobytes() == pol2.params.tobytes()


# ---------------------------------------------------------------- 12. refusals
def test_refusals(P):
    rng = np.random.default_rng(12)
    env = P.HipVecEnv(num_envs=8, Q=8, max_actions=5, seed=1)
    pol = P.HipPolicy(72, 128, 2, 4, seed=1)
    ro = P.BufferRollouts()
    P.collect_rollouts_steps_(ro, env, pol, 6, 1.0)
    ds = P.construct_dataset(ro)
    idx = np.arange(1, 9)
    bf = P.HipPolicy(72, 128, 2, 4, seed=1, dtype="bf16")
    st = P.state(env)
    for call in (lambda: P.batch_state_values(bf, st), lambda: P.compute_values_(ro, env, bf), lambda: P.compute_gae_critic_(ro, env, bf, 0.99, 0.95),
                 lambda: P.value_forward_backward(bf, ds, idx), lambda: P.value_train_(bf, P.Optimiser(P.Adam()), ds, 8, 1, verbose=False)):
        with pytest.raises(P.PPOError, match="a bf16-dtype critic is not supported"):
            call()
    wide = P.HipCritic(216, 128, 2)
    for call in (lambda: P.compute_values_(ro, env, wide), lambda: P.compute_gae_critic_(ro, env, wide, 0.99, 0.95),
                 lambda: P.value_forward_backward(wide, ds, idx), lambda: P.value_train_(wide, P.Optimiser(P.Adam()), ds, 8, 1, verbose=False)):
        with pytest.raises(P.PPOError, match=r"the critic's input width F = 216 differs from the buffer's F = 72"):
            call()
    critic = P.HipCritic(72, 128, 2)
    for call in (lambda: P.value_forward_backward(critic, ds, idx, target="lambda_returns"),
                 lambda: P.value_train_(critic, P.Optimiser(P.Adam()), ds, 8, 1, target="lambda_returns", verbose=False)):
        with pytest.raises(P.PPOError, match="needs ppo_rollouts_compute_gae on these rollouts first"):
            call()
    L = P._lib.lib()                                     # an unknown target at the C ABI
    one = np.zeros(1, np.float64)
    i0 = np.zeros(1, np.int64)
    assert L.ppo_value_forward_backward(critic._h, ro._h, i0.ctypes.data_as(P._lib.c_i64p), 1, 1, 7, one.ctypes.data_as(P._lib.c_f64p)) == -4
    assert "unknown target" in P._lib.last_error()
    P.compute_gae_critic_(ro, env, critic, 0.99, 0.95)
    assert np.isfinite(P.value_forward_backward(critic, ds, idx, target="lambda_returns"))
