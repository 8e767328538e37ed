"""Time-limit truncations bootstrapped on the device: the GAE scan with a bootstrap column, the replay that
tells a time limit from the optimum and rebuilds the state an episode was cut in, and both end to end through the critic.
References: the float64 restatement and the CPU-oracle replay of tests/gae_boot_ref.py.  The device scan works in IEEE fp64 in
a fixed order with -ffp-contract=off, so it is held bit-exact."""
import numpy as np
import pytest

import gae_boot_ref
import value_ref

pytestmark = pytest.mark.gpu

GAMMA, LAM = 0.99, 0.95


@pytest.fixture(scope="module")
def P(ppo):
    if ppo.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests must run on the GPU box")
    return ppo


@pytest.fixture()
def knobs(P):
    yield P
    P.set_rollout_compact(None)
    P.set_rollout_persistent(None)


def _critic(P, hid, L, rng, seed=5):
    c = P.HipCritic(72, hid, L, seed=seed)
    c.params = (c.params + (rng.normal(size=c.num_params) * 0.03).astype(np.float32)).astype(np.float32)
    return c


# ---------------------------------------------------------------- 1. the scan
# one lane per column: (77, 130), (1, 1); LDS-tiled, 128 columns: (45, 16388) with a ragged last workgroup, (33, 65536);
# 256 columns: (16, 262144)
@pytest.mark.parametrize("T,N", [(77, 130), (1, 1), (45, 16388), (33, 65536), (16, 262144)])
def test_scan_with_boot_column(P, T, N):
    rng = np.random.default_rng(T * 1000003 + N)
    r = rng.normal(size=(T, N)).astype(np.float32)
    v = rng.normal(size=(T + 1, N)).astype(np.float32)
    d = (rng.random((T, N)) < 0.05).astype(np.uint8)
    if T * N == 1:
        d[:] = 1
    boot = np.zeros((T, N), np.float32)
    ends = np.flatnonzero(d.reshape(-1))
    vals = (rng.uniform(0.5, 3.0, size=ends[::2].size) * rng.choice([-1.0, 1.0], size=ends[::2].size)).astype(np.float32)
    boot.reshape(-1)[ends[::2]] = vals
    nz = int(np.count_nonzero(boot))
    if T * N > 1:
        assert nz >= 1 and ends.size - nz >= 1
    assert nz == ends[::2].size and not boot[d == 0].any()
    adv, ret = P.gae_boot_tn(r, d, v, boot, GAMMA, LAM)
    a64, r64 = gae_boot_ref.gae_boot(r, d, v, boot, GAMMA, LAM)
    assert np.array_equal(adv, a64) and np.array_equal(ret, r64)
    adv2, ret2 = P.gae_boot_tn(r, d, v, boot, GAMMA, LAM)
    assert adv.tobytes() == adv2.tobytes() and ret.tobytes() == ret2.tobytes()
    a0, r0 = P.gae_boot_tn(r, d, v, np.zeros((T, N), np.float32), GAMMA, LAM)
    p0, q0 = P.gae_tn(r, d, v, GAMMA, LAM)
    assert np.array_equal(a0, p0) and np.array_equal(r0, q0)
    assert not np.array_equal(adv, p0)


# ---------------------------------------------------------------- 2. detection and final states
def _check_detection(P, orc, ro, Q, least):
    T, N = ro.dims()
    st, act = ro.state_data
    done, valid = ro.terminal, ro.valid
    ends = done & valid
    flags, fst, fact = P.truncated_transitions_(ro)
    rflags, rst, ract = gae_boot_ref.replay_buffer(orc, Q, st, act, ro.selected_actions - 1, ends)
    assert flags.dtype == bool and flags.shape == (T, N)
    assert np.array_equal(flags, rflags)
    assert not flags[~ends].any()
    K = int(flags.sum())
    assert K >= least, (K, least)
    assert fst.shape == (K, 4 * Q, 72) and fact.shape == (K,)
    assert fst.tobytes() == rst.tobytes() and fact.tobytes() == ract.tobytes()
    only_flags = P.truncated_transitions_(ro, fetch_states=False)
    assert np.array_equal(only_flags[0], flags) and only_flags[1] is None and only_flags[2] is None
    return flags, fst, fact


@pytest.mark.parametrize("persistent", [1, 0], ids=["one_launch", "per_step"])
@pytest.mark.parametrize("compact", [0, 1], ids=["expanded", "compact"])
def test_detection_q8(knobs, orc, compact, persistent):
    P = knobs
    P.set_rollout_compact(compact)
    P.set_rollout_persistent(persistent)
    env = P.HipVecEnv(num_envs=48, Q=8, max_actions=7, seed=31)
    pol = P.HipPolicy(72, 128, 2, 4, seed=2)
    ro = P.BufferRollouts()
    P.collect_rollouts_steps_(ro, env, pol, 20, GAMMA)
    _check_detection(P, orc, ro, 8, 48 * (20 // 7))


@pytest.mark.parametrize("compact", [0, 1], ids=["expanded", "compact"])
def test_detection_q32(knobs, orc, compact):
    P = knobs
    P.set_rollout_compact(compact)
    env = P.HipVecEnv(num_envs=20, Q=32, max_actions=6, seed=5)
    pol = P.HipPolicy(72, 128, 2, 4, seed=2)
    ro = P.BufferRollouts()
    P.collect_rollouts_steps_(ro, env, pol, 13, 1.0)
    _check_detection(P, orc, ro, 32, 20 * (13 // 6))


def test_detection_episodes_form(P, orc):
    """Whole episodes: envs that played theirs record done = 1, valid = 0, which is no episode end.  40 episodes can hold
    at most 40 truncations (N * (T // max_actions) = 48 counts idle envs' rows too), so all 40 are asked for."""
    env = P.HipVecEnv(num_envs=16, Q=8, max_actions=6, seed=9)
    pol = P.HipPolicy(72, 128, 2, 4, seed=2)
    ro = P.BufferRollouts()
    P.collect_rollouts_(ro, env, pol, 40, 1.0)
    T, N = ro.dims()
    flags, _, _ = _check_detection(P, orc, ro, 8, min(N * (T // 6), 40))
    assert (ro.terminal & ~ro.valid).any() and not flags[~ro.valid].any()


def _crafted_buffer(P, orc):
    """[3, 8] transitions of the crafted Q = 8 states, action 0 everywhere; row 1 is flagged done: columns 0..3 reach the
    optimum there, columns 4..7 do not.  Rows 0 and 2 hold the same two states and are not done."""
    term, act, _, _ = gae_boot_ref.crafted_states(orc, False)
    cut, _, _, _ = gae_boot_ref.crafted_states(orc, True)
    T, N = 3, 8
    st = np.empty((T, N, 32, 72), np.int8)
    st[:, :4], st[:, 4:] = term, cut
    done = np.zeros((T, N), np.uint8)
    done[1] = 1
    env = P.HipVecEnv(num_envs=N, Q=8, max_actions=7, seed=3)
    ro = P.BufferRollouts()
    ro.set_columns(env, st, np.full((T, N), act, np.uint32), np.ones((T, N), np.int64), np.full((T, N), 1 / 128, np.float32),
                   np.full((T, N), 4.0, np.float32), done)
    return ro, env, cut


def test_crafted_terminals_are_not_truncations(P, orc):
    ro, env, cut = _crafted_buffer(P, orc)
    flags, fst, fact = _check_detection(P, orc, ro, 8, 4)
    want = np.zeros((3, 8), bool)
    want[1, 4:] = True
    assert np.array_equal(flags, want) and len(fst) == 4
    assert not np.array_equal(fst[0], cut)                       # the state behind the step, not the stored one
    critic = _critic(P, 128, 2, np.random.default_rng(1))
    adv, ret = P.compute_gae_critic_(ro, env, critic, GAMMA, LAM, bootstrap_truncated=True)
    boot = ro.boot_values
    assert ro.n_truncated == 4
    assert not boot[~want].any() and np.all(boot[1, :4] == 0.0) and np.all(boot[1, 4:] != 0.0)
    plain_a, plain_r = P.compute_gae_critic_(ro, env, critic, GAMMA, LAM)
    assert adv[:, :4].tobytes() == plain_a[:, :4].tobytes() and ret[:, :4].tobytes() == plain_r[:, :4].tobytes()
    assert np.all(adv[1, 4:] != plain_a[1, 4:])


# ---------------------------------------------------------------- 3. end to end
@pytest.mark.parametrize("hid,L", [(128, 2), (256, 2), (128, 3)])
@pytest.mark.parametrize("compact", [0, 1], ids=["expanded", "compact"])
def test_end_to_end(knobs, compact, hid, L):
    P = knobs
    P.set_rollout_compact(compact)
    rng = np.random.default_rng(600 + hid + L)
    env = P.HipVecEnv(num_envs=48, Q=8, max_actions=7, seed=31)
    pol = P.HipPolicy(72, 128, 2, 4, seed=2)
    critic = _critic(P, hid, L, rng)
    ro = P.BufferRollouts()
    P.collect_rollouts_steps_(ro, env, pol, 20, GAMMA)
    T, N = ro.dims()
    adv, ret = P.compute_gae_critic_(ro, env, critic, GAMMA, LAM, bootstrap_truncated=True)
    boot = ro.boot_values
    # the lambda-returns value training regresses on are the bootstrapped ones
    ds = P.construct_dataset(ro)
    loss = P.value_forward_backward(critic, ds, np.arange(1, T * N + 1), target="lambda_returns")
    st, act = ro.state_data
    v64 = value_ref.values_np(critic.params, 72, hid, L, st.reshape(-1, 32, 72), act.reshape(-1))
    l64 = float(np.mean((v64 - ret.reshape(-1).astype(np.float64)) ** 2))
    assert abs(loss - l64) <= 1e-5 * max(1.0, abs(l64)), (loss, l64)     # tests/test_gpu_value.py's bar for this loss
    # boot = the critic's value of the final states, 0 elsewhere
    flags, fst, fact = P.truncated_transitions_(ro)
    K = int(flags.sum())
    assert ro.n_truncated == K and K >= N * (T // 7)
    vfin = P.batch_state_values(critic, P.StateData(fst, fact))
    assert np.array_equal(boot[flags].view(np.uint32), vfin.view(np.uint32))
    assert not boot[~flags].any()
    assert np.count_nonzero(vfin) >= K - 2
    # the same numbers from host-supplied values, and from the float64 restatement
    v = P.compute_values_(ro, env, critic)
    adv2, ret2 = P.compute_gae_(ro, v, GAMMA, LAM, final_values=boot)
    assert adv.tobytes() == adv2.tobytes() and ret.tobytes() == ret2.tobytes()
    assert ro.boot_values.tobytes() == boot.tobytes()
    done = ro.terminal
    a64, r64 = gae_boot_ref.gae_boot(ro.raw_rewards, done, v, boot, GAMMA, LAM)
    assert adv.tobytes() == a64.tobytes() and ret.tobytes() == r64.tobytes()
    # against the plain call: different wherever a truncation bootstraps, the same on the open tails
    pa, pr = P.compute_gae_critic_(ro, env, critic, GAMMA, LAM)
    hit = flags & (boot != 0.0)
    assert hit.sum() >= K - 2 and np.all(adv[hit] != pa[hit]) and np.all(ret[hit] != pr[hit])
    for n in range(N):
        last = np.flatnonzero(done[:, n])
        t0 = last[-1] + 1 if last.size else 0
        assert adv[t0:, n].tobytes() == pa[t0:, n].tobytes() and ret[t0:, n].tobytes() == pr[t0:, n].tobytes()
    assert P.compute_gae_critic_(ro, env, critic, GAMMA, LAM, fetch=False, bootstrap_truncated=True) is None
    again = P.compute_gae_critic_(ro, env, critic, GAMMA, LAM, bootstrap_truncated=True)
    assert again[0].tobytes() == adv.tobytes() and again[1].tobytes() == ret.tobytes()
    assert ro.boot_values.tobytes() == boot.tobytes()


# ---------------------------------------------------------------- 4. refusals and the off switch
class _Evaluator:
    def __init__(self):
        self.loss = None

    def __call__(self, policy, env, optimizer):
        pass


def test_refusals(P):
    rng = np.random.default_rng(4)
    critic = _critic(P, 128, 2, rng)
    T, N = 3, 10
    st = rng.integers(-3, 7, size=(T, N, 32, 72)).astype(np.int8)
    shaped = P.BufferRollouts()                                  # ppo_rollouts_create_shape: no env template
    shaped.set_columns(None, st, rng.integers(1, 256, size=(T, N)).astype(np.uint32), np.ones((T, N), np.int64),
                       np.ones((T, N), np.float32), rng.normal(size=(T, N)).astype(np.float32), np.zeros((T, N), np.uint8))
    for call in (lambda: P.compute_gae_critic_(shaped, None, critic, GAMMA, LAM, bootstrap_truncated=True),
                 lambda: P.truncated_transitions_(shaped)):
        with pytest.raises(P.PPOError, match="ppo_rollouts_compute_gae_boot") as e:
            call()
        assert e.value.status == -4
    # ... which that buffer takes
    v = rng.normal(size=(T + 1, N)).astype(np.float32)
    fv = np.zeros((T, N), np.float32)
    adv, ret = P.compute_gae_(shaped, v, GAMMA, LAM, final_values=fv)
    pa, pr = P.compute_gae_(shaped, v, GAMMA, LAM)
    assert np.array_equal(adv, pa) and np.array_equal(ret, pr)
    for bad in (np.zeros((T + 1, N), np.float32), np.zeros((T, N + 1), np.float32), np.zeros(T * N, np.float32)):
        with pytest.raises(P.PPOError, match="final_values must be"):
            P.compute_gae_(shaped, v, GAMMA, LAM, final_values=bad)
    env = P.HipVecEnv(num_envs=8, Q=8, max_actions=5, seed=1)
    pol = P.HipPolicy(72, 128, 2, 4, seed=1)
    ro = P.BufferRollouts()
    P.collect_rollouts_steps_(ro, env, pol, 6, 1.0)
    with pytest.raises(P.PPOError, match="needs ppo_rollouts_compute_gae_boot or ppo_rollouts_compute_gae_critic_boot"):
        ro.boot_values
    bf = P.HipPolicy(72, 128, 2, 4, seed=1, dtype="bf16")
    with pytest.raises(P.PPOError, match="a bf16-dtype critic is not supported"):
        P.compute_gae_critic_(ro, env, bf, GAMMA, LAM, bootstrap_truncated=True)


def test_ppo_iterate_off_switch_and_on(P):
    P.save_loss.register(_Evaluator)(lambda ev, loss: setattr(ev, "loss", {k: list(v) for k, v in loss.items()}))

    def run(**kw):
        env = P.HipVecEnv(num_envs=64, Q=8, max_actions=8, seed=21)
        pol, opt = P.HipPolicy(72, 128, 2, 4, seed=3), P.Optimiser(P.Adam(3e-4))
        critic, copt = P.HipCritic(72, 128, 2, seed=4), P.Optimiser(P.Adam(1e-3))
        loss = P.ppo_iterate_(pol, env, opt, 64, 64, 2, _Evaluator(), 1, GAMMA, 0.05, 0.01, verbose=False, critic=critic,
                              critic_optimizer=copt, gae_lambda=0.9, value_epochs=2, **kw)
        return loss, pol.params.tobytes(), critic.params.tobytes()

    today = run()
    off = run(bootstrap_truncated=False)
    assert off == today and "truncated" not in today[0]
    on, pp, cp = run(bootstrap_truncated=True)
    assert len(on["truncated"]) == 2 and all(k > 0 for k in on["truncated"])
    assert len(on["value"]) == len(today[0]["value"]) == 4 and np.all(np.isfinite(on["value"]))
    assert sorted(on) == sorted(list(today[0]) + ["truncated"])
    assert cp != today[2]                                        # the critic saw other targets
