"""The time-limit bootstrap as far as a machine without a GPU can see it: the entry points are declared, bound, exported and
in the Julia shim; their null checks; ppo_iterate_'s second **options name; the float64 restatement (tests/gae_boot_ref.py)
against the C oracle's plain scan and against a closed form; and the two facts the device replay stands on, checked on the
CPU oracle env: an observation gives back the env state it was made from, and the crafted terminal recipe is one."""
import os
import re

import numpy as np
import pytest

import gae_boot_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOUR = ("ppo_gae_boot_tn", "ppo_rollouts_truncated", "ppo_rollouts_compute_gae_boot", "ppo_rollouts_compute_gae_critic_boot")


def test_entry_points_declared_bound_exported(ppo):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppo_hip.h")).read(), flags=re.S)
    jl = open(os.path.join(ROOT, "julia", "ProximalPolicyOptimizationHIP.jl")).read()
    L = ppo._lib.lib()
    for name in FOUR + ("ppo_rollouts_get_boot",):
        m = re.search(r"int32_t\s+%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
        assert m, "%s is not declared in include/ppo_hip.h" % name
        assert len(ppo._lib.SIGNATURES[name]) == m.group(1).count(",") + 1, name
        assert hasattr(L, name), "%s is not exported by libppo_hip.so" % name
    for name in FOUR:
        assert "(:%s, LIB)" % name in jl, "%s has no ccall in the Julia shim" % name
    for name in ("gae_boot_tn", "truncated_transitions_", "compute_gae_", "compute_gae_critic_"):
        assert name in ppo.__all__ and callable(getattr(ppo, name))
    mk = open(os.path.join(ROOT, "proximalpolicyoptimization.jl_amd", "csrc", "Makefile")).read()
    assert "ppo_gae_boot.hip" in mk


def test_null_handles_are_argument_errors(ppo):
    L, p = ppo._lib.lib(), ppo._lib
    k = np.zeros(1, np.int64)
    one = np.zeros(2, np.float32)
    f = one.ctypes.data_as(p.c_f32p)
    assert L.ppo_gae_boot_tn(None, None, None, None, 1, 1, 0.99, 0.95, f, f) == -1
    assert "null" in p.last_error()
    assert L.ppo_gae_boot_tn(f, None, f, f, -1, 1, 0.99, 0.95, f, f) == -1
    assert L.ppo_gae_boot_tn(None, None, None, None, 0, 5, 0.99, 0.95, None, None) == 0      # nothing to do
    assert L.ppo_rollouts_truncated(None, None, None, None, 0, k.ctypes.data_as(p.c_i64p)) == -1
    assert "null" in p.last_error()
    assert L.ppo_rollouts_compute_gae_boot(None, f, f, 0.99, 0.95, None, None) == -1
    assert L.ppo_rollouts_compute_gae_critic_boot(None, None, None, 0.99, 0.95, None, None, None) == -1
    assert "null" in p.last_error()
    assert L.ppo_rollouts_get_boot(None, f) == -1


class _Evaluator:
    pass


def test_ppo_iterate_takes_bootstrap_truncated_and_nothing_else(ppo):
    args = (None, None, None, 8, 8, 0, _Evaluator(), 1, 0.99, 0.05, 0.01)
    today = ppo.ppo_iterate_(*args, verbose=False)
    assert today == {"ppo": [], "entropy": [], "lr": []}
    assert ppo.ppo_iterate_(*args, verbose=False, bootstrap_truncated=False) == today
    assert ppo.ppo_iterate_(*args, verbose=False, bootstrap_truncated=True) == today          # no critic, no GAE
    assert ppo.ppo_iterate_(*args, verbose=False, parallel=None, bootstrap_truncated=True) == today
    for bad in ({"paralel": None}, {"bootstrap": True}, {"bootstrap_truncated": True, "bootstrap_truncate": True}):
        with pytest.raises(TypeError, match="unexpected keyword argument"):
            ppo.ppo_iterate_(*args, verbose=False, **bad)
    # a critic's loss dict gains "truncated" only with the option
    critic = object()
    with_c = ppo.ppo_iterate_(*args, verbose=False, critic=critic, critic_optimizer=object())
    assert "truncated" not in with_c
    assert ppo.ppo_iterate_(*args, verbose=False, critic=critic, critic_optimizer=object(), bootstrap_truncated=False) == with_c
    got = ppo.ppo_iterate_(*args, verbose=False, critic=critic, critic_optimizer=object(), bootstrap_truncated=True)
    assert got == dict(with_c, truncated=[])
    with pytest.raises(ppo.PPOError, match="disk-backed rollouts"):
        ppo.ppo_iterate_(*args, "/nonexistent", False, critic=critic, critic_optimizer=object(), bootstrap_truncated=True)


def test_restatement_with_zero_boot_is_the_plain_scan(orc):
    rng = np.random.default_rng(77130)
    T, N = 77, 130
    r = rng.normal(size=(T, N)).astype(np.float32)
    d = (rng.random((T, N)) < 0.05).astype(np.uint8)
    v = rng.normal(size=(T + 1, N)).astype(np.float32)
    adv, ret = gae_boot_ref.gae_boot(r, d, v, np.zeros((T, N), np.float32), 0.99, 0.95)
    a0, r0 = orc.gae_tn(r, d, v, 0.99, 0.95)
    assert d.sum() > 100
    assert adv.tobytes() == a0.tobytes() and ret.tobytes() == r0.tobytes()


def test_closed_form_on_one_column():
    """Constant reward r, V = v* = r / (1 - gamma) everywhere, done at the last row: bootstrapped from v* every TD error
    vanishes; the plain scan charges the cut episode -gamma v* at its end."""
    T, gamma, lam, r = 40, 0.99, 0.95, 0.5
    vs = r / (1.0 - gamma)
    rew = np.full((T, 1), r, np.float32)
    done = np.zeros((T, 1), np.uint8)
    done[-1] = 1
    V = np.full((T + 1, 1), vs, np.float32)
    boot = np.zeros((T, 1), np.float32)
    boot[-1] = vs
    adv, ret = gae_boot_ref.gae_boot(rew, done, V, boot, gamma, lam)
    assert np.abs(adv).max() <= 1e-6 * abs(vs)
    assert np.abs(ret - np.float32(vs)).max() <= 1e-6 * abs(vs)
    plain, _ = gae_boot_ref.gae_plain(rew, done, V, gamma, lam)
    assert abs(float(plain[-1, 0]) - (-gamma * vs)) <= 1e-6 * abs(vs)
    assert abs(float(plain[0, 0])) > 1e-3 * abs(vs) or T > 200       # and the error reaches back through the trace


@pytest.mark.parametrize("Q", [8, 32])
def test_observation_gives_back_the_env_state(orc, Q):
    """60 steps of 64 envs under uniformly random actions on active quads (max_actions = 12, auto reset): feature 0 / 36 of
    observation row v is score[v] / degree[v] wherever quad v >> 2 is active, and no inactive vertex is non-zero."""
    rng = np.random.default_rng(Q)
    N = 64
    env = orc.Env(Q=Q, max_actions=12, N=N, seed=3)
    env.reset()
    V = 4 * Q
    ends = 0
    for _ in range(60):
        obs = env.observe_all()
        sc, dg, act = env.score.copy(), env.degree.copy(), env.active.copy()
        for n in range(N):
            on = ((int(act[n]) >> (np.arange(V) >> 2)) & 1).astype(bool)
            assert not sc[n][~on].any() and not dg[n][~on].any()
            s2, d2 = gae_boot_ref.state_from_observation(obs[n], act[n])
            assert np.array_equal(s2, sc[n]) and np.array_equal(d2, dg[n])
            quads = np.flatnonzero([(int(act[n]) >> q) & 1 for q in range(Q)])
            env.step_one(n, int(rng.choice(quads)) * 16 + int(rng.integers(16)))
            if env.done[n]:
                ends += 1
                env.reset_one(n)
    assert ends >= N * (60 // 12)


def test_crafted_terminal_recipe(orc):
    rp = gae_boot_ref.Replay(orc, 8)
    for extra, want_trunc in ((False, False), (True, True)):
        obs, act, sc, dg = gae_boot_ref.crafted_states(orc, extra)
        s2, d2 = gae_boot_ref.state_from_observation(obs, act)
        assert np.array_equal(s2, sc) and np.array_equal(d2, dg)
        tr, _, act2, rew = rp.step(sc, dg, act, 0)
        assert tr == want_trunc and rew == 4.0 and act2 == 0x3F
