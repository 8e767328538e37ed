"""The critic across two data-parallel ranks on ONE GPU (gloo for the exchange, like tests/test_gpu_two_ranks.py):
value_train_(..., parallel=), the value-clip statistics, explained_variance_(..., parallel=) and ppo_iterate_(..., critic=,
parallel=) -- replicas bit-identical, the all-reduced gradient and the loss history those of the union of the shards,
the statistics exact sums over both ranks.

The two rank processes are started ONCE for the module and run every scenario in turn, each leaving its results in its own
.npz files; a test reads the files of its scenario.  The ranks are joined against a deadline: a missed collective ends the
children and fails the tests, it cannot hang them."""
import ctypes as C
import os
import socket
import time
from datetime import timedelta

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F, HID, LAYERS = 72, 128, 2
N_PER_RANK, T, B = 24, 8, 80                    # 192 local samples: minibatches of 80, 80, 32
DEADLINE = 120.0                                # seconds for both ranks to run all scenarios
# chosen on the CPU from the deltas of the clip scenario (test_clip_statistics_are_global).  The issue's first try, 0.05, left
# all 216 states of the last epoch outside (|delta| between 1.0 and 1.7 after six Adam(1e-3) steps on returns of this size);
# a scan over 0.5, 1, 1.5, 2, 3, 5 gave 216, 216, 204, 132, 10 and 0 outside.  2.0: 132 of 216 outside, and no |delta| within
# 0.008 of it
CLIP = 2.0
TARGETS = ("returns", "lambda_returns")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _deltas(P, critic, n):
    L = P._lib.lib()
    L.ppo_debug_value_deltas.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.ppo_debug_value_deltas.restype = C.c_int32
    d = np.zeros(n, np.float32)
    assert L.ppo_debug_value_deltas(critic._h, n, d.ctypes.data) == 0, P._lib.last_error()
    return d


class _Eval:
    def __call__(self, policy, env, optimizer):
        pass


def _shard(P, dp, total, steps=None, episodes=None, max_actions=10):
    off, n = dp.env_shard(total)
    env = P.HipVecEnv(num_envs=n, Q=8, max_actions=max_actions, seed=5, global_offset=off)
    pol = P.HipPolicy(F, HID, LAYERS, 4, seed=3)
    ro = P.BufferRollouts()
    if steps:
        P.collect_rollouts_steps_(ro, env, pol, steps, 1.0)
    else:
        P.collect_rollouts_(ro, env, pol, episodes, 0.99)
    return env, pol, ro


def _columns(ro):
    st, act = ro.state_data
    return dict(st=st.reshape(-1, 32, F), act=act.reshape(-1), ret=ro.rewards.reshape(-1))


def _equal_shards(P, dp, base, target):
    """Scenario 2: one full-shard step with Descent(0.1), then two epochs of ragged minibatches in a shared order (with Adam:
    six more steps of Descent(0.1) on returns of this size diverge)."""
    env, pol, ro = _shard(P, dp, 2 * N_PER_RANK, steps=T)
    ds = P.construct_dataset(ro)
    critic = P.HipCritic(F, HID, LAYERS, seed=4)
    copt = P.Optimiser(P.Descent(0.1))
    cols = _columns(ro)
    cols["t"] = cols["ret"]
    if target == "lambda_returns":
        _, lam = P.compute_gae_critic_(ro, env, critic, 0.99, 0.95)
        cols["t"] = lam.reshape(-1)
    mh1, _ = P.value_train_(critic, copt, ds, len(ds), 1, target=target, parallel=dp, verbose=False)
    grad1 = critic.grad()
    params1 = critic.params.copy()
    perm = np.stack([np.random.default_rng(100 + e).permutation(len(ds)) + 1 for e in range(2)])
    mh, _ = P.value_train_(critic, P.Optimiser(P.Adam(1e-3)), ds, B, 2, target=target, perm=perm, parallel=dp, verbose=False)
    np.savez(base + "_eq_%s_rank%d.npz" % (target, dp.rank), grad1=grad1, params1=params1, mh1=mh1, mh=mh, params=critic.params,
             n=len(ds), **cols)


def _unequal_shards(P, dp, base):
    """Scenario 3: 14 + 13 envs, 84 / 78 samples, batch 40 in storage order -> steps of 40+40, 40+38 and 4+0 samples."""
    env, pol, ro = _shard(P, dp, 27, steps=6)
    ds = P.construct_dataset(ro)
    critic = P.HipCritic(F, HID, LAYERS, seed=4)
    copt = P.Optimiser(P.Adam(1e-3))
    perm = np.stack([np.arange(len(ds)) + 1])
    mh, _ = P.value_train_(critic, copt, ds, 40, 1, perm=perm, parallel=dp, verbose=False)
    try:                                        # above the SHORTEST shard: refused on every rank alike, nobody left waiting
        P.value_train_(critic, copt, ds, 80, 1, parallel=dp, verbose=False)
        bad = ""
    except P.PPOError as e:
        bad = str(e)
    np.savez(base + "_uneq_rank%d.npz" % dp.rank, mh=mh, params=critic.params, bad=bad, index=ro.index(), n=len(ds), **_columns(ro))


def _clip_statistics(P, dp, base, clip=CLIP):
    """Scenario 4: unequal shards again, so that a mean of the ranks' fractions is not the global fraction."""
    env, pol, ro = _shard(P, dp, 27, steps=T)
    ds = P.construct_dataset(ro)
    critic = P.HipCritic(F, HID, LAYERS, seed=4)
    critic.value_clip = clip
    P.compute_values_(ro, env, critic)
    P.value_train_(critic, P.Optimiser(P.Adam(1e-3)), ds, 40, 2, seed=11, parallel=dp, verbose=False)
    st = critic.last_value_stats()
    np.savez(base + "_clip_rank%d.npz" % dp.rank, epochs_run=st["epochs_run"], clip_fraction=st["clip_fraction"],
             mean_sq_change=st["mean_sq_change"], deltas=_deltas(P, critic, len(ds)), params=critic.params)


def _explained_variance(P, dp, base):
    """Scenario 5: whole episodes, so that idle envs leave invalid transitions in both shards."""
    env, pol, ro = _shard(P, dp, 2 * N_PER_RANK, episodes=40)
    critic = P.HipCritic(F, HID, LAYERS, seed=4)
    _, lam = P.compute_gae_critic_(ro, env, critic, 0.99, 0.95)
    T_, _ = ro.dims()
    ev = P.explained_variance_(ro, "lambda_returns", parallel=dp)
    local = P.explained_variance_(ro, "lambda_returns")
    vals = P.compute_values_(ro, env, critic)[:T_]
    np.savez(base + "_ev_rank%d.npz" % dp.rank, ev=ev, local=local, t=lam, v=vals, valid=ro.valid)


def _iterate(P, dp, base):
    """Scenario 6: the critic-driven PPO iteration, every training call and the explained variance across the ranks."""
    P.save_loss.register(_Eval)(lambda ev, loss: None)
    off, n = dp.env_shard(2 * N_PER_RANK)
    env = P.HipVecEnv(num_envs=n, Q=8, max_actions=10, seed=5, global_offset=off)
    pol = P.HipPolicy(F, HID, LAYERS, 4, seed=3)
    critic = P.HipCritic(F, HID, LAYERS, seed=4)
    pol.target_kl = float("inf")
    loss = P.ppo_iterate_(pol, env, P.Optimiser(P.Adam(1e-3)), 2 * N_PER_RANK, B, 2, _Eval(), 2, 0.99, 0.05, 0.01, verbose=False,
                          critic=critic, critic_optimizer=P.Optimiser(P.Adam(1e-3)), parallel=dp)
    np.savez(base + "_it_rank%d.npz" % dp.rank, policy=pol.params, critic=critic.params,
             **{"loss_" + k: np.asarray(v, np.float64) for k, v in loss.items()})


def _rank_main(rank, world, port, base):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch
    import torch.distributed as dist
    import ppo_amd as P
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world,
                            timeout=timedelta(seconds=DEADLINE))
    torch.cuda.set_device(0)
    dp = P.DataParallel(rank, world)
    for target in TARGETS:
        _equal_shards(P, dp, base, target)
    _unequal_shards(P, dp, base)
    _clip_statistics(P, dp, base)
    _explained_variance(P, dp, base)
    _iterate(P, dp, base)
    torch.cuda.synchronize()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def P(ppo):
    if ppo.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests must run on the GPU box")
    return ppo


@pytest.fixture(scope="module")
def ranks(P, tmp_path_factory):
    """Runs the two ranks once.  -> load(name): the two ranks' files of a scenario; fails with what went wrong in the rank
    processes when the scenario did not get that far."""
    import torch.multiprocessing as mp
    base = str(tmp_path_factory.mktemp("vdp") / "dp")
    ctx = mp.spawn(_rank_main, args=(2, _free_port(), base), nprocs=2, join=False)
    end = time.monotonic() + DEADLINE
    why = None
    try:
        while not ctx.join(timeout=1.0):
            if time.monotonic() > end:
                why = "the rank processes did not finish within %d s (a missed collective?)" % DEADLINE
                break
    except Exception as e:                      # noqa: BLE001 -- a rank raised: reported by the tests whose files are missing
        why = "a rank process failed: %s" % e
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.terminate()
            p.join(10)

    def load(name):
        files = [base + "_%s_rank%d.npz" % (name, r) for r in (0, 1)]
        if not all(os.path.isfile(f) for f in files):
            pytest.fail(why or "scenario %s left no results" % name)
        return [np.load(f) for f in files]
    load.why = why
    return load


def test_rank_processes_finished(ranks):
    assert ranks.why is None, ranks.why


# ---------------------------------------------------------------- 1. one rank through the hook
def test_identity_hook_single_rank(P):
    """world = 1 with a hook that leaves the buffer alone: the separate all-reduce and optimiser launches must leave exactly
    the parameters and the mse history of the run without `parallel`."""
    calls = []

    def identity(ctx, buf, n):
        calls.append(n)
        return 0

    class Hooked:
        rank, world, force_hook = 0, 1, True

        def make_hook(self, policy):
            return P._lib.ALLREDUCE_FN(identity)

    got = []
    for par in (None, Hooked()):
        env = P.HipVecEnv(num_envs=64, Q=8, max_actions=10, seed=3)
        pol = P.HipPolicy(F, HID, LAYERS, 4, seed=5)
        ro = P.BufferRollouts()
        P.collect_rollouts_steps_(ro, env, pol, 8, 1.0)
        critic = P.HipCritic(F, HID, LAYERS, seed=4)
        mh, lh = P.value_train_(critic, P.Optimiser(P.Adam(1e-3)), P.construct_dataset(ro), 128, 2, seed=1, parallel=par,
                                verbose=False)
        got.append((critic.params.copy(), mh, lh))
    assert np.array_equal(got[0][0], got[1][0]) and got[0][1] == got[1][1] and got[0][2] == got[1][2]
    assert np.all(np.isfinite(got[0][0])) and np.all(np.isfinite(got[0][1]))
    n = int(got[0][0].size) + 2
    assert calls == [n] * 8, "four minibatches per epoch, the gradient and the two loss slots each time; no other exchange"


# ---------------------------------------------------------------- 2. two equal shards
@pytest.fixture(scope="module")
def union(P):
    """The unsharded run's rollouts (RNG keyed by global env id: the shards are its columns), collected once."""
    env = P.HipVecEnv(num_envs=2 * N_PER_RANK, Q=8, max_actions=10, seed=5)
    pol = P.HipPolicy(F, HID, LAYERS, 4, seed=3)
    ro = P.BufferRollouts()
    P.collect_rollouts_steps_(ro, env, pol, T, 1.0)
    return env, ro


@pytest.mark.parametrize("target", TARGETS)
def test_two_equal_shards(P, ranks, union, target):
    import value_ref
    r0, r1 = ranks("eq_" + target)
    assert np.array_equal(r0["grad1"], r1["grad1"]), "the all-reduced gradient is the same buffer on both ranks"
    assert np.array_equal(r0["params1"], r1["params1"]) and np.array_equal(r0["mh1"], r1["mh1"])
    assert np.array_equal(r0["params"], r1["params"]), "replicas must hold bit-identical parameters after training"
    assert np.array_equal(r0["mh"], r1["mh"]) and r0["mh"].shape == (2,), "the mse history is the global one"
    assert np.all(np.isfinite(r0["params"])) and np.all(np.isfinite(r0["mh"]))
    assert int(r0["n"]) == int(r1["n"]) == N_PER_RANK * T
    # the same gradient from one process over the 48-env union (another slab partition: fp32 rounding only)
    env, ro = union
    critic = P.HipCritic(F, HID, LAYERS, seed=4)
    p0 = critic.params.copy()
    if target == "lambda_returns":
        P.compute_gae_critic_(ro, env, critic, 0.99, 0.95, fetch=False)
    ds = P.construct_dataset(ro)
    st, _ = ro.state_data
    assert np.array_equal(st[:, :N_PER_RANK].reshape(-1, 32, F), r0["st"]) and np.array_equal(st[:, N_PER_RANK:].reshape(-1, 32, F), r1["st"])
    loss_union = P.value_forward_backward(critic, ds, np.arange(1, len(ds) + 1), target=target)
    g_union = critic.grad()
    err_union = np.abs(r0["grad1"] - g_union).max() / np.abs(g_union).max()
    # and from the float64 restatement over the transitions and targets the two ranks held
    cat = lambda k: np.concatenate([r0[k], r1[k]])
    loss64, g64, _ = value_ref.loss_grad(p0, F, HID, LAYERS, cat("st"), cat("act"), cat("t"))
    err64 = np.abs(r0["grad1"] - g64).max() / np.abs(g64).max()
    print("two equal shards, %s: grad vs union %.3g (bar 2e-6), vs float64 %.3g (bar 2e-5); loss %.9g union %.9g float64 %.9g"
          % (target, err_union, err64, r0["mh1"][0], loss_union, loss64))
    assert err_union <= 2e-6
    assert err64 <= 2e-5
    assert abs(r0["mh1"][0] - loss64) <= 1e-5 * (1 + abs(loss64)), "the loss of the step is the mean over the union"
    assert not np.array_equal(r0["params"], r0["params1"]) and np.all(np.isfinite(r0["params"]))


# ---------------------------------------------------------------- 3. unequal shards
def test_two_unequal_shards(P, ranks):
    """Same number of collectives on both ranks although one runs out of samples; every step's gradient is the mean over
    the samples both contributed: the mse history against a float64 replay of the three union batches with Flux.Adam."""
    import value_ref
    r0, r1 = ranks("uneq")
    assert (int(r0["n"]), int(r1["n"])) == (84, 78)
    assert np.array_equal(r0["params"], r1["params"]) and np.array_equal(r0["mh"], r1["mh"])
    for r in (r0, r1):
        assert "batch_size" in str(r["bad"]), str(r["bad"])
        assert np.array_equal(r["index"], np.arange(int(r["n"]))), "storage order is dataset order here"
    p = np.asarray(P.HipCritic(F, HID, LAYERS, seed=4).params, np.float64)
    m, v, bp = np.zeros_like(p), np.zeros_like(p), [0.9, 0.999]
    losses = []
    for b in range(3):
        sel = [slice(40 * b, min(40 * (b + 1), int(r["n"]))) for r in (r0, r1)]
        cat = lambda k: np.concatenate([r[k][s] for r, s in zip((r0, r1), sel)])
        assert len(cat("act")) == (80, 78, 4)[b]
        loss, g, _ = value_ref.loss_grad(p, F, HID, LAYERS, cat("st"), cat("act"), cat("ret"))
        losses.append(loss)
        m = 0.9 * m + 0.1 * g
        v = 0.999 * v + 0.001 * g * g
        p = p - m / (1 - bp[0]) / (np.sqrt(v / (1 - bp[1])) + 1e-8) * 1e-3
        bp = [bp[0] * 0.9, bp[1] * 0.999]
    want = float(np.mean(losses))
    print("unequal shards: mse history %.9g, float64 replay %.9g; parameters after the three steps differ by at most %.3g"
          % (r0["mh"][0], want, np.abs(p - r0["params"]).max()))
    assert abs(want - r0["mh"][0]) <= 1e-5 * (1 + abs(want))


# ---------------------------------------------------------------- 4. clip statistics
def test_clip_statistics_are_global(ranks):
    r0, r1 = ranks("clip")
    for k in ("epochs_run", "clip_fraction", "mean_sq_change", "params"):
        assert np.array_equal(r0[k], r1[k]), k
    assert int(r0["epochs_run"]) == 2
    d = [r["deltas"] for r in (r0, r1)]
    assert (d[0].size, d[1].size) == (14 * T, 13 * T)
    n = d[0].size + d[1].size
    outside = sum(int(np.count_nonzero(np.abs(x) > np.float32(CLIP))) for x in d)
    print("clip statistics: %d of %d outside c = %g; |delta| quantiles 5/50/95 %%: %s"
          % (outside, n, CLIP, np.quantile(np.abs(np.concatenate(d)), [0.05, 0.5, 0.95])))
    assert 0.05 * n <= outside <= 0.95 * n, "both sides of the clip must be populated"
    assert r0["clip_fraction"][-1] == outside / n
    msq = float(sum(np.sum(x.astype(np.float64) ** 2) for x in d)) / n
    assert abs(r0["mean_sq_change"][-1] - msq) <= 1e-12 * msq


# ---------------------------------------------------------------- 5. explained variance
def test_explained_variance_is_global(ranks):
    r0, r1 = ranks("ev")
    assert float(r0["ev"]) == float(r1["ev"])
    on = [r["valid"].astype(bool) for r in (r0, r1)]
    assert all(0 < o.sum() < o.size for o in on)
    t = np.concatenate([r["t"].astype(np.float64)[o] for r, o in zip((r0, r1), on)])
    v = np.concatenate([r["v"].astype(np.float64)[o] for r, o in zip((r0, r1), on)])
    want = 1.0 - np.var(t - v) / np.var(t)
    print("explained variance: global %.15g, numpy %.15g, local %.15g / %.15g" % (r0["ev"], want, r0["local"], r1["local"]))
    assert abs(float(r0["ev"]) - want) <= 1e-10
    assert float(r0["local"]) != float(r0["ev"]) or float(r1["local"]) != float(r0["ev"])
    for r, o in zip((r0, r1), on):              # the local value is the rank's own
        tl, vl = r["t"].astype(np.float64)[o], r["v"].astype(np.float64)[o]
        assert abs(float(r["local"]) - (1.0 - np.var(tl - vl) / np.var(tl))) <= 1e-9


# ---------------------------------------------------------------- 6. ppo_iterate_
def test_ppo_iterate_with_critic_across_ranks(ranks):
    r0, r1 = ranks("it")
    assert sorted(r0.files) == sorted(r1.files)
    assert sorted(k[5:] for k in r0.files if k.startswith("loss_")) == ["approx_kl", "clip_fraction", "entropy", "explained_variance",
                                                                        "lr", "ppo", "value"]
    for k in r0.files:
        assert np.array_equal(r0[k], r1[k]), k
        assert np.all(np.isfinite(r0[k])), k
    assert r0["loss_value"].shape == (4,) and r0["loss_ppo"].shape == (4,) and r0["loss_explained_variance"].shape == (2,)
