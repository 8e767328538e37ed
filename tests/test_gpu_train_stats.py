"""Per-epoch KL / clip-fraction statistics, target-KL early stopping and the critic's explained variance on the device.

1. the ratio the loss tail stores is the one its surrogate formed (bit identities against the loss terms), in every
   train-forward family, each asserted by its kernel name (ppo_debug_train_route);
2. it is right: against float64 probabilities at the logit-space bar tests/test_gpu_parity.py::test_policy_forward holds the
   forward to (bf16: the bar tests/test_gpu_bf16.py holds device probabilities to);
3. the fp64 reduction against numpy within a derived bound, order independence, bitwise repeatability;
4. early stopping: identities between four runs from the same start;
5. two ranks take the same decision from the same global statistics, and add no collective when the target is off;
   (the ratios are stored and reduced while a target_kl is set only: every case sets one, float("inf") to record)
6. the five value moments against numpy; 7. ppo_iterate_'s loss dict.

TEST_RECORD_DIR=<dir>: append the measured worst case per route to <dir>/train_stats.jsonl."""
import ctypes as C
import json
import os
import socket
import time

import numpy as np
import pytest

import train_stats_ref as ref
from oracle import np_oracle
from test_train_route import route

pytestmark = pytest.mark.gpu

F, ENT = 72, 0.01
EPS = 0.2


@pytest.fixture(scope="module")
def P(ppo):
    if ppo.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests must run on the GPU box")
    return ppo


@pytest.fixture()
def knobs(P):
    yield P
    P.set_bwd_split_bf16(None)
    P.set_rollout_compact(None)
    P.set_train_tile_max_tiles(None)


def _record(rec):
    d = os.environ.get("TEST_RECORD_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "train_stats.jsonl"), "a") as f:
            f.write(json.dumps(rec) + "\n")


def _debug(P):
    L = P._lib.lib()
    L.ppo_debug_train_ratios.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.ppo_debug_train_ratios.restype = C.c_int32
    L.ppo_debug_train_outputs.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.ppo_debug_train_outputs.restype = C.c_int32
    return L


def _ratios(P, pol, n):
    out = np.zeros(n, np.float32)
    assert _debug(P).ppo_debug_train_ratios(pol._h, n, out.ctypes.data) == 0, P._lib.last_error()
    return out


def _loss_terms(P, pol, B):
    lt = np.zeros((B, 2), np.float64)
    assert _debug(P).ppo_debug_train_outputs(pol._h, B, None, lt.ctypes.data) == 0, P._lib.last_error()
    return lt


def _columns(ro, Q):
    st, act = ro.state_data
    return dict(states=st.reshape(-1, 4 * Q, F), active=act.reshape(-1), a0=(ro.selected_actions.reshape(-1) - 1).astype(np.int32),
                p_old=ro.selected_action_probabilities.reshape(-1), adv=ro.rewards.reshape(-1), Q=Q)


def _perturbed_rollout(P, hid, L, Q, N, T, dtype="f32", seed=1, scale=0.01):
    """An engine rollout, then the policy moved away from the one that collected it: ratios on both sides of the clip range."""
    rng = np.random.default_rng(1000 * hid + 10 * L + Q + seed)
    pol = P.HipPolicy(F, hid, L, 4, seed=seed, dtype=dtype)
    env = P.HipVecEnv(num_envs=N, Q=Q, max_actions=12, seed=7 + seed)
    ro = P.BufferRollouts()
    P.collect_rollouts_steps_(ro, env, pol, T, 0.99)
    pol.params = (pol.params + (rng.normal(size=pol.num_params) * scale).astype(np.float32)).astype(np.float32)
    pol.target_kl = float("inf")                         # the ratios are stored while a target is set: record, never stop
    return pol, ro, rng


# family -> (knob setup, dtype, Q, HID, L, compact, B, smaller B on the same route, forward kernel)
FAMILIES = {
    "x6-h256": ({}, "f32", 8, 256, 2, False, 1024, 600, "k_policy_fwd_train_x6<256>"),
    "x6-h128": ({}, "f32", 8, 128, 2, False, 700, 300, "k_policy_fwd_train_x6<128>"),
    "x6t": ({}, "f32", 8, 256, 2, False, 4096, 2048, "k_policy_fwd_train_x6t<256,2>"),
    "x6s": ({}, "f32", 32, 256, 2, False, 256, 100, "k_policy_fwd_train_x6s<256,4>"),
    "split": ({"split": 0}, "f32", 8, 256, 2, False, 500, 300, "k_policy_fwd_train_split<72,256,2,0>"),
    "mode2": ({"split": 0}, "f32", 8, 256, 2, False, 700, 600, "k_policy_fwd<72,256,2,1,0>"),
    "mode2-L3": ({}, "f32", 8, 256, 3, False, 700, 300, "k_policy_fwd<72,256,2,1,1>"),
    "mode4": ({"split": 0, "compact": True}, "f32", 8, 256, 2, True, 700, 600, "k_policy_fwd<72,256,4,1,0>"),
    "bf16": ({}, "bf16", 8, 256, 2, False, 700, 300, "k_policy_fwd_bf16<72,256,2,1>"),
    "tile": ({"tile": 512}, "f32", 8, 256, 2, False, 500, 300, "k_policy_train_tile<72,256>"),
}


def _setup(P, fam):
    setup, dtype, Q, hid, L, compact, B, B2, kernel = FAMILIES[fam]
    if "split" in setup:
        P.set_bwd_split_bf16(setup["split"])
    if "compact" in setup:
        P.set_rollout_compact(True)
    if "tile" in setup:
        P.set_train_tile_max_tiles(setup["tile"])
    N, T = (512, 8) if Q == 8 else (64, 4)
    pol, ro, rng = _perturbed_rollout(P, hid, L, Q, N, T, dtype)
    ds = P.construct_dataset(ro)
    assert len(ds) >= B
    for n in (B, B2):
        assert route(P, dtype, F, hid, L, 4 * Q, compact, n)[0] == kernel, (fam, n, route(P, dtype, F, hid, L, 4 * Q, compact, n))
    sel0 = rng.permutation(len(ds))[:B]
    c = _columns(ro, Q)
    c = {k: (v[sel0] if k != "Q" else v) for k, v in c.items()}
    return pol, ds, sel0, c, (dtype, Q, hid, L, B, B2)


@pytest.mark.parametrize("fam", list(FAMILIES))
def test_stored_ratio_is_the_tails_own(P, knobs, fam):
    pol, ds, sel0, c, (dtype, Q, hid, L, B, B2) = _setup(P, fam)
    adv = c["adv"].astype(np.float32)
    clip = np.where(adv >= 0, (1.0 + EPS) * adv.astype(np.float64), (1.0 - EPS) * adv.astype(np.float64))
    # the case holds both kinds, judged on the float64 restatement of the probabilities
    r64 = ref.ratios(pol.params, F, hid, L, c["states"], c["active"], Q, c["a0"], c["p_old"])
    un64 = r64 * adv.astype(np.float64) < clip
    assert un64.sum() >= B // 20 and (~un64).sum() >= B // 20, (int(un64.sum()), B)
    P.forward_backward(pol, ds, sel0 + 1, EPS, ENT)
    lt = _loss_terms(P, pol, B)
    r = _ratios(P, pol, B)
    assert np.all(np.isfinite(r)) and np.all(r > 0)
    g = (r * adv).astype(np.float64)                   # fl(fl(ps / po) * adv): numpy's float32 product is the device's
    un = g < clip
    assert un.any() and (~un).any()
    assert np.array_equal(g[un].view(np.uint64), lt[un, 0].view(np.uint64)), "unclipped: the loss term is ratio * advantage"
    assert np.all(g[~un] >= clip[~un])
    assert np.array_equal(clip[~un].view(np.uint64), lt[~un, 0].view(np.uint64)), "clipped: the loss term is the clip value"
    # nothing writes outside the minibatch: a smaller one leaves the entries behind it alone
    P.forward_backward(pol, ds, sel0[:B2] + 1, EPS, ENT)
    r2 = _ratios(P, pol, B)
    assert np.array_equal(r2[B2:].view(np.uint32), r[B2:].view(np.uint32))
    assert np.array_equal(r2[:B2].view(np.uint32), r[:B2].view(np.uint32)), "a state's ratio does not depend on the minibatch"


@pytest.mark.parametrize("fam", list(FAMILIES))
def test_stored_ratio_against_float64(P, knobs, fam):
    pol, ds, sel0, c, (dtype, Q, hid, L, B, B2) = _setup(P, fam)
    P.forward_backward(pol, ds, sel0 + 1, EPS, ENT)
    r = _ratios(P, pol, B).astype(np.float64)
    rec = dict(case="ratio", family=fam, B=B)
    if dtype == "bf16":
        want = np_oracle.action_probabilities_bf16(pol.params, F, hid, c["states"], np_oracle.batch_masks(c["active"], Q))
        want = want[np.arange(B), c["a0"]]
        po = c["p_old"].astype(np.float64)
        tol = (5e-3 * want + 1e-6) / po + 2.0 ** -23 * (want / po)
        err = np.abs(r - want / po)
        rec.update(worst=float((err / tol).max()), unit="fraction of the bf16 probability bar")
        _record(rec)
        assert np.all(err <= tol), rec
    else:
        r64 = ref.ratios(pol.params, F, hid, L, c["states"], c["active"], Q, c["a0"], c["p_old"])
        tol = 1e-4 * np.maximum(1.0, ref.logits_max(pol.params, F, hid, L, c["states"], c["active"], Q)) + 2.0 ** -23
        err = np.abs(np.log(r) - np.log(r64))
        rec.update(worst=float(err.max()), worst_over_tol=float((err / tol).max()), unit="|log r_dev - log r_64|")
        _record(rec)
        assert np.all(err <= tol), rec


@pytest.mark.parametrize("n", [4096, 5000])
def test_epoch_reduction_against_numpy(P, n):
    N, T = (512, 8) if n == 4096 else (1000, 5)
    pol, ro, rng = _perturbed_rollout(P, 256, 2, 8, N, T, seed=2)
    p0 = pol.params.copy()
    ds = P.construct_dataset(ro)
    assert len(ds) == n
    perm = np.stack([rng.permutation(n) + 1 for _ in range(3)])
    runs = []
    for _ in range(2):
        opt = P.Optimiser(P.Descent(0.0))                 # the parameters never move: three epochs see the same ratios
        P.ppo_train_(pol, opt, ds, EPS, 1024, 3, ENT, perm=perm, verbose=False)
        runs.append(pol.last_train_stats())
    assert np.array_equal(pol.params, p0)
    st = runs[0]
    assert runs[1] == st, "a second identical run repeats the first bit for bit"
    assert st["epochs_run"] == 3 and not st["stopped_early"]
    r = _ratios(P, pol, n)                                # the latest epoch's column
    assert np.all(np.isfinite(r)) and np.all(r > 0) and np.unique(r).size > n // 2
    s1, s3, c, _ = ref.ratio_sums(r, EPS)
    b1, b3 = ref.sum_bound(r)
    want = P.kl_stats(r, EPS)
    assert 0 < want["clip_fraction"] < 1
    for e in range(3):
        assert st["clip_fraction"][e] * n == c, "the clip count is exact"
        assert abs(st["old_approx_kl"][e] * n - s1) <= b1, (e, st["old_approx_kl"][e] * n - s1, b1)
        assert abs(st["approx_kl"][e] * n - s3) <= b3, (e, st["approx_kl"][e] * n - s3, b3)
    assert abs(st["approx_kl"][2] - want["approx_kl"]) <= b3 / n and abs(st["old_approx_kl"][2] - want["old_approx_kl"]) <= b1 / n
    _record(dict(case="reduction", n=n, err_kl=abs(st["approx_kl"][2] * n - s3), bound_kl=b3,
                 err_old_kl=abs(st["old_approx_kl"][2] * n - s1), bound_old_kl=b1))


def _early_start(P):
    c = ref.EARLY
    pol = P.HipPolicy(c["F"], c["HID"], c["L"], 4, seed=c["policy_seed"])
    env = P.HipVecEnv(num_envs=c["N"], Q=c["Q"], max_actions=c["max_actions"], seed=c["env_seed"])
    ro = P.BufferRollouts()
    P.collect_rollouts_steps_(ro, env, pol, c["T"], c["discount"])
    return pol.params.copy(), ro


def _early_run(P, p0, ds, perm, target, epochs):
    c = ref.EARLY
    pol = P.HipPolicy(c["F"], c["HID"], c["L"], 4, seed=0)
    pol.params = p0
    pol.target_kl = target
    assert pol.target_kl == target
    opt = P.Optimiser(P.Adam(c["eta"]))
    hist = P.ppo_train_(pol, opt, ds, c["eps"], c["batch"], epochs, c["ent"], perm=perm[:epochs], verbose=False)
    os_ = opt.get_state()
    return dict(hist=hist, stats=pol.last_train_stats(), params=pol.params.copy(), m=os_["members"][0]["m"],
                v=os_["members"][0]["v"], bp=os_["members"][0]["beta_pow"], epochs=os_["epochs"])


def test_early_stopping_is_consistent(P):
    c = ref.EARLY
    p0, ro = _early_start(P)
    ds = P.construct_dataset(ro)
    n = len(ds)
    assert n == c["N"] * c["T"]
    perm0 = ref.early_perms(n)
    # the property the choice of j needs, on the rollout this device collected, restated in float64
    k64, _, _ = ref.restated_run(p0, c["F"], c["HID"], c["L"], _columns(ro, c["Q"]), perm0, c["batch"], c["eps"], c["ent"], c["eta"])
    assert ref.first_rise(k64) is not None, k64
    perm = perm0 + 1
    A = _early_run(P, p0, ds, perm, float("inf"), 6)
    k = A["stats"]["approx_kl"]
    assert A["stats"]["epochs_run"] == 6 and not A["stats"]["stopped_early"] and len(k) == 6 and np.all(np.isfinite(k))
    j = ref.first_rise(k)
    assert j is not None, k
    target = (k[j] + max(k[:j])) / 2
    _record(dict(case="early", k_dev=k, k_f64=k64, j=j, target=target))
    B = _early_run(P, p0, ds, perm, target, 6)
    sb = B["stats"]
    assert sb["epochs_run"] == j + 1 and sb["stopped_early"]
    assert all(len(h) == j + 1 for h in B["hist"])
    for key in ("approx_kl", "old_approx_kl", "clip_fraction"):
        assert sb[key] == A["stats"][key][:j + 1], key
    assert [h[:j + 1] for h in A["hist"]] == list(B["hist"])
    Cr = _early_run(P, p0, ds, perm, None, j + 1)
    assert Cr["stats"]["epochs_run"] == j + 1 and not Cr["stats"]["stopped_early"]
    assert len(Cr["stats"]["approx_kl"]) == j + 1 and np.all(np.isnan(Cr["stats"]["approx_kl"])), "target off: not collected"
    for key in ("params", "m", "v", "bp"):
        assert np.array_equal(Cr[key], B[key]), key
    assert Cr["epochs"] == B["epochs"] == j + 1
    D = _early_run(P, p0, ds, perm, None, 6)
    assert np.array_equal(D["params"], A["params"]) and D["epochs"] == A["epochs"] == 6, "recording changes nothing"
    assert D["stats"]["epochs_run"] == 6 and all(len(h) == 6 for h in D["hist"]) and list(D["hist"]) == list(A["hist"])
    assert all(np.all(np.isnan(D["stats"][key])) for key in ("approx_kl", "old_approx_kl", "clip_fraction"))
    # a target no epoch exceeds never stops; the setter refuses what the header says it refuses
    pol = P.HipPolicy(c["F"], c["HID"], c["L"], 4, seed=0)
    for bad in (-1.0, float("nan")):
        with pytest.raises(P.PPOError):
            pol.target_kl = bad
    for ok in (0.01, float("inf"), None):
        pol.target_kl = ok
        assert pol.target_kl == ok
    pol.target_kl = 0.0
    assert pol.target_kl is None
    # ... and with the target off the train forward stores nothing
    P.forward_backward(pol, ds, np.arange(1, 65), c["eps"], c["ent"])
    assert _debug(P).ppo_debug_train_ratios(pol._h, 64, np.zeros(64, np.float32).ctypes.data) == -1
    assert "no ratios stored" in P._lib.last_error()
    pol.target_kl = float("inf")
    P.forward_backward(pol, ds, np.arange(1, 65), c["eps"], c["ent"])
    assert np.all(_ratios(P, pol, 64) > 0)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


RANK_EPOCHS, RANK_BATCH, RANK_EPS = 5, 40, 0.5


def _stats_rank_main(rank, world, port, base):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import torch
    import torch.distributed as dist
    import ppo_amd as P
    import train_stats_ref as ref
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    torch.cuda.set_device(0)
    dp = P.DataParallel(rank, world)
    calls = [0]
    inner = P.DataParallel.allreduce_

    def counted(t):
        calls[0] += 1
        return inner(t)
    dp.allreduce_ = counted
    off, n = dp.env_shard(27)                            # 14 + 13 envs: unequal shards
    env = P.HipVecEnv(num_envs=n, Q=8, max_actions=10, seed=5, global_offset=off)
    pol = P.HipPolicy(72, 128, 2, 4, seed=3)
    p0 = pol.params.copy()
    ro = P.BufferRollouts()
    P.collect_rollouts_steps_(ro, env, pol, 6, 0.99)     # 84 / 78 local samples: 3 steps per epoch, the last one ragged
    ds = P.construct_dataset(ro)
    perm = np.stack([np.random.default_rng(50 + e).permutation(len(ds)) + 1 for e in range(RANK_EPOCHS)])
    out = {}

    def run(tag, target, epochs):
        pol.params = p0
        pol.target_kl = target
        opt = P.Optimiser(P.Adam(1e-3))
        calls[0] = 0
        P.ppo_train_(pol, opt, ds, RANK_EPS, RANK_BATCH, epochs, 0.01, perm=perm[:epochs], parallel=dp, verbose=False)
        torch.cuda.synchronize()
        st = pol.last_train_stats()
        out[tag + "_calls"] = calls[0]
        out[tag + "_epochs"] = st["epochs_run"]
        out[tag + "_stopped"] = int(st["stopped_early"])
        out[tag + "_kl"] = np.array(st["approx_kl"])
        out[tag + "_old"] = np.array(st["old_approx_kl"])
        out[tag + "_clip"] = np.array(st["clip_fraction"])
        out[tag + "_params"] = pol.params.copy()
        return st
    first = run("inf", float("inf"), RANK_EPOCHS)
    L = P._lib.lib()
    L.ppo_debug_train_ratios.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.ppo_debug_train_ratios.restype = C.c_int32
    col = np.zeros(len(ds), np.float32)
    assert L.ppo_debug_train_ratios(pol._h, len(ds), col.ctypes.data) == 0
    out["inf_last_column"] = col                          # this rank's ratios of the last epoch
    k = first["approx_kl"]
    j = ref.first_rise(k, last=RANK_EPOCHS - 2)
    out["j"] = -1 if j is None else j
    if j is not None:                                     # global statistics: both ranks derive the same target
        run("stop", (k[j] + max(k[:j])) / 2, RANK_EPOCHS)
    run("off", None, RANK_EPOCHS)
    np.savez(base + "_s%d.npz" % rank, **out)
    dist.destroy_process_group()


def test_two_ranks_agree_on_the_stop(P, tmp_path):
    import torch.multiprocessing as mp
    base = str(tmp_path / "st")
    ctx = mp.spawn(_stats_rank_main, args=(2, _free_port(), base), nprocs=2, join=False)
    deadline = time.time() + 300
    while not ctx.join(timeout=5):                         # neither rank hangs in a collective the other never issues
        if time.time() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the two ranks did not finish within 300 s")
    r0, r1 = np.load(base + "_s0.npz"), np.load(base + "_s1.npz")
    nb = 3                                                 # max over ranks of ceil(84 / 40), ceil(78 / 40)
    j = int(r0["j"])
    assert j >= 1 and int(r1["j"]) == j, (r0["inf_kl"], r1["inf_kl"])
    for tag in ("inf", "stop"):
        assert int(r0[tag + "_epochs"]) == int(r1[tag + "_epochs"])
        for key in ("_kl", "_old", "_clip", "_params"):
            assert np.array_equal(r0[tag + key], r1[tag + key]), tag + key
    assert int(r0["inf_epochs"]) == RANK_EPOCHS and int(r0["inf_stopped"]) == 0
    assert int(r0["stop_epochs"]) == j + 1 and int(r0["stop_stopped"]) == 1 and int(r1["stop_stopped"]) == 1
    assert np.array_equal(r0["stop_kl"], r0["inf_kl"][:j + 1])
    # collectives: the shard-length exchange and the status agreement, one per optimiser step, and with a target one per epoch
    for r in (r0, r1):
        assert int(r["off_calls"]) == 2 + RANK_EPOCHS * nb, "target off: the hook is called as often as before"
        assert int(r["inf_calls"]) == 2 + RANK_EPOCHS * nb + RANK_EPOCHS
        assert int(r["stop_calls"]) == 2 + (j + 1) * nb + (j + 1)
    # target off: the same training, nothing collected
    assert np.array_equal(r0["off_params"], r1["off_params"]) and np.array_equal(r0["off_params"], r0["inf_params"])
    assert int(r0["off_epochs"]) == RANK_EPOCHS and np.all(np.isnan(r0["off_kl"])) and np.all(np.isnan(r1["off_kl"]))
    # the global statistics are those of the union of the two ranks' columns, not of either rank's own
    assert not np.array_equal(r0["inf_last_column"][:78], r1["inf_last_column"][:78])
    both = np.concatenate([r0["inf_last_column"], r1["inf_last_column"]])
    s1, s3, c, n = ref.ratio_sums(both, RANK_EPS)
    assert abs(r0["inf_kl"][-1] * n - s3) <= ref.sum_bound(both)[1]
    assert r0["inf_clip"][-1] * n == c


def test_value_moments_against_numpy(P):
    env = P.HipVecEnv(num_envs=48, Q=8, max_actions=9, seed=13)
    pol = P.HipPolicy(F, 128, 2, 4, seed=2)
    critic = P.HipCritic(F, 128, 2, seed=4)
    ro = P.BufferRollouts()
    P.collect_rollouts_(ro, env, pol, 100, 0.99)           # whole episodes: idle envs leave invalid transitions
    valid = ro.valid
    assert 0 < valid.sum() < valid.size
    with pytest.raises(P.PPOError, match="needs ppo_rollouts_compute_values or ppo_rollouts_compute_gae on these rollouts first"):
        P.explained_variance_(ro, "returns")
    _, lam = P.compute_gae_critic_(ro, env, critic, 0.99, 0.95)
    T, N = ro.dims()
    vals = P.compute_values_(ro, env, critic)[:T]
    i0 = int(ro.index()[0])                                # the first transition of the dataset
    L = P._lib.lib()
    for name, col in (("returns", ro.rewards), ("lambda_returns", lam)):
        sums = np.zeros(5, np.float64)
        assert L.ppo_rollouts_value_moments(ro._h, P.VALUE_TARGETS[name], sums.ctypes.data_as(P._lib.c_f64p)) == 0
        want, mags = ref.value_moments(col, vals, valid, i0)
        n = want[0]
        assert sums[0] == n == valid.sum()
        for q in range(1, 5):
            assert abs(sums[q] - want[q]) <= n * 2.0 ** -52 * mags[q], (name, q, sums[q], want[q])
        ev = P.explained_variance_(ro, name)
        t, d = col.astype(np.float64)[valid.astype(bool)], (col.astype(np.float64) - vals)[valid.astype(bool)]
        assert abs(ev - (1.0 - np.var(d) / np.var(t))) <= 1e-9
        again = np.zeros(5, np.float64)
        assert L.ppo_rollouts_value_moments(ro._h, P.VALUE_TARGETS[name], again.ctypes.data_as(P._lib.c_f64p)) == 0
        assert np.array_equal(again, sums)
    # a new collection invalidates the values
    P.collect_rollouts_(ro, env, pol, 100, 0.99)
    with pytest.raises(P.PPOError, match="on these rollouts first"):
        P.explained_variance_(ro, "returns")


class _Eval:
    def __call__(self, policy, env, optimizer):
        pass


def test_ppo_iterate_reports_the_statistics(P):
    P.save_loss.register(_Eval)(lambda ev, loss: None)
    env = P.HipVecEnv(num_envs=32, Q=8, max_actions=8, seed=3)
    pol = P.HipPolicy(F, 128, 2, 4, seed=1)
    critic = P.HipCritic(F, 128, 2, seed=2)
    pol.target_kl = float("inf")
    loss = P.ppo_iterate_(pol, env, P.Optimiser(P.Adam(1e-3)), 64, 64, 2, _Eval(), 3, 0.99, 0.2, 0.01, verbose=False,
                          critic=critic, critic_optimizer=P.Optimiser(P.Adam(1e-3)))
    assert sorted(loss) == ["approx_kl", "clip_fraction", "entropy", "explained_variance", "lr", "ppo", "value"]
    assert len(loss["approx_kl"]) == len(loss["clip_fraction"]) == len(loss["ppo"]) == len(loss["entropy"]) == len(loss["lr"]) == 6
    assert len(loss["explained_variance"]) == 2 and len(loss["value"]) == 6
    assert all(np.all(np.isfinite(v)) for v in loss.values())
    assert all(k >= 0 for k in loss["approx_kl"]) and all(0 <= c <= 1 for c in loss["clip_fraction"])
    # a target that the first epoch exceeds: one epoch per iteration, every history cut alike
    pol.target_kl = 1e-12
    loss = P.ppo_iterate_(pol, env, P.Optimiser(P.Adam(1e-3)), 64, 64, 2, _Eval(), 3, 0.99, 0.2, 0.01, verbose=False)
    assert sorted(loss) == ["approx_kl", "clip_fraction", "entropy", "lr", "ppo"]
    assert all(len(v) == 2 for v in loss.values())
