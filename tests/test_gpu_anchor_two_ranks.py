"""KL-anchored PPO across two data-parallel ranks on ONE GPU (gloo for the exchange, like tests/test_gpu_distill_two_ranks.py):
ppo_train_(..., parallel=) with an adaptive anchor on shards of unequal length, each rank filling its own shard's targets from
its copy of the teacher -- replicas bit-identical, histories, anchor KL and coefficients equal on both ranks, the anchor KL that of
the union of the shards, against the single-rank float64 schedule on the union.

The two rank processes are started ONCE for the module and joined against a deadline: a missed collective ends the children
and fails the tests, it cannot hang them."""
import os
import socket
import time
from datetime import timedelta

import numpy as np
import pytest

import anchor_ref as ref
from test_gpu_imitation import ETA, schedule_bars

pytestmark = pytest.mark.gpu

F, HID, LAYERS = 72, 128, 2
DEADLINE = 120.0                                # seconds for both ranks
BATCH = 40                                      # 14 + 13 envs, 6 steps: 84 / 78 samples -> steps of 40+40, 40+38 and 4+0 samples
EPS = 0.2
COEF0 = 1.0
# far below the divergence between two independently initialised policies: the rule doubles the coefficient behind the epochs,
# and the float64 replay below asserts that it moves
TARGET = 0.002


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


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
    off, n = dp.env_shard(27)
    env = P.HipVecEnv(num_envs=n, Q=8, max_actions=10, seed=5, global_offset=off)
    pol = P.HipPolicy(F, HID, LAYERS, 4, seed=3)
    teacher = P.HipPolicy(F, 256, 2, 4, seed=17)
    ro = P.BufferRollouts()
    P.set_rollout_compact(rank)                 # one shard in each storage form: modes 20 and 21 side by side
    P.collect_rollouts_steps_(ro, env, pol, 6, 1.0)
    P.set_rollout_compact(None)
    P.fill_targets_(ro, teacher)
    ds = P.construct_dataset(ro)
    p0 = pol.params.copy()
    perm = np.stack([np.arange(len(ds)) + 1] * 2)
    pol.kl_anchor = (COEF0, "column", TARGET)
    pol.target_kl = float("inf")
    ph, eh, lh = P.ppo_train_(pol, P.Optimiser(P.Adam(ETA)), ds, EPS, BATCH, 2, 0.0, perm=perm, parallel=dp, verbose=False)
    ast, st = pol.last_anchor_stats(), pol.last_train_stats()
    stt, act = ro.state_data
    np.savez(base + "_rank%d.npz" % rank, ph=ph, eh=eh, lh=lh, params=pol.params, p0=p0, index=ro.index(), n=len(ds),
             akl=ast["anchor_kl"], acoef=ast["anchor_coef"], final=pol.kl_anchor[0], approx_kl=st["approx_kl"],
             st=stt.reshape(-1, 32, F), act=act.reshape(-1), q=ro.action_targets.reshape(-1, 128),
             actions=ro.selected_actions.reshape(-1) - 1, p_old=ro.selected_action_probabilities.reshape(-1), adv=ro.rewards.reshape(-1))
    torch.cuda.synchronize()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def P(ppo):
    if ppo.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests must run on the GPU box")
    return ppo


@pytest.fixture(scope="module")
def ranks(P, tmp_path_factory):
    import torch.multiprocessing as mp
    base = str(tmp_path_factory.mktemp("ddp") / "dp")
    ctx = mp.spawn(_rank_main, args=(2, _free_port(), base), nprocs=2, join=False)
    end = time.monotonic() + DEADLINE
    why = None
    try:
        while not ctx.join(timeout=1.0):
            if time.monotonic() > end:
                why = "the rank processes did not finish within %d s (a missed collective?)" % DEADLINE
                break
    except Exception as e:                      # noqa: BLE001 -- a rank raised: reported by the test
        why = "a rank process failed: %s" % e
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.terminate()
            p.join(10)
    files = [base + "_rank%d.npz" % r for r in (0, 1)]
    if why or not all(os.path.isfile(f) for f in files):
        pytest.fail(why or "the ranks left no results")
    return [np.load(f) for f in files]


def test_two_unequal_shards(P, ranks):
    """Both ranks hold the same parameters, histories, anchor KL and coefficients; the anchor KL is the union's; the rule moved
    the coefficient on both ranks alike."""
    r0, r1 = ranks
    assert (int(r0["n"]), int(r1["n"])) == (84, 78)
    assert np.array_equal(r0["params"], r1["params"]), "replicas must hold bit-identical parameters after training"
    for k in ("ph", "eh", "lh", "akl", "acoef", "approx_kl"):
        assert np.array_equal(r0[k], r1[k]) and r0[k].shape == (2,), k
    assert float(r0["final"]) == float(r1["final"]) and np.array_equal(r0["p0"], r1["p0"])
    for r in (r0, r1):
        assert np.array_equal(r["index"], np.arange(int(r["n"]))), "storage order is dataset order here"
    st, act, q, actions, p_old, adv = (np.concatenate([r0[k], r1[k]]) for k in ("st", "act", "q", "actions", "p_old", "adv"))
    n0, n1 = int(r0["n"]), int(r1["n"])
    perms = [[np.arange(n0), np.arange(n1)]] * 2
    r = ref.adam_schedule(r0["p0"], F, HID, LAYERS, st, act, actions, p_old.astype(np.float32), adv.astype(np.float32), EPS, q, COEF0,
                          BATCH, perms, target=TARGET, eta=ETA, shards=[(0, n0), (n0, n0 + n1)])
    ok, fig = schedule_bars(r0["params"], r["params"], r0["ph"], r["hist"], 6)
    print("unequal shards: loss history", r0["ph"].tolist(), "float64 replay", r["hist"], "anchor kl", r0["akl"].tolist(), r["kl"],
          "coef", r0["acoef"].tolist(), r["coef"], float(r0["final"]), r["final_coef"], fig)
    assert ok, fig
    assert r["coef"][1] != r["coef"][0] or r["final_coef"] != r["coef"][1], "the float64 replay must move the coefficient by itself"
    assert r0["acoef"].tolist() == r["coef"] and float(r0["final"]) == r["final_coef"]
    assert np.max(np.abs(r0["akl"] - np.asarray(r["kl"])) / (1 + np.abs(r["kl"]))) <= 1e-5, (r0["akl"], r["kl"])
