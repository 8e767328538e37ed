#!/usr/bin/env python3
"""What the critic's all-reduce costs per PPO iteration with a critic on TWO ranks SHARING ONE GPU, the exchange over gloo
(a host round trip of the gradient buffer per optimiser step): 4096 envs x 128 steps split over the ranks, Policy(72,HID,2,4)
and a critic of the same shape, 4 epochs, 2048 samples per rank and step.  Every iteration is collect + compute_gae_critic_ +
ppo_train_(advantage = "gae", parallel) + value_train_(target = "lambda_returns"); the two kinds ALTERNATE in one pair of
processes, each ending in a device synchronise:
    local      value_train_ without `parallel`: every rank trains its own critic on its own shard (all a tree without
               ppo_value_train_dp can do: the only kind timed when --tree names one)
    allreduce  value_train_(..., parallel=dp): one more all-reduce per value step, replicas identical
A record of the host-side cost on a shared GPU, not a speed claim: gloo through host memory says nothing about RCCL over xGMI.
Usage: tools/value_dp_timing.py [--pairs 6] [--hid 256] [--tree DIR] [--out FILE.json]"""
import argparse
import inspect
import json
import os
import socket
import statistics
import sys
import time

N, T, EPOCHS, MB = 4096, 128, 4, 2048


def rank_main(rank, world, port, tree, pairs, hid, out):
    sys.path.insert(0, tree)
    import torch
    import torch.distributed as dist
    import ppo_amd as PPO
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    torch.cuda.set_device(0)
    dp = PPO.DataParallel(rank, world)
    off, n = dp.env_shard(N)
    env = PPO.HipVecEnv(num_envs=n, Q=8, max_actions=32, seed=7, global_offset=off)
    pol, opt = PPO.HipPolicy(72, hid, 2, 4, seed=0), PPO.Optimiser(PPO.Adam(3e-4))
    critic, copt = PPO.HipCritic(72, hid, 2, seed=1), PPO.Optimiser(PPO.Adam(1e-3))
    kinds = ["local"] + (["allreduce"] if "parallel" in inspect.signature(PPO.value_train_).parameters else [])

    def iteration(kind, it):
        PPO.synchronize()
        dist.barrier()
        t0 = time.perf_counter()
        ro = PPO.BufferRollouts()
        PPO.collect_rollouts_steps_(ro, env, pol, T, 1.0)
        ds = PPO.construct_dataset(ro)
        PPO.compute_gae_critic_(ro, env, critic, 0.99, 0.95, fetch=False)
        PPO.ppo_train_(pol, opt, ds, 0.05, MB, EPOCHS, 0.01, seed=it, parallel=dp, verbose=False, advantage="gae")
        extra = {"parallel": dp} if kind == "allreduce" else {}
        PPO.value_train_(critic, copt, ds, MB, EPOCHS, target="lambda_returns", seed=it, verbose=False, **extra)
        PPO.synchronize()
        return time.perf_counter() - t0

    for _ in range(2):                                      # warm-up: every kernel and collective of both kinds has run
        for k in kinds:
            iteration(k, 0)
    times = {k: [] for k in kinds}
    for i in range(pairs):
        for k in kinds:
            times[k].append(iteration(k, i + 1))
    dist.barrier()
    if rank == 0:
        med = {k: statistics.median(v) for k, v in times.items()}
        res = {"workload": "%d envs x %d steps over %d ranks sharing one GPU (gloo), Policy(72,%d,2,4) and a critic of the same shape, "
                           "%d epochs, %d samples per rank and step" % (N, T, world, hid, EPOCHS, MB),
               "tree": os.path.basename(os.path.abspath(tree)), "pairs": pairs, "seconds": times, "median_s": med,
               "spread": {k: (max(v) - min(v)) / med[k] for k, v in times.items()}}
        if "allreduce" in med:
            res["allreduce_over_local"] = med["allreduce"] / med["local"]
        if out:
            os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
            json.dump(res, open(out, "w"), indent=1)
        print(json.dumps({k: v for k, v in res.items() if k != "seconds"}))
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--hid", type=int, default=256)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(rank_main, args=(2, port, os.path.abspath(a.tree), a.pairs, a.hid, a.out), nprocs=2, join=True)


if __name__ == "__main__":
    main()
