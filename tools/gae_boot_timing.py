#!/usr/bin/env python3
"""What bootstrapping time-limit truncations costs at the headline shape (4096 envs x 128 steps, HipCritic(72,256,2), the
benchmark's max_actions = 128, so every env is cut once: K = 4096) and at max_actions = 32 and 12 (K about T*N / max_actions).
compute_gae_critic_(fetch=False) with and without bootstrap_truncated, alternating, every call ending in a synchronise:
median and spread of the wall time; then one profiled pass for the device time of the pieces (scan with and without the boot
column, replay, the extra critic forward).  A record, not a gate.  Writes profiles/gae_boot_timing.json, or the file named
second.  Usage: tools/gae_boot_timing.py [repetitions] [out.json]"""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ppo_amd as PPO

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 30
N, T = 4096, 128
KERNELS = ("k_gae_tn", "k_gae_boot_tn", "k_boot_flags", "k_boot_states", "k_value_fwd_predict")


def timed(fn):
    t0 = time.perf_counter()
    fn()
    PPO.synchronize()
    return time.perf_counter() - t0


def spread(x):
    x = np.asarray(x)
    return {"median_ms": 1e3 * float(np.median(x)), "min_ms": 1e3 * float(x.min()), "max_ms": 1e3 * float(x.max()), "n": int(x.size)}


out = {"workload": "%d envs x %d steps, Q = 8, HipCritic(72,256,2), compute_gae_critic_(fetch=False), gamma 0.99, lambda 0.95" % (N, T),
       "cases": {}}
for max_actions in (128, 32, 12):
    for compact in (0, 1):
        PPO.set_rollout_compact(compact)
        env = PPO.HipVecEnv(num_envs=N, Q=8, max_actions=max_actions, seed=7)
        pol = PPO.HipPolicy(72, 256, 2, 4, seed=0)
        critic = PPO.HipCritic(72, 256, 2, seed=1)
        ro = PPO.BufferRollouts()
        PPO.collect_rollouts_steps_(ro, env, pol, T, 0.99)
        plain = lambda: PPO.compute_gae_critic_(ro, env, critic, 0.99, 0.95, fetch=False)
        boot = lambda: PPO.compute_gae_critic_(ro, env, critic, 0.99, 0.95, fetch=False, bootstrap_truncated=True)
        for _ in range(3):
            plain(); boot()
        tp, tb = [], []
        for _ in range(REPS):
            tp.append(timed(plain)); tb.append(timed(boot))
        rec = {"K": int(ro.n_truncated), "done_transitions": int(ro.terminal.sum()), "plain": spread(tp), "bootstrapped": spread(tb)}
        rec["extra_median_ms"] = rec["bootstrapped"]["median_ms"] - rec["plain"]["median_ms"]
        PPO.profile_enable(True)
        for _ in range(10):
            plain(); boot()
        PPO.synchronize()
        rec["device_ms_per_launch"] = {}
        for k in KERNELS:
            ms, n = PPO.profile_get(k)
            if n:
                rec["device_ms_per_launch"][k] = {"mean_ms": ms / n, "launches": int(n)}
        PPO.profile_enable(False)
        out["cases"]["max_actions_%d_%s" % (max_actions, "compact" if compact else "expanded")] = rec
        print(max_actions, "compact" if compact else "expanded", json.dumps(rec))
PPO.set_rollout_compact(None)
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "gae_boot_timing.json")
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(out, open(OUT, "w"), indent=1)
