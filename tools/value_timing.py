#!/usr/bin/env python3
"""What a device critic costs per PPO iteration at the headline shape (4096 envs x 128 steps, Policy(72,256,2,4), 4 epochs,
minibatch 4096): iterations with and without a critic of the policy's shape, ALTERNATING in one process on one GPU, each
ending in a device synchronise.  Without: collect + ppo_train_ (advantage = returns).  With: collect + compute_gae_critic_ +
ppo_train_(advantage = "gae") + value_train_(target = "lambda_returns", same epochs).  Writes profiles/value_timing.json, or
the file named third.  A fourth argument sets critic.value_clip (PPO's clipped value loss and its per-epoch statistics).
Usage: tools/value_timing.py [pairs] [hid] [out.json] [value_clip]"""
import json, os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ppo_amd as PPO

PAIRS = int(sys.argv[1]) if len(sys.argv) > 1 else 8
HID = int(sys.argv[2]) if len(sys.argv) > 2 else 256
N, T, EPOCHS, MB = 4096, 128, 4, 4096
env = PPO.HipVecEnv(num_envs=N, Q=8, max_actions=32, seed=7)
pol = PPO.HipPolicy(72, HID, 2, 4, seed=0)
opt = PPO.Optimiser(PPO.Adam(3e-4))
critic = PPO.HipCritic(72, HID, 2, seed=1)
copt = PPO.Optimiser(PPO.Adam(1e-3))
CLIP = float(sys.argv[4]) if len(sys.argv) > 4 else None
if CLIP is not None:
    critic.value_clip = CLIP


def iteration(with_critic, it):
    PPO.synchronize()
    t0 = time.perf_counter()
    ro = PPO.BufferRollouts()
    PPO.collect_rollouts_steps_(ro, env, pol, T, 1.0)
    ds = PPO.construct_dataset(ro)
    if with_critic:
        PPO.compute_gae_critic_(ro, env, critic, 0.99, 0.95, fetch=False)
        PPO.ppo_train_(pol, opt, ds, 0.05, MB, EPOCHS, 0.01, seed=it, verbose=False, advantage="gae")
        PPO.value_train_(critic, copt, ds, MB, EPOCHS, target="lambda_returns", seed=it, verbose=False)
    else:
        PPO.ppo_train_(pol, opt, ds, 0.05, MB, EPOCHS, 0.01, seed=it, verbose=False)
    PPO.synchronize()
    return time.perf_counter() - t0


for w in (False, True, False, True):                    # warm-up: every kernel of both iterations has run
    iteration(w, 0)
times = {False: [], True: []}
for i in range(PAIRS):
    for w in (False, True):
        times[w].append(iteration(w, i + 1))
med = {w: statistics.median(v) for w, v in times.items()}
out = {"workload": "%d envs x %d steps, Policy(72,%d,2,4) and a critic of the same shape, %d epochs, minibatch %d" % (N, T, HID, EPOCHS, MB),
       "pairs": PAIRS, "value_clip": CLIP, "without_critic_s": times[False], "with_critic_s": times[True],
       "median_without_s": med[False], "median_with_s": med[True], "ratio": med[True] / med[False],
       "env_steps_per_s_without": N * T / med[False], "env_steps_per_s_with": N * T / med[True],
       "spread_without": (max(times[False]) - min(times[False])) / med[False]}
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "value_timing%s.json" % ("" if HID == 256 else "_%d" % HID))
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(out, open(OUT, "w"), indent=1)
print(json.dumps({k: v for k, v in out.items() if not k.endswith("_s") or k.startswith("median")}))
