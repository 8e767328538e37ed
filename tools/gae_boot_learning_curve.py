#!/usr/bin/env python3
"""tools/value_learning_curve.py's critic schedule and seeds (4096 envs x 128 steps, max_actions 32, Policy(72,256,2,4), 4
epochs, minibatch 4096, Adam 3e-4; HipCritic(72,256,2), GAE lambda 0.95, Adam 1e-3, gamma 1.0) once with the plain GAE and
once with time-limit truncations bootstrapped: the evaluator's average return every four iterations and, per iteration, the
critic's explained variance before its update -- against the returns column like DESIGN.md 7a (never bootstrapped), and
against the lambda-returns the critic is actually trained on (explained_variance_).  A record, not a gate.  Writes
profiles/gae_boot_learning_curve.json, or the file named second.  Usage: tools/gae_boot_learning_curve.py [iterations] [out.json]"""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ppo_amd as PPO

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 24
LAM = 0.95
out = {"workload": "4096 envs x 128 steps, max_actions 32, Policy(72,256,2,4), 4 epochs, minibatch 4096, gamma 1.0, eps 0.05, "
                   "entropy_weight 0.01, Adam 3e-4; critic: HipCritic(72,256,2), GAE lambda %.2f, Adam 1e-3, 4 epochs on the lambda-returns" % LAM,
       "runs": {}}
for mode in ("plain", "bootstrapped"):
    env = PPO.HipVecEnv(num_envs=4096, Q=8, max_actions=32, seed=7)
    ev = PPO.HipVecEnv(num_envs=1024, Q=8, max_actions=32, seed=99)
    pol = PPO.HipPolicy(72, 256, 2, 4, seed=0)
    opt = PPO.Optimiser(PPO.Adam(3e-4))
    critic, copt = PPO.HipCritic(72, 256, 2, seed=1), PPO.Optimiser(PPO.Adam(1e-3))
    curve = []
    t0 = time.perf_counter()
    for it in range(ITERS):
        if it % 4 == 0:
            m, s = PPO.average_returns(pol, ev, 1024)
            curve.append({"iteration": it, "average_return": m, "std": s})
        ro = PPO.BufferRollouts()
        PPO.collect_rollouts_steps_(ro, env, pol, 128, 1.0)
        rec = {"iteration": it, "mean_reward_per_step": float(ro.raw_rewards.mean())}
        ds = PPO.construct_dataset(ro)
        PPO.compute_gae_critic_(ro, env, critic, 1.0, LAM, fetch=False, bootstrap_truncated=(mode == "bootstrapped"))
        if mode == "bootstrapped":
            rec["truncated"] = int(ro.n_truncated)
        rec["explained_variance_returns"] = PPO.explained_variance_(ro, "returns")
        rec["explained_variance_lambda_returns"] = PPO.explained_variance_(ro, "lambda_returns")
        ph, eh, _ = PPO.ppo_train_(pol, opt, ds, 0.05, 4096, 4, 0.01, seed=it, verbose=False, advantage="gae")
        vh, _ = PPO.value_train_(critic, copt, ds, 4096, 4, target="lambda_returns", seed=it, verbose=False)
        rec.update(value_loss=vh[-1], ppo_loss=ph[-1], entropy_loss=eh[-1])
        curve.append(rec)
    m, s = PPO.average_returns(pol, ev, 1024)
    curve.append({"iteration": ITERS, "average_return": m, "std": s})
    PPO.synchronize()
    out["runs"][mode] = {"curve": curve, "wall_s_incl_evaluator_and_host_copies": time.perf_counter() - t0}
    print(mode, "average return", " -> ".join("%.2f" % c["average_return"] for c in curve if "average_return" in c))
    for k in ("explained_variance_returns", "explained_variance_lambda_returns"):
        print(mode, k, " ".join("%.2f" % c[k] for c in curve if k in c))
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "gae_boot_learning_curve.json")
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(out, open(OUT, "w"), indent=1)
