#!/usr/bin/env python3
"""tools/learning_curve.py's schedule (4096 envs x 128 steps, Policy(72,256,2,4), 4 epochs, minibatch 4096, Adam 3e-4, same
seeds, fp32) once with the returns advantage and once with a device critic (GAE(gamma, 0.95) from its values, the critic
trained on the lambda-returns with Adam 1e-3): the evaluator's average return every four iterations and, for the critic
run, the explained variance 1 - Var(returns - V) / Var(returns) of the values it had BEFORE each update.  A record, not a
gate.  Both runs keep learning_curve.py's gamma = 1.0.  Writes profiles/value_learning_curve.json, or the file
named second.  Usage: tools/value_learning_curve.py [iterations] [out.json]"""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ppo_amd as PPO

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 24
LAM = 0.95
out = {"workload": "4096 envs x 128 steps, Policy(72,256,2,4), 4 epochs, minibatch 4096, gamma 1.0, eps 0.05, entropy_weight 0.01, "
                   "Adam 3e-4; critic: HipCritic(72,256,2), GAE lambda %.2f, Adam 1e-3, 4 epochs on the lambda-returns" % LAM, "runs": {}}
for mode in ("returns", "critic"):
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
        if mode == "critic":
            v = PPO.compute_values_(ro, env, critic)[:-1]
            ret = ro.rewards
            rec["explained_variance"] = float(1.0 - np.var(ret - v) / max(np.var(ret), 1e-12))
            PPO.compute_gae_critic_(ro, env, critic, 1.0, LAM, fetch=False)
            ph, eh, _ = PPO.ppo_train_(pol, opt, ds, 0.05, 4096, 4, 0.01, seed=it, verbose=False, advantage="gae")
            vh, _ = PPO.value_train_(critic, copt, ds, 4096, 4, target="lambda_returns", seed=it, verbose=False)
            rec["value_loss"] = vh[-1]
        else:
            ph, eh, _ = PPO.ppo_train_(pol, opt, ds, 0.05, 4096, 4, 0.01, seed=it, verbose=False)
        rec.update(ppo_loss=ph[-1], entropy_loss=eh[-1])
        curve.append(rec)
    m, s = PPO.average_returns(pol, ev, 1024)
    curve.append({"iteration": ITERS, "average_return": m, "std": s})
    PPO.synchronize()
    out["runs"][mode] = {"curve": curve, "wall_s_incl_evaluator_and_host_copies": time.perf_counter() - t0}
    print(mode, "average return", " -> ".join("%.2f" % c["average_return"] for c in curve if "average_return" in c))
    if mode == "critic":
        print("explained variance", " ".join("%.2f" % c["explained_variance"] for c in curve if "explained_variance" in c))
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "value_learning_curve.json")
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(out, open(OUT, "w"), indent=1)
