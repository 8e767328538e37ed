"""Summed gaps on 7o's setting: untrained Policy(72,256,2,4) seed 0, 64 starts at K = 64, plain / children / parents."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ppo_amd as PPO
N, K, T = 4096, 64, 128
pol = PPO.HipPolicy(72, 256, 2, 4, seed=0)
src = PPO.HipVecEnv(num_envs=N // K, Q=8, max_actions=T, seed=11)
it = src.internal()
starts = (it["score"], it["degree"], src.active_quads())
out = {}
for mode, rounds in ((None, 4), ("children", 4), ("parents", 1), ("parents", 4), ("parents", 16)):
    r = PPO.beam_search_states_distinct_(PPO.HipVecEnv(num_envs=N, Q=8, max_actions=T, seed=7), pol, *starts, K, distinct=mode, rounds=rounds)
    out["%s_rounds%d" % (mode, rounds)] = {"initial_gap_sum": int(r["initial_gap"].sum()), "best_gap_sum": int(r["best_gap"].sum()),
                                           "mean_best_step": float(r["best_step"].mean())}
print(json.dumps(out, indent=1))
