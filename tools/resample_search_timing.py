#!/usr/bin/env python3
"""What a resample event costs and what the resampling search delivers against the best-of-K search.

4096 envs, Policy(72,256,2,4), max_actions 128, 64 starts x 64 clones (one round), survivors 16: search_resample_states_ at
intervals 1, 4 and 16 against search_best_states_, each call on a fresh identical env, the four alternating, three rounds
behind one warm-up round.  Per call: wall time, env-steps (the tick advance of the envs) per second of it, the library's own
profile scopes -- k_search_resample (one launch per event), the tracked step (k_env_step) and the policy forward
(k_policy_fwd_rollout) of the same loop -- and the mean best gap over the starts.

A record, not a gate.  Writes profiles/resample_search_timing.json, or the file named first.
Usage: tools/resample_search_timing.py [out.json]"""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ppo_amd as PPO

N, HID, MAX_ACTIONS, ROUNDS = 4096, 256, 128, 3
M, K, SURVIVORS, INTERVALS = 64, 64, 16, (1, 4, 16)
KW = dict(num_envs=N, Q=8, max_actions=MAX_ACTIONS, seed=7)
SCOPES = ("k_search_resample", "k_env_step", "k_policy_fwd_rollout", "k_env_observe")
pol = PPO.HipPolicy(72, HID, 2, 4, seed=0)
src = PPO.HipVecEnv(num_envs=M, Q=8, max_actions=MAX_ACTIONS, seed=11)
it = src.internal()
starts = (it["score"], it["degree"], src.active_quads())


def profiled(fn):
    """One call on a fresh env: wall time, env-steps, the scopes and the gaps."""
    env = PPO.HipVecEnv(**KW)
    PPO.synchronize()
    PPO.profile_enable(True)
    t0 = time.perf_counter()
    r = fn(env)
    PPO.synchronize()
    wall = time.perf_counter() - t0
    scopes = {k: PPO.profile_get(k) for k in SCOPES}
    PPO.profile_enable(False)
    steps = int(env.internal()["tick"].astype(np.int64).sum())
    d = {"wall_ms": 1e3 * wall, "env_steps": steps, "env_steps_per_s": steps / wall,
         "mean_initial_gap": float(r["initial_gap"].mean()), "mean_best_gap": float(r["best_gap"].mean())}
    for k, (ms, n) in scopes.items():
        d[k] = {"total_ms": ms, "launches": int(n), "mean_us": 1e3 * ms / max(n, 1)}
    return d


calls = {"best_of_k": lambda env: PPO.search_best_states_(env, pol, *starts, K)}
for R in INTERVALS:
    calls["interval_%d" % R] = (lambda R: lambda env: PPO.search_resample_states_(env, pol, *starts, K, R, SURVIVORS))(R)
runs = {name: [] for name in calls}
for i in range(ROUNDS + 1):
    for name, fn in calls.items():
        d = profiled(fn)
        if i:                                                 # the first round is the warm-up: allocations, code objects
            runs[name].append(d)
            print(name, json.dumps(d))
med = lambda name, f: float(np.median([f(d) for d in runs[name]]))
summary = {}
for name in calls:
    summary[name] = {"wall_ms": med(name, lambda d: d["wall_ms"]), "env_steps": med(name, lambda d: d["env_steps"]),
                     "env_steps_per_s": med(name, lambda d: d["env_steps_per_s"]),
                     "mean_best_gap": med(name, lambda d: d["mean_best_gap"]),
                     "mean_initial_gap": med(name, lambda d: d["mean_initial_gap"]),
                     "events": med(name, lambda d: d["k_search_resample"]["launches"]),
                     "k_search_resample_us": med(name, lambda d: d["k_search_resample"]["mean_us"]),
                     "k_env_step_us": med(name, lambda d: d["k_env_step"]["mean_us"]),
                     "k_policy_fwd_rollout_us": med(name, lambda d: d["k_policy_fwd_rollout"]["mean_us"])}
    s = summary[name]
    s["event_over_forward"] = s["k_search_resample_us"] / s["k_policy_fwd_rollout_us"]
out = {"workload": "%d starts x %d clones, survivors %d, %d envs, Policy(72,%d,2,4), max_actions %d, Q = 8; medians of %d runs"
                   % (M, K, SURVIVORS, N, HID, MAX_ACTIONS, ROUNDS),
       "median": summary, "runs": runs}
print(json.dumps(summary, indent=1))
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "resample_search_timing.json")
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(out, open(OUT, "w"), indent=1)
