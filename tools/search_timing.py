#!/usr/bin/env python3
"""What the best-state bookkeeping costs the env step, and what the best-of-K search delivers.

1. Tracking cost: best_states_ against evaluate_trajectories("best") on the same env shape, policy and trajectory count
   (4096 envs, Policy(72,256,2,4), max_actions 128, one trajectory per env), alternating, three rounds, each on a fresh
   identical env so both play the same trajectories.  Per call: the library's own k_env_step profile scope (the tracked
   step reports under the same name), k_policy_fwd_rollout of the same steps beside it, and the wall time.
2. Search throughput: search_best_states_ with 64 starts x 64 clones on 4096 envs (one round), env-steps per second of
   wall time (the steps are the tick advance of the envs).

A record, not a gate.  Writes profiles/search_timing.json, or the file named first.  Usage: tools/search_timing.py [out.json]"""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ppo_amd as PPO

N, HID, MAX_ACTIONS, ROUNDS = 4096, 256, 128, 3
KW = dict(num_envs=N, Q=8, max_actions=MAX_ACTIONS, seed=7)
pol = PPO.HipPolicy(72, HID, 2, 4, seed=0)


def profiled(fn):
    """(result, wall seconds, {scope: (total ms, launches)}) of one call on a fresh env."""
    env = PPO.HipVecEnv(**KW)
    PPO.synchronize()
    PPO.profile_enable(True)
    t0 = time.perf_counter()
    r = fn(env)
    PPO.synchronize()
    wall = time.perf_counter() - t0
    scopes = {k: PPO.profile_get(k) for k in ("k_env_step", "k_policy_fwd_rollout", "k_env_observe")}
    PPO.profile_enable(False)
    return r, wall, scopes, env


def row(wall, scopes):
    d = {"wall_ms": 1e3 * wall}
    for k, (ms, n) in scopes.items():
        d[k] = {"total_ms": ms, "launches": int(n), "mean_us": 1e3 * ms / max(n, 1)}
    return d


out = {"tracking": {"workload": "%d envs, Policy(72,%d,2,4), max_actions %d, %d trajectories, Q = 8" % (N, HID, MAX_ACTIONS, N),
                    "rounds": []}}
tracked = lambda env: PPO.best_states_(env, pol, N)
plain = lambda env: PPO.evaluate_trajectories(env, pol, N, "best")
for fn in (plain, tracked):                                   # warm-up: allocations, code objects
    profiled(fn)
for _ in range(ROUNDS):
    b, wb, sb, _ = profiled(plain)
    t, wt, st, _ = profiled(tracked)
    assert np.array_equal(t["length"] > 0, np.ones(N, bool))
    out["tracking"]["rounds"].append({"evaluate_best": row(wb, sb), "best_states": row(wt, st)})
    print(json.dumps(out["tracking"]["rounds"][-1]))
rs = out["tracking"]["rounds"]
med = lambda who, k: float(np.median([r[who][k]["mean_us"] for r in rs]))
out["tracking"]["median_mean_us"] = {who: {k: med(who, k) for k in ("k_env_step", "k_policy_fwd_rollout")}
                                     for who in ("evaluate_best", "best_states")}
m = out["tracking"]["median_mean_us"]
out["tracking"]["tracked_over_plain_env_step"] = m["best_states"]["k_env_step"] / m["evaluate_best"]["k_env_step"]
out["tracking"]["tracked_env_step_over_policy_forward"] = m["best_states"]["k_env_step"] / m["best_states"]["k_policy_fwd_rollout"]

# ---- search: 64 starts x 64 clones, one round on 4096 envs
M, K = 64, 64
src = PPO.HipVecEnv(num_envs=M, Q=8, max_actions=MAX_ACTIONS, seed=11)
it = src.internal()
starts = (it["score"], it["degree"], src.active_quads())
runs = []
for i in range(ROUNDS + 1):
    (r, wall, scopes, env) = profiled(lambda env: PPO.search_best_states_(env, pol, *starts, K))
    steps = int(env.internal()["tick"].astype(np.int64).sum())
    if i:                                                     # the first run is the warm-up
        runs.append({"wall_ms": 1e3 * wall, "env_steps": steps, "env_steps_per_s": steps / wall,
                     "mean_initial_gap": float(r["initial_gap"].mean()), "mean_best_gap": float(r["best_gap"].mean())})
        print(json.dumps(runs[-1]))
out["search"] = {"workload": "%d starts x %d clones, %d envs, Policy(72,%d,2,4), max_actions %d" % (M, K, N, HID, MAX_ACTIONS),
                 "runs": runs, "median_env_steps_per_s": float(np.median([r["env_steps_per_s"] for r in runs]))}
print(json.dumps({k: v for k, v in out["tracking"].items() if k != "rounds"}), json.dumps(out["search"]["median_env_steps_per_s"]))
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "search_timing.json")
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(out, open(OUT, "w"), indent=1)
