#!/usr/bin/env python3
"""What the selection forwards (k_policy_fwd modes 14 / 15) cost beside the sampled per-step forward (MODE 1),
and what the temperature does to a search.

Timing.  4096 envs, Policy(72,256,2,4), Q = 8, max_actions = 128, best_states_ with 4096 trajectories (one per env).  Four
variants, each one launch of its forward over all envs per loop step:

  parent_sampled    the library and package of the parent commit (a checkout of it, built, named with --parent-root):
                    k_policy_fwd_rollout;
  branch_sampled    this tree, the default selection: the same kernel through launch_policy_select's fall-through;
  branch_tempered   this tree, ("sample", 0.5): k_policy_fwd_tempered;
  branch_greedy     this tree, ("greedy", 1.0): k_policy_fwd_greedy.

A library is loaded once per process, so every variant runs in a child process of its own (one warm-up call, then one timed
call on a fresh identical env); the driver alternates the children, three rounds, and takes the median of three: us per
forward launch, us per env-step launch, wall ms of the call.  The tempered forward is judged against the parent's median plus
the parent's own run-to-run spread (highest minus lowest of its three runs in this same call); the greedy forward is reported
against the parent's median.

Search quality (--quality, one process, no parent): the resampling search of tools/resample_search_timing.py (64 starts x 64
clones, interval 4, 16 survivors) at temperatures 0.5, 1 and 2: the mean best gap over the starts, and -- from a plain roll-out
of the same 64 clones per start, best_states_ without a reset -- the mean number of distinct action sequences among a start's
clones.

A record, not a gate.  Writes profiles/select_timing.json (without --parent-root: the branch variants alone, to
profiles/select_timing_branch_only.json; --quality: profiles/select_search_quality.json), or the file named last.
Usage: tools/select_timing.py [--parent-root DIR | --quality] [out.json]"""
import json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, HID, T, ROUNDS = 4096, 256, 128, 3
KINDS = {"sampled": (None, "k_policy_fwd_rollout"), "tempered": (("sample", 0.5), "k_policy_fwd_tempered"),
         "greedy": (("greedy", 1.0), "k_policy_fwd_greedy")}


def child(root, kind):
    sys.path.insert(0, root)
    import ppo_amd as PPO
    pol = PPO.HipPolicy(72, HID, 2, 4, seed=0)
    sel, fwd = KINDS[kind]
    if sel is not None:
        pol.selection = sel
    out = None
    for timed in (False, True):
        env = PPO.HipVecEnv(num_envs=N, Q=8, max_actions=T, seed=7)
        PPO.synchronize()
        PPO.profile_enable(True)
        t0 = time.perf_counter()
        r = PPO.best_states_(env, pol, N)
        PPO.synchronize()
        wall = time.perf_counter() - t0
        d = {"wall_ms": 1e3 * wall, "env_steps": int(r["length"].sum()), "mean_best_gap": float(r["best_gap"].mean())}
        for name, k in (("forward", fwd), ("env_step", "k_env_step"), ("observe", "k_env_observe")):
            ms, n = PPO.profile_get(k)
            d[name] = {"kernel": k, "launches": int(n), "mean_us": 1e3 * ms / max(n, 1)}
        PPO.profile_enable(False)
        if timed:
            out = d
    print("RESULT " + json.dumps(out))


def run_child(root, kind):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, kind], capture_output=True, text=True,
                       timeout=300)
    if p.returncode != 0:
        sys.exit("child %s %s failed (%d):\n%s" % (root, kind, p.returncode, p.stderr[-2000:]))
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def quality(out_path):
    sys.path.insert(0, ROOT)
    import ppo_amd as PPO
    M, K, R, SURVIVORS = 64, 64, 4, 16
    src = PPO.HipVecEnv(num_envs=M, Q=8, max_actions=T, seed=11)
    it = src.internal()
    starts = (it["score"], it["degree"], src.active_quads())
    clones = tuple(np.repeat(x, K, axis=0) for x in starts)
    rows = {}
    for tau in (0.5, 1.0, 2.0):
        pol = PPO.HipPolicy(72, HID, 2, 4, seed=0)
        pol.selection = ("sample", tau)
        env = PPO.HipVecEnv(num_envs=N, Q=8, max_actions=T, seed=7)
        r = PPO.search_resample_states_(env, pol, *starts, K, R, SURVIVORS)
        best = PPO.search_best_states_(PPO.HipVecEnv(num_envs=N, Q=8, max_actions=T, seed=7), pol, *starts, K)
        env = PPO.HipVecEnv(num_envs=N, Q=8, max_actions=T, seed=7)
        env.set_internal(*clones)
        acts = PPO._best_states(env, pol, N, False, False, False, True)["actions"].reshape(M, K, T)
        distinct = [len({a.tobytes() for a in acts[s]}) for s in range(M)]
        prefix8 = [len({a[:8].tobytes() for a in acts[s]}) for s in range(M)]
        rows["%g" % tau] = {"mean_initial_gap": float(r["initial_gap"].mean()), "resample_mean_best_gap": float(r["best_gap"].mean()),
                            "best_of_k_mean_best_gap": float(best["best_gap"].mean()),
                            "mean_distinct_clone_paths": float(np.mean(distinct)),
                            "mean_distinct_first_8_actions": float(np.mean(prefix8))}
        print(tau, json.dumps(rows["%g" % tau]), flush=True)
    out = {"workload": "%d starts x %d clones, interval %d, %d survivors, %d envs, untrained Policy(72,%d,2,4) seed 0, max_actions %d, "
                       "Q = 8; one call per temperature on a fresh env" % (M, K, R, SURVIVORS, N, HID, T), "by_temperature": rows}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(out, open(out_path, "w"), indent=1)


def main(argv):
    if "--quality" in argv:
        argv.remove("--quality")
        return quality(argv[0] if argv else os.path.join(ROOT, "profiles", "select_search_quality.json"))
    parent_root = None
    if "--parent-root" in argv:
        i = argv.index("--parent-root")
        parent_root = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    default = "select_timing.json" if parent_root else "select_timing_branch_only.json"
    out_path = argv[0] if argv else os.path.join(ROOT, "profiles", default)
    variants = ([("parent_sampled", parent_root, "sampled")] if parent_root else []) + \
        [("branch_sampled", ROOT, "sampled"), ("branch_tempered", ROOT, "tempered"), ("branch_greedy", ROOT, "greedy")]
    runs = {v: [] for v, _, _ in variants}
    for rnd in range(ROUNDS):
        for v, root, kind in variants:
            d = run_child(root, kind)
            runs[v].append(d)
            print(rnd, v, round(d["forward"]["mean_us"], 2), round(d["env_step"]["mean_us"], 2), round(d["wall_ms"], 2), flush=True)
    summary = {}
    for v, ds in runs.items():
        s = {"forward_kernel": ds[0]["forward"]["kernel"], "forward_launches": ds[0]["forward"]["launches"],
             "env_steps": ds[0]["env_steps"], "mean_best_gap": ds[0]["mean_best_gap"]}
        for name, f in (("forward_us", lambda d: d["forward"]["mean_us"]), ("env_step_us", lambda d: d["env_step"]["mean_us"]),
                        ("observe_us", lambda d: d["observe"]["mean_us"]), ("wall_ms", lambda d: d["wall_ms"])):
            x = [f(d) for d in ds]
            s[name] = {"median": float(np.median(x)), "min": min(x), "max": max(x)}
        summary[v] = s
    verdict = {}
    if parent_root:
        p, b, t, g = (summary[v]["forward_us"] for v in ("parent_sampled", "branch_sampled", "branch_tempered", "branch_greedy"))
        bar = p["median"] + (p["max"] - p["min"])
        verdict = {"bar_us": bar, "tempered_no_slower_than_bar": bool(t["median"] <= bar), "tempered_over_parent": t["median"] / p["median"],
                   "greedy_below_parent_median": bool(g["median"] < p["median"]), "greedy_over_parent": g["median"] / p["median"],
                   "greedy_minus_parent_us": g["median"] - p["median"],
                   "branch_sampled_inside_parent_spread": bool(p["min"] <= b["median"] <= p["max"]),
                   "branch_sampled_over_parent": b["median"] / p["median"]}
    out = {"workload": "%d envs, Policy(72,%d,2,4), Q = 8, max_actions = %d, best_states_ with %d trajectories; every variant in "
                       "its own process, alternating, medians (and min, max) of %d runs" % (N, HID, T, N, ROUNDS),
           "summary": summary, "against_parent": verdict, "runs": runs}
    print(json.dumps({"summary": summary, "against_parent": verdict}, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(out, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        main(sys.argv[1:])
