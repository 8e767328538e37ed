#!/usr/bin/env python3
"""What the action paths cost the resampling search.

The workload of tools/resample_search_timing.py: 4096 envs, Policy(72,256,2,4), max_actions 128, 64 starts x 64 clones (one
round), survivors 16, search_resample_states_ at intervals 1, 4 and 16, every call on a fresh identical env.  Three variants:

  parent        the library and package of the parent commit (a checkout of it, built, named with --parent-root);
  branch        this tree, path=False: the event must run the work it ran before;
  branch_path   this tree, path=True: the tracked step stores its action, a copy carries the donor's played prefix, a fold
                that takes a record takes its path.

A library is loaded once per process, so every variant runs in a child process of its own (one warm-up pass over the three
intervals, then one timed pass); the driver alternates the children parent, branch, branch_path, three rounds, and takes the
median of three per variant and interval: us per event (k_search_resample, one launch per event), us per tracked step
(k_env_step), wall ms of the call.  The branch without the path is judged against the parent's own run-to-run spread (its
lowest and highest of the three runs of this same call); with the path the ratio to the parent's event is reported.

A record, not a gate.  Writes profiles/search_paths_timing.json (without --parent-root: the two branch variants alone, to
profiles/search_paths_timing_branch_only.json), or the file named last.
Usage: tools/search_paths_timing.py [--parent-root DIR] [out.json]"""
import json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, HID, MAX_ACTIONS, ROUNDS = 4096, 256, 128, 3
M, K, SURVIVORS, INTERVALS = 64, 64, 16, (1, 4, 16)
SCOPES = ("k_search_resample", "k_env_step", "k_policy_fwd_rollout")


def child(root, with_path):
    sys.path.insert(0, root)
    import ppo_amd as PPO
    pol = PPO.HipPolicy(72, HID, 2, 4, seed=0)
    src = PPO.HipVecEnv(num_envs=M, Q=8, max_actions=MAX_ACTIONS, seed=11)
    it = src.internal()
    starts = (it["score"], it["degree"], src.active_quads())
    kw = {"path": True} if with_path else {}
    out = {}
    for timed in (False, True):
        for R in INTERVALS:
            env = PPO.HipVecEnv(num_envs=N, Q=8, max_actions=MAX_ACTIONS, seed=7)
            PPO.synchronize()
            PPO.profile_enable(True)
            t0 = time.perf_counter()
            r = PPO.search_resample_states_(env, pol, *starts, K, R, SURVIVORS, **kw)
            PPO.synchronize()
            wall = time.perf_counter() - t0
            d = {"wall_ms": 1e3 * wall, "mean_best_gap": float(r["best_gap"].mean()),
                 "mean_best_step": float(r["best_step"].mean())}
            for k in SCOPES:
                ms, n = PPO.profile_get(k)
                d[k] = {"launches": int(n), "mean_us": 1e3 * ms / max(n, 1)}
            PPO.profile_enable(False)
            if timed:
                out["interval_%d" % R] = d
    print("RESULT " + json.dumps(out))


def run_child(root, with_path):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, str(int(with_path))], capture_output=True,
                       text=True, timeout=300)
    if p.returncode != 0:
        sys.exit("child %s failed (%d):\n%s" % (root, p.returncode, p.stderr[-2000:]))
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main(argv):
    parent_root = None
    if "--parent-root" in argv:
        i = argv.index("--parent-root")
        parent_root = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    # the committed record holds all three variants: a run without the parent never lands on it by default
    default = "search_paths_timing.json" if parent_root else "search_paths_timing_branch_only.json"
    out_path = argv[0] if argv else os.path.join(ROOT, "profiles", default)
    variants = ([("parent", parent_root, False)] if parent_root else []) + [("branch", ROOT, False), ("branch_path", ROOT, True)]
    runs = {v: {"interval_%d" % R: [] for R in INTERVALS} for v, _, _ in variants}
    for rnd in range(ROUNDS):
        for v, root, with_path in variants:
            res = run_child(root, with_path)
            for k, d in res.items():
                runs[v][k].append(d)
            print(rnd, v, json.dumps({k: (round(d["k_search_resample"]["mean_us"], 2), round(d["k_env_step"]["mean_us"], 2),
                                          round(d["wall_ms"], 2)) for k, d in res.items()}), flush=True)
    pick = {"event_us": lambda d: d["k_search_resample"]["mean_us"], "tracked_step_us": lambda d: d["k_env_step"]["mean_us"],
            "forward_us": lambda d: d["k_policy_fwd_rollout"]["mean_us"], "wall_ms": lambda d: d["wall_ms"]}
    summary = {}
    for v in runs:
        summary[v] = {}
        for k, ds in runs[v].items():
            s = {"events": ds[0]["k_search_resample"]["launches"], "mean_best_gap": ds[0]["mean_best_gap"],
                 "mean_best_step": ds[0]["mean_best_step"]}
            for name, f in pick.items():
                x = [f(d) for d in ds]
                s[name] = {"median": float(np.median(x)), "min": min(x), "max": max(x)}
            summary[v][k] = s
    verdict = {}
    if parent_root:
        for k in summary["parent"]:
            verdict[k] = {}
            for name in ("event_us", "tracked_step_us", "wall_ms"):
                p, b, bp = (summary[v][k][name] for v in ("parent", "branch", "branch_path"))
                verdict[k][name] = {"branch_inside_parent_spread": bool(p["min"] <= b["median"] <= p["max"]),
                                    "branch_over_parent": b["median"] / p["median"],
                                    "branch_path_over_parent": bp["median"] / p["median"]}
    out = {"workload": "%d starts x %d clones, survivors %d, %d envs, Policy(72,%d,2,4), max_actions %d, Q = 8; every variant in "
                       "its own process, alternating, medians (and min, max) of %d runs"
                       % (M, K, SURVIVORS, N, HID, MAX_ACTIONS, ROUNDS),
           "summary": summary, "against_parent": verdict, "runs": runs}
    print(json.dumps({"summary": summary, "against_parent": verdict}, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(out, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], bool(int(sys.argv[3])))
    else:
        main(sys.argv[1:])
