#!/usr/bin/env python3
"""What the teacher-forced forward (k_policy_fwd MODE 11) costs beside the sampled per-step forward (MODE 1).

4096 envs, Policy(72,256,2,4), Q = 8, max_actions = T = 128.  Three variants, each T launches of its forward over all envs:

  parent_sampled   the library and package of the parent commit (a checkout of it, built, named with --parent-root):
                   collect_rollouts_steps_ with the per-step launches (set_rollout_persistent(False)), k_policy_fwd_rollout;
  branch_sampled   this tree, the same call: the sampled forward must be what it was;
  branch_forced    this tree, collect_paths_ of 4096 paths of T flips on quads that stay active (reset states as starts):
                   k_policy_fwd_forced, k_env_step_forced.

A library is loaded once per process, so every variant runs in a child process of its own (one warm-up call, then one timed
call on a fresh identical env); the driver alternates the children, three rounds, and takes the median of three: us per
forward launch, us per env-step launch, wall ms of the call.  The forced forward is judged against the parent's median plus
the parent's own run-to-run spread (highest minus lowest of its three runs in this same call).

A record, not a gate.  Writes profiles/collect_paths_timing.json (without --parent-root: the two branch variants alone, to
profiles/collect_paths_timing_branch_only.json), or the file named last.
Usage: tools/collect_paths_timing.py [--parent-root DIR] [out.json]"""
import json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, HID, T, ROUNDS = 4096, 256, 128, 3
SCOPES = {"sampled": ("k_policy_fwd_rollout", "k_env_step"), "forced": ("k_policy_fwd_forced", "k_env_step_forced")}


def child(root, kind):
    sys.path.insert(0, root)
    import ppo_amd as PPO
    pol = PPO.HipPolicy(72, HID, 2, 4, seed=0)
    PPO.set_rollout_persistent(False)
    PPO.set_rollout_compact(False)
    rng = np.random.default_rng(3)
    # flips (types 0 and 1) on quads 0 .. 5: active in every reset state, and flips keep the set of active quads
    paths = (16 * rng.integers(0, 6, (N, T)) + 4 * rng.integers(0, 4, (N, T)) + rng.integers(0, 2, (N, T)) + 1).astype(np.int16)
    out = None
    for timed in (False, True):
        env = PPO.HipVecEnv(num_envs=N, Q=8, max_actions=T, seed=7)
        ro = PPO.BufferRollouts()
        it = env.internal()
        starts = (it["score"], it["degree"], env.active_quads())
        PPO.synchronize()
        PPO.profile_enable(True)
        t0 = time.perf_counter()
        if kind == "forced":
            PPO.collect_paths_(ro, env, pol, *starts, paths, 1.0)
        else:
            PPO.collect_rollouts_steps_(ro, env, pol, T, 1.0)
        PPO.synchronize()
        wall = time.perf_counter() - t0
        fwd, step = SCOPES[kind]
        d = {"wall_ms": 1e3 * wall, "transitions": len(ro)}
        for name, k in (("forward", fwd), ("env_step", step), ("observe", "k_env_observe")):
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


def main(argv):
    parent_root = None
    if "--parent-root" in argv:
        i = argv.index("--parent-root")
        parent_root = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    default = "collect_paths_timing.json" if parent_root else "collect_paths_timing_branch_only.json"
    out_path = argv[0] if argv else os.path.join(ROOT, "profiles", default)
    variants = ([("parent_sampled", parent_root, "sampled")] if parent_root else []) + \
        [("branch_sampled", ROOT, "sampled"), ("branch_forced", ROOT, "forced")]
    runs = {v: [] for v, _, _ in variants}
    for rnd in range(ROUNDS):
        for v, root, kind in variants:
            d = run_child(root, kind)
            runs[v].append(d)
            print(rnd, v, round(d["forward"]["mean_us"], 2), round(d["env_step"]["mean_us"], 2), round(d["wall_ms"], 2), flush=True)
    summary = {}
    for v, ds in runs.items():
        s = {"forward_kernel": ds[0]["forward"]["kernel"], "forward_launches": ds[0]["forward"]["launches"],
             "transitions": ds[0]["transitions"]}
        for name, f in (("forward_us", lambda d: d["forward"]["mean_us"]), ("env_step_us", lambda d: d["env_step"]["mean_us"]),
                        ("observe_us", lambda d: d["observe"]["mean_us"]), ("wall_ms", lambda d: d["wall_ms"])):
            x = [f(d) for d in ds]
            s[name] = {"median": float(np.median(x)), "min": min(x), "max": max(x)}
        summary[v] = s
    verdict = {}
    if parent_root:
        p, b, f = (summary[v]["forward_us"] for v in ("parent_sampled", "branch_sampled", "branch_forced"))
        bar = p["median"] + (p["max"] - p["min"])
        verdict = {"bar_us": bar, "forced_no_slower_than_bar": bool(f["median"] <= bar), "forced_over_parent": f["median"] / p["median"],
                   "branch_sampled_inside_parent_spread": bool(p["min"] <= b["median"] <= p["max"]),
                   "branch_sampled_over_parent": b["median"] / p["median"]}
    out = {"workload": "%d envs, Policy(72,%d,2,4), Q = 8, T = max_actions = %d, expanded storage, per-step launches; every variant in "
                       "its own process, alternating, medians (and min, max) of %d runs" % (N, HID, T, ROUNDS),
           "summary": summary, "against_parent": verdict, "runs": runs}
    print(json.dumps({"summary": summary, "against_parent": verdict}, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(out, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        main(sys.argv[1:])
