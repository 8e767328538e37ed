#!/usr/bin/env python3
"""What a step of beam search costs beside a step of the best-of-K search.

The benchmark's env shape: 4096 envs, Policy(72,256,2,4), Q = 8, max_actions = 128.  K = 64 and K = 256, one round
(num_starts = N / K starts, the reset states of the first envs), so every resident env is a slot.

  branch_beam     this tree: beam_search_states_(path=True); per step the probabilities forward over all envs
                  (k_policy_fwd_probs), k_beam_select, k_beam_expand, k_env_observe;
  parent_search   the library and package of the parent commit (a checkout of it, built, named with --parent-root):
                  search_best_states_(path=True) at the same N, K and starts: per step k_policy_fwd_rollout, k_env_step,
                  k_env_observe -- the per-step cost the existing searches pay.

A library is loaded once per process, so every (variant, K) runs in a child process of its own: one warm-up call, then
CALLS timed calls, each on a fresh identical env, with the library's kernel-timing tables on (HIP events around every launch).
The driver alternates the children, ROUNDS rounds; reported per (variant, K): median, min and max over all timed calls of the
wall time of the call and of the mean time per launch of every kernel, and the steps a call ran.

A record, not a gate.  Writes profiles/beam_search_timing.json (without --parent-root: the beam alone, to
profiles/beam_search_timing_branch_only.json), or the file named last.
Usage: tools/beam_search_timing.py [--parent-root DIR] [out.json]"""
import json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, HID, T, ROUNDS, CALLS = 4096, 256, 128, 2, 5
KERNELS = {"beam": ("k_policy_fwd_probs", "k_beam_select", "k_beam_expand", "k_env_observe"),
           "search": ("k_policy_fwd_rollout", "k_env_step", "k_env_observe")}


def child(root, kind, K):
    sys.path.insert(0, root)
    import ppo_amd as PPO
    pol = PPO.HipPolicy(72, HID, 2, 4, seed=0)
    src = PPO.HipVecEnv(num_envs=N // K, Q=8, max_actions=T, seed=11)
    it = src.internal()
    starts = (it["score"], it["degree"], src.active_quads())
    out = []
    for call in range(CALLS + 1):
        env = PPO.HipVecEnv(num_envs=N, Q=8, max_actions=T, seed=7)
        PPO.synchronize()
        PPO.profile_enable(True)
        t0 = time.perf_counter()
        if kind == "beam":
            r = PPO.beam_search_states_(env, pol, *starts, K, path=True)
        else:
            r = PPO.search_best_states_(env, pol, *starts, K, path=True)
        PPO.synchronize()
        d = {"wall_ms": 1e3 * (time.perf_counter() - t0), "best_gap_sum": int(r["best_gap"].sum()),
             "initial_gap_sum": int(r["initial_gap"].sum())}
        for k in KERNELS[kind]:
            ms, n = PPO.profile_get(k)
            d[k] = {"launches": int(n), "mean_us": 1e3 * ms / max(n, 1)}
        PPO.profile_enable(False)
        if call:                                                 # call 0 is the warm-up
            out.append(d)
    print("RESULT " + json.dumps(out))


def run_child(root, kind, K):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, kind, str(K)], capture_output=True, text=True,
                       timeout=300)
    if p.returncode != 0:
        sys.exit("child %s %s %d failed (%d):\n%s" % (root, kind, K, p.returncode, p.stderr[-2000:]))
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def stats(x):
    return {"median": float(np.median(x)), "min": float(min(x)), "max": float(max(x))}


def main(argv):
    parent_root = None
    if "--parent-root" in argv:
        i = argv.index("--parent-root")
        parent_root = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    default = "beam_search_timing.json" if parent_root else "beam_search_timing_branch_only.json"
    out_path = argv[0] if argv else os.path.join(ROOT, "profiles", default)
    variants = [("branch_beam", ROOT, "beam")] + ([("parent_search", parent_root, "search")] if parent_root else [])
    runs = {}
    for rnd in range(ROUNDS):
        for K in (64, 256):
            for v, root, kind in variants:
                ds = run_child(root, kind, K)
                runs.setdefault("%s_K%d" % (v, K), []).extend(ds)
                print(rnd, v, K, [round(d["wall_ms"], 2) for d in ds], flush=True)
    summary = {}
    for key, ds in runs.items():
        kind = "beam" if key.startswith("branch_beam") else "search"
        s = {"calls": len(ds), "wall_ms": stats([d["wall_ms"] for d in ds]), "steps": ds[0]["k_env_observe"]["launches"],
             "best_gap_sum": ds[0]["best_gap_sum"], "initial_gap_sum": ds[0]["initial_gap_sum"]}
        for k in KERNELS[kind]:
            s[k + "_us"] = stats([d[k]["mean_us"] for d in ds])
        per_step = [sum(d[k]["mean_us"] for k in KERNELS[kind]) for d in ds]
        s["kernels_per_step_us"] = stats(per_step)
        summary[key] = s
    out = {"workload": "%d envs, Policy(72,%d,2,4), Q = 8, max_actions = %d, one round of N / K starts; every (variant, K) in its own "
                       "process, alternating, %d rounds of one warm-up and %d timed calls; median (min, max) over the timed calls"
                       % (N, HID, T, ROUNDS, CALLS),
           "summary": summary, "runs": runs}
    print(json.dumps(summary, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(out, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    else:
        main(sys.argv[1:])
