#!/usr/bin/env python3
"""What a step of the distinct beam costs beside a step of the plain beam, with tools/beam_search_timing.py's
protocol.

The benchmark's env shape: 4096 envs, Policy(72,256,2,4), Q = 8, max_actions = 128.  K = 64 and K = 256, one round
(num_starts = N / K starts, the reset states of the first envs), so every resident env is a slot.

  branch_distinct  this tree: beam_search_states_distinct_(path=True, distinct="parents", rounds=R), R = 1 and 4; per step the
                   probabilities forward (k_policy_fwd_probs), R launches each of k_beam_select_window and k_beam_children,
                   one k_beam_commit, k_env_observe;
  parent_beam      the library and package of the parent commit (a checkout of it, built, named with --parent-root):
                   beam_search_states_(path=True) at the same N, K and starts: k_policy_fwd_probs, k_beam_select,
                   k_beam_expand, k_env_observe.

A library is loaded once per process, so every (variant, K, R) runs in a child process of its own: one warm-up call -- for the
distinct beam with log=True, from whose `examined` the windows a step actually used are counted --, then CALLS timed calls, each
on a fresh identical env, with the library's kernel-timing tables on (HIP events around every launch).  The driver alternates
the children, ROUNDS rounds; reported per variant: median, min and max over all timed calls of the wall time of the call and of
the time PER STEP of every kernel (its total over the call divided by the steps the call ran: a step launches the windowed
select and the children kernel R times), and the steps a call ran.  The cost scales with the rounds a policy makes necessary.

A record, not a gate.  Writes profiles/beam_distinct_timing.json (without --parent-root: the distinct beam alone, to
profiles/beam_distinct_timing_branch_only.json), or the file named last.
Usage: tools/beam_distinct_timing.py [--parent-root DIR] [out.json]"""
import json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, HID, T, ROUNDS, CALLS = 4096, 256, 128, 2, 5
KERNELS = {"distinct": ("k_policy_fwd_probs", "k_beam_select_window", "k_beam_children", "k_beam_commit", "k_env_observe"),
           "plain": ("k_policy_fwd_probs", "k_beam_select", "k_beam_expand", "k_env_observe")}


def child(root, kind, K, R):
    sys.path.insert(0, root)
    import ppo_amd as PPO
    pol = PPO.HipPolicy(72, HID, 2, 4, seed=0)
    src = PPO.HipVecEnv(num_envs=N // K, Q=8, max_actions=T, seed=11)
    it = src.internal()
    starts = (it["score"], it["degree"], src.active_quads())
    opts = dict(distinct="parents", rounds=R) if kind == "distinct" else {}
    out, windows = [], None
    for call in range(CALLS + 1):
        env = PPO.HipVecEnv(num_envs=N, Q=8, max_actions=T, seed=7)
        PPO.synchronize()
        PPO.profile_enable(True)
        t0 = time.perf_counter()
        search = PPO.beam_search_states_distinct_ if kind == "distinct" else PPO.beam_search_states_
        r = search(env, pol, *starts, K, path=True, log=(call == 0 and kind == "distinct"), **opts)
        PPO.synchronize()
        d = {"wall_ms": 1e3 * (time.perf_counter() - t0), "best_gap_sum": int(r["best_gap"].sum()),
             "initial_gap_sum": int(r["initial_gap"].sum())}
        steps = max(PPO.profile_get("k_env_observe")[1], 1)
        d["steps"] = int(steps)
        for k in KERNELS[kind]:
            ms, n = PPO.profile_get(k)
            d[k] = {"launches": int(n), "us_per_step": 1e3 * ms / steps}
        PPO.profile_enable(False)
        if call:                                                 # call 0 is the warm-up
            out.append(d)
        elif kind == "distinct":
            ex = r["examined"][r["examined"] >= 0]
            used = -(-ex // 256)
            windows = {"mean_per_step": float(used.mean()), "max": int(used.max()),
                       "histogram": {str(w): int((used == w).sum()) for w in range(0, R + 1)},
                       "accepted_mean": float((r["rank"] >= 0).sum(axis=2)[r["examined"] >= 0].mean())}
    print("RESULT " + json.dumps({"calls": out, "windows": windows}))


def run_child(root, kind, K, R):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, kind, str(K), str(R)], capture_output=True,
                       text=True, timeout=300)
    if p.returncode != 0:
        sys.exit("child %s %s %d %d failed (%d):\n%s" % (root, kind, K, R, p.returncode, p.stderr[-2000:]))
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def stats(x):
    return {"median": float(np.median(x)), "min": float(min(x)), "max": float(max(x))}


def main(argv):
    parent_root = None
    if "--parent-root" in argv:
        i = argv.index("--parent-root")
        parent_root = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    default = "beam_distinct_timing.json" if parent_root else "beam_distinct_timing_branch_only.json"
    out_path = argv[0] if argv else os.path.join(ROOT, "profiles", default)
    runs, windows = {}, {}
    for rnd in range(ROUNDS):
        for K in (64, 256):
            variants = [("branch_distinct_K%d_rounds%d" % (K, R), ROOT, "distinct", R) for R in (1, 4)]
            if parent_root:
                variants.insert(1, ("parent_beam_K%d" % K, parent_root, "plain", 0))
            for key, root, kind, R in variants:
                res = run_child(root, kind, K, R)
                runs.setdefault(key, []).extend(res["calls"])
                if res["windows"]:
                    windows[key] = res["windows"]
                print(rnd, key, [round(d["wall_ms"], 2) for d in res["calls"]], flush=True)
    summary = {}
    for key, ds in runs.items():
        kind = "distinct" if key.startswith("branch_distinct") else "plain"
        s = {"calls": len(ds), "wall_ms": stats([d["wall_ms"] for d in ds]), "steps": ds[0]["steps"],
             "best_gap_sum": ds[0]["best_gap_sum"], "initial_gap_sum": ds[0]["initial_gap_sum"]}
        for k in KERNELS[kind]:
            s[k + "_us_per_step"] = stats([d[k]["us_per_step"] for d in ds])
        s["kernels_per_step_us"] = stats([sum(d[k]["us_per_step"] for k in KERNELS[kind]) for d in ds])
        if key in windows:
            s["windows_used"] = windows[key]
        summary[key] = s
    out = {"workload": "%d envs, Policy(72,%d,2,4), Q = 8, max_actions = %d, one round of N / K starts, mode parents; every variant in "
                       "its own process, alternating, %d rounds of one warm-up and %d timed calls; median (min, max) over the timed "
                       "calls; kernel times are per STEP (total of the call / steps)" % (N, HID, T, ROUNDS, CALLS),
           "summary": summary, "runs": runs}
    print(json.dumps(summary, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(out, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]))
    else:
        main(sys.argv[1:])
