#!/usr/bin/env python3
"""What the imitation train forward (k_policy_fwd MODE 12) costs beside the fp32-MFMA PPO train forward (MODE 2),
and a whole imitate_train_ call beside ppo_train_.

4096 envs, Policy(72,256,2,4), Q = 8, T = max_actions = 128, expanded storage, one epoch of 128 minibatches of 4096.  Variants:

  parent_fp32     the library and package of the parent commit (a checkout of it, built, named with --parent-root):
                  ppo_train_ after set_bwd_split_bf16(0) -- k_policy_fwd MODE 2 and the fp32 fused backward;
  branch_fp32     this tree, the same call: MODE 2 must be what it was;
  branch_imitate_fp32  this tree, imitate_train_ (uniform weights) after set_bwd_split_bf16(0): MODE 12 between the same
                  neighbours as MODE 2 above (the fp32 backward, Adam) -- the like-for-like comparison of the two forwards;
  branch_imitate  this tree, imitate_train_ under the default knobs: MODE 12 and the split-fp32 backward;
  branch_ppo      this tree, ppo_train_ under the default knobs (the split-fp32 train forward), for the whole-call comparison.

A library is loaded once per process, so every variant runs in a child process of its own (one warm-up call, then one timed
call); the driver alternates the children, three rounds, and takes the median of three: us per train-forward launch and wall ms
of the call.  The imitation forward (like for like) is judged against the parent's median plus the parent's own run-to-run
spread (highest minus lowest of its three runs in this same call); the default-knob figure is reported beside it.

A record, not a gate.  Writes profiles/imitation_timing.json (without --parent-root: the branch variants alone, to
profiles/imitation_timing_branch_only.json), or the file named last.
Usage: tools/imitation_timing.py [--parent-root DIR] [out.json]"""
import json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, HID, T, MB, ROUNDS = 4096, 256, 128, 4096, 3
KINDS = {"fp32": ("k_policy_fwd_train", 0), "ppo": ("k_policy_fwd_train", None), "imitate": ("k_policy_fwd_imitate", None),
         "imitate_fp32": ("k_policy_fwd_imitate", 0)}


def child(root, kind):
    sys.path.insert(0, root)
    import ppo_amd as PPO
    scope, split = KINDS[kind]
    PPO.set_rollout_compact(False)
    env = PPO.HipVecEnv(num_envs=N, Q=8, max_actions=T, seed=7)
    pol = PPO.HipPolicy(72, HID, 2, 4, seed=0)
    ro = PPO.BufferRollouts()
    PPO.collect_rollouts_steps_(ro, env, pol, T, 1.0)
    ds = PPO.construct_dataset(ro)
    opt = PPO.Optimiser(PPO.Adam(1e-5))
    PPO.set_bwd_split_bf16(split)
    out = None
    for timed in (False, True):
        PPO.synchronize()
        PPO.profile_enable(True)
        t0 = time.perf_counter()
        if kind.startswith("imitate"):
            PPO.imitate_train_(pol, opt, ds, MB, 1, 0.01, seed=1, verbose=False)
        else:
            PPO.ppo_train_(pol, opt, ds, 0.05, MB, 1, 0.01, seed=1, verbose=False)
        PPO.synchronize()
        wall = time.perf_counter() - t0
        ms, n = PPO.profile_get(scope)
        out = {"wall_ms": 1e3 * wall, "forward": {"scope": scope, "launches": int(n), "mean_us": 1e3 * ms / max(n, 1)}}
        PPO.profile_enable(False)
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
    default = "imitation_timing.json" if parent_root else "imitation_timing_branch_only.json"
    out_path = argv[0] if argv else os.path.join(ROOT, "profiles", default)
    variants = ([("parent_fp32", parent_root, "fp32")] if parent_root else []) + \
        [("branch_fp32", ROOT, "fp32"), ("branch_imitate_fp32", ROOT, "imitate_fp32"), ("branch_imitate", ROOT, "imitate"),
         ("branch_ppo", ROOT, "ppo")]
    runs = {v: [] for v, _, _ in variants}
    for rnd in range(ROUNDS):
        for v, root, kind in variants:
            d = run_child(root, kind)
            runs[v].append(d)
            print(rnd, v, round(d["forward"]["mean_us"], 2), round(d["wall_ms"], 2), flush=True)
    summary = {}
    for v, ds in runs.items():
        s = {"forward_scope": ds[0]["forward"]["scope"], "forward_launches": ds[0]["forward"]["launches"]}
        for name, f in (("forward_us", lambda d: d["forward"]["mean_us"]), ("wall_ms", lambda d: d["wall_ms"])):
            x = [f(d) for d in ds]
            s[name] = {"median": float(np.median(x)), "min": min(x), "max": max(x)}
        summary[v] = s
    verdict = {"imitate_call_over_ppo_call": summary["branch_imitate"]["wall_ms"]["median"] / summary["branch_ppo"]["wall_ms"]["median"]}
    if parent_root:
        p, b, f, d = (summary[v]["forward_us"] for v in ("parent_fp32", "branch_fp32", "branch_imitate_fp32", "branch_imitate"))
        bar = p["median"] + (p["max"] - p["min"])
        verdict.update({"bar_us": bar, "imitate_no_slower_than_bar": bool(f["median"] <= bar), "imitate_over_parent": f["median"] / p["median"],
                        "imitate_default_knobs_over_parent": d["median"] / p["median"],
                        "branch_fp32_inside_parent_spread": bool(p["min"] <= b["median"] <= p["max"]),
                        "branch_fp32_over_parent": b["median"] / p["median"]})
    out = {"workload": "%d envs, Policy(72,%d,2,4), Q = 8, T = max_actions = %d, expanded storage, one epoch of minibatches of %d; every "
                       "variant in its own process, alternating, medians (and min, max) of %d runs" % (N, HID, T, MB, ROUNDS),
           "summary": summary, "verdict": verdict, "runs": runs}
    print(json.dumps({"summary": summary, "verdict": verdict}, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(out, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        main(sys.argv[1:])
