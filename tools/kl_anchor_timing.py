#!/usr/bin/env python3
"""What the KL-anchored train forward (k_policy_fwd MODE 20) costs beside the two forwards whose halves it joins:
the distillation train forward (MODE 17) and the plain objective's Train-mode k_policy_fwd (MODE 2, forced onto that kernel with
set_bwd_split_bf16(0), set_train_tile_max_tiles(0) and set_fwd_split_max_states(0)).

4096 envs, Policy(72,256,2,4), Q = 8, T = max_actions = 128, expanded storage, one epoch of 128 minibatches of 4096 (the headline
minibatch).  Variants:

  parent_distill  the library and package of the parent commit (a checkout of it, built, named with --parent-root):
                  distill_train_ on a filled column -- MODE 17;
  parent_train    the same checkout: ppo_train_ under the three knobs above -- MODE 2;
  branch_distill, branch_train   this tree, the same two calls: both kernels must be what they were;
  branch_anchored this tree: ppo_train_ with kl_anchor = (1.0, "column") under the same knobs (the backward is then the one
                  branch_train runs) -- MODE 20.

A library is loaded once per process, so every variant runs in a child process of its own (one warm-up call, then one timed
call); the driver alternates the children, three rounds, and reports min / median / max of three: us per train-forward launch and
wall ms of the call.  A record, not a gate.  Writes profiles/kl_anchor_timing.json (without --parent-root: the branch variants
alone, to profiles/kl_anchor_timing_branch_only.json), or the file named last.
Usage: tools/kl_anchor_timing.py [--parent-root DIR] [out.json]"""
import json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, HID, T, MB, ROUNDS = 4096, 256, 128, 4096, 3
KINDS = {"distill": "k_policy_fwd_distill", "train": "k_policy_fwd_train", "anchored": "k_policy_fwd_train_anchored"}


def child(root, kind):
    sys.path.insert(0, root)
    import ppo_amd as PPO
    scope = KINDS[kind]
    PPO.set_rollout_compact(False)
    env = PPO.HipVecEnv(num_envs=N, Q=8, max_actions=T, seed=7)
    pol = PPO.HipPolicy(72, HID, 2, 4, seed=0)
    ro = PPO.BufferRollouts()
    PPO.collect_rollouts_steps_(ro, env, pol, T, 1.0)
    ds = PPO.construct_dataset(ro)
    opt = PPO.Optimiser(PPO.Adam(1e-5))
    if kind != "train":
        PPO.fill_targets_(ro, PPO.HipPolicy(72, HID, 2, 4, seed=5))
    if kind != "distill":
        PPO.set_bwd_split_bf16(0)
        PPO.set_train_tile_max_tiles(0)
        PPO.set_fwd_split_max_states(0)
    if kind == "anchored":
        pol.kl_anchor = (1.0, "column")
    out = None
    for timed in (False, True):
        PPO.synchronize()
        PPO.profile_enable(True)
        t0 = time.perf_counter()
        if kind == "distill":
            PPO.distill_train_(pol, opt, ds, MB, 1, 0.01, seed=1, verbose=False)
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
    default = "kl_anchor_timing.json" if parent_root else "kl_anchor_timing_branch_only.json"
    out_path = argv[0] if argv else os.path.join(ROOT, "profiles", default)
    variants = ([("parent_distill", parent_root, "distill"), ("parent_train", parent_root, "train")] if parent_root else []) + \
        [("branch_distill", ROOT, "distill"), ("branch_train", ROOT, "train"), ("branch_anchored", ROOT, "anchored")]
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
    side = "parent" if parent_root else "branch"
    slower = max(summary[side + "_distill"]["forward_us"]["median"], summary[side + "_train"]["forward_us"]["median"])
    verdict = {"anchored_forward_over_slower_of_%s_distill_and_train" % side: summary["branch_anchored"]["forward_us"]["median"] / slower,
               "anchored_forward_minus_slower_us": summary["branch_anchored"]["forward_us"]["median"] - slower}
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
