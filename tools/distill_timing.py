#!/usr/bin/env python3
"""What the distillation train forward (k_policy_fwd MODE 17) costs beside the imitation train forward (MODE 12), a
whole distill_train_ call beside imitate_train_, and fill_targets_ over a whole buffer.

4096 envs, Policy(72,256,2,4), Q = 8, T = max_actions = 128, expanded storage, one epoch of 128 minibatches of 4096.  Variants:

  parent_imitate  the library and package of the parent commit (a checkout of it, built, named with --parent-root):
                  imitate_train_ (uniform weights, default knobs) -- MODE 12 must be what it was;
  branch_imitate  this tree, the same call;
  branch_distill  this tree, fill_targets_ with a teacher of the same shape (timed by itself: wall ms around the call and a
                  synchronize, 524,288 states), then distill_train_ on that column: MODE 17 between MODE 12's neighbours.

A library is loaded once per process, so every variant runs in a child process of its own (one warm-up call, then one timed
call); the driver alternates the children, three rounds, and reports min / median / max of three: us per train-forward launch,
wall ms of the call, wall ms of the fill.  The distillation forward reads 512 B more per state than imitation's (2 MiB per
launch here); what that costs is reported against branch_imitate's median of the same call of this tool.

A record, not a gate.  Writes profiles/distill_timing.json (without --parent-root: the branch variants alone, to
profiles/distill_timing_branch_only.json), or the file named last.
Usage: tools/distill_timing.py [--parent-root DIR] [out.json]"""
import json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, HID, T, MB, ROUNDS = 4096, 256, 128, 4096, 3
KINDS = {"imitate": "k_policy_fwd_imitate", "distill": "k_policy_fwd_distill"}


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
    fill_ms = []
    if kind == "distill":
        teacher = PPO.HipPolicy(72, HID, 2, 4, seed=5)
        for _ in range(2):
            PPO.synchronize()
            t0 = time.perf_counter()
            PPO.fill_targets_(ro, teacher)
            PPO.synchronize()
            fill_ms.append(1e3 * (time.perf_counter() - t0))
    out = None
    for timed in (False, True):
        PPO.synchronize()
        PPO.profile_enable(True)
        t0 = time.perf_counter()
        if kind == "distill":
            PPO.distill_train_(pol, opt, ds, MB, 1, 0.01, seed=1, verbose=False)
        else:
            PPO.imitate_train_(pol, opt, ds, MB, 1, 0.01, seed=1, verbose=False)
        PPO.synchronize()
        wall = time.perf_counter() - t0
        ms, n = PPO.profile_get(scope)
        out = {"wall_ms": 1e3 * wall, "forward": {"scope": scope, "launches": int(n), "mean_us": 1e3 * ms / max(n, 1)}}
        PPO.profile_enable(False)
    if fill_ms:
        out["fill_ms"] = fill_ms[-1]
        out["fill_states"] = N * T
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
    default = "distill_timing.json" if parent_root else "distill_timing_branch_only.json"
    out_path = argv[0] if argv else os.path.join(ROOT, "profiles", default)
    variants = ([("parent_imitate", parent_root, "imitate")] if parent_root else []) + \
        [("branch_imitate", ROOT, "imitate"), ("branch_distill", ROOT, "distill")]
    runs = {v: [] for v, _, _ in variants}
    for rnd in range(ROUNDS):
        for v, root, kind in variants:
            d = run_child(root, kind)
            runs[v].append(d)
            print(rnd, v, round(d["forward"]["mean_us"], 2), round(d["wall_ms"], 2), round(d.get("fill_ms", 0.0), 2), flush=True)
    summary = {}
    for v, ds in runs.items():
        s = {"forward_scope": ds[0]["forward"]["scope"], "forward_launches": ds[0]["forward"]["launches"]}
        fields = [("forward_us", lambda d: d["forward"]["mean_us"]), ("wall_ms", lambda d: d["wall_ms"])]
        if "fill_ms" in ds[0]:
            fields.append(("fill_ms", lambda d: d["fill_ms"]))
            s["fill_states"] = ds[0]["fill_states"]
        for name, f in fields:
            x = [f(d) for d in ds]
            s[name] = {"median": float(np.median(x)), "min": min(x), "max": max(x)}
        summary[v] = s
    bi, bd = summary["branch_imitate"], summary["branch_distill"]
    verdict = {"distill_forward_over_imitate_forward": bd["forward_us"]["median"] / bi["forward_us"]["median"],
               "distill_forward_minus_imitate_forward_us": bd["forward_us"]["median"] - bi["forward_us"]["median"],
               "imitate_forward_spread_us": bi["forward_us"]["max"] - bi["forward_us"]["min"],
               "distill_call_over_imitate_call": bd["wall_ms"]["median"] / bi["wall_ms"]["median"],
               "fill_ns_per_state": 1e6 * bd["fill_ms"]["median"] / bd["fill_states"]}
    if parent_root:
        p = summary["parent_imitate"]["forward_us"]
        verdict.update({"branch_imitate_inside_parent_spread": bool(p["min"] <= bi["forward_us"]["median"] <= p["max"]),
                        "branch_imitate_over_parent": bi["forward_us"]["median"] / p["median"]})
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
