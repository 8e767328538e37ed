#!/usr/bin/env python3
"""What the truncated-sampling forward (k_policy_fwd mode 16) costs beside the tempered one (mode 14), and what
top-k / nucleus truncation does to a search.  tools/select_timing.py's shape and method.

Timing.  4096 envs, Policy(72,256,2,4), max_actions = 128, best_states_ with 4096 trajectories (one per env), one launch of the
forward over all envs per loop step.  Variants:

  parent_tempered        the library and package of the parent commit (a checkout of it, built, named with --parent-root),
                         ("sample", 0.5): k_policy_fwd_tempered;
  parent_default         the parent, default selection: k_policy_fwd_rollout;
  branch_default         this tree, default selection and truncation: k_policy_fwd_rollout through launch_policy_select;
  branch_tempered        this tree, ("sample", 0.5), default truncation: k_policy_fwd_tempered;
  branch_top_k5          this tree, ("sample", 0.5) + (5, 1.0): k_policy_fwd_truncated;
  branch_top_p09         this tree, ("sample", 0.5) + (0, 0.9): k_policy_fwd_truncated;
  branch_q32_tempered    this tree, Q = 32 (512 actions, four tiles per state), ("sample", 0.5): k_policy_fwd_tempered;
  branch_q32_top_p09     this tree, Q = 32, ("sample", 0.5) + (0, 0.9): k_policy_fwd_truncated.

A library is loaded once per process, so every variant runs in a child process of its own (one warm-up call, then one timed
call on a fresh identical env); the driver alternates the children, three rounds: min / median / max of us per forward launch.
The branch's default and tempered medians are judged against the parent's median of the same kernel plus the parent's own
run-to-run spread; the truncated forward is reported against the parent's tempered median and has no bar.

Search quality (--quality, one process, no parent): the resampling search of tools/resample_search_timing.py (64 starts x 64
clones, interval 4, 16 survivors, max_actions 128, Policy(72,256,2,4)) at temperatures 1 and 2 with no truncation, (0, 0.9)
and (5, 1.0): the mean best gap over the starts and -- from a plain roll-out of the same 64 clones per start -- the mean number
of distinct action sequences among a start's clones.  Once on the untrained policy of seed 0 and once on that policy sharpened
by SHARPEN_ROUNDS rounds of the loop of examples/train_on_search_paths.py (search_best_states_(path) at temperature 1 ->
collect_paths_ -> imitate_train_, 256 starts x 16 clones per round), restated here because the example trains a hidden-128
policy on max_actions 32.

A record, not a gate.  Writes profiles/truncate_timing.json (without --parent-root: the branch variants alone, to
profiles/truncate_timing_branch_only.json; --quality: profiles/truncate_search_quality.json), or the file named last.
Usage: tools/truncate_timing.py [--parent-root DIR | --quality] [out.json]"""
import json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, HID, T, ROUNDS, SHARPEN_ROUNDS = 4096, 256, 128, 3, 5
TEMPERED = ("sample", 0.5)
KINDS = {"default": (8, None, None, "k_policy_fwd_rollout"), "tempered": (8, TEMPERED, None, "k_policy_fwd_tempered"),
         "top_k5": (8, TEMPERED, (5, 1.0), "k_policy_fwd_truncated"), "top_p09": (8, TEMPERED, (0, 0.9), "k_policy_fwd_truncated"),
         "q32_tempered": (32, TEMPERED, None, "k_policy_fwd_tempered"),
         "q32_top_p09": (32, TEMPERED, (0, 0.9), "k_policy_fwd_truncated")}


def child(root, kind):
    sys.path.insert(0, root)
    import ppo_amd as PPO
    pol = PPO.HipPolicy(72, HID, 2, 4, seed=0)
    Q, sel, trunc, fwd = KINDS[kind]
    if sel is not None:
        pol.selection = sel
    if trunc is not None:
        pol.truncation = trunc
    out = None
    for timed in (False, True):
        env = PPO.HipVecEnv(num_envs=N, Q=Q, max_actions=T, seed=7)
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


def sharpen(PPO, policy):
    """SHARPEN_ROUNDS rounds of the example's loop on `policy`: best-of-16 search paths of 256 fresh starts, cloned."""
    optimizer = PPO.Optimiser(PPO.Adam(3e-4))
    search_env = PPO.HipVecEnv(num_envs=256 * 16, Q=8, max_actions=T, seed=7)
    env = PPO.HipVecEnv(num_envs=256, Q=8, max_actions=T, seed=8)
    rollouts = PPO.BufferRollouts()
    log = []
    for r in range(SHARPEN_ROUNDS):
        fresh = PPO.HipVecEnv(num_envs=256, Q=8, max_actions=T, seed=1000 + r)
        st = fresh.internal()
        starts = (st["score"], st["degree"], fresh.active_quads())
        found = PPO.search_best_states_(search_env, policy, *starts, 16, path=True)
        PPO.collect_paths_(rollouts, env, policy, *starts, found["path"], 1.0)
        dataset = PPO.construct_dataset(rollouts)
        ph, eh, _ = PPO.imitate_train_(policy, optimizer, dataset, min(1024, len(dataset)), 2, 0.01, seed=r, verbose=False,
                                       weights="uniform", advantage="returns")
        log.append({"round": r, "search_mean_best_gap": float(found["best_gap"].mean()), "transitions": len(dataset),
                    "clone_loss": float(ph[-1])})
        print("sharpen", json.dumps(log[-1]), flush=True)
    return log


def quality(out_path):
    sys.path.insert(0, ROOT)
    import ppo_amd as PPO
    M, K, R, SURVIVORS = 64, 64, 4, 16
    src = PPO.HipVecEnv(num_envs=M, Q=8, max_actions=T, seed=11)
    it = src.internal()
    starts = (it["score"], it["degree"], src.active_quads())
    clones = tuple(np.repeat(x, K, axis=0) for x in starts)
    out = {"workload": "%d starts x %d clones, interval %d, %d survivors, %d envs, Policy(72,%d,2,4) seed 0, max_actions %d, Q = 8; one "
                       "call per setting on a fresh env; sharpened: %d rounds of search_best_states_(path, 256 starts x 16 clones) "
                       "-> collect_paths_ -> imitate_train_(uniform, 2 epochs, Adam 3e-4)" % (M, K, R, SURVIVORS, N, HID, T, SHARPEN_ROUNDS)}
    pol = PPO.HipPolicy(72, HID, 2, 4, seed=0)
    for name in ("untrained", "sharpened"):
        if name == "sharpened":
            out["sharpen_log"] = sharpen(PPO, pol)
        rows = {}
        for tau in (1.0, 2.0):
            for trunc in ((0, 1.0), (0, 0.9), (5, 1.0)):
                with PPO.selecting(pol, "sample", tau, *trunc):
                    env = PPO.HipVecEnv(num_envs=N, Q=8, max_actions=T, seed=7)
                    r = PPO.search_resample_states_(env, pol, *starts, K, R, SURVIVORS)
                    best = PPO.search_best_states_(PPO.HipVecEnv(num_envs=N, Q=8, max_actions=T, seed=7), pol, *starts, K)
                    env = PPO.HipVecEnv(num_envs=N, Q=8, max_actions=T, seed=7)
                    env.set_internal(*clones)
                    acts = PPO._best_states(env, pol, N, False, False, False, True)["actions"].reshape(M, K, T)
                distinct = [len({a.tobytes() for a in acts[s]}) for s in range(M)]
                prefix8 = [len({a[:8].tobytes() for a in acts[s]}) for s in range(M)]
                key = "tau %g, top_k %d, top_p %g" % (tau, trunc[0], trunc[1])
                rows[key] = {"mean_initial_gap": float(r["initial_gap"].mean()), "resample_mean_best_gap": float(r["best_gap"].mean()),
                             "best_of_k_mean_best_gap": float(best["best_gap"].mean()),
                             "mean_distinct_clone_paths": float(np.mean(distinct)),
                             "mean_distinct_first_8_actions": float(np.mean(prefix8))}
                print(name, key, json.dumps(rows[key]), flush=True)
        out[name] = rows
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(out, open(out_path, "w"), indent=1)


def main(argv):
    if "--quality" in argv:
        argv.remove("--quality")
        return quality(argv[0] if argv else os.path.join(ROOT, "profiles", "truncate_search_quality.json"))
    parent_root = None
    if "--parent-root" in argv:
        i = argv.index("--parent-root")
        parent_root = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    default = "truncate_timing.json" if parent_root else "truncate_timing_branch_only.json"
    out_path = argv[0] if argv else os.path.join(ROOT, "profiles", default)
    variants = ([("parent_tempered", parent_root, "tempered"), ("parent_default", parent_root, "default")] if parent_root else []) + \
        [("branch_" + k, ROOT, k) for k in ("default", "tempered", "top_k5", "top_p09", "q32_tempered", "q32_top_p09")]
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
    fw = {v: summary[v]["forward_us"] for v in summary}
    verdict = {"q32_truncated_minus_tempered_us": fw["branch_q32_top_p09"]["median"] - fw["branch_q32_tempered"]["median"],
               "q32_rank_pass_exceeds_the_forward": bool(fw["branch_q32_top_p09"]["median"] > 2 * fw["branch_q32_tempered"]["median"]),
               "q8_top_k5_minus_tempered_us": fw["branch_top_k5"]["median"] - fw["branch_tempered"]["median"],
               "q8_top_p09_minus_tempered_us": fw["branch_top_p09"]["median"] - fw["branch_tempered"]["median"]}
    if parent_root:
        p14, p1 = fw["parent_tempered"], fw["parent_default"]
        bar14, bar1 = p14["median"] + (p14["max"] - p14["min"]), p1["median"] + (p1["max"] - p1["min"])
        verdict.update({"bar_tempered_us": bar14, "bar_default_us": bar1,
                        "branch_tempered_no_slower_than_bar": bool(fw["branch_tempered"]["median"] <= bar14),
                        "branch_default_no_slower_than_bar": bool(fw["branch_default"]["median"] <= bar1),
                        "branch_default_no_slower_than_tempered_bar": bool(fw["branch_default"]["median"] <= bar14),
                        "top_k5_over_parent_tempered": fw["branch_top_k5"]["median"] / p14["median"],
                        "top_p09_over_parent_tempered": fw["branch_top_p09"]["median"] / p14["median"]})
    out = {"workload": "%d envs, Policy(72,%d,2,4), Q = 8 (q32: 32), max_actions = %d, best_states_ with %d trajectories; every variant "
                       "in its own process, alternating, medians (and min, max) of %d runs" % (N, HID, T, N, ROUNDS),
           "summary": summary, "verdict": verdict, "runs": runs}
    print(json.dumps({"summary": summary, "verdict": verdict}, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(out, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        main(sys.argv[1:])
