#!/usr/bin/env python3
"""What ranking by the critic's value costs the resampling search, and what it finds.

The workload of tools/resample_search_timing.py: 4096 envs, Policy(72,256,2,4), max_actions 128, 64 starts x 64 clones (one
round), survivors 16, search_resample_states_ at intervals 1, 4 and 16, every call on a fresh identical env.  Variants:

  parent             the library and package of the parent commit (a checkout of it, built, named with --parent-root);
  branch             this tree without a critic: the event must run the work it ran before;
  branch_value_256   this tree, critic HipCritic(72,256,2), value_weight 1;
  branch_value_64    this tree, critic HipCritic(72,64,2) (zero-padded to the 128 kernel), value_weight 1.

A first child process trains the policy with the 256 critic for TRAIN_ITERS ppo_iterate_ rounds (4096 episodes each, discount
1, so the critic estimates the score reduction still to come), then fits both critics to the final policy for FIT_ITERS rounds
of collect / GAE / value_train_, and leaves all three parameter vectors in a file every other child loads: all variants
search with the same policy.  A library is loaded once per process, so every variant runs in a child of its own (one warm-up
pass over the intervals, then one timed pass); the driver alternates the children, three rounds, and takes the median (and
min, max) of three per variant and interval: wall ms of the call; us per event (k_search_resample), per observation
(k_env_observe: the loop's and the events'), per value forward (k_value_fwd_predict), per tracked step (k_env_step) and per
policy forward; the mean best gap over the starts.  The branch without a critic is judged against the parent's own
run-to-run spread; there is no bar on the gap.

A record, not a gate.  Writes profiles/value_resample_timing.json (without --parent-root:
profiles/value_resample_timing_branch_only.json), or the file named last.
Usage: tools/value_resample_timing.py [--parent-root DIR] [out.json]"""
import json, os, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, HID, MAX_ACTIONS, ROUNDS = 4096, 256, 128, 3
M, K, SURVIVORS, INTERVALS = 64, 64, 16, (1, 4, 16)
TRAIN_ITERS, FIT_ITERS, EPOCHS, MB = 3, 2, 4, 4096
CRITICS = {"value_256": 256, "value_64": 64}
SCOPES = ("k_search_resample", "k_env_step", "k_policy_fwd_rollout", "k_env_observe", "k_value_fwd_predict")


def train(params_path):
    sys.path.insert(0, ROOT)
    import ppo_amd as PPO

    class Evaluator:
        def __call__(self, policy, env, optimizer):
            pass
    PPO.save_loss.register(Evaluator)(lambda ev, loss: None)
    env = PPO.HipVecEnv(num_envs=N, Q=8, max_actions=MAX_ACTIONS, seed=7)
    pol, opt = PPO.HipPolicy(72, HID, 2, 4, seed=0), PPO.Optimiser(PPO.Adam(3e-4))
    critics = {k: PPO.HipCritic(72, h, 2, seed=1) for k, h in CRITICS.items()}
    copts = {k: PPO.Optimiser(PPO.Adam(1e-3)) for k in CRITICS}
    loss = PPO.ppo_iterate_(pol, env, opt, N, MB, TRAIN_ITERS, Evaluator(), EPOCHS, 1.0, 0.05, 0.01, verbose=False,
                            critic=critics["value_256"], critic_optimizer=copts["value_256"], gae_lambda=0.95)
    fit = {k: [] for k in CRITICS}
    for it in range(FIT_ITERS):
        ro = PPO.BufferRollouts()
        PPO.collect_rollouts_(ro, env, pol, N, 1.0)
        ds = PPO.construct_dataset(ro)
        for k in CRITICS:
            PPO.compute_gae_critic_(ro, env, critics[k], 1.0, 0.95, fetch=False)
            v, _ = PPO.value_train_(critics[k], copts[k], ds, MB, EPOCHS, target="lambda_returns", seed=it + 1, verbose=False)
            fit[k] += v
    np.savez(params_path, policy=pol.params, **{k: c.params for k, c in critics.items()})
    print("RESULT " + json.dumps({"value_loss_while_training": loss["value"], "value_loss_fitting": fit}))


def child(root, mode, params_path):
    sys.path.insert(0, root)
    import ppo_amd as PPO
    par = np.load(params_path)
    pol = PPO.HipPolicy(72, HID, 2, 4, seed=0)
    pol.params = par["policy"]
    kw = {}
    if mode in CRITICS:
        critic = PPO.HipCritic(72, CRITICS[mode], 2, seed=1)
        critic.params = par[mode]
        kw = {"critic": critic, "value_weight": 1.0}
    src = PPO.HipVecEnv(num_envs=M, Q=8, max_actions=MAX_ACTIONS, seed=11)
    it = src.internal()
    starts = (it["score"], it["degree"], src.active_quads())
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
                 "mean_initial_gap": float(r["initial_gap"].mean()), "mean_best_step": float(r["best_step"].mean())}
            for k in SCOPES:
                ms, n = PPO.profile_get(k)
                d[k] = {"launches": int(n), "mean_us": 1e3 * ms / max(n, 1)}
            PPO.profile_enable(False)
            if timed:
                out["interval_%d" % R] = d
    print("RESULT " + json.dumps(out))


def run_child(*args):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + list(args), capture_output=True, text=True,
                       timeout=600)
    if p.returncode != 0:
        sys.exit("child %s failed (%d):\n%s" % (args, p.returncode, p.stderr[-2000:]))
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main(argv):
    parent_root = None
    if "--parent-root" in argv:
        i = argv.index("--parent-root")
        parent_root = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    default = "value_resample_timing.json" if parent_root else "value_resample_timing_branch_only.json"
    out_path = argv[0] if argv else os.path.join(ROOT, "profiles", default)
    variants = ([("parent", parent_root, "plain")] if parent_root else []) + [("branch", ROOT, "plain")] + \
               [("branch_" + k, ROOT, k) for k in CRITICS]
    with tempfile.TemporaryDirectory() as tmp:
        params = os.path.join(tmp, "params.npz")
        training = run_child("train", params)
        print("trained", json.dumps(training), flush=True)
        runs = {v: {"interval_%d" % R: [] for R in INTERVALS} for v, _, _ in variants}
        for rnd in range(ROUNDS):
            for v, root, mode in variants:
                res = run_child(root, mode, params)
                for k, d in res.items():
                    runs[v][k].append(d)
                print(rnd, v, json.dumps({k: (round(d["k_search_resample"]["mean_us"], 2), round(d["k_env_step"]["mean_us"], 2),
                                              round(d["wall_ms"], 2), d["mean_best_gap"]) for k, d in res.items()}), flush=True)
    pick = {"event_us": lambda d: d["k_search_resample"]["mean_us"], "observe_us": lambda d: d["k_env_observe"]["mean_us"],
            "value_forward_us": lambda d: d["k_value_fwd_predict"]["mean_us"], "tracked_step_us": lambda d: d["k_env_step"]["mean_us"],
            "forward_us": lambda d: d["k_policy_fwd_rollout"]["mean_us"], "wall_ms": lambda d: d["wall_ms"]}
    summary = {}
    for v in runs:
        summary[v] = {}
        for k, ds in runs[v].items():
            s = {"events": ds[0]["k_search_resample"]["launches"], "value_forwards": ds[0]["k_value_fwd_predict"]["launches"],
                 "mean_initial_gap": ds[0]["mean_initial_gap"], "mean_best_gap": ds[0]["mean_best_gap"],
                 "mean_best_step": ds[0]["mean_best_step"]}
            for name, f in pick.items():
                x = [f(d) for d in ds]
                s[name] = {"median": float(np.median(x)), "min": min(x), "max": max(x)}
            summary[v][k] = s
    verdict = {}
    for k in summary["branch"]:
        verdict[k] = {}
        for name in ("event_us", "tracked_step_us", "wall_ms"):
            b = summary["branch"][k][name]
            e = {"value_%d_over_branch" % h: summary["branch_value_%d" % h][k][name]["median"] / b["median"] for h in CRITICS.values()}
            if parent_root:
                p = summary["parent"][k][name]
                e.update(branch_inside_parent_spread=bool(p["min"] <= b["median"] <= p["max"]), branch_over_parent=b["median"] / p["median"])
            verdict[k][name] = e
    out = {"workload": "%d starts x %d clones, survivors %d, %d envs, Policy(72,%d,2,4), max_actions %d, Q = 8, value_weight 1; "
                       "policy and critics trained for %d ppo_iterate_ rounds and %d fitting rounds; every variant in its own "
                       "process, alternating, medians (and min, max) of %d runs"
                       % (M, K, SURVIVORS, N, HID, MAX_ACTIONS, TRAIN_ITERS, FIT_ITERS, ROUNDS),
           "training": training, "summary": summary, "against_branch_and_parent": verdict, "runs": runs}
    print(json.dumps({"summary": summary, "against_branch_and_parent": verdict}, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(out, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        if sys.argv[2] == "train":
            train(sys.argv[3])
        else:
            child(sys.argv[2], sys.argv[3], sys.argv[4])
    else:
        main(sys.argv[1:])
