#!/usr/bin/env python3
"""Per-step device cost of ClipNorm in an optimiser chain (GPU box).

Runs ppo_train epochs at the benchmark's step (one 4096-state minibatch, HID = 256) under `rocprofv3 --kernel-trace
--stats`, once with Optimiser(Adam(3e-4), ExpDecay(1.0, 0.5, 1000, 1e-6)) and once with ClipNorm(0.5) in front of the
same chain, each in a fresh child process, and compares the optimiser launches:
  without ClipNorm: k_grad_reduce<ChainFuse>            (slab reduction + chain, one launch)
  with ClipNorm:    k_grad_reduce<ClipFuse> + k_clip_apply  (phase 1 + phase 2)

  python3 tools/clip_step_timing.py OUTDIR [--epochs N]      -> OUTDIR/{base,clip}/..., OUTDIR/summary.json
  python3 tools/clip_step_timing.py --run base|clip [--epochs N]   (the workload itself)"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, HID, F = 4096, 256, 72


def workload(which, epochs):
    sys.path.insert(0, ROOT)
    import numpy as np
    import ppo_amd as P
    rng = np.random.default_rng(0)
    pol = P.HipPolicy(F, HID, 2, 4, seed=3)
    states = rng.integers(-3, 7, size=(B, 32, F)).astype(np.int8)
    active = rng.integers(1, 2 ** 8, size=B, dtype=np.uint64).astype(np.uint32)
    probs = P.batch_action_probabilities(pol, P.StateData(states, active)).T.astype(np.float64)
    cdf = np.cumsum(probs, axis=1)
    a0 = (cdf < (rng.random(B) * cdf[:, -1])[:, None]).sum(axis=1)
    p_old = (probs[np.arange(B), a0] * rng.uniform(0.8, 1.25, B)).astype(np.float32)
    adv = (rng.normal(size=B) * 3).astype(np.float32)
    ro = P.BufferRollouts()
    ro.set_columns(None, states[None], active[None], a0[None].astype(np.int64) + 1, p_old[None], adv[None])
    ds = P.construct_dataset(ro)
    members = [P.Adam(3e-4), P.ExpDecay(1.0, 0.5, 1000, 1e-6)]
    if which == "clip":
        members.insert(0, P.ClipNorm(0.5))
    opt = P.Optimiser(*members)
    P.ppo_train_(pol, opt, ds, 0.05, B, epochs, 0.01, seed=1, verbose=False)
    P.synchronize()


def stats(d):
    f = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not f:
        raise SystemExit("no kernel_stats.csv under " + d)
    with open(f[0]) as fh:
        return {r["Name"]: (int(r["Calls"]), float(r["AverageNs"])) for r in csv.DictReader(fh)}


def pick(st, key):
    hits = [(n, v) for n, v in st.items() if key in n]
    return hits[0] if hits else (None, (0, 0.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--run", choices=["base", "clip"])
    ap.add_argument("--epochs", type=int, default=200)
    a = ap.parse_args()
    if a.run:
        return workload(a.run, a.epochs)
    res = {}
    for which in ("base", "clip"):
        d = os.path.join(a.out, which)
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
               sys.executable, os.path.abspath(__file__), "--run", which, "--epochs", str(a.epochs)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        with open(os.path.join(a.out, which + ".log"), "w") as fh:
            fh.write(r.stdout)
        if r.returncode != 0:
            print(r.stdout[-3000:])
            raise SystemExit("%s: exit %d" % (which, r.returncode))
        res[which] = stats(d)
    base = pick(res["base"], "k_grad_reduce<ChainFuse>")
    ph1, ph2 = pick(res["clip"], "k_grad_reduce<ClipFuse>"), pick(res["clip"], "k_clip_apply")
    out = {
        "shape": {"states_per_step": B, "HID": HID, "F": F, "epochs": a.epochs},
        "base_chain": "Optimiser(Adam(3e-4), ExpDecay(1.0, 0.5, 1000, 1e-6))",
        "clip_chain": "Optimiser(ClipNorm(0.5), Adam(3e-4), ExpDecay(1.0, 0.5, 1000, 1e-6))",
        "k_reduce_chain_us": base[1][1] / 1e3, "k_reduce_chain_calls": base[1][0],
        "k_reduce_clip_us": ph1[1][1] / 1e3, "k_reduce_clip_calls": ph1[1][0],
        "k_clip_apply_us": ph2[1][1] / 1e3, "k_clip_apply_calls": ph2[1][0],
        "clip_cost_per_step_us": (ph1[1][1] + ph2[1][1] - base[1][1]) / 1e3,
        "kernels": {w: {n: {"calls": c, "avg_us": v / 1e3} for n, (c, v) in res[w].items()} for w in res},
    }
    with open(os.path.join(a.out, "summary.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "kernels"}, indent=1))


if __name__ == "__main__":
    main()
