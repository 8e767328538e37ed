#!/usr/bin/env python3
"""How often a greedy step changes the state on the device ("Greedy has fixed points"): best_states_(actions=True)
under ("greedy", 1) and, for comparison, ("sample", 1); 24 envs, Q = 8, max_actions 20, env seed 13, one trajectory per env; the
device's actions replayed on the oracle env (tests/select_ref.py state_changes).  Two policies: glorot_params(72,256,2,seed=3)
and tests/golden/poly-30-policy.  A record.  Writes profiles/select_greedy_moves.json, or the file named first.
Usage: tools/select_greedy_moves.py [out.json]"""
import json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import ppo_amd as P
from oracle import oracle as orc
import episodes_ref as ref, select_ref as S
out = {}
for name, params, hid in (("glorot_72_256_2_seed3", orc.glorot_params(72, 256, 2, seed=3), 256),
                          ("poly-30-policy", np.load(os.path.join(ROOT, "tests", "golden", "poly-30-policy.npz"))["params"], 128)):
    case = dict(S.GREEDY_COVERAGE, hid=hid)
    pol = P.HipPolicy(72, hid, 2, 4, seed=0); pol.params = params
    for sel in (("greedy", 1.0), ("sample", 1.0)):
        pol.selection = sel
        env = P.HipVecEnv(**ref.env_kw_of(case))
        got = P.best_states_(env, pol, 24, actions=True)
        acts = (got["actions"].astype(np.int32) - 1).T          # [T, N], one trajectory per env
        cols = dict(actions=acts)
        changed, total = S.state_changes(orc, case, cols)
        distinct = len(set(int(a) for a in acts[acts >= 0]))
        out["%s %s" % (name, sel[0])] = dict(changed=changed, steps=total, distinct_actions=distinct, mean_best_gap=float(got["best_gap"].mean()),
                                           mean_initial_gap=float(got["initial_gap"].mean()), improved=int((got["best_step"] > 0).sum()))
        print(name, sel, out["%s %s" % (name, sel[0])], flush=True)
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "select_greedy_moves.json")
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(out, open(OUT, "w"), indent=1)
