#!/usr/bin/env python3
"""Seeded training runs at the headline shape whose results two builds of this repository must reproduce bit for bit
(4096 envs, Q = 8, Policy(72,256,2,4) and a critic of that shape, minibatch 4096, 4 epochs):
  a_*: ppo_iterate_ with a critic, 4096 episodes per iteration, 3 iterations;
  b_*: the steps-mode loop of tools/value_timing.py (128 steps x 4096 envs, GAE from the critic, ppo_train_ and value_train_
       with a seeded device permutation), 2 iterations.
Each leaves the policy's and the critic's parameters and every loss / learning-rate history in OUT.npz.
Usage: tools/seeded_train_run.py OUT.npz                  (run with the tree this file lies in; needs a GPU)
       tools/seeded_train_run.py --compare A.npz B.npz    (no GPU: one line per array, exit status 1 unless all are equal)"""
import os, sys
import numpy as np

if sys.argv[1] == "--compare":
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    assert sorted(a.files) == sorted(b.files), (a.files, b.files)
    same = {k: a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in a.files}
    for k in a.files:
        print("%-12s %-8s %-10s %s" % (k, a[k].dtype, a[k].shape, "bit-identical" if same[k] else "DIFFERENT"))
    sys.exit(0 if all(same.values()) else 1)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ppo_amd as PPO

OUT = os.path.abspath(sys.argv[1])
N, T, EPOCHS, MB, HID = 4096, 128, 4, 4096, 256


class Evaluator:
    def __call__(self, policy, env, optimizer):
        pass


PPO.save_loss.register(Evaluator)(lambda ev, loss: None)


def fresh():
    return (PPO.HipVecEnv(num_envs=N, Q=8, max_actions=32, seed=7), PPO.HipPolicy(72, HID, 2, 4, seed=0),
            PPO.Optimiser(PPO.Adam(3e-4)), PPO.HipCritic(72, HID, 2, seed=1), PPO.Optimiser(PPO.Adam(1e-3)))


out = {}
env, pol, opt, critic, copt = fresh()
loss = PPO.ppo_iterate_(pol, env, opt, N, MB, 3, Evaluator(), EPOCHS, 0.99, 0.05, 0.01, verbose=False, critic=critic,
                        critic_optimizer=copt, gae_lambda=0.95)
for k, v in loss.items():
    out["a_" + k] = np.asarray(v, np.float64)
out["a_pol"], out["a_critic"] = pol.params, critic.params

env, pol, opt, critic, copt = fresh()
hist = {k: [] for k in ("ppo", "entropy", "lr", "value", "value_lr")}
for it in (1, 2):
    ro = PPO.BufferRollouts()
    PPO.collect_rollouts_steps_(ro, env, pol, T, 1.0)
    ds = PPO.construct_dataset(ro)
    PPO.compute_gae_critic_(ro, env, critic, 0.99, 0.95, fetch=False)
    p, e, lr = PPO.ppo_train_(pol, opt, ds, 0.05, MB, EPOCHS, 0.01, seed=it, verbose=False, advantage="gae")
    v, vl = PPO.value_train_(critic, copt, ds, MB, EPOCHS, target="lambda_returns", seed=it, verbose=False)
    for k, x in zip(("ppo", "entropy", "lr", "value", "value_lr"), (p, e, lr, v, vl)):
        hist[k] += x
for k, v in hist.items():
    out["b_" + k] = np.asarray(v, np.float64)
out["b_pol"], out["b_critic"] = pol.params, critic.params
PPO.synchronize()
os.makedirs(os.path.dirname(OUT), exist_ok=True)
np.savez(OUT, **out)
print("seeded run ->", OUT)
