#!/usr/bin/env python3
"""Usage example: policy distillation without a host trip -- move what a wide policy learned into a narrow one.

    teacher = a trained Policy(72,256,2,4) (--teacher file saved by PPO.save_policy), or one trained here for --iterations
    PPO.collect_rollouts_steps_(rollouts, env, teacher, T, discount)         # the teacher's own state distribution
    PPO.fill_targets_(rollouts, teacher)                                     # its whole action distribution per stored state
    PPO.distill_train_(student, optimizer, PPO.construct_dataset(rollouts), minibatch, epochs)   # soft-target cross-entropy

The student, Policy(72,128,2,4), sees every action's probability in every state, not one sampled action per state as behaviour
cloning (imitate_train_) would.  The loss distill_train_ reports is the cross-entropy; its floor is the targets' entropy, so
the script also prints the mean KL(teacher || student) and how often both pick the same arg-max action, on a HELD-OUT
collection (other envs, collected by the teacher after training the student never saw), before and after.

This script shows the calls and prints what it measures.  How many transitions and epochs a student of a given width needs,
and how its returns compare with the teacher's, has not been measured; the script makes no such claim.
Run on the GPU box:  python examples/distill_policy.py --iterations 3
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ppo_amd as PPO  # noqa: E402


def agreement(teacher, student, rollouts):
    """(mean KL(teacher || student), arg-max agreement) over the states a buffer holds, on the host from the two forwards."""
    st, act = rollouts.state_data
    s = PPO.StateData(st.reshape(-1, st.shape[2], st.shape[3]), act.reshape(-1))
    pt = PPO.batch_action_probabilities(teacher, s).T.astype(np.float64)
    ps = PPO.batch_action_probabilities(student, s).T.astype(np.float64)
    keep = pt > 0
    kl = float((pt[keep] * (np.log(pt[keep]) - np.log(np.maximum(ps[keep], 1e-300)))).sum() / len(pt))
    return kl, float((pt.argmax(axis=1) == ps.argmax(axis=1)).mean())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--teacher", help="a policy file written by PPO.save_policy (default: train one here)")
    ap.add_argument("--iterations", type=int, default=3, help="PPO iterations of the teacher trained here")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=32, help="T of the collections")
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatch", type=int, default=1024)
    ap.add_argument("--student-width", type=int, default=128)
    ap.add_argument("--lr", type=float, default=1e-3)
    a = ap.parse_args()
    env = PPO.HipVecEnv(num_envs=a.envs, Q=8, max_actions=a.steps, seed=7)
    held_env = PPO.HipVecEnv(num_envs=max(64, a.envs // 8), Q=8, max_actions=a.steps, seed=1007)
    if a.teacher:
        teacher = PPO.load_policy(a.teacher)
    else:
        teacher = PPO.HipPolicy(72, 256, 2, 4, seed=0)
        opt = PPO.Optimiser(PPO.Adam(3e-4))
        ro = PPO.BufferRollouts()
        for it in range(a.iterations):
            PPO.collect_rollouts_steps_(ro, env, teacher, a.steps, 0.99)
            ph, eh, _ = PPO.ppo_train_(teacher, opt, PPO.construct_dataset(ro), 0.05, a.minibatch, 2, 0.01, seed=it, verbose=False)
            print("teacher iteration %d: ppo loss %.4f, entropy loss %.4f, mean return %.3f" % (it + 1, ph[-1], eh[-1], float(ro.rewards[0].mean())))
    student = PPO.HipPolicy(72, a.student_width, 2, 4, seed=1)
    rollouts, held_out = PPO.BufferRollouts(), PPO.BufferRollouts()
    PPO.collect_rollouts_steps_(held_out, held_env, teacher, a.steps, 0.99)
    PPO.collect_rollouts_steps_(rollouts, env, teacher, a.steps, 0.99)
    PPO.fill_targets_(rollouts, teacher)
    kl0, same0 = agreement(teacher, student, held_out)
    print("held-out, before: mean KL(teacher || student) %.5f, arg-max agreement %.3f" % (kl0, same0))
    ce, _, _ = PPO.distill_train_(student, PPO.Optimiser(PPO.Adam(a.lr)), PPO.construct_dataset(rollouts), a.minibatch, a.epochs,
                                  seed=11, verbose=False)
    q = rollouts.action_targets.astype(np.float64)
    floor = float(-(np.where(q > 0, q * np.log(np.where(q > 0, q, 1.0)), 0.0)).sum() / (q.shape[0] * q.shape[1]))
    print("cross-entropy per epoch: %s (floor, the targets' entropy: %.4f)" % (" ".join("%.4f" % c for c in ce), floor))
    kl1, same1 = agreement(teacher, student, held_out)
    print("held-out, after:  mean KL(teacher || student) %.5f, arg-max agreement %.3f" % (kl1, same1))


if __name__ == "__main__":
    main()
