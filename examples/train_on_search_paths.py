#!/usr/bin/env python3
"""Usage example: a self-imitation (expert-iteration) loop without a host trip -- search, collect the winners' paths, train.

    starts = reset states of a fresh env
    found  = PPO.search_best_states_(search_env, policy, *starts, K, path=True)      # best of K trajectories per start
    PPO.collect_paths_(rollouts, env, policy, *starts, found["path"], discount)      # the paths as an ordinary rollout buffer
    PPO.imitate_train_(policy, optimizer, PPO.construct_dataset(rollouts), minibatch, epochs, entropy_weight)   # --loss clone

collect_paths_ replays every path on the device and leaves the state in front of each step, the path's action, the
probability the CURRENT policy gives that action, reward, terminal flags and returns in the buffer, so every consumer of a
sampled buffer takes it unchanged.

The data is OFF-POLICY.  The actions were chosen by another sampler -- the best of K draws of the policy, not one draw -- and
p_old is the current policy's probability of that sampler's action, not the probability the action was sampled with.
--loss chooses what is minimised on it:
    clone (default)  imitate_train_, uniform weights: the cross-entropy -mean log pi(a | s) of the paths' actions (behaviour
                     cloning, as in expert iteration); p_old is not read
    sil              imitate_train_(weights="positive_advantage"): -mean(max(adv, 0) log pi(a | s)) (self-imitation); adv is
                     the buffer's returns, or with --critic GAE at lambda = 1 (R - V), bootstrapped where a path was cut
    ppo              ppo_train_: the ratio p_new / p_old starts at 1 and the clipped surrogate limits how far one call moves
                     the policy towards the searched actions; it is not the importance weight PPO's derivation assumes
A path that ends short of the optimum is a truncation (terminal flag set on its last entry): with --critic the advantage is
GAE bootstrapped from the critic's value of the state the path was cut in (compute_gae_critic_(..., bootstrap_truncated=True);
lambda 0.95 for --loss ppo, 1 for --loss sil).

--temperature sets the policy's selection for the SEARCH step alone (with PPO.selecting(policy, "sample", tau): ...): the K
clones of a start sample from softmax(logits / tau), so a temperature above 1 keeps them apart once training has sharpened the
policy, and one below 1 focuses an untrained one.  collect_paths_ and the training calls never read the selection: p_old and
the loss stay those of the untempered policy.  Each round also scores the policy's mode, the greedy roll-out
(selecting(policy, "greedy")), next to the sampled return.

--top-k / --top-p truncate what the search's clones sample from (HipPolicy.truncation, through selecting(..., top_k=, top_p=)):
the k likeliest actions, or the likeliest set that reaches probability mass top_p, renormalised.  With a temperature above 1
that keeps the clones apart without moving probability onto the long tail of moves the policy has learnt to be useless.  Like
the temperature it is the search step's alone.

--search beam replaces the best-of-K search by beam_search_states_: the result comes from the K = --clones action
sequences the policy finds likeliest, so the paths depend on the policy and the start alone, not on Philox ticks or on the
resident env a start landed in; --temperature, --top-k and --top-p are then not read.  --distinct children|parents makes it
the distinct beam: K different states per step instead of K spellings of a few, so that the round's paths differ;
--beam-rounds is its budget, 256 candidates examined per step and round (--rounds is taken: the training rounds).

--anchor COEF adds the step this loop ends in: fine-tuning the cloned policy with PPO on its OWN sampled rollouts without losing
it.  Behind the rounds a frozen copy of the policy becomes the anchor; every PPO iteration collects with the current policy,
fill_targets_(rollouts, frozen) leaves the frozen copy's distribution of every visited state in the buffer, and ppo_train_
minimises the PPO loss plus COEF * KL(frozen || policy) (policy.kl_anchor = (COEF, "column", --anchor-target)).
With --anchor-target d > 0 the coefficient doubles behind an epoch whose mean anchor KL exceeds 1.5 d and halves below d / 1.5.
COEF = 0 records the divergence of plain PPO from the cloned policy.

This script shows the calls and prints what it measures each round (the mean gap the search reaches, the transitions
collected, the losses, the mean return of the plain stochastic policy).  Whether the loop learns faster or better than
ppo_iterate_ on sampled rollouts, and which --loss serves it best, has not been measured; the script makes no such claim.
Run on the GPU box:  python examples/train_on_search_paths.py --rounds 10
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ppo_amd as PPO  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--starts", type=int, default=256, help="start states per round (one resident env replays one path)")
    ap.add_argument("--clones", type=int, default=16, help="K: trajectories the search plays from every start")
    ap.add_argument("--search", choices=("best_of_k", "beam"), default="best_of_k",
                    help="best_of_k: the best of K sampled trajectories; beam: the K likeliest action sequences (K <= %d)" % PPO.BEAM_MAX_K)
    ap.add_argument("--distinct", choices=("children", "parents"), default=None,
                    help="--search beam: keep K different states per step; parents: also different from the step's parents")
    ap.add_argument("--beam-rounds", type=int, default=4,
                    help="--distinct: windows of 256 candidates a step may examine (1 .. %d)" % PPO.BEAM_MAX_ROUNDS)
    ap.add_argument("--critic", action="store_true", help="GAE advantage from a device critic, bootstrapped where a path was cut")
    ap.add_argument("--loss", choices=("ppo", "clone", "sil"), default="clone",
                    help="clone: cross-entropy on the paths' actions; sil: weighted by max(advantage, 0); ppo: the clipped surrogate")
    ap.add_argument("--temperature", type=float, default=1.0,
                    help="selection temperature of the search step (1: the policy's own distribution; > 1 flatter, < 1 sharper)")
    ap.add_argument("--top-k", type=int, default=0, help="the search step samples from the k likeliest actions only (0: all)")
    ap.add_argument("--top-p", type=float, default=1.0,
                    help="the search step samples from the likeliest actions that reach this probability mass only (1: all)")
    ap.add_argument("--anchor", type=float, default=None, metavar="COEF",
                    help="behind the rounds: PPO on sampled rollouts with the penalty COEF * KL(frozen cloned policy || policy)")
    ap.add_argument("--anchor-target", type=float, default=0.0, help="--anchor: adapt COEF towards this mean KL (0: fixed)")
    ap.add_argument("--ppo-iterations", type=int, default=5, help="--anchor: PPO iterations behind the rounds")
    args = ap.parse_args()

    discount, epsilon, entropy_weight, max_actions = 1.0, 0.05, 0.01, 32
    policy = PPO.HipPolicy(72, 128, 2, 4, seed=0)
    optimizer = PPO.Optimiser(PPO.Adam(3e-4))
    critic = PPO.HipCritic(72, 128, 2, seed=1) if args.critic else None
    critic_optimizer = PPO.Optimiser(PPO.Adam(1e-3)) if args.critic else None
    search_env = PPO.HipVecEnv(num_envs=args.starts * args.clones, Q=8, max_actions=max_actions, seed=7)
    env = PPO.HipVecEnv(num_envs=args.starts, Q=8, max_actions=max_actions, seed=8)
    eval_env = PPO.HipVecEnv(num_envs=1024, Q=8, max_actions=max_actions, seed=99)
    rollouts = PPO.BufferRollouts()

    for r in range(args.rounds):
        fresh = PPO.HipVecEnv(num_envs=args.starts, Q=8, max_actions=max_actions, seed=1000 + r)   # this round's reset states
        st = fresh.internal()
        starts = (st["score"], st["degree"], fresh.active_quads())
        if args.search == "beam":                             # deterministic: the selection and the truncation are not read
            found = PPO.beam_search_states_distinct_(search_env, policy, *starts, args.clones, path=True,
                                                     distinct=args.distinct, rounds=args.beam_rounds)
        else:
            with PPO.selecting(policy, "sample", args.temperature, top_k=args.top_k, top_p=args.top_p):   # the search alone; restored behind it
                found = PPO.search_best_states_(search_env, policy, *starts, args.clones, path=True)
        PPO.collect_paths_(rollouts, env, policy, *starts, found["path"], discount)
        dataset = PPO.construct_dataset(rollouts)
        n = len(dataset)
        if n == 0:                                            # every start was its own best state: nothing to imitate
            print("round %d: the search improved no start" % r)
            continue
        advantage = "returns"
        if critic is not None:
            PPO.compute_gae_critic_(rollouts, env, critic, discount, 1.0 if args.loss == "sil" else 0.95, fetch=False,
                                    bootstrap_truncated=True)
            advantage = "gae"
        if args.loss == "ppo":
            ph, eh, _ = PPO.ppo_train_(policy, optimizer, dataset, epsilon, min(1024, n), 2, entropy_weight, seed=r, verbose=False,
                                       advantage=advantage)
        else:
            ph, eh, _ = PPO.imitate_train_(policy, optimizer, dataset, min(1024, n), 2, entropy_weight, seed=r, verbose=False,
                                           weights="uniform" if args.loss == "clone" else "positive_advantage", advantage=advantage)
        line = "round %d: gap %.2f -> %.2f over %d starts, %d transitions, %s loss %.4f, entropy loss %.4f" % (
            r, found["initial_gap"].mean(), found["best_gap"].mean(), args.starts, n, args.loss, ph[-1], eh[-1])
        if critic is not None:
            vh, _ = PPO.value_train_(critic, critic_optimizer, dataset, min(1024, n), 2, target="lambda_returns", seed=r, verbose=False)
            line += ", value loss %.4f, %d cut paths" % (vh[-1], rollouts.n_truncated)
        ret, dev = PPO.average_returns(policy, eval_env, 1024)
        with PPO.selecting(policy, "greedy"):
            gret, _ = PPO.average_returns(policy, eval_env, 1024)
        print(line + "; stochastic policy: mean return %.3f (std %.3f), greedy %.3f" % (ret, dev, gret))
    if args.anchor is not None:
        frozen = PPO.HipPolicy(72, 128, 2, 4, seed=0)
        frozen.params = policy.params                         # the cloned policy, from here on the anchor
        policy.kl_anchor = (args.anchor, "column", args.anchor_target)
        sampled = PPO.BufferRollouts()
        for it in range(args.ppo_iterations):
            PPO.collect_rollouts_steps_(sampled, env, policy, max_actions, discount)
            PPO.fill_targets_(sampled, frozen)                # the anchor's distribution of every visited state, on the device
            dataset = PPO.construct_dataset(sampled)
            ph, eh, _ = PPO.ppo_train_(policy, optimizer, dataset, epsilon, min(1024, len(dataset)), 2, entropy_weight, seed=it,
                                       verbose=False)
            stats = policy.last_anchor_stats()
            ret, dev = PPO.average_returns(policy, eval_env, 1024)
            print("anchored PPO %d: loss %.4f (surrogate + coef * cross-entropy), anchor KL %s at coef %s, next coef %.4g; "
                  "mean return %.3f (std %.3f)" % (it, ph[-1], ["%.5f" % k for k in stats["anchor_kl"]],
                                                   ["%.4g" % c for c in stats["anchor_coef"]], policy.kl_anchor[0], ret, dev))
    return policy


if __name__ == "__main__":
    main()
