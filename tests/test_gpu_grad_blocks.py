"""Every gradient block of the training pass against a bar set by the block's own fp32 floor (tests/grad_blocks_ref.py).

The bar of the other fp32 gradient tests, max|g - g64| <= 2e-5 max|g64| over the whole flat gradient, cannot see an error in
a block that is small next to the largest one, and on peaked policies it lies below what plain fp32 arithmetic delivers.
Here, per block (W1, b1, ..., W_L, b_L, the output layer) and per 32-unit feature tile of every W:

    || g[block] - g64[block] ||_2 <= M floor(block),    floor(block) = || grad32[block] - grad64[block] ||_2,   M = 4
    || g[tile] - g64[tile] ||_2   <= M max(floor(tile), floor(block) sqrt(n_tile / n_block))

with grad32 / grad64 the same loss differentiated by torch in float32 / float64: the bar comes from the reference alone and
scales with the conditioning of the minibatch.  The cases: one per train-forward family of advantage_modes_ref.FAMILIES at
the state counts that table names, the route asserted by kernel name; the three-product and the fused fp32-MFMA backward at 37
and 385 states; one and four hidden layers; a padded width; reference-trained (peaked) weights on two rollouts each and a
near-init policy with its output layer multiplied by 8.  tests/test_grad_blocks_host.py shows on the CPU what the cases rest
on.  The bf16 families are recorded per block against the restated bf16 arithmetic and held to the bars they already have:
their noise is flipped bf16 roundings, for which the fp32 floor is no model.

TEST_RECORD_DIR=<dir>: every case appends one line to <dir>/grad_blocks.jsonl: case, route, per-block err / floor, worst tile,
old metric (profiles/grad_blocks_test_record.jsonl is such a file)."""
import json
import os

import numpy as np
import pytest

import grad_blocks_ref as gb
from oracle import np_oracle
from test_train_route import route

pytestmark = pytest.mark.gpu
am = gb.am
LOSS_BAR = 1e-5                                 # the loss bar of every fp32 gradient test here
BF16_BAR, BF16_L2, BF16_LOSS = 1e-2, 3e-3, 2e-3   # tests/test_gpu_bf16.py: per element, in the 2-norm, on the losses


@pytest.fixture(scope="module")
def P(ppo):
    if ppo.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests must run on the GPU box")
    return ppo


@pytest.fixture()
def knobs(P):
    yield P
    P.set_bwd_split_bf16(None)
    P.set_rollout_compact(None)
    P.set_train_tile_max_tiles(None)
    P.set_bwd_small_max_tiles(None)


def _record(rec):
    print(json.dumps(rec))
    d = os.environ.get("TEST_RECORD_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "grad_blocks.jsonl"), "a") as f:
            f.write(json.dumps(rec) + "\n")


def _setup(P, name):
    """Set the case's knobs and assert its route by kernel name -> (forward kernel, backward kernel)."""
    sh = gb.shape_of(name)
    if name in am.FAMILIES:
        c = am.FAMILIES[name]
        if "split" in c["setup"]:
            P.set_bwd_split_bf16(c["setup"]["split"])
        if "compact" in c["setup"]:
            P.set_rollout_compact(True)
        if "tile" in c["setup"]:
            P.set_train_tile_max_tiles(c["setup"]["tile"])
        got = route(P, c["dtype"], c["F"], c["hid"], c["L"], 4 * c["Q"], c["compact"], c["B"])
        if c["fwd"] is None:                               # the split-fp32 forward from compact storage, named by the library
            assert got[0].startswith("k_policy_fwd_train_x6") and got[1] == "k_policy_bwd_x6<72,256>", got
        else:
            assert got[0] == c["fwd"], (name, got)
    else:
        c = gb.EXTRA[name]
        if "split" in c["knobs"]:
            P.set_bwd_split_bf16(c["knobs"]["split"])
        if "small" in c["knobs"]:
            P.set_bwd_small_max_tiles(c["knobs"]["small"])
        got = route(P, "f32", 72, sh["HID"], c["L"], 32, False, c["B"])
        assert got == c["route"], (name, got)
    return sh, got


def _policy(P, sh, params):
    pol = P.HipPolicy(sh["F"], sh["hid"], sh["L"], 4, dtype=sh["dtype"])
    pol.params = params
    return pol


def _dataset(P, name, d, sh):
    """(policy with the case's parameters, dataset whose positions are the case's storage order)."""
    if name in am.FAMILIES and am.FAMILIES[name]["compact"]:
        # compact storage exists for engine rollouts only: collect the one the oracle collected, and show that it is
        r = am.ROLLOUT
        env = P.HipVecEnv(num_envs=r["N"], Q=r["Q"], max_actions=r["max_actions"], seed=r["env_seed"])
        pol = _policy(P, sh, d["collect_params"])
        ro = P.BufferRollouts()
        P.collect_rollouts_steps_(ro, env, pol, r["T"], r["discount"])
        n = r["N"] * r["T"]
        st, act = ro.state_data
        assert np.array_equal(st.reshape(n, 32, 72), d["states"]) and np.array_equal(act.reshape(n), d["active"])
        assert np.array_equal(ro.selected_actions.reshape(n) - 1, d["a0"])
        assert np.array_equal(ro.selected_action_probabilities.reshape(n), d["p_old"])
        assert np.array_equal(ro.rewards.reshape(n), d["R"])
        pol.params = d["params"]
        return pol, P.construct_dataset(ro)
    T, N = d["T"], d["N"]
    H, F = d["states"].shape[1:]
    ro = P.BufferRollouts()
    ro.set_columns(None, d["states"].reshape(T, N, H, F), d["active"].reshape(T, N), d["a0"].reshape(T, N).astype(np.int64) + 1,
                   d["p_old"].reshape(T, N), d["R"].reshape(T, N))
    return _policy(P, sh, d["params"]), P.construct_dataset(ro)


@pytest.mark.parametrize("name", gb.F32_CASES)
def test_every_block_within_its_fp32_floor(P, orc, knobs, name):
    sh, got = _setup(P, name)
    d = gb.case(name, orc)
    assert d["kept"] >= 0.5
    pol, ds = _dataset(P, name, d, sh)
    lp, le = P.forward_backward(pol, ds, d["sel0"] + 1, gb.EPS, gb.ENT)
    g = pol.grad()
    ref = gb.reference(sh, d["params"], gb.minibatch(d))
    assert g.shape == ref["g64"].shape
    mult, worst, old = gb.multiples(g, ref["g64"], ref["fb"], ref["ft"], ref["blocks"], ref["tiles"])
    el = max(abs(lp - ref["lp"]) / (1 + abs(ref["lp"])), abs(le - ref["le"]) / (1 + abs(ref["le"])))
    rec = dict(case=name, fwd=got[0], bwd=got[1], B=len(d["sel0"]), err_over_floor={k: round(v, 3) for k, v in mult.items()},
               worst_tile=[worst[0], round(worst[1], 3)], old_metric=old,
               old_metric_fp32=float(np.abs(ref["g32"] - ref["g64"]).max() / np.abs(ref["g64"]).max()), loss_err_over_bar=el / LOSS_BAR)
    _record(rec)
    assert el <= LOSS_BAR, rec
    assert max(mult.values()) <= gb.M, rec
    assert worst[1] <= gb.M, rec


@pytest.mark.parametrize("name", gb.BF16_FAMILIES)
def test_bf16_families_recorded_per_block(P, orc, knobs, name):
    sh, got = _setup(P, name)
    d = gb.case(name, orc)
    pol, ds = _dataset(P, name, d, sh)
    lp, le = P.forward_backward(pol, ds, d["sel0"] + 1, gb.EPS, gb.ENT)
    g = pol.grad()
    mb = gb.minibatch(d)
    g16, olp, ole = np_oracle.step_batch_grad_chunked(np_oracle.step_batch_grad_bf16, d["params"], sh["F"], sh["hid"], mb["states"],
                                                      np_oracle.batch_masks(mb["active"], sh["Q"]), mb["a0"], mb["p_old"], mb["adv"],
                                                      gb.EPS, gb.ENT, chunk=512)
    bl = gb.blocks(sh["F"], sh["hid"], sh["HID"], sh["L"])
    rel = {k: float(np.linalg.norm(g[s] - g16[s]) / np.linalg.norm(g16[s])) for k, s in bl.items()}
    err = float(np.abs(g - g16).max() / np.abs(g16).max())
    l2 = float(np.linalg.norm(g - g16) / np.linalg.norm(g16))
    el = max(abs(lp - olp) / (1 + abs(olp)), abs(le - ole) / (1 + abs(ole)))
    rec = dict(case=name, fwd=got[0], bwd=got[1], B=len(d["sel0"]), rel_l2_vs_bf16_restatement=rel, err_over_max=err, l2=l2,
               loss_err=el)
    _record(rec)
    assert err <= BF16_BAR and l2 <= BF16_L2 and el <= BF16_LOSS, rec          # the bars these families already have
