"""The dW1 tail tile of the HID = 256 split backward (csrc/ppo_policy_bwd_x6.hip): the accumulator of inputs 64 .. 95, of
which inputs 64 .. 71 and the ones column at 72 (db1) are ever non-zero.  It is the one accumulator tile a register-saving
change can move out of the register file across the dH1 chain (measured: parking its nine live columns in wave-private LDS
buys a W2 ring of 6 without scratch, and the deeper ring is not faster -- DESIGN.md section 3d -- so the shipped kernel keeps it
in registers).  Whatever form the kernel takes, a wrong lane mask, a lost restore or an LDS overlap there shows in
dW1[:, 64:72] and db1 and nowhere else, so these are compared on their own against the fp32-MFMA backward
(ppo_set_bwd_split_bf16(0)) at the tolerance tests/test_gpu_split_backward.py holds the whole gradient to (4e-6 of the
gradient's largest element), and a second identical launch must agree bit for bit.  Minibatch shapes: fewer tiles than
workgroups, exactly one tile per workgroup, several per workgroup with a ragged last round, and Q = 32 states (4 tiles each).

The states come from the CPU oracle's env and enter through set_columns, so that the test can first assert on the CPU that
the chosen minibatch has non-zero features in every one of the columns 64 .. 71 (all-zero columns would hide a lost tile).
The padded columns 73 .. 95 never reach the flat gradient and are no part of this test."""
import numpy as np
import pytest

from oracle import np_oracle

pytestmark = pytest.mark.gpu

F, HID, EPS, ENT = 72, 256, 0.05, 0.01
NWG = 256                     # workgroups of the HID = 256 split backward (one per CU); a tile is 32 state rows


@pytest.fixture()
def P(ppo):
    if ppo.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests must run on the GPU box")
    ppo.set_bwd_small_max_tiles(0)            # the fused backward at every minibatch size
    ppo.set_train_tile_max_tiles(0)
    yield ppo
    ppo.set_bwd_small_max_tiles(None)
    ppo.set_train_tile_max_tiles(None)
    ppo.set_bwd_split_bf16(None)


def _off_the_kink(params, states, delta=2e-6):
    """True per state when no hidden unit's pre-activation lies within `delta` of leakyrelu's kink, where two precisions can
    disagree about the derivative (see tests/test_gpu_split_backward.py)."""
    n, H = states.shape[:2]
    a = states.reshape(-1, F).astype(np.float64).T
    ok = np.ones(n, bool)
    for (W, b) in np_oracle.unpack_params(params, F, HID, 2)[:-1]:
        z = W.astype(np.float64) @ a + b.astype(np.float64)[:, None]
        ok &= np.abs(z).min(axis=0).reshape(n, H).min(axis=1) >= delta
        a = np.where(z > 0, z, 0.01 * z)
    return ok


# (quads, envs, steps, minibatch states): tiles = states * quads / 8
CASES = [
    (8, 48, 24, 100),       # fewer tiles than workgroups: 156 workgroups write an all-zero tile
    (8, 48, 24, 256),       # exactly one tile per workgroup
    (8, 48, 24, 600),       # two full rounds and a ragged third (88 of 256 workgroups)
    (32, 32, 8, 150),       # 4 tiles per state: 600 tiles, ragged as above
]


@pytest.mark.parametrize("Q,N,T,B", CASES, ids=["Q%d-%dstates" % (c[0], c[3]) for c in CASES])
def test_dw1_tail_columns_and_db1(P, orc, Q, N, T, B):
    H = 4 * Q
    tiles = B * H // 32
    assert (tiles < NWG) == (B == 100) and (tiles == NWG) == (B == 256) and (tiles <= NWG or tiles % NWG != 0)
    pol = P.HipPolicy(F, HID, 2, 4, seed=B + 1)
    rng = np.random.default_rng(1000 * Q + B)
    pol.params = pol.params + (rng.normal(size=pol.num_params) * 0.02).astype(np.float32)
    # a rollout of the oracle's env under this policy, on the CPU
    oenv = orc.Env(Q=Q, max_actions=12, N=N, seed=B)
    oenv.reset()
    ref = orc.collect_rollouts_tn(oenv, pol.params, HID, T, mode_dev=True)
    returns = orc.compute_returns_tn(ref["rewards"], ref["done"], 1.0)
    states = ref["states"].reshape(-1, H, F)
    pool = np.flatnonzero(_off_the_kink(pol.params, states))
    assert len(pool) >= 64
    sel0 = pool[rng.choice(len(pool), size=B, replace=B > len(pool))]
    # the chosen states exercise the tail tile: every column 64 .. 71 is non-zero somewhere, and most tiles carry some
    tail = states[sel0].reshape(-1, 32, F)[:, :, 64:72]
    assert (tail != 0).any(axis=(0, 1)).all(), "a feature column of 64 .. 71 is zero in the whole minibatch"
    assert (tail != 0).any(axis=(1, 2)).mean() >= 0.5, "most tiles have nothing in columns 64 .. 71"

    ro = P.BufferRollouts()
    ro.set_columns(None, ref["states"], ref["active"], ref["actions"].astype(np.int64) + 1, ref["p_sel"], returns)
    ds = P.construct_dataset(ro)
    out = {}
    for mode in (0, 1):
        P.set_bwd_split_bf16(mode)
        P.forward_backward(pol, ds, sel0 + 1, EPS, ENT)
        out[mode] = pol.grad().copy()
        if mode == 1:
            P.forward_backward(pol, ds, sel0 + 1, EPS, ENT)
            assert np.array_equal(out[1], pol.grad()), "two identical launches differ"
    scale = np.abs(out[0]).max()
    (W0, b0), (W1, b1) = (np_oracle.unpack_params(out[m], F, HID, 2)[0] for m in (0, 1))
    assert W0.shape == (HID, F) and np.abs(W0[:, 64:72]).max() > 0 and np.abs(b0).max() > 0
    d_w = np.abs(W1[:, 64:72] - W0[:, 64:72]).max() / scale
    d_b = np.abs(b1 - b0).max() / scale
    d_rest = np.abs(W1[:, :64] - W0[:, :64]).max() / scale
    print("Q %d B %d tiles %d: dW1[:,64:72] %.3g  db1 %.3g  (dW1[:,:64] %.3g) of max|g|" % (Q, B, tiles, d_w, d_b, d_rest))
    assert d_w <= 4e-6 and d_b <= 4e-6, (d_w, d_b)
