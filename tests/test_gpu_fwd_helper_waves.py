"""The two-tile split train forward (k_policy_fwd_train_x6t) with its helper waves.

Two extra waves per workgroup (helper i serves tile i of every pass) load, convert and pack the state rows of the NEXT pass
into an LDS image the compute waves read at the top of layer 1, and run the loss tail of the pass behind barrier (2) while the
compute waves are already in the next pass's layer 1.  What can go wrong is a hand-over: an image, a transition id or a tail
input of the wrong pass or tile, a tail that reads partial logits the next pass has overwritten, a tail lost or doubled in a
last pass that has one real tile.  The sizes put those cases on few workgroups (G = the grid cap: 256 at HID = 256, 512 at 128):

    B = 2        one pass, one workgroup: the prologue image, one tail per helper
    B = 3        odd: the last pass has one real tile and one discarded
    B = 5        several workgroups, one of them partial
    B = 4 G + 1  workgroups with three passes beside workgroups with two, the uneven last pass

HID = 128 runs the same kernel without helper waves (they measured level there): its rows and tails stay on the compute waves,
and the same hand-overs across passes are checked.  set_fwd_split_t2_min_tiles(hid, 2) forces the two-tile form at these sizes.  Per case: every state's dY rows and loss terms
are bit-identical under a permutation of the minibatch; forward_backward repeats bitwise; the gradient is within 2e-5 max|g|
of the float64 autograd gradient and the losses within 1e-5; and the gradient is within 4e-6 max|g| of the fp32-MFMA pass --
the bars of tests/test_gpu_split_backward.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import np_oracle

pytestmark = pytest.mark.gpu

F, EPS, ENT = 72, 0.05, 0.01
GRID_CAP = {256: 256, 128: 512}
CASES = [(256, 2, False), (256, 3, False), (256, 3, True), (256, 5, False), (256, 4 * 256 + 1, False), (256, 4 * 256 + 1, True),
         (128, 3, False), (128, 3, True), (128, 4 * 512 + 1, False), (128, 4 * 512 + 1, True)]


@pytest.fixture()
def P(ppo):
    if ppo.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests must run on the GPU box")
    ppo.set_bwd_small_max_tiles(0)            # the fused backward at every minibatch size
    ppo.set_train_tile_max_tiles(0)
    ppo.set_fwd_split_t2_min_tiles(256, 2)    # two tiles per pass from the smallest minibatch that has two
    ppo.set_fwd_split_t2_min_tiles(128, 2)

    def restore():
        ppo.set_bwd_small_max_tiles(None)
        ppo.set_train_tile_max_tiles(None)
        ppo.set_bwd_split_bf16(None)
        ppo.set_rollout_compact(None)
        ppo.set_fwd_split_t2_min_tiles(256, None)
        ppo.set_fwd_split_t2_min_tiles(128, None)

    try:
        yield ppo
    finally:
        restore()


def _route(P, hid, compact, states):
    fn = P._lib.lib().ppo_debug_train_route
    fn.argtypes = [C.c_int32] * 6 + [C.c_int64, C.c_char_p, C.c_char_p, C.c_int64]
    fn.restype = C.c_int32
    fwd, bwd = C.create_string_buffer(128), C.create_string_buffer(128)
    assert fn(0, F, hid, 2, 32, int(compact), states, fwd, bwd, 128) == 0
    return fwd.value.decode(), bwd.value.decode()


def _off_the_kink(params, hid, states, delta=2e-6):
    """True per state when no hidden unit's pre-activation lies within `delta` of leakyrelu's kink (there fp32 and float64
    disagree about the sign and a whole gradient row differs between ANY two precisions: tests/test_gpu_split_backward.py)."""
    a = states.reshape(-1, F).astype(np.float64).T
    ok = np.ones(states.shape[0], bool)
    for (W, b) in np_oracle.unpack_params(params, F, hid, 2)[:-1]:
        z = W.astype(np.float64) @ a + b.astype(np.float64)[:, None]
        ok &= (np.abs(z).min(axis=0).reshape(states.shape[0], 32).min(axis=1) >= delta)
        a = np.where(z > 0, z, 0.01 * z)
    return ok


def _outputs(P, pol, ds, sel):
    l1, l2 = P.forward_backward(pol, ds, sel, EPS, ENT)
    B = len(sel)
    dy = np.zeros((B, 32, 4), np.float32)
    lt = np.zeros((B, 2), np.float64)
    L = P._lib.lib()
    L.ppo_debug_train_outputs.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.ppo_debug_train_outputs.restype = C.c_int32
    assert L.ppo_debug_train_outputs(pol._h, B, dy.ctypes.data, lt.ctypes.data) == 0
    return dy, lt, (l1, l2)


_REF = {}          # (hid, B) -> (inputs, float64 reference): computed once, shared by the two storage forms, never modified


def _reference(hid, B, params, cols):
    key = (hid, B)
    if key in _REF and all(np.array_equal(x, y) for x, y in zip(_REF[key][0], (params,) + cols)):
        return _REF[key][1]
    st, act, a0, po, adv = cols
    ref = np_oracle.step_batch_grad_chunked(np_oracle.step_batch_grad_torch, params, F, hid, st, np_oracle.batch_masks(act, 8),
                                            a0, po, adv, EPS, ENT, chunk=1024)
    _REF[key] = ((params,) + cols, ref)
    return ref


@pytest.mark.parametrize("hid,B,compact", CASES)
def test_helper_waves_hand_every_state_its_image_and_tail(P, hid, B, compact):
    assert B in (2, 3, 5, 4 * GRID_CAP[hid] + 1)
    P.set_rollout_compact(compact)
    P.set_bwd_split_bf16(True)
    assert _route(P, hid, compact, B)[0] == "k_policy_fwd_train_x6t<%d,2>" % hid
    rng = np.random.default_rng(1000 * hid + B)
    env = P.HipVecEnv(num_envs=48, Q=8, max_actions=12, seed=B)
    pol = P.HipPolicy(F, hid, 2, 4, seed=B + 1)
    pol.params = pol.params + (rng.normal(size=pol.num_params) * 0.02).astype(np.float32)
    ro = P.BufferRollouts()
    P.collect_rollouts_steps_(ro, env, pol, 48 if B > 1152 else 24, 1.0)      # step_batch! wants B <= 48 T transitions
    ds = P.construct_dataset(ro)
    st, act = ro.state_data
    st, act = st.reshape(-1, 32, F), act.reshape(-1)
    pool = np.flatnonzero(_off_the_kink(pol.params, hid, st))
    assert len(pool) >= 64                                           # (a minibatch may repeat samples)
    sel0 = pool[rng.choice(len(pool), size=B, replace=B > len(pool))]
    sel = sel0 + 1
    params = pol.params.copy()

    # 1. permutation invariance: a state's dY rows and loss terms follow it to any pass, tile and workgroup
    perm = rng.permutation(B)
    dy_a, lt_a, (lp, le) = _outputs(P, pol, ds, sel)
    g = pol.grad().copy()
    dy_b, lt_b, _ = _outputs(P, pol, ds, sel[perm])
    assert np.isfinite(dy_a).all() and np.isfinite(lt_a).all() and np.abs(dy_a).max() > 0
    distinct = len(np.unique(np.concatenate([st[sel0].reshape(B, -1).astype(np.int64), act[sel0].reshape(B, 1).astype(np.int64)], axis=1), axis=0))
    assert np.unique(lt_a[:, 1]).size >= (distinct + 1) // 2       # the inputs carry information (many transitions share a state)
    assert np.array_equal(dy_b.view(np.uint32), dy_a[perm].view(np.uint32))
    assert np.array_equal(lt_b.view(np.uint64), lt_a[perm].view(np.uint64))

    # 2. bitwise repeat
    lp2, le2 = P.forward_backward(pol, ds, sel, EPS, ENT)
    assert np.array_equal(g, pol.grad()) and (lp2, le2) == (lp, le)

    # 3. float64 autograd
    cols = (st[sel0], act[sel0], (ro.selected_actions.reshape(-1)[sel0] - 1).astype(np.int32),
            ro.selected_action_probabilities.reshape(-1)[sel0], ro.rewards.reshape(-1)[sel0])
    g64, olp, ole = _reference(hid, B, params, cols)
    scale = np.abs(g64).max()
    e1 = np.abs(g - g64).max() / scale
    print("hid %d B %d compact %d: |g - g64| / max|g64| = %.3e, loss %.3e %.3e" % (hid, B, compact, e1, abs(lp - olp), abs(le - ole)))
    assert e1 <= 2e-5
    assert abs(lp - olp) <= 1e-5 * (1 + abs(olp)) and abs(le - ole) <= 1e-5 * (1 + abs(ole))

    # 4. the fp32-MFMA pass of the same minibatch
    P.set_bwd_split_bf16(False)
    assert "x6" not in _route(P, hid, compact, B)[0]
    P.forward_backward(pol, ds, sel, EPS, ENT)
    d01 = np.abs(pol.grad() - g).max() / scale
    print("   |split - fp32 MFMA| / max|g64| = %.3e" % d01)
    assert d01 <= 4e-6
