"""The two-tile split train forward (k_policy_fwd_train_x6t) hands every state its own loss tail.

Each workgroup takes its tiles two per pass, several passes per launch, and the loss tail of a pass reads inputs (active
word, action, old probability, advantage) that were fetched one pass ahead.  A tail paired with the wrong state, or one
lost in the last (partial) pass, changes that state's dL/dlogits rows and loss terms.  So the same minibatch runs twice,
once as given and once permuted: states move to other passes and workgroups, and every state's dY rows and loss terms must
come out bit for bit the same.  dY and the loss terms of one state depend on that state and the minibatch size alone."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F, EPS, ENT = 72, 0.05, 0.01


@pytest.fixture(scope="module")
def P(ppo):
    if ppo.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests must run on the GPU box")
    return ppo


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


@pytest.mark.parametrize("hid,B", [(256, 4096), (256, 1537), (128, 4096)])
def test_train_forward_tail_follows_its_state(P, hid, B):
    rng = np.random.default_rng(hid + B)
    pol = P.HipPolicy(F, hid, 2, 4, seed=3)
    pol.params = (pol.params + (rng.normal(size=pol.num_params) * 0.02).astype(np.float32)).astype(np.float32)
    env = P.HipVecEnv(num_envs=1024, Q=8, max_actions=128, seed=11)
    ro = P.BufferRollouts()
    P.collect_rollouts_steps_(ro, env, pol, 8, 1.0)
    ds = P.construct_dataset(ro)
    assert len(ds) >= B
    sel = rng.permutation(len(ds))[:B] + 1
    perm = rng.permutation(B)
    dy_a, lt_a, _ = _outputs(P, pol, ds, sel)
    dy_b, lt_b, _ = _outputs(P, pol, ds, sel[perm])
    # the inputs carry information: states differ in their rows and loss terms
    assert np.isfinite(dy_a).all() and np.isfinite(lt_a).all()
    assert np.unique(lt_a[:, 1]).size > B // 2 and np.abs(dy_a).max() > 0
    bad = np.nonzero(~(dy_b == dy_a[perm]).all(axis=(1, 2)))[0]
    assert bad.size == 0, "dY of %d states moved with the permutation, first at position %d" % (bad.size, bad[0])
    assert np.array_equal(lt_b.view(np.uint64), lt_a[perm].view(np.uint64))
    assert np.array_equal(dy_b.view(np.uint32), dy_a[perm].view(np.uint32))
