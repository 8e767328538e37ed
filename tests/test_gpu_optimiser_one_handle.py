"""Every optimiser handle is a chain (include/ppo_hip.h): ppo_adam_create(pol, ...) and ppo_optimiser_create(pol, 1, [Adam])
make the same thing, and the ppo_adam_* and ppo_optimiser_*(member 0) accessors read and write the same state on either.

Optimiser A is the Python Optimiser(Adam(...)), which binds through ppo_adam_create; optimiser B is a raw
ppo_optimiser_create handle of Adam alone, which Python never makes.  Both train the same policy on the same minibatches:
parameters, m, v and the float64 beta powers must agree bit for bit through the fused launch (k_reduce_adam) and the
standalone one (k_adam), B must run the Adam kernels and not the chain kernels, and state taken through one set of
accessors must resume through the other.  hidden = 50 runs on the 128-wide kernels, so every state copy crosses the
user-width / kernel-width conversion."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_optimiser_chain import _dataset, _same

pytestmark = pytest.mark.gpu

EPS, ENT = 0.05, 0.01
PPO_OPT_ADAM, PPO_OPT_EXPDECAY, PPO_ERR_ARG = 1, 2, -1
ETA, BETA, EPSILON = 2e-3, (0.8, 0.99), 1e-7
ADAM_ROW = [ETA, BETA[0], BETA[1], EPSILON, 0.0]


@pytest.fixture(scope="module")
def P(ppo):
    if ppo.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests must run on the GPU box")
    return ppo


def _f32(P, a):
    return a.ctypes.data_as(P._lib.c_f32p)


def _f64(P, a):
    return a.ctypes.data_as(P._lib.c_f64p)


class _RawChain:
    """Stands in for an Optimiser in ppo_train_ / step_batch_: its handle is a raw ppo_optimiser_create chain."""

    def __init__(self, P, pol, kinds=(PPO_OPT_ADAM,), rows=(ADAM_ROW,)):
        self._P = P
        k, h = np.array(kinds, np.int32), np.ascontiguousarray(rows, np.float64)
        self._h = C.c_void_p()
        P._lib.call("ppo_optimiser_create", pol._h, len(k), k.ctypes.data_as(P._lib.c_i32p), _f64(P, h), C.byref(self._h))

    def _handle(self, policy):
        return self._h

    def _pull(self):
        pass

    def destroy(self):
        self._P._lib.call("ppo_adam_destroy", self._h)
        self._h = None


def _adam_state(P, h, n):
    m, v, bp = np.empty(n, np.float32), np.empty(n, np.float32), np.empty(2, np.float64)
    P._lib.call("ppo_adam_get_state", h, _f32(P, m), _f32(P, v), _f64(P, bp))
    return m, v, bp


def _member_state(P, h, n):
    m, v, bp, cnt = np.empty(n, np.float32), np.empty(n, np.float32), np.empty(2, np.float64), C.c_int64(-1)
    P._lib.call("ppo_optimiser_get_state", h, 0, _f32(P, m), _f32(P, v), _f64(P, bp), C.byref(cnt))
    assert cnt.value == 0
    return m, v, bp


def _lr_and_eta(P, h):
    lr, eta = C.c_double(0), C.c_double(0)
    P._lib.call("ppo_adam_get_lr", h, C.byref(lr))
    P._lib.call("ppo_optimiser_get_eta", h, 0, C.byref(eta))
    return lr.value, eta.value


def _hyper(P, h):
    row = np.full(5, -1.0)
    P._lib.call("ppo_optimiser_get_hyper", h, 0, _f64(P, row))
    return list(row)


def _same_everywhere(P, polA, polB, hA, hB, steps, where):
    """Parameters and the Adam state of the two handles, each read through both sets of accessors."""
    assert _same(polA.params, polB.params), where + ": parameters"
    n = polA.num_params
    ref = _adam_state(P, hA, n)
    assert np.any(ref[0] != 0) and np.any(ref[1] != 0), where + ": the update left no state"
    # beta^(steps + 1), multiplied up one step at a time as the engine does after each launch
    want = [BETA[0], BETA[1]]
    for _ in range(steps):
        want = [want[0] * BETA[0], want[1] * BETA[1]]
    assert list(ref[2]) == want, where + ": beta powers"
    for name, got in (("optimiser_get_state(B)", _member_state(P, hB, n)), ("optimiser_get_state(A)", _member_state(P, hA, n)),
                      ("adam_get_state(B)", _adam_state(P, hB, n))):
        assert _same(ref[0], got[0]) and _same(ref[1], got[1]), "%s: m, v through %s" % (where, name)
        assert np.array_equal(ref[2], got[2]), "%s: beta powers through %s" % (where, name)
    assert _lr_and_eta(P, hA) == (ETA, ETA) and _lr_and_eta(P, hB) == (ETA, ETA), where + ": lr"


def _launches(P, *names):
    return [P.profile_get(k)[1] for k in names]


@pytest.mark.parametrize("hid", [128, 50], ids=["h128", "padded-h50"])
def test_adam_alone_is_one_handle(P, hid):
    rng = np.random.default_rng(1)
    polA, polB = (P.HipPolicy(72, hid, 2, 4, seed=3) for _ in range(2))
    start = polA.params
    ds = _dataset(P, polA, rng, 64, 72)
    perm = np.stack([rng.permutation(64) + 1 for _ in range(2)])
    optA = P.Optimiser(P.Adam(ETA, BETA, EPSILON))
    optB = _RawChain(P, polB)
    P.profile_enable(True)
    try:
        # fused path: one epoch of two minibatches; B runs k_reduce_adam, never k_reduce_chain
        P.ppo_train_(polA, optA, ds, EPS, 32, 1, ENT, perm=perm[:1], verbose=False)
        before = _launches(P, "k_reduce_adam", "k_reduce_chain")
        P.ppo_train_(polB, optB, ds, EPS, 32, 1, ENT, perm=perm[:1], verbose=False)
        after = _launches(P, "k_reduce_adam", "k_reduce_chain")
        assert after[0] == before[0] + 2 and after[1] == before[1], "a chain of Adam alone runs the Adam kernels (fused)"
        hA, hB = optA.members[0]._h, optB._h
        assert not _same(start, polA.params), "the epoch moved nothing"
        _same_everywhere(P, polA, polB, hA, hB, 2, "fused")

        # unfused path: two step_batch! calls; B runs k_adam, never k_chain_update
        for s in (0, 32):
            P.step_batch_(polA, optA, ds, perm[1][s:s + 32], EPS, ENT)
        before = _launches(P, "k_adam", "k_chain_update")
        for s in (0, 32):
            P.step_batch_(polB, optB, ds, perm[1][s:s + 32], EPS, ENT)
        after = _launches(P, "k_adam", "k_chain_update")
        assert after[0] == before[0] + 2 and after[1] == before[1], "a chain of Adam alone runs the Adam kernels (unfused)"
        _same_everywhere(P, polA, polB, hA, hB, 4, "unfused")
    finally:
        P.profile_enable(False)

    # state round trip: out of A through ppo_adam_get_state, into a fresh chain-created handle through
    # ppo_optimiser_set_state; the epoch count keys the seeded device permutation
    m, v, bp = _adam_state(P, hA, polA.num_params)
    ep = C.c_int64(0)
    P._lib.call("ppo_adam_get_epoch_count", hA, C.byref(ep))
    assert ep.value == 1
    optC = _RawChain(P, polB)
    P._lib.call("ppo_optimiser_set_state", optC._h, 0, _f32(P, m), _f32(P, v), _f64(P, bp), None)
    P._lib.call("ppo_adam_set_epoch_count", optC._h, ep.value)
    P.ppo_train_(polA, optA, ds, EPS, 32, 1, ENT, seed=17, verbose=False)
    P.ppo_train_(polB, optC, ds, EPS, 32, 1, ENT, seed=17, verbose=False)
    _same_everywhere(P, polA, polB, hA, optC._h, 6, "resumed")

    # hyper-parameters: ppo_adam_set_lr is member 0's eta; set_hyper on Adam leaves the beta powers alone
    P._lib.call("ppo_adam_set_lr", hB, 5e-4)
    assert _hyper(P, hB) == [5e-4, BETA[0], BETA[1], EPSILON, 0.0]
    assert _lr_and_eta(P, hB) == (5e-4, 5e-4)
    new = np.array([1e-3, 0.7, 0.9, 1e-6, 0.0])
    P._lib.call("ppo_optimiser_set_hyper", hA, 0, _f64(P, new))
    assert _hyper(P, hA) == list(new)
    assert np.array_equal(_adam_state(P, hA, polA.num_params)[2], bp * np.array(BETA) * np.array(BETA))
    optB.destroy()
    optC.destroy()


def test_adam_accessors_refuse_a_longer_chain(P):
    pol = P.HipPolicy(72, 128, 2, 4, seed=3)
    opt = _RawChain(P, pol, (PPO_OPT_ADAM, PPO_OPT_EXPDECAY), ([1e-3, 0.9, 0.999, 1e-8, 0.0], [1.0, 0.5, 2.0, 1e-6, 0.0]))
    L, n = P._lib.lib(), pol.num_params
    m, v, bp, eta = np.zeros(n, np.float32), np.zeros(n, np.float32), np.ones(2), C.c_double(0)
    assert L.ppo_adam_set_lr(opt._h, 1e-3) == PPO_ERR_ARG
    assert L.ppo_adam_get_state(opt._h, _f32(P, m), _f32(P, v), _f64(P, bp)) == PPO_ERR_ARG
    assert L.ppo_adam_set_state(opt._h, _f32(P, m), _f32(P, v), _f64(P, bp)) == PPO_ERR_ARG
    assert L.ppo_optimiser_get_eta(opt._h, 2, C.byref(eta)) == PPO_ERR_ARG
    assert L.ppo_optimiser_get_eta(opt._h, 1, C.byref(eta)) == 0 and eta.value == 1.0
    lr = C.c_double(0)
    assert L.ppo_adam_get_lr(opt._h, C.byref(lr)) == 0 and lr.value == 1e-3 * 1.0
    opt.destroy()
