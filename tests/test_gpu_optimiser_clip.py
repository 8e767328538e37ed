"""ClipValue, ClipNorm, WeightDecay, InvDecay and AdamW on the device, bit for bit against ClipRef
(tests/test_optimiser_clip.py): the replay of tests/test_gpu_optimiser_chain.py -- policy A trains through the engine,
policy B replays it with forward_backward -> ClipRef -> set_params -- through every update path: the fused ppo_train
(k_reduce_clip + k_clip_apply for a chain with ClipNorm, k_reduce_chain otherwise), the world-1 all-reduce hook and
step_batch! (k_chain_clip1 + k_clip_apply, or k_chain_update).

ClipNorm's thresh is set from the first minibatch: the median of the per-array norms of D where ClipNorm sits, so that
across the steps some arrays clip and others do not; the restatement asserts that both branches ran."""
import numpy as np
import pytest

from test_gpu_optimiser_chain import P, world1, _dataset, _same  # noqa: F401  (P, world1: fixtures)
from test_optimiser_clip import ClipRef, flux_arrays

pytestmark = pytest.mark.gpu

EPS, ENT = 0.05, 0.01


def _chains(P):
    """chain id -> member factory of thresh (ignored by chains without ClipNorm)."""
    return {
        "clipnorm+adam": lambda t: [P.ClipNorm(t), P.Adam(1e-3)],
        "adam+clipnorm": lambda t: [P.Adam(1e-3), P.ClipNorm(t)],
        "clipvalue+momentum": lambda t: [P.ClipValue(2e-3), P.Momentum(0.05, 0.9)],
        "weightdecay+adam+expdecay": lambda t: [P.WeightDecay(0.05), P.Adam(1e-3), P.ExpDecay(1.0, 0.5, 2, 1e-6, 0)],
        "invdecay+rmsprop": lambda t: [P.InvDecay(0.3), P.RMSProp(1e-3, 0.9, 1e-8)],
        "adamw": lambda t: P.AdamW(2e-3, (0.9, 0.999), 0.05).members,
        "clipnorm+adamw": lambda t: [P.ClipNorm(t), P.Adam(1.0, (0.9, 0.999)), P.WeightDecay(0.05), P.Descent(2e-3)],
        "clipnorm+invdecay+adam+weightdecay": lambda t: [P.ClipNorm(t), P.InvDecay(0.2), P.Adam(1e-3), P.WeightDecay(0.01)],
    }


def _setup(P, shape, dtype, ds_seed, B, epochs):
    F, hid, L = shape
    rng = np.random.default_rng(ds_seed)
    pol = P.HipPolicy(F, hid, L, 4, seed=3, dtype=dtype)
    ds = _dataset(P, pol, rng, B, F)
    perm = np.stack([rng.permutation(len(ds)) + 1 for _ in range(epochs)])
    return pol, ds, perm


def _thresh(P, make, shape, dtype, ds_seed, B, bs, epochs):
    """Median per-array norm of D at ClipNorm's position on the first minibatch (1.0 for chains without ClipNorm)."""
    members = make(1.0)
    names = [type(m).__name__ for m in members]
    if "ClipNorm" not in names:
        return 1.0
    c = names.index("ClipNorm")
    pol, ds, perm = _setup(P, shape, dtype, ds_seed, B, epochs)
    P.forward_backward(pol, ds, perm[0][:bs], EPS, ENT)
    ref = ClipRef(members[:c], pol.num_params)
    d = ref.delta(pol.grad(), pol.params)
    norms = [np.sqrt(np.sum(d[lo:hi].astype(np.float64) ** 2)) for lo, hi in flux_arrays(*shape)]
    return float(np.median(norms))


def _engine(P, make, shape, dtype, ds_seed, B, bs, epochs, path, parallel, t):
    pol, ds, perm = _setup(P, shape, dtype, ds_seed, B, epochs)
    n = len(ds)
    opt = P.Optimiser(*make(t))
    params, lrs = [], []
    for ep in range(epochs):
        if path == "step_batch":
            for s in range(0, n, bs):
                P.step_batch_(pol, opt, ds, perm[ep][s:s + bs], EPS, ENT)
        else:
            _, _, lr = P.ppo_train_(pol, opt, ds, EPS, bs, 1, ENT, perm=perm[ep:ep + 1],
                                    parallel=parallel() if parallel else None, verbose=False)
            lrs += lr
        params.append(pol.params)
    return params, opt, lrs, (pol, ds, perm)


def _check_state(opt, ref):
    st = opt.get_state()
    for j, (d, r) in enumerate(zip(st["members"], ref.m)):
        where = "member %d (%s)" % (j, d["kind"])
        assert d["kind"] == r["kind"], where
        if r["kind"] in ("ClipValue", "ClipNorm"):
            assert d["thresh"] == r["o"].thresh, where
        elif r["kind"] == "WeightDecay":
            assert d["wd"] == r["o"].wd, where
        elif r["kind"] == "InvDecay":
            assert d["gamma"] == r["o"].gamma and d["count"] == r["count"], where
        else:
            assert d["eta"] == r["eta"], where
        for key in ("m", "v", "velocity", "acc"):
            if key in r:
                assert _same(d[key], r[key]), where + " " + key
        if "beta_pow" in r:
            assert np.array_equal(d["beta_pow"], r["beta_pow"]), where
        if r["kind"] == "ExpDecay":
            assert d["count"] == r["count"], where


def _replay(P, chain, shape=(72, 128, 2), dtype="f32", B=300, bs=96, epochs=2, path="train", parallel=None, ds_seed=0):
    make = _chains(P)[chain]
    t = _thresh(P, make, shape, dtype, ds_seed, B, bs, epochs)
    pA, optA, lrA, (_, ds, perm) = _engine(P, make, shape, dtype, ds_seed, B, bs, epochs, path, parallel, t)
    F, hid, L = shape
    polB = P.HipPolicy(F, hid, L, 4, seed=3, dtype=dtype)
    ref = ClipRef(make(t), polB.num_params, flux_arrays(F, hid, L))
    x = polB.params
    n = len(ds)
    for ep in range(epochs):
        for s in range(0, n, bs):
            P.forward_backward(polB, ds, perm[ep][s:s + bs], EPS, ENT)
            x = ref.step(x, polB.grad())
            polB.params = x
        assert _same(pA[ep], x), "parameters after epoch %d" % ep
        if path != "step_batch":
            assert lrA[ep] == ref.lr(), "lr history, epoch %d" % ep
    _check_state(optA, ref)
    assert not np.array_equal(pA[-1], P.HipPolicy(F, hid, L, 4, seed=3, dtype=dtype).params), "the chain moved nothing"
    if any(type(m).__name__ == "ClipNorm" for m in optA.members):
        flags = np.array(ref.clipped)
        assert flags.any() and not flags.all(), "ClipNorm: both branches (clip / no clip) must run: %s" % flags.tolist()
    pA2, _, lrA2, _ = _engine(P, make, shape, dtype, ds_seed, B, bs, epochs, path, parallel, t)
    assert all(_same(a, b) for a, b in zip(pA, pA2)) and lrA2 == lrA, "bitwise repeat"


# ---------------------------------------------------------------- every chain: fused ppo_train
@pytest.mark.parametrize("chain", list(_chains(None)))
def test_clip_chain_fused_train(P, chain):
    _replay(P, chain)


# ---------------------------------------------------------------- the other update paths
@pytest.mark.parametrize("chain", ["adam+clipnorm", "clipnorm+adamw", "invdecay+rmsprop"])
def test_clip_chain_hook_path(P, world1, chain):
    """DataParallel(force_hook=True) at world 1: slab reduction, all-reduce hook, then k_chain_clip1 + k_clip_apply."""
    _replay(P, chain, parallel=world1)


@pytest.mark.parametrize("chain", ["clipnorm+adam", "clipvalue+momentum"])
def test_clip_chain_step_batch(P, chain):
    _replay(P, chain, path="step_batch")


@pytest.mark.parametrize("shape,dtype", [((72, 256, 2), "bf16"), ((72, 128, 3), "f32"), ((216, 256, 2), "f32"),
                                         ((72, 50, 2), "f32")], ids=["bf16-h256", "L3", "F216", "padded-h50"])
def test_clip_chain_shapes(P, shape, dtype):
    _replay(P, "clipnorm+invdecay+adam+weightdecay", shape=shape, dtype=dtype, B=200, bs=64)


def test_clip_chain_bench_minibatch(P):
    """One 4096-state minibatch per step at HID = 256, the benchmark's shape."""
    _replay(P, "adam+clipnorm", shape=(72, 256, 2), B=4096, bs=4096, epochs=2)


# ---------------------------------------------------------------- resume
def test_clip_chain_resume(P):
    """2 epochs in one go == 1 epoch, get_state -> a fresh chain -> set_state, 1 more epoch (InvDecay's count, the hyper
    values of the stateless members, Adam's state)."""
    make = _chains(P)["clipnorm+invdecay+adam+weightdecay"]
    rng = np.random.default_rng(9)
    polA = P.HipPolicy(72, 128, 2, 4, seed=4)
    ds = _dataset(P, polA, rng, 300, 72)
    optA = P.Optimiser(*make(0.05))
    _, _, lrA = P.ppo_train_(polA, optA, ds, EPS, 64, 2, ENT, seed=17, verbose=False)
    polC = P.HipPolicy(72, 128, 2, 4, seed=4)
    optC = P.Optimiser(*make(0.05))
    _, _, lr1 = P.ppo_train_(polC, optC, ds, EPS, 64, 1, ENT, seed=17, verbose=False)
    st = optC.get_state()
    assert st["epochs"] == 1 and st["members"][1]["count"] == 5
    optD = P.Optimiser(*make(123.0))               # the checkpoint's thresh replaces the constructor's
    optD.set_state(polC, st)
    assert optD.members[0].thresh == 0.05
    _, _, lr2 = P.ppo_train_(polC, optD, ds, EPS, 64, 1, ENT, seed=17, verbose=False)
    assert _same(polA.params, polC.params)
    assert lr1 + lr2 == lrA
    sa, sd = optA.get_state(), optD.get_state()
    assert sa["epochs"] == sd["epochs"] == 2 and sd["members"][1]["count"] == 10
    for a, d in zip(sa["members"], sd["members"]):
        assert a.keys() == d.keys()
        for k in a:
            assert np.array_equal(a[k], d[k]) if isinstance(a[k], np.ndarray) else a[k] == d[k], (a["kind"], k)


# ---------------------------------------------------------------- the C ABI
def test_clip_abi_errors(P):
    import ctypes as C
    pol = P.HipPolicy(72, 128, 2, 4, seed=1)
    lib = P._lib.lib()
    for kinds, row in (([8], [float("nan")]), ([7], [-0.5])):
        k = np.array(kinds, np.int32)
        h = np.array(row + [0.0] * 4, np.float64)
        out = C.c_void_p()
        assert lib.ppo_optimiser_create(pol._h, 1, P._p(k, P._lib.c_i32p), P._p(h, P._lib.c_f64p), C.byref(out)) == -1
    k = np.array([9, 1], np.int32)
    h = np.array([[0.1, 0, 0, 0, 0], [1e-3, 0.9, 0.999, 1e-8, 0]], np.float64)
    out = C.c_void_p()
    assert lib.ppo_optimiser_create(pol._h, 2, P._p(k, P._lib.c_i32p), P._p(h, P._lib.c_f64p), C.byref(out)) == 0
    try:
        e = C.c_double(0)
        assert lib.ppo_optimiser_get_eta(out, 0, C.byref(e)) == -1        # WeightDecay has no eta
        assert lib.ppo_optimiser_set_eta(out, 0, C.c_double(0.5)) == -1
        assert lib.ppo_optimiser_get_eta(out, 1, C.byref(e)) == 0 and e.value == 1e-3
        hy = np.zeros(5, np.float64)
        assert lib.ppo_optimiser_get_hyper(out, 0, P._p(hy, P._lib.c_f64p)) == 0 and hy[0] == 0.1
        hy[0] = 0.25
        assert lib.ppo_optimiser_set_hyper(out, 0, P._p(hy, P._lib.c_f64p)) == 0
        assert lib.ppo_optimiser_get_hyper(out, 0, P._p(hy, P._lib.c_f64p)) == 0 and hy[0] == 0.25
        lr = C.c_double(0)
        assert lib.ppo_adam_get_lr(out, C.byref(lr)) == 0 and lr.value == 1e-3   # the members with eta only
    finally:
        lib.ppo_adam_destroy(out)
