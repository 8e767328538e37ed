"""Flux.Optimiser chains on the device (k_reduce_chain: the slab reduction with the chain fused in, single-rank ppo_train;
k_chain_update: the all-reduce hook path, step_batch!, ppo_adam_apply), bit for bit against the numpy restatement of the
arithmetic contract (tests/test_optimiser_chain.py, ChainRef).

Replay: policy A trains through the engine with an explicit permutation; policy B replays it minibatch by minibatch --
forward_backward -> grad() -> ChainRef -> params = -- so B's gradient is A's (forward_backward runs the same reduction,
tests/test_gpu_bench_shapes.py part (c)) and the only arithmetic that differs is the chain's.  After every epoch the
parameters, every member's state, its eta and the lr history must agree exactly, and a second engine run must repeat A
bit for bit.  A padded width (hidden = 50 runs on the 128 kernels) checks that the zero-padded units stay zero: a moved
padded unit would change A's later gradients and no longer match B, whose padding set_params writes as zeros."""
import numpy as np
import pytest

from test_optimiser_chain import ChainRef

pytestmark = pytest.mark.gpu

EPS, ENT = 0.05, 0.01


@pytest.fixture(scope="module")
def P(ppo):
    if ppo.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests must run on the GPU box")
    return ppo


@pytest.fixture(scope="module")
def world1(P):
    """A one-rank process group: ppo_train then updates through the all-reduce hook and k_chain_update."""
    import socket
    import torch.distributed as dist
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
    try:
        yield lambda: P.DataParallel(0, 1, force_hook=True)
    finally:
        P.rccl_finalize()
        dist.destroy_process_group()


def _chains(P):
    return {
        "adam+expdecay": lambda: [P.Adam(1e-3), P.ExpDecay(1.0, 0.5, 2, 1e-6, 0)],
        "expdecay+adam": lambda: [P.ExpDecay(1.0, 0.5, 3, 0.2, 1), P.Adam(2e-3, (0.8, 0.99), 1e-7)],
        "descent": lambda: [P.Descent(0.02)],
        "momentum": lambda: [P.Momentum(0.01, 0.9)],
        "nesterov": lambda: [P.Nesterov(0.01, 0.8)],
        "rmsprop": lambda: [P.RMSProp(1e-3, 0.9, 1e-8)],
        "expdecay1+descent": lambda: [P.ExpDecay(1.0, 0.5, 1, 1e-6, 0), P.Descent(0.02)],
        "descent+momentum+expdecay+rmsprop": lambda: [P.Descent(0.5), P.Momentum(0.02, 0.9), P.ExpDecay(1.0, 0.5, 2, 0.3, 1),
                                                      P.RMSProp(2e-3, 0.8, 1e-7)],
        "nesterov+rmsprop+adam+expdecay": lambda: [P.Nesterov(0.5, 0.7), P.RMSProp(1.0, 0.95, 1e-6), P.Adam(1e-3),
                                                   P.ExpDecay(1.0, 0.25, 2, 1e-6, 2)],
    }


CHAIN_IDS = list(_chains(None))


def _dataset(P, pol, rng, B, F):
    """B random states (Q = 8) through set_columns: actions sampled from the policy, p_old near p, advantages of both signs."""
    states = rng.integers(-3, 7, size=(B, 32, F)).astype(np.int8)
    active = rng.integers(1, 2 ** 8, size=B, dtype=np.uint64).astype(np.uint32)
    probs = P.batch_action_probabilities(pol, P.StateData(states, active)).T.astype(np.float64)
    cdf = np.cumsum(probs, axis=1)
    a0 = (cdf < (rng.random(B) * cdf[:, -1])[:, None]).sum(axis=1)
    p_old = (probs[np.arange(B), a0] * rng.uniform(0.8, 1.25, B)).astype(np.float32)
    adv = (rng.normal(size=B) * 3).astype(np.float32)
    ro = P.BufferRollouts()
    ro.set_columns(None, states[None], active[None], a0[None].astype(np.int64) + 1, p_old[None], adv[None])
    return P.construct_dataset(ro)


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _check_state(opt, ref, epoch):
    st = opt.get_state()
    for j, (d, r) in enumerate(zip(st["members"], ref.m)):
        where = "epoch %d member %d (%s)" % (epoch, j, d["kind"])
        assert d["kind"] == r["kind"] and d["eta"] == r["eta"], where
        for key in ("m", "v", "velocity", "acc"):
            if key in r:
                assert _same(d[key], r[key]), where + " " + key
        if "beta_pow" in r:
            assert np.array_equal(d["beta_pow"], r["beta_pow"]), where
        if "count" in r:
            assert d["count"] == r["count"], where
    return st


def _engine(P, make, shape, dtype, ds_seed, B, bs, epochs, path, parallel):
    """Train policy A through the engine; returns (A's parameters after each epoch, its chain, lr history, inputs)."""
    F, hid, L = shape
    rng = np.random.default_rng(ds_seed)
    pol = P.HipPolicy(F, hid, L, 4, seed=3, dtype=dtype)
    ds = _dataset(P, pol, rng, B, F)
    n = len(ds)
    perm = np.stack([rng.permutation(n) + 1 for _ in range(epochs)])
    opt = P.Optimiser(*make())
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


def _replay(P, make, shape=(72, 128, 2), dtype="f32", B=300, bs=96, epochs=2, path="train", parallel=None, ds_seed=0):
    pA, optA, lrA, (polA, ds, perm) = _engine(P, make, shape, dtype, ds_seed, B, bs, epochs, path, parallel)
    F, hid, L = shape
    polB = P.HipPolicy(F, hid, L, 4, seed=3, dtype=dtype)
    ref = ChainRef(make(), polB.num_params)
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
    _check_state(optA, ref, epochs)
    assert not np.array_equal(pA[-1], P.HipPolicy(F, hid, L, 4, seed=3, dtype=dtype).params), "the chain moved nothing"
    assert P.get_optimizer_learning_rate(optA) == ref.lr(), "decayed etas pulled back into the members"
    # reproducibility: a second engine run from the same inputs repeats the first bit for bit
    pA2, optA2, lrA2, _ = _engine(P, make, shape, dtype, ds_seed, B, bs, epochs, path, parallel)
    assert all(_same(a, b) for a, b in zip(pA, pA2)) and lrA2 == lrA, "bitwise repeat"
    return optA, ref


# ---------------------------------------------------------------- every chain: fused ppo_train, world 1
@pytest.mark.parametrize("chain", CHAIN_IDS)
def test_chain_fused_train(P, chain):
    make = _chains(P)[chain]
    for epochs in (1, 2):                        # the member state is compared after the first epoch and after the second
        _replay(P, make, epochs=epochs)


# ---------------------------------------------------------------- every update path
@pytest.mark.parametrize("chain", ["adam+expdecay", "nesterov+rmsprop+adam+expdecay", "momentum"])
def test_chain_hook_path(P, world1, chain):
    """DataParallel(force_hook=True) at world 1: slab reduction, all-reduce hook, then k_chain_update."""
    _replay(P, _chains(P)[chain], parallel=world1)


@pytest.mark.parametrize("chain", ["expdecay+adam", "descent+momentum+expdecay+rmsprop"])
def test_chain_step_batch(P, chain):
    _replay(P, _chains(P)[chain], path="step_batch")


@pytest.mark.parametrize("shape,dtype", [((72, 256, 2), "bf16"), ((72, 128, 3), "f32"), ((216, 256, 2), "f32"),
                                         ((72, 50, 2), "f32")], ids=["bf16-h256", "L3", "F216", "padded-h50"])
def test_chain_shapes(P, shape, dtype):
    _replay(P, _chains(P)["nesterov+rmsprop+adam+expdecay"], shape=shape, dtype=dtype, B=200, bs=64)


def test_chain_bench_minibatch(P):
    """One 4096-state minibatch per step at HID = 256, the benchmark's shape (k_reduce_chain at full size)."""
    _replay(P, _chains(P)["adam+expdecay"], shape=(72, 256, 2), B=4096, bs=4096, epochs=2)


# ---------------------------------------------------------------- resume
def test_chain_resume(P):
    """2 epochs in one go == 1 epoch, get_state -> a fresh chain -> set_state, 1 more epoch: parameters, member state, eta,
    and the device minibatch permutation (keyed by the epoch count the state carries) all bit-identical."""
    make = _chains(P)["nesterov+rmsprop+adam+expdecay"]
    rng = np.random.default_rng(9)
    polA = P.HipPolicy(72, 128, 2, 4, seed=4)
    ds = _dataset(P, polA, rng, 300, 72)
    optA = P.Optimiser(*make())
    _, _, lrA = P.ppo_train_(polA, optA, ds, EPS, 64, 2, ENT, seed=17, verbose=False)
    polC = P.HipPolicy(72, 128, 2, 4, seed=4)
    optC = P.Optimiser(*make())
    _, _, lr1 = P.ppo_train_(polC, optC, ds, EPS, 64, 1, ENT, seed=17, verbose=False)
    st = optC.get_state()
    assert st["epochs"] == 1
    optD = P.Optimiser(*make())
    optD.set_state(polC, st)
    _, _, lr2 = P.ppo_train_(polC, optD, ds, EPS, 64, 1, ENT, seed=17, verbose=False)
    assert _same(polA.params, polC.params)
    assert lr1 + lr2 == lrA
    sa, sd = optA.get_state(), optD.get_state()
    assert sa["epochs"] == sd["epochs"] == 2
    for a, d in zip(sa["members"], sd["members"]):
        assert a.keys() == d.keys()
        for k in a:
            assert np.array_equal(a[k], d[k]) if isinstance(a[k], np.ndarray) else a[k] == d[k], (a["kind"], k)
    assert [m.eta for m in optA.members] == [m.eta for m in optD.members]
    assert optA.members[3].eta < 1.0                 # the ExpDecay member decayed inside the run
