"""The advantage modes "gae", "gae_normalised" and "returns_normalised" of ppo_train / step_batch on the device.

1. every train-forward family reads the advantage column it is handed, each asserted by its kernel name
   (ppo_debug_train_route): gradient and losses against float64 fed with that column; bit identities against a run in mode
   "returns" on a buffer that holds the same numbers in its returns column (gradient, loss terms, stored ratios); the loss
   term is ratio * A or the clip value of A, bit for bit.  The inputs make a wrong column, a neighbouring state's value or an
   unnormalised column visible (tests/test_advantage_modes_host.py shows that on the CPU; asserted again here);
2. k_adv_normalise at every width around and beyond its 1024 threads: the advantage the tail consumed, read back from the
   loss term of an all-clipped minibatch, within 1 fp32 ulp of numpy's float64 normalisation.  Derived, not measured: two
   fp64 reductions in different orders differ by about B 2^-53 relative, ten orders of magnitude below half an fp32 ulp, so
   the two results can differ only at a rounding tie.  Constant columns, a large mean, repeated states, a small minibatch
   after a large one, a dataset whose order is not the transition order;
3. the epoch loop in each mode against a replay through forward_backward and the oracle's Adam, bit for bit: every
   minibatch is normalised over its own slice of the epoch's order, the short last one included.

TEST_RECORD_DIR=<dir>: append the measured worst case of every case to <dir>/advantage_modes.jsonl."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import advantage_modes_ref as ref
from test_train_route import route

pytestmark = pytest.mark.gpu

BAR, LOSS_BAR = 2e-5, 1e-5                      # fp32: max|g - g64| <= BAR max|g64|, the bar of every fp32 gradient test here
BF16_BAR, BF16_L2, BF16_LOSS = 1e-2, 3e-3, 2e-3   # tests/test_gpu_bf16.py: per element, in the 2-norm, on the losses
EPS, ENT = ref.EPS, ref.ENT
U32, U64 = np.uint32, np.uint64


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
    P.set_fwd_split_t2_min_tiles(128, None)


def _record(rec):
    print(json.dumps(rec))
    d = os.environ.get("TEST_RECORD_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "advantage_modes.jsonl"), "a") as f:
            f.write(json.dumps(rec) + "\n")


def _debug(P):
    L = P._lib.lib()
    L.ppo_debug_train_ratios.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.ppo_debug_train_ratios.restype = C.c_int32
    L.ppo_debug_train_outputs.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.ppo_debug_train_outputs.restype = C.c_int32
    return L


def _ratios(P, pol, n):
    out = np.zeros(n, np.float32)
    assert _debug(P).ppo_debug_train_ratios(pol._h, n, out.ctypes.data) == 0, P._lib.last_error()
    return out


def _loss_terms(P, pol, B):
    lt = np.zeros((B, 2), np.float64)
    assert _debug(P).ppo_debug_train_outputs(pol._h, B, None, lt.ctypes.data) == 0, P._lib.last_error()
    return lt


def _policy(P, c, params):
    pol = P.HipPolicy(c["F"], c["hid"], c["L"], 4, dtype=c["dtype"])
    pol.params = params
    pol.target_kl = float("inf")                         # the ratios are stored while a target is set: record, never stop
    return pol


def _load(P, d, returns):
    """A [T, N] buffer through set_columns with `returns` in the returns column and an explicit terminal column."""
    T, N = d["T"], d["N"]
    H, F = d["states"].shape[1:]
    ro = P.BufferRollouts()
    ro.set_columns(None, d["states"].reshape(T, N, H, F), d["active"].reshape(T, N), d["a0"].reshape(T, N).astype(np.int64) + 1,
                   d["p_old"].reshape(T, N), np.asarray(returns, np.float32).reshape(T, N), d["terminal"])
    return ro


def _gae(P, orc, ro, V, raw, terminal):
    """The device's GAE column, flat: the array compute_gae_ returns, which is the oracle's scan bit for bit."""
    A, _ = P.compute_gae_(ro, V, ref.GAMMA, ref.LAM)
    want, _ = orc.gae_tn(raw, terminal, V, ref.GAMMA, ref.LAM)
    assert np.array_equal(A.view(U32), want.view(U32))
    return A.reshape(-1)


def _run(P, pol, ds, sel0, mode, eps=EPS):
    lp, le = P.forward_backward(pol, ds, sel0 + 1, eps, ENT, advantage=mode)
    return dict(lp=lp, le=le, g=pol.grad(), lt=_loss_terms(P, pol, len(sel0)), r=_ratios(P, pol, len(sel0)))


def _same_bits(a, b, what):
    assert np.array_equal(a["g"].view(U32), b["g"].view(U32)), what + ": gradient"
    assert np.array_equal(a["lt"].view(U64), b["lt"].view(U64)), what + ": loss terms"
    assert np.array_equal(a["r"].view(U32), b["r"].view(U32)), what + ": stored ratios"
    assert (a["lp"], a["le"]) == (b["lp"], b["le"]), what + ": losses"


def _against_reference(c, d, out, adv, rec, eps=EPS):
    """Gradient and both losses of a run against the float64 reference (bf16: its restated arithmetic) fed with `adv`."""
    g64, olp, ole = ref.reference_gradient(c, d["params"], ref.minibatch(d), adv, eps=eps)
    scale = float(np.abs(g64).max())
    assert scale > 0
    err = float(np.abs(out["g"] - g64).max() / scale)
    l2 = float(np.linalg.norm(out["g"] - g64) / np.linalg.norm(g64))
    bf16 = c["dtype"] == "bf16"
    bar, lbar = (BF16_BAR, BF16_LOSS) if bf16 else (BAR, LOSS_BAR)
    el = max(abs(out["lp"] - olp) / (1 + abs(olp)), abs(out["le"] - ole) / (1 + abs(ole)))
    rec.update(err_over_max=err, err_over_bar=err / bar, l2=l2, loss_err_over_bar=el / lbar)
    _record(rec)
    assert err <= bar, rec
    assert not bf16 or l2 <= BF16_L2, rec
    assert el <= lbar, rec


def _assert_loss_terms(out, adv, eps=EPS):
    """loss_terms[:, 0] is fl32(ratio * A) where unclipped and (1 +- eps) * double(A) where clipped, bit for bit."""
    adv = np.asarray(adv, np.float32)
    clip = ref.clip_value(adv, eps)
    gain = (out["r"] * adv).astype(np.float64)            # fl(fl(ps / po) * adv): numpy's float32 product is the device's
    un = gain < clip
    assert 20 * un.sum() >= len(adv) and 20 * (~un).sum() >= len(adv), (int(un.sum()), len(adv))
    assert np.array_equal(gain[un].view(U64), out["lt"][un, 0].view(U64)), "unclipped: the loss term is ratio * advantage"
    assert np.all(gain[~un] >= clip[~un])
    assert np.array_equal(clip[~un].view(U64), out["lt"][~un, 0].view(U64)), "clipped: the loss term is the clip value"


def _setup(P, fam):
    """Set the family's knobs and assert its route by kernel name."""
    c = ref.FAMILIES[fam]
    if "split" in c["setup"]:
        P.set_bwd_split_bf16(c["setup"]["split"])
    if "compact" in c["setup"]:
        P.set_rollout_compact(True)
    if "tile" in c["setup"]:
        P.set_train_tile_max_tiles(c["setup"]["tile"])
    got = route(P, c["dtype"], c["F"], c["hid"], c["L"], 4 * c["Q"], c["compact"], c["B"])
    if c["fwd"] is None:                                   # the split-fp32 forward from compact storage, named by the library
        assert got[0].startswith("k_policy_fwd_train_x6") and got[1] == "k_policy_bwd_x6<72,256>", got
    else:
        assert got[0] == c["fwd"], (fam, got)
    return c, got


def _expanded(P, orc, fam):
    c, got = _setup(P, fam)
    d = ref.expanded_case(fam)
    pol = _policy(P, c, d["params"])
    ro = _load(P, d, d["R"])
    A = _gae(P, orc, ro, d["V"], d["R"].reshape(d["T"], d["N"]), d["terminal"])
    return c, got, d, pol, ro, A


def _compact(P, orc, fam):
    """An engine rollout in compact storage, then the policy moved away from the one that collected it."""
    c, got = _setup(P, fam)
    r = ref.ROLLOUT
    p0, moved = ref.rollout_start()
    env = P.HipVecEnv(num_envs=r["N"], Q=r["Q"], max_actions=r["max_actions"], seed=r["env_seed"])
    pol = _policy(P, c, p0)
    ro = P.BufferRollouts()
    P.collect_rollouts_steps_(ro, env, pol, r["T"], r["discount"])
    pol.params = moved
    n = r["N"] * r["T"]
    st, act = ro.state_data
    d = ref.compact_case(fam, moved, st.reshape(n, 32, c["F"]), act.reshape(n), (ro.selected_actions.reshape(n) - 1).astype(np.int32),
                         ro.selected_action_probabilities.reshape(n), ro.rewards.reshape(n))
    A = _gae(P, orc, ro, d["V"], ro.raw_rewards, ro.terminal.astype(np.uint8))
    return c, got, d, pol, ro, A


def _family(P, orc, fam):
    return (_compact if ref.FAMILIES[fam]["compact"] else _expanded)(P, orc, fam)


# ---------------------------------------------------------------- 1. every family reads the column it is given
@pytest.mark.parametrize("fam", list(ref.FAMILIES))
def test_family_reads_the_gae_column(P, orc, knobs, fam):
    c, got, d, pol, ro, A = _family(P, orc, fam)
    cond = ref.family_conditions(d, A)                     # a wrong column, state or clip side cannot pass
    ds = P.construct_dataset(ro)
    sel0 = d["sel0"]
    out = _run(P, pol, ds, sel0, "gae")
    _against_reference(c, d, out, A[sel0], dict(case="family", family=fam, mode="gae", fwd=got[0], bwd=got[1], **cond))
    _assert_loss_terms(out, A[sel0])
    if c["compact"]:
        # lambda = 1, V = 0: the GAE column IS the returns column, and the two modes are one computation
        r = ref.ROLLOUT
        A1, _ = P.compute_gae_(ro, np.zeros((r["T"] + 1, r["N"]), np.float32), r["discount"], 1.0)
        assert np.array_equal(A1.view(U32), ro.rewards.view(U32))
        _same_bits(_run(P, pol, ds, sel0, "gae"), _run(P, pol, ds, sel0, "returns"), "lambda = 1, V = 0")
    else:
        # a second buffer with the same columns but A in the returns column, trained in mode "returns"
        ro2 = _load(P, d, A)
        same = _run(P, pol, P.construct_dataset(ro2), sel0, "returns")
        _same_bits(out, same, "A as the returns column")
        # ... and the first buffer's own returns column gives another gradient: the identity is not vacuous
        other = _run(P, pol, ds, sel0, "returns")
        assert not np.array_equal(other["g"], out["g"]) and not np.array_equal(other["lt"][:, 0], out["lt"][:, 0])
        assert np.array_equal(other["r"].view(U32), out["r"].view(U32)), "a state's ratio does not depend on the advantage"


@pytest.mark.parametrize("fam", list(ref.FAMILIES))
def test_family_normalised_modes(P, orc, knobs, fam):
    c, got, d, pol, ro, A = _family(P, orc, fam)
    ds = P.construct_dataset(ro)
    sel0 = d["sel0"]
    for mode, col in (("gae_normalised", A), ("returns_normalised", d["R"])):
        adv = ref.normalise64(col[sel0])
        out = _run(P, pol, ds, sel0, mode)
        _against_reference(c, d, out, adv, dict(case="family", family=fam, mode=mode, fwd=got[0], bwd=got[1]))


# ---------------------------------------------------------------- 2. the normaliser itself, at every width
NORM = dict(dtype="f32", F=ref.NORM_F, Q=ref.NORM_Q, hid=ref.NORM_HID, L=ref.NORM_L)


def _normaliser_route(P, *sizes):
    """k_policy_fwd_train_x6<128> at every size: the two-tile form of the split forward is switched off."""
    P.set_fwd_split_t2_min_tiles(128, 0)
    for B in sizes:
        assert route(P, "f32", ref.NORM_F, ref.NORM_HID, ref.NORM_L, 4 * ref.NORM_Q, False, B)[0] == ref.NORM_KERNEL, B


@pytest.mark.parametrize("name", list(ref.NORMALISER))
def test_normaliser_at_every_width(P, orc, knobs, name):
    n, B, col, contents = ref.NORMALISER[name]
    _normaliser_route(P, B)
    d = ref.normaliser_case(name, orc.gae_tn)
    assert ref.all_clipped64(d) == 0, "the float64 restatement clips every sample"
    pol = _policy(P, NORM, d["params"])
    ro = _load(P, d, d["R"])
    if col == "gae":
        assert np.array_equal(_gae(P, orc, ro, d["V"], d["R"].reshape(d["T"], d["N"]), d["terminal"]).view(U32), d["x"].view(U32))
    ds = P.construct_dataset(ro)
    sel0 = d["sel0"]
    out = _run(P, pol, ds, sel0, col + "_normalised", eps=ref.NORM_EPS)
    adv, again = ref.advantage_from_term(out["lt"][:, 0])
    assert np.array_equal(again.view(U64), out["lt"][:, 0].view(U64)), "every term is (1 +- eps) * double(adv): adv is recovered"
    ulps = ref.ulp_distance(adv, d["want"])
    _record(dict(case="normaliser", name=name, B=B, worst_ulp=int(ulps.max()), differing=int((ulps > 0).sum())))
    assert ulps.max() <= 1, (name, int(ulps.max()), int(np.argmax(ulps)))
    if B != n:                                             # repeated states: the scatter writes equal values
        first = {}
        for i, s in enumerate(sel0):
            assert adv[i] == adv[first.setdefault(s, i)]
    if contents == "constant" or B == 1:
        # std = 0: the advantage is exactly 0, and the gradient is that of a "returns" run on an all-zero column
        assert not adv.any() and not d["want"].any()
        zero = _run(P, pol, P.construct_dataset(_load(P, d, np.zeros(n, np.float32))), sel0, "returns", eps=ref.NORM_EPS)
        assert np.array_equal(zero["g"].view(U32), out["g"].view(U32)) and np.abs(out["g"]).max() > 0
        assert np.array_equal(zero["lt"].view(U64), out["lt"].view(U64))


def test_small_minibatch_after_a_large_one(P, orc, knobs):
    """300 states after 5000 on the same policy: nothing the larger minibatch left behind (its scratch column, its loss terms)
    leaks into the smaller one.  Against a fresh policy with the same parameters, bit for bit."""
    _normaliser_route(P, 5000, 300)
    d = ref.normaliser_case("B5000")
    ds = P.construct_dataset(_load(P, d, d["R"]))
    small = d["sel0"][1000:1300]
    used = _policy(P, NORM, d["params"])
    _run(P, used, ds, d["sel0"], "returns_normalised", eps=ref.NORM_EPS)
    after = _run(P, used, ds, small, "returns_normalised", eps=ref.NORM_EPS)
    fresh = _run(P, _policy(P, NORM, d["params"]), ds, small, "returns_normalised", eps=ref.NORM_EPS)
    _same_bits(after, fresh, "300 after 5000")
    # and it is the 300's own normalisation: where a sample is clipped, the term is the clip value of numpy's advantage
    want = ref.normalise64(d["R"][small])
    adv, _ = ref.advantage_from_term(after["lt"][:, 0])
    clipped = after["lt"][:, 0] == ref.clip_value(adv, ref.NORM_EPS)
    assert 4 * clipped.sum() >= 300 and ref.ulp_distance(adv[clipped], want[clipped]).max() <= 1


def test_normalised_modes_on_an_episode_dataset(P, orc, knobs):
    """Episode-mode rollouts: ro.index() is not arange and some transitions are invalid.  The normaliser gathers and scatters by
    transition id: the gradient of a minibatch of dataset positions against float64, the columns gathered through ro.index()."""
    c = dict(dtype="f32", F=72, Q=8, hid=128, L=2)
    B = 200
    assert route(P, "f32", 72, 128, 2, 32, False, B)[0] == ref.NORM_KERNEL
    rng = np.random.default_rng(77)
    p0 = ref.make_params(72, 128, 2, 21)
    env = P.HipVecEnv(num_envs=16, Q=8, max_actions=6, seed=9)
    pol = _policy(P, c, p0)
    ro = P.BufferRollouts()
    P.collect_rollouts_(ro, env, pol, 40, ref.GAMMA)        # whole episodes: idle envs leave invalid transitions
    moved = (p0 + (rng.normal(size=p0.size) * 0.01).astype(np.float32)).astype(np.float32)
    pol.params = moved
    idx, valid = ro.index(), ro.valid
    assert 0 < valid.sum() < valid.size and len(idx) == valid.sum() and not np.array_equal(idx, np.arange(len(idx)))
    T, N = ro.dims()
    V = (rng.normal(size=(T + 1, N)) * 5).astype(np.float32)
    A, _ = P.compute_gae_(ro, V, ref.GAMMA, ref.LAM)
    st, act = ro.state_data
    cols = dict(params=moved, states=st.reshape(-1, 32, 72)[idx], active=act.reshape(-1)[idx],
                a0=(ro.selected_actions.reshape(-1)[idx] - 1).astype(np.int32), p_old=ro.selected_action_probabilities.reshape(-1)[idx])
    pool, _ = ref.trainable_pool(c, moved, cols["states"], cols["active"], cols["a0"], cols["p_old"])
    cols["sel0"] = rng.choice(pool, size=B, replace=len(pool) < B)
    ds = P.construct_dataset(ro)
    assert len(ds) == len(idx)
    for mode, col in (("returns_normalised", ro.rewards), ("gae_normalised", A)):
        x = col.reshape(-1)[idx][cols["sel0"]]
        assert np.unique(x).size > 8
        out = _run(P, pol, ds, cols["sel0"], mode)
        _against_reference(c, cols, out, ref.normalise64(x), dict(case="episodes", mode=mode, B=B, dataset=len(idx), pool=len(pool)))


# ---------------------------------------------------------------- 3. the epoch loop in each mode
def _loop(P, orc, mode, seed):
    """ppo_train_ over 2500 states in minibatches of 1100, 1100 and 300 against a second policy that runs forward_backward on
    the same slices, the oracle's Adam on grad(), then params =.  seed: the Feistel order instead of an explicit perm."""
    c, d = ref.LOOP, ref.loop_dataset()
    shape = dict(dtype="f32", F=ref.NORM_F, Q=ref.NORM_Q, hid=c["hid"], L=2)
    n, batch = c["n"], c["batch"]
    assert route(P, "f32", 72, c["hid"], 2, 32, False, batch)[0] == "k_policy_fwd_train_x6t<128,2>"
    assert route(P, "f32", 72, c["hid"], 2, 32, False, n % batch)[0] == "k_policy_fwd_train_x6<128>"
    ro = _load(P, d, d["R"])
    _gae(P, orc, ro, d["V"], d["R"].reshape(d["T"], d["N"]), d["terminal"])
    ds = P.construct_dataset(ro)
    polA, polB = _policy(P, shape, d["params"]), _policy(P, shape, d["params"])
    optA = P.Optimiser(P.Adam(c["eta"]))
    p = d["params"].copy()
    m, v, bp = np.zeros_like(p), np.zeros_like(p), np.array([0.9, 0.999])
    for ep in range(c["epochs"]):
        if seed is None:
            order = d["perm"][ep]
            h = P.ppo_train_(polA, optA, ds, c["eps"], batch, 1, c["ent"], perm=(order + 1)[None], verbose=False, advantage=mode)
        else:
            order = orc.feistel_perm(n, seed, ep)           # keyed by the epochs the optimiser has trained
            h = P.ppo_train_(polA, optA, ds, c["eps"], batch, 1, c["ent"], seed=seed, verbose=False, advantage=mode)
        lps, les = [], []
        for s in range(0, n, batch):
            lp, le = P.forward_backward(polB, ds, order[s:s + batch] + 1, c["eps"], c["ent"], advantage=mode)
            orc.adam_step(p, polB.grad(), m, v, bp, c["eta"])
            polB.params = p
            lps.append(lp)
            les.append(le)
        assert len(lps) == 3
        assert np.array_equal(polA.params.view(U32), p.view(U32)), "parameters after epoch %d" % ep
        # the tolerance of test_gpu_parity.py::test_ppo_train_epochs_with_explicit_perm
        assert np.allclose(h[0], [np.mean(lps)], rtol=1e-4, atol=1e-6) and np.allclose(h[1], [np.mean(les)], rtol=1e-4, atol=1e-7)
    dm, dv, dbp = optA.members[0].get_state()
    assert np.array_equal(dm.view(U32), m.view(U32)) and np.array_equal(dv.view(U32), v.view(U32)) and np.array_equal(dbp, bp)
    assert not np.array_equal(p, d["params"])


@pytest.mark.parametrize("mode", ["gae", "returns_normalised", "gae_normalised"])
def test_epoch_loop_in_each_mode(P, orc, knobs, mode):
    _loop(P, orc, mode, None)


def test_epoch_loop_with_the_seeded_order(P, orc, knobs):
    _loop(P, orc, "gae_normalised", 2 ** 32 + 7)
