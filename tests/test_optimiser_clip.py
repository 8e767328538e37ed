"""Flux.Optimiser members without an eta (ClipValue, ClipNorm, WeightDecay, InvDecay; include/ppo_hip.h kinds 7..10) and
Flux 0.13's AdamW, CPU side: a numpy restatement of their arithmetic contract on top of ChainRef
(tests/test_optimiser_chain.py), by-hand first steps, the device's ClipNorm summation order emulated against math.fsum,
the Python classes, and the Julia shim's rows for them.

ClipRef is also the reference of tests/test_gpu_optimiser_clip.py, which replays the device's training step by step."""
import math
import os

import numpy as np
import pytest

from test_optimiser_chain import ChainRef, _hard_vector

f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_ETA = ("ClipValue", "ClipNorm", "WeightDecay", "InvDecay")


def flux_arrays(F, hid, L, out=4):
    """[lo, hi) of each of the 2L + 2 arrays of Flux.params(Policy(F, hid, L, out)) in the flat vector: W1, b1, (W, b) per
    hidden->hidden layer, W3, b3."""
    sizes = [hid * F, hid] + [hid * hid, hid] * (L - 1) + [out * hid, out]
    ends = np.cumsum(sizes)
    return [(int(e - s), int(e)) for s, e in zip(sizes, ends)]


def clip_norm_of(d):
    """nrm = f32(sqrt(S)), S = the exact float64 sum of the (exact) squares rounded once."""
    return f32(math.sqrt(math.fsum((d.astype(f64) ** 2).tolist())))


class ClipRef(ChainRef):
    """ChainRef with the members that have no eta.  `arrays`: the [lo, hi) ranges ClipNorm takes its norms over (default:
    the whole vector as one array).  `clipped` records, per ClipNorm application, one bool per array."""

    def __init__(self, members, n, arrays=None):
        self.arrays = arrays if arrays is not None else [(0, n)]
        self.clipped = []
        self.m = []
        for o in members:
            k = type(o).__name__
            if k in NO_ETA:
                st = {"kind": k, "o": o}
                if k == "InvDecay":
                    st["count"] = 0
            else:
                st = ChainRef([o], n).m[0]
            self.m.append(st)

    def delta(self, g, x=None):
        d = np.asarray(g, f32).copy()
        for st in self.m:
            o, k = st["o"], st["kind"]
            dd = d.astype(f64)
            if k == "ClipValue":
                t = o.thresh
                d = np.where(dd > t, t, np.where(dd < -t, -t, dd)).astype(f32)
            elif k == "ClipNorm":
                d, flags = d.copy(), []
                for lo, hi in self.arrays:
                    nrm = clip_norm_of(d[lo:hi])
                    flags.append(bool(f64(nrm) > o.thresh))
                    if flags[-1]:
                        d[lo:hi] = (d[lo:hi].astype(f64) * (o.thresh / f64(nrm))).astype(f32)
                self.clipped.append(flags)
            elif k == "WeightDecay":
                d = (dd + o.wd * np.asarray(x, f32).astype(f64)).astype(f32)
            elif k == "InvDecay":
                st["count"] += 1
                d = (dd * (1.0 / (1.0 + o.gamma * st["count"]))).astype(f32)
            else:
                one = ChainRef.__new__(ChainRef)
                one.m = [st]
                d = one.delta(d)
        return d

    def step(self, params, g):
        x = np.asarray(params, f32)
        return (x - self.delta(g, x)).astype(f32)

    def lr(self):
        p = 1.0
        for st in self.m:
            if st["kind"] not in NO_ETA:
                p *= st["eta"]
        return p


# ---------------------------------------------------------------- by hand
def test_clipvalue_by_hand(ppo):
    g = np.array([0.5, -2.0, 0.0, 1e-3, np.nan, -0.25, np.inf], f32)
    r = ClipRef([ppo.ClipValue(0.3)], g.size)
    d = r.delta(g)
    assert np.array_equal(d[[0, 1, 2, 3, 5, 6]], np.array([f32(0.3), f32(-0.3), 0.0, f32(1e-3), -0.25, f32(0.3)], f32))
    assert np.isnan(d[4])                          # NaN stays NaN


def test_weightdecay_by_hand(ppo):
    g, x = np.array([0.5, -2.0, 0.0], f32), np.array([1.0, 3.0, -0.7], f32)
    r = ClipRef([ppo.WeightDecay(0.01), ppo.Descent(0.1)], 3)
    D = (g.astype(f64) + 0.01 * x.astype(f64)).astype(f32)
    assert np.array_equal(r.delta(g, x), (D.astype(f64) * 0.1).astype(f32))
    assert np.array_equal(r.step(x, g), x - (D.astype(f64) * 0.1).astype(f32))


def test_invdecay_by_hand(ppo):
    g = np.array([0.5, -2.0, 3.0], f32)
    r = ClipRef([ppo.InvDecay(0.5)], 3)
    for n in (1, 2, 3):                            # n counts its update! calls, starting at 1
        assert np.array_equal(r.delta(g), (g.astype(f64) * (1 / (1 + 0.5 * n))).astype(f32))
    assert r.m[0]["count"] == 3


def test_clipnorm_by_hand_clip_and_no_clip(ppo):
    g = np.array([3.0, 4.0, 0.5, 0.5, 0.0], f32)  # arrays [0, 2) (norm 5) and [2, 5) (norm sqrt(0.5))
    arrays = [(0, 2), (2, 5)]
    r = ClipRef([ppo.ClipNorm(1.0)], 5, arrays)
    d = r.delta(g)
    assert r.clipped == [[True, False]]
    assert np.array_equal(d[:2], (g[:2].astype(f64) * (1.0 / 5.0)).astype(f32))
    assert np.array_equal(d[2:], g[2:])
    r = ClipRef([ppo.ClipNorm(5.0)], 5, arrays)    # nrm == thresh: not clipped (strictly greater)
    assert np.array_equal(r.delta(g), g) and r.clipped == [[False, False]]
    r = ClipRef([ppo.ClipNorm(0.0)], 5, arrays)    # thresh 0: every non-zero array is scaled to zero
    assert np.all(r.delta(g) == 0) and r.clipped == [[True, True]]


def test_clipnorm_after_adam_uses_adams_output(ppo):
    g = np.array([1.0, -1.0, 2.0, 0.0], f32)
    r = ClipRef([ppo.Adam(0.1), ppo.ClipNorm(0.1)], 4)
    ref = ChainRef([ppo.Adam(0.1)], 4)
    d0 = ref.delta(g)
    nrm = clip_norm_of(d0)
    assert f64(nrm) > 0.1
    assert np.array_equal(r.delta(g), (d0.astype(f64) * (0.1 / f64(nrm))).astype(f32))


def test_zero_gradient_adds_nothing(ppo):
    """Zero-padded hidden units: zero gradient, zero parameter and zero state give D = 0 through every new member."""
    r = ClipRef([ppo.ClipNorm(1e-3), ppo.WeightDecay(0.1), ppo.InvDecay(), ppo.ClipValue(0.5)], 6)
    x = np.zeros(6, f32)
    for _ in range(3):
        x = r.step(x, np.zeros(6, f32))
    assert np.all(x == 0)


# ---------------------------------------------------------------- ClipNorm's sum: the device's order against fsum
def _dd_add(h, l, bh, bl):
    s = h + bh
    if not math.isfinite(s):
        return s, 0.0
    v = s - h
    e = (h - (s - v)) + (bh - v)
    e += l + bl
    h2 = s + e
    return h2, e - (h2 - s)


def _shfl_down_tree(h, l, width):
    h, l = list(h), list(l)
    off = width // 2
    while off >= 1:
        nh, nl = [], []
        for j in range(width):
            src = j + off if j + off < width else j          # out of the segment: the lane's own value
            a = _dd_add(h[j], l[j], h[src], l[src])
            nh.append(a[0])
            nl.append(a[1])
        h, l, off = nh, nl, off // 2
    return h[0], l[0]


def device_sum_of_squares(d):
    """k_chain_clip1 + k_clip_apply on one array (starting at a multiple of 32): per 32 elements the double-double shuffle
    tree, then 256 threads over the slots (strided, 8 per round, (0, 0) past the end), each wave's 64-lane tree, the 4
    waves in order."""
    q = [float(v) * float(v) for v in d.astype(f64)]
    q += [0.0] * (-len(q) % 32)
    slots = [_shfl_down_tree(q[k:k + 32], [0.0] * 32, 32) for k in range(0, len(q), 32)]
    th = []
    for t in range(256):
        h, l = 0.0, 0.0
        for s in range(t, len(slots), 8 * 256):
            for u in range(8):
                v = slots[s + 256 * u] if s + 256 * u < len(slots) else (0.0, 0.0)
                h, l = _dd_add(h, l, v[0], v[1])
        th.append((h, l))
    waves = [_shfl_down_tree([p[0] for p in th[64 * w:64 * w + 64]], [p[1] for p in th[64 * w:64 * w + 64]], 64)
             for w in range(4)]
    H, Lo = waves[0]
    for w in range(1, 4):
        H, Lo = _dd_add(H, Lo, waves[w][0], waves[w][1])
    return H + Lo


@pytest.mark.parametrize("n", [4, 50, 2048, 70000])
def test_device_order_sum_is_the_correctly_rounded_sum(n):
    rng = np.random.default_rng(n)
    for _ in range(3):
        d = _hard_vector(rng, n)
        assert device_sum_of_squares(d) == math.fsum((d.astype(f64) ** 2).tolist())
    d = (rng.normal(size=n) * 1e-3).astype(f32)
    d[0] = 1e4                                     # one large term on top of many small ones
    assert device_sum_of_squares(d) == math.fsum((d.astype(f64) ** 2).tolist())


def test_flux_arrays_layout(ppo):
    assert flux_arrays(72, 128, 2) == [(0, 9216), (9216, 9344), (9344, 25728), (25728, 25856), (25856, 26368),
                                       (26368, 26372)]
    for F, hid, L in ((72, 50, 2), (216, 256, 3), (72, 64, 1)):
        a = flux_arrays(F, hid, L)
        assert len(a) == 2 * L + 2 and a[-1][1] == F * hid + hid + (L - 1) * (hid * hid + hid) + 4 * hid + 4


# ---------------------------------------------------------------- the binding
def test_member_defaults_and_fields(ppo):
    """Flux 0.13 legacy constructors: ClipValue(thresh), ClipNorm(thresh), WeightDecay(wd = 0), InvDecay(gamma = 0.001)."""
    assert ppo.ClipValue(0.5).thresh == 0.5 and ppo.ClipNorm(2).thresh == 2.0
    assert ppo.WeightDecay().wd == 0.0 and ppo.WeightDecay(1e-4).wd == 1e-4
    assert ppo.InvDecay().gamma == 0.001 and ppo.InvDecay(0.5).gamma == 0.5
    for cls in (ppo.ClipValue, ppo.ClipNorm):
        with pytest.raises(TypeError):             # no default thresh, as in Flux
            cls()
    for m in (ppo.ClipValue(1), ppo.ClipNorm(1), ppo.WeightDecay(), ppo.InvDecay()):
        assert not hasattr(m, "eta")


def test_adamw_expansion(ppo):
    o = ppo.AdamW()
    assert isinstance(o, ppo.Optimiser)
    assert [type(m) for m in o.members] == [ppo.Adam, ppo.WeightDecay, ppo.Descent]
    a, w, d = o.members
    assert (a.eta, a.beta, a.epsilon, w.wd, d.eta) == (1.0, (0.9, 0.999), 1e-8, 0.0, 0.001)
    a, w, d = ppo.AdamW(3e-4, (0.8, 0.99), 1e-2).members
    assert (a.eta, a.beta, w.wd, d.eta) == (1.0, (0.8, 0.99), 1e-2, 3e-4)
    with pytest.raises(AttributeError):           # WeightDecay has no eta: the reference's lr printout fails on AdamW
        ppo.get_optimizer_learning_rate(ppo.AdamW())
    kinds, hyper = ppo.AdamW(3e-4, (0.8, 0.99), 1e-2)._check()
    assert kinds.tolist() == [1, 9, 3]
    assert hyper.tolist() == [[1.0, 0.8, 0.99, 1e-8, 0.0], [1e-2, 0, 0, 0, 0], [3e-4, 0, 0, 0, 0]]


def test_check_accepts_the_new_members(ppo):
    opt = ppo.Optimiser(ppo.ClipNorm(0.5), ppo.Adam(1, (0.9, 0.999)), ppo.WeightDecay(1e-4), ppo.Descent(3e-4))
    kinds, hyper = opt._check()
    assert kinds.tolist() == [8, 1, 9, 3]
    assert hyper[0].tolist() == [0.5, 0, 0, 0, 0] and hyper[2].tolist() == [1e-4, 0, 0, 0, 0]
    kinds, hyper = ppo.Optimiser(ppo.ClipValue(2.0), ppo.InvDecay(0.25), ppo.Momentum())._check()
    assert kinds.tolist() == [7, 10, 4] and hyper[0][0] == 2.0 and hyper[1][0] == 0.25
    with pytest.raises(ppo.PPOError, match="appears twice"):
        ppo.Optimiser(ppo.ClipNorm(1.0), ppo.Adam(), ppo.ClipNorm(2.0))._check()


@pytest.mark.parametrize("bad", [-1.0, float("nan")])
def test_thresh_errors_are_arg_errors(ppo, bad):
    for cls in (ppo.ClipNorm, ppo.ClipValue):
        opt = ppo.Optimiser(ppo.Adam(), cls(bad))
        for run in (lambda: ppo.step_batch_(None, opt, None, [1], 0.1, 0.01),
                    lambda: ppo.ppo_train_(None, opt, None, 0.1, 1, 1, 0.01, verbose=False)):
            with pytest.raises(ppo.PPOError, match="thresh") as e:
                run()
            assert e.value.status == -1


def test_learning_rate_mirror_stays_faithful(ppo):
    """get_optimizer_learning_rate iterates opt.eta like the reference, so it fails on a member without one."""
    for m in (ppo.ClipNorm(0.5), ppo.ClipValue(1.0), ppo.WeightDecay(), ppo.InvDecay()):
        with pytest.raises(AttributeError):
            ppo.get_optimizer_learning_rate(ppo.Optimiser(m, ppo.Adam(3e-4)))
    assert ClipRef([ppo.ClipNorm(0.5), ppo.Adam(3e-4), ppo.InvDecay(), ppo.ExpDecay(0.5)], 1).lr() == 3e-4 * 0.5


def test_julia_shim_rows_for_the_new_members():
    src = open(os.path.join(ROOT, "julia", "ProximalPolicyOptimizationHIP.jl")).read()
    for name, kind, field in (("ClipValue", 7, "thresh"), ("ClipNorm", 8, "thresh"), ("WeightDecay", 9, "wd"),
                              ("InvDecay", 10, "gamma")):
        assert "member_row(o::Flux.%s) = (Int32(%d), [Float64(o.%s)" % (name, kind, field) in src, name
    assert ":ppo_optimiser_set_hyper" in src and "hasproperty(o, :eta)" in src
