"""Flux.Optimiser chains (Adam, ExpDecay, Descent, Momentum, Nesterov, RMSProp; include/ppo_hip.h ppo_optimiser_create),
CPU side: a numpy restatement of the arithmetic contract of Flux 0.13's legacy Flux.Optimise (Float64 hyper-parameters
against Float32 arrays: float64 wherever a float64 operand enters, float32 on every store), anchored where the repository
has an independent answer (Adam: the C oracle's adam_step, bit for bit; ExpDecay: an emulation of Flux's IdDict counter);
get_optimizer_learning_rate on chains; and the chains the binding refuses before any library call.

ChainRef is also the reference of tests/test_gpu_optimiser_chain.py, which replays the device's training step by step."""
import numpy as np
import pytest

f32, f64 = np.float32, np.float64


# ---------------------------------------------------------------- the restatement: one function per member
def adam_apply(st, d, eta, beta1, beta2, eps):
    dd = d.astype(f64)
    mn = (beta1 * st["m"].astype(f64) + (1.0 - beta1) * dd).astype(f32)
    vn = (beta2 * st["v"].astype(f64) + ((1.0 - beta2) * dd) * dd).astype(f32)
    st["m"], st["v"] = mn, vn
    bp = st["beta_pow"]
    out = (mn.astype(f64) / (1.0 - bp[0]) / (np.sqrt(vn.astype(f64) / (1.0 - bp[1])) + eps) * eta).astype(f32)
    st["beta_pow"] = np.array([bp[0] * beta1, bp[1] * beta2], f64)
    return out


def expdecay_eta(st, decay, step, clip, start):
    """Advance ExpDecay's update count; decay first when on schedule (Flux: exactly one array's counter on schedule)."""
    st["count"] += 1
    n = st["count"]
    if n > start and n % step == 0 and (step > 1 or n == start + 1 or n == 1):
        st["eta"] = max(st["eta"] * decay, clip)
    return st["eta"]


def scale_apply(d, eta):                        # Descent, and ExpDecay with its eta of this step
    return (d.astype(f64) * eta).astype(f32)


def momentum_apply(st, d, eta, rho):
    v = (rho * st["velocity"].astype(f64) - eta * d.astype(f64)).astype(f32)
    st["velocity"] = v
    return -v


def nesterov_apply(st, d, eta, rho):
    v0, dd = st["velocity"].astype(f64), d.astype(f64)
    dn = (rho * rho) * v0 - ((1.0 + rho) * eta) * dd
    st["velocity"] = (rho * v0 - eta * dd).astype(f32)
    return (-dn).astype(f32)


def rmsprop_apply(st, d, eta, rho, eps):
    dd = d.astype(f64)
    acc = (rho * st["acc"].astype(f64) + ((1.0 - rho) * dd) * dd).astype(f32)
    st["acc"] = acc
    return (dd * (eta / (np.sqrt(acc).astype(f64) + eps))).astype(f32)     # sqrt of the Float32 array: a float32 root


class ChainRef:
    """Flux.update!(Optimiser(members...), params, grads) on the flat parameter vector: D = g, each member's apply! in
    chain order, x -= D.  Built from the package's member objects (their hyper-parameters at construction)."""

    def __init__(self, members, n):
        self.m = []
        for o in members:
            k = type(o).__name__
            st = {"kind": k, "o": o, "eta": float(o.eta)}
            if k == "Adam":
                st.update(m=np.zeros(n, f32), v=np.zeros(n, f32), beta_pow=np.array(o.beta, f64))
            elif k in ("Momentum", "Nesterov"):
                st["velocity"] = np.zeros(n, f32)
            elif k == "RMSProp":
                st["acc"] = np.zeros(n, f32)
            elif k == "ExpDecay":
                st["count"] = 0
            self.m.append(st)

    def delta(self, g):
        d = np.asarray(g, f32).copy()
        for st in self.m:
            o, k = st["o"], st["kind"]
            if k == "Adam":
                d = adam_apply(st, d, st["eta"], o.beta[0], o.beta[1], o.epsilon)
            elif k == "ExpDecay":
                d = scale_apply(d, expdecay_eta(st, o.decay, o.step, o.clip, o.start))
            elif k == "Descent":
                d = scale_apply(d, st["eta"])
            elif k == "Momentum":
                d = momentum_apply(st, d, st["eta"], o.rho)
            elif k == "Nesterov":
                d = nesterov_apply(st, d, st["eta"], o.rho)
            elif k == "RMSProp":
                d = rmsprop_apply(st, d, st["eta"], o.rho, o.epsilon)
            else:
                raise AssertionError(k)
        return d

    def step(self, params, g):
        return (np.asarray(params, f32) - self.delta(g)).astype(f32)

    def lr(self):
        p = 1.0
        for st in self.m:
            p *= st["eta"]
        return p


# ---------------------------------------------------------------- anchors
def _hard_vector(rng, n):
    """Gradients with zeros, float32 denormals, large values and ordinary ones."""
    g = (rng.normal(size=n) * 10.0 ** rng.integers(-6, 3, size=n)).astype(f32)
    g[::7] = 0.0
    g[1::11] = (rng.normal(size=g[1::11].size) * 1e-40).astype(f32)        # denormal
    g[2::13] = (rng.normal(size=g[2::13].size) * 1e30).astype(f32)
    g[3::17] = -0.0
    return g


@pytest.mark.parametrize("eta,b1,b2,eps", [(1e-4, 0.9, 0.999, 1e-8), (3e-3, 0.5, 0.99, 1e-6)])
def test_adam_restatement_matches_oracle_bitwise(ppo, orc, eta, b1, b2, eps):
    rng = np.random.default_rng(11)
    n = 4099
    p_ref = (rng.normal(size=n) * 0.1).astype(f32)
    p_orc, m, v, bp = p_ref.copy(), np.zeros(n, f32), np.zeros(n, f32), np.array([b1, b2], f64)
    ref = ChainRef([ppo.Adam(eta, (b1, b2), eps)], n)
    for _ in range(6):
        g = _hard_vector(rng, n)
        orc.adam_step(p_orc, g, m, v, bp, eta, b1, b2, eps)
        with np.errstate(over="ignore"):         # (1e30)^2 stores inf into v, on both sides
            p_ref = ref.step(p_ref, g)
        st = ref.m[0]
        assert np.array_equal(p_ref.view(np.uint32), p_orc.view(np.uint32))
        assert np.array_equal(st["m"].view(np.uint32), m.view(np.uint32))
        assert np.array_equal(st["v"].view(np.uint32), v.view(np.uint32))
        assert np.array_equal(st["beta_pow"], bp)


def _flux_expdecay(eta, decay, step, clip, start, steps, arrays=6):
    """Flux 0.13 apply!(::ExpDecay) literally, over `arrays` parameter arrays per update! (an IdDict of counters): the
    eta every array of each step was scaled with."""
    current, out = {}, []
    for _ in range(steps):
        used = []
        for x in range(arrays):
            n = current[x] = current.get(x, 0) + 1
            if n > start and n % step == 0 and sum(1 for c in current.values() if c > start and c % step == 0) == 1:
                eta = max(eta * decay, clip)
            used.append(eta)
        assert len(set(used)) == 1               # every array of a step sees the same eta
        out.append(used[0])
    return out


# (eta, decay, decay_step, clip, start, steps) -> the eta of steps 1..steps
SCHEDULE = [
    ((1.0, 0.5, 3, 1e-6, 0, 10), [1, 1, .5, .5, .5, .25, .25, .25, .125, .125]),
    ((1.0, 0.5, 1, 1e-6, 0, 5), [.5, .5, .5, .5, .5]),                       # decay_step 1: decays ONCE
    ((1.0, 0.5, 1, 1e-6, 3, 6), [1, 1, 1, .5, .5, .5]),                      # ... at the first step past start
    ((1.0, 0.5, 2, 1e-6, 3, 9), [1, 1, 1, .5, .5, .25, .25, .125, .125]),    # start > 0: steps 4, 6, 8
    ((1.0, 0.1, 2, 0.05, 0, 8), [1, .1, .1, .05, .05, .05, .05, .05]),       # clipped at 0.05
    ((1e-3, 0.1, 1000, 1e-4, 0, 3), [1e-3, 1e-3, 1e-3]),                     # Flux defaults
]


@pytest.mark.parametrize("args,expect", SCHEDULE, ids=["s%d" % i for i in range(len(SCHEDULE))])
def test_expdecay_schedule(ppo, args, expect):
    eta, decay, step, clip, start, steps = args
    ref = ChainRef([ppo.ExpDecay(eta, decay, step, clip, start)], 1)
    got = []
    for _ in range(steps):
        ref.delta(np.ones(1, f32))
        got.append(ref.m[0]["eta"])
    assert np.allclose(got, expect, rtol=1e-15, atol=0)
    assert got == _flux_expdecay(eta, decay, step, clip, start, steps)


def test_expdecay_rule_matches_flux_counter():
    rng = np.random.default_rng(3)
    for _ in range(200):
        step, start, steps = int(rng.integers(1, 5)), int(rng.integers(-2, 6)), int(rng.integers(1, 20))
        st = {"eta": 1.0, "count": 0}
        mine = [expdecay_eta(st, 0.5, step, 1e-3, start) for _ in range(steps)]
        assert mine == _flux_expdecay(1.0, 0.5, step, 1e-3, start, steps), (step, start, steps)


def test_members_by_hand(ppo):
    """Each member's first two steps on small numbers, written out in float64 and rounded like the contract says."""
    g1, g2 = np.array([0.5, -2.0, 0.0], f32), np.array([0.25, 1.0, 0.0], f32)
    G1, G2 = g1.astype(f64), g2.astype(f64)
    r = ChainRef([ppo.Momentum(0.1, 0.9)], 3)
    v1 = (-0.1 * G1).astype(f32)
    assert np.array_equal(r.delta(g1), -v1)
    v2 = (0.9 * v1.astype(f64) - 0.1 * G2).astype(f32)
    assert np.array_equal(r.delta(g2), -v2)
    r = ChainRef([ppo.Nesterov(0.1, 0.9)], 3)
    assert np.array_equal(r.delta(g1), (((1 + 0.9) * 0.1) * G1).astype(f32))
    assert np.array_equal(r.delta(g2), (-((0.9 * 0.9) * v1.astype(f64) - ((1 + 0.9) * 0.1) * G2)).astype(f32))
    r = ChainRef([ppo.RMSProp(0.01, 0.9, 1e-8)], 3)
    a1 = (((1 - 0.9) * G1) * G1).astype(f32)
    assert np.array_equal(r.delta(g1), (G1 * (0.01 / (np.sqrt(a1).astype(f64) + 1e-8))).astype(f32))
    r = ChainRef([ppo.Descent(0.3), ppo.ExpDecay(2.0, 0.5, 1, 1e-6, 0)], 3)
    assert np.array_equal(r.delta(g1), ((G1 * 0.3).astype(f32).astype(f64) * 1.0).astype(f32))
    assert r.lr() == 0.3 * 1.0


def test_zero_gradient_never_moves(ppo):
    """Zero gradient with zero state gives D = 0 for every member (zero-padded hidden units stay zero)."""
    chain = [ppo.Adam(1e-3), ppo.Momentum(), ppo.Nesterov(), ppo.RMSProp()]
    for perm in ([0, 1, 2, 3], [3, 2, 1, 0]):
        r = ChainRef([chain[i] for i in perm] + [ppo.ExpDecay()], 5)
        x = np.zeros(5, f32)
        for _ in range(3):
            x = r.step(x, np.zeros(5, f32))
        assert np.all(x == 0)


# ---------------------------------------------------------------- the binding
def test_learning_rate_of_chains(ppo):
    opt = ppo.Optimiser(ppo.Adam(1e-4), ppo.ExpDecay(1.0, 0.5, 1000, 1e-6))
    assert ppo.get_optimizer_learning_rate(opt) == 1e-4
    opt = ppo.Optimiser(ppo.Descent(0.1), ppo.Momentum(0.01, 0.9), ppo.ExpDecay(0.5))
    assert ppo.get_optimizer_learning_rate(opt) == (1.0 * 0.1) * 0.01 * 0.5
    opt.members[0].eta = 0.2                     # Flux lets the user assign eta
    assert ppo.get_optimizer_learning_rate(opt) == (1.0 * 0.2) * 0.01 * 0.5
    for m in (ppo.Descent(), ppo.ExpDecay(), ppo.Momentum(), ppo.Nesterov(), ppo.RMSProp()):
        with pytest.raises(TypeError):           # a bare member is not iterable, like the reference
            ppo.get_optimizer_learning_rate(m)


def test_member_defaults(ppo):
    """Flux 0.13 legacy constructor defaults and field names."""
    e = ppo.ExpDecay()
    assert (e.eta, e.decay, e.step, e.clip, e.start) == (1e-3, 0.1, 1000, 1e-4, 0)
    assert ppo.Descent().eta == 0.1
    assert (ppo.Momentum().eta, ppo.Momentum().rho) == (0.01, 0.9)
    assert (ppo.Nesterov().eta, ppo.Nesterov().rho) == (1e-3, 0.9)
    r = ppo.RMSProp()
    assert (r.eta, r.rho, r.epsilon) == (1e-3, 0.9, 1e-8)


class ClipNorm:                                  # stand-ins of Flux's members without eta
    def __init__(self, thresh=10.0):
        self.thresh = thresh


class WeightDecay:
    def __init__(self, wd=0.0):
        self.wd = wd


class InvDecay:
    def __init__(self, gamma=0.001):
        self.gamma = gamma


class AMSGrad:                                   # has eta, but is not a member the device runs
    def __init__(self, eta=1e-3):
        self.eta = eta


def _refused(ppo, opt, match):
    """Every entry point refuses the chain with PPO_ERR_UNSUPPORTED before it touches the (absent) policy or library."""
    for run in (lambda: ppo.step_batch_(None, opt, None, [1], 0.1, 0.01),
                lambda: ppo.ppo_train_(None, opt, None, 0.1, 1, 1, 0.01, verbose=False),
                lambda: ppo.step_epoch_(None, opt, None, 0.1, 1, 0.01)):
        with pytest.raises(ppo.PPOError, match=match) as e:
            run()
        assert e.value.status == -4


def test_refused_chains(ppo):
    _refused(ppo, ppo.Optimiser(ppo.Adam(), ClipNorm()), "ClipNorm has no eta")
    _refused(ppo, ppo.Optimiser(WeightDecay(), ppo.Adam()), "WeightDecay has no eta")
    _refused(ppo, ppo.Optimiser(InvDecay()), "InvDecay has no eta")
    _refused(ppo, ppo.Optimiser(ppo.Optimiser(ppo.Adam())), "Optimiser has no eta")   # nested; AdamW is such a composite
    _refused(ppo, ppo.Optimiser(ppo.Descent(), AMSGrad()), "AMSGrad is not supported")
    _refused(ppo, ppo.Optimiser(ppo.Adam(), ppo.ExpDecay(), ppo.Adam()), "Adam appears twice")
    _refused(ppo, ppo.Optimiser(ppo.Descent(), ppo.Descent()), "Descent appears twice")
    _refused(ppo, ppo.Optimiser(ppo.Adam(), ppo.ExpDecay(), ppo.Descent(), ppo.Momentum(), ppo.RMSProp()), "1 to 4 members")
    _refused(ppo, ppo.Optimiser(), "1 to 4 members")


def test_bare_member_is_not_an_optimiser(ppo):
    with pytest.raises(AttributeError):          # as before: the training entry points take the composite
        ppo.step_batch_(None, ppo.Adam(), None, [1], 0.1, 0.01)
