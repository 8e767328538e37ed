"""The rule of the value-ranked resampling search without a device: tests/value_resample_ref.py replayed with
value_ref.values_np(..., float32) as the stand-in critic.

1. unit properties of the rule: ord is monotone (+-0, denormals, infinities), the one-rounding fma, value_weight = 0 is 7h's
   ranking, a value that is not finite ranks as 0;
2. the inputs of tests/test_gpu_value_resample.py hold the situations that matter -- conditions on the inputs, checked on the
   reference alone: in at least a third of the events the survivors differ from the ones (cur_gap, clone) keeps, an event keeps
   a clone whose cur_gap is strictly higher than a discarded one's, terminal clones beside live ones, a start that takes its
   result at an event fold;
3. value_weight = 0 replays resample_ref's and path_ref's references exactly;
4. the header, the binding table and the Python signature carry the feature."""
import inspect
import os
from fractions import Fraction

import numpy as np
import pytest

import path_ref as pref
import resample_ref as rref
import search_ref as sref
import value_resample_ref as vref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- 1. the rule
def _sweep():
    tiny = np.float32(1e-45)                                     # the smallest denormal
    xs = [-np.inf, -3.4e38, -1e10, -7.5, -1.0, -1e-30, -1.2e-38, -1e-40, -tiny, -0.0, 0.0, tiny, 1e-40, 1.2e-38, 1e-30, 0.5, 1.0,
          1.0000001, 2.0, 1e10, 3.4e38, np.inf]
    rng = np.random.default_rng(0)
    more = rng.integers(0, 2 ** 32, size=4000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    more = more[~np.isnan(more)]
    return np.asarray(xs, np.float32), more


def test_ord_is_monotone():
    xs, more = _sweep()
    o = vref.ord32(xs).astype(np.int64)
    assert np.all(np.diff(o) > 0), "strictly increasing over the ordered sweep, -0.0 before +0.0"
    assert vref.ord32(np.float32(-0.0)) + 1 == vref.ord32(np.float32(0.0))
    srt = more[np.argsort(vref.ord32(more), kind="stable")]
    assert np.all(np.diff(srt.astype(np.float64)) >= 0), "sorting by ord sorts the floats"
    a, b = more[:-1], more[1:]
    assert np.array_equal(vref.ord32(a) < vref.ord32(b), (a < b) | ((a == 0) & (b == 0) & np.signbit(a) & ~np.signbit(b)))
    assert int(vref.ord32(np.float32(np.inf))) < 0xFFFFFFFF, "no score of a live clone maps to the terminal key"


def test_score_is_one_rounding():
    # 1 + 2^-24 + 2^-60 lies just above the midpoint of 1 and 1 + 2^-23: one rounding goes up, rounding through float64
    # (which drops the 2^-60 first) goes to the even neighbour 1.0
    q = Fraction(1) + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 60)
    assert vref.round_f32(q) == np.float32(1.0) + np.float32(2.0 ** -23)
    assert vref.round_f32(Fraction(1) + Fraction(1, 2 ** 24)) == np.float32(1.0), "a tie goes to the even mantissa"
    assert vref.round_f32(Fraction(0)) == 0.0 and not np.signbit(vref.round_f32(Fraction(0)))
    assert np.isinf(vref.round_f32(Fraction(2) ** 128)) and vref.round_f32(-Fraction(2) ** 128) < 0
    rng = np.random.default_rng(1)
    for _ in range(300):                                         # where float64 holds the sum exactly, it is the reference
        v, w, g = np.float32(rng.normal()), np.float32(rng.integers(0, 9)), int(rng.integers(0, 40))
        assert vref.score(g, v, w) == np.float32(np.float64(g) - np.float64(w) * np.float64(v))
    assert vref.score(3, np.float32(0.75), 4.0) == 0.0 and not np.signbit(vref.score(3, np.float32(0.75), 4.0))


def test_weight_zero_is_gap_ranking():
    rng = np.random.default_rng(2)
    for _ in range(50):
        K = int(rng.integers(1, 20))
        cur = [int(x) for x in rng.integers(0, 6, size=K)]
        done = [int(x) for x in rng.random(K) < 0.25]
        vals = rng.normal(size=K).astype(np.float32) * 100
        m0 = int(rng.integers(1, K + 1))
        order, m, donor_of, s = vref.rank_live_value(cur, vals, done, m0, 0.0)
        assert (order, m, donor_of) == rref.rank_live(cur, done, m0)
        assert all(s[c] == cur[c] for c in order)


def test_non_finite_value_ranks_as_zero():
    cur, done = [5, 3, 4, 4, 2], [0, 0, 0, 0, 1]
    for bad in (np.nan, np.inf, -np.inf):
        vals = np.array([1.0, bad, 1.0, -0.25, 9.0], np.float32)
        zero = np.where(np.isfinite(vals), vals, 0).astype(np.float32)
        got = vref.rank_live_value(cur, vals, done, 2, 2.0)
        want = vref.rank_live_value(cur, zero, done, 2, 2.0)
        assert got[:3] == want[:3] and np.array_equal(got[3], want[3], equal_nan=True)
        assert got[3][1] == 3.0 and got[0] == [2, 0, 1, 3]       # s = 3, 3, 2, 4.5: clones 0 and 1 tie, the index decides
    order = vref.rank_live_value([0, 0], np.array([0.0, -0.0], np.float32), [0, 0], 1, 1.0)[0]
    assert order == [0, 1], "fmaf(-1, +-0, +0) is +0 for both: the clone index decides"


# ---------------------------------------------------------------- 2. the situations the device test depends on
@pytest.mark.parametrize("name", list(vref.SHAPES))
def test_shapes_hold_what_matters(orc, name):
    M, K, N, T, R, m0 = vref.SHAPES[name]["shape"]
    want = vref.host_reference(orc, name)
    evs = want["events"]
    ran = [e for e in evs if e["order"]]
    differ = sum(vref.differs_from_gap_ranking(e) for e in ran)
    higher = sum(vref.keeps_a_higher_gap(e) for e in ran)
    mixed = sum(vref.terminal_among_live(e) for e in evs)
    at_event = int((want["fold_event"] >= 0).sum())
    print(name, vref.SHAPES[name], "events with live clones", len(ran), "survivors differ", differ, "keeps a higher gap", higher,
          "terminal beside live", mixed, "results taken at an event fold", at_event, "best", want["best_gap"].tolist())
    assert 3 * differ >= len(ran) > 0, "in at least a third of the events the survivors are not the gap ranking's"
    assert higher >= 1, "an event keeps a clone whose cur_gap is strictly higher than a discarded one's"


def test_some_shape_has_terminal_clones_and_an_event_fold(orc):
    mixed = {n: sum(vref.terminal_among_live(e) for e in vref.host_reference(orc, n)["events"]) for n in vref.SHAPES}
    at_event = {n: int((vref.host_reference(orc, n)["fold_event"] >= 0).sum()) for n in vref.SHAPES}
    print("terminal beside live", mixed, "results taken at an event fold", at_event)
    assert max(mixed.values()) >= 1 and max(at_event.values()) >= 1


def test_non_finite_critic_gives_every_kind_of_value(orc):
    """The critic of the device test's non-finite case, as the float32 stand-in: +inf, NaN and finite values among the live
    clones of shape A, and every value that is not finite ranked as 0."""
    import episodes_ref as ref
    import value_ref
    hid, L = vref.NON_FINITE["critic"]
    p = vref.non_finite_critic_params(orc)
    with np.errstate(all="ignore"):
        got = vref.replay(orc, "A", lambda start, ev, states, active, done: value_ref.values_np(p, ref.F, hid, L, states, active,
                                                                                              np.float32))
    live = np.concatenate([e["values"][e["order"]] for e in got["events"] if e["order"]])
    print("live values", live.size, "NaN", int(np.isnan(live).sum()), "inf", int(np.isinf(live).sum()))
    assert np.isnan(live).any() and np.isinf(live).any() and 4 * np.isfinite(live).sum() >= live.size
    assert all(e["s"][c] == e["cur_gap"][c] for e in got["events"] for c in e["order"] if not np.isfinite(e["values"][c]))


def test_reference_is_consistent(orc):
    """What the replay returns obeys the rule's invariants: donors are survivors, a path has best_step entries and replays to
    best_state, the log of survivors matches the donors rows."""
    name = "A"
    M, K, N, T, R, m0 = vref.SHAPES[name]["shape"]
    want, st = vref.host_reference(orc, name), vref.starts(orc, name)
    for e in want["events"]:
        row = want["donors"][e["start"], e["event"]]
        assert set(np.flatnonzero(row == -1)) == e["survivors"] and np.isin(row[row >= 0], list(e["survivors"])).all()
        assert all(np.isnan(e["s"][c]) == bool(e["done"][c]) for c in range(K))
    for s in range(M):
        back = pref.apply_path(orc, vref.env_kw(name), (st[0][s], st[1][s], int(st[2][s])), want["path"][s])
        assert np.array_equal(back["state"], want["best_state"][s]) and back["applied"] == want["best_step"][s]
        assert back["gap"] == want["best_gap"][s]


# ---------------------------------------------------------------- 3. weight 0 is 7h / 7i
@pytest.mark.parametrize("name", ["A", "C"])
def test_weight_zero_replays_the_plain_references(orc, name):
    assert vref.SHAPES[name]["shape"] == rref.SHAPES[name] and vref.SHAPES[name]["Q"] == rref.CASE["Q"]
    st = vref.starts(orc, name)
    assert all(np.array_equal(a, b) for a, b in zip(st, sref.search_starts(orc, st[2].shape[0])))
    got = vref.replay(orc, name, vref.host_values(orc, name), w=0.0)
    old, paths = rref.reference(orc, name), pref.resample_reference(orc, name)
    for k in ("best_state", "best_active", "best_gap", "best_step", "initial_gap", "best_clone", "donors", "clone_gaps", "tick"):
        assert np.array_equal(got[k], old[k]), k
    assert np.array_equal(got["path"], paths["path"]) and np.array_equal(got["fold_event"], paths["fold_event"])


# ---------------------------------------------------------------- 4. the interface
def test_interface_carries_the_feature(ppo):
    name = "ppo_search_resample_states_value"
    assert name in ppo._lib.SIGNATURES and len(ppo._lib.SIGNATURES[name]) == 22
    assert name in open(os.path.join(ROOT, "include", "ppo_hip.h")).read()
    assert "search_resample_states_value" in open(os.path.join(ROOT, "julia", "ProximalPolicyOptimizationHIP.jl")).read()
    par = inspect.signature(ppo.search_resample_states_).parameters
    assert par["critic"].default is None and par["value_weight"].default == 1.0 and par["values"].default is False
    with pytest.raises(ppo.PPOError) as err:                     # refused before anything touches a device
        ppo.search_resample_states_(object(), None, None, None, None, 1, 1, 1, critic=None, values=True)
    assert err.value.status == -4
