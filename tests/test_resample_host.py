"""What the resampling search can be held to without a device: the binding table, the argument checks, the rule on small
hand-made inputs, and that the shapes tests/test_gpu_resample.py runs really contain the situations it depends on (the
reference is tests/resample_ref.py)."""
import numpy as np
import pytest

import resample_ref as rref
import search_ref as sref
from test_abi import _header_prototypes


def test_binding_table_holds_the_new_symbol(ppo):
    protos = _header_prototypes()
    name = "ppo_search_resample_states"
    assert name in ppo._lib.SIGNATURES and name in protos
    assert len(ppo._lib.SIGNATURES[name]) == protos[name] == protos["ppo_search_best_states"] + 3
    # the parameter order of ppo_search_best_states, then interval, survivors, donors_or_null
    assert ppo._lib.SIGNATURES[name][:-3] == ppo._lib.SIGNATURES["ppo_search_best_states"]
    assert ppo._lib.SIGNATURES[name][-3:] == [ppo._lib.C.c_int64, ppo._lib.C.c_int64, ppo._lib.c_i32p]
    for fn in ("search_resample_states_", "check_resample"):
        assert callable(getattr(ppo, fn)) and fn in ppo.__all__, fn


def test_argument_checks(ppo):
    assert ppo.check_resample(48, 12, 2, 3) == (12, 2, 3)
    assert ppo.check_resample(3, 1, 1, 1) == (1, 1, 1)
    assert ppo.check_resample(64, 16, 1000, 16) == (16, 1000, 16)
    for N, K, R, m0 in ((48, 12, 0, 3), (48, 12, -1, 3),             # interval >= 1
                        (48, 12, 2, 0), (48, 12, 2, 13),              # 1 <= survivors <= K
                        (48, 0, 2, 1), (48, 49, 2, 3), (8192, 8193, 1, 1)):   # 1 <= K <= N
        with pytest.raises(ppo.PPOError) as err:
            ppo.check_resample(N, K, R, m0)
        assert err.value.status == -1, (N, K, R, m0)
    assert ppo.check_resample(8192, 4096, 1, 1) == (4096, 1, 1)
    with pytest.raises(ppo.PPOError) as err:
        ppo.check_resample(8192, 4097, 1, 1)
    assert err.value.status == -4
    with pytest.raises(ppo.PPOError) as err:                          # HipVecEnv only
        ppo.search_resample_states_(object(), None, None, None, None, 1, 1, 1)
    assert err.value.status == -4


def test_rank_rule():
    # clones 1 and 4 are terminal; live by (gap, clone): 3 (2), 0 (5), 2 (5), 5 (5), 6 (9)
    cur, done = [5, 0, 5, 2, 0, 5, 9], [0, 1, 0, 0, 1, 0, 0]
    order, m, donor_of = rref.rank_live(cur, done, 2)
    assert order == [3, 0, 2, 5, 6] and m == 2
    assert donor_of == {2: 3, 5: 0, 6: 3}                             # rank rho >= m takes rank (rho - m) % m
    assert rref.cut_between_equals(dict(order=order, m=m, cur_gap=cur))
    order, m, donor_of = rref.rank_live(cur, done, 7)                 # m = min(m0, live): everyone survives
    assert m == 5 and donor_of == {}
    order, m, donor_of = rref.rank_live([3, 1], [1, 1], 1)            # no live clone
    assert order == [] and m == 0 and donor_of == {}
    order, m, donor_of = rref.rank_live([4, 4, 4, 4], [0, 0, 0, 0], 1)
    assert donor_of == {1: 0, 2: 0, 3: 0}


def test_fold_rule():
    rec = lambda g: dict(best_gap=g, best_step=0)
    r = rref.fold_into(None, [rec(6), rec(4), rec(4)])
    assert (r["best_gap"], r["best_clone"]) == (4, 1)                 # ties to the lowest clone
    r2 = rref.fold_into(r, [rec(4), rec(5), rec(9)])
    assert r2 is r                                                    # an equal gap does not replace: the earlier fold keeps a tie
    r3 = rref.fold_into(r, [rec(7), rec(5), rec(3)])
    assert (r3["best_gap"], r3["best_clone"]) == (3, 2)


@pytest.fixture(scope="module")
def refs(orc):
    return {name: rref.reference(orc, name) for name in rref.SHAPES}


def test_shapes_contain_what_the_device_test_needs(refs):
    count = lambda name, pred: sum(1 for ev in refs[name]["events"] if pred(ev))
    for name, r in refs.items():
        print(name, rref.SHAPES[name], "events", len(r["events"]), "cut between equals", count(name, rref.cut_between_equals),
              "terminal among live", count(name, rref.terminal_among_live), "discarded record beats survivors",
              count(name, rref.discarded_record_beats_survivors), "best", r["best_gap"].tolist(), "without the folds",
              r["nofold"]["best_gap"].tolist())
    total = lambda pred: sum(count(name, pred) for name in refs)
    assert total(rref.cut_between_equals) >= 1
    assert count("B", rref.terminal_among_live) >= 1
    assert total(rref.discarded_record_beats_survivors) >= 1
    # the fold decides a result: the last fold alone ends elsewhere
    differ = [(name, s) for name, r in refs.items() for s in range(rref.SHAPES[name][0])
              if r["best_gap"][s] != r["nofold"]["best_gap"][s]]
    assert ("A", 0) in differ and refs["A"]["best_gap"][0] < refs["A"]["nofold"]["best_gap"][0]
    # a start solved to gap 0 in shape B
    assert (refs["B"]["best_gap"] == 0).any()
    # four rounds, the last one ragged; idle envs never play
    M, K, N = rref.SHAPES["D"][:3]
    assert -(-M // (N // K)) == 4 and M % (N // K) != 0
    assert not refs["C"]["tick"][65:].any() and not refs["C"]["played"][65:].any() and refs["C"]["played"][:65].all()


def test_records_are_consistent(refs):
    for name, r in refs.items():
        M, K, N, T, R, m0 = rref.SHAPES[name]
        assert r["donors"].shape == (M, (T - 1) // R, K)
        assert (r["best_gap"] <= r["initial_gap"]).all() and (r["best_gap"] >= 0).all()
        assert (r["best_gap"] <= r["nofold"]["best_gap"]).all(), "the event folds can only keep more"
        assert (r["best_gap"] <= r["clone_gaps"].min(axis=1)).all()
        assert ((r["best_step"] >= 0) & (r["best_step"] <= T)).all()
        for s in range(M):
            V = r["best_state"].shape[1] // 2
            assert sref.score_gap(r["best_state"][s, :V], int(r["best_active"][s]))[1] == r["best_gap"][s]
        for ev in r["events"]:
            row = r["donors"][ev["start"], ev["event"]]
            live = [c for c in range(K) if not ev["done"][c]]
            assert sorted(live) == sorted(ev["order"]) and ev["m"] == min(m0, len(live))
            assert all((row[c] == -2) == bool(ev["done"][c]) for c in range(K))
            receivers = [c for c in range(K) if row[c] >= 0]
            assert receivers == sorted(ev["donor_of"]) and all(row[c] in ev["order"][:ev["m"]] for c in receivers)
            assert not set(receivers) & set(int(row[c]) for c in receivers), "donors are never receivers"
        if m0 == K:
            assert not (r["donors"] >= 0).any()


def test_no_event_is_the_best_of_k_search(orc, refs):
    """R = max_actions: every output equals search_ref.search_replay, field for field."""
    M, K, N, T, R, m0 = rref.SHAPES["H"]
    assert R >= T and rref.SHAPES["H"][:4] == rref.SHAPES["C"][:4]
    got = refs["H"]
    want = sref.search_replay(orc, rref.env_kw(rref.SHAPES["H"]), rref.policy_params(orc), rref.CASE["hid"], rref.CASE["L"],
                              sref.search_starts(orc, M), K)
    assert not got["events"] and got["donors"].size == 0
    for k in ("best_state", "best_active", "best_gap", "best_clone", "best_step", "initial_gap", "clone_gaps", "tick"):
        assert np.array_equal(got[k], want[k]), k
        if k in got["nofold"]:
            assert np.array_equal(got["nofold"][k], want[k]), k


def test_survivors_equal_k_copies_nothing(orc, refs):
    """survivors == K: best_gap and initial_gap are the best-of-K search's (best_clone may differ: an earlier fold keeps a tie)."""
    M, K, N, T, R, m0 = rref.SHAPES["G"]
    got = refs["G"]
    want = sref.search_replay(orc, rref.env_kw(rref.SHAPES["G"]), rref.policy_params(orc), rref.CASE["hid"], rref.CASE["L"],
                              sref.search_starts(orc, M), K)
    for k in ("best_gap", "initial_gap", "clone_gaps", "tick"):
        assert np.array_equal(got[k], want[k]), k
