"""What the action paths can be held to without a device: the binding table, the argument checks, the rule of
tests/path_ref.py on every shape of resample_ref.SHAPES -- the path has best_step entries and replaying it from the start
with step_one gives best_state and best_active exactly -- and that the shapes tests/test_gpu_search_paths.py runs contain
the situations it depends on."""
import numpy as np
import pytest

import episodes_ref as ref
import path_ref as pref
import resample_ref as rref
import search_ref as sref
from test_abi import _header_prototypes

RESULT = ("best_state", "best_active", "best_gap", "best_step", "initial_gap", "best_clone")


def test_binding_table_holds_the_new_symbols(ppo):
    protos, sig, L = _header_prototypes(), ppo._lib.SIGNATURES, ppo._lib
    for new, old in (("ppo_best_states_actions", "ppo_best_states"), ("ppo_search_best_states_path", "ppo_search_best_states"),
                     ("ppo_search_resample_states_path", "ppo_search_resample_states")):
        assert new in sig and new in protos, new
        assert len(sig[new]) == protos[new] == protos[old] + 1
        assert sig[new][:-1] == sig[old] and sig[new][-1] == L.c_i16p, "the plain call's parameters, then the int16 rows"
    assert "ppo_env_apply_paths" in protos and len(sig["ppo_env_apply_paths"]) == protos["ppo_env_apply_paths"] == 12
    assert sig["ppo_env_apply_paths"][5:7] == [L.c_i16p, L.C.c_int64]
    for fn in ("apply_paths_", "check_paths"):
        assert callable(getattr(ppo, fn)) and fn in ppo.__all__, fn
    lib = L.lib()
    for name in ("ppo_best_states_actions", "ppo_search_best_states_path", "ppo_search_resample_states_path",
                 "ppo_env_apply_paths"):
        assert hasattr(lib, name), name


def test_path_argument_checks(ppo):
    got = ppo.check_paths([[1, 128, 0, 0], [5, 0, 7, -3]], 2, 8)
    assert got.dtype == np.int16 and got.flags["C_CONTIGUOUS"]
    assert got.tolist() == [[0, 127, -1, -1], [4, -1, 6, -1]], "1-based in, 0-based out; anything <= 0 is padding"
    assert ppo.check_paths(np.full((3, 1), 512, np.int64), 3, 32).tolist() == [[511]] * 3
    for paths, M, Q in (([[129]], 1, 8), ([[1, 513]], 1, 32),           # an index above 16 Q
                        (np.zeros((2, 0), np.int16), 2, 8),              # stride >= 1
                        ([[1, 2]], 2, 8), ([1, 2], 2, 8),                 # one row per start
                        ([[1.0, 2.0]], 1, 8)):                            # integers
        with pytest.raises(ppo.PPOError) as err:
            ppo.check_paths(paths, M, Q)
        assert err.value.status == -1, (paths, M, Q)
    with pytest.raises(ppo.PPOError) as err:                              # HipVecEnv only
        ppo.apply_paths_(object(), None, None, None, None)
    assert err.value.status == -4


def test_encoding():
    rows = pref.padded([[0, 127], [], [5]], 3)
    assert rows.dtype == np.int16 and rows.tolist() == [[0, 127, -1], [-1, -1, -1], [5, -1, -1]]
    assert pref.one_based(rows).dtype == np.int16 and pref.one_based(rows).tolist() == [[1, 128, 0], [0, 0, 0], [6, 0, 0]]


@pytest.fixture(scope="module")
def refs(orc):
    return {name: pref.resample_reference(orc, name) for name in rref.SHAPES}


def _lengths(r):
    return (r["path"] >= 0).sum(axis=1)


def _closes(orc, env_kw, starts, r):
    """Replaying every start's path gives its result: state, active word, gap, and best_step actions applied."""
    for s in range(starts[2].shape[0]):
        got = pref.apply_path(orc, env_kw, (starts[0][s], starts[1][s], int(starts[2][s])), r["path"][s])
        assert np.array_equal(got["state"], r["best_state"][s]), s
        assert (got["active"], got["gap"], got["applied"]) == (r["best_active"][s], r["best_gap"][s], r["best_step"][s]), s


@pytest.mark.parametrize("name", list(rref.SHAPES))
def test_resample_path_leads_to_the_best_state(orc, refs, name):
    M, K, N, T, R, m0 = rref.SHAPES[name]
    r, want = refs[name], rref.reference(orc, name)
    assert r["path"].shape == (M, T) and r["path"].dtype == np.int16
    n = _lengths(r)
    assert np.array_equal(n, r["best_step"]), "the path has best_step entries"
    assert all((r["path"][s, :n[s]] >= 0).all() and (r["path"][s, n[s]:] == -1).all() for s in range(M)), "-1 behind them only"
    assert (r["path"] < 16 * rref.CASE["Q"]).all()
    _closes(orc, rref.env_kw(rref.SHAPES[name]), sref.search_starts(orc, M), r)
    for k in RESULT + ("donors", "clone_gaps", "tick"):               # the history changes nothing that was there before
        assert np.array_equal(r[k], want[k]), k


def test_shapes_contain_what_the_device_test_needs(orc, refs):
    for name, r in refs.items():
        print(name, rref.SHAPES[name], "fold event", r["fold_event"].tolist(), "copies", r["copies"].tolist(), "path length",
              _lengths(r).tolist(), "best gap", r["best_gap"].tolist())
    # a result taken at an event fold, not the last one, whose lineage crossed at least two copies: every start of shape A
    a = refs["A"]
    assert (a["fold_event"] >= 0).all() and a["copies"].tolist() == [5, 8, 5, 4] and _lengths(a).tolist() == [15, 22, 16, 12]
    # a lineage that crossed at least ten copies
    b = refs["B"]
    assert (int(b["copies"][4]), int(b["copies"][5])) == (11, 12)
    # empty paths
    f = refs["F"]
    assert f["best_step"].tolist()[1:] == [0, 0] and not (f["path"][1:] >= 0).any()
    # a path that ends on a terminal state at gap 0: nothing can be played behind it
    solved = [s for s in range(rref.SHAPES["B"][0]) if b["best_gap"][s] == 0]
    assert solved == [4] and _lengths(b)[4] == 17 < rref.SHAPES["B"][3]
    starts = sref.search_starts(orc, rref.SHAPES["B"][0])
    longer = np.append(b["path"][4, :17], [0, 1, 2]).astype(np.int16)
    assert pref.apply_path(orc, rref.env_kw(rref.SHAPES["B"]), (starts[0][4], starts[1][4], int(starts[2][4])), longer)["applied"] == 17
    # the start of a receiver whose discarded record beats every survivor's: only the fold keeps the path -- at the end no
    # clone of the start holds a history that begins with it
    disc = sorted({(name, ev["start"]) for name in refs for ev in rref.reference(orc, name)["events"]
                   if rref.discarded_record_beats_survivors(ev)})
    assert disc == [("A", 0)]
    p = tuple(int(x) for x in a["path"][0, :_lengths(a)[0]])
    assert not any(h[:len(p)] == p for h in a["final_hist"][0])
    # no event (shape H) and no copy (shape G): the best-of-K search's paths
    assert (refs["H"]["fold_event"] == -1).all() and not refs["H"]["copies"].any() and not refs["G"]["copies"].any()


@pytest.mark.parametrize("shape", sref.SEARCH_SHAPES, ids=lambda s: "M%d-K%d-N%d" % s)
def test_search_path_leads_to_the_best_state(orc, shape):
    M, K, N = shape
    r, want = pref.search_reference(orc, shape), sref.search_reference(orc, shape)
    for k in RESULT:
        assert np.array_equal(r[k], want[k]), k
    assert r["path"].shape == (M, sref.SEARCH_CASE["M"]) and np.array_equal(_lengths(r), r["best_step"])
    _closes(orc, sref.search_env_kw(N), sref.search_starts(orc, M), r)


def test_no_event_is_the_best_of_k_path(orc, refs):
    M, K, N, T, R, m0 = rref.SHAPES["H"]
    want = pref.search_paths(orc, rref.env_kw(rref.SHAPES["H"]), rref.policy_params(orc), rref.CASE["hid"], rref.CASE["L"],
                             sref.search_starts(orc, M), K)
    assert np.array_equal(refs["H"]["path"], want["path"])


@pytest.mark.parametrize("name", sref.COVERAGE_CASES)
def test_trajectory_actions_are_the_replayed_ones(orc, name):
    case = ref.by_name(name)
    rows, rec = pref.trajectory_actions(orc, case), sref.oracle_record(orc, case)
    assert rows.shape == (case["episodes"], case["M"])
    assert np.array_equal((rows >= 0).sum(axis=1), rec["length"])
    # trajectory 0 of env 0 is the column's first: its best_step-prefix leads to its best state
    e = ref._env(orc, ref.env_kw_of(case), 1)
    e.episode[0] = 1
    e.reset()
    got = pref.apply_path(orc, ref.env_kw_of(case), sref.state_of(e, 0), rows[0, :rec["best_step"][0]])
    assert np.array_equal(got["state"], rec["best_state"][0]) and got["gap"] == rec["best_gap"][0]


@pytest.mark.parametrize("name", list(pref.APPLY_CASES))
def test_apply_inputs_hold_the_ragged_rows(orc, name):
    kw, starts, paths = pref.apply_inputs(orc, name)
    T, n = kw["max_actions"], (paths >= 0).sum(axis=1)
    assert paths.shape[1] == pref.APPLY_STRIDE > T
    assert n[0] == 0 and n[1] == pref.APPLY_STRIDE and n[2] == T and 0 < n[3:].min() and len(set(n.tolist())) >= 5
    res = [pref.apply_path(orc, kw, (starts[0][i], starts[1][i], int(starts[2][i])), paths[i]) for i in range(len(n))]
    applied = np.array([r["applied"] for r in res])
    assert np.array_equal(applied, np.minimum(n, T)), "no start is solved on the way: the time limit alone cuts a path"
    assert applied[1] == T < n[1], "entries behind a terminal state"
    assert res[0]["gap"] == sref.score_gap(starts[0][0], int(starts[2][0]))[1] and res[0]["trace"] == []
