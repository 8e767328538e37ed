"""The advantage-mode device tests (tests/test_gpu_advantage_modes.py), the part that needs no device: the inputs those cases
run on have, judged on the float64 restatement alone, the properties the cases rest on; and the restatements themselves."""
import numpy as np
import pytest

import advantage_modes_ref as ref


_ROLLOUT = []


def _compact_case(orc, fam):
    """The engine rollout of the compact-storage families on the CPU oracle (bit for bit the device's: test_rollout_bitexact)."""
    c, r = ref.FAMILIES[fam], ref.ROLLOUT
    p0, moved = ref.rollout_start()
    if not _ROLLOUT:
        env = orc.Env(Q=r["Q"], max_actions=r["max_actions"], N=r["N"], seed=r["env_seed"])
        env.reset()
        _ROLLOUT.append(orc.collect_rollouts_tn(env, p0, r["hid"], r["T"], mode_dev=True))
    ro = _ROLLOUT[0]
    n = r["N"] * r["T"]
    R = orc.compute_returns_tn(ro["rewards"], ro["done"], r["discount"])
    d = ref.compact_case(fam, moved, ro["states"].reshape(n, 32, c["F"]), ro["active"].reshape(n), ro["actions"].reshape(n),
                         ro["p_sel"].reshape(n), R.reshape(n))
    A = orc.gae_tn(ro["rewards"], ro["done"], d["V"], ref.GAMMA, ref.LAM)[0].reshape(n)
    return d, A


@pytest.mark.parametrize("fam", list(ref.FAMILIES))
def test_family_inputs_meet_their_conditions(orc, fam):
    """Every row of the family table: A and R differ in sign on a quarter of the minibatch, A has both signs on a quarter each,
    the float64 ratios leave B / 20 samples on each side of the clip."""
    c = ref.FAMILIES[fam]
    if c["compact"]:
        d, A = _compact_case(orc, fam)
    else:
        d = ref.expanded_case(fam)
        A = ref.expanded_advantages(d, orc.gae_tn)
        assert d["T"] * d["N"] == c["B"] and sorted(d["sel0"]) == list(range(c["B"]))
        ratio = d["p64"] / d["p_old"].astype(np.float64)
        assert ratio.min() > 0.79 and ratio.max() < 1.26
    got = ref.family_conditions(d, A)
    print(fam, got)
    assert got["B"] == c["B"]
    # the normalised columns are other numbers than the raw ones: a stale or unnormalised column cannot pass for them
    for col in (A, d["R"]):
        x = col[d["sel0"]]
        assert np.abs(ref.normalise64(x) - x).max() > 0.1


@pytest.mark.parametrize("name", list(ref.NORMALISER))
def test_normaliser_inputs_are_all_clipped(orc, name):
    """Every size and content of the normaliser cases: the float64 restatement clips all B samples (the cap on cases left
    out is zero), so that every loss term is (1 +- eps) * advantage."""
    n, B, col, contents = ref.NORMALISER[name]
    d = ref.normaliser_case(name, orc.gae_tn)
    assert len(d["sel0"]) == B and len(d["states"]) == n
    assert ref.all_clipped64(d) == 0
    xs = d["x"][d["sel0"]].astype(np.float64)
    if contents == "constant" or B == 1:
        assert not d["want"].any(), "std = 0: the advantage is exactly 0"
    else:
        # the side of the mean is not a question of the reduction order (two fp64 orders differ by about B 2^-53 relative)
        assert np.abs(xs - d["mean"]).min() > 1e-9 * max(1.0, abs(d["mean"]))
        assert (d["want"] > 0).any() and (d["want"] < 0).any()
    if name.startswith("repeats"):
        assert np.unique(d["sel0"]).size < B
    if contents == "large-mean":
        assert abs(d["mean"]) > 1e4 * xs.std()


def test_restatements():
    rng = np.random.default_rng(0)
    x = (rng.normal(size=3000) * 3 + 5).astype(np.float32)
    z = ref.normalise64(x).astype(np.float64)
    assert abs(z.mean()) < 1e-6 and abs(z.std() - 1) < 1e-6 and z.dtype == np.float64
    assert not ref.normalise64(np.full(7, 2.5, np.float32)).any() and not ref.normalise64(np.float32([3.0])).any()
    # a clipped term gives its advantage back bit for bit, and that advantage the term
    adv = (rng.normal(size=5000) * np.exp(rng.normal(size=5000) * 3)).astype(np.float32)
    adv[:2] = (0.0, -0.0)
    term = ref.clip_value(adv, ref.NORM_EPS)
    back, again = ref.advantage_from_term(term)
    assert np.array_equal(back[2:].view(np.uint32), adv[2:].view(np.uint32)) and not back[:2].any()
    assert np.array_equal(again.view(np.uint64), term.view(np.uint64))
    # ulp distances: neighbours, across zero, equal values
    one = np.float32(1.0)
    assert ref.ulp_distance([one], [np.nextafter(one, np.float32(2))])[0] == 1
    tiny = np.nextafter(np.float32(0), one)
    assert ref.ulp_distance([tiny], [-tiny])[0] == 2 and ref.ulp_distance([0.0], [-0.0])[0] == 0
    assert ref.ulp_distance([one], [np.float32(1.5)])[0] == 2 ** 22
    # the clip sides: ratio 2 with a positive advantage and 1 / 2 with a negative one are clipped, the converse is not
    assert not ref.unclipped64([2.0, 0.5, 1.0], np.float32([1, -1, 0]), 0.2).any()
    assert ref.unclipped64([0.5, 2.0], np.float32([1, -1]), 0.2).all()
    assert ref.buffer_shape(300) == (2, 150) and ref.buffer_shape(1025) == (1, 1025)


def test_loop_dataset_shape():
    c, d = ref.LOOP, ref.loop_dataset()
    sizes = [min(c["batch"], c["n"] - s) for s in range(0, c["n"], c["batch"])]
    assert sizes == [1100, 1100, 300] and d["T"] * d["N"] == c["n"]
    assert all(sorted(p) == list(range(c["n"])) for p in d["perm"]) and not np.array_equal(d["perm"][0], d["perm"][1])
