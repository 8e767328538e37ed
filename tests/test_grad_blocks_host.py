"""What tests/test_gpu_grad_blocks.py rests on, shown on the CPU from the reference alone (tests/grad_blocks_ref.py):

  * the block and tile cuts tile the flat gradient exactly, at every depth, at F = 72 and 216 and at a padded width;
  * grad64 is the C oracle's float64 gradient (1e-12 of max|g|);
  * the routes the extra cases name are the ones the library picks under their knobs;
  * in every case the kink and clip filters keep at least half of the candidate states;
  * the fp32 floor is positive in every block and tile of every case;
  * what the bar can and cannot see: the low bf16 piece of H1 dropped in the dW2 product, or of W2 in the dH1 product,
    restated in torch.  Measured, per block, as a multiple of the floor (the bar is M = 4), next to the old metric
    max|g - g64| / max|g64| (its bar is 2e-5):

        case            drop        block multiples       worst tile       old metric with the drop (without)
        x6-h128         H1 in dW2   W2 3.9                W2[0,0] 4.4      1.06e-6 (6.7e-7)
        x6-h128         W2 in dH1   W1 3.7, b1 4.1        W1[0] 4.2        1.01e-6 (6.7e-7)
        x6-h256         H1 in dW2   W2 3.5                W2[2,3] 4.3      7.0e-7 (7.0e-7)
        x6-h256         W2 in dH1   W1 3.2, b1 3.6        W1[3] 3.4        7.6e-7 (7.0e-7)
        poly-30-seed17  H1 in dW2   W2 1.01               W2[0,0] 1.03     5.0e-5 (5.0e-5)
        poly-30-seed17  W2 in dH1   W1 1.00, b1 1.01      W1[1] 1.00       5.1e-5 (5.0e-5)

    A low-piece drop sits at the bar near initialisation and is invisible on a peaked policy, where the conditioning of the
    minibatch sets a floor 50 times higher; the old metric sees it nowhere.  The multiples are recorded (printed by
    test_low_piece_drops_measured), not asserted above M; profiles/grad_blocks_mutations.txt has the same drops made in the
    kernel itself."""
import json

import numpy as np
import pytest

import grad_blocks_ref as gb
from oracle import np_oracle
from test_train_route import route

SHAPES = [(F, hid, L) for F in (72, 216) for L in (1, 2, 3, 4) for hid in (128, 256, 50)]


@pytest.mark.parametrize("F,hid,L", SHAPES)
def test_cuts_tile_the_flat_gradient(F, hid, L):
    HID = gb.kernel_width(hid)
    n = gb.num_params(F, hid, L)
    bl, tl = gb.blocks(F, hid, HID, L), gb.tiles(F, hid, HID, L)
    assert list(bl) == [x % l for l in range(1, L + 1) for x in ("W%d", "b%d")] + ["out"]
    # the blocks are consecutive and cover the vector; they are unpack_params' arrays
    at = 0
    for s in bl.values():
        assert s.start == at and s.stop > s.start
        at = s.stop
    assert at == n
    marked = np.arange(n, dtype=np.float32)
    layers = np_oracle.unpack_params(marked, F, hid, L)
    for l, (W, b) in enumerate(layers[:-1], 1):
        assert np.array_equal(marked[bl["W%d" % l]], W.ravel(order="F")) and np.array_equal(marked[bl["b%d" % l]], b)
    assert np.array_equal(marked[bl["out"]], np.concatenate([layers[-1][0].ravel(order="F"), layers[-1][1]]))
    # the tiles of a W partition that W; a tile is 32 consecutive units of the matrix on each side (the last one ragged)
    nt = -(-hid // 32)
    assert len(tl) == nt + (L - 1) * nt * nt and nt <= HID // 32
    for l in range(1, L + 1):
        mine = [idx for (par, idx) in tl.values() if par == "W%d" % l]
        allidx = np.concatenate(mine)
        assert np.array_equal(np.sort(allidx), np.arange(bl["W%d" % l].start, bl["W%d" % l].stop))
    W1 = layers[0][0]
    for t in range(nt):
        assert np.array_equal(np.sort(marked[tl["W1[%d]" % t][1]]), np.sort(W1[32 * t:32 * t + 32].ravel()))
    if L >= 2:
        W2 = layers[1][0]
        to, ti = nt - 1, 0
        assert np.array_equal(np.sort(marked[tl["W2[%d,%d]" % (to, ti)][1]]),
                              np.sort(W2[32 * to:32 * to + 32, 32 * ti:32 * ti + 32].ravel()))


@pytest.mark.parametrize("F,hid,L,Q", [(72, 128, 1, 8), (72, 128, 2, 8), (72, 256, 3, 8), (72, 128, 4, 8), (216, 128, 2, 8),
                                       (72, 50, 2, 8), (72, 256, 2, 32)])
def test_grad64_is_the_c_oracle(orc, F, hid, L, Q):
    rng = np.random.default_rng(F + hid + L + Q)
    B = 5
    params = gb.am.make_params(F, hid, L, 3)
    states = gb.am.random_states(rng, params, F, hid, L, B, Q)
    active = rng.integers(1, 2 ** Q, size=B, dtype=np.uint64).astype(np.uint32)
    probs = gb.am.probabilities(params, "f32", F, hid, L, states, active, Q)
    a0 = gb.am.sample_actions(rng, probs)
    p_old = (probs[np.arange(B), a0] / gb.am.ratios_off_the_clip(rng, B, gb.EPS)).astype(np.float32)
    adv = rng.normal(size=B).astype(np.float32)
    g, lp, le = gb.grad64(params, F, hid, states, np_oracle.batch_masks(active, Q), a0, p_old, adv, gb.EPS, gb.ENT, n_hidden=L)
    want, olp, ole = orc.step_batch_grad_f64(params, F, hid, states, active, a0, p_old, adv, gb.EPS, gb.ENT, n_hidden=L)
    assert np.abs(g - want).max() <= 1e-12 * np.abs(want).max()
    assert abs(lp - olp) <= 1e-12 and abs(le - ole) <= 1e-12
    # and B_global scales it like step_batch_grad_torch's
    g2, _, _ = gb.grad64(params, F, hid, states, np_oracle.batch_masks(active, Q), a0, p_old, adv, gb.EPS, gb.ENT, n_hidden=L,
                         B_global=2 * B)
    assert np.abs(2 * g2 - want).max() <= 1e-12 * np.abs(want).max()


def test_extra_cases_name_their_routes(ppo):
    """The knobs of the backwards the family table does not pin select the kernels the cases name (queried without a
    device, as tests/test_train_route.py does)."""
    try:
        for name, c in gb.EXTRA.items():
            ppo.set_bwd_split_bf16(c["knobs"].get("split"))
            ppo.set_bwd_small_max_tiles(c["knobs"].get("small"))
            sh = gb.shape_of(name)
            assert route(ppo, "f32", 72, sh["HID"], c["L"], 32, False, c["B"]) == c["route"], name
    finally:
        ppo.set_bwd_split_bf16(None)
        ppo.set_bwd_small_max_tiles(None)


@pytest.mark.parametrize("name", gb.F32_CASES)
def test_case_keeps_half_its_states_and_has_a_floor(orc, name):
    d, sh = gb.case(name, orc), gb.shape_of(name)
    assert d["kept"] >= 0.5, (name, d["kept"])
    mb = gb.minibatch(d)
    assert len(mb["states"]) == (gb.am.FAMILIES[name]["B"] if name in gb.am.FAMILIES else gb.EXTRA[name]["B"])
    # the minibatch itself holds no state on the kink and no ratio at the clip
    assert gb.value_ref.off_the_kink(d["params"], sh["F"], sh["hid"], sh["L"], mb["states"], delta=gb.KINK).all()
    p = gb.am.probabilities(d["params"], "f32", sh["F"], sh["hid"], sh["L"], mb["states"], mb["active"], sh["Q"])
    r64 = p[np.arange(len(p)), mb["a0"]] / mb["p_old"].astype(np.float64)
    assert np.all(np.abs(r64 - (1 - gb.EPS)) > 1e-3) and np.all(np.abs(r64 - (1 + gb.EPS)) > 1e-3)
    ref = gb.reference(sh, d["params"], mb)
    assert all(f > 0 for f in ref["fb"].values()) and all(f > 0 for f in ref["ft"].values()), ref["fb"]
    # the reference holds its own bar: M floors contain the floor
    mult, worst, old = gb.multiples(ref["g32"], ref["g64"], ref["fb"], ref["ft"], ref["blocks"], ref["tiles"])
    assert all(abs(m - 1) < 1e-12 for m in mult.values()) and worst[1] <= 1 + 1e-12


@pytest.mark.parametrize("name", ["x6-h128", "x6-h256", "poly-30-seed17"])
def test_low_piece_drops_measured(orc, name):
    """The two simulated low-piece drops of the module docstring: recorded as multiples of the floor, with the old metric.
    Asserted: the drop moves only the blocks downstream of the product it is taken in."""
    d, sh = gb.case(name, orc), gb.shape_of(name)
    mb = gb.minibatch(d)
    ref = gb.reference(sh, d["params"], mb)
    old32 = float(np.abs(ref["g32"] - ref["g64"]).max() / np.abs(ref["g64"]).max())
    for which, moved in (("H1 in dW2", {"W2"}), ("W2 in dH1", {"W1", "b1"})):
        g = gb.grad32_low_piece_dropped(which, d["params"], sh["F"], sh["hid"], mb["states"], np_oracle.batch_masks(mb["active"], 8),
                                        mb["a0"], mb["p_old"], mb["adv"], gb.EPS, gb.ENT)
        mult, worst, old = gb.multiples(g, ref["g64"], ref["fb"], ref["ft"], ref["blocks"], ref["tiles"])
        print(json.dumps(dict(case=name, drop=which, multiples={k: round(v, 2) for k, v in mult.items()}, worst_tile=worst,
                              old_metric=old, old_metric_fp32=old32)))
        for k, m in mult.items():
            assert np.isfinite(m) and (k in moved or abs(m - 1) < 1e-12), (which, k, m)
