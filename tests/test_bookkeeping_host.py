"""tests/bookkeeping_ref.py held against plain numpy, and its case tables against the branches of the kernels, on a machine
without a GPU: the fixed-order restatements agree with numpy's own sums within the derived bounds; every ratio case keeps each
log sum's smallest term at least 100 x above the bound the device is held to; every regime of csrc/ppo_stats.hip and of the
compaction in csrc/ppo_gae_boot.hip is hit by a size of the tables; the four test-only entry points are exported, stay out of
the header and refuse null arguments."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bookkeeping_ref as ref
import train_stats_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "proximalpolicyoptimization.jl_amd", "csrc")
DEBUG = ("ppo_debug_ratio_stats", "ppo_debug_value_clip_stats", "ppo_debug_value_moments", "ppo_debug_compact_flags")


def _define(src, name):
    m = re.search(r"#define\s+%s\s+(\S+)" % name, src)
    assert m, name
    return m.group(1)


def test_constants_are_the_kernels():
    stats = open(os.path.join(CSRC, "ppo_stats.hip")).read()
    assert int(_define(stats, "STATS_THREADS")) == ref.STATS_THREADS
    assert int(_define(stats, "STATS_PER_BLOCK")) == ref.STATS_PER_BLOCK
    assert int(_define(stats, "STATS_MAX_BLOCKS")) == ref.STATS_MAX_BLOCKS
    boot = open(os.path.join(CSRC, "ppo_gae_boot.hip")).read()
    assert int(_define(boot, "CP_ITEMS")) * 256 == ref.CP_BLOCK and _define(boot, "CP_BLOCK") == "(256"
    assert "-ffp-contract=off" in open(os.path.join(CSRC, "Makefile")).read()


def test_debug_entry_points_exported_outside_the_header(ppo):
    hdr = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()
    L = ppo._lib.lib()
    for name in DEBUG:
        assert hasattr(L, name), "%s is not exported by libppo_hip.so" % name
        assert name not in hdr and name not in ppo._lib.SIGNATURES


def test_every_stats_regime_has_a_size():
    geo = [ref.stats_geometry(n) for n in ref.STATS_SIZES]
    for name, hit in ref.STATS_REGIMES.items():
        assert any(hit(g) for g in geo), name
    g = ref.stats_geometry(ref.STATS_SIZES[-1])
    assert g == dict(n=4198403, blocks=1024, finish_passes=16, groups_per_thread=5, tail=3, capped=True)
    assert ref.stats_geometry(262147)["blocks"] == 65 and ref.stats_geometry(262144)["finish_passes"] == 1
    assert ref.stats_geometry(524288)["blocks"] == 128                     # the benchmark's buffer


def test_every_compaction_regime_has_a_size_and_a_pattern():
    geo = [ref.compact_geometry(n) for n in ref.COMPACT_SIZES]
    for name, hit in ref.COMPACT_REGIMES.items():
        assert any(hit(g) for g in geo), name
    assert ref.compact_geometry(262144) == dict(n=262144, blocks=256, chunks=1, last_width=1024)
    assert ref.compact_geometry(262145) == dict(n=262145, blocks=257, chunks=2, last_width=1)
    assert ref.compact_geometry(524288)["blocks"] == 512
    seen = set()
    for n in ref.COMPACT_SIZES:
        pats = ref.patterns_for(n)
        assert {"none", "all", "first", "random7", "random_bytes"} <= set(pats)
        for p in pats:
            f = ref.flags_case(n, p)
            assert f.dtype == np.uint8 and f.shape == (n,)
            K, ids = ref.compact_ref(f)
            assert ids.dtype == np.int32 and np.all(ids[K:] == -1) and np.all(f[ids[:K]] != 0) and np.all(np.diff(ids[:K]) > 0)
            assert K == np.count_nonzero(f)
            per_block = np.add.reduceat((f != 0).astype(np.int64), np.arange(0, n, ref.CP_BLOCK))
            if K == 0:
                seen.add("K == 0")
            if K == n:
                seen.add("K == n")
            if K and (per_block == 0).any():
                seen.add("blocks without a flag")
            if (per_block[:-1] == ref.CP_BLOCK).any():
                seen.add("full blocks")
            if p == "random_bytes":
                assert K > 0 or n < 64
                assert set(np.unique(f)) - {0, 1} or K == 0
            if p == "random_empty_blocks":
                assert not per_block[::3].any() and per_block[:n // ref.CP_BLOCK][1::3].all()
            if p == "random7" and n >= 5000:
                assert abs(K / n - 1 / 7) < 0.02
        seen.update(pats)
    assert seen >= set(ref.PATTERNS) | {"K == 0", "K == n", "blocks without a flag", "full blocks"}


def test_fixed_order_sum_is_a_sum():
    """Against math.fsum (exact) within n 2^-53 sum|x| at every size class, and exact where every order is: small integers."""
    import math
    rng = np.random.default_rng(0)
    for n in (1, 2, 3, 4, 5, 63, 1023, 4097, 4099, 8195, 262147):
        x = rng.normal(size=n)
        got = ref.fixed_order_sum(x)
        assert abs(got - math.fsum(x)) <= n * 2.0 ** -53 * np.abs(x).sum()
        assert ref.fixed_order_sum(np.ones(n)) == n
        assert ref.fixed_order_sum(np.arange(n, dtype=np.float64)) == n * (n - 1) // 2
    # the order is not numpy's: some size gives another rounding than np.sum (otherwise the restatement restates nothing)
    assert any(ref.fixed_order_sum(x) != float(np.sum(x)) for x in (rng.normal(size=n) for n in (4099, 8195, 262147)))
    # one element added twice or dropped moves the result
    x = rng.normal(size=4099)
    for i in (0, 4095, 4096, 4098):
        y = x.copy()
        y[i] = 0.0
        assert ref.fixed_order_sum(y) != ref.fixed_order_sum(x)


@pytest.mark.parametrize("n", ref.STATS_SIZES)
def test_ratio_cases(n):
    r, eps = ref.ratio_case(n)
    assert r.dtype == np.float32 and r.shape == (n,) and np.all(r > 0)
    s1, s3, c, cnt = ref.ratio_sums(r, eps)
    p1, p3, pc, pn = train_stats_ref.ratio_sums(r, eps)
    b1, b3 = train_stats_ref.sum_bound(r)
    assert cnt == n == pn and c == pc
    assert abs(s1 - p1) <= b1 and abs(s3 - p3) <= b3
    # the precondition of the device test: no single term can hide inside the bound
    m1, m3 = ref.ratio_margin(r, eps)
    assert m1 >= 100 and m3 >= 100, (n, m1, m3)
    # ratios one float32 ulp on either side of the clip range, decided in float64 as ratio_term does
    rd = r.astype(np.float64)
    for centre in (1.0 + eps, 1.0 - eps):
        near = np.abs(rd - centre) <= 2.0 ** -22
        if n >= 6:
            assert (np.abs(rd[near] - 1.0) > eps).any() and (np.abs(rd[near] - 1.0) <= eps).any(), (n, centre)
    if n >= 24:
        assert 0 < c < n


@pytest.mark.parametrize("n", ref.STATS_SIZES)
def test_value_clip_cases(n):
    d = ref.value_clip_case(n)
    c = ref.VCLIP_C
    cnt, sq, m = ref.value_clip_sums(d, c)
    dd = d.astype(np.float64)
    assert m == n and cnt == np.count_nonzero(np.abs(dd) > float(c))
    assert abs(sq - float(np.sum(dd * dd))) <= n * 2.0 ** -52 * float(np.sum(dd * dd))
    assert ref.value_clip_sums(d, np.float32(np.inf))[0] == 0.0
    if n >= 24:
        assert (np.abs(d) == c).sum() >= 2 and (d == c).any() and (d == -c).any()
        assert np.signbit(d[d == 0]).any() and 0 < cnt < n
    if n & 3 and n > 4:
        assert np.abs(d[-1]) == c or d[-1] == 0 or np.abs(np.abs(d[-1]) - c) < 1e-6, "a planted value sits in the tail"


@pytest.mark.parametrize("n", ref.STATS_SIZES)
@pytest.mark.parametrize("mask", ref.MASKS)
def test_moments_cases(n, mask):
    t, v, valid, i0 = ref.moments_case(n, mask)
    assert valid[i0] and not valid[:i0].any()
    if mask != "all" and n > 1:
        assert i0 != 0
    if mask == "single":
        assert valid.sum() == 1 and i0 == n - 1
    got = ref.moment_sums(t, v, valid, i0)
    want, mags = train_stats_ref.value_moments(t, v, valid, i0)
    assert got[0] == want[0] == np.count_nonzero(valid)
    for q in range(1, 5):
        assert abs(got[q] - want[q]) <= want[0] * 2.0 ** -52 * mags[q], (q, got[q], want[q])
    if mask == "half" and n >= 1023:
        assert 0.4 < want[0] / n < 0.6 and set(np.unique(valid)) >= {0, 1, 2, 255}


def test_loss_and_sampler_cases(orc):
    for A in ref.LOSS_A:
        for B in (1, 5, 257):
            probs, a1, p_old, adv = ref.loss_case(B, A)
            assert probs.shape == (B, A) and np.all(probs[np.arange(B), a1 - 1] > 0) and (probs == 0).any()
            assert np.abs(probs.sum(axis=1) - 1).max() < 1e-5
            p, u = ref.sampler_case(B, A)
            a, err = orc.categorical_sample(p[0], u[0])
            assert a == A - 1 and err == 1, "row 0 walks off the end onto a zero entry"
            assert u[-1] < 1.0


def test_null_arguments_are_refused(ppo):
    L = ppo._lib.lib()
    one = np.zeros(4, np.float64)
    for name in DEBUG:
        getattr(L, name).restype = C.c_int32
    L.ppo_debug_ratio_stats.argtypes = [C.c_void_p, C.c_int64, C.c_double, C.c_void_p]
    L.ppo_debug_value_clip_stats.argtypes = [C.c_void_p, C.c_int64, C.c_float, C.c_void_p]
    L.ppo_debug_value_moments.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    L.ppo_debug_compact_flags.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    assert L.ppo_debug_ratio_stats(None, 1, 0.2, one.ctypes.data) != 0
    assert L.ppo_debug_value_clip_stats(None, 1, 0.2, one.ctypes.data) != 0
    assert L.ppo_debug_value_moments(None, None, None, 0, 1, one.ctypes.data) != 0
    assert L.ppo_debug_compact_flags(None, 1, None, None) != 0
