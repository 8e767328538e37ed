"""Plain-numpy references for the small kernels behind the numbers a PPO user reads (test helper, CPU only): the three
statistics reductions of csrc/ppo_stats.hip restated in the summation order that file documents, the truncation compaction of
csrc/ppo_gae_boot.hip (np.flatnonzero), and the table of sizes at which each of their branches opens.

The order of the reductions depends on the element count n only:
    blocks = clamp(ceil(n / 4096), 1, 1024) of 256 threads; thread g of the grid adds the four elements of the 16-byte groups
    g, g + 256 blocks, ... in ascending order, then element 4 (n >> 2) + g if that is below n (so the n & 3 elements behind the
    last whole group go to the first threads of block 0);  xor-butterfly 32, 16, .. 1 over each wave of 64;  the block's four
    waves in order;  one more wave: lane l adds the partials of blocks l, l + 64, ... to 0.0 in order, then the butterfly.
The library is built with -ffp-contract=off, so every step is one IEEE fp64 operation and numpy's is the same operation.  A
thread that skips an element (no such element, or an invalid transition) is restated as adding +0.0: an accumulator starts at
+0.0 and a sum is -0.0 only if both operands are, so no accumulator is ever -0.0 and x + 0.0 == x bit for bit."""
import numpy as np

import train_stats_ref

STATS_THREADS, STATS_PER_BLOCK, STATS_MAX_BLOCKS, FINISH_LANES = 256, 4096, 1024, 64
CP_BLOCK, SCAN_CHUNK = 1024, 256


# ---------------------------------------------------------------- geometry
def stats_geometry(n):
    """What a reduction over n elements runs: blocks, passes of the finishing wave over the block partials, the largest
    number of 16-byte groups one thread walks, the scalar tail n & 3, and whether a whole group exists."""
    blocks = min(max(-(-n // STATS_PER_BLOCK), 1), STATS_MAX_BLOCKS)
    total = blocks * STATS_THREADS
    n4 = n >> 2
    return dict(n=n, blocks=blocks, finish_passes=-(-blocks // FINISH_LANES), groups_per_thread=-(-n4 // total), tail=n & 3,
                capped=-(-n // STATS_PER_BLOCK) > STATS_MAX_BLOCKS)


def compact_geometry(n):
    """Blocks of 1024 flags, chunks of 256 block counts the scan walks with a carry, flags in the last block."""
    nb = -(-n // CP_BLOCK)
    return dict(n=n, blocks=nb, chunks=-(-nb // SCAN_CHUNK), last_width=n - (nb - 1) * CP_BLOCK)


# ---------------------------------------------------------------- the fixed order
def _butterfly(a):
    """[rows, 64] -> [rows]: v = v + shfl_xor(v, off) for off = 32 .. 1, lane 0's result."""
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        a = a + a[:, lanes ^ off]
    return a[:, 0]


def fixed_order_sum(terms):
    """sum(terms) in the device's order; terms [n] float64, the addend of every element (0.0 where the kernel skips one)."""
    terms = np.ascontiguousarray(terms, np.float64)
    n = terms.size
    g = stats_geometry(n)
    total, n4 = g["blocks"] * STATS_THREADS, n >> 2
    thread = np.arange(total, dtype=np.int64)
    acc = np.zeros(total, np.float64)
    for it in range(g["groups_per_thread"]):
        q = thread + it * total
        live = q < n4
        base = np.where(live, q, 0) * 4
        for j in range(4):
            acc = acc + np.where(live, terms[base + j], 0.0)
    i = 4 * n4 + thread
    live = i < n
    acc = acc + np.where(live, terms[np.where(live, i, 0)], 0.0)
    waves = _butterfly(acc.reshape(-1, 64)).reshape(g["blocks"], STATS_THREADS // 64)
    part = waves[:, 0]
    for w in range(1, STATS_THREADS // 64):
        part = part + waves[:, w]
    rows = np.zeros(g["finish_passes"] * FINISH_LANES, np.float64)
    rows[:g["blocks"]] = part
    s = np.zeros(FINISH_LANES, np.float64)
    for row in rows.reshape(-1, FINISH_LANES):
        s = s + row
    return float(_butterfly(s[None, :])[0])


def ratio_terms(r, eps):
    """The four addends of k_ratio_stats per element as ratio_term forms them: double(r), one fp64 log, -lg, (rd - 1) - lg,
    |rd - 1| > eps in float64, 1."""
    rd = np.asarray(r, np.float32).reshape(-1).astype(np.float64)
    lg = np.log(rd)
    return -lg, (rd - 1.0) - lg, (np.abs(rd - 1.0) > float(eps)).astype(np.float64), np.ones(rd.size, np.float64)


def ratio_sums(r, eps):
    """(sum(-log r), sum((r - 1) - log r), clip count, n) in the device's order (numpy's log, so the first two are held to
    train_stats_ref.sum_bound; the counts are sums of small integers and exact in any order)."""
    return tuple(fixed_order_sum(t) for t in ratio_terms(r, eps))


def value_clip_sums(delta, c):
    """(count(|delta| > c) with both in float32, sum(double(delta)^2), n) in the device's order."""
    d = np.asarray(delta, np.float32).reshape(-1)
    dd = d.astype(np.float64)
    return (fixed_order_sum((np.abs(d) > np.float32(c)).astype(np.float64)), fixed_order_sum(dd * dd),
            fixed_order_sum(np.ones(d.size, np.float64)))


def moment_terms(t, v, valid, i0):
    t64, v64 = np.asarray(t, np.float32).reshape(-1).astype(np.float64), np.asarray(v, np.float32).reshape(-1).astype(np.float64)
    on = np.asarray(valid).reshape(-1) != 0
    st, sd = t64[i0], t64[i0] - v64[i0]
    x = t64 - st
    y = (t64 - v64) - sd
    return [np.where(on, a, 0.0) for a in (np.ones(t64.size), x, x * x, y, y * y)]


def moment_sums(t, v, valid, i0):
    """(n, sum x, sum x^2, sum y, sum y^2) over the valid elements in the device's order, x = t - t[i0],
    y = (t - v) - (t[i0] - v[i0]), every operation in float64 on the float32 inputs."""
    return tuple(fixed_order_sum(a) for a in moment_terms(t, v, valid, i0))


# ---------------------------------------------------------------- cases: the reductions
# 1 block with no whole group (1, 2, 3), with a tail of 1 (5) and 3 (1023), exactly full (4096); 2 blocks with tails 1 and 3;
# 64 blocks = one full pass of the finishing wave; 65 = a second pass and a tail of 3; the capped grid: 1026 blocks' worth on
# 1024, so some threads walk a fifth group, with a tail of 3
STATS_SIZES = (1, 2, 3, 5, 1023, 4096, 4097, 4099, 262144, 262147, 4194304 + 4096 + 3)
STATS_REGIMES = {
    "one block": lambda g: g["blocks"] == 1,
    "two blocks": lambda g: g["blocks"] == 2,
    "no whole group": lambda g: g["groups_per_thread"] == 0,
    "finish: one full pass": lambda g: g["blocks"] == 64,
    "finish: second pass": lambda g: g["finish_passes"] == 2 and g["blocks"] == 65,
    "finish: 16 passes": lambda g: g["finish_passes"] == 16,
    "grid stride": lambda g: g["capped"] and g["groups_per_thread"] > STATS_PER_BLOCK // (4 * STATS_THREADS),
    "tail 0": lambda g: g["tail"] == 0,
    "tail 1": lambda g: g["tail"] == 1,
    "tail 2": lambda g: g["tail"] == 2,
    "tail 3": lambda g: g["tail"] == 3,
    "tail behind two blocks": lambda g: g["tail"] == 3 and g["blocks"] == 2,
    "tail behind the capped grid": lambda g: g["tail"] == 3 and g["capped"],
}


def _f32_neighbours(x):
    x = np.float32(x)
    return [x, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))]


def _plant(col, values, n):
    """Write `values` (cycled) at up to 24 positions spread over the column, the first and the last element included."""
    pos = np.unique(np.linspace(0, n - 1, min(n, 24)).astype(np.int64))
    for k, p in enumerate(pos):
        col[p] = values[k % len(values)]
    return pos


def ratio_case(n):
    """-> (float32 ratios [n], eps).  Log-uniform in [0.5, 0.95] u [1.05, 2] with eps = 0.2, so that no single term of either
    log sum is near zero: sum_bound grows like n^2 2^-53 mean|term|, and a test that holds a sum to it sees a dropped or
    doubled element only while the smallest term stands well above it (ratio_margin; the host test asserts 100 x).  At the
    largest size that needs min|term| / mean|term| above 0.2, which |r - 1| = 0.2 misses ((r - 1) - log r is 0.018 there):
    that case draws from [0.45, 0.6] u [1.5, 2] and clips at eps = 0.5.  Planted on top, the tail included: the float32
    neighbours of 1 + eps and 1 - eps, whose |double(r) - 1| lie on either side of eps by one float32 ulp."""
    rng = np.random.default_rng(7000 + n % 9973)
    (lo, eps) = (((0.45, 0.6), (1.5, 2.0)), 0.5) if n > 1 << 22 else (((0.5, 0.95), (1.05, 2.0)), 0.2)
    side = rng.random(n) < 0.5
    u = rng.random(n)
    a = np.where(side, np.log(lo[0][0]), np.log(lo[1][0]))
    b = np.where(side, np.log(lo[0][1]), np.log(lo[1][1]))
    r = np.exp(a + (b - a) * u).astype(np.float32)
    _plant(r, _f32_neighbours(1.0 + eps) + _f32_neighbours(1.0 - eps), n)
    return r, eps


def ratio_margin(r, eps):
    """(min|term| / bound for sum(-log r), likewise for sum((r - 1) - log r)) with train_stats_ref.sum_bound."""
    t1, t3, _, _ = ratio_terms(r, eps)
    b1, b3 = train_stats_ref.sum_bound(r)
    return float(np.abs(t1).min() / b1), float(np.abs(t3).min() / b3)


VCLIP_C = np.float32(0.25)


def value_clip_case(n):
    """float32 changes V - V_old with, planted on top (tail included): |delta| == c exactly on both signs (not counted: the
    comparison is strict), the float32 neighbours of c, -0.0f and +0.0f."""
    rng = np.random.default_rng(8000 + n % 9973)
    d = (rng.normal(size=n) * 0.3).astype(np.float32)
    c = VCLIP_C
    _plant(d, [c, -c, np.nextafter(c, np.float32(1)), -np.nextafter(c, np.float32(1)), np.nextafter(c, np.float32(0)),
               np.float32(-0.0), np.float32(0.0)], n)
    return d


MASKS = ("all", "half", "single")


def moments_case(n, mask):
    """-> (t, v float32 [n], valid uint8 [n], first_id = the first valid index).  "half": about every second element, never
    element 0 when n > 1, some bytes other than 1; "single": the last element only (in the scalar tail when n & 3)."""
    rng = np.random.default_rng(9000 + n % 9973 + MASKS.index(mask))
    t = (rng.normal(size=n) * 2 + 1).astype(np.float32)
    v = (t + rng.normal(size=n) * 0.5).astype(np.float32)
    if mask == "all":
        valid = np.ones(n, np.uint8)
    elif mask == "half":
        valid = (rng.random(n) < 0.5).astype(np.uint8) * rng.choice(np.array([1, 1, 2, 255], np.uint8), size=n)
        valid[-1] = 1
        if n > 1:
            valid[0] = 0
    else:
        valid = np.zeros(n, np.uint8)
        valid[-1] = 1
    return t, v, valid, int(np.flatnonzero(valid)[0])


# ---------------------------------------------------------------- cases: the compaction
# below, at and above one wave (63, 64, 65), one 256-flag item (255, 256, 257) and one block (1023, 1024, 1025); 5 blocks with
# a ragged last one; 256 blocks = exactly one chunk of the scan; 257 = a carry into a last block one flag wide; 512 = the
# benchmark's; 1025 blocks = four carries and a last block one flag wide
COMPACT_SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 5000, 262144, 262145, 524288, 1048577)
COMPACT_REGIMES = {
    "one block": lambda g: g["blocks"] == 1,
    "part of one wave": lambda g: g["n"] < 64,
    "block offsets other than 0": lambda g: 1 < g["blocks"] <= SCAN_CHUNK,
    "exactly one scan chunk": lambda g: g["blocks"] == SCAN_CHUNK,
    "one carry": lambda g: g["chunks"] == 2,
    "several carries": lambda g: g["chunks"] > 2,
    "ragged last block": lambda g: 1 < g["last_width"] < CP_BLOCK,
    "last block one flag wide": lambda g: g["last_width"] == 1 and g["blocks"] > 1,
    "carry into a one-flag block": lambda g: g["last_width"] == 1 and g["blocks"] == SCAN_CHUNK + 1,
}
PATTERNS = ("none", "all", "first", "last", "mod64", "mod256", "mod1024", "random7", "random_empty_blocks", "random_bytes")


def patterns_for(n):
    """The patterns that say something at n flags: `last` needs a second flag, `mod m` one whole period, and emptying every
    third block a second block."""
    out = []
    for p in PATTERNS:
        if p == "last" and n < 2:
            continue
        if p.startswith("mod") and n < int(p[3:]):
            continue
        if p == "random_empty_blocks" and n <= CP_BLOCK:
            continue
        out.append(p)
    return out


def flags_case(n, pattern):
    """uint8 flags [n].  random7: density 1/7 (the benchmark's 1 / max_actions); random_empty_blocks: density 1/3 with blocks
    0, 3, 6, ... of 1024 flags cleared; random_bytes: density 1/7 with set bytes drawn from 2 .. 255 (the kernels test != 0)."""
    rng = np.random.default_rng(100003 * PATTERNS.index(pattern) + n)
    i = np.arange(n)
    if pattern == "none":
        f = np.zeros(n, bool)
    elif pattern == "all":
        f = np.ones(n, bool)
    elif pattern == "first":
        f = i == 0
    elif pattern == "last":
        f = i == n - 1
    elif pattern.startswith("mod"):
        m = int(pattern[3:])
        f = (i % m == 0) | (i % m == m - 1)
    elif pattern == "random_empty_blocks":
        f = (rng.random(n) < 1 / 3) & ((i // CP_BLOCK) % 3 != 0)
    else:
        f = rng.random(n) < 1 / 7
    flags = f.astype(np.uint8)
    if pattern == "random_bytes":
        flags = flags * rng.integers(2, 256, size=n).astype(np.uint8)
    return flags


def compact_ref(flags):
    """-> (K, ids [n] int32: the ascending positions of the non-zero flags, then -1)."""
    ids = np.flatnonzero(np.asarray(flags).reshape(-1)).astype(np.int32)
    out = np.full(np.asarray(flags).size, -1, np.int32)
    out[:ids.size] = ids
    return int(ids.size), out


# ---------------------------------------------------------------- cases: the standalone loss and the sampler
LOSS_B = (1, 3, 4, 5, 255, 256, 257, 1000, 4099)
LOSS_A = (128, 512)


def loss_case(B, A):
    """probabilities [B, A] float32 (a masked softmax: a quarter of every row is exactly 0), 1-based actions on positive
    entries, old probabilities within 0.8 .. 1.25 of the new ones, advantages of both signs."""
    rng = np.random.default_rng(11 * B + A)
    logits = rng.normal(size=(B, A)) * 2
    logits[rng.random((B, A)) < 0.25] = -np.inf
    logits[:, 0] = 0.0
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    probs = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    a1 = np.array([rng.choice(np.flatnonzero(probs[b] > 0)) for b in range(B)], np.int64) + 1
    p_old = (probs[np.arange(B), a1 - 1] * rng.uniform(0.8, 1.25, B)).astype(np.float32)
    adv = rng.normal(size=B).astype(np.float32)
    return probs, a1, p_old, adv


def sampler_case(B, A):
    """probabilities [B, A] and uniforms [B]; row 0's walk runs off the end onto a zero entry (mass 0.5, u = 0.75), and the
    last row's uniform is the largest float32 below 1."""
    rng = np.random.default_rng(13 * B + A)
    p = rng.random((B, A)).astype(np.float32)
    p[rng.random((B, A)) < 0.3] = 0
    p[:, 7] += 0.1
    p = (p / p.sum(axis=1, keepdims=True, dtype=np.float32)).astype(np.float32)
    u = rng.random(B).astype(np.float32)
    u[-1] = np.nextafter(np.float32(1), np.float32(0))
    p[0] = 0
    p[0, 0] = 0.5
    u[0] = 0.75
    return p, u
