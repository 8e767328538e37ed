"""Which kernels run a training minibatch (csrc/ppo_route.hip: train_route), queried through ppo_debug_train_route on the
CPU.  The expected route is the launch chain as it stood before the choice moved into one function, restated: the one-tile
pass (launch_policy_train_tile), then the train forward (split-fp32 x6 -> 2/4-waves-per-state split -> k_policy_fwd or
bf16), then the backward (three-product -> split-fp32 x6 -> k_policy_bwd or bf16).  Kernels are named as a kernel trace
lists them demangled, without spaces; the GPU tests assert the same names against what forward_backward runs."""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPE = {"f32": 0, "bf16": 1}
ERR_UNSUPPORTED = -4
DEFAULT = dict(split=1, train_tile=0, small=384, small_split=0, fwd_split=512, x6_max=1 << 30, t2=1536, t2_128=1024)
NO_BF16 = "unsupported policy/state shape (F,HID,H) for the gfx950 bf16 kernels"
NO_FP32 = "unsupported policy/state shape (F,HID,H) for the gfx950 kernels"
NO_COMPACT = "compact rollouts need the built-in env's F = 72"


def route(ppo, dtype, F, hid, L, H, compact, states):
    """(forward kernel, backward kernel), or ("none", error text)."""
    lib = ppo._lib.lib()
    fn = lib.ppo_debug_train_route
    fn.argtypes = [C.c_int32] * 6 + [C.c_int64, C.c_char_p, C.c_char_p, C.c_int64]
    fn.restype = C.c_int32
    fwd, bwd = C.create_string_buffer(128), C.create_string_buffer(128)
    s = fn(DTYPE[dtype], F, hid, L, H, int(compact), states, fwd, bwd, 128)
    if s != 0:
        assert s == ERR_UNSUPPORTED and fwd.value == b"none" and bwd.value == b"none", (s, fwd.value, bwd.value)
        return ("none", ppo._lib.last_error())
    return (fwd.value.decode(), bwd.value.decode())


def expected(dtype, F, hid, L, H, compact, B, k=DEFAULT):
    f32, tps = dtype == "f32", H // 32
    tiles = B * tps
    images = F == 72 and L == 2                  # ppo_policy_create allocates the split-fp32 weight images (w1x, w2fx, w2x)
    # forward_backward_dev: the one-tile pass up to train_tile tiles (L = 2, fp32), where launch_policy_train_tile covers it
    if tiles <= k["train_tile"] and L == 2 and f32 and F == 72 and H == 32 and not compact:
        return ("k_policy_train_tile<72,%d>" % hid, "k_policy_wgrad<72,%d,true>" % hid)
    # launch_policy_train_fwd: launch_policy_train_fwd_x6, then launch_policy_train_fwd_split, then MODE 2 / 4
    if k["split"] and B <= k["x6_max"] and f32 and L == 2 and F == 72 and (tps == 1 or (tps == 4 and hid == 256)) and images:
        if tps == 4:
            fwd = "k_policy_fwd_train_x6s<256,4>"
        elif hid == 256 and k["t2"] > 0 and B >= k["t2"]:
            fwd = "k_policy_fwd_train_x6t<256,2>"
        elif hid == 128 and k["t2_128"] > 0 and B >= k["t2_128"]:
            fwd = "k_policy_fwd_train_x6t<128,2>"
        else:
            fwd = "k_policy_fwd_train_x6<%d>" % hid
    elif B <= k["fwd_split"] and f32 and F == 72 and tps == 1 and L == 2:
        fwd = "k_policy_fwd_train_split<72,%d,%d,%d>" % (hid, 4 if B <= 256 else 2, int(compact))
    else:
        mode = 4 if compact else 2
        if not f32:
            if F != 72:
                return ("none", NO_BF16)
            fwd = "k_policy_fwd_bf16<72,%d,%d,%d>" % (hid, mode, tps)
        else:
            if not (F == 72 or tps == 1):
                return ("none", NO_FP32)
            if mode == 4 and F != 72:
                return ("none", NO_COMPACT)
            fwd = "k_policy_fwd<%d,%d,%d,%d,%d>" % (F, hid, mode, tps, int(L != 2))
    # backward: launch_policy_bwd_small, else launch_policy_bwd (bf16, then launch_policy_bwd_x6, then k_policy_bwd)
    fused_ok = L == 2 and not (F == 216 and hid == 256)
    split_covers = bool(k["split"]) and fused_ok and F == 72 and images
    small_max = k["small_split"] if split_covers else k["small"]
    if (tiles <= small_max or not fused_ok) and f32:
        bwd = "k_policy_bwd_data%s<%d,%d>" % ("" if L == 2 else "_deep", F, hid)
    elif not f32:
        bwd = "k_policy_bwd_bf16<72,%d>" % hid
    elif k["split"] and L == 2 and images:
        bwd = "k_policy_bwd_x6<72,%d>" % hid
    else:
        bwd = "k_policy_bwd<%d,%d>" % (F, hid)
    return (fwd, bwd)


# states on both sides of every switch point: 4 / 2 waves per state (256), the three-product backward (384 tiles), the split
# train forward (512 states), the two-tile x6 form (1024 / 1536 tiles)
SIZES = [1, 2, 255, 256, 257, 383, 384, 385, 511, 512, 513, 1023, 1024, 1025, 1535, 1536, 1537, 4096, 65536]
SHAPES = list(itertools.product(("f32", "bf16"), (72, 216), (128, 256), (1, 2, 3), (8, 32), (False, True)))


@pytest.fixture()
def knobs(ppo):
    yield ppo
    ppo.set_bwd_split_bf16(None)
    ppo.set_train_tile_max_tiles(None)
    ppo.set_bwd_small_max_tiles(None)
    ppo.set_fwd_split_max_states(None)
    ppo.set_fwd_split_t2_min_tiles(128, None)
    ppo.set_fwd_split_t2_min_tiles(256, None)


def _check_all(ppo, k, sizes=SIZES):
    for (dtype, F, hid, L, Q, compact) in SHAPES:
        for B in sizes:
            got = route(ppo, dtype, F, hid, L, 4 * Q, compact, B)
            assert got == expected(dtype, F, hid, L, 4 * Q, compact, B, k), (dtype, F, hid, L, Q, compact, B)


def test_bench_routes(knobs):
    """The shapes bench.py and the GPU suite run, spelled out."""
    P = knobs
    assert route(P, "f32", 72, 256, 2, 32, False, 4096) == ("k_policy_fwd_train_x6t<256,2>", "k_policy_bwd_x6<72,256>")
    assert route(P, "f32", 72, 256, 2, 32, True, 4096) == ("k_policy_fwd_train_x6t<256,2>", "k_policy_bwd_x6<72,256>")
    assert route(P, "f32", 72, 128, 2, 32, False, 4096) == ("k_policy_fwd_train_x6t<128,2>", "k_policy_bwd_x6<72,128>")
    assert route(P, "f32", 72, 256, 2, 32, False, 1535) == ("k_policy_fwd_train_x6<256>", "k_policy_bwd_x6<72,256>")
    assert route(P, "f32", 72, 128, 2, 32, False, 1023) == ("k_policy_fwd_train_x6<128>", "k_policy_bwd_x6<72,128>")
    assert route(P, "f32", 72, 256, 2, 128, False, 8192) == ("k_policy_fwd_train_x6s<256,4>", "k_policy_bwd_x6<72,256>")
    assert route(P, "f32", 72, 128, 2, 128, False, 1024) == ("k_policy_fwd<72,128,2,4,0>", "k_policy_bwd_x6<72,128>")
    assert route(P, "f32", 72, 256, 3, 32, False, 4096) == ("k_policy_fwd<72,256,2,1,1>", "k_policy_bwd_data_deep<72,256>")
    assert route(P, "f32", 72, 256, 1, 32, False, 4096) == ("k_policy_fwd<72,256,2,1,1>", "k_policy_bwd_data_deep<72,256>")
    assert route(P, "bf16", 72, 256, 2, 32, False, 65536) == ("k_policy_fwd_bf16<72,256,2,1>", "k_policy_bwd_bf16<72,256>")
    assert route(P, "f32", 216, 256, 2, 32, False, 4096) == ("k_policy_fwd<216,256,2,1,0>", "k_policy_bwd_data<216,256>")
    P.set_bwd_split_bf16(0)
    assert route(P, "f32", 72, 256, 2, 32, False, 384) == ("k_policy_fwd_train_split<72,256,2,0>", "k_policy_bwd_data<72,256>")
    assert route(P, "f32", 72, 256, 2, 32, False, 385) == ("k_policy_fwd_train_split<72,256,2,0>", "k_policy_bwd<72,256>")
    assert route(P, "f32", 72, 256, 2, 32, False, 513) == ("k_policy_fwd<72,256,2,1,0>", "k_policy_bwd<72,256>")


def test_none_routes(knobs):
    P = knobs
    assert route(P, "f32", 216, 128, 2, 128, False, 64) == ("none", NO_FP32)
    assert route(P, "f32", 216, 128, 3, 32, True, 64) == ("none", NO_COMPACT)
    assert route(P, "f32", 216, 256, 2, 128, True, 64) == ("none", NO_FP32)
    assert route(P, "bf16", 216, 256, 2, 32, False, 64) == ("none", NO_BF16)


def test_default_route_table(knobs):
    _check_all(knobs, DEFAULT)


def test_route_table_split_off(knobs):
    knobs.set_bwd_split_bf16(0)
    _check_all(knobs, dict(DEFAULT, split=0))
    knobs.set_bwd_split_bf16(None)
    _check_all(knobs, DEFAULT, sizes=[384, 385, 4096])


@pytest.mark.parametrize("setter,key,values", [
    ("set_train_tile_max_tiles", "train_tile", (384, 1536, 0)),
    ("set_bwd_small_max_tiles", "small", (0, 1024, 100000)),
    ("set_fwd_split_max_states", "fwd_split", (0, 256, 4096)),
])
def test_setter_moves_its_switch_and_minus_one_restores(knobs, setter, key, values):
    for split in (1, 0):
        knobs.set_bwd_split_bf16(split)
        for v in values:
            getattr(knobs, setter)(v)
            _check_all(knobs, dict(DEFAULT, split=split, **{key: v}), sizes=[1, 256, 257, 384, 385, 512, 513, 1536, 4096])
        getattr(knobs, setter)(None)
        _check_all(knobs, dict(DEFAULT, split=split), sizes=[1, 384, 385, 512, 513, 4096])


def test_t2_setter_and_minus_one_restores(knobs):
    P = knobs
    P.set_fwd_split_t2_min_tiles(256, 200)
    P.set_fwd_split_t2_min_tiles(128, 0)
    assert route(P, "f32", 72, 256, 2, 32, True, 199) == ("k_policy_fwd_train_x6<256>", "k_policy_bwd_x6<72,256>")
    assert route(P, "f32", 72, 256, 2, 32, True, 200) == ("k_policy_fwd_train_x6t<256,2>", "k_policy_bwd_x6<72,256>")
    _check_all(P, dict(DEFAULT, t2=200, t2_128=0), sizes=[1, 199, 200, 1024, 4096])
    P.set_fwd_split_t2_min_tiles(256, None)
    P.set_fwd_split_t2_min_tiles(128, None)
    _check_all(P, DEFAULT, sizes=[200, 1023, 1024, 1535, 1536])
    with pytest.raises(P.PPOError):
        P.set_fwd_split_t2_min_tiles(192, 100)


_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import ppo_amd as P
from test_train_route import route
cases = json.loads(sys.argv[2])
out = []
for c in cases:
    if c[0] == "set":
        getattr(P, c[1])(*c[2:])
    else:
        out.append(route(P, *c))
print(json.dumps(out))
"""


def _child(env, cases):
    e = dict(os.environ, **env)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, json.dumps(cases)], env=e, cwd=os.path.join(ROOT, "tests"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return [tuple(x) for x in json.loads(r.stdout.strip().splitlines()[-1])]


def test_environment_sets_the_knobs_and_minus_one_restores_it():
    """Each variable is read once at load; a setter's -1 returns to the variable's value, not to the built-in default."""
    env = {"PPO_FWD_SPLIT_MAX_TILES": "1000", "PPO_FWD_SPLIT_T2_MIN_TILES": "600", "PPO_BWD_SMALL_MAX_TILES_SPLIT": "300",
           "PPO_TRAIN_TILE_MAX_TILES": "64", "PPO_FWD_SPLIT_MAX_STATES": "100"}
    k = dict(DEFAULT, x6_max=1000, t2=600, small_split=300, train_tile=64, fwd_split=100)
    shapes = [("f32", 72, 256, 2, 32, False), ("f32", 72, 128, 2, 32, True), ("f32", 72, 256, 2, 128, False)]
    sizes = [1, 64, 65, 100, 101, 299, 300, 301, 599, 600, 1000, 1001, 4096]
    cases = [list(s) + [B] for s in shapes for B in sizes]
    moved = [("set", "set_fwd_split_t2_min_tiles", 256, 0), ("set", "set_bwd_small_max_tiles", 0),
             ("set", "set_train_tile_max_tiles", 0), ("set", "set_fwd_split_max_states", 0)]
    restored = [("set", "set_fwd_split_t2_min_tiles", 256, -1), ("set", "set_bwd_small_max_tiles", None),
                ("set", "set_train_tile_max_tiles", None), ("set", "set_fwd_split_max_states", None)]
    got = _child(env, cases + moved + cases + restored + cases)
    n = len(cases)
    want = [expected(*c, k=k) for c in cases]
    assert got[:n] == want
    assert got[n:2 * n] == [expected(*c, k=dict(k, t2=0, small=0, train_tile=0, fwd_split=0)) for c in cases]
    assert got[2 * n:] == want
    # PPO_BWD_SPLIT_BF16=0 at load: -1 restores off
    c = ["f32", 72, 256, 2, 32, False, 4096]
    got = _child({"PPO_BWD_SPLIT_BF16": "0"}, [c, ("set", "set_bwd_split_bf16", 1), c, ("set", "set_bwd_split_bf16", None), c])
    assert got == [expected(*c, k=dict(DEFAULT, split=0)), expected(*c), expected(*c, k=dict(DEFAULT, split=0))]
