"""The reductions, the scan and the compaction behind the numbers a PPO user reads, at the sizes where their branches open
(tests/bookkeeping_ref.py names them; tests/test_bookkeeping_host.py checks that the tables reach every branch):

1. the truncation compaction (csrc/ppo_gae_boot.hip) through ppo_debug_compact_flags against np.flatnonzero, up to 1025 blocks;
2. the three statistics reductions (csrc/ppo_stats.hip) through their debug entry points against the fixed-order restatement:
   value-clip sums and value moments bit for bit, the ratio kernel's counts exactly and its two log sums within
   train_stats_ref.sum_bound, from one element to the capped grid;
3. ppo_loss_with_entropy and categorical_sample against the CPU oracle at batch sizes around their block sizes, A = 128 and 512;
4. one buffer of 2048 envs x 129 steps (258 compaction blocks, 65 reduction blocks) through the public path.

TEST_RECORD_DIR=<dir>: append what every case measured to <dir>/bookkeeping_sizes.jsonl."""
import ctypes as C
import json
import os
import time

import numpy as np
import pytest

import bookkeeping_ref as ref
import gae_boot_ref
import train_stats_ref

pytestmark = pytest.mark.gpu

GAMMA, LAM = 0.99, 0.95


def _record(rec):
    print(json.dumps(rec))
    d = os.environ.get("TEST_RECORD_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "bookkeeping_sizes.jsonl"), "a") as f:
            f.write(json.dumps(rec) + "\n")


@pytest.fixture(scope="module")
def P(ppo):
    if ppo.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests must run on the GPU box")
    t0 = time.time()
    yield ppo
    ppo.set_rollout_compact(None)
    _record(dict(case="total", seconds=round(time.time() - t0, 2)))


def _debug(P):
    L = P._lib.lib()
    for name, args in (("ppo_debug_ratio_stats", [C.c_void_p, C.c_int64, C.c_double, C.c_void_p]),
                       ("ppo_debug_value_clip_stats", [C.c_void_p, C.c_int64, C.c_float, C.c_void_p]),
                       ("ppo_debug_value_moments", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
                       ("ppo_debug_compact_flags", [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
                       ("ppo_debug_train_ratios", [C.c_void_p, C.c_int64, C.c_void_p])):
        getattr(L, name).argtypes = args
        getattr(L, name).restype = C.c_int32
    return L


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


# ---------------------------------------------------------------- 1. compaction
def _compact(P, flags):
    n = flags.size
    ids = np.full(n, 7, np.int32)
    K = C.c_int64(-5)
    assert _debug(P).ppo_debug_compact_flags(flags.ctypes.data, n, ids.ctypes.data, C.byref(K)) == 0, P._lib.last_error()
    return K.value, ids


@pytest.mark.parametrize("n", ref.COMPACT_SIZES)
def test_compaction_against_flatnonzero(P, n):
    geo = ref.compact_geometry(n)
    for pattern in ref.patterns_for(n):
        flags = ref.flags_case(n, pattern)
        K_ref, ids_ref = ref.compact_ref(flags)
        K, ids = _compact(P, flags)
        _record(dict(case="compact", n=n, pattern=pattern, K=K, K_ref=K_ref, blocks=geo["blocks"], chunks=geo["chunks"],
                     last_width=geo["last_width"], wrong=int(np.count_nonzero(ids != ids_ref))))
        assert K == K_ref, (pattern, K, K_ref)
        assert np.array_equal(ids[:K], ids_ref[:K]), (pattern, int(np.flatnonzero(ids[:K] != ids_ref[:K])[0]))
        assert np.all(ids[K:] == -1), (pattern, "a write behind the K-th entry")
        K2, ids2 = _compact(P, flags)
        assert K2 == K and ids2.tobytes() == ids.tobytes(), (pattern, "a second call repeats the first")


# ---------------------------------------------------------------- 2. the three reductions
@pytest.mark.parametrize("n", ref.STATS_SIZES)
def test_ratio_stats(P, n):
    r, eps = ref.ratio_case(n)
    L = _debug(P)
    out, again = np.full(4, np.nan), np.full(4, np.nan)
    assert L.ppo_debug_ratio_stats(r.ctypes.data, n, eps, out.ctypes.data) == 0, P._lib.last_error()
    assert L.ppo_debug_ratio_stats(r.ctypes.data, n, eps, again.ctypes.data) == 0, P._lib.last_error()
    s1, s3, c, cnt = ref.ratio_sums(r, eps)
    b1, b3 = train_stats_ref.sum_bound(r)
    m1, m3 = ref.ratio_margin(r, eps)
    g = ref.stats_geometry(n)
    _record(dict(case="ratio", n=n, blocks=g["blocks"], finish_passes=g["finish_passes"], tail=g["tail"], err_old_kl=abs(out[0] - s1),
                 bound_old_kl=b1, err_kl=abs(out[1] - s3), bound_kl=b3, min_term_over_bound=[m1, m3], clipped=out[2], n_dev=out[3]))
    assert m1 >= 100 and m3 >= 100
    assert out[3] == n == cnt, "the element count is exact"
    assert out[2] == c == np.count_nonzero(np.abs(r.astype(np.float64) - 1.0) > eps), "the clip count is exact"
    assert abs(out[0] - s1) <= b1, (out[0] - s1, b1)
    assert abs(out[1] - s3) <= b3, (out[1] - s3, b3)
    assert _bits(out).tobytes() == _bits(again).tobytes()


@pytest.mark.parametrize("n", ref.STATS_SIZES)
def test_value_clip_stats(P, n):
    d = ref.value_clip_case(n)
    L = _debug(P)
    g = ref.stats_geometry(n)
    for c in (ref.VCLIP_C, np.float32(np.inf)):
        out, again = np.full(3, np.nan), np.full(3, np.nan)
        assert L.ppo_debug_value_clip_stats(d.ctypes.data, n, float(c), out.ctypes.data) == 0, P._lib.last_error()
        assert L.ppo_debug_value_clip_stats(d.ctypes.data, n, float(c), again.ctypes.data) == 0, P._lib.last_error()
        want = np.array(ref.value_clip_sums(d, c))
        _record(dict(case="value_clip", n=n, c=float(c), blocks=g["blocks"], finish_passes=g["finish_passes"], tail=g["tail"],
                     dev=out.tolist(), ref=want.tolist(), bit_equal=bool(np.array_equal(_bits(out), _bits(want)))))
        assert np.array_equal(_bits(out), _bits(want)), (float(c), out, want)
        assert out[2] == n and (out[0] == 0 if np.isinf(c) else out[0] == np.count_nonzero(np.abs(d) > c))
        assert _bits(out).tobytes() == _bits(again).tobytes()


@pytest.mark.parametrize("n", ref.STATS_SIZES)
def test_value_moments(P, n):
    L = _debug(P)
    g = ref.stats_geometry(n)
    for mask in ref.MASKS:
        t, v, valid, i0 = ref.moments_case(n, mask)
        out, again = np.full(5, np.nan), np.full(5, np.nan)
        assert L.ppo_debug_value_moments(t.ctypes.data, v.ctypes.data, valid.ctypes.data, i0, n, out.ctypes.data) == 0, P._lib.last_error()
        assert L.ppo_debug_value_moments(t.ctypes.data, v.ctypes.data, valid.ctypes.data, i0, n, again.ctypes.data) == 0, P._lib.last_error()
        want = np.array(ref.moment_sums(t, v, valid, i0))
        _record(dict(case="moments", n=n, mask=mask, first_id=i0, blocks=g["blocks"], finish_passes=g["finish_passes"], tail=g["tail"],
                     dev=out.tolist(), ref=want.tolist(), bit_equal=bool(np.array_equal(_bits(out), _bits(want)))))
        assert np.array_equal(_bits(out), _bits(want)), (mask, out, want)
        assert out[0] == np.count_nonzero(valid)
        assert _bits(out).tobytes() == _bits(again).tobytes()


# ---------------------------------------------------------------- 3. the standalone loss and the sampler
@pytest.mark.parametrize("A", ref.LOSS_A)
@pytest.mark.parametrize("B", ref.LOSS_B)
def test_loss_with_entropy(P, orc, B, A):
    probs, a1, p_old, adv = ref.loss_case(B, A)
    lin = P.get_linear_action_index(a1, A)
    assert np.array_equal(lin, a1 + np.arange(B) * A)
    lp, le = P.ppo_loss_with_entropy(probs.T, lin, p_old, adv, 0.05)
    olp, ole = orc.ppo_loss_with_entropy(probs, lin, p_old, adv, 0.05)
    _record(dict(case="loss", B=B, A=A, err_ppo=abs(lp - olp), bar_ppo=1e-6 * (1 + abs(olp)), err_entropy=abs(le - ole),
                 bar_entropy=1e-5 * (1 + abs(ole))))
    assert abs(lp - olp) <= 1e-6 * (1 + abs(olp)), (lp, olp)
    assert abs(le - ole) <= 1e-5 * (1 + abs(ole)), (le, ole)
    assert P.ppo_loss_with_entropy(probs.T, lin, p_old, adv, 0.05) == (lp, le)


@pytest.mark.parametrize("A", ref.LOSS_A)
@pytest.mark.parametrize("B", ref.LOSS_B)
def test_categorical_sample(P, orc, B, A):
    p, u = ref.sampler_case(B, A)
    a, ps, err = P.categorical_sample(p, u)
    want = [orc.categorical_sample(p[b], u[b]) for b in range(B)]
    oa, oerr = np.array([w[0] for w in want]), np.array([w[1] for w in want])
    _record(dict(case="sampler", B=B, A=A, wrong=int(np.count_nonzero(a != oa + 1)), off_the_end=int(oerr.sum())))
    assert np.array_equal(a, oa + 1) and np.array_equal(err, oerr)
    assert ps.tobytes() == p[np.arange(B), oa].tobytes()
    assert err[0] == 1 and a[0] == A, "row 0 walks off the end"


# ---------------------------------------------------------------- 4. one buffer through the public path
PUB_N, PUB_T, PUB_SAMPLES = 2048, 129, 2000


@pytest.fixture(scope="module")
def big(P):
    """2048 envs x 129 steps from compact storage: 264,192 transitions = 258 compaction blocks (two scan chunks) and 65
    reduction blocks (two passes of the finishing wave)."""
    P.set_rollout_compact(1)
    env = P.HipVecEnv(num_envs=PUB_N, Q=8, max_actions=7, seed=31)
    pol = P.HipPolicy(72, 128, 2, 4, seed=2)
    critic = P.HipCritic(72, 128, 2, seed=5)
    rng = np.random.default_rng(77)
    critic.params = (critic.params + (rng.normal(size=critic.num_params) * 0.03).astype(np.float32)).astype(np.float32)
    ro = P.BufferRollouts()
    P.collect_rollouts_steps_(ro, env, pol, PUB_T, GAMMA)
    assert ro.dims() == (PUB_T, PUB_N)
    assert ref.compact_geometry(PUB_T * PUB_N)["blocks"] == 258 and ref.stats_geometry(PUB_T * PUB_N)["blocks"] == 65
    flags, fst, fact = P.truncated_transitions_(ro)
    yield dict(env=env, pol=pol, critic=critic, ro=ro, flags=flags, fst=fst, fact=fact)
    P.set_rollout_compact(None)


def test_public_truncations_against_replay(P, orc, big):
    ro, flags, fst, fact = big["ro"], big["flags"], big["fst"], big["fact"]
    n = PUB_T * PUB_N
    rng = np.random.default_rng(5)
    ends = (ro.terminal & ro.valid).reshape(-1)
    f = flags.reshape(-1)
    ids = np.flatnonzero(f)
    K = ids.size
    assert fst.shape == (K, 32, 72) and fact.shape == (K,) and K == int(f.sum())
    assert not f[~ends].any() and PUB_N * (PUB_T // 7) // 2 <= K <= int(ends.sum())
    # the sampled positions: the first, the last, both sides of the second scan chunk's first transition id, 2000 others
    k0 = int(np.searchsorted(ids, ref.SCAN_CHUNK * ref.CP_BLOCK))
    assert 0 < k0 < K and ids[k0 - 1] < ref.SCAN_CHUNK * ref.CP_BLOCK <= ids[k0]
    ks = np.unique(np.concatenate([[0, K - 1, k0 - 2, k0 - 1, k0, k0 + 1], rng.choice(K, PUB_SAMPLES, replace=False)]))
    end_ids = np.flatnonzero(ends)
    sampled_ends = np.unique(np.concatenate([end_ids[[0, -1]], rng.choice(end_ids, PUB_SAMPLES, replace=False)]))
    need = np.unique(np.concatenate([sampled_ends, ids[ks]]))
    # the stored states of those transitions only, through the dataset's getindex (steps mode: dataset order = storage order)
    index = ro.index()
    assert index.size == n and np.array_equal(index, np.arange(n))
    ds = P.construct_dataset(ro)
    got = ds[need + 1]
    states, active, a0 = got["state"].vertex_score, got["state"].action_mask, np.asarray(got["selected_action"]) - 1
    at = {int(t): j for j, t in enumerate(need)}
    rp = gae_boot_ref.Replay(orc, 8)

    def replay(t):
        j = at[int(t)]
        sc, dg = gae_boot_ref.state_from_observation(states[j], active[j])
        return rp.step(sc, dg, active[j], a0[j])

    wrong_flags = sum(int(replay(t)[0] != bool(f[t])) for t in sampled_ends)
    wrong_states = 0
    for k in ks:
        tr, obs, act, _ = replay(ids[k])
        wrong_states += int(not tr or obs.tobytes() != fst[k].tobytes() or act != fact[k])
    _record(dict(case="public_truncations", n=n, K=K, ends=int(ends.sum()), blocks=258, first_position_of_chunk_2=k0,
                 sampled_ends=int(sampled_ends.size), sampled_truncations=int(f[sampled_ends].sum()), wrong_flags=wrong_flags,
                 sampled_positions=int(ks.size), wrong_states=wrong_states))
    assert wrong_flags == 0 and wrong_states == 0
    assert f[sampled_ends].any()


def test_public_gae_bootstrap(P, big):
    ro, env, critic, flags = big["ro"], big["env"], big["critic"], big["flags"]
    adv, ret = P.compute_gae_critic_(ro, env, critic, GAMMA, LAM, bootstrap_truncated=True)
    boot = ro.boot_values
    K = int(flags.sum())
    assert ro.n_truncated == K
    vfin = P.batch_state_values(critic, P.StateData(big["fst"], big["fact"]))
    wrong = int(np.count_nonzero(boot[flags].view(np.uint32) != vfin.view(np.uint32)))
    v = P.compute_values_(ro, env, critic)
    a64, r64 = gae_boot_ref.gae_boot(ro.raw_rewards, ro.terminal, v, boot, GAMMA, LAM)
    _record(dict(case="public_gae", K=K, boot_wrong=wrong, boot_nonzero_outside=int(np.count_nonzero(boot[~flags])),
                 adv_wrong=int(np.count_nonzero(adv.view(np.uint32) != a64.view(np.uint32))),
                 ret_wrong=int(np.count_nonzero(ret.view(np.uint32) != r64.view(np.uint32)))))
    assert wrong == 0 and np.count_nonzero(vfin) >= K // 2
    assert not boot[~flags].any()
    assert adv.tobytes() == a64.tobytes() and ret.tobytes() == r64.tobytes()
    # the moments over this buffer: 65 blocks, bit for bit against the restatement
    sums = np.zeros(5, np.float64)
    assert P._lib.lib().ppo_rollouts_value_moments(ro._h, P.VALUE_TARGETS["lambda_returns"], sums.ctypes.data_as(P._lib.c_f64p)) == 0
    i0 = int(ro.index()[0])
    want = np.array(ref.moment_sums(ret, v[:PUB_T], ro.valid, i0))
    _record(dict(case="public_moments", n=PUB_T * PUB_N, blocks=65, dev=sums.tolist(), ref=want.tolist(),
                 bit_equal=bool(np.array_equal(_bits(sums), _bits(want)))))
    assert np.array_equal(_bits(sums), _bits(want)), (sums, want)


def test_public_epoch_statistics(P, big):
    """One epoch in slices of 65536 (four full and a ragged fifth of 2048) with parameters that never move: the statistics of
    the epoch are those of the ratio column it left (as tests/test_gpu_train_stats.py::test_epoch_reduction_against_numpy)."""
    ro = big["ro"]
    n = PUB_T * PUB_N
    rng = np.random.default_rng(9)
    pol = P.HipPolicy(72, 128, 2, 4, seed=2)
    pol.params = (pol.params + (rng.normal(size=pol.num_params) * 0.01).astype(np.float32)).astype(np.float32)
    pol.target_kl = float("inf")
    p0 = pol.params.copy()
    ds = P.construct_dataset(ro)
    assert len(ds) == n
    perm = (rng.permutation(n) + 1)[None, :]
    eps = 0.05
    P.ppo_train_(pol, P.Optimiser(P.Descent(0.0)), ds, eps, 65536, 1, 0.01, perm=perm, verbose=False)
    assert np.array_equal(pol.params, p0)
    st = pol.last_train_stats()
    assert st["epochs_run"] == 1 and not st["stopped_early"]
    r = np.zeros(n, np.float32)
    assert _debug(P).ppo_debug_train_ratios(pol._h, n, r.ctypes.data) == 0, P._lib.last_error()
    assert np.all(np.isfinite(r)) and np.all(r > 0) and np.unique(r).size > n // 8
    s1, s3, c, _ = train_stats_ref.ratio_sums(r, eps)
    b1, b3 = train_stats_ref.sum_bound(r)
    _record(dict(case="public_epoch", n=n, blocks=65, clip_fraction=st["clip_fraction"][0], err_kl=abs(st["approx_kl"][0] * n - s3),
                 bound_kl=b3, err_old_kl=abs(st["old_approx_kl"][0] * n - s1), bound_old_kl=b1))
    assert 0 < c < n
    assert abs(st["clip_fraction"][0] * n - c) <= 1e-6, "the clip count is exact (the fraction is one fp64 division of it)"
    assert abs(st["old_approx_kl"][0] * n - s1) <= b1 and abs(st["approx_kl"][0] * n - s3) <= b3
