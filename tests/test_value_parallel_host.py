"""The data-parallel critic, as far as a machine without a GPU can see it: ppo_value_train_dp and
ppo_rollouts_value_moments_shifts are declared, bound and exported; the argument checks that read no handle; the merge of the
ranks' explained-variance rows (value_moments_row, explained_variance_from_shards) against numpy float64 over the union; and
ppo_iterate_'s signature with `parallel`."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import train_stats_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"ppo_value_train_dp": 14, "ppo_rollouts_value_moments_shifts": 4}
ERR_ARG = -1


def test_new_functions_declared_bound_exported(ppo):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppo_hip.h")).read(), flags=re.S)
    jl = open(os.path.join(ROOT, "julia", "ProximalPolicyOptimizationHIP.jl")).read()
    L = ppo._lib.lib()
    for name, n in NEW.items():
        m = re.search(r"int32_t\s+%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
        assert m, "%s is not declared in include/ppo_hip.h" % name
        assert m.group(1).count(",") + 1 == n == len(ppo._lib.SIGNATURES[name]), name
        assert hasattr(L, name), "%s is not exported by libppo_hip.so" % name
        assert "(:%s, LIB)" % name in jl, "%s has no ccall in the Julia shim" % name
    # the data-parallel call is ppo_value_train's parameters with ppo_train's four in front of the histories
    assert ppo._lib.SIGNATURES["ppo_value_train_dp"] == (ppo._lib.SIGNATURES["ppo_value_train"][:8] + ppo._lib.SIGNATURES["ppo_train"][10:14]
                                                         + ppo._lib.SIGNATURES["ppo_value_train"][8:])


def test_argument_checks_without_a_device(ppo):
    L = ppo._lib.lib()
    p = ppo._lib
    f64 = np.zeros(2, np.float64)
    h = f64.ctypes.data_as(p.c_f64p)
    no_hook = p.ALLREDUCE_FN(0)
    identity = p.ALLREDUCE_FN(lambda ctx, buf, n: 0)

    def train(epochs, rank, world, hook):
        return L.ppo_value_train_dp(None, None, None, 1, epochs, 0, None, 0, rank, world, hook, None, h, h)

    assert train(1, 0, 2, no_hook) == ERR_ARG
    assert "world > 1 needs an all-reduce hook" in p.last_error()
    assert train(1, 2, 2, identity) == ERR_ARG
    assert "bad epochs/rank/world" in p.last_error()
    assert train(1, -1, 2, identity) == ERR_ARG and "bad epochs/rank/world" in p.last_error()
    assert train(1, 0, 0, identity) == ERR_ARG and "bad epochs/rank/world" in p.last_error()
    assert train(-1, 0, 1, no_hook) == ERR_ARG
    assert "bad epochs/rank/world" in p.last_error()
    # well-formed rank / world: the handles are looked at next, with or without a hook
    for args in ((1, 0, 1, no_hook), (1, 1, 2, identity), (0, 0, 1, identity)):
        assert train(*args) == ERR_ARG
        assert "null" in p.last_error()
    assert L.ppo_value_train(None, None, None, 1, -1, 0, None, 0, h, h) == ERR_ARG
    assert L.ppo_rollouts_value_moments_shifts(None, 0, h, h) == ERR_ARG
    assert "null" in p.last_error()
    assert L.ppo_rollouts_value_moments_shifts(None, 0, h, None) == ERR_ARG
    # an unknown target never reaches the library, with or without `parallel`
    dp = ppo.DataParallel(0, 2)
    for fn in (lambda: ppo.value_train_(None, None, None, 1, 1, target="td0", parallel=dp),
               lambda: ppo.explained_variance_(None, target="td0", parallel=dp)):
        with pytest.raises(ppo.PPOError, match="value target must be one of"):
            fn()


def _row(ppo, t, v, shift_at):
    """A shard's row the way explained_variance_ builds it: the device's five sums, shifted by the shard's transition
    `shift_at`, and the two shifts."""
    sums, _ = ref.value_moments(t, v, np.ones(t.size, np.uint8), shift_at)
    return ppo.value_moments_row(sums, (t[shift_at], t[shift_at] - v[shift_at]))


def _union_ev(t, v):
    return 1.0 - np.var(t - v) / np.var(t)


def test_merge_of_shards_against_the_union(ppo):
    rng = np.random.default_rng(257)
    t = rng.normal(size=257) * 3.0 + 40.0                              # a mean far from zero: the shifts matter
    v = t + rng.normal(size=257) * 0.7 - 0.3
    cuts = [(0, 1), (1, 101), (101, 257)]                              # shards of 1, 100 and 156
    rows = [_row(ppo, t[a:b], v[a:b], s) for (a, b), s in zip(cuts, (0, 37, 155))]
    assert [r[0] for r in rows] == [1.0, 100.0, 156.0]
    assert rows[0][2] == 0.0 and rows[0][4] == 0.0 and rows[0][1] == t[0]
    want = _union_ev(t, v)
    got = ppo.explained_variance_from_shards(rows)
    assert abs(got - want) <= 1e-12, (got, want)
    # every shard's mean and M2 are those of the shard, whatever the shift
    for (a, b), r in zip(cuts, rows):
        d = t[a:b] - v[a:b]
        assert abs(r[1] - t[a:b].mean()) <= 1e-12 and abs(r[3] - d.mean()) <= 1e-12
        assert abs(r[2] - ((t[a:b] - t[a:b].mean()) ** 2).sum()) <= 1e-9 and abs(r[4] - ((d - d.mean()) ** 2).sum()) <= 1e-9
    # as a [world, 5] array, the form the all-reduce hands back, and one shard alone against the single-rank formula
    assert ppo.explained_variance_from_shards(np.array(rows)) == got
    sums, _ = ref.value_moments(t, v, np.ones(257, np.uint8), 12)
    one = ppo.explained_variance_from_shards([ppo.value_moments_row(sums, (t[12], t[12] - v[12]))])
    assert abs(one - want) <= 1e-12 and abs(ppo.explained_variance_from_sums(sums) - want) <= 1e-12
    # an empty shard is skipped, wherever it stands
    empty = ppo.value_moments_row(np.zeros(5), (0.0, 0.0))
    assert empty == (0.0,) * 5
    for at in range(4):
        assert ppo.explained_variance_from_shards(rows[:at] + [empty] + rows[at:]) == got
    assert ppo.explained_variance_from_shards([(0.0, 5.0, 7.0, 1.0, 2.0)] + rows) == got    # n == 0 decides, not the rest
    # the merge differs from the shards' own values: it is not an average of them
    assert abs(ppo.explained_variance_from_shards(rows[1:2]) - want) > 1e-3


def test_merge_without_variance_is_nan(ppo):
    rng = np.random.default_rng(3)
    t = np.full(50, 2.5)
    v = rng.normal(size=50)
    rows = [_row(ppo, t[:20], v[:20], 3), _row(ppo, t[20:], v[20:], 0)]
    assert np.isnan(ppo.explained_variance_from_shards(rows))
    assert np.isnan(ppo.explained_variance_from_shards([]))
    assert np.isnan(ppo.explained_variance_from_shards([(0.0,) * 5, (0.0,) * 5]))
    # two constant shards with DIFFERENT constants do have variance
    rows = [_row(ppo, np.full(20, 1.0), v[:20], 0), _row(ppo, np.full(30, 2.0), v[20:], 0)]
    tt = np.concatenate([np.full(20, 1.0), np.full(30, 2.0)])
    assert abs(ppo.explained_variance_from_shards(rows) - _union_ev(tt, v)) <= 1e-12


def test_ppo_iterate_signature_with_parallel(ppo):
    """The positional parameters and the named keywords are what they were; `parallel` can be passed by keyword only, and no
    other unknown keyword is swallowed."""
    sig = inspect.signature(ppo.ppo_iterate_)
    ps = list(sig.parameters.values())
    assert [p.name for p in ps[:13]] == ["policy", "env", "optimizer", "episodes_per_iteration", "minibatch_size", "num_ppo_iterations",
                                         "evaluator", "epochs_per_iteration", "discount", "epsilon", "entropy_weight", "state_data_path",
                                         "verbose"]
    assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in ps[:13])
    kw = {p.name: p.default for p in ps if p.kind is inspect.Parameter.KEYWORD_ONLY}
    for name, default in {"critic": None, "critic_optimizer": None, "gae_lambda": 0.95, "value_epochs": None}.items():
        assert kw[name] == default
    assert "parallel" not in [p.name for p in ps if p.kind in (inspect.Parameter.POSITIONAL_ONLY, inspect.Parameter.POSITIONAL_OR_KEYWORD)]
    args = [None] * 5 + [0, None, 1, 0.99, 0.05, 0.01, None, False]        # zero iterations: nothing is touched
    sig.bind(*args, parallel=ppo.DataParallel(0, 2))
    with pytest.raises(TypeError):
        sig.bind(*args, ppo.DataParallel(0, 2))                            # a 14th positional argument
    assert ppo.ppo_iterate_(*args, parallel=ppo.DataParallel(0, 2)) == {"ppo": [], "entropy": [], "lr": []}
    assert ppo.ppo_iterate_(*args, parallel=None) == ppo.ppo_iterate_(*args)
    with pytest.raises(TypeError):
        ppo.ppo_iterate_(*args, ppo.DataParallel(0, 2))
    with pytest.raises(TypeError, match="paralel"):
        ppo.ppo_iterate_(*args, paralel=None)
    with pytest.raises(ppo.PPOError, match="disk-backed"):                 # still refused, with or without parallel
        ppo.ppo_iterate_(*(args[:11] + ["/nonexistent", False]), critic=object(), critic_optimizer=object(),
                         parallel=ppo.DataParallel(0, 2))
    for fn in (ppo.value_train_, ppo.explained_variance_, ppo.ppo_train_):
        assert inspect.signature(fn).parameters["parallel"].default is None
