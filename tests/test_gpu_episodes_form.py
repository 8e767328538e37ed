"""The whole-episode rollout form (ppo_collect_rollouts_episodes) and the evaluators on it (ppo_average_returns,
ppo_evaluate_trajectories, ppo_average_best_returns, ppo_average_normalized_returns) against the CPU oracle, at the sizes
where their pieces can go wrong: more than one block of k_env_step, idle envs, quota boundaries inside a block and a wave,
all three per-step rollout kernels, ragged columns, Q = 32, HID = 256, three hidden layers, bf16, both storage forms.
tests/episodes_ref.py holds the reference and the case tables; tests/test_episodes_host.py checks both without a device.

1. rollouts, fp32: structure, index, every column of every env against the teacher-forced replay, actions and
   probabilities of the replayed columns against the oracle's own rollout, returns against the env-major flat scan; then a
   second episodes-form call and a steps-form call on the same env;
2. rollouts, bf16: against the device's own steps form;
3. a minibatch and a dataset read that straddle column ends of a ragged buffer;
4. the three evaluators, per trajectory and as (mean, std).

TEST_RECORD_DIR=<dir>: append what every case measured to <dir>/episodes_form.jsonl."""
import json
import os
import time

import numpy as np
import pytest

import episodes_ref as ref

pytestmark = pytest.mark.gpu

BAR = 2e-5                                   # the bar of every fp32 gradient test of the project
STEPS_AFTER = 5                              # rows of the steps-form call that follows the two episodes-form calls


def _record(rec):
    print(json.dumps(rec))
    d = os.environ.get("TEST_RECORD_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "episodes_form.jsonl"), "a") as f:
            f.write(json.dumps(rec) + "\n")


@pytest.fixture(scope="module")
def P(ppo):
    if ppo.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests must run on the GPU box")
    t0 = time.time()
    yield ppo
    _record(dict(case="total", seconds=round(time.time() - t0, 2)))


@pytest.fixture
def knobs(P):
    yield P
    P.set_rollout_compact(None)
    P.set_rollout_persistent(None)


def _policy(P, orc, case, dtype="f32"):
    pol = P.HipPolicy(ref.F, case["hid"], case["L"], 4, seed=0, dtype=dtype)
    pol.params = ref.policy_params(orc, case)
    return pol


def _columns(ro):
    st, act = ro.state_data
    return dict(states=st, active=act, actions=(ro.selected_actions - 1).astype(np.int32),
                p_sel=ro.selected_action_probabilities, rewards=ro.raw_rewards, done=ro.terminal, returns=ro.rewards)


def _structure(case, ro, num_episodes):
    """What holds for every episodes-form buffer, whatever played it.  Returns (valid, terminal, raw rewards, index)."""
    N, M = case["N"], case["M"]
    Tmax = -(-num_episodes // N) * M
    T, n_ = ro.dims()
    valid, term, raw = ro.valid, ro.terminal, ro.raw_rewards
    lens = valid.sum(axis=0)
    assert n_ == N and valid.shape == (T, N)
    assert T == min(Tmax, -(-int(lens.max()) // 8) * 8), "rows: up to the first poll (every 8 steps) that finds every quota used"
    assert np.array_equal(valid, np.arange(T)[:, None] < lens[None, :]), "valid flags form a prefix of every column"
    busy = np.flatnonzero(lens)
    assert term[lens[busy] - 1, busy].all(), "every column ends on a terminal"
    assert np.array_equal((valid & term).sum(axis=0), ref.quotas(N, num_episodes))
    assert len(ro) == int(valid.sum())
    assert not raw[~valid].any() and term[~valid].all(), "an invalid row has reward 0 and terminal 1"
    index = ro.index()
    assert np.array_equal(index, ref.env_major_index(valid))
    return valid, term, raw, index


def _episode_lengths(valid, term):
    out = []
    for n in range(valid.shape[1]):
        ends = np.flatnonzero(term[:, n] & valid[:, n]) + 1
        out.extend(np.diff(np.concatenate([[0], ends])).tolist())
    return np.array(out, np.int64)


def _check_call(orc, case, env, ro, exp, num_episodes, discount, what, episode0=None, tick0=None):
    """One episodes-form call against the reference.  exp: expected_episodes of the replayed columns."""
    kw = ref.env_kw_of(case)
    valid, term, raw, index = _structure(case, ro, num_episodes)
    got = _columns(ro)
    rec = ref.teacher_forced(orc, kw, got["actions"], num_episodes, episode0, tick0)
    bad = dict(valid=int(np.count_nonzero(rec["valid"] != valid)))
    for k in ("states", "active", "rewards", "done"):
        a, b = got[k][valid], rec[k][valid]
        bad[k] = int(np.count_nonzero(a.view(np.uint8) != b.astype(a.dtype).view(np.uint8)))
    lens = valid.sum(axis=0)
    bad["length"] = bad["actions"] = bad["p_sel"] = bad["replayed_states"] = 0
    for n, col in exp.items():
        k = col["length"]
        if lens[n] != k:
            bad["length"] += 1
            continue
        bad["actions"] += int(np.count_nonzero(got["actions"][:k, n] != col["actions"]))
        bad["p_sel"] += int(np.count_nonzero(got["p_sel"][:k, n].view(np.uint32) != col["p_sel"].view(np.uint32)))
        bad["replayed_states"] += int(got["states"][:k, n].tobytes() != col["states"].tobytes())
        bad["length"] += int(rec["episode"][n] != col["episode_after"] or rec["tick"][n] != col["tick_after"])
    want = ref.flat_returns(orc, raw, term, index, discount)
    bad["returns"] = int(np.count_nonzero(got["returns"].reshape(-1)[index].view(np.uint32) != want.view(np.uint32)))
    flags = env.error_flags()
    lengths = _episode_lengths(valid, term)
    _record(dict(case=case["name"], call=what, N=case["N"], episodes=num_episodes, T=int(valid.shape[0]), len=len(ro),
                 idle_envs=int((lens == 0).sum()), replayed_columns=len(exp), short_episodes=int((lengths < case["M"]).sum()),
                 discount=float(discount), error_flags=flags, mismatches=bad))
    assert not any(bad.values()), (case["name"], what, bad)
    assert flags & ~32 == 0
    assert lengths.size == num_episodes
    return rec


# ---------------------------------------------------------------- 1. rollouts, fp32
@pytest.mark.parametrize("case,form", ref.ROLLOUT_RUNS, ids=lambda v: v["name"] if isinstance(v, dict) else v)
def test_rollout_against_oracle(P, knobs, orc, case, form):
    P.set_rollout_compact(form == "compact")
    kw, ne, N = ref.env_kw_of(case), case["episodes"], case["N"]
    params = ref.policy_params(orc, case)
    env, pol, ro = P.HipVecEnv(**kw), _policy(P, orc, case), P.BufferRollouts()
    P.collect_rollouts_(ro, env, pol, ne, 1.0)
    exp = ref.reference(orc, case)
    rec = _check_call(orc, case, env, ro, exp, ne, 1.0, "first/" + form)
    lens = rec["valid"].sum(axis=0)
    for n in case["short"]:                                  # the ragged column the case is placed on
        assert exp[n]["done"][:case["M"] - 1].any() and (lens[n] < lens.max() or N == 1)
    # a second call on the same env and buffer: every env is reset, episode counters and ticks continue
    cols = ref.edge_columns(case)
    ep0, tk0 = np.zeros(N, np.int64), np.zeros(N, np.int64)
    for n in cols:
        ep0[n], tk0[n] = exp[n]["episode_after"], exp[n]["tick_after"]
    exp2 = ref.expected_episodes(orc, kw, params, case["hid"], case["L"], ne, cols, ep0, tk0)
    P.collect_rollouts_(ro, env, pol, ne, 0.99)
    rec2 = _check_call(orc, case, env, ro, exp2, ne, 0.99, "second/" + form, rec["episode"], rec["tick"])
    # then the steps form: the envs that finished their quota are reset, the ones that never played go on unplayed
    P.collect_rollouts_steps_(ro, env, pol, STEPS_AFTER, 1.0)
    ep, tk = rec2["episode"].copy(), rec2["tick"].copy()
    for n in cols:
        ep[n], tk[n] = exp2[n]["episode_after"], exp2[n]["tick_after"]
    exp3 = ref.expected_steps(orc, kw, params, case["hid"], case["L"], STEPS_AFTER, cols, ep, tk, rec2["fresh"])
    got = _columns(ro)
    assert ro.dims() == (STEPS_AFTER, N) and len(ro) == STEPS_AFTER * N and ro.valid.all()
    bad = {k: sum(int(got[k][:, n].tobytes() != exp3[n][k].astype(got[k].dtype).tobytes()) for n in cols)
           for k in ("states", "active", "actions", "p_sel", "rewards", "done")}
    tn = orc.compute_returns_tn(got["rewards"], got["done"], 1.0)
    bad["returns"] = int(np.count_nonzero(got["returns"].view(np.uint32) != tn.view(np.uint32)))
    _record(dict(case=case["name"], call="steps/" + form, N=N, T=STEPS_AFTER, replayed_columns=len(cols),
                 never_played=int(rec2["fresh"].sum()), mismatches=bad))
    assert not any(bad.values()), (case["name"], bad)
    assert env.error_flags() & ~32 == 0


# ---------------------------------------------------------------- 2. rollouts, bf16
@pytest.mark.parametrize("hid", ref.BF16_HID)
def test_rollout_bf16_against_the_steps_form(P, knobs, orc, hid):
    """The bf16 forward is held to its oracle at a tolerance, so the reference of the episode logic is the device's own
    steps form on a fresh identical env (reset once: both start at episode counter 1), launch by launch."""
    case = dict(ref.by_name("70x100"), hid=hid)
    kw, ne = ref.env_kw_of(case), case["episodes"]
    P.set_rollout_persistent(0)
    pol = _policy(P, orc, case, "bf16")
    env, ro = P.HipVecEnv(**kw), P.BufferRollouts()
    P.collect_rollouts_(ro, env, pol, ne, 0.99)
    valid, term, raw, index = _structure(case, ro, ne)
    twin, steps = P.HipVecEnv(**kw), P.BufferRollouts()
    P.reset_(twin)
    P.collect_rollouts_steps_(steps, twin, pol, valid.shape[0], 0.99)
    a, b = _columns(ro), _columns(steps)
    bad = {k: int(np.count_nonzero(a[k][valid].view(np.uint8) != b[k][valid].view(np.uint8))) for k in a}
    lengths = _episode_lengths(valid, term)
    _record(dict(case="bf16-70x100-h%d" % hid, N=70, episodes=ne, T=int(valid.shape[0]), len=len(ro),
                 short_episodes=int((lengths < case["M"]).sum()), mismatches=bad))
    assert not any(bad.values()), bad
    assert (lengths < case["M"]).any() and lengths.size == ne
    assert env.error_flags() & ~32 == 0


# ---------------------------------------------------------------- 3. downstream of a ragged buffer
@pytest.mark.parametrize("form", ref.BOTH)
def test_minibatch_across_column_ends(P, knobs, orc, form):
    """64 dataset indices, two on each side of 16 column ends of the 300-env / 450-episode buffer (the short column's among
    them): ds[[..]] returns the rows the index names, forward_backward differentiates those transitions."""
    case = ref.by_name(ref.DOWNSTREAM)
    kw, ne, N = ref.env_kw_of(case), case["episodes"], case["N"]
    P.set_rollout_compact(form == "compact")
    env, pol, ro = P.HipVecEnv(**kw), _policy(P, orc, case), P.BufferRollouts()
    P.collect_rollouts_(ro, env, pol, ne, 0.99)
    valid, term, raw, index = _structure(case, ro, ne)
    got = _columns(ro)
    rec = ref.teacher_forced(orc, kw, got["actions"], ne)
    ends = np.cumsum(valid.sum(axis=0))                      # 1-based dataset position of every column's last transition
    short = case["short"][0]
    at = sorted({short - 1, short, 0, 1, 63, 64, 100, 148, 149, 150, 151, 200, 255, 256, 296, 297})
    sel = np.unique(np.concatenate([ends[at] + d for d in (-1, 0, 1, 2)]))[:64]
    assert sel.size == 64 and sel.min() >= 1 and sel.max() <= len(ro)
    flat = index[sel - 1]
    assert np.unique(flat % N).size >= 17 and np.unique(flat // N).size >= 4
    ds = P.construct_dataset(ro)
    batch = ds[sel]
    assert batch["state"].vertex_score.tobytes() == rec["states"].reshape(-1, 32, ref.F)[flat].tobytes()
    assert np.array_equal(batch["state"].action_mask, rec["active"].reshape(-1)[flat])
    assert np.array_equal(np.asarray(batch["selected_action"]) - 1, got["actions"].reshape(-1)[flat])
    assert np.array_equal(batch["returns"], ref.flat_returns(orc, raw, term, index, 0.99)[sel - 1])
    rng = np.random.default_rng(3)                           # move the policy off the one that collected: ratios != 1
    pol.params = (pol.params + (rng.normal(size=pol.num_params) * 0.01).astype(np.float32)).astype(np.float32)
    lp, le = P.forward_backward(pol, ds, sel, 0.05, 0.01)
    g = pol.grad()
    g64, olp, ole = orc.step_batch_grad_f64(pol.params, ref.F, case["hid"], rec["states"].reshape(-1, 32, ref.F)[flat],
                                            rec["active"].reshape(-1)[flat], got["actions"].reshape(-1)[flat],
                                            got["p_sel"].reshape(-1)[flat], got["returns"].reshape(-1)[flat], 0.05, 0.01,
                                            n_hidden=case["L"])
    scale = float(np.abs(g64).max())
    err = float(np.abs(g - g64).max())
    _record(dict(case="minibatch/" + form, B=int(sel.size), columns=int(np.unique(flat % N).size), err=err, bar=BAR * scale,
                 err_loss=abs(lp - olp), err_entropy=abs(le - ole)))
    assert scale > 0 and err <= BAR * scale + 1e-9
    assert abs(lp - olp) <= 1e-5 * (1 + abs(olp)) and abs(le - ole) <= 1e-5 * (1 + abs(ole))


# ---------------------------------------------------------------- 4. evaluators
_PLAYED = {}


def _played(P, orc, case):
    """The trajectories the evaluators of this case play are the ones collect_rollouts_ plays on a fresh identical env:
    its teacher-forced record (every column), tied to the oracle on the replayed columns.  Once per case."""
    if case["name"] not in _PLAYED:
        kw, ne = ref.env_kw_of(case), case["episodes"]
        env, pol, ro = P.HipVecEnv(**kw), _policy(P, orc, case), P.BufferRollouts()
        P.collect_rollouts_(ro, env, pol, ne, 1.0)
        _PLAYED[case["name"]] = _check_call(orc, case, env, ro, ref.reference(orc, case), ne, 1.0, "evaluator-record")
    return _PLAYED[case["name"]]


@pytest.mark.parametrize("kind", ["return", "best", "normalized"])
@pytest.mark.parametrize("case", ref.EVAL_CASES, ids=lambda c: c["name"])
def test_evaluators_against_oracle(P, knobs, orc, case, kind):
    kw, nt = ref.env_kw_of(case), case["episodes"]
    rec = _played(P, orc, case)
    skip = ref.normalized_of_skippers(orc, case) if kind == "normalized" else None
    want = ref.evaluator_values(kind, rec, skip)
    assert want.shape == (nt,)
    pol = _policy(P, orc, case)
    env = P.HipVecEnv(**kw)
    got = P.evaluate_trajectories(env, pol, nt, kind)
    assert env.error_flags() & ~32 == 0
    env = P.HipVecEnv(**kw)
    if kind == "return":
        mean, std = P.average_returns(pol, env, nt)
    elif kind == "best":
        mean, std = P.average_best_returns(env, pol, nt)
    else:
        mean, std = P.average_normalized_returns(env, pol, nt)
    skips = int(ref.skip_table(orc, kw, nt).sum()) if kind == "normalized" else 0
    _record(dict(case=case["name"], call="evaluate/" + kind, N=case["N"], episodes=nt, skipping_envs=sorted(skip) if skip else [],
                 skips_taken=skips, mismatches=int(np.count_nonzero(got != want)),
                 err_mean=abs(mean - want.mean()), err_std=abs(std - want.std(ddof=1))))
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    if kind == "normalized":
        assert set(skip) <= set(case["special"]) and (want == 1.0).sum() >= skips
    assert abs(mean - want.mean()) < 1e-9 and abs(std - want.std(ddof=1)) < 1e-9
    assert env.error_flags() & ~32 == 0
