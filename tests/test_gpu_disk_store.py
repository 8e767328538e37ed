"""The out-of-core rollout store (csrc/ppo_disk.hip) byte for byte and through its write failures.

In process: rollout.bin of a streamed collection equals tests/disk_store_ref.py's encode() of the memory-resident collection
of the same seed (snapshots: the CPU env replayed under its actions) through every branch of the pinned ring, a sink reused for
a second collection of another length and storage form, and the loader against damaged copies of a good file.

In one fresh child process (this file run as a script, never an exec of the running process): write failures, injected as a
soft RLIMIT_FSIZE around the call under test -- a host I/O error, nothing on the device is involved.  The contract
(include/ppo_hip.h): the synchronous collection fails itself, a failed deferred finish is reported once by the first wait
point, the directory never yields a dataset afterwards, and the engine stays usable.  A second child runs with
PPO_DISK_ASYNC=1 in its environment and never calls set_disk_async.

TEST_RECORD_DIR=<dir>: one line per case goes to <dir>/disk_store.jsonl.
DISK_STORE_PACKAGE_ROOT=<checkout> (child only): run the cases against the package of another checkout (A/B)."""
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import disk_store_ref as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, HID, MAXA, SEED, PSEED, GAMMA = 96, 128, 9, 21, 4, 0.99
WRITE_FAILED = re.compile(r"write.*failed", re.I | re.S)


def _record(**kw):
    d = os.environ.get("TEST_RECORD_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "disk_store.jsonl"), "a") as f:
            f.write(json.dumps(kw) + "\n")


def _env_kw(Q):
    return dict(num_envs=N, Q=Q, max_actions=MAXA, seed=SEED)


def _fresh(P, Q=8):
    return P.HipVecEnv(**_env_kw(Q)), P.HipPolicy(72, HID, 2, 4, seed=PSEED)


_EXPECT = {}


def expected_blobs(P, orc, Q, lengths):
    """encode() of consecutive collections of `lengths` steps on one fresh env and policy: {(k, version): bytes}.  Every column
    but the snapshots from memory-resident collections, the snapshots from the CPU env replayed over all of them."""
    key = (Q, tuple(lengths))
    if key not in _EXPECT:
        env, pol = _fresh(P, Q)
        cols = []
        for T in lengths:
            ro = P.BufferRollouts()
            P.collect_rollouts_steps_(ro, env, pol, T, GAMMA)
            cols.append(D.columns_from_memory(orc, _env_kw(Q), ro, 1))
        assert env.error_flags() & ~32 == 0
        cat = {k: np.concatenate([c[k] for c in cols]) for k in ("actions", "active", "rewards", "done")}
        snap = D.replay_snapshots(orc, _env_kw(Q), cat["actions"], check=cat)
        out, t0 = {}, 0
        for k, c in enumerate(cols):
            out[(k, 1)] = D.encode(c, 1)
            c2 = dict(c, states=snap[t0:t0 + c["T"]], template=D.template_table(orc, Q))
            out[(k, 2)] = D.encode(c2, 2)
            t0 += c["T"]
        _EXPECT[key] = out
    return _EXPECT[key]


def _first_difference(got, want):
    if len(got) != len(want):
        return "%d bytes, expected %d" % (len(got), len(want))
    i = next(i for i in range(len(got)) if got[i] != want[i])
    return "first differing byte at offset %d of %d" % (i, len(got))


class _environ:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ================================================================ in process: byte for byte through the ring
@pytest.fixture()
def P(ppo):
    if ppo.device_count() == 0:
        pytest.skip("no GPU")
    yield ppo
    ppo.set_disk_async(None)
    ppo.set_rollout_compact(None)
    ppo.set_rollout_persistent(None)


def _case(form, slots, T, Q=8, persistent=None, batch=None, deferred=False, fit3=False):
    return dict(form=form, slots=slots, T=T, Q=Q, persistent=persistent, batch=batch, deferred=deferred, fit3=fit3)


def _case_id(c):
    s = "%s-q%d-ring%d-T%d" % (c["form"], c["Q"], c["slots"], c["T"])
    s += {None: "", 1: "-one_launch", 0: "-per_step"}[c["persistent"]]
    s += "" if c["batch"] is None else "-batch%d" % c["batch"]
    return s + ("-deferred" if c["deferred"] else "") + ("-fit3" if c["fit3"] else "")


# ring 2, 3, 5, 64 x T in {1, ring-1, ring, ring+1, 2*ring+1, 20}: T below the ring, a wrap exactly at the ring, an odd ring, a
# last persistent chunk shorter than the others (chunk = min(ring / 2, 8): T = 11 at ring 5, 129 and 20 at ring 64); both forms,
# Q = 32 in both, one launch on / off, PPO_DISK_BATCH unset / 1 / beyond the ring, the deferred finish with the ring grown to T
# and (fit3) with PPO_DISK_ASYNC_MAX_BYTES letting 3 records in, so that it runs behind back-pressure
RING_CASES = [
    _case("snapshot", 2, 1),
    _case("snapshot", 2, 2, persistent=1, batch=1),
    _case("snapshot", 2, 3, persistent=0),
    _case("snapshot", 2, 5, deferred=True),
    _case("snapshot", 2, 20, deferred=True, fit3=True),
    _case("expanded", 2, 20, persistent=0, batch=100),
    _case("snapshot", 3, 2),
    _case("expanded", 3, 3, deferred=True),
    _case("snapshot", 3, 4, persistent=1, batch=1),
    _case("snapshot", 3, 7, batch=100),
    _case("snapshot", 3, 20, persistent=0, deferred=True, fit3=True),
    _case("snapshot", 5, 4),
    _case("expanded", 5, 5, persistent=1),
    _case("snapshot", 5, 6, deferred=True),
    _case("snapshot", 5, 11, batch=1),
    _case("expanded", 5, 20, deferred=True, fit3=True),
    _case("snapshot", 64, 1, deferred=True),
    _case("snapshot", 64, 63),
    _case("snapshot", 64, 64, deferred=True, batch=100),
    _case("snapshot", 64, 65, persistent=0),
    _case("snapshot", 64, 129, persistent=1),
    _case("snapshot", 64, 20, persistent=1),
    _case("snapshot", 5, 20, Q=32),
    _case("expanded", 3, 7, Q=32, deferred=True),
]
assert len(RING_CASES) <= 24


@pytest.mark.parametrize("c", RING_CASES, ids=_case_id)
def test_file_is_the_restatement_byte_for_byte(P, orc, tmp_path, c):
    version = 2 if c["form"] == "snapshot" else 1
    want = expected_blobs(P, orc, c["Q"], [c["T"]])[(0, version)]
    rec = D.record_bytes(version, N, 4 * c["Q"], 72, 4 * c["Q"])
    if c["form"] == "expanded":
        P.set_rollout_compact(False)
    P.set_rollout_persistent(c["persistent"])
    P.set_disk_async(c["deferred"])
    env, pol = _fresh(P, c["Q"])
    disk = P.DiskRollouts(str(tmp_path / "store"))
    with _environ(PPO_DISK_BATCH=c["batch"], PPO_DISK_ASYNC_MAX_BYTES=3 * rec + rec // 2 if c["fit3"] else None):
        P.collect_rollouts_steps_(disk, env, pol, c["T"], GAMMA, pinned_slots=c["slots"])
        P.disk_sync(disk)
    got = D.read(D.rollout_bin(disk.state_data_directory))
    same = got == want
    _record(test="byte_for_byte", case=_case_id(c), bytes=len(got), same=same)
    assert same, _first_difference(got, want)
    assert len(got) == D.file_bytes(version, N, 4 * c["Q"], 72, 4 * c["Q"], c["T"])
    assert env.error_flags() & ~32 == 0


@pytest.mark.parametrize("order", ["snapshot20_then_expanded7", "expanded5_then_snapshot20"])
def test_one_sink_reused_for_another_length_and_form(P, orc, tmp_path, order):
    """One attach, two ppo_collect_rollouts into the same buffer in deferred mode: the second has another T (the ring is
    rebuilt) and the other storage form (the records are re-obtained), and its begin is what settles the first's deferred
    finish.  After ppo_rollouts_disk_sync the file is the second collection's."""
    (f1, T1), (f2, T2) = {"snapshot20_then_expanded7": ((2, 20), (1, 7)), "expanded5_then_snapshot20": ((1, 5), (2, 20))}[order]
    want = expected_blobs(P, orc, 8, [T1, T2])
    env, pol = _fresh(P)
    dev = P.BufferRollouts()
    h = dev._ensure(env, 0)
    d = str(tmp_path / "store")
    P.call("ppo_rollouts_attach_disk", h, d.encode(), 2)
    P.set_disk_async(True)
    P.set_rollout_compact(f1 == 2)
    P.call("ppo_collect_rollouts", h, env._h, pol._h, T1, GAMMA, 0, 0)
    P.set_rollout_compact(f2 == 2)
    P.call("ppo_collect_rollouts", h, env._h, pol._h, T2, GAMMA, 0, 0)
    P.call("ppo_rollouts_disk_sync", h)
    got = D.read(D.rollout_bin(d))
    _record(test="reuse", case=order, bytes=len(got), same=got == want[(1, f2)])
    assert got == want[(1, f2)], _first_difference(got, want[(1, f2)])
    # and once more into the same sink, synchronously, the first collection's shape again (the ring shrinks back)
    P.set_disk_async(False)
    P.set_rollout_compact(f1 == 2)
    env, pol = _fresh(P)
    P.call("ppo_collect_rollouts", h, env._h, pol._h, T1, GAMMA, 0, 0)
    P.call("ppo_rollouts_detach_disk", h)
    got = D.read(D.rollout_bin(d))
    assert got == want[(0, f1)], _first_difference(got, want[(0, f1)])


def _columns_of(ro):
    st, act = ro.state_data
    return [st, act, ro.selected_actions, ro.selected_action_probabilities, ro.rewards, ro.raw_rewards, ro.terminal]


def test_loader_refuses_damaged_files_and_keeps_the_buffer(P, orc, tmp_path):
    T, Tprev = 6, 4
    blobs = expected_blobs(P, orc, 8, [T])
    good = blobs[(0, 2)]
    hdr, rec = D.header_bytes(2), D.record_bytes(2, N, 32, 72, 32)
    ret0 = hdr + T * rec
    for form in (2, 1):                                           # the restatement's own bytes load: the loader reads this format
        P.set_rollout_compact(form == 2)
        env, pol = _fresh(P)
        disk = P.DiskRollouts(str(tmp_path / ("engine%d" % form)))
        P.collect_rollouts_steps_(disk, env, pol, T, GAMMA, pinned_slots=3)
        assert D.read(D.rollout_bin(disk.state_data_directory)) == blobs[(0, form)]
    P.set_rollout_compact(None)

    def flip(b, at, bit=0):
        return b[:at] + bytes([b[at] ^ (1 << bit)]) + b[at + 1:]
    damaged = {
        "truncated_in_header": (good[:20], "bad header"),
        "truncated_in_tag": (good[:hdr - 5], "bad header"),
        "truncated_in_record_3": (good[:hdr + 3 * rec + rec // 3], "truncated"),
        "truncated_at_returns": (good[:ret0], "returns column missing"),
        "truncated_one_byte_short": (good[:-1], "returns column missing"),
        "wrong_magic": (b"PPOS" + good[4:], "bad header"),
        "version_7": (good[:4] + bytes([7, 0, 0, 0]) + good[8:], "bad header"),
        "N_off_by_one": (good[:8] + (N + 1).to_bytes(8, "little") + good[16:], "shape mismatch"),
        "flipped_hash_bit": (flip(good, D.HEADER + 3, 5), "another env"),
    }
    env, pol = _fresh(P)
    prev = P.BufferRollouts()
    P.collect_rollouts_steps_(prev, env, pol, Tprev, GAMMA)               # the buffer's previous contents: another length
    before = _columns_of(prev)
    gd = tmp_path / "good"
    os.makedirs(str(gd))
    open(D.rollout_bin(gd), "wb").write(good)
    for name, (blob, msg) in damaged.items():
        if name == "flipped_hash_bit":                            # a well-formed file, of another env
            D.decode(blob)
        else:
            with pytest.raises(ValueError):
                D.decode(blob)
        d = tmp_path / name
        os.makedirs(str(d))
        open(D.rollout_bin(d), "wb").write(blob)
        with pytest.raises(P.PPOError, match=msg):
            P.call("ppo_rollouts_load_disk", prev._h, str(d).encode())
        assert prev.dims() == (Tprev, N), name
        for a, b in zip(before, _columns_of(prev)):
            assert np.array_equal(a, b), name
        _record(test="loader", case=name, refused=True)
    # a following good load into the same buffer works, and training data is the memory-resident collection's
    P.call("ppo_rollouts_load_disk", prev._h, str(gd).encode())
    env, pol = _fresh(P)
    mem = P.BufferRollouts()
    P.collect_rollouts_steps_(mem, env, pol, T, GAMMA)
    for a, b in zip(_columns_of(mem), _columns_of(prev)):
        assert np.array_equal(a, b)
    with pytest.raises(P.PPOError, match="missing"):
        P.load_disk_rollouts(str(tmp_path / "nowhere"), env)


def test_disk_sync_reaches_the_library_for_an_empty_device_buffer(P, tmp_path, monkeypatch):
    """A device buffer of length 0 is falsy: disk_sync must not take the DiskRollouts itself for the buffer."""
    env, _ = _fresh(P)
    disk = P.DiskRollouts(str(tmp_path / "store"))
    dev = P.BufferRollouts()
    h = dev._ensure(env, 0)
    P.call("ppo_rollouts_attach_disk", h, disk.state_data_directory.encode(), 2)
    disk._device = dev
    assert len(dev) == 0 and not dev
    seen = []
    mod = sys.modules[P.disk_sync.__module__]
    real = mod.call
    monkeypatch.setattr(mod, "call", lambda name, *a: (seen.append(name), real(name, *a))[1])
    P.disk_sync(disk)
    assert seen == ["ppo_rollouts_disk_sync", "ppo_rollouts_detach_disk"]


# ================================================================ the child process: write failures
T_FAULT = 20
LIMITS = ("inside_record_3", "record_boundary", "inside_returns", "buffered_tail", "file_size")


def fault_cases():
    """L x {synchronous, deferred} x {ring 2, ring >= T} through the Python calls (wait point: disk_sync), then one case per
    other wait point through the C ABI.  A deferred ring of 2 exists only under a PPO_DISK_ASYNC_MAX_BYTES of two records."""
    out = []
    for L in LIMITS:
        for mode in ("sync", "deferred"):
            for ring in (2, 32):
                out.append(dict(name="%s-%s-ring%d" % (L, mode, ring), L=L, mode=mode, ring=ring, wait="disk_sync"))
    for wait, L, ring in (("detach", "inside_returns", 32), ("detach", "inside_record_3", 2), ("next_collect", "inside_returns", 32),
                          ("attach", "inside_returns", 32), ("destroy", "inside_returns", 32), ("destroy", "record_boundary", 2)):
        out.append(dict(name="%s-deferred-ring%d-%s" % (L, ring, wait), L=L, mode="deferred", ring=ring, wait=wait))
    return out


ENVVAR_CASES = [dict(name="envvar-file_size", L="file_size", mode="envvar", ring=16, wait="disk_sync"),
                dict(name="envvar-inside_returns", L="inside_returns", mode="envvar", ring=16, wait="disk_sync"),
                dict(name="envvar-inside_record_3", L="inside_record_3", mode="envvar", ring=16, wait="disk_sync")]
# the cases in which the parent commit lost the error without a report
SILENT_ON_PARENT = ("buffered_tail-sync-ring2", "buffered_tail-sync-ring32", "inside_returns-deferred-ring32-detach",
                    "inside_returns-deferred-ring32-next_collect", "envvar-inside_returns")


class _Child:
    """Runs in the child process only."""

    def __init__(self, log, work):
        self.log, self.work, self.k = log, work, 0
        root = os.environ.get("DISK_STORE_PACKAGE_ROOT", ROOT)
        for p in (ROOT, root):
            if p in sys.path:
                sys.path.remove(p)
            sys.path.insert(0, p)
        D.ignore_sigxfsz()
        import ppo_amd
        from oracle import oracle
        oracle.build()
        self.P, self.orc = ppo_amd, oracle
        self.off = D.fault_offsets(2, N, 32, 72, 32, T_FAULT)
        self.rec = D.record_bytes(2, N, 32, 72, 32)

    def say(self, **kw):
        with open(self.log, "a") as f:
            f.write(json.dumps(kw) + "\n")

    def dir(self, tag):
        self.k += 1
        return os.path.join(self.work, "%s_%d" % (tag, self.k))

    def budget(self, c):
        return _environ(PPO_DISK_ASYNC_MAX_BYTES=2 * self.rec + self.rec // 2 if (c["mode"] == "deferred" and c["ring"] == 2) else None)

    def collect_py(self, c, d):
        P = self.P
        env, pol = _fresh(P)
        disk = P.DiskRollouts(d)
        stages = []
        with self.budget(c):
            try:
                P.collect_rollouts_steps_(disk, env, pol, T_FAULT, GAMMA, pinned_slots=c["ring"])
            except P.PPOError as e:
                stages.append(("collect", str(e)))
            try:
                P.disk_sync(disk)
            except P.PPOError as e:
                stages.append(("disk_sync", str(e)))
        return stages

    def warm_up(self):
        """every ring and mode once, to a scratch directory: pinned records are in the pool, whatever files the runtime writes
        are written, and the expected bytes are known before any limit is lowered"""
        P = self.P
        self.want = expected_blobs(P, self.orc, 8, [T_FAULT, T_FAULT])
        for c in ([dict(mode="envvar", ring=16)] if self.envvar else
                  [dict(mode=m, ring=r) for m in ("sync", "deferred") for r in (2, 32)]):
            self.set_mode(c)
            d = self.dir("warm")
            assert self.collect_py(c, d) == []
            assert D.read(D.rollout_bin(d)) == self.want[(0, 2)], "warm-up file differs from the restatement"

    def set_mode(self, c):
        if c["mode"] != "envvar":                                 # the env-var child never calls set_disk_async
            self.P.set_disk_async(c["mode"] == "deferred")

    def run(self, c):
        P = self.P
        L, fails = self.off[c["L"]][0], self.off[c["L"]][1]
        self.set_mode(c)
        d = self.dir(c["name"])
        t0 = time.time()
        problems = []
        if c["wait"] == "disk_sync":
            with D.file_size_limit(L):
                stages = self.collect_py(c, d)
        else:
            stages = self.run_abi(c, d, L, problems)
        took = time.time() - t0
        if fails:
            if len(stages) != 1:
                problems.append("reported %d times, expected once: %r" % (len(stages), stages))
            for where, msg in stages:
                if not WRITE_FAILED.search(msg):
                    problems.append("%s: the message does not say that a write failed: %r" % (where, msg))
                if c["mode"] == "sync" and where != "collect":
                    problems.append("synchronous mode: reported by %s, not by the collecting call" % where)
            try:                                                  # the directory never yields a dataset
                if c["wait"] != "next_collect":                   # (there it holds the following, good collection by now)
                    env, _ = _fresh(P)
                    P.load_disk_rollouts(d, env)
                    problems.append("load_disk_rollouts took the directory of the failed collection")
            except P.PPOError:
                pass
            # the engine stays usable: the same collection to a fresh directory, the limit restored
            if c["wait"] != "next_collect":
                d2 = self.dir(c["name"] + "_again")
                again = self.collect_py(c, d2)
                if again or D.read(D.rollout_bin(d2)) != self.want[(0, 2)]:
                    problems.append("the same collection after the failure: %r" % (again or "file differs"))
        else:
            if stages:
                problems.append("control case reported %r" % stages)
            elif D.read(D.rollout_bin(d)) != self.want[(0, 2)]:
                problems.append("control case: file differs from the restatement")
        if took > 10:
            problems.append("took %.1f s" % took)
        return dict(stages=stages, problems=problems, seconds=round(took, 3))

    def run_abi(self, c, d, L, problems):
        """attach once, collect under the limit, then the wait point under test"""
        P = self.P
        env, pol = _fresh(P)
        dev = P.BufferRollouts()
        h = dev._ensure(env, 0)
        stages = []

        def step(where, name, *args):
            try:
                P.call(name, *args)
                return True
            except P.PPOError as e:
                stages.append((where, str(e)))
                return False
        with self.budget(c):
            P.call("ppo_rollouts_attach_disk", h, d.encode(), c["ring"])
            try:                                                  # an unrelated message in ppo_last_error: what destroy leaves is its own
                P.call("ppo_compute_returns", None, None, -1, 1.0, 0, None)
            except P.PPOError:
                pass
            with D.file_size_limit(L):
                first = step("collect", "ppo_collect_rollouts", h, env._h, pol._h, T_FAULT, GAMMA, 0, 0)
                if c["wait"] == "detach":
                    step("detach", "ppo_rollouts_detach_disk", h)
                elif c["wait"] == "attach":                       # a second attach settles the first sink: reports, attaches nothing
                    if not step("attach", "ppo_rollouts_attach_disk", h, self.dir("second").encode(), c["ring"]):
                        step("attach_again", "ppo_rollouts_attach_disk", h, self.dir("second").encode(), c["ring"])
                elif c["wait"] == "destroy":
                    h_, dev._h = dev._h, None
                    P._lib.lib().ppo_rollouts_destroy(h_)
                    msg = P._lib.last_error()
                    if first:
                        stages.append(("destroy", msg))           # no status: ppo_last_error is what is left
                elif c["wait"] == "next_collect":
                    if first and step("next_collect", "ppo_collect_rollouts", h, env._h, pol._h, T_FAULT, GAMMA, 0, 0):
                        problems.append("the next collection started although the previous file had failed")
            if c["wait"] == "next_collect" and first:
                # the refused call started nothing: the collection after it is the SECOND collection of this env, byte for byte
                if os.path.exists(D.rollout_bin(d)):
                    problems.append("the refused collection left a rollout.bin")
                ok = step("third_collect", "ppo_collect_rollouts", h, env._h, pol._h, T_FAULT, GAMMA, 0, 0) and \
                    step("sync", "ppo_rollouts_disk_sync", h)
                if ok and D.read(D.rollout_bin(d)) != self.want[(1, 2)]:
                    problems.append("the collection after the refused one is not this env's second collection")
        return stages

    def main(self, envvar):
        self.envvar = envvar
        self.say(case="warm_up", phase="begin")
        self.warm_up()
        self.say(case="warm_up", phase="end", problems=[])
        for c in (ENVVAR_CASES if envvar else fault_cases()):
            self.say(case=c["name"], phase="begin")
            try:
                r = self.run(c)
            except Exception as e:                                # an unexpected error is this case's finding, the rest still runs
                r = dict(stages=[], problems=["%s: %s" % (type(e).__name__, e)], seconds=None)
            self.say(case=c["name"], phase="end", **r)
        self.say(case="all", phase="end", problems=[])


def _run_child(tmp, envvar):
    log = os.path.join(str(tmp), "envvar.jsonl" if envvar else "faults.jsonl")
    work = os.path.join(str(tmp), "work_envvar" if envvar else "work")
    os.makedirs(work)
    cases = ENVVAR_CASES if envvar else fault_cases()
    env = dict(os.environ)
    env.pop("PPO_DISK_ASYNC", None)
    env.pop("PPO_DISK_ASYNC_MAX_BYTES", None)
    env.pop("PPO_DISK_BATCH", None)
    if envvar:
        env["PPO_DISK_ASYNC"] = "1"
    limit = 90 + 5 * len(cases)                                   # import, oracle build and warm-up, then a few seconds per case
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "child", "envvar" if envvar else "main", log, work],
                         env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=ROOT)
    try:
        out, _ = p.communicate(timeout=limit)
        timed_out = False
    except subprocess.TimeoutExpired:
        p.kill()
        out, _ = p.communicate()
        timed_out = True
    lines = [json.loads(x) for x in open(log)] if os.path.exists(log) else []
    last = lines[-1]["case"] if lines else "(nothing logged)"
    tail = out.decode("utf-8", "replace")[-2000:]
    assert not timed_out, "the child hit its time limit of %d s; last case logged: %s\n%s" % (limit, last, tail)
    assert p.returncode == 0, "the child ended with status %s; last case logged: %s\n%s" % (p.returncode, last, tail)
    res = {x["case"]: x for x in lines if x["phase"] == "end"}
    for name, r in res.items():
        _record(test="write_failure", case=name, **{k: v for k, v in r.items() if k not in ("case", "phase")})
    return res


@pytest.fixture(scope="module")
def fault_results(ppo, tmp_path_factory):
    if ppo.device_count() == 0:
        pytest.skip("no GPU")
    return _run_child(tmp_path_factory.mktemp("faults"), False)


@pytest.fixture(scope="module")
def envvar_results(ppo, fault_results, tmp_path_factory):       # after the first child: one child holds the GPU at a time
    return _run_child(tmp_path_factory.mktemp("envvar"), True)


@pytest.mark.parametrize("name", [c["name"] for c in fault_cases()])
def test_write_failure_is_reported_and_survivable(fault_results, name):
    r = fault_results[name]
    assert r["problems"] == [], r


@pytest.mark.parametrize("name", [c["name"] for c in ENVVAR_CASES])
def test_deferred_mode_from_the_environment_alone(envvar_results, name):
    r = envvar_results[name]
    assert r["problems"] == [], r
    if name != "envvar-file_size":
        assert r["stages"] and r["stages"][0][0] in ("collect", "disk_sync")


if __name__ == "__main__" and len(sys.argv) == 5 and sys.argv[1] == "child":
    _Child(sys.argv[3], sys.argv[4]).main(sys.argv[2] == "envvar")
