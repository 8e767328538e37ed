"""An independent restatement of <dir>/rollout.bin, the out-of-core rollout store's file (numpy only).

Written from the format comment at the top of csrc/ppo_disk.hip, not from its code, and it takes nothing from a file the
engine wrote or from the engine's loader:

  header (40 bytes, little endian): "PPOR", u32 version, i64 N, i32 H, i32 F, i32 A, i32 V, i64 T
  version 2 only, a 16-byte tag:    u64 FNV-1a of the [H][36] template-vertex table (offset basis: STORE_BASIS below), i32 0, i32 0
  T records:                        [states][active u32 N][actions i32 N, 0-based][p_sel f32 N][raw rewards f32 N][done u8 N]
  the returns column:               [T][N] f32
  version 1 states: the N*H*F int8 observations;  version 2 states: N*2V int8 snapshots, score[V] then degree[V] per env

`columns` is a dict of plain arrays: N, H, F, A, V, T, states ([T,N,H,F] for version 1, [T,N,2V] for version 2), active, actions
(0-based), p_sel, rewards (raw), done, returns (all [T,N]) and, for version 2, template ([H,36] int8).

Also here: where the columns come from in the GPU tests (the memory-resident collection of the same seed, the CPU env replayed
under its actions for the snapshots), the byte offsets the write-failure cases land on, and the file-size limit they are
injected with."""
import contextlib
import errno
import os
import resource
import signal
import struct

import numpy as np

HEADER = 40
TAG = 16
TPL = 36
_HDR = "<4sIqiiiiq"
SECTIONS = ("active", "actions", "p_sel", "rewards", "done")
_DT = {"active": "<u4", "actions": "<i4", "p_sel": "<f4", "rewards": "<f4", "done": "u1"}


class ShortFile(ValueError):
    """decode(): the bytes end inside `section` (of record `record`, where that applies)."""

    def __init__(self, section, record=None, have=0, need=0):
        self.section, self.record = section, record
        where = section if record is None else "%s of record %d" % (section, record)
        ValueError.__init__(self, "rollout.bin ends early: %s needs %d bytes, %d are left" % (where, need, have))


FNV_BASIS = 14695981039346656037      # the published 64-bit offset basis
# What the store hashes with: the published basis without its last digit.  Found by this restatement (the first version used
# FNV_BASIS and no tag matched); every file written so far carries it and the tag is checked on load, so it is part of the
# format and stays.  Any fixed basis serves the tag's purpose, telling two template tables apart.
STORE_BASIS = 1469598103934665603


def fnv1a(data, basis=STORE_BASIS):
    h = basis
    for b in bytes(data):
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def state_bytes(version, H, F, V):
    """per env and step"""
    return H * F if version == 1 else 2 * V


def header_bytes(version):
    return HEADER + (TAG if version == 2 else 0)


def record_bytes(version, N, H, F, V):
    return N * state_bytes(version, H, F, V) + 17 * N


def file_bytes(version, N, H, F, V, T):
    """40 (+16) + T*(N*state_bytes + 17N) + 4TN: the formula tests/test_gpu_parity.py and tests/test_gpu_disk_async.py assert"""
    return header_bytes(version) + T * record_bytes(version, N, H, F, V) + 4 * T * N


def encode(columns, version):
    c = columns
    N, H, F, A, V, T = (int(c[k]) for k in ("N", "H", "F", "A", "V", "T"))
    assert version in (1, 2)
    out = [struct.pack(_HDR, b"PPOR", version, N, H, F, A, V, T)]
    if version == 2:
        tpl = np.asarray(c["template"])
        assert tpl.dtype == np.int8 and tpl.shape == (H, TPL)
        out.append(struct.pack("<Qii", fnv1a(tpl.tobytes()), 0, 0))
    st = np.asarray(c["states"])
    assert st.dtype == np.int8 and st.shape == ((T, N, H, F) if version == 1 else (T, N, 2 * V)), st.shape
    cols = {}
    for k in SECTIONS + ("returns",):
        a = np.asarray(c[k])
        assert a.shape == (T, N), (k, a.shape)
        want = np.dtype(_DT.get(k, "<f4"))
        assert a.dtype.kind == want.kind and a.dtype.itemsize == want.itemsize, (k, a.dtype)    # no silent conversion
        cols[k] = a.astype(want, copy=False)
    for t in range(T):
        out.append(st[t].tobytes())
        out.extend(cols[k][t].tobytes() for k in SECTIONS)
    out.append(cols["returns"].tobytes())
    return b"".join(out)


def decode(data):
    data = bytes(data)
    pos = 0

    def take(n, section, record=None):
        nonlocal pos
        if len(data) - pos < n:
            raise ShortFile(section, record, len(data) - pos, n)
        pos += n
        return data[pos - n:pos]

    magic, version, N, H, F, A, V, T = struct.unpack(_HDR, take(HEADER, "header"))
    if magic != b"PPOR":
        raise ValueError("rollout.bin: bad magic %r" % magic)
    if version not in (1, 2):
        raise ValueError("rollout.bin: unknown version %d" % version)
    c = dict(N=N, H=H, F=F, A=A, V=V, T=T)
    if version == 2:
        c["template_hash"], kind, zero = struct.unpack("<Qii", take(TAG, "tag"))
        if (kind, zero) != (0, 0):
            raise ValueError("rollout.bin: tag words (%d, %d), expected zeros" % (kind, zero))
    sb = N * state_bytes(version, H, F, V)
    st = np.empty((T, sb), np.int8)
    cols = {k: np.empty((T, N), _DT[k]) for k in SECTIONS}
    for t in range(T):
        st[t] = np.frombuffer(take(sb, "states", t), np.int8)
        for k in SECTIONS:
            cols[k][t] = np.frombuffer(take(N * cols[k].itemsize, k, t), _DT[k])
    c["states"] = st.reshape((T, N, H, F) if version == 1 else (T, N, 2 * V))
    c.update(cols)
    c["returns"] = np.frombuffer(take(4 * T * N, "returns"), "<f4").reshape(T, N).copy()
    if pos != len(data):
        raise ValueError("rollout.bin: %d bytes behind the returns column" % (len(data) - pos))
    return version, c


def same(a, b):
    """two column dicts hold the same bits (floats compared as bits: -0.0 and NaN payloads count)"""
    if set(a) != set(b):
        return False
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            return False
    return True


def with_hash(columns):
    """what decode(encode(columns, 2)) returns for `columns`: the table is stored as its hash"""
    c = {k: v for k, v in columns.items() if k != "template"}
    c["template_hash"] = fnv1a(np.asarray(columns["template"]).tobytes())
    return c


# ---------------------------------------------------------------- where the expected columns come from
def template_table(orc, Q):
    """[H][36] template vertex ids of the CPU env, -1 = missing"""
    H = 4 * Q
    return np.array([[orc.lib().orc_env_template(Q, h, t) for t in range(TPL)] for h in range(H)], np.int8)


def replay_snapshots(orc, env_kw, actions0, check=None):
    """score[V] then degree[V] of every env in front of each step: the CPU env of a fresh device env (reset of episode
    counter 0), stepped under the recorded 0-based actions [T,N] with the collectors' auto-reset.  check = dict(active,
    rewards, done): the replay must reproduce these recorded columns too, or the actions are not this env's."""
    e = orc.Env(Q=env_kw["Q"], max_actions=env_kw["max_actions"], N=env_kw["num_envs"], seed=env_kw["seed"],
                global_offset=env_kw.get("global_offset", 0))
    e.episode[:] = 0
    e.tick[:] = 0
    e.reset()
    T, N = actions0.shape
    snap = np.empty((T, N, 2 * e.V), np.int8)
    for t in range(T):
        snap[t, :, :e.V] = e.score
        snap[t, :, e.V:] = e.degree
        if check is not None:
            assert np.array_equal(np.asarray(e.active), check["active"][t]), ("active", t)
        e.step_all(actions0[t])
        done = np.asarray(e.done).astype(bool)
        if check is not None:
            assert np.array_equal(np.asarray(e.reward), check["rewards"][t]), ("rewards", t)
            assert np.array_equal(done, np.asarray(check["done"][t]).astype(bool)), ("done", t)
        for n in np.flatnonzero(done):
            e.reset_one(int(n))
    assert not (np.asarray(e.err) & ~32).any()
    return snap


def columns_from_memory(orc, env_kw, ro, version):
    """The expected columns of a streamed collection: every column but the snapshots from the getters of the memory-resident
    BufferRollouts `ro` of the same seed, the snapshots and the table from the CPU env."""
    st, act = ro.state_data
    T, N, H, F = st.shape
    Q = env_kw["Q"]
    c = dict(N=N, H=H, F=F, A=16 * Q, V=4 * Q, T=T,
             active=act.astype(np.uint32), actions=(ro.selected_actions - 1).astype(np.int32),
             p_sel=ro.selected_action_probabilities, rewards=ro.raw_rewards, done=ro.terminal.astype(np.uint8),
             returns=ro.rewards)
    if version == 1:
        c["states"] = st
    else:
        c["states"] = replay_snapshots(orc, env_kw, c["actions"], check=c)
        c["template"] = template_table(orc, Q)
    return c


# ---------------------------------------------------------------- write failures: offsets and the injection
def fault_offsets(version, N, H, F, V, T):
    """name -> (L, a write failure is expected).  L is the soft RLIMIT_FSIZE around the call under test."""
    hdr, rec, size = header_bytes(version), record_bytes(version, N, H, F, V), file_bytes(version, N, H, F, V, T)
    ret0 = hdr + T * rec
    assert T > 4 and 4 * T * N >= 4096 + 1024
    return {"inside_record_3": (hdr + 3 * rec + rec // 2, True),
            "record_boundary": (hdr + 5 * rec, True),
            "inside_returns": (size - 4096 - 512, True),
            "buffered_tail": (size - 100, True),
            "file_size": (size, False),
            "_returns_start": (ret0, None)}


def ignore_sigxfsz():
    """a write past the soft limit then fails with EFBIG instead of ending the process"""
    signal.signal(signal.SIGXFSZ, signal.SIG_IGN)


@contextlib.contextmanager
def file_size_limit(nbytes):
    """Lower the SOFT RLIMIT_FSIZE of this process to `nbytes` around the body and restore it.  While it is in force a write
    that reaches offset `nbytes` of a file is cut short there and the next one fails with EFBIG (SIGXFSZ must be ignored:
    ignore_sigxfsz).  A host I/O error: nothing on the device is involved."""
    soft, hard = resource.getrlimit(resource.RLIMIT_FSIZE)
    resource.setrlimit(resource.RLIMIT_FSIZE, (int(nbytes), hard))
    try:
        yield
    finally:
        resource.setrlimit(resource.RLIMIT_FSIZE, (soft, hard))


def is_efbig(exc):
    return isinstance(exc, OSError) and exc.errno == errno.EFBIG


def read(path):
    with open(path, "rb") as f:
        return f.read()


def rollout_bin(d):
    return os.path.join(str(d), "rollout.bin")
