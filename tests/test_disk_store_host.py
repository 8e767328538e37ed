"""CPU checks of tests/disk_store_ref.py, the independent restatement of rollout.bin that tests/test_gpu_disk_store.py
compares the engine's file with: encode and decode are inverses, the sizes are the formula the existing streaming tests
assert, a short file names the section it ends in, the snapshot replay agrees with the CPU env's own collection, and the
file-size limit the write-failure cases are injected with behaves on a plain file as those cases assume."""
import os

import numpy as np
import pytest

import disk_store_ref as D


def _columns(rng, version, Q, N, T):
    H, F, A, V = 4 * Q, 72, 16 * Q, 4 * Q
    c = dict(N=N, H=H, F=F, A=A, V=V, T=T,
             active=rng.integers(0, 2 ** 32, (T, N), dtype=np.uint64).astype(np.uint32),
             actions=rng.integers(0, A, (T, N)).astype(np.int32),
             p_sel=rng.random((T, N), dtype=np.float32),
             rewards=rng.normal(size=(T, N)).astype(np.float32),
             done=rng.integers(0, 2, (T, N)).astype(np.uint8),
             returns=rng.normal(size=(T, N)).astype(np.float32))
    c["rewards"][0, 0] = -0.0                                            # bits, not values
    if version == 1:
        c["states"] = rng.integers(-128, 128, (T, N, H, F)).astype(np.int8)
    else:
        c["states"] = rng.integers(-128, 128, (T, N, 2 * V)).astype(np.int8)
        c["template"] = rng.integers(-1, V, (H, D.TPL)).astype(np.int8)
    return c


SHAPES = [(8, 5, 3), (32, 3, 2), (8, 7, 1)]                               # (Q, N, T): Q = 8, Q = 32, T = 1


@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("Q,N,T", SHAPES)
def test_decode_inverts_encode_and_sizes_follow_the_formula(version, Q, N, T):
    c = _columns(np.random.default_rng(Q + N + T + version), version, Q, N, T)
    blob = D.encode(c, version)
    sb = 4 * Q * 72 if version == 1 else 8 * Q
    assert len(blob) == 40 + (16 if version == 2 else 0) + T * (N * sb + 17 * N) + 4 * T * N
    assert len(blob) == D.file_bytes(version, N, c["H"], c["F"], c["V"], T)
    v, back = D.decode(blob)
    assert v == version
    assert D.same(back, D.with_hash(c) if version == 2 else c)
    assert D.encode(dict(back, template=c.get("template")), version) == blob
    # the layout, spelled out once more for record 0: actions sit behind states and active, done is the record's last N bytes
    hdr, rec = D.header_bytes(version), D.record_bytes(version, N, c["H"], c["F"], c["V"])
    assert blob[:4] == b"PPOR" and blob[4:8] == bytes([version, 0, 0, 0])
    assert blob[hdr + N * sb + 4 * N:hdr + N * sb + 8 * N] == c["actions"][0].astype("<i4").tobytes()
    assert blob[hdr + rec - N:hdr + rec] == c["done"][0].tobytes()
    assert blob[-4 * T * N:] == c["returns"].astype("<f4").tobytes()


def test_the_columns_are_told_apart():
    """every column moves the bytes, and no two columns move the same ones"""
    c = _columns(np.random.default_rng(1), 2, 8, 4, 3)
    base = D.encode(c, 2)
    seen = set()
    for k in ("states", "active", "actions", "p_sel", "rewards", "done", "returns", "template"):
        m = dict(c)
        m[k] = c[k].copy()
        bits = m[k].view(np.uint32 if m[k].dtype.kind == "f" else m[k].dtype).reshape(-1)
        bits[-1] ^= 1                                                   # the last element's lowest bit
        blob = D.encode(m, 2)
        diff = tuple(i for i in range(len(base)) if base[i] != blob[i])
        assert diff and diff not in seen, k
        seen.add(diff)
    # the hash is FNV-1a (the published vectors), started from the store's own basis
    assert D.fnv1a(b"", D.FNV_BASIS) == 0xCBF29CE484222325 and D.fnv1a(b"a", D.FNV_BASIS) == 0xAF63DC4C8601EC8C
    assert D.fnv1a(b"") == D.STORE_BASIS == D.FNV_BASIS // 10


@pytest.mark.parametrize("version", [1, 2])
def test_a_short_file_names_the_section_it_ends_in(version):
    Q, N, T = 8, 3, 4
    c = _columns(np.random.default_rng(9), version, Q, N, T)
    blob = D.encode(c, version)
    hdr, rec = D.header_bytes(version), D.record_bytes(version, N, c["H"], c["F"], c["V"])
    sb = N * D.state_bytes(version, c["H"], c["F"], c["V"])
    cuts = [(10, "header", None), (hdr + 2 * rec + sb - 1, "states", 2), (hdr + 2 * rec + sb + 4 * N + 1, "actions", 2),
            (hdr + 3 * rec + rec - 1, "done", 3), (hdr + T * rec, "returns", None), (len(blob) - 1, "returns", None)]
    if version == 2:
        cuts.append((47, "tag", None))
    for cut, section, record in cuts:
        with pytest.raises(D.ShortFile) as ei:
            D.decode(blob[:cut])
        assert (ei.value.section, ei.value.record) == (section, record), cut
    with pytest.raises(ValueError, match="magic"):
        D.decode(b"QPOR" + blob[4:])
    with pytest.raises(ValueError, match="version 7"):
        D.decode(blob[:4] + bytes([7, 0, 0, 0]) + blob[8:])
    with pytest.raises(ValueError, match="behind the returns"):
        D.decode(blob + b"\0")


@pytest.mark.parametrize("Q", [8, 32])
def test_snapshot_replay_agrees_with_the_cpu_envs_own_collection(orc, Q):
    """The snapshots are the one column no getter returns.  Replayed under the actions the CPU collection took, the env must
    reproduce that collection's active, rewards and done, and the observations expanded from the snapshots through the
    template table must be the observations it recorded (auto-resets included: max_actions 5 < T)."""
    kw = dict(num_envs=6, Q=Q, max_actions=5, seed=11, global_offset=3)
    T = 12
    e = orc.Env(Q=Q, max_actions=5, N=6, seed=11, global_offset=3)
    e.episode[:] = 0
    e.tick[:] = 0
    e.reset()
    r = orc.collect_rollouts_tn(e, orc.glorot_params(72, 128, 2, seed=2), 128, T)
    assert r["done"].sum() >= 6
    snap = D.replay_snapshots(orc, kw, r["actions"], check=r)
    tpl = D.template_table(orc, Q).astype(np.int64)
    V = 4 * Q
    own = (r["active"][:, :, None] >> (np.arange(4 * Q) // 4)[None, None, :]) & 1                 # [T,N,H]: the half-edge's quad
    there = (tpl >= 0)[None, None] & (((r["active"][:, :, None, None] >> (np.maximum(tpl, 0) // 4)[None, None]) & 1) == 1)
    ok = there & (own[..., None] == 1)
    idx = np.broadcast_to(np.maximum(tpl, 0)[None, None], ok.shape).reshape(T, 6, -1)
    sc = np.take_along_axis(snap[:, :, :V], idx, axis=2).reshape(ok.shape)
    dg = np.take_along_axis(snap[:, :, V:], idx, axis=2).reshape(ok.shape)
    obs = np.concatenate([np.where(ok, sc, 0), np.where(ok, dg, 0)], axis=3).astype(np.int8)
    assert np.array_equal(obs, r["states"])


def test_fault_offsets_land_where_the_cases_say():
    N, T, Q = 96, 20, 8
    off = D.fault_offsets(2, N, 4 * Q, 72, 4 * Q, T)
    hdr, rec, size = 56, 7776, 163256                                     # the figures of the issue, for this one shape
    assert (D.header_bytes(2), D.record_bytes(2, N, 32, 72, 32), D.file_bytes(2, N, 32, 72, 32, T)) == (hdr, rec, size)
    assert off["_returns_start"][0] == 155576
    L = off["inside_record_3"][0]
    assert hdr + 3 * rec < L < hdr + 4 * rec
    assert (off["record_boundary"][0] - hdr) % rec == 0 and hdr < off["record_boundary"][0] < 155576
    assert 155576 < off["inside_returns"][0] <= size - 4096
    assert off["buffered_tail"][0] == size - 100 and off["file_size"] == (size, False)
    assert all(off[k][1] for k in ("inside_record_3", "record_boundary", "inside_returns", "buffered_tail"))


def test_file_size_limit_cuts_a_write_short_then_fails_then_lifts(tmp_path):
    """What the write-failure cases rely on, on a plain file: under the soft limit L a write that reaches L is cut short
    there, the next one fails with EFBIG, and once the limit is restored writes go through again."""
    D.ignore_sigxfsz()
    L = 5000
    fd = os.open(str(tmp_path / "plain.bin"), os.O_WRONLY | os.O_CREAT, 0o644)
    try:
        with D.file_size_limit(L):
            assert os.write(fd, b"a" * 4096) == 4096
            assert os.write(fd, b"b" * 4096) == L - 4096                 # cut short at L
            with pytest.raises(OSError) as ei:
                os.write(fd, b"c" * 16)
            assert D.is_efbig(ei.value)
        assert os.write(fd, b"d" * 4096) == 4096                         # the limit is back where it was
    finally:
        os.close(fd)
    blob = D.read(str(tmp_path / "plain.bin"))
    assert blob == b"a" * 4096 + b"b" * (L - 4096) + b"d" * 4096
    # a buffered stream shows the same failure only when it is flushed: the tail case of the synchronous path
    with D.file_size_limit(100):
        f = open(str(tmp_path / "stream.bin"), "wb")
        f.write(b"e" * 200)                                               # sits in the buffer
        with pytest.raises(OSError) as ei:
            f.flush()
        assert D.is_efbig(ei.value)
    assert os.path.getsize(str(tmp_path / "stream.bin")) == 100
    try:
        f.close()
    except OSError:
        pass
