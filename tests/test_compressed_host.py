"""Host side of the device decode of Kaldi compressed matrices: the C ABI declaration and its argument checks (refused before any
device call), the header table of ScpBatchLoader with its second kind of direct entry, load_compressed, and the grouping of
ScpGroupReader - no GPU."""

import ctypes as C
import importlib.util
import io
import os
import re

import numpy as np
import pytest

import compressed_cases as cc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_script():
    spec = importlib.util.spec_from_file_location("extract_embeddings_compressed", os.path.join(REPO, "asv-subtools_amd", "pytorch", "pipeline", "onestep",
                                                                                                "extract_embeddings.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ----------------------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_and_listed():
    from libs.amd import capi
    hdr = open(os.path.join(REPO, "include", "asv_amd.h")).read()
    assert re.search(r"\bint\s+asv_decode_compressed\s*\(", hdr)
    assert "asv_decode_compressed" in capi.SYMBOLS
    assert len(capi.lib().asv_decode_compressed.argtypes) == 8


def test_bad_arguments_are_refused_before_any_device_call():
    from libs.amd import capi
    lib = capi.lib()
    p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_longlong))
    pu8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_ubyte))
    byte_off, frame_off, formats = np.array([0, 64], dtype=np.int64), np.array([0, 2, 4], dtype=np.int64), np.array([1, 1], dtype=np.uint8)
    assert lib.asv_decode_compressed(None, None, None, None, 1, 4, None, None) < 0
    assert b"asv_decode_compressed" in lib.asv_last_error()
    # (host memory stands in for the two device pointers: every refusal below comes before the library looks at them)
    fake = np.zeros(256, dtype=np.uint8)
    call = lambda b, f, fmt, n=2, dim=4: lib.asv_decode_compressed(fake.ctypes.data, p64(b), p64(f), pu8(fmt), n, dim, fake.ctypes.data, None)
    assert lib.asv_decode_compressed(None, p64(byte_off), p64(frame_off), pu8(formats), 2, 4, fake.ctypes.data, None) < 0
    assert lib.asv_decode_compressed(fake.ctypes.data, p64(byte_off), p64(frame_off), pu8(formats), 2, 4, None, None) < 0
    for bad in (8, 17, 100):
        assert call(np.array([0, bad], dtype=np.int64), frame_off, formats) < 0
        msg = lib.asv_last_error()
        assert b"asv_decode_compressed" in msg and b"16" in msg, msg
    assert call(byte_off, frame_off, formats, n=0) < 0 and b"asv_decode_compressed" in lib.asv_last_error()
    assert call(byte_off, frame_off, formats, dim=0) < 0 and b"asv_decode_compressed" in lib.asv_last_error()
    assert call(byte_off, np.array([0, 3, 2], dtype=np.int64), formats) < 0 and b"decrease" in lib.asv_last_error()
    assert call(byte_off, np.array([1, 3, 4], dtype=np.int64), formats) < 0
    assert call(np.array([64, 0], dtype=np.int64), frame_off, formats) < 0                     # byte offsets have to increase ...
    assert call(np.array([0, 48], dtype=np.int64), frame_off, formats) < 0                     # ... past the body in front: 16 + 8 * 4 + 2 * 4 = 56 bytes
    for fmt in (0, 4, 255):
        assert call(byte_off, frame_off, np.array([1, fmt], dtype=np.uint8)) < 0 and b"format" in lib.asv_last_error()


def test_wrapper_exists_next_to_ingest():
    from libs.amd import frontend
    assert callable(frontend.decode_compressed) and callable(frontend.ingest)
    assert frontend.COMPRESSED_FORMATS == {"CM ": 1, "CM2": 2, "CM3": 3}
    assert frontend.compressed_body_bytes(np.array([1, 2, 3]), np.array([5, 5, 5]), 7).tolist() == [16 + 56 + 35, 16 + 70, 16 + 35]


def test_case_builders_are_valid_entries():
    """What the helper builds from random bytes is what the host reader reads: shapes, value range, and every byte value from 256 rows on."""
    rng = np.random.RandomState(0)
    m = cc.host_decode(1, cc.cm_body(rng, 257, 5, -3.0, 9.0))
    assert m.shape == (257, 5) and m.dtype == np.float32 and m.min() >= -3.0 - 1e-4 and m.max() <= 6.0 + 1e-4
    body = cc.cm_body(rng, 257, 5)
    data = np.frombuffer(body[16 + 40:], dtype=np.uint8).reshape(5, 257)
    assert all(len(set(col.tolist())) == 256 for col in data)
    assert cc.host_decode(2, cc.cm2_body(rng, 7, 3)).shape == (7, 3) and cc.host_decode(3, cc.cm3_body(rng, 7, 3)).shape == (7, 3)


# ----------------------------------------------------------------------------------------------------------------------------------
DIM = 23
KINDS = ["CM ", "FM ", "CM2", "range", "CM3", "DM ", "CM ", "text", "CM ", "FM ", "CM3", "CM2"]
ROWS = [57, 40, 130, 64, 37, 9, 257, 5, 1, 88, 65, 3]
FORMAT = {"CM ": 1, "CM2": 2, "CM3": 3}


def write_table(tmp_path, kinds=KINDS, rows=ROWS, dim=DIM, seed=3):
    """One ark with an entry per kind ('range': a compressed entry addressed with a range specifier; 'text': a text matrix in a file of
    its own) -> (scp path, scp lines, the bodies by entry or None)."""
    rng = np.random.RandomState(seed)
    entries, bodies, text = [], [], {}
    for i, (kind, T) in enumerate(zip(kinds, rows)):
        key = "utt%02d" % i
        if kind in FORMAT or kind == "range":
            fmt = FORMAT.get(kind, 1)
            body = cc.BODY[fmt](rng, T, dim)
            entries.append((key, cc.compressed_payload(fmt, body)))
            bodies.append((fmt, body) if kind != "range" else None)
        elif kind == "text":
            m = rng.randn(T, dim).astype(np.float32)
            text[key] = " [\n" + "\n".join(" ".join("%.6g" % v for v in row) for row in m) + " ]\n"
            entries.append((key, b""))
            bodies.append(None)
        else:
            m = rng.randn(T, dim).astype(np.float32 if kind == "FM " else np.float64)
            entries.append((key, cc.float_payload(m)))
            bodies.append(None)
    ark = str(tmp_path / "feats.ark")
    lines = cc.write_ark(ark, entries)
    for i, kind in enumerate(kinds):
        key = "utt%02d" % i
        if kind == "range":
            lines[i] += "[2:%d]" % (rows[i] - 3)
        if kind == "text":
            path = tmp_path / (key + ".txt")
            path.write_text(text[key])
            lines[i] = "%s %s" % (key, path)
    scp = tmp_path / "feats.scp"
    scp.write_text("\n".join(lines) + "\n")
    return str(scp), lines, bodies


def want_rows(kinds=KINDS, rows=ROWS):
    return [T - 4 if kind == "range" else T for kind, T in zip(kinds, rows)]


@pytest.mark.parametrize("table", [True, False])
def test_entries_are_classified_and_lengths_come_from_the_headers(tmp_path, monkeypatch, table):
    """index_all() (one native pass + the second pass over the `CM` candidates) and the per-entry path agree on every kind of entry;
    lengths() and shape() of the direct entries - compressed ones included - read headers only."""
    ee = load_script()
    scp, lines, bodies = write_table(tmp_path)
    entries = ee.read_scp("scp:" + scp)
    loader = ee.ScpBatchLoader(entries, threads=2)
    if table:
        assert loader.index_all() is True
    else:
        loader._table = False                                               # the per-entry path (no native library / too many files)
    want_fmt = [FORMAT.get(kind, 0) for kind in KINDS]
    assert [loader.compressed_format(i) for i in range(len(KINDS))] == want_fmt
    assert [loader._direct(i) is not None for i in range(len(KINDS))] == [kind == "FM " for kind in KINDS]
    assert loader.has_compressed()
    for i, kind in enumerate(KINDS):
        h = loader._direct_compressed(i)
        if kind in FORMAT:
            path, body_off, r, c, fmt = h
            assert (r, c, fmt) == (ROWS[i], DIM, FORMAT[kind])
            with open(path, "rb") as f:
                f.seek(body_off)
                assert f.read(len(bodies[i][1])) == bodies[i][1]            # the body offset: behind the token, at the global header
        else:
            assert h is None
    real = ee.read_matrix
    direct = {lines[i].split(None, 1)[1] for i, kind in enumerate(KINDS) if kind in FORMAT or kind == "FM "}

    def guarded(rx):
        assert rx not in direct, "a direct entry was decoded to learn its shape: %r" % rx
        return real(rx)

    monkeypatch.setattr(ee, "read_matrix", guarded)
    assert loader.lengths().tolist() == want_rows()
    for i, kind in enumerate(KINDS):
        if kind in FORMAT or kind == "FM ":
            assert tuple(loader.shape(i)) == (ROWS[i], DIM)
    loader.close()


def test_lengths_of_a_compressed_table_without_a_single_decode(tmp_path, monkeypatch):
    ee = load_script()
    kinds = ["CM ", "CM2", "CM3", "CM "]
    scp, _, _ = write_table(tmp_path, kinds, [11, 7, 300, 64])

    def refuse(rx):
        raise AssertionError("read_matrix(%r)" % rx)

    monkeypatch.setattr(ee, "read_matrix", refuse)
    monkeypatch.setattr(ee, "matrix_rows", refuse)
    for table in (True, False):
        loader = ee.ScpBatchLoader(ee.read_scp("scp:" + scp))
        if not table:
            loader._table = False
        assert loader.lengths().tolist() == [11, 7, 300, 64]
        assert ee.ScpGroupReader(ee.read_scp("scp:" + scp)).peek_dim() == DIM
        loader.close()


@pytest.mark.parametrize("native", [True, False])
def test_load_compressed_reads_the_bodies_as_they_are(tmp_path, monkeypatch, native):
    from libs.support import kaldi_io, native_io
    ee = load_script()
    scp, lines, bodies = write_table(tmp_path)
    entries = ee.read_scp("scp:" + scp)
    loader = ee.ScpBatchLoader(entries, threads=3)
    loader.index_all()
    if not native:
        monkeypatch.setattr(native_io, "lib", lambda: None)                 # the same reads from Python
    idx = [i for i, kind in enumerate(KINDS) if kind in FORMAT][::-1]       # (any order: the table is random access)
    raw = np.full(1 << 16, 0xEE, dtype=np.uint8)
    buf = raw[(-raw.ctypes.data) % 16:][:60000]
    byte_off, frame_off, formats, used = loader.load_compressed(idx, buf)
    assert byte_off.dtype == np.int64 and frame_off.dtype == np.int64 and formats.dtype == np.uint8
    assert (byte_off % 16 == 0).all() and (np.diff(byte_off) > 0).all() and byte_off[0] == 0
    assert frame_off.tolist() == np.concatenate([[0], np.cumsum([ROWS[i] for i in idx])]).tolist()
    assert formats.tolist() == [FORMAT[KINDS[i]] for i in idx]
    assert used == int(byte_off[-1]) + (len(bodies[idx[-1]][1]) + 15) // 16 * 16 and (buf[used:] == 0xEE).all()
    for k, i in enumerate(idx):
        fmt, body = bodies[i]
        got = buf[int(byte_off[k]):int(byte_off[k]) + len(body)].tobytes()
        assert got == body                                                  # the file's slice
        m = kaldi_io.read_mat(io.BytesIO(cc.compressed_payload(fmt, got)))
        want = ee.read_matrix(lines[i].split(None, 1)[1])
        assert np.array_equal(np.asarray(m, dtype=np.float32).view(np.uint32), want.view(np.uint32))
    with pytest.raises(ValueError):
        loader.load_compressed(idx, buf[:used - 16])                        # a buffer that is too small is refused, not overrun
    with pytest.raises(ValueError):
        loader.load_compressed([1], buf)                                    # an `FM ` entry
    loader.close()


def test_load_compressed_refuses_a_header_that_disagrees_with_the_table(tmp_path):
    from libs.support import kaldi_io
    ee = load_script()
    kinds, rows = ["CM ", "CM ", "CM3"], [20, 33, 12]
    scp, lines, bodies = write_table(tmp_path, kinds, rows)
    loader = ee.ScpBatchLoader(ee.read_scp("scp:" + scp))
    assert loader.index_all()
    buf = np.zeros(1 << 14, dtype=np.uint8)
    buf = buf[(-buf.ctypes.data) % 16:]
    loader.load_compressed([0, 1, 2], buf)
    # the archive changes under the table: entry 1 now says 32 rows
    path, body_off = loader._direct_compressed(1)[:2]
    with open(path, "r+b") as f:
        f.seek(body_off + 8)
        f.write(np.array([32], dtype="<i4").tobytes())
    with pytest.raises(kaldi_io.BadInputFormat) as e:
        loader.load_compressed([0, 1, 2], buf)
    assert "utt01" in str(e.value) or lines[1].split(None, 1)[1] in str(e.value)
    loader.close()


# ----------------------------------------------------------------------------------------------------------------------------------
def read_all(reader, feats, byte_buffer, max_utts=1024):
    groups = []
    while True:
        keys, offs, frames = reader.read_group(feats, max_utts, byte_buffer=byte_buffer) if byte_buffer is not None else reader.read_group(feats, max_utts)
        if not keys:
            return groups
        groups.append((keys, np.array(offs), frames))


def aligned(n):
    raw = np.zeros(n + 16, dtype=np.uint8)
    return raw[(-raw.ctypes.data) % 16:][:n]


def test_groups_are_cut_where_the_kind_changes(tmp_path):
    ee = load_script()
    scp, lines, bodies = write_table(tmp_path)
    reader = ee.ScpGroupReader(ee.read_scp("scp:" + scp), threads=2)
    feats, buf = np.zeros((4096, DIM), dtype=np.float32), aligned(1 << 17)
    groups = read_all(reader, feats, buf)
    reader.close()
    assert [k for g in groups for k in g[0]] == ["utt%02d" % i for i in range(len(KINDS))]          # every key once, in scp order
    is_c = [kind in FORMAT for kind in KINDS]
    runs = [[0]]
    for i in range(1, len(KINDS)):
        if is_c[i] != is_c[i - 1]:
            runs.append([])
        runs[-1].append(i)
    assert [g[0] for g in groups] == [["utt%02d" % i for i in run] for run in runs]
    rows = want_rows()
    for (keys, offs, frames), run in zip(groups, runs):
        assert offs.tolist() == np.concatenate([[0], np.cumsum([rows[i] for i in run])]).tolist()
        if is_c[run[0]]:
            assert isinstance(frames, ee.CompressedGroup) and frames.frames == offs[-1] and frames.frame_off.tolist() == offs.tolist()
            assert frames.formats.tolist() == [FORMAT[KINDS[i]] for i in run] and (frames.byte_off % 16 == 0).all()
        else:
            assert frames == offs[-1]
    # without a byte buffer nothing changes: one group, decoded on the host
    reader = ee.ScpGroupReader(ee.read_scp("scp:" + scp), threads=2)
    one = read_all(reader, feats, None)
    reader.close()
    assert len(one) == 1 and one[0][2] == sum(rows) and one[0][0] == ["utt%02d" % i for i in range(len(KINDS))]
    for i, kind in enumerate(KINDS):
        if kind in FORMAT:
            a = int(one[0][1][i])
            assert np.array_equal(feats[a:a + ROWS[i]].view(np.uint32), cc.host_decode(*bodies[i]).view(np.uint32))


def test_groups_are_cut_at_the_byte_cap_and_by_rows(tmp_path):
    ee = load_script()
    kinds, rows = ["CM ", "CM2", "CM ", "CM3", "CM ", "CM2", "CM "], [50, 50, 50, 50, 50, 50, 50]
    scp, lines, bodies = write_table(tmp_path, kinds, rows)
    size = lambda fmt: (16 + {1: 8 * DIM + 50 * DIM, 2: 2 * 50 * DIM, 3: 50 * DIM}[fmt] + 15) // 16 * 16
    sizes = [size(FORMAT[k]) for k in kinds]
    assert sizes[1] == (16 + 2 * 50 * DIM + 15) // 16 * 16 and sizes[1] > sizes[0] > sizes[3]          # 'CM2': twice the data bytes
    feats = np.zeros((4096, DIM), dtype=np.float32)
    cap = sizes[0] + sizes[1] + sizes[2] + 8                                                               # three fit, the fourth does not
    reader = ee.ScpGroupReader(ee.read_scp("scp:" + scp))
    groups = read_all(reader, feats, aligned(cap))
    reader.close()
    want, used = [[]], 0
    for i, s in enumerate(sizes):
        if used + s > cap:
            want.append([])
            used = 0
        want[-1].append("utt%02d" % i)
        used += s
    assert [g[0] for g in groups] == want and len(want) == 3
    assert all(isinstance(g[2], ee.CompressedGroup) and g[2].used_bytes <= cap for g in groups)
    # an entry whose body does not fit the byte buffer at all takes the host decode, in its place
    reader = ee.ScpGroupReader(ee.read_scp("scp:" + scp))
    groups = read_all(reader, feats, aligned(sizes[0] + 16))
    reader.close()
    assert [g[0] for g in groups] == [["utt00"], ["utt01"], ["utt02"], ["utt03"], ["utt04"], ["utt05"], ["utt06"]]
    assert [isinstance(g[2], ee.CompressedGroup) for g in groups] == [True, False, True, True, True, False, True]
    assert np.array_equal(feats[:50].view(np.uint32), cc.host_decode(*bodies[5]).view(np.uint32))          # (the last host-decoded group: utt05)
    # the row cap cuts a compressed group as it cuts any other (same batches on both routes)
    for byte_buffer in (aligned(1 << 16), None):
        reader = ee.ScpGroupReader(ee.read_scp("scp:" + scp))
        reader.row_pad = 4
        groups = read_all(reader, np.zeros((170, DIM), dtype=np.float32), byte_buffer)
        reader.close()
        assert [len(g[0]) for g in groups] == [3, 3, 1]
    # an utterance longer than a whole batch buffer stays on the host path
    reader = ee.ScpGroupReader(ee.read_scp("scp:" + scp))
    keys, offs, frames = reader.read_group(np.zeros((40, DIM), dtype=np.float32), 1024, byte_buffer=aligned(1 << 16))
    reader.close()
    assert keys == ["utt00"] and isinstance(frames, np.ndarray) and np.array_equal(frames.view(np.uint32), cc.host_decode(*bodies[0]).view(np.uint32))
