"""asv_encode_compressed (csrc/kernels_encode.hip) against the NumPy restatement of Kaldi's quantiser (tests/compress_cases.py): BYTE
equality, no tolerance, with canary bytes around and between the bodies; then makeFeatures.py / computeVad.py end to end on synthetic
wavs."""

import ctypes as C
import importlib.util
import io
import os
import wave

import numpy as np
import pytest

import compress_cases as cc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5
TOKEN = {1: b"CM ", 2: b"CM2 "}


def body_sizes(formats, rows, dim):
    from libs.amd import frontend
    return np.asarray(frontend.compressed_body_bytes(np.asarray(formats), np.asarray(rows), dim), dtype=np.int64)


def run_encode(mats, formats=None, residues=None, front=64, back=64):
    """The C entry point on a canary-filled buffer -> (buffer uint8 host, byte_off, formats, status host, sizes).  residues[u]: body u
    starts at the next offset with that residue mod 64 (a multiple of 16).  Asserts that the input rows came through unchanged."""
    import torch
    from libs.amd import capi
    dim = mats[0].shape[1]
    rows = np.array([m.shape[0] for m in mats], dtype=np.int64)
    frame_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    formats = np.array([cc.auto_format(r) for r in rows] if formats is None else formats, dtype=np.uint8)
    sizes = body_sizes(formats, rows, dim)
    byte_off, at = np.zeros(len(mats), dtype=np.int64), front
    for u in range(len(mats)):
        while residues is not None and at % 64 != residues[u]:
            at += 16
        byte_off[u] = at
        at += (int(sizes[u]) + 15) // 16 * 16
    host_in = np.ascontiguousarray(np.concatenate(mats, axis=0), dtype=np.float32)
    feats = torch.from_numpy(host_in).cuda()
    buf = torch.full((at + back,), CANARY, dtype=torch.uint8, device="cuda")
    status = torch.full((len(mats),), -7, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_longlong))
    capi.check(capi.lib().asv_encode_compressed(C.c_void_p(feats.data_ptr()), p64(frame_off), p64(byte_off), formats.ctypes.data_as(C.POINTER(C.c_ubyte)), len(mats), dim,
                                                C.c_void_p(buf.data_ptr()), C.c_void_p(status.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "asv_encode_compressed")
    torch.cuda.synchronize()
    assert np.array_equal(feats.cpu().numpy().view(np.uint32), host_in.view(np.uint32)), "the input rows were changed"
    return buf.cpu().numpy(), byte_off, formats, status.cpu().numpy(), sizes


def expected_buffer(n_bytes, mats, formats, byte_off):
    want = np.full(n_bytes, CANARY, dtype=np.uint8)
    for m, f, a in zip(mats, formats, byte_off):
        fmt, body = cc.kaldi_compress(m, fmt=int(f))
        want[int(a):int(a) + len(body)] = np.frombuffer(body, dtype=np.uint8)
    return want


def assert_same_bytes(got, want, what=""):
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError("%s: %d bytes differ, first at %d (got %d, want %d)" % (what, len(bad), bad[0], got[bad[0]], want[bad[0]]))


def check(mats, formats=None, residues=None):
    got, byte_off, formats, status, _ = run_encode(mats, formats, residues)
    assert status.tolist() == [0] * len(mats)
    assert_same_bytes(got, expected_buffer(len(got), mats, formats, byte_off), str([m.shape for m in mats]))
    return got, byte_off, formats


# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,rows,dim", cc.SHAPE_CASES + [("normal", 65, 33), ("normal", 1000, 32)], ids=lambda v: str(v))
def test_one_matrix_per_call(kind, rows, dim):
    check([cc.make_matrix(kind, rows, dim, seed=1)])


@pytest.mark.parametrize("rows", [1, 2, 3, 4, 5, 8])
def test_short_matrices_forced_to_the_one_byte_format(rows):
    """'CM ' below the automatic rule's 9 rows: the chain over s[0..3] with "previous + 1" for the missing ones (n < 5: no radix select),
    and the first row counts that take it (5, 8)."""
    check([cc.make_matrix("normal", rows, 23, seed=2)], formats=[1])
    check([cc.make_matrix("ties", rows, 65, seed=2)], formats=[1])


@pytest.mark.parametrize("kind,rows,dim", cc.KIND_CASES, ids=lambda v: str(v))
def test_kinds(kind, rows, dim):
    check([cc.make_matrix(kind, rows, dim, seed=4)])


def test_a_long_matrix():
    check([cc.make_matrix("fbank", 20000, 80, seed=5)])


def batch():
    return [cc.make_matrix(("fbank", "normal", "ties")[i % 3], r, 80, seed=10 + i) for i, r in enumerate(cc.BATCH_ROWS)]


def test_a_ragged_batch_in_one_call_and_its_decode():
    import torch
    from libs.amd import frontend
    mats = batch()
    got, byte_off, formats = check(mats)
    assert formats.tolist() == [1, 2, 1, 2, 1, 2, 1]
    # the device decode of the encoded bytes = the host reader on them, by bits
    frame_off = np.concatenate([[0], np.cumsum(cc.BATCH_ROWS)]).astype(np.int64)
    rows = frontend.decode_compressed(torch.from_numpy(got).cuda(), byte_off, frame_off, formats, 80).cpu().numpy()
    from libs.support import kaldi_io
    for u, m in enumerate(mats):
        body = got[int(byte_off[u]):int(byte_off[u]) + int(body_sizes(formats[u], m.shape[0], 80))].tobytes()
        want = np.ascontiguousarray(kaldi_io.read_mat(io.BytesIO(b"\0B" + TOKEN[int(formats[u])] + body)), dtype=np.float32)
        assert np.array_equal(rows[int(frame_off[u]):int(frame_off[u + 1])].view(np.uint32), want.view(np.uint32)), u


def test_the_batch_at_shifted_body_offsets():
    """Bodies start at multiples of 16: they walk the four residues mod 64, neighbours never at the same one (and the columns behind
    them start at every residue mod 4)."""
    mats = batch()
    want = [16, 48, 0, 32, 48, 16, 32]
    got, byte_off, _ = check(mats, residues=want)
    assert (byte_off % 64).tolist() == want


def test_the_wrapper_lays_the_bodies_out_and_picks_the_formats():
    import torch
    from libs.amd import frontend
    mats = batch()
    frame_off = np.concatenate([[0], np.cumsum(cc.BATCH_ROWS)]).astype(np.int64)
    feats = torch.from_numpy(np.concatenate(mats)).cuda()
    out, byte_off, formats, status = frontend.encode_compressed(feats, frame_off)
    assert out.dtype == torch.uint8 and status.dtype == torch.int32 and status.cpu().tolist() == [0] * 7
    assert formats.tolist() == [1, 2, 1, 2, 1, 2, 1] and (byte_off % 16 == 0).all() and byte_off[0] == 0
    host = out.cpu().numpy()
    for m, f, a in zip(mats, formats, byte_off):
        fmt, body = cc.kaldi_compress(m)
        assert fmt == f and host[int(a):int(a) + len(body)].tobytes() == body
    with pytest.raises(ValueError):
        frontend.encode_compressed(feats, np.array([0, 5, 5, feats.shape[0]]))     # an empty utterance


def test_status_flags_a_nan_and_leaves_the_others_exact():
    mats = batch()
    mats[3] = mats[3].copy()
    mats[3][2, 17] = np.nan
    got, byte_off, formats, status, sizes = run_encode(mats)
    assert status.tolist() == [0, 0, 0, 1, 0, 0, 0]
    clean = [m if u != 3 else np.zeros_like(m) for u, m in enumerate(mats)]
    want = expected_buffer(len(got), clean, formats, byte_off)
    a, b = int(byte_off[3]), int(byte_off[3]) + int(sizes[3])
    got[a:b] = want[a:b]                                                        # (utterance 3's own span is unspecified)
    assert_same_bytes(got, want, "around the utterance with the NaN")
    mats[5] = mats[5].copy()
    mats[5][0, 0] = -np.inf
    assert run_encode(mats)[3].tolist() == [0, 0, 0, 1, 0, 1, 0]


def test_vad_with_frames_context_zero():
    """compute-vad's defaults (context 0, proportion 0.6): a frame is voiced iff its own energy is above the threshold."""
    import torch
    from libs.amd import frontend
    rng = np.random.RandomState(0)
    rows = (40, 1, 300)
    mats = [(5.0 + 4.0 * rng.rand(r, 5)).astype(np.float32) for r in rows]
    frame_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    voiced, counts = frontend.vad_energy(torch.from_numpy(np.concatenate(mats)).cuda(), frame_off, 5.5, 0.5, 0, 0.6)
    voiced = voiced.cpu().numpy()
    for u, m in enumerate(mats):
        e = m[:, 0]
        thr = np.float32(5.5) + np.float32(0.5) * np.float32(e.astype(np.float64).sum()) / np.float32(len(e))
        want = (e > thr).astype(np.uint8)
        assert np.array_equal(voiced[int(frame_off[u]):int(frame_off[u + 1])], want) and counts[u] == want.sum()
    assert 0 < counts[2] < 300


# ----------------------------------------------------------------------------------------------------------------------------------
def load_script(name):
    spec = importlib.util.spec_from_file_location(name.replace(".", "_"), os.path.join(REPO, "asv-subtools_amd", name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


SECONDS = (0.4, 0.05, 1.2, 0.1, 0.75, 0.2)          # with 60 ms frames: 0.05 s has no frame, 0.1 s has 5 ('CM2')


def make_data(tmp_path):
    d = tmp_path / "data" / "dev"
    d.mkdir(parents=True)
    rng = np.random.RandomState(11)
    waves, lines = {}, []
    for i, s in enumerate(SECONDS):
        n = int(s * 16000)
        x = 3000.0 * rng.randn(n) * (0.002 + (np.sin(np.arange(n) / 1500.0 + i) > 0))      # loud and quiet stretches
        x = x.astype("<i2")
        path = tmp_path / ("w%d.wav" % i)
        with wave.open(str(path), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(16000)
            f.writeframes(x.tobytes())
        waves["utt%d" % i] = x
        lines.append("utt%d %s\n" % (i, path))
    (d / "wav.scp").write_text("".join(lines))
    return str(d), waves


def read_entries(scp):
    """[(key, token, the bytes behind the token up to the next entry's key or the end of the ark)]"""
    lines = [l.split(" ", 1) for l in open(scp).read().splitlines()]
    out = []
    for i, (key, rx) in enumerate(lines):
        path, off = rx.rsplit(":", 1)
        data = open(path, "rb").read()
        end = int(lines[i + 1][1].rsplit(":", 1)[1]) - len(lines[i + 1][0]) - 1 if i + 1 < len(lines) else len(data)
        assert data[int(off):int(off) + 2] == b"\0B"
        token = data[int(off) + 2:int(off) + 5]
        skip = 6 if token == b"CM2" else 5
        out.append((key, token, data[int(off) + skip:end]))
    return out


def test_make_features_and_compute_vad_end_to_end(tmp_path):
    from libs.amd import frontend, kaldi_conf
    from libs.support import kaldi_io
    mf, cv = load_script("makeFeatures.py"), load_script("computeVad.py")
    d, waves = make_data(tmp_path)
    conf, vadconf = tmp_path / "fbank.conf", tmp_path / "vad.conf"
    conf.write_text("--frame-length=60\n--use-energy=true\n")      # (no --dither: read as 0, with a logged note)
    vadconf.write_text("--vad-energy-threshold=5.5\n--vad-energy-mean-scale=0.5\n")
    exp = str(tmp_path / "exp")
    with pytest.warns(UserWarning, match="utt1 is shorter than one frame"):
        mf.main(["--exp", exp, "--vad-config", str(vadconf), d, "fbank", str(conf)])
    keys = [k for k in waves if k != "utt1"]                                    # the 0.05 s file: no frame
    opts = kaldi_conf.read_feature_conf(str(conf), "fbank")
    feats = dict(zip(waves, [t.cpu().numpy() for t in frontend.fbank(list(waves.values()), **opts)]))
    assert feats["utt1"].shape[0] == 0 and feats["utt3"].shape == (5, 24) and feats["utt5"].shape == (15, 24)
    name = "_".join(p for p in d.split("/") if p)
    ark = os.path.join(exp, "fbank", name, "raw_fbank_%s.1.ark" % name)
    assert os.path.exists(ark)
    entries = read_entries(os.path.join(d, "feats.scp"))
    assert [e[0] for e in entries] == keys
    for key, token, body in entries:
        fmt, want = cc.kaldi_compress(feats[key])
        assert token == TOKEN[fmt][:3] and body == want, key
    assert [e[1] for e in entries] == [b"CM ", b"CM ", b"CM2", b"CM ", b"CM "]
    assert open(os.path.join(d, "utt2num_frames")).read() == "".join("%s %d\n" % (k, feats[k].shape[0]) for k in keys)
    # the decisions taken in the same pass = computeVad.py on that feats.scp afterwards
    vad_scp = open(os.path.join(d, "vad.scp")).read()
    vad_ark = os.path.join(exp, "vad", name, "vad_%s.1.ark" % name)
    vad_bytes = open(vad_ark, "rb").read()
    os.remove(os.path.join(d, "vad.scp"))
    os.remove(vad_ark)
    cv.main(["--exp", exp, d, str(vadconf)])
    assert open(os.path.join(d, "vad.scp")).read() == vad_scp and open(vad_ark, "rb").read() == vad_bytes
    flags = dict(kaldi_io.read_vec_flt_scp(os.path.join(d, "vad.scp")))
    assert list(flags) == keys
    for key, m in kaldi_io.read_mat_scp(os.path.join(d, "feats.scp")):          # compute-vad's rule on what a reader of feats.scp sees
        e = np.ascontiguousarray(m, dtype=np.float32)[:, 0]
        thr = np.float32(5.5) + np.float32(0.5) * np.float32(e.astype(np.float64).sum()) / np.float32(len(e))
        assert flags[key].dtype == np.float32 and np.array_equal(flags[key], (e > thr).astype(np.float32)), key
    assert 0 < sum(v.sum() for v in flags.values()) < sum(len(v) for v in flags.values())
    # --compress false: float32 matrices, the front-end's rows by bits
    mf.main(["--exp", exp, "--compress", "false", "--write-utt2num-frames", "false", d, "fbank", str(conf)])
    entries = read_entries(os.path.join(d, "feats.scp"))
    assert [e[0] for e in entries] == keys and {e[1] for e in entries} == {b"FM "}
    for key, m in kaldi_io.read_mat_scp(os.path.join(d, "feats.scp")):
        assert np.array_equal(np.ascontiguousarray(m, dtype=np.float32).view(np.uint32), feats[key].view(np.uint32)), key


def test_make_features_mfcc_and_a_rate_mismatch(tmp_path):
    from libs.amd import frontend, kaldi_conf
    mf = load_script("makeFeatures.py")
    d, waves = make_data(tmp_path)
    conf = tmp_path / "mfcc.conf"
    conf.write_text("--num-ceps=20\n--dither=0\n")
    exp = str(tmp_path / "exp")
    mf.main(["--exp", exp, "--nj", "4", d, "mfcc", str(conf)])
    opts = kaldi_conf.read_feature_conf(str(conf), "mfcc")
    feats = dict(zip(waves, [t.cpu().numpy() for t in frontend.mfcc(list(waves.values()), **opts)]))
    entries = read_entries(os.path.join(d, "feats.scp"))
    assert [e[0] for e in entries] == list(waves)                               # 25 ms frames: the 0.05 s file has 3
    assert [e[1] for e in entries] == [b"CM ", b"CM2", b"CM ", b"CM2", b"CM ", b"CM "]
    for key, token, body in entries:
        assert feats[key].shape[1] == 20 and body == cc.kaldi_compress(feats[key])[1], key
    assert open(os.path.join(d, "utt2num_frames")).read() == "".join("%s %d\n" % (k, feats[k].shape[0]) for k in waves)
    assert not os.path.exists(os.path.join(d, "vad.scp"))
    conf8 = tmp_path / "mfcc8k.conf"
    conf8.write_text("--sample-frequency=8000\n--dither=0\n")
    with pytest.raises(SystemExit):
        mf.main(["--exp", exp, d, "mfcc", str(conf8)])
