"""Host side of the device compressor and of makeFeatures.py / computeVad.py: the C ABI declaration and its refusals (before any device
call), the NumPy restatement of the quantiser against the fixture decoded by the reference's reader, its error bound, the Kaldi .conf
reader, the compressed ark writer and the command lines' refusals - no GPU."""

import ctypes as C
import importlib.util
import io
import logging
import os
import re
import struct
import subprocess
import wave

import numpy as np
import pytest

import compress_cases as cc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "compress_roundtrip.npz")
TOKEN = {1: b"CM ", 2: b"CM2 "}


def load_script(name):
    spec = importlib.util.spec_from_file_location(name.replace(".", "_"), os.path.join(REPO, "asv-subtools_amd", name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def host_decode(fmt, body):
    from libs.support import kaldi_io
    return np.ascontiguousarray(kaldi_io.read_mat(io.BytesIO(b"\0B" + TOKEN[fmt] + body)), dtype=np.float32)


# ----------------------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_listed_and_exported():
    from libs.amd import capi
    hdr = open(os.path.join(REPO, "include", "asv_amd.h")).read()
    assert re.search(r"\bint\s+asv_encode_compressed\s*\(", hdr)
    assert hdr.index("asv_encode_compressed(") > hdr.index("int asv_decode_compressed(")
    assert "asv_encode_compressed" in capi.SYMBOLS
    assert len(capi.lib().asv_encode_compressed.argtypes) == 9
    exported = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT asv_encode_compressed\b", exported)
    mk = open(os.path.join(REPO, "asv-subtools_amd", "csrc", "Makefile")).read()
    assert "kernels_encode.hip" in mk and re.search(r"CXXFLAGS_kernels_encode\s*=.*-ffp-contract=off", mk)
    assert "#pragma clang fp contract(off)" in open(os.path.join(REPO, "asv-subtools_amd", "csrc", "kernels_encode.hip")).read()


def test_bad_arguments_are_refused_before_any_device_call():
    from libs.amd import capi
    lib = capi.lib()
    p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_longlong))
    pu8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_ubyte))
    # 2 utterances of 9 and 3 rows, dim 4: 'CM ' body of 16 + 32 + 36 = 84 bytes at 0, 'CM2' body at 96
    frame_off, byte_off, formats = np.array([0, 9, 12], dtype=np.int64), np.array([0, 96], dtype=np.int64), np.array([1, 2], dtype=np.uint8)
    # (host memory stands in for the device pointers: every refusal below comes before the library looks at them)
    fake = np.zeros(512, dtype=np.uint8)
    ptr = fake.ctypes.data

    def refused(f=frame_off, b=byte_off, fmt=formats, n=2, dim=4, feats=ptr, out=ptr, status=ptr, word=None):
        rc = lib.asv_encode_compressed(feats, p64(f) if f is not None else None, p64(b) if b is not None else None, pu8(fmt) if fmt is not None else None,
                                       n, dim, out, status, None)
        msg = lib.asv_last_error()
        assert rc < 0 and b"asv_encode_compressed" in msg, (rc, msg)
        if word is not None:
            assert word in msg, msg

    for kw in ({"feats": None}, {"f": None}, {"b": None}, {"fmt": None}, {"out": None}, {"status": None}):
        refused(word=b"null", **kw)
    refused(n=0)
    refused(n=-3)
    refused(dim=0)
    refused(f=np.array([0, 9, 9], dtype=np.int64))                                 # an empty utterance
    refused(f=np.array([0, 9, 5], dtype=np.int64))                                 # decreasing
    refused(f=np.array([1, 9, 12], dtype=np.int64))                                # not from 0
    refused(f=np.array([0, 0, 3], dtype=np.int64), fmt=np.array([1, 2], dtype=np.uint8))      # format 1 with fewer than 1 row
    for bad in (8, 100, 97):
        refused(b=np.array([0, bad], dtype=np.int64), word=b"16")
    refused(b=np.array([0, 80], dtype=np.int64))                                   # inside the body in front (84 bytes)
    refused(b=np.array([96, 0], dtype=np.int64))                                   # not increasing
    refused(b=np.array([-16, 96], dtype=np.int64))
    for fmt in (0, 3, 4, 255):
        refused(fmt=np.array([1, fmt], dtype=np.uint8), word=b"format")


def test_wrapper_and_layout_helpers():
    from libs.amd import frontend
    assert callable(frontend.encode_compressed) and callable(frontend.read_wav_pcm16)
    assert frontend.compressed_auto_format(np.array([1, 8, 9, 1000])).tolist() == [2, 2, 1, 1]
    assert [cc.auto_format(r) for r in (1, 8, 9, 1000)] == [2, 2, 1, 1]


# ----------------------------------------------------------------------------------------------------------------------------------
def golden_entries():
    z = np.load(GOLDEN)
    for name in z.files:
        if name.startswith("in_"):
            tag = name[3:]
            yield tag, int(tag.split("_")[1]), z[name], z["body_" + tag].tobytes(), (z["ref_" + tag] if "ref_" + tag in z.files else None)


def check_bound(mat, fmt, body):
    """max of |decoded - x| / (step / 2 + range / 65535) over the matrix"""
    dec = host_decode(fmt, body).astype(np.float64)
    ratio = np.abs(dec - mat.astype(np.float64)) / cc.error_bound(mat, fmt, body)
    return float(ratio.max())


def check_structure(mat, fmt, body):
    rows, cols = mat.shape
    mn, rng, r, c = struct.unpack("<ffii", body[:16])
    assert (r, c) == (rows, cols) and rng > 0 and np.isfinite(mn) and np.isfinite(rng)
    from libs.amd import frontend
    assert len(body) == int(frontend.compressed_body_bytes(fmt, rows, cols))
    if fmt == 1:
        pct = np.frombuffer(body[16:16 + 8 * cols], dtype="<u2").reshape(cols, 4).astype(np.int64)
        assert (np.diff(pct, axis=1) > 0).all(), "percentiles must increase strictly"
        assert (pct[:, 0] <= 65532).all()


def test_golden_bodies_are_reproduced_and_read_as_the_reference_reads_them():
    z = np.load(GOLDEN)
    assert z["cases"].tolist() == ["%s %d %d" % c for c in cc.GOLDEN_CASES]
    kinds, n, n_ref = set(), 0, 0
    for i, (kind, rows, cols) in enumerate(cc.GOLDEN_CASES):
        kinds.add(kind)
        assert np.array_equal(cc.make_matrix(kind, rows, cols, seed=i).view(np.uint32), z["in_%02d_1" % i].view(np.uint32))
    assert kinds == set(cc.KINDS)
    for tag, fmt, mat, body, ref in golden_entries():
        got_fmt, got = cc.kaldi_compress(mat, fmt=fmt)
        assert got_fmt == fmt and got == body, tag                                  # byte for byte
        if mat.shape[0] > 8 or fmt == 2:
            assert cc.kaldi_compress(mat)[0] == fmt                                 # the automatic choice
        dec = host_decode(fmt, body)
        if ref is not None:
            assert np.array_equal(dec.view(np.uint32), ref.view(np.uint32)), tag    # the repo's reader = the reference's
            n_ref += 1
        worst = check_bound(mat, fmt, body)
        print("%s %s: worst |decoded - x| / bound = %.4f" % (tag, mat.shape, worst))
        assert worst <= 1.0, (tag, worst)
        check_structure(mat, fmt, body)
        n += 1
    assert n >= 12 and n_ref >= 10


def test_the_bound_holds_over_the_prototype_sweep():
    """|decoded - x| <= step / 2 + range / 65535 for every value: rows x columns x kinds of the prototype, nothing excluded."""
    worst = 0.0
    for rows in (1, 2, 4, 5, 8, 9, 63, 64, 65, 257, 1000):
        for cols in (1, 23, 80):
            for kind in ("normal", "ties", "constant", "max_col", "fbank"):
                mat = cc.make_matrix(kind, rows, cols, seed=3)
                fmt, body = cc.kaldi_compress(mat)
                assert fmt == (1 if rows > 8 else 2)
                check_structure(mat, fmt, body)
                ratio = check_bound(mat, fmt, body)
                assert ratio <= 1.0, (kind, rows, cols, ratio)
                worst = max(worst, ratio)
    print("worst |decoded - x| / bound over the sweep: %.4f" % worst)


def test_format_rule_and_the_short_column_chain():
    rng = np.random.RandomState(5)
    assert cc.kaldi_compress(rng.randn(8, 3))[0] == 2 and cc.kaldi_compress(rng.randn(9, 3))[0] == 1
    for rows in (1, 2, 3, 4):
        mat = rng.randn(rows, 6).astype(np.float32)
        fmt, body = cc.kaldi_compress(mat, fmt=1)
        check_structure(mat, 1, body)
        pct = np.frombuffer(body[16:16 + 48], dtype="<u2").reshape(6, 4).astype(np.int64)
        for k in range(rows, 4):
            assert (pct[:, k] == pct[:, k - 1] + 1).all()                           # no such element: previous + 1
    fmt, body = cc.kaldi_compress(np.full((12, 2), 3.0, dtype=np.float32))          # max == min -> range 1 + |min|
    assert struct.unpack("<ff", body[:8]) == (3.0, 4.0)
    assert np.frombuffer(body[16:32], dtype="<u2").tolist() == [0, 1, 2, 3] * 2


# ----------------------------------------------------------------------------------------------------------------------------------
# the reference's conf/*.conf (settings only)
CONFS = {
    "sre-fbank-81.conf": ("fbank", "--sample-frequency=16000\n--use-energy=true\n--low-freq=40\n--high-freq=-200\n--num-mel-bins=80\n--frame-length=25\n--frame-shift=10\n--dither=0\n"),
    "sre-fbank-40.conf": ("fbank", "--sample-frequency=16000\n--use-energy=true\n--low-freq=40\n--high-freq=-200\n--num-mel-bins=40\n--frame-length=25\n--frame-shift=10\n"),
    "sre-mfcc-23.conf": ("mfcc", "--sample-frequency=16000\n--frame-length=25 # the default is 25.\n--low-freq=40 # the default.\n--num-mel-bins=23\n"
                                 "--high-freq=-200 # the default is zero meaning use the Nyquist (8k in this case).\n--num-ceps=23 # higher than the default which is 12.\n\n"),
    "sre-plp-20.conf": ("plp", "--sample-frequency=16000\n--frame-length=25 # the default is 25.\n--low-freq=40 # the default.\n--num-mel-bins=23\n--lpc-order=19\n"
                               "--high-freq=-200 # the default is zero meaning use the Nyquist (8k in this case).\n--num-ceps=20 # higher than the default which is 12.\n\n"),
    "asvspoof-fbank-160.conf": ("fbank", "--sample-frequency=16000 \n--frame-length=50\n--frame-shift=4\n--num-mel-bins=160\n--use-energy=false\n--high-freq=0\n--low-freq=0\n"
                                         "--remove-dc-offset=false\n"),
    "asvspoof-spectrogram.conf": ("spectrogram", "--sample-frequency=16000\n--frame-length=25\n--frame-shift=4\n--raw-energy=false\n--remove-dc-offset=false\n"),
}
VAD_55 = "--vad-energy-threshold=5.5\n--vad-energy-mean-scale=0.5\n"


def test_conf_reader_types_and_kaldi_defaults(tmp_path, caplog):
    from libs.amd import frontend, kaldi_conf
    kind, text = CONFS["sre-fbank-81.conf"]
    path = tmp_path / "sre-fbank-81.conf"
    path.write_text(text)
    with caplog.at_level(logging.WARNING, logger="asv_amd.kaldi_conf"):
        o = kaldi_conf.read_feature_conf(str(path), kind)
    assert not [r for r in caplog.records if "dither" in r.getMessage()]            # the file sets it
    assert o["sample_frequency"] == 16000.0 and isinstance(o["sample_frequency"], float)
    assert o["use_energy"] is True and o["num_mel_bins"] == 80 and isinstance(o["num_mel_bins"], int)
    assert (o["low_freq"], o["high_freq"], o["frame_length"], o["frame_shift"], o["dither"]) == (40.0, -200.0, 25.0, 10.0, 0.0)
    # what the conf omits: Kaldi's FbankOptions / FrameExtractionOptions / MelBanksOptions, not torchaudio's
    assert o["energy_floor"] == 0.0 and frontend._DEFAULTS["energy_floor"] == 1.0
    assert (o["preemphasis_coefficient"], o["window_type"], o["snip_edges"], o["remove_dc_offset"], o["raw_energy"]) == (0.97, "povey", True, True, True)
    assert frontend.feature_dim(kind, **o) == 81
    # every file parses, and the dict is one the front-end accepts
    for name, (kind, text) in CONFS.items():
        o = kaldi_conf.read_feature_conf(text, kind)
        frontend.fbank_options(kind, **o)
        assert o["dither"] == 0.0
    m = kaldi_conf.read_feature_conf(CONFS["sre-mfcc-23.conf"][1], "mfcc")
    assert (m["num_ceps"], m["num_mel_bins"], m["use_energy"], m["cepstral_lifter"], m["low_freq"]) == (23, 23, True, 22.0, 40.0)      # MfccOptions: use_energy true
    assert frontend._MFCC_DEFAULTS["use_energy"] is False
    p = kaldi_conf.read_feature_conf(CONFS["sre-plp-20.conf"][1], "plp")
    assert (p["lpc_order"], p["num_ceps"], p["compress_factor"], p["cepstral_scale"], p["use_energy"]) == (19, 20, 0.33333, 1.0, True)
    s = kaldi_conf.read_feature_conf(CONFS["asvspoof-spectrogram.conf"][1], "spectrogram")
    assert s["raw_energy"] is False and s["remove_dc_offset"] is False and s["frame_shift"] == 4.0 and "num_mel_bins" not in s
    assert kaldi_conf.read_feature_conf("", "fbank")["num_mel_bins"] == 23 and kaldi_conf.read_feature_conf("", "mfcc")["num_ceps"] == 13


def test_conf_reader_dither_and_unknown_keys(caplog):
    from libs.amd import kaldi_conf
    with caplog.at_level(logging.WARNING, logger="asv_amd.kaldi_conf"):
        o = kaldi_conf.read_feature_conf(CONFS["sre-fbank-40.conf"][1], "fbank")
    notes = [r.getMessage() for r in caplog.records if "dither" in r.getMessage()]
    assert o["dither"] == 0.0 and len(notes) == 1 and "not applied" in notes[0]
    with pytest.raises(ValueError, match="dither"):
        kaldi_conf.read_feature_conf("--dither=1\n", "fbank")
    assert kaldi_conf.read_feature_conf("--dither=0.0\n", "fbank")["dither"] == 0.0
    with pytest.raises(ValueError, match="--num-cepstra"):
        kaldi_conf.read_feature_conf("--num-cepstra=20\n", "mfcc")
    with pytest.raises(ValueError, match="--num-ceps"):
        kaldi_conf.read_feature_conf("--num-ceps=20\n", "fbank")                   # a key of another feature kind
    with pytest.raises(ValueError, match="num-mel-bins"):
        kaldi_conf.read_feature_conf("--num-mel-bins=many\n", "fbank")
    with pytest.raises(ValueError, match="line 2"):
        kaldi_conf.read_feature_conf("--num-mel-bins=40\nnum-ceps 3\n", "fbank")


def test_vad_conf_takes_compute_vad_defaults():
    from libs.amd import kaldi_conf
    v = kaldi_conf.read_vad_conf(VAD_55)
    assert (v["vad_energy_threshold"], v["vad_energy_mean_scale"], v["vad_frames_context"], v["vad_proportion_threshold"]) == (5.5, 0.5, 0, 0.6)
    v = kaldi_conf.read_vad_conf("--vad-frames-context=2 # wider\n--vad-proportion-threshold=0.12\n")
    assert (v["vad_energy_threshold"], v["vad_frames_context"], v["vad_proportion_threshold"]) == (5.0, 2, 0.12)
    with pytest.raises(ValueError, match="--vad-energy"):
        kaldi_conf.read_vad_conf("--vad-energy=5\n")


# ----------------------------------------------------------------------------------------------------------------------------------
def test_compressed_ark_scp_round_trip(tmp_path):
    from libs.support import kaldi_io
    mats = [("utt-a", cc.make_matrix("fbank", 57, 23, 1)), ("utt-b", cc.make_matrix("normal", 3, 23, 2)), ("utt-c", cc.make_matrix("ties", 9, 23, 3))]
    items = [(k,) + cc.kaldi_compress(m) for k, m in mats]
    assert [f for _, f, _ in items] == [1, 2, 1]
    ark, scp = str(tmp_path / "raw.ark"), str(tmp_path / "feats.scp")
    kaldi_io.write_compressed_ark_scp(ark, scp, items)
    lines = open(scp).read().splitlines()
    data = open(ark, "rb").read()
    at = 0
    for line, (key, fmt, body) in zip(lines, items):
        k, rx = line.split(" ", 1)
        path, off = rx.rsplit(":", 1)
        assert k == key and path == os.path.abspath(ark)
        assert data[at:at + len(key) + 1] == (key + " ").encode() and int(off) == at + len(key) + 1      # the offset: at the \0B
        assert data[int(off):int(off) + 2 + len(TOKEN[fmt])] == b"\0B" + TOKEN[fmt]
        at = int(off) + 2 + len(TOKEN[fmt]) + len(body)
    assert at == len(data)
    got = list(kaldi_io.read_mat_scp(scp))
    assert [k for k, _ in got] == [k for k, _ in mats]
    for (_, m), (_, fmt, body) in zip(got, items):
        assert np.array_equal(np.ascontiguousarray(m, dtype=np.float32).view(np.uint32), host_decode(fmt, body).view(np.uint32))
    assert [k for k, _ in kaldi_io.read_mat_ark(ark)] == [k for k, _ in mats]
    with pytest.raises(kaldi_io.UnknownMatrixHeader):
        kaldi_io.write_compressed_ark_scp(ark, scp, [("x", 7, b"")])


# ----------------------------------------------------------------------------------------------------------------------------------
def write_wav(path, seconds, rate=16000, seed=0):
    rng = np.random.RandomState(seed)
    x = (3000.0 * rng.randn(int(seconds * rate))).astype("<i2")
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(x.tobytes())


def data_dir(tmp_path, rate=16000, entry=None):
    d = tmp_path / "data" / "train"
    d.mkdir(parents=True)
    write_wav(tmp_path / "a.wav", 0.3, rate)
    (d / "wav.scp").write_text("utt-a %s\n" % (entry or (tmp_path / "a.wav")))
    conf = tmp_path / "fbank.conf"
    conf.write_text("--num-mel-bins=40\n--dither=0\n")
    return str(d), str(conf)


def run_refused(mod, argv, capsys, word):
    with pytest.raises(SystemExit) as e:
        mod.main(argv)
    assert e.value.code == 1
    err = capsys.readouterr().err
    assert word in err, err
    return err


def test_make_features_refusals(tmp_path, capsys, monkeypatch):
    """None of these gets as far as a device: the message names the cause and the exit status is 1."""
    import torch
    monkeypatch.setattr(torch.cuda, "current_device", lambda: pytest.fail("a refused request reached the device"))
    mf = load_script("makeFeatures.py")
    d, conf = data_dir(tmp_path)
    exp = ["--exp", str(tmp_path / "exp")]
    run_refused(mf, exp + ["--pitch", "true", d, "fbank", conf], capsys, "pitch")
    run_refused(mf, exp + ["--cmvn", "true", d, "fbank", conf], capsys, "cmvn")
    run_refused(mf, exp + ["--use-gpu", "false", d, "fbank", conf], capsys, "--use-gpu")
    assert "[exit] Invalid base feature type fbnk ,just fbank/mfcc/plp" in run_refused(mf, exp + [d, "fbnk", conf], capsys, "fbnk")
    run_refused(mf, exp + [d, "fbank"], capsys, "Num of parameters is not equal to 3")
    dither = tmp_path / "dither.conf"
    dither.write_text("--dither=1.0\n")
    run_refused(mf, exp + [d, "fbank", str(dither)], capsys, "dither")
    unknown = tmp_path / "unknown.conf"
    unknown.write_text("--num-mel-bin=40\n")
    run_refused(mf, exp + [d, "fbank", str(unknown)], capsys, "--num-mel-bin")
    # the three kinds of input this path does not read
    open(os.path.join(d, "segments"), "w").write("seg-a utt-a 0.0 0.2\n")
    run_refused(mf, exp + [d, "fbank", conf], capsys, "segments")
    os.remove(os.path.join(d, "segments"))
    open(os.path.join(d, "wav.scp"), "w").write("utt-a sox %s -t wav - |\n" % (tmp_path / "a.wav"))
    assert "utt-a" in run_refused(mf, exp + [d, "fbank", conf], capsys, "|")
    assert not os.path.exists(os.path.join(d, "feats.scp"))


def test_a_rate_mismatch_is_refused_by_name(tmp_path):
    from libs.amd import featprep
    d, conf = data_dir(tmp_path, rate=8000)
    with pytest.raises(featprep.Refused, match="8000 Hz.*sample_frequency 16000"):
        list(featprep._batches(featprep.read_wav_scp(d), 16000.0, 1200.0, 512, 2))
    assert featprep.data_name("data/train/") == "data_train" and featprep.data_name("/x//y/z") == "x_y_z" and featprep.data_name("train") == "train"


def test_compute_vad_refusals(tmp_path, capsys):
    cv = load_script("computeVad.py")
    run_refused(cv, [str(tmp_path)], capsys, "Num of parameters is not equal to 2")
    bad = tmp_path / "vad.conf"
    bad.write_text("--vad-energy=5\n")
    (tmp_path / "feats.scp").write_text("")
    run_refused(cv, [str(tmp_path), str(bad)], capsys, "--vad-energy")
