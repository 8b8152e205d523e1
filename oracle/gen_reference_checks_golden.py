#!/usr/bin/env python3
"""Generate the fixtures that let the checks against the REFERENCE itself run without it (build container only: needs the
reference tree of oracle/gen_golden.py, read-only, and oracle/_ref from `make -C oracle -f Makefile.ref`):

  tests/golden/reference_differential.npz   the reference's embeddings for every case of tests/test_reference_differential.py
                                            (oracle/gen_golden.py --adhoc: its blueprint + its own extract_embedding() on CPU)
  tests/golden/kaldi_io_reference.npz       what the reference's vendored kaldi_io.py writes / reads for the inputs of
                                            tests/test_host_io.py::test_wire_format_against_the_reference_kaldi_io; it is
                                            also checked here to read back what this repository's kaldi_io writes
  tests/golden/reference_wavs.npz           the first 5 s of the first four recordings of runtime/test/wav (channel 0, int16)
  tests/golden/reference_wavs_features.npz  their fbank-80 and mfcc-20 through the compiled kaldifeat code

    PYTHONDONTWRITEBYTECODE=1 python oracle/gen_reference_checks_golden.py
"""

import ctypes as C
import glob
import importlib.util
import json
import os
import subprocess
import sys
import tempfile
import wave

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
sys.path[:0] = [REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "asv-subtools_amd", "pytorch")]
from oracle.gen_golden import REF  # noqa: E402


def differential():
    import test_reference_differential as T
    specs, out = [], {}
    with tempfile.TemporaryDirectory() as d:
        for i, case in enumerate(T.CASES):
            spec = T.spec_of(case)
            path = os.path.join(d, "adhoc.npz")
            subprocess.run([sys.executable, os.path.join(REPO, "oracle", "gen_golden.py"), "--adhoc", json.dumps(spec), path], check=True,
                           env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
            out["case%02d" % i] = np.load(path)["embeddings"]
            specs.append(spec)
            print("differential %2d %s" % (i, spec["creation"][:70]))
    out["meta"] = np.array(json.dumps(specs))
    np.savez_compressed(os.path.join(GOLDEN, "reference_differential.npz"), **out)


def kaldi_io_wire():
    import test_host_io as T
    from libs.support import kaldi_io
    spec = importlib.util.spec_from_file_location("ref_kaldi_io", os.path.join(REF, "pytorch", "libs", "support", "kaldi_io.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    x = T.wire_format_inputs()
    with tempfile.TemporaryDirectory() as d:
        for name in ("cm", "txt"):
            with open(os.path.join(d, name + ".ark"), "wb") as f:
                f.write(x[name])
        ref_cm = dict(R.read_mat_ark(os.path.join(d, "cm.ark")))["cm"]
        ref_txt = dict(R.read_mat_ark(os.path.join(d, "txt.ark")))["tx"]
        with open(os.path.join(d, "ref_out.ark"), "wb") as f:
            R.write_mat(f, x["m32"], key="a"); R.write_mat(f, x["m64"], key="b"); R.write_vec_flt(f, x["v32"], key="v")
        with open(os.path.join(d, "mine_out.ark"), "wb") as f:
            kaldi_io.write_mat(f, x["m32"], key="a"); kaldi_io.write_mat(f, x["m64"], key="b"); kaldi_io.write_vec_flt(f, x["v32"], key="v")
        got = {}
        with open(os.path.join(d, "mine_out.ark"), "rb") as f:      # the reference reads what this repository wrote
            for read in (R.read_mat, R.read_mat, R.read_vec_flt):
                k = R.read_key(f)
                got[k] = read(f)
        with open(os.path.join(d, "ref_out.ark"), "rb") as f:
            ref_out = f.read()
    assert np.array_equal(got["a"], x["m32"]) and np.array_equal(got["b"], x["m64"]) and np.array_equal(got["v"], x["v32"])
    np.savez_compressed(os.path.join(GOLDEN, "kaldi_io_reference.npz"), ref_out=np.frombuffer(ref_out, dtype=np.uint8),
                        ref_cm=ref_cm, ref_txt=ref_txt)
    print("kaldi_io: %d bytes written by the reference" % len(ref_out))


def reference_wavs():
    from oracle import gen_fbank_golden as G
    lib = C.CDLL(os.path.join(REPO, "oracle", "_ref", "libkaldifeat_ref.so"))
    lib.kaldifeat_ref_fbank.restype = C.c_int
    lib.kaldifeat_ref_mfcc.restype = C.c_int
    waves, feats, meta = {}, {}, []
    for path in sorted(glob.glob(os.path.join(REF, "runtime", "test", "wav", "*.wav")))[:4]:
        name = os.path.splitext(os.path.basename(path))[0]
        with wave.open(path, "rb") as f:
            assert f.getsampwidth() == 2
            sr = f.getframerate()
            pcm = np.frombuffer(f.readframes(min(f.getnframes(), 5 * sr)), dtype="<i2").reshape(-1, f.getnchannels())[:, 0].copy()
        x = pcm.astype(np.float32)
        waves[name] = pcm
        feats[name + "/fbank"] = G.reference_fbank(lib, x, num_bins=80, sample_rate=float(sr))
        feats[name + "/mfcc"] = G.reference_mfcc(lib, x, num_ceps=20, num_bins=30, sample_rate=float(sr))
        meta.append(dict(name=name, sample_rate=sr))
        print("wav %s: %d samples, %d frames" % (name, len(pcm), len(feats[name + "/fbank"])))
    waves["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(GOLDEN, "reference_wavs.npz"), **waves)
    np.savez_compressed(os.path.join(GOLDEN, "reference_wavs_features.npz"), **feats)


if __name__ == "__main__":
    kaldi_io_wire()
    reference_wavs()
    differential()
