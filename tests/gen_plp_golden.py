"""Writes tests/golden/plp_spectrogram.npz: the int16 wave bank of tests/plp_cases.py, and for every case there the outputs of the
REFERENCE's own PLP / spectrogram code (runtime/kaldifeat/csrc, float32), its frame offsets, and e_ref = the largest distance of those
outputs from the float64 restatement (the yardstick of the device tests: the device must stay within 4 e_ref of the restatement).

    python tests/gen_plp_golden.py --reference /path/to/reference/runtime | --lib prebuilt.so

The reference's sources are compiled where they lie, together with tests/plp_ref_wrap.cc, into a temporary directory that is removed
afterwards (g++ -O1, the flags of oracle/Makefile.ref; about two minutes).  Nothing compiled is kept, no test runs this script, and
the tests read the .npz only.  Every reference value must be finite, and no spectrogram case may need more than
plp_cases.EXCLUDE_FRACTION of its values left out: the script checks both.
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [HERE, REPO, os.path.join(REPO, "asv-subtools_amd", "pytorch")]

import plp_cases as P          # noqa: E402

SRCS = ["feature-plp.cc", "feature-spectrogram.cc", "feature-window.cc", "feature-functions.cc", "mel-computations.cc", "matrix-functions.cc"]


def build(ref_runtime, out_dir):
    import torch
    tdir = os.path.dirname(torch.__file__)
    lib = os.path.join(out_dir, "libplp_ref.so")
    cmd = ["g++", "-O1", "-std=c++17", "-fPIC", "-D_GLIBCXX_USE_CXX11_ABI=%d" % int(torch._C._GLIBCXX_USE_CXX11_ABI), "-I" + ref_runtime,
           "-I" + os.path.join(tdir, "include"), "-I" + os.path.join(tdir, "include", "torch", "csrc", "api", "include"), "-shared", "-o", lib,
           os.path.join(HERE, "plp_ref_wrap.cc")] + [os.path.join(ref_runtime, "kaldifeat", "csrc", s) for s in SRCS] + \
          ["-L" + os.path.join(tdir, "lib"), "-ltorch", "-ltorch_cpu", "-lc10", "-Wl,-rpath," + os.path.join(tdir, "lib")]
    subprocess.check_call(cmd)
    return lib


def reference(lib, kind, o, wave):
    wave = np.ascontiguousarray(wave, dtype=np.float32)
    cap = max(1, P.F.num_frames(len(wave), o["sample_frequency"], o["frame_length"], o["frame_shift"], o["snip_edges"])) + 2
    out = np.zeros((cap, 2048), dtype=np.float32)
    dim = C.c_int(0)
    fp, ci, cf = C.POINTER(C.c_float), C.c_int, C.c_float
    frame = [wave.ctypes.data_as(fp), ci(len(wave)), cf(o["sample_frequency"]), cf(o["frame_length"]), cf(o["frame_shift"]),
             cf(o["preemphasis_coefficient"]), ci(o["remove_dc_offset"]), o["window_type"].encode(), ci(o["round_to_power_of_two"]), ci(o["snip_edges"])]
    tail = [out.ctypes.data_as(fp), ci(cap), C.byref(dim)]
    if kind == "plp":
        assert float(o["cepstral_lifter"]) == int(o["cepstral_lifter"])          # an int32 in the reference's PlpOptions
        n = lib.plp_ref_plp(*frame, ci(o["num_mel_bins"]), cf(o["low_freq"]), cf(o["high_freq"]), cf(o["vtln_warp"]), cf(o["vtln_low"]), cf(o["vtln_high"]),
                            ci(o["lpc_order"]), ci(o["num_ceps"]), cf(o["compress_factor"]), ci(int(o["cepstral_lifter"])), cf(o["cepstral_scale"]),
                            ci(o["use_energy"]), cf(o["energy_floor"]), ci(o["raw_energy"]), ci(o["htk_compat"]), *tail)
    else:
        n = lib.plp_ref_spectrogram(*frame, cf(o["energy_floor"]), ci(o["raw_energy"]), *tail)
    assert n >= 0
    return out.reshape(-1)[:n * dim.value].reshape(n, dim.value).copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="", help="the reference's runtime/ directory")
    ap.add_argument("--lib", default="", help="a library built by an earlier run (skips the compilation)")
    ap.add_argument("--out", default=P.GOLDEN)
    args = ap.parse_args()
    if not (args.reference or args.lib):
        ap.error("one of --reference and --lib is needed")
    with tempfile.TemporaryDirectory() as tmp:
        lib = C.CDLL(args.lib or build(args.reference, tmp))
        bank = P.make_bank()
        fixture = {"wave_" + k: v for k, v in bank.items()}
        for name, kind, kw, utts in P.CASES:
            o = P.full_options(kind, kw)
            rows, off, want = [], [0], []
            for u in utts:
                w = bank[u].astype(np.float32)
                if len(w) < P.F.window_size(o["sample_frequency"], o["frame_length"]) and o["snip_edges"]:
                    r = np.zeros((0, 0), dtype=np.float32)                        # the reference does not take a wave without a frame
                else:
                    r = reference(lib, kind, o, w)
                w64 = P.restate(kind, w, o, np.float64)
                assert r.shape[0] == w64.shape[0] and (r.shape[0] == 0 or r.shape == w64.shape), (name, u, r.shape, w64.shape)
                assert np.isfinite(r).all(), (name, u)
                rows.append(r.reshape(r.shape[0], w64.shape[1]))
                want.append(w64)
                off.append(off[-1] + r.shape[0])
            ref, want = np.concatenate(rows, axis=0), np.concatenate(want, axis=0)
            keep = P.mask_of(kind, want)
            err = np.abs(ref.astype(np.float64) - want)
            e_ref = float(err[keep].max())
            w32 = np.concatenate([P.restate(kind, bank[u].astype(np.float32), o, np.float32) for u in utts], axis=0)
            print("%-24s %4d x %3d  |ref| <= %8.3f  e_ref %.3e  (all values: %.3e)  f32 restatement vs f64 %.3e  vs reference %.3e" % (
                name, ref.shape[0], ref.shape[1], np.abs(ref).max(), e_ref, err.max(), np.abs(w32.astype(np.float64) - want)[keep].max(),
                np.abs(w32.astype(np.float64) - ref)[keep].max()))
            fixture["ref_" + name] = ref
            fixture["off_" + name] = np.asarray(off, dtype=np.int64)
            fixture["eref_" + name] = np.float64(e_ref)
            fixture["opts_" + name] = np.frombuffer(P.options_json(name).encode(), dtype=np.uint8)
        np.savez_compressed(args.out, **fixture)
    print("%s: %d bytes" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
