#!/usr/bin/env python3
"""Generate tests/golden/compress_roundtrip.npz: the NumPy restatement of Kaldi's compressed-matrix quantiser (compress_cases.kaldi_compress)
on a dozen small matrices, each payload decoded by the REFERENCE's own reader (pytorch/libs/support/kaldi_io.py read_mat; 'CM ' only - it
refuses 'CM2', for which the fixture keeps input and body alone).  Data only: the inputs, the bodies, the reference-decoded floats.

Build container only (needs the reference tree, read-only):   PYTHONDONTWRITEBYTECODE=1 python tests/gen_compress_golden.py
"""
import io
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import compress_cases as cc  # noqa: E402


def reference_kaldi_io():
    for n, attrs in (("tkinter", {"N": None}), ("tkinter.messagebox", {"NO": None}), ("turtle", {"xcor": None})):      # stray imports of the reference tree
        m = types.ModuleType(n)
        m.__dict__.update(attrs)
        m.__path__ = []
        sys.modules.setdefault(n, m)
    import importlib.util
    spec = importlib.util.spec_from_file_location("reference_kaldi_io", os.path.join(REF, "pytorch", "libs", "support", "kaldi_io.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = reference_kaldi_io()
    out = {"cases": np.array(["%s %d %d" % c for c in cc.GOLDEN_CASES])}
    for i, (kind, rows, cols) in enumerate(cc.GOLDEN_CASES):
        mat = cc.make_matrix(kind, rows, cols, seed=i)
        for fmt in ((1, 2) if rows <= 8 else (1,)):                 # small matrices: the automatic 'CM2' and a forced 'CM ' (the n < 5 chain)
            f, body = cc.kaldi_compress(mat, fmt=fmt)
            assert f == fmt
            tag = "%02d_%d" % (i, fmt)
            out["in_" + tag] = mat
            out["body_" + tag] = np.frombuffer(body, dtype=np.uint8)
            if fmt == 1:
                dec = ref.read_mat(io.BytesIO(b"\0BCM " + body))
                out["ref_" + tag] = np.ascontiguousarray(dec, dtype=np.float32)
                assert out["ref_" + tag].shape == mat.shape
    path = os.path.join(HERE, "golden", "compress_roundtrip.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
