# -*- coding:utf-8 -*-
"""What the ivector-adapt-plda*.py scripts of this directory share: the reference's command line (positional arguments only,
the usage line and a plain exit when their count is wrong) plus `--gpu-id N`, reading the adaptation vectors, writing the
Kaldi text <Plda>.  The adaptation-set statistics are accumulated on the MI355X (asv_scatter_f64); there is no CPU path: a
script that needs them exits non-zero without a ROCm device or the library.
"""

import os
import sys
import traceback

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "pytorch"))


def parse(argv, usage, count):
    """-> (positional arguments, gpu id string).  `--gpu-id N` / `--gpu-id=N` may stand anywhere; with another number of
    positional arguments than `count` the usage line is printed and the process ends as the reference's does (sys.exit())."""
    args, gpu_id, i = [], "", 1
    while i < len(argv):
        a = argv[i]
        if a == "--gpu-id" and i + 1 < len(argv):
            gpu_id, i = argv[i + 1], i + 2
        elif a.startswith("--gpu-id="):
            gpu_id, i = a.split("=", 1)[1], i + 1
        else:
            args.append(a)
            i += 1
    if len(args) != count:
        print(usage + " \n")
        sys.exit()
    return args, gpu_id


def select_device(gpu_id):
    """`--gpu-id N`: the device the statistics kernel runs on (default: the current one)."""
    if gpu_id != "":
        import torch
        torch.cuda.set_device(int(gpu_id))


def read_vectors(rspecifier):
    """'ark:...' / 'scp:...' -> [n, dim] float32, as the reference's `for _, vec in kaldi_io.read_vec_flt_auto(...)` loop sees them."""
    from libs.support import kaldi_io
    vecs = [np.asarray(v, dtype=np.float32) for _, v in kaldi_io.read_vec_flt_auto(rspecifier)]
    if not vecs:
        raise ValueError("%s: no vectors" % rspecifier)
    return np.stack(vecs)


def run(body):
    """Runs body(); any error is printed and becomes exit status 1."""
    try:
        body()
    except SystemExit:
        raise
    except BaseException as e:
        if not isinstance(e, KeyboardInterrupt):
            traceback.print_exc()
        sys.exit(1)
