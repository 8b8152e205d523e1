#!/usr/bin/env python3
# -*- coding:utf-8 -*-
"""Minimum normalised detection cost of a scored trial list on an MI355X - command-line compatible with the reference's
kaldi/sid/compute_min_dcf.py (called as `sid/compute_min_dcf.py --p-target 0.01 --c-miss 1 --c-fa 1 <scores> <trials>` by
score/pyplda/test_*.sh and the cnsrc recipes): the four-decimal value on stdout, one explanatory line on stderr.

The text files are parsed here; the scores go to the device as float32 and libasv_amd.so sorts and sweeps them
(asv_min_dcf).  There is no CPU path: without a ROCm device or the library this exits non-zero.
"""

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "pytorch"))


def get_args(argv):
    parser = argparse.ArgumentParser(description="Minimum detection cost and the threshold it is reached at.  "
                                     "Usage: sid/compute_min_dcf.py [options] <scores-file> <trials-file>",
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("--p-target", type=float, dest="p_target", default=0.01, help="Prior probability of a target trial.")
    parser.add_argument("--c-miss", type=float, dest="c_miss", default=1, help="Cost of a missed detection.")
    parser.add_argument("--c-fa", type=float, dest="c_fa", default=1, help="Cost of a false alarm.")
    parser.add_argument("scores_filename", help="Rows '<utt1> <utt2> <score>'.")
    parser.add_argument("trials_filename", help="Rows '<utt1> <utt2> <target/nontarget>'.")
    args = parser.parse_args(argv)
    if args.c_fa <= 0:
        raise ValueError("--c-fa must be greater than 0")
    if args.c_miss <= 0:
        raise ValueError("--c-miss must be greater than 0")
    if args.p_target <= 0 or args.p_target >= 1:
        raise ValueError("--p-target must be greater than 0 and less than 1")
    return args


def _rows(path):
    with open(path) as f:
        for n, line in enumerate(f, 1):
            parts = line.split()
            if len(parts) != 3:
                raise ValueError("%s:%d: expected three fields, got %r" % (path, n, line.rstrip("\n")))
            yield parts


def read_scored_trials(scores_filename, trials_filename):
    """-> (scores float64 [n], labels int32 [n]) in the order of the scores file.  Every scored pair must be in the trials file
    (a later line of the trials file overrides an earlier one for the same pair)."""
    kind = {}
    for utt1, utt2, target in _rows(trials_filename):
        kind[(utt1, utt2)] = target
    scores, labels = [], []
    for utt1, utt2, score in _rows(scores_filename):
        if (utt1, utt2) not in kind:
            raise KeyError("Missing entry for %s and %s %s" % (utt1, utt2, scores_filename))
        scores.append(float(score))
        labels.append(1 if kind[(utt1, utt2)] == "target" else 0)
    return np.asarray(scores, dtype=np.float64), np.asarray(labels, dtype=np.int32)


def main(argv=None, scoring=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    sys.stderr.write(" ".join([sys.argv[0]] + argv) + "\n")
    args = get_args(argv)
    scores, labels = read_scored_trials(args.scores_filename, args.trials_filename)
    if scoring is None:
        from libs.amd import scoring
    value, threshold = scoring.min_dcf(scores.astype(np.float32), labels, p_target=args.p_target, c_miss=args.c_miss, c_fa=args.c_fa)
    sys.stdout.write("%.4f\n" % value)
    sys.stderr.write("minDCF is %.4f at threshold %.4f (p-target=%s, c-miss=%s,c-fa=%s)\n" % (value, threshold, args.p_target, args.c_miss, args.c_fa))
    return 0


if __name__ == "__main__":
    sys.exit(main())
