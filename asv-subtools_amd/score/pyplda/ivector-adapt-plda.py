# -*- coding:utf-8 -*-
"""Kaldi-style unsupervised PLDA adaptation (ivector-adapt-plda) on an MI355X - command-line compatible with the reference's
score/pyplda/ivector-adapt-plda.py (PldaUnsupervisedAdaptor, scales 1.0 / 0.3 / 0.7): PLDA statistics ark + unlabelled
in-domain vectors -> Kaldi text <Plda> (libs.amd.scoring.Plda.adapt_unsupervised).

    python3 ivector-adapt-plda.py [--gpu-id N] <plda> <adapt-ivector-rspecifier> <plda-adapt>
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import adapt_common as common  # noqa: E402

USAGE = "<plda> <adapt-ivector-rspecifier> <plda-adapt>"


def main():
    args, gpu_id = common.parse(sys.argv, USAGE, 3)

    def body():
        from libs.amd import scoring
        common.select_device(gpu_id)
        plda = scoring.Plda.read_stats_ark(args[0])
        plda.adapt_unsupervised(common.read_vectors(args[1])).write_kaldi_text(args[2])
    common.run(body)


if __name__ == "__main__":
    main()
