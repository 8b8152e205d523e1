# -*- coding:utf-8 -*-
"""CORAL+ domain adaptation of a PLDA model on an MI355X - command-line compatible with the reference's
score/pyplda/ivector-adapt-plda-coralplus.py: out-of-domain PLDA statistics ark + unlabelled in-domain vectors -> Kaldi text
<Plda> (libs.amd.scoring.coral_plus, the reference's scales 0.8 / 0.8).

    python3 ivector-adapt-plda-coralplus.py [--gpu-id N] <plda> <adapt-ivector-rspecifier> <plda-adapt>
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
        out_model = scoring.PldaCovariances.read_stats_ark(args[0])
        scoring.coral_plus(out_model, common.read_vectors(args[1])).to_plda().write_kaldi_text(args[2])
    common.run(body)


if __name__ == "__main__":
    main()
