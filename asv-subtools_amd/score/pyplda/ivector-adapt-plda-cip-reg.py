# -*- coding:utf-8 -*-
"""CIP-reg (CORAL + regularised interpolation) domain adaptation of a PLDA model on an MI355X - command-line compatible with
the reference's score/pyplda/ivector-adapt-plda-cip-reg.py: out-of-domain PLDA statistics ark + unlabelled in-domain vectors +
in-domain PLDA statistics ark -> Kaldi text <Plda> (libs.amd.scoring.cip_reg, weight 0.5).

    python3 ivector-adapt-plda-cip-reg.py [--gpu-id N] <plda-out-domain> <adapt-ivector-rspecifier> <plda-in-domain> <plda-adapt>
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import adapt_common as common  # noqa: E402

USAGE = "<plda-out-domain> <adapt-ivector-rspecifier> <plda-in-domain> <plda-adapt>"


def main():
    args, gpu_id = common.parse(sys.argv, USAGE, 4)

    def body():
        from libs.amd import scoring
        common.select_device(gpu_id)
        out_model = scoring.PldaCovariances.read_stats_ark(args[0])
        in_model = scoring.PldaCovariances.read_stats_ark(args[2])
        scoring.cip_reg(out_model, common.read_vectors(args[1]), in_model).to_plda().write_kaldi_text(args[3])
    common.run(body)


if __name__ == "__main__":
    main()
