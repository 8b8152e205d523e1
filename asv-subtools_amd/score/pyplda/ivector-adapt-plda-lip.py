# -*- coding:utf-8 -*-
"""LIP (linear interpolation of two PLDA models) - command-line compatible with the reference's
score/pyplda/ivector-adapt-plda-lip.py: out-of-domain + in-domain PLDA statistics arks -> Kaldi text <Plda>
(libs.amd.scoring.lip, weight 0.4).  D x D host algebra only: --gpu-id is accepted for symmetry and not used.

    python3 ivector-adapt-plda-lip.py [--gpu-id N] <plda-out-domain> <plda-in-domain> <plda-adapt>
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import adapt_common as common  # noqa: E402

USAGE = "<plda-out-domain> <plda-in-domain> <plda-adapt>"


def main():
    args, gpu_id = common.parse(sys.argv, USAGE, 3)

    def body():
        from libs.amd import scoring
        out_model = scoring.PldaCovariances.read_stats_ark(args[0])
        in_model = scoring.PldaCovariances.read_stats_ark(args[1])
        scoring.lip(out_model, in_model).to_plda().write_kaldi_text(args[2])
    common.run(body)


if __name__ == "__main__":
    main()
