#!/usr/bin/env python3
# -*- coding:utf-8 -*-
"""Energy VAD decisions of a data directory on an MI355X - command-line compatible with the reference's computeVad.sh
(sid/compute_vad_decision.sh: compute-vad scp:feats.scp ark,scp:vad.ark,vad.scp):

    computeVad.py [--nj N] [--exp exp/features] [--gpu-id N] <data-dir> <vad-config>

Reads <data-dir>/feats.scp (compressed entries are read as they lie on disk and decoded on the device), writes
<exp>/vad/<name>/vad_<name>.1.ark and <data-dir>/vad.scp: one float vector of 0 / 1 per utterance, as compute-vad writes.
<vad-config> is a Kaldi .conf with --vad-energy-threshold, --vad-energy-mean-scale, --vad-frames-context, --vad-proportion-threshold;
omitted keys take compute-vad's defaults 5.0, 0.5, 0, 0.6.  --nj is accepted and ignored.
"""

import argparse
import os
import sys
import traceback

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "pytorch"))


def get_args(argv=None):
    p = argparse.ArgumentParser(description="Compute energy VAD decisions of a data directory on the device.", allow_abbrev=False)
    p.add_argument("--nj", type=int, default=20, help="accepted and ignored")
    p.add_argument("--exp", type=str, default="exp/features")
    p.add_argument("--gpu-id", type=str, default="")
    p.add_argument("positional", nargs="*")
    return p.parse_args(argv)


def main(argv=None):
    args = get_args(argv)
    try:
        from libs.amd import featprep
        if len(args.positional) != 2:
            raise featprep.Refused("[exit] Num of parameters is not equal to 2\nusage:computeVad.py <data-dir> <vad-config>")
        data_dir, config = args.positional
        import torch
        if args.gpu_id != "":
            torch.cuda.set_device(int(args.gpu_id))
        featprep.compute_vad(data_dir, config, exp=args.exp)
        print("Compute VAD done.")
    except BaseException as e:
        if isinstance(e, ValueError) and type(e).__name__ == "Refused":
            print(str(e), file=sys.stderr)
        elif not isinstance(e, (KeyboardInterrupt, SystemExit)):
            traceback.print_exc()
        sys.exit(1)


if __name__ == "__main__":
    main()
