#!/usr/bin/env python3
# -*- coding:utf-8 -*-
"""Kaldi features of a data directory, computed and compressed on an MI355X - command-line compatible with the reference's
makeFeatures.sh (steps/make_{fbank,mfcc,plp,spectrogram}.sh: compute-*-feats | copy-feats --compress=true):

    makeFeatures.py [--pitch false] [--cmvn false] [--nj N] [--exp exp/features] [--use-gpu true] [--gpu-id N]
                    [--compress true] [--write-utt2num-frames true] [--vad-config FILE] <data-dir> <feature-type> <feature-config>

<feature-type>: fbank | mfcc | plp | spectrogram.  <feature-config>: a Kaldi .conf (`--num-mel-bins=80` lines; omitted keys take the
Kaldi binaries' defaults, libs/amd/kaldi_conf.py), or a .yaml in the form of the online extraction script.  Reads <data-dir>/wav.scp
(plain paths to 16-bit PCM files), writes <exp>/<type>/<name>/raw_<type>_<name>.1.ark, <data-dir>/feats.scp in wav.scp order and
<data-dir>/utt2num_frames; --vad-config FILE also writes <exp>/vad/<name>/vad_<name>.1.ark and <data-dir>/vad.scp in the same pass - the
decisions computeVad.py would take on that feats.scp afterwards.  The archive holds Kaldi's compressed matrices ('CM ' for more than 8
rows, else 'CM2'), produced on the device (asv_encode_compressed); --compress false writes float32 'FM ' matrices.  An utterance
shorter than one frame is skipped with a warning, as Kaldi does.

Refused, with a message: --pitch true (no pitch on this path), --cmvn true (per-speaker cmvn.scp is not what the extraction path
reads: it normalises with a sliding window), --use-gpu false, a `segments` file, wav.scp entries that are commands, files whose sample
rate is not the config's sample_frequency, dither.  --nj is accepted and ignored: one process feeds one device.
"""

import argparse
import os
import sys
import traceback

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "pytorch"))


def to_bool(text):
    if str(text).lower() not in ("true", "false"):
        raise argparse.ArgumentTypeError("true or false, not %r" % (text,))
    return str(text).lower() == "true"


def get_args(argv=None):
    p = argparse.ArgumentParser(description="Make Kaldi features of a data directory on the device.", allow_abbrev=False)
    p.add_argument("--pitch", type=to_bool, default=False)
    p.add_argument("--pitch-config", type=str, default="subtools/conf/pitch.conf")
    p.add_argument("--cmvn", type=to_bool, default=False)
    p.add_argument("--nj", type=int, default=20, help="accepted and ignored")
    p.add_argument("--exp", type=str, default="exp/features")
    p.add_argument("--use-gpu", type=to_bool, default=True)
    p.add_argument("--gpu-id", type=str, default="")
    p.add_argument("--compress", type=to_bool, default=True)
    p.add_argument("--write-utt2num-frames", type=to_bool, default=True)
    p.add_argument("--vad-config", type=str, default="")
    p.add_argument("--batch-seconds", type=float, default=1200.0, help="Upper bound of audio per batch.")
    p.add_argument("--batch-utts", type=int, default=512, help="Upper bound of utterances per batch.")
    p.add_argument("--num-readers", type=int, default=4, help="WAV reader threads.")
    p.add_argument("positional", nargs="*")
    return p.parse_args(argv)


def check_args(args):
    """The refusals that need neither a file nor a device."""
    from libs.amd import featprep
    if len(args.positional) != 3:
        raise featprep.Refused("[exit] Num of parameters is not equal to 3\nusage:makeFeatures.py [--pitch false|true] [--nj 20|int] <data-dir> <feature-type> <feature-config>\n"
                               "[note] Base <feature-type> could be fbank/mfcc/plp/spectrogram and the option --pitch defaults false")
    featprep.check_feature_type(args.positional[1])
    if args.pitch:
        raise featprep.Refused("--pitch true: Kaldi pitch features are not computed on this path")
    if args.cmvn:
        raise featprep.Refused("--cmvn true: per-speaker cmvn.scp is not what this extraction path reads (it applies a sliding-window CMN itself); "
                               "run Kaldi's compute_cmvn_stats.sh on the data directory if another tool needs it")
    if not args.use_gpu:
        raise featprep.Refused("--use-gpu false: asv-subtools_amd computes features on a ROCm device only; there is no CPU path")
    return args.positional


def main(argv=None):
    args = get_args(argv)
    try:
        from libs.amd import featprep
        data_dir, feature_type, config = check_args(args)
        import torch
        if args.gpu_id != "":
            torch.cuda.set_device(int(args.gpu_id))
        n, skipped = featprep.make_features(data_dir, feature_type, config, exp=args.exp, compress=args.compress,
                                            write_utt2num_frames=args.write_utt2num_frames, vad_config=args.vad_config or None,
                                            batch_seconds=args.batch_seconds, batch_utts=args.batch_utts, num_readers=args.num_readers)
        print("Make features done. (%d utterances%s)" % (n, ", %d shorter than one frame skipped" % skipped if skipped else ""))
        if args.vad_config:
            print("Compute VAD done.")
    except BaseException as e:
        if isinstance(e, ValueError) and type(e).__name__ == "Refused":
            print(str(e), file=sys.stderr)
        elif not isinstance(e, (KeyboardInterrupt, SystemExit)):
            traceback.print_exc()
        sys.exit(1)


if __name__ == "__main__":
    main()
