# -*- coding:utf-8 -*-
"""Waveform-in embedding extractor - the command line of the reference's online script
(/root/reference/pytorch/pipeline/onestep/extract_embeddings_online.py:26-66; called by
pipeline/extract_xvectors_for_pytorch_new.sh):

    extract_embeddings_online.py [--nnet-config CFG | --model-blueprint PY --model-creation CTOR]
                                 --data-type raw --feat-config feat.yaml [--max-chunk N]
                                 [--use-gpu true] [--gpu-id N] model-path wav.scp vectors-wspecifier

wav.scp holds "utt-id path.wav" lines (reference libs/support/utils.py:625-638); feat.yaml holds the reference's
feature_extraction_conf: {feature_type: fbank|mfcc|plp|spectrogram, kaldi_featset: {...torchaudio names...}, mean_var_conf: {...}}
(the four feature types of the reference's makeFeatures.sh; plp adds lpc_order / compress_factor / cepstral_scale).  The width the
options give must be the model's inputs_dim: anything else is a ValueError naming both numbers, before the first launch.

Where the reference decodes, computes torchaudio features, uploads and embeds one utterance at a time (lines 118-135),
this script ships 16-bit PCM (half the bytes of float features), and runs front-end + extractor on the device per batch:
    reader threads  wav files -> int16 samples packed in a pinned buffer
    device          H2D, (asv_desilence_pcm16,) asv_fbank_pcm16 (+ asv_cmvn), asv_net_extract, D2H
    writer          embeddings -> Kaldi vector ark (same bytes as kaldi_io.write_vec_flt per entry), input order
and prints "RTF:<device seconds per second of audio>" like the reference (line 138).

--de-silence true --amp-th N (what every "online" launcher of the reference passes) trims each waveform as the reference's
processor.py:149-175 de_sil -> signal_processing.py:13-55 de_silence does: blocks of int(0.1 * sample rate) samples whose mean
absolute amplitude is not above N (16-bit counts) are dropped, the rest concatenated; an utterance in which no block survives is
kept whole (processor.py:170-171).  The batch is trimmed on the device between the upload and the features (asv_desilence_pcm16,
sample for sample what libs.amd.frontend.de_silence_host gives); ASV_AMD_DEVICE_DESILENCE=0 trims in the reader threads on the
host instead.  Decided deviation: the threshold is N for EVERY utterance.  In the reference the retry of processor.py:166-169
never changes what an utterance yields (line 168 drops the retry's length, so line 171 puts the whole waveform back), but it
halves the generator-local threshold for every later utterance of the same DataLoader worker - a function of how utterances
are dealt to its 2 workers, which is not reproduced.  The RTF line counts the frames after trimming, as the reference's does.

Not offered: --data-type shard (tar shards of the training pipeline); --data-type kaldi never worked in the reference
(egs_online.py:258-259 uses an undefined dataset) and is rejected too.  WAV files must be 16-bit PCM; the first channel is
used (processor.py:138).
"""

import argparse
import os
import sys
import time
import traceback

sys.path.insert(0, "subtools/pytorch")
sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")))

import numpy as np
import torch
import yaml

import libs.support.kaldi_io as kaldi_io
import libs.support.utils as utils
from libs.amd import frontend


def get_args(argv=None):
    parser = argparse.ArgumentParser(description="Extract embeddings form a piece of feats.scp or pipeline")
    parser.add_argument("--nnet-config", type=str, default="", help="This config contains model_blueprint and model_creation.")
    parser.add_argument("--model-blueprint", type=str, default=None, help="A *.py which includes the instance of nnet in this training.")
    parser.add_argument("--model-creation", type=str, default=None, help="A command to create the model class, e.g. Xvector(40,2).")
    parser.add_argument("--data-type", type=str, default="raw", choices=["raw", "shard", "kaldi"], help="raw: wav.scp")
    parser.add_argument("--de-silence", type=str, default="false", choices=["true", "false"], help="Drop the silent 0.1 s blocks of every waveform (see --amp-th).")
    parser.add_argument("--amp-th", type=int, default=50, help="De_silence threshold (16bit)")
    parser.add_argument("--max-chunk", type=int, default=10000, help="Select chunk_size of features when extracting xvector")
    parser.add_argument("--feat-config", type=str, default="", help="The config yaml of feat extraction")
    parser.add_argument("--use-gpu", type=str, default="true", choices=["true", "false"], help="The MI355X path needs a GPU; 'false' is rejected.")
    parser.add_argument("--gpu-id", type=str, default="", help="Specify a fixed gpu, or select gpu automatically.")
    parser.add_argument("--batch-seconds", type=float, default=1200.0, help="Upper bound of audio per batch.")
    parser.add_argument("--batch-utts", type=int, default=512, help="Upper bound of utterances per batch.")
    parser.add_argument("--num-readers", type=int, default=4, help="WAV reader threads.")
    parser.add_argument("model_path", metavar="model-path", type=str, help="The model used to extract embeddings.")
    parser.add_argument("feats_rspecifier", metavar="feats-rspecifier", type=str, help="wav.scp")
    parser.add_argument("vectors_wspecifier", metavar="vectors-wspecifier", type=str, help="")
    return parser.parse_args(argv)


read_wav_pcm16 = frontend.read_wav_pcm16          # (shared with makeFeatures.py)


def check_args(args):
    """The refusals of the command line that need no device; returns the de-silence threshold (--amp-th) or None (--de-silence false)."""
    if not utils.to_bool(args.use_gpu):
        raise RuntimeError("asv-subtools_amd extracts on a ROCm device only (--use-gpu=true); there is no CPU path")
    if args.data_type != "raw":
        raise ValueError("Do not support datatype: {0} now.".format(args.data_type))
    if not utils.to_bool(args.de_silence):
        return None
    if args.amp_th < 0:
        raise ValueError("--amp-th must not be negative: {0}".format(args.amp_th))
    return args.amp_th


def device_desilence():
    """ASV_AMD_DEVICE_DESILENCE=0: --de-silence trims in the reader threads on the host (frontend.de_silence_host), not on the device."""
    return os.environ.get("ASV_AMD_DEVICE_DESILENCE", "1") != "0"


def check_feature_width(model, kind, featset, sample_frequency=None):
    """ValueError unless features of `kind` under `featset` are as wide as the model's input (no launch involved)."""
    from libs.amd import engine as amd_engine, ir
    kw = dict(featset) if sample_frequency is None else dict(featset, sample_frequency=float(sample_frequency))
    try:
        want = amd_engine.infer_feat_dim(model)
    except ir.TraceError:
        return                                                       # a model that does not say: the engine compares per batch
    width = frontend.feature_dim(kind, **kw)
    if width != want:
        raise ValueError("feat-config gives %s features of width %d, but the model's inputs_dim is %d" % (kind, width, want))


def extract_wavs(model, items, w, feat_conf, max_chunk, batch_seconds=1200.0, batch_utts=512, num_readers=4, amp_th=None):
    """items: [(key, wav path)].  amp_th: the de-silence threshold, None: no trimming.  Returns (number written, device seconds, audio
    seconds as frames * 0.01 like the reference)."""
    import queue
    import threading
    from concurrent.futures import ThreadPoolExecutor
    kind = feat_conf.get("feature_type", "mfcc")
    featset = dict(feat_conf.get("kaldi_featset", {}) or {})
    check_feature_width(model, kind, featset)                        # before the engine exists: nothing has touched the device yet
    engine = model._amd_engine()
    mv = feat_conf.get("mean_var_conf", {})
    mean_norm = bool(mv.get("mean_norm", True)) if mv is not None else False      # processor.py:410-413: {} -> defaults, None -> identity
    std_norm = bool(mv.get("std_norm", False)) if mv is not None else False
    dev = torch.device("cuda", engine.device_index)
    batches = queue.Queue(maxsize=2)
    trim_device = amp_th is not None and device_desilence()
    read = read_wav_pcm16
    if amp_th is not None and not trim_device:
        def read(path):
            wav, sr = read_wav_pcm16(path)
            return frontend.de_silence_host(wav, sr, min_eng=amp_th), sr

    free_bufs = queue.Queue()                    # two pinned staging buffers rotate between the producer and the consumer
    for _ in range(2):
        free_bufs.put(None)

    def produce():
        """Every file is read and decoded ONCE: decoded utterances that do not fit the audio budget of the batch being built
        stay in `pending` for the next one (the first version re-read the tail of every 512-file group 3-4 times)."""
        try:
            with ThreadPoolExecutor(max_workers=max(1, num_readers)) as pool:
                pending, pos = [], 0              # [(key, samples, rate)]
                while pos < len(items) or pending:
                    # decode ahead until the pending audio certainly fills one batch (or the list ends)
                    while pos < len(items) and (len(pending) < batch_utts and sum(len(wv) / float(sr) for _, wv, sr in pending) <= batch_seconds):
                        group = items[pos:pos + max(8, num_readers * 4)]
                        for (key, _), (wav, sr) in zip(group, pool.map(lambda it: read(it[1]), group)):
                            pending.append((key, wav, sr))
                        pos += len(group)
                    # cut at the audio budget / utterance cap (at least one utterance)
                    total, n = 0.0, 0
                    for _, wav, sr in pending[:batch_utts]:
                        if n > 0 and total + len(wav) / float(sr) > batch_seconds:
                            break
                        total += len(wav) / float(sr)
                        n += 1
                    take, pending = pending[:n], pending[n:]
                    rates = {sr for _, _, sr in take}
                    if len(rates) != 1:
                        raise ValueError("mixed sample rates in one batch: %s" % sorted(rates))
                    off = np.zeros(n + 1, dtype=np.int64)
                    np.cumsum([len(wav) for _, wav, _ in take], out=off[1:])
                    host = free_bufs.get()        # blocks until the consumer has uploaded the batch that used it
                    if host is None or host.numel() < int(off[-1]):
                        host = torch.empty(max(int(off[-1]), int(batch_seconds * 16000)), dtype=torch.int16).pin_memory()
                    hv = host.numpy()
                    for (_, wav, _), a, b in zip(take, off[:-1], off[1:]):
                        hv[a:b] = wav
                    batches.put(([k for k, _, _ in take], host, off, rates.pop()))
            batches.put(None)
        except BaseException as e:
            batches.put(e)

    t = threading.Thread(target=produce, daemon=True)
    t.start()
    n_done, dev_ms, audio_s = 0, 0.0, 0.0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.device(dev):
        while True:
            item = batches.get()
            if item is None:
                break
            if isinstance(item, BaseException):
                raise item
            keys, host, off, sr = item
            wave_dev = host[:int(off[-1])].to(dev, non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()             # the upload has read the pinned buffer: hand it back
            free_bufs.put(host)
            check_feature_width(model, kind, featset, sr)            # (the spectrogram's width follows the files' sample rate)
            e0.record()
            if trim_device:
                wave_dev, off = frontend.de_silence_device(wave_dev, off, sr, min_eng=amp_th)
            feats, frame_off = frontend.fbank_device(wave_dev, off, kind=kind, mean_norm=mean_norm, std_norm=std_norm,
                                                     **dict(featset, sample_frequency=float(sr)))    # processor.py:428
            keep = [i for i in range(len(keys)) if frame_off[i + 1] > frame_off[i]]
            if len(keep) != len(keys):
                for i in set(range(len(keys))) - set(keep):
                    print("Warning: {0} is shorter than one frame, skipped".format(keys[i]))
            emb = _extract_subset(engine, feats, frame_off, keep, max_chunk) if keep else None
            e1.record()
            if emb is not None:
                out = emb.cpu().numpy()
                e1.synchronize()
                dev_ms += e0.elapsed_time(e1)
                audio_s += float(frame_off[-1]) * 0.01
                w.write(kaldi_io.vec_flt_ark_bytes([keys[i] for i in keep], out))
                n_done += len(keep)
    t.join()
    return n_done, dev_ms * 1e-3, audio_s


def _extract_subset(engine, feats, frame_off, keep, max_chunk):
    """Utterances with at least one frame only (the others have no rows in `feats`, so the packed matrix is unchanged)."""
    lens = [int(frame_off[i + 1] - frame_off[i]) for i in keep]
    offs = np.zeros(len(keep) + 1, dtype=np.int32)
    np.cumsum(lens, out=offs[1:])
    return engine.extract_device_guarded(feats, offs, max_chunk=max_chunk)       # (synchronous loop: the range guard's wait costs nothing here)


def main(argv=None):
    print(" ".join(sys.argv))
    args = get_args(argv)
    try:
        if args.nnet_config != "":
            model_blueprint, model_creation = utils.read_nnet_config(args.nnet_config)
        elif args.model_blueprint is not None and args.model_creation is not None:
            model_blueprint, model_creation = args.model_blueprint, args.model_creation
        else:
            raise ValueError("Expected nnet_config or (model_blueprint, model_creation) to exist.")
        amp_th = check_args(args)
        with open(args.feat_config, "r") as fin:
            feat_conf = yaml.load(fin, Loader=yaml.FullLoader) or {}

        model = utils.create_model_from_py(model_blueprint, model_creation)
        model.load_state_dict(torch.load(args.model_path, map_location="cpu"), strict=False)
        model = utils.select_model_device(model, args.use_gpu, gpu_id=args.gpu_id)
        model.eval()
        items = []
        with open(args.feats_rspecifier, "r", encoding="utf8") as fin:
            for line in fin:
                arr = line.strip().split()
                if not arr:
                    continue
                assert len(arr) == 2, "wav.scp lines are 'utt-id path.wav' (pipes are not supported): %r" % line
                items.append((arr[0], arr[1]))
        t0 = time.perf_counter()
        with kaldi_io.open_or_fd(args.vectors_wspecifier, "wb") as w:
            n_done, dev_s, audio_s = extract_wavs(model, items, w, feat_conf, args.max_chunk, args.batch_seconds, args.batch_utts, args.num_readers, amp_th=amp_th)
        loop_s = time.perf_counter() - t0
        if os.environ.get("ASV_AMD_REPORT_TIMING", "0") not in ("0", "", "false"):
            # the read -> device -> write loop alone (model load and start-up excluded), and the device clock the RTF line divides
            print("Loop: {0} utterances in {1:.4f} s = {2:.1f} utterances/s, device {3:.4f} s, {4:.2f} s of audio".format(
                n_done, loop_s, n_done / loop_s if loop_s > 0 else 0.0, dev_s, audio_s))
        print("Extracted {0} embeddings.".format(n_done))
        print("RTF:{:.7f}".format(dev_s / audio_s if audio_s > 0 else 0.0))
    except BaseException as e:
        if not isinstance(e, KeyboardInterrupt):
            traceback.print_exc()
        sys.exit(1)


if __name__ == "__main__":
    main()
