# -*- coding:utf-8 -*-
"""Data preparation on the device: what the reference's makeFeatures.sh (steps/make_{fbank,mfcc,plp,spectrogram}.sh -> compute-*-feats |
copy-feats --compress=true) and computeVad.sh (sid/compute_vad_decision.sh -> compute-vad) leave in a data directory, written from
wav.scp by the device front-end, the device compressor (asv_encode_compressed) and the device energy VAD.  The command lines are
asv-subtools_amd/makeFeatures.py and computeVad.py; this module holds their work so that it can be called (and tested) as functions.
"""

import importlib.util
import os
import struct
import sys
import warnings

import numpy as np

from . import frontend, kaldi_conf
from ..support import kaldi_io

FEATURE_TYPES = ("fbank", "mfcc", "plp", "spectrogram")


class Refused(ValueError):
    """A request this path does not serve; the message names the cause."""


def data_name(data_dir):
    """The reference's `name` of a data directory (makeFeatures.sh:45): its path components joined with '_'."""
    return "_".join(p for p in data_dir.replace("/", " ").split() if p)


def check_feature_type(feature_type):
    if feature_type not in FEATURE_TYPES:
        raise Refused("[exit] Invalid base feature type %s ,just fbank/mfcc/plp" % feature_type)      # (makeFeatures.sh:42)


def read_wav_scp(data_dir):
    """[(key, wav path)] of <data-dir>/wav.scp; refuses what this path does not read: a segments file, command entries."""
    if os.path.exists(os.path.join(data_dir, "segments")):
        raise Refused("%s has a segments file: features of segments of recordings are not offered on this path (extract-segments first)" % data_dir)
    items = []
    with open(os.path.join(data_dir, "wav.scp"), "r", encoding="utf8") as f:
        for no, line in enumerate(f, 1):
            line = line.strip()
            if not line:
                continue
            parts = line.split(None, 1)
            if len(parts) != 2:
                raise Refused("wav.scp line %d: expected 'utt-id path.wav', got %r" % (no, line))
            if parts[1].endswith("|"):
                raise Refused("wav.scp line %d (%s) is a command ending in '|': piped entries are not read on this path, write the audio to 16-bit PCM files" %
                              (no, parts[0]))
            items.append((parts[0], parts[1]))
    return items


def read_feature_config(path, feature_type):
    """The frontend keywords of <feature-config>: a Kaldi .conf (Kaldi's defaults for what it omits), or a .yaml in the online script's
    form {feature_type, kaldi_featset} (torchaudio's defaults, as there)."""
    if path.endswith((".yaml", ".yml")):
        import yaml
        with open(path, "r") as f:
            doc = yaml.load(f, Loader=yaml.FullLoader) or {}
        kind = doc.get("feature_type", feature_type)
        if kind != feature_type:
            raise Refused("%s says feature_type %s, the command line %s" % (path, kind, feature_type))
        opts = dict(doc.get("kaldi_featset", {}) or {})
        frontend.fbank_options(feature_type, **opts)                 # (refuses unknown keys and dither here, before any file is read)
        return opts
    return kaldi_conf.read_feature_conf(path, feature_type)


def _batches(items, sample_frequency, batch_seconds, batch_utts, num_readers):
    """(keys, packed int16 samples, sample offsets) per batch of at most batch_seconds of audio / batch_utts files, in order."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=max(1, num_readers)) as pool:
        take, total = [], 0.0
        step = max(8, num_readers * 4)
        for pos in range(0, len(items), step):
            group = items[pos:pos + step]
            for (key, path), (wav, sr) in zip(group, pool.map(lambda it: frontend.read_wav_pcm16(it[1]), group)):
                if float(sr) != float(sample_frequency):
                    raise Refused("%s (%s) is sampled at %d Hz, the feature config says sample_frequency %g: resample the file or change the config" %
                                  (key, path, sr, sample_frequency))
                seconds = len(wav) / float(sr)
                if take and (total + seconds > batch_seconds or len(take) >= batch_utts):
                    yield _pack(take)
                    take, total = [], 0.0
                take.append((key, wav))
                total += seconds
        if take:
            yield _pack(take)


def _pack(take):
    off = np.zeros(len(take) + 1, dtype=np.int64)
    np.cumsum([len(w) for _, w in take], out=off[1:])
    return [k for k, _ in take], np.concatenate([w for _, w in take]), off


def _vad_vectors(writer, keys, voiced, frame_off):
    """compute-vad's output: one float vector of 0 / 1 per utterance."""
    flags = voiced.cpu().numpy().astype(np.float32)
    for k, a, b in zip(keys, frame_off[:-1], frame_off[1:]):
        writer.write(k, b"\0BFV \4" + struct.pack("<I", int(b - a)), flags[int(a):int(b)].tobytes())


def make_features(data_dir, feature_type, feature_config, exp="exp/features", compress=True, write_utt2num_frames=True, vad_config=None, device=None,
                  batch_seconds=1200.0, batch_utts=512, num_readers=4):
    """wav.scp -> <exp>/<type>/<name>/raw_<type>_<name>.1.ark, <data-dir>/feats.scp (wav.scp order) and utt2num_frames; with vad_config
    also <exp>/vad/<name>/vad_<name>.1.ark and <data-dir>/vad.scp in the same pass, decided on the rows a reader of feats.scp gets (the
    decoded compressed ones).  Returns (utterances written, utterances skipped as shorter than one frame)."""
    import torch
    check_feature_type(feature_type)
    opts = read_feature_config(feature_config, feature_type)
    vad = kaldi_conf.read_vad_conf(vad_config) if vad_config else None
    items = read_wav_scp(data_dir)
    sample_frequency = opts.get("sample_frequency", 16000.0)
    name = data_name(data_dir)
    out_dir = os.path.join(exp, feature_type, name)
    os.makedirs(out_dir, exist_ok=True)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    n_done, n_skipped = 0, 0
    vad_writer = None
    u2n = open(os.path.join(data_dir, "utt2num_frames"), "w") if write_utt2num_frames else None
    feats_writer = kaldi_io.ArkScpWriter(os.path.join(out_dir, "raw_%s_%s.1.ark" % (feature_type, name)), os.path.join(data_dir, "feats.scp"))
    try:
        if vad is not None:
            os.makedirs(os.path.join(exp, "vad", name), exist_ok=True)
            vad_writer = kaldi_io.ArkScpWriter(os.path.join(exp, "vad", name, "vad_%s.1.ark" % name), os.path.join(data_dir, "vad.scp"))
        with torch.cuda.device(dev):
            for keys, samples, sample_off in _batches(items, sample_frequency, batch_seconds, batch_utts, num_readers):
                wave_dev = torch.from_numpy(samples).to(dev)
                feats, frame_off = frontend.fbank_device(wave_dev, sample_off, kind=feature_type, **opts)
                rows_of = np.diff(frame_off)
                for k in (k for k, r in zip(keys, rows_of) if r == 0):
                    warnings.warn("%s is shorter than one frame: no features, left out of feats.scp" % k)
                    n_skipped += 1
                keys = [k for k, r in zip(keys, rows_of) if r > 0]
                if not keys:
                    continue
                frame_off = np.concatenate([[0], np.cumsum(rows_of[rows_of > 0])]).astype(np.int64)      # (the others have no rows in feats)
                dim = int(feats.shape[1])
                rows = feats
                if compress:
                    body_bytes, byte_off, formats, status = frontend.encode_compressed(feats, frame_off)
                    if vad is not None:
                        rows = frontend.decode_compressed(body_bytes, byte_off, frame_off, formats, dim)
                    bad = np.flatnonzero(status.cpu().numpy())
                    if len(bad):
                        raise ValueError("the features of %s hold a NaN or an infinity: no compressed form (Kaldi asserts on such a matrix)" % keys[int(bad[0])])
                    host = body_bytes.cpu().numpy()
                    sizes = frontend.compressed_body_bytes(formats, np.diff(frame_off), dim)
                    for k, f, a, size in zip(keys, formats, byte_off, sizes):
                        feats_writer.write(k, b"\0B" + kaldi_io.COMPRESSED_TOKENS[int(f)], host[int(a):int(a) + int(size)].data)
                else:
                    host = feats.cpu().numpy()
                    for k, a, b in zip(keys, frame_off[:-1], frame_off[1:]):
                        feats_writer.write(k, kaldi_io.float_matrix_head(int(b - a), dim), host[int(a):int(b)].data)
                if vad is not None:
                    voiced, _ = frontend.vad_energy(rows, frame_off, **vad)
                    _vad_vectors(vad_writer, keys, voiced, frame_off)
                if u2n is not None:
                    u2n.write("".join("%s %d\n" % (k, r) for k, r in zip(keys, np.diff(frame_off))))
                n_done += len(keys)
    finally:
        feats_writer.close()
        if vad_writer is not None:
            vad_writer.close()
        if u2n is not None:
            u2n.close()
    return n_done, n_skipped


def _extract_script():
    """pipeline/onestep/extract_embeddings.py as a module: its scp loader is the one every reader of feats.scp here goes through."""
    name = "asv_amd_extract_embeddings"
    if name not in sys.modules:
        path = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "pipeline", "onestep", "extract_embeddings.py"))
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        sys.modules[name] = mod
    return sys.modules[name]


def compute_vad(data_dir, vad_config, exp="exp/features", device=None, batch_frames=1 << 18, batch_utts=1024):
    """<data-dir>/feats.scp -> <exp>/vad/<name>/vad_<name>.1.ark and <data-dir>/vad.scp: compute-vad's float vectors of 0 / 1, from the
    energy VAD on the device.  Compressed entries are read as they lie on disk and decoded on the device.  Returns the number written."""
    import torch
    vad = kaldi_conf.read_vad_conf(vad_config)
    ee = _extract_script()
    entries = ee.read_scp("scp:" + os.path.join(data_dir, "feats.scp"))
    name = data_name(data_dir)
    out_dir = os.path.join(exp, "vad", name)
    os.makedirs(out_dir, exist_ok=True)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    reader = ee.ScpGroupReader(entries)
    n_done = 0
    try:
        with kaldi_io.ArkScpWriter(os.path.join(out_dir, "vad_%s.1.ark" % name), os.path.join(data_dir, "vad.scp")) as w, torch.cuda.device(dev):
            dim = reader.peek_dim()
            if dim is None:
                return 0
            host_rows = np.empty((batch_frames, dim), dtype=np.float32)
            raw = np.empty(batch_frames * dim * 2 + 16 * (batch_utts + 2), dtype=np.uint8)
            byte_buffer = raw[(-raw.ctypes.data) % 16:][:len(raw) - 16]
            while True:
                keys, offs, frames = reader.read_group(host_rows, batch_utts, byte_buffer=byte_buffer)
                if not keys:
                    break
                frame_off = np.asarray(offs, dtype=np.int64)
                if isinstance(frames, ee.CompressedGroup):
                    rows = frontend.decode_compressed(torch.from_numpy(byte_buffer[:frames.used_bytes]).to(dev), frames.byte_off, frames.frame_off, frames.formats, dim)
                elif isinstance(frames, np.ndarray):
                    rows = torch.from_numpy(frames).to(dev)
                else:
                    rows = torch.from_numpy(host_rows[:frames]).to(dev)
                voiced, _ = frontend.vad_energy(rows, frame_off, **vad)
                _vad_vectors(w, keys, voiced, frame_off)
                n_done += len(keys)
    finally:
        reader.close()
    return n_done
