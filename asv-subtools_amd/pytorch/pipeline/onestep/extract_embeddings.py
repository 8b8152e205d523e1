# -*- coding:utf-8 -*-
"""Offline embedding extractor - same command line as the reference script
(/root/reference/pytorch/pipeline/onestep/extract_embeddings.py:17-45), so
`pipeline/extract_xvectors_for_pytorch.sh` can call it unchanged:

    extract_embeddings.py [--nnet-config CFG | --model-blueprint PY --model-creation CTOR]
                          [--use-gpu true] [--gpu-id N] model-path feats-rspecifier vectors-wspecifier

Differences are internal: features are read in bulk and embedded in packed ragged batches by
libasv_amd.so instead of one `model.extract_embedding()` call, one H2D copy, ~15 launches and one
blocking D2H per utterance (reference lines 73-83).  Output order and bytes per entry are the same
(`key SP \\0B FV \\4 dim data`).  Any error prints a traceback and exits 1 (reference 85-88) - the
calling shell script greps the log for "Error".

Extra options: --batch-frames / --batch-utts bound a batch; --verbose true restores the reference's
per-utterance "Process utterance for key ..." line (a measurable cost at >100k utterances/s).

Raw features: the reference's shell script puts `apply-cmvn-sliding ... scp:feats.scp ark:- | select-voiced-frames ark:-
scp,s,cs:vad.scp ark:- |` in front of this script (pipeline/extract_xvectors_for_pytorch.sh:105-118).  --cmn-window N
[--cmn-center true|false --cmn-norm-vars true|false --cmn-min-window N] and --vad-scp vad.scp do both on the device, in one
launch per batch between the H2D copy and the extraction (libs.amd.pipeline.DeviceSets, asv_ingest_frames), so the
feats-rspecifier can be the raw `scp:feats.scp`.  As select-voiced-frames does, an utterance without a VAD entry, with a VAD
vector of another length than its matrix, or without a voiced frame is skipped with a WARNING line on stderr.

Compressed features: Kaldi's make_fbank.sh / make_mfcc.sh write feats.scp as compressed matrices by default (`\0BCM `; also `CM2`, `CM3`).  With `scp:`
input (not --sharded) the bodies of such 'file:offset' entries are read as they lie on disk - one byte per value - and decoded on the device
(asv_decode_compressed) in front of the ingest / the extraction: the same float32 rows, bit for bit, as the host reader's.  Range-specified entries,
pipes, text and float64 matrices go through the host reader as before; ASV_AMD_DEVICE_DECODE=0 sends everything there.

Sliding (diarisation) mode: `--sliding true --segments data/segments [--window 1.5 --period 0.75 --min-segment 0.5 --hard-min false
--frame-shift 0.01 --subsegments-out subsegments]` is the `sliding=true` branch of the reference's shell script
(pipeline/extract_xvectors_for_pytorch.sh:57-84): every segment is cut into uniform overlapping sub-segments
(libs.amd.subsegments, the rules of kaldi/utils/data/get_uniform_subsegments.py and subsegment_data_dir.sh) and one vector per
sub-segment is written under the sub-segment's id.  The reference reads each sub-segment as a range 'file:offset[first:last]' of its
parent - the whole parent per window; here a parent is read and uploaded once per batch and the windows are built on the device
(asv_ingest_windows), --cmn-window applying per window as it does in the reference's pipe.  `scp:` input only, no --vad-scp (the
reference replaces the VAD by all ones in this mode), not with --sharded.

Multi-GPU (--sharded true, launched as `python -m torch.distributed.run --nproc-per-node N ... extract_embeddings.py ...`, one
process per GPU): replaces the reference's `nj` jobs over a length-balanced split of feats.scp and the final
`cat xvector.JOB.scp` (pipeline/extract_xvectors_for_pytorch.sh:90-100,125-151; splitDataByLength.sh:44-80).  Every rank reads
the scp (feats-rspecifier must be `scp:...`; lengths from --utt2num-frames or from the matrix headers), takes its shard of
libs.amd.shard.balance_by_length, extracts it, ONE all-gather (RCCL over xGMI) collects the embeddings and rank 0 writes the
vectors in scp order.
"""

import argparse
import collections
import os
import re
import sys
import time
import traceback

sys.path.insert(0, "subtools/pytorch")
sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")))

import numpy as np
import torch

import libs.support.kaldi_io as kaldi_io
import libs.support.utils as utils


def get_args(argv=None):
    parser = argparse.ArgumentParser(description="Extract embeddings form a piece of feats.scp or pipeline")
    parser.add_argument("--nnet-config", type=str, default="", help="This config contains model_blueprint and model_creation.")
    parser.add_argument("--model-blueprint", type=str, default=None, help="A *.py which includes the instance of nnet in this training.")
    parser.add_argument("--model-creation", type=str, default=None, help="A command to create the model class, e.g. Xvector(40,2).")
    parser.add_argument("--use-gpu", type=str, default="true", choices=["true", "false"], help="The MI355X path needs a GPU; 'false' is rejected.")
    parser.add_argument("--gpu-id", type=str, default="", help="Specify a fixed gpu, or select gpu automatically.")
    parser.add_argument("--batch-frames", type=int, default=65536, help="Upper bound of frames per packed batch.")
    parser.add_argument("--batch-utts", type=int, default=1024, help="Upper bound of utterances per packed batch.")
    parser.add_argument("--max-chunk", type=int, default=0, help="Override the model's maxChunk (0 = the decorator's value).")
    parser.add_argument("--verbose", type=str, default="false", choices=["true", "false"])
    parser.add_argument("--sharded", type=str, default="false", choices=["true", "false"],
                        help="One process per GPU under torch.distributed.run: shard the scp by length, all-gather, rank 0 writes.")
    parser.add_argument("--utt2num-frames", type=str, default="", help="Kaldi utt2num_frames of the scp (sharded mode; default: read the matrix headers).")
    parser.add_argument("--cmn-window", type=int, default=0, help="Sliding-window CMN on the device (apply-cmvn-sliding --cmn-window); 0 = off.")
    parser.add_argument("--cmn-center", type=str, default="true", choices=["true", "false"], help="apply-cmvn-sliding --center.")
    parser.add_argument("--cmn-norm-vars", type=str, default="false", choices=["true", "false"], help="apply-cmvn-sliding --norm-vars.")
    parser.add_argument("--cmn-min-window", type=int, default=100, help="apply-cmvn-sliding --min-cmn-window; only read when not centred.")
    parser.add_argument("--vad-scp", type=str, default="", help="Kaldi scp of per-frame VAD vectors: select-voiced-frames on the device.")
    parser.add_argument("--sliding", type=str, default="false", choices=["true", "false"],
                        help="Diarisation mode of the reference's extract_xvectors_for_pytorch.sh: one vector per uniform sub-segment of every segment.")
    parser.add_argument("--segments", type=str, default="", help="Kaldi segments file of the data directory (sliding mode); its first field is a key of the scp.")
    parser.add_argument("--window", type=float, default=1.5, help="Sub-segment length in seconds (sliding mode).")
    parser.add_argument("--period", type=float, default=0.75, help="Sub-segment shift in seconds (sliding mode).")
    parser.add_argument("--min-segment", type=float, default=0.5, help="Shortest remainder that becomes a sub-segment of its own (sliding mode).")
    parser.add_argument("--hard-min", type=str, default="false", choices=["true", "false"], help="Drop segments shorter than --min-segment first (sliding mode).")
    parser.add_argument("--frame-shift", type=float, default=0.01, help="Seconds per feature row (sliding mode).")
    parser.add_argument("--subsegments-out", type=str, default="", help="Write the sub-segments here: '<new-utt> <utt> <start> <end>' (sliding mode).")
    parser.add_argument("model_path", metavar="model-path", type=str, help="The model used to extract embeddings.")
    parser.add_argument("feats_rspecifier", metavar="feats-rspecifier", type=str, help="")
    parser.add_argument("vectors_wspecifier", metavar="vectors-wspecifier", type=str, help="")
    return parser.parse_args(argv)


def ingest_options(args):
    """libs.amd.pipeline.IngestOptions of the command line, or None when the features are read as they are."""
    from libs.amd.pipeline import IngestOptions
    if args.vad_scp and utils.to_bool(args.sharded):
        raise ValueError("--sharded true does not take --vad-scp: balancing the shards by voiced counts and dropping entries from the gather "
                         "are not built; run without --sharded, or select the voiced frames beforehand")
    if args.cmn_window < 0:
        raise ValueError("--cmn-window %d: pass a window length in frames, or 0 for none" % args.cmn_window)
    center = utils.to_bool(args.cmn_center)
    if args.cmn_window > 0 and not center and not 0 < args.cmn_min_window <= args.cmn_window:
        raise ValueError("--cmn-center false needs 0 < --cmn-min-window <= --cmn-window (got %d, %d)" % (args.cmn_min_window, args.cmn_window))
    if args.cmn_window == 0 and not args.vad_scp:
        return None
    return IngestOptions(args.cmn_window, args.cmn_min_window, center, utils.to_bool(args.cmn_norm_vars), bool(args.vad_scp))


SlidingOptions = collections.namedtuple("SlidingOptions", "segments window period min_segment hard_min frame_shift subsegments_out")


def sliding_options(args):
    """The sliding (diarisation) mode of the command line, or None.  What the mode does not take is refused here, before anything is
    set up: each would be a change of its own."""
    if not utils.to_bool(args.sliding):
        return None
    if utils.to_bool(args.sharded):
        raise ValueError("--sliding true does not take --sharded true: sharding the windows of a parent over ranks (and uploading it on each) is not built")
    if args.vad_scp:
        raise ValueError("--sliding true does not take --vad-scp: the reference replaces the VAD by all ones in this mode (createVisualVad.sh)")
    if not _SCP_PREFIX.match(args.feats_rspecifier):
        raise ValueError("--sliding true needs random access to the parents' rows: pass 'scp:feats.scp', not %r" % args.feats_rspecifier)
    if not args.segments:
        raise ValueError("--sliding true needs --segments: the Kaldi segments file whose segments are cut into windows")
    if not (args.window > 0 and 0 < args.period and args.min_segment >= 0 and args.frame_shift > 0):
        raise ValueError("--sliding true needs positive --window, --period and --frame-shift (got %r, %r, %r)" % (args.window, args.period, args.frame_shift))
    return SlidingOptions(args.segments, args.window, args.period, args.min_segment, utils.to_bool(args.hard_min), args.frame_shift, args.subsegments_out)


def refuse_ranged_entries(entries):
    """Sliding mode addresses the rows of a parent by the windows' own ranges: a source entry that carries one already is refused
    (the reference would go through normalize_data_range.pl)."""
    for key, rxfile in entries:
        if _RANGE.search(rxfile):
            raise ValueError("--sliding true: scp entry %r carries a range specifier (%s): windows of ranges are not built" % (key, rxfile))


class VadTable(object):
    """The per-frame VAD vectors of a Kaldi scp (`vad.scp`, written by compute-vad-decision), looked up by utterance key: the second
    input of select-voiced-frames.  flags_for() fills the uint8 flag buffer of one batch and applies that program's rules: a frame is
    kept when its flag is non-zero; a flag that is neither 0 nor 1 is an error (Kaldi asserts it); an utterance with no entry, with a
    vector of another length than its matrix has rows, or without a voiced frame is skipped with one WARNING line on stderr.
    The scp is parsed once.  A plain binary float vector entry 'file.ark:offset' is `\0B FV \4 <int32 dim>` + 4 * dim bytes, and dim has
    to equal the matrix's row count, which is known: the header and the 4 * T payload bytes of every entry of a batch are read in one
    call into libasv_io.so (native threads, the GIL released), the payload straight into the batch's float buffer.  Everything else - text, double vectors, pipes, a read that runs into
    the end of the file - goes through kaldi_io.read_vec_flt."""

    def __init__(self, path, threads=4, warn=None):
        from libs.support import native_io
        self.entries = read_scp(path)
        self.threads = max(1, int(threads))
        self.skipped = 0
        self._warn = warn if warn is not None else (lambda line: print(line, file=sys.stderr))
        self._fds = {}
        self._lut = None                                   # descriptor per path, once all are open
        n = len(self.entries)
        keys = self.entries.keys() if hasattr(self.entries, "plain_index") else [k for k, _ in self.entries]
        self.index = {k: i for i, k in enumerate(keys)}
        self._file = np.full(n, -1, dtype=np.int64)        # entry -> index into self._paths of a plain 'file:offset' entry, or -1
        self._offset = np.zeros(n, dtype=np.int64)
        self._paths = []
        if native_io.lib() is None:
            return
        if hasattr(self.entries, "plain_index"):
            pid, poff, paths = self.entries.plain_index()
            remap = np.full(len(paths) + 1, -1, dtype=np.int64)
            for j, name in enumerate(paths):
                if os.path.isfile(name):
                    remap[j] = len(self._paths)
                    self._paths.append(name)
            self._file[:] = remap[np.asarray(pid[:n])]
            self._offset[:] = np.where(self._file >= 0, np.asarray(poff[:n]), 0)
        else:
            ids = {}
            for i, (_, rx) in enumerate(self.entries):
                name, sep, o = rx.rpartition(":")
                if sep and o.isdigit():
                    if name not in ids:
                        ids[name] = len(self._paths) if os.path.isfile(name) else -1
                        if ids[name] >= 0:
                            self._paths.append(name)
                    self._file[i], self._offset[i] = ids[name], int(o)

    def close(self):
        for fd in self._fds.values():
            os.close(fd)
        self._fds.clear()

    def _descriptors(self):
        if self._lut is None:
            for j, name in enumerate(self._paths):
                self._fds[j] = os.open(name, os.O_RDONLY)
            self._lut = np.asarray([self._fds[j] for j in range(len(self._paths))], dtype=np.int32)
        return self._lut

    def flags_for(self, keys, offsets, flags):
        """flags[offsets[i]:offsets[i + 1]] = the 0 / 1 flags of utterance keys[i] (zeros for a skipped one), for every i.
        Returns (the keys that keep at least one frame, kept_off int64 [n + 1]: running sum of the kept frames per utterance)."""
        from libs.amd.frontend import kept_offsets
        from libs.support import native_io
        n = len(keys)
        off = np.asarray(offsets, dtype=np.int64)
        rows = np.diff(off)
        total = int(off[-1])
        flags[:total] = 0
        entry = np.asarray([self.index.get(key, -1) for key in keys], dtype=np.int64)
        cause = [None] * n                                   # why an utterance is skipped
        for i in np.flatnonzero(entry < 0):
            cause[i] = "no VAD entry"
        have = entry >= 0
        fast = np.flatnonzero(have & (self._file[np.where(have, entry, 0)] >= 0)) if len(self._paths) else np.zeros(0, dtype=np.int64)
        handled = np.zeros(n, dtype=bool)                    # read (or refused for its length) by the batched reads below
        if len(fast):
            # ONE native call, two positioned reads per entry: its 10 header bytes into head[j], its 4 T payload bytes straight to
            # values[off[i]:off[i + 1]] - frame g of the batch is values[g]
            head = np.zeros((len(fast), 16), dtype=np.uint8)
            values = np.zeros(total, dtype=np.float32)
            e = entry[fast]
            fds, pos = self._descriptors()[self._file[e]], self._offset[e]
            some = rows[fast] > 0
            try:
                native_io.pread_batch(np.concatenate((fds, fds[some])), np.concatenate((pos, pos[some] + 10)),
                                      np.concatenate((np.full(len(fast), 10, dtype=np.int64), 4 * rows[fast][some])), 0,
                                      np.concatenate((head.ctypes.data + 16 * np.arange(len(fast), dtype=np.int64), values.ctypes.data + 4 * off[fast][some])),
                                      threads=self.threads)
            except OSError:
                # a read ran into the end of its file (a vector shorter than its matrix, last in its archive): nothing of this call
                # is used, every entry of the group goes through read_vec_flt below, which names the short one
                fast = fast[:0]
        if len(fast):
            binary = (head[:, 0] == 0) & (head[:, 1] == ord("B")) & (head[:, 2] == ord("F")) & (head[:, 3] == ord("V")) & (head[:, 4] == ord(" ")) & (head[:, 5] == 4)
            dims = np.ascontiguousarray(head[:, 6:10]).view("<i4").ravel()
            fits = binary & (dims == rows[fast])
            for i, d in zip(fast[binary & ~fits].tolist(), dims[binary & ~fits].tolist()):
                cause[i] = "its VAD vector has %d entries, its feature matrix %d rows" % (d, rows[i])
            handled[fast[binary]] = True                     # (not a plain binary float vector: read_vec_flt below)
            good = np.zeros(n, dtype=bool)
            good[fast[fits]] = True
            if not good.all():
                values[~np.repeat(good, rows)] = 0.0         # what was read for the others is not a flag vector of this length
            voiced = values != 0.0
            bad = voiced & (values != 1.0)
            if bad.any():
                g = int(np.flatnonzero(bad)[0])
                i = int(np.searchsorted(off, g, side="right")) - 1
                raise ValueError("the VAD vector of %s holds %r at frame %d: select-voiced-frames takes 0 or 1 only" % (keys[i], float(values[g]), g - int(off[i])))
            flags[:total] = voiced
        slow = np.flatnonzero(have & ~handled)
        for i in slow.tolist():
            v = np.asarray(kaldi_io.read_vec_flt(self.entries[int(entry[i])][1]))
            if v.shape[0] != rows[i]:
                cause[i] = "its VAD vector has %d entries, its feature matrix %d rows" % (v.shape[0], rows[i])
                continue
            if ((v != 0.0) & (v != 1.0)).any():
                g = int(np.flatnonzero((v != 0.0) & (v != 1.0))[0])
                raise ValueError("the VAD vector of %s holds %r at frame %d: select-voiced-frames takes 0 or 1 only" % (keys[i], float(v[g]), g))
            flags[int(off[i]):int(off[i + 1])] = v != 0.0
        counts, kept_off = kept_offsets(flags, off)
        empty = np.flatnonzero(counts == 0)
        if len(empty) == 0:
            return list(keys), kept_off
        for i in empty.tolist():
            self.skipped += 1
            self._warn("WARNING: skipping utterance %s: %s" % (keys[i], cause[i] if cause[i] is not None else "no voiced frame"))
        drop = set(empty.tolist())
        return [key for i, key in enumerate(keys) if i not in drop], kept_off


def extract_stream(model, r, w, batch_frames, batch_utts, max_chunk, verbose=False, reader=None, ingest=None, vad=None):
    """feature ark stream -> embedding ark stream, pipelined in three stages over two buffer sets:
      reader thread   next packed batch -> pinned host buffer (the bodies of compressed scp entries: as they are -> pinned byte buffer)   (kaldi_io.IndexedArkReader for ark files - native index + batched reads -,
                      kaldi_io.PackedArkReader for pipes: block reads, no per-utterance arrays; ScpGroupReader for `scp:` input)
      device          async H2D, asv_net_extract, async D2H into a pinned result buffer + the range status word   (libs.amd.pipeline.DeviceSets:
                      each buffer set has its own engine - same weights, own activation arena - on its own HIP stream)
      writer          previous batch's vectors -> one write() of the assembled ark bytes
    so reading batch i+1 and writing batch i-1 overlap the device work of batch i.  Output order = input order.
    A batch whose activations left the range of the default mode's operand split is re-run with bf16 halves before it is written
    (DeviceSets.finish; the reference's f32 forward has no such limit).
    `ingest` (IngestOptions): the input is RAW features - sliding CMN and, with `vad` (a VadTable), voiced-frame selection run on the
    device in front of the extraction; a second reader stage (its own thread, so that the VAD reads of group i overlap the matrix reads of
    group i + 1) fetches a group's VAD vectors into the set's page-locked flag buffer.  Vectors are written for the utterances that keep
    at least one frame."""
    import queue
    import threading
    from libs.amd.pipeline import DeviceSets
    method = type(model).extract_embedding
    if max_chunk is None:
        max_chunk = getattr(method, "max_chunk", 10000)
    if reader is None:
        # an ark FILE of plain float32 matrices: native header index + one batched positioned read per group (libasv_io.so: 240 k
        # utterances/s from the page cache against 58 k for the sequential parser); pipes, stdin, other matrix kinds: the sequential reader
        reader = kaldi_io.IndexedArkReader.open(r, threads=_reader_threads()) if os.environ.get("ASV_AMD_INDEXED_READER", "1") != "0" else None
        if reader is None:
            reader = kaldi_io.PackedArkReader(r)
    dim = reader.peek_dim()
    if dim is None:
        return 0
    # the device lays a batch out with kHalo = 4 zero rows in front of, between and behind the utterances and works in tiles of 64 /
    # 128 / 256 rows: a group is cut so that its ROWS fit --batch-frames (65 536 = 256 tiles of 256 rows: 321 utterances of 200 frames
    # fill whole rounds of tiles on the 256 CUs; 327 - the frames alone - were 2.04 rounds of 128-row tiles, i.e. three)
    reader.row_pad = 4
    # Kaldi's feature scripts write COMPRESSED matrices by default: where the scp table holds such entries their bodies are read as they
    # lie on disk into a page-locked byte buffer and decoded on the device (a quarter of the bytes read and copied, no numpy decode per
    # utterance); ASV_AMD_DEVICE_DECODE=0 keeps the host decode (A/B runs, escape hatch)
    compressed = os.environ.get("ASV_AMD_DEVICE_DECODE", "1") != "0" and hasattr(reader, "has_compressed") and reader.has_compressed()
    sets = DeviceSets(model, batch_frames, batch_utts, dim, max_chunk, n_sets=3, results="host", ingest=ingest, compressed=compressed)
    free_sets, batches = queue.Queue(), queue.Queue()
    for k in range(sets.n_sets):
        free_sets.put(k)

    def produce():
        try:
            while True:
                k = free_sets.get()
                if compressed:
                    keys, offsets, frames = reader.read_group(sets.host_buffer(k), batch_utts, byte_buffer=sets.byte_buffer(k))
                else:
                    keys, offsets, frames = reader.read_group(sets.host_buffer(k), batch_utts)
                staged.put((k, keys, offsets, frames, None))
                if not keys:
                    return
        except BaseException as e:                    # surfaces in the consumer
            staged.put(e)

    def attach_flags():
        # second stage of the reader (its own thread: the VAD reads of group i overlap the matrix reads of group i + 1)
        try:
            while True:
                item = staged.get()
                if isinstance(item, BaseException):
                    batches.put(item)
                    return
                k, keys, offsets, frames, _ = item
                voiced = None
                if keys:
                    a = clock()
                    rows = frames.frames if isinstance(frames, CompressedGroup) else frames
                    flags = np.zeros(rows.shape[0], dtype=np.uint8) if isinstance(rows, np.ndarray) else sets.flag_buffer(k)[:rows]
                    voiced = (flags,) + vad.flags_for(keys, offsets, flags)
                    spent["vad"] += clock() - a
                batches.put((k, keys, offsets, frames, voiced))
                if not keys:
                    return
        except BaseException as e:
            batches.put(e)

    clock = time.perf_counter
    spent = {"reader": 0.0, "submit": 0.0, "device": 0.0, "write": 0.0}       # where the consumer thread's time goes (ASV_AMD_REPORT_TIMING)
    staged = batches
    if vad is not None:
        spent["vad"] = 0.0                                                    # ... and what the VAD reads take on their own thread
        staged = queue.Queue()
        threading.Thread(target=attach_flags, daemon=True).start()
    t = threading.Thread(target=produce, daemon=True)
    t.start()
    n_done, in_flight = 0, None

    def finish(item):
        k, keys = item
        a = clock()
        vectors = sets.finish(k)                      # waits for the batch; range guard (re-run on the bf16-halves twin if flagged)
        b = clock()
        if vectors is None:                           # no utterance of the batch kept a frame: nothing was submitted
            free_sets.put(k)
            return 0
        if verbose:
            for key in keys:
                print("Process utterance for key {0}".format(key))
        w.write(kaldi_io.vec_flt_ark_bytes(keys, vectors))
        free_sets.put(k)
        spent["device"] += b - a
        spent["write"] += clock() - b
        return len(keys)

    t0 = clock()
    while True:
        a = clock()
        item = batches.get()
        b = clock()
        spent["reader"] += b - a
        if isinstance(item, BaseException):
            raise item
        k, keys, offsets, frames, voiced = item
        if not keys:
            break
        flags = kept_off = None
        if voiced is not None:
            flags, keys, kept_off = voiced            # (the keys that keep a frame: one vector each)
        if isinstance(frames, CompressedGroup):       # compressed bodies in the set's byte buffer: decoded on the device
            sets.submit_compressed(k, frames.byte_off, frames.frame_off, frames.formats, frames.used_bytes, voiced=flags, kept_off=kept_off)
        elif voiced is not None:
            sets.submit(k, offsets, frames, voiced=flags, kept_off=kept_off)
        else:
            sets.submit(k, offsets, frames)
        spent["submit"] += clock() - b
        if in_flight is not None:
            n_done += finish(in_flight)
        in_flight = (k, keys)
    if in_flight is not None:
        n_done += finish(in_flight)
    t.join()
    _report_loop("stream", n_done, clock() - t0, sets, spent)
    return n_done


def _reader_threads():
    """Native reader threads per process: ASV_AMD_READER_THREADS, else 8 for one or two ranks on the host and 4 from three ranks on
    (WORLD_SIZE / LOCAL_WORLD_SIZE), at most the cores this process may run on.  Positioned reads from the page cache scale to ~8 threads
    for one process (186 k utterances/s of 200 x 80 f32 on 8 threads against 172 k on 4 and 92 k on one, on the GPU box's 256-core host);
    with 4 - 8 ranks reading at once 4 threads per rank give the best aggregate and 8 lose 6 - 16 % (tools/bench_loaders.py,
    profiles/r6*_loaders*.txt)."""
    try:
        cores = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        cores = os.cpu_count() or 1
    try:
        ranks = int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1")))
    except ValueError:
        ranks = 1
    default = 8 if ranks <= 2 else 4
    return max(1, min(int(os.environ.get("ASV_AMD_READER_THREADS", str(default))), cores))


def _report_loop(path, n, seconds, sets, spent=None):
    """ASV_AMD_REPORT_TIMING=1: one line with the rate of the read -> device -> write loop alone (model load, engine compilation and
    process start excluded; tools/bench_pipeline.py and bench.py's supplementary.ark_to_ark read it)."""
    if os.environ.get("ASV_AMD_REPORT_TIMING", "0") not in ("0", "", "false"):
        print("Loop[{0}]: {1} utterances in {2:.4f} s = {3:.1f} utterances/s (reader -> device -> writer; range re-runs: {4})".format(
            path, n, seconds, n / max(seconds, 1e-9), sets.range_reruns))
        if spent:
            print("Loop[{0}] consumer thread: ".format(path) + ", ".join("{0} {1:.4f} s".format(k, v) for k, v in spent.items()))
        print("Loop[{0}] submit pieces: ".format(path) + ", ".join("{0} {1:.4f} s".format(k, v) for k, v in sets.submit_seconds.items()))


_SCP_PREFIX = re.compile(r"^scp(,[a-z_,]*)?:")


class ScpTable(object):
    """The entries of a Kaldi scp table as a read-only sequence of (key, rxfile) tuples over ONE native parse of the file's bytes
    (libasv_io.so asv_io_parse_scp): the tuples are made when asked for.  Every rank of a --sharded run walks the WHOLE table - it needs
    every length to balance the shards - and as a Python list of tuples + a per-entry parse in ScpBatchLoader.index_all that was
    0.12 - 0.18 s per 50 000 entries and rank: the part of the host work that did not scale with the ranks (tools/bench_loaders.py,
    profiles/r6h_loaders_before.txt).  `plain_index()` hands the loader the parsed 'path:offset' arrays."""

    def __init__(self, data, parsed):
        self._data, self._p, self._n = data, parsed, int(parsed["n"])

    def __len__(self):
        return self._n

    def _entry(self, i):
        p, d = self._p, self._data
        a, b = int(p["key_off"][i]), int(p["rx_off"][i])
        return d[a:a + int(p["key_len"][i])].decode("latin1"), d[b:b + int(p["rx_len"][i])].decode("latin1")

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self._entry(k) for k in range(*i.indices(self._n))]
        if i < 0:
            i += self._n
        if not 0 <= i < self._n:
            raise IndexError(i)
        return self._entry(i)

    def __iter__(self):
        return (self._entry(i) for i in range(self._n))

    def __eq__(self, other):                               # (a sequence of tuples: equal to the list the Python parse returns)
        try:
            return len(other) == self._n and all(x == tuple(y) for x, y in zip(self, other))
        except TypeError:
            return NotImplemented

    __hash__ = None

    def keys(self, a=0, b=None):
        """The keys of entries [a, b) (what rank 0 writes a segment's vectors under)."""
        p, d = self._p, self._data
        b = self._n if b is None else b
        return [d[int(o):int(o) + int(l)].decode("latin1") for o, l in zip(p["key_off"][a:b], p["key_len"][a:b])]

    def plain_index(self):
        """(path id per entry or -1, byte offset per entry, the distinct paths) of the entries of the plain form 'path:offset'."""
        return self._p["path_id"], self._p["offset"], self._p["paths"]


def read_scp(path):
    """The (key, rxfile) entries of a Kaldi scp rspecifier: 'scp:feats.scp', with options ('scp,p:', 'scp,s,cs:' - accepted and ignored,
    like the reference's read_mat_scp), 'scp:-' (stdin), 'scp:cmd |' (a pipe), .gz; the prefix is optional.  A ScpTable (one native
    parse) when libasv_io.so is there, else a list of tuples - the same sequence either way."""
    m = _SCP_PREFIX.match(path)
    name = path[m.end():] if m else path
    if name.strip() == "-":
        data = sys.stdin.buffer.read() if hasattr(sys.stdin, "buffer") else sys.stdin.read().encode("latin1")
    else:
        fd = kaldi_io.open_or_fd(name.strip(), "rb")
        try:
            data = fd.read()
        finally:
            fd.close()
    from libs.support import native_io
    parsed = native_io.parse_scp(data) if native_io.lib() is not None else None
    if parsed is not None:
        return ScpTable(data, parsed)
    return [tuple(line.strip().split(None, 1)) for line in data.decode("latin1").splitlines() if line.strip()]


_RANGE = re.compile(r"\[([0-9]*):?([0-9]*)(?:,([0-9]*):?([0-9]*))?\]$")


def split_range(rxfile):
    """Kaldi scp range specifier 'file.ark:123[r0:r1]' / '[r0:r1,c0:c1]' (both ends inclusive, either part may be empty) ->
    (rxfile without it, row slice, column slice).  The nj-job splits of the reference go through Kaldi's copy-feats, which
    accepts such entries."""
    m = _RANGE.search(rxfile)
    if not m:
        return rxfile, slice(None), slice(None)
    def sl(a, b):
        return slice(int(a) if a else None, int(b) + 1 if b else None)
    body = rxfile[:m.start()]
    return body, sl(m.group(1), m.group(2)), sl(m.group(3), m.group(4))


def read_matrix(rxfile):
    """float32 matrix behind an scp entry, range specifier applied."""
    body, rows, cols = split_range(rxfile)
    return np.ascontiguousarray(kaldi_io.read_mat(body)[rows, cols], dtype=np.float32)


def matrix_rows(rxfile):
    """Number of rows of the matrix behind an scp entry, from its header only (FM / DM / CM / CM2 / CM3 - the compressed
    formats share the GlobalHeader), or by decoding it (text); a range specifier is applied to the count."""
    import struct
    body, rows, _ = split_range(rxfile)
    fd = kaldi_io.open_or_fd(body, "rb")
    try:
        head = fd.read(2)
        if head != b"\0B":
            fd.close()
            n = int(kaldi_io.read_mat(body).shape[0])
        else:
            tag = fd.read(3)
            if tag in (b"FM ", b"DM "):
                n = struct.unpack("<bibi", fd.read(10))[1]
            elif tag == b"CM ":
                n = struct.unpack("<ffii", fd.read(16))[2]
            elif tag in (b"CM2", b"CM3"):
                fd.read(1)                                # the space behind the 3-letter token
                n = struct.unpack("<ffii", fd.read(16))[2]
            else:
                raise kaldi_io.UnknownMatrixHeader("The header contained '%s'" % tag)
    finally:
        fd.close()
    return len(range(*rows.indices(n)))


class PackedBatch(object):
    """The matrices of one batch as row slices of ONE buffer: `packed` [frames, D] float32, `offsets` int32 [n + 1]; `turn`: the slot of
    the loader's buffer rotation this batch consumed (always - the caller's pipeline rotates with it); `own_array`: the batch did not
    fit that buffer (one utterance longer than a whole batch) and lies in an array of its own.  A sequence of the [T_k, D] views, made
    when asked for (the device path takes `packed` and `offsets` as they are: 321 views per batch were 50 000 slicing calls per run
    that nobody looked at)."""

    def __init__(self, packed, offsets, turn, own_array=False):
        self.packed, self.offsets, self.turn, self.own_array = packed, offsets, turn, own_array

    def __len__(self):
        return len(self.offsets) - 1

    def __getitem__(self, k):
        if isinstance(k, slice):
            return [self[j] for j in range(*k.indices(len(self)))]
        if k < 0:
            k += len(self)
        if not 0 <= k < len(self):
            raise IndexError(k)
        return self.packed[int(self.offsets[k]):int(self.offsets[k + 1])]

    def __iter__(self):
        return (self[k] for k in range(len(self)))


class ScpBatchLoader(object):
    """Loads the utterances of a batch from scp entries into one packed buffer - the host side of the sharded path and of `scp:` input.

    Until round 4 a rank read its shard one `read_mat` at a time (open, parse, array) and concatenated the batch: 10 k utterances/s
    (0.65 GB/s) per rank against 56 k for the sequential stream reader and ~950 k the device extracts.  Here an uncompressed float32
    entry 'file.ark:offset' (what copy-feats / the reference's make_features write) costs one 15-byte header pread and one read of its
    payload straight into its rows of the batch buffer; everything else - float64, compressed, text matrices, range specifiers,
    pipes - goes through read_matrix and is copied in.  A COMPRESSED 'file.ark:offset' entry ('CM ' / 'CM2' / 'CM3': what Kaldi's
    make_fbank.sh / make_mfcc.sh write) is a second kind of direct entry: its format, body offset, rows and columns are in the header
    table too (lengths() and shape() answer from it), and load_compressed() reads the bodies of a batch as they are into a byte
    buffer for the device decode - fill() / load_batch() still decode such an entry on the host.  Two buffers alternate: libs.amd.shard.extract_sharded fetches batch k + 1
    while batch k is on the device.  The buffers are the loader's own arrays, or the CALLER's (`buffers`: e.g. the page-locked
    input buffers of libs.amd.pipeline.DeviceSets, so that the H2D copy starts from where the file was read to; `before_fill(turn)`
    is then called before buffer `turn` is overwritten - the caller waits for its copy out of it there).  `loader(i)` (one
    utterance) stays available: it is what extract_sharded takes as `load_utt`.
    The payload reads of a batch are ONE call into libasv_io.so (csrc/host_io.c: positioned reads on `threads` native threads,
    the GIL released for the whole call); without that library (not built) the same reads are issued from Python, one per
    utterance.  Measured on the build host (20 000 x [200, 80] float32 from the page cache; LABLOG.md row "a16, e (host side)"):
    203 k utterances/s = 13 GB/s on 4 native threads (1: 92 k, 8: 213 k); the Python reads: 66 k on one thread and LESS when
    split over Python threads (4: 43 k - a 64 KiB read is ~12 us, the Python around it ~3 us under the GIL, the hand-over
    between threads costs more than it buys); the round-3 path (read_mat per utterance + concatenate): 10 k.
    Descriptors: one per ark file, kept in an LRU of `max_open` (a feats.scp of an augmented / nj-split feature directory names
    more files than the soft RLIMIT_NOFILE allows open at once - ADVICE r4); the files of the batch being read are never evicted."""

    def __init__(self, entries, threads=4, buffers=None, before_fill=None, max_open=256):
        import collections
        import threading
        self.entries = entries
        self.threads = max(1, int(threads))
        self.max_open = max(1, int(max_open))
        self._fds = collections.OrderedDict()            # path -> descriptor, least recently used first
        self._heads = {}
        self._table = None                               # index_all(): (plain, file id, payload offset, rows, cols) arrays + the file list
        self._ctable = None                              # index_all(): (format 0 / 1 / 2 / 3, body offset, rows, cols) arrays of the COMPRESSED direct entries
        self._cheads = {}
        self._bufs = list(buffers) if buffers is not None else [None, None]
        self._own = buffers is None
        self._before_fill = before_fill
        self._turn = 0
        self._lock = threading.Lock()

    def __call__(self, i):
        return read_matrix(self.entries[i][1])

    def close(self):
        with self._lock:
            for fd in self._fds.values():
                os.close(fd)
            self._fds.clear()

    def _fd(self, path, keep=()):
        """Descriptor of `path` (opened on demand, most recently used last); beyond max_open the least recently used one that the
        current batch (`keep`) does not need is closed."""
        with self._lock:
            fd = self._fds.get(path)
            if fd is not None:
                self._fds.move_to_end(path)
                return fd
            if len(self._fds) >= self.max_open:
                for old in list(self._fds):
                    if len(self._fds) < self.max_open:
                        break
                    if old not in keep:
                        os.close(self._fds.pop(old))
            fd = self._fds[path] = os.open(path, os.O_RDONLY)
            return fd

    def _direct(self, i):
        """(path, payload offset, rows, cols) of entry i if it is a plain float32 'file:offset' entry, else None (parsed once)."""
        h = self._heads.get(i, 0)
        if h != 0:
            return h
        if self._table:
            plain, fid, pos, rows, cols, files = self._table
            return (files[fid[i]], int(pos[i]), int(rows[i]), int(cols[i])) if plain[i] else None
        import struct
        rxfile = self.entries[i][1]
        h = None
        if not (rxfile.endswith("]") or rxfile.endswith("|") or ":" not in rxfile):
            path, _, off = rxfile.rpartition(":")
            if off.isdigit() and (path in self._fds or os.path.isfile(path)):
                off = int(off)
                head = os.pread(self._fd(path), 15, off)
                if len(head) == 15 and head[:5] == b"\0BFM " and head[5] == 4 and head[10] == 4:
                    h = (path, off + 15, struct.unpack_from("<i", head, 6)[0], struct.unpack_from("<i", head, 11)[0])
        self._heads[i] = h
        return h

    @staticmethod
    def _parse_compressed(heads):
        """heads uint8 [m, 22+]: the first bytes of m entries -> (format uint8 [m]: 1 'CM ', 2 'CM2', 3 'CM3', 0 none of them; token length,
        rows, cols of the 16-byte global header {float min, float range, int32 rows, int32 cols} behind the token)."""
        cm = (heads[:, 0] == 0) & (heads[:, 1] == ord("B")) & (heads[:, 2] == ord("C")) & (heads[:, 3] == ord("M"))
        fmt = np.zeros(len(heads), dtype=np.uint8)
        fmt[cm & (heads[:, 4] == ord(" "))] = 1
        fmt[cm & (heads[:, 4] == ord("2")) & (heads[:, 5] == ord(" "))] = 2
        fmt[cm & (heads[:, 4] == ord("3")) & (heads[:, 5] == ord(" "))] = 3
        token = np.where(fmt == 1, 5, 6).astype(np.int64)
        at = token[:, None] + np.arange(8, 16, dtype=np.int64)[None]
        counts = np.ascontiguousarray(np.take_along_axis(heads, at, axis=1)).view("<i4")
        rows, cols = counts[:, 0].astype(np.int64), counts[:, 1].astype(np.int64)
        fmt[(rows < 1) | (cols < 1)] = 0                     # (an empty or damaged matrix: the host reader deals with it)
        return fmt, token, rows, cols

    def _direct_compressed(self, i):
        """(path, body offset, rows, cols, format) of entry i if it is a Kaldi compressed matrix ('CM ' = 1, 'CM2' = 2, 'CM3' = 3) behind a
        'file:offset' entry without range specifier, else None.  The body starts at the 16-byte global header behind the token."""
        if self._ctable is not None:
            fmt, body, rows, cols = self._ctable
            if not fmt[i]:
                return None
            return self._table[5][self._table[1][i]], int(body[i]), int(rows[i]), int(cols[i]), int(fmt[i])
        h = self._cheads.get(i, 0)
        if h != 0:
            return h
        rxfile = self.entries[i][1]
        h = None
        if not (rxfile.endswith("]") or rxfile.endswith("|") or ":" not in rxfile):
            path, _, off = rxfile.rpartition(":")
            if off.isdigit() and (path in self._fds or os.path.isfile(path)):
                off = int(off)
                head = os.pread(self._fd(path), 22, off)
                if len(head) >= 21:
                    fmt, token, rows, cols = self._parse_compressed(np.frombuffer(head.ljust(22, b"\0"), dtype=np.uint8)[None])
                    if fmt[0] and len(head) >= int(token[0]) + 16:
                        h = (path, off + int(token[0]), int(rows[0]), int(cols[0]), int(fmt[0]))
        self._cheads[i] = h
        return h

    def compressed_format(self, i):
        """1 / 2 / 3 when entry i is a compressed direct entry ('CM ' / 'CM2' / 'CM3': its body can be read as it is and decoded on the
        device), else 0."""
        h = self._direct_compressed(i)
        return h[4] if h is not None else 0

    def has_compressed(self):
        """Does the table hold a compressed direct entry?  From the header table where there is one, else entry by entry up to the first."""
        if self.index_all():
            return bool(self._ctable[0].any())
        return any(self._direct_compressed(i) is not None for i in range(len(self.entries)))

    def _index_compressed(self, cand, heads15, lut, fid, off):
        """Second header pass of index_all: the candidates whose first 15 bytes did not say `\\0BFM ` but `\\0BCM` get 22 bytes read (token +
        global header; one native call) - the table of the compressed direct entries.  Per rank under --sharded: no collective."""
        from libs.support import native_io
        n = len(self.entries)
        fmt_all, body, rows, cols = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        maybe = cand[(heads15[:, 0] == 0) & (heads15[:, 1] == ord("B")) & (heads15[:, 2] == ord("C")) & (heads15[:, 3] == ord("M"))]
        if len(maybe):
            heads = np.zeros((len(maybe), 32), dtype=np.uint8)
            try:
                native_io.pread_batch(lut[fid[maybe]], off[maybe], np.full(len(maybe), 22, dtype=np.int64), heads.ctypes.data,
                                      np.arange(len(maybe), dtype=np.int64) * 32, threads=self.threads)
            except OSError:
                # (a 21-byte 'CM ' entry without a single column at the very end of a file: the same reads one by one, short ones allowed)
                heads[:] = 0
                for j, i in enumerate(maybe.tolist()):
                    got = os.pread(int(lut[fid[i]]), 22, int(off[i]))
                    if len(got) == 22 or (len(got) == 21 and got[4:5] == b" "):
                        heads[j, :len(got)] = np.frombuffer(got, dtype=np.uint8)
            fmt, token, r, c = self._parse_compressed(heads)
            good = fmt > 0
            at = maybe[good]
            fmt_all[at], body[at], rows[at], cols[at] = fmt[good], off[at] + token[good], r[good], c[good]
        self._ctable = (fmt_all, body, rows, cols)

    def index_all(self, ranks=None):
        """`ranks` = (rank, world, gather) under --sharded with more than one rank: the header pass is SHARED - every rank reads the
        headers of one contiguous 1 / world of the entries and `gather(local uint8 array) -> [world, ...] array` (an all-gather)
        completes the table on every rank (round 6: the per-rank pass over the WHOLE table was what did not scale on one host - 0.10 s
        per 50 000 entries on every rank, 64 % of a rank's host work at 8 ranks, tools/bench_loaders.py).  Every rank must hold the same
        table; the ranks first compare (entries, plain candidates, a checksum of their offsets) and fall back to the whole pass, each on
        its own, if they differ; a failed header read on any rank sends all of them to the per-entry path together.

        Headers of ALL plain float32 'file:offset' entries in one native call (15 bytes each, libasv_io.so asv_io_pread_batch) and a
        vectorised parse: arrays (plain, file id, payload offset, rows, cols) that load_batch() indexes with a batch's entry numbers -
        per batch a handful of numpy operations instead of ~10 Python operations per utterance (50 000 utterances: 0.15 s of
        interpreter time on the reader thread, under the GIL the submitting thread needs too; the header pass itself 0.2 s -> 0.03 s).
        Without the native library, with more files than `max_open`, or if any header read fails, the per-entry path stays in charge
        (returns False)."""
        if self._table is not None:
            return self._table is not False
        self._table = False
        from libs.support import native_io
        sharing = ranks is not None and ranks[1] > 1
        if native_io.lib() is None:
            if sharing:
                ranks[2](np.zeros((1, 16), dtype=np.uint8))          # take part in the agreement (as "nothing to share"): nobody waits for this rank
            return False
        n = len(self.entries)
        if hasattr(self.entries, "plain_index"):
            # the table was parsed natively (ScpTable): path ids and offsets are arrays already - no per-entry Python
            pid, poff, paths = self.entries.plain_index()
            remap = np.full(len(paths) + 1, -1, dtype=np.int32)          # (slot -1 = "not plain": stays -1)
            files = []
            for k, path in enumerate(paths):
                if os.path.isfile(path):
                    remap[k] = len(files)
                    files.append(path)
            fid_all = remap[pid]                                          # pid = -1 indexes the last slot
            cand = np.flatnonzero(fid_all >= 0).astype(np.int64)
            fid, off = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int64)
            fid[cand], off[cand] = fid_all[cand], poff[cand]
        else:
            files, ids, cand, c_fid, c_off = [], {}, [], [], []
            for i, (_, rx) in enumerate(self.entries):
                path, sep, o = rx.rpartition(":")
                if not sep or not o.isdigit():                # (range specifiers end in ']', pipes in '|': neither is all digits)
                    continue
                j = ids.get(path)
                if j is None:
                    j = ids[path] = len(files) if os.path.isfile(path) else -1
                    if j >= 0:
                        files.append(path)
                if j >= 0:
                    cand.append(i)
                    c_fid.append(j)
                    c_off.append(int(o))
            fid, off = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int64)
            fid[cand], off[cand] = c_fid, c_off
        if len(cand) == 0 or len(files) > self.max_open:
            if sharing:
                ranks[2](np.zeros((1, 16), dtype=np.uint8))          # (as above)
            return False
        cand = np.asarray(cand, dtype=np.int64)
        keep = set(files)
        lut = np.asarray([self._fd(path, keep=keep) for path in files], dtype=np.int32)
        nc = len(cand)
        shared = False
        if sharing:
            rank, world, gather = ranks
            mine = np.zeros((1, 16), dtype=np.uint8)
            mine.view("<i8")[0, 0], mine.view("<i8")[0, 1] = nc * 1000003 + n, int(np.bitwise_xor.reduce(off[cand] * 31 + fid[cand]))
            seen = gather(mine)
            shared = bool((seen == mine[None]).all())          # the same table on every rank (else: every rank for itself, no further collective)
        if shared:
            per = -(-nc // world)
            lo, hi = min(rank * per, nc), min((rank + 1) * per, nc)
            local = np.zeros((per + 1, 16), dtype=np.uint8)      # last row: this rank's reads succeeded
            try:
                if hi > lo:
                    native_io.pread_batch(lut[fid[cand[lo:hi]]], off[cand[lo:hi]], np.full(hi - lo, 15, dtype=np.int64), local.ctypes.data,
                                          np.arange(hi - lo, dtype=np.int64) * 16, threads=self.threads)
                local[per, 0] = 1
            except OSError:
                pass
            full = gather(local)
            if not (full[:, per, 0] == 1).all():
                return False                              # every rank sees the same flags: all of them take the per-entry path
            heads = np.ascontiguousarray(full[:, :per].reshape(-1, 16)[:nc])
        else:
            heads = np.zeros((nc, 16), dtype=np.uint8)
            try:
                native_io.pread_batch(lut[fid[cand]], off[cand], np.full(nc, 15, dtype=np.int64), heads.ctypes.data,
                                      np.arange(nc, dtype=np.int64) * 16, threads=self.threads)
            except OSError:
                return False                              # (an offset at the very end of a file: the per-entry path names the entry)
        ok = (heads[:, 0] == 0) & (heads[:, 1] == ord("B")) & (heads[:, 2] == ord("F")) & (heads[:, 3] == ord("M")) & (heads[:, 4] == ord(" ")) & \
             (heads[:, 5] == 4) & (heads[:, 10] == 4)
        rows_c = np.ascontiguousarray(heads[:, 6:10]).view("<i4").ravel()
        cols_c = np.ascontiguousarray(heads[:, 11:15]).view("<i4").ravel()
        plain = np.zeros(n, dtype=bool)
        rows, cols = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        good = cand[ok]
        plain[good], rows[good], cols[good] = True, rows_c[ok], cols_c[ok]
        self._table = (plain, fid, off + 15, rows, cols, files)
        self._index_compressed(cand, heads, lut, fid, off)
        return True

    def lengths(self):
        """Frames of every entry, from the headers (what the length-balanced sharding needs when no utt2num_frames is given)."""
        if self.index_all():
            plain, _, _, rows, _, _ = self._table
            fmt, _, c_rows, _ = self._ctable
            out = np.where(fmt > 0, c_rows, rows)
            for i in np.nonzero(~plain & (fmt == 0))[0]:
                out[i] = matrix_rows(self.entries[i][1])
            return out
        out = np.empty(len(self.entries), dtype=np.int64)
        for i, (_, rx) in enumerate(self.entries):
            h = self._direct(i) or self._direct_compressed(i)
            out[i] = h[2] if h is not None else matrix_rows(rx)
        return out

    def shape(self, i, slow=None):
        """(rows, cols) of entry i: from its header if it is a plain float32 or a compressed direct entry, else by decoding it (the
        matrix is kept in `slow[i]` for the fill that follows)."""
        h = self._direct(i) or self._direct_compressed(i)
        if h is not None:
            return h[2], h[3]
        m = slow.get(i) if slow is not None else None
        if m is None:
            m = self(i)
            if slow is not None:
                slow[i] = m
        return m.shape

    def fill(self, indices, packed, offs, slow=None):
        """Reads the matrices of `indices` into packed[offs[k]:offs[k + 1]] (C-contiguous [frames, dim] float32); `slow`: already
        decoded matrices of non-plain entries by entry index."""
        heads = [self._direct(i) for i in indices]
        dim = packed.shape[1]
        n = len(indices)
        slow = slow if slow is not None else {}
        ks = [k for k in range(n) if heads[k] is not None]
        paths = {heads[k][0] for k in ks}
        fds = {path: self._fd(path, keep=paths) for path in paths}
        for k in range(n):
            if heads[k] is None:
                i = indices[k]
                m = slow[i] if i in slow else self(i)
                packed[int(offs[k]):int(offs[k + 1])] = m
        if not ks:
            return
        from libs.support import native_io
        if native_io.lib() is not None:
            try:
                native_io.pread_batch([fds[heads[k][0]] for k in ks], [heads[k][1] for k in ks], [(int(offs[k + 1]) - int(offs[k])) * dim * 4 for k in ks],
                                      packed.ctypes.data, [int(offs[k]) * dim * 4 for k in ks], threads=self.threads)
            except OSError as e:
                k = ks[e.args[2]] if len(e.args) > 2 else ks[0]
                raise kaldi_io.BadInputFormat("scp entry %r: %s" % (self.entries[indices[k]][1], e.args[1]))
            return
        raw = memoryview(packed.reshape(-1).view(np.uint8))
        for k in ks:
            h, a, b = heads[k], int(offs[k]), int(offs[k + 1])
            fd, pos, want = fds[h[0]], h[1], (b - a) * dim * 4
            got, view = 0, raw[a * dim * 4:b * dim * 4]
            while got < want:
                r = os.preadv(fd, [view[got:]], pos + got)
                if r <= 0:
                    raise kaldi_io.BadInputFormat("scp entry %r: the archive ends inside the matrix" % (self.entries[indices[k]][1],))
                got += r

    def fill_rows(self, spans, packed):
        """Rows of parents into a packed buffer (the sliding mode): `spans` = [(entry, row0, row1, at)] - rows [row0, row1) of entry's
        matrix go to packed[at:at + row1 - row0].  A plain float32 direct entry costs one positioned read of exactly those rows (all of
        a call's in one native call); every other kind is decoded on the host - ONCE per parent: the last decoded matrix is kept, the
        spans of a long parent follow one another."""
        from libs.support import native_io
        dim = packed.shape[1]
        fds, pos, size, at_byte, who = [], [], [], [], []
        for i, row0, row1, at in spans:
            h = self._direct(i)
            if h is not None and h[3] == dim and 0 <= row0 <= row1 <= h[2]:
                fds.append(h[0]); pos.append(h[1] + row0 * dim * 4); size.append((row1 - row0) * dim * 4); at_byte.append(at * dim * 4); who.append(i)
                continue
            if getattr(self, "_last_parent", (None, None))[0] != i:
                self._last_parent = (i, self(i))
            m = self._last_parent[1]
            if m.shape[1] != dim or row1 > m.shape[0]:
                raise kaldi_io.BadInputFormat("scp entry %r is %d x %d: rows %d:%d of %d columns were asked for" % (
                    self.entries[i][1], m.shape[0], m.shape[1], row0, row1, dim))
            packed[at:at + row1 - row0] = m[row0:row1]
        if not who:
            return
        paths = set(fds)
        fds = [self._fd(path, keep=paths) for path in fds]
        if native_io.lib() is not None:
            try:
                native_io.pread_batch(fds, pos, size, packed.ctypes.data, at_byte, threads=self.threads)
            except OSError as e:
                k = e.args[2] if len(e.args) > 2 else 0
                raise kaldi_io.BadInputFormat("scp entry %r: %s" % (self.entries[who[k]][1], e.args[1]))
            return
        raw = memoryview(packed.reshape(-1).view(np.uint8))
        for k in range(len(who)):
            got = 0
            while got < size[k]:
                r = os.preadv(fds[k], [raw[at_byte[k] + got:at_byte[k] + size[k]]], pos[k] + got)
                if r <= 0:
                    raise kaldi_io.BadInputFormat("scp entry %r: the archive ends inside the matrix" % (self.entries[who[k]][1],))
                got += r

    def load_compressed(self, indices, byte_buffer):
        """The BODIES of the compressed direct entries `indices` (each from its 16-byte global header, as it lies in the file), read in one
        native call into the caller's uint8 `byte_buffer` (e.g. the page-locked staging buffer of libs.amd.pipeline.DeviceSets), every
        body at a 16-byte boundary: what libs.amd.frontend.decode_compressed / DeviceSets.submit_compressed take.  Returns (byte_offsets
        int64 [n], frame_offsets int64 [n + 1], formats uint8 [n], used_bytes).  The rows and columns the device will address come from
        the header table; they are compared here with the header of every body as it was read, before anything is copied on."""
        from libs.amd.frontend import compressed_body_bytes
        from libs.support import native_io
        if byte_buffer.dtype != np.uint8 or byte_buffer.ndim != 1 or not byte_buffer.flags["C_CONTIGUOUS"] or byte_buffer.ctypes.data % 16:
            raise ValueError("load_compressed: byte_buffer must be a contiguous 1-D uint8 array that starts at a 16-byte boundary")
        n = len(indices)
        if self._ctable is not None:                         # the header table: a batch's arguments by array indexing, as _fill_table
            idx = np.asarray(indices, dtype=np.int64)
            t_fmt, t_body, t_rows, t_cols = self._ctable
            formats, pos, rows, cols = t_fmt[idx], t_body[idx], t_rows[idx], t_cols[idx]
            if not formats.all():
                raise ValueError("scp entry %r is not a compressed direct entry" % (self.entries[int(idx[np.flatnonzero(formats == 0)[0]])][1],))
            files, fid = self._table[5], self._table[1][idx]
            paths = [files[j] for j in fid.tolist()]
        else:
            heads = [self._direct_compressed(int(i)) for i in indices]
            for i, h in zip(indices, heads):
                if h is None:
                    raise ValueError("scp entry %r is not a compressed direct entry" % (self.entries[int(i)][1],))
            pos = np.asarray([h[1] for h in heads], dtype=np.int64)
            rows = np.asarray([h[2] for h in heads], dtype=np.int64)
            cols = np.asarray([h[3] for h in heads], dtype=np.int64)
            formats = np.asarray([h[4] for h in heads], dtype=np.uint8)
            paths = [h[0] for h in heads]
        if n and (cols != cols[0]).any():
            raise ValueError("feature matrices of different widths in one batch: %s" % sorted(set(cols.tolist())))
        size = compressed_body_bytes(formats, rows, cols).astype(np.int64) if n else np.zeros(0, dtype=np.int64)
        byte_off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum((size + 15) // 16 * 16, out=byte_off[1:])
        used = int(byte_off[-1])
        if used > byte_buffer.shape[0]:
            raise ValueError("load_compressed: the bodies take %d bytes, the buffer holds %d" % (used, byte_buffer.shape[0]))
        frame_off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(rows, out=frame_off[1:])
        byte_off = byte_off[:-1].copy()
        used_paths = set(paths)
        fds = {path: self._fd(path, keep=used_paths) for path in used_paths}
        if native_io.lib() is not None:
            try:
                native_io.pread_batch([fds[path] for path in paths], pos, size, byte_buffer.ctypes.data, byte_off, threads=self.threads)
            except OSError as e:
                k = e.args[2] if len(e.args) > 2 else 0
                raise kaldi_io.BadInputFormat("scp entry %r: %s" % (self.entries[int(indices[k])][1], e.args[1]))
        else:
            raw = memoryview(byte_buffer)
            for k, path in enumerate(paths):
                a, want, got = int(byte_off[k]), int(size[k]), 0
                while got < want:
                    r = os.preadv(fds[path], [raw[a + got:a + want]], int(pos[k]) + got)
                    if r <= 0:
                        raise kaldi_io.BadInputFormat("scp entry %r: the archive ends inside the matrix" % (self.entries[int(indices[k])][1],))
                    got += r
        if n:
            counts = byte_buffer[(byte_off[:, None] + np.arange(8, 16, dtype=np.int64)[None]).ravel()].reshape(n, 8).view("<i4")
            bad = np.flatnonzero((counts[:, 0] != rows) | (counts[:, 1] != cols))
            if len(bad):
                k = int(bad[0])
                raise kaldi_io.BadInputFormat("scp entry %r: its header now says %d x %d, the header table %d x %d (the archive changed under the run?)" % (
                    self.entries[int(indices[k])][1], int(counts[k, 0]), int(counts[k, 1]), int(rows[k]), int(cols[k])))
        return byte_off, frame_off, formats, used

    def load_batch(self, indices):
        slow = {}
        idx = np.asarray(indices, dtype=np.int64)
        fast = bool(self._table) and len(idx) > 0 and bool(self._table[0][idx].all())     # every entry of the batch is in the header table
        if fast:
            _, _, _, t_rows, t_cols, _ = self._table
            cols = t_cols[idx]
            dim = int(cols[0])
            if (cols != dim).any():
                raise ValueError("feature matrices of different widths in one batch: %s" % sorted(set(cols.tolist())))
            offs = np.zeros(len(idx) + 1, dtype=np.int32)
            np.cumsum(t_rows[idx], out=offs[1:])
        else:
            shapes = [self.shape(i, slow) for i in indices]
            dims = {c for _, c in shapes}
            if len(dims) != 1:
                raise ValueError("feature matrices of different widths in one batch: %s" % sorted(dims))
            dim = dims.pop()
            offs = np.zeros(len(indices) + 1, dtype=np.int32)
            np.cumsum([r for r, _ in shapes], out=offs[1:])
        total = int(offs[-1])
        own = False
        turn, self._turn = self._turn, (self._turn + 1) % len(self._bufs)
        if self._before_fill is not None:
            self._before_fill(turn)
        buf = self._bufs[turn]
        if self._own:
            if buf is None or buf.size < total * dim:
                buf = self._bufs[turn] = np.empty(max(total * dim, 1), dtype=np.float32)
            packed = buf[:total * dim].reshape(total, dim)
        elif buf.ndim == 2 and buf.shape[1] == dim and buf.shape[0] >= total:
            packed = buf[:total]
        else:                                          # does not fit the caller's buffer (one utterance longer than a whole batch): its own array
            packed, own = np.empty((total, dim), dtype=np.float32), True       # (the slot of the rotation is consumed all the same)
        if fast:
            self._fill_table(idx, packed, offs, dim)
        else:
            self.fill(indices, packed, offs, slow)
        return PackedBatch(packed, offs, turn, own)

    def _fill_table(self, idx, packed, offs, dim):
        """fill() for a batch whose entries are all in the header table: the arguments of the one native read call by array indexing."""
        from libs.support import native_io
        _, t_fid, t_pos, _, _, files = self._table
        fid = t_fid[idx]
        used = np.unique(fid)
        keep = {files[j] for j in used.tolist()}
        lut = np.zeros(len(files), dtype=np.int32)
        for j in used.tolist():
            lut[j] = self._fd(files[j], keep=keep)
        o64 = offs.astype(np.int64)
        try:
            native_io.pread_batch(lut[fid], t_pos[idx], (o64[1:] - o64[:-1]) * (dim * 4), packed.ctypes.data, o64[:-1] * (dim * 4), threads=self.threads)
        except OSError as e:
            k = e.args[2] if len(e.args) > 2 else 0
            raise kaldi_io.BadInputFormat("scp entry %r: %s" % (self.entries[int(idx[k])][1], e.args[1]))


class CompressedGroup(object):
    """What ScpGroupReader.read_group returns in the place of the row count for a group of compressed direct entries: the bodies lie
    in the caller's byte buffer (ScpBatchLoader.load_compressed), the rows are still to be decoded (DeviceSets.submit_compressed)."""

    def __init__(self, frames, byte_off, frame_off, formats, used_bytes):
        self.frames, self.byte_off, self.frame_off, self.formats, self.used_bytes = frames, byte_off, frame_off, formats, used_bytes


class ScpGroupReader(object):
    """kaldi_io.PackedArkReader's interface (peek_dim / read_group) over scp entries IN SCP ORDER: what extract_stream reads `scp:`
    input through when the run is not sharded - batches are written as they finish, memory is one batch, the keys print as they go
    (the reference's loop over read_mat_scp does the same one utterance at a time, extract_embeddings.py:70-83).  Packed ragged
    batches have no padding, so nothing is gained by sorting a single process's utterances by length."""

    def __init__(self, entries, threads=4):
        self.entries = entries
        self.loader = ScpBatchLoader(entries, threads=threads)
        self._at = 0
        self._slow = {}
        self.row_pad = 0                                   # as kaldi_io.PackedArkReader.row_pad

    def close(self):
        self.loader.close()

    def peek_dim(self):
        if self._at >= len(self.entries):
            return None
        return int(self.loader.shape(self._at, self._slow)[1])

    def has_compressed(self):
        return self.loader.has_compressed()

    def _compressed_bytes(self, i, cap, byte_cap):
        """Bytes entry i takes in a byte buffer (its body, rounded up to 16) if it goes the compressed route: a compressed direct entry
        whose rows fit a batch buffer and whose body fits the byte buffer; else 0 (host decode, as every other kind of entry)."""
        h = self.loader._direct_compressed(i)
        if h is None or h[2] > cap:
            return 0
        _, _, rows, cols, fmt = h                           # (libs.amd.frontend.compressed_body_bytes, on plain integers: once per entry)
        size = (16 + (8 * cols + rows * cols if fmt == 1 else 2 * rows * cols if fmt == 2 else rows * cols) + 15) // 16 * 16
        return size if size <= byte_cap else 0

    def read_group(self, feats, max_utts=1024, byte_buffer=None):
        """`byte_buffer` (uint8, e.g. DeviceSets.byte_buffer(k)): compressed direct entries are NOT decoded here - a group is cut where
        the kind changes between them and everything else, and a group of them comes back as (keys, offsets, CompressedGroup) with the
        bodies in byte_buffer; it is cut by rows exactly as any other group, and by the bytes the buffer holds."""
        cap, dim = feats.shape
        idx, offs, used = [], [0], 0
        byte_cap = byte_buffer.shape[0] if byte_buffer is not None else 0
        kind, used_bytes = None, 0
        while len(idx) < max_utts and self._at < len(self.entries):
            i = self._at
            rows, cols = self.loader.shape(i, self._slow)
            if byte_buffer is not None:
                size = self._compressed_bytes(i, cap, byte_cap)
                if kind is None:
                    kind = size > 0
                if kind != (size > 0) or used_bytes + size > byte_cap:
                    break
            if cols != dim:
                raise kaldi_io.BadInputFormat("scp entry '%s' has %d columns, the table started with %d" % (self.entries[i][0], cols, dim))
            if rows > cap:
                if idx:
                    break                                  # flush what we have first
                self._at += 1
                big = np.empty((rows, dim), dtype=np.float32)
                self.loader.fill([i], big, np.array([0, rows], dtype=np.int32), self._slow)
                self._slow.pop(i, None)
                return [self.entries[i][0]], np.array([0, rows], dtype=np.int32), big
            if used + rows > cap or (idx and used + rows + self.row_pad * (len(idx) + 2) > cap):
                break
            idx.append(i)
            used += rows
            offs.append(used)
            self._at += 1
            if kind:
                used_bytes += size
        offs = np.asarray(offs, dtype=np.int32)
        if idx and kind:
            byte_off, frame_off, formats, used_bytes = self.loader.load_compressed(idx, byte_buffer)
            return [self.entries[i][0] for i in idx], offs, CompressedGroup(used, byte_off, frame_off, formats, used_bytes)
        if idx:
            self.loader.fill(idx, feats[:used], offs, self._slow)
            for i in idx:
                self._slow.pop(i, None)
        return [self.entries[i][0] for i in idx], offs, used


def sliding_windows(entries, lengths, opts, warn=None):
    """The windows of a sliding run: (ids, windows, subsegments) - `windows` = [(entry index, first row, rows)] in processing order
    (the parents in scp order, each one's windows in start order), `ids` the sub-segment ids the vectors are written under,
    `subsegments` everything libs.amd.subsegments.uniform_subsegments made of the segments file (what --subsegments-out holds)."""
    from libs.amd import subsegments
    keys = entries.keys() if hasattr(entries, "plain_index") else [k for k, _ in entries]
    index = {}
    for i, key in enumerate(keys):
        index.setdefault(key, i)
    with kaldi_io.open_or_fd(opts.segments, "rb") as f:
        lines = [line for line in f.read().decode("latin1").splitlines() if line.strip()]
    for line in lines:
        if len(line.split()) < 4:
            raise ValueError("--segments %s: a line needs '<utt> <rec> <start> <end>', got %r" % (opts.segments, line))
        if line.split()[0] not in index:
            raise ValueError("--segments %s: %r is not a key of the features' scp" % (opts.segments, line.split()[0]))
    subs = subsegments.uniform_subsegments(lines, opts.window, opts.period, opts.min_segment, True, opts.hard_min)
    num_frames = {utt: int(lengths[index[utt]]) for utt in {s[1] for s in subs}}
    kept, first, last = subsegments.frame_ranges(subs, num_frames, opts.frame_shift,
                                                 warn=warn if warn is not None else (lambda line: print("WARNING: " + line, file=sys.stderr)))
    # (a stable sort: windows of equal start - two segments of one parent - keep the order of the segments file)
    order = sorted(range(len(kept)), key=lambda w: (index[kept[w][1]], first[w]))
    return [kept[w][0] for w in order], [(index[kept[w][1]], first[w], last[w] - first[w] + 1) for w in order], subs


def extract_sliding_scp(model, entries, w, opts, batch_frames, batch_utts, max_chunk, verbose=False, ingest=None):
    """The reference's sliding (diarisation) mode over scp entries: every segment of opts.segments is cut into uniform overlapping
    sub-segments (libs.amd.subsegments), each a row range of its parent's matrix, and one vector per sub-segment is written under the
    sub-segment's id.  The reference reads a range-specified scp - the whole parent once per window; here a parent's rows are read and
    uploaded ONCE per batch that holds windows of it (libs.amd.subsegments.cut_spans: whole parents, or spans of a long one), and
    asv_ingest_windows builds the batch of windows from the resident rows, CMN per window (DeviceSets.submit_windows).  Plain float32
    direct entries are read by positioned reads of the spans' rows; compressed direct entries that fit a buffer set travel as their
    bodies and are decoded on the device (ASV_AMD_DEVICE_DECODE=0: on the host); every other kind is decoded on the host, once per
    parent.  The loop is extract_stream's: reader thread, three buffer sets, the writer behind the device."""
    import queue
    import threading
    from libs.amd import subsegments
    from libs.amd.pipeline import DeviceSets, IngestOptions
    if max_chunk is None:
        max_chunk = getattr(type(model).extract_embedding, "max_chunk", 10000)
    if ingest is None:
        ingest = IngestOptions()                        # --cmn-window 0: the windows' rows as they are
    refuse_ranged_entries(entries)
    loader = ScpBatchLoader(entries, threads=_reader_threads())
    clock = time.perf_counter
    try:
        # (the header pass, the windows and the cut are this mode's own host work: counted into the loop's clock below - the
        #  range-specified scp they replace comes ready-made)
        t_windows = clock()
        loader.index_all()
        lengths = loader.lengths()
        ids, windows, subs = sliding_windows(entries, lengths, opts)
        if opts.subsegments_out:
            with open(opts.subsegments_out, "w") as f:
                f.write("".join(line + "\n" for line in subsegments.format_subsegments(subs)))
        if not windows:
            return 0
        dim = int(loader.shape(windows[0][0])[1])
        for p in sorted({win[0] for win in windows}):
            h = loader._direct(p) or loader._direct_compressed(p)
            if h is not None and h[3] != dim:
                raise kaldi_io.BadInputFormat("scp entry '%s' has %d columns, the table started with %d" % (entries[p][0], h[3], dim))
        device_decode = os.environ.get("ASV_AMD_DEVICE_DECODE", "1") != "0"
        whole = {p for p in {win[0] for win in windows} if device_decode and loader.compressed_format(p) and lengths[p] <= batch_frames}
        batches = subsegments.cut_spans(lengths, windows, batch_frames, batch_utts, whole=whole)
        t_windows = clock() - t_windows
        sets = DeviceSets(model, batch_frames, batch_utts, dim, max_chunk, n_sets=3, results="host", ingest=ingest, compressed=bool(whole), windows=True)
        free_sets, staged = queue.Queue(), queue.Queue()
        for k in range(sets.n_sets):
            free_sets.put(k)

        def produce():
            try:
                for batch in batches:
                    k = free_sets.get()
                    w0, w1 = batch.spans[0].w0, batch.spans[-1].w1
                    if batch.own:                         # one window longer than a whole buffer: an array of its own, submit()'s own path
                        span = batch.spans[0]
                        big = np.empty((span.row1 - span.row0, dim), dtype=np.float32)
                        loader.fill_rows([(span.parent, span.row0, span.row1, 0)], big)
                        staged.put((k, w0, w1, big, None, None, None))
                        continue
                    at, fills, start = 0, [], np.zeros(w1 - w0, dtype=np.int64)
                    for span in batch.spans:
                        fills.append((span.parent, span.row0, span.row1, at))
                        for j in range(span.w0, span.w1):
                            start[j - w0] = at + windows[j][1] - span.row0
                        at += span.row1 - span.row0
                    rows = np.asarray([windows[j][2] for j in range(w0, w1)], dtype=np.int64)
                    packed = None
                    if batch.whole:
                        packed = loader.load_compressed([span.parent for span in batch.spans], sets.byte_buffer(k))
                    else:
                        loader.fill_rows(fills, sets.host_buffer(k))
                    staged.put((k, w0, w1, at, start, rows, packed))
                staged.put(None)
            except BaseException as e:                    # surfaces in the consumer
                staged.put(e)

        spent = {"windows": t_windows, "reader": 0.0, "submit": 0.0, "device": 0.0, "write": 0.0}
        t = threading.Thread(target=produce, daemon=True)
        t.start()
        n_done, in_flight = 0, None

        def finish(item):
            k, keys = item
            a = clock()
            vectors = sets.finish(k)
            b = clock()
            if verbose:
                for key in keys:
                    print("Process utterance for key {0}".format(key))
            w.write(kaldi_io.vec_flt_ark_bytes(keys, vectors))
            free_sets.put(k)
            spent["device"] += b - a
            spent["write"] += clock() - b
            return len(keys)

        t0 = clock()
        while True:
            a = clock()
            item = staged.get()
            b = clock()
            spent["reader"] += b - a
            if isinstance(item, BaseException):
                raise item
            if item is None:
                break
            k, w0, w1, frames, start, rows, packed = item
            if start is None:
                sets.submit(k, np.array([0, frames.shape[0]], dtype=np.int32), frames)
            else:
                sets.submit_windows(k, frames, start, rows, packed=packed)
            spent["submit"] += clock() - b
            if in_flight is not None:
                n_done += finish(in_flight)
            in_flight = (k, ids[w0:w1])
        if in_flight is not None:
            n_done += finish(in_flight)
        t.join()
        _report_loop("sliding", n_done, t_windows + clock() - t0, sets, spent)
        return n_done
    finally:
        loader.close()


def _shard_segment_utts(lengths=None, batch_frames=0, batch_utts=0, row_pad=0):
    """Utterances per rank between two gathers of the sharded path (ASV_AMD_SHARD_SEGMENT, default 4096; 0 = one gather at the very
    end), rounded to whole batches of the mean utterance: a segment's last batch is a partial one, and on a device-bound run (f32x)
    a 245-utterance batch costs what a 321-utterance batch costs - 13 segments of 4096 x 200-frame utterances were 169 batches
    instead of 156 (profiles/r5x_ark_*.json: --sharded 195 k utterances/s in f32x against 250 k through the stream path, while the
    host-bound bf16 run was already level)."""
    want = max(0, int(os.environ.get("ASV_AMD_SHARD_SEGMENT", "4096")))
    if want == 0 or lengths is None or len(lengths) == 0 or batch_frames <= 0:
        return want
    mean = float(np.mean(lengths))
    per_batch = int(max(1, min(batch_utts if batch_utts > 0 else 1 << 30, (batch_frames - row_pad) // max(1.0, mean + row_pad))))
    return max(per_batch, int(round(want / float(per_batch))) * per_batch)


def extract_sharded_scp(extract_batch, entries, lengths, w, batch_frames, batch_utts, verbose=False, device=None, loader=None, row_pad=0,
                        segment_utts=None, timing=None):
    """Sharded extraction of scp entries (one call per rank, torch.distributed initialised or not):
        extract_batch(list of [T, D] float32 matrices) -> [b, E] tensor
    The scp is walked in segments of `segment_utts` utterances per rank (default: ASV_AMD_SHARD_SEGMENT = 4096): every rank extracts
    its length-balanced share of a segment, one all-gather per segment, and rank 0 writes the segment's ark entries to `w` - in scp
    order - on a writer thread while the next segment is being extracted (libs.amd.shard.extract_sharded_segments).
    Returns the number of embeddings (on every rank)."""
    import queue
    import threading
    import torch.distributed as dist
    from libs.amd import shard
    rank = dist.get_rank() if (dist.is_available() and dist.is_initialized()) else 0
    load = loader if loader is not None else ScpBatchLoader(entries, threads=_reader_threads())
    # (only rank 0 writes: the keys of a segment are made when it is written - 50 000 tuples up front on every rank were part of the
    #  per-rank cost that does not shrink with the number of ranks)
    keys_of = entries.keys if hasattr(entries, "keys") and not isinstance(entries, dict) else (lambda a, b: [k for k, _ in entries[a:b]])
    todo, failed = queue.Queue(), []

    def write_segments():
        while True:
            item = todo.get()
            if item is None:
                return
            a, b, emb = item
            if failed:
                continue
            try:
                seg_keys = keys_of(a, b)
                if verbose:
                    for key in seg_keys:
                        print("Process utterance for key {0}".format(key))
                w.write(kaldi_io.vec_flt_ark_bytes(seg_keys, emb.cpu().numpy(), as_buffer=True))
            except Exception as e:                       # re-raised on the caller's thread below
                failed.append(e)

    writer = threading.Thread(target=write_segments, name="asv-shard-writer", daemon=True) if rank == 0 else None
    if writer is not None:
        writer.start()
    try:
        n = shard.extract_sharded_segments(extract_batch, lengths, load, (lambda a, b, emb: todo.put((a, b, emb))) if rank == 0 else (lambda a, b, emb: None),
                                           _shard_segment_utts(lengths, batch_frames, batch_utts, row_pad) if segment_utts is None else segment_utts,
                                           max_frames=batch_frames, max_utts=batch_utts, device=device, row_pad=row_pad, timing=timing)
    finally:
        t0 = time.perf_counter()
        if writer is not None:
            todo.put(None)
            writer.join()
        if timing is not None:
            timing["writer_join"] = timing.get("writer_join", 0.0) + time.perf_counter() - t0
        if loader is None:
            load.close()
    if failed:
        raise failed[0]
    return n


def index_ranks(device=None):
    """(rank, world, gather) for ScpBatchLoader.index_all under an initialised process group of more than one rank, else None.  `gather`
    all-gathers a uint8 array - through device memory under NCCL / RCCL (`device`), host memory under gloo."""
    import torch.distributed as dist
    if not dist.is_initialized() or dist.get_world_size() < 2 or os.environ.get("ASV_AMD_SHARD_INDEX", "1") == "0":
        return None
    world = dist.get_world_size()
    where = device if (device is not None and dist.get_backend() == "nccl") else torch.device("cpu")

    def gather(local):
        t = torch.from_numpy(np.ascontiguousarray(local)).to(where)
        out = torch.empty((world * t.shape[0],) + tuple(t.shape[1:]), dtype=torch.uint8, device=where)      # (the concatenated form: gloo takes no other)
        dist.all_gather_into_tensor(out, t)
        return out.cpu().numpy().reshape((world,) + tuple(t.shape))

    return dist.get_rank(), world, gather


def run_sharded(args, model, max_chunk, verbose):
    import torch.distributed as dist
    from libs.amd.pipeline import DeviceSets
    if not _SCP_PREFIX.match(args.feats_rspecifier):
        raise ValueError("--sharded needs random access to the features: pass 'scp:feats.scp' (the reference shards feats.scp too, "
                         "splitDataByLength.sh:44-80), not %r" % args.feats_rspecifier)
    entries = read_scp(args.feats_rspecifier)
    engine = model._amd_engine()
    dev = torch.device("cuda", engine.device_index)
    if max_chunk is None:
        max_chunk = getattr(type(model).extract_embedding, "max_chunk", 10000)
    # the device side is the stream path's: page-locked input buffers the loader reads the files INTO, asynchronous H2D, two engines
    # on two HIP streams, the range status word behind every batch (libs.amd.pipeline.DeviceSets) - until round 5 this path copied a
    # pageable batch synchronously into ONE engine and never looked at the status word
    sets = DeviceSets(model, args.batch_frames, args.batch_utts, engine.feat_dim, max_chunk, n_sets=3, results="device", ingest=ingest_options(args))
    loader = ScpBatchLoader(entries, threads=_reader_threads(),
                            buffers=[sets.host_buffer(k) for k in range(sets.n_sets)], before_fill=sets.input_consumed)
    # all headers in one native call (also what lengths() below reads) - under several ranks each reads 1 / world of them and one
    # all-gather completes the table (ASV_AMD_SHARD_INDEX=0: every rank reads all of them)
    loader.index_all(ranks=index_ranks(dev))
    if args.utt2num_frames:
        table = dict(line.split() for line in open(args.utt2num_frames) if line.strip())
        lengths = np.array([int(table[k]) for k, _ in entries], dtype=np.int64)
    else:
        lengths = loader.lengths()                     # one 15-byte pread per plain float32 entry (a descriptor per ark file, not per entry)

    spent = {"finish": 0.0}

    def extract_batch(mats):
        if getattr(mats, "packed", None) is not None:        # ScpBatchLoader: the batch already lies packed in one (page-locked) buffer
            k = mats.turn                                    # the slot the loader consumed: an over-long batch (own array) keeps the rotation too
            t0 = time.perf_counter()
            sets.finish(k)                                   # the batch before last (same set): done by now; range guard
            spent["finish"] += time.perf_counter() - t0
            return sets.submit(k, mats.offsets, mats.packed if mats.own_array else int(mats.offsets[-1]))
        offs = np.zeros(len(mats) + 1, dtype=np.int32)
        np.cumsum([m.shape[0] for m in mats], out=offs[1:])
        sets.finish(0)
        return sets.submit(0, offs, np.concatenate(mats, axis=0))

    extract_batch.flush = sets.flush                       # extract_sharded_segments calls it before it reads the last results ...
    base = sets.submitted
    extract_batch.final_through = lambda: sets.final_through() - base      # ... and reads a segment's results once its last submission is final
    rank = dist.get_rank() if dist.is_initialized() else 0
    w = kaldi_io.open_or_fd(args.vectors_wspecifier, "wb") if rank == 0 else None
    try:
        t0 = time.perf_counter()
        with torch.cuda.device(dev):
            n = extract_sharded_scp(extract_batch, entries, lengths, w, args.batch_frames, args.batch_utts, verbose, device=dev, loader=loader, row_pad=4,
                                    timing=spent)
        if rank == 0:
            _report_loop("sharded", n, time.perf_counter() - t0, sets, spent)
        if rank == 0 and dist.is_initialized():
            with open("/proc/self/maps") as f:
                rccl = "librccl" in f.read()
            print("Sharded over {0} rank(s); embeddings collected by all_gather_into_tensor, backend {1} (librccl mapped: {2}).".format(
                dist.get_world_size(), dist.get_backend(), rccl))
        return n
    finally:
        loader.close()
        if w is not None:
            w.close()


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
        if not utils.to_bool(args.use_gpu):
            raise RuntimeError("asv-subtools_amd extracts on a ROCm device only (--use-gpu=true); there is no CPU path")

        sharded = utils.to_bool(args.sharded)
        sliding = sliding_options(args)               # (refuses what the sliding mode does not take before anything is set up)
        ingest = ingest_options(args)                 # (refuses --sharded true --vad-scp before anything is set up)
        if sharded:
            import torch.distributed as dist
            os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # dmabuf IPC for RCCL on these hosts
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            local_rank = int(os.environ.get("LOCAL_RANK", "0"))
            if args.gpu_id == "":
                args.gpu_id = str(local_rank)                               # one process per GPU
            torch.cuda.set_device(int(args.gpu_id))
            # the process group exists at every world size, 1 included (under torch.distributed.run --nproc-per-node 1 or without
            # a launcher): the collection step is then always RCCL's all-gather - one code path, exercised on a single GPU too
            if "RANK" not in os.environ or "WORLD_SIZE" not in os.environ:
                os.environ["RANK"], os.environ["WORLD_SIZE"] = "0", "1"
            if "MASTER_PORT" not in os.environ:
                # a free local port only for the launcher-less single-rank run: ranks of a real job that each picked their own
                # port would wait for one another until the rendezvous times out
                if int(os.environ["WORLD_SIZE"]) != 1:
                    raise RuntimeError("--sharded with WORLD_SIZE=%s needs MASTER_PORT (and MASTER_ADDR) in the environment: launch with "
                                       "`python -m torch.distributed.run --nproc-per-node N ...` or export them" % os.environ["WORLD_SIZE"])
                import socket
                with socket.socket() as sock:
                    sock.bind(("127.0.0.1", 0))
                    os.environ["MASTER_PORT"] = str(sock.getsockname()[1])
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", int(args.gpu_id)))   # "nccl" is RCCL on ROCm
            # RCCL builds its communicator inside the first collective (0.1 - 0.2 s): here, with the model still to be loaded, not
            # inside the extraction loop in front of the all-gather
            wdev = torch.device("cuda", int(args.gpu_id))
            warm = torch.zeros(2, dtype=torch.int64, device=wdev)
            dist.all_reduce(warm, op=dist.ReduceOp.MAX)                       # (the two collectives of libs/amd/shard.py, each once)
            wsrc = torch.zeros((8, 8), dtype=torch.float32, device=wdev)
            wdst = torch.empty((8 * dist.get_world_size(), 8), dtype=torch.float32, device=wdev)
            dist.all_gather_into_tensor(wdst, wsrc)
            torch.cuda.synchronize(wdev)
            del warm, wsrc, wdst

        model = utils.create_model_from_py(model_blueprint, model_creation)
        model.load_state_dict(torch.load(args.model_path, map_location="cpu"), strict=False)
        model = utils.select_model_device(model, args.use_gpu, gpu_id=args.gpu_id)
        model.eval()
        max_chunk = args.max_chunk if args.max_chunk > 0 else None
        verbose = utils.to_bool(args.verbose)

        n_done = 0
        vad = VadTable(args.vad_scp, threads=_reader_threads()) if args.vad_scp else None
        if sliding is not None:
            with kaldi_io.open_or_fd(args.vectors_wspecifier, "wb") as w:
                n_done = extract_sliding_scp(model, read_scp(args.feats_rspecifier), w, sliding, args.batch_frames, args.batch_utts, max_chunk, verbose,
                                             ingest=ingest)
        elif sharded:
            import torch.distributed as dist
            n_done = run_sharded(args, model, max_chunk, verbose)
            if dist.is_initialized():
                dist.barrier()
                dist.destroy_process_group()
        elif _SCP_PREFIX.match(args.feats_rspecifier):
            # random-access input without --sharded (the reference's script reads `scp:` through read_mat_scp): the stream loop over
            # a reader that fills its batches from the scp entries in order - vectors are written batch by batch, in scp order
            reader = ScpGroupReader(read_scp(args.feats_rspecifier), threads=_reader_threads())
            try:
                with kaldi_io.open_or_fd(args.vectors_wspecifier, "wb") as w:
                    n_done = extract_stream(model, None, w, args.batch_frames, args.batch_utts, max_chunk, verbose, reader=reader, ingest=ingest, vad=vad)
            finally:
                reader.close()
        else:
            with kaldi_io.open_or_fd(args.feats_rspecifier, "rb") as r, kaldi_io.open_or_fd(args.vectors_wspecifier, "wb") as w:
                n_done = extract_stream(model, r, w, args.batch_frames, args.batch_utts, max_chunk, verbose, ingest=ingest, vad=vad)
        if vad is None:
            print("Extracted {0} embeddings.".format(n_done))
        else:
            vad.close()
            print("Extracted {0} embeddings; skipped {1} utterances (no usable VAD vector or no voiced frame).".format(n_done, vad.skipped))
            if n_done == 0 and vad.skipped > 0:
                raise RuntimeError("every utterance was skipped (select-voiced-frames exits 1 when it wrote nothing)")
    except BaseException as e:
        if not isinstance(e, KeyboardInterrupt):
            traceback.print_exc()
        sys.exit(1)


if __name__ == "__main__":
    main()
