# -*- coding:utf-8 -*-
"""Device side of the pipelined extraction loops of pipeline/onestep/extract_embeddings.py (the stream path AND the sharded path):
buffer sets of {page-locked host input, device input, own engine on its own HIP stream, page-locked result / status word}, one
batch per set in flight, so that reading batch i + 1 and writing batch i - 1 overlap the device work of batch i and consecutive
batches overlap on the device (the small launches at the end of one beside the wide GEMMs at the start of the next).

It is also where the range guard of the default precision mode reaches the scripts (VERDICT r4 / ADVICE r4): 'f32x' splits operands
into IEEE-half halves; an activation beyond +-65504 raises a status bit (asv_net_status).  Engine.extract_batch() checks it; the
scripts go through Engine.extract_device(), which cannot (no host synchronisation) - so every batch submitted here carries an
asynchronous copy of the status word behind its result copy (asv_net_status_async, no extra wait), and a batch that raised the bit
is re-run on the engine's bf16-halves twin ('f32x-bf16': the whole f32 exponent range, ~6e-6 relative) before its vectors are
handed on, with the same RuntimeWarning.  The fp32 reference has no such limit
(/root/reference/pytorch/pipeline/onestep/extract_embeddings.py:70-83 writes whatever the f32 forward gives).
"""

import collections
import os
import warnings

import numpy as np

from . import capi

# What DeviceSets does to RAW features before the extractor reads them (asv_ingest_frames, one launch per batch): sliding-window CMN
# with Kaldi's apply-cmvn-sliding options (cmn_window = 0: none) and, with flags=True, select-voiced-frames by one flag per raw frame
# handed to submit().  The defaults are those of the reference's extract_xvectors_for_pytorch.sh:105-118.
IngestOptions = collections.namedtuple("IngestOptions", "cmn_window min_window center norm_vars flags")
IngestOptions.__new__.__defaults__ = (0, 100, True, False, False)


class DeviceSets(object):
    """`n_sets` buffer sets (and `n_engines` engines, each on its own HIP stream) for batches of at most `batch_frames` frames / `batch_utts` utterances.

        sets = DeviceSets(model, batch_frames, batch_utts, dim, max_chunk)
        buf = sets.host_buffer(k)                      # [batch_frames, dim] float32 numpy view of page-locked memory: the reader fills it
        sets.submit(k, offsets, frames)                # async: H2D, extraction, result (+ status) copy; `frames` = rows used of buffer k,
                                                       #        or an ndarray of its own (one utterance longer than the whole buffer)
        sets.input_consumed(k)                         # blocks until buffer k may be refilled (its H2D has finished)
        vectors = sets.finish(k)                       # blocks until the batch is done; range guard; [n, E] float32:
                                                       #   results='host': numpy view of page-locked memory (valid until the next submit(k))
                                                       #   results='device': a CUDA tensor of its own (stays valid)
    ingest=IngestOptions(...): the rows the reader fills are RAW features - every set also holds a second device buffer and (flags=True)
    a page-locked flag buffer with its device twin, and submit(k, offsets, frames, voiced) puts the fused CMN + selection launch between the
    H2D copies and the extraction, on the same stream (no synchronisation: the kept counts come from the host flags).  The engine sees
    the compacted rows and offsets; utterances that keep no frame are left out (finish() returns one vector per utterance that kept some).
    compressed=True: the reader may hand over Kaldi COMPRESSED matrices as they lie on disk - every set also holds a page-locked uint8
    staging buffer (byte_buffer(k), filled by ScpBatchLoader.load_compressed) with its device twin, and submit_compressed() copies the
    bytes used and decodes them on the engine's stream (asv_decode_compressed) into the rows submit() would have copied, then goes on as
    submit() does.  A quarter of the H2D bytes, and no decode on the host.
    windows=True (with ingest=, without flags): submit_windows() takes the rows of a set as PARENT matrices and a list of windows of them
    (the reference's sliding / diarisation mode) - one launch (asv_ingest_windows) gathers and normalises every window as an utterance of
    its own into the rows the engine reads; overlapping windows are uploaded once.
    ASV_AMD_PIPELINE_ENGINES=1 keeps one engine on one stream (device-resident rate of two: +5 % x-vector, +9 % ECAPA, +19 %
    ResNet34-SE, profiles/r3h_streams.txt)."""

    def __init__(self, model, batch_frames, batch_utts, dim, max_chunk, n_sets=3, results="host", n_engines=2, warm=True, ingest=None, compressed=False, windows=False):
        import torch
        assert results in ("host", "device")
        self.torch = torch
        self.results = results
        self.max_chunk = int(max_chunk)
        engine = model._amd_engine()
        if dim != engine.feat_dim:
            raise ValueError("the input holds %d-dimensional features, the model expects %d" % (dim, engine.feat_dim))
        self.dev = dev = torch.device("cuda", engine.device_index)
        self.n_sets = n_sets
        # engines / streams are fewer than buffer sets: a third set lets the reader fill batch i + 2 while batch i + 1 waits behind
        # batch i on the device and batch i - 1 is being written (with two sets the read of batch i + 1 only started once batch
        # i - 1 had been written: 173 k instead of 240 k utterances/s through the f32x stream path, profiles/r5a_ark_to_ark.json)
        if os.environ.get("ASV_AMD_PIPELINE_ENGINES", "2") == "1":
            n_engines = 1
        if n_engines <= 1:
            self.engines = [engine]
            self.streams = [torch.cuda.current_stream(dev)]
        else:
            # (cached on the model like the first engine: a second loop over the same model compiles nothing)
            self.engines = [engine] + [model._amd_engine(replica=k) for k in range(1, n_engines)]
            self.streams = [torch.cuda.Stream(device=dev) for _ in range(n_engines)]
        self._next_engine = 0
        self.embed_dim = engine.embed_dim
        self.watch = engine._range_fallback_applies()
        self.host_in = [torch.empty((batch_frames, dim), dtype=torch.float32).pin_memory() for _ in range(n_sets)]
        self.host_np = [t.numpy() for t in self.host_in]
        self.dev_in = [torch.empty((batch_frames, dim), dtype=torch.float32, device=dev) for _ in range(n_sets)]
        self.status_host = [torch.zeros(1, dtype=torch.int32).pin_memory() for _ in range(n_sets)]
        self.ingest = ingest
        self.dev_raw = self.host_flags = self.flags_np = self.dev_flags = None          # ingest=None: nothing is allocated, nothing is launched
        if ingest is not None:
            if ingest.cmn_window > 0 and not ingest.center and not 0 < ingest.min_window <= ingest.cmn_window:
                raise ValueError("sliding CMN without centring needs 0 < min_window <= cmn_window (got %d, %d)" % (ingest.min_window, ingest.cmn_window))
            self.dev_raw = [torch.empty((batch_frames, dim), dtype=torch.float32, device=dev) for _ in range(n_sets)]
            if ingest.flags:
                self.host_flags = [torch.zeros(batch_frames, dtype=torch.uint8).pin_memory() for _ in range(n_sets)]
                self.flags_np = [t.numpy() for t in self.host_flags]
                self.dev_flags = [torch.empty(batch_frames, dtype=torch.uint8, device=dev) for _ in range(n_sets)]
        if windows and (ingest is None or ingest.flags):
            raise ValueError("windows=True needs ingest=IngestOptions(...) without flags: the raw rows need a device buffer of their own, "
                             "and the reference's sliding mode has no VAD")
        self.windows = bool(windows)
        self.batch_utts = int(batch_utts)
        self.host_bytes = self.bytes_np = self.dev_bytes = None                          # compressed=False: nothing is allocated, nothing is launched
        if compressed:
            # the worst case of a full batch: 'CM2' takes 2 bytes per value, every body its global header, 'CM ' its column headers, and
            # each starts at a 16-byte boundary
            size = 2 * batch_frames * dim + batch_utts * (32 + 8 * dim)
            self.host_bytes = [torch.zeros(size, dtype=torch.uint8).pin_memory() for _ in range(n_sets)]
            self.bytes_np = [t.numpy() for t in self.host_bytes]
            self.dev_bytes = [torch.zeros(size, dtype=torch.uint8, device=dev) for _ in range(n_sets)]
        if results == "host":
            self.dev_out = [torch.empty((batch_utts, self.embed_dim), dtype=torch.float32, device=dev) for _ in range(n_sets)]
            self.host_out = [torch.empty((batch_utts, self.embed_dim), dtype=torch.float32).pin_memory() for _ in range(n_sets)]
        self.h2d = [torch.cuda.Event() for _ in range(n_sets)]
        self.done = [torch.cuda.Event() for _ in range(n_sets)]
        self.pending = [None] * n_sets                   # (feats tensor, offsets, out tensor, n, engine index, submission number) of the batch in flight on a set
        self.submitted = 0                               # submit() calls so far
        if warm:
            # one full-size batch of zeros through every engine now: the activation arenas (grown on demand by the first extraction:
            # a few hundred MB of hipMalloc per engine) and the segment tables exist before the first real batch arrives
            utts = max(1, min(batch_utts, batch_frames // 204))
            offs = (np.arange(utts + 1, dtype=np.int64) * (batch_frames // utts)).astype(np.int32)
            with torch.cuda.device(dev):
                self.dev_in[0][:int(offs[-1])].zero_()
                for e, eng in enumerate(self.engines):
                    with torch.cuda.stream(self.streams[e]):
                        eng.extract_device(self.dev_in[0][:int(offs[-1])], offs, max_chunk=self.max_chunk)
                        if ingest is not None:         # (the ingest kernel's code object, and this thread's offset staging in the library)
                            self._ingest(self.dev_in[0][:int(offs[-1])], offs.astype(np.int64), None, None, self.dev_raw[0])
                        if self.windows:               # (the windows kernel's code object and its staging: asked for by the caller alone)
                            self._ingest_windows(self.dev_in[0][:int(offs[-1])], (offs[:-1].astype(np.int64), np.diff(offs).astype(np.int64)), self.dev_raw[0])
                        if compressed:                 # (the decode kernel's code object and its offset staging; a one-row 'CM3' body of zeros)
                            self._decode(self.dev_bytes[0], np.zeros(1, dtype=np.int64), np.array([0, 1], dtype=np.int64), np.full(1, 3, dtype=np.uint8),
                                         (self.dev_in if ingest is None else self.dev_raw)[0])
                        if self.watch:
                            eng.status_async(self.status_host[0])
                for st in self.streams:
                    st.synchronize()
            self.status_host[0].zero_()
        self.range_reruns = 0
        self.submit_seconds = {}                         # host time inside submit() by piece (ASV_AMD_REPORT_TIMING)

    def host_buffer(self, k):
        return self.host_np[k]

    def flag_buffer(self, k):
        """[batch_frames] uint8 numpy view of set k's page-locked flag buffer (ingest with flags): the reader fills it next to host_buffer(k)."""
        return self.flags_np[k]

    def byte_buffer(self, k):
        """uint8 numpy view of set k's page-locked staging buffer for compressed bodies (compressed=True)."""
        return self.bytes_np[k]

    def _decode(self, dev_bytes, byte_off, frame_off, formats, out):
        from . import frontend
        return frontend.decode_compressed(dev_bytes, byte_off, frame_off, formats, out.shape[1], out=out)

    def _ingest(self, raw, raw_off, dev_flags, kept_off, out):
        from . import frontend
        o = self.ingest
        return frontend.ingest(raw, raw_off, voiced=dev_flags, cmn_window=o.cmn_window, min_window=o.min_window, center=o.center,
                               norm_vars=o.norm_vars, out=out, kept_off=kept_off)[0]

    def _ingest_windows(self, raw, windows, out):
        from . import frontend
        o = self.ingest
        return frontend.ingest_windows(raw, windows[0], windows[1], cmn_window=o.cmn_window, min_window=o.min_window, center=o.center,
                                       norm_vars=o.norm_vars, out=out)[0]

    def submit_windows(self, k, frames, win_start, win_len, packed=None):
        """The first `frames` rows of host_buffer(k) are RAW rows of parent matrices; window w is rows [win_start[w], win_start[w] +
        win_len[w]) of them and becomes one utterance: copied once, then gathered and normalised per window (asv_ingest_windows, the
        options of `ingest`) into the rows the engine reads - everything behind that is submit()'s.  `packed` = (byte_off, frame_off,
        formats, used_bytes): the rows lie in byte_buffer(k) as compressed bodies instead and are decoded on the device first, as
        submit_compressed() does.  `frames` may also be a [rows, dim] f32 CUDA tensor of the caller's (rows that are on the device
        already, e.g. one long parent whose windows take several batches): nothing is copied; the caller has made sure that the tensor
        is complete before the call and keeps it alive until finish(k)."""
        torch = self.torch
        if not self.windows:
            raise ValueError("these buffer sets were made without windows=True")
        start, rows = np.ascontiguousarray(win_start, dtype=np.int64), np.ascontiguousarray(win_len, dtype=np.int64)
        if start.ndim != 1 or start.shape != rows.shape or not 1 <= len(start) <= self.batch_utts:
            raise ValueError("submit_windows: between 1 and batch_utts windows, one start and one length each (got %d)" % len(start))
        cap = self.dev_in[k].shape[0]
        resident = isinstance(frames, torch.Tensor)
        if resident:
            if frames.dim() != 2 or frames.dtype != torch.float32 or frames.device != self.dev or not frames.is_contiguous() or frames.shape[1] != self.dev_in[k].shape[1]:
                raise ValueError("submit_windows: resident rows must be a contiguous [rows, %d] f32 tensor on %s" % (self.dev_in[k].shape[1], self.dev))
            have = frames.shape[0]
        else:
            have = frames = int(frames)
            if not 0 < have <= cap:
                raise ValueError("submit_windows: %d raw rows do not fit the buffer set (%d rows)" % (have, cap))
        if (start < 0).any() or (rows < 1).any() or (start + rows > have).any():
            raise ValueError("submit_windows: a window is empty or lies outside the %d raw rows" % have)
        offsets = np.zeros(len(start) + 1, dtype=np.int64)
        np.cumsum(rows, out=offsets[1:])
        if int(offsets[-1]) > cap:
            raise ValueError("submit_windows: the windows hold %d rows, the buffer set %d" % (int(offsets[-1]), cap))
        if packed is not None:
            if self.dev_bytes is None or resident:
                raise ValueError("submit_windows: compressed bodies need buffer sets made with compressed=True (and rows of the set's own)")
            byte_off, frame_off, formats, used_bytes = packed
            frame_off = np.ascontiguousarray(frame_off, dtype=np.int64)
            if int(frame_off[-1]) != have or not 0 < int(used_bytes) <= self.dev_bytes[k].shape[0]:
                raise ValueError("submit_windows: the compressed bodies hold %d rows in %d bytes, the call says %d rows (byte buffer: %d)" % (
                    int(frame_off[-1]), int(used_bytes), have, self.dev_bytes[k].shape[0]))
            packed = (np.ascontiguousarray(byte_off, dtype=np.int64), frame_off, formats, int(used_bytes))
        return self._submit(k, offsets.astype(np.int32), frames, packed, None, None, windows=(start, rows))

    def submit(self, k, offsets, frames, voiced=None, kept_off=None):
        """`voiced` (ingest with flags): one uint8 flag per raw row - flag_buffer(k)[:frames] as the reader filled it, or an array of its
        own; `kept_off`: its per-utterance running sum where the caller has it already (frontend.kept_offsets)."""
        return self._submit(k, offsets, frames, None, voiced, kept_off)

    def submit_compressed(self, k, byte_off, frame_off, formats, used_bytes, voiced=None, kept_off=None):
        """The batch lies in byte_buffer(k)[:used_bytes] as compressed bodies (what ScpBatchLoader.load_compressed returned): the bytes
        are copied, decoded on the engine's stream into the rows submit() copies, and everything behind that is submit()'s."""
        if self.dev_bytes is None:
            raise ValueError("these buffer sets were made without compressed=True")
        frame_off = np.ascontiguousarray(frame_off, dtype=np.int64)
        rows, used_bytes = int(frame_off[-1]), int(used_bytes)
        if rows > self.dev_in[k].shape[0] or not 0 < used_bytes <= self.dev_bytes[k].shape[0]:
            raise ValueError("a compressed batch of %d rows in %d bytes does not fit the buffer set (%d rows, %d bytes)" % (
                rows, used_bytes, self.dev_in[k].shape[0], self.dev_bytes[k].shape[0]))
        return self._submit(k, frame_off.astype(np.int32), rows, (np.ascontiguousarray(byte_off, dtype=np.int64), frame_off, formats, used_bytes), voiced, kept_off)

    def _submit(self, k, offsets, frames, packed, voiced, kept_off, windows=None):
        """submit() (`packed` None: `frames` rows of host_buffer(k), or an array of its own) and submit_compressed() (`packed` = (byte_off,
        frame_off, formats, used_bytes) of byte_buffer(k)): they differ in what is copied to the device and in the decode launch behind
        the copy - the flags, the ingest, the extraction, the result copy and the status word are the same code.  `windows` (submit_windows:
        (start, rows) of every window of the raw rows; `offsets` are then the windows' own) swaps the ingest launch for the windows one."""
        torch = self.torch
        assert self.pending[k] is None, "set %d still holds a batch: finish() it first" % k
        n = len(offsets) - 1
        raw_off = None
        if self.ingest is not None:
            raw_off = np.ascontiguousarray(offsets, dtype=np.int64)
            if self.ingest.flags:
                if voiced is None:
                    raise ValueError("these buffer sets select voiced frames: submit() needs the flags of the batch")
                from . import frontend
                voiced = np.asarray(voiced)
                if voiced.dtype != np.uint8 or voiced.ndim != 1 or voiced.shape[0] < int(raw_off[-1]):
                    raise ValueError("voiced must hold one uint8 flag per raw frame")
                if kept_off is None:
                    kept_off = frontend.kept_offsets(voiced, raw_off)[1]
                kept_off = np.ascontiguousarray(kept_off, dtype=np.int64)
                counts = np.diff(kept_off)
                # the engine rejects empty utterances: those that keep nothing are not handed to it
                offsets = np.concatenate((kept_off[:1], kept_off[1:][counts > 0])).astype(np.int32)
                n = len(offsets) - 1
                if n == 0:
                    return None                              # nothing of this batch is kept: nothing is copied or launched, finish(k) gives None
            elif voiced is not None:
                raise ValueError("these buffer sets were made without flags (IngestOptions.flags)")
        e = self._next_engine                            # consecutive batches alternate between the engines (each on its own stream: in
        self._next_engine = (e + 1) % len(self.engines)  # order, so the status word copied behind a batch is that batch's alone)
        out = None
        if self.results == "device":
            # a block of the ENGINE stream's pool (the stream that writes it), marked as used by the consumer's stream too: the caching
            # allocator then hands it out again only after both streams have passed its last use (allocated on the caller's
            # stream, a block the collector thread had just freed there could be overwritten under a still-pending cat / index kernel)
            consumer = torch.cuda.current_stream(self.dev)
            with torch.cuda.stream(self.streams[e]):
                out = torch.empty((n, self.embed_dim), dtype=torch.float32, device=self.dev)
            if consumer != self.streams[e]:
                out.record_stream(consumer)
        import time
        t = [time.perf_counter()]
        with torch.cuda.device(self.dev), torch.cuda.stream(self.streams[e]):
            own = packed is None and isinstance(frames, np.ndarray)
            if isinstance(frames, torch.Tensor):         # (submit_windows: rows that are on the device already)
                feats = frames
            elif packed is not None:                     # compressed bodies: only the bytes used travel; the rows are decoded behind the copy
                self.dev_bytes[k][:packed[3]].copy_(self.host_bytes[k][:packed[3]], non_blocking=True)
                feats = (self.dev_in if self.ingest is None else self.dev_raw)[k][:frames]
            elif own:                                    # one utterance longer than a whole batch buffer: a pageable copy of its own
                feats = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.float32)).to(self.dev)
            else:
                feats = (self.dev_in if self.ingest is None else self.dev_raw)[k][:frames]
                feats.copy_(self.host_in[k][:frames], non_blocking=True)
            flags = None
            if self.ingest is not None and self.ingest.flags:
                rows = feats.shape[0]
                if own:
                    flags = torch.from_numpy(np.ascontiguousarray(voiced[:rows])).to(self.dev)
                else:
                    if voiced.ctypes.data != self.flags_np[k].ctypes.data:
                        self.flags_np[k][:rows] = voiced[:rows]
                    flags = self.dev_flags[k][:rows]
                    flags.copy_(self.host_flags[k][:rows], non_blocking=True)
            self.h2d[k].record()
            t.append(time.perf_counter())
            if packed is not None:
                self._decode(self.dev_bytes[k], packed[0], packed[1], packed[2], feats)
                t.append(time.perf_counter())
            if windows is not None:                      # raw parent rows -> one normalised utterance per window: what the engine (and a range re-run) reads
                feats = self._ingest_windows(feats, windows, self.dev_in[k])
                t.append(time.perf_counter())
            elif self.ingest is not None:                # raw rows -> normalised kept rows, compacted: what the engine (and a range re-run) reads
                feats = self._ingest(feats, raw_off, flags, kept_off, None if own else self.dev_in[k])
                t.append(time.perf_counter())
            if self.results == "host":
                out = self.dev_out[k][:n]
            self.engines[e].extract_device(feats, offsets, max_chunk=self.max_chunk, out=out)
            t.append(time.perf_counter())
            if self.results == "host":
                self.host_out[k][:n].copy_(out, non_blocking=True)
            if self.watch:
                self.engines[e].status_async(self.status_host[k])
            self.done[k].record()
            t.append(time.perf_counter())
        pieces = ("h2d",) + (("decode",) if packed is not None else ()) + (("ingest",) if self.ingest is not None else ()) + ("extract", "d2h")
        for i, name in enumerate(pieces):
            self.submit_seconds[name] = self.submit_seconds.get(name, 0.0) + t[i + 1] - t[i]
        self.submitted += 1
        self.pending[k] = (feats, np.array(offsets, dtype=np.int32), out, n, e, self.submitted)
        return out

    def final_through(self):
        """Every submission numbered <= this (1-based, in submit() order) has been finish()ed - synchronised, range-checked and, where
        flagged, re-run: its result may be read from any stream.  Exact whatever set each batch used (the sharded path releases a
        segment to the gather by it; a rule of "n_sets submissions later" only held while batches rotated over the sets)."""
        live = [p[5] for p in self.pending if p is not None]
        return (min(live) - 1) if live else self.submitted

    def input_consumed(self, k):
        if self.pending[k] is not None:
            self.h2d[k].synchronize()

    def finish(self, k):
        p = self.pending[k]
        if p is None:
            return None
        feats, offsets, out, n, e, _ = p
        self.done[k].synchronize()
        if self.watch and (int(self.status_host[k][0]) & capi.STATUS_HALF_RANGE):
            torch = self.torch
            warnings.warn("asv-subtools_amd: an activation left the IEEE-half range of the f32x mode's operand split (|x| > 65504 or NaN): "
                          "re-running the batch with bf16 operand halves (precision 'f32x-bf16')", RuntimeWarning)
            twin = self.engines[e].wide_range_twin()
            with torch.cuda.device(self.dev), torch.cuda.stream(self.streams[e]):
                twin.extract_device(feats, offsets, max_chunk=self.max_chunk, out=out)
                if self.results == "host":
                    self.host_out[k][:n].copy_(out, non_blocking=True)
                self.streams[e].synchronize()
            self.status_host[k].zero_()
            self.range_reruns += 1
        self.pending[k] = None
        return self.host_out[k][:n].numpy() if self.results == "host" else out

    def flush(self):
        """Finishes every batch in flight (results='device': afterwards every tensor submit() returned is final and safe to read
        from any stream)."""
        for k in range(self.n_sets):
            self.finish(k)
