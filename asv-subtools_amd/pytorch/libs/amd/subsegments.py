# -*- coding:utf-8 -*-
"""Host rules of the reference's sliding (diarisation) extraction mode, pure Python:

    pytorch/pipeline/extract_xvectors_for_pytorch.sh --sliding true --window 1.5 --period 0.75 --min-segment 0.5 [--hard-min true]

cuts every segment of a data directory into uniform overlapping sub-segments (kaldi/utils/data/get_uniform_subsegments.py) and
extracts one embedding per sub-segment from a ROW RANGE of the segment's feature matrix (kaldi/utils/data/subsegment_data_dir.sh:
146-199 writes 'file:offset[first:last]' entries).  Here:

    uniform_subsegments()   the cut, line for line what the reference prints for the options of the shell script
    frame_ranges()          times -> inclusive row ranges (the awk rule of subsegment_data_dir.sh:195 + fix_subsegment_feats.pl)
    cut_spans()             which rows of which parents a buffer set of libs.amd.pipeline.DeviceSets holds for a batch of windows
"""

import collections
import warnings


def _fields(segment):
    if isinstance(segment, str):
        parts = segment.strip().split()
        return parts[0], parts[1], float(parts[2]), float(parts[3])
    utt, rec, start, end = segment
    return utt, rec, float(start), float(end)


def uniform_subsegments(segments, window=1.5, period=0.75, min_segment=0.5, constant_duration=True, hard_min=False):
    """`segments`: an iterable of (utt, rec, start, end) or of lines of a Kaldi segments file.  Returns [(new_utt, utt, start, end)]: the
    lines get_uniform_subsegments.py prints for --max-segment-duration=window --overlap-duration=(window - period as perl prints it)
    --max-remaining-duration=min_segment --constant-duration=<constant_duration>, in its order.  start / end are relative to the segment's
    start and are the floats the printed '%.3f' text parses back to (subsegment_data_dir.sh reads the text).  The id is
    '{utt}-{s:08d}-{e:08d}' in hundredths of a second: truncated inside the loop, rounded for the tail - the reference does both.
    hard_min: segments shorter than min_segment are dropped first (extract_xvectors_for_pytorch.sh:62-68)."""
    window, min_segment = float(window), float(min_segment)
    overlap = float("%.15g" % (window - float(period)))             # perl -e "print ($window-$period)" prints 15 significant digits
    shift = window - overlap
    threshold = window if constant_duration else window + min_segment
    out = []

    def emit(utt, s_id, e_id, s, e):
        out.append(("{0}-{1:08d}-{2:08d}".format(utt, s_id, e_id), utt, float("%.3f" % s), float("%.3f" % e)))

    for segment in segments:
        if isinstance(segment, str) and not segment.strip():
            continue
        utt, _, start_time, end_time = _fields(segment)
        if hard_min and not end_time - start_time >= min_segment:
            continue
        dur = end_time - start_time
        start = start_time
        while dur > threshold:
            end = start + window
            s_rel, e_rel = start - start_time, end - start_time
            emit(utt, int(100 * s_rel), int(100 * e_rel), s_rel, s_rel + window)
            start += shift
            dur -= shift
        if constant_duration:
            if dur < 0:
                continue
            if dur < min_segment:
                start = max(end_time - window, start_time)
            end = min(start + window, end_time)
        else:
            end = end_time
        emit(utt, int(round(100 * (start - start_time))), int(round(100 * (end - start_time))), start - start_time, end - start_time)
    return out


def format_subsegments(subsegments):
    """The lines of a Kaldi subsegments file: '<new-utt> <utt> <start> <end>' with three decimals."""
    return ["{0} {1} {2:.3f} {3:.3f}".format(*s) for s in subsegments]


def frame_ranges(subsegments, num_frames, frame_shift=0.01, warn=None):
    """Row ranges of sub-segments inside their parents' feature matrices.  `subsegments`: [(new_utt, utt, start, end)]; `num_frames`:
    rows of every parent by utt.  Returns (kept, first, last): the sub-segments that have rows, and their first and last row (inclusive)
    as lists.  first = int(start / shift + 0.5), last = int(end / shift - 0.5) in double arithmetic, truncated toward zero
    (subsegment_data_dir.sh:195); last is clipped to the parent's last row (fix_subsegment_feats.pl).  A sub-segment left with
    first > last is dropped with a warning - Kaldi fails when it reads such a range."""
    shift = float(frame_shift)
    kept, first, last = [], [], []
    for sub in subsegments:
        new_utt, utt, start, end = sub
        if utt not in num_frames:
            raise KeyError("sub-segment %s: no feature matrix for %s" % (new_utt, utt))
        a, b = int(float(start) / shift + 0.5), int(float(end) / shift - 0.5)
        b = min(b, int(num_frames[utt]) - 1)
        if a > b:
            line = "sub-segment %s of %s has no frames (rows %d:%d of %d): dropped" % (new_utt, utt, a, b, int(num_frames[utt]))
            if warn is not None:
                warn(line)
            else:
                warnings.warn(line, RuntimeWarning)
            continue
        kept.append(sub)
        first.append(a)
        last.append(b)
    return kept, first, last


# rows [row0, row1) of parent `parent` hold windows [w0, w1) (indices into the caller's window list), every one of them entirely
Span = collections.namedtuple("Span", "parent row0 row1 w0 w1")
# what one buffer set holds: spans one behind the other; own: ONE window longer than a whole buffer, in an array of its own; whole: every
# span is a parent from its first row to its last (what a compressed body decodes to)
SpanBatch = collections.namedtuple("SpanBatch", "spans own whole")


def cut_spans(parent_lengths, windows, batch_frames, batch_utts, whole=()):
    """Cuts a list of windows into batches for buffer sets of `batch_frames` rows / `batch_utts` utterances.  `windows`: [(parent, first
    row, rows)] in processing order - the windows of a parent one behind the other, in start order; `parent_lengths`: rows by parent
    (a sequence or a mapping).  A batch holds whole parents, or a SPAN of a long one: the rows from its first untaken window's start to
    the end of the last window taken.  A batch ends where the raw rows of its spans, the rows of its windows or the number of its
    windows would exceed the set.  Every window lies entirely inside exactly one span; order is kept.  A window longer than
    batch_frames is a batch of its own (own=True).  `whole`: parents (none longer than batch_frames) that are taken from their first
    row to their last wherever one of their windows is taken - a compressed body is decoded as a whole; a batch holds spans of such
    parents only, or of the others only."""
    batch_frames, batch_utts = int(batch_frames), int(batch_utts)
    if batch_frames < 1 or batch_utts < 1:
        raise ValueError("cut_spans: batch_frames and batch_utts must be positive")
    batches, spans = [], []
    raw = win_rows = n_win = 0
    kind = False

    def flush():
        batches.append(SpanBatch(list(spans), False, kind))
        del spans[:]
    i, n = 0, len(windows)
    while i < n:
        parent, start, rows = windows[i]
        if start < 0 or rows < 1 or start + rows > parent_lengths[parent]:
            raise ValueError("cut_spans: window %d (rows %d + %d) lies outside parent %r of %d rows" % (i, start, rows, parent, parent_lengths[parent]))
        if rows > batch_frames:
            if parent in whole:
                raise ValueError("cut_spans: parent %r is to be taken whole and is longer than a batch" % (parent,))
            if spans:
                flush()
                raw = win_rows = n_win = 0
            batches.append(SpanBatch([Span(parent, start, start + rows, i, i + 1)], True, False))
            i += 1
            continue
        entire = parent in whole
        if entire and parent_lengths[parent] > batch_frames:
            raise ValueError("cut_spans: parent %r is to be taken whole and is longer than a batch" % (parent,))
        if spans and kind != entire:
            flush()
            raw = win_rows = n_win = 0
        kind = entire
        row0, row1, j = (0, parent_lengths[parent], i) if entire else (start, start, i)
        while j < n and windows[j][0] == parent:
            _, a, r = windows[j]
            if a < row0:
                raise ValueError("cut_spans: the windows of parent %r are not in start order" % (parent,))
            if a < 0 or r < 1 or a + r > parent_lengths[parent]:
                raise ValueError("cut_spans: window %d (rows %d + %d) lies outside parent %r of %d rows" % (j, a, r, parent, parent_lengths[parent]))
            end = row1 if entire else max(row1, a + r)
            if r > batch_frames or raw + end - row0 > batch_frames or win_rows + r > batch_frames or n_win + 1 > batch_utts:
                break
            row1, win_rows, n_win, j = end, win_rows + r, n_win + 1, j + 1
        if j > i:
            spans.append(Span(parent, row0, row1, i, j))
            raw += row1 - row0
            i = j
            if j < n and windows[j][0] == parent and windows[j][2] <= batch_frames:
                flush()                                          # the parent goes on: its next window opens the next batch
                raw = win_rows = n_win = 0
        else:                                                    # not even this window fits behind what the batch holds already
            assert spans, "a window that fits a batch fits an empty one"
            flush()
            raw = win_rows = n_win = 0
    if spans:
        flush()
    return batches


def extract_sliding(model, feats, win_start, win_len, ingest=None, batch_frames=65536, batch_utts=1024, max_chunk=None):
    """One embedding per window of ONE parent matrix: `feats` [T, dim] float32 (numpy, or a CUDA tensor), window w = rows
    [win_start[w], win_start[w] + win_len[w]), each normalised as an utterance of its own (`ingest`: libs.amd.pipeline.IngestOptions,
    default sliding CMN over 300 frames, centred - the reference's).  The matrix is uploaded once; the windows go through
    DeviceSets.submit_windows in batches that read the resident rows.  Returns [n, E] float32 numpy, in the order of the windows."""
    import numpy as np
    import torch
    from .pipeline import DeviceSets, IngestOptions
    if ingest is None:
        ingest = IngestOptions(cmn_window=300)
    start, rows = np.ascontiguousarray(win_start, dtype=np.int64), np.ascontiguousarray(win_len, dtype=np.int64)
    if start.ndim != 1 or start.shape != rows.shape:
        raise ValueError("extract_sliding: one start and one length per window")
    if isinstance(feats, torch.Tensor) and feats.is_cuda:
        parent = feats.contiguous().float()
    else:
        host = feats.numpy() if isinstance(feats, torch.Tensor) else feats
        parent = torch.from_numpy(np.ascontiguousarray(host, dtype=np.float32)).to(torch.device("cuda", model._amd_engine().device_index))
    if parent.dim() != 2:
        raise ValueError("extract_sliding: feats must be one [T, dim] matrix")
    if len(start) and ((start < 0).any() or (rows < 1).any() or (start + rows > parent.shape[0]).any()):
        raise ValueError("extract_sliding: a window is empty or lies outside the %d rows of feats" % parent.shape[0])
    if max_chunk is None:
        max_chunk = getattr(type(model).extract_embedding, "max_chunk", 10000)
    if len(start) == 0:
        return np.zeros((0, model._amd_engine().embed_dim), dtype=np.float32)
    batch_frames = max(int(batch_frames), int(rows.max()))
    sets = DeviceSets(model, batch_frames, batch_utts, parent.shape[1], max_chunk, n_sets=2, results="host", ingest=ingest, windows=True)
    torch.cuda.current_stream(parent.device).synchronize()           # the engines' streams read the parent: its upload has finished
    out, held, k, i = [], None, 0, 0
    while i < len(start):
        j, used = i, 0
        while j < len(start) and j - i < batch_utts and used + int(rows[j]) <= batch_frames:
            used += int(rows[j])
            j += 1
        sets.submit_windows(k, parent, start[i:j], rows[i:j])
        if held is not None:
            out.append(sets.finish(held).copy())
        held, k, i = k, (k + 1) % sets.n_sets, j
    out.append(sets.finish(held).copy())
    return np.concatenate(out, axis=0)
