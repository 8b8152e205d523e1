"""Host side of the sliding (diarisation) extraction mode: the sub-segment rules of libs.amd.subsegments against what the reference's own
get_uniform_subsegments.py printed (tests/golden/subsegments.npz, written by tests/gen_subsegments_golden.py), the frame rule, the span
cutter and the script's refusals.  No GPU."""

import importlib.util
import os
import warnings

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_script():
    spec = importlib.util.spec_from_file_location("extract_embeddings_sliding", os.path.join(REPO, "asv-subtools_amd", "pytorch", "pipeline", "onestep",
                                                                                            "extract_embeddings.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(REPO, "tests", "golden", "subsegments.npz"))
    return {k: g[k] for k in g.files}


# ----------------------------------------------------------------------------------------------------------------------------------
def test_the_fixture_holds_the_cases_it_is_meant_to(golden):
    segs = [str(s).split() for s in golden["segments"]]
    assert 30 <= len(segs) <= 40
    starts = {s[2] for s in segs}
    assert {"0.07", "0.29", "10.5"} <= starts
    durs = sorted(round(float(s[3]) - float(s[2]), 2) for s in segs)
    for want in (0.3, 1.5, 1.51, 1.99, 2.01, 4.1, 600.0):
        assert want in durs, want
    assert [tuple(o) for o in golden["option_sets"]] == [(1.5, 0.75, 0.5, 1.0), (3.0, 1.0, 0.5, 1.0), (1.5, 0.75, 0.5, 0.0)]
    assert all(len(golden["lines_%d" % k]) > 600 for k in range(3))


@pytest.mark.parametrize("k", range(3))
def test_uniform_subsegments_reproduces_every_line_of_the_reference(golden, k):
    from libs.amd import subsegments
    window, period, min_segment, constant = golden["option_sets"][k]
    lines = [str(s) for s in golden["segments"]]
    want = [str(s) for s in golden["lines_%d" % k]]
    got = subsegments.uniform_subsegments(lines, window, period, min_segment, constant_duration=bool(constant))
    assert subsegments.format_subsegments(got) == want
    # tuples in, the same out; the times are the floats the printed text parses back to
    tuples = [(p[0], p[1], float(p[2]), float(p[3])) for p in (line.split() for line in lines)]
    assert subsegments.uniform_subsegments(tuples, window, period, min_segment, constant_duration=bool(constant)) == got
    for (new_utt, utt, start, end), line in zip(got, want):
        f = line.split()
        assert (new_utt, utt) == (f[0], f[1]) and start == float(f[2]) and end == float(f[3])


def test_the_defaults_are_the_shell_scripts(golden):
    from libs.amd import subsegments
    lines = [str(s) for s in golden["segments"]]
    assert subsegments.format_subsegments(subsegments.uniform_subsegments(lines)) == [str(s) for s in golden["lines_0"]]


def test_hard_min_drops_short_segments_first():
    from libs.amd import subsegments
    segs = [("a", "r", 0.0, 0.49), ("b", "r", 1.0, 1.5), ("c", "r", 0.29, 0.78), ("d", "r", 2.0, 4.0)]
    soft = subsegments.uniform_subsegments(segs)
    assert [s[1] for s in soft] == ["a", "b", "c", "d", "d"]                   # a short segment is one short sub-segment
    hard = subsegments.uniform_subsegments(segs, hard_min=True)
    # awk's `$4 - $3 >= min` in double arithmetic: 1.5 - 1.0 is 0.5 and stays; 0.78 - 0.29 is 0.49 and goes, as 0.49 - 0.0 does
    assert [s[1] for s in hard] == ["b", "d", "d"]
    assert hard == [s for s in soft if s[1] in ("b", "d")]
    assert subsegments.uniform_subsegments(segs, min_segment=0.3, hard_min=True) == subsegments.uniform_subsegments(segs, min_segment=0.3)


def test_frame_ranges_on_hand_computed_cases():
    """first = int(start / shift + 0.5), last = int(end / shift - 0.5), last clipped to the parent's last row.  This restates the awk line
    of kaldi/utils/data/subsegment_data_dir.sh:195 and fix_subsegment_feats.pl: the Kaldi binaries that script needs
    (feat-to-len for utt2num_frames among them) are not available here, so the rule is checked against cases worked out by hand, the
    example of the script's own comment first."""
    from libs.amd import subsegments
    subs = [("u-1", "u", 0.0, 0.01),          # the script's comment: one frame, [0:0]
            ("u-2", "u", 0.0, 1.5),           # a 1.5 s window at 10 ms: rows 0 ... 149
            ("u-3", "u", 0.75, 2.25),         # 75 ... 224
            ("u-4", "u", 7.21, 8.93),         # the script's other example: 721 ... 892
            ("u-5", "u", 8.5, 10.0),          # 850 ... 999 - the parent has 990 rows: clipped to 989
            ("v-1", "v", 0.0, 0.4),
            ("v-2", "v", 0.004, 0.006)]       # int(0.9) = 0, int(0.1) = 0
    kept, first, last = subsegments.frame_ranges(subs, {"u": 990, "v": 40})
    assert kept == subs
    assert list(zip(first, last)) == [(0, 0), (0, 149), (75, 224), (721, 892), (850, 989), (0, 39), (0, 0)]
    assert last[1] - first[1] + 1 == 150
    # another frame shift: 1.5 s at 20 ms is 75 rows
    _, first, last = subsegments.frame_ranges([("u-2", "u", 0.0, 1.5)], {"u": 990}, frame_shift=0.02)
    assert (first, last) == ([0], [74])
    with pytest.raises(KeyError):
        subsegments.frame_ranges([("w-1", "w", 0.0, 1.0)], {"u": 990})


def test_frame_ranges_drops_a_sub_segment_without_rows():
    from libs.amd import subsegments
    subs = [("u-1", "u", 0.0, 1.5), ("u-2", "u", 9.95, 11.45), ("u-3", "u", 0.75, 2.25)]      # u-2 starts behind the parent's last row
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        kept, first, last = subsegments.frame_ranges(subs, {"u": 990})
    assert kept == [subs[0], subs[2]] and first == [0, 75] and last == [149, 224]
    assert len(w) == 1 and "u-2" in str(w[0].message)
    said = []
    kept, _, _ = subsegments.frame_ranges(subs, {"u": 990}, warn=said.append)
    assert len(kept) == 2 and len(said) == 1 and "u-2" in said[0]


# ----------------------------------------------------------------------------------------------------------------------------------
def check_cut(lengths, windows, batch_frames, batch_utts, whole=()):
    """The properties every cut has to have; returns the batches."""
    from libs.amd import subsegments
    batches = subsegments.cut_spans(lengths, windows, batch_frames, batch_utts, whole=whole)
    seen = []
    for batch in batches:
        assert batch.spans
        taken = [j for span in batch.spans for j in range(span.w0, span.w1)]
        seen += taken
        for span in batch.spans:
            assert span.w1 > span.w0 and 0 <= span.row0 < span.row1 <= lengths[span.parent]
            for j in range(span.w0, span.w1):                                   # every window lies entirely inside its span
                parent, a, n = windows[j]
                assert parent == span.parent and span.row0 <= a and a + n <= span.row1
            if batch.whole:
                assert span.parent in whole and (span.row0, span.row1) == (0, lengths[span.parent])
            else:
                assert span.parent not in whole
                assert span.row0 == windows[span.w0][1]                         # from the first window's start ...
                assert span.row1 == max(windows[j][1] + windows[j][2] for j in range(span.w0, span.w1))      # ... to the end of the last taken
        if batch.own:
            assert len(batch.spans) == 1 and len(taken) == 1 and windows[taken[0]][2] > batch_frames
        else:
            assert sum(span.row1 - span.row0 for span in batch.spans) <= batch_frames
            assert sum(windows[j][2] for j in taken) <= batch_frames and len(taken) <= batch_utts
    assert seen == list(range(len(windows)))                                    # every window exactly once, in order
    return batches


def sliding(parent, rows, window=150, period=75):
    out = [(parent, a, window) for a in range(0, rows - window + 1, period)]
    if not out or out[-1][1] + window < rows:
        out.append((parent, max(rows - window, 0), min(window, rows)))
    return out


def test_span_cutter_takes_whole_parents_where_they_fit():
    lengths = [40, 333, 700]
    windows = sliding(0, 40) + sliding(1, 333) + sliding(2, 700)
    batches = check_cut(lengths, windows, 65536, 1024)
    assert len(batches) == 1 and [(s.parent, s.row0, s.row1) for s in batches[0].spans] == [(0, 0, 40), (1, 0, 333), (2, 0, 700)]


def test_span_cutter_cuts_a_parent_longer_than_the_buffer():
    lengths = [40, 333, 700]
    windows = sliding(0, 40) + sliding(1, 333) + sliding(2, 700)
    batches = check_cut(lengths, windows, 256, 1024)
    assert sum(1 for b in batches for s in b.spans if s.parent == 2) >= 4       # 700 rows through 256-row sets
    assert not any(b.own for b in batches)
    # the window count ends a batch too
    batches = check_cut(lengths, windows, 65536, 4)
    assert max(sum(s.w1 - s.w0 for s in b.spans) for b in batches) == 4 and len(batches) == -(-len(windows) // 4)
    # ... and so do the windows' rows: two parents fit raw, their windows do not
    batches = check_cut([300, 300], sliding(0, 300, 150, 10) + sliding(1, 300, 150, 10), 1000, 1024)
    assert len(batches) > 1


def test_span_cutter_a_window_longer_than_the_buffer_is_a_batch_of_its_own():
    lengths = [100, 900, 100]
    windows = [(0, 0, 100), (1, 0, 150), (1, 100, 600), (1, 650, 150), (2, 0, 100)]
    batches = check_cut(lengths, windows, 256, 16)
    own = [b for b in batches if b.own]
    assert len(own) == 1 and own[0].spans[0] == (1, 100, 700, 2, 3)


def test_span_cutter_whole_parents_are_batches_of_their_own_kind():
    lengths = [200, 500, 200, 120]
    windows = sliding(0, 200) + sliding(1, 500) + sliding(2, 200) + sliding(3, 120)
    batches = check_cut(lengths, windows, 1024, 1024, whole={1, 3})
    assert [b.whole for b in batches] == [False, True, False, True]
    # a whole parent whose windows take two batches is taken whole twice
    batches = check_cut(lengths, windows, 1024, 3, whole={1})
    assert sum(1 for b in batches for s in b.spans if s.parent == 1) == 2
    from libs.amd import subsegments
    with pytest.raises(ValueError):
        subsegments.cut_spans(lengths, windows, 256, 1024, whole={1})           # 500 rows cannot be taken whole by 256-row sets
    with pytest.raises(ValueError):
        subsegments.cut_spans(lengths, [(0, 100, 150)], 256, 16)                # beyond the parent
    with pytest.raises(ValueError):
        subsegments.cut_spans(lengths, [(0, 50, 100), (0, 0, 100)], 256, 16)    # not in start order


def test_span_cutter_on_random_tables():
    rng = np.random.RandomState(2)
    for _ in range(30):
        lengths = rng.randint(1, 900, size=rng.randint(1, 6)).tolist()
        windows = []
        for p, rows in enumerate(lengths):
            starts = np.sort(rng.randint(0, rows, size=rng.randint(0, 12)))
            windows += [(p, int(a), int(rng.randint(1, rows - a + 1))) for a in starts]
        if windows:
            check_cut(lengths, windows, int(rng.randint(64, 700)), int(rng.randint(1, 9)))


# ----------------------------------------------------------------------------------------------------------------------------------
def test_the_new_options_default_to_off():
    script = load_script()
    args = script.get_args(["m", "scp:feats.scp", "ark:out.ark"])
    assert (args.sliding, args.segments, args.window, args.period, args.min_segment, args.hard_min, args.frame_shift, args.subsegments_out) == \
        ("false", "", 1.5, 0.75, 0.5, "false", 0.01, "")
    assert script.sliding_options(args) is None and script.ingest_options(args) is None
    args = script.get_args(["--sliding", "true", "--segments", "seg", "--hard-min", "true", "--window", "3", "--period", "1", "m", "scp,p:feats.scp", "ark:out.ark"])
    assert script.sliding_options(args) == ("seg", 3.0, 1.0, 0.5, True, 0.01, "")


@pytest.mark.parametrize("argv, word", [
    (["--sliding", "true", "--segments", "seg", "--sharded", "true", "m", "scp:feats.scp", "ark:o"], "--sharded"),
    (["--sliding", "true", "--segments", "seg", "--vad-scp", "vad.scp", "m", "scp:feats.scp", "ark:o"], "--vad-scp"),
    (["--sliding", "true", "--segments", "seg", "m", "ark:feats.ark", "ark:o"], "scp:"),
    (["--sliding", "true", "--segments", "seg", "m", "ark:cat feats.ark |", "ark:o"], "scp:"),
    (["--sliding", "true", "m", "scp:feats.scp", "ark:o"], "--segments"),
])
def test_what_the_sliding_mode_does_not_take_is_refused(argv, word):
    script = load_script()
    with pytest.raises(ValueError) as e:
        script.sliding_options(script.get_args(argv))
    assert word in str(e.value)


def test_a_parent_that_carries_a_range_is_refused(tmp_path):
    script = load_script()
    script.refuse_ranged_entries([("a", "feats.ark:17"), ("b", "gunzip -c feats.gz |")])
    for rx in ("feats.ark:17[0:99]", "feats.ark:17[0:99,0:22]", "gunzip -c feats.gz |[3:7]"):
        with pytest.raises(ValueError) as e:
            script.refuse_ranged_entries([("a", "feats.ark:5"), ("b", rx)])
        assert "range" in str(e.value) and "'b'" in str(e.value)
    # ... through the table the script parses
    scp = tmp_path / "feats.scp"
    scp.write_text("a feats.ark:5\nb feats.ark:17[0:99]\n")
    with pytest.raises(ValueError):
        script.refuse_ranged_entries(script.read_scp("scp:%s" % scp))


def test_sliding_windows_of_a_table(tmp_path):
    """The windows of a run from a segments file and the parents' row counts: parents in scp order, each one's windows in start order."""
    script = load_script()
    seg = tmp_path / "segments"
    seg.write_text("p2 r 0.0 7.0\np0 r 0.0 0.4\np2 r 10.0 13.3\n")
    entries = [("p0", "x.ark:5"), ("p1", "x.ark:999"), ("p2", "x.ark:9999")]
    opts = script.SlidingOptions(str(seg), 1.5, 0.75, 0.5, False, 0.01, "")
    ids, windows, subs = script.sliding_windows(entries, [40, 333, 700], opts)
    assert ids[0] == "p0-00000000-00000040" and windows[0] == (0, 0, 40)
    assert [w[0] for w in windows] == [0] + [2] * 13 and len(subs) == 14
    assert [w[1] for w in windows[1:]] == sorted(w[1] for w in windows[1:]) and windows[1][1:] == (0, 150) and windows[2][1:] == (0, 150)
    assert ids[1] == ids[2] == "p2-00000000-00000150" and windows[-1] == (2, 600, 100)      # (the remainder of 1.0 s is no shorter than min_segment: it stays a window of its own)
    with pytest.raises(ValueError):
        seg.write_text("nobody r 0.0 7.0\n")
        script.sliding_windows(entries, [40, 333, 700], opts)


def test_fill_rows_reads_spans_of_direct_and_other_entries(tmp_path):
    """ScpBatchLoader.fill_rows: rows [row0, row1) of a parent straight from a float32 entry, and from the ONE host decode of every other kind."""
    import compressed_cases as cc
    script = load_script()
    rng = np.random.RandomState(4)
    plain = rng.randn(300, 7).astype(np.float32)
    body = cc.cm_body(rng, 280, 7)
    double = rng.randn(90, 7)
    lines = cc.write_ark(str(tmp_path / "feats.ark"), [("a", cc.float_payload(plain)), ("b", cc.compressed_payload(1, body)), ("c", cc.float_payload(double))])
    (tmp_path / "feats.scp").write_text("\n".join(lines) + "\n")
    entries = script.read_scp("scp:%s" % (tmp_path / "feats.scp"))
    loader = script.ScpBatchLoader(entries, threads=2)
    decodes = []
    plain_call = script.ScpBatchLoader.__call__
    try:
        script.ScpBatchLoader.__call__ = lambda self, i: (decodes.append(i), plain_call(self, i))[1]
        loader.index_all()
        out = np.full((400, 7), -1.0, dtype=np.float32)
        loader.fill_rows([(0, 100, 250, 0), (1, 10, 110, 150), (1, 100, 200, 250), (2, 0, 50, 350)], out)
        assert decodes == [1, 2]                                                # the compressed parent once for its two spans; the float32 one never
    finally:
        script.ScpBatchLoader.__call__ = plain_call
        loader.close()
    cm = cc.host_decode(1, body)
    assert np.array_equal(out[:150], plain[100:250]) and np.array_equal(out[150:250], cm[10:110]) and np.array_equal(out[250:350], cm[100:200])
    assert np.array_equal(out[350:], double[:50].astype(np.float32))
    with pytest.raises(Exception):
        loader2 = script.ScpBatchLoader(entries, threads=2)
        try:
            loader2.fill_rows([(2, 0, 91, 0)], out)                             # beyond the parent's rows
        finally:
            loader2.close()
