"""asv_ingest_frames called from ONE thread on TWO streams with no synchronisation in between, as libs.amd.pipeline.DeviceSets calls it:
the library stages the host offsets per thread and reuses an unchanged upload, so a call on the second stream may read a slot whose
copy was queued on the first - behind work that has not run yet.  Every result has to equal the same call made alone."""

import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIM = 30
LENS = [[200] * 12, [100, 300, 200, 250, 150, 400, 1000], [2400], [37, 1, 0, 650, 299, 300, 301, 812]]      # four partitions of 2400 frames
OPTS = dict(cmn_window=300, center=True)


def test_two_streams_unchanged_then_changed_offsets_without_synchronisation():
    import torch
    from libs.amd import frontend, synth
    dev = torch.device("cuda", 0)
    total = 2400
    assert all(sum(l) == total for l in LENS)
    x = torch.from_numpy(synth.synth_feats(total, DIM, 77) * 3.0 + 1.5).to(dev)
    rng = np.random.RandomState(4)
    flag_sets = [(rng.rand(total) < p).astype(np.uint8) for p in (0.7, 0.4)]
    cases = []                                            # (frame offsets, device flags or None, kept offsets)
    for lens in LENS:
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        cases.append((off, None, off))
        for f in flag_sets:
            cases.append((off, torch.from_numpy(f).to(dev), frontend.kept_offsets(f, off)[1]))
    # every case alone, synchronised: what each call below has to reproduce bit for bit
    want = []
    for off, fl, kept_off in cases:
        want.append(frontend.ingest(x, off, voiced=fl, kept_off=kept_off, **OPTS)[0].clone())
    torch.cuda.synchronize(dev)
    # the order of calls: every case on stream A then at once on stream B (unchanged offsets, the other stream), the next case differs
    # (changed offsets) - 24 calls and 12 changes of the offsets, more than the library's staging slots, all queued while stream A is
    # still held up by a long-running kernel in front of its first call
    failures = []

    def calls():                                          # a thread of its own: the library's staging starts empty
        try:
            a, b = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
            outs = []
            with torch.cuda.device(dev):
                with torch.cuda.stream(a):
                    torch.cuda._sleep(20_000_000)         # a spinning kernel on stream A: its copies and kernels queue up behind it
                for k, (off, fl, kept_off) in enumerate(cases):
                    for s in ((a, b) if k % 2 == 0 else (b, a)):
                        out = torch.full((total, DIM), 7.0, dtype=torch.float32, device=dev)
                        s.wait_stream(torch.cuda.current_stream(dev))      # (the fill above ran on this thread's default stream)
                        with torch.cuda.stream(s):
                            got, _ = frontend.ingest(x, off, voiced=fl, kept_off=kept_off, out=out, **OPTS)
                        outs.append((k, got, out))
                a.synchronize()
                b.synchronize()
            for k, got, out in outs:
                if not torch.equal(got.view(torch.int32), want[k].view(torch.int32)) or not bool((out[got.shape[0]:] == 7.0).all()):
                    failures.append(k)
        except BaseException as e:
            failures.append(e)

    t = threading.Thread(target=calls)
    t.start()
    t.join()
    assert not failures, failures
