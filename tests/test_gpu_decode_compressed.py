"""asv_decode_compressed (csrc/kernels_decode.hip) through libs.amd.frontend.decode_compressed against the host reader
(libs.support.kaldi_io.read_mat) on the same bytes: equal by uint32 view, no tolerance - the decode is sequential float32 arithmetic on
both sides (an FMA or a multiplication by a rounded 1 / 63 in the kernel shows here as last-bit differences in half / 7 % of the values)."""

import threading

import numpy as np
import pytest

import compressed_cases as cc

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC0BEEF                                 # the canary rows around `out`: a NaN pattern no decode produces
MARGIN = 4                                            # canary rows before and after `out`
BYTE_MARGIN = 256                                     # canary bytes before and after the bodies


def decode(batch, dim, byte_margin=0, fill=0xA5):
    """batch: (format, body) per utterance -> (the decoded rows as a CUDA tensor, the whole `out` allocation with its canary rows, frame
    offsets, the byte tensor as the kernel saw it, the bytes as they were before)."""
    import torch
    from libs.amd import frontend
    dev = torch.device("cuda", 0)
    host, byte_off = cc.pack([b for _, b in batch], front=byte_margin, back=byte_margin, fill=fill)
    rows = [np.frombuffer(b[8:12], dtype="<i4")[0] for _, b in batch]
    frame_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    total = int(frame_off[-1])
    whole = torch.from_numpy(np.full((total + 2 * MARGIN, dim), NAN_BITS, dtype=np.uint32).view(np.float32)).to(dev)
    d_bytes = torch.from_numpy(host).to(dev)
    got = frontend.decode_compressed(d_bytes[byte_margin:], byte_off - byte_margin, frame_off, np.array([f for f, _ in batch], dtype=np.uint8), dim,
                                     out=whole[MARGIN:MARGIN + total])
    torch.cuda.synchronize(dev)
    return got, whole, frame_off, d_bytes, host


def check_exact(batch, dim, got, frame_off):
    g = got.cpu().numpy()
    for k, (fmt, body) in enumerate(batch):
        want = cc.host_decode(fmt, body)
        have = g[int(frame_off[k]):int(frame_off[k + 1])]
        assert have.shape == want.shape
        diff = have.view(np.uint32) != want.view(np.uint32)
        assert not diff.any(), "utterance %d (format %d, %d x %d): %d of %d values differ, first at %s: %r against %r" % (
            k, fmt, want.shape[0], dim, int(diff.sum()), diff.size, np.argwhere(diff)[0].tolist(), have[diff][0], want[diff][0])


def check_margins(whole, total, d_bytes, host):
    w = whole.cpu().numpy().view(np.uint32)
    assert (w[:MARGIN] == NAN_BITS).all() and (w[MARGIN + total:] == NAN_BITS).all(), "rows outside `out` were written"
    assert np.array_equal(d_bytes.cpu().numpy(), host), "the input bytes were written"


@pytest.mark.parametrize("dim", [1, 23, 64, 65, 80])
@pytest.mark.parametrize("rows", [1, 3, 63, 64, 65, 257])
def test_cm_one_matrix_is_exact(rows, dim):
    rng = np.random.RandomState(1000 * rows + dim)
    batch = [(1, cc.cm_body(rng, rows, dim))]
    if rows == 257:                                    # every byte value in every column: all three segments of the quantiser and their ends
        data = np.frombuffer(batch[0][1][16 + 8 * dim:], dtype=np.uint8).reshape(dim, rows)
        assert all(len(set(col.tolist())) == 256 for col in data)
    got, whole, frame_off, d_bytes, host = decode(batch, dim)
    check_exact(batch, dim, got, frame_off)
    check_margins(whole, rows, d_bytes, host)


RAGGED = [200, 1, 65, 129, 64, 3, 257, 90]            # 8 utterances: column starts of every residue mod 4, tile remainders of every kind


def ragged_batch(dim=23, seed=11):
    rng = np.random.RandomState(seed)
    return [(1, cc.cm_body(rng, T, dim)) for T in RAGGED]


def mixed_batch(dim=80, seed=12):
    rng = np.random.RandomState(seed)
    return [(f, cc.BODY[f](rng, T, dim)) for f, T in ((1, 70), (2, 37), (3, 130), (1, 5), (3, 1), (2, 129), (1, 257))]


def test_cm_ragged_batch_is_exact():
    batch = ragged_batch()
    residues = {(16 + 8 * 23 + c * T) % 4 for T in RAGGED for c in range(23)}
    assert residues == {0, 1, 2, 3}
    got, _, frame_off, _, _ = decode(batch, 23)
    check_exact(batch, 23, got, frame_off)


@pytest.mark.parametrize("name,gmin,grange,pct", [
    ("equal percentiles", -3.25, 17.0, (31000, 31000, 31000, 31000)),
    ("0/0/65535/65535", -3.25, 17.0, (0, 0, 65535, 65535)),
    ("range 0", 4.75, 0.0, None),
    ("negative min", -1234.5, 77.7, None),
    ("large magnitude", -9876.543, 1.2345e4, None),
    ("large min, small range", 1.0e4, 0.37, None),
])
def test_cm_degenerate_headers_are_exact(name, gmin, grange, pct):
    rng = np.random.RandomState(5)
    batch = [(1, cc.cm_body(rng, 257, 23, gmin, grange, percentiles=pct)), (1, cc.cm_body(rng, 66, 23, gmin, grange, percentiles=pct))]
    got, _, frame_off, _, _ = decode(batch, 23)
    check_exact(batch, 23, got, frame_off)


@pytest.mark.parametrize("fmt", [2, 3])
@pytest.mark.parametrize("rows,dim", [(37, 23), (130, 80)])
def test_cm2_cm3_are_exact(fmt, rows, dim):
    rng = np.random.RandomState(100 * fmt + rows)
    batch = [(fmt, cc.BODY[fmt](rng, rows, dim)), (fmt, cc.BODY[fmt](rng, rows, dim, -9876.543, 1.2345e4))]
    got, whole, frame_off, d_bytes, host = decode(batch, dim)
    check_exact(batch, dim, got, frame_off)
    check_margins(whole, 2 * rows, d_bytes, host)


def test_mixed_formats_in_one_batch_are_exact():
    batch = mixed_batch()
    got, _, frame_off, _, _ = decode(batch, 80)
    check_exact(batch, 80, got, frame_off)


@pytest.mark.parametrize("which", ["ragged", "mixed"])
def test_bounds_canaries_and_utterances_alone(which):
    """Nothing outside `out` and nothing of `bytes` is written, and an utterance decoded alone equals its rows of the batch decode (no
    tile of one utterance reaches into a neighbour, whatever the gap bytes between the bodies hold)."""
    batch, dim = (ragged_batch(), 23) if which == "ragged" else (mixed_batch(), 80)
    got, whole, frame_off, d_bytes, host = decode(batch, dim, byte_margin=BYTE_MARGIN)
    check_exact(batch, dim, got, frame_off)
    check_margins(whole, int(frame_off[-1]), d_bytes, host)
    together = got.cpu().numpy().view(np.uint32)
    for k, item in enumerate(batch):
        alone, whole1, off1, b1, h1 = decode([item], dim, byte_margin=BYTE_MARGIN, fill=0x3C)
        check_margins(whole1, int(off1[-1]), b1, h1)
        assert np.array_equal(alone.cpu().numpy().view(np.uint32), together[int(frame_off[k]):int(frame_off[k + 1])]), k


def test_two_streams_changing_offsets_without_synchronisation():
    """One thread, two streams, no synchronisation in between, the offsets alternating between two shapes (unchanged offsets on the other
    stream, then changed ones: more changes than the library has staging slots) - as DeviceSets calls it, and as
    tests/test_gpu_ingest_streams.py asks of asv_ingest_frames, whose offset staging this entry point shares."""
    import torch
    from libs.amd import frontend
    dev = torch.device("cuda", 0)
    dim = 23
    shapes = [[(1, 200), (1, 65), (3, 64), (2, 31)], [(1, 3), (2, 129), (1, 257), (3, 7), (1, 90)]]
    cases, rng = [], np.random.RandomState(21)
    for r in range(6):
        batch = [(f, cc.BODY[f](rng, T, dim)) for f, T in shapes[r % 2]]
        host, byte_off = cc.pack([b for _, b in batch])
        frame_off = np.concatenate([[0], np.cumsum([T for _, T in shapes[r % 2]])]).astype(np.int64)
        want = np.concatenate([cc.host_decode(f, b) for f, b in batch])
        cases.append((torch.from_numpy(host).to(dev), byte_off, frame_off, np.array([f for f, _ in batch], dtype=np.uint8), want))
    torch.cuda.synchronize(dev)
    failures = []

    def calls():                                          # a thread of its own: the library's staging starts empty
        try:
            a, b = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
            outs = []
            with torch.cuda.device(dev):
                with torch.cuda.stream(a):
                    torch.cuda._sleep(20_000_000)         # a spinning kernel on stream A: its copies and kernels queue up behind it
                for rep in range(2):
                    for k, (d_bytes, byte_off, frame_off, formats, want) in enumerate(cases):
                        for s in ((a, b) if k % 2 == 0 else (b, a)):
                            out = torch.full((want.shape[0] + 2, dim), 7.0, dtype=torch.float32, device=dev)
                            s.wait_stream(torch.cuda.current_stream(dev))      # (the fill above ran on this thread's default stream)
                            with torch.cuda.stream(s):
                                got = frontend.decode_compressed(d_bytes, byte_off, frame_off, formats, dim, out=out)
                            outs.append((k, got, out))
                a.synchronize()
                b.synchronize()
            for j, (k, got, out) in enumerate(outs):
                if not np.array_equal(got.cpu().numpy().view(np.uint32), cases[k][4].view(np.uint32)) or not bool((out[got.shape[0]:] == 7.0).all()):
                    failures.append((j, k))
        except BaseException as e:
            failures.append(e)

    t = threading.Thread(target=calls)
    t.start()
    t.join()
    assert not failures, failures
