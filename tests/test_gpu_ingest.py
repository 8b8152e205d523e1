"""asv_ingest_frames (csrc/kernels_ingest.hip) through libs.amd.frontend.ingest: sliding-window CMN over the raw frames and
voiced-frame selection in one launch, against the float64 restatement of Kaldi's window rule (oracle/fbank_oracle.py sliding_cmn - the
yardstick asv_cmvn_sliding is held to, same inputs and the same 2e-5) and, bit for bit, against the launches it replaces."""

import functools

import numpy as np
import pytest

from oracle import fbank_oracle

pytestmark = pytest.mark.gpu

LENS = [650, 299, 300, 301, 1, 37, 0, 1200]
DIMS = [23, 30, 80]                                     # a partial column block, a partial column block, two blocks
OPTS = [dict(cmn_window=300, center=True),
        dict(cmn_window=600, min_window=100, center=False),                     # apply-cmvn-sliding's own defaults
        dict(cmn_window=100, min_window=20, center=False, norm_vars=True),
        dict(cmn_window=64, center=True, norm_vars=True)]
OFF = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def mats(dim):
    from libs.amd import synth
    return tuple(synth.synth_feats(T, dim, 40 + i) * 3.0 + 1.5 for i, T in enumerate(LENS))


@functools.lru_cache(maxsize=None)
def flags():
    """Per utterance, in turn: Bernoulli(0.6), all ones, all zeros, only the last frame, alternating, all ones for the rest."""
    rng = np.random.RandomState(11)
    out = []
    for i, T in enumerate(LENS):
        if i == 0:
            f = rng.rand(T) < 0.6
        elif i == 2:
            f = np.zeros(T, dtype=bool)
        elif i == 3:
            f = np.arange(T) == T - 1
        elif i == 4:
            f = (np.arange(T) + 1) % 2 == 1
        else:
            f = np.ones(T, dtype=bool)
        out.append(f.astype(np.uint8))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def restated(dim, k):
    """The float64 restatement of every utterance (all raw frames), computed once per (dim, option set)."""
    return tuple(fbank_oracle.sliding_cmn(m, **OPTS[k]) if len(m) else m for m in mats(dim))


def packed(dim):
    import torch
    return torch.from_numpy(np.concatenate(mats(dim), axis=0)).cuda()


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("k", range(len(OPTS)))
def test_cmn_then_selection_matches_the_restatement(dim, k):
    import torch
    from libs.amd import frontend
    fl = np.concatenate(flags())
    counts = [int(f.sum()) for f in flags()]
    x = packed(dim)
    for voiced in (fl, torch.from_numpy(fl).cuda()):                          # host flags (counts on the host) and device flags (one small D2H)
        before = x.clone()
        kept, kept_off = frontend.ingest(x, OFF, voiced=voiced, **OPTS[k])
        assert list(np.diff(kept_off)) == counts and kept_off[0] == 0 and kept.shape == (sum(counts), dim)
        assert torch.equal(x, before)                                          # the input is read only
        got = kept.cpu().numpy()
        for i, (want, f) in enumerate(zip(restated(dim, k), flags())):
            if counts[i]:
                err = np.abs(got[kept_off[i]:kept_off[i + 1]] - want[f > 0]).max()
                assert err < 2e-5, (OPTS[k], dim, LENS[i], err)


@pytest.mark.parametrize("dim", DIMS)
def test_selection_alone_copies_rows_bit_for_bit(dim):
    from libs.amd import frontend
    fl = np.concatenate(flags())
    x = packed(dim)
    kept, kept_off = frontend.ingest(x, OFF, voiced=fl, cmn_window=0)
    host = np.concatenate(mats(dim), axis=0)
    assert np.array_equal(kept.cpu().numpy().view(np.uint32), host[fl > 0].view(np.uint32))
    assert list(np.diff(kept_off)) == [int(f.sum()) for f in flags()]
    # ... and equals the existing two-launch selection
    import torch
    old, old_off = frontend.select_voiced(x, torch.from_numpy(fl).cuda(), OFF, np.diff(kept_off))
    assert torch.equal(old, kept) and np.array_equal(old_off, kept_off)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("k", range(len(OPTS)))
def test_without_flags_equals_cmvn_sliding_bit_for_bit(dim, k):
    import torch
    from libs.amd import frontend
    x = packed(dim)
    got, off = frontend.ingest(x, OFF, voiced=None, **OPTS[k])
    assert np.array_equal(off, OFF) and got.shape == x.shape
    want = frontend.cmvn_sliding(x, OFF, **{"min_window": 100, **OPTS[k]})
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (OPTS[k], dim)
    # ... so cmvn_sliding + select_voiced (the launches this replaces) give the fused result's bits too
    fl = np.concatenate(flags())
    fused, kept_off = frontend.ingest(x, OFF, voiced=fl, **OPTS[k])
    composed, _ = frontend.select_voiced(want, torch.from_numpy(fl).cuda(), OFF, np.diff(kept_off))
    assert torch.equal(fused.view(torch.int32), composed.view(torch.int32)), (OPTS[k], dim)


@pytest.mark.parametrize("dim", [30, 80])
def test_an_utterance_does_not_depend_on_its_neighbours(dim):
    import torch
    from libs.amd import frontend
    fl = flags()
    x = packed(dim)
    whole, kept_off = frontend.ingest(x, OFF, voiced=np.concatenate(fl), **OPTS[0])
    for i in (0, 3, 7):                                                        # first, middle, last (1200 frames: ten workgroups)
        alone = torch.from_numpy(mats(dim)[i]).cuda()
        got, off1 = frontend.ingest(alone, [0, LENS[i]], voiced=fl[i], **OPTS[0])
        assert off1[-1] == kept_off[i + 1] - kept_off[i]
        assert torch.equal(got.view(torch.int32), whole[kept_off[i]:kept_off[i + 1]].view(torch.int32)), (dim, i)


def test_output_buffer_and_handed_in_offsets():
    """`out=` (the pipeline's preallocated buffer: rows beyond the kept ones stay untouched) and `kept_off=` (counts the caller has)."""
    import torch
    from libs.amd import frontend
    fl = np.concatenate(flags())
    x = packed(30)
    ref, kept_off = frontend.ingest(x, OFF, voiced=fl, **OPTS[0])
    out = torch.full((x.shape[0] + 5, 30), 7.0, dtype=torch.float32, device=x.device)
    got, off2 = frontend.ingest(x, OFF, voiced=torch.from_numpy(fl).cuda(), out=out, kept_off=kept_off, **OPTS[0])
    assert got.data_ptr() == out.data_ptr() and np.array_equal(off2, kept_off)
    assert torch.equal(got, ref) and bool((out[ref.shape[0]:] == 7.0).all())
    # an utterance whose flags hold MORE voiced frames than the caller's count never writes beyond its span
    short = kept_off.copy()
    short[1:] -= 10                                                            # utterance 0 claims 10 rows fewer than its flags keep
    out.fill_(7.0)
    got, _ = frontend.ingest(x, OFF, voiced=torch.from_numpy(fl).cuda(), out=out, kept_off=short, **OPTS[0])
    n0 = int(short[1])
    assert torch.equal(got[:n0], ref[:n0]) and torch.equal(got[n0:], ref[n0 + 10:]) and bool((out[got.shape[0]:] == 7.0).all())
    # nothing kept at all: nothing is written, an empty result
    none, off0 = frontend.ingest(x, OFF, voiced=np.zeros(x.shape[0], dtype=np.uint8), **OPTS[0])
    assert none.shape == (0, 30) and not off0.any()


def test_bad_arguments_return_the_library_error():
    import torch
    from libs.amd import capi, frontend
    x = packed(30)
    fl = torch.from_numpy(np.concatenate(flags())).cuda()
    good = frontend.kept_offsets(np.concatenate(flags()), OFF)[1]
    down = OFF.copy()
    down[3], down[4] = down[4], down[3]                                        # decreasing frame offsets
    with pytest.raises(capi.AsvError):
        frontend.ingest(x, down, voiced=fl, kept_off=good, **OPTS[0])
    long = good.copy()
    long[3:] += LENS[2] + 1                                                    # utterance 2 claims more rows than it has frames
    with pytest.raises(capi.AsvError):
        frontend.ingest(x, OFF, voiced=fl, kept_off=long, out=torch.empty((int(long[-1]), 30), device=x.device), **OPTS[0])
    back = good.copy()
    back[2] = back[1] - 1                                                      # decreasing output offsets
    with pytest.raises(capi.AsvError):
        frontend.ingest(x, OFF, voiced=fl, kept_off=back, **OPTS[0])
    with pytest.raises(capi.AsvError):                                         # a causal window needs a positive minimum
        frontend.ingest(x, OFF, voiced=fl, kept_off=good, cmn_window=300, center=False, min_window=0)
    with pytest.raises(capi.AsvError):                                         # without flags every frame is kept
        frontend.ingest(x, OFF, voiced=None, kept_off=good, **OPTS[0])
    lib = capi.lib()
    p = lambda a: a.ctypes.data_as(lib.asv_ingest_frames.argtypes[2])
    out = torch.empty_like(x)
    assert lib.asv_ingest_frames(x.data_ptr(), fl.data_ptr(), p(OFF), p(good), len(LENS), 0, 300, 100, 1, 0, out.data_ptr(), None) < 0      # dim <= 0
    torch.cuda.synchronize()
    # the library still works after the refusals
    kept, _ = frontend.ingest(x, OFF, voiced=fl, kept_off=good, **OPTS[0])
    assert kept.shape[0] == good[-1] and bool(torch.isfinite(kept).all())
