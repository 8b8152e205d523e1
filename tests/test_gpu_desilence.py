"""asv_desilence_pcm16 (csrc/kernels_desilence.hip) through the C ABI and through libs.amd.frontend.de_silence_device against
libs.amd.frontend.de_silence_host and the reference's own outputs (tests/golden/de_silence.npz): samples AND out_offsets equal, no
tolerance - the rule is integer arithmetic on both sides.  Every call runs with 64 sentinel samples behind `out` (and in front of it),
which must come back unchanged, and with the input compared before and after."""

import ctypes as C

import numpy as np
import pytest

import de_silence_cases as dc

pytestmark = pytest.mark.gpu

GUARD = 64                                            # sentinel samples in front of and behind `out`
SENTINEL = -21846                                     # 0xAAAA: no test input holds it


def host_rule(x, win, min_eng):
    from libs.amd import frontend
    return frontend.de_silence_host(x, 1, win_len=win, min_eng=min_eng)


def run_capi(utts, win, min_eng, shift=0):
    """The batch through the C ABI -> (per-utterance outputs, out_offsets).  shift: samples the packed wave is moved from its 16-byte
    aligned allocation (1: every even start becomes odd).  Checks the guards around `out`, the untouched rest of `out` and the input."""
    import torch
    from libs.amd import capi
    dev = torch.device("cuda", 0)
    off = dc.offsets(utts)
    total = int(off[-1])
    host = np.full(total + shift + 8, SENTINEL, dtype=np.int16)            # (8 more: a batch without samples still has an address)
    host[shift:shift + total] = np.concatenate(utts)
    d_wave = torch.from_numpy(host).to(dev)
    whole = torch.full((total + 2 * GUARD,), SENTINEL, dtype=torch.int16, device=dev)
    out_off = np.full(len(utts) + 1, -7, dtype=np.int64)
    with torch.cuda.device(dev):
        capi.check(capi.lib().asv_desilence_pcm16(C.c_void_p(d_wave.data_ptr() + 2 * shift), off.ctypes.data_as(C.POINTER(C.c_longlong)), len(utts), win,
                                                  float(min_eng), C.c_void_p(whole.data_ptr() + 2 * GUARD), out_off.ctypes.data_as(C.POINTER(C.c_longlong)),
                                                  C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "asv_desilence_pcm16")
    torch.cuda.synchronize(dev)
    w = whole.cpu().numpy()
    assert out_off[0] == 0 and (np.diff(out_off) >= 0).all() and out_off[-1] <= total, out_off
    kept = int(out_off[-1])
    assert (w[:GUARD] == SENTINEL).all(), "samples in front of `out` were written"
    assert (w[GUARD + kept:] == SENTINEL).all(), "samples behind out_offsets[-1] were written"
    assert np.array_equal(d_wave.cpu().numpy(), host), "the input was written"
    body = w[GUARD:GUARD + kept]
    return [body[int(a):int(b)] for a, b in zip(out_off[:-1], out_off[1:])], out_off


def run_frontend(utts, sample_rate, min_eng, **kw):
    import torch
    from libs.amd import frontend
    dev = torch.device("cuda", 0)
    off = dc.offsets(utts)
    d_wave = torch.from_numpy(np.concatenate(utts)).to(dev)
    out, out_off = frontend.de_silence_device(d_wave, off, sample_rate, min_eng=min_eng, **kw)
    assert out.dtype == torch.int16 and out.is_cuda and out.shape == (int(out_off[-1]),)
    o = out.cpu().numpy()
    return [o[int(a):int(b)] for a, b in zip(out_off[:-1], out_off[1:])], out_off


def check(got, out_off, want):
    assert out_off.tolist() == dc.offsets(want).tolist()
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, k
        diff = g != w
        assert not diff.any(), "utterance %d: %d of %d samples differ, first at %d" % (k, int(diff.sum()), diff.size, int(np.argmax(diff)))


# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dc.golden_cases(), ids=lambda c: c.name)
def test_golden_case_alone(case):
    """A batch of one, through the C ABI (at an even and at an odd address) and through the wrapper: the reference's samples."""
    win = int(0.1 * case.sample_rate)
    assert np.array_equal(host_rule(case.x, win, case.min_eng), case.y)
    for shift in (0, 1):
        got, out_off = run_capi([case.x], win, case.min_eng, shift=shift)
        check(got, out_off, [case.y])
    got, out_off = run_frontend([case.x], case.sample_rate, case.min_eng)
    check(got, out_off, [case.y])


@pytest.mark.parametrize("sample_rate, min_eng", sorted({(c.sample_rate, c.min_eng) for c in dc.golden_cases()}))
def test_golden_cases_packed(sample_rate, min_eng):
    """Every fixture case of one (sample rate, threshold) as ONE packed batch: odd-length cases move their successors to odd samples."""
    cases = [c for c in dc.golden_cases() if (c.sample_rate, c.min_eng) == (sample_rate, min_eng)]
    got, out_off = run_capi([c.x for c in cases], int(0.1 * sample_rate), min_eng)
    check(got, out_off, [c.y for c in cases])
    got, out_off = run_frontend([c.x for c in cases], sample_rate, min_eng)
    check(got, out_off, [c.y for c in cases])


@pytest.mark.parametrize("win", [1, 7, 64, 65, 1600])
def test_odd_starts_and_empty_utterances(win):
    utts = dc.odd_batch(win)
    off = dc.offsets(utts)
    assert len(utts[0]) == 0 and len(utts[4]) == 0 and len(utts[-1]) == 0 and (off[1:-1] % 2 == 1).any()
    want = [host_rule(x, win, 50) for x in utts]
    assert any(len(w) < len(x) for w, x in zip(want, utts)) and np.array_equal(want[6], utts[6])          # trimmed ones, and the fall-back
    for shift in (0, 1):
        got, out_off = run_capi(utts, win, 50, shift=shift)
        check(got, out_off, want)
    got, out_off = run_frontend(utts, 1, 50, win_len=win)
    check(got, out_off, want)


def test_only_empty_utterances():
    import torch
    from libs.amd import frontend
    empty = np.zeros(0, dtype=np.int16)
    got, out_off = run_capi([empty, empty, empty], 64, 50)
    assert out_off.tolist() == [0, 0, 0, 0] and all(len(g) == 0 for g in got)
    out, out_off = frontend.de_silence_device(torch.zeros(0, dtype=torch.int16, device="cuda:0"), np.zeros(3, dtype=np.int64), 16000)
    assert out.shape == (0,) and out_off.tolist() == [0, 0, 0]


def test_block_scan_crosses_a_workgroup():
    x = dc.long_utterance()
    assert -(-len(x) // 7) == 700
    want = host_rule(x, 7, 50)
    assert 0 < len(want) < len(x)
    for shift in (0, 1):
        got, out_off = run_capi([x], 7, 50, shift=shift)
        check(got, out_off, [want])
    pad = np.array([900, -900, 3], dtype=np.int16)     # behind another utterance: the long one's blocks start at block 1, on an odd sample
    got, out_off = run_capi([pad, x, pad], 7, 50)
    check(got, out_off, [host_rule(pad, 7, 50), want, host_rule(pad, 7, 50)])


@pytest.fixture(scope="module")
def many():
    """The 600-utterance batch, its host results and its device results: computed once, shared, read-only."""
    utts, silent = dc.many_utterances()
    want = [host_rule(x, 64, 50) for x in utts]
    got, out_off = run_capi(list(utts), 64, 50)
    return utts, silent, want, got, out_off


def test_utterance_scan_crosses_a_workgroup(many):
    utts, silent, want, got, out_off = many
    assert len(utts) == 600 and all(1 <= -(-len(x) // 64) <= 3 for x in utts)
    assert sum(silent) > 80 and all(np.array_equal(w, x) for s, w, x in zip(silent, want, utts) if s)      # the fall-backs ...
    assert sum(len(w) < len(x) for w, x in zip(want, utts)) > 200                                          # ... next to trimmed utterances
    check(got, out_off, want)


def test_neighbour_independence(many):
    """An utterance's output in the batch of 600 equals its output as a batch of one: the first, the last, every neighbour of the first
    few fall-backs, and the fall-backs themselves."""
    utts, silent, want, got, out_off = many
    picks = {0, len(utts) - 1}
    for i in [k for k, s in enumerate(silent) if s][:7]:
        picks.update(j for j in (i - 1, i, i + 1) if 0 <= j < len(utts))
    assert 18 <= len(picks) <= 24
    for i in sorted(picks):
        alone, alone_off = run_capi([utts[i]], 64, 50)
        assert alone_off.tolist() == [0, len(got[i])] and np.array_equal(alone[0], got[i]), i


def test_wrapper_feeds_the_features():
    """fbank_packed(de_silence=...) = fbank_packed of the host-trimmed waveforms, bit for bit; None is the old path."""
    from libs.amd import frontend
    cases = [c for c in dc.golden_cases() if (c.sample_rate, c.min_eng) == (16000, 50.0) and len(c.y) >= 400]
    opts = dict(num_mel_bins=30, dither=0.0, energy_floor=0.0, sample_frequency=16000.0)
    feats, frame_off = frontend.fbank_packed([c.x for c in cases], de_silence={"win_len": 0.1, "min_eng": 50}, mean_norm=True, **opts)
    want, want_off = frontend.fbank_packed([c.y for c in cases], mean_norm=True, **opts)
    assert frame_off.tolist() == want_off.tolist() and np.array_equal(feats.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))
    plain, plain_off = frontend.fbank_packed([c.x for c in cases], de_silence=None, mean_norm=True, **opts)
    assert plain_off[-1] > want_off[-1]
    with pytest.raises(TypeError):
        frontend.fbank_packed([c.x for c in cases], de_silence={"amp_th": 50}, **opts)


def test_bad_arguments_leave_out_untouched():
    import torch
    from libs.amd import capi
    dev = torch.device("cuda", 0)
    lib = capi.lib()
    wave = torch.from_numpy(dc.utterance(np.random.RandomState(3), 64, 8)).to(dev)
    out = torch.full((64 + GUARD,), SENTINEL, dtype=torch.int16, device=dev)
    with torch.cuda.device(dev):
        for name, call in dc.bad_calls(lib, wave.data_ptr(), out.data_ptr()).items():
            out_off = np.full(3, -5, dtype=np.int64)
            assert call(out_off) < 0, name
            assert b"asv_desilence_pcm16" in lib.asv_last_error(), name
            assert (out_off == -5).all(), name
        torch.cuda.synchronize(dev)
        assert (out.cpu().numpy() == SENTINEL).all()
        # and the same arguments put right run
        out_off = np.zeros(3, dtype=np.int64)
        good = np.array([0, 32, 64], dtype=np.int64)
        capi.check(lib.asv_desilence_pcm16(wave.data_ptr(), good.ctypes.data_as(C.POINTER(C.c_longlong)), 2, 8, 50.0, out.data_ptr(),
                                           out_off.ctypes.data_as(C.POINTER(C.c_longlong)), None), "asv_desilence_pcm16")
    w = wave.cpu().numpy()
    want = [host_rule(w[:32], 8, 50), host_rule(w[32:], 8, 50)]
    o = out.cpu().numpy()
    assert out_off.tolist() == dc.offsets(want).tolist() and np.array_equal(o[:int(out_off[-1])], np.concatenate(want))
    assert (o[int(out_off[-1]):] == SENTINEL).all()
