"""Host side of --de-silence: libs.amd.frontend.de_silence_host against what the reference's own de_silence returned for the constructed
cases of tests/golden/de_silence.npz (tests/gen_de_silence_golden.py), the C ABI declaration and its argument checks (refused before any
device call), and the command line of the waveform-in script - no GPU."""

import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

import de_silence_cases as dc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_script():
    spec = importlib.util.spec_from_file_location("extract_embeddings_online_desilence", os.path.join(REPO, "asv-subtools_amd", "pytorch", "pipeline", "onestep",
                                                                                                      "extract_embeddings_online.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_holds_the_cases_the_rule_can_go_wrong_at():
    cases = dc.golden_cases()
    names = [c.name for c in cases]
    assert len(cases) >= 20 and len(set(names)) == len(names)
    assert {c.sample_rate for c in cases} == {8000, 16000, 44100} and {c.min_eng for c in cases} >= {12.5, 50.0, 100.0}
    for c in cases:
        assert c.x.dtype == np.int16 and c.y.dtype == np.int16 and 0 < len(c.y) <= len(c.x)
        whole = len(c.y) == len(c.x)
        assert whole == (c.name.endswith("kept_whole") or c.name.startswith("f_loud") or c.name == "b_short_loud"), c.name      # the named exceptions
    assert any((c.x == -32768).any() for c in cases)
    assert any(len(c.x) % int(0.1 * c.sample_rate) == 1 for c in cases) and any(len(c.x) % int(0.1 * c.sample_rate) == 0 for c in cases)
    assert any(len(c.x) < int(0.1 * c.sample_rate) for c in cases)


@pytest.mark.parametrize("case", dc.golden_cases(), ids=lambda c: c.name)
def test_host_rule_equals_the_reference_sample_for_sample(case):
    from libs.amd import frontend
    got = frontend.de_silence_host(case.x, case.sample_rate, min_eng=case.min_eng)
    assert got.dtype == np.int16 and np.array_equal(got, case.y)
    assert np.array_equal(got, dc.plain_rule(case.x, int(0.1 * case.sample_rate), case.min_eng))


def test_host_rule_on_the_synthetic_batches_equals_the_plain_loop():
    """The inputs of the device tests: the vectorised host rule against the block-by-block loop."""
    from libs.amd import frontend
    for win in (1, 7, 64, 65, 1600):
        for x in dc.odd_batch(win):
            assert np.array_equal(frontend.de_silence_host(x, 1, win_len=win, min_eng=50), dc.plain_rule(x, win, 50.0))


def test_host_rule_edge_cases_and_refusals():
    from libs.amd import frontend
    empty = np.zeros(0, dtype=np.int16)
    assert frontend.de_silence_host(empty, 16000).shape == (0,)
    x = np.array([-32768] * 5 + [0] * 5, dtype=np.int16)
    assert frontend.de_silence_host(x, 50, min_eng=32767).tolist() == [-32768] * 5        # win = 5: 5 * 32768 > 32767 * 5; in 16 bits |-32768| would be negative
    assert frontend.de_silence_host(x, 50, min_eng=0).tolist() == [-32768] * 5            # strict: 0 > 0 drops the silent block
    assert frontend.de_silence_host(np.zeros(7, dtype=np.int16), 50, min_eng=0).tolist() == [0] * 7
    with pytest.raises(ValueError):
        frontend.de_silence_host(x.astype(np.float32), 16000)
    with pytest.raises(ValueError):
        frontend.de_silence_host(x, 5)                                                    # int(0.1 * 5) = 0 samples
    with pytest.raises(ValueError):
        frontend.de_silence_host(x, 16000, min_eng=-1)
    with pytest.raises(ValueError):
        frontend.de_silence_host(x, 16000, min_eng=float("nan"))


def test_device_wrapper_refuses_float32():
    import torch
    from libs.amd import frontend
    with pytest.raises(ValueError, match="int16"):
        frontend.de_silence_device(torch.zeros(3200, dtype=torch.float32), np.array([0, 3200]), 16000)


def test_entry_point_is_declared_and_listed():
    from libs.amd import capi
    hdr = open(os.path.join(REPO, "include", "asv_amd.h")).read()
    assert re.search(r"\bint\s+asv_desilence_pcm16\s*\(", hdr)
    assert "asv_desilence_pcm16" in capi.SYMBOLS
    assert len(capi.lib().asv_desilence_pcm16.argtypes) == 8
    assert "kernels_desilence.hip" in open(os.path.join(REPO, "asv-subtools_amd", "csrc", "Makefile")).read()


def test_bad_arguments_are_refused_before_any_device_call():
    from libs.amd import capi
    lib = capi.lib()
    # (host memory stands in for the two device pointers: every refusal below comes before the library looks at them)
    wave, out = np.zeros(64, dtype=np.int16), np.full(64, 77, dtype=np.int16)
    for name, call in dc.bad_calls(lib, wave.ctypes.data, out.ctypes.data).items():
        out_off = np.full(3, -5, dtype=np.int64)
        assert call(out_off) < 0, name
        assert b"asv_desilence_pcm16" in lib.asv_last_error(), name
        assert (out == 77).all() and (out_off == -5).all(), name


def test_script_takes_de_silence_on_its_command_line():
    ee = load_script()
    base = ["--model-blueprint", "m.py", "--model-creation", "X()", "--feat-config", "feat.yaml", "final.params", "wav.scp", "ark:out.ark"]
    assert ee.check_args(ee.get_args(base)) is None                                                   # the default: no trimming
    assert ee.check_args(ee.get_args(["--de-silence", "false", "--amp-th", "100"] + base)) is None
    assert ee.check_args(ee.get_args(["--de-silence", "true"] + base)) == 50                          # --amp-th's default, the reference's
    assert ee.check_args(ee.get_args(["--de-silence", "true", "--amp-th", "100"] + base)) == 100
    with pytest.raises(ValueError):
        ee.check_args(ee.get_args(["--de-silence", "true", "--amp-th", "-1"] + base))
    with pytest.raises(ValueError):
        ee.check_args(ee.get_args(["--data-type", "shard"] + base))                                   # still refused
    with pytest.raises(RuntimeError):
        ee.check_args(ee.get_args(["--use-gpu", "false"] + base))
    assert "not offered by the device path" not in open(ee.__file__).read()


def test_script_chooses_the_trimming_side_by_environment(monkeypatch):
    ee = load_script()
    monkeypatch.delenv("ASV_AMD_DEVICE_DESILENCE", raising=False)
    assert ee.device_desilence() is True
    monkeypatch.setenv("ASV_AMD_DEVICE_DESILENCE", "0")
    assert ee.device_desilence() is False
    monkeypatch.setenv("ASV_AMD_DEVICE_DESILENCE", "1")
    assert ee.device_desilence() is True
