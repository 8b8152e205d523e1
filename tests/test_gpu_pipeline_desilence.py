"""wav.scp -> ark with --de-silence true: the waveform-in script trims on the device (asv_desilence_pcm16) what
libs.amd.frontend.de_silence_host trims on the host - the same vectors, byte for byte, as the script run without the flag on wav files
that hold the host-trimmed samples, and as the script trimming in its reader threads (ASV_AMD_DEVICE_DESILENCE=0)."""

import os
import subprocess
import sys
import wave

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu


def write_wavs(folder, waves):
    folder.mkdir()
    scp = folder / "wav.scp"
    with open(scp, "w") as f:
        for i, wv in enumerate(waves):
            path = folder / ("u%d.wav" % i)
            with wave.open(str(path), "wb") as wf:
                wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(16000)
                wf.writeframes(wv.astype("<i2").tobytes())
            f.write("utt%d %s\n" % (i, path))
    return scp


def test_online_script_de_silence_matches_host_trimmed_wavs(tmp_path):
    import torch
    import yaml
    from libs.amd import frontend, synth
    from libs.support import kaldi_io
    import libs.support.utils as utils
    g, sd = helpers.golden_state_dict("xvector_c1")                # Xvector(30, ...)
    rng = np.random.RandomState(9)
    hush = lambda n: rng.randint(-2, 3, size=n).astype(np.int16)   # +-2 counts
    waves = [synth.synth_wave(n, 900 + i).astype(np.int16) for i, n in enumerate([16000, 20000, 5100, 24000, 20011])]
    waves[0][1600:4800] = 0                                         # two whole blocks of zeros ...
    waves[0][8000:9700] = hush(1700)                                # ... and a quiet stretch that covers only block 5 entirely
    waves[1] = hush(20000)                                          # wholly silent: kept whole
    waves[2][:4800] = 0                                             # three silent blocks and a loud tail of 300 samples: less than one 25 ms frame is left
    waves[4][:3300] = hush(3300)
    waves[4][-1000:] = 0                                            # the tail block (811 samples) and part of the block before it
    trimmed = [frontend.de_silence_host(wv, 16000, min_eng=50) for wv in waves]
    assert [len(t) for t in trimmed] == [16000 - 4800, 20000, 300, 24000, 20011 - 3200 - 811]
    scp, scp_trimmed = write_wavs(tmp_path / "raw", waves), write_wavs(tmp_path / "trimmed", trimmed)
    featset = {"num_mel_bins": 30, "dither": 0.0, "energy_floor": 0.0}
    conf = tmp_path / "feat.yaml"
    conf.write_text(yaml.safe_dump({"feature_type": "fbank", "kaldi_featset": featset, "mean_var_conf": {"mean_norm": True, "std_norm": False}}))
    params = tmp_path / "final.params"
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, str(params))
    cfg = tmp_path / "nnet.config"
    utils.write_nnet_config(os.path.join(helpers.MODEL_DIR, "xvector.py"), str(g["creation"]), str(cfg))
    script = os.path.join(helpers.REPO, "asv-subtools_amd", "pytorch", "pipeline", "onestep", "extract_embeddings_online.py")

    def run(name, flags, wav_scp, **env):
        out_ark = tmp_path / (name + ".ark")
        res = subprocess.run([sys.executable, script, "--nnet-config", str(cfg), "--data-type", "raw", "--feat-config", str(conf), "--gpu-id", "0",
                              "--batch-utts", "2"] + flags + [str(params), str(wav_scp), str(out_ark)], capture_output=True, text=True,
                             env=dict(os.environ, ASV_AMD_PRECISION="f32", **env), timeout=600)
        assert res.returncode == 0, res.stdout + res.stderr
        assert "RTF:" in res.stdout and "utt2 is shorter than one frame" in res.stdout, res.stdout
        assert "Extracted 4 embeddings." in res.stdout
        with open(out_ark, "rb") as f:
            return list(kaldi_io.read_vec_flt_ark(str(out_ark))), f.read(), res.stdout

    device, device_bytes, device_log = run("device", ["--de-silence", "true", "--amp-th", "50"], scp)
    plain, plain_bytes, plain_log = run("plain", [], scp_trimmed)
    assert [k for k, _ in device] == [k for k, _ in plain] == ["utt0", "utt1", "utt3", "utt4"]
    for (k, a), (_, b) in zip(device, plain):
        assert a.dtype == np.float32 and a.shape == (512,) and a.tobytes() == b.tobytes(), k
    assert device_bytes == plain_bytes
    # the RTF line counts the frames after trimming: both runs saw the same frames (the line itself is a measured time)
    host, host_bytes, _ = run("host", ["--de-silence", "true", "--amp-th", "50"], scp, ASV_AMD_DEVICE_DESILENCE="0")
    assert host_bytes == device_bytes
