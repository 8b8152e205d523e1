"""A compressed feats.scp (what Kaldi's make_fbank.sh / make_mfcc.sh write by default) through pipeline/onestep/extract_embeddings.py:
the device decode route (bodies read as they are, asv_decode_compressed in front of the ingest / the engine) against the host decode
(ASV_AMD_DEVICE_DECODE=0) - plain, with --cmn-window, with --cmn-window and --vad-scp.  The decoded features are bit-identical and
the 12 utterances form the same single batch on both routes, so the output archives have to be equal byte for byte."""

import importlib.util
import os

import numpy as np
import pytest

import compressed_cases as cc
import helpers
from helpers import rel_err

pytestmark = pytest.mark.gpu

DIM = 23
CREATION = "Xvector(23,10,training=False)"
LENS = [60, 300, 123, 64, 257, 61, 200, 99, 128, 65, 180, 291]
FORMATS = [1, 1, 2, 1, 1, 3, 1, 1, 1, 2, 1, 3]                              # mostly 'CM ' (the scripts' default), the header-only formats among them
SILENT = 4


def load_script():
    spec = importlib.util.spec_from_file_location("extract_embeddings_compressed_gpu", os.path.join(helpers.REPO, "asv-subtools_amd", "pytorch", "pipeline",
                                                                                                    "onestep", "extract_embeddings.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Data(object):
    pass


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    import torch
    from libs.amd import synth
    from libs.support import kaldi_io
    d = Data()
    d.dir = tmp_path_factory.mktemp("compressed")
    d.ee = load_script()
    d.read_matrix = d.ee.read_matrix
    model = helpers.build_model("xvector.py", CREATION)
    d.sd = synth.synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 0)
    d.params = str(d.dir / "final.params")
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in d.sd.items()}, d.params)
    rng = np.random.RandomState(8)
    d.keys = ["utt%02d" % i for i in range(len(LENS))]
    d.bodies = [cc.BODY[f](rng, T, DIM, -6.0, 14.0) for f, T in zip(FORMATS, LENS)]
    lines = cc.write_ark(str(d.dir / "feats.ark"), [(k, cc.compressed_payload(f, b)) for k, f, b in zip(d.keys, FORMATS, d.bodies)])
    d.scp = str(d.dir / "feats.scp")
    open(d.scp, "w").write("\n".join(lines) + "\n")
    # a second table over the same archive plus float32 entries: compressed, `FM ` and range-specified entries mixed
    plain = [(k + "f", cc.float_payload(cc.host_decode(FORMATS[i], d.bodies[i]))) for i, k in enumerate(d.keys) if i % 4 == 1]
    flines = cc.write_ark(str(d.dir / "plain.ark"), plain)
    mixed, d.mixed_keys = [], []
    for i, line in enumerate(lines):
        if i % 4 == 2:
            line += "[3:%d]" % (LENS[i] - 5)
        mixed.append(line)
        if i % 4 == 1:
            mixed.append(flines[i // 4])
    d.mixed_keys = [line.split()[0] for line in mixed]
    d.mixed_scp = str(d.dir / "mixed.scp")
    open(d.mixed_scp, "w").write("\n".join(mixed) + "\n")
    d.flags = [(rng.rand(T) < 0.7).astype(np.float32) for T in LENS]
    d.flags[SILENT][:] = 0.0
    d.vad_scp = str(d.dir / "vad.scp")
    with open(d.dir / "vad.ark", "wb") as f, open(d.vad_scp, "w") as s:
        for k, v in zip(d.keys, d.flags):
            f.write((k + " ").encode())
            s.write("%s %s:%d\n" % (k, d.dir / "vad.ark", f.tell()))
            kaldi_io.write_vec_flt(f, v)
    d.runs = {}
    return d


def run(d, monkeypatch, name, scp, extra, device_decode):
    """One run of the script's main() in this process (cached per name): the bytes of the output archive, and how often the host
    decoder was asked for a direct compressed entry."""
    if name not in d.runs:
        out = str(d.dir / ("xvector_%s.ark" % name))
        monkeypatch.setenv("ASV_AMD_DEVICE_DECODE", "1" if device_decode else "0")
        monkeypatch.setenv("ASV_AMD_PRECISION", "f32")
        decoded = []
        real = d.read_matrix
        monkeypatch.setattr(d.ee, "read_matrix", lambda rx: (decoded.append(rx), real(rx))[1])
        d.ee.main(["--model-blueprint", os.path.join(helpers.MODEL_DIR, "xvector.py"), "--model-creation", CREATION, "--use-gpu", "true", "--gpu-id", "0",
                   "--batch-frames", "4096", "--batch-utts", "64"] + extra + [d.params, "scp:" + scp, "ark:" + out])
        d.runs[name] = (open(out, "rb").read(), decoded)
    return d.runs[name]


@pytest.mark.parametrize("mode", ["plain", "cmn", "cmn_vad"])
def test_device_decode_equals_host_decode_byte_for_byte(data, monkeypatch, mode):
    from libs.support import kaldi_io
    d = data
    extra = {"plain": [], "cmn": ["--cmn-window", "300"], "cmn_vad": ["--cmn-window", "300", "--vad-scp", d.vad_scp]}[mode]
    dev, decoded = run(d, monkeypatch, mode + "_device", d.scp, extra, True)
    assert decoded == [], "the device route decoded on the host: %r" % decoded       # not a single read_matrix call for a direct compressed entry
    host, decoded = run(d, monkeypatch, mode + "_host", d.scp, extra, False)
    assert len(decoded) == len(LENS)                                                  # (the other route: every entry through the numpy decode)
    assert dev == host
    import io
    got = list(kaldi_io.read_vec_flt_ark(io.BytesIO(dev)))
    want_keys = [k for i, k in enumerate(d.keys) if not (mode == "cmn_vad" and i == SILENT)]
    assert [k for k, _ in got] == want_keys
    assert all(np.isfinite(v).all() and np.abs(v).max() > 0 for _, v in got)


def test_plain_run_is_the_model_on_the_host_decoded_features(data, monkeypatch):
    """Not only equal to the other route: the vectors are the model's on what kaldi_io.read_mat decodes."""
    import io
    from libs.support import kaldi_io
    d = data
    dev, _ = run(d, monkeypatch, "plain_device", d.scp, [], True)
    model = helpers.build_model("xvector.py", CREATION, d.sd)
    model.cuda()
    model.amd_precision = "f32"
    want = model.extract_embedding_batch([cc.host_decode(f, b) for f, b in zip(FORMATS, d.bodies)]).numpy()
    got = np.stack([v for _, v in kaldi_io.read_vec_flt_ark(io.BytesIO(dev))])
    assert got.shape == want.shape and rel_err(got, want) < 1e-4, rel_err(got, want)          # (the gate the f32 path holds everywhere; the same kernels on the same rows)


def test_mixed_table_keeps_key_order_and_completeness(data, monkeypatch):
    """Compressed, `FM ` and range-specified entries in one table: the device route cuts a group wherever the kind changes, so its
    batches are NOT the host route's - the keys come out once each and in scp order, and the vectors agree within the gate the
    pipeline tests hold against the oracle (1e-4 relative; in practice they are equal)."""
    import io
    from libs.support import kaldi_io
    d = data
    dev, decoded = run(d, monkeypatch, "mixed_device", d.mixed_scp, ["--cmn-window", "300"], True)
    host, _ = run(d, monkeypatch, "mixed_host", d.mixed_scp, ["--cmn-window", "300"], False)
    ranged = [line.split(None, 1)[1] for line in open(d.mixed_scp).read().splitlines() if line.endswith("]")]
    assert sorted(decoded) == sorted(ranged) and len(ranged) == 3                     # only the range-specified entries were decoded on the host
    a, b = list(kaldi_io.read_vec_flt_ark(io.BytesIO(dev))), list(kaldi_io.read_vec_flt_ark(io.BytesIO(host)))
    assert [k for k, _ in a] == d.mixed_keys and [k for k, _ in b] == d.mixed_keys and len(set(d.mixed_keys)) == len(LENS) + 3
    for (k, v), (_, w) in zip(a, b):
        assert rel_err(v, w) < 1e-4, (k, rel_err(v, w))
    # an `FM ` copy of a compressed entry holds the same features: the same vector
    for (k, v) in a:
        if k.endswith("f"):
            twin = dict(a)[k[:-1]]
            assert rel_err(v, twin) < 1e-4, k
