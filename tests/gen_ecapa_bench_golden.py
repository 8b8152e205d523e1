#!/usr/bin/env python3
"""Generate tests/golden/ecapa_bench_*.npz by running the REFERENCE's benchmark ECAPA-TDNN blueprint (model/ecapa-tdnn-xvector.py,
the file launcher/runEcapaXvector.py trains).  Build container only (needs the reference tree, like oracle/gen_golden.py, whose
shims, synthetic weights and `run_extractor_case` this file uses unchanged).  Outputs only, as every other extractor fixture.

For every case it also runs the reference model in float64 on the same inputs and prints the distance of the stored float32
embeddings from it (`rel_err` of tests/helpers.py, per utterance): the room the reference's own arithmetic takes of the 1e-4 gate.

    PYTHONDONTWRITEBYTECODE=1 python tests/gen_ecapa_bench_golden.py [case ...]
"""

import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import gen_golden as G  # noqa: E402

BLUEPRINT = "ecapa-tdnn-xvector.py"
UTT_FRAMES = (300, 150, 129, 64, 37, 9, 5, 3, 2, 1)
UTTS = [(T, 7400 + i) for i, T in enumerate(UTT_FRAMES)]
CASES = {
    "ecapa_bench_default": dict(blueprint=BLUEPRINT, creation="ECAPA_TDNN(80,10,training=False)", dim=80, utts=UTTS, wseed=41),
    # the recipe's own arguments (launcher/runEcapaXvector.py:196-224): fc2 without a nonlinearity, BatchNorm affine=False
    "ecapa_bench_launcher": dict(blueprint=BLUEPRINT, creation="ECAPA_TDNN(80,10,training=False,channels=512,embd_dim=192,%s)" % G.LAUNCHER_FC2,
                                 dim=80, utts=UTTS, wseed=42),
    "ecapa_bench_c1024_far": dict(blueprint=BLUEPRINT,
                                  creation="ECAPA_TDNN(40,10,training=False,channels=1024,embd_dim=256,fc1=True,extracted_embedding='far')",
                                  dim=40, utts=UTTS, wseed=43),
    "ecapa_bench_stats": dict(blueprint=BLUEPRINT, creation="ECAPA_TDNN(80,10,training=False,pooling='statistics',extracted_embedding='near_affine')",
                              dim=80, utts=UTTS, wseed=44),
    "ecapa_bench_multihead": dict(blueprint=BLUEPRINT, creation="ECAPA_TDNN(80,10,training=False,pooling='multi-head',pooling_params={'num_head':4})",
                                  dim=80, utts=UTTS, wseed=45),
}


def float64_distance(name, case, synth, path):
    """The reference in float64 (same weights, same features) against the float32 embeddings just stored."""
    import numpy as np
    import torch
    import libs.support.utils as utils
    model = utils.create_model_from_py(os.path.join(G.REF, "pytorch", "model", case["blueprint"]), case["creation"])
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = synth.synth_state_dict(shapes, case["wseed"])
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model.double().eval()
    stored = np.load(path)["embeddings"]
    worst = 0.0
    for i, (T, seed) in enumerate(case["utts"]):
        e64 = model.extract_embedding(synth.synth_feats(T, case["dim"], seed).astype(np.float64)).numpy().astype(np.float64)
        err = float(np.abs(stored[i].astype(np.float64) - e64).max() / max(np.abs(e64).max(), 1e-30))
        worst = max(worst, err)
        print("  %s T=%d: float32 vs float64 rel_err %.3g" % (name, T, err))
    print("%s: worst float32 vs float64 rel_err %.3g" % (name, worst))


def main(argv):
    if not os.path.isdir(G.REF):
        sys.exit("gen_ecapa_bench_golden.py needs the reference tree at %s (build container only)" % G.REF)
    G.install_shims()
    sys.path.insert(0, os.path.join(G.REF, "pytorch"))
    os.makedirs(G.GOLDEN, exist_ok=True)
    synth = G.load_synth()
    for name in argv or list(CASES):
        path = os.path.join(G.GOLDEN, name + ".npz")
        G.run_extractor_case(name, CASES[name], synth, path)
        float64_distance(name, CASES[name], synth, path)


if __name__ == "__main__":
    main(sys.argv[1:])
