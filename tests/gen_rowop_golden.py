#!/usr/bin/env python3
"""Generate tests/golden/rowop_*.npz by running the REFERENCE with the layer options the row op covers: the activations beyond
relu / tanh / sigmoid (reference libs/nnet/activation.py:69-94) and `ln_replace` (LayerNorm in place of the BatchNorm,
libs/nnet/components.py:365-386).  Build container only (needs the reference tree, like oracle/gen_golden.py, whose shims,
synthetic weights and `run_extractor_case` this file uses).  Outputs only, as every other extractor fixture.

The shipped snowdar / ECAPA blueprints drop `ln_replace` (and the snowdar one `negative_slope`) before it reaches a layer -
their option defaults do not name it; the LayerNorm and slope fixtures therefore come from tests/rowop_blueprint.py, run
here against the reference's own layer classes.  'gelu' has no fixture: the reference's factory calls
torch.nn.GELU(inplace=...), a TypeError with the torch it runs on, so the reference cannot produce a gelu output
(tests/test_rowop_host.py pins the op against torch.nn.functional.gelu instead).

Every fixture has utterances of 1 and 2 frames next to one of about 200 and one of 37 - but the ECAPA one, whose shortest
utterances have 3 and 2 frames: the reference's ECAPA pooling takes torch.var over the frames and answers one frame with NaN.

    PYTHONDONTWRITEBYTECODE=1 python tests/gen_rowop_golden.py [case ...]
"""

import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import gen_golden as G  # noqa: E402

LX = "rowop_blueprint.py"                     # tests/rowop_blueprint.py: layer options unfiltered
BN_HALF = "'bn_params':{'momentum':0.5,'affine':%s,'track_running_stats':True}"


def _utts(seed, long=200):
    return [(long, seed), (37, seed + 1), (2, seed + 2), (1, seed + 3)]


CASES = {
    # a new activation in every layer of the standard x-vector (act -> BN): frames domain / frames and utts domain
    "rowop_xvector_swish": dict(blueprint="xvector.py", creation="Xvector(24,10,nonlinearity='swish',training=False)", dim=24, utts=_utts(8000), wseed=41),
    "rowop_xvector_leaky_near": dict(blueprint="xvector.py", creation="Xvector(30,10,nonlinearity='leaky_relu',training=False,extracted_embedding='near')",
                                     dim=30, utts=_utts(8100, 201), wseed=42),
    # the snowdar and ECAPA blueprints with new activations (act -> BN)
    "rowop_snowdar_mish": dict(blueprint="snowdar_xvector.py",
                               creation="Xvector(40,10,training=False,tdnn_layer_params={'nonlinearity':'mish'},extracted_embedding='near')",
                               dim=40, utts=_utts(8200), wseed=43),
    "rowop_ecapa_fc_dswish": dict(blueprint="ecapa_tdnn_xvector.py",
                                  creation="ECAPA_TDNN(80,10,training=False,ecapa_params={'channels':512,'embd_dim':192,'mfa_conv':1536},fc1=True,"
                                           "fc1_params={'nonlinearity':'double_swish'},fc2_params={'nonlinearity':'selu'})",
                                  dim=80, utts=[(200, 8500), (37, 8501), (3, 8502), (2, 8503)], wseed=46),       # (one frame: NaN in the reference, torch.var)
    # act -> LN, learnable (bn_params' affine is on), frames and utts domain
    "rowop_lx_mish_ln": dict(blueprint=LX, creation="RowopXvector(40,10,layer_params={'nonlinearity':'mish','ln_replace':True})",
                             dim=40, utts=_utts(8600), wseed=47),
    # LN -> act (always learnable)
    "rowop_lx_selu_lnfirst": dict(blueprint=LX, creation="RowopXvector(40,10,layer_params={'nonlinearity':'selu','bn-relu':True,'ln_replace':True})",
                                  dim=40, utts=_utts(8700, 199), wseed=48),
    # BN -> act with a non-default slope, BatchNorm without affine
    "rowop_lx_leaky02_bnfirst": dict(blueprint=LX,
                                     creation="RowopXvector(40,10,layer_params={'nonlinearity':'leaky_relu','nonlinearity_params':{'inplace':True,"
                                              "'negative_slope':0.2},'bn-relu':True,'bn_params':{'momentum':0.1,'affine':False,'track_running_stats':True}})",
                                     dim=40, utts=_utts(8800), wseed=49),
    # the embedding head of the reference's Conformer recipe (launcher/runTransformerXvector.py:262-267): ReLU -> LN layers (the
    # ReLU stays in the GEMM epilogue), tdnn6 = double_swish -> LN without affine, tdnn7 = LN with affine and no activation
    "rowop_lx_head_ln": dict(blueprint=LX,
                             creation="RowopXvector(30,10,layer_params={'ln_replace':True},tdnn6_params={'nonlinearity':'double_swish','ln_replace':True,%s},"
                                      "tdnn7_params={'nonlinearity':'','ln_replace':True,%s})" % (BN_HALF % "False", BN_HALF % "True"),
                             dim=30, utts=_utts(8900), wseed=50),
}


def main(argv):
    import numpy as np
    if not os.path.isdir(G.REF):
        sys.exit("gen_rowop_golden.py needs the reference tree at %s (build container only)" % G.REF)
    G.install_shims()
    sys.path.insert(0, os.path.join(G.REF, "pytorch"))
    os.makedirs(G.GOLDEN, exist_ok=True)
    synth = G.load_synth()
    for name in argv or list(CASES):
        case, path = dict(CASES[name]), os.path.join(G.GOLDEN, name + ".npz")
        if case["blueprint"] == LX:               # an absolute path wins in run_extractor_case's join with the reference's model directory
            case["blueprint"] = os.path.join(REPO, "tests", LX)
        G.run_extractor_case(name, case, synth, path)
        if case["blueprint"] != CASES[name]["blueprint"]:
            with np.load(path) as g:
                out = {k: g[k] for k in g.files}
            out["blueprint"] = np.array(LX)       # the fixture names the file, not where it lay
            np.savez_compressed(path, **out)


if __name__ == "__main__":
    main(sys.argv[1:])
