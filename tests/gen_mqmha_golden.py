#!/usr/bin/env python3
"""Generate tests/golden/ecapa_mqmha_*.npz by running the REFERENCE ECAPA-TDNN with pooling='mqmha' (MQMHASP,
reference libs/nnet/pooling.py:590-701).  Build container only (needs the reference tree, like oracle/gen_golden.py, whose
shims, synthetic weights and `run_extractor_case` this file uses).  Outputs only, as every other extractor fixture.

The one pin: the reference's pooling.py calls `compute_statistics` (:636, :654) without defining or importing it - as shipped,
extract_embedding ends in NameError.  The only definition in the reference tree is model/transformer_xvector.py:12-25; called
with its default `dim=2` it sums over the query axis of the 5-D view, which contradicts the reshapes and shape comments at
pooling.py:637-655 (they want the LAST axis summed and kept).  The name is therefore bound to the reference's own function,
called with `dim = x.dim() - 1` and the summed axis put back; the arithmetic is the reference's.

    PYTHONDONTWRITEBYTECODE=1 python tests/gen_mqmha_golden.py [case ...]
"""

import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import gen_golden as G  # noqa: E402

SMALL = "ecapa_params={'channels':512,'embd_dim':%d,'mfa_conv':%d}"
CASES = {
    # the reference's current ECAPA recipe (launcher/runEcapaXvector_roadmap.py:228-250) on the 512-channel trunk
    "ecapa_mqmha_roadmap": dict(blueprint="ecapa_tdnn_xvector.py",
                                creation="ECAPA_TDNN(80,10,training=False,pooling='mqmha',pooling_params={'hidden_size':64,'num_q':2,'share':False,"
                                         "'num_head':2,'affine_layers':2,'time_attention':True,'stddev':True},%s,%s)" % (SMALL % (192, 1536), G.LAUNCHER_FC2),
                                dim=80, utts=[(300, 7000), (150, 7001), (37, 7002), (2, 7003), (1, 7004)], wseed=31),
    # shared logits (one per head, query and frame), one affine layer, no time attention, three queries, fc1 + "far"
    "ecapa_mqmha_shared": dict(blueprint="ecapa_tdnn_xvector.py",
                               creation="ECAPA_TDNN(40,10,training=False,pooling='mqmha',pooling_params={'share':True,'num_head':4,'num_q':3,"
                                        "'affine_layers':1,'time_attention':False},%s,fc1=True,extracted_embedding='far')" % (SMALL % (128, 768)),
                               dim=40, utts=[(200, 7100), (41, 7101), (3, 7102)], wseed=32),
    # one head, one query, un-shared; the blueprint's defaults for the rest (hidden 128, two layers, time attention)
    "ecapa_mqmha_q1": dict(blueprint="ecapa_tdnn_xvector.py",
                           creation="ECAPA_TDNN(80,10,training=False,pooling='mqmha',pooling_params={'num_q':1,'num_head':1,'share':False},"
                                    "ecapa_params={'channels':512,'mfa_conv':768},extracted_embedding='near_affine')",
                           dim=80, utts=[(150, 7200), (20, 7201)], wseed=33),
}


def bind_compute_statistics():
    import importlib.util
    import libs.nnet.pooling as ref_pooling
    spec = importlib.util.spec_from_file_location("ref_transformer_xvector", os.path.join(G.REF, "pytorch", "model", "transformer_xvector.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    ref_pooling.compute_statistics = lambda x, m, stddev=True: tuple(
        t.unsqueeze(-1) if t.numel() else t for t in ref.compute_statistics(x, m, dim=x.dim() - 1, stddev=stddev))


def main(argv):
    if not os.path.isdir(G.REF):
        sys.exit("gen_mqmha_golden.py needs the reference tree at %s (build container only)" % G.REF)
    G.install_shims()
    sys.path.insert(0, os.path.join(G.REF, "pytorch"))
    os.makedirs(G.GOLDEN, exist_ok=True)
    synth = G.load_synth()
    bind_compute_statistics()
    for name in argv or list(CASES):
        G.run_extractor_case(name, CASES[name], synth, os.path.join(G.GOLDEN, name + ".npz"))


if __name__ == "__main__":
    main(sys.argv[1:])
