#!/usr/bin/env python3
"""Workload for profiling the multi-query multi-head attentive pooling: ECAPA-TDNN at the BASELINE shape (channels 1024, MFA 1536) with
the reference recipe's pooling (num_q 2, num_head 2, hidden 64, un-shared logits, two layers, time attention), 256 utterances of 300
frames, synthetic weights.  Run it under `rocprofv3 --kernel-trace --stats`, once as it is (one mq_attentive_pool_kernel launch per
extraction) and once with ASV_AMD_MQPOOL=0 (four attentive_pool_kernel launches):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/mqpool_profile_workload.py bf16
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "asv-subtools_amd", "pytorch"), os.path.join(REPO, "tests")]


def main(precision, steps=12):
    import torch
    import helpers
    from libs.amd import synth
    model = helpers.build_model("ecapa_tdnn_xvector.py", "ECAPA_TDNN(80,10,training=False,pooling='mqmha',pooling_params={'hidden_size':64,'num_q':2,"
                                "'share':False,'num_head':2,'affine_layers':2,'time_attention':True,'stddev':True})")
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 31).items()})
    model.cuda()
    model.amd_precision = precision
    eng = model._amd_engine()
    feats = torch.from_numpy(np.concatenate([synth.synth_feats(300, 80, 7500 + i) for i in range(256)])).cuda()
    offsets = np.arange(257, dtype=np.int32) * 300
    for _ in range(steps):
        out = eng.extract_device(feats, offsets)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    print("%s mqpool=%s: %d extractions of 256 x 300 frames; pooling ops: %s" % (
        precision, os.environ.get("ASV_AMD_MQPOOL", "1"), steps, [op.kind for op in eng.ops if "pool" in op.kind]))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "bf16")
