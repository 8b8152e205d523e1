#!/usr/bin/env python3
"""Generate tests/golden/transformer_*.npz by running the REFERENCE's TransformerXvector (model/transformer_xvector.py,
libs/nnet/transformer/) on CPU.  Build container only (needs the reference tree, like oracle/gen_golden.py, whose shims and
synthetic weights this file uses).  Outputs only, as every other extractor fixture; the cases: tests/transformer_cases.py.

Per case the generator records the reference's state-dict keys and shapes and the largest magnitude ANY module of the reference
produces on the fixture's utterances (forward hooks on every module), and refuses to write a fixture that does not stay below the
f32m range limit with a factor-4 margin - the tests assert status() == 0 on these fixtures - or whose embeddings are not finite.

    PYTHONDONTWRITEBYTECODE=1 python tests/gen_transformer_golden.py [case ...]
"""

import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from oracle import gen_golden as G  # noqa: E402
import transformer_cases as TC  # noqa: E402


def run_case(name, case, synth):
    import numpy as np
    import torch
    import libs.support.utils as utils                     # the reference's (G.REF/pytorch is first on sys.path)

    torch.set_num_threads(min(16, os.cpu_count() or 1))
    blueprint = os.path.join(G.REF, "pytorch", "model", TC.BLUEPRINT)
    model = utils.create_model_from_py(blueprint, case["creation"])
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = synth.synth_state_dict(shapes, case["wseed"])
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model.eval()
    peak = [0.0]

    def hook(mod, inputs, output):
        for o in (output if isinstance(output, (tuple, list)) else (output,)):
            if isinstance(o, torch.Tensor) and o.numel() and o.is_floating_point():
                peak[0] = max(peak[0], float(o.detach().abs().max()))

    handles = [m.register_forward_hook(hook) for m in model.modules()]
    embs = []
    for (T, seed) in case["utts"]:
        x = synth.synth_feats(T, case["dim"], seed)
        peak[0] = max(peak[0], float(np.abs(x).max()))
        embs.append(model.extract_embedding(x).numpy().astype(np.float32))
    for h in handles:
        h.remove()
    embs = np.stack(embs)
    if not np.isfinite(embs).all():
        sys.exit("%s: the reference's embeddings are not finite" % name)
    print("%s: %d parameters, %d keys, largest activation %.4g, largest embedding value %.4g"
          % (name, sum(int(np.prod(s)) for s in shapes.values()), len(shapes), peak[0], float(np.abs(embs).max())))
    if peak[0] * TC.RANGE_MARGIN >= TC.RANGE_LIMIT:
        sys.exit("%s: activations reach %.4g: not a factor %g below the f32m range limit %g" % (name, peak[0], TC.RANGE_MARGIN, TC.RANGE_LIMIT))
    path = os.path.join(G.GOLDEN, name + ".npz")
    np.savez_compressed(
        path, embeddings=embs, utts=np.asarray(case["utts"], dtype=np.int64), wseed=np.int64(case["wseed"]), dim=np.int64(case["dim"]),
        creation=np.array(case["creation"]), blueprint=np.array(TC.BLUEPRINT),
        shape_keys=np.array(list(shapes.keys())), shape_vals=np.array([",".join(str(d) for d in s) for s in shapes.values()]),
        torch_version=np.array(torch.__version__), max_activation=np.float64(peak[0]))
    print("wrote %s: embeddings %s" % (path, embs.shape))


def main(argv):
    if not os.path.isdir(G.REF):
        sys.exit("gen_transformer_golden.py needs the reference tree at %s (build container only)" % G.REF)
    G.install_shims()
    sys.path.insert(0, os.path.join(G.REF, "pytorch"))
    os.makedirs(G.GOLDEN, exist_ok=True)
    synth = G.load_synth()
    for name in argv or list(TC.CASES):
        run_case(name, TC.CASES[name], synth)


if __name__ == "__main__":
    main(sys.argv[1:])
