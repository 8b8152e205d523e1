#!/usr/bin/env python3
"""Generate tests/golden/repvgg_*.npz by running the REFERENCE's RepVggXvector (model/repvgg_xvector.py, libs/nnet/repvgg.py) on
CPU.  Build container only (needs the reference tree, like oracle/gen_golden.py, whose shims and synthetic weights this file
uses).  Outputs only, as every other extractor fixture; the cases and what a fixture holds beyond the usual: tests/repvgg_cases.py.

Per case the generator records the largest magnitude ANY module of the reference produces on the fixture's utterances (forward
hooks on every module, the branch outputs a fused block never forms included) and refuses to write a fixture that does not stay
below the f32m range limit with a factor-4 margin: the tests assert status() == 0 on these fixtures.

    PYTHONDONTWRITEBYTECODE=1 python tests/gen_repvgg_golden.py [case ...]
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
import repvgg_cases as RC  # noqa: E402


def run_case(name, case, synth):
    import numpy as np
    import torch
    import libs.support.utils as utils                     # the reference's (G.REF/pytorch is first on sys.path)
    from libs.nnet.repvgg import repvgg_model_convert      # likewise

    torch.set_num_threads(os.cpu_count() or 1)
    blueprint = os.path.join(G.REF, "pytorch", "model", RC.BLUEPRINT)
    training_creation = case.get("from_training")
    model = utils.create_model_from_py(blueprint, training_creation or case["creation"])
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = RC.scaled_state_dict(synth, shapes, case["wseed"], case["gamma_scale"])
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    if training_creation:
        model = repvgg_model_convert(model)
        want = utils.create_model_from_py(blueprint, case["creation"])      # the deploy form as constructed: same keys and shapes
        assert {k: tuple(v.shape) for k, v in want.state_dict().items()} == {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.eval()
    peak = [0.0]

    def hook(mod, inputs, output):
        if isinstance(output, torch.Tensor) and output.numel():
            peak[0] = max(peak[0], float(output.detach().abs().max()))

    handles = [m.register_forward_hook(hook) for m in model.modules()]
    embs = []
    for (T, seed) in case["utts"]:
        x = synth.synth_feats(T, case["dim"], seed)
        peak[0] = max(peak[0], float(np.abs(x).max()))
        embs.append(model.extract_embedding(x).numpy().astype(np.float32))
    for h in handles:
        h.remove()
    embs = np.stack(embs)
    assert np.isfinite(embs).all(), name
    print("%s: largest activation %.4g, largest embedding value %.4g" % (name, peak[0], float(np.abs(embs).max())))
    if peak[0] * RC.RANGE_MARGIN >= RC.RANGE_LIMIT:
        sys.exit("%s: activations reach %.4g: not a factor %g below the f32m range limit %g - lower gamma_scale" % (name, peak[0], RC.RANGE_MARGIN, RC.RANGE_LIMIT))
    out = dict(
        embeddings=embs, utts=np.asarray(case["utts"], dtype=np.int64), wseed=np.int64(case["wseed"]), dim=np.int64(case["dim"]),
        creation=np.array(case["creation"]), blueprint=np.array(RC.BLUEPRINT),
        shape_keys=np.array(list(shapes.keys())), shape_vals=np.array([",".join(str(d) for d in s) for s in shapes.values()]),
        torch_version=np.array(torch.__version__),
        gamma_scale=np.float64(case["gamma_scale"]), max_activation=np.float64(peak[0]),
        from_training=np.int64(1 if training_creation else 0), training_creation=np.array(training_creation or ""),
    )
    if training_creation:
        dk = model.state_dict()
        out["deploy_keys"] = np.array(list(dk.keys()))
        out["deploy_shapes"] = np.array([",".join(str(d) for d in v.shape) for v in dk.values()])
    path = os.path.join(G.GOLDEN, name + ".npz")
    np.savez_compressed(path, **out)
    print("wrote %s: embeddings %s" % (path, embs.shape))


def main(argv):
    if not os.path.isdir(G.REF):
        sys.exit("gen_repvgg_golden.py needs the reference tree at %s (build container only)" % G.REF)
    G.install_shims()
    sys.path.insert(0, os.path.join(G.REF, "pytorch"))
    os.makedirs(G.GOLDEN, exist_ok=True)
    synth = G.load_synth()
    for name in argv or list(RC.CASES):
        run_case(name, RC.CASES[name], synth)


if __name__ == "__main__":
    main(sys.argv[1:])
