"""The RepVGG / RepSPK fixtures (tests/golden/repvgg_*.npz, written by tests/gen_repvgg_golden.py) and how a test rebuilds their
models (TEST INFRASTRUCTURE, shared by the generator and the tests).

A fixture holds the reference's outputs, the case description and two things the other extractor fixtures do not have:
  gamma_scale   the constant the synthesised BatchNorm gammas of the trunk (`repvgg.*.bn.weight`, `repvgg.*.rbr_identity.weight`) are
                multiplied by.  Three summed branches per block let the activations of a default-depth trunk grow to ~1e6 with the
                plain synthetic weights - beyond the range of the IEEE-half operand split of the default precision mode; the damped
                trunk stays far inside it, so the tests can assert that no range bit was raised.
  from_training 1: `shape_keys` describe the TRAINING form; the model under test is that checkpoint converted to the deploy form
                (the generator used the reference's repvgg_model_convert, the tests use this package's).
  max_activation  the largest magnitude any module of the reference produced on the fixture's utterances (forward hooks).
"""

import numpy as np

RANGE_LIMIT = 57344.0          # beyond it the 8-bit half of the f32m operand split has no finite value (device_utils.h mx_range_bits)
RANGE_MARGIN = 4.0

SMALL = "repvgg_config={'repvgg_params':{'num_blocks':[1,2,2,1]}%s}"
UTTS5 = lambda seed: [(200, seed), (37, seed + 1), (9, seed + 2), (2, seed + 3), (1, seed + 4)]

CASES = {
    # RepSPK blocks (the blueprint's default block), a [1, 2, 2, 1] trunk over 40 bins
    "repvgg_spk_small": dict(creation="RepVggXvector(40,10,training=False,%s)" % (SMALL % ""), dim=40, utts=UTTS5(9100), wseed=61, gamma_scale=1.0),
    # RepVGG blocks, the same trunk
    "repvgg_vgg_small": dict(creation="RepVggXvector(40,10,training=False,%s)" % (SMALL % ",'block':'RepVGG'"), dim=40, utts=UTTS5(9200), wseed=62,
                             gamma_scale=1.0),
    # the deploy form of repvgg_spk_small's checkpoint
    "repvgg_spk_deploy": dict(creation="RepVggXvector(40,10,training=False,deploy=True,%s)" % (SMALL % ""), dim=40, utts=UTTS5(9100), wseed=61,
                              gamma_scale=1.0, from_training="RepVggXvector(40,10,training=False,%s)" % (SMALL % "")),
    # the blueprint's defaults: RepSPK [2, 4, 14, 1], base width 32, 80 bins; damped (see above)
    "repvgg_spk_default": dict(creation="RepVggXvector(80,10,training=False)", dim=80, utts=[(120, 9300), (64, 9301), (9, 9302)], wseed=63, gamma_scale=0.6),
    # a frame-weighting pooling behind the trunk, and fc1.  The attentive pooling forms its variance as sum a x^2 - mean^2 in float32
    # (pooling.py), which cancels badly on some short utterances: the 33-frame utterance is one whose float32 and float64 evaluations
    # of the same program agree to 4e-6 (seed 9401 at that length: 2.5e-4, more than the 1e-4 gate the fixture is held to)
    "repvgg_spk_attentive": dict(creation="RepVggXvector(40,10,training=False,pooling='attentive',pooling_params={'hidden_size':32,'context':[-1,0,1]},"
                                          "fc1=True,%s)" % (SMALL % ""), dim=40, utts=[(150, 9400), (33, 9403), (9, 9402)], wseed=64, gamma_scale=1.0),
}
BLUEPRINT = "repvgg_xvector.py"


def is_trunk_gamma(key):
    return key.startswith("repvgg.") and (key.endswith(".bn.weight") or key.endswith(".rbr_identity.weight"))


def scaled_state_dict(synth, shapes, wseed, gamma_scale):
    """The synthetic state dict of a fixture: libs.amd.synth's recipe with the trunk's BatchNorm gammas damped."""
    sd = synth.synth_state_dict(shapes, int(wseed))
    if float(gamma_scale) != 1.0:
        for k in sd:
            if is_trunk_gamma(k):
                sd[k] = (sd[k] * np.float32(gamma_scale)).astype(np.float32)
    return sd


def golden_model(name):
    """(fixture, model of THIS package with the fixture's weights) - for a from_training fixture the training-form model converted by
    libs.nnet.repvgg.repvgg_model_convert."""
    import helpers
    from libs.amd import synth
    g, shapes = helpers.load_golden(name)
    sd = scaled_state_dict(synth, shapes, int(g["wseed"]), float(g["gamma_scale"]))
    if int(g["from_training"]):
        from libs.nnet.repvgg import repvgg_model_convert
        model = repvgg_model_convert(helpers.build_model(BLUEPRINT, str(g["training_creation"]), sd), do_copy=False)
        model.eval()
        return g, model
    return g, helpers.build_model(BLUEPRINT, str(g["creation"]), sd)
