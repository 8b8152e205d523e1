"""The transformer x-vector fixtures (tests/golden/transformer_*.npz, written by tests/gen_transformer_golden.py) and how a test
rebuilds their models (TEST INFRASTRUCTURE, shared by the generator and the tests).

A fixture holds the reference's outputs (CPU, float32), the case description, the reference's state-dict keys and shapes, and
`max_activation`: the largest magnitude any module of the reference produced on the fixture's utterances (forward hooks), which the
generator requires to stay a factor RANGE_MARGIN below the range limit of the f32m operand split - so the tests can assert that no
range bit was raised.  The weights are regenerated from `wseed` (libs.amd.synth: LayerNorm gammas and betas are randomised like
every other 1-D weight / bias, there is no BatchNorm in this blueprint)."""

RANGE_LIMIT = 57344.0          # beyond it the 8-bit half of the f32m operand split has no finite value (device_utils.h mx_range_bits)
RANGE_MARGIN = 4.0
BLUEPRINT = "transformer_xvector.py"

_SMALL = ("transformer_type='transformer',transformer_params={'attention_dim':64,'attention_heads':2,'num_blocks':2,'linear_units':128,%s},"
          "tansformer_out={'out_dim':96},pooling_params={'hidden_size':32%s},embd_dim=64")
_LIN = _SMALL % ("'input_layer':'linear','pos_enc_type':'no_pos'", "")
_CONV = _SMALL % ("'input_layer':'conv2d','pos_enc_type':'abs_pos','activation_type':'swish'", ",'time_attention':True")

CASES = {
    # per-frame linear input layer, no positions: 300-row sequences per default chunk; T = 301 runs as chunks of 150 / 151
    "transformer_lin_small": dict(creation="TransformerXvector(40,10,training=False,%s)" % _LIN, dim=40,
                                  utts=[(2, 9600), (37, 9601), (65, 9602), (130, 9603), (301, 9604)], wseed=71),
    # the unpadded stride-2 front, absolute positions, the pooling's time attention, a row-op activation in the feed-forward;
    # T = 7 owns one row, T = 650 runs as three chunks
    "transformer_conv_small": dict(creation="TransformerXvector(40,10,training=False,%s)" % _CONV, dim=40,
                                   utts=[(7, 9700), (8, 9701), (11, 9702), (37, 9703), (301, 9704), (650, 9705)], wseed=72),
    # the blueprint's defaults behind transformer_type='transformer': 80 bins, d = 256, 4 heads, 6 blocks, 2048 units, out_dim 1536
    "transformer_default": dict(creation="TransformerXvector(80,10,training=False,transformer_type='transformer')", dim=80,
                                utts=[(37, 9800), (200, 9801), (301, 9802)], wseed=73),
    # fc1 and the 'far' position on the small conv model
    "transformer_far": dict(creation="TransformerXvector(40,10,training=False,fc1=True,extracted_embedding='far',%s)" % _CONV, dim=40,
                            utts=[(37, 9900)], wseed=74),
}


def golden_model(name):
    """(fixture, shapes, model of THIS package with the fixture's weights)."""
    import helpers
    from libs.amd import synth
    g, shapes = helpers.load_golden(name)
    sd = synth.synth_state_dict(shapes, int(g["wseed"]))
    return g, shapes, helpers.build_model(BLUEPRINT, str(g["creation"]), sd)
