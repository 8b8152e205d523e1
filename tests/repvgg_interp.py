"""numpy interpreter of a traced RepVGG / RepSPK program (TEST INFRASTRUCTURE): tests/ir_interp.py plus the 'grid_conv' op.

A tap (dt, df) of a grid convolution is the row offset dt * pitch + df of the grid's row layout (frequency fastest, `pitch` rows per
frame, the rows behind the `width` bins zero), so the op is a tap-by-tap layer of ir_interp with those offsets - which reads zeros
outside the utterance and, on a reach-2 grid (pitch >= width + 2), in the pad rows a frequency offset of +-2 lands in.  A tap that
wrapped into the neighbouring frame instead would read real values there: the interpreter, like the device, has no mask for it."""

import numpy as np

import ir_interp
from libs.amd import ir as _ir


def grid_conv_as_layer(graph, op):
    """The 'grid_conv' op as the 'tdnn' op ir_interp runs: sorted row offsets, dense [out, in, span] kernel, bias, activation."""
    pitch = graph.grid_spec(op.inp.tid)[3]
    offs = [dt * pitch + df for dt, df in op.taps]
    left = min(offs)
    dense = np.zeros(op.weight.shape[:2] + (max(offs) - left + 1,), dtype=op.weight.dtype)
    for k, o in enumerate(offs):
        dense[:, :, o - left] = op.weight[:, :, k]
    return _ir.Op("tdnn", op.out, inp=op.inp, inp2=None, weight=dense, bias=op.bias, taps=sorted(offs), w_left=left, act1=op.act, scale=None, shift=None,
                  affine_first=False, act2=None, seg_bias=None, seg_scale=None, res=None)


def lowered_ops(graph, ops=None):
    return [grid_conv_as_layer(graph, op) if op.kind == "grid_conv" else op for op in (graph.ops if ops is None else ops)]


def run_graph(graph, feats, dtype=np.float64, ops=None):
    return ir_interp.run_graph(graph, feats, dtype, lowered_ops(graph, ops))


def extract(graph, feats, max_chunk=10000, dtype=np.float64, ops=None):
    return ir_interp.extract(graph, feats, max_chunk, dtype, lowered_ops(graph, ops))


# ------------------------------------------------------------------------------------------ the 16-bit modes, emulated
#
# What the 16-bit precision modes round, restated on [T, F, C] maps in float64 arithmetic: the features and every grid tensor are
# stored in the element type (ties to even), the weights of the grid layers are rounded to it once, products are exact and sums
# are f32-or-better; the pooled tail (per-bin statistics, the embedding layers) runs in f32 on the device and is left unrounded
# here.  The cosine between this evaluation and the float64 one is the loss the number format itself causes on a fixture - the
# yardstick the device's 16-bit results are held to (tests/test_gpu_repvgg.py).

def run_graph_rounded(graph, feats, et):
    """One utterance through a statistics-pooling RepVGG / RepSPK program with the roundings of the 16-bit mode `et` ('bf16' | 'f16';
    'f64': none).  Ops: grid_input, grid_conv, im2col (the stride-2 gathers), tdnn (grid layers and the pooled tail), per-bin pool."""
    from conv_cases import conv_map
    from pool_cases import round_to
    rnd = (lambda a: np.asarray(a, dtype=np.float64)) if et == "f64" else (lambda a: round_to(a, et).astype(np.float64))
    maps = {}

    def decode(op):
        pitch = graph.grid_spec(op.inp.tid)[3]
        pos = []
        for off in op.taps:
            a = int(np.rint(off / float(pitch)))
            pos.append((a, off - a * pitch))
        return pos, np.stack([op.weight[:, :, off - op.w_left] for off in op.taps], axis=2)

    for op in graph.ops:
        if op.kind == "grid_input":
            maps[op.out.tid] = rnd(feats)[:, :, None]
        elif op.kind == "grid_conv":
            z = conv_map(maps[op.inp.tid], rnd(op.weight), op.taps) + (0 if op.bias is None else op.bias.astype(np.float64))
            maps[op.out.tid] = rnd(np.maximum(z, 0) if op.act == "relu" else z)
        elif op.kind == "im2col":
            x = maps[op.inp.tid]
            T, F, C = x.shape
            To, Fo = (T + 1) // 2, (F + 1) // 2
            assert op.stride == 2 and getattr(op, "b", None) is None
            out = np.zeros((To, Fo, C * len(op.taps)))
            for k, (dt, df) in enumerate(op.taps):            # out[t', f'] = x[2 t' + dt, 2 f' + df], zeros outside the map
                ti, fi = 2 * np.arange(To) + dt, 2 * np.arange(Fo) + df
                tv, fv = (ti >= 0) & (ti < T), (fi >= 0) & (fi < F)
                out[np.ix_(np.flatnonzero(tv), np.flatnonzero(fv), np.arange(k * C, (k + 1) * C))] = x[np.ix_(ti[tv], fi[fv])]
            maps[op.out.tid] = out
        elif op.kind == "tdnn" and graph.grid_spec(op.inp.tid) is not None:
            assert op.scale is None and op.inp2 is None and op.res is None and op.seg_scale is None and op.seg_bias is None
            pos, w = decode(op)
            z = conv_map(maps[op.inp.tid], rnd(w), pos) + op.bias.astype(np.float64)
            maps[op.out.tid] = rnd(np.maximum(z, 0) if op.act1 == "relu" else z)
        elif op.kind == "pool":
            assert op.per_bin and op.stddev
            x = maps[op.inp.tid]
            mean = x.mean(axis=0)
            var = ((x - mean) ** 2).sum(axis=0) / float(x.shape[0] - 1 if (op.unbiased == 1 and x.shape[0] > 1) else x.shape[0])
            maps[op.out.tid] = np.concatenate([mean, np.sqrt(np.maximum(var, op.eps))], axis=1).reshape(-1)      # bin f: [mean | std]
        elif op.kind == "tdnn":
            z = op.weight[:, :, 0].astype(np.float64) @ maps[op.inp.tid] + (0 if op.bias is None else op.bias.astype(np.float64))
            s = 1 if op.scale is None else op.scale.astype(np.float64)
            t = 0 if op.shift is None else op.shift.astype(np.float64)
            z = ir_interp._act(z * s + t, op.act1) if op.affine_first else ir_interp._act(z, op.act1) * s + t
            maps[op.out.tid] = ir_interp._act(z, op.act2)
        else:
            raise AssertionError("run_graph_rounded: unexpected op %s" % op.kind)
    return maps[graph.output.tid][:graph.output.channels]
