"""The row op (asv_rowop_desc_t, csrc/kernels_rowop.hip) alone: its numpy model, the one-op cases, their inputs, references
and error measures (TEST INFRASTRUCTURE, shared by tests/test_rowop_host.py, tests/rowop_interp.py and
tests/test_gpu_rowop_kernel.py).

Model      rowop_model(z, op fields, dtype): z * scale0 + shift0 -> act0 -> LayerNorm over the channels (biased variance)
           -> act1 -> z * scale1 + shift1, every step optional, in `dtype` (float64: the reference of the GPU test).  GELU is
           evaluated as 0.5 x erfc(-x / sqrt 2) - the same function as 0.5 x (1 + erf(x / sqrt 2)), without its cancellation
           in the negative tail, where the 16-bit gate (one unit in the last place of the RESULT) needs a relative reference.
Inputs     3 N(0,1) with the values 0, +-20.5, +-30, +-88, +-100 planted in different rows, one row of mean 100 and deviation 1,
           one constant row.  The constant is 0.71875 = 23 / 32: sums of up to 3000 copies are exact in f32 in any order, so the
           row's variance is exactly 0 on every implementation and the row checks the eps path alone.  Everything is rounded to
           the element type first: the device's conversion is exact and the reference sees the kernel's numbers.
           Columns of the buffer outside the view hold FILL.
Parameters scale U(0.5, 1.5), shift 0.5 N(0,1) (a folded eval BatchNorm); gamma U(0.5, 1.5), beta 0.2 N(0,1) (libs/amd/synth.py).
Gates      f32 buffers: e = max |y - y64| / max |y64| per case; e_dev <= 4 e_ref + 2^-24 with e_ref torch's float32 CPU result.
           16-bit buffers: every element within one unit in the last place of round(y64) in that type.
"""

import functools
import math
import os
import zlib

import numpy as np

ELEM_TYPES = ("f32", "bf16", "f16")
FRAME_LENGTHS = (1, 2, 37, 64, 65)                  # 169 rows: a multiple of no block size
UTT_ROWS = 5
PLANTED = (0.0, 20.5, -20.5, 30.0, -30.0, 88.0, -88.0, 100.0, -100.0)
CONST = 0.71875
FILL = 7.0
LEAKY_SLOPE = 0.2
SELU_ALPHA, SELU_SCALE = 1.6732632423543772848170429916717, 1.0507009873554804934193349852946
NEW_ACTS = ("leaky_relu", "selu", "mish", "swish", "gelu", "double_swish")

# (name, domain, channels, buffer width, channel offset of the view, in place)
LAYOUTS = (
    ("c16", "frames", 16, 32, 0, False),            # 4 lanes (f32) / 2 lanes (16-bit) per row: 16 / 32 rows share a wave
    ("c48", "frames", 48, 48, 0, False),            # 12 / 6 pieces: a group of 16 / 8 lanes, partly filled
    ("c48_inplace", "frames", 48, 48, 0, True),
    ("c48_off16", "frames", 48, 96, 16, False),     # a view inside a wider buffer
    ("c1500", "frames", 1500, 1500, 0, False),      # pitch 1504: the statistics must not see the padding; 375 / 188 pieces
    ("c3000_utts", "utts", 3000, 3000, 0, False),   # 12 pieces per lane, f32 rows (the utts domain is always f32)
)

# op name -> fields of the op (tables are drawn per case)
OPS = dict([(a, dict(act0=a)) for a in NEW_ACTS] + [
    ("ln", dict(ln=True)),
    ("ln_affine", dict(ln=True, ln_affine=True)),
    ("mish_ln", dict(act0="mish", ln=True, ln_affine=True)),               # act -> LN
    ("ln_selu", dict(ln=True, ln_affine=True, act1="selu")),               # LN -> act
    ("affine_dswish", dict(affine0=True, act0="double_swish")),            # affine -> act (the "bn-relu" order)
    ("swish_affine", dict(act0="swish", affine1=True)),                    # act -> affine (act -> BatchNorm)
])


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def round_to(a, et):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if et == "f32":
        return a
    import torch
    return torch.from_numpy(a).to({"bf16": torch.bfloat16, "f16": torch.float16}[et]).float().numpy()


# ------------------------------------------------------------------------------------------ the model

def _erfc(x):
    import torch
    return torch.erfc(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))).numpy().astype(x.dtype)


def act_model(x, name, slope=0.01):
    """Activation `name` on a numpy array, in the array's dtype; finite for every finite x."""
    if not name:
        return x
    one = x.dtype.type(1)
    with np.errstate(over="ignore", under="ignore"):
        if name == "relu":
            return np.maximum(x, 0)
        if name == "tanh":
            return np.tanh(x)
        if name == "sigmoid":
            return one / (one + np.exp(-x))
        if name == "leaky_relu":
            return np.where(x > 0, x, x * x.dtype.type(slope))
        if name == "selu":
            return x.dtype.type(SELU_SCALE) * np.where(x > 0, x, x.dtype.type(SELU_ALPHA) * np.expm1(np.minimum(x, 0)))
        if name == "mish":
            sp = np.where(x > 20, x, np.log1p(np.exp(np.minimum(x, 20))))
            return x * np.tanh(sp)
        if name == "swish":
            return x / (one + np.exp(-x))
        if name == "gelu":
            return x.dtype.type(0.5) * x * _erfc(-x * x.dtype.type(math.sqrt(0.5)))
        if name == "double_swish":
            return x / (one + np.exp(one - x))
    raise AssertionError("unknown activation %r" % (name,))


def rowop_model(z, dtype=np.float64, act0=None, slope0=0.01, ln=False, eps=1e-5, gamma=None, beta=None, act1=None, slope1=0.01,
                scale0=None, shift0=None, scale1=None, shift1=None):
    """[rows, C] -> [rows, C] in `dtype`."""
    z = np.asarray(z, dtype=dtype)
    t = lambda a: np.asarray(a, dtype=dtype)
    if scale0 is not None:
        z = z * t(scale0) + t(shift0)
    z = act_model(z, act0, slope0)
    if ln:
        mu = z.mean(axis=1, keepdims=True, dtype=dtype)
        d = z - mu
        var = (d * d).mean(axis=1, keepdims=True, dtype=dtype)
        z = d / np.sqrt(var + dtype(eps))
        if gamma is not None:
            z = z * t(gamma) + t(beta)
    z = act_model(z, act1, slope1)
    if scale1 is not None:
        z = z * t(scale1) + t(shift1)
    return z.astype(dtype)


def rowop_torch(z, dtype, act0=None, slope0=0.01, ln=False, eps=1e-5, gamma=None, beta=None, act1=None, slope1=0.01,
                scale0=None, shift0=None, scale1=None, shift1=None):
    """The same op from torch's own modules / functionals on the CPU, in torch dtype `dtype`: LeakyReLU, SELU, SiLU, F.gelu
    (exact), x * tanh(softplus(x)), x * sigmoid(x - 1), F.layer_norm."""
    import torch
    import torch.nn.functional as F
    z = torch.from_numpy(np.array(z)).to(dtype)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)

    def act(x, name, slope):
        if not name:
            return x
        return {"relu": torch.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid, "leaky_relu": torch.nn.LeakyReLU(negative_slope=slope),
                "selu": torch.nn.SELU(), "mish": lambda v: v * torch.tanh(F.softplus(v)), "swish": torch.nn.SiLU(), "gelu": F.gelu,
                "double_swish": lambda v: v * torch.sigmoid(v - 1.0)}[name](x)
    if scale0 is not None:
        z = z * t(scale0) + t(shift0)
    z = act(z, act0, slope0)
    if ln:
        z = F.layer_norm(z, (z.shape[1],), None if gamma is None else t(gamma), None if beta is None else t(beta), eps)
    z = act(z, act1, slope1)
    if scale1 is not None:
        z = z * t(scale1) + t(shift1)
    return z.numpy()


# ------------------------------------------------------------------------------------------ cases

class Case(object):
    def __init__(self, layout, op):
        self.layout, self.op = layout, op
        self.lname, self.domain, self.channels, self.width, self.ch_off, self.inplace = layout

    @property
    def name(self):
        return "%s-%s" % (self.lname, self.op)

    __repr__ = name.fget

    @property
    def elem_types(self):
        return ELEM_TYPES if self.domain == "frames" else ("f32",)

    @property
    def lengths(self):
        return FRAME_LENGTHS if self.domain == "frames" else (1,) * UTT_ROWS


def all_cases():
    return [Case(l, op) for l in LAYOUTS for op in OPS]


@functools.lru_cache(maxsize=None)
def _inputs(lname, et):
    """The buffer [rows, width] of a layout, rounded to `et` (one per layout and type, shared by its ops; read-only)."""
    layout = [l for l in LAYOUTS if l[0] == lname][0]
    _, domain, C, width, off, _ = layout
    rows = sum(FRAME_LENGTHS) if domain == "frames" else UTT_ROWS
    rng = _rng("rowop-x", lname)
    buf = np.full((rows, width), FILL, dtype=np.float64)
    x = 3.0 * rng.randn(rows, C)
    r_mean, r_const = (rows - 2, rows - 1) if domain == "utts" else (40, 104)
    free = [r for r in range(rows) if r not in (r_mean, r_const)]
    for k, v in enumerate(PLANTED):                              # every planted value in another row where there are enough
        x[free[(7 * k + 3) % len(free)], (5 * k + 1) % C] = v
    x[r_mean] = 100.0 + rng.randn(C)
    x[r_const] = CONST
    buf[:, off:off + C] = x
    out = round_to(buf, et)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _fields(lname, op):
    layout = [l for l in LAYOUTS if l[0] == lname][0]
    C = layout[2]
    spec = dict(OPS[op])
    rng = _rng("rowop-p", lname, op)
    f = dict(act0=spec.get("act0"), act1=spec.get("act1"), slope0=LEAKY_SLOPE, slope1=LEAKY_SLOPE, ln=bool(spec.get("ln")), eps=1e-5)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    if spec.get("ln_affine"):
        f["gamma"], f["beta"] = f32(rng.uniform(0.5, 1.5, C)), f32(0.2 * rng.randn(C))
    for k in ("0", "1"):
        if spec.get("affine" + k):
            f["scale" + k], f["shift" + k] = f32(rng.uniform(0.5, 1.5, C)), f32(0.5 * rng.randn(C))
    return f


def fields(case):
    """The op's fields (rowop_model keywords); leave the arrays unchanged."""
    return dict(_fields(case.lname, case.op))


def inputs(case, et):
    return _inputs(case.lname, et)


@functools.lru_cache(maxsize=None)
def _reference64(lname, op, et):
    case = Case([l for l in LAYOUTS if l[0] == lname][0], op)
    x = inputs(case, et)[:, case.ch_off:case.ch_off + case.channels]
    ref = rowop_model(x, np.float64, **fields(case))
    ref.setflags(write=False)
    return ref


def reference64(case, et):
    """float64 result [rows, C] of the case on the inputs rounded to `et` (computed once, read-only)."""
    return _reference64(case.lname, case.op, et)


def reference_torch32(case, et):
    import torch
    x = inputs(case, et)[:, case.ch_off:case.ch_off + case.channels]
    return rowop_torch(x, torch.float32, **fields(case))


# ------------------------------------------------------------------------------------------ error measures

def max_err(y, y64):
    """max |y - y64| / max |y64| over the case."""
    y, y64 = np.asarray(y, dtype=np.float64), np.asarray(y64, dtype=np.float64)
    return float(np.abs(y - y64).max() / np.abs(y64).max())


def ulp_distance(got, y64, et):
    """Per element: units in the last place of the 16-bit type between `got` (values of that type, held as f32) and y64 rounded to
    it.  +0 and -0 are the same value."""
    import torch
    dt = {"bf16": torch.bfloat16, "f16": torch.float16}[et]

    def ordinal(a, dtype64):
        t = torch.from_numpy(np.array(a, dtype=np.float64 if dtype64 else np.float32)).to(dt)
        bits = t.view(torch.int16).numpy().astype(np.int64) & 0xFFFF
        mag = bits & 0x7FFF
        return np.where(bits & 0x8000, -mag, mag)
    g32 = np.ascontiguousarray(got, dtype=np.float32)
    assert np.array_equal(round_to(g32, et), g32), "the device's values are not values of the element type"
    return np.abs(ordinal(g32, False) - ordinal(y64, True))


# ------------------------------------------------------------------------------------------ model fixtures (tests/gen_rowop_golden.py)

LX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rowop_blueprint.py")
# fixture -> the row ops of its program, in order: (act0, slope0, ln, has gamma / beta, act1, has scale1 / shift1, utts domain)
F, U = False, True
FIXTURES = {
    "rowop_xvector_swish": [("swish", 0.01, F, F, None, True, F)] * 5,
    "rowop_xvector_leaky_near": [("leaky_relu", 0.01, F, F, None, True, F)] * 5 + [("leaky_relu", 0.01, F, F, None, True, U)],
    "rowop_snowdar_mish": [("mish", 0.01, F, F, None, True, F)] * 5 + [("mish", 0.01, F, F, None, True, U)] * 2,
    "rowop_ecapa_fc_dswish": [("double_swish", 0.01, F, F, None, True, U), ("selu", 0.01, F, F, None, True, U)],
    "rowop_lx_mish_ln": [("mish", 0.01, True, True, None, F, F)] * 3 + [("mish", 0.01, True, True, None, F, U)] * 2,
    "rowop_lx_selu_lnfirst": [(None, 0.01, True, True, "selu", F, F)] * 3 + [(None, 0.01, True, True, "selu", F, U)] * 2,
    "rowop_lx_leaky02_bnfirst": [("leaky_relu", 0.2, F, F, None, F, F)] * 3 + [("leaky_relu", 0.2, F, F, None, F, U)] * 2,
    "rowop_lx_head_ln": [(None, 0.01, True, True, None, F, F)] * 3 + [("double_swish", 0.01, True, F, None, F, U), (None, 0.01, True, True, None, F, U)],
}

def golden_model(name):
    """(fixture, numpy state_dict, the blueprint built from this repository with the fixture's synthetic weights, strictly loaded)."""
    import helpers
    g, sd = helpers.golden_state_dict(name)
    blueprint = str(g["blueprint"])
    return g, sd, helpers.build_model(LX if blueprint == os.path.basename(LX) else blueprint, str(g["creation"]), sd)



# ------------------------------------------------------------------------------------------ the device

PRECISION = {"f32": 0, "bf16": 1, "f16": 3}


def make_desc(case, f=None):
    """(capi.RowopDesc of the case, the arrays it borrows)."""
    import ctypes as C
    from libs.amd import capi
    f = fields(case) if f is None else f
    d = capi.RowopDesc()
    d.struct_size = C.sizeof(capi.RowopDesc)
    d.channels = case.channels
    d.in_buf, d.in_ch_off, d.out_buf, d.out_ch_off = 1, case.ch_off, (1 if case.inplace else 2), case.ch_off
    d.act0, d.act1 = capi.ROWOP_ACT_BY_NAME[f["act0"]], capi.ROWOP_ACT_BY_NAME[f["act1"]]
    d.slope0, d.slope1, d.ln, d.eps = f["slope0"], f["slope1"], int(f["ln"]), f["eps"]
    keep = []
    for k in ("scale0", "shift0", "gamma", "beta", "scale1", "shift1"):
        if f.get(k) is not None:
            keep.append(f[k])
            setattr(d, k, capi.f32_ptr(f[k]))
    return d, keep


def run_device(case, et):
    """asv_rowop_forward on the case -> the WHOLE output buffer [rows, width] as float32."""
    import ctypes as C
    import torch
    from libs.amd import capi
    L = capi.lib()
    x = inputs(case, et)
    d, keep = make_desc(case)
    dev = torch.device("cuda", 0)
    xd = torch.from_numpy(np.array(x)).to(dev)
    yd = torch.full_like(xd, float("nan"))
    offsets = np.concatenate([[0], np.cumsum(case.lengths)]).astype(np.int32)
    with torch.cuda.device(dev):
        rc = L.asv_rowop_forward(C.byref(d), PRECISION[et], capi.DOMAIN_FRAMES if case.domain == "frames" else capi.DOMAIN_UTTS, case.width,
                                 C.c_void_p(xd.data_ptr()), offsets.ctypes.data_as(capi.c_int32_p), len(case.lengths), C.c_void_p(yd.data_ptr()),
                                 C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    capi.check(rc, "asv_rowop_forward")
    del keep
    return yd.cpu().numpy()
