"""fi_act16_conv_forward_{bf16,f16} (csrc/conv_act16.hip: the implicit-GEMM convolution that reads and writes 16-bit
channels-last tensors) held to float64, element by element, through the raw C entry point.

Every launch writes into a NaN-filled output with a sentinel tail of 64 elements behind it that must stay untouched.  The
reference is tests/fp64_ref.py's conv_ref / epilogue / abs_epilogue in float64 on the operands AS ROUNDED to the 16-bit type
(their products are exact in fp32), computed once per (shape, type) and shared.  The bar is derived, not measured:
    |float(y) - ref| <= B + u (|ref| + B) + s
B = 2^-24 (4 sqrt(n) + 16) m is the project's fp32 bar for the accumulation and the fp32 epilogue (n = Cin R S, m the
reference on absolute values), u the unit roundoff of the one rounding at the store (2^-8 bf16, 2^-11 fp16), s = 2^-25 the
spacing of fp16's subnormals (0 for bf16, which has fp32's exponent range).  A truncating store fails it; a wrong tap or
halo fails it by orders of magnitude.  Inputs: x standard normal, w standard normal / sqrt(n); max |ref| < 6000 is
asserted on the CPU side before the launch (fp16 overflows at 65504).

The known-answer cases use small integers (every partial sum exact in fp32, every result exact in the 16-bit type) and
compare with torch.equal; the determinism cases compare bits between three copies of an image in one batch (whose tiles
sit at different places of the grid) and between two runs."""
import functools
import math

import pytest
import torch

import fp64_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
UNIT = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
SUBNORMAL = {"bf16": 0.0, "f16": 2.0 ** -25}
TAIL = 64

# (N, H, W, Cin, Cout, k, stride)
SHAPES_1X1 = [
    (1, 1, 1, 32, 8, 1, 1),          # one pixel, the smallest eligible channels
    (2, 5, 7, 64, 96, 1, 1),         # a part-filled pixel tile, Cout no multiple of 64
    (3, 9, 15, 96, 264, 1, 1),       # 405 pixels with tiles crossing images, three 32-channel K blocks, Cout = 2 * 128 + 8
    (1, 2, 130, 32, 40, 1, 1),       # wide and short
    (2, 7, 9, 64, 128, 1, 2),        # stride 2 on an odd map -> 4 x 5
    (2, 8, 8, 256, 512, 1, 2),       # a stage entry
]
SHAPES_3X3 = [
    (1, 1, 1, 32, 8, 3, 1),          # only the centre tap is live
    (2, 3, 5, 64, 40, 3, 1),
    (3, 1, 16, 32, 64, 3, 1),        # only the middle tap row
    (2, 13, 11, 96, 136, 3, 1),      # odd both ways, three K blocks, Cout tail 8
    (2, 20, 28, 32, 64, 3, 1),       # 1120 pixels, whole tiles plus a remainder
    (4, 2, 2, 128, 256, 3, 1),       # every pixel on a border, tiles span images
    (1, 16, 16, 256, 256, 3, 1),     # the trunk's channel count
]
# The launcher takes 64-row channel tiles for Cout <= 64 and wherever 128-row tiles would give at most 256 workgroups, which
# is every shape above: these reach the 128-row tiles (K blocks of 64 and of 32) and sit on both sides of the switch.
SHAPES_WIDE_GRID = [
    (2, 128, 128, 64, 136, 1, 1),    # 256 pixel tiles x 2 = 512 workgroups: 128-row tiles, K block 64, Cout tail 8
    (1, 176, 128, 32, 264, 3, 1),    # 176 x 3 = 528: 128-row tiles, K block 32, 3x3, Cout = 2 * 128 + 8
    (1, 256, 128, 32, 72, 1, 1),     # 256 x 1 = 256: the last grid on 64-row tiles (two of them, the second holds 8)
    (1, 257, 128, 32, 72, 1, 1),     # 257 x 1: the first on 128-row tiles
]
EPI_SHAPES = [SHAPES_1X1[2], SHAPES_3X3[3]]
EPILOGUES = {
    "none": dict(),
    "bias": dict(bias=True),
    "scale_bias": dict(scale=True, bias=True),
    "residual": dict(residual=True),
    "relu": dict(relu=True),
    "all": dict(scale=True, bias=True, residual=True, relu=True),
}


def _lib16():
    from feature_intertwiner_amd import _lib, act16
    return _lib, act16.load()


def _out_hw(H, W, k, stride):
    pad = (k - 1) // 2
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


@functools.lru_cache(maxsize=None)
def _operands(shape, sfx):
    """Seeded 16-bit operands on the device, and the float64 convolution / its absolute twin, both [N, OH, OW, Cout]."""
    N, H, W, Cin, Cout, k, stride = shape
    dtype = DTYPES[sfx]
    n = Cin * k * k
    g = torch.Generator().manual_seed(1000 * sum(shape) + k)
    x = torch.randn((N, H, W, Cin), generator=g).to(dtype)
    w = (torch.randn((Cout, k, k, Cin), generator=g) / math.sqrt(n)).to(dtype)
    OH, OW = _out_hw(H, W, k, stride)
    scale = 0.5 + torch.rand(Cout, generator=g)
    bias = torch.randn(Cout, generator=g)
    res = torch.randn((N, OH, OW, Cout), generator=g).to(dtype)
    xd, wd = x.to(DEV), w.to(DEV)
    x_nchw, w_log = xd.permute(0, 3, 1, 2), wd.permute(0, 3, 1, 2)
    pad = (k - 1) // 2
    acc = R.conv_ref(x_nchw, w_log, (stride, stride), (pad, pad), channels_last=True)
    acc_abs = R.conv_ref(x_nchw.abs(), w_log.abs(), (stride, stride), (pad, pad), channels_last=True)
    return dict(x=xd, w=wd, scale=scale.to(DEV), bias=bias.to(DEV), res=res.to(DEV), acc=acc, acc_abs=acc_abs, n=n,
                out=(N, OH, OW, Cout))


def _launch(shape, sfx, x, w, scale=None, bias=None, residual=None, relu=False):
    """One launch into a NaN-filled output with a sentinel tail; returns y [N, OH, OW, Cout] (the tail is checked here)."""
    _lib, L = _lib16()
    N, H, W, Cin, Cout, k, stride = shape
    OH, OW = _out_hw(H, W, k, stride)
    numel = N * OH * OW * Cout
    buf = torch.full((numel + TAIL,), float("nan"), device=DEV, dtype=DTYPES[sfx])
    buf[numel:] = 7.0
    pad = (k - 1) // 2
    assert L.fi_act16_conv_eligible(N, H, W, Cin, Cout, k, k, stride, pad, _lib.ptr(x), _lib.ptr(w), _lib.ptr(residual),
                                    _lib.ptr(buf)) == 1
    fn = getattr(L, "fi_act16_conv_forward_" + sfx)
    _lib.check(fn(_lib.ptr(x), _lib.ptr(w), _lib.ptr(scale), _lib.ptr(bias), _lib.ptr(residual), _lib.ptr(buf), N, H, W, Cin,
                  Cout, k, k, stride, pad, 1 if relu else 0, _lib.current_stream()), "fi_act16_conv_forward")
    torch.cuda.synchronize()
    assert torch.equal(buf[numel:], torch.full((TAIL,), 7.0, device=DEV, dtype=DTYPES[sfx])), "sentinel tail written"
    return buf[:numel].view(N, OH, OW, Cout)


def _check(shape, sfx, scale=False, bias=False, residual=False, relu=False, what=""):
    o = _operands(shape, sfx)
    sc = o["scale"] if scale else None
    bi = o["bias"] if bias else None
    rs = o["res"] if residual else None
    ref = R.epilogue(o["acc"], sc, bi, rs, relu, channel_dim=3)
    mag = R.abs_epilogue(o["acc_abs"], sc, bi, rs, channel_dim=3)
    assert float(ref.abs().max()) < 6000.0                          # fp16-safe, decided before the launch
    y = _launch(shape, sfx, o["x"], o["w"], sc, bi, rs, relu)
    assert tuple(y.shape) == o["out"]
    got = y.to(torch.float64)
    B = R.U * (4.0 * math.sqrt(o["n"]) + 16.0) * mag
    allow = B + UNIT[sfx] * (ref.abs() + B) + SUBNORMAL[sfx]
    d = (got - ref).abs()
    d = torch.where(torch.isfinite(got), d, torch.full_like(d, float("inf")))          # every element, NaN = not written
    ratio = d / allow
    worst = float(ratio.max())
    print("%s %s %s: worst |d| / bar = %.3f" % (what, sfx, shape, worst))
    if not worst <= 1.0:
        k = int(torch.argmax(ratio.reshape(-1)))
        raise AssertionError("%s %s %s: element %d off the bar by %.3gx (got %r, ref %r)" % (
            what, sfx, shape, k, worst, float(got.reshape(-1)[k]), float(ref.reshape(-1)[k])))


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("shape", SHAPES_1X1, ids=lambda s: "x".join(map(str, s)))
def test_1x1_against_float64(shape, sfx):
    _check(shape, sfx, what="1x1")


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("shape", SHAPES_3X3, ids=lambda s: "x".join(map(str, s)))
def test_3x3_against_float64(shape, sfx):
    _check(shape, sfx, what="3x3")


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("shape", SHAPES_WIDE_GRID, ids=lambda s: "x".join(map(str, s)))
def test_wide_grids_against_float64(shape, sfx):
    """With every epilogue operand: the 128-row tiles' staged store and shortcut read."""
    _check(shape, sfx, what="wide grid", **EPILOGUES["all"])


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("epi", sorted(EPILOGUES))
@pytest.mark.parametrize("shape", EPI_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_epilogues_against_float64(shape, epi, sfx):
    _check(shape, sfx, what="epilogue " + epi, **EPILOGUES[epi])


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("shape", [(2, 5, 7, 32, 40, 1, 1), (2, 5, 7, 32, 40, 3, 1)], ids=["1x1", "3x3"])
def test_known_answers_are_exact(shape, sfx):
    """Small integers: x in -2..2, w in -1..1, so every partial sum is an integer below 2^24 and every result an integer of
    magnitude at most 256 (exact in bf16, and to 2048 in fp16).  The operands are asymmetric (Cout = 40 channels, 70
    pixels, nothing square): exchanging rows and columns of either shows."""
    N, H, W, Cin, Cout, k, stride = shape
    dtype = DTYPES[sfx]
    g = torch.Generator().manual_seed(7 + k)
    x = torch.randint(-2, 3, (N, H, W, Cin), generator=g).to(dtype)
    w = torch.randint(-1, 2, (Cout, k, k, Cin), generator=g).to(dtype)
    pad = (k - 1) // 2
    ref = R.conv_ref(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), (stride, stride), (pad, pad), channels_last=True)
    assert float(ref.abs().max()) <= 256.0 and float(ref.abs().max()) >= 8.0
    assert torch.equal(ref, ref.round())
    y = _launch(shape, sfx, x.to(DEV), w.to(DEV))
    assert torch.equal(y.cpu(), ref.to(dtype))


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("shape", EPI_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bits_do_not_depend_on_placement_or_run(shape, sfx):
    """One image repeated three times in a batch (its pixels fall into different tiles at different offsets) gives three
    bit-equal outputs, and a second run repeats the first bit for bit."""
    o = _operands(shape, sfx)
    x = o["x"][:1].expand(3, -1, -1, -1).contiguous()
    res = o["res"][:1].expand(3, -1, -1, -1).contiguous()
    shape3 = (3,) + tuple(shape[1:])
    a = _launch(shape3, sfx, x, o["w"], o["scale"], o["bias"], res, True).clone()
    b = _launch(shape3, sfx, x, o["w"], o["scale"], o["bias"], res, True)
    bits = lambda t: t.view(torch.int16)
    assert torch.equal(bits(a), bits(b))
    assert torch.equal(bits(a[0]), bits(a[1])) and torch.equal(bits(a[0]), bits(a[2]))
    assert bool(torch.isfinite(a.float()).all())
