"""fi_pyr16_lateral_{bf16,f16} and fi_pyr16_head1x1_{bf16,f16} (csrc/conv_pyr16.hip: the pyramid's top-down step that reads
the coarser level at half resolution, and the RPN's stacked 1x1 heads that read a 16-bit map and write fp32 in the anchors'
order) held to float64, element by element, through the raw C entry points.

The discipline is tests/test_gpu_act16_conv.py's.  Every launch writes into a NaN-filled output with a sentinel tail of 64
elements behind it that must stay untouched.  The reference is tests/fp64_ref.py's conv_ref in float64 on the operands AS
ROUNDED to the 16-bit type, computed once per (shape, type) and shared.  The bars are that file's, derived, not measured:
    lateral  |float(y) - ref| <= B + u (|ref| + B) + s          head  |y - ref| <= B
B = 2^-24 (4 sqrt(n) + 16) m with n = Cin and m the reference on absolute values, |bias| and |top| included; u the unit
roundoff of the one rounding at the lateral's store (2^-8 bf16, 2^-11 fp16), s = 2^-25 the spacing of fp16's subnormals (0
for bf16).  The heads store fp32 unrounded, so B stands alone.  Inputs: x and top standard normal, w standard normal /
sqrt(Cin); max |ref| < 6000 is asserted before the launch.

The exact cases compare with torch.equal: zero weights and no bias (y must be top repeated 2x along H and W, bit for bit:
the half-resolution index on its own), small integers (every partial sum and result exact), three copies of an image in one
batch and two runs (bit-equal).

Measured on an MI355X, worst |d| / bar over all shapes (the tests print it per case): lateral bf16 0.995, fp16 0.987 (the
bar is essentially u |ref| and a round-to-nearest store comes within a hair of half a spacing = u |ref| somewhere among
4.5 million elements); heads bf16 0.026, fp16 0.026."""
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

# (N, H, W, Cin, Cout)
LATERAL_SHAPES = [
    (1, 2, 2, 32, 8),                # one top pixel feeds all four outputs
    (3, 6, 10, 96, 72),              # 60 pixels per image: the first pixel tile crosses two image borders; three K blocks of 32
    (2, 2, 66, 64, 40),              # a tile boundary inside a row, at an odd column
    (1, 16, 16, 256, 256),           # the pyramid's channel count
    (2, 128, 128, 64, 136),          # 512 workgroups: the 128-row tiles, with a Cout tail of 8
]
HEAD_SHAPES = [
    (1, 1, 1, 32, 1),                # smallest
    (1, 3, 3, 32, 12),
    (2, 5, 7, 64, 18),
    (3, 9, 15, 96, 18),              # tiles cross images: the flat store run starts mid-tensor
    (1, 2, 130, 512, 18),            # the RPN's Cin
    (2, 4, 4, 512, 64),              # a full channel tile
]
_ids = lambda s: "x".join(map(str, s))


def _libs():
    from feature_intertwiner_amd import _lib, pyr16
    return _lib, pyr16.load()


def _up2(t):
    """[N, h, w, C] -> [N, 2h, 2w, C], nearest neighbour."""
    return t.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


@functools.lru_cache(maxsize=None)
def _operands(shape, sfx, with_top):
    """Seeded 16-bit operands on the device and the float64 1x1 convolution / its absolute twin, both [N, H, W, Cout]."""
    N, H, W, Cin, Cout = shape
    dtype = DTYPES[sfx]
    g = torch.Generator().manual_seed(1000 * sum(shape) + (1 if with_top else 0))
    x = torch.randn((N, H, W, Cin), generator=g).to(dtype).to(DEV)
    w = (torch.randn((Cout, Cin), generator=g) / math.sqrt(Cin)).to(dtype).to(DEV)
    bias = torch.randn(Cout, generator=g).to(DEV)
    top = torch.randn((N, H // 2, W // 2, Cout), generator=g).to(dtype).to(DEV) if with_top else None
    x_nchw, w_log = x.permute(0, 3, 1, 2), w.view(Cout, Cin, 1, 1)
    acc = R.conv_ref(x_nchw, w_log, channels_last=True)
    acc_abs = R.conv_ref(x_nchw.abs(), w_log.abs(), channels_last=True)
    return dict(x=x, w=w, bias=bias, top=top, acc=acc, acc_abs=acc_abs)


def _launch_lateral(shape, sfx, x, w, bias, top):
    """One launch into a NaN-filled output with a sentinel tail; returns y [N, H, W, Cout] (the tail is checked here)."""
    _lib, L = _libs()
    N, H, W, Cin, Cout = shape
    numel = N * H * W * Cout
    buf = torch.full((numel + TAIL,), float("nan"), device=DEV, dtype=DTYPES[sfx])
    buf[numel:] = 7.0
    assert L.fi_pyr16_lateral_eligible(N, H, W, Cin, Cout, _lib.ptr(x), _lib.ptr(w), _lib.ptr(top), _lib.ptr(buf)) == 1
    fn = getattr(L, "fi_pyr16_lateral_" + sfx)
    _lib.check(fn(_lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(top), _lib.ptr(buf), N, H, W, Cin, Cout,
                  _lib.current_stream()), "fi_pyr16_lateral")
    torch.cuda.synchronize()
    assert torch.equal(buf[numel:], torch.full((TAIL,), 7.0, device=DEV, dtype=DTYPES[sfx])), "sentinel tail written"
    return buf[:numel].view(N, H, W, Cout)


def _launch_head(shape, sfx, x, w, bias, offset=0):
    """As above for the heads: fp32 output, `offset` floats behind a 16-byte boundary; the floats in front stay too."""
    _lib, L = _libs()
    N, H, W, Cin, Cout = shape
    numel = N * H * W * Cout
    buf = torch.full((offset + numel + TAIL,), float("nan"), device=DEV, dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    buf[:offset] = 7.0
    buf[offset + numel:] = 7.0
    y = buf[offset:]
    assert y.data_ptr() % 16 == (4 * offset) % 16
    assert L.fi_pyr16_head1x1_eligible(N, H, W, Cin, Cout, _lib.ptr(x), _lib.ptr(w), _lib.ptr(y)) == 1
    fn = getattr(L, "fi_pyr16_head1x1_" + sfx)
    _lib.check(fn(_lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(y), N, H, W, Cin, Cout, _lib.current_stream()),
               "fi_pyr16_head1x1")
    torch.cuda.synchronize()
    guard = torch.cat((buf[:offset], buf[offset + numel:]))
    assert torch.equal(guard, torch.full_like(guard, 7.0)), "sentinel written"
    return y[:numel].view(N, H, W, Cout)


def _worst(got, ref, allow, what):
    d = (got - ref).abs()
    d = torch.where(torch.isfinite(got), d, torch.full_like(d, float("inf")))          # every element, NaN = not written
    ratio = d / allow
    worst = float(ratio.max())
    print("%s: worst |d| / bar = %.3f" % (what, worst))
    if not worst <= 1.0:
        k = int(torch.argmax(ratio.reshape(-1)))
        raise AssertionError("%s: element %d off the bar by %.3gx (got %r, ref %r)" % (
            what, k, worst, float(got.reshape(-1)[k]), float(ref.reshape(-1)[k])))


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", LATERAL_SHAPES, ids=_ids)
def test_lateral_against_float64(shape, with_bias, sfx):
    o = _operands(shape, sfx, True)
    bias = o["bias"] if with_bias else None
    up = _up2(o["top"])
    ref = R.epilogue(o["acc"], None, bias, up, False, channel_dim=3)
    mag = R.abs_epilogue(o["acc_abs"], None, bias, up, channel_dim=3)
    assert float(ref.abs().max()) < 6000.0                          # fp16-safe, decided before the launch
    y = _launch_lateral(shape, sfx, o["x"], o["w"], bias, o["top"])
    B = R.U * (4.0 * math.sqrt(shape[3]) + 16.0) * mag
    allow = B + UNIT[sfx] * (ref.abs() + B) + SUBNORMAL[sfx]
    _worst(y.to(torch.float64), ref, allow, "lateral %s %s %s" % (sfx, shape, "bias" if with_bias else "no bias"))


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("shape", [(3, 6, 10, 96, 72), (2, 2, 66, 64, 40)], ids=_ids)
def test_lateral_with_zero_weights_is_the_top_map_repeated(shape, sfx):
    """acc = 0 and no bias: y = round16(0 + float(top)) = top, at (oh >> 1, ow >> 1), bit for bit."""
    o = _operands(shape, sfx, True)
    y = _launch_lateral(shape, sfx, o["x"], torch.zeros_like(o["w"]), None, o["top"])
    assert torch.equal(y.view(torch.int16), _up2(o["top"]).view(torch.int16))


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_lateral_known_answer_is_exact(sfx):
    """Integers in -2..2 for x, w, bias and top: |acc| <= 4 Cin = 128, every partial sum an integer, the result an integer of
    magnitude at most 132 (exact in bf16 up to 256, in fp16 up to 2048).  Nothing is square: 2 x 4 x 6 pixels, 40 channels."""
    shape = (2, 4, 6, 32, 40)
    N, H, W, Cin, Cout = shape
    dtype = DTYPES[sfx]
    g = torch.Generator().manual_seed(17)
    x = torch.randint(-2, 3, (N, H, W, Cin), generator=g).to(dtype)
    w = torch.randint(-2, 3, (Cout, Cin), generator=g).to(dtype)
    bias = torch.randint(-2, 3, (Cout,), generator=g).float()
    top = torch.randint(-2, 3, (N, H // 2, W // 2, Cout), generator=g).to(dtype)
    ref = R.conv_ref(x.permute(0, 3, 1, 2), w.view(Cout, Cin, 1, 1), channels_last=True) + bias.double() + _up2(top).double()
    assert float(ref.abs().max()) <= 132.0 and float(ref.abs().max()) >= 8.0
    assert torch.equal(ref, ref.round())
    y = _launch_lateral(shape, sfx, x.to(DEV), w.to(DEV), bias.to(DEV), top.to(DEV))
    assert torch.equal(y.cpu(), ref.to(dtype))


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("shape", [(3, 6, 10, 96, 72), (2, 2, 66, 64, 40)], ids=_ids)
def test_lateral_bits_do_not_depend_on_placement_or_run(shape, sfx):
    """One image repeated three times in a batch (its pixels fall into different tiles at different offsets) gives three
    bit-equal outputs, and a second run repeats the first bit for bit."""
    o = _operands(shape, sfx, True)
    x = o["x"][:1].expand(3, -1, -1, -1).contiguous()
    top = o["top"][:1].expand(3, -1, -1, -1).contiguous()
    shape3 = (3,) + tuple(shape[1:])
    a = _launch_lateral(shape3, sfx, x, o["w"], o["bias"], top).clone()
    b = _launch_lateral(shape3, sfx, x, o["w"], o["bias"], top)
    bits = lambda t: t.view(torch.int16)
    assert torch.equal(bits(a), bits(b))
    assert torch.equal(bits(a[0]), bits(a[1])) and torch.equal(bits(a[0]), bits(a[2]))
    assert bool(torch.isfinite(a.float()).all())


def _check_head(shape, with_bias, sfx, offset=0):
    o = _operands(shape, sfx, False)
    bias = o["bias"] if with_bias else None
    ref = R.epilogue(o["acc"], None, bias, None, False, channel_dim=3)
    mag = R.abs_epilogue(o["acc_abs"], None, bias, None, channel_dim=3)
    assert float(ref.abs().max()) < 6000.0
    y = _launch_head(shape, sfx, o["x"], o["w"], bias, offset)
    assert y.dtype is torch.float32
    B = R.U * (4.0 * math.sqrt(shape[3]) + 16.0) * mag
    _worst(y.to(torch.float64), ref, B, "head %s %s %s offset %d" % (sfx, shape, "bias" if with_bias else "no bias", offset))


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=_ids)
def test_head_against_float64(shape, with_bias, sfx):
    _check_head(shape, with_bias, sfx)


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
def test_head_writes_an_output_that_is_only_4_byte_aligned(with_bias, sfx):
    """Cout 18, y one float behind a 16-byte boundary: the flat run needs no wider alignment."""
    _check_head((3, 9, 15, 96, 18), with_bias, sfx, offset=1)


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_head_known_answer_is_exact(sfx):
    """Integers in -2..2: every partial sum and the fp32 result are exact.  300 pixels x 18 channels: three pixel tiles, the
    last part-filled, none starting at a multiple of anything in the output but 128 * 18 floats."""
    shape = (2, 10, 15, 64, 18)
    N, H, W, Cin, Cout = shape
    dtype = DTYPES[sfx]
    g = torch.Generator().manual_seed(23)
    x = torch.randint(-2, 3, (N, H, W, Cin), generator=g).to(dtype)
    w = torch.randint(-2, 3, (Cout, Cin), generator=g).to(dtype)
    bias = torch.randint(-2, 3, (Cout,), generator=g).float()
    ref = R.conv_ref(x.permute(0, 3, 1, 2), w.view(Cout, Cin, 1, 1), channels_last=True) + bias.double()
    assert float(ref.abs().max()) <= 258.0 and float(ref.abs().max()) >= 8.0
    y = _launch_head(shape, sfx, x.to(DEV), w.to(DEV), bias.to(DEV))
    assert torch.equal(y.cpu(), ref.float())


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_head_bits_do_not_depend_on_placement_or_run(sfx):
    shape = (3, 9, 15, 96, 18)
    o = _operands(shape, sfx, False)
    x = o["x"][:1].expand(3, -1, -1, -1).contiguous()
    a = _launch_head(shape, sfx, x, o["w"], o["bias"]).clone()
    b = _launch_head(shape, sfx, x, o["w"], o["bias"])
    bits = lambda t: t.view(torch.int32)
    assert torch.equal(bits(a), bits(b))
    assert torch.equal(bits(a[0]), bits(a[1])) and torch.equal(bits(a[0]), bits(a[2]))
    assert bool(torch.isfinite(a).all())
