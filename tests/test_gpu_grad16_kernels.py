"""fi_grad16_relu_grad / fi_grad16_conv_dgrad / fi_grad16_conv_wgrad (csrc/conv_grad16.hip, include/fi_grad16.h) held to
float64, element by element, through the raw C entry points, for bf16 and fp16.

Every launch writes into NaN-filled outputs with a sentinel tail of 64 elements behind them that must stay untouched.  The
references are tests/fp64_ref.py's dgrad_ref / wgrad_ref in float64 on the operands AS ROUNDED to the 16-bit type (their
products are exact in fp32) and the same on absolute values, computed once per (shape, type) and shared.  The bars are
derived, not measured, with B = 2^-24 (4 sqrt(n) + 16) m the project's fp32 bar of a sum of n terms in any order (m: the
reference on absolute values):
    dgrad   |dx - ref| <= B + u (|ref| + B) + s,  n = Cout R S; u the unit roundoff of the ONE rounding at the store
            (2^-8 bf16, 2^-11 fp16), s = 2^-25 the spacing of fp16's subnormals (0 for bf16)
    wgrad   |dw - ref| <= B,  n = N OH OW (an fp32 output: no rounding; the atomics of a split pixel range are one more
            order of the same sum)
    colsum  |colsum - ref| <= B,  n = N OH OW
Inputs: x and g standard normal rounded to the type, wt standard normal / sqrt(n); max |ref| < 6000 is asserted on the host
before the launch (fp16 overflows at 65504).

The shapes are the smallest at which each mechanism can go wrong (see SHAPES).  The known-answer cases use small integers
(every partial sum exact in fp32, every result exact in the type) and compare with torch.equal."""
import functools
import math

import pytest
import torch

import fp64_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
BITS = {"bf16": 8, "f16": 11}
UNIT = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
SUBNORMAL = {"bf16": 0.0, "f16": 2.0 ** -25}
TAIL = 64
RELU_GRAD, DGRAD, WGRAD = 0, 1, 2

# (N, H, W, Cin, Cout, k, stride)
SHAPES = [
    (1, 1, 1, 32, 32, 1, 1),         # a K tile that is almost all padding
    (2, 5, 7, 64, 96, 1, 1),         # 70 pixels; Cout no multiple of 64
    (3, 9, 15, 96, 160, 1, 1),       # tiles cross images; three channel blocks
    (2, 7, 9, 64, 128, 1, 2),        # stride 2, odd map
    (2, 8, 8, 64, 128, 1, 2),        # stride 2, even map
    (1, 1, 1, 32, 32, 3, 1),         # only the centre tap is live
    (3, 1, 16, 32, 64, 3, 1),        # only the middle tap row is live
    (2, 13, 11, 96, 160, 3, 1),
    (4, 2, 2, 128, 256, 3, 1),       # every pixel on a border
    (2, 64, 64, 32, 32, 1, 1),       # 8192 pixels = 256 K blocks of the weight gradient: the pixel range is split
    (1, 40, 40, 64, 64, 3, 1),       # 1600 pixels = 50 K blocks, nine taps: split too
]
# The data gradient takes 128-row channel tiles only where they give more than 256 workgroups, which none of the shapes
# above does: 130 x 128 pixels x 160 channels = 130 pixel tiles x 2, with a reduction block of 32 and of 64.
SHAPES_DGRAD_WIDE = [
    (1, 130, 128, 160, 32, 1, 1),
    (1, 130, 128, 160, 64, 1, 1),
]
_ids = lambda s: "x".join(map(str, s))


def _libs():
    from feature_intertwiner_amd import _lib, grad16
    return _lib, grad16.load()


def _geom(shape):
    N, H, W, Cin, Cout, k, stride = shape
    pad = (k - 1) // 2
    return pad, (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def _nan_buf(numel, dtype):
    buf = torch.full((numel + TAIL,), float("nan"), device=DEV, dtype=dtype)
    buf[numel:] = 7.0
    return buf


def _tail_ok(buf, numel):
    assert torch.equal(buf[numel:], torch.full((TAIL,), 7.0, device=DEV, dtype=buf.dtype)), "sentinel tail written"


def _logical_w(wt):
    """wt [Cin, R, S, Cout] (transposed, taps flipped) -> the weight [Cout, Cin, R, S] it is the operand of."""
    return wt.flip(1, 2).permute(3, 0, 1, 2)


@functools.lru_cache(maxsize=None)
def _operands(shape, sfx):
    """Seeded 16-bit operands on the device and the float64 references with their absolute twins."""
    N, H, W, Cin, Cout, k, stride = shape
    pad, OH, OW = _geom(shape)
    dtype = DTYPES[sfx]
    gen = torch.Generator().manual_seed(977 * sum(shape) + k)
    x = torch.randn((N, H, W, Cin), generator=gen).to(dtype).to(DEV)
    g = torch.randn((N, OH, OW, Cout), generator=gen).to(dtype).to(DEV)
    wt = (torch.randn((Cin, k, k, Cout), generator=gen) / math.sqrt(Cout * k * k)).to(dtype).to(DEV)
    add = torch.randn((N, H, W, Cin), generator=gen).to(dtype).to(DEV)
    x_l, g_l, w_l = x.permute(0, 3, 1, 2), g.permute(0, 3, 1, 2), _logical_w(wt)
    st, pd = (stride, stride), (pad, pad)
    nhwc = lambda t: t.permute(0, 2, 3, 1)
    tapm = lambda t: t.permute(0, 2, 3, 1)                           # [Cout, Cin, R, S] -> [Cout, R, S, Cin]
    return dict(x=x, g=g, wt=wt, add=add,
                dx=nhwc(R.dgrad_ref(g_l, w_l, st, pd, (H, W))), dx_abs=nhwc(R.dgrad_ref(g_l.abs(), w_l.abs(), st, pd, (H, W))),
                dw=tapm(R.wgrad_ref(x_l, g_l, k, k, st, pd)), dw_abs=tapm(R.wgrad_ref(x_l.abs(), g_l.abs(), k, k, st, pd)))


def _dgrad(shape, sfx, g, wt, add=None):
    _lib, L = _libs()
    N, H, W, Cin, Cout, k, stride = shape
    pad, OH, OW = _geom(shape)
    numel = N * H * W * Cin
    buf = _nan_buf(numel, DTYPES[sfx])
    args = (N, H, W, Cin, Cout, k, k, stride, pad)
    assert L.fi_grad16_eligible(DGRAD, *args, _lib.ptr(g), _lib.ptr(wt), _lib.ptr(add), _lib.ptr(buf)) == 1
    _lib.check(getattr(L, "fi_grad16_conv_dgrad_" + sfx)(_lib.ptr(g), _lib.ptr(wt), _lib.ptr(add), _lib.ptr(buf), *args,
                                                         _lib.current_stream()), "fi_grad16_conv_dgrad")
    torch.cuda.synchronize()
    _tail_ok(buf, numel)
    return buf[:numel].view(N, H, W, Cin)


def _wgrad(shape, sfx, g, x):
    _lib, L = _libs()
    N, H, W, Cin, Cout, k, stride = shape
    pad, OH, OW = _geom(shape)
    numel = Cout * k * k * Cin
    buf = _nan_buf(numel, torch.float32)
    args = (N, H, W, Cin, Cout, k, k, stride, pad)
    assert L.fi_grad16_eligible(WGRAD, *args, _lib.ptr(g), _lib.ptr(x), None, _lib.ptr(buf)) == 1
    _lib.check(getattr(L, "fi_grad16_conv_wgrad_" + sfx)(_lib.ptr(g), _lib.ptr(x), _lib.ptr(buf), *args,
                                                         _lib.current_stream()), "fi_grad16_conv_wgrad")
    torch.cuda.synchronize()
    _tail_ok(buf, numel)
    return buf[:numel].view(Cout, k, k, Cin)


def _relu_grad(sfx, dy, y, relu, colsum=True):
    """dy, y [N, OH, OW, C] -> (g, colsum)."""
    _lib, L = _libs()
    N, OH, OW, C = dy.shape
    numel = dy.numel()
    gbuf = _nan_buf(numel, DTYPES[sfx])
    sbuf = _nan_buf(C, torch.float32) if colsum else None
    assert L.fi_grad16_eligible(RELU_GRAD, N, OH, OW, 32, C, 1, 1, 1, 0, _lib.ptr(dy), _lib.ptr(y), _lib.ptr(gbuf),
                                _lib.ptr(sbuf)) == 1
    _lib.check(getattr(L, "fi_grad16_relu_grad_" + sfx)(_lib.ptr(dy), _lib.ptr(y), _lib.ptr(gbuf), _lib.ptr(sbuf), N, OH, OW,
                                                        C, 1 if relu else 0, _lib.current_stream()), "fi_grad16_relu_grad")
    torch.cuda.synchronize()
    _tail_ok(gbuf, numel)
    if colsum:
        _tail_ok(sbuf, C)
    return gbuf[:numel].view(N, OH, OW, C), (sbuf[:C] if colsum else None)


def _held(got, ref, allow, what):
    got = got.to(torch.float64)
    d = (got - ref).abs()
    d = torch.where(torch.isfinite(got), d, torch.full_like(d, float("inf")))          # every element, NaN = not written
    ratio = torch.where(d == 0, torch.zeros_like(d), d / allow)                       # (a zero bar admits only d == 0)
    worst = float(ratio.max())
    print("%s: worst |d| / bar = %.3f" % (what, worst))
    if not worst <= 1.0:
        k = int(torch.argmax(ratio.reshape(-1)))
        raise AssertionError("%s: element %d off the bar by %.3gx (got %r, ref %r)" % (
            what, k, worst, float(got.reshape(-1)[k]), float(ref.reshape(-1)[k])))


def _dgrad_allow(ref, mag, n, sfx):
    B = R.U * (4.0 * math.sqrt(n) + 16.0) * mag
    return B + UNIT[sfx] * (ref.abs() + B) + SUBNORMAL[sfx]


def _check_dgrad(shape, sfx, with_add):
    N, H, W, Cin, Cout, k, stride = shape
    o = _operands(shape, sfx)
    ref, mag = o["dx"], o["dx_abs"]
    if with_add:
        ref, mag = ref + o["add"].to(torch.float64), mag + o["add"].to(torch.float64).abs()
    assert float(ref.abs().max()) < 6000.0                          # fp16-safe, decided before the launch
    dx = _dgrad(shape, sfx, o["g"], o["wt"], o["add"] if with_add else None)
    _held(dx, ref, _dgrad_allow(ref, mag, Cout * k * k, sfx), "dgrad%s %s %s" % (" + dx_add" if with_add else "", sfx, shape))
    return dx


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("shape", SHAPES + SHAPES_DGRAD_WIDE, ids=_ids)
def test_dgrad_against_float64(shape, sfx):
    dx = _check_dgrad(shape, sfx, with_add=False)
    N, H, W, Cin, Cout, k, stride = shape
    if stride == 2:
        # the product lands on the even pixels; every other pixel is an exact zero written by the same launch
        assert float(dx[:, 1::2].abs().max()) == 0.0 and float(dx[:, :, 1::2].abs().max()) == 0.0
        assert torch.count_nonzero(dx[:, (H - 1) // 2 * 2, :]) > 0 and torch.count_nonzero(dx[:, :, (W - 1) // 2 * 2]) > 0
        if H % 2 == 1:
            assert torch.count_nonzero(dx[:, H - 1]) > 0 and torch.count_nonzero(dx[:, :, W - 1]) > 0     # row 6, column 8
        else:
            assert torch.count_nonzero(dx[:, H - 1]) == 0 and torch.count_nonzero(dx[:, :, W - 1]) == 0   # row 7, column 7


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3], SHAPES[4], SHAPES[7], SHAPES_DGRAD_WIDE[1]], ids=_ids)
def test_dgrad_with_dx_add_against_float64(shape, sfx):
    """dx_add on every pixel -- on the zero pixels of a stride-2 layer it comes through unchanged."""
    dx = _check_dgrad(shape, sfx, with_add=True)
    if shape[6] == 2:
        add = _operands(shape, sfx)["add"]
        assert torch.equal(dx[:, 1::2], add[:, 1::2]) and torch.equal(dx[:, :, 1::2], add[:, :, 1::2])


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_wgrad_against_float64(shape, sfx):
    N, H, W, Cin, Cout, k, stride = shape
    pad, OH, OW = _geom(shape)
    o = _operands(shape, sfx)
    assert float(o["dw"].abs().max()) < 6000.0
    dw = _wgrad(shape, sfx, o["g"], o["x"])
    allow = R.U * (4.0 * math.sqrt(N * OH * OW) + 16.0) * o["dw_abs"]
    _held(dw, o["dw"], allow, "wgrad %s %s" % (sfx, shape))
    if shape == (1, 1, 1, 32, 32, 3, 1):
        dead = torch.ones(3, 3, dtype=torch.bool)
        dead[1, 1] = False
        assert float(dw[:, dead.to(DEV)].abs().max()) == 0.0         # the eight dead taps: EXACTLY zero
        assert torch.count_nonzero(dw[:, 1, 1]) > 0
    if shape == (3, 1, 16, 32, 64, 3, 1):
        assert float(dw[:, 0].abs().max()) == 0.0 and float(dw[:, 2].abs().max()) == 0.0


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("shape", [(2, 5, 7, 32, 64, 1, 1), (2, 7, 9, 32, 64, 1, 2), (2, 5, 7, 32, 64, 3, 1)], ids=_ids)
def test_known_answers_are_exact(shape, sfx):
    """Small integers: g in -2..2, wt and x in -1..1 / -2..2: every partial sum is an integer below 2^24; the data gradient
    stays within 256 (exact in bf16, and to 2048 in fp16), the weight gradient is fp32.  Nothing is square: exchanging rows
    and columns of an operand shows."""
    N, H, W, Cin, Cout, k, stride = shape
    pad, OH, OW = _geom(shape)
    dtype = DTYPES[sfx]
    gen = torch.Generator().manual_seed(11 + k + stride)
    g = torch.randint(-2, 3, (N, OH, OW, Cout), generator=gen).to(dtype).to(DEV)
    wt = torch.randint(-1, 2, (Cin, k, k, Cout), generator=gen).to(dtype).to(DEV)
    x = torch.randint(-2, 3, (N, H, W, Cin), generator=gen).to(dtype).to(DEV)
    st, pd = (stride, stride), (pad, pad)
    dx_ref = R.dgrad_ref(g.permute(0, 3, 1, 2), _logical_w(wt), st, pd, (H, W)).permute(0, 2, 3, 1)
    dw_ref = R.wgrad_ref(x.permute(0, 3, 1, 2), g.permute(0, 3, 1, 2), k, k, st, pd).permute(0, 2, 3, 1)
    assert 8.0 <= float(dx_ref.abs().max()) <= 256.0 and torch.equal(dx_ref, dx_ref.round())
    assert 8.0 <= float(dw_ref.abs().max()) < 2.0 ** 24
    assert torch.equal(_dgrad(shape, sfx, g, wt), dx_ref.to(dtype))
    assert torch.equal(_wgrad(shape, sfx, g, x), dw_ref.to(torch.float32))


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_dgrad_rounds_the_sum_with_dx_add_once(sfx):
    """acc = 1 + e/2 with e = the rounding unit at 1 (exact in fp32, rounds to 1 in the type) and dx_add = e: acc + dx_add
    lies above the tie and rounds UP once; rounding acc first gives the tie 1 + e, which goes to the even 1."""
    p = BITS[sfx]
    dtype = DTYPES[sfx]
    shape = (1, 3, 3, 32, 32, 1, 1)
    e = 2.0 ** -p
    g = torch.zeros((1, 3, 3, 32), dtype=torch.float64)
    g[..., 0] = 1.0
    g[..., 1] = e / 2
    g[:, 1] *= -1.0                                                  # and mirrored: the middle row is negative
    wt = torch.zeros((32, 1, 1, 32), dtype=torch.float64)
    wt[..., 0] = 1.0
    wt[..., 1] = 1.0
    add = torch.full((1, 3, 3, 32), e, dtype=torch.float64)
    add[:, 1] *= -1.0
    g16, wt16, add16 = g.to(dtype).to(DEV), wt.to(dtype).to(DEV), add.to(dtype).to(DEV)
    assert torch.equal(g16.double().cpu(), g) and torch.equal(add16.double().cpu(), add)      # operands exact in the type
    acc = R.dgrad_ref(g16.permute(0, 3, 1, 2), _logical_w(wt16), (1, 1), (0, 0), (3, 3)).permute(0, 2, 3, 1)
    once = (acc + add16.double()).to(dtype)
    twice = (acc.to(dtype).double() + add16.double()).to(dtype)
    assert torch.equal(once.double().abs().cpu(), torch.full((1, 3, 3, 32), 1.0 + 2 * e, dtype=torch.float64))
    assert not torch.equal(once, twice)                              # the case separates the two
    assert torch.equal(_dgrad(shape, sfx, g16, wt16, add16), once)


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3], SHAPES[7]], ids=_ids)
def test_dgrad_bits_do_not_depend_on_placement_or_run(shape, sfx):
    """One image repeated three times in a batch (its pixels fall into different tiles at different offsets) gives three
    bit-equal gradients, and a second run repeats the first bit for bit."""
    o = _operands(shape, sfx)
    g = o["g"][:1].expand(3, -1, -1, -1).contiguous()
    add = o["add"][:1].expand(3, -1, -1, -1).contiguous()
    shape3 = (3,) + tuple(shape[1:])
    a = _dgrad(shape3, sfx, g, o["wt"], add).clone()
    b = _dgrad(shape3, sfx, g, o["wt"], add)
    bits = lambda t: t.view(torch.int16)
    assert torch.equal(bits(a), bits(b))
    assert torch.equal(bits(a[0]), bits(a[1])) and torch.equal(bits(a[0]), bits(a[2]))


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[8]], ids=_ids)
def test_wgrad_of_one_part_repeats_bit_for_bit(shape, sfx):
    """What the header promises: with ONE part of the pixel range (fewer than 16 K blocks of 32 pixels: 70 and 16 pixels
    here) dw is stored plainly and two runs agree bit for bit.  It promises nothing of the kind for a split range."""
    N, H, W, Cin, Cout, k, stride = shape
    pad, OH, OW = _geom(shape)
    assert N * OH * OW < 16 * 32
    o = _operands(shape, sfx)
    a = _wgrad(shape, sfx, o["g"], o["x"]).clone()
    b = _wgrad(shape, sfx, o["g"], o["x"])
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("rows", [(1, 1, 1, 32), (2, 5, 7, 96), (3, 9, 15, 160), (2, 64, 64, 32), (1, 3, 3, 2080)], ids=_ids)
def test_relu_grad_mask_and_column_sums(rows, sfx):
    """g is dy * (y > 0) exactly (y == 0 and y == -0.0 mask to zero), relu = 0 copies dy, colsum is within the fp32 bar of
    a sum over the rows.  2080 channels: past the 2048 a workgroup takes."""
    dtype = DTYPES[sfx]
    gen = torch.Generator().manual_seed(5 + sum(rows))
    dy = torch.randn(rows, generator=gen).to(dtype)
    y = torch.randn(rows, generator=gen).to(dtype)
    flat = y.view(-1)
    flat[0::7] = 0.0
    flat[3::11] = -0.0
    dy, y = dy.to(DEV), y.to(DEV)
    want = dy * (y > 0).to(dtype)
    assert torch.count_nonzero(want) > 0 and torch.count_nonzero(want) < want.numel()
    n = rows[0] * rows[1] * rows[2]
    for relu, ref_g in ((1, want), (0, dy)):
        g, s = _relu_grad(sfx, dy, y, relu)
        assert torch.equal(g, ref_g), relu
        ref = ref_g.to(torch.float64).sum((0, 1, 2))
        mag = ref_g.to(torch.float64).abs().sum((0, 1, 2))
        assert float(ref.abs().max()) < 6000.0
        _held(s, ref, R.U * (4.0 * math.sqrt(n) + 16.0) * mag, "colsum relu=%d %s %s" % (relu, sfx, rows))
    g, s = _relu_grad(sfx, dy, y, 1, colsum=False)                   # colsum is optional
    assert s is None and torch.equal(g, want)
    zero_y = torch.zeros_like(y)
    zero_y.view(-1)[1::2] = -0.0
    g, s = _relu_grad(sfx, dy, zero_y, 1)
    assert torch.count_nonzero(g) == 0 and torch.count_nonzero(s) == 0
