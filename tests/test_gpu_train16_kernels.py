"""fi_train16_conv_dgrad_gated (csrc/conv_train16.hip, include/fi_train16.h) through the raw C entry points, bf16 and fp16:
bit-equal to fi_grad16_relu_grad(fi_grad16_conv_dgrad(g, wt, dx_add), gate) run on the same buffers, within the data
gradient's float64 bar after the select on the gate, and its column sums within the fp32 bar of a sum of its OWN dx.

Every launch writes into NaN-filled outputs with a sentinel tail of 64 elements behind them that must stay untouched
(dx and colsum alike).  The float64 reference is tests/fp64_ref.py's dgrad_ref on the operands AS ROUNDED to the 16-bit
type, and the same on absolute values, computed once per (shape, type) and shared.  Bars, derived and not measured, with
B(n, m) = 2^-24 (4 sqrt(n) + 16) m the project's fp32 bar of a sum of n terms of magnitude sum m in any order:
    dx      |dx - ref| <= B(Cout R S, |ref|_abs) + u (|ref| + B) + s where the gate is > 0 (u: the unit roundoff of the ONE
            rounding, 2^-8 bf16 / 2^-11 fp16; s = 2^-25 the spacing of fp16's subnormals, 0 for bf16); EXACTLY zero elsewhere.
            The select is on the gate, never on the computed value: no element is left out.
    colsum  |colsum - sum64(dx)| <= B(N H W, sum |dx|): the kernel's own stored dx, summed in float64.

Shapes: those of tests/test_gpu_grad16_kernels.py, restated (each names its mechanism), and one with three channel tiles
and eight pixel tiles, so that several workgroups add into each sum."""
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
TINY = {"bf16": 2.0 ** -133, "f16": 2.0 ** -24}          # the smallest subnormal of the type
TAIL = 64
RELU_GRAD, DGRAD = 0, 1

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
    (2, 64, 64, 32, 32, 1, 1),       # 8192 pixels: 64 pixel tiles add into each of 32 sums
    (1, 40, 40, 64, 64, 3, 1),       # 1600 pixels, nine taps
    (3, 17, 19, 288, 64, 1, 1),      # three channel tiles x eight pixel tiles: several workgroups per sum
]
# 128-row channel tiles are taken only where they give more than 256 workgroups: 130 x 128 pixels x 160 channels = 130 pixel
# tiles x 2, with a reduction block of 32 and of 64
SHAPES_DGRAD_WIDE = [
    (1, 130, 128, 160, 32, 1, 1),
    (1, 130, 128, 160, 64, 1, 1),
]
GATES = ["random", "positive", "zero", "special"]
_ids = lambda s: "x".join(map(str, s))


def _libs():
    from feature_intertwiner_amd import _lib, grad16, train16
    return _lib, grad16.load(), train16.load()


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
    """Seeded 16-bit operands on the device and the float64 reference of the UNGATED gradient with its absolute twin."""
    N, H, W, Cin, Cout, k, stride = shape
    pad, OH, OW = _geom(shape)
    dtype = DTYPES[sfx]
    gen = torch.Generator().manual_seed(977 * sum(shape) + k)
    g = torch.randn((N, OH, OW, Cout), generator=gen).to(dtype).to(DEV)
    wt = (torch.randn((Cin, k, k, Cout), generator=gen) / math.sqrt(Cout * k * k)).to(dtype).to(DEV)
    add = torch.randn((N, H, W, Cin), generator=gen).to(dtype).to(DEV)
    y = torch.randn((N, H, W, Cin), generator=gen)
    g_l, w_l = g.permute(0, 3, 1, 2), _logical_w(wt)
    st, pd = (stride, stride), (pad, pad)
    nhwc = lambda t: t.permute(0, 2, 3, 1)
    return dict(g=g, wt=wt, add=add, y=y,
                dx=nhwc(R.dgrad_ref(g_l, w_l, st, pd, (H, W))), dx_abs=nhwc(R.dgrad_ref(g_l.abs(), w_l.abs(), st, pd, (H, W))))


@functools.lru_cache(maxsize=None)
def _gate(shape, sfx, kind):
    """[N, H, W, Cin] of the type.  'random': post-ReLU-like, about half zeros; 'special': that with -0.0, +0.0, NaN, the
    smallest subnormal and a negative value at known positions (every fifth element in turn)."""
    dtype = DTYPES[sfx]
    y = _operands(shape, sfx)["y"]
    if kind == "positive":
        gate = y.abs() + 0.5
    elif kind == "zero":
        gate = torch.zeros_like(y)
    else:
        gate = torch.relu(y)
    gate = gate.to(dtype)
    if kind == "special":
        flat = gate.view(-1)
        flat[0::5] = -0.0
        flat[1::5] = 0.0
        flat[2::5] = float("nan")
        flat[3::5] = TINY[sfx]
        flat[4::5] = -1.5
        assert float(flat[3]) == TINY[sfx] and float(flat[3]) > 0.0      # representable: it is > 0 and opens the gate
    return gate.to(DEV)


def _open(gate):
    """Where the select lets the value through: gate > 0 (false for +-0, a negative value and NaN)."""
    return gate.to(torch.float64) > 0


def _args(shape):
    N, H, W, Cin, Cout, k, stride = shape
    pad, OH, OW = _geom(shape)
    return (N, H, W, Cin, Cout, k, k, stride, pad)


def _gated(shape, sfx, g, wt, gate, add=None, colsum=True):
    """One launch of the entry point under test -> (dx [N, H, W, Cin], colsum [Cin] or None)."""
    _lib, _, L = _libs()
    N, H, W, Cin = shape[:4]
    numel = N * H * W * Cin
    buf = _nan_buf(numel, DTYPES[sfx])
    sbuf = _nan_buf(Cin, torch.float32) if colsum else None
    args = _args(shape)
    assert L.fi_train16_eligible(*args, _lib.ptr(g), _lib.ptr(gate), _lib.ptr(add), _lib.ptr(buf)) == 1
    _lib.check(getattr(L, "fi_train16_conv_dgrad_gated_" + sfx)(_lib.ptr(g), _lib.ptr(wt), _lib.ptr(add), _lib.ptr(gate),
                                                                _lib.ptr(buf), _lib.ptr(sbuf), *args,
                                                                _lib.current_stream()), "fi_train16_conv_dgrad_gated")
    torch.cuda.synchronize()
    _tail_ok(buf, numel)
    if colsum:
        _tail_ok(sbuf, Cin)
    return buf[:numel].view(N, H, W, Cin), (sbuf[:Cin] if colsum else None)


def _two_launches(shape, sfx, g, wt, gate, add=None):
    """The pair the gated launch replaces, through the EXISTING entry points: (relu_grad(dgrad(..), gate), its colsum)."""
    _lib, L, _ = _libs()
    N, H, W, Cin = shape[:4]
    numel = N * H * W * Cin
    args = _args(shape)
    dx = _nan_buf(numel, DTYPES[sfx])
    assert L.fi_grad16_eligible(DGRAD, *args, _lib.ptr(g), _lib.ptr(wt), _lib.ptr(add), _lib.ptr(dx)) == 1
    _lib.check(getattr(L, "fi_grad16_conv_dgrad_" + sfx)(_lib.ptr(g), _lib.ptr(wt), _lib.ptr(add), _lib.ptr(dx), *args,
                                                         _lib.current_stream()), "fi_grad16_conv_dgrad")
    out = _nan_buf(numel, DTYPES[sfx])
    s = _nan_buf(Cin, torch.float32)
    _lib.check(getattr(L, "fi_grad16_relu_grad_" + sfx)(_lib.ptr(dx), _lib.ptr(gate), _lib.ptr(out), _lib.ptr(s), N, H, W,
                                                        Cin, 1, _lib.current_stream()), "fi_grad16_relu_grad")
    torch.cuda.synchronize()
    return out[:numel].view(N, H, W, Cin), s[:Cin]


def _bits(t):
    return t.view(torch.int16)


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


def _check(shape, sfx, kind, with_add):
    N, H, W, Cin, Cout, k, stride = shape
    o = _operands(shape, sfx)
    gate = _gate(shape, sfx, kind)
    add = o["add"] if with_add else None
    ref, mag = o["dx"], o["dx_abs"]
    if with_add:
        ref, mag = ref + add.to(torch.float64), mag + add.to(torch.float64).abs()
    assert float(ref.abs().max()) < 6000.0                          # fp16-safe, decided before the launch
    what = "gated%s %s %s %s" % (" + dx_add" if with_add else "", kind, sfx, shape)
    dx, s = _gated(shape, sfx, o["g"], o["wt"], gate, add)
    # 1. the two launches it replaces, on the same buffers: bit for bit
    want, want_s = _two_launches(shape, sfx, o["g"], o["wt"], gate, add)
    assert torch.equal(_bits(dx), _bits(want)), what
    # 2. float64 after the select on the gate: every element
    opened = _open(gate)
    B = R.U * (4.0 * math.sqrt(Cout * k * k) + 16.0) * mag
    allow = torch.where(opened, B + UNIT[sfx] * (ref.abs() + B) + SUBNORMAL[sfx], torch.zeros_like(B))
    _held(dx, torch.where(opened, ref, torch.zeros_like(ref)), allow, what)
    # 3. the sums of the values as stored
    d64 = dx.to(torch.float64)
    own, own_abs = d64.sum((0, 1, 2)), d64.abs().sum((0, 1, 2))
    bar = R.U * (4.0 * math.sqrt(N * H * W) + 16.0) * own_abs
    _held(s, own, bar, what + " colsum")
    _held(want_s, own, bar, what + " colsum of relu_grad")           # the same sum in another order
    if kind == "zero":
        assert torch.count_nonzero(dx) == 0 and torch.count_nonzero(s) == 0
    if kind == "positive":
        assert torch.count_nonzero(dx) > 0.9 * dx.numel()
    # 4. colsum is optional and dx does not depend on it; a second run repeats dx bit for bit
    again, none = _gated(shape, sfx, o["g"], o["wt"], gate, add, colsum=False)
    assert none is None and torch.equal(_bits(again), _bits(dx)), what
    return dx


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "dx_add"])
@pytest.mark.parametrize("shape", SHAPES + SHAPES_DGRAD_WIDE, ids=_ids)
def test_gated_dgrad_equals_the_two_launches_and_holds_to_float64(shape, with_add, sfx):
    dx = _check(shape, sfx, "random", with_add)
    N, H, W, Cin, Cout, k, stride = shape
    if stride == 2 and not with_add:
        # the product lands on the even pixels; every other pixel of a cell is an exact zero written by the same launch
        assert float(dx[:, 1::2].abs().max()) == 0.0 and float(dx[:, :, 1::2].abs().max()) == 0.0
        assert torch.count_nonzero(dx[:, (H - 1) // 2 * 2, :]) > 0 and torch.count_nonzero(dx[:, :, (W - 1) // 2 * 2]) > 0
    if stride == 2 and with_add:
        # on the odd pixels dx_add comes through, gated: all (up to four) pixels of a cell are gated and summed
        add, gate = _operands(shape, sfx)["add"], _gate(shape, sfx, "random")
        want = torch.where(gate > 0, add, torch.zeros_like(add))
        assert torch.equal(dx[:, 1::2], want[:, 1::2]) and torch.equal(dx[:, :, 1::2], want[:, :, 1::2])
        assert torch.count_nonzero(dx[:, 1::2]) > 0


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("kind", ["positive", "zero", "special"])
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3], SHAPES[7], SHAPES[11]], ids=_ids)
def test_gate_contents(shape, kind, sfx):
    """All positive, all zero, and the special values: -0.0, +0.0, NaN and a negative value select zero, the smallest
    subnormal (> 0) lets the value through."""
    dx = _check(shape, sfx, kind, with_add=True)
    if kind == "special":
        flat = dx.reshape(-1)
        for k in (0, 1, 2, 4):
            assert torch.count_nonzero(flat[k::5]) == 0, k
        assert torch.count_nonzero(flat[3::5]) > 0.9 * flat[3::5].numel()


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("shape", [(2, 5, 7, 32, 64, 1, 1), (2, 7, 9, 32, 64, 1, 2), (2, 5, 7, 32, 64, 3, 1)], ids=_ids)
def test_known_answers_are_exact(shape, sfx):
    """Small integers: g in -2..2, wt in -1..1, dx_add in -2..2: every partial sum is an integer below 2^24, the gradient
    stays within 256 (exact in bf16, and to 2048 in fp16), and a column sums at most 126 such values: below 2^24 too, so
    every fp32 sum is exact in ANY order and colsum is compared with torch.equal."""
    N, H, W, Cin, Cout, k, stride = shape
    pad, OH, OW = _geom(shape)
    dtype = DTYPES[sfx]
    gen = torch.Generator().manual_seed(11 + k + stride)
    g = torch.randint(-2, 3, (N, OH, OW, Cout), generator=gen).to(dtype).to(DEV)
    wt = torch.randint(-1, 2, (Cin, k, k, Cout), generator=gen).to(dtype).to(DEV)
    add = torch.randint(-2, 3, (N, H, W, Cin), generator=gen).to(dtype).to(DEV)
    gate = torch.randint(-1, 3, (N, H, W, Cin), generator=gen).to(dtype).to(DEV)        # -1, 0 closed; 1, 2 open
    ref = R.dgrad_ref(g.permute(0, 3, 1, 2), _logical_w(wt), (stride, stride), (pad, pad), (H, W)).permute(0, 2, 3, 1)
    ref = ref + add.to(torch.float64)
    ref = torch.where(gate.to(torch.float64) > 0, ref, torch.zeros_like(ref))
    assert 8.0 <= float(ref.abs().max()) <= 256.0 and torch.equal(ref, ref.round())
    assert N * H * W * 256 < 2 ** 24
    dx, s = _gated(shape, sfx, g, wt, gate, add)
    assert torch.equal(dx, ref.to(dtype))
    assert torch.equal(s, ref.sum((0, 1, 2)).to(torch.float32))
    assert torch.count_nonzero(s) > 0


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_python_wrapper_returns_what_the_entry_point_writes(sfx):
    """train16.dgrad_gated16 on logical-NCHW channels-last tensors: the same bits, the counter, and no grad16 launch."""
    from feature_intertwiner_amd import grad16, train16
    shape = SHAPES[3]
    N, H, W, Cin, Cout, k, stride = shape
    o = _operands(shape, sfx)
    gate = _gate(shape, sfx, "random")
    want, _ = _gated(shape, sfx, o["g"], o["wt"], gate, o["add"])
    nchw = lambda t: t.permute(0, 3, 1, 2)
    train16.reset_stats()
    grad16.reset_stats()
    dx, s = train16.dgrad_gated16(nchw(o["g"]), o["wt"], nchw(gate), (H, W), stride=stride, pad=0, dx_add=nchw(o["add"]))
    assert dx.is_contiguous(memory_format=torch.channels_last) and tuple(dx.shape) == (N, Cin, H, W)
    assert torch.equal(_bits(dx.permute(0, 2, 3, 1).contiguous()), _bits(want.contiguous()))
    assert s.dtype == torch.float32 and tuple(s.shape) == (Cin,)
    dx2, none = train16.dgrad_gated16(nchw(o["g"]), o["wt"], nchw(gate), (H, W), stride=stride, colsum=False)
    assert none is None
    assert train16.stats()["gated"] == 2 and grad16.stats() == {"relu_grad": 0, "dgrad": 0, "wgrad": 0, "weights": 0}
