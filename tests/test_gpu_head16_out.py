"""fi_head16_out1x1_{bf16,f16} (include/fi_head16.h, csrc/head16_out.hip): the heads' 1x1 output layer -- 16-bit rows in, fp32
out, any number of output channels, optional sigmoid, optional 2 x 2 pixel shuffle -- through the raw C entry points.

The discipline is tests/test_gpu_pyr16_kernels.py's.  Every launch writes into a NaN-filled fp32 output that starts ONE float
behind a 16-byte boundary (4-byte alignment is all the kernel may assume), with a sentinel in front and a sentinel tail of 64
floats behind it that must stay untouched.  Operands: x standard normal, w standard normal / sqrt(Cin), both rounded to the
type, bias standard normal fp32; computed once per (shape, type) and shared.

Shapes (P, Cin, Cout): ten combinations that cover P in {1, 127, 128, 129, 600} (below, at and past a pixel tile; five
tiles), Cin in {32, 96, 256, 1024} (K blocks of 32 and of 64) and Cout in {1, 63, 64, 65, 81, 405} (below, at and past a
channel tile; seven tiles with a tail of 21).

Rows, no activation, against float64: |y - ref| <= B = 2^-24 (4 sqrt(Cin) + 16) m, the derived bar of
tests/test_gpu_pyr16_kernels.py; ref is fp64_ref.conv_ref on the rounded operands plus the bias, m the same on absolute
values, |bias| included.
Rows, no activation, against fi_pyr16_head1x1: bit-equal, column block by column block, to that entry point run on the weight
rows [64 j, 64 j + 64) -- the same loop, the same acc + bias.
Shuffle: (n, H, W) in {(1, 1, 1), (3, 3, 5), (2, 14, 14)} with P = 4 n H W; the [n, Cout, 2H, 2W] result is bit-equal to the rows
result permuted (tiles cross images and output rows: 4W = 20 and 56 do not divide 128).
Sigmoid: the yardstick is what the path does today, torch.sigmoid in fp32 on the kernel's own pre-activations (its act = 0
output); both are measured against float64 sigmoid of those pre-activations, and the kernel's largest absolute error may be at
most 2 x torch's + 2^-24 (two evaluations of one function to a few units in the last place by formulas that may differ; 2^-24
is one spacing below 1).  With pre-activations of +-100 the outputs are finite and within [0, 1].
Small integers (every sum exact): the known answer with torch.equal, rows and shuffle.

Measured on an MI355X (the tests print every line): rows against float64, worst |d| / bar over all shapes 0.034 (bf16) and
0.037 (fp16), both at 129 x 32 x 405; the sigmoid's numbers stand under test_sigmoid_is_as_close_as_torchs."""
import functools
import math

import pytest
import torch

import fp64_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
TAIL, OFFSET = 64, 1
ROWS, SHUFFLE = 0, 1

# (P, Cin, Cout)
SHAPES = [
    (1, 32, 1),
    (127, 96, 63),
    (128, 256, 64),
    (129, 1024, 65),
    (600, 256, 81),
    (600, 1024, 405),
    (129, 32, 405),
    (127, 256, 1),
    (128, 96, 81),
    (1, 1024, 64),
]
# (n, H, W, Cin, Cout): P = 4 n H W
SHUFFLES = [
    (1, 1, 1, 32, 1),
    (3, 3, 5, 96, 65),
    (2, 14, 14, 256, 81),
]
_ids = lambda s: "x".join(map(str, s))


def _libs():
    from feature_intertwiner_amd import _lib, head16
    return _lib, head16.load()


@functools.lru_cache(maxsize=None)
def _operands(P, Cin, Cout, sfx):
    """Seeded 16-bit operands on the device, the float64 product [P, Cout] and its absolute twin."""
    dtype = DTYPES[sfx]
    g = torch.Generator().manual_seed(1000 * (P + Cin + Cout) + 7)
    x = torch.randn((P, Cin), generator=g).to(dtype).to(DEV)
    w = (torch.randn((Cout, Cin), generator=g) / math.sqrt(Cin)).to(dtype).to(DEV)
    bias = torch.randn(Cout, generator=g).to(DEV)
    x_nchw, w_log = x.view(1, 1, P, Cin).permute(0, 3, 1, 2), w.view(Cout, Cin, 1, 1)
    acc = R.conv_ref(x_nchw, w_log, channels_last=True).view(P, Cout)
    acc_abs = R.conv_ref(x_nchw.abs(), w_log.abs(), channels_last=True).view(P, Cout)
    return dict(x=x, w=w, bias=bias, acc=acc, acc_abs=acc_abs)


def _launch(sfx, x, w, bias, P, Cin, Cout, act=0, layout=ROWS, nhw=(0, 0, 0)):
    """One launch into a NaN-filled output one float behind a 16-byte boundary, sentinels around it; returns the P * Cout
    floats flat (the sentinels are checked here)."""
    _lib, L = _libs()
    numel = P * Cout
    buf = torch.full((OFFSET + numel + TAIL,), float("nan"), device=DEV, dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    buf[:OFFSET] = 7.0
    buf[OFFSET + numel:] = 7.0
    y = buf[OFFSET:]
    assert y.data_ptr() % 16 == 4
    n, H, W = nhw
    assert L.fi_head16_out1x1_eligible(P, Cin, Cout, act, layout, n, H, W, _lib.ptr(x), _lib.ptr(w), _lib.ptr(y)) == 1
    fn = getattr(L, "fi_head16_out1x1_" + sfx)
    _lib.check(fn(_lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(y), P, Cin, Cout, act, layout, n, H, W,
                  _lib.current_stream()), "fi_head16_out1x1")
    torch.cuda.synchronize()
    guard = torch.cat((buf[:OFFSET], buf[OFFSET + numel:]))
    assert torch.equal(guard, torch.full_like(guard, 7.0)), "sentinel written"
    out = y[:numel]
    assert not bool(torch.isnan(out).any()), "an element was not written"
    return out


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_rows_against_float64(shape, with_bias, sfx):
    P, Cin, Cout = shape
    o = _operands(P, Cin, Cout, sfx)
    bias = o["bias"] if with_bias else None
    ref = R.epilogue(o["acc"], None, bias, None, channel_dim=1)
    mag = R.abs_epilogue(o["acc_abs"], None, bias, None, channel_dim=1)
    y = _launch(sfx, o["x"], o["w"], bias, P, Cin, Cout).view(P, Cout)
    B = R.U * (4.0 * math.sqrt(Cin) + 16.0) * mag
    ratio = (y.to(torch.float64) - ref).abs() / B
    worst = float(ratio.max())
    print("rows %s %s %s: worst |d| / bar = %.3f" % (sfx, shape, "bias" if with_bias else "no bias", worst))
    assert worst <= 1.0, (shape, sfx, worst)


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_rows_are_bit_equal_to_the_rpn_head_kernel_block_by_block(shape, sfx):
    from feature_intertwiner_amd import pyr16
    _lib, _ = _libs()
    P, Cin, Cout = shape
    o = _operands(P, Cin, Cout, sfx)
    y = _launch(sfx, o["x"], o["w"], o["bias"], P, Cin, Cout).view(P, Cout)
    fn = getattr(pyr16.load(), "fi_pyr16_head1x1_" + sfx)
    for j in range(0, Cout, 64):
        rows = min(64, Cout - j)
        wj, bj = o["w"][j:j + rows].contiguous(), o["bias"][j:j + rows].contiguous()
        yj = torch.full((P, rows), float("nan"), device=DEV, dtype=torch.float32)
        _lib.check(fn(_lib.ptr(o["x"]), _lib.ptr(wj), _lib.ptr(bj), _lib.ptr(yj), 1, 1, P, Cin, rows, _lib.current_stream()),
                   "fi_pyr16_head1x1")
        torch.cuda.synchronize()
        assert _bits_equal(y[:, j:j + rows], yj), (shape, sfx, j)


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("act", [0, 1], ids=["linear", "sigmoid"])
@pytest.mark.parametrize("shape", SHUFFLES, ids=_ids)
def test_shuffle_is_the_rows_result_permuted(shape, act, sfx):
    n, H, W, Cin, Cout = shape
    P = 4 * n * H * W
    o = _operands(P, Cin, Cout, sfx)
    rows = _launch(sfx, o["x"], o["w"], o["bias"], P, Cin, Cout, act=act)
    shuf = _launch(sfx, o["x"], o["w"], o["bias"], P, Cin, Cout, act=act, layout=SHUFFLE, nhw=(n, H, W))
    # row p = ((i H + h) W + w) 4 + 2a + b  ->  y[i, co, 2h + a, 2w + b]
    want = rows.view(n, H, W, 2, 2, Cout).permute(0, 5, 1, 3, 2, 4).reshape(n, Cout, 2 * H, 2 * W)
    assert _bits_equal(shuf.view(n, Cout, 2 * H, 2 * W), want), (shape, sfx)
    assert float(want.abs().max()) > 0.1


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_sigmoid_is_as_close_as_torchs(sfx):
    """Measured on an MI355X, largest absolute error against float64 sigmoid of the kernel's own pre-activations (x scaled
    by 3: pre-activations within about +-15), e_torch / e_kernel, bound 2 e_torch + 2^-24:
        bf16  600 x 1024 x 405  8.897e-8 / 8.897e-8 (2.376e-7)   600 x 256 x 81  8.771e-8 / 8.771e-8   129 x 32 x 405  8.782e-8 / 8.782e-8
        fp16  600 x 1024 x 405  8.843e-8 / 8.843e-8 (2.365e-7)   600 x 256 x 81  8.768e-8 / 8.768e-8   129 x 32 x 405  8.787e-8 / 8.787e-8
    The two agree to every printed digit: the kernel's 1 / (1 + expf(-v)) with an IEEE division is torch's formula."""
    for P, Cin, Cout in ((600, 1024, 405), (600, 256, 81), (129, 32, 405)):
        o = _operands(P, Cin, Cout, sfx)
        x = (o["x"].float() * 3.0).to(DTYPES[sfx])              # pre-activations of a few units: both tails of the curve
        pre = _launch(sfx, x, o["w"], o["bias"], P, Cin, Cout, act=0)
        got = _launch(sfx, x, o["w"], o["bias"], P, Cin, Cout, act=1)
        exact = torch.sigmoid(pre.to(torch.float64))
        e_torch = float((torch.sigmoid(pre).to(torch.float64) - exact).abs().max())
        e_kernel = float((got.to(torch.float64) - exact).abs().max())
        print("sigmoid %s %s: pre in [%.1f, %.1f]  e_torch %.3e  e_kernel %.3e  bound %.3e"
              % (sfx, (P, Cin, Cout), float(pre.min()), float(pre.max()), e_torch, e_kernel, 2 * e_torch + 2.0 ** -24))
        assert float(pre.max()) > 4.0 and float(pre.min()) < -4.0
        assert e_kernel <= 2.0 * e_torch + 2.0 ** -24, (sfx, e_kernel, e_torch)
        assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_sigmoid_saturates_inside_the_unit_interval(sfx):
    """Pre-activations of exactly +-100 (x = +-1 in one channel, w = 100, exact in both types): finite, within [0, 1]."""
    P, Cin, Cout = 130, 32, 65
    dtype = DTYPES[sfx]
    x = torch.zeros((P, Cin), dtype=dtype)
    x[:, 0] = torch.where(torch.arange(P) % 2 == 0, 1.0, -1.0).to(dtype)
    w = torch.zeros((Cout, Cin), dtype=dtype)
    w[:, 0] = 100.0
    pre = _launch(sfx, x.to(DEV), w.to(DEV), None, P, Cin, Cout, act=0).view(P, Cout)
    assert torch.equal(pre[0::2], torch.full_like(pre[0::2], 100.0)) and torch.equal(pre[1::2], torch.full_like(pre[1::2], -100.0))
    y = _launch(sfx, x.to(DEV), w.to(DEV), None, P, Cin, Cout, act=1).view(P, Cout)
    assert bool(torch.isfinite(y).all()) and float(y.min()) >= 0.0 and float(y.max()) <= 1.0
    assert float(y[0::2].min()) == 1.0 and float(y[1::2].max()) <= 2.0 ** -126      # 1 / (1 + e^100) = 3.7e-44: subnormal or 0


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("shape", [(3, 3, 5, 96, 65), (2, 2, 17, 64, 130)], ids=_ids)
def test_small_integers_give_the_known_answer(shape, sfx):
    n, H, W, Cin, Cout = shape
    P = 4 * n * H * W
    dtype = DTYPES[sfx]
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randint(-2, 3, (P, Cin), generator=g).to(dtype)
    w = torch.randint(-2, 3, (Cout, Cin), generator=g).to(dtype)
    bias = torch.randint(-2, 3, (Cout,), generator=g).float()
    ref = (x.double() @ w.double().t() + bias.double())
    assert float(ref.abs().max()) <= 4.0 * Cin + 2 and float(ref.abs().max()) >= 8.0 and torch.equal(ref, ref.round())
    rows = _launch(sfx, x.to(DEV), w.to(DEV), bias.to(DEV), P, Cin, Cout).view(P, Cout)
    assert torch.equal(rows.cpu(), ref.float())
    shuf = _launch(sfx, x.to(DEV), w.to(DEV), bias.to(DEV), P, Cin, Cout, layout=SHUFFLE, nhw=(n, H, W))
    want = ref.float().view(n, H, W, 2, 2, Cout).permute(0, 5, 1, 3, 2, 4).reshape(n, Cout, 2 * H, 2 * W)
    assert torch.equal(shuf.view(n, Cout, 2 * H, 2 * W).cpu(), want)


def test_python_wrapper_shapes_counts_and_refusals():
    from feature_intertwiner_amd import _lib, head16
    o = _operands(4 * 3 * 3 * 5, 96, 65, "bf16")
    x = o["x"].view(3, 3, 5, 4 * 96).permute(0, 3, 1, 2)                 # [n, (a, b, c), H, W] channels-last
    head16.reset_stats()
    with torch.no_grad():
        rows = head16.out1x1_16(o["x"].view(180, 1, 1, 96).permute(0, 3, 1, 2), o["w"], o["bias"])
        assert tuple(rows.shape) == (180, 65) and rows.dtype is torch.float32
        shuf = head16.out1x1_16(x, o["w"], o["bias"], act=head16.NONE, layout=head16.SHUFFLE)
        assert tuple(shuf.shape) == (3, 65, 6, 10) and shuf.is_contiguous()
        assert _bits_equal(shuf, rows.view(3, 3, 5, 2, 2, 65).permute(0, 5, 1, 3, 2, 4).reshape(3, 65, 6, 10))
        w32 = o["w"].float().view(65, 96, 1, 1)                           # an fp32 1x1 weight: its 16-bit copy is cached
        again = head16.out1x1_16(x, w32, o["bias"], layout=head16.SHUFFLE)
        assert _bits_equal(again, shuf)
        assert head16.stats() == {"crop": 0, "conv": 0, "out": 3, "weights": 0}
        with pytest.raises(_lib.FiError, match="weight"):
            head16.out1x1_16(x, o["w"][:, :64].contiguous(), None, layout=head16.SHUFFLE)
        with pytest.raises(_lib.FiError, match="fi_head16_out1x1_eligible"):
            head16.out1x1_16(x, o["w"], o["bias"], act=2, layout=head16.SHUFFLE)
    assert head16.stats()["out"] == 3
