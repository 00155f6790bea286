"""The planned 16-bit forward entry fi_conv2d_forward_live_{bf16,f16}: what fi_conv2d_forward_plan_* names is what the launch
runs.  The shapes are the smallest that reach each fast kernel through the planner (tests/test_capi_and_host.py holds the
query to them on the host) and one generic neighbour of each.

  * plan and launch agree on the OPERAND: with weight = w and weight16 = the 16-bit copy of 2 w, the output is the float64
    reference (tests/fp64_ref.py, operands rounded to the type) of 2 w exactly where the query names a variant that reads
    the copy, and of w everywhere else -- elementwise, within the project's bar, on a NaN-filled output;
  * the planned launch and the "run this kernel" entry of the same kernel give the same bits;
  * conv._conv_fwd passes this step's copy where it has one and converts a temporary only where the planner reads it;
  * an x that is not 16-byte aligned takes the generic kernel instead of raising.

The 12-wide flat row is the one shape here the detector does not run.  It found the flat kernel staging 13 patch rows
where a 128-pixel tile that starts at column 8 of a 12-wide row needs 14 (227 x 32 x 12 x 12 -> 256, bf16: element
(156, 31, 5, 0) = 0.4335 against a reference of -2.8276, 5.2e4 times the bar); 12-wide maps now run a 14-row
instantiation of that kernel."""
import functools

import pytest
import torch

import fp64_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
PRECISION = {"bf16": "bf16", "f16": "fp16"}

# name -> (N, Cin, H, W, Cout, R, pad, explicit output size, expected variant with a copy)
SHAPES = {
    "patch_w16": (1, 32, 96, 128, 256, 3, 1, False, "PATCH_W16"),              # 192 tiles
    "patch_w16_nb": (1, 32, 88, 128, 256, 3, 1, False, "GENERIC_BM64"),        # 176
    "patch": (1, 32, 96, 128, 256, 3, 1, True, "PATCH"),                       # explicit out_h / out_w: fp32 weights
    "flat14": (167, 32, 14, 14, 256, 3, 1, False, "PATCH_FLAT_W16"),           # 512 flat tiles
    "flat14_nb": (166, 32, 14, 14, 256, 3, 1, False, "GENERIC_BM128"),         # 510
    "flat12": (227, 32, 12, 12, 256, 3, 1, False, "PATCH_FLAT_W16"),           # 512
    "flat12_nb": (226, 32, 12, 12, 256, 3, 1, False, "GENERIC_BM64"),          # 510
    "reg1x1": (1, 64, 96, 128, 256, 1, 0, False, "REG1X1_W16"),                # 192
    "reg1x1_nb": (1, 64, 95, 128, 256, 1, 0, False, "GENERIC_BM64"),           # 190
}
W16_ROWS = [k for k, v in SHAPES.items() if v[-1].endswith("_W16")]


@functools.lru_cache(maxsize=None)
def _problem(name, sfx):
    """Seeded operands of a shape (x, tap-major w) and the float64 reference / magnitude of conv(x, w) on operands rounded
    to the type.  Computed once per (shape, type), shared, never written."""
    N, Cin, H, W, Cout, Rr, pad = SHAPES[name][:7]
    g = torch.Generator(device=DEV).manual_seed(sorted(SHAPES).index(name))
    x = torch.randn(N, Cin, H, W, device=DEV, generator=g)
    w = torch.randn(Cout, Rr, Rr, Cin, device=DEV, generator=g) / (Cin * Rr * Rr) ** 0.5
    dt = DTYPES[sfx]
    xr, wl = x.to(dt).float(), w.to(dt).float().permute(0, 3, 1, 2)
    ref = R.conv_ref(xr, wl, (1, 1), (pad, pad))
    mag = R.conv_ref(xr.abs(), wl.abs(), (1, 1), (pad, pad))
    return x, w, ref, mag


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _planned_launch(name, sfx, x, w, w16, y, bias=None, residual=None, gate=None, relu=0):
    """fi_conv2d_forward_live_<sfx> on the shape `name`; returns the variant its query names for the same arguments."""
    from feature_intertwiner_amd import _lib
    L = _lib.load()
    N, Cin, H, W, Cout, Rr, pad, explicit = SHAPES[name][:8]
    oh, ow = (H, W) if explicit else (0, 0)
    args = (_lib.ptr(x), _lib.ptr(w), _lib.ptr(w16), _lib.ptr(bias), None, _lib.ptr(residual), _lib.ptr(gate), _lib.ptr(y),
            N, Cin, H, W, Cout, Rr, Rr, 1, 1, pad, pad, relu, 1, oh, ow, 0)
    variant = _lib.conv16_variant(getattr(L, "fi_conv2d_forward_plan_" + sfx), *args)
    _lib.check(getattr(L, "fi_conv2d_forward_live_" + sfx)(*args, None, _lib.current_stream()), "fi_conv2d_forward_live_" + sfx)
    torch.cuda.synchronize()
    return _lib.CONV16_VARIANTS[variant]


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_launch_reads_the_operand_the_plan_names(name, sfx):
    x, w, ref, mag = _problem(name, sfx)
    Cin, Rr = SHAPES[name][1], SHAPES[name][5]
    w16 = (2.0 * w).to(DTYPES[sfx])              # (a power of two: the reference of 2 w is twice the reference of w)
    y = _nan(*ref.shape)
    variant = _planned_launch(name, sfx, x, w, w16, y)
    assert variant == SHAPES[name][-1]
    f = 2.0 if variant.endswith("_W16") else 1.0
    worst = R.check_bar(y, f * ref, f * mag, Cin * Rr * Rr, "%s %s with a copy (%s)" % (name, sfx, variant))
    y = _nan(*ref.shape)
    plain = _planned_launch(name, sfx, x, w, None, y)
    assert not plain.endswith("_W16")
    worst = max(worst, R.check_bar(y, ref, mag, Cin * Rr * Rr, "%s %s without a copy (%s)" % (name, sfx, plain)))
    print("%s %s: %s / %s, worst |d|/(2^-24 m) %.2f" % (name, sfx, variant, plain, worst))


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("name", W16_ROWS)
def test_planned_launch_and_kernel_entry_give_the_same_bits(name, sfx):
    from feature_intertwiner_amd import _lib
    L = _lib.load()
    x, w, ref, _ = _problem(name, sfx)
    N, Cin, H, W, Cout, Rr = SHAPES[name][:6]
    w16 = w.to(DTYPES[sfx])
    g = torch.Generator(device=DEV).manual_seed(7)
    bias = torch.randn(Cout, device=DEV, generator=g)
    residual = torch.randn(ref.shape, device=DEV, generator=g)
    gate = torch.randn(ref.shape, device=DEV, generator=g)
    gate[gate.abs() < 0.3] = 0.0
    for kw in (dict(bias=bias), dict(residual=residual), dict(gate=gate), dict(relu=1)):
        y_plan, y_entry = _nan(*ref.shape), _nan(*ref.shape)
        assert _planned_launch(name, sfx, x, w, w16, y_plan, **kw) == SHAPES[name][-1]
        epi = (_lib.ptr(kw.get("bias")), None, _lib.ptr(kw.get("residual")), _lib.ptr(kw.get("gate")), _lib.ptr(y_entry))
        if Rr == 3:
            rc = getattr(L, "fi_conv3x3_forward_gated_%sw" % sfx)(_lib.ptr(x), _lib.ptr(w16), *epi, N, Cin, H, W, Cout,
                                                                  kw.get("relu", 0), 0, _lib.current_stream())
        else:
            rc = getattr(L, "fi_conv1x1_forward_gated_%sw" % sfx)(_lib.ptr(x), _lib.ptr(w16), *epi, N, Cin, H * W, Cout,
                                                                  kw.get("relu", 0), _lib.current_stream())
        _lib.check(rc, "kernel entry")
        torch.cuda.synchronize()
        assert torch.equal(y_plan, y_entry), (name, sfx, sorted(kw))


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_conv_fwd_converts_a_temporary_only_where_the_plan_reads_the_copy(sfx):
    from feature_intertwiner_amd import conv as C
    x, w, ref, mag = _problem("reg1x1", sfx)
    Cout, Cin = w.shape[0], w.shape[3]
    w = w.view(Cout, Cin, 1, 1)
    C.invalidate_step_state()
    try:
        C._cached_bf16(w, DTYPES[sfx])                       # as _prepare_step leaves a model weight: in the cache
        assert len(C._COPIES.having("lowp")) == 1
        y_cached = C._conv_fwd(x, w, None, (1, 1), (0, 0), precision=PRECISION[sfx])
        assert len(C._COPIES.having("lowp")) == 1
        fresh = w.clone()
        y_fresh = C._conv_fwd(x, fresh, None, (1, 1), (0, 0), precision=PRECISION[sfx])
        torch.cuda.synchronize()
        assert len(C._COPIES.having("lowp")) == 2 and fresh.data_ptr() in C._COPIES.table
        assert torch.equal(y_cached, y_fresh)
        R.check_bar(y_fresh, ref, mag, Cin, "reg1x1 through _conv_fwd")
        xn, wn, refn, magn = _problem("reg1x1_nb", sfx)
        yn = C._conv_fwd(xn, wn.view(Cout, Cin, 1, 1).clone(), None, (1, 1), (0, 0), precision=PRECISION[sfx])
        torch.cuda.synchronize()
        assert len(C._COPIES.having("lowp")) == 2                # the generic kernel reads the fp32 weights: nothing converted
        R.check_bar(yn, refn, magn, Cin, "reg1x1_nb through _conv_fwd")
    finally:
        C.invalidate_step_state()


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_conv_fwd_with_a_misaligned_x_takes_the_generic_kernel(sfx):
    from feature_intertwiner_amd import _lib, conv as C
    x, w, ref, mag = _problem("patch_w16", sfx)
    buf = torch.empty(x.numel() + 1, device=DEV)
    xm = buf[1:].view(x.shape)
    xm.copy_(x)
    assert xm.data_ptr() % 16 == 4 and xm.is_contiguous()
    N, Cin, H, W, Cout = SHAPES["patch_w16"][:5]
    y = _nan(*ref.shape)
    a = (_lib.ptr(xm), _lib.ptr(w), 16, None, None, None, None, _lib.ptr(y), N, Cin, H, W, Cout, 3, 3, 1, 1, 1, 1, 0, 1, 0, 0, 0)
    assert _lib.CONV16_VARIANTS[_lib.conv16_variant(getattr(_lib.load(), "fi_conv2d_forward_plan_" + sfx), *a)] == "GENERIC_BM64"
    C.invalidate_step_state()
    try:
        got = C._conv_fwd(xm, w, None, (1, 1), (1, 1), w_tap_major=True, precision=PRECISION[sfx])
        torch.cuda.synchronize()
        assert len(C._COPIES.having("lowp")) == 0
    finally:
        C.invalidate_step_state()
    R.check_bar(got, ref, mag, Cin * 9, "3x3 with x at a 4-byte offset")
