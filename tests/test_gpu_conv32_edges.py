"""The fp32 convolution entries of the C ABI -- fi_conv2d_forward_live, fi_conv2d_forward_gated, fi_conv2d_weight_grad and
fi_conv2d_weight_grad_batch -- held to float64, element by element, at the smallest shapes that reach each kernel the
planners can pick and at one neighbour on the other side of every threshold (tests/test_capi_and_host.py holds the same
shapes to the plan queries on the host).

Every case first asks fi_conv2d_forward_plan / fi_conv2d_weight_grad_plan for the same arguments and asserts the kernel key:
a shape that stops reaching its kernel fails there instead of quietly testing the generic one.  The launch then writes into
a NaN-filled output (or an accumulating entry into a non-zero one, compared by its increment) and every element is held to
the project's bar of tests/fp64_ref.py, 2^-24 (4 sqrt(n) + 16) m, n being the length of the dot product.  The references
are computed once per shape on the device and shared.

The 12-wide flat rows are shapes the detector does not run.  They found conv3x3_patch_kernel<true> staging 13 patch rows
where a 128-pixel tile that starts at column 8 of a 12-wide row needs 14: the four pixels on the last row of every third
tile lost their bottom taps (227 x 16 x 12 x 12 -> 256: element (161, 237, 9, 0), on the last row of tile 181, was -0.2196
against a reference of -2.2183, 1.03e5 times the bar; the same as the data gradient, weight_layout 2, and through
conv2d).  12-wide maps now run a 14-row instantiation of that kernel; with the fix every case here is within 7.9 units
of 2^-24 m, an eighth of the bar at n = 144 (64 units)."""
import ctypes
import functools

import pytest
import torch

import fp64_ref as R
from test_gpu_conv16_plan import _nan
from test_gpu_wgrad16_plan import _geom

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# ---- forward ------------------------------------------------------------------------------------------------------------
# name -> (N, Cin, H, W, Cout, R, stride, pad, weight_layout, expected kernel key); tile counts: pixel tiles x Cout tiles
FWD = {
    "patch": (1, 16, 128, 128, 256, 3, 1, 1, 1, "conv3x3_patch"),                    # 128 x 2 = 256 tiles of 8 x 16
    "patch_nb": (1, 16, 120, 128, 256, 3, 1, 1, 1, "conv_fwd_bm64_3x3"),             # 240
    "patch_straddle": (3, 16, 44, 128, 256, 3, 1, 1, 1, "conv3x3_patch"),            # 132 stacked rows: 17 row tiles, 44 % 8
    "patch_cout160": (1, 16, 128, 128, 160, 3, 1, 1, 1, "conv3x3_patch"),            # second Cout tile: 32 of 128 rows
    "flat14": (168, 16, 14, 14, 256, 3, 1, 1, 1, "conv3x3_patch_flat"),              # 258 x 2 flat tiles of 128 pixels
    "flat14_nb": (166, 16, 14, 14, 256, 3, 1, 1, 1, "conv_fwd_bm64_3x3"),            # 255 x 2
    "flat14_h7": (335, 16, 7, 14, 256, 3, 1, 1, 1, "conv3x3_patch_flat"),            # 98-pixel images: a tile spans two
    "flat12": (227, 16, 12, 12, 256, 3, 1, 1, 1, "conv3x3_patch_flat"),              # 256 x 2, the last tile partly filled
    "flat12_nb": (226, 16, 12, 12, 256, 3, 1, 1, 1, "conv_fwd_bm64_3x3"),            # 255 x 2
    "flat12_h10": (273, 16, 10, 12, 256, 3, 1, 1, 1, "conv3x3_patch_flat"),          # 256 x 2, H != W
    "dgrad_patch": (1, 16, 128, 128, 256, 3, 1, 1, 2, "conv3x3_patch"),              # weight_layout 2: the data gradient
    "dgrad_flat14": (168, 16, 14, 14, 256, 3, 1, 1, 2, "conv3x3_patch_flat"),
    "dgrad_flat12": (227, 16, 12, 12, 256, 3, 1, 1, 2, "conv3x3_patch_flat"),
    "reg1x1": (1, 128, 128, 128, 256, 1, 1, 0, 1, "conv1x1_reg"),                    # 256 tiles
    "reg1x1_nb_tiles": (1, 128, 124, 128, 256, 1, 1, 0, 1, "conv_fwd_bm64_1x1"),     # 248
    "reg1x1_nb_cin": (1, 96, 128, 128, 256, 1, 1, 0, 1, "conv_fwd_bm64_1x1"),        # Cin < 128
    "reg1x1_nb_hw": (1, 128, 127, 129, 256, 1, 1, 0, 1, "conv_fwd_bm64_1x1"),        # H * W % 4 != 0
    "generic_bm128": (1, 16, 512, 256, 256, 3, 2, 1, 1, "conv_fwd_bm128_3x3"),       # 512 tiles of 128 x 128
    "generic_bm64": (1, 16, 508, 256, 256, 3, 2, 1, 1, "conv_fwd_bm64_3x3"),         # 508
    "stem": (2, 3, 64, 64, 64, 7, 2, 3, 0, "conv_fwd_bm64_7x7"),                     # weight_layout 0
    # the generic kernel's launch plan: 513 x 2 = 1026 tiles of 128 x 128 are a main launch of 512 x 2 and a tail of 128
    # pixels on 64 x 64 tiles; 513 pixel tiles in the XCD-aware order are a grid padded to 520; 16 pixels are one tile
    "tail": (1, 96, 216, 304, 256, 1, 1, 0, 1, "conv_fwd_bm128_1x1"),                # K = 96 < 128: plain tile order
    "tail_swizzled": (1, 16, 432, 608, 256, 3, 2, 1, 1, "conv_fwd_bm128_3x3"),       # the main launch swizzled, nx 512
    "swizzled_pad": (1, 16, 432, 608, 128, 3, 2, 1, 1, "conv_fwd_bm128_3x3"),        # 513 x 1 tiles, no tail
    "tiny": (1, 16, 4, 4, 64, 3, 1, 1, 1, "conv_fwd_bm64_3x3"),                      # P = 16 < 64: no 64-pixel tiles
}
# name -> what fi_conv2d_forward_launches plans for the shape's first (or only) launch with NCHW output and 16-byte aligned
# operands: (form, tile rows, tile pixels, flags, grid x, grid y); _lib.FWD_FORMS / LAUNCH_FLAGS name forms and flags
FWD_LAUNCH = {
    "patch": ("PATCH", 128, 128, "tap_major vec_out", 256, 1),
    "patch_nb": ("GENERIC", 64, 64, "tap_major vec_out", 240, 4),                    # 480 workgroups < 1024: 64-pixel tiles
    "patch_straddle": ("PATCH", 128, 128, "tap_major vec_out", 272, 1),              # 136 pixel tiles x 2
    "patch_cout160": ("PATCH", 128, 128, "tap_major vec_out", 256, 1),
    "flat14": ("PATCH_FLAT13", 128, 128, "tap_major", 528, 1),                       # 258 pixel tiles padded to 264, x 2
    "flat14_nb": ("GENERIC", 64, 64, "tap_major vec_out", 509, 4),
    "flat14_h7": ("PATCH_FLAT13", 128, 128, "tap_major", 528, 1),
    "flat12": ("PATCH_FLAT14", 128, 128, "tap_major vec_out", 512, 1),
    "flat12_nb": ("GENERIC", 64, 64, "tap_major vec_out", 509, 4),
    "flat12_h10": ("PATCH_FLAT14", 128, 128, "tap_major vec_out", 512, 1),
    "dgrad_patch": ("PATCH", 128, 128, "tap_major vec_out", 256, 1),
    "dgrad_flat14": ("PATCH_FLAT13", 128, 128, "tap_major", 528, 1),
    "dgrad_flat12": ("PATCH_FLAT14", 128, 128, "tap_major vec_out", 512, 1),
    "reg1x1": ("REG1X1", 128, 128, "tap_major vec_out", 256, 1),
    "reg1x1_nb_tiles": ("GENERIC", 64, 64, "tap_major vec_out", 248, 4),
    "reg1x1_nb_cin": ("GENERIC", 64, 64, "tap_major vec_out", 256, 4),
    "reg1x1_nb_hw": ("GENERIC", 64, 64, "tap_major", 256, 4),                        # H * W % 4 != 0: scalar epilogue
    "generic_bm128": ("GENERIC", 128, 128, "tap_major vec_out", 256, 2),             # nx 256 < 512: plain tile order
    "generic_bm64": ("GENERIC", 64, 64, "tap_major vec_out", 508, 4),
    "stem": ("GENERIC", 64, 128, "vec_out", 16, 1),                                  # row-major weights: no 64-pixel form
    "tail": ("GENERIC", 128, 128, "tap_major vec_out", 512, 2),
    "tail_swizzled": ("GENERIC", 128, 128, "tap_major vec_out swizzled", 512, 2),
    "swizzled_pad": ("GENERIC", 128, 128, "tap_major vec_out swizzled", 520, 1),
    "tiny": ("GENERIC", 64, 128, "tap_major vec_out", 1, 1),
}
# ... with channels-last output (test_forward_channels_last_output)
FWD_LAUNCH_CL = {
    "patch": ("PATCH", 128, 128, "tap_major channels_last vec_out", 256, 1),
    "patch_nb": ("GENERIC", 64, 128, "tap_major channels_last", 120, 4),             # no 64-pixel channels-last form
}
# the second launch of a main / tail pair, and (p_base, pixels) of the two: every pixel belongs to exactly one
TAIL = {name: (("GENERIC", 64, 64, "tap_major vec_out", 2, 4), (0, 65536), (65536, 128)) for name in ("tail", "tail_swizzled")}
FLAT = ["flat14", "flat14_h7", "flat12", "flat12_h10"]
EPILOGUES = ["bias", "scale_bias", "residual", "gate", "relu", "all"]


def _logical(w, layout):
    """The stored weight of a forward launch as the reference's [Cout, Cin, R, S]."""
    return w if layout == 0 else w.permute(0, 3, 1, 2)


@functools.lru_cache(maxsize=None)
def _fwd_problem(name):
    """Seeded operands of a forward shape (x, w in the layout the launch reads) and the float64 reference / magnitude of
    the accumulator.  Computed once per shape, shared, never written."""
    N, Cin, H, W, Cout, k, st, pd, layout = FWD[name][:9]
    g = torch.Generator(device=DEV).manual_seed(1000 + sorted(FWD).index(name))
    x = torch.randn(N, Cin, H, W, device=DEV, generator=g)
    shape = (Cout, Cin, k, k) if layout == 0 else (Cout, k, k, Cin)
    w = torch.randn(shape, device=DEV, generator=g) / (Cin * k * k) ** 0.5
    if layout == 2:
        # the launch is the data gradient of a convolution whose weight is wf [Cin-of-the-launch, Cout-of-the-launch, R, S]
        wf = w.permute(3, 0, 1, 2)
        ref = R.dgrad_ref(x, wf, (st, st), (pd, pd), in_hw=(H, W))
        mag = R.dgrad_ref(x.abs(), wf.abs(), (st, st), (pd, pd), in_hw=(H, W))
    else:
        ref = R.conv_ref(x, _logical(w, layout), (st, st), (pd, pd))
        mag = R.conv_ref(x.abs(), _logical(w, layout).abs(), (st, st), (pd, pd))
    return x, w, ref, mag


@functools.lru_cache(maxsize=None)
def _epilogue_operands(name):
    """bias, scale [Cout], residual and gate (zeros where |g| < 0.3) of a shape's output."""
    ref = _fwd_problem(name)[2]
    g = torch.Generator(device=DEV).manual_seed(2000 + sorted(FWD).index(name))
    bias = torch.randn(ref.shape[1], device=DEV, generator=g)
    scale = torch.randn(ref.shape[1], device=DEV, generator=g)
    residual = torch.randn(ref.shape, device=DEV, generator=g)
    gate = torch.randn(ref.shape, device=DEV, generator=g)
    gate[gate.abs() < 0.3] = 0.0
    return bias, scale, residual, gate


def launch_summary(launch):
    """(form, tile rows, tile pixels, flags, grid x, grid y) of a planned forward launch, as FWD_LAUNCH states it."""
    from feature_intertwiner_amd import _lib
    return (_lib.FWD_FORMS[launch.form], launch.tile_rows, launch.tile_pixels,
            " ".join(k for k, bit in _lib.LAUNCH_FLAGS.items() if launch.flags & bit), launch.grid_x, launch.grid_y)


def expected_launches(name, output_layout=0):
    """[summary of every launch] and [(p_base, pixels)] (None for a single launch) that the tables state for a shape."""
    first = (FWD_LAUNCH_CL if output_layout else FWD_LAUNCH)[name]
    if name in TAIL and not output_layout:
        return [first, TAIL[name][0]], list(TAIL[name][1:])
    return [first], None


def _fwd_launch(name, y, bias=None, scale=None, residual=None, gate=None, relu=0, output_layout=0):
    """The planned key, form, tiles, flags and grid of the shape's launches, asserted, then the call:
    fi_conv2d_forward_live, or _gated with a gate."""
    from feature_intertwiner_amd import _lib
    L = _lib.load()
    x, w = _fwd_problem(name)[:2]
    N, Cin, H, W, Cout, k, st, pd, layout, expect = FWD[name]
    args = (_lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(scale), _lib.ptr(residual), _lib.ptr(gate), _lib.ptr(y),
            N, Cin, H, W, Cout, k, k, st, st, pd, pd, relu, layout, 0, 0, output_layout)
    key = _lib.planned_kernel(L.fi_conv2d_forward_plan, *args)
    assert key == expect, (name, key)
    planned = _lib.planned_launches(L.fi_conv2d_forward_launches, *args)
    summaries, ranges = expected_launches(name, output_layout)
    assert [launch_summary(p) for p in planned] == summaries, (name, [launch_summary(p) for p in planned])
    assert ranges is None or [(p.p_base, p.pixels) for p in planned] == ranges
    if gate is not None:
        _lib.check(L.fi_conv2d_forward_gated(*args, _lib.current_stream()), "fi_conv2d_forward_gated")
    else:
        _lib.check(L.fi_conv2d_forward_live(*args, None, _lib.current_stream()), "fi_conv2d_forward_live")
    torch.cuda.synchronize()
    return key


def _dot(name):
    N, Cin, H, W, Cout, k = FWD[name][:6]
    return Cin * k * k


@pytest.mark.parametrize("name", sorted(FWD))
def test_forward_is_the_float64_reference_at_every_kernels_boundary(name):
    x, w, ref, mag = _fwd_problem(name)
    y = _nan(*ref.shape)
    key = _fwd_launch(name, y)
    worst = R.check_bar(y, ref, mag, _dot(name), "%s (%s)" % (name, key))
    print("%s %s: %s, worst |d|/(2^-24 m) %.2f" % (name, FWD[name][:9], key, worst))
    if name in TAIL:
        assert not torch.isnan(y).any()          # the output started NaN-filled: main and tail launch wrote every pixel


@pytest.mark.parametrize("kind", EPILOGUES)
@pytest.mark.parametrize("name", FLAT + ["patch", "patch_cout160"])
def test_forward_epilogues(name, kind):
    """bias, scale + bias, residual, gate and ReLU in the kernel's epilogue, one at a time and all together: the vector
    epilogue of full 2-D tiles, the general one of a partial Cout tile, the 8-byte pairs of the flat tiles."""
    x, w, acc, acc_mag = _fwd_problem(name)
    bias, scale, residual, gate = _epilogue_operands(name)
    kw = {"bias": dict(bias=bias), "scale_bias": dict(scale=scale, bias=bias), "residual": dict(residual=residual),
          "gate": dict(gate=gate), "relu": dict(relu=1),
          "all": dict(scale=scale, bias=bias, residual=residual, gate=gate, relu=1)}[kind]
    y = _nan(*acc.shape)
    key = _fwd_launch(name, y, **kw)
    ep = dict(kw)
    relu = bool(ep.pop("relu", 0))
    ref = R.epilogue(acc, relu=relu, **ep)
    ep.pop("gate", None)
    mag = R.abs_epilogue(acc_mag, **ep)
    worst = R.check_bar(y, ref, mag, _dot(name), "%s %s (%s)" % (name, kind, key))
    if "gate" in kw:
        assert not y[gate <= 0].any()                            # exact zeros, not small numbers
    print("%s %s: %s, worst |d|/(2^-24 m) %.2f" % (name, kind, key, worst))


@pytest.mark.parametrize("name", ["patch", "patch_nb"])
def test_forward_channels_last_output(name):
    x, w, ref, mag = _fwd_problem(name)
    bias = _epilogue_operands(name)[0]
    N, Cout, OH, OW = ref.shape
    y = _nan(N, OH, OW, Cout)
    key = _fwd_launch(name, y, bias=bias, relu=1, output_layout=1)
    worst = R.check_bar(y, R.epilogue(ref, bias=bias, relu=True).permute(0, 2, 3, 1), R.abs_epilogue(mag, bias=bias).permute(0, 2, 3, 1),
                        _dot(name), "%s channels-last (%s)" % (name, key))
    print("%s channels-last: %s, worst |d|/(2^-24 m) %.2f" % (name, key, worst))


@pytest.mark.parametrize("Cin", [16, 144])
def test_conv2d_backward_on_12_wide_maps(Cin):
    """Through Python: conv2d(...).backward on 228 x Cin x 12 x 12 -> 256.  The forward runs the flat kernel for both Cin
    (257 x 2 tiles); the data gradient, whose output channels are the layer's Cin, runs it only for Cin = 144 (two Cout tiles
    of the launch; with 16 channels it is a narrow layer of the generic kernel).  y, dX and dW elementwise."""
    from feature_intertwiner_amd import _lib, conv as C
    N, H, W, Cout = 228, 12, 12, 256
    g = torch.Generator(device=DEV).manual_seed(3000 + Cin)
    x = torch.randn(N, Cin, H, W, device=DEV, generator=g).requires_grad_(True)
    w = (torch.randn(Cout, Cin, 3, 3, device=DEV, generator=g) / (Cin * 9) ** 0.5).requires_grad_(True)
    dy = torch.randn(N, Cout, H, W, device=DEV, generator=g)
    C.FLOP_LOG = {}
    try:
        y = C.conv2d(x, w, None, (1, 1), (1, 1))
        y.backward(dy)
        torch.cuda.synchronize()
    finally:
        used, C.FLOP_LOG = dict(C.FLOP_LOG), None
        C.invalidate_step_state()
    assert used.get("conv3x3_patch_flat", (0, 0))[0] == (2 if Cin == 144 else 1), used
    xd, wd = x.detach(), w.detach()
    worst_y = R.check_bar(y.detach(), R.conv_ref(xd, wd, (1, 1), (1, 1)), R.conv_ref(xd.abs(), wd.abs(), (1, 1), (1, 1)),
                          Cin * 9, "y, Cin %d" % Cin)
    worst_dx = R.check_bar(x.grad, R.dgrad_ref(dy, wd, (1, 1), (1, 1), in_hw=(H, W)),
                           R.dgrad_ref(dy.abs(), wd.abs(), (1, 1), (1, 1), in_hw=(H, W)), Cout * 9, "dX, Cin %d" % Cin)
    worst_dw = R.check_bar(w.grad, R.wgrad_ref(xd, dy, 3, 3, (1, 1), (1, 1)), R.wgrad_ref(xd.abs(), dy.abs(), 3, 3, (1, 1), (1, 1)),
                           N * H * W, "dW, Cin %d" % Cin)
    print("conv2d backward Cin %d: %s, worst |d|/(2^-24 m) y %.2f dX %.2f dW %.2f" % (
        Cin, {k: v[0] for k, v in used.items()}, worst_y, worst_dx, worst_dw))


def test_strided_data_gradient_of_a_3x3_stride_3_layer():
    """conv._strided_dgrad in fp32 on the row of tests/test_gpu_conv16_edges.py whose third residue class starts one row
    and column into dz (a negative padding, which the function used to refuse)."""
    from test_gpu_conv16_edges import check_strided_dgrad
    print("3x3_s3_7x7 fp32: worst |d|/(2^-24 m) %.2f" % check_strided_dgrad("3x3_s3_7x7", "fp32"))


# ---- weight gradient ----------------------------------------------------------------------------------------------------
# name -> (N, Cin, H, W, Cout, R, stride, pad, weight_layout, expected kernel key).  The key tells tile height and window
# class apart; the kernel form and its flags (fi_conv2d_weight_grad_launch) follow from the name, see wgrad_form_and_flags.
WGRAD = {
    # row-major vector kernel (same-size stride-1 layer, H * W % 4 == 0, Cin % 128 == 0), the smallest maps it accepts
    "vec_3x3": (1, 128, 4, 4, 128, 3, 1, 1, 1, "conv_wgrad_bm64_3x3"),
    "vec_1x1": (1, 128, 4, 4, 128, 1, 1, 0, 1, "conv_wgrad_bm64_1x1"),
    "vec_3x3_cout96": (2, 128, 6, 6, 96, 3, 1, 1, 1, "conv_wgrad_bm64_3x3"),         # the second Cout tile half empty
    "vec_1x1_cout96": (2, 128, 6, 6, 96, 1, 1, 0, 1, "conv_wgrad_bm64_1x1"),
    "vec_3x3_u16": (1, 128, 16, 16, 128, 3, 1, 1, 1, "conv_wgrad_bm64_3x3"),         # OW % 16 == 0: the row-uniform form
    "vec_1x1_u16": (1, 128, 16, 16, 128, 1, 1, 0, 1, "conv_wgrad_bm64_1x1"),
    "vec_5x5": (2, 128, 6, 6, 96, 5, 1, 2, 1, "conv_wgrad_bm64_other"),              # run-time window
    "vec_swizzled": (8, 128, 64, 64, 128, 3, 1, 1, 1, "conv_wgrad_bm64_3x3"),        # 32768 pixels: the 1-D XCD-aware grid
    # Cin == 64: two taps per 128-column tile; nine taps leave the last tile half empty
    "half_3x3": (2, 64, 6, 6, 96, 3, 1, 1, 1, "conv_wgrad_bm64_3x3"),
    "half_1x1": (2, 64, 6, 6, 96, 1, 1, 0, 1, "conv_wgrad_bm64_1x1"),
    "half_3x3_u16": (1, 64, 16, 16, 64, 3, 1, 1, 1, "conv_wgrad_bm64_3x3"),
    "half_1x1_u16": (1, 64, 16, 16, 64, 1, 1, 0, 1, "conv_wgrad_bm64_1x1"),
    "half_5x5": (2, 64, 6, 6, 96, 5, 1, 2, 1, "conv_wgrad_bm64_other"),
    # scalar kernel, tap-major dW: H * W % 4 != 0, or not a same-size layer
    "scalar_3x3": (2, 128, 5, 5, 64, 3, 1, 1, 1, "conv_wgrad_bm64_3x3"),
    "scalar_1x1": (2, 128, 5, 5, 64, 1, 1, 0, 1, "conv_wgrad_bm64_1x1"),
    "scalar_5x5": (2, 128, 5, 5, 64, 5, 1, 2, 1, "conv_wgrad_bm64_other"),
    "strided_3x3": (2, 128, 9, 9, 64, 3, 2, 1, 1, "conv_wgrad_bm64_3x3"),
    # scalar kernel, dW [Cout][Cin][R][S]
    "rowmajor_3x3": (2, 16, 5, 5, 64, 3, 1, 1, 0, "conv_wgrad_bm64_3x3"),
    "rowmajor_1x1": (2, 16, 5, 5, 64, 1, 1, 0, 0, "conv_wgrad_bm64_1x1"),
    "rowmajor_7x7": (2, 3, 16, 16, 64, 7, 2, 3, 0, "conv_wgrad_bm64_7x7"),
    "rowmajor_5x5": (2, 16, 6, 6, 64, 5, 1, 2, 0, "conv_wgrad_bm64_other"),
    # both sides of the tile-height threshold: 16 tiles of 128 rows x ceil(pixels / 512) splits >= 768
    "bm128": (6, 1024, 64, 64, 256, 1, 1, 0, 1, "conv_wgrad_bm128_1x1"),
    "bm64": (5, 1024, 64, 64, 256, 1, 1, 0, 1, "conv_wgrad_bm64_1x1"),
    # several pixel splits, the last one short: 1188 pixels in 3 splits of 400 (25 K-steps of 16) leave it 388, its last
    # K-step 4 -- on the vector kernel, its two-tap form and (1250 output pixels of a stride-2 layer, 3 x 432) the scalar one
    "vec_partial_split": (3, 128, 18, 22, 128, 3, 1, 1, 1, "conv_wgrad_bm64_3x3"),
    "half_partial_split": (3, 64, 18, 22, 128, 3, 1, 1, 1, "conv_wgrad_bm64_3x3"),
    "scalar_partial_split": (2, 128, 49, 49, 64, 3, 2, 1, 1, "conv_wgrad_bm64_3x3"),
}
# (splits, pixels per split) the library's query must answer for the partial-split rows
PARTIAL_SPLIT = {"vec_partial_split": (3, 400), "half_partial_split": (3, 400), "scalar_partial_split": (3, 432)}


def wgrad_form_and_flags(name):
    """(_lib.WGRAD_FORMS name, {swizzled, row_uniform} flags) of a single-problem launch of a WGRAD row."""
    form = {"vec": "VEC", "bm128": "VEC", "bm64": "VEC", "half": "VEC_TWO_TAP", "scalar": "SCALAR_TAP_MAJOR",
            "strided": "SCALAR_TAP_MAJOR", "rowmajor": "SCALAR_ROW_MAJOR"}[name.split("_")[0]]
    flags = set()
    if name.endswith("_u16") or name in ("vec_swizzled", "bm128", "bm64"):          # OW % 16 == 0 on a vector form
        flags.add("row_uniform")
    if name == "vec_swizzled":                                                       # 32768 pixels
        flags.add("swizzled")
    return form, flags


def _wgrad_operands(shape, seed):
    N, Cin, H, W, Cout, k, st, pd = shape
    g = torch.Generator(device=DEV).manual_seed(seed)
    OH, OW = R.out_size(H, W, k, k, (st, st), (pd, pd))
    x = torch.randn(N, Cin, H, W, device=DEV, generator=g)
    dy = torch.randn(N, Cout, OH, OW, device=DEV, generator=g)
    return x, dy, N * OH * OW


def _wgrad_refs(x, dy, k, st, pd):
    return (R.wgrad_ref(x, dy, k, k, (st, st), (pd, pd)), R.wgrad_ref(x.abs(), dy.abs(), k, k, (st, st), (pd, pd)),
            dy.double().sum((0, 2, 3)), dy.double().abs().sum((0, 2, 3)))


@functools.lru_cache(maxsize=None)
def _wgrad_problem(name):
    """x, dy, the pixel count and the float64 (dW, m of dW, dbias, m of dbias) of a weight-gradient shape, dW in the
    logical [Cout, Cin, R, S]."""
    shape = WGRAD[name][:8]
    x, dy, pixels = _wgrad_operands(shape, 4000 + sorted(WGRAD).index(name))
    return (x, dy, pixels) + _wgrad_refs(x, dy, *shape[5:8])


def _stored(dw_logical, layout):
    """A logical [Cout, Cin, R, S] tensor as the layout the entry writes."""
    return dw_logical if layout == 0 else dw_logical.permute(0, 2, 3, 1)


def _wgrad_plan(x, dy, dw, db, shape, layout, flags, n=1):
    """(kernel key, problems per launch, pixel splits, pixels per split) of the launch, from the library's queries."""
    from feature_intertwiner_amd import _lib
    a = (_lib.ptr(x), _lib.ptr(dy), _lib.ptr(dw), *_geom(shape), layout, _lib.ptr(db), flags, n)
    L = _lib.load()
    key, per = _lib.wgrad_plan(L.fi_conv2d_weight_grad_plan, *a)
    splits, pps = _lib.wgrad_plan(L.fi_conv2d_weight_grad_split_plan, *a)
    return _lib.KERNEL_KEYS[key], per, splits, pps


def _wgrad_launch(x, dy, dw, db, shape, layout, flags, n=1):
    """(form, {swizzled, row_uniform} flags) of the launch, from fi_conv2d_weight_grad_launch."""
    from feature_intertwiner_amd import _lib
    (p,) = _lib.planned_launches(_lib.load().fi_conv2d_weight_grad_launch, _lib.ptr(x), _lib.ptr(dy), _lib.ptr(dw), *_geom(shape),
                                 layout, _lib.ptr(db), flags, n)
    assert bool(p.flags & _lib.LAUNCH_FLAGS["tap_major"]) == (_lib.WGRAD_FORMS[p.form] != "SCALAR_ROW_MAJOR")
    return _lib.WGRAD_FORMS[p.form], {k for k in ("swizzled", "row_uniform") if p.flags & _lib.LAUNCH_FLAGS[k]}


@pytest.mark.parametrize("name", sorted(WGRAD))
def test_weight_gradient_is_the_float64_reference_on_every_launch_branch(name):
    """fi_conv2d_weight_grad with dbias into NaN-filled outputs (the call clears them), and under FI_OUTPUTS_ZEROED without
    dbias into a dW that already holds values: the increment is the reference."""
    from feature_intertwiner_amd import _lib
    L = _lib.load()
    N, Cin, H, W, Cout, k, st, pd, layout, expect = WGRAD[name]
    shape = WGRAD[name][:8]
    x, dy, pixels, ref, mag, db_ref, db_mag = _wgrad_problem(name)
    stored = (Cout, Cin, k, k) if layout == 0 else (Cout, k, k, Cin)

    dw, db = _nan(*stored), _nan(Cout)
    key, per, splits, pps = _wgrad_plan(x, dy, dw, db, shape, layout, 0)
    assert (key, per) == (expect, 1), (name, key, per)
    assert _wgrad_launch(x, dy, dw, db, shape, layout, 0) == wgrad_form_and_flags(name), name
    if name in PARTIAL_SPLIT:
        assert (splits, pps) == PARTIAL_SPLIT[name] and (splits - 1) * pps < pixels < splits * pps, (name, splits, pps, pixels)
    _lib.check(L.fi_conv2d_weight_grad(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(dw), *_geom(shape), layout, _lib.ptr(db), 0,
                                       _lib.current_stream()), name)
    torch.cuda.synchronize()
    worst = R.check_bar(dw, _stored(ref, layout), _stored(mag, layout), pixels, "%s dW (%s)" % (name, key))
    worst_db = R.check_bar(db, db_ref, db_mag, pixels, "%s dbias (%s)" % (name, key))

    g = torch.Generator(device=DEV).manual_seed(5000 + sorted(WGRAD).index(name))
    before = torch.randn(stored, device=DEV, generator=g) * float(pixels) ** 0.5      # the size of the increment
    dw = before.clone()
    assert _wgrad_plan(x, dy, dw, None, shape, layout, _lib.OUTPUTS_ZEROED)[0] == expect
    _lib.check(L.fi_conv2d_weight_grad(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(dw), *_geom(shape), layout, None,
                                       _lib.OUTPUTS_ZEROED, _lib.current_stream()), name)
    torch.cuda.synchronize()
    worst_inc = R.check_increment(dw, before, _stored(ref, layout), _stored(mag, layout), pixels, "%s dW increment (%s)" % (name, key))
    print("%s %s: %s, %d splits of %d pixels (of %d), worst |d|/(2^-24 m) dW %.2f dbias %.2f increment %.2f" % (
        name, WGRAD[name][:9], key, splits, pps, pixels, worst, worst_db, worst_inc))


def test_weight_gradient_batch_launch_against_float64():
    """One fi_conv2d_weight_grad_batch launch of per_launch problems with operands of their own: every problem's dW and
    dbias is the float64 reference of ITS x and dy."""
    from feature_intertwiner_amd import _lib
    L = _lib.load()
    shape, n = (2, 128, 8, 8, 128, 3, 1, 1), 5
    probs = [_wgrad_operands(shape, 6000 + i) for i in range(n)]
    dws = [torch.zeros(128, 3, 3, 128, device=DEV) for _ in range(n)]
    dbs = [torch.zeros(128, device=DEV) for _ in range(n)]
    key, per, splits, pps = _wgrad_plan(probs[0][0], probs[0][1], dws[0], dbs[0], shape, 1, _lib.OUTPUTS_ZEROED, n)
    assert (key, per) == ("conv_wgrad_bm64_3x3", n)
    assert _wgrad_launch(probs[0][0], probs[0][1], dws[0], dbs[0], shape, 1, _lib.OUTPUTS_ZEROED, n) == ("VEC", {"swizzled"})
    arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        _lib.check(L.fi_conv2d_weight_grad_batch(arr([p[0] for p in probs]), arr([p[1] for p in probs]), arr(dws), arr(dbs), n,
                                                 *_geom(shape), 1, _lib.OUTPUTS_ZEROED, _lib.current_stream()),
                   "fi_conv2d_weight_grad_batch")
        torch.cuda.synchronize()
    finally:
        _lib.prof_enable(False)
    assert _lib.prof_get(key)[0] == 1
    worst = 0.0
    for i, (x, dy, pixels) in enumerate(probs):
        ref, mag, db_ref, db_mag = _wgrad_refs(x, dy, 3, 1, 1)
        worst = max(worst, R.check_bar(dws[i], _stored(ref, 1), _stored(mag, 1), pixels, "problem %d dW" % i),
                    R.check_bar(dbs[i], db_ref, db_mag, pixels, "problem %d dbias" % i))
    print("batch of %d in one launch: %s, %d splits of %d pixels, worst |d|/(2^-24 m) %.2f" % (n, key, splits, pps, worst))
