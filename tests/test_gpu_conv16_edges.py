"""The 16-bit forward / data-gradient entry fi_conv2d_forward_live_{bf16,f16} held to float64, element by element, at the
edge shapes of every kernel behind plan_forward16 (csrc/conv_bf16.hip): the generic kernel's scalar gather, clamp-and-shift
loader and two-load stride-2 gather on narrow and odd maps, the 2-D patch tiles on stacked short images and ragged widths,
the flat tiles on H != W, the register 1x1 kernel on 2 x 2 and 14 x 14 maps, tap-reversed weights on all of them, the
epilogue operands, channels-last output, a device live count that ends inside a tile, and the sub-kernels
conv._strided_dgrad launches.  The fp32 twin of this file is tests/test_gpu_conv32_edges.py.

Every case first asks fi_conv2d_forward_plan_<sfx> with the real pointers and asserts the variant of CASES (the host test
test_16bit_forward_plan_holds_the_edge_shape_table of tests/test_capi_and_host.py holds the same table without a GPU): a
shape that stops reaching its kernel fails there instead of quietly testing the generic one.  The launch writes into a
NaN-filled output and every element is held to the project's bar of tests/fp64_ref.py, 2^-24 (4 sqrt(n) + 16) m, n being the
length of the dot product.  Reference and m are computed in float64 on operands rounded to the 16-bit type (their products
are exact in fp32, so only the order of the summation remains), once per (shape, type), and shared.

Measured on an MI355X, worst |d| / (2^-24 m) over both types, every case passing: patch 2.45 (patch_h1, f16), flat 2.62
(flat14_cout160, bf16), reg1x1 2.27 (reg1x1_roi_cout160, f16), generic 2.42 (bm128_s2, bf16; channels-last and live-count
launches included), epilogues 2.51 (flat12_h10 scale + bias, f16), strided dgrad 1.28 (3x3_s3_7x7, bf16).  The bar is 38.6
units at n = 32 (the 1x1 rows on 32 channels), 83.9 at n = 288 (3x3 on 32 channels): nothing is above a fifteenth of it.
Where a shape runs a fast kernel with a copy and the generic one without, the two results have the same worst ratio: all
forward kernels add the taps in the same order on the same MFMA.

No kernel was wrong.  One case found a host bug: conv._strided_dgrad refused 3x3 / stride 3 / pad 1 ("unsupported
stride/padding combination").  Input rows ih = 3q + 2 are read by tap 0 of output row q + 1 only, so the class's stride-1
correlation starts one row (column) INTO dz -- a padding of -1, which the function asserted against.  It now crops dz by
the negative padding and launches with padding 0; 3x3_s3_7x7 holds the result to the reference."""
import functools

import pytest
import torch

import fp64_ref as R
from test_gpu_conv16_plan import DTYPES, PRECISION, _nan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

B64, B128 = "GENERIC_BM64", "GENERIC_BM128"


def _c(N, Cin, H, W, Cout, k, stride=(1, 1), pad=None, layout=1, out_hw=None, copy=B64, plain=None):
    """A row of CASES; k: the window (an int or (R, S)), pad defaults to the same-size padding of a stride-1 layer."""
    r, s = (k, k) if isinstance(k, int) else k
    ph, pw = ((r - 1) // 2, (s - 1) // 2) if pad is None else pad
    return (N, Cin, H, W, Cout, r, s, stride[0], stride[1], ph, pw, layout, out_hw, copy, copy if plain is None else plain)


def _patch(N, Cin, H, W, Cout, layout=1):
    return _c(N, Cin, H, W, Cout, 3, layout=layout, copy="PATCH_W16", plain="PATCH")


def _flat(N, H, W, Cout=256, layout=1):
    return _c(N, 32, H, W, Cout, 3, layout=layout, copy="PATCH_FLAT_W16", plain=B128)


# name -> (N, Cin, H, W, Cout, R, S, stride_h, stride_w, pad_h, pad_w, weight_layout, out_hw, variant with a 16-bit copy of
# the weight, variant without).  Tiles: pixel tiles x Cout tiles of 128 output channels.
CASES = {
    # 2-D patch tiles of 8 stacked rows x 16 columns, from 192 workgroups
    "patch_w20": _patch(3, 32, 128, 20, 256),                    # 48 x 2 x 2 = 192; the second column tile holds 4 of 16
    "patch_h3": _patch(256, 32, 3, 16, 256),                     # 96 x 1 x 2 = 192; every tile stacks 2 2/3 images
    "patch_h1": _patch(768, 32, 1, 16, 256),                     # 96 x 1 x 2 = 192; only the middle tap row is ever live
    "patch_straddle_cout160": _patch(9, 32, 44, 32, 160),        # 50 x 2 x 2 = 200; last row tile half filled, Cout tile 32 / 128
    "patch_cin96": _patch(1, 96, 96, 128, 256),                  # 12 x 8 x 2 = 192; three channel blocks
    "patch_w20_dgrad": _patch(3, 32, 128, 20, 256, layout=2),    # tap-reversed weights
    "patch_h3_dgrad": _patch(256, 32, 3, 16, 256, layout=2),
    # flat tiles of 128 consecutive pixels, from 512 workgroups (a copy only); without one the generic kernel's 128 rows
    "flat14_h7": _flat(334, 7, 14),                              # 256 x 2 = 512
    "flat14_h2": _flat(1166, 2, 14),                             # 256 x 2; a tile spans five images
    "flat14_h1": _flat(2332, 1, 14),                             # 256 x 2; a tile spans ten images
    "flat12_h10": _flat(273, 10, 12),                            # 256 x 2; the 14-row instantiation
    "flat12_h1": _flat(2721, 1, 12),                             # 256 x 2
    "flat14_cout160": _flat(167, 14, 14, Cout=160),              # 256 x 2; the second Cout tile holds 32 of 128
    "flat14_h7_dgrad": _flat(334, 7, 14, layout=2),
    "flat12_h10_dgrad": _flat(273, 10, 12, layout=2),
    "flat14_h7_nb": _c(333, 32, 7, 14, 256, 3, copy=B128),       # 255 x 2 = 510 flat tiles; 292 x 2 generic ones
    # 1x1 with the weights in registers, from 192 workgroups (a copy only)
    "reg1x1_hw4": _c(3041, 64, 2, 2, 256, 1, copy="REG1X1_W16", plain=B64),              # 96 x 2; the last tile holds one quad
    "reg1x1_roi_cout160": _c(63, 192, 14, 14, 160, 1, copy="REG1X1_W16", plain=B64),     # 97 x 2; three stages; quads cross images
    "reg1x1_cin128": _c(1, 128, 96, 128, 256, 1, copy="REG1X1_W16", plain=B64),          # 96 x 2; two stages
    "reg1x1_cin128_dgrad": _c(1, 128, 96, 128, 256, 1, layout=2, copy="REG1X1_W16", plain=B64),
    # generic kernel, narrow maps: W < 4 the scalar gather, W = 4 the boundary of the 16-byte gather (every halo a register
    # shift), W = 5..7 a part-filled second quad whose load is clamped to column W - 4
    "narrow_w2": _c(8, 32, 2, 2, 64, 3),
    "narrow_w3": _c(8, 32, 3, 3, 64, 3),
    "narrow_w4": _c(8, 32, 4, 4, 64, 3),                         # 128 virtual pixels: one whole pixel tile
    "narrow_w5": _c(8, 32, 5, 5, 64, 3),
    "narrow_w6": _c(8, 32, 6, 6, 64, 3),
    "narrow_w7": _c(8, 32, 7, 7, 64, 3),
    "win5x5_w4": _c(8, 32, 4, 4, 64, 5),
    "win1x1_w2": _c(8, 32, 2, 2, 64, 1),
    "win1x1_w5": _c(8, 32, 5, 5, 64, 1),
    "win7x7_one_pixel": _c(192, 128, 7, 7, 256, 7, pad=(0, 0)),  # one output pixel per image; R S = 49; 6 x 2 tiles
    # a sub-kernel of the strided data gradient called directly: a 2x1 window whose explicit output size is one larger than
    # the natural 3 x 5, so the last row and column read past the input and must read zeros
    "sdgrad_win2x1_out_hw": _c(2, 64, 4, 5, 32, (2, 1), pad=(0, 0), out_hw=(4, 6)),
    # column stride 2: W = 8 is the boundary of the two-load gather, W = 7 the scalar one
    "s2_w7": _c(4, 32, 7, 7, 64, 3, stride=(2, 2), pad=(1, 1)),
    "s2_w8": _c(4, 32, 8, 8, 64, 3, stride=(2, 2), pad=(1, 1)),
    "s2_w9": _c(4, 32, 9, 9, 64, 3, stride=(2, 2), pad=(1, 1)),
    "s2_w17": _c(4, 32, 17, 17, 64, 3, stride=(2, 2), pad=(1, 1)),
    "s2_1x1_w8": _c(4, 32, 8, 8, 64, 1, stride=(2, 2)),
    "s2_1x1_w9": _c(4, 32, 9, 9, 64, 1, stride=(2, 2)),
    "s12_w12": _c(4, 32, 12, 12, 64, 3, stride=(1, 2), pad=(1, 1)),
    "s21_w12": _c(4, 32, 12, 12, 64, 3, stride=(2, 1), pad=(1, 1)),
    "s3_w16": _c(4, 32, 16, 16, 64, 3, stride=(3, 3), pad=(1, 1)),
    # 128-row tiles from 512 workgroups
    "bm128_s2": _c(1, 32, 512, 256, 256, 3, stride=(2, 2), pad=(1, 1), copy=B128),       # 256 x 2 = 512
    "bm128_ragged": _c(1, 32, 252, 130, 130, 3, copy=B128),      # 260 x 2 = 520; 33 quads per row, the last half filled; Cout tail 2
    # Cout tails on 64-row tiles, odd map
    "cout40": _c(3, 32, 13, 11, 40, 3),
    "cout81": _c(3, 32, 13, 11, 81, 3),
    # the grid is padded to a multiple of 8 pixel tiles: 1 (7 workgroups return at once) and 9
    "grid_one_tile": _c(1, 32, 5, 7, 64, 3),                     # 40 virtual pixels
    "grid_nine_tiles": _c(2, 32, 20, 28, 64, 3),                 # 1120 virtual pixels
    # the epilogue shapes of the generic kernel: whole pixel tiles, OW % 4 == 0 -- the first Cout tile of 64 rows takes
    # epilogue_full_nchw, the second (32 of 64) the general path; and a ragged one (pair and scalar stores)
    "gen_epi": _c(2, 32, 12, 16, 96, 3),                         # 3 x 2 tiles
    "gen_ragged": _c(3, 32, 13, 11, 81, 3),
    # channels-last output: a part-filled Cout group of 32 rows, and whole 128-pixel tiles
    "cl_cout36": _c(2, 32, 9, 10, 36, 3),
    "cl_whole_tiles": _c(2, 32, 8, 16, 64, 3),                   # 256 virtual pixels
    # device live count: 48 virtual pixels per image, 3 tiles of 128
    "live_w6": _c(8, 32, 6, 6, 64, 3),
}
EPILOGUES = ["bias", "scale_bias", "residual", "gate", "relu", "all"]
# shape -> launched with a 16-bit copy
EPILOGUE_SHAPES = {"patch_straddle_cout160": True, "flat12_h10": True, "reg1x1_roi_cout160": True, "gen_epi": False,
                   "gen_ragged": False}


def _dot(name):
    N, Cin, H, W, Cout, r, s = CASES[name][:7]
    return Cin * r * s


def group(name):
    """The group a case's worst ratio is recorded under."""
    head = name.split("_")[0]
    return {"patch": "patch", "reg1x1": "reg1x1", "sdgrad": "strided_dgrad"}.get(head, "flat" if head.startswith("flat") else "generic")


@functools.lru_cache(maxsize=None)
def _problem(name, sfx):
    """Seeded operands of a shape (x, tap-major w as the launch reads it, its 16-bit copy) and the float64 reference /
    magnitude of the accumulator on operands rounded to the type.  Computed once per (shape, type), shared, never written."""
    N, Cin, H, W, Cout, r, s, sh, sw, ph, pw, layout, out_hw = CASES[name][:13]
    g = torch.Generator(device=DEV).manual_seed(1600 + sorted(CASES).index(name))
    x = torch.randn(N, Cin, H, W, device=DEV, generator=g)
    w = torch.randn(Cout, r, s, Cin, device=DEV, generator=g) / (Cin * r * s) ** 0.5
    dt = DTYPES[sfx]
    xr, wr = x.to(dt).float(), w.to(dt).float()
    if layout == 2:
        # the launch is the data gradient of a convolution whose weight is wf [Cin-of-the-launch, Cout-of-the-launch, R, S]
        assert out_hw is None
        wf = wr.permute(3, 0, 1, 2)
        ref = R.dgrad_ref(xr, wf, (sh, sw), (ph, pw), in_hw=(H, W))
        mag = R.dgrad_ref(xr.abs(), wf.abs(), (sh, sw), (ph, pw), in_hw=(H, W))
    else:
        wl = wr.permute(0, 3, 1, 2)
        ref = R.conv_ref(xr, wl, (sh, sw), (ph, pw), out_hw=out_hw)
        mag = R.conv_ref(xr.abs(), wl.abs(), (sh, sw), (ph, pw), out_hw=out_hw)
    return x, w, w.to(dt), ref, mag


@functools.lru_cache(maxsize=None)
def _epilogue_operands(name, sfx):
    """bias, scale [Cout], residual and gate (zeros where |g| < 0.3) of a shape's output; residual and gate are views at
    16 bytes of their buffers, so that [1:] of the same buffers puts them 4 bytes past a multiple of 16 (_shifted)."""
    ref = _problem(name, sfx)[3]
    g = torch.Generator(device=DEV).manual_seed(2600 + sorted(CASES).index(name))
    bias = torch.randn(ref.shape[1], device=DEV, generator=g)
    scale = torch.randn(ref.shape[1], device=DEV, generator=g)
    residual = torch.randn(ref.shape, device=DEV, generator=g)
    gate = torch.randn(ref.shape, device=DEV, generator=g)
    gate[gate.abs() < 0.3] = 0.0
    return bias, scale, residual, gate


def _shifted(t):
    """A contiguous copy of t whose address is 4 bytes past a multiple of 16."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def _launch(name, sfx, y, copy, expect=None, bias=None, scale=None, residual=None, gate=None, relu=0, output_layout=0,
            live=None):
    """Asserts the variant fi_conv2d_forward_plan_<sfx> names for exactly these arguments (CASES' unless `expect` is
    given), then launches fi_conv2d_forward_live_<sfx>; returns the variant."""
    from feature_intertwiner_amd import _lib
    L = _lib.load()
    x, w, w16 = _problem(name, sfx)[:3]
    N, Cin, H, W, Cout, r, s, sh, sw, ph, pw, layout, out_hw = CASES[name][:13]
    oh, ow = out_hw if out_hw is not None else (0, 0)
    args = (_lib.ptr(x), _lib.ptr(w), _lib.ptr(w16 if copy else None), _lib.ptr(bias), _lib.ptr(scale), _lib.ptr(residual),
            _lib.ptr(gate), _lib.ptr(y), N, Cin, H, W, Cout, r, s, sh, sw, ph, pw, relu, layout, oh, ow, output_layout)
    variant = _lib.CONV16_VARIANTS[_lib.conv16_variant(getattr(L, "fi_conv2d_forward_plan_" + sfx), *args)]
    assert variant == (expect if expect is not None else CASES[name][13 if copy else 14]), (name, sfx, copy, variant)
    _lib.check(getattr(L, "fi_conv2d_forward_live_" + sfx)(*args, _lib.ptr(live), _lib.current_stream()),
               "fi_conv2d_forward_live_" + sfx)
    torch.cuda.synchronize()
    return variant


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_is_the_float64_reference_at_every_kernels_edge(name, sfx):
    """With a 16-bit copy of the weight and without one (once where both plans are the same generic kernel, which never
    reads the copy)."""
    x, w, w16, ref, mag = _problem(name, sfx)
    copy_variant, plain_variant = CASES[name][13:15]
    out = []
    for copy in ((True, False) if copy_variant != plain_variant else (False,)):
        y = _nan(*ref.shape)
        variant = _launch(name, sfx, y, copy)
        worst = R.check_bar(y, ref, mag, _dot(name), "%s %s (%s)" % (name, sfx, variant))
        out.append("%s %.2f" % (variant, worst))
        print("RATIO %s %s %s %s %.2f" % (group(name), name, sfx, variant, worst))
    print("%s %s %s: worst |d|/(2^-24 m) %s" % (name, sfx, CASES[name][:13], ", ".join(out)))


def _epilogue_kw(kind, bias, scale, residual, gate):
    return {"bias": dict(bias=bias), "scale_bias": dict(scale=scale, bias=bias), "residual": dict(residual=residual),
            "gate": dict(gate=gate), "relu": dict(relu=1),
            "all": dict(scale=scale, bias=bias, residual=residual, gate=gate, relu=1)}[kind]


def _check_epilogue(name, sfx, kind, copy, shift):
    x, w, w16, acc, acc_mag = _problem(name, sfx)
    bias, scale, residual, gate = _epilogue_operands(name, sfx)
    kw = _epilogue_kw(kind, bias, scale, residual, gate)
    launch_kw = {k: (_shifted(v) if shift and k in ("residual", "gate") else v) for k, v in kw.items()}
    y = _nan(*acc.shape)
    variant = _launch(name, sfx, y, copy, **launch_kw)
    ep = dict(kw)
    relu = bool(ep.pop("relu", 0))
    ref = R.epilogue(acc, relu=relu, **ep)
    ep.pop("gate", None)
    mag = R.abs_epilogue(acc_mag, **ep)
    what = "%s %s %s%s (%s)" % (name, sfx, kind, " shifted" if shift else "", variant)
    worst = R.check_bar(y, ref, mag, _dot(name), what)
    if "gate" in kw:
        assert not y[gate <= 0].any(), what                      # exact zeros, not small numbers
    print("RATIO epilogues %s %s %s %.2f" % (name, sfx, what.replace(" ", "_"), worst))


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("kind", EPILOGUES)
@pytest.mark.parametrize("name", sorted(EPILOGUE_SHAPES))
def test_forward_epilogues_are_the_float64_reference(name, kind, sfx):
    """bias, scale + bias, residual, gate and ReLU in every variant's epilogue, one at a time and all together.  gen_epi
    runs epilogue_full_nchw (first Cout tile) and the general path (second) in one launch; gen_ragged the general path's
    pair and scalar stores; the patch and 1x1 rows a whole and a 32-of-128 Cout tile; the flat row its 8-byte pairs."""
    _check_epilogue(name, sfx, kind, EPILOGUE_SHAPES[name], shift=False)


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("kind", ["residual", "gate", "all"])
@pytest.mark.parametrize("name", ["gen_epi", "gen_ragged"])
def test_generic_epilogue_reads_residual_and_gate_at_a_4_byte_offset(name, kind, sfx):
    _check_epilogue(name, sfx, kind, False, shift=True)


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("kind", ["bias", "scale_bias", "relu"])
@pytest.mark.parametrize("name", ["cl_cout36", "cl_whole_tiles"])
def test_channels_last_output_of_the_generic_kernel(name, kind, sfx):
    """output_layout 1: the result, permuted to NCHW, is within the bar and bit-equal to the NCHW launch of the same call."""
    x, w, w16, acc, acc_mag = _problem(name, sfx)
    bias, scale, _, _ = _epilogue_operands(name, sfx)
    kw = _epilogue_kw(kind, bias, scale, None, None)
    N, Cout, OH, OW = acc.shape
    y_cl, y = _nan(N, OH, OW, Cout), _nan(N, Cout, OH, OW)
    variant = _launch(name, sfx, y_cl, False, output_layout=1, **kw)
    _launch(name, sfx, y, False, **kw)
    ep = dict(kw)
    relu = bool(ep.pop("relu", 0))
    got = y_cl.permute(0, 3, 1, 2)
    worst = R.check_bar(got, R.epilogue(acc, relu=relu, **ep), R.abs_epilogue(acc_mag, **ep), _dot(name),
                        "%s %s %s channels-last (%s)" % (name, sfx, kind, variant))
    assert torch.equal(got, y), (name, sfx, kind, float((got - y).abs().max()))
    print("RATIO generic %s %s channels-last_%s %.2f" % (name, sfx, kind, worst))


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("count", [0, 1, 3, 8])
def test_live_count_that_ends_inside_a_tile(count, sfx):
    """include/fi_capi.h: tiles whose pixels all lie in images >= *n_live_dev are skipped, their outputs not written.  8
    images of 48 virtual pixels (6 rows of two quads) on tiles of 128: a count of 3 ends 16 pixels into the second tile.
    Images below the count are the reference; images whose tiles all start at or past the count keep the NaN fill."""
    name = "live_w6"
    x, w, w16, ref, mag = _problem(name, sfx)
    N, per_image, tile = 8, 6 * 2 * 4, 128
    live = torch.tensor([count], device=DEV, dtype=torch.int32)
    y = _nan(*ref.shape)
    variant = _launch(name, sfx, y, False, live=live)
    worst = 0.0
    if count:
        worst = R.check_bar(y[:count], ref[:count], mag[:count], _dot(name), "live_w6 %s count %d (%s)" % (sfx, count, variant))
    skipped = [n for n in range(N) if (n * per_image // tile) * tile >= count * per_image]
    assert skipped == {0: list(range(8)), 1: [3, 4, 5, 6, 7], 3: [6, 7], 8: []}[count]
    for n in skipped:
        assert torch.isnan(y[n]).all(), (count, n)
    print("RATIO generic %s %s live_count_%d %.2f" % (name, sfx, count, worst))


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("name", ["patch_h3", "reg1x1_hw4"])
def test_patch_and_1x1_kernels_compute_every_image_under_a_live_count(name, sfx):
    """fi_conv2d_forward_live_<p>: the patch / 1x1 kernels compute every image."""
    x, w, w16, ref, mag = _problem(name, sfx)
    live = torch.tensor([1], device=DEV, dtype=torch.int32)
    y = _nan(*ref.shape)
    variant = _launch(name, sfx, y, True, live=live)
    worst = R.check_bar(y, ref, mag, _dot(name), "%s %s with a live count of 1 (%s)" % (name, sfx, variant))
    print("RATIO %s %s %s live_count_1 %.2f" % (group(name), name, sfx, worst))


# ---- the strided data gradient ---------------------------------------------------------------------------------------
# name -> (window, stride, pad, in_hw); Cout 64 -> Cin 32.  Odd sizes make the residue classes differ in size; on (8, 8)
# the 2-tap classes ask for one output row / column more than their window gives (the launch's explicit out_h / out_w)
STRIDED = {
    "3x3_s2_7x9": (3, 2, 1, (7, 9)),
    "3x3_s2_8x8": (3, 2, 1, (8, 8)),
    "1x1_s2_7x9": (1, 2, 0, (7, 9)),
    "1x1_s2_8x8": (1, 2, 0, (8, 8)),
    "3x3_s3_7x7": (3, 3, 1, (7, 7)),
}


def check_strided_dgrad(name, precision, dt=None):
    """conv._strided_dgrad of a STRIDED row under `precision` against dgrad_ref on operands rounded to dt (None: fp32, not
    rounded); n of an element: Cout times the taps that reach its class.  Returns the worst |d| / (2^-24 m)."""
    from feature_intertwiner_amd import conv as C
    k, st, pd, (H, W) = STRIDED[name]
    N, Cout, Cin = 2, 64, 32
    OH, OW = R.out_size(H, W, k, k, (st, st), (pd, pd))
    g = torch.Generator(device=DEV).manual_seed(3600 + sorted(STRIDED).index(name))
    dz = torch.randn(N, Cout, OH, OW, device=DEV, generator=g)
    w = torch.randn(Cout, Cin, k, k, device=DEV, generator=g) / (Cout * k * k) ** 0.5
    dzr, wr = (dz, w) if dt is None else (dz.to(dt).float(), w.to(dt).float())
    ref = R.dgrad_ref(dzr, wr, (st, st), (pd, pd), in_hw=(H, W))
    mag = R.dgrad_ref(dzr.abs(), wr.abs(), (st, st), (pd, pd), in_hw=(H, W))
    n = torch.zeros(1, 1, H, W, device=DEV, dtype=torch.float64)
    windows = set()
    for a in range(min(st, H)):
        for b in range(min(st, W)):
            Th, Tw = C._class_taps(a, k, st, pd)[1], C._class_taps(b, k, st, pd)[1]
            n[:, :, a::st, b::st] = Cout * Th * Tw
            if Th * Tw:
                windows.add((Th, Tw))
    assert windows == ({(1, 1), (1, 2), (2, 1), (2, 2)} if (k, st) == (3, 2) else {(1, 1)})
    C.invalidate_step_state()
    try:
        got = C._strided_dgrad(dz, w, (H, W), (st, st), (pd, pd), precision=precision)
        torch.cuda.synchronize()
    finally:
        C.invalidate_step_state()
    worst = R.check_bar(got, ref, mag, n, "strided dgrad %s %s" % (name, precision))
    assert not got[(n == 0).expand_as(got)].any()                # positions no tap reaches: exact zeros
    return worst


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("name", sorted(STRIDED))
def test_strided_data_gradient_is_the_float64_reference(name, sfx):
    """One stride-1 launch per residue class of the input positions: 1x1, 1x2, 2x1 and 2x2 windows with an explicit output
    size."""
    worst = check_strided_dgrad(name, PRECISION[sfx], DTYPES[sfx])
    print("RATIO strided_dgrad %s %s _strided_dgrad %.2f" % (name, sfx, worst))
