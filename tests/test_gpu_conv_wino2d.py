"""conv3x3_wino_flat_kernel on 2-D maps: the Winograd F(2x2,3x3) form of the conv3x3_patch slot (3x3 / stride 1 / pad 1,
W % 16 == 0, even H, Cin >= 64, NCHW output, 8-byte aligned y / residual / gate), held to float64 element by element with
the project's bar of tests/fp64_ref.py, 2^-24 (4 sqrt(n) + 16) m with n = 9 Cin, unchanged (112 units at Cin 64; measured:
at most 3.43 units of 2^-24 m over the Winograd cases, 5.4 - 7.1 for the direct kernels on the same shapes).

Shapes (N, Cin, H, W, Cout) are the smallest the 2-D patch rule admits, ceil(N H / 8) (W / 16) ceil(Cout / 128) >= 256:
128 x 128 (4096 tiles, exactly 128 groups of 32), 103 images of 10 x 16 (8 tiles per row, 5 tile rows: every group spans
image boundaries, 4120 tiles leave the last group a quarter full, H % 8 != 0), 70 x 48 (24 tiles per row: groups wrap in
mid-row), odd and even numbers of 16-channel blocks (LDS buffer parity), a partly filled second Cout tile, four Cout tiles;
and the neighbours that keep the kernels they had: odd H, Cin 48, channels-last output and a 4-byte aligned y (the direct
patch kernel, bit-identical with and without FI_NO_WINOGRAD), 240 workgroups (conv_fwd_bm64_3x3).  Both forms share the
plan key and the profiling counter, so that the Winograd form ran is shown by running a case with and without
FI_NO_WINOGRAD: one launch counted each time, both within the bar, and outputs that differ in at least one bit."""
import functools
import os

import pytest
import torch

import fp64_ref as R
from test_gpu_conv16_plan import _nan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATCH_KEY = "conv3x3_patch"

# name -> (N, Cin, H, W, Cout, weight_layout, expected kernel key)
SHAPES = {
    "s128": (1, 64, 128, 128, 256, 1, PATCH_KEY),
    "s128_dgrad": (1, 64, 128, 128, 256, 2, PATCH_KEY),
    "n103": (103, 64, 10, 16, 256, 1, PATCH_KEY),
    "n103_dgrad": (103, 64, 10, 16, 256, 2, PATCH_KEY),
    "w48": (5, 64, 70, 48, 256, 1, PATCH_KEY),
    "cin80": (1, 80, 128, 128, 256, 1, PATCH_KEY),
    "cin96": (1, 96, 128, 128, 256, 1, PATCH_KEY),
    "cout160": (1, 64, 128, 128, 160, 1, PATCH_KEY),
    "cout512": (1, 64, 64, 128, 512, 1, PATCH_KEY),
    "nb_odd_h": (3, 64, 43, 128, 256, 1, PATCH_KEY),
    "nb_cin48": (1, 48, 128, 128, 256, 1, PATCH_KEY),
    "nb_wg240": (1, 64, 120, 128, 256, 1, "conv_fwd_bm64_3x3"),
}
WINOGRAD = ["s128", "s128_dgrad", "n103", "n103_dgrad", "w48", "cin80", "cin96", "cout160", "cout512"]
EPILOGUES = ["bias", "scale_bias", "residual", "gate", "relu", "all"]


@functools.lru_cache(maxsize=None)
def _problem(name):
    """Seeded operands (x, w as the launch reads it) and the float64 reference / magnitude; computed once, never written."""
    N, Cin, H, W, Cout, layout = SHAPES[name][:6]
    g = torch.Generator(device=DEV).manual_seed(9000 + sorted(SHAPES).index(name))
    x = torch.randn(N, Cin, H, W, device=DEV, generator=g)
    w = torch.randn(Cout, 3, 3, Cin, device=DEV, generator=g) / (Cin * 9) ** 0.5
    if layout == 2:
        wf = w.permute(3, 0, 1, 2)          # the forward weight [Cin-of-the-launch, Cout-of-the-launch, R, S]
        ref = R.dgrad_ref(x, wf, (1, 1), (1, 1), in_hw=(H, W))
        mag = R.dgrad_ref(x.abs(), wf.abs(), (1, 1), (1, 1), in_hw=(H, W))
    else:
        wl = w.permute(0, 3, 1, 2)
        ref = R.conv_ref(x, wl, (1, 1), (1, 1))
        mag = R.conv_ref(x.abs(), wl.abs(), (1, 1), (1, 1))
    return x, w, ref, mag


def _offset(t, byte):
    """A copy of t at an address that is `byte` (4 or 8) past a multiple of 16."""
    buf = torch.empty(t.numel() + 4, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[byte // 4:byte // 4 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == byte
    return v


@functools.lru_cache(maxsize=None)
def _epilogue_operands(name):
    """bias, scale [Cout], residual and gate (zeros where |g| < 0.3), the last two at 8-byte-but-not-16-byte addresses."""
    ref = _problem(name)[2]
    g = torch.Generator(device=DEV).manual_seed(9500 + sorted(SHAPES).index(name))
    bias = torch.randn(ref.shape[1], device=DEV, generator=g)
    scale = torch.randn(ref.shape[1], device=DEV, generator=g)
    residual = torch.randn(ref.shape, device=DEV, generator=g)
    gate = torch.randn(ref.shape, device=DEV, generator=g)
    gate[gate.abs() < 0.3] = 0.0
    return bias, scale, _offset(residual, 8), _offset(gate, 8)


def _launch(name, y, x=None, bias=None, scale=None, residual=None, gate=None, relu=0, output_layout=0):
    """Asserts the planned key, then launches fi_conv2d_forward_live (or _gated); returns the launches counted under it."""
    from feature_intertwiner_amd import _lib
    L = _lib.load()
    x0, w = _problem(name)[:2]
    x = x0 if x is None else x
    N, Cin, H, W, Cout, layout, expect = SHAPES[name]
    args = (_lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(scale), _lib.ptr(residual), _lib.ptr(gate), _lib.ptr(y),
            N, Cin, H, W, Cout, 3, 3, 1, 1, 1, 1, relu, layout, 0, 0, output_layout)
    key = _lib.planned_kernel(L.fi_conv2d_forward_plan, *args)
    assert key == expect, (name, key)
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        if gate is not None:
            _lib.check(L.fi_conv2d_forward_gated(*args, _lib.current_stream()), "fi_conv2d_forward_gated")
        else:
            _lib.check(L.fi_conv2d_forward_live(*args, None, _lib.current_stream()), "fi_conv2d_forward_live")
        torch.cuda.synchronize()
    finally:
        _lib.prof_enable(False)
    return _lib.prof_get(key)[0]


def _form(name, y):
    """The _lib.FWD_FORMS name of the one launch fi_conv2d_forward_launches plans for the shape."""
    from feature_intertwiner_amd import _lib
    x, w = _problem(name)[:2]
    N, Cin, H, W, Cout, layout = SHAPES[name][:6]
    (launch,) = _lib.planned_launches(_lib.load().fi_conv2d_forward_launches, _lib.ptr(x), _lib.ptr(w), None, None, None, None,
                                      _lib.ptr(y), N, Cin, H, W, Cout, 3, 3, 1, 1, 1, 1, 0, layout, 0, 0, 0)
    return _lib.FWD_FORMS[launch.form]


def _direct(fn):
    """fn() with FI_NO_WINOGRAD=1 (the library reads it per call)."""
    old = os.environ.get("FI_NO_WINOGRAD")
    os.environ["FI_NO_WINOGRAD"] = "1"
    try:
        return fn()
    finally:
        if old is None:
            del os.environ["FI_NO_WINOGRAD"]
        else:
            os.environ["FI_NO_WINOGRAD"] = old


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.fixture(autouse=True)
def _switch_unset():
    assert "FI_NO_WINOGRAD" not in os.environ and "FI_NO_PATCH" not in os.environ
    yield


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_forward_and_data_gradient_are_the_float64_reference(name):
    x, w, ref, mag = _problem(name)
    y = _nan(*ref.shape)
    assert _launch(name, y) == 1
    worst = R.check_bar(y, ref, mag, SHAPES[name][1] * 9, name)
    print("%s %s: worst |d|/(2^-24 m) %.2f" % (name, SHAPES[name], worst))


@pytest.mark.parametrize("kind", EPILOGUES)
@pytest.mark.parametrize("name", ["s128", "s128_dgrad", "cout160"])
def test_epilogues(name, kind):
    """scale, bias, residual, ReLU and gate, one at a time and all together; residual and gate 8-byte aligned only."""
    x, w, acc, acc_mag = _problem(name)
    bias, scale, residual, gate = _epilogue_operands(name)
    kw = {"bias": dict(bias=bias), "scale_bias": dict(scale=scale, bias=bias), "residual": dict(residual=residual),
          "gate": dict(gate=gate), "relu": dict(relu=1),
          "all": dict(scale=scale, bias=bias, residual=residual, gate=gate, relu=1)}[kind]
    y = _nan(*acc.shape)
    assert _launch(name, y, **kw) == 1
    ep = dict(kw)
    relu = bool(ep.pop("relu", 0))
    ref = R.epilogue(acc, relu=relu, **ep)
    ep.pop("gate", None)
    mag = R.abs_epilogue(acc_mag, **ep)
    worst = R.check_bar(y, ref, mag, SHAPES[name][1] * 9, "%s %s" % (name, kind))
    if "gate" in kw:
        assert not y[gate <= 0].any()                            # exact zeros, not small numbers
    print("%s %s: worst |d|/(2^-24 m) %.2f" % (name, kind, worst))


def test_an_image_gives_the_same_bits_wherever_it_sits_in_the_batch():
    """10 x 16 maps are 40 tiles: groups of 32 straddle images, and an image starts at every multiple of 8 in a group."""
    x, w, ref, mag = _problem("n103")
    y = _nan(*ref.shape)
    _launch("n103", y)
    g = torch.Generator(device=DEV).manual_seed(9100)
    x2 = torch.randn(x.shape, device=DEV, generator=g)
    moves = [(3, 100), (0, 102), (50, 1), (77, 42)]              # tile offsets 120 -> 4000, 0 -> 4080, 2000 -> 40, ...
    for src, dst in moves:
        x2[dst] = x[src]
    y2 = _nan(*ref.shape)
    _launch("n103", y2, x=x2)
    for src, dst in moves:
        assert _same_bits(y2[dst], y[src]), (src, dst)
    assert not torch.equal(y2[99], y[2])


@pytest.mark.parametrize("name", ["s128", "s128_dgrad"])
def test_the_winograd_form_ran(name):
    """With and without FI_NO_WINOGRAD: the planned form, the same key, one launch counted each, both within the bar,
    different bits."""
    x, w, ref, mag = _problem(name)
    y_w, y_d = _nan(*ref.shape), _nan(*ref.shape)
    assert _form(name, y_w) == "WINO" and _direct(lambda: _form(name, y_d)) == "PATCH"
    assert _launch(name, y_w) == 1
    assert _direct(lambda: _launch(name, y_d)) == 1
    worst_w = R.check_bar(y_w, ref, mag, SHAPES[name][1] * 9, name + " winograd")
    worst_d = R.check_bar(y_d, ref, mag, SHAPES[name][1] * 9, name + " direct")
    differ = int((y_w.view(torch.int32) != y_d.view(torch.int32)).sum())
    print("%s: worst |d|/(2^-24 m) winograd %.2f, direct %.2f; %d of %d elements differ" % (
        name, worst_w, worst_d, differ, y_w.numel()))
    assert differ >= 1


@pytest.mark.parametrize("name", ["nb_odd_h", "nb_cin48"])
def test_odd_heights_and_narrow_layers_keep_the_direct_kernel(name):
    """Odd H, Cin < 64: the switch changes nothing, bit for bit."""
    x, w, ref, mag = _problem(name)
    y_a, y_b = _nan(*ref.shape), _nan(*ref.shape)
    assert _launch(name, y_a) == 1
    assert _direct(lambda: _launch(name, y_b)) == 1
    R.check_bar(y_a, ref, mag, SHAPES[name][1] * 9, name)
    assert _same_bits(y_a, y_b)


def test_channels_last_output_keeps_the_direct_kernel():
    x, w, ref, mag = _problem("s128")
    N, Cin, H, W, Cout = SHAPES["s128"][:5]
    y_a, y_b = _nan(N, H, W, Cout), _nan(N, H, W, Cout)
    assert _launch("s128", y_a, output_layout=1) == 1
    assert _direct(lambda: _launch("s128", y_b, output_layout=1)) == 1
    R.check_bar(y_a, ref.permute(0, 2, 3, 1), mag.permute(0, 2, 3, 1), Cin * 9, "s128 channels-last")
    assert _same_bits(y_a, y_b)


def test_a_four_byte_aligned_output_keeps_the_direct_kernel():
    x, w, ref, mag = _problem("s128")
    y_a = _offset(_nan(*ref.shape), 4)
    y_b = _offset(_nan(*ref.shape), 4)
    assert _launch("s128", y_a) == 1
    assert _direct(lambda: _launch("s128", y_b)) == 1
    R.check_bar(y_a, ref, mag, SHAPES["s128"][1] * 9, "s128 y % 8 == 4")
    assert _same_bits(y_a, y_b)


def test_closed_gates_give_exact_zeros():
    x, w, acc, acc_mag = _problem("s128")
    bias, scale, residual, gate = _epilogue_operands("s128")
    closed = _offset(torch.zeros_like(gate), 8)
    y = _nan(*acc.shape)
    assert _launch("s128", y, scale=scale, bias=bias, residual=residual, gate=closed) == 1
    assert not y.view(torch.int32).any()
