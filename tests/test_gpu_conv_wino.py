"""conv3x3_wino_flat_kernel, the Winograd F(2x2,3x3) form of the conv3x3_patch_flat slot (3x3 / stride 1 / pad 1 on 14 x 14
maps, Cin >= 64), held to float64 element by element with the project's bar of tests/fp64_ref.py, 2^-24 (4 sqrt(n) + 16) m,
unchanged: a CPU emulation of the algorithm with a sequential fp32 channel chain stayed within 3.6 units of 2^-24 m on
random and post-ReLU inputs (direct form: 1.7 - 4.7), the bar at Cin 64 is 112 units.

Shapes (N, Cin, 14, 14, Cout) are the smallest the flat rule admits (168 images x 2 Cout tiles = 516 flat tiles; 8232
Winograd tiles = 257 groups of 32 and a quarter of one, groups that span image boundaries), an odd image count, odd and
even numbers of 16-channel blocks (LDS buffer parity), a partly filled second Cout tile, and the neighbours that must stay
on the kernels they had: N = 166 (conv_fwd_bm64_3x3), Cin = 48 and Cin = 16 (the direct flat kernel).  Both forms share
the plan key and the profiling counter, so that the variant ran is shown by running a case with and without FI_NO_WINOGRAD:
one launch counted each time, both within the bar, and outputs that differ in at least one bit."""
import functools
import os

import pytest
import torch

import fp64_ref as R
from test_gpu_conv16_plan import _nan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLAT_KEY = "conv3x3_patch_flat"

# name -> (N, Cin, Cout, weight_layout, expected kernel key, Winograd form expected)
SHAPES = {
    "w64": (168, 64, 256, 1, FLAT_KEY, True),
    "w64_dgrad": (168, 64, 256, 2, FLAT_KEY, True),
    "w64_n169": (169, 64, 256, 1, FLAT_KEY, True),
    "w80": (168, 80, 256, 1, FLAT_KEY, True),
    "w96": (168, 96, 256, 1, FLAT_KEY, True),
    "w64_cout160": (168, 64, 160, 1, FLAT_KEY, True),
    "nb_n166": (166, 64, 256, 1, "conv_fwd_bm64_3x3", False),
    "nb_cin48": (168, 48, 256, 1, FLAT_KEY, False),
    "nb_cin16": (168, 16, 256, 1, FLAT_KEY, False),
}
EPILOGUES = ["bias", "scale_bias", "residual", "gate", "relu", "all"]


@functools.lru_cache(maxsize=None)
def _problem(name):
    """Seeded operands (x, w as the launch reads it) and the float64 reference / magnitude; computed once, never written."""
    N, Cin, Cout, layout = SHAPES[name][:4]
    g = torch.Generator(device=DEV).manual_seed(7000 + sorted(SHAPES).index(name))
    x = torch.randn(N, Cin, 14, 14, device=DEV, generator=g)
    w = torch.randn(Cout, 3, 3, Cin, device=DEV, generator=g) / (Cin * 9) ** 0.5
    if layout == 2:
        wf = w.permute(3, 0, 1, 2)          # the forward weight [Cin-of-the-launch, Cout-of-the-launch, R, S]
        ref = R.dgrad_ref(x, wf, (1, 1), (1, 1), in_hw=(14, 14))
        mag = R.dgrad_ref(x.abs(), wf.abs(), (1, 1), (1, 1), in_hw=(14, 14))
    else:
        wl = w.permute(0, 3, 1, 2)
        ref = R.conv_ref(x, wl, (1, 1), (1, 1))
        mag = R.conv_ref(x.abs(), wl.abs(), (1, 1), (1, 1))
    return x, w, ref, mag


def _offset8(t):
    """A copy of t at an address that is a multiple of 8 but not of 16."""
    buf = torch.empty(t.numel() + 4, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[2:2 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 8
    return v


@functools.lru_cache(maxsize=None)
def _epilogue_operands(name):
    """bias, scale [Cout], residual and gate (zeros where |g| < 0.3), the last two at 8-byte-but-not-16-byte addresses."""
    ref = _problem(name)[2]
    g = torch.Generator(device=DEV).manual_seed(8000 + sorted(SHAPES).index(name))
    bias = torch.randn(ref.shape[1], device=DEV, generator=g)
    scale = torch.randn(ref.shape[1], device=DEV, generator=g)
    residual = torch.randn(ref.shape, device=DEV, generator=g)
    gate = torch.randn(ref.shape, device=DEV, generator=g)
    gate[gate.abs() < 0.3] = 0.0
    return bias, scale, _offset8(residual), _offset8(gate)


def _launch(name, y, x=None, bias=None, scale=None, residual=None, gate=None, relu=0):
    """Asserts the planned key, then launches fi_conv2d_forward_live (or _gated); returns the launches counted under it."""
    from feature_intertwiner_amd import _lib
    L = _lib.load()
    x0, w = _problem(name)[:2]
    x = x0 if x is None else x
    N, Cin, Cout, layout, expect = SHAPES[name][:5]
    args = (_lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(scale), _lib.ptr(residual), _lib.ptr(gate), _lib.ptr(y),
            N, Cin, 14, 14, Cout, 3, 3, 1, 1, 1, 1, relu, layout, 0, 0, 0)
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
    N, Cin, Cout, layout = SHAPES[name][:4]
    (launch,) = _lib.planned_launches(_lib.load().fi_conv2d_forward_launches, _lib.ptr(x), _lib.ptr(w), None, None, None, None,
                                      _lib.ptr(y), N, Cin, 14, 14, Cout, 3, 3, 1, 1, 1, 1, 0, layout, 0, 0, 0)
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
@pytest.mark.parametrize("name", ["w64", "w64_dgrad", "w64_cout160"])
def test_epilogues(name, kind):
    """scale, bias, residual, ReLU and gate, one at a time and all together; residual and gate 8-byte aligned only."""
    x, w, acc, acc_mag = _problem(name)
    bias, scale, residual, gate = _epilogue_operands(name)
    kw = {"bias": dict(bias=bias), "scale_bias": dict(scale=scale, bias=bias), "residual": dict(residual=residual),
          "gate": dict(gate=gate), "relu": dict(relu=1),
          "all": dict(scale=scale, bias=bias, residual=residual, gate=gate, relu=1)}[kind]
    y = _nan(*acc.shape)
    _launch(name, y, **kw)
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
    x, w, ref, mag = _problem("w64")
    y = _nan(*ref.shape)
    _launch("w64", y)
    g = torch.Generator(device=DEV).manual_seed(7100)
    x2 = torch.randn(x.shape, device=DEV, generator=g)
    x2[100] = x[3]
    y2 = _nan(*ref.shape)
    _launch("w64", y2, x=x2)
    assert torch.equal(y2[100].view(torch.int32), y[3].view(torch.int32))
    assert not torch.equal(y2[99], y[2])


@pytest.mark.parametrize("name", ["w64", "w64_dgrad"])
def test_the_winograd_form_ran(name):
    """With and without FI_NO_WINOGRAD: the planned form, the same key, one launch counted each, both within the bar,
    different bits."""
    x, w, ref, mag = _problem(name)
    y_w, y_d = _nan(*ref.shape), _nan(*ref.shape)
    assert _form(name, y_w) == "WINO14" and _direct(lambda: _form(name, y_d)) == "PATCH_FLAT13"
    assert _launch(name, y_w) == 1
    assert _direct(lambda: _launch(name, y_d)) == 1
    worst_w = R.check_bar(y_w, ref, mag, SHAPES[name][1] * 9, name + " winograd")
    worst_d = R.check_bar(y_d, ref, mag, SHAPES[name][1] * 9, name + " direct")
    differ = int((y_w.view(torch.int32) != y_d.view(torch.int32)).sum())
    print("%s: worst |d|/(2^-24 m) winograd %.2f, direct %.2f; %d of %d elements differ" % (
        name, worst_w, worst_d, differ, y_w.numel()))
    assert differ >= 1


@pytest.mark.parametrize("name", ["nb_cin48", "nb_cin16"])
def test_narrow_layers_keep_the_direct_kernel(name):
    """Cin < 64: the switch changes nothing, bit for bit."""
    x, w, ref, mag = _problem(name)
    y_a, y_b = _nan(*ref.shape), _nan(*ref.shape)
    _launch(name, y_a)
    _direct(lambda: _launch(name, y_b))
    assert torch.equal(y_a.view(torch.int32), y_b.view(torch.int32))
