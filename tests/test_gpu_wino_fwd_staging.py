"""The input staging of conv3x3_wino_flat_kernel (csrc/conv3x3_wino.hip): per window row one 8-byte load of the two centre
columns, the halo columns from the neighbouring lanes by a wave shift and one 4-byte load for the edges of a group of 32 tiles
(FI_WINO_STAGING_PAIR, taken when x is 8-byte aligned), against the staging with 4-byte loads only that
FI_WINO_SCALAR_STAGING=1 (read per call) or an x at a 4-byte address selects.  Both stage the same values, so y is the same bit
for bit; each case also holds y to float64 with the project's bar of tests/fp64_ref.py, 2^-24 (4 sqrt(n) + 16) m, n = 9 Cin.
y is NaN-filled before every launch, and every launch asserts its planned key first.

The shapes are rows of tests/test_gpu_conv_wino.py (14 x 14: 7 tiles a row, a group of 32 wraps rows four times and spans
images; N 169 leaves the last group partly full) and tests/test_gpu_conv_wino2d.py (10 x 16: 8 tiles a row, the last group a
quarter full; 70 x 48: 24 tiles a row, groups begin and end in mid-row, so the edge loads of tiles 0 and 31 carry real data;
128 x 128: a group is half a row), whose operands and float64 references are shared, not recomputed.

The exactness test puts powers of two at the places where a halo could come from the wrong lane (corners, columns 0 and
W - 1, both sides of a group cut, the last pixel of the batch) and takes weights that are multiples of 1/4 in [-2, 2]: every
transform-domain value, product and sum is then a multiple of 2^-4 below 2^18, exact in fp32, so y equals the float64
reference with either staging."""
import os

import pytest
import torch

import fp64_ref as R
import test_gpu_conv_wino as F
import test_gpu_conv_wino2d as D
from test_gpu_conv16_plan import _nan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SWITCH = "FI_WINO_SCALAR_STAGING"

# (module of the row, name): five group geometries, a data gradient (flip) of each slot, Cin 80 (an odd number of blocks),
# Cout 160
CASES = [(F, "w64"), (F, "w64_n169"), (D, "n103"), (D, "w48"), (D, "s128"), (F, "w64_dgrad"), (D, "s128_dgrad"), (F, "w80"),
         (D, "cout160")]


def _scalar(fn):
    """fn() with FI_WINO_SCALAR_STAGING=1 (the library reads it per call)."""
    assert SWITCH not in os.environ
    os.environ[SWITCH] = "1"
    try:
        return fn()
    finally:
        del os.environ[SWITCH]


@pytest.fixture(autouse=True)
def _switches_unset():
    assert SWITCH not in os.environ and "FI_NO_WINOGRAD" not in os.environ and "FI_NO_PATCH" not in os.environ
    yield


def _geom(mod, name):
    """(N, Cin, H, W, Cout, weight_layout) of a row of either module's table."""
    s = mod.SHAPES[name]
    return (s[0], s[1], 14, 14, s[2], s[3]) if mod is F else s[:6]


def _planned(x, w, y, geom):
    """(form, staging) of the one launch planned for these operands."""
    from feature_intertwiner_amd import _lib
    N, Cin, H, W, Cout, layout = geom
    (p,) = _lib.planned_launches(_lib.load().fi_conv2d_forward_launches, _lib.ptr(x), _lib.ptr(w), None, None, None, None,
                                 _lib.ptr(y), N, Cin, H, W, Cout, 3, 3, 1, 1, 1, 1, 0, layout, 0, 0, 0)
    return _lib.FWD_FORMS[p.form], _lib.WINO_STAGINGS[p.staging]


def _both(mod, name, x=None, **kw):
    """The row launched with the planned staging and with the switch: (y, y_scalar), both plans asserted."""
    x0, w, ref = mod._problem(name)[:3]
    x = x0 if x is None else x
    form = "WINO14" if mod is F else "WINO"
    y_p, y_s = _nan(*ref.shape), _nan(*ref.shape)
    assert _planned(x, w, y_p, _geom(mod, name)) == (form, "PAIR")
    assert _scalar(lambda: _planned(x, w, y_s, _geom(mod, name))) == (form, "SCALAR")
    assert mod._launch(name, y_p, x=x, **kw) == 1
    assert _scalar(lambda: mod._launch(name, y_s, x=x, **kw)) == 1
    return y_p, y_s


@pytest.mark.parametrize("mod,name", CASES, ids=[n for _, n in CASES])
def test_both_stagings_give_the_same_bits_within_the_float64_bar(mod, name):
    x, w, ref, mag = mod._problem(name)
    y_p, y_s = _both(mod, name)
    assert torch.equal(y_p, y_s)
    worst = R.check_bar(y_p, ref, mag, _geom(mod, name)[1] * 9, name)
    print("%s %s: worst |d|/(2^-24 m) %.2f" % (name, _geom(mod, name), worst))


@pytest.mark.parametrize("mod,name", [(F, "w64"), (D, "s128")], ids=["w64", "s128"])
def test_full_epilogue(mod, name):
    """scale, bias, residual, ReLU and gate together."""
    x, w, acc, acc_mag = mod._problem(name)
    bias, scale, residual, gate = mod._epilogue_operands(name)
    y_p, y_s = _both(mod, name, scale=scale, bias=bias, residual=residual, gate=gate, relu=1)
    assert torch.equal(y_p, y_s)
    ref = R.epilogue(acc, relu=True, scale=scale, bias=bias, residual=residual, gate=gate)
    mag = R.abs_epilogue(acc_mag, scale=scale, bias=bias, residual=residual)
    R.check_bar(y_p, ref, mag, _geom(mod, name)[1] * 9, name + " all")
    assert not y_p[gate <= 0].any()


@pytest.mark.parametrize("name", ["w48", "s128_dgrad"])
def test_an_x_at_a_four_byte_address_takes_the_scalar_staging(name):
    """The 2-D rule does not ask for an aligned x: the plan says SCALAR, the form stays, the bits are the aligned run's."""
    x, w, ref, mag = D._problem(name)
    y_p, y_s = _both(D, name)
    x4 = D._offset(x, 4)
    assert x4.data_ptr() % 8 == 4
    y_4 = _nan(*ref.shape)
    assert _planned(x4, w, y_4, _geom(D, name)) == ("WINO", "SCALAR")
    assert D._launch(name, y_4, x=x4) == 1
    assert torch.equal(y_4, y_p) and torch.equal(y_4, y_s)
    R.check_bar(y_4, ref, mag, _geom(D, name)[1] * 9, name + " x % 8 == 4")


def _hot_pixels(N, H, W):
    """(image, row, column) of the probes: corners, both ends of an inner row, both sides of every cut between groups of 32
    tiles that falls inside a tile row (first image), and the last pixel of the batch."""
    tx_n = W // 2
    at = {(0, 0, 0), (0, 0, W - 1), (0, H - 1, 0), (0, H - 1, W - 1), (0, 5, 0), (0, 5, W - 1), (N - 1, H - 1, W - 1)}
    for t in range(32, (H // 2) * tx_n, 32):
        ty, tx = divmod(t, tx_n)
        if tx:                                                       # tile t - 1 is the left neighbour of tile t
            at |= {(0, 2 * ty, 2 * tx - 1), (0, 2 * ty, 2 * tx), (0, 2 * ty + 1, 2 * tx - 1), (0, 2 * ty + 1, 2 * tx)}
    return sorted(at)


@pytest.mark.parametrize("flip", [0, 1], ids=["forward", "dgrad"])
@pytest.mark.parametrize("shape", [(169, 64, 14, 14, 256), (5, 64, 70, 48, 256), (1, 64, 128, 128, 256)],
                         ids=["14x14_n169", "70x48", "128x128"])
def test_one_hot_inputs_are_exact_with_either_staging(shape, flip):
    from feature_intertwiner_amd import _lib
    L = _lib.load()
    N, Cin, H, W, Cout = shape
    hot = _hot_pixels(N, H, W)
    if W == 128:
        assert (0, 0, 63) in hot and (0, 0, 64) in hot                # tile 32 starts the second half of a row
    if W == 48:
        assert (0, 2, 15) in hot and (0, 2, 16) in hot                # tile 32 = tile row 1, tile column 8
    x = torch.zeros(N, Cin, H, W, device=DEV)
    for k, (n, r, c) in enumerate(hot):
        x[n, 25, r, c] = 2.0 ** (k % 11)                              # channel 25: block 1, second channel of its thread
    g = torch.Generator(device=DEV).manual_seed(9900 + W)
    w = (torch.randint(-8, 9, (Cout, 3, 3, Cin), device=DEV, generator=g).float() / 4).contiguous()
    wl = w.permute(0, 3, 1, 2)
    ref = R.conv_ref(x, wl, (1, 1), (1, 1), tap_reversed=bool(flip))
    assert ref.abs().max() > 0
    layout = 2 if flip else 1
    form, key = ("WINO14", "conv3x3_patch_flat") if W == 14 else ("WINO", "conv3x3_patch")
    ys = []
    for staging, run in (("PAIR", lambda fn: fn()), ("SCALAR", _scalar)):
        y = _nan(N, Cout, H, W)
        args = (_lib.ptr(x), _lib.ptr(w), None, None, None, None, _lib.ptr(y), N, Cin, H, W, Cout, 3, 3, 1, 1, 1, 1, 0, layout,
                0, 0, 0)

        def launch():
            assert _lib.planned_kernel(L.fi_conv2d_forward_plan, *args) == key
            assert _planned(x, w, y, (N, Cin, H, W, Cout, layout)) == (form, staging)
            _lib.check(L.fi_conv2d_forward_live(*args, None, _lib.current_stream()), "fi_conv2d_forward_live")
            torch.cuda.synchronize()
        run(launch)
        bad = (y.double() != ref).nonzero()
        assert bad.numel() == 0, (staging, bad[:8].tolist())
        ys.append(y)
    assert torch.equal(ys[0], ys[1])
