"""The Winograd F(2x2,3x3) weight gradient (csrc/conv3x3_wino_wgrad.hip) held to float64, element by element, at the
smallest shapes at which each piece of the kernel can go wrong, in the manner of
tests/test_gpu_conv32_edges.py::test_weight_gradient_is_the_float64_reference_on_every_launch_branch: the plan is asked
first (a shape that stops reaching the kernel fails there), the launch writes dW and dbias into NaN-filled outputs, then
under FI_OUTPUTS_ZEROED into a dW that already holds values; every element is within the bar of tests/fp64_ref.py,
2^-24 (4 sqrt(n) + 16) m with n the pixels and m the DIRECT form's magnitude.  The direct kernel's worst error on the
same operands (FI_NO_WINOGRAD_WGRAD=1) is printed next to it.  tests/test_wino_wgrad_plan.py holds the rule on the host.

The kernel takes no batch, and its rule wants Cout in whole blocks of 64: a batch and Cout 288 are neighbours here.

Measured worst |d| in units of 2^-24 m (fixed seeds): 1.2-7.8 from 12 tiles up, where the direct kernel reads 2.1-6.2 -- but
24.4 on `smallest_map` (4 tiles, bar 32; direct 3.8): with a single stage the transform-domain terms of an element do not
average out, and a CPU emulation over 8 random (cout, cin) pairs had predicted 3.7 where the worst of 589 824 elements is
6 x that.  The bar is not widened for it: a change of the accumulation or transform order that costs another third on
this case fails here, and should."""
import functools
import os

import pytest
import torch

import fp64_ref as R
from test_gpu_conv16_plan import _nan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SWITCH = "FI_NO_WINOGRAD_WGRAD"

# name -> (N, Cin, H, W, Cout); tiles are 2 x 2 pixels, a stage 4 tiles, a split whole stages and at least 32 tiles
CASES = {
    "smallest_map": (1, 256, 4, 4, 256),          # 4 tiles: one stage, one split
    "h_ne_w": (2, 256, 6, 4, 256),                # 3 x 2 tiles per image: 12 tiles, stages cut across rows and the image
    # 9 tiles per image: 261 tiles in 9 splits of 32 -- stages and splits cut in mid-row and across images; the last split
    # has 5 tiles, its last stage 1
    "nine_tiles": (29, 256, 6, 6, 256),
    "roi_map": (3, 256, 14, 14, 256),             # 147 tiles: 5 splits of 32, the last 19 (its last stage 3)
    "row_uniform": (1, 256, 16, 16, 256),         # the direct kernel's row-uniform neighbour: 64 tiles, 2 splits
    "cin512": (1, 512, 8, 8, 256),                # 8 Cin blocks
    "cout512": (1, 256, 8, 8, 512),               # 8 Cout blocks
    "cout320": (2, 256, 6, 6, 320),               # 5 Cout blocks (the last 128-row tile of the direct kernel is half empty)
    "full_splits": (4, 256, 16, 16, 256),         # 256 tiles: 8 splits of 32, all full -- the atomic accumulation
}
# (splits, tiles per split, tiles) the split query must answer
SPLITS = {"smallest_map": (1, 4, 4), "h_ne_w": (1, 12, 12), "nine_tiles": (9, 32, 261), "roi_map": (5, 32, 147),
          "row_uniform": (2, 32, 64), "cin512": (1, 16, 16), "cout512": (1, 16, 16), "cout320": (1, 20, 18),
          "full_splits": (8, 32, 256)}


def _geom(shape, k=3, st=1, pd=1):
    N, Cin, H, W, Cout = shape
    return (N, Cin, H, W, Cout, k, k, st, st, pd, pd)


def _with_switch(fn):
    assert SWITCH not in os.environ
    os.environ[SWITCH] = "1"
    try:
        return fn()
    finally:
        del os.environ[SWITCH]


def _launch(x, dy, dw, db, geom, flags=0, n=1):
    from feature_intertwiner_amd import _lib
    (p,) = _lib.planned_launches(_lib.load().fi_conv2d_weight_grad_launch, _lib.ptr(x), _lib.ptr(dy), _lib.ptr(dw), *geom, 1,
                                 _lib.ptr(db), flags, n)
    return p


def _is_wino(p):
    from feature_intertwiner_amd import _lib
    return bool(p.flags & _lib.LAUNCH_FLAGS["winograd"])


def _run(x, dy, dw, db, geom, flags=0):
    from feature_intertwiner_amd import _lib
    _lib.check(_lib.load().fi_conv2d_weight_grad(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(dw), *geom, 1, _lib.ptr(db), flags,
                                                 _lib.current_stream()), "fi_conv2d_weight_grad")
    torch.cuda.synchronize()


def _refs(x, dy, k=3, st=1, pd=1):
    """float64 dW and its m in the stored tap-major layout [Cout, R, S, Cin], dbias and its m."""
    ref = R.wgrad_ref(x, dy, k, k, (st, st), (pd, pd)).permute(0, 2, 3, 1)
    mag = R.wgrad_ref(x.abs(), dy.abs(), k, k, (st, st), (pd, pd)).permute(0, 2, 3, 1)
    return ref, mag, dy.double().sum((0, 2, 3)), dy.double().abs().sum((0, 2, 3))


@functools.lru_cache(maxsize=None)
def _problem(name):
    N, Cin, H, W, Cout = CASES[name]
    g = torch.Generator(device=DEV).manual_seed(7000 + sorted(CASES).index(name))
    x = torch.randn(N, Cin, H, W, device=DEV, generator=g)
    dy = torch.randn(N, Cout, H, W, device=DEV, generator=g)
    return (x, dy) + _refs(x, dy)


@pytest.mark.parametrize("name", sorted(CASES))
def test_winograd_weight_gradient_is_the_float64_reference(name):
    from feature_intertwiner_amd import _lib
    shape = CASES[name]
    N, Cin, H, W, Cout = shape
    geom, pixels = _geom(shape), N * H * W
    x, dy, ref, mag, db_ref, db_mag = _problem(name)

    dw, db = _nan(Cout, 3, 3, Cin), _nan(Cout)
    p = _launch(x, dy, dw, db, geom)
    assert _is_wino(p) and _lib.WGRAD_FORMS[p.form] == "VEC", name
    key = _lib.KERNEL_KEYS[p.kernel_id]
    assert key in ("conv_wgrad_bm64_3x3", "conv_wgrad_bm128_3x3")
    splits, tps, tiles = SPLITS[name]
    assert (p.splits, p.pixels_per_split) == (splits, 4 * tps) and tiles == N * (H // 2) * (W // 2), (name, p.splits, p.pixels_per_split)
    assert (splits - 1) * tps < tiles <= splits * tps
    if name == "nine_tiles":          # the last split and the last stage are both partly filled
        assert tiles - (splits - 1) * tps < tps and (tiles - (splits - 1) * tps) % 4 != 0 and splits > 1
    _run(x, dy, dw, db, geom)
    worst = R.check_bar(dw, ref, mag, pixels, "%s dW" % name)
    worst_db = R.check_bar(db, db_ref, db_mag, pixels, "%s dbias" % name)

    g = torch.Generator(device=DEV).manual_seed(8000 + sorted(CASES).index(name))
    before = torch.randn((Cout, 3, 3, Cin), device=DEV, generator=g) * float(pixels) ** 0.5      # the size of the increment
    dw = before.clone()
    assert _is_wino(_launch(x, dy, dw, None, geom, _lib.OUTPUTS_ZEROED))
    _run(x, dy, dw, None, geom, _lib.OUTPUTS_ZEROED)
    worst_inc = R.check_increment(dw, before, ref, mag, pixels, "%s dW increment" % name)

    dwd, dbd = _nan(Cout, 3, 3, Cin), _nan(Cout)
    assert not _with_switch(lambda: _is_wino(_launch(x, dy, dwd, dbd, geom)))
    _with_switch(lambda: _run(x, dy, dwd, dbd, geom))
    direct = R.check_bar(dwd, ref, mag, pixels, "%s dW, direct form" % name)
    print("%s %s: %s, %d splits of %d tiles (of %d), worst |d|/(2^-24 m) dW %.2f (direct form %.2f) dbias %.2f increment %.2f" % (
        name, shape, key, splits, tps, tiles, worst, direct, worst_db, worst_inc))


def test_known_answers_are_exact():
    """x one-hot at a map corner, an edge and an interior pixel (one input channel each); for every one of them and each of
    the nine taps an output channel whose dy is one-hot at the pixel that pairs with it through that tap (none where that
    pixel is outside the map).  Every value is a product of 1 and 1/2^n: dW must EQUAL the float64 reference -- a wrong
    window origin, tap order or halo selection changes it."""
    shape = (1, 256, 8, 8, 256)
    N, Cin, H, W, Cout = shape
    x = torch.zeros(N, Cin, H, W, device=DEV)
    dy = torch.zeros(N, Cout, H, W, device=DEV)
    spots = ((0, 0), (0, 3), (5, 2), (7, 7), (4, 7))          # corner, top edge, interior, far corner, right edge
    for ci, (py, px) in enumerate(spots):
        x[0, 70 * ci % Cin, py, px] = 0.5 ** ci
        for t in range(9):
            oy, ox = py - (t // 3 - 1), px - (t % 3 - 1)          # dW[co][r][s][ci] = sum dy[oy][ox] x[oy + r - 1][ox + s - 1]
            if 0 <= oy < H and 0 <= ox < W:
                dy[0, (9 * ci + t) * 5 % Cout, oy, ox] = 0.25 * (t + 1)
    ref = R.wgrad_ref(x, dy, 3, 3, (1, 1), (1, 1)).permute(0, 2, 3, 1)
    assert int((ref != 0).sum()) == 4 + 6 + 9 + 4 + 6
    dw, db = _nan(Cout, 3, 3, Cin), _nan(Cout)
    assert _is_wino(_launch(x, dy, dw, db, _geom(shape)))
    _run(x, dy, dw, db, _geom(shape))
    assert torch.equal(dw.double(), ref), (dw.double() - ref).abs().max()
    assert torch.equal(db.double(), dy.double().sum((0, 2, 3)))


# name -> (N, Cin, H, W, Cout, window, stride, pad, byte offset of x): each fails one condition of the rule; one pixel split
NEIGHBOURS = {
    "odd_h": (2, 256, 3, 4, 256, 3, 1, 1, 0),
    "odd_w": (2, 256, 4, 5, 256, 3, 1, 1, 0),
    "cin128": (2, 128, 6, 6, 256, 3, 1, 1, 0),
    "stride2": (2, 256, 8, 8, 256, 3, 2, 1, 0),
    "x_offset4": (2, 256, 6, 6, 256, 3, 1, 1, 4),
    "cout288": (2, 256, 6, 6, 288, 3, 1, 1, 0),
}


@pytest.mark.parametrize("name", sorted(NEIGHBOURS))
def test_neighbours_keep_their_kernel(name):
    """A shape beside the rule plans no Winograd launch and computes bit for bit what it computes with the form switched
    off (a single pixel split: the direct kernels' own results repeat, which is checked first)."""
    N, Cin, H, W, Cout, k, st, pd, off = NEIGHBOURS[name]
    geom = _geom((N, Cin, H, W, Cout), k, st, pd)
    OH, OW = R.out_size(H, W, k, k, (st, st), (pd, pd))
    g = torch.Generator(device=DEV).manual_seed(9000 + sorted(NEIGHBOURS).index(name))
    xs = torch.randn(N * Cin * H * W + 4, device=DEV, generator=g)
    x = xs[off // 4:off // 4 + N * Cin * H * W].view(N, Cin, H, W)
    assert x.data_ptr() % 16 == off
    dy = torch.randn(N, Cout, OH, OW, device=DEV, generator=g)
    outs = []
    for switched in (False, False, True):
        dw, db = _nan(Cout, 3, 3, Cin), _nan(Cout)
        p = _with_switch(lambda: _launch(x, dy, dw, db, geom)) if switched else _launch(x, dy, dw, db, geom)
        assert not _is_wino(p) and p.splits == 1, name
        if switched:
            _with_switch(lambda: _run(x, dy, dw, db, geom))
        else:
            _run(x, dy, dw, db, geom)
        outs.append((dw, db))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "the direct form does not repeat"
    assert torch.equal(outs[0][0], outs[2][0]) and torch.equal(outs[0][1], outs[2][1]), name
    ref, mag, db_ref, db_mag = _refs(x, dy, k, st, pd)
    R.check_bar(outs[0][0], ref, mag, N * OH * OW, "%s dW" % name)


def test_a_batch_stays_on_the_direct_kernel():
    from feature_intertwiner_amd import _lib
    shape = (2, 256, 8, 8, 256)
    x, dy = torch.zeros(shape[:4], device=DEV), torch.zeros(2, 256, 8, 8, device=DEV)
    dw = torch.zeros(256, 3, 3, 256, device=DEV)
    p = _launch(x, dy, dw, None, _geom(shape), _lib.OUTPUTS_ZEROED, n=3)
    assert p.per_launch == 3 and not _is_wino(p)
    assert _is_wino(_launch(x, dy, dw, None, _geom(shape), _lib.OUTPUTS_ZEROED, n=1))


def test_the_new_form_runs_in_the_slot_of_the_direct_kernel():
    """With and without the switch: the same kernel key, one launch counted each time, both within the bar -- and dW
    differing in at least one bit, so the two runs were not the same kernel."""
    from feature_intertwiner_amd import _lib
    name = "roi_map"
    shape = CASES[name]
    N, Cin, H, W, Cout = shape
    geom = _geom(shape)
    x, dy, ref, mag, db_ref, db_mag = _problem(name)
    got = {}
    for switched in (False, True):
        dw, db = _nan(Cout, 3, 3, Cin), _nan(Cout)

        def go():
            key = _lib.KERNEL_KEYS[_launch(x, dy, dw, db, geom).kernel_id]
            _lib.prof_reset()
            _lib.prof_enable(True)
            try:
                _run(x, dy, dw, db, geom)
            finally:
                _lib.prof_enable(False)
            return key, _lib.prof_get(key)[0]
        key, count = _with_switch(go) if switched else go()
        assert count == 1, (switched, key, count)
        R.check_bar(dw, ref, mag, N * H * W, "dW, switch %s" % switched)
        R.check_bar(db, db_ref, db_mag, N * H * W, "dbias, switch %s" % switched)
        got[switched] = (key, dw)
    assert got[False][0] == got[True][0]
    assert not torch.equal(got[False][1], got[True][1])
