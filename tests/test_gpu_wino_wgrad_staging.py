"""The staging of the Winograd F(2x2,3x3) weight gradient (csrc/conv3x3_wino_wgrad.hip): the two centre columns of a window
row through one 8-byte load, against the staging with 4-byte loads only that FI_WINO_WGRAD_SCALAR_STAGING=1 (read per call)
keeps reachable.  The values staged and every floating-point operation are the same, so a launch of ONE pixel split -- one
chain per accumulator, no atomics between workgroups -- must give dW and dbias bit for bit equal to the other staging, and
both within the float64 bar of tests/test_gpu_conv_wino_wgrad.py, 2^-24 (4 sqrt(n) + 16) m.  Outputs are NaN-filled before
each launch."""
import os

import pytest
import torch

import fp64_ref as R
from test_gpu_conv16_plan import _nan
from test_gpu_conv_wino_wgrad import _geom, _is_wino, _launch, _refs, _run

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SWITCH = "FI_WINO_WGRAD_SCALAR_STAGING"

# name -> (N, Cin, H, W, Cout), all of one pixel split
SINGLE = {
    "tx4": (1, 256, 8, 8, 256),                   # 4 tiles a row: every stage has both image edges
    "tx8": (1, 256, 4, 16, 256),                  # 8 tiles a row: stages at the left edge and at the right edge
    "one_tile_row": (1, 256, 2, 24, 256),         # TX = 12, a single tile row: top and bottom window rows both padded
    "cout320": (1, 256, 8, 8, 320),
    "cin512": (1, 512, 8, 8, 256),
    "w14": (1, 256, 6, 14, 256),                  # W % 8 != 0: 7 tiles a row, stages cut in mid-row
    "w12": (1, 256, 4, 12, 256),
}


def _scalar(fn):
    assert SWITCH not in os.environ
    os.environ[SWITCH] = "1"
    try:
        return fn()
    finally:
        del os.environ[SWITCH]


def _both(x, dy, shape, splits):
    """(dW, dbias) of the paired and of the scalar staging; the plan is the same launch for both."""
    N, Cin, H, W, Cout = shape
    out = []
    for scalar in (False, True):
        dw, db = _nan(Cout, 3, 3, Cin), _nan(Cout)
        p = _scalar(lambda: _launch(x, dy, dw, db, _geom(shape))) if scalar else _launch(x, dy, dw, db, _geom(shape))
        assert _is_wino(p) and p.splits == splits, (shape, p.splits)
        if scalar:
            _scalar(lambda: _run(x, dy, dw, db, _geom(shape)))
        else:
            _run(x, dy, dw, db, _geom(shape))
        out.append((dw, db))
    return out


@pytest.mark.parametrize("name", sorted(SINGLE))
def test_single_split_equals_the_scalar_staging_bit_for_bit(name):
    shape = SINGLE[name]
    N, Cin, H, W, Cout = shape
    g = torch.Generator(device=DEV).manual_seed(12000 + sorted(SINGLE).index(name))
    x = torch.randn(N, Cin, H, W, device=DEV, generator=g)
    dy = torch.randn(N, Cout, H, W, device=DEV, generator=g)
    (dw, db), (dws, dbs) = _both(x, dy, shape, 1)
    assert torch.equal(dw, dws), (name, (dw - dws).abs().max())
    assert torch.equal(db, dbs), name
    ref, mag, db_ref, db_mag = _refs(x, dy)
    worst = R.check_bar(dw, ref, mag, N * H * W, "%s dW" % name)
    worst_db = R.check_bar(db, db_ref, db_mag, N * H * W, "%s dbias" % name)
    print("%s %s: worst |d|/(2^-24 m) dW %.2f dbias %.2f, equal to the scalar staging" % (name, shape, worst, worst_db))


def test_several_splits_are_the_float64_reference():
    shape = (4, 256, 16, 16, 256)                 # 256 tiles: 8 splits of 32, added with atomics
    N, Cin, H, W, Cout = shape
    g = torch.Generator(device=DEV).manual_seed(12100)
    x = torch.randn(N, Cin, H, W, device=DEV, generator=g)
    dy = torch.randn(N, Cout, H, W, device=DEV, generator=g)
    ref, mag, db_ref, db_mag = _refs(x, dy)
    for which, (dw, db) in zip(("paired", "scalar"), _both(x, dy, shape, 8)):
        worst = R.check_bar(dw, ref, mag, N * H * W, "%s dW" % which)
        worst_db = R.check_bar(db, db_ref, db_mag, N * H * W, "%s dbias" % which)
        print("%s staging %s, 8 splits: worst |d|/(2^-24 m) dW %.2f dbias %.2f" % (which, shape, worst, worst_db))


def test_known_answers_at_the_edges_and_between_quads_are_exact():
    """x one-hot at a corner, a left-edge, a right-edge pixel and on either side of the boundary between the two stages of a
    tile row (columns 7 | 8 of a 16-wide map), one input channel each; for each of them and each of the nine taps an output
    channel whose dy is one-hot at the pixel that pairs with it through that tap.  Products of 1 and 1/2^n: dW must EQUAL the
    float64 reference with either staging."""
    shape = (1, 256, 8, 16, 256)
    N, Cin, H, W, Cout = shape
    x = torch.zeros(N, Cin, H, W, device=DEV)
    dy = torch.zeros(N, Cout, H, W, device=DEV)
    spots = ((0, 0), (3, 0), (4, 15), (2, 7), (5, 8), (7, 15))
    for ci, (py, px) in enumerate(spots):
        x[0, 41 * ci % Cin, py, px] = 0.5 ** ci
        for t in range(9):
            oy, ox = py - (t // 3 - 1), px - (t % 3 - 1)
            if 0 <= oy < H and 0 <= ox < W:
                dy[0, (9 * ci + t) * 3 % Cout, oy, ox] = 0.25 * (t + 1)
    ref = R.wgrad_ref(x, dy, 3, 3, (1, 1), (1, 1)).permute(0, 2, 3, 1)
    assert int((ref != 0).sum()) == 4 + 6 + 6 + 9 + 9 + 4
    for dw, db in _both(x, dy, shape, 1):
        assert torch.equal(dw.double(), ref), (dw.double() - ref).abs().max()
        assert torch.equal(db.double(), dy.double().sum((0, 2, 3)))
