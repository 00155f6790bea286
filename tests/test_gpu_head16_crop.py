"""fi_head16_pyramid_crop_forward_{bf16,f16} (include/fi_head16.h, csrc/head16_crop.hip): RoIAlign that reads 16-bit
channels-last maps and writes 16-bit channels-last crops, held BIT FOR BIT to roi16.pyramid_crop16(...).to(dtype) laid out
[n, h, w, C] -- the fp32 value is fi_roi16_pyramid_crop_forward's and the store rounds it once to nearest even, which is what
.to(dtype) does, so no tolerance is involved: one differing element fails.  Both entry points are called through ctypes on
crops filled with NaN and followed by a 64-element sentinel tail, so a row or an element the kernel does not write, and a
store past the end, show.

Cases (each for bf16 and fp16): maps of 2 x {16 x 16, 8 x 8, 5 x 3, 2 x 2}, all four or the first alone (level NULL); depth 8
(one lane per bin), 24 (3 lanes: 85 bin groups and an idle lane), 256 and 264 (33 lanes); crops 1 x 1 (the double-precision
midpoint), 7 x 7 (one slab), 14 x 14 (four slabs, the last of 4 bins) and 3 x 5; 1, 5 and 257 boxes that cycle through inside /
partly outside / wholly outside (extrapolation 0 and 2.5) / degenerate (y1 == y2) / whole map / random; rows with a level
outside the pyramid and with a box_ind outside the batch (zeros), and a row with level -1 (still NaN).  Two runs are
bit-equal; permuted boxes give permuted rows; the Python wrapper returns act16's logical [n, C, h, w] channels-last tensor
and counts its launches."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRECISIONS = {"bf16": torch.bfloat16, "fp16": torch.float16}
SUFFIX = {"bf16": "bf16", "fp16": "f16"}
SIZES4 = [(16, 16), (8, 8), (5, 3), (2, 2)]
P, I = ctypes.c_void_p, ctypes.c_int
TAIL, SENTINEL = 64, -7.0


def _maps(prec, depth, sizes, batch, seed):
    dtype = PRECISIONS[prec]
    g = torch.Generator().manual_seed(seed)
    return [torch.randn((batch, depth, h, w), generator=g).to(dtype).contiguous(memory_format=torch.channels_last).to(DEV)
            for h, w in sizes]


def _boxes(n, seed):
    rs = np.random.RandomState(seed)
    rows = []
    for i in range(n):
        k = i % 6
        if k == 0:        # inside
            y1, x1 = rs.uniform(0.0, 0.6, 2)
            b = [y1, x1, y1 + rs.uniform(0.05, 0.4), x1 + rs.uniform(0.05, 0.4)]
        elif k == 1:      # partly outside
            y1, x1 = rs.uniform(-0.3, 0.9, 2)
            b = [y1, x1, y1 + rs.uniform(0.2, 0.6), x1 + rs.uniform(0.2, 0.6)]
        elif k == 2:      # wholly outside
            b = [1.2, 1.3, 1.6, 1.7] if i % 12 == 2 else [-0.7, -0.6, -0.2, -0.1]
        elif k == 3:      # degenerate: y1 == y2
            y = rs.uniform(0, 1)
            b = [y, rs.uniform(0, 0.5), y, rs.uniform(0.5, 1.0)]
        elif k == 4:      # the whole map
            b = [0.0, 0.0, 1.0, 1.0]
        else:
            b = list(rs.uniform(-0.1, 1.1, 4))
        rows.append(b)
    return torch.from_numpy(np.asarray(rows, np.float32))


def _rows(n, num_levels, batch, seed, with_level):
    """(box_ind, level, bad): with five or more boxes the last rows are the ones without a source."""
    rs = np.random.RandomState(seed + 1)
    ind = rs.randint(0, batch, n).astype(np.int32)
    level = (2 + rs.randint(0, num_levels, n)).astype(np.int32)
    bad = {"zero": [], "unwritten": []}
    if n >= 5 and with_level:
        level[n - 3], ind[n - 2], level[n - 1] = 2 + num_levels, batch, -1
        bad = {"zero": [n - 3, n - 2], "unwritten": [n - 1]}
        if n >= 8:
            level[n - 5], ind[n - 4] = 1, -1
            bad["zero"] += [n - 5, n - 4]
    elif n >= 5:
        ind[n - 2] = batch
        bad["zero"] = [n - 2]
    return torch.from_numpy(ind), (torch.from_numpy(level) if with_level else None), bad


def _new(prec, maps, boxes, ind, level, batch, depth, ch, cw, extrap):
    """The raw entry point on NaN-filled crops with a sentinel tail: int16 bit patterns [n, ch, cw, depth]."""
    from feature_intertwiner_amd import _lib, head16
    fn = getattr(head16.load(), "fi_head16_pyramid_crop_forward_" + SUFFIX[prec])
    nl, n = len(maps), boxes.shape[0]
    buf = torch.full((n * ch * cw * depth + TAIL,), float("nan"), device=DEV, dtype=PRECISIONS[prec])
    buf[-TAIL:] = SENTINEL
    rc = fn((P * nl)(*[m.data_ptr() for m in maps]), (I * nl)(*[m.shape[2] for m in maps]),
            (I * nl)(*[m.shape[3] for m in maps]), nl, _lib.ptr(boxes), _lib.ptr(ind), _lib.ptr(level), n, batch,
            depth, ch, cw, float(extrap), _lib.ptr(buf), _lib.current_stream())
    _lib.check(rc, "fi_head16_pyramid_crop_forward")
    torch.cuda.synchronize()
    assert bool((buf[-TAIL:] == SENTINEL).all()), "the sentinel tail was written"
    return buf[:-TAIL].view(n, ch, cw, depth)


def _ref(prec, maps, boxes, ind, level, ch, cw, extrap):
    """roi16.pyramid_crop16(...).to(dtype) permuted to [n, h, w, C]."""
    from feature_intertwiner_amd import roi16
    with torch.no_grad():
        wide = roi16.pyramid_crop16(maps, boxes, ind, level, ch, cw, extrapolation_value=extrap)
    assert wide.dtype is torch.float32
    return wide.to(PRECISIONS[prec]).permute(0, 2, 3, 1).contiguous()


def _bits(t):
    return t.contiguous().view(torch.int16)


#        depth, sizes, with_level, (crop_h, crop_w), boxes, extrapolation
CASES = [
    (8, SIZES4[:1], False, (1, 1), 1, 0.0),
    (8, SIZES4, True, (7, 7), 5, 2.5),
    (24, SIZES4[:1], False, (3, 5), 5, 2.5),
    (24, SIZES4, True, (14, 14), 257, 0.0),
    (24, SIZES4, True, (1, 1), 257, 2.5),
    (256, SIZES4, True, (7, 7), 257, 2.5),
    (256, SIZES4, True, (14, 14), 5, 0.0),
    (256, SIZES4[:1], False, (7, 7), 1, 0.0),
    (264, SIZES4, True, (14, 14), 257, 2.5),
    (264, SIZES4, True, (3, 5), 257, 0.0),
    (264, SIZES4[:1], True, (7, 7), 5, 0.0),
]


@pytest.mark.parametrize("prec", sorted(PRECISIONS))
@pytest.mark.parametrize("case", range(len(CASES)))
def test_crops_are_the_fp32_crops_rounded_once(prec, case):
    depth, sizes, with_level, (ch, cw), n, extrap = CASES[case]
    batch = 2
    maps = _maps(prec, depth, sizes, batch, seed=100 + case)
    boxes = _boxes(n, seed=200 + case).to(DEV)
    ind, level, bad = _rows(n, len(sizes), batch, 300 + case, with_level)
    ind, level = ind.to(DEV), (level.to(DEV) if level is not None else None)
    got = _new(prec, maps, boxes, ind, level, batch, depth, ch, cw, extrap)
    ref = _ref(prec, maps, boxes, ind, level, ch, cw, extrap)
    live = [r for r in range(n) if r not in bad["unwritten"]]
    assert got.shape == ref.shape
    diff = int((_bits(got[live]) != _bits(ref[live])).sum())
    assert diff == 0, "%d elements differ" % diff
    for r in bad["zero"]:
        assert bool((_bits(got[r]) == 0).all()), r
    for r in bad["unwritten"]:
        assert bool(torch.isnan(got[r]).all()), r
    assert not bool(torch.isnan(got[live]).any())             # every other element was written
    if n >= 8:
        assert float(got[live].float().abs().max()) > 0.1
        if extrap != 0.0:
            assert bool((got[live].float() == extrap).any())  # some bin fell outside its map
    again = _new(prec, maps, boxes, ind, level, batch, depth, ch, cw, extrap)
    assert torch.equal(_bits(again), _bits(got))              # a second run (NaN rows compare as bit patterns)


@pytest.mark.parametrize("prec", sorted(PRECISIONS))
def test_permuted_boxes_give_permuted_rows(prec):
    n, depth = 257, 256
    maps = _maps(prec, depth, SIZES4, 2, seed=11)
    boxes = _boxes(n, seed=12).to(DEV)
    ind, level, _ = _rows(n, 4, 2, 13, True)
    ind, level = ind.to(DEV), level.to(DEV)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(14)).to(DEV)
    a = _new(prec, maps, boxes, ind, level, 2, depth, 7, 7, 0.0)
    b = _new(prec, maps, boxes[perm].contiguous(), ind[perm].contiguous(), level[perm].contiguous(), 2, depth, 7, 7, 0.0)
    assert torch.equal(_bits(a[perm]), _bits(b))


def test_python_wrapper_returns_a_channels_last_tensor_and_counts():
    from feature_intertwiner_amd import _lib, head16, roi16
    maps = _maps("bf16", 24, SIZES4, 2, seed=21)
    boxes = _boxes(16, seed=22).to(DEV)
    ind, level, bad = _rows(16, 4, 2, 23, True)
    ind, level = ind.to(DEV), level.to(DEV)
    head16.reset_stats()
    roi16.reset_stats()
    with torch.no_grad():
        got = head16.pyramid_crop16_cl(maps, boxes, ind, level, 7, 7)
        assert head16.stats() == {"crop": 1, "conv": 0, "out": 0, "weights": 0} and roi16.stats() == {"crop": 0}
        assert got.dtype is torch.bfloat16 and tuple(got.shape) == (16, 24, 7, 7)
        assert got.is_contiguous(memory_format=torch.channels_last)
        ref = _ref("bf16", maps, boxes, ind, level, 7, 7, 0.0)
        assert torch.equal(_bits(got.permute(0, 2, 3, 1)[:15]), _bits(ref[:15]))      # (row 15 has level -1: unwritten)
        one = head16.pyramid_crop16_cl(maps[:1], boxes, ind.clamp(0, 1), None, 3, 5, extrapolation_value=2.5)
        assert torch.equal(_bits(one.permute(0, 2, 3, 1)), _bits(_ref("bf16", maps[:1], boxes, ind.clamp(0, 1), None, 3, 5, 2.5)))
        empty = head16.pyramid_crop16_cl(maps, boxes[:0], ind[:0], level[:0], 7, 7)
        assert tuple(empty.shape) == (0, 24, 7, 7)
        with pytest.raises(_lib.FiError, match="share dtype"):
            head16.pyramid_crop16_cl([maps[0], maps[1].to(torch.float16)], boxes, ind, level, 7, 7)
        with pytest.raises(_lib.FiError, match="fi_head16_crop_eligible"):
            head16.pyramid_crop16_cl(maps, boxes, ind, level, 7, 65)
        with pytest.raises(_lib.FiError, match="fi_head16_crop_eligible"):
            head16.pyramid_crop16_cl(_maps("bf16", 12, [(4, 4)], 2, seed=24), boxes, ind, None, 7, 7)      # depth 12
    assert head16.stats()["crop"] == 3              # the refused calls were not counted (the empty one was)
