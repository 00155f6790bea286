"""fi_roi16_pyramid_crop_forward_{bf16,f16} (include/fi_roi16.h, csrc/crop_roi16.hip): RoIAlign that reads 16-bit
channels-last maps, held BIT FOR BIT to fi_pyramid_crop_forward_nhwc on the widened maps -- the widening is exact and the
arithmetic is the fp32 kernel's, so no tolerance is involved: one differing element fails.  Both entry points are called
through ctypes on crops filled with NaN, so a row or an element the kernel does not write shows.

Cases (each for bf16 and fp16): depth 8 (one lane), 24, 256 and 264 (a last chunk of 8 channels behind a full one); maps of
1x1, 2x3, 7x5 and 16x16, one map (level NULL and given) and four; crops 7x7, 14x14, 1x1 (the double-precision midpoint), 3x5
and 14x15; 1, 3 and 300 boxes that cycle through inside / straddling / fully outside (extrapolation 0 and 0.25) / degenerate
(y1 == y2) / inverted / ending exactly on the last pixel / whole map; map values N(0, 1) rounded to the type (four-tap
results inexact in fp32) with +0, -0, the largest finite value and, for fp16, subnormals planted; rows with level 6 and 1
and with box_ind = batch and -1 (zeros), and a row with level -1 (still NaN).
One 3-box / 3x5 / 16x16 case is held to oracle.crop_and_resize_forward on the widened map as well; two runs are bit-equal;
permuted boxes give permuted rows; the Python wrapper counts its launches and refuses an enabled grad mode, mixed dtypes and
an fp32 map."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRECISIONS = {"bf16": torch.bfloat16, "fp16": torch.float16}
SUFFIX = {"bf16": "bf16", "fp16": "f16"}
SIZES4 = [(16, 16), (7, 5), (2, 3), (1, 1)]
P, I = ctypes.c_void_p, ctypes.c_int


def _maps(prec, depth, sizes, batch, seed):
    """Seeded 16-bit channels-last maps with the special values planted in the first elements of each."""
    dtype = PRECISIONS[prec]
    g = torch.Generator().manual_seed(seed)
    special = [0.0, -0.0, torch.finfo(dtype).max, 1.0, -1.0]
    if prec == "fp16":
        special += [2.0 ** -24, -3 * 2.0 ** -24, 1023 * 2.0 ** -24]            # subnormals of IEEE half
    out = []
    for h, w in sizes:
        m = torch.randn((batch, depth, h, w), generator=g).to(dtype).contiguous(memory_format=torch.channels_last)
        flat = m.permute(0, 2, 3, 1).reshape(-1)                                # the memory, in its own order
        assert flat.data_ptr() == m.data_ptr()
        k = min(len(special), flat.numel())
        flat[:k] = torch.tensor(special[:k], dtype=torch.float64).to(dtype)
        out.append(m.to(DEV))
    return out


def _boxes(n, seed):
    rs = np.random.RandomState(seed)
    rows = []
    for i in range(n):
        k = i % 8
        if k == 0:        # fully inside
            y1, x1 = rs.uniform(0.0, 0.6, 2)
            b = [y1, x1, y1 + rs.uniform(0.05, 0.4), x1 + rs.uniform(0.05, 0.4)]
        elif k == 1:      # partly outside
            y1, x1 = rs.uniform(-0.3, 0.9, 2)
            b = [y1, x1, y1 + rs.uniform(0.2, 0.6), x1 + rs.uniform(0.2, 0.6)]
        elif k == 2:      # fully outside
            b = [1.2, 1.3, 1.6, 1.7] if i % 16 == 2 else [-0.7, -0.6, -0.2, -0.1]
        elif k == 3:      # degenerate: y1 == y2
            y = rs.uniform(0, 1)
            b = [y, rs.uniform(0, 0.5), y, rs.uniform(0.5, 1.0)]
        elif k == 4:      # inverted
            y1, x1 = rs.uniform(0.4, 0.9, 2)
            b = [y1, x1, y1 - rs.uniform(0.1, 0.4), x1 - rs.uniform(0.1, 0.4)]
        elif k == 5:      # ends exactly on the last pixel
            b = [rs.uniform(0.0, 0.9), rs.uniform(0.0, 0.9), 1.0, 1.0]
        elif k == 6:      # the whole map
            b = [0.0, 0.0, 1.0, 1.0]
        else:
            b = list(rs.uniform(-0.1, 1.1, 4))
        rows.append(b)
    return torch.from_numpy(np.asarray(rows, np.float32))


def _rows(n, num_levels, batch, seed, with_level):
    """(box_ind, level, bad): the last five of eight or more rows are the ones without a source."""
    rs = np.random.RandomState(seed + 1)
    ind = rs.randint(0, batch, n).astype(np.int32)
    level = (2 + rs.randint(0, num_levels, n)).astype(np.int32)
    bad = {}
    if n >= 8 and with_level:
        level[n - 5], level[n - 4], level[n - 1] = 6 if num_levels == 4 else 2 + num_levels, 1, -1
        ind[n - 3], ind[n - 2] = batch, -1
        bad = {"zero": [n - 5, n - 4, n - 3, n - 2], "unwritten": [n - 1]}
    elif n >= 8:
        ind[n - 3], ind[n - 2] = batch, -1
        bad = {"zero": [n - 3, n - 2], "unwritten": []}
    return torch.from_numpy(ind), (torch.from_numpy(level) if with_level else None), bad


def _call(fn, what, maps, boxes, ind, level, batch, depth, ch, cw, extrap):
    from feature_intertwiner_amd import _lib
    nl = len(maps)
    crops = torch.full((boxes.shape[0], depth, ch, cw), float("nan"), device=DEV, dtype=torch.float32)
    rc = fn((P * nl)(*[m.data_ptr() for m in maps]), (I * nl)(*[m.shape[2] for m in maps]),
            (I * nl)(*[m.shape[3] for m in maps]), nl, _lib.ptr(boxes), _lib.ptr(ind), _lib.ptr(level), boxes.shape[0], batch,
            depth, ch, cw, float(extrap), _lib.ptr(crops), _lib.current_stream())
    _lib.check(rc, what)
    return crops


def _new(prec, maps, *args):
    from feature_intertwiner_amd import roi16
    fn = getattr(roi16.load(), "fi_roi16_pyramid_crop_forward_" + SUFFIX[prec])
    return _call(fn, "fi_roi16_pyramid_crop_forward", maps, *args)


def _ref(maps, *args):
    """fi_pyramid_crop_forward_nhwc on the widened maps, still channels-last."""
    from feature_intertwiner_amd import _lib
    wide = [m.float() for m in maps]
    for w, m in zip(wide, maps):
        assert w.is_contiguous(memory_format=torch.channels_last) and torch.equal(w.to(m.dtype).view(torch.int16),
                                                                                  m.view(torch.int16))
    return _call(_lib.load().fi_pyramid_crop_forward_nhwc, "fi_pyramid_crop_forward_nhwc", wide, *args)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


#        depth, sizes, with_level, (crop_h, crop_w), boxes, extrapolation
CASES = [
    (8, [(1, 1)], False, (1, 1), 3, 0.0),
    (8, [(2, 3)], True, (7, 7), 1, 0.0),
    (24, [(2, 3)], True, (3, 5), 3, 0.25),
    (24, [(7, 5)], False, (14, 14), 300, 0.25),
    (24, SIZES4, True, (14, 15), 3, 0.0),
    (256, [(16, 16)], False, (7, 7), 1, 0.0),
    (256, SIZES4, True, (7, 7), 300, 0.25),
    (256, SIZES4, True, (1, 1), 300, 0.0),
    (264, SIZES4, True, (14, 14), 300, 0.0),
    (264, [(16, 16)], True, (7, 7), 300, 0.25),
    (264, SIZES4, True, (3, 5), 3, 0.0),
]


@pytest.mark.parametrize("prec", sorted(PRECISIONS))
@pytest.mark.parametrize("case", range(len(CASES)))
def test_crops_are_bit_equal_to_the_fp32_kernel_on_the_widened_maps(prec, case):
    depth, sizes, with_level, (ch, cw), n, extrap = CASES[case]
    batch = 2
    maps = _maps(prec, depth, sizes, batch, seed=100 + case)
    boxes = _boxes(n, seed=200 + case).to(DEV)
    ind, level, bad = _rows(n, len(sizes), batch, 300 + case, with_level)
    ind, level = ind.to(DEV), (level.to(DEV) if level is not None else None)
    args = (boxes, ind, level, batch, depth, ch, cw, extrap)
    got = _new(prec, maps, *args)
    ref = _ref(maps, *args)
    torch.cuda.synchronize()
    assert _bits_equal(got, ref), "%d elements differ" % int((got.view(torch.int32) != ref.view(torch.int32)).sum())
    for r in bad.get("zero", []):
        assert not bool(got[r].any()) and not bool(torch.isnan(got[r]).any()), r
    for r in bad.get("unwritten", []):
        assert bool(torch.isnan(got[r]).all()), r
    live = [r for r in range(n) if r not in bad.get("unwritten", [])]
    assert not bool(torch.isnan(got[live]).any())             # every other element was written
    if n >= 8:
        assert float(got[live].abs().max()) > 0.1
        if extrap != 0.0:
            assert bool((got[live] == extrap).any())          # some bin fell outside its map
    assert _bits_equal(_new(prec, maps, *args), got)          # a second run


@pytest.mark.parametrize("prec", sorted(PRECISIONS))
def test_crops_are_bit_equal_to_the_oracle_on_the_widened_map(prec):
    from oracle import oracle as O
    maps = _maps(prec, 24, [(16, 16)], 2, seed=7)
    boxes = _boxes(3, seed=8)
    boxes[2] = torch.tensor([0.1, -0.2, 0.95, 1.0])           # inside, straddling and one ending on the last column
    ind = torch.tensor([1, 0, 1], dtype=torch.int32)
    got = _new(prec, maps, boxes.to(DEV), ind.to(DEV), None, 2, 24, 3, 5, 0.25).cpu().numpy()
    exp = O.crop_and_resize_forward(maps[0].float().contiguous().cpu().numpy(), boxes.numpy(), ind.numpy(), 3, 5, 0.25)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    assert np.abs(got).max() > 0.1


@pytest.mark.parametrize("prec", sorted(PRECISIONS))
def test_permuted_boxes_give_permuted_rows(prec):
    n, depth = 300, 256
    maps = _maps(prec, depth, SIZES4, 2, seed=11)
    boxes = _boxes(n, seed=12).to(DEV)
    ind, level, _ = _rows(n, 4, 2, 13, True)
    ind, level = ind.to(DEV), level.to(DEV)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(14)).to(DEV)
    a = _new(prec, maps, boxes, ind, level, 2, depth, 7, 7, 0.0)
    b = _new(prec, maps, boxes[perm].contiguous(), ind[perm].contiguous(), level[perm].contiguous(), 2, depth, 7, 7, 0.0)
    assert _bits_equal(a[perm], b)


def test_python_wrapper_counts_and_refuses():
    from feature_intertwiner_amd import _lib, roi16
    maps = _maps("bf16", 24, SIZES4, 2, seed=21)
    boxes = _boxes(16, seed=22).to(DEV)
    ind, level, _ = _rows(16, 4, 2, 23, True)
    ind, level = ind.to(DEV), level.to(DEV)
    roi16.reset_stats()
    with torch.no_grad():
        got = roi16.pyramid_crop16(maps, boxes, ind, level, 7, 7)
        assert roi16.stats() == {"crop": 1}
        assert got.dtype is torch.float32 and tuple(got.shape) == (16, 24, 7, 7) and got.is_contiguous()
        ref = _ref(maps, boxes, ind, level, 2, 24, 7, 7, 0.0)
        assert _bits_equal(got[:15], ref[:15])                # (row 15 has level -1: unwritten)
        one = roi16.pyramid_crop16(maps[:1], boxes, ind, None, 3, 5, extrapolation_value=0.25)      # level NULL, one map
        assert roi16.stats() == {"crop": 2}
        assert _bits_equal(one, _ref(maps[:1], boxes, ind, None, 2, 24, 3, 5, 0.25))
        empty = roi16.pyramid_crop16(maps, boxes[:0], ind[:0], level[:0], 7, 7)
        assert tuple(empty.shape) == (0, 24, 7, 7)
        mixed = [maps[0], maps[1].to(torch.float16)]
        with pytest.raises(_lib.FiError, match="share dtype"):
            roi16.pyramid_crop16(mixed, boxes, ind, level, 7, 7)
        with pytest.raises(_lib.FiError, match="bfloat16 / float16"):
            roi16.pyramid_crop16([m.float() for m in maps], boxes, ind, level, 7, 7)
        with pytest.raises(_lib.FiError, match="fi_roi16_crop_eligible"):
            roi16.pyramid_crop16(maps, boxes, ind, level, 15, 15)
        with pytest.raises(_lib.FiError, match="fi_roi16_crop_eligible"):
            roi16.pyramid_crop16(_maps("bf16", 12, [(4, 4)], 2, seed=24), boxes, ind, None, 7, 7)    # depth 12
    count = roi16.stats()["crop"]
    with torch.enable_grad():
        with pytest.raises(_lib.FiError, match="no_grad"):
            roi16.pyramid_crop16(maps, boxes, ind, level, 7, 7)
    assert roi16.stats()["crop"] == count
