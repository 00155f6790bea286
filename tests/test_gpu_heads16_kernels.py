"""libfi_heads16.so on the GPU, bf16 and fp16: RoIAlign's backward from 16-bit channels-last crop gradients and the backward of
the mask head's class-selected output layer.

Crop backward.  Maps 2 x C x {16x16, 8x8, 4x4, 2x2} (levels 2..5), crops 1x1, 7x7, 14x14 and 3x5, C = 8, 72 and 264 (one lane
per bin, 9 lanes per bin and bins that straddle a wavefront's 64 values, and 33 lanes per bin: more than one pass of the
workgroup).  The boxes, by name in _boxes(): random boxes inside the map on every level; boxes partly and wholly outside
(invalid taps); the whole map (0, 0, 1, 1) on every level and its corners as zero-size boxes (integer coordinates:
floor == ceil); zero-size boxes inside; 64 identical small boxes on one cell of one image (contention); rows with level -1,
level 1 and 6 and box_ind -1 and 2, whose gradient rows are NaN: they must add nothing.
  - accumulate = 0 into buffers full of NaN: fp64_ref.check_crop_bwd on the widened, permuted gradient with that helper's
    bar (the kernel adds with atomics: no bitwise claim), and every cell no tap reaches is exactly zero;
  - accumulate = 1 into pre-filled buffers: fp64_ref.check_increment on the difference, and the cells no tap reaches keep
    their bits.  The pre-fill is what an accumulating launch meets in a step -- ANOTHER gradient's backward over the same
    boxes -- plus 2^-6 noise on every cell: check_increment widens the bar by ONE rounding of |before| + |after|, while a
    cell that n atomics reach rounds its running sum n times, so the helper's bar is the right one only where |before| is
    of the size of the increment's own m, as it is here (the 64-fold contended cell included);
  - no boxes: accumulate = 0 clears, accumulate = 1 leaves every bit;
  - depth 12 and a gradient 2 bytes off 16: FI_ERR_UNSUPPORTED from the entry point, the buffers keep their bits.
Adjoint.  <head16.pyramid_crop16_cl(x), d> against <x, crop_backward16(d)> in float64, x and d 16-bit values.  The forward
rounds each crop value once to 16 bits behind an fp32 interpolation of at most 8 roundings of values below 2 max|x|; the
backward carries check_crop_bwd's bar.  So
    |lhs - rhs| <= sum |d| (u16 |y| + s16 + 16 2^-24 max|x|) + sum |x| 2^-24 (4 sqrt(n) + 16) m
with u16 = UNIT, s16 = the fp16 subnormal floor, (m, n) the backward reference's magnitudes and tap counts.
Class rows.  du, colsum, dweight and dbias against fp64_ref.class_row_bwd_ref on the widened operands, the RoI's
(a, b, pixel) rows as that reference's pixels.  du is one 16-bit rounding of one fp32 product:
    |du - ref| <= 2^-24 |ref| + u16 (1 + 2^-24) |ref| + s16,   exactly 0 where u <= 0 (u holds +0 and -0.0);
each sum is held to B(count, sum |terms|) = 2^-24 (4 sqrt(count) + 16) sum |terms| through fp64_ref.check_bar, the
accumulated ones through check_increment (pre-fills of a quarter of the terms' size, so that the one rounding per RoI of a
class's running sum stays inside the helper's 2^-23 (|before| + |after|)); rows of classes without a RoI keep their bits.
The sums are fp32 atomics (the header says so): the test prints whether two runs agreed bitwise and asserts nothing on it;
du must agree bitwise."""
import ctypes

import numpy as np
import pytest
import torch

import fp64_ref as R
from test_gpu_grad16_layer import CL, DEV, DTYPES, SUBNORMAL, UNIT, _B, _held

pytestmark = pytest.mark.gpu
SIZES = (16, 8, 4, 2)
BATCH = 2
_ids = lambda s: "x".join(map(str, s))


def _boxes(seed=3):
    """(boxes [n, 4] fp32, box_ind [n] int32, level [n] int32, dead [n] bool: rows that must add nothing)."""
    rs = np.random.RandomState(seed)
    rows = []                                                     # (y1, x1, y2, x2, image, level)
    for lvl in (2, 3, 4, 5):
        for _ in range(5):                                        # inside the map
            y1, x1 = rs.uniform(0.0, 0.6, 2)
            rows.append((y1, x1, y1 + rs.uniform(0.05, 0.39), x1 + rs.uniform(0.05, 0.39), rs.randint(0, BATCH), lvl))
        rows.append((0.0, 0.0, 1.0, 1.0, 0, lvl))                 # the whole map: integer coordinates at its ends
        rows.append((0.0, 0.0, 0.0, 0.0, 1, lvl))                 # zero-size boxes on two corners: integer coordinates
        rows.append((1.0, 1.0, 1.0, 1.0, 0, lvl))
        rows.append((0.37, 0.52, 0.37, 0.52, 1, lvl))             # a zero-size box inside
        rows.append((-0.3, 0.2, 0.6, 1.4, 0, lvl))                # partly outside
        rows.append((0.5, -0.5, 1.5, 0.5, 1, lvl))
    rows.append((1.5, 1.5, 2.0, 2.0, 0, 2))                       # wholly outside
    rows.append((-2.0, -2.0, -1.0, -1.0, 1, 3))
    rows.append((0.2, 1.2, 0.8, 1.9, 0, 4))                       # one axis wholly outside
    rows += [(0.40, 0.41, 0.43, 0.44, 1, 3)] * 64                 # contention: 64 identical boxes on one cell
    live = len(rows)
    rows += [(0.1, 0.1, 0.9, 0.9, 0, -1), (0.1, 0.1, 0.9, 0.9, 1, -1),          # level -1
             (0.1, 0.1, 0.9, 0.9, 0, 1), (0.1, 0.1, 0.9, 0.9, 0, 6),            # a level out of range
             (0.1, 0.1, 0.9, 0.9, -1, 2), (0.1, 0.1, 0.9, 0.9, BATCH, 3)]       # a box_ind out of range
    order = rs.permutation(len(rows))                             # the dead rows sit among the others
    a = np.asarray(rows, np.float64)[order]
    dead = torch.from_numpy(order >= live)
    return (torch.from_numpy(a[:, :4].astype(np.float32)).to(DEV), torch.from_numpy(a[:, 4].astype(np.int32)).to(DEV),
            torch.from_numpy(a[:, 5].astype(np.int32)).to(DEV), dead.to(DEV))


def _bufs(C, fill, gen=None):
    out = []
    for s in SIZES:
        if fill == "nan":
            t = torch.full((BATCH, C, s, s), float("nan"))
        else:
            t = 0.5 * torch.randn((BATCH, C, s, s), generator=gen)
        out.append(t.to(DEV).contiguous(memory_format=CL))
    return out


def _grads(n, C, ch, cw, dtype, dead, seed):
    """(g16 logical [n, C, ch, cw] in channels-last memory, its exact fp32 NCHW widening with the dead rows zeroed)."""
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn((n, C, ch, cw), generator=gen).to(dtype).to(DEV).contiguous(memory_format=CL)
    wide = g.float().contiguous()
    g[dead] = float("nan")
    wide[dead] = 0.0
    return g, wide


@pytest.fixture
def rect_taps(monkeypatch):
    """fp64_ref.crop_bwd_ref asks the oracle for square crops; this makes it ask for ch x cw."""
    from oracle import oracle as O
    orig = O.crop_taps

    def use(ch, cw):
        monkeypatch.setattr(O, "crop_taps", lambda boxes, H, W, a, b: orig(boxes, H, W, ch, cw))
    return use


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("C", [8, 72, 264])
@pytest.mark.parametrize("crop", [(1, 1), (7, 7), (14, 14), (3, 5)], ids=_ids)
def test_crop_backward_clears_adds_and_accumulates(crop, C, sfx, rect_taps):
    from feature_intertwiner_amd import heads16
    ch, cw = crop
    rect_taps(ch, cw)
    boxes, ind, level, dead = _boxes()
    n = boxes.shape[0]
    g16, wide = _grads(n, C, ch, cw, DTYPES[sfx], dead, 17 + C + ch)
    what = "crop backward %dx%d C %d %s" % (ch, cw, C, sfx)
    heads16.reset_stats()

    bufs = _bufs(C, "nan")
    out = heads16.crop_backward16(g16, bufs, boxes, ind, level, crop, accumulate=False)
    torch.cuda.synchronize()
    assert all(o is b for o, b in zip(out, bufs)) and all(bool(torch.isfinite(b).all()) for b in bufs), what
    worst = R.check_crop_bwd(bufs, wide, boxes, ind, level, ch, what=what)
    refs, mags, cnts = R.crop_bwd_ref(wide, boxes, ind, level, [tuple(b.shape) for b in bufs], ch)
    print("%s: worst |d| / (2^-24 m) = %.3f" % (what, worst))
    for b, cnt in zip(bufs, cnts):
        untouched = (cnt == 0).expand_as(b)
        assert bool((b[untouched] == 0).all()), what + ": a cell no tap reaches is not zero"
    assert float(cnts[1].max()) >= 64 and bool((cnts[0] == 0).any())           # the contended cell; an unreached one
    assert any(bool((r != 0).any()) for r in refs)

    # the pre-fill: another gradient's backward (what an accumulating launch meets in a step) plus 2^-6 noise on every cell
    other, _ = _grads(n, C, ch, cw, DTYPES[sfx], dead, 91 + C + cw)
    gen = torch.Generator().manual_seed(5)
    before = _bufs(C, "nan")
    heads16.crop_backward16(other, before, boxes, ind, level, crop, accumulate=False)
    for b in before:
        b += 2.0 ** -6 * torch.randn(tuple(b.shape), generator=gen).to(DEV).contiguous(memory_format=CL)
    after = [t.clone(memory_format=torch.preserve_format) for t in before]
    heads16.crop_backward16(g16, after, boxes, ind, level, crop, accumulate=True)
    torch.cuda.synchronize()
    for l, (a, b) in enumerate(zip(after, before)):
        R.check_increment(a, b, refs[l], mags[l], torch.clamp_min(cnts[l], 1.0).expand_as(refs[l]),
                          "%s accumulate level %d" % (what, l + 2))
        untouched = (cnts[l] == 0).expand_as(a)
        assert torch.equal(a[untouched], b[untouched]), what + ": accumulate changed a cell no tap reaches"
    assert heads16.stats()["crop_bwd"] == 3


def test_the_boxes_hold_the_cases_they_are_there_for():
    """Integer coordinates (a valid tap with floor == ceil), invalid taps next to valid ones, and boxes without a valid
    tap, read from the oracle's own bin assignment."""
    from oracle import oracle as O
    boxes, ind, level, dead = _boxes()
    b, lv, dd = boxes.cpu().numpy(), level.cpu().numpy(), dead.cpu().numpy()
    for crop in ((1, 1), (7, 7), (14, 14), (3, 5)):
        integer = partly = wholly = 0
        for l, s in enumerate(SIZES):
            sel = (lv == l + 2) & ~dd
            t = O.crop_taps(b[sel], s, s, *crop)
            integer += int(((t["y_valid"] != 0) & (t["y0"] == t["y1"])).sum())
            partly += int(((t["y_valid"] != 0).any(1) & (t["y_valid"] == 0).any(1)).sum())
            wholly += int(((t["y_valid"] == 0).all(1) | (t["x_valid"] == 0).all(1)).sum())
        assert integer > 0 and wholly > 0 and (partly > 0 or crop[0] == 1), (crop, integer, partly, wholly)


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_crop_backward_without_boxes_and_refused_calls(sfx):
    from feature_intertwiner_amd import _lib, heads16
    L = heads16.load()
    dtype = DTYPES[sfx]
    C = 8
    none = torch.empty((0, C, 7, 7), device=DEV, dtype=dtype).contiguous(memory_format=CL)
    b0 = torch.empty((0, 4), device=DEV)
    i0 = torch.empty((0,), device=DEV, dtype=torch.int32)
    bufs = _bufs(C, "nan")
    heads16.crop_backward16(none, bufs, b0, i0, i0, 7, accumulate=False)
    torch.cuda.synchronize()
    assert all(bool((b == 0).all()) for b in bufs)
    gen = torch.Generator().manual_seed(2)
    before = _bufs(C, "randn", gen)
    after = [t.clone(memory_format=torch.preserve_format) for t in before]
    heads16.crop_backward16(none, after, b0, i0, i0, 7, accumulate=True)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(after, before))

    # what fi_heads16_eligible refuses: the status, and not a bit of the buffers changes (accumulate = 0 would clear them)
    boxes, ind, level, dead = _boxes()
    n = boxes.shape[0]
    fn = getattr(L, "fi_heads16_pyramid_crop_backward_" + sfx)
    hs = (ctypes.c_int * 4)(*SIZES)
    for depth, shift in ((12, 0), (8, 2)):
        bufs = _bufs(depth, "nan")
        keep = [t.clone(memory_format=torch.preserve_format) for t in bufs]
        g = torch.zeros(n * 49 * depth + 8, device=DEV, dtype=dtype)
        ptrs = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in bufs])
        with torch.cuda.device(torch.device(DEV)):
            rc = fn(ctypes.c_void_p(g.data_ptr() + shift), ptrs, hs, hs, 4, _lib.ptr(boxes), _lib.ptr(ind), _lib.ptr(level), n,
                    BATCH, depth, 7, 7, 0, _lib.current_stream())
        torch.cuda.synchronize()
        assert rc == -3 and b"fi_heads16_pyramid_crop_backward" in _lib.load().fi_last_error(), (depth, shift, rc)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(bufs, keep)), (depth, shift)
    with pytest.raises(_lib.FiError, match="fi_heads16_eligible"):
        heads16.crop_backward16(torch.zeros((n, 12, 7, 7), device=DEV, dtype=dtype).contiguous(memory_format=CL),
                                _bufs(12, "nan"), boxes, ind, level, 7, accumulate=False)


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("size,C", [(7, 72), (14, 264)], ids=["7x72", "14x264"])
def test_crop_backward_is_the_adjoint_of_the_16bit_crop_forward(size, C, sfx):
    from feature_intertwiner_amd import head16, heads16
    dtype = DTYPES[sfx]
    boxes, ind, level, dead = _boxes()
    keep = ~dead                                                  # the forward leaves level -1 rows unwritten
    boxes, ind, level = boxes[keep].contiguous(), ind[keep].contiguous(), level[keep].contiguous()
    n = boxes.shape[0]
    gen = torch.Generator().manual_seed(23 + C)
    maps = [torch.randn((BATCH, C, s, s), generator=gen).to(dtype).to(DEV).contiguous(memory_format=CL) for s in SIZES]
    d16 = torch.randn((n, C, size, size), generator=gen).to(dtype).to(DEV).contiguous(memory_format=CL)
    with torch.no_grad():
        y = head16.pyramid_crop16_cl(maps, boxes, ind, level, size, size)
    bufs = _bufs(C, "nan")
    heads16.crop_backward16(d16, bufs, boxes, ind, level, size, accumulate=False)
    torch.cuda.synchronize()
    d64, y64 = d16.to(torch.float64), y.to(torch.float64)
    lhs = float((y64 * d64).sum())
    rhs = sum(float((m.to(torch.float64) * b.to(torch.float64)).sum()) for m, b in zip(maps, bufs))
    xmax = max(float(m.abs().max()) for m in maps)
    e_fwd = float((d64.abs() * (UNIT[sfx] * y64.abs() + SUBNORMAL[sfx] + 16.0 * R.U * xmax)).sum())
    _, mags, cnts = R.crop_bwd_ref(d16.float().contiguous(), boxes, ind, level, [tuple(b.shape) for b in bufs], size)
    e_bwd = sum(float((m.to(torch.float64).abs() * R.U * (4.0 * torch.sqrt(c) + 16.0) * g).sum())
                for m, g, c in zip(maps, mags, cnts))
    print("adjoint %d C %d %s: lhs %.9g rhs %.9g |d| %.3g bound %.3g (forward %.3g, backward %.3g)"
          % (size, C, sfx, lhs, rhs, abs(lhs - rhs), e_fwd + e_bwd, e_fwd, e_bwd))
    assert abs(lhs) > 1.0 and abs(lhs - rhs) <= e_fwd + e_bwd


# ---- class rows -----------------------------------------------------------------------------------------------------------
# (n, H, W, C, K)
ROWS = [(5, 14, 14, 256, 81), (5, 3, 2, 72, 3), (1, 1, 1, 8, 1), (5, 1, 1, 8, 300), (1, 14, 14, 72, 300), (5, 3, 2, 256, 1),
        (1, 3, 2, 8, 81), (5, 14, 14, 8, 3), (5, 1, 1, 256, 3), (1, 3, 2, 72, 81)]


def _row_inputs(shape, sfx, seed):
    n, H, W, C, K = shape
    dtype = DTYPES[sfx]
    gen = torch.Generator().manual_seed(seed)
    u = torch.relu(torch.randn((n, 4 * C, H, W), generator=gen))             # exact zeros where the ReLU cut
    flat = u.view(-1)
    if flat.numel():
        flat[1::7] = -0.0
        flat[2::11] = 0.0
    u16 = u.to(dtype).to(DEV).contiguous(memory_format=CL)
    d = torch.randn((n, 2, 2, H, W), generator=gen).to(DEV)
    w16 = (torch.randn((K, C), generator=gen) / 4.0).to(dtype).to(DEV)
    cls = torch.randint(0, K, (n,), generator=gen).to(DEV)
    if K == 3:
        cls[:] = 2                                                            # every RoI in one class, two classes empty
    dw0 = (0.25 * torch.randn((K, C), generator=gen)).to(DEV)
    db0 = (0.25 * torch.randn((K,), generator=gen)).to(DEV)
    return d, u16, w16, cls, dw0, db0


def _as_rows(t, n, C, HW):
    """[n, 4 C, H, W] with channels (a, b, c) -> [n, C, 4 HW]: the RoI's (a, b, pixel) rows as the reference's pixels."""
    return t.reshape(n, 4, C, HW).permute(0, 2, 1, 3).reshape(n, C, 4 * HW)


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("shape", ROWS, ids=_ids)
def test_class_rows_backward(shape, sfx):
    from feature_intertwiner_amd import heads16
    n, H, W, C, K = shape
    HW = H * W
    d, u16, w16, cls, dw0, db0 = _row_inputs(shape, sfx, 41 + n + H + C + K)
    what = "class rows %s %s" % (_ids(shape), sfx)
    heads16.reset_stats()
    runs = []
    for _ in range(2):
        dw, db = dw0.clone(), db0.clone()
        du, s = heads16.class_rows_grad16(d, u16, w16, cls, dweight=dw, dbias=db)
        torch.cuda.synchronize()
        runs.append((du, s, dw, db))
    du, s, dw, db = runs[0]
    assert du.dtype == u16.dtype and du.is_contiguous(memory_format=CL) and tuple(du.shape) == tuple(u16.shape)
    assert torch.equal(du.view(torch.int16), runs[1][0].view(torch.int16)), what + ": du differs between two runs"
    print("%s: two runs bitwise equal -- colsum %s, dweight %s, dbias %s" % (
        what, torch.equal(s, runs[1][1]), torch.equal(dw, runs[1][2]), torch.equal(db, runs[1][3])))

    x = _as_rows(u16.to(torch.float64), n, C, HW)
    dx, dw_ref, mw, db_ref, mb, cnt = R.class_row_bwd_ref(d.reshape(n, 4 * HW), x, w16, cls, K, True)
    # du: one fp32 product, one 16-bit rounding; exactly zero where u <= 0
    ref = dx.abs()
    allow = R.U * ref + UNIT[sfx] * (1.0 + R.U) * ref + SUBNORMAL[sfx]
    _held(_as_rows(du.to(torch.float64), n, C, HW), dx, allow, what + " du")
    off = _as_rows((u16.to(torch.float64) > 0), n, C, HW)
    assert bool((_as_rows(du.to(torch.float64), n, C, HW)[~off] == 0).all()) and bool((~off).any()) and bool(off.any())
    assert not bool((du.view(torch.int16)[~(u16 > 0)] != 0).any()), what + ": a masked element is not +0"
    # colsum: the sums of du AS STORED
    du64 = du.to(torch.float64)
    print("%s colsum: worst |d| / (2^-24 m) = %.3f" % (
        what, R.check_bar(s, du64.sum((0, 2, 3)), du64.abs().sum((0, 2, 3)), n * HW, what + " colsum")))
    # dweight / dbias: accumulated into the pre-fill; classes without a RoI keep their bits
    hit = torch.zeros(K, dtype=torch.bool, device=DEV)
    hit[cls] = True
    assert torch.equal(dw[~hit], dw0[~hit]) and torch.equal(db[~hit], db0[~hit]), what + ": an untouched class changed"
    assert K == 1 or n >= K or bool((~hit).any())
    print("%s dweight: worst |d| / (2^-24 m) = %.3f" % (
        what, R.check_increment(dw[hit], dw0[hit], dw_ref[hit], mw[hit], cnt[hit][:, None].expand_as(mw[hit]), what + " dweight")))
    print("%s dbias: worst |d| / (2^-24 m) = %.3f" % (
        what, R.check_increment(db[hit], db0[hit], db_ref[hit], mb[hit], cnt[hit], what + " dbias")))
    # without dweight / dbias / colsum: the same du
    du2, s2 = heads16.class_rows_grad16(d, u16, w16, cls, colsum=False)
    assert s2 is None and torch.equal(du2.view(torch.int16), du.view(torch.int16))
    assert heads16.stats()["class_rows"] == 3


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_class_rows_backward_without_rois_and_refused_calls(sfx):
    from feature_intertwiner_amd import _lib, heads16
    dtype = DTYPES[sfx]
    u16 = torch.empty((0, 32, 3, 2), device=DEV, dtype=dtype).contiguous(memory_format=CL)
    d = torch.empty((0, 2, 2, 3, 2), device=DEV)
    w16 = torch.ones((5, 8), device=DEV, dtype=dtype)
    cls = torch.empty((0,), device=DEV, dtype=torch.int64)
    dw, db = torch.full((5, 8), 3.0, device=DEV), torch.full((5,), 2.0, device=DEV)
    du, s = heads16.class_rows_grad16(d, u16, w16, cls, dweight=dw, dbias=db)
    torch.cuda.synchronize()
    assert tuple(du.shape) == (0, 32, 3, 2) and bool((s == 0).all()) and bool((dw == 3.0).all()) and bool((db == 2.0).all())
    with pytest.raises(_lib.FiError, match="fi_heads16_eligible"):        # C = 12
        heads16.class_rows_grad16(torch.zeros((1, 2, 2, 3, 2), device=DEV),
                                  torch.zeros((1, 48, 3, 2), device=DEV, dtype=dtype).contiguous(memory_format=CL),
                                  torch.zeros((5, 12), device=DEV, dtype=dtype), torch.zeros(1, device=DEV, dtype=torch.int64))
