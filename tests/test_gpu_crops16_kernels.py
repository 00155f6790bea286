"""libfi_crops16.so through its raw entry points, bf16 and fp16.

Patch rows.  Maps 2 x C x {16x24, 8x12, 4x6, 2x3} and p6 as the step-2 level of the 2x3 tensor (1x2), 3 anchors per pixel,
C = 256 and C = 8, 40 rows and none.  The rows hold the four corners of a level (taps off the map), three anchors of one
pixel, two horizontally and two diagonally adjacent pixels, a padding row, both images, a repeated anchor, and a p6 row
next to a p5 row that meet on p5 pixels (0, 0) and (0, 2).
  - forward: torch.equal to fi_pyramid_patch_rows_forward on the unpacked maps (p6 as its own fp32 map);
  - backward, per tensor: S = old + the float64 sum of fp64_ref.patch_rows_bwd_ref (p6's reference added into p5's grid at
    the even pixels).  got is ONE rounding of an fp32 sum of `terms` values plus old, so
        |got - S| <= 1/2 ulp16(got) + 2^-24 (4 sqrt(n) + 16) m,     m = |old| + sum |d|,  n = terms + 1
    -- half a unit of the 16-bit result for the rounding, fp64_ref.check_bar's allowance for the fp32 sum in front of it;
    untouched elements keep their bits; a second run from the same inputs gives the same bits.
Gate-pack.  (2, 256, 5, 7), (1, 256, 1, 2), (3, 64, 16, 24), (1, 8, 3, 3) and N = 0; d holds normal values, +-0, exact ties
between two 16-bit neighbours, values below the type's smallest subnormal, fp16-subnormal magnitudes and values beyond
the type's maximum; y holds positives, negatives, +0, -0 and the smallest subnormal.
  - g is torch.equal to grad16.relu_grad16(act16.pack(d), y)'s, and to act16.pack(d) without y.  relu_grad16 takes
    C % 32 == 0 only: for the 8-channel shape the reference is its definition, act16.pack(d) where y > 0 and +0 elsewhere;
  - the sums are within fp64_ref.check_bar of the float64 sums of g (m = sum |g|, n = pixels); a channel whose g holds an
    infinity (the value beyond the maximum) must sum to that infinity -- the bar is for finite sums."""
import ctypes
import math

import pytest
import torch

import fp64_ref as R
from test_gpu_grad16_layer import CL, DEV, DTYPES

pytestmark = pytest.mark.gpu
# (mantissa bits, exponent of the smallest normal)
FORMAT = {"bf16": (7, -126), "f16": (10, -14)}
SIZES = ((16, 24), (8, 12), (4, 6), (2, 3))
PER_LOC = 3


def ulp16(got, sfx):
    """The spacing of the 16-bit format at |got| (float64), the subnormal spacing below the smallest normal."""
    mant, emin = FORMAT[sfx]
    a = got.to(torch.float64).abs()
    e = torch.floor(torch.log2(torch.clamp_min(a, 2.0 ** (emin - 1)))).clamp_min(float(emin))
    return torch.pow(torch.full_like(e, 2.0), e - mant)


def held16(got, ref, mag, n, sfx, what):
    """|got - ref| <= 1/2 ulp16(got) + check_bar's allowance 2^-24 (4 sqrt(n) + 16) m, per element."""
    got64 = got.to(torch.float64)
    n = n.to(torch.float64) if torch.is_tensor(n) else torch.tensor(float(n), dtype=torch.float64, device=got.device)
    allow = 0.5 * ulp16(got64, sfx) + R.U * (4.0 * torch.sqrt(n) + 16.0) * mag
    d = (got64 - ref).abs()
    d = torch.where(torch.isfinite(got64), d, torch.full_like(d, float("inf")))
    ratio = torch.where(d == 0, torch.zeros_like(d), d / allow)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print("%s: worst |d| / bound = %.3f" % (what, worst))
    assert worst <= 1.0, (what, worst)


def _starts():
    out, s = [], 0
    for h, w in SIZES + ((1, 2),):
        out.append(s)
        s += h * w * PER_LOC
    return out


def _rows(n_extra=23, seed=5):
    st = _starts()
    widths = [w for _, w in SIZES] + [2]

    def a(l, h, w, k=0):
        return st[l] + (h * widths[l] + w) * PER_LOC + k
    rows = [(0, a(0, 0, 0)), (0, a(0, 0, 23, 1)), (1, a(0, 15, 0, 2)), (0, a(0, 15, 23)),       # the corners of a level
            (1, a(1, 3, 5, 0)), (1, a(1, 3, 5, 1)), (1, a(1, 3, 5, 2)),                          # three anchors of one pixel
            (0, a(0, 7, 10)), (0, a(0, 7, 11, 1)),                                               # horizontal neighbours
            (1, a(2, 1, 2)), (1, a(2, 2, 3, 2)),                                                 # diagonal neighbours
            (-1, a(1, 2, 2)),                                                                    # a padding row
            (0, a(4, 0, 0)), (0, a(3, 0, 1, 1)),                    # p6 (0, 0) and p5 (0, 1): both reach p5 (0, 0) and (0, 2)
            (1, a(4, 0, 1, 2)), (1, a(3, 1, 2)),                    # p6 (0, 1) = p5 (0, 2), and p5's last pixel
            (0, a(0, 7, 10))]                                                                    # a repeated anchor
    gen = torch.Generator().manual_seed(seed)
    total = st[-1] + 2 * PER_LOC
    for _ in range(n_extra):
        rows.append((int(torch.randint(0, 2, (1,), generator=gen)), int(torch.randint(0, total, (1,), generator=gen))))
    image = torch.tensor([r[0] for r in rows], dtype=torch.int64, device=DEV)
    anchor = torch.tensor([r[1] for r in rows], dtype=torch.int64, device=DEV)
    return image, anchor


def _tables(tensors):
    """The five levels: the four tensors, and the last one once more with step 2."""
    lv = list(tensors) + [tensors[-1]]
    n = len(lv)
    return ((ctypes.c_void_p * n)(*[t.data_ptr() for t in lv]), (ctypes.c_int * n)(*[t.shape[2] for t in lv]),
            (ctypes.c_int * n)(*[t.shape[3] for t in lv]), (ctypes.c_int * n)(1, 1, 1, 1, 2), n)


def _call(fn, what, *args):
    from feature_intertwiner_amd import _lib
    with torch.cuda.device(torch.device(DEV)):
        _lib.check(fn(*args, _lib.current_stream()), what)


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("C,with_rows", [(256, True), (8, True), (256, False)])
def test_patch_rows_forward_bits_and_in_place_backward(C, with_rows, sfx):
    from feature_intertwiner_amd import _lib, act16, crops16
    from feature_intertwiner_amd.sub_module import _PatchRowsFn
    L = crops16.load()
    dtype = DTYPES[sfx]
    gen = torch.Generator().manual_seed(11 + C)
    maps = [torch.randn((2, C, h, w), generator=gen).to(dtype).to(DEV).contiguous(memory_format=CL) for h, w in SIZES]
    image, anchor = _rows()
    if not with_rows:
        image, anchor = image[:0], anchor[:0]
    rows = image.numel()
    assert rows == (40 if with_rows else 0)
    ptrs, hs, ws, st, n = _tables(maps)
    out = torch.full((rows, 9 * C), float("nan"), device=DEV)
    _call(getattr(L, "fi_crops16_patch_rows_forward_" + sfx), "forward", ptrs, hs, ws, st, n, PER_LOC, _lib.ptr(image),
          _lib.ptr(anchor), rows, 2, C, _lib.ptr(out))
    wide = [act16.unpack(m) for m in maps]
    wide.append(wide[3][:, :, ::2, ::2].contiguous())
    with torch.no_grad():
        want = _PatchRowsFn.apply(image, anchor, PER_LOC, None, *wide)
    assert torch.equal(out, want)
    if with_rows:
        assert float(out.abs().max()) > 0.0 and bool((out.view(rows, 9, C)[11] == 0).all())     # the padding row
        assert bool((out.view(rows, 9, C)[0, 0] == 0).all())                                    # a tap off the map

    # backward, in place into gradients that hold something already
    old = [(0.5 * torch.randn(tuple(m.shape), generator=gen)).to(dtype).to(DEV).contiguous(memory_format=CL) for m in maps]
    d = torch.randn((rows, 9 * C), generator=gen).to(DEV)
    runs = []
    for _ in range(2):
        grads = [t.clone(memory_format=torch.preserve_format) for t in old]
        gp, _, _, _, _ = _tables(grads)
        _call(getattr(L, "fi_crops16_patch_rows_backward_" + sfx), "backward", _lib.ptr(d), gp, hs, ws, st, n, PER_LOC,
              _lib.ptr(image), _lib.ptr(anchor), rows, 2, C)
        torch.cuda.synchronize()
        runs.append(grads)
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))                            # two runs, the same bits
    grads = runs[0]
    if not with_rows:
        for g, o in zip(grads, old):
            assert torch.equal(g.view(torch.int16), o.view(torch.int16))
        return
    shapes = [tuple(m.shape) for m in maps] + [(2, C, 1, 2)]
    refs, mags, _ = R.patch_rows_bwd_ref(d.view(rows, 9, C), shapes, image, anchor, PER_LOC)
    cnts, _, _ = R.patch_rows_bwd_ref(torch.ones_like(d).view(rows, 9, C), shapes, image, anchor, PER_LOC)
    for t in (refs, mags, cnts):                                      # p6 lives on the even pixels of p5's grid
        t[3] = t[3].clone()
        t[3][:, :, ::2, ::2] += t[4]
    assert float(cnts[3][0, 0, 0, 0]) >= 2 and float(cnts[3][0, 0, 0, 2]) >= 2      # the p6 row and the p5 row met there
    assert float(cnts[1][1, 0, 3, 5]) >= 3 and float(cnts[0][0, 0, 7, 10]) >= 3
    for l in range(4):
        o64 = old[l].to(torch.float64)
        touched = cnts[l] > 0
        assert bool(touched.any()) and (l > 0 or not bool(touched.all()))
        same = grads[l].view(torch.int16) == old[l].view(torch.int16)
        assert bool((same | touched).all()), "level %d: an untouched element changed" % l
        held16(grads[l], torch.where(touched, o64 + refs[l], o64), o64.abs() + mags[l], cnts[l] + 1.0, sfx,
               "patch rows backward C %d %s level %d" % (C, sfx, l))


def _special(sfx):
    mant, emin = FORMAT[sfx]
    tie = 2.0 ** -(mant + 1)
    sub = 2.0 ** (emin - mant)                                        # the smallest subnormal
    big = 3.4e38 if sfx == "bf16" else 7.0e4                          # beyond the maximum: rounds to infinity
    v = [0.0, -0.0, 1.0 + tie, 1.0 + 3 * tie, -(1.0 + tie), -(2.0 + 6 * tie), sub / 4, -sub / 4, sub / 2, 1.5 * sub, -2.5 * sub,
         1.3 * 2.0 ** -16, -1.7 * 2.0 ** -20, 2.0 ** -24, 3 * 2.0 ** -25, 2.0 ** -25, big, -big]
    return torch.tensor(v, dtype=torch.float32)


def _gate_inputs(shape, sfx, seed):
    dtype = DTYPES[sfx]
    _, emin = FORMAT[sfx]
    gen = torch.Generator().manual_seed(seed)
    d = torch.randn(shape, generator=gen)
    sp = _special(sfx)
    flat = d.view(-1)
    if flat.numel():
        pos = torch.randperm(flat.numel(), generator=gen)[:2 * sp.numel()]
        flat[pos] = torch.cat((sp, sp))                               # each value twice: with luck under both mask bits
    y = torch.randn(shape, generator=gen).to(dtype)
    if y.numel():
        yf = y.view(-1)
        sub = torch.tensor(2.0 ** (emin - FORMAT[sfx][0]), dtype=torch.float64).to(dtype)
        for k, val in enumerate((torch.tensor(0.0).to(dtype), torch.tensor(-0.0).to(dtype), sub, -sub)):
            yf[k::7] = val                                            # +0, -0, the smallest subnormal, its negative
    return d.to(DEV), y.to(DEV).contiguous(memory_format=CL)


def _check_sums(s, g, what):
    g64 = g.to(torch.float64)
    ref, mag = g64.sum((0, 2, 3)), g64.abs().sum((0, 2, 3))
    fin = torch.isfinite(ref) & torch.isfinite(mag)
    P = g.shape[0] * g.shape[2] * g.shape[3]
    print("%s: sums worst |d| / (2^-24 m) = %.3f" % (what, R.check_bar(s[fin], ref[fin], mag[fin], max(P, 1), what)))
    got = s[~fin].to(torch.float64)                                  # an infinity in g: the sum is that infinity (or NaN for both)
    assert bool(((got == ref[~fin]) | (torch.isnan(got) & torch.isnan(ref[~fin]))).all()), what


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("shape", [(2, 256, 5, 7), (1, 256, 1, 2), (3, 64, 16, 24), (1, 8, 3, 3)],
                         ids=lambda s: "x".join(map(str, s)))
def test_gate_pack_bits_and_sums(shape, sfx):
    from feature_intertwiner_amd import _lib, act16, crops16, grad16
    L = crops16.load()
    dtype = DTYPES[sfx]
    d, y = _gate_inputs(shape, sfx, 31 + shape[1] + shape[2])
    N, C, H, W = shape
    d_cl = d.contiguous(memory_format=CL)
    packed = act16.pack(d, dtype)
    if C % 32 == 0:
        want = grad16.relu_grad16(packed, y)[0]
    else:                                                             # relu_grad16 takes C % 32 == 0: its definition
        want = torch.where(y > 0, packed, torch.zeros_like(packed))
    fn = getattr(L, "fi_crops16_gate_pack_" + sfx)
    for mask, ref in ((y, want), (None, packed)):
        g = torch.full(shape, float("nan"), device=DEV).to(dtype).contiguous(memory_format=CL)
        s = torch.full((C,), float("nan"), device=DEV)
        _call(fn, "gate_pack", _lib.ptr(d_cl), _lib.ptr(mask), _lib.ptr(g), _lib.ptr(s), N, H, W, C)
        torch.cuda.synchronize()
        assert torch.equal(g.view(torch.int16), ref.view(torch.int16)), "g bits (%s)" % ("masked" if mask is not None else "plain")
        _check_sums(s, g, "gate-pack %s %s %s" % (shape, sfx, "masked" if mask is not None else "plain"))
        g2 = torch.empty_like(g)
        _call(fn, "gate_pack", _lib.ptr(d_cl), _lib.ptr(mask), _lib.ptr(g2), None, N, H, W, C)     # without sums
        assert torch.equal(g2.view(torch.int16), g.view(torch.int16))
    # the special values really are in there: an infinity, a signed zero from an underflow, a masked-off element
    assert bool(torch.isinf(packed).any()) and bool((want == 0).any()) and bool((want != 0).any())
    # the wrapper: the same launch
    gw, sw = crops16.gate_pack16(d_cl, y)
    assert torch.equal(gw.view(torch.int16), want.view(torch.int16)) and gw.is_contiguous(memory_format=CL)
    _check_sums(sw, gw, "gate_pack16 wrapper")
    gp, sp = crops16.gate_pack16(d_cl, None, dtype=dtype, colsum=False)
    assert sp is None and torch.equal(gp.view(torch.int16), packed.view(torch.int16))


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_gate_pack_of_an_empty_batch_zero_fills_the_sums(sfx):
    from feature_intertwiner_amd import _lib, crops16
    L = crops16.load()
    s = torch.ones(256, device=DEV)
    d = torch.empty((0, 256, 5, 7), device=DEV).contiguous(memory_format=CL)
    g = torch.empty((0, 256, 5, 7), device=DEV, dtype=DTYPES[sfx]).contiguous(memory_format=CL)
    _call(getattr(L, "fi_crops16_gate_pack_" + sfx), "gate_pack", _lib.ptr(d), None, _lib.ptr(g), _lib.ptr(s), 0, 5, 7, 256)
    torch.cuda.synchronize()
    assert bool((s == 0).all())
    gw, sw = crops16.gate_pack16(d, None, dtype=DTYPES[sfx])
    assert tuple(gw.shape) == (0, 256, 5, 7) and bool((sw == 0).all())
    assert math.isfinite(float(sw.sum()))
