"""fi_fpn16_topdown_grad (csrc/fpn16.hip, include/fi_fpn16.h) through the raw C entry points, for bf16 and fp16.

Every launch writes into NaN-filled outputs with a sentinel tail of 64 elements behind them that must stay untouched.
g is held to torch.equal: the header fixes the fp32 expression and its order -- t = (f00 + f01) + (f10 + f11), v = own + t,
one rounding -- and torch's fp32 adds are the same IEEE operations, its .to(dtype) the same round-to-nearest-even (an
fp16 overflow goes to infinity in both).  colsum is held to float64 of the ROUNDED g with relu_grad's bar of
tests/test_gpu_grad16_kernels.py: |colsum - ref| <= 2^-24 (4 sqrt(n) + 16) sum |g|, n = N H W (an fp32 sum of n terms in
any order; the atomics are one more order of the same sum).
Inputs: standard normal rounded to the type; max |v| < 6000 is asserted (fp16 overflows at 65504).

Shapes (N, H, W, C) of the COARSE map, the smallest at which each mechanism can go wrong: one lane; 12 and 20 lanes per
pixel, which do not divide the 256 threads, on odd maps; several workgroups per channel, so that the global atomics meet;
261 lanes per pixel, past the 2048 channels whose sums one workgroup holds.  Every shape runs with both operands, with
`fine` only and with `own` only, and `own` only again in place (the read-only column-sum pass)."""
import functools
import math

import pytest
import torch

import fp64_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
BITS = {"bf16": 8, "f16": 11}
TAIL = 64

SHAPES = [
    (1, 1, 1, 8),
    (2, 3, 5, 96),
    (3, 7, 9, 160),
    (2, 40, 36, 256),                # several workgroups, atomics
    (1, 2, 2, 2088),                 # past one channel tile
]
MODES = ["both", "fine", "own"]
_ids = lambda s: "x".join(map(str, s))


def _libs():
    from feature_intertwiner_amd import _lib, fpn16
    return _lib, fpn16.load()


def _nan_buf(numel, dtype):
    buf = torch.full((numel + TAIL,), float("nan"), device=DEV, dtype=dtype)
    buf[numel:] = 7.0
    return buf


def _tail_ok(buf, numel):
    assert torch.equal(buf[numel:], torch.full((TAIL,), 7.0, device=DEV, dtype=buf.dtype)), "sentinel tail written"


def _expression(own, fine, dtype):
    """The header's fp32 expression in its order, rounded once: own [N, H, W, C], fine [N, 2H, 2W, C], either may be None."""
    if fine is None:
        return own.float().to(dtype)
    f = fine.float()
    t = (f[:, 0::2, 0::2] + f[:, 0::2, 1::2]) + (f[:, 1::2, 0::2] + f[:, 1::2, 1::2])
    v = t if own is None else own.float() + t
    return v.to(dtype)


@functools.lru_cache(maxsize=None)
def _operands(shape, sfx):
    """Seeded 16-bit operands on the device and, per mode, the expected g with its float64 column sums."""
    N, H, W, C = shape
    dtype = DTYPES[sfx]
    gen = torch.Generator().manual_seed(131 * sum(shape) + C)
    own = torch.randn((N, H, W, C), generator=gen).to(dtype).to(DEV)
    fine = torch.randn((N, 2 * H, 2 * W, C), generator=gen).to(dtype).to(DEV)
    out = dict(t_own=own, t_fine=fine)
    for mode in MODES:
        g = _expression(own if mode != "fine" else None, fine if mode != "own" else None, dtype)
        g64 = g.to(torch.float64)
        out[mode] = (g, g64.sum((0, 1, 2)), g64.abs().sum((0, 1, 2)))
    return out


def _topdown(shape, sfx, own, fine, colsum=True, g_buf=None):
    """-> (g [N, H, W, C], colsum [C] or None); g_buf: write there instead of a NaN-filled buffer (in place)."""
    _lib, L = _libs()
    N, H, W, C = shape
    numel = N * H * W * C
    gbuf = _nan_buf(numel, DTYPES[sfx]) if g_buf is None else g_buf
    sbuf = _nan_buf(C, torch.float32) if colsum else None
    for t, n in ((own, numel), (fine, 4 * numel)):
        assert t is None or (t.is_contiguous() and t.numel() >= n)          # the kernel's reads stay inside the operands
    assert L.fi_fpn16_eligible(N, H, W, C, _lib.ptr(own), _lib.ptr(fine), _lib.ptr(gbuf), _lib.ptr(sbuf)) == 1
    _lib.check(getattr(L, "fi_fpn16_topdown_grad_" + sfx)(_lib.ptr(own), _lib.ptr(fine), _lib.ptr(gbuf), _lib.ptr(sbuf),
                                                          N, H, W, C, _lib.current_stream()), "fi_fpn16_topdown_grad")
    torch.cuda.synchronize()
    _tail_ok(gbuf, numel)
    if colsum:
        _tail_ok(sbuf, C)
    return gbuf[:numel].view(N, H, W, C), (sbuf[:C] if colsum else None)


def _sums_held(s, ref, mag, n, what):
    allow = R.U * (4.0 * math.sqrt(n) + 16.0) * mag
    d = (s.to(torch.float64) - ref).abs()
    assert bool(torch.isfinite(s).all())
    worst = float(torch.where(d == 0, torch.zeros_like(d), d / allow).max())
    print("%s: worst |d| / bar = %.3f" % (what, worst))
    assert worst <= 1.0, what


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_topdown_grad_bits_and_column_sums(shape, mode, sfx):
    ops = _operands(shape, sfx)
    want, s_ref, s_mag = ops[mode]
    own = ops["t_own"] if mode != "fine" else None
    fine = ops["t_fine"] if mode != "own" else None
    assert float(want.float().abs().max()) < 6000.0
    n = shape[0] * shape[1] * shape[2]
    g, s = _topdown(shape, sfx, own, fine)
    assert torch.equal(g.view(torch.int16), want.view(torch.int16))
    _sums_held(s, s_ref, s_mag, n, "%s %s %s colsum" % (sfx, shape, mode))
    # colsum = NULL: the same g
    g2, s2 = _topdown(shape, sfx, own, fine, colsum=False)
    assert s2 is None and torch.equal(g2.view(torch.int16), want.view(torch.int16))      # and two runs agree bit for bit
    if mode == "own":
        # in place, nothing to add: a read-only pass that sums -- the tensor keeps its bits, the tail included
        numel = own.numel()
        buf = torch.cat([own.reshape(-1), torch.full((TAIL,), 7.0, device=DEV, dtype=own.dtype)])
        g3, s3 = _topdown(shape, sfx, buf[:numel].view(shape), None, g_buf=buf)
        assert g3.data_ptr() == buf.data_ptr() and torch.equal(g3.view(torch.int16), own.view(torch.int16))
        _sums_held(s3, s_ref, s_mag, n, "%s %s in place colsum" % (sfx, shape))


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3]], ids=_ids)
def test_topdown_grad_in_place_with_a_fine_operand(shape, sfx):
    """g = own: every lane reads the 8 values it then writes."""
    ops = _operands(shape, sfx)
    want, s_ref, s_mag = ops["both"]
    numel = want.numel()
    buf = torch.cat([ops["t_own"].reshape(-1), torch.full((TAIL,), 7.0, device=DEV, dtype=want.dtype)])
    g, s = _topdown(shape, sfx, buf[:numel].view(shape), ops["t_fine"], g_buf=buf)
    assert torch.equal(g.view(torch.int16), want.view(torch.int16))
    _sums_held(s, s_ref, s_mag, shape[0] * shape[1] * shape[2], "%s %s in place + fine colsum" % (sfx, shape))


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_small_integer_known_answers_are_exact(sfx):
    """Integers in [-4, 4]: every partial sum is exact in fp32 and every result exact in the type, whatever the order; the
    column sums are integers below 2^24 and exact as well."""
    dtype = DTYPES[sfx]
    shape = (2, 5, 6, 40)
    N, H, W, C = shape
    gen = torch.Generator().manual_seed(5)
    own = torch.randint(-4, 5, (N, H, W, C), generator=gen).to(torch.float64)
    fine = torch.randint(-4, 5, (N, 2 * H, 2 * W, C), generator=gen).to(torch.float64)
    cells = fine.view(N, H, 2, W, 2, C).sum((2, 4))
    for o, f, want in ((own, fine, own + cells), (None, fine, cells), (own, None, own)):
        g, s = _topdown(shape, sfx, None if o is None else o.to(dtype).to(DEV), None if f is None else f.to(dtype).to(DEV))
        assert torch.equal(g.double().cpu(), want)
        assert torch.equal(s.double().cpu(), want.sum((0, 1, 2)))
    # one pixel, one cell: 1 + (2 + 3 + 4 + 5) in channel 0, zeros elsewhere
    own1 = torch.zeros((1, 1, 1, 8), dtype=dtype, device=DEV)
    fine1 = torch.zeros((1, 2, 2, 8), dtype=dtype, device=DEV)
    own1[..., 0] = 1.0
    fine1[0, :, :, 0] = torch.tensor([[2.0, 3.0], [4.0, 5.0]], dtype=dtype, device=DEV)
    g, s = _topdown((1, 1, 1, 8), sfx, own1, fine1)
    assert g.flatten().tolist() == [15.0] + [0.0] * 7 and s.tolist() == [15.0] + [0.0] * 7


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_the_cell_sum_and_the_add_are_rounded_once(sfx):
    """t = 1 + e/2 with e = the rounding unit at 1 (exact in fp32, rounds to 1 in the type) and own = e: own + t lies above
    the tie and rounds UP once; rounding t first gives the tie 1 + e, which goes to the even 1."""
    p = BITS[sfx]
    dtype = DTYPES[sfx]
    shape = (1, 3, 3, 16)
    e = 2.0 ** -p
    fine = torch.zeros((1, 6, 6, 16), dtype=torch.float64)
    fine[:, 0::2, 0::2] = 1.0
    fine[:, 1::2, 1::2] = e / 2                                      # the other diagonal of the cell
    fine[:, 2:4] *= -1.0                                             # and mirrored: the middle coarse row is negative
    own = torch.full((1, 3, 3, 16), e, dtype=torch.float64)
    own[:, 1] *= -1.0
    f16, o16 = fine.to(dtype).to(DEV), own.to(dtype).to(DEV)
    assert torch.equal(f16.double().cpu(), fine) and torch.equal(o16.double().cpu(), own)      # operands exact in the type
    t = fine.view(1, 3, 2, 3, 2, 16).sum((2, 4))
    once = (own + t).to(dtype)
    twice = (own + t.to(dtype).double()).to(dtype)
    assert torch.equal(once.double().abs(), torch.full((1, 3, 3, 16), 1.0 + 2 * e, dtype=torch.float64))
    assert not torch.equal(once, twice)                              # the case separates the two
    g, s = _topdown(shape, sfx, o16, f16)
    assert torch.equal(g.cpu(), once)
    assert torch.equal(s.double().cpu(), once.double().sum((0, 1, 2)))


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_bits_do_not_depend_on_placement_or_run(sfx):
    """One image repeated three times in a batch (its pixels fall into different workgroups at different offsets) gives
    three bit-equal gradients, and a second run repeats the first bit for bit."""
    shape = (1, 7, 9, 160)
    ops = _operands(shape, sfx)
    own3, fine3 = ops["t_own"].repeat(3, 1, 1, 1), ops["t_fine"].repeat(3, 1, 1, 1)
    a, _ = _topdown((3, 7, 9, 160), sfx, own3, fine3)
    b, _ = _topdown((3, 7, 9, 160), sfx, own3, fine3)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    for i in range(3):
        assert torch.equal(a[i].view(torch.int16), ops["both"][0][0].view(torch.int16))


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_the_python_wrapper(sfx):
    """fpn16.topdown_grad16 on [N, C, H, W] channels-last tensors: the same bits, the counters, `out` in place."""
    from feature_intertwiner_amd import _lib, fpn16
    shape = (2, 3, 5, 96)
    ops = _operands(shape, sfx)
    own, fine = ops["t_own"].permute(0, 3, 1, 2), ops["t_fine"].permute(0, 3, 1, 2)
    fpn16.reset_stats()
    g, s = fpn16.topdown_grad16(own, fine)
    assert g.is_contiguous(memory_format=torch.channels_last) and tuple(g.shape) == tuple(own.shape)
    assert torch.equal(g.permute(0, 2, 3, 1).view(torch.int16), ops["both"][0].view(torch.int16))
    _sums_held(s, ops["both"][1], ops["both"][2], 30, "wrapper colsum")
    g, s = fpn16.topdown_grad16(None, fine, colsum=False)
    assert s is None and torch.equal(g.permute(0, 2, 3, 1).view(torch.int16), ops["fine"][0].view(torch.int16))
    assert fpn16.stats()["topdown"] == 2 and fpn16.stats()["sums"] == 0
    g, s = fpn16.topdown_grad16(own, None, out=own)
    assert g is own and fpn16.stats()["sums"] == 1
    _sums_held(s, ops["own"][1], ops["own"][2], 30, "wrapper read-only colsum")
    with pytest.raises(_lib.FiError, match="double-resolution"):
        fpn16.topdown_grad16(own, own)
    with pytest.raises(_lib.FiError, match="fi_fpn16_eligible"):
        fpn16.topdown_grad16(own[:, :4].contiguous(memory_format=torch.channels_last), None)
