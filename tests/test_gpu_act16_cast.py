"""fi_act16_pack_{bf16,f16} / fi_act16_unpack_{bf16,f16}: the transposing casts between fp32 NCHW and the 16-bit
channels-last tensors (csrc/conv_act16.hip), bit for bit against torch on the CPU.

pack is x.permute(0, 2, 3, 1).contiguous().to(dtype) (round to nearest even), unpack the exact widening back.  The values
include +-0, the rounding ties of each type (1 + 2^-8 rounds down to even and 1 + 3 * 2^-8 up to even in bf16; the 2^-11
analogues in fp16), fp16's overflow boundary (65519 -> 65504, 65520 -> inf) and its subnormal range."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
SHAPES = [(1, 8, 1, 1), (2, 24, 5, 7), (3, 264, 9, 15), (1, 64, 2, 130)]


def _specials(dtype):
    t = 2.0 ** -8 if dtype is torch.bfloat16 else 2.0 ** -11
    v = [0.0, -0.0, 1.0, -1.0, 1.0 + t, 1.0 + 3 * t, -(1.0 + t), -(1.0 + 3 * t), 1.0 + t * 1.0001, 1.0 + t * 0.9999,
         65504.0, 65519.0, 65520.0, -65519.0, -65520.0, 1.0e5,
         2.0 ** -14, 2.0 ** -15, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 2.0 ** -26, -(2.0 ** -24), 3.0 * 2.0 ** -25,
         6.0e-8, 5.9e-8, 1.0e-7, 3.3e-6]
    return torch.tensor(v, dtype=torch.float32)


def _values(shape, dtype):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g) * 4.0
    flat = x.reshape(-1)
    sp = _specials(dtype)
    n = min(flat.numel(), sp.numel())
    idx = torch.randperm(flat.numel(), generator=g)[:n]
    flat[idx] = sp[:n]
    if flat.numel() >= 2 * sp.numel():                   # fp16's subnormals, a ramp of them
        ramp = torch.arange(sp.numel(), dtype=torch.float32) * (2.0 ** -25) * 0.75
        flat[torch.randperm(flat.numel(), generator=g)[:sp.numel()]] = ramp
    return flat.reshape(shape)


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("prec", sorted(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pack_and_unpack_are_bit_equal_to_torch(shape, prec):
    from feature_intertwiner_amd import act16
    dtype = DTYPES[prec]
    x = _values(shape, dtype)
    want = x.permute(0, 2, 3, 1).contiguous().to(dtype)                     # [N, H, W, C] on the CPU
    act16.reset_stats()
    y = act16.pack(x.to(DEV), dtype)
    assert y.dtype is dtype and tuple(y.shape) == tuple(shape) and y.is_contiguous(memory_format=torch.channels_last)
    got = y.permute(0, 2, 3, 1)
    assert got.is_contiguous()                                              # NHWC in memory
    assert torch.equal(_bits(got.cpu()), _bits(want))
    back = act16.unpack(y)
    assert back.dtype is torch.float32 and tuple(back.shape) == tuple(shape) and back.is_contiguous()
    wide = want.to(torch.float32).permute(0, 3, 1, 2).contiguous()
    assert torch.equal(back.cpu().view(torch.int32), wide.view(torch.int32))
    assert act16.stats() == {"conv": 0, "pack": 1, "unpack": 1}


@pytest.mark.parametrize("prec", sorted(DTYPES))
def test_raw_entry_points_leave_a_sentinel_tail_alone(prec):
    """Through the C entry points on NaN-filled outputs with 64 sentinel elements behind them."""
    from feature_intertwiner_amd import _lib, act16
    L = act16.load()
    dtype, sfx = DTYPES[prec], {"bf16": "bf16", "fp16": "f16"}[prec]
    N, C, H, W = 3, 264, 9, 15
    x = _values((N, C, H, W), dtype).to(DEV)
    numel = x.numel()
    buf = torch.full((numel + 64,), float("nan"), device=DEV, dtype=dtype)
    buf[numel:] = 7.0
    _lib.check(getattr(L, "fi_act16_pack_" + sfx)(_lib.ptr(x), _lib.ptr(buf), N, C, H, W, _lib.current_stream()), "pack")
    out = torch.full((numel + 64,), float("nan"), device=DEV, dtype=torch.float32)
    out[numel:] = 7.0
    _lib.check(getattr(L, "fi_act16_unpack_" + sfx)(_lib.ptr(buf), _lib.ptr(out), N, C, H, W, _lib.current_stream()),
               "unpack")
    torch.cuda.synchronize()
    assert bool((buf[numel:] == 7.0).all()) and bool((out[numel:] == 7.0).all())
    want = x.cpu().permute(0, 2, 3, 1).contiguous().to(dtype)
    assert torch.equal(_bits(buf[:numel].cpu()), _bits(want.reshape(-1)))
    assert torch.equal(out[:numel].cpu().view(N, C, H, W), want.to(torch.float32).permute(0, 3, 1, 2).contiguous())
