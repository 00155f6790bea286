"""The transposed 3x3 / stride 2 / padding 1 / output_padding 1 convolution (csrc/conv_transpose.hip, libfi_convt.so,
conv.ConvTranspose3x3 / conv.convt_bn_act) against F.conv_transpose2d in float64 on the CPU and its autograd.

Tolerance: the project's own (tests/test_gpu_conv.py), |d| <= 2e-5 * sqrt(k) * (max|ref| + 1e-6) with k the reduction
length: y 4 Cin (the most taps any output element sums), dx 9 Cout, dw N H W, dbias 4 N H W; dgamma and dbeta are sums
over the same N * 2H * 2W elements as dbias and take its k.  Inputs are standard normal: a wrong tap or halo shows."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (N, Cin, Cout, H, W)
SHAPES = [
    (1, 16, 8, 1, 1),          # every halo read is outside the image
    (2, 32, 24, 5, 7),         # ragged tile in both directions, Cout below a wavefront's share, image stride
    (3, 48, 136, 9, 33),       # more than one tile along Cout, rows and columns; three channel blocks: the double buffer wraps
    (2, 16, 4, 2, 70),         # wide, short map
    (1, 256, 256, 16, 16),     # the model's channel count
    (2, 12, 20, 6, 5),         # not kernel-eligible: the four-class composition, same assertions
]
ELIGIBLE = SHAPES[:5]
EPS = 1e-5


def _tol(ref, k):
    return 2e-5 * math.sqrt(k) * (ref.abs().max().item() + 1e-6)


def _close(got, ref, k, what):
    err = (got.detach().cpu().double() - ref).abs().max().item()
    print("%s: max|d| %.3e, bound %.3e" % (what, err, _tol(ref, k)))
    assert got.shape == ref.shape, what
    assert err <= _tol(ref, k), (what, err, _tol(ref, k))


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs and the float64 reference of a shape, computed once: plain (bias only) and fused (eval BN + ReLU)."""
    N, Cin, Cout, H, W = shape
    g = torch.Generator().manual_seed(sum(shape))
    c = {"x": torch.randn(N, Cin, H, W, generator=g), "w": torch.randn(Cin, Cout, 3, 3, generator=g),
         "b": torch.randn(Cout, generator=g), "gamma": torch.rand(Cout, generator=g) + 0.5,
         "beta": torch.randn(Cout, generator=g), "mean": torch.randn(Cout, generator=g),
         "var": torch.rand(Cout, generator=g) * 1.5 + 0.5, "gy": torch.randn(N, Cout, 2 * H, 2 * W, generator=g)}
    xd, wd, bd = (c[k].double().requires_grad_(True) for k in ("x", "w", "b"))
    yd = F.conv_transpose2d(xd, wd, bd, stride=2, padding=1, output_padding=1)
    yd.backward(c["gy"].double())
    c["plain"] = {"y": yd.detach(), "dx": xd.grad, "dw": wd.grad, "db": bd.grad}
    xd, wd, bd, gd, ed = (c[k].double().requires_grad_(True) for k in ("x", "w", "b", "gamma", "beta"))
    z = F.conv_transpose2d(xd, wd, bd, stride=2, padding=1, output_padding=1)
    yd = F.relu(F.batch_norm(z, c["mean"].double(), c["var"].double(), gd, ed, False, 0.0, EPS))
    yd.backward(c["gy"].double())
    c["fused"] = {"y": yd.detach(), "dx": xd.grad, "dw": wd.grad, "db": bd.grad, "dgamma": gd.grad, "dbeta": ed.grad}
    return c


def _modules(c, shape):
    from feature_intertwiner_amd.conv import ConvTranspose3x3
    _, Cin, Cout, _, _ = shape
    conv = ConvTranspose3x3(Cin, Cout, kernel_size=3, stride=2, padding=1, output_padding=1)
    bn = nn.BatchNorm2d(Cout, eps=EPS)
    with torch.no_grad():
        conv.weight.copy_(c["w"])
        conv.bias.copy_(c["b"])
        bn.weight.copy_(c["gamma"])
        bn.bias.copy_(c["beta"])
        bn.running_mean.copy_(c["mean"])
        bn.running_var.copy_(c["var"])
    return conv.to(DEV), bn.to(DEV).eval()


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_plain(shape):
    c = _case(shape)
    conv, _ = _modules(c, shape)
    with torch.no_grad():
        y = conv(c["x"].to(DEV))
    _close(y, c["plain"]["y"], 4 * shape[1], "y")


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_fused_nchw_and_channels_last(shape):
    from feature_intertwiner_amd.conv import convt_bn_act
    c = _case(shape)
    conv, bn = _modules(c, shape)
    with torch.no_grad():
        y = convt_bn_act(c["x"].to(DEV), conv, bn, relu=True)
        ycl = convt_bn_act(c["x"].to(DEV), conv, bn, relu=True, channels_last_out=True)
    _close(y, c["fused"]["y"], 4 * shape[1], "y fused")
    assert y.is_contiguous() and ycl.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(ycl.contiguous(), y), "channels-last and NCHW outputs differ"


@pytest.mark.parametrize("shape", SHAPES)
def test_backward_plain(shape):
    N, Cin, Cout, H, W = shape
    c = _case(shape)
    conv, _ = _modules(c, shape)
    x = c["x"].to(DEV).requires_grad_(True)
    conv(x).backward(c["gy"].to(DEV))
    r = c["plain"]
    _close(x.grad, r["dx"], 9 * Cout, "dx")
    _close(conv.weight.grad, r["dw"], N * H * W, "dw")
    _close(conv.bias.grad, r["db"], 4 * N * H * W, "dbias")


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_backward_fused(shape, channels_last):
    from feature_intertwiner_amd.conv import convt_bn_act
    N, Cin, Cout, H, W = shape
    c = _case(shape)
    conv, bn = _modules(c, shape)
    x = c["x"].to(DEV).requires_grad_(True)
    y = convt_bn_act(x, conv, bn, relu=True, channels_last_out=channels_last)
    gy = c["gy"].to(DEV)
    y.backward(gy.contiguous(memory_format=torch.channels_last) if channels_last else gy)
    r = c["fused"]
    _close(x.grad, r["dx"], 9 * Cout, "dx")
    _close(conv.weight.grad, r["dw"], N * H * W, "dw")
    _close(conv.bias.grad, r["db"], 4 * N * H * W, "dbias")
    _close(bn.weight.grad, r["dgamma"], 4 * N * H * W, "dgamma")
    _close(bn.bias.grad, r["dbeta"], 4 * N * H * W, "dbeta")


@pytest.mark.parametrize("shape", [(1, 16, 8, 1, 1), (2, 16, 24, 5, 7)])
def test_exact_known_answer(shape):
    """x integers in [-2, 2], w in {-1, 0, 1}, Cin = 16: every partial sum is an integer below 2^24, exact in fp32."""
    from feature_intertwiner_amd.conv import ConvTranspose3x3
    N, Cin, Cout, H, W = shape
    g = torch.Generator().manual_seed(11)
    x = torch.randint(-2, 3, (N, Cin, H, W), generator=g).float()
    w = torch.randint(-1, 2, (Cin, Cout, 3, 3), generator=g).float()
    b = torch.randint(-3, 4, (Cout,), generator=g).float()
    ref = F.conv_transpose2d(x.double(), w.double(), b.double(), stride=2, padding=1, output_padding=1)
    conv = ConvTranspose3x3(Cin, Cout, kernel_size=3, stride=2, padding=1, output_padding=1)
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
        y = conv.to(DEV)(x.to(DEV))
    assert torch.equal(y.cpu().double(), ref)


@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_and_composition_agree(shape):
    """Both native routes: the fused kernel takes the eligible shapes (and only those); the four-class composition of
    existing kernels computes the same values within the forward tolerance."""
    from feature_intertwiner_amd import conv as C
    N, Cin, Cout, H, W = shape
    assert C.load_convt().fi_conv_transpose3x3s2_eligible(N, Cin, H, W, Cout, 0, None, None) == (shape in ELIGIBLE)
    c = _case(shape)
    conv, bn = _modules(c, shape)
    x = c["x"].to(DEV)
    with torch.no_grad():
        y = C.convt_bn_act(x, conv, bn, relu=True)
        C.CONVT_COMPOSE_ONLY = True
        try:
            yc = C.convt_bn_act(x, conv, bn, relu=True)
        finally:
            C.CONVT_COMPOSE_ONLY = False
    _close(yc, c["fused"]["y"], 4 * Cin, "y composition")
    d = (y - yc).abs().max().item()
    assert d <= _tol(c["fused"]["y"], 4 * Cin), d


def test_determinism_and_placement():
    """Two runs are bit-equal, and one image repeated three times in a batch gives three bit-equal outputs: an element's
    bits do not depend on where its tile sits in the grid or the batch."""
    from feature_intertwiner_amd.conv import convt_bn_act
    shape = (3, 48, 136, 9, 33)
    c = _case(shape)
    conv, bn = _modules(c, shape)
    x = c["x"][1:2].expand(3, -1, -1, -1).contiguous().to(DEV)
    with torch.no_grad():
        for cl in (False, True):
            y1 = convt_bn_act(x, conv, bn, relu=False, channels_last_out=cl)
            y2 = convt_bn_act(x, conv, bn, relu=False, channels_last_out=cl)
            assert torch.equal(y1, y2)
            assert torch.equal(y1[0], y1[1]) and torch.equal(y1[0], y1[2])
    _close(y1[:1], F.batch_norm(F.conv_transpose2d(c["x"][1:2].double(), c["w"].double(), c["b"].double(), stride=2,
                                                   padding=1, output_padding=1), c["mean"].double(), c["var"].double(),
                                c["gamma"].double(), c["beta"].double(), False, 0.0, EPS), 4 * 48, "y of the repeated image")


def test_stride1_geometry():
    """kernel 3 / stride 1 / padding 1 / output_padding 0: an ordinary 3x3 convolution with the weight transposed and
    flipped (the generator of an OptTrans whose two maps have one size)."""
    from feature_intertwiner_amd.conv import ConvTranspose3x3
    N, Cin, Cout, H, W = 2, 16, 24, 6, 6
    g = torch.Generator().manual_seed(5)
    x, w, b = torch.randn(N, Cin, H, W, generator=g), torch.randn(Cin, Cout, 3, 3, generator=g), torch.randn(Cout, generator=g)
    gy = torch.randn(N, Cout, H, W, generator=g)
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
    yd = F.conv_transpose2d(xd, wd, bd, stride=1, padding=1)
    yd.backward(gy.double())
    conv = ConvTranspose3x3(Cin, Cout, kernel_size=3, stride=1, padding=1)
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
    conv = conv.to(DEV)
    xg = x.to(DEV).requires_grad_(True)
    y = conv(xg)
    y.backward(gy.to(DEV))
    _close(y, yd.detach(), 9 * Cin, "y")
    _close(xg.grad, xd.grad, 9 * Cout, "dx")
    _close(conv.weight.grad, wd.grad, N * H * W, "dw")
    _close(conv.bias.grad, bd.grad, N * H * W, "dbias")


def test_c_entry_point_on_raw_pointers():
    from feature_intertwiner_amd import _lib
    from feature_intertwiner_amd.conv import load_convt
    shape = (2, 32, 24, 5, 7)
    N, Cin, Cout, H, W = shape
    c = _case(shape)
    L = load_convt()
    x, w, b = (c[k].to(DEV).contiguous() for k in ("x", "w", "b"))
    y = torch.full((N, Cout, 2 * H, 2 * W), float("nan"), device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.fi_conv_transpose3x3s2_eligible(N, Cin, H, W, Cout, 0, p(x), p(y)) == 1
    assert L.fi_conv_transpose3x3s2_forward(p(x), p(w), p(b), None, p(y), N, Cin, H, W, Cout, 0, 0, st) == 0
    torch.cuda.synchronize()
    _close(y, c["plain"]["y"], 4 * Cin, "y (C entry)")
    # channels-last through the same entry: the same bits
    ycl = torch.full((N, 2 * H, 2 * W, Cout), float("nan"), device=DEV)
    assert L.fi_conv_transpose3x3s2_forward(p(x), p(w), p(b), None, p(ycl), N, Cin, H, W, Cout, 0, 1, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(ycl.permute(0, 3, 1, 2).contiguous(), y)
    # invalid arguments: a status before anything is launched, y untouched
    before = y.clone()
    assert L.fi_conv_transpose3x3s2_forward(None, p(w), p(b), None, p(y), N, Cin, H, W, Cout, 0, 0, st) == -1
    assert L.fi_conv_transpose3x3s2_forward(p(x), p(w), p(b), None, p(y), N, Cin, 0, W, Cout, 0, 0, st) == -1
    assert L.fi_conv_transpose3x3s2_forward(p(x), p(w), p(b), None, p(y), N, 12, H, W, Cout, 0, 0, st) == -3
    assert b"Cin % 16" in _lib.load().fi_last_error()
    assert L.fi_conv_transpose3x3s2_forward(p(x), p(w), p(b), None, ctypes.c_void_p(y.data_ptr() + 4), N, Cin, H, W, Cout,
                                            0, 0, st) == -3
    assert L.fi_conv_transpose3x3s2_forward(p(x), p(w), p(b), None, p(ycl), N, Cin, H, W, 22, 0, 1, st) == -3
    torch.cuda.synchronize()
    assert torch.equal(y, before)


def test_dev_make_up_maps_upsample_fac_2():
    """Dev.make_up_maps at DEV.UPSAMPLE_FAC = 2 (eval BN with non-trivial running statistics) against the stock
    ConvTranspose2d -> BatchNorm2d -> ReLU sequence in float64 carrying the same state dict; channels-last output."""
    from feature_intertwiner_amd.config import make_config
    from feature_intertwiner_amd.conv import ConvTranspose3x3
    from feature_intertwiner_amd.sub_module import Dev
    torch.manual_seed(4)
    cfg = make_config(backbone="resnet50", image_size=256, batch_size=2, train_rois_per_image=48)
    cfg.DEV.UPSAMPLE_FAC = 2.0
    assert cfg.ROIS.METHOD == 'roi_align'
    dev = Dev(cfg, 256)
    seq = dev.upsample[0]
    assert isinstance(seq[0], ConvTranspose3x3)
    with torch.no_grad():
        seq[0].weight.normal_()
        seq[0].bias.normal_()
        seq[1].weight.uniform_(0.5, 1.5)
        seq[1].bias.normal_()
        seq[1].running_mean.normal_()
        seq[1].running_var.uniform_(0.5, 2.0)
    stock = nn.Sequential(nn.ConvTranspose2d(256, 256, kernel_size=3, stride=2, padding=1, output_padding=1),
                          nn.BatchNorm2d(256), nn.ReLU())
    stock.load_state_dict(seq.state_dict())
    stock = stock.double().eval()
    dev = dev.to(DEV).eval()
    maps = [torch.randn(2, 256, 8, 8), torch.randn(1, 256, 4, 4)]
    with torch.no_grad():
        out = dev.make_up_maps([m.to(DEV) for m in maps])
        ref = [stock(m.double()) for m in maps]
    for o, r in zip(out, ref):
        assert o.is_contiguous(memory_format=torch.channels_last)
        _close(o, r, 4 * 256, "make-up map %s" % (tuple(r.shape),))
