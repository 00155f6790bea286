"""The ResNet trunk on 16-bit channels-last tensors (MODEL.ACT_PRECISION, feature_intertwiner_amd/act16.py): one block, the
whole trunk, the whole model.

Block.  An identity and a stride-2 projection Bottleneck on a 2 x 256 x 9 x 7 input: the module's output is bit-equal to the
same block chained by hand from conv_bn_act16 calls, and EVERY one of those calls is held to the bar of
tests/test_gpu_act16_conv.py against float64 computed from the GPU's own previous 16-bit output -- each layer is checked on
its own and no tolerance accumulates.

Trunk.  ResNet-50 with stage 5 on 2 x 3 x 64 x 64, seeded (conv weights N(0, 2 / fan_in); BatchNorm gamma in [0.75, 1.25],
beta and mean 0.1 N(0, 1), variance in [0.5, 1.5]; gamma halved for every bn3 and projection BatchNorm so the residual sum
does not grow).  The reference is a float64 replica on stock F.conv2d carrying the same state dict.  Per level c2..c5 the
relative Frobenius error of the 16-bit trunk, e_act, and of the existing 16-bit-operand path on fp32 tensors
(conv precision bf16 / fp16), e_old, are taken against THAT reference in the same test, and e_act <= 1.5 e_old is required.
The margin is not fitted to the kernel: a CPU emulation of both roundings gave e_old 4.1e-3 .. 7.3e-3 and e_act 5.0e-3 ..
8.5e-3 for bf16 (ratios 1.14 .. 1.22; fp16 1.14 .. 1.20) -- the extra rounding per block is the shortcut read -- and a wrong
layer gives an error of order 1.

Model.  MaskRCNN (resnet50, 256^2) with ACT_PRECISION = 'bf16' in inference: reference shapes, finite values, and
act16.stats() shows 52 conv (16 blocks x 3 + 4 projections), 1 pack and 4 unpack launches; mode='train' raises
NotImplementedError; with ACT_PRECISION absent the counters stay 0 and two runs are bit-equal."""
import math

import pytest
import torch
import torch.nn.functional as F

import fp64_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRECISIONS = {"bf16": (torch.bfloat16, 2.0 ** -8, 0.0), "fp16": (torch.float16, 2.0 ** -11, 2.0 ** -25)}


def _randomise(module, seed):
    """Seeded parameters and running statistics as the module docstring states them."""
    import torch.nn as nn
    g = torch.Generator().manual_seed(seed)
    for name, m in module.named_modules():
        if isinstance(m, nn.Conv2d):
            fan_in = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
            m.weight.data.copy_(torch.randn(m.weight.shape, generator=g) * math.sqrt(2.0 / fan_in))
            if m.bias is not None:
                m.bias.data.copy_(0.01 * torch.randn(m.bias.shape, generator=g))
        elif isinstance(m, nn.BatchNorm2d):
            halve = name.endswith("bn3") or ".downsample." in name or name.startswith("downsample.")
            m.weight.data.copy_((0.75 + 0.5 * torch.rand(m.weight.shape, generator=g)) * (0.5 if halve else 1.0))
            m.bias.data.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
            m.running_mean.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
            m.running_var.copy_(0.5 + torch.rand(m.bias.shape, generator=g))
    return module.eval()


def _check_call(x16, conv, bn, relu, residual, y16, prec, what):
    """One conv_bn_act16 call against float64 from ITS OWN 16-bit inputs, every element, the derived bar."""
    from feature_intertwiner_amd import conv as C
    dtype, unit, sub = PRECISIONS[prec]
    scale, shift = C._cached_fold(conv, bn)
    w16 = conv.weight.detach().to(dtype)
    acc = R.conv_ref(x16, w16, conv.stride, conv.padding)
    acc_abs = R.conv_ref(x16.abs(), w16.abs(), conv.stride, conv.padding)
    ref = R.epilogue(acc, scale, shift, residual, relu)
    mag = R.abs_epilogue(acc_abs, scale, shift, residual)
    n = conv.weight.shape[1] * conv.weight.shape[2] * conv.weight.shape[3]
    B = R.U * (4.0 * math.sqrt(n) + 16.0) * mag
    allow = B + unit * (ref.abs() + B) + sub
    got = y16.to(torch.float64)
    assert tuple(got.shape) == tuple(ref.shape), what
    d = torch.where(torch.isfinite(got), (got - ref).abs(), torch.full_like(ref, float("inf")))
    worst = float((d / allow).max())
    print("%s %s: worst |d| / bar = %.3f" % (what, prec, worst))
    assert worst <= 1.0, (what, worst)


@pytest.mark.parametrize("prec", sorted(PRECISIONS))
@pytest.mark.parametrize("kind", ["identity", "projection_stride2"])
def test_block_equals_its_hand_chained_layers_and_each_layer_holds_the_bar(kind, prec):
    from feature_intertwiner_amd import _lib, act16
    from feature_intertwiner_amd.conv import Conv2d
    from feature_intertwiner_amd.sub_module import Bottleneck, _bn
    import torch.nn as nn
    dtype = PRECISIONS[prec][0]
    if kind == "identity":
        block = Bottleneck(256, 64)
    else:
        block = Bottleneck(256, 128, 2, nn.Sequential(Conv2d(256, 512, kernel_size=1, stride=2), _bn(512)))
    block = _randomise(block, 11).to(DEV)
    x = torch.randn((2, 256, 9, 7), generator=torch.Generator().manual_seed(5)).to(DEV)
    with torch.no_grad():
        x16 = act16.pack(x, dtype)
        act16.reset_stats()
        out = block(x16)
        assert act16.stats()["conv"] == (3 if kind == "identity" else 4)
        assert out.dtype is dtype and out.is_contiguous(memory_format=torch.channels_last)
        assert tuple(out.shape) == ((2, 256, 9, 7) if kind == "identity" else (2, 512, 5, 4))
        a = act16.conv_bn_act16(x16, block.conv1, block.bn1, relu=True)
        _check_call(x16, block.conv1, block.bn1, True, None, a, prec, kind + " conv1")
        b = act16.conv_bn_act16(a, block.conv2, block.bn2, relu=True)
        _check_call(a, block.conv2, block.bn2, True, None, b, prec, kind + " conv2")
        res = x16
        if block.downsample is not None:
            res = act16.conv_bn_act16(x16, block.downsample[0], block.downsample[1], relu=False)
            _check_call(x16, block.downsample[0], block.downsample[1], False, None, res, prec, kind + " projection")
        c = act16.conv_bn_act16(b, block.conv3, block.bn3, relu=True, residual=res)
        _check_call(b, block.conv3, block.bn3, True, res, c, prec, kind + " conv3")
        assert torch.equal(out.view(torch.int16), c.view(torch.int16))
        assert bool(torch.isfinite(out.float()).all()) and float(out.float().abs().max()) > 0.1
    # what the path refuses is an error, never another path
    with pytest.raises(_lib.FiError):
        act16.conv_bn_act16(x16, block.conv1, block.bn1)                    # grad mode enabled
    with torch.no_grad():
        block.bn1.train()
        with pytest.raises(_lib.FiError):
            act16.conv_bn_act16(x16, block.conv1, block.bn1)                # a training-mode BatchNorm
        block.bn1.eval()
        odd = _randomise(Conv2d(256, 20, kernel_size=1), 3).to(DEV)         # Cout % 8 != 0: the library's query says no
        with pytest.raises(_lib.FiError):
            act16.conv_bn_act16(x16, odd, _randomise(_bn(20), 4).to(DEV))


# ---- the float64 replica of the trunk on stock F.conv2d ---------------------------------------------------------------
def _bn64(x, sd, name, eps):
    g, b, m, v = (sd[name + k].double() for k in (".weight", ".bias", ".running_mean", ".running_var"))
    s = g / torch.sqrt(v + eps)
    return x * s.view(1, -1, 1, 1) + (b - m * s).view(1, -1, 1, 1)


def _conv64(x, sd, name, stride, pad):
    return F.conv2d(x, sd[name + ".weight"].double(), sd[name + ".bias"].double(), stride=stride, padding=pad)


def _trunk64(resnet, images):
    sd = {k: v.detach().cpu() for k, v in resnet.state_dict().items()}
    eps = resnet.C1[1].eps
    x = F.relu(_bn64(_conv64(images.double(), sd, "C1.0", 2, 3), sd, "C1.1", eps))
    x = F.max_pool2d(F.pad(x, resnet.C1[3].pads(x.shape[2], x.shape[3])), 3, 2)      # SamePad2d(3, 2): 1 right, 1 bottom
    out = []
    for stage_name in ("C2", "C3", "C4", "C5"):
        stage = getattr(resnet, stage_name)
        for i, block in enumerate(stage):
            p = "%s.%d." % (stage_name, i)
            y = F.relu(_bn64(_conv64(x, sd, p + "conv1", block.stride, 0), sd, p + "bn1", eps))
            y = F.relu(_bn64(_conv64(y, sd, p + "conv2", 1, 1), sd, p + "bn2", eps))
            y = _bn64(_conv64(y, sd, p + "conv3", 1, 0), sd, p + "bn3", eps)
            r = x
            if block.downsample is not None:
                r = _bn64(_conv64(x, sd, p + "downsample.0", block.stride, 0), sd, p + "downsample.1", eps)
            x = F.relu(y + r)
        out.append(x)
    return out


@pytest.mark.parametrize("prec", sorted(PRECISIONS))
def test_trunk_is_as_close_to_float64_as_the_existing_16bit_path(prec):
    """Measured on an MI355X (e_old -> e_act per level c2..c5; the test prints them; float64 maxima 13.0 / 16.9 / 27.0 / 22.2):
    bf16  4.40e-3 -> 5.23e-3, 6.07e-3 -> 7.09e-3, 6.87e-3 -> 7.96e-3, 7.82e-3 -> 8.49e-3: ratios 1.19 1.17 1.16 1.09
    fp16  5.71e-4 -> 6.74e-4, 7.78e-4 -> 8.88e-4, 8.23e-4 -> 9.63e-4, 9.01e-4 -> 1.07e-3: ratios 1.18 1.14 1.17 1.19"""
    from feature_intertwiner_amd import act16
    from feature_intertwiner_amd import conv as C
    from feature_intertwiner_amd.sub_module import ResNet, _pad_maxpool
    dtype = PRECISIONS[prec][0]
    resnet = _randomise(ResNet("resnet50", stage5=True), 2024)
    images = torch.randn((2, 3, 64, 64), generator=torch.Generator().manual_seed(9))
    ref = _trunk64(resnet, images)
    assert [tuple(r.shape) for r in ref] == [(2, 256, 16, 16), (2, 512, 8, 8), (2, 1024, 4, 4), (2, 2048, 2, 2)]
    print("float64 maxima c2..c5:", ["%.1f" % float(r.abs().max()) for r in ref])
    assert all(float(r.abs().max()) < 1000.0 for r in ref)                  # fp16-safe
    resnet = resnet.to(DEV)
    stages = [resnet.C2, resnet.C3, resnet.C4, resnet.C5]
    prev = C.conv_precision()
    C.set_conv_precision(prec)
    try:
        with torch.no_grad():
            x = C.conv_bn_act(images.to(DEV), resnet.C1[0], resnet.C1[1], relu=True)
            x = _pad_maxpool(x, resnet.C1[3], resnet.C1[4])
            old, m = [], x
            for stage in stages:                                            # the existing path: 16-bit operands, fp32 tensors
                m = stage(m)
                old.append(m)
            act16.reset_stats()
            new, m = [], act16.pack(x, dtype)
            for stage in stages:
                m = stage(m)
                new.append(act16.unpack(m))
            assert act16.stats() == {"conv": 52, "pack": 1, "unpack": 4}
    finally:
        C.set_conv_precision(prev)
    err = lambda t, r: float((t.double().cpu() - r).norm() / r.norm())
    for lvl, (o, n_, r) in enumerate(zip(old, new, ref), start=2):
        assert o.dtype is torch.float32 and n_.dtype is torch.float32 and tuple(n_.shape) == tuple(r.shape)
        e_old, e_act = err(o, r), err(n_, r)
        print("%s c%d: e_old %.3e  e_act %.3e  ratio %.3f" % (prec, lvl, e_old, e_act, e_act / e_old))
        assert e_old > 0.0 and e_old < 0.05, (lvl, e_old)                   # the yardstick itself is the 16-bit path
        assert e_act <= 1.5 * e_old, (lvl, e_act, e_old)


def _model(act=None):
    from feature_intertwiner_amd.config import make_config
    from feature_intertwiner_amd.model import MaskRCNN
    from feature_intertwiner_amd.synthetic import SyntheticProposals, synthetic_batch
    torch.manual_seed(1)
    cfg = make_config(backbone="resnet50", image_size=256, batch_size=2)
    if act is not None:
        cfg.MODEL.ACT_PRECISION = act
    model = MaskRCNN(cfg).to(DEV)
    batch = synthetic_batch(2, 256, device=DEV)
    model.external_proposals = SyntheticProposals(batch[2], 256, cycle=1)      # the same rows at every call
    windows = torch.tensor([[0, 0, 256, 256], [0, 16, 256, 240]], dtype=torch.float32)
    return model, batch, windows


def test_model_inference_runs_the_trunk_on_16bit_tensors():
    from feature_intertwiner_amd import act16
    model, batch, windows = _model("bf16")
    act16.reset_stats()
    det, masks = model([batch[0], windows], mode='inference')
    assert det.shape == (2, 100, 6) and masks.shape == (2, 100, 81, 28, 28)
    assert det.dtype is torch.float32 and masks.dtype is torch.float32
    assert bool(torch.isfinite(det).all()) and bool(torch.isfinite(masks).all())
    assert act16.stats() == {"conv": 52, "pack": 1, "unpack": 4}            # 16 blocks x 3 + 4 projections
    with pytest.raises(NotImplementedError, match="training"):
        model(list(batch), mode='train')


def test_without_the_switch_nothing_changes():
    from feature_intertwiner_amd import act16
    model, batch, windows = _model(None)
    assert not hasattr(model.config.MODEL, "ACT_PRECISION")
    act16.reset_stats()
    det, masks = model([batch[0], windows], mode='inference')
    det2, masks2 = model([batch[0], windows], mode='inference')
    assert act16.stats() == {"conv": 0, "pack": 0, "unpack": 0}
    assert torch.equal(det, det2) and torch.equal(masks, masks2)
    assert det.shape == (2, 100, 6) and masks.shape == (2, 100, 81, 28, 28)
