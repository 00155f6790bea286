"""The feature pyramid and the RPN on 16-bit channels-last tensors (MODEL.ACT_SCOPE = 'pyramid' next to a 16-bit
MODEL.ACT_PRECISION; feature_intertwiner_amd/pyr16.py): the FPN module, its accuracy, the RPN module, the whole model.

FPN.  ResNet-50 stages with stage 5 on 2 x 3 x 64 x 64, seeded as tests/test_gpu_act16_trunk.py seeds its trunk (conv weights
N(0, 2 / fan_in), conv biases 0.01 N(0, 1); BatchNorm gamma in [0.75, 1.25], beta and mean 0.1 N(0, 1), variance in
[0.5, 1.5]; gamma halved for every bn3 and projection BatchNorm).  FPN.forward returns five 16-bit channels-last maps that
are bit-equal to the same launches chained by hand, p6 is p5[:, :, ::2, ::2], and the counters show 3 lateral launches, no
head launch, 52 + 1 + 4 convolutions, 1 pack and NO unpack.

Accuracy.  The reference is a float64 replica of trunk, pyramid and RPN on stock F.conv2d carrying the same parameters.  Per
level, for p2..p5 and for the RPN's logits and bbox on p2..p6, the relative Frobenius error of scope 'pyramid', e_new, and of
the path as it was -- scope 'trunk' with the conv precision of the same type -- e_old, are taken against THAT reference in
the same test; 0 < e_old < 0.05 and e_new <= 1.5 e_old are required.  1.5 is the trunk test's bound: the new path adds one
store rounding per tensor (relative 2^-9 / sqrt(3) = 1.1e-3 rms for bf16, 1.4e-4 for fp16) next to an e_old of several 1e-3
(bf16) / 1e-4 (fp16).

RPN.  On a 16-bit map RPN.forward gives logits, probs, bbox in fp32 with the fp32 branch's shapes and anchor order (the
accuracy test compares them with the reference per level), in one head launch per call, and logits / bbox are views of the
head's output: no permute copy.

Model.  MaskRCNN (resnet50, 256^2) with ACT_PRECISION = 'bf16', ACT_SCOPE = 'pyramid' in inference: reference shapes, fp32,
finite; 62 = 52 + 1 + 4 + 5 convolutions, 1 pack, 4 unpack (p2..p5 for the Dev stage), 3 lateral and 5 head launches; two
runs bit-equal; mode='train' raises; with ACT_SCOPE absent pyr16's counters stay 0.

Measured on an MI355X (e_old -> e_new per level, the test prints every line; float64 maxima p2..p6 61.9 / 54.4 / 44.6 /
15.8 / 15.6):
    bf16  p2..p5 8.09e-3 -> 8.53e-3, 8.74e-3 -> 9.12e-3, 8.50e-3 -> 8.75e-3, 9.25e-3 -> 9.43e-3: ratios 1.054 1.042 1.029 1.020
          RPN logits p2..p6 ratios 1.056 1.010 1.002 1.000 1.000, bbox 1.022 1.007 1.009 1.000 1.000 (e_old 5.5e-3 .. 1.5e-2)
    fp16  p2..p5 1.03e-3 -> 1.08e-3, 1.10e-3 -> 1.14e-3, 1.06e-3 -> 1.09e-3, 1.21e-3 -> 1.23e-3: ratios 1.056 1.043 1.028 1.016
          RPN logits p2..p6 ratios 1.021 1.033 1.024 1.000 1.000, bbox 1.031 0.994 1.034 1.000 1.000 (e_old 7.3e-4 .. 2.0e-3)
On p5 / p6 the ratio is exactly 1: every tensor the old path reads there is rounded to the type on the read, which is the
value the new path stored."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRECISIONS = {"bf16": torch.bfloat16, "fp16": torch.float16}


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
            halve = name.endswith("bn3") or ".downsample." in name
            m.weight.data.copy_((0.75 + 0.5 * torch.rand(m.weight.shape, generator=g)) * (0.5 if halve else 1.0))
            m.bias.data.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
            m.running_mean.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
            m.running_var.copy_(0.5 + torch.rand(m.bias.shape, generator=g))
    return module.eval()


def _config(prec=None, scope=None):
    from feature_intertwiner_amd.config import make_config
    cfg = make_config(backbone="resnet50", image_size=256, batch_size=2)
    if prec is not None:
        cfg.MODEL.ACT_PRECISION = prec
    if scope is not None:
        cfg.MODEL.ACT_SCOPE = scope
    return cfg


def _fpn_and_rpn(cfg, seed=2024):
    from feature_intertwiner_amd.sub_module import FPN, RPN, ResNet
    fpn = _randomise(FPN(cfg, *ResNet("resnet50", stage5=True).stages(), out_channels=256), seed)
    rpn = _randomise(RPN(3, 1, 256), seed + 1)
    return fpn, rpn


# ---- the float64 replica on stock F.conv2d -----------------------------------------------------------------------------
def _conv64(x, conv, stride=None, pad=None):
    stride = conv.stride if stride is None else stride
    pad = conv.padding if pad is None else pad
    return F.conv2d(x, conv.weight.detach().double().cpu(), conv.bias.detach().double().cpu(), stride=stride, padding=pad)


def _bn64(x, bn):
    g, b, m, v = (t.detach().double().cpu() for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))
    s = g / torch.sqrt(v + bn.eps)
    return x * s.view(1, -1, 1, 1) + (b - m * s).view(1, -1, 1, 1)


def _trunk64(fpn, images):
    x = F.relu(_bn64(_conv64(images.double(), fpn.C1[0], 2, 3), fpn.C1[1]))
    x = F.max_pool2d(F.pad(x, fpn.C1[3].pads(x.shape[2], x.shape[3])), 3, 2)       # SamePad2d(3, 2): 1 right, 1 bottom
    out = []
    for stage in (fpn.C2, fpn.C3, fpn.C4, fpn.C5):
        for block in stage:
            y = F.relu(_bn64(_conv64(x, block.conv1, block.stride, 0), block.bn1))
            y = F.relu(_bn64(_conv64(y, block.conv2, 1, 1), block.bn2))
            y = _bn64(_conv64(y, block.conv3, 1, 0), block.bn3)
            r = x
            if block.downsample is not None:
                r = _bn64(_conv64(x, block.downsample[0], block.stride, 0), block.downsample[1])
            x = F.relu(y + r)
        out.append(x)
    return out


def _pyramid64(fpn, images):
    c2, c3, c4, c5 = _trunk64(fpn, images)
    up = lambda t: t.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    p5 = _conv64(c5, fpn.P5_conv1)
    p4 = _conv64(c4, fpn.P4_conv1) + up(p5)
    p3 = _conv64(c3, fpn.P3_conv1) + up(p4)
    p2 = _conv64(c2, fpn.P2_conv1) + up(p3)
    p2, p3, p4, p5 = (_conv64(p, m[1], 1, 1) for p, m in
                      ((p2, fpn.P2_conv2), (p3, fpn.P3_conv2), (p4, fpn.P4_conv2), (p5, fpn.P5_conv2)))
    return [p2, p3, p4, p5, p5[:, :, ::2, ::2]]


def _rpn64(rpn, p):
    x = F.relu(_conv64(p, rpn.conv_shared, 1, 1))
    logits = _conv64(x, rpn.conv_class).permute(0, 2, 3, 1).reshape(p.shape[0], -1, 2)
    bbox = _conv64(x, rpn.conv_bbox).permute(0, 2, 3, 1).reshape(p.shape[0], -1, 4)
    return logits, bbox


def _images():
    return torch.randn((2, 3, 64, 64), generator=torch.Generator().manual_seed(9))


@pytest.mark.parametrize("prec", sorted(PRECISIONS))
def test_fpn_returns_16bit_maps_equal_to_the_hand_chained_launches(prec):
    from feature_intertwiner_amd import act16, pyr16
    from feature_intertwiner_amd import conv as C
    from feature_intertwiner_amd.sub_module import _pad_maxpool
    dtype = PRECISIONS[prec]
    fpn, _ = _fpn_and_rpn(_config(prec, "pyramid"))
    fpn = fpn.to(DEV)
    images = _images().to(DEV)
    with torch.no_grad():
        act16.reset_stats()
        pyr16.reset_stats()
        out = fpn(images, mode='inference')
        assert pyr16.stats() == {"lateral": 3, "head": 0}
        assert act16.stats() == {"conv": 52 + 1 + 4, "pack": 1, "unpack": 0}
        assert len(out) == 6
        maps, ot_loss = out[:5], out[5]
        assert tuple(ot_loss.shape) == (2, 3) and ot_loss.dtype is torch.float32 and not bool(ot_loss.any())
        for m, side in zip(maps, (16, 8, 4, 2, 1)):
            assert tuple(m.shape) == (2, 256, side, side) and m.dtype is dtype
            assert m.is_contiguous(memory_format=torch.channels_last)
            assert bool(torch.isfinite(m.float()).all())
        assert float(maps[0].float().abs().max()) > 0.1
        assert torch.equal(maps[4], maps[3][:, :, ::2, ::2])
        # the same launches by hand
        x = C.conv_bn_act(images, fpn.C1[0], fpn.C1[1], relu=True)
        m = act16.pack(_pad_maxpool(x, fpn.C1[3], fpn.C1[4]), dtype)
        c = []
        for stage in (fpn.C2, fpn.C3, fpn.C4, fpn.C5):
            m = stage(m)
            c.append(m)
        p5 = pyr16.conv_bias_act16(c[3], fpn.P5_conv1)
        p4 = pyr16.lateral16(c[2], fpn.P4_conv1, p5)
        p3 = pyr16.lateral16(c[1], fpn.P3_conv1, p4)
        p2 = pyr16.lateral16(c[0], fpn.P2_conv1, p3)
        hand = [pyr16.conv_bias_act16(p, s[1]) for p, s in
                ((p2, fpn.P2_conv2), (p3, fpn.P3_conv2), (p4, fpn.P4_conv2), (p5, fpn.P5_conv2))]
        for lvl, (a, b) in enumerate(zip(maps[:4], hand), start=2):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), lvl
        # train mode is refused, with or without the scope
        with pytest.raises(NotImplementedError, match="training"):
            fpn(images, mode='train')


@pytest.mark.parametrize("prec", sorted(PRECISIONS))
def test_pyramid_and_rpn_are_as_close_to_float64_as_the_existing_path(prec):
    from feature_intertwiner_amd import pyr16
    from feature_intertwiner_amd import conv as C
    cfg = _config(prec, "trunk")
    fpn, rpn = _fpn_and_rpn(cfg)
    images = _images()
    ref_p = _pyramid64(fpn, images)
    ref_rpn = [_rpn64(rpn, p) for p in ref_p]
    assert [tuple(r.shape) for r in ref_p] == [(2, 256, s, s) for s in (16, 8, 4, 2, 1)]
    print("float64 maxima p2..p6:", ["%.1f" % float(r.abs().max()) for r in ref_p])
    assert all(float(r.abs().max()) < 1000.0 for r in ref_p)               # fp16-safe
    fpn, rpn = fpn.to(DEV), rpn.to(DEV)
    prev = C.conv_precision()
    C.set_conv_precision(prec)
    try:
        with torch.no_grad():
            old_p = fpn(images.to(DEV), mode='inference')[:5]              # the path as it was: fp32 maps behind c2..c5
            old_rpn = [rpn(p) for p in old_p]
            cfg.MODEL.ACT_SCOPE = "pyramid"
            pyr16.reset_stats()
            new_p = fpn(images.to(DEV), mode='inference')[:5]
            new_rpn = [rpn(p) for p in new_p]
            assert pyr16.stats() == {"lateral": 3, "head": 5}
    finally:
        C.set_conv_precision(prev)
    err = lambda t, r: float((t.double().cpu() - r).norm() / r.norm())

    def hold(what, o, n_, r):
        assert tuple(o.shape) == tuple(r.shape) and tuple(n_.shape) == tuple(r.shape), what
        e_old, e_new = err(o, r), err(n_, r)
        print("%s %s: e_old %.3e  e_new %.3e  ratio %.3f" % (prec, what, e_old, e_new, e_new / e_old))
        assert e_old > 0.0 and e_old < 0.05, (what, e_old)                  # the yardstick itself is the 16-bit path
        assert e_new <= 1.5 * e_old, (what, e_new, e_old)

    for lvl in range(4):
        assert old_p[lvl].dtype is torch.float32 and new_p[lvl].dtype is PRECISIONS[prec]
        hold("p%d" % (lvl + 2), old_p[lvl], new_p[lvl].float(), ref_p[lvl])
    for lvl in range(5):
        (lo, po, bo), (ln, pn, bn), (lr, br) = old_rpn[lvl], new_rpn[lvl], ref_rpn[lvl]
        for t in (ln, pn, bn):
            assert t.dtype is torch.float32
        assert tuple(pn.shape) == tuple(po.shape)
        hold("rpn logits on p%d" % (lvl + 2), lo, ln, lr)
        hold("rpn bbox on p%d" % (lvl + 2), bo, bn, br)
        assert torch.equal(pn, torch.softmax(ln, dim=2))


@pytest.mark.parametrize("prec", sorted(PRECISIONS))
def test_rpn_on_a_16bit_map_is_one_head_launch_and_makes_no_permute_copy(prec):
    from feature_intertwiner_amd import _lib, act16, pyr16
    from feature_intertwiner_amd.sub_module import RPN
    rpn = _randomise(RPN(3, 1, 256), 77).to(DEV)
    x = torch.randn((2, 256, 6, 10), generator=torch.Generator().manual_seed(3)).to(DEV)
    with torch.no_grad():
        x16 = act16.pack(x, PRECISIONS[prec])
        act16.reset_stats()
        pyr16.reset_stats()
        logits, probs, bbox = rpn(x16)
        assert pyr16.stats() == {"lateral": 0, "head": 1}
        assert act16.stats() == {"conv": 1, "pack": 0, "unpack": 0}
        ref = rpn(x16.float().contiguous())                                  # the fp32 branch on the same (rounded) map
    for t, r in zip((logits, probs, bbox), ref):
        assert t.dtype is torch.float32 and tuple(t.shape) == tuple(r.shape)
        assert float((t - r).norm() / r.norm()) < 0.02                       # the same anchors in the same order
    assert tuple(logits.shape) == (2, 6 * 10 * 3, 2) and tuple(bbox.shape) == (2, 6 * 10 * 3, 4)
    # logits and bbox are views of the head's [N, H, W, 6A] fp32 output: one storage of exactly that size
    store = bbox.untyped_storage()
    assert store.data_ptr() == logits.untyped_storage().data_ptr()
    assert store.nbytes() == 2 * 6 * 10 * 18 * 4
    assert bbox.storage_offset() == 2 and logits.storage_offset() == 0
    assert tuple(bbox.stride()) == (6 * 10 * 18, 6, 1) and tuple(logits.stride()) == (6 * 10 * 18, 6, 1)
    # a stride-2 RPN on a 16-bit map is an error, not another path
    rpn2 = _randomise(RPN(3, 2, 256), 78).to(DEV)
    with torch.no_grad(), pytest.raises(_lib.FiError, match="anchor_stride"):
        rpn2(x16)


def _model(act=None, scope=None):
    from feature_intertwiner_amd.model import MaskRCNN
    from feature_intertwiner_amd.synthetic import SyntheticProposals, synthetic_batch
    torch.manual_seed(1)
    model = MaskRCNN(_config(act, scope)).to(DEV)
    batch = synthetic_batch(2, 256, device=DEV)
    model.external_proposals = SyntheticProposals(batch[2], 256, cycle=1)      # the same rows at every call
    windows = torch.tensor([[0, 0, 256, 256], [0, 16, 256, 240]], dtype=torch.float32)
    return model, batch, windows


def test_model_inference_runs_pyramid_and_rpn_on_16bit_tensors():
    from feature_intertwiner_amd import act16, pyr16
    model, batch, windows = _model("bf16", "pyramid")
    act16.reset_stats()
    pyr16.reset_stats()
    det, masks = model([batch[0], windows], mode='inference')
    assert act16.stats() == {"conv": 62, "pack": 1, "unpack": 4}            # 52 trunk + P5_conv1 + 4 smoothing + 5 shared
    assert pyr16.stats() == {"lateral": 3, "head": 5}
    assert det.shape == (2, 100, 6) and masks.shape == (2, 100, 81, 28, 28)
    assert det.dtype is torch.float32 and masks.dtype is torch.float32
    assert bool(torch.isfinite(det).all()) and bool(torch.isfinite(masks).all())
    det2, masks2 = model([batch[0], windows], mode='inference')
    assert torch.equal(det, det2) and torch.equal(masks, masks2)
    with pytest.raises(NotImplementedError, match="training"):
        model(list(batch), mode='train')


def test_without_the_scope_no_pyr16_kernel_runs():
    from feature_intertwiner_amd import pyr16
    model, batch, windows = _model("bf16", None)
    assert not hasattr(model.config.MODEL, "ACT_SCOPE")
    pyr16.reset_stats()
    det, masks = model([batch[0], windows], mode='inference')
    assert pyr16.stats() == {"lateral": 0, "head": 0}
    assert det.shape == (2, 100, 6) and masks.shape == (2, 100, 81, 28, 28)
