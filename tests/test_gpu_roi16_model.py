"""The Dev stage's make-up layer and RoIAlign on 16-bit channels-last pyramid maps (MODEL.ACT_SCOPE = 'roi' next to a 16-bit
MODEL.ACT_PRECISION; feature_intertwiner_amd/roi16.py): the Dev module, its accuracy, the whole model.

Dev.  Dev of make_config(resnet50, 256, batch 2), seeded as tests/test_gpu_pyr16_model.py seeds its modules (conv weights
N(0, 2 / fan_in), conv biases 0.01 N(0, 1); BatchNorm gamma in [0.75, 1.25], beta and mean 0.1 N(0, 1), variance in
[0.5, 1.5]), in eval().  Inputs: seeded N(0, 1) 16-bit p2..p5 of 2 x 256 x {64, 32, 16, 8}^2 and 2 x 64 fixed seeded RoIs that
span all four levels.  make_up_maps returns four 16-bit channels-last maps, each bit-equal to conv_bn_act16 called by hand;
one Dev call shows 4 convolutions, 2 crops and no unpack.

Accuracy.  The reference is a float64 replica: F.conv2d, BatchNorm, ReLU on the widened maps, then a float64 bilinear crop
with the oracle's tap indices and fractions.  Against it, the relative Frobenius error of the 7x7 and the 14x14 crops under
the new path, e_new, and under the path as it was -- unpack, conv_bn_act with the CONV_PRECISION of the same type, the fp32
crop -- e_old; 0 < e_old < 0.05 and e_new <= 1.5 e_old are required.  1.5 is the bound of the trunk and pyramid tests: the
new path adds ONE store rounding, the make-up map's (relative 2^-9 / sqrt(3) rms for bf16, 2^-12 / sqrt(3) for fp16), which
RoIAlign's convex interpolation does not amplify, next to an e_old that carries the rounding of the same map's inputs and
weights.

Model.  MaskRCNN (resnet50, 256^2, batch 2) with ACT_PRECISION = 'bf16', ACT_SCOPE = 'roi' in inference: reference shapes,
fp32, finite; 1 pack and 0 unpack; the convolution count of scope 'pyramid' (taken in the same test) plus 4 -- the make-up
pass runs once --; 4 crops with DEV.SWITCH on and with it off; 3 lateral and 5 head launches; two runs bit-equal; fp16 runs;
mode='train' and DEV.UPSAMPLE_FAC = 2 raise; under 'pyramid' (4 unpacks) and without a scope roi16's counter stays 0.

Measured on an MI355X (e_old -> e_new, the test prints every line):
    bf16  crops 7x7 1.391e-3 -> 1.972e-3 (ratio 1.418), 14x14 1.397e-3 -> 1.979e-3 (1.416)
    fp16  crops 7x7 1.751e-4 -> 2.471e-4 (ratio 1.412), 14x14 1.757e-4 -> 2.481e-4 (1.412)
The ratio is sqrt(2): the N(0, 1) inputs are values of the type already, so the old path's error is the rounding of the
weights alone (its fp32 map is not rounded), and the new path adds one independent rounding of the same size at the store."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRECISIONS = {"bf16": torch.bfloat16, "fp16": torch.float16}
SIDES = (64, 32, 16, 8)


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
            m.weight.data.copy_(0.75 + 0.5 * torch.rand(m.weight.shape, generator=g))
            m.bias.data.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
            m.running_mean.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
            m.running_var.copy_(0.5 + torch.rand(m.bias.shape, generator=g))
    return module.eval()


def _config(prec=None, scope=None, **kw):
    from feature_intertwiner_amd.config import make_config
    cfg = make_config(backbone="resnet50", image_size=256, batch_size=2, **kw)
    if prec is not None:
        cfg.MODEL.ACT_PRECISION = prec
    if scope is not None:
        cfg.MODEL.ACT_SCOPE = scope
    return cfg


def _dev(prec):
    from feature_intertwiner_amd.sub_module import Dev
    return _randomise(Dev(_config(prec, "roi"), depth=256), 2025).to(DEV)


def _maps16(prec):
    g = torch.Generator().manual_seed(31)
    return [torch.randn((2, 256, s, s), generator=g).to(PRECISIONS[prec]).contiguous(memory_format=torch.channels_last).to(DEV)
            for s in SIDES]


def _rois():
    """[2, 64, 4] normalised boxes; their sizes run through what the level rule sends to p2, p3, p4 and p5."""
    rs = np.random.RandomState(41)
    side = np.array([0.1, 0.3, 0.5, 0.9, 1.4])[np.arange(128) % 5] * rs.uniform(0.9, 1.1, 128)
    aspect = rs.uniform(0.7, 1.4, 128)
    h, w = side * aspect, side / aspect
    cy, cx = rs.uniform(0.3, 0.7, 128), rs.uniform(0.3, 0.7, 128)
    boxes = np.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], 1).astype(np.float32)
    return torch.from_numpy(boxes).view(2, 64, 4)


def _box_rows(dev, rois):
    boxes = rois.reshape(-1, 4)
    box_ind = torch.arange(2, device=rois.device, dtype=torch.int32).repeat_interleave(64)
    level = dev.level_info(rois)[0]
    return boxes, box_ind, level


def _crop64(ups, boxes, box_ind, level, size):
    """float64 bilinear crops [n, C, size, size] of the float64 maps `ups` with the oracle's tap indices and fractions; a bin
    whose sample falls outside its map is 0."""
    from oracle import oracle as O
    crops = torch.zeros((boxes.shape[0], ups[0].shape[1], size, size), dtype=torch.float64)
    for l, up in enumerate(ups):
        sel = torch.nonzero(level == l + 2).view(-1)
        t = O.crop_taps(boxes[sel].numpy(), up.shape[2], up.shape[3], size, size)
        T = {k: torch.from_numpy(v.astype(np.float64 if v.dtype == np.float32 else np.int64)) for k, v in t.items()}
        img = up[box_ind[sel].long()].permute(0, 2, 3, 1)                      # [n, H, W, C]
        n = torch.arange(sel.numel()).view(-1, 1, 1)
        tap = lambda yy, xx: img[n, T[yy].unsqueeze(2), T[xx].unsqueeze(1)]     # [n, size, size, C]
        fx, fy = T["x_frac"].view(-1, 1, size, 1), T["y_frac"].view(-1, size, 1, 1)
        top = tap("y0", "x0") + (tap("y0", "x1") - tap("y0", "x0")) * fx
        bot = tap("y1", "x0") + (tap("y1", "x1") - tap("y1", "x0")) * fx
        val = top + (bot - top) * fy
        ok = (T["y_valid"].unsqueeze(2) * T["x_valid"].unsqueeze(1)).bool().unsqueeze(3)
        crops[sel] = torch.where(ok, val, torch.zeros_like(val)).permute(0, 3, 1, 2)
    return crops


@functools.lru_cache(maxsize=None)
def _reference(prec):
    """{7: crops, 14: crops} in float64 on the CPU from the widened maps (computed once per type)."""
    dev = _dev(prec)
    seq = dev.upsample[0]
    conv, bn = seq[0], seq[1]
    w, b = conv.weight.detach().double().cpu(), conv.bias.detach().double().cpu()
    g, beta, mean, var = (t.detach().double().cpu() for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))
    s = g / torch.sqrt(var + bn.eps)
    ups = []
    for m in _maps16(prec):
        y = F.conv2d(m.double().cpu().contiguous(), w, b, stride=1, padding=1)
        ups.append(F.relu(y * s.view(1, -1, 1, 1) + (beta - mean * s).view(1, -1, 1, 1)))
    rois = _rois()
    boxes, box_ind, level = (t.cpu() for t in _box_rows(dev, rois.to(DEV)))
    assert sorted(set(level.tolist())) == [2, 3, 4, 5]
    return {size: _crop64(ups, boxes, box_ind, level, size) for size in (7, 14)}


@pytest.mark.parametrize("prec", sorted(PRECISIONS))
def test_make_up_maps_are_the_hand_launched_16bit_convolutions(prec):
    from feature_intertwiner_amd import _lib, act16, roi16
    dev, maps = _dev(prec), _maps16(prec)
    rois = _rois().to(DEV)
    with torch.no_grad():
        act16.reset_stats()
        up = dev.make_up_maps(maps)
        assert act16.stats() == {"conv": 4, "pack": 0, "unpack": 0}
        assert len(up) == 4
        seq = dev.upsample[0]
        for m, u, side in zip(maps, up, SIDES):
            assert u.dtype is PRECISIONS[prec] and tuple(u.shape) == (2, 256, side, side)
            assert u.is_contiguous(memory_format=torch.channels_last)
            hand = act16.conv_bn_act16(m, seq[0], seq[1], relu=True)
            assert torch.equal(u.view(torch.int16), hand.view(torch.int16))
            assert float(u.float().max()) > 0.5 and float(u.float().min()) == 0.0
        # one call of the stage: the make-up pass, the 7x7 and the 14x14 crop; nothing is unpacked
        act16.reset_stats()
        roi16.reset_stats()
        pooled, mask, feat = dev(maps, rois)
        assert act16.stats() == {"conv": 4, "pack": 0, "unpack": 0}
        assert roi16.stats() == {"crop": 2}
        assert tuple(pooled.shape) == (128, 256, 7, 7) and tuple(mask.shape) == (128, 256, 14, 14)
        assert pooled.dtype is torch.float32 and mask.dtype is torch.float32
        # ... and with the maps handed in, only the crops
        act16.reset_stats()
        roi16.reset_stats()
        pooled2, mask2, _ = dev(maps, rois, up_maps=up)
        assert act16.stats()["conv"] == 0 and roi16.stats() == {"crop": 2}
        assert torch.equal(pooled, pooled2) and torch.equal(mask, mask2)
        dev.upsample[0][1].train()                                     # a training-mode BatchNorm is an error
        with pytest.raises(_lib.FiError, match="training mode"):
            dev.make_up_maps(maps)
        dev.upsample[0][1].eval()


@pytest.mark.parametrize("prec", sorted(PRECISIONS))
def test_crops_are_as_close_to_float64_as_the_existing_path(prec):
    from feature_intertwiner_amd import act16
    from feature_intertwiner_amd import conv as C
    ref = _reference(prec)
    dev, maps = _dev(prec), _maps16(prec)
    boxes, box_ind, level = _box_rows(dev, _rois().to(DEV))
    prev = C.conv_precision()
    C.set_conv_precision(prec)
    try:
        with torch.no_grad():
            old_up = dev.make_up_maps([act16.unpack(m) for m in maps])          # the path as it was
            assert all(u.dtype is torch.float32 for u in old_up)
            new_up = dev.make_up_maps(maps)
            old = {s: dev._crop(old_up, boxes, box_ind, level, s) for s in (7, 14)}
            new = {s: dev._crop(new_up, boxes, box_ind, level, s) for s in (7, 14)}
    finally:
        C.set_conv_precision(prev)
    err = lambda t, r: float((t.double().cpu() - r).norm() / r.norm())
    for s in (7, 14):
        assert tuple(new[s].shape) == tuple(ref[s].shape) == tuple(old[s].shape) and new[s].dtype is torch.float32
        e_old, e_new = err(old[s], ref[s]), err(new[s], ref[s])
        print("%s crops %dx%d: e_old %.3e  e_new %.3e  ratio %.3f" % (prec, s, s, e_old, e_new, e_new / e_old))
        assert e_old > 0.0 and e_old < 0.05, (s, e_old)                        # the yardstick itself is the 16-bit path
        assert e_new <= 1.5 * e_old, (s, e_new, e_old)


def _model(act=None, scope=None, **kw):
    from feature_intertwiner_amd.model import MaskRCNN
    from feature_intertwiner_amd.synthetic import SyntheticProposals, synthetic_batch
    torch.manual_seed(1)
    model = MaskRCNN(_config(act, scope, **kw)).to(DEV)
    batch = synthetic_batch(2, 256, device=DEV)
    model.external_proposals = SyntheticProposals(batch[2], 256, cycle=1)      # the same rows at every call
    windows = torch.tensor([[0, 0, 256, 256], [0, 16, 256, 240]], dtype=torch.float32)
    return model, batch, windows


def _run(model, batch, windows):
    from feature_intertwiner_amd import act16, pyr16, roi16
    for m in (act16, pyr16, roi16):
        m.reset_stats()
    det, masks = model([batch[0], windows], mode='inference')
    assert det.shape == (2, 100, 6) and masks.shape == (2, 100, 81, 28, 28)
    assert det.dtype is torch.float32 and masks.dtype is torch.float32
    assert bool(torch.isfinite(det).all()) and bool(torch.isfinite(masks).all())
    return det, masks, act16.stats(), pyr16.stats(), roi16.stats()


def test_model_inference_unpacks_nothing_and_runs_the_make_up_pass_once():
    model, batch, windows = _model("bf16", "pyramid")
    _, _, a_pyr, p_pyr, r_pyr = _run(model, batch, windows)
    assert a_pyr["unpack"] == 4 and a_pyr["pack"] == 1 and r_pyr == {"crop": 0}
    del model
    model, batch, windows = _model("bf16", "roi")
    det, masks, a_roi, p_roi, r_roi = _run(model, batch, windows)
    assert a_roi["pack"] == 1 and a_roi["unpack"] == 0
    assert a_roi["conv"] == a_pyr["conv"] + 4                           # the make-up layer, once for both Dev calls
    assert r_roi == {"crop": 4}
    assert p_roi == p_pyr == {"lateral": 3, "head": 5}
    det2, masks2, a2, _, r2 = _run(model, batch, windows)
    assert torch.equal(det, det2) and torch.equal(masks, masks2) and a2 == a_roi and r2 == r_roi
    with pytest.raises(NotImplementedError, match="training"):
        model(list(batch), mode='train')


def test_model_inference_fp16_and_without_the_dev_stage():
    model, batch, windows = _model("fp16", "roi")
    _, _, a, p, r = _run(model, batch, windows)
    assert a["pack"] == 1 and a["unpack"] == 0 and r == {"crop": 4} and p == {"lateral": 3, "head": 5}
    conv_with = a["conv"]
    del model
    model, batch, windows = _model("bf16", "roi", dev_switch=False)     # the two crops read the 16-bit p2..p5 directly
    _, _, a, p, r = _run(model, batch, windows)
    assert a["pack"] == 1 and a["unpack"] == 0 and r == {"crop": 4}
    assert a["conv"] == conv_with - 4                                   # no make-up layer


def test_roi_scope_refuses_the_transposed_make_up_layer_and_older_scopes_do_not_reach_roi16():
    from feature_intertwiner_amd.model import MaskRCNN
    cfg = _config("bf16", "roi")
    cfg.DEV.UPSAMPLE_FAC = 2.
    with pytest.raises(NotImplementedError, match="DEV.UPSAMPLE_FAC"):
        MaskRCNN(cfg)
    model, batch, windows = _model("bf16", None)
    assert not hasattr(model.config.MODEL, "ACT_SCOPE")
    _, _, a, p, r = _run(model, batch, windows)
    assert r == {"crop": 0} and p == {"lateral": 0, "head": 0}
