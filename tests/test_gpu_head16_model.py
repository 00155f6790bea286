"""The box head and the mask head on 16-bit channels-last crops (MODEL.ACT_SCOPE = 'detect' next to a 16-bit
MODEL.ACT_PRECISION; feature_intertwiner_amd/head16.py): the two modules' accuracy, the whole model.

Modules.  Classifier and Mask of make_config(resnet50, 256, batch 2), seeded as tests/test_gpu_roi16_model.py seeds its modules
(conv weights N(0, 2 / fan_in), conv biases 0.01 N(0, 1); BatchNorm gamma in [0.75, 1.25], beta and mean 0.1 N(0, 1), variance
in [0.5, 1.5]; here also the linears and the transposed convolution, N(0, 2 / fan_in) and 0.01 N(0, 1)), in eval(), on seeded
N(0, 1) 16-bit crops of 128 x 256 x 7 x 7 and 32 x 256 x 14 x 14.  Outputs: probs and bbox of the box head, the masks.

Accuracy.  The reference is a float64 replica (convolutions as tests/fp64_ref.py's conv_ref, folded BatchNorm, ReLU, linears,
softmax / sigmoid) on the widened crops and the fp32 weights.  e_new is the relative Frobenius error of the 16-bit forward,
e_old that of the modules' existing forward on the widened fp32 NCHW crops with conv.set_conv_precision of the same type,
behind conv.prepare_step as in the model (the 3x3 weights channels-last, the 16-bit copies made).  Required: 0 < e_old < 0.05
and e_new <= 1.5 e_old, the bound of the trunk, pyramid and roi tests: under CONV_PRECISION every head layer of the existing
forward -- the convolutions, and linear_bn_act / linear through the 16-bit weight-gradient kernel, whose rows (128) are a
multiple of 64 -- rounds its operands to the type, so the 16-bit tensors the new path stores are the roundings the old path
applies when the next layer reads them, and e_old is like for like for all three outputs.
e_q -- the replica with the new path's roundings (weights, and every stored layer output, round-to-nearest-even) against the
plain replica -- is printed next to them: what the roundings alone cost.

Model.  MaskRCNN (resnet50, 256^2, batch 2) with ACT_PRECISION = 'bf16', ACT_SCOPE = 'detect' in inference: reference shapes,
fp32, finite; 1 pack and 0 unpack; act16's convolution count EQUAL to that of scope 'roi' taken in the same test (the
difference is 0: under 'roi' the heads and the feature extractor ran on the fp32 kernels and were never in that counter);
roi16 launches nothing; head16 shows 2 crops, 7 convolutions, 2 output launches and 3 weight copies; a second run is bit-equal
and makes no copy; an in-place change of classifier.conv1.weight remakes one copy and changes the output; fp16 runs;
DEV.SWITCH off runs (four convolutions fewer: the crops read p2..p5); under 'roi' and without a scope head16's counters stay 0.

Measured on an MI355X (the test prints every line; also in DESIGN section 5), e_old / e_q / e_new (e_new / e_old):
    bf16  probs 4.927e-3 / 4.928e-3 / 4.925e-3 (1.000)   bbox 3.617e-3 / 3.617e-3 / 3.617e-3 (1.000)   masks 2.625e-3 / 2.626e-3 / 2.625e-3 (1.000)
    fp16  probs 6.198e-4 / 6.276e-4 / 6.326e-4 (1.021)   bbox 4.558e-4 / 4.559e-4 / 4.559e-4 (1.000)   masks 3.296e-4 / 3.296e-4 / 3.296e-4 (1.000)
The old path's error IS the operand roundings (e_old = e_q to three digits), which confirms that it is like for like.
fp16's e_old for probs moved between 6.198e-4 and 6.234e-4 from run to run (e_new / e_old 1.015 to 1.021): the old path's 16-bit product accumulates over
its split with atomics."""
import functools
import math

import pytest
import torch

import fp64_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRECISIONS = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _randomise(module, seed):
    """Seeded parameters and running statistics as the module docstring states them."""
    import torch.nn as nn
    g = torch.Generator().manual_seed(seed)
    for name, m in module.named_modules():
        if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d, nn.Linear)):
            fan_in = m.weight[0].numel() if not isinstance(m, nn.ConvTranspose2d) else m.weight.shape[0]
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


def _heads():
    from feature_intertwiner_amd.sub_module import Classifier, Mask
    cfg = _config()
    box = _randomise(Classifier(depth=256, num_classes=cfg.DATASET.NUM_CLASSES, pool_size=7, config=cfg), 2031).to(DEV)
    mask = _randomise(Mask(depth=256, num_classes=cfg.DATASET.NUM_CLASSES), 2032).to(DEV)
    return box, mask


def _crops16(prec):
    g = torch.Generator().manual_seed(53)
    make = lambda n, s: torch.randn((n, s, s, 256), generator=g).to(PRECISIONS[prec]).to(DEV).permute(0, 3, 1, 2)
    return make(128, 7), make(32, 14)


def _layer64(x, conv, bn, dtype, pad):
    """relu(bn(conv(x))) in float64; dtype: the new path's roundings (weight, stored output), or None."""
    w = conv.weight.detach()
    w = (w.to(dtype) if dtype is not None else w).double()
    y = R.conv_ref(x, w, pad=(pad, pad)) + conv.bias.detach().double().view(1, -1, 1, 1)
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    y = torch.relu((y - bn.running_mean.double().view(1, -1, 1, 1)) * s.view(1, -1, 1, 1) + bn.bias.detach().double().view(1, -1, 1, 1))
    return y.to(dtype).double() if dtype is not None else y


def _box64(box, x, dtype):
    rnd = (lambda t: t.to(dtype).double()) if dtype is not None else (lambda t: t.double())
    y = _layer64(x.double(), box.conv1, box.bn1, dtype, 0)
    y = _layer64(y, box.conv2, box.bn2, dtype, 0).view(x.shape[0], -1)
    logits = y @ rnd(box.linear_class.weight.detach()).t() + box.linear_class.bias.detach().double()
    bbox = y @ rnd(box.linear_bbox.weight.detach()).t() + box.linear_bbox.bias.detach().double()
    return torch.softmax(logits, 1), bbox.view(bbox.shape[0], -1, 4)


def _mask64(mask, x, dtype):
    rnd = (lambda t: t.to(dtype).double()) if dtype is not None else (lambda t: t.double())
    y = x.double()
    for conv, bn in ((mask.conv1, mask.bn1), (mask.conv2, mask.bn2), (mask.conv3, mask.bn3), (mask.conv4, mask.bn4)):
        y = _layer64(y, conv, bn, dtype, 1)
    n, _, H, W = y.shape
    # the 2 x 2 / stride 2 transposed convolution: out[n, c, 2h + a, 2w + b] = sum_i y[n, i, h, w] W[i, c, a, b] + bias[c]
    u = torch.einsum("nihw,icab->nchawb", y, rnd(mask.deconv.weight.detach())).reshape(n, -1, 2 * H, 2 * W)
    u = torch.relu(u + mask.deconv.bias.detach().double().view(1, -1, 1, 1))
    u = u.to(dtype).double() if dtype is not None else u
    z = torch.einsum("nchw,kc->nkhw", u, rnd(mask.conv5.weight.detach()[:, :, 0, 0]))
    return torch.sigmoid(z + mask.conv5.bias.detach().double().view(1, -1, 1, 1))


@functools.lru_cache(maxsize=None)
def _references(prec):
    """{output: (float64 reference, float64 replica with the new path's roundings)}, computed once per type."""
    box, mask = _heads()
    x7, x14 = _crops16(prec)
    with torch.no_grad():
        pb, bb = _box64(box, x7, None)
        pq, bq = _box64(box, x7, PRECISIONS[prec])
        m, mq = _mask64(mask, x14, None), _mask64(mask, x14, PRECISIONS[prec])
    return {"probs": (pb, pq), "bbox": (bb, bq), "masks": (m, mq)}


@pytest.mark.parametrize("prec", sorted(PRECISIONS))
def test_heads_are_as_close_to_float64_as_the_existing_forward(prec):
    from feature_intertwiner_amd import act16, head16, roi16
    from feature_intertwiner_amd import conv as C
    ref = _references(prec)
    box, mask = _heads()
    x7, x14 = _crops16(prec)
    assert x7.is_contiguous(memory_format=torch.channels_last) and x14.dtype is PRECISIONS[prec]
    prev = C.conv_precision()
    C.set_conv_precision(prec)
    try:
        with torch.no_grad():
            C.prepare_step(box)
            C.prepare_step(mask)
            _, p_old, b_old = box(x7.float().contiguous())                     # the path as it was: fp32 NCHW crops
            m_old = mask(x14.float().contiguous())
            for m in (act16, head16, roi16):
                m.reset_stats()
            _, p_new, b_new = box(x7)
            assert head16.stats() == {"crop": 0, "conv": 2, "out": 1, "weights": 2}
            m_new = mask(x14)
            assert head16.stats() == {"crop": 0, "conv": 7, "out": 2, "weights": 3}
            assert act16.stats() == {"conv": 0, "pack": 0, "unpack": 0} and roi16.stats() == {"crop": 0}
    finally:
        C.set_conv_precision(prev)
    err = lambda t, r: float((t.double() - r).norm() / r.norm())
    for name, old, new in (("probs", p_old, p_new), ("bbox", b_old, b_new), ("masks", m_old, m_new)):
        r, q = ref[name]
        assert tuple(new.shape) == tuple(r.shape) == tuple(old.shape) and new.dtype is torch.float32
        assert new.is_contiguous() and bool(torch.isfinite(new).all())
        e_old, e_new, e_q = err(old, r), err(new, r), err(q, r)
        print("%s %s: e_old %.3e  e_q %.3e  e_new %.3e  e_new / e_old %.3f  e_new / e_q %.3f"
              % (prec, name, e_old, e_q, e_new, e_new / e_old, e_new / e_q))
        assert e_old > 0.0 and e_old < 0.05, (name, e_old)                     # the yardstick itself is the 16-bit path
        assert e_new <= 1.5 * e_old, (name, e_new, e_old)
    assert tuple(p_new.shape) == (128, 81) and tuple(b_new.shape) == (128, 81, 4) and tuple(m_new.shape) == (32, 81, 28, 28)


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
    from feature_intertwiner_amd import act16, head16, pyr16, roi16
    for m in (act16, pyr16, roi16, head16):
        m.reset_stats()
    det, masks = model([batch[0], windows], mode='inference')
    assert det.shape == (2, 100, 6) and masks.shape == (2, 100, 81, 28, 28)
    assert det.dtype is torch.float32 and masks.dtype is torch.float32
    assert bool(torch.isfinite(det).all()) and bool(torch.isfinite(masks).all())
    return det, masks, act16.stats(), pyr16.stats(), roi16.stats(), head16.stats()


ZERO = {"crop": 0, "conv": 0, "out": 0, "weights": 0}


def test_model_inference_keeps_both_heads_16bit():
    model, batch, windows = _model("bf16", "roi")
    _, _, a_roi, p_roi, r_roi, h_roi = _run(model, batch, windows)
    assert r_roi == {"crop": 4} and h_roi == ZERO
    del model
    model, batch, windows = _model("bf16", "detect")
    det, masks, a, p, r, h = _run(model, batch, windows)
    assert a["pack"] == 1 and a["unpack"] == 0
    assert a["conv"] == a_roi["conv"]               # minus 0: 'roi' ran the heads and the feature extractor on fp32 kernels
    assert p == p_roi == {"lateral": 3, "head": 5}
    assert r == {"crop": 0}
    assert h == {"crop": 2, "conv": 7, "out": 2, "weights": 3}
    assert float(masks.min()) >= 0.0 and float(masks.max()) <= 1.0 and float(masks.max()) > float(masks.min())
    det2, masks2, a2, _, r2, h2 = _run(model, batch, windows)
    assert torch.equal(det, det2) and torch.equal(masks, masks2) and a2 == a and r2 == r
    assert h2 == {"crop": 2, "conv": 7, "out": 2, "weights": 0}
    with torch.no_grad():
        model.classifier.conv1.weight.mul_(0.5)     # in place: the version counter moves, the address does not
    det3, masks3, _, _, _, h3 = _run(model, batch, windows)
    assert h3 == {"crop": 2, "conv": 7, "out": 2, "weights": 1}
    assert not torch.equal(det, det3)
    with pytest.raises(NotImplementedError, match="training"):
        model(list(batch), mode='train')


def test_model_inference_fp16_and_without_the_dev_stage():
    model, batch, windows = _model("fp16", "detect")
    _, _, a, p, r, h = _run(model, batch, windows)
    assert a["pack"] == 1 and a["unpack"] == 0 and r == {"crop": 0} and p == {"lateral": 3, "head": 5}
    assert h == {"crop": 2, "conv": 7, "out": 2, "weights": 3}
    conv_with = a["conv"]
    del model
    model, batch, windows = _model("bf16", "detect", dev_switch=False)  # the two crops read the 16-bit p2..p5 directly
    _, _, a, p, r, h = _run(model, batch, windows)
    assert a["pack"] == 1 and a["unpack"] == 0 and r == {"crop": 0}
    assert h == {"crop": 2, "conv": 7, "out": 2, "weights": 3}
    assert a["conv"] == conv_with - 4                                   # no make-up layer


def test_detect_refusals_and_older_scopes_do_not_reach_head16():
    from feature_intertwiner_amd.model import MaskRCNN
    cfg = _config("bf16", "detect")
    cfg.DEV.CLS_MERGE_FEAT = True
    with pytest.raises(NotImplementedError, match="DEV.CLS_MERGE_FEAT"):
        MaskRCNN(cfg)
    model, batch, windows = _model("bf16", None)
    assert not hasattr(model.config.MODEL, "ACT_SCOPE")
    _, _, a, p, r, h = _run(model, batch, windows)
    assert h == ZERO and r == {"crop": 0}
