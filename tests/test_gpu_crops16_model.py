"""TRAIN.ACT_SCOPE = 'crops': the detector's train step with p2..p5 kept 16-bit channels-last up to the RoI crops.  The
detector of tests/test_gpu_fpn16_model.py: ResNet-50, 256^2, 2 images, 64 RoIs, synthetic proposals, the fp32 model's weights;
bf16 and fp16 (fp16 with LOSS_SCALE 1024).

Loss: every term of the train-mode loss tracks fp32's within the 5 % + 1e-3 that file grants.

Counters of ONE workflow.train_step, derived from 'pyramid' (tests/test_gpu_fpn16_model.py: gated 48, premasked 48,
relu_grad 4, dgrad 12, wgrad 60, pack 5 / unpack 5, topdown 3, sums 5):
  - the four smoothed maps are neither unpacked in forward nor their gradients packed in backward: train16 'pack' 1 (the
    stem map) and 'unpack' 1 (its gradient);
  - the make-up layer now runs as train16.conv_bn_act16 on each of p2..p5: four more weight gradients (64) and four more
    plain data gradients (16: p_l comes from a smoothing layer without a ReLU and carries no gate to claim);
  - the crops claim the Gate16 of u2..u5 and leave the masked gradient and its sums there: four more premasked backwards
    (52), no further relu_grad16 (4: the trunk's projections), no further gated launch (48), no fallback;
  - the pyramid's own launches are untouched: the smoothing layers still only sum (5), the coarser laterals and P5_conv1
    still add (3), fpn16's 'lateral' 3 / 'conv' 5 / 'weights' 8;
  - crops16: ONE patch gather and ONE in-place patch scatter (all five levels each), four gate-packs, one crops node.
Weight gradients: the make-up layer's (its four launches, one per level, are summed by autograd into one gradient, so the
float64 check takes each level's (g, x) pair and holds the SUM) and the four smoothing layers', from the (g, x) their
weight gradients were recorded with; every g above 2^-14 -- but for the make-up launch of a level that holds no RoI (the
boxes of a 256^2 image fall on the finest levels): RoIAlign's gradient into that level is exactly zero, and so is g.
This check runs BOTH types with LOSS_SCALE 1024: a level that holds a handful of RoIs sees gradients of 2e-5 unscaled
(measured, bf16), which bf16 carries but which lies below the 2^-14 the check asks of every g.
Learning: five steps, all finite, the last loss below the first.  Neutrality: with the scope absent or 'pyramid',
crops16.stats() stays zero."""
import math

import pytest
import torch

import fp64_ref as R
from test_gpu_grad16_layer import DEV, DTYPES, _B, _held
from test_gpu_train16_block import _counts, _record, _reset
from test_gpu_train16_trunk import PRECISION
from test_gpu_fpn16_layer import _check_bias_layer_grads
from test_gpu_fpn16_model import _detector, _fp32_reference

pytestmark = pytest.mark.gpu
ZERO = {"patch_fwd": 0, "patch_bwd": 0, "gate_pack": 0, "crops": 0}


def _check_make_up_grads(wg, conv, bn, what):
    """The shared make-up layer ran once per level: its parameter gradients are the sums over the four recorded (g, x)
    pairs.  d beta = sum of the column sums of g; dW = scale * sum of the unscaled weight gradients (+ the fp32 roundings of
    the fold), the bars of tests/test_gpu_train16_block.py added over the levels."""
    Cout, Cin = conv.weight.shape[0], conv.weight.shape[1]
    scale = bn._fi_fold[0].to(torch.float64)
    s_ref = torch.zeros(Cout, dtype=torch.float64, device=DEV)
    B_s = torch.zeros_like(s_ref)
    dwp = torch.zeros((Cout, Cin, 3, 3), dtype=torch.float64, device=DEV)
    B_w = torch.zeros_like(dwp)
    live = 0
    for _, a, _, _ in wg:
        g, x16, k, _, stride, pad = a
        assert (k, stride, pad) == (3, 1, 1) and g.shape[1] == Cout
        top = float(g.float().abs().max())
        assert top == 0.0 or top > 2.0 ** -14                        # a level without RoIs: an exactly zero gradient
        live += top > 0.0
        x16 = x16.detach()
        P = g.shape[0] * g.shape[2] * g.shape[3]
        g64 = g.to(torch.float64)
        s_ref += g64.sum((0, 2, 3))
        B_s += _B(P, g64.abs().sum((0, 2, 3)))
        dwp += R.wgrad_ref(x16, g, 3, 3, (1, 1), (1, 1))
        B_w += _B(P, R.wgrad_ref(x16.abs(), g.abs(), 3, 3, (1, 1), (1, 1)))
    n = len(wg)
    assert live >= 1
    # autograd adds the four fp32 gradients: n - 1 further roundings of the running sum
    _held(bn.bias.grad, s_ref, B_s + n * R.U * (s_ref.abs() + B_s), what + " d beta")
    ref = scale.view(-1, 1, 1, 1) * dwp
    scB = scale.abs().view(-1, 1, 1, 1) * B_w
    dw = conv.weight.grad
    assert dw.dtype == torch.float32 and dw.shape == conv.weight.shape
    _held(dw, ref, scB + (n + 1) * R.U * (ref.abs() + scB), what + " dW")


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_detector_train_step_up_to_the_crops_on_16_bit_tensors(sfx):
    from feature_intertwiner_amd import conv as C, crops16, fpn16, roi16, train16
    from feature_intertwiner_amd.workflow import compute_loss, set_optimizer, train_step
    fp32 = _fp32_reference()
    prec = PRECISION[sfx]
    cfg, model, batch = _detector(prec, "crops", prec, loss_scale=1024.0 if prec == "fp16" else None)
    model.load_state_dict(fp32["weights"])
    _, terms = compute_loss(model, list(batch))                      # grad mode on: 16-bit tensors up to the crops
    for k in ("rpn_cls", "rpn_bbox", "mrcnn_cls", "mrcnn_bbox", "mrcnn_mask"):
        a, b = fp32["terms"][k], float(terms[k])
        print("%s %s: fp32 %.6f, TRAIN.ACT_SCOPE 'crops' %.6f" % (sfx, k, a, b))
        assert abs(a - b) <= 0.05 * abs(a) + 1e-3, (k, a, b)
    del terms
    opt = set_optimizer(model, cfg.TRAIN)
    _reset()
    fpn16.reset_stats()
    crops16.reset_stats()
    roi16.reset_stats()
    hist = [float(train_step(model, opt, list(batch))["total"])]
    cnt, t, f, c = _counts(), train16.stats(), fpn16.stats(), crops16.stats()
    assert cnt == dict(gated=48, premasked=52, fallback=0, relu_grad=4, dgrad=16, wgrad=64), cnt
    assert t["pack"] == 1 and t["unpack"] == 1, t                    # the stem map and its gradient only
    assert f == dict(topdown=3, sums=5, lateral=3, conv=5, top_to_autograd=0, weights=8), f
    assert c == dict(patch_fwd=1, patch_bwd=1, gate_pack=4, crops=1), c
    assert roi16.stats()["crop"] == 3                                # 7x7, 14x14 and the graph-less big-box crop
    hist += [float(train_step(model, opt, list(batch))["total"]) for _ in range(4)]
    assert hist[-1] < hist[0] and all(math.isfinite(h) for h in hist), hist
    assert train16.stats()["fallback"] == 0 and fpn16.stats()["top_to_autograd"] == 0
    assert C.conv_precision() == "fp32"


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_make_up_and_smoothing_weight_gradients_against_float64(sfx, monkeypatch):
    """One backward of the train-mode loss (no optimiser step, so the gradients are still there): the make-up layer's and
    the four smoothing layers' parameter gradients against float64 on the recorded (g, x)."""
    from feature_intertwiner_amd import crops16, train16
    from feature_intertwiner_amd.workflow import compute_loss
    fp32 = _fp32_reference()
    prec = PRECISION[sfx]
    cfg, model, batch = _detector(prec, "crops", prec, loss_scale=1024.0)
    model.load_state_dict(fp32["weights"])
    calls = _record(monkeypatch)
    assert cfg.TRAIN.LOSS_SCALE == 1024.0
    for p in model.parameters():
        p.grad = None
    loss, _ = compute_loss(model, list(batch))
    scale = float(getattr(cfg.TRAIN, "LOSS_SCALE", 1.0))
    (loss * scale).backward()
    torch.cuda.synchronize()
    wg = [k for k in calls if k[0] == "wgrad16"]
    assert len(wg) == 64
    fpn = model.fpn
    smooth = [fpn.P2_conv2[1], fpn.P3_conv2[1], fpn.P4_conv2[1], fpn.P5_conv2[1]]
    # backward order: the heads are fp32; the first 16-bit weight gradients are the make-up layer's four launches, then
    # the four smoothing layers (p2 first: its gradient is complete first), then the laterals and the trunk
    _check_make_up_grads(wg[:4], model.dev_roi.upsample[0][0], model.dev_roi.upsample[0][1], "make-up %s" % sfx)
    by_size = sorted(wg[4:8], key=lambda k: -k[1][0].shape[2])
    _check_bias_layer_grads(by_size, smooth, "smoothing %s" % sfx)
    assert train16.stats()["fallback"] == 0 and crops16.stats()["gate_pack"] >= 4


def test_without_the_scope_nothing_of_crops16_runs():
    from feature_intertwiner_amd import crops16
    from feature_intertwiner_amd.workflow import set_optimizer, train_step
    for scope in (None, "pyramid"):
        cfg, model, batch = _detector("bf16", scope, "bf16")
        opt = set_optimizer(model, cfg.TRAIN)
        crops16.reset_stats()
        loss = float(train_step(model, opt, list(batch))["total"])
        assert math.isfinite(loss)
        assert crops16.stats() == ZERO
        del model, opt
