"""TRAIN.ACT_SCOPE = 'heads': the detector's train step with the box and mask heads forward and backward on 16-bit
channels-last crops.  The detector of tests/test_gpu_fpn16_model.py: ResNet-50, 256^2, 2 images, 64 RoIs, synthetic proposals,
the fp32 model's weights; bf16 and fp16 (fp16 with LOSS_SCALE 1024).

Loss: every term of the train-mode loss tracks fp32's within the 5 % + 1e-3 that file grants.

Counters of ONE workflow.train_step, derived from 'crops' (tests/test_gpu_crops16_model.py: gated 48, premasked 52,
relu_grad 4, dgrad 16, wgrad 64, pack 1 / unpack 1, gate-pack 4, patch gather / scatter 1 / 1):
  - the box head: the full-window layer, conv2 and the stacked class + box output layer -- three weight gradients, two gated
    data gradients (conv2 claims the full-window layer's gate, the output layer conv2's), one plain one (the full-window
    layer's, to the crop node), two premasked backwards;
  - the mask head's graph batch: conv1..conv4 and the transposed convolution -- five weight gradients, four gated data
    gradients (conv2..conv4 and the transposed convolution), one plain one (conv1's, to the crop node), five premasked
    backwards; conv5's backward is the ONE class-rows launch, which holds its weight gradient too;
  - so gated 48 + 2 + 4 = 54, plain 16 + 2 = 18, premasked 52 + 2 + 5 = 59, relu_grad stays 4, fallback 0, and weight
    gradients 64 + 3 + 5 = 72.  (The issue's reading of the code says 73: it counts a wgrad16 launch for conv5.  Here conv5's
    d weight leaves the class-rows kernel, as the issue's section 1(b) asks, so no ninth launch exists.)
  - train16 pack 1 / unpack 1; crops16: gate-pack 4, patch gather and scatter 1 each, and its own crop node does not run;
    heads16: one crop node, two crop_backward16 launches, one class-rows launch; head16: three RoIAlign launches (7 x 7,
    graph batch, rest batch); roi16: two (the feature extractor's rows, the graph-less big-box crop).
Learning: five steps, all finite, the last loss below the first.
Parameter gradients: one backward with LOSS_SCALE 1024 for both types; classifier.conv1 / bn1 (as the 1x1 layer on the crop's
[7, 7, 256] run that its backward runs), mask.conv4 / bn4, mask.deconv and mask.conv5 against float64 from their recorded
(g, x) -- (d, u) for conv5 -- with the bars of tests/test_gpu_heads16_box.py and tests/test_gpu_heads16_mask.py; every
recorded g above 2^-14.
Refusals when the model is built; neutrality: with the scope absent, 'trunk', 'pyramid' or 'crops' heads16.stats() stays zero
(the 'crops' counters themselves are held by tests/test_gpu_crops16_model.py); MRCNN.MASK_HEAD_ON_POSITIVE_SLOTS under 'heads'
runs and builds no rest crop."""
import math
import types

import pytest
import torch

import fp64_ref as R
from test_gpu_grad16_layer import DEV, DTYPES, _B, _held
from test_gpu_train16_block import _check_param_grads, _counts, _record, _reset
from test_gpu_train16_trunk import PRECISION
from test_gpu_fpn16_model import _detector, _fp32_reference

pytestmark = pytest.mark.gpu
ZERO = {"crop_bwd": 0, "class_rows": 0, "crops": 0}


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_detector_train_step_with_both_heads_on_16_bit_crops(sfx):
    from feature_intertwiner_amd import conv as C, crops16, fpn16, head16, heads16, roi16, train16
    from feature_intertwiner_amd.workflow import compute_loss, set_optimizer, train_step
    fp32 = _fp32_reference()
    prec = PRECISION[sfx]
    cfg, model, batch = _detector(prec, "heads", prec, loss_scale=1024.0 if prec == "fp16" else None)
    model.load_state_dict(fp32["weights"])
    _, terms = compute_loss(model, list(batch))
    for k in ("rpn_cls", "rpn_bbox", "mrcnn_cls", "mrcnn_bbox", "mrcnn_mask"):
        a, b = fp32["terms"][k], float(terms[k])
        print("%s %s: fp32 %.6f, TRAIN.ACT_SCOPE 'heads' %.6f" % (sfx, k, a, b))
        assert abs(a - b) <= 0.05 * abs(a) + 1e-3, (k, a, b)
    del terms
    opt = set_optimizer(model, cfg.TRAIN)
    _reset()
    for m in (fpn16, crops16, heads16, head16, roi16):
        m.reset_stats()
    hist = [float(train_step(model, opt, list(batch))["total"])]
    cnt, t, c, h = _counts(), train16.stats(), crops16.stats(), heads16.stats()
    print("%s counters: %s, train16 %s, crops16 %s, heads16 %s, head16 %s, roi16 %s" % (sfx, cnt, t, c, h, head16.stats(),
                                                                                     roi16.stats()))
    assert cnt == dict(gated=54, premasked=59, fallback=0, relu_grad=4, dgrad=18, wgrad=72), cnt
    assert t["pack"] == 1 and t["unpack"] == 1, t
    assert c == dict(patch_fwd=1, patch_bwd=1, gate_pack=4, crops=0), c
    assert h == dict(crop_bwd=2, class_rows=1, crops=1), h
    assert head16.stats()["crop"] == 3 and roi16.stats()["crop"] == 2
    hist += [float(train_step(model, opt, list(batch))["total"]) for _ in range(4)]
    assert hist[-1] < hist[0] and all(math.isfinite(v) for v in hist), hist
    assert train16.stats()["fallback"] == 0 and fpn16.stats()["top_to_autograd"] == 0
    assert C.conv_precision() == "fp32"


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_head_weight_gradients_against_float64(sfx, monkeypatch):
    from feature_intertwiner_amd import heads16
    from feature_intertwiner_amd.workflow import compute_loss
    fp32 = _fp32_reference()
    prec = PRECISION[sfx]
    cfg, model, batch = _detector(prec, "heads", prec, loss_scale=1024.0)
    model.load_state_dict(fp32["weights"])
    calls = _record(monkeypatch)
    rows = []

    def rec(*a, _fn=heads16.class_rows_grad16, **kw):
        rows.append((a[0].clone(), a[1], a[2], a[3]))
        return _fn(*a, **kw)
    monkeypatch.setattr(heads16, "class_rows_grad16", rec)
    for p in model.parameters():
        p.grad = None
    loss, _ = compute_loss(model, list(batch))
    (loss * float(cfg.TRAIN.LOSS_SCALE)).backward()
    torch.cuda.synchronize()
    wg = [k for k in calls if k[0] == "wgrad16"]
    assert len(wg) == 72 and len(rows) == 1
    cls_head, mask = model.classifier, model.mask
    # backward order: the mask head ran last, so its layers come first -- the transposed convolution, conv4, ... -- then the
    # box head's output layer, conv2 and full-window layer
    assert [k[1][2] for k in wg[:8]] == [1, 3, 3, 3, 3, 1, 1, 1]      # (k[1] = (g, x, R, S, stride, pad))
    deconv, conv4, window = wg[0], wg[1], wg[7]
    assert deconv[1][0].shape[1] == 4 * 256 and deconv[1][2] == 1 and conv4[1][2] == 3 and conv4[1][0].shape[1] == 256
    assert window[1][1].shape[1] == 49 * 256 and window[1][0].shape[1] == 1024
    for k in (deconv, conv4, window):
        assert float(k[1][0].float().abs().max()) > 2.0 ** -14
    _check_param_grads([conv4], [(mask.conv4, mask.bn4)], sfx, "heads %s mask.conv4" % sfx)
    as_rows = lambda w: w.detach().permute(0, 2, 3, 1).reshape(w.shape[0], -1, 1, 1).contiguous()
    w_rows = as_rows(cls_head.conv1.weight)
    w_rows.grad = as_rows(cls_head.conv1.weight.grad)
    surrogate = types.SimpleNamespace(weight=w_rows, bias=cls_head.conv1.bias, kernel_size=(1, 1), stride=(1, 1), padding=(0, 0))
    _check_param_grads([window], [(surrogate, cls_head.bn1)], sfx, "heads %s classifier.conv1" % sfx)
    # mask.deconv, from its recorded (g, x): the bars of tests/test_gpu_heads16_mask.py
    g, x = deconv[1][0], deconv[1][1].detach()
    P = g.shape[0] * g.shape[2] * g.shape[3]
    cin, cout = mask.deconv.weight.shape[0], mask.deconv.weight.shape[1]
    to_param = lambda v: v.reshape(2, 2, cout, cin).permute(3, 2, 0, 1)
    _held(mask.deconv.weight.grad, to_param(R.wgrad_ref(x, g, 1, 1, (1, 1), (0, 0))),
          _B(P, to_param(R.wgrad_ref(x.abs(), g.abs(), 1, 1, (1, 1), (0, 0)))), "heads %s mask.deconv dW" % sfx)
    g64 = g.to(torch.float64)
    s_ab, m_ab = g64.sum((0, 2, 3)).view(4, cout), g64.abs().sum((0, 2, 3)).view(4, cout)
    B_ab = _B(P, m_ab)
    _held(mask.deconv.bias.grad, s_ab.sum(0), B_ab.sum(0) + 4.0 * R.U * (s_ab.abs() + B_ab).sum(0),
          "heads %s mask.deconv d bias" % sfx)
    # mask.conv5, from the class-rows launch's recorded (d, u, w, cls)
    d, u, w16, cls = rows[0]
    n, C4, H, W = u.shape
    Cc, K = C4 // 4, w16.shape[0]
    assert float(d.abs().max()) > 2.0 ** -14
    x5 = u.detach().to(torch.float64).reshape(n, 4, Cc, H * W).permute(0, 2, 1, 3).reshape(n, Cc, 4 * H * W)
    _, dw_ref, mw, db_ref, mb, cnt = R.class_row_bwd_ref(d.reshape(n, 4 * H * W), x5, w16, cls, K, True)
    R.check_bar(mask.conv5.weight.grad.view(K, Cc), dw_ref, mw, cnt[:, None].expand_as(mw), "heads %s mask.conv5 dW" % sfx)
    R.check_bar(mask.conv5.bias.grad, db_ref, mb, cnt, "heads %s mask.conv5 d bias" % sfx)


def test_refusals_when_the_model_is_built():
    from feature_intertwiner_amd.config import make_config
    from feature_intertwiner_amd.model import MaskRCNN
    cfg = make_config("resnet50", 256, 2, 64, dev_switch=True, loss_choice="l2")
    cfg.TRAIN.ACT_PRECISION, cfg.TRAIN.ACT_SCOPE = "bf16", "heads"
    MaskRCNN(cfg)                                                    # builds
    cfg.DEV.CLS_MERGE_FEAT = True
    with pytest.raises(NotImplementedError, match=r"TRAIN\.ACT_SCOPE = 'heads' needs DEV\.CLS_MERGE_FEAT"):
        MaskRCNN(cfg)
    cfg.DEV.CLS_MERGE_FEAT = False
    cfg.DEV.UPSAMPLE_FAC = 2.                                        # what 'crops' refuses is refused too
    with pytest.raises(NotImplementedError, match=r"TRAIN\.ACT_SCOPE = 'heads' needs DEV\.UPSAMPLE_FAC"):
        MaskRCNN(cfg)
    cfg.DEV.UPSAMPLE_FAC = 1.
    cfg.TRAIN.ACT_PRECISION = "fp32"
    with pytest.raises(ValueError, match=r"TRAIN\.ACT_SCOPE = 'heads' needs TRAIN\.ACT_PRECISION"):
        MaskRCNN(cfg)


def test_without_the_scope_nothing_of_heads16_runs():
    from feature_intertwiner_amd import heads16
    from feature_intertwiner_amd.workflow import set_optimizer, train_step
    for scope in (None, "trunk", "pyramid", "crops"):
        cfg, model, batch = _detector("bf16", scope, "bf16")
        opt = set_optimizer(model, cfg.TRAIN)
        heads16.reset_stats()
        loss = float(train_step(model, opt, list(batch))["total"])
        assert math.isfinite(loss)
        assert heads16.stats() == ZERO, scope
        del model, opt


def test_mask_head_on_positive_slots_builds_no_rest_crop():
    from feature_intertwiner_amd import head16, heads16
    from feature_intertwiner_amd.model import MaskRCNN
    from feature_intertwiner_amd.workflow import set_optimizer, train_step
    cfg, model, batch = _detector("bf16", "heads", "bf16")
    cfg.MRCNN.MASK_HEAD_ON_POSITIVE_SLOTS = True                     # (the model reads the setting at every step)
    opt = set_optimizer(model, cfg.TRAIN)
    heads16.reset_stats()
    head16.reset_stats()
    loss = float(train_step(model, opt, list(batch))["total"])
    assert math.isfinite(loss)
    assert heads16.stats() == dict(crop_bwd=2, class_rows=1, crops=1)
    assert head16.stats()["crop"] == 2                               # 7 x 7 and the graph batch: no rest crop
