"""TRAIN.ACT_SCOPE = 'pyramid': the ResNet-50 trunk + FPN on a 2 x 3 x 64 x 96 image (c2 16 x 24 ... c5 2 x 3), and the
detector's train step.

Trunk + FPN (random eval-mode BatchNorm statistics, unit-gain weights), bf16 and fp16:
  - p2..p5 are torch.equal to the unpacked FPN._pyramid16 (the inference launches) of the same c2..c5 under no_grad, p6 is
    the stride-2 subsample of p5;
  - the counters of the BACKWARD, derived: the trunk has 52 layers and the pyramid 8, each runs one weight gradient: 60
    wgrad.  In the trunk every layer whose output has a claimer is premasked: all but the four projections (no ReLU) --
    c2..c4 are claimed by the next stage's first conv1 once the lateral's gradient arrives through the lateral_box, c5 by
    P5_conv1, its only reader -- so 48 gated launches, 48 premasked, 4 relu_grad (the projections sum their dy with it), 0
    fallback.  The ungated data gradients: the layers whose input carries no gate to claim -- the four projections (conv1
    next to them claims it), C2's first conv1 on the packed stem map, the four smoothing layers and the three laterals: 12.
    fi_fpn16_topdown_grad: the four smoothing layers and the finest lateral only sum (5), the two coarser laterals and
    P5_conv1 add what the finer lateral left (3), no lateral returns a top gradient to autograd.  The boundary casts: the
    four fp32 p gradients are packed (4) and the packed stem map's gradient is unpacked (1) -- no c-level cast;
  - the parameter gradients of the eight pyramid layers and of the 52 trunk layers are held to float64 on the (g, x) each
    weight gradient was recorded with, every g above 2^-14.
Detector: the fp32 model and the 'pyramid' model load the same weights; the train-mode loss tracks fp32's within the 5 %
per term tests/test_gpu_train16_trunk.py grants; workflow.train_step runs unchanged, its counters are the trunk + FPN's, and
it learns.  With TRAIN.ACT_SCOPE absent fpn16.stats() stays zero."""
import math

import pytest
import torch

from test_gpu_grad16_layer import DEV, DTYPES
from test_gpu_train16_block import _check_param_grads, _counts, _record, _reset, _zero_grads
from test_gpu_train16_trunk import PRECISION, _stage_layers, _trunk
from test_gpu_fpn16_layer import _check_bias_layer_grads, _check_topdown_calls, _fpn_counts, _record_topdown

pytestmark = pytest.mark.gpu
ZERO = {"topdown": 0, "sums": 0, "lateral": 0, "conv": 0, "top_to_autograd": 0, "weights": 0}


def _config(prec, scope):
    from feature_intertwiner_amd.config import make_config
    cfg = make_config(backbone="resnet50", image_size=256, batch_size=2, train_rois_per_image=48)
    cfg.TRAIN.ACT_PRECISION = prec
    if scope is not None:
        cfg.TRAIN.ACT_SCOPE = scope
    return cfg


def _fpn(prec, seed):
    from feature_intertwiner_amd import sub_module
    net = _trunk(seed)
    fpn = sub_module.FPN(_config(prec, "pyramid"), net.C1, net.C2, net.C3, net.C4, net.C5, out_channels=256)
    gen = torch.Generator().manual_seed(seed + 2)
    own = [fpn.P5_conv1, fpn.P4_conv1, fpn.P3_conv1, fpn.P2_conv1, fpn.P5_conv2[1], fpn.P4_conv2[1], fpn.P3_conv2[1],
           fpn.P2_conv2[1]]
    with torch.no_grad():
        for m in own:                                                # unit gain, as _trunk's
            cout, cin, k, _ = m.weight.shape
            m.weight.copy_(torch.randn(m.weight.shape, generator=gen) / math.sqrt(cin * k * k))
            m.bias.copy_(0.25 * torch.randn(cout, generator=gen))
    fpn.to(DEV)
    fpn.eval()
    return net, fpn


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_trunk_and_pyramid_forward_bits_counters_and_gradients(sfx, monkeypatch):
    from feature_intertwiner_amd import act16, fpn16, train16
    net, fpn = _fpn(PRECISION[sfx], 81)
    gen = torch.Generator().manual_seed(83)
    image = torch.randn((2, 3, 64, 96), generator=gen).to(DEV)
    dys = [torch.randn(s, generator=gen).to(DEV) for s in
           ((2, 256, 16, 24), (2, 256, 8, 12), (2, 256, 4, 6), (2, 256, 2, 3), (2, 256, 1, 2))]
    c = {}
    hooks = [stage.register_forward_hook(lambda m, i, o, lvl=lvl: c.__setitem__(lvl, o.detach()))
             for lvl, stage in ((2, net.C2), (3, net.C3), (4, net.C4), (5, net.C5))]
    calls = _record(monkeypatch)
    tcalls = _record_topdown(monkeypatch)
    _zero_grads([fpn])
    fpn16.reset_stats()
    outs = fpn(image, mode="train")
    for h in hooks:
        h.remove()
    p = outs[:5]
    assert all(t.dtype == torch.float32 and t.is_contiguous() and t.requires_grad for t in p)
    assert [tuple(t.shape) for t in p] == [tuple(d.shape) for d in dys]
    assert all(c[lvl].dtype == DTYPES[sfx] for lvl in (2, 3, 4, 5))
    assert fpn16.stats()["lateral"] == 3 and fpn16.stats()["conv"] == 5
    _reset()
    fpn16.reset_stats()
    torch.autograd.backward(p, dys)
    torch.cuda.synchronize()
    cnt = _counts()
    assert cnt == dict(gated=48, premasked=48, fallback=0, relu_grad=4, dgrad=12, wgrad=60), cnt
    assert _fpn_counts() == dict(topdown=3, sums=5, top_to_autograd=0), _fpn_counts()
    t = train16.stats()
    assert t["pack"] == 4 and t["unpack"] == 1, t                    # the four p gradients in, the stem map's gradient out
    # the forward: the inference launches on the same c2..c5
    with torch.no_grad():
        ref = fpn._pyramid16(c)
        for got, want in zip(p[:4], ref[:4]):
            assert torch.equal(got, act16.unpack(want))
        assert torch.equal(p[4], p[3][:, :, ::2, ::2]) and torch.equal(p[4], act16.unpack(ref[4]))
    assert all(bool(torch.isfinite(t.detach()).all()) and float(t.detach().abs().max()) > 0.0 for t in p)
    # the gradients
    _check_topdown_calls(list(tcalls), DTYPES[sfx])
    wg = [k for k in calls if k[0] == "wgrad16"]
    assert len(wg) == 60
    assert min(float(k[1][0].float().abs().max()) for k in wg) > 2.0 ** -14
    pyramid = [fpn.P2_conv2[1], fpn.P3_conv2[1], fpn.P4_conv2[1], fpn.P5_conv2[1], fpn.P2_conv1, fpn.P3_conv1, fpn.P4_conv1,
               fpn.P5_conv1]                                         # in the order the backward visits them
    _check_bias_layer_grads(wg[:8], pyramid, "pyramid %s" % sfx)
    layers = _stage_layers(net)
    assert len(layers) == 52
    _check_param_grads(wg[8:], layers, sfx, "trunk under the pyramid %s" % sfx)
    for prm in fpn.C1[0].parameters():
        assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()) and float(prm.grad.abs().max()) > 0.0


_FP32 = {}


def _detector(act, scope, conv_precision, loss_scale=None):
    from feature_intertwiner_amd.config import make_config
    from feature_intertwiner_amd.model import MaskRCNN
    from feature_intertwiner_amd.synthetic import SyntheticProposals, synthetic_batch
    batch = synthetic_batch(2, 256, device=DEV)
    torch.manual_seed(7)
    cfg = make_config("resnet50", 256, 2, 64, dev_switch=True, loss_choice="l2", conv_precision=conv_precision)
    if act is not None:
        cfg.TRAIN.ACT_PRECISION = act
    if scope is not None:
        cfg.TRAIN.ACT_SCOPE = scope
    if loss_scale is not None:
        cfg.TRAIN.LOSS_SCALE = loss_scale
    model = MaskRCNN(cfg).to(DEV)
    model.external_proposals = SyntheticProposals(batch[2], 256, seed=7)
    model.generator = torch.Generator(device=DEV).manual_seed(5)
    return cfg, model, batch


def _fp32_reference():
    from feature_intertwiner_amd.workflow import compute_loss
    if not _FP32:
        _, model, batch = _detector(None, None, "fp32")
        with torch.no_grad():
            _, terms = compute_loss(model, list(batch))
        _FP32["terms"] = {k: float(v) for k, v in terms.items()}
        _FP32["weights"] = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        del model
    return _FP32


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_detector_train_step_on_16_bit_pyramid_tensors(sfx):
    from feature_intertwiner_amd import conv as C, fpn16, train16
    from feature_intertwiner_amd.workflow import compute_loss, set_optimizer, train_step
    fp32 = _fp32_reference()
    prec = PRECISION[sfx]
    cfg, model, batch = _detector(prec, "pyramid", prec, loss_scale=1024.0 if prec == "fp16" else None)
    model.load_state_dict(fp32["weights"])
    _, terms = compute_loss(model, list(batch))                      # grad mode on: trunk and pyramid on 16-bit tensors
    for k in ("rpn_cls", "rpn_bbox", "mrcnn_cls", "mrcnn_bbox", "mrcnn_mask"):
        a, b = fp32["terms"][k], float(terms[k])
        print("%s %s: fp32 %.6f, TRAIN.ACT_SCOPE 'pyramid' %.6f" % (sfx, k, a, b))
        assert abs(a - b) <= 0.05 * abs(a) + 1e-3, (k, a, b)
    del terms
    opt = set_optimizer(model, cfg.TRAIN)
    _reset()
    fpn16.reset_stats()
    hist = [float(train_step(model, opt, list(batch))["total"])]
    cnt, t, f = _counts(), train16.stats(), fpn16.stats()
    assert cnt == dict(gated=48, premasked=48, fallback=0, relu_grad=4, dgrad=12, wgrad=60), cnt
    assert t["pack"] == 5 and t["unpack"] == 5, t                    # the stem map and p2..p5, forward and backward
    assert f == dict(topdown=3, sums=5, lateral=3, conv=5, top_to_autograd=0, weights=8), f
    hist += [float(train_step(model, opt, list(batch))["total"]) for _ in range(4)]
    assert hist[-1] < hist[0] and all(math.isfinite(h) for h in hist), hist
    assert train16.stats()["fallback"] == 0 and fpn16.stats()["top_to_autograd"] == 0
    assert C.conv_precision() == "fp32"


def test_without_the_scope_nothing_of_fpn16_runs():
    """TRAIN.ACT_PRECISION alone is the parent's train step: c2..c5 are unpacked and the pyramid runs on fp32 tensors."""
    from feature_intertwiner_amd import fpn16, train16
    from feature_intertwiner_amd.workflow import set_optimizer, train_step
    cfg, model, batch = _detector("bf16", None, "bf16")
    assert not hasattr(cfg.TRAIN, "ACT_SCOPE")
    opt = set_optimizer(model, cfg.TRAIN)
    _reset()
    fpn16.reset_stats()
    loss = float(train_step(model, opt, list(batch))["total"])
    assert math.isfinite(loss)
    assert fpn16.stats() == ZERO
    assert _counts() == dict(gated=47, premasked=47, fallback=0, relu_grad=5, dgrad=5, wgrad=52)
    assert train16.stats()["pack"] == 5 and train16.stats()["unpack"] == 5
