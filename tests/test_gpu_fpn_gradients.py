"""GPU: every gradient of the ResNet-50-FPN trunk in TRAINING mode against a float64 restatement from stock torch
functions (lib/sub_module.py:38-228: stem, SamePad + max-pool, bottleneck stages, lateral + top-down + smoothing).

This is the path on which round 3 moved work between autograd nodes: the stem's pooling on own kernels, every ReLU mask
applied in a reader's data-gradient epilogue (conv.Gate), the shortcut / projection / FPN-lateral gradients handed over
through GradBoxes and added (and masked) inside the first convolution's kernels, BatchNorm sums taken from the weight
gradient, the top-down upsampling's one-pass backward.  Run with and without the per-step state of prepare_step
(gradient arena, scaled W^T from the batched transpose, weight gradients queued and launched several at a time)."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _reference(x, sd):
    conv = lambda name, inp, stride=1, pad=0: F.conv2d(inp, sd[name + ".weight"], sd[name + ".bias"], stride=stride, padding=pad)
    bn = lambda name, inp: F.batch_norm(inp, sd[name + ".running_mean"], sd[name + ".running_var"], sd[name + ".weight"],
                                        sd[name + ".bias"], False, 0.0, 0.001)
    x = F.relu(bn("C1.1", conv("C1.0", x, 2, 3)))
    x = F.max_pool2d(F.pad(x, (0, 1, 0, 1)), 3, 2)                       # SamePad2d(3, 2) + MaxPool2d(3, 2)
    outs = {}
    for stage, blocks, stride in (("C2", 3, 1), ("C3", 4, 2), ("C4", 6, 2), ("C5", 3, 2)):
        for i in range(blocks):
            p = "%s.%d." % (stage, i)
            st = stride if i == 0 else 1
            out = F.relu(bn(p + "bn1", conv(p + "conv1", x, st)))
            out = F.relu(bn(p + "bn2", conv(p + "conv2", out, 1, 1)))
            out = bn(p + "bn3", conv(p + "conv3", out))
            res = bn(p + "downsample.1", conv(p + "downsample.0", x, st)) if i == 0 else x
            x = F.relu(out + res)
        outs[stage] = x
    up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")
    p5 = conv("P5_conv1", outs["C5"])
    p4 = conv("P4_conv1", outs["C4"]) + up(p5)
    p3 = conv("P3_conv1", outs["C3"]) + up(p4)
    p2 = conv("P2_conv1", outs["C2"]) + up(p3)
    return [conv("P%d_conv2.1" % l, p, 1, 1) for l, p in ((2, p2), (3, p3), (4, p4), (5, p5))]


def _worst_deviation(seed, arena):
    """(forward, gradients): worst relative L2 distance from the float64 restatement over the outputs / over the input
    gradient and every parameter gradient."""
    from feature_intertwiner_amd import conv as C
    from feature_intertwiner_amd.config import make_config
    from feature_intertwiner_amd.sub_module import FPN, ResNet
    torch.manual_seed(seed)
    cfg = make_config("resnet50", 128, 2, 16)
    r = ResNet("resnet50", stage5=True)
    fpn = FPN(cfg, *r.stages(), out_channels=256)
    for m in fpn.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.weight.data.uniform_(0.6, 1.4)
            m.bias.data.normal_(0, 0.1)
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.6, 1.4)
    fpn.eval()                                               # BatchNorm always evaluates (lib/model.py:265-267)
    x = torch.randn(2, 3, 128, 128)
    sd = {k: v.detach().double().requires_grad_("running" not in k) for k, v in fpn.state_dict().items()
          if v.dtype.is_floating_point}
    xd = x.double().requires_grad_(True)
    ref = _reference(xd, sd)
    gys = [torch.randn(t.shape) for t in ref]
    sum((t * g.double()).sum() for t, g in zip(ref, gys)).backward()
    fpn = fpn.to(DEV)
    try:
        for rep in range(2 if arena else 1):
            for p in fpn.parameters():
                p.grad = None
            if arena:
                C.prepare_step(fpn)                          # 2nd round: the (conv, bn) pairs are known -> scaled W^T
            xg = x.to(DEV).requires_grad_(True)
            p2, p3, p4, p5, p6, _ = fpn(xg, "train")
            sum((t * g.to(DEV)).sum() for t, g in zip((p2, p3, p4, p5), gys)).backward()
            torch.cuda.synchronize()
        rel = lambda got, want: float((got.cpu().double() - want).norm() / (want.norm() + 1e-30))
        fwd = max(rel(got.detach(), want.detach()) for got, want in zip((p2, p3, p4, p5), ref))
        assert all(p.grad is not None for p in fpn.parameters())
        grad = max([rel(xg.grad, xd.grad)] + [rel(p.grad, sd[k].grad) for k, p in fpn.named_parameters()])
        return fwd, grad
    finally:
        C.invalidate_step_state()


@pytest.mark.parametrize("arena", [False, True])
def test_fpn_training_gradients_match_float64(arena):
    """Forward values: 1e-5 on every input.  Gradients: a ReLU / max-pool decision on a value within rounding distance
    of a tie may fall the other way than in float64 (e.g. the batched BatchNorm fold differs from the in-layer one in
    the last bit); that moves the gradient inside ONE receptive field -- up to 4e-3 in relative L2 for the parameters
    of an 8 x 8 layer, nothing elsewhere -- and is a property of the input, not of the kernels.  So: three inputs; on
    at least one of them EVERY gradient is within 2e-5 of float64 (measured 1.7e-6: masks, scales, hand-offs and sums
    are exact), and on all of them within 3e-2 (a wrong mask, scale or hand-off moves gradients by 1e-1 .. 1)."""
    devs = [_worst_deviation(seed, arena) for seed in (18, 17, 19)]
    assert max(f for f, _ in devs) <= 1e-5, devs
    assert min(g for _, g in devs) <= 2e-5, devs
    assert max(g for _, g in devs) <= 3e-2, devs
