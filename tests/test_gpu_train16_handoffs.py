"""The gradient hand-offs of the 16-bit training path (train16: res_grad_to, dx_give_to, dx_add_from, the lateral chain through
unpack's backward, Bottleneck._forward_train16) against an INDEPENDENT reference: stock torch autograd in float64.

The reference restates the blocks from F.conv2d and the eval-BatchNorm formula, on the same rounded operands: the leaf as
rounded to the 16-bit type, each weight as rounded to the type (what the forward launch multiplies), and every layer
output REPLACED by the 16-bit path's own stored output (recorded per layer; straight-through gradient) with the ReLU mask
taken from that stored output -- after the layer's float64 value has been held to it within 2 u, layer by layer.  So the
point at which the network is linearised is the 16-bit path's, while the backward is plain float64 autograd with no
boxes, gates or hand-offs in it.  (Rounding the float64 forward on its own does NOT do: measured on the trunk, two
forwards that round independently drift to a relative distance of 1.1 u by c4, enough ReLU masks near zero flip, and
the gradients of even the last layer sit 11 u (bf16) to 90 u (fp16) apart -- a distance of the order of sqrt(u) that
says nothing about the backward.)  What remains between the two gradients is the 16-bit path's own backward rounding: per layer on the path ONE rounding of the data gradient and ONE of
the scaled transposed weight, each a relative error of at most u (2^-8 bf16, 2^-11 fp16).  n such errors add to at most
u sqrt(n) in quadrature; the bar on the relative L2 distance is twice that, 2 u sqrt(2 layers) (the factor covers that the
errors are relative to local magnitudes and the rare mask that flips on an fp32-vs-float64 tie).  It is derived, not fitted.
A lost or misrouted hand-off is an O(1) error; each case PROVES that on its own reference: the same reference with the
hand-off in question left out (shortcut detached, projection detached, lateral terms dropped) must lie more than two bars
away, so a gradient within one bar of the full reference cannot have lost it.

Cases: an identity block on a leaf (the shortcut through res_grad_to / dx_add_from), the stride-2 projection block behind a
producing layer with a lateral reader (dx_give_to, the chain lateral -> projection's dx_add -> conv1's gated launch,
unpack's backward into the box), the ResNet-50 trunk with all three laterals, a pair of filled boxes handed to one layer
(the one 16-bit add), and the error a frozen stem gets."""
import math

import pytest
import torch
import torch.nn.functional as F

from test_gpu_grad16_layer import CL, DEV, DTYPES, UNIT, _act, _layer
from test_gpu_train16_block import _block
from test_gpu_train16_trunk import _trunk

pytestmark = pytest.mark.gpu


class _Ref(object):
    """float64 leaves of the parameters of (conv, bn) pairs and the restated layer."""

    def __init__(self, dtype, outs):
        self.dtype, self.p, self.outs = dtype, {}, outs      # outs: conv -> the output the 16-bit path stored for it

    def params(self, conv, bn):
        if conv not in self.p:
            leaf = lambda t: t.detach().to(torch.float64).requires_grad_()
            self.p[conv] = dict(w=leaf(conv.weight.detach().to(self.dtype)), b=leaf(conv.bias), gamma=leaf(bn.weight),
                                beta=leaf(bn.bias))
        return self.p[conv]

    def layer(self, x, conv, bn, relu=True, res=None):
        q = self.params(conv, bn)
        z = F.conv2d(x, q["w"], q["b"], stride=conv.stride, padding=conv.padding)
        inv = 1.0 / torch.sqrt(bn.running_var.to(torch.float64) + bn.eps)
        y = (z - bn.running_mean.to(torch.float64).view(1, -1, 1, 1)) * (q["gamma"] * inv).view(1, -1, 1, 1) + \
            q["beta"].view(1, -1, 1, 1)
        if res is not None:
            y = y + res
        k = self.outs[conv].to(torch.float64)
        if relu:
            y = y * (k > 0).to(torch.float64)              # the mask the 16-bit path applied
        assert _rel(y.detach(), k) <= 2.0 * UNIT_OF[self.dtype], "the restated layer is not the 16-bit path's"
        return y + (k - y.detach())                        # its stored value, straight-through

    def block(self, x, b, drop_shortcut=False):
        out = self.layer(x, b.conv1, b.bn1)
        out = self.layer(out, b.conv2, b.bn2)
        res = x if b.downsample is None else self.layer(x, b.downsample[0], b.downsample[1], relu=False)
        return self.layer(out, b.conv3, b.bn3, res=res.detach() if drop_shortcut else res)


UNIT_OF = {torch.bfloat16: UNIT["bf16"], torch.float16: UNIT["f16"]}


def _recorded(monkeypatch):
    """conv -> the output train16.conv_bn_act16 returned for it, for every call from here on."""
    from feature_intertwiner_amd import train16
    outs = {}

    def rec(x16, conv, bn, *a, _fn=train16.conv_bn_act16, **kw):
        y = _fn(x16, conv, bn, *a, **kw)
        outs[conv] = y.detach()
        return y
    monkeypatch.setattr(train16, "conv_bn_act16", rec)
    return outs


def _rel(a, b):
    a, b = a.to(torch.float64), b.to(torch.float64)
    return float((a - b).norm() / b.norm())


def _bar(sfx, layers):
    return 2.0 * UNIT[sfx] * math.sqrt(2.0 * layers)


def _compare(sfx, layers, what, got_leaf, ref_leaf, dropped, pairs):
    """got within one bar of the full reference; every reference with a hand-off left out more than two bars away."""
    bar = _bar(sfx, layers)
    for name, d in dropped.items():
        away = _rel(d, ref_leaf)
        print("%s %s: reference without %s is %.3f away (bar %.4f)" % (what, sfx, name, away, bar))
        assert away > 2.0 * bar, (name, away, bar)
    r = _rel(got_leaf, ref_leaf)
    print("%s %s: d leaf rel L2 %.5f (bar %.4f)" % (what, sfx, r, bar))
    assert r <= bar, (what, r, bar)
    for name, got, ref in pairs:
        r = _rel(got, ref)
        print("%s %s: %s rel L2 %.5f (bar %.4f)" % (what, sfx, name, r, bar))
        assert got.shape == ref.shape and r <= bar, (what, name, r, bar)


def _param_pairs(ref, named):
    out = []
    for name, conv, bn in named:
        q = ref.p[conv]
        out += [(name + " dW", conv.weight.grad, q["w"].grad), (name + " d conv-bias", conv.bias.grad, q["b"].grad),
                (name + " d gamma", bn.weight.grad, q["gamma"].grad), (name + " d beta", bn.bias.grad, q["beta"].grad)]
    return out


def _leaf_grad(ref_out_fn, leaf):
    """d loss / d leaf of the float64 restatement: ref_out_fn(x64) -> [(output, weight of the loss)]."""
    x = leaf.detach().to(torch.float64).requires_grad_()
    loss = sum((o * w.to(torch.float64)).sum() for o, w in ref_out_fn(x))
    loss.backward()
    return x.grad


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_identity_block_shortcut_gradient_against_float64_autograd(sfx, monkeypatch):
    dtype = DTYPES[sfx]
    outs = _recorded(monkeypatch)
    gen = torch.Generator().manual_seed(81)
    block = _block(256, 64, 1, False, seed=82)
    leaf = _act((2, 256, 8, 8), dtype, gen)
    dy = torch.randn((2, 256, 8, 8), generator=gen).to(dtype).to(DEV).contiguous(memory_format=CL)
    y = block(leaf)
    y.backward(dy)
    ref = _Ref(dtype, outs)
    want = _leaf_grad(lambda x: [(ref.block(x, block), dy)], leaf)
    no_shortcut = _leaf_grad(lambda x: [(_Ref(dtype, outs).block(x, block, drop_shortcut=True), dy)], leaf)
    _compare(sfx, 3, "identity block", leaf.grad, want, {"the shortcut": no_shortcut},
             _param_pairs(ref, [("conv1", block.conv1, block.bn1), ("conv3", block.conv3, block.bn3)]))


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_stride_2_projection_block_with_a_lateral_against_float64_autograd(sfx, monkeypatch):
    from feature_intertwiner_amd import train16
    outs = _recorded(monkeypatch)
    from feature_intertwiner_amd.conv import GradBox
    dtype = DTYPES[sfx]
    gen = torch.Generator().manual_seed(83)
    conv0, bn0 = _layer(64, 256, 1, 1, seed=84)
    block = _block(256, 128, 2, True, seed=85)
    leaf = _act((2, 64, 7, 9), dtype, gen)
    dy = torch.randn((2, 512, 4, 5), generator=gen).to(dtype).to(DEV).contiguous(memory_format=CL)
    dz = torch.randn((2, 256, 7, 9), generator=gen).to(DEV)
    x = train16.conv_bn_act16(leaf, conv0, bn0)
    box = block.lateral_box = GradBox()
    y = block(x)
    z = train16.unpack(x, box)
    train16.reset_stats()
    torch.autograd.backward([y, z], [dy, dz])
    assert train16.stats()["fallback"] == 0 and train16.stats()["gated"] == 3 and box.value is None

    def restated(ref, lateral=True, projection=True):
        def fn(x64):
            h = ref.layer(x64, conv0, bn0)
            out = ref.layer(h, block.conv1, block.bn1)
            out = ref.layer(out, block.conv2, block.bn2)
            res = ref.layer(h if projection else h.detach(), block.downsample[0], block.downsample[1], relu=False)
            outs = [(ref.layer(out, block.conv3, block.bn3, res=res), dy)]
            return outs + ([(h, dz)] if lateral else [])
        return fn

    ref = _Ref(dtype, outs)
    want = _leaf_grad(restated(ref), leaf)
    dropped = {"the lateral": _leaf_grad(restated(_Ref(dtype, outs), lateral=False), leaf),
               "the projection's dx": _leaf_grad(restated(_Ref(dtype, outs), projection=False), leaf)}
    _compare(sfx, 5, "stride-2 projection + lateral", leaf.grad, want, dropped,
             _param_pairs(ref, [("producer", conv0, bn0), ("conv1", block.conv1, block.bn1),
                                ("projection", block.downsample[0], block.downsample[1])]))


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_trunk_with_laterals_against_float64_autograd(sfx, monkeypatch):
    from feature_intertwiner_amd import conv as fconv, train16
    outs = _recorded(monkeypatch)
    dtype = DTYPES[sfx]
    net = _trunk(71)
    stages = (net.C2, net.C3, net.C4, net.C5)
    gen = torch.Generator().manual_seed(92)
    leaf = torch.randn((2, 64, 20, 24), generator=gen).to(dtype).to(DEV).contiguous(memory_format=CL).requires_grad_()
    shapes = {2: (2, 256, 20, 24), 3: (2, 512, 10, 12), 4: (2, 1024, 5, 6), 5: (2, 2048, 3, 3)}
    # the weights of the loss: c3's twice, c4's four times c2's, so that each lateral carries a share of the leaf's gradient
    # that its loss would show (asserted below)
    gain = {2: 1.0, 3: 2.0, 4: 4.0, 5: 1.0}
    dz = {lvl: (gain[lvl] * torch.randn(s, generator=gen)).to(DEV) for lvl, s in shapes.items()}
    x, c, boxes = leaf, {}, {}
    for lvl, stage in zip((2, 3, 4, 5), stages):
        if lvl > 2:
            boxes[lvl - 1] = stage[0].lateral_box = fconv.GradBox()
        x = c[lvl] = stage(x)
    z = [train16.unpack(c[lvl], boxes.get(lvl)) for lvl in (2, 3, 4, 5)]
    train16.reset_stats()
    torch.autograd.backward(z, [dz[lvl] for lvl in (2, 3, 4, 5)])
    assert train16.stats()["fallback"] == 0 and train16.stats()["gated"] == 47
    assert all(b.value is None for b in boxes.values())

    def restated(ref, levels):
        def fn(x64):
            outs, h = [], x64
            for lvl, stage in zip((2, 3, 4, 5), stages):
                for b in stage:
                    h = ref.block(h, b)
                if lvl in levels:
                    outs.append((h, dz[lvl]))
            return outs
        return fn

    ref = _Ref(dtype, outs)
    want = _leaf_grad(restated(ref, (2, 3, 4, 5)), leaf)
    dropped = {"the lateral of c%d" % lvl: _leaf_grad(restated(_Ref(dtype, outs), [l for l in (2, 3, 4, 5) if l != lvl]), leaf)
               for lvl in (2, 3, 4)}
    first, last = net.C2[0], net.C5[2]
    _compare(sfx, 52, "trunk + laterals", leaf.grad, want, dropped,
             _param_pairs(ref, [("C2.0 conv1", first.conv1, first.bn1), ("C2.0 projection", first.downsample[0], first.downsample[1]),
                                ("C3.0 conv1", net.C3[0].conv1, net.C3[0].bn1), ("C4.5 conv3", net.C4[5].conv3, net.C4[5].bn3),
                                ("C5.2 conv2", last.conv2, last.bn2)]))


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_a_pair_of_filled_boxes_costs_one_16_bit_add(sfx):
    """dx_add_from=(a, b) with both filled: the layer adds their 16-bit sum in its data-gradient epilogue -- the same bits
    as ONE box holding that sum -- empties both and counts the add; against no box at all the gradient moves by the sum."""
    from feature_intertwiner_amd import train16
    from feature_intertwiner_amd.conv import GradBox
    dtype = DTYPES[sfx]
    gen = torch.Generator().manual_seed(95)
    conv, bn = _layer(64, 96, 3, 1, seed=96)
    leaf = _act((2, 64, 5, 7), dtype, gen)
    dy = torch.randn((2, 96, 5, 7), generator=gen).to(dtype).to(DEV).contiguous(memory_format=CL)
    va, vb = (torch.randn((2, 64, 5, 7), generator=gen).to(dtype).to(DEV).contiguous(memory_format=CL) for _ in range(2))

    def run(values):
        boxes = tuple(GradBox() for _ in values)
        y = train16.conv_bn_act16(leaf, conv, bn, dx_add_from=boxes if len(boxes) != 1 else boxes[0])
        for b, v in zip(boxes, values):
            b.value = v
        leaf.grad = None
        y.backward(dy)
        assert all(b.value is None for b in boxes)
        return leaf.grad.clone()

    train16.reset_stats()
    pair = run((va, vb))
    assert train16.pair_adds() == 1
    one = run(((va + vb).contiguous(memory_format=CL),))
    none = run(())
    assert train16.pair_adds() == 1
    assert pair.is_contiguous(memory_format=CL) and torch.equal(pair.view(torch.int16), one.view(torch.int16))
    # independent of the box code: dx moves by va + vb, up to the roundings of the add and of the two stores
    moved, want = pair.double() - none.double(), va.double() + vb.double()
    slack = UNIT[sfx] * (2.0 * want.abs() + pair.double().abs() + none.double().abs()) + 2.0 ** -24
    assert bool(((moved - want).abs() <= slack).all()) and float(want.abs().max()) > 1.0


def test_a_frozen_stem_is_refused_with_a_message_that_names_the_setting():
    """The 16-bit trunk needs a packed map that requires grad: with the stem frozen the train-mode forward says so."""
    from feature_intertwiner_amd import _lib
    from feature_intertwiner_amd.config import make_config
    from feature_intertwiner_amd.sub_module import FPN, ResNet
    torch.manual_seed(3)
    cfg = make_config("resnet50", 128, 2, 16)
    cfg.TRAIN.ACT_PRECISION = "bf16"
    r = ResNet("resnet50", stage5=True)
    fpn = FPN(cfg, *r.stages(), out_channels=256).to(DEV).eval()
    for p in list(fpn.C1.parameters()):
        p.requires_grad_(False)
    with pytest.raises(_lib.FiError, match="TRAIN.ACT_PRECISION.*stem"):
        fpn(torch.randn(2, 3, 128, 128, device=DEV), mode='train')
