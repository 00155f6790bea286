"""fpn16.lateral16 / fpn16.conv_bias_act16: the feature pyramid's layers on 16-bit channels-last tensors that require grad.

A chain of three laterals at the real channel counts under a P5_conv1-like layer that produces their top, and a smoothing
layer on each of the four levels, with conv.GATES on and off:
    c5 [2, 2048, 2, 3] -> top [2, 256, 2, 3];  c4 [2, 1024, 4, 6], c3 [2, 512, 8, 12], c2 [2, 256, 16, 24].
What is held: the forward's bits equal pyr16's under no_grad; the counters are the design's (derived below); with GATES on
no lateral returns a top gradient to autograd and a lateral's dx goes to a box whose taker flag is up; each g_l is
torch.equal to the header's fp32 expression on the operands its launch was recorded with; every recorded wgrad / dgrad
launch replays within its float64 bar on exactly its recorded operands (test_gpu_train16_block._replay); and the
parameter gradients as they reach the parameters are held to float64 from the (g, x) of their recorded launch with the bars
of tests/test_gpu_grad16_layer.py for a layer without a fold (scale 1: no product, so dW keeps the weight gradient's own
bar B_w and d bias the column sums' bar B_s).  Every g stays above 2^-14 (asserted): the regime the bars are stated for.

Counters, eight layers.  Every layer runs one wgrad16 and one dgrad16: 8 and 8, no relu_grad16, no gated launch (the
leaves carry no gate).  fi_fpn16_topdown_grad, GATES on: the four smoothing layers and the finest lateral have nothing to add
and only sum (5 'sums'), the two coarser laterals and the top's layer add what the box holds (3 'topdown'), 0
'top_to_autograd'.  GATES off: each of the three laterals returns the 2 x 2 sums of its g to autograd (3 'topdown', 3
'top_to_autograd'), autograd adds them, and all eight layers only sum (8 'sums').

Two single layers besides: a bias-only layer behind a conv + BatchNorm + ReLU layer claims that layer's Gate16 (one gated
data gradient, the producer premasked, the same bits into the leaf as with GATES off), and a bias-only layer WITH a ReLU
adds what its box holds before it masks."""
import math

import pytest
import torch

import fp64_ref as R
from test_gpu_grad16_layer import CL, DEV, DTYPES, _B, _act, _held
from test_gpu_train16_block import _counts, _dy, _record, _replay, _reset, _zero_grads

pytestmark = pytest.mark.gpu


def _bias_conv(cin, cout, k, seed, weight_cl=False):
    from feature_intertwiner_amd.conv import Conv2d
    gen = torch.Generator().manual_seed(seed)
    conv = Conv2d(cin, cout, kernel_size=k, stride=1, padding=(k - 1) // 2)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) / math.sqrt(cin * k * k))
        conv.bias.copy_(0.5 * torch.randn(cout, generator=gen))
    conv = conv.to(DEV)
    if weight_cl:
        conv.weight.data = conv.weight.data.contiguous(memory_format=CL)
    return conv


def _record_topdown(monkeypatch):
    from feature_intertwiner_amd import fpn16
    calls = []

    def rec(own, fine, colsum=True, out=None, _fn=fpn16.topdown_grad16):
        res = _fn(own, fine, colsum=colsum, out=out)
        calls.append((own, fine, res[0], res[1]))
        return res
    monkeypatch.setattr(fpn16, "topdown_grad16", rec)
    return calls


def _check_topdown_calls(tcalls, dtype):
    """Each recorded launch: g is the header's expression on (own, fine), the sums are within relu_grad's bar of float64."""
    for own, fine, g, s in tcalls:
        if fine is None:
            assert g is own
        else:
            f = fine.float()
            t = (f[:, :, 0::2, 0::2] + f[:, :, 0::2, 1::2]) + (f[:, :, 1::2, 0::2] + f[:, :, 1::2, 1::2])
            want = (t if own is None else own.float() + t).to(dtype)
            assert torch.equal(g.view(torch.int16), want.view(torch.int16))
        if s is not None:
            g64 = g.to(torch.float64)
            P = g.shape[0] * g.shape[2] * g.shape[3]
            _held(s, g64.sum((0, 2, 3)), _B(P, g64.abs().sum((0, 2, 3))), "topdown colsum")


def _check_bias_layer_grads(calls, convs, what):
    """The parameter gradients of bias-only `convs` (in backward order) against float64, from the (g, x) each layer's
    weight gradient was recorded with."""
    wg = [c for c in calls if c[0] == "wgrad16"]
    assert len(wg) == len(convs)
    for conv, (_, a, _, _) in zip(convs, wg):
        g, x16, k, _, stride, pad = a
        x16 = x16.detach()
        Cout, Cin = conv.weight.shape[0], conv.weight.shape[1]
        assert (k, stride, pad) == (conv.kernel_size[0], conv.stride[0], conv.padding[0]) and g.shape[1] == Cout
        assert float(g.float().abs().max()) > 2.0 ** -14
        P = g.shape[0] * g.shape[2] * g.shape[3]
        st, pd = (stride, stride), (pad, pad)
        g64 = g.to(torch.float64)
        tag = "%s %dx%d %d->%d" % (what, k, k, Cin, Cout)
        db = conv.bias.grad
        assert db.dtype == torch.float32 and tuple(db.shape) == (Cout,)
        _held(db, g64.sum((0, 2, 3)), _B(P, g64.abs().sum((0, 2, 3))), tag + " d bias")
        dw = conv.weight.grad
        assert dw.dtype == torch.float32 and dw.shape == conv.weight.shape and dw.stride() == conv.weight.stride()
        _held(dw, R.wgrad_ref(x16, g, k, k, st, pd), _B(P, R.wgrad_ref(x16.abs(), g.abs(), k, k, st, pd)), tag + " dW")


def _fpn_counts():
    from feature_intertwiner_amd import fpn16
    s = fpn16.stats()
    return dict(topdown=s["topdown"], sums=s["sums"], top_to_autograd=s["top_to_autograd"])


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_three_laterals_under_a_top_layer_with_gates_on_and_off(sfx, monkeypatch):
    from feature_intertwiner_amd import conv as fconv, fpn16, pyr16
    dtype = DTYPES[sfx]
    gen = torch.Generator().manual_seed(91)
    P5 = _bias_conv(2048, 256, 1, seed=92)
    lat = {4: _bias_conv(1024, 256, 1, seed=93), 3: _bias_conv(512, 256, 1, seed=94), 2: _bias_conv(256, 256, 1, seed=95)}
    smooth = {l: _bias_conv(256, 256, 3, seed=96 + l, weight_cl=(l == 3)) for l in (5, 4, 3, 2)}
    hw = {5: (2, 3), 4: (4, 6), 3: (8, 12), 2: (16, 24)}
    cin = {5: 2048, 4: 1024, 3: 512, 2: 256}
    c = {l: _act((2, cin[l]) + hw[l], dtype, gen) for l in (5, 4, 3, 2)}
    dys = [_dy((2, 256) + hw[l], dtype, gen) for l in (5, 4, 3, 2)]
    modules = [P5] + list(lat.values()) + list(smooth.values())
    # the backward visits: the smoothing layers finest first (the last applied), then the laterals finest first, then P5
    order = [smooth[2], smooth[3], smooth[4], smooth[5], lat[2], lat[3], lat[4], P5]
    calls = _record(monkeypatch)
    tcalls = _record_topdown(monkeypatch)
    seen = {}

    def forward(gates):
        top = {l: fconv.GradBox() if gates else None for l in (5, 4, 3)}
        give = fconv.GradBox()
        give.taker = gates                                            # level 3's dx has a taker, as a trunk stage would be
        pre = {5: fpn16.conv_bias_act16(c[5], P5, gate_dx=True, top_grad_from=top[5])}
        pre[4] = fpn16.lateral16(c[4], lat[4], pre[5], top_grad_to=top[5], top_grad_from=top[4], dx_give_to=fconv.GradBox())
        pre[3] = fpn16.lateral16(c[3], lat[3], pre[4], top_grad_to=top[4], top_grad_from=top[3], dx_give_to=give)
        pre[2] = fpn16.lateral16(c[2], lat[2], pre[3], top_grad_to=top[3])
        outs = [fpn16.conv_bias_act16(pre[l], smooth[l]) for l in (5, 4, 3, 2)]
        seen["pre"], seen["outs"], seen["give"] = {l: t.detach() for l, t in pre.items()}, [o.detach() for o in outs], give
        seen["top"] = top
        return outs

    grads = {}
    for gates in (True, False):
        prev, fconv.GATES = fconv.GATES, gates
        try:
            _zero_grads(modules)
            for t in c.values():
                t.grad = None
            del calls[:], tcalls[:]
            outs = forward(gates)
            _reset()
            fpn16.reset_stats()
            torch.autograd.backward(outs, dys)
            torch.cuda.synchronize()
        finally:
            fconv.GATES = prev
        cnt = _counts()
        assert cnt == dict(gated=0, premasked=0, fallback=0, relu_grad=0, dgrad=8, wgrad=8), (gates, cnt)
        want = dict(topdown=3, sums=5, top_to_autograd=0) if gates else dict(topdown=3, sums=8, top_to_autograd=3)
        assert _fpn_counts() == want, (gates, _fpn_counts())
        if gates:
            # level 3's data gradient went through the box with a taker; the box without one was not used
            assert c[3].grad is None and seen["give"].value is not None
            dx3 = seen["give"].value
            assert dx3.dtype == dtype and tuple(dx3.shape) == tuple(c[3].shape) and dx3.is_contiguous(memory_format=CL)
            assert all(b.value is None for b in seen["top"].values())            # every top box was emptied by its taker
        else:
            dx3 = c[3].grad
        grads[gates] = [c[5].grad, c[4].grad, dx3, c[2].grad]
        for t in grads[gates]:
            assert t.dtype == dtype and bool(torch.isfinite(t.float()).all()) and float(t.float().abs().max()) > 0.0
        _check_topdown_calls(list(tcalls), dtype)
        _check_bias_layer_grads(list(calls), order, "pyramid %s %s" % (sfx, "boxes" if gates else "autograd"))
        _replay(list(calls), sfx)
    # the forward: pyr16's launches under no_grad
    with torch.no_grad():
        pre = {5: pyr16.conv_bias_act16(c[5].detach(), P5)}
        for l in (4, 3, 2):
            pre[l] = pyr16.lateral16(c[l].detach(), lat[l], pre[l + 1])
        outs0 = [pyr16.conv_bias_act16(pre[l], smooth[l]) for l in (5, 4, 3, 2)]
    for l in (5, 4, 3, 2):
        assert torch.equal(seen["pre"][l].view(torch.int16), pre[l].view(torch.int16))
    for a, b in zip(seen["outs"], outs0):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and bool(torch.isfinite(a.float()).all())
    # the two routes differ by where the 2 x 2 sums are rounded, not in what they compute
    for a, b in zip(grads[True], grads[False]):
        assert float((a.float() - b.float()).abs().max()) <= 0.05 * float(b.float().abs().max())


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_the_top_layer_claims_its_input_s_gate(sfx, monkeypatch):
    """x = a 16-bit conv + BN + ReLU layer's output (it carries a Gate16) and the bias-only layer its only reader: one gated
    data gradient, the producer is premasked and runs no relu_grad16; with GATES off it masks and sums itself.  Both give
    the leaf the same bits."""
    from feature_intertwiner_amd import conv as fconv, fpn16, train16
    from test_gpu_grad16_layer import _layer
    from test_gpu_train16_block import _check_param_grads
    dtype = DTYPES[sfx]
    gen = torch.Generator().manual_seed(97)
    conv0, bn0 = _layer(64, 512, 1, 1, seed=98)
    P5 = _bias_conv(512, 256, 1, seed=99)
    leaf = _act((2, 64, 5, 7), dtype, gen)
    dy = _dy((2, 256, 5, 7), dtype, gen)
    calls = _record(monkeypatch)
    got = {}
    for gates in (True, False):
        prev, fconv.GATES = fconv.GATES, gates
        try:
            _zero_grads([conv0, bn0, P5])
            leaf.grad = None
            del calls[:]
            y = fpn16.conv_bias_act16(train16.conv_bn_act16(leaf, conv0, bn0), P5, gate_dx=True)
            _reset()
            fpn16.reset_stats()
            y.backward(dy)
            torch.cuda.synchronize()
        finally:
            fconv.GATES = prev
        n = 1 if gates else 0
        assert _counts() == dict(gated=n, premasked=n, fallback=0, relu_grad=1 - n, dgrad=2 - n, wgrad=2), (gates, _counts())
        assert _fpn_counts() == dict(topdown=0, sums=1, top_to_autograd=0)
        got[gates] = leaf.grad.clone()
        _check_bias_layer_grads([c for c in calls if c[0] == "wgrad16"][:1], [P5], "top layer %s" % sfx)
        _check_param_grads([c for c in calls if c[0] == "wgrad16"][1:], [(conv0, bn0)], sfx, "producer %s" % sfx)
        _replay(list(calls), sfx)
    assert torch.equal(got[True].view(torch.int16), got[False].view(torch.int16))


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_a_bias_layer_with_a_relu_masks_after_the_add(sfx, monkeypatch):
    """conv_bias_act16(relu=True) with a finer gradient waiting in its box: the 2 x 2 sums are added to dy first (one
    fi_fpn16_topdown_grad launch, no sums), then relu_grad16 masks with the layer's own y and sums -- g = (dy + sums) *
    (y > 0) exactly; the forward is pyr16's launch."""
    from feature_intertwiner_amd import conv as fconv, fpn16, pyr16
    dtype = DTYPES[sfx]
    gen = torch.Generator().manual_seed(101)
    layer = _bias_conv(64, 96, 3, seed=102)
    x = _act((2, 64, 5, 7), dtype, gen)
    dy = _dy((2, 96, 5, 7), dtype, gen)
    fine = _dy((2, 96, 10, 14), dtype, gen)
    calls = _record(monkeypatch)
    tcalls = _record_topdown(monkeypatch)
    box = fconv.GradBox()
    y = fpn16.conv_bias_act16(x, layer, relu=True, top_grad_from=box)
    assert box.taker
    box.value = fine                                                 # what a finer lateral's backward would leave
    _reset()
    fpn16.reset_stats()
    y.backward(dy)
    torch.cuda.synchronize()
    assert box.value is None
    assert _counts() == dict(gated=0, premasked=0, fallback=0, relu_grad=1, dgrad=1, wgrad=1)
    assert _fpn_counts() == dict(topdown=1, sums=0, top_to_autograd=0)
    _check_topdown_calls(list(tcalls), dtype)
    (own, f, summed, s), = tcalls
    assert own is not None and f is fine and s is None
    name, a, kw, (g, _) = calls[0]
    assert name == "relu_grad16" and a[0] is summed
    assert torch.equal(g, summed * (y.detach() > 0).to(dtype)) and 0 < int(torch.count_nonzero(g)) < g.numel()
    _check_bias_layer_grads(list(calls), [layer], "relu layer %s" % sfx)
    _replay(list(calls), sfx)
    with torch.no_grad():
        y0 = pyr16.conv_bias_act16(x.detach(), layer, relu=True)
    assert torch.equal(y.detach().view(torch.int16), y0.view(torch.int16))
