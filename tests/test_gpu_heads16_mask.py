"""The mask head with a graph on 16-bit channels-last crops (sub_module.Mask._forward_train16), bf16 and fp16: Mask(32, 5) on
[3, 32, 14, 14] crops, the loss reading classes (4, 1, 4).

  - forward: the selected logits are torch.equal to the inference launches on the same weights -- four head16.conv_bn_act16,
    head16.deconv2x2_act16, head16.out1x1_16 over all 5 classes -- at column cls[i];
  - counters of one backward: conv2..conv4 and the transposed convolution claim their input's Gate16, so 4 gated data
    gradients and 1 plain one (conv1's, to autograd), 5 weight gradients, ONE class-rows launch, 5 premasked layers (conv1..4
    and the transposed convolution), no fallback and NO relu_grad16;
  - every recorded backward launch replays within its float64 bar on exactly its recorded operands
    (test_gpu_train16_block._replay), the crop gradient being conv1's recorded data gradient;
  - the parameter gradients of conv1..4 / bn1..4 are held to float64 from their recorded (g, x) with the propagated bars of
    tests/test_gpu_grad16_layer.py (test_gpu_train16_block._check_param_grads);
  - the transposed convolution, from ITS recorded (g, x), P = n H W rows: dW[ci, co, a, b] within B(P, sum |g| |x|) of the
    float64 sum; d bias[co] is the fp32 sum over (a, b) of the four column sums the class-rows launch left in the gate:
        |db - ref| <= sum_ab B(P, m_ab) + 4 2^-24 sum_ab (|s_ab| + B(P, m_ab)),     m_ab = sum |g| of column (a, b, co);
  - conv5: d weight and d bias within B(count, sum |terms|) of fp64_ref.class_row_bwd_ref on (d, u); classes without a RoI
    get exactly zero."""
import math

import pytest
import torch

import fp64_ref as R
from test_gpu_grad16_layer import CL, DEV, DTYPES, _B, _held
from test_gpu_train16_block import _check_param_grads, _counts, _record, _replay, _reset

pytestmark = pytest.mark.gpu
N, DEPTH, HW, K = 3, 32, 14, 5


def _mask(seed, depth=DEPTH):
    from feature_intertwiner_amd import sub_module
    gen = torch.Generator().manual_seed(seed)
    m = sub_module.Mask(depth, K)
    with torch.no_grad():
        for conv, bn in ((m.conv1, m.bn1), (m.conv2, m.bn2), (m.conv3, m.bn3), (m.conv4, m.bn4)):
            cout, cin, k, _ = conv.weight.shape
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) / math.sqrt(cin * k * k))
            conv.bias.copy_(0.5 * torch.randn(cout, generator=gen))
            bn.weight.copy_(0.5 + torch.rand(cout, generator=gen))
            bn.weight[::5] *= -1.0
            bn.bias.copy_(0.5 * torch.randn(cout, generator=gen))
            bn.running_mean.copy_(0.5 * torch.randn(cout, generator=gen))
            bn.running_var.copy_(0.25 + torch.rand(cout, generator=gen))
        m.deconv.weight.copy_(torch.randn(m.deconv.weight.shape, generator=gen) / 16.0)
        m.deconv.bias.copy_(0.5 * torch.randn(m.deconv.bias.shape, generator=gen))
        m.conv5.weight.copy_(torch.randn(m.conv5.weight.shape, generator=gen) / 16.0)
        m.conv5.bias.copy_(torch.randn(K, generator=gen))
    return m.to(DEV).eval()


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_mask_head_trains_on_16bit_crops(sfx, monkeypatch):
    from feature_intertwiner_amd import act16, head16, heads16
    dtype = DTYPES[sfx]
    m = _mask(83)
    gen = torch.Generator().manual_seed(89)
    x16 = torch.randn((N, DEPTH, HW, HW), generator=gen).to(dtype).to(DEV).contiguous(memory_format=CL).requires_grad_()
    cls = torch.tensor([4, 1, 4], dtype=torch.int64, device=DEV)
    d = torch.randn((N, 2, 2, HW, HW), generator=gen).to(DEV)
    sel = m(x16, shuffled=False, activate=False, select_class=cls)
    assert sel.dtype == torch.float32 and tuple(sel.shape) == (N, 2, 2, HW, HW) and sel.requires_grad
    with torch.no_grad():
        v = x16.detach()
        for conv, bn in ((m.conv1, m.bn1), (m.conv2, m.bn2), (m.conv3, m.bn3), (m.conv4, m.bn4)):
            v = head16.conv_bn_act16(v, conv, bn, relu=True)
        u = head16.deconv2x2_act16(v, m.deconv, relu=True)
        C = u.shape[1] // 4
        frac = float((u > 0).float().mean())
        assert 0.1 < frac < 0.9, frac
        rows = u.permute(0, 2, 3, 1).reshape(N * HW * HW * 4, C).view(N * HW * HW * 4, C, 1, 1)
        w16 = act16.weight16(m.conv5.weight, dtype).view(K, C)
        full = head16.out1x1_16(rows, w16, m.conv5.bias, act=head16.NONE, layout=head16.ROWS).view(N, HW, HW, 2, 2, K)
        for i in range(N):
            assert torch.equal(sel[i], full[i, :, :, :, :, int(cls[i])].permute(2, 3, 0, 1)), i
    # a 16-bit crop without the training form's arguments is still the inference form, or an error with a graph
    from feature_intertwiner_amd import _lib
    with pytest.raises(_lib.FiError):
        m(x16, shuffled=False, activate=False)

    calls = _record(monkeypatch)
    _reset()
    heads16.reset_stats()
    sel.backward(d)
    torch.cuda.synchronize()
    recorded = list(calls)
    assert _counts() == dict(gated=4, premasked=5, fallback=0, relu_grad=0, dgrad=1, wgrad=5), _counts()
    assert heads16.stats()["class_rows"] == 1
    plain = [c for c in recorded if c[0] == "dgrad16"]
    assert len(plain) == 1 and x16.grad is not None and x16.grad.dtype == dtype
    assert torch.equal(x16.grad.view(torch.int16), plain[0][3].view(torch.int16))          # the crop gradient: conv1's dgrad16
    wg = [c for c in recorded if c[0] == "wgrad16"]
    assert wg[0][1][0].shape[1] == 4 * C                                                   # the transposed convolution's comes first
    layers = [(m.conv4, m.bn4), (m.conv3, m.bn3), (m.conv2, m.bn2), (m.conv1, m.bn1)]
    _check_param_grads([c for c in recorded if c is not wg[0]], layers, sfx, "mask head %s" % sfx)

    # the transposed convolution, from its recorded (g, x)
    g, x = wg[0][1][0], wg[0][1][1].detach()
    P = g.shape[0] * g.shape[2] * g.shape[3]
    cin, cout = m.deconv.weight.shape[0], m.deconv.weight.shape[1]
    to_param = lambda t: t.reshape(2, 2, cout, cin).permute(3, 2, 0, 1)
    ref = to_param(R.wgrad_ref(x, g, 1, 1, (1, 1), (0, 0)))
    mag = to_param(R.wgrad_ref(x.abs(), g.abs(), 1, 1, (1, 1), (0, 0)))
    dw = m.deconv.weight.grad
    assert dw.shape == m.deconv.weight.shape and dw.stride() == m.deconv.weight.stride()
    _held(dw, ref, _B(P, mag), "mask head %s deconv dW" % sfx)
    g64 = g.to(torch.float64)
    s_ab, m_ab = g64.sum((0, 2, 3)).view(4, cout), g64.abs().sum((0, 2, 3)).view(4, cout)
    B_ab = _B(P, m_ab)
    _held(m.deconv.bias.grad, s_ab.sum(0), B_ab.sum(0) + 4.0 * R.U * (s_ab.abs() + B_ab).sum(0), "mask head %s deconv d bias" % sfx)
    # conv5, from (d, u)
    x5 = u.to(torch.float64).reshape(N, 4, C, HW * HW).permute(0, 2, 1, 3).reshape(N, C, 4 * HW * HW)
    _, dw_ref, mw, db_ref, mb, cnt = R.class_row_bwd_ref(d.reshape(N, 4 * HW * HW), x5, w16, cls, K, True)
    R.check_bar(m.conv5.weight.grad.view(K, C), dw_ref, mw, cnt[:, None].expand_as(mw), "conv5 dweight")
    R.check_bar(m.conv5.bias.grad, db_ref, mb, cnt, "conv5 dbias")
    for k in (0, 2, 3):
        assert bool((m.conv5.weight.grad[k] == 0).all()) and float(m.conv5.bias.grad[k]) == 0.0
    # every recorded launch against float64 on its recorded operands
    _replay(recorded, sfx)
