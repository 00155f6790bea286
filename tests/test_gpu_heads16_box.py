"""The box head with a graph on 16-bit channels-last crops (sub_module.Classifier._forward_train16), bf16 and fp16:
Classifier(32, 5, 7) on [6, 32, 7, 7] crops -- the full-window layer 32 x 7 x 7 -> 1024, conv2 1024 -> 1024, the class (5) and box
(20) linears as one stacked output layer.

  - forward: logits and boxes are torch.equal to the inference _forward16 on the same weights;
  - counters of one backward: conv2 and the output layer claim their input's Gate16, so 2 gated data gradients and 1 plain
    one (the full-window layer's, to autograd), 3 weight gradients, 2 premasked layers, no fallback and NO relu_grad16;
  - every recorded backward launch replays within its float64 bar on exactly its recorded operands
    (test_gpu_train16_block._replay); the crop gradient is the full-window layer's recorded data gradient, re-viewed;
  - conv2 / bn2 and conv1 / bn1 are held to float64 from their recorded (g, x) with the propagated bars of
    tests/test_gpu_grad16_layer.py (test_gpu_train16_block._check_param_grads) -- the full-window layer AS the 1x1 layer on
    the crop's [7, 7, 32] run that its backward runs, its weight and weight gradient re-viewed in that order;
  - the output layer: its recorded g is the fp32 gradient zero-padded from 25 to 32 columns and rounded once; the two
    linears' weight gradients are rows 0..4 and 5..24 of the float64 product within B(6, sum |g| |x|); their bias gradients
    are the fp32 column sums of the gradient within B(6, sum |d|)."""
import math
import types

import pytest
import torch

import fp64_ref as R
from test_gpu_grad16_layer import CL, DEV, DTYPES, _B, _held
from test_gpu_train16_block import _check_param_grads, _counts, _record, _replay, _reset

pytestmark = pytest.mark.gpu
N, DEPTH, POOL, K = 6, 32, 7, 5


def _head(seed, depth=DEPTH):
    from feature_intertwiner_amd import sub_module
    from feature_intertwiner_amd.config import make_config
    cfg = make_config("resnet50", 256, 2, 64, dev_switch=True, loss_choice="ot", ot_L=5)
    gen = torch.Generator().manual_seed(seed)
    c = sub_module.Classifier(depth, K, POOL, cfg)
    with torch.no_grad():
        for conv, bn in ((c.conv1, c.bn1), (c.conv2, c.bn2)):
            cout, cin, k, _ = conv.weight.shape
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) / math.sqrt(cin * k * k))
            conv.bias.copy_(0.5 * torch.randn(cout, generator=gen))
            bn.weight.copy_(0.5 + torch.rand(cout, generator=gen))
            bn.weight[::5] *= -1.0
            bn.bias.copy_(0.5 * torch.randn(cout, generator=gen))
            bn.running_mean.copy_(0.5 * torch.randn(cout, generator=gen))
            bn.running_var.copy_(0.25 + torch.rand(cout, generator=gen))
        for lin in (c.linear_class, c.linear_bbox):
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=gen) / 32.0)
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=gen))
    return c.to(DEV).eval()


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_box_head_trains_on_16bit_crops(sfx, monkeypatch):
    dtype = DTYPES[sfx]
    c = _head(97)
    gen = torch.Generator().manual_seed(101)
    x16 = torch.randn((N, DEPTH, POOL, POOL), generator=gen).to(dtype).to(DEV).contiguous(memory_format=CL).requires_grad_()
    logits, probs, bbox = c(x16)
    assert logits.dtype == torch.float32 and tuple(logits.shape) == (N, K) and tuple(bbox.shape) == (N, K, 4)
    assert logits.requires_grad and bbox.requires_grad
    with torch.no_grad():
        want = c(x16.detach())
    assert torch.equal(logits, want[0]) and torch.equal(probs, want[1]) and torch.equal(bbox, want[2])
    dl = torch.randn((N, K), generator=gen).to(DEV)
    db = torch.randn((N, K, 4), generator=gen).to(DEV)

    calls = _record(monkeypatch)
    _reset()
    torch.autograd.backward([logits, bbox], [dl, db])
    torch.cuda.synchronize()
    recorded = list(calls)
    assert _counts() == dict(gated=2, premasked=2, fallback=0, relu_grad=0, dgrad=1, wgrad=3), _counts()
    plain = [r for r in recorded if r[0] == "dgrad16"]
    assert len(plain) == 1 and x16.grad is not None and x16.grad.dtype == dtype
    assert torch.equal(x16.grad.permute(0, 2, 3, 1).reshape(N, -1).view(torch.int16),
                       plain[0][3].reshape(N, -1).view(torch.int16))
    wg = [r for r in recorded if r[0] == "wgrad16"]
    assert [r[1][0].shape[1] for r in wg] == [32, 1024, 1024]          # the output layer (25 -> 32 columns), conv2, conv1
    _check_param_grads([wg[1]], [(c.conv2, c.bn2)], sfx, "box head %s conv2" % sfx)
    # the full-window layer as the 1x1 layer its backward runs: weight and gradient in the crop's [7, 7, 32] order
    as_rows = lambda t: t.detach().permute(0, 2, 3, 1).reshape(t.shape[0], -1, 1, 1).contiguous()
    w_rows = as_rows(c.conv1.weight)
    w_rows.grad = as_rows(c.conv1.weight.grad)
    assert c.conv1.weight.grad.shape == c.conv1.weight.shape and c.conv1.weight.grad.stride() == c.conv1.weight.stride()
    window = types.SimpleNamespace(weight=w_rows, bias=c.conv1.bias, kernel_size=(1, 1), stride=(1, 1), padding=(0, 0))
    _check_param_grads([wg[2]], [(window, c.bn1)], sfx, "box head %s full window" % sfx)
    # the stacked output layer
    g, x = wg[0][1][0], wg[0][1][1].detach()
    d = torch.cat((dl, db.reshape(N, 4 * K)), 1)
    assert torch.equal(g.reshape(N, 32)[:, :5 * K], d.to(dtype)) and bool((g.reshape(N, 32)[:, 5 * K:] == 0).all())
    ref = R.wgrad_ref(x, g, 1, 1, (1, 1), (0, 0)).reshape(32, -1)
    bar = _B(N, R.wgrad_ref(x.abs(), g.abs(), 1, 1, (1, 1), (0, 0)).reshape(32, -1))
    _held(c.linear_class.weight.grad, ref[:K], bar[:K], "box head %s d linear_class" % sfx)
    _held(c.linear_bbox.weight.grad, ref[K:5 * K], bar[K:5 * K], "box head %s d linear_bbox" % sfx)
    d64 = d.to(torch.float64)
    _held(torch.cat((c.linear_class.bias.grad, c.linear_bbox.bias.grad)), d64.sum(0), _B(N, d64.abs().sum(0)),
          "box head %s d linear biases" % sfx)
    # every recorded launch against float64 on its recorded operands
    _replay(recorded, sfx)
