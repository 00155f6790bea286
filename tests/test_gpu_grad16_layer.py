"""grad16.conv_bn_act16: the differentiable conv + eval-BatchNorm (+ shortcut) + ReLU layer on 16-bit channels-last tensors.

The forward's bits equal act16.conv_bn_act16 under no_grad; every gradient autograd returns is held to float64.  The
reference takes the ReLU mask from the kernel's OWN y (g = dy * (y > 0) is then exact, a select) and the data gradient's
weight AS ROUNDED (grad16.weight_t16); d gamma / d conv-bias / dW go through fp64_ref.fold_grad_ref.  The bars are those of
tests/test_gpu_grad16_kernels.py, with B(n, m) = 2^-24 (4 sqrt(n) + 16) m, propagated through fi_bn_fold_grad:
    s  = d beta   B_s  = B(P, sum |g|)                                           P = N OH OW
    dW'           B_w  = B(P, wgrad on absolute values)
    dW = scale dW'       |scale| B_w + 2^-24 (|ref| + |scale| B_w)               (one fp32 product)
    d gamma       inv_std (sum_k |W_k| B_w,k + |cb - mean| B_s)  +  B(K, m)      K = Cin R S; the first term is what the
                  errors of dW' and s become in the exact formula, the second fi_bn_fold_grad's own sum with
                  m = inv_std (sum_k |W_k| (|dW'_k| + B_w,k) + |cb - mean| (|s| + B_s))
    d conv-bias   |scale| B_s + B(1, |scale| (|s| + B_s))
    dx            B + u (|ref| + B) + s16,  B = B(Cout R S, dgrad on absolute values)    (tests/test_gpu_grad16_kernels.py)
"""
import math

import pytest
import torch

import fp64_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
UNIT = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
SUBNORMAL = {"bf16": 0.0, "f16": 2.0 ** -25}
CL = torch.channels_last

# (N, H, W, Cin, Cout, k, stride)
LAYERS = [(2, 13, 11, 96, 160, 3, 1), (2, 7, 9, 64, 128, 1, 2)]
_ids = lambda s: "x".join(map(str, s))


def _B(n, mag):
    return R.U * (4.0 * math.sqrt(n) + 16.0) * mag


def _held(got, ref, allow, what):
    got = got.to(torch.float64)
    d = (got - ref).abs()
    d = torch.where(torch.isfinite(got), d, torch.full_like(d, float("inf")))
    ratio = torch.where(d == 0, torch.zeros_like(d), d / allow)
    worst = float(ratio.max())
    print("%s: worst |d| / bar = %.3f" % (what, worst))
    if not worst <= 1.0:
        k = int(torch.argmax(ratio.reshape(-1)))
        raise AssertionError("%s: element %d off the bar by %.3gx (got %r, ref %r)" % (
            what, k, worst, float(got.reshape(-1)[k]), float(ref.reshape(-1)[k])))


def _layer(cin, cout, k, stride, seed, bias=True, weight_cl=False):
    """A conv + eval-mode BatchNorm with non-trivial parameters and running statistics."""
    gen = torch.Generator().manual_seed(seed)
    conv = torch.nn.Conv2d(cin, cout, k, stride=stride, padding=(k - 1) // 2, bias=bias)
    bn = torch.nn.BatchNorm2d(cout, eps=1e-3)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) / math.sqrt(cin * k * k))
        if bias:
            conv.bias.copy_(0.5 * torch.randn(cout, generator=gen))
        bn.weight.copy_(0.5 + torch.rand(cout, generator=gen))
        bn.weight[::5] *= -1.0
        bn.bias.copy_(0.5 * torch.randn(cout, generator=gen))
        bn.running_mean.copy_(0.5 * torch.randn(cout, generator=gen))
        bn.running_var.copy_(0.25 + torch.rand(cout, generator=gen))
    conv, bn = conv.to(DEV), bn.to(DEV)
    if weight_cl:
        conv.weight.data = conv.weight.data.contiguous(memory_format=CL)
    bn.eval()
    return conv, bn


def _act(shape, dtype, gen, scale=1.0):
    """A 16-bit channels-last [N, C, H, W] leaf."""
    t = (scale * torch.randn(shape, generator=gen)).to(dtype).to(DEV).contiguous(memory_format=CL)
    return t.requires_grad_()


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _check_layer_backward(sfx, conv, bn, x16, y, dy, got, what):
    """got: dict of the gradients autograd returned for x / w / b / gamma / beta / res (each may be absent)."""
    from feature_intertwiner_amd import grad16
    dtype = DTYPES[sfx]
    k, stride, pad = conv.kernel_size[0], conv.stride[0], conv.padding[0]
    N, Cin, H, W = x16.shape
    Cout, OH, OW = y.shape[1], y.shape[2], y.shape[3]
    P, K = N * OH * OW, Cin * k * k
    st, pd = (stride, stride), (pad, pad)
    scale = bn._fi_fold[0]
    g = dy * (y > 0).to(dtype)                                       # exact: the kernel's own mask
    g64 = g.to(torch.float64)
    s_ref, s_mag = g64.sum((0, 2, 3)), g64.abs().sum((0, 2, 3))
    B_s = _B(P, s_mag)
    dwp = R.wgrad_ref(x16.detach(), g, k, k, st, pd)                 # [Cout, Cin, R, S]
    B_w = _B(P, R.wgrad_ref(x16.detach().abs(), g.abs(), k, k, st, pd))
    w64 = conv.weight.detach().to(torch.float64)
    cb = conv.bias.detach() if conv.bias is not None else None
    dW, dgam, _, dcb, _ = R.fold_grad_ref(dwp.reshape(Cout, Cin, -1), w64.reshape(Cout, Cin, -1), s_ref, scale,
                                          bn.running_mean, bn.running_var, bn.eps, cb)
    inv = 1.0 / torch.sqrt(bn.running_var.to(torch.float64) + bn.eps)
    sc = scale.to(torch.float64).abs()
    off = ((cb.to(torch.float64) if cb is not None else 0.0) - bn.running_mean.to(torch.float64)).abs()
    if "res" in got:
        assert got["res"].dtype == dtype and got["res"].is_contiguous(memory_format=CL)
        assert torch.equal(got["res"], g), what + " d residual"
    if "beta" in got:
        assert got["beta"].dtype == torch.float32 and tuple(got["beta"].shape) == (Cout,)
        _held(got["beta"], s_ref, B_s, what + " d beta")
    if "w" in got:
        dw = got["w"]
        assert dw.dtype == torch.float32 and tuple(dw.shape) == (Cout, Cin, k, k)
        assert tuple(dw.stride()) == (k * k * Cin, 1, k * Cin, Cin)              # a view of the tap-major buffer
        ref = dW.reshape(Cout, Cin, k, k)
        scB = sc.view(-1, 1, 1, 1) * B_w
        _held(dw, ref, scB + R.U * (ref.abs() + scB), what + " dW")
    if "gamma" in got:
        assert got["gamma"].dtype == torch.float32 and tuple(got["gamma"].shape) == (Cout,)
        wa = w64.abs().reshape(Cout, -1)
        carried = inv * ((wa * B_w.reshape(Cout, -1)).sum(1) + off * B_s)
        m = inv * ((wa * (dwp.abs().reshape(Cout, -1) + B_w.reshape(Cout, -1))).sum(1) + off * (s_ref.abs() + B_s))
        _held(got["gamma"], dgam, carried + _B(K, m), what + " d gamma")
    if "b" in got:
        _held(got["b"], dcb, sc * B_s + _B(1, sc * (s_ref.abs() + B_s)), what + " d conv bias")
    if "x" in got:
        dx = got["x"]
        assert dx.dtype == dtype and tuple(dx.shape) == (N, Cin, H, W) and dx.is_contiguous(memory_format=CL)
        wt = grad16.weight_t16(conv, bn, scale, dtype)               # as rounded, from the registry
        assert tuple(wt.shape) == (Cin, k, k, Cout) and wt.dtype == dtype and wt.is_contiguous()
        w_l = wt.flip(1, 2).permute(3, 0, 1, 2)
        ref = R.dgrad_ref(g, w_l, st, pd, (H, W))
        B = _B(Cout * k * k, R.dgrad_ref(g.abs(), w_l.abs(), st, pd, (H, W)))
        _held(dx, ref, B + UNIT[sfx] * (ref.abs() + B) + SUBNORMAL[sfx], what + " dx")
        # ... and wt itself: scale folded in fp32, taps flipped, transposed, ONE rounding
        want = (conv.weight.detach() * scale.view(-1, 1, 1, 1)).flip(2, 3).permute(1, 2, 3, 0).to(dtype)
        assert torch.equal(wt, want)


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("shape", LAYERS, ids=_ids)
def test_layer_forward_bits_and_gradients(shape, with_res, sfx):
    from feature_intertwiner_amd import act16, grad16
    N, H, W, Cin, Cout, k, stride = shape
    dtype = DTYPES[sfx]
    conv, bn = _layer(Cin, Cout, k, stride, seed=sum(shape))
    gen = torch.Generator().manual_seed(3 + sum(shape))
    x16 = _act((N, Cin, H, W), dtype, gen)
    pad = (k - 1) // 2
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    res = _act((N, Cout, OH, OW), dtype, gen) if with_res else None
    with torch.no_grad():
        y0 = act16.conv_bn_act16(x16, conv, bn, relu=True, residual=res)
    y = grad16.conv_bn_act16(x16, conv, bn, relu=True, residual=res)
    assert y.requires_grad and y.dtype == dtype and y.is_contiguous(memory_format=CL)
    assert torch.equal(y.view(torch.int16), y0.view(torch.int16))                # the same single launch
    assert 0 < int(torch.count_nonzero(y)) < y.numel()
    dy = torch.randn(y.shape, generator=gen).to(dtype).to(DEV).contiguous(memory_format=CL)
    leaves = [("x", x16), ("w", conv.weight), ("b", conv.bias), ("gamma", bn.weight), ("beta", bn.bias)]
    if with_res:
        leaves.append(("res", res))
    grad16.reset_stats()
    grads = torch.autograd.grad(y, [t for _, t in leaves], dy)
    assert grad16.stats() == {"relu_grad": 1, "dgrad": 1, "wgrad": 1, "weights": 1}
    got = {name: gr for (name, _), gr in zip(leaves, grads)}
    _check_layer_backward(sfx, conv, bn, x16, y.detach(), dy, got, "%s %s%s" % (sfx, shape, " + residual" if with_res else ""))


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_no_data_gradient_launch_when_the_input_needs_none(sfx):
    from feature_intertwiner_amd import grad16
    dtype = DTYPES[sfx]
    conv, bn = _layer(64, 128, 1, 2, seed=5)
    gen = torch.Generator().manual_seed(6)
    x16 = _act((2, 64, 7, 9), dtype, gen).detach()
    y = grad16.conv_bn_act16(x16, conv, bn)
    grad16.reset_stats()
    y.float().sum().backward()
    assert grad16.stats() == {"relu_grad": 1, "dgrad": 0, "wgrad": 1, "weights": 0}
    assert conv.weight.grad is not None and bn.weight.grad is not None and bn.bias.grad is not None
    assert tuple(conv.weight.grad.shape) == tuple(conv.weight.shape)


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_the_scaled_transposed_weight_is_rebuilt_when_its_sources_change_and_not_before(sfx):
    from feature_intertwiner_amd import grad16
    dtype = DTYPES[sfx]
    conv, bn = _layer(32, 64, 3, 1, seed=9, bias=False)
    gen = torch.Generator().manual_seed(10)
    x16 = _act((1, 32, 5, 6), dtype, gen)

    def step():
        y = grad16.conv_bn_act16(x16, conv, bn)
        torch.autograd.grad(y.float().sum(), [x16])
        return grad16.weight_t16(conv, bn, bn._fi_fold[0], dtype)

    grad16.reset_stats()
    a = step()
    assert grad16.stats()["weights"] == 1
    b = step()
    assert grad16.stats()["weights"] == 1 and b is a                 # not before
    with torch.no_grad():
        conv.weight.mul_(0.5)
    c = step()
    assert grad16.stats()["weights"] == 2 and c is not a             # the weight changed in place
    want = (conv.weight.detach() * bn._fi_fold[0].view(-1, 1, 1, 1)).flip(2, 3).permute(1, 2, 3, 0).to(dtype)
    assert torch.equal(c, want)
    with torch.no_grad():
        bn.weight.mul_(2.0)
    d = step()
    assert grad16.stats()["weights"] == 3 and d is not c             # the fold changed
    want = (conv.weight.detach() * bn._fi_fold[0].view(-1, 1, 1, 1)).flip(2, 3).permute(1, 2, 3, 0).to(dtype)
    assert torch.equal(d, want)
    assert step() is d and grad16.stats()["weights"] == 3


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_three_layer_bottleneck_runs_and_every_backward_launch_replays_within_the_bars(sfx, monkeypatch):
    """1x1 64 -> 64, 3x3 64 -> 64 (its weight stored channels-last), 1x1 64 -> 256 with a 16-bit shortcut, on 2 x 8 x 8.
    The backward launches are recorded with their inputs and outputs; each is then held to float64 on exactly those."""
    from feature_intertwiner_amd import grad16
    dtype = DTYPES[sfx]
    gen = torch.Generator().manual_seed(21)
    l1 = _layer(64, 64, 1, 1, seed=31)
    l2 = _layer(64, 64, 3, 1, seed=32, weight_cl=True)
    l3 = _layer(64, 256, 1, 1, seed=33)
    x16 = _act((2, 64, 8, 8), dtype, gen)
    res = _act((2, 256, 8, 8), dtype, gen)
    calls = []
    for name in ("relu_grad16", "wgrad16", "dgrad16"):
        def rec(*a, _fn=getattr(grad16, name), _name=name, **kw):
            out = _fn(*a, **kw)
            calls.append((_name, a, kw, out))
            return out
        monkeypatch.setattr(grad16, name, rec)
    h1 = grad16.conv_bn_act16(x16, *l1)
    h2 = grad16.conv_bn_act16(h1, *l2)
    y = grad16.conv_bn_act16(h2, *l3, relu=True, residual=res)
    dy = torch.randn(y.shape, generator=gen).to(dtype).to(DEV).contiguous(memory_format=CL)
    grad16.reset_stats()
    y.backward(dy)
    torch.cuda.synchronize()
    assert grad16.stats() == {"relu_grad": 3, "dgrad": 3, "wgrad": 3, "weights": 3}
    params = [p for conv, bn in (l1, l2, l3) for p in (conv.weight, conv.bias, bn.weight, bn.bias)]
    for t in [x16, res] + params:
        assert t.grad is not None and bool(torch.isfinite(t.grad.float()).all())
        assert float(t.grad.float().abs().max()) > 0.0
    assert x16.grad.dtype == dtype and res.grad.dtype == dtype
    assert [c[0] for c in calls] == ["relu_grad16", "wgrad16", "dgrad16"] * 3
    for name, a, kw, out in list(calls):                             # (the replayed launches are recorded too)
        if name == "relu_grad16":
            dyi, yi = a[0], a[1]
            g, s = out
            want = dyi * (yi > 0).to(dtype)
            assert torch.equal(g, want)
            w64 = want.to(torch.float64)
            _held(s, w64.sum((0, 2, 3)), _B(2 * 8 * 8, w64.abs().sum((0, 2, 3))), "replay colsum")
        elif name == "wgrad16":
            g, x, k, _, stride, pad = a
            x = x.detach()
            ref = R.wgrad_ref(x, g, k, k, (stride, stride), (pad, pad)).permute(0, 2, 3, 1)
            mag = R.wgrad_ref(x.abs(), g.abs(), k, k, (stride, stride), (pad, pad)).permute(0, 2, 3, 1)
            # fi_bn_fold_grad has scaled the buffer in place since: replay the launch on its recorded inputs
            _held(grad16.wgrad16(g, x, k, k, stride, pad), ref, _B(2 * 8 * 8, mag), "replay wgrad %dx%d" % (k, k))
        else:
            g, wt, in_hw, stride, pad = a
            k = wt.shape[1]
            w_l = wt.flip(1, 2).permute(3, 0, 1, 2)
            ref = R.dgrad_ref(g, w_l, (stride, stride), (pad, pad), in_hw)
            B = _B(wt.shape[3] * k * k, R.dgrad_ref(g.abs(), w_l.abs(), (stride, stride), (pad, pad), in_hw))
            _held(out, ref, B + UNIT[sfx] * (ref.abs() + B) + SUBNORMAL[sfx], "replay dgrad %dx%d" % (k, k))


# N 2 on 2 x 3, 32 channels: the fewest channels fi_grad16_eligible takes for all three kinds (tests/test_grad16_host.py), an
# odd map smaller than every tile, and 12 pixels, at which every gradient is the same bits on every run, so that torch.equal
# can be asked of all of them:
#   dW       wgrad16 adds with atomics only once it splits its pixel range, from 1024 pixels on (csrc/conv_grad16.hip,
#            wgrad_split);
#   the sums relu_grad16 adds its threads' partial column sums with atomics in LDS; at 32 channels the threads of its first
#            wave hold rows 0 .. 15 and every other wave adds exact zeros, so up to 16 pixels the order of the adds is that of
#            the lanes of one instruction (at 5 x 7 the last bits of d beta, d gamma and d conv.bias differ between two runs of
#            the SAME layer function).
ONE_PATH = [(2, 2, 3, 32, 32, 1, 1), (2, 2, 3, 32, 32, 3, 1)]


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("shape", ONE_PATH, ids=_ids)
def test_grad16_layer_is_the_train16_layer_without_a_hand_off(shape, with_res, sfx):
    """grad16.conv_bn_act16 and train16.conv_bn_act16 with no hand-off are one code path: the same bits in y and in every
    gradient, the same launches, and no gate traffic -- the Gate16 on the output is never claimed."""
    from feature_intertwiner_amd import grad16, train16
    N, H, W, Cin, Cout, k, stride = shape
    dtype = DTYPES[sfx]
    gen = torch.Generator().manual_seed(40 + sum(shape))
    x0 = _act((N, Cin, H, W), dtype, gen).detach()
    res0 = _act((N, Cout, H, W), dtype, gen).detach() if with_res else None
    dy = torch.randn((N, Cout, H, W), generator=gen).to(dtype).to(DEV).contiguous(memory_format=CL)
    train16.reset_stats()
    out = {}
    for name, layer in (("grad16", grad16.conv_bn_act16), ("train16", train16.conv_bn_act16)):
        conv, bn = _layer(Cin, Cout, k, stride, seed=sum(shape))
        x16 = x0.clone().requires_grad_()
        res = res0.clone().requires_grad_() if with_res else None
        y = layer(x16, conv, bn, relu=True, residual=res)
        assert 0 < int(torch.count_nonzero(y)) < y.numel()
        leaves = [x16, conv.weight, conv.bias, bn.weight, bn.bias] + ([res] if with_res else [])
        grad16.reset_stats()
        grads = torch.autograd.grad(y, leaves, dy)
        out[name] = (y.detach(),) + tuple(grads), grad16.stats()
    (a, stats_a), (b, stats_b) = out["grad16"], out["train16"]
    assert stats_a == stats_b == {"relu_grad": 1, "dgrad": 1, "wgrad": 1, "weights": 1}
    st = train16.stats()
    assert st["gated"] == st["premasked"] == st["fallback"] == 0 and train16.pair_adds() == 0
    names = ["y", "dx", "dW", "d conv.bias", "d gamma", "d beta"] + (["d residual"] if with_res else [])
    assert len(a) == len(b) == len(names)
    for what, ta, tb in zip(names, a, b):
        assert ta.dtype == tb.dtype and ta.shape == tb.shape, what
        assert torch.equal(ta, tb), what                 # (the strides of dW differ for a 1x1 layer: the values do not)
    assert bool(torch.isfinite(a[2]).all()) and float(a[2].abs().max()) > 0.0
