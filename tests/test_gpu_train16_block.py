"""sub_module.Bottleneck on 16-bit channels-last tensors that require grad (TRAIN.ACT_PRECISION, train16.conv_bn_act16):
identity blocks with `input_sole` on and off, C2's stride-1 projection block, the stride-2 projection block with and
without a lateral gradient, and a chain of three identity blocks -- on 2 x 8 x 8, and 2 x 7 x 9 for the stride-2 block.

What is held: the forward's bits equal the inference branch under no_grad; the counters give the launch counts of the
design (a steady-state inner block: 3 gated data gradients, 3 weight gradients, 0 relu_grad); the gated form's data
gradients are torch.equal to the ungated form's (conv.GATES = False) on the same inputs; every recorded backward launch
-- gated dgrad, dgrad, wgrad, relu_grad -- replays within its float64 bar on exactly its recorded operands; and the
parameter gradients of BOTH forms are held to float64 with the propagated bars of tests/test_gpu_grad16_layer.py (the
forms differ only by the order in which the column sums s were added).
A block output handed to two consumers against the contract makes `fallback` rise and leaves the gradients correct."""
import math

import pytest
import torch

import fp64_ref as R
from test_gpu_grad16_layer import CL, DEV, DTYPES, SUBNORMAL, UNIT, _B, _act, _held, _layer

pytestmark = pytest.mark.gpu


def _randomize(block, seed):
    """Non-trivial convolution and BatchNorm parameters and running statistics, as _layer's."""
    gen = torch.Generator().manual_seed(seed)
    pairs = [(block.conv1, block.bn1), (block.conv2, block.bn2), (block.conv3, block.bn3)]
    if block.downsample is not None:
        pairs.append((block.downsample[0], block.downsample[1]))
    with torch.no_grad():
        for conv, bn in pairs:
            cout, cin, k, _ = conv.weight.shape
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) / math.sqrt(cin * k * k))
            conv.bias.copy_(0.5 * torch.randn(cout, generator=gen))
            bn.weight.copy_(0.5 + torch.rand(cout, generator=gen))
            bn.weight[::5] *= -1.0
            bn.bias.copy_(0.5 * torch.randn(cout, generator=gen))
            bn.running_mean.copy_(0.5 * torch.randn(cout, generator=gen))
            bn.running_var.copy_(0.25 + torch.rand(cout, generator=gen))
    block.to(DEV)
    block.eval()
    return block


def _block(inplanes, planes, stride, project, seed, input_sole=False):
    from feature_intertwiner_amd import sub_module
    from feature_intertwiner_amd.conv import Conv2d
    down = None
    if project:
        down = torch.nn.Sequential(Conv2d(inplanes, planes * 4, kernel_size=1, stride=stride),
                                   torch.nn.BatchNorm2d(planes * 4, eps=0.001, momentum=0.01))
    b = _randomize(sub_module.Bottleneck(inplanes, planes, stride, down), seed)
    b.input_sole = input_sole
    return b


def _layers_of(block):
    """(conv, bn) in the order the BACKWARD visits them."""
    out = [(block.conv3, block.bn3)]
    if block.downsample is not None:
        out.append((block.downsample[0], block.downsample[1]))
    return out + [(block.conv2, block.bn2), (block.conv1, block.bn1)]


def _record(monkeypatch):
    from feature_intertwiner_amd import grad16, train16
    calls = []
    for mod, name in ((grad16, "relu_grad16"), (grad16, "wgrad16"), (grad16, "dgrad16"), (train16, "dgrad_gated16")):
        def rec(*a, _fn=getattr(mod, name), _name=name, **kw):
            out = _fn(*a, **kw)
            calls.append((_name, a, kw, out))
            return out
        monkeypatch.setattr(mod, name, rec)
    return calls


def _reset():
    from feature_intertwiner_amd import act16, grad16, train16
    train16.reset_stats()
    grad16.reset_stats()
    act16.reset_stats()


def _counts():
    from feature_intertwiner_amd import grad16, train16
    t, g = train16.stats(), grad16.stats()
    return dict(gated=t["gated"], premasked=t["premasked"], fallback=t["fallback"], relu_grad=g["relu_grad"],
                dgrad=g["dgrad"], wgrad=g["wgrad"])


def _zero_grads(modules):
    for m in modules:
        for p in m.parameters():
            p.grad = None


def _replay(calls, sfx):
    """Every recorded launch against float64 on exactly its recorded operands."""
    from feature_intertwiner_amd import grad16
    dtype = DTYPES[sfx]
    assert calls
    for name, a, kw, out in list(calls):                             # (the replayed launches are recorded too)
        if name == "relu_grad16":
            dyi, yi = a[0], a[1]
            g, s = out
            want = dyi * (yi > 0).to(dtype) if kw.get("relu", True) else dyi
            assert torch.equal(g, want)
            w64 = want.to(torch.float64)
            P = want.shape[0] * want.shape[2] * want.shape[3]
            if s is not None:
                _held(s, w64.sum((0, 2, 3)), _B(P, w64.abs().sum((0, 2, 3))), "replay colsum")
        elif name == "wgrad16":
            g, x, k, _, stride, pad = a
            x = x.detach()
            P = g.shape[0] * g.shape[2] * g.shape[3]
            ref = R.wgrad_ref(x, g, k, k, (stride, stride), (pad, pad)).permute(0, 2, 3, 1)
            mag = R.wgrad_ref(x.abs(), g.abs(), k, k, (stride, stride), (pad, pad)).permute(0, 2, 3, 1)
            # fi_bn_fold_grad has scaled the buffer in place since: replay the launch on its recorded inputs
            _held(grad16.wgrad16(g, x, k, k, stride, pad), ref, _B(P, mag), "replay wgrad %dx%d" % (k, k))
        else:
            if name == "dgrad16":
                g, wt, in_hw, stride, pad = a
                gate, dx, s = None, out, None
            else:
                g, wt, gate, in_hw, stride, pad = a
                dx, s = out
            add = kw.get("dx_add")
            k = wt.shape[1]
            w_l = wt.flip(1, 2).permute(3, 0, 1, 2)
            ref = R.dgrad_ref(g, w_l, (stride, stride), (pad, pad), in_hw)
            mag = R.dgrad_ref(g.abs(), w_l.abs(), (stride, stride), (pad, pad), in_hw)
            if add is not None:
                ref, mag = ref + add.to(torch.float64), mag + add.to(torch.float64).abs()
            B = _B(wt.shape[3] * k * k, mag)
            allow = B + UNIT[sfx] * (ref.abs() + B) + SUBNORMAL[sfx]
            if gate is not None:
                opened = gate.detach().to(torch.float64) > 0             # the select is on the gate: every element is held
                ref = torch.where(opened, ref, torch.zeros_like(ref))
                allow = torch.where(opened, allow, torch.zeros_like(allow))
            _held(dx, ref, allow, "replay %s %dx%d / %d%s" % (name, k, k, stride, " + dx_add" if add is not None else ""))
            if s is not None:
                d64 = dx.to(torch.float64)
                P = dx.shape[0] * dx.shape[2] * dx.shape[3]
                _held(s, d64.sum((0, 2, 3)), _B(P, d64.abs().sum((0, 2, 3))), "replay gated colsum")


def _check_param_grads(calls, layers, sfx, what):
    """The parameter gradients of `layers` (in backward order) against float64, from the (g, x) each layer's weight
    gradient was recorded with: the bars of tests/test_gpu_grad16_layer.py."""
    wg = [c for c in calls if c[0] == "wgrad16"]
    assert len(wg) == len(layers)
    for (conv, bn), (_, a, _, _) in zip(layers, wg):
        g, x16, k, _, stride, pad = a
        x16 = x16.detach()
        Cout, Cin = conv.weight.shape[0], conv.weight.shape[1]
        assert (k, stride, pad) == (conv.kernel_size[0], conv.stride[0], conv.padding[0]) and g.shape[1] == Cout
        P, K = g.shape[0] * g.shape[2] * g.shape[3], Cin * k * k
        st, pd = (stride, stride), (pad, pad)
        scale = bn._fi_fold[0]
        g64 = g.to(torch.float64)
        s_ref, s_mag = g64.sum((0, 2, 3)), g64.abs().sum((0, 2, 3))
        B_s = _B(P, s_mag)
        dwp = R.wgrad_ref(x16, g, k, k, st, pd)
        B_w = _B(P, R.wgrad_ref(x16.abs(), g.abs(), k, k, st, pd))
        w64 = conv.weight.detach().to(torch.float64)
        cb = conv.bias.detach()
        dW, dgam, _, dcb, _ = R.fold_grad_ref(dwp.reshape(Cout, Cin, -1), w64.reshape(Cout, Cin, -1), s_ref, scale,
                                              bn.running_mean, bn.running_var, bn.eps, cb)
        inv = 1.0 / torch.sqrt(bn.running_var.to(torch.float64) + bn.eps)
        sc = scale.to(torch.float64).abs()
        off = (cb.to(torch.float64) - bn.running_mean.to(torch.float64)).abs()
        tag = "%s %dx%d %d->%d" % (what, k, k, Cin, Cout)
        _held(bn.bias.grad, s_ref, B_s, tag + " d beta")
        dw = conv.weight.grad
        assert dw.dtype == torch.float32 and dw.shape == conv.weight.shape and dw.stride() == conv.weight.stride()
        ref = dW.reshape(Cout, Cin, k, k)
        scB = sc.view(-1, 1, 1, 1) * B_w
        _held(dw, ref, scB + R.U * (ref.abs() + scB), tag + " dW")
        wa = w64.abs().reshape(Cout, -1)
        carried = inv * ((wa * B_w.reshape(Cout, -1)).sum(1) + off * B_s)
        m = inv * ((wa * (dwp.abs().reshape(Cout, -1) + B_w.reshape(Cout, -1))).sum(1) + off * (s_ref.abs() + B_s))
        _held(bn.weight.grad, dgam, carried + _B(K, m), tag + " d gamma")
        _held(conv.bias.grad, dcb, sc * B_s + _B(1, sc * (s_ref.abs() + B_s)), tag + " d conv bias")


def _run(build_graph, modules, gates, monkeypatch=None):
    """One forward + backward of build_graph() -> (outputs, weights of the loss, leaves) with conv.GATES = gates."""
    from feature_intertwiner_amd import conv as fconv
    prev = fconv.GATES
    fconv.GATES = gates
    try:
        _zero_grads(modules)
        outs, dys, leaves = build_graph()
        for t in leaves:
            t.grad = None
        _reset()
        torch.autograd.backward(outs, dys)
        torch.cuda.synchronize()
    finally:
        fconv.GATES = prev
    return [o.detach() for o in outs], [t.grad.clone() for t in leaves], _counts()


def _both_forms(sfx, build_graph, modules, layers, expect_gated, expect_ungated, monkeypatch, what):
    """Runs the gated and the ungated form on the same inputs and checks everything the module docstring lists."""
    calls = _record(monkeypatch)
    outs_g, grads_g, cnt_g = _run(build_graph, modules, True)
    gated_calls = list(calls)
    assert cnt_g == expect_gated, (what, cnt_g)
    _check_param_grads(gated_calls, layers, sfx, what + " gated")
    del calls[:]
    outs_u, grads_u, cnt_u = _run(build_graph, modules, False)
    ungated_calls = list(calls)
    assert cnt_u == expect_ungated, (what, cnt_u)
    _check_param_grads(ungated_calls, layers, sfx, what + " ungated")
    for a, b in zip(outs_g, outs_u):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    for a, b in zip(grads_g, grads_u):
        assert a.dtype == DTYPES[sfx] and float(a.float().abs().max()) > 0.0
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), what + ": data gradients of the two forms differ"
    _replay(gated_calls, sfx)
    _replay(ungated_calls, sfx)
    return outs_g, gated_calls


def _dy(shape, dtype, gen):
    return torch.randn(shape, generator=gen).to(dtype).to(DEV).contiguous(memory_format=CL)


def _same_as_inference(block, x16, y):
    with torch.no_grad():
        y0 = block(x16.detach())
    assert not y0.requires_grad and torch.equal(y.view(torch.int16), y0.view(torch.int16))
    assert 0 < int(torch.count_nonzero(y)) < y.numel()


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("sole", [True, False], ids=["input_sole", "shared_input"])
def test_identity_block_behind_a_producing_layer(sole, sfx, monkeypatch):
    """x = a 16-bit layer's output (it carries a Gate16).  input_sole: conv1 claims it -- 3 gated launches, the producer
    and conv1 / conv2 are premasked, only conv3 (whose output nobody claimed) runs relu_grad.  Otherwise conv1 runs the
    ungated data gradient with the shortcut's gradient as dx_add and the producer masks itself."""
    from feature_intertwiner_amd import train16
    dtype = DTYPES[sfx]
    gen = torch.Generator().manual_seed(41)
    conv0, bn0 = _layer(64, 256, 1, 1, seed=40)
    block = _block(256, 64, 1, False, seed=42, input_sole=sole)
    leaf = _act((2, 64, 8, 8), dtype, gen)
    dy = _dy((2, 256, 8, 8), dtype, gen)
    seen = {}

    def graph():
        x = train16.conv_bn_act16(leaf, conv0, bn0)
        y = block(x)
        seen["x"], seen["y"] = x.detach(), y.detach()
        return [y], [dy], [leaf]

    layers = _layers_of(block) + [(conv0, bn0)]
    n = 3 if sole else 2
    _both_forms(sfx, graph, [block, conv0, bn0], layers,
                dict(gated=n, premasked=n, fallback=0, relu_grad=4 - n, dgrad=4 - n, wgrad=4),
                dict(gated=0, premasked=0, fallback=0, relu_grad=4, dgrad=4, wgrad=4), monkeypatch, "identity %s" % sfx)
    _same_as_inference(block, seen["x"], seen["y"])


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_stride_1_projection_block_on_a_leaf(sfx, monkeypatch):
    """C2's first block: the input is the packed stem map, no gate -- conv1 runs the ungated data gradient with the
    projection's dx (through the box) as dx_add.  The projection (no ReLU) sums its dy with relu_grad16(relu=False)."""
    dtype = DTYPES[sfx]
    gen = torch.Generator().manual_seed(43)
    block = _block(64, 64, 1, True, seed=44)
    leaf = _act((2, 64, 8, 8), dtype, gen)
    dy = _dy((2, 256, 8, 8), dtype, gen)
    seen = {}

    def graph():
        y = block(leaf)
        seen["y"] = y.detach()
        return [y], [dy], [leaf]

    _both_forms(sfx, graph, [block], _layers_of(block),
                dict(gated=2, premasked=2, fallback=0, relu_grad=2, dgrad=2, wgrad=4),
                dict(gated=0, premasked=0, fallback=0, relu_grad=4, dgrad=4, wgrad=4), monkeypatch, "C2 projection %s" % sfx)
    _same_as_inference(block, leaf, seen["y"])


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("lateral", [True, False], ids=["lateral", "no_lateral"])
def test_stride_2_projection_block(lateral, sfx, monkeypatch):
    """2 x 7 x 9 -> 4 x 5.  With a lateral_box the unpacked copy of x has a reader of its own; its gradient comes back
    packed through the box, is chained as the projection's dx_add, and conv1 -- the cell form -- sees x's whole gradient
    and claims x's gate: the producer is premasked."""
    from feature_intertwiner_amd import act16, train16
    from feature_intertwiner_amd.conv import GradBox
    dtype = DTYPES[sfx]
    gen = torch.Generator().manual_seed(45)
    conv0, bn0 = _layer(64, 256, 1, 1, seed=46)
    block = _block(256, 128, 2, True, seed=47)
    leaf = _act((2, 64, 7, 9), dtype, gen)
    dy = _dy((2, 512, 4, 5), dtype, gen)
    dz = torch.randn((2, 256, 7, 9), generator=gen).to(DEV)
    seen = {}

    def graph():
        x = train16.conv_bn_act16(leaf, conv0, bn0)
        box = None
        if lateral:
            box = block.lateral_box = GradBox()
        y = block(x)
        assert block.lateral_box is None
        seen["x"], seen["y"] = x.detach(), y.detach()
        if not lateral:
            return [y], [dy], [leaf]
        z = train16.unpack(x, box)                                   # applied after the block: its backward runs first
        return [y, z], [dy, dz], [leaf]

    layers = _layers_of(block) + [(conv0, bn0)]
    if lateral:
        gated = dict(gated=3, premasked=3, fallback=0, relu_grad=2, dgrad=2, wgrad=5)
    else:
        gated = dict(gated=2, premasked=2, fallback=0, relu_grad=3, dgrad=3, wgrad=5)
    _both_forms(sfx, graph, [block, conv0, bn0], layers, gated,
                dict(gated=0, premasked=0, fallback=0, relu_grad=5, dgrad=5, wgrad=5), monkeypatch,
                "stride-2 projection %s%s" % (sfx, " + lateral" if lateral else ""))
    _same_as_inference(block, seen["x"], seen["y"])
    if lateral:
        assert train16.stats()["pack"] == 1 and act16.stats()["pack"] == 1       # the lateral gradient, packed once


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_chain_of_three_identity_blocks(sfx, monkeypatch):
    """The middle block is the steady state: 3 gated data gradients, 3 weight gradients, premasked 3, no relu_grad."""
    dtype = DTYPES[sfx]
    gen = torch.Generator().manual_seed(48)
    blocks = [_block(256, 64, 1, False, seed=50 + i, input_sole=i > 0) for i in range(3)]
    chain = torch.nn.Sequential(*blocks)
    leaf = _act((2, 256, 8, 8), dtype, gen, scale=0.5)
    dy = _dy((2, 256, 8, 8), dtype, gen)
    seen = {}

    def graph():
        y = chain(leaf)
        seen["y"] = y.detach()
        return [y], [dy], [leaf]

    layers = _layers_of(blocks[2]) + _layers_of(blocks[1]) + _layers_of(blocks[0])
    _, gated_calls = _both_forms(sfx, graph, blocks, layers,
                                 dict(gated=8, premasked=8, fallback=0, relu_grad=1, dgrad=1, wgrad=9),
                                 dict(gated=0, premasked=0, fallback=0, relu_grad=9, dgrad=9, wgrad=9), monkeypatch,
                                 "chain %s" % sfx)
    with torch.no_grad():
        y0 = chain(leaf.detach())
    assert torch.equal(seen["y"].view(torch.int16), y0.view(torch.int16))
    # the order of the gated form's launches: the last block's conv3 masks itself, then eight layers of (wgrad, gated),
    # the middle block's three among them, then the first conv1 on the leaf
    names = [c[0] for c in gated_calls]
    assert names == ["relu_grad16"] + ["wgrad16", "dgrad_gated16"] * 8 + ["wgrad16", "dgrad16"]
    assert names[7:13] == ["wgrad16", "dgrad_gated16"] * 3               # the middle block


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_two_consumers_against_the_contract_fall_back_and_stay_correct(sfx, monkeypatch):
    """A layer's output handed to TWO blocks that both promise to be its only reader: both claim the gate, autograd adds
    their gradients into a tensor neither wrote, the producer sees that it is not the claimed one, masks and sums it
    itself (fallback) -- and the gradients equal the ungated form's bit for bit."""
    from feature_intertwiner_amd import train16
    dtype = DTYPES[sfx]
    gen = torch.Generator().manual_seed(60)
    conv0, bn0 = _layer(64, 256, 1, 1, seed=61)
    a = _block(256, 64, 1, False, seed=62, input_sole=True)
    b = _block(256, 64, 1, False, seed=63, input_sole=True)
    leaf = _act((2, 64, 8, 8), dtype, gen)
    dya, dyb = _dy((2, 256, 8, 8), dtype, gen), _dy((2, 256, 8, 8), dtype, gen)

    def graph():
        x = train16.conv_bn_act16(leaf, conv0, bn0)
        return [a(x), b(x)], [dya, dyb], [leaf]

    layers = _layers_of(b) + _layers_of(a) + [(conv0, bn0)]
    _both_forms(sfx, graph, [a, b, conv0, bn0], layers,
                dict(gated=6, premasked=4, fallback=1, relu_grad=3, dgrad=1, wgrad=7),
                dict(gated=0, premasked=0, fallback=0, relu_grad=7, dgrad=7, wgrad=7), monkeypatch, "two consumers %s" % sfx)
