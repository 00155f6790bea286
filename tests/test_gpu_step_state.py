"""What conv.prepare_step launches and publishes across the life of a model: the batched weight transpose runs when a
weight, a BatchNorm fold or the step state changed and not otherwise; the 16-bit copies follow the weights."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# calls of fi_weight_transpose_batch by (first prepare_step, prepare_step after a forward + backward pass, prepare_step
# with nothing changed, after an in-place weight update, after invalidate_step_state()), measured on the commit before
# the step-state registry (same test, same module)
TRANSPOSE_LAUNCHES = {"fp32": [1, 1, 0, 1, 1], "bf16": [1, 1, 0, 1, 1]}


class _Counting(object):
    """Stands in for the library handle (as tests/step_record.py's Recorder does); counts the calls of one entry and
    keeps the arguments of the last one."""

    def __init__(self, real, name):
        self._real, self._name, self.calls, self.last = real, name, 0, None

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name != self._name:
            return fn

        def counted(*a):
            self.calls += 1
            self.last = a
            return fn(*a)
        return counted


def _tiny():
    from feature_intertwiner_amd import conv as C

    class Tiny(nn.Module):
        def __init__(self):
            super().__init__()
            self.c3 = C.Conv2d(32, 32, kernel_size=3, padding=1)
            self.bn3 = nn.BatchNorm2d(32)
            self.up = C.Conv2d(32, 128, kernel_size=1)
            self.c1 = C.Conv2d(128, 128, kernel_size=1)
            self.down = C.Conv2d(128, 256, kernel_size=1, stride=2)

        def forward(self, x):
            return self.down(self.c1(self.up(C.conv_bn_act(x, self.c3, self.bn3, relu=True))))

    torch.manual_seed(3)
    net = Tiny().to(DEV).eval()
    net.bn3.running_var.uniform_(0.5, 1.5)
    return net


def _flat(w):
    """An alias of a weight (same address, same version counter) in the tap-major order the 16-bit copies have."""
    f = w.detach().permute(0, 2, 3, 1).reshape(-1)
    assert f.data_ptr() == w.data_ptr()
    return f


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_prepare_step_transposes_only_when_something_changed(precision):
    from feature_intertwiner_amd import _lib, conv as C
    before = C.conv_precision()
    C.invalidate_step_state()
    C.set_conv_precision(precision)
    real = _lib.load()
    counter = _lib._lib = _Counting(real, "fi_weight_transpose_batch")
    try:
        net = _tiny()
        x = torch.randn(1, 32, 8, 8, device=DEV)
        convs = [net.c3, net.up, net.c1, net.down]

        def launches(fn=None):
            n = counter.calls
            if fn is not None:
                fn()
            C.prepare_step(net)
            return counter.calls - n

        def published():
            return [C._cached_bf16(_flat(m.weight), torch.bfloat16, make=False) for m in convs]

        def train():
            net(x.clone().requires_grad_(True)).sum().backward()
            net.zero_grad(set_to_none=True)

        def update():
            with torch.no_grad():
                for m in convs:
                    m.weight.mul_(1.5)

        got = [launches()]
        got.append(launches(train))
        if precision == "bf16":
            pub = published()
            assert all(p is not None for p in pub)
        # a weight no plan knows, converted on the fly (as the backward pass does with its transposed temporaries): kept
        # while nothing is republished, released with its fp32 source when the next training step republishes
        temp = torch.randn(64, 64, 1, 1, device=DEV)
        t16 = C._cached_bf16(temp)
        got.append(launches())
        assert C._cached_bf16(temp, make=False) is t16
        if precision == "bf16":
            assert all(a is b for a, b in zip(published(), pub))
        got.append(launches(update))
        assert C._cached_bf16(temp, make=False) is None
        if precision == "bf16":
            for m, p in zip(convs, published()):
                assert p is not None and torch.equal(p, _flat(m.weight).to(torch.bfloat16))
        got.append(launches(C.invalidate_step_state))
        torch.cuda.synchronize()
        print("fi_weight_transpose_batch launches (%s): %s" % (precision, got))
        assert got == TRANSPOSE_LAUNCHES[precision]
    finally:
        _lib._lib = real
        C.set_conv_precision(before)
        C.invalidate_step_state()


def test_a_precision_switch_rebuilds_the_plan():
    """A plan built under a 16-bit precision has no fragment-major copies; the same model stepped in fp32 afterwards gets
    them (the persistent 1x1 kernel reads them)."""
    from feature_intertwiner_amd import _lib, conv as C, step_state as S
    before = C.conv_precision()
    C.invalidate_step_state()
    real = _lib.load()
    try:
        net = _tiny()
        C.set_conv_precision("bf16")
        C.prepare_step(net)
        assert not C._COPIES.having(S.FRAG)
        C.set_conv_precision("fp32")
        C.prepare_step(net)
        w = net.c1.weight
        assert C._COPIES.lookup(w, S.FRAG, (128, 128)) is not None                         # forward: W, keyed by the weight
        wt = C._COPIES.lookup(w, S.WT, (False, tuple(w.shape)))
        assert wt is not None and C._COPIES.lookup(wt, S.FRAG, (128, 128)) is not None      # data gradient: keyed by W^T
        assert len(C._COPIES.having(S.FRAG)) == 2
        # ... and the forward pass of that layer reads the copy: weight_layout 3, the persistent kernel's
        x = torch.randn(2, 128, 128, 128, device=DEV)
        counter = _lib._lib = _Counting(real, "fi_conv2d_forward_live")
        y = C.conv2d(x, w, net.c1.bias)
        torch.cuda.synchronize()
        assert counter.calls == 1 and counter.last[19] == 3
        assert counter.last[1].value == C._COPIES.lookup(w, S.FRAG, (128, 128)).data_ptr()
        ref = torch.nn.functional.conv2d(x.double(), w.detach().double(), net.c1.bias.detach().double())
        assert float((y.detach().double() - ref).abs().max()) <= 1e-4 * float(ref.abs().max())
    finally:
        _lib._lib = real
        C.set_conv_precision(before)
        C.invalidate_step_state()
