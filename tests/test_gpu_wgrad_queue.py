"""conv's queue of deferred weight gradients, one flush trigger at a time, in fp32: identical conv + eval-BatchNorm layers on
[2, 128, 8, 8] maps (the smallest geometry the fp32 planner batches) are queued and launched together when the queue is
full, when it has aged, when a layer is used again, and at the end of the backward pass.  The library handle is swapped
for a logger of the weight-gradient and BatchNorm-fold entry points (in call order, with the batch size and the stream
argument); every gradient is checked against a float64 restatement from stock torch functions with the bar of
test_gpu_conv.py::test_batchnorm_gradients_from_the_weight_gradient, and every logged call must carry the stream that
is current in the test body."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

WGRAD, WGRAD_BATCH = "fi_conv2d_weight_grad", "fi_conv2d_weight_grad_batch"
FOLD, FOLD_BATCH = "fi_bn_fold_grad", "fi_bn_fold_grad_batch"
_N_AT = {WGRAD: None, FOLD: None, WGRAD_BATCH: 4, FOLD_BATCH: 10}       # entry -> position of its `n` argument


class _Logger(object):
    """Stands in for the loaded library (as tests/step_record.py's Recorder does): appends (name, n or None, stream) of
    every call of the four entries to `log`."""

    def __init__(self, real, log):
        self._real, self._log = real, log

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in _N_AT:
            return fn

        def logged(*a):
            at = _N_AT[name]
            self._log.append((name, None if at is None else int(a[at]), a[-1].value or 0))
            return fn(*a)
        return logged


class _Net(nn.Module):
    """`uses`: which of the 128-channel conv + BatchNorm + ReLU layers forward applies, in order.  n_small 1x1 convolutions
    on 16 channels (never queued) run in series before them ("first": on the input, their result repeated to 128
    channels) or after them ("last": on the first 16 channels of the result)."""

    def __init__(self, uses, n_small=0, small="last"):
        super().__init__()
        from feature_intertwiner_amd import conv as C
        self.uses, self.small_at = tuple(uses), small
        # (conv, bn) as neighbouring children, as in the detector: the gradient arena then holds the BatchNorm's sums too
        self.blocks = nn.ModuleList([nn.Sequential(C.Conv2d(128, 128, 3, padding=1, bias=False),
                                                   nn.BatchNorm2d(128, eps=0.001)) for _ in range(max(uses) + 1)])
        self.small = nn.ModuleList([C.Conv2d(16, 16, 1) for _ in range(n_small)])
        with torch.no_grad():
            for _, bn in self.blocks:
                bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(0, 0.3)
                bn.running_mean.normal_(0, 0.5); bn.running_var.uniform_(0.5, 2.0)
        self.eval()
        self.log = None

    def _small(self, y):
        for m in self.small:
            y = m(y)
        return y

    def forward(self, x):
        from feature_intertwiner_amd import conv as C
        C.prepare_step(self)
        y = x
        if self.small and self.small_at == "first":
            y = self._small(y).repeat(1, 8, 1, 1)
        for k, i in enumerate(self.uses):
            y = C.conv_bn_act(y, self.blocks[i][0], self.blocks[i][1], relu=True)
            if self.log is not None:        # fires when y's gradient is there: right before this use's backward runs
                y.register_hook(lambda g, k=k: self.log.append(("backward of use", k, None)))
        if self.small and self.small_at == "last":
            y = self._small(y[:, :16])
        return y

    def reference(self, x, gy):
        """{name: gradient} of the same function of float64 copies on the host, and the input's gradient as "x"."""
        sd = {k: v.detach().cpu().double().requires_grad_("running" not in k) for k, v in self.state_dict().items()
              if v.dtype.is_floating_point}

        def small(y):
            for j in range(len(self.small)):
                y = F.conv2d(y, sd["small.%d.weight" % j], sd["small.%d.bias" % j])
            return y
        xd = x.cpu().double().requires_grad_(True)
        y = xd
        if self.small and self.small_at == "first":
            y = small(y).repeat(1, 8, 1, 1)
        for i in self.uses:
            y = F.conv2d(y, sd["blocks.%d.0.weight" % i], None, padding=1)
            y = F.relu(F.batch_norm(y, sd["blocks.%d.1.running_mean" % i], sd["blocks.%d.1.running_var" % i],
                                    sd["blocks.%d.1.weight" % i], sd["blocks.%d.1.bias" % i], False, 0.0, 0.001))
        if self.small and self.small_at == "last":
            y = small(y[:, :16])
        y.backward(gy.cpu().double())
        ref = {k: v.grad for k, v in sd.items() if v.requires_grad}
        ref["x"] = xd.grad
        return ref


def _run(net, channels, batch=None, age=None, unchecked=()):
    """One forward and backward pass of `net` under the logger with conv.WGRAD_BATCH / WGRAD_BATCH_AGE set as given:
    checks every gradient (but those named in `unchecked`) against float64 and every logged call's stream, and returns
    the log."""
    from feature_intertwiner_amd import _lib, conv as C
    net = net.to(DEV)
    g = torch.Generator(device=DEV).manual_seed(len(net.uses) + 10 * len(net.small))
    x = torch.randn(2, channels, 8, 8, device=DEV, generator=g).requires_grad_(True)
    log = net.log = []
    saved = (C.WGRAD_BATCH, C.WGRAD_BATCH_AGE)
    real = _lib.load()
    stream = _lib.current_stream().value or 0
    try:
        if batch is not None:
            C.WGRAD_BATCH = batch
        if age is not None:
            C.WGRAD_BATCH_AGE = age
        _lib._lib = _Logger(real, log)
        y = net(x)
        gy = torch.randn(y.shape, device=DEV, generator=g)
        y.backward(gy)
        torch.cuda.synchronize()
        assert not C._WGQ["queues"] and not C._WGQ["armed"], C._WGQ
        ref = net.reference(x.detach(), gy)
        got = dict((k, p.grad) for k, p in net.named_parameters())
        got["x"] = x.grad
        assert set(got) == set(ref)
        for name, b in ref.items():
            err = float((got[name].cpu().double() - b).abs().max())
            assert name in unchecked or err <= 2e-4 * float(b.abs().max()) + 1e-9, (name, err, log)
        calls = [e for e in log if e[0] in _N_AT]
        assert calls and all(e[2] == stream for e in calls), (stream, calls)
    finally:
        _lib._lib = real
        C.WGRAD_BATCH, C.WGRAD_BATCH_AGE = saved
        net.log = None
        C.invalidate_step_state()
    return [e[:2] for e in log]


def _only(log, *names):
    return [e for e in log if e[0] in names]


def test_end_of_pass_flushes_one_batch():
    """Three layers, default WGRAD_BATCH: nothing is launched per layer, the end of the pass launches all three weight
    gradients together and their three folds together."""
    torch.manual_seed(31)
    log = _run(_Net((0, 1, 2)), 128)
    assert _only(log, WGRAD, WGRAD_BATCH) == [(WGRAD_BATCH, 3)], log
    assert _only(log, FOLD, FOLD_BATCH) == [(FOLD_BATCH, 3)], log
    assert log.index((WGRAD_BATCH, 3)) > log.index(("backward of use", 0)), log     # after the last layer's backward began


def test_full_queue_is_flushed_at_once():
    """WGRAD_BATCH = 2: the queue is launched when it holds two, before the third layer's backward runs; the third goes
    alone at the end of the pass, with a single fold."""
    torch.manual_seed(32)
    log = _run(_Net((0, 1, 2)), 128, batch=2)
    assert _only(log, WGRAD, WGRAD_BATCH) == [(WGRAD_BATCH, 2), (WGRAD_BATCH, 1)], log
    assert _only(log, FOLD, FOLD_BATCH) == [(FOLD_BATCH, 2), (FOLD, None)], log
    third = log.index(("backward of use", 0))          # (use 0 is the first in forward: its backward is the third to run)
    assert log.index((WGRAD_BATCH, 2)) < log.index((FOLD_BATCH, 2)) < third < log.index((WGRAD_BATCH, 1)) < \
        log.index((FOLD, None)), log


@pytest.mark.parametrize("small", ["first", "last"])
def test_aged_queue_is_flushed(small):
    """Ten 16-channel 1x1 layers, never queued, beside the three 128-channel ones.  "first": they precede them in forward,
    so their backward runs AFTER the three were queued -- with WGRAD_BATCH_AGE = 9 the batch is launched before the last
    of the ten weight gradients, not at the end of the pass.  "last": they follow them in forward, their backward runs
    before anything is queued, and the batch leaves at the end of the pass, after all ten."""
    from feature_intertwiner_amd import conv as C
    assert C.WGRAD_BATCH_AGE == 9
    torch.manual_seed(33)
    log = _run(_Net((0, 1, 2), n_small=10, small=small), 16 if small == "first" else 128)
    wg = _only(log, WGRAD, WGRAD_BATCH)
    assert sorted(wg) == [(WGRAD, None)] * 10 + [(WGRAD_BATCH, 3)], log
    assert _only(log, FOLD, FOLD_BATCH) == [(FOLD_BATCH, 3)], log
    if small == "first":
        assert wg.index((WGRAD_BATCH, 3)) < 9, wg      # before the last of the ten
        assert wg[-1] == (WGRAD, None)
    else:
        assert wg[-1] == (WGRAD_BATCH, 3), wg


def test_reused_layer_flushes_the_queue_and_is_launched_at_once():
    """Layer 0, layer 1, layer 0 again: the backward of layer 0's second use and of layer 1 are queued; the backward of its
    first use -- the second to reach the layer's gradient slot -- launches the queue first (the fold scales dW in place)
    and then adds its own weight gradient at once.  The parameter's gradient is the sum of both uses.
    Not checked here: d gamma of the reused layer's BatchNorm.  The flush comes after this use's fi_bn_act_backward has
    added its sums to the block the queued use's fold reads, so that fold's (bias - mean) * s term counts them too; the
    queue's order is pinned as it is, and the d gamma of a reused, queued layer is a defect of its own."""
    torch.manual_seed(34)
    log = _run(_Net((0, 1, 0)), 128, unchecked=("blocks.0.1.weight",))
    assert _only(log, WGRAD, WGRAD_BATCH) == [(WGRAD_BATCH, 2), (WGRAD, None)], log
    assert _only(log, FOLD, FOLD_BATCH) == [(FOLD_BATCH, 2)], log
    again = log.index(("backward of use", 0))
    assert again < log.index((WGRAD_BATCH, 2)) < log.index((FOLD_BATCH, 2)) < log.index((WGRAD, None)), log
