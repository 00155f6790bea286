"""conv.FLOP_LOG gets its keys from the library's plan queries (fi_conv2d_forward_plan, fi_conv2d_weight_grad_plan,
fi_gemm_nt_plan): for shapes on both sides of every threshold of the kernel selection, the kernel the log names is the one
whose profiling counter the launch incremented -- launch for launch, forward, data gradient and weight gradient."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# N, Cin, H, W, Cout, R, stride, pad (tests/test_capi_and_host.py holds the expected key of each forward / weight gradient)
SHAPES = [
    (1, 16, 128, 128, 256, 3, 1, 1), (1, 16, 120, 128, 256, 3, 1, 1),       # 2-D patch tiles | generic
    (168, 16, 14, 14, 256, 3, 1, 1), (166, 16, 14, 14, 256, 3, 1, 1),       # flat patch tiles | generic
    (1, 128, 128, 128, 256, 1, 1, 0), (1, 128, 124, 128, 256, 1, 1, 0),     # 1x1 registers | generic
    (1, 96, 128, 128, 256, 1, 1, 0),
    (1, 16, 512, 256, 256, 3, 2, 1), (1, 16, 508, 256, 256, 3, 2, 1),       # generic 128-row | 64-row tiles
    (2, 3, 64, 64, 64, 7, 2, 3),
    (6, 1024, 64, 64, 256, 1, 1, 0), (5, 1024, 64, 64, 256, 1, 1, 0),       # weight gradient 128-row | 64-row tiles
]


def _logged(fn):
    """Run fn with the flop log and the profiling counters on: (FLOP_LOG, {conv counter: launches})."""
    from feature_intertwiner_amd import _lib, conv as C
    C.FLOP_LOG = {}
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        _lib.prof_enable(False)
        used, C.FLOP_LOG = dict(C.FLOP_LOG), None
    ran = {k: _lib.prof_get(k)[0] for k in _lib.KERNEL_IDS if k.startswith("conv")}
    return used, {k: n for k, n in ran.items() if n}


def _assert_agree(used, ran, what):
    print(what, "logged", {k: v[0] for k, v in used.items()}, "ran", ran)
    assert used, what
    for k, (n, flops) in used.items():
        assert ran.get(k, 0) == n and flops > 0, (what, k, n, ran)
    assert set(ran) <= set(used), (what, sorted(set(ran) - set(used)))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_flop_log_keys_are_the_kernels_that_ran(shape):
    from feature_intertwiner_amd.conv import conv2d
    N, Cin, H, W, Cout, R, st, pd = shape
    g = torch.Generator(device=DEV).manual_seed(sum(shape))
    x = torch.randn(N, Cin, H, W, device=DEV, generator=g).requires_grad_(True)
    w = (torch.randn(Cout, Cin, R, R, device=DEV, generator=g) / (Cin * R * R) ** 0.5).requires_grad_(True)

    def run():
        y = conv2d(x, w, None, (st, st), (pd, pd))
        y.backward(torch.ones_like(y))
    used, ran = _logged(run)
    _assert_agree(used, ran, str(shape))
    assert sum(n for n, _ in used.values()) >= 3               # forward, data gradient, weight gradient


def test_flop_log_flat_patch_gate_alignment_fallback():
    """The flat patch kernel reads the gate in 8-byte pieces: a gate at a 4-byte address goes to the generic kernel."""
    from feature_intertwiner_amd import conv as C
    x = torch.randn(168, 16, 14, 14, device=DEV)
    w = torch.randn(256, 3, 3, 16, device=DEV) * 0.1
    buf = torch.randn(168 * 256 * 14 * 14 + 4, device=DEV)
    outs = {}
    for off in (2, 1):
        gate = buf[off:off + 168 * 256 * 14 * 14].view(168, 256, 14, 14)
        assert gate.data_ptr() % 8 == (4 * off) % 8
        used, ran = _logged(lambda: outs.__setitem__(off, C._conv_fwd(x, w, None, (1, 1), (1, 1), w_tap_major=True, gate=gate)))
        _assert_agree(used, ran, "gate offset %d" % off)
        assert ("conv3x3_patch_flat" in used) == (off == 2), used
    ref = torch.nn.functional.conv2d(x.double(), w.permute(0, 3, 1, 2).double(), padding=1)
    for off in (2, 1):
        exp = ref * (buf[off:off + ref.numel()].view_as(ref) > 0)
        assert (outs[off].double() - exp).abs().max().item() <= 2e-5 * 12 * ref.abs().max().item()


@pytest.mark.parametrize("n,key", [(6, "conv_wgrad_bm128_1x1"), (5, "conv_wgrad_bm64_1x1")])
def test_flop_log_batched_weight_gradient(n, key):
    """n identical 1x1 layers whose weight gradients travel in one fi_conv2d_weight_grad_batch launch: the batch count
    enters the tile choice, and the log asks with it."""
    from feature_intertwiner_amd import conv as C

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.convs = torch.nn.ModuleList([C.Conv2d(1024, 256, 1, bias=False) for _ in range(n)])

        def forward(self, x):
            C.prepare_step(self)
            return sum(m(x) for m in self.convs)
    torch.manual_seed(n)
    net = Net().to(DEV)
    x = torch.randn(1, 1024, 64, 64, device=DEV)
    try:
        used, ran = _logged(lambda: net(x).sum().backward())
    finally:
        C.invalidate_step_state()
    _assert_agree(used, ran, "batch of %d" % n)
    assert used[key][0] == 1 and sum(v[0] for k, v in used.items() if "wgrad" in k) == 1, used
    ref = x[0].sum((1, 2)).expand(256, 1024)                   # dW of y.sum(): the pixel sum of every input channel
    for m in net.convs:
        assert (m.weight.grad.view(256, 1024) - ref).abs().max().item() <= 2e-5 * 64 * ref.abs().max().item()


@pytest.mark.parametrize("K", [24576, 20480])
def test_flop_log_gemm(K):
    from feature_intertwiner_amd.conv import linear
    g = torch.Generator(device=DEV).manual_seed(K)
    x = torch.randn(256, K, device=DEV, generator=g).requires_grad_(True)
    w = (torch.randn(1024, K, device=DEV, generator=g) / K ** 0.5).requires_grad_(True)

    def run():
        y = linear(x, w)
        y.backward(torch.ones_like(y))
    used, ran = _logged(run)
    _assert_agree(used, ran, "gemm K=%d" % K)
    assert ("conv_wgrad_bm128_1x1" if K == 24576 else "conv_wgrad_bm64_1x1") in used, used
