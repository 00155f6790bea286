"""fi_conv2d_weight_grad_plan_{bf16,f16} names what the weight-gradient entries of the 16-bit path launch: for the shapes on
both sides of every threshold of the kernel selection (tests/test_capi_and_host.py holds the expected answers of the same
shapes on the host) the launch behaves as the named variant does, is correct against float64, and a batch takes as many
launches as the plan's per_launch says -- through the C ABI and through conv's queue of deferred weight gradients."""
import ctypes
import math

import pytest
import torch

import fp64_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPE = {"bf16": torch.bfloat16, "f16": torch.float16}

# N, Cin, H, W, Cout, R, stride, pad
FLAT = [(1, 64, 8, 8, 64, 1, 1, 0), (1, 64, 8, 8, 64, 3, 1, 1)]
ROWS = [(1, 64, 6, 6, 64, 1, 1, 0), (1, 64, 9, 9, 64, 1, 1, 0), (1, 64, 8, 8, 96, 1, 1, 0), (1, 96, 8, 8, 64, 1, 1, 0),
        (1, 64, 8, 8, 64, 3, 1, 0), (1, 64, 16, 16, 64, 3, 2, 1)]
GENERIC = [(2, 64, 3, 3, 64, 3, 1, 1), (1, 64, 6, 6, 64, 3, 2, 1), (1, 64, 16, 16, 64, 3, 3, 1)]


def _geom(shape):
    N, Cin, H, W, Cout, k, st, pd = shape
    return (N, Cin, H, W, Cout, k, k, st, st, pd, pd)


def _plan(sfx, x, dy, dw, db, shape, flags, n=1):
    from feature_intertwiner_amd import _lib
    v, per = _lib.wgrad_plan(getattr(_lib.load(), "fi_conv2d_weight_grad_plan_" + sfx), _lib.ptr(x), _lib.ptr(dy),
                             _lib.ptr(dw), _lib.ptr(db), *_geom(shape), flags, n)
    return _lib.WGRAD16_VARIANTS[v], per


def _at_offset(t, floats):
    """A copy of t that starts `floats` elements into a 16-byte aligned buffer."""
    buf = torch.empty(t.numel() + 4, device=DEV)
    assert buf.data_ptr() % 16 == 0
    out = buf[floats:floats + t.numel()].view(t.shape)
    out.copy_(t)
    return out


def _problem(shape, seed, off_x=0, off_dy=0):
    """x, dy and the float64 references of one problem: (dW, its magnitude) per operand type, and (db, its magnitude)."""
    N, Cin, H, W, Cout, k, st, pd = shape
    g = torch.Generator(device=DEV).manual_seed(seed)
    OH, OW = R.out_size(H, W, k, k, (st, st), (pd, pd))
    x = _at_offset(torch.randn(N, Cin, H, W, device=DEV, generator=g), off_x)
    dy = _at_offset(torch.randn(N, Cout, OH, OW, device=DEV, generator=g), off_dy)
    refs = {}
    for sfx, dt in DTYPE.items():
        xr, dyr = x.to(dt).float(), dy.to(dt).float()
        refs[sfx] = (R.wgrad_ref(xr, dyr, k, k, (st, st), (pd, pd)), R.wgrad_ref(xr.abs(), dyr.abs(), k, k, (st, st), (pd, pd)))
    # (the bias gradient sums the fp32 dy: the kernels add the values up before they round them)
    refs["db"] = (dy.double().sum((0, 2, 3)), dy.double().abs().sum((0, 2, 3)))
    return x, dy, refs, N * OH * OW


_PROBLEMS = {}


def _shared_problem(shape, off_x=0, off_dy=0):
    key = (shape, off_x, off_dy)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = _problem(shape, 100 + len(_PROBLEMS), off_x, off_dy)
    return _PROBLEMS[key]


def _check(dw, db, refs, sfx, pixels, what, rows=slice(None)):
    got = dw.permute(0, 3, 1, 2)                                  # tap-major [Cout][R][S][Cin] -> logical
    worst = R.check_bar(got[rows], refs[sfx][0][rows], refs[sfx][1][rows], pixels, what)
    if db is not None:
        worst = max(worst, R.check_bar(db, refs["db"][0], refs["db"][1], pixels, what + " dbias"))
    return worst


@pytest.mark.parametrize("sfx", ["bf16", "f16"])
def test_rows_live_is_honoured_where_the_plan_says_flat(sfx):
    """Only the flat kernel reads rows_live_dev: with one live row, a FLAT launch leaves every row tile but the first at
    the zeros the call filled dW with, and a ROWS launch of the neighbouring shape computes every row."""
    from feature_intertwiner_amd import _lib
    rows_entry = getattr(_lib.load(), "fi_conv2d_weight_grad_rows_" + sfx)
    live = torch.tensor([1], device=DEV, dtype=torch.int32)
    for shape, expect in (((1, 64, 8, 8, 192, 1, 1, 0), "FLAT"), ((1, 64, 6, 6, 192, 1, 1, 0), "ROWS")):
        x, dy, refs, pixels = _shared_problem(shape)
        dw = torch.full((192, 1, 1, 64), float("nan"), device=DEV)
        variant, _ = _plan(sfx, x, dy, dw, None, shape, 0)
        assert variant == expect, (shape, variant)
        _lib.check(rows_entry(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(dw), *_geom(shape), 0, _lib.ptr(live), _lib.current_stream()),
                   "fi_conv2d_weight_grad_rows")
        torch.cuda.synchronize()
        if variant == "FLAT":
            assert not dw[64:].any(), shape                       # row tiles of 64: the two past the live row are skipped
            print(shape, variant, _check(dw, None, refs, sfx, pixels, str(shape), rows=slice(0, 64)))
        else:
            print(shape, variant, _check(dw, None, refs, sfx, pixels, str(shape)))


@pytest.mark.parametrize("sfx", ["bf16", "f16"])
def test_every_variant_is_correct_at_its_threshold_shapes(sfx):
    """The launch entry on the shapes of the host table: the variant the query names, then dW (and dbias) against float64 --
    into NaN-filled outputs that the call clears, and into zeros under FI_OUTPUTS_ZEROED."""
    from feature_intertwiner_amd import _lib
    launch = getattr(_lib.load(), "fi_conv2d_weight_grad_db_" + sfx)
    cases = [(s, n, 0, 0) for n, ss in (("FLAT", FLAT), ("ROWS", ROWS), ("GENERIC", GENERIC)) for s in ss]
    cases += [(FLAT[0], "ROWS", 1, 0), (FLAT[0], "ROWS", 0, 1)]   # x / dy at +4 bytes
    for shape, expect, off_x, off_dy in cases:
        x, dy, refs, pixels = _shared_problem(shape, off_x, off_dy)
        assert x.data_ptr() % 16 == 4 * off_x and dy.data_ptr() % 16 == 4 * off_dy
        N, Cin, H, W, Cout, k, st, pd = shape
        for with_db in (False, True):
            for flags in (0, _lib.OUTPUTS_ZEROED):
                fill = 0.0 if flags else float("nan")
                dw = torch.full((Cout, k, k, Cin), fill, device=DEV)
                db = torch.full((Cout,), fill, device=DEV) if with_db else None
                what = "%s %s db=%s flags=%d" % (sfx, shape, with_db, flags)
                assert _plan(sfx, x, dy, dw, db, shape, flags) == (expect, 1), what
                _lib.check(launch(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(dw), _lib.ptr(db), *_geom(shape), flags,
                                  _lib.current_stream()), what)
                torch.cuda.synchronize()
                print(what, expect, _check(dw, db, refs, sfx, pixels, what))


@pytest.mark.parametrize("sfx", ["bf16", "f16"])
def test_a_batch_takes_the_launches_the_plan_says(sfx):
    """fi_conv2d_weight_grad_batch_<p>: ceil(n / per_launch) launches, per_launch being the query's answer for the batch's
    first problem -- one for 5 problems, two for 26, one each without FI_OUTPUTS_ZEROED or on a map of fewer than 64
    pixels --, and every problem's dW and dbias correct."""
    from feature_intertwiner_amd import _lib
    batch = getattr(_lib.load(), "fi_conv2d_weight_grad_batch_" + sfx)
    Z = _lib.OUTPUTS_ZEROED
    for shape, n, flags, launches in (((2, 128, 8, 8, 128, 3, 1, 1), 5, Z, 1), ((2, 128, 8, 8, 128, 3, 1, 1), 26, Z, 2),
                                      ((2, 128, 8, 8, 128, 3, 1, 1), 5, 0, 5), ((2, 128, 6, 6, 128, 3, 1, 1), 3, Z, 3)):
        x, dy, refs, pixels = _shared_problem(shape)
        # (the problems share x and dy: what differs between them is where the results go)
        dws = [torch.full((128, 3, 3, 128), 0.0 if flags else float("nan"), device=DEV) for _ in range(n)]
        dbs = [torch.full((128,), 0.0 if flags else float("nan"), device=DEV) for _ in range(n)]
        arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
        _, per = _plan(sfx, x, dy, dws[0], dbs[0], shape, flags, n)
        assert math.ceil(n / per) == launches, (shape, n, flags, per)
        _lib.prof_reset()
        _lib.prof_enable(True)
        try:
            _lib.check(batch(arr([x] * n), arr([dy] * n), arr(dws), arr(dbs), n, *_geom(shape), 1, flags,
                             _lib.current_stream()), "fi_conv2d_weight_grad_batch")
            torch.cuda.synchronize()
        finally:
            _lib.prof_enable(False)
        assert _lib.prof_get("conv_bf16_wgrad")[0] == launches, (shape, n, flags)
        worst = max(_check(dws[i], dbs[i], refs, sfx, pixels, "%s problem %d of %d" % (shape, i, n)) for i in range(n))
        print(sfx, shape, n, flags, "per launch", per, worst)


@pytest.mark.parametrize("precision,sfx", [("bf16", "bf16"), ("fp16", "f16")])
def test_conv_queues_what_the_plan_batches(precision, sfx):
    """Three identical 3x3 layers in 16-bit precision: on 8 x 8 maps their weight gradients are queued and travel in one
    launch, on 6 x 6 maps (fewer than 64 pixels per image: not the flat kernel) none is queued and each is launched at
    once."""
    from feature_intertwiner_amd import _lib, conv as C

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.convs = torch.nn.ModuleList([C.Conv2d(128, 128, 3, padding=1, bias=False) for _ in range(3)])

        def forward(self, x):
            C.prepare_step(self)
            return sum(m(x) for m in self.convs)
    torch.manual_seed(3)
    net = Net().to(DEV)
    queued = []
    defer = C._defer_wgrad
    C._defer_wgrad = lambda *a: queued.append(a[0]) or defer(*a)
    C.set_conv_precision(precision)
    try:
        for side, launches in ((8, 1), (6, 3)):
            shape = (2, 128, side, side, 128, 3, 1, 1)
            x, gy, refs, pixels = _shared_problem(shape)
            del queued[:]
            for p in net.parameters():
                p.grad = None
            _lib.prof_reset()
            _lib.prof_enable(True)
            try:
                (net(x) * gy).sum().backward()
                torch.cuda.synchronize()
            finally:
                _lib.prof_enable(False)
            assert _lib.prof_get("conv_bf16_wgrad")[0] == launches, side
            assert len(queued) == (3 if launches == 1 else 0) and not C._WGQ["queues"], (side, queued)
            for m in net.convs:
                R.check_bar(m.weight.grad, refs[sfx][0], refs[sfx][1], pixels, "%d x %d through conv" % (side, side))
    finally:
        C._defer_wgrad = defer
        C.set_conv_precision("fp32")
        C.invalidate_step_state()
