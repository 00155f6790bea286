"""fi_conv2d_weight_grad_batch on the Winograd F(2x2,3x3) form of the 3x3 slot (csrc/conv3x3_wino_wgrad.hip with a
fi::WgradBatch): batches of 2 and 3 problems with operands of their own at the smallest shape the rule sends there (the
floor of tests/test_wino_wgrad_batch_plan.py, found through the query), one launch each.  Every problem's dW and dbias is held
to float64 with the bar of tests/test_gpu_conv_wino_wgrad.py, 2^-24 (4 sqrt(n) + 16) m; the outputs of a problem past the
batch's count keep their guard values; the same batch on the direct kernel (FI_NO_WINOGRAD_WGRAD=1) is within the bar of
it."""
import ctypes
import functools
import os

import pytest
import torch

import fp64_ref as R
from test_wino_wgrad_batch_plan import N, W, floor_height

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SWITCH = "FI_NO_WINOGRAD_WGRAD"
CIN = COUT = 256
GUARD = -12345.5


@functools.lru_cache(maxsize=None)
def _shape():
    H = floor_height()
    assert H is not None
    return (N, CIN, H, W, COUT)


@functools.lru_cache(maxsize=None)
def _problem(i):
    """Operands of problem i and their float64 dW (tap-major), its m, dbias, its m -- computed once, never written."""
    n_, Cin, H, w, Cout = _shape()
    g = torch.Generator(device=DEV).manual_seed(11000 + i)
    x = torch.randn(n_, Cin, H, w, device=DEV, generator=g)
    dy = torch.randn(n_, Cout, H, w, device=DEV, generator=g)
    ref = R.wgrad_ref(x, dy, 3, 3, (1, 1), (1, 1)).permute(0, 2, 3, 1)
    mag = R.wgrad_ref(x.abs(), dy.abs(), 3, 3, (1, 1), (1, 1)).permute(0, 2, 3, 1)
    return x, dy, ref, mag, dy.double().sum((0, 2, 3)), dy.double().abs().sum((0, 2, 3))


def _batch(n, with_db, switched=False):
    """One fi_conv2d_weight_grad_batch call of n problems (the pointer tables hold one problem more, which the call must
    not touch).  Returns (plan, launches counted in the slot, dWs, dbiases), the last of each being the guard."""
    from feature_intertwiner_amd import _lib
    L = _lib.load()
    n_, Cin, H, w, Cout = _shape()
    geom = (n_, Cin, H, w, Cout, 3, 3, 1, 1, 1, 1)
    probs = [_problem(i) for i in range(n + 1)]
    dws = [torch.zeros(Cout, 3, 3, Cin, device=DEV) for _ in range(n)] + [torch.full((Cout, 3, 3, Cin), GUARD, device=DEV)]
    dbs = [torch.zeros(Cout, device=DEV) for _ in range(n)] + [torch.full((Cout,), GUARD, device=DEV)]
    arr = lambda ts: (ctypes.c_void_p * (n + 1))(*[t.data_ptr() for t in ts])

    def go():
        (p,) = _lib.planned_launches(L.fi_conv2d_weight_grad_launch, _lib.ptr(probs[0][0]), _lib.ptr(probs[0][1]), _lib.ptr(dws[0]),
                                     *geom, 1, _lib.ptr(dbs[0]) if with_db else None, _lib.OUTPUTS_ZEROED, n)
        key = _lib.KERNEL_KEYS[p.kernel_id]
        _lib.prof_reset()
        _lib.prof_enable(True)
        try:
            _lib.check(L.fi_conv2d_weight_grad_batch(arr([q[0] for q in probs]), arr([q[1] for q in probs]), arr(dws),
                                                     arr(dbs) if with_db else None, n, *geom, 1, _lib.OUTPUTS_ZEROED,
                                                     _lib.current_stream()), "fi_conv2d_weight_grad_batch")
            torch.cuda.synchronize()
        finally:
            _lib.prof_enable(False)
        return p, _lib.prof_get(key)[0]

    if switched:
        assert SWITCH not in os.environ
        os.environ[SWITCH] = "1"
        try:
            p, count = go()
        finally:
            del os.environ[SWITCH]
    else:
        p, count = go()
    return p, count, dws, dbs


@pytest.mark.parametrize("n,with_db", [(2, True), (3, True), (3, False)])
def test_batched_winograd_weight_gradient_is_the_float64_reference(n, with_db):
    from feature_intertwiner_amd import _lib
    n_, Cin, H, w, Cout = _shape()
    pixels = n_ * H * w
    p, count, dws, dbs = _batch(n, with_db)
    assert p.flags & _lib.LAUNCH_FLAGS["winograd"] and p.per_launch == n and count == 1
    d, dcount, ddws, ddbs = _batch(n, with_db, switched=True)
    assert not d.flags & _lib.LAUNCH_FLAGS["winograd"] and d.per_launch == n and dcount == 1 and d.kernel_id == p.kernel_id
    worst = worst_db = worst_direct = 0.0
    for i in range(n):
        x, dy, ref, mag, db_ref, db_mag = _problem(i)
        worst = max(worst, R.check_bar(dws[i], ref, mag, pixels, "problem %d of %d dW" % (i, n)))
        worst_direct = max(worst_direct, R.check_bar(ddws[i], ref, mag, pixels, "problem %d of %d dW, direct" % (i, n)))
        R.check_bar(dws[i], ddws[i].double(), mag, pixels, "problem %d of %d dW against the direct batch" % (i, n))
        assert not torch.equal(dws[i], ddws[i])                      # two kernels
        if with_db:
            worst_db = max(worst_db, R.check_bar(dbs[i], db_ref, db_mag, pixels, "problem %d of %d dbias" % (i, n)))
            R.check_bar(dbs[i], ddbs[i].double(), db_mag, pixels, "problem %d of %d dbias against the direct batch" % (i, n))
        else:
            assert bool((dbs[i] == 0).all())
    for t in (dws[n], dbs[n], ddws[n], ddbs[n]):
        assert bool((t == GUARD).all()), "a problem past the batch's count was written"
    print("batch of %d on %s, dbias %s: %d splits of %d tiles a problem, worst |d|/(2^-24 m) dW %.2f (direct batch %.2f) dbias %.2f" % (
        n, _shape(), with_db, p.splits, p.pixels_per_split // 4, worst, worst_direct, worst_db))
