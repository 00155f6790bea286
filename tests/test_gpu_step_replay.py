"""GPU: every convolution / GEMM launch of a real train step, replayed at the C ABI and checked ELEMENTWISE against a
float64 reference (tests/fp64_ref.py) with the fp32 bar |got - ref| <= 2^-24 (4 sqrt(K) + 16) m.

One train step runs with the library handle swapped for a recorder (tests/step_record.py); every fi_conv* /
fi_gemm_nt* call is split by its argtypes (_lib.SIGNATURES) into integer arguments and pointer arguments, of which
only NULL / non-NULL is kept, and deduplicated.  Each distinct record is then called again with the same integers on
fresh seeded operands in the layouts the arguments declare (fragment-major 1x1 weights through
fi_weight_transpose_batch), with residual / scale / bias / gate only where the step passed them (gates hold exact
zeros), outputs pre-zeroed under FI_OUTPUTS_ZEROED and NaN otherwise -- so an element the call should write and does not
fails.  Static-capacity entries (_live / _rows) run with device counts {0, 1, N//5, N}: the live part against the
reference, the rest as the header defines it (not written / zero-written, or computed).  The 16-bit entries are compared
with the reference on operands rounded to that type (RNE): their products are exact in fp32, so the same bar holds.
An entry name without a replay handler fails the test."""
import collections
import ctypes
import math
import time

import numpy as np
import pytest
import torch

import fp64_ref as R
import step_record

DEV = "cuda:0"

_XIN = ["N", "Cin", "H", "W", "Cout", "R", "S", "sh", "sw", "ph", "pw"]
_FWD = _XIN + ["relu", "layout", "oh", "ow", "ocl"]
# entry point -> (family, argument names in C order); the names in _PTRS are pointers, every other one an integer
_PTRS = {"x", "w", "w16", "bias", "scale", "residual", "gate", "y", "dy", "dw", "dbias", "xs", "dys", "dws", "dbs", "a", "b", "c",
         "ws", "live", "stream"}
SPECS = {
    "fi_conv2d_forward": ("fwd", ["x", "w", "bias", "scale", "residual", "y"] + _FWD + ["stream"]),
    "fi_conv2d_forward_gated": ("fwd", ["x", "w", "bias", "scale", "residual", "gate", "y"] + _FWD + ["stream"]),
    "fi_conv2d_forward_live": ("fwd", ["x", "w", "bias", "scale", "residual", "gate", "y"] + _FWD + ["live", "stream"]),
    "fi_conv3x3_forward_bf16w": ("fwd3x3w", ["x", "w", "bias", "scale", "residual", "y", "N", "Cin", "H", "W", "Cout",
                                             "relu", "flip", "stream"]),
    "fi_conv3x3_forward_gated_bf16w": ("fwd3x3w", ["x", "w", "bias", "scale", "residual", "gate", "y", "N", "Cin", "H",
                                                   "W", "Cout", "relu", "flip", "stream"]),
    "fi_conv1x1_forward_bf16w": ("fwd1x1w", ["x", "w", "bias", "scale", "residual", "y", "N", "Cin", "HW", "Cout", "relu",
                                             "stream"]),
    "fi_conv1x1_forward_gated_bf16w": ("fwd1x1w", ["x", "w", "bias", "scale", "residual", "gate", "y", "N", "Cin", "HW",
                                                   "Cout", "relu", "stream"]),
    "fi_conv2d_weight_grad": ("wgrad", ["x", "dy", "dw"] + _XIN + ["layout", "dbias", "flags", "stream"]),
    "fi_conv2d_weight_grad_bf16": ("wgrad", ["x", "dy", "dw"] + _XIN + ["flags", "stream"]),
    "fi_conv2d_weight_grad_db_bf16": ("wgrad", ["x", "dy", "dw", "dbias"] + _XIN + ["flags", "stream"]),
    "fi_conv2d_weight_grad_rows_bf16": ("wgrad", ["x", "dy", "dw"] + _XIN + ["flags", "live", "stream"]),
    "fi_conv2d_weight_grad_batch": ("wgrad_batch", ["xs", "dys", "dws", "dbs", "n"] + _XIN + ["layout", "flags", "stream"]),
    "fi_gemm_nt": ("gemm", ["a", "b", "bias", "c", "M", "N", "K", "relu", "ws", "stream"]),
    "fi_gemm_nt_rows": ("gemm", ["a", "b", "bias", "c", "M", "N", "K", "relu", "ws", "live", "stream"]),
    "fi_gemm_nt_affine": ("gemm", ["a", "b", "scale", "bias", "c", "M", "N", "K", "relu", "ws", "live", "stream"]),
}
for _stem in ("fi_conv2d_forward", "fi_conv2d_forward_gated", "fi_conv2d_forward_live"):
    for _t in ("bf16", "f16"):
        SPECS["%s_%s" % (_stem, _t)] = SPECS[_stem]
for _t in ("bf16", "f16"):      # the planned entry of the 16-bit path also takes the weights' 16-bit copy (or NULL)
    SPECS["fi_conv2d_forward_live_" + _t] = ("fwd", ["x", "w", "w16", "bias", "scale", "residual", "gate", "y"] + _FWD +
                                             ["live", "stream"])
for _n in list(SPECS):
    if _n.endswith("_bf16w"):
        SPECS[_n.replace("_bf16w", "_f16w")] = SPECS[_n]
    if _n.startswith("fi_conv2d_weight_grad") and _n.endswith("_bf16"):
        SPECS[_n.replace("_bf16", "_f16")] = SPECS[_n]
for _t in ("bf16", "f16"):
    SPECS["fi_conv2d_weight_grad_batch_" + _t] = SPECS["fi_conv2d_weight_grad_batch"]


def recorded_entry(name):
    """The launches the replay covers: every fi_conv* / fi_gemm_nt* entry except the host-side queries."""
    return (name.startswith("fi_conv") or name.startswith("fi_gemm_nt")) and \
        not name.endswith("_eligible") and not name.endswith("_workspace_bytes") and \
        not name.endswith("_plan") and "_plan_" not in name and not name.endswith("_layout") and \
        not name.endswith("_launch") and not name.endswith("_launches")


def lowp_dtype(name):
    if "bf16" in name:
        return torch.bfloat16
    if "f16" in name:
        return torch.float16
    return None


def test_replay_specs_match_the_library_signatures():
    """(CPU) every recorded entry point of _lib.SIGNATURES has a replay spec whose argument list matches its argtypes:
    integers where the spec names an integer, pointers where it names a tensor."""
    from feature_intertwiner_amd import _lib
    names = [n for n in _lib.SIGNATURES if recorded_entry(n)]
    assert len(names) >= 30
    missing = [n for n in names if n not in SPECS]
    assert not missing, missing
    for n in names:
        fam, args = SPECS[n]
        types = _lib.SIGNATURES[n][1]
        assert len(args) == len(types), (n, len(args), len(types))
        for a, t in zip(args, types):
            is_int = t in (ctypes.c_int, ctypes.c_long)
            assert is_int == (a not in _PTRS), (n, a, t)


# ---- recording (tests/step_record.py) ------------------------------------------------------------------------------------
def _record_step(cfg_kw, size, batch_size, steps=2):
    records, model = step_record.record_step(cfg_kw, size, batch_size, recorded_entry, SPECS, _PTRS, steps=steps)
    del model
    torch.cuda.empty_cache()
    return records


# ---- replay -------------------------------------------------------------------------------------------------------------
class _Ctx(object):
    def __init__(self, seed):
        self.g = torch.Generator(device=DEV).manual_seed(seed)

    def randn(self, *shape, scale=1.0):
        t = torch.randn(*shape, generator=self.g, device=DEV, dtype=torch.float32)
        return t * scale if scale != 1.0 else t

    def gate(self, *shape):
        t = self.randn(*shape)
        t[torch.rand(*shape, generator=self.g, device=DEV) < 0.25] = 0.0       # exact zeros: (gate > 0) is 0 there
        return t


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV, dtype=torch.float32)


def _round(t, dt):
    return t if dt is None else t.to(dt).float()


def _frag_major(W):
    """Fragment-major copy of a [M][K] matrix (flags 1 | 2 of FiTransposeDesc: D = src), as weight_layout 3 reads it."""
    from feature_intertwiner_amd import _lib
    from feature_intertwiner_amd.conv import _TR_DESC
    M, K = W.shape
    dst = torch.empty(M * K, device=DEV, dtype=torch.float32)
    desc = np.zeros(1, dtype=_TR_DESC)
    desc[0] = (W.data_ptr(), dst.data_ptr(), M, K, 1, 3, 0, 0)
    table = torch.from_numpy(desc.view(np.uint8).copy()).to(DEV)
    tiles = ((M + 31) // 32) * ((K + 31) // 32)
    _lib.check(_lib.load().fi_weight_transpose_batch(_lib.ptr(table), 1, tiles, _lib.current_stream()),
               "fi_weight_transpose_batch")
    torch.cuda.synchronize()
    return dst


def _live_counts(n):
    return sorted({0, 1, n // 5, n}) if n > 1 else [0, n]


def _check_live(got, ref, mag, n, live, dim, dead_ok, what):
    """Elements with index < live along `dim` against the reference; the rest either as dead_ok allows (NaN = not
    written, 0 = zero-written) or computed (within the bar)."""
    worst = 0.0
    sl = [slice(None)] * got.dim()
    sl[dim] = slice(0, live)
    if live > 0:
        worst = R.check_bar(got[tuple(sl)], ref[tuple(sl)], mag[tuple(sl)], n, what + " live part")
    sl[dim] = slice(live, None)
    g, r, m = got[tuple(sl)].to(torch.float64), ref[tuple(sl)], mag[tuple(sl)]
    if g.numel():
        allowed = torch.zeros_like(g, dtype=torch.bool)
        if "nan" in dead_ok:
            allowed |= torch.isnan(g)
        if "zero" in dead_ok:
            allowed |= g == 0
        g = torch.where(allowed, r, g)
        R.check_bar(g, r, m, n, what + " dead part")
    return worst


def _replay_fwd(name, fam, I, nul, ctx):
    from feature_intertwiner_amd import _lib
    L = _lib.load()
    dt = lowp_dtype(name)
    N, Cin, Cout = I["N"], I["Cin"], I["Cout"]
    if fam == "fwd":
        H, W, Rr, S = I["H"], I["W"], I["R"], I["S"]
        stride, pad = (I["sh"], I["sw"]), (I["ph"], I["pw"])
        relu, layout, ocl = I["relu"], I["layout"], I["ocl"]
        OH, OW = (I["oh"], I["ow"]) if I["oh"] > 0 else R.out_size(H, W, Rr, S, stride, pad)
    elif fam == "fwd3x3w":
        H, W, Rr, S, stride, pad = I["H"], I["W"], 3, 3, (1, 1), (1, 1)
        relu, layout, ocl, OH, OW = I["relu"], 2 if I["flip"] else 1, 0, I["H"], I["W"]
    else:
        H, W, Rr, S, stride, pad = 1, I["HW"], 1, 1, (1, 1), (0, 0)
        relu, layout, ocl, OH, OW = I["relu"], 1, 0, 1, I["HW"]
    K = Cin * Rr * S
    x = ctx.randn(N, Cin, H, W)
    ws = 1.0 / math.sqrt(K)
    if layout == 0:
        w = ctx.randn(Cout, Cin, Rr, S, scale=ws)
        wl = w
    elif layout in (1, 2):
        w = ctx.randn(Cout, Rr, S, Cin, scale=ws)
        wl = w.permute(0, 3, 1, 2)
    else:
        assert layout == 3 and Rr * S == 1, I
        W2 = ctx.randn(Cout, Cin, scale=ws)
        w = _frag_major(W2)
        wl = W2.view(Cout, Cin, 1, 1)
    if fam != "fwd":                      # weights handed over in 16 bits
        w = w.to(dt)
        wl = w.float().permute(0, 3, 1, 2) if fam == "fwd3x3w" else w.float().view(Cout, Cin, 1, 1)
    else:
        wl = _round(wl, dt)
    out_shape = (N, Cout, OH, OW)
    bias = None if nul["bias"] else ctx.randn(Cout)
    scale = None if nul["scale"] else ctx.randn(Cout)
    residual = None if nul["residual"] else ctx.randn(*out_shape)
    gate = None if nul.get("gate", True) else ctx.gate(*out_shape)
    has_live = "live" in nul and not nul["live"]
    xr = _round(x, dt)
    acc = R.conv_ref(xr, wl, stride, pad, (OH, OW), tap_reversed=layout == 2)
    ref = R.epilogue(acc, scale, bias, residual, bool(relu), gate)
    del acc
    mag = R.abs_epilogue(R.conv_ref(xr.abs(), wl.abs(), stride, pad, (OH, OW), tap_reversed=layout == 2),
                         scale, bias, residual)
    del xr
    worst = 0.0
    for live in (_live_counts(N) if has_live else [None]):
        y = _nan(N, OH, OW, Cout) if ocl else _nan(*out_shape)
        # the 16-bit copy where the step handed one over: the same weights in the declared layout
        w16 = None if nul.get("w16", True) else w.to(dt)
        P = {"x": x, "w": w, "w16": w16, "bias": bias, "scale": scale, "residual": residual, "gate": gate, "y": y}
        lv = None if live is None else torch.tensor([live], device=DEV, dtype=torch.int32)
        args = []
        for k in SPECS[name][1]:
            if k == "stream":
                args.append(_lib.current_stream())
            elif k == "live":
                args.append(_lib.ptr(lv))
            elif k not in _PTRS:
                args.append(I[k])
            else:
                args.append(_lib.ptr(P[k]))
        _lib.check(getattr(L, name)(*args), "replay " + name)
        torch.cuda.synchronize()
        got = y.permute(0, 3, 1, 2) if ocl else y
        what = "%s %s live=%s" % (name, I, live)
        if live is None:
            worst = max(worst, R.check_bar(got, ref, mag, K, what))
        else:
            worst = max(worst, _check_live(got, ref, mag, K, live, 0, ("nan",), what))
        del y, got
    return worst


def _wgrad_problem(name, I, nul, ctx, zeroed, tap_major):
    N, Cin, H, W, Cout, Rr, S = (I[k] for k in ("N", "Cin", "H", "W", "Cout", "R", "S"))
    stride, pad = (I["sh"], I["sw"]), (I["ph"], I["pw"])
    OH, OW = R.out_size(H, W, Rr, S, stride, pad)
    x = ctx.randn(N, Cin, H, W)
    dy = ctx.randn(N, Cout, OH, OW)
    fill = (lambda *s: torch.zeros(s, device=DEV)) if zeroed else _nan
    dw = fill(Cout, Rr, S, Cin) if tap_major else fill(Cout, Cin, Rr, S)
    db = None if nul.get("dbias", True) else fill(Cout)
    return x, dy, dw, db, stride, pad, N * OH * OW


def _wgrad_check(name, I, x, dy, dw, db, stride, pad, n, tap_major, live=None):
    dt = lowp_dtype(name)
    Cout, Rr, S = I["Cout"], I["R"], I["S"]
    xr, dyr = _round(x, dt), _round(dy, dt)
    ref = R.wgrad_ref(xr, dyr, Rr, S, stride, pad)
    mag = R.wgrad_ref(xr.abs(), dyr.abs(), Rr, S, stride, pad)
    got = dw.permute(0, 3, 1, 2) if tap_major else dw
    what = "%s %s live=%s" % (name, I, live)
    if live is None:
        worst = R.check_bar(got, ref, mag, n, what)
    else:
        # rows past the live count: zero (filled by the call, or pre-zeroed under FI_OUTPUTS_ZEROED) or computed
        worst = _check_live(got, ref, mag, n, live, 0, ("zero",), what)
    if db is not None:
        # the bias gradient sums the fp32 dy (the 16-bit kernels add up the values before rounding them)
        worst = max(worst, R.check_bar(db, dy.double().sum((0, 2, 3)), dy.double().abs().sum((0, 2, 3)), n,
                                       what + " dbias"))
    return worst


def _replay_wgrad(name, I, nul, ctx):
    from feature_intertwiner_amd import _lib
    L = _lib.load()
    tap_major = lowp_dtype(name) is not None or I.get("layout", 0) == 1
    zeroed = bool(I["flags"] & 1)
    x, dy, dw, db, stride, pad, n = _wgrad_problem(name, I, nul, ctx, zeroed, tap_major)
    has_live = "live" in nul and not nul["live"]
    worst = 0.0
    for live in (_live_counts(I["Cout"]) if has_live else [None]):
        if live is not None:
            dw.fill_(0.0 if zeroed else float("nan"))
        P = {"x": x, "dy": dy, "dw": dw, "dbias": db}
        lv = None if live is None else torch.tensor([live], device=DEV, dtype=torch.int32)
        args = []
        for k in SPECS[name][1]:
            if k == "stream":
                args.append(_lib.current_stream())
            elif k == "live":
                args.append(_lib.ptr(lv))
            elif k not in _PTRS:
                args.append(I[k])
            else:
                args.append(_lib.ptr(P[k]))
        _lib.check(getattr(L, name)(*args), "replay " + name)
        torch.cuda.synchronize()
        worst = max(worst, _wgrad_check(name, I, x, dy, dw, db if live is None else None, stride, pad, n, tap_major,
                                        live))
    return worst


def _replay_wgrad_batch(name, I, nul, ctx):
    from feature_intertwiner_amd import _lib
    L = _lib.load()
    tap_major = lowp_dtype(name) is not None or I["layout"] == 1
    zeroed = bool(I["flags"] & 1)
    probs = [_wgrad_problem(name, I, {"dbias": nul["dbs"]}, ctx, zeroed, tap_major) for _ in range(I["n"])]
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    xs, dys, dws = arr([p[0] for p in probs]), arr([p[1] for p in probs]), arr([p[2] for p in probs])
    dbs = None if nul["dbs"] else arr([p[3] for p in probs])
    ints = [I[k] for k in ("n",) + tuple(_XIN) + ("layout", "flags")]
    _lib.check(getattr(L, name)(xs, dys, dws, dbs, *ints, _lib.current_stream()), "replay " + name)
    torch.cuda.synchronize()
    worst = 0.0
    for i in range(len(probs)):
        x, dy, dw, db, stride, pad, n = probs[i]
        worst = max(worst, _wgrad_check(name + "[%d/%d]" % (i, I["n"]), I, x, dy, dw, db, stride, pad, n, tap_major))
        probs[i] = None
    return worst


def _replay_gemm(name, I, nul, ctx):
    from feature_intertwiner_amd import _lib
    L = _lib.load()
    M, N, K = I["M"], I["N"], I["K"]
    a, b = ctx.randn(M, K), ctx.randn(N, K, scale=1.0 / math.sqrt(K))
    bias = None if nul["bias"] else ctx.randn(N)
    scale = None if nul.get("scale", True) else ctx.randn(N)
    ws = torch.empty((int(L.fi_gemm_nt_workspace_bytes(M, N, K)) + 3) // 4, device=DEV, dtype=torch.float32)
    ref = R.epilogue(R.linear_ref(a, b), scale, bias, relu=bool(I["relu"]))
    mag = R.abs_epilogue(R.linear_ref(a.abs(), b.abs()), scale, bias)
    has_live = "live" in nul and not nul["live"]
    worst = 0.0
    for live in (_live_counts(M) if has_live else [None]):
        c = _nan(M, N)
        P = {"a": a, "b": b, "bias": bias, "scale": scale, "c": c, "ws": ws}
        lv = None if live is None else torch.tensor([live], device=DEV, dtype=torch.int32)
        args = []
        for k in SPECS[name][1]:
            if k == "stream":
                args.append(_lib.current_stream())
            elif k == "live":
                args.append(_lib.ptr(lv))
            elif k not in _PTRS:
                args.append(I[k])
            else:
                args.append(_lib.ptr(P[k]))
        _lib.check(getattr(L, name)(*args), "replay " + name)
        torch.cuda.synchronize()
        what = "%s %s live=%s" % (name, I, live)
        if live is None:
            worst = max(worst, R.check_bar(c, ref, mag, K, what))
        else:
            # rows past the live count rounded up to the tile height are written as zeros
            worst = max(worst, _check_live(c, ref, mag, K, live, 0, ("zero",), what))
    return worst


def replay(records, label):
    t0 = time.time()
    count = collections.Counter()
    worst = collections.defaultdict(float)
    unhandled = sorted({r[0] for r in records if r[0] not in SPECS})
    failures = []
    for i, (name, ints, nulls) in enumerate(records):
        if name not in SPECS:
            continue
        fam = SPECS[name][0]
        I, nul = dict(ints), dict(nulls)
        ctx = _Ctx(1000 + i)
        try:
            if fam.startswith("fwd"):
                w = _replay_fwd(name, fam, I, nul, ctx)
            elif fam == "wgrad":
                w = _replay_wgrad(name, I, nul, ctx)
            elif fam == "wgrad_batch":
                w = _replay_wgrad_batch(name, I, nul, ctx)
            else:
                w = _replay_gemm(name, I, nul, ctx)
            worst[name] = max(worst[name], w)
        except AssertionError as e:
            failures.append(str(e)[:600])
        count[name] += 1
        del ctx
    torch.cuda.empty_cache()
    wall = time.time() - t0
    print("\n[%s] %d distinct records replayed in %.1f s; unhandled entry names: %d %s" % (
        label, sum(count.values()), wall, len(unhandled), unhandled))
    for name in sorted(count):
        print("  %-40s records %4d   worst |d|/(2^-24 m) %8.2f" % (name, count[name], worst[name]))
    return count, unhandled, failures


WORKLOADS = [
    ("configs[2] fp32", dict(backbone="resnet101", image_size=1024, batch_size=4, train_rois_per_image=512,
                             dev_switch=True, loss_choice="ot", ot_L=50), 1024, 4),
    ("configs[4] slice bf16", dict(backbone="resnet101", image_size=1344, batch_size=2, train_rois_per_image=1000,
                                   dev_switch=True, loss_choice="ot", ot_L=50, conv_precision="bf16"), 1344, 2),
    ("configs[4] slice fp16", dict(backbone="resnet101", image_size=1344, batch_size=2, train_rois_per_image=1000,
                                   dev_switch=True, loss_choice="ot", ot_L=50, conv_precision="fp16"), 1344, 2),
]


@pytest.mark.gpu
@pytest.mark.parametrize("label,kw,size,bs", WORKLOADS, ids=["configs2_fp32", "configs4_bf16", "configs4_fp16"])
def test_step_conv_launches_match_fp64_elementwise(label, kw, size, bs):
    t0 = time.time()
    records = _record_step(kw, size, bs)
    t_rec = time.time() - t0
    count, unhandled, failures = replay(records, label)
    print("[%s] wall time %.1f s (step recording %.1f s)" % (label, time.time() - t0, t_rec))
    assert not unhandled, "recorded entry points without a replay handler: %s" % unhandled
    assert not failures, "%d of %d records off the bar:\n%s" % (len(failures), sum(count.values()),
                                                                "\n".join(failures[:20]))
    fams = collections.Counter(SPECS[n][0] for n in count)
    assert fams["wgrad"] + fams["wgrad_batch"] > 0 and fams["fwd"] > 0, count
    if "fp32" in label:
        for n in ("fi_conv2d_forward_live", "fi_conv2d_weight_grad", "fi_conv2d_weight_grad_batch", "fi_gemm_nt_affine"):
            assert count[n] > 0, (n, count)
    else:
        t = "bf16" if "bf16" in label else "f16"
        assert sum(c for n, c in count.items() if n.endswith(t) or n.endswith(t + "w")) > 0, count
