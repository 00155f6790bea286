"""GPU: the non-convolution launches of real train steps -- the BatchNorm / fully connected backward passes, the mask
head's class-row backward, the RPN's patch rows, the row gathers, pooling / upsampling / ReLU / interleave glue, the
weight transposes and BatchNorm folds, and the clip + SGD step -- replayed at the C ABI and checked elementwise against
float64 (tests/fp64_ref.py) or bit for bit.

Two steps of each workload run with the recorder of tests/step_record.py, which keeps the numeric arguments, the NULL
pattern and the address modulo 16 of every pointer (plus what the handlers' `extra` functions read: host pointer
arrays, device descriptor tables, aliasing).  Each distinct record is replayed on fresh seeded operands at the same
misalignment, shaped like the step's (exact zeros in ReLU outputs and gates, all-zero class rows, padding rows, level
starts and map borders, distinct indices, a gamma == 0 channel and |beta| / |gamma| >> 1).  Write-only outputs are
pre-filled with NaN; accumulated ones with random finite values and checked by their increment.  Every operand built at
a chosen misalignment sits between two guard zones of sentinel floats, which must be intact after the launch (a store a
few elements before a buffer or past its tail is an error even where the allocation has room).  The clip + SGD step is
checked in-step: every parameter, gradient and momentum buffer is snapshotted before optim.clip_and_step.

fi_bn_act_backward and gamma == 0: the kernel recovers xhat as (y - beta) / gamma from the forward's output, which holds
no xhat where gamma == 0; include/fi_capi.h documents that dgamma is written as 0 there and that the error of dgamma
grows with (|y| + |residual| + |beta|) / |gamma|.  The replay checks exactly that (the m of the bar carries the term,
the gamma == 0 channel must read 0).  Each workload prints the recorded model's worst |beta| / |gamma| and its number of
gamma == 0 channels (informational: the models start from gamma = 1, and no caller checks gamma)."""
import collections
import ctypes
import math
import os
import time

import numpy as np
import pytest
import torch

import fp64_ref as R
import step_record
from step_record import DEV

HERE = os.path.dirname(os.path.abspath(__file__))
TINY = 2.0 ** -126                      # smallest normal fp32

_PTRS = {"dy", "y", "scale", "gamma", "beta", "residual", "dz", "g_out", "dshift", "dgamma", "dbias", "dw", "w", "s",
         "mean", "var", "conv_bias", "g", "gs", "colsum", "bias", "d", "x", "weight", "cls", "dx", "dweight", "workspace",
         "maps", "grads", "heights", "widths", "image", "anchor", "out", "src", "index", "dst", "front", "src_row",
         "c00", "c01", "c10", "c11", "add", "gate", "table", "partial", "norm_coef", "dets", "keep", "num", "proposals",
         "dws", "ws", "ss", "scales", "means", "vars", "cbs", "dgammas", "dbiases", "stream"}
SPECS = {
    "fi_bn_act_backward": ("bn_act", ["dy", "y", "scale", "gamma", "beta", "residual", "N", "C", "HW", "relu", "dz",
                                      "g_out", "dshift", "dgamma", "dbias", "layout", "flags", "stream"]),
    "fi_bn_fold_grad": ("fold", ["dw", "w", "s", "scale", "mean", "var", "eps", "conv_bias", "dgamma", "dbias", "Cout",
                                 "Cin", "taps", "dw_tap_major", "w_tap_major", "stream"]),
    "fi_bn_fold_grad_batch": ("fold_batch", ["dws", "ws", "ss", "scales", "means", "vars", "eps", "cbs", "dgammas",
                                             "dbiases", "n", "Cout", "Cin", "taps", "dw_tap_major", "w_tap_major",
                                             "stream"]),
    "fi_rows_mask_scale": ("rows_mask", ["dy", "y", "scale", "g", "gs", "colsum", "M", "N", "ld_out", "relu", "flags",
                                         "stream"]),
    "fi_rows_affine_act": ("rows_affine", ["y", "scale", "bias", "M", "N", "relu", "stream"]),
    "fi_class_row_conv1x1_backward": ("class_row", ["d", "x", "weight", "cls", "dx", "dweight", "dbias", "N", "C", "HW",
                                                    "num_classes", "gated", "workspace", "stream"]),
    "fi_pyramid_patch_rows_forward": ("patch_fwd", ["maps", "heights", "widths", "levels", "per_loc", "image", "anchor",
                                                    "rows", "channels", "out", "stream"]),
    "fi_pyramid_patch_rows_backward": ("patch_bwd", ["d", "grads", "heights", "widths", "levels", "per_loc", "image",
                                                     "anchor", "rows", "channels", "stream"]),
    "fi_rows_gather": ("rows_gather", ["src", "index", "dst", "n_index", "row_len", "stream"]),
    "fi_rows_scatter_add": ("rows_scatter", ["src", "index", "dst", "n_index", "row_len", "stream"]),
    "fi_rows_combine": ("rows_combine", ["front", "n_front", "src", "src_row", "dst", "rows", "row_len", "stream"]),
    "fi_maxpool3x3s2_forward": ("pool_fwd", ["x", "y", "planes", "height", "width", "stream"]),
    "fi_maxpool3x3s2_backward": ("pool_bwd", ["dy", "x", "dx", "planes", "height", "width", "positive_only", "stream"]),
    "fi_sum2x2": ("sum2x2", ["dy", "out", "planes", "height", "width", "stream"]),
    "fi_relu_mask": ("relu_mask", ["dy", "y", "out", "n", "stream"]),
    "fi_stride2_interleave": ("interleave", ["c00", "c01", "c10", "c11", "add", "dx", "planes", "height", "width",
                                             "stream"]),
    "fi_stride2_interleave_gated": ("interleave", ["c00", "c01", "c10", "c11", "add", "gate", "dx", "planes", "height",
                                                   "width", "stream"]),
    "fi_weight_transpose_batch": ("transpose", ["table", "n", "total_tiles", "stream"]),
    "fi_bn_fold_batch": ("bn_fold", ["table", "n", "max_channels", "stream"]),
    "fi_proposal_gather": ("gather_props", ["dets", "pre_nms", "det_stride", "keep", "keep_stride", "num", "batch",
                                            "proposal_count", "norm_h", "norm_w", "proposals", "stream"]),
    "fi_sgd_clip_step": ("sgd", ["table", "n", "total_chunks", "max_norm", "partial", "norm_coef", "stream"]),
    "fi_sgd_clip_step_guarded": ("sgd", ["table", "n", "total_chunks", "max_norm", "partial", "norm_coef", "stream"]),
}

# device entries checked by other tests (the step-level ones by the headline / crop / detector tests)
CHECKED_ELSEWHERE = {
    "fi_crop_and_resize_forward": "tests/test_gpu_crop.py::test_forward_bit_exact_adversarial",
    "fi_crop_and_resize_backward": "tests/test_gpu_crop.py::test_backward_vs_oracle",
    "fi_crop_and_resize_taps": "tests/test_gpu_crop.py::test_taps_bit_exact",
    "fi_pyramid_crop_forward": "tests/test_gpu_crop.py::test_pyramid_matches_per_level_oracle",
    "fi_pyramid_crop_backward": "tests/test_gpu_crop.py::test_pyramid_matches_per_level_oracle",
    "fi_pyramid_crop_forward_nhwc": "tests/test_gpu_crop.py::test_pyramid_channels_last_matches_per_level_oracle",
    "fi_pyramid_crop_backward_nhwc": "tests/test_gpu_crop.py::test_pyramid_channels_last_matches_per_level_oracle",
    # the NCHW accumulating form is never reached in-step (configs[0]'s Dev stage is off); the channels-last one is
    # checked in-step by tests/test_gpu_headline_config.py::test_configs2_full_size_two_steps_operators_vs_oracle
    "fi_pyramid_crop_backward_accumulate":
        "tests/test_gpu_crop.py::test_accumulating_pyramid_crop_backward_matches_fp64_elementwise",
    "fi_pyramid_crop_backward_nhwc_accumulate":
        "tests/test_gpu_headline_config.py::test_configs2_full_size_two_steps_operators_vs_oracle",
    "fi_roi_pool_forward": "tests/test_gpu_roipool.py::test_forward_exact",
    "fi_roi_pool_backward": "tests/test_gpu_roipool.py::test_backward_vs_oracle",
    "fi_nms_sorted": "tests/test_gpu_nms.py::test_pth_nms_matches_oracle",
    "fi_sinkhorn_forward": "tests/test_gpu_loss_kernels.py::test_sinkhorn_forward_matches_fp64",
    "fi_class_mean_forward": "tests/test_gpu_loss_kernels.py::test_class_mean_matches_fp64",
    "fi_class_mean_backward": "tests/test_gpu_loss_kernels.py::test_class_mean_matches_fp64",
    "fi_detector_losses": "tests/test_gpu_loss_kernels.py::test_detector_losses_match_fp64_at_the_edge_shapes",
    "fi_rpn_targets": "tests/test_gpu_targets.py::test_rpn_target_kernels_equal_the_tensor_formulation",
    "fi_detection_targets": "tests/test_gpu_targets.py::test_detection_target_kernel_equals_the_tensor_formulation",
    "fi_meta_stats_forward": "tests/test_gpu_loss_kernels.py::test_meta_stats_match_fp64",
    "fi_meta_stats_backward": "tests/test_gpu_loss_kernels.py::test_meta_stats_match_fp64",
    "fi_meta_stats_sums": "tests/test_gpu_loss_kernels.py::test_meta_stats_match_fp64",
    "fi_meta_stats_from_sums": "tests/test_gpu_loss_kernels.py::test_meta_stats_match_fp64",
    "fi_dev_stage_index": "tests/test_gpu_static_dev.py::test_index_kernel_equals_its_tensor_formulation",
    "fi_proposal_candidates": "tests/test_gpu_detector.py::test_proposal_candidates_edge_cases",
    "fi_proposal_candidates_ws": "tests/test_gpu_detector.py::test_proposal_candidates_edge_cases",
}
# host-side queries and settings; fi_calib_copy is bench.py's calibration copy, never part of a step
HOST_ONLY = {"fi_calib_copy", "fi_version", "fi_last_error", "fi_prof_enable", "fi_prof_reset", "fi_prof_get", "fi_prof_kernel_name",
             "fi_sgd_chunks", "fi_conv1x1_ring_eligible", "fi_conv2d_forward_plan", "fi_conv2d_weight_grad_plan", "fi_gemm_nt_plan",
             "fi_conv2d_forward_plan_bf16", "fi_conv2d_forward_plan_f16", "fi_conv2d_weight_grad_plan_bf16",
             "fi_conv2d_weight_grad_plan_f16", "fi_conv2d_weight_grad_layout", "fi_conv2d_weight_grad_split_plan",
             "fi_conv2d_forward_launches", "fi_conv2d_weight_grad_launch", "fi_gemm_nt_launch"}


def _conv_specs():
    import test_gpu_step_replay as C
    return C.SPECS


def classify(name):
    groups = []
    if name in _conv_specs():
        groups.append("conv replay")
    if name in SPECS:
        groups.append("glue replay")
    if name in CHECKED_ELSEWHERE:
        groups.append("elsewhere")
    if name in HOST_ONLY or name.endswith("_workspace_bytes"):
        groups.append("host")
    return groups


def test_every_device_entry_is_classified_once():
    """(CPU) every entry of _lib.SIGNATURES falls into exactly one of: the conv replay's SPECS, this file's handlers,
    CHECKED_ELSEWHERE (whose test functions must exist), host-only; and this file's specs match the argtypes."""
    import ast
    from feature_intertwiner_amd import _lib
    bad = {n: classify(n) for n in _lib.SIGNATURES if len(classify(n)) != 1}
    assert not bad, bad
    root = os.path.dirname(HERE)
    for name, where in CHECKED_ELSEWHERE.items():
        path, fn = where.split("::")
        tree = ast.parse(open(os.path.join(root, path)).read())
        assert fn in {f.name for f in tree.body if isinstance(f, ast.FunctionDef)}, (name, where)
    for n, (_, args) in SPECS.items():
        types = _lib.SIGNATURES[n][1]
        assert len(args) == len(types), (n, len(args), len(types))
        for a, t in zip(args, types):
            assert (t in (ctypes.c_int, ctypes.c_long, ctypes.c_float)) == (a not in _PTRS), (n, a, t)
    assert set(HANDLERS) | {"sgd"} == {f for f, _ in SPECS.values()}


# ---- recording: what the pointer arguments alone do not tell -------------------------------------------------------------
def _host_array(v, k):
    return [v[i] for i in range(k)]


def _ex_fold_batch(a):
    n = a["n"] if isinstance(a["n"], int) else a["n"].value
    tab = lambda key: None if step_record.is_null(a[key]) else tuple(
        (x or 0) % 16 if key in ("dws", "ws") else bool(x) for x in _host_array(a[key], n))
    return tuple((key, tab(key)) for key in ("dws", "ws", "cbs", "dgammas", "dbiases"))


def _ex_levels(a):
    k = a["levels"] if isinstance(a["levels"], int) else a["levels"].value
    return (("heights", tuple(_host_array(a["heights"], k))), ("widths", tuple(_host_array(a["widths"], k))))


def _ex_relu_mask(a):
    return (("aliased", step_record.address(a["out"]) == step_record.address(a["dy"])),)


_TR_FIELDS = ("rows", "cols", "taps", "pad")


def _ex_transpose(a):
    from feature_intertwiner_amd.conv import _TR_DESC
    n = a["n"] if isinstance(a["n"], int) else a["n"].value
    d = np.frombuffer(step_record.read_device(step_record.address(a["table"]), n * _TR_DESC.itemsize), dtype=_TR_DESC)
    return tuple((int(r["rows"]), int(r["cols"]), int(r["taps"]), int(r["pad"]), int(r["row_scale"]) != 0) for r in d)


_BN_DESC = np.dtype([("gamma", "<u8"), ("beta", "<u8"), ("mean", "<u8"), ("var", "<u8"), ("cb", "<u8"), ("scale", "<u8"),
                     ("shift", "<u8"), ("ch", "<i4"), ("eps", "<f4")])


def _ex_bn_fold(a):
    n = a["n"] if isinstance(a["n"], int) else a["n"].value
    d = np.frombuffer(step_record.read_device(step_record.address(a["table"]), n * _BN_DESC.itemsize), dtype=_BN_DESC)
    return tuple((int(r["ch"]), float(r["eps"]), int(r["cb"]) != 0) for r in d)


EXTRA = {"fi_bn_fold_grad_batch": _ex_fold_batch, "fi_pyramid_patch_rows_forward": _ex_levels,
         "fi_pyramid_patch_rows_backward": _ex_levels, "fi_relu_mask": _ex_relu_mask,
         "fi_weight_transpose_batch": _ex_transpose, "fi_bn_fold_batch": _ex_bn_fold}


def recorded_entry(name):
    """Every device entry point that is not the conv replay's, not checked elsewhere and not a host query: an entry the
    step reaches without a handler here shows up unclassified."""
    return name.startswith("fi_") and not classify(name)[:1] == ["conv replay"] and name not in HOST_ONLY and \
        not name.endswith("_workspace_bytes") and name not in CHECKED_ELSEWHERE


# ---- replay helpers ------------------------------------------------------------------------------------------------------
class _Ctx(object):
    def __init__(self, seed, bn):
        self.g = torch.Generator(device=DEV).manual_seed(seed)
        self.bn = bn                          # the recorded model's BatchNorm (gamma, beta) pairs by channel count

    def randn(self, *shape, scale=1.0):
        t = torch.randn(*shape, generator=self.g, device=DEV, dtype=torch.float32)
        return t * scale if scale != 1.0 else t

    def rand(self, *shape):
        return torch.rand(*shape, generator=self.g, device=DEV, dtype=torch.float32)

    def relu_out(self, *shape):
        return torch.relu(self.randn(*shape))                 # exact zeros on half of it

    def perm(self, n):
        return torch.randperm(n, generator=self.g, device=DEV)

    def gamma_beta(self, C):
        """gamma / beta of a BatchNorm of the recorded model with C channels (cycled from the largest if none has C),
        with channel 0 at gamma == 0 and channel 1 at |beta| / |gamma| = 2000."""
        src = self.bn.get(C) or max(self.bn.values(), key=lambda p: p[0].numel())
        idx = torch.arange(C, device=DEV) % src[0].numel()
        ga, be = src[0][idx].clone(), src[1][idx].clone()
        ga[0] = 0.0
        if C > 1:
            ga[1], be[1] = 1e-3, 2.0
        return ga, be


GUARD = 64                              # sentinel floats on either side of every _at / _place buffer (256 bytes: the
SENTINEL = -6.0221e23                   # address modulo 16 is that of `align`)
_GUARDED = []                           # (base, first element of the view, n) since the last _call


def _at(n, align, fill=float("nan")):
    """n floats starting `align` bytes past a 16-byte boundary (a storage offset into a larger buffer), between two
    guard zones of GUARD sentinel floats that _call checks after the launch."""
    assert align % 4 == 0, align
    base = torch.empty(n + 2 * GUARD + 4, device=DEV, dtype=torch.float32)
    lo = GUARD + align // 4
    base[:lo] = SENTINEL
    base[lo + n:] = SENTINEL
    t = base[lo: lo + n]
    assert t.data_ptr() % 16 == align % 16, (t.data_ptr(), align)
    if fill is not None:
        t.fill_(fill)
    _GUARDED.append((base, lo, n))
    return t


def _check_guards(what):
    """Every sentinel around the operands built since the last call is intact (a store before a buffer or past its
    tail lands in one); forgets the buffers."""
    zones, _GUARDED[:] = list(_GUARDED), []
    if not zones:
        return
    hit = torch.stack([(base[:lo] != SENTINEL).any() | (base[lo + n:] != SENTINEL).any() for base, lo, n in zones])
    if bool(hit.any()):
        msgs = []
        for k in torch.nonzero(hit).reshape(-1).tolist():
            base, lo, n = zones[k]
            before = torch.nonzero(base[:lo] != SENTINEL).reshape(-1) - lo
            after = torch.nonzero(base[lo + n:] != SENTINEL).reshape(-1)
            msgs.append("operand %d (%d floats): elements %s before its start, %s past its end overwritten" % (
                k, n, before.tolist()[:8], after.tolist()[:8]))
        raise AssertionError("%s wrote outside its operands: %s" % (what, "; ".join(msgs)))


def _place(src, align):
    t = _at(src.numel(), align, None).view(src.shape)
    t.copy_(src)
    return t


def _random_fill(t, ctx):
    t.copy_(ctx.randn(*t.shape))
    return t


def _call(name, I, P):
    from feature_intertwiner_amd import _lib
    args = []
    for k in SPECS[name][1]:
        if k == "stream":
            args.append(_lib.current_stream())
        elif k not in _PTRS:
            args.append(I[k])
        else:
            v = P.get(k)
            args.append(_lib.ptr(v) if (v is None or torch.is_tensor(v)) else v)
    _lib.check(getattr(_lib.load(), name)(*args), "replay " + name)
    torch.cuda.synchronize()
    _check_guards("%s %s" % (name, I))


def _exact(got, ref, what, nan_equal=False):
    """nan_equal: a NaN where the reference holds a NaN counts as equal (inputs with NaN planted on purpose)."""
    got, ref = got.double(), ref.double()
    bad = ~(got == ref)
    if nan_equal:
        bad &= ~(torch.isnan(got) & torch.isnan(ref))
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError("%s: element %d of %d not bit-exact (got %r, ref %r; %d elements differ)" % (
            what, i, got.numel(), float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]), int(bad.sum())))
    return 0.0


# ---- handlers: (name, ints, nulls, aligns, extra, ctx) -> worst |d| / (2^-24 m) ----------------------------------------
def _h_bn_act(name, I, nul, al, ex, ctx):
    N, C, HW, relu, layout, zeroed = I["N"], I["C"], I["HW"], I["relu"], I["layout"], bool(I["flags"] & 1)
    has_gamma = not nul["gamma"]
    xh = ctx.randn(N, C, HW)
    if has_gamma:
        ga, be = ctx.gamma_beta(C)
        if dict(ex).get("live_gamma"):            # C == 1: the only channel would be the gamma == 0 one
            ga[0] = 0.75
        if nul["beta"]:                           # the kernel then takes beta = 0
            be = torch.zeros_like(be)
        inv = 0.5 + ctx.rand(C)
        scale = ga * inv
    else:                                         # conv + bias + ReLU: unit scale, no BatchNorm
        ga, be, scale = torch.ones(C, device=DEV), torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    res = None if nul["residual"] else ctx.randn(N, C, HW)
    pre = ga.view(1, -1, 1) * xh + be.view(1, -1, 1)
    if res is not None:
        pre = pre + res
    y = torch.relu(pre) if relu else pre
    dy = ctx.randn(N, C, HW)
    if layout == 1:
        dy_s, y_s = dy.permute(0, 2, 1).contiguous(), y.permute(0, 2, 1).contiguous()
    else:
        dy_s, y_s = dy, y
    P = {"dy": _place(dy_s, al.get("dy", 0)), "y": _place(y_s, al.get("y", 0)), "scale": scale,
         "gamma": ga if has_gamma else None, "beta": None if nul["beta"] else be,
         "residual": None if res is None else _place(res, al.get("residual", 0)),
         "dz": _at(N * C * HW, al.get("dz", 0)).view(N, C, HW),
         "g_out": None if nul["g_out"] else _at(N * C * HW, al.get("g_out", 0)).view(N, C, HW)}
    if dict(ex).get("split_sums"):                # three buffers of their own (the step's are slices of one arena)
        parts = [_at(C, al.get(k, 0), None) for k in ("dshift", "dgamma", "dbias")]
        for t in parts:
            _random_fill(t, ctx) if zeroed else t.fill_(float("nan"))
        before = torch.cat(parts)
    else:
        sums = _at(3 * C, al.get("dshift", 0), None)
        if zeroed:
            _random_fill(sums, ctx)
        else:
            sums.fill_(float("nan"))
        before = sums.clone()
        parts = [sums[:C], sums[C:2 * C], sums[2 * C:]]
    P["dshift"] = parts[0]
    P["dgamma"] = None if nul["dgamma"] else parts[1]
    P["dbias"] = None if nul["dbias"] else parts[2]
    _call(name, I, P)
    what = "%s %s" % (name, I)
    g32 = torch.where(y > 0, dy, torch.zeros_like(dy)) if relu else dy
    _exact(P["dz"], g32 * scale.view(1, -1, 1), what + " dz")
    if P["g_out"] is not None:
        _exact(P["g_out"], g32, what + " g_out")
    g, ds, ms, dgam, mg = R.bn_act_bwd_ref(dy, y, xh, ga, be, relu, res)
    n = N * HW
    chk = (lambda got, b, ref, m, w: R.check_increment(got, b, ref, m, n, w)) if zeroed else \
        (lambda got, b, ref, m, w: R.check_bar(got, ref, m, n, w))
    worst = chk(P["dshift"], before[:C], ds, ms, what + " dshift")
    if P["dbias"] is not None:
        sc = scale.double()
        worst = max(worst, chk(P["dbias"], before[2 * C:], ds * sc, ms * sc.abs(), what + " dbias"))
    if P["dgamma"] is not None:
        live = ga != 0
        worst = max(worst, chk(P["dgamma"][live], before[C:2 * C][live], dgam[live], mg[live], what + " dgamma"))
        # the documented behaviour at gamma == 0: nothing is added
        _exact(P["dgamma"][~live], before[C:2 * C][~live] if zeroed else torch.zeros_like(P["dgamma"][~live]),
               what + " dgamma at gamma == 0")
    return worst


def _fold_problem(I, ctx, dw_al, w_al, nul):
    Co, Ci, T = I["Cout"], I["Cin"], I["taps"]
    dwp = ctx.randn(Co, Ci, T)
    w = ctx.randn(Co, Ci, T, scale=1.0 / math.sqrt(Ci * T))
    store = lambda t, tm: (t.permute(0, 2, 1) if tm else t).contiguous()
    s = ctx.randn(Co, scale=8.0)
    ga, _ = ctx.gamma_beta(Co)
    var, mean = 0.1 + ctx.rand(Co), ctx.randn(Co)
    scale = ga * torch.rsqrt(var + I["eps"])
    cb = None if nul.get("conv_bias", True) else ctx.randn(Co)
    dg = None if nul.get("dgamma", True) else _random_fill(torch.empty(Co, device=DEV), ctx)
    db = None if nul.get("dbias", True) else _random_fill(torch.empty(Co, device=DEV), ctx)
    return dict(dwp=dwp, w=w, dw=_place(store(dwp, I["dw_tap_major"]), dw_al), w_s=_place(store(w, I["w_tap_major"]), w_al),
                s=s, scale=scale, mean=mean, var=var, cb=cb, dgamma=dg, dbias=db,
                dg0=None if dg is None else dg.clone(), db0=None if db is None else db.clone())


def _fold_check(name, I, p, what):
    Co, Ci, T = I["Cout"], I["Cin"], I["taps"]
    dwS, dgam, mg, dbias, mb = R.fold_grad_ref(p["dwp"], p["w"], p["s"], p["scale"], p["mean"], p["var"], I["eps"], p["cb"])
    got = p["dw"].view(Co, T, Ci).permute(0, 2, 1) if I["dw_tap_major"] else p["dw"].view(Co, Ci, T)
    _exact(got, p["dwp"] * p["scale"].view(-1, 1, 1), what + " dW")
    worst = 0.0
    if p["dgamma"] is not None:
        worst = R.check_increment(p["dgamma"], p["dg0"], dgam, mg, Ci * T, what + " dgamma")
    if p["dbias"] is not None:
        worst = max(worst, R.check_increment(p["dbias"], p["db0"], dbias, mb, 1, what + " dbias"))
    return worst


def _h_fold(name, I, nul, al, ex, ctx):
    p = _fold_problem(I, ctx, al.get("dw", 0), al.get("w", 0), nul)
    _call(name, I, {"dw": p["dw"], "w": p["w_s"], "s": p["s"], "scale": p["scale"], "mean": p["mean"], "var": p["var"],
                    "conv_bias": p["cb"], "dgamma": p["dgamma"], "dbias": p["dbias"]})
    return _fold_check(name, I, p, "%s %s %s" % (name, I, al))


def _h_fold_batch(name, I, nul, al, ex, ctx):
    ex = dict(ex)
    n = I["n"]
    probs = []
    for j in range(n):
        pick = lambda key: ex[key] is not None and ex[key][j]
        probs.append(_fold_problem(I, ctx, ex["dws"][j], ex["ws"][j],
                                   {"conv_bias": not pick("cbs"), "dgamma": not pick("dgammas"), "dbias": not pick("dbiases")}))
    arr = lambda key, lst: None if ex.get(key, 0) is None else (ctypes.c_void_p * n)(*[0 if t is None else t.data_ptr()
                                                                                        for t in lst])
    col = lambda k: (ctypes.c_void_p * n)(*[probs[j][k].data_ptr() for j in range(n)])
    P = {"dws": col("dw"), "ws": col("w_s"), "ss": col("s"), "scales": col("scale"), "means": col("mean"),
         "vars": col("var"), "cbs": arr("cbs", [p["cb"] for p in probs]),
         "dgammas": arr("dgammas", [p["dgamma"] for p in probs]), "dbiases": arr("dbiases", [p["dbias"] for p in probs])}
    _call(name, I, P)
    return max(_fold_check(name, I, p, "%s %s [%d/%d]" % (name, I, j, n)) for j, p in enumerate(probs))


def _h_rows_mask(name, I, nul, al, ex, ctx):
    M, N, ld, relu, zeroed = I["M"], I["N"], I["ld_out"], I["relu"], bool(I["flags"] & 1)
    dy = _place(ctx.randn(M, N), al.get("dy", 0))
    y = None if nul["y"] else _place(ctx.relu_out(M, N), al.get("y", 0))
    scale = None if nul["scale"] else ctx.randn(N)
    SENT = 12345.0                                          # padding columns of the zero-padded operands stay put
    g = None if nul["g"] else _at(M * ld, al.get("g", 0), SENT).view(M, ld)
    gs = None if nul["gs"] else _at(M * ld, al.get("gs", 0), SENT).view(M, ld)
    if g is not None:
        g[:, :N] = float("nan")
    if gs is not None:
        gs[:, :N] = float("nan")
    colsum = None if nul["colsum"] else _at(N, al.get("colsum", 0), None)
    if colsum is not None:
        _random_fill(colsum, ctx) if zeroed else colsum.fill_(float("nan"))
    c0 = None if colsum is None else colsum.clone()
    _call(name, I, {"dy": dy, "y": y, "scale": scale, "g": g, "gs": gs, "colsum": colsum})
    what = "%s %s" % (name, I)
    g32 = torch.where(y > 0, dy, torch.zeros_like(dy)) if relu else dy
    for out, ref in ((g, g32), (gs, g32 * (scale if scale is not None else 1.0))):
        if out is not None:
            _exact(out[:, :N], ref, what + " rows")
            if ld > N:
                _exact(out[:, N:], torch.full_like(out[:, N:], SENT), what + " padding columns")
    if colsum is None:
        return 0.0
    _, cs, mc = R.rows_mask_scale_ref(dy, y if y is not None else dy, relu)
    return R.check_increment(colsum, c0, cs, mc, M, what + " colsum") if zeroed else \
        R.check_bar(colsum, cs, mc, M, what + " colsum")


def _h_rows_affine(name, I, nul, al, ex, ctx):
    M, N, relu = I["M"], I["N"], I["relu"]
    y0 = ctx.randn(M, N, scale=4.0)
    y = _place(y0, al.get("y", 0))
    sc = None if nul["scale"] else ctx.randn(N)
    b = None if nul["bias"] else ctx.randn(N)
    _call(name, I, {"y": y, "scale": sc, "bias": b})
    ref = y0.double() * (sc.double() if sc is not None else 1.0) + (b.double() if b is not None else 0.0)
    m = (y0.double() * (sc.double() if sc is not None else 1.0)).abs() + (b.double().abs() if b is not None else 0.0)
    if relu:
        ref = ref.clamp_min(0.0)
    d = (y.double() - ref).abs()
    lim = 2.0 * R.U * m                                      # one rounding of the product, one of the sum (or one fused)
    assert bool(torch.isfinite(y).all()) and bool((d <= lim).all()), "%s %s: %.3g ulp" % (
        name, I, float((d / (R.U * m).clamp_min(1e-300)).max()))
    return float((d / (R.U * m).clamp_min(1e-300)).max())


def _class_rows(N, K, ctx):
    """Several rows per class, 3/4 of the rows all-zero later; classes drawn from a few (thousands of rows share one)."""
    few = ctx.perm(K)[:max(1, min(K, 6))]
    return few[torch.randint(0, few.numel(), (N,), generator=ctx.g, device=DEV)].to(torch.int64)


def _h_class_row(name, I, nul, al, ex, ctx):
    from feature_intertwiner_amd import _lib
    N, C, HW, K, gated = I["N"], I["C"], I["HW"], I["num_classes"], I["gated"]
    opt = dict(ex)        # dead: fraction of all-zero rows; dead_rows: leading rows forced dead; unused_class: no row has it
    frac, lead, unused = opt.get("dead", 0.75), opt.get("dead_rows", 0), opt.get("unused_class")
    d = ctx.randn(N, HW)
    dead = ctx.rand(N) < frac
    d[dead] = 0.0
    if N > 2 and frac < 1.0 and lead <= 2:
        d[2] = 0.0
        d[2, HW // 2] = 1.5                                  # one row with a single non-zero
    d[:lead] = 0.0
    x = ctx.relu_out(N, C, HW)
    w = ctx.randn(K, C)
    cls = _class_rows(N, K, ctx)
    if unused is not None:
        cls[cls == unused] = (unused + 1) % K
    dx = None if nul["dx"] else _at(N * C * HW, al.get("dx", 0)).view(N, C, HW)
    dwt = None if nul["dweight"] else _random_fill(torch.empty(K, C, device=DEV), ctx)
    dbt = None if nul["dbias"] else _random_fill(torch.empty(K, device=DEV), ctx)
    w0, b0 = (None if dwt is None else dwt.clone()), (None if dbt is None else dbt.clone())
    ws = torch.empty(int(_lib.load().fi_class_row_conv1x1_workspace_bytes(N, C)) // 4 + 4, device=DEV)
    _call(name, I, {"d": _place(d, al.get("d", 0)), "x": _place(x, al.get("x", 0)), "weight": w, "cls": cls, "dx": dx,
                    "dweight": dwt, "dbias": dbt, "workspace": ws})
    what = "%s %s" % (name, I)
    rdx, rdw, mw, rdb, mb, nk = R.class_row_bwd_ref(d, x, w, cls, K, gated)
    worst = 0.0
    if dx is not None:
        ref32 = w[cls][:, :, None] * d[:, None, :]
        if gated:
            ref32 = torch.where(x > 0, ref32, torch.zeros_like(ref32))
        _exact(dx, ref32, what + " dx")
    if dwt is not None:
        worst = R.check_increment(dwt, w0, rdw, mw, nk[:, None].expand_as(rdw), what + " dweight")
    if dbt is not None:
        worst = max(worst, R.check_increment(dbt, b0, rdb, mb, nk, what + " dbias"))
    if unused is not None:                                   # nothing is added to the rows of a class without rows
        if dwt is not None:
            _exact(dwt[unused], w0[unused], what + " dweight of the unused class")
        if dbt is not None:
            _exact(dbt[unused], b0[unused], what + " dbias of the unused class")
    return worst


def _patch_operands(I, ex, ctx):
    """ex beyond the level sizes: B (images, 2), pad (fraction of padding rows, 0.1), dup (the last `dup` rows repeat row
    0's image and anchor, 0)."""
    ex = dict(ex)
    hs, ws = ex["heights"], ex["widths"]
    B, pad, dup = ex.get("B", 2), ex.get("pad", 0.1), ex.get("dup", 0)
    per, rows, C = I["per_loc"], I["rows"], I["channels"]
    counts = [h * w * per for h, w in zip(hs, ws)]
    total = sum(counts)
    anchor = torch.randint(0, total, (rows,), generator=ctx.g, device=DEV)
    starts = np.cumsum([0] + counts[:-1]).tolist()
    special = []
    for l, (s0, h, w) in enumerate(zip(starts, hs, ws)):
        special += [s0, s0 + per * (w - 1), s0 + per * (h - 1) * w, s0 + counts[l] - 1]   # level start, map corners
    k = min(len(special), rows)
    anchor[:k] = torch.tensor(special[:k], device=DEV)
    image = torch.randint(0, B, (rows,), generator=ctx.g, device=DEV)
    image[ctx.rand(rows) < pad] = -1                         # padding rows
    if dup:
        image[0] = B - 1
        image[rows - dup:] = image[0]
        anchor[rows - dup:] = anchor[0]
    shapes = [(B, C, h, w) for h, w in zip(hs, ws)]
    return shapes, image.to(torch.int64), anchor.to(torch.int64)


def _h_patch_fwd(name, I, nul, al, ex, ctx):
    shapes, image, anchor = _patch_operands(I, ex, ctx)
    maps = [ctx.randn(*s) for s in shapes]
    n = len(maps)
    out = _at(I["rows"] * 9 * I["channels"], al.get("out", 0)).view(I["rows"], 9, I["channels"])
    hs, ws = (ctypes.c_int * n)(*[s[2] for s in shapes]), (ctypes.c_int * n)(*[s[3] for s in shapes])
    _call(name, I, {"maps": (ctypes.c_void_p * n)(*[m.data_ptr() for m in maps]), "heights": hs, "widths": ws,
                    "image": image, "anchor": anchor, "out": out})
    return _exact(out, R.patch_rows_ref(maps, image, anchor, I["per_loc"]), "%s %s" % (name, I))


def _h_patch_bwd(name, I, nul, al, ex, ctx):
    shapes, image, anchor = _patch_operands(I, ex, ctx)
    n = len(shapes)
    d = _place(ctx.randn(I["rows"], 9, I["channels"]), al.get("d", 0))
    grads = [ctx.randn(*s) for s in shapes]
    before = [g.clone() for g in grads]
    hs, ws = (ctypes.c_int * n)(*[s[2] for s in shapes]), (ctypes.c_int * n)(*[s[3] for s in shapes])
    _call(name, I, {"d": d, "grads": (ctypes.c_void_p * n)(*[g.data_ptr() for g in grads]), "heights": hs, "widths": ws,
                    "image": image, "anchor": anchor})
    refs, mags, cnts = R.patch_rows_bwd_ref(d, shapes, image, anchor, I["per_loc"])
    return max(R.check_increment(g, b, r, m, c, "%s %s level %d" % (name, I, l))
               for l, (g, b, r, m, c) in enumerate(zip(grads, before, refs, mags, cnts)))


def _h_rows_gather(name, I, nul, al, ex, ctx):
    n, L = I["n_index"], I["row_len"]
    src = ctx.randn(n + 7, L)
    idx = ctx.perm(n + 7)[:n].contiguous()
    dst = _at(n * L, al.get("dst", 0)).view(n, L)
    _call(name, I, {"src": _place(src, al.get("src", 0)), "index": idx, "dst": dst})
    return _exact(dst, src[idx], "%s %s" % (name, I))


def _h_rows_scatter(name, I, nul, al, ex, ctx):
    n, L = I["n_index"], I["row_len"]
    src = ctx.randn(n, L)
    idx = ctx.perm(n + 7)[:n].contiguous()
    dst = _place(ctx.randn(n + 7, L), al.get("dst", 0))
    ref = dst.clone()
    ref[idx] += src                                          # distinct indices: one fp32 add per element
    _call(name, I, {"src": _place(src, al.get("src", 0)), "index": idx, "dst": dst})
    return _exact(dst, ref, "%s %s" % (name, I))


def _h_rows_combine(name, I, nul, al, ex, ctx):
    rows, nf, L = I["rows"], I["n_front"], I["row_len"]
    front = None if nul["front"] else _place(ctx.randn(max(nf, 1), L)[:nf], al.get("front", 0))
    S = rows + 3
    src = ctx.randn(S, L)
    src_row = ctx.perm(S)[:rows].clone()
    src_row[ctx.rand(rows) < dict(ex).get("neg", 0.3)] = -1      # neg: the fraction of rows nothing is gathered into
    dst = _at(rows * L, al.get("dst", 0)).view(rows, L)
    _call(name, I, {"front": front, "src": _place(src, al.get("src", 0)), "src_row": src_row, "dst": dst})
    ref = torch.where((src_row >= 0)[:, None], src[src_row.clamp_min(0)], torch.zeros(rows, L, device=DEV))
    if nf:
        ref[:nf] = front + ref[:nf]
    return _exact(dst, ref, "%s %s" % (name, I))


def _pool_input(P, H, W, ctx, ex=()):
    """A ReLU output with ties, as the stem's; ex `signed`: values of both signs with ties and plane 0 all negative (no
    window of it holds a zero or a positive); ex `nan`: that many NaN at random places."""
    opt = dict(ex)
    if opt.get("signed"):
        x = ctx.randn(P, H, W)
        x[:, ::3] = torch.round(x[:, ::3] * 2) * 0.5
        x[0] = -x[0].abs() - 0.5
    else:
        x = ctx.relu_out(P, H, W)
        x[:, ::3] = torch.relu(torch.round(x[:, ::3] * 2) * 0.5)        # ties
    if opt.get("nan"):
        x.view(-1)[ctx.perm(x.numel())[:opt["nan"]]] = float("nan")
    return x


def _h_pool_fwd(name, I, nul, al, ex, ctx):
    P, H, W = I["planes"], I["height"], I["width"]
    x = _place(_pool_input(P, H, W, ctx, ex), al.get("x", 0))
    ref = torch.nn.functional.max_pool2d(x.view(1, P, H, W), 3, 2, 0, ceil_mode=True)[0]
    y = _at(ref.numel(), al.get("y", 0)).view(ref.shape)
    _call(name, I, {"x": x, "y": y})
    return _exact(y, ref, "%s %s" % (name, I), nan_equal=bool(dict(ex).get("nan")))


def _h_pool_bwd(name, I, nul, al, ex, ctx):
    P, H, W = I["planes"], I["height"], I["width"]
    x = _place(_pool_input(P, H, W, ctx, ex), al.get("x", 0))
    xr = x.detach().clone().view(1, P, H, W).requires_grad_(True)
    yr = torch.nn.functional.max_pool2d(xr, 3, 2, 0, ceil_mode=True)
    dy = ctx.randn(*yr.shape)
    yr.backward(dy)
    ref = xr.grad[0] * (x > 0) if I["positive_only"] else xr.grad[0]
    dx = _at(P * H * W, al.get("dx", 0)).view(P, H, W)
    _call(name, I, {"dy": _place(dy[0], al.get("dy", 0)), "x": x, "dx": dx})
    return _exact(dx, ref, "%s %s" % (name, I))


def _h_sum2x2(name, I, nul, al, ex, ctx):
    P, H, W = I["planes"], I["height"], I["width"]
    xr = torch.zeros(1, P, H, W, device=DEV, requires_grad=True)
    up = torch.nn.functional.interpolate(xr, scale_factor=2, mode="nearest")
    dy = ctx.randn(*up.shape)
    up.backward(dy)
    out = _at(P * H * W, al.get("out", 0)).view(P, H, W)
    _call(name, I, {"dy": _place(dy[0], al.get("dy", 0)), "out": out})
    return _exact(out, xr.grad[0], "%s %s" % (name, I))


def _h_relu_mask(name, I, nul, al, ex, ctx):
    n = I["n"]
    dy = _place(ctx.randn(n), al.get("dy", 0))
    y = _place(ctx.relu_out(n), al.get("y", 0))
    ref = torch.where(y > 0, dy, torch.zeros_like(dy))
    out = dy if dict(ex)["aliased"] else _at(n, al.get("out", 0))
    _call(name, I, {"dy": dy, "y": y, "out": out})
    return _exact(out, ref, "%s %s aliased=%s" % (name, I, dict(ex)["aliased"]))


def _h_interleave(name, I, nul, al, ex, ctx):
    P, H, W = I["planes"], I["height"], I["width"]
    ref = torch.zeros(P, H, W, device=DEV)
    Pm = {}
    for a in (0, 1):
        for b in (0, 1):
            k = "c%d%d" % (a, b)
            if nul[k]:
                continue
            c = ctx.randn(P, (H - a + 1) // 2, (W - b + 1) // 2)
            Pm[k] = _place(c, al.get(k, 0))
            ref[:, a::2, b::2] = c
    add = None if nul["add"] else _place(ctx.randn(P, H, W), al.get("add", 0))
    if add is not None:
        ref = ref + add
    gate = None if nul.get("gate", True) else _place(ctx.relu_out(P, H, W), al.get("gate", 0))
    if gate is not None:
        ref = torch.where(gate > 0, ref, torch.zeros_like(ref))
    dx = _at(P * H * W, al.get("dx", 0)).view(P, H, W)
    Pm.update(add=add, gate=gate, dx=dx)
    _call(name, I, Pm)
    return _exact(dx, ref, "%s %s %s" % (name, I, al))


def _frag_index(M, K):
    """Position of D[m][k] in the fragment-major layout of include/fi_capi.h (FiTransposeDesc flag 1)."""
    m = torch.arange(M, device=DEV)[:, None]
    k = torch.arange(K, device=DEV)[None, :]
    return ((m >> 5) * (K >> 4) + (k >> 4)) * 512 + ((k & 7) >> 2) * 256 + (((k & 15) >> 3) * 32 + (m & 31)) * 4 + (k & 3)


def _h_transpose(name, I, nul, al, ex, ctx):
    from feature_intertwiner_amd import _lib
    from feature_intertwiner_amd.conv import _TR_DESC
    desc = np.zeros(len(ex), dtype=_TR_DESC)
    probs, base = [], 0
    for i, (rows, cols, taps, flags, has_rs) in enumerate(ex):
        src = ctx.randn(rows, taps, cols)
        rs = ctx.randn(rows) if has_rs else None
        dst = _at(rows * taps * cols, 0)
        desc[i] = (src.data_ptr(), dst.data_ptr(), rows, cols, taps, flags, base, 0 if rs is None else rs.data_ptr())
        base += taps * ((rows + 31) // 32) * ((cols + 31) // 32)
        probs.append((rows, cols, taps, flags, src, rs, dst))
    assert base == I["total_tiles"], (base, I["total_tiles"])
    table = torch.from_numpy(desc.view(np.uint8).copy()).to(DEV)
    _call(name, I, {"table": table})
    for i, (rows, cols, taps, flags, src, rs, dst) in enumerate(probs):
        what = "%s descriptor %d %s" % (name, i, (rows, cols, taps, flags, rs is not None))
        if flags & 1:
            D = src[:, 0, :] if flags & 2 else (src[:, 0, :] * (rs[:, None] if rs is not None else 1.0)).t()
            ref = torch.empty_like(dst)
            ref[_frag_index(*D.shape).reshape(-1)] = D.reshape(-1)
            _exact(dst, ref, what)
        else:
            ref = src * rs[:, None, None] if rs is not None else src
            _exact(dst.view(cols, taps, rows), ref.permute(2, 1, 0), what)
    return 0.0


def _h_bn_fold(name, I, nul, al, ex, ctx):
    desc = np.zeros(len(ex), dtype=_BN_DESC)
    probs = []
    for i, (ch, eps, has_cb) in enumerate(ex):
        ga, be = ctx.gamma_beta(ch)
        mean, var = ctx.randn(ch), 0.01 + ctx.rand(ch) * 4
        cb = ctx.randn(ch) if has_cb else None
        sc, sh = _at(ch, 0), _at(ch, 0)
        desc[i] = (ga.data_ptr(), be.data_ptr(), mean.data_ptr(), var.data_ptr(), 0 if cb is None else cb.data_ptr(),
                   sc.data_ptr(), sh.data_ptr(), ch, eps)
        probs.append((ga, be, mean, var, cb, sc, sh, eps))
    table = torch.from_numpy(desc.view(np.uint8).copy()).to(DEV)
    _call(name, I, {"table": table})
    worst = 0.0
    for i, (ga, be, mean, var, cb, sc, sh, eps) in enumerate(probs):
        # bound: rsqrtf within 2 ulp, then products / sums each rounded once -> 4 ulp of scale, 8 ulp of the shift's m
        eps32 = float(np.float32(eps))
        rsc = ga.double() / torch.sqrt(var.double() + eps32)
        rsh = be.double() - mean.double() * rsc + (cb.double() * rsc if cb is not None else 0.0)
        msh = be.double().abs() + (mean.double() * rsc).abs() + ((cb.double() * rsc).abs() if cb is not None else 0.0)
        for got, ref, m, k, w in ((sc, rsc, rsc.abs(), 4.0, "scale"), (sh, rsh, msh, 8.0, "shift")):
            d = (got.double() - ref).abs()
            r = d / (R.U * m).clamp_min(1e-300)
            assert bool(torch.isfinite(got).all()) and bool((d <= k * R.U * m).all()), \
                "%s descriptor %d %s: %.3g ulp" % (name, i, w, float(r.max()))
            worst = max(worst, float(r.max()))
    return worst


def _h_gather_props(name, I, nul, al, ex, ctx):
    B, pre, st, ks, cnt = I["batch"], I["pre_nms"], I["det_stride"], I["keep_stride"], I["proposal_count"]
    dets = ctx.rand(B, pre, st) * 1000.0
    keep = torch.stack([ctx.perm(pre)[:ks] for _ in range(B)]).to(torch.int64) if ks <= pre else \
        torch.randint(0, pre, (B, ks), generator=ctx.g, device=DEV)
    num = torch.randint(0, min(ks, cnt) + 1, (B,), generator=ctx.g, device=DEV).to(torch.int32)
    num[0] = min(ks, cnt)
    opt = dict(ex)        # num: the counts (0, or more than keep_stride); bad_keep: entries -1 and pre_nms in image 0's list
    if opt.get("num") is not None:
        num = torch.tensor(opt["num"], device=DEV, dtype=torch.int32)
    if opt.get("bad_keep"):
        keep[0, 0], keep[0, ks - 1] = -1, pre
    out = _at(B * cnt * 4, al.get("proposals", 0)).view(B, cnt, 4)
    _call(name, I, {"dets": dets, "keep": keep, "num": num, "proposals": out})
    nrm = torch.tensor([I["norm_h"], I["norm_w"], I["norm_h"], I["norm_w"]], device=DEV, dtype=torch.float32)
    ref = torch.zeros(B, cnt, 4, device=DEV)
    for b in range(B):
        k = min(int(num[b]), ks, cnt)                        # a count past the list or the output reads neither
        kk = keep[b, :k]
        ok = (kk >= 0) & (kk < pre)                          # an entry that is no row of dets gives a row of zeros
        ref[b, :k] = torch.where(ok[:, None], dets[b, kk.clamp(0, pre - 1), :4] / nrm, torch.zeros(k, 4, device=DEV))
    return _exact(out, ref, "%s %s" % (name, I))


HANDLERS = {"bn_act": _h_bn_act, "fold": _h_fold, "fold_batch": _h_fold_batch, "rows_mask": _h_rows_mask,
            "rows_affine": _h_rows_affine, "class_row": _h_class_row, "patch_fwd": _h_patch_fwd,
            "patch_bwd": _h_patch_bwd, "rows_gather": _h_rows_gather, "rows_scatter": _h_rows_scatter,
            "rows_combine": _h_rows_combine, "pool_fwd": _h_pool_fwd, "pool_bwd": _h_pool_bwd, "sum2x2": _h_sum2x2,
            "relu_mask": _h_relu_mask, "interleave": _h_interleave, "transpose": _h_transpose, "bn_fold": _h_bn_fold,
            "gather_props": _h_gather_props}


# ---- clip + SGD, in-step --------------------------------------------------------------------------------------------------
class _SgdCheck(object):
    """Wraps optim.clip_and_step for the steps of one workload: snapshots parameters, gradients and momentum buffers,
    lets the kernel run, and checks the norm, the clip factor and every updated element against fp64.  The calls whose
    index is in `guard_calls` take the guarded form (skip_nonfinite=True, fi_sgd_clip_step_guarded) whatever the step
    asked for: with finite gradients every check applies to it as well."""

    def __init__(self, opt, guard_calls=()):
        self.opt, self.calls, self.worst, self.fail = opt, 0, 0.0, []
        self.guard_calls, self.guarded_applied = set(guard_calls), 0

    def __enter__(self):
        from feature_intertwiner_amd import optim
        self.optim, self.real = optim, optim.clip_and_step
        optim.clip_and_step = self.wrapped
        return self

    def __exit__(self, *a):
        self.optim.clip_and_step = self.real

    def wrapped(self, optimizer, max_norm, skip_nonfinite=False):
        if self.calls in self.guard_calls:
            skip_nonfinite = True
        snap = []
        for grp in optimizer.param_groups:
            for p in grp["params"]:
                if p.grad is None:
                    continue
                buf = optimizer.state[p].get("momentum_buffer") if grp["momentum"] else None
                snap.append((p, p.detach().clone(), p.grad.detach().clone(), None if buf is None else buf.clone(),
                             float(grp["weight_decay"]), float(grp["momentum"]), float(grp["lr"])))
        torch.cuda.synchronize()
        out = self.real(optimizer, max_norm, skip_nonfinite=skip_nonfinite)
        torch.cuda.synchronize()
        try:
            self.check(optimizer, max_norm, skip_nonfinite, snap)
        except AssertionError as e:
            self.fail.append(str(e)[:600])
        self.calls += 1
        return out

    def check(self, optimizer, max_norm, guarded, snap):
        c = self.optim._CACHE[optimizer]
        norm_got, coef_got = float(c["out"][0]), float(c["out"][1])
        ref_norm, n = R.grad_norm_ref([s[2] for s in snap])
        what = "clip_and_step (guarded=%s, %d tensors, %d elements)" % (guarded, len(snap), n)
        w = R.check_bar(torch.tensor([norm_got]), torch.tensor([ref_norm], dtype=torch.float64),
                        torch.tensor([ref_norm], dtype=torch.float64), n, what + " norm")
        self.worst = max(self.worst, w)
        if guarded and float(c["out"][2]) != 0.0:
            # a skipped step leaves parameters, gradients and momentum buffers as they were (a buffer the call created
            # for the first step stays zero)
            for i, (p, p0, g0, b0, wd, mom, lr) in enumerate(snap):
                _exact(p.detach(), p0, "%s skipped step: parameter %d" % (what, i))
                _exact(p.grad, g0, "%s skipped step: gradient %d" % (what, i))
                buf = optimizer.state[p].get("momentum_buffer") if mom else None
                if buf is not None:
                    _exact(buf, b0 if b0 is not None else torch.zeros_like(buf),
                           "%s skipped step: momentum buffer %d" % (what, i))
            return
        if guarded:
            self.guarded_applied += 1
        if max_norm:
            mn = np.float32(max_norm)
            expect = min(np.float32(1.0), np.float32(mn / (np.float32(norm_got) + np.float32(1e-6))))
            assert coef_got == float(expect), (what, coef_got, float(expect))
            cref = R.clip_coef_ref(ref_norm, max_norm)
            assert abs(coef_got - cref) <= cref * R.U * (4 * math.sqrt(n) + 20), (what, coef_got, cref)
        else:
            assert coef_got == 1.0, (what, coef_got)
        for i, (p, p0, g0, b0, wd, mom, lr) in enumerate(snap):
            buf = optimizer.state[p].get("momentum_buffer") if mom else None
            rp, rb, rg, mp, mb, mg = R.sgd_ref(p0, g0, b0 if b0 is not None else (torch.zeros_like(p0) if mom else None),
                                               coef_got, wd, mom, lr)
            # at most 5 fp32 roundings per element (scale, weight decay, momentum, step): 8 ulp of the m each, plus
            # 4 x 2^-126 for intermediates below the normal range that the device may flush to zero (parameters and
            # gradients near 1e-36 occur in-step)
            for got, ref, m, k in ((p.detach(), rp, mp, "param"), (buf, rb, mb, "momentum buffer")):
                if got is None:
                    continue
                d = (got.double() - ref).abs()
                ok = bool((d <= 8.0 * R.U * m + 4.0 * TINY).all()) and bool(torch.isfinite(got).all())
                r = float((d / (R.U * m + TINY).clamp_min(1e-300)).max())
                if not ok:
                    j = int(torch.argmax(d / (R.U * m).clamp_min(1e-300)))
                    others = [q for q, *_ in snap if q is not p and q.grad is not None and
                              q.grad.untyped_storage().data_ptr() == p.grad.untyped_storage().data_ptr()]
                    raise AssertionError("%s tensor %d %s %s: %.3g ulp at %d (got %r ref %r p0 %r g0 %r b0 %r coef %r "
                                         "wd %r mom %r lr %r; %d other gradients share its storage)" % (
                                             what, i, tuple(p.shape), k, r, j, float(got.reshape(-1)[j]),
                                             float(ref.reshape(-1)[j]), float(p0.reshape(-1)[j]),
                                             float(g0.reshape(-1)[j]),
                                             None if b0 is None else float(b0.reshape(-1)[j]), coef_got, wd, mom, lr,
                                             len(others)))
                self.worst = max(self.worst, r)
            _exact(p.grad, (g0 * coef_got) if coef_got != 1.0 else g0, "%s tensor %d gradient" % (what, i))


# ---- workloads ---------------------------------------------------------------------------------------------------------
def _bn_params(model):
    out = {}
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d) and m.affine:
            out.setdefault(m.num_features, (m.weight.detach().float().clone(), m.bias.detach().float().clone()))
    return out


def _conditioning(model):
    """Worst |beta| / |gamma| over the recorded model's BatchNorm channels, and the number of gamma == 0 channels."""
    worst, zeros = 0.0, 0
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d) and m.affine:
            ga, be = m.weight.detach().double(), m.bias.detach().double()
            zeros += int((ga == 0).sum())
            nz = ga != 0
            if bool(nz.any()):
                worst = max(worst, float((be[nz].abs() / ga[nz].abs()).max()))
    return worst, zeros


def replay(records, label, model):
    t0 = time.time()
    bn = _bn_params(model)
    count = collections.Counter()
    worst = collections.defaultdict(float)
    failures = []
    for i, (name, ints, nulls, aligns, ex) in enumerate(records):
        fam = SPECS[name][0]
        count[name] += 1
        if fam == "sgd":
            continue                                          # checked in-step (_SgdCheck)
        I, nul, al = dict(ints), dict(nulls), dict(aligns)
        try:
            w = HANDLERS[fam](name, I, nul, al, ex, _Ctx(3000 + i, bn))
            worst[name] = max(worst[name], w)
        except AssertionError as e:
            failures.append(str(e)[:600])
    torch.cuda.empty_cache()
    print("\n[%s] %d distinct records replayed in %.1f s" % (label, sum(count.values()), time.time() - t0))
    for name in sorted(count):
        print("  %-40s records %4d   worst |d|/(2^-24 m) %8.2f" % (name, count[name], worst[name]))
    return count, failures


WORKLOADS = [
    ("configs[2] fp32", dict(backbone="resnet101", image_size=1024, batch_size=4, train_rois_per_image=512,
                             dev_switch=True, loss_choice="ot", ot_L=50), 1024, 4),
    ("configs[4] slice bf16", dict(backbone="resnet101", image_size=1344, batch_size=2, train_rois_per_image=1000,
                                   dev_switch=True, loss_choice="ot", ot_L=50, conv_precision="bf16"), 1344, 2),
    ("configs[0] DEV.SWITCH off", dict(backbone="resnet50", image_size=512, batch_size=2, train_rois_per_image=64,
                                       dev_switch=False), 512, 2),
]
# bf16 trains without a loss scale, so its steps call the plain fi_sgd_clip_step; the second step of the configs[4] slice
# is made to take the guarded form (the fp16 path's), which is then checked at full size like the plain one
GUARD_CALLS = {"configs[4] slice bf16": (1,)}
# entries each workload must reach (from the first recordings): a refactor must not make the test pass vacuously
REQUIRED = {
    "configs[2] fp32": {"fi_bn_fold_grad", "fi_bn_fold_grad_batch", "fi_class_row_conv1x1_backward",
                        "fi_pyramid_patch_rows_forward", "fi_pyramid_patch_rows_backward", "fi_maxpool3x3s2_forward",
                        "fi_maxpool3x3s2_backward", "fi_sum2x2", "fi_stride2_interleave_gated", "fi_sgd_clip_step"},
    "configs[4] slice bf16": {"fi_bn_act_backward", "fi_rows_affine_act", "fi_sgd_clip_step", "fi_sgd_clip_step_guarded"},
    "configs[0] DEV.SWITCH off": {"fi_sgd_clip_step"},
}


@pytest.mark.gpu
@pytest.mark.parametrize("label,kw,size,bs", WORKLOADS, ids=["configs2_fp32", "configs4_bf16", "configs0"])
def test_step_glue_launches_match_fp64_elementwise(label, kw, size, bs):
    t0 = time.time()
    box = {}

    def around(model, opt):
        box["sgd"] = _SgdCheck(opt, GUARD_CALLS.get(label, ()))
        return box["sgd"]
    records, model = step_record.record_step(kw, size, bs, recorded_entry, SPECS, _PTRS, align=True, extra=EXTRA,
                                             around=around)
    t_rec = time.time() - t0
    cond, zeros = _conditioning(model)
    sgd = box["sgd"]
    unclassified = sorted({r[0] for r in records if r[0] not in SPECS})
    count, failures = replay([r for r in records if r[0] in SPECS], label, model)
    print("  %-40s calls %5d   worst |d|/(2^-24 m) %8.2f" % ("clip_and_step (in-step)", sgd.calls, sgd.worst))
    print("[%s] worst |beta|/|gamma| of the model %.3g, gamma == 0 channels %d; wall time %.1f s (recording %.1f s)" % (
        label, cond, zeros, time.time() - t0, t_rec))
    del model
    torch.cuda.empty_cache()
    assert not unclassified, "recorded entry points without a handler or classification: %s" % unclassified
    assert not failures, "%d of %d records off:\n%s" % (len(failures), sum(count.values()), "\n".join(failures[:20]))
    assert not sgd.fail, sgd.fail
    assert sgd.calls == 2, sgd.calls
    assert sgd.guarded_applied == len(GUARD_CALLS.get(label, ())), "guarded steps checked: %d" % sgd.guarded_applied
    missing = sorted(REQUIRED[label] - set(count))
    assert not missing, "entries the workload no longer reaches: %s (seen: %s)" % (missing, sorted(count))
