"""CPU: the C-ABI library builds for gfx950, loads, and exports exactly the symbols that
include/fi_capi.h declares; the Python mirror keeps the reference's names and call
shapes; the product path has no CPU fallback.  No kernel is launched here."""
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "fi_capi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fi_[a-z0-9_]+)\s*\(", src)))


def test_library_builds_and_exports_every_declared_symbol():
    from feature_intertwiner_amd import build
    path = build.build_hip()
    assert os.path.exists(path)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    exported = set(re.findall(r" T (fi_[a-z0-9_]+)", nm))
    declared = _declared()
    assert len(declared) >= 18
    assert set(declared) <= exported, sorted(set(declared) - exported)
    # nothing but the declared API (and no torch types) leaks out with the fi_ prefix
    assert exported <= set(declared), sorted(exported - set(declared))
    # device code for gfx950 is embedded
    assert b"gfx950" in open(path, "rb").read()


def test_ctypes_binding_covers_the_header_and_loads():
    from feature_intertwiner_amd import _lib
    assert sorted(_lib.SIGNATURES.keys()) == _declared()
    L = _lib.load()
    assert L.fi_version().startswith(b"fi_hip")
    assert L.fi_nms_workspace_bytes(4, 6000) == 4 * 6000 * 94 * 8
    assert L.fi_nms_workspace_bytes(1, 64) == 64 * 8
    assert L.fi_prof_kernel_name(0) == b"crop_fwd_flat_kernel<7, 7, 8>" and L.fi_prof_kernel_name(45) == b"gemm_slab_reduce_kernel"


def test_argument_validation_without_a_gpu():
    """Invalid sizes are rejected on the host before any HIP call."""
    from feature_intertwiner_amd import _lib
    L = _lib.load()
    assert L.fi_crop_and_resize_forward(None, None, None, 1, 1, 1, 8, 8, 0, 7, 0.0, None, None, None) == -1
    assert b"crop size" in L.fi_last_error()
    assert L.fi_crop_and_resize_forward(None, None, None, 1, 1, 1, 8, 8, 65, 7, 0.0, None, None, None) == -3
    assert L.fi_sinkhorn_forward(None, None, 1, 300, 1, 1.0, 5, 0, None, None, None, None, None) == -3
    assert L.fi_sinkhorn_forward(None, None, 1, 16, 1, 1.0, 0, 0, None, None, None, None, None) == -1
    assert L.fi_nms_sorted(None, 1, 10, 3, 0.5, 0, 0, None, None, None, None) == -1
    assert L.fi_roi_pool_forward(None, None, 1, 1, 1, 4, 4, 0, 7, 1.0, None, None, None) == -1
    assert L.fi_class_mean_forward(None, None, 0, 8, 500, None, None, None, None) == -3
    assert L.fi_class_mean_workspace_bytes(2048, 1024, 81) == 32 * 81 * 1024 * 4
    # channels-last pyramid crop: level array required with several maps, crop bounded by the LDS tile
    import ctypes
    ptrs = (ctypes.c_void_p * 2)(16, 32)
    hs = (ctypes.c_int * 2)(8, 4)
    assert L.fi_pyramid_crop_forward_nhwc(ptrs, hs, hs, 2, 16, 16, None, 1, 1, 64, 7, 7, 0.0, 16, None) == -1
    assert b"level" in L.fi_last_error()
    assert L.fi_pyramid_crop_forward_nhwc(ptrs, hs, hs, 0, 16, 16, 16, 1, 1, 64, 7, 7, 0.0, 16, None) == -1
    # bf16-weight patch convolution and the optimiser step validate before touching the device
    assert L.fi_conv3x3_forward_bf16w(16, 16, None, None, None, 16, 1, 32, 8, 18, 128, 0, 0, None) == -3
    assert b"W % 4" in L.fi_last_error()
    assert L.fi_conv3x3_forward_bf16w(None, 16, None, None, None, 16, 1, 32, 8, 16, 128, 0, 0, None) == -1
    assert L.fi_conv1x1_forward_bf16w(16, 16, None, None, None, 16, 1, 96, 64, 128, 0, None) == -3     # Cin % 64
    assert L.fi_conv1x1_forward_bf16w(16, 16, None, None, None, 16, 1, 64, 50, 128, 0, None) == -3     # H*W % 4
    assert L.fi_conv1x1_forward_bf16w(None, 16, None, None, None, 16, 1, 64, 64, 128, 0, None) == -1
    assert L.fi_sgd_chunks(0) == 0 and L.fi_sgd_chunks(1) == 1 and L.fi_sgd_chunks(8193) == 2
    assert L.fi_sgd_clip_step(None, 0, 0, 1.0, None, None, None) == 0
    assert L.fi_sgd_clip_step(None, 3, 5, 1.0, None, None, None) == -1
    # conv: layouts are validated before anything is launched
    a = [16, 16, None, None, None, 16]
    assert L.fi_conv2d_forward(*a, 1, 32, 8, 8, 64, 3, 3, 1, 1, 1, 1, 0, 5, 0, 0, 0, None) == -1
    assert b"weight_layout" in L.fi_last_error()
    assert L.fi_conv2d_forward(*a, 1, 32, 8, 8, 64, 3, 3, 1, 1, 1, 1, 0, 1, 0, 0, 2, None) == -1
    assert b"output_layout" in L.fi_last_error()
    assert L.fi_conv2d_forward(*a, 1, 30, 8, 8, 64, 3, 3, 1, 1, 1, 1, 0, 1, 0, 0, 0, None) == -1      # tap-major needs Cin % 16
    assert L.fi_conv2d_forward(*a, 1, 32, 8, 8, 62, 3, 3, 1, 1, 1, 1, 0, 1, 0, 0, 1, None) == -1      # NHWC needs Cout % 4
    assert L.fi_bn_act_backward(16, 16, 16, None, None, None, 1, 8, 16, 1, 16, None, 16, None, None, 3, 0, None) == -1


def test_round3_entry_points_validate_and_gradient_handoffs_on_the_host():
    """The entry points added for the unscaled-gradient backward reject bad arguments before any HIP call, and the
    host-side hand-off logic (GradBox pairs, Gate claims) behaves on CPU tensors: nothing is claimed, nothing is given."""
    import torch
    from feature_intertwiner_amd import _lib, conv as C
    L = _lib.load()
    a = [16, 16, None, None, None, 32, 16]                   # x, w, bias, scale, residual, gate, y
    assert L.fi_conv2d_forward_gated(*a, 1, 32, 8, 8, 64, 1, 1, 1, 1, 0, 0, 0, 1, 0, 0, 1, None) == -1      # gate + NHWC output
    assert b"gate" in L.fi_last_error()
    assert L.fi_relu_mask(None, None, None, -1, None) == -1
    assert L.fi_relu_mask(None, None, None, 0, None) == 0
    assert L.fi_relu_mask(None, 16, 16, 8, None) == -1
    assert L.fi_bn_fold_grad(None, 16, 16, 16, 16, 16, 0.001, None, None, None, 8, 8, 1, 0, 0, None) == -1
    assert L.fi_bn_fold_grad(16, 16, 16, 16, 16, 16, 0.001, None, None, None, 0, 8, 1, 0, 0, None) == -1
    assert L.fi_bn_fold_batch(None, 0, 0, None) == 0 and L.fi_bn_fold_batch(None, 3, 64, None) == -1
    assert L.fi_sum2x2(16, 16, 1, 4, 5, None) == -1                                   # odd width
    assert L.fi_sum2x2(None, None, 0, 4, 4, None) == 0
    assert L.fi_maxpool3x3s2_forward(16, 16, 1, 8, 6, None) == -1                     # width % 4
    assert L.fi_maxpool3x3s2_backward(16, 16, 16, 1, 2, 8, 0, None) == -1             # height < 3
    assert L.fi_stride2_interleave_gated(None, None, None, None, None, None, None, 1, 4, 4, None) == -1
    # GradBox pairs: (compact, full) for the compact 1x1 / stride-2 path, one value alone, nothing -> None
    b1, b2 = C.GradBox(), C.GradBox()
    assert C._take_boxes(None) is None and C._take_boxes((b1, b2)) is None
    t = torch.ones(1, 2, 4, 4)
    cp = C._Compact(torch.ones(1, 2, 2, 2), (4, 4))
    b1.value = cp
    assert C._take_boxes((b1, b2)) is cp and b1.value is None
    b1.value, b2.value = cp, t
    got = C._take_boxes((b1, b2))
    assert isinstance(got, tuple) and got[0] is cp and got[1] is t and b1.value is None and b2.value is None
    b1.value = t
    assert C._take_boxes(b1) is t
    # a Gate is only ever claimed for a CUDA tensor that requires grad, and only a taker's box is given to
    x = torch.ones(1, 2, 4, 4, requires_grad=True)
    x._fi_gate = C.Gate()
    assert C._claim_gate(x, True) is False and not x._fi_gate.claimed
    assert C.GradBox().taker is False


def _planned(query, *args):
    import ctypes
    from feature_intertwiner_amd import _lib
    k = ctypes.c_int(-1)
    tail = (None,) if query.__name__ == "fi_conv2d_weight_grad_plan" else ()       # its per_launch: not asked for
    rc = query(*args, ctypes.byref(k), *tail)
    return _lib.KERNEL_KEYS[k.value] if rc == 0 else rc


def test_plan_queries_name_the_kernel_on_both_sides_of_every_threshold():
    """fi_conv2d_forward_plan / fi_conv2d_weight_grad_plan / fi_gemm_nt_plan are the planners of the launch entries run on the
    host: aligned fake pointer values, shapes on both sides of every threshold of the kernel selection.  The expected keys
    follow from the constants of csrc/conv_igemm.hip (tile counts in the comments); tests/test_gpu_conv_plan.py holds the
    same shapes to the profiling counters of the launches on the GPU."""
    from feature_intertwiner_amd import _lib
    L = _lib.load()
    X, Wt, Y, G = 0x10000, 0x20000, 0x30000, 0x40000

    def fwd(N, Cin, H, W, Cout, R, stride, pad, layout, gate=None, y=Y):
        return _planned(L.fi_conv2d_forward_plan, X, Wt, None, None, None, gate, y, N, Cin, H, W, Cout, R, R, stride, stride,
                        pad, pad, 0, layout, 0, 0, 0)

    # 3x3 / s1 / p1, tap-major, Cin 16, Cout 256: 2-D patch tiles from 256 workgroups, flat ones (14 x 14 maps) from 512
    assert fwd(1, 16, 128, 128, 256, 3, 1, 1, 1) == "conv3x3_patch"                     # 256 tiles
    assert fwd(1, 16, 120, 128, 256, 3, 1, 1, 1) == "conv_fwd_bm64_3x3"                 # 240
    assert fwd(168, 16, 14, 14, 256, 3, 1, 1, 1) == "conv3x3_patch_flat"                # 516
    assert fwd(166, 16, 14, 14, 256, 3, 1, 1, 1) == "conv_fwd_bm64_3x3"                 # 510
    # 12-wide maps: flat tiles too (their 14 patch rows are an instantiation of their own), forward and data gradient; a
    # 10-wide tile would touch 16
    assert fwd(227, 16, 12, 12, 256, 3, 1, 1, 1) == "conv3x3_patch_flat"                # 512
    assert fwd(227, 16, 12, 12, 256, 3, 1, 1, 2) == "conv3x3_patch_flat"
    assert fwd(273, 16, 10, 12, 256, 3, 1, 1, 1) == "conv3x3_patch_flat"                # 512, H != W
    assert fwd(226, 16, 12, 12, 256, 3, 1, 1, 1) == "conv_fwd_bm64_3x3"                 # 510
    assert fwd(400, 16, 10, 10, 256, 3, 1, 1, 1) == "conv_fwd_bm128_3x3"                # width 10
    assert fwd(168, 16, 14, 14, 256, 3, 1, 1, 1, gate=G + 8) == "conv3x3_patch_flat"
    # a gate that is 4- but not 8-byte aligned: not the flat kernel -- the generic one, whose 516 tiles take 128 rows
    assert fwd(168, 16, 14, 14, 256, 3, 1, 1, 1, gate=G + 4) == "conv_fwd_bm128_3x3"
    assert fwd(168, 16, 14, 14, 256, 3, 1, 1, 1, y=Y + 4) == "conv_fwd_bm128_3x3"       # ... and so for y
    # 1x1 / s1, Cout 256: weights in registers from 256 tiles and 128 input channels; fragment-major weights: its ring form
    assert fwd(1, 128, 128, 128, 256, 1, 1, 0, 1) == "conv1x1_reg"
    assert fwd(1, 128, 124, 128, 256, 1, 1, 0, 1) == "conv_fwd_bm64_1x1"                # 248 tiles
    assert fwd(1, 96, 128, 128, 256, 1, 1, 0, 1) == "conv_fwd_bm64_1x1"                 # Cin < 128
    assert fwd(1, 128, 128, 128, 256, 1, 1, 0, 3) == "conv1x1_reg"
    # generic tile height, 3x3 / s2 / p1: 128 rows from 512 tiles of 128 x 128; narrow layers always 64
    assert fwd(1, 16, 512, 256, 256, 3, 2, 1, 1) == "conv_fwd_bm128_3x3"                # 512
    assert fwd(1, 16, 508, 256, 256, 3, 2, 1, 1) == "conv_fwd_bm64_3x3"                 # 508
    assert fwd(2, 3, 64, 64, 64, 7, 2, 3, 0) == "conv_fwd_bm64_7x7"

    # weight gradient 1x1, Cin 1024, Cout 256, 64 x 64 maps: 16 tiles of 128 rows x ceil(pixels / 512) splits x batch >= 768
    def wgrad(N, n, flags=_lib.OUTPUTS_ZEROED, x=X):
        return _planned(L.fi_conv2d_weight_grad_plan, x, Y, Wt, N, 1024, 64, 64, 256, 1, 1, 1, 1, 0, 0, 1, None, flags, n)

    assert wgrad(6, 1) == "conv_wgrad_bm128_1x1" and wgrad(5, 1) == "conv_wgrad_bm64_1x1"
    assert wgrad(6, 1, flags=0) == "conv_wgrad_bm128_1x1"
    assert wgrad(1, 6) == "conv_wgrad_bm128_1x1" and wgrad(1, 5) == "conv_wgrad_bm64_1x1"
    # what fi_conv2d_weight_grad_batch cannot put into one launch runs problem by problem: the single launch's tiles
    assert wgrad(1, 6, flags=0) == "conv_wgrad_bm64_1x1" and wgrad(1, 6, x=X + 4) == "conv_wgrad_bm64_1x1"

    # ... and says so: how many of the n problems the first launch carries
    def per_launch(N, n, flags=_lib.OUTPUTS_ZEROED, x=X):
        return _lib.wgrad_plan(L.fi_conv2d_weight_grad_plan, x, Y, Wt, N, 1024, 64, 64, 256, 1, 1, 1, 1, 0, 0, 1, None, flags,
                               n)[1]

    assert per_launch(1, 6) == 6 and per_launch(1, 6, flags=0) == 1 and per_launch(1, 6, x=X + 4) == 1
    assert per_launch(6, 1) == 1 and per_launch(1, 26) == _lib.WGRAD_BATCH_MAX

    # ... and how the launch cuts its pixels: (splits, pixels per split), a multiple of 16, the last split the short one
    def splits(N, Cin, H, W, Cout, k, pad, n=1):
        return _lib.wgrad_plan(L.fi_conv2d_weight_grad_split_plan, X, Y, Wt, N, Cin, H, W, Cout, k, k, 1, 1, pad, pad, 1, None,
                               _lib.OUTPUTS_ZEROED, n)

    assert splits(6, 1024, 64, 64, 256, 1, 0) == (48, 512) and splits(5, 1024, 64, 64, 256, 1, 0) == (32, 640)
    assert splits(3, 128, 18, 22, 128, 3, 1) == (3, 400)                                # 1188 pixels: the last split has 388
    assert splits(1, 128, 4, 4, 128, 3, 1) == (1, 16)
    assert L.fi_conv2d_weight_grad_split_plan(X, Y, Wt, 1, 128, 4, 4, 128, 3, 3, 1, 1, 1, 1, 1, None, 0, 1, None, None) == -1

    # fi_conv2d_weight_grad_layout: tap-major dW for whole 128-channel tiles, or 64 channels on a same-size stride-1 layer
    # with aligned operands; a tap-major request is rejected on exactly the shapes that answer 0
    def layout(Cin, stride=1, x=X):
        import ctypes
        v = ctypes.c_int(-1)
        g = (x, Y, 2, Cin, 16, 16, 64, 3, 3, stride, stride, 1, 1)
        assert L.fi_conv2d_weight_grad_layout(*g, ctypes.byref(v)) == 0
        rc = _planned(L.fi_conv2d_weight_grad_plan, x, Y, Wt, *g[2:], 1, None, 0, 1)
        assert (rc == -1 and b"weight_layout 1" in L.fi_last_error()) if v.value == 0 else isinstance(rc, str), (g, rc)
        return v.value

    assert layout(128) == 1 and layout(128, stride=2) == 1 and layout(64) == 1
    assert layout(64, stride=2) == 0 and layout(64, x=X + 4) == 0 and layout(32) == 0
    assert L.fi_conv2d_weight_grad_layout(X, Y, 0, 64, 16, 16, 64, 3, 3, 1, 1, 1, 1, None) == -1

    # the GEMM on the same tile counts (M = Cout, N = Cin, K = pixels), and its workspace: splits x M x N floats
    def gemm(M, N, K, a=X):
        return _planned(L.fi_gemm_nt_plan, a, Wt, None, None, Y, M, N, K, 0, G)

    assert gemm(256, 1024, 24576) == "conv_wgrad_bm128_1x1" and gemm(256, 1024, 20480) == "conv_wgrad_bm64_1x1"
    assert gemm(64, 1024, 24576) == "conv_wgrad_bm64_1x1"
    mb = 4 * 256 * 1024
    assert L.fi_gemm_nt_workspace_bytes(256, 1024, 24576) == 48 * mb
    assert L.fi_gemm_nt_workspace_bytes(256, 1024, 20480) == 32 * mb
    assert L.fi_gemm_nt_workspace_bytes(2048, 1024, 12544) == 8 * 4 * 2048 * 1024
    assert L.fi_gemm_nt_workspace_bytes(1408, 1024, 25088) == 11 * 4 * 1408 * 1024

    # an argument the launch entry rejects is rejected by the query, with the same status (and before any HIP call)
    a = [16, 16, None, None, None, 32, 16]
    for tail in ((1, 32, 8, 8, 64, 3, 3, 1, 1, 1, 1, 0, 5, 0, 0, 0),           # weight_layout
                 (1, 32, 8, 8, 64, 3, 3, 1, 1, 1, 1, 0, 1, 0, 0, 2),           # output_layout
                 (1, 30, 8, 8, 64, 3, 3, 1, 1, 1, 1, 0, 1, 0, 0, 0),           # tap-major needs Cin % 16
                 (1, 32, 8, 8, 64, 1, 1, 1, 1, 0, 0, 0, 1, 0, 0, 1),           # gate + channels-last output
                 (1, 64, 8, 8, 64, 1, 1, 1, 1, 0, 0, 0, 3, 0, 0, 0),           # ring weights on an ineligible shape
                 (0, 32, 8, 8, 64, 3, 3, 1, 1, 1, 1, 0, 1, 0, 0, 0)):          # empty batch
        assert _planned(L.fi_conv2d_forward_plan, *a, *tail) == L.fi_conv2d_forward_live(*a, *tail, None, None) == -1, tail
    assert _planned(L.fi_conv2d_forward_plan, None, *a[1:], 1, 32, 8, 8, 64, 3, 3, 1, 1, 1, 1, 0, 1, 0, 0, 0) == -1
    w = (16, 16, 16, 1, 32, 8, 8, 64, 3, 3, 1, 1, 1, 1, 1, None, 0)            # tap-major dW needs Cin % 128 (or Cin == 64)
    assert _planned(L.fi_conv2d_weight_grad_plan, *w, 1) == L.fi_conv2d_weight_grad(*w, None) == -1
    assert b"weight_layout 1" in L.fi_last_error()
    assert _planned(L.fi_conv2d_weight_grad_plan, *w[:14], 0, None, 0, 0) == -1                      # n < 1
    for g in ((16, 16, None, None, 16, 8, 100, 64, 0, 16),                     # N % 128
              (16, 16, None, None, 16, 8, 128, 62, 0, 16),                     # K % 4
              (16, 16, 8, None, 16, 8, 128, 64, 0, 16),                        # scale not 16-byte aligned
              (16, 16, None, None, 16, 8, 128, 64, 0, None)):                  # no workspace
        assert _planned(L.fi_gemm_nt_plan, *g) == L.fi_gemm_nt_affine(*g, None, None) == -1, g


def _with_env(name, fn):
    """fn() with `name`=1 in the environment (the library reads these switches per call)."""
    assert name not in os.environ
    os.environ[name] = "1"
    try:
        return fn()
    finally:
        del os.environ[name]


def test_launch_queries_hold_every_decision_of_a_launch_on_both_sides_of_its_threshold():
    """fi_conv2d_forward_launches / fi_conv2d_weight_grad_launch / fi_gemm_nt_launch answer with the whole launch plan --
    form, tiles, flags, grid, the pixel ranges of a main / tail pair -- that the launchers dispatch on.  Aligned fake
    pointers; the expected values follow from the rules stated with FiConvLaunch in include/fi_capi.h (tile counts in the
    comments); tests/test_gpu_conv32_edges.py holds the launches of its tables' shapes to the float64 reference."""
    import ctypes
    import test_gpu_conv32_edges as E
    from feature_intertwiner_amd import _lib
    L = _lib.load()
    X, Wt, Y, G = 0x10000, 0x20000, 0x30000, 0x40000

    def fwd(N, Cin, H, W, Cout, R, stride, pad, layout, ol=0, y=Y, gate=None):
        planned = _lib.planned_launches(L.fi_conv2d_forward_launches, X, Wt, None, None, None, gate, y, N, Cin, H, W, Cout, R, R,
                                        stride, stride, pad, pad, 0, layout, 0, 0, ol)
        return [E.launch_summary(p) for p in planned], [(p.p_base, p.pixels) for p in planned]

    def row(name, **kw):
        return fwd(*E.FWD[name][:9], **kw)[0]

    # every forward row of the GPU table: the plan the GPU test asserts before it launches, here without a device
    for name in E.FWD:
        for ol in (0, 1) if name in E.FWD_LAUNCH_CL else (0,):
            expect, ranges = E.expected_launches(name, ol)
            got = fwd(*E.FWD[name][:9], ol=ol)
            assert got[0] == expect and (ranges is None or got[1] == ranges), (name, ol, got)
    # tail launch: 513 x 2 = 1026 tiles of 128 x 128 -> 512 x 2 tiles over 65536 pixels + 128 pixels on 64 x 64 tiles at
    # p_base 65536; K = 96 < 128 keeps the plain tile order.  1024 tiles: one launch
    tail = ("GENERIC", 64, 64, "tap_major vec_out", 2, 4)
    assert fwd(1, 96, 216, 304, 256, 1, 1, 0, 1) == ([("GENERIC", 128, 128, "tap_major vec_out", 512, 2), tail],
                                                     [(0, 65536), (65536, 128)])
    assert fwd(1, 96, 256, 256, 256, 1, 1, 0, 1) == ([("GENERIC", 128, 128, "tap_major vec_out", 512, 2)], [(0, 65536)])
    # ... with a swizzled main launch (3x3: nx 512, already a multiple of 8); without a tail 513 tiles pad to 520; the
    # generic_bm128 row (nx 256) is the unswizzled side
    assert fwd(1, 16, 432, 608, 256, 3, 2, 1, 1) == ([("GENERIC", 128, 128, "tap_major vec_out swizzled", 512, 2), tail],
                                                     [(0, 65536), (65536, 128)])
    assert fwd(1, 16, 432, 608, 128, 3, 2, 1, 1)[0] == [("GENERIC", 128, 128, "tap_major vec_out swizzled", 520, 1)]
    assert "swizzled" not in row("generic_bm128")[0][3]
    # 64-pixel tiles: fewer than 1024 workgroups of 64 x 128 (patch_nb: 120 x 4); not at 1024, not below 64 pixels
    assert row("patch_nb") == [("GENERIC", 64, 64, "tap_major vec_out", 240, 4)]
    assert fwd(1, 64, 256, 512, 64, 1, 1, 0, 1)[0] == [("GENERIC", 64, 128, "tap_major vec_out", 1024, 1)]
    assert fwd(1, 16, 4, 4, 64, 3, 1, 1, 1)[0] == [("GENERIC", 64, 128, "tap_major vec_out", 1, 1)]
    # vector epilogue: needs OH * OW % 4 == 0 (reg1x1_nb_hw: 127 x 129) and a 16-byte aligned y
    assert "vec_out" in row("patch_nb")[0][3] and "vec_out" not in row("reg1x1_nb_hw")[0][3]
    assert row("patch_nb", y=Y + 4) == [("GENERIC", 64, 64, "tap_major", 240, 4)]
    # row-major weights (7x7 is instantiated for them alone), channels-last output, the flat kernel's 13 / 14 patch rows
    assert row("stem") == [("GENERIC", 64, 128, "vec_out", 16, 1)]
    assert _lib.WINDOWS[_lib.planned_launches(L.fi_conv2d_forward_launches, X, Wt, None, None, None, None, Y, 2, 3, 64, 64, 64, 7, 7,
                                              2, 2, 3, 3, 0, 0, 0, 0, 0)[0].window] == "7x7"
    assert _lib.WINDOWS[_lib.planned_launches(L.fi_conv2d_forward_launches, X, Wt, None, None, None, None, Y, 2, 16, 64, 64, 64, 7, 7,
                                              2, 2, 3, 3, 0, 1, 0, 0, 0)[0].window] == "other"      # tap-major 7x7: run-time window
    assert row("patch_nb", ol=1) == [("GENERIC", 64, 128, "tap_major channels_last", 120, 4)]
    assert row("flat14")[0][0] == "PATCH_FLAT13" and row("flat12")[0][0] == "PATCH_FLAT14"
    # Winograd: the 14 x 14 instantiation on a flat slot, H and W at run time on a 2-D one (a row of
    # tests/test_gpu_conv_wino2d.py); FI_NO_WINOGRAD, read per call, turns both into the direct form; 8-byte alignment of a gate
    w14, w2d = (168, 64, 14, 14, 256, 3, 1, 1, 1), (1, 64, 128, 128, 256, 3, 1, 1, 1)
    assert fwd(*w14)[0] == [("WINO14", 128, 128, "tap_major", 528, 1)]               # 8232 tiles: 258 groups of 32 -> 264, x 2
    assert fwd(*w2d)[0] == [("WINO", 128, 128, "tap_major", 256, 1)]                 # 4096 tiles: 128 groups, x 2
    assert _with_env("FI_NO_WINOGRAD", lambda: fwd(*w14)[0]) == [("PATCH_FLAT13", 128, 128, "tap_major", 528, 1)]
    assert _with_env("FI_NO_WINOGRAD", lambda: fwd(*w2d)[0]) == [("PATCH", 128, 128, "tap_major vec_out", 256, 1)]
    assert fwd(*w2d, gate=G + 8)[0][0][0] == "WINO" and fwd(*w2d, gate=G + 4)[0][0][0] == "PATCH"
    assert _with_env("FI_NO_PATCH", lambda: fwd(*w2d)[0][0][0]) == "GENERIC"
    assert _with_env("FI_NO_REG1X1", lambda: row("reg1x1")[0][0]) == "GENERIC" and row("reg1x1")[0][0] == "REG1X1"
    assert fwd(1, 128, 128, 128, 256, 1, 1, 0, 3)[0][0][0] == "RING"

    # weight gradient: the form and flags of every row of the GPU table
    def wgrad(name, n=1, flags=0):
        N, Cin, H, W, Cout, k, st, pd, layout = E.WGRAD[name][:9]
        (p,) = _lib.planned_launches(L.fi_conv2d_weight_grad_launch, X, Y, Wt, N, Cin, H, W, Cout, k, k, st, st, pd, pd, layout, None,
                                     flags, n)
        assert _lib.KERNEL_KEYS[p.kernel_id] == E.WGRAD[name][9] or n > 1
        return (_lib.WGRAD_FORMS[p.form], {k for k in ("swizzled", "row_uniform") if p.flags & _lib.LAUNCH_FLAGS[k]}), p

    for name in E.WGRAD:
        assert wgrad(name)[0] == E.wgrad_form_and_flags(name), name
    assert {E.wgrad_form_and_flags(n)[0] for n in E.WGRAD} == set(_lib.WGRAD_FORMS)
    # the 1-D XCD-aware grid: from 32768 pixels (unless FI_NO_WG_SWZ) and for any batch, whatever the switch
    assert "swizzled" in wgrad("vec_swizzled")[0][1] and "swizzled" not in wgrad("bm128")[0][1]              # 24576 pixels
    assert "swizzled" not in _with_env("FI_NO_WG_SWZ", lambda: wgrad("vec_swizzled"))[0][1]
    for name in ("vec_3x3", "vec_swizzled"):
        both, p = _with_env("FI_NO_WG_SWZ", lambda: wgrad(name, n=5, flags=_lib.OUTPUTS_ZEROED))
        assert "swizzled" in both[1] and p.per_launch == 5, name
    assert "swizzled" not in wgrad("vec_3x3", n=5)[0][1] and wgrad("half_3x3", n=5, flags=_lib.OUTPUTS_ZEROED)[1].per_launch == 1
    # the launch query and the older readers agree: tile rows, grid = column tiles x Cout tiles x splits
    p = wgrad("vec_partial_split")[1]
    assert (p.tile_rows, p.window, p.grid_x, p.grid_y, p.grid_z, p.splits, p.pixels_per_split) == (64, 1, 9, 2, 3, 3, 400)
    # fi_gemm_nt: the vector form on the K of tests/test_gpu_conv_plan.py::test_flop_log_gemm
    for K, rows_, splits, pps in ((24576, 128, 48, 512), (20480, 64, 32, 640)):
        (p,) = _lib.planned_launches(L.fi_gemm_nt_launch, X, Wt, None, None, Y, 256, 1024, K, 0, G)
        assert (_lib.WGRAD_FORMS[p.form], p.tile_rows, p.splits, p.pixels_per_split) == ("VEC", rows_, splits, pps)
        assert (p.grid_x, p.grid_y, p.grid_z) == (8, 256 // rows_, splits) and p.flags == 1 | 16      # tap-major, row-uniform
    # rejected argument lists: the same status as the launch entry, nothing written
    a = [16, 16, None, None, None, 32, 16]
    out, n = (_lib.ConvLaunch * 2)(), ctypes.byref(ctypes.c_int(-1))
    bad = (1, 32, 8, 8, 64, 3, 3, 1, 1, 1, 1, 0, 5, 0, 0, 0)
    assert L.fi_conv2d_forward_launches(*a, *bad, out, n) == L.fi_conv2d_forward_live(*a, *bad, None, None) == -1
    assert L.fi_conv2d_forward_launches(*a, *bad[:12], 1, 0, 0, 0, None, None) == -1
    w = (16, 16, 16, 1, 32, 8, 8, 64, 3, 3, 1, 1, 1, 1, 1, None, 0)
    assert L.fi_conv2d_weight_grad_launch(*w, 1, out) == L.fi_conv2d_weight_grad(*w, None) == -1
    assert L.fi_conv2d_weight_grad_launch(*w[:14], 0, None, 0, 0, out) == -1 and L.fi_conv2d_weight_grad_launch(*w, 1, None) == -1
    g = (16, 16, None, None, 16, 8, 100, 64, 0, 16)
    assert L.fi_gemm_nt_launch(*g, out) == L.fi_gemm_nt_affine(*g, None, None) == -1


def test_fp32_launchers_only_dispatch():
    """Every threshold, alignment test and environment switch of the fp32 convolutions lives in the planners of
    csrc/conv_igemm.hip: launch_fwd, launch_wgrad and fi_conv2d_forward_live behind its plan_forward call hold none."""
    src = open(os.path.join(ROOT, "feature_intertwiner_amd", "csrc", "conv_igemm.hip")).read()

    def body(signature, start_after=None):
        at = src.index(signature)
        i, depth = src.index("{", src.index(")", at)), 0
        for j in range(i, len(src)):
            depth += {"{": 1, "}": -1}.get(src[j], 0)
            if depth == 0:
                text = src[i:j + 1]
                return text[text.index(start_after):] if start_after else text
        raise AssertionError(signature)

    bodies = {"launch_fwd": body("void launch_fwd("), "launch_wgrad_bm": body("void launch_wgrad_bm("),
              "launch_wgrad": body("void launch_wgrad("),
              "fi_conv2d_forward_live": body("int fi_conv2d_forward_live(", start_after="plan_forward(")}
    for name, text in bodies.items():
        assert "hipLaunchKernelGGL" in text or "launch_wgrad_bm" in text, name
        for token in ("getenv", "% 16 == 0", "1024", "32768", ">= 512", "rem * 3"):
            assert token not in text, (name, token)


def test_16bit_forward_plan_names_the_variant_on_both_sides_of_every_threshold():
    """fi_conv2d_forward_plan_{bf16,f16} is the planner of fi_conv2d_forward_live_{bf16,f16} run on the host: aligned fake
    pointer values, shapes on both sides of every threshold of csrc/conv_bf16.hip (tile counts in the comments: 8 x 16 or
    128-pixel tiles x 128 output channels), each with and without a 16-bit weight copy.  tests/test_gpu_conv16_plan.py
    holds the launches of the same shapes to the variant named here."""
    import ctypes
    from feature_intertwiner_amd import _lib
    L = _lib.load()
    X, Wt, W16, Y, G, RES = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000

    def plan(sfx, N, Cin, H, W, R, stride, pad, copy, Cout=256, x=X, y=Y, residual=None, gate=None, out_hw=(0, 0), ocl=0,
             w16=W16):
        v = ctypes.c_int(-1)
        rc = getattr(L, "fi_conv2d_forward_plan_" + sfx)(x, Wt, w16 if copy else None, None, None, residual, gate, y, N, Cin,
                                                          H, W, Cout, R, R, stride, stride, pad, pad, 0, 1, out_hw[0],
                                                          out_hw[1], ocl, ctypes.byref(v))
        return _lib.CONV16_VARIANTS[v.value] if rc == 0 else rc

    def both(sfx, *a, **kw):
        return plan(sfx, *a, True, **kw), plan(sfx, *a, False, **kw)

    for sfx in ("bf16", "f16"):
        c3 = lambda N, H, W, **kw: both(sfx, N, 32, H, W, 3, 1, 1, **kw)              # 3x3 / s1 / p1, Cin 32
        c1 = lambda N, Cin, H, W, **kw: both(sfx, N, Cin, H, W, 1, 1, 0, **kw)        # 1x1 / s1 / p0
        # 2-D patch tiles from 192 workgroups
        assert c3(1, 96, 128) == ("PATCH_W16", "PATCH")                               # 12 x 8 x 2 = 192 tiles
        assert c3(1, 88, 128) == ("GENERIC_BM64", "GENERIC_BM64")                     # 176
        assert c3(1, 96, 132) == ("PATCH_W16", "PATCH")                               # 216, the last column tile partial
        assert c3(1, 96, 130) == ("GENERIC_BM64", "GENERIC_BM64")                     # W % 4 != 0
        # flat tiles (widths 12 and 14) from 512 workgroups, only with a copy; the generic kernel's 128 rows from 512 of
        # ITS tiles (rows padded to quads: 14 -> 16 columns)
        assert c3(167, 14, 14) == ("PATCH_FLAT_W16", "GENERIC_BM128")                 # 256 x 2 = 512 flat; 293 x 2 generic
        assert c3(166, 14, 14) == ("GENERIC_BM128", "GENERIC_BM128")                  # 510 flat; 291 x 2 generic
        # (227 x 144 pixels are 256 generic tiles x 2 = 512: 128 rows.  The issue's table says GENERIC_BM64 for this
        # launch without a copy; the parent commit's bm rule -- `tiles < 512 ? 64 : 128` -- gives 128 rows.)
        assert c3(227, 12, 12) == ("PATCH_FLAT_W16", "GENERIC_BM128")                 # 512 flat
        assert c3(226, 12, 12) == ("GENERIC_BM64", "GENERIC_BM64")                    # 510 flat, 510 generic
        assert c3(400, 10, 10) == ("GENERIC_BM128", "GENERIC_BM128")                  # width 10: 15 patch rows per tile
        # 16-byte alignment of every tensor the fast kernels touch
        for kw in (dict(gate=G + 8), dict(residual=RES + 8), dict(x=X + 8), dict(y=Y + 8)):
            assert c3(167, 14, 14, **kw) == ("GENERIC_BM128", "GENERIC_BM128"), kw
        # an explicit output size, channels-last output: no variant that reads the copy
        assert c3(1, 96, 128, out_hw=(96, 128)) == ("PATCH", "PATCH")
        assert c3(1, 96, 128, ocl=1) == ("GENERIC_BM64", "GENERIC_BM64")
        # 1x1: weights in registers from 192 tiles, whole 64-channel stages, whole quads, more than 64 output channels
        assert c1(1, 64, 96, 128) == ("REG1X1_W16", "GENERIC_BM64")                   # 96 x 2 = 192
        assert c1(1, 64, 95, 128) == ("GENERIC_BM64", "GENERIC_BM64")                 # 190
        assert c1(1, 96, 96, 128) == ("GENERIC_BM64", "GENERIC_BM64")                 # Cin % 64
        assert c1(3, 64, 65, 63) == ("GENERIC_BM64", "GENERIC_BM64")                  # H*W % 4
        assert c1(4, 64, 128, 128) == ("REG1X1_W16", "GENERIC_BM128")                 # 1024 tiles
        assert c1(1, 64, 96, 128, Cout=64) == ("GENERIC_BM64", "GENERIC_BM64")
        # generic tile height, 3x3 / s2 / p1
        assert both(sfx, 1, 32, 512, 256, 3, 2, 1) == ("GENERIC_BM128", "GENERIC_BM128")      # 512
        assert both(sfx, 1, 32, 508, 256, 3, 2, 1) == ("GENERIC_BM64", "GENERIC_BM64")        # 508

        # an argument the launch entry rejects is rejected by the query, with the same status (and before any HIP call)
        live = getattr(L, "fi_conv2d_forward_live_" + sfx)
        query = getattr(L, "fi_conv2d_forward_plan_" + sfx)
        ok = (1, 32, 96, 128, 256, 3, 3, 1, 1, 1, 1, 0, 1, 0, 0, 0)
        for ptrs, tail, status in (((X, Wt, W16, None, None, None, None, Y), (1, 48) + ok[2:], -3),      # Cin % 32
                                   ((None, Wt, W16, None, None, None, None, Y), ok, -1),                 # no x
                                   ((X, Wt, W16 + 8, None, None, None, None, Y), ok, -1),                # copy misaligned
                                   ((X, Wt + 8, None, None, None, None, None, Y), ok, -1),               # weight misaligned
                                   ((X, Wt, None, None, None, None, G, Y), ok[:-1] + (1,), -1),          # gate + channels-last
                                   ((X, Wt, W16, None, None, None, None, Y), (0,) + ok[1:], -1)):        # empty batch
            v = ctypes.c_int(-1)
            assert query(*ptrs, *tail, ctypes.byref(v)) == live(*ptrs, *tail, None, None) == status, (ptrs, tail)
        assert query(X, Wt, None, None, None, None, None, Y, *ok, None) == -1


def test_16bit_forward_plan_holds_the_edge_shape_table():
    """Every row of tests/test_gpu_conv16_edges.py's CASES reaches the variant the table names, with a 16-bit weight copy
    and without one, for both types: the planner run on the host with aligned fake pointer values.  The GPU file asserts
    the same answers with its real pointers before every launch; a row that stops reaching its kernel fails here first."""
    import ctypes
    import test_gpu_conv16_edges as E
    from feature_intertwiner_amd import _lib
    L = _lib.load()
    X, Wt, W16, Y = 0x10000, 0x20000, 0x30000, 0x40000
    assert len(E.CASES) >= 50 and set(E.EPILOGUE_SHAPES) <= set(E.CASES)
    for sfx in ("bf16", "f16"):
        query = getattr(L, "fi_conv2d_forward_plan_" + sfx)
        for name, row in E.CASES.items():
            N, Cin, H, W, Cout, R, S, sh, sw, ph, pw, layout, out_hw, with_copy, without = row
            oh, ow = out_hw if out_hw is not None else (0, 0)
            got = []
            for w16 in (W16, None):
                v = ctypes.c_int(-1)
                rc = query(X, Wt, w16, None, None, None, None, Y, N, Cin, H, W, Cout, R, S, sh, sw, ph, pw, 0, layout, oh, ow,
                           0, ctypes.byref(v))
                assert rc == 0, (sfx, name, rc)
                got.append(_lib.CONV16_VARIANTS[v.value])
            assert tuple(got) == (with_copy, without), (sfx, name, got)
    # every fast variant and both generic tile heights are in the table, each fast one also with tap-reversed weights
    for variant in ("PATCH_W16", "PATCH_FLAT_W16", "REG1X1_W16"):
        assert {row[11] for row in E.CASES.values() if row[13] == variant} == {1, 2}, variant
    assert {row[14] for row in E.CASES.values()} == {"GENERIC_BM64", "GENERIC_BM128", "PATCH"}


def test_16bit_weight_grad_plan_names_the_variant_on_both_sides_of_every_threshold():
    """fi_conv2d_weight_grad_plan_{bf16,f16} is the planner of fi_conv2d_weight_grad_db_{bf16,f16} and of the batch entry
    run on the host: aligned fake pointer values, shapes on both sides of every threshold of the weight gradient's kernel
    selection in csrc/conv_bf16.hip, and the number of problems a launch carries.  tests/test_gpu_wgrad16_plan.py holds
    the launches of the same shapes to the answers named here."""
    from feature_intertwiner_amd import _lib
    L = _lib.load()
    X, DY, DW, DB = 0x10000, 0x20000, 0x30000, 0x40000
    Z = _lib.OUTPUTS_ZEROED

    for sfx in ("bf16", "f16"):
        query = getattr(L, "fi_conv2d_weight_grad_plan_" + sfx)
        launch = getattr(L, "fi_conv2d_weight_grad_db_" + sfx)

        def plan(shape, flags=0, n=1, x=X, dy=DY, db=None):
            N, Cin, H, W, Cout, R, stride, pad = shape
            v, per = _lib.wgrad_plan(query, x, dy, DW, db, N, Cin, H, W, Cout, R, R, stride, stride, pad, pad, flags, n)
            return _lib.WGRAD16_VARIANTS[v], per

        flat = [(1, 64, 8, 8, 64, 1, 1, 0), (1, 64, 8, 8, 64, 3, 1, 1)]
        rows = [(1, 64, 6, 6, 64, 1, 1, 0),          # H * W = 36 < 64
                (1, 64, 9, 9, 64, 1, 1, 0),          # H * W % 4
                (1, 64, 8, 8, 96, 1, 1, 0),          # Cout % 64
                (1, 96, 8, 8, 64, 1, 1, 0),          # Cin % 64
                (1, 64, 8, 8, 64, 3, 1, 0),          # output smaller than the input
                (1, 64, 16, 16, 64, 3, 2, 1)]        # stride 2
        generic = [(2, 64, 3, 3, 64, 3, 1, 1),       # OW < 4
                   (1, 64, 6, 6, 64, 3, 2, 1),       # W < 8 at stride 2
                   (1, 64, 16, 16, 64, 3, 3, 1)]     # stride 3
        for name, shapes in (("FLAT", flat), ("ROWS", rows), ("GENERIC", generic)):
            for shape in shapes:
                assert plan(shape) == (name, 1), shape
                assert plan(shape, db=DB) == (name, 1), shape
                # only the flat kernel carries several problems, and only into outputs the caller has cleared
                assert plan(shape, flags=Z, n=5) == (name, 5 if name == "FLAT" else 1), shape
        assert plan(flat[0], x=X + 4) == ("ROWS", 1) and plan(flat[0], dy=DY + 4) == ("ROWS", 1)
        assert plan(flat[0], flags=Z, n=5, x=X + 4) == ("ROWS", 1)
        assert _lib.WGRAD_BATCH_MAX == 24                                        # FI_WGRAD_BATCH_MAX of fi_capi.h
        assert plan(flat[0], flags=Z, n=26) == ("FLAT", _lib.WGRAD_BATCH_MAX)
        assert plan(flat[0], flags=0, n=5) == ("FLAT", 1)
        assert plan(flat[0], flags=Z, n=1) == ("FLAT", 1)
        # operands of 2 GiB: not the flat kernel, so not one launch either (the batch entry once judged this by a second
        # copy of the predicate that had no size limit)
        assert plan((8192, 1024, 8, 8, 64, 1, 1, 0), flags=Z, n=3) == ("ROWS", 1)
        assert plan((8191, 1024, 8, 8, 64, 1, 1, 0), flags=Z, n=3) == ("FLAT", 3)

        # an argument the launch entry rejects is rejected by the query, with the same status (and before any HIP call)
        import ctypes
        v, per = ctypes.c_int(-1), ctypes.c_int(-1)
        out = (ctypes.byref(v), ctypes.byref(per))
        g = (1, 64, 8, 8, 64, 1, 1, 1, 1, 0, 0)
        assert query(None, DY, DW, None, *g, 0, 1, *out) == launch(None, DY, DW, None, *g, 0, None) == -1      # no x
        assert query(X, DY, DW, None, 0, *g[1:], 0, 1, *out) == launch(X, DY, DW, None, 0, *g[1:], 0, None) == -1    # N = 0
        # (65536 tiles of (tap, 128 input channels): a grid-size requirement, checked before the outputs are cleared)
        big = (1, 128 * 65536, 8, 8, 64, 1, 1, 1, 1, 0, 0)
        assert query(X, DY, DW, None, *big, 0, 1, *out) == launch(X, DY, DW, None, *big, 0, None) == -1
        assert query(X, DY, DW, None, *g, 0, 0, *out) == -1                                                  # n = 0
        assert query(X, DY, DW, None, *g, 0, 1, None, None) == -1
        assert (v.value, per.value) == (-1, -1)


def test_weight_gradient_layout_and_batching_are_stated_once():
    """Which dW layout a weight gradient can be written in and which layers travel several to a launch is decided in
    csrc/conv_igemm.hip and csrc/conv_bf16.hip alone: conv._conv_backward and its two halves ask and restate neither."""
    import inspect
    from feature_intertwiner_amd import conv
    src = "".join(inspect.getsource(f) for f in (conv._conv_backward, conv._weight_grad, conv._data_grad))
    for token in ("0x7fffff00", "% 16 == 0 and dz", "Cin == 64", "% 64", "(3, 3, (1, 1))"):
        assert token not in src, token


def test_conv_owns_no_stream_of_its_own():
    """Weight gradients run on the stream their layer's backward runs on: conv.py makes no stream and no event and waits
    for none, and data_parallel has no weight-gradient stream to wait for."""
    import inspect
    from feature_intertwiner_amd import conv, data_parallel
    src = inspect.getsource(conv)
    for token in ("torch.cuda.Stream(", "wait_stream", "wait_event", "torch.cuda.Event"):
        assert token not in src, token
    assert not hasattr(data_parallel, "conv_wgrad_stream")


def test_forward_kernel_selection_of_the_16bit_path_is_stated_once():
    """The tile sizes and thresholds that choose a 16-bit forward kernel live in csrc/conv_bf16.hip alone: conv._conv_fwd
    hands the launch entry what it has and restates none of them."""
    import inspect
    from feature_intertwiner_amd import conv
    src = inspect.getsource(conv._conv_fwd)
    for token in ("192", "512", "126", "% 64", "Cout > 64", "forward_gated"):
        assert token not in src, token
    assert "tail" not in inspect.signature(conv._lowp_fn).parameters


def test_reference_shaped_python_surface():
    import inspect
    from feature_intertwiner_amd.roi_align.crop_and_resize import CropAndResizeFunction
    from feature_intertwiner_amd.roi_align.roi_align import RoIAlign
    from feature_intertwiner_amd.roi_pooling.functions.roi_pool import RoIPoolFunction
    from feature_intertwiner_amd.roi_pooling.modules.roi_pool import _RoIPooling
    from feature_intertwiner_amd.nms.nms_wrapper import nms
    from feature_intertwiner_amd.nms.pth_nms import pth_nms
    from feature_intertwiner_amd.OT_module import OptTrans
    assert list(inspect.signature(CropAndResizeFunction.__init__).parameters)[1:] == \
        ["crop_height", "crop_width", "extrapolation_value"]
    assert list(inspect.signature(RoIAlign.__init__).parameters)[1:] == \
        ["crop_height", "crop_width", "extrapolation_value", "transform_fpcoor"]
    assert list(inspect.signature(RoIPoolFunction.__init__).parameters)[1:] == \
        ["pooled_height", "pooled_width", "spatial_scale"]
    assert list(inspect.signature(_RoIPooling.__init__).parameters)[1:] == \
        ["pooled_height", "pooled_width", "spatial_scale"]
    assert list(inspect.signature(nms).parameters)[:2] == ["dets", "thresh"]
    assert list(inspect.signature(pth_nms).parameters)[:2] == ["dets", "thresh"]
    assert list(inspect.signature(OptTrans.__init__).parameters)[1:] == [
        "config", "ch_x", "spatial_x", "ch_y", "spatial_y", "epsilon", "L", "remove_bias", "C_form",
        "no_bp_P_L", "skip_critic"]
    import types
    cfg = types.SimpleNamespace(DEV=types.SimpleNamespace(OT_ONE_DIM_FORM="conv"))
    m = OptTrans(cfg, ch_x=1024)
    assert sorted(m.state_dict().keys()) == ["G_net.0.bias", "G_net.0.weight", "critic.0.bias", "critic.0.weight"]
    assert m.critic[0].weight.shape == (256, 1024, 3) and m.epsilon == 1.0 and m.L == 5
    m2 = OptTrans(cfg, ch_x=256, spatial_x=32, spatial_y=64)
    assert m2.two_dim and m2.G_net[0].stride == (2, 2) and m2.critic[3].out_channels == 64


def test_no_cpu_fallback():
    from feature_intertwiner_amd import _lib
    from feature_intertwiner_amd.roi_align.crop_and_resize import CropAndResizeFunction
    from feature_intertwiner_amd.nms.pth_nms import pth_nms
    from feature_intertwiner_amd.OT_module import sinkhorn_loss
    with pytest.raises(_lib.FiError):
        CropAndResizeFunction(7, 7)(torch.zeros(1, 1, 8, 8), torch.zeros(1, 4), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(_lib.FiError):
        pth_nms(torch.zeros(4, 5), 0.5)
    with pytest.raises(_lib.FiError):
        sinkhorn_loss(torch.zeros(1, 4, 1), torch.zeros(1, 4, 1))


def test_product_does_not_import_the_oracle():
    pkg = os.path.join(ROOT, "feature_intertwiner_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                text = open(os.path.join(d, f)).read()
                assert "import oracle" not in text and "from oracle" not in text, f
                assert "libfi_oracle" not in text, f


def test_level_assignment_matches_oracle(oracle):
    import numpy as np
    from feature_intertwiner_amd.intertwiner import roi_level, merge_feat_vec
    rs = np.random.RandomState(0)
    y1, x1 = rs.uniform(0, 0.7, (2, 500))
    rois = np.stack([y1, x1, y1 + np.exp(rs.uniform(-6, -0.3, 500)), x1 + np.exp(rs.uniform(-6, -0.3, 500))], 1)
    rois = rois.astype(np.float32)
    got = roi_level(torch.from_numpy(rois), 1024 * 1024).numpy()
    exp = oracle.roi_level(rois, 1024 * 1024)
    # torch.log vs np.log may differ in the last ulp exactly at a .5 boundary: allow none here
    assert np.array_equal(got, exp)
    f = torch.rand(2, 3, 8, 5)
    c = torch.randint(0, 4, (2, 3, 1, 5)).float()
    m, cs = merge_feat_vec(f, c)
    assert torch.allclose(cs, c.sum((0, 1)))
    assert torch.allclose(m, (f * c).sum((0, 1)) / (cs + 1e-20))


def test_checkpoint_file_round_trip(tmp_path):
    """tools/utils.py:567-586 file layout; resume restores weights, counters and the history buffer."""
    import numpy as np
    import torch
    from feature_intertwiner_amd.checkpoint import load_model, save_model
    from feature_intertwiner_amd.config import make_config
    from feature_intertwiner_amd.model import MaskRCNN
    cfg = make_config(backbone="resnet50", image_size=128, batch_size=1, train_rois_per_image=16)
    torch.manual_seed(0)
    a = MaskRCNN(cfg)
    a.initialize_buffer(torch.device("cpu"))
    a.feature_buffer.buffer.normal_()
    a.feature_buffer.buffer_cnt.fill_(3)
    path = str(tmp_path / "mask_rcnn_ep_0002_iter_000123.pth")
    save_model(a, path, epoch=2, iter=123, loss_data={"x": [1.0]})
    raw = torch.load(path, weights_only=False)
    assert sorted(raw) == ['buffer', 'buffer_cnt', 'epoch', 'iter', 'loss_data', 'state_dict']
    assert isinstance(raw['buffer'], np.ndarray) and raw['buffer'].shape == (1, 1024, 81)
    torch.manual_seed(1)
    b = MaskRCNN(cfg)
    ep, it, loss_data, missing, unexpected = load_model(b, path)
    assert (ep, it) == (2, 124) and loss_data == {"x": [1.0]} and not missing and not unexpected
    for (k, v), (k2, v2) in zip(a.state_dict().items(), b.state_dict().items()):
        assert k == k2 and torch.equal(v, v2)
    assert torch.equal(a.feature_buffer.buffer, b.feature_buffer.buffer)
    assert torch.equal(a.feature_buffer.buffer_cnt, b.feature_buffer.buffer_cnt)
    # bare state dict == pretrain model
    torch.save(a.state_dict(), path)
    assert load_model(MaskRCNN(cfg), path)[:2] == (1, 1)


def test_relu_boundary_evidence_tells_an_event_from_a_bug():
    """workflow._relu_boundary_evidence (advisor: a deviating rpn.conv_shared channel was classified as a ReLU-boundary
    event by footprint only): a sign disagreement between the dense kernel and the row form counts as an event only when
    the float64 pre-activation is within rounding of zero."""
    import types
    import torch
    from feature_intertwiner_amd.workflow import _relu_boundary_evidence
    g = torch.Generator().manual_seed(5)
    per_loc, H, W, Cin, Cout, R = 3, 4, 4, 2, 8, 6
    weight = torch.randn(Cout, Cin, 3, 3, generator=g)
    bias = torch.randn(Cout, generator=g)
    ws = weight.permute(0, 2, 3, 1).reshape(Cout, -1)
    patches = torch.randn(R, 9 * Cin, generator=g)
    # row 2, channel 5: a pre-activation at rounding distance from zero
    bias[5] = -float(patches[2].double() @ ws[5].double())
    z = patches @ ws.t() + bias
    anchor = torch.tensor([0, 7, 13, 20, 31, 47])             # pixel = anchor // per_loc
    img = torch.zeros(R, dtype=torch.long)
    valid = torch.ones(R, dtype=torch.bool)
    dense = torch.zeros(1, Cout, H, W)
    pix = anchor // per_loc
    dense[0, :, pix // W, pix % W] = torch.relu(z).t()
    rpn = types.SimpleNamespace(conv_shared=types.SimpleNamespace(weight=weight, bias=bias))
    probe = {"rows": (img, anchor, valid, per_loc), "patches": patches, "z_rows": z.clone(), "dense_y": [dense.clone()]}
    assert all(e["rows_disagreeing"] == 0 for e in _relu_boundary_evidence(probe, rpn, [5, 1]))
    # the event: the row form lands just above zero, the dense kernel on zero
    probe["z_rows"][2, 5] = 1e-9
    probe["dense_y"][0][0, 5, pix[2] // W, pix[2] % W] = 0.0
    ev = _relu_boundary_evidence(probe, rpn, [5])[0]
    assert ev["rows_disagreeing"] == 1 and ev["within_rounding"] and ev["max_abs_z_over_scale"] <= 16
    # a bug: the evaluations disagree where |z| is far from zero
    r = int(torch.argmax(z[:, 1].abs()))
    probe["z_rows"][r, 1] = -z[r, 1]
    ev = _relu_boundary_evidence(probe, rpn, [1])[0]
    assert ev["rows_disagreeing"] == 1 and not ev["within_rounding"]
