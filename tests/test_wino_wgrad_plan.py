"""The rule that sends a weight gradient to its Winograd F(2x2,3x3) form (plan_wgrad in csrc/conv_igemm.hip, stated with
FI_LAUNCH_WINOGRAD in include/fi_capi.h), on both sides of each of its conditions: the host-only queries
fi_conv2d_weight_grad_launch / _plan / _split_plan with aligned fake pointers, no GPU.  tests/test_gpu_conv_wino_wgrad.py
holds the launches of such shapes to float64."""
import os

X, DY, DW = 0x10000, 0x40000, 0x20000
ZEROED = 1


def _launch(N, Cin, H, W, Cout, k=3, st=1, pd=1, x=X, dy=DY, flags=0, n=1):
    from feature_intertwiner_amd import _lib
    (p,) = _lib.planned_launches(_lib.load().fi_conv2d_weight_grad_launch, x, dy, DW, N, Cin, H, W, Cout, k, k, st, st, pd, pd, 1,
                                 None, flags, n)
    return p


def _wino(*a, **kw):
    from feature_intertwiner_amd import _lib
    return bool(_launch(*a, **kw).flags & _lib.LAUNCH_FLAGS["winograd"])


def _with_env(name, fn):
    assert name not in os.environ
    os.environ[name] = "1"
    try:
        return fn()
    finally:
        del os.environ[name]


def test_flag_value_and_forms_are_as_the_header_says():
    from feature_intertwiner_amd import _lib
    assert _lib.LAUNCH_FLAGS["winograd"] == 32
    assert _lib.WGRAD_FORMS == ("VEC", "VEC_TWO_TAP", "SCALAR_TAP_MAJOR", "SCALAR_ROW_MAJOR")
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fi_capi.h")).read()
    assert "FI_LAUNCH_WINOGRAD = 32" in hdr


def test_every_condition_of_the_rule_on_both_sides():
    from feature_intertwiner_amd import _lib
    base = (2, 256, 8, 8, 256)
    assert _wino(*base)
    # input channels: from 256 (128 and 64 keep the direct kernel: every plan the older tests pin)
    assert not _wino(2, 128, 8, 8, 256) and not _wino(2, 64, 8, 8, 256) and _wino(2, 384, 8, 8, 256)
    # output channels: whole blocks of 64
    assert _wino(2, 256, 8, 8, 320) and _wino(2, 256, 8, 8, 512) and not _wino(2, 256, 8, 8, 288)
    # even H and W (3 x 4 and 4 x 5 maps are still the vector form: H * W % 4 == 0)
    assert _wino(2, 256, 6, 4, 256) and not _wino(2, 256, 3, 4, 256) and not _wino(2, 256, 4, 5, 256)
    assert _lib.WGRAD_FORMS[_launch(2, 256, 3, 4, 256).form] == "VEC" == _lib.WGRAD_FORMS[_launch(2, 256, 4, 5, 256).form]
    # window, stride, padding
    assert not _wino(2, 256, 8, 8, 256, st=2) and not _wino(2, 256, 8, 8, 256, k=1, pd=0) and not _wino(2, 256, 8, 8, 256, k=5, pd=2)
    # alignment of either operand (the vector form's own rule)
    assert not _wino(*base, x=X + 4) and not _wino(*base, dy=DY + 4) and not _wino(*base, x=X + 8)
    assert _wino(*base, x=X + 16, dy=DY + 32)
    # the environment switches, read per call
    assert not _with_env("FI_NO_WINOGRAD_WGRAD", lambda: _wino(*base))
    assert not _with_env("FI_NO_WINOGRAD", lambda: _wino(*base))
    assert _wino(*base)
    # a batch stays on the direct kernel's one launch; problems the batch entry loops over are single launches
    p = _launch(*base, flags=ZEROED, n=5)
    assert p.per_launch == 5 and not p.flags & _lib.LAUNCH_FLAGS["winograd"]
    p = _launch(*base, flags=0, n=5)
    assert p.per_launch == 1 and p.flags & _lib.LAUNCH_FLAGS["winograd"]


def test_the_launch_keeps_its_slot_and_reports_what_the_kernel_does():
    from feature_intertwiner_amd import _lib
    L = _lib.load()
    for shape in ((2, 256, 8, 8, 256), (672, 256, 14, 14, 256), (4, 256, 256, 256, 512)):
        p = _launch(*shape)
        d = _with_env("FI_NO_WINOGRAD_WGRAD", lambda: _launch(*shape))
        assert p.kernel_id == d.kernel_id and _lib.KERNEL_KEYS[p.kernel_id] in ("conv_wgrad_bm64_3x3", "conv_wgrad_bm128_3x3")
        assert _lib.WGRAD_FORMS[p.form] == "VEC" and p.per_launch == 1 and p.window == 1 and p.tile_rows == 64
        f = _lib.LAUNCH_FLAGS
        assert p.flags == f["tap_major"] | f["swizzled"] | f["winograd"]
        N, Cin, H, W, Cout = shape
        tiles = N * (H // 2) * (W // 2)
        assert (p.grid_x, p.grid_y, p.grid_z) == (Cin // 64, Cout // 64, p.splits)
        # whole stages of 4 tiles, every split but the last full, the last not empty
        assert p.pixels_per_split % 16 == 0 and p.pixels == N * H * W
        tps = p.pixels_per_split // 4
        assert (p.splits - 1) * tps < tiles <= p.splits * tps
        # one round of the 256 CUs at most, no split under 32 tiles unless it is the only one
        assert p.grid_x * p.grid_y * p.splits <= 256 and (p.splits == 1 or tps >= 32)
        a = (X, DY, DW, N, Cin, H, W, Cout, 3, 3, 1, 1, 1, 1, 1, None, 0, 1)
        assert _lib.wgrad_plan(L.fi_conv2d_weight_grad_split_plan, *a) == (p.splits, p.pixels_per_split)
        assert _lib.wgrad_plan(L.fi_conv2d_weight_grad_plan, *a) == (p.kernel_id, 1)
    # the step's shapes: 16 blocks x 16 splits (256 -> 256), 32 blocks x 8 splits (256 -> 512 on the largest map)
    assert _launch(672, 256, 14, 14, 256).splits == 16 and _launch(4, 256, 256, 256, 512).splits == 8
    assert _launch(2, 256, 8, 8, 256).splits == 1 and _launch(29, 256, 6, 6, 256).splits == 9
