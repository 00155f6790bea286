"""CPU: libfi_fpn16.so (the backward of the pyramid's top-down step on 16-bit channels-last tensors, include/fi_fpn16.h)
builds for gfx950, exports exactly what its header declares, answers the eligibility query on both sides of every rule
and validates its arguments on the host before any HIP call; TRAIN.ACT_SCOPE is absent by default ('trunk'), 'pyramid'
needs a 16-bit TRAIN.ACT_PRECISION and anything else is a ValueError naming both settings, when the model is built and at
the call.  No kernel is launched here."""
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fi_fpn16_eligible", "fi_fpn16_topdown_grad_bf16", "fi_fpn16_topdown_grad_f16"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fi_fpn16.h")).read(), flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(fi_[a-z0-9_]+)\s*\(", _header())))


def test_library_builds_and_exports_every_declared_symbol():
    from feature_intertwiner_amd import build
    build.build_hip()
    path = build.FPN16_LIB_PATH
    assert os.path.exists(path)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    exported = set(re.findall(r" T (fi_[a-z0-9_]+)", nm))
    declared = _declared()
    assert declared == NAMES
    assert exported == set(declared), (sorted(exported), declared)
    assert b"gfx950" in open(path, "rb").read()


def test_the_twelve_other_libraries_gained_no_export():
    """The new entry points live in the new library alone, and no other header speaks of them."""
    from feature_intertwiner_amd import build
    build.build_hip()
    others = (build.LIB_PATH, build.EVAL_LIB_PATH, build.COCOEVAL_LIB_PATH, build.COCOMASK_LIB_PATH, build.OT_LIB_PATH,
              build.CONVT_LIB_PATH, build.ACT16_LIB_PATH, build.PYR16_LIB_PATH, build.ROI16_LIB_PATH, build.HEAD16_LIB_PATH,
              build.GRAD16_LIB_PATH, build.TRAIN16_LIB_PATH)
    assert len(set(others)) == 12 and build.FPN16_LIB_PATH not in others
    for path in others:
        nm = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert "fi_fpn16" not in nm, path
    for header in os.listdir(os.path.join(ROOT, "include")):
        if header != "fi_fpn16.h":
            assert "fi_fpn16" not in open(os.path.join(ROOT, "include", header)).read(), header


def test_the_header_names_no_other_16_bit_backward_library():
    """tests/test_grad16_host.py and tests/test_train16_host.py scan every other header for their prefixes."""
    text = open(os.path.join(ROOT, "include", "fi_fpn16.h")).read()
    for prefix in ("fi_grad" + "16", "fi_train" + "16"):
        assert prefix not in text


def test_ctypes_table_matches_the_header():
    from feature_intertwiner_amd import fpn16
    assert sorted(fpn16.SIGNATURES.keys()) == _declared()
    src = _header()
    for name, (res, args) in fpn16.SIGNATURES.items():
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1).split(",")
        assert len(params) == len(args), name
        assert res is fpn16.ctypes.c_int
        for p, a in zip(params, args):
            is_ptr = "*" in p or "fi_stream_t" in p
            assert (a is fpn16.ctypes.c_void_p) == is_ptr, (name, p.strip())
            assert is_ptr or a is fpn16.ctypes.c_int
    L = fpn16.load()
    assert L.fi_fpn16_eligible.restype is fpn16.ctypes.c_int


def test_eligibility_query_on_both_sides_of_every_rule():
    from feature_intertwiner_amd import fpn16
    el = fpn16.load().fi_fpn16_eligible
    none = (None, None, None, None)
    #          N, H, W, C, own, fine, g, colsum
    assert el(4, 32, 32, 256, 64, 128, 192, 260) == 1                 # p5 at 4 x 1024^2
    assert el(1, 1, 1, 8, *none) == 1                                 # smallest
    assert el(0, 1, 1, 8, *none) == 0 and el(-1, 1, 1, 8, *none) == 0
    assert el(1, 0, 1, 8, *none) == 0 and el(1, 1, 0, 8, *none) == 0
    assert el(1, 3, 5, 0, *none) == 0 and el(1, 3, 5, -8, *none) == 0
    for C, want in ((8, 1), (16, 1), (96, 1), (2088, 1), (4, 0), (12, 0), (100, 0), (2049, 0)):      # C % 8
        assert el(1, 3, 5, C, *none) == want, C
    # alignment: 16 bytes for each of the three 16-bit tensors ...
    for k in range(3):
        ptrs = [64, 128, 192, 256]
        assert el(1, 3, 5, 8, *ptrs) == 1
        ptrs[k] += 8
        assert el(1, 3, 5, 8, *ptrs) == 0, k
        ptrs[k] += 2 - 8
        assert el(1, 3, 5, 8, *ptrs) == 0, k
    # ... and 4 for the fp32 sums
    assert el(1, 3, 5, 8, 64, 128, 192, 260) == 1
    assert el(1, 3, 5, 8, 64, 128, 192, 262) == 0
    assert el(1, 3, 5, 8, 64, 128, 192, 257) == 0
    assert el(1, 3, 5, 8, 64, 128, 64, None) == 1                     # in place: g is own
    # N * 2H * 2W below 2^31
    assert el(1, 1 << 15, 1 << 14, 8, *none) == 0                     # 2^29 coarse pixels: 2^31 fine ones
    assert el(1, (1 << 15) - 1, 1 << 14, 8, *none) == 1
    assert el(2, 1 << 14, 1 << 13, 8, *none) == 1                     # 2^30 fine pixels
    assert el(8, 1 << 14, 1 << 13, 8, *none) == 0
    # the workgroup count: at most 512 coarse pixels and 2048 channels per workgroup
    assert el(1, 1 << 14, 1 << 14, 2048, *none) == 1                  # 2^19 row groups x 1 channel tile
    assert el(1, 1 << 14, 1 << 14, 2048 << 11, *none) == 1            # x 2^11
    assert el(1, 1 << 14, 1 << 14, 2048 << 12, *none) == 0            # x 2^12 = 2^31


@pytest.mark.parametrize("suffix", ["bf16", "f16"])
def test_argument_validation_without_a_gpu(suffix):
    """Invalid calls are rejected on the host before any HIP call: the statuses, and nothing launched (there is no GPU
    here -- a HIP call would answer FI_ERR_HIP, -2)."""
    from feature_intertwiner_amd import _lib, fpn16
    L = fpn16.load()
    last = _lib.load().fi_last_error
    names = ["own", "fine", "g", "colsum", "N", "H", "W", "C", "stream"]
    ok = (64, 128, 192, 256, 1, 4, 4, 32, None)
    fn = getattr(L, "fi_fpn16_topdown_grad_" + suffix)

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return fn(*a)

    assert call(g=None) == -1 and b"null" in last()
    assert call(own=None, fine=None) == -1 and b"both null" in last()
    assert call(N=-1) == -1
    assert call(H=0) == -1 and call(W=0) == -1 and call(C=0) == -1 and call(H=-3) == -1 and call(C=-8) == -1
    assert call(C=12) == -3 and b"C % 8" in last()
    assert call(C=4) == -3
    assert call(own=72) == -3 and call(fine=136) == -3 and call(g=200) == -3 and call(g=194) == -3
    assert call(colsum=258) == -3                                    # fp32: 4 bytes
    assert call(H=1 << 15, W=1 << 14) == -3                          # 2^31 fine pixels
    assert call(own=None, fine=None, g=None, colsum=None, N=0) == 0  # empty batch: nothing to launch


def test_python_layer_refuses_what_it_cannot_run():
    """The wrapper and both layers take GPU tensors only; pyr16's public functions keep refusing grad mode."""
    from feature_intertwiner_amd import _lib, fpn16, pyr16
    cl = torch.channels_last
    x = torch.zeros(1, 32, 4, 4, dtype=torch.bfloat16).contiguous(memory_format=cl)
    top = torch.zeros(1, 32, 2, 2, dtype=torch.bfloat16).contiguous(memory_format=cl)
    conv = torch.nn.Conv2d(32, 32, 1)
    with pytest.raises(_lib.FiError, match="GPU only"):
        fpn16.topdown_grad16(top, x)
    with pytest.raises(_lib.FiError, match="both None"):
        fpn16.topdown_grad16(None, None)
    with pytest.raises(_lib.FiError, match="GPU only"):
        fpn16.lateral16(x.requires_grad_(), conv, top)
    with pytest.raises(_lib.FiError, match="GPU only"):
        fpn16.conv_bias_act16(x, conv)
    with pytest.raises(_lib.FiError):
        pyr16.lateral16(x, conv, top)
    with pytest.raises(_lib.FiError):
        pyr16.conv_bias_act16(x, conv)
    fpn16.reset_stats()
    assert fpn16.stats() == {"topdown": 0, "sums": 0, "lateral": 0, "conv": 0, "top_to_autograd": 0, "weights": 0}


def _cfg():
    from feature_intertwiner_amd.config import make_config
    return make_config(backbone="resnet50", image_size=256, batch_size=2, train_rois_per_image=48)


def test_train_act_scope_is_absent_by_default_and_checked_when_the_model_is_built():
    from feature_intertwiner_amd import fpn16
    from feature_intertwiner_amd.model import MaskRCNN
    cfg = _cfg()
    assert not hasattr(cfg.TRAIN, "ACT_SCOPE")                       # make_config does not set it
    assert fpn16.train_scope(cfg) == "trunk"
    cfg.TRAIN.ACT_SCOPE = "trunk"
    assert fpn16.train_scope(cfg) == "trunk"                         # next to fp32 as well
    MaskRCNN(cfg)
    for prec in ("bf16", "fp16"):
        cfg.TRAIN.ACT_PRECISION = prec
        for scope in ("trunk", "pyramid"):
            cfg.TRAIN.ACT_SCOPE = scope
            assert fpn16.train_scope(cfg) == scope
    MaskRCNN(cfg)                                                    # 'pyramid' next to 'fp16' builds
    for bad in ("roi", "detect", "fpn", "", 1, None):
        cfg.TRAIN.ACT_SCOPE = bad
        with pytest.raises(ValueError, match=r"TRAIN\.ACT_SCOPE.*TRAIN\.ACT_PRECISION"):
            fpn16.train_scope(cfg)
        with pytest.raises(ValueError, match=r"TRAIN\.ACT_SCOPE.*TRAIN\.ACT_PRECISION"):
            MaskRCNN(cfg)


def test_pyramid_scope_needs_a_16_bit_train_act_precision():
    from feature_intertwiner_amd import fpn16
    from feature_intertwiner_amd.model import MaskRCNN
    cfg = _cfg()
    cfg.TRAIN.ACT_SCOPE = "pyramid"                                  # TRAIN.ACT_PRECISION absent: fp32
    with pytest.raises(ValueError, match=r"TRAIN\.ACT_SCOPE = 'pyramid' needs TRAIN\.ACT_PRECISION"):
        MaskRCNN(cfg)
    cfg.TRAIN.ACT_PRECISION = "fp32"
    with pytest.raises(ValueError, match=r"TRAIN\.ACT_SCOPE.*TRAIN\.ACT_PRECISION"):
        fpn16.train_scope(cfg)
    with pytest.raises(ValueError, match=r"TRAIN\.ACT_SCOPE.*TRAIN\.ACT_PRECISION"):
        MaskRCNN(cfg)
    # a 16-bit MODEL.ACT_PRECISION is another setting and does not carry it
    cfg.MODEL.ACT_PRECISION = "bf16"
    with pytest.raises(ValueError, match=r"TRAIN\.ACT_SCOPE.*TRAIN\.ACT_PRECISION"):
        MaskRCNN(cfg)


def test_the_scope_is_checked_again_at_the_call():
    """A configuration changed after the model was built: FPN.forward asks again, before anything runs."""
    from feature_intertwiner_amd.model import MaskRCNN
    cfg = _cfg()
    model = MaskRCNN(cfg)
    cfg.TRAIN.ACT_SCOPE = "pyramid"
    with pytest.raises(ValueError, match=r"TRAIN\.ACT_SCOPE.*TRAIN\.ACT_PRECISION"):
        model.fpn(torch.zeros(1, 3, 64, 64), mode="train")


def test_the_ot_loss_stays_refused_under_the_pyramid_scope():
    from feature_intertwiner_amd.model import MaskRCNN
    cfg = _cfg()
    cfg.TRAIN.FPN_OT_LOSS = True
    cfg.TRAIN.ACT_PRECISION = "bf16"
    cfg.TRAIN.ACT_SCOPE = "pyramid"
    with pytest.raises(NotImplementedError, match="FPN_OT_LOSS"):
        MaskRCNN(cfg)
