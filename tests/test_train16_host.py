"""CPU: libfi_train16.so (the gated data gradient with column sums on 16-bit channels-last tensors,
include/fi_train16.h) builds for gfx950, exports exactly what its header declares, answers the eligibility query on both
sides of every rule and validates its arguments on the host before any HIP call; TRAIN.ACT_PRECISION is absent by default, a value that is
none of 'fp32' / 'bf16' / 'fp16' is a ValueError and a 16-bit one with TRAIN.FPN_OT_LOSS a NotImplementedError when the
model is built.  No kernel is launched here."""
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fi_train16_conv_dgrad_gated_bf16", "fi_train16_conv_dgrad_gated_f16", "fi_train16_eligible"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fi_train16.h")).read(), flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(fi_[a-z0-9_]+)\s*\(", _header())))


def test_library_builds_and_exports_every_declared_symbol():
    from feature_intertwiner_amd import build
    build.build_hip()
    path = build.TRAIN16_LIB_PATH
    assert os.path.exists(path)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    exported = set(re.findall(r" T (fi_[a-z0-9_]+)", nm))
    declared = _declared()
    assert declared == NAMES
    assert exported == set(declared), (sorted(exported), declared)
    assert b"gfx950" in open(path, "rb").read()


def test_the_eleven_other_libraries_gained_no_export():
    """The new entry points live in the new library alone."""
    from feature_intertwiner_amd import build
    build.build_hip()
    others = (build.LIB_PATH, build.EVAL_LIB_PATH, build.COCOEVAL_LIB_PATH, build.COCOMASK_LIB_PATH, build.OT_LIB_PATH,
              build.CONVT_LIB_PATH, build.ACT16_LIB_PATH, build.PYR16_LIB_PATH, build.ROI16_LIB_PATH, build.HEAD16_LIB_PATH,
              build.GRAD16_LIB_PATH)
    assert len(set(others)) == 11 and build.TRAIN16_LIB_PATH not in others
    for path in others:
        nm = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert "fi_train16" not in nm, path
    for header in os.listdir(os.path.join(ROOT, "include")):
        if header != "fi_train16.h":
            assert "fi_train16" not in open(os.path.join(ROOT, "include", header)).read(), header


def test_ctypes_table_matches_the_header():
    from feature_intertwiner_amd import train16
    assert sorted(train16.SIGNATURES.keys()) == _declared()
    src = _header()
    for name, (res, args) in train16.SIGNATURES.items():
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1).split(",")
        assert len(params) == len(args), name
        assert res is train16.ctypes.c_int
        for p, a in zip(params, args):
            is_ptr = "*" in p or "fi_stream_t" in p
            assert (a is train16.ctypes.c_void_p) == is_ptr, (name, p.strip())
            assert is_ptr or a is train16.ctypes.c_int
    L = train16.load()
    assert L.fi_train16_eligible.restype is train16.ctypes.c_int


def test_eligibility_query_on_both_sides_of_every_rule():
    from feature_intertwiner_amd import train16
    el = train16.load().fi_train16_eligible
    none = (None, None, None, None)
    #          N, H, W, Cin, Cout, R, S, stride, pad, g, gate, dx_add, dx
    assert el(2, 336, 336, 64, 64, 1, 1, 1, 0, 64, 128, None, 256) == 1             # C2's conv1 at 2 x 1344^2
    assert el(1, 1, 1, 32, 32, 1, 1, 1, 0, *none) == 1                              # smallest
    assert el(1, 5, 7, 48, 32, 1, 1, 1, 0, *none) == 0                              # Cin % 32
    assert el(1, 5, 7, 0, 32, 1, 1, 1, 0, *none) == 0
    assert el(1, 5, 7, 32, 48, 1, 1, 1, 0, *none) == 0                              # Cout % 32
    assert el(1, 5, 7, 32, 8, 1, 1, 1, 0, *none) == 0
    assert el(1, 5, 7, 32, 0, 1, 1, 1, 0, *none) == 0
    assert el(1, 5, 7, 96, 160, 1, 1, 1, 0, *none) == 1                             # multiples of 32, not of 64
    # alignment: 16 bytes for each of the four 16-bit tensors, the gate included
    for k in range(4):
        ptrs = [64, 128, 192, 256]
        assert el(1, 5, 7, 32, 32, 1, 1, 1, 0, *ptrs) == 1
        ptrs[k] += 8
        assert el(1, 5, 7, 32, 32, 1, 1, 1, 0, *ptrs) == 0, k
        ptrs[k] += 2 - 8
        assert el(1, 5, 7, 32, 32, 1, 1, 1, 0, *ptrs) == 0, k
    assert el(1, 5, 7, 32, 32, 1, 1, 2, 0, *none) == 1                              # 1x1 stride 2
    assert el(1, 5, 7, 32, 32, 1, 1, 3, 0, *none) == 0
    assert el(1, 5, 7, 32, 32, 1, 1, 1, 1, *none) == 0                              # 1x1 takes no padding
    assert el(1, 5, 7, 32, 32, 3, 3, 1, 1, *none) == 1                              # 3x3 stride 1 pad 1
    assert el(1, 5, 7, 32, 32, 3, 3, 2, 1, *none) == 0                              # 3x3 stride 2
    assert el(1, 5, 7, 32, 32, 3, 3, 1, 0, *none) == 0                              # pad mismatch
    assert el(1, 5, 7, 32, 32, 3, 3, 1, 2, *none) == 0
    assert el(1, 9, 9, 32, 32, 5, 5, 1, 2, *none) == 0                              # 5x5
    assert el(1, 5, 7, 32, 32, 3, 1, 1, 1, *none) == 0                              # not square
    assert el(0, 5, 7, 32, 32, 1, 1, 1, 0, *none) == 0
    assert el(1, 0, 7, 32, 32, 1, 1, 1, 0, *none) == 0
    assert el(1, 5, 0, 32, 32, 1, 1, 1, 0, *none) == 0
    assert el(1, 1 << 16, 1 << 15, 32, 32, 1, 1, 1, 0, *none) == 0                  # 2^31 pixels
    assert el(1, 1 << 15, 1 << 15, 32, 32, 1, 1, 1, 0, *none) == 1                  # 2^30 pixels
    assert el(1, 5, 7, 1 << 15, 1 << 16, 1, 1, 1, 0, *none) == 0                    # 2^31 weights
    assert el(1, 5, 7, 1 << 15, 1 << 15, 1, 1, 1, 0, *none) == 1


def test_eligibility_is_the_ungated_data_gradient_s():
    """The same answer as fi_grad16_eligible(FI_GRAD16_DGRAD) on every geometry of the forward's table and around it."""
    from feature_intertwiner_amd import grad16, train16
    el = train16.load().fi_train16_eligible
    ref = grad16.load().fi_grad16_eligible
    none = (None, None, None, None)
    for N, H, W in ((1, 1, 1), (2, 13, 11), (2, 336, 336), (4, 64, 64)):
        for Cin, Cout in ((32, 32), (64, 256), (96, 160), (1024, 2048), (2048, 512), (48, 32), (32, 40)):
            for R, stride, pad in ((1, 1, 0), (1, 2, 0), (3, 1, 1), (3, 2, 1), (5, 1, 2)):
                geom = (N, H, W, Cin, Cout, R, R, stride, pad)
                assert el(*geom, *none) == ref(grad16.DGRAD, *geom, *none), geom


@pytest.mark.parametrize("suffix", ["bf16", "f16"])
def test_argument_validation_without_a_gpu(suffix):
    """Invalid calls are rejected on the host before any HIP call: the statuses, and nothing launched (there is no GPU
    here -- a HIP call would answer FI_ERR_HIP, -2)."""
    from feature_intertwiner_amd import _lib, train16
    L = train16.load()
    last = _lib.load().fi_last_error
    names = ["g", "wt", "dx_add", "gate", "dx", "colsum", "N", "H", "W", "Cin", "Cout", "R", "S", "stride", "pad", "stream"]
    ok = (64, 128, None, 192, 256, 320, 1, 4, 4, 32, 32, 1, 1, 1, 0, None)
    fn = getattr(L, "fi_train16_conv_dgrad_gated_" + suffix)

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return fn(*a)

    assert call(g=None) == -1 and b"null" in last()
    assert call(wt=None) == -1 and call(gate=None) == -1 and call(dx=None) == -1
    assert call(N=-1) == -1
    assert call(H=0) == -1 and call(W=0) == -1 and call(Cin=0) == -1 and call(Cout=0) == -1
    assert call(R=0) == -1 and call(S=0) == -1 and call(stride=0) == -1 and call(pad=-1) == -1
    assert call(Cin=48) == -3 and b"Cin % 32" in last()
    assert call(Cout=48) == -3 and call(Cout=8) == -3
    assert call(g=72) == -3 and call(wt=136) == -3 and call(dx_add=8) == -3 and call(gate=200) == -3 and call(dx=264) == -3
    assert call(colsum=322) == -3                                    # fp32: 4 bytes
    assert call(R=3, S=3, stride=2, pad=1) == -3
    assert call(R=5, S=5, pad=2) == -3
    assert call(R=3, S=3, pad=0) == -3
    assert call(stride=3) == -3
    assert call(H=1 << 16, W=1 << 15) == -3                          # 2^31 pixels
    assert call(g=None, wt=None, gate=None, dx=None, colsum=None, N=0) == 0      # empty batch: nothing to launch


def test_python_layer_refuses_what_it_cannot_run():
    """conv_bn_act16 and the wrapper take GPU tensors only, and an eval-mode BatchNorm; neither is another path."""
    from feature_intertwiner_amd import _lib, act16, grad16, train16
    cl = torch.channels_last
    x = torch.zeros(1, 32, 4, 4, dtype=torch.bfloat16).contiguous(memory_format=cl)
    conv = torch.nn.Conv2d(32, 32, 1, bias=False)
    bn = torch.nn.BatchNorm2d(32)
    bn.eval()
    with pytest.raises(_lib.FiError, match="GPU only"):
        train16.conv_bn_act16(x.requires_grad_(), conv, bn)
    bn.train()
    with pytest.raises(_lib.FiError, match="training mode"):
        train16.conv_bn_act16(x, conv, bn)
    with pytest.raises(_lib.FiError):
        train16.dgrad_gated16(x, torch.zeros(32, 1, 1, 32, dtype=torch.bfloat16), x, (4, 4))
    train16.reset_stats()
    assert train16.stats() == {"gated": 0, "premasked": 0, "fallback": 0, "pack": 0, "unpack": 0}
    # the earlier modules keep their counters: a gated launch is counted here, not there
    assert sorted(grad16.stats()) == ["dgrad", "relu_grad", "weights", "wgrad"]
    assert sorted(act16.stats()) == ["conv", "pack", "unpack"]


def _cfg():
    from feature_intertwiner_amd.config import make_config
    return make_config(backbone="resnet50", image_size=256, batch_size=2, train_rois_per_image=48)


def test_train_act_precision_is_absent_by_default_and_checked_when_the_model_is_built():
    from feature_intertwiner_amd import train16
    from feature_intertwiner_amd.model import MaskRCNN
    cfg = _cfg()
    assert not hasattr(cfg.TRAIN, "ACT_PRECISION")                   # make_config does not set it
    assert train16.act_precision(cfg) == "fp32"
    for good in ("fp32", "bf16", "fp16"):
        cfg.TRAIN.ACT_PRECISION = good
        assert train16.act_precision(cfg) == good
    MaskRCNN(cfg)                                                    # 'fp16' builds
    for bad in ("fp8", "half", 16, None):
        cfg.TRAIN.ACT_PRECISION = bad
        with pytest.raises(ValueError, match="ACT_PRECISION"):
            MaskRCNN(cfg)


def test_16_bit_training_with_the_ot_loss_is_refused_when_the_model_is_built():
    from feature_intertwiner_amd.model import MaskRCNN
    cfg = _cfg()
    cfg.TRAIN.FPN_OT_LOSS = True
    cfg.TRAIN.ACT_PRECISION = "fp32"
    MaskRCNN(cfg)
    cfg.TRAIN.ACT_PRECISION = "bf16"
    with pytest.raises(NotImplementedError, match="FPN_OT_LOSS"):
        MaskRCNN(cfg)


def test_model_act_precision_still_refuses_training():
    """MODEL.ACT_PRECISION stays an inference setting, with or without a 16-bit TRAIN.ACT_PRECISION next to it.  The
    case without one pins behaviour that predates TRAIN.ACT_PRECISION (it held before); the case with one is new."""
    from feature_intertwiner_amd.model import MaskRCNN
    for tact in (None, "bf16"):
        cfg = _cfg()
        cfg.MODEL.ACT_PRECISION = "bf16"
        if tact is not None:
            cfg.TRAIN.ACT_PRECISION = tact
        model = MaskRCNN(cfg)
        with pytest.raises(NotImplementedError, match="training"):
            model([torch.zeros(2, 3, 256, 256), None, None, None], mode="train")
