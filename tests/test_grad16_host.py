"""CPU: libfi_grad16.so (the backward operators of a convolution on 16-bit channels-last tensors, include/fi_grad16.h)
builds for gfx950, exports exactly what its header declares, answers the eligibility query on both sides of every rule and
validates its arguments on the host before any HIP call.  No kernel is launched here."""
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fi_grad16_conv_dgrad_bf16", "fi_grad16_conv_dgrad_f16", "fi_grad16_conv_wgrad_bf16", "fi_grad16_conv_wgrad_f16",
         "fi_grad16_eligible", "fi_grad16_relu_grad_bf16", "fi_grad16_relu_grad_f16"]
RELU_GRAD, DGRAD, WGRAD = 0, 1, 2


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fi_grad16.h")).read(), flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(fi_[a-z0-9_]+)\s*\(", _header())))


def test_library_builds_and_exports_every_declared_symbol():
    from feature_intertwiner_amd import build
    build.build_hip()
    path = build.GRAD16_LIB_PATH
    assert os.path.exists(path)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    exported = set(re.findall(r" T (fi_[a-z0-9_]+)", nm))
    declared = _declared()
    assert declared == NAMES
    assert exported == set(declared), (sorted(exported), declared)
    assert b"gfx950" in open(path, "rb").read()


def test_the_ten_other_libraries_gained_no_export():
    """The new entry points live in the new library alone."""
    from feature_intertwiner_amd import build
    build.build_hip()
    others = (build.LIB_PATH, build.EVAL_LIB_PATH, build.COCOEVAL_LIB_PATH, build.COCOMASK_LIB_PATH, build.OT_LIB_PATH,
              build.CONVT_LIB_PATH, build.ACT16_LIB_PATH, build.PYR16_LIB_PATH, build.ROI16_LIB_PATH, build.HEAD16_LIB_PATH)
    assert len(set(others)) == 10 and build.GRAD16_LIB_PATH not in others
    for path in others:
        nm = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert "fi_grad16" not in nm, path
    for header in os.listdir(os.path.join(ROOT, "include")):
        if header != "fi_grad16.h":
            assert "fi_grad16" not in open(os.path.join(ROOT, "include", header)).read(), header


def test_ctypes_table_matches_the_header():
    from feature_intertwiner_amd import grad16
    assert sorted(grad16.SIGNATURES.keys()) == _declared()
    src = _header()
    for name, (res, args) in grad16.SIGNATURES.items():
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1).split(",")
        assert len(params) == len(args), name
        assert res is grad16.ctypes.c_int
        for p, a in zip(params, args):
            is_ptr = "*" in p or "fi_stream_t" in p
            assert (a is grad16.ctypes.c_void_p) == is_ptr, (name, p.strip())
            assert is_ptr or a is grad16.ctypes.c_int
    L = grad16.load()
    assert L.fi_grad16_eligible.restype is grad16.ctypes.c_int
    for kind, macro in ((grad16.RELU_GRAD, "FI_GRAD16_RELU_GRAD"), (grad16.DGRAD, "FI_GRAD16_DGRAD"),
                        (grad16.WGRAD, "FI_GRAD16_WGRAD")):
        assert re.search(r"#define %s %d\b" % (macro, kind), src), macro


@pytest.mark.parametrize("kind", [RELU_GRAD, DGRAD, WGRAD])
def test_eligibility_query_on_both_sides_of_every_rule(kind):
    from feature_intertwiner_amd import grad16
    el = grad16.load().fi_grad16_eligible
    none = (None, None, None, None)
    #          kind, N, H, W, Cin, Cout, R, S, stride, pad, p0, p1, p2, p3
    assert el(kind, 2, 336, 336, 64, 64, 1, 1, 1, 0, 64, 128, None, 256) == 1       # C2's conv1 at 2 x 1344^2
    assert el(kind, 1, 1, 1, 32, 32, 1, 1, 1, 0, *none) == 1                        # smallest
    assert el(kind, 1, 5, 7, 48, 32, 1, 1, 1, 0, *none) == 0                        # Cin % 32
    assert el(kind, 1, 5, 7, 0, 32, 1, 1, 1, 0, *none) == 0
    assert el(kind, 1, 5, 7, 32, 48, 1, 1, 1, 0, *none) == 0                        # Cout % 32
    assert el(kind, 1, 5, 7, 32, 8, 1, 1, 1, 0, *none) == 0
    assert el(kind, 1, 5, 7, 32, 0, 1, 1, 1, 0, *none) == 0
    assert el(kind, 1, 5, 7, 96, 160, 1, 1, 1, 0, *none) == 1                       # multiples of 32, not of 64
    # alignment: 16 bytes for a 16-bit tensor, 4 for an fp32 one (colsum, dw); WGRAD does not look at p2
    fp32_out = kind != DGRAD
    for k in range(4):
        ptrs = [64, 128, 192, 256]
        assert el(kind, 1, 5, 7, 32, 32, 1, 1, 1, 0, *ptrs) == 1
        ptrs[k] += 8
        refused = not ((k == 3 and fp32_out) or (k == 2 and kind == WGRAD))
        assert el(kind, 1, 5, 7, 32, 32, 1, 1, 1, 0, *ptrs) == (0 if refused else 1), k
        ptrs[k] += 2 - 8
        if not (k == 2 and kind == WGRAD):
            assert el(kind, 1, 5, 7, 32, 32, 1, 1, 1, 0, *ptrs) == 0, k
    assert el(kind, 1, 5, 7, 32, 32, 1, 1, 2, 0, *none) == 1                        # 1x1 stride 2
    assert el(kind, 1, 5, 7, 32, 32, 1, 1, 3, 0, *none) == 0
    assert el(kind, 1, 5, 7, 32, 32, 1, 1, 1, 1, *none) == 0                        # 1x1 takes no padding
    assert el(kind, 1, 5, 7, 32, 32, 3, 3, 1, 1, *none) == 1                        # 3x3 stride 1 pad 1
    assert el(kind, 1, 5, 7, 32, 32, 3, 3, 2, 1, *none) == 0                        # 3x3 stride 2
    assert el(kind, 1, 5, 7, 32, 32, 3, 3, 1, 0, *none) == 0                        # pad mismatch
    assert el(kind, 1, 5, 7, 32, 32, 3, 3, 1, 2, *none) == 0
    assert el(kind, 1, 9, 9, 32, 32, 5, 5, 1, 2, *none) == 0                        # 5x5
    assert el(kind, 1, 5, 7, 32, 32, 3, 1, 1, 1, *none) == 0                        # not square
    assert el(kind, 0, 5, 7, 32, 32, 1, 1, 1, 0, *none) == 0
    assert el(kind, 1, 0, 7, 32, 32, 1, 1, 1, 0, *none) == 0
    assert el(kind, 1, 5, 0, 32, 32, 1, 1, 1, 0, *none) == 0
    assert el(kind, 1, 1 << 16, 1 << 15, 32, 32, 1, 1, 1, 0, *none) == 0            # 2^31 pixels
    assert el(kind, 1, 1 << 15, 1 << 15, 32, 32, 1, 1, 1, 0, *none) == 1            # 2^30 pixels
    assert el(kind, 1, 5, 7, 1 << 15, 1 << 16, 1, 1, 1, 0, *none) == 0              # 2^31 weights
    assert el(kind, 1, 5, 7, 1 << 15, 1 << 15, 1, 1, 1, 0, *none) == 1


def test_eligibility_refuses_an_unknown_kind_and_covers_the_forward():
    """Every geometry the forward takes with Cin % 32 == 0 and Cout % 32 == 0 is taken by all three kinds."""
    from feature_intertwiner_amd import act16, grad16
    el = grad16.load().fi_grad16_eligible
    fwd = act16.load().fi_act16_conv_eligible
    none = (None, None, None, None)
    assert el(3, 1, 5, 7, 32, 32, 1, 1, 1, 0, *none) == 0 and el(-1, 1, 5, 7, 32, 32, 1, 1, 1, 0, *none) == 0
    for N, H, W in ((1, 1, 1), (2, 13, 11), (2, 336, 336), (4, 64, 64)):
        for Cin, Cout in ((32, 32), (64, 256), (96, 160), (1024, 2048), (2048, 512)):
            for R, stride, pad in ((1, 1, 0), (1, 2, 0), (3, 1, 1)):
                assert fwd(N, H, W, Cin, Cout, R, R, stride, pad, *none) == 1
                for kind in (RELU_GRAD, DGRAD, WGRAD):
                    assert el(kind, N, H, W, Cin, Cout, R, R, stride, pad, *none) == 1, (kind, N, H, W, Cin, Cout, R, stride)


def _caller(fn, names, ok):
    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return fn(*a)
    return call


@pytest.mark.parametrize("suffix", ["bf16", "f16"])
def test_argument_validation_without_a_gpu(suffix):
    """Invalid calls are rejected on the host before any HIP call: the statuses, and nothing launched (there is no GPU
    here -- a HIP call would answer FI_ERR_HIP, -2)."""
    from feature_intertwiner_amd import _lib, grad16
    L = grad16.load()
    last = _lib.load().fi_last_error

    relu = _caller(getattr(L, "fi_grad16_relu_grad_" + suffix),
                   ["dy", "y", "g", "colsum", "N", "OH", "OW", "Cout", "relu", "stream"],
                   (64, 128, 192, 256, 1, 4, 4, 32, 1, None))
    assert relu(dy=None) == -1 and b"null" in last()
    assert relu(g=None) == -1
    assert relu(y=None) == -1                                        # the mask needs y
    assert relu(N=-1) == -1 and relu(OH=0) == -1 and relu(OW=0) == -1 and relu(Cout=0) == -1
    assert relu(Cout=48) == -3 and b"Cout % 32" in last()
    assert relu(dy=72) == -3 and relu(y=136) == -3 and relu(g=200) == -3 and relu(colsum=258) == -3
    assert relu(OH=1 << 16, OW=1 << 15) == -3                         # 2^31 rows
    assert relu(dy=None, y=None, g=None, colsum=None, N=0) == 0      # empty batch: nothing to launch

    names = ["g", "wt", "dx_add", "dx", "N", "H", "W", "Cin", "Cout", "R", "S", "stride", "pad", "stream"]
    dgrad = _caller(getattr(L, "fi_grad16_conv_dgrad_" + suffix), names, (64, 128, None, 256, 1, 4, 4, 32, 32, 1, 1, 1, 0, None))
    assert dgrad(g=None) == -1 and b"null" in last()
    assert dgrad(wt=None) == -1 and dgrad(dx=None) == -1
    assert dgrad(N=-1) == -1
    assert dgrad(H=0) == -1 and dgrad(W=0) == -1 and dgrad(Cin=0) == -1 and dgrad(Cout=0) == -1
    assert dgrad(R=0) == -1 and dgrad(S=0) == -1 and dgrad(stride=0) == -1 and dgrad(pad=-1) == -1
    assert dgrad(Cin=48) == -3 and b"Cin % 32" in last()
    assert dgrad(Cout=48) == -3 and dgrad(Cout=8) == -3
    assert dgrad(g=72) == -3 and dgrad(wt=136) == -3 and dgrad(dx_add=8) == -3 and dgrad(dx=264) == -3
    assert dgrad(R=3, S=3, stride=2, pad=1) == -3
    assert dgrad(R=5, S=5, pad=2) == -3
    assert dgrad(R=3, S=3, pad=0) == -3
    assert dgrad(stride=3) == -3
    assert dgrad(g=None, wt=None, dx=None, N=0) == 0

    names = ["g", "x", "dw", "N", "H", "W", "Cin", "Cout", "R", "S", "stride", "pad", "stream"]
    wgrad = _caller(getattr(L, "fi_grad16_conv_wgrad_" + suffix), names, (64, 128, 256, 1, 4, 4, 32, 32, 1, 1, 1, 0, None))
    assert wgrad(g=None) == -1 and b"null" in last()
    assert wgrad(x=None) == -1 and wgrad(dw=None) == -1
    assert wgrad(N=-1) == -1
    assert wgrad(H=0) == -1 and wgrad(W=0) == -1 and wgrad(Cin=0) == -1 and wgrad(Cout=0) == -1
    assert wgrad(R=0) == -1 and wgrad(S=0) == -1 and wgrad(stride=0) == -1 and wgrad(pad=-1) == -1
    assert wgrad(Cin=48) == -3 and b"Cin % 32" in last()
    assert wgrad(Cout=48) == -3
    assert wgrad(g=72) == -3 and wgrad(x=136) == -3 and wgrad(dw=258) == -3
    assert wgrad(R=3, S=3, stride=2, pad=1) == -3
    assert wgrad(R=5, S=5, pad=2) == -3
    assert wgrad(R=3, S=3, pad=0) == -3
    assert wgrad(g=None, x=None, dw=None, N=0) == 0


def test_python_layer_refuses_what_it_cannot_run():
    """The wrappers and conv_bn_act16 take GPU tensors only, and an eval-mode BatchNorm; neither is another path."""
    from feature_intertwiner_amd import _lib, grad16
    cl = torch.channels_last
    x = torch.zeros(1, 32, 4, 4, dtype=torch.bfloat16).contiguous(memory_format=cl)
    conv = torch.nn.Conv2d(32, 32, 1, bias=False)
    bn = torch.nn.BatchNorm2d(32)
    bn.eval()
    with pytest.raises(_lib.FiError, match="GPU only"):
        grad16.conv_bn_act16(x.requires_grad_(), conv, bn)
    bn.train()
    with pytest.raises(_lib.FiError, match="training mode"):
        grad16.conv_bn_act16(x, conv, bn)
    with pytest.raises(_lib.FiError):
        grad16.relu_grad16(x, x)
    with pytest.raises(_lib.FiError):
        grad16.dgrad16(x, torch.zeros(32, 1, 1, 32, dtype=torch.bfloat16), (4, 4))
    with pytest.raises(_lib.FiError):
        grad16.wgrad16(x, x, 1, 1)
    grad16.reset_stats()
    assert grad16.stats() == {"relu_grad": 0, "dgrad": 0, "wgrad": 0, "weights": 0}


def test_training_the_model_on_16_bit_activations_is_still_refused():
    from feature_intertwiner_amd.config import make_config
    from feature_intertwiner_amd.model import MaskRCNN
    cfg = make_config(backbone="resnet50", image_size=256, batch_size=2, train_rois_per_image=48)
    cfg.MODEL.ACT_PRECISION = "bf16"
    model = MaskRCNN(cfg)
    with pytest.raises(NotImplementedError, match="training"):
        model([torch.zeros(2, 3, 256, 256), None, None, None], mode="train")
