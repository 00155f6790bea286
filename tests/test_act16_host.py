"""CPU: libfi_act16.so (convolutions on 16-bit channels-last activation tensors and the casts at their boundary,
include/fi_act16.h) builds for gfx950, exports exactly what its header declares, answers the eligibility query on both sides
of every rule and validates its arguments on the host before any HIP call.  No kernel is launched here."""
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fi_act16_conv_eligible", "fi_act16_conv_forward_bf16", "fi_act16_conv_forward_f16", "fi_act16_pack_bf16",
         "fi_act16_pack_f16", "fi_act16_unpack_bf16", "fi_act16_unpack_f16"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fi_act16.h")).read(), flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(fi_[a-z0-9_]+)\s*\(", _header())))


def test_library_builds_and_exports_every_declared_symbol():
    from feature_intertwiner_amd import build
    build.build_hip()
    path = build.ACT16_LIB_PATH
    assert os.path.exists(path)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    exported = set(re.findall(r" T (fi_[a-z0-9_]+)", nm))
    declared = _declared()
    assert declared == NAMES
    assert exported == set(declared), (sorted(exported), declared)
    assert b"gfx950" in open(path, "rb").read()


def test_the_other_libraries_gained_no_export():
    """The new entry points live in the new library alone."""
    from feature_intertwiner_amd import build
    build.build_hip()
    for path in (build.LIB_PATH, build.CONVT_LIB_PATH):
        nm = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert "fi_act16" not in nm, path
    for header in ("fi_capi.h", "fi_convt.h"):
        assert "fi_act16" not in open(os.path.join(ROOT, "include", header)).read()


def test_ctypes_table_matches_the_header():
    from feature_intertwiner_amd import act16
    assert sorted(act16.SIGNATURES.keys()) == _declared()
    src = _header()
    for name, (res, args) in act16.SIGNATURES.items():
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1).split(",")
        assert len(params) == len(args), name
        assert res is act16.ctypes.c_int
        for p, a in zip(params, args):
            is_ptr = "*" in p or "fi_stream_t" in p
            assert (a is act16.ctypes.c_void_p) == is_ptr, (name, p.strip())
            assert is_ptr or a is act16.ctypes.c_int
    L = act16.load()
    assert L.fi_act16_conv_eligible.restype is act16.ctypes.c_int


def test_eligibility_query_on_both_sides_of_every_rule():
    from feature_intertwiner_amd import act16
    el = act16.load().fi_act16_conv_eligible
    #          N, H, W, Cin, Cout, R, S, stride, pad, x, w, residual, y
    assert el(2, 336, 336, 64, 64, 1, 1, 1, 0, 64, 128, None, 256) == 1          # C2's conv1 at 2 x 1344^2
    assert el(1, 1, 1, 32, 8, 1, 1, 1, 0, None, None, None, None) == 1           # smallest
    assert el(1, 5, 7, 48, 8, 1, 1, 1, 0, None, None, None, None) == 0           # Cin % 32
    assert el(1, 5, 7, 0, 8, 1, 1, 1, 0, None, None, None, None) == 0
    assert el(1, 5, 7, 32, 12, 1, 1, 1, 0, None, None, None, None) == 0          # Cout % 8
    assert el(1, 5, 7, 32, 0, 1, 1, 1, 0, None, None, None, None) == 0
    for k in range(4):                                                           # each pointer at + 8 bytes
        ptrs = [64, 128, 192, 256]
        assert el(1, 5, 7, 32, 8, 1, 1, 1, 0, *ptrs) == 1
        ptrs[k] += 8
        assert el(1, 5, 7, 32, 8, 1, 1, 1, 0, *ptrs) == 0, k
    assert el(1, 5, 7, 32, 8, 1, 1, 2, 0, None, None, None, None) == 1           # 1x1 stride 2
    assert el(1, 5, 7, 32, 8, 1, 1, 3, 0, None, None, None, None) == 0
    assert el(1, 5, 7, 32, 8, 1, 1, 1, 1, None, None, None, None) == 0           # 1x1 takes no padding
    assert el(1, 5, 7, 32, 8, 3, 3, 1, 1, None, None, None, None) == 1           # 3x3 stride 1 pad 1
    assert el(1, 5, 7, 32, 8, 3, 3, 2, 1, None, None, None, None) == 0           # 3x3 stride 2
    assert el(1, 5, 7, 32, 8, 3, 3, 1, 0, None, None, None, None) == 0           # pad mismatch
    assert el(1, 5, 7, 32, 8, 3, 3, 1, 2, None, None, None, None) == 0
    assert el(1, 9, 9, 32, 8, 5, 5, 1, 2, None, None, None, None) == 0           # 5x5
    assert el(1, 5, 7, 32, 8, 3, 1, 1, 1, None, None, None, None) == 0           # not square
    assert el(0, 5, 7, 32, 8, 1, 1, 1, 0, None, None, None, None) == 0
    assert el(1, 0, 7, 32, 8, 1, 1, 1, 0, None, None, None, None) == 0
    assert el(1, 1 << 16, 1 << 15, 32, 8, 1, 1, 1, 0, None, None, None, None) == 0      # 2^31 pixels
    assert el(1, 1 << 15, 1 << 15, 32, 8, 1, 1, 1, 0, None, None, None, None) == 1      # 2^30 pixels


@pytest.mark.parametrize("suffix", ["bf16", "f16"])
def test_argument_validation_without_a_gpu(suffix):
    """Invalid calls are rejected on the host before any HIP call."""
    from feature_intertwiner_amd import _lib, act16
    L = act16.load()
    fwd = getattr(L, "fi_act16_conv_forward_" + suffix)
    last = _lib.load().fi_last_error
    #   x, w, scale, bias, residual, y, N, H, W, Cin, Cout, R, S, stride, pad, relu, stream
    ok = (64, 128, None, None, None, 256, 1, 4, 4, 32, 8, 1, 1, 1, 0, 0, None)

    def call(**kw):
        names = ["x", "w", "scale", "bias", "residual", "y", "N", "H", "W", "Cin", "Cout", "R", "S", "stride", "pad",
                 "relu", "stream"]
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return fwd(*a)

    assert call(x=None) == -1 and b"null" in last()
    assert call(w=None) == -1
    assert call(y=None) == -1
    assert call(N=-1) == -1
    assert call(H=0) == -1 and call(W=0) == -1 and call(Cin=0) == -1 and call(Cout=0) == -1
    assert call(R=0) == -1 and call(stride=0) == -1 and call(pad=-1) == -1
    assert call(Cin=48) == -3 and b"Cin % 32" in last()
    assert call(Cout=12) == -3
    assert call(y=264) == -3 and call(x=72) == -3 and call(w=136) == -3 and call(residual=8) == -3
    assert call(R=3, S=3, stride=2, pad=1) == -3
    assert call(R=5, S=5, pad=2) == -3
    assert call(R=3, S=3, pad=0) == -3
    assert call(x=None, w=None, y=None, N=0) == 0                    # empty batch: nothing to launch
    for stem in ("pack", "unpack"):
        cast = getattr(L, "fi_act16_%s_%s" % (stem, suffix))
        #   src, dst, N, C, H, W, stream
        assert cast(None, 64, 1, 8, 2, 2, None) == -1 and b"null" in last()
        assert cast(64, None, 1, 8, 2, 2, None) == -1
        assert cast(64, 128, -1, 8, 2, 2, None) == -1
        assert cast(64, 128, 1, 0, 2, 2, None) == -1 and cast(64, 128, 1, 8, 0, 2, None) == -1
        assert cast(64, 128, 1, 12, 2, 2, None) == -3 and b"C % 8" in last()
        p16 = (64, 136) if stem == "pack" else (136, 64)             # the 16-bit tensor at + 8 bytes
        assert cast(p16[0], p16[1], 1, 8, 2, 2, None) == -3
        assert cast(None, None, 0, 8, 2, 2, None) == 0


def test_python_layer_refuses_what_it_cannot_run():
    """pack / unpack / conv_bn_act16 take GPU tensors only; a CPU tensor is an error, never another path."""
    from feature_intertwiner_amd import _lib, act16
    with pytest.raises(_lib.FiError):
        act16.pack(torch.zeros(1, 8, 2, 2), torch.bfloat16)
    with pytest.raises(_lib.FiError):
        act16.unpack(torch.zeros(1, 8, 2, 2, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last))
    assert act16.dtype_of("bf16") is torch.bfloat16 and act16.dtype_of("fp16") is torch.float16
    with pytest.raises(ValueError):
        act16.dtype_of("fp8")
    act16.reset_stats()
    assert act16.stats() == {"conv": 0, "pack": 0, "unpack": 0}


def test_config_switch_defaults_to_fp32_and_training_is_refused():
    from feature_intertwiner_amd.config import make_config
    from feature_intertwiner_amd.model import MaskRCNN
    cfg = make_config(backbone="resnet50", image_size=256, batch_size=2, train_rois_per_image=48)
    assert getattr(cfg.MODEL, "ACT_PRECISION", "fp32") == "fp32"
    cfg.MODEL.ACT_PRECISION = "bf16"
    model = MaskRCNN(cfg)
    with pytest.raises(NotImplementedError, match="training"):
        model([torch.zeros(2, 3, 256, 256), None, None, None], mode="train")
