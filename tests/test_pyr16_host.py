"""CPU: libfi_pyr16.so (the pyramid's lateral step and the RPN's stacked 1x1 heads on 16-bit channels-last tensors,
include/fi_pyr16.h) builds for gfx950, exports exactly what its header declares, answers both eligibility queries on both
sides of every rule and validates its arguments on the host before any HIP call; MODEL.ACT_SCOPE defaults to 'trunk' and
refuses what MODEL.ACT_PRECISION cannot carry.  No kernel is launched here."""
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fi_pyr16_head1x1_bf16", "fi_pyr16_head1x1_eligible", "fi_pyr16_head1x1_f16", "fi_pyr16_lateral_bf16",
         "fi_pyr16_lateral_eligible", "fi_pyr16_lateral_f16"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fi_pyr16.h")).read(), flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(fi_[a-z0-9_]+)\s*\(", _header())))


def test_library_builds_and_exports_every_declared_symbol():
    from feature_intertwiner_amd import build
    build.build_hip()
    path = build.PYR16_LIB_PATH
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
    for path in (build.LIB_PATH, build.CONVT_LIB_PATH, build.ACT16_LIB_PATH):
        nm = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert "fi_pyr16" not in nm, path
    for header in ("fi_capi.h", "fi_convt.h", "fi_act16.h"):
        assert "fi_pyr16" not in open(os.path.join(ROOT, "include", header)).read()


def test_ctypes_table_matches_the_header():
    from feature_intertwiner_amd import pyr16
    assert sorted(pyr16.SIGNATURES.keys()) == _declared()
    src = _header()
    for name, (res, args) in pyr16.SIGNATURES.items():
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1).split(",")
        assert len(params) == len(args), name
        assert res is pyr16.ctypes.c_int
        for p, a in zip(params, args):
            is_ptr = "*" in p or "fi_stream_t" in p
            assert (a is pyr16.ctypes.c_void_p) == is_ptr, (name, p.strip())
            assert is_ptr or a is pyr16.ctypes.c_int
    L = pyr16.load()
    assert L.fi_pyr16_lateral_eligible.restype is pyr16.ctypes.c_int
    pyr16.reset_stats()
    assert pyr16.stats() == {"lateral": 0, "head": 0}


def test_lateral_eligibility_on_both_sides_of_every_rule():
    from feature_intertwiner_amd import pyr16
    el = pyr16.load().fi_pyr16_lateral_eligible
    #          N, H, W, Cin, Cout, x, w, top, y
    assert el(2, 336, 336, 256, 256, 64, 128, 192, 256) == 1                     # P2's lateral at 2 x 1344^2
    assert el(1, 2, 2, 32, 8, None, None, None, None) == 1                       # smallest
    assert el(1, 3, 2, 32, 8, None, None, None, None) == 0                       # odd H
    assert el(1, 2, 3, 32, 8, None, None, None, None) == 0                       # odd W
    assert el(1, 0, 2, 32, 8, None, None, None, None) == 0                       # even, but below 2
    assert el(1, 2, 0, 32, 8, None, None, None, None) == 0
    assert el(1, 4, 6, 31, 8, None, None, None, None) == 0                       # Cin 31 / 32
    assert el(1, 4, 6, 32, 8, None, None, None, None) == 1
    assert el(1, 4, 6, 48, 8, None, None, None, None) == 0
    assert el(1, 4, 6, 0, 8, None, None, None, None) == 0
    assert el(1, 4, 6, 32, 7, None, None, None, None) == 0                       # Cout 7 / 8
    assert el(1, 4, 6, 32, 12, None, None, None, None) == 0
    assert el(1, 4, 6, 32, 0, None, None, None, None) == 0
    for k in range(4):                                                           # each pointer at + 8 bytes
        ptrs = [64, 128, 192, 256]
        assert el(1, 4, 6, 32, 8, *ptrs) == 1
        ptrs[k] += 8
        assert el(1, 4, 6, 32, 8, *ptrs) == 0, k
    assert el(0, 4, 6, 32, 8, None, None, None, None) == 0
    assert el(1, 1 << 16, 1 << 15, 32, 8, None, None, None, None) == 0           # 2^31 pixels
    assert el(1, 1 << 15, 1 << 15, 32, 8, None, None, None, None) == 1           # 2^30 pixels
    assert el(1, 2, 2, 1 << 16, 1 << 15, None, None, None, None) == 0            # 2^31 weights
    assert el(1, 2, 2, 1 << 15, 1 << 15, None, None, None, None) == 1


def test_head_eligibility_on_both_sides_of_every_rule():
    from feature_intertwiner_amd import pyr16
    el = pyr16.load().fi_pyr16_head1x1_eligible
    #          N, H, W, Cin, Cout, x, w, y
    assert el(2, 336, 336, 512, 18, 64, 128, 260) == 1                           # the RPN's heads on P2 at 2 x 1344^2
    assert el(1, 1, 1, 32, 1, None, None, None) == 1                             # smallest; odd maps are fine
    assert el(1, 3, 5, 32, 18, None, None, None) == 1
    assert el(1, 3, 5, 32, 0, None, None, None) == 0                             # Cout 0 / 1 / 64 / 65
    assert el(1, 3, 5, 32, 1, None, None, None) == 1
    assert el(1, 3, 5, 32, 64, None, None, None) == 1
    assert el(1, 3, 5, 32, 65, None, None, None) == 0
    assert el(1, 3, 5, 31, 18, None, None, None) == 0                            # Cin 31 / 32
    assert el(1, 3, 5, 32, 18, None, None, None) == 1
    assert el(1, 3, 5, 0, 18, None, None, None) == 0
    for k in range(2):                                                           # x and w at + 8 bytes
        ptrs = [64, 128, 256]
        assert el(1, 3, 5, 32, 18, *ptrs) == 1
        ptrs[k] += 8
        assert el(1, 3, 5, 32, 18, *ptrs) == 0, k
    assert el(1, 3, 5, 32, 18, 64, 128, 256 + 8) == 1                            # y: 4-byte alignment is all it needs
    assert el(1, 3, 5, 32, 18, 64, 128, 256 + 4) == 1
    assert el(1, 3, 5, 32, 18, 64, 128, 256 + 2) == 0
    assert el(0, 3, 5, 32, 18, None, None, None) == 0
    assert el(1, 0, 5, 32, 18, None, None, None) == 0
    assert el(1, 1 << 16, 1 << 15, 32, 18, None, None, None) == 0                # 2^31 pixels
    assert el(1, 1 << 15, 1 << 15, 32, 18, None, None, None) == 1


@pytest.mark.parametrize("suffix", ["bf16", "f16"])
def test_argument_validation_without_a_gpu(suffix):
    """Invalid calls are rejected on the host before any HIP call (the pointers are not device memory)."""
    from feature_intertwiner_amd import _lib, pyr16
    L = pyr16.load()
    last = _lib.load().fi_last_error
    lat = getattr(L, "fi_pyr16_lateral_" + suffix)
    names = ["x", "w", "bias", "top", "y", "N", "H", "W", "Cin", "Cout", "stream"]
    ok = (64, 128, None, 192, 256, 1, 4, 4, 32, 8, None)

    def call(fn, names, ok, **kw):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return fn(*a)

    c = lambda **kw: call(lat, names, ok, **kw)
    assert c(x=None) == -1 and b"null" in last()
    assert c(w=None) == -1 and c(top=None) == -1 and c(y=None) == -1
    assert c(N=-1) == -1
    assert c(H=0) == -1 and c(W=0) == -1 and c(Cin=0) == -1 and c(Cout=0) == -1
    assert c(H=3) == -3 and b"even" in last()
    assert c(W=5) == -3
    assert c(Cin=31) == -3 and c(Cin=48) == -3
    assert c(Cout=7) == -3 and c(Cout=12) == -3
    assert c(x=72) == -3 and c(w=136) == -3 and c(top=200) == -3 and c(y=264) == -3
    assert c(x=None, w=None, top=None, y=None, N=0) == 0              # empty batch: nothing to launch

    head = getattr(L, "fi_pyr16_head1x1_" + suffix)
    hnames = ["x", "w", "bias", "y", "N", "H", "W", "Cin", "Cout", "stream"]
    hok = (64, 128, None, 260, 1, 3, 5, 32, 18, None)
    h = lambda **kw: call(head, hnames, hok, **kw)
    assert h(x=None) == -1 and b"null" in last()
    assert h(w=None) == -1 and h(y=None) == -1
    assert h(N=-1) == -1
    assert h(H=0) == -1 and h(W=0) == -1 and h(Cin=0) == -1 and h(Cout=0) == -1
    assert h(Cout=65) == -3 and b"Cout <= 64" in last()
    assert h(Cin=31) == -3
    assert h(x=72) == -3 and h(w=136) == -3 and h(y=258) == -3
    assert h(x=None, w=None, y=None, N=0) == 0


def test_python_layer_refuses_what_it_cannot_run():
    """lateral16 / head1x1_16 / conv_bias_act16 take GPU tensors only; a CPU tensor is an error, never another path."""
    from feature_intertwiner_amd import _lib, pyr16
    from feature_intertwiner_amd.conv import Conv2d
    cl = lambda *shape: torch.zeros(*shape, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    conv = Conv2d(32, 8, kernel_size=1)
    with torch.no_grad():
        with pytest.raises(_lib.FiError):
            pyr16.lateral16(cl(1, 32, 2, 2), conv, cl(1, 8, 1, 1))
        with pytest.raises(_lib.FiError):
            pyr16.head1x1_16(cl(1, 32, 2, 2), conv.weight, conv.bias)
        with pytest.raises(_lib.FiError):
            pyr16.conv_bias_act16(cl(1, 32, 2, 2), conv)


def test_act_scope_defaults_to_trunk_and_needs_a_16bit_precision():
    from feature_intertwiner_amd import pyr16
    from feature_intertwiner_amd.config import make_config
    from feature_intertwiner_amd.model import MaskRCNN
    cfg = make_config(backbone="resnet50", image_size=256, batch_size=2, train_rois_per_image=48)
    assert getattr(cfg.MODEL, "ACT_SCOPE", "trunk") == "trunk"
    assert pyr16.act_scope(cfg.MODEL) == "trunk"
    cfg.MODEL.ACT_SCOPE = "pyramid"                                   # ACT_PRECISION absent
    with pytest.raises(ValueError, match="ACT_SCOPE.*ACT_PRECISION"):
        pyr16.act_scope(cfg.MODEL)
    with pytest.raises(ValueError, match="ACT_SCOPE.*ACT_PRECISION"):
        MaskRCNN(cfg)
    cfg.MODEL.ACT_PRECISION = "fp32"
    with pytest.raises(ValueError, match="ACT_SCOPE.*ACT_PRECISION"):
        pyr16.act_scope(cfg.MODEL)
    for prec in ("bf16", "fp16"):
        cfg.MODEL.ACT_PRECISION = prec
        assert pyr16.act_scope(cfg.MODEL) == "pyramid"
    cfg.MODEL.ACT_SCOPE = "heads"                                     # any other value
    with pytest.raises(ValueError, match="ACT_SCOPE.*ACT_PRECISION"):
        pyr16.act_scope(cfg.MODEL)
    cfg.MODEL.ACT_SCOPE = "pyramid"
    cfg.MODEL.ACT_PRECISION = "bf16"
    model = MaskRCNN(cfg)
    with pytest.raises(NotImplementedError, match="training"):
        model([torch.zeros(2, 3, 256, 256), None, None, None], mode="train")
    model.config.MODEL.ACT_SCOPE = "heads"                            # changed after construction: caught at the call
    with pytest.raises(ValueError, match="ACT_SCOPE"):
        model([torch.zeros(2, 3, 256, 256), None], mode="inference")
