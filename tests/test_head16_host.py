"""CPU: libfi_head16.so (RoIAlign that writes 16-bit channels-last crops and the heads' fp32 1x1 output layer,
include/fi_head16.h) builds for gfx950, exports exactly what its header declares, answers its two eligibility queries on both
sides of every rule and validates its arguments on the host before any HIP call; MODEL.ACT_SCOPE accepts 'detect' next to a
16-bit MODEL.ACT_PRECISION, and a configuration 'detect' cannot run is refused when the model is built.  No kernel is
launched here."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fi_head16_crop_eligible", "fi_head16_out1x1_bf16", "fi_head16_out1x1_eligible", "fi_head16_out1x1_f16",
         "fi_head16_pyramid_crop_forward_bf16", "fi_head16_pyramid_crop_forward_f16"]
P, I = ctypes.c_void_p, ctypes.c_int


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fi_head16.h")).read(), flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(fi_[a-z0-9_]+)\s*\(", _header())))


def _table(*ptrs):
    return (P * len(ptrs))(*ptrs)


def test_library_builds_and_exports_every_declared_symbol():
    from feature_intertwiner_amd import build
    build.build_hip()
    path = build.HEAD16_LIB_PATH
    assert os.path.exists(path)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    exported = set(re.findall(r" T (fi_[a-z0-9_]+)", nm))
    declared = _declared()
    assert declared == NAMES
    assert exported == set(declared), (sorted(exported), declared)
    assert b"gfx950" in open(path, "rb").read()
    for other in (build.LIB_PATH, build.ACT16_LIB_PATH, build.PYR16_LIB_PATH, build.ROI16_LIB_PATH):
        assert "fi_head16" not in subprocess.check_output(["nm", "-D", "--defined-only", other], text=True), other


def test_shared_device_headers_are_dependencies_of_the_library():
    from feature_intertwiner_amd import build
    assert "crop_dev.h" in build.HEAD16_HEADERS and "conv_act16_dev.h" in build.HEAD16_HEADERS
    src = lambda name: open(os.path.join(build.CSRC, name)).read()
    assert '#include "crop_dev.h"' in src("head16_crop.hip") and "make_tap(" in src("head16_crop.hip")
    assert "struct Tap" not in src("head16_crop.hip")
    assert '#include "conv_act16_dev.h"' in src("head16_out.hip") and "conv_main_loop<" in src("head16_out.hip")
    assert "__shared__ float" not in src("head16_crop.hip")           # no LDS tile


def test_ctypes_table_matches_the_header():
    from feature_intertwiner_amd import head16
    assert sorted(head16.SIGNATURES.keys()) == _declared()
    src = _header()
    host_array = (ctypes.POINTER(P), ctypes.POINTER(I))
    for name, (res, args) in head16.SIGNATURES.items():
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1).split(",")
        assert len(params) == len(args), name
        assert res is I
        for p, a in zip(params, args):
            p = p.strip()
            if p.endswith("_host"):                       # host arrays: a typed pointer
                assert a is (host_array[0] if "void" in p else host_array[1]), (name, p)
            elif "*" in p or "fi_stream_t" in p:
                assert a is P, (name, p)
            elif p.startswith("float"):
                assert a is ctypes.c_float, (name, p)
            else:
                assert a is I, (name, p)
    L = head16.load()
    assert L.fi_head16_crop_eligible.restype is I
    head16.reset_stats()
    assert head16.stats() == {"crop": 0, "conv": 0, "out": 0, "weights": 0}


def test_crop_eligibility_on_both_sides_of_every_rule():
    from feature_intertwiner_amd import head16
    el = head16.load().fi_head16_crop_eligible
    #          num_levels, depth, crop_h, crop_w, table, crops
    assert el(4, 256, 7, 7, _table(64, 128, 192, 256), 512) == 1                 # the model's calls
    assert el(4, 256, 14, 14, _table(64, 128, 192, 256), 512) == 1
    assert el(1, 8, 1, 1, None, None) == 1                                       # smallest; NULL counts as aligned
    assert el(1, 8, 7, 7, _table(None), None) == 1
    assert el(1, 8, 7, 7, None, None) == 1                                       # depth 8 / 12 / 264 / 0 / 4 / 2056
    assert el(1, 12, 7, 7, None, None) == 0
    assert el(1, 264, 7, 7, None, None) == 1
    assert el(1, 0, 7, 7, None, None) == 0 and el(1, 4, 7, 7, None, None) == 0
    assert el(1, 2056, 7, 7, None, None) == 1                                    # more than 256 lanes' worth: chunks
    for k in range(4):                                                           # a misaligned map: each level at + 8 bytes
        ptrs = [64, 128, 192, 256]
        assert el(4, 8, 7, 7, _table(*ptrs), 512) == 1
        ptrs[k] += 8
        assert el(4, 8, 7, 7, _table(*ptrs), 512) == 0, k
    assert el(2, 8, 7, 7, _table(64, 128, 192 + 8), 512) == 1                    # ... only the first num_levels entries count
    assert el(1, 8, 7, 7, _table(64), 512 + 16) == 1                             # misaligned crops: 16 bytes, not 4 or 8
    assert el(1, 8, 7, 7, _table(64), 512 + 8) == 0
    assert el(1, 8, 7, 7, _table(64), 512 + 4) == 0
    assert el(1, 8, 15, 15, None, None) == 1                                     # no LDS tile: no bound on the bins ...
    assert el(1, 8, 64, 64, None, None) == 1
    assert el(1, 8, 3, 65, None, None) == 0 and el(1, 8, 65, 3, None, None) == 0     # ... but an axis holds 64 table entries
    assert el(1, 8, 0, 7, None, None) == 0 and el(1, 8, 7, 0, None, None) == 0
    assert el(0, 8, 7, 7, None, None) == 0 and el(8, 8, 7, 7, None, None) == 1 and el(9, 8, 7, 7, None, None) == 0


def test_out_eligibility_on_both_sides_of_every_rule():
    from feature_intertwiner_amd import head16
    el = head16.load().fi_head16_out1x1_eligible
    #          P, Cin, Cout, act, layout, n, H, W, x, w, y
    assert el(2000, 1024, 405, 0, 0, 0, 0, 0, 256, 512, 1028) == 1               # the box head's call (y 4-byte aligned)
    assert el(200 * 196 * 4, 256, 81, 1, 1, 200, 14, 14, 256, 512, 1028) == 1    # the mask head's
    for cout in (1, 64, 65, 405):                                                # any Cout >= 1
        assert el(128, 32, cout, 0, 0, 0, 0, 0, None, None, None) == 1, cout
    assert el(128, 32, 0, 0, 0, 0, 0, 0, None, None, None) == 0
    assert el(128, 32, 8, 0, 0, 0, 0, 0, None, None, None) == 1                  # Cin 32 / 48 / 0 / 96
    assert el(128, 48, 8, 0, 0, 0, 0, 0, None, None, None) == 0
    assert el(128, 0, 8, 0, 0, 0, 0, 0, None, None, None) == 0
    assert el(128, 96, 8, 0, 0, 0, 0, 0, None, None, None) == 1
    assert el(0, 32, 8, 0, 0, 0, 0, 0, None, None, None) == 0                    # P >= 1 (the entry point returns before)
    assert el(1, 32, 8, 0, 0, 0, 0, 0, None, None, None) == 1
    assert el(128, 32, 8, 2, 0, 0, 0, 0, None, None, None) == 0                  # the switches
    assert el(128, 32, 8, -1, 0, 0, 0, 0, None, None, None) == 0
    assert el(128, 32, 8, 1, 0, 0, 0, 0, None, None, None) == 1
    assert el(128, 32, 8, 0, 2, 1, 1, 32, None, None, None) == 0
    assert el(128, 32, 8, 0, 0, 0, 0, 0, 256 + 8, 512, 1024) == 0                # x / w 16 bytes, y 4
    assert el(128, 32, 8, 0, 0, 0, 0, 0, 256, 512 + 8, 1024) == 0
    assert el(128, 32, 8, 0, 0, 0, 0, 0, 256, 512, 1024 + 4) == 1
    assert el(128, 32, 8, 0, 0, 0, 0, 0, 256, 512, 1024 + 2) == 0
    assert el(3 * 3 * 5 * 4, 32, 8, 0, 1, 3, 3, 5, None, None, None) == 1        # layout 1: P == n H W 4
    assert el(3 * 3 * 5 * 4 + 4, 32, 8, 0, 1, 3, 3, 5, None, None, None) == 0
    assert el(3 * 3 * 5 * 4 - 1, 32, 8, 0, 1, 3, 3, 5, None, None, None) == 0
    assert el(3 * 3 * 5, 32, 8, 0, 1, 3, 3, 5, None, None, None) == 0
    assert el(180, 32, 8, 0, 1, 0, 3, 5, None, None, None) == 0 and el(180, 32, 8, 0, 1, 3, 0, 5, None, None, None) == 0
    assert el(4, 32, 8, 0, 1, 1, 1, 1, None, None, None) == 1
    assert el(4 * 65536, 32, 8, 0, 1, 1, 1, 65536, None, None, None) == 1        # the shuffle walk's W bound
    assert el(4 * 65537, 32, 8, 0, 1, 1, 1, 65537, None, None, None) == 0
    assert el(1 << 30, 32, 8, 0, 1, 1 << 20, 1 << 20, 1 << 20, None, None, None) == 0     # products past 2^63: no wrap
    assert el((1 << 31) - 1, 32, 64, 0, 0, 0, 0, 0, None, None, None) == 1       # extents and grid below 2^31
    assert el((1 << 31) - 1, 32, 1 << 20, 0, 0, 0, 0, 0, None, None, None) == 0  # 2^24 x 2^14 workgroups
    assert el(128, 1 << 16, 1 << 15, 0, 0, 0, 0, 0, None, None, None) == 0       # Cout * Cin = 2^31


@pytest.mark.parametrize("suffix", ["bf16", "f16"])
def test_crop_argument_validation_without_a_gpu(suffix):
    """Invalid calls are rejected on the host before any HIP call (the pointers are not device memory)."""
    from feature_intertwiner_amd import _lib, head16
    L = head16.load()
    last = _lib.load().fi_last_error
    fn = getattr(L, "fi_head16_pyramid_crop_forward_" + suffix)
    names = ["maps", "hs", "ws", "num_levels", "boxes", "box_ind", "level", "num_boxes", "batch", "depth", "crop_h", "crop_w",
             "extrap", "crops", "stream"]
    tab4 = lambda *p: _table(*(p + (0,) * 5))            # nine entries: a bad num_levels never reads past the array
    ints = lambda *v: (I * 9)(*(v + (4,) * (9 - len(v))))
    ok = (tab4(64, 128, 192, 256), ints(8, 4, 2, 1), ints(8, 4, 2, 1), 4, 1024, 2048, 4096, 3, 2, 8, 7, 7, 0.0, 8192, None)

    def c(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return fn(*a)

    assert c(maps=None) == -1 and b"null" in last()
    assert c(hs=None) == -1 and c(ws=None) == -1
    assert c(boxes=None) == -1 and c(box_ind=None) == -1 and c(crops=None) == -1
    assert c(num_boxes=-1) == -1
    assert c(depth=0) == -1 and c(crop_h=0) == -1 and c(crop_w=0) == -1 and c(batch=0) == -1
    assert c(depth=-8) == -1 and c(crop_h=-7) == -1 and c(batch=-1) == -1
    assert c(maps=tab4(64, 0, 192, 256)) == -1 and b"level entry" in last()      # a null map, an empty map
    assert c(hs=ints(8, 0, 2, 1)) == -1
    assert c(level=None) == -1 and b"level" in last()                            # level[] is needed with four maps ...
    assert c(depth=12) == -3 and b"depth % 8" in last()
    assert c(depth=4) == -3
    for k in range(4):
        p = [64, 128, 192, 256]
        p[k] += 8
        assert c(maps=tab4(*p)) == -3, k
    assert c(crops=8192 + 8) == -3
    assert c(crop_h=3, crop_w=65) == -3
    assert c(num_levels=0) == -3 and c(num_levels=9) == -3
    assert c(num_boxes=1 << 30, depth=256, crop_h=14, crop_w=14) == -3 and b"grid" in last()     # 2^30 boxes x 4 slabs
    assert c(num_boxes=0) == 0                                                    # no boxes: nothing to launch
    assert c(num_boxes=0, maps=None, hs=None, ws=None, boxes=None, box_ind=None, level=None, crops=None) == 0


@pytest.mark.parametrize("suffix", ["bf16", "f16"])
def test_out_argument_validation_without_a_gpu(suffix):
    from feature_intertwiner_amd import _lib, head16
    L = head16.load()
    last = _lib.load().fi_last_error
    fn = getattr(L, "fi_head16_out1x1_" + suffix)
    names = ["x", "w", "bias", "y", "P", "Cin", "Cout", "act", "layout", "n", "H", "W", "stream"]
    ok = (256, 512, 1024, 2048, 180, 32, 81, 1, 1, 3, 3, 5, None)

    def c(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return fn(*a)

    assert c(x=None) == -1 and b"null" in last()
    assert c(w=None) == -1 and c(y=None) == -1
    assert c(P=-1) == -1 and c(Cin=0) == -1 and c(Cout=0) == -1 and c(Cin=-32) == -1 and c(Cout=-1) == -1
    assert c(Cin=48) == -3 and b"Cin % 32" in last()
    assert c(x=256 + 8) == -3 and c(w=512 + 8) == -3 and c(y=2048 + 2) == -3
    assert c(act=2) == -3 and c(layout=2) == -3 and c(act=-1) == -3
    assert c(P=184) == -3 and c(n=0) == -3 and c(H=-3) == -3 and c(W=0) == -3     # layout 1: P == n H W 4
    assert c(P=0) == 0                                                            # no rows: nothing to launch
    assert c(P=0, x=None, w=None, bias=None, y=None) == 0


def test_python_layer_refuses_what_it_cannot_run():
    """The wrappers take 16-bit channels-last GPU tensors under no_grad; anything else is an error and counts nothing."""
    from feature_intertwiner_amd import _lib, head16
    import torch.nn as nn
    cl = lambda dtype: torch.zeros(1, 32, 4, 4, dtype=dtype).contiguous(memory_format=torch.channels_last)
    boxes, ind = torch.zeros(1, 4), torch.zeros(1, dtype=torch.int32)
    head16.reset_stats()
    conv, bn = nn.Conv2d(32, 32, 1), nn.BatchNorm2d(32).eval()
    with torch.no_grad():
        with pytest.raises(_lib.FiError):                 # a CPU tensor
            head16.pyramid_crop16_cl([cl(torch.bfloat16)], boxes, ind, None, 7, 7)
        with pytest.raises(_lib.FiError):                 # an fp32 map
            head16.pyramid_crop16_cl([cl(torch.float32)], boxes, ind, None, 7, 7)
        with pytest.raises(_lib.FiError):
            head16.pyramid_crop16_cl([], boxes, ind, None, 7, 7)
        for dtype in (torch.bfloat16, torch.float32):
            with pytest.raises(_lib.FiError):
                head16.out1x1_16(cl(dtype), torch.zeros(8, 32))
            with pytest.raises(_lib.FiError):
                head16.conv_bn_act16(cl(dtype), conv, bn)
            with pytest.raises(_lib.FiError):
                head16.window_bn_act16(cl(dtype), conv, bn)
            with pytest.raises(_lib.FiError):
                head16.deconv2x2_act16(cl(dtype), nn.ConvTranspose2d(32, 32, 2, 2))
    assert head16.stats() == {"crop": 0, "conv": 0, "out": 0, "weights": 0}


def test_python_layer_refuses_an_enabled_grad_mode():
    """Forward only: the grad-mode check comes first, so it shows on any tensor."""
    from feature_intertwiner_amd import _lib, head16
    import torch.nn as nn
    x = torch.zeros(1, 32, 4, 4, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    head16.reset_stats()
    with torch.enable_grad():
        with pytest.raises(_lib.FiError, match="no_grad"):
            head16.pyramid_crop16_cl([x], torch.zeros(1, 4), torch.zeros(1, dtype=torch.int32), None, 7, 7)
        with pytest.raises(_lib.FiError, match="no_grad"):
            head16.out1x1_16(x, torch.zeros(8, 32))
        with pytest.raises(_lib.FiError, match="no_grad"):
            head16.conv_bn_act16(x, nn.Conv2d(32, 32, 1), nn.BatchNorm2d(32).eval())
    assert head16.stats() == {"crop": 0, "conv": 0, "out": 0, "weights": 0}


def test_act_scope_accepts_detect_next_to_a_16bit_precision():
    from feature_intertwiner_amd import pyr16
    from feature_intertwiner_amd.config import make_config
    assert pyr16.SCOPES == ("trunk", "pyramid", "roi", "detect")
    cfg = make_config(backbone="resnet50", image_size=256, batch_size=2, train_rois_per_image=48)
    cfg.MODEL.ACT_SCOPE = "detect"                                    # ACT_PRECISION absent
    with pytest.raises(ValueError, match="ACT_SCOPE.*ACT_PRECISION"):
        pyr16.act_scope(cfg.MODEL)
    cfg.MODEL.ACT_PRECISION = "fp32"
    with pytest.raises(ValueError, match="ACT_SCOPE.*ACT_PRECISION"):
        pyr16.act_scope(cfg.MODEL)
    for prec in ("bf16", "fp16"):
        cfg.MODEL.ACT_PRECISION = prec
        assert pyr16.act_scope(cfg.MODEL) == "detect"
    cfg.MODEL.ACT_SCOPE = "heads"                                     # still no scope
    with pytest.raises(ValueError, match="ACT_SCOPE.*ACT_PRECISION"):
        pyr16.act_scope(cfg.MODEL)


def test_detect_scope_refuses_what_it_has_no_kernel_for():
    """Raised when the model is built, on the CPU: an error, not another path."""
    from feature_intertwiner_amd.config import make_config
    from feature_intertwiner_amd.model import MaskRCNN

    def cfg_detect(**kw):
        cfg = make_config(backbone="resnet50", image_size=256, batch_size=2, train_rois_per_image=48, **kw)
        cfg.MODEL.ACT_PRECISION = "bf16"
        cfg.MODEL.ACT_SCOPE = "detect"
        return cfg

    cfg = cfg_detect(dev_switch=True)
    assert not cfg.DEV.CLS_MERGE_FEAT                                 # the shipped default
    cfg.DEV.CLS_MERGE_FEAT = True
    with pytest.raises(NotImplementedError, match="DEV.CLS_MERGE_FEAT"):
        MaskRCNN(cfg)
    cfg.MODEL.ACT_SCOPE = "roi"                                       # the older scope runs the feature extractor in fp32
    MaskRCNN(cfg)
    cfg = cfg_detect(dev_switch=True)
    cfg.DEV.UPSAMPLE_FAC = 2.
    with pytest.raises(NotImplementedError, match="'detect'.*DEV.UPSAMPLE_FAC"):
        MaskRCNN(cfg)
    cfg = cfg_detect(dev_switch=True)
    cfg.ROIS.METHOD = "roi_pool"
    with pytest.raises(NotImplementedError, match="'detect'.*ROIS.METHOD"):
        MaskRCNN(cfg)
    model = MaskRCNN(cfg_detect(dev_switch=True))                     # what 'detect' runs builds
    with pytest.raises(NotImplementedError, match="training"):
        model([torch.zeros(2, 3, 256, 256), None, None, None], mode="train")
