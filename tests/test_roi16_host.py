"""CPU: libfi_roi16.so (RoIAlign that reads 16-bit channels-last pyramid maps, include/fi_roi16.h) builds for gfx950, exports
exactly what its header declares, answers its eligibility query on both sides of every rule and validates its arguments on
the host before any HIP call; MODEL.ACT_SCOPE accepts 'roi' next to a 16-bit MODEL.ACT_PRECISION, and a configuration 'roi'
cannot run is refused when the model is built.  No kernel is launched here."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fi_roi16_crop_eligible", "fi_roi16_pyramid_crop_forward_bf16", "fi_roi16_pyramid_crop_forward_f16"]
P, I = ctypes.c_void_p, ctypes.c_int


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fi_roi16.h")).read(), flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(fi_[a-z0-9_]+)\s*\(", _header())))


def _table(*ptrs):
    return (P * len(ptrs))(*ptrs)


def test_library_builds_and_exports_every_declared_symbol():
    from feature_intertwiner_amd import build
    build.build_hip()
    path = build.ROI16_LIB_PATH
    assert os.path.exists(path)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    exported = set(re.findall(r" T (fi_[a-z0-9_]+)", nm))
    declared = _declared()
    assert declared == NAMES
    assert exported == set(declared), (sorted(exported), declared)
    assert b"gfx950" in open(path, "rb").read()
    for other in (build.LIB_PATH, build.ACT16_LIB_PATH, build.PYR16_LIB_PATH):     # the entry points live in the new library alone
        assert "fi_roi16" not in subprocess.check_output(["nm", "-D", "--defined-only", other], text=True), other


def test_shared_device_header_is_a_dependency_of_both_libraries():
    from feature_intertwiner_amd import build
    assert "crop_dev.h" in build.ROI16_HEADERS
    src = lambda name: open(os.path.join(build.CSRC, name)).read()
    assert '#include "crop_dev.h"' in src("crop_and_resize.hip")
    assert '#include "crop_dev.h"' in src("crop_roi16.hip")
    assert "struct Tap" not in src("crop_and_resize.hip") and "struct Tap" in src("crop_dev.h")


def test_ctypes_table_matches_the_header():
    from feature_intertwiner_amd import roi16
    assert sorted(roi16.SIGNATURES.keys()) == _declared()
    src = _header()
    host_array = (ctypes.POINTER(P), ctypes.POINTER(I))
    for name, (res, args) in roi16.SIGNATURES.items():
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
    L = roi16.load()
    assert L.fi_roi16_crop_eligible.restype is I
    roi16.reset_stats()
    assert roi16.stats() == {"crop": 0}


def test_eligibility_on_both_sides_of_every_rule():
    from feature_intertwiner_amd import roi16
    el = roi16.load().fi_roi16_crop_eligible
    #          num_levels, depth, crop_h, crop_w, table, crops
    assert el(4, 256, 7, 7, _table(64, 128, 192, 256), 260) == 1                 # the model's call
    assert el(4, 256, 14, 14, _table(64, 128, 192, 256), 260) == 1
    assert el(1, 8, 1, 1, None, None) == 1                                       # smallest; NULL counts as aligned
    assert el(1, 8, 7, 7, _table(None), None) == 1
    assert el(1, 8, 7, 7, None, None) == 1                                       # depth 8 / 12 / 0 / 4
    assert el(1, 12, 7, 7, None, None) == 0
    assert el(1, 0, 7, 7, None, None) == 0
    assert el(1, 4, 7, 7, None, None) == 0
    assert el(1, 264, 7, 7, None, None) == 1
    for k in range(4):                                                           # each level at + 8 bytes
        ptrs = [64, 128, 192, 256]
        assert el(4, 8, 7, 7, _table(*ptrs), 512) == 1
        ptrs[k] += 8
        assert el(4, 8, 7, 7, _table(*ptrs), 512) == 0, k
    assert el(2, 8, 7, 7, _table(64, 128, 192 + 8), 512) == 1                    # ... only the first num_levels entries count
    assert el(1, 8, 7, 7, _table(64), 512 + 4) == 1                              # crops: 4-byte alignment is all it needs
    assert el(1, 8, 7, 7, _table(64), 512 + 8) == 1
    assert el(1, 8, 7, 7, _table(64), 512 + 2) == 0
    assert el(1, 8, 10, 22, None, None) == 1                                     # crop_h * crop_w 220 / 221
    assert el(1, 8, 13, 17, None, None) == 0
    assert el(1, 8, 14, 15, None, None) == 1                                     # 210 / 225
    assert el(1, 8, 15, 15, None, None) == 0
    assert el(1, 8, 0, 7, None, None) == 0 and el(1, 8, 7, 0, None, None) == 0   # crop_h, crop_w >= 1
    assert el(1, 8, 3, 64, None, None) == 1                                      # an axis holds 64 table entries
    assert el(1, 8, 3, 65, None, None) == 0 and el(1, 8, 65, 3, None, None) == 0
    assert el(0, 8, 7, 7, None, None) == 0                                       # num_levels 0 / 1 / 8 / 9
    assert el(1, 8, 7, 7, None, None) == 1
    assert el(8, 8, 7, 7, None, None) == 1
    assert el(9, 8, 7, 7, None, None) == 0


@pytest.mark.parametrize("suffix", ["bf16", "f16"])
def test_argument_validation_without_a_gpu(suffix):
    """Invalid calls are rejected on the host before any HIP call (the pointers are not device memory)."""
    from feature_intertwiner_amd import _lib, roi16
    L = roi16.load()
    last = _lib.load().fi_last_error
    fn = getattr(L, "fi_roi16_pyramid_crop_forward_" + suffix)
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
    assert c(maps=tab4(64, 0, 192, 256)) == -1 and b"level entry" in last()      # a null map, an empty map
    assert c(hs=ints(8, 0, 2, 1)) == -1
    assert c(level=None) == -1 and b"level" in last()                            # level[] is needed with four maps ...
    assert c(depth=12) == -3 and b"depth % 8" in last()
    assert c(depth=4) == -3
    for k in range(4):
        p = [64, 128, 192, 256]
        p[k] += 8
        assert c(maps=tab4(*p)) == -3, k
    assert c(crops=8192 + 2) == -3
    assert c(crop_h=13, crop_w=17) == -3 and c(crop_h=15, crop_w=15) == -3
    assert c(crop_h=3, crop_w=65) == -3
    assert c(num_levels=0) == -3 and c(num_levels=9) == -3
    assert c(num_boxes=1 << 30, depth=256, crop_h=14, crop_w=14) == -3 and b"grid" in last()     # 2^30 boxes x 4 chunks
    assert c(num_boxes=0) == 0                                                    # no boxes: nothing to launch
    assert c(num_boxes=0, maps=None, hs=None, ws=None, boxes=None, box_ind=None, level=None, crops=None) == 0


def test_python_layer_refuses_what_it_cannot_run():
    """pyramid_crop16 takes 16-bit channels-last GPU tensors of one dtype under no_grad; anything else is an error."""
    from feature_intertwiner_amd import _lib, roi16
    cl = lambda dtype: torch.zeros(1, 8, 4, 4, dtype=dtype).contiguous(memory_format=torch.channels_last)
    boxes, ind = torch.zeros(1, 4), torch.zeros(1, dtype=torch.int32)
    with torch.no_grad():
        with pytest.raises(_lib.FiError):                 # a CPU tensor
            roi16.pyramid_crop16([cl(torch.bfloat16)], boxes, ind, None, 7, 7)
        with pytest.raises(_lib.FiError):                 # an fp32 map
            roi16.pyramid_crop16([cl(torch.float32)], boxes, ind, None, 7, 7)
        with pytest.raises(_lib.FiError):
            roi16.pyramid_crop16([], boxes, ind, None, 7, 7)
    assert roi16.stats()["crop"] == 0


def test_act_scope_accepts_roi_next_to_a_16bit_precision():
    from feature_intertwiner_amd import pyr16
    from feature_intertwiner_amd.config import make_config
    cfg = make_config(backbone="resnet50", image_size=256, batch_size=2, train_rois_per_image=48)
    cfg.MODEL.ACT_SCOPE = "roi"                                       # ACT_PRECISION absent
    with pytest.raises(ValueError, match="ACT_SCOPE.*ACT_PRECISION"):
        pyr16.act_scope(cfg.MODEL)
    cfg.MODEL.ACT_PRECISION = "fp32"
    with pytest.raises(ValueError, match="ACT_SCOPE.*ACT_PRECISION"):
        pyr16.act_scope(cfg.MODEL)
    for prec in ("bf16", "fp16"):
        cfg.MODEL.ACT_PRECISION = prec
        assert pyr16.act_scope(cfg.MODEL) == "roi"
    cfg.MODEL.ACT_SCOPE = "heads"                                     # still no scope
    with pytest.raises(ValueError, match="ACT_SCOPE.*ACT_PRECISION"):
        pyr16.act_scope(cfg.MODEL)


def test_roi_scope_refuses_what_it_has_no_kernel_for():
    """Raised when the model is built, on the CPU: an error, not another path."""
    from feature_intertwiner_amd.config import make_config
    from feature_intertwiner_amd.model import MaskRCNN
    from feature_intertwiner_amd.sub_module import Dev

    def cfg_roi(**kw):
        cfg = make_config(backbone="resnet50", image_size=256, batch_size=2, train_rois_per_image=48, **kw)
        cfg.MODEL.ACT_PRECISION = "bf16"
        cfg.MODEL.ACT_SCOPE = "roi"
        return cfg

    cfg = cfg_roi(dev_switch=True)
    Dev(cfg, depth=256)                                               # what 'roi' runs builds
    cfg.ROIS.METHOD = "roi_pool"
    with pytest.raises(NotImplementedError, match="ROIS.METHOD"):
        Dev(cfg, depth=256)
    with pytest.raises(NotImplementedError, match="ROIS.METHOD"):
        MaskRCNN(cfg)
    cfg = cfg_roi(dev_switch=True)
    cfg.DEV.UPSAMPLE_FAC = 2.
    with pytest.raises(NotImplementedError, match="DEV.UPSAMPLE_FAC"):
        Dev(cfg, depth=256)
    with pytest.raises(NotImplementedError, match="DEV.UPSAMPLE_FAC"):
        MaskRCNN(cfg)
    cfg.MODEL.ACT_SCOPE = "pyramid"                                   # the older scope unpacks in front of the Dev stage
    Dev(cfg, depth=256)
    model = MaskRCNN(cfg_roi(dev_switch=True))
    with pytest.raises(NotImplementedError, match="training"):
        model([torch.zeros(2, 3, 256, 256), None, None, None], mode="train")
