"""CPU: libfi_heads16.so (RoIAlign's backward from 16-bit channels-last crop gradients and the backward of the mask head's
class-selected output layer, include/fi_heads16.h) builds for gfx950, exports exactly what its header declares, answers the
eligibility query on both sides of its rules and validates its arguments on the host before any HIP call.  No kernel is
launched here."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fi_heads16_class_rows_backward_bf16", "fi_heads16_class_rows_backward_f16", "fi_heads16_eligible",
         "fi_heads16_pyramid_crop_backward_bf16", "fi_heads16_pyramid_crop_backward_f16"]
CROP_BWD, CLASS_ROWS = 0, 1


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fi_heads16.h")).read(), flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(fi_[a-z0-9_]+)\s*\(", _header())))


def test_library_builds_and_exports_every_declared_symbol():
    from feature_intertwiner_amd import build
    build.build_hip()
    path = build.HEADS16_LIB_PATH
    assert os.path.exists(path)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    exported = set(re.findall(r" T (fi_[a-z0-9_]+)", nm))
    declared = _declared()
    assert declared == NAMES
    assert exported == set(declared), (sorted(exported), declared)
    assert b"gfx950" in open(path, "rb").read()


def test_the_fourteen_other_libraries_and_headers_gained_nothing():
    from feature_intertwiner_amd import build
    build.build_hip()
    others = (build.LIB_PATH, build.EVAL_LIB_PATH, build.COCOEVAL_LIB_PATH, build.COCOMASK_LIB_PATH, build.OT_LIB_PATH,
              build.CONVT_LIB_PATH, build.ACT16_LIB_PATH, build.PYR16_LIB_PATH, build.ROI16_LIB_PATH, build.HEAD16_LIB_PATH,
              build.GRAD16_LIB_PATH, build.TRAIN16_LIB_PATH, build.FPN16_LIB_PATH, build.CROPS16_LIB_PATH)
    assert len(set(others)) == 14 and build.HEADS16_LIB_PATH not in others
    for path in others:
        nm = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert "fi_heads16" not in nm, path
    for header in os.listdir(os.path.join(ROOT, "include")):
        if header != "fi_heads16.h":
            assert "fi_heads16" not in open(os.path.join(ROOT, "include", header)).read(), header


def test_ctypes_table_matches_the_header():
    from feature_intertwiner_amd import heads16
    assert sorted(heads16.SIGNATURES.keys()) == _declared()
    src = _header()
    for name, (res, args) in heads16.SIGNATURES.items():
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1).split(",")
        assert len(params) == len(args), name
        assert res is ctypes.c_int
        for p, a in zip(params, args):
            is_ptr = "*" in p or "fi_stream_t" in p
            assert (a is ctypes.c_void_p) == is_ptr, (name, p.strip())
            assert is_ptr or a is ctypes.c_int
    heads16.load()
    kinds = dict(re.findall(r"#define FI_HEADS16_(\w+) (\d)", open(os.path.join(ROOT, "include", "fi_heads16.h")).read()))
    assert (int(kinds["CROP_BWD"]), int(kinds["CLASS_ROWS"])) == (heads16.CROP_BWD, heads16.CLASS_ROWS) == \
        (CROP_BWD, CLASS_ROWS)
    heads16.reset_stats()
    assert heads16.stats() == {"crop_bwd": 0, "class_rows": 0, "crops": 0}


def test_eligibility_query_on_both_sides_of_every_rule():
    from feature_intertwiner_amd import heads16
    el = heads16.load().fi_heads16_eligible
    none = (None, None, None, None)

    def table(n, value=64):
        return (ctypes.c_void_p * n)(*([value] * n))
    #  kind, m, C, h, w, n, f32_ptrs, p0, p1, p2, p3
    assert el(CROP_BWD, 4, 256, 14, 14, 2048, table(4), 128, *none[1:]) == 1
    assert el(CROP_BWD, 1, 8, 1, 1, 1, None, *none) == 1                      # smallest
    for C, want in ((8, 1), (72, 1), (264, 1), (1 << 20, 1), ((1 << 20) + 8, 0), (4, 0), (12, 0), (0, 0), (-8, 0)):
        assert el(CROP_BWD, 4, C, 7, 7, 40, None, *none) == want, C
    for h, w, want in ((64, 64, 1), (65, 7, 0), (7, 65, 0), (0, 7, 0), (7, 0, 0)):
        assert el(CROP_BWD, 4, 8, h, w, 40, None, *none) == want, (h, w)
    assert el(CROP_BWD, 8, 8, 7, 7, 40, table(8), *none) == 1 and el(CROP_BWD, 9, 8, 7, 7, 40, None, *none) == 0
    assert el(CROP_BWD, 0, 8, 7, 7, 40, None, *none) == 0
    ptrs = table(4)
    ptrs[2] = 68                                                              # the maps: 4 bytes
    assert el(CROP_BWD, 4, 8, 7, 7, 40, ptrs, *none) == 1
    ptrs[2] = 66
    assert el(CROP_BWD, 4, 8, 7, 7, 40, ptrs, *none) == 0
    assert el(CROP_BWD, 4, 8, 7, 7, 40, None, 136, *none[1:]) == 0            # grads: 16 bytes
    assert el(CROP_BWD, 4, 8, 7, 7, 0, None, *none) == 0 and el(CROP_BWD, 4, 8, 7, 7, -1, None, *none) == 0
    top = (1 << 31) - 1
    assert el(CROP_BWD, 4, 8, 7, 7, top, None, *none) == 1                    # one slab per box
    assert el(CROP_BWD, 4, 8, 14, 14, top // 4, None, *none) == 1 and el(CROP_BWD, 4, 8, 14, 14, top // 4 + 1, None, *none) == 0

    assert el(CLASS_ROWS, 81, 256, 14, 14, 512, table(3), 64, 128, 192, 260) == 1
    assert el(CLASS_ROWS, 1, 8, 1, 1, 1, None, *none) == 1
    assert el(CLASS_ROWS, 300, 8, 1, 1, 1, None, *none) == 1 and el(CLASS_ROWS, 100000, 8, 1, 1, 1, None, *none) == 1   # any K
    assert el(CLASS_ROWS, 0, 8, 1, 1, 1, None, *none) == 0
    for C, want in ((8, 1), (72, 1), (256, 1), (2088, 1), (4, 0), (12, 0), (100, 0)):
        assert el(CLASS_ROWS, 3, C, 3, 2, 5, None, *none) == want, C
    assert el(CLASS_ROWS, 3, 8, 1 << 14, 1 << 14, 1, None, *none) == 1 and el(CLASS_ROWS, 3, 8, 1 << 14, (1 << 14) + 1, 1, None, *none) == 0
    assert el(CLASS_ROWS, 3, 8, 3, 2, 0, None, *none) == 0
    for k in range(3):                                                        # u, w, du: 16 bytes each
        p = [64, 128, 192, 256]
        p[k] += 8
        assert el(CLASS_ROWS, 3, 8, 3, 2, 5, None, *p) == 0, k
    assert el(CLASS_ROWS, 3, 8, 3, 2, 5, None, 64, 128, 192, 260) == 1 and el(CLASS_ROWS, 3, 8, 3, 2, 5, None, 64, 128, 192, 262) == 0
    for k in range(3):                                                        # colsum, dweight, dbias: 4 bytes, or absent
        f = table(3)
        f[k] = 70
        assert el(CLASS_ROWS, 3, 8, 3, 2, 5, f, *none) == 0, k
        f[k] = None
        assert el(CLASS_ROWS, 3, 8, 3, 2, 5, f, *none) == 1, k
    assert el(2, 4, 8, 7, 7, 40, None, *none) == 0 and el(-1, 4, 8, 7, 7, 40, None, *none) == 0      # no such kind


@pytest.mark.parametrize("suffix", ["bf16", "f16"])
def test_argument_validation_without_a_gpu(suffix):
    """Invalid calls are rejected on the host before any HIP call: the statuses, and nothing launched or cleared (there is
    no GPU here -- a HIP call would answer FI_ERR_HIP, -2)."""
    from feature_intertwiner_amd import _lib, heads16
    L = heads16.load()
    last = _lib.load().fi_last_error
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    crop = getattr(L, "fi_heads16_pyramid_crop_backward_" + suffix)
    names = ["grads", "maps", "hs", "ws", "levels", "boxes", "box_ind", "level", "n", "batch", "depth", "ch", "cw", "acc",
             "stream"]
    ok = (1024, (ctypes.c_void_p * 2)(64, 128), ints(8, 4), ints(8, 4), 2, 2048, 4096, 8192, 3, 2, 8, 7, 7, 1, None)

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return crop(*a)

    assert call(n=0) == 0                                            # accumulate and no boxes: nothing to do
    assert call(n=-1) == -1 and call(batch=0) == -1 and call(depth=0) == -1 and call(ch=0) == -1 and call(cw=0) == -1
    assert call(grads=None) == -1 and b"null" in last()
    assert call(boxes=None) == -1 and call(box_ind=None) == -1 and call(maps=None) == -1
    assert call(level=None) == -1 and b"level" in last()
    assert call(levels=0) == -1 and call(levels=9) == -1
    assert call(hs=ints(8, 0)) == -1
    assert call(depth=12) == -3 and b"depth % 8" in last()
    assert call(grads=1032) == -3 and call(ch=65) == -3
    assert call(maps=(ctypes.c_void_p * 2)(64, 130)) == -3
    assert call(depth=12, acc=0) == -3                               # refused before the maps are cleared

    rows = getattr(L, "fi_heads16_class_rows_backward_" + suffix)
    rnames = ["d", "u", "w", "cls", "du", "colsum", "dweight", "dbias", "n", "H", "W", "C", "K", "stream"]
    rok = (64, 128, 256, 512, 1024, None, 2048, 4096, 2, 3, 2, 8, 5, None)

    def rcall(**kw):
        a = list(rok)
        for k, v in kw.items():
            a[rnames.index(k)] = v
        return rows(*a)

    assert rcall(n=0) == 0                                           # no RoIs, no column sums: nothing to do
    assert rcall(n=-1) == -1 and rcall(H=0) == -1 and rcall(W=0) == -1 and rcall(C=0) == -1 and rcall(K=0) == -1
    for k in ("d", "u", "w", "cls", "du"):
        assert rcall(**{k: None}) == -1 and b"null" in last(), k
    assert rcall(C=12) == -3 and b"C % 8" in last()
    assert rcall(u=136) == -3 and rcall(w=264) == -3 and rcall(du=1032) == -3 and rcall(d=66) == -3
    assert rcall(dweight=2050) == -3 and rcall(dbias=4098) == -3 and rcall(colsum=70, C=12) == -3


def test_python_layer_refuses_what_it_cannot_run():
    """CPU tensors and empty map lists are errors of the wrappers, raised before any library call; there is no fallback."""
    import torch
    from feature_intertwiner_amd import _lib, heads16
    cl = torch.channels_last
    d16 = torch.zeros(1, 8, 7, 7, dtype=torch.bfloat16).contiguous(memory_format=cl)
    buf = torch.zeros(1, 8, 4, 4).contiguous(memory_format=cl)
    boxes, ind = torch.zeros(1, 4), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(_lib.FiError, match="GPU only"):
        heads16.crop_backward16(d16, [buf], boxes, ind, None, 7, accumulate=False)
    with pytest.raises(_lib.FiError, match="no maps"):
        heads16.crop_backward16(d16, [], boxes, ind, None, 7, accumulate=False)
    with pytest.raises(_lib.FiError, match="GPU only"):
        heads16.class_rows_grad16(torch.zeros(1, 2, 2, 3, 2), torch.zeros(1, 32, 3, 2, dtype=torch.bfloat16).contiguous(memory_format=cl),
                                  torch.zeros(5, 8, dtype=torch.bfloat16), torch.zeros(1, dtype=torch.int64))
    spec = (boxes, ind, ind, 7)
    with pytest.raises(_lib.FiError, match="no maps"):
        heads16.pyramid_crops_heads16([], spec, spec, None, spec)
    with pytest.raises(_lib.FiError, match="GPU only"):
        heads16.pyramid_crops_heads16([d16], spec, spec, None, spec)


def test_heads_scope_is_accepted_next_to_a_16_bit_precision_and_refuses_by_name():
    """TRAIN.ACT_SCOPE = 'heads': accepted by fpn16.train_scope next to a 16-bit TRAIN.ACT_PRECISION only; heads16.check_config
    refuses, when the model is built, everything 'crops' refuses and DEV.CLS_MERGE_FEAT; conv.GATES off is an error at the
    call."""
    from feature_intertwiner_amd import _lib, conv, fpn16, heads16
    from feature_intertwiner_amd.config import make_config
    from feature_intertwiner_amd.model import MaskRCNN
    cfg = make_config("resnet50", 256, 2, 64, dev_switch=True, loss_choice="l2")
    cfg.TRAIN.ACT_SCOPE = "heads"
    with pytest.raises(ValueError, match=r"TRAIN\.ACT_SCOPE = 'heads' needs TRAIN\.ACT_PRECISION"):
        MaskRCNN(cfg)
    for prec in ("bf16", "fp16"):
        cfg.TRAIN.ACT_PRECISION = prec
        assert fpn16.train_scope(cfg) == "heads"
        heads16.check_config(cfg)
    MaskRCNN(cfg)
    cfg.DEV.CLS_MERGE_FEAT = True
    with pytest.raises(NotImplementedError, match=r"TRAIN\.ACT_SCOPE = 'heads' needs DEV\.CLS_MERGE_FEAT"):
        MaskRCNN(cfg)
    cfg.TRAIN.ACT_SCOPE = "crops"
    heads16.check_config(cfg)                                        # another scope: nothing to check
    cfg.TRAIN.ACT_SCOPE, cfg.DEV.CLS_MERGE_FEAT = "heads", False
    for name, value, pattern in (("UPSAMPLE_FAC", 2., "UPSAMPLE_FAC"), ("BIG_SUPERVISE", True, "BIG_SUPERVISE")):
        old = getattr(cfg.DEV, name)
        setattr(cfg.DEV, name, value)
        with pytest.raises(NotImplementedError, match=r"TRAIN\.ACT_SCOPE = 'heads' needs.*" + pattern):
            heads16.check_config(cfg)
        setattr(cfg.DEV, name, old)
    assert conv.GATES
    conv.GATES = False
    try:
        with pytest.raises(_lib.FiError, match=r"TRAIN\.ACT_SCOPE = 'heads' needs conv\.GATES"):
            heads16.require_gates()
    finally:
        conv.GATES = True
    heads16.require_gates()
