"""CPU: libfi_crops16.so (the RPN's patch rows on 16-bit channels-last maps and the masked pack of RoIAlign's gradient,
include/fi_crops16.h) builds for gfx950, exports exactly what its header declares, answers the eligibility query on both
sides of its rules and validates its arguments on the host before any HIP call; TRAIN.ACT_SCOPE = 'crops' is accepted next
to a 16-bit TRAIN.ACT_PRECISION only, and every configuration the 16-bit route to the crops cannot carry is refused with an
error that names the setting, when the model is built or at the call.  No kernel is launched here."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fi_crops16_eligible", "fi_crops16_gate_pack_bf16", "fi_crops16_gate_pack_f16",
         "fi_crops16_patch_rows_backward_bf16", "fi_crops16_patch_rows_backward_f16",
         "fi_crops16_patch_rows_forward_bf16", "fi_crops16_patch_rows_forward_f16"]
PATCH_FWD, PATCH_BWD, GATE_PACK = 0, 1, 2


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fi_crops16.h")).read(), flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(fi_[a-z0-9_]+)\s*\(", _header())))


def test_library_builds_and_exports_every_declared_symbol():
    from feature_intertwiner_amd import build
    build.build_hip()
    path = build.CROPS16_LIB_PATH
    assert os.path.exists(path)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    exported = set(re.findall(r" T (fi_[a-z0-9_]+)", nm))
    declared = _declared()
    assert declared == NAMES
    assert exported == set(declared), (sorted(exported), declared)
    assert all(n.startswith("fi_crops16_") for n in exported)
    assert b"gfx950" in open(path, "rb").read()


def test_the_thirteen_other_libraries_and_headers_gained_nothing():
    """The new entry points live in the new library alone, no other header speaks of them, and the new header names no
    other 16-bit library's prefix (their host tests scan every header for theirs)."""
    from feature_intertwiner_amd import build
    build.build_hip()
    others = (build.LIB_PATH, build.EVAL_LIB_PATH, build.COCOEVAL_LIB_PATH, build.COCOMASK_LIB_PATH, build.OT_LIB_PATH,
              build.CONVT_LIB_PATH, build.ACT16_LIB_PATH, build.PYR16_LIB_PATH, build.ROI16_LIB_PATH, build.HEAD16_LIB_PATH,
              build.GRAD16_LIB_PATH, build.TRAIN16_LIB_PATH, build.FPN16_LIB_PATH)
    assert len(set(others)) == 13 and build.CROPS16_LIB_PATH not in others
    for path in others:
        nm = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert "fi_crops16" not in nm, path
    for header in os.listdir(os.path.join(ROOT, "include")):
        if header != "fi_crops16.h":
            assert "fi_crops16" not in open(os.path.join(ROOT, "include", header)).read(), header
    text = open(os.path.join(ROOT, "include", "fi_crops16.h")).read()
    for stem in ("act", "pyr", "grad", "train", "fpn", "roi", "head"):
        assert "fi_" + stem + "16" not in text, stem


def test_ctypes_table_matches_the_header():
    from feature_intertwiner_amd import crops16
    assert sorted(crops16.SIGNATURES.keys()) == _declared()
    src = _header()
    for name, (res, args) in crops16.SIGNATURES.items():
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1).split(",")
        assert len(params) == len(args), name
        assert res is ctypes.c_int
        for p, a in zip(params, args):
            is_ptr = "*" in p or "fi_stream_t" in p
            assert (a is ctypes.c_void_p) == is_ptr, (name, p.strip())
            assert is_ptr or a is ctypes.c_int
    L = crops16.load()
    assert L.fi_crops16_eligible.restype is ctypes.c_int
    kinds = dict(re.findall(r"#define FI_CROPS16_(\w+) (\d)", open(os.path.join(ROOT, "include", "fi_crops16.h")).read()))
    assert (int(kinds["PATCH_FWD"]), int(kinds["PATCH_BWD"]), int(kinds["GATE_PACK"])) == \
        (crops16.PATCH_FWD, crops16.PATCH_BWD, crops16.GATE_PACK) == (PATCH_FWD, PATCH_BWD, GATE_PACK)


def test_eligibility_query_on_both_sides_of_every_rule():
    from feature_intertwiner_amd import crops16
    el = crops16.load().fi_crops16_eligible
    none = (None, None, None, None)

    def table(n, value=64):
        return (ctypes.c_void_p * n)(*([value] * n))
    #          kind, levels, C, n, level_ptrs, p0, p1, p2, p3
    for kind in (PATCH_FWD, PATCH_BWD):
        assert el(kind, 5, 256, 512, table(5), 128, *none[1:]) == 1         # the RPN's rows of a 2-image step
        assert el(kind, 1, 8, 1, None, *none) == 1                          # smallest
        for C, want in ((8, 1), (16, 1), (2088, 1), (4, 0), (12, 0), (100, 0), (0, 0), (-8, 0)):
            assert el(kind, 4, C, 40, None, *none) == want, C
        assert el(kind, 8, 8, 40, table(8), *none) == 1                     # at most 8 levels
        assert el(kind, 9, 8, 40, table(9), *none) == 0
        assert el(kind, 9, 8, 40, None, *none) == 0 and el(kind, 0, 8, 40, None, *none) == 0
        ptrs = table(4)
        ptrs[2] = 72                                                        # one level 8 bytes off
        assert el(kind, 4, 8, 40, ptrs, *none) == 0
        ptrs[2] = 66
        assert el(kind, 4, 8, 40, ptrs, *none) == 0
        assert el(kind, 4, 8, 40, table(4), 128, *none[1:]) == 1
        assert el(kind, 4, 8, 40, table(4), 136, *none[1:]) == 0            # the fp32 rows: 16 bytes too
        assert el(kind, 4, 8, 0, None, *none) == 0 and el(kind, 4, 8, -1, None, *none) == 0
        assert el(kind, 4, 8, 1 << 20, None, *none) == 1 and el(kind, 4, 8, (1 << 20) + 1, None, *none) == 0
    assert el(GATE_PACK, 0, 256, 2 * 64 * 64, None, 64, 128, 192, 260) == 1
    assert el(GATE_PACK, 0, 8, 1, None, *none) == 1
    assert el(GATE_PACK, 0, 8, 0, None, *none) == 0
    for C, want in ((8, 1), (64, 1), (2088, 1), (4, 0), (12, 0), (100, 0)):
        assert el(GATE_PACK, 0, C, 35, None, *none) == want, C
    for k in range(3):                                                      # d, y, g: 16 bytes each
        ptrs = [64, 128, 192, 256]
        ptrs[k] += 8
        assert el(GATE_PACK, 0, 8, 35, None, *ptrs) == 0, k
        ptrs[k] += 2 - 8
        assert el(GATE_PACK, 0, 8, 35, None, *ptrs) == 0, k
    assert el(GATE_PACK, 0, 8, 35, None, 64, None, 192, 260) == 1           # no mask; the sums: 4 bytes
    assert el(GATE_PACK, 0, 8, 35, None, 64, None, 192, 262) == 0
    assert el(GATE_PACK, 0, 8, 35, None, 64, None, 192, None) == 1
    assert el(GATE_PACK, 0, 8, (1 << 31) - 1, None, *none) == 1
    assert el(3, 4, 8, 40, None, *none) == 0 and el(-1, 4, 8, 40, None, *none) == 0      # no such kind


@pytest.mark.parametrize("suffix", ["bf16", "f16"])
def test_argument_validation_without_a_gpu(suffix):
    """Invalid calls are rejected on the host before any HIP call: the statuses, and nothing launched (there is no GPU
    here -- a HIP call would answer FI_ERR_HIP, -2)."""
    from feature_intertwiner_amd import _lib, crops16
    L = crops16.load()
    last = _lib.load().fi_last_error
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    maps = (ctypes.c_void_p * 9)(64, 128, 128, 256, 320, 384, 448, 512, 576)   # levels 1 and 2 share a tensor
    names = ["maps", "heights", "widths", "steps", "levels", "per_loc", "image", "anchor", "rows", "N", "C", "out", "stream"]
    ok = (maps, ints(4, 2, 2), ints(6, 3, 3), ints(1, 1, 2), 3, 3, 1024, 2048, 4, 2, 8, 4096, None)
    fwd = getattr(L, "fi_crops16_patch_rows_forward_" + suffix)
    bwd = getattr(L, "fi_crops16_patch_rows_backward_" + suffix)

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        f = fwd(*a)
        b = bwd(a[11], *a[:11], None)                                # d first, no out
        assert f == b, (kw, f, b)
        return f

    assert call(rows=0) == 0                                         # nothing to launch
    assert call(rows=-1) == -1 and call(N=0) == -1 and call(C=0) == -1 and call(per_loc=0) == -1
    assert call(image=None) == -1 and b"null" in last()
    assert call(out=None) == -1
    assert call(levels=0) == -1 and call(levels=9, heights=ints(*[2] * 9), widths=ints(*[2] * 9), steps=None) == -1
    assert call(heights=ints(4, 0, 2)) == -1 and call(steps=ints(1, 0, 2)) == -1
    assert call(heights=ints(4, 2, 3)) == -1 and b"share a tensor" in last()      # one pointer, two sizes
    assert call(C=12) == -3 and b"C % 8" in last()
    assert call(out=4104) == -3
    bad = (ctypes.c_void_p * 3)(64, 72, 256)
    assert call(maps=bad, heights=ints(4, 2, 1), widths=ints(6, 3, 2)) == -3
    assert call(rows=(1 << 20) + 1) == -3

    gp = getattr(L, "fi_crops16_gate_pack_" + suffix)
    gnames = ["d", "y", "g", "sums", "N", "H", "W", "C", "stream"]
    gok = (64, 128, 192, 256, 1, 3, 3, 8, None)

    def gcall(**kw):
        a = list(gok)
        for k, v in kw.items():
            a[gnames.index(k)] = v
        return gp(*a)

    assert gcall(d=None) == -1 and b"null" in last()
    assert gcall(g=None) == -1
    assert gcall(N=-1) == -1 and gcall(H=0) == -1 and gcall(W=0) == -1 and gcall(C=0) == -1
    assert gcall(C=12) == -3 and b"C % 8" in last()
    assert gcall(d=72) == -3 and gcall(y=136) == -3 and gcall(g=194) == -3 and gcall(sums=258) == -3
    assert gcall(N=1 << 11, H=1 << 10, W=1 << 10) == -3              # 2^31 pixels
    assert gcall(d=None, y=None, g=None, sums=None, N=0) == 0        # empty batch, no sums: nothing to do


def test_python_layer_refuses_what_it_cannot_run():
    """A CPU tensor or a wrong layout raises FiError before any HIP call."""
    from feature_intertwiner_amd import _lib, crops16
    cl = torch.channels_last
    m = torch.zeros(1, 8, 4, 4, dtype=torch.bfloat16).contiguous(memory_format=cl)
    img, anc = torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(_lib.FiError, match="GPU only"):
        crops16.patch_rows16([m], img, anc, 3)
    with pytest.raises(_lib.FiError, match="GPU only"):
        crops16.patch_rows16([m.clone().requires_grad_()], img, anc, 3)
    with pytest.raises(_lib.FiError, match="GPU only"):
        crops16.patch_rows_grad16(torch.zeros(3, 72), [m], img, anc, 3)
    with pytest.raises(_lib.FiError, match="GPU only"):
        crops16.gate_pack16(torch.zeros(1, 8, 4, 4).contiguous(memory_format=cl), m)
    with pytest.raises(_lib.FiError, match="GPU only"):
        crops16.pyramid_crops16([m], [(torch.zeros(2, 4), torch.zeros(2, dtype=torch.int32),
                                       torch.full((2,), 2, dtype=torch.int32), 7)])
    with pytest.raises(_lib.FiError, match="no maps"):
        crops16.patch_rows16([], img, anc, 3)
    with pytest.raises(_lib.FiError, match="no maps or no crops"):
        crops16.pyramid_crops16([m], [])
    if torch.cuda.is_available():                                    # the layout checks come behind the device check
        dev = "cuda:0"
        nchw = torch.zeros(2, 8, 4, 4, dtype=torch.bfloat16, device=dev)
        fp32 = torch.zeros(2, 8, 4, 4, device=dev).contiguous(memory_format=cl)
        with pytest.raises(_lib.FiError, match="channels-last"):
            crops16.patch_rows16([nchw], img.to(dev), anc.to(dev), 3)
        with pytest.raises(_lib.FiError, match="channels-last"):
            crops16.patch_rows16([fp32], img.to(dev), anc.to(dev), 3)
        with pytest.raises(_lib.FiError, match="channels-last float32"):
            crops16.gate_pack16(torch.zeros(2, 8, 4, 4, device=dev), None, dtype=torch.bfloat16)
        with pytest.raises(_lib.FiError, match="one step"):
            crops16.patch_rows16([nchw.contiguous(memory_format=cl)], img.to(dev), anc.to(dev), 3, steps=[1, 2])
    crops16.reset_stats()
    assert crops16.stats() == {"patch_fwd": 0, "patch_bwd": 0, "gate_pack": 0, "crops": 0}


def _cfg():
    from feature_intertwiner_amd.config import make_config
    return make_config(backbone="resnet50", image_size=256, batch_size=2, train_rois_per_image=48)


def test_crops_scope_is_accepted_next_to_a_16_bit_precision_only():
    from feature_intertwiner_amd import fpn16
    from feature_intertwiner_amd.model import MaskRCNN
    cfg = _cfg()
    assert not hasattr(cfg.TRAIN, "ACT_SCOPE")                       # make_config does not set it
    for prec in ("bf16", "fp16"):
        cfg.TRAIN.ACT_PRECISION = prec
        cfg.TRAIN.ACT_SCOPE = "crops"
        assert fpn16.train_scope(cfg) == "crops"
        MaskRCNN(cfg)
    for prec in ("fp32", None):
        cfg = _cfg()
        cfg.TRAIN.ACT_SCOPE = "crops"
        if prec is not None:
            cfg.TRAIN.ACT_PRECISION = prec
        with pytest.raises(ValueError, match=r"TRAIN\.ACT_SCOPE.*TRAIN\.ACT_PRECISION"):
            fpn16.train_scope(cfg)
        with pytest.raises(ValueError, match=r"TRAIN\.ACT_SCOPE = 'crops' needs TRAIN\.ACT_PRECISION"):
            MaskRCNN(cfg)
    cfg.MODEL.ACT_PRECISION = "bf16"                                 # another setting: it does not carry the scope
    with pytest.raises(ValueError, match=r"TRAIN\.ACT_SCOPE.*TRAIN\.ACT_PRECISION"):
        MaskRCNN(cfg)


def _set(cfg, path, value):
    node, name = path.split(".")
    setattr(getattr(cfg, node), name, value)


@pytest.mark.parametrize("path,value,names", [
    ("DEV.SWITCH", False, r"DEV\.SWITCH"),
    ("DEV.UPSAMPLE_FAC", 2.0, r"DEV\.UPSAMPLE_FAC"),
    ("ROIS.METHOD", "roi_pool", r"ROIS\.METHOD"),
    ("DEV.BIG_FEAT_DETACH", False, r"DEV\.BIG_FEAT_DETACH"),
    ("DEV.BIG_SUPERVISE", True, r"DEV\.BIG_SUPERVISE"),
    ("RPN.ANCHOR_STRIDE", 2, r"RPN\.ANCHOR_STRIDE"),
])
def test_what_the_scope_cannot_carry_is_refused_when_the_model_is_built(path, value, names):
    from feature_intertwiner_amd import crops16
    from feature_intertwiner_amd.model import MaskRCNN
    cfg = _cfg()
    cfg.TRAIN.ACT_PRECISION = "bf16"
    _set(cfg, path, value)
    for scope in (None, "pyramid"):                                  # the other scopes build with it as before
        if scope is not None:
            cfg.TRAIN.ACT_SCOPE = scope
        crops16.check_config(cfg)
    if path != "DEV.BIG_SUPERVISE":
        MaskRCNN(cfg)
    cfg.TRAIN.ACT_SCOPE = "crops"
    with pytest.raises(NotImplementedError, match=r"TRAIN\.ACT_SCOPE = 'crops' needs.*" + names):
        crops16.check_config(cfg)
    with pytest.raises(NotImplementedError, match=r"TRAIN\.ACT_SCOPE = 'crops' needs.*" + names):
        MaskRCNN(cfg)


def test_the_ot_loss_stays_refused_under_the_crops_scope():
    from feature_intertwiner_amd import crops16
    from feature_intertwiner_amd.model import MaskRCNN
    cfg = _cfg()
    cfg.TRAIN.FPN_OT_LOSS = True
    cfg.TRAIN.ACT_PRECISION = "fp16"
    cfg.TRAIN.ACT_SCOPE = "crops"
    with pytest.raises(NotImplementedError, match=r"TRAIN\.ACT_SCOPE = 'crops' needs.*FPN_OT_LOSS"):
        crops16.check_config(cfg)
    with pytest.raises(NotImplementedError, match="FPN_OT_LOSS"):
        MaskRCNN(cfg)


def test_gates_off_is_refused_at_the_call(monkeypatch):
    """conv.GATES off: the dense RPN would need a graph, which has no 16-bit form.  The refusal names the setting."""
    from feature_intertwiner_amd import _lib, conv, crops16
    monkeypatch.setattr(conv, "GATES", False)
    with pytest.raises(_lib.FiError, match=r"TRAIN\.ACT_SCOPE = 'crops' needs conv\.GATES"):
        crops16.require_gates()
    monkeypatch.setattr(conv, "GATES", True)
    crops16.require_gates()
