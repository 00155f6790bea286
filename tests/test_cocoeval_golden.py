"""CPU: the NumPy restatement of the COCO evaluation (tests/cocoeval_ref.py) equals the golden made from the
reference's own COCO / COCOeval / maskApi.c (scripts/gen_golden_cocoeval.py) bit for bit; `rle_from_string` inverts
the strings of the unmold golden; libfi_cocoeval.so exports what its header declares and validates its arguments."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cocoeval_ref as R
from cocoeval_cases import LARGE, cocoeval_cases, inputs_sha256

CASES = {c["name"]: c for c in cocoeval_cases()}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "cocoeval.npz"))


def test_inputs_regenerate(golden):
    assert str(golden["inputs_sha256"]) == inputs_sha256(list(CASES.values())), "RNG drift: regenerate the golden"
    assert list(golden["cases"]) == list(CASES) and list(golden["decided"]) == ["empty"]
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "cocoeval.npz")) <= 676 * 1024
    assert float(golden["large/bbox/reference_seconds"]) > 0


@pytest.mark.parametrize("case,iou_type", [(n, t) for n, c in CASES.items() for t in c["types"]])
def test_restatement_equals_golden(golden, case, iou_type):
    got = R.evaluate_case(CASES[case], iou_type)
    R.assert_equal_golden(got, golden, "%s/%s/" % (case, iou_type), large=case == LARGE)


def test_golden_covers_the_issue_cases(golden):
    g = golden
    assert g["ties/bbox/dt_scores"].size > np.unique(g["ties/bbox/dt_scores"]).size          # score ties
    ed = {k: g["edges/bbox/" + k] for k in ("ious", "precision", "recall", "iou_keys", "ev_keys", "dt_matches")}
    assert (ed["ious"] == 0.5).any() and (ed["ious"] == 0.75).any() and (ed["ious"] == 0.95).any()
    cats = CASES["edges"]["categories"]
    for c in (13, 21, 34):            # no gt anywhere / only ignored gts / nothing: a -1 plane
        assert (ed["precision"][:, :, cats.index(c)] == -1).all() and (ed["recall"][:, cats.index(c)] == -1).all()
    assert (ed["precision"][:, :, cats.index(3), 0] > -1).all()
    assert (g["maxdets/bbox/ev_keys"][:, 3] == 100).any()                 # a pair cut to maxDets[-1]
    per_image = {}
    for r in CASES["maxdets"]["results"]:
        per_image[r["image_id"]] = per_image.get(r["image_id"], 0) + 1
    assert max(per_image.values()) > 100
    assert g["empty/bbox/dt_ids"].size == 0 and (g["empty/bbox/recall"] == 0).any()
    assert (g["segm_special/segm/ious"] == -1).any()                      # the size-mismatch pair
    assert (g["segm_special/segm/ious"] == 1).any()
    assert g["large/bbox/stats"].shape == (12,) and g["large/bbox/recall"].shape == (10, 80, 4, 3)
    # a crowd matched by several detections at one threshold
    m = g["edges/bbox/dt_matches"]
    assert np.count_nonzero(m == 31) > 10


def test_rle_from_string_inverts_the_unmold_golden(golden_dir):
    from feature_intertwiner_amd.cocoeval import rle_from_string
    u = np.load(os.path.join(golden_dir, "unmold.npz"))
    n = 0
    for key in [k for k in u.files if k.endswith("/strings")]:
        base = key[:-len("strings")]
        cnts = np.split(u[base + "counts"], np.cumsum(u[base + "rle_len"])[:-1]) if len(u[base + "rle_len"]) else []
        strs = np.split(u[key], np.cumsum(u[base + "str_len"])[:-1]) if len(u[base + "str_len"]) else []
        for c, s in zip(cnts, strs):
            got = rle_from_string(s.tobytes())
            assert got.dtype == np.uint32 and np.array_equal(got, c)
            assert np.array_equal(R.rle_from_string(s.tobytes()), c)
            n += 1
    assert n > 200
    assert rle_from_string(b"").size == 0
    assert np.array_equal(rle_from_string("0" + chr(48 + (16 | 0x20)) + "0"), [0, 16])


def test_cocoeval_library_header_exports_and_bindings_match():
    from feature_intertwiner_amd import build, cocoeval
    build.build_hip()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "fi_cocoeval.h")).read()
    declared = sorted(set(re.findall(r"\b(fi_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))
    nm = subprocess.check_output(["nm", "-D", "--defined-only", build.COCOEVAL_LIB_PATH], text=True)
    exported = sorted(set(re.findall(r" T (fi_[a-z0-9_]+)", nm)))
    assert declared == exported == sorted(cocoeval.SIGNATURES) and len(declared) == 5
    assert b"gfx950" in open(build.COCOEVAL_LIB_PATH, "rb").read()
    needed = subprocess.check_output(["readelf", "-d", build.COCOEVAL_LIB_PATH], text=True)
    assert "[libfi_hip.so]" in needed and "$ORIGIN" in needed
    assert not re.search(r"(RPATH|RUNPATH).*\[/", needed)                  # no absolute path of the build tree
    # every entry point's comment cites the reference lines it replaces
    assert src.count("Replaces:") == 4 and "cocoeval.py:233-311" in src and "maskApi.c:77-96" in src


def test_c_entry_points_validate_without_a_gpu():
    from feature_intertwiner_amd import _lib, cocoeval
    L = cocoeval.load()
    err = lambda: _lib.load().fi_last_error()                                                    # noqa: E731
    x = ctypes.c_void_p(64)                                   # a non-null pointer that is never dereferenced
    assert L.fi_coco_match_workspace_bytes(1000, 4) == 16000 and L.fi_coco_match_workspace_bytes(-1, 4) == 0
    assert L.fi_coco_rle_stats(None, None, -1, None, None, None) == -1
    assert L.fi_coco_rle_stats(None, None, 0, None, None, None) == 0
    assert L.fi_coco_rle_stats(None, x, 3, x, x, None) == -1 and b"null" in err()
    assert L.fi_coco_iou(-1, *[None] * 3, 0, *[None] * 9, None) == -1
    assert L.fi_coco_iou(0, *[None] * 3, 0, *[None] * 9, None) == 0
    assert L.fi_coco_iou(2, x, x, x, 5, x, x, None, *[None] * 5, x, None) == -1 and b"null" in err()
    assert L.fi_coco_iou(2, x, x, x, 5, x, x, x, x, None, None, None, None, x, None) == -1 and b"segm" in err()
    m = [None] * 11
    assert L.fi_coco_match(1, *m, 0, 4, *[None] * 5, None) == -1                     # T = 0
    assert L.fi_coco_match(1, *m, 10, 0, *[None] * 5, None) == -1                    # A = 0
    assert L.fi_coco_match(1, *m, 17, 4, *[None] * 5, None) == -3 and b"T * A <= 64" in err()
    assert L.fi_coco_match(-1, *m, 10, 4, *[None] * 5, None) == -1                   # negative count
    assert L.fi_coco_match(0, *m, 10, 4, *[None] * 5, None) == 0
    assert L.fi_coco_match(1, *m, 10, 4, *[None] * 5, None) == -1 and b"null" in err()
    a = [None] * 10
    assert L.fi_coco_accumulate(80, *a, 10, 0, 4, 3, None, None, None, None) == -1   # R = 0
    assert L.fi_coco_accumulate(80, *a, 10, 101, 4, 0, None, None, None, None) == -1  # M = 0
    assert L.fi_coco_accumulate(80, *a, 0, 101, 4, 3, None, None, None, None) == -1  # T = 0
    assert L.fi_coco_accumulate(-1, *a, 10, 101, 4, 3, None, None, None, None) == -1
    assert L.fi_coco_accumulate(80, *a, 10, 1025, 4, 3, None, None, None, None) == -3 and b"R <= 1024" in err()
    assert L.fi_coco_accumulate(0, *a, 10, 101, 4, 3, None, None, None, None) == 0
    assert L.fi_coco_accumulate(80, *a, 10, 101, 4, 3, None, None, None, None) == -1 and b"null" in err()


def test_python_surface_raises_without_a_gpu():
    import torch
    from feature_intertwiner_amd import _lib, cocoeval, workflow
    assert callable(workflow.evaluate_coco)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.FiError, match="GPU only"):
            cocoeval.pack_results([])
    with pytest.raises(_lib.FiError, match="pack_ground_truth"):
        cocoeval.evaluate(object(), object())
