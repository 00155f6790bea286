"""CPU: the NumPy restatement of polygon -> RLE and of the RLE merge (tests/cocopoly_ref.py) equals the golden made
from the reference's own maskApi.c / COCO.annToRLE / COCOeval (scripts/gen_golden_cocopoly.py) bit for bit;
libfi_cocomask.so exports what its header declares, bounds the keys of every polygon and validates its arguments."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import cocoeval_ref as R
import cocopoly_cases as C
import cocopoly_ref as P

POLYS = C.poly_cases()
SMALL = [c for c in POLYS if c[0] != C.ZIGZAG]
GROUPS = C.merge_cases()
DATASETS = {d["name"]: d for d in C.datasets()}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "cocopoly.npz"))


@functools.lru_cache(maxsize=None)
def batch():
    """The random batch and its restated keys and counts, computed once for the tests that need them."""
    polys, sizes = C.random_batch()
    keys = [P.poly_keys(p, h, w)[0] for p, (h, w) in zip(polys, sizes)]
    return polys, sizes, keys, [P.poly_counts(p, h, w) for p, (h, w) in zip(polys, sizes)]


def test_inputs_regenerate(golden):
    assert str(golden["inputs_sha256"]) == C.inputs_sha256(), "input drift: regenerate the golden"
    assert list(golden["poly/names"]) == [c[0] for c in SMALL] and list(golden["merge/names"]) == [g[0] for g in GROUPS]
    assert list(golden["datasets"]) == list(DATASETS)
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "cocopoly.npz")) <= 64 * 1024
    assert float(golden["batch/reference_seconds"]) > 0


def test_single_polygons_equal_golden(golden):
    exp = P.golden_counts(golden, "poly/")
    for j, (name, h, w, p) in enumerate(SMALL):
        got = P.poly_counts(p, h, w)
        assert got.dtype == np.uint32 and np.array_equal(got, exp[j]), (name, got, exp[j])
        assert tuple(golden["poly/size"][j]) == (h, w)
        area, box = P.stats(got, h, w)
        assert area == golden["poly/area"][j] and np.array_equal(box, golden["poly/bbox"][j]), name
    by = {c[0]: e for c, e in zip(SMALL, exp)}
    # what the issue's cases are there for
    assert list(by["vertical_line"]) == [12 * 15] and list(by["one_point"]) == [12 * 15]
    assert list(by["outside"]) == [12 * 15] and list(by["sliver_cancels"]) == [12 * 15]
    assert list(by["whole_image"]) == [0, 12 * 15] and list(by["image_1x1_around"]) == [0, 1]
    assert np.array_equal(by["closed_twice"], by["square_int"]) and np.array_equal(by["odd_length"], by["square_int"])
    assert np.array_equal(by["repeated_vertex"], by["square_int"])


def test_zigzag_and_batch_equal_golden_digests(golden):
    _, h, w, p = [c for c in POLYS if c[0] == C.ZIGZAG][0]
    z = P.poly_counts(p, h, w)
    assert C.digest([z]) == str(golden["zigzag/sha256"]) and len(z) == int(golden["zigzag/num_counts"])
    area, box = P.stats(z, h, w)
    assert area == golden["zigzag/area"][0] and np.array_equal(box, golden["zigzag/bbox"][0])
    counts = batch()[3]
    assert C.digest(counts) == str(golden["batch/sha256"])
    assert sum(len(c) for c in counts) == int(golden["batch/total_counts"])


@pytest.mark.parametrize("intersect", [0, 1])
def test_merge_equals_golden(golden, intersect):
    key = "merge%d/" % intersect
    exp = P.golden_counts(golden, key)
    for j, (name, h, w, parts) in enumerate(GROUPS):
        got, gh, gw = P.merge([(P.poly_counts(p, h, w), h, w) for p in parts], bool(intersect))
        assert np.array_equal(got, exp[j]) and (gh, gw) == tuple(golden[key + "size"][j]), (name, got, exp[j])
        area, box = P.stats(got, gh, gw)
        assert area == golden[key + "area"][j] and np.array_equal(box, golden[key + "bbox"][j]), name
    # the same part twice: the union is the part, not the parity of the two
    j = [g[0] for g in GROUPS].index("same_twice")
    assert np.array_equal(exp[j], P.poly_counts(GROUPS[j][3][0], GROUPS[j][1], GROUPS[j][2]))


@pytest.mark.parametrize("name", list(DATASETS))
def test_ann_to_rle_and_evaluation_equal_golden(golden, name):
    case = DATASETS[name]
    sizes = C.image_sizes(case)
    exp = P.golden_counts(golden, name + "/ann_")
    kinds = set()
    for a, e, hw in zip(case["annotations"], exp, golden[name + "/ann_size"]):
        c, h, w = P.ann_to_rle(a, sizes)
        assert np.array_equal(c, e) and (h, w) == tuple(hw), a["id"]
        s = a["segmentation"]
        kinds.add("poly%d" % min(len(s), 2) if isinstance(s, list) else type(s["counts"]).__name__)
    assert kinds == {"poly1", "poly2", "list", "bytes"}                  # uncompressed RLE and COCO string too
    anns = P.with_rle_segmentations(case["annotations"], sizes)
    for iou_type in case["types"]:
        got = R.evaluate(anns, case["results"], [i for i, _, _ in case["images"]], case["categories"], iou_type)
        R.assert_equal_golden(got, golden, "%s/%s/" % (name, iou_type))
        assert got["stats"][0] > 0


def test_library_header_exports_and_bindings_match():
    from feature_intertwiner_amd import build, cocomask
    build.build_hip()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "fi_cocomask.h")).read()
    declared = sorted(set(re.findall(r"\b(fi_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))
    nm = subprocess.check_output(["nm", "-D", "--defined-only", build.COCOMASK_LIB_PATH], text=True)
    exported = sorted(set(re.findall(r" T (fi_[a-z0-9_]+)", nm)))
    assert declared == exported == sorted(cocomask.SIGNATURES) and len(declared) == 4
    assert b"gfx950" in open(build.COCOMASK_LIB_PATH, "rb").read()
    needed = subprocess.check_output(["readelf", "-d", build.COCOMASK_LIB_PATH], text=True)
    assert "[libfi_hip.so]" in needed and "$ORIGIN" in needed
    assert not re.search(r"(RPATH|RUNPATH).*\[/", needed)                  # no absolute path of the build tree
    # every comment block of entry points cites the reference lines it replaces
    blocks = re.findall(r"/\* -{20,}.*?-{20,} \*/", src, flags=re.S)
    assert len(blocks) == 3 and all("Replaces:" in b for b in blocks)
    assert "maskApi.c:161-201" in src and "maskApi.c:49-70" in src and "coco.py" in src
    assert int(re.search(r"#define FI_COCOMASK_LDS_KEYS (\d+)", src).group(1)) == C.LDS_KEYS


def test_bound_covers_the_true_key_count():
    from feature_intertwiner_amd import cocomask
    polys, sizes, batch_keys, batch_counts = batch()
    items = [(n, h, w, p) for n, h, w, p in POLYS] + [("batch%d" % j, h, w, p)
                                                     for j, (p, (h, w)) in enumerate(zip(polys, sizes))]
    keys = [P.poly_keys(p, h, w)[0] for _, h, w, p in POLYS] + batch_keys
    counts = [P.poly_counts(p, h, w) for _, h, w, p in POLYS] + batch_counts
    xy, off = cocomask.flatten_polygons([p for _, _, _, p in items])
    bound = cocomask.poly_bound(xy, off)
    assert bound.shape == (len(items),)
    tight = 0
    for (name, h, w, p), b, k, c in zip(items, bound, keys, counts):
        assert k.size <= b, (name, k.size, b)
        assert len(c) <= b + 1
        tight += k.size == b and b > 0
    by = dict(zip([n for n, _, _, _ in items], bound))
    assert by["bound_attained"] == 2 and P.poly_keys(*[(p, h, w) for n, h, w, p in POLYS if n == "bound_attained"][0]
                                                     )[0].size == 2
    assert by["lds_threshold"] == C.LDS_KEYS and by["above_threshold"] == C.LDS_KEYS + 1
    assert by[C.ZIGZAG] > 8 * C.LDS_KEYS and by["vertical_line"] == 0
    assert tight >= 1


def test_c_entry_points_validate_without_a_gpu():
    from feature_intertwiner_amd import _lib, cocomask
    L = cocomask.load()
    err = lambda: _lib.load().fi_last_error()                                                    # noqa: E731
    x = ctypes.c_void_p(64)                                   # a non-null pointer that is never dereferenced
    hp = lambda a: ctypes.c_void_p(a.ctypes.data)                                                # noqa: E731
    xy, off, out = np.array([0., 0, 4, 0, 4, 4]), np.array([0, 3], np.int64), np.zeros(1, np.int64)
    assert L.fi_cocomask_poly_bound(hp(xy), hp(off), 1, hp(out)) == 0 and out[0] == 8
    assert L.fi_cocomask_poly_bound(None, None, 0, None) == 0
    assert L.fi_cocomask_poly_bound(None, None, -1, None) == -1
    assert L.fi_cocomask_poly_bound(None, hp(off), 1, hp(out)) == -1 and b"null" in err()
    bad = np.array([0., 0, np.nan, 0, 4, 4])
    assert L.fi_cocomask_poly_bound(hp(bad), hp(off), 1, hp(out)) == -1 and b"finite" in err()
    bad = np.array([0., 0, 4, 3e9, 4, 4])
    assert L.fi_cocomask_poly_bound(hp(bad), hp(off), 1, hp(out)) == -1 and b"finite" in err()
    empty = np.array([0, 0], np.int64)
    assert L.fi_cocomask_poly_bound(hp(xy), hp(empty), 1, hp(out)) == -1 and b"vertex" in err()
    assert L.fi_cocomask_workspace_bytes(1000, 7) == 4000 and L.fi_cocomask_workspace_bytes(-1, 7) == 0
    assert L.fi_cocomask_workspace_bytes(1000, 0) == 0
    assert L.fi_cocomask_from_polygons(None, None, None, None, 0, 0, None, None, None, None) == 0
    assert L.fi_cocomask_from_polygons(None, None, None, None, -1, 0, None, None, None, None) == -1
    assert L.fi_cocomask_from_polygons(x, x, x, x, 2, -1, x, x, x, None) == -1
    assert L.fi_cocomask_from_polygons(x, x, x, x, 2, 1 << 30, x, x, x, None) == -1 and b"2^30" in err()
    assert L.fi_cocomask_from_polygons(x, x, None, x, 2, 10, x, x, x, None) == -1 and b"null" in err()
    assert L.fi_cocomask_from_polygons(x, x, x, x, 2, 10, x, x, None, None) == -1 and b"workspace" in err()
    assert L.fi_cocomask_merge(None, None, None, None, 0, 0, 0, None, None, None, None) == 0
    assert L.fi_cocomask_merge(None, None, None, None, -1, 0, 0, None, None, None, None) == -1
    assert L.fi_cocomask_merge(x, x, x, x, 2, 10, 2, x, x, x, None) == -1 and b"intersect" in err()
    assert L.fi_cocomask_merge(x, x, x, x, 2, 1 << 30, 0, x, x, x, None) == -1 and b"2^30" in err()
    assert L.fi_cocomask_merge(x, None, x, x, 2, 10, 0, x, x, x, None) == -1 and b"null" in err()
    assert L.fi_cocomask_merge(x, x, x, x, 2, 10, 1, x, x, None, None) == -1 and b"workspace" in err()


def test_python_surface_decided_inputs_without_a_gpu():
    import torch
    from feature_intertwiner_amd import _lib, cocoeval, cocomask
    with pytest.raises(_lib.FiError, match="at least 6 numbers"):
        cocomask.flatten_polygons([[1, 1, 5, 1]])
    xy, off = cocomask.flatten_polygons([[1, 1, 5, 1, 5, 5, 9], [0, 0, 1, 0, 1, 1, 0, 1]])
    assert list(off) == [0, 3, 7] and xy.size == 14                       # the odd number is dropped
    if not torch.cuda.is_available():
        with pytest.raises(_lib.FiError, match="GPU only"):
            cocomask.from_polygons([[1, 1, 5, 1, 5, 5]], [(8, 8)])
        with pytest.raises(_lib.FiError, match="GPU only"):
            cocoeval.load_ground_truth({"images": [], "categories": [], "annotations": []})
    with pytest.raises(_lib.FiError, match="no 'images'"):
        cocoeval.load_ground_truth({"annotations": []})
    assert callable(cocomask.ann_to_rle) and callable(cocomask.merge)
