"""CPU: the NumPy restatement of the inference unmolding (tests/unmold_ref.py) equals the golden made from the
reference's own `_unmold_detections` and maskApi.c (scripts/gen_golden_unmold.py) bit for bit, and its resize equals
the installed Pillow's on random shapes."""
import os

import numpy as np
import pytest

import unmold_ref as R
from unmold_cases import inputs_sha256, unmold_cases


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "unmold.npz"))


def test_inputs_regenerate(golden):
    assert str(golden["inputs_sha256"]) == inputs_sha256(unmold_cases()), "RNG drift: regenerate the golden"


def split(flat, lens):
    return np.split(flat, np.cumsum(lens)[:-1]) if len(lens) else []


@pytest.mark.parametrize("case", [c[0] for c in unmold_cases()])
def test_restatement_equals_golden(golden, case):
    name, det, masks, hw, win = [c for c in unmold_cases() if c[0] == case][0]
    for b in range(det.shape[0]):
        k = "%s/%d/" % (name, b)
        H, W = (int(v) for v in hw[b])
        boxes, cls, scores, full, _ = R.unmold_detections(det[b], masks[b], (H, W), win[b])
        assert np.array_equal(boxes, golden[k + "boxes"])
        assert np.array_equal(cls, golden[k + "class_ids"])
        assert np.array_equal(scores.view(np.uint32), golden[k + "scores"].view(np.uint32))
        if k + "dense" in golden:
            assert np.array_equal(np.packbits(full, axis=-1), golden[k + "dense"])
        import hashlib
        assert hashlib.sha256(full.tobytes()).hexdigest() == str(golden[k + "dense_sha256"])
        cnts = split(golden[k + "counts"], golden[k + "rle_len"])
        strs = split(golden[k + "strings"], golden[k + "str_len"])
        assert len(cnts) == len(strs) == boxes.shape[0]
        for j in range(boxes.shape[0]):
            c = R.rle_counts(full[j])
            assert np.array_equal(c, cnts[j])
            assert R.rle_string(c) == strs[j].tobytes()
            assert np.array_equal(R.rle_decode(c, (H, W)), full[j])


def test_golden_covers_the_issue_cases(golden):
    names = list(golden["cases"])
    assert {"mixed", "edges", "full100", "empty", "outside", "coco81", "mask14x20", "mask64"} <= set(names)
    assert golden["empty/0/boxes"].shape == (0, 4) and golden["empty/0/counts"].size == 0
    assert golden["full100/0/boxes"].shape[0] == 100
    # all-zero mask after the threshold: a single count H*W
    cnts = split(golden["edges/0/counts"], golden["edges/0/rle_len"])
    assert any(c.size == 1 and c[0] == 61 * 47 for c in cnts)
    assert any(c[0] == 0 for c in cnts)              # a mask that starts with a one (box at 0, 0)


def test_rle_string_quirks():
    assert R.rle_string(np.array([5], np.uint32)) == bytes([48 + 5])
    assert R.rle_string(np.array([16], np.uint32)) == bytes([48 + (16 | 0x20), 48])       # sign bit set -> 2 chars
    # counts i > 2 are delta-coded against cnts[i-2]; cnts[2] is raw
    s = R.rle_string(np.array([3, 4, 9, 4, 5], np.uint32))
    assert s == bytes([48 + 3, 48 + 4, 48 + 9, 48 + 0, 48 + ((5 - 9) & 0x1F)])
    s = R.rle_string(np.array([0, 30, 2, 1], np.uint32))              # 1 - 30 = -29: negative delta
    assert s[-2:] == bytes([48 + ((-29) & 0x1F | 0x20), 48 + ((-29 >> 5) & 0x1F)])


def test_resize_equals_pillow():
    Image = pytest.importorskip("PIL.Image")
    rs = np.random.RandomState(7)
    for t in range(150):
        mh, mw = (28, 28) if t < 100 else tuple(rs.randint(1, 65, 2))
        img = rs.randint(0, 256, (mh, mw)).astype(np.uint8)
        h, w = rs.randint(1, 120, 2) if t % 3 else rs.randint(1, 28, 2)            # a third downsample
        ref = np.asarray(Image.fromarray(img, "L").resize((int(w), int(h)), Image.BILINEAR))
        assert np.array_equal(R.resize_bilinear(img, int(h), int(w)), ref), (mh, mw, h, w)


def test_eval_library_header_exports_and_bindings_match():
    import re
    import subprocess
    from feature_intertwiner_amd import build, postprocess
    build.build_hip()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "fi_eval.h")).read()
    declared = sorted(set(re.findall(r"\b(fi_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))
    nm = subprocess.check_output(["nm", "-D", "--defined-only", build.EVAL_LIB_PATH], text=True)
    exported = sorted(set(re.findall(r" T (fi_[a-z0-9_]+)", nm)))
    assert declared == exported == sorted(postprocess.SIGNATURES) and len(declared) == 4
    assert b"gfx950" in open(build.EVAL_LIB_PATH, "rb").read()
    needed = subprocess.check_output(["readelf", "-d", build.EVAL_LIB_PATH], text=True)
    assert "[libfi_hip.so]" in needed and "$ORIGIN" in needed            # no absolute path of the build tree


def test_c_entry_points_validate_without_a_gpu():
    import ctypes
    from feature_intertwiner_amd import _lib, postprocess
    L = postprocess.load()
    hw = (ctypes.c_int32 * 4)(480, 640, 5000, 10)
    assert L.fi_unmold_workspace_bytes(2, 100, 28, 28) == 1024 + 200 * 784
    assert L.fi_unmold_workspace_bytes(0, 100, 28, 28) == 0
    args = [None] * 3 + [hw, None]
    assert L.fi_unmold_prepare(*args, 1, 100, 81, 65, 28, *([None] * 7), None) == -3       # mask > 64
    assert b"1..64" in _lib.load().fi_last_error()          # the message is libfi_hip's, as for every entry point
    assert L.fi_unmold_prepare(*args, 2, 100, 81, 28, 28, *([None] * 7), None) == -3       # image 5000 px
    assert b"4096" in _lib.load().fi_last_error()
    assert L.fi_unmold_prepare(*args, 1, 0, 81, 28, 28, *([None] * 7), None) == -1         # no detection rows
    assert L.fi_unmold_prepare(*args, 1, 100, 81, 28, 28, *([None] * 7), None) == -1       # null pointers
    assert L.fi_unmold_encode(None, hw, None, None, 1, 100, 28, 0, None, None, None, None, None) == -3
    assert L.fi_unmold_paste(None, hw, None, None, 1, 100, 28, 28, None, -1, None, None) == -1
    assert L.fi_unmold_paste(None, hw, None, None, 1, 100, 28, 28, None, 0, None, None) == 0  # nothing to write
