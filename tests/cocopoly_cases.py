"""Inputs of the polygon -> RLE goldens (tests/golden/cocopoly.npz, scripts/gen_golden_cocopoly.py): deterministic,
plain Python and NumPy.

  poly_cases()     [(name, h, w, flat coordinate list)]: one polygon each, the smallest shapes at which rleFrPoly
                   can go wrong.
  merge_cases()    [(name, h, w, [polygon, ..])]: the parts of one object, merged with intersect = 0 and 1.
  random_batch()   seeded polygons and image sizes for the offsets and the batching (SHA-256 only in the golden).
  datasets()       two small data sets in the form of tests/cocoeval_cases.py, with polygon ground truth."""
import hashlib
import json

import numpy as np

from cocoeval_cases import _ann, _bbox_of, _blob, _plain, _res, _rle_of

LDS_KEYS = 4096                      # FI_COCOMASK_LDS_KEYS: larger bounds are sorted in the global workspace
ZIGZAG = "zigzag_global"             # far above the LDS threshold: SHA-256 only as well


def _sweeps(last_x):
    """Eight horizontal sweeps of 512 pixels: the bound is 8 * 512 = 4096, plus ceil(5 * last_x / 5) for the closing
    edge when the last vertex leaves x = 0."""
    xs = [0, 512, 0, 512, 0, 512, 0, 512, last_x]
    out = []
    for j, x in enumerate(xs):
        out += [x, 3 + 7 * j]
    return out


def _zigzag():
    rs = np.random.RandomState(31)
    out = []
    for j in range(240):
        x = rs.uniform(0, 300) if j % 2 == 0 else rs.uniform(700, 1024)
        out += [round(float(x), 2), round(float(rs.uniform(-20, 1044)), 2)]
    return out


def poly_cases():
    H, W = 12, 15
    sq = lambda a, b: [a, a, b, a, b, b, a, b]                                                   # noqa: E731
    cases = [
        ("triangle", H, W, [2, 2, 10, 3, 5, 9]),
        ("square_int", H, W, sq(2, 8)),
        ("square_half", H, W, sq(2.5, 8.5)),
        # 5 * c + .5 on or next to an integer in double: 0.1, 0.3, 0.7, 0.9, 8.3, 2.29 / 2.31
        ("square_dec_a", H, W, [2.1, 2.3, 8.3, 2.3, 8.3, 8.7, 2.1, 8.7]),
        ("square_dec_b", H, W, [2.29, 2.31, 8.29, 2.31, 8.31, 8.69, 2.3, 8.7]),
        ("square_dec_c", H, W, [0.1, 0.3, 0.7, 0.3, 0.7, 0.9, 0.1, 0.9]),
        ("square_dec_d", H, W, [1.1, 1.9, 9.9, 1.9, 9.9, 10.1, 1.1, 10.1]),
        ("octants", 16, 16, [5, 1, 9, 2, 13, 5, 14, 9, 11, 13, 7, 14, 3, 11, 1, 6]),
        ("octants_reversed", 16, 16, [1, 6, 3, 11, 7, 14, 11, 13, 14, 9, 13, 5, 9, 2, 5, 1]),
        ("diamond", 16, 16, [8, 2, 14, 8, 8, 14, 2, 8]),
        ("vertical_line", H, W, [5, 2, 5, 9, 5, 4]),
        ("one_point", H, W, [4, 4, 4, 4, 4, 4]),
        ("repeated_vertex", H, W, [2, 2, 8, 2, 8, 2, 8, 8, 2, 8]),
        ("closed_twice", H, W, [2, 2, 8, 2, 8, 8, 2, 8, 2, 2]),
        ("odd_length", H, W, [2, 2, 8, 2, 8, 8, 2, 8, 99]),
        ("negative", H, W, [-3, -2, 6, -2, 6, 5, -3, 5]),
        # (-0.3, 0): (int) truncates towards zero, floor would not
        ("small_negative", H, W, [-0.25, -0.15, 6, -0.05, 6, 5, -0.29, 5]),
        ("small_negative_b", H, W, [-0.1, -0.1, 4.2, -0.2, 4.2, 3.3, -0.21, 3.3]),
        ("steep_through_zero", H, W, [-4, 1, 3, 10, -2.3, 12]),
        ("steep_negative", H, W, [-1.4, 0, 2.2, 11, -0.7, 6]),
        ("beyond", H, W, [5, 5, 20, 5, 20, 20, 5, 20]),
        ("outside", H, W, [20, 20, 30, 20, 30, 30]),
        ("outside_negative", H, W, [-10, -10, -5, -10, -5, -3]),
        ("outside_above", H, W, [2, -9, 8, -9, 8, -3]),
        ("whole_image", H, W, [-5, -5, 30, -5, 30, 30, -5, 30]),
        ("whole_exact", H, W, [0, 0, 15, 0, 15, 12, 0, 12]),
        ("touch_w_minus_1", H, W, [10, 3, 14, 3, 14, 12, 10, 12]),
        ("touch_w", H, W, [10, 3, 15, 3, 15, 12, 10, 12]),
        ("touch_w_half", H, W, [10, 3, 14.5, 3, 14.5, 11.5, 10, 11.5]),
        ("image_1x1_exact", 1, 1, [0, 0, 1, 0, 1, 1, 0, 1]),
        ("image_1x1_around", 1, 1, [-1, -1, 2, -1, 2, 2, -1, 2]),
        ("image_1x1_inside", 1, 1, [0.2, 0.2, 0.8, 0.2, 0.8, 0.8]),
        ("image_w1", 9, 1, [0, 1, 1, 1, 1, 7, 0, 7]),
        ("image_h1", 1, 9, [1, 0, 7, 0, 7, 1, 1, 1]),
        ("bow_tie", H, W, [2, 2, 10, 10, 10, 2, 2, 10]),
        ("sliver_cancels", H, W, [2, 5.0, 10, 5.05, 2, 5.1]),
        ("one_column", H, W, [3.4, 2, 3.6, 2, 3.6, 9, 3.4, 9]),
        ("bound_attained", H, W, [0.4, 1, 0.6, 1, 0.6, 5, 0.4, 5]),
        ("star", 40, 40, [20, 2, 25, 38, 3, 12, 37, 12, 9, 36]),
        ("lds_threshold", 64, 600, _sweeps(0)),                     # bound == 4096: the last LDS size
        ("above_threshold", 64, 600, _sweeps(0.2)),                 # bound == 4097: the first global size
        (ZIGZAG, 1024, 1024, _zigzag()),
    ]
    return cases


def merge_cases():
    H, W = 20, 24
    A = [2, 2, 8, 2, 8, 8, 2, 8]
    B = [12, 10, 18, 10, 18, 16, 12, 16]              # disjoint from A
    C = [5, 5, 11, 5, 11, 11, 5, 11]                  # overlaps A
    D = [4, 4, 6, 4, 6, 6, 4, 6]                      # inside A
    T = [1, 12, 9, 19, 1, 19]
    X = [14, 1, 22, 9, 22, 1, 14, 9]                  # bow-tie
    full = [-5, -5, 40, -5, 40, 40, -5, 40]
    empty = [30, 30, 35, 30, 35, 35]
    return [("one", H, W, [A]), ("disjoint", H, W, [A, B]), ("overlapping", H, W, [A, C]), ("nested", H, W, [A, D]),
            ("same_twice", H, W, [A, A]), ("seven", H, W, [A, B, C, D, T, X, A]), ("with_full", H, W, [C, full]),
            ("with_empty", H, W, [empty, C, B]), ("full_and_empty", H, W, [full, empty]),
            ("column_order", 7, 5, [[0, 0, 2, 0, 2, 7, 0, 7], [1, 2, 5, 2, 5, 5, 1, 5], [3, 0, 4, 0, 4, 7, 3, 7]])]


def random_polygons(seed, n):
    """n polygons of 3 .. 40 vertices in images of 1 x 1 .. 480 x 640, some vertices out of range; coordinates with two
    decimals (as COCO stores them), integers or halves.  Returns (polygons, sizes [(h, w)])."""
    rs = np.random.RandomState(seed)
    polys, sizes = [], []
    for j in range(n):
        h = 1 if j % 97 == 0 else int(rs.randint(1, 481))
        w = 1 if j % 89 == 0 else int(rs.randint(1, 641))
        k = int(rs.randint(3, 41))
        lo, hi = (-0.2, 1.2) if j % 3 == 0 else (0.0, 1.0)
        x = rs.uniform(lo * w - (3 if j % 3 == 0 else 0), hi * w + (3 if j % 3 == 0 else 0), k)
        y = rs.uniform(lo * h - (3 if j % 3 == 0 else 0), hi * h + (3 if j % 3 == 0 else 0), k)
        xy = np.stack([x, y], 1).ravel()
        mode = j % 5
        xy = np.round(xy, 2) if mode < 3 else (np.round(xy) if mode == 3 else np.round(xy * 2) / 2)
        polys.append([float(v) for v in xy] + ([7.0] if j % 11 == 0 else []))
        sizes.append((h, w))
    return polys, sizes


def random_batch():
    return random_polygons(2024, 2000)


def _poly_ann(aid, img, cat, parts, crowd=0):
    xs = np.concatenate([np.asarray(p, np.float64)[0::2] for p in parts])
    ys = np.concatenate([np.asarray(p, np.float64)[1::2] for p in parts])
    box = [float(xs.min()), float(ys.min()), float(xs.max() - xs.min()), float(ys.max() - ys.min())]
    return _ann(aid, img, cat, box, area=0.8 * box[2] * box[3], crowd=crowd, segm=[list(p) for p in parts])


def _ellipse(cx, cy, rx, ry, k, phase=0.0):
    a = phase + 2 * np.pi * np.arange(k) / k
    out = np.stack([cx + rx * np.cos(a), cy + ry * np.sin(a)], 1).ravel()
    return [float(v) for v in np.round(out, 2)]


def _dataset(name, seed, with_bbox, types):
    rs = np.random.RandomState(seed)
    images = [(3, 40, 50), (8, 30, 60), (9, 40, 50), (14, 25, 25)]
    cats = [2, 5, 11]
    A, R = [], []
    aid = 400
    for img, H, W in images[:3]:
        for j in range(4):
            cy, cx = rs.uniform(8, H - 8), rs.uniform(8, W - 8)
            ry, rx = rs.uniform(3, 9), rs.uniform(3, 11)
            cat = cats[int(rs.randint(0, 3))]
            parts = [_ellipse(cx, cy, rx, ry, int(rs.randint(5, 14)), rs.uniform(0, 1))]
            if j == 1:                                              # an object of two parts, one out of the image
                parts.append(_ellipse(cx + rx, cy - ry, 4.5, 3.5, 7))
            if j == 2 and img == 8:                                 # three parts, two of them overlapping
                parts += [_ellipse(cx - 2, cy, 3, 3, 6), [1, 1, 6, 1.5, 5.5, 7, 1.25, 6.75]]
            aid += 3
            A.append(_poly_ann(aid, img, cat, parts))
            for q in range(int(rs.randint(1, 4))):                  # detections near the object
                m = _blob(H, W, cy + rs.uniform(-2, 2), cx + rs.uniform(-2, 2), ry * rs.uniform(0.7, 1.2),
                          rx * rs.uniform(0.7, 1.2))
                if m.any():
                    R.append(_res(img, cat, _bbox_of(m), rs.uniform(0.2, 1.0), _rle_of(m, True), with_bbox))
    # a crowd as a COCO string and a regular object as an uncompressed RLE, next to the polygons
    H, W = 40, 50
    crowd = np.zeros((H, W), np.uint8)
    crowd[5:30, 20:48] = 1
    A.append(_ann(aid + 5, 3, 5, _bbox_of(crowd), area=float(crowd.sum()), crowd=1, segm=_rle_of(crowd, True)))
    blob = _blob(H, W, 28, 14, 7, 9)
    A.append(_ann(aid + 9, 9, 2, _bbox_of(blob), area=float(blob.sum()), segm=_rle_of(blob, False)))
    R.append(_res(3, 5, _bbox_of(crowd), 0.55, _rle_of(np.roll(crowd, 2, 1), True), with_bbox))
    R.append(_res(9, 2, _bbox_of(blob), 0.9, _rle_of(blob, True), with_bbox))
    R.append(_res(14, 11, [2, 2, 9, 9], 0.4, _rle_of(_blob(25, 25, 8, 8, 4, 4), True), with_bbox))   # no gt there
    return {"name": name, "images": images, "categories": cats, "annotations": A, "results": R, "types": types}


def datasets():
    return [_dataset("polys_a", 61, True, ("bbox", "segm")), _dataset("polys_b", 62, False, ("segm", "bbox"))]


def dataset_dict(case):
    """The case as the dict of an instances_*.json."""
    return {"images": [{"id": i, "height": h, "width": w} for i, h, w in case["images"]],
            "categories": [{"id": c, "name": str(c), "supercategory": "x"} for c in case["categories"]],
            "annotations": case["annotations"]}


def image_sizes(case):
    return {i: (h, w) for i, h, w in case["images"]}


def digest(counts_list):
    """SHA-256 of the lengths (int64) followed by all counts (uint32): how the golden keeps the large cases."""
    h = hashlib.sha256(np.array([len(c) for c in counts_list], np.int64).tobytes())
    for c in counts_list:
        h.update(np.ascontiguousarray(c, np.uint32).tobytes())
    return h.hexdigest()


def inputs_sha256():
    h = hashlib.sha256()
    polys, sizes = random_batch()
    h.update(json.dumps([poly_cases(), merge_cases(), polys, sizes], sort_keys=True, default=_plain).encode())
    for c in datasets():
        h.update(json.dumps({k: c[k] for k in ("name", "images", "categories", "annotations", "results", "types")},
                            sort_keys=True, default=_plain).encode())
    return h.hexdigest()
