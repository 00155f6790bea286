"""Seeded inputs of the COCO evaluation goldens (tests/golden/cocoeval.npz, scripts/gen_golden_cocoeval.py).

Each case is a dict: 'name', 'images' [(id, height, width)], 'categories' [id], 'annotations' (COCO ground-truth
dicts), 'results' (the dicts of postprocess.coco_results, or with a 'segmentation' only) and 'types', the iouTypes it
is evaluated with.  Ids are non-zero and not contiguous, as in COCO."""
import hashlib
import json

import numpy as np

import unmold_ref
from unmold_cases import unmold_cases

LARGE = "large"                       # stored in the golden as SHA-256 + stats + recall only


def _ann(aid, img, cat, bbox, area=None, crowd=0, segm=None):
    a = {"id": aid, "image_id": img, "category_id": cat, "bbox": [float(v) for v in bbox],
         "area": float(bbox[2] * bbox[3] if area is None else area), "iscrowd": int(crowd)}
    if segm is not None:
        a["segmentation"] = segm
    return a


def _res(img, cat, bbox, score, segm=None, with_bbox=True):
    r = {"image_id": img, "category_id": cat, "score": np.float32(score)}
    if with_bbox:
        r["bbox"] = list(bbox)
    if segm is not None:
        r["segmentation"] = segm
    return r


def _random_boxes(rs, n, H, W, lo=4.0):
    w = rs.uniform(lo, 0.6 * W, n)
    h = rs.uniform(lo, 0.6 * H, n)
    x = rs.uniform(0, W - w)
    y = rs.uniform(0, H - h)
    return np.stack([x, y, w, h], 1)


def _jitter(rs, box, amount):
    x, y, w, h = box
    return [x + rs.uniform(-amount, amount) * w, y + rs.uniform(-amount, amount) * h,
            w * (1 + rs.uniform(-amount, amount)), h * (1 + rs.uniform(-amount, amount))]


def _detect(rs, gts, img, cats, H, W, n_extra, results, quant=None):
    """Detections around the ground truths of one image plus random ones."""
    for g in gts:
        for _ in range(rs.randint(0, 3)):
            s = rs.uniform(0.05, 1.0)
            results.append(_res(img, g["category_id"], _jitter(rs, g["bbox"], rs.choice([0.02, 0.1, 0.3])),
                                s if quant is None else np.round(s * quant) / quant))
    for b in _random_boxes(rs, n_extra, H, W):
        s = rs.uniform(0.0, 0.7)
        results.append(_res(img, int(rs.choice(cats)), list(b), s if quant is None else np.round(s * quant) / quant))


def _generic(rs, name, n_img, cats, quant=None, crowd_p=0.1, dup_p=0.0, gt_max=7, extra=6):
    images = [(100 + 7 * i, 200 + 10 * (i % 3), 240 + 16 * (i % 4)) for i in range(n_img)]
    anns, results, aid = [], [], 9000
    for img, H, W in images:
        gts = []
        for b in _random_boxes(rs, rs.randint(0, gt_max + 1), H, W):
            aid += rs.randint(1, 5)
            g = _ann(aid, img, int(rs.choice(cats)), b, area=b[2] * b[3] * rs.uniform(0.4, 1.0),
                     crowd=rs.rand() < crowd_p)
            gts.append(g)
            if rs.rand() < dup_p:                                # the same box again: an IoU tie
                aid += 1
                gts.append(_ann(aid, img, g["category_id"], b, area=g["area"]))
        anns += gts
        _detect(rs, gts, img, cats, H, W, rs.randint(0, extra + 1), results, quant)
    return {"name": name, "images": images, "categories": list(cats), "annotations": anns, "results": results,
            "types": ("bbox",)}


def _edges():
    """Integer boxes: areas on the 32^2 / 96^2 edges, IoU exactly 0.5 and 0.75, crowds matched several times,
    images with ground truths only / detections only / neither, categories without (non-ignored) ground truth."""
    images = [(1, 300, 400), (2, 300, 400), (3, 300, 400), (4, 300, 400), (5, 300, 400)]
    cats = [3, 5, 8, 13, 21, 34]          # 13: detections but no gt; 21: only crowd gts; 34: nothing at all
    A = [
        _ann(11, 1, 3, [10, 10, 32, 32]), _ann(12, 1, 3, [100, 10, 96, 96]), _ann(13, 1, 3, [10, 150, 16, 64]),
        _ann(14, 1, 3, [200, 150, 33, 31], area=1024), _ann(15, 1, 3, [300, 200, 50, 50], area=9216.0),
        # IoU exactly 0.5 (intersection 1, union 2) and 0.75 (3 / 4), 0.95 (19 / 20)
        _ann(21, 2, 5, [10, 10, 1, 1]), _ann(22, 2, 5, [50, 10, 3, 1]), _ann(23, 2, 5, [90, 10, 19, 1]),
        _ann(24, 2, 5, [10, 50, 40, 40]), _ann(25, 2, 5, [10, 50, 40, 40]), _ann(26, 2, 5, [10, 50, 40, 40]),
        # a crowd that covers several detections, next to a regular gt
        _ann(31, 2, 8, [100, 100, 200, 150], crowd=1), _ann(32, 2, 8, [120, 120, 30, 30]),
        _ann(33, 2, 8, [0, 0, 20, 20], area=5),
        _ann(41, 3, 3, [20, 20, 60, 60]), _ann(42, 3, 8, [5, 5, 100, 40]),           # image 3: gts only
        _ann(51, 1, 21, [10, 10, 100, 100], crowd=1), _ann(52, 2, 21, [10, 10, 50, 50], crowd=1),
    ]
    R = [
        _res(1, 3, [10, 10, 32, 32], 0.9), _res(1, 3, [100, 10, 96, 96], 0.8), _res(1, 3, [12, 150, 16, 64], 0.7),
        _res(1, 3, [200, 150, 32, 32], 0.6), _res(1, 3, [300, 200, 96, 96], 0.5), _res(1, 3, [350, 250, 8, 8], 0.4),
        _res(2, 5, [10, 10, 2, 1], 0.9), _res(2, 5, [50, 10, 4, 1], 0.8), _res(2, 5, [90, 10, 20, 1], 0.7),
        _res(2, 5, [10, 50, 40, 40], 0.6), _res(2, 5, [10, 50, 40, 40], 0.6), _res(2, 5, [11, 50, 40, 40], 0.6),
        _res(2, 5, [10, 51, 40, 40], 0.3), _res(2, 5, [300, 250, 10, 10], 0.95),       # overlaps nothing
        _res(2, 8, [110, 110, 40, 40], 0.9), _res(2, 8, [150, 150, 50, 50], 0.8), _res(2, 8, [200, 120, 60, 60], 0.7),
        _res(2, 8, [120, 120, 30, 30], 0.6), _res(2, 8, [121, 121, 30, 30], 0.5), _res(2, 8, [0, 0, 20, 20], 0.4),
        _res(4, 3, [20, 20, 60, 60], 0.9), _res(4, 13, [5, 5, 10, 10], 0.8),            # image 4: detections only
        _res(1, 13, [30, 30, 40, 40], 0.5), _res(1, 21, [20, 20, 50, 50], 0.9), _res(2, 21, [10, 10, 50, 50], 0.2),
    ]
    return {"name": "edges", "images": images, "categories": cats, "annotations": A, "results": R,
            "types": ("bbox",)}


def _maxdets(rs):
    """More than 100 detections in one (image, category) and in one image."""
    images = [(7, 200, 200), (9, 200, 200)]
    cats = [1, 2, 3]
    A, R = [], []
    boxes = _random_boxes(rs, 12, 200, 200)
    for j, b in enumerate(boxes):
        A.append(_ann(500 + 3 * j, 7, 1 if j < 9 else 2, b))
    for j in range(130):
        b = _jitter(rs, boxes[j % 9], 0.25)
        R.append(_res(7, 1, b, np.round(rs.uniform(0, 1) * 50) / 50))
    for j in range(30):
        R.append(_res(7, 2, _jitter(rs, boxes[9 + j % 3], 0.2), rs.uniform(0, 1)))
    for b in _random_boxes(rs, 5, 200, 200):
        A.append(_ann(600 + len(A), 9, 1, b))
        R.append(_res(9, 1, _jitter(rs, b, 0.05), rs.uniform(0.5, 1)))
        R.append(_res(9, 3, _jitter(rs, b, 0.05), rs.uniform(0.5, 1)))
    return {"name": "maxdets", "images": images, "categories": cats, "annotations": A, "results": R,
            "types": ("bbox",)}


def _rle_of(mask, as_string):
    c = unmold_ref.rle_counts(mask)
    H, W = mask.shape
    return {"size": [H, W], "counts": unmold_ref.rle_string(c) if as_string else [int(v) for v in c]}


def _blob(H, W, cy, cx, ry, rx):
    yy, xx = np.mgrid[0:H, 0:W]
    return ((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) <= 1.0).astype(np.uint8)


def _bbox_of(mask):
    ys, xs = np.nonzero(mask)
    return [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)]


def _segm_unmold():
    """The detections of the unmold case 'mixed' (tests/unmold_cases.py through tests/unmold_ref.py) against
    rectangle and blob ground truths derived from the detected boxes."""
    name, det, masks, hw, win = [c for c in unmold_cases() if c[0] == "mixed"][0]
    rs = np.random.RandomState(99)
    images, A, R = [], [], []
    aid = 70
    for b in range(det.shape[0]):
        H, W = int(hw[b, 0]), int(hw[b, 1])
        img = 11 * (b + 1)
        images.append((img, H, W))
        boxes, cls, scores, full, _ = unmold_ref.unmold_detections(det[b], masks[b], (H, W), win[b])
        rles = [{"size": [H, W], "counts": unmold_ref.rle_string(unmold_ref.rle_counts(full[j]))}
                for j in range(boxes.shape[0])]
        R += unmold_ref.coco_results(img, boxes, cls, scores, rles, lambda c: 7 * c)
        for j in range(0, boxes.shape[0], 3):
            y1, x1, y2, x2 = (int(v) for v in boxes[j])
            y1, x1, y2, x2 = max(y1, 0), max(x1, 0), min(y2, H), min(x2, W)
            m = np.zeros((H, W), np.uint8)
            if j % 2:
                m = _blob(H, W, (y1 + y2) / 2.0, (x1 + x2) / 2.0, max(1.0, (y2 - y1) / 2.0), max(1.0, (x2 - x1) / 2.0))
            else:
                m[y1:y2, x1:x2] = 1
            if not m.any():
                continue
            aid += 2
            A.append(_ann(aid, img, 7 * int(cls[j]), _bbox_of(m), area=float(m.sum()), crowd=rs.rand() < 0.15,
                          segm=_rle_of(m, as_string=bool(j % 4))))
    return {"name": "segm_unmold", "images": images, "categories": [7, 14, 21, 28], "annotations": A, "results": R,
            "types": ("bbox", "segm")}


def _segm_special():
    """Results with a 'segmentation' only (loadRes takes area and bbox from the RLE): a mask of zero runs, an
    all-zero mask, a full-image mask and a pair of different sizes whose RLE boxes overlap."""
    H, W = 40, 50
    images = [(5, H, W), (6, H, W)]
    full = np.ones((H, W), np.uint8)
    rect = np.zeros((H, W), np.uint8)
    rect[5:25, 10:30] = 1
    blob = _blob(H, W, 20, 25, 12, 15)
    other = np.zeros((30, 60), np.uint8)               # another image size
    other[5:25, 10:30] = 1
    A = [_ann(1001, 5, 1, _bbox_of(rect), area=float(rect.sum()), segm=_rle_of(rect, True)),
         _ann(1002, 5, 1, _bbox_of(blob), area=float(blob.sum()), segm=_rle_of(blob, False)),
         _ann(1003, 5, 1, [0, 0, W, H], area=float(H * W), crowd=1, segm=_rle_of(full, True)),
         _ann(1004, 6, 1, _bbox_of(rect), area=float(rect.sum()), segm=_rle_of(rect, False)),
         _ann(1005, 6, 2, _bbox_of(blob), area=float(blob.sum()), segm=_rle_of(blob, True))]
    seg = lambda m: _rle_of(m, True)                                           # noqa: E731
    R = [_res(5, 1, None, 0.9, seg(rect), False), _res(5, 1, None, 0.8, seg(blob), False),
         _res(5, 1, None, 0.7, seg(full), False), _res(5, 1, None, 0.6, {"size": [H, W], "counts": b""}, False),
         _res(5, 1, None, 0.5, seg(np.zeros((H, W), np.uint8)), False),
         _res(5, 1, None, 0.45, seg(np.roll(blob, 3, 1)), False),
         _res(6, 1, None, 0.9, seg(other), False), _res(6, 1, None, 0.3, seg(np.roll(rect, 2, 0)), False),
         _res(6, 2, None, 0.8, seg(blob), False), _res(6, 2, None, 0.8, seg(full), False)]
    return {"name": "segm_special", "images": images, "categories": [1, 2], "annotations": A, "results": R,
            "types": ("segm", "bbox")}


def _large(rs):
    """About 500 images x 80 categories x up to 100 detections per image."""
    cats = list(range(1, 91))[:80]
    images = [(1000 + 3 * i, 480, 640) for i in range(500)]
    A, R, aid = [], [], 10 ** 6
    for img, H, W in images:
        present = rs.choice(cats, rs.randint(1, 7), replace=False)
        gts = []
        for b in _random_boxes(rs, rs.randint(0, 15), H, W, lo=6.0):
            aid += 1
            gts.append(_ann(aid, img, int(rs.choice(present)), b, area=b[2] * b[3] * rs.uniform(0.3, 1.0),
                            crowd=rs.rand() < 0.03))
        A += gts
        res = []
        _detect(rs, gts * 3, img, cats, H, W, 100, res, quant=1000)
        order = rs.permutation(len(res))[:100]
        R += [res[i] for i in sorted(order)]
    return {"name": LARGE, "images": images, "categories": cats, "annotations": A, "results": R, "types": ("bbox",)}


def cocoeval_cases(large=True):
    rs = np.random.RandomState(4321)
    out = [_generic(rs, "generic", 6, [1, 2, 4, 9, 17]),
           _generic(rs, "ties", 8, [2, 3], quant=10, crowd_p=0.2, dup_p=0.5, gt_max=9, extra=10),
           _edges(), _maxdets(rs)]
    empty = _generic(rs, "empty", 3, [1, 2])
    empty["results"] = []
    out += [empty, _segm_unmold(), _segm_special()]
    if large:
        out.append(_large(np.random.RandomState(777)))
    return out


def _plain(o):
    if isinstance(o, bytes):
        return o.decode("ascii")
    if isinstance(o, np.generic):
        return float(o) if isinstance(o, np.floating) else int(o)
    raise TypeError(type(o))


def inputs_sha256(cases):
    h = hashlib.sha256()
    for c in cases:
        h.update(json.dumps({k: c[k] for k in ("name", "images", "categories", "annotations", "results", "types")},
                            sort_keys=True, default=_plain).encode())
    return h.hexdigest()
