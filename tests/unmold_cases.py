"""Seeded inputs of the unmold goldens (tests/golden/unmold.npz, scripts/gen_golden_unmold.py).

Each case is a batch in the model's inference layout: detections [bs, D, 6] fp32 (y1, x1, y2, x2 in molded-image
pixels, class id, score; zero rows pad), mrcnn_mask [bs, D, K, mh, mw] fp32, the original image shapes [bs, 2] and the
windows [bs, 4] (y1, x1, y2, x2 of the real image inside the molded one)."""
import hashlib

import numpy as np

# name -> small enough to keep the full dense masks in the golden
DENSE_LIMIT = 1 << 20


def _masks(rs, bs, D, K, mh, mw):
    return (1.0 / (1.0 + np.exp(-3.0 * rs.standard_normal((bs, D, K, mh, mw))))).astype(np.float32)


def _molded(rs, H, W, size=256, top=True):
    """resize_image-style window for an H x W original inside a square `size` image."""
    scale = size / max(H, W)
    h, w = int(round(H * scale)), int(round(W * scale))
    ty = (size - h) // 2 if top else 0
    tx = (size - w) // 2
    return np.array([ty, tx, ty + h, tx + w], np.float32)


def _random_dets(rs, D, n, win, zero_area=()):
    det = np.zeros((D, 6), np.float32)
    wy1, wx1, wy2, wx2 = win
    for i in range(n):
        y1 = rs.uniform(wy1, wy2 - 2)
        x1 = rs.uniform(wx1, wx2 - 2)
        y2 = min(wy2, y1 + rs.uniform(1.5, 0.6 * (wy2 - wy1)))
        x2 = min(wx2, x1 + rs.uniform(1.5, 0.6 * (wx2 - wx1)))
        det[i] = (y1, x1, y2, x2, rs.randint(1, 5), 1.0 - i / (n + 1.0))
    for i in zero_area:
        det[i, 2] = det[i, 0] + 0.2            # truncates to a zero-height box
    return det


def _edge_mask(rs, mh, mw):
    """Values at the bytescale rounding edges: (k + 0.5)/255 +- one ulp around the threshold byte, with cmin = 0 and
    cmax = 1 so that scale = 255."""
    k = rs.randint(120, 136, (mh, mw)).astype(np.float32)
    v = (k + np.float32(0.5)) / np.float32(255)
    v = np.where(rs.rand(mh, mw) < 0.5, np.nextafter(v, np.float32(0)), v)
    v = np.where(rs.rand(mh, mw) < 0.3, np.nextafter(v, np.float32(1)), v).astype(np.float32)
    v[0, 0], v[-1, -1] = 0.0, 1.0
    return v


def _edges_case(rs):
    """Window = whole image, scale 1: every box is exact in image pixels."""
    H, W, D, K, mh, mw = 61, 47, 24, 4, 28, 28
    boxes = [(5, 5, 6, 6), (3, 10, 4, 30), (10, 3, 40, 4), (7, 8, 27, 20), (11, 9, 39, 37), (0, 0, H, W),
             (0, 2, 20, 12), (40, 30, H, 45), (20, 35, 33, W), (0, 40, H, W), (30, 0, H, 15), (12, 12, 50, 40),
             (15, 15, 45, 35), (2, 2, 9, 44), (50, 1, 60, 46), (8, 20, 8, 30), (33, 5, 58, 26), (0, 0, 1, 1),
             (H - 1, W - 1, H, W), (25, 25, 26, 26)]
    det = np.zeros((1, D, 6), np.float32)
    for i, (y1, x1, y2, x2) in enumerate(boxes):
        det[0, i] = (y1 + 0.25, x1 + 0.75, y2 + 0.5, x2 + 0.125, 1 + i % (K - 1), 0.99 - 0.01 * i)
    masks = _masks(rs, 1, D, K, mh, mw)
    for i in range(len(boxes)):
        c = int(det[0, i, 4])
        if i % 5 == 1:
            masks[0, i, c] = 0.75                                       # constant: cscale = 0
        elif i % 5 == 2:
            masks[0, i, c] = _edge_mask(rs, mh, mw)
        elif i == 12:
            masks[0, i, c] = np.where(np.arange(mw) < 14, 0.1, 0.9)     # sharp vertical edge
    masks[0, 14, int(det[0, 14, 4])] = np.float32(0.3)                  # constant below the threshold: all zero
    return det, masks, np.array([[H, W]], np.int32), np.array([[0, 0, H, W]], np.float32)


def unmold_cases():
    """[(name, detections, mrcnn_mask, image_hw, windows)]"""
    out = []
    rs = np.random.RandomState(1234)

    # two originals of different shapes, padded on top / left; padded rows, zero-area rows in the middle
    hw = np.array([[120, 160], [150, 101]], np.int32)
    wins = np.stack([_molded(rs, 120, 160), _molded(rs, 150, 101, top=False)])
    D, K = 100, 5
    det = np.stack([_random_dets(rs, D, 37, wins[0], zero_area=(4, 17)), _random_dets(rs, D, 52, wins[1], (0, 30))])
    out.append(("mixed", det, _masks(rs, 2, D, K, 28, 28), hw, wins))

    det, masks, hw1, win1 = _edges_case(rs)
    out.append(("edges", det, masks, hw1, win1))

    # N = 100 (no class-0 row), overlapping boxes
    win = np.array([0, 0, 64, 48], np.float32)
    det = _random_dets(rs, 100, 100, win)[None]
    out.append(("full100", det, _masks(rs, 1, 100, 5, 28, 28), np.array([[64, 48]], np.int32), win[None]))

    # N = 0 in one image, a normal image next to it
    det = np.zeros((2, 100, 6), np.float32)
    det[1] = _random_dets(rs, 100, 9, np.array([0, 0, 40, 40], np.float32))
    det[0, 1:5] = det[1, 1:5]                                           # rows after the first class-0 row are ignored
    out.append(("empty", det, _masks(rs, 2, 100, 5, 28, 28), np.array([[33, 21], [40, 40]], np.int32),
                np.array([[0, 0, 33, 21], [0, 0, 40, 40]], np.float32)))

    # boxes that leave the image: the paste is clipped
    det = np.zeros((1, 8, 6), np.float32)
    det[0, :6] = [(-10, -5, 20, 15, 1, .9), (30, 30, 70, 55, 2, .8), (-3, 10, 5, 80, 3, .7),
                  (50, -20, 90, 10, 1, .6), (-50, -50, -10, -10, 2, .5), (45, 5, 70, 20, 3, .4)]
    out.append(("outside", det, _masks(rs, 1, 8, 4, 28, 28), np.array([[48, 40]], np.int32),
                np.array([[0, 0, 48, 40]], np.float32)))

    # COCO-shaped original through a 1024 window, all 81 classes
    win = _molded(rs, 480, 640, size=1024)
    det = _random_dets(rs, 100, 23, win)
    det[:23, 4] = rs.randint(1, 81, 23)
    out.append(("coco81", det[None], _masks(rs, 1, 100, 81, 28, 28), np.array([[480, 640]], np.int32), win[None]))

    # other mask sizes: 14 x 20 and 64 x 64
    win = np.array([0, 0, 50, 70], np.float32)
    out.append(("mask14x20", _random_dets(rs, 12, 10, win)[None], _masks(rs, 1, 12, 5, 14, 20),
                np.array([[50, 70]], np.int32), win[None]))
    out.append(("mask64", _random_dets(rs, 6, 6, win)[None], _masks(rs, 1, 6, 5, 64, 64),
                np.array([[50, 70]], np.int32), win[None]))
    return out


def inputs_sha256(cases):
    h = hashlib.sha256()
    for name, det, masks, hw, win in cases:
        h.update(name.encode())
        for a in (det, masks, hw, win):
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()
