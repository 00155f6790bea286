"""NumPy restatement of polygon -> RLE (rleFrPoly, datasets/eval/common/maskApi.c:161-201), of the merge of RLEs
(rleMerge, maskApi.c:49-70) and of COCO.annToRLE (pycocotools/coco.py:405-424).  TEST INFRASTRUCTURE.

Its own structure: every upsampled point of every edge at once (one array per polygon), and the C's "sort, difference,
cancel zero differences in pairs" as its meaning: a toggle at every distinct key < h * w of odd multiplicity.  Merging
works on toggle positions: the covered state after each position, for all members at once.  Checked bit for bit against
the reference's own code through tests/golden/cocopoly.npz (tests/test_cocopoly_golden.py)."""
import numpy as np

import cocoeval_ref


def _trunc(a):
    """(int) of a double: towards zero.  NaN (the slope 0 / 0 of a repeated vertex) becomes 0; it is never used."""
    return np.nan_to_num(np.trunc(a), nan=0.0).astype(np.int64)


def poly_keys(xy, h, w):
    """The boundary keys x * h + y of rleFrPoly before sorting, in point order."""
    p = np.asarray(xy, np.float64).reshape(-1)
    k = p.size // 2
    p = p[:2 * k].reshape(k, 2)
    X, Y = _trunc(5.0 * p[:, 0] + .5), _trunc(5.0 * p[:, 1] + .5)
    X1, Y1 = np.roll(X, -1), np.roll(Y, -1)
    dx, dy = np.abs(X1 - X), np.abs(Y1 - Y)
    n = np.maximum(dx, dy) + 1                                   # points per edge
    xmajor = dx >= dy
    flip = np.where(xmajor, X > X1, Y > Y1)
    xs, xe = np.where(flip, X1, X), np.where(flip, X, X1)
    ys, ye = np.where(flip, Y1, Y), np.where(flip, Y, Y1)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(xmajor, (ye - ys).astype(np.float64) / dx, (xe - xs).astype(np.float64) / dy)
    e = np.repeat(np.arange(k), n)                               # edge of every point
    d = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    t = np.where(flip[e], n[e] - 1 - d, d)
    with np.errstate(invalid="ignore"):
        minor_x = _trunc(xs[e].astype(np.float64) + s[e] * t.astype(np.float64) + .5)
        minor_y = _trunc(ys[e].astype(np.float64) + s[e] * t.astype(np.float64) + .5)
    u = np.where(xmajor[e], t + xs[e], minor_x)
    v = np.where(xmajor[e], minor_y, t + ys[e])
    u0, u1, v0, v1 = u[:-1], u[1:], v[:-1], v[1:]
    xd = np.where(u1 < u0, u1, u1 - 1).astype(np.float64)
    xd = (xd + .5) / 5.0 - .5
    keep = (u1 != u0) & (np.floor(xd) == xd) & (xd >= 0) & (xd <= float(w - 1))
    yd = np.minimum(v0, v1).astype(np.float64)
    yd = np.ceil(np.clip((yd + .5) / 5.0 - .5, 0.0, float(h)))
    return (xd[keep].astype(np.int64) * h + yd[keep].astype(np.int64)), int(n.sum())


def counts_from_toggles(tog, hw):
    return np.diff(np.concatenate([[0], np.asarray(tog, np.int64), [hw]])).astype(np.uint32)


def poly_counts(xy, h, w):
    """rleFrPoly: the uint32 counts of one polygon in an h x w image."""
    keys, _ = poly_keys(xy, h, w)
    vals, mult = np.unique(keys, return_counts=True)
    return counts_from_toggles(vals[(mult % 2 == 1) & (vals < h * w)], h * w)


def merge(rles, intersect=False):
    """rleMerge on a list of (counts, h, w) with canonical members: (counts, h, w)."""
    if len(rles) == 0:
        return np.zeros(0, np.uint32), 0, 0
    c0, h, w = rles[0]
    if len(rles) == 1:
        return np.asarray(c0, np.uint32).copy(), h, w
    if any((hh, ww) != (h, w) for _, hh, ww in rles[1:]):
        return np.zeros(0, np.uint32), 0, 0
    togs = [np.cumsum(np.asarray(c, np.int64))[:-1] for c, _, _ in rles]
    pos = np.unique(np.concatenate(togs))
    pos = pos[pos < h * w]
    # member i is set after position x iff an odd number of its toggles is <= x
    state = np.stack([np.searchsorted(t, pos, side="right") % 2 == 1 for t in togs])
    covered = state.all(0) if intersect else state.any(0)
    change = covered != np.concatenate([[False], covered[:-1]])
    return counts_from_toggles(pos[change], h * w), h, w


def ann_to_rle(ann, image_sizes):
    """COCO.annToRLE: (counts, h, w) of one annotation."""
    segm = ann["segmentation"]
    if isinstance(segm, list):
        h, w = image_sizes[ann["image_id"]]
        return merge([(poly_counts(p, h, w), h, w) for p in segm])
    return cocoeval_ref.to_rle(segm)


def with_rle_segmentations(annotations, image_sizes):
    """The annotations with every 'segmentation' as an uncompressed RLE (what COCOeval._toMask leaves behind)."""
    out = []
    for a in annotations:
        c, h, w = ann_to_rle(a, image_sizes)
        out.append(dict(a, segmentation={"size": [int(h), int(w)], "counts": [int(v) for v in c]}))
    return out


def golden_counts(golden, key):
    """The uint32 counts of every RLE string that the golden stores under `key`."""
    strings, lens = golden[key + "strings"], golden[key + "str_len"]
    return [cocoeval_ref.rle_from_string(s.tobytes()) for s in np.split(strings, np.cumsum(lens)[:-1])]


def stats(counts, h, w):
    """(maskUtils.area, maskUtils.toBbox) of one RLE."""
    return cocoeval_ref.rle_area(counts), np.asarray(cocoeval_ref.rle_to_bbox(counts, h, w), np.float64)
