"""COCO detection evaluation on the GPU: what the reference's test_model does after the result dicts
(lib/workflow.py:453-470): `loadRes`, `COCOeval(gt, dt, iouType).evaluate()`, `accumulate()`, `summarize()`.

iouType 'bbox' and 'segm' with the reference's `Params` defaults (pycocotools/cocoeval.py:501-510, useCats = 1).  IoU,
greedy matching, the tp / fp prefix sums, the precision envelope and the recall lookup are the kernels of
csrc/cocoeval.hip (include/fi_cocoeval.h); this module packs the dicts into device arrays, orders them (stable
`torch.sort` on device tensors) and reads the result tables back.  Every number is bit-equal to the reference's
(tests/golden/cocoeval.npz).  Decisions where the reference raises or misbehaves are in DESIGN.md §2."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import FiError, check, current_stream

LIB_PATH = _lib.sublibrary_path("cocoeval")
_p, _i, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
# name -> (restype, argtypes); mirrors include/fi_cocoeval.h one to one
SIGNATURES = {
    "fi_coco_rle_stats": (_i, [_p, _p, _ll, _p, _p, _p]),
    "fi_coco_iou": (_i, [_ll, _p, _p, _p, _ll] + [_p] * 9 + [_p]),
    "fi_coco_match_workspace_bytes": (ctypes.c_size_t, [_ll, _i]),
    "fi_coco_match": (_i, [_ll] + [_p] * 11 + [_i, _i] + [_p] * 5 + [_p]),
    "fi_coco_accumulate": (_i, [_i] + [_p] * 10 + [_i] * 4 + [_p] * 3 + [_p]),
}


def load():
    """Load libfi_cocoeval.so (after libfi_hip.so, which it links against) and attach the signatures."""
    return _lib.load_sublibrary("cocoeval", SIGNATURES)


class Params:
    """pycocotools/cocoeval.py:501-510 `setDetParams` (useCats = 1)."""

    def __init__(self):
        self.iou_thrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.rec_thrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.max_dets = [1, 10, 100]
        self.area_rng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
        self.area_lbl = ['all', 'small', 'medium', 'large']


def rle_from_string(s):
    """rleFrString (datasets/eval/common/maskApi.c:217-230): the uint32 counts of a COCO RLE string."""
    b = np.frombuffer(s.encode("ascii") if isinstance(s, str) else bytes(s), np.uint8).astype(np.int64) - 48
    if b.size == 0:
        return np.zeros(0, np.uint32)
    last = (b & 0x20) == 0                                   # the last character of each number
    if not last[-1]:
        raise FiError("rle_from_string: the string ends inside a number")
    start = np.concatenate([[0], np.flatnonzero(last)[:-1] + 1])
    k = np.arange(b.size) - np.repeat(start, np.diff(np.concatenate([start, [b.size]])))
    if k.max() > 11:
        raise FiError("rle_from_string: a number of more than 12 characters")
    x = np.add.reduceat((b & 0x1f) << (5 * k), start)
    end = np.flatnonzero(last)
    x = np.where(b[end] & 0x10, x | (-1 << (5 * (k[end] + 1))), x)
    # counts m > 2 are coded as differences to cnts[m - 2]
    c = x.copy()
    c[2::2] = np.cumsum(x[2::2])
    c[1::2] = np.cumsum(x[1::2])
    return (c & 0xFFFFFFFF).astype(np.uint32)


def _segm_counts(segm, what):
    if not isinstance(segm, dict) or "counts" not in segm or "size" not in segm:
        raise FiError("%s: 'segmentation' must be an uncompressed RLE {'size', 'counts'} or a COCO RLE string; "
                      "polygons are converted only by pack_ground_truth(..., image_sizes=...) / load_ground_truth "
                      "(cocomask.ann_to_rle)" % what)
    c = segm["counts"]
    c = rle_from_string(c) if isinstance(c, (bytes, str)) else np.asarray(c, np.int64).astype(np.uint32)
    h, w = (int(v) for v in segm["size"])
    if c.size >= 2 and (h < 1 or w < 1):
        raise FiError("%s: an RLE with runs needs a size of at least 1 x 1 (got %d x %d)" % (what, h, w))
    return c, h, w


def _device(device):
    if not torch.cuda.is_available():
        raise FiError("COCO evaluation runs on the GPU only; there is no CPU fallback")
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


_DUMMY = {}


def ptr(t):
    """Device pointer of a tensor (None -> NULL); an empty tensor gives a valid 16-byte buffer, not NULL."""
    if t is None:
        return None
    if t.numel() == 0:
        if t.device not in _DUMMY:
            _DUMMY[t.device] = torch.zeros(16, dtype=torch.uint8, device=t.device)
        t = _DUMMY[t.device]
    return ctypes.c_void_p(t.data_ptr())


def _up(a, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(dev, non_blocking=False)


class Packed:
    """Device-resident annotations.  Host: image_id, category_id [n] int64.  Device: box [n, 4], area [n] fp64,
    ann_id [n] int64, crowd [n] uint8, score [n] fp64 and, with segmentations, rles [n, 4] int64, counts (uint32 as
    int32), rle_box [n, 4], rle_area [n]."""
    rles = counts = rle_box = rle_area = None
    image_ids = category_ids = None


def _pack(L, dev, image_id, category_id, box, area, ann_id, crowd, score, rle_list, area_from_rle, box_from_rle):
    P = Packed()
    n = len(image_id)
    P.n, P.device = n, dev
    P.image_id = np.asarray(image_id, np.int64).reshape(n)
    P.category_id = np.asarray(category_id, np.int64).reshape(n)
    P.ann_id = _up(np.asarray(ann_id, np.int64).reshape(n), torch.int64, dev)
    P.crowd = _up(np.asarray(crowd, np.uint8).reshape(n), torch.uint8, dev)
    P.score = _up(np.asarray(score, np.float64).reshape(n), torch.float64, dev)
    P.box = _up(np.asarray(box, np.float64).reshape(n, 4), torch.float64, dev)
    P.area = _up(np.asarray(area, np.float64).reshape(n), torch.float64, dev)
    if rle_list is not None:
        if isinstance(rle_list, tuple):                       # already on the device: cocomask.ann_to_rle
            P.rles, P.counts = rle_list
        else:
            lens = np.array([c.size for c, _, _ in rle_list], np.int64)
            desc = np.zeros((n, 4), np.int64)
            desc[:, 0] = np.cumsum(lens) - lens
            desc[:, 1] = lens
            desc[:, 2:] = np.array([(h, w) for _, h, w in rle_list], np.int64).reshape(n, 2)
            flat = np.concatenate([c for c, _, _ in rle_list] + [np.zeros(1, np.uint32)])
            P.rles = _up(desc, torch.int64, dev)
            P.counts = _up(flat.view(np.int32), torch.int32, dev)
        P.rle_box = torch.empty(n, 4, dtype=torch.float64, device=dev)
        P.rle_area = torch.empty(n, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            check(L.fi_coco_rle_stats(ptr(P.counts), ptr(P.rles), n, ptr(P.rle_box), ptr(P.rle_area),
                                      current_stream()), "fi_coco_rle_stats")
        if area_from_rle:                                     # loadRes: maskUtils.area
            P.area = P.rle_area
        if box_from_rle is not None:                          # loadRes: maskUtils.toBbox where 'bbox' is absent
            m = _up(np.asarray(box_from_rle, bool), torch.bool, dev)
            P.box = torch.where(m[:, None], P.rle_box, P.box)
    return P


def pack_ground_truth(annotations, image_ids, category_ids, device=None, image_sizes=None):
    """The ground truth of COCOeval: a list of COCO annotation dicts ('id', 'image_id', 'category_id', 'bbox',
    'area', 'iscrowd' and, for segm, 'segmentation' as a polygon list, an uncompressed RLE or a COCO string) and the
    image and category ids of the data set (COCO.getImgIds() / getCatIds()).  Polygons need `image_sizes`, a dict
    image id -> (height, width); they are converted on the GPU as COCO.annToRLE does (cocomask.ann_to_rle).
    Returns a device-resident, reusable object."""
    L = load()
    dev = _device(device)
    anns = list(annotations)
    ids = np.array([a["id"] for a in anns], np.int64)
    if (ids == 0).any():
        raise FiError("pack_ground_truth: an annotation id of 0 (0 is 'no match' in dtMatches / gtMatches)")
    seg = [("segmentation" in a) for a in anns]
    if any(seg) and not all(seg):
        raise FiError("pack_ground_truth: some annotations have a 'segmentation' and some have none")
    rl = None
    if anns and all(seg):
        if any(isinstance(a["segmentation"], (list, tuple)) for a in anns):
            if image_sizes is None:
                raise FiError("pack_ground_truth: polygons in 'segmentation' need image_sizes = {image id: (height, "
                              "width)} (or load_ground_truth on the whole data set)")
            from . import cocomask
            rl = cocomask.ann_to_rle(anns, image_sizes, dev)
        else:
            rl = [_segm_counts(a["segmentation"], "pack_ground_truth") for a in anns]
    P = _pack(L, dev, [a["image_id"] for a in anns], [a["category_id"] for a in anns],
              [a["bbox"] for a in anns], [a["area"] for a in anns], ids,
              [1 if a.get("iscrowd") else 0 for a in anns], np.zeros(len(anns)), rl, False, None)
    P.image_ids = np.unique(np.asarray(list(image_ids), np.int64))
    P.category_ids = np.unique(np.asarray(list(category_ids), np.int64))
    return P


def load_ground_truth(source, device=None):
    """pack_ground_truth of a whole COCO data set: `source` is the path of an instances_*.json or the loaded dict.
    Image sizes come from 'images'; image and category ids are those of COCO.getImgIds() / getCatIds()."""
    if isinstance(source, dict):
        data = source
    else:
        import json
        with open(source) as f:
            data = json.load(f)
    for key in ("images", "categories", "annotations"):
        if key not in data:
            raise FiError("load_ground_truth: the data set has no %r" % key)
    sizes = {im["id"]: (im["height"], im["width"]) for im in data["images"]}
    return pack_ground_truth(data["annotations"], list(sizes), [c["id"] for c in data["categories"]], device, sizes)


def pack_results(results, device=None):
    """`COCO.loadRes` (pycocotools/coco.py:292-356) on the dicts of postprocess.coco_results: ids are 1-based in
    list order; if the first result has a 'bbox', area = w * h for all; otherwise area = rleArea and a missing bbox
    = rleToBbox of the 'segmentation'.  An empty list is "no detections" (DESIGN.md §2)."""
    L = load()
    dev = _device(device)
    res = list(results)
    n = len(res)
    by_box = n > 0 and "bbox" in res[0] and not list(res[0]["bbox"]) == []
    if n and not by_box and "segmentation" not in res[0]:
        raise FiError("pack_results: results need a 'bbox' or a 'segmentation'")
    seg = [("segmentation" in r) for r in res]
    rl = [_segm_counts(r["segmentation"], "pack_results") for r in res] if n and all(seg) else None
    if by_box:
        box = [r["bbox"] for r in res]
        area = [r["bbox"][2] * r["bbox"][3] for r in res]
        from_rle = None
    else:
        box = [r.get("bbox", [0, 0, 0, 0]) for r in res]
        area = np.zeros(n)
        from_rle = [("bbox" not in r) for r in res]
    return _pack(L, dev, [r["image_id"] for r in res], [r["category_id"] for r in res], box, area,
                 np.arange(1, n + 1), np.zeros(n), [r["score"] for r in res], rl, n > 0 and not by_box, from_rle)


def _summarize(precision, recall, P, ap, iou_thr=None, area='all', max_dets=100):
    """`_summarize` of pycocotools/cocoeval.py:425-455 without the printing."""
    aind = [i for i, a in enumerate(P.area_lbl) if a == area]
    mind = [i for i, m in enumerate(P.max_dets) if m == max_dets]
    s = precision if ap == 1 else recall
    if iou_thr is not None:
        s = s[np.where(iou_thr == P.iou_thrs)[0]]
    s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
    return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])


_STAT_ROWS = lambda md: [(1, None, 'all', md[-1]), (1, .5, 'all', md[-1]), (1, .75, 'all', md[-1]),      # noqa: E731
                         (1, None, 'small', md[-1]), (1, None, 'medium', md[-1]), (1, None, 'large', md[-1]),
                         (0, None, 'all', md[0]), (0, None, 'all', md[1]), (0, None, 'all', md[-1]),
                         (0, None, 'small', md[-1]), (0, None, 'medium', md[-1]), (0, None, 'large', md[-1])]


class Evaluation:
    """The result of `evaluate`: precision [T, R, K, A, M], recall [T, K, A, M], scores [T, R, K, A, M] (fp64, as
    COCOeval.eval), `stats` (the 12 numbers of `_summarizeDets`), `summary()`, and for inspection
    `matches(image_id, category_id, area_index)` and `ious(image_id, category_id)`."""

    def summary(self):
        """The 12 lines that COCOeval.summarize prints."""
        P = self.params
        if self.stats is None:
            raise FiError("summary() needs three maxDets, as COCOeval.summarize does")
        lines = []
        for (ap, thr, area, md), v in zip(_STAT_ROWS(P.max_dets), self.stats):
            iou = '{:0.2f}:{:0.2f}'.format(P.iou_thrs[0], P.iou_thrs[-1]) if thr is None else '{:0.2f}'.format(thr)
            lines.append(' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'.format(
                'Average Precision' if ap == 1 else 'Average Recall', '(AP)' if ap == 1 else '(AR)', iou, area, md, v))
        return "\n".join(lines)

    def _pair(self, image_id, category_id):
        i = np.searchsorted(self.img_ids, image_id)
        k = np.searchsorted(self.cat_ids, category_id)
        if i >= len(self.img_ids) or k >= len(self.cat_ids) or self.img_ids[i] != image_id or \
                self.cat_ids[k] != category_id:
            return None
        key = k * len(self.img_ids) + i
        p = int(np.searchsorted(self.pairs, key))
        return p if p < len(self.pairs) and self.pairs[p] == key else None

    def _host(self):
        if self._h is None:                                   # one download, on first inspection
            self._h = {k: v.cpu().numpy() for k, v in self._dev.items()}
        return self._h

    def ious(self, image_id, category_id):
        """COCOeval.ious[image_id, category_id]: fp64 [D, G], or [] where either side is empty."""
        p = self._pair(image_id, category_id)
        if p is None:
            return []
        D, G = int(self.dt_off[p + 1] - self.dt_off[p]), int(self.gt_off[p + 1] - self.gt_off[p])
        if D == 0 or G == 0:
            return []
        return self._host()["ious"][self.iou_off[p]:self.iou_off[p + 1]].reshape(D, G)

    def matches(self, image_id, category_id, area_index):
        """The evalImgs entry of (category, area range, image) (cocoeval.py:299-311), None where the pair has neither
        ground truths nor detections."""
        p = self._pair(image_id, category_id)
        if p is None:
            return None
        h = self._host()
        T, A, a = len(self.params.iou_thrs), len(self.params.area_rng), area_index
        d0, d1, g0, g1 = (int(v) for v in (self.dt_off[p], self.dt_off[p + 1], self.gt_off[p], self.gt_off[p + 1]))
        G = g1 - g0
        gtind = h["gt_order"][g0 * A + a * G:g0 * A + (a + 1) * G].astype(np.int64)
        return {"image_id": image_id, "category_id": category_id, "aRng": self.params.area_rng[a],
                "maxDet": self.params.max_dets[-1], "dtIds": h["dt_id"][d0:d1], "gtIds": h["gt_id"][g0:g1][gtind],
                "dtMatches": h["dt_match"][d0:d1, a, :].T.astype(np.float64),
                "gtMatches": h["gt_match"][g0:g1, a, :][gtind].T.astype(np.float64),
                "dtScores": h["dt_score"][d0:d1], "gtIgnore": h["gt_ignore"][g0:g1, a][gtind].astype(np.int64),
                "dtIgnore": h["dt_ignore"][d0:d1, a, :].T.astype(bool)}


def _index(packed, img_ids, cat_ids):
    """Rows of `packed` inside the evaluated images and categories, and their (category, image) key."""
    if packed.n == 0 or len(img_ids) == 0 or len(cat_ids) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    ii = np.minimum(np.searchsorted(img_ids, packed.image_id), len(img_ids) - 1)
    kk = np.minimum(np.searchsorted(cat_ids, packed.category_id), len(cat_ids) - 1)
    sel = np.flatnonzero((img_ids[ii] == packed.image_id) & (cat_ids[kk] == packed.category_id))
    return sel, kk[sel] * len(img_ids) + ii[sel]


def _scan(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def evaluate(gt, dt, iou_type="bbox", img_ids=None, params=None):
    """COCOeval(gt, dt, iou_type) with params.imgIds = img_ids (default: every image of the ground truth):
    evaluate(), accumulate() and summarize().  `gt` / `dt` come from pack_ground_truth / pack_results.  Runs on the
    current stream of the ground truth's device; the one host synchronisation reads the result tables."""
    L = load()
    if not isinstance(gt, Packed) or not isinstance(dt, Packed) or gt.image_ids is None:
        raise FiError("evaluate needs pack_ground_truth(...) and pack_results(...) objects")
    if iou_type not in ("bbox", "segm"):
        raise FiError("iou_type must be 'bbox' or 'segm' (got %r)" % (iou_type,))
    P = params if params is not None else Params()
    dev = gt.device
    if dt.device != dev:
        raise FiError("ground truth on %s, results on %s" % (dev, dt.device))
    if dt.n and not np.isin(dt.image_id, gt.image_ids).all():
        raise FiError("Results do not correspond to current coco set (an image_id that the ground truth lacks)")
    segm = iou_type == "segm"
    if segm and ((gt.n and gt.rles is None) or (dt.n and dt.rles is None)):
        raise FiError("iou_type 'segm' needs a 'segmentation' (RLE) in every annotation and result")
    img_ids = np.unique(np.asarray(gt.image_ids if img_ids is None else list(img_ids), np.int64))
    cat_ids = gt.category_ids
    T, R, K, A, M = len(P.iou_thrs), len(P.rec_thrs), len(cat_ids), len(P.area_rng), len(P.max_dets)
    if T < 1 or R < 1 or A < 1 or M < 1:
        raise FiError("evaluate needs at least one iou threshold, recall threshold, area range and maxDets")
    max_dets = sorted(int(m) for m in P.max_dets)
    I = len(img_ids)
    gsel, gkey = _index(gt, img_ids, cat_ids)
    dsel, dkey = _index(dt, img_ids, cat_ids)
    pairs = np.unique(np.concatenate([gkey, dkey]))
    NP = len(pairs)
    gpair, dpair = np.searchsorted(pairs, gkey), np.searchsorted(pairs, dkey)
    gcnt = np.bincount(gpair, minlength=NP).astype(np.int64)
    dfull = np.bincount(dpair, minlength=NP).astype(np.int64)
    dcnt = np.minimum(dfull, max_dets[-1])
    gt_off, dt_off, full_off, iou_off = _scan(gcnt), _scan(dcnt), _scan(dfull), _scan(dcnt * gcnt)
    NG, ND, E = int(gt_off[-1]), int(dt_off[-1]), int(iou_off[-1])
    pair_k = pairs // max(I, 1)
    cat_dt_off = _scan(np.bincount(pair_k, weights=dcnt, minlength=K)[:K])
    cat_gt_off = _scan(np.bincount(pair_k, weights=gcnt, minlength=K)[:K])
    dt_rank = np.arange(ND, dtype=np.int64) - np.repeat(dt_off[:-1], dcnt)
    take = np.repeat(full_off[:-1], dcnt) + dt_rank                # the first maxDets[-1] of every pair
    i64, f64, u8 = torch.int64, torch.float64, torch.uint8
    with torch.cuda.device(dev):
        st = current_stream()
        up = lambda a, t=i64: _up(a, t, dev)                                                     # noqa: E731
        # detections by (pair, descending score), stable: argsort(-score, kind='mergesort') of cocoeval.py:171
        dsel_t = up(dsel)
        o1 = torch.sort(dt.score[dsel_t], descending=True, stable=True).indices
        o2 = torch.sort(up(dpair)[o1], stable=True).indices
        didx = dsel_t[o1[o2][up(take)]]
        gidx = up(gsel[np.argsort(gpair, kind="stable")])
        d = {"dt_id": dt.ann_id[didx], "dt_score": dt.score[didx], "gt_id": gt.ann_id[gidx]}
        dt_area, gt_area, gt_crowd = dt.area[didx], gt.area[gidx], gt.crowd[gidx].contiguous()
        dt_off_t, gt_off_t, iou_off_t = up(dt_off), up(gt_off), up(iou_off)
        d["ious"] = torch.empty(max(E, 1), dtype=f64, device=dev)[:E]
        if segm:
            rle_args = [dt.rles[didx].contiguous(), dt.counts, dt.rle_area[didx].contiguous(),
                        gt.rles[gidx].contiguous(), gt.counts]
            dbox, gbox = dt.rle_box[didx].contiguous(), gt.rle_box[gidx].contiguous()
        else:
            rle_args = [None] * 5
            dbox, gbox = dt.box[didx].contiguous(), gt.box[gidx].contiguous()
        check(L.fi_coco_iou(NP, ptr(dt_off_t), ptr(gt_off_t), ptr(iou_off_t), E, ptr(dbox), ptr(gbox), ptr(gt_crowd),
                            *[ptr(t) for t in rle_args], ptr(d["ious"]), st), "fi_coco_iou")
        thr_t, rng_t = up(np.asarray(P.iou_thrs, np.float64), f64), up(np.asarray(P.area_rng, np.float64), f64)
        d["dt_match"] = torch.empty(ND, A, T, dtype=i64, device=dev)
        d["dt_ignore"] = torch.empty(ND, A, T, dtype=u8, device=dev)
        d["gt_match"] = torch.empty(NG, A, T, dtype=i64, device=dev)
        d["gt_ignore"] = torch.empty(NG, A, dtype=u8, device=dev)
        d["gt_order"] = torch.empty(max(1, L.fi_coco_match_workspace_bytes(NG, A) // 4), dtype=torch.int32,
                                    device=dev)
        check(L.fi_coco_match(NP, ptr(dt_off_t), ptr(gt_off_t), ptr(iou_off_t), ptr(d["ious"]), ptr(dt_area),
                              ptr(d["dt_id"]), ptr(gt_area), ptr(gt_crowd), ptr(d["gt_id"]), ptr(thr_t), ptr(rng_t),
                              T, A, ptr(d["dt_match"]), ptr(d["dt_ignore"]), ptr(d["gt_match"]), ptr(d["gt_ignore"]),
                              ptr(d["gt_order"]), st), "fi_coco_match")
        # accumulate's order: each category's detections by descending score, stable (cocoeval.py:364)
        a1 = torch.sort(d["dt_score"], descending=True, stable=True).indices
        a2 = torch.sort(up(np.repeat(pair_k, dcnt))[a1], stable=True).indices
        order = a1[a2].contiguous()
        precision = torch.empty(T, R, K, A, M, dtype=f64, device=dev)
        recall = torch.empty(T, K, A, M, dtype=f64, device=dev)
        scores = torch.empty(T, R, K, A, M, dtype=f64, device=dev)
        # named, so that every buffer outlives the launch that reads it
        cdo_t, cgo_t, rank_t = up(cat_dt_off), up(cat_gt_off), up(dt_rank, torch.int32)
        rec_t, md_t = up(np.asarray(P.rec_thrs, np.float64), f64), up(np.asarray(max_dets), torch.int32)
        check(L.fi_coco_accumulate(K, ptr(cdo_t), ptr(cgo_t), ptr(order), ptr(rank_t), ptr(d["dt_score"]),
                                   ptr(d["dt_match"]), ptr(d["dt_ignore"]), ptr(d["gt_ignore"]), ptr(rec_t),
                                   ptr(md_t), T, R, A, M, ptr(precision), ptr(recall), ptr(scores), st),
              "fi_coco_accumulate")
        ev = Evaluation()
        # the one host synchronisation: the result tables
        ev.precision, ev.recall, ev.scores = precision.cpu().numpy(), recall.cpu().numpy(), scores.cpu().numpy()
    ev.params, ev.iou_type = P, iou_type
    ev.img_ids, ev.cat_ids, ev.pairs = img_ids, cat_ids, pairs
    ev.dt_off, ev.gt_off, ev.iou_off = dt_off, gt_off, iou_off
    ev._dev, ev._h = d, None
    pm = Params.__new__(Params)
    pm.__dict__.update(P.__dict__)
    pm.max_dets = max_dets
    ev.params = pm
    if M != 3:                 # _summarizeDets reads maxDets[0..2]: "only for the default parameter setting"
        ev.stats = None
        return ev
    ev.stats = np.array([_summarize(ev.precision, ev.recall, pm, *row) for row in _STAT_ROWS(max_dets)], np.float64)
    return ev
