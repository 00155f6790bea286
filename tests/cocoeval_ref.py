"""NumPy restatement of the reference's COCO detection evaluation, for the tests and the probe.

Restates datasets/eval/common/maskApi.c (`rleFrString` :217-230, `rleArea` :72-75, `rleToBbox` :133-146, `bbIou`
:109-120, `rleIou` :77-96), pycocotools/coco.py `loadRes` (:292-356) and pycocotools/cocoeval.py `evaluate`,
`evaluateImg`, `accumulate`, `_summarizeDets` with the `Params` defaults (useCats = 1).  `evaluate` returns the
canonical flat form that scripts/gen_golden_cocoeval.py also extracts from the reference's own COCOeval object
(tests/golden/cocoeval.npz)."""
import copy

import numpy as np

IOU_THRS = np.linspace(.5, 0.95, 10, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, 101, endpoint=True)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
BIG = ("ious", "dt_ids", "gt_ids", "dt_matches", "gt_matches", "dt_scores", "gt_ignore", "dt_ignore", "precision",
       "scores")


def rle_from_string(s):
    cnts = []
    p = 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = s[p] - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x & 0xFFFFFFFF)
    return np.array(cnts, np.uint32)


def rle_area(cnts):
    return int(np.asarray(cnts, np.uint64)[1::2].sum() & 0xFFFFFFFF)


def rle_to_bbox(cnts, h, w):
    M = 0xFFFFFFFF
    m = (len(cnts) // 2) * 2
    if m == 0:
        return [0.0, 0.0, 0.0, 0.0]
    xs, ys, xe, ye, cc = w, h, 0, 0, 0
    for j in range(m):
        cc = (cc + int(cnts[j])) & M
        t = (cc - j % 2) & M
        y = t % h
        x = (t - y) // h
        xs, xe, ys, ye = min(xs, x), max(xe, x), min(ys, y), max(ye, y)
    return [float(xs), float(ys), float((xe - xs + 1) & M), float((ye - ys + 1) & M)]


def bb_iou(dt, gt, iscrowd):
    o = np.zeros((len(dt), len(gt)))
    for g, G in enumerate(gt):
        ga = G[2] * G[3]
        for d, D in enumerate(dt):
            da = D[2] * D[3]
            w = min(D[2] + D[0], G[2] + G[0]) - max(D[0], G[0])
            if w <= 0:
                continue
            h = min(D[3] + D[1], G[3] + G[1]) - max(D[1], G[1])
            if h <= 0:
                continue
            i = w * h
            u = da if iscrowd[g] else da + ga - i
            o[d, g] = np.float64(i) / np.float64(u)
    return o


def rle_iou(dt, gt, iscrowd):
    """dt, gt: lists of (counts, h, w)."""
    M = 0xFFFFFFFF
    o = bb_iou([rle_to_bbox(*r) for r in dt], [rle_to_bbox(*r) for r in gt], iscrowd)
    for g, (gc, gh, gw) in enumerate(gt):
        for d, (dc, dh, dw) in enumerate(dt):
            if not o[d, g] > 0:
                continue
            if dh != gh or dw != gw:
                o[d, g] = -1
                continue
            ca, ka, cb, kb = int(dc[0]), len(dc), int(gc[0]), len(gc)
            va = vb = 0
            a = b = 1
            i = u = 0
            ct = 1
            while ct > 0:
                c = min(ca, cb)
                if va or vb:
                    u = (u + c) & M
                    if va and vb:
                        i = (i + c) & M
                ct = 0
                ca -= c
                if not ca and a < ka:
                    ca = int(dc[a])
                    a += 1
                    va = not va
                ct = (ct + ca) & M
                cb -= c
                if not cb and b < kb:
                    cb = int(gc[b])
                    b += 1
                    vb = not vb
                ct = (ct + cb) & M
            if i == 0:
                u = 1
            elif iscrowd[g]:
                u = rle_area(dc)
            o[d, g] = np.float64(i) / np.float64(u)
    return o


def to_rle(segm):
    """annToRLE for an uncompressed RLE or a COCO string: (counts uint32, h, w)."""
    h, w = segm["size"]
    c = segm["counts"]
    if isinstance(c, (bytes, str)):
        c = rle_from_string(c.encode("ascii") if isinstance(c, str) else c)
    return np.asarray(c, np.uint32), int(h), int(w)


def load_res(results):
    """coco.py loadRes on a list of result dicts (copied): ids 1.., area, bbox, iscrowd."""
    anns = copy.deepcopy(results)
    if not anns:
        return anns                              # the reference raises on anns[0]; here: no detections
    if "bbox" in anns[0] and not anns[0]["bbox"] == []:
        for i, a in enumerate(anns):
            bb = a["bbox"]
            a["area"] = bb[2] * bb[3]
            a["id"] = i + 1
            a["iscrowd"] = 0
    elif "segmentation" in anns[0]:
        for i, a in enumerate(anns):
            r = to_rle(a["segmentation"])
            a["area"] = rle_area(r[0])
            if "bbox" not in a:
                a["bbox"] = rle_to_bbox(*r)
            a["id"] = i + 1
            a["iscrowd"] = 0
    return anns


def evaluate(annotations, results, image_ids, category_ids, iou_type="bbox", iou_thrs=IOU_THRS, rec_thrs=REC_THRS,
             max_dets=MAX_DETS, area_rng=AREA_RNG):
    """COCOeval(gt, gt.loadRes(results), iou_type): evaluate(), accumulate(), summarize() in the canonical form."""
    img_ids = list(np.unique(image_ids))
    cat_ids = list(np.unique(category_ids))
    iset, cset = set(img_ids), set(cat_ids)
    gts, dts = {}, {}
    for src, dst in ((annotations, gts), (load_res(results), dts)):
        for a in src:
            if a["image_id"] in iset and a["category_id"] in cset:
                dst.setdefault((a["image_id"], a["category_id"]), []).append(a)
    T, R, K, A, M = len(iou_thrs), len(rec_thrs), len(cat_ids), len(area_rng), len(max_dets)
    max_det = max_dets[-1]
    out = {k: [] for k in BIG[:8]}
    out["iou_keys"], out["ev_keys"] = [], []
    ious = {}
    for i, img in enumerate(img_ids):
        for k, cat in enumerate(cat_ids):
            gt, dt = gts.get((img, cat), []), dts.get((img, cat), [])
            if not gt and not dt:
                continue
            inds = np.argsort([-d["score"] for d in dt], kind="mergesort")
            dt = [dt[j] for j in inds][:max_det]
            crowd = [int(g["iscrowd"]) for g in gt]
            if not gt or not dt:
                ious[img, cat] = np.zeros((0, 0))
            elif iou_type == "segm":
                ious[img, cat] = rle_iou([to_rle(d["segmentation"]) for d in dt],
                                         [to_rle(g["segmentation"]) for g in gt], crowd)
            else:
                ious[img, cat] = bb_iou([d["bbox"] for d in dt], [g["bbox"] for g in gt], crowd)
            if ious[img, cat].size:
                out["iou_keys"].append((img, cat, len(dt), len(gt)))
                out["ious"].append(ious[img, cat].ravel())
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    for k, cat in enumerate(cat_ids):
        for a, rng in enumerate(area_rng):
            E = []
            for i, img in enumerate(img_ids):
                gt, dt = gts.get((img, cat), []), dts.get((img, cat), [])
                if not gt and not dt:
                    continue
                ig = np.array([int(bool(g["iscrowd"]) or g["area"] < rng[0] or g["area"] > rng[1]) for g in gt], int)
                gtind = np.argsort(ig, kind="mergesort")
                gt = [gt[j] for j in gtind]
                ig = ig[gtind]
                dtind = np.argsort([-d["score"] for d in dt], kind="mergesort")
                dt = [dt[j] for j in dtind[:max_det]]
                crowd = [int(g["iscrowd"]) for g in gt]
                iou = ious[img, cat][:, gtind] if ious[img, cat].size else ious[img, cat]
                G, D = len(gt), len(dt)
                gtm, dtm, dtig = np.zeros((T, G)), np.zeros((T, D)), np.zeros((T, D))
                if iou.size:
                    for ti, t in enumerate(iou_thrs):
                        for di in range(D):
                            best, m = min([t, 1 - 1e-10]), -1
                            for gi in range(G):
                                if gtm[ti, gi] > 0 and not crowd[gi]:
                                    continue
                                if m > -1 and ig[m] == 0 and ig[gi] == 1:
                                    break
                                if iou[di, gi] < best:
                                    continue
                                best, m = iou[di, gi], gi
                            if m == -1:
                                continue
                            dtig[ti, di] = ig[m]
                            dtm[ti, di] = gt[m]["id"]
                            gtm[ti, m] = dt[di]["id"]
                out_rng = np.array([d["area"] < rng[0] or d["area"] > rng[1] for d in dt], bool).reshape(1, D)
                dtig = np.logical_or(dtig, np.logical_and(dtm == 0, np.repeat(out_rng, T, 0)))
                sc = np.array([d["score"] for d in dt], np.float64)
                E.append((dtm, dtig, ig, sc))
                out["ev_keys"].append((k, a, i, D, G))
                out["dt_ids"].append(np.array([d["id"] for d in dt], np.float64))
                out["gt_ids"].append(np.array([g["id"] for g in gt], np.float64))
                out["dt_matches"].append(dtm.ravel())
                out["gt_matches"].append(gtm.ravel())
                out["dt_scores"].append(sc)
                out["gt_ignore"].append(ig.astype(np.float64))
                out["dt_ignore"].append(dtig.astype(np.float64).ravel())
            if not E:
                continue
            for m, md in enumerate(max_dets):
                sc = np.concatenate([e[3][:md] for e in E])
                inds = np.argsort(-sc, kind="mergesort")
                sc = sc[inds]
                dtm = np.concatenate([e[0][:, :md] for e in E], axis=1)[:, inds]
                dtig = np.concatenate([e[1][:, :md] for e in E], axis=1)[:, inds]
                npig = np.count_nonzero(np.concatenate([e[2] for e in E]) == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dtig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtig))
                tp_sum = np.cumsum(tps, axis=1).astype(float)
                fp_sum = np.cumsum(fps, axis=1).astype(float)
                for t in range(T):
                    tp, fp = tp_sum[t], fp_sum[t]
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    if nd:
                        pr = np.maximum.accumulate(pr[::-1])[::-1]
                    q, ss = np.zeros(R), np.zeros(R)
                    pi = np.searchsorted(rc, rec_thrs, side="left")
                    ok = pi < nd
                    q[ok] = pr[pi[ok]]
                    ss[ok] = sc[pi[ok]]
                    precision[t, :, k, a, m] = q
                    scores[t, :, k, a, m] = ss
    res = {k: (np.concatenate(v) if v else np.zeros(0)) for k, v in out.items() if k in BIG}
    res["iou_keys"] = np.array(out["iou_keys"], np.int64).reshape(-1, 4)
    res["ev_keys"] = np.array(out["ev_keys"], np.int64).reshape(-1, 5)
    res.update(precision=precision, recall=recall, scores=scores)
    res["stats"] = summarize(precision, recall, iou_thrs, max_dets)
    return res


def summarize(precision, recall, iou_thrs=IOU_THRS, max_dets=MAX_DETS):
    """_summarizeDets: the 12 COCO numbers (area labels all / small / medium / large = indices 0..3)."""
    def one(ap, iou_thr=None, area=0, md=max_dets[-1]):
        mind = [i for i, m in enumerate(max_dets) if m == md]
        s = precision if ap else recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == iou_thrs)[0]]
        s = s[:, :, :, [area], mind] if ap else s[:, :, [area], mind]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
    st = np.zeros(12)
    st[0] = one(1)
    st[1] = one(1, iou_thr=.5)
    st[2] = one(1, iou_thr=.75)
    st[3], st[4], st[5] = one(1, area=1), one(1, area=2), one(1, area=3)
    st[6], st[7], st[8] = one(0, md=max_dets[0]), one(0, md=max_dets[1]), one(0, md=max_dets[2])
    st[9], st[10], st[11] = one(0, area=1), one(0, area=2), one(0, area=3)
    return st


def evaluate_case(case, iou_type, **kw):
    """`evaluate` on a case of tests/cocoeval_cases.py."""
    return evaluate(case["annotations"], case["results"], [i for i, _, _ in case["images"]], case["categories"],
                    iou_type, **kw)


def canonical_from(ev):
    """The canonical flat form from a feature_intertwiner_amd.cocoeval.Evaluation, through its public accessors."""
    out = {k: [] for k in BIG[:8]}
    iou_keys, ev_keys = [], []
    A = len(ev.params.area_rng)
    for img in ev.img_ids:
        for cat in ev.cat_ids:
            m = ev.ious(int(img), int(cat))
            if len(m):
                iou_keys.append((img, cat) + m.shape)
                out["ious"].append(m.ravel())
    for k, cat in enumerate(ev.cat_ids):
        for a in range(A):
            for i, img in enumerate(ev.img_ids):
                e = ev.matches(int(img), int(cat), a)
                if e is None:
                    continue
                ev_keys.append((k, a, i, len(e["dtIds"]), len(e["gtIds"])))
                out["dt_ids"].append(np.asarray(e["dtIds"], np.float64))
                out["gt_ids"].append(np.asarray(e["gtIds"], np.float64))
                out["dt_matches"].append(e["dtMatches"].ravel())
                out["gt_matches"].append(e["gtMatches"].ravel())
                out["dt_scores"].append(np.asarray(e["dtScores"], np.float64))
                out["gt_ignore"].append(e["gtIgnore"].astype(np.float64))
                out["dt_ignore"].append(e["dtIgnore"].astype(np.float64).ravel())
    res = {k: (np.concatenate(v) if v else np.zeros(0)) for k, v in out.items()}
    res["iou_keys"] = np.array(iou_keys, np.int64).reshape(-1, 4)
    res["ev_keys"] = np.array(ev_keys, np.int64).reshape(-1, 5)
    res.update(precision=ev.precision, recall=ev.recall, scores=ev.scores, stats=ev.stats)
    return res


def assert_equal_golden(got, golden, key, large=False):
    """Raw uint64 equality of every array of the canonical form with the golden (SHA-256 for the large case)."""
    import hashlib
    for name in BIG + ("iou_keys", "ev_keys", "recall", "stats"):
        v = np.ascontiguousarray(got[name])
        if large and name in BIG + ("iou_keys", "ev_keys"):
            assert hashlib.sha256(v.tobytes()).hexdigest() == str(golden[key + name + "_sha256"]), (key, name)
            continue
        exp = golden[key + name]
        assert v.shape == exp.shape and v.dtype == exp.dtype, (key, name, v.shape, exp.shape, v.dtype, exp.dtype)
        bits = np.uint64 if v.dtype == np.float64 else v.dtype
        bad = np.flatnonzero(v.view(bits).ravel() != exp.view(bits).ravel())
        assert bad.size == 0, (key, name, bad[:8], v.ravel()[bad[:8]], exp.ravel()[bad[:8]])
