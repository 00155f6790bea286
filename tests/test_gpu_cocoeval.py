"""GPU: COCO evaluation (csrc/cocoeval.hip, feature_intertwiner_amd/cocoeval.py) is bit-equal to the golden made from
the reference's own COCO / COCOeval / maskApi.c (tests/golden/cocoeval.npz) for bbox and segm, and equal to the NumPy
restatement (tests/cocoeval_ref.py) on shapes that the golden does not hold."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cocoeval_ref as R
from cocoeval_cases import LARGE, cocoeval_cases
from unmold_cases import unmold_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = {c["name"]: c for c in cocoeval_cases()}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "cocoeval.npz"))


def _evaluate(case, iou_type, **kw):
    from feature_intertwiner_amd import cocoeval
    gt = cocoeval.pack_ground_truth(case["annotations"], [i for i, _, _ in case["images"]], case["categories"])
    dt = cocoeval.pack_results(case["results"])
    return cocoeval.evaluate(gt, dt, iou_type, **kw), gt, dt


def _same(got, exp):
    for name in R.BIG + ("iou_keys", "ev_keys", "recall", "stats"):
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(exp[name])
        assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape)
        bits = np.uint64 if a.dtype == np.float64 else a.dtype
        assert np.array_equal(a.view(bits), b.view(bits)), name


@pytest.mark.parametrize("case,iou_type", [(n, t) for n, c in CASES.items() for t in c["types"]])
def test_bit_equal_vs_golden(golden, case, iou_type):
    ev, _, _ = _evaluate(CASES[case], iou_type)
    got = R.canonical_from(ev)
    R.assert_equal_golden(got, golden, "%s/%s/" % (case, iou_type), large=case == LARGE)
    assert len(ev.summary().splitlines()) == 12 and ev.summary().startswith(" Average Precision  (AP) @[ IoU=0.50:0.95")


def test_evaluate_twice_gives_identical_bytes():
    from feature_intertwiner_amd import cocoeval
    for name, iou_type in (("ties", "bbox"), ("segm_unmold", "segm"), (LARGE, "bbox")):
        ev1, gt, dt = _evaluate(CASES[name], iou_type)
        ev2 = cocoeval.evaluate(gt, dt, iou_type)
        for k in ("precision", "recall", "scores", "stats"):
            assert getattr(ev1, k).tobytes() == getattr(ev2, k).tobytes()
        h1, h2 = ev1._host(), ev2._host()
        for k in h1:
            assert h1[k].tobytes() == h2[k].tobytes(), k


def test_img_ids_subset_equals_restatement():
    case = CASES["generic"]
    ids = [i for i, _, _ in case["images"]][1:4]
    ev, _, _ = _evaluate(case, "bbox", img_ids=ids)
    _same(R.canonical_from(ev), R.evaluate(case["annotations"], case["results"], ids, case["categories"], "bbox"))


def test_raw_c_entry_points():
    """fi_coco_iou / fi_coco_match / fi_coco_accumulate on the (image 2, category 5) pair of 'edges'."""
    from feature_intertwiner_amd import _lib, cocoeval
    L = cocoeval.load()
    case = CASES["edges"]
    anns = [a for a in case["annotations"] if (a["image_id"], a["category_id"]) == (2, 5)]
    res = [r for r in R.load_res(case["results"]) if (r["image_id"], r["category_id"]) == (2, 5)]
    res = [res[i] for i in np.argsort([-r["score"] for r in res], kind="mergesort")]
    D, G, T, Rn, A, M = len(res), len(anns), 10, 101, 4, 3
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(DEV)          # noqa: E731
    P = _lib.ptr
    st = _lib.current_stream()
    dt_off, gt_off, iou_off = t([0, D], np.int64), t([0, G], np.int64), t([0, D * G], np.int64)
    dbox, gbox = t([r["bbox"] for r in res], np.float64), t([a["bbox"] for a in anns], np.float64)
    crowd = t([a["iscrowd"] for a in anns], np.uint8)
    ious = torch.full((D * G + 4,), -7.0, dtype=torch.float64, device=DEV)
    assert L.fi_coco_iou(1, P(dt_off), P(gt_off), P(iou_off), D * G, P(dbox), P(gbox), P(crowd), *[None] * 5,
                         P(ious), st) == 0
    exp = R.bb_iou([r["bbox"] for r in res], [a["bbox"] for a in anns], [a["iscrowd"] for a in anns])
    host = ious.cpu().numpy()
    assert np.array_equal(host[:D * G].view(np.uint64), exp.ravel().view(np.uint64))
    assert (host[D * G:] == -7.0).all()                                  # nothing past num_elems
    dm = torch.empty(D, A, T, dtype=torch.int64, device=DEV)
    di = torch.empty(D, A, T, dtype=torch.uint8, device=DEV)
    gm = torch.empty(G, A, T, dtype=torch.int64, device=DEV)
    gi = torch.empty(G, A, dtype=torch.uint8, device=DEV)
    assert L.fi_coco_match_workspace_bytes(G, A) == 4 * G * A
    ws = torch.empty(G * A, dtype=torch.int32, device=DEV)
    darea, did = t([r["area"] for r in res], np.float64), t([r["id"] for r in res], np.int64)
    garea, gid = t([a["area"] for a in anns], np.float64), t([a["id"] for a in anns], np.int64)
    thr, rng = t(R.IOU_THRS, np.float64), t(R.AREA_RNG, np.float64)
    assert L.fi_coco_match(1, P(dt_off), P(gt_off), P(iou_off), P(ious), P(darea), P(did), P(garea), P(crowd), P(gid),
                           P(thr), P(rng), T, A, P(dm), P(di), P(gm), P(gi), P(ws), st) == 0
    score = t([r["score"] for r in res], np.float64)
    order, rank = t(np.arange(D), np.int64), t(np.arange(D), np.int32)
    prec = torch.empty(T, Rn, 1, A, M, dtype=torch.float64, device=DEV)
    rec = torch.empty(T, 1, A, M, dtype=torch.float64, device=DEV)
    sco = torch.empty(T, Rn, 1, A, M, dtype=torch.float64, device=DEV)
    rec_thrs, max_dets = t(R.REC_THRS, np.float64), t(R.MAX_DETS, np.int32)
    assert L.fi_coco_accumulate(1, P(dt_off), P(gt_off), P(order), P(rank), P(score), P(dm), P(di), P(gi),
                                P(rec_thrs), P(max_dets), T, Rn, A, M, P(prec), P(rec), P(sco), st) == 0
    ref = R.evaluate(case["annotations"], case["results"], [2], [5], "bbox")
    n = ref["ev_keys"].shape[0]
    assert n == A
    assert np.array_equal(dm.permute(1, 2, 0).cpu().numpy().astype(np.float64).ravel(), ref["dt_matches"])
    assert np.array_equal(di.permute(1, 2, 0).cpu().numpy().astype(np.float64).ravel(), ref["dt_ignore"])
    gtind = ws.cpu().numpy().reshape(A, G)
    gmh = gm.cpu().numpy()
    got_gm = np.concatenate([gmh[gtind[a], a, :].T.ravel() for a in range(A)]).astype(np.float64)
    assert np.array_equal(got_gm, ref["gt_matches"])
    for got, name in ((prec, "precision"), (rec, "recall"), (sco, "scores")):
        assert np.array_equal(got.cpu().numpy().view(np.uint64), ref[name].view(np.uint64)), name


def _unmolded_case():
    """The unmold case 'mixed' on the GPU, with ground truth derived from the same boxes."""
    from feature_intertwiner_amd.postprocess import coco_results, unmold_detections
    name, det, masks, hw, win = [c for c in unmold_cases() if c[0] == "mixed"][0]
    out = unmold_detections(torch.from_numpy(det).to(DEV), torch.from_numpy(masks).to(DEV), hw,
                            torch.from_numpy(win).to(DEV))
    results = coco_results(out, [11, 22], lambda c: 7 * c)
    anns = []
    rs = np.random.RandomState(5)
    for r in results[::2]:
        x, y, w, h = r["bbox"]
        H, W = r["segmentation"]["size"]
        m = np.zeros((H, W), np.uint8)
        m[max(y, 0):y + h, max(x, 0):x + w + int(rs.randint(0, 3))] = 1
        import unmold_ref
        anns.append({"id": 300 + 2 * len(anns), "image_id": r["image_id"], "category_id": r["category_id"],
                     "bbox": [float(x), float(y), float(w + 1), float(h)], "area": float(m.sum()),
                     "iscrowd": int(rs.rand() < 0.1),
                     "segmentation": {"size": [H, W], "counts": unmold_ref.rle_string(unmold_ref.rle_counts(m))}})
    return anns, results


@pytest.mark.parametrize("iou_type", ["bbox", "segm"])
def test_unmold_to_evaluate_equals_restatement(iou_type):
    from feature_intertwiner_amd import cocoeval
    anns, results = _unmolded_case()
    gt = cocoeval.pack_ground_truth(anns, [11, 22], [7, 14, 21, 28])
    ev = cocoeval.evaluate(gt, cocoeval.pack_results(results), iou_type)
    exp = R.evaluate(anns, results, [11, 22], [7, 14, 21, 28], iou_type)
    _same(R.canonical_from(ev), exp)
    assert ev.stats[0] > 0


def test_evaluate_coco_after_a_real_test_step():
    """The synthetic inference of test_gpu_unmold.py, then workflow.evaluate_coco on its result dicts."""
    from feature_intertwiner_amd import cocoeval, workflow
    from feature_intertwiner_amd.config import make_config
    from feature_intertwiner_amd.model import MaskRCNN
    from feature_intertwiner_amd.synthetic import SyntheticProposals, synthetic_batch
    torch.manual_seed(1)
    cfg = make_config("resnet50", 256, 2)
    model = MaskRCNN(cfg).to(DEV)
    batch = synthetic_batch(2, 256, device=DEV)
    model.external_proposals = SyntheticProposals(batch[2], 256)
    K = cfg.DATASET.NUM_CLASSES
    meta = np.zeros((2, 8 + K + 1), np.float32)
    meta[:, 0] = [0, 1]
    meta[:, 1:4] = [[240, 240, 3], [300, 280, 3]]
    meta[:, 4:8] = [[0, 0, 256, 256], [0, 16, 256, 240]]
    meta[:, -1] = [501, 502]
    results, _ = workflow.test_step(model, batch[0], torch.from_numpy(meta), category_map=lambda c: 7 * c)
    assert len(results) > 0
    cats = sorted({r["category_id"] for r in results}) + [7 * (K + 1)]
    anns = [{"id": 40 + j, "image_id": r["image_id"], "category_id": r["category_id"],
             "bbox": [float(v) for v in r["bbox"]], "area": float(r["bbox"][2] * r["bbox"][3]), "iscrowd": j % 7 == 3,
             "segmentation": r["segmentation"]} for j, r in enumerate(results[::3])]
    gt = cocoeval.pack_ground_truth(anns, [501, 502, 503], cats)
    for iou_type in ("bbox", "segm"):
        m_ap, ev = workflow.evaluate_coco(results, gt, iou_type)
        exp = R.evaluate(anns, results, [501, 502, 503], cats, iou_type)
        _same(R.canonical_from(ev), exp)
        assert m_ap == exp["stats"][0] and m_ap > 0


def test_limits():
    """No limit on a pair: 600 ground truths x 150 detections (cut to 100).  T * A is limited to 64."""
    from feature_intertwiner_amd import _lib, cocoeval
    rs = np.random.RandomState(11)
    xy = rs.randint(0, 400, (600, 2))
    wh = rs.randint(5, 60, (600, 2))
    anns = [{"id": 1 + j, "image_id": 1, "category_id": 1, "bbox": [float(v) for v in (*xy[j], *wh[j])],
             "area": float(wh[j, 0] * wh[j, 1]), "iscrowd": int(j % 50 == 7)} for j in range(600)]
    results = [{"image_id": 1, "category_id": 1, "score": np.float32(rs.randint(0, 40) / 40.0),
                "bbox": [float(xy[j * 4, 0] + rs.randint(-3, 4)), float(xy[j * 4, 1]), float(wh[j * 4, 0]),
                         float(wh[j * 4, 1] + rs.randint(-3, 4))]} for j in range(150)]
    gt = cocoeval.pack_ground_truth(anns, [1], [1])
    dt = cocoeval.pack_results(results)
    first = cocoeval.evaluate(gt, dt, "bbox")
    _same(R.canonical_from(first), R.evaluate(anns, results, [1], [1], "bbox"))
    # the documented maximum: T * A = 64 lanes of one wave
    p = cocoeval.Params()
    p.iou_thrs = np.linspace(0.2, 0.95, 16)
    ev = cocoeval.evaluate(gt, dt, "bbox", params=p)
    exp = R.evaluate(anns, results, [1], [1], "bbox", iou_thrs=p.iou_thrs)
    _same(R.canonical_from(ev), exp)
    p.iou_thrs = np.linspace(0.2, 0.95, 17)
    with pytest.raises(_lib.FiError, match="T \\* A <= 64"):
        cocoeval.evaluate(gt, dt, "bbox", params=p)
    p = cocoeval.Params()
    p.rec_thrs = np.linspace(0, 1, 1025)
    with pytest.raises(_lib.FiError, match="R <= 1024"):
        cocoeval.evaluate(gt, dt, "bbox", params=p)
    # the device is still fine afterwards
    assert cocoeval.evaluate(gt, dt, "bbox").precision.tobytes() == first.precision.tobytes()


def test_decided_inputs():
    from feature_intertwiner_amd import _lib, cocoeval
    case = CASES["generic"]
    ids = [i for i, _, _ in case["images"]]
    bad = [dict(case["annotations"][0], id=0)]
    with pytest.raises(_lib.FiError, match="id of 0"):
        cocoeval.pack_ground_truth(bad, ids, case["categories"])
    gt = cocoeval.pack_ground_truth(case["annotations"], ids, case["categories"])
    with pytest.raises(_lib.FiError, match="do not correspond"):
        cocoeval.evaluate(gt, cocoeval.pack_results([dict(case["results"][0], image_id=12345)]))
    with pytest.raises(_lib.FiError, match="segm"):
        cocoeval.evaluate(gt, cocoeval.pack_results(case["results"]), "segm")
    poly = [dict(case["annotations"][0], segmentation=[[1, 1, 5, 1, 5, 5]])]
    with pytest.raises(_lib.FiError, match="polygons"):
        cocoeval.pack_ground_truth(poly, ids, case["categories"])
    ev = cocoeval.evaluate(gt, cocoeval.pack_results([]))                 # an empty result list: no detections
    assert ev.stats[0] == 0 and ev.stats[8] == 0 and ev._host()["dt_id"].size == 0
