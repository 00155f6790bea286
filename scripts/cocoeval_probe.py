"""Timing probe of the GPU COCO evaluation (feature_intertwiner_amd/cocoeval.py) -> profiles/cocoeval_probe.txt.

Runs the large golden case (tests/cocoeval_cases.py) and a val2017-sized synthetic one (5000 images, 80 categories,
100 detections per image) for bbox, and a 500-image rectangle-mask case for segm.  Reports the wall time of pack +
evaluate (upload, kernels, final reads; host clock around a device synchronise), the time of each C entry point from
HIP events around its launch, the number of launches, and the time of the NumPy restatement (tests/cocoeval_ref.py)
on this machine's host.  The reference's own time, recorded in the golden, is from the build machine's CPU.

    python scripts/cocoeval_probe.py [--out profiles/cocoeval_probe.txt] [--no-ref-val]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cocoeval_ref as R  # noqa: E402
import unmold_ref  # noqa: E402
from cocoeval_cases import LARGE, _ann, _detect, _random_boxes, _res, cocoeval_cases  # noqa: E402
from feature_intertwiner_amd import cocoeval  # noqa: E402


def synthetic(n_img, segm=False, seed=5):
    rs = np.random.RandomState(seed)
    cats = list(range(1, 81))
    images = [(1 + i, 480, 640) for i in range(n_img)]
    A, Rs, aid = [], [], 0
    for img, H, W in images:
        present = rs.choice(cats, rs.randint(1, 7), replace=False)
        gts = []
        for b in _random_boxes(rs, rs.randint(1, 15), H, W, lo=6.0):
            aid += 1
            b = np.floor(b) if segm else b
            gts.append(_ann(aid, img, int(rs.choice(present)), b, crowd=rs.rand() < 0.03))
        A += gts
        res = []
        _detect(rs, gts * 4, img, cats, H, W, 100, res, quant=1000)
        Rs += [res[i] for i in sorted(rs.permutation(len(res))[:100])]
    if segm:
        def rect(b, H=480, W=640):
            x, y, w, h = (int(max(v, 0)) for v in b)
            x, y = min(x, W - 1), min(y, H - 1)
            w, h = max(1, min(w, W - x)), max(1, min(h, H - y))
            runs = []
            pos = 0
            for c in range(x, x + w):
                runs += [c * H + y - pos, h]
                pos = c * H + y + h
            runs.append(H * W - pos)
            return {"size": [H, W], "counts": unmold_ref.rle_string(np.array(runs, np.uint32))}
        for a in A:
            a["segmentation"] = rect(a["bbox"])
        Rs = [_res(r["image_id"], r["category_id"], None, r["score"], rect(r["bbox"]), False) for r in Rs]
    return {"name": "synthetic%d%s" % (n_img, "_segm" if segm else ""), "images": images, "categories": cats,
            "annotations": A, "results": Rs}


class Timed:
    """Wraps the C entry points of the loaded library with HIP events."""

    def __init__(self, L):
        self.L, self.events = L, []
        for name in cocoeval.SIGNATURES:
            if name.endswith("_bytes"):
                continue
            setattr(self, name, self._wrap(name, getattr(L, name)))

    def __getattr__(self, name):
        return getattr(self.L, name)

    def _wrap(self, name, fn):
        def call(*a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*a)
            e1.record()
            self.events.append((name, e0, e1))
            return rc
        return call


def run(case, iou_type, out, ref=True, reps=5):
    ids = [i for i, _, _ in case["images"]]

    def once():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gt = cocoeval.pack_ground_truth(case["annotations"], ids, case["categories"])
        dt = cocoeval.pack_results(case["results"])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ev = cocoeval.evaluate(gt, dt, iou_type)
        torch.cuda.synchronize()
        return t1 - t0, time.perf_counter() - t1, ev

    once()                                                      # warm-up: code objects, allocator, sort plans
    timed = Timed(cocoeval.load())
    cocoeval._coco = timed
    runs = [once() for _ in range(reps)]
    cocoeval._coco = timed.L
    per = {}
    for name, e0, e1 in timed.events:
        per.setdefault(name, []).append(e0.elapsed_time(e1))
    ev = runs[-1][2]
    out.append("%s / %s: %d gts, %d results, %d (image, category) pairs, mAP %.6f" % (
        case["name"], iou_type, len(case["annotations"]), len(case["results"]), len(ev.pairs), ev.stats[0]))
    out.append("  pack (dicts -> device arrays, host Python)   median %8.1f ms" % (1e3 * np.median([r[0] for r in runs])))
    out.append("  evaluate (upload, sorts, kernels, reads)     median %8.1f ms  min %.1f  max %.1f" % (
        1e3 * np.median([r[1] for r in runs]), 1e3 * min(r[1] for r in runs), 1e3 * max(r[1] for r in runs)))
    for name, v in per.items():
        out.append("    %-22s %d launch(es) per evaluation, median %8.3f ms (HIP events around the launch)" % (
            name, len(v) // reps, float(np.median(v))))
    out.append("  kernel launches of this library per pack + evaluate: %d (independent of the number of images)"
               % (len(timed.events) // reps))
    if ref:
        t0 = time.perf_counter()
        exp = R.evaluate_case(dict(case, images=case["images"]), iou_type)
        t = time.perf_counter() - t0
        same = all(np.array_equal(getattr(ev, k).view(np.uint64), exp[k].view(np.uint64))
                   for k in ("precision", "recall", "scores"))
        out.append("  tests/cocoeval_ref.py on this host            %8.1f s   (tables bit-equal: %s)" % (t, same))
    print(out[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cocoeval_probe.txt"))
    ap.add_argument("--no-ref-val", action="store_true", help="skip the host restatement at val2017 size")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    out = ["COCO evaluation probe on %s (torch %s)" % (torch.cuda.get_device_name(0), torch.__version__), ""]
    g = np.load(os.path.join(ROOT, "tests", "golden", "cocoeval.npz"))
    large = [c for c in cocoeval_cases() if c["name"] == LARGE][0]
    run(large, "bbox", out)
    out.append("  the reference's COCOeval evaluate() + accumulate() on the build machine's CPU (golden): %.1f s"
               % float(g["large/bbox/reference_seconds"]))
    out.append("")
    run(synthetic(500, segm=True), "segm", out)
    out.append("")
    run(synthetic(5000), "bbox", out, ref=not args.no_ref_val, reps=3)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
