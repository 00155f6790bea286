"""Golden vectors for polygon ground truth -> RLE (feature_intertwiner_amd/cocomask.py) from the REFERENCE'S OWN code.
TEST INFRASTRUCTURE; build machine only (reads the reference checkout, which does not exist on the GPU box).  No test
reads this script; tests read only its output, tests/golden/cocopoly.npz.

The reference's _mask.pyx + maskApi.c are compiled in a temporary directory outside the repository and its COCO /
COCOeval imported unmodified, by `build_mask_module` / `import_reference` of scripts/gen_golden_cocoeval.py.  On the
inputs of tests/cocopoly_cases.py it runs

  maskUtils.frPyObjects (rleFrPoly)      every single polygon: RLE string, maskUtils.area, maskUtils.toBbox
  maskUtils.merge, intersect = 0 and 1   every multi-part case
  COCO.annToRLE                          every annotation of the two data sets
  COCOeval evaluate / accumulate / summarize, bbox and segm, on the two data sets with polygon ground truth, in the
                                         canonical flat form of tests/cocoeval_ref.py

The random batch and the polygon far above the LDS threshold keep SHA-256 digests of their counts only; the batch
also keeps the reference's wall time for the conversion (a stated baseline).

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_cocopoly.py   ->  tests/golden/cocopoly.npz
"""
import contextlib
import copy
import hashlib
import io
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import cocoeval_ref  # noqa: E402
import cocopoly_cases as C  # noqa: E402
from gen_golden_cocoeval import import_reference, run_case  # noqa: E402
from gen_golden_unmold import _pin_zip_times  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "cocopoly.npz")


def _bytes(s):
    return s.encode("ascii") if isinstance(s, str) else bytes(s)


def _pack_strings(out, key, rles):
    strs = [_bytes(r["counts"]) for r in rles]
    out[key + "strings"] = np.frombuffer(b"".join(strs), np.uint8).copy()
    out[key + "str_len"] = np.array([len(s) for s in strs], np.int64)
    out[key + "size"] = np.array([r["size"] for r in rles], np.int64).reshape(len(rles), 2)


def _chunked(fn, rles, step=200):
    """The reference's area / toBbox take at most 255 RLEs a call under the installed NumPy."""
    return np.concatenate([np.asarray(fn(rles[i:i + step])) for i in range(0, len(rles), step)])


def main():
    COCO, COCOeval, cython_version = import_reference()
    from datasets.eval.PythonAPI.pycocotools import mask as maskUtils
    out = {"inputs_sha256": np.array(C.inputs_sha256()), "numpy_version": np.array(np.__version__),
           "cython_version": np.array(cython_version)}
    # single polygons
    cases = C.poly_cases()
    small = [c for c in cases if c[0] != C.ZIGZAG]
    rles = [maskUtils.frPyObjects([list(p)], h, w)[0] for _, h, w, p in small]
    out["poly/names"] = np.array([c[0] for c in small])
    _pack_strings(out, "poly/", rles)
    out["poly/area"] = np.asarray(maskUtils.area(rles), np.uint32)
    out["poly/bbox"] = np.asarray(maskUtils.toBbox(rles), np.float64).reshape(len(rles), 4)
    _, h, w, p = [c for c in cases if c[0] == C.ZIGZAG][0]
    z = maskUtils.frPyObjects([list(p)], h, w)[0]
    zc = cocoeval_ref.rle_from_string(_bytes(z["counts"]))
    out["zigzag/sha256"] = np.array(C.digest([zc]))
    out["zigzag/num_counts"] = np.array(len(zc), np.int64)
    out["zigzag/area"] = np.asarray(maskUtils.area([z]), np.uint32)
    out["zigzag/bbox"] = np.asarray(maskUtils.toBbox([z]), np.float64).reshape(1, 4)
    # multi-part objects
    groups = C.merge_cases()
    out["merge/names"] = np.array([g[0] for g in groups])
    for intersect in (0, 1):
        merged = [maskUtils.merge(maskUtils.frPyObjects([list(p) for p in parts], h, w), intersect)
                  for _, h, w, parts in groups]
        key = "merge%d/" % intersect
        _pack_strings(out, key, merged)
        out[key + "area"] = np.asarray(maskUtils.area(merged), np.uint32)
        out[key + "bbox"] = np.asarray(maskUtils.toBbox(merged), np.float64).reshape(len(merged), 4)
    # the random batch: digests and the reference's time
    polys, sizes = C.random_batch()
    t0 = time.time()
    batch = [maskUtils.frPyObjects([p], h, w)[0] for p, (h, w) in zip(polys, sizes)]
    seconds = time.time() - t0
    counts = [cocoeval_ref.rle_from_string(_bytes(r["counts"])) for r in batch]
    out["batch/sha256"] = np.array(C.digest(counts))
    out["batch/total_counts"] = np.array(sum(len(c) for c in counts), np.int64)
    out["batch/area_sha256"] = np.array(hashlib.sha256(np.asarray(_chunked(maskUtils.area, batch), np.uint32).tobytes())
                                        .hexdigest())
    out["batch/bbox_sha256"] = np.array(hashlib.sha256(np.ascontiguousarray(_chunked(maskUtils.toBbox, batch), np.float64)
                                                       .tobytes()).hexdigest())
    # a stated baseline (this build machine's CPU).  A rerun keeps the recorded value while the new measurement is
    # within a factor of four of it, so that the file regenerates byte for byte.
    sec = float(round(seconds, 3))
    if os.path.exists(OUT) and "batch/reference_seconds" in np.load(OUT):
        old = float(np.load(OUT)["batch/reference_seconds"])
        sec = old if 0.25 * old <= sec <= 4.0 * old else sec
    out["batch/reference_seconds"] = np.array(sec)
    print("batch: %d polygons, %.3f s" % (len(polys), seconds))
    # the data sets: annToRLE of every annotation, then the evaluation
    out["datasets"] = np.array([d["name"] for d in C.datasets()])
    for case in C.datasets():
        with contextlib.redirect_stdout(io.StringIO()):
            gt = COCO()
            gt.dataset = copy.deepcopy(C.dataset_dict(case))
            gt.createIndex()
        anns = [gt.annToRLE(a) for a in gt.dataset["annotations"]]
        _pack_strings(out, case["name"] + "/ann_", anns)
        for iou_type in case["types"]:
            res, _ = run_case(COCO, COCOeval, case, iou_type)
            print(case["name"], iou_type, "stats[0] = %.6f" % res["stats"][0])
            for k, v in res.items():
                out["%s/%s/%s" % (case["name"], iou_type, k)] = v
    buf = io.BytesIO()
    np.savez_compressed(buf, **out)
    data = _pin_zip_times(buf.getvalue())
    with open(OUT, "wb") as f:
        f.write(data)
    print("wrote", OUT, len(data), "bytes")


if __name__ == "__main__":
    main()
