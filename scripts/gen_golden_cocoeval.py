"""Golden vectors for the COCO evaluation (feature_intertwiner_amd/cocoeval.py) from the REFERENCE'S OWN code.
TEST INFRASTRUCTURE; build machine only (reads the reference checkout, which does not exist on the GPU box).  No test
reads this script; tests read only its output, tests/golden/cocoeval.npz.

  1. Copies datasets/eval/PythonAPI/pycocotools/_mask.pyx and datasets/eval/common/maskApi.{c,h} into a temporary
     directory OUTSIDE the repository (in the reference's PythonAPI/ + common/ layout: the pyx names
     ../common/maskApi.c), compiles them there with the installed Cython and loads the module as
     datasets.eval.PythonAPI.pycocotools._mask.
  2. Imports the reference's COCO and COCOeval unmodified through oracle/_ref_import.install().  Two shims of old
     NumPy behaviour (third-party, not reference text): `np.float = float`, and an `np.linspace` that casts `num`
     to int (Params passes `np.round(...) + 1`).
  3. Runs COCO() / loadRes / COCOeval(...).evaluate() / accumulate() / summarize() on the in-memory datasets of
     tests/cocoeval_cases.py and writes the canonical flat form of tests/cocoeval_ref.py: every ious matrix, every
     evalImgs entry, precision / recall / scores / stats.  The large case keeps SHA-256 digests of the big arrays,
     `stats` and `recall`, and the reference's wall time for evaluate() + accumulate() (a stated baseline).

The "empty" case has an empty result list, where loadRes raises on anns[0].  Its golden is the reference's COCOeval
run on a detection COCO object with no annotations (the decision of DESIGN.md §2); it is marked `decided`.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_cocoeval.py   ->  tests/golden/cocoeval.npz
"""
import atexit
import contextlib
import copy
import hashlib
import importlib.util
import io
import os
import shutil
import subprocess
import sys
import sysconfig
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
from cocoeval_cases import LARGE, cocoeval_cases, inputs_sha256  # noqa: E402
from cocoeval_ref import BIG  # noqa: E402
from gen_golden_unmold import _pin_zip_times  # noqa: E402

REF = os.environ.get("FI_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "cocoeval.npz")
DECIDED = ("empty",)
MASK_NAME = "datasets.eval.PythonAPI.pycocotools._mask"


def build_mask_module():
    import Cython
    tmp = tempfile.mkdtemp(prefix="fi_ref_pycocotools_")
    assert not os.path.abspath(tmp).startswith(ROOT), tmp
    atexit.register(shutil.rmtree, tmp, True)
    api, common = os.path.join(tmp, "PythonAPI", "pycocotools"), os.path.join(tmp, "common")
    os.makedirs(api)
    os.makedirs(common)
    shutil.copy(os.path.join(REF, "datasets", "eval", "PythonAPI", "pycocotools", "_mask.pyx"), api)
    for f in ("maskApi.c", "maskApi.h"):
        shutil.copy(os.path.join(REF, "datasets", "eval", "common", f), common)
    subprocess.check_call([sys.executable, "-m", "cython", "-3", "_mask.pyx"], cwd=api)
    so = os.path.join(api, "_mask" + sysconfig.get_config_var("EXT_SUFFIX"))
    subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-fPIC", "-shared", "-w", "-o", so, os.path.join(api, "_mask.c"),
                           os.path.join(common, "maskApi.c"), "-I" + common, "-I" + sysconfig.get_paths()["include"],
                           "-I" + np.get_include(), "-lm"])
    spec = importlib.util.spec_from_file_location(MASK_NAME, so)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, Cython.__version__


def import_reference():
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from _ref_import import install
    install()
    np.float = float
    linspace = np.linspace
    np.linspace = lambda start, stop, num=50, **kw: linspace(start, stop, int(num), **kw)
    import matplotlib
    matplotlib.use("Agg")
    mod, cython_version = build_mask_module()
    sys.modules[MASK_NAME] = mod
    from datasets.eval.PythonAPI.pycocotools.coco import COCO
    from datasets.eval.PythonAPI.pycocotools.cocoeval import COCOeval
    return COCO, COCOeval, cython_version


def canonical(ev):
    """The flat form of tests/cocoeval_ref.evaluate from a COCOeval object after accumulate() and summarize()."""
    p = ev.params
    out = {k: [] for k in BIG[:8]}
    iou_keys, ev_keys = [], []
    for img in p.imgIds:
        for cat in p.catIds:
            m = ev.ious[img, cat]
            if len(m):
                iou_keys.append((img, cat) + m.shape)
                out["ious"].append(np.ascontiguousarray(m).ravel())
    I, A = len(p.imgIds), len(p.areaRng)
    for k in range(len(p.catIds)):
        for a in range(A):
            for i in range(I):
                e = ev.evalImgs[(k * A + a) * I + i]
                if e is None:
                    continue
                ev_keys.append((k, a, i, len(e["dtIds"]), len(e["gtIds"])))
                out["dt_ids"].append(np.array(e["dtIds"], np.float64))
                out["gt_ids"].append(np.array(e["gtIds"], np.float64))
                out["dt_matches"].append(np.asarray(e["dtMatches"], np.float64).ravel())
                out["gt_matches"].append(np.asarray(e["gtMatches"], np.float64).ravel())
                out["dt_scores"].append(np.array(e["dtScores"], np.float64))
                out["gt_ignore"].append(np.asarray(e["gtIgnore"], np.float64))
                out["dt_ignore"].append(np.asarray(e["dtIgnore"], np.float64).ravel())
    res = {k: (np.concatenate(v) if v else np.zeros(0)) for k, v in out.items()}
    res["iou_keys"] = np.array(iou_keys, np.int64).reshape(-1, 4)
    res["ev_keys"] = np.array(ev_keys, np.int64).reshape(-1, 5)
    for k in ("precision", "recall", "scores"):
        res[k] = np.asarray(ev.eval[k], np.float64)
    res["stats"] = np.asarray(ev.stats, np.float64)
    return res


def run_case(COCO, COCOeval, case, iou_type):
    with contextlib.redirect_stdout(io.StringIO()):
        gt = COCO()
        gt.dataset = {"images": [{"id": i, "height": h, "width": w} for i, h, w in case["images"]],
                      "categories": [{"id": c, "name": str(c), "supercategory": "x"} for c in case["categories"]],
                      "annotations": copy.deepcopy(case["annotations"])}
        gt.createIndex()
        results = copy.deepcopy(case["results"])
        if results:
            dt = gt.loadRes(results)
        else:                                            # decided: an empty result list is "no detections"
            dt = COCO()
            dt.dataset = {"images": list(gt.dataset["images"]), "categories": list(gt.dataset["categories"]),
                          "annotations": []}
            dt.createIndex()
        ev = COCOeval(gt, dt, iou_type)
        t0 = time.time()
        ev.evaluate()
        ev.accumulate()
        seconds = time.time() - t0
        ev.summarize()
    return canonical(ev), seconds


def main():
    COCO, COCOeval, cython_version = import_reference()
    cases = cocoeval_cases()
    out = {"inputs_sha256": np.array(inputs_sha256(cases)), "numpy_version": np.array(np.__version__),
           "cython_version": np.array(cython_version), "cases": np.array([c["name"] for c in cases]),
           "decided": np.array(DECIDED)}
    for case in cases:
        for iou_type in case["types"]:
            res, seconds = run_case(COCO, COCOeval, case, iou_type)
            key = "%s/%s/" % (case["name"], iou_type)
            print(key, "stats[0] = %.6f" % res["stats"][0], "%.1f s" % seconds)
            for k, v in res.items():
                if case["name"] == LARGE and k in BIG + ("iou_keys", "ev_keys"):
                    out[key + k + "_sha256"] = np.array(hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest())
                else:
                    out[key + k] = v
            if case["name"] == LARGE:
                # a stated baseline (this build machine's CPU).  A rerun keeps the recorded value while the new
                # measurement is within a factor of two of it, so that the file regenerates byte for byte.
                name = key + "reference_seconds"
                sec = float(round(seconds, 1))
                if os.path.exists(OUT) and name in np.load(OUT):
                    old = float(np.load(OUT)[name])
                    sec = old if 0.5 * old <= sec <= 2.0 * old else sec
                out[name] = np.array(sec)
    buf = io.BytesIO()
    np.savez_compressed(buf, **out)
    data = _pin_zip_times(buf.getvalue())
    with open(OUT, "wb") as f:
        f.write(data)
    print("wrote", OUT, len(data), "bytes")


if __name__ == "__main__":
    main()
