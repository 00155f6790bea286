"""Golden vectors for the inference unmolding (feature_intertwiner_amd/postprocess.py) from the REFERENCE'S OWN code.
TEST INFRASTRUCTURE; build machine only (reads the reference checkout, which does not exist on the GPU box).  No test
reads this script; tests read only its output, tests/golden/unmold.npz.

  1. Imports the reference's lib/workflow.py through oracle/_ref_import.install().  Modules it cannot load are stubbed
     with empty placeholders: the vendored pycocotools (its Cython part is not built) and tools.visualize.
  2. Runs its `_unmold_detections` unmodified on the seeded cases of tests/unmold_cases.py.  `scipy.misc.imresize`
     (removed in SciPy 1.3) is supplied by a restatement of SciPy 1.0's imresize / toimage / bytescale on top of the
     installed Pillow: that shim restates a third-party library, not the reference.
  3. Copies datasets/eval/common/maskApi.{c,h} into a temporary directory OUTSIDE the repository, compiles them there
     and calls `rleEncode` and `rleToString` through ctypes on the reference's full masks.
  4. Writes tests/golden/unmold.npz: per case the boxes, class ids, scores, every RLE count and string, the full dense
     masks when they are small and their SHA-256 otherwise; the SHA-256 of the regenerated inputs; the Pillow and NumPy
     versions.

The "outside" case has boxes that leave the image, where the reference raises inside NumPy.  Its golden is the
restatement of tests/unmold_ref.py with the paste clipped to the image (the decision of DESIGN.md §2); it is marked
`decided` in the file.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_unmold.py   ->  tests/golden/unmold.npz
"""
import atexit
import ctypes
import hashlib
import io
import os
import shutil
import subprocess
import sys
import tempfile
import types

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from unmold_cases import DENSE_LIMIT, inputs_sha256, unmold_cases  # noqa: E402
import unmold_ref  # noqa: E402

REF = os.environ.get("FI_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "unmold.npz")
DECIDED = ("outside",)


# ---------------------------------------------------------------- SciPy 1.0 imresize, restated on the installed Pillow
def _bytescale(data, cmin=None, cmax=None, high=255, low=0):
    if data.dtype == np.uint8:
        return data
    if cmin is None:
        cmin = data.min()
    if cmax is None:
        cmax = data.max()
    cscale = cmax - cmin
    if cscale < 0:
        raise ValueError("`cmax` should be larger than `cmin`.")
    elif cscale == 0:
        cscale = 1
    scale = float(high - low) / cscale
    bytedata = (data - cmin) * scale + low
    return (bytedata.clip(low, high) + 0.5).astype(np.uint8)


def _toimage(arr):
    data = np.asarray(arr)
    assert data.ndim == 2
    shape = (data.shape[1], data.shape[0])
    return Image.frombytes('L', shape, _bytescale(data).tobytes())


def _imresize(arr, size, interp='bilinear', mode=None):
    assert interp == 'bilinear' and mode is None and isinstance(size, tuple)
    im = _toimage(arr)
    size = (size[1], size[0])
    return np.array(im.resize(size, resample=Image.BILINEAR))


def import_reference():
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from _ref_import import install
    install()
    import scipy.misc
    scipy.misc.imresize = _imresize
    for name in ("datasets.eval.PythonAPI.pycocotools", "datasets.eval.PythonAPI.pycocotools.mask",
                 "datasets.eval.PythonAPI.pycocotools.cocoeval", "tools.visualize"):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    sys.modules["datasets.eval.PythonAPI.pycocotools.cocoeval"].COCOeval = None
    sys.modules["datasets.eval.PythonAPI.pycocotools"].mask = sys.modules["datasets.eval.PythonAPI.pycocotools.mask"]
    sys.modules["tools.visualize"].display_instances = None
    import matplotlib
    matplotlib.use("Agg")
    from lib import workflow
    return workflow


# ---------------------------------------------------------------- maskApi.c, compiled outside the repository
class _RLE(ctypes.Structure):
    _fields_ = [("h", ctypes.c_size_t), ("w", ctypes.c_size_t), ("m", ctypes.c_size_t),
                ("cnts", ctypes.POINTER(ctypes.c_uint32))]


def build_mask_api():
    tmp = tempfile.mkdtemp(prefix="fi_ref_maskapi_")
    assert not os.path.abspath(tmp).startswith(ROOT), tmp
    atexit.register(shutil.rmtree, tmp, True)
    src = os.path.join(REF, "datasets", "eval", "common")
    for f in ("maskApi.c", "maskApi.h"):
        shutil.copy(os.path.join(src, f), tmp)
    so = os.path.join(tmp, "maskapi.so")
    subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-fPIC", "-shared", "-o", so,
                           os.path.join(tmp, "maskApi.c"), "-lm"])
    L = ctypes.CDLL(so)
    L.rleEncode.argtypes = [ctypes.POINTER(_RLE), ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t]
    L.rleToString.argtypes = [ctypes.POINTER(_RLE)]
    L.rleToString.restype = ctypes.c_void_p
    L.rleFree.argtypes = [ctypes.POINTER(_RLE)]
    libc = ctypes.CDLL(None)
    libc.free.argtypes = [ctypes.c_void_p]
    return L, libc


def encode(L, libc, full):
    """maskUtils.encode(np.asfortranarray(full)) for one [H, W] mask: (counts, string)."""
    H, W = full.shape
    fort = np.asfortranarray(full.astype(np.uint8))
    buf = np.ascontiguousarray(fort.T)                 # column-major bytes
    r = _RLE()
    L.rleEncode(ctypes.byref(r), buf.ctypes.data, H, W, 1)
    cnts = np.ctypeslib.as_array(r.cnts, (r.m,)).copy()
    p = L.rleToString(ctypes.byref(r))
    s = ctypes.string_at(p)
    libc.free(p)
    L.rleFree(ctypes.byref(r))
    return cnts.astype(np.uint32), s


def main():
    wf = import_reference()
    L, libc = build_mask_api()
    cases = unmold_cases()
    out = {"inputs_sha256": np.array(inputs_sha256(cases)), "pillow_version": np.array(PIL.__version__),
           "numpy_version": np.array(np.__version__), "cases": np.array([c[0] for c in cases]),
           "decided": np.array(DECIDED)}
    for name, det, masks, hw, win in cases:
        bs = det.shape[0]
        for b in range(bs):
            H, W = int(hw[b, 0]), int(hw[b, 1])
            if name in DECIDED:
                boxes, cls, scores, full, _ = unmold_ref.unmold_detections(det[b], masks[b], (H, W), win[b])
                full = full.transpose(1, 2, 0)
            else:
                mm = np.ascontiguousarray(masks[b].transpose(0, 2, 3, 1))        # workflow.py:389 permute
                boxes, cls, scores, full = wf._unmold_detections(det[b], mm, (H, W, 3), win[b].astype(np.int64), True)
            n = boxes.shape[0]
            full = np.asarray(full, np.uint8).reshape(H, W, n) if n else np.zeros((H, W, 0), np.uint8)
            cnts, strs = [], []
            for j in range(n):
                c, s = encode(L, libc, full[:, :, j])
                cnts.append(c)
                strs.append(s)
            k = "%s/%d/" % (name, b)
            out[k + "boxes"] = boxes.astype(np.int32).reshape(n, 4)
            out[k + "class_ids"] = cls.astype(np.int32)
            out[k + "scores"] = scores.astype(np.float32)
            out[k + "rle_len"] = np.array([len(c) for c in cnts], np.int64)
            out[k + "counts"] = np.concatenate(cnts).astype(np.uint32) if n else np.zeros(0, np.uint32)
            out[k + "str_len"] = np.array([len(s) for s in strs], np.int64)
            out[k + "strings"] = np.frombuffer(b"".join(strs), np.uint8)
            dense = np.ascontiguousarray(full.transpose(2, 0, 1))                 # [n, H, W]
            out[k + "dense_sha256"] = np.array(hashlib.sha256(dense.tobytes()).hexdigest())
            if dense.size <= DENSE_LIMIT:
                out[k + "dense"] = np.packbits(dense, axis=-1)
    buf = io.BytesIO()
    np.savez_compressed(buf, **out)
    # np.savez writes zip members with the current time: pin it so that a rerun is byte-identical
    data = _pin_zip_times(buf.getvalue())
    with open(OUT, "wb") as f:
        f.write(data)
    print("wrote", OUT, len(data), "bytes")


def _pin_zip_times(data):
    import zipfile
    src = zipfile.ZipFile(io.BytesIO(data))
    dst_buf = io.BytesIO()
    with zipfile.ZipFile(dst_buf, "w", zipfile.ZIP_DEFLATED) as dst:
        for info in src.infolist():
            zi = zipfile.ZipInfo(info.filename, date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o600 << 16
            dst.writestr(zi, src.read(info.filename))
    return dst_buf.getvalue()


if __name__ == "__main__":
    main()
