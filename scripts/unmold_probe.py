"""Times postprocess.unmold_detections at 8 images x 100 detections, COCO-sized originals (640 x 480 through a
1024 window) and realistic box sizes, against the NumPy restatement (tests/unmold_ref.py) on the host.

    python scripts/unmold_probe.py [--iters 50] [--out profiles/unmold_probe.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from feature_intertwiner_amd.postprocess import unmold_detections  # noqa: E402
import unmold_ref as R  # noqa: E402


def inputs(bs=8, D=100, K=81, H=480, W=640, seed=0):
    rs = np.random.RandomState(seed)
    win = np.array([128, 0, 896, 1024], np.float32)                     # 640 x 480 at scale 1.6, padded top/bottom
    det = np.zeros((bs, D, 6), np.float32)
    for b in range(bs):
        n = D - 5 * b                                                   # 100 .. 65 detections
        hgt = np.exp(rs.uniform(np.log(16), np.log(480), n))            # 10 .. 300 px in the original
        wid = hgt * np.exp(rs.uniform(-0.7, 0.7, n))
        y1 = rs.uniform(win[0], win[2] - 8, n)
        x1 = rs.uniform(win[1], win[3] - 8, n)
        det[b, :n, 0], det[b, :n, 1] = y1, x1
        det[b, :n, 2] = np.minimum(win[2], y1 + hgt)
        det[b, :n, 3] = np.minimum(win[3], x1 + wid)
        det[b, :n, 4] = rs.randint(1, K, n)
        det[b, :n, 5] = np.sort(rs.uniform(0.05, 1, n))[::-1]
    masks = (1 / (1 + np.exp(-4 * rs.standard_normal((bs, D, K, 28, 28))))).astype(np.float32)
    return det, masks, np.tile([[H, W]], (bs, 1)).astype(np.int32), np.tile(win, (bs, 1))


def gpu_ms(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-images", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    det, masks, hw, win = inputs()
    d, m, w = (torch.from_numpy(x).cuda() for x in (det, masks, win))
    lines = ["unmold probe: 8 images x 100 detection rows, 640x480 originals, 81 classes, 28x28 masks"]
    out = unmold_detections(d, m, hw, w)
    n = [int(o["boxes"].shape[0]) for o in out]
    boxes = np.concatenate([o["boxes"].cpu().numpy() for o in out])
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    counts = sum(len(c) for o in out for c in o["rle_counts"])
    chars = sum(len(r["counts"]) for o in out for r in o["rle"])
    lines.append("detections kept %s (total %d); box area px: median %d, max %d; RLE counts %d, string bytes %d" %
                 (n, sum(n), int(np.median(area)), int(area.max()), counts, chars))
    for label, kw in (("rle", dict(rle=True)), ("rle+dense", dict(rle=True, dense=True)),
                      ("dense only", dict(rle=False, dense=True)), ("boxes only", dict(rle=False))):
        ms = gpu_ms(lambda: unmold_detections(d, m, hw, w, **kw), a.iters)
        extra = ""
        if kw.get("dense"):
            mb = sum(n) * 480 * 640 / 1e6
            extra = "  (dense writes %.1f MB)" % mb
        lines.append("GPU %-11s %8.3f ms per batch, wall clock incl. host sync and D2H%s" % (label, ms, extra))
    t0 = time.perf_counter()
    for b in range(a.host_images):
        _, _, _, full, _ = R.unmold_detections(det[b], masks[b], (480, 640), win[b])
        for j in range(full.shape[0]):
            R.rle_string(R.rle_counts(full[j]))
    host_ms = (time.perf_counter() - t0) * 1e3 / a.host_images * 8
    lines.append("host NumPy restatement %.1f ms per batch (extrapolated from %d images)" % (host_ms, a.host_images))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
