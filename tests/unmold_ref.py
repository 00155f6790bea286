"""NumPy restatement of the reference's inference unmolding (lib/workflow.py:523-600 `_unmold_detections`,
tools/image_utils.py:172-189 `unmold_mask`, datasets/eval/common/maskApi.c `rleEncode` / `rleToString`).

`scipy.misc.imresize` (removed in SciPy 1.3) is restated from SciPy 1.0 (`toimage` -> `bytescale`) and Pillow's 8-bit
BILINEAR resample (`precompute_coeffs`, `normalize_coeffs_8bpc`, 22-bit fixed point, horizontal pass first).  Pure
NumPy: no Pillow, no GPU.  tests/test_unmold_golden.py pins it to the golden made from the reference's own code."""
import numpy as np

PRECISION_BITS = 22


def bytescale(m):
    """SciPy 1.0 bytescale of a float32 array: fp32 arithmetic, each operation rounded."""
    m = np.asarray(m, np.float32)
    cmin, cmax = m.min(), m.max()
    cscale = np.float32(cmax - cmin)
    if cscale == 0:
        cscale = np.float32(1)
    scale = np.float32(255.0 / float(cscale))        # one rounding of the fp64 quotient == the fp32 division
    v = (m - cmin) * scale
    return (np.clip(v, np.float32(0), np.float32(255)) + np.float32(0.5)).astype(np.uint8)


def coeffs(in_size, out_size):
    """Pillow precompute_coeffs + normalize_coeffs_8bpc for the bilinear filter: [(xmin, [int weights])]."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = fs
    ss = 1.0 / fs
    res = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(in_size, int(center + support + 0.5))
        ws = []
        for x in range(xmax - xmin):
            t = abs((x + xmin - center + 0.5) * ss)
            ws.append(1.0 - t if t < 1.0 else 0.0)
        ww = 0.0
        for w in ws:
            ww += w
        if ww != 0.0:
            ws = [w / ww for w in ws]
        res.append((xmin, [int(0.5 + w * (1 << PRECISION_BITS)) for w in ws]))
    return res


def _pass(img, size, axis):
    img = np.moveaxis(img, axis, 0)
    out = np.empty((size,) + img.shape[1:], np.int64)
    for o, (lo, ks) in enumerate(coeffs(img.shape[0], size)):
        acc = np.full(img.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for k, w in enumerate(ks):
            acc += img[lo + k].astype(np.int64) * w
        out[o] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_bilinear(img, h, w):
    """Pillow Image.resize((w, h), BILINEAR) of an 'L' image (uint8 [rows, cols])."""
    cur = np.asarray(img, np.uint8)
    if w != cur.shape[1]:
        cur = _pass(cur, w, 1)
    if h != cur.shape[0]:
        cur = _pass(cur, h, 0)
    return cur.astype(np.uint8)


def unmold_mask(mask, box, hw):
    """tools/image_utils.py:172-189; the paste is clipped to the image."""
    y1, x1, y2, x2 = (int(v) for v in box)
    H, W = hw
    m = resize_bilinear(bytescale(mask), y2 - y1, x2 - x1) >= 128
    full = np.zeros((H, W), np.uint8)
    cy1, cy2, cx1, cx2 = max(y1, 0), min(y2, H), max(x1, 0), min(x2, W)
    if cy1 < cy2 and cx1 < cx2:
        full[cy1:cy2, cx1:cx2] = m[cy1 - y1:cy2 - y1, cx1 - x1:cx2 - x1]
    return full


def image_boxes(det_boxes, hw, window):
    """lib/workflow.py:562-570 in float64, truncated to int32 (out of range or NaN -> INT32_MIN, as on x86-64)."""
    window = np.asarray(window, np.float64)
    scale = min(hw[0] / (window[2] - window[0]), hw[1] / (window[3] - window[1]))
    shift = np.array([window[0], window[1], window[0], window[1]])
    v = (np.asarray(det_boxes, np.float32).astype(np.float64) - shift) * scale
    ok = (v >= -2.0 ** 31) & (v < 2.0 ** 31)
    return np.where(ok, v, -2.0 ** 31).astype(np.int64).astype(np.int32)


def unmold_detections(det, masks, hw, window):
    """One image: det [D, 6] fp32, masks [D, K, mh, mw] fp32 -> boxes int32 [n, 4], class_ids int32 [n],
    scores fp32 [n], full masks uint8 [n, H, W] and the source rows [n]."""
    det = np.asarray(det, np.float32)
    zero = np.where(det[:, 4] == 0)[0]
    N = int(zero[0]) if zero.size else det.shape[0]
    boxes = image_boxes(det[:N, :4], hw, window)
    class_ids = det[:N, 4].astype(np.int32)
    scores = det[:N, 5].copy()
    h = boxes[:, 2].astype(np.int64) - boxes[:, 0]
    w = boxes[:, 3].astype(np.int64) - boxes[:, 1]
    # (y2-y1)*(x2-x1) > 0; boxes flipped on both axes and extents >= 2^31 are dropped too
    keep = np.where((h > 0) & (w > 0) & (h < 2 ** 31) & (w < 2 ** 31))[0]
    H, W = int(hw[0]), int(hw[1])
    full = np.zeros((keep.size, H, W), np.uint8)
    for j, i in enumerate(keep):
        full[j] = unmold_mask(masks[i, class_ids[i]], boxes[i], (H, W))
    return boxes[keep], class_ids[keep], scores[keep], full, keep.astype(np.int32)


def rle_counts(full):
    """maskApi.c rleEncode of one [H, W] 0/1 mask in column-major order."""
    flat = np.asarray(full, np.uint8).T.reshape(-1)
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    if flat.size and flat[0] != 0:
        change = np.concatenate([[0], change])
    edges = np.concatenate([[0], change, [flat.size]])
    return np.diff(edges).astype(np.uint32)


def rle_string(cnts):
    """maskApi.c rleToString: 6-bit characters, counts i > 2 as cnts[i] - cnts[i-2]."""
    out = bytearray()
    c64 = np.asarray(cnts, np.int64)
    for i in range(c64.size):
        x = int(c64[i]) - (int(c64[i - 2]) if i > 2 else 0)
        more = True
        while more:
            c = x & 0x1F
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(c + 48)
    return bytes(out)


def rle_decode(cnts, hw):
    H, W = hw
    flat = np.zeros(H * W, np.uint8)
    pos, v = 0, 0
    for c in cnts:
        flat[pos:pos + int(c)] = v
        pos += int(c)
        v ^= 1
    return flat.reshape(W, H).T


def coco_results(image_id, boxes, class_ids, scores, rles, category_map):
    """lib/workflow.py:400-413 (inference): one result dict per detection."""
    res = []
    for j in range(len(class_ids)):
        y1, x1, y2, x2 = (int(v) for v in boxes[j])
        cid = int(class_ids[j])
        res.append({"image_id": image_id,
                    "category_id": category_map(cid) if callable(category_map) else category_map[cid],
                    "bbox": [x1, y1, x2 - x1, y2 - y1],
                    "score": np.float32(scores[j]),
                    "segmentation": rles[j]})
    return res
