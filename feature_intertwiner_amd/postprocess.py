"""Inference unmolding on the GPU: the loop body of the reference's test_model (lib/workflow.py:366-432).

`unmold_detections` turns the inference outputs (detections [bs, D, 6] in molded pixels, mrcnn_mask
[bs, D, K, mh, mw] sigmoids) into what `_unmold_detections` (lib/workflow.py:523-600) and `maskUtils.encode` give,
bit for bit: int32 image-space boxes, class ids, scores, COCO RLE and, on request, the full-image uint8 masks.  The
kernels are in csrc/unmold.hip; this module only allocates, scans the per-detection sizes and splits the results.
One host synchronisation reads the sizes (the results go to the host anyway).  `coco_results` builds the
reference's result dicts (lib/workflow.py:405-413)."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import FiError, check, current_stream, ptr, require_cuda

LIB_PATH = _lib.sublibrary_path("eval")
_p, _i, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
# name -> (restype, argtypes); mirrors include/fi_eval.h one to one
SIGNATURES = {
    "fi_unmold_workspace_bytes": (ctypes.c_size_t, [_i] * 4),
    "fi_unmold_prepare": (_i, [_p] * 5 + [_i] * 5 + [_p] * 7 + [_p]),
    "fi_unmold_encode": (_i, [_p] * 4 + [_i] * 4 + [_p] * 4 + [_p]),
    "fi_unmold_paste": (_i, [_p] * 4 + [_i] * 4 + [_p, _ll, _p, _p]),
}


def load():
    """Load libfi_eval.so (after libfi_hip.so, which it links against) and attach the signatures."""
    return _lib.load_sublibrary("eval", SIGNATURES)


def _host_int32(x, cols):
    a = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(np.asarray(a)[:, :cols], dtype=np.int32)


def _to_device(a, dtype, device):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    return t.pin_memory().to(device, non_blocking=True)


def unmold_detections(detections, mrcnn_mask, image_shapes, windows, rle=True, dense=False):
    """detections [bs, D, 6] and mrcnn_mask [bs, D, K, mh, mw] (device, fp32), image_shapes [bs, >=2] original
    (H, W, ...) and windows [bs, 4] (y1, x1, y2, x2 in molded pixels), host or device.  Runs on the current stream.

    Returns one dict per image: 'boxes' int32 [n, 4] (y1, x1, y2, x2), 'class_ids' int32 [n], 'scores' fp32 [n]
    (device), 'image_shape' (H, W); with rle=True 'rle' (a list of {'size': [H, W], 'counts': bytes}) and
    'rle_counts' (a list of uint32 arrays); with dense=True 'masks' uint8 [H, W, n] (device, a permuted view of
    [n, H, W], the reference's layout)."""
    require_cuda(detections, mrcnn_mask)
    L = load()
    dev = detections.device
    if detections.dim() != 3 or detections.size(2) != 6:
        raise FiError("detections must be [bs, D, 6] (got %s)" % (tuple(detections.shape),))
    bs, D = detections.shape[:2]
    if mrcnn_mask.dim() != 5 or tuple(mrcnn_mask.shape[:2]) != (bs, D):
        raise FiError("mrcnn_mask must be [bs, D, K, mh, mw] (got %s)" % (tuple(mrcnn_mask.shape),))
    K, mh, mw = mrcnn_mask.shape[2:]
    det = detections.detach().float().contiguous()
    msk = mrcnn_mask.detach().float().contiguous()
    hw = _host_int32(image_shapes, 2)
    if hw.shape[0] != bs:
        raise FiError("image_shapes has %d rows for a batch of %d" % (hw.shape[0], bs))
    hw_dev = _to_device(hw, torch.int32, dev)
    if torch.is_tensor(windows):
        win = windows.detach().to(dev, torch.float32).contiguous()
    else:
        win = _to_device(np.asarray(windows, np.float32).reshape(bs, 4), torch.float32, dev)
    slots = bs * D
    boxes = torch.empty(slots, 4, dtype=torch.int32, device=dev)
    class_ids = torch.empty(slots, dtype=torch.int32, device=dev)
    scores = torch.empty(slots, dtype=torch.float32, device=dev)
    num_valid = torch.empty(bs, dtype=torch.int32, device=dev)
    sizes = torch.empty(slots, 2, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(max(1, L.fi_unmold_workspace_bytes(bs, D, mh, mw)), dtype=torch.uint8, device=dev)
    hw_ptr = hw.ctypes.data_as(ctypes.c_void_p)
    st = current_stream()
    check(L.fi_unmold_prepare(ptr(det), ptr(msk), ptr(hw_dev), hw_ptr, ptr(win), bs, D, K, mh, mw, ptr(boxes),
                              ptr(class_ids), ptr(scores), ptr(num_valid), ptr(sizes), ptr(status), ptr(ws), st),
          "fi_unmold_prepare")
    offsets = (sizes.cumsum(0) - sizes).contiguous()
    # the one host synchronisation: valid counts, per-slot sizes, status
    head = torch.cat([num_valid.long(), status.long(), sizes.view(-1)]).cpu().numpy()
    n = head[:bs].astype(np.int64)
    if head[bs]:
        raise FiError("unmold: %s" % "; ".join(m for bit, m in ((1, "a class id is outside [0, K)"),
                                                                (2, "a window has zero or negative extent"))
                                                if int(head[bs]) & bit))
    sz = head[bs + 1:].reshape(slots, 2)
    out = [{"boxes": boxes.view(bs, D, 4)[b, :n[b]], "class_ids": class_ids.view(bs, D)[b, :n[b]],
            "scores": scores.view(bs, D)[b, :n[b]], "image_shape": (int(hw[b, 0]), int(hw[b, 1]))}
           for b in range(bs)]
    if rle:
        tot_c, tot_s = int(sz[:, 0].sum()), int(sz[:, 1].sum())
        counts = torch.empty(max(1, tot_c), dtype=torch.int32, device=dev)
        strings = torch.empty(max(1, tot_s), dtype=torch.uint8, device=dev)
        check(L.fi_unmold_encode(ptr(hw_dev), hw_ptr, ptr(boxes), ptr(num_valid), bs, D, mh, mw, ptr(ws),
                                 ptr(offsets), ptr(counts), ptr(strings), st), "fi_unmold_encode")
        counts_h = counts.cpu().numpy().view(np.uint32)
        strings_h = strings.cpu().numpy().tobytes()
        co = np.concatenate([[0], np.cumsum(sz[:, 0])])
        so = np.concatenate([[0], np.cumsum(sz[:, 1])])
        for b in range(bs):
            H, W = out[b]["image_shape"]
            out[b]["rle"], out[b]["rle_counts"] = [], []
            for j in range(n[b]):
                s = b * D + j
                out[b]["rle_counts"].append(counts_h[co[s]:co[s + 1]])
                out[b]["rle"].append({"size": [H, W], "counts": strings_h[so[s]:so[s + 1]]})
    if dense:
        per = n * hw[:, 0].astype(np.int64) * hw[:, 1]
        total = int(per.sum())
        masks = torch.empty(max(16, total), dtype=torch.uint8, device=dev)
        check(L.fi_unmold_paste(ptr(hw_dev), hw_ptr, ptr(boxes), ptr(num_valid), bs, D, mh, mw, ptr(ws), total,
                                ptr(masks), st), "fi_unmold_paste")
        base = 0
        for b in range(bs):
            H, W = out[b]["image_shape"]
            out[b]["masks"] = masks[base:base + int(per[b])].view(int(n[b]), H, W).permute(1, 2, 0)
            base += int(per[b])
    return out


def coco_results(unmolded, coco_image_ids, category_map):
    """lib/workflow.py:400-413 (mode 'inference'): one dict per detection with 'image_id', 'category_id'
    (category_map[class_id], or category_map(class_id) for a callable, in place of dataset.get_source_class_id),
    'bbox' [x1, y1, w, h] of the int boxes, 'score' (np.float32) and 'segmentation' (the COCO RLE)."""
    results = []
    for img, image_id in zip(unmolded, coco_image_ids):
        if "rle" not in img:
            raise FiError("coco_results needs unmold_detections(..., rle=True)")
        boxes = img["boxes"].cpu().numpy()
        cls = img["class_ids"].cpu().numpy()
        scores = img["scores"].cpu().numpy()
        for j in range(cls.shape[0]):
            y1, x1, y2, x2 = (int(v) for v in boxes[j])
            c = int(cls[j])
            results.append({"image_id": image_id,
                            "category_id": category_map(c) if callable(category_map) else category_map[c],
                            "bbox": [x1, y1, x2 - x1, y2 - y1],
                            "score": scores[j],
                            "segmentation": img["rle"][j]})
    return results
