"""A plain NumPy restatement of the target kernels (csrc/targets.hip: fi_rpn_targets, fi_detection_targets) with every
rule stated, ties included.  A specification for the tests, not a fast path.

Decisions (IoU, thresholds, the crowd test, claims, counts, ranking) are taken in np.float32, one operation at a time, in
the order of iou_of in targets.hip (= layers.bbox_overlaps, "+ 10e-20" included); the kernel file is built with
-ffp-contract=off, so they are the kernels' bit for bit.  Ties:
  * the best GT of a box          np.argmax over the GTs      -> the first (lowest-index) maximum
  * the best anchor of a GT       np.argmax over the anchors  -> the lowest anchor index
  * "the k largest keys"          np.argsort(-key, kind="stable") -> largest key first, lower index first
RPN keys enter through the clamp of key_of (float bits - 0x3F800000, clamped to [0, 0x800000]); the detection kernel
ranks raw float bits.  Real-valued outputs (refinements, mini-mask boxes) are float64 from the same selected pairs.

GT rows: class id > 0 valid, < 0 crowd, 0 padding.  Boxes are (y1, x1, y2, x2)."""
from collections import namedtuple

import numpy as np

EPS_IOU = np.float32(10e-20)

RpnTargets = namedtuple("RpnTargets", "match deltas row_image row_anchor")
DetTargets = namedtuple("DetTargets", "rois class_ids deltas mask_boxes mask_box_ids is_positive sel")


def iou_f32(a, b):
    """IoU [N, M] of boxes a [N, 4] against b [M, 4] in fp32, in the operation order of iou_of."""
    a, b = np.asarray(a, np.float32)[:, None, :], np.asarray(b, np.float32)[None, :, :]
    zero = np.float32(0)
    y1, x1 = np.maximum(a[..., 0], b[..., 0]), np.maximum(a[..., 1], b[..., 1])
    y2, x2 = np.minimum(a[..., 2], b[..., 2]), np.minimum(a[..., 3], b[..., 3])
    inter = np.maximum(x2 - x1, zero) * np.maximum(y2 - y1, zero)
    a1 = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    a2 = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    out = inter / (a1 + a2 - inter + EPS_IOU)
    assert out.dtype == np.float32
    return out


def iou_f64(a, b):
    """The same IoU in float64 (the tests' margin check: how far a pair lies from a threshold)."""
    a, b = np.asarray(a, np.float64)[:, None, :], np.asarray(b, np.float64)[None, :, :]
    y1, x1 = np.maximum(a[..., 0], b[..., 0]), np.maximum(a[..., 1], b[..., 1])
    y2, x2 = np.minimum(a[..., 2], b[..., 2]), np.minimum(a[..., 3], b[..., 3])
    inter = np.maximum(x2 - x1, 0) * np.maximum(y2 - y1, 0)
    a1 = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    a2 = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    return inter / (a1 + a2 - inter + 1e-19)


def refine_f64(box, gt, std):
    """layers.box_refinement(box, gt) / std in float64; box, gt [N, 4]."""
    box, gt, std = np.asarray(box, np.float64), np.asarray(gt, np.float64), np.asarray(std, np.float32).astype(np.float64)
    h, w = box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]
    cy, cx = box[:, 0] + 0.5 * h, box[:, 1] + 0.5 * w
    gh, gw = gt[:, 2] - gt[:, 0], gt[:, 3] - gt[:, 1]
    gcy, gcx = gt[:, 0] + 0.5 * gh, gt[:, 1] + 0.5 * gw
    return np.stack([(gcy - cy) / h, (gcx - cx) / w, np.log(gh / h), np.log(gw / w)], 1) / std


def rpn_key(x):
    """key_of: the order-preserving integer image of a sampling key in [1, 2]."""
    bits = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.int64)
    return np.clip(bits - 0x3F800000, 0, 0x800000)


def largest_first(key, idx, k):
    """The k entries of idx with the largest key[idx]; equal keys: the lower index first (idx is ascending)."""
    return idx[np.argsort(-key[idx], kind="stable")][:k]


def _best_gt(iou, ids):
    """iou [N, G] fp32 -> (best IoU over the valid GTs, its first index, highest IoU over the crowd boxes)."""
    vv = np.where((ids > 0)[None, :], iou, np.float32(0))
    crowd = np.where((ids < 0)[None, :], iou, np.float32(0)).max(1)
    return vv, vv.max(1), np.argmax(vv, 1), crowd


def rpn_candidates(anchors, ids, gts, neg_thres, pos_thres):
    """One image, before the balancing: (candidate class [A] in {1, -1, 0}, best GT [A], IoU over valid GTs [A, G])."""
    vv, best, arg, crowd = _best_gt(iou_f32(anchors, gts), ids)
    m = np.zeros(len(anchors), np.float32)
    m[(best < np.float32(neg_thres)) & (crowd < np.float32(0.001))] = -1
    m[np.argmax(vv, 0)[ids > 0]] = 1                   # every valid GT claims its best anchor: the lowest index of the maximum
    m[best >= np.float32(pos_thres)] = 1
    return m, arg, vv


def rpn_targets_ref(anchors, gt_class_ids, gt_boxes, key_pos, key_neg, neg_thres, pos_thres, n_total, bbox_std_dev,
                    candidates=None):
    """fi_rpn_targets.  Returns match [b, A] fp32, deltas [b, A, 4] float64 (zero where match != 1), row_image and
    row_anchor [b * n_total] int64 (the non-zero anchors of every image in anchor order, -1 padded).
    candidates: per image, what rpn_candidates returned for it (the keys do not enter it), to save computing it again."""
    anchors = np.asarray(anchors, np.float32)
    ids, gts = np.asarray(gt_class_ids, np.int64), np.asarray(gt_boxes, np.float32)
    b, A = ids.shape[0], anchors.shape[0]
    match = np.zeros((b, A), np.float32)
    deltas = np.zeros((b, A, 4), np.float64)
    row_image = np.full((b, n_total), -1, np.int64)
    row_anchor = np.full((b, n_total), -1, np.int64)
    for i in range(b):
        cand, arg = (candidates[i] if candidates else rpn_candidates(anchors, ids[i], gts[i], neg_thres, pos_thres))[:2]
        pos_c, neg_c = np.nonzero(cand == 1)[0], np.nonzero(cand == -1)[0]
        keep_pos = min(len(pos_c), n_total // 2)
        keep_neg = min(len(neg_c), max(n_total - keep_pos, 0))
        pos = largest_first(rpn_key(key_pos[i]), pos_c, keep_pos)
        neg = largest_first(rpn_key(key_neg[i]), neg_c, keep_neg)
        match[i, pos], match[i, neg] = 1, -1
        deltas[i, pos] = refine_f64(anchors[pos], gts[i][arg[pos]], bbox_std_dev)
        nz = np.nonzero(match[i])[0]
        row_image[i, :len(nz)], row_anchor[i, :len(nz)] = i, nz
    return RpnTargets(match, deltas, row_image.reshape(-1), row_anchor.reshape(-1))


def det_candidates(proposals, num, ids, gts):
    """One image: (positive candidates, negative candidates, best GT [P]) of the first `num` proposals."""
    _, best, arg, crowd = _best_gt(iou_f32(proposals, gts), ids)
    valid = np.arange(len(proposals)) < num
    pos_c = np.nonzero((best >= np.float32(0.5)) & valid)[0]
    neg_c = np.nonzero((best < np.float32(0.5)) & (crowd < np.float32(0.001)) & valid)[0]
    return pos_c, neg_c, arg


def det_targets_ref(proposals, num_proposals, gt_class_ids, gt_boxes, key_pos, key_neg, rois_per_image, positive_cap,
                    negatives_per_positive, use_mini_mask, bbox_std_dev):
    """fi_detection_targets.  Slots: the positives by descending key_pos, then the negatives by descending key_neg, then
    unused (all-zero) slots.  Returns rois [b, R, 4] fp32 (the proposal rows, bitwise), class_ids [b, R] int32, deltas
    and mask_boxes [b, R, 4] float64, mask_box_ids [b, R] int32 (image * G + the slot's GT; image * G on unused slots),
    is_positive [b, R] fp32 and sel [b, R]: the proposal index in every slot, -1 on unused ones."""
    props = np.asarray(proposals, np.float32)
    ids, gts = np.asarray(gt_class_ids, np.int64), np.asarray(gt_boxes, np.float32)
    b, P = props.shape[:2]
    G, R = ids.shape[1], int(rois_per_image)
    rois = np.zeros((b, R, 4), np.float32)
    cls = np.zeros((b, R), np.int32)
    deltas, mask_boxes = np.zeros((b, R, 4), np.float64), np.zeros((b, R, 4), np.float64)
    box_ids = np.zeros((b, R), np.int32)
    is_pos = np.zeros((b, R), np.float32)
    sel = np.full((b, R), -1, np.int64)
    for i in range(b):
        pos_c, neg_c, arg = det_candidates(props[i], int(num_proposals[i]), ids[i], gts[i])
        pos_cnt = min(len(pos_c), int(positive_cap))
        neg_want = int(np.floor(np.float64(negatives_per_positive) * np.float64(pos_cnt) - np.float64(pos_cnt)))
        neg_cnt = max(min(neg_want, len(neg_c), R, R - pos_cnt), 0)
        kp = np.ascontiguousarray(key_pos[i], np.float32).view(np.uint32).astype(np.int64)      # raw float bits
        kn = np.ascontiguousarray(key_neg[i], np.float32).view(np.uint32).astype(np.int64)
        pos, neg = largest_first(kp, pos_c, pos_cnt), largest_first(kn, neg_c, neg_cnt)
        used = np.concatenate([pos, neg]).astype(np.int64)
        n = len(used)
        sel[i, :n] = used
        rois[i, :n] = props[i][used]
        box_ids[i] = i * G
        box_ids[i, :n] += arg[used].astype(np.int32)
        g = arg[pos]
        cls[i, :pos_cnt] = ids[i][g]
        is_pos[i, :pos_cnt] = 1
        deltas[i, :pos_cnt] = refine_f64(props[i][pos], gts[i][g], bbox_std_dev)
        if use_mini_mask:
            bx, gt = props[i][pos].astype(np.float64), gts[i][g].astype(np.float64)
            gh, gw = gt[:, 2] - gt[:, 0], gt[:, 3] - gt[:, 1]
            mask_boxes[i, :pos_cnt] = np.stack([(bx[:, 0] - gt[:, 0]) / gh, (bx[:, 1] - gt[:, 1]) / gw,
                                                (bx[:, 2] - gt[:, 0]) / gh, (bx[:, 3] - gt[:, 1]) / gw], 1)
        else:
            mask_boxes[i, :pos_cnt] = props[i][pos]
    return DetTargets(rois, cls, deltas, mask_boxes, box_ids, is_pos, sel)
