/*
 * fi_cocoeval.h -- C ABI of libfi_cocoeval.so, the MI355X (gfx950) kernels of COCO detection evaluation (iouType
 * bbox and segm, useCats = 1): the step after the result dicts of the evaluation path (include/fi_eval.h).  A library
 * of its own next to libfi_hip.so (include/fi_capi.h), which it links against and whose conventions it follows:
 * device pointers, a hipStream_t as void*, caller-allocated outputs and workspaces, no host synchronisation, FI_OK or
 * a negative FI_ERR_* status with the message in libfi_hip's fi_last_error().
 *
 * Layout shared by the entry points.  A "pair" is one (image, category) that has at least one ground truth or one
 * detection among the evaluated images and categories.  Pairs are ordered by (category index, image index).  The
 * ground truths of a pair keep annotation order; its detections are ordered by descending score (stable) and cut to
 * maxDets[-1].  dt_off / gt_off [num_pairs + 1] are the exclusive scans of the per-pair counts, iou_off
 * [num_pairs + 1] that of D_p * G_p.  Boxes are [x, y, w, h] doubles, ids are non-zero int64 (0 means "no match").
 * An RLE is a row (first count, number of counts, h, w) of int64 into a flat uint32 count array: the form that
 * fi_unmold_encode writes.
 */
#ifndef FI_COCOEVAL_H_
#define FI_COCOEVAL_H_

#include "fi_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------
 * RLE bounding box and area.
 * Replaces: rleToBbox  datasets/eval/common/maskApi.c:133-146 and rleArea  maskApi.c:72-75 (maskUtils.toBbox /
 *           maskUtils.area in loadRes, pycocotools/coco.py:337-339, and the pre-test boxes of rleIou).
 * rles [num_rles, 4] int64, counts uint32; bbox [num_rles, 4] and area [num_rles] fp64 (uint32 arithmetic as in the
 * C, then converted).  An RLE with fewer than two counts has the box (0, 0, 0, 0).
 * ---------------------------------------------------------------------- */
int fi_coco_rle_stats(const uint32_t *counts, const long long *rles, long long num_rles, double *bbox, double *area,
                      fi_stream_t stream);

/* ------------------------------------------------------------------------
 * IoU of every (detection, ground truth) of every pair.
 * Replaces: COCOeval.computeIoU  pycocotools/cocoeval.py:161-188 -> maskUtils.iou -> bbIou  maskApi.c:109-120 and
 *           rleIou  maskApi.c:77-96.  Bit-exact (tests/golden/cocoeval.npz).
 * ious [num_elems] fp64: pair p at iou_off[p], row-major [D_p, G_p].  gt_crowd [num_gt] uint8 turns the union into
 * the detection's area.  bbox: the five RLE arguments are NULL.  segm: dt_box / gt_box are the RLE boxes of
 * fi_coco_rle_stats (the pre-test), dt_rles / gt_rles [., 4] the RLEs of each detection / ground truth in the same
 * order, dt_rle_area the detections' rleArea; a pair of different sizes whose boxes overlap gives -1.
 * ---------------------------------------------------------------------- */
int fi_coco_iou(long long num_pairs, const long long *dt_off, const long long *gt_off, const long long *iou_off,
                long long num_elems, const double *dt_box, const double *gt_box, const uint8_t *gt_crowd,
                const long long *dt_rles, const uint32_t *dt_counts, const double *dt_rle_area,
                const long long *gt_rles, const uint32_t *gt_counts, double *ious, fi_stream_t stream);

/* ------------------------------------------------------------------------
 * Greedy matching of every (pair, area range, IoU threshold).
 * Replaces: COCOeval.evaluateImg  pycocotools/cocoeval.py:233-311 over the loop of evaluate()  :150-156.
 * iou_thrs [T], area_rng [A, 2] fp64 (device); T * A <= 64.  gt_crowd is both iscrowd and the `ignore` flag
 * (cocoeval.py:105-107).  Outputs: dt_match, dt_ignore [num_dt, A, T] (matched ground-truth id or 0; matched to an
 * ignored ground truth, or unmatched with dt_area outside the range), gt_match [num_gt, A, T] (detection id or 0),
 * gt_ignore [num_gt, A].  workspace: fi_coco_match_workspace_bytes(num_gt, A) bytes; afterwards it holds, as int32,
 * gtind of cocoeval.py:255 for pair p and range a at gt_off[p] * A + a * G_p (ignored ground truths last).
 * No limit on the ground truths or detections of a pair.
 * ---------------------------------------------------------------------- */
size_t fi_coco_match_workspace_bytes(long long num_gt, int A);
int fi_coco_match(long long num_pairs, const long long *dt_off, const long long *gt_off, const long long *iou_off,
                  const double *ious, const double *dt_area, const long long *dt_id, const double *gt_area,
                  const uint8_t *gt_crowd, const long long *gt_id, const double *iou_thrs, const double *area_rng,
                  int T, int A, long long *dt_match, uint8_t *dt_ignore, long long *gt_match, uint8_t *gt_ignore,
                  void *workspace, fi_stream_t stream);

/* ------------------------------------------------------------------------
 * Precision / recall / score tables.
 * Replaces: COCOeval.accumulate  pycocotools/cocoeval.py:313-417.
 * cat_dt_off / cat_gt_off [K + 1]: the detections / ground truths of category k (pairs are category-major);
 * order [num_dt] int64: the detection indices of each category by descending score, stable (ties keep image order,
 * then rank); dt_rank [num_dt] int32: rank inside the pair (the cut to max_dets[m]); rec_thrs [R] ascending,
 * max_dets [M] int32 (device).  R <= 1024, M <= 16, T * A <= 64.
 * Outputs fp64, every cell written: precision, scores [T, R, K, A, M], recall [T, K, A, M]; -1 where the category
 * has no pair or no ground truth that is not ignored.
 * ---------------------------------------------------------------------- */
int fi_coco_accumulate(int K, const long long *cat_dt_off, const long long *cat_gt_off, const long long *order,
                       const int32_t *dt_rank, const double *dt_score, const long long *dt_match,
                       const uint8_t *dt_ignore, const uint8_t *gt_ignore, const double *rec_thrs,
                       const int32_t *max_dets, int T, int R, int A, int M, double *precision, double *recall,
                       double *scores, fi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FI_COCOEVAL_H_ */
