/*
 * fi_eval.h -- C ABI of libfi_eval.so, the MI355X (gfx950) kernels of the EVALUATION path (inference
 * post-processing).  They are not part of a train step, so they live in a library of their own next to
 * libfi_hip.so (include/fi_capi.h), which it links against and whose conventions it follows: device pointers unless
 * the name ends in _host, a hipStream_t as void*, caller-allocated outputs and workspaces, no host synchronisation,
 * FI_OK or a negative FI_ERR_* status with the message in libfi_hip's fi_last_error().
 */
#ifndef FI_EVAL_H_
#define FI_EVAL_H_

#include "fi_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------
 * Inference unmolding: detections -> image-space boxes, full-image masks and COCO RLE.
 * Replaces: the per-image / per-detection host loop of test_model  lib/workflow.py:366-432:
 *           _unmold_detections  lib/workflow.py:523-600 (N, float64 box transform, zero-area filter),
 *           unmold_mask  tools/image_utils.py:172-189 (scipy.misc.imresize = SciPy 1.0 bytescale + Pillow 8-bit
 *           BILINEAR resize, `>= 0.5` threshold, paste), maskUtils.encode -> rleEncode / rleToString
 *           datasets/eval/common/maskApi.c:32-41, :203-215.  Bit-exact (tests/golden/unmold.npz).
 * detections [batch, num_dets, 6] fp32 (y1, x1, y2, x2 in molded pixels, class id, score; the first row with
 * class id 0 ends an image's detections); mrcnn_mask [batch, num_dets, num_classes, mask_h, mask_w] fp32;
 * windows [batch, 4] fp32 (y1, x1, y2, x2); image_hw [batch, 2] int32 original (H, W) and image_hw_host the same
 * values on the host (checked here: 1..4096 px per side).  mask_h, mask_w in 1..64.
 * Outputs, per image b, slots b*num_dets + j for j < num_valid[b] (later slots are not written):
 *   boxes [., 4] int32 (y1, x1, y2, x2 in image pixels), class_ids [.] int32, scores [.] fp32, num_valid [batch];
 *   sizes [batch*num_dets][2] int64: the number of RLE counts and the length of the COCO string of each slot
 *   (0 for unused slots).
 * Decisions: masks are pasted clipped to the image; boxes flipped on both axes or with an extent of
 * 2^31 px or more are dropped like zero-area ones; if dev_status != NULL, a class id outside [0, num_classes)
 * sets bit 0 (its mask is all zero) and a window of zero or negative extent sets bit 1 (the image has no
 * detections).
 * workspace: fi_unmold_workspace_bytes(batch, num_dets, mask_h, mask_w) bytes, kept between the three calls.
 * fi_unmold_encode: offsets [batch*num_dets][2] int64 = exclusive scan of sizes; writes the counts (uint32) and
 * the string characters (no terminator) of every used slot at those offsets.
 * fi_unmold_paste: dense uint8 masks [n_b, H_b, W_b] of every image, back to back (masks 16-byte aligned,
 * total_bytes = sum over images of num_valid[b] * H_b * W_b); it writes every byte.
 * ---------------------------------------------------------------------- */
size_t fi_unmold_workspace_bytes(int batch, int num_dets, int mask_h, int mask_w);
int fi_unmold_prepare(const float *detections, const float *mrcnn_mask, const int32_t *image_hw,
                      const int32_t *image_hw_host, const float *windows, int batch, int num_dets, int num_classes,
                      int mask_h, int mask_w, int32_t *boxes, int32_t *class_ids, float *scores, int32_t *num_valid,
                      long long *sizes, int32_t *dev_status, void *workspace, fi_stream_t stream);
int fi_unmold_encode(const int32_t *image_hw, const int32_t *image_hw_host, const int32_t *boxes,
                     const int32_t *num_valid, int batch, int num_dets, int mask_h, int mask_w, const void *workspace,
                     const long long *offsets, uint32_t *counts, uint8_t *strings, fi_stream_t stream);
int fi_unmold_paste(const int32_t *image_hw, const int32_t *image_hw_host, const int32_t *boxes,
                    const int32_t *num_valid, int batch, int num_dets, int mask_h, int mask_w, const void *workspace,
                    long long total_bytes, uint8_t *masks, fi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FI_EVAL_H_ */
