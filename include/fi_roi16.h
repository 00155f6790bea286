/*
 * fi_roi16.h -- C ABI of libfi_roi16.so: pyramid RoIAlign that READS 16-bit channels-last maps (bf16 / IEEE half,
 * [batch, H, W, depth] in memory: the tensors of include/fi_act16.h) and writes the fp32 NCHW crops the box head, the
 * feature extractor and the mask head consume, MI355X (gfx950).  A library of its own next to libfi_hip.so
 * (include/fi_capi.h), which it links against and whose conventions it follows: device pointers, a hipStream_t as void*,
 * caller-allocated outputs, no host synchronisation, FI_OK or a negative FI_ERR_* status with the message in libfi_hip's
 * fi_last_error().  Every argument is checked on the host before any HIP call; num_boxes == 0 is FI_OK and launches
 * nothing.  Forward only.
 */
#ifndef FI_ROI16_H_
#define FI_ROI16_H_

#include "fi_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------
 * 1 when fi_roi16_pyramid_crop_forward_{bf16,f16} takes this call, 0 otherwise.  HOST function, no GPU work; the table
 * of level pointers (host memory; NULL = not known yet) and crops are only inspected for alignment (a NULL pointer is
 * taken as aligned).  THE one statement of the rules:
 * 1 <= num_levels <= 8, depth % 8 == 0 (and >= 8), 1 <= crop_h, crop_w <= 64 and crop_h * crop_w <= 220 (the fp32
 * channels-last kernel's bounds: its LDS tables and tile), every level map 16-byte aligned, crops 4-byte aligned.
 * The one rule that needs the box count is checked by the entry point itself: num_boxes * ceil(depth / chunk), the
 * workgroup count, stays below 2^31 (chunk = 64..256 channels by the tile's size), FI_ERR_UNSUPPORTED otherwise.
 * There is no scalar-lane kernel behind a refusal.
 * ---------------------------------------------------------------------- */
int fi_roi16_crop_eligible(int num_levels, int depth, int crop_h, int crop_w,
                           const void *const *level_images_host, const void *crops);

/* ------------------------------------------------------------------------
 * crops[i] = RoIAlign of box i on the map of its level and image, one launch for all levels.
 * Replaces: fi_pyramid_crop_forward_nhwc (include/fi_capi.h) behind four fi_act16_unpack launches -- the same contract
 *           with level maps [batch, level_h[l], level_w[l], depth] in bf16 / half (by the entry point's suffix).
 * level_images_host / level_h_host / level_w_host [num_levels]: HOST arrays (device pointers and extents of the maps).
 * boxes [num_boxes, 4] fp32 (y1, x1, y2, x2, normalised), box_ind [num_boxes] int32 (image), level [num_boxes] int32
 * (pyramid level, 2 = first map; may be NULL when num_levels == 1).  crops [num_boxes, depth, crop_h, crop_w] FP32.
 * Rows: a level outside [2, 2 + num_levels) or a box_ind outside [0, batch) gives a row of zeros; level[i] == -1 leaves
 * the row unwritten.  A bin whose sample falls outside the map is extrapolation_value.
 * Arithmetic: the box transform of fi_pyramid_crop_forward_nhwc, operation order kept; the four taps are widened
 * exactly to fp32 and interpolated by its expression in its order (top = tl + (tr - tl) * fx, bot likewise,
 * top + (bot - top) * fy, each operation rounded separately).  The crops are BIT-IDENTICAL to
 * fi_pyramid_crop_forward_nhwc on the widened maps; nothing is rounded to 16 bits.  Every element is written once by
 * one lane, no atomics.
 * Status: FI_ERR_INVALID_ARG for num_boxes < 0, batch, depth, crop_h or crop_w < 1, a null table / boxes / box_ind /
 * crops, a null map or an extent < 1 in the table, a null level with num_levels > 1; FI_ERR_UNSUPPORTED for a call
 * fi_roi16_crop_eligible answers 0 -- all before anything is launched.
 * ---------------------------------------------------------------------- */
int fi_roi16_pyramid_crop_forward_bf16(const void *const *level_images_host, const int *level_h_host,
                                       const int *level_w_host, int num_levels, const float *boxes,
                                       const int32_t *box_ind, const int32_t *level, int num_boxes, int batch,
                                       int depth, int crop_h, int crop_w, float extrapolation_value, float *crops,
                                       fi_stream_t stream);
int fi_roi16_pyramid_crop_forward_f16(const void *const *level_images_host, const int *level_h_host,
                                      const int *level_w_host, int num_levels, const float *boxes,
                                      const int32_t *box_ind, const int32_t *level, int num_boxes, int batch,
                                      int depth, int crop_h, int crop_w, float extrapolation_value, float *crops,
                                      fi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FI_ROI16_H_ */
