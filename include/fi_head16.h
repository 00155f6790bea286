/*
 * fi_head16.h -- C ABI of libfi_head16.so: the two kernels that keep the box head and the mask head on 16-bit
 * channels-last tensors (bf16 / IEEE half, [N, H, W, C] in memory: the tensors of include/fi_act16.h), MI355X (gfx950):
 * pyramid RoIAlign that reads 16-bit channels-last maps and WRITES 16-bit channels-last crops, and a 1x1 output layer
 * that reads 16-bit rows and writes fp32 for any number of output channels, with an optional sigmoid and an optional
 * 2 x 2 pixel shuffle in its epilogue.  The layers between them run on fi_act16_conv_forward.  A library of its own next
 * to libfi_hip.so (include/fi_capi.h), which it links against and whose conventions it follows: device pointers, a
 * hipStream_t as void*, caller-allocated outputs, no host synchronisation, FI_OK or a negative FI_ERR_* status with the
 * message in libfi_hip's fi_last_error().  Every argument is checked on the host before any HIP call; num_boxes == 0 and
 * P == 0 are FI_OK and launch nothing.  Forward only.
 */
#ifndef FI_HEAD16_H_
#define FI_HEAD16_H_

#include "fi_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------
 * 1 when fi_head16_pyramid_crop_forward_{bf16,f16} takes this call, 0 otherwise.  HOST function, no GPU work; the table
 * of level pointers (host memory; NULL = not known yet) and crops are only inspected for alignment (a NULL pointer is
 * taken as aligned).  THE one statement of the rules:
 * 1 <= num_levels <= 8, depth % 8 == 0 (and >= 8), 1 <= crop_h, crop_w <= 64 (the per-axis sampling tables), every
 * level map and crops 16-byte aligned.  There is no LDS tile and hence no bound on crop_h * crop_w or rule on channel
 * chunks.  The one rule that needs the box count is checked by the entry point itself: num_boxes * ceil(crop_h * crop_w
 * / 64), the workgroup count, stays below 2^31, FI_ERR_UNSUPPORTED otherwise.
 * ---------------------------------------------------------------------- */
int fi_head16_crop_eligible(int num_levels, int depth, int crop_h, int crop_w,
                            const void *const *level_images_host, const void *crops);

/* ------------------------------------------------------------------------
 * crops[i] = RoIAlign of box i on the map of its level and image, one launch for all levels, 16-bit in and out.
 * Replaces: fi_roi16_pyramid_crop_forward (include/fi_roi16.h) and the fp32 NCHW crops it writes -- the same contract
 *           for the level table, boxes, box_ind, level, batch and extrapolation_value.
 * crops [num_boxes, crop_h, crop_w, depth] in the maps' 16-bit type: a box's crop is one contiguous run, and viewed as
 * [num_boxes, 1, 1, crop_h * crop_w * depth] it is the operand row of a full-window convolution with a tap-major weight.
 * Rows: a level outside [2, 2 + num_levels) or a box_ind outside [0, batch) gives a row of zeros; level[i] == -1 leaves
 * the row unwritten.  A bin whose sample falls outside the map is extrapolation_value (rounded to the type).
 * Arithmetic: the fp32 value fi_roi16_pyramid_crop_forward forms (the same box transform, the four taps widened exactly,
 * top = tl + (tr - tl) * fx, bot likewise, top + (bot - top) * fy, each operation rounded separately), then ONE
 * round-to-nearest-even to the 16-bit type at the store.  Every element is written once by one lane (8 channels of a
 * bin: one 16-byte store), no atomics.
 * Status: FI_ERR_INVALID_ARG for num_boxes < 0, batch, depth, crop_h or crop_w < 1, a null table / boxes / box_ind /
 * crops, a null map or an extent < 1 in the table, a null level with num_levels > 1; FI_ERR_UNSUPPORTED for a call
 * fi_head16_crop_eligible answers 0 -- all before anything is launched.
 * ---------------------------------------------------------------------- */
int fi_head16_pyramid_crop_forward_bf16(const void *const *level_images_host, const int *level_h_host,
                                        const int *level_w_host, int num_levels, const float *boxes,
                                        const int32_t *box_ind, const int32_t *level, int num_boxes, int batch,
                                        int depth, int crop_h, int crop_w, float extrapolation_value, void *crops,
                                        fi_stream_t stream);
int fi_head16_pyramid_crop_forward_f16(const void *const *level_images_host, const int *level_h_host,
                                       const int *level_w_host, int num_levels, const float *boxes,
                                       const int32_t *box_ind, const int32_t *level, int num_boxes, int batch,
                                       int depth, int crop_h, int crop_w, float extrapolation_value, void *crops,
                                       fi_stream_t stream);

/* ------------------------------------------------------------------------
 * 1 when fi_head16_out1x1_{bf16,f16} takes this call, 0 otherwise.  HOST function; the pointers are only inspected for
 * alignment (NULL = not known yet, taken as aligned).  THE one statement of the rules:
 * P >= 1, Cin % 32 == 0 (and >= 32), Cout >= 1 (any value: 64-row channel tiles over the grid), act 0 or 1, layout 0 or
 * 1, x and w 16-byte aligned, y 4-byte aligned, and P, Cout * Cin and the workgroup count ceil(P / 128) * ceil(Cout / 64)
 * all below 2^31.  layout 1 needs n, H, W >= 1 and P == n * H * W * 4; layout 0 ignores n, H and W.
 * ---------------------------------------------------------------------- */
int fi_head16_out1x1_eligible(int P, int Cin, int Cout, int act, int layout, int n, int H, int W, const void *x,
                              const void *w, const void *y);

/* ------------------------------------------------------------------------
 * y = act(x w^T + bias) in fp32, stored unrounded, one launch.
 * Replaces: the box head's stacked class + box linears (lib/sub_module.py, Classifier.forward) and the mask head's conv5,
 *           sigmoid and pixel shuffle (Mask.forward) with the permute copy behind them.
 * x [P, Cin] and w [Cout, Cin] 16-bit (bf16 / half by the entry point's suffix); bias [Cout] fp32, optional (NULL);
 * y FP32.  act: 0 = none, 1 = sigmoid, 1 / (1 + exp(-v)) evaluated in fp32 on v = acc + bias.
 * layout 0 (rows): y[p, co], a [P, Cout] matrix.
 * layout 1 (shuffle): y is [n, Cout, 2H, 2W]; row p = ((i * H + h) * W + w) * 4 + 2a + b goes to y[i, co, 2h + a, 2w + b]
 * -- x is the (a, b, c)-ordered output of a 2 x 2 / stride 2 transposed convolution run as a 1x1 convolution.
 * Arithmetic: the main loop of fi_act16_conv_forward on 64-row channel tiles, as fi_pyr16_head1x1 (include/fi_pyr16.h):
 * the 16-bit products are exact in fp32 and accumulate in fp32, input channels ascending; acc + bias is one fp32
 * addition.  With act 0 an element's bits are those fi_pyr16_head1x1 produces for the same weight row.  Every element is
 * written once, no atomics, no split over the reduction.  Stores: 4 bytes per lane; layout 0, neighbouring lanes on
 * neighbouring channels of a row (runs of up to 64 floats); layout 1, neighbouring lanes on neighbouring floats of an
 * output row (runs of up to 2W floats).
 * Status: FI_ERR_INVALID_ARG for a null x / w / y, P < 0, Cin or Cout < 1; FI_ERR_UNSUPPORTED for a call
 * fi_head16_out1x1_eligible answers 0 -- both before anything is launched.
 * ---------------------------------------------------------------------- */
int fi_head16_out1x1_bf16(const void *x, const void *w, const float *bias, float *y, int P, int Cin, int Cout, int act,
                          int layout, int n, int H, int W, fi_stream_t stream);
int fi_head16_out1x1_f16(const void *x, const void *w, const float *bias, float *y, int P, int Cin, int Cout, int act,
                         int layout, int n, int H, int W, fi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FI_HEAD16_H_ */
