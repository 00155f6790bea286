/*
 * fi_heads16.h -- C ABI of libfi_heads16.so: the two memory-bound backward launches that let a train step run its box and
 * mask heads on 16-bit channels-last crops (bf16 / IEEE half), MI355X (gfx950): the RoIAlign backward that reads 16-bit
 * channels-last crop gradients ([num_boxes, crop_h, crop_w, depth] in memory) and adds into fp32 channels-last pyramid
 * gradient maps, and the backward of the mask head's last 1x1 layer when the loss reads one class per RoI.  The
 * convolutions, the forward RoIAlign and the pack of the fp32 maps belong to other libraries; nothing of them is restated.
 * A library of its own next to libfi_hip.so (include/fi_capi.h), which it links against and whose conventions it
 * follows: device pointers, a hipStream_t as void*, caller-allocated outputs, no host synchronisation, FI_OK or a negative
 * FI_ERR_* status with the message in libfi_hip's fi_last_error().  Every argument is checked on the host before any HIP
 * call.
 */
#ifndef FI_HEADS16_H_
#define FI_HEADS16_H_

#include "fi_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FI_HEADS16_CROP_BWD 0
#define FI_HEADS16_CLASS_ROWS 1

/* ------------------------------------------------------------------------
 * 1 when the entry point of `kind` takes the call, 0 otherwise.  HOST function, no GPU work; the pointers are only
 * inspected for alignment (NULL = absent or not known yet, taken as aligned).  THE statement of the rules:
 * every kind: C % 8 == 0 (C >= 8), n >= 1, h >= 1, w >= 1.
 * FI_HEADS16_CROP_BWD: m = pyramid levels, 1..8; C = depth <= 2^20; h x w = the crop, each at most 64; n = boxes, and the launch's
 *   n * ceil(h w / 64) workgroups below 2^31; f32_ptrs (NULL, or a HOST array of m device pointers: the gradient maps) each
 *   4-byte aligned; p0 = grads 16-byte aligned; p1..p3 unused.
 * FI_HEADS16_CLASS_ROWS: m = K classes, any K >= 1; C = the channels of one of the four (a, b) groups; h x w = the map
 *   H x W of a RoI with H * W <= 2^28; n = RoIs; ceil(C / 64) <= 65535; f32_ptrs (NULL, or a HOST array of 3 device
 *   pointers: colsum, dweight, dbias, each of which may be NULL) each 4-byte aligned; p0 = u, p1 = w, p2 = du 16-byte
 *   aligned; p3 = d 4-byte aligned.
 * ---------------------------------------------------------------------- */
int fi_heads16_eligible(int kind, int m, int C, int h, int w, int n, const void *const *f32_ptrs, const void *p0,
                        const void *p1, const void *p2, const void *p3);

/* ------------------------------------------------------------------------
 * The backward of the single-tap pyramid RoIAlign that writes 16-bit channels-last crops.  grads [num_boxes, crop_h,
 * crop_w, depth] 16-bit; level_grads_host a HOST array of num_levels device pointers to fp32 channels-last maps
 * [batch, level_h_host[l], level_w_host[l], depth]; boxes [num_boxes, 4] fp32 (y1, x1, y2, x2, normalised), box_ind and
 * level int32 [num_boxes] -- box i reads map level[i] - 2 of image box_ind[i]; level may be NULL with one map: the
 * contract of fi_pyramid_crop_backward_nhwc.  accumulate == 0: every map is zero-filled first (hipMemsetAsync on the
 * stream, also when num_boxes == 0); accumulate != 0: the maps are added to as they stand.
 * Arithmetic, per bin (y, x) with a valid tap pair and channel c: g = (float)grads[i][y][x][c], exact;
 *     gtop = (1 - fy) * g, gbot = fy * g;   TL += (1 - fx) * gtop, TR += fx * gtop, BL += (1 - fx) * gbot, BR += fx * gbot
 * each product rounded to fp32 on its own, (i0, i1, frac, valid) of an axis from the sampling table of the forward (the
 * box transform of the reference, operation order kept), each sum an fp32 ATOMIC add: the sums depend on the order in
 * which the adds arrive, and their last bits may differ between two runs, as those of the fp32 atomic form do.
 * Nothing is added for a box whose level is outside [2, 2 + num_levels) -- level[i] == -1 included --, whose box_ind is
 * outside [0, batch), or for a bin whose tap is invalid on either axis.
 * One workgroup per (box, slab of 64 bins).  A lane reads 8 channels of a bin with one 16-byte load; the wavefront then
 * re-deals its 512 values through 1 KB of LDS so that lane L of atomic instruction j holds value 64 j + L of the run:
 * neighbouring lanes add to neighbouring channels, a wave-instruction covers 256 contiguous bytes of a map row wherever
 * depth >= 64.  One launch; num_boxes == 0 launches nothing.
 * Status: FI_ERR_INVALID_ARG for num_boxes < 0, batch, depth, crop_h or crop_w < 1, a null pointer, num_levels outside
 * 1..8, a map size < 1, level == NULL with several maps and boxes to read it for; FI_ERR_UNSUPPORTED for what fi_heads16_eligible answers 0 --
 * before anything is launched or cleared.
 * ---------------------------------------------------------------------- */
int fi_heads16_pyramid_crop_backward_bf16(const void *grads, float *const *level_grads_host, const int *level_h_host,
                                          const int *level_w_host, int num_levels, const float *boxes,
                                          const int32_t *box_ind, const int32_t *level, int num_boxes, int batch, int depth,
                                          int crop_h, int crop_w, int accumulate, fi_stream_t stream);
int fi_heads16_pyramid_crop_backward_f16(const void *grads, float *const *level_grads_host, const int *level_h_host,
                                         const int *level_w_host, int num_levels, const float *boxes,
                                         const int32_t *box_ind, const int32_t *level, int num_boxes, int batch, int depth,
                                         int crop_h, int crop_w, int accumulate, fi_stream_t stream);

/* ------------------------------------------------------------------------
 * The backward of logits[i, a, b, h, w] = bias[cls[i]] + sum_c u[i, h, w, (2a + b) C + c] * w[cls[i], c]: the mask head's
 * last 1x1 layer behind the 2 x 2 / stride 2 transposed convolution run as a 1x1 layer, when the loss reads the class
 * cls[i] of RoI i and nothing else.
 * d fp32 [n, 2, 2, H, W]; u 16-bit [n, H, W, 4 C], the ReLU output of the layer in front, channel (2a + b) C + c;
 * w 16-bit [K, C]; cls int64 [n], each in [0, K).
 *     du[i, h, w, (2a + b) C + c] = u > 0 ? round_to_nearest_even_16(d[i, a, b, h, w] * (float)w[cls[i], c]) : +0
 * one rounding of one fp32 product; u == 0, u == -0.0 and a NaN u select zero.  Every element of du is written exactly
 * once; its bits depend neither on the grid nor on the run.
 *     colsum[(2a + b) C + c] (fp32, [4 C], optional) = sum over i, h, w of (float)du, the values AS STORED
 *     dweight[cls[i], c] (fp32, [K, C], optional) += sum over a, b, h, w of d[i, a, b, h, w] * (float)u[i, h, w, (2a + b) C + c]
 *     dbias[cls[i]] (fp32, [K], optional) += sum over a, b, h, w of d[i, a, b, h, w]
 * colsum is zero-filled by the call (hipMemsetAsync on the stream, also when n == 0); dweight and dbias are ACCUMULATED
 * into, and rows of classes no RoI has are not touched.  A RoI whose class lies outside [0, K) gets du = +0 and adds
 * nothing.
 * The ATOMIC form is what is built: one workgroup per (RoI, tile of channels) sums everything that shares a destination
 * on chip -- a thread keeps 8 channels for all its rows in fp32 registers, the threads of a workgroup combine in LDS --
 * and then adds one value per (RoI, channel) to dweight, one per (RoI, (a, b), channel) to colsum and one per RoI to
 * dbias with global fp32 atomics.  No class table is kept on chip, so K is not bounded.  du is bit-reproducible; the
 * three sums are NOT: their last bits depend on the order of the adds.
 * One launch; n == 0 launches nothing.
 * Status: FI_ERR_INVALID_ARG for n < 0, H, W, C or K < 1, a null d, u, w, cls or du; FI_ERR_UNSUPPORTED for what
 * fi_heads16_eligible answers 0 -- before anything is launched or cleared.
 * ---------------------------------------------------------------------- */
int fi_heads16_class_rows_backward_bf16(const float *d, const void *u, const void *w, const int64_t *cls, void *du,
                                        float *colsum, float *dweight, float *dbias, int n, int H, int W, int C, int K,
                                        fi_stream_t stream);
int fi_heads16_class_rows_backward_f16(const float *d, const void *u, const void *w, const int64_t *cls, void *du,
                                       float *colsum, float *dweight, float *dbias, int n, int H, int W, int C, int K,
                                       fi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FI_HEADS16_H_ */
