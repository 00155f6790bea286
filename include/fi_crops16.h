/*
 * fi_crops16.h -- C ABI of libfi_crops16.so: the three memory-bound launches that let a train step keep its feature
 * pyramid on 16-bit channels-last tensors (bf16 / IEEE half, [N, H, W, C] in memory) up to the RoI crops, MI355X (gfx950):
 * the gather of the RPN's 3 x 3 patches at the sampled anchors from 16-bit maps, its backward INTO 16-bit gradient maps
 * (sparse, in place, without atomics) and the pass that turns the fp32 channels-last gradient of a RoIAlign backward
 * into the masked 16-bit gradient of the layer in front of it, with that layer's column sums.  The convolutions and
 * RoIAlign itself belong to other libraries; nothing of them is restated here.
 * A library of its own next to libfi_hip.so (include/fi_capi.h), which it links against and whose conventions it
 * follows: device pointers, a hipStream_t as void*, caller-allocated outputs, no host synchronisation, FI_OK or a negative
 * FI_ERR_* status with the message in libfi_hip's fi_last_error().  Every argument is checked on the host before any HIP
 * call.
 *
 * Pyramid levels.  A level l is described by (pointer, heights[l], widths[l], steps[l]): heights / widths are the size of
 * the TENSOR behind the pointer ([N, heights[l], widths[l], C], 16-bit), and the level is its subsample with stride
 * steps[l] >= 1: ceil(heights[l] / steps[l]) x ceil(widths[l] / steps[l]) pixels, level pixel (h, w) being tensor pixel
 * (h steps[l], w steps[l]).  steps == NULL means 1 everywhere.  The coarsest level of a pyramid whose last map is the
 * stride-2 subsample of the one before it is thus that map's tensor once more, with step 2.  Two levels that share a
 * tensor give the SAME pointer, height and width.
 * Anchors.  Row r is (image[r], anchor[r]) of the level-major anchor list: level l holds its pixel count times
 * anchors_per_location anchors, anchor a of level l sits on level pixel (a - start_l) / anchors_per_location.  A row with
 * image[r] < 0 or >= N, or an anchor outside the list, is a padding row.  Tap t = 0..8 of a row is the level pixel
 * (h + t / 3 - 1, w + t % 3 - 1).
 */
#ifndef FI_CROPS16_H_
#define FI_CROPS16_H_

#include "fi_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FI_CROPS16_PATCH_FWD 0
#define FI_CROPS16_PATCH_BWD 1
#define FI_CROPS16_GATE_PACK 2

/* ------------------------------------------------------------------------
 * 1 when the entry point of `kind` takes the call, 0 otherwise.  HOST function, no GPU work; the pointers are only
 * inspected for alignment (NULL = absent or not known yet, taken as aligned).  THE statement of the rules:
 * every kind: C % 8 == 0 (C >= 8), n >= 1.
 * FI_CROPS16_PATCH_FWD / _BWD: n = rows, at most 2^20; 1 <= levels <= 8; level_ptrs (NULL, or a HOST array of `levels`
 *   device pointers: the maps / the gradient maps) each 16-byte aligned; p0 = the fp32 rows (out / d) 16-byte aligned;
 *   p1..p3 unused.
 * FI_CROPS16_GATE_PACK: n = N * H * W pixels, n and the workgroup count of the launch below 2^31; levels and level_ptrs
 *   unused; p0 = d, p1 = y, p2 = g 16-byte aligned, p3 = sums 4-byte aligned.
 * ---------------------------------------------------------------------- */
int fi_crops16_eligible(int kind, int levels, int C, int n, const void *const *level_ptrs, const void *p0, const void *p1,
                        const void *p2, const void *p3);

/* ------------------------------------------------------------------------
 * out[r][t][c] (fp32, [rows][9][C]) = (float)map_l[image[r]][tap t of row r][c], exact; 0 where the tap falls outside the
 * level and for padding rows.  One pixel's C channels are contiguous: a thread moves 8 channels, one 16-byte load and two
 * 16-byte stores.  Every element of out is written exactly once.  One launch; rows == 0 launches nothing.
 * Status: FI_ERR_INVALID_ARG for rows < 0, N, C or anchors_per_location < 1, a null pointer, levels outside 1..8, a map
 * size or step < 1; FI_ERR_UNSUPPORTED for what fi_crops16_eligible answers 0 -- before anything is launched.
 * ---------------------------------------------------------------------- */
int fi_crops16_patch_rows_forward_bf16(const void *const *maps, const int *heights, const int *widths, const int *steps,
                                       int levels, int anchors_per_location, const int64_t *image, const int64_t *anchor,
                                       int rows, int N, int C, float *out, fi_stream_t stream);
int fi_crops16_patch_rows_forward_f16(const void *const *maps, const int *heights, const int *widths, const int *steps,
                                      int levels, int anchors_per_location, const int64_t *image, const int64_t *anchor,
                                      int rows, int N, int C, float *out, fi_stream_t stream);

/* ------------------------------------------------------------------------
 * The backward of the gather, added IN PLACE into 16-bit gradient maps.  For every element of a gradient tensor that is
 * the destination of at least one (row, tap):
 *     grads_l[image][pixel][c] = round_to_nearest_even_16((float)old + S),   S = sum of d[r][t][c] over those (r, t)
 * S starts at 0 and adds in fp32 in ascending (r, t) order; old is added last; ONE rounding.  Destinations are compared
 * by tensor (pointer), image and tensor pixel, so rows of two levels that share a tensor and meet on one of its pixels
 * are summed into one store.  Each touched element is written exactly once, by the workgroup of the first (r, t) that
 * reaches it; untouched elements are neither read nor written.  No atomics, no dense fp32 map: two runs give the same
 * bits.  One workgroup per (r, t) walks the row list for the other rows with a tap on its pixel -- rows^2 * 9 small
 * integer steps, meant for the few hundred sampled anchors of a train step.  d is fp32 [rows][9][C].
 * One launch; rows == 0 launches nothing.  Status as the forward's; two levels with one pointer and different sizes are
 * FI_ERR_INVALID_ARG.
 * ---------------------------------------------------------------------- */
int fi_crops16_patch_rows_backward_bf16(const float *d, void *const *grads, const int *heights, const int *widths,
                                        const int *steps, int levels, int anchors_per_location, const int64_t *image,
                                        const int64_t *anchor, int rows, int N, int C, fi_stream_t stream);
int fi_crops16_patch_rows_backward_f16(const float *d, void *const *grads, const int *heights, const int *widths,
                                       const int *steps, int levels, int anchors_per_location, const int64_t *image,
                                       const int64_t *anchor, int rows, int N, int C, fi_stream_t stream);

/* ------------------------------------------------------------------------
 * d fp32 [N, H, W, C] -> g 16-bit [N, H, W, C], one pass over d:
 *     g = y > 0 ? round_to_nearest_even_16(d) : +0          y (16-bit, [N, H, W, C]) == NULL: no mask
 *     sums[c] = sum over the N*H*W pixels of (float)g[.., c]      of the values AS ROUNDED; sums == NULL: none
 * Every element of g is written exactly once; its bits depend neither on the grid nor on the run.  No saturation: a value
 * beyond the type's range rounds to infinity as IEEE 754 says.  sums is zero-filled by the call (hipMemsetAsync on the
 * stream); a thread keeps 8 channels for all its pixels and sums them in fp32 registers, the threads of a workgroup
 * combine in LDS, the workgroup adds one value per channel with an fp32 atomic: sums is NOT bit-reproducible, g is.
 * N == 0 zero-fills sums and launches nothing.
 * Status: FI_ERR_INVALID_ARG for N < 0, H, W or C < 1, a null d or g; FI_ERR_UNSUPPORTED for what fi_crops16_eligible
 * answers 0 -- both before anything is launched.
 * ---------------------------------------------------------------------- */
int fi_crops16_gate_pack_bf16(const float *d, const void *y, void *g, float *sums, int N, int H, int W, int C,
                              fi_stream_t stream);
int fi_crops16_gate_pack_f16(const float *d, const void *y, void *g, float *sums, int N, int H, int W, int C,
                             fi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FI_CROPS16_H_ */
