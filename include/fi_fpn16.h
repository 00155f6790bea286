/*
 * fi_fpn16.h -- C ABI of libfi_fpn16.so: the backward of the feature pyramid's top-down step on 16-bit channels-last
 * activation tensors (bf16 / IEEE half, [N, H, W, C] in memory), MI355X (gfx950).  The forward of that step (the lateral
 * launch of the 16-bit pyramid library) adds the coarser level read at half resolution, so the gradient into the coarser
 * level is the sum over each 2 x 2 cell of the finer level's gradient.  This library adds that sum to the coarser level's
 * own gradient with one rounding and sums the result per channel -- the bias gradient of the layer that made the coarser
 * level -- in one launch.  The data and weight gradients of the pyramid's convolutions are those of the 16-bit backward
 * library and of the gated data gradient of the 16-bit training library; nothing of them is restated here.
 * A library of its own next to libfi_hip.so (include/fi_capi.h), which it links against and whose conventions it
 * follows: device pointers, a hipStream_t as void*, caller-allocated outputs, no host synchronisation, FI_OK or a negative
 * FI_ERR_* status with the message in libfi_hip's fi_last_error().  Every argument is checked on the host before any HIP
 * call; N == 0 is FI_OK and launches nothing.
 *
 * Tensors: H, W are the COARSE map.  own and g [N, H, W, C], fine [N, 2H, 2W, C], all 16-bit (bf16 / half by the entry
 * point's suffix); colsum [C] fp32.
 */
#ifndef FI_FPN16_H_
#define FI_FPN16_H_

#include "fi_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------
 * 1 when fi_fpn16_topdown_grad_* takes the call, 0 otherwise.  HOST function, no GPU work; the pointers are only
 * inspected for alignment (NULL = absent or not known yet, taken as aligned).  THE statement of the rules:
 * Eligible: N, H, W >= 1, C % 8 == 0 (C >= 8), own, fine and g 16-byte aligned, colsum 4-byte aligned, and N*2H*2W and
 * the workgroup count of the launch both below 2^31.
 * ---------------------------------------------------------------------- */
int fi_fpn16_eligible(int N, int H, int W, int C, const void *own, const void *fine, const void *g, const void *colsum);

/* ------------------------------------------------------------------------
 * The top-down step's backward with column sums, one kernel launch.  Per element, all in fp32, in exactly this order,
 * every operation rounded on its own (no contraction):
 *     t = ((float)fine[n,2h,2w,c] + (float)fine[n,2h,2w+1,c]) + ((float)fine[n,2h+1,2w,c] + (float)fine[n,2h+1,2w+1,c])
 *     v = (float)own[n,h,w,c] + t          own == NULL: v = t          fine == NULL: v = (float)own
 *     g[n,h,w,c] = round_to_nearest_even_16(v)                         ONE rounding, at the store
 *     colsum[c]  = sum over the N*H*W pixels of (float)g[.., c]        of the values AS ROUNDED
 * own and fine are optional (NULL), not both.  g is REQUIRED and may be own itself (in place: a lane reads the 8 values
 * it then writes).  With fine == NULL and g == own nothing would change and the store is skipped: the call is a
 * read-only column-sum pass over own.  Every element of g is written exactly once by one lane; its bits depend neither on
 * the grid nor on the run.  No saturation: an fp16 overflow rounds to infinity as IEEE 754 says (keeping the gradients
 * in range is the loss scale's business).
 * colsum is optional (NULL).  It is zero-filled by the call (hipMemsetAsync on the stream).  A thread keeps 8 channels
 * for all its pixels and sums them in fp32 registers; the threads of a workgroup combine in LDS; the workgroup adds one
 * value per channel with an fp32 ATOMIC (global_atomic_add_f32).  The order of that sum, and with it the last bits of
 * colsum, may differ between two runs: colsum is NOT bit-reproducible.  g does not depend on it.
 * Status: FI_ERR_INVALID_ARG for N < 0, H, W or C < 1, a null g, or own and fine both null; FI_ERR_UNSUPPORTED for a call
 * fi_fpn16_eligible answers 0 -- both before anything is launched.
 * ---------------------------------------------------------------------- */
int fi_fpn16_topdown_grad_bf16(const void *own, const void *fine, void *g, float *colsum, int N, int H, int W, int C,
                               fi_stream_t stream);
int fi_fpn16_topdown_grad_f16(const void *own, const void *fine, void *g, float *colsum, int N, int H, int W, int C,
                              fi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FI_FPN16_H_ */
