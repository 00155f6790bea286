/*
 * fi_train16.h -- C ABI of libfi_train16.so: the GATED data gradient of a convolution on 16-bit channels-last activation
 * tensors (bf16 / IEEE half, [N, H, W, C] in memory), MI355X (gfx950).  It is the data gradient of the 16-bit backward
 * library (conv_dgrad of include's grad16 header) with the PRODUCING layer's ReLU mask and that layer's column sums in
 * the epilogue: what took a data-gradient launch and a mask-and-sum launch per layer takes one.  A library of its own
 * next to libfi_hip.so (include/fi_capi.h), which it links against and whose conventions it follows: device pointers, a
 * hipStream_t as void*, caller-allocated outputs, no host synchronisation, FI_OK or a negative FI_ERR_* status with the
 * message in libfi_hip's fi_last_error().  Every argument is checked on the host before any HIP call; N == 0 is FI_OK
 * and launches nothing.
 *
 * Tensors (those of the ungated data gradient): g [N, OH, OW, Cout] with OH = (H + 2 pad - R) / stride + 1, the masked
 * output gradient of the layer; dx, dx_add and gate [N, H, W, Cin]; all 16-bit (bf16 / half by the entry point's suffix).
 */
#ifndef FI_TRAIN16_H_
#define FI_TRAIN16_H_

#include "fi_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------
 * 1 when fi_train16_conv_dgrad_gated_* takes the call, 0 otherwise.  HOST function, no GPU work; the four 16-bit
 * pointers are only inspected for alignment (NULL = not known yet, taken as aligned).  The rules are those of the
 * ungated data gradient, stated again for these pointers:
 * Geometry: R == S == 1 with stride 1 or 2 and pad 0, or R == S == 3 with stride 1 and pad 1 (what Bottleneck uses).
 * Eligible: N, H, W >= 1, Cin % 32 == 0, Cout % 32 == 0 (both >= 32), g, gate, dx_add and dx 16-byte aligned, and
 * N*H*W, N*OH*OW, Cout*R*S*Cin and the workgroup count of the launch all below 2^31.
 * wt (16 bytes) and colsum (4 bytes) are checked by the entry point itself.
 * ---------------------------------------------------------------------- */
int fi_train16_eligible(int N, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, const void *g,
                        const void *gate, const void *dx_add, const void *dx);

/* ------------------------------------------------------------------------
 * The gated data gradient with column sums, one kernel launch.  With acc the fp32 reduction of the ungated kernel,
 *     acc[n,h,w,ci] = sum_{r,s,co} g[n,oh,ow,co] * wt[ci,r',s',co]:
 *     t          = round_to_nearest_even_16(acc + (float)dx_add)       exactly what the ungated data gradient stores
 *     dx         = (float)gate > 0 ? t : 0                             a select: gate == 0, -0.0 and NaN select zero
 *     colsum[ci] = sum over the N*H*W pixels of (float)dx              of the values AS STORED
 * wt [Cin, R, S, Cout], 16-bit: the TRANSPOSED, TAP-FLIPPED weight with the BatchNorm scale of co folded in and rounded
 * once.  gate [N, H, W, Cin], 16-bit, REQUIRED: the layer's input, i.e. the producing layer's post-ReLU output.  dx_add
 * [N, H, W, Cin], 16-bit, optional (NULL).  colsum [Cin] fp32, optional (NULL): the `s` of fi_bn_fold_grad for the
 * PRODUCING layer.
 * dx is bit-equal to the mask-and-sum operator applied (with y = gate) to the ungated data gradient of the same g, wt
 * and dx_add: the same main loop, the same tiles (chosen from Cin, N*OH*OW and Cout % 64 as there), the same mapping of
 * accumulators to outputs, one rounding, then the select.  Every element of dx is written exactly once by one lane and
 * two runs agree bit for bit on dx.
 * Stride 1 and the 1x1 / stride-2 scatter are both covered: in the scatter the (up to four) pixels of a 2 x 2 cell are
 * all gated and summed; the pixels an odd map does not have are skipped.
 * colsum is zero-filled by the call (hipMemsetAsync on the stream).  A thread keeps 8 channels for all its pixels and
 * sums them in fp32 registers; the threads of a workgroup combine in LDS; the workgroup adds one value per channel with
 * an fp32 ATOMIC (global_atomic_add_f32).  The order of that sum, and with it the last bits of colsum, may differ
 * between two runs: colsum is NOT bit-reproducible.  dx does not depend on it.
 * Status: FI_ERR_INVALID_ARG for a null g / wt / gate / dx, N < 0, H, W, Cin, Cout, R, S or stride < 1, pad < 0;
 * FI_ERR_UNSUPPORTED for a call fi_train16_eligible answers 0, a wt not aligned to 16 bytes or a colsum not aligned to
 * 4 -- both before anything is launched.
 * ---------------------------------------------------------------------- */
int fi_train16_conv_dgrad_gated_bf16(const void *g, const void *wt, const void *dx_add, const void *gate, void *dx,
                                     float *colsum, int N, int H, int W, int Cin, int Cout, int R, int S, int stride,
                                     int pad, fi_stream_t stream);
int fi_train16_conv_dgrad_gated_f16(const void *g, const void *wt, const void *dx_add, const void *gate, void *dx,
                                    float *colsum, int N, int H, int W, int Cin, int Cout, int R, int S, int stride,
                                    int pad, fi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FI_TRAIN16_H_ */
