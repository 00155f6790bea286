/*
 * fi_act16.h -- C ABI of libfi_act16.so: convolutions that READ AND WRITE 16-bit channels-last activation tensors
 * (bf16 / IEEE half, [N, H, W, C] in memory), and the transposing casts at the boundary to the fp32 NCHW tensors of
 * the rest of the library, MI355X (gfx950).  A library of its own next to libfi_hip.so (include/fi_capi.h), which it
 * links against and whose conventions it follows: device pointers, a hipStream_t as void*, caller-allocated outputs, no
 * host synchronisation, FI_OK or a negative FI_ERR_* status with the message in libfi_hip's fi_last_error().
 * Every argument is checked on the host before any HIP call; N == 0 is FI_OK and launches nothing.
 */
#ifndef FI_ACT16_H_
#define FI_ACT16_H_

#include "fi_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------
 * 1 when fi_act16_conv_forward_{bf16,f16} takes this call, 0 otherwise.  HOST function, no GPU work; the four tensor
 * pointers are only inspected for alignment (NULL = not known yet, taken as aligned).  THE one statement of the rules:
 * Geometry: R == S == 1 with stride 1 or 2 and pad 0, or R == S == 3 with stride 1 and pad 1 (what Bottleneck uses).
 * Eligible: N, H, W >= 1, Cin % 32 == 0, Cout % 8 == 0, x / w / residual / y 16-byte aligned, and N*H*W, N*OH*OW,
 * Cout*R*S*Cin and the workgroup count all below 2^31.
 * ---------------------------------------------------------------------- */
int fi_act16_conv_eligible(int N, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad,
                           const void *x, const void *w, const void *residual, const void *y);

/* ------------------------------------------------------------------------
 * y = act(conv(x, w) * scale[co] + bias[co] + residual), one launch, 16-bit tensors in and out.
 * Replaces: conv + eval BatchNorm (+ shortcut) + ReLU of the ResNet trunk's Bottleneck, lib/sub_module.py:84-128, on
 *           tensors of half the bytes (the reference computes them in fp32 NCHW through cuDNN).
 * x [N, H, W, Cin], w [Cout, R, S, Cin] (tap-major), residual and y [N, OH, OW, Cout]: all 16-bit (bf16 / half by the
 * entry point's suffix), OH = (H + 2 pad - R) / stride + 1.  scale, bias [Cout] fp32, each optional (NULL): the folded
 * eval-mode BatchNorm.  residual optional (NULL).  relu != 0: max(., 0) last.
 * Arithmetic: the 16-bit products are exact in fp32 and accumulate in fp32 (v_mfma_f32_32x32x16_{bf16,f16}), taps in
 * row-major order, input channels ascending; acc * scale + bias + residual, then ReLU, in fp32 (each operation rounded
 * separately); ONE round-to-nearest-even to the 16-bit type at the store.  Every element is written once by one lane, no
 * atomics, no split over the reduction: an element's bits do not depend on where its tile sits in the grid or the batch.
 * Status: FI_ERR_INVALID_ARG for a null x / w / y, N < 0, H, W, Cin, Cout, R, S or stride < 1, pad < 0;
 * FI_ERR_UNSUPPORTED for a call fi_act16_conv_eligible answers 0 -- both before anything is launched.
 * ---------------------------------------------------------------------- */
int fi_act16_conv_forward_bf16(const void *x, const void *w, const float *scale, const float *bias,
                               const void *residual, void *y, int N, int H, int W, int Cin, int Cout,
                               int R, int S, int stride, int pad, int relu, fi_stream_t stream);
int fi_act16_conv_forward_f16(const void *x, const void *w, const float *scale, const float *bias,
                              const void *residual, void *y, int N, int H, int W, int Cin, int Cout,
                              int R, int S, int stride, int pad, int relu, fi_stream_t stream);

/* ------------------------------------------------------------------------
 * The transposing casts at the boundary, tiled through LDS.
 * pack:   y_nhwc [N, H, W, C] 16-bit = round-to-nearest-even(x_nchw [N, C, H, W] fp32)
 * unpack: y_nchw [N, C, H, W] fp32   = x_nhwc [N, H, W, C] 16-bit, widened exactly
 * Replaces: nothing of the reference (its tensors are fp32 NCHW throughout).
 * Status: FI_ERR_INVALID_ARG for a null pointer, N < 0, C, H or W < 1; FI_ERR_UNSUPPORTED for C % 8 != 0, a 16-bit
 * pointer that is not 16-byte aligned, an fp32 pointer that is not 4-byte aligned, N*H*W or the workgroup count of
 * 2^31 or more.
 * ---------------------------------------------------------------------- */
int fi_act16_pack_bf16(const float *x_nchw, void *y_nhwc, int N, int C, int H, int W, fi_stream_t stream);
int fi_act16_pack_f16(const float *x_nchw, void *y_nhwc, int N, int C, int H, int W, fi_stream_t stream);
int fi_act16_unpack_bf16(const void *x_nhwc, float *y_nchw, int N, int C, int H, int W, fi_stream_t stream);
int fi_act16_unpack_f16(const void *x_nhwc, float *y_nchw, int N, int C, int H, int W, fi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FI_ACT16_H_ */
