/*
 * fi_convt.h -- C ABI of libfi_convt.so: the transposed 3x3 / stride 2 convolution of the 2x make-up layer and of the
 * 2-D OptTrans generator, MI355X (gfx950).  A library of its own next to libfi_hip.so (include/fi_capi.h), which it
 * links against and whose conventions it follows: device pointers, a hipStream_t as void*, caller-allocated outputs, no
 * host synchronisation, FI_OK or a negative FI_ERR_* status with the message in libfi_hip's fi_last_error().
 */
#ifndef FI_CONVT_H_
#define FI_CONVT_H_

#include "fi_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------
 * 1 when fi_conv_transpose3x3s2_forward takes this call, 0 otherwise.  HOST function, no GPU work; x and y are only
 * inspected for alignment (NULL = not known yet, taken as aligned).
 * Replaces: nothing of the reference (cuDNN chose its own algorithm behind nn.ConvTranspose2d, lib/sub_module.py:312-314);
 *           it is the routing question of conv.ConvTranspose3x3.
 * Eligible: N >= 1, Cin % 16 == 0, Cout >= 1, H >= 1, W >= 1, H * W <= 2^26, at most 2^31 - 1 workgroups of 4 x 16 input
 * pixels x 128 output channels, x 4-byte and y 16-byte aligned, and Cout % 4 == 0 for a channels-last output.
 * ---------------------------------------------------------------------- */
int fi_conv_transpose3x3s2_eligible(int N, int Cin, int H, int W, int Cout, int out_nhwc, const float *x, const float *y);

/* ------------------------------------------------------------------------
 * y = act(conv_transpose2d(x, weight, stride 2, padding 1, output_padding 1) * scale[co] + bias[co]), one launch.
 * Replaces: nn.ConvTranspose2d(256, 256, kernel_size=3, stride=2, padding=1, output_padding=1) + BatchNorm2d + ReLU
 *           lib/sub_module.py:312-314 (the make-up layer at DEV.UPSAMPLE_FAC = 2, lib/config.py:205; applied at :549-557)
 *           and the stride-2 generator p2_ot .. p4_ot of OptTrans  lib/OT_module.py:24-36.
 * x [N, Cin, H, W]; weight [Cin, Cout, 3, 3] (torch's ConvTranspose2d layout, read as it is stored);
 * y [N, Cout, 2H, 2W], or [N, 2H, 2W, Cout] with out_nhwc = 1 (channels-last).
 * scale, bias [Cout], each optional (NULL): an eval-mode BatchNorm folded by the caller (scale = gamma / sqrt(var + eps),
 * bias = beta + (conv_bias - mean) * scale), or the plain convolution bias with scale NULL.  relu != 0: max(., 0) last.
 * Arithmetic: exact fp32 (v_mfma_f32_32x32x2_f32, an fp32 fma chain); every output element is the sum over the input
 * channels, in one fixed order, of the 1, 2, 2 or 4 taps that reach its parity class -- no zero-stuffed product, no
 * atomics, every element written exactly once: the bits of an element do not depend on the batch or the grid.
 * Status: FI_ERR_INVALID_ARG for a null x / weight / y, N < 0, Cin, Cout, H or W < 1; FI_ERR_UNSUPPORTED for a call
 * fi_conv_transpose3x3s2_eligible answers 0 (Cin % 16 != 0, a misaligned y, ...) -- both before anything is launched.
 * N == 0 is FI_OK and launches nothing.
 * ---------------------------------------------------------------------- */
int fi_conv_transpose3x3s2_forward(const float *x, const float *weight, const float *bias, const float *scale, float *y,
                                   int N, int Cin, int H, int W, int Cout, int relu, int out_nhwc, fi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FI_CONVT_H_ */
