/*
 * fi_pyr16.h -- C ABI of libfi_pyr16.so: the two layers that carry 16-bit channels-last activation tensors (bf16 / IEEE
 * half, [N, H, W, C] in memory) from the ResNet trunk through the feature pyramid to the RPN's outputs, MI355X (gfx950):
 * the lateral 1x1 convolution that adds the top-down map read at HALF resolution, and the stacked 1x1 RPN heads that read
 * a 16-bit map and write fp32 in the anchors' order.  Both run the main loop of fi_act16_conv_forward (include/fi_act16.h,
 * csrc/conv_act16_dev.h); only their epilogues are their own.  A library of its own next to libfi_hip.so
 * (include/fi_capi.h), which it links against and whose conventions it follows: device pointers, a hipStream_t as void*,
 * caller-allocated outputs, no host synchronisation, FI_OK or a negative FI_ERR_* status with the message in libfi_hip's
 * fi_last_error().  Every argument is checked on the host before any HIP call; N == 0 is FI_OK and launches nothing.
 */
#ifndef FI_PYR16_H_
#define FI_PYR16_H_

#include "fi_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------
 * 1 when fi_pyr16_lateral_{bf16,f16} takes this call, 0 otherwise.  HOST function, no GPU work; the four tensor
 * pointers are only inspected for alignment (NULL = not known yet, taken as aligned).  THE one statement of the rules:
 * N >= 1, H and W even and >= 2, Cin % 32 == 0 (and >= 32), Cout % 8 == 0 (and >= 8), x / w / top / y 16-byte aligned,
 * and N*H*W, Cout*Cin and the workgroup count all below 2^31.
 * ---------------------------------------------------------------------- */
int fi_pyr16_lateral_eligible(int N, int H, int W, int Cin, int Cout, const void *x, const void *w, const void *top,
                              const void *y);

/* ------------------------------------------------------------------------
 * y[n, oh, ow, :] = round16((conv1x1(x, w)[n, oh, ow, :] + bias) + float(top[n, oh >> 1, ow >> 1, :])), one launch.
 * Replaces: the FPN's top-down step, lateral 1x1 convolution + 2x nearest upsampling of the coarser level + add
 *           (lib/model.py's FPN.forward), without the upsampled map ever being written.
 * x [N, H, W, Cin], w [Cout, Cin], top [N, H/2, W/2, Cout], y [N, H, W, Cout]: all 16-bit (bf16 / half by the entry
 * point's suffix).  bias [Cout] fp32, optional (NULL).  top is required.  No activation.
 * Arithmetic: the 16-bit products are exact in fp32 and accumulate in fp32 (v_mfma_f32_32x32x16_{bf16,f16}), input
 * channels ascending; acc + bias, then + top, in fp32 (each operation rounded separately); ONE round-to-nearest-even to
 * the 16-bit type at the store.  The address of top is formed from the pixel's own (image, oh, ow).  Every element is
 * written once by one lane, no atomics, no split over the reduction: an element's bits do not depend on where its tile
 * sits in the grid or the batch.
 * Status: FI_ERR_INVALID_ARG for a null x / w / top / y, N < 0, H, W, Cin or Cout < 1; FI_ERR_UNSUPPORTED for a call
 * fi_pyr16_lateral_eligible answers 0 -- both before anything is launched.
 * ---------------------------------------------------------------------- */
int fi_pyr16_lateral_bf16(const void *x, const void *w, const float *bias, const void *top, void *y, int N, int H, int W,
                          int Cin, int Cout, fi_stream_t stream);
int fi_pyr16_lateral_f16(const void *x, const void *w, const float *bias, const void *top, void *y, int N, int H, int W,
                         int Cin, int Cout, fi_stream_t stream);

/* ------------------------------------------------------------------------
 * 1 when fi_pyr16_head1x1_{bf16,f16} takes this call, 0 otherwise.  HOST function; pointers as above.  The rules:
 * N, H, W >= 1, 1 <= Cout <= 64, Cin % 32 == 0 (and >= 32), x and w 16-byte aligned, y 4-byte aligned, and N*H*W,
 * Cout*Cin and the workgroup count all below 2^31.
 * ---------------------------------------------------------------------- */
int fi_pyr16_head1x1_eligible(int N, int H, int W, int Cin, int Cout, const void *x, const void *w, const void *y);

/* ------------------------------------------------------------------------
 * y[n, oh, ow, :] = conv1x1(x, w)[n, oh, ow, :] + bias in fp32, stored unrounded, one launch.
 * Replaces: the RPN's class and box 1x1 convolutions over their stacked filters (lib/sub_module.py, RPN.forward) and the
 *           permute(0, 2, 3, 1).contiguous() copy behind them: y is already in the anchors' order.
 * x [N, H, W, Cin] and w [Cout, Cin] 16-bit; bias [Cout] fp32, optional (NULL); y [N, H, W, Cout] FP32 channels-last.
 * Cout need not be a multiple of anything: one 64-row channel tile holds every output channel (rows past Cout are
 * zeros), the y bytes of a pixel tile are one contiguous run and are stored as such, 4 bytes per lane, neighbouring lanes
 * on neighbouring floats.  Accumulation as above; acc + bias is one fp32 addition.  Every element is written once.
 * Status: FI_ERR_INVALID_ARG for a null x / w / y, N < 0, H, W, Cin or Cout < 1; FI_ERR_UNSUPPORTED for a call
 * fi_pyr16_head1x1_eligible answers 0 -- both before anything is launched.
 * ---------------------------------------------------------------------- */
int fi_pyr16_head1x1_bf16(const void *x, const void *w, const float *bias, float *y, int N, int H, int W, int Cin, int Cout,
                          fi_stream_t stream);
int fi_pyr16_head1x1_f16(const void *x, const void *w, const float *bias, float *y, int N, int H, int W, int Cin, int Cout,
                         fi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FI_PYR16_H_ */
