/*
 * fi_grad16.h -- C ABI of libfi_grad16.so: the BACKWARD operators of a convolution on 16-bit channels-last activation
 * tensors (bf16 / IEEE half, [N, H, W, C] in memory), MI355X (gfx950): the ReLU mask with the column sums, the data
 * gradient and the weight gradient of the layers fi_act16_conv_forward (include/fi_act16.h) runs.  A library of its own
 * next to libfi_hip.so (include/fi_capi.h), which it links against and whose conventions it follows: device pointers, a
 * hipStream_t as void*, caller-allocated outputs, no host synchronisation, FI_OK or a negative FI_ERR_* status with the
 * message in libfi_hip's fi_last_error().  Every argument is checked on the host before any HIP call; N == 0 is FI_OK
 * and launches nothing.
 *
 * Tensors (those of fi_act16_conv_forward): x [N, H, W, Cin], y / dy / g [N, OH, OW, Cout] with
 * OH = (H + 2 pad - R) / stride + 1, all 16-bit (bf16 / half by the entry point's suffix).
 */
#ifndef FI_GRAD16_H_
#define FI_GRAD16_H_

#include "fi_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FI_GRAD16_RELU_GRAD 0
#define FI_GRAD16_DGRAD 1
#define FI_GRAD16_WGRAD 2

/* ------------------------------------------------------------------------
 * 1 when the entry point of that kind takes the call, 0 otherwise.  HOST function, no GPU work; the pointers are only
 * inspected for alignment (NULL = not known yet, taken as aligned).  THE one statement of the rules.
 * kind                   p0   p1   p2       p3
 * FI_GRAD16_RELU_GRAD    dy   y    g        colsum (fp32)
 * FI_GRAD16_DGRAD        g    wt   dx_add   dx
 * FI_GRAD16_WGRAD        g    x    (unused) dw (fp32)
 * Geometry: R == S == 1 with stride 1 or 2 and pad 0, or R == S == 3 with stride 1 and pad 1 (what Bottleneck uses).
 * Eligible: kind one of the three, N, H, W >= 1, Cin % 32 == 0, Cout % 32 == 0 (both >= 32), every 16-bit tensor 16-byte
 * aligned and every fp32 tensor 4-byte aligned, and N*H*W, N*OH*OW, Cout*R*S*Cin and the workgroup count of the
 * launch all below 2^31.
 * ---------------------------------------------------------------------- */
int fi_grad16_eligible(int kind, int N, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad,
                       const void *p0, const void *p1, const void *p2, const void *p3);

/* ------------------------------------------------------------------------
 * g = relu ? dy * (y > 0) : dy on the N * OH * OW rows of Cout channels, and their column sums.
 * g: a 16-bit store that is exact (a select: dy where y > 0, else zero; y == 0, y == -0.0 and a NaN y select zero).
 * g may be dy itself.  y may be NULL when relu == 0.
 * colsum [Cout] fp32, optional (NULL): colsum[co] = sum over the rows of g -- the `s` of fi_bn_fold_grad.  It is
 * zero-filled by the call.  The rows of a workgroup are summed in fp32 in registers and LDS; the workgroups add their
 * part with fp32 ATOMICS (global_atomic_add_f32), so the order of the sum, and with it the last bits of colsum, may
 * differ between two runs.  g does not depend on it.
 * Status: FI_ERR_INVALID_ARG for a null dy / g (or y with relu != 0), N < 0, OH, OW or Cout < 1; FI_ERR_UNSUPPORTED for
 * what fi_grad16_eligible(FI_GRAD16_RELU_GRAD) refuses (Cout % 32, alignment, N*OH*OW >= 2^31).
 * ---------------------------------------------------------------------- */
int fi_grad16_relu_grad_bf16(const void *dy, const void *y, void *g, float *colsum, int N, int OH, int OW, int Cout,
                             int relu, fi_stream_t stream);
int fi_grad16_relu_grad_f16(const void *dy, const void *y, void *g, float *colsum, int N, int OH, int OW, int Cout,
                            int relu, fi_stream_t stream);

/* ------------------------------------------------------------------------
 * The data gradient, one launch:
 *     dx[n,h,w,ci] = sum_{r,s,co} g[n,oh,ow,co] * wt[ci,r',s',co] (+ dx_add[n,h,w,ci])
 * wt [Cin, R, S, Cout], 16-bit: the TRANSPOSED, TAP-FLIPPED weight, wt[ci,r',s',co] = W[co,ci,R-1-r',S-1-s'], which
 * the caller has already multiplied by the BatchNorm scale of co and rounded once.  dx and the optional dx_add
 * [N, H, W, Cin] are 16-bit.
 * Arithmetic: the 16-bit products are exact in fp32 and accumulate in fp32 (v_mfma_f32_32x32x16_{bf16,f16}); then the
 * add of dx_add in fp32; ONE round-to-nearest-even at the store.  Every element of dx is written exactly once by one
 * lane; no atomics, no split of the reduction: the bits do not depend on the tile's place in the grid or the batch, and
 * two runs agree bit for bit.
 * Stride 1 is the forward's own reduction with the two channel counts swapped and runs through the forward's main loop
 * (taps in row-major order of r', s'; co ascending).  Stride 2 (1x1 only): the product lands on the pixels (2 oh, 2 ow);
 * the SAME launch writes zero (+ dx_add) to every other pixel of dx -- no memset.
 * Status: FI_ERR_INVALID_ARG for a null g / wt / dx, N < 0, H, W, Cin, Cout, R, S or stride < 1, pad < 0;
 * FI_ERR_UNSUPPORTED for a call fi_grad16_eligible(FI_GRAD16_DGRAD) answers 0 -- both before anything is launched.
 * ---------------------------------------------------------------------- */
int fi_grad16_conv_dgrad_bf16(const void *g, const void *wt, const void *dx_add, void *dx, int N, int H, int W, int Cin,
                              int Cout, int R, int S, int stride, int pad, fi_stream_t stream);
int fi_grad16_conv_dgrad_f16(const void *g, const void *wt, const void *dx_add, void *dx, int N, int H, int W, int Cin,
                             int Cout, int R, int S, int stride, int pad, fi_stream_t stream);

/* ------------------------------------------------------------------------
 * The weight gradient:
 *     dw[co,r,s,ci] = sum_{n,oh,ow} g[n,oh,ow,co] * x[n, oh*stride - pad + r, ow*stride - pad + s, ci]
 * dw [Cout, R, S, Cin] fp32, TAP-MAJOR: the dw_tap_major operand of fi_bn_fold_grad.  A tap outside the map contributes
 * zero and no address outside x is formed.  The call zero-fills or fully overwrites dw itself.
 * Arithmetic: exact 16-bit products, fp32 accumulation over the pixels in ascending order inside a workgroup
 * (v_mfma_f32_32x32x16_{bf16,f16}; both operands are transposed LDS reads, ds_read_b64_tr_b16).
 * The pixel range is split over workgroups when the channel tiles and taps alone would not fill the machine.  With ONE
 * part, dw is stored plainly and two runs agree bit for bit.  With several, dw is zero-filled (hipMemsetAsync on the
 * stream) and the parts are combined with fp32 ATOMICS (global_atomic_add_f32), as fi_conv2d_weight_grad does: two
 * runs then agree to within the bound of an fp32 sum in any order, NOT bit for bit.
 * Status: FI_ERR_INVALID_ARG for a null g / x / dw, N < 0, H, W, Cin, Cout, R, S or stride < 1, pad < 0;
 * FI_ERR_UNSUPPORTED for a call fi_grad16_eligible(FI_GRAD16_WGRAD) answers 0 -- both before anything is launched.
 * ---------------------------------------------------------------------- */
int fi_grad16_conv_wgrad_bf16(const void *g, const void *x, float *dw, int N, int H, int W, int Cin, int Cout, int R,
                              int S, int stride, int pad, fi_stream_t stream);
int fi_grad16_conv_wgrad_f16(const void *g, const void *x, float *dw, int N, int H, int W, int Cin, int Cout, int R,
                             int S, int stride, int pad, fi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FI_GRAD16_H_ */
