// conv_act16.hip -- libfi_act16.so (include/fi_act16.h): implicit-GEMM convolution on 16-bit channels-last tensors
// (v_mfma_f32_32x32x16_bf16, fp32 accumulation) and the transposing casts at the boundary to fp32 NCHW.
// conv_act16_f16.hip includes this file with FI_E16_HALF defined: the same kernels on IEEE half under the *_f16 names.
//
// Orientation, LDS layout, pipeline and the main loop itself: conv_act16_dev.h, which conv_pyr16.hip (libfi_pyr16.so) shares.
// Epilogue.  C/D map col = lane & 31 (pixel), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (channel): a register quad
// is 4 consecutive channels of one pixel.  Stored straight from that map a wave's instruction touches 32 pixels with 16
// bytes each (a stride of Cout * 2 bytes): the layers with Cin = 64 have ONE K block and are all epilogue, and ran at
// 1.4 TB/s that way.  So the fp32 tile goes through LDS once more and leaves as 16-byte stores, 16 neighbouring lanes per
// 256 contiguous bytes of a pixel; the shortcut is read the same way.
#include <stdint.h>

#include "fi_common.h"
#include "conv_act16_dev.h"
#include "../../include/fi_act16.h"

namespace {

// BM: channel tile (128, or 64 for the narrow layers), BK: K block (64, or 32 when Cin % 64 != 0)
template <int BM, int BK>
__global__ __launch_bounds__(kThreads) void act16_conv_kernel(const E16 *__restrict__ x, const E16 *__restrict__ w,
                                                              const float *__restrict__ scale,
                                                              const float *__restrict__ bias,
                                                              const E16 *__restrict__ residual, E16 *__restrict__ y,
                                                              Geom g)
{
    __shared__ u32x4 smem[tile_smem_chunks<BM, BK>()];
    f32x4 *Cs = reinterpret_cast<f32x4 *>(smem);
    const int tid = threadIdx.x;
    const int m0 = (int)(blockIdx.x % (unsigned)g.mtiles) * BM;
    const int n0 = (int)(blockIdx.x / (unsigned)g.mtiles) * BN;          // < P < 2^31 (host check)
    f32x16 acc[BM / 64][2];
    conv_main_loop<BM, BK>(x, w, g, smem, m0, n0, acc);

    // epilogue.  The fp32 tile through LDS (tile_to_lds), then acc * scale + bias + residual, ReLU in fp32 and ONE rounding,
    // 8 channels of one pixel per lane and store.
    constexpr int RC = BM / 4;                     // 16-byte chunks per tile row
    tile_to_lds<BM>(acc, Cs);
    constexpr int CH8 = BM / 8;                    // 8-channel groups per tile row; kThreads % CH8 == 0: a thread keeps its group
    const int cg = tid % CH8;
    const int co = m0 + cg * 8;
    if (co >= g.Cout) return;                      // Cout % 8 == 0: a group is whole or absent
    float sc[8], bi[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        sc[j] = scale ? scale[co + j] : 1.f;
        bi[j] = bias ? bias[co + j] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < BN * CH8 / kThreads; ++i) {
        const int pr = (tid + i * kThreads) / CH8;
        const long p = (long)n0 + pr;
        if (p >= g.P) break;                       // pr grows with i
        const long o = p * g.Cout + co;
        const f32x4 lo = Cs[pr * RC + ((2 * cg) ^ (pr & 15))], hi = Cs[pr * RC + ((2 * cg + 1) ^ (pr & 15))];
        float v[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = lo[j];
            v[4 + j] = hi[j];
        }
        if (scale) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = v[j] * sc[j];
        }
        if (bias) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = v[j] + bi[j];
        }
        if (residual) {
            const e16x8 rr = *reinterpret_cast<const e16x8 *>(residual + o);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = v[j] + (float)rr[j];
        }
        e16x8 out;
#pragma unroll
        for (int j = 0; j < 8; ++j) out[j] = (E16)((g.relu && !(v[j] > 0.f) && v[j] == v[j]) ? 0.f : v[j]);
        *reinterpret_cast<e16x8 *>(y + o) = out;
    }
}

// ---- the casts: a 32-channel x 64-pixel tile of one image through LDS ---------------------------------------------
constexpr int CT = 32, PT = 64;

struct CastGeom {
    int C, HW;
    int ctiles, ptiles;
};

__global__ __launch_bounds__(kThreads) void act16_pack_kernel(const float *__restrict__ x, E16 *__restrict__ y, CastGeom g)
{
    __shared__ float tile[CT][PT + 1];
    const int tid = threadIdx.x;
    unsigned b = blockIdx.x;
    const int pt = (int)(b % (unsigned)g.ptiles);
    b /= (unsigned)g.ptiles;
    const int ct = (int)(b % (unsigned)g.ctiles);
    const long n = b / (unsigned)g.ctiles;
    const int c0 = ct * CT, p0 = pt * PT;
    {   // read: neighbouring lanes take neighbouring pixels of one channel
        const int p = tid % PT;
#pragma unroll
        for (int i = 0; i < CT * PT / kThreads; ++i) {
            const int c = tid / PT + i * (kThreads / PT);
            if (c0 + c < g.C && p0 + p < g.HW) tile[c][p] = x[(n * g.C + c0 + c) * g.HW + p0 + p];
        }
    }
    __syncthreads();
    {   // write: 8 channels of one pixel, 16 bytes (C % 8 == 0: a chunk is whole or absent)
        const int p = tid / (CT / 8), q = tid % (CT / 8);
        if (p0 + p < g.HW && c0 + q * 8 < g.C) {
            e16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (E16)tile[q * 8 + j][p];
            *reinterpret_cast<e16x8 *>(y + (n * g.HW + p0 + p) * g.C + c0 + q * 8) = o;
        }
    }
}

__global__ __launch_bounds__(kThreads) void act16_unpack_kernel(const E16 *__restrict__ x, float *__restrict__ y, CastGeom g)
{
    __shared__ float tile[CT][PT + 1];
    const int tid = threadIdx.x;
    unsigned b = blockIdx.x;
    const int pt = (int)(b % (unsigned)g.ptiles);
    b /= (unsigned)g.ptiles;
    const int ct = (int)(b % (unsigned)g.ctiles);
    const long n = b / (unsigned)g.ctiles;
    const int c0 = ct * CT, p0 = pt * PT;
    {
        const int p = tid / (CT / 8), q = tid % (CT / 8);
        if (p0 + p < g.HW && c0 + q * 8 < g.C) {
            const e16x8 v = *reinterpret_cast<const e16x8 *>(x + (n * g.HW + p0 + p) * g.C + c0 + q * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) tile[q * 8 + j][p] = (float)v[j];
        }
    }
    __syncthreads();
    {
        const int p = tid % PT;
#pragma unroll
        for (int i = 0; i < CT * PT / kThreads; ++i) {
            const int c = tid / PT + i * (kThreads / PT);
            if (c0 + c < g.C && p0 + p < g.HW) y[(n * g.C + c0 + c) * g.HW + p0 + p] = tile[c][p];
        }
    }
}

// THE statement of what the convolution takes (the pointers may be NULL: not known yet)
bool conv_eligible(int N, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, const void *x, const void *w,
                   const void *residual, const void *y)
{
    if (N < 1 || H < 1 || W < 1 || Cin < 32 || Cin % 32 != 0 || Cout < 8 || Cout % 8 != 0) return false;
    const bool g1 = R == 1 && S == 1 && (stride == 1 || stride == 2) && pad == 0;
    const bool g3 = R == 3 && S == 3 && stride == 1 && pad == 1;
    if (!g1 && !g3) return false;
    if ((((uintptr_t)x | (uintptr_t)w | (uintptr_t)residual | (uintptr_t)y) & 15) != 0) return false;
    const long OH = (H + 2 * pad - R) / stride + 1, OW = (W + 2 * pad - S) / stride + 1;
    const long P = (long)N * OH * OW;
    if ((long)N * H * W > kIntMax || P > kIntMax || (long)Cout * R * S * Cin > kIntMax) return false;
    const long blocks = ((P + BN - 1) / BN) * fi::ceil_div(Cout, conv_bm(Cout, P));
    return blocks <= kIntMax;
}

bool cast_eligible(int N, int C, int H, int W, const void *p16, const void *p32)
{
    if (C % 8 != 0 || ((uintptr_t)p16 & 15) != 0 || ((uintptr_t)p32 & 3) != 0) return false;
    if ((long)N * H * W > kIntMax) return false;
    const long blocks = (long)N * fi::ceil_div(C, CT) * (((long)H * W + PT - 1) / PT);
    return blocks <= kIntMax;
}

template <bool kPack>
int launch_cast(const void *src, void *dst, int N, int C, int H, int W, fi_stream_t stream, const char *name)
{
    FI_REQUIRE(N >= 0 && C >= 1 && H >= 1 && W >= 1, "N >= 0, C, H, W >= 1");
    if (N == 0) return FI_OK;
    FI_REQUIRE(src && dst, "null pointer");
    if (!cast_eligible(N, C, H, W, kPack ? dst : src, kPack ? src : dst)) {
        fi::set_error("%s: unsupported call (N %d, C %d, H %d, W %d, src %p, dst %p): needs C %% 8 == 0, the 16-bit tensor "
                      "aligned to 16 bytes, N * H * W < 2^31", name, N, C, H, W, src, dst);
        return FI_ERR_UNSUPPORTED;
    }
    CastGeom g;
    g.C = C;
    g.HW = H * W;
    g.ctiles = fi::ceil_div(C, CT);
    g.ptiles = fi::ceil_div(g.HW, PT);
    const unsigned blocks = (unsigned)((long)N * g.ctiles * g.ptiles);
    hipStream_t st = (hipStream_t)stream;
    if (kPack)
        hipLaunchKernelGGL(act16_pack_kernel, dim3(blocks), dim3(kThreads), 0, st, (const float *)src, (E16 *)dst, g);
    else
        hipLaunchKernelGGL(act16_unpack_kernel, dim3(blocks), dim3(kThreads), 0, st, (const E16 *)src, (float *)dst, g);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

}  // namespace

extern "C" {

#ifndef FI_E16_HALF
int fi_act16_conv_eligible(int N, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, const void *x,
                           const void *w, const void *residual, const void *y)
{
    return conv_eligible(N, H, W, Cin, Cout, R, S, stride, pad, x, w, residual, y) ? 1 : 0;
}
#endif

int FI16(fi_act16_conv_forward)(const void *x, const void *w, const float *scale, const float *bias, const void *residual,
                                void *y, int N, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad,
                                int relu, fi_stream_t stream)
{
    FI_REQUIRE(N >= 0 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1, "N >= 0, H, W, Cin, Cout >= 1");
    FI_REQUIRE(R >= 1 && S >= 1 && stride >= 1 && pad >= 0, "R, S, stride >= 1, pad >= 0");
    if (N == 0) return FI_OK;
    FI_REQUIRE(x && w && y, "null pointer");
    if (!conv_eligible(N, H, W, Cin, Cout, R, S, stride, pad, x, w, residual, y)) {
        fi::set_error("fi_act16_conv_forward: unsupported call (N %d, H %d, W %d, Cin %d, Cout %d, R %d, S %d, stride %d, "
                      "pad %d, x %p, w %p, residual %p, y %p): needs 1x1 / stride 1 or 2 / pad 0 or 3x3 / stride 1 / pad 1, "
                      "Cin %% 32 == 0, Cout %% 8 == 0, tensors aligned to 16 bytes, extents below 2^31",
                      N, H, W, Cin, Cout, R, S, stride, pad, x, w, residual, (const void *)y);
        return FI_ERR_UNSUPPORTED;
    }
    Geom g;
    g.N = N; g.H = H; g.W = W; g.Cin = Cin; g.Cout = Cout; g.RS = R * S; g.S = S; g.stride = stride; g.pad = pad;
    g.OH = (H + 2 * pad - R) / stride + 1;
    g.OW = (W + 2 * pad - S) / stride + 1;
    g.P = N * g.OH * g.OW;
    const int bm = conv_bm(Cout, g.P);
    g.mtiles = fi::ceil_div(Cout, bm);
    g.relu = relu ? 1 : 0;
    const unsigned blocks = (unsigned)((long)fi::ceil_div(g.P, BN) * g.mtiles);
    hipStream_t st = (hipStream_t)stream;
    const E16 *xe = (const E16 *)x, *we = (const E16 *)w, *re = (const E16 *)residual;
    E16 *ye = (E16 *)y;
#define FI_ACT16_LAUNCH(BM_, BK_) \
    hipLaunchKernelGGL((act16_conv_kernel<BM_, BK_>), dim3(blocks), dim3(kThreads), 0, st, xe, we, scale, bias, re, ye, g)
    if (bm == 64) {
        if (Cin % 64 == 0) FI_ACT16_LAUNCH(64, 64); else FI_ACT16_LAUNCH(64, 32);
    } else {
        if (Cin % 64 == 0) FI_ACT16_LAUNCH(128, 64); else FI_ACT16_LAUNCH(128, 32);
    }
#undef FI_ACT16_LAUNCH
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int FI16(fi_act16_pack)(const float *x_nchw, void *y_nhwc, int N, int C, int H, int W, fi_stream_t stream)
{
    return launch_cast<true>(x_nchw, y_nhwc, N, C, H, W, stream, "fi_act16_pack");
}

int FI16(fi_act16_unpack)(const void *x_nhwc, float *y_nchw, int N, int C, int H, int W, fi_stream_t stream)
{
    return launch_cast<false>(x_nhwc, y_nchw, N, C, H, W, stream, "fi_act16_unpack");
}

}  // extern "C"
