// conv_pyr16.hip -- libfi_pyr16.so (include/fi_pyr16.h): the feature pyramid's lateral step and the RPN's stacked 1x1 heads
// on 16-bit channels-last tensors.  conv_pyr16_f16.hip includes this file with FI_E16_HALF defined: the same kernels on
// IEEE half under the *_f16 names.
//
// Both kernels are 1x1 / stride 1 convolutions on the main loop of conv_act16_dev.h (tiles, swizzled LDS, summation order:
// see there) and hand the fp32 tile to LDS the same way; what is theirs is the epilogue.
// Lateral.  As fi_act16_conv_forward's: a lane takes 8 channels of one pixel, 16 neighbouring lanes cover 256 contiguous
// bytes of y.  The map it adds is the COARSER level's, [N, H/2, W/2, Cout], read at (oh >> 1, ow >> 1): the nearest-neighbour
// 2x upsampling is an index, not a tensor.  A pixel tile may span images and rows, so the lane derives (image, oh, ow) from
// its own flattened pixel.  The four pixels of a 2 x 2 block read the same 16 bytes of top; two of them sit next to each
// other in the tile and the other two a row further: the repeats are served by the cache, HBM sees top once.
// Heads.  Cout = 6 x anchors (18) is no multiple of 8 and the consumer wants fp32 [N, H*W, Cout].  One 64-row channel tile
// holds every output channel (the loop forms zero rows past Cout), so the y bytes of a pixel tile are ONE contiguous run
// of pixels x Cout floats starting at n0 * Cout: the epilogue walks that run flat, element e = (pixel e / Cout, channel
// e % Cout), a wavefront's store instruction covering 256 contiguous bytes whatever Cout is.
#include <stdint.h>

#include "fi_common.h"
#include "conv_act16_dev.h"
#include "../../include/fi_pyr16.h"

namespace {

template <int BM, int BK>
__global__ __launch_bounds__(kThreads) void pyr16_lateral_kernel(const E16 *__restrict__ x, const E16 *__restrict__ w,
                                                                 const float *__restrict__ bias,
                                                                 const E16 *__restrict__ top, E16 *__restrict__ y, Geom g)
{
    __shared__ u32x4 smem[tile_smem_chunks<BM, BK>()];
    f32x4 *Cs = reinterpret_cast<f32x4 *>(smem);
    const int tid = threadIdx.x;
    const int m0 = (int)(blockIdx.x % (unsigned)g.mtiles) * BM;
    const int n0 = (int)(blockIdx.x / (unsigned)g.mtiles) * BN;          // < P < 2^31 (host check)
    f32x16 acc[BM / 64][2];
    conv_main_loop<BM, BK>(x, w, g, smem, m0, n0, acc);

    constexpr int RC = BM / 4;                     // 16-byte chunks per tile row
    tile_to_lds<BM>(acc, Cs);
    constexpr int CH8 = BM / 8;                    // 8-channel groups per tile row; kThreads % CH8 == 0: a thread keeps its group
    const int cg = tid % CH8;
    const int co = m0 + cg * 8;
    if (co >= g.Cout) return;                      // Cout % 8 == 0: a group is whole or absent
    float bi[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) bi[j] = bias ? bias[co + j] : 0.f;
    const int HW = g.H * g.W, H2 = g.H >> 1, W2 = g.W >> 1;            // H, W even (host check)
#pragma unroll
    for (int i = 0; i < BN * CH8 / kThreads; ++i) {
        const int pr = (tid + i * kThreads) / CH8;
        const long p = (long)n0 + pr;
        if (p >= g.P) break;                       // pr grows with i
        const int img = (int)(p / HW);
        const int rem = (int)(p - (long)img * HW);
        const int oh = rem / g.W, ow = rem - oh * g.W;
        const long t = (((long)img * H2 + (oh >> 1)) * W2 + (ow >> 1)) * g.Cout + co;
        const long o = p * g.Cout + co;
        const f32x4 lo = Cs[pr * RC + ((2 * cg) ^ (pr & 15))], hi = Cs[pr * RC + ((2 * cg + 1) ^ (pr & 15))];
        const e16x8 tt = *reinterpret_cast<const e16x8 *>(top + t);
        float v[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = lo[j];
            v[4 + j] = hi[j];
        }
        if (bias) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = v[j] + bi[j];
        }
        e16x8 out;
#pragma unroll
        for (int j = 0; j < 8; ++j) out[j] = (E16)(v[j] + (float)tt[j]);
        *reinterpret_cast<e16x8 *>(y + o) = out;
    }
}

constexpr int HBM = 64;           // the heads' channel tile: every output channel in one

template <int BK>
__global__ __launch_bounds__(kThreads) void pyr16_head_kernel(const E16 *__restrict__ x, const E16 *__restrict__ w,
                                                              const float *__restrict__ bias, float *__restrict__ y, Geom g)
{
    __shared__ u32x4 smem[tile_smem_chunks<HBM, BK>()];
    const int tid = threadIdx.x;
    const int n0 = (int)blockIdx.x * BN;           // < P < 2^31 (host check); mtiles == 1
    f32x16 acc[1][2];
    conv_main_loop<HBM, BK>(x, w, g, smem, 0, n0, acc);

    constexpr int RC = HBM / 4;
    tile_to_lds<HBM>(acc, reinterpret_cast<f32x4 *>(smem));
    const float *Cf = reinterpret_cast<const float *>(smem);
    const long left = (long)g.P - n0;
    const int total = (int)(left < BN ? left : BN) * g.Cout;           // floats of this tile's run, <= 128 * 64
    float *run = y + (long)n0 * g.Cout;
    for (int e = tid; e < total; e += kThreads) {
        const int pr = e / g.Cout, c = e - pr * g.Cout;
        float v = Cf[(pr * RC + ((c >> 2) ^ (pr & 15))) * 4 + (c & 3)];
        if (bias) v = v + bias[c];
        run[e] = v;
    }
}

bool sizes_ok(long pixels, long weights, long blocks)
{
    return pixels <= kIntMax && weights <= kIntMax && blocks <= kIntMax;
}

// THE statement of what the lateral takes (the pointers may be NULL: not known yet)
bool lateral_eligible(int N, int H, int W, int Cin, int Cout, const void *x, const void *w, const void *top, const void *y)
{
    if (N < 1 || H < 2 || W < 2 || H % 2 != 0 || W % 2 != 0) return false;
    if (Cin < 32 || Cin % 32 != 0 || Cout < 8 || Cout % 8 != 0) return false;
    if ((((uintptr_t)x | (uintptr_t)w | (uintptr_t)top | (uintptr_t)y) & 15) != 0) return false;
    const long P = (long)N * H * W;
    if (P > kIntMax) return false;
    return sizes_ok(P, (long)Cout * Cin, ((P + BN - 1) / BN) * fi::ceil_div(Cout, conv_bm(Cout, P)));
}

// ... and the heads
bool head_eligible(int N, int H, int W, int Cin, int Cout, const void *x, const void *w, const void *y)
{
    if (N < 1 || H < 1 || W < 1 || Cin < 32 || Cin % 32 != 0 || Cout < 1 || Cout > HBM) return false;
    if ((((uintptr_t)x | (uintptr_t)w) & 15) != 0 || ((uintptr_t)y & 3) != 0) return false;
    const long P = (long)N * H * W;
    return sizes_ok(P, (long)Cout * Cin, (P + BN - 1) / BN);
}

Geom geom_1x1(int N, int H, int W, int Cin, int Cout, int mtiles)
{
    Geom g;
    g.N = N; g.H = H; g.W = W; g.Cin = Cin; g.Cout = Cout; g.RS = 1; g.S = 1; g.stride = 1; g.pad = 0;
    g.OH = H;
    g.OW = W;
    g.P = N * H * W;
    g.mtiles = mtiles;
    g.relu = 0;
    return g;
}

}  // namespace

extern "C" {

#ifndef FI_E16_HALF
int fi_pyr16_lateral_eligible(int N, int H, int W, int Cin, int Cout, const void *x, const void *w, const void *top,
                              const void *y)
{
    return lateral_eligible(N, H, W, Cin, Cout, x, w, top, y) ? 1 : 0;
}

int fi_pyr16_head1x1_eligible(int N, int H, int W, int Cin, int Cout, const void *x, const void *w, const void *y)
{
    return head_eligible(N, H, W, Cin, Cout, x, w, y) ? 1 : 0;
}
#endif

int FI16(fi_pyr16_lateral)(const void *x, const void *w, const float *bias, const void *top, void *y, int N, int H, int W,
                           int Cin, int Cout, fi_stream_t stream)
{
    FI_REQUIRE(N >= 0 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1, "N >= 0, H, W, Cin, Cout >= 1");
    if (N == 0) return FI_OK;
    FI_REQUIRE(x && w && top && y, "null pointer");
    if (!lateral_eligible(N, H, W, Cin, Cout, x, w, top, y)) {
        fi::set_error("fi_pyr16_lateral: unsupported call (N %d, H %d, W %d, Cin %d, Cout %d, x %p, w %p, top %p, y %p): "
                      "needs H and W even, Cin %% 32 == 0, Cout %% 8 == 0, tensors aligned to 16 bytes, extents below 2^31",
                      N, H, W, Cin, Cout, x, w, top, (const void *)y);
        return FI_ERR_UNSUPPORTED;
    }
    const int bm = conv_bm(Cout, (long)N * H * W);
    const Geom g = geom_1x1(N, H, W, Cin, Cout, fi::ceil_div(Cout, bm));
    const unsigned blocks = (unsigned)((long)fi::ceil_div(g.P, BN) * g.mtiles);
    hipStream_t st = (hipStream_t)stream;
    const E16 *xe = (const E16 *)x, *we = (const E16 *)w, *te = (const E16 *)top;
    E16 *ye = (E16 *)y;
#define FI_PYR16_LAUNCH(BM_, BK_) \
    hipLaunchKernelGGL((pyr16_lateral_kernel<BM_, BK_>), dim3(blocks), dim3(kThreads), 0, st, xe, we, bias, te, ye, g)
    if (bm == 64) {
        if (Cin % 64 == 0) FI_PYR16_LAUNCH(64, 64); else FI_PYR16_LAUNCH(64, 32);
    } else {
        if (Cin % 64 == 0) FI_PYR16_LAUNCH(128, 64); else FI_PYR16_LAUNCH(128, 32);
    }
#undef FI_PYR16_LAUNCH
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int FI16(fi_pyr16_head1x1)(const void *x, const void *w, const float *bias, float *y, int N, int H, int W, int Cin,
                           int Cout, fi_stream_t stream)
{
    FI_REQUIRE(N >= 0 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1, "N >= 0, H, W, Cin, Cout >= 1");
    if (N == 0) return FI_OK;
    FI_REQUIRE(x && w && y, "null pointer");
    if (!head_eligible(N, H, W, Cin, Cout, x, w, y)) {
        fi::set_error("fi_pyr16_head1x1: unsupported call (N %d, H %d, W %d, Cin %d, Cout %d, x %p, w %p, y %p): needs "
                      "Cout <= 64, Cin %% 32 == 0, x and w aligned to 16 bytes, y to 4, extents below 2^31",
                      N, H, W, Cin, Cout, x, w, (const void *)y);
        return FI_ERR_UNSUPPORTED;
    }
    const Geom g = geom_1x1(N, H, W, Cin, Cout, 1);
    const unsigned blocks = (unsigned)fi::ceil_div(g.P, BN);
    hipStream_t st = (hipStream_t)stream;
    const E16 *xe = (const E16 *)x, *we = (const E16 *)w;
    if (Cin % 64 == 0)
        hipLaunchKernelGGL((pyr16_head_kernel<64>), dim3(blocks), dim3(kThreads), 0, st, xe, we, bias, y, g);
    else
        hipLaunchKernelGGL((pyr16_head_kernel<32>), dim3(blocks), dim3(kThreads), 0, st, xe, we, bias, y, g);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

}  // extern "C"
