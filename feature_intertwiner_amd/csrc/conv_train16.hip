// conv_train16.hip -- libfi_train16.so (include/fi_train16.h): the data gradient of a convolution on 16-bit channels-last
// tensors with the PRODUCING layer's ReLU mask and column sums in its epilogue (v_mfma_f32_32x32x16_bf16, fp32
// accumulation).  conv_train16_f16.hip includes this file with FI_E16_HALF defined: the same kernel on IEEE half under
// the *_f16 name.
//
// The reduction IS conv_main_loop of conv_act16_dev.h, launched as the ungated data gradient of conv_grad16.hip launches
// it: the same Geom (channel counts swapped, stride 1, the forward's padding), the same tile choice (conv_bm(Cin, P), K
// block 64 / 32 by Cout % 64), the same grid order and, behind tile_to_lds, the same lane -> (pixel, 8 channels) map.  An
// element's fp32 sum is therefore formed in the same order, gets the same dx_add and the same ONE rounding; the select on
// the gate follows the rounding, so dx is bit-equal to relu_grad(dgrad(..), gate) by construction.
//
// Column sums.  tid % (BM / 8) is a thread's channel group and kThreads is a multiple of BM / 8: a thread keeps its 8
// channels for all the pixels it writes and sums the values AS STORED in 8 fp32 registers.  After a barrier (every
// thread has read the fp32 tile) the threads lay their partials down as a [kThreads / (BM / 8)][BM] fp32 image in the
// tile's bytes (8 KB), and after another one thread per channel adds the column in a fixed order and gives colsum ONE
// global fp32 atomic: ceil(P / 128) adds per address and launch, in the order the workgroups arrive.
// LDS: tile_smem_chunks<BM, BK>() chunks, the ungated kernel's -- a single float more would cost the <64, 32> instance
// (32 KB, five workgroups in 160 KB) one of its five.
#include <stdint.h>

#include "fi_common.h"
#include "conv_act16_dev.h"
#include "../../include/fi_train16.h"

namespace {

// g: the geometry of the LOOP (its "input" is the gradient map OH x OW, its rows are the Cin channels of dx, its reduction
// the Cout channels of g); H, W: the map of dx; cell: 1, or 2 for the stride-2 scatter
template <int BM, int BK>
__global__ __launch_bounds__(kThreads) void dgrad_gated_kernel(const E16 *__restrict__ gr, const E16 *__restrict__ wt,
                                                               const E16 *__restrict__ dx_add,
                                                               const E16 *__restrict__ gate, E16 *__restrict__ dx,
                                                               float *__restrict__ colsum, Geom g, int H, int W, int cell)
{
    __shared__ u32x4 smem[tile_smem_chunks<BM, BK>()];
    f32x4 *Cs = reinterpret_cast<f32x4 *>(smem);
    const int tid = threadIdx.x;
    const int m0 = (int)(blockIdx.x % (unsigned)g.mtiles) * BM;
    const int n0 = (int)(blockIdx.x / (unsigned)g.mtiles) * BN;          // < P < 2^31 (host check)
    f32x16 acc[BM / 64][2];
    conv_main_loop<BM, BK>(gr, wt, g, smem, m0, n0, acc);

    constexpr int RC = BM / 4;
    tile_to_lds<BM>(acc, Cs);
    constexpr int CH8 = BM / 8;
    const int cg = tid % CH8;
    const int ci = m0 + cg * 8;
    float part[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) part[j] = 0.f;
    // the stored value of one pixel: the ungated kernel's rounding, then the select, then the sum of what is stored
    auto finish = [&](const float (&v)[8], long o) {
        const e16x8 gt = *reinterpret_cast<const e16x8 *>(gate + o);
        e16x8 out;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            out[j] = (E16)v[j];
            if (!((float)gt[j] > 0.f)) out[j] = (E16)0.f;
            part[j] += (float)out[j];
        }
        *reinterpret_cast<e16x8 *>(dx + o) = out;
    };
    if (ci < g.Cout) {                             // Cin % 8 == 0: a group is whole or absent
#pragma unroll
        for (int i = 0; i < BN * CH8 / kThreads; ++i) {
            const int pr = (tid + i * kThreads) / CH8;
            const long p = (long)n0 + pr;
            if (p >= g.P) break;                   // pr grows with i
            const f32x4 lo = Cs[pr * RC + ((2 * cg) ^ (pr & 15))], hi = Cs[pr * RC + ((2 * cg + 1) ^ (pr & 15))];
            float v[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = lo[j];
                v[4 + j] = hi[j];
            }
            if (cell == 1) {
                const long o = p * g.Cout + ci;
                if (dx_add) {
                    const e16x8 rr = *reinterpret_cast<const e16x8 *>(dx_add + o);
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = v[j] + (float)rr[j];
                }
                finish(v, o);
            } else {
                const int img = (int)(p / ((long)g.OH * g.OW));
                const int rem = (int)(p - (long)img * g.OH * g.OW);
                const int oh = rem / g.OW, ow = rem - oh * g.OW;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int h = 2 * oh + (q >> 1), w = 2 * ow + (q & 1);
                    if (h >= H || w >= W) continue;    // the odd row / column an odd map does not have
                    const long o = (((long)img * H + h) * W + w) * g.Cout + ci;
                    float u[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) u[j] = q == 0 ? v[j] : 0.f;
                    if (dx_add) {
                        const e16x8 rr = *reinterpret_cast<const e16x8 *>(dx_add + o);
#pragma unroll
                        for (int j = 0; j < 8; ++j) u[j] = u[j] + (float)rr[j];
                    }
                    finish(u, o);
                }
            }
        }
    }
    if (colsum) {                                  // uniform over the workgroup
        // row tid / CH8 of a [kThreads / CH8][BM] fp32 image in the bytes of the tile, once every thread has read it
        constexpr int ROWS = kThreads / CH8;
        float *sums = reinterpret_cast<float *>(smem);
        __syncthreads();
        f32x4 *mine = reinterpret_cast<f32x4 *>(sums + (tid / CH8) * BM + cg * 8);
        mine[0] = f32x4{part[0], part[1], part[2], part[3]};
        mine[1] = f32x4{part[4], part[5], part[6], part[7]};
        __syncthreads();
        if (tid < BM && m0 + tid < g.Cout) {
            float t = 0.f;
#pragma unroll
            for (int r = 0; r < ROWS; ++r) t += sums[r * BM + tid];
            atomicAdd(&colsum[m0 + tid], t);
        }
    }
}

// THE statement of what the entry points take (the pointers may be NULL: not known yet): the ungated data gradient's
// rules on g, gate, dx_add and dx
bool train_eligible(int N, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, const void *gp,
                    const void *gate, const void *dx_add, const void *dx)
{
    if (N < 1 || H < 1 || W < 1 || Cin < 32 || Cin % 32 != 0 || Cout < 32 || Cout % 32 != 0) return false;
    const bool g1 = R == 1 && S == 1 && (stride == 1 || stride == 2) && pad == 0;
    const bool g3 = R == 3 && S == 3 && stride == 1 && pad == 1;
    if (!g1 && !g3) return false;
    if ((((uintptr_t)gp | (uintptr_t)gate | (uintptr_t)dx_add | (uintptr_t)dx) & 15) != 0) return false;
    const long OH = (H + 2 * pad - R) / stride + 1, OW = (W + 2 * pad - S) / stride + 1;
    const long P = (long)N * OH * OW;
    if ((long)N * H * W > kIntMax || P > kIntMax || (long)Cout * R * S * Cin > kIntMax) return false;
    const long blocks = ((P + BN - 1) / BN) * fi::ceil_div(Cin, conv_bm(Cin, P));
    return blocks <= kIntMax;
}

}  // namespace

extern "C" {

#ifndef FI_E16_HALF
int fi_train16_eligible(int N, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, const void *g,
                        const void *gate, const void *dx_add, const void *dx)
{
    return train_eligible(N, H, W, Cin, Cout, R, S, stride, pad, g, gate, dx_add, dx) ? 1 : 0;
}
#endif

int FI16(fi_train16_conv_dgrad_gated)(const void *g, const void *wt, const void *dx_add, const void *gate, void *dx,
                                      float *colsum, int N, int H, int W, int Cin, int Cout, int R, int S, int stride,
                                      int pad, fi_stream_t stream)
{
    FI_REQUIRE(N >= 0 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1, "N >= 0, H, W, Cin, Cout >= 1");
    FI_REQUIRE(R >= 1 && S >= 1 && stride >= 1 && pad >= 0, "R, S, stride >= 1, pad >= 0");
    if (N == 0) return FI_OK;
    FI_REQUIRE(g && wt && gate && dx, "null pointer");
    if (!train_eligible(N, H, W, Cin, Cout, R, S, stride, pad, g, gate, dx_add, dx) || ((uintptr_t)wt & 15) != 0 ||
        ((uintptr_t)colsum & 3) != 0) {
        fi::set_error("fi_train16_conv_dgrad_gated: unsupported call (N %d, H %d, W %d, Cin %d, Cout %d, R %d, S %d, "
                      "stride %d, pad %d, g %p, wt %p, dx_add %p, gate %p, dx %p, colsum %p): needs 1x1 / stride 1 or 2 / "
                      "pad 0 or 3x3 / stride 1 / pad 1, Cin %% 32 == 0, Cout %% 32 == 0, the 16-bit tensors aligned to 16 "
                      "bytes, colsum to 4, extents below 2^31",
                      N, H, W, Cin, Cout, R, S, stride, pad, g, wt, dx_add, gate, (const void *)dx, (const void *)colsum);
        return FI_ERR_UNSUPPORTED;
    }
    // the loop's convolution: the gradient map in, Cin channel rows out, stride 1, the forward's padding
    Geom q;
    q.OH = (H + 2 * pad - R) / stride + 1;
    q.OW = (W + 2 * pad - S) / stride + 1;
    q.N = N; q.H = q.OH; q.W = q.OW; q.Cin = Cout; q.Cout = Cin; q.RS = R * S; q.S = S; q.stride = 1; q.pad = pad;
    q.P = N * q.OH * q.OW;
    const int bm = conv_bm(Cin, q.P);
    q.mtiles = fi::ceil_div(Cin, bm);
    q.relu = 0;
    const unsigned blocks = (unsigned)((long)fi::ceil_div(q.P, BN) * q.mtiles);
    hipStream_t st = (hipStream_t)stream;
    if (colsum) FI_HIP_CHECK(hipMemsetAsync(colsum, 0, sizeof(float) * (size_t)Cin, st));
    const E16 *ge = (const E16 *)g, *we = (const E16 *)wt, *ae = (const E16 *)dx_add, *te = (const E16 *)gate;
    E16 *de = (E16 *)dx;
#define FI_TRAIN16_LAUNCH(BM_, BK_)                                                                                  \
    hipLaunchKernelGGL((dgrad_gated_kernel<BM_, BK_>), dim3(blocks), dim3(kThreads), 0, st, ge, we, ae, te, de, colsum, \
                       q, H, W, stride)
    if (bm == 64) {
        if (Cout % 64 == 0) FI_TRAIN16_LAUNCH(64, 64); else FI_TRAIN16_LAUNCH(64, 32);
    } else {
        if (Cout % 64 == 0) FI_TRAIN16_LAUNCH(128, 64); else FI_TRAIN16_LAUNCH(128, 32);
    }
#undef FI_TRAIN16_LAUNCH
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

}  // extern "C"
