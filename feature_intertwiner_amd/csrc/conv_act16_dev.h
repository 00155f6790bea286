// conv_act16_dev.h -- device code of the implicit-GEMM convolution on 16-bit channels-last tensors, shared by
// conv_act16.hip (fi_act16_conv_forward, libfi_act16.so) and conv_pyr16.hip (fi_pyr16_lateral / fi_pyr16_head1x1,
// libfi_pyr16.so): the 16-bit type of the translation unit, the vector types, the launch geometry, the XOR-swizzled LDS
// index, the main loop and the hand-over of the fp32 tile to LDS.  Every kernel goes through THIS loop, so an element's
// sum is formed in one order whichever library launches it: taps outer (row-major), input channels ascending.  Only the
// epilogues differ and they stay with their kernels.
//
// Orientation.  D[m][p] = sum_k A[m][k] B[k][p] with m = output channel, p = output pixel flattened over N*OH*OW (a pixel
// tile may span images) and k = (tap, input channel).  In NHWC with tap-major weights BOTH operands are contiguous along
// k: a weight row w[m][tap][ci..] and an activation row x[pixel of the tap][ci..].  A lane's MFMA fragment -- A[row][8h+j],
// B[8h+j][col], j = 0..7 -- is therefore ONE 16-byte chunk of such a row: global -> LDS is 16-byte loads and 16-byte LDS
// writes with no conversion and no transposing write, LDS -> registers one 16-byte read per fragment.
// LDS.  A tile row holds BK 16-bit values = CPR chunks of 16 bytes.  Chunk c of row r is stored at chunk position
// c ^ ((r / (16 / CPR)) % CPR): the 16 lanes the hardware serves together read 16 consecutive rows at one chunk index,
// and with the XOR they fall on 16 different 16-byte slots of the 256-byte bank row (no conflict); the writes of a row's
// chunks by neighbouring lanes stay inside that row's bytes (no conflict either).
// Pipeline.  Register staging with two LDS buffers: the loads of K block i+1 are issued before the MFMAs of block i and
// written to the other buffer after them; one barrier per K block.
// 3x3.  The B row of tap (r, s) for output pixel (oh, ow) is input pixel (oh + r - 1, ow + s - 1); outside the map the
// chunk is a zero selected on the way to LDS and NO address is formed.  Rows of the tile past the last pixel / channel
// are zeros too.
// The file is included with FI_E16_HALF defined or not (the *_f16.hip twins); everything is in an unnamed namespace, so
// the two instances in one library do not meet.
#pragma once
#include <stdint.h>

#include "fi_common.h"

#ifdef FI_E16_HALF
#define E16 _Float16
#define MFMA16 __builtin_amdgcn_mfma_f32_32x32x16_f16
#define FI16(stem) stem##_f16
#else
#define E16 __bf16
#define MFMA16 __builtin_amdgcn_mfma_f32_32x32x16_bf16
#define FI16(stem) stem##_bf16
#endif

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef E16 e16x8 __attribute__((ext_vector_type(8)));
typedef E16 e16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;     // 4 wavefronts, 2 (channels) x 2 (pixels)
constexpr int BN = 128;           // pixel tile

constexpr long kIntMax = 2147483647L;

constexpr long kCUs = 256;        // compute units of an MI355X

struct Geom {
    int N, H, W, Cin, Cout, RS, S, stride, pad, OH, OW;
    int P;            // N * OH * OW
    int mtiles;       // channel tiles (the fast index of the grid: the workgroups of one pixel tile run together)
    int relu;
};

template <int CPR>
__device__ __forceinline__ int lds_chunk(int row, int c)
{
    return row * CPR + (c ^ ((row / (16 / CPR)) & (CPR - 1)));
}

// 16-byte chunks of LDS a kernel on BM x BN tiles with K blocks of BK declares: two staging buffers per operand; the
// epilogue reuses the bytes for the fp32 output tile
template <int BM, int BK>
constexpr int tile_smem_chunks()
{
    return 2 * (BM + BN) * (BK / 8) > BN * BM / 4 ? 2 * (BM + BN) * (BK / 8) : BN * BM / 4;
}

// The channel tile of a launch: 64 rows where a 128-row tile would be at most half full (C2's conv1 / conv2), and where
// 128-row tiles would give at most one workgroup per compute unit (the 3x3 layers of C4 / C5: a lone workgroup leaves every
// SIMD with a single wavefront and nothing to hide its barrier behind).  Measured, bf16 (profiles/act16_probe.txt): 3x3
// 256 -> 256 on 4 x 64 x 64, 256 workgroups of 128 rows 0.072 ms, 512 of 64 rows 0.064 ms; 3x3 128 -> 128 on 2 x 168 x 168,
// 441 of 128 rows 0.060 ms, 882 of 64 rows 0.066 ms -- past one workgroup per CU the larger tile's reuse wins.
inline int conv_bm(int Cout, long P)
{
    if (Cout <= 64) return 64;
    const long blocks128 = ((P + BN - 1) / BN) * ((Cout + 127) / 128);
    return blocks128 <= kCUs ? 64 : 128;
}

// The main loop.  BM: channel tile (128, or 64 for the narrow layers), BK: K block (64, or 32 when Cin % 64 != 0).
// acc[mi][ni] is the 32 x 32 block (channels wm * BM / 2 + 32 mi.., pixels wn * 64 + 32 ni..) of the tile at channel m0,
// pixel n0; smem: tile_smem_chunks<BM, BK>() chunks.  Ends on a barrier: the LDS is free for the epilogue.
template <int BM, int BK>
__device__ __forceinline__ void conv_main_loop(const E16 *__restrict__ x, const E16 *__restrict__ w, const Geom &g,
                                               u32x4 *smem, int m0, int n0, f32x16 (&acc)[BM / 64][2])
{
    constexpr int CPR = BK / 8;                    // 16-byte chunks per tile row
    constexpr int A_IT = BM * CPR / kThreads;      // chunks a thread stages per K block
    constexpr int B_IT = BN * CPR / kThreads;
    constexpr int MI = BM / 64;                    // 32 x 32 blocks per wavefront along the channels
    constexpr int NI = 2;                          // ... and along the pixels
    u32x4(*As)[BM * CPR] = reinterpret_cast<u32x4(*)[BM * CPR]>(smem);
    u32x4(*Bs)[BN * CPR] = reinterpret_cast<u32x4(*)[BN * CPR]>(smem + 2 * BM * CPR);

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;

    // what this thread stages: the same tile rows and chunk index in every K block
    long a_off[A_IT];                              // element offset of w[m][tap 0][chunk], -1: no such channel
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
        const int id = tid + i * kThreads, m = m0 + id / CPR;
        a_off[i] = m < g.Cout ? ((long)m * g.RS * g.Cin + (id % CPR) * 8) : -1;
    }
    long b_img[B_IT];                              // pixel index of the image's first pixel
    int b_ih[B_IT], b_iw[B_IT];                    // input pixel of tap (0, 0); a row past the last pixel: far outside
#pragma unroll
    for (int i = 0; i < B_IT; ++i) {
        const int id = tid + i * kThreads;
        const long p = (long)n0 + id / CPR;
        if (p < g.P) {
            const int img = (int)(p / ((long)g.OH * g.OW));
            const int rem = (int)(p - (long)img * g.OH * g.OW);
            const int oh = rem / g.OW, ow = rem - oh * g.OW;
            b_img[i] = (long)img * g.H * g.W;
            b_ih[i] = oh * g.stride - g.pad;
            b_iw[i] = ow * g.stride - g.pad;
        } else {
            b_img[i] = 0;
            b_ih[i] = -(1 << 30);
            b_iw[i] = -(1 << 30);
        }
    }

    const int kblocks = g.Cin / BK;
    const int iters = g.RS * kblocks;
    u32x4 ra[A_IT], rb[B_IT];
    const u32x4 zero = {0u, 0u, 0u, 0u};

    auto load = [&](int it) {
        const int tap = it / kblocks, kb = it - tap * kblocks;
        const int r = tap / g.S, s = tap - r * g.S;
#pragma unroll
        for (int i = 0; i < A_IT; ++i) {
            ra[i] = zero;
            if (a_off[i] >= 0)
                ra[i] = *reinterpret_cast<const u32x4 *>(w + a_off[i] + (long)tap * g.Cin + kb * BK);
        }
#pragma unroll
        for (int i = 0; i < B_IT; ++i) {
            const int ih = b_ih[i] + r, iw = b_iw[i] + s;
            rb[i] = zero;
            if ((unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W) {
                const int ch = (tid + i * kThreads) % CPR;
                rb[i] = *reinterpret_cast<const u32x4 *>(x + (b_img[i] + (long)ih * g.W + iw) * g.Cin + kb * BK + ch * 8);
            }
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < A_IT; ++i) {
            const int id = tid + i * kThreads;
            As[buf][lds_chunk<CPR>(id / CPR, id % CPR)] = ra[i];
        }
#pragma unroll
        for (int i = 0; i < B_IT; ++i) {
            const int id = tid + i * kThreads;
            Bs[buf][lds_chunk<CPR>(id / CPR, id % CPR)] = rb[i];
        }
    };

#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.f;

    const int fr = lane & 31, fh = lane >> 5;      // fragment row / column, and which 8 of the 16 k
    load(0);
    stage(0);
    __syncthreads();
    for (int it = 0; it < iters; ++it) {
        const int buf = it & 1;
        if (it + 1 < iters) load(it + 1);
#pragma unroll
        for (int kk = 0; kk < BK / 16; ++kk) {
            e16x8 a[MI], b[NI];
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
                a[mi] = *reinterpret_cast<const e16x8 *>(&As[buf][lds_chunk<CPR>(wm * (BM / 2) + mi * 32 + fr, kk * 2 + fh)]);
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
                b[ni] = *reinterpret_cast<const e16x8 *>(&Bs[buf][lds_chunk<CPR>(wn * (BN / 2) + ni * 32 + fr, kk * 2 + fh)]);
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = MFMA16(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
        }
        if (it + 1 < iters) stage(buf ^ 1);        // last read two barriers ago
        __syncthreads();
    }
}

// The accumulators go through LDS (free: the loop ends on a barrier) so that an epilogue's global accesses can run along
// the channels of one pixel: fp32 tile Cs[pixel][channel] of RC = BM / 4 16-byte chunks per row, chunk c of pixel row pr at
// Cs[pr * RC + (c ^ (pr & 15))] -- the 16 lanes served together write 16 different pixels at one channel offset and land
// on 16 different slots.  C/D map of the MFMA: col = lane & 31 (pixel), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
// (channel): a register quad is 4 consecutive channels of one pixel.  Ends on a barrier.
template <int BM>
__device__ __forceinline__ void tile_to_lds(const f32x16 (&acc)[BM / 64][2], f32x4 *Cs)
{
    constexpr int MI = BM / 64, NI = 2, RC = BM / 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int fr = lane & 31, fh = lane >> 5;
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
        const int pr = wn * (BN / 2) + ni * 32 + fr;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int cc = (wm * (BM / 2) + mi * 32 + 8 * q + 4 * fh) / 4;
                f32x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = acc[mi][ni][4 * q + j];
                Cs[pr * RC + (cc ^ (pr & 15))] = v;
            }
        }
    }
    __syncthreads();
}

}  // namespace
