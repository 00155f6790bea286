// conv_act16.hip -- libfi_act16.so (include/fi_act16.h): implicit-GEMM convolution on 16-bit channels-last tensors
// (v_mfma_f32_32x32x16_bf16, fp32 accumulation) and the transposing casts at the boundary to fp32 NCHW.
// conv_act16_f16.hip includes this file with FI_E16_HALF defined: the same kernels on IEEE half under the *_f16 names.
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
// written to the other buffer after them; one barrier per K block.  K blocks run taps outer (row-major), channels inner:
// one fixed summation order per element whatever the grid.
// 3x3.  The B row of tap (r, s) for output pixel (oh, ow) is input pixel (oh + r - 1, ow + s - 1); outside the map the
// chunk is a zero selected on the way to LDS and NO address is formed.  Rows of the tile past the last pixel / channel
// are zeros too.
// Epilogue.  C/D map col = lane & 31 (pixel), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (channel): a register quad
// is 4 consecutive channels of one pixel.  Stored straight from that map a wave's instruction touches 32 pixels with 16
// bytes each (a stride of Cout * 2 bytes): the layers with Cin = 64 have ONE K block and are all epilogue, and ran at
// 1.4 TB/s that way.  So the fp32 tile goes through LDS once more and leaves as 16-byte stores, 16 neighbouring lanes per
// 256 contiguous bytes of a pixel; the shortcut is read the same way.
#include <stdint.h>

#include "fi_common.h"
#include "../../include/fi_act16.h"

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

// BM: channel tile (128, or 64 for the narrow layers), BK: K block (64, or 32 when Cin % 64 != 0)
template <int BM, int BK>
__global__ __launch_bounds__(kThreads) void act16_conv_kernel(const E16 *__restrict__ x, const E16 *__restrict__ w,
                                                              const float *__restrict__ scale,
                                                              const float *__restrict__ bias,
                                                              const E16 *__restrict__ residual, E16 *__restrict__ y,
                                                              Geom g)
{
    constexpr int CPR = BK / 8;                    // 16-byte chunks per tile row
    constexpr int A_IT = BM * CPR / kThreads;      // chunks a thread stages per K block
    constexpr int B_IT = BN * CPR / kThreads;
    constexpr int MI = BM / 64;                    // 32 x 32 blocks per wavefront along the channels
    constexpr int NI = 2;                          // ... and along the pixels
    // two staging buffers per operand; the epilogue reuses the bytes for the fp32 output tile
    constexpr int STAGE_CHUNKS = 2 * (BM + BN) * CPR, OUT_CHUNKS = BN * BM / 4;
    __shared__ u32x4 smem[STAGE_CHUNKS > OUT_CHUNKS ? STAGE_CHUNKS : OUT_CHUNKS];
    u32x4(*As)[BM * CPR] = reinterpret_cast<u32x4(*)[BM * CPR]>(smem);
    u32x4(*Bs)[BN * CPR] = reinterpret_cast<u32x4(*)[BN * CPR]>(smem + 2 * BM * CPR);
    f32x4 *Cs = reinterpret_cast<f32x4 *>(smem);

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = (int)(blockIdx.x % (unsigned)g.mtiles) * BM;
    const int n0 = (int)(blockIdx.x / (unsigned)g.mtiles) * BN;          // < P < 2^31 (host check)

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

    f32x16 acc[MI][NI];
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

    // epilogue.  The accumulators go through LDS (free now: the loop ends on a barrier) so that the global accesses are
    // whole 16-byte chunks along the channels with neighbouring lanes on neighbouring chunks of one pixel: fp32 tile
    // Cs[pixel][channel], its 16-byte chunks XORed with (pixel & 15) -- the 16 lanes served together write 16 different
    // pixels at one channel offset and land on 16 different slots.  Then acc * scale + bias + residual, ReLU in fp32 and
    // ONE rounding, 8 channels of one pixel per lane and store.
    constexpr int RC = BM / 4;                     // 16-byte chunks per tile row
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

constexpr long kIntMax = 2147483647L;

constexpr long kCUs = 256;        // compute units of an MI355X

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
