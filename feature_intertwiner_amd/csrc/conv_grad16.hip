// conv_grad16.hip -- libfi_grad16.so (include/fi_grad16.h): the backward operators of a convolution on 16-bit
// channels-last tensors -- ReLU mask + column sums, data gradient, weight gradient (v_mfma_f32_32x32x16_bf16, fp32
// accumulation).  conv_grad16_f16.hip includes this file with FI_E16_HALF defined: the same kernels on IEEE half under the
// *_f16 names.
//
// Data gradient.  dx = conv(g, wt) with the channel counts swapped, so it IS conv_main_loop of conv_act16_dev.h: A rows are
// wt[ci][tap][co..], B rows g[pixel of the tap][co..], both contiguous along the reduction.  The epilogue is the forward's
// (fp32 tile through LDS, 8 channels of a pixel per lane, one rounding); for the 1x1 / stride-2 layers the loop runs over
// the OH x OW pixels of g and the epilogue scatters each to (2 oh, 2 ow) and writes the (up to) three other pixels of its
// 2 x 2 cell as zero (+ dx_add): every pixel of dx belongs to exactly one cell, so dx is covered without a memset.
//
// Weight gradient.  dw[co][tap][ci] = sum_p g[p][co] x[pixel of (p, tap)][ci]: D[m][n] = sum_k A[m][k] B[k][n] with m = co,
// n = ci and k = the PIXEL.  In memory both operands are contiguous along the channels, i.e. along m and n, not along k:
// each MFMA fragment (8 consecutive k of one m / n per lane) is a COLUMN of the staged tile.  The tiles are staged as they
// lie in memory -- pixel rows of 128 channels, 16-byte chunks, no transposing write -- and read with ds_read_b64_tr_b16,
// which hands a 16-lane group a 4 (rows) x 16 (columns) block column-major: lane i of the group receives column i of
// the 4 rows and lane 4q + p supplies the address of row q, columns 4p..4p+3.  Two such reads are one fragment.
// LDS image: 256-byte rows, chunk ch of row r at 256 r + 16 (ch ^ (((r & 3) << 2) | ((r >> 2) & 3))): the 32 lanes of a
// half address rows r0..r0+3 (r & 3 = q) at 4 consecutive chunks in two row groups, the XOR spreads them over all 64
// banks; a row's 16 chunk writes stay inside its 256 bytes.  The read needs EXEC all ones: the tiles are padded with zeros
// (pixel rows past the last pixel, channels past the last channel, taps outside the map) and every lane of every wave
// reads in every K block -- nothing is masked or branched around.
// A workgroup: 128 (co) x 128 (ci) of ONE tap over a range of K blocks of 32 pixels, 4 waves of 64 x 64, register staging
// with two LDS buffers like the forward (32 KB).  The tap is the fastest grid index: the nine workgroups that stage the
// same g tile run together and share it in L2.
#include <stdint.h>

#include "fi_common.h"
#include "conv_act16_dev.h"
#include "../../include/fi_grad16.h"

namespace {

typedef short s16x4 __attribute__((ext_vector_type(4)));     // what the builtin of ds_read_b64_tr_b16 returns, either type

// ---- ReLU mask + column sums ---------------------------------------------------------------------------------------
constexpr int RG_ROWS = 128;      // pixel rows of a workgroup
constexpr int RG_CH = 2048;       // channels of a workgroup (its column sums live in LDS)

__global__ __launch_bounds__(kThreads) void relu_grad_kernel(const E16 *dy, const E16 *__restrict__ y, E16 *g,
                                                             float *__restrict__ colsum, int P, int Cout, int relu)
{
    __shared__ float sums[RG_CH];
    const int tid = threadIdx.x;
    const int c_base = (int)blockIdx.y * RG_CH;
    const int cw = Cout - c_base < RG_CH ? Cout - c_base : RG_CH;      // % 8 == 0
    const int C8 = cw / 8;
    if (colsum) {
        for (int c = tid; c < cw; c += kThreads) sums[c] = 0.f;
        __syncthreads();
    }
    // a thread keeps its 8 channels: lanes_c threads across a row, rstep rows at a time
    const int lanes_c = C8 < kThreads ? C8 : kThreads;
    const int rstep = kThreads / lanes_c;
    const long row0 = (long)blockIdx.x * RG_ROWS;
    const long row_end = row0 + RG_ROWS < P ? row0 + RG_ROWS : (long)P;
    if (tid < lanes_c * rstep) {
        for (int cg = tid % lanes_c; cg < C8; cg += lanes_c) {
            float acc[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = 0.f;
            for (long row = row0 + tid / lanes_c; row < row_end; row += rstep) {
                const long o = row * Cout + c_base + cg * 8;
                e16x8 d = *reinterpret_cast<const e16x8 *>(dy + o);
                if (relu) {
                    const e16x8 yy = *reinterpret_cast<const e16x8 *>(y + o);
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (!((float)yy[j] > 0.f)) d[j] = (E16)0.f;
                }
                *reinterpret_cast<e16x8 *>(g + o) = d;
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += (float)d[j];
            }
            if (colsum) {
#pragma unroll
                for (int j = 0; j < 8; ++j) atomicAdd(&sums[cg * 8 + j], acc[j]);
            }
        }
    }
    if (colsum) {
        __syncthreads();
        for (int c = tid; c < cw; c += kThreads) atomicAdd(&colsum[c_base + c], sums[c]);
    }
}

// ---- data gradient -------------------------------------------------------------------------------------------------
// g: the geometry of the LOOP (its "input" is the gradient map OH x OW, its rows are the Cin channels of dx, its reduction
// the Cout channels of g); H, W: the map of dx; cell: 1, or 2 for the stride-2 scatter
template <int BM, int BK>
__global__ __launch_bounds__(kThreads) void dgrad_kernel(const E16 *__restrict__ gr, const E16 *__restrict__ wt,
                                                         const E16 *__restrict__ dx_add, E16 *__restrict__ dx, Geom g,
                                                         int H, int W, int cell)
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
    if (ci >= g.Cout) return;                      // Cin % 8 == 0: a group is whole or absent
#pragma unroll
    for (int i = 0; i < BN * CH8 / kThreads; ++i) {
        const int pr = (tid + i * kThreads) / CH8;
        const long p = (long)n0 + pr;
        if (p >= g.P) break;                       // pr grows with i
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
            e16x8 out;
#pragma unroll
            for (int j = 0; j < 8; ++j) out[j] = (E16)v[j];
            *reinterpret_cast<e16x8 *>(dx + o) = out;
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
                e16x8 out;
#pragma unroll
                for (int j = 0; j < 8; ++j) out[j] = (E16)u[j];
                *reinterpret_cast<e16x8 *>(dx + o) = out;
            }
        }
    }
}

// ---- weight gradient -----------------------------------------------------------------------------------------------
constexpr int WG_T = 128;         // channel tile, co and ci alike: one 256-byte LDS row
constexpr int WG_KP = 32;         // pixels of a K block
constexpr int WG_CPR = WG_T / 8;  // 16-byte chunks of a row
constexpr int WG_IT = WG_KP * WG_CPR / kThreads;      // chunks a thread stages per operand and K block
// The split.  Every part ends in 128 x 128 fp32 atomics, so a part must be worth them: measured over the ResNet-101 trunk
// (profiles/grad16_probe.txt), parts of >= 256 pixels aiming at 4 workgroups per CU took 14.0 ms per backward pass, parts of
// >= 512 pixels aiming at 2 per CU 10.5 ms, >= 1024 pixels at 2 per CU 10.6 ms, >= 1024 at 1 per CU 12.3 ms (the 3x3 layers
// of C2 then run 144 long workgroups); K blocks of 64 pixels (64 KB of LDS) with parts of >= 512 gave 10.3 ms -- not
// worth twice the LDS.
constexpr int WG_MIN_KB = 16;     // fewest K blocks of a pixel split (512 pixels) unless it is the only one
constexpr long WG_TARGET = 2 * kCUs;                  // workgroups the split aims for

struct WGeom {
    int H, W, Cin, Cout, S, stride, pad, OH, OW;
    int P;                        // N * OH * OW
    int taps, mtiles, ntiles;     // grid: tap fastest, then the co tile, the ci tile, the pixel split
    int kblocks, kb_per_split;
    int atomic;                   // more than one split: add into the zero-filled dw
};

// chunk index (16-byte units) of chunk ch of row r in a tile image
__device__ __forceinline__ int wg_chunk(int row, int ch)
{
    return row * WG_CPR + (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

// the 4 x 16 block at rows r0.., chunks c0, c0 + 1 of the image, transposed: this lane's column, rows r0..r0+3
__device__ __forceinline__ e16x4 wg_tr_read(const u32x4 *tile, int r0, int c0, int q, int p)
{
    const char *a = reinterpret_cast<const char *>(tile + wg_chunk(r0 + q, c0 + (p >> 1))) + 8 * (p & 1);
    return __builtin_bit_cast(e16x4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3))) *)a));
}

__global__ __launch_bounds__(kThreads) void wgrad_kernel(const E16 *__restrict__ gr, const E16 *__restrict__ x,
                                                         float *__restrict__ dw, WGeom g)
{
    __shared__ u32x4 smem[2][2][WG_KP * WG_CPR];   // [buffer][g tile, x tile]
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    unsigned b = blockIdx.x;
    const int tap = (int)(b % (unsigned)g.taps);
    b /= (unsigned)g.taps;
    const int co0 = (int)(b % (unsigned)g.mtiles) * WG_T;
    b /= (unsigned)g.mtiles;
    const int ci0 = (int)(b % (unsigned)g.ntiles) * WG_T;
    const int split = (int)(b / (unsigned)g.ntiles);
    const int r = tap / g.S, s = tap - r * g.S;
    const int kb0 = split * g.kb_per_split;
    const int kb1 = kb0 + g.kb_per_split < g.kblocks ? kb0 + g.kb_per_split : g.kblocks;      // kb0 < kb1 (host)

    // what this thread stages: the same tile rows and chunk in every K block, of both operands
    const int ch = tid % WG_CPR;
    const bool g_has = co0 + ch * 8 < g.Cout, x_has = ci0 + ch * 8 < g.Cin;      // % 8 == 0: a chunk is whole or absent
    u32x4 rg[WG_IT], rx[WG_IT];
    const u32x4 zero = {0u, 0u, 0u, 0u};

    auto load = [&](int kb) {
#pragma unroll
        for (int i = 0; i < WG_IT; ++i) {
            const int row = tid / WG_CPR + i * (kThreads / WG_CPR);
            const long p = (long)kb * WG_KP + row;
            rg[i] = zero;
            rx[i] = zero;
            if (p < g.P) {
                if (g_has) rg[i] = *reinterpret_cast<const u32x4 *>(gr + p * g.Cout + co0 + ch * 8);
                const unsigned ohw = (unsigned)(g.OH * g.OW);
                const unsigned img = (unsigned)p / ohw, rem = (unsigned)p - img * ohw;
                const int oh = (int)(rem / (unsigned)g.OW), ow = (int)(rem - (unsigned)oh * (unsigned)g.OW);
                const int ih = oh * g.stride - g.pad + r, iw = ow * g.stride - g.pad + s;
                if (x_has && (unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W)
                    rx[i] = *reinterpret_cast<const u32x4 *>(x + (((long)img * g.H + ih) * g.W + iw) * g.Cin + ci0 + ch * 8);
            }
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < WG_IT; ++i) {
            const int row = tid / WG_CPR + i * (kThreads / WG_CPR);
            smem[buf][0][wg_chunk(row, ch)] = rg[i];
            smem[buf][1][wg_chunk(row, ch)] = rx[i];
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.f;

    // the transposed read of a fragment: 16-lane group (lane >> 4) & 1 takes columns 16.. of the 32, k half lane >> 5
    const int fh = lane >> 5, fg = (lane >> 4) & 1, fq = (lane & 15) >> 2, fp = lane & 3;
    load(kb0);
    stage(0);
    __syncthreads();
    for (int kb = kb0; kb < kb1; ++kb) {
        const int buf = (kb - kb0) & 1;
        if (kb + 1 < kb1) load(kb + 1);
#pragma unroll
        for (int kk = 0; kk < WG_KP / 16; ++kk) {
            e16x8 a[2], bb[2];
            const int k0 = kk * 16 + 8 * fh;
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) {
                const int c0 = (wm * 64 + mi * 32) / 8 + 2 * fg;
                const e16x4 lo = wg_tr_read(smem[buf][0], k0, c0, fq, fp), hi = wg_tr_read(smem[buf][0], k0 + 4, c0, fq, fp);
                a[mi] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
            }
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const int c0 = (wn * 64 + ni * 32) / 8 + 2 * fg;
                const e16x4 lo = wg_tr_read(smem[buf][1], k0, c0, fq, fp), hi = wg_tr_read(smem[buf][1], k0 + 4, c0, fq, fp);
                bb[ni] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
            }
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = MFMA16(a[mi], bb[ni], acc[mi][ni], 0, 0, 0);
        }
        if (kb + 1 < kb1) stage(buf ^ 1);          // last read two barriers ago
        __syncthreads();
    }

    // C/D map: col = lane & 31 (ci), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (co): 32 lanes, 128 contiguous bytes
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const int ci = ci0 + wn * 64 + ni * 32 + (lane & 31);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int co = co0 + wm * 64 + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * fh;
                if (co < g.Cout && ci < g.Cin) {
                    float *o = dw + ((long)co * g.taps + tap) * g.Cin + ci;
                    if (g.atomic) atomicAdd(o, acc[mi][ni][e]); else *o = acc[mi][ni][e];
                }
            }
        }
}

// the cut of the pixel range: enough workgroups for two per compute unit, no part shorter than WG_MIN_KB K blocks
void wgrad_split(long base, int kblocks, int &kb_per_split, int &splits)
{
    long want = base >= WG_TARGET ? 1 : WG_TARGET / base;
    const long most = kblocks / WG_MIN_KB > 1 ? kblocks / WG_MIN_KB : 1;
    if (want > most) want = most;
    kb_per_split = (int)((kblocks + want - 1) / want);
    splits = (kblocks + kb_per_split - 1) / kb_per_split;
}

// THE statement of what the three entry points take (the pointers may be NULL: not known yet)
bool grad_eligible(int kind, int N, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, const void *p0,
                   const void *p1, const void *p2, const void *p3)
{
    if (kind != FI_GRAD16_RELU_GRAD && kind != FI_GRAD16_DGRAD && kind != FI_GRAD16_WGRAD) return false;
    if (N < 1 || H < 1 || W < 1 || Cin < 32 || Cin % 32 != 0 || Cout < 32 || Cout % 32 != 0) return false;
    const bool g1 = R == 1 && S == 1 && (stride == 1 || stride == 2) && pad == 0;
    const bool g3 = R == 3 && S == 3 && stride == 1 && pad == 1;
    if (!g1 && !g3) return false;
    const bool p3_fp32 = kind != FI_GRAD16_DGRAD;
    if ((((uintptr_t)p0 | (uintptr_t)p1) & 15) != 0) return false;
    if (kind != FI_GRAD16_WGRAD && ((uintptr_t)p2 & 15) != 0) return false;
    if (((uintptr_t)p3 & (p3_fp32 ? 3 : 15)) != 0) return false;
    const long OH = (H + 2 * pad - R) / stride + 1, OW = (W + 2 * pad - S) / stride + 1;
    const long P = (long)N * OH * OW;
    if ((long)N * H * W > kIntMax || P > kIntMax || (long)Cout * R * S * Cin > kIntMax) return false;
    long blocks;
    if (kind == FI_GRAD16_RELU_GRAD) {
        blocks = (P + RG_ROWS - 1) / RG_ROWS;
        if (fi::ceil_div(Cout, RG_CH) > 65535) return false;
    } else if (kind == FI_GRAD16_DGRAD) {
        blocks = ((P + BN - 1) / BN) * fi::ceil_div(Cin, conv_bm(Cin, P));
    } else {
        const long base = (long)R * S * fi::ceil_div(Cout, WG_T) * fi::ceil_div(Cin, WG_T);
        int per, splits;
        wgrad_split(base, (int)((P + WG_KP - 1) / WG_KP), per, splits);
        blocks = base * splits;
    }
    return blocks <= kIntMax;
}

}  // namespace

extern "C" {

#ifndef FI_E16_HALF
int fi_grad16_eligible(int kind, int N, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, const void *p0,
                       const void *p1, const void *p2, const void *p3)
{
    return grad_eligible(kind, N, H, W, Cin, Cout, R, S, stride, pad, p0, p1, p2, p3) ? 1 : 0;
}
#endif

int FI16(fi_grad16_relu_grad)(const void *dy, const void *y, void *g, float *colsum, int N, int OH, int OW, int Cout,
                              int relu, fi_stream_t stream)
{
    FI_REQUIRE(N >= 0 && OH >= 1 && OW >= 1 && Cout >= 1, "N >= 0, OH, OW, Cout >= 1");
    if (N == 0) return FI_OK;
    FI_REQUIRE(dy && g && (y || !relu), "null pointer");
    // the rows of a 1x1 / stride 1 layer on an OH x OW map: the geometry the query is asked with
    if (!grad_eligible(FI_GRAD16_RELU_GRAD, N, OH, OW, 32, Cout, 1, 1, 1, 0, dy, y, g, colsum)) {
        fi::set_error("fi_grad16_relu_grad: unsupported call (N %d, OH %d, OW %d, Cout %d, dy %p, y %p, g %p, colsum %p): "
                      "needs Cout %% 32 == 0, the 16-bit tensors aligned to 16 bytes, colsum to 4, N * OH * OW < 2^31",
                      N, OH, OW, Cout, dy, y, (const void *)g, (const void *)colsum);
        return FI_ERR_UNSUPPORTED;
    }
    const int P = N * OH * OW;
    hipStream_t st = (hipStream_t)stream;
    if (colsum) FI_HIP_CHECK(hipMemsetAsync(colsum, 0, sizeof(float) * (size_t)Cout, st));
    hipLaunchKernelGGL(relu_grad_kernel, dim3((unsigned)fi::ceil_div(P, RG_ROWS), (unsigned)fi::ceil_div(Cout, RG_CH)),
                       dim3(kThreads), 0, st, (const E16 *)dy, (const E16 *)y, (E16 *)g, colsum, P, Cout, relu ? 1 : 0);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int FI16(fi_grad16_conv_dgrad)(const void *g, const void *wt, const void *dx_add, void *dx, int N, int H, int W, int Cin,
                               int Cout, int R, int S, int stride, int pad, fi_stream_t stream)
{
    FI_REQUIRE(N >= 0 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1, "N >= 0, H, W, Cin, Cout >= 1");
    FI_REQUIRE(R >= 1 && S >= 1 && stride >= 1 && pad >= 0, "R, S, stride >= 1, pad >= 0");
    if (N == 0) return FI_OK;
    FI_REQUIRE(g && wt && dx, "null pointer");
    if (!grad_eligible(FI_GRAD16_DGRAD, N, H, W, Cin, Cout, R, S, stride, pad, g, wt, dx_add, dx)) {
        fi::set_error("fi_grad16_conv_dgrad: unsupported call (N %d, H %d, W %d, Cin %d, Cout %d, R %d, S %d, stride %d, "
                      "pad %d, g %p, wt %p, dx_add %p, dx %p): needs 1x1 / stride 1 or 2 / pad 0 or 3x3 / stride 1 / pad 1, "
                      "Cin %% 32 == 0, Cout %% 32 == 0, tensors aligned to 16 bytes, extents below 2^31",
                      N, H, W, Cin, Cout, R, S, stride, pad, g, wt, dx_add, (const void *)dx);
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
    const E16 *ge = (const E16 *)g, *we = (const E16 *)wt, *ae = (const E16 *)dx_add;
    E16 *de = (E16 *)dx;
#define FI_GRAD16_LAUNCH(BM_, BK_) \
    hipLaunchKernelGGL((dgrad_kernel<BM_, BK_>), dim3(blocks), dim3(kThreads), 0, st, ge, we, ae, de, q, H, W, stride)
    if (bm == 64) {
        if (Cout % 64 == 0) FI_GRAD16_LAUNCH(64, 64); else FI_GRAD16_LAUNCH(64, 32);
    } else {
        if (Cout % 64 == 0) FI_GRAD16_LAUNCH(128, 64); else FI_GRAD16_LAUNCH(128, 32);
    }
#undef FI_GRAD16_LAUNCH
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int FI16(fi_grad16_conv_wgrad)(const void *g, const void *x, float *dw, int N, int H, int W, int Cin, int Cout, int R,
                               int S, int stride, int pad, fi_stream_t stream)
{
    FI_REQUIRE(N >= 0 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1, "N >= 0, H, W, Cin, Cout >= 1");
    FI_REQUIRE(R >= 1 && S >= 1 && stride >= 1 && pad >= 0, "R, S, stride >= 1, pad >= 0");
    if (N == 0) return FI_OK;
    FI_REQUIRE(g && x && dw, "null pointer");
    if (!grad_eligible(FI_GRAD16_WGRAD, N, H, W, Cin, Cout, R, S, stride, pad, g, x, nullptr, dw)) {
        fi::set_error("fi_grad16_conv_wgrad: unsupported call (N %d, H %d, W %d, Cin %d, Cout %d, R %d, S %d, stride %d, "
                      "pad %d, g %p, x %p, dw %p): needs 1x1 / stride 1 or 2 / pad 0 or 3x3 / stride 1 / pad 1, "
                      "Cin %% 32 == 0, Cout %% 32 == 0, g / x aligned to 16 bytes, dw to 4, extents below 2^31",
                      N, H, W, Cin, Cout, R, S, stride, pad, g, x, (const void *)dw);
        return FI_ERR_UNSUPPORTED;
    }
    WGeom q;
    q.H = H; q.W = W; q.Cin = Cin; q.Cout = Cout; q.S = S; q.stride = stride; q.pad = pad;
    q.OH = (H + 2 * pad - R) / stride + 1;
    q.OW = (W + 2 * pad - S) / stride + 1;
    q.P = N * q.OH * q.OW;
    q.taps = R * S;
    q.mtiles = fi::ceil_div(Cout, WG_T);
    q.ntiles = fi::ceil_div(Cin, WG_T);
    q.kblocks = fi::ceil_div(q.P, WG_KP);
    const long base = (long)q.taps * q.mtiles * q.ntiles;
    int splits;
    wgrad_split(base, q.kblocks, q.kb_per_split, splits);
    q.atomic = splits > 1 ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    if (q.atomic) FI_HIP_CHECK(hipMemsetAsync(dw, 0, sizeof(float) * (size_t)Cout * q.taps * Cin, st));
    hipLaunchKernelGGL(wgrad_kernel, dim3((unsigned)(base * splits)), dim3(kThreads), 0, st, (const E16 *)g, (const E16 *)x,
                       dw, q);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

}  // extern "C"
