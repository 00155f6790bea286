// conv3x3_wino_wgrad.hip -- Winograd F(2x2,3x3) form of the weight gradient of the 3x3 / stride 1 / pad 1 convolution on NCHW
// maps with even H and W for gfx950.  Reached from launch_wgrad (csrc/conv_igemm.hip) when plan_wgrad sets
// FI_LAUNCH_WINOGRAD; it runs in the conv_wgrad_bm*_3x3 slot of the direct kernel and shares the slot's profiling counter.
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "fi_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;

// -------------------------------------------------------------------------------------
// dW[co][ci] = Gt [ sum over images and tiles (A dY At) . (Bt d B) ] G with the forward kernel's tiles (conv3x3_wino.hip):
// 2 x 2 output tiles, 4 x 4 input windows starting at (2ty - 1, 2tx - 1), B / G / A its matrices.  Sixteen independent
// Cout x Cin GEMMs whose reduction axis is the tiles: 16 MFMA positions per tile where the direct form needs 36.
// A workgroup owns a 64 (Cout) x 64 (Cin) block x 16 positions over one pixel split -- a range of the flattened (image,
// tile row, tile column) space, a whole number of stages of WG_STAGE tiles; a wavefront keeps the 16 transform-domain
// accumulators of its 32 x 32 sub-block (256 registers: one wavefront per SIMD).  Per stage:
//   Yt = A dY At and V = Bt d B are computed ONCE per workgroup on the way into LDS (a thread: one tile x one channel of
//        each operand; x through clamped loads, 4 x (4 + 8 + 4 bytes) -- never an address outside x -- padding selected
//        to zero afterwards, dy through two 8-byte loads), stored [tile][channel][position] with a channel pitch of 20 floats: a
//        lane's 16 A or B operands of one (channel, tile) are four conflict-free ds_read_b128.  The tile pitch is 8 floats
//        more than 64 channels, so the ds_write_b128 of the 4 tiles x 2 channels of a lane group fall on distinct banks;
//   v_mfma_f32_32x32x2_f32 takes two tiles (the half-wavefronts) of one position: 32 MFMAs per wavefront and stage.
// The loop is software pipelined by hand like the forward kernel's, one slot per MFMA, with TWO stages of loads in flight
// (one wavefront per SIMD has nothing else to cover a miss: with one stage in flight the kernel waited for memory every
// stage and lost to the direct kernel on every 2-D map): the loads of stage s + 2 sit in the slots of stage s's first
// tile pair, the transforms and LDS stores of stage s + 1 and the tile decode of stage s + 3 in the slots of the second.
// An accumulator is one chain over the tiles of the split in order; the splits add with atomics.
// A batch (fi::WgradBatch, by value) is several problems of one geometry in one launch: the flattened workgroup index is
// (problem, split, block), and a problem takes fewer, longer splits than it would alone -- the 64 x 64 x 9 atomic adds of
// a workgroup are paid per split.
// The bias gradient is the sum of the dy values a thread stages (Cin block 0 only).
// -------------------------------------------------------------------------------------
constexpr int WG_B = fi::WINO_WG_BLOCK;
constexpr int WG_STAGE = fi::WINO_WG_STAGE;
constexpr int WG_CP = 20;                         // floats per (tile, channel): 16 lanes x 16 bytes at this pitch cover the 64 banks once
constexpr int WG_TP = WG_B * WG_CP + 8;           // floats per tile

struct WgGeom {
    int N, Cin, H, W, Cout;
    int ntiles, tiles_per_split, splits;
    int gx, gy;                                   // Cin blocks, Cout blocks
    unsigned mul_tt, sft_tt, mul_tx, sft_tx;      // magic numbers of tiles per image / per tile row (fi::magic_div)
};

__device__ __forceinline__ int fast_div(int n, unsigned mul, unsigned sft)
{
    return mul ? (int)(__umulhi((unsigned)n, mul) >> sft) : n;
}

// BATCH: several problems of one geometry in one launch -- the workgroup order has the problem in front, (problem, pixel
// split, block), so that a problem's operands stay in one L2, and x / dy / dw / dbias are taken from the by-value table (the
// arguments are not read).  The plain kernel is its own instantiation, with no table among its arguments: the stage loop's
// schedule is sensitive to everything around it, and a run-time `if (wb.n)` in ONE kernel cost the plain launches 10 %.
// PAIR: the two centre columns of a window row (2 tx and 2 tx + 1: never clamped, 8-byte aligned -- x is 16-byte aligned, H
// and W are even) come with ONE 8-byte load: 12 loads of x per thread and stage where the scalar staging has 16.  The values
// staged and every floating-point operation are those of the scalar staging (PAIR = false, which FI_WINO_WGRAD_SCALAR_STAGING
// keeps reachable): the results are the same bit for bit.
struct NoBatch {};
template <bool BATCH, bool PAIR>
__global__ __launch_bounds__(kThreads, 1) void conv3x3_wino_wgrad_kernel(const float *__restrict__ x,
                                                                        const float *__restrict__ dy,
                                                                        float *__restrict__ dw,
                                                                        float *__restrict__ dbias, WgGeom g,
                                                                        typename std::conditional<BATCH, fi::WgradBatch, NoBatch>::type wb)
{
    __shared__ __attribute__((aligned(16))) float Ys[2][WG_STAGE][WG_TP];     // A dY At [tile][cout][position]
    __shared__ __attribute__((aligned(16))) float Vs[2][WG_STAGE][WG_TP];     // Bt d B  [tile][cin][position]

    // XCD-aware order (1-D launch): the workgroups, sorted by (pixel split, block), are cut into 8 contiguous bands, one
    // per XCD -- the blocks of a split read the same dy / x ranges, so a split is fetched into ONE L2
    const int blocks = g.gx * g.gy;
    int nblk = blocks * g.splits;                                    // workgroups of one problem
    if constexpr (BATCH) nblk *= wb.n;
    const int per_xcd = (nblk + 7) >> 3;
    int idx = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if (idx >= nblk) return;
    if constexpr (BATCH) {
        const int prob = idx / (blocks * g.splits);
        idx -= prob * blocks * g.splits;
        x = wb.x[prob];
        dy = wb.dy[prob];
        dw = wb.dw[prob];
        dbias = wb.db[prob];
    }
    const int sp = idx / blocks, blk = idx - sp * blocks;
    const int by = blk / g.gx, bx = blk - by * g.gx;
    const int m0 = by * WG_B, c0 = bx * WG_B;
    const int t_begin = sp * g.tiles_per_split;
    const int t_end = min(g.ntiles, t_begin + g.tiles_per_split);
    if (t_begin >= t_end) return;

    const int H = g.H, W = g.W, HW = H * W;
    const int TX = W / 2, TY = H / 2, TT = TY * TX;                   // tiles per row, per column, per image

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, khalf = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;

    // ---- staging: a thread owns tile (tid & 3) of the stage and channel (tid >> 2) of both blocks ---------------------
    // window rows / columns outside the image are read at a valid coordinate of the tile and selected to zero; a tile past
    // the end of the split reads the split's first tile and stages zeros
    const int s_j = tid & 3, s_c = tid >> 2;
    // Two stages are in flight: the stage k's loads go to register set k & 1 and its halo flags to flag set k & 1; the
    // offsets (one set) are those of the newest decode, which the next loads use.
    int s_xo = 0, s_yo = 0;                       // element offsets: the (image, channel) plane of x, the tile's first pixel of dy
    int s_ro[4], s_co[4];
    bool s_ok[2] = {false, false}, s_rok[2][4], s_cok[2][4];
    int d_n = 0, d_ty = 0, d_tx = 0;              // decode in flight
    bool d_ok = false;
    auto decode_tile = [&](int t) {
        d_ok = t < t_end;
        const int tc = d_ok ? t : t_begin;
        d_n = fast_div(tc, g.mul_tt, g.sft_tt);
        const int rem = tc - d_n * TT;
        d_ty = fast_div(rem, g.mul_tx, g.sft_tx);
        d_tx = rem - d_ty * TX;
    };
    auto decode_rows = [&](int par) {
        s_ok[par] = d_ok;
        s_ro[1] = 2 * d_ty * W;
        s_ro[2] = s_ro[1] + W;
        s_ro[0] = d_ty > 0 ? s_ro[1] - W : s_ro[1];
        s_ro[3] = d_ty < TY - 1 ? s_ro[2] + W : s_ro[2];
        s_rok[par][0] = d_ok && d_ty > 0;
        s_rok[par][1] = s_rok[par][2] = d_ok;
        s_rok[par][3] = d_ok && d_ty < TY - 1;
    };
    auto decode_cols = [&](int par) {
        s_co[1] = 2 * d_tx;
        s_co[2] = s_co[1] + 1;
        s_co[0] = d_tx > 0 ? s_co[1] - 1 : s_co[1];
        s_co[3] = d_tx < TX - 1 ? s_co[2] + 1 : s_co[2];
        s_cok[par][0] = d_tx > 0;
        s_cok[par][1] = s_cok[par][2] = true;
        s_cok[par][3] = d_tx < TX - 1;
        s_xo = (d_n * g.Cin + c0 + s_c) * HW;                        // < 2^31 (wgrad_same_size)
        s_yo = (d_n * g.Cout + m0 + s_c) * HW + s_ro[1] + s_co[1];
    };
    float raw[2][16];                             // the window, [row][column]
    float2 ry[2][2];                              // the dy tile, one row each
    auto load_x = [&](int par, int r, int c) {                       // (c is a constant wherever this is called)
        if (PAIR && c == 1) {
            const float2 v = *reinterpret_cast<const float2 *>(x + s_xo + s_ro[r] + s_co[1]);
            raw[par][4 * r + 1] = v.x;
            raw[par][4 * r + 2] = v.y;
        } else if (!PAIR || c != 2) {
            raw[par][4 * r + c] = x[s_xo + s_ro[r] + s_co[c]];
        }
    };
    auto load_y = [&](int par, int r) { ry[par][r] = *reinterpret_cast<const float2 *>(dy + s_yo + r * W); };
    float sd[4][4];                               // Bt d of the window being staged
    auto scol = [&](int par, int c) {
        const float d0 = (s_rok[par][0] && s_cok[par][c]) ? raw[par][c] : 0.0f;
        const float d1 = (s_rok[par][1] && s_cok[par][c]) ? raw[par][4 + c] : 0.0f;
        const float d2 = (s_rok[par][2] && s_cok[par][c]) ? raw[par][8 + c] : 0.0f;
        const float d3 = (s_rok[par][3] && s_cok[par][c]) ? raw[par][12 + c] : 0.0f;
        sd[0][c] = d0 - d2;
        sd[1][c] = d1 + d2;
        sd[2][c] = d2 - d1;
        sd[3][c] = d1 - d3;
    };
    auto srow = [&](int buf, int r) {                                // (Bt d) B
        f32x4_t v;
        v.x = sd[r][0] - sd[r][2];
        v.y = sd[r][1] + sd[r][2];
        v.z = sd[r][2] - sd[r][1];
        v.w = sd[r][1] - sd[r][3];
        *reinterpret_cast<f32x4_t *>(&Vs[buf][s_j][s_c * WG_CP + 4 * r]) = v;
    };
    float yt[4][2];                               // A dY of the tile being staged
    float bsum = 0.0f;
    auto ycols = [&](int par) {
        const float a = s_ok[par] ? ry[par][0].x : 0.0f, b = s_ok[par] ? ry[par][0].y : 0.0f;
        const float c = s_ok[par] ? ry[par][1].x : 0.0f, d = s_ok[par] ? ry[par][1].y : 0.0f;
        yt[0][0] = a;     yt[0][1] = b;
        yt[1][0] = a + c; yt[1][1] = b + d;
        yt[2][0] = a - c; yt[2][1] = b - d;
        yt[3][0] = -c;    yt[3][1] = -d;
        bsum += (a + b) + (c + d);
    };
    auto yrow = [&](int buf, int r) {                                // (A dY) At
        f32x4_t v;
        v.x = yt[r][0];
        v.y = yt[r][0] + yt[r][1];
        v.z = yt[r][0] - yt[r][1];
        v.w = -yt[r][1];
        *reinterpret_cast<f32x4_t *>(&Ys[buf][s_j][s_c * WG_CP + 4 * r]) = v;
    };

    f32x16 acc[16];
#pragma unroll
    for (int q = 0; q < 16; ++q)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[q][e] = 0.0f;

    // prologue: stages 0 and 1 loaded, stage 0 staged, stage 2 decoded
    const int steps = (t_end - t_begin + WG_STAGE - 1) / WG_STAGE;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        decode_tile(t_begin + k * WG_STAGE + s_j);
        decode_rows(k);
        decode_cols(k);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) load_x(k, r, c);
        load_y(k, 0);
        load_y(k, 1);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) scol(0, c);
#pragma unroll
    for (int r = 0; r < 4; ++r) srow(0, r);
    ycols(0);
#pragma unroll
    for (int r = 0; r < 4; ++r) yrow(0, r);
    decode_tile(t_begin + 2 * WG_STAGE + s_j);
    decode_rows(0);
    decode_cols(0);
    __syncthreads();

    // operands of the two tile pairs of a stage: the half-wavefront khalf takes tile 2 * pair + khalf
    f32x4_t aq[2][4], bq[2][4];
    const int a_off = khalf * WG_TP + (wm * 32 + l31) * WG_CP;
    const int b_off = khalf * WG_TP + (wn * 32 + l31) * WG_CP;
    // stage st, PP its parity (compile time: the register sets are statically indexed)
    auto stage = [&](int st, auto PP) {
        constexpr int P = decltype(PP)::value;
        const float *__restrict__ ya = &Ys[P][0][0] + a_off;
        const float *__restrict__ vb = &Vs[P][0][0] + b_off;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            aq[0][i] = *reinterpret_cast<const f32x4_t *>(ya + 4 * i);
            bq[0][i] = *reinterpret_cast<const f32x4_t *>(vb + 4 * i);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[p][q >> 2][q & 3], bq[p][q >> 2][q & 3], acc[q], 0, 0, 0);
                if (p == 0) {
                    // the second pair's operands (slots 0 .. 7), and the loads of stage st + 2 into the register set stage
                    // st has left, a window column per 4 slots (a stage past the split's end re-reads the first tile and is
                    // dropped: no branch on the stage count)
                    if (q < 4) aq[1][q] = *reinterpret_cast<const f32x4_t *>(ya + 2 * WG_TP + 4 * q);
                    else if (q < 8) bq[1][q - 4] = *reinterpret_cast<const f32x4_t *>(vb + 2 * WG_TP + 4 * (q - 4));
                    load_x(P, q & 3, q >> 2);
                    if (q < 2) load_y(P, q);
                } else {
                    // the transforms and LDS stores of stage st + 1 (loaded a stage and a half ago), then the tile decode of
                    // stage st + 3 into its flag set
                    if (q < 4) scol(P ^ 1, q);
                    else if (q < 8) srow(P ^ 1, q - 4);
                    else if (q == 8) ycols(P ^ 1);
                    else if (q < 13) yrow(P ^ 1, q - 9);
                    else if (q == 13) decode_tile(t_begin + (st + 3) * WG_STAGE + s_j);
                    else if (q == 14) decode_rows(P ^ 1);
                    else decode_cols(P ^ 1);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __syncthreads();
    };
    // (an odd count runs one stage of zeros: the loop body has no branch on the stage count and none that diverges -- only
    // fast_div's uniform `mul ? ... : n` --, so the accumulators stay in place: with `if (st + 1 < steps)` around the second
    // stage the compiler copied them at the join and spilled 103 registers)
    for (int st = 0; st < steps; st += 2) {
        stage(st, fi::Int<0>{});
        stage(st + 1, fi::Int<1>{});
    }

    // ---- epilogue: lane = one input channel x 16 output channels (rows (e&3) + 8*(e>>2) + 4*khalf); Gt M G per pair ------
    // (the halvings are exact)
    const int ci = c0 + wn * 32 + l31;
    const int mb = m0 + wm * 32 + 4 * khalf;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int co = mb + (e & 3) + 8 * (e >> 2);
        float rw[3][4];                                              // Gt M
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float m1 = acc[4 + c][e], m2 = acc[8 + c][e];
            const float hs = 0.5f * (m1 + m2);
            rw[0][c] = acc[c][e] + hs;
            rw[1][c] = 0.5f * (m1 - m2);
            rw[2][c] = acc[12 + c][e] + hs;
        }
        float *__restrict__ o = dw + (size_t)co * 9 * g.Cin + ci;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float hs = 0.5f * (rw[i][1] + rw[i][2]);
            atomicAdd(o + (size_t)(3 * i + 0) * g.Cin, rw[i][0] + hs);
            atomicAdd(o + (size_t)(3 * i + 1) * g.Cin, 0.5f * (rw[i][1] - rw[i][2]));
            atomicAdd(o + (size_t)(3 * i + 2) * g.Cin, rw[i][3] + hs);
        }
        __builtin_amdgcn_sched_barrier(0);        // 16 accumulator reads at a time: hoisted together they spill
    }
    if (dbias != nullptr && bx == 0) {            // the 4 lanes that share s_c hold the 4 tiles of a stage
        float v = bsum;
        v += __shfl_xor(v, 1, 64);
        v += __shfl_xor(v, 2, 64);
        if (s_j == 0) atomicAdd(dbias + m0 + s_c, v);
    }
}

}  // namespace

namespace fi {

void launch_conv3x3_wino_wgrad(const WinoWgradArgs &a, hipStream_t st, const WgradBatch *batch)
{
    WgGeom g;
    g.N = a.N; g.Cin = a.Cin; g.H = a.H; g.W = a.W; g.Cout = a.Cout;
    const int TX = a.W / 2, TT = (a.H / 2) * TX;
    g.ntiles = a.N * TT;
    g.tiles_per_split = a.tiles_per_split;
    g.splits = a.splits;
    g.gx = a.Cin / WG_B;
    g.gy = a.Cout / WG_B;
    magic_div((unsigned)TT, g.mul_tt, g.sft_tt);
    magic_div((unsigned)TX, g.mul_tx, g.sft_tx);
    const long nblk = (long)g.gx * g.gy * g.splits * (batch ? batch->n : 1);
    const dim3 grid((unsigned)(((nblk + 7) / 8) * 8));
    const dim3 block(kThreads);
    // (the staging is no part of the plan: both instantiations run the planned launch and give the same bits; the switch is
    // there for the probe and the tests)
    const bool scalar_staging = getenv("FI_WINO_WGRAD_SCALAR_STAGING") != nullptr;
    if (batch) {
        auto k = scalar_staging ? conv3x3_wino_wgrad_kernel<true, false> : conv3x3_wino_wgrad_kernel<true, true>;
        hipLaunchKernelGGL(k, grid, block, 0, st, a.x, a.dy, a.dw, a.dbias, g, *batch);
    } else {
        auto k = scalar_staging ? conv3x3_wino_wgrad_kernel<false, false> : conv3x3_wino_wgrad_kernel<false, true>;
        hipLaunchKernelGGL(k, grid, block, 0, st, a.x, a.dy, a.dw, a.dbias, g, NoBatch{});
    }
}

}  // namespace fi
