// conv3x3_wino.hip -- Winograd F(2x2,3x3) form of the 3x3 / stride 1 / pad 1 convolution on NCHW maps with even H and W
// (forward and data gradient: the mask head's 14 x 14 layers, and the backbone / FPN / RPN layers on 2-D maps) for gfx950.
// Reached from fi_conv2d_forward_live when plan_forward (csrc/conv_igemm.hip) sets FwdPlan::wino; it runs in the
// conv3x3_patch_flat slot (14 x 14) or the conv3x3_patch slot (W % 16 == 0) and shares the slot's profiling counter.
#include <stdint.h>

#include "fi_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kThreads = 256;
constexpr int BK = 16;               // input channels per block

struct Epilogue {
    const float *bias;
    const float *scale;
    const float *residual;
    int relu;
    const float *gate;
};

struct WinoGeom {
    int N, Cin, H, W, Cout;
    int flip;            // taps applied in reverse order (data gradient)
    int ptiles, mtiles;  // groups of WN_GROUP tiles, Cout tiles
    const float *zero;
};

// -------------------------------------------------------------------------------------
// 3x3 / stride 1 / pad 1 on maps with even H and W: Winograd F(2x2,3x3), 16 MFMAs where the direct form needs 36
// -------------------------------------------------------------------------------------
// Y = At [ (G g Gt) . (Bt d B) ] A per 2x2 output tile: an H x W map is exactly H/2 x W/2 tiles whose 4 x 4 input windows
// start at (2ty - 1, 2tx - 1), so no tile is ragged and only the outermost window row / column is padding.  A workgroup
// owns 32 CONSECUTIVE tiles of the flattened (image, tile row, tile column) space (on a map of 64 or more tiles per row:
// 2 output rows x 64 columns; on narrow maps a group wraps rows and spans images) x 128 output channels (4 wavefronts
// x 32); a wavefront keeps the 16 transform-domain accumulators of its 32 x 32 block (256 registers: one wavefront per
// SIMD).  Per block of 16 input channels:
//   V = Bt d B  is computed ONCE per workgroup on the way into LDS (a thread: one tile x two channels, its 4 x 4 window
//               read at clamped coordinates -- never an address outside x -- padding selected to zero afterwards),
//               stored [channel][tile][position] with a tile pitch of 20 floats: a lane's 16 B operands of one channel
//               are four conflict-free ds_read_b128.  Two stagings, one instantiation each, chosen by plan_forward:
//                 PAIR    (x 8-byte aligned) 8 read instructions per channel: the centre columns 2tx, 2tx + 1 of a window
//                         row are one 8-byte load (H and W even: aligned, never clamped in x); the halo columns 2tx - 1
//                         and 2tx + 2 are the neighbouring tiles' centre values, and the 32 tiles of a group are 32
//                         consecutive lanes of a wavefront, so they arrive by a DPP wave shift when the value is
//                         consumed.  Only tile 0 (left) and tile 31 (right) of a group have a halo no lane holds: one
//                         4-byte load per window row, which every other lane aims at its own centre and drops.  Where
//                         the neighbouring lane is not the neighbouring tile (a tile row's first / last tile, the
//                         batch's last tile) the halo is padding and the s_cok select drops what was shifted in.
//                 scalar  (any x; FI_WINO_SCALAR_STAGING) 16 four-byte loads per channel.
//               Both stage the same values, so the outputs are the same bit for bit (the first block, staged in front of
//               the loop, takes the 4-byte loads with either);
//   U = G g Gt  is computed by every lane from the tap-major weights the direct kernel loads as well (9 x 16 bytes per
//               half block of 4 channels, double buffered in registers): 28 VALU operations per (cout, cin), in the
//               shadow of the 16 MFMAs of the channel before.  flip only changes which tap goes where in g.
// The loop is software pipelined by hand, one channel (16 MFMAs) per step: the LDS reads and the weight transform of
// step s + 1 sit between the MFMAs of step s, the next block's input loads at step 0 (PAIR: one per slot, scalar: two),
// its weight loads at steps 1 and 4, its input transform and LDS stores at steps 5 and 6.
// 128 MFMAs per wavefront and channel block (direct: 288).  An accumulator is a chain over the channels in a fixed
// order (block by block, pair (k, k + 8) by pair) and the output transform is lane-local, so an output element's
// arithmetic does not depend on the tile's place in its group or in the batch.
constexpr int WN_GROUP = fi::WINO_GROUP;                       // tiles per workgroup
constexpr int WN_TP = 20;                           // floats per tile of V: 16 lanes x 16 bytes at this pitch cover the 64 banks once
constexpr int WN_CP = WN_GROUP * WN_TP;             // floats per channel of V
typedef float f32x4_t __attribute__((ext_vector_type(4)));

// Epilogue in the flat kernel's order: scale, bias, residual, ReLU, gate.  ONE instance for every combination (with four
// the compiler reads all 256 sums out of the accumulator registers in front of the branch and spills): an absent
// residual / gate is loaded from the page of zeros (stride 0) and selected away.
__device__ __forceinline__ void wino_epilogue(const f32x16 (&acc)[16], const Epilogue &ep, float *__restrict__ y, size_t obase,
                                              bool tile_ok, int mb, int Cout, const float *__restrict__ zero, int W,
                                              size_t HW)
{
    const bool has_sc = ep.scale != nullptr, has_bi = ep.bias != nullptr, relu = ep.relu != 0;
    const bool has_res = ep.residual != nullptr, has_gate = ep.gate != nullptr;
    const float *__restrict__ sp = has_sc ? ep.scale : zero;
    const float *__restrict__ bp = has_bi ? ep.bias : zero;
    const float *__restrict__ rp = has_res ? ep.residual : zero;
    const float *__restrict__ gp = has_gate ? ep.gate : zero;
    const int smul = has_sc ? 1 : 0, bmul = has_bi ? 1 : 0;
    const size_t rmul = has_res ? 1 : 0, gmul = has_gate ? 1 : 0;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int mr = (e & 3) + 8 * (e >> 2);
        const int mrow = min(mb + mr, Cout - 1) - mb;              // clamped row, relative to mb
        const bool row_ok = mb + mr < Cout;
        const size_t o = obase + (size_t)mrow * HW;
        const float sc = sp[(mb + mrow) * smul], bi = bp[(mb + mrow) * bmul];
        const float2 r0 = *reinterpret_cast<const float2 *>(rp + o * rmul);
        const float2 r1 = *reinterpret_cast<const float2 *>(rp + (o + W) * rmul);
        const float2 g0 = *reinterpret_cast<const float2 *>(gp + o * gmul);
        const float2 g1 = *reinterpret_cast<const float2 *>(gp + (o + W) * gmul);
        // At M A: rows first (p[i][0] = m_i0 + m_i1 + m_i2, p[i][1] = m_i1 - m_i2 - m_i3), then columns
        float p[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            p[i][0] = (acc[4 * i][e] + acc[4 * i + 1][e]) + acc[4 * i + 2][e];
            p[i][1] = (acc[4 * i + 1][e] - acc[4 * i + 2][e]) - acc[4 * i + 3][e];
        }
        float t[4];                                                  // (row 0: t0 t1) (row 1: t2 t3)
        t[0] = (p[0][0] + p[1][0]) + p[2][0];
        t[1] = (p[0][1] + p[1][1]) + p[2][1];
        t[2] = (p[1][0] - p[2][0]) - p[3][0];
        t[3] = (p[1][1] - p[2][1]) - p[3][1];
        const float rr[4] = {r0.x, r0.y, r1.x, r1.y}, gt[4] = {g0.x, g0.y, g1.x, g1.y};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v = t[j];
            v = has_sc ? v * sc : v;
            v = has_bi ? v + bi : v;
            v = has_res ? v + rr[j] : v;
            v = relu ? fmaxf(v, 0.0f) : v;
            v = (has_gate && !(gt[j] > 0.0f)) ? 0.0f : v;
            t[j] = v;
        }
        if (tile_ok && row_ok) {
            *reinterpret_cast<float2 *>(y + o) = make_float2(t[0], t[1]);
            *reinterpret_cast<float2 *>(y + o + W) = make_float2(t[2], t[3]);
        }
    }
}

// H and W even, Cin % 16 == 0 (plan_forward).  FIX: H == W == FIX at compile time (the 14 x 14 RoI maps: the tile decode and
// the strides fold to constants), 0: H and W from g.  PAIR: the staging (header comment); it needs x 8-byte aligned.
template <int FIX, bool PAIR>
__global__ __launch_bounds__(kThreads, 1) void conv3x3_wino_flat_kernel(const float *__restrict__ x,
                                                                       const float *__restrict__ w, Epilogue ep,
                                                                       float *__restrict__ y, WinoGeom g)
{
    __shared__ __attribute__((aligned(16))) float Vs[2][BK][WN_CP];

    // XCD-aware order: XCD c owns a contiguous band of tile groups, Cout tiles innermost
    const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3;
    const int per_xcd = (g.ptiles + 7) >> 3;
    const int mt = local % g.mtiles;
    const int pt = xcd * per_xcd + local / g.mtiles;
    if (pt >= g.ptiles) return;
    const int m0 = mt * 128;
    const int H = FIX ? FIX : g.H, W = FIX ? FIX : g.W;
    const int TX = W / 2, TT = (H / 2) * TX;                         // tiles per row, per image
    const int HW = H * W;
    const int ntiles = g.N * TT;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, khalf = lane >> 5;

    // ---- input staging: a thread owns tile (tid & 31) of the group and channels (tid >> 5), (tid >> 5) + 8 -----------
    // window rows / columns outside the image are read at the clamped (valid) coordinate and selected to zero; a tile past
    // the end of the batch reads tile 0
    const int s_t = pt * WN_GROUP + (tid & 31);
    const bool s_ok = s_t < ntiles;
    const int s_tc = s_ok ? s_t : 0;
    const int s_n = s_tc / TT, s_rem = s_tc - s_n * TT;
    const int s_ty = s_rem / TX, s_tx = s_rem - s_ty * TX;
    int s_ro[4], s_co[4];
    bool s_rok[4], s_cok[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int yy = 2 * s_ty - 1 + r, xx = 2 * s_tx - 1 + r;
        s_rok[r] = s_ok && yy >= 0 && yy < H;
        s_cok[r] = xx >= 0 && xx < W;
        s_ro[r] = min(max(yy, 0), H - 1) * W;
        s_co[r] = min(max(xx, 0), W - 1);
    }
    const int s_base = (s_n * g.Cin + (tid >> 5)) * HW;              // < 2^31 (patch_eligible)
    // PAIR, in the loop: raw[i][4 r + 1], [4 r + 2] hold the centre pair of window row r and [4 r] the group-edge value (the
    // left halo of tile 0, the right halo of tile 31, a dropped re-read of the own centre elsewhere); [4 r + 3] is not used
    const bool s_t0 = (tid & 31) == 0, s_t31 = (tid & 31) == 31;
    const int s_ce = s_t0 ? s_co[0] : (s_t31 ? s_co[3] : 2 * s_tx);
    float raw[2][16];
    auto pair_load = [&](const float *__restrict__ xb, int i, int r) {
        const float2 v = *reinterpret_cast<const float2 *>(xb + s_base + i * 8 * HW + s_ro[r] + 2 * s_tx);
        raw[i][4 * r + 1] = v.x;
        raw[i][4 * r + 2] = v.y;
    };
    auto edge_load = [&](const float *__restrict__ xb, int i, int r) {
        raw[i][4 * r] = xb[s_base + i * 8 * HW + s_ro[r] + s_ce];
    };
    // window value (row r, column c) of channel i before the padding select.  PAIR: the halo columns are the centre
    // values of the lane below (wave_shr:1) / above (wave_shl:1); all 64 lanes are active wherever this runs
    auto win = [&](int i, int r, int c) -> float {
        if (!PAIR || c == 1 || c == 2) return raw[i][4 * r + c];
        const int mine = __builtin_bit_cast(int, raw[i][4 * r + (c == 0 ? 2 : 1)]);
        const int edge = __builtin_bit_cast(int, raw[i][4 * r]);     // what a lane without a source lane keeps
        const int theirs = c == 0 ? __builtin_amdgcn_update_dpp(edge, mine, 0x138, 0xf, 0xf, false)
                                  : __builtin_amdgcn_update_dpp(edge, mine, 0x130, 0xf, 0xf, false);
        return (c == 0 ? s_t0 : s_t31) ? raw[i][4 * r] : __builtin_bit_cast(float, theirs);
    };
    // the first block, in front of the loop: 4-byte loads with either staging (once per workgroup; with the shifts here as
    // well the <14, PAIR> instantiation spilled 63 registers around the loop)
    auto stage_load = [&](int cb) {
        const float *__restrict__ xb = x + (size_t)cb * BK * HW;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) raw[i][4 * r + c] = xb[s_base + i * 8 * HW + s_ro[r] + s_co[c]];
    };
    auto stage_store = [&](int buf, int i) {
        {
            float t[4][4];                                           // Bt d
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float d0 = (s_rok[0] && s_cok[c]) ? raw[i][c] : 0.0f;
                const float d1 = (s_rok[1] && s_cok[c]) ? raw[i][4 + c] : 0.0f;
                const float d2 = (s_rok[2] && s_cok[c]) ? raw[i][8 + c] : 0.0f;
                const float d3 = (s_rok[3] && s_cok[c]) ? raw[i][12 + c] : 0.0f;
                t[0][c] = d0 - d2;
                t[1][c] = d1 + d2;
                t[2][c] = d2 - d1;
                t[3][c] = d1 - d3;
            }
            f32x4_t *__restrict__ vp = reinterpret_cast<f32x4_t *>(&Vs[buf][(tid >> 5) + 8 * i][(tid & 31) * WN_TP]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {                            // (Bt d) B
                f32x4_t v;
                v.x = t[r][0] - t[r][2];
                v.y = t[r][1] + t[r][2];
                v.z = t[r][2] - t[r][1];
                v.w = t[r][1] - t[r][3];
                vp[r] = v;
            }
        }
    };

    // ---- weights: 4 consecutive channels of (output channel, tap) per 16-byte load; U = G g Gt per channel ------------
    const int am = min(m0 + wave * 32 + l31, g.Cout - 1);          // rows past Cout re-read the last row
    const float *__restrict__ a_base = w + (size_t)am * 9 * g.Cin + khalf * 8;
    auto load_g = [&](float (&gq)[9][4], int cb, int h) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const float4 v = *reinterpret_cast<const float4 *>(a_base + (size_t)(g.flip ? 8 - tap : tap) * g.Cin + cb * BK + h * 4);
            gq[tap][0] = v.x; gq[tap][1] = v.y; gq[tap][2] = v.z; gq[tap][3] = v.w;
        }
    };
    // the halvings are exact, so the fused forms round like .5 * (a + b + c) and .5 * (a - b + c)
    auto utrans = [&](float (&u)[16], const float (&gq)[9][4], int k) {
        float t[4][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float g0 = gq[c][k], g1 = gq[3 + c][k], g2 = gq[6 + c][k];
            const float hs = 0.5f * (g0 + g2);
            t[0][c] = g0;
            t[1][c] = __builtin_fmaf(0.5f, g1, hs);
            t[2][c] = __builtin_fmaf(-0.5f, g1, hs);
            t[3][c] = g2;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float hs = 0.5f * (t[r][0] + t[r][2]);
            u[4 * r + 0] = t[r][0];
            u[4 * r + 1] = __builtin_fmaf(0.5f, t[r][1], hs);
            u[4 * r + 2] = __builtin_fmaf(-0.5f, t[r][1], hs);
            u[4 * r + 3] = t[r][2];
        }
    };

    f32x16 acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.0f;

    float ga[9][4], gb[9][4];        // weights of the two half blocks (4 channels each) in flight / in use
    float u[2][16];                  // U of the current and the next step
    f32x4_t bq[2][4];                // V of the current and the next step
    auto bread = [&](f32x4_t (&b)[4], const float *__restrict__ vb) {
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i] = *reinterpret_cast<const f32x4_t *>(vb + 4 * i);
    };
    const int ncb = g.Cin / BK;
    stage_load(0);
    load_g(ga, 0, 0);
    load_g(gb, 0, 1);
    stage_store(0, 0);
    stage_store(0, 1);
    utrans(u[0], ga, 0);
    __syncthreads();
    // The same work cut into pieces that sit between the MFMAs of a step (slot q follows MFMA q; nothing moves across a
    // slot's end): a piece is at most 8 VALU operations, 2 loads or one LDS access, well inside the 64 cycles of an MFMA.
    float ut[4][3];                  // G g of the U being built
    float sd[4][4];                  // Bt d of the tile being staged
    auto ucol = [&](const float (&gq)[9][4], int k, int c) {
        const float g0 = gq[c][k], g1 = gq[3 + c][k], g2 = gq[6 + c][k];
        const float hs = 0.5f * (g0 + g2);
        ut[0][c] = g0;
        ut[1][c] = __builtin_fmaf(0.5f, g1, hs);
        ut[2][c] = __builtin_fmaf(-0.5f, g1, hs);
        ut[3][c] = g2;
    };
    auto urow = [&](float (&uo)[16], int r) {
        const float hs = 0.5f * (ut[r][0] + ut[r][2]);
        uo[4 * r + 0] = ut[r][0];
        uo[4 * r + 1] = __builtin_fmaf(0.5f, ut[r][1], hs);
        uo[4 * r + 2] = __builtin_fmaf(-0.5f, ut[r][1], hs);
        uo[4 * r + 3] = ut[r][2];
    };
    auto scol = [&](int i, int c) {
        // the wave shifts of win run in front of the selects: with every lane active
        const float v0 = win(i, 0, c), v1 = win(i, 1, c), v2 = win(i, 2, c), v3 = win(i, 3, c);
        const float d0 = (s_rok[0] && s_cok[c]) ? v0 : 0.0f;
        const float d1 = (s_rok[1] && s_cok[c]) ? v1 : 0.0f;
        const float d2 = (s_rok[2] && s_cok[c]) ? v2 : 0.0f;
        const float d3 = (s_rok[3] && s_cok[c]) ? v3 : 0.0f;
        sd[0][c] = d0 - d2;
        sd[1][c] = d1 + d2;
        sd[2][c] = d2 - d1;
        sd[3][c] = d1 - d3;
    };
    auto srow = [&](int buf, int i, int r) {
        f32x4_t v;
        v.x = sd[r][0] - sd[r][2];
        v.y = sd[r][1] + sd[r][2];
        v.z = sd[r][2] - sd[r][1];
        v.w = sd[r][1] - sd[r][3];
        reinterpret_cast<f32x4_t *>(&Vs[buf][(tid >> 5) + 8 * i][(tid & 31) * WN_TP])[r] = v;
    };
    auto load_g1 = [&](float (&gq)[9][4], int cb, int h, int tap) {
        const float4 v = *reinterpret_cast<const float4 *>(a_base + (size_t)(g.flip ? 8 - tap : tap) * g.Cin + cb * BK + h * 4);
        gq[tap][0] = v.x; gq[tap][1] = v.y; gq[tap][2] = v.z; gq[tap][3] = v.w;
    };

    for (int cb = 0; cb < ncb; ++cb) {
        const int nb = cb + 1 < ncb ? cb + 1 : cb;                   // the last block re-reads itself and drops it (no branch)
        const float *__restrict__ vb = &Vs[cb & 1][khalf * 8][l31 * WN_TP];
        const float *__restrict__ xn = x + (size_t)nb * BK * HW;
        bread(bq[0], vb);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 8; ++s) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(u[s & 1][q], bq[s & 1][q >> 2][q & 3], acc[q], 0, 0, 0);
                // V of step s + 1 (this block's; the next block's step 0 is read behind the barrier)
                if (s < 7 && q < 4)
                    bq[(s + 1) & 1][q] = *reinterpret_cast<const f32x4_t *>(vb + (s + 1) * WN_CP + 4 * q);
                // U of step s + 1: odd slots 1 .. 13
                if (q == 1 || q == 3 || q == 5) {
                    if (s + 1 < 4)
                        ucol(ga, s + 1, q >> 1);
                    else if (s + 1 < 8)
                        ucol(gb, s - 3, q >> 1);
                    else
                        ucol(ga, 0, q >> 1);                         // step 0 of the next block
                }
                if (q == 7 || q == 9 || q == 11 || q == 13) urow(u[(s + 1) & 1], (q - 7) >> 1);
                // the next block's input: 16 (PAIR) or 32 loads at step 0, transformed and stored at steps 5 and 6 (even
                // slots)
                if (s == 0 && PAIR) {
                    const int i = q >> 3, r = q & 3;
                    if (q & 4)
                        edge_load(xn, i, r);
                    else
                        pair_load(xn, i, r);
                }
                if (s == 0 && !PAIR) {
                    const int e0 = 2 * (q & 7), i = q >> 3;
                    raw[i][e0] = xn[s_base + i * 8 * HW + s_ro[e0 >> 2] + s_co[e0 & 3]];
                    raw[i][e0 + 1] = xn[s_base + i * 8 * HW + s_ro[e0 >> 2] + s_co[(e0 & 3) + 1]];
                }
                if ((s == 5 || s == 6) && (q & 1) == 0) {
                    if (q < 8)
                        scol(s - 5, q >> 1);
                    else
                        srow((cb + 1) & 1, s - 5, (q - 8) >> 1);     // unconditional: the loop body stays one basic block
                }
                // weights: the second half block's at step 1 (first used in step 3), the next block's first half at step 4
                if (s == 1 && q < 9) load_g1(gb, cb, 1, q);
                if (s == 4 && q < 9) load_g1(ga, nb, 0, q);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __syncthreads();
    }

    // ---- epilogue: lane = one tile (2 x 2 pixels) x 16 channels (rows (e&3) + 8*(e>>2) + 4*khalf) ---------------------
    const int mb = m0 + wave * 32 + 4 * khalf;
    const int o_t = pt * WN_GROUP + l31;
    const bool tile_ok = o_t < ntiles;
    const int o_tc = tile_ok ? o_t : 0;
    const int o_n = o_tc / TT, o_rem = o_tc - o_n * TT;
    const int o_ty = o_rem / TX, o_tx = o_rem - o_ty * TX;
    const size_t obase = ((size_t)o_n * g.Cout + mb) * HW + (size_t)(2 * o_ty) * W + 2 * o_tx;
    wino_epilogue(acc, ep, y, obase, tile_ok, mb, g.Cout, g.zero, W, (size_t)HW);
}

}  // namespace

namespace fi {

void launch_conv3x3_wino_flat(const WinoArgs &a, hipStream_t st)
{
    WinoGeom g;
    g.N = a.N; g.Cin = a.Cin; g.H = a.H; g.W = a.W; g.Cout = a.Cout;
    g.flip = a.flip;
    g.ptiles = ceil_div(a.N * (a.H / 2) * (a.W / 2), WN_GROUP);
    g.mtiles = ceil_div(a.Cout, 128);
    g.zero = a.zero;
    const Epilogue ep = {a.bias, a.scale, a.residual, a.relu, a.gate};
    auto k = a.hw14 ? (a.pair ? conv3x3_wino_flat_kernel<WINO_HW, true> : conv3x3_wino_flat_kernel<WINO_HW, false>)
                    : (a.pair ? conv3x3_wino_flat_kernel<0, true> : conv3x3_wino_flat_kernel<0, false>);
    hipLaunchKernelGGL(k, dim3((unsigned)a.grid), dim3(kThreads), 0, st, a.x, a.w, ep, a.y, g);
}

}  // namespace fi
