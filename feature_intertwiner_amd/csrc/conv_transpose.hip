// conv_transpose.hip -- fp32 transposed 3x3 / stride 2 / padding 1 / output_padding 1 convolution on the CDNA4 matrix
// cores (gfx950): nn.ConvTranspose2d(256, 256, 3, stride=2, padding=1, output_padding=1) + BatchNorm2d + ReLU of the
// reference's make-up layer (lib/sub_module.py:312-314, DEV.UPSAMPLE_FAC = 2 of lib/config.py:205) and the stride-2
// generator of OptTrans (lib/OT_module.py:24-36), which ran through cuDNN.  libfi_convt.so, include/fi_convt.h.
//
// Arithmetic: exact fp32 -- v_mfma_f32_32x32x2_f32 is bit-for-bit an fp32 fma chain (as conv_igemm.hip).
//
// With oy = 2 iy - 1 + r, ox = 2 ix - 1 + s the output splits into four parity classes, each a small stride-1
// correlation of x (weight w[ci][co][r][s], tap index 3 r + s; terms with h + 1 == H or w + 1 == W are zero):
//   y[2h  ][2w  ] = w4 x[h][w]
//   y[2h  ][2w+1] = w3 x[h][w+1] + w5 x[h][w]
//   y[2h+1][2w  ] = w1 x[h+1][w] + w7 x[h][w]
//   y[2h+1][2w+1] = w0 x[h+1][w+1] + w2 x[h+1][w] + w6 x[h][w+1] + w8 x[h][w]
// 9 tap products per 4 output pixels; the zero-stuffed form multiplies 9 per output pixel.
//
// One launch computes all four classes.  A workgroup of 4 wavefronts owns 4 rows x 16 columns of INPUT pixels (8 x 32
// output pixels) x 128 output channels, each wavefront 32 of the channels.  Per block of 16 input channels the
// (4+1) x (16+1) input patch -- the tile plus one halo row below and one halo column to the right -- is staged into LDS
// ONCE; the nine taps are nine (LDS offset, class accumulator) pairs.  Weights do not go through LDS: a lane loads the
// nine taps of (its output channel, one input channel) -- 36 contiguous bytes of the weight as torch stores it --
// straight into its MFMA A-operand registers (as conv3x3_patch_kernel of conv_igemm.hip does).  MFMA column
// n = l31 + 32 j is input pixel (row l31 / 8, column 2 (l31 % 8) + j) of the tile, so the two column tiles of a lane are
// NEIGHBOURING pixels: they share two of their three patch columns (6 LDS values per lane and channel pair feed 18
// MFMAs), and the lane ends up with output columns 4 (l31 % 8) .. + 3 of rows 2h and 2h + 1 for 16 channels -- written
// already interleaved, 16 bytes at a time (8 when W is odd), or as NHWC groups of 4 channels.
// Per wavefront and channel block: 144 MFMAs in 4 classes x 2 tiles = 128 accumulator registers per lane, against
// 24 weight loads, 6 patch loads, 6 LDS stores and ONE barrier per thread.  The patch of block t + 1 and the weights of
// channel pair k + 1 are requested before the MFMAs of block t / pair k.
//
// Bounds: a patch element outside the image is loaded from the clamped (last) row / column and replaced by zero on its
// way to LDS -- no address outside x is formed; weight rows past Cout re-read the last row and are never stored.
// Every output element is written exactly once by exactly one lane, its sum taken in a fixed channel order: no atomics,
// and the bits of an element do not depend on where its tile sits in the grid or the batch.
#include <stdint.h>

#include "fi_common.h"
#include "../../include/fi_convt.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4_v __attribute__((ext_vector_type(4)));
typedef f32x4_v f32x4_u __attribute__((aligned(4)));    // 16-byte load from a 4-byte aligned address

constexpr int kThreads = 256;
constexpr int BK = 16;                       // input channels per block
constexpr int BM = 128;                      // output channels per workgroup (4 wavefronts x 32)
constexpr int TH = 4, TW = 16;               // input pixels per workgroup
constexpr int PR = TH + 1, PC = TW + 1;      // patch rows / columns (tile + halo)
constexpr int PW = 18;                       // patch row pitch (even: the 8-byte reads of an even column are aligned)
constexpr int PP = PR * PW + 2;              // floats per channel
constexpr int ITEMS = BK * PR * PC;          // patch elements per channel block
constexpr int PER_THREAD = (ITEMS + kThreads - 1) / kThreads;
static_assert(PP % 2 == 0 && (TH - 1 + 1) * PW + (TW - 2) + 2 < PP, "patch pitch");

struct ConvtGeom {
    int N, Cin, H, W, Cout;
    int tiles_x, tiles_y, mtiles;
    int relu;
    int vec4;            // NCHW: W even -> a lane's 4 output columns are one aligned 16-byte store
};

template <bool ONHWC>
__global__ __launch_bounds__(kThreads, 2) void convt3x3s2_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                                 const float *__restrict__ bias,
                                                                 const float *__restrict__ scale, float *__restrict__ y,
                                                                 ConvtGeom g)
{
    __shared__ __attribute__((aligned(16))) float Ps[2][BK][PP];

    // Cout tiles innermost: the workgroups that share an input patch are neighbours in the launch order
    int pt = blockIdx.x / g.mtiles;
    const int mt = blockIdx.x - pt * g.mtiles;
    const int tx = pt % g.tiles_x;
    pt /= g.tiles_x;
    const int ty = pt % g.tiles_y;
    const int n = pt / g.tiles_y;
    const int h0 = ty * TH, w0 = tx * TW, m0 = mt * BM;
    const int HW = g.H * g.W;                                       // 16 * HW < 2^31 (launcher)

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, khalf = lane >> 5;

    // ---- patch staging: one element per item; outside the image: the clamped element, zero selected at the store ----
    int it_goff[PER_THREAD], it_lds[PER_THREAD];
    unsigned it_in = 0;
#pragma unroll
    for (int i = 0; i < PER_THREAD; ++i) {
        const int wi = tid + kThreads * i;
        const bool item = wi < ITEMS;
        const int wc = item ? wi : 0;
        const int ch = wc / (PR * PC);
        const int rem = wc - ch * (PR * PC);
        const int prow = rem / PC, pcol = rem - prow * PC;
        const int hh = h0 + prow, ww = w0 + pcol;
        if (item && hh < g.H && ww < g.W) it_in |= 1u << i;
        it_goff[i] = ch * HW + min(hh, g.H - 1) * g.W + min(ww, g.W - 1);
        // (a thread without an item stores to the channel's last pad float, which nothing reads: no branch around the
        // LDS stores, so the block loop stays ONE basic block and the loads keep their place ahead of the MFMAs)
        it_lds[i] = item ? ch * PP + prow * PW + pcol : PP - 1;
    }
    const float *__restrict__ xn = x + (size_t)n * g.Cin * HW;
    float preg[PER_THREAD];
    auto stage_load = [&](int cb) {
        const float *__restrict__ xb = xn + (size_t)cb * BK * HW;
#pragma unroll
        for (int i = 0; i < PER_THREAD; ++i) preg[i] = xb[it_goff[i]];
    };
    auto stage_store = [&](int buf) {
        float *__restrict__ pb = &Ps[buf][0][0];
#pragma unroll
        for (int i = 0; i < PER_THREAD; ++i)
            pb[it_lds[i]] = ((it_in >> i) & 1u) ? preg[i] : 0.0f;
    };

    // ---- A operand: the nine taps of (output channel, input channel), straight into registers ---------------------
    const int am = min(m0 + wave * 32 + l31, g.Cout - 1);           // rows past Cout re-read the last row
    const float *__restrict__ a_base = w + ((size_t)(khalf * 8) * g.Cout + am) * 9;
    const size_t a_step = (size_t)g.Cout * 9;                        // one input channel further
    auto load_a = [&](float (&a)[9], int cb, int kk) {
        const float *__restrict__ p = a_base + (size_t)(cb * BK + kk) * a_step;
        const f32x4_v v0 = *reinterpret_cast<const f32x4_u *>(p);
        const f32x4_v v1 = *reinterpret_cast<const f32x4_u *>(p + 4);
        a[0] = v0.x; a[1] = v0.y; a[2] = v0.z; a[3] = v0.w;
        a[4] = v1.x; a[5] = v1.y; a[6] = v1.z; a[7] = v1.w;
        a[8] = p[8];
    };

    // ---- B operand: rows h, h+1 x columns c, c+1, c+2 of the patch (c = the lane's even column) --------------------
    const int boff = (l31 >> 3) * PW + 2 * (l31 & 7);
    auto load_b = [&](float (&v)[6], const float *__restrict__ pbuf, int kk) {
        const float *__restrict__ p = pbuf + kk * PP + boff;
        const float2 r0 = *reinterpret_cast<const float2 *>(p);
        const float2 r1 = *reinterpret_cast<const float2 *>(p + PW);
        v[0] = r0.x; v[1] = r0.y; v[2] = p[2];
        v[3] = r1.x; v[4] = r1.y; v[5] = p[PW + 2];
    };

    f32x16 acc[4][2];                         // [class 2a + b: output (2h + a, 2w + b)][column tile j]
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[c][j][e] = 0.0f;

    const int ncb = g.Cin / BK;
    stage_load(0);
    stage_store(0);
    __syncthreads();

    float areg[2][9];
    float breg[2][6];
    load_a(areg[0], 0, 0);
    for (int cb = 0; cb < ncb; ++cb) {
        const float *__restrict__ pbuf = &Ps[cb & 1][0][0] + khalf * 8 * PP;
        const bool more = cb + 1 < ncb;
        const int cbn = more ? cb + 1 : cb;
        // unconditional (a branch would make the waits behind it count for the path without the loads): the last block
        // re-reads its own patch and drops it
        stage_load(cbn);
        load_b(breg[0], pbuf, 0);
        // issue order (the compiler otherwise folds the two register sets into one and requests the operands of pair
        // k + 1 behind the MFMAs of pair k that still read them): patch loads and the LDS reads of pair 0 first, then
        // per channel pair the 3 weight loads and 4 LDS reads of the NEXT pair ahead of the 18 MFMAs of this one
        __builtin_amdgcn_sched_group_barrier(0x020, PER_THREAD, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            const int cur = kk & 1, nxt = cur ^ 1;
            if (kk < 7) {
                load_a(areg[nxt], cb, kk + 1);
                load_b(breg[nxt], pbuf, kk + 1);
            } else {
                load_a(areg[nxt], cbn, 0);               // first channel pair of the next block
            }
            const float(&a)[9] = areg[cur];
            const float(&v)[6] = breg[cur];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float x00 = v[j], x01 = v[j + 1], x10 = v[3 + j], x11 = v[4 + j];
                acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4], x00, acc[0][j], 0, 0, 0);
                acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[3], x01, acc[1][j], 0, 0, 0);
                acc[2][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1], x10, acc[2][j], 0, 0, 0);
                acc[3][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], x11, acc[3][j], 0, 0, 0);
                acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[5], x00, acc[1][j], 0, 0, 0);
                acc[2][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[7], x00, acc[2][j], 0, 0, 0);
                acc[3][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2], x10, acc[3][j], 0, 0, 0);
                acc[3][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[6], x01, acc[3][j], 0, 0, 0);
                acc[3][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[8], x00, acc[3][j], 0, 0, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x020, 3, 0);
            if (kk < 7) __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 18, 0);
        }
        stage_store((cb + 1) & 1);                   // (last block: into the buffer nothing reads any more)
        __syncthreads();
    }

    // ---- epilogue: lane = 2 neighbouring input pixels x 4 classes x 16 channels (rows (e&3) + 8*(e>>2) + 4*khalf) ---
    const int hh = h0 + (l31 >> 3), wq = w0 + 2 * (l31 & 7);
    if (hh >= g.H || wq >= g.W) return;
    const bool two = wq + 1 < g.W;                                   // the lane's second pixel is inside the image
    const int mb = m0 + wave * 32 + 4 * khalf;
    const bool has_sc = scale != nullptr, has_bi = bias != nullptr, relu = g.relu != 0;
    const size_t OW = 2 * (size_t)g.W, OH = 2 * (size_t)g.H;
    auto fin = [&](float v, float sc, float bi) {
        v = has_sc ? v * sc : v;
        v = has_bi ? v + bi : v;
        return relu ? fmaxf(v, 0.0f) : v;
    };
    if (ONHWC) {
        // channels-last: accumulator rows (e & 3) are 4 consecutive channels of one pixel (Cout % 4 == 0)
        float *__restrict__ yp = y + (((size_t)n * OH + 2 * hh) * OW + 2 * wq) * g.Cout;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int co = mb + 8 * q;
            if (co >= g.Cout) continue;
            float sc[4], bi[4];
#pragma unroll
            for (int e4 = 0; e4 < 4; ++e4) {
                sc[e4] = has_sc ? scale[co + e4] : 1.0f;
                bi[e4] = has_bi ? bias[co + e4] : 0.0f;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if (j == 1 && !two) continue;
                    float t[4];
#pragma unroll
                    for (int e4 = 0; e4 < 4; ++e4) t[e4] = fin(acc[c][j][4 * q + e4], sc[e4], bi[e4]);
                    float *__restrict__ p = yp + ((size_t)(c >> 1) * OW + 2 * j + (c & 1)) * g.Cout + co;
                    *reinterpret_cast<float4 *>(p) = make_float4(t[0], t[1], t[2], t[3]);
                }
        }
        return;
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int co = mb + (e & 3) + 8 * (e >> 2);
        if (co >= g.Cout) continue;
        const float sc = has_sc ? scale[co] : 1.0f;
        const float bi = has_bi ? bias[co] : 0.0f;
        float *__restrict__ yp = y + (((size_t)n * g.Cout + co) * OH + 2 * hh) * OW + 2 * wq;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const float t0 = fin(acc[2 * a][0][e], sc, bi), t1 = fin(acc[2 * a + 1][0][e], sc, bi);
            const float t2 = fin(acc[2 * a][1][e], sc, bi), t3 = fin(acc[2 * a + 1][1][e], sc, bi);
            float *__restrict__ p = yp + a * OW;
            if (g.vec4) {
                *reinterpret_cast<float4 *>(p) = make_float4(t0, t1, t2, t3);
            } else {
                *reinterpret_cast<float2 *>(p) = make_float2(t0, t1);
                if (two) *reinterpret_cast<float2 *>(p + 2) = make_float2(t2, t3);
            }
        }
    }
}

// the sizes and alignments the kernel takes (the pointers may be NULL: not known yet)
bool convt_eligible(int N, int Cin, int H, int W, int Cout, int out_nhwc, const float *x, const float *y)
{
    if (N < 1 || Cin < 16 || Cin % 16 != 0 || Cout < 1 || H < 1 || W < 1) return false;
    if ((long)H * W > (1L << 26)) return false;                       // 16 channels of one image index with an int
    if (out_nhwc && Cout % 4 != 0) return false;
    if (((uintptr_t)x & 3) != 0 || ((uintptr_t)y & 15) != 0) return false;
    const long blocks = (long)N * fi::ceil_div(H, TH) * fi::ceil_div(W, TW) * fi::ceil_div(Cout, BM);
    return blocks <= 2147483647L;
}

}  // namespace

extern "C" {

int fi_conv_transpose3x3s2_eligible(int N, int Cin, int H, int W, int Cout, int out_nhwc, const float *x, const float *y)
{
    return convt_eligible(N, Cin, H, W, Cout, out_nhwc != 0, x, y) ? 1 : 0;
}

int fi_conv_transpose3x3s2_forward(const float *x, const float *weight, const float *bias, const float *scale, float *y,
                                   int N, int Cin, int H, int W, int Cout, int relu, int out_nhwc, fi_stream_t stream)
{
    FI_REQUIRE(N >= 0 && Cin >= 1 && Cout >= 1 && H >= 1 && W >= 1, "N >= 0, Cin, Cout, H, W >= 1");
    FI_REQUIRE(out_nhwc == 0 || out_nhwc == 1, "out_nhwc: 0 = y [N][Cout][2H][2W], 1 = y [N][2H][2W][Cout]");
    if (N == 0) return FI_OK;
    FI_REQUIRE(x && weight && y, "null pointer");
    if (!convt_eligible(N, Cin, H, W, Cout, out_nhwc, x, y)) {
        fi::set_error("fi_conv_transpose3x3s2_forward: unsupported call (N %d, Cin %d, H %d, W %d, Cout %d, out_nhwc %d, "
                      "x %p, y %p): needs Cin %% 16 == 0, y aligned to 16 bytes, Cout %% 4 == 0 for channels-last",
                      N, Cin, H, W, Cout, out_nhwc, (const void *)x, (const void *)y);
        return FI_ERR_UNSUPPORTED;
    }
    ConvtGeom g;
    g.N = N; g.Cin = Cin; g.H = H; g.W = W; g.Cout = Cout;
    g.tiles_x = fi::ceil_div(W, TW);
    g.tiles_y = fi::ceil_div(H, TH);
    g.mtiles = fi::ceil_div(Cout, BM);
    g.relu = relu ? 1 : 0;
    g.vec4 = (W % 2 == 0) ? 1 : 0;
    const unsigned blocks = (unsigned)((long)N * g.tiles_x * g.tiles_y * g.mtiles);
    hipStream_t st = (hipStream_t)stream;
    if (out_nhwc)
        hipLaunchKernelGGL(convt3x3s2_kernel<true>, dim3(blocks), dim3(kThreads), 0, st, x, weight, bias, scale, y, g);
    else
        hipLaunchKernelGGL(convt3x3s2_kernel<false>, dim3(blocks), dim3(kThreads), 0, st, x, weight, bias, scale, y, g);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

}  // extern "C"
