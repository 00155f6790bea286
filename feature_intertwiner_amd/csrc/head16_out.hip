// head16_out.hip -- libfi_head16.so (include/fi_head16.h): the heads' 1x1 output layer, 16-bit rows in, fp32 out, for any
// number of output channels: the box head's stacked class + box linears (405 columns) and the mask head's conv5 with its
// sigmoid and the 2 x 2 pixel shuffle (81 channels).  head16_out_f16.hip includes this file with FI_E16_HALF defined: the
// same kernel on IEEE half under the *_f16 name.
//
// A 1x1 / stride 1 convolution on the main loop of conv_act16_dev.h (tiles, swizzled LDS, summation order: see there) on
// 64-row channel tiles, as pyr16_head_kernel (conv_pyr16.hip), whose Cout <= 64 it lifts: the channel tiles are the fast
// index of the grid, so the workgroups that read one pixel tile of x run together and HBM sees it once.  The fp32 tile goes
// to LDS the shared way; what is this kernel's own is the epilogue, one float per lane and store instruction:
// Rows.     y[p, co]: the tile's floats are mc = min(64, Cout - m0) contiguous channels of each of its pixels; the walk is
//           flat over (pixel, channel), neighbouring lanes on neighbouring channels.
// Shuffle.  Row p = ((i * H + h) * W + w) * 4 + 2a + b of x belongs at y[i, co, 2h + a, 2w + b].  The 4W rows of one (i, h)
//           are two output rows of 2W floats per channel.  A lane takes one slot ((i, h) group, a, 2w + b) -- one position
//           of the output plane -- and walks the tile's channels, 4 per 16-byte LDS read: neighbouring lanes write
//           neighbouring floats of an output row, runs of 2W floats, and the slot's divisions are done once.  A pixel tile
//           of 128 rows starts and ends inside a group (it crosses output rows and images), so the slots cover every group
//           the tile touches and those whose row is another tile's idle: up to 8W lanes, none at W = 1, 43 % at W = 14.
//           Meant for the small maps of the heads; the host refuses W > 65536.
//           The first form walked flat over (channel, slot) with four integer divisions and a 4-byte LDS read per float
//           (the swizzle spreads 16 pixels of one channel over 8 slots of 16 bytes: conflicts) and lost to the launches it replaces;
//           DESIGN section 5 has both figures.  With K = 256 the main loop is four K blocks long: the launch is bound by this epilogue.
// Sigmoid: 1 / (1 + exp(-v)) in fp32 with the library's expf and an IEEE division; exp overflows to +inf for v < -88.7 and
// the quotient is then exactly 0, so the result stays within [0, 1] for every finite v.
#include <stdint.h>

#include "fi_common.h"
#include "conv_act16_dev.h"
#include "../../include/fi_head16.h"

namespace {

constexpr int OBM = 64;           // the channel tile: pyr16_head_kernel's
constexpr int kMaxShuffleW = 65536;

__device__ __forceinline__ float finish(float v, const float *__restrict__ bias, int co, int act)
{
    if (bias) v = v + bias[co];
    if (act) v = 1.0f / (1.0f + expf(-v));
    return v;
}

template <int BK, int LAYOUT>
__global__ __launch_bounds__(kThreads) void head16_out_kernel(const E16 *__restrict__ x, const E16 *__restrict__ w,
                                                              const float *__restrict__ bias, float *__restrict__ y, Geom g,
                                                              int act, int H, int W)
{
    __shared__ u32x4 smem[tile_smem_chunks<OBM, BK>()];
    const int tid = threadIdx.x;
    const int m0 = (int)(blockIdx.x % (unsigned)g.mtiles) * OBM;
    const int n0 = (int)(blockIdx.x / (unsigned)g.mtiles) * BN;          // < P < 2^31 (host check)
    f32x16 acc[1][2];
    conv_main_loop<OBM, BK>(x, w, g, smem, m0, n0, acc);

    constexpr int RC = OBM / 4;
    tile_to_lds<OBM>(acc, reinterpret_cast<f32x4 *>(smem));
    const float *Cf = reinterpret_cast<const float *>(smem);
    const int np = min(BN, g.P - n0);               // pixels and channels of this tile
    const int mc = min(OBM, g.Cout - m0);
    if (LAYOUT == 0) {
        float *__restrict__ run = y + (long)n0 * g.Cout + m0;
        const int total = np * mc;
        for (int e = tid; e < total; e += kThreads) {
            const int pr = e / mc, c = e - pr * mc;
            const float v = Cf[(pr * RC + ((c >> 2) ^ (pr & 15))) * 4 + (c & 3)];
            run[(long)pr * g.Cout + c] = finish(v, bias, m0 + c, act);
        }
    } else {
        const int G = 4 * W, W2 = 2 * W;            // rows of x per (image, h) group; floats per output row
        const int q0 = n0 / G;
        const int slots = ((n0 + np - 1) / G - q0 + 1) * G;          // <= 128 + 2 G: fits (host check on W)
        const f32x4 *Cs = reinterpret_cast<const f32x4 *>(smem);
        const long plane = (long)(2 * H) * W2;      // floats of one (image, channel) of y
        // a lane keeps its slot -- one output position -- and walks the tile's channels: the index arithmetic is done once
        // per slot, the tile is read 16 bytes (4 channels) at a time, and each of the 4 stores of a wavefront covers
        // neighbouring floats of output rows
        for (int s = tid; s < slots; s += kThreads) {
            const int qi = s / G, r = s - qi * G;
            const int a = r / W2, wb = r - a * W2;
            const int q = q0 + qi;
            const int pr = q * G + (wb >> 1) * 4 + 2 * a + (wb & 1) - n0;      // q * G + ... <= P
            if (pr < 0 || pr >= np) continue;       // the row is another tile's
            const int i = q / H, hh = q - i * H;
            float *__restrict__ dst = y + ((long)i * g.Cout + m0) * plane + (long)(2 * hh + a) * W2 + wb;
            for (int c4 = 0; c4 * 4 < mc; ++c4) {
                const f32x4 v = Cs[pr * RC + (c4 ^ (pr & 15))];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = c4 * 4 + j;
                    if (c < mc) dst[(long)c * plane] = finish(v[j], bias, m0 + c, act);
                }
            }
        }
    }
}

#ifndef FI_E16_HALF
// THE statement of what the kernel takes (the pointers may be NULL: not known yet): head_eligible's limits
// (conv_pyr16.hip) without its Cout <= 64, with the tile count over both grid axes, and the switches
bool out_eligible(int P, int Cin, int Cout, int act, int layout, int n, int H, int W, const void *x, const void *w,
                  const void *y)
{
    if (P < 1 || Cin < 32 || Cin % 32 != 0 || Cout < 1) return false;
    if ((act != 0 && act != 1) || (layout != 0 && layout != 1)) return false;
    if ((((uintptr_t)x | (uintptr_t)w) & 15) != 0 || ((uintptr_t)y & 3) != 0) return false;
    if (layout == 1) {
        if (n < 1 || H < 1 || W < 1 || W > kMaxShuffleW) return false;
        long rows = (long)n * H;                    // < 2^62; each further product is compared before the next
        if (rows > P) return false;
        rows *= W;
        if (rows > P) return false;
        if (rows * 4 != P) return false;
    }
    const long blocks = (((long)P + BN - 1) / BN) * (((long)Cout + OBM - 1) / OBM);
    return (long)Cout * Cin <= kIntMax && blocks <= kIntMax;
}
#endif

}  // namespace

extern "C" {

#ifndef FI_E16_HALF
int fi_head16_out1x1_eligible(int P, int Cin, int Cout, int act, int layout, int n, int H, int W, const void *x,
                              const void *w, const void *y)
{
    return out_eligible(P, Cin, Cout, act, layout, n, H, W, x, w, y) ? 1 : 0;
}
#endif

int FI16(fi_head16_out1x1)(const void *x, const void *w, const float *bias, float *y, int P, int Cin, int Cout, int act,
                           int layout, int n, int H, int W, fi_stream_t stream)
{
    FI_REQUIRE(P >= 0 && Cin >= 1 && Cout >= 1, "P >= 0, Cin, Cout >= 1");
    if (P == 0) return FI_OK;
    FI_REQUIRE(x && w && y, "null pointer");
    if (fi_head16_out1x1_eligible(P, Cin, Cout, act, layout, n, H, W, x, w, y) != 1) {
        fi::set_error("fi_head16_out1x1: unsupported call (P %d, Cin %d, Cout %d, act %d, layout %d, n %d, H %d, W %d, x %p, "
                      "w %p, y %p): needs Cin %% 32 == 0, act and layout 0 or 1, x and w aligned to 16 bytes, y to 4, extents "
                      "and the grid below 2^31, and with layout 1 P == n * H * W * 4 and W <= %d",
                      P, Cin, Cout, act, layout, n, H, W, x, w, (const void *)y, kMaxShuffleW);
        return FI_ERR_UNSUPPORTED;
    }
    Geom g;
    g.N = 1; g.H = 1; g.W = P; g.Cin = Cin; g.Cout = Cout; g.RS = 1; g.S = 1; g.stride = 1; g.pad = 0;
    g.OH = 1;
    g.OW = P;
    g.P = P;
    g.mtiles = fi::ceil_div(Cout, OBM);
    g.relu = 0;
    const unsigned blocks = (unsigned)((long)fi::ceil_div(P, BN) * g.mtiles);
    hipStream_t st = (hipStream_t)stream;
    const E16 *xe = (const E16 *)x, *we = (const E16 *)w;
#define FI_HEAD16_LAUNCH(BK_, LAYOUT_) \
    hipLaunchKernelGGL((head16_out_kernel<BK_, LAYOUT_>), dim3(blocks), dim3(kThreads), 0, st, xe, we, bias, y, g, act, H, W)
    if (layout == 0) {
        if (Cin % 64 == 0) FI_HEAD16_LAUNCH(64, 0); else FI_HEAD16_LAUNCH(32, 0);
    } else {
        if (Cin % 64 == 0) FI_HEAD16_LAUNCH(64, 1); else FI_HEAD16_LAUNCH(32, 1);
    }
#undef FI_HEAD16_LAUNCH
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

}  // extern "C"
