// fpn16.hip -- libfi_fpn16.so (include/fi_fpn16.h): the backward of the feature pyramid's top-down step on 16-bit
// channels-last tensors.  The forward (fi_pyr16_lateral) adds the coarser level read at half resolution: coarse pixel
// (h, w) is read by the four fine pixels (2h + i, 2w + j).  Its backward into the coarse level is therefore the sum of the
// 2 x 2 cell of the fine gradient, added to the coarse level's own gradient, rounded once -- and the per-channel sums of the
// result, which are the bias gradient of the layer that produced the coarse level.  One launch.  fpn16_f16.hip includes
// this file with FI_E16_HALF defined: the same kernel on IEEE half under the *_f16 name.
//
// HBM bound: per lane of 8 channels five 16-byte loads and one 16-byte store, no reuse.  The lanes run along the channels:
// the two fine pixels of a row of the cell are neighbours in memory, so the lanes of a pixel read 2 C 16-bit values at a
// stretch, twice.  A thread keeps its 8 channels for all its rows and sums the values AS STORED in 8 fp32 registers; the
// threads of a workgroup combine in LDS (ds_add_f32), the workgroup adds one value per channel with a global fp32 atomic
// -- relu_grad_kernel's scheme (conv_grad16.hip).  A workgroup takes FP_CH channels (its sums are 8 KB of LDS) and `rows`
// coarse pixels; the host sizes `rows` (a multiple of the rows one pass of the threads covers, at most FP_ROWS) so that a
// level of a few thousand pixels still gives every compute unit a workgroup and a large one does not send thousands of
// workgroups to the same C atomic addresses.
#include <stdint.h>

#include "fi_common.h"
#include "conv_act16_dev.h"
#include "../../include/fi_fpn16.h"

namespace {

constexpr int FP_ROWS = 512;      // most coarse pixels of a workgroup
constexpr int FP_CH = 2048;       // channels of a workgroup (its column sums live in LDS)
// row groups aimed at: two per compute unit with a fine operand (five loads per lane and pixel), one without (one load:
// every workgroup ends with one atomic per channel on the same C addresses, and those then weigh more than the reads)
constexpr long FP_GROUPS_FINE = 2 * kCUs, FP_GROUPS_OWN = kCUs;

// own / g: [P][C], fine: [P / W][2][2 W][C] -- image n, row h flatten to t = n H + h, the fine rows of t are 2 t and 2 t + 1
__global__ __launch_bounds__(kThreads) void topdown_grad_kernel(const E16 *own, const E16 *__restrict__ fine, E16 *g,
                                                                float *__restrict__ colsum, int P, int W, int C, int rows,
                                                                int ctiles, int store)
{
    __shared__ float sums[FP_CH];
    const int tid = threadIdx.x;
    const int c_base = (int)(blockIdx.x % (unsigned)ctiles) * FP_CH;
    const int cw = C - c_base < FP_CH ? C - c_base : FP_CH;            // % 8 == 0
    const int C8 = cw / 8;
    if (colsum) {
        for (int c = tid; c < cw; c += kThreads) sums[c] = 0.f;
        __syncthreads();
    }
    // a thread keeps its 8 channels: lanes_c threads across a pixel, rstep pixels at a time
    const int lanes_c = C8 < kThreads ? C8 : kThreads;
    const int rstep = kThreads / lanes_c;
    const long row0 = (long)(blockIdx.x / (unsigned)ctiles) * rows;
    const long row_end = row0 + rows < P ? row0 + rows : (long)P;
    if (tid < lanes_c * rstep) {
        for (int cg = tid % lanes_c; cg < C8; cg += lanes_c) {
            float acc[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = 0.f;
            const int c = c_base + cg * 8;
            for (long row = row0 + tid / lanes_c; row < row_end; row += rstep) {
                const long o = row * C + c;
                float v[8];
                if (fine) {
                    const int t = (int)(row / W), w = (int)(row - (long)t * W);
                    const long p00 = (4L * t * W + 2L * w) * C + c;        // fine pixel (2 t, 2 w); its row is 2 W pixels
                    const long p10 = p00 + 2L * W * C;
                    const e16x8 f00 = *reinterpret_cast<const e16x8 *>(fine + p00);
                    const e16x8 f01 = *reinterpret_cast<const e16x8 *>(fine + p00 + C);
                    const e16x8 f10 = *reinterpret_cast<const e16x8 *>(fine + p10);
                    const e16x8 f11 = *reinterpret_cast<const e16x8 *>(fine + p10 + C);
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = ((float)f00[j] + (float)f01[j]) + ((float)f10[j] + (float)f11[j]);
                    if (own) {
                        const e16x8 a = *reinterpret_cast<const e16x8 *>(own + o);
#pragma unroll
                        for (int j = 0; j < 8; ++j) v[j] = (float)a[j] + v[j];
                    }
                } else {
                    const e16x8 a = *reinterpret_cast<const e16x8 *>(own + o);
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = (float)a[j];
                }
                e16x8 out;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    out[j] = (E16)v[j];                                 // the one rounding
                    acc[j] += (float)out[j];
                }
                if (store) *reinterpret_cast<e16x8 *>(g + o) = out;
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

// coarse pixels of a workgroup: a whole number of passes of its threads, `groups` row groups when the map allows
int rows_per_group(long P, int C, long groups)
{
    const int cw = C < FP_CH ? C : FP_CH;
    const int lanes_c = cw / 8 < kThreads ? cw / 8 : kThreads;
    const int rstep = kThreads / lanes_c;
    long rows = (P + groups - 1) / groups;
    rows = (rows + rstep - 1) / rstep * rstep;
    if (rows < 2L * rstep) rows = 2L * rstep;
    if (rows > FP_ROWS) rows = FP_ROWS;                 // C < 32: fewer rows than one pass, the threads past them idle
    return (int)rows;
}

// THE statement of what the entry points take (the pointers may be NULL: absent or not known yet)
bool fpn_eligible(int N, int H, int W, int C, const void *own, const void *fine, const void *g, const void *colsum)
{
    if (N < 1 || H < 1 || W < 1 || C < 8 || C % 8 != 0) return false;
    if ((((uintptr_t)own | (uintptr_t)fine | (uintptr_t)g) & 15) != 0 || ((uintptr_t)colsum & 3) != 0) return false;
    const long P = (long)N * H * W;
    if (4 * P > kIntMax) return false;                  // N * 2H * 2W
    const int rows = rows_per_group(P, C, FP_GROUPS_FINE);         // the smaller groups: the larger count
    return ((P + rows - 1) / rows) * fi::ceil_div(C, FP_CH) <= kIntMax;
}

}  // namespace

extern "C" {

#ifndef FI_E16_HALF
int fi_fpn16_eligible(int N, int H, int W, int C, const void *own, const void *fine, const void *g, const void *colsum)
{
    return fpn_eligible(N, H, W, C, own, fine, g, colsum) ? 1 : 0;
}
#endif

int FI16(fi_fpn16_topdown_grad)(const void *own, const void *fine, void *g, float *colsum, int N, int H, int W, int C,
                                fi_stream_t stream)
{
    FI_REQUIRE(N >= 0 && H >= 1 && W >= 1 && C >= 1, "N >= 0, H, W, C >= 1");
    if (N == 0) return FI_OK;
    FI_REQUIRE(g, "null pointer");
    FI_REQUIRE(own || fine, "own and fine are both null");
    if (!fpn_eligible(N, H, W, C, own, fine, g, colsum)) {
        fi::set_error("fi_fpn16_topdown_grad: unsupported call (N %d, H %d, W %d, C %d, own %p, fine %p, g %p, colsum %p): "
                      "needs C %% 8 == 0, the 16-bit tensors aligned to 16 bytes, colsum to 4, N*2H*2W and the workgroup "
                      "count below 2^31", N, H, W, C, own, fine, (const void *)g, (const void *)colsum);
        return FI_ERR_UNSUPPORTED;
    }
    const int P = N * H * W;
    const int rows = rows_per_group(P, C, fine ? FP_GROUPS_FINE : FP_GROUPS_OWN);
    const int ctiles = fi::ceil_div(C, FP_CH);
    const unsigned blocks = (unsigned)((long)fi::ceil_div(P, rows) * ctiles);
    const int store = (fine == nullptr && g == own) ? 0 : 1;       // nothing to change: a read-only column-sum pass
    hipStream_t st = (hipStream_t)stream;
    if (colsum) FI_HIP_CHECK(hipMemsetAsync(colsum, 0, sizeof(float) * (size_t)C, st));
    hipLaunchKernelGGL(topdown_grad_kernel, dim3(blocks), dim3(kThreads), 0, st, (const E16 *)own, (const E16 *)fine,
                       (E16 *)g, colsum, P, W, C, rows, ctiles, store);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

}  // extern "C"
