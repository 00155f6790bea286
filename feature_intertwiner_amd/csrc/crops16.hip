// crops16.hip -- libfi_crops16.so (include/fi_crops16.h): the three memory-bound launches between the 16-bit feature
// pyramid of a train step and its fp32 RoI crops.  crops16_f16.hip includes this file with FI_E16_HALF defined: the same
// kernels on IEEE half under the *_f16 names.
//
// Patch rows, forward.  One workgroup per row; its 9 x C/8 (tap, 8 channels) items go round the threads, so the 32 lanes
// of a 256-channel tap read 512 contiguous bytes and write 1 KB.  (The fp32 NCHW gather reads 256 strided values.)
// Patch rows, backward.  The gradient maps are 16-bit, so adding with atomics is out, and a dense fp32 map is what the
// launch is there to avoid.  One workgroup per (row, tap) owns the tap's pixel: it walks the row list, 256 rows at a time,
// for every row with a tap on the same pixel of the same tensor and image -- a row has at most one such tap, so ascending
// rows ARE ascending (row, tap) -- and adds their d in that order; the moment the FIRST match turns out not to be the
// workgroup's own (row, tap) it leaves: that earlier workgroup writes the pixel.  The survivor adds the old value last and
// stores once.  Matches are compared in tensor pixels, so a level that is the step-2 subsample of another level's tensor
// meets that level's rows.
// Gate-pack.  relu_grad_kernel (conv_grad16.hip) reading fp32 instead of 16-bit gradients: a thread keeps its 8 channels
// for all its pixels and sums the values AS STORED in 8 fp32 registers; the threads of a workgroup combine in LDS, the
// workgroup adds one value per channel with a global fp32 atomic.  The host sizes the pixels of a workgroup as the
// top-down kernel of the pyramid's backward does (two row groups per compute unit, at most GP_ROWS).
#include <stdint.h>

#include "fi_common.h"
#include "conv_act16_dev.h"
#include "../../include/fi_crops16.h"

namespace {

constexpr int kLevelsMax = 8;
constexpr long kPatchRowsMax = 1L << 20;      // rows of a patch launch (its backward is quadratic in them)
constexpr int GP_ROWS = 512;                  // most pixels of a gate-pack workgroup
constexpr int GP_CH = 2048;                   // channels of a gate-pack workgroup (its column sums live in LDS)
constexpr long GP_GROUPS = 2 * kCUs;          // row groups aimed at

struct Levels16 {
    E16 *base[kLevelsMax];                    // the tensor behind the level
    int TH[kLevelsMax], TW[kLevelsMax];       // its size
    int H[kLevelsMax], W[kLevelsMax];         // the level: ceil(T / step)
    int step[kLevelsMax];
    long start[kLevelsMax];                   // first anchor of the level
    int levels, per_loc, N;
};

// level and level pixel of row (img, a); false for a padding row
__device__ __forceinline__ bool locate(const Levels16 &lv, long img, long a, int &l, int &h, int &w)
{
    if (img < 0 || img >= lv.N || a < 0) return false;
    l = 0;
    while (l + 1 < lv.levels && a >= lv.start[l + 1]) ++l;
    const long pix = (a - lv.start[l]) / lv.per_loc;
    if (pix >= (long)lv.H[l] * lv.W[l]) return false;
    h = (int)(pix / lv.W[l]);
    w = (int)(pix - (long)h * lv.W[l]);
    return true;
}

__global__ __launch_bounds__(kThreads) void patch_fwd_kernel(Levels16 lv, const long *__restrict__ image,
                                                             const long *__restrict__ anchor, float *__restrict__ out, int C)
{
    const long r = blockIdx.x;
    const long img = image[r];
    int l = 0, h = 0, w = 0;
    const bool ok = locate(lv, img, anchor[r], l, h, w);
    const int C8 = C / 8;
    const int items = 9 * C8;
    float *__restrict__ o = out + r * 9 * (long)C;
    for (int it = threadIdx.x; it < items; it += kThreads) {
        const int tap = it / C8, cg = it - tap * C8;
        f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
        if (ok) {
            const int hh = h + tap / 3 - 1, ww = w + tap % 3 - 1;
            if (hh >= 0 && hh < lv.H[l] && ww >= 0 && ww < lv.W[l]) {
                // hh < ceil(TH / step): hh * step < TH, the tensor pixel exists
                const long pix = (img * lv.TH[l] + (long)hh * lv.step[l]) * lv.TW[l] + (long)ww * lv.step[l];
                const e16x8 v = *reinterpret_cast<const e16x8 *>(lv.base[l] + pix * C + cg * 8);
                lo = f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
                hi = f32x4{(float)v[4], (float)v[5], (float)v[6], (float)v[7]};
            }
        }
        f32x4 *dst = reinterpret_cast<f32x4 *>(o + (long)tap * C + cg * 8);
        dst[0] = lo;
        dst[1] = hi;
    }
}

// tap offset -1 / 0 / 1 of a row whose centre is `delta` tensor pixels from the target on a level of stride s; 2: none
__device__ __forceinline__ int tap_of(int delta, int s)
{
    return delta == 0 ? 0 : delta == s ? 1 : delta == -s ? -1 : 2;
}

__global__ __launch_bounds__(kThreads) void patch_bwd_kernel(Levels16 lv, const long *__restrict__ image,
                                                             const long *__restrict__ anchor, const float *__restrict__ d,
                                                             int rows, int C)
{
    __shared__ unsigned long long s_mask[kThreads / 64];
    __shared__ signed char s_tap[kThreads];
    const int tid = threadIdx.x;
    const int r = (int)blockIdx.x, tap = (int)blockIdx.y;
    const long img = image[r];
    int l = 0, h = 0, w = 0;
    if (!locate(lv, img, anchor[r], l, h, w)) return;                 // (uniform: the whole workgroup leaves)
    const int hh = h + tap / 3 - 1, ww = w + tap % 3 - 1;
    if (hh < 0 || hh >= lv.H[l] || ww < 0 || ww >= lv.W[l]) return;
    E16 *const base = lv.base[l];
    const int y = hh * lv.step[l], x = ww * lv.step[l];               // the tensor pixel this workgroup owns: y < TH, x < TW
    const long own = (long)r * 9 + tap;
    const int c = ((int)blockIdx.z * kThreads + tid) * 8;
    const bool lane_on = c < C;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    bool seen = false;                                                // the first match was met (and was this workgroup's)
    for (int r0 = 0; r0 < rows; r0 += kThreads) {
        const int rr = r0 + tid;
        int t2 = -1;
        if (rr < rows && image[rr] == img) {
            int l2 = 0, h2 = 0, w2 = 0;
            if (locate(lv, img, anchor[rr], l2, h2, w2) && lv.base[l2] == base) {
                const int s2 = lv.step[l2];
                // tap (ty, tx) of rr is tensor pixel ((h2 + ty) s2, (w2 + tx) s2); (y, x) lies inside the tensor, so a tap that
                // lands on it lies inside rr's level
                const int ty = tap_of(y - h2 * s2, s2), tx = tap_of(x - w2 * s2, s2);
                if (ty != 2 && tx != 2) t2 = (ty + 1) * 3 + tx + 1;
            }
        }
        const unsigned long long m = __ballot(t2 >= 0);
        s_tap[tid] = (signed char)t2;
        if ((tid & 63) == 0) s_mask[tid >> 6] = m;
        __syncthreads();
        for (int wv = 0; wv < kThreads / 64; ++wv) {
            unsigned long long mm = s_mask[wv];
            while (mm) {
                const int j = wv * 64 + __builtin_ctzll(mm);
                mm &= mm - 1;
                const long k2 = (long)(r0 + j) * 9 + s_tap[j];
                if (!seen) {
                    if (k2 != own) return;                            // an earlier (row, tap) owns the pixel (uniform)
                    seen = true;
                }
                if (lane_on) {
                    const f32x4 *src = reinterpret_cast<const f32x4 *>(d + k2 * C + c);
                    const f32x4 lo = src[0], hi = src[1];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        acc[q] += lo[q];
                        acc[4 + q] += hi[q];
                    }
                }
            }
        }
        __syncthreads();
    }
    if (!lane_on) return;
    E16 *dst = base + ((img * lv.TH[l] + y) * lv.TW[l] + x) * C + c;
    const e16x8 old = *reinterpret_cast<const e16x8 *>(dst);
    e16x8 out;
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = (E16)((float)old[j] + acc[j]);     // the one rounding
    *reinterpret_cast<e16x8 *>(dst) = out;
}

// d: [P][C] fp32, y / g: [P][C] 16-bit
__global__ __launch_bounds__(kThreads) void gate_pack_kernel(const float *__restrict__ d, const E16 *__restrict__ y,
                                                             E16 *__restrict__ g, float *__restrict__ colsum, int P, int C,
                                                             int rows, int ctiles)
{
    __shared__ float sums[GP_CH];
    const int tid = threadIdx.x;
    const int c_base = (int)(blockIdx.x % (unsigned)ctiles) * GP_CH;
    const int cw = C - c_base < GP_CH ? C - c_base : GP_CH;            // % 8 == 0
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
            for (long row = row0 + tid / lanes_c; row < row_end; row += rstep) {
                const long o = row * C + c_base + cg * 8;
                const f32x4 lo = *reinterpret_cast<const f32x4 *>(d + o);
                const f32x4 hi = *reinterpret_cast<const f32x4 *>(d + o + 4);
                e16x8 out;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    out[j] = (E16)lo[j];                               // the one rounding
                    out[4 + j] = (E16)hi[j];
                }
                if (y) {
                    const e16x8 yy = *reinterpret_cast<const e16x8 *>(y + o);
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (!((float)yy[j] > 0.f)) out[j] = (E16)0.f;
                }
                *reinterpret_cast<e16x8 *>(g + o) = out;
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += (float)out[j];
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

// pixels of a gate-pack workgroup: a whole number of passes of its threads, GP_GROUPS row groups when the map allows
int rows_per_group(long P, int C)
{
    const int cw = C < GP_CH ? C : GP_CH;
    const int lanes_c = cw / 8 < kThreads ? cw / 8 : kThreads;
    const int rstep = kThreads / lanes_c;
    long rows = (P + GP_GROUPS - 1) / GP_GROUPS;
    rows = (rows + rstep - 1) / rstep * rstep;
    if (rows < 2L * rstep) rows = 2L * rstep;
    if (rows > GP_ROWS) rows = GP_ROWS;                 // C < 32: fewer rows than one pass, the threads past them idle
    return (int)rows;
}

// THE statement of what the entry points take (the pointers may be NULL: absent or not known yet)
bool crops_eligible(int kind, int levels, int C, long n, const void *const *level_ptrs, const void *p0, const void *p1,
                    const void *p2, const void *p3)
{
    if (C < 8 || C % 8 != 0 || n < 1 || n > kIntMax) return false;
    if (kind == FI_CROPS16_PATCH_FWD || kind == FI_CROPS16_PATCH_BWD) {
        if (levels < 1 || levels > kLevelsMax || n > kPatchRowsMax) return false;
        if (level_ptrs)
            for (int l = 0; l < levels; ++l)
                if (((uintptr_t)level_ptrs[l] & 15) != 0) return false;
        if (((uintptr_t)p0 & 15) != 0) return false;
        return fi::ceil_div(C, 8 * kThreads) <= 65535;              // the channel tiles of the backward: grid z
    }
    if (kind == FI_CROPS16_GATE_PACK) {
        if ((((uintptr_t)p0 | (uintptr_t)p1 | (uintptr_t)p2) & 15) != 0 || ((uintptr_t)p3 & 3) != 0) return false;
        const int rows = rows_per_group(n, C);
        return ((n + rows - 1) / rows) * fi::ceil_div(C, GP_CH) <= kIntMax;
    }
    return false;
}

// the level table of a patch launch; `ptrs` are the maps (forward) or the gradient maps (backward)
int make_levels(Levels16 &lv, const void *const *ptrs, const int *heights, const int *widths, const int *steps, int levels,
                int per_loc, int N)
{
    FI_REQUIRE(levels >= 1 && levels <= kLevelsMax, "1..8 pyramid levels");
    long start = 0;
    for (int l = 0; l < levels; ++l) {
        const int step = steps ? steps[l] : 1;
        FI_REQUIRE(heights[l] >= 1 && widths[l] >= 1 && step >= 1, "bad map size or step");
        FI_REQUIRE(ptrs[l], "null level map");
        for (int k = 0; k < l; ++k)
            FI_REQUIRE(ptrs[k] != ptrs[l] || (heights[k] == heights[l] && widths[k] == widths[l]),
                       "two levels share a tensor but not its size");
        lv.base[l] = static_cast<E16 *>(const_cast<void *>(ptrs[l]));
        lv.TH[l] = heights[l];
        lv.TW[l] = widths[l];
        lv.H[l] = (heights[l] + step - 1) / step;
        lv.W[l] = (widths[l] + step - 1) / step;
        lv.step[l] = step;
        lv.start[l] = start;
        start += (long)lv.H[l] * lv.W[l] * per_loc;
    }
    lv.levels = levels;
    lv.per_loc = per_loc;
    lv.N = N;
    return FI_OK;
}

}  // namespace

extern "C" {

#ifndef FI_E16_HALF
int fi_crops16_eligible(int kind, int levels, int C, int n, const void *const *level_ptrs, const void *p0, const void *p1,
                        const void *p2, const void *p3)
{
    return crops_eligible(kind, levels, C, n, level_ptrs, p0, p1, p2, p3) ? 1 : 0;
}
#endif

int FI16(fi_crops16_patch_rows_forward)(const void *const *maps, const int *heights, const int *widths, const int *steps,
                                        int levels, int anchors_per_location, const int64_t *image, const int64_t *anchor,
                                        int rows, int N, int C, float *out, fi_stream_t stream)
{
    FI_REQUIRE(rows >= 0 && N >= 1 && C >= 1 && anchors_per_location >= 1, "rows >= 0, N, C, anchors_per_location >= 1");
    if (rows == 0) return FI_OK;
    FI_REQUIRE(maps && heights && widths && image && anchor && out, "null pointer");
    Levels16 lv = {};
    const int rc = make_levels(lv, maps, heights, widths, steps, levels, anchors_per_location, N);
    if (rc != FI_OK) return rc;
    if (!crops_eligible(FI_CROPS16_PATCH_FWD, levels, C, rows, maps, out, nullptr, nullptr, nullptr)) {
        fi::set_error("fi_crops16_patch_rows_forward: unsupported call (%d levels, C %d, %d rows, out %p): needs C %% 8 == 0, "
                      "the maps and out aligned to 16 bytes, at most 2^20 rows", levels, C, rows, (const void *)out);
        return FI_ERR_UNSUPPORTED;
    }
    hipLaunchKernelGGL(patch_fwd_kernel, dim3((unsigned)rows), dim3(kThreads), 0, (hipStream_t)stream, lv,
                       reinterpret_cast<const long *>(image), reinterpret_cast<const long *>(anchor), out, C);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int FI16(fi_crops16_patch_rows_backward)(const float *d, void *const *grads, const int *heights, const int *widths,
                                         const int *steps, int levels, int anchors_per_location, const int64_t *image,
                                         const int64_t *anchor, int rows, int N, int C, fi_stream_t stream)
{
    FI_REQUIRE(rows >= 0 && N >= 1 && C >= 1 && anchors_per_location >= 1, "rows >= 0, N, C, anchors_per_location >= 1");
    if (rows == 0) return FI_OK;
    FI_REQUIRE(d && grads && heights && widths && image && anchor, "null pointer");
    Levels16 lv = {};
    const int rc = make_levels(lv, grads, heights, widths, steps, levels, anchors_per_location, N);
    if (rc != FI_OK) return rc;
    if (!crops_eligible(FI_CROPS16_PATCH_BWD, levels, C, rows, grads, d, nullptr, nullptr, nullptr)) {
        fi::set_error("fi_crops16_patch_rows_backward: unsupported call (%d levels, C %d, %d rows, d %p): needs C %% 8 == 0, "
                      "the gradient maps and d aligned to 16 bytes, at most 2^20 rows", levels, C, rows, (const void *)d);
        return FI_ERR_UNSUPPORTED;
    }
    hipLaunchKernelGGL(patch_bwd_kernel, dim3((unsigned)rows, 9, (unsigned)fi::ceil_div(C, 8 * kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, lv, reinterpret_cast<const long *>(image),
                       reinterpret_cast<const long *>(anchor), d, rows, C);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int FI16(fi_crops16_gate_pack)(const float *d, const void *y, void *g, float *sums, int N, int H, int W, int C,
                               fi_stream_t stream)
{
    FI_REQUIRE(N >= 0 && H >= 1 && W >= 1 && C >= 1, "N >= 0, H, W, C >= 1");
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {
        if (sums) FI_HIP_CHECK(hipMemsetAsync(sums, 0, sizeof(float) * (size_t)C, st));
        return FI_OK;
    }
    FI_REQUIRE(d && g, "null pointer");
    const long P = (long)N * H * W;
    if (!crops_eligible(FI_CROPS16_GATE_PACK, 0, C, P > kIntMax ? 0 : P, nullptr, d, y, g, sums)) {
        fi::set_error("fi_crops16_gate_pack: unsupported call (N %d, H %d, W %d, C %d, d %p, y %p, g %p, sums %p): needs "
                      "C %% 8 == 0, d, y and g aligned to 16 bytes, sums to 4, N*H*W and the workgroup count below 2^31",
                      N, H, W, C, (const void *)d, y, (const void *)g, (const void *)sums);
        return FI_ERR_UNSUPPORTED;
    }
    const int rows = rows_per_group(P, C);
    const int ctiles = fi::ceil_div(C, GP_CH);
    const unsigned blocks = (unsigned)((long)fi::ceil_div((int)P, rows) * ctiles);
    if (sums) FI_HIP_CHECK(hipMemsetAsync(sums, 0, sizeof(float) * (size_t)C, st));
    hipLaunchKernelGGL(gate_pack_kernel, dim3(blocks), dim3(kThreads), 0, st, d, (const E16 *)y, (E16 *)g, sums, (int)P, C,
                       rows, ctiles);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

}  // extern "C"
