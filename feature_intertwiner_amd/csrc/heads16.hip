// heads16.hip -- libfi_heads16.so (include/fi_heads16.h): the two memory-bound backward launches of a train step whose box
// and mask heads run on 16-bit channels-last crops.  heads16_f16.hip includes this file with FI_E16_HALF defined: the same
// kernels on IEEE half under the *_f16 names.
//
// Crop backward.  crop_bwd_cl_kernel (crop_and_resize.hip) without its LDS transposition: the gradient arrives
// [box][bin][channel], so a box's slab of 64 bins is ONE contiguous run of 64 * depth values.  One workgroup per (box, slab):
// the two sampling tables (crop_dev.h) by crop_h + crop_w lanes, then one table entry per bin -- the four cell offsets and
// the four weights -- by one lane per bin.  The run is walked 256 lanes x 16 bytes at a time.  The atomics are what the
// kernel is bound by, and a wave-instruction of fp32 atomics runs at full rate only on contiguous bytes, so a lane does not
// add the 8 channels it loaded (its neighbours would sit 32 bytes apart): each wavefront parks its 1 KB in LDS and lane L of
// step j takes value 64 j + L of it -- for every j the 64 lanes hold 64 consecutive values of the run, i.e. consecutive
// channels of a bin (up to the bin's end), and each of the four taps is one atomic instruction on 256 contiguous bytes of a
// map row when depth >= 64.  (bin, channel) of a value: one division per lane and pass, then steps of 64.
// Class rows.  gate_pack_kernel's shape (crops16.hip) on the rows (pixel, (a, b)) of ONE RoI: a thread keeps 8 channels,
// the row groups side by side are a multiple of 4, so a thread's rows share (a, b) and its d values are one plane of d.  It
// keeps 8 sums of d * u and 8 sums of the stored du in fp32 registers; the threads of the workgroup combine in LDS; the
// workgroup adds one value per channel to dweight[cls], one per ((a, b), channel) to colsum, and -- the workgroup of the
// RoI's first channel tile -- one to dbias[cls].  The channel tile shrinks from 512 to 64 while the grid has fewer than two
// workgroups per compute unit; the tiles partition the channels, so the count of atomics per (RoI, channel) stays one.
#include <stdint.h>

#include "fi_common.h"
#include "conv_act16_dev.h"
#include "crop_dev.h"
#include "../../include/fi_heads16.h"

namespace {

constexpr int kSlab = 64;                     // bins of a crop-backward workgroup
constexpr int CR_CT = 512;                    // most channels of a class-rows workgroup: 64 lanes of 8
constexpr int CR_CT_MIN = 64;
constexpr long CR_GROUPS = 2 * kCUs;          // workgroups aimed at
constexpr long kHWMax = 1L << 28;
constexpr int kDepthMax = 1 << 20;            // a slab's 64 * depth values are counted in an int

struct LevelSetF {
    float *img[kMaxLevels];
    int H[kMaxLevels];
    int W[kMaxLevels];
    int n;
};

struct Cell {
    int tl, tr, bl, br;                       // cell index (row * W + column) of the four taps; tl < 0: the bin adds nothing
    float wy0, fy, wx0, fx;
};

// orders the LDS accesses of ONE wavefront's lanes for the compiler (the hardware keeps them in order anyway)
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(kThreads) void crop_bwd16_kernel(LevelSetF ls, const E16 *__restrict__ grads,
                                                              const float *__restrict__ boxes,
                                                              const int *__restrict__ box_ind, const int *__restrict__ level,
                                                              int num_boxes, int batch, int depth, int crop_h, int crop_w,
                                                              int slabs)
{
    __shared__ Tap s_ty[kMaxCrop];
    __shared__ Tap s_tx[kMaxCrop];
    __shared__ Cell s_cell[kSlab];
    __shared__ __attribute__((aligned(16))) E16 s_stage[kThreads * 8];      // 1 KB per wavefront

    const int tid = threadIdx.x;
    const int bins = crop_h * crop_w;
    const int box = blockIdx.x / slabs;
    const int slab = blockIdx.x - box * slabs;
    const int b_begin = slab * kSlab;
    const int nb = min(bins - b_begin, kSlab);

    BoxHeader h;
    if (!load_box(ls, boxes, box_ind, level, box, batch, h)) return;      // (uniform: the whole workgroup leaves)
    if (tid < crop_h) s_ty[tid] = make_tap(h.y1, h.y2, h.H, crop_h, tid);
    if (tid >= 64 && tid < 64 + crop_w) s_tx[tid - 64] = make_tap(h.x1, h.x2, h.W, crop_w, tid - 64);
    __syncthreads();
    if (tid < nb) {
        const int b = b_begin + tid;
        const int y = b / crop_w;
        const int x = b - y * crop_w;
        const Tap ty = s_ty[y];
        const Tap tx = s_tx[x];
        Cell c;
        c.tl = -1;
        c.tr = c.bl = c.br = 0;
        c.wy0 = c.fy = c.wx0 = c.fx = 0.0f;
        if (ty.valid & tx.valid) {            // 0 <= i0 <= i1 <= extent - 1 on both axes
            const int r0 = ty.i0 * h.W, r1 = ty.i1 * h.W;
            c.tl = r0 + tx.i0;
            c.tr = r0 + tx.i1;
            c.bl = r1 + tx.i0;
            c.br = r1 + tx.i1;
            c.wy0 = 1.0f - ty.frac;
            c.fy = ty.frac;
            c.wx0 = 1.0f - tx.frac;
            c.fx = tx.frac;
        }
        s_cell[tid] = c;
    }
    __syncthreads();

    float *__restrict__ dst = ls.img[h.lvl] + (size_t)h.img * h.H * h.W * depth;
    const E16 *__restrict__ src = grads + ((size_t)box * bins + b_begin) * depth;      // 16-byte aligned: depth % 8 == 0
    const int total = nb * depth;             // values of the slab
    const int items = total / 8;
    const int lane = tid & 63, wave = tid >> 6;
    const int q64 = 64 / depth, r64 = 64 - q64 * depth;
    const E16 *mine = s_stage + wave * 512;
    // A wavefront stages and reads only ITS 1 KB of s_stage, and the LDS operations of one wavefront execute in program
    // order: no workgroup barrier is needed inside the loop, only the compiler must not move the reads over the writes
    for (int i0 = 0; i0 < items; i0 += kThreads) {
        if (i0 + tid < items)
            *reinterpret_cast<u32x4 *>(s_stage + tid * 8) = *reinterpret_cast<const u32x4 *>(src + (size_t)(i0 + tid) * 8);
        wave_sync();
        int flat = (i0 + wave * 64) * 8 + lane;
        int bin = flat / depth;
        int c = flat - bin * depth;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (flat < total) {                // bin < nb
                const Cell cell = s_cell[bin];
                if (cell.tl >= 0) {
                    const float gv = (float)mine[64 * j + lane];
                    const float gtop = cell.wy0 * gv;
                    const float gbot = cell.fy * gv;
                    float *p = dst + c;
                    atomicAdd(p + (size_t)cell.tl * depth, cell.wx0 * gtop);
                    atomicAdd(p + (size_t)cell.tr * depth, cell.fx * gtop);
                    atomicAdd(p + (size_t)cell.bl * depth, cell.wx0 * gbot);
                    atomicAdd(p + (size_t)cell.br * depth, cell.fx * gbot);
                }
            }
            flat += 64;
            bin += q64;
            c += r64;
            if (c >= depth) {
                c -= depth;
                ++bin;
            }
        }
        wave_sync();                           // the stage is rewritten by the next pass
    }
}

// d: [n][4][HW] fp32; u / du: [n][HW * 4 rows][C] 16-bit, row = pixel * 4 + (2a + b); w: [K][C]
__global__ __launch_bounds__(kThreads) void class_rows_bwd_kernel(const float *__restrict__ d, const E16 *__restrict__ u,
                                                                  const E16 *__restrict__ w, const long *__restrict__ cls,
                                                                  E16 *__restrict__ du, float *__restrict__ colsum,
                                                                  float *__restrict__ dweight, float *__restrict__ dbias,
                                                                  int HW, int C, int K, int CT)
{
    __shared__ float s_dw[CR_CT];
    __shared__ float s_col[4 * CR_CT];
    __shared__ float s_part[kThreads / 64];
    const int tid = threadIdx.x;
    const long i = blockIdx.x;
    const int c_base = (int)blockIdx.y * CT;
    const int cw = C - c_base < CT ? C - c_base : CT;                  // % 8 == 0, <= 512
    const int lanes_c = cw / 8;                                        // <= 64
    const int rstep = (kThreads / lanes_c) & ~3;                       // >= 4: a thread's rows share (a, b)
    const int rows = 4 * HW;
    const long k = cls[i];
    const E16 *__restrict__ u_i = u + (size_t)i * rows * C + c_base;
    E16 *__restrict__ du_i = du + (size_t)i * rows * C + c_base;
    const int cg = tid % lanes_c, g = tid / lanes_c;
    const bool on = g < rstep;

    if (k < 0 || k >= K) {                                             // no such class (uniform): zeros, no sums
        if (on) {
            e16x8 zero;
#pragma unroll
            for (int j = 0; j < 8; ++j) zero[j] = (E16)0.f;
            for (int row = g; row < rows; row += rstep) *reinterpret_cast<e16x8 *>(du_i + (size_t)row * C + cg * 8) = zero;
        }
        return;
    }
    for (int c = tid; c < cw; c += kThreads) s_dw[c] = 0.f;
    for (int c = tid; c < 4 * CT; c += kThreads) s_col[c] = 0.f;
    __syncthreads();

    if (on) {
        const int ab = g & 3;
        const e16x8 wv = *reinterpret_cast<const e16x8 *>(w + (size_t)k * C + c_base + cg * 8);
        float wf[8], acc_w[8], acc_c[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            wf[j] = (float)wv[j];
            acc_w[j] = acc_c[j] = 0.f;
        }
        const float *__restrict__ d_ab = d + ((size_t)i * 4 + ab) * HW;
        for (int row = g; row < rows; row += rstep) {                  // row % 4 == ab
            const float dv = d_ab[row >> 2];
            const size_t o = (size_t)row * C + cg * 8;
            const e16x8 uu = *reinterpret_cast<const e16x8 *>(u_i + o);
            e16x8 out;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float uf = (float)uu[j];
                E16 r = (E16)(dv * wf[j]);                             // the one rounding
                if (!(uf > 0.f)) r = (E16)0.f;
                out[j] = r;
                acc_c[j] += (float)r;
                acc_w[j] += dv * uf;
            }
            *reinterpret_cast<e16x8 *>(du_i + o) = out;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (dweight) atomicAdd(&s_dw[cg * 8 + j], acc_w[j]);
            if (colsum) atomicAdd(&s_col[ab * CT + cg * 8 + j], acc_c[j]);
        }
    }
    float bsum = 0.f;
    if (dbias && blockIdx.y == 0) {                                    // (uniform)
        const float *__restrict__ d_i = d + (size_t)i * rows;
        for (int t = tid; t < rows; t += kThreads) bsum += d_i[t];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) bsum += __shfl_xor(bsum, off, 64);
        if ((tid & 63) == 0) s_part[tid >> 6] = bsum;
    }
    __syncthreads();
    if (dweight)
        for (int c = tid; c < cw; c += kThreads) atomicAdd(&dweight[(size_t)k * C + c_base + c], s_dw[c]);
    if (colsum)
        for (int t = tid; t < 4 * cw; t += kThreads) {
            const int ab = t / cw, c = t - ab * cw;
            atomicAdd(&colsum[(size_t)ab * C + c_base + c], s_col[ab * CT + c]);
        }
    if (dbias && blockIdx.y == 0 && tid == 0) atomicAdd(&dbias[k], (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]));
}

// channels of a class-rows workgroup: halved from CR_CT while the grid stays under CR_GROUPS workgroups
int class_rows_tile(long n, int C)
{
    int ct = CR_CT;
    while (ct > CR_CT_MIN && n * ((C + ct - 1) / ct) < CR_GROUPS) ct /= 2;
    return ct;
}

#ifndef FI_E16_HALF
// THE statement of what the entry points take (the pointers may be NULL: absent or not known yet)
bool heads_eligible(int kind, int m, int C, int h, int w, int n, const void *const *f32_ptrs, const void *p0, const void *p1,
                    const void *p2, const void *p3)
{
    if (C < 8 || C % 8 != 0 || n < 1 || h < 1 || w < 1) return false;
    if (kind == FI_HEADS16_CROP_BWD) {
        if (m < 1 || m > kMaxLevels || h > kMaxCrop || w > kMaxCrop || C > kDepthMax) return false;
        if (f32_ptrs)
            for (int l = 0; l < m; ++l)
                if (((uintptr_t)f32_ptrs[l] & 3) != 0) return false;
        if (((uintptr_t)p0 & 15) != 0) return false;
        return (long)n * ((h * w + kSlab - 1) / kSlab) <= kIntMax;
    }
    if (kind == FI_HEADS16_CLASS_ROWS) {
        if (m < 1 || (long)h * w > kHWMax) return false;
        if (f32_ptrs)
            for (int l = 0; l < 3; ++l)
                if (((uintptr_t)f32_ptrs[l] & 3) != 0) return false;
        if ((((uintptr_t)p0 | (uintptr_t)p1 | (uintptr_t)p2) & 15) != 0 || ((uintptr_t)p3 & 3) != 0) return false;
        return (C + CR_CT_MIN - 1) / CR_CT_MIN <= 65535;
    }
    return false;
}
#endif

}  // namespace

extern "C" {

#ifndef FI_E16_HALF
int fi_heads16_eligible(int kind, int m, int C, int h, int w, int n, const void *const *f32_ptrs, const void *p0,
                        const void *p1, const void *p2, const void *p3)
{
    return heads_eligible(kind, m, C, h, w, n, f32_ptrs, p0, p1, p2, p3) ? 1 : 0;
}
#endif

int FI16(fi_heads16_pyramid_crop_backward)(const void *grads, float *const *level_grads_host, const int *level_h_host,
                                           const int *level_w_host, int num_levels, const float *boxes,
                                           const int32_t *box_ind, const int32_t *level, int num_boxes, int batch, int depth,
                                           int crop_h, int crop_w, int accumulate, fi_stream_t stream)
{
    FI_REQUIRE(num_boxes >= 0 && batch >= 1 && depth >= 1 && crop_h >= 1 && crop_w >= 1,
               "num_boxes >= 0, batch, depth, crop_h, crop_w >= 1");
    FI_REQUIRE(num_levels >= 1 && num_levels <= kMaxLevels, "1 <= num_levels <= 8");
    FI_REQUIRE(level_grads_host && level_h_host && level_w_host, "null level arrays");
    FI_REQUIRE(num_boxes == 0 || (grads && boxes && box_ind), "null pointer");
    LevelSetF ls = {};
    ls.n = num_levels;
    for (int l = 0; l < num_levels; ++l) {
        ls.img[l] = level_grads_host[l];
        ls.H[l] = level_h_host[l];
        ls.W[l] = level_w_host[l];
        FI_REQUIRE(ls.img[l] && ls.H[l] >= 1 && ls.W[l] >= 1, "bad level entry");
    }
    FI_REQUIRE(num_boxes == 0 || level != nullptr || num_levels == 1, "level[] is required with more than one map");
    // an empty call is held to the rules too (as one box), so that what clears the maps is what could have added to them
    if (fi_heads16_eligible(FI_HEADS16_CROP_BWD, num_levels, depth, crop_h, crop_w, num_boxes > 0 ? num_boxes : 1,
                            reinterpret_cast<const void *const *>(level_grads_host), grads, nullptr, nullptr, nullptr) != 1) {
        fi::set_error("fi_heads16_pyramid_crop_backward: unsupported call (num_levels %d, depth %d, crop %dx%d, %d boxes, "
                      "grads %p): needs depth %% 8 == 0, crop_h, crop_w <= %d, grads aligned to 16 bytes, the maps to 4, "
                      "boxes x slabs of %d bins below 2^31", num_levels, depth, crop_h, crop_w, num_boxes, grads, kMaxCrop,
                      kSlab);
        return FI_ERR_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    for (int l = 0; !accumulate && l < num_levels; ++l)
        FI_HIP_CHECK(hipMemsetAsync(ls.img[l], 0, sizeof(float) * (size_t)batch * depth * ls.H[l] * ls.W[l], st));
    if (num_boxes == 0) return FI_OK;
    const int slabs = fi::ceil_div(crop_h * crop_w, kSlab);
    hipLaunchKernelGGL(crop_bwd16_kernel, dim3((unsigned)((long)num_boxes * slabs)), dim3(kThreads), 0, st, ls,
                       static_cast<const E16 *>(grads), boxes, box_ind, level, num_boxes, batch, depth, crop_h, crop_w, slabs);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int FI16(fi_heads16_class_rows_backward)(const float *d, const void *u, const void *w, const int64_t *cls, void *du,
                                         float *colsum, float *dweight, float *dbias, int n, int H, int W, int C, int K,
                                         fi_stream_t stream)
{
    FI_REQUIRE(n >= 0 && H >= 1 && W >= 1 && C >= 1 && K >= 1, "n >= 0, H, W, C, K >= 1");
    FI_REQUIRE(n == 0 || (d && u && w && cls && du), "null pointer");
    const void *f32[3] = {colsum, dweight, dbias};
    if (fi_heads16_eligible(FI_HEADS16_CLASS_ROWS, K, C, H, W, n > 0 ? n : 1, f32, u, w, du, d) != 1) {
        fi::set_error("fi_heads16_class_rows_backward: unsupported call (n %d, H %d, W %d, C %d, K %d, d %p, u %p, w %p, "
                      "du %p, colsum %p, dweight %p, dbias %p): needs C %% 8 == 0, u, w and du aligned to 16 bytes, the fp32 "
                      "tensors to 4, H * W <= 2^28", n, H, W, C, K, (const void *)d, u, w, du, (const void *)colsum,
                      (const void *)dweight, (const void *)dbias);
        return FI_ERR_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    if (colsum) FI_HIP_CHECK(hipMemsetAsync(colsum, 0, sizeof(float) * 4 * (size_t)C, st));
    if (n == 0) return FI_OK;
    const int ct = class_rows_tile(n, C);
    hipLaunchKernelGGL(class_rows_bwd_kernel, dim3((unsigned)n, (unsigned)fi::ceil_div(C, ct)), dim3(kThreads), 0, st, d,
                       static_cast<const E16 *>(u), static_cast<const E16 *>(w), reinterpret_cast<const long *>(cls),
                       static_cast<E16 *>(du), colsum, dweight, dbias, H * W, C, K, ct);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

}  // extern "C"
