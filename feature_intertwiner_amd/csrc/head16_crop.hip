// head16_crop.hip -- libfi_head16.so (include/fi_head16.h): pyramid RoIAlign (single bilinear tap per bin) that reads 16-bit
// channels-last maps ([batch][H][W][depth], bf16) and WRITES 16-bit channels-last crops [num_boxes][ch][cw][depth], the
// operand of the box and mask heads' 16-bit layers.  head16_crop_f16.hip includes this file with FI_E16_HALF defined: the
// same kernel on IEEE half under the *_f16 name.
//
// The gather is roi16_crop_fwd_kernel's (crop_roi16.hip): the RoI's sampling table (crop_dev.h: the box transform of the
// reference, operation order kept) computed once by crop_h + crop_w lanes and parked in two LDS tables, a lane's 16-byte
// load holding 8 channels of a tap, depth / 8 lanes covering a bin, 256 / (depth / 8) bin groups side by side, a lane
// keeping 4 bins x 4 taps = 16 loads of 16 bytes in flight.  What is gone is everything behind the gather: source and
// destination are both channels-last, so there is no LDS tile, no transpose, no second barrier and no rule on channel
// chunks -- the 8 interpolated channels are rounded once and leave as ONE 16-byte store, neighbouring lanes on
// neighbouring 16 bytes of the bin's depth * 2 contiguous bytes.  A box's crop is one contiguous run of ch * cw * depth
// values.
// Grid: one workgroup = one RoI x one slab of 64 bins (one trip of 16 groups x 4 bins at depth 128, two at depth 256).  The
// 7 x 7 crop is one slab per box, the 14 x 14 crop four: the mask head's 200 detections are 800 workgroups, not 200.  Every
// slab's workgroup recomputes the box's two tables (crop_h + crop_w lanes, one barrier).
// depth / 8 need not divide 256: with 3 lanes per bin 85 groups run and one lane idles; with 33, 7 groups and 25 idle
// lanes.  depth / 8 > 256: one group of 256 lanes walks the channels in chunks of 2048.
// Arithmetic: roi16_crop_fwd_kernel's fp32 value (taps widened exactly, top = tl + (tr - tl) * fx, bot = bl + (br - bl)
// * fx, top + (bot - top) * fy, each operation rounded separately: fi_common.h turns contraction off), then one
// round-to-nearest-even to the 16-bit type.
#include <stdint.h>

#include "fi_common.h"
#include "crop_dev.h"
#include "../../include/fi_head16.h"

#ifdef FI_E16_HALF
#define FI16(stem) stem##_f16
#define E16 _Float16
#else
#define FI16(stem) stem##_bf16
#define E16 __bf16
#endif

namespace {

constexpr int kThreads = 256;
constexpr int kVec = 8;                 // channels per lane: one 16-byte load, one 16-byte store
constexpr int kSlab = 64;               // bins per workgroup
constexpr long kIntMax = 2147483647L;

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef E16 e16x8 __attribute__((ext_vector_type(8)));

// channel q (0..7) of the 8 a 16-byte load holds, widened exactly; q is a compile-time constant after unrolling
__device__ __forceinline__ float widen(const u32x4 &v, int q)
{
#ifdef FI_E16_HALF
    const f16x8 h = __builtin_bit_cast(f16x8, v);
    return (float)h[q];
#else
    const unsigned w = v[q >> 1];       // little endian: the even channel is the low half
    return __uint_as_float((q & 1) ? (w & 0xffff0000u) : (w << 16));
#endif
}

// Register budget: 16 loads of 4 registers are 64 VGPRs in flight; crop_roi16.hip records that the compiler, left alone,
// widens all of them before it interpolates and ends above 230.  There is no LDS tile to bound the residency here, so the
// budget is the only limit: (4, 4) -- 128 registers, four workgroups per CU -- compiles to 124 VGPRs for both types,
// without scratch.  Other budgets were not evaluated on the GPU.
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4, 4))) void head16_crop_fwd_kernel(
    LevelSet16 ls, const float *__restrict__ boxes, const int *__restrict__ box_ind, const int *__restrict__ level,
    int num_boxes, int batch, int depth, int crop_h, int crop_w, float extrap, int slabs, uint16_t *__restrict__ crops)
{
    __shared__ Tap s_ty[kMaxCrop];
    __shared__ Tap s_tx[kMaxCrop];

    const int tid = threadIdx.x;
    const int bins = crop_h * crop_w;
    const int box = blockIdx.x / slabs;
    const int slab = blockIdx.x - box * slabs;
    const int b_begin = slab * kSlab;
    const int b_end = min(bins, b_begin + kSlab);
    uint16_t *__restrict__ out = crops + (size_t)box * bins * depth;      // 16-byte aligned: depth % 8 == 0

    BoxHeader h;
    if (!load_box(ls, boxes, box_ind, level, box, batch, h)) {
        if (level && level[box] == -1) return;      // level -1: a row of static capacity that nobody reads -- not even written
        u32x4 *__restrict__ o = reinterpret_cast<u32x4 *>(out + (size_t)b_begin * depth);
        const int n16 = (b_end - b_begin) * (depth / kVec);
        const u32x4 zero = {0u, 0u, 0u, 0u};
        for (int i = tid; i < n16; i += kThreads) o[i] = zero;
        return;
    }
    if (tid < crop_h) s_ty[tid] = make_tap(h.y1, h.y2, h.H, crop_h, tid);
    if (tid >= 64 && tid < 64 + crop_w) s_tx[tid - 64] = make_tap(h.x1, h.x2, h.W, crop_w, tid - 64);
    __syncthreads();

    const int lanes = min(depth / kVec, kThreads);      // lanes per bin (consecutive lanes: consecutive 8-channel groups)
    const int ng = kThreads / lanes;                    // bin groups; the lanes past ng * lanes have no bin
    const int g = tid / lanes;
    if (g >= ng) return;
    const int c_first = (tid - g * lanes) * kVec;
    const int W = h.W;
    e16x8 ex;
#pragma unroll
    for (int q = 0; q < kVec; ++q) ex[q] = (E16)extrap;
    const u32x4 exv = __builtin_bit_cast(u32x4, ex);
    for (int c = c_first; c < depth; c += lanes * kVec) {      // one trip unless depth / 8 > 256
        // 2-byte elements: the offsets below count them
        const uint16_t *__restrict__ src =
            static_cast<const uint16_t *>(ls.img[h.lvl]) + (size_t)h.img * h.H * h.W * depth + c;
        constexpr int UNROLL = 4;
        for (int b0 = b_begin + g; b0 < b_end; b0 += ng * UNROLL) {
            u32x4 tl[UNROLL], tr[UNROLL], bl[UNROLL], br[UNROLL];
            float fx[UNROLL], fy[UNROLL];
            int ok[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int b = b0 + u * ng;
                ok[u] = 0;
                fx[u] = fy[u] = 0.0f;
                if (b < b_end) {
                    const int y = b / crop_w;
                    const int x = b - y * crop_w;
                    const Tap ty = s_ty[y];
                    const Tap tx = s_tx[x];
                    ok[u] = (ty.valid & tx.valid) ? 1 : 2;
                    if (ok[u] == 1) {
                        const size_t r0 = (size_t)ty.i0 * W, r1 = (size_t)ty.i1 * W;
                        tl[u] = *reinterpret_cast<const u32x4 *>(src + (r0 + tx.i0) * depth);
                        tr[u] = *reinterpret_cast<const u32x4 *>(src + (r0 + tx.i1) * depth);
                        bl[u] = *reinterpret_cast<const u32x4 *>(src + (r1 + tx.i0) * depth);
                        br[u] = *reinterpret_cast<const u32x4 *>(src + (r1 + tx.i1) * depth);
                        fx[u] = tx.frac;
                        fy[u] = ty.frac;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int b = b0 + u * ng;
                if (ok[u] == 0) continue;
                u32x4 *__restrict__ dst = reinterpret_cast<u32x4 *>(out + (size_t)b * depth + c);
                if (ok[u] == 1) {
                    e16x8 r;
#pragma unroll
                    for (int q = 0; q < kVec; ++q) {
                        const float vtl = widen(tl[u], q), vtr = widen(tr[u], q);
                        const float vbl = widen(bl[u], q), vbr = widen(br[u], q);
                        const float dt = vtr - vtl;
                        const float top = vtl + dt * fx[u];
                        const float db = vbr - vbl;
                        const float bot = vbl + db * fx[u];
                        const float dv = bot - top;
                        r[q] = (E16)(top + dv * fy[u]);
                    }
                    *dst = __builtin_bit_cast(u32x4, r);
                } else {
                    *dst = exv;
                }
            }
        }
    }
}

#ifndef FI_E16_HALF
// THE statement of what the kernel takes (the pointers may be NULL: not known yet)
bool crop_eligible(int num_levels, int depth, int crop_h, int crop_w, const void *const *level_images_host,
                   const void *crops)
{
    if (num_levels < 1 || num_levels > kMaxLevels) return false;
    if (depth < kVec || depth % kVec != 0) return false;
    if (crop_h < 1 || crop_w < 1 || crop_h > kMaxCrop || crop_w > kMaxCrop) return false;
    if (level_images_host)
        for (int l = 0; l < num_levels; ++l)
            if (((uintptr_t)level_images_host[l] & 15) != 0) return false;
    return ((uintptr_t)crops & 15) == 0;
}
#endif

}  // namespace

extern "C" {

#ifndef FI_E16_HALF
int fi_head16_crop_eligible(int num_levels, int depth, int crop_h, int crop_w, const void *const *level_images_host,
                            const void *crops)
{
    return crop_eligible(num_levels, depth, crop_h, crop_w, level_images_host, crops) ? 1 : 0;
}
#endif

int FI16(fi_head16_pyramid_crop_forward)(const void *const *level_images_host, const int *level_h_host,
                                         const int *level_w_host, int num_levels, const float *boxes,
                                         const int32_t *box_ind, const int32_t *level, int num_boxes, int batch,
                                         int depth, int crop_h, int crop_w, float extrapolation_value, void *crops,
                                         fi_stream_t stream)
{
    FI_REQUIRE(num_boxes >= 0 && batch >= 1 && depth >= 1 && crop_h >= 1 && crop_w >= 1,
               "num_boxes >= 0, batch, depth, crop_h, crop_w >= 1");
    if (num_boxes == 0) return FI_OK;
    FI_REQUIRE(level_images_host && level_h_host && level_w_host && boxes && box_ind && crops, "null pointer");
    if (fi_head16_crop_eligible(num_levels, depth, crop_h, crop_w, level_images_host, crops) != 1) {
        fi::set_error("fi_head16_pyramid_crop_forward: unsupported call (num_levels %d, depth %d, crop %dx%d, crops %p): "
                      "needs 1 <= num_levels <= %d, depth %% 8 == 0, crop_h, crop_w <= %d, every map and crops aligned "
                      "to 16 bytes", num_levels, depth, crop_h, crop_w, (const void *)crops, kMaxLevels, kMaxCrop);
        return FI_ERR_UNSUPPORTED;
    }
    LevelSet16 ls = {};
    ls.n = num_levels;
    for (int l = 0; l < num_levels; ++l) {
        ls.img[l] = level_images_host[l];
        ls.H[l] = level_h_host[l];
        ls.W[l] = level_w_host[l];
        FI_REQUIRE(ls.img[l] && ls.H[l] >= 1 && ls.W[l] >= 1, "bad level entry");
    }
    FI_REQUIRE(level != nullptr || num_levels == 1, "level[] is required with more than one map");
    const int slabs = fi::ceil_div(crop_h * crop_w, kSlab);
    const long nblk = (long)num_boxes * slabs;
    if (nblk > kIntMax) {
        fi::set_error("fi_head16_pyramid_crop_forward: unsupported call: %d boxes x %d slabs of %d bins is a grid of 2^31 "
                      "workgroups or more", num_boxes, slabs, kSlab);
        return FI_ERR_UNSUPPORTED;
    }
    hipLaunchKernelGGL(head16_crop_fwd_kernel, dim3((unsigned)nblk), dim3(kThreads), 0, (hipStream_t)stream, ls, boxes,
                       box_ind, level, num_boxes, batch, depth, crop_h, crop_w, extrapolation_value, slabs,
                       static_cast<uint16_t *>(crops));
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

}  // extern "C"
