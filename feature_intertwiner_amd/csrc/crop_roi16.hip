// crop_roi16.hip -- libfi_roi16.so (include/fi_roi16.h): pyramid RoIAlign (single bilinear tap per bin) that READS 16-bit
// channels-last maps ([batch][H][W][depth], bf16) and writes the fp32 [num_boxes][depth][ch][cw] crops the heads consume.
// crop_roi16_f16.hip includes this file with FI_E16_HALF defined: the same kernel on IEEE half under the *_f16 name.
//
// The kernel has the shape of crop_fwd_cl_kernel (crop_and_resize.hip): one 256-thread workgroup = one RoI x one channel
// chunk, the RoI's sampling table (crop_dev.h: the box transform of the reference, operation order kept) computed once by
// crop_h + crop_w lanes and parked in two LDS tables, lanes running over channels, results transposed through an LDS
// tile [channels][bins | 1] and written back as one contiguous fp32 block.
// What differs is the gather: the map's elements are 2 bytes, so a lane's 16-byte load holds 8 channels, not 4: cpb / 8
// lanes cover a bin and 256 / (cpb / 8) bin groups run side by side.  A lane keeps 4 bins x 4 taps in flight: 16 loads of
// 16 bytes, the 256 bytes per lane the fp32 kernel's comment derives.  The bytes a tap pulls from L2 / HBM are half of the
// fp32 map's.  What pick_chunk() makes of the model's two launches on 256-channel maps (cpb = channels per workgroup):
//   7 x 7:   256 channels would be a 50176-byte tile, over the rule's 28 KB, so cpb = 128: a 25088-byte tile (+ 2 KB of
//            tables; 5 workgroups per CU fit by LDS), 2 chunks per box, 16 lanes per bin (256 contiguous bytes of a tap),
//            16 bin groups, ONE trip of 16 x 4 = 64 slots for the 49 bins (15 slots empty).  The fp32 kernel at the same cpb
//            has 32 lanes per bin, 8 groups and two trips of 32 slots.
//   14 x 14: the rule stops at cpb = 64: a 50432-byte tile (3 workgroups per CU by LDS), 4 chunks per box, 8 lanes per bin
//            (128 bytes of a tap), 32 bin groups, two trips of 128 slots for the 196 bins.
// A map of 256 channels never runs at cpb = 256; only crops of at most 27 bins do (256 * 27 * 4 <= 28 KB).
// Tried and dropped: the tile's rows permuted (channel 8 * lane + q in row q * lanes + lane).  A ds_write_b32 is served in
// groups of 32 lanes over 32 banks; at 7 x 7 a group is 2 bins x 16 lanes with a lane stride of 8 * 49 words, which is 8
// banks (4-way), and with the lane as the row the stride is the odd pitch: 32 banks but for one pair.  The 7 x 7 launch
// went from 0.070-0.072 ms to 0.072-0.093 ms, so the store conflicts are not what bounds it (profiles/roi16_probe.txt has
// the kept form).
// Arithmetic: the four taps are widened exactly to fp32 (bf16: a 16-bit shift; half: v_cvt_f32_f16) and interpolated by
// the fp32 kernel's expression in its order, each operation rounded separately (fi_common.h turns contraction off):
// top = tl + (tr - tl) * fx, bot = bl + (br - bl) * fx, top + (bot - top) * fy.  The crops are bit-identical to
// fi_pyramid_crop_forward_nhwc on the widened maps; nothing is rounded to 16 bits.
#include <stdint.h>

#include "fi_common.h"
#include "crop_dev.h"
#include "../../include/fi_roi16.h"

#ifdef FI_E16_HALF
#define FI16(stem) stem##_f16
#else
#define FI16(stem) stem##_bf16
#endif

namespace {

constexpr int kThreads = 256;
constexpr int kVec = 8;                 // channels per lane: one 16-byte load
constexpr int kMaxBins = 220;           // crop_h * crop_w the LDS tile holds (the fp32 channels-last kernel's bound)
constexpr long kIntMax = 2147483647L;

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

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

// Left alone the compiler widens all 16 loads of a lane before it interpolates (234..260 VGPRs: two waves per SIMD).  The
// attribute is a register budget for the compiler; what the hardware admits follows from the registers the kernel ends up
// with.  (3, 3) was chosen for the 14 x 14 launch, whose 50 KB tile allows three workgroups per CU, and for the generic
// instantiation: <14, 14> and <7, 7> come out at 126 (bf16) / 128 (half) VGPRs, <0, 0> at 127 / 154, none with scratch.
// For <7, 7> alone -- a 25 KB tile, five workgroups per CU by LDS -- the budget was NOT evaluated on the GPU: compiled
// with (4, 4) it has the same 126 / 128 registers (four waves per SIMD fit either way), while <0, 0> on half spills 25
// registers to scratch, which is why the one attribute all three share says three.
template <int CH, int CW>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(3, 3))) void roi16_crop_fwd_kernel(
    LevelSet16 ls, const float *__restrict__ boxes, const int *__restrict__ box_ind,
    const int *__restrict__ level, int num_boxes, int batch, int depth, int crop_h_rt,
    int crop_w_rt, float extrap, int cpb, int chunks, float *__restrict__ crops)
{
    const int crop_h = CH ? CH : crop_h_rt;
    const int crop_w = CW ? CW : crop_w_rt;
    const int bins = crop_h * crop_w;
    const int pitch = bins | 1;
    extern __shared__ float s_dyn[];          // [cpb][pitch]
    __shared__ Tap s_ty[kMaxCrop];
    __shared__ Tap s_tx[kMaxCrop];

    const int tid = threadIdx.x;
    const int box = blockIdx.x / chunks;
    const int chunk = blockIdx.x - box * chunks;
    const int c_begin = chunk * cpb;
    const int c_count = min(cpb, depth - c_begin);       // a multiple of 8: depth and cpb are
    const int total = c_count * bins;
    float *__restrict__ out = crops + ((size_t)box * depth + c_begin) * bins;

    BoxHeader h;
    if (!load_box(ls, boxes, box_ind, level, box, batch, h)) {
        if (level && level[box] == -1) return;      // level -1: a row of static capacity that nobody reads -- not even written
        for (int i = tid; i < total; i += kThreads) out[i] = 0.0f;
        return;
    }
    if (tid < crop_h) s_ty[tid] = make_tap(h.y1, h.y2, h.H, crop_h, tid);
    if (tid >= 64 && tid < 64 + crop_w) s_tx[tid - 64] = make_tap(h.x1, h.x2, h.W, crop_w, tid - 64);
    __syncthreads();

    const int lanes = cpb / kVec;              // lanes per bin (consecutive lanes: consecutive 8-channel groups)
    const int c = (tid % lanes) * kVec;        // first channel of this lane
    const int g = tid / lanes;                 // bin group
    const int ng = kThreads / lanes;
    // 2-byte elements: the offsets below count them
    const uint16_t *__restrict__ src =
        static_cast<const uint16_t *>(ls.img[h.lvl]) + (size_t)h.img * h.H * h.W * depth + c_begin + c;
    const int W = h.W;
    if (c < c_count) {
        constexpr int UNROLL = 4;
        for (int b0 = g; b0 < bins; b0 += ng * UNROLL) {
            u32x4 tl[UNROLL], tr[UNROLL], bl[UNROLL], br[UNROLL];
            float fx[UNROLL], fy[UNROLL];
            int ok[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int b = b0 + u * ng;
                ok[u] = 0;
                fx[u] = fy[u] = 0.0f;
                if (b < bins) {
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
                if (ok[u] == 1) {
#pragma unroll
                    for (int q = 0; q < kVec; ++q) {
                        const float vtl = widen(tl[u], q), vtr = widen(tr[u], q);
                        const float vbl = widen(bl[u], q), vbr = widen(br[u], q);
                        const float dt = vtr - vtl;
                        const float top = vtl + dt * fx[u];
                        const float db = vbr - vbl;
                        const float bot = vbl + db * fx[u];
                        const float dv = bot - top;
                        s_dyn[(c + q) * pitch + b] = top + dv * fy[u];
                    }
                } else if (ok[u] == 2) {
#pragma unroll
                    for (int q = 0; q < kVec; ++q) s_dyn[(c + q) * pitch + b] = extrap;
                }
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < total; i += kThreads) {
        const int cc = i / bins;
        out[i] = s_dyn[cc * pitch + (i - cc * bins)];
    }
}

// channels per workgroup: the rule of crop_and_resize.hip's pick_cl_chunk (the LDS tile is fp32 there and here) -- 256
// halved while the tile exceeds 28 KB or half the chunk already covers the map, never below 64
int pick_chunk(int depth, int bins)
{
    const int pitch = bins | 1;
    int cpb = 256;
    while (cpb > 64 && ((long)cpb * pitch * 4 > 28 * 1024 || cpb / 2 >= depth)) cpb /= 2;
    return cpb;
}

#ifndef FI_E16_HALF
// THE statement of what the kernel takes (the pointers may be NULL: not known yet)
bool crop_eligible(int num_levels, int depth, int crop_h, int crop_w, const void *const *level_images_host,
                   const void *crops)
{
    if (num_levels < 1 || num_levels > kMaxLevels) return false;
    if (depth < kVec || depth % kVec != 0) return false;
    if (crop_h < 1 || crop_w < 1 || crop_h > kMaxCrop || crop_w > kMaxCrop || (long)crop_h * crop_w > kMaxBins) return false;
    if (level_images_host)
        for (int l = 0; l < num_levels; ++l)
            if (((uintptr_t)level_images_host[l] & 15) != 0) return false;
    return ((uintptr_t)crops & 3) == 0;
}
#endif

}  // namespace

extern "C" {

#ifndef FI_E16_HALF
int fi_roi16_crop_eligible(int num_levels, int depth, int crop_h, int crop_w, const void *const *level_images_host,
                           const void *crops)
{
    return crop_eligible(num_levels, depth, crop_h, crop_w, level_images_host, crops) ? 1 : 0;
}
#endif

int FI16(fi_roi16_pyramid_crop_forward)(const void *const *level_images_host, const int *level_h_host,
                                        const int *level_w_host, int num_levels, const float *boxes,
                                        const int32_t *box_ind, const int32_t *level, int num_boxes, int batch,
                                        int depth, int crop_h, int crop_w, float extrapolation_value, float *crops,
                                        fi_stream_t stream)
{
    FI_REQUIRE(num_boxes >= 0 && batch >= 1 && depth >= 1 && crop_h >= 1 && crop_w >= 1,
               "num_boxes >= 0, batch, depth, crop_h, crop_w >= 1");
    if (num_boxes == 0) return FI_OK;
    FI_REQUIRE(level_images_host && level_h_host && level_w_host && boxes && box_ind && crops, "null pointer");
    if (fi_roi16_crop_eligible(num_levels, depth, crop_h, crop_w, level_images_host, crops) != 1) {
        fi::set_error("fi_roi16_pyramid_crop_forward: unsupported call (num_levels %d, depth %d, crop %dx%d, crops %p): "
                      "needs 1 <= num_levels <= %d, depth %% 8 == 0, crop_h, crop_w <= %d and crop_h * crop_w <= %d, every "
                      "map aligned to 16 bytes and crops to 4", num_levels, depth, crop_h, crop_w, (const void *)crops,
                      kMaxLevels, kMaxCrop, kMaxBins);
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
    const int bins = crop_h * crop_w;
    const int cpb = pick_chunk(depth, bins);
    const int chunks = fi::ceil_div(depth, cpb);
    const long nblk = (long)num_boxes * chunks;
    if (nblk > kIntMax) {
        fi::set_error("fi_roi16_pyramid_crop_forward: unsupported call: %d boxes x %d channel chunks is a grid of 2^31 "
                      "workgroups or more", num_boxes, chunks);
        return FI_ERR_UNSUPPORTED;
    }
    const size_t lds = sizeof(float) * (size_t)cpb * (bins | 1);
    auto k = (crop_h == 7 && crop_w == 7)     ? roi16_crop_fwd_kernel<7, 7>
             : (crop_h == 14 && crop_w == 14) ? roi16_crop_fwd_kernel<14, 14>
                                              : roi16_crop_fwd_kernel<0, 0>;
    hipLaunchKernelGGL(k, dim3((unsigned)nblk), dim3(kThreads), lds, (hipStream_t)stream, ls, boxes, box_ind, level,
                       num_boxes, batch, depth, crop_h, crop_w, extrapolation_value, cpb, chunks, crops);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

}  // extern "C"
