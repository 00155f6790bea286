// fi_common.h -- shared host-side helpers for libfi_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/fi_capi.h"

// Every fp32 multiply/add in this library is rounded separately: sampling
// coordinates feed floorf/ceilf and IoUs feed a threshold compare, both of which
// decide integer outputs that must match the CPU specification bit for bit.
#pragma clang fp contract(off)

namespace fi {

template <int V>
struct Int {
    static constexpr int value = V;      // a compile-time integer as a function argument (generic lambdas)
};

void set_error(const char *fmt, ...);

// conv1x1_ring.hip (called from fi_conv2d_forward with weight_layout 3)
struct RingArgs {
    const float *x, *wF, *bias, *scale, *residual, *gate;
    float *y;
    const float *zero;
    int N, Cin, HW, Cout, relu;
};
int launch_conv1x1_ring(const RingArgs &a, hipStream_t st);

// conv3x3_wino.hip (launched by fi_conv2d_forward_live when plan_forward picks the Winograd form of a patch slot, flat or
// 2-D): any NCHW map with even H and W, y / residual / gate 8-byte aligned; x 8-byte aligned for the PAIR staging
constexpr int WINO_HW = 14;          // H == W == 14 (the RoI maps, 7 x 7 tiles of 2 x 2 pixels) keeps a compile-time instantiation
constexpr int WINO_GROUP = 32;       // 2 x 2 tiles per workgroup
struct WinoArgs {
    const float *x, *w, *bias, *scale, *residual, *gate;
    float *y;
    const float *zero;
    int N, Cin, H, W, Cout, relu, flip;
    int hw14;                        // the plan's choice: the WINO_HW instantiation (FI_FWD_WINO14), else H and W at run time
    int grid;                        // ... its grid
    int pair;                        // ... and its staging: FI_WINO_STAGING_PAIR (x 8-byte aligned), else 4-byte loads only
};
void launch_conv3x3_wino_flat(const WinoArgs &a, hipStream_t st);

// conv3x3_wino_wgrad.hip (launched by launch_wgrad when plan_wgrad sets FI_LAUNCH_WINOGRAD): the weight gradient of the same
// layers over the same 2 x 2 tiles; x / dy NCHW and 16-byte aligned, dW tap-major, the pixel splits add with atomics
constexpr int WINO_WG_BLOCK = 64;    // a workgroup's Cout and Cin block (Cin and Cout are multiples of it: plan_wgrad)
constexpr int WINO_WG_STAGE = 4;     // 2 x 2 tiles per LDS stage; a pixel split is a whole number of stages
constexpr int WINO_WG_SLOTS = 256;   // workgroups blocks x splits may reach: one per CU (82 KB of LDS, 512 registers per lane)
constexpr int WINO_WG_MIN_TILES = 32;     // fewest tiles of a split (8 stages) unless it is the only one
// A batch (fi_conv2d_weight_grad_batch) takes the kernel from this many tiles per problem; its splits minimise
// rounds of WINO_WG_SLOTS workgroups x (tiles per split + WINO_WG_FIXED_TILES)
constexpr int WINO_WG_BATCH_MIN_TILES = 1024;
// a workgroup's prologue and atomic epilogue in tiles of the stage loop: profiles/wino_wgrad_probe.txt, 256 -> 256 on N4 maps,
// 133.1 us at 256 tiles per split (64 x 64) and 428.6 us at 1024 (128 x 128): 0.385 us per tile, 35 us fixed = 90 tiles; a
// round of the C4 x12 batch (1024 tiles) takes 434 us, 40 us above its tiles
constexpr int WINO_WG_FIXED_TILES = 96;
struct WinoWgradArgs {
    const float *x, *dy;
    float *dw, *dbias;               // dbias may be null
    int N, Cin, H, W, Cout;
    int tiles_per_split, splits;     // the plan's cut of the N * H/2 * W/2 tiles (a batch: of every problem)
};

// Several weight gradients of ONE geometry in one launch (fi_conv2d_weight_grad_batch): the operand pointers of every
// problem travel by value in the kernel arguments -- no device-side table, no host-to-device copy per launch.
constexpr int kWgBatchMax = FI_WGRAD_BATCH_MAX;
struct WgradBatch {
    int n;                                   // 0: a plain launch (the kernel's own x / dy / dw / dbias arguments)
    const float *x[kWgBatchMax];
    const float *dy[kWgBatchMax];
    float *dw[kWgBatchMax];
    float *db[kWgBatchMax];
};
// batch: null, or the problems of one launch (a.x / a.dy / a.dw / a.dbias are then not read).  FI_WINO_WGRAD_SCALAR_STAGING
// in the environment, read per call, takes the instantiation that stages with 4-byte loads only (the same results)
void launch_conv3x3_wino_wgrad(const WinoWgradArgs &a, hipStream_t st, const WgradBatch *batch = nullptr);

// n / d == umulhi(n, mul) >> sft for 0 <= n < 2^31 (mul = ceil(2^(32+sft) / d), 32 + sft = 31 + ceil(log2 d)); mul == 0
// encodes d == 1
inline void magic_div(unsigned d, unsigned &mul, unsigned &sft)
{
    if (d <= 1) {
        mul = 0;
        sft = 0;
        return;
    }
    unsigned L = 0;
    while ((1ull << L) < d) ++L;                   // ceil(log2 d)
    const unsigned total = 31 + L;                 // 2^total / d < 2^32
    const unsigned long long num = 1ull << total;
    mul = (unsigned)((num + d - 1) / d);
    sft = total - 32;                              // L >= 1 for d >= 2
}

#define FI_HIP_CHECK(expr)                                                         \
    do {                                                                           \
        hipError_t _e = (expr);                                                    \
        if (_e != hipSuccess) {                                                    \
            fi::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),   \
                          __FILE__, __LINE__);                                     \
            return FI_ERR_HIP;                                                     \
        }                                                                          \
    } while (0)

#define FI_REQUIRE(cond, msg)                                                      \
    do {                                                                           \
        if (!(cond)) {                                                             \
            fi::set_error("invalid argument: %s (%s)", msg, #cond);                \
            return FI_ERR_INVALID_ARG;                                             \
        }                                                                          \
    } while (0)

// RAII kernel timer: when profiling is enabled records a start event on `stream`
// at construction and a stop event at destruction (i.e. around the launch).
class ProfScope {
  public:
    ProfScope(int kernel_id, hipStream_t stream);
    ~ProfScope();

  private:
    int id_;
    hipStream_t stream_;
    hipEvent_t start_;
    bool active_;
};

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

}  // namespace fi
