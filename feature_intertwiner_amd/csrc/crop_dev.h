// crop_dev.h -- device code that crop_and_resize.hip (libfi_hip.so) and crop_roi16.hip (libfi_roi16.so) share: the RoI's
// sampling table (the box transform of the reference, operation order kept) and the per-workgroup box header.  Everything
// is in an unnamed namespace, so the instances in different libraries do not meet.
//
// Arithmetic specification: lib/roi_align/src/crop_and_resize.c:31-110 of the reference -- see oracle/fi_oracle.c
// (orc_axis_taps()), which both users are tested against bit for bit.
#pragma once
#include <stdint.h>

#include "fi_common.h"

namespace {

constexpr int kMaxCrop = 64;   // LDS table entries per axis
constexpr int kMaxLevels = 8;

struct Tap {
    int i0;      // floorf(coord)
    int i1;      // ceilf(coord)
    float frac;  // coord - i0
    int valid;   // 0 when coord is outside [0, extent-1]
};

struct LevelSet {
    const float *img[kMaxLevels];
    int H[kMaxLevels];
    int W[kMaxLevels];
    int n;
};

// ... and its sibling for 16-bit channels-last maps (bf16 / half: the kernel knows which)
struct LevelSet16 {
    const void *img[kMaxLevels];
    int H[kMaxLevels];
    int W[kMaxLevels];
    int n;
};

// Sampling coordinate k of one axis.  Keeps the operation order of the
// reference exactly (each * / + rounded to fp32; the crop == 1 case goes through
// double because of the 0.5 literal) -- oracle: orc_axis_taps().
// c(k) = base + (float)k * step: the two numbers the coordinate of every bin of one axis is made of.  crop == 1: the
// reference's double-precision midpoint as base and a zero step (base + 0 * 0 = base up to the sign of zero, which no
// result depends on: the validity tests, floorf / ceilf and 1 - frac are the same for +0 and -0).
__device__ __forceinline__ void axis_coeff(float lo, float hi, int extent, int crop, float *base, float *step)
{
    const float span = (float)(extent - 1);
    if (crop > 1) {
        const float d = hi - lo;
        const float m = d * span;
        *step = m / (float)(crop - 1);
        *base = lo * span;
    } else {
        const float s = lo + hi;
        const double dc = 0.5 * (double)s * (double)(extent - 1);
        *base = (float)dc;
        *step = 0.0f;
    }
}

__device__ __forceinline__ Tap tap_at(float c, int extent)
{
    const float span = (float)(extent - 1);
    Tap t;
    if (c < 0.0f || c > span) {
        t.valid = 0;
        t.i0 = 0;
        t.i1 = 0;
        t.frac = 0.0f;
    } else {
        t.valid = 1;
        t.i0 = (int)floorf(c);
        t.i1 = (int)ceilf(c);
        t.frac = c - (float)t.i0;  // via the int, as the reference: keeps -0.0 - 0 == -0.0
    }
    return t;
}

__device__ __forceinline__ Tap make_tap(float lo, float hi, int extent, int crop, int k)
{
    float base, step;
    axis_coeff(lo, hi, extent, crop, &base, &step);
    if (crop > 1) {
        const float off = (float)k * step;
        return tap_at(base + off, extent);
    }
    return tap_at(base, extent);
}

// Resolve the (uniform) per-workgroup box header.  Returns false when the box has
// no valid source (bad image index or level): the caller writes zeros.
struct BoxHeader {
    int lvl, H, W, img;
    float y1, x1, y2, x2;
};

template <typename LS>
__device__ __forceinline__ bool load_box(const LS &ls, const float *__restrict__ boxes,
                                         const int *__restrict__ box_ind,
                                         const int *__restrict__ level, int box, int batch,
                                         BoxHeader &h)
{
    h.lvl = level ? (level[box] - 2) : 0;
    h.img = box_ind[box];
    const bool ok = (h.lvl >= 0) && (h.lvl < ls.n) && (h.img >= 0) && (h.img < batch);
    if (!ok) return false;
    h.H = ls.H[h.lvl];
    h.W = ls.W[h.lvl];
    const float *b = boxes + 4 * (size_t)box;  // scalar loads: no alignment demand on callers
    h.y1 = b[0];
    h.x1 = b[1];
    h.y2 = b[2];
    h.x2 = b[3];
    return true;
}

}  // namespace
