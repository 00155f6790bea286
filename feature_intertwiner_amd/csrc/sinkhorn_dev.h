// sinkhorn_dev.h -- device code of the Sinkhorn kernels, shared by sinkhorn.hip (fi_sinkhorn_forward, libfi_hip.so)
// and sinkhorn_bp.hip (fi_ot_sinkhorn_backprop, libfi_ot.so): the thread layout, the LDS block, the cost tile, the two
// mat-vec reductions and the loss sum.  Both kernels go through THIS code, so the forward arithmetic of the second is the
// first's bit for bit: the same accumulation order per element, the same reduction trees, the same explicit fmafs.
//
// Layout: one 1024-thread workgroup (16 wavefronts) per problem, S <= 256.  Thread tid holds the 8 x 8 tile
// (ti, tj) = (tid >> 5, tid & 31) of an S x S matrix: lanes 0-31 of wavefront w hold row tile 2w, lanes 32-63 row tile 2w + 1.
#pragma once
#include "fi_common.h"

namespace fi_ot_dev {

constexpr int kThreads = 1024;
constexpr int kMaxS = 256;
constexpr int kT = 8;         // tile edge held per thread
constexpr int kDChunk = 16;   // feature columns staged per pass (D > 1)
constexpr int kStride = 260;  // LDS row stride of the staged, transposed chunk
#define FI_OT_EPS 1e-20f

// v (DPP-moved) with zero where the control selects no source lane
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_mov(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xF, true));
}

struct Smem {
    float a[kMaxS];
    float b[kMaxS];
    float nx[kMaxS];  // ||x_i|| + eps (cosine) -- divisor
    float ny[kMaxS];
    float red[16][kMaxS];
    float xs[kDChunk][kStride];
    float ys[kDChunk][kStride];
    float wsum[16];
};

// sm.nx / sm.ny = ||row|| + eps of x and y (cosine with the normaliser inside); ends with a barrier
__device__ __forceinline__ void row_norms(Smem &sm, const float *__restrict__ x, const float *__restrict__ y, int S, int D)
{
    const int tid = threadIdx.x;
    if (tid < 2 * kMaxS) {
        const int i = tid & (kMaxS - 1);
        const float *__restrict__ src = (tid < kMaxS) ? x : y;
        float ss = 0.0f;
        if (i < S)
            for (int d = 0; d < D; ++d) {
                const float v = src[(size_t)i * D + d];
                ss = fmaf(v, v, ss);
            }
        const float nrm = sqrtf(ss) + FI_OT_EPS;
        if (tid < kMaxS) sm.nx[i] = nrm; else sm.ny[i] = nrm;
    }
    __syncthreads();
}

// cost tile C[r][c] for rows ti*8+r, cols tj*8+c of problem (x, y).
__device__ void cost_tile(Smem &sm, const float *__restrict__ x, const float *__restrict__ y, int S,
                          int D, int l2_cost, int normalize, int ti, int tj, float (&C)[kT][kT])
{
    const int tid = threadIdx.x;
    float acc[kT][kT];
#pragma unroll
    for (int r = 0; r < kT; ++r)
#pragma unroll
        for (int c = 0; c < kT; ++c) acc[r][c] = 0.0f;

    for (int d0 = 0; d0 < D; d0 += kDChunk) {
        const int dc = min(kDChunk, D - d0);
        __syncthreads();  // previous chunk fully consumed
        for (int e = tid; e < kMaxS * kDChunk; e += kThreads) {
            const int i = e / kDChunk;
            const int d = e - i * kDChunk;
            float xv = 0.0f, yv = 0.0f;
            if (i < S && d < dc) {
                xv = x[(size_t)i * D + d0 + d];
                yv = y[(size_t)i * D + d0 + d];
                if (normalize) {  // x /= (||x|| + eps), OT_module.py:111-112
                    xv = xv / sm.nx[i];
                    yv = yv / sm.ny[i];
                }
            }
            sm.xs[d][i] = xv;
            sm.ys[d][i] = yv;
        }
        __syncthreads();
        for (int d = 0; d < dc; ++d) {
            float xr[kT], yc[kT];
#pragma unroll
            for (int r = 0; r < kT; ++r) xr[r] = sm.xs[d][ti * kT + r];
#pragma unroll
            for (int c = 0; c < kT; ++c) yc[c] = sm.ys[d][tj * kT + c];
#pragma unroll
            for (int r = 0; r < kT; ++r)
#pragma unroll
                for (int c = 0; c < kT; ++c) {
                    if (l2_cost) {
                        const float df = xr[r] - yc[c];
                        acc[r][c] = fmaf(df, df, acc[r][c]);
                    } else {
                        acc[r][c] = fmaf(xr[r], yc[c], acc[r][c]);
                    }
                }
        }
    }
#pragma unroll
    for (int r = 0; r < kT; ++r)
#pragma unroll
        for (int c = 0; c < kT; ++c) C[r][c] = l2_cost ? sqrtf(acc[r][c]) : (1.0f - acc[r][c]);
}

// K tile from the cost tile: exp(-eps_inv C) inside the S x S problem, 0 outside
__device__ __forceinline__ float gibbs_inside(float c, float eps_inv) { return expf(-eps_inv * c); }
__device__ __forceinline__ float gibbs(float c, float eps_inv, bool in) { return in ? gibbs_inside(c, eps_inv) : 0.0f; }

// the row of its tile whose full sum row_sum leaves in a lane
__device__ __forceinline__ int row_of_lane(int lane) { return ((lane & 1) << 2) | (lane & 2) | ((lane >> 2) & 1); }

// Reduce over the 32 lanes that share a row tile, HALVING the values a lane carries at every step: the pair
// (lane, partner) splits its rows -- the lower lane keeps the first half and is sent the partner's, the
// upper lane the second half -- so 8 values need 4 + 2 + 1 exchanges (quad_perm xor 1, xor 2, ds_swizzle xor 4: partners
// always carry the same rows), then the one value left is folded by row_ror:8 and ds_swizzle xor 16.
// Every lane ends with the FULL sum of one row, r = row_of_lane(lane), and the caller does ONE
// division.  (Before: five DPP steps on all 8 values, the sums in lane 31 only, which then did 8 divisions
// one after the other -- under an exec mask, so at the full cost for the wavefront: 136 instructions, now ~40.)
__device__ __forceinline__ float row_sum(const float (&part)[kT], int lane)
{
    float v4[4], v2[2], v;
    {
        const bool up = lane & 1;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float keep = up ? part[k + 4] : part[k], send = up ? part[k] : part[k + 4];
            v4[k] = keep + dpp_mov<0xB1, 0xF>(send);          // quad_perm [1,0,3,2]
        }
    }
    {
        const bool up = lane & 2;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const float keep = up ? v4[k + 2] : v4[k], send = up ? v4[k] : v4[k + 2];
            v2[k] = keep + dpp_mov<0x4E, 0xF>(send);          // quad_perm [2,3,0,1]
        }
    }
    {
        const bool up = lane & 4;
        const float keep = up ? v2[1] : v2[0], send = up ? v2[0] : v2[1];
        v = keep + __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(send), 0x101F));   // lane ^ 4
    }
    v += dpp_mov<0x128, 0xF>(v);                              // row_ror:8 = lane ^ 8
    v += __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x401F));   // lane ^ 16
    return v;
}

// (K vec)[ti*8 + row_of_lane(lane)] in every lane: 64 FMAs, then row_sum.  vec: an LDS vector indexed by column.
__device__ __forceinline__ float matvec_rows(const float (&K)[kT][kT], const float *vec, int tj, int lane)
{
    float bv[kT];
#pragma unroll
    for (int c = 0; c < kT; ++c) bv[c] = vec[tj * kT + c];
    float part[kT];
#pragma unroll
    for (int r = 0; r < kT; ++r) {
        float s = 0.0f;
#pragma unroll
        for (int c = 0; c < kT; ++c) s = fmaf(K[r][c], bv[c], s);
        part[r] = s;
    }
    return row_sum(part, lane);
}

// per-column partial sums of a wavefront's two row tiles into sm.red[wave]: lane l + lane l^32 in every lane
// (v_permlane32_swap: no LDS crossbar); col_sum after a barrier finishes the 16-way sum
__device__ __forceinline__ void stage_cols(Smem &sm, float (&part)[kT], int tj, int lane, int wave)
{
#pragma unroll
    for (int c = 0; c < kT; ++c) {
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_int(part[c]), __float_as_int(part[c]), false, false);
        part[c] = __int_as_float(sw[0]) + __int_as_float(sw[1]);
    }
    if (lane < 32) {
#pragma unroll
        for (int c = 0; c < kT; ++c) sm.red[wave][tj * kT + c] = part[c];
    }
}

// the column partials of K^T vec (vec: an LDS vector indexed by row) staged into sm.red
__device__ __forceinline__ void matvec_cols_stage(Smem &sm, const float (&K)[kT][kT], const float *vec, int ti, int tj,
                                                  int lane, int wave)
{
    float av[kT];
#pragma unroll
    for (int r = 0; r < kT; ++r) av[r] = vec[ti * kT + r];
    float part[kT];
#pragma unroll
    for (int c = 0; c < kT; ++c) {
        float s = 0.0f;
#pragma unroll
        for (int r = 0; r < kT; ++r) s = fmaf(K[r][c], av[r], s);
        part[c] = s;
    }
    stage_cols(sm, part, tj, lane, wave);
}

__device__ __forceinline__ float col_sum(const Smem &sm, int j)
{
    float s = 0.0f;
#pragma unroll
    for (int w = 0; w < 16; ++w) s += sm.red[w][j];
    return s;
}

// *out = the sum of `local` over the workgroup in a fixed order (butterfly inside a wavefront, then the 16 wavefronts
// in turn); holds one barrier
__device__ __forceinline__ void block_sum_to(Smem &sm, float local, int lane, int wave, float *out)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) local += __shfl_xor(local, off, 64);
    if (lane == 0) sm.wsum[wave] = local;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.0f;
        for (int w = 0; w < 16; ++w) s += sm.wsum[w];
        *out = s;
    }
}

}  // namespace fi_ot_dev
