// sinkhorn.hip -- batched entropic-OT (Sinkhorn) term of the intertwiner loss, gfx950.
//
// Specification: OptTrans._sinkhorn_iterate, lib/OT_module.py:104-135 (oracle:
// orc_sinkhorn).  The reference evaluates each problem with 2L+6 tiny torch kernels
// inside a Python loop over classes and loss terms (up to 240 problems, :100-101).
//
// One launch solves every problem: one 1024-thread workgroup (16 wavefronts, one
// CU) per problem, S <= 256 samples.  The S x S Gibbs kernel K = exp(-C/eps) never
// touches memory: it lives in REGISTERS as a 32 x 32 grid of 8x8 tiles, one tile
// (64 VGPRs) per thread -- 256 KB of K would not fit the 160 KB LDS.  Each of the
// 2L dependent mat-vecs is then
//   K b   : 64 FMAs/thread, row sums reduced across the 32 lanes that share a row
//           tile (cross-lane shuffles inside a half-wavefront),
//   K^T a : 64 FMAs/thread, column sums reduced across row tiles: one xor-32
//           shuffle inside the wavefront, then a 16-way sum through LDS.
// The scaling vectors a, b live in LDS.  The cost matrix is recomputed for the
// final <P, C> instead of being held in 64 more registers.  The roofline that
// binds is on-chip (fp32 FMA issue + LDS/barrier latency); HBM traffic is 2*S*D
// floats in and 1 float out per problem.
// The device code (layout, LDS block, cost tile, reductions) is in sinkhorn_dev.h, which sinkhorn_bp.hip shares.
#include "sinkhorn_dev.h"

namespace {

using namespace fi_ot_dev;

__global__ __launch_bounds__(kThreads) void sinkhorn_kernel(const float *__restrict__ xs_all,
                                                            const float *__restrict__ ys_all, int S,
                                                            int D, float eps_inv, int L, int cost_mode,
                                                            float *__restrict__ loss,
                                                            float *__restrict__ plan,
                                                            float *__restrict__ xn_out,
                                                            float *__restrict__ yn_out)
{
    __shared__ Smem sm;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int tj = tid & 31;   // column tile
    const int ti = tid >> 5;   // row tile (lanes 0-31 and 32-63 of a wave hold ti = 2w, 2w+1)
    const size_t prob = blockIdx.x;
    const int l2_cost = (cost_mode == 1);
    const int normalize = (cost_mode == 0);  // mode 2: rows are already normalised
    const float *__restrict__ x = xs_all + prob * (size_t)S * D;
    const float *__restrict__ y = ys_all + prob * (size_t)S * D;

    // ---- row norms (cosine) ----------------------------------------------------
    if (normalize) {
        row_norms(sm, x, y, S, D);
        if (xn_out && yn_out) {
            for (int e = tid; e < S * D; e += kThreads) {
                const int i = e / D;
                xn_out[prob * (size_t)S * D + e] = x[e] / sm.nx[i];
                yn_out[prob * (size_t)S * D + e] = y[e] / sm.ny[i];
            }
        }
    }

    // ---- K tile in registers ------------------------------------------------------
    float K[kT][kT];
    {
        float C[kT][kT];
        cost_tile(sm, x, y, S, D, l2_cost, normalize, ti, tj, C);
#pragma unroll
        for (int r = 0; r < kT; ++r)
#pragma unroll
            for (int c = 0; c < kT; ++c)
                K[r][c] = gibbs(C[r][c], eps_inv, (ti * kT + r < S) && (tj * kT + c < S));
    }

    const float u = 1.0f / (float)S;
    if (tid < kMaxS) {
        sm.b[tid] = (tid < S) ? u : 0.0f;
        sm.a[tid] = (tid < S) ? u : 0.0f;
    }
    __syncthreads();

    for (int it = 0; it < L; ++it) {
        // ---- a = u / (K b + eps): row sums, one row and ONE division per lane (sinkhorn_dev.h, row_sum) ----
        {
            const float v = matvec_rows(K, sm.b, tj, lane);
            const int i = ti * kT + row_of_lane(lane);
            const float ai = u / (v + FI_OT_EPS);
            if ((tj & 24) == 0 && i < S) sm.a[i] = ai;
        }
        __syncthreads();
        // ---- b = u / (K^T a + eps): column sums through sm.red ------------------------
        matvec_cols_stage(sm, K, sm.a, ti, tj, lane, wave);
        __syncthreads();
        if (tid < kMaxS) {
            const float s = col_sum(sm, tid);
            if (tid < S) sm.b[tid] = u / (s + FI_OT_EPS);
        }
        __syncthreads();
    }

    // ---- P = a K b^T, loss = <P, C> -----------------------------------------------
    float C[kT][kT];
    cost_tile(sm, x, y, S, D, l2_cost, normalize, ti, tj, C);
    float local = 0.0f;
#pragma unroll
    for (int r = 0; r < kT; ++r) {
        const int i = ti * kT + r;
        const float ai = sm.a[i];
#pragma unroll
        for (int c = 0; c < kT; ++c) {
            const int j = tj * kT + c;
            const float ak = ai * K[r][c];
            const float p = ak * sm.b[j];
            if (i < S && j < S) {
                local = fmaf(p, C[r][c], local);
                if (plan) plan[prob * (size_t)S * S + (size_t)i * S + j] = p;
            }
        }
    }
    block_sum_to(sm, local, lane, wave, loss + prob);
}

}  // namespace

extern "C" {

int fi_sinkhorn_forward(const float *x, const float *y, int num_problems, int S, int D,
                        float eps_inv, int L, int cost_mode, float *loss, float *plan, float *xn_out,
                        float *yn_out, fi_stream_t stream)
{
    FI_REQUIRE(num_problems >= 0 && D >= 1 && L >= 1, "num_problems >= 0, D >= 1, L >= 1");
    FI_REQUIRE(cost_mode >= 0 && cost_mode <= 2, "cost_mode in {0 cosine, 1 l2, 2 dot}");
    if (S < 1 || S > kMaxS) {
        fi::set_error("fi_sinkhorn_forward supports 1 <= S <= %d samples (got %d)", kMaxS, S);
        return FI_ERR_UNSUPPORTED;
    }
    if (num_problems == 0) return FI_OK;
    FI_REQUIRE(x && y && loss, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    fi::ProfScope prof(FI_K_SINKHORN, st);
    hipLaunchKernelGGL(sinkhorn_kernel, dim3(num_problems), dim3(kThreads), 0, st, x, y, S, D,
                       eps_inv, L, cost_mode, loss, plan, xn_out, yn_out);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

}  // extern "C"
