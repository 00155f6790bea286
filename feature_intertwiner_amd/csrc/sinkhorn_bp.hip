// sinkhorn_bp.hip -- the Sinkhorn term differentiated THROUGH its L iterations (no_bp_P_L=False), gfx950.
//
// Specification: OptTrans._sinkhorn_iterate, lib/OT_module.py:104-135, without the detach of :129-131.
// fi_sinkhorn_forward (sinkhorn.hip) returns the plan P, which is d loss / d C only when P is a constant; this kernel
// returns d loss / d C of   loss = sum (a_L K b_L^T) o C,  K = exp(-eps_inv C),
//     b_0 = u = 1/S,  a_l = u / (K b_{l-1} + 1e-20),  b_l = u / (K^T a_l + 1e-20).
//
// One launch, one 1024-thread workgroup per problem, in four phases (layout and forward arithmetic: sinkhorn_dev.h, the
// code fi_sinkhorn_forward runs, so `loss` has its bits):
//   1 forward   K in registers (64 per thread), a_1..a_L and b_0..b_L written to the workspace; the cost tile C is
//               parked there too, in padded 256-float rows (K and a second 64-register tile cannot live together:
//               1024 threads are 4 wavefronts per SIMD, 128 registers per lane; fi_sinkhorn_forward, which
//               recomputes C next to K, pays for it with scratch);
//   2 seed      C read back and K rebuilt a row at a time:  loss,  abar = G b_L,  bbar = G^T a_L,  G = K o C;  then
//               the K tile is rebuilt whole for the sweep (no tile is live across the reductions in between);
//   3 sweep     for l = L..1:  ubar_l = -bbar o b_l^2 / u;  abar += K ubar_l  (row sums);
//                              vbar_l = -abar o a_l^2 / u;  bbar  = K^T vbar_l (column sums);  abar = 0
//               -- the forward's two mat-vecs on the same K, ubar_l and vbar_l written to the workspace;
//   4 update    K is dropped;  M = sum_l a_l ubar_l^T + vbar_l b_{l-1}^T  accumulates in its 64 registers from the 2L
//               saved vector pairs (128 FMAs per thread and iteration), then C is read back row by row,
//               K = exp(-eps_inv C) recomputed and  dC = P o (1 - eps_inv C) - eps_inv K o M  stored.
// No scratch.  No atomics; every reduction runs in a fixed order, so a problem's bits do not depend on its neighbours
// or on the run.  A thread reads back its own C rows and b_l entries; a_l in the sweep and the vectors of phase 4 come
// from other threads of the workgroup, behind barriers.
// Workspace per problem: (4 L + 1) vectors of 256 floats (entries >= S are written as zeros, so no phase masks them)
// and the 256 x 256 cost matrix.
#include "sinkhorn_dev.h"

#include "../../include/fi_ot.h"

namespace {

using namespace fi_ot_dev;

// a_1..a_L, b_0..b_L, ubar_1..ubar_L, vbar_1..vbar_L (256 floats each), then the 256 x 256 cost matrix
__host__ __device__ inline size_t ws_floats_per_problem(int L)
{
    return ((size_t)4 * (size_t)L + 1) * kMaxS + (size_t)kMaxS * kMaxS;
}

// The value exists in a register HERE: the compiler may not defer the arithmetic that makes it to its first use (it
// would carry the operands instead -- for a 64-register tile twice the registers -- and spill).  No instruction.
__device__ __forceinline__ void pin(float &v) { asm volatile("" : "+v"(v)); }

// one row of K from its row of C: gibbs() of sinkhorn_dev.h with its select written as a bit mask per row and per column
// (the same bits: the value or +0) -- 64 separate conditions would sit in scalar register pairs across the 64 exps
__device__ __forceinline__ void gibbs_row(const float (&cv)[kT], float eps_inv, int rm, const int (&cm)[kT], float (&k)[kT])
{
#pragma unroll
    for (int c = 0; c < kT; ++c) {
        k[c] = __int_as_float(__float_as_int(gibbs_inside(cv[c], eps_inv)) & (rm & cm[c]));
        pin(k[c]);
    }
}

struct Row8 {
    float4 lo, hi;
};
__device__ __forceinline__ void unpack(const Row8 &v, float (&f)[kT])
{
    f[0] = v.lo.x; f[1] = v.lo.y; f[2] = v.lo.z; f[3] = v.lo.w;
    f[4] = v.hi.x; f[5] = v.hi.y; f[6] = v.hi.z; f[7] = v.hi.w;
}

__global__ __launch_bounds__(kThreads) void sinkhorn_bp_kernel(const float *__restrict__ xs_all,
                                                               const float *__restrict__ ys_all, int S, int D,
                                                               float eps_inv, int L, int cost_mode,
                                                               float *__restrict__ loss, float *dcost,
                                                               float *ws_all)
{
    __shared__ Smem sm;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int tj = tid & 31;   // column tile
    const int ti = tid >> 5;   // row tile
    const size_t prob = blockIdx.x;
    const int l2_cost = (cost_mode == 1);
    const int normalize = (cost_mode == 0);
    const float *__restrict__ x = xs_all + prob * (size_t)S * D;
    const float *__restrict__ y = ys_all + prob * (size_t)S * D;
    // Workspace vectors: uniform pointers (scalar registers) indexed by 32-bit per-lane offsets.
    float *wA = ws_all + prob * ws_floats_per_problem(L);   // a_1 .. a_L
    float *wB = wA + (size_t)L * kMaxS;                         // b_0 .. b_L
    float *wU = wB + ((size_t)L + 1) * kMaxS;                   // ubar_1 .. ubar_L
    float *wV = wU + (size_t)L * kMaxS;                         // vbar_1 .. vbar_L
    float *wCall = wV + (size_t)L * kMaxS;                      // C, 256 x 256
    const unsigned utid = (unsigned)tid;
    const unsigned rows0 = (unsigned)(ti * kT), cols0 = (unsigned)(tj * kT);
    // this thread's 8 x 8 tile of the parked cost matrix: row r at wC + r * kMaxS, 8 floats (32-byte aligned)
    float *wC = wCall + (rows0 * kMaxS + cols0);

    if (normalize) row_norms(sm, x, y, S, D);

    // ---- phase 1: the forward, iterates kept; C parked in the workspace (padded rows: no masks, whole-row accesses) ----
    float K[kT][kT];
    {
        float C[kT][kT];
        cost_tile(sm, x, y, S, D, l2_cost, normalize, ti, tj, C);
        int cm[kT];
#pragma unroll
        for (int c = 0; c < kT; ++c) cm[c] = (tj * kT + c < S) ? -1 : 0;
#pragma unroll
        for (int r = 0; r < kT; ++r) {
            Row8 row;
            row.lo = make_float4(C[r][0], C[r][1], C[r][2], C[r][3]);
            row.hi = make_float4(C[r][4], C[r][5], C[r][6], C[r][7]);
            *reinterpret_cast<Row8 *>(wC + r * kMaxS) = row;
            gibbs_row(C[r], eps_inv, (ti * kT + r < S) ? -1 : 0, cm, K[r]);
            __builtin_amdgcn_sched_barrier(0);     // a row at a time: C[r] dies as K[r] appears (register budget)
        }
    }

    const float u = 1.0f / (float)S;
    if (tid < kMaxS) {
        const float b0 = (tid < S) ? u : 0.0f;
        sm.b[tid] = b0;
        sm.a[tid] = b0;
        wB[utid] = b0;
    }
    __syncthreads();

    for (int it = 0; it < L; ++it) {
        {
            const float v = matvec_rows(K, sm.b, tj, lane);
            const int i = ti * kT + row_of_lane(lane);
            const float ai = u / (v + FI_OT_EPS);
            if ((tj & 24) == 0 && i < S) sm.a[i] = ai;
        }
        __syncthreads();
        if (tid < kMaxS) (wA + (size_t)it * kMaxS)[utid] = sm.a[tid];          // sm.a[>= S] stays 0
        matvec_cols_stage(sm, K, sm.a, ti, tj, lane, wave);
        __syncthreads();
        if (tid < kMaxS) {
            const float s = col_sum(sm, tid);
            if (tid < S) sm.b[tid] = u / (s + FI_OT_EPS);
            (wB + ((size_t)it + 1) * kMaxS)[utid] = sm.b[tid];
        }
        __syncthreads();
    }

    // ---- phase 2: loss and the adjoints of a_L, b_L ----------------------------------------------------------------------
    // K is DROPPED here and rebuilt from the parked C, a row at a time (64 exps, the bits of phase 1), once for the sums
    // of this phase and once more as the tile of the sweep: no 64-register tile is live across the reductions between
    // the two loops, where the register allocator otherwise parks part of it in scratch for the whole kernel.
    // Outside the problem K = 0 and C is finite: p = g = 0, and fmaf(0, c, local) = local, so the loss sum has the bits
    // of fi_sinkhorn_forward's, which skips those elements.
    float aseed;          // (G b_L)[ti*8 + row_of_lane(lane)]
    float bbar = 0.0f;    // thread j < 256: the adjoint of b_l[j]
    {
        float local = 0.0f, rowp[kT], colp[kT], bv[kT];
        int cm[kT];
#pragma unroll
        for (int c = 0; c < kT; ++c) {
            colp[c] = 0.0f;
            bv[c] = sm.b[cols0 + c];
            cm[c] = (tj * kT + c < S) ? -1 : 0;
        }
#pragma unroll
        for (int r = 0; r < kT; ++r) {
            const float ai = sm.a[rows0 + r];
            float cv[kT], k[kT];
            unpack(*reinterpret_cast<const Row8 *>(wC + r * kMaxS), cv);
            gibbs_row(cv, eps_inv, (ti * kT + r < S) ? -1 : 0, cm, k);
            float s = 0.0f;
#pragma unroll
            for (int c = 0; c < kT; ++c) {
                const float ak = ai * k[c];
                const float p = ak * bv[c];
                local = fmaf(p, cv[c], local);
                const float g = k[c] * cv[c];
                s = fmaf(g, bv[c], s);
                colp[c] = fmaf(g, ai, colp[c]);
            }
            rowp[r] = s;
            pin(rowp[r]);                          // this row's sums exist now: its k and C die here
            pin(local);
#pragma unroll
            for (int c = 0; c < kT; ++c) pin(colp[c]);
            __builtin_amdgcn_sched_barrier(0);     // keep the loads of later rows behind this row's arithmetic
        }
        aseed = row_sum(rowp, lane);
        stage_cols(sm, colp, tj, lane, wave);
        block_sum_to(sm, local, lane, wave, loss + prob);          // its barrier also publishes sm.red
        if (tid < kMaxS) bbar = col_sum(sm, tid);
        pin(aseed);
        pin(bbar);
        // K again, for the sweep -- through a pointer the compiler knows nothing about, so that the rows are LOADED
        // again and not kept (with their exps) from the loop above
        const float *wC2 = wC;
        asm volatile("" : "+v"(wC2));
#pragma unroll
        for (int r = 0; r < kT; ++r) {
            float cv[kT];
            unpack(*reinterpret_cast<const Row8 *>(wC2 + r * kMaxS), cv);
            gibbs_row(cv, eps_inv, (ti * kT + r < S) ? -1 : 0, cm, K[r]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // ---- phase 3: the reverse sweep (sm.b carries ubar_l, sm.a carries vbar_l) -------------------------------------------
    for (int l = L; l >= 1; --l) {
        if (tid < kMaxS) {
            const float bl = (wB + (size_t)l * kMaxS)[utid];                    // this thread wrote it
            const float ub = -(bbar * bl * bl) / u;
            sm.b[tid] = ub;
            (wU + ((size_t)l - 1) * kMaxS)[utid] = ub;
        }
        __syncthreads();
        {
            float v = matvec_rows(K, sm.b, tj, lane);
            v += aseed;                                                          // abar = G b_L + K ubar_L at l = L,
            aseed = 0.0f;                                                        // K ubar_l after it
            const unsigned i = rows0 + (unsigned)row_of_lane(lane);
            const float al = (wA + ((size_t)l - 1) * kMaxS)[i];
            const float vb = -(v * al * al) / u;                                 // rows >= S: K = 0, a = 0
            if ((tj & 24) == 0) {
                sm.a[i] = vb;
                (wV + ((size_t)l - 1) * kMaxS)[i] = vb;
            }
        }
        __syncthreads();
        // (at l = 1 the column sums that follow are not used: b_0 is a constant.  One mat-vec in 2 L, and the loop
        // keeps a single exit.)
        matvec_cols_stage(sm, K, sm.a, ti, tj, lane, wave);
        __syncthreads();
        if (tid < kMaxS) bbar = col_sum(sm, tid);
    }

    // ---- phase 4: M from the saved pairs, then dC ------------------------------------------------------------------------
    float M[kT][kT];
#pragma unroll
    for (int r = 0; r < kT; ++r)
#pragma unroll
        for (int c = 0; c < kT; ++c) M[r][c] = 0.0f;
    for (int l = 0; l < L; ++l) {
        float av[kT], vv[kT], uv[kT], bv[kT];
        unpack(*reinterpret_cast<const Row8 *>(wA + (size_t)l * kMaxS + rows0), av);
        unpack(*reinterpret_cast<const Row8 *>(wV + (size_t)l * kMaxS + rows0), vv);
        unpack(*reinterpret_cast<const Row8 *>(wU + (size_t)l * kMaxS + cols0), uv);
        unpack(*reinterpret_cast<const Row8 *>(wB + (size_t)l * kMaxS + cols0), bv);     // b_{l-1} of step l
#pragma unroll
        for (int r = 0; r < kT; ++r)
#pragma unroll
            for (int c = 0; c < kT; ++c) {
                M[r][c] = fmaf(av[r], uv[c], M[r][c]);
                M[r][c] = fmaf(vv[r], bv[c], M[r][c]);
            }
    }
    if (tid < kMaxS) {                                                           // a_L, b_L back into LDS
        sm.a[tid] = (wA + ((size_t)L - 1) * kMaxS)[utid];
        sm.b[tid] = (wB + (size_t)L * kMaxS)[utid];
    }
    __syncthreads();
    // dC = P o (1 - eps_inv C) - eps_inv K o M from the parked C; K = exp(-eps_inv C) again, the bits of phase 1
    float *out = dcost + prob * (size_t)S * S;
    unsigned t3 = utid;
    asm volatile("" : "+v"(t3));                             // the tile's address made again from the thread index, so
    const float *wC3 = wCall + ((t3 >> 5) * (kT * kMaxS) + (t3 & 31) * kT);   // that no pointer is carried across the sweep
    const int nr = S - ti * kT, nc = S - tj * kT;            // rows / columns of the tile inside the problem
    float bv[kT];
#pragma unroll
    for (int c = 0; c < kT; ++c) bv[c] = sm.b[cols0 + c];
#pragma unroll
    for (int r = 0; r < kT; ++r) {
        const float ai = sm.a[rows0 + r];
        float cv[kT];
        unpack(*reinterpret_cast<const Row8 *>(wC3 + r * kMaxS), cv);
        const unsigned at = (rows0 + r) * (unsigned)S + cols0;
#pragma unroll
        for (int c = 0; c < kT; ++c) {
            const float k = gibbs_inside(cv[c], eps_inv);
            const float p = (ai * k) * bv[c];
            const float d = p * (1.0f - eps_inv * cv[c]) - (eps_inv * k) * M[r][c];
            if (r < nr && c < nc) out[at + c] = d;
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

}  // namespace

extern "C" {

size_t fi_ot_sinkhorn_backprop_workspace_bytes(int num_problems, int S, int L)
{
    if (num_problems < 0 || S < 1 || S > kMaxS || L < 1) return 0;
    return (size_t)num_problems * ws_floats_per_problem(L) * sizeof(float);
}

int fi_ot_sinkhorn_backprop(const float *x, const float *y, int num_problems, int S, int D, float eps_inv, int L,
                            int cost_mode, float *loss, float *dcost, void *workspace, size_t workspace_bytes,
                            fi_stream_t stream)
{
    FI_REQUIRE(num_problems >= 0 && D >= 1 && L >= 1, "num_problems >= 0, D >= 1, L >= 1");
    FI_REQUIRE(cost_mode >= 0 && cost_mode <= 2, "cost_mode in {0 cosine, 1 l2, 2 dot}");
    if (S < 1 || S > kMaxS) {
        fi::set_error("fi_ot_sinkhorn_backprop supports 1 <= S <= %d samples (got %d)", kMaxS, S);
        return FI_ERR_UNSUPPORTED;
    }
    if (num_problems == 0) return FI_OK;
    FI_REQUIRE(x && y && loss && dcost && workspace, "null pointer");
    FI_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace aligned to 16 bytes");
    FI_REQUIRE(workspace_bytes >= fi_ot_sinkhorn_backprop_workspace_bytes(num_problems, S, L),
               "workspace smaller than fi_ot_sinkhorn_backprop_workspace_bytes");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sinkhorn_bp_kernel, dim3(num_problems), dim3(kThreads), 0, st, x, y, S, D, eps_inv, L, cost_mode,
                       loss, dcost, (float *)workspace);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

}  // extern "C"
