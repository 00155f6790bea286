// cocomask.hip -- COCO polygon ground truth to RLE on the GPU (evaluation path, in front of cocoeval.hip).
//
// Specification: datasets/eval/common/maskApi.c `rleFrPoly` (:161-201) and `rleMerge` (:49-70), as COCO.annToRLE
// (pycocotools/coco.py:405-424) calls them.  Restatement: tests/cocopoly_ref.py; goldens from the reference's own
// code: tests/golden/cocopoly.npz.  Everything the reference computes in double is computed in double, one rounded
// operation at a time (-ffp-contract=off), and every (int) conversion truncates towards zero, as in the C.
//
// Launches (one workgroup of 256 per polygon / per group; nothing depends on the image size):
//   fi_cocomask_from_polygons  frpoly_kernel.  Each wave takes edges; its lanes take the upsampled points d = 1..n
//                       of the edge and recompute (u, v) of points d - 1 and d from the step index: the point list
//                       of the C is never materialised.  A boundary key x * h + y is appended (LDS atomic counter)
//                       where u changes.  The keys are sorted (bitonic network in which every exchange is ascending,
//                       so any length works without padding), in LDS up to FI_COCOMASK_LDS_KEYS and otherwise in
//                       the global workspace.  The C's "difference, cancel zero differences in pairs" is: a toggle at
//                       every distinct key < h * w of odd multiplicity; the counts are the differences of the
//                       toggles from 0, and a last count closes the mask at h * w.  So: the last key of each run of
//                       equal keys finds the run's start by bisection, a block scan ranks the odd runs, the toggles
//                       are written to the output and differenced in place.
//   fi_cocomask_merge   merge_kernel.  A group of one is a copy.  Otherwise every count but the last of every member
//                       becomes an event (position << 1 | switches-on); the events are sorted the same way, a block
//                       scan of +1 / -1 gives the coverage after each position, and a toggle is written where
//                       "covered" (coverage > 0 for the union, == members for the intersection) changes.
#include "fi_common.h"
#include "../../include/fi_cocomask.h"

#include <cmath>
#include <cstdlib>

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kLdsKeys = FI_COCOMASK_LDS_KEYS;
constexpr long long kMaxTotal = 1LL << 30;

// block-wide inclusive scan; `total` gets the sum
__device__ inline int block_scan(int v, int *s_wave, int &total)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) s_wave[wid] = x;
    __syncthreads();
    total = 0;
    for (int w = 0; w < kWaves; ++w) {
        const int s = s_wave[w];
        if (w < wid) x += s;
        total += s;
    }
    __syncthreads();
    return x;
}

// Ascending sort of a[0, n) (LDS or global) by the workgroup.  Bitonic merges whose first stage compares i with its
// mirror image in the block (i ^ (k - 1)): every exchange then puts the minimum at the lower index, so the elements
// past n, which would all be +inf, never move and are simply skipped.
__device__ inline void block_sort(uint32_t *a, int n)
{
    __syncthreads();
    for (long long k = 2; (k >> 1) < n; k <<= 1) {
        for (long long j = k - 1; j > 0; j = (j == k - 1) ? (k >> 2) : (j >> 1)) {
            for (long long i = threadIdx.x; i < n; i += kThreads) {
                const long long l = i ^ j;
                if (l > i && l < n) {
                    const uint32_t x = a[i], y = a[l];
                    if (x > y) {
                        a[i] = y;
                        a[l] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// the first index of the sorted a[0, n) whose element is >= key
__device__ inline int lower_bound(const uint32_t *a, int n, uint32_t key)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// out[0, nt) holds ascending toggle positions: turn them into counts in place and close the mask at hw.
// Chunks from the top, so that out[i - 1] is read before its own chunk is rewritten.  Returns the number of counts.
__device__ inline int toggles_to_counts(uint32_t *out, int nt, uint32_t hw)
{
    __syncthreads();
    const uint32_t last = nt ? out[nt - 1] : 0u;
    for (int c = (nt + kThreads - 1) / kThreads - 1; c >= 0; --c) {
        const int i = c * kThreads + (int)threadIdx.x;
        uint32_t cur = 0, prev = 0;
        if (i < nt) {
            cur = out[i];
            prev = i ? out[i - 1] : 0u;
        }
        __syncthreads();
        if (i < nt) out[i] = cur - prev;
        __syncthreads();
    }
    if (threadIdx.x == 0) out[nt] = hw - last;
    return nt + 1;
}

__device__ inline int scale5(double c) { return (int)(5.0 * c + .5); }

__global__ __launch_bounds__(kThreads) void frpoly_kernel(
    const double *__restrict__ xy, const long long *__restrict__ poly_off, const long long *__restrict__ sizes,
    const long long *__restrict__ key_off, long long *__restrict__ rles, uint32_t *__restrict__ counts,
    uint32_t *__restrict__ ws)
{
    __shared__ uint32_t s_keys[kLdsKeys];
    __shared__ int s_wave[kWaves];
    __shared__ unsigned s_n;
    const long long p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const long long v0 = poly_off[p], K = poly_off[p + 1] - v0;
    const long long h = sizes[p * 2], w = sizes[p * 2 + 1];
    const long long k0 = key_off[p];
    const long long cap_ll = key_off[p + 1] - k0;
    const unsigned cap = cap_ll < 0 ? 0u : (unsigned)(cap_ll < kMaxTotal ? cap_ll : kMaxTotal);
    uint32_t *keys = cap <= (unsigned)kLdsKeys ? s_keys : ws + k0;
    uint32_t *out = counts + k0 + p;
    if (tid == 0) s_n = 0;
    __syncthreads();
    const double hd = (double)h, wlast = (double)(w - 1);
    for (long long e = wid; e < K; e += kWaves) {
        const double *a = xy + (v0 + e) * 2, *b = xy + (v0 + (e + 1 == K ? 0 : e + 1)) * 2;
        int xs = scale5(a[0]), ys = scale5(a[1]), xe = scale5(b[0]), ye = scale5(b[1]);
        const int dx = abs(xe - xs), dy = abs(ye - ys);
        // dx == 0: u is the same at every point of the edge (slope 0, or 0 / 0 for a repeated vertex): no key.
        // The pair (last point of an edge, first point of the next) is one vertex and emits nothing either
        // (fi_cocomask.h), so the points of an edge are all that has to be looked at.
        if (dx == 0) continue;
        const bool xmajor = dx >= dy;
        const bool flip = xmajor ? xs > xe : ys > ye;
        if (flip) {
            int t = xs; xs = xe; xe = t;
            t = ys; ys = ye; ye = t;
        }
        const int n = xmajor ? dx : dy;
        const double s = xmajor ? (double)(ye - ys) / (double)dx : (double)(xe - xs) / (double)dy;
        for (int d = 1 + lane; d <= n; d += 64) {
            const int t0 = flip ? n - (d - 1) : d - 1, t1 = flip ? n - d : d;
            int u0, u1, w0, w1;                                 // (u, v) of points d - 1 and d
            if (xmajor) {
                u0 = t0 + xs;
                u1 = t1 + xs;
                w0 = (int)((double)ys + s * (double)t0 + .5);
                w1 = (int)((double)ys + s * (double)t1 + .5);
            } else {
                w0 = t0 + ys;
                w1 = t1 + ys;
                u0 = (int)((double)xs + s * (double)t0 + .5);
                u1 = (int)((double)xs + s * (double)t1 + .5);
            }
            if (u1 == u0) continue;
            double xd = (double)(u1 < u0 ? u1 : u1 - 1);
            xd = (xd + .5) / 5.0 - .5;
            if (floor(xd) != xd || xd < 0 || xd > wlast) continue;
            double yd = (double)(w1 < w0 ? w1 : w0);
            yd = (yd + .5) / 5.0 - .5;
            if (yd < 0) yd = 0; else if (yd > hd) yd = hd;
            yd = ceil(yd);
            const uint32_t key = (uint32_t)((int)xd * (int)h + (int)yd);
            const unsigned at = atomicAdd(&s_n, 1u);
            if (at < cap) keys[at] = key;                       // never beyond the bound (proof in fi_cocomask.h)
        }
    }
    __syncthreads();
    const int nk = (int)(s_n < cap ? s_n : cap);
    block_sort(keys, nk);
    const uint32_t hw = (uint32_t)(h * w);
    int nt = 0;
    for (int i0 = 0; i0 < nk; i0 += kThreads) {
        const int i = i0 + tid;
        int emit = 0;
        uint32_t key = 0;
        if (i < nk) {
            key = keys[i];
            if (key < hw && (i + 1 == nk || keys[i + 1] != key)) emit = (i - lower_bound(keys, i, key) + 1) & 1;
        }
        int tot;
        const int x = block_scan(emit, s_wave, tot);
        if (emit) out[nt + x - 1] = key;
        nt += tot;
    }
    const int m = toggles_to_counts(out, nt, hw);
    if (tid == 0) {
        long long *row = rles + p * 4;
        row[0] = k0 + p;
        row[1] = m;
        row[2] = h;
        row[3] = w;
    }
}

__global__ __launch_bounds__(kThreads) void merge_kernel(
    const long long *__restrict__ rles, const uint32_t *__restrict__ counts, const long long *__restrict__ group_off,
    const long long *__restrict__ out_off, int intersect, long long *__restrict__ out_rles,
    uint32_t *__restrict__ out_counts, uint32_t *__restrict__ ws)
{
    __shared__ uint32_t s_keys[kLdsKeys];
    __shared__ int s_wave[kWaves];
    const long long g = blockIdx.x;
    const int tid = threadIdx.x;
    const long long r0 = group_off[g], n = group_off[g + 1] - r0;
    const long long o0 = out_off[g];
    const long long cap_ll = out_off[g + 1] - o0;
    const int cap = cap_ll < 0 ? 0 : (int)(cap_ll < kMaxTotal ? cap_ll : kMaxTotal);
    uint32_t *out = out_counts + o0;
    long long *row = out_rles + g * 4;
    if (n <= 0) {
        if (tid == 0) {
            row[0] = o0;
            row[1] = row[2] = row[3] = 0;
        }
        return;
    }
    const long long h = rles[r0 * 4 + 2], w = rles[r0 * 4 + 3];
    if (n == 1) {
        const uint32_t *c = counts + rles[r0 * 4];
        long long m = rles[r0 * 4 + 1];
        m = m < 0 ? 0 : (m < cap ? m : cap);
        for (long long j = tid; j < m; j += kThreads) out[j] = c[j];
        if (tid == 0) {
            row[0] = o0;
            row[1] = m;
            row[2] = h;
            row[3] = w;
        }
        return;
    }
    int differ = 0;
    for (long long i = 1 + tid; i < n; i += kThreads)
        differ |= rles[(r0 + i) * 4 + 2] != h || rles[(r0 + i) * 4 + 3] != w;
    if (__syncthreads_or(differ) || cap < 2) {
        if (tid == 0) {
            row[0] = o0;
            row[1] = row[2] = row[3] = 0;
        }
        return;
    }
    // events: member i's count j < m - 1 ends at position c[0] + .. + c[j], where the mask switches on (j even) or off
    uint32_t *ev = cap <= kLdsKeys ? s_keys : ws + o0;
    long long ne_ll = 0;
    for (long long i = 0; i < n; ++i) {
        const uint32_t *c = counts + rles[(r0 + i) * 4];
        const long long m1 = rles[(r0 + i) * 4 + 1] - 1;
        uint32_t run = 0;
        for (long long j0 = 0; j0 < m1; j0 += kThreads) {
            const long long j = j0 + tid;
            int tot;
            const int x = block_scan(j < m1 ? (int)c[j] : 0, s_wave, tot);
            if (j < m1 && ne_ll + j < cap) ev[ne_ll + j] = ((run + (uint32_t)x) << 1) | (uint32_t)((j & 1) == 0);
            run += (uint32_t)tot;
        }
        if (m1 > 0) ne_ll += m1;
    }
    const int ne = (int)(ne_ll < cap ? ne_ll : cap);
    block_sort(ev, ne);
    const uint32_t hw = (uint32_t)(h * w);
    const int members = (int)n;
    int cov0 = 0, nt = 0;
    for (int i0 = 0; i0 < ne; i0 += kThreads) {
        const int i = i0 + tid;
        uint32_t e = 0;
        int d = 0;
        if (i < ne) {
            e = ev[i];
            d = (e & 1u) ? 1 : -1;
        }
        int tot;
        const int cov = cov0 + block_scan(d, s_wave, tot);      // the coverage after event i
        cov0 += tot;
        int emit = 0;
        const uint32_t pos = e >> 1;
        if (i < ne && pos < hw && (i + 1 == ne || (ev[i + 1] >> 1) != pos)) {
            // the events at `pos`: first those that switch off, then those that switch on
            const int lo0 = lower_bound(ev, i, pos << 1), lo1 = lower_bound(ev, i + 1, (pos << 1) | 1u);
            const int before = cov - ((i + 1 - lo1) - (lo1 - lo0));
            const bool in0 = intersect ? before == members : before > 0;
            const bool in1 = intersect ? cov == members : cov > 0;
            emit = in0 != in1;
        }
        const int x = block_scan(emit, s_wave, tot);
        if (emit && nt + x - 1 < cap - 1) out[nt + x - 1] = pos;
        nt += tot;
    }
    if (nt > cap - 1) nt = cap - 1;
    const int m = toggles_to_counts(out, nt, hw);
    if (tid == 0) {
        row[0] = o0;
        row[1] = m;
        row[2] = h;
        row[3] = w;
    }
}

}  // namespace

extern "C" {

int fi_cocomask_poly_bound(const double *xy, const long long *poly_off, long long num_polys, long long *bound)
{
    FI_REQUIRE(num_polys >= 0, "num_polys >= 0");
    if (num_polys == 0) return FI_OK;
    FI_REQUIRE(xy && poly_off && bound, "null pointer");
    for (long long p = 0; p < num_polys; ++p) {
        const long long v0 = poly_off[p], K = poly_off[p + 1] - v0;
        FI_REQUIRE(v0 >= 0 && K >= 1, "every polygon needs at least one vertex (poly_off ascending)");
        long long b = 0;
        for (long long e = 0; e < K; ++e) {
            const double x0 = xy[(v0 + e) * 2], y0 = xy[(v0 + e) * 2 + 1];
            // finite and small enough for (int)(5 * c + .5)
            FI_REQUIRE(std::fabs(x0) <= 1e8 && std::fabs(y0) <= 1e8, "coordinates finite and at most 1e8 in magnitude");
            const double x1 = xy[(v0 + (e + 1 == K ? 0 : e + 1)) * 2];
            FI_REQUIRE(std::fabs(x1) <= 1e8, "coordinates finite and at most 1e8 in magnitude");
            const long long dx = std::llabs((long long)(int)(5.0 * x1 + .5) - (long long)(int)(5.0 * x0 + .5));
            b += (dx + 4) / 5;
        }
        bound[p] = b;
    }
    return FI_OK;
}

size_t fi_cocomask_workspace_bytes(long long total_keys, long long num_items)
{
    if (total_keys <= 0 || num_items <= 0) return 0;
    return (size_t)total_keys * sizeof(uint32_t);
}

int fi_cocomask_from_polygons(const double *xy, const long long *poly_off, const long long *sizes,
                              const long long *key_off, long long num_polys, long long total_keys, long long *rles,
                              uint32_t *counts, void *workspace, fi_stream_t stream)
{
    FI_REQUIRE(num_polys >= 0 && num_polys < (1LL << 31), "0 <= num_polys < 2^31");
    FI_REQUIRE(total_keys >= 0 && total_keys < kMaxTotal, "0 <= total_keys < 2^30");
    if (num_polys == 0) return FI_OK;
    FI_REQUIRE(xy && poly_off && sizes && key_off && rles && counts, "null pointer");
    FI_REQUIRE(workspace || total_keys == 0, "null workspace");
    hipLaunchKernelGGL(frpoly_kernel, dim3((unsigned)num_polys), dim3(kThreads), 0, (hipStream_t)stream, xy, poly_off,
                       sizes, key_off, rles, counts, (uint32_t *)workspace);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int fi_cocomask_merge(const long long *rles, const uint32_t *counts, const long long *group_off,
                      const long long *out_off, long long num_groups, long long total_counts, int intersect,
                      long long *out_rles, uint32_t *out_counts, void *workspace, fi_stream_t stream)
{
    FI_REQUIRE(num_groups >= 0 && num_groups < (1LL << 31), "0 <= num_groups < 2^31");
    FI_REQUIRE(total_counts >= 0 && total_counts < kMaxTotal, "0 <= total_counts < 2^30");
    FI_REQUIRE(intersect == 0 || intersect == 1, "intersect is 0 or 1");
    if (num_groups == 0) return FI_OK;
    FI_REQUIRE(rles && counts && group_off && out_off && out_rles && out_counts, "null pointer");
    FI_REQUIRE(workspace || total_counts == 0, "null workspace");
    hipLaunchKernelGGL(merge_kernel, dim3((unsigned)num_groups), dim3(kThreads), 0, (hipStream_t)stream, rles, counts,
                       group_off, out_off, intersect, out_rles, out_counts, (uint32_t *)workspace);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

}  // extern "C"
