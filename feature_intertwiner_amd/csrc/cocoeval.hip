// cocoeval.hip -- COCO detection evaluation (iouType bbox / segm, useCats = 1) on the GPU (evaluation path).
//
// Specification: datasets/eval/common/maskApi.c `rleArea` (:72-75), `rleIou` (:77-96), `bbIou` (:109-120),
// `rleToBbox` (:133-146) and datasets/eval/PythonAPI/pycocotools/cocoeval.py `computeIoU` (:161-188), `evaluateImg`
// (:233-311), `accumulate` (:313-417).  Restatement: tests/cocoeval_ref.py; goldens from the reference's own code:
// tests/golden/cocoeval.npz.  Everything the reference computes in double is computed in double, one rounded
// operation at a time (-ffp-contract=off), so the results are bit-equal.
//
// A "pair" is one (image, category) with at least one ground truth or detection.  The caller orders the pairs by
// (category, image), the ground truths of a pair in annotation order and its detections by descending score
// (stable), cut to maxDets[-1]; *_off are the exclusive scans of the per-pair counts.
//
// Launches (none depends on the number of images):
//   fi_coco_rle_stats   coco_rle_stats_kernel: one thread per RLE, rleToBbox and rleArea.
//   fi_coco_iou         coco_iou_kernel: one thread per (detection, ground truth) element of every pair (the pair is
//                       found by bisection of iou_off); bbIou, and for segm the rleIou walk where that is > 0.
//   fi_coco_match       coco_match_kernel: one wave per pair.  The wave first sorts the ground truths "ignored last"
//                       for each area range (ballot partition), then lane a*T + t runs the serial greedy matcher
//                       of (area range a, threshold t): the 40 problems of a pair walk the same IoU tile, so its
//                       loads are wave-wide broadcasts.  The matched state is the gt_match output itself (each lane
//                       reads back only what it wrote), so nothing is sized by the pair: no LDS, no limit on the
//                       ground truths or detections of a pair.
//   fi_coco_accumulate  coco_accumulate_kernel: one workgroup per (category, area range, maxDets, threshold).  Two
//                       chunked passes over the category's detections in global score order: forward block scans
//                       of tp / fp find, for every recall threshold, the first position whose recall reaches it;
//                       the backward pass rebuilds the prefix sums from the totals and carries the running maximum
//                       of the precision (the envelope) from the right.
#include "fi_common.h"
#include "../../include/fi_cocoeval.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxProblems = 64;      // T * A: one lane per (area range, threshold)
constexpr int kMaxRec = 1024;         // R: recall thresholds held in LDS
constexpr int kMaxM = 16;

struct Rle {
    const uint32_t *cnts;
    long long m;
    uint32_t h, w;
};

__device__ inline Rle rle_at(const uint32_t *counts, const long long *desc, long long i)
{
    Rle r;
    r.cnts = counts + desc[i * 4];
    r.m = desc[i * 4 + 1];
    r.h = (uint32_t)desc[i * 4 + 2];
    r.w = (uint32_t)desc[i * 4 + 3];
    return r;
}

__global__ __launch_bounds__(kThreads) void coco_rle_stats_kernel(
    const uint32_t *__restrict__ counts, const long long *__restrict__ desc, long long n, double *__restrict__ bbox,
    double *__restrict__ area)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const Rle r = rle_at(counts, desc, i);
    uint32_t a = 0;
    for (long long j = 1; j < r.m; j += 2) a += r.cnts[j];
    area[i] = (double)a;
    const long long m = (r.m / 2) * 2;
    double *bb = bbox + i * 4;
    if (m == 0 || r.h == 0) {                                     // h == 0 with runs is refused by the caller
        bb[0] = bb[1] = bb[2] = bb[3] = 0.0;
        return;
    }
    uint32_t xs = r.w, ys = r.h, xe = 0, ye = 0, cc = 0;
    for (long long j = 0; j < m; ++j) {
        cc += r.cnts[j];
        const uint32_t t = cc - (uint32_t)(j % 2), y = t % r.h, x = (t - y) / r.h;
        xs = min(xs, x);
        xe = max(xe, x);
        ys = min(ys, y);
        ye = max(ye, y);
    }
    bb[0] = (double)xs;
    bb[2] = (double)(uint32_t)(xe - xs + 1);
    bb[1] = (double)ys;
    bb[3] = (double)(uint32_t)(ye - ys + 1);
}

__device__ inline double bb_iou(const double *D, const double *G, bool crowd)
{
    const double ga = G[2] * G[3], da = D[2] * D[3];
    const double w = fmin(D[2] + D[0], G[2] + G[0]) - fmax(D[0], G[0]);
    if (w <= 0) return 0.0;
    const double h = fmin(D[3] + D[1], G[3] + G[1]) - fmax(D[1], G[1]);
    if (h <= 0) return 0.0;
    const double i = w * h;
    const double u = crowd ? da : da + ga - i;
    return i / u;
}

__device__ inline double rle_iou(const Rle &dt, const Rle &gt, bool crowd, double dt_area)
{
    if (dt.h != gt.h || dt.w != gt.w) return -1.0;
    uint32_t ca = dt.cnts[0], cb = gt.cnts[0], i = 0, u = 0, ct = 1;
    long long a = 1, b = 1;
    bool va = false, vb = false;
    while (ct > 0) {
        const uint32_t c = min(ca, cb);
        if (va || vb) {
            u += c;
            if (va && vb) i += c;
        }
        ct = 0;
        ca -= c;
        if (!ca && a < dt.m) {
            ca = dt.cnts[a++];
            va = !va;
        }
        ct += ca;
        cb -= c;
        if (!cb && b < gt.m) {
            cb = gt.cnts[b++];
            vb = !vb;
        }
        ct += cb;
    }
    if (i == 0)
        u = 1;
    else if (crowd)
        u = (uint32_t)dt_area;
    return (double)i / (double)u;
}

__global__ __launch_bounds__(kThreads) void coco_iou_kernel(
    long long P, const long long *__restrict__ dt_off, const long long *__restrict__ gt_off,
    const long long *__restrict__ iou_off, long long E, const double *__restrict__ dt_box,
    const double *__restrict__ gt_box, const uint8_t *__restrict__ gt_crowd, const long long *__restrict__ dt_rle,
    const uint32_t *__restrict__ dt_counts, const double *__restrict__ dt_rle_area,
    const long long *__restrict__ gt_rle, const uint32_t *__restrict__ gt_counts, double *__restrict__ ious)
{
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (e >= E) return;
    long long lo = 0, hi = P;                                      // the last pair with iou_off[p] <= e
    while (hi - lo > 1) {
        const long long mid = (lo + hi) / 2;
        if (iou_off[mid] <= e) lo = mid; else hi = mid;
    }
    const long long p = lo, G = gt_off[p + 1] - gt_off[p], r = e - iou_off[p];
    if (G <= 0 || r >= (dt_off[p + 1] - dt_off[p]) * G) return;    // inconsistent offsets: write nothing
    const long long d = dt_off[p] + r / G, g = gt_off[p] + r % G;
    const bool crowd = gt_crowd[g] != 0;
    double o = bb_iou(dt_box + d * 4, gt_box + g * 4, crowd);
    if (dt_counts && o > 0) o = rle_iou(rle_at(dt_counts, dt_rle, d), rle_at(gt_counts, gt_rle, g), crowd,
                                       dt_rle_area[d]);
    ious[e] = o;
}

__global__ __launch_bounds__(64) void coco_match_kernel(
    const long long *__restrict__ dt_off, const long long *__restrict__ gt_off, const long long *__restrict__ iou_off,
    const double *__restrict__ ious, const double *__restrict__ dt_area, const long long *__restrict__ dt_id,
    const double *__restrict__ gt_area, const uint8_t *__restrict__ gt_crowd, const long long *__restrict__ gt_id,
    const double *__restrict__ iou_thrs, const double *__restrict__ area_rng, int T, int A,
    long long *__restrict__ dt_match, uint8_t *__restrict__ dt_ignore, long long *__restrict__ gt_match,
    uint8_t *__restrict__ gt_ignore, int32_t *__restrict__ gt_order)
{
    const long long p = blockIdx.x;
    const int lane = threadIdx.x;
    const long long d0 = dt_off[p], g0 = gt_off[p], io = iou_off[p];
    const int D = (int)(dt_off[p + 1] - d0), G = (int)(gt_off[p + 1] - g0);
    const unsigned long long lt = (1ULL << lane) - 1ULL;
    // gtind = argsort(_ignore, mergesort): the regular ground truths first, each group in annotation order
    for (int a = 0; a < A; ++a) {
        const double lo = area_rng[a * 2], hi = area_rng[a * 2 + 1];
        int32_t *order = gt_order + g0 * A + (long long)a * G;
        int regular = 0;
        for (int base = 0; base < G; base += 64) {
            const int g = base + lane;
            const bool ig = g < G && (gt_crowd[g0 + g] != 0 || gt_area[g0 + g] < lo || gt_area[g0 + g] > hi);
            regular += __popcll(__ballot(g < G && !ig));
        }
        int nreg = 0, nign = 0;
        for (int base = 0; base < G; base += 64) {
            const int g = base + lane;
            const bool in = g < G;
            const bool ig = in && (gt_crowd[g0 + g] != 0 || gt_area[g0 + g] < lo || gt_area[g0 + g] > hi);
            const unsigned long long mr = __ballot(in && !ig), mi = __ballot(ig);
            if (in) {
                gt_ignore[(g0 + g) * A + a] = ig;
                order[ig ? regular + nign + __popcll(mi & lt) : nreg + __popcll(mr & lt)] = g;
            }
            nreg += __popcll(mr);
            nign += __popcll(mi);
        }
    }
    __threadfence_block();
    __syncthreads();
    if (lane >= A * T) return;
    const int a = lane / T, t = lane % T;
    const int32_t *order = gt_order + g0 * A + (long long)a * G;
    const double lo = area_rng[a * 2], hi = area_rng[a * 2 + 1];
    const double bar = fmin(iou_thrs[t], 1 - 1e-10);
    const long long AT = (long long)A * T, col = (long long)a * T + t;
    for (int g = 0; g < G; ++g) gt_match[(g0 + g) * AT + col] = 0;
    for (int d = 0; d < D; ++d) {
        double best = bar;
        int m = -1;
        bool m_ig = false;
        const double *row = ious + io + (long long)d * G;
        for (int pos = 0; pos < G; ++pos) {
            const int g = order[pos];
            // if this gt already matched, and not a crowd, continue
            if (gt_match[(g0 + g) * AT + col] != 0 && !gt_crowd[g0 + g]) continue;
            const bool ig = gt_ignore[(g0 + g) * A + a] != 0;
            // if dt matched to reg gt, and on ignore gt, stop
            if (m > -1 && !m_ig && ig) break;
            if (row[g] < best) continue;
            best = row[g];
            m = g;
            m_ig = ig;
        }
        const double ar = dt_area[d0 + d];
        dt_match[(d0 + d) * AT + col] = m >= 0 ? gt_id[g0 + m] : 0;
        dt_ignore[(d0 + d) * AT + col] = m >= 0 ? m_ig : (ar < lo || ar > hi);
        if (m >= 0) gt_match[(g0 + m) * AT + col] = dt_id[d0 + d];
    }
}

struct Tri {
    int keep, tp, fp;
};

// block-wide inclusive scan of three counters; `total` gets the sums
__device__ inline Tri block_scan3(Tri v, Tri *s_wave, Tri &total)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    Tri x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int k = __shfl_up(x.keep, o, 64), t = __shfl_up(x.tp, o, 64), f = __shfl_up(x.fp, o, 64);
        if (lane >= o) {
            x.keep += k;
            x.tp += t;
            x.fp += f;
        }
    }
    if (lane == 63) s_wave[wid] = x;
    __syncthreads();
    total = Tri{0, 0, 0};
    for (int w = 0; w < kWaves; ++w) {
        const Tri s = s_wave[w];
        if (w < wid) {
            x.keep += s.keep;
            x.tp += s.tp;
            x.fp += s.fp;
        }
        total.keep += s.keep;
        total.tp += s.tp;
        total.fp += s.fp;
    }
    __syncthreads();
    return x;
}

__global__ __launch_bounds__(kThreads) void coco_accumulate_kernel(
    int K, const long long *__restrict__ cat_dt_off, const long long *__restrict__ cat_gt_off,
    const long long *__restrict__ order, const int32_t *__restrict__ dt_rank, const double *__restrict__ dt_score,
    const long long *__restrict__ dt_match, const uint8_t *__restrict__ dt_ignore,
    const uint8_t *__restrict__ gt_ignore, const double *__restrict__ rec_thrs, const int32_t *__restrict__ max_dets,
    int T, int R, int A, int M, double *__restrict__ precision, double *__restrict__ recall,
    double *__restrict__ scores)
{
    __shared__ Tri s_wave[kWaves];
    __shared__ double s_dwave[kWaves];
    __shared__ long long s_at[kMaxRec];          // position (in `order`) of the recall threshold's precision
    __shared__ double s_val[kThreads];
    __shared__ int s_count[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int t = blockIdx.y;
    const int m = blockIdx.x % M, a = (blockIdx.x / M) % A, k = blockIdx.x / (M * A);
    const long long n0 = cat_dt_off[k], n1 = cat_dt_off[k + 1], g0 = cat_gt_off[k], g1 = cat_gt_off[k + 1];
    const long long AT = (long long)A * T, col = (long long)a * T + t;
    const long long rec_at = (((long long)t * K + k) * A + a) * M + m;
    auto cell = [&](int r) { return ((((long long)t * R + r) * K + k) * A + a) * M + m; };
    // npig: the ground truths of the category that are not ignored in this area range
    int c = 0;
    for (long long g = g0 + tid; g < g1; g += kThreads) c += gt_ignore[g * A + a] == 0;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) s_count[wid] = c;
    for (int r = tid; r < R; r += kThreads) s_at[r] = -1;
    __syncthreads();
    long long npig_i = 0;
    for (int w = 0; w < kWaves; ++w) npig_i += s_count[w];
    if ((n1 == n0 && g1 == g0) || npig_i == 0) {                  // no image of the category, or npig == 0
        if (tid == 0) recall[rec_at] = -1.0;
        for (int r = tid; r < R; r += kThreads) precision[cell(r)] = scores[cell(r)] = -1.0;
        return;
    }
    const double npig = (double)npig_i;
    const int cut = max_dets[m];
    auto flags = [&](long long j) {
        Tri v = {0, 0, 0};
        if (j < n1) {
            const long long idx = order[j];
            if (dt_rank[idx] < cut) {
                const bool ig = dt_ignore[idx * AT + col] != 0, mt = dt_match[idx * AT + col] != 0;
                v.keep = 1;
                v.tp = mt && !ig;
                v.fp = !mt && !ig;
            }
        }
        return v;
    };
    // forward: prefix sums; position j serves the thresholds in (rc[before j], rc[j]]  (searchsorted 'left')
    Tri base = {0, 0, 0};
    for (long long j0 = n0; j0 < n1; j0 += kThreads) {
        const long long j = j0 + tid;
        const Tri v = flags(j);
        Tri tot;
        Tri x = block_scan3(v, s_wave, tot);
        if (v.keep) {
            const int tp = base.tp + x.tp;
            const bool first = base.keep + x.keep == 1;
            if (first || v.tp) {
                const double cur = (double)tp / npig;
                int r = 0;
                if (!first) {
                    const double prev = (double)(tp - 1) / npig;
                    int lo = 0, hi = R;                              // the first threshold above prev
                    while (lo < hi) {
                        const int mid = (lo + hi) / 2;
                        if (rec_thrs[mid] > prev) hi = mid; else lo = mid + 1;
                    }
                    r = lo;
                }
                for (; r < R && rec_thrs[r] <= cur; ++r) s_at[r] = j;
            }
        }
        base.keep += tot.keep;
        base.tp += tot.tp;
        base.fp += tot.fp;
    }
    __syncthreads();
    const Tri total = base;
    if (tid == 0) recall[rec_at] = total.keep ? (double)total.tp / npig : 0.0;
    for (int r = tid; r < R; r += kThreads)
        if (s_at[r] < 0) precision[cell(r)] = scores[cell(r)] = 0.0;   // beyond the last recall: left at 0
    // backward: pr = tp / (fp + tp + spacing(1)) and its running maximum from the right
    const long long chunks = (n1 - n0 + kThreads - 1) / kThreads;
    Tri right = {0, 0, 0};
    double carry = -1.0;
    for (long long ch = chunks - 1; ch >= 0; --ch) {
        const long long j0 = n0 + ch * kThreads, j = j0 + tid;
        const Tri v = flags(j);
        Tri tot;
        Tri x = block_scan3(v, s_wave, tot);
        double pr = -1.0;
        if (v.keep) {
            const double tp = (double)(total.tp - right.tp - tot.tp + x.tp);
            const double fp = (double)(total.fp - right.fp - tot.fp + x.fp);
            pr = tp / (fp + tp + 2.220446049250313e-16);
        }
        double sm = pr;                                             // suffix maximum inside the wave
        for (int o = 1; o < 64; o <<= 1) {
            const double y = __shfl_down(sm, o, 64);
            if (lane + o < 64) sm = fmax(sm, y);
        }
        if (lane == 0) s_dwave[wid] = sm;
        __syncthreads();
        double after = carry;
        for (int w = kWaves - 1; w > wid; --w) after = fmax(after, s_dwave[w]);
        s_val[tid] = fmax(sm, after);
        double all = carry;
        for (int w = 0; w < kWaves; ++w) all = fmax(all, s_dwave[w]);
        carry = all;
        __syncthreads();
        for (int r = tid; r < R; r += kThreads) {
            const long long at = s_at[r];
            if (at >= j0 && at < j0 + kThreads) {
                precision[cell(r)] = s_val[at - j0];
                scores[cell(r)] = dt_score[order[at]];
            }
        }
        __syncthreads();
        right.tp += tot.tp;
        right.fp += tot.fp;
    }
}

int check_counts(int T, int A)
{
    FI_REQUIRE(T >= 1 && A >= 1, "T >= 1 and A >= 1");
    if ((long long)T * A > kMaxProblems) {
        fi::set_error("fi_coco supports T * A <= %d (iou thresholds x area ranges, one lane each; got %d x %d)",
                      kMaxProblems, T, A);
        return FI_ERR_UNSUPPORTED;
    }
    return FI_OK;
}

}  // namespace

extern "C" {

int fi_coco_rle_stats(const uint32_t *counts, const long long *rles, long long num_rles, double *bbox, double *area,
                      fi_stream_t stream)
{
    FI_REQUIRE(num_rles >= 0 && num_rles < (1LL << 31) * kThreads, "0 <= num_rles < 2^39");
    if (num_rles == 0) return FI_OK;
    FI_REQUIRE(counts && rles && bbox && area, "null pointer");
    const unsigned blocks = (unsigned)((num_rles + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(coco_rle_stats_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, counts, rles,
                       num_rles, bbox, area);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int fi_coco_iou(long long num_pairs, const long long *dt_off, const long long *gt_off, const long long *iou_off,
                long long num_elems, const double *dt_box, const double *gt_box, const uint8_t *gt_crowd,
                const long long *dt_rles, const uint32_t *dt_counts, const double *dt_rle_area,
                const long long *gt_rles, const uint32_t *gt_counts, double *ious, fi_stream_t stream)
{
    FI_REQUIRE(num_pairs >= 0 && num_elems >= 0, "num_pairs >= 0 and num_elems >= 0");
    FI_REQUIRE(num_elems < (1LL << 31) * kThreads, "num_elems < 2^39");
    if (num_elems == 0) return FI_OK;
    FI_REQUIRE(num_pairs >= 1, "num_elems > 0 needs num_pairs >= 1");
    FI_REQUIRE(dt_off && gt_off && iou_off && dt_box && gt_box && gt_crowd && ious, "null pointer");
    const bool segm = dt_rles || dt_counts || dt_rle_area || gt_rles || gt_counts;
    FI_REQUIRE(!segm || (dt_rles && dt_counts && dt_rle_area && gt_rles && gt_counts),
               "segm needs all five RLE arguments, bbox none of them");
    const unsigned blocks = (unsigned)((num_elems + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(coco_iou_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, num_pairs, dt_off,
                       gt_off, iou_off, num_elems, dt_box, gt_box, gt_crowd, dt_rles, dt_counts, dt_rle_area, gt_rles,
                       gt_counts, ious);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

size_t fi_coco_match_workspace_bytes(long long num_gt, int A)
{
    if (num_gt <= 0 || A <= 0) return 0;
    return (size_t)num_gt * A * sizeof(int32_t);
}

int fi_coco_match(long long num_pairs, const long long *dt_off, const long long *gt_off, const long long *iou_off,
                  const double *ious, const double *dt_area, const long long *dt_id, const double *gt_area,
                  const uint8_t *gt_crowd, const long long *gt_id, const double *iou_thrs, const double *area_rng,
                  int T, int A, long long *dt_match, uint8_t *dt_ignore, long long *gt_match, uint8_t *gt_ignore,
                  void *workspace, fi_stream_t stream)
{
    int rc = check_counts(T, A);
    if (rc != FI_OK) return rc;
    FI_REQUIRE(num_pairs >= 0 && num_pairs < (1LL << 31), "0 <= num_pairs < 2^31");
    if (num_pairs == 0) return FI_OK;
    FI_REQUIRE(dt_off && gt_off && iou_off && ious && dt_area && dt_id && gt_area && gt_crowd && gt_id && iou_thrs &&
                   area_rng && dt_match && dt_ignore && gt_match && gt_ignore && workspace, "null pointer");
    hipLaunchKernelGGL(coco_match_kernel, dim3((unsigned)num_pairs), dim3(64), 0, (hipStream_t)stream, dt_off, gt_off,
                       iou_off, ious, dt_area, dt_id, gt_area, gt_crowd, gt_id, iou_thrs, area_rng, T, A, dt_match,
                       dt_ignore, gt_match, gt_ignore, (int32_t *)workspace);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int fi_coco_accumulate(int K, const long long *cat_dt_off, const long long *cat_gt_off, const long long *order,
                       const int32_t *dt_rank, const double *dt_score, const long long *dt_match,
                       const uint8_t *dt_ignore, const uint8_t *gt_ignore, const double *rec_thrs,
                       const int32_t *max_dets, int T, int R, int A, int M, double *precision, double *recall,
                       double *scores, fi_stream_t stream)
{
    int rc = check_counts(T, A);
    if (rc != FI_OK) return rc;
    FI_REQUIRE(K >= 0 && R >= 1 && M >= 1, "K >= 0, R >= 1 and M >= 1");
    if (R > kMaxRec || M > kMaxM || T > 65535) {
        fi::set_error("fi_coco_accumulate supports R <= %d recall thresholds, M <= %d maxDets and T <= 65535 (got "
                      "R = %d, M = %d, T = %d)", kMaxRec, kMaxM, R, M, T);
        return FI_ERR_UNSUPPORTED;
    }
    FI_REQUIRE((long long)K * A * M < (1LL << 31), "K * A * M < 2^31");
    if (K == 0) return FI_OK;
    FI_REQUIRE(cat_dt_off && cat_gt_off && order && dt_rank && dt_score && dt_match && dt_ignore && gt_ignore &&
                   rec_thrs && max_dets && precision && recall && scores, "null pointer");
    hipLaunchKernelGGL(coco_accumulate_kernel, dim3((unsigned)(K * A * M), (unsigned)T), dim3(kThreads), 0,
                       (hipStream_t)stream, K, cat_dt_off, cat_gt_off, order, dt_rank, dt_score, dt_match, dt_ignore,
                       gt_ignore, rec_thrs, max_dets, T, R, A, M, precision, recall, scores);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

}  // extern "C"
