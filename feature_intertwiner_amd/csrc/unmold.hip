// unmold.hip -- inference detections to image-space boxes, full-image masks and COCO RLE (evaluation path).
//
// Specification: lib/workflow.py:523-600 `_unmold_detections` and :405-413, tools/image_utils.py:172-189
// `unmold_mask` (SciPy 1.0 imresize = bytescale + Pillow 8-bit BILINEAR resize, threshold, paste) and
// datasets/eval/common/maskApi.c `rleEncode` (:32-41) / `rleToString` (:203-215).  Restatement:
// tests/unmold_ref.py; goldens from the reference's own code: tests/golden/unmold.npz.
//
// Launches (fi_unmold_prepare = 1 + 2, fi_unmold_encode = 3, fi_unmold_paste = 4):
//   1. unmold_rows_kernel: one workgroup per image.  N (first class-0 row), float64 box transform, zero-area
//      filter and order-preserving compaction (ballot scan).
//   2. unmold_measure_kernel<false>: one workgroup per detection slot.  Bytescales the class mask into the
//      workspace and walks the box in column-major (RLE) order to count the runs and the string characters.
//   3. unmold_measure_kernel<true>: the same walk, writing the counts and the characters at caller offsets.
//   4. unmold_paste_kernel: dense [n, H, W] uint8 masks, 16 bytes per thread.
//
// The walk.  The mask is 0 outside the (clipped) box, so a run boundary at linear position q = x*H + y
// (v(q) != v(q-1), v(-1) = 0) can only fall on a box pixel or on the first pixel after a box column.  Each
// column of the clipped box therefore has ch + 1 candidate slots: its ch box pixels and the "after" slot
// x*H + cy2.  When cy2 == H the after slot is the top of the next column: it does not exist past the last
// image column, and it is that column's first box pixel (counted there) when cy1 == 0 and the box continues.
// A tile of 256 candidates is ranked with a block scan; the last three boundaries of earlier tiles are carried,
// because count i is T_i - T_{i-1} and rleToString codes it as cnts[i] - cnts[i-2] for i > 2.
//
// Every resized pixel is recomputed from the 28x28 bytes (Pillow's coefficients in double, 22-bit integer
// weights, horizontal pass first), so no LDS or workspace is sized by the image.
#include "fi_common.h"
#include "../../include/fi_eval.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxMask = 64;
constexpr int kMaxImage = 4096;
constexpr int kPrecision = 22;

enum : int { kStatusClass = 1, kStatusWindow = 2 };

__device__ inline double tent(double x)
{
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}

// Pillow precompute_coeffs (bilinear, support 1) for one output index; the weights are recomputed per tap.
struct Taps {
    int lo, n;
    double center, ss, ww;
};

__device__ inline Taps taps(int out_idx, int in_size, int out_size)
{
    Taps t;
    const double scale = (double)in_size / (double)out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * fs;
    t.center = (out_idx + 0.5) * scale;
    t.ss = 1.0 / fs;
    int xmin = (int)(t.center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(t.center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    t.lo = xmin;
    t.n = xmax - xmin;
    double ww = 0.0;
    for (int k = 0; k < t.n; ++k) ww += tent((k + xmin - t.center + 0.5) * t.ss);
    t.ww = ww;
    return t;
}

__device__ inline int weight(const Taps &t, int k)           // normalize_coeffs_8bpc
{
    double w = tent((k + t.lo - t.center + 0.5) * t.ss);
    if (t.ww != 0.0) w /= t.ww;
    return (int)(0.5 + w * (double)(1 << kPrecision));
}

__device__ inline int clip8(int acc)
{
    const int v = acc >> kPrecision;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// Pillow Image.resize((w, h), BILINEAR) of the mh x mw 'L' image `s`, output pixel (r, c).
__device__ int resized_px(const uint8_t *s, int mh, int mw, int h, int w, int r, int c)
{
    const bool hpass = (w != mw), vpass = (h != mh);
    Taps tx;
    int wx[4] = {0, 0, 0, 0};
    if (hpass) {
        tx = taps(c, mw, w);
        for (int k = 0; k < 4 && k < tx.n; ++k) wx[k] = weight(tx, k);
    }
    auto hrow = [&](int rr) -> int {
        const uint8_t *row = s + rr * mw;
        if (!hpass) return row[c];
        int acc = 1 << (kPrecision - 1);
        for (int k = 0; k < tx.n; ++k) acc += (int)row[tx.lo + k] * (k < 4 ? wx[k] : weight(tx, k));
        return clip8(acc);
    };
    if (!vpass) return hrow(r);
    const Taps ty = taps(r, mh, h);
    int acc = 1 << (kPrecision - 1);
    for (int k = 0; k < ty.n; ++k) acc += hrow(ty.lo + k) * weight(ty, k);
    return clip8(acc);
}

struct Box {
    int y1, x1, y2, x2;
};

// mask value (0/1) of image pixel (y, x), which must lie inside the box
__device__ inline int mask_at(const uint8_t *s, int mh, int mw, const Box &b, int y, int x)
{
    return resized_px(s, mh, mw, b.y2 - b.y1, b.x2 - b.x1, y - b.y1, x - b.x1) >= 128;
}

__device__ inline int32_t to_int32(double v)          // numpy astype(int32) on x86-64: out of range -> INT_MIN
{
    return (v >= -2147483648.0 && v < 2147483648.0) ? (int32_t)v : INT32_MIN;
}

// block-wide exclusive scan of one int per thread; `total` gets the sum
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
    int base = 0;
    total = 0;
    for (int w = 0; w < kWaves; ++w) {
        const int t = s_wave[w];
        if (w < wid) base += t;
        total += t;
    }
    __syncthreads();
    return base + x - v;
}

__device__ inline int str_chars(long long x)           // rleToString characters of one (delta-coded) count
{
    int n = 0;
    bool more = true;
    while (more) {
        const int c = (int)(x & 0x1f);
        x >>= 5;
        more = (c & 0x10) ? x != -1 : x != 0;
        ++n;
    }
    return n;
}

__device__ inline void str_write(long long x, uint8_t *dst)
{
    bool more = true;
    while (more) {
        int c = (int)(x & 0x1f);
        x >>= 5;
        more = (c & 0x10) ? x != -1 : x != 0;
        if (more) c |= 0x20;
        *dst++ = (uint8_t)(c + 48);
    }
}

__global__ __launch_bounds__(kThreads) void unmold_rows_kernel(
    const float *__restrict__ det, const int32_t *__restrict__ image_hw, const float *__restrict__ windows, int D,
    int K, int32_t *__restrict__ boxes, int32_t *__restrict__ class_ids, float *__restrict__ scores,
    int32_t *__restrict__ num_valid, int32_t *__restrict__ src_row, int32_t *__restrict__ dev_status)
{
    __shared__ int s_first;
    __shared__ int s_wave[kWaves];
    const int b = blockIdx.x;
    const float *d = det + (size_t)b * D * 6;
    if (threadIdx.x == 0) s_first = D;
    __syncthreads();
    for (int i = threadIdx.x; i < D; i += kThreads)
        if (d[i * 6 + 4] == 0.0f) atomicMin(&s_first, i);
    __syncthreads();
    const float *win = windows + b * 4;
    const double H = image_hw[b * 2], W = image_hw[b * 2 + 1];
    const double wy1 = win[0], wx1 = win[1], wy2 = win[2], wx2 = win[3];
    int N = s_first;
    if (!(wy2 - wy1 > 0.0) || !(wx2 - wx1 > 0.0)) {              // the reference divides by the window extent
        if (threadIdx.x == 0 && N > 0 && dev_status) atomicOr(dev_status, kStatusWindow);
        N = 0;
    }
    const double hs = H / (wy2 - wy1), ws = W / (wx2 - wx1);
    const double scale = hs < ws ? hs : ws;
    int base = 0;
    for (int i0 = 0; i0 < N; i0 += kThreads) {
        const int i = i0 + threadIdx.x;
        int keep = 0;
        int32_t bx[4];
        if (i < N) {
            const float *r = d + i * 6;
            bx[0] = to_int32(((double)r[0] - wy1) * scale);
            bx[1] = to_int32(((double)r[1] - wx1) * scale);
            bx[2] = to_int32(((double)r[2] - wy1) * scale);
            bx[3] = to_int32(((double)r[3] - wx1) * scale);
            const long long h = (long long)bx[2] - bx[0], w = (long long)bx[3] - bx[1];
            keep = h > 0 && w > 0 && h <= INT32_MAX && w <= INT32_MAX;     // no int overflow
        }
        int total;
        const int rank = block_scan(keep, s_wave, total);
        if (keep) {
            const float *r = d + i * 6;
            const int o = b * D + base + rank;
            for (int k = 0; k < 4; ++k) boxes[o * 4 + k] = bx[k];
            const int c = (int)r[4];
            class_ids[o] = c;
            scores[o] = r[5];
            src_row[o] = i;
            if ((c < 0 || c >= K) && dev_status) atomicOr(dev_status, kStatusClass);
        }
        base += total;
    }
    if (threadIdx.x == 0) num_valid[b] = base;
}

struct Slot {
    Box box;
    int H, W;
};

template <bool WRITE>
__global__ __launch_bounds__(kThreads) void unmold_measure_kernel(
    const float *__restrict__ mrcnn_mask, const int32_t *__restrict__ image_hw, const int32_t *__restrict__ boxes,
    const int32_t *__restrict__ class_ids, const int32_t *__restrict__ num_valid, const int32_t *__restrict__ src_row,
    int D, int K, int mh, int mw, uint8_t *__restrict__ scaled, long long *__restrict__ sizes,
    const long long *__restrict__ offsets, uint32_t *__restrict__ counts, uint8_t *__restrict__ strings)
{
    __shared__ uint8_t s_mask[kMaxMask * kMaxMask];
    __shared__ float s_red[2][kWaves];
    __shared__ int s_wave[kWaves];
    __shared__ int s_cur[kThreads];
    __shared__ int s_tp[3 + kThreads];
    const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int slot = b * D + j;
    const int M = mh * mw;
    uint8_t *sc = scaled + (size_t)slot * M;
    if (j >= num_valid[b]) {
        if (!WRITE && tid == 0) sizes[slot * 2] = sizes[slot * 2 + 1] = 0;
        return;
    }
    if (!WRITE) {
        // SciPy 1.0 bytescale of mrcnn_mask[b, src, class] (fp32, every operation rounded)
        const int c = class_ids[slot];
        const bool ok = c >= 0 && c < K;
        const float *m = mrcnn_mask + (((size_t)b * D + src_row[slot]) * K + (ok ? c : 0)) * M;
        float lo = INFINITY, hi = -INFINITY;
        for (int e = tid; e < M; e += kThreads) {
            const float v = ok ? m[e] : 0.0f;
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
        }
        for (int o = 32; o > 0; o >>= 1) {
            lo = fminf(lo, __shfl_xor(lo, o, 64));
            hi = fmaxf(hi, __shfl_xor(hi, o, 64));
        }
        if ((tid & 63) == 0) {
            s_red[0][tid >> 6] = lo;
            s_red[1][tid >> 6] = hi;
        }
        __syncthreads();
        float cmin = s_red[0][0], cmax = s_red[1][0];
        for (int w = 1; w < kWaves; ++w) {
            cmin = fminf(cmin, s_red[0][w]);
            cmax = fmaxf(cmax, s_red[1][w]);
        }
        float cscale = cmax - cmin;
        if (cscale == 0.0f) cscale = 1.0f;
        const float scale = (float)(255.0 / (double)cscale);       // == the IEEE fp32 division
        for (int e = tid; e < M; e += kThreads) {
            float v = ((ok ? m[e] : 0.0f) - cmin) * scale;
            v = fminf(fmaxf(v, 0.0f), 255.0f) + 0.5f;
            const uint8_t u = (uint8_t)(int)v;
            s_mask[e] = u;
            sc[e] = u;
        }
    } else {
        for (int e = tid; e < M; e += kThreads) s_mask[e] = sc[e];
    }
    Box bx;
    bx.y1 = boxes[slot * 4 + 0];
    bx.x1 = boxes[slot * 4 + 1];
    bx.y2 = boxes[slot * 4 + 2];
    bx.x2 = boxes[slot * 4 + 3];
    const int H = image_hw[b * 2], W = image_hw[b * 2 + 1];
    const int cy1 = max(bx.y1, 0), cy2 = min(bx.y2, H), cx1 = max(bx.x1, 0), cx2 = min(bx.x2, W);
    const int ch = cy2 - cy1, cw = cx2 - cx1;
    const long long C = (ch > 0 && cw > 0) ? (long long)cw * (ch + 1) : 0;
    const long long coff = WRITE ? offsets[slot * 2] : 0, soff = WRITE ? offsets[slot * 2 + 1] : 0;
    if (tid < 3) s_tp[tid] = 0;                                    // T_{-1} = 0 (the other two are never read)
    __syncthreads();
    long long ntrans = 0, nchars = 0;
    for (long long t0 = 0; t0 < C; t0 += kThreads) {
        const long long t = t0 + tid;
        int flag = 0, q = 0, cur = -1;
        int x = 0, s = 0;
        if (t < C) {
            x = cx1 + (int)(t / (ch + 1));
            s = (int)(t % (ch + 1));
            if (s < ch) cur = mask_at(s_mask, mh, mw, bx, cy1 + s, x);
        }
        s_cur[tid] = cur;
        __syncthreads();
        if (t < C) {
            int prev = 0;
            bool cand = true;
            if (s < ch) {
                q = x * H + cy1 + s;
                if (s > 0)
                    prev = tid > 0 ? s_cur[tid - 1] : mask_at(s_mask, mh, mw, bx, cy1 + s - 1, x);
                else if (cy1 == 0 && cy2 == H && x - 1 >= cx1)
                    prev = mask_at(s_mask, mh, mw, bx, H - 1, x - 1);  // bottom of the previous box column
            } else {
                cur = 0;
                if (cy2 < H) {
                    q = x * H + cy2;
                } else {
                    q = (x + 1) * H;
                    cand = (x + 1 < W) && !(cy1 == 0 && x + 1 < cx2);
                }
                prev = tid > 0 ? s_cur[tid - 1] : mask_at(s_mask, mh, mw, bx, cy2 - 1, x);
            }
            flag = cand && cur != prev;
        }
        int total;
        const int rank = block_scan(flag, s_wave, total);
        if (flag) s_tp[3 + rank] = q;
        __syncthreads();
        int len = 0;
        long long code = 0;
        if (flag) {
            const long long i = ntrans + rank;
            const long long cnt = (long long)s_tp[3 + rank] - s_tp[2 + rank];
            code = i > 2 ? cnt - ((long long)s_tp[1 + rank] - s_tp[rank]) : cnt;
            len = str_chars(code);
            if (WRITE) counts[coff + i] = (uint32_t)cnt;
        }
        int tile_chars;
        const int cpos = block_scan(len, s_wave, tile_chars);
        if (WRITE && flag) str_write(code, strings + soff + nchars + cpos);
        if (tid == 0) {
            const int a = s_tp[total], bb = s_tp[total + 1], cc = s_tp[total + 2];
            s_tp[0] = a;
            s_tp[1] = bb;
            s_tp[2] = cc;
        }
        ntrans += total;
        nchars += tile_chars;
        __syncthreads();
    }
    if (tid == 0) {                                                // the last run ends at H*W
        const long long i = ntrans;
        const long long cnt = (long long)H * W - s_tp[2];
        const long long code = i > 2 ? cnt - ((long long)s_tp[1] - s_tp[0]) : cnt;
        if (WRITE) {
            counts[coff + i] = (uint32_t)cnt;
            str_write(code, strings + soff + nchars);
        } else {
            sizes[slot * 2] = ntrans + 1;
            sizes[slot * 2 + 1] = nchars + str_chars(code);
        }
    }
}

constexpr int kPasteBytes = 16;

__global__ __launch_bounds__(kThreads) void unmold_paste_kernel(
    const int32_t *__restrict__ image_hw, const int32_t *__restrict__ boxes, const int32_t *__restrict__ num_valid,
    int batch, int D, int mh, int mw, const uint8_t *__restrict__ scaled, long long total, uint8_t *__restrict__ out)
{
    const long long f0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * kPasteBytes;
    if (f0 >= total) return;
    // locate byte f0: image b, detection j, pixel (y, x)
    int b = 0;
    long long rem = f0;
    for (; b < batch; ++b) {
        const long long sz = (long long)num_valid[b] * image_hw[b * 2] * image_hw[b * 2 + 1];
        if (rem < sz) break;
        rem -= sz;
    }
    if (b >= batch) return;                                        // total_bytes larger than the masks: no work
    int H = image_hw[b * 2], W = image_hw[b * 2 + 1];
    const long long hw = (long long)H * W;
    int j = (int)(rem / hw);
    const int pix = (int)(rem - (long long)j * hw);
    int y = pix / W, x = pix - y * W;
    union {
        uint8_t u8[kPasteBytes];
        uint4 v;
    } buf;
    buf.v = make_uint4(0, 0, 0, 0);
    const int nb = (int)min((long long)kPasteBytes, total - f0);
    int slot = -1;
    Box bx = {0, 0, 0, 0};
    const uint8_t *s = nullptr;
    for (int k = 0; k < nb; ++k) {
        if (b * D + j != slot) {
            slot = b * D + j;
            bx.y1 = boxes[slot * 4 + 0];
            bx.x1 = boxes[slot * 4 + 1];
            bx.y2 = boxes[slot * 4 + 2];
            bx.x2 = boxes[slot * 4 + 3];
            s = scaled + (size_t)slot * mh * mw;
        }
        const bool in = y >= bx.y1 && y < bx.y2 && x >= bx.x1 && x < bx.x2;
        buf.u8[k] = in ? (uint8_t)mask_at(s, mh, mw, bx, y, x) : 0;
        if (++x == W) {
            x = 0;
            if (++y == H) {
                y = 0;
                if (++j == num_valid[b]) {                        // next image with detections
                    j = 0;
                    do {
                        ++b;
                    } while (b < batch && num_valid[b] == 0);
                    if (b >= batch) break;
                    H = image_hw[b * 2];
                    W = image_hw[b * 2 + 1];
                }
            }
        }
    }
    if (nb == kPasteBytes) {
        *reinterpret_cast<uint4 *>(out + f0) = buf.v;
    } else {
        for (int k = 0; k < nb; ++k) out[f0 + k] = buf.u8[k];
    }
}

int check_sizes(const int32_t *image_hw_host, int batch, int D, int K, int mh, int mw)
{
    FI_REQUIRE(batch >= 0 && D >= 1 && K >= 1, "batch >= 0, num_dets >= 1, num_classes >= 1");
    if (mh < 1 || mw < 1 || mh > kMaxMask || mw > kMaxMask) {
        fi::set_error("fi_unmold supports masks of 1..%d x 1..%d (got %d x %d)", kMaxMask, kMaxMask, mh, mw);
        return FI_ERR_UNSUPPORTED;
    }
    if ((long long)batch * D > (1LL << 24)) {
        fi::set_error("fi_unmold supports batch * num_dets <= 2^24 (got %lld)", (long long)batch * D);
        return FI_ERR_UNSUPPORTED;
    }
    FI_REQUIRE(batch == 0 || image_hw_host, "null image_hw_host");
    for (int b = 0; b < batch; ++b) {
        const int H = image_hw_host[b * 2], W = image_hw_host[b * 2 + 1];
        if (H < 1 || W < 1 || H > kMaxImage || W > kMaxImage) {
            fi::set_error("fi_unmold supports images of 1..%d px per side (image %d is %d x %d)", kMaxImage, b, H,
                          W);
            return FI_ERR_UNSUPPORTED;
        }
    }
    return FI_OK;
}

}  // namespace

extern "C" {

size_t fi_unmold_workspace_bytes(int batch, int num_dets, int mask_h, int mask_w)
{
    if (batch <= 0 || num_dets <= 0 || mask_h <= 0 || mask_w <= 0) return 0;
    const size_t slots = (size_t)batch * num_dets;
    return ((slots * sizeof(int32_t) + 255) & ~(size_t)255) + slots * mask_h * mask_w;
}

int fi_unmold_prepare(const float *detections, const float *mrcnn_mask, const int32_t *image_hw,
                      const int32_t *image_hw_host, const float *windows, int batch, int num_dets, int num_classes,
                      int mask_h, int mask_w, int32_t *boxes, int32_t *class_ids, float *scores, int32_t *num_valid,
                      long long *sizes, int32_t *dev_status, void *workspace, fi_stream_t stream)
{
    int rc = check_sizes(image_hw_host, batch, num_dets, num_classes, mask_h, mask_w);
    if (rc != FI_OK) return rc;
    if (batch == 0) return FI_OK;
    FI_REQUIRE(detections && mrcnn_mask && image_hw && windows && boxes && class_ids && scores && num_valid && sizes &&
                   workspace, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    const size_t slots = (size_t)batch * num_dets;
    int32_t *src_row = (int32_t *)workspace;
    uint8_t *scaled = (uint8_t *)workspace + ((slots * sizeof(int32_t) + 255) & ~(size_t)255);
    hipLaunchKernelGGL(unmold_rows_kernel, dim3(batch), dim3(kThreads), 0, st, detections, image_hw, windows,
                       num_dets, num_classes, boxes, class_ids, scores, num_valid, src_row, dev_status);
    FI_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(unmold_measure_kernel<false>, dim3(num_dets, batch), dim3(kThreads), 0, st, mrcnn_mask,
                       image_hw, boxes, class_ids, num_valid, src_row, num_dets, num_classes, mask_h, mask_w, scaled,
                       sizes, nullptr, nullptr, nullptr);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int fi_unmold_encode(const int32_t *image_hw, const int32_t *image_hw_host, const int32_t *boxes,
                     const int32_t *num_valid, int batch, int num_dets, int mask_h, int mask_w, const void *workspace,
                     const long long *offsets, uint32_t *counts, uint8_t *strings, fi_stream_t stream)
{
    int rc = check_sizes(image_hw_host, batch, num_dets, 1, mask_h, mask_w);
    if (rc != FI_OK) return rc;
    if (batch == 0) return FI_OK;
    FI_REQUIRE(image_hw && boxes && num_valid && workspace && offsets && counts && strings, "null pointer");
    const size_t slots = (size_t)batch * num_dets;
    uint8_t *scaled = (uint8_t *)workspace + ((slots * sizeof(int32_t) + 255) & ~(size_t)255);
    hipLaunchKernelGGL(unmold_measure_kernel<true>, dim3(num_dets, batch), dim3(kThreads), 0, (hipStream_t)stream,
                       nullptr, image_hw, boxes, nullptr, num_valid, nullptr, num_dets, 1, mask_h, mask_w, scaled,
                       nullptr, offsets, counts, strings);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int fi_unmold_paste(const int32_t *image_hw, const int32_t *image_hw_host, const int32_t *boxes,
                    const int32_t *num_valid, int batch, int num_dets, int mask_h, int mask_w, const void *workspace,
                    long long total_bytes, uint8_t *masks, fi_stream_t stream)
{
    int rc = check_sizes(image_hw_host, batch, num_dets, 1, mask_h, mask_w);
    if (rc != FI_OK) return rc;
    FI_REQUIRE(total_bytes >= 0 && total_bytes <= (long long)batch * num_dets * kMaxImage * kMaxImage,
               "0 <= total_bytes <= batch * num_dets * 4096^2");
    if (total_bytes == 0) return FI_OK;
    FI_REQUIRE(image_hw && boxes && num_valid && workspace && masks, "null pointer");
    FI_REQUIRE(((uintptr_t)masks & 15) == 0, "masks 16-byte aligned");
    const size_t slots = (size_t)batch * num_dets;
    const uint8_t *scaled = (const uint8_t *)workspace + ((slots * sizeof(int32_t) + 255) & ~(size_t)255);
    const long long threads = (total_bytes + kPasteBytes - 1) / kPasteBytes;
    const long long blocks = (threads + kThreads - 1) / kThreads;
    FI_REQUIRE(blocks < (1LL << 31), "grid too large");
    hipLaunchKernelGGL(unmold_paste_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, image_hw,
                       boxes, num_valid, batch, num_dets, mask_h, mask_w, scaled, total_bytes, masks);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

}  // extern "C"
