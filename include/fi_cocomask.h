/*
 * fi_cocomask.h -- C ABI of libfi_cocomask.so, the MI355X (gfx950) kernels that turn COCO polygon ground truth into
 * RLEs: the `annToRLE` step in front of the COCO evaluation (include/fi_cocoeval.h).  A library of its own next to
 * libfi_hip.so (include/fi_capi.h), which it links against and whose conventions it follows: device pointers, a
 * hipStream_t as void*, caller-allocated outputs and workspaces, no host synchronisation, FI_OK or a negative
 * FI_ERR_* status with the message in libfi_hip's fi_last_error().
 *
 * An RLE is a row (first count, number of counts, h, w) of int64 into a flat uint32 count array: the form that
 * fi_coco_rle_stats / fi_coco_iou read, so the outputs go to them unchanged.  Masks are column-major, h * w < 2^31.
 *
 * Up to FI_COCOMASK_LDS_KEYS keys (one polygon's boundary keys, or one merge group's input counts) are sorted in
 * LDS; anything larger is sorted in the global workspace by the same workgroup.  There is no limit on the size of a
 * polygon or of a group.
 */
#ifndef FI_COCOMASK_H_
#define FI_COCOMASK_H_

#include "fi_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FI_COCOMASK_LDS_KEYS 4096

/* ------------------------------------------------------------------------
 * Upper bound on the boundary keys of each polygon.  HOST function: host pointers, no GPU work.
 * Replaces: the allocation `x=malloc(sizeof(int)*k)` of rleFrPoly  datasets/eval/common/maskApi.c:182-190 (the
 *           reference sizes its key array by the number of upsampled points, 5 x the perimeter in pixels).
 * xy: flat (x, y) doubles of all polygons; poly_off [num_polys + 1]: the first VERTEX of each polygon (polygon p has
 * poly_off[p + 1] - poly_off[p] >= 1 vertices).  bound [num_polys].  Coordinates must be finite and at most 1e8 in
 * magnitude (5 * c has to fit an int).
 *
 * bound = sum over the edges (closing edge included) of ceil(|X1 - X0| / 5), X = (int)(5 * x + .5).  Proof: a key
 * is emitted only between two consecutive upsampled points whose u differs, with xd = (U + .5) / 5 - .5 an integer
 * >= 0, U the smaller of the two u.  Two consecutive points of different edges are the same vertex: their u can
 * differ only where an x-major edge (u = X exactly) meets a y-major one (u = (int)(X + s * t + .5), truncated towards
 * zero, which is X + 1 for X < 0), so only with U < 0, and xd < 0 emits nothing.  Inside one edge u is monotone in
 * the step and moves by at most 1 per step, so every U occurs at most once; those with U >= 0 are distinct integers
 * of [min(X0, X1), max(X0, X1) - 1], and xd is an integer only for U = 2 (mod 5): at most ceil(|X1 - X0| / 5) of
 * |X1 - X0| consecutive integers.  The bound is attained (a rectangle from x = 0.4 to x = 0.6: 2 keys).
 * The RLE of a polygon has at most bound + 1 counts.
 * ---------------------------------------------------------------------- */
int fi_cocomask_poly_bound(const double *xy, const long long *poly_off, long long num_polys, long long *bound);

/* ------------------------------------------------------------------------
 * One RLE per polygon.
 * Replaces: rleFrPoly  datasets/eval/common/maskApi.c:161-201 (through frPyObjects / frPoly, pycocotools/_mask.pyx
 *           :260-308).  Bit-exact (tests/golden/cocopoly.npz): the same double arithmetic, one rounded operation at
 *           a time, and (int) truncation towards zero.
 * xy, poly_off as above but on the device; sizes [num_polys, 2] int64 (h, w), both >= 1; key_off [num_polys + 1]
 * int64: the exclusive scan of fi_cocomask_poly_bound's output, total_keys = key_off[num_polys] (the host's copy).
 * Outputs: rles [num_polys, 4]; polygon p's counts start at counts[key_off[p] + p] (capacity bound + 1; the row
 * carries the true length), so counts holds total_keys + num_polys uint32.  Nothing else is written.
 * workspace: fi_cocomask_workspace_bytes(total_keys, num_polys) bytes; polygon p's keys live at key_off[p] when its
 * bound exceeds FI_COCOMASK_LDS_KEYS.  A repeated vertex (zero-length edge, slope 0 / 0 in the C) emits nothing.
 * ---------------------------------------------------------------------- */
size_t fi_cocomask_workspace_bytes(long long total_keys, long long num_items);
int fi_cocomask_from_polygons(const double *xy, const long long *poly_off, const long long *sizes,
                              const long long *key_off, long long num_polys, long long total_keys, long long *rles,
                              uint32_t *counts, void *workspace, fi_stream_t stream);

/* ------------------------------------------------------------------------
 * Union or intersection of groups of RLEs.
 * Replaces: rleMerge  datasets/eval/common/maskApi.c:49-70 (maskUtils.merge in COCO.annToRLE, pycocotools/coco.py
 *           :405-424).
 * rles [., 4] / counts: the input RLEs; group g is the rows group_off[g] .. group_off[g + 1] - 1.  out_off
 * [num_groups + 1] int64: the exclusive scan of each group's summed number of counts (or of an upper bound of it,
 * such as the capacities bound + 1 of fi_cocomask_from_polygons), total_counts = out_off[num_groups] (the host's
 * copy).  Group g's result is written at out_counts[out_off[g]] and is never longer than its inputs together;
 * out_rles [num_groups, 4].  A group of one is a copy, an empty group gives (., 0, 0, 0),
 * a group whose members differ in (h, w) gives h = w = m = 0, as the C does.  The members of a larger group must be
 * canonical (counts sum to h * w, only the first may be 0: what rleFrPoly and rleEncode make); the result is then
 * the canonical RLE that the C's sequential pairwise merge gives, whatever the order.
 * workspace: fi_cocomask_workspace_bytes(total_counts, num_groups) bytes.
 * ---------------------------------------------------------------------- */
int fi_cocomask_merge(const long long *rles, const uint32_t *counts, const long long *group_off,
                      const long long *out_off, long long num_groups, long long total_counts, int intersect,
                      long long *out_rles, uint32_t *out_counts, void *workspace, fi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FI_COCOMASK_H_ */
