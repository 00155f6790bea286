"""COCO ground-truth segmentations to RLE on the GPU: `COCO.annToRLE` (pycocotools/coco.py:405-424), the step of
`COCOeval._toMask` in front of the mask IoU.

Polygons are rasterised by `rleFrPoly` and the parts of one object are united by `rleMerge`; both are the kernels of
csrc/cocomask.hip (include/fi_cocomask.h).  This module flattens the Python lists, sizes the buffers from the
library's bound and assembles one (rles, counts) pair in the layout of cocoeval.py.  Every count is bit-equal to the
reference's (tests/golden/cocopoly.npz).  Decisions where the reference raises or misbehaves are in DESIGN.md §2."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import FiError, check, current_stream

LIB_PATH = _lib.sublibrary_path("cocomask")
_p, _i, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
# name -> (restype, argtypes); mirrors include/fi_cocomask.h one to one
SIGNATURES = {
    "fi_cocomask_poly_bound": (_i, [_p, _p, _ll, _p]),
    "fi_cocomask_workspace_bytes": (ctypes.c_size_t, [_ll, _ll]),
    "fi_cocomask_from_polygons": (_i, [_p, _p, _p, _p, _ll, _ll, _p, _p, _p, _p]),
    "fi_cocomask_merge": (_i, [_p, _p, _p, _p, _ll, _ll, _i, _p, _p, _p, _p]),
}


def load():
    """Load libfi_cocomask.so (after libfi_hip.so, which it links against) and attach the signatures."""
    return _lib.load_sublibrary("cocomask", SIGNATURES)


def _host_ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def flatten_polygons(polygons):
    """Flat (x, y) doubles and the first vertex of each polygon.  `int(len(p) / 2)` vertices, as frPoly
    (_mask.pyx:266): an odd-length list drops its last number.  Fewer than 6 numbers raise."""
    xy, off = [], [0]
    for p in polygons:
        a = np.asarray(p, np.float64).reshape(-1)
        if a.size < 6:
            raise FiError("a polygon needs at least 6 numbers (3 vertices); got %d" % a.size)
        a = a[:a.size // 2 * 2]
        xy.append(a)
        off.append(off[-1] + a.size // 2)
    flat = np.ascontiguousarray(np.concatenate(xy)) if xy else np.zeros(0, np.float64)
    return flat, np.asarray(off, np.int64)


def poly_bound(xy, poly_off):
    """fi_cocomask_poly_bound on host arrays: an upper bound on the boundary keys of each polygon."""
    L = load()
    n = len(poly_off) - 1
    bound = np.zeros(max(n, 1), np.int64)
    xy = np.ascontiguousarray(xy, np.float64)
    poly_off = np.ascontiguousarray(poly_off, np.int64)
    check(L.fi_cocomask_poly_bound(_host_ptr(xy), _host_ptr(poly_off), n, _host_ptr(bound)), "fi_cocomask_poly_bound")
    return bound[:n]


def _scan(v):
    return np.concatenate([[0], np.cumsum(v)]).astype(np.int64)


def _from_polygons(L, dev, polygons, sizes):
    from .cocoeval import _up, ptr
    xy, off = flatten_polygons(polygons)
    n = len(off) - 1
    sizes = np.asarray(sizes, np.int64).reshape(n, 2)
    if n and (sizes.min() < 1 or (sizes[:, 0] * sizes[:, 1]).max() >= 2 ** 31):
        raise FiError("from_polygons: every (h, w) needs h >= 1, w >= 1 and h * w < 2^31")
    bound = poly_bound(xy, off)
    key_off = _scan(bound)
    total = int(key_off[-1])
    i64 = torch.int64
    rles = torch.empty(n, 4, dtype=i64, device=dev)
    # zeros: the slack behind each RLE (capacity bound + 1) has defined bytes; one spare count: never an empty array
    counts = torch.zeros(total + n + 1, dtype=torch.int32, device=dev)
    ws = torch.empty(max(1, L.fi_cocomask_workspace_bytes(total, n) // 4), dtype=torch.int32, device=dev)
    xy_t, off_t = _up(xy, torch.float64, dev), _up(off, i64, dev)
    sz_t, ko_t = _up(sizes, i64, dev), _up(key_off, i64, dev)
    with torch.cuda.device(dev):
        check(L.fi_cocomask_from_polygons(ptr(xy_t), ptr(off_t), ptr(sz_t), ptr(ko_t), n, total, ptr(rles),
                                          ptr(counts), ptr(ws), current_stream()), "fi_cocomask_from_polygons")
    return rles, counts, bound + 1


def from_polygons(polygons, sizes, device=None):
    """`maskUtils.frPyObjects` on polygons (rleFrPoly): a list of flat [x0, y0, x1, y1, ..] lists and one (h, w) per
    polygon -> device (rles [n, 4] int64, counts uint32 as int32), one RLE per polygon."""
    from .cocoeval import _device
    L = load()
    rles, counts, _ = _from_polygons(L, _device(device), list(polygons), sizes)
    return rles, counts


def _merge(L, dev, rles, counts, group_off, out_off, intersect):
    from .cocoeval import _up, ptr
    g = len(group_off) - 1
    total = int(out_off[-1])
    out_rles = torch.empty(g, 4, dtype=torch.int64, device=dev)
    out_counts = torch.zeros(total + 1, dtype=torch.int32, device=dev)
    ws = torch.empty(max(1, L.fi_cocomask_workspace_bytes(total, g) // 4), dtype=torch.int32, device=dev)
    go_t, oo_t = _up(group_off, torch.int64, dev), _up(out_off, torch.int64, dev)
    with torch.cuda.device(dev):
        check(L.fi_cocomask_merge(ptr(rles), ptr(counts), ptr(go_t), ptr(oo_t), g, total, int(bool(intersect)),
                                  ptr(out_rles), ptr(out_counts), ptr(ws), current_stream()), "fi_cocomask_merge")
    return out_rles, out_counts


def merge(rles, counts, group_off, intersect=False):
    """`maskUtils.merge` (rleMerge) over groups: group g is the rows group_off[g] .. group_off[g + 1] - 1 of `rles`.
    Returns device (rles [num_groups, 4], counts).  Reads the input lengths back once to size the output."""
    L = load()
    group_off = np.asarray(group_off, np.int64).reshape(-1)
    n = rles.shape[0]
    if group_off.size < 1 or group_off[0] != 0 or group_off[-1] != n or (np.diff(group_off) < 0).any():
        raise FiError("merge: group_off must ascend from 0 to the number of RLEs")
    m = rles[:, 1].cpu().numpy()
    out_off = _scan(m)[group_off]
    return _merge(L, rles.device, rles.contiguous(), counts, group_off, out_off, intersect)


def ann_to_rle(annotations, image_sizes, device=None):
    """`COCO.annToRLE` for a list of annotations whose 'segmentation' is a polygon list (the parts of one object are
    united), an uncompressed RLE ('counts' a list) or a COCO RLE string.  `image_sizes` maps image id -> (height,
    width) and sizes the polygons; an RLE carries its own size.  Returns one device (rles [n, 4], counts) pair in
    annotation order."""
    from .cocoeval import _device, _segm_counts, _up
    L = load()
    dev = _device(device)
    anns = list(annotations)
    n = len(anns)
    polys, sizes, group, poly_idx, host, host_idx = [], [], [0], [], [], []
    for j, a in enumerate(anns):
        segm = a["segmentation"]
        if isinstance(segm, (list, tuple)):
            if len(segm) == 0:
                raise FiError("ann_to_rle: annotation %r has an empty polygon list" % (a.get("id"),))
            if image_sizes is None or a["image_id"] not in image_sizes:
                raise FiError("ann_to_rle: polygons need image_sizes[%r] = (height, width)" % (a["image_id"],))
            hw = tuple(int(v) for v in image_sizes[a["image_id"]])
            polys += list(segm)
            sizes += [hw] * len(segm)
            group.append(len(polys))
            poly_idx.append(j)
        else:
            host.append(_segm_counts(segm, "ann_to_rle"))
            host_idx.append(j)
    lens = np.array([c.size for c, _, _ in host], np.int64)
    desc = np.zeros((len(host), 4), np.int64)
    desc[:, 0] = np.cumsum(lens) - lens
    desc[:, 1] = lens
    desc[:, 2:] = np.array([(h, w) for _, h, w in host], np.int64).reshape(len(host), 2)
    flat = np.concatenate([c for c, _, _ in host] + [np.zeros(0, np.uint32)]).astype(np.uint32)
    n_host = int(flat.size)
    rles = torch.empty(n, 4, dtype=torch.int64, device=dev)
    parts = [_up(flat.view(np.int32), torch.int32, dev)]
    if host:
        rles[_up(np.asarray(host_idx, np.int64), torch.int64, dev)] = _up(desc, torch.int64, dev)
    if polys:
        part_rles, part_counts, cap = _from_polygons(L, dev, polys, sizes)
        group = np.asarray(group, np.int64)
        out_off = _scan(cap)[group]                       # capacities: an upper bound of the parts' lengths
        m_rles, m_counts = _merge(L, dev, part_rles, part_counts, group, out_off, False)
        m_rles[:, 0] += n_host
        rles[_up(np.asarray(poly_idx, np.int64), torch.int64, dev)] = m_rles
        parts.append(m_counts)
    else:
        parts.append(torch.zeros(1, dtype=torch.int32, device=dev))
    return rles, torch.cat(parts)
