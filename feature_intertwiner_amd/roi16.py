"""RoIAlign that reads 16-bit channels-last pyramid maps and writes the fp32 NCHW crops the heads consume (libfi_roi16.so,
include/fi_roi16.h, csrc/crop_roi16.hip).  Inference only (MODEL.ACT_SCOPE = 'roi' next to a 16-bit MODEL.ACT_PRECISION).

Maps are act16's: [N, C, H, W]-shaped torch.channels_last bfloat16 / float16.  The crops are bit-identical to
fi_pyramid_crop_forward_nhwc on the widened maps.  Which calls the kernel takes is decided by fi_roi16_crop_eligible
alone; nothing here restates its rules, and a call it refuses is an error -- there is no fallback to another path.
"""
import ctypes

import torch

from . import _lib
from . import act16 as _act16
from . import conv as _conv
from . import pyr16 as _pyr16

LIB_PATH = _lib.sublibrary_path("roi16")
_cp, _ci, _cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
_pp, _ip = ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int)
_CROP = (_ci, [_pp, _ip, _ip, _ci, _cp, _cp, _cp, _ci, _ci, _ci, _ci, _ci, _cf, _cp, _cp])
# name -> (restype, argtypes); mirrors include/fi_roi16.h one to one
SIGNATURES = {
    "fi_roi16_crop_eligible": (_ci, [_ci, _ci, _ci, _ci, _pp, _cp]),
    "fi_roi16_pyramid_crop_forward_bf16": _CROP,
    "fi_roi16_pyramid_crop_forward_f16": _CROP,
}
_STATS = {"crop": 0}


def load():
    """Load libfi_roi16.so (after libfi_hip.so, which it links against) and attach the signatures."""
    return _lib.load_sublibrary("roi16", SIGNATURES)


def stats():
    """Host counters of the launches since reset_stats(): {'crop'}."""
    return dict(_STATS)


def reset_stats():
    _lib.zero_counters(_STATS)


def pyramid_crop16(maps16, boxes, box_ind, level, crop_h, crop_w, extrapolation_value=0.0):
    """crops[i] = crop_h x crop_w RoIAlign of box i from maps16[level[i] - 2] (image box_ind[i]): fp32
    [num_boxes, C, crop_h, crop_w], one launch for all levels.  Rows with a level outside the pyramid or a box_ind outside
    the batch are zeros; a row with level -1 is left unwritten.  `level` may be None for a single map."""
    maps16 = list(maps16)
    if not maps16:
        raise _lib.FiError("pyramid_crop16: no maps")
    prec = _act16._require_act16(maps16[0], "pyramid_crop16")
    _pyr16._require_inference("pyramid_crop16")
    first = maps16[0]
    for m in maps16[1:]:
        _act16._require_act16(m, "pyramid_crop16")
        if m.dtype != first.dtype or m.device != first.device or m.shape[:2] != first.shape[:2]:
            raise _lib.FiError("pyramid_crop16: the maps must share dtype, device, batch and channel count; got %s %s on %s "
                               "next to %s %s on %s" % (m.dtype, tuple(m.shape), m.device, first.dtype, tuple(first.shape),
                                                        first.device))
    _lib.require_cuda(boxes, box_ind, level)
    L = load()
    nl = len(maps16)
    B, C = first.shape[:2]
    boxes_c = boxes.detach().contiguous().float()
    ind_c = box_ind.detach().contiguous().to(torch.int32)
    lvl_c = None if level is None else level.detach().contiguous().to(torch.int32)
    N = boxes_c.shape[0]
    if boxes_c.dim() != 2 or boxes_c.shape[1] != 4 or ind_c.numel() != N or (lvl_c is not None and lvl_c.numel() != N):
        raise _lib.FiError("pyramid_crop16: boxes [n, 4] with box_ind [n] and level [n]; got %s, %s, %s"
                           % (tuple(boxes.shape), tuple(box_ind.shape), None if level is None else tuple(level.shape)))
    crop_h, crop_w = int(crop_h), int(crop_w)
    crops = torch.empty((N, C, max(crop_h, 0), max(crop_w, 0)), device=first.device, dtype=torch.float32)
    ptrs = (ctypes.c_void_p * nl)(*[m.data_ptr() for m in maps16])
    hs = (ctypes.c_int * nl)(*[m.shape[2] for m in maps16])
    ws = (ctypes.c_int * nl)(*[m.shape[3] for m in maps16])
    if N > 0 and L.fi_roi16_crop_eligible(nl, C, crop_h, crop_w, ptrs, _lib.ptr(crops)) != 1:
        raise _lib.FiError("pyramid_crop16: fi_roi16_crop_eligible refuses this call (%d maps, %d channels, crop %d x %d); "
                           "there is no fallback" % (nl, C, crop_h, crop_w))
    _act16._launch(first.device, "fi_roi16_pyramid_crop_forward", _conv._lowp_fn(L, "roi16_pyramid_crop_forward", prec),
                   ptrs, hs, ws, nl, _lib.ptr(boxes_c), _lib.ptr(ind_c), _lib.ptr(lvl_c), N, B, C, crop_h, crop_w,
                   float(extrapolation_value), _lib.ptr(crops))
    _STATS["crop"] += 1
    return crops
