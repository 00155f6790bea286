"""Training on 16-bit channels-last pyramid maps up to the RoI crops (TRAIN.ACT_SCOPE = 'crops' next to a 16-bit
TRAIN.ACT_PRECISION): the three launches of libfi_crops16.so (include/fi_crops16.h, csrc/crops16.hip) as thin wrappers, the
differentiable patch gather of the RPN's row form (`patch_rows16`) and the differentiable pair of RoIAlign crops of the
Dev stage (`pyramid_crops16`).

The forwards of the crops are roi16's launches (bit-equal crops); their backward is the fp32 channels-last RoIAlign
backward of libfi_hip.so into ONE set of buffers, and one gate-pack launch per level that masks with the make-up layer's
output, rounds once and sums -- the make-up layer's backward finds its masked gradient and column sums in its Gate16 and
runs no relu_grad16.  The patch rows' backward adds into the 16-bit tensor the make-up layer's data gradient left in a
conv.GradBox, in place, and returns it as the level map's only gradient.

Plain allocations, single process, as train16 and fpn16.  Which calls the kernels take is decided by fi_crops16_eligible
alone; a call it refuses is an error -- there is no fallback to another path.
"""
import ctypes

import torch

from . import _lib
from . import act16
from . import conv as _conv
from . import fpn16
from . import roi16
from . import train16

LIB_PATH = _lib.sublibrary_path("crops16")
_cp, _ci = ctypes.c_void_p, ctypes.c_int
_PATCH_FWD = (_ci, [_cp, _cp, _cp, _cp, _ci, _ci, _cp, _cp, _ci, _ci, _ci, _cp, _cp])
_PATCH_BWD = (_ci, [_cp, _cp, _cp, _cp, _cp, _ci, _ci, _cp, _cp, _ci, _ci, _ci, _cp])
_GATE_PACK = (_ci, [_cp, _cp, _cp, _cp, _ci, _ci, _ci, _ci, _cp])
# name -> (restype, argtypes); mirrors include/fi_crops16.h one to one
SIGNATURES = {
    "fi_crops16_eligible": (_ci, [_ci, _ci, _ci, _ci, _cp, _cp, _cp, _cp, _cp]),
    "fi_crops16_patch_rows_forward_bf16": _PATCH_FWD,
    "fi_crops16_patch_rows_forward_f16": _PATCH_FWD,
    "fi_crops16_patch_rows_backward_bf16": _PATCH_BWD,
    "fi_crops16_patch_rows_backward_f16": _PATCH_BWD,
    "fi_crops16_gate_pack_bf16": _GATE_PACK,
    "fi_crops16_gate_pack_f16": _GATE_PACK,
}
PATCH_FWD, PATCH_BWD, GATE_PACK = 0, 1, 2          # FI_CROPS16_* kinds of fi_crops16_eligible
SCOPE = "crops"
_STATS = {"patch_fwd": 0, "patch_bwd": 0, "gate_pack": 0, "crops": 0}


def load():
    """Load libfi_crops16.so (after libfi_hip.so, which it links against) and attach the signatures."""
    return _lib.load_sublibrary("crops16", SIGNATURES)


def stats():
    """Host counters since reset_stats(): 'patch_fwd' / 'patch_bwd' launches of the two patch-row kernels, 'gate_pack'
    launches of fi_crops16_gate_pack, 'crops' calls of pyramid_crops16 (roi16.stats() counts their RoIAlign launches)."""
    return dict(_STATS)


def reset_stats():
    _lib.zero_counters(_STATS)


def check_config(config):
    """What a model is built with under TRAIN.ACT_SCOPE = 'crops': NotImplementedError, naming the setting, for every
    configuration the 16-bit route to the crops cannot carry.  Any other scope: nothing to check."""
    if fpn16.train_scope(config) != SCOPE:
        return
    why = unsupported(config)
    if why is not None:
        raise NotImplementedError("TRAIN.ACT_SCOPE = 'crops' needs " + why)


def unsupported(config):
    """What the 16-bit route to the crops cannot carry in `config`, as the text behind "TRAIN.ACT_SCOPE = ... needs ", or
    None: the one list of check_config, which heads16.check_config shares."""
    dev, why = config.DEV, None
    if not dev.SWITCH:
        why = "DEV.SWITCH = True (got False): without the Dev stage there is no make-up layer in front of the crops"
    elif dev.UPSAMPLE_FAC != 1.:
        why = "DEV.UPSAMPLE_FAC = 1 (got %r): the transposed make-up layer has no 16-bit kernel" % (dev.UPSAMPLE_FAC,)
    elif config.ROIS.METHOD != 'roi_align':
        why = "ROIS.METHOD = 'roi_align' (got %r): RoIPool has no kernel on 16-bit channels-last maps" % (config.ROIS.METHOD,)
    elif not dev.BIG_FEAT_DETACH or dev.BIG_SUPERVISE:
        why = "DEV.BIG_FEAT_DETACH = True and DEV.BIG_SUPERVISE = False (got %r, %r): the big-box crop of the raw 16-bit " \
              "maps has no gradient route" % (dev.BIG_FEAT_DETACH, dev.BIG_SUPERVISE)
    elif config.RPN.ANCHOR_STRIDE != 1:
        why = "RPN.ANCHOR_STRIDE = 1 (got %r): the stride-2 shared convolution has no 16-bit kernel and no row form" \
              % (config.RPN.ANCHOR_STRIDE,)
    elif getattr(config.TRAIN, "FPN_OT_LOSS", False):
        why = "TRAIN.FPN_OT_LOSS = False: the optimal-transport branch of the pyramid reads fp32 maps"
    return why


def require_gates(scope=SCOPE):
    """The refusal at the call: with conv.GATES off the dense RPN builds a graph, and that has no 16-bit form."""
    if not _conv.GATES:
        raise _lib.FiError("TRAIN.ACT_SCOPE = %r needs conv.GATES on" % (scope,) + ": the dense RPN with a graph and the gradient "
                           "hand-offs through autograd have no 16-bit form; there is no fallback")


def _levels(what, maps16, steps):
    """(prec, N, C, ptrs, heights, widths, steps) of the level tensors; they share dtype, device, batch and channels."""
    maps16 = list(maps16)
    if not maps16:
        raise _lib.FiError("%s: no maps" % what)
    steps = [1] * len(maps16) if steps is None else [int(s) for s in steps]
    if len(steps) != len(maps16) or min(steps) < 1:
        raise _lib.FiError("%s: one step >= 1 per level, got %r for %d levels" % (what, steps, len(maps16)))
    first = maps16[0]
    prec = act16._require_act16(first, what)
    for m in maps16[1:]:
        act16._require_act16(m, what)
        if m.dtype != first.dtype or m.device != first.device or m.shape[:2] != first.shape[:2]:
            raise _lib.FiError("%s: the maps must share dtype, device, batch and channel count; got %s %s on %s next to "
                               "%s %s on %s" % (what, m.dtype, tuple(m.shape), m.device, first.dtype, tuple(first.shape),
                                                first.device))
    n = len(maps16)
    return (prec, first.shape[0], first.shape[1], (ctypes.c_void_p * n)(*[m.data_ptr() for m in maps16]),
            (ctypes.c_int * n)(*[m.shape[2] for m in maps16]), (ctypes.c_int * n)(*[m.shape[3] for m in maps16]),
            (ctypes.c_int * n)(*steps))


def _rows(what, image, anchor):
    _lib.require_cuda(image, anchor)
    if image.dim() != 1 or anchor.shape != image.shape:
        raise _lib.FiError("%s: image [rows] and anchor [rows], got %s and %s" % (what, tuple(image.shape),
                                                                                 tuple(anchor.shape)))
    return image.detach().to(torch.int64).contiguous(), anchor.detach().to(torch.int64).contiguous()


def _require(L, what, kind, levels, C, n, ptrs, *p):
    if L.fi_crops16_eligible(kind, levels, C, n, ptrs, *[_lib.ptr(t) for t in p]) != 1:
        raise _lib.FiError("%s: fi_crops16_eligible refuses this call (%d levels, C %d, n %d); there is no fallback"
                           % (what, levels, C, n))


def _patch_rows_launch(maps16, image, anchor, per_loc, steps):
    prec, N, C, ptrs, hs, ws, st = _levels("patch_rows16", maps16, steps)
    image, anchor = _rows("patch_rows16", image, anchor)
    L = load()
    R = image.numel()
    out = torch.empty((R, 9 * C), device=image.device, dtype=torch.float32)
    if R > 0 and N > 0:
        _require(L, "patch_rows16", PATCH_FWD, len(ptrs), C, R, ptrs, out, None, None, None)
        act16._launch(image.device, "fi_crops16_patch_rows_forward", _conv._lowp_fn(L, "crops16_patch_rows_forward", prec),
                      ptrs, hs, ws, st, len(ptrs), int(per_loc), _lib.ptr(image), _lib.ptr(anchor), R, N, C, _lib.ptr(out))
    else:
        out.zero_()
    _STATS["patch_fwd"] += 1
    return out


def patch_rows_grad16(d, grads16, image, anchor, per_loc, steps=None):
    """Adds the patch gradients d [rows, 9 C] (fp32) into the 16-bit channels-last level gradients `grads16` IN PLACE:
    every pixel a (row, tap) reaches becomes round16(old + the fp32 sum of its d in ascending (row, tap) order), one store
    per element, no atomics; every other element is left alone.  Levels that share a tensor (the same tensor twice, the
    second with a step) are summed into it.  One launch.  Raises _lib.FiError for what fi_crops16_eligible refuses."""
    prec, N, C, ptrs, hs, ws, st = _levels("patch_rows_grad16", grads16, steps)
    image, anchor = _rows("patch_rows_grad16", image, anchor)
    _lib.require_cuda(d)
    R = image.numel()
    if d.dtype != torch.float32 or d.dim() != 2 or tuple(d.shape) != (R, 9 * C) or not d.is_contiguous():
        raise _lib.FiError("patch_rows_grad16: d must be a contiguous float32 [%d, %d] tensor, got %s %s"
                           % (R, 9 * C, d.dtype, tuple(d.shape)))
    L = load()
    if R > 0 and N > 0:
        _require(L, "patch_rows_grad16", PATCH_BWD, len(ptrs), C, R, ptrs, d, None, None, None)
        act16._launch(d.device, "fi_crops16_patch_rows_backward", _conv._lowp_fn(L, "crops16_patch_rows_backward", prec),
                      _lib.ptr(d), ptrs, hs, ws, st, len(ptrs), int(per_loc), _lib.ptr(image), _lib.ptr(anchor), R, N, C)
    _STATS["patch_bwd"] += 1
    return grads16


def gate_pack16(d, y=None, dtype=None, colsum=True):
    """(g, s): g = round16(d) where y > 0, else 0 -- d an fp32 [N, C, H, W] tensor in channels-last memory, y the 16-bit
    channels-last output of the layer whose ReLU masks (None: no mask, `dtype` names the type) -- and, when `colsum`,
    s [C] fp32 = the per-channel sums of g (else None).  One launch, one pass over d.  Raises _lib.FiError for what
    fi_crops16_eligible refuses; there is no fallback."""
    _lib.require_cuda(d)
    if d.dim() != 4 or d.dtype != torch.float32 or not d.is_contiguous(memory_format=torch.channels_last):
        raise _lib.FiError("gate_pack16: d must be a 4-d channels-last float32 tensor, got %s %s with strides %s"
                           % (d.dtype, tuple(d.shape), tuple(d.stride())))
    if y is not None:
        act16._require_act16(y, "gate_pack16 (y)")
        if y.shape != d.shape or (dtype is not None and dtype != y.dtype):
            raise _lib.FiError("gate_pack16: y %s %s does not match d %s (dtype %s)" % (y.dtype, tuple(y.shape),
                                                                                       tuple(d.shape), dtype))
        dtype = y.dtype
    if dtype not in act16._PRECISION_OF:
        raise _lib.FiError("gate_pack16: dtype must be torch.bfloat16 or torch.float16, got %s" % (dtype,))
    L = load()
    N, C, H, W = d.shape
    g = torch.empty((N, C, H, W), device=d.device, dtype=dtype, memory_format=torch.channels_last)
    s = torch.empty(C, device=d.device, dtype=torch.float32) if colsum else None
    if N > 0:
        if H < 1 or W < 1:
            raise _lib.FiError("gate_pack16: an empty map %s" % (tuple(d.shape),))
        _require(L, "gate_pack16", GATE_PACK, 0, C, N * H * W, None, d, y, g, s)
    act16._launch(d.device, "fi_crops16_gate_pack", _conv._lowp_fn(L, "crops16_gate_pack", act16._PRECISION_OF[dtype]),
                  _lib.ptr(d), _lib.ptr(y), _lib.ptr(g), _lib.ptr(s), N, max(H, 1), max(W, 1), C)
    _STATS["gate_pack"] += 1
    return g, s


class _PatchRows16Fn(torch.autograd.Function):
    """sub_module._PatchRowsFn on 16-bit maps.  `tensors` are the DISTINCT level tensors, index[l] the tensor of level l.
    Backward: per tensor, what boxes[l] of its first level holds (the make-up layer's data gradient, a 16-bit channels-last
    tensor) or zeros; ONE fi_crops16_patch_rows_backward launch adds the rows' contributions in place; the tensors go to
    autograd as the maps' only gradients."""

    @staticmethod
    def forward(ctx, image, anchor, per_loc, boxes, steps, index, *tensors):
        maps = [tensors[i] for i in index]
        out = _patch_rows_launch(maps, image, anchor, per_loc, steps)
        ctx.save_for_backward(image, anchor)
        ctx.per_loc, ctx.boxes, ctx.steps, ctx.index = int(per_loc), boxes, steps, index
        ctx.like = [(tuple(t.shape), t.dtype, t.device) for t in tensors]
        return out

    @staticmethod
    def backward(ctx, d):
        image, anchor = ctx.saved_tensors
        d = d.contiguous().float()
        grads = []
        for i, (shape, dtype, dev) in enumerate(ctx.like):
            l = ctx.index.index(i)
            base = None
            if ctx.boxes is not None and ctx.boxes[l] is not None:
                base, ctx.boxes[l].value = ctx.boxes[l].value, None
            if base is None:
                base = torch.empty(shape, device=dev, dtype=dtype, memory_format=torch.channels_last).zero_()
            elif not (torch.is_tensor(base) and tuple(base.shape) == shape and base.dtype == dtype and
                      base.is_contiguous(memory_format=torch.channels_last)):
                raise _lib.FiError("patch_rows16: the gradient left for level %d is not a %s channels-last tensor of shape "
                                   "%s (TRAIN.ACT_SCOPE = 'crops' adds in place; there is no fallback)" % (l, dtype, shape))
            grads.append(base)
        patch_rows_grad16(d, [grads[i] for i in ctx.index], image, anchor, ctx.per_loc, ctx.steps)
        return (None,) * 6 + tuple(grads)


def patch_rows16(maps16, image, anchor, per_loc, grad_boxes=None, steps=None):
    """rows [R, 9 C] fp32: the 3 x 3 x C patch (tap-major) around the pixel of anchor (image[r], anchor[r]) of the
    level-major anchor list on its 16-bit channels-last level map -- the widened values, zeros outside the map and for
    padding rows (image[r] < 0).  One launch.
    steps: per level, the stride at which the level subsamples its tensor (None: 1).  A pyramid whose last map is the
    stride-2 subsample of the one before it passes that tensor twice, the second time with step 2.
    With grad mode on and a map that requires grad the call is differentiable: grad_boxes[l] (a conv.GradBox or None) is
    where another reader of level l's tensor left ITS 16-bit gradient; backward adds the rows' contributions into it in
    place (into zeros when it is empty) and returns it as the tensor's gradient.
    Raises _lib.FiError for what fi_crops16_eligible refuses; there is no fallback."""
    maps16 = list(maps16)
    if not (torch.is_grad_enabled() and any(m.requires_grad for m in maps16)):
        return _patch_rows_launch(maps16, image, anchor, per_loc, steps)
    _levels("patch_rows16", maps16, steps)                 # the argument checks, before the graph node is made
    tensors, index = [], []
    for m in maps16:
        hit = [i for i, t in enumerate(tensors) if t is m]
        if not hit:
            tensors.append(m)
        index.append(hit[0] if hit else len(tensors) - 1)
    steps = None if steps is None else [int(s) for s in steps]
    L = load()
    C = maps16[0].shape[1]
    if image.numel() > 0 and maps16[0].shape[0] > 0:
        _require(L, "patch_rows16 (backward)", PATCH_BWD, len(maps16), C, image.numel(), None, None, None, None, None)
    return _PatchRows16Fn.apply(image, anchor, int(per_loc), grad_boxes, steps, index, *tensors)


class _PyramidCrops16Fn(torch.autograd.Function):
    """Every crop of `specs` from the same 16-bit maps, forward: one roi16.pyramid_crop16 launch each.  Backward, with
    every crop's gradient in ONE call: fi_pyramid_crop_backward_nhwc for the first that has one, ..._accumulate for the
    others, into one set of fp32 channels-last buffers; per level one gate-pack launch -- masked with the map where the map's
    Gate16 was claimed, and the column sums left there -- whose 16-bit result is the map's gradient."""

    @staticmethod
    def forward(ctx, specs, gates, *maps):
        crops, saved = [], []
        for boxes, box_ind, level, size in specs:
            crops.append(roi16.pyramid_crop16(maps, boxes, box_ind, level, size, size))
            saved.append((boxes.detach().contiguous().float(), box_ind.detach().contiguous().to(torch.int32),
                          level.detach().contiguous().to(torch.int32), int(size)))
        ctx.specs, ctx.gates = saved, gates
        ctx.save_for_backward(*maps)
        ctx.set_materialize_grads(False)
        return tuple(crops)

    @staticmethod
    def backward(ctx, *ds):
        maps = ctx.saved_tensors
        nl = len(maps)
        if all(d is None for d in ds):
            return (None,) * (2 + nl)
        L = _lib.load()
        B, C = maps[0].shape[:2]
        dev = maps[0].device
        bufs = [torch.empty(tuple(m.shape), device=dev, dtype=torch.float32, memory_format=torch.channels_last) for m in maps]
        ptrs = (ctypes.c_void_p * nl)(*[t.data_ptr() for t in bufs])
        hs = (ctypes.c_int * nl)(*[m.shape[2] for m in maps])
        ws = (ctypes.c_int * nl)(*[m.shape[3] for m in maps])
        first = True
        for (boxes, box_ind, level, size), d in zip(ctx.specs, ds):
            if d is None:
                continue
            d = d.contiguous().float()
            fn, what = (L.fi_pyramid_crop_backward_nhwc, "fi_pyramid_crop_backward_nhwc") if first else \
                (L.fi_pyramid_crop_backward_nhwc_accumulate, "fi_pyramid_crop_backward_nhwc_accumulate")
            act16._launch(dev, what, fn, _lib.ptr(d), ptrs, hs, ws, nl, _lib.ptr(boxes), _lib.ptr(box_ind), _lib.ptr(level),
                          boxes.shape[0], B, C, size, size)
            if _lib.TAP is not None:
                _lib.TAP("pyramid_crop_backward", grads=d, boxes=boxes, box_ind=box_ind, level=level, crop=size,
                         accumulate=not first, level_grads=bufs)
            first = False
        out = []
        for buf, u, gate in zip(bufs, maps, ctx.gates):
            g, s = gate_pack16(buf, u if gate is not None else None, dtype=u.dtype, colsum=gate is not None)
            if gate is not None:
                gate.leave(g, s)
            out.append(g)
        return (None, None) + tuple(out)


def pyramid_crops16(maps16, specs):
    """[crops_0, crops_1, ...]: for every (boxes, box_ind, level, size) of `specs` the size x size RoIAlign of its boxes
    from the 16-bit channels-last maps16 -- roi16.pyramid_crop16's fp32 NCHW crops, bit for bit -- as ONE autograd node:
    its backward receives every crop's gradient in one call (see _PyramidCrops16Fn) and returns 16-bit map gradients.
    The caller promises that these crops are the maps' ONLY readers: a map that carries a train16.Gate16 (the output of
    train16.conv_bn_act16 with a ReLU) is claimed with conv.GATES on; its gradient is then masked here and its producer
    runs a premasked backward.  A map without a gate gets the plain rounded gradient.
    Raises _lib.FiError for what the eligibility queries refuse; there is no fallback."""
    maps16, specs = list(maps16), [tuple(s) for s in specs]
    if not maps16 or not specs:
        raise _lib.FiError("pyramid_crops16: no maps or no crops")
    for m in maps16:
        act16._require_act16(m, "pyramid_crops16")
    L = load()
    for m in maps16:
        N, C, H, W = m.shape
        if N > 0:
            _require(L, "pyramid_crops16 (gate-pack)", GATE_PACK, 0, C, N * H * W, None, None, m, None, None)
    gates = [train16._claim_gate16(m, True) for m in maps16]
    crops = _PyramidCrops16Fn.apply(specs, gates, *maps16)
    _STATS["crops"] += 1
    return list(crops)
