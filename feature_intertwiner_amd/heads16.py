"""The backward launches of the box and mask heads on 16-bit channels-last crops: the two entry points of libfi_heads16.so
(include/fi_heads16.h, csrc/heads16.hip) as thin wrappers -- `crop_backward16`, RoIAlign's backward from a 16-bit
channels-last crop gradient into fp32 channels-last map gradients (the buffers crops16.gate_pack16 then packs), and
`class_rows_grad16`, the backward of the mask head's last 1x1 layer when the loss reads one class per RoI -- and the two
differentiable pieces built on them: `pyramid_crops_heads16`, the crops of both heads and of the feature extractor as one
autograd node that returns 16-bit map gradients; `class_rows_out16`, the class-selected output layer of the mask head, and
`deconv2x2_bias_act16`, the transposed convolution in front of it as a premasked 1x1 layer; `window_bn_act16` and
`stacked_out16`, the box head's full-window layer and stacked class + box output layer.  The heads' forwards are head16's
launches (bit-equal outputs); their other layers with a graph are train16.conv_bn_act16.

TRAIN.ACT_SCOPE = 'heads' (next to a 16-bit TRAIN.ACT_PRECISION) is everything 'crops' does plus this module: Dev.forward
builds the crop node, sub_module.Classifier and sub_module.Mask take its 16-bit crops through these layers, and only the
class logits, the boxes, the selected mask logits and the feature extractor's rows stay fp32.  `check_config` refuses what
the scope cannot carry when the model is built.  Plain allocations, single process, as train16, fpn16 and crops16.  Which calls the two
kernels take is decided by fi_heads16_eligible alone; a call it or the other libraries' queries refuse is an error -- there
is no fallback to another path.
"""
import ctypes

import torch

from . import _lib
from . import act16
from . import conv as _conv
from . import crops16
from . import fpn16
from . import grad16
from . import head16
from . import roi16
from . import train16

LIB_PATH = _lib.sublibrary_path("heads16")
_cp, _ci = ctypes.c_void_p, ctypes.c_int
_CROP_BWD = (_ci, [_cp, _cp, _cp, _cp, _ci, _cp, _cp, _cp, _ci, _ci, _ci, _ci, _ci, _ci, _cp])
_CLASS_ROWS = (_ci, [_cp, _cp, _cp, _cp, _cp, _cp, _cp, _cp, _ci, _ci, _ci, _ci, _ci, _cp])
# name -> (restype, argtypes); mirrors include/fi_heads16.h one to one
SIGNATURES = {
    "fi_heads16_eligible": (_ci, [_ci, _ci, _ci, _ci, _ci, _ci, _cp, _cp, _cp, _cp, _cp]),
    "fi_heads16_pyramid_crop_backward_bf16": _CROP_BWD,
    "fi_heads16_pyramid_crop_backward_f16": _CROP_BWD,
    "fi_heads16_class_rows_backward_bf16": _CLASS_ROWS,
    "fi_heads16_class_rows_backward_f16": _CLASS_ROWS,
}
CROP_BWD, CLASS_ROWS = 0, 1          # FI_HEADS16_* kinds of fi_heads16_eligible
_STATS = {"crop_bwd": 0, "class_rows": 0, "crops": 0}


def load():
    """Load libfi_heads16.so (after libfi_hip.so, which it links against) and attach the signatures."""
    return _lib.load_sublibrary("heads16", SIGNATURES)


def stats():
    """Host counters since reset_stats(): 'crop_bwd' launches of fi_heads16_pyramid_crop_backward, 'class_rows' launches of
    fi_heads16_class_rows_backward, 'crops' calls of pyramid_crops_heads16 (head16.stats() and roi16.stats() count its
    RoIAlign launches, crops16.stats() its gate-pack launches)."""
    return dict(_STATS)


def reset_stats():
    _lib.zero_counters(_STATS)


SCOPE = "heads"


def check_config(config):
    """What a model is built with under TRAIN.ACT_SCOPE = 'heads': NotImplementedError, naming the setting, for everything
    'crops' refuses (crops16.unsupported) and for DEV.CLS_MERGE_FEAT, whose merged feature has no route into the box head's
    16-bit rows.  Any other scope: nothing to check."""
    if fpn16.train_scope(config) != SCOPE:
        return
    why = crops16.unsupported(config)
    if why is None and config.DEV.CLS_MERGE_FEAT:
        why = "DEV.CLS_MERGE_FEAT = False (got True): the feature extractor's fp32 rows are not merged into the box head's " \
              "16-bit rows"
    if why is not None:
        raise NotImplementedError("TRAIN.ACT_SCOPE = 'heads' needs " + why)


def require_gates():
    """The refusal at the call: the heads' gradient hand-offs (Gate16) need conv.GATES on, as 'crops' does."""
    crops16.require_gates(SCOPE)


def crop_backward16(d16, level_bufs, boxes, box_ind, level, size, accumulate):
    """Adds RoIAlign's backward of the crop gradient d16 -- 16-bit, logical [n, C, size, size] in channels-last memory, what
    head16.pyramid_crop16_cl returns -- into level_bufs, the fp32 channels-last [B, C, H_l, W_l] gradient maps of the
    pyramid levels 2, 3, ...; box i belongs to level[i] (int) of image box_ind[i].  accumulate False zero-fills the maps
    first.  The adds are fp32 atomics: the last bits of the sums may differ between two runs.  Rows with a level outside
    the pyramid (-1 included) or a box_ind outside the batch add nothing.  One launch.  `size` may be an int or (h, w);
    `level` None with a single map.  Returns level_bufs.
    Raises _lib.FiError for what fi_heads16_eligible refuses; there is no fallback."""
    level_bufs = list(level_bufs)
    if not level_bufs:
        raise _lib.FiError("crop_backward16: no maps")
    _lib.require_cuda(d16, boxes, box_ind, level, *level_bufs)
    ch, cw = (int(size), int(size)) if not isinstance(size, (tuple, list)) else (int(size[0]), int(size[1]))
    first = level_bufs[0]
    for t in level_bufs:
        if t.dim() != 4 or t.dtype != torch.float32 or not t.is_contiguous(memory_format=torch.channels_last) or \
                t.shape[:2] != first.shape[:2] or t.device != first.device:
            raise _lib.FiError("crop_backward16: the maps must be float32 channels-last [B, C, H, W] tensors of one batch, "
                               "channel count and device; got %s %s with strides %s" % (t.dtype, tuple(t.shape),
                                                                                     tuple(t.stride())))
    B, C = first.shape[:2]
    if d16.dtype not in act16._PRECISION_OF or d16.dim() != 4 or tuple(d16.shape[1:]) != (C, ch, cw) or \
            not d16.permute(0, 2, 3, 1).is_contiguous():
        raise _lib.FiError("crop_backward16: d16 must be a bfloat16 / float16 [n, %d, %d, %d] tensor in channels-last memory, "
                           "got %s %s with strides %s" % (C, ch, cw, d16.dtype, tuple(d16.shape), tuple(d16.stride())))
    prec = act16._PRECISION_OF[d16.dtype]
    n = d16.shape[0]
    boxes_c = boxes.detach().contiguous().float()
    ind_c = box_ind.detach().contiguous().to(torch.int32)
    lvl_c = None if level is None else level.detach().contiguous().to(torch.int32)
    if boxes_c.dim() != 2 or tuple(boxes_c.shape) != (n, 4) or ind_c.numel() != n or (lvl_c is not None and lvl_c.numel() != n):
        raise _lib.FiError("crop_backward16: boxes [%d, 4] with box_ind [%d] and level [%d]; got %s, %s, %s"
                           % (n, n, n, tuple(boxes.shape), tuple(box_ind.shape), None if level is None else tuple(level.shape)))
    L = load()
    nl = len(level_bufs)
    ptrs = (ctypes.c_void_p * nl)(*[t.data_ptr() for t in level_bufs])
    hs = (ctypes.c_int * nl)(*[t.shape[2] for t in level_bufs])
    ws = (ctypes.c_int * nl)(*[t.shape[3] for t in level_bufs])
    if B > 0:
        if L.fi_heads16_eligible(CROP_BWD, nl, C, ch, cw, max(n, 1), ptrs, _lib.ptr(d16), None, None, None) != 1:
            raise _lib.FiError("crop_backward16: fi_heads16_eligible refuses this call (%d maps, %d channels, crop %d x %d, "
                               "%d boxes); there is no fallback" % (nl, C, ch, cw, n))
        act16._launch(first.device, "fi_heads16_pyramid_crop_backward", _conv._lowp_fn(L, "heads16_pyramid_crop_backward", prec),
                      _lib.ptr(d16), ptrs, hs, ws, nl, _lib.ptr(boxes_c), _lib.ptr(ind_c), _lib.ptr(lvl_c), n, B, C, ch, cw,
                      1 if accumulate else 0)
        _STATS["crop_bwd"] += 1
    return level_bufs


def class_rows_grad16(d, u16, w16, cls, dweight=None, dbias=None, colsum=True):
    """(du, s): the backward of logits[i, a, b] = bias[cls[i]] + <u16[i, (a, b, :)], w16[cls[i]]> per pixel.
    d: fp32 [n, 2, 2, H, W], the gradient of the selected logits; u16: the 16-bit channels-last [n, 4 C, H, W] ReLU output
    of the transposed convolution run as a 1x1 layer (head16.deconv2x2_act16: channels ordered (a, b, c)); w16: the 16-bit
    [K, C] weight the forward read; cls: int64 [n] in [0, K).
    du = u16 > 0 ? round16(d * w16[cls]) : 0, like u16; s [4 C] fp32 = the per-channel sums of du as stored (None without
    `colsum`); dweight [K, C] / dbias [K] (fp32, optional) are ACCUMULATED into: the sums of d * u16 and of d over the rows
    of each RoI, added to the row of its class.  du is bit-reproducible; the sums are fp32 atomics of per-RoI partial sums.
    One launch.  Raises _lib.FiError for what fi_heads16_eligible refuses; there is no fallback."""
    prec = act16._require_act16(u16, "class_rows_grad16 (u16)")
    _lib.require_cuda(d, w16, cls, dweight, dbias)
    n, C4, H, W = u16.shape
    if C4 % 4 != 0:
        raise _lib.FiError("class_rows_grad16: u16 holds (a, b, c)-ordered channels; %d is no multiple of 4" % C4)
    C = C4 // 4
    if d.dtype != torch.float32 or tuple(d.shape) != (n, 2, 2, H, W) or not d.is_contiguous():
        raise _lib.FiError("class_rows_grad16: d must be a contiguous float32 [%d, 2, 2, %d, %d] tensor, got %s %s"
                           % (n, H, W, d.dtype, tuple(d.shape)))
    if w16.dtype != u16.dtype or w16.dim() != 2 or w16.shape[1] != C or not w16.is_contiguous() or w16.shape[0] < 1:
        raise _lib.FiError("class_rows_grad16: w16 must be a contiguous %s [K, %d] matrix, got %s %s"
                           % (u16.dtype, C, w16.dtype, tuple(w16.shape)))
    K = w16.shape[0]
    if cls.dtype != torch.int64 or tuple(cls.shape) != (n,) or not cls.is_contiguous():
        raise _lib.FiError("class_rows_grad16: cls must be a contiguous int64 [%d] tensor, got %s %s"
                           % (n, cls.dtype, tuple(cls.shape)))
    for t, shape, name in ((dweight, (K, C), "dweight"), (dbias, (K,), "dbias")):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous()):
            raise _lib.FiError("class_rows_grad16: %s must be a contiguous float32 %s tensor, got %s %s"
                               % (name, shape, t.dtype, tuple(t.shape)))
    L = load()
    du = torch.empty_like(u16, memory_format=torch.channels_last)
    s = torch.empty(C4, device=u16.device, dtype=torch.float32) if colsum else None
    if H < 1 or W < 1:
        raise _lib.FiError("class_rows_grad16: an empty map %s" % (tuple(u16.shape),))
    f32 = (ctypes.c_void_p * 3)(*[None if t is None else t.data_ptr() for t in (s, dweight, dbias)])
    if L.fi_heads16_eligible(CLASS_ROWS, K, C, H, W, max(n, 1), f32, _lib.ptr(u16), _lib.ptr(w16), _lib.ptr(du),
                             _lib.ptr(d)) != 1:
        raise _lib.FiError("class_rows_grad16: fi_heads16_eligible refuses this call (n %d, H %d, W %d, C %d, K %d); there "
                           "is no fallback" % (n, H, W, C, K))
    act16._launch(u16.device, "fi_heads16_class_rows_backward", _conv._lowp_fn(L, "heads16_class_rows_backward", prec),
                  _lib.ptr(d), _lib.ptr(u16), _lib.ptr(w16), _lib.ptr(cls), _lib.ptr(du), _lib.ptr(s), _lib.ptr(dweight),
                  _lib.ptr(dbias), n, H, W, C, K)
    _STATS["class_rows"] += 1
    return du, s


def _spec(spec):
    boxes, box_ind, level, size = spec
    return (boxes.detach().contiguous().float(), box_ind.detach().contiguous().to(torch.int32),
            level.detach().contiguous().to(torch.int32), int(size))


class _PyramidCropsHeads16Fn(torch.autograd.Function):
    """The crops of both heads and of the feature extractor from the same 16-bit maps.  Forward: one
    head16.pyramid_crop16_cl launch for each 16-bit crop, one roi16.pyramid_crop16 launch for the fp32 rows.  Backward,
    with every reader's gradient in ONE call: RoIAlign's backward is linear in the boxes, so each reader's gradient goes
    through its own launch over its own boxes -- crop_backward16 for the 16-bit ones, fi_pyramid_crop_backward_nhwc for
    the fp32 rows; the first launch zero-fills, the others accumulate -- into one set of fp32 channels-last buffers; then
    per level one gate-pack launch exactly as crops16._PyramidCrops16Fn."""

    @staticmethod
    def forward(ctx, box_spec, mask_spec, rest_spec, feat_spec, gates, *maps):
        pooled = head16.pyramid_crop16_cl(maps, box_spec[0], box_spec[1], box_spec[2], box_spec[3], box_spec[3])
        front = head16.pyramid_crop16_cl(maps, mask_spec[0], mask_spec[1], mask_spec[2], mask_spec[3], mask_spec[3])
        rest = None
        if rest_spec is not None:
            rest = head16.pyramid_crop16_cl(maps, rest_spec[0], rest_spec[1], rest_spec[2], rest_spec[3], rest_spec[3])
            ctx.mark_non_differentiable(rest)
        feat = roi16.pyramid_crop16(maps, feat_spec[0], feat_spec[1], feat_spec[2], feat_spec[3], feat_spec[3])
        ctx.specs, ctx.gates, ctx.has_rest = (box_spec, mask_spec, feat_spec), gates, rest is not None
        ctx.save_for_backward(*maps)
        ctx.set_materialize_grads(False)
        return (pooled, front, rest, feat) if rest is not None else (pooled, front, feat)

    @staticmethod
    def backward(ctx, *ds):
        maps = ctx.saved_tensors
        nl = len(maps)
        d_pooled, d_front, d_feat = (ds[0], ds[1], ds[3]) if ctx.has_rest else ds
        if d_pooled is None and d_front is None and d_feat is None:
            return (None,) * (5 + nl)
        B, C = maps[0].shape[:2]
        dev, dtype = maps[0].device, maps[0].dtype
        bufs = [torch.empty(tuple(m.shape), device=dev, dtype=torch.float32, memory_format=torch.channels_last) for m in maps]
        first = True
        for (boxes, box_ind, level, size), d in zip(ctx.specs[:2], (d_pooled, d_front)):
            if d is None:                                   # a reader without a gradient: its boxes are never touched
                continue
            d = d.to(dtype).contiguous(memory_format=torch.channels_last)
            crop_backward16(d, bufs, boxes, box_ind, level, size, accumulate=not first)
            if _lib.TAP is not None:
                _lib.TAP("pyramid_crop_backward", grads=d, boxes=boxes, box_ind=box_ind, level=level, crop=size,
                         accumulate=not first, level_grads=bufs)
            first = False
        if d_feat is not None:
            boxes, box_ind, level, size = ctx.specs[2]
            L = _lib.load()
            d = d_feat.contiguous().float()
            ptrs = (ctypes.c_void_p * nl)(*[t.data_ptr() for t in bufs])
            hs = (ctypes.c_int * nl)(*[m.shape[2] for m in maps])
            ws = (ctypes.c_int * nl)(*[m.shape[3] for m in maps])
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
            g, s = crops16.gate_pack16(buf, u if gate is not None else None, dtype=u.dtype, colsum=gate is not None)
            if gate is not None:
                gate.leave(g, s)
            out.append(g)
        return (None,) * 5 + tuple(out)


def pyramid_crops_heads16(maps16, box_spec, mask_spec, rest_spec, feat_spec):
    """(pooled, front, rest, feat) from the 16-bit channels-last maps16 as ONE autograd node; every spec is
    (boxes, box_ind, level, size):
      pooled  the size x size crops of box_spec, 16-bit channels-last (head16.pyramid_crop16_cl): the box head's input;
      front   the crops of mask_spec, 16-bit channels-last: the mask head's graph batch;
      rest    the crops of rest_spec, 16-bit channels-last, marked non-differentiable -- None when rest_spec is None;
      feat    the crops of feat_spec as fp32 NCHW (roi16.pyramid_crop16, bit for bit): the feature extractor's rows.
    The readers share no tensor.  The backward receives every reader's gradient in one call (see
    _PyramidCropsHeads16Fn) and returns 16-bit map gradients; a reader without a gradient costs nothing.  The caller promises
    that these crops are the maps' ONLY readers: a map that carries a train16.Gate16 is claimed with conv.GATES on, its
    gradient is masked here and its producer runs a premasked backward (crops16.pyramid_crops16's contract).
    Raises _lib.FiError for what the eligibility queries refuse; there is no fallback."""
    maps16 = list(maps16)
    if not maps16:
        raise _lib.FiError("pyramid_crops_heads16: no maps")
    for m in maps16:
        act16._require_act16(m, "pyramid_crops_heads16")
    L, Lc = load(), crops16.load()
    specs = [_spec(s) for s in (box_spec, mask_spec, feat_spec)]
    rest = None if rest_spec is None else _spec(rest_spec)
    C = maps16[0].shape[1]
    for boxes, _, _, size in specs[:2]:
        if L.fi_heads16_eligible(CROP_BWD, len(maps16), C, size, size, max(boxes.shape[0], 1), None, None, None, None,
                                 None) != 1:
            raise _lib.FiError("pyramid_crops_heads16: fi_heads16_eligible refuses the backward of a %d x %d crop of %d "
                               "channels from %d maps; there is no fallback" % (size, size, C, len(maps16)))
    for m in maps16:
        N, _, H, W = m.shape
        if N > 0:
            crops16._require(Lc, "pyramid_crops_heads16 (gate-pack)", crops16.GATE_PACK, 0, C, N * H * W, None, None, m, None,
                             None)
    gates = [train16._claim_gate16(m, True) for m in maps16]
    out = _PyramidCropsHeads16Fn.apply(specs[0], specs[1], rest, specs[2], gates, *maps16)
    _STATS["crops"] += 1
    return (out[0], out[1], out[2], out[3]) if rest is not None else (out[0], out[1], None, out[2])


class _ClassRowsOut16Fn(torch.autograd.Function):
    """The mask head's last layer when the loss reads one class per RoI.  Forward: the fp32 output launch over ALL K classes
    on the rows (RoI, pixel, (a, b)) of u16 (head16.out1x1_16, no activation, rows layout) and a gather of column cls[i].
    Backward: ONE class_rows_grad16 launch -- du masked with u16 > 0 and rounded once, d weight and d bias added to the
    rows of the classes, and the column sums of du left in u16's Gate16 when this layer claimed it."""

    @staticmethod
    def forward(ctx, u16, weight, bias, cls, gate):
        n, C4, H, W = u16.shape
        K, C = weight.shape[0], C4 // 4
        w16 = act16.weight16(weight, u16.dtype).view(K, C)
        rows = u16.permute(0, 2, 3, 1).reshape(n * H * W * 4, C).view(n * H * W * 4, C, 1, 1)
        logits = head16.out1x1_16(rows, w16, bias, act=head16.NONE, layout=head16.ROWS)          # [(i, p, ab), K]
        pick = cls.view(n, 1, 1).expand(n, H * W * 4, 1)
        sel = logits.view(n, H * W * 4, K).gather(2, pick).view(n, H * W, 4).permute(0, 2, 1).reshape(n, 2, 2, H, W)
        ctx.save_for_backward(u16, w16, cls)
        ctx.gate, ctx.kc = gate, (K, C)
        return sel

    @staticmethod
    def backward(ctx, d):
        u16, w16, cls = ctx.saved_tensors
        K, C = ctx.kc
        _, need_w, need_b = ctx.needs_input_grad[:3]
        dw = torch.zeros((K, C), device=u16.device, dtype=torch.float32) if need_w else None
        db = torch.zeros((K,), device=u16.device, dtype=torch.float32) if need_b else None
        du, s = class_rows_grad16(d.contiguous().float(), u16, w16, cls, dweight=dw, dbias=db, colsum=ctx.gate is not None)
        if ctx.gate is not None:
            ctx.gate.leave(du, s)
        return du, None if dw is None else dw.view(K, C, 1, 1), db, None, None


def class_rows_out16(u16, conv, cls):
    """sel [n, 2, 2, H, W] fp32: the logits of class cls[i] of RoI i behind the 2 x 2 / stride 2 transposed convolution run
    as a 1x1 layer -- u16 [n, 4 C, H, W], 16-bit channels-last with channels ordered (a, b, c), its ReLU output
    (head16.deconv2x2_act16) -- through the 1x1 convolution `conv` (C -> K, with or without a bias):
    sel[i, a, b, h, w] = out1x1_16(rows of u16)[(i, h, w, a, b), cls[i]], bit for bit.  Every class is evaluated, as the
    reference does; the loss's selection is applied behind the launch.  Differentiable: see _ClassRowsOut16Fn.  The caller
    promises that this layer is u16's ONLY reader: a Gate16 on u16 is claimed with conv.GATES on, and u16's producer then
    finds its masked gradient and column sums there.
    Raises _lib.FiError for what the eligibility queries refuse; there is no fallback."""
    act16._require_act16(u16, "class_rows_out16")
    _lib.require_cuda(cls)
    n, C4, H, W = u16.shape
    w = conv.weight
    if C4 % 4 != 0 or w.dim() != 4 or tuple(w.shape[1:]) != (C4 // 4, 1, 1) or w.dtype != torch.float32:
        raise _lib.FiError("class_rows_out16: a float32 [K, %s, 1, 1] weight behind (a, b, c)-ordered channels, got %s and "
                           "%d channels" % (C4 // 4 if C4 % 4 == 0 else "C", tuple(w.shape), C4))
    if cls.dtype != torch.int64 or tuple(cls.shape) != (n,):
        raise _lib.FiError("class_rows_out16: cls must be an int64 [%d] tensor, got %s %s" % (n, cls.dtype, tuple(cls.shape)))
    if load().fi_heads16_eligible(CLASS_ROWS, w.shape[0], C4 // 4, max(H, 1), max(W, 1), max(n, 1), None, None, None, None,
                                  None) != 1:
        raise _lib.FiError("class_rows_out16: fi_heads16_eligible refuses this layer (n %d, H %d, W %d, C %d, K %d); there "
                           "is no fallback" % (n, H, W, C4 // 4, w.shape[0]))
    gate = train16._claim_gate16(u16, True)
    return _ClassRowsOut16Fn.apply(u16, w, conv.bias, cls.contiguous(), gate)


def deconv_weight_t16(deconv, dtype):
    """The data-gradient operand of a 2 x 2 / stride 2 transposed convolution run as a 1x1 layer to (a, b, c)-ordered
    channels: wt[ci, 0, 0, (a, b, co)] = W[ci, co, a, b] rounded once to `dtype`, contiguous [Cin, 1, 1, 4 Cout].  Kept in
    conv's registry per (tensor, version) of the weight, as head16's operand copies."""
    cin, cout = deconv.weight.shape[0], deconv.weight.shape[1]
    return head16._head_copy("deconv_t", dtype, deconv.weight, (),
                             lambda: deconv.weight.detach().permute(0, 2, 3, 1).reshape(cin, 1, 1, 4 * cout).to(dtype)
                             .contiguous())


class _Deconv2x2Act16Fn(torch.autograd.Function):
    """u = relu(deconv as a 1x1 layer + bias): head16.deconv2x2_act16's launch.  Backward, with g = dy * (u > 0): g and its
    column sums s come from u's Gate16 when its claimer wrote this very dy (premasked: no relu_grad16), else from
    relu_grad16; d bias = s summed over (a, b); dW = wgrad16 of g, [4 Cout, Cin] rows (a, b, co), re-laid to the
    [Cin, Cout, 2, 2] parameter; dx = the gated data gradient when this layer claimed its input's gate, dgrad16 otherwise."""

    @staticmethod
    def forward(ctx, x16, weight, bias, deconv, in_gate, out_gate):
        u = head16.deconv2x2_act16(x16, deconv, relu=True)            # grad mode is off inside a Function's forward
        ctx.save_for_backward(x16, u, weight)
        ctx.deconv, ctx.in_gate, ctx.out_gate = deconv, in_gate, out_gate
        return u

    @staticmethod
    def backward(ctx, dy):
        x16, u, w = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        cin, cout = w.shape[0], w.shape[1]
        g, s = train16.masked_grad16(dy, u, ctx.out_gate, True, need_b)
        dw = db = dx = None
        if need_w:
            dwp = grad16.wgrad16(g, x16, 1, 1, 1, 0)                    # [4 Cout, 1, 1, Cin], rows (a, b, co)
            dw = dwp.view(2, 2, cout, cin).permute(3, 2, 0, 1).contiguous()
        if need_b:
            db = s.view(4, cout).sum(0)
        if need_x:
            dx = train16.data_grad16(g, deconv_weight_t16(ctx.deconv, x16.dtype), x16, ctx.in_gate, 1, 0)
        return dx, dw, db, None, None, None


def deconv2x2_bias_act16(x16, deconv, gate_dx=False):
    """head16.deconv2x2_act16 (the 2 x 2 / stride 2 transposed convolution before its pixel shuffle, with bias and ReLU:
    [n, 4 Cout, H, W] 16-bit channels-last, channels ordered (a, b, c)) with grad mode ON: the same launch, bit-equal output,
    which carries a train16.Gate16 -- a reader that sees its whole gradient (class_rows_out16) leaves the masked gradient
    and its column sums there and this layer runs no relu_grad16.  gate_dx: the caller's promise that this layer sees
    x16's WHOLE gradient; a Gate16 on x16 is then claimed and the data gradient is the gated launch.
    Raises _lib.FiError for what the eligibility queries refuse; there is no fallback."""
    act16._require_act16(x16, "deconv2x2_bias_act16")
    if deconv.bias is None:
        raise _lib.FiError("deconv2x2_bias_act16: the layer must carry its own bias")
    N, Cin, H, W = x16.shape
    cout = deconv.weight.shape[1]
    in_gate = train16._claim_gate16(x16, gate_dx)
    train16.require_backward16("deconv2x2_bias_act16", (N, H, W, Cin, 4 * cout, 1, 1, 1, 0), True, in_gate)
    return train16.with_out_gate16(True, lambda out_gate: _Deconv2x2Act16Fn.apply(x16, deconv.weight, deconv.bias, deconv,
                                                                                  in_gate, out_gate))


# ---- the box head's layers ----------------------------------------------------------------------------------------------
def _rows_view(x16):
    """[n, C, h, w] channels-last -> the same memory as [n, h w C, 1, 1]: a full-window layer's operand as a 1x1 layer's."""
    n, C, h, w = x16.shape
    return x16.permute(0, 2, 3, 1).reshape(n, h * w * C).view(n, h * w * C, 1, 1)


def window_weight_t16(conv, bn, scale, dtype):
    """The data-gradient operand of a full-window layer behind the eval-mode `bn`, run as a 1x1 layer on the crop's
    [R, S, Cin] run: wt[(r, s, ci), 0, 0, co] = W[co, ci, r, s] * scale[co] in fp32, rounded once; [R S Cin, 1, 1, Cout]."""
    cout = conv.weight.shape[0]
    return head16._head_copy(("window_t", _conv._fold_key(conv, bn)), dtype, conv.weight, (),
                             lambda: (conv.weight.detach() * scale.view(-1, 1, 1, 1)).permute(2, 3, 1, 0).reshape(-1, 1, 1, cout)
                             .to(dtype).contiguous())


class _WindowBnAct16Fn(torch.autograd.Function):
    """y = relu(bn(conv(x16))) for a convolution whose kernel is the whole map: head16.window_bn_act16's launch.  Backward,
    on the crop viewed as [n, 1, 1, R S Cin]: g and s from y's Gate16 (premasked) or relu_grad16; dW' = wgrad16 (tap-major
    [Cout, R S Cin]) and fi_bn_fold_grad as train16's 3x3 layers; dx = dgrad16 on the scaled, transposed weight."""

    @staticmethod
    def forward(ctx, x16, weight, bias, gamma, beta, conv, bn, scale, out_gate):
        y = head16.window_bn_act16(x16, conv, bn, relu=True)
        ctx.save_for_backward(x16, y, weight, scale)
        ctx.conv, ctx.bn, ctx.out_gate = conv, bn, out_gate
        return y

    @staticmethod
    def backward(ctx, dy):
        x16, y, w, scale = ctx.saved_tensors
        conv, bn = ctx.conv, ctx.bn
        need_x, need_w, need_b, need_gamma, need_beta = ctx.needs_input_grad[:5]
        Cout, Cin, R, S = w.shape
        g, s = train16.masked_grad16(dy, y, ctx.out_gate, True, True)
        xv = _rows_view(x16)
        # dW' [Cout, 1, 1, R S Cin] is tap-major: its [Cout, R, S, Cin] view goes through the 3x3 layers' channels-last view
        dwp, dgamma, dbias = train16.fold_weight_grad16(g, xv, w, conv, bn, scale, s, 1, 1, 1, 0, need_w, need_gamma, need_b)
        dw = train16.dw_view16(dwp.view(Cout, R, S, Cin), R, S) if need_w else None
        dx = None
        if need_x:
            dxv = train16.data_grad16(g, window_weight_t16(conv, bn, scale, x16.dtype), xv, None, 1, 0)
            dx = dxv.view(x16.shape[0], R, S, Cin).permute(0, 3, 1, 2)
        return dx, dw, dbias, dgamma, s if need_beta else None, None, None, None, None


def window_bn_act16(x16, conv, bn):
    """head16.window_bn_act16 (relu(bn(conv(x16))) for a kernel that is the whole map, [n, Cout, 1, 1]) with grad mode ON:
    the same launch, bit-equal output, which carries a train16.Gate16.  The weight gradient has the channels-last strides
    of the tap-major buffer.  Raises _lib.FiError for what the eligibility queries refuse; there is no fallback."""
    act16.require_eval_bn("heads16.window_bn_act16", bn)
    act16._require_act16(x16, "heads16.window_bn_act16")
    fold = act16.eval_fold("heads16.window_bn_act16", conv, bn)
    n, C, h, w = x16.shape
    Cout = conv.weight.shape[0]
    if tuple(conv.weight.shape[1:]) != (C, h, w):
        raise _lib.FiError("heads16.window_bn_act16: the layer's kernel must be the whole %d x %d map of %d channels (weight "
                           "%s)" % (h, w, C, tuple(conv.weight.shape)))
    train16.require_backward16("heads16.window_bn_act16", (n, 1, 1, h * w * C, Cout, 1, 1, 1, 0))
    return train16.with_out_gate16(True, lambda out_gate: _WindowBnAct16Fn.apply(x16, conv.weight, conv.bias, bn.weight,
                                                                                 bn.bias, conv, bn, fold[0], out_gate))


def stacked_linear_t16(linears, dtype):
    """The data-gradient operand of head16.stacked_linear16's matrix: its transpose, zero-padded to the next multiple of 32
    columns, [Cin, 1, 1, Kp] 16-bit.  Kept in conv's registry per (tensors, versions) of the weights, as the other operand
    copies."""
    ws = [l.weight for l in linears]
    K, Cin = sum(w.shape[0] for w in ws), ws[0].shape[1]
    Kp = (K + 31) // 32 * 32

    def make():
        wt = torch.zeros((Cin, 1, 1, Kp), device=ws[0].device, dtype=dtype)
        wt[:, 0, 0, :K] = torch.cat([w.detach() for w in ws], 0).to(dtype).t()
        return wt
    return head16._head_copy("stack_t", dtype, ws[0], ws[1:], make)


class _StackedOut16Fn(torch.autograd.Function):
    """heads [n, sum of rows] fp32 = x16 . stacked(weights)^T + stacked(biases): head16.out1x1_16 on head16.stacked_linear16's
    operands.  Backward: the fp32 gradient is zero-padded to the next multiple of 32 columns and cast with torch ops (it is
    tiny); dx = the gated data gradient on the padded, transposed 16-bit weight when the layer claimed x16's gate, dgrad16
    otherwise; dW = wgrad16, its rows split back onto the layers; the bias gradients are the fp32 column sums."""

    @staticmethod
    def forward(ctx, x16, linears, in_gate, *params):
        w, b = head16.stacked_linear16(linears, x16.dtype)
        y = head16.out1x1_16(x16, w, b, act=head16.NONE, layout=head16.ROWS)
        ctx.save_for_backward(x16, w)
        ctx.in_gate, ctx.rows = in_gate, [l.weight.shape[0] for l in linears]
        ctx.wt = lambda: stacked_linear_t16(linears, x16.dtype)
        return y

    @staticmethod
    def backward(ctx, d):
        x16, w = ctx.saved_tensors
        n, Cin = x16.shape[0], x16.shape[1]
        K = w.shape[0]
        Kp = (K + 31) // 32 * 32
        d = d.contiguous().float()
        g = torch.zeros((n, Kp), device=d.device, dtype=x16.dtype)
        g[:, :K] = d
        g = g.view(n, Kp, 1, 1)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = train16.data_grad16(g, ctx.wt(), x16, ctx.in_gate, 1, 0)
        need = ctx.needs_input_grad[3:]
        dwp = grad16.wgrad16(g, x16, 1, 1, 1, 0).view(Kp, Cin) if any(need[0::2]) else None
        db = d.sum(0) if any(need[1::2]) else None
        out, at = [], 0
        for i, r in enumerate(ctx.rows):
            out.append(dwp[at:at + r] if ctx.needs_input_grad[3 + 2 * i] else None)
            out.append(db[at:at + r] if ctx.needs_input_grad[4 + 2 * i] else None)
            at += r
        return (dx, None, None) + tuple(out)


def stacked_out16(x16, linears, gate_dx=False):
    """fp32 [n, sum of rows]: several nn.Linear layers over the same [n, Cin, 1, 1] 16-bit input as ONE output launch
    (head16.out1x1_16 on their stacked weights and biases), differentiable: see _StackedOut16Fn.  gate_dx: the caller's
    promise that this layer sees x16's whole gradient; a Gate16 on x16 is then claimed.
    Raises _lib.FiError for what the eligibility queries refuse; there is no fallback."""
    act16._require_act16(x16, "stacked_out16")
    linears = tuple(linears)
    n, Cin, H, W = x16.shape
    if (H, W) != (1, 1) or any(l.bias is None or l.weight.shape[1] != Cin for l in linears):
        raise _lib.FiError("stacked_out16: [n, Cin, 1, 1] rows and linear layers of Cin inputs with a bias each, got %s"
                           % (tuple(x16.shape),))
    K = sum(l.weight.shape[0] for l in linears)
    in_gate = train16._claim_gate16(x16, gate_dx)
    train16.require_backward16("stacked_out16", (n, 1, 1, Cin, (K + 31) // 32 * 32, 1, 1, 1, 0), False, in_gate)
    params = []
    for l in linears:
        params += [l.weight, l.bias]
    return _StackedOut16Fn.apply(x16, linears, in_gate, *params)
