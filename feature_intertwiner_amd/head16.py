"""The box head and the mask head on 16-bit channels-last crops (libfi_head16.so, include/fi_head16.h, csrc/head16_crop.hip,
csrc/head16_out.hip): RoIAlign that reads 16-bit pyramid maps and writes 16-bit channels-last crops, the heads' layers on the
existing fi_act16_conv_forward entry point, and the 1x1 output layer that writes fp32 for any number of output channels with
an optional sigmoid and pixel shuffle.  Inference only (MODEL.ACT_SCOPE = 'detect' next to a 16-bit MODEL.ACT_PRECISION).

Tensors are act16's: [N, C, H, W]-shaped torch.channels_last bfloat16 / float16.  Which calls the kernels take is decided by
fi_head16_crop_eligible / fi_head16_out1x1_eligible / fi_act16_conv_eligible alone; nothing here restates their rules, and a
call they refuse is an error -- there is no fallback to another path.

Weights.  Three operands are re-laid-out 16-bit copies that no other path keeps: the box head's full-window weight in tap-major
order ([1024, 7 * 7 * 256]: Classifier.conv1 is full_window, so prepare_step leaves it row-major), the class and box linears
stacked to one [405, 1024] matrix with their stacked bias, and the mask head's transposed convolution as a 1x1 weight to
(a, b, c)-ordered channels with its bias repeated.  Each is made once per (tensors, versions) and kept in conv's registry of
weight copies (step_state.HEAD); stats()['weights'] counts the copies made.  The other layers' weights are the 16-bit copies
act16.weight16 already keeps there.
"""
import ctypes

import torch

from . import _lib
from . import act16 as _act16
from . import conv as _conv
from . import pyr16 as _pyr16
from . import step_state as _step_state

LIB_PATH = _lib.sublibrary_path("head16")
_cp, _ci, _cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
_pp, _ip = ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int)
_CROP = (_ci, [_pp, _ip, _ip, _ci, _cp, _cp, _cp, _ci, _ci, _ci, _ci, _ci, _cf, _cp, _cp])
_OUT = (_ci, [_cp, _cp, _cp, _cp, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _cp])
# name -> (restype, argtypes); mirrors include/fi_head16.h one to one
SIGNATURES = {
    "fi_head16_crop_eligible": (_ci, [_ci, _ci, _ci, _ci, _pp, _cp]),
    "fi_head16_pyramid_crop_forward_bf16": _CROP,
    "fi_head16_pyramid_crop_forward_f16": _CROP,
    "fi_head16_out1x1_eligible": (_ci, [_ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _cp, _cp, _cp]),
    "fi_head16_out1x1_bf16": _OUT,
    "fi_head16_out1x1_f16": _OUT,
}
_STATS = {"crop": 0, "conv": 0, "out": 0, "weights": 0}
ROWS, SHUFFLE = 0, 1          # out1x1_16's layouts
NONE, SIGMOID = 0, 1          # ... and activations


def load():
    """Load libfi_head16.so (after libfi_hip.so, which it links against) and attach the signatures."""
    return _lib.load_sublibrary("head16", SIGNATURES)


def stats():
    """Host counters since reset_stats(): {'crop', 'conv', 'out'} launches and {'weights'} operand copies made."""
    return dict(_STATS)


def reset_stats():
    _lib.zero_counters(_STATS)


def pyramid_crop16_cl(maps16, boxes, box_ind, level, crop_h, crop_w, extrapolation_value=0.0):
    """crops[i] = crop_h x crop_w RoIAlign of box i from maps16[level[i] - 2] (image box_ind[i]) in the maps' 16-bit type:
    logical shape [num_boxes, C, crop_h, crop_w] in channels-last memory ([num_boxes, crop_h, crop_w, C]), one launch for
    all levels.  The values are roi16.pyramid_crop16's rounded once to the type.  Rows with a level outside the pyramid or
    a box_ind outside the batch are zeros; a row with level -1 is left unwritten.  `level` may be None for a single map."""
    _pyr16._require_inference("pyramid_crop16_cl")
    maps16 = list(maps16)
    if not maps16:
        raise _lib.FiError("pyramid_crop16_cl: no maps")
    prec = _act16._require_act16(maps16[0], "pyramid_crop16_cl")
    first = maps16[0]
    for m in maps16[1:]:
        _act16._require_act16(m, "pyramid_crop16_cl")
        if m.dtype != first.dtype or m.device != first.device or m.shape[:2] != first.shape[:2]:
            raise _lib.FiError("pyramid_crop16_cl: the maps must share dtype, device, batch and channel count; got %s %s on "
                               "%s next to %s %s on %s" % (m.dtype, tuple(m.shape), m.device, first.dtype,
                                                           tuple(first.shape), first.device))
    _lib.require_cuda(boxes, box_ind, level)
    L = load()
    nl = len(maps16)
    B, C = first.shape[:2]
    boxes_c = boxes.detach().contiguous().float()
    ind_c = box_ind.detach().contiguous().to(torch.int32)
    lvl_c = None if level is None else level.detach().contiguous().to(torch.int32)
    N = boxes_c.shape[0]
    if boxes_c.dim() != 2 or boxes_c.shape[1] != 4 or ind_c.numel() != N or (lvl_c is not None and lvl_c.numel() != N):
        raise _lib.FiError("pyramid_crop16_cl: boxes [n, 4] with box_ind [n] and level [n]; got %s, %s, %s"
                           % (tuple(boxes.shape), tuple(box_ind.shape), None if level is None else tuple(level.shape)))
    crop_h, crop_w = int(crop_h), int(crop_w)
    crops = torch.empty((N, max(crop_h, 0), max(crop_w, 0), C), device=first.device, dtype=first.dtype)
    ptrs = (ctypes.c_void_p * nl)(*[m.data_ptr() for m in maps16])
    hs = (ctypes.c_int * nl)(*[m.shape[2] for m in maps16])
    ws = (ctypes.c_int * nl)(*[m.shape[3] for m in maps16])
    if N > 0 and L.fi_head16_crop_eligible(nl, C, crop_h, crop_w, ptrs, _lib.ptr(crops)) != 1:
        raise _lib.FiError("pyramid_crop16_cl: fi_head16_crop_eligible refuses this call (%d maps, %d channels, crop %d x "
                           "%d); there is no fallback" % (nl, C, crop_h, crop_w))
    _act16._launch(first.device, "fi_head16_pyramid_crop_forward", _conv._lowp_fn(L, "head16_pyramid_crop_forward", prec),
                   ptrs, hs, ws, nl, _lib.ptr(boxes_c), _lib.ptr(ind_c), _lib.ptr(lvl_c), N, B, C, crop_h, crop_w,
                   float(extrapolation_value), _lib.ptr(crops))
    _STATS["crop"] += 1
    return crops.permute(0, 3, 1, 2)


# ---- operand copies -------------------------------------------------------------------------------------------------------
def _head_copy(what, dtype, first, others, make):
    """The copy `make()` builds from the tensors (first, *others), once per (tensors, versions): kept in the record of
    `first` in conv's registry, which checks first's owner and version; the addresses and versions of the others are
    part of what a lookup expects."""
    expect = (what, dtype, tuple((t.data_ptr(), t._version) for t in others))
    got = _conv._COPIES.lookup(first, _step_state.HEAD, expect)
    if got is None:
        got = make()
        _conv._COPIES.publish(first, _step_state.HEAD, got, expect)
        _STATS["weights"] += 1
    return got


def window_weight16(weight, dtype):
    """The tap-major 16-bit [Cout, R * S * Cin] copy of a full-window [Cout, Cin, R, S] weight: the order of a
    channels-last crop's [R, S, Cin] run."""
    Cout = weight.shape[0]
    return _head_copy("window", dtype, weight, (),
                      lambda: weight.detach().to(dtype).permute(0, 2, 3, 1).contiguous().view(Cout, -1))


def stacked_linear16(linears, dtype):
    """(weight [sum of rows, Cin] 16-bit, bias [sum of rows] fp32) of several nn.Linear layers over the same input, stacked
    in their order."""
    tensors = [l.weight for l in linears] + [l.bias for l in linears]
    if any(t is None for t in tensors):
        raise _lib.FiError("stacked_linear16: every layer needs a bias")
    return _head_copy("stack", dtype, tensors[0], tensors[1:],
                      lambda: (torch.cat([l.weight.detach() for l in linears], 0).to(dtype),
                               torch.cat([l.bias.detach() for l in linears], 0).float()))


def deconv_weight16(deconv, dtype):
    """(weight [4 * Cout, Cin] 16-bit with rows ordered (a, b, c), bias [4 * Cout] fp32 or None) of a 2 x 2 / stride 2
    transposed convolution run as a 1x1 convolution: out[n, c, 2h + a, 2w + b] = y[n, (a, b, c), h, w]."""
    cin, cout = deconv.weight.shape[0], deconv.weight.shape[1]
    others = () if deconv.bias is None else (deconv.bias,)
    return _head_copy("deconv", dtype, deconv.weight, others,
                      lambda: (deconv.weight.detach().permute(2, 3, 1, 0).reshape(4 * cout, cin).to(dtype).contiguous(),
                               None if deconv.bias is None else deconv.bias.detach().float().repeat(4)))


# ---- the heads' layers on fi_act16_conv_forward ---------------------------------------------------------------------------
def _conv_launch(what, x16, prec, w16, scale, shift, relu, N, H, W, Cin, Cout, R, S, stride, pad):
    """One fi_act16_conv_forward launch, counted in stats()['conv']: y [N, Cout, OH, OW] 16-bit channels-last."""
    A = _act16.load()
    OH = (H + 2 * pad - R) // stride + 1
    OW = (W + 2 * pad - S) // stride + 1
    y = torch.empty((N, Cout, max(OH, 0), max(OW, 0)), device=x16.device, dtype=x16.dtype,
                    memory_format=torch.channels_last)
    args = (N, H, W, Cin, Cout, R, S, stride, pad)
    if N > 0 and A.fi_act16_conv_eligible(*args, _lib.ptr(x16), _lib.ptr(w16), None, _lib.ptr(y)) != 1:
        raise _lib.FiError("%s: fi_act16_conv_eligible refuses this layer (N %%d, H %%d, W %%d, Cin %%d, Cout %%d, "
                           "R %%d, S %%d, stride %%d, pad %%d); there is no fallback" % what % args)
    _act16._launch(x16.device, "fi_act16_conv_forward", _conv._lowp_fn(A, "act16_conv_forward", prec), _lib.ptr(x16),
                   _lib.ptr(w16), _lib.ptr(scale), _lib.ptr(shift), None, _lib.ptr(y), *args, 1 if relu else 0)
    _STATS["conv"] += 1
    return y


def _enter(what, x16):
    _pyr16._require_inference(what)
    return _act16._require_act16(x16, what)


def window_bn_act16(x16, conv, bn, relu=True):
    """act(bn(conv(x16))) for a convolution whose kernel is the whole map (the box head's 7x7 layer on 7x7 crops): a 1x1
    layer on the crop viewed as [n, 1, 1, R * S * Cin] with the tap-major weight; [n, Cout, 1, 1]."""
    prec = _enter("window_bn_act16", x16)
    n, C, h, w = x16.shape
    Cout = conv.weight.shape[0]
    if tuple(conv.weight.shape[1:]) != (C, h, w) or tuple(conv.padding) != (0, 0) or tuple(conv.dilation) != (1, 1) or \
            conv.groups != 1:
        raise _lib.FiError("window_bn_act16: the layer's kernel must be the whole %d x %d map of %d channels without padding "
                           "(weight %s, padding %s)" % (h, w, C, tuple(conv.weight.shape), tuple(conv.padding)))
    scale, shift = _act16.eval_fold("window_bn_act16", conv, bn)
    w16 = window_weight16(conv.weight, x16.dtype)
    return _conv_launch("window_bn_act16", x16, prec, w16, scale, shift, relu, n, 1, 1, h * w * C, Cout, 1, 1, 1, 0)


def conv_bn_act16(x16, conv, bn, relu=True):
    """act(bn(conv(x16))) for a 1x1 or a padded 3x3 layer of a head (what fi_act16_conv_eligible takes): act16.conv_bn_act16
    without a residual, counted here."""
    prec = _enter("conv_bn_act16", x16)
    N, Cin, H, W = x16.shape
    Cout, wc, R, S = conv.weight.shape
    stride, pad = conv.stride, conv.padding
    if stride[0] != stride[1] or pad[0] != pad[1] or tuple(conv.dilation) != (1, 1) or conv.groups != 1 or wc != Cin:
        raise _lib.FiError("conv_bn_act16: the layer must be a dense square-stride convolution of the input's %d channels "
                           "(stride %s, padding %s, dilation %s, groups %d, weight %s)"
                           % (Cin, tuple(stride), tuple(pad), tuple(conv.dilation), conv.groups, tuple(conv.weight.shape)))
    scale, shift = _act16.eval_fold("conv_bn_act16", conv, bn)
    w16 = _act16.weight16(conv.weight, x16.dtype)
    return _conv_launch("conv_bn_act16", x16, prec, w16, scale, shift, relu, N, H, W, Cin, Cout, R, S, stride[0], pad[0])


def deconv2x2_act16(x16, deconv, relu=True):
    """The 2 x 2 / stride 2 transposed convolution BEFORE its pixel shuffle, with bias and ReLU: [n, 4 * Cout, H, W] 16-bit
    channels-last with channels ordered (a, b, c) -- in memory the rows ((n, h, w), a, b) of Cout values that
    out1x1_16(layout=SHUFFLE) reads."""
    prec = _enter("deconv2x2_act16", x16)
    N, Cin, H, W = x16.shape
    if deconv.kernel_size != (2, 2) or deconv.stride != (2, 2) or deconv.padding != (0, 0) or \
            deconv.output_padding != (0, 0) or deconv.groups != 1 or deconv.weight.shape[0] != Cin:
        raise _lib.FiError("deconv2x2_act16: the layer must be a dense 2 x 2 / stride 2 transposed convolution of the input's "
                           "%d channels without padding (weight %s)" % (Cin, tuple(deconv.weight.shape)))
    w16, b4 = deconv_weight16(deconv, x16.dtype)
    return _conv_launch("deconv2x2_act16", x16, prec, w16, None, b4, relu, N, H, W, Cin, w16.shape[0], 1, 1, 1, 0)


# ---- the output layer -----------------------------------------------------------------------------------------------------
def out1x1_16(x16, weight, bias=None, act=NONE, layout=ROWS):
    """act(x w^T + bias) in fp32, one launch.  weight: a 16-bit [Cout, Cin] matrix of x16's type, or an fp32
    [Cout, Cin, 1, 1] convolution weight (its 16-bit copy is act16.weight16's).  act: NONE or SIGMOID.
    layout ROWS: x16 [N, Cin, H, W] -> fp32 [N * H * W, Cout].
    layout SHUFFLE: x16 [n, 4 * Cin, H, W] with channels ordered (a, b, c), deconv2x2_act16's output -> fp32
    [n, Cout, 2H, 2W] with y[n, co, 2h + a, 2w + b]."""
    prec = _enter("out1x1_16", x16)
    L = load()
    N, C, H, W = x16.shape
    if layout == SHUFFLE and C % 4 != 0:
        raise _lib.FiError("out1x1_16: the shuffle layout reads (a, b, c)-ordered channels; %d is no multiple of 4" % C)
    Cin = C // 4 if layout == SHUFFLE else C
    P = N * H * W * (4 if layout == SHUFFLE else 1)
    if weight.dim() == 4 and tuple(weight.shape[1:]) == (Cin, 1, 1) and weight.dtype == torch.float32:
        _lib.require_cuda(weight)
        weight = _act16.weight16(weight, x16.dtype).view(weight.shape[0], Cin)      # once per (tensor, version)
    if weight.dim() != 2 or weight.shape[1] != Cin or weight.dtype != x16.dtype or not weight.is_contiguous():
        raise _lib.FiError("out1x1_16: expected a contiguous %s [Cout, %d] or an fp32 [Cout, %d, 1, 1] weight, got %s %s"
                           % (x16.dtype, Cin, Cin, weight.dtype, tuple(weight.shape)))
    _lib.require_cuda(weight, bias)
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != weight.shape[0] or not bias.is_contiguous()):
        raise _lib.FiError("out1x1_16: the bias must be fp32 [%d], got %s %s" % (weight.shape[0], bias.dtype, tuple(bias.shape)))
    Cout = weight.shape[0]
    shape = (N, Cout, 2 * H, 2 * W) if layout == SHUFFLE else (P, Cout)
    y = torch.empty(shape, device=x16.device, dtype=torch.float32)
    args = (P, Cin, Cout, int(act), int(layout), N, H, W)
    if P > 0 and L.fi_head16_out1x1_eligible(*args, _lib.ptr(x16), _lib.ptr(weight), _lib.ptr(y)) != 1:
        raise _lib.FiError("out1x1_16: fi_head16_out1x1_eligible refuses this layer (P %d, Cin %d, Cout %d, act %d, layout %d, "
                           "n %d, H %d, W %d); there is no fallback" % args)
    _act16._launch(x16.device, "fi_head16_out1x1", _conv._lowp_fn(L, "head16_out1x1", prec), _lib.ptr(x16), _lib.ptr(weight),
                   _lib.ptr(bias), _lib.ptr(y), *args)
    _STATS["out"] += 1
    return y
