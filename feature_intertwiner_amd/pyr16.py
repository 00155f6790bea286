"""16-bit channels-last activation tensors past the trunk: the feature pyramid's lateral step and the RPN's stacked 1x1 heads
(libfi_pyr16.so, include/fi_pyr16.h, csrc/conv_pyr16.hip), and the bias-only convolutions between them on the existing
fi_act16_conv_forward entry point.  Inference only (MODEL.ACT_SCOPE = 'pyramid' next to a 16-bit MODEL.ACT_PRECISION).

Tensors are act16's: [N, C, H, W]-shaped torch.channels_last bfloat16 / float16.  Which calls the two kernels take is
decided by fi_pyr16_lateral_eligible / fi_pyr16_head1x1_eligible alone; nothing here restates their rules, and a call they
refuse is an error -- there is no fallback to another path.
"""
import ctypes

import torch

from . import _lib
from . import act16 as _act16
from . import conv as _conv

LIB_PATH = _lib.sublibrary_path("pyr16")
_cp, _ci = ctypes.c_void_p, ctypes.c_int
_LATERAL = (_ci, [_cp, _cp, _cp, _cp, _cp, _ci, _ci, _ci, _ci, _ci, _cp])
_HEAD = (_ci, [_cp, _cp, _cp, _cp, _ci, _ci, _ci, _ci, _ci, _cp])
# name -> (restype, argtypes); mirrors include/fi_pyr16.h one to one
SIGNATURES = {
    "fi_pyr16_lateral_eligible": (_ci, [_ci, _ci, _ci, _ci, _ci, _cp, _cp, _cp, _cp]),
    "fi_pyr16_lateral_bf16": _LATERAL,
    "fi_pyr16_lateral_f16": _LATERAL,
    "fi_pyr16_head1x1_eligible": (_ci, [_ci, _ci, _ci, _ci, _ci, _cp, _cp, _cp]),
    "fi_pyr16_head1x1_bf16": _HEAD,
    "fi_pyr16_head1x1_f16": _HEAD,
}
_STATS = {"lateral": 0, "head": 0}
SCOPES = ("trunk", "pyramid", "roi", "detect")


def load():
    """Load libfi_pyr16.so (after libfi_hip.so, which it links against) and attach the signatures."""
    return _lib.load_sublibrary("pyr16", SIGNATURES)


def stats():
    """Host counters of the launches since reset_stats(): {'lateral', 'head'}."""
    return dict(_STATS)


def reset_stats():
    _lib.zero_counters(_STATS)


def act_scope(model_cfg):
    """MODEL.ACT_SCOPE of a configuration's MODEL node: 'trunk' (absent: the 16-bit tensors end behind C5), 'pyramid'
    (they run on through p2..p6 to the RPN's outputs), 'roi' (everything 'pyramid' does, and the make-up layer and
    RoIAlign read and write them too: roi16) or 'detect' (everything 'roi' does, and the crops and both heads stay 16-bit
    channels-last up to the fp32 outputs: head16).  Every scope but 'trunk' needs a 16-bit MODEL.ACT_PRECISION; ValueError
    otherwise, and for any other value."""
    scope = getattr(model_cfg, "ACT_SCOPE", "trunk")
    act = getattr(model_cfg, "ACT_PRECISION", "fp32")
    if scope not in SCOPES:
        raise ValueError("MODEL.ACT_SCOPE is 'trunk', 'pyramid', 'roi' or 'detect', got %r (MODEL.ACT_PRECISION = %r)" % (scope, act))
    if scope != "trunk" and act not in _conv._LOWP:
        raise ValueError("MODEL.ACT_SCOPE = %r needs MODEL.ACT_PRECISION = 'bf16' or 'fp16', got %r" % (scope, act))
    return scope


def _require_inference(what):
    if torch.is_grad_enabled():
        raise _lib.FiError("%s is forward only: call it under torch.no_grad() (training on 16-bit activation tensors is "
                           "not built)" % what)


def conv_bias_act16(x16, conv, relu=False):
    """act(conv(x16) + bias) on 16-bit channels-last tensors for a convolution with its own bias and no BatchNorm
    (P5_conv1, the smoothing convolutions, the RPN's shared convolution): one fi_act16_conv_forward launch with no
    scale, counted in act16.stats()['conv'].  Raises _lib.FiError for a layer fi_act16_conv_eligible refuses."""
    prec = _act16._require_act16(x16, "conv_bias_act16")
    _require_inference("conv_bias_act16")
    return _act16._conv16("conv_bias_act16", x16, prec, conv, None, conv.bias, relu, None)


def _require_1x1(what, weight, Cin):
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (1, 1) or weight.shape[1] != Cin:
        raise _lib.FiError("%s: expected a [Cout, %d, 1, 1] weight, got %s" % (what, Cin, tuple(weight.shape)))


def lateral16(x16, conv, top16):
    """round16((conv1x1(x16) + bias) + top16[:, :, oh >> 1, ow >> 1]): the pyramid's top-down step, one launch; top16 is
    the coarser level [N, Cout, H/2, W/2] and is read at half resolution -- no upsampled map exists."""
    prec = _act16._require_act16(x16, "lateral16")
    _act16._require_act16(top16, "lateral16 (top)")
    _require_inference("lateral16")
    L = load()
    dtype = x16.dtype
    N, Cin, H, W = x16.shape
    _require_1x1("lateral16", conv.weight, Cin)
    Cout = conv.weight.shape[0]
    if tuple(conv.stride) != (1, 1) or tuple(conv.padding) != (0, 0) or tuple(conv.dilation) != (1, 1) or conv.groups != 1:
        raise _lib.FiError("lateral16: the layer must be a dense 1x1 convolution of stride 1 without padding (stride %s, "
                           "padding %s, dilation %s, groups %d)"
                           % (tuple(conv.stride), tuple(conv.padding), tuple(conv.dilation), conv.groups))
    if top16.dtype != dtype or tuple(top16.shape) != (N, Cout, H // 2, W // 2):
        raise _lib.FiError("lateral16: top %s %s is not the half-resolution map %s %s of the output"
                           % (top16.dtype, tuple(top16.shape), dtype, (N, Cout, H // 2, W // 2)))
    w16 = _act16.weight16(conv.weight, dtype)
    y = torch.empty((N, Cout, H, W), device=x16.device, dtype=dtype, memory_format=torch.channels_last)
    args = (N, H, W, Cin, Cout)
    if N > 0 and L.fi_pyr16_lateral_eligible(*args, _lib.ptr(x16), _lib.ptr(w16), _lib.ptr(top16), _lib.ptr(y)) != 1:
        raise _lib.FiError("lateral16: fi_pyr16_lateral_eligible refuses this layer (N %d, H %d, W %d, Cin %d, Cout %d); "
                           "there is no fallback" % args)
    _act16._launch(x16.device, "fi_pyr16_lateral", _conv._lowp_fn(L, "pyr16_lateral", prec), _lib.ptr(x16), _lib.ptr(w16),
                   _lib.ptr(conv.bias), _lib.ptr(top16), _lib.ptr(y), *args)
    _STATS["lateral"] += 1
    return y


def head1x1_16(x16, weight, bias=None):
    """conv1x1(x16, weight) + bias in fp32 for a [Cout, Cin, 1, 1] fp32 weight with Cout <= 64, one launch: an fp32 tensor of
    logical shape [N, Cout, H, W] in channels-last memory ([N, H, W, Cout]: the anchors' order)."""
    prec = _act16._require_act16(x16, "head1x1_16")
    _require_inference("head1x1_16")
    L = load()
    N, Cin, H, W = x16.shape
    _require_1x1("head1x1_16", weight, Cin)
    Cout = weight.shape[0]
    w16 = _act16.weight16(weight, x16.dtype)
    y = torch.empty((N, Cout, H, W), device=x16.device, dtype=torch.float32, memory_format=torch.channels_last)
    args = (N, H, W, Cin, Cout)
    if N > 0 and L.fi_pyr16_head1x1_eligible(*args, _lib.ptr(x16), _lib.ptr(w16), _lib.ptr(y)) != 1:
        raise _lib.FiError("head1x1_16: fi_pyr16_head1x1_eligible refuses this layer (N %d, H %d, W %d, Cin %d, Cout %d); "
                           "there is no fallback" % args)
    _act16._launch(x16.device, "fi_pyr16_head1x1", _conv._lowp_fn(L, "pyr16_head1x1", prec), _lib.ptr(x16), _lib.ptr(w16),
                   _lib.ptr(bias), _lib.ptr(y), *args)
    _STATS["head"] += 1
    return y
