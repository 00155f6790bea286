"""Backward of the convolutions on 16-bit channels-last activation tensors (libfi_grad16.so, include/fi_grad16.h,
csrc/conv_grad16.hip): the ReLU mask with its column sums, the data gradient and the weight gradient as thin wrappers,
and `conv_bn_act16`, the differentiable form of act16.conv_bn_act16 for use WITH grad mode on.

Step one of 16-bit training: the operators and one differentiable layer.  The model is not wired to THIS layer --
MaskRCNN(mode='train') with a 16-bit MODEL.ACT_PRECISION keeps raising; TRAIN.ACT_PRECISION runs the trunk on train16's
layer, which calls the operators here.  Which layers the kernels take is decided by
fi_grad16_eligible alone; nothing here restates its rules, and a layer it refuses is an error -- there is no fallback.
"""
import ctypes

import torch

from . import _lib
from . import act16
from . import conv as _conv
from . import step_state

LIB_PATH = _lib.sublibrary_path("grad16")
_cp, _ci = ctypes.c_void_p, ctypes.c_int
_RELU = (_ci, [_cp, _cp, _cp, _cp, _ci, _ci, _ci, _ci, _ci, _cp])
_DGRAD = (_ci, [_cp, _cp, _cp, _cp, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _cp])
_WGRAD = (_ci, [_cp, _cp, _cp, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _cp])
# name -> (restype, argtypes); mirrors include/fi_grad16.h one to one
SIGNATURES = {
    "fi_grad16_eligible": (_ci, [_ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _cp, _cp, _cp, _cp]),
    "fi_grad16_relu_grad_bf16": _RELU,
    "fi_grad16_relu_grad_f16": _RELU,
    "fi_grad16_conv_dgrad_bf16": _DGRAD,
    "fi_grad16_conv_dgrad_f16": _DGRAD,
    "fi_grad16_conv_wgrad_bf16": _WGRAD,
    "fi_grad16_conv_wgrad_f16": _WGRAD,
}
RELU_GRAD, DGRAD, WGRAD = 0, 1, 2          # FI_GRAD16_* kinds of fi_grad16_eligible
_STATS = {"relu_grad": 0, "dgrad": 0, "wgrad": 0, "weights": 0}


def load():
    """Load libfi_grad16.so (after libfi_hip.so, which it links against) and attach the signatures."""
    return _lib.load_sublibrary("grad16", SIGNATURES)


def stats():
    """Host counters since reset_stats(): the launches {'relu_grad', 'dgrad', 'wgrad'} and 'weights', the data-gradient
    operands (scaled, flipped, transposed 16-bit weights) built."""
    return dict(_STATS)


def reset_stats():
    _lib.zero_counters(_STATS)


def _require_eligible(L, what, kind, geom, *ptrs):
    if L.fi_grad16_eligible(kind, *geom, *[_lib.ptr(p) for p in ptrs]) != 1:
        raise _lib.FiError("%s: fi_grad16_eligible refuses this layer (N %%d, H %%d, W %%d, Cin %%d, Cout %%d, R %%d, S %%d, "
                           "stride %%d, pad %%d); there is no fallback" % what % tuple(geom))


def relu_grad16(dy, y, relu=True, colsum=True):
    """(g, s): g = dy * (y > 0) (dy itself copied when relu is False) as a 16-bit channels-last tensor and, when
    `colsum`, s [Cout] fp32 = the per-channel sums of g (else None).  One launch."""
    prec = act16._require_act16(dy, "relu_grad16 (dy)")
    if relu or y is not None:
        act16._require_act16(y, "relu_grad16 (y)")
        if y.dtype != dy.dtype or y.shape != dy.shape:
            raise _lib.FiError("relu_grad16: y %s %s does not match dy %s %s" % (y.dtype, tuple(y.shape), dy.dtype,
                                                                                tuple(dy.shape)))
    L = load()
    N, C, OH, OW = dy.shape
    g = torch.empty_like(dy, memory_format=torch.channels_last)
    s = torch.empty(C, device=dy.device, dtype=torch.float32) if colsum else None
    if N > 0:
        _require_eligible(L, "relu_grad16", RELU_GRAD, (N, OH, OW, 32, C, 1, 1, 1, 0), dy, y, g, s)
    elif s is not None:
        s.zero_()
    act16._launch(dy.device, "fi_grad16_relu_grad", _conv._lowp_fn(L, "grad16_relu_grad", prec), _lib.ptr(dy), _lib.ptr(y),
                  _lib.ptr(g), _lib.ptr(s), N, OH, OW, C, 1 if relu else 0)
    _STATS["relu_grad"] += 1
    return g, s


def dgrad16(g, wt, in_hw, stride=1, pad=0, dx_add=None):
    """dx [N, Cin, H, W] (16-bit channels-last) of a layer whose masked output gradient is g [N, Cout, OH, OW]; wt
    [Cin, R, S, Cout] the contiguous 16-bit data-gradient operand (transposed, taps flipped, BatchNorm scale folded in);
    dx_add: a 16-bit tensor added before the one rounding.  One launch."""
    prec = act16._require_act16(g, "dgrad16 (g)")
    _lib.require_cuda(wt)
    if wt.dim() != 4 or wt.dtype != g.dtype or not wt.is_contiguous() or wt.shape[3] != g.shape[1]:
        raise _lib.FiError("dgrad16: wt must be a contiguous [Cin, R, S, Cout] tensor of g's dtype and %d channels, got %s %s"
                           % (g.shape[1], wt.dtype, tuple(wt.shape)))
    L = load()
    N, Cout, OH, OW = g.shape
    Cin, R, S, _ = wt.shape
    H, W = in_hw
    if (H + 2 * pad - R) // stride + 1 != OH or (W + 2 * pad - S) // stride + 1 != OW:
        raise _lib.FiError("dgrad16: a %dx%d / stride %d / pad %d layer on %dx%d does not give g's %dx%d"
                           % (R, S, stride, pad, H, W, OH, OW))
    if dx_add is not None:
        act16._require_act16(dx_add, "dgrad16 (dx_add)")
        if dx_add.dtype != g.dtype or tuple(dx_add.shape) != (N, Cin, H, W):
            raise _lib.FiError("dgrad16: dx_add %s %s does not match dx %s %s"
                               % (dx_add.dtype, tuple(dx_add.shape), g.dtype, (N, Cin, H, W)))
    dx = torch.empty((N, Cin, H, W), device=g.device, dtype=g.dtype, memory_format=torch.channels_last)
    geom = (N, H, W, Cin, Cout, R, S, stride, pad)
    if N > 0:
        _require_eligible(L, "dgrad16", DGRAD, geom, g, wt, dx_add, dx)
    act16._launch(g.device, "fi_grad16_conv_dgrad", _conv._lowp_fn(L, "grad16_conv_dgrad", prec), _lib.ptr(g), _lib.ptr(wt),
                  _lib.ptr(dx_add), _lib.ptr(dx), *geom)
    _STATS["dgrad"] += 1
    return dx


def wgrad16(g, x16, R, S, stride=1, pad=0):
    """dw [Cout, R, S, Cin] fp32 (tap-major: the dw_tap_major operand of fi_bn_fold_grad) from g [N, Cout, OH, OW] and
    x16 [N, Cin, H, W], both 16-bit channels-last.  One kernel launch (and the zero fill when the pixel range is split)."""
    prec = act16._require_act16(g, "wgrad16 (g)")
    act16._require_act16(x16, "wgrad16 (x)")
    L = load()
    N, Cout, OH, OW = g.shape
    _, Cin, H, W = x16.shape
    if x16.dtype != g.dtype or x16.shape[0] != N or (H + 2 * pad - R) // stride + 1 != OH or \
            (W + 2 * pad - S) // stride + 1 != OW:
        raise _lib.FiError("wgrad16: x %s %s and g %s %s are not the two sides of a %dx%d / stride %d / pad %d layer"
                           % (x16.dtype, tuple(x16.shape), g.dtype, tuple(g.shape), R, S, stride, pad))
    dw = torch.empty((Cout, R, S, Cin), device=g.device, dtype=torch.float32)
    geom = (N, H, W, Cin, Cout, R, S, stride, pad)
    if N > 0:
        _require_eligible(L, "wgrad16", WGRAD, geom, g, x16, None, dw)
    else:
        dw.zero_()
    act16._launch(g.device, "fi_grad16_conv_wgrad", _conv._lowp_fn(L, "grad16_conv_wgrad", prec), _lib.ptr(g),
                  _lib.ptr(x16), _lib.ptr(dw), *geom)
    _STATS["wgrad"] += 1
    return dw


@torch.no_grad()
def weight_t16(conv, bn, scale, dtype):
    """The data-gradient operand of `conv` behind the eval-mode `bn`: wt[ci, r', s', co] = W[co, ci, R-1-r', S-1-s'] *
    scale[co] in fp32, rounded ONCE to `dtype`, contiguous [Cin, R, S, Cout].  Kept in conv's registry (step_state) per
    (tensor, version) of the weight and key of the fold; rebuilt when either changes."""
    w = conv.weight
    expect = (dtype, _conv._fold_key(conv, bn))
    wt = _conv._COPIES.lookup(w, step_state.WT16, expect)
    if wt is None:
        wt = (w.detach() * scale.view(-1, 1, 1, 1)).flip(2, 3).permute(1, 2, 3, 0).to(dtype).contiguous()
        _conv._COPIES.publish(w, step_state.WT16, wt, expect)
        _STATS["weights"] += 1
    return wt


def conv_bn_act16(x16, conv, bn, relu=True, residual=None):
    """act(bn(conv(x16)) [+ residual]) on 16-bit channels-last tensors for use with grad mode ON: the forward is the single
    fi_act16_conv_forward launch of act16.conv_bn_act16 (bit-equal output), the backward three launches of
    libfi_grad16.so and fi_bn_fold_grad.  Gradients: x16 and residual 16-bit channels-last, conv.weight fp32 [Cout, Cin,
    R, S] with channels-last strides (a view of the tap-major buffer), bn.weight / bn.bias (and conv.bias) fp32.  Raises
    _lib.FiError for a training-mode BatchNorm or a layer fi_act16_conv_eligible / fi_grad16_eligible refuses.
    This is train16's layer without a hand-off: its output carries a train16.Gate16 that costs nothing unclaimed."""
    from . import train16          # here: train16 imports this module
    return train16._layer16("grad16.conv_bn_act16", _dw_permuted, x16, conv, bn, relu, residual, False, None, None, None)


def _dw_permuted(dwp, R, S):
    return dwp.permute(0, 3, 1, 2)          # channels-last strides for a 1x1 layer too
