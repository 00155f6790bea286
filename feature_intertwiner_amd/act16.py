"""16-bit channels-last activation tensors: the ResNet trunk's conv + eval-BatchNorm (+ shortcut) + ReLU layers reading and
writing bf16 / fp16 [N, H, W, C] tensors (libfi_act16.so, include/fi_act16.h, csrc/conv_act16.hip), and the transposing
casts at the boundary to the fp32 NCHW tensors of the rest of the model.  Inference only (MODEL.ACT_PRECISION).

A 16-bit activation tensor is a [N, C, H, W]-shaped torch.channels_last tensor of dtype bfloat16 / float16: a consumer
sees logical NCHW, the memory is NHWC.  Which layers the kernel takes is decided by fi_act16_conv_eligible alone; nothing
here restates its rules, and a layer it refuses is an error -- there is no fallback to another path.
"""
import ctypes

import torch

from . import _lib
from . import conv as _conv

LIB_PATH = _lib.sublibrary_path("act16")
_cp, _ci = ctypes.c_void_p, ctypes.c_int
_FWD = (_ci, [_cp, _cp, _cp, _cp, _cp, _cp, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _cp])
_CAST = (_ci, [_cp, _cp, _ci, _ci, _ci, _ci, _cp])
# name -> (restype, argtypes); mirrors include/fi_act16.h one to one
SIGNATURES = {
    "fi_act16_conv_eligible": (_ci, [_ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _cp, _cp, _cp, _cp]),
    "fi_act16_conv_forward_bf16": _FWD,
    "fi_act16_conv_forward_f16": _FWD,
    "fi_act16_pack_bf16": _CAST,
    "fi_act16_pack_f16": _CAST,
    "fi_act16_unpack_bf16": _CAST,
    "fi_act16_unpack_f16": _CAST,
}
_PRECISION_OF = {dtype: prec for prec, (_, dtype) in _conv._LOWP.items()}      # torch dtype -> 'bf16' / 'fp16'
_STATS = {"conv": 0, "pack": 0, "unpack": 0}


def load():
    """Load libfi_act16.so (after libfi_hip.so, which it links against) and attach the signatures."""
    return _lib.load_sublibrary("act16", SIGNATURES)


def stats():
    """Host counters of the launches since reset_stats(): {'conv', 'pack', 'unpack'}."""
    return dict(_STATS)


def reset_stats():
    _lib.zero_counters(_STATS)


def dtype_of(precision):
    """torch dtype of MODEL.ACT_PRECISION 'bf16' / 'fp16'."""
    if precision not in _conv._LOWP:
        raise ValueError("a 16-bit activation precision is 'bf16' or 'fp16', got %r" % (precision,))
    return _conv._LOWP[precision][1]


def is_act16(x):
    return x.dtype in _PRECISION_OF


def _require_act16(x, what):
    _lib.require_cuda(x)
    if x.dim() != 4 or x.dtype not in _PRECISION_OF or not x.is_contiguous(memory_format=torch.channels_last):
        raise _lib.FiError("%s: expected a 4-d channels-last bfloat16 / float16 tensor, got %s %s with strides %s"
                           % (what, x.dtype, tuple(x.shape), tuple(x.stride())))
    return _PRECISION_OF[x.dtype]


def _launch(dev, what, fn, *args):
    """fn(*args, stream) with `dev` current (entered only when it is not: the context manager costs more than the call)."""
    if dev.index is None or dev.index == torch.cuda.current_device():
        _lib.check(fn(*args, _lib.current_stream()), what)
    else:
        with torch.cuda.device(dev):
            _lib.check(fn(*args, _lib.current_stream()), what)


def pack(x, dtype):
    """fp32 NCHW [N, C, H, W] -> the 16-bit channels-last tensor (round to nearest even), one launch."""
    _lib.require_cuda(x)
    if dtype not in _PRECISION_OF:
        raise _lib.FiError("act16.pack: dtype must be torch.bfloat16 or torch.float16, got %s" % (dtype,))
    if x.dim() != 4 or x.dtype != torch.float32:
        raise _lib.FiError("act16.pack: expected a 4-d float32 tensor, got %s %s" % (x.dtype, tuple(x.shape)))
    L = load()
    x = x.contiguous()
    N, C, H, W = x.shape
    y = torch.empty((N, C, H, W), device=x.device, dtype=dtype, memory_format=torch.channels_last)
    _launch(x.device, "fi_act16_pack", _conv._lowp_fn(L, "act16_pack", _PRECISION_OF[dtype]), _lib.ptr(x), _lib.ptr(y),
            N, C, H, W)
    _STATS["pack"] += 1
    return y


def unpack(x16):
    """The 16-bit channels-last tensor -> fp32 NCHW (exact widening), one launch."""
    prec = _require_act16(x16, "act16.unpack")
    L = load()
    N, C, H, W = x16.shape
    y = torch.empty((N, C, H, W), device=x16.device, dtype=torch.float32)
    _launch(x16.device, "fi_act16_unpack", _conv._lowp_fn(L, "act16_unpack", prec), _lib.ptr(x16), _lib.ptr(y), N, C, H, W)
    _STATS["unpack"] += 1
    return y


def conv_bn_act16(x16, conv, bn, relu=True, residual=None):
    """act(bn(conv(x16)) [+ residual]) on 16-bit channels-last tensors, one launch; `bn` an eval-mode BatchNorm2d whose
    fold (scale, shift) is the cached one of conv.refresh_bn_folds.  Raises _lib.FiError for a training-mode BatchNorm,
    an enabled grad mode, or a layer fi_act16_conv_eligible refuses."""
    prec = _require_act16(x16, "conv_bn_act16")
    if torch.is_grad_enabled():
        raise _lib.FiError("conv_bn_act16 is forward only: call it under torch.no_grad() (training on 16-bit activation "
                           "tensors is not built)")
    scale, shift = eval_fold("conv_bn_act16", conv, bn)
    return _conv16("conv_bn_act16", x16, prec, conv, scale, shift, relu, residual)


def require_eval_bn(what, bn):
    if bn.training or not bn.track_running_stats:
        raise _lib.FiError("%s folds an eval-mode BatchNorm with running statistics; got one in training mode" % what)


def eval_fold(what, conv, bn):
    """(scale, shift) of the eval-mode `bn` behind `conv`: the cached fold of conv.refresh_bn_folds, refreshed when a
    parameter changed.  Raises _lib.FiError for one in training mode."""
    require_eval_bn(what, bn)
    _conv._FOLD_PAIRS[bn] = conv
    fold = _conv._cached_fold(conv, bn)
    if fold is None:
        _conv.refresh_bn_folds()
        fold = _conv._cached_fold(conv, bn)
    return fold


def weight16(weight, dtype):
    """The tap-major [Cout, R, S, Cin] 16-bit copy of a [Cout, Cin, R, S] weight: a view of a channels-last (or 1x1)
    weight goes through conv's registry; a 3x3 weight still stored [Cout, Cin, R, S] (no prepare_step yet) is converted
    for this call and not registered -- the registry would pin one tap-major temporary per call."""
    wt = weight.permute(0, 2, 3, 1)                 # (no graph: grad mode is off)
    if wt.is_contiguous():
        return _conv._cached_bf16(wt, dtype)
    return wt.to(dtype).contiguous()


def _conv16(what, x16, prec, conv, scale, shift, relu, residual):
    """One fi_act16_conv_forward launch of `conv` on x16 with the fp32 per-channel scale / shift (each may be None)."""
    L = load()
    dtype = x16.dtype
    N, Cin, H, W = x16.shape
    Cout, _, R, S = conv.weight.shape
    stride, pad = conv.stride, conv.padding
    if stride[0] != stride[1] or pad[0] != pad[1] or tuple(conv.dilation) != (1, 1) or conv.groups != 1 or \
            conv.weight.shape[1] != Cin:
        raise _lib.FiError(what + ": the layer must be a dense square-stride convolution of the input's %d channels "
                           "(stride %s, padding %s, dilation %s, groups %d, weight %s)"
                           % (Cin, tuple(stride), tuple(pad), tuple(conv.dilation), conv.groups, tuple(conv.weight.shape)))
    OH = (H + 2 * pad[0] - R) // stride[0] + 1
    OW = (W + 2 * pad[1] - S) // stride[1] + 1
    if residual is not None:
        _require_act16(residual, what + " (residual)")
        if residual.dtype != dtype or tuple(residual.shape) != (N, Cout, OH, OW):
            raise _lib.FiError("%s: residual %s %s does not match the output %s %s"
                               % (what, residual.dtype, tuple(residual.shape), dtype, (N, Cout, OH, OW)))
    w16 = weight16(conv.weight, dtype)
    y = torch.empty((N, Cout, max(OH, 0), max(OW, 0)), device=x16.device, dtype=dtype, memory_format=torch.channels_last)
    args = (N, H, W, Cin, Cout, R, S, stride[0], pad[0])
    if N > 0 and L.fi_act16_conv_eligible(*args, _lib.ptr(x16), _lib.ptr(w16), _lib.ptr(residual), _lib.ptr(y)) != 1:
        raise _lib.FiError("%s: fi_act16_conv_eligible refuses this layer (N %%d, H %%d, W %%d, Cin %%d, Cout %%d, "
                           "R %%d, S %%d, stride %%d, pad %%d); there is no fallback" % what % args)
    _launch(x16.device, "fi_act16_conv_forward", _conv._lowp_fn(L, "act16_conv_forward", prec), _lib.ptr(x16),
            _lib.ptr(w16), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(residual), _lib.ptr(y), *args, 1 if relu else 0)
    _STATS["conv"] += 1
    return y
