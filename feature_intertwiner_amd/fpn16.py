"""Training the feature pyramid on 16-bit channels-last activation tensors (TRAIN.ACT_SCOPE = 'pyramid' next to a 16-bit
TRAIN.ACT_PRECISION): the backward of the top-down step of libfi_fpn16.so (include/fi_fpn16.h, csrc/fpn16.hip) as a thin
wrapper, the differentiable lateral step `lateral16` and the differentiable bias-only convolution `conv_bias_act16`.

The forwards are the launches of inference (pyr16.lateral16, pyr16.conv_bias_act16: bit-equal outputs).  The backwards
are grad16's weight and data gradient, train16's gated data gradient where the layer claimed its input's Gate16, and ONE
launch of this library per layer for everything between them: the 2 x 2 sum of the finer lateral's gradient, its add to
the layer's own output gradient with one rounding, and the column sums that are the layer's bias gradient.  The top-down
gradients travel from lateral to lateral through conv.GradBox (conv.GATES on) -- autograd never sees them -- and each
lateral gives its data gradient to the next trunk stage's lateral_box directly.

Plain allocations, single process, as train16.  Which calls the kernel takes is decided by fi_fpn16_eligible alone; a call
it refuses is an error -- there is no fallback to another path.
"""
import ctypes

import torch

from . import _lib
from . import act16
from . import conv as _conv
from . import grad16
from . import pyr16
from . import step_state
from . import train16

LIB_PATH = _lib.sublibrary_path("fpn16")
_cp, _ci = ctypes.c_void_p, ctypes.c_int
_TOPDOWN = (_ci, [_cp, _cp, _cp, _cp, _ci, _ci, _ci, _ci, _cp])
# name -> (restype, argtypes); mirrors include/fi_fpn16.h one to one
SIGNATURES = {
    "fi_fpn16_eligible": (_ci, [_ci, _ci, _ci, _ci, _cp, _cp, _cp, _cp]),
    "fi_fpn16_topdown_grad_bf16": _TOPDOWN,
    "fi_fpn16_topdown_grad_f16": _TOPDOWN,
}
SCOPES = ("trunk", "pyramid", "crops", "heads")
_BIAS_ONLY = "bias-only"          # where grad16.weight_t16 keeps the key of a BatchNorm fold (a tuple): no fold, scale 1
_STATS = {"topdown": 0, "sums": 0, "lateral": 0, "conv": 0, "top_to_autograd": 0, "weights": 0}


def load():
    """Load libfi_fpn16.so (after libfi_hip.so, which it links against) and attach the signatures."""
    return _lib.load_sublibrary("fpn16", SIGNATURES)


def stats():
    """Host counters since reset_stats(): 'topdown' launches of fi_fpn16_topdown_grad that wrote a gradient map, 'sums' its
    read-only column-sum launches; 'lateral' / 'conv' the forwards of the two differentiable layers here (pyr16.stats() and
    act16.stats() count their launches too); 'top_to_autograd' lateral backwards that returned the coarser level's gradient
    to autograd instead of leaving it in a GradBox; 'weights' the transposed 16-bit weights built."""
    return dict(_STATS)


def reset_stats():
    _lib.zero_counters(_STATS)


def train_scope(config):
    """config.TRAIN.ACT_SCOPE: 'trunk' (also when absent: the 16-bit tensors of a train step end behind C5), 'pyramid'
    (they run on through the laterals and the smoothing convolutions to p2..p5) or 'crops' (everything 'pyramid' does, and
    the RPN, the make-up layer and RoIAlign read the 16-bit p2..p5 as well: crops16) or 'heads' (everything 'crops' does,
    and the box and mask heads run forward and backward on 16-bit channels-last crops: heads16).  Every scope but 'trunk'
    needs a 16-bit TRAIN.ACT_PRECISION; ValueError otherwise, and for any other value."""
    train = getattr(config, "TRAIN", None)
    scope = getattr(train, "ACT_SCOPE", "trunk")
    prec = getattr(train, "ACT_PRECISION", "fp32")
    if not isinstance(scope, str) or scope not in SCOPES:
        raise ValueError("TRAIN.ACT_SCOPE is 'trunk', 'pyramid', 'crops' or 'heads', got %r (TRAIN.ACT_PRECISION = %r)" % (scope, prec))
    if scope != "trunk" and (not isinstance(prec, str) or prec not in _conv._LOWP):
        raise ValueError("TRAIN.ACT_SCOPE = %r needs TRAIN.ACT_PRECISION = 'bf16' or 'fp16', got %r" % (scope, prec))
    return scope


def topdown_grad16(own, fine, colsum=True, out=None):
    """(g, s): g [N, C, H, W] (16-bit channels-last) = round16(own + the 2 x 2 sums of fine [N, C, 2H, 2W]) -- either operand
    may be None, not both -- and, when `colsum`, s [C] fp32 = the per-channel sums of g (else None).  out: where g is written
    (it may be `own`: in place); a new tensor when None.  With fine None and out = own nothing is stored: the call only
    sums.  One launch.  Raises _lib.FiError for what fi_fpn16_eligible refuses; there is no fallback."""
    if own is None and fine is None:
        raise _lib.FiError("topdown_grad16: own and fine are both None")
    first = own if own is not None else fine
    prec = act16._require_act16(first, "topdown_grad16 (%s)" % ("own" if own is not None else "fine"))
    if own is not None:
        N, C, H, W = own.shape
    else:
        N, C, H, W = fine.shape[0], fine.shape[1], fine.shape[2] // 2, fine.shape[3] // 2
    if fine is not None:
        act16._require_act16(fine, "topdown_grad16 (fine)")
        if fine.dtype != first.dtype or tuple(fine.shape) != (N, C, 2 * H, 2 * W):
            raise _lib.FiError("topdown_grad16: fine %s %s is not the double-resolution map %s %s of the coarse level"
                               % (fine.dtype, tuple(fine.shape), first.dtype, (N, C, 2 * H, 2 * W)))
    if out is None:
        out = torch.empty((N, C, H, W), device=first.device, dtype=first.dtype, memory_format=torch.channels_last)
    else:
        act16._require_act16(out, "topdown_grad16 (out)")
        if out.dtype != first.dtype or tuple(out.shape) != (N, C, H, W):
            raise _lib.FiError("topdown_grad16: out %s %s does not match the coarse level %s %s"
                               % (out.dtype, tuple(out.shape), first.dtype, (N, C, H, W)))
    L = load()
    s = torch.empty(C, device=first.device, dtype=torch.float32) if colsum else None
    if N > 0:
        if H < 1 or W < 1 or L.fi_fpn16_eligible(N, H, W, C, _lib.ptr(own), _lib.ptr(fine), _lib.ptr(out), _lib.ptr(s)) != 1:
            raise _lib.FiError("topdown_grad16: fi_fpn16_eligible refuses this call (N %d, H %d, W %d, C %d); there is no "
                               "fallback" % (N, H, W, C))
    elif s is not None:
        s.zero_()
    if N > 0:
        act16._launch(first.device, "fi_fpn16_topdown_grad", _conv._lowp_fn(L, "fpn16_topdown_grad", prec), _lib.ptr(own),
                      _lib.ptr(fine), _lib.ptr(out), _lib.ptr(s), N, H, W, C)
    read_only = fine is None and own is not None and out.data_ptr() == own.data_ptr()
    _STATS["sums" if read_only else "topdown"] += 1
    return out, s


@torch.no_grad()
def weight_t16(conv, dtype):
    """The data-gradient operand of a convolution with its own bias and no BatchNorm: wt[ci, r', s', co] =
    W[co, ci, R-1-r', S-1-s'] rounded ONCE to `dtype`, contiguous [Cin, R, S, Cout] -- grad16.weight_t16 with scale 1.  Kept
    in conv's registry (step_state) per (tensor, version) of the weight, under a key no BatchNorm fold can have."""
    w = conv.weight
    expect = (dtype, _BIAS_ONLY)
    wt = _conv._COPIES.lookup(w, step_state.WT16, expect)
    if wt is None:
        wt = w.detach().flip(2, 3).permute(1, 2, 3, 0).to(dtype).contiguous()
        _conv._COPIES.publish(w, step_state.WT16, wt, expect)
        _STATS["weights"] += 1
    return wt


def _take(box):
    if box is None:
        return None
    v, box.value = box.value, None
    return v


def _will_take(box):
    """Raise the taker flag of a box this layer's backward will empty (conv.GATES on, a graph being recorded)."""
    if box is not None and _conv.GATES and torch.is_grad_enabled():
        box.taker = True


class _Lateral16Fn(torch.autograd.Function):
    """y = round16((conv1x1(x16) + bias) + top16 at half resolution): fi_pyr16_lateral.  Backward, with dy the gradient
    autograd delivers and `fine` what the next finer lateral left in `top_grad_from`: g = round16(dy + 2x2 sums of fine)
    and s = sum_p g in ONE fi_fpn16_topdown_grad launch (no fine: g = dy and the launch only sums); d bias = s; dW = wgrad16
    of g; dx = dgrad16 of g, to `dx_give_to` when its taker flag is up; d top = g itself, left in `top_grad_to` for the
    coarser layer -- which sums its 2 x 2 cells in ITS launch -- or, without a taker there, the 2 x 2 sums of g rounded once
    more and returned to autograd."""

    @staticmethod
    def forward(ctx, x16, weight, bias, top16, conv, top_grad_to, top_grad_from, dx_give_to):
        y = pyr16.lateral16(x16, conv, top16)              # grad mode is off inside a Function's forward
        ctx.save_for_backward(x16, weight)
        ctx.conv, ctx.top_grad_to, ctx.top_grad_from, ctx.dx_give_to = conv, top_grad_to, top_grad_from, dx_give_to
        return y

    @staticmethod
    def backward(ctx, dy):
        x16, w = ctx.saved_tensors
        need_x, need_w, need_b, need_top = ctx.needs_input_grad[:4]
        dy = dy.contiguous(memory_format=torch.channels_last)
        g, s = _own_plus_fine(dy, _take(ctx.top_grad_from), need_b)
        dw = train16.dw_view16(grad16.wgrad16(g, x16, 1, 1, 1, 0), 1, 1) if need_w else None
        dx = None
        if need_x:
            dx = grad16.dgrad16(g, weight_t16(ctx.conv, x16.dtype), (x16.shape[2], x16.shape[3]), 1, 0)
            if ctx.dx_give_to is not None and ctx.dx_give_to.taker:
                ctx.dx_give_to.value = dx                   # picked up by the first block of the next trunk stage
                dx = None
        dtop = None
        if need_top:
            if ctx.top_grad_to is not None and ctx.top_grad_to.taker:
                ctx.top_grad_to.value = g                   # picked up by the coarser level's lateral (or P5_conv1)
            else:
                dtop = topdown_grad16(None, g, colsum=False)[0]
                _STATS["top_to_autograd"] += 1
        return dx, dw, s, dtop, None, None, None, None


def _own_plus_fine(dy, fine, want_sums):
    """(g, s) of a layer without a ReLU: one fi_fpn16_topdown_grad launch, read-only when nothing is added, none at all
    when there is nothing to add and nothing to sum."""
    if fine is not None:
        return topdown_grad16(dy, fine, colsum=want_sums)
    if want_sums:
        return topdown_grad16(dy, None, colsum=True, out=dy)
    return dy, None


def _require_bias_layer(what, conv):
    if conv.bias is None:
        raise _lib.FiError("%s: the layer must carry its own bias (a bias-only convolution: no BatchNorm behind it)" % what)


def lateral16(x16, conv, top16, top_grad_to=None, top_grad_from=None, dx_give_to=None):
    """pyr16.lateral16 with grad mode ON: the forward is the single fi_pyr16_lateral launch (bit-equal output).
    top_grad_from: a GradBox in which the next FINER lateral leaves its g; this layer raises its taker flag here and adds
    the 2 x 2 sums of that g to its own output gradient in backward.
    top_grad_to: the GradBox of the COARSER layer (the producer of top16): this layer leaves its g there when that box's
    taker flag is up, and returns the 2 x 2 sums of g to autograd otherwise.
    dx_give_to: a GradBox that receives this layer's data gradient instead of autograd when its taker flag is up (the
    lateral_box of the next trunk stage's first block).
    The givers must run first in backward.  Autograd sees to it: top16 is an input of this layer, so the coarser layer's
    backward waits for this one whether or not a gradient is returned.
    Raises _lib.FiError for what the eligibility queries refuse; there is no fallback."""
    act16._require_act16(x16, "fpn16.lateral16")
    act16._require_act16(top16, "fpn16.lateral16 (top)")
    _require_bias_layer("fpn16.lateral16", conv)
    N, Cin, H, W = x16.shape
    Cout = conv.weight.shape[0]
    train16.require_backward16("fpn16.lateral16", (N, H, W, Cin, Cout, 1, 1, 1, 0), relu=False)
    if N > 0:
        if load().fi_fpn16_eligible(N, H, W, Cout, None, None, None, None) != 1:
            raise _lib.FiError("fpn16.lateral16: fi_fpn16_eligible refuses this layer (N %d, H %d, W %d, C %d); there is no "
                               "fallback" % (N, H, W, Cout))
    _will_take(top_grad_from)
    y = _Lateral16Fn.apply(x16, conv.weight, conv.bias, top16, conv, top_grad_to, top_grad_from, dx_give_to)
    _STATS["lateral"] += 1
    return y


class _ConvBiasAct16Fn(torch.autograd.Function):
    """y = act(conv(x16) + bias): fi_act16_conv_forward without a scale.  Backward: g and s = sum_p g from ONE launch --
    fi_fpn16_topdown_grad (with what `top_grad_from` holds; read-only without it), or relu_grad16 behind it for a layer with
    a ReLU; d bias = s; dW = wgrad16 of g; dx = the gated data gradient when this layer claimed its input's Gate16 (the
    producer's column sums are left in the gate), dgrad16 otherwise."""

    @staticmethod
    def forward(ctx, x16, weight, bias, conv, relu, top_grad_from, in_gate):
        y = pyr16.conv_bias_act16(x16, conv, relu=relu)    # grad mode is off inside a Function's forward
        ctx.save_for_backward(x16, weight, y if relu else None)
        ctx.conv, ctx.relu, ctx.top_grad_from, ctx.in_gate = conv, relu, top_grad_from, in_gate
        return y

    @staticmethod
    def backward(ctx, dy):
        x16, w, y = ctx.saved_tensors
        conv = ctx.conv
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        _, _, R, S = w.shape
        stride, pad = conv.stride[0], conv.padding[0]
        dy = dy.contiguous(memory_format=torch.channels_last)
        fine = _take(ctx.top_grad_from)
        if ctx.relu:
            if fine is not None:
                dy = topdown_grad16(dy, fine, colsum=False)[0]
            g, s = grad16.relu_grad16(dy, y, relu=True, colsum=need_b)
        else:
            g, s = _own_plus_fine(dy, fine, need_b)
        dw = train16.dw_view16(grad16.wgrad16(g, x16, R, S, stride, pad), R, S) if need_w else None
        dx = None
        if need_x:
            dx = train16.data_grad16(g, weight_t16(conv, x16.dtype), x16, ctx.in_gate, stride, pad)
        return dx, dw, s, None, None, None, None


def conv_bias_act16(x16, conv, relu=False, gate_dx=False, top_grad_from=None):
    """pyr16.conv_bias_act16 with grad mode ON (P5_conv1, the smoothing convolutions): the forward is the single
    fi_act16_conv_forward launch (bit-equal output).
    top_grad_from: as lateral16's -- the finest lateral above this layer leaves its g there (P5_conv1).
    gate_dx: the caller's promise that this layer sees x16's WHOLE gradient.  If x16 carries a train16.Gate16 and
    conv.GATES is on, the layer claims it: its data gradient is train16.dgrad_gated16 and the producer runs no
    relu_grad16 (c5: P5_conv1 is its only reader).
    Raises _lib.FiError for what the eligibility queries refuse; there is no fallback."""
    act16._require_act16(x16, "fpn16.conv_bias_act16")
    _require_bias_layer("fpn16.conv_bias_act16", conv)
    N, Cin, H, W = x16.shape
    Cout, _, R, S = conv.weight.shape
    in_gate = train16._claim_gate16(x16, gate_dx)
    stride, pad = conv.stride[0], conv.padding[0]
    train16.require_backward16("fpn16.conv_bias_act16", (N, H, W, Cin, Cout, R, S, stride, pad), relu, in_gate)
    if N > 0:
        OH, OW = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
        if OH < 1 or OW < 1 or load().fi_fpn16_eligible(N, OH, OW, Cout, None, None, None, None) != 1:
            raise _lib.FiError("fpn16.conv_bias_act16: fi_fpn16_eligible refuses this layer's output (N %d, H %d, W %d, "
                               "C %d); there is no fallback" % (N, OH, OW, Cout))
    _will_take(top_grad_from)
    y = _ConvBiasAct16Fn.apply(x16, conv.weight, conv.bias, conv, bool(relu), top_grad_from, in_gate)
    _STATS["conv"] += 1
    return y
