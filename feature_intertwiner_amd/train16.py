"""Training the ResNet trunk on 16-bit channels-last activation tensors (TRAIN.ACT_PRECISION): the gated data gradient of
libfi_train16.so (include/fi_train16.h, csrc/conv_train16.hip) as a thin wrapper, `Gate16`, the differentiable layer
`conv_bn_act16` with the gradient hand-offs of the fp32 path (conv.GradBox) and the differentiable boundary casts
`pack` / `unpack`.

The forward of a layer is act16's single fi_act16_conv_forward launch.  Its backward is grad16's operators (relu_grad16,
wgrad16, fi_bn_fold_grad, dgrad16) with two changes: gradients can travel through GradBoxes instead of autograd, and a
consumer that sees the whole gradient of its input runs the GATED data gradient -- one launch that applies the producing
layer's ReLU mask and leaves that layer's column sums on its Gate16, so the producer runs no relu_grad16 at all.

The steps of that backward are written here once -- require_backward16, with_out_gate16, masked_grad16,
fold_weight_grad16, dw_view16, data_grad16 -- and the layers of fpn16 and heads16 call them; grad16.conv_bn_act16 is this
module's layer without a hand-off.

Plain allocations: the gradient arena and the deferred / batched weight-gradient queues of the fp32 path are not wired.
Which layers the kernels take is decided by fi_train16_eligible / fi_grad16_eligible alone; a layer they refuse is an
error -- there is no fallback to another path.
"""
import ctypes

import torch

from . import _lib
from . import act16
from . import conv as _conv
from . import grad16

LIB_PATH = _lib.sublibrary_path("train16")
_cp, _ci = ctypes.c_void_p, ctypes.c_int
_GATED = (_ci, [_cp, _cp, _cp, _cp, _cp, _cp, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _cp])
# name -> (restype, argtypes); mirrors include/fi_train16.h one to one
SIGNATURES = {
    "fi_train16_eligible": (_ci, [_ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _cp, _cp, _cp, _cp]),
    "fi_train16_conv_dgrad_gated_bf16": _GATED,
    "fi_train16_conv_dgrad_gated_f16": _GATED,
}
_STATS = {"gated": 0, "premasked": 0, "fallback": 0, "pack": 0, "unpack": 0}
_PAIR_ADDS = [0]


def load():
    """Load libfi_train16.so (after libfi_hip.so, which it links against) and attach the signatures."""
    return _lib.load_sublibrary("train16", SIGNATURES)


def stats():
    """Host counters since reset_stats(): 'gated' launches of the gated data gradient (they are not grad16 launches and do
    not count there); 'premasked' layer backwards that took their masked gradient and column sums from their Gate16 and
    ran no relu_grad16; 'fallback' layer backwards whose gate WAS claimed but whose incoming gradient was not the tensor
    the claimer wrote, so that they ran relu_grad16 after all; 'pack' / 'unpack' the boundary casts this module launched,
    forward and backward (act16.stats() counts them too)."""
    return dict(_STATS)


def reset_stats():
    _lib.zero_counters(_STATS)
    _PAIR_ADDS[0] = 0


def pair_adds():
    """16-bit adds of two GradBox values that could not be chained (see conv_bn_act16) since reset_stats()."""
    return _PAIR_ADDS[0]


def act_precision(config):
    """config.TRAIN.ACT_PRECISION: 'fp32' (also when absent), 'bf16' or 'fp16'; anything else is a ValueError."""
    p = getattr(getattr(config, "TRAIN", None), "ACT_PRECISION", "fp32")
    if p != "fp32" and p not in _conv._LOWP:
        raise ValueError("TRAIN.ACT_PRECISION must be 'fp32', 'bf16' or 'fp16', got %r" % (p,))
    return p


def check_config(config):
    """What a model is built with: ValueError for a TRAIN.ACT_PRECISION that is none of the three, NotImplementedError
    for a 16-bit one together with TRAIN.FPN_OT_LOSS (the lateral hand-off is not set up on that branch)."""
    p = act_precision(config)
    if p != "fp32" and getattr(config.TRAIN, "FPN_OT_LOSS", False):
        raise NotImplementedError("TRAIN.ACT_PRECISION = %r with TRAIN.FPN_OT_LOSS is not built: the optimal-transport "
                                  "branch of the pyramid has no route for the lateral gradients" % (p,))
    return p


def dgrad_gated16(g, wt, gate, in_hw, stride=1, pad=0, dx_add=None, colsum=True):
    """(dx, s): dx [N, Cin, H, W] (16-bit channels-last) = grad16.dgrad16(g, wt, in_hw, stride, pad, dx_add) masked with
    (gate > 0), bit for bit what relu_grad16 of it would give, and, when `colsum`, s [Cin] fp32 = the per-channel sums of
    dx (else None).  gate: the layer's input [N, Cin, H, W], i.e. the producing layer's post-ReLU output.  One launch.
    Raises _lib.FiError for what fi_train16_eligible refuses; there is no fallback."""
    prec = act16._require_act16(g, "dgrad_gated16 (g)")
    _lib.require_cuda(wt)
    if wt.dim() != 4 or wt.dtype != g.dtype or not wt.is_contiguous() or wt.shape[3] != g.shape[1]:
        raise _lib.FiError("dgrad_gated16: wt must be a contiguous [Cin, R, S, Cout] tensor of g's dtype and %d channels, "
                           "got %s %s" % (g.shape[1], wt.dtype, tuple(wt.shape)))
    L = load()
    N, Cout, OH, OW = g.shape
    Cin, R, S, _ = wt.shape
    H, W = in_hw
    if (H + 2 * pad - R) // stride + 1 != OH or (W + 2 * pad - S) // stride + 1 != OW:
        raise _lib.FiError("dgrad_gated16: a %dx%d / stride %d / pad %d layer on %dx%d does not give g's %dx%d"
                           % (R, S, stride, pad, H, W, OH, OW))
    for name, t in (("gate", gate), ("dx_add", dx_add)):
        if t is None and name == "dx_add":
            continue
        act16._require_act16(t, "dgrad_gated16 (%s)" % name)
        if t.dtype != g.dtype or tuple(t.shape) != (N, Cin, H, W):
            raise _lib.FiError("dgrad_gated16: %s %s %s does not match dx %s %s"
                               % (name, t.dtype, tuple(t.shape), g.dtype, (N, Cin, H, W)))
    dx = torch.empty((N, Cin, H, W), device=g.device, dtype=g.dtype, memory_format=torch.channels_last)
    s = torch.empty(Cin, device=g.device, dtype=torch.float32) if colsum else None
    geom = (N, H, W, Cin, Cout, R, S, stride, pad)
    if N > 0:
        if L.fi_train16_eligible(*geom, _lib.ptr(g), _lib.ptr(gate), _lib.ptr(dx_add), _lib.ptr(dx)) != 1:
            raise _lib.FiError("dgrad_gated16: fi_train16_eligible refuses this layer (N %d, H %d, W %d, Cin %d, Cout %d, "
                               "R %d, S %d, stride %d, pad %d); there is no fallback" % geom)
    elif s is not None:
        s.zero_()
    act16._launch(g.device, "fi_train16_conv_dgrad_gated", _conv._lowp_fn(L, "train16_conv_dgrad_gated", prec), _lib.ptr(g),
                  _lib.ptr(wt), _lib.ptr(dx_add), _lib.ptr(gate), _lib.ptr(dx), _lib.ptr(s), *geom)
    _STATS["gated"] += 1
    return dx, s


class Gate16(object):
    """Travels with the output y of a differentiable 16-bit conv + BN + ReLU layer (attribute `_fi_gate16` of the tensor):
    the analogue of conv.Gate, which cannot carry the sums.  A consumer told it sees y's WHOLE gradient
    (conv_bn_act16(gate_dx=True)) claims it; its backward runs the gated data gradient with gate = y, leaves the column
    sums here and remembers the tensor it wrote.  The producer's backward takes both only when the dy that arrives is
    that very tensor (same storage, shape, strides and version); otherwise it masks and sums itself."""
    __slots__ = ("claimed", "sums", "wrote", "version")

    def __init__(self):
        self.claimed = False
        self.sums = None
        self.wrote = None         # the dx of the gated launch (held: its storage cannot be handed out again meanwhile)
        self.version = -1

    def leave(self, dx, sums):
        self.wrote, self.sums, self.version = dx, sums, dx._version

    def take(self, dy):
        """The sums when dy is the tensor the claimer wrote, else None; the gate is emptied either way."""
        w, s, v = self.wrote, self.sums, self.version
        self.wrote = self.sums = None
        if w is None or s is None or dy.data_ptr() != w.data_ptr() or dy.shape != w.shape or dy.dtype != w.dtype or \
                dy.stride() != w.stride() or dy._version != v:
            return None
        return s


def _claim_gate16(x16, gate_dx):
    if not _conv.GATES or not gate_dx or not (torch.is_grad_enabled() and x16.requires_grad):
        return None
    gate = getattr(x16, "_fi_gate16", None)
    if gate is None:
        return None
    gate.claimed = True
    return gate


def _take_boxes16(boxes):
    """The 16-bit value left in a GradBox, or in a pair of them: one value as it is, two as their sum (one 16-bit add,
    one more rounding; counted by pair_adds()).  Bottleneck never needs the add: it chains the lateral's gradient through
    the projection's dx_add instead.  The boxes are emptied."""
    if boxes is None:
        return None
    if isinstance(boxes, _conv.GradBox):
        boxes = (boxes,)
    vals = []
    for b in boxes:
        v, b.value = b.value, None
        if v is not None:
            vals.append(v)
    if not vals:
        return None
    if len(vals) == 1:
        return vals[0]
    _PAIR_ADDS[0] += len(vals) - 1
    out = vals[0]
    for v in vals[1:]:
        out = out + v
    return out.contiguous(memory_format=torch.channels_last)


# ---- the steps every 16-bit layer backward shares (this module's layer, fpn16's and heads16's) ----------------------------
_KINDS = ((grad16.WGRAD, "wgrad"), (grad16.DGRAD, "dgrad"), (grad16.RELU_GRAD, "relu_grad"))


def require_backward16(what, geom, relu=True, in_gate=None):
    """The eligibility preamble of a layer with geom = (N, H, W, Cin, Cout, R, S, stride, pad): _lib.FiError, prefixed
    `what`, unless fi_grad16_eligible takes its weight and data gradient (and its ReLU mask when `relu`) and, when the
    layer claimed its input's gate, fi_train16_eligible the gated launch.  An empty batch launches nothing: no query."""
    if geom[0] <= 0:
        return
    L = grad16.load()
    for kind, name in (_KINDS if relu else _KINDS[:2]):
        grad16._require_eligible(L, "%s (%s)" % (what, name), kind, geom, None, None, None, None)
    if in_gate is not None and load().fi_train16_eligible(*geom, None, None, None, None) != 1:
        raise _lib.FiError("%s: fi_train16_eligible refuses this layer %s; there is no fallback" % (what, geom))


def with_out_gate16(relu, apply):
    """y = apply(gate) with gate a new Gate16, hung on y as `_fi_gate16`, for a layer with a ReLU while a graph is
    recorded; apply(None) otherwise."""
    gate = Gate16() if (relu and torch.is_grad_enabled()) else None
    y = apply(gate)
    if gate is not None:
        y._fi_gate16 = gate
    return y


def masked_grad16(dy, y, out_gate, relu, want_sums):
    """(g, s) with g = dy * (y > 0) and s = sum_p g: dy itself and the sums on `out_gate` when the gate was claimed and
    its claimer wrote this very dy (counted 'premasked'); else one relu_grad16 launch -- counted 'fallback' when the gate
    WAS claimed: masking a masked gradient again is idempotent and recomputes the sums.  dy as autograd delivers it."""
    dy = dy.contiguous(memory_format=torch.channels_last)
    if out_gate is not None and out_gate.claimed:
        s = out_gate.take(dy)
        if s is not None:
            _STATS["premasked"] += 1
            return dy, s
        _STATS["fallback"] += 1
    return grad16.relu_grad16(dy, y, relu=relu, colsum=want_sums)


def fold_weight_grad16(g, x_rows, w, conv, bn, scale, s, R, S, stride, pad, need_w, need_gamma, need_b):
    """(dW, d gamma, d conv.bias) of a layer behind the folded eval-mode `bn`: dW' = wgrad16 of the UNSCALED g on x_rows
    as an R x S layer, then ONE fi_bn_fold_grad launch: dW = scale * dW' in place, d gamma = inv_std (<W, dW'> +
    (conv_bias - mean) s), d conv_bias = scale * s.  dW is the tap-major buffer [Cout, R, S, Cin]: the caller views it
    (dw_view16).  All None when none of the three is needed."""
    if not (need_w or need_gamma or need_b):
        return None, None, None
    dwp = grad16.wgrad16(g, x_rows, R, S, stride, pad)
    Cout, Cin, taps = w.shape[0], w.shape[1], w.shape[2] * w.shape[3]
    has_bias = conv.bias is not None
    dgamma = torch.zeros(Cout, device=g.device, dtype=torch.float32) if need_gamma else None
    dbias = torch.zeros(Cout, device=g.device, dtype=torch.float32) if (need_b and has_bias) else None
    w_tap_major = taps > 1 and not w.is_contiguous()       # conv._dense(): contiguous or channels-last
    act16._launch(g.device, "fi_bn_fold_grad", _lib.load().fi_bn_fold_grad, _lib.ptr(dwp), _lib.ptr(w), _lib.ptr(s),
                  _lib.ptr(scale), _lib.ptr(bn.running_mean), _lib.ptr(bn.running_var), float(bn.eps),
                  _lib.ptr(conv.bias) if has_bias else None, _lib.ptr(dgamma), _lib.ptr(dbias), Cout, Cin, taps,
                  1, 1 if w_tap_major else 0)
    return dwp, dgamma, dbias


def dw_view16(dwp, R, S):
    """The tap-major weight gradient with the strides of its parameter: [Cout, Cin, 1, 1] contiguous for a 1x1 layer,
    channels-last strides for a 3x3 one (what prepare_step gives the weight; optim.clip_and_step wants gradient and
    parameter to share their strides, and autograd re-lays a gradient that does not)."""
    Cout, _, _, Cin = dwp.shape
    return dwp.view(Cout, Cin, 1, 1) if R * S == 1 else dwp.permute(0, 3, 1, 2)


def data_grad16(g, wt, x16, in_gate, stride, pad, dx_add=None):
    """dx of g on the data-gradient operand wt, like x16: the gated launch, which leaves dx and the producer's column
    sums on `in_gate`, when the layer claimed its input's gate; dgrad16 otherwise."""
    hw = (x16.shape[2], x16.shape[3])
    if in_gate is None:
        return grad16.dgrad16(g, wt, hw, stride, pad, dx_add=dx_add)
    dx, s_in = dgrad_gated16(g, wt, x16, hw, stride, pad, dx_add=dx_add, colsum=True)
    in_gate.leave(dx, s_in)
    return dx


class _ConvBnAct16Fn(torch.autograd.Function):
    """y = act(conv(x16, W) * scale + shift (+ residual)), scale / shift the eval-BatchNorm fold, with the hand-offs of
    conv._ConvBnActFn.  Backward: g and s from masked_grad16; dW, d gamma and d conv.bias from fold_weight_grad16, d beta
    = s; the shortcut gradient g goes to `res_grad_to` or to autograd; dx = data_grad16 of g on the SCALED weight plus
    what `dx_add_from` holds, and goes to `dx_give_to` or to autograd."""

    @staticmethod
    def forward(ctx, x16, weight, bias, gamma, beta, residual, conv, bn, relu, prec, scale, shift, res_grad_to,
                dx_add_from, dx_give_to, in_gate, out_gate, what, dw_view):
        y = act16._conv16(what, x16, prec, conv, scale, shift, relu, residual)
        ctx.save_for_backward(x16, y, weight, scale)
        ctx.conv, ctx.bn, ctx.relu, ctx.has_res = conv, bn, relu, residual is not None
        ctx.res_grad_to, ctx.dx_add_from, ctx.dx_give_to = res_grad_to, dx_add_from, dx_give_to
        ctx.in_gate, ctx.out_gate, ctx.dw_view = in_gate, out_gate, dw_view
        return y

    @staticmethod
    def backward(ctx, dy):
        x16, y, w, scale = ctx.saved_tensors
        conv, bn = ctx.conv, ctx.bn
        need_x, need_w, need_b, need_gamma, need_beta, need_res = ctx.needs_input_grad[:6]
        R, S = w.shape[2], w.shape[3]
        stride, pad = conv.stride[0], conv.padding[0]
        g, s = masked_grad16(dy, y, ctx.out_gate, ctx.relu, need_w or need_b or need_gamma or need_beta)
        dwp, dgamma, dbias = fold_weight_grad16(g, x16, w, conv, bn, scale, s, R, S, stride, pad, need_w, need_gamma, need_b)
        dw = ctx.dw_view(dwp, R, S) if need_w else None
        g_res = g if (ctx.has_res and need_res) else None
        if g_res is not None and ctx.res_grad_to is not None:
            ctx.res_grad_to.value = g_res           # picked up by the block's first convolution
            g_res = None
        add = _take_boxes16(ctx.dx_add_from)
        dx = None
        if need_x:
            dx = data_grad16(g, grad16.weight_t16(conv, bn, scale, x16.dtype), x16, ctx.in_gate, stride, pad, dx_add=add)
            if ctx.dx_give_to is not None:
                ctx.dx_give_to.value = dx           # picked up (and added) by the backward of the block's first conv
                dx = None
        return (dx, dw, dbias, dgamma, s if need_beta else None, g_res) + (None,) * 13


def conv_bn_act16(x16, conv, bn, relu=True, residual=None, gate_dx=False, dx_add_from=None, res_grad_to=None,
                  dx_give_to=None):
    """act(bn(conv(x16)) [+ residual]) on 16-bit channels-last tensors with grad mode ON: the forward is the single
    fi_act16_conv_forward launch of act16.conv_bn_act16 (bit-equal output).
    gate_dx: the caller's promise that this layer sees x16's WHOLE gradient (nothing else reads x16, or every other
    gradient into it reaches this layer through dx_add_from).  If x16 carries a Gate16 and conv.GATES is on, the layer
    claims it: its data gradient is the gated launch and the producer skips relu_grad16.
    res_grad_to: a GradBox that receives the shortcut's gradient g instead of autograd.
    dx_give_to: a GradBox that receives this layer's dx instead of autograd.
    dx_add_from: a GradBox, or a pair of them, whose 16-bit value is added in the data gradient's epilogue (dx_add).  Two
    values in a pair cost one 16-bit add (pair_adds()); chain the first through its giver's own dx_add_from instead,
    as Bottleneck does -- that costs one more 16-bit rounding of the chained value and no pass.
    The givers must run first in backward: apply them AFTER the taker in forward (conv.GradBox).
    Raises _lib.FiError for a CPU tensor, a training-mode BatchNorm or a layer the eligibility queries refuse."""
    return _layer16("train16.conv_bn_act16", dw_view16, x16, conv, bn, relu, residual, gate_dx, dx_add_from, res_grad_to,
                    dx_give_to)


def _layer16(what, dw_view, x16, conv, bn, relu, residual, gate_dx, dx_add_from, res_grad_to, dx_give_to):
    """conv_bn_act16 under the caller's name `what`, the weight gradient viewed by dw_view(dwp, R, S): the one
    differentiable conv + eval-BatchNorm + ReLU layer (grad16.conv_bn_act16 is this without a hand-off)."""
    act16.require_eval_bn(what, bn)               # the order of the refusals: the BatchNorm, the tensor, then the lookup
    prec = act16._require_act16(x16, what)
    fold = act16.eval_fold(what, conv, bn)
    N, Cin, H, W = x16.shape
    Cout, _, R, S = conv.weight.shape
    in_gate = _claim_gate16(x16, gate_dx)
    require_backward16(what, (N, H, W, Cin, Cout, R, S, conv.stride[0], conv.padding[0]), True, in_gate)
    return with_out_gate16(relu, lambda out_gate: _ConvBnAct16Fn.apply(
        x16, conv.weight, conv.bias, bn.weight, bn.bias, residual, conv, bn, bool(relu), prec, fold[0], fold[1],
        res_grad_to, dx_add_from, dx_give_to, in_gate, out_gate, what, dw_view))


class _PackFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dtype):
        _STATS["pack"] += 1
        return act16.pack(x, dtype)

    @staticmethod
    def backward(ctx, d16):
        _STATS["unpack"] += 1
        return act16.unpack(d16.contiguous(memory_format=torch.channels_last)), None


class _UnpackFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x16, grad_box):
        ctx.grad_box, ctx.dtype = grad_box, x16.dtype
        _STATS["unpack"] += 1
        return act16.unpack(x16)

    @staticmethod
    def backward(ctx, d):
        _STATS["pack"] += 1
        d16 = act16.pack(d.float(), ctx.dtype)
        if ctx.grad_box is not None and ctx.grad_box.taker:
            ctx.grad_box.value = d16               # picked up by the first convolution of the next stage's first block
            return None, None
        return d16, None


def pack(x, dtype):
    """act16.pack (fp32 NCHW -> 16-bit channels-last, one launch), differentiable: the backward is act16.unpack of the
    16-bit gradient."""
    return _PackFn.apply(x, dtype)


def unpack(x16, grad_box=None):
    """act16.unpack (16-bit channels-last -> fp32 NCHW, one launch), differentiable: the backward is act16.pack of the fp32
    NCHW gradient (one rounding), given to `grad_box` when one is set and its taker flag is up, else to autograd."""
    return _UnpackFn.apply(x16, grad_box)
