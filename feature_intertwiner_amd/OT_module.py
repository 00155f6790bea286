"""Drop-in for lib/OT_module.py of the reference: `OptTrans`, the optimal-transport
(Sinkhorn) intertwiner loss.

Same constructor, same sub-module names (`G_net`, `critic` -> identical state-dict
keys), same forward contract `OptTrans(...)(x, y) -> loss[bs]`.  What differs is the
execution: the reference loops in Python over the batch and the three loss terms and
runs 2L+6 small kernels per Sinkhorn problem (lib/OT_module.py:95-135); here all
3*bs problems of a forward go through ONE launch of the HIP Sinkhorn kernel
(feature_intertwiner_amd/csrc/sinkhorn.hip).

Autograd: with `no_bp_P_L=True` (the reference default, and the model's unless
DEV.OT_NO_BP_P_L says otherwise) the transport plan P is a constant (:129-131), so
d loss / d C = P and the backward is two small batched products with the saved plan.
With `no_bp_P_L=False` the loss is differentiated through the L iterations: ONE launch of
csrc/sinkhorn_bp.hip (libfi_ot.so, include/fi_ot.h) returns the same loss bits and
d loss / d C, which takes the plan's place in the same backward.  The row normalisation
`x / (||x|| + 1e-20)` is done out of place in torch (the reference's in-place `x /= ...`
on the critic's ReLU output, :111-112, raises in modern autograd; forward values are
identical).
"""
import ctypes

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from .conv import Conv1d, Conv2d, ConvTranspose3x3

EPS = 1e-20

OT_LIB_PATH = _lib.sublibrary_path("ot")
_p, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
# name -> (restype, argtypes); mirrors include/fi_ot.h one to one
OT_SIGNATURES = {
    "fi_ot_sinkhorn_backprop_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i]),
    "fi_ot_sinkhorn_backprop": (_i, [_p, _p, _i, _i, _i, _f, _i, _i, _p, _p, _p, ctypes.c_size_t, _p]),
}


def load_ot():
    """Load libfi_ot.so (after libfi_hip.so, which it links against) and attach the signatures."""
    return _lib.load_sublibrary("ot", OT_SIGNATURES)


def _cost_backward(cost_mode, x, y, plan, grad_loss, difference_form=False):
    """(gx, gy) of sum_p grad_loss[p] <plan_p, C_p(x, y)> with `plan` a constant: the transport plan in the detached
    form, d loss / d C (entries of either sign) in the differentiable one.
    difference_form (l2 cost): sum_j w_ij (x_i - y_j) from the differences themselves, one feature column at a time,
    not as x_i sum_j w_ij - sum_j w_ij y_j: with w = plan / |x_i - y_j| the two sums are large where a pair is close and
    cancel (at D = 1, S = 256 the result is off by 1.7e-4 of its largest element; the difference form by 1e-6)."""
    g = grad_loss.view(-1, 1, 1)
    if cost_mode == 1 and difference_form:
        dist = torch.cdist(x, y, compute_mode="donot_use_mm_for_euclid_dist")
        w = torch.where(dist > 0, plan / dist.clamp_min(1e-30), torch.zeros_like(plan))
        gx, gy = torch.empty_like(x), torch.empty_like(y)
        for d in range(x.size(2)):
            wd = w * (x[:, :, d, None] - y[:, None, :, d])
            gx[:, :, d] = wd.sum(2)
            gy[:, :, d] = -wd.sum(1)
        return gx * g, gy * g
    if cost_mode == 2 and x.size(2) == 1:
        # D = 1 (the model's 1-D form): the two plan-vector products as broadcast multiply + row / column sums
        gx = -(plan * y.transpose(1, 2)).sum(2, keepdim=True) * g
        gy = -(plan * x).sum(1).unsqueeze(2) * g
    elif cost_mode == 2:
        gx = -torch.bmm(plan, y) * g
        gy = -torch.bmm(plan.transpose(1, 2), x) * g
    else:
        # d|x_i - y_j| / dx_i = (x_i - y_j) / |x_i - y_j|, and 0 at coincident points (the subgradient
        # torch.norm's backward uses); dividing by a clamped distance instead would weight the
        # (x_i - y_j) = 0 pairs -- every pair of ReLU-dead critic outputs -- by P / 1e-30.  The distances come
        # from the differences, as the kernel computes its cost: cdist's default for more than 25 samples is
        # |x|^2 + |y|^2 - 2 <x, y>, whose cancellation leaves a pair 1e-3 apart with a distance off by tens of percent
        dist = torch.cdist(x, y, compute_mode="donot_use_mm_for_euclid_dist")
        w = torch.where(dist > 0, plan / dist.clamp_min(1e-30), torch.zeros_like(plan))
        gx = (w.sum(2, keepdim=True) * x - torch.bmm(w, y)) * g
        gy = (w.sum(1).unsqueeze(2) * y - torch.bmm(w.transpose(1, 2), x)) * g
    return gx, gy


class _SinkhornLoss(torch.autograd.Function):
    """loss[p] = <P_p, C_p>, P detached.  cost_mode 2: C = 1 - x y^T (rows normalised
    by the caller); cost_mode 1: C_ij = ||x_i - y_j||."""

    @staticmethod
    def forward(ctx, x, y, eps_inv, L, cost_mode):
        _lib.require_cuda(x, y)
        lib = _lib.load()
        x = x.contiguous().float()
        y = y.contiguous().float()
        P, S, D = x.shape
        loss = torch.empty((P,), device=x.device, dtype=torch.float32)
        need_plan = x.requires_grad or y.requires_grad
        plan = torch.empty((P, S, S), device=x.device, dtype=torch.float32) if need_plan else None
        with torch.cuda.device(x.device):
            _lib.check(lib.fi_sinkhorn_forward(_lib.ptr(x), _lib.ptr(y), P, S, D, float(eps_inv), int(L),
                                               int(cost_mode), _lib.ptr(loss), _lib.ptr(plan), None, None,
                                               _lib.current_stream()), "fi_sinkhorn_forward")
        ctx.cost_mode = int(cost_mode)
        if need_plan:
            ctx.save_for_backward(x, y, plan)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        x, y, plan = ctx.saved_tensors
        gx, gy = _cost_backward(ctx.cost_mode, x, y, plan, grad_loss)
        return gx, gy, None, None, None


class _SinkhornLossBackprop(torch.autograd.Function):
    """loss[p] = <P_p, C_p> differentiated through the L iterations (P not detached): fi_ot_sinkhorn_backprop returns the
    loss (the bits of fi_sinkhorn_forward's) and d loss / d C in one launch; the chain from C to x, y is
    _cost_backward's.  Used only when a gradient is needed.  First derivatives only."""

    @staticmethod
    def forward(ctx, x, y, eps_inv, L, cost_mode):
        _lib.require_cuda(x, y)
        lib = load_ot()
        x = x.contiguous().float()
        y = y.contiguous().float()
        P, S, D = x.shape
        # loss, d loss / d C and the workspace from the caching allocator, on the current stream
        loss = torch.empty((P,), device=x.device, dtype=torch.float32)
        dcost = torch.empty((P, S, S), device=x.device, dtype=torch.float32)
        nbytes = lib.fi_ot_sinkhorn_backprop_workspace_bytes(P, S, int(L))
        ws = torch.empty((max(1, nbytes // 4),), device=x.device, dtype=torch.float32)
        with torch.cuda.device(x.device):
            _lib.check(lib.fi_ot_sinkhorn_backprop(_lib.ptr(x), _lib.ptr(y), P, S, D, float(eps_inv), int(L),
                                                   int(cost_mode), _lib.ptr(loss), _lib.ptr(dcost), _lib.ptr(ws),
                                                   ws.numel() * 4, _lib.current_stream()), "fi_ot_sinkhorn_backprop")
        ctx.cost_mode = int(cost_mode)
        ctx.save_for_backward(x, y, dcost)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        x, y, dcost = ctx.saved_tensors
        gx, gy = _cost_backward(ctx.cost_mode, x, y, dcost, grad_loss, difference_form=True)
        return gx, gy, None, None, None


def _sinkhorn_apply(x, y, epsilon_inv, L, cost_mode, detach_plan):
    if not detach_plan and torch.is_grad_enabled() and (x.requires_grad or y.requires_grad):
        return _SinkhornLossBackprop.apply(x, y, epsilon_inv, L, cost_mode)
    return _SinkhornLoss.apply(x, y, epsilon_inv, L, cost_mode)      # no gradient asked for: the forward alone


def sinkhorn_loss(x, y, epsilon_inv=1.0, L=5, C_form="cosine", detach_plan=True):
    """Batched `_sinkhorn_iterate` (lib/OT_module.py:104-135): x, y [P, S, D] -> loss [P].  detach_plan is the
    reference's no_bp_P_L: True (default) treats the plan as a constant in the backward, False differentiates through
    the L iterations (same loss bits; S <= 256; first derivatives only)."""
    if C_form == "cosine":
        xn = x / (torch.norm(x, p=2, dim=2, keepdim=True) + EPS)
        yn = y / (torch.norm(y, p=2, dim=2, keepdim=True) + EPS)
        loss = _sinkhorn_apply(xn, yn, epsilon_inv, L, 2, detach_plan)
    elif C_form == "l2":
        loss = _sinkhorn_apply(x, y, epsilon_inv, L, 1, detach_plan)
    else:
        raise ValueError("unknown C_form %r" % (C_form,))
    if _lib.TAP is not None:
        _lib.TAP("sinkhorn", x=x, y=y, eps_inv=float(epsilon_inv), L=int(L), C_form=C_form, loss=loss,
                 detach_plan=bool(detach_plan))
    return loss


def _generator(ch_x, ch_y, two_dim, upsample):
    """G_net (lib/OT_module.py:24-41): maps the small-object feature towards the big-object one.
    2-D: transposed 3x3 conv (stride 2 when the spatial size has to double) + BN + ReLU; 1-D: Conv1d k3 + ReLU."""
    if not two_dim:
        return nn.Sequential(Conv1d(ch_x, ch_y, kernel_size=3, padding=1, stride=1), nn.ReLU())
    stride, out_pad = (2, 1) if upsample else (1, 0)
    return nn.Sequential(ConvTranspose3x3(ch_x, ch_y, kernel_size=3, padding=1, stride=stride, output_padding=out_pad),
                         nn.BatchNorm2d(ch_y), nn.ReLU())


def _critic(ch_y, two_dim, one_dim_form):
    """critic (lib/OT_module.py:43-65): the embedding whose channels are the OT samples."""
    if two_dim:
        layers = []
        for cin, cout in ((ch_y, int(ch_y / 2)), (int(ch_y / 2), int(ch_y / 4))):
            layers += [Conv2d(cin, cout, kernel_size=3, padding=1, stride=2), nn.BatchNorm2d(cout), nn.ReLU()]
        return nn.Sequential(*layers)
    if one_dim_form == 'conv':
        return nn.Sequential(Conv1d(ch_y, int(ch_y / 4), kernel_size=3, padding=1, stride=1), nn.ReLU())
    if one_dim_form == 'fc':
        return nn.Linear(ch_y, int(ch_y / 8))
    raise ValueError("DEV.OT_ONE_DIM_FORM must be 'conv' or 'fc', got %r" % (one_dim_form,))


class OptTrans(nn.Module):
    def __init__(self, config, ch_x, spatial_x=-1, ch_y=-1, spatial_y=-1,
                 epsilon=1., L=5, remove_bias=False, C_form='cosine', no_bp_P_L=True, skip_critic=False):
        super(OptTrans, self).__init__()
        self.config = config
        self.epsilon = 1. / epsilon   # stored inverted, as the reference (:13)
        self.L, self.remove_bias, self.no_bp_P_L = L, remove_bias, bool(no_bp_P_L)
        self.C_form, self.skip_critic = C_form, skip_critic
        self.two_dim = spatial_x > 1
        ch_y = ch_x if ch_y == -1 else ch_y
        spatial_y = spatial_x if spatial_y == -1 else spatial_y
        self.G_net = _generator(ch_x, ch_y, self.two_dim, upsample=(spatial_x != spatial_y))
        if not skip_critic:
            self.critic = _critic(ch_y, self.two_dim, getattr(getattr(config, "DEV", None), "OT_ONE_DIM_FORM", "conv"))

    def forward(self, x, y):
        """x (small-object feature) [n, ch, 1] or [n, ch, h, w]; y (big-object feature, detached
        by the caller) same layout.  Returns loss [n] (:67-81)."""
        x_upsample = self.G_net(x)
        bs = x_upsample.size(0)
        cx = self._critic_samples(x_upsample)   # [bs, S, D]
        cy = self._critic_samples(y)
        if self.remove_bias:
            return sinkhorn_loss(cx, cy, self.epsilon, self.L, self.C_form, self.no_bp_P_L)
        # the three terms 2*T(x_up, y) - T(x_up, x_up) - T(y, y) as 3*bs problems, one launch
        xs = torch.cat((cx, cx, cy), 0)
        ys = torch.cat((cy, cx, cy), 0)
        t = sinkhorn_loss(xs, ys, self.epsilon, self.L, self.C_form, self.no_bp_P_L)
        return 2 * t[:bs] - t[bs:2 * bs] - t[2 * bs:]

    def _critic_samples(self, v):
        c = self.critic(v)
        return c.reshape(c.size(0), c.size(1), -1)   # bs, channel_num (samples), spatial (features)

    def _basic_compute_loss(self, x, y):
        """T(x, y) of the reference (:83-102): critic on both, one Sinkhorn per sample."""
        return sinkhorn_loss(self._critic_samples(x), self._critic_samples(y), self.epsilon, self.L,
                             self.C_form, self.no_bp_P_L)
