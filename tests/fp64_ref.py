"""Float64 references of the convolution / GEMM / RoIAlign-backward launches and the elementwise bar they are
checked with (tests/test_fp64_ref_cpu.py pins both on the CPU; tests/test_gpu_step_replay.py and the crop tests use
them on the device).

Every reference is written as a sum over the R x S taps of shifted matrix products (no convolution library), in
float64, on whatever device its tensors live on.  Weights are passed in their LOGICAL form [Cout, Cin, R, S]; the
callers convert the storage layouts of include/fi_capi.h (0: [Cout,Cin,R,S], 1: [Cout,R,S,Cin], 2: as 1 with the taps
applied in reverse order, 3: fragment-major 1x1).

The bar.  For an element i that sums n_i products, an fp32 kernel that accumulates in any order is within
    |got_i - ref_i| <= 2^-24 * (4 * sqrt(n_i) + 16) * m_i
of the exact value, where m_i is the same reference evaluated on absolute values (|x|, |w|, |scale|, |bias|,
|residual|; |G| for a crop).  It bounds each element by its OWN magnitude, so a wrong small element fails it -- a bar
relative to max|ref| lets it pass."""
import math

import numpy as np
import torch

U = 2.0 ** -24


def _f64(t):
    return t.to(torch.float64)


def _padded(x, stride, pad, R, S, OH, OW):
    """x [N,C,H,W] zero-padded so that every window of an OH x OW output (taps outside the input read zeros, also past
    the far border when out_hw overrides the size) lies inside."""
    N, C, H, W = x.shape
    need_h = (OH - 1) * stride[0] + R
    need_w = (OW - 1) * stride[1] + S
    bot = max(0, need_h - H - pad[0])
    right = max(0, need_w - W - pad[1])
    return torch.nn.functional.pad(x, (pad[1], right, pad[0], bot))


def _tap(xp, r, s, stride, OH, OW):
    return xp[:, :, r:r + (OH - 1) * stride[0] + 1:stride[0], s:s + (OW - 1) * stride[1] + 1:stride[1]]


def out_size(H, W, R, S, stride, pad):
    return (H + 2 * pad[0] - R) // stride[0] + 1, (W + 2 * pad[1] - S) // stride[1] + 1


def conv_ref(x, w, stride=(1, 1), pad=(0, 0), out_hw=None, tap_reversed=False, channels_last=False):
    """y [N,Cout,OH,OW] (float64) = sum over taps (r,s) of w[:, :, r, s] . x_pad[:, :, r + stride*oh, s + stride*ow];
    w [Cout,Cin,R,S].  tap_reversed: tap (r,s) uses w[..., R-1-r, S-1-s] (weight layout 2).  out_hw overrides the output
    size.  channels_last: the result is returned [N,OH,OW,Cout]."""
    x, w = _f64(x), _f64(w)
    N, Cin, H, W = x.shape
    Cout, Cin2, R, S = w.shape
    assert Cin == Cin2, (x.shape, w.shape)
    stride, pad = tuple(stride), tuple(pad)
    OH, OW = out_hw if out_hw is not None else out_size(H, W, R, S, stride, pad)
    xp = _padded(x, stride, pad, R, S, OH, OW)
    y = torch.zeros((N, OH, OW, Cout), dtype=torch.float64, device=x.device)
    for r in range(R):
        for s in range(S):
            wk = w[:, :, R - 1 - r, S - 1 - s] if tap_reversed else w[:, :, r, s]
            xs = _tap(xp, r, s, stride, OH, OW).permute(0, 2, 3, 1)
            y += torch.matmul(xs, wk.t())
    return y if channels_last else y.permute(0, 3, 1, 2).contiguous()


def dgrad_ref(dy, w, stride=(1, 1), pad=(0, 0), in_hw=None):
    """dx [N,Cin,H,W] (float64) of y = conv(x, w, stride, pad): every tap scatters dy . w[:, :, r, s] back to the input
    positions it read."""
    dy, w = _f64(dy), _f64(w)
    N, Cout, OH, OW = dy.shape
    _, Cin, R, S = w.shape
    stride, pad = tuple(stride), tuple(pad)
    H, W = in_hw
    PH = max((OH - 1) * stride[0] + R, H + pad[0])
    PW = max((OW - 1) * stride[1] + S, W + pad[1])
    dxp = torch.zeros((N, PH, PW, Cin), dtype=torch.float64, device=dy.device)
    g = dy.permute(0, 2, 3, 1)
    for r in range(R):
        for s in range(S):
            dxp[:, r:r + (OH - 1) * stride[0] + 1:stride[0], s:s + (OW - 1) * stride[1] + 1:stride[1], :] += \
                torch.matmul(g, w[:, :, r, s])
    return dxp[:, pad[0]:pad[0] + H, pad[1]:pad[1] + W, :].permute(0, 3, 1, 2).contiguous()


def wgrad_ref(x, dy, R, S, stride=(1, 1), pad=(0, 0)):
    """dw [Cout,Cin,R,S] (float64) = sum over images and output pixels of dy (x) the window of x at tap (r,s)."""
    x, dy = _f64(x), _f64(dy)
    N, Cout, OH, OW = dy.shape
    Cin = x.shape[1]
    stride, pad = tuple(stride), tuple(pad)
    xp = _padded(x, stride, pad, R, S, OH, OW)
    g = dy.permute(1, 0, 2, 3).reshape(Cout, -1)
    dw = torch.zeros((Cout, Cin, R, S), dtype=torch.float64, device=x.device)
    for r in range(R):
        for s in range(S):
            xs = _tap(xp, r, s, stride, OH, OW).permute(1, 0, 2, 3).reshape(Cin, -1)
            dw[:, :, r, s] = torch.matmul(g, xs.t())
    return dw


def linear_ref(a, b):
    """a [M,K] . b [N,K]^T in float64."""
    return torch.matmul(_f64(a), _f64(b).t())


def epilogue(acc, scale=None, bias=None, residual=None, relu=False, gate=None, channel_dim=1):
    """acc * scale[c] + bias[c] (+ residual), then ReLU, then * (gate > 0) -- the epilogue of fi_conv2d_forward(_gated)
    and fi_gemm_nt_affine; per-channel vectors broadcast along `channel_dim`."""
    shape = [1] * acc.dim()
    shape[channel_dim] = -1
    y = acc
    if scale is not None:
        y = y * _f64(scale).reshape(shape)
    if bias is not None:
        y = y + _f64(bias).reshape(shape)
    if residual is not None:
        y = y + _f64(residual)
    if relu:
        y = torch.clamp_min(y, 0.0)
    if gate is not None:
        y = y * (gate > 0).to(torch.float64)
    return y


def abs_epilogue(acc_abs, scale=None, bias=None, residual=None, channel_dim=1):
    """m_i of the bar for the epilogue above: the magnitude the fp32 sum rounds against."""
    shape = [1] * acc_abs.dim()
    shape[channel_dim] = -1
    m = acc_abs
    if scale is not None:
        m = m * _f64(scale).abs().reshape(shape)
    if bias is not None:
        m = m + _f64(bias).abs().reshape(shape)
    if residual is not None:
        m = m + _f64(residual).abs()
    return m


def bar_ratio(got, ref, mag, n):
    """Per-element |got - ref| / (2^-24 * (4 sqrt(n) + 16) * m).  n: a number or a tensor broadcastable to ref.
    Returns (worst ratio of |d| / (2^-24 m) -- the number the tests print --, worst ratio to the bar, index of that
    element).  A non-finite result counts as infinitely far."""
    got, ref, mag = _f64(got), _f64(ref), _f64(mag)
    d = (got - ref).abs()
    if torch.is_tensor(n):
        n = n.to(torch.float64)
        allow = U * (4.0 * torch.sqrt(n) + 16.0) * mag
    else:
        allow = U * (4.0 * math.sqrt(n) + 16.0) * mag
    bad = ~torch.isfinite(got)
    d = torch.where(bad, torch.full_like(d, float("inf")), d)
    tiny = torch.finfo(torch.float64).tiny
    to_bar = torch.where(d == 0, torch.zeros_like(d), d / torch.clamp_min(allow, tiny))
    in_u = torch.where(d == 0, torch.zeros_like(d), d / torch.clamp_min(U * mag, tiny))
    if to_bar.numel() == 0:
        return 0.0, 0.0, None
    k = int(torch.argmax(to_bar.reshape(-1)))
    return float(in_u.max()), float(to_bar.reshape(-1)[k]), np.unravel_index(k, tuple(to_bar.shape))


def check_bar(got, ref, mag, n, what=""):
    """Asserts the bar for every element; returns the worst |d| / (2^-24 m)."""
    worst_u, worst, idx = bar_ratio(got, ref, mag, n)
    if worst > 1.0:
        raise AssertionError("%s: element %s off the fp32 bar by %.3gx (got %r, ref %r, m %r)" % (
            what, idx, worst, float(_f64(got)[idx]), float(ref[idx]), float(mag[idx])))
    return worst_u


# ---- RoIAlign backward ------------------------------------------------------------------------------------------------
def crop_bwd_ref(grads, boxes, box_ind, level, map_shapes, crop, chunk=256):
    """Float64 gradients of the pyramid maps ([B,C,H,W] each, level l + 2 <-> map_shapes[l]) of a crop-and-resize whose
    output gradient is grads [N,C,crop,crop]: the bins' taps from the oracle's own bin assignment (oracle.crop_taps,
    the reference's C), weights (1-fy)(1-fx), (1-fy) fx, fy (1-fx), fy fx, added with index_add_ on the device of
    `grads`.  Rows with an out-of-pyramid level or an image index outside [0, B) contribute nothing.
    Returns (gradients, magnitudes m (the same on |G|), tap counts n) -- three lists over the levels."""
    from oracle import oracle as O
    dev = grads.device
    boxes_np = np.asarray(boxes.cpu().numpy() if torch.is_tensor(boxes) else boxes, np.float32)
    ind_np = np.asarray(box_ind.cpu().numpy() if torch.is_tensor(box_ind) else box_ind).astype(np.int64)
    lvl_np = np.asarray(level.cpu().numpy() if torch.is_tensor(level) else level).astype(np.int64)
    G = _f64(grads)
    outs, mags, cnts = [], [], []
    for li, shp in enumerate(map_shapes):
        B, C, H, W = shp
        acc = torch.zeros((B * H * W, C), dtype=torch.float64, device=dev)
        mag = torch.zeros_like(acc)
        cnt = torch.zeros((B * H * W,), dtype=torch.float64, device=dev)
        sel = np.nonzero((lvl_np == li + 2) & (ind_np >= 0) & (ind_np < B))[0]
        for c0 in range(0, len(sel), chunk):
            s = sel[c0:c0 + chunk]
            t = O.crop_taps(boxes_np[s], H, W, crop, crop)
            tt = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in t.items()}
            fy = tt["y_frac"].to(torch.float64)[:, :, None]              # [n, crop, 1]
            fx = tt["x_frac"].to(torch.float64)[:, None, :]              # [n, 1, crop]
            valid = ((tt["y_valid"] != 0)[:, :, None] & (tt["x_valid"] != 0)[:, None, :]).to(torch.float64)
            wts = torch.stack([(1 - fy) * (1 - fx), (1 - fy) * fx, fy * (1 - fx), fy * fx], -1) * valid[..., None]
            img = torch.from_numpy(ind_np[s]).to(dev)[:, None, None]
            y0, y1 = tt["y0"].long()[:, :, None], tt["y1"].long()[:, :, None]
            x0, x1 = tt["x0"].long()[:, None, :], tt["x1"].long()[:, None, :]
            # invalid taps may carry out-of-range indices: clamp them (their weight is zero)
            y0, y1 = y0.clamp(0, H - 1), y1.clamp(0, H - 1)
            x0, x1 = x0.clamp(0, W - 1), x1.clamp(0, W - 1)
            idx = torch.stack([(img * H + y0) * W + x0, (img * H + y0) * W + x1,
                               (img * H + y1) * W + x0, (img * H + y1) * W + x1], -1)     # [n, crop, crop, 4]
            g = G[torch.from_numpy(s).to(dev)].permute(0, 2, 3, 1)                       # [n, crop, crop, C]
            contrib = (g[:, :, :, None, :] * wts[..., None]).reshape(-1, C)
            acc.index_add_(0, idx.reshape(-1), contrib)
            mag.index_add_(0, idx.reshape(-1), contrib.abs())
            cnt.index_add_(0, idx.reshape(-1), (wts != 0).to(torch.float64).reshape(-1) *
                           valid[..., None].expand_as(wts).reshape(-1))
            del contrib, g
        outs.append(acc.reshape(B, H, W, C).permute(0, 3, 1, 2))
        mags.append(mag.reshape(B, H, W, C).permute(0, 3, 1, 2))
        cnts.append(cnt.reshape(B, 1, H, W))
    return outs, mags, cnts


def check_crop_bwd(got_levels, grads, boxes, box_ind, level, crop, before=None, what=""):
    """Checks every level's gradient (got_levels: tensors [B,C,H,W] in any memory format) against crop_bwd_ref with the
    bar; `before` (the buffers' contents before an accumulating launch) widens it by 2^-23 (|before_i| + |after_i|) and
    the increment is what is compared.  Returns the worst |d| / (2^-24 m)."""
    shapes = [tuple(t.shape) for t in got_levels]
    refs, mags, cnts = crop_bwd_ref(grads, boxes, box_ind, level, shapes, crop)
    worst = 0.0
    for li, (got, ref, mag, n) in enumerate(zip(got_levels, refs, mags, cnts)):
        got = _f64(got.to(ref.device))
        if before is not None:
            b = _f64(before[li].to(ref.device))
            inc = got - b
            # 2^-23 (|before| + |after|) on top of the bar: folded into m as 2 (|before| + |after|) / (4 sqrt(n) + 16)
            extra = 2.0 * (b.abs() + got.abs()) / (4.0 * torch.sqrt(n) + 16.0)
            worst = max(worst, check_bar(inc, ref, mag + extra, n, "%s level %d" % (what, li + 2)))
        else:
            worst = max(worst, check_bar(got, ref, mag, n, "%s level %d" % (what, li + 2)))
    return worst
