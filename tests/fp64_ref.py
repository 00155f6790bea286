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
relative to max|ref| lets it pass.

Further down: the references of the BatchNorm / glue / SGD launches (tests/test_gpu_step_glue_replay.py) and of the loss
and statistics kernels -- the five detector losses, the per-class means, the meta-loss statistics, Sinkhorn
(tests/test_gpu_loss_kernels.py)."""
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


def check_increment(after, before, ref, mag, n, what=""):
    """An ACCUMULATED output: (after - before) against the reference with the bar, widened by the rounding of the
    accumulation, 2^-23 (|before| + |after|) (folded into m as in check_crop_bwd).  Returns the worst |d| / (2^-24 m)."""
    a, b = _f64(after), _f64(before)
    n_t = n if torch.is_tensor(n) else torch.full_like(a, float(n))
    extra = 2.0 * (b.abs() + a.abs()) / (4.0 * torch.sqrt(_f64(n_t)) + 16.0)
    return check_bar(a - b, ref, _f64(mag) + extra, n_t, what)


# ---- BatchNorm / fully connected backward passes ----------------------------------------------------------------------
def bn_act_bwd_ref(dy, y, xhat, gamma, beta, relu, residual=None):
    """fi_bn_act_backward on [N,C,HW] tensors: y = act(gamma[c] * xhat + beta[c] (+ residual)) was the forward's fp32
    output.  Returns g = dy * (y > 0 | 1) (fp64), dshift = sum g, dgamma = sum g * xhat (the TRUE xhat), each with its
    m of the bar over N * HW terms.  The kernel recovers xhat as (y - residual - beta) / gamma from the rounded y, so
    the m of dgamma carries the conditioning term (|y| + |residual| + |beta|) / |gamma| per element; a channel with
    gamma == 0 gets m = inf (the header documents that the kernel writes 0 there)."""
    dy, y, xh = _f64(dy), _f64(y), _f64(xhat)
    g = dy * (y > 0).to(torch.float64) if relu else dy
    ga = _f64(gamma).reshape(1, -1, 1)
    be = _f64(beta).reshape(1, -1, 1)
    r = _f64(residual).abs() if residual is not None else torch.zeros_like(y)
    cond = (y.abs() + r + be.abs()) / ga.abs()            # inf where gamma == 0
    dshift, m_shift = g.sum((0, 2)), g.abs().sum((0, 2))
    dgamma = (g * xh).sum((0, 2))
    m_gamma = (g.abs() * (xh.abs() + cond)).nan_to_num(nan=0.0, posinf=float("inf")).sum((0, 2))
    return g, dshift, m_shift, dgamma, m_gamma


def rows_mask_scale_ref(dy, y, relu):
    """fi_rows_mask_scale on rows [M][N]: g = dy * (y > 0 | 1) (fp64) and colsum = sum over rows of g, with its m."""
    dy = _f64(dy)
    g = dy * (_f64(y) > 0).to(torch.float64) if relu else dy
    return g, g.sum(0), g.abs().sum(0)


def fold_grad_ref(dwp, w, s, scale, mean, var, eps, conv_bias=None):
    """fi_bn_fold_grad in LOGICAL layouts: dwp (the weight gradient of the unscaled g) and w as [Cout][Cin][taps].
    Returns dW = scale * dW', d gamma = inv_std (<W, dW'> + (conv_bias - mean) s), d bias = scale * s (fp64) and the m
    of d gamma and d bias (the bar over K = Cin * taps)."""
    dwp, w, s = _f64(dwp), _f64(w), _f64(s)
    sc, inv = _f64(scale), 1.0 / torch.sqrt(_f64(var) + float(eps))
    cb = _f64(conv_bias) if conv_bias is not None else torch.zeros_like(s)
    Co = dwp.shape[0]
    dot = (dwp.reshape(Co, -1) * w.reshape(Co, -1)).sum(1)
    adot = (dwp.reshape(Co, -1) * w.reshape(Co, -1)).abs().sum(1)
    mu = _f64(mean)
    dgamma = inv * (dot + (cb - mu) * s)
    m_gamma = inv * (adot + (cb - mu).abs() * s.abs())
    return sc.reshape(-1, *([1] * (dwp.dim() - 1))) * dwp, dgamma, m_gamma, sc * s, (sc * s).abs()


def class_row_bwd_ref(d, x, w, cls, num_classes, gated):
    """fi_class_row_conv1x1_backward: d [N,HW], x [N,C,HW], w [K,C], cls [N].  Returns dx (fp64), dweight [K,C] and
    dbias [K] with their m, and the number of terms per class (rows of the class * HW) for the bar."""
    d, x, w = _f64(d), _f64(x), _f64(w)
    cls = cls.long()
    dx = w[cls][:, :, None] * d[:, None, :]
    if gated:
        dx = dx * (x > 0).to(torch.float64)
    v, av = (x * d[:, None, :]).sum(2), (x * d[:, None, :]).abs().sum(2)
    K, C = num_classes, x.shape[1]
    dw = torch.zeros((K, C), dtype=torch.float64, device=x.device).index_add_(0, cls, v)
    mw = torch.zeros_like(dw).index_add_(0, cls, av)
    db = torch.zeros(K, dtype=torch.float64, device=x.device).index_add_(0, cls, d.sum(1))
    mb = torch.zeros_like(db).index_add_(0, cls, d.abs().sum(1))
    rows = torch.zeros(K, dtype=torch.float64, device=x.device).index_add_(0, cls, torch.ones_like(d[:, 0]))
    return dx, dw, mw, db, mb, torch.clamp_min(rows * d.shape[1], 1.0)


def _patch_index(shapes, image, anchor, per_loc, tap_shift=0):
    """For every row and tap: (level, flat index into [B*C... per level]) -- as lists over the levels of (row, tap, h, w,
    image) selections; tap_shift plants an off-by-one tap (for the tests of the bar)."""
    image, anchor = image.long(), anchor.long()
    starts, s = [], 0
    for (B, C, H, W) in shapes:
        starts.append(s)
        s += H * W * per_loc
    out = []
    tap = torch.arange(9, device=image.device)
    dh = (tap + tap_shift) // 3 - 1
    dw = (tap + tap_shift) % 3 - 1
    for l, (B, C, H, W) in enumerate(shapes):
        end = starts[l + 1] if l + 1 < len(starts) else s
        sel = (image >= 0) & (anchor >= starts[l]) & (anchor < end)
        pix = (anchor - starts[l]) // per_loc
        h = (pix // W)[:, None] + dh[None, :]
        w = (pix % W)[:, None] + dw[None, :]
        ok = sel[:, None] & (h >= 0) & (h < H) & (w >= 0) & (w < W)
        out.append((ok, h.clamp(0, H - 1), w.clamp(0, W - 1)))
    return out


def patch_rows_ref(maps, image, anchor, per_loc, tap_shift=0):
    """fi_pyramid_patch_rows_forward: out [rows][9][C] (fp64) = maps[l][image][c][h + tap/3 - 1][w + tap%3 - 1], 0
    outside the map and for padding rows (image < 0)."""
    shapes = [tuple(m.shape) for m in maps]
    C = shapes[0][1]
    out = torch.zeros((image.numel(), 9, C), dtype=torch.float64, device=maps[0].device)
    img = image.long().clamp_min(0)[:, None].expand(-1, 9)
    for m, (ok, h, w) in zip(maps, _patch_index(shapes, image, anchor, per_loc, tap_shift)):
        vals = _f64(m).permute(0, 2, 3, 1)[img, h, w]            # [rows, 9, C]
        out += vals * ok[..., None].to(torch.float64)
    return out


def patch_rows_bwd_ref(d, shapes, image, anchor, per_loc, tap_shift=0):
    """fi_pyramid_patch_rows_backward: the gradients [B,C,H,W] of every level (fp64), their m and the number of
    terms per element (at most 9 per row set)."""
    d = _f64(d)
    img = image.long().clamp_min(0)[:, None].expand(-1, 9)
    gs, ms, ns = [], [], []
    for (B, C, H, W), (ok, h, w) in zip(shapes, _patch_index(shapes, image, anchor, per_loc, tap_shift)):
        flat = ((img * H + h) * W + w)[ok]
        acc = torch.zeros((B * H * W, C), dtype=torch.float64, device=d.device).index_add_(0, flat, d[ok])
        mag = torch.zeros_like(acc).index_add_(0, flat, d[ok].abs())
        cnt = torch.zeros((B * H * W,), dtype=torch.float64, device=d.device).index_add_(
            0, flat, torch.ones_like(flat, dtype=torch.float64))
        gs.append(acc.reshape(B, H, W, C).permute(0, 3, 1, 2))
        ms.append(mag.reshape(B, H, W, C).permute(0, 3, 1, 2))
        ns.append(torch.clamp_min(cnt, 1.0).reshape(B, 1, H, W))
    return gs, ms, ns


# ---- clip + SGD ---------------------------------------------------------------------------------------------------------
def grad_norm_ref(grads):
    """sqrt(sum g^2) over all gradients in fp64, and the total element count (n of the bar)."""
    tot = sum(float((_f64(g) ** 2).sum()) for g in grads)
    return math.sqrt(tot), sum(g.numel() for g in grads)


def clip_coef_ref(norm, max_norm):
    """clip_grad_norm_'s factor min(1, max_norm / (norm + 1e-6))."""
    return min(1.0, float(max_norm) / (float(norm) + 1e-6))


def sgd_ref(p, g, buf, coef, wd, mom, lr):
    """torch.optim.SGD's step (no dampening / nesterov) on a gradient scaled by coef, in fp64: returns (p', buf', g')
    and their m -- the magnitudes the fp32 operations round against (each element goes through at most 5 of them)."""
    p, g = _f64(p), _f64(g)
    gs = g * float(coef)
    u = gs + wd * p if wd else gs
    mu = gs.abs() + (wd * p.abs() if wd else 0.0)
    if buf is not None:
        b = mom * _f64(buf) + u
        mb = mom * _f64(buf).abs() + mu
    else:
        b, mb = u, mu
    return p - lr * b, b, gs, p.abs() + lr * mb, mb, gs.abs()


# ---- the five detector losses (fi_detector_losses) ---------------------------------------------------------------------
def _t64(a, device=None):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=device if device is not None else t.device, dtype=torch.float64)


def _smooth_l1(d):
    a = d.abs()
    return torch.where(a < 1.0, 0.5 * d * d, a - 0.5), torch.where(a < 1.0, d, torch.sign(d))


def _lse_rows(lg):
    mx = lg.max(1, keepdim=True)[0]
    e = torch.exp(lg - mx)
    se = e.sum(1, keepdim=True)
    return (mx + torch.log(se)).squeeze(1), e / se


def detector_losses_ref(rpn_match, rpn_deltas, row_image, row_anchor, row_logits, row_bbox, roi_cls, cls_logits, roi_deltas,
                        roi_bbox, mask_cls, mask_logits, mask_targets):
    """fi_detector_losses in float64 (include/fi_capi.h, csrc/losses.hip; lib/layers.py:808-934 of the reference).
    rpn_match [b,A], rpn_deltas [b,A,4], row_image / row_anchor [Rr] (-1: padding row), row_logits [Rr,2], row_bbox [Rr,4],
    roi_cls [N], cls_logits [N,K], roi_deltas [N,4], roi_bbox [N,K,4], mask_cls [Nm], mask_logits [Nm,2,2,h,w] (the target
    class's channel before the pixel shuffle), mask_targets [Nm,2h,2w].
    Returns (losses [5], factors [5] = d loss / d stored gradient = 1 / count (0 for the switched-off class loss), the five
    UNNORMALISED gradient tensors, counts [4] = rows with match != 0, RPN positives, RoI positives, positive mask rows).
    Padding rows, rows that do not enter a loss, the box rows off the target class and non-positive mask rows have an
    exactly zero gradient; the class-logit gradient is softmax - onehot on every RoI whether or not the loss is on."""
    dev = row_logits.device if torch.is_tensor(row_logits) else None
    T = lambda a: _t64(a, dev)
    I = lambda a: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(device=dev).long()
    match, deltas, rl, rb = T(rpn_match), T(rpn_deltas), T(row_logits), T(row_bbox)
    im, an = I(row_image), I(row_anchor)
    valid = im >= 0
    i0, a0 = im.clamp(min=0), an.clamp(min=0)
    m = torch.where(valid, match[i0, a0], torch.zeros_like(rl[:, 0]))
    on, pos = (m != 0).to(torch.float64), (m == 1).to(torch.float64)
    lse, p = _lse_rows(rl)
    onehot = torch.stack((1.0 - pos, pos), 1)
    n_rpn, n_rpn_pos = on.sum(), pos.sum()
    l_rpn_cls = (on * (lse - (rl * onehot).sum(1))).sum() / n_rpn.clamp(min=1)
    g_row_logits = on[:, None] * (p - onehot)
    tgt = torch.where(valid[:, None], deltas[i0, a0], torch.zeros_like(rb))
    v, g = _smooth_l1(rb - tgt)
    l_rpn_box = (pos[:, None] * v).sum() / (4.0 * n_rpn_pos).clamp(min=1)
    g_row_bbox = pos[:, None] * g

    cl, rd, rbb = T(cls_logits), T(roi_deltas), T(roi_bbox)
    t = I(roi_cls)
    N, K = cl.shape
    lse, p = _lse_rows(cl)
    oh = torch.zeros_like(cl)
    oh[torch.arange(N, device=cl.device), t] = 1.0
    fg = (t > 0).to(torch.float64)
    n_fg = fg.sum()
    has_fg = (n_fg > 0).to(torch.float64)
    l_cls = (lse - (cl * oh).sum(1)).sum() / N * has_fg
    g_cls = p - oh
    v, g = _smooth_l1(rbb[torch.arange(N, device=cl.device), t] - rd)                    # [N,4]: the target class's row
    l_box = (fg[:, None] * v).sum() / (4.0 * n_fg).clamp(min=1)
    g_box = torch.zeros_like(rbb)
    g_box[torch.arange(N, device=cl.device), t] = fg[:, None] * g

    ml, mt = T(mask_logits), T(mask_targets)
    Nm, _, _, h, w = ml.shape
    mpos = (I(mask_cls) > 0).to(torch.float64)
    # the pixel shuffle of the TARGET: logits [a][b][y][x] face target[2y + a][2x + b]  (ab >> 1 = a, ab & 1 = b)
    tu = mt.reshape(Nm, h, 2, w, 2).permute(0, 2, 4, 1, 3)
    pr, q = 1.0 / (1.0 + torch.exp(-ml)), 1.0 / (1.0 + torch.exp(ml))            # sigmoid and 1 - sigmoid
    lp, lq = torch.log(pr).clamp(min=-100.0), torch.log(q).clamp(min=-100.0)      # F.binary_cross_entropy's clamp
    bce = -(tu * lp + (1.0 - tu) * lq)
    n_mask = mpos.sum()
    l_mask = (mpos.view(-1, 1, 1, 1, 1) * bce).sum() / (n_mask * 4 * h * w).clamp(min=1)
    # BCE's backward (p - t) / max((1 - p) p, 1e-12) times the sigmoid's p (1 - p)
    g_mask = mpos.view(-1, 1, 1, 1, 1) * ((pr - tu) / (q * pr).clamp(min=1e-12) * (pr * q))

    one = torch.ones((), dtype=torch.float64, device=rl.device)
    losses = torch.stack((l_rpn_cls, l_rpn_box, l_cls, l_box, l_mask))
    factors = torch.stack((one / n_rpn.clamp(min=1), one / (4.0 * n_rpn_pos).clamp(min=1), has_fg / N,
                           one / (4.0 * n_fg).clamp(min=1), one / (n_mask * 4 * h * w).clamp(min=1)))
    counts = torch.stack((n_rpn, n_rpn_pos, n_fg, n_mask))
    return losses, factors, [g_row_logits, g_row_bbox, g_cls, g_box, g_mask], counts


# ---- per-class means (fi_class_mean_forward / _backward) ----------------------------------------------------------------
def class_mean_ref(features, gt, K):
    """features [N,F], gt [N] -> feat [F,K] (column c = mean of the rows with label c, 0 < c < K; zero when the class has
    no row), cnt [K], and for the bar the per-class sum |x| [F,K] and the row count (= cnt).  Labels outside (0, K)
    -- background, negative, >= K -- contribute nothing."""
    x = _t64(features)
    g = (gt if torch.is_tensor(gt) else torch.from_numpy(np.ascontiguousarray(gt))).to(x.device).long().reshape(-1)
    N, F_ = x.shape
    ok = (g > 0) & (g < K)
    idx = g[ok]
    s = torch.zeros((K, F_), dtype=torch.float64, device=x.device).index_add_(0, idx, x[ok])
    sa = torch.zeros((K, F_), dtype=torch.float64, device=x.device).index_add_(0, idx, x[ok].abs())
    cnt = torch.zeros(K, dtype=torch.float64, device=x.device).index_add_(0, idx, torch.ones_like(idx, dtype=torch.float64))
    feat = torch.where(cnt[:, None] > 0, s / cnt.clamp(min=1)[:, None], torch.zeros_like(s))
    return feat.t().contiguous(), cnt, sa.t().contiguous(), cnt.clone()


def class_mean_bwd_ref(grad_feat, gt, cnt, K):
    """grad_features [N,F] = grad_feat[:, gt[n]] / cnt[gt[n]] for 0 < gt[n] < K (and cnt > 0), exactly 0 otherwise."""
    gf, c = _t64(grad_feat), _t64(cnt).reshape(-1)
    g = (gt if torch.is_tensor(gt) else torch.from_numpy(np.ascontiguousarray(gt))).to(gf.device).long().reshape(-1)
    ok = (g > 0) & (g < K)
    gc = g.clamp(0, K - 1)
    ok = ok & (c[gc] > 0)
    out = gf.t()[gc] / c[gc].clamp(min=1)[:, None]
    return torch.where(ok[:, None], out, torch.zeros_like(out))


# ---- the statistics side of the meta loss (fi_meta_stats_*) ---------------------------------------------------------------
META_EPS = 1e-20


def meta_stats_ref(big_feat, big_cnt, small_feat, small_cnt, buffer, buffer_cnt):
    """fi_meta_stats_forward (= _sums + _from_sums on one rank) in float64.  big_feat / small_feat: LOGICAL [G,S,F,K]
    tensors (any strides), big_cnt / small_cnt [G,S,K] (or [G,S,1,K]), buffer [F,K] and buffer_cnt [K]: the history
    BEFORE the step.  Returns a dict: the merged means b_feat / s_feat [F,K] and counts b_cnt / s_cnt [K]; active (the
    step has small-object statistics: the count-weighted small sums do not add up to 0); the history after the step
    buffer / buffer_cnt (the old one when not active); SMALL / BIG [K-1,F] (foreground classes, transposed); on [K-1];
    and the magnitudes m_b_feat, m_s_feat, m_buffer for the bar (the same formulas on absolute values)."""
    bf, sf = _t64(big_feat), _t64(small_feat)
    G, S, F_, K = bf.shape
    bc, sc = _t64(big_cnt).reshape(G, S, 1, K), _t64(small_cnt).reshape(G, S, 1, K)
    buf, oc = _t64(buffer).reshape(F_, K), _t64(buffer_cnt).reshape(K)

    def merged(f, c):
        s, a, n = (f * c).sum((0, 1)), (f * c).abs().sum((0, 1)), c.sum((0, 1)).reshape(K)
        return s / (n + META_EPS), a / (n + META_EPS), n, s
    b_feat, m_b, b_cnt, _ = merged(bf, bc)
    s_feat, m_s, s_cnt, s_sum = merged(sf, sc)
    active = bool(s_sum.sum() != 0)
    if active:
        nc = oc + b_cnt
        new_buf = (buf * oc + b_feat * b_cnt) / (nc + META_EPS)
        m_buf = (buf.abs() * oc + m_b * b_cnt) / (nc + META_EPS)
    else:
        nc, new_buf, m_buf = oc, buf, buf.abs()
    on = ((s_cnt > 0) & (nc > 0))[1:].to(torch.float64)
    return dict(b_feat=b_feat, s_feat=s_feat, b_cnt=b_cnt, s_cnt=s_cnt, active=active, buffer=new_buf, buffer_cnt=nc,
                SMALL=s_feat[:, 1:].t().contiguous(), BIG=new_buf[:, 1:].t().contiguous(), on=on,
                m_b_feat=m_b, m_s_feat=m_s, m_buffer=m_buf)


def meta_stats_bwd_ref(dsmall, s_cnt, small_cnt):
    """fi_meta_stats_backward: d small_feat [G,S,F,K] = dsmall[k-1][f] / (s_cnt[k] + eps) * small_cnt[g][s][k], 0 for the
    background class k = 0.  dsmall [K-1,F], s_cnt [K] (the merged small counts), small_cnt [G,S,K]."""
    d, c = _t64(dsmall), _t64(s_cnt).reshape(-1)
    K = c.numel()
    sc = _t64(small_cnt)
    G, S = sc.shape[:2]
    sc = sc.reshape(G, S, 1, K)
    per = torch.zeros((d.shape[1], K), dtype=torch.float64, device=d.device)
    per[:, 1:] = d.t() / (c[1:] + META_EPS)
    return per[None, None] * sc


# ---- Sinkhorn (fi_sinkhorn_forward, OT_module.sinkhorn_loss) --------------------------------------------------------------
OT_EPS = 1e-20


def _ot_cost(x, y, mode):
    """mode 0: 1 - <x / (|x| + eps), y / (|y| + eps)>; 1: |x_i - y_j| (zero subgradient at coincident points, as
    torch.norm's); 2: 1 - <x, y> on rows the caller normalised."""
    if mode == 0:
        x = x / (x.norm(dim=1, keepdim=True) + OT_EPS)
        y = y / (y.norm(dim=1, keepdim=True) + OT_EPS)
    if mode == 1:
        ss = ((x[:, None, :] - y[None, :, :]) ** 2).sum(2)
        return torch.where(ss > 0, torch.sqrt(torch.where(ss > 0, ss, torch.ones_like(ss))), torch.zeros_like(ss))
    return 1.0 - x @ y.t()


def _ot_plan(C, eps_inv, L):
    K = torch.exp(-eps_inv * C)
    S = C.shape[0]
    u = torch.full((S, 1), 1.0 / S, dtype=torch.float64, device=C.device)
    a = b = u
    for _ in range(L):
        a = u / (K @ b + OT_EPS)
        b = u / (K.t() @ a + OT_EPS)
    return a * K * b.t()


def sinkhorn_ref(x, y, eps_inv, L, mode):
    """One problem of lib/OT_module.py:104-135 in float64: x, y [S,D]; eps_inv = 1 / epsilon as the C ABI takes it; L
    iterations from a = b = 1/S; returns (loss = <P, C>, plan P [S,S])."""
    C = _ot_cost(_t64(x), _t64(y), mode)
    P = _ot_plan(C, float(eps_inv), int(L))
    return (P * C).sum(), P


def sinkhorn_detached_plan_loss(x, y, eps_inv, L, form):
    """The differentiable loss of OT_module.sinkhorn_loss on float64 tensors x, y [P,S,D] (they may require grad):
    loss[p] = <P_p.detach(), C_p(x, y)>, form 'cosine' (out-of-place normalisation) or 'l2'."""
    mode = {"cosine": 0, "l2": 1}[form]
    out = []
    for p in range(x.shape[0]):
        C = _ot_cost(x[p], y[p], mode)
        out.append((_ot_plan(C, float(eps_inv), int(L)).detach() * C).sum())
    return torch.stack(out)
