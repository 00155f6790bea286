"""CPU: the float64 references of tests/fp64_ref.py against torch's own float64 convolutions / autograd and the
reference's C RoIAlign backward, and the elementwise fp32 bar checked both ways -- a legitimate fp32 result (torch's CPU
float32 convolution, oneDNN off so that no Winograd-style algorithm sets the error) passes it, and the kernel mistakes
it exists to catch (a missing K-slice of one output block, a dropped pixel split of a weight gradient, a row shifted by
one column at a tile edge, a crop cell missing one box) fail it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fp64_ref as R
from helpers import adversarial_boxes

D = torch.float64


def _close(a, b, rel=1e-12):
    scale = float(b.abs().max()) + 1e-300
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= rel * scale, float((a - b).abs().max()) / scale


CASES = [  # N, Cin, H, W, Cout, R, S, stride, pad
    (2, 5, 9, 11, 7, 3, 3, (1, 1), (1, 1)),
    (1, 4, 10, 13, 6, 3, 3, (2, 2), (1, 1)),
    (2, 3, 15, 15, 4, 7, 7, (2, 2), (3, 3)),
    (1, 6, 7, 9, 5, 1, 1, (1, 1), (0, 0)),
    (1, 6, 9, 8, 5, 1, 1, (2, 2), (0, 0)),
    (1, 3, 8, 7, 2, 2, 3, (1, 2), (0, 1)),
]


@pytest.mark.parametrize("case", CASES)
def test_conv_dgrad_wgrad_refs_equal_torch_float64(case):
    N, Cin, H, W, Cout, Rr, Ss, stride, pad = case
    g = torch.Generator().manual_seed(sum(case[:7]))
    x = torch.randn(N, Cin, H, W, generator=g, dtype=D, requires_grad=True)
    w = torch.randn(Cout, Cin, Rr, Ss, generator=g, dtype=D, requires_grad=True)
    y = F.conv2d(x, w, stride=stride, padding=pad)
    _close(R.conv_ref(x.detach(), w.detach(), stride, pad), y.detach())
    _close(R.conv_ref(x.detach(), w.detach(), stride, pad, channels_last=True), y.detach().permute(0, 2, 3, 1))
    # weight layout 2: tap (r,s) reads w[R-1-r][S-1-s]
    _close(R.conv_ref(x.detach(), w.detach().flip(2, 3), stride, pad, tap_reversed=True), y.detach())
    dy = torch.randn(y.shape, generator=g, dtype=D)
    dx, dw = torch.autograd.grad(y, (x, w), dy)
    _close(R.dgrad_ref(dy, w.detach(), stride, pad, (H, W)), dx)
    _close(R.wgrad_ref(x.detach(), dy, Rr, Ss, stride, pad), dw)
    # the data gradient is also conv_transpose2d
    oph, opw = H - ((y.shape[2] - 1) * stride[0] - 2 * pad[0] + Rr), W - ((y.shape[3] - 1) * stride[1] - 2 * pad[1] + Ss)
    if oph < stride[0] and opw < stride[1]:
        _close(R.dgrad_ref(dy, w.detach(), stride, pad, (H, W)),
               F.conv_transpose2d(dy, w.detach(), stride=stride, padding=pad, output_padding=(oph, opw)))


def test_stride1_data_gradient_is_a_tap_reversed_forward():
    """The fp32 path's data gradient: the forward on dy with W^T stored [Cin,R,S,Cout], taps reversed, padding R-1-pad."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 5, 9, 10, generator=g, dtype=D, requires_grad=True)
    w = torch.randn(6, 5, 3, 3, generator=g, dtype=D)
    y = F.conv2d(x, w, padding=1)
    dy = torch.randn(y.shape, generator=g, dtype=D)
    (dx,) = torch.autograd.grad(y, (x,), dy)
    wt = w.permute(1, 0, 2, 3)                              # logical [Cin,Cout,R,S] of the stored W^T
    _close(R.conv_ref(dy, wt, (1, 1), (1, 1), tap_reversed=True), dx)


def test_out_hw_override_reads_zeros_outside():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(1, 3, 6, 7, generator=g, dtype=D)
    w = torch.randn(4, 3, 3, 3, generator=g, dtype=D)
    big = F.conv2d(F.pad(x, (1, 6, 1, 5)), w)                # zeros far past the border
    got = R.conv_ref(x, w, (1, 1), (1, 1), out_hw=(9, 10))
    _close(got, big[:, :, :9, :10])
    got = R.conv_ref(x, w, (2, 2), (1, 1), out_hw=(5, 5))
    _close(got, F.conv2d(F.pad(x, (1, 6, 1, 6)), w, stride=2)[:, :, :5, :5])
    # and smaller than the natural size
    _close(R.conv_ref(x, w, (1, 1), (1, 1), out_hw=(4, 3)), F.conv2d(x, w, padding=1)[:, :, :4, :3])


def test_linear_and_epilogue():
    g = torch.Generator().manual_seed(5)
    a = torch.randn(37, 20, generator=g, dtype=D)
    b = torch.randn(16, 20, generator=g, dtype=D)
    _close(R.linear_ref(a, b), F.linear(a, b))
    acc = torch.randn(2, 16, 3, 3, generator=g, dtype=D)
    sc, bi = torch.randn(16, generator=g, dtype=D), torch.randn(16, generator=g, dtype=D)
    res, gate = torch.randn(acc.shape, generator=g, dtype=D), torch.randn(acc.shape, generator=g, dtype=D)
    gate[0, 0, 0, 0] = 0.0
    exp = torch.relu(acc * sc[None, :, None, None] + bi[None, :, None, None] + res) * (gate > 0)
    _close(R.epilogue(acc, sc, bi, res, True, gate), exp)
    assert R.epilogue(acc, sc, bi, res, True, gate)[0, 0, 0, 0] == 0
    _close(R.epilogue(R.linear_ref(a, b), sc, bi, relu=True), torch.relu(F.linear(a, b) * sc + bi))


def test_crop_bwd_ref_equals_oracle(oracle):
    rs = np.random.RandomState(21)
    B, C = 2, 5
    shapes = [(B, C, s, s) for s in (40, 20, 10, 5)]
    N = 160
    boxes = adversarial_boxes(rs, N, 40, 40)
    ind = rs.randint(0, B, N).astype(np.int32)
    ind[3] = B + 1
    level = rs.randint(1, 7, N).astype(np.int32)
    for crop in (7, 14):
        G = rs.standard_normal((N, C, crop, crop)).astype(np.float32)
        refs, mags, cnts = R.crop_bwd_ref(torch.from_numpy(G), boxes, ind, level, shapes, crop)
        good = (ind >= 0) & (ind < B)
        for l in range(4):
            sel = np.nonzero((level == l + 2) & good)[0]
            e = oracle.crop_and_resize_backward(G[sel], boxes[sel], ind[sel], shapes[l])
            R.check_bar(torch.from_numpy(e), refs[l], mags[l], cnts[l], "crop %d level %d" % (crop, l + 2))
            assert float(refs[l].abs().max()) > 0


# ---- the bar: a legitimate fp32 result passes, the mistakes fail -------------------------------------------------------
def _conv3x3_fp32():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(1, 256, 24, 40, generator=g)
    w = torch.randn(64, 256, 3, 3, generator=g) * 0.05
    with torch.backends.mkldnn.flags(enabled=False):
        y = F.conv2d(x, w, padding=1)
    ref = R.conv_ref(x, w, (1, 1), (1, 1))
    mag = R.conv_ref(x.abs(), w.abs(), (1, 1), (1, 1))
    return x, w, y, ref, mag


def _wgrad_fp32():
    g = torch.Generator().manual_seed(8)
    x = torch.randn(1, 48, 256, 256, generator=g)          # K = 65536 pixels per weight element
    dy = torch.randn(1, 64, 256, 256, generator=g)
    with torch.backends.mkldnn.flags(enabled=False):
        dw = torch.nn.grad.conv2d_weight(x, (64, 48, 1, 1), dy)
    ref = R.wgrad_ref(x, dy, 1, 1)
    mag = R.wgrad_ref(x.abs(), dy.abs(), 1, 1)
    return x, dy, dw, ref, mag


def test_bar_passes_fp32_conv_and_fails_missing_k_slice_and_shifted_row():
    x, w, y, ref, mag = _conv3x3_fp32()
    K = 256 * 9
    worst = R.check_bar(y, ref, mag, K, "fp32 3x3x256")
    print("fp32 3x3x256 conv: worst |d|/(2^-24 m) = %.2f" % worst)
    # one 32 x 32 output block (32 channels x 32 pixels of a row) without its last 32-channel K-slice
    bad = y.clone()
    with torch.backends.mkldnn.flags(enabled=False):
        part = F.conv2d(x[:, -32:], w[:, -32:], padding=1)
    bad[0, 32:64, 5, 0:32] -= part[0, 32:64, 5, 0:32]
    assert R.bar_ratio(bad, ref, mag, K)[1] > 1.0
    # one output row shifted by one column at a tile edge (columns 16..31 of row 9 of one channel)
    bad = y.clone()
    bad[0, 17, 9, 16:32] = y[0, 17, 9, 15:31]
    assert R.bar_ratio(bad, ref, mag, K)[1] > 1.0


def test_bar_passes_fp32_wgrad_and_fails_a_dropped_pixel_split():
    x, dy, dw, ref, mag = _wgrad_fp32()
    K = 256 * 256
    worst = R.check_bar(dw, ref, mag, K, "fp32 wgrad K=65536")
    print("fp32 weight gradient K=65536: worst |d|/(2^-24 m) = %.2f" % worst)
    # eight pixel splits of 8192 pixels, fp32 partial sums; the fourth one dropped
    xs = x.reshape(48, -1)
    gs = dy.reshape(64, -1)
    parts = [gs[:, i * 8192:(i + 1) * 8192] @ xs[:, i * 8192:(i + 1) * 8192].t() for i in range(8)]
    full = sum(parts).reshape(64, 48, 1, 1)
    assert R.bar_ratio(full, ref, mag, K)[1] <= 1.0
    dropped = (full - parts[3].reshape(64, 48, 1, 1))
    assert R.bar_ratio(dropped, ref, mag, K)[1] > 1.0
    # ... also when only ONE weight element loses its split (one whose split sum is of typical size, |.| ~ 90)
    co, ci = np.unravel_index(int(torch.argmin((parts[3].abs() - 90.0).abs())), (64, 48))
    one = full.clone()
    one[co, ci] -= parts[3][co, ci]
    assert R.bar_ratio(one, ref, mag, K)[1] > 1.0


def test_bar_fails_a_crop_cell_missing_one_box(oracle):
    rs = np.random.RandomState(22)
    B, C, H = 1, 4, 32
    N, crop = 64, 7
    boxes = adversarial_boxes(rs, N, H, H)
    ind = np.zeros(N, np.int32)
    level = np.full(N, 2, np.int32)
    G = rs.standard_normal((N, C, crop, crop)).astype(np.float32)
    got = oracle.crop_and_resize_backward(G, boxes, ind, (B, C, H, H))
    refs, mags, cnts = R.crop_bwd_ref(torch.from_numpy(G), boxes, ind, level, [(B, C, H, H)], crop)
    R.check_bar(torch.from_numpy(got), refs[0], mags[0], cnts[0], "oracle crop backward")
    # the contribution of box 0 (an ordinary box) to the cell it touches most, left out of that one cell
    one = oracle.crop_and_resize_backward(G[:1], boxes[:1], ind[:1], (B, C, H, H))
    k = np.unravel_index(np.argmax(np.abs(one)), one.shape)
    assert (cnts[0][0, 0][k[2], k[3]] > 1), "the cell must hold more than one tap"
    bad = got.copy()
    bad[k] -= one[k]
    assert R.bar_ratio(torch.from_numpy(bad), refs[0], mags[0], cnts[0])[1] > 1.0


# ---- BatchNorm / class-row / patch-row / clip + SGD references (tests/test_gpu_step_glue_replay.py) ---------------------
def _fails(fn):
    with pytest.raises(AssertionError):
        fn()


@pytest.mark.parametrize("relu,res", [(True, False), (True, True), (False, False)])
def test_bn_act_bwd_ref_equals_autograd_and_the_bar_takes_fp32(relu, res):
    """dshift / dgamma of y = act(gamma xhat + beta (+ r)) against torch float64 autograd; an fp32 evaluation of the
    kernel's formula (xhat recovered from the fp32 y) passes the bar even at |beta| / |gamma| = 2000, and dgamma summed
    over a missing image fails it."""
    g = torch.Generator().manual_seed(5)
    N, C, HW = 3, 6, 23
    xh = torch.randn(N, C, HW, generator=g, dtype=D)
    ga = torch.randn(C, generator=g, dtype=D, requires_grad=True)
    be = torch.randn(C, generator=g, dtype=D, requires_grad=True)
    with torch.no_grad():
        ga[1], be[1] = 1e-3, 2.0
    r = torch.randn(N, C, HW, generator=g, dtype=D) if res else None
    pre = ga.view(1, -1, 1) * xh + be.view(1, -1, 1) + (r if res else 0.0)
    y = torch.relu(pre) if relu else pre
    dy = torch.randn(N, C, HW, generator=g, dtype=D)
    (y * dy).sum().backward()
    gg, ds, ms, dgam, mg = R.bn_act_bwd_ref(dy, y.detach(), xh, ga.detach(), be.detach(), relu, r)
    _close(ds, be.grad)
    _close(dgam, ga.grad)
    # the kernel's arithmetic in fp32, from the fp32 forward output
    y32, r32 = y.detach().float(), (r.float() if res else 0.0)
    g32 = torch.where(y32 > 0, dy.float(), torch.zeros_like(y32)) if relu else dy.float()
    xr = (y32 - r32 - be.detach().float().view(1, -1, 1)) / ga.detach().float().view(1, -1, 1)
    got = (g32 * xr).sum((0, 2))
    R.check_bar(got, dgam, mg, N * HW, "fp32 dgamma")
    R.check_bar(g32.sum((0, 2)), ds, ms, N * HW, "fp32 dshift")
    _fails(lambda: R.check_bar((g32 * xr)[1:].sum((0, 2)), dgam, mg, N * HW))


def test_rows_mask_scale_colsum_bar_rejects_a_dropped_row():
    g = torch.Generator().manual_seed(6)
    dy, y = torch.randn(300, 16, generator=g), torch.relu(torch.randn(300, 16, generator=g))
    gr, cs, mc = R.rows_mask_scale_ref(dy, y, True)
    _close(cs, torch.where(y > 0, dy, torch.zeros_like(dy)).double().sum(0))
    R.check_bar(gr.float().sum(0), cs, mc, 300)
    _fails(lambda: R.check_bar(gr.float()[torch.arange(300) != 137].sum(0), cs, mc, 300))


@pytest.mark.parametrize("taps,bias", [(9, True), (1, False), (9, False)])
def test_fold_grad_ref_equals_autograd_and_rejects_a_swapped_tap_order(taps, bias):
    """d gamma / d conv-bias / dW of conv + eval-BatchNorm from the weight gradient of the unscaled g (fi_bn_fold_grad)
    against torch float64 autograd of the whole layer; reading W in the other (tap-major) order fails the bar."""
    g = torch.Generator().manual_seed(7 + taps)
    k = 3 if taps == 9 else 1
    N, Ci, Co, H = 2, 5, 4, 6
    x = torch.randn(N, Ci, H, H, generator=g, dtype=D)
    w = torch.randn(Co, Ci, k, k, generator=g, dtype=D, requires_grad=True)
    cb = torch.randn(Co, generator=g, dtype=D, requires_grad=True) if bias else None
    ga = torch.randn(Co, generator=g, dtype=D, requires_grad=True)
    be = torch.randn(Co, generator=g, dtype=D)
    mean, var, eps = torch.randn(Co, generator=g, dtype=D), torch.rand(Co, generator=g, dtype=D) + 0.1, 1e-3
    z = F.conv2d(x, w, cb, padding=k // 2)
    inv = 1.0 / torch.sqrt(var + eps)
    y = (z - mean.view(1, -1, 1, 1)) * (ga * inv).view(1, -1, 1, 1) + be.view(1, -1, 1, 1)
    gy = torch.randn(y.shape, generator=g, dtype=D)
    (y * gy).sum().backward()
    dwp = R.wgrad_ref(x, gy, k, k, pad=(k // 2, k // 2)).reshape(Co, Ci, taps)
    s = gy.sum((0, 2, 3))
    scale = ga.detach() * inv
    dW, dgam, mg, dcb, mb = R.fold_grad_ref(dwp, w.detach().reshape(Co, Ci, taps), s, scale, mean, var, eps,
                                            cb.detach() if bias else None)
    _close(dW.reshape(w.shape), w.grad)
    _close(dgam, ga.grad)
    if bias:
        _close(dcb, cb.grad)
    got = R.fold_grad_ref(dwp.float(), w.detach().float().reshape(Co, Ci, taps), s.float(), scale.float(), mean.float(),
                          var.float(), eps, cb.detach().float() if bias else None)[1]
    R.check_bar(got.float(), dgam, mg, Ci * taps)
    if taps > 1:
        swapped = w.detach().permute(0, 2, 3, 1).reshape(Co, Ci, taps)        # W in tap-major order read as channel-major
        bad = R.fold_grad_ref(dwp, swapped, s, scale, mean, var, eps, cb.detach() if bias else None)[1]
        _fails(lambda: R.check_bar(bad, dgam, mg, Ci * taps))


@pytest.mark.parametrize("gated", [False, True])
def test_class_row_bwd_ref_equals_the_dense_autograd_and_rejects_a_double_accumulate(gated):
    g = torch.Generator().manual_seed(8)
    N, C, K, HW = 12, 5, 7, 10
    x = torch.relu(torch.randn(N, C, HW, generator=g, dtype=D)).requires_grad_(True)
    w = torch.randn(K, C, generator=g, dtype=D, requires_grad=True)
    b = torch.randn(K, generator=g, dtype=D, requires_grad=True)
    cls = torch.tensor([0, 3, 3, 6, 0, 0, 3, 1, 1, 6, 6, 3])
    d = torch.randn(N, HW, generator=g, dtype=D)
    d[1::2] = 0.0
    y = torch.einsum("kc,nch->nkh", w, x) + b.view(1, -1, 1)
    (y[torch.arange(N), cls] * d).sum().backward()
    dx, dw, mw, db, mb, nk = R.class_row_bwd_ref(d, x.detach(), w.detach(), cls, K, gated)
    _close(dw, w.grad)
    _close(db, b.grad)
    _close(dx, x.grad * (x.detach() > 0) if gated else x.grad)
    before = torch.randn(K, C, generator=g, dtype=D)
    R.check_increment((before + dw).float(), before.float(), dw, mw, nk[:, None].expand_as(dw))
    _fails(lambda: R.check_increment((before + 2 * dw).float(), before.float(), dw, mw, nk[:, None].expand_as(dw)))


def test_patch_rows_refs_are_adjoint_and_reject_an_off_by_one_tap():
    """The backward reference is the adjoint of the forward one (torch autograd through the forward); border anchors,
    level starts and padding rows included.  An off-by-one tap fails the bar (forward and backward)."""
    g = torch.Generator().manual_seed(9)
    shapes = [(2, 3, 5, 7), (2, 3, 3, 4)]
    per = 3
    total = sum(h * w * per for _, _, h, w in shapes)
    anchor = torch.cat([torch.tensor([0, 5 * 7 * per, total - 1, per * 6, per * 28]),
                        torch.randint(0, total, (20,), generator=g)])
    image = torch.randint(0, 2, (25,), generator=g)
    image[3] = -1
    maps = [torch.randn(*s, generator=g, dtype=D, requires_grad=True) for s in shapes]
    out = R.patch_rows_ref(maps, image, anchor, per)
    # a hand-made element: row 0 is anchor 0 of level 0, pixel (0, 0); tap 4 is the centre, tap 0 reads outside
    assert float(out[0, 4, 1]) == float(maps[0][image[0], 1, 0, 0]) and float(out[0, 0].abs().sum()) == 0.0
    assert float(out[3].abs().sum()) == 0.0                                    # padding row
    d = torch.randn(out.shape, generator=g, dtype=D)
    (out * d).sum().backward()
    gs, ms, ns = R.patch_rows_bwd_ref(d, shapes, image, anchor, per)
    for gr, m in zip(gs, maps):
        _close(gr, m.grad)
    R.check_bar(gs[0].float(), gs[0], ms[0], ns[0])
    bad_f = R.patch_rows_ref([m.detach() for m in maps], image, anchor, per, tap_shift=1)
    _fails(lambda: R.check_bar(bad_f, out.detach(), out.detach().abs(), 9))
    bad_b = R.patch_rows_bwd_ref(d, shapes, image, anchor, per, tap_shift=1)[0]
    _fails(lambda: R.check_bar(bad_b[0], gs[0], ms[0], ns[0]))


@pytest.mark.parametrize("momentum", [0.9, 0.0])
def test_sgd_ref_equals_torch_clip_and_sgd_and_rejects_a_missing_clip(momentum):
    g = torch.Generator().manual_seed(10)
    ps = [torch.randn(s, generator=g, dtype=D) for s in ((6, 5), (7,), (3, 2, 2))]
    gs = [torch.randn(p.shape, generator=g, dtype=D) * 3 for p in ps]
    bufs = [torch.randn(p.shape, generator=g, dtype=D) for p in ps]
    tp = [p.clone().requires_grad_(True) for p in ps]
    for t, gr in zip(tp, gs):
        t.grad = gr.clone()
    opt = torch.optim.SGD([{"params": tp[:2], "weight_decay": 1e-4}, {"params": tp[2:], "weight_decay": 0.0}],
                          lr=0.02, momentum=momentum)
    if momentum:
        for t, b in zip(tp, bufs):
            opt.state[t]["momentum_buffer"] = b.clone()
    norm = torch.nn.utils.clip_grad_norm_(tp, 5.0)
    opt.step()
    rn, n = R.grad_norm_ref(gs)
    assert abs(rn - float(norm)) <= 1e-12 * rn and n == sum(p.numel() for p in ps)
    coef = R.clip_coef_ref(rn, 5.0)
    assert coef < 1.0
    for i, (p, gr, b, t) in enumerate(zip(ps, gs, bufs, tp)):
        wd = 1e-4 if i < 2 else 0.0
        rp, rb, rg, mp, mb, mg = R.sgd_ref(p, gr, b if momentum else None, coef, wd, momentum, 0.02)
        _close(rp, t.detach())
        _close(rg, t.grad)
        if momentum:
            _close(rb, opt.state[t]["momentum_buffer"])
        R.check_bar(rp.float(), rp, mp, 1)
        bad = R.sgd_ref(p, gr, b if momentum else None, 1.0, wd, momentum, 0.02)[0]       # the clip factor left out
        _fails(lambda: R.check_bar(bad, rp, mp, 1))


# ---- loss and statistics references (tests/test_gpu_loss_kernels.py) -----------------------------------------------------
def _loss_case(seed, b=2, A=40, Rr=37, N=9, K=7, Nm=5, h=3, w=4):
    g = torch.Generator().manual_seed(seed)
    match = torch.zeros(b, A, dtype=D)
    deltas = torch.zeros(b, A, 4, dtype=D)
    im = torch.randint(0, b, (Rr,), generator=g)
    an = torch.randperm(A, generator=g)[:Rr] if Rr <= A else torch.randint(0, A, (Rr,), generator=g)
    im[torch.rand(Rr, generator=g) < 0.3] = -1                                   # padding rows, interleaved
    an[im < 0] = -1
    v = im >= 0
    kind = torch.randint(0, 2, (Rr,), generator=g).to(D) * 2 - 1                 # +1 / -1
    match[im[v], an[v]] = kind[v]
    deltas[im[v], an[v]] = torch.randn(int(v.sum()), 4, generator=g, dtype=D) * (kind[v] == 1)[:, None]
    ids = torch.randint(0, K, (N,), generator=g)
    ids[0] = 0
    mids = torch.randint(0, 2, (Nm,), generator=g) * torch.randint(1, K, (Nm,), generator=g)
    mk = lambda *s: (torch.randn(*s, generator=g, dtype=D) * 2).requires_grad_(True)
    return dict(match=match, deltas=deltas, im=im, an=an, ids=ids, mids=mids,
                tdel=torch.randn(N, 4, generator=g, dtype=D) * (ids > 0)[:, None],
                tmask=(torch.rand(Nm, 2 * h, 2 * w, generator=g) > 0.5).to(D),
                row_logits=mk(Rr, 2), row_bbox=mk(Rr, 4), cls_logits=mk(N, K), roi_bbox=mk(N, K, 4),
                mask_logits=mk(Nm, 2, 2, h, w))


def _layers_five(c, ids=None, mids=None):
    """The five loss functions of layers.py on the case's tensors (whatever their dtype and device)."""
    from feature_intertwiner_amd import layers as L
    ids = c["ids"] if ids is None else ids
    mids = c["mids"] if mids is None else mids
    rc, rb = L.compute_rpn_losses_on_rows(c["match"], c["deltas"], c["im"], c["an"], c["im"] >= 0, c["row_logits"],
                                          c["row_bbox"])
    return [rc, rb, L.compute_mrcnn_class_loss(ids[None], c["cls_logits"][None]),
            L.compute_mrcnn_bbox_loss(c["tdel"][None], ids[None], c["roi_bbox"][None]),
            L.compute_mrcnn_mask_loss_selected(c["tmask"][None], mids[None], c["mask_logits"][None])]


def _ref_of_case(c, ids=None, mids=None):
    d = lambda t: t.detach()
    return R.detector_losses_ref(c["match"], c["deltas"], c["im"], c["an"], d(c["row_logits"]), d(c["row_bbox"]),
                                 c["ids"] if ids is None else ids, d(c["cls_logits"]), c["tdel"], d(c["roi_bbox"]),
                                 c["mids"] if mids is None else mids, d(c["mask_logits"]), c["tmask"])


@pytest.mark.parametrize("fg", [True, False])
def test_detector_losses_ref_equals_the_loss_functions_in_float64(fg):
    """Values and gradients (autograd) of layers.py's five loss functions run in float64: the stored gradients times
    their factors are the gradients of the losses; padding rows, rows off the target class and non-positive mask rows
    are exactly zero; without any foreground the class loss and its factor are 0 while softmax - onehot stays stored."""
    c = _loss_case(11)
    ids = c["ids"] if fg else torch.zeros_like(c["ids"])
    mids = c["mids"] if fg else torch.zeros_like(c["mids"])
    outs = ("row_logits", "row_bbox", "cls_logits", "roi_bbox", "mask_logits")
    five = _layers_five(c, ids, mids)
    losses, factors, grads, counts = _ref_of_case(c, ids, mids)
    for k, (lv, name) in enumerate(zip(five, outs)):
        (gr,) = torch.autograd.grad(lv, c[name])
        lv = lv.detach()
        assert abs(float(lv) - float(losses[k])) <= 1e-12 * max(1.0, abs(float(lv))), (k, float(lv), float(losses[k]))
        assert float((grads[k] * factors[k] - gr.reshape(grads[k].shape)).abs().max()) <= 1e-12
    pad = c["im"] < 0
    assert int(pad.sum()) > 0 and float(grads[0][pad].abs().max()) == 0 and float(grads[1][pad].abs().max()) == 0
    assert float(counts[0]) == float((c["im"] >= 0).sum())
    off = torch.ones_like(grads[3], dtype=torch.bool)
    off[torch.arange(len(ids)), ids] = False
    assert float(grads[3][off].abs().max()) == 0 and float(grads[3][ids == 0].abs().max()) == 0
    assert float(grads[4][mids == 0].abs().max()) == 0
    if fg:
        assert float(counts[2]) == float((ids > 0).sum()) > 0 and float(counts[3]) == float((mids > 0).sum()) > 0
    else:
        assert [float(v) for v in losses[2:]] == [0.0, 0.0, 0.0] and float(factors[2]) == 0.0
        assert float(factors[3]) == 1.0 and float(factors[4]) == 1.0 and float(grads[2].abs().max()) > 0


def test_detector_losses_ref_smooth_l1_edges_and_the_target_shuffle():
    """|d| == 1, d == 0 and |d| just below 1 take the documented branch, and the mask target is read at
    [2y + a][2x + b]: a target that is 1 on exactly one pixel moves exactly one logit's loss term."""
    c = _loss_case(12, Rr=6, N=1, Nm=1, h=2, w=3)
    z = torch.zeros(1, 4, dtype=D)
    d = torch.tensor([[1.0, -1.0, 0.0, 1.0 - 2.0 ** -24]], dtype=D)
    ids = torch.tensor([3])
    box = torch.zeros(1, 7, 4, dtype=D)
    box[0, 3] = d
    out = R.detector_losses_ref(c["match"], c["deltas"], c["im"], c["an"], c["row_logits"].detach(), c["row_bbox"].detach(),
                                ids, c["cls_logits"].detach()[:1], z, box, torch.tensor([2]),
                                torch.zeros(1, 2, 2, 2, 3, dtype=D), torch.zeros(1, 4, 6, dtype=D))
    assert torch.equal(out[2][3][0, 3], torch.tensor([1.0, -1.0, 0.0, 1.0 - 2.0 ** -24], dtype=D))
    assert abs(float(out[0][3]) - (0.5 + 0.5 + 0.0 + 0.5 * (1.0 - 2.0 ** -24) ** 2) / 4) <= 1e-15
    base = float(out[0][4])
    assert abs(base - np.log(2.0)) <= 1e-15
    for (a, b, y, x) in ((0, 1, 1, 2), (1, 0, 0, 1)):
        tm = torch.zeros(1, 4, 6, dtype=D)
        tm[0, 2 * y + a, 2 * x + b] = 1.0
        lg = torch.zeros(1, 2, 2, 2, 3, dtype=D)
        lg[0, a, b, y, x] = 3.0                                  # the logit facing the set pixel: its term becomes -log p
        got = R.detector_losses_ref(c["match"], c["deltas"], c["im"], c["an"], c["row_logits"].detach(),
                                    c["row_bbox"].detach(), ids, c["cls_logits"].detach()[:1], z, box, torch.tensor([2]),
                                    lg, tm)
        exp = (23 * np.log(2.0) + np.log1p(np.exp(-3.0))) / 24
        assert abs(float(got[0][4]) - exp) <= 1e-15, (a, b, y, x)
        assert abs(float(got[2][4][0, a, b, y, x]) - (1 / (1 + np.exp(-3.0)) - 1.0)) <= 1e-15


def test_detector_losses_ref_returns_the_reference_values(golden_dir):
    """On the inputs of tests/golden/layers.npz, re-laid as the kernel reads them (rows of the non-zero anchors, the mask
    probabilities as un-shuffled logits of the target class): the five values the reference's loss functions returned.
    The fixture holds float32 results, so the bar is float32's (2e-6, as the existing tests of these values)."""
    import os
    from helpers import golden_loss_inputs
    gold = np.load(os.path.join(golden_dir, "layers.npz"))
    li = golden_loss_inputs()
    match = li["rpn_match"]
    B, A = match.shape
    per_anchor = np.zeros((B, A, 4), np.float32)
    rows = []
    for b in range(B):
        pos = np.nonzero(match[b] == 1)[0]
        per_anchor[b, pos] = li["rpn_bbox_target"][b, :len(pos)]
        nz = np.nonzero(match[b])[0]
        rows += [(b, a) for a in nz] + [(-1, -1)] * 5
    im, an = np.array(rows, np.int64).T
    ids = li["cls_ids"]
    Rn = ids.shape[1]
    p = li["mask_pred"].astype(np.float64)
    sel = np.take_along_axis(p, ids.reshape(B, Rn, 1, 1, 1).astype(np.int64), 2)[:, :, 0]
    logit = np.log(sel) - np.log1p(-sel)
    un = logit.reshape(B * Rn, 14, 2, 14, 2).transpose(0, 2, 4, 1, 3)
    losses = R.detector_losses_ref(match.astype(np.float64), per_anchor, im, an,
                                   li["rpn_logits"][np.maximum(im, 0), np.maximum(an, 0)],
                                   li["rpn_bbox_pred"][np.maximum(im, 0), np.maximum(an, 0)], ids.reshape(-1),
                                   li["cls_logits"].reshape(B * Rn, -1), li["bbox_target"].reshape(-1, 4),
                                   li["bbox_pred"].reshape(B * Rn, -1, 4), ids.reshape(-1), un,
                                   li["mask_target"].reshape(B * Rn, 28, 28))[0]
    names = ("loss_rpn_class", "loss_rpn_bbox", "loss_mrcnn_class", "loss_mrcnn_bbox", "loss_mrcnn_mask")
    for v, k in zip(losses, names):
        assert abs(float(v) - float(gold[k])) <= 2e-6 * max(1.0, abs(float(gold[k]))), (k, float(v), float(gold[k]))


def test_class_mean_ref_equals_the_oracle_and_the_bar_rejects_a_dropped_row(oracle):
    rs = np.random.RandomState(5)
    N, F_, K = 300, 37, 50
    x = rs.standard_normal((N, F_)).astype(np.float32)
    gt = rs.randint(-3, K + 8, N).astype(np.int32)
    gt[gt == 7] = 8                                              # an empty class
    ef, ec = oracle.class_mean(x, gt, K)
    feat, cnt, sa, rows = R.class_mean_ref(x, gt, K)
    assert np.array_equal(cnt.numpy(), ec[0].astype(np.float64)) and float(cnt[7]) == 0 and float(cnt[0]) == 0
    assert float(feat[:, 7].abs().max()) == 0 and float(feat[:, 0].abs().max()) == 0
    mag = sa / rows.clamp(min=1)[None]
    R.check_bar(torch.from_numpy(ef), feat, mag, rows[None].clamp(min=1).expand_as(feat), "oracle class mean")
    # fp32 sums of all rows of the class but one fail it
    c = int(torch.argmax(cnt))
    keep = np.nonzero(gt == c)[0][1:]
    bad = torch.from_numpy(ef).clone()
    bad[:, c] = torch.from_numpy(x[keep].sum(0) / float(cnt[c]))
    assert R.bar_ratio(bad, feat, mag, rows[None].clamp(min=1).expand_as(feat))[1] > 1.0
    # the backward is the adjoint: autograd through a dense float64 restatement
    xd = torch.from_numpy(x).double().requires_grad_(True)
    g = torch.from_numpy(gt).long()
    ok = (g > 0) & (g < K)
    oh = torch.zeros(N, K, dtype=D)
    oh[torch.arange(N)[ok], g[ok]] = 1.0
    dense = (xd.t() @ oh) / oh.sum(0).clamp(min=1)
    _close(feat, dense.detach())
    w = torch.from_numpy(rs.standard_normal((F_, K)))
    (dense * w).sum().backward()
    got = R.class_mean_bwd_ref(w, gt, cnt, K)
    _close(got, xd.grad)
    assert float(got[~ok].abs().max()) == 0


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("S,Dm,L", [(9, 3, 5), (33, 17, 1), (40, 1, 50)])
def test_sinkhorn_ref_equals_the_oracle(oracle, S, Dm, L, mode):
    rs = np.random.RandomState(S + Dm)
    x = rs.standard_normal((S, Dm)).astype(np.float32)
    y = rs.standard_normal((S, Dm)).astype(np.float32)
    if Dm == 1:
        x, y = np.maximum(x, 0), np.maximum(y, 0)
    v, pl = oracle.sinkhorn(x, y, 1.0, L, "l2" if mode else "cosine", return_plan=True)
    loss, plan = R.sinkhorn_ref(x, y, 1.0, L, mode)
    assert abs(float(loss) - float(v)) <= 1e-5 * abs(float(loss)) + 1e-9
    assert np.allclose(pl, plan.numpy(), rtol=1e-4, atol=1e-10)
    if mode == 0:                                                 # mode 2 = mode 0 on rows normalised by the caller
        xn = torch.from_numpy(x).double()
        yn = torch.from_numpy(y).double()
        xn, yn = xn / (xn.norm(dim=1, keepdim=True) + 1e-20), yn / (yn.norm(dim=1, keepdim=True) + 1e-20)
        l2, p2 = R.sinkhorn_ref(xn, yn, 1.0, L, 2)
        assert abs(float(l2) - float(loss)) <= 1e-13 and float((p2 - plan).abs().max()) <= 1e-15
    assert abs(float(plan.sum(0).sum()) - 1.0) <= 1e-12           # columns marginals 1/S after the last b update
    # the differentiable form returns the same value
    lt = R.sinkhorn_detached_plan_loss(torch.from_numpy(x).double()[None], torch.from_numpy(y).double()[None], 1.0, L,
                                       "l2" if mode else "cosine")
    assert abs(float(lt[0]) - float(loss)) <= 1e-13


@pytest.mark.parametrize("layout", ["stacked", "one_launch_view"])
def test_meta_stats_ref_equals_the_tensor_formulation(layout):
    """intertwiner.meta_loss's tensor path on the CPU, in float64, over three steps (the second without small-object
    statistics): history, counts, the l2 loss from SMALL / BIG / on, and the gradient into the small class features
    (meta_stats_bwd_ref of the loss's gradient with respect to SMALL)."""
    from types import SimpleNamespace as NS
    from helpers import golden_meta_inputs
    from feature_intertwiner_amd import intertwiner as IT
    K, F_ = 9, 21
    G, S = (2, 3) if layout == "stacked" else (1, 3)
    cfg = NS(DEV=NS(LOSS_CHOICE="l2", INST_LOSS=False))
    buf = IT.FeatureBuffer(1, F_, K, "cpu")
    buf.buffer, buf.buffer_cnt = buf.buffer.double(), buf.buffer_cnt.double()
    seen = []
    for step in (0, 2, 1):
        bf, bc, sf, sc = [torch.from_numpy(a).double() for a in golden_meta_inputs(step, K, F_, G=G, activation="sigmoid")]
        if layout == "one_launch_view":
            view = lambda t: t[0].permute(1, 0, 2).reshape(F_, S * K).contiguous().view(F_, S, K).permute(1, 0, 2).unsqueeze(0)
            bf, sf = view(bf), view(sf)
        old = (buf.buffer[0].clone(), buf.buffer_cnt.reshape(-1).clone())
        ref = R.meta_stats_ref(bf, bc, sf, sc, *old)
        sf = sf.detach().requires_grad_(True)
        loss = IT.meta_loss(cfg, buf, None, [bf, bc, sf, sc, None, None])
        loss.backward()
        seen.append(ref["active"])
        _close(ref["buffer"], buf.buffer[0])
        assert torch.equal(ref["buffer_cnt"], buf.buffer_cnt.reshape(-1))
        if not ref["active"]:
            assert torch.equal(ref["buffer"], old[0]) and float(loss) == 0.0
            continue
        SM = ref["SMALL"].clone().requires_grad_(True)
        on = ref["on"]
        exp = ((((SM - ref["BIG"]) ** 2).mean(1)) * on).sum() / on.sum().clamp(min=1)
        assert float(on.sum()) > 0 and abs(float(exp) - float(loss)) <= 1e-13 * abs(float(loss))
        exp.backward()
        _close(R.meta_stats_bwd_ref(SM.grad, ref["s_cnt"], sc), sf.grad)
        assert float(R.meta_stats_bwd_ref(SM.grad, ref["s_cnt"], sc)[..., 0].abs().max()) == 0
    assert seen == [True, False, True]
