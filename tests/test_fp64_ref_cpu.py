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
