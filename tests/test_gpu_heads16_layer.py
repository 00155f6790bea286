"""heads16.pyramid_crops_heads16 behind a make-up layer and heads16.class_rows_out16, bf16 and fp16.

The node.  The maps, the make-up layer and the 14 boxes are those of tests/test_gpu_crops16_layer.py (four 16-bit maps
2 x 256 x {16x24, 8x12, 4x6, 2x3} through a 3x3 conv + eval BatchNorm + ReLU with a Gate16 each; one box with a level outside
the pyramid, one degenerate).  The box head reads all 14 boxes at 7x7, the mask head's graph batch boxes 0..5 at 14x14, the
rest batch boxes 6..13, the feature extractor a permutation of the 14 at 14x14 in fp32.
  - forward: the 16-bit crops are torch.equal to head16.pyramid_crop16_cl of the same maps and boxes, the fp32 rows to
    roi16.pyramid_crop16; the rest crop does not require grad;
  - backward, all three readers in one call: two crop_backward16 launches (the first clears) and one accumulating
    fi_pyramid_crop_backward_nhwc, in that order (the _lib.TAP records), four gate-pack launches; per level the reference
    is the sum of the three fp64_ref.crop_bwd_ref results where u > 0 and 0 elsewhere, and the returned g is ONE 16-bit
    rounding of an fp32 sum of n taps:
        |g - ref| <= 1/2 ulp16(g) + 2^-24 (4 sqrt(n) + 16) m        on the summed m and n of the three readers
    (check_crop_bwd's bar plus the gate-pack rounding, as tests/test_gpu_crops16_layer.py); masked-off elements are
    exactly +0; the sums left in the gates are within fp64_ref.check_bar of the float64 sums of g; the make-up layer runs
    four premasked backwards and no relu_grad16;
  - a reader with no gradient is skipped: with the mask head's batch alone ONE launch runs, and it clears; with the feature
    extractor's rows alone the fp32 launch clears.
The class-selected output layer, on [3, 4 x 32, 14, 14] with 5 classes.
  - forward: sel[i, a, b, h, w] is out1x1_16 of the rows of u16 at column cls[i], bit for bit;
  - backward: ONE class-rows launch and nothing else; u16's gradient has the bits of heads16.class_rows_grad16 on the same
    operands (tests/test_gpu_heads16_kernels.py holds that launch to float64); d weight and d bias are within
    B(count, sum |terms|) of fp64_ref.class_row_bwd_ref; rows of classes without a RoI are exactly zero;
  - with a Gate16 on u16 the layer claims it and leaves du and its column sums there."""
import pytest
import torch

import fp64_ref as R
from test_gpu_grad16_layer import CL, DEV, DTYPES
from test_gpu_crops16_kernels import held16
from test_gpu_crops16_layer import _boxes, _record_gate_pack, _setup

pytestmark = pytest.mark.gpu
FRONT = 6


def _specs(gen):
    boxes, ind, level = _boxes()
    order = torch.randperm(boxes.shape[0], generator=gen).to(DEV)
    box = (boxes, ind, level, 7)
    front = (boxes[:FRONT].contiguous(), ind[:FRONT].contiguous(), level[:FRONT].contiguous(), 14)
    rest = (boxes[FRONT:].contiguous(), ind[FRONT:].contiguous(), level[FRONT:].contiguous(), 14)
    feat = (boxes[order].contiguous(), ind[order].contiguous(), level[order].contiguous(), 14)
    return box, front, rest, feat


def _check_maps(calls, us, readers, sfx, what):
    """readers: (spec, d) with d the reader's crop gradient; the checks of test_gpu_crops16_layer._check over their sum."""
    shapes = [tuple(u.shape) for u in us]
    ref = [torch.zeros(s, dtype=torch.float64, device=DEV) for s in shapes]
    mag = [torch.zeros(s, dtype=torch.float64, device=DEV) for s in shapes]
    cnt = [torch.zeros((s[0], 1, s[2], s[3]), dtype=torch.float64, device=DEV) for s in shapes]
    for (boxes, ind, level, size), d in readers:
        r, m, n = R.crop_bwd_ref(d.float().contiguous(), boxes, ind, level, shapes, size)
        for l in range(4):
            ref[l] += r[l]
            mag[l] += m[l]
            cnt[l] += n[l]
    assert len(calls) == 4
    for l, (d32, y, g, s) in enumerate(calls):
        assert y.data_ptr() == us[l].data_ptr() and g.dtype == us[l].dtype and g.is_contiguous(memory_format=CL)
        opened = us[l].detach() > 0
        assert bool((g[~opened].view(torch.int16) == 0).all()), "masked-off elements are +0"
        want = torch.where(opened, ref[l], torch.zeros_like(ref[l]))
        held16(g, want, mag[l], torch.clamp_min(cnt[l], 1.0), sfx, "%s level %d" % (what, l + 2))
        assert float(g.float().abs().max()) > 0.0
        g64 = g.to(torch.float64)
        P = g.shape[0] * g.shape[2] * g.shape[3]
        R.check_bar(s, g64.sum((0, 2, 3)), g64.abs().sum((0, 2, 3)), P, "%s sums level %d" % (what, l + 2))


def _tap(monkeypatch):
    from feature_intertwiner_amd import _lib
    taps = []
    monkeypatch.setattr(_lib, "TAP", lambda name, **kw: taps.append((kw["crop"], kw["accumulate"], kw["grads"].dtype))
                        if name == "pyramid_crop_backward" else None)
    return taps


def _rand16(shape, dtype, gen):
    return torch.randn(shape, generator=gen).to(dtype).to(DEV).contiguous(memory_format=CL)


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_three_readers_behind_a_make_up_layer(sfx, monkeypatch):
    from feature_intertwiner_amd import crops16, grad16, head16, heads16, roi16, train16
    dtype = DTYPES[sfx]
    conv, bn, ps, us, gen = _setup(sfx, 61)
    box, front, rest, feat = _specs(gen)
    calls = _record_gate_pack(monkeypatch)
    taps = _tap(monkeypatch)
    heads16.reset_stats()
    crops16.reset_stats()
    pooled, cfront, crest, cfeat = heads16.pyramid_crops_heads16(us, box, front, rest, feat)
    assert heads16.stats()["crops"] == 1
    assert pooled.dtype == dtype and tuple(pooled.shape) == (14, 256, 7, 7) and pooled.is_contiguous(memory_format=CL)
    assert cfront.dtype == dtype and tuple(cfront.shape) == (FRONT, 256, 14, 14) and cfront.requires_grad
    assert crest.dtype == dtype and tuple(crest.shape) == (14 - FRONT, 256, 14, 14) and not crest.requires_grad
    assert cfeat.dtype == torch.float32 and tuple(cfeat.shape) == (14, 256, 14, 14) and cfeat.is_contiguous()
    with torch.no_grad():
        det = [u.detach() for u in us]
        for got, (b, i, l, size) in ((pooled, box), (cfront, front), (crest, rest)):
            assert torch.equal(got.view(torch.int16), head16.pyramid_crop16_cl(det, b, i, l, size, size).view(torch.int16))
        assert torch.equal(cfeat, roi16.pyramid_crop16(det, feat[0], feat[1], feat[2], 14, 14))
    assert bool((pooled[13] == 0).all())                              # the level outside the pyramid
    d7 = _rand16(tuple(pooled.shape), dtype, gen)
    d14 = _rand16(tuple(cfront.shape), dtype, gen)
    dfeat = torch.randn(tuple(cfeat.shape), generator=gen).to(DEV)
    train16.reset_stats()
    grad16.reset_stats()
    torch.autograd.backward([pooled, cfront, cfeat], [d7, d14, dfeat])
    torch.cuda.synchronize()
    assert taps == [(7, False, dtype), (14, True, dtype), (14, True, torch.float32)], taps
    assert heads16.stats()["crop_bwd"] == 2 and crops16.stats()["gate_pack"] == 4
    t, g = train16.stats(), grad16.stats()
    assert t["premasked"] == 4 and t["fallback"] == 0 and g["relu_grad"] == 0, (t, g)
    assert g["wgrad"] == 4 and g["dgrad"] == 4
    _check_maps(calls, us, [(box, d7), (front, d14), (feat, dfeat)], sfx, "three readers %s" % sfx)
    for p in ps:
        assert p.grad is not None and p.grad.dtype == dtype and bool(torch.isfinite(p.grad.float()).all())
        assert float(p.grad.float().abs().max()) > 0.0
    for prm in list(conv.parameters()) + list(bn.parameters()):
        assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()) and float(prm.grad.abs().max()) > 0.0


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("reader", ["front", "feat"])
def test_a_reader_without_a_gradient_is_skipped(reader, sfx, monkeypatch):
    from feature_intertwiner_amd import grad16, heads16, train16
    dtype = DTYPES[sfx]
    conv, bn, ps, us, gen = _setup(sfx, 67)
    box, front, rest, feat = _specs(gen)
    calls = _record_gate_pack(monkeypatch)
    taps = _tap(monkeypatch)
    heads16.reset_stats()
    pooled, cfront, crest, cfeat = heads16.pyramid_crops_heads16(us, box, front, None, feat)
    assert crest is None
    train16.reset_stats()
    grad16.reset_stats()
    if reader == "front":
        d = _rand16(tuple(cfront.shape), dtype, gen)
        cfront.backward(d)
        spec, want_taps, launches = front, [(14, False, dtype)], 1
    else:
        d = torch.randn(tuple(cfeat.shape), generator=gen).to(DEV)
        cfeat.backward(d)
        spec, want_taps, launches = feat, [(14, False, torch.float32)], 0
    torch.cuda.synchronize()
    assert taps == want_taps, taps
    assert heads16.stats()["crop_bwd"] == launches
    assert train16.stats()["premasked"] == 4 and grad16.stats()["relu_grad"] == 0
    _check_maps(calls, us, [(spec, d)], sfx, "%s alone %s" % (reader, sfx))
    del pooled


def _mask_tail(sfx, seed, gate):
    from feature_intertwiner_amd import train16
    dtype = DTYPES[sfx]
    gen = torch.Generator().manual_seed(seed)
    n, C, H, W, K = 3, 32, 14, 14, 5
    u = torch.relu(torch.randn((n, 4 * C, H, W), generator=gen))
    u16 = u.to(dtype).to(DEV).contiguous(memory_format=CL).requires_grad_()
    conv5 = torch.nn.Conv2d(C, K, 1).to(DEV)
    with torch.no_grad():
        conv5.weight.copy_((torch.randn((K, C, 1, 1), generator=gen) / 4.0).to(DEV))
        conv5.bias.copy_(torch.randn(K, generator=gen).to(DEV))
    cls = torch.tensor([4, 1, 4], dtype=torch.int64, device=DEV)      # classes 0, 2 and 3 have no RoI
    if gate:
        u16._fi_gate16 = train16.Gate16()
    d = torch.randn((n, 2, 2, H, W), generator=gen).to(DEV)
    return u16, conv5, cls, d


@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("gate", [False, True], ids=["autograd", "gate16"])
def test_class_selected_output_layer(gate, sfx):
    from feature_intertwiner_amd import act16, conv as C_, grad16, head16, heads16, train16
    dtype = DTYPES[sfx]
    u16, conv5, cls, d = _mask_tail(sfx, 71, gate)
    n, C4, H, W = u16.shape
    C, K, HW = C4 // 4, conv5.weight.shape[0], H * W
    assert C_.GATES
    heads16.reset_stats()
    grad16.reset_stats()
    train16.reset_stats()
    sel = heads16.class_rows_out16(u16, conv5, cls)
    assert sel.dtype == torch.float32 and tuple(sel.shape) == (n, 2, 2, H, W) and sel.requires_grad
    with torch.no_grad():
        w16 = act16.weight16(conv5.weight, dtype).view(K, C)
        rows = u16.detach().permute(0, 2, 3, 1).reshape(n * HW * 4, C).view(n * HW * 4, C, 1, 1)
        full = head16.out1x1_16(rows, w16, conv5.bias, act=head16.NONE, layout=head16.ROWS).view(n, H, W, 2, 2, K)
        for i in range(n):
            assert torch.equal(sel[i], full[i, :, :, :, :, int(cls[i])].permute(2, 3, 0, 1)), i
    sel.backward(d)
    torch.cuda.synchronize()
    assert heads16.stats()["class_rows"] == 1
    assert grad16.stats() == {k: 0 for k in grad16.stats()} and train16.stats()["gated"] == 0
    dw_direct = torch.zeros((K, C), device=DEV)
    db_direct = torch.zeros((K,), device=DEV)
    du, s = heads16.class_rows_grad16(d, u16.detach(), w16, cls, dweight=dw_direct, dbias=db_direct)
    assert u16.grad is not None and u16.grad.dtype == dtype
    assert torch.equal(u16.grad.view(torch.int16), du.view(torch.int16))
    x = u16.detach().to(torch.float64).reshape(n, 4, C, HW).permute(0, 2, 1, 3).reshape(n, C, 4 * HW)
    _, dw_ref, mw, db_ref, mb, cnt = R.class_row_bwd_ref(d.reshape(n, 4 * HW), x, w16, cls, K, True)
    dw, db = conv5.weight.grad, conv5.bias.grad
    assert tuple(dw.shape) == (K, C, 1, 1) and tuple(db.shape) == (K,)
    print("class rows layer %s: dweight worst |d| / (2^-24 m) = %.3f, dbias %.3f" % (
        sfx, R.check_bar(dw.view(K, C), dw_ref, mw, cnt[:, None].expand_as(mw), "dweight"),
        R.check_bar(db, db_ref, mb, cnt, "dbias")))
    for k in (0, 2, 3):
        assert bool((dw[k] == 0).all()) and float(db[k]) == 0.0
    assert float(dw[4].abs().max()) > 0.0 and float(db[1].abs()) > 0.0
    g16 = u16._fi_gate16 if gate else None
    if gate:
        assert g16.claimed and g16.wrote is not None
        assert torch.equal(g16.wrote.view(torch.int16), u16.grad.view(torch.int16))
        g64 = du.to(torch.float64)
        R.check_bar(g16.sums, g64.sum((0, 2, 3)), g64.abs().sum((0, 2, 3)), n * HW, "sums left in the gate")
        assert g16.take(g16.wrote) is not None                       # what a producer's backward would find
