"""crops16.pyramid_crops16 behind a make-up layer, and crops16.patch_rows16 with its gradient hand-off, bf16 and fp16.

Four 16-bit maps 2 x 256 x {16x24, 8x12, 4x6, 2x3}; the make-up layer (3x3 conv + eval BatchNorm + ReLU,
train16.conv_bn_act16) gives u2..u5 with a real ReLU pattern and a Gate16 each.  14 boxes over levels 2..5 and both images,
one with a level outside the pyramid, one degenerate.
  - the 7x7 and 14x14 crops are torch.equal to roi16.pyramid_crop16 of the same maps;
  - backward with random fp32 crop gradients: per level the reference is the sum of the two fp64_ref.crop_bwd_ref results
    where u > 0 and 0 elsewhere.  The returned g is ONE 16-bit rounding of an fp32 sum of n taps, so
        |g - ref| <= 1/2 ulp16(g) + 2^-24 (4 sqrt(n) + 16) m        on the summed m and n of the two crops
    (tests/test_gpu_crops16_kernels.py); masked-off elements are exactly +0;
  - the sums left in the gate are within fp64_ref.check_bar of the float64 sums of the returned g;
  - the make-up layer counts one premasked backward per level and no relu_grad16; its parameter gradients are finite;
  - with only the 7x7 crop used, the 14x14 crop's gradient arrives as None -- ONE RoIAlign backward runs, none accumulates
    -- and the result holds against the 7x7 reference alone.
patch_rows16 under grad mode: the rows are torch.equal to the raw launch; backward adds into the 16-bit tensor a GradBox
holds IN PLACE and returns that very tensor, a level without a box gets zeros plus its rows, and p6 as p5 with step 2 gets
no gradient of its own."""
import pytest
import torch

import fp64_ref as R
from test_gpu_grad16_layer import CL, DEV, DTYPES, _layer
from test_gpu_crops16_kernels import PER_LOC, SIZES, _rows, held16

pytestmark = pytest.mark.gpu


def _boxes():
    b = torch.tensor([[0.05, 0.10, 0.45, 0.60], [0.20, 0.25, 0.30, 0.33], [0.00, 0.00, 1.00, 1.00], [0.55, 0.40, 0.95, 0.90],
                      [0.10, 0.50, 0.80, 0.70], [0.33, 0.33, 0.66, 0.66], [0.70, 0.05, 0.99, 0.35], [0.02, 0.60, 0.40, 0.98],
                      [0.25, 0.25, 0.75, 0.75], [0.40, 0.10, 0.60, 0.90], [0.15, 0.15, 0.50, 0.45], [0.60, 0.60, 0.90, 0.95],
                      [0.30, 0.20, 0.30, 0.70],                       # degenerate: no height
                      [0.10, 0.10, 0.90, 0.90]], dtype=torch.float32)
    level = torch.tensor([2, 2, 5, 3, 4, 2, 3, 4, 5, 3, 2, 4, 3, 6], dtype=torch.int32)      # the last: outside the pyramid
    ind = torch.tensor([0, 1, 0, 1, 0, 1, 0, 1, 1, 0, 0, 1, 1, 0], dtype=torch.int32)
    return b.to(DEV), ind.to(DEV), level.to(DEV)


def _setup(sfx, seed):
    from feature_intertwiner_amd import train16
    dtype = DTYPES[sfx]
    gen = torch.Generator().manual_seed(seed)
    conv, bn = _layer(256, 256, 3, 1, seed + 1, weight_cl=True)
    ps = [torch.randn((2, 256, h, w), generator=gen).to(dtype).to(DEV).contiguous(memory_format=CL).requires_grad_()
          for h, w in SIZES]
    us = [train16.conv_bn_act16(p, conv, bn, relu=True) for p in ps]
    for u in us:
        frac = float((u > 0).float().mean())
        assert 0.2 < frac < 0.8, frac                                # a real ReLU pattern
    return conv, bn, ps, us, gen


def _record_gate_pack(monkeypatch):
    from feature_intertwiner_amd import crops16
    calls = []

    def rec(d, y=None, dtype=None, colsum=True, _fn=crops16.gate_pack16):
        out = _fn(d, y, dtype=dtype, colsum=colsum)
        calls.append((d.clone(), y, out[0], out[1]))
        return out
    monkeypatch.setattr(crops16, "gate_pack16", rec)
    return calls


def _check(calls, us, crops_and_grads, boxes, ind, level, sfx, what):
    shapes = [tuple(u.shape) for u in us]
    ref = [torch.zeros(s, dtype=torch.float64, device=DEV) for s in shapes]
    mag = [torch.zeros(s, dtype=torch.float64, device=DEV) for s in shapes]
    cnt = [torch.zeros((s[0], 1, s[2], s[3]), dtype=torch.float64, device=DEV) for s in shapes]
    for size, d in crops_and_grads:
        r, m, n = R.crop_bwd_ref(d, boxes, ind, level, shapes, size)
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


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_two_crops_behind_a_make_up_layer(sfx, monkeypatch):
    from feature_intertwiner_amd import crops16, grad16, roi16, train16
    conv, bn, ps, us, gen = _setup(sfx, 41)
    boxes, ind, level = _boxes()
    calls = _record_gate_pack(monkeypatch)
    crops16.reset_stats()
    c7, c14 = crops16.pyramid_crops16(us, [(boxes, ind, level, 7), (boxes, ind, level, 14)])
    assert crops16.stats()["crops"] == 1
    assert c7.dtype == torch.float32 and tuple(c7.shape) == (14, 256, 7, 7) and c7.is_contiguous() and c7.requires_grad
    assert tuple(c14.shape) == (14, 256, 14, 14) and c14.is_contiguous()
    with torch.no_grad():
        det = [u.detach() for u in us]
        assert torch.equal(c7, roi16.pyramid_crop16(det, boxes, ind, level, 7, 7))
        assert torch.equal(c14, roi16.pyramid_crop16(det, boxes, ind, level, 14, 14))
    assert bool((c7[13] == 0).all()) and bool((c14[13] == 0).all())   # the level outside the pyramid
    d7 = torch.randn(tuple(c7.shape), generator=gen).to(DEV)
    d14 = torch.randn(tuple(c14.shape), generator=gen).to(DEV)
    train16.reset_stats()
    grad16.reset_stats()
    torch.autograd.backward([c7, c14], [d7, d14])
    torch.cuda.synchronize()
    assert crops16.stats()["gate_pack"] == 4
    t, g = train16.stats(), grad16.stats()
    assert t["premasked"] == 4 and t["fallback"] == 0 and g["relu_grad"] == 0, (t, g)
    assert g["wgrad"] == 4 and g["dgrad"] == 4
    _check(calls, us, [(7, d7), (14, d14)], boxes, ind, level, sfx, "two crops %s" % sfx)
    for p in ps:
        assert p.grad is not None and p.grad.dtype == DTYPES[sfx] and bool(torch.isfinite(p.grad.float()).all())
        assert float(p.grad.float().abs().max()) > 0.0
    for prm in list(conv.parameters()) + list(bn.parameters()):
        assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()) and float(prm.grad.abs().max()) > 0.0


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_one_of_the_two_crops_unused(sfx, monkeypatch):
    from feature_intertwiner_amd import _lib, crops16, grad16, train16
    conv, bn, ps, us, gen = _setup(sfx, 47)
    boxes, ind, level = _boxes()
    calls = _record_gate_pack(monkeypatch)
    taps = []
    monkeypatch.setattr(_lib, "TAP", lambda name, **kw: taps.append((kw["crop"], kw["accumulate"]))
                        if name == "pyramid_crop_backward" else None)
    c7, c14 = crops16.pyramid_crops16(us, [(boxes, ind, level, 7), (boxes, ind, level, 14)])
    d7 = torch.randn(tuple(c7.shape), generator=gen).to(DEV)
    train16.reset_stats()
    grad16.reset_stats()
    c7.backward(d7)
    torch.cuda.synchronize()
    assert taps == [(7, False)], taps                                # the 14x14 gradient was None: nothing launched for it
    assert train16.stats()["premasked"] == 4 and grad16.stats()["relu_grad"] == 0
    _check(calls, us, [(7, d7)], boxes, ind, level, sfx, "one crop %s" % sfx)
    del c14


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_patch_rows16_adds_into_the_boxed_gradient_in_place(sfx):
    from feature_intertwiner_amd import conv as C, crops16
    dtype = DTYPES[sfx]
    gen = torch.Generator().manual_seed(53)
    ps = [torch.randn((2, 256, h, w), generator=gen).to(dtype).to(DEV).contiguous(memory_format=CL).requires_grad_()
          for h, w in SIZES]
    image, anchor = _rows()
    maps, steps = ps + [ps[3]], [1, 1, 1, 1, 2]
    with torch.no_grad():
        raw = crops16.patch_rows16(maps, image, anchor, PER_LOC, steps=steps)
    boxes = [C.GradBox() for _ in range(4)] + [None]
    for b in boxes[:4]:
        b.taker = True
    crops16.reset_stats()
    rows = crops16.patch_rows16(maps, image, anchor, PER_LOC, boxes, steps)
    assert rows.requires_grad and torch.equal(rows, raw) and tuple(rows.shape) == (40, 9 * 256)
    left = [(0.5 * torch.randn(tuple(p.shape), generator=gen)).to(dtype).to(DEV).contiguous(memory_format=CL) for p in ps]
    for l in (0, 1, 3):                                              # level 2 of the list (p4) stays empty: zeros
        boxes[l].value = left[l].clone(memory_format=torch.preserve_format)
    held = [b.value for b in boxes[:4]]
    seen = {}
    for l, p in enumerate(ps):
        p.register_hook(lambda g, l=l: seen.__setitem__(l, g.data_ptr()))      # what the backward hands to autograd
    d = torch.randn(tuple(rows.shape), generator=gen).to(DEV)
    rows.backward(d)
    torch.cuda.synchronize()
    assert crops16.stats() == {"patch_fwd": 1, "patch_bwd": 1, "gate_pack": 0, "crops": 0}
    assert all(b.value is None for b in boxes[:4])
    shapes = [tuple(p.shape) for p in ps] + [(2, 256, 1, 2)]
    refs, mags, _ = R.patch_rows_bwd_ref(d.view(40, 9, 256), shapes, image, anchor, PER_LOC)
    cnts, _, _ = R.patch_rows_bwd_ref(torch.ones_like(d).view(40, 9, 256), shapes, image, anchor, PER_LOC)
    for t in (refs, mags, cnts):
        t[3] = t[3].clone()
        t[3][:, :, ::2, ::2] += t[4]
    for l, p in enumerate(ps):
        assert p.grad is not None and p.grad.dtype == dtype
        if held[l] is not None:
            assert seen[l] == held[l].data_ptr()                     # in place: the boxed tensor IS the gradient
        old = (left[l] if held[l] is not None else torch.zeros_like(left[l])).to(torch.float64)
        touched = cnts[l] > 0
        assert bool(((p.grad.view(torch.int16) == old.to(dtype).view(torch.int16)) | touched).all())
        held16(p.grad, torch.where(touched, old + refs[l], old), old.abs() + mags[l], cnts[l] + 1.0, sfx,
               "patch_rows16 backward %s level %d" % (sfx, l))
