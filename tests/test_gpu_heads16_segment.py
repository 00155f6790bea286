"""The pieces of heads16 together, bf16 and fp16: make-up layer -> heads16.pyramid_crops_heads16 -> Classifier and Mask on
16-bit crops with a graph -> one backward.  The maps, the make-up layer and the 14 boxes are those of
tests/test_gpu_crops16_layer.py (256 channels); Classifier(256, 5, 7) reads the 7 x 7 crops of all boxes, Mask(256, 5) the
14 x 14 crops of boxes 0..5 with the classes (4, 1, 4, 2, 1, 3); the rest batch and the feature extractor's rows get no
gradient.

  - the heads' inputs ARE the node's outputs (16-bit channels-last, requiring grad) and both take their training branch;
  - counters of the one backward, the sum of the three pieces' own (tests/test_gpu_heads16_box.py, _mask.py, _layer.py):
    gated 2 + 4, plain data gradients 1 + 1 + 4 (the make-up layers'), weight gradients 3 + 5 + 4, premasked 2 + 5 + 4, no
    fallback, NO relu_grad16, two crop_backward16 launches (the first clears), one class-rows launch, four gate-packs, no
    fp32 RoIAlign backward;
  - the crop gradients the node received (the _lib.TAP records) are 16-bit channels-last, and the map gradients hold against
    float64 on exactly those: test_gpu_heads16_layer._check_maps;
  - every parameter of the three modules and every map leaf has a finite, non-zero gradient."""
import pytest
import torch

from test_gpu_grad16_layer import CL, DEV, DTYPES
from test_gpu_crops16_layer import _record_gate_pack, _setup
from test_gpu_heads16_box import _head
from test_gpu_heads16_layer import FRONT, _check_maps, _specs
from test_gpu_heads16_mask import _mask
from test_gpu_train16_block import _counts, _reset

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sfx", sorted(DTYPES))
def test_make_up_layer_to_both_heads_and_back(sfx, monkeypatch):
    from feature_intertwiner_amd import _lib, crops16, heads16
    dtype = DTYPES[sfx]
    conv, bn, ps, us, gen = _setup(sfx, 103)
    box, front, rest, feat = _specs(gen)
    box_head, mask_head = _head(107, depth=256), _mask(109, depth=256)
    cls = torch.tensor([4, 1, 4, 2, 1, 3], dtype=torch.int64, device=DEV)
    assert cls.numel() == FRONT
    calls = _record_gate_pack(monkeypatch)
    taps = []
    monkeypatch.setattr(_lib, "TAP", lambda name, **kw: taps.append(kw) if name == "pyramid_crop_backward" else None)
    pooled, cfront, crest, cfeat = heads16.pyramid_crops_heads16(us, box, front, rest, feat)
    logits, _, bbox = box_head(pooled)
    sel = mask_head(cfront, shuffled=False, activate=False, select_class=cls)
    assert logits.requires_grad and sel.requires_grad and tuple(sel.shape) == (FRONT, 2, 2, 14, 14)
    d = [torch.randn(tuple(t.shape), generator=gen).to(DEV) for t in (logits, bbox, sel)]
    _reset()
    heads16.reset_stats()
    crops16.reset_stats()
    torch.autograd.backward([logits, bbox, sel], d)
    torch.cuda.synchronize()
    assert _counts() == dict(gated=6, premasked=11, fallback=0, relu_grad=0, dgrad=6, wgrad=12), _counts()
    h = heads16.stats()
    assert h["crop_bwd"] == 2 and h["class_rows"] == 1 and crops16.stats()["gate_pack"] == 4, (h, crops16.stats())
    assert [(t["crop"], t["accumulate"], t["grads"].dtype) for t in taps] == [(7, False, dtype), (14, True, dtype)]
    for t in taps:
        assert t["grads"].is_contiguous(memory_format=CL)
    _check_maps(calls, us, [(box, taps[0]["grads"]), (front, taps[1]["grads"])], sfx, "both heads %s" % sfx)
    for p in ps:
        assert p.grad is not None and p.grad.dtype == dtype and bool(torch.isfinite(p.grad.float()).all())
        assert float(p.grad.float().abs().max()) > 0.0
    for mod in (conv, bn, box_head, mask_head):
        for name, prm in mod.named_parameters():
            assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()) and float(prm.grad.abs().max()) > 0.0, name
    del crest, cfeat
