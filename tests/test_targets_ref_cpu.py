"""tests/targets_ref.py (the NumPy restatement the GPU edge tests compare the target kernels with) held to what the project
already trusts, on inputs without ties: the tensor formulation of layers.py on the CPU and the oracle's line-by-line
restatement of lib/layers.py:439-604; one hand-written tie case per kernel pins the tie rule itself; and every input of
tests/test_gpu_target_edges.py is checked here, without a GPU, to be what it is named for and to keep its margin from the
thresholds."""
import numpy as np
import pytest
import torch

import target_edge_cases as EC
import targets_ref as TR
from test_targets import _candidates, _cfg, _gt, _perm_dropping


def _unique_keys(b, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([1.0 + (torch.randperm(n, generator=g).float() + 0.5) / n for _ in range(b)])


def _pyramid(cfg):
    from feature_intertwiner_amd import layers as L
    return L.generate_pyramid_priors(cfg.RPN.ANCHOR_SCALES, cfg.RPN.ANCHOR_RATIOS, cfg.MODEL.BACKBONE_SHAPES,
                                     cfg.MODEL.BACKBONE_STRIDES, 1).astype(np.float32)


@pytest.mark.parametrize("crowd,pos_thres", [(False, 0.7), (True, 0.7), (False, 0.4)])
def test_rpn_ref_equals_the_tensor_formulation_and_the_oracle(oracle, crowd, pos_thres):
    from feature_intertwiner_amd import layers as L
    cfg = _cfg(backbone="resnet50", image_size=256)
    cfg.RPN.TARGET_POS_THRES = pos_thres
    anchors = _pyramid(cfg)
    A, n_total = len(anchors), cfg.RPN.TRAIN_ANCHORS_PER_IMAGE
    cls, boxes = _gt(np.random.RandomState(3), 3, 12, 256, [12, 7, 0], crowd)
    kp, kn = _unique_keys(3, A, 1), _unique_keys(3, A, 2)
    ref = TR.rpn_targets_ref(anchors, cls, boxes, kp.numpy(), kn.numpy(), cfg.RPN.TARGET_NEG_THRES, pos_thres, n_total,
                             cfg.DATA.BBOX_STD_DEV)
    match, deltas = L._rpn_target_tensors(torch.from_numpy(anchors), torch.from_numpy(cls), torch.from_numpy(boxes), cfg, kp, kn)
    match, deltas = match.numpy(), deltas.numpy()
    assert np.array_equal(ref.match, match)
    assert np.all(ref.deltas[ref.match != 1] == 0)
    assert np.allclose(deltas, ref.deltas, rtol=1e-5, atol=1e-6)
    ra = ref.row_anchor.reshape(3, n_total)
    for i in range(3):
        m0 = _candidates(oracle, anchors, cls[i], boxes[i], cfg)
        pos_c, neg_c = np.nonzero(m0 == 1)[0], np.nonzero(m0 == -1)[0]
        cand, _, _ = TR.rpn_candidates(anchors, cls[i], boxes[i], cfg.RPN.TARGET_NEG_THRES, pos_thres)
        assert np.array_equal(cand, m0)                                     # the candidate sets are the reference's
        kept_pos, kept_neg = np.nonzero(ref.match[i] == 1)[0], np.nonzero(ref.match[i] == -1)[0]
        if pos_thres < 0.5 and i == 0:
            assert len(pos_c) > 128 and len(kept_pos) == 128
        exp_match, exp_bbox = oracle.generate_rpn_target(anchors, cls[i], boxes[i], cfg, _perm_dropping(pos_c, kept_pos),
                                                         _perm_dropping(neg_c, kept_neg))
        assert np.array_equal(ref.match[i], exp_match)                      # ... and so is the balancing
        n_pos = int((exp_match == 1).sum())
        if i < 2:
            assert n_pos > 0 and n_pos + int((exp_match == -1).sum()) == 256
        exp = exp_bbox[:n_pos] / np.asarray(cfg.DATA.BBOX_STD_DEV, np.float32)
        assert np.allclose(exp, ref.deltas[i][exp_match == 1], rtol=1e-5, atol=1e-6)
        nz = np.nonzero(exp_match)[0]
        assert np.array_equal(ra[i, :len(nz)], nz) and np.all(ra[i, len(nz):] == -1)


class _RecordedCrop(object):
    """Stands in for the GPU-only crop of the tensor branch: records the boxes and box ids it is called with."""
    last = None

    def __init__(self, h, w, extrapolation_value=0):
        self.shape = (h, w)

    def __call__(self, image, boxes, box_ind):
        _RecordedCrop.last = (boxes.clone(), box_ind.clone())
        return torch.zeros((boxes.size(0), 1) + self.shape)


@pytest.mark.parametrize("crowd,mini,ratio", [(False, True, 0.33), (True, True, 0.5), (True, False, 0.33)])
def test_det_ref_equals_the_tensor_branch(monkeypatch, crowd, mini, ratio):
    from feature_intertwiner_amd import layers as L
    monkeypatch.setattr(L, "CropAndResizeFunction", _RecordedCrop)
    b, G, P, R = 3, 14, 700, 96
    cfg = _cfg(backbone="resnet50", image_size=512, batch_size=b, train_rois_per_image=R)
    cfg.MRCNN.USE_MINI_MASK, cfg.ROIS.ROI_POSITIVE_RATIO = mini, ratio
    rs = np.random.RandomState(9)
    cls, boxes = _gt(rs, b, G, 512, [14, 9, 0], crowd)
    # coordinates on a 2^-10 grid: box centres and their differences are then exact in fp32, so the tensor branch's
    # refinements carry the roundings of the divisions and of log only, which the bar covers (with free fp32
    # coordinates the cancellation in (gcy - cy) / h alone costs up to ~3e-5 on a 0.02-high box)
    q = lambda a: (np.round(a * 1024) / 1024).astype(np.float32)
    gtn = q(boxes / 512.0)
    props = np.zeros((b, P, 4), np.float32)
    num = np.array([P, 500, 300], np.int64)
    for i in range(b):
        n = int(num[i])
        k = n // 2 if (cls[i] != 0).any() else 0
        src = gtn[i][rs.randint(0, max(int((cls[i] != 0).sum()), 1), k)]
        jit = src * (1 + 0.12 * (rs.uniform(size=(k, 4)) - 0.5)).astype(np.float32)
        y1x1 = rs.uniform(0, 0.8, (n - k, 2))
        rnd = np.concatenate([y1x1, y1x1 + rs.uniform(0.02, 0.2, (n - k, 2))], 1)
        props[i, :n] = q(np.clip(np.concatenate([jit, rnd], 0), 0, 1))[rs.permutation(n)]
    kp, kn = _unique_keys(b, P, 3), _unique_keys(b, P, 4)
    T = torch.from_numpy
    rois, ids, deltas, _ = L.det_target_from_keys(T(props), T(num), T(cls), T(gtn), torch.zeros(b, G, 56, 56), cfg, kp, kn,
                                                  kernels=False)
    mboxes, mids = _RecordedCrop.last
    ref = TR.det_targets_ref(props, num, cls, gtn, kp.numpy(), kn.numpy(), R, int(R * ratio), 1.0 / ratio, mini,
                             cfg.DATA.BBOX_STD_DEV)
    assert np.array_equal(rois.numpy().view(np.int32), ref.rois.view(np.int32))
    assert np.array_equal(ids.numpy(), ref.class_ids) and ids.dtype == torch.int32
    assert np.allclose(deltas.numpy(), ref.deltas, rtol=1e-5, atol=1e-6) and np.all(ref.deltas[ref.is_positive == 0] == 0)
    assert np.allclose(mboxes.view(b, R, 4).numpy(), ref.mask_boxes, rtol=1e-5, atol=1e-6)
    used = ref.sel >= 0
    assert np.array_equal(mids.view(b, R).numpy()[used], ref.mask_box_ids[used])
    n_pos = ref.is_positive.sum(1)
    cap = int(R * ratio)
    assert n_pos[0] == cap and n_pos[2] == 0 and (ref.sel[2] == -1).all()
    assert (ref.sel[0] >= 0).sum() == min(R, cap + int(np.floor(cap / ratio - cap)))
    if crowd:                                                               # a proposal on the crowd box is in no slot
        on = TR.iou_f32(props[0], gtn[0][1:2])[:, 0] >= np.float32(0.001)
        assert on.any() and not np.isin(np.nonzero(on)[0], ref.sel[0][int(n_pos[0]):]).any()


def test_rpn_tie_rule_by_hand():
    """12 disjoint 8x8 anchors in a row; GTs equal to anchors 2, 5, 7, 9 -> four positive candidates, eight negative ones;
    n_total = 4 keeps two of each.  Positive keys: anchor 7 highest, the others tie -> 7, then the LOWEST index 2.
    Negative keys: anchor 10 at 2.0 (the clamp's top), anchors 3 and 4 tie -> 10, then 3."""
    anchors = np.array([[0, 10 * i, 8, 10 * i + 8] for i in range(12)], np.float32)
    ids = np.array([[1, 2, 3, 4]])
    gts = anchors[[2, 5, 7, 9]][None]
    kp, kn = np.full((1, 12), 1.5, np.float32), np.full((1, 12), 1.5, np.float32)
    kp[0, 7] = 1.75
    kn[0, 10], kn[0, 3], kn[0, 4] = 2.0, 1.75, 1.75
    ref = TR.rpn_targets_ref(anchors, ids, gts, kp, kn, 0.3, 0.7, 4, EC.STD)
    assert ref.match[0].tolist() == [0, 0, 1, -1, 0, 0, 0, 1, 0, 0, -1, 0]
    assert ref.row_anchor.tolist() == [2, 3, 7, 10] and ref.row_image.tolist() == [0, 0, 0, 0]
    assert np.all(ref.deltas == 0)                                          # GT == anchor: no refinement
    assert TR.rpn_key(np.array([0.5, 1.0, 2.0, 3.0], np.float32)).tolist() == [0, 0, 0x800000, 0x800000]


def test_det_tie_rule_by_hand():
    """Proposals 0..5 equal GT 0 (class 3), 6..11 overlap nothing.  R = 6 at ratio 0.5: three positives, three negatives.
    Positive keys: 4 highest, the others tie -> 4, 0, 1.  Negative keys: 9 and 10 tie at the top -> 9, 10, then 6."""
    gts = np.array([[[0, 0, 0.5, 0.5], [0.5, 0.5, 1, 1]]], np.float32)
    ids = np.array([[3, 4]])
    props = np.array([[[0, 0, 0.5, 0.5]] * 6 + [[0.5, 0, 0.75, 0.25]] * 6], np.float32)
    kp, kn = np.full((1, 12), 1.5, np.float32), np.full((1, 12), 1.5, np.float32)
    kp[0, 4] = 1.75
    kn[0, 9] = kn[0, 10] = 1.75
    ref = TR.det_targets_ref(props, [12], ids, gts, kp, kn, 6, 3, 2.0, True, EC.STD)
    assert ref.sel[0].tolist() == [4, 0, 1, 9, 10, 6]
    assert ref.class_ids[0].tolist() == [3, 3, 3, 0, 0, 0] and ref.is_positive[0].tolist() == [1, 1, 1, 0, 0, 0]
    assert ref.mask_boxes[0, :3].tolist() == [[0, 0, 1, 1]] * 3 and np.all(ref.mask_boxes[0, 3:] == 0)
    ref = TR.det_targets_ref(props, [5], ids, gts, kp, kn, 6, 3, 2.0, True, EC.STD)         # only proposals 0..4 count
    assert ref.sel[0].tolist() == [4, 0, 1, -1, -1, -1]


@pytest.mark.parametrize("name", list(EC.RPN_CASES))
def test_rpn_edge_inputs_are_what_they_are_named_for(name):
    c, ref = EC.rpn_with_keys(name, "coarse")                  # (the margin check is part of it)
    in_tie, seen = EC.rpn_situations(c, ref)
    assert seen >= EC.RPN_SEEN[name], seen
    assert in_tie > 0 or name == "A1"                          # (one anchor cannot tie)


@pytest.mark.parametrize("name", list(EC.DET_CASES))
def test_det_edge_inputs_are_what_they_are_named_for(name):
    c = EC.det_case(name, "k16")
    EC.det_margins_hold(c)
    seen = EC.det_situations(c, EC.det_ref(c))
    assert seen >= EC.DET_SEEN[name], seen
