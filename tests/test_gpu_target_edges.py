"""GPU: the target kernels (csrc/targets.hip: fi_rpn_targets, fi_detection_targets) against tests/targets_ref.py -- a plain
NumPy restatement with every tie rule stated, which tests/test_targets_ref_cpu.py holds to the tensor formulation and the
oracle -- at the shapes where the kernels take another path (tests/target_edge_cases.py): one anchor, a partly filled
workgroup and 255 empty wavefronts, the first two-chunk wavefront (A = 16385), two trips of the four-chunk loop with a
partial chunk (A = 65637), n_total 2 / 3 / 256 / 4096, G = 1 and 256, P up to the full width of the LDS sort, R > P,
pos_cap = 0, no proposals, crowd-only images, a GT no anchor reaches, duplicate anchors and GTs, IoU exactly 0.5, and sampling
keys that tie at every selection boundary.  Discrete outputs are exact; refinements and mask boxes meet rtol 1e-5 /
atol 1e-6 against float64 (the bar of test_rpn_target_kernels_equal_the_reference_rules: the few fp32 roundings of refine()
and the one-ulp freedom of logf).  Every input keeps 1e-5 from every threshold in float64 except the designed pairs
(target_edge_cases.DESIGNED_*), and every case asserts on the reference output that what it is named for occurred."""
import ctypes

import numpy as np
import pytest
import torch

import target_edge_cases as EC
import targets_ref as TR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL, ATOL = 1e-5, 1e-6


def _cfg(**kw):
    from feature_intertwiner_amd.config import make_config
    cfg = make_config(backbone="resnet50", image_size=256, **kw)
    assert cfg.RPN.TARGET_NEG_THRES == EC.NEG_THRES and cfg.RPN.TARGET_POS_THRES == EC.POS_THRES
    assert np.array_equal(np.asarray(cfg.DATA.BBOX_STD_DEV, np.float32), EC.STD)
    return cfg


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check_rpn(c, ref, match, deltas):
    b, n_total = len(c["kinds"]), c["n_total"]
    m, d = match.cpu().numpy(), deltas.cpu().numpy()
    assert np.array_equal(m, ref.match)
    assert np.all(d[ref.match != 1] == 0)
    pos = ref.match == 1
    err = np.abs(d[pos] - ref.deltas[pos])
    print("rpn deltas: %d positives, largest error %.3g" % (pos.sum(), err.max() if err.size else 0.0))
    assert np.allclose(d[pos], ref.deltas[pos], rtol=RTOL, atol=ATOL)
    n, ri, ra = match._fi_rows
    assert n == n_total
    assert np.array_equal(ra.cpu().numpy(), ref.row_anchor) and np.array_equal(ri.cpu().numpy(), ref.row_image)


@pytest.mark.parametrize("name,keys", [(n, k) for n in EC.RPN_CASES for k in ("unique", "coarse")] +
                         [("A16385", "equal"), ("A65637", "equal"), ("A65637_n4096", "equal")])
def test_rpn_target_kernels_at_edge_shapes(name, keys):
    from feature_intertwiner_amd import layers as L
    c, ref = EC.rpn_with_keys(name, keys)                      # (asserts the margins from the thresholds)
    in_tie, seen = EC.rpn_situations(c, ref)
    assert seen >= EC.RPN_SEEN[name], seen
    if keys != "unique" and name != "A1":                      # (one anchor cannot tie)
        assert in_tie > 0                                      # a selection boundary fell inside a run of equal keys
    if keys == "equal":                                        # the kept set: the first candidates in anchor order
        for i, (cand, _, _) in enumerate(c["cands"]):
            pos_c = np.nonzero(cand == 1)[0]
            kept = np.nonzero(ref.match[i] == 1)[0]
            assert np.array_equal(kept, pos_c[:len(kept)])
    cfg = _cfg()
    cfg.RPN.TRAIN_ANCHORS_PER_IMAGE = c["n_total"]
    match, deltas = L.rpn_target_from_keys(T(c["anchors"]), T(c["ids"]), T(c["gts"]), cfg, T(c["kp"]), T(c["kn"]), kernels=True)
    torch.cuda.synchronize()
    assert getattr(match, "_fi_rows", None) is not None        # the kernels ran
    _check_rpn(c, ref, match, deltas)


def _det_c_entry(c, rois_per_image=None, n_proposals=None, max_gt=None, out=None):
    """fi_detection_targets through its C entry; returns (status, outputs as in DetTargets order without sel)."""
    from feature_intertwiner_amd import _lib
    L = _lib.load()
    b, P, G = c["props"].shape[0], c["P"], c["G"]
    R = c["R"] if rois_per_image is None else rois_per_image
    if out is None:
        out = [torch.empty((b, R, 4), device=DEV), torch.empty((b, R), device=DEV, dtype=torch.int32),
               torch.empty((b, R, 4), device=DEV), torch.empty((b, R, 4), device=DEV),
               torch.empty((b, R), device=DEV, dtype=torch.int32), torch.empty((b, R), device=DEV)]
    ins = [T(c["props"]), T(c["num"]), T(c["ids"]), T(c["gts"]), T(c["kp"]), T(c["kn"])]
    std = (ctypes.c_float * 4)(*[float(v) for v in EC.STD])
    with torch.cuda.device(DEV):
        rc = L.fi_detection_targets(*[_lib.ptr(t) for t in ins], b, P if n_proposals is None else n_proposals,
                                    G if max_gt is None else max_gt, R, c["pos_cap"], c["npp"], 1 if c["mini"] else 0, std,
                                    *[_lib.ptr(t) for t in out], _lib.current_stream())
    torch.cuda.synchronize()
    return rc, out


def _check_det(c, ref, rois, ids, deltas, what):
    used = ref.sel >= 0
    rois, ids, deltas = rois.cpu().numpy(), ids.cpu().numpy(), deltas.cpu().numpy()
    for i, r in zip(*np.nonzero((rois.view(np.int32) != ref.rois.view(np.int32)).any(2))):
        print("%s: image %d slot %d holds %s, expected proposal %d = %s" % (what, i, r, rois[i, r], ref.sel[i, r], ref.rois[i, r]))
    # the proposal in every slot, bitwise; unused slots all-zero
    assert np.array_equal(rois.view(np.int32), ref.rois.view(np.int32)), what
    for i in range(len(rois)):
        assert np.array_equal(rois[i][used[i]].view(np.int32), c["props"][i][ref.sel[i][used[i]]].view(np.int32)), what
    assert np.all(rois.view(np.int32)[~used] == 0) and np.all(deltas.view(np.int32)[ref.is_positive == 0] == 0), what
    assert ids.dtype == np.int32 and np.array_equal(ids, ref.class_ids), what
    assert np.allclose(deltas, ref.deltas, rtol=RTOL, atol=ATOL), what


@pytest.mark.parametrize("name,keys", [(n, k) for n in EC.DET_CASES for k in ("unique", "k16", "equal")])
def test_detection_target_kernel_at_edge_shapes(name, keys):
    from feature_intertwiner_amd import layers as L
    c = EC.det_case(name, keys)
    EC.det_margins_hold(c)
    ref = EC.det_ref(c)
    seen = EC.det_situations(c, ref)
    assert seen >= EC.DET_SEEN[name], seen
    b, R, G = len(c["kinds"]), c["R"], c["G"]
    used, isp = ref.sel >= 0, ref.is_positive == 1
    # the C entry: every output, slot by slot
    rc, (rois, ids, deltas, mboxes, mids, is_pos) = _det_c_entry(c)
    assert rc == 0
    _check_det(c, ref, rois, ids, deltas, "C entry")
    mboxes, mids, is_pos = mboxes.cpu().numpy(), mids.cpu().numpy(), is_pos.cpu().numpy()
    assert np.array_equal(is_pos, ref.is_positive)
    assert np.array_equal(mids[isp], ref.mask_box_ids[isp])
    # (every other slot: some mask of its own image -- the crop reads it, and the result is multiplied by is_positive)
    first = (np.arange(b) * G)[:, None]
    assert np.all((mids >= first) & (mids < first + G))
    assert np.all(mboxes.view(np.int32)[~isp] == 0)
    err = np.abs(mboxes[isp] - ref.mask_boxes[isp])
    print("mask boxes: %d positives, largest error %.3g" % (isp.sum(), err.max() if err.size else 0.0))
    assert np.allclose(mboxes, ref.mask_boxes, rtol=RTOL, atol=ATOL)
    # the wrapper
    cfg = _cfg(train_rois_per_image=R)
    cfg.ROIS.ROI_POSITIVE_RATIO, cfg.MRCNN.USE_MINI_MASK = c["ratio"], c["mini"]
    masks = (torch.rand(b, G, 56, 56, generator=torch.Generator().manual_seed(1)) > 0.5).float().to(DEV)
    w_rois, w_ids, w_deltas, w_mask = L.det_target_from_keys(T(c["props"]), T(c["num"]), T(c["ids"]), T(c["gts"]), masks, cfg,
                                                             T(c["kp"]), T(c["kn"]), kernels=True)
    torch.cuda.synchronize()
    _check_det(c, ref, w_rois, w_ids, w_deltas, "wrapper")
    w_mask = w_mask.cpu().numpy()
    assert w_mask.shape == (b, R, 28, 28) and np.all(w_mask[~isp] == 0) and np.all((w_mask == 0) | (w_mask == 1))


def test_mask_targets_of_constant_mini_masks():
    """Mini-masks constant per GT (all ones / all zeros), positives = shrunken copies strictly inside their GT box: every
    positive's 28x28 target is its GT's constant, every other slot's is zero.  A wrong mask_box_id, a mask box outside
    [0, 1] or a wrong is_positive shows here."""
    from feature_intertwiner_amd import layers as L
    b, G, P, R = 3, 9, 64, 64
    rs = np.random.RandomState(4)
    gts = np.array([[(4 + 20 * r) / 64, (4 + 20 * q) / 64, (20 + 20 * r) / 64, (20 + 20 * q) / 64]
                    for r in range(3) for q in range(3)], np.float32)          # 3 x 3 disjoint 16/64 boxes
    gts = np.stack([gts[rs.permutation(G)] for _ in range(b)])
    ids = rs.randint(1, 81, (b, G)).astype(np.int64)
    ids[1, 6:] = 0
    const = rs.randint(0, 2, (b, G)).astype(np.float32)
    const[:, 0], const[:, 1] = 1, 0
    props = np.zeros((b, P, 4), np.float32)
    for i in range(b):
        g = rs.randint(0, 6, P)
        shrink = rs.randint(1, 3, (P, 4)) / 64.0 * np.array([1, 1, -1, -1])
        props[i] = gts[i][g] + shrink                                           # IoU >= (12 / 16)^2 > 0.5
        far = rs.uniform(size=P) < 0.4
        props[i][far] = (62 / 64, 1 / 64, 63 / 64, 3 / 64)                       # background
    num = np.array([P, P - 17, P], np.int64)
    c = dict(props=props, num=num, ids=ids, gts=gts, kp=EC.det_keys("k16", b, P, 5), kn=EC.det_keys("k16", b, P, 6), P=P, G=G,
             R=R, ratio=0.5, pos_cap=32, npp=2.0, mini=True, kinds=["rich"] * b, keys="k16")
    for i in range(b):
        assert EC._far_from(TR.iou_f64(gts[i][ids[i] > 0], props[i]), (0.5,)).all()
    ref = EC.det_ref(c)
    isp = ref.is_positive == 1
    assert isp.sum(1).min() > 5 and (ref.sel[isp] >= 0).all()
    want = np.zeros((b, R), np.float32)
    for i in range(b):
        want[i][isp[i]] = const[i][ref.mask_box_ids[i][isp[i]] - i * G]
    assert (want[isp] == 1).any() and (want[isp] == 0).any()
    cfg = _cfg(train_rois_per_image=R)
    cfg.ROIS.ROI_POSITIVE_RATIO = 0.5
    masks = T(const)[:, :, None, None].expand(b, G, 56, 56).contiguous()
    rois, cls, deltas, tmask = L.det_target_from_keys(T(props), T(num), T(ids), T(gts), masks, cfg, T(c["kp"]), T(c["kn"]),
                                                      kernels=True)
    torch.cuda.synchronize()
    _check_det(c, ref, rois, cls, deltas, "wrapper")
    tmask = tmask.cpu().numpy()
    assert np.array_equal(tmask, np.broadcast_to(want[:, :, None, None], tmask.shape))


# ---------------------------------------------------------------------------------------------------------------
# limits
# ---------------------------------------------------------------------------------------------------------------
def test_c_entries_refuse_sizes_past_their_limits_and_write_nothing():
    from feature_intertwiner_amd import _lib
    L = _lib.load()
    c = EC.det_case("P2", "unique")
    b, R = len(c["kinds"]), c["R"]
    for kw in (dict(max_gt=257), dict(n_proposals=2049)):
        out = [torch.full((b, R, 4), 7.0, device=DEV), torch.full((b, R), 7, device=DEV, dtype=torch.int32),
               torch.full((b, R, 4), 7.0, device=DEV), torch.full((b, R, 4), 7.0, device=DEV),
               torch.full((b, R), 7, device=DEV, dtype=torch.int32), torch.full((b, R), 7.0, device=DEV)]
        rc, out = _det_c_entry(c, out=out, **kw)
        assert rc != 0, kw
        assert all(bool((t == 7).all()) for t in out), kw
    A, G = 64, 4
    anchors, ids, gts = T(EC.synth_anchors(A)), torch.ones(1, 257, dtype=torch.int64, device=DEV), torch.zeros(1, 257, 4, device=DEV)
    kp, kn = T(EC.rpn_keys("unique", 1, A, 1)), T(EC.rpn_keys("unique", 1, A, 2))
    std = (ctypes.c_float * 4)(*[float(v) for v in EC.STD])
    ws = torch.empty(int(L.fi_rpn_targets_workspace_bytes(1, A, 257)) // 4 + 1, device=DEV)
    for max_gt, n_total in ((257, 256), (G, 1), (G, 4097)):
        match, deltas = torch.full((1, A), 7.0, device=DEV), torch.full((1, A, 4), 7.0, device=DEV)
        ri, ra = (torch.full((4097,), 7, dtype=torch.int64, device=DEV) for _ in range(2))
        with torch.cuda.device(DEV):
            rc = L.fi_rpn_targets(_lib.ptr(anchors), _lib.ptr(ids), _lib.ptr(gts), _lib.ptr(kp), _lib.ptr(kn), 1, A, max_gt,
                                  EC.NEG_THRES, EC.POS_THRES, n_total, std, _lib.ptr(match), _lib.ptr(deltas), _lib.ptr(ri),
                                  _lib.ptr(ra), _lib.ptr(ws), _lib.current_stream())
        torch.cuda.synchronize()
        assert rc != 0, (max_gt, n_total)
        assert all(bool((t == 7).all()) for t in (match, deltas, ri, ra)), (max_gt, n_total)


def test_wrappers_fall_back_to_the_tensor_formulation_past_the_limits():
    """G = 257 (both wrappers) and P = 2049: the tensor formulation runs and, on unique keys and without IoU ties among
    GTs or anchors (asserted), agrees with the reference."""
    from feature_intertwiner_amd import layers as L
    c = EC.rpn_fallback_case()
    ref = TR.rpn_targets_ref(c["anchors"], c["ids"], c["gts"], c["kp"], c["kn"], EC.NEG_THRES, EC.POS_THRES, c["n_total"], EC.STD)
    assert (ref.match == 1).sum() > 20
    cfg = _cfg()
    match, deltas = L.rpn_target_from_keys(T(c["anchors"]), T(c["ids"]), T(c["gts"]), cfg, T(c["kp"]), T(c["kn"]), kernels=True)
    assert getattr(match, "_fi_rows", None) is None            # not the kernels
    assert np.array_equal(match.cpu().numpy(), ref.match)
    d = deltas.cpu().numpy()
    assert np.all(d[ref.match != 1] == 0) and np.allclose(d, ref.deltas, rtol=RTOL, atol=ATOL)
    for name in ("G257", "P2049"):
        c = EC.det_fallback_case(name)
        ref = EC.det_ref(c)
        assert ref.is_positive.sum() > 20
        cfg = _cfg(train_rois_per_image=c["R"])
        cfg.ROIS.ROI_POSITIVE_RATIO = c["ratio"]
        b, G = c["ids"].shape
        rois, ids, deltas, tmask = L.det_target_from_keys(T(c["props"]), T(c["num"]), T(c["ids"]), T(c["gts"]),
                                                          torch.ones(b, G, 56, 56, device=DEV), cfg, T(c["kp"]), T(c["kn"]),
                                                          kernels=True)
        _check_det(c, ref, rois, ids, deltas, name)
        assert np.all(tmask.cpu().numpy()[ref.is_positive == 0] == 0)
