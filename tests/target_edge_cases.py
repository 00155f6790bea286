"""Inputs of tests/test_gpu_target_edges.py, built on the CPU so that tests/test_targets_ref_cpu.py can hold them to what
they are named for without a GPU.  Anchors are synthetic (boxes with sides 8..64 on a 128-pixel canvas, tiled with
quarter-pixel shifts and shuffled); GT coordinates are multiples of 1/4 pixel (RPN) or 1/64 (normalised proposals), so
the designed exact-threshold pairs are exact in fp32.  Every generated box is re-drawn until its float64 IoU with every
box it is compared with lies further than MARGIN from every threshold it is compared with; the designed pairs are exempt
and named (DESIGNED_*)."""
import functools

import numpy as np

import targets_ref as TR

MARGIN = 1e-5
NEG_THRES, POS_THRES = 0.3, 0.7
STD = np.array([0.1, 0.1, 0.2, 0.2], np.float32)

# the only pairs that sit on a threshold on purpose
DESIGNED_RPN = ()                                    # (none: the RPN cases have IoU exactly 1 and 0.25 pairs, on no threshold)
DESIGNED_DET = ("proposal 0 = the upper half of GT 0: IoU exactly 0.5, positive",)


# ---------------------------------------------------------------------------------------------------------------
# RPN
# ---------------------------------------------------------------------------------------------------------------
def synth_anchors(A, seed=0):
    base = []
    for h, w in ((8, 8), (16, 16), (32, 32), (64, 64), (8, 16), (16, 8), (16, 32), (32, 16), (32, 64), (64, 32)):
        for y in np.arange(0, 128 - h + 1, h / 2):
            for x in np.arange(0, 128 - w + 1, w / 2):
                base.append((y, x, y + h, x + w))
    base = np.array(base, np.float64)
    copies = -(-A // len(base))
    tiled = np.concatenate([base + np.array([0.25 * k, 0.25 * ((5 * k) % 32)] * 2) for k in range(copies)])
    out = tiled[np.random.RandomState(seed).permutation(len(tiled))][:A].astype(np.float32)
    assert out.shape == (A, 4)
    return out


def _far_from(iou64, thresholds):
    return np.all([np.abs(iou64 - t).min(0) > MARGIN for t in thresholds], 0)


def _draw_gt(rs, anchors, n, near, crowd=False, lo=0.0, hi=136.0, src=None):
    """n quarter-pixel boxes: copies of random anchors (of src, if given) shifted by up to a pixel (near) or free boxes
    with sides 8..64."""
    src = anchors if src is None else src
    out = np.zeros((0, 4), np.float32)
    thresholds = (0.001,) if crowd else (NEG_THRES, POS_THRES)
    while len(out) < n:
        m = 2 * (n - len(out)) + 4
        if near:
            bx = src[rs.randint(0, len(src), m)].astype(np.float64) + np.tile(rs.randint(-4, 5, (m, 2)) / 4.0, (1, 2))
        else:
            hw = rs.randint(32, 257, (m, 2)) / 4.0
            y1x1 = np.floor(rs.uniform(lo, hi - hw) * 4) / 4.0
            bx = np.concatenate([y1x1, y1x1 + hw], 1)
        bx = bx.astype(np.float32)
        out = np.concatenate([out, bx[_far_from(TR.iou_f64(anchors, bx), thresholds)]])
    return out[:n]


def _pad(G, ids, boxes):
    i, b = np.zeros(G, np.int64), np.zeros((G, 4), np.float32)
    i[:len(ids)], b[:len(ids)] = ids, boxes
    return i, b


def _tiny_claims(anchors, want, G):
    """4x4 boxes on a 4-pixel grid, each below every threshold with every anchor (IoU <= 0.25), taken one by one until
    they claim exactly `want` distinct anchors: an image with exactly `want` positive candidates."""
    boxes, claimed = [], set()
    for y in range(0, 128, 4):
        for x in range(0, 128, 4):
            if len(claimed) == want:
                break
            bx = np.array([[y, x, y + 4, x + 4]], np.float32)
            iou = TR.iou_f32(anchors, bx)[:, 0]
            a = int(np.argmax(iou))
            if a not in claimed and len(boxes) < G and iou.max() > 0:
                claimed.add(a)
                boxes.append(bx[0])
    assert len(claimed) == want, "cannot place %d single-claim GTs" % want
    return np.ones(len(boxes), np.int64), np.array(boxes, np.float32)


def rpn_image(kind, rs, anchors, G, n_total):
    A = len(anchors)
    cls = lambda n: rs.randint(1, 81, n)
    if kind == "valid":                      # G valid boxes, half of them near an anchor: many positives
        k = G // 2
        return _pad(G, cls(G), np.concatenate([_draw_gt(rs, anchors, G - k, True), _draw_gt(rs, anchors, k, False)]))
    if kind == "valid_near":                 # G valid boxes, all near an anchor: many positives
        return _pad(G, cls(G), _draw_gt(rs, anchors, G, True))
    if kind == "valid_big":                  # G valid boxes, all near an anchor with sides >= 16: many positives per GT
        big = anchors[np.minimum(anchors[:, 2] - anchors[:, 0], anchors[:, 3] - anchors[:, 1]) >= 16]
        return _pad(G, cls(G), _draw_gt(rs, anchors, G, True, src=big))
    if kind == "equal":                      # a GT equal to an anchor (IoU 1) [+ free boxes]
        bx = np.concatenate([anchors[A // 2][None], _draw_gt(rs, anchors, min(G - 1, 3), False)])
        return _pad(G, cls(len(bx)), bx)
    if kind == "none":
        return _pad(G, [], np.zeros((0, 4), np.float32))
    if kind == "crowd_only":
        n = min(G, 2)
        return _pad(G, -np.ones(n, np.int64), _draw_gt(rs, anchors, n, False, crowd=True))
    if kind == "half_crowd":                 # a crowd box over the left half of the canvas, valid boxes on the right
        crowd = np.array([[-8, -8, 144, 64]], np.float32)
        assert _far_from(TR.iou_f64(anchors, crowd), (0.001,)).all()
        n = min(G - 1, 6)
        return _pad(G, np.concatenate([[-1], cls(n)]), np.concatenate([crowd, _draw_gt(rs, anchors, n, False, lo=64.0)]))
    if kind == "few":                        # a crowd box over everything and one valid box: fewer candidates than n_total
        crowd = np.array([[-8, -8, 144, 144]], np.float32)
        assert _far_from(TR.iou_f64(anchors, crowd), (0.001,)).all()
        return _pad(G, [7, -1], np.concatenate([_draw_gt(rs, anchors, 1, True), crowd]))
    if kind == "unreachable":                # one valid GT no anchor overlaps: it claims anchor 0
        return _pad(G, [5], np.array([[300, 300, 320, 324]], np.float32))
    if kind == "dup_gt":                     # two identical valid GTs [+ free boxes]
        one = _draw_gt(rs, anchors, 1, True)
        bx = np.concatenate([one, one, _draw_gt(rs, anchors, min(G - 2, 2), False)])
        return _pad(G, cls(len(bx)), bx)
    if kind == "exact":                      # exactly n_total // 2 positive candidates
        return _pad(G, *_tiny_claims(anchors, n_total // 2, G))
    if kind == "dup_anchor":                 # anchors 1 and A - 1 are the same 6x6 box, the best of a 4x4 GT inside them
        return _pad(G, [9], np.array([[201, 201, 205, 205]], np.float32))
    raise KeyError(kind)


def rpn_keys(mode, b, A, seed):
    rs = np.random.RandomState(seed)
    u = np.stack([(rs.permutation(A) + 0.5) / A for _ in range(b)])
    if mode == "unique":
        k = (1.0 + u).astype(np.float32)
        assert all(len(np.unique(r)) == A for r in k)
    elif mode == "coarse":                   # 64 distinct values, a block equal to 1.0, a few equal to 2.0
        k = (1.0 + np.floor(u * 64) / 64).astype(np.float32)
        k[:, A // 3:A // 3 + max(A // 8, 1)] = 1.0
        k[:, :3] = 2.0
        k[:, A - 1] = 2.0
    else:
        k = np.full((b, A), 1.5, np.float32)
    return k


# name -> (A, n_total, G, image kinds)
RPN_CASES = {
    "A1": (1, 2, 1, ("equal", "none", "crowd_only")),
    "A65": (65, 3, 4, ("valid", "exact", "unreachable", "dup_gt")),
    "A257": (257, 256, 256, ("valid", "half_crowd", "none", "few")),
    "A16384": (16384, 256, 130, ("valid", "exact", "half_crowd", "dup_anchor")),
    "A16385": (16385, 4096, 256, ("valid_near", "few", "dup_gt", "equal")),
    "A65637": (65537 + 100, 256, 256, ("valid", "exact", "unreachable")),
    "A65637_n4096": (65537 + 100, 4096, 256, ("valid_big", "half_crowd", "none")),
}


# what the images of every case must contain: "more" positive candidates than n_total // 2, "exact"ly n_total // 2 of
# them, fewer candidates than n_total ("padded" rows), all n_total rows "filled"
RPN_SEEN = {"A1": {"padded"}, "A65": {"more", "exact", "filled"}, "A257": {"more", "padded", "filled"},
            "A16384": {"more", "exact", "filled"}, "A16385": {"padded", "filled"}, "A65637": {"more", "exact", "filled"},
            "A65637_n4096": {"more", "filled"}}


@functools.lru_cache(maxsize=2)
def rpn_geometry(name):
    """Anchors, GTs, the margin check and the candidate classes of a case: shared by its key modes."""
    c = rpn_case(name)
    rpn_margins_hold(c)
    c["cands"] = [TR.rpn_candidates(c["anchors"], i, g, NEG_THRES, POS_THRES) for i, g in zip(c["ids"], c["gts"])]
    return c


def rpn_with_keys(name, keys):
    """The case with sampling keys of one mode and its reference output."""
    c = dict(rpn_geometry(name))
    b, A = c["ids"].shape[0], len(c["anchors"])
    c["keys"], c["kp"], c["kn"] = keys, rpn_keys(keys, b, A, 1), rpn_keys(keys, b, A, 2)
    ref = TR.rpn_targets_ref(c["anchors"], c["ids"], c["gts"], c["kp"], c["kn"], NEG_THRES, POS_THRES, c["n_total"], STD,
                             candidates=c["cands"])
    return c, ref


def rpn_case(name):
    A, n_total, G, kinds = RPN_CASES[name]
    rs = np.random.RandomState(17)
    anchors = synth_anchors(A)
    if "dup_anchor" in kinds:
        anchors[1] = anchors[A - 1] = (200, 200, 206, 206)
    imgs = [rpn_image(k, rs, anchors, G, n_total) for k in kinds]
    ids, gts = np.stack([i for i, _ in imgs]), np.stack([g for _, g in imgs])
    return dict(name=name, kinds=kinds, anchors=anchors, ids=ids, gts=gts, n_total=n_total)


def rpn_margins_hold(c):
    """Every IoU the kernels compare with a threshold lies further than MARGIN from it, in float64."""
    for ids, gts in zip(c["ids"], c["gts"]):
        valid = gts[ids > 0]
        for g in range(0, len(valid), 32):
            assert _far_from(TR.iou_f64(c["anchors"], valid[g:g + 32]), (NEG_THRES, POS_THRES)).all()
        if (ids < 0).any():
            assert _far_from(TR.iou_f64(c["anchors"], gts[ids < 0]), (0.001,)).all()


def boundary_in_tie(key, cand, keep):
    """The selection of `keep` of the candidates `cand` cuts through a run of equal keys."""
    if not 0 < keep < len(cand):
        return False
    k = np.sort(key[cand])[::-1]
    return bool(k[keep - 1] == k[keep])


def rpn_situations(c, ref):
    """Assert, on the reference output, that every image of the case is what its kind says.  Returns the number of
    selection boundaries that fell inside a run of equal keys."""
    n_total, A = c["n_total"], len(c["anchors"])
    ra = ref.row_anchor.reshape(len(c["kinds"]), n_total)
    in_tie = 0
    seen = set()
    for i, kind in enumerate(c["kinds"]):
        cand, arg, vv = c["cands"][i]
        pos_c, neg_c = np.nonzero(cand == 1)[0], np.nonzero(cand == -1)[0]
        n_pos, n_neg = int((ref.match[i] == 1).sum()), int((ref.match[i] == -1).sum())
        in_tie += boundary_in_tie(TR.rpn_key(c["kp"][i]), pos_c, n_pos) + boundary_in_tie(TR.rpn_key(c["kn"][i]), neg_c, n_neg)
        if len(pos_c) > n_total // 2:
            seen.add("more")
        if len(pos_c) + len(neg_c) < n_total:
            seen.add("padded")
            assert (ra[i] == -1).any()
        elif n_pos + n_neg == n_total and (ra[i] >= 0).all():
            seen.add("filled")
        if kind in ("valid", "valid_near", "valid_big"):
            assert (c["ids"][i] > 0).all() and n_pos > 0
        elif kind == "equal":
            assert vv.max() == 1.0 and ref.match[i, A // 2] == 1 and np.all(ref.deltas[i, A // 2] == 0)
        elif kind in ("none", "crowd_only"):
            assert n_pos == 0 and len(pos_c) == 0
            if kind == "crowd_only":
                assert (c["ids"][i] < 0).any() and not (c["ids"][i] > 0).any()
        elif kind == "half_crowd":
            under = TR.iou_f32(c["anchors"], c["gts"][i][:1])[:, 0] >= np.float32(0.001)
            assert (cand[under] != -1).all() and (A < 64 or (under.any() and (cand[~under] == -1).any()))
        elif kind == "few":
            assert len(pos_c) + len(neg_c) < n_total and (ra[i] == -1).any()
        elif kind == "unreachable":
            assert vv.max() == 0 and cand[0] == 1 and ref.match[i, 0] == 1 and len(pos_c) == 1
        elif kind == "dup_gt":
            assert np.array_equal(c["gts"][i][0], c["gts"][i][1]) and (arg != 1).all()
        elif kind == "exact":
            assert len(pos_c) == n_total // 2 and n_pos == n_total // 2
            seen.add("exact")
        elif kind == "dup_anchor":
            assert np.array_equal(c["anchors"][1], c["anchors"][A - 1])
            assert cand[1] == 1 and cand[A - 1] == 0 and ref.match[i, 1] == 1 and len(pos_c) == 1
    return in_tie, seen


# ---------------------------------------------------------------------------------------------------------------
# detection
# ---------------------------------------------------------------------------------------------------------------
def _grid_boxes(rs, n, lo, hi, smin=6, smax=40):
    hw = rs.randint(smin, smax + 1, (n, 2))
    y1x1 = np.floor(rs.uniform(lo * 64, hi * 64 - hw))
    return (np.concatenate([y1x1, y1x1 + hw], 1) / 64.0).astype(np.float32)


def det_image(kind, rs, P, G):
    """(ids [G], gts [G, 4], proposals [P, 4]).  Slot 0: a valid GT alone in the corner [0.75, 1]^2; with G >= 4 slot 1 is
    a crowd box alone in [0.75, 1] x [0, 0.25] and slots 2, 3 are one box with two classes; the rest lie in [0, 0.72]^2.
    Proposal 0 is the upper half of GT 0 (IoU exactly 0.5), proposal 1 the crowd box, proposal 2 the box of slots 2, 3."""
    ids, gts = np.zeros(G, np.int64), np.zeros((G, 4), np.float32)
    gts[0], ids[0] = (50 / 64, 50 / 64, 62 / 64, 62 / 64), 11
    if G >= 4:
        gts[1], ids[1] = (50 / 64, 2 / 64, 62 / 64, 14 / 64), -1
        gts[2] = gts[3] = _grid_boxes(rs, 1, 0.0, 0.72, 12, 30)[0]
        ids[2], ids[3] = 21, 22
        for g in range(4, G):                    # (proposal 2 = the box of slots 2, 3 keeps its margin from these too)
            while True:
                gts[g] = _grid_boxes(rs, 1, 0.0, 0.72)[0]
                if _far_from(TR.iou_f64(gts[g:g + 1], gts[2:3]), (0.5,)).all():
                    break
        ids[4:] = rs.randint(1, 81, G - 4)
    if kind == "none":
        ids[:] = 0
    elif kind == "crowd_only":
        ids[ids != 0] = -1
    valid, crowd = gts[ids > 0], gts[ids < 0]
    src = gts[ids != 0] if (ids != 0).any() else gts
    frac = {"rich": 0.6, "negpoor": 0.97}.get(kind, 0.5)
    props = np.zeros((0, 4), np.float32)
    while len(props) < P:
        m = 2 * (P - len(props)) + 8
        cp = src[rs.randint(0, len(src), m)] + rs.randint(-2, 3, (m, 4)).astype(np.float32) / 64
        p = np.where(rs.uniform(size=(m, 1)) < frac, cp, _grid_boxes(rs, m, 0.0, 1.0, 3, 30)).astype(np.float32)
        ok = (p[:, 2] > p[:, 0]) & (p[:, 3] > p[:, 1])
        if len(valid):
            ok &= _far_from(TR.iou_f64(valid, p), (0.5,))
        if len(crowd):
            ok &= _far_from(TR.iou_f64(crowd, p), (0.001,))
        props = np.concatenate([props, p[ok]])
    props = np.ascontiguousarray(props[:P])
    designed = [(50 / 64, 50 / 64, 56 / 64, 62 / 64)] + ([gts[1], gts[2]] if G >= 4 else [])
    for j, d in enumerate(designed[:P]):
        props[j] = d
    return ids, gts, props


def det_keys(mode, b, P, seed):
    rs = np.random.RandomState(seed)
    u = np.stack([(rs.permutation(P) + 0.5) / P for _ in range(b)])
    if mode == "unique":
        return (1.0 + u).astype(np.float32)
    if mode == "k16":
        return (1.0 + np.floor(u * 16) / 16).astype(np.float32)
    return np.full((b, P), 1.25, np.float32)


# name -> (P, R, ROI_POSITIVE_RATIO, G, USE_MINI_MASK, ((image kind, num_proposals), ...)); num -17 means P - 17
DET_CASES = {
    "P1_cap0": (1, 1, 0.33, 1, True, (("rich", 1), ("rich", 0), ("none", 1))),
    "P2": (2, 3, 0.5, 1, False, (("rich", 2), ("rich", 1), ("none", 2), ("rich", 0))),
    "P1023": (1023, 64, 0.33, 256, True, (("rich", 1023), ("negpoor", -17), ("crowd_only", 1023), ("rich", 1))),
    "P1024": (1024, 512, 1.0, 16, False, (("rich", 1024), ("none", -17), ("rich", 0), ("negpoor", 1024))),
    "P1025": (1025, 64, 0.5, 16, True, (("negpoor", 1025), ("rich", -17), ("crowd_only", 1), ("none", 1025))),
    "P2047": (2047, 3000, 0.33, 16, False, (("rich", 2047), ("negpoor", 2047), ("rich", -17), ("rich", 0))),
    "P2048": (2048, 3000, 0.5, 256, True, (("rich", 2048), ("negpoor", -17), ("crowd_only", 2048), ("none", 2048))),
    "P2048_R512": (2048, 512, 0.33, 16, True, (("rich", 2048), ("rich", -17), ("negpoor", 2048), ("rich", 1))),
}


DET_SEEN = {
    "P1_cap0": {"cap0", "half", "none", "num0", "zero_slots"},
    "P2": {"half", "negpoor", "none", "num0", "zero_slots"},
    "P1023": {"capped", "dup_gt_selected", "crowd_only", "half", "negpoor", "on_crowd", "zero_slots"},
    "P1024": {"capped", "dup_gt_selected", "half", "none", "num0", "on_crowd", "zero_slots", "no_negatives"},
    "P1025": {"capped", "dup_gt_selected", "crowd_only", "half", "none", "on_crowd", "zero_slots"},
    "P2047": {"capped", "dup_gt_selected", "half", "negpoor", "num0", "on_crowd", "zero_slots"},
    "P2048": {"capped", "dup_gt_selected", "crowd_only", "half", "negpoor", "none", "on_crowd", "zero_slots"},
    "P2048_R512": {"capped", "dup_gt_selected", "half", "negpoor", "on_crowd", "zero_slots"},
}


def det_case(name, keys):
    P, R, ratio, G, mini, images = DET_CASES[name]
    rs = np.random.RandomState(23)
    kinds = [k for k, _ in images]
    num = np.array([P + n if n < 0 else n for _, n in images], np.int64)
    assert (num >= 0).all() and (num <= P).all()
    imgs = [det_image(k, rs, P, G) for k in kinds]
    b = len(imgs)
    kp, kn = det_keys(keys, b, P, 3), det_keys(keys, b, P, 4)
    if P >= 3:                                   # proposal 2 (the box of GT slots 2, 3) holds the row's largest positive key:
        for row in kp:                           # wherever it is a candidate it is in a slot, and its class is looked at
            top = int(np.argmax(row))
            row[2], row[top] = row[top], row[2]
    return dict(name=name, keys=keys, kinds=kinds, P=P, R=R, ratio=ratio, G=G, mini=mini, num=num,
                ids=np.stack([i[0] for i in imgs]), gts=np.stack([i[1] for i in imgs]),
                props=np.stack([i[2] for i in imgs]), kp=kp, kn=kn, pos_cap=int(R * ratio), npp=1.0 / ratio)


def det_ref(c):
    return TR.det_targets_ref(c["props"], c["num"], c["ids"], c["gts"], c["kp"], c["kn"], c["R"], c["pos_cap"], c["npp"],
                              c["mini"], STD)


def det_margins_hold(c):
    for i in range(len(c["kinds"])):
        ids, gts, props = c["ids"][i], c["gts"][i], c["props"][i]
        if (ids > 0).any():
            far = _far_from(TR.iou_f64(gts[ids > 0], props), (0.5,))
            if ids[0] > 0:
                far[0] = True                                  # DESIGNED_DET
                assert TR.iou_f32(props[:1], gts[:1])[0, 0] == np.float32(0.5)
            assert far.all()
        if (ids < 0).any():
            assert _far_from(TR.iou_f64(gts[ids < 0], props), (0.001,)).all()


def det_situations(c, ref):
    """Assert on the reference output that the case contains what it is named for; returns what was seen."""
    P, R, G = c["P"], c["R"], c["G"]
    seen = set()
    for i, kind in enumerate(c["kinds"]):
        num = int(c["num"][i])
        pos_c, neg_c, arg = TR.det_candidates(c["props"][i], num, c["ids"][i], c["gts"][i])
        n_pos = int(ref.is_positive[i].sum())
        n_used = int((ref.sel[i] >= 0).sum())
        n_neg = n_used - n_pos
        neg_want = int(np.floor(c["npp"] * n_pos - n_pos))
        if c["keys"] != "unique":
            kp = c["kp"][i].view(np.uint32).astype(np.int64)
            kn = c["kn"][i].view(np.uint32).astype(np.int64)
            if boundary_in_tie(kp, pos_c, n_pos) or boundary_in_tie(kn, neg_c, n_neg):
                seen.add("tie")
        if num == 0:
            assert n_used == 0
            seen.add("num0")
        if kind in ("none", "crowd_only"):
            assert n_pos == 0 and n_used == 0 and len(pos_c) == 0
            seen.add(kind)
            if kind == "crowd_only" and num > 1:
                assert len(neg_c) < num              # proposals on a crowd box are no negatives either
        if len(pos_c) > c["pos_cap"]:
            seen.add("capped")
            assert n_pos == c["pos_cap"]
        if c["pos_cap"] == 0:
            seen.add("cap0")
        if n_pos and len(neg_c) < min(neg_want, R - n_pos):
            seen.add("negpoor")
            assert n_neg == len(neg_c)
        if n_used < R:
            seen.add("zero_slots")
        if c["ratio"] == 1.0 and n_pos:
            assert n_neg == 0                        # ROI_POSITIVE_RATIO 1: no negatives are wanted
            seen.add("no_negatives")
        if c["ids"][i, 0] > 0 and num >= 1:
            assert 0 in pos_c                        # IoU exactly 0.5 is positive
            seen.add("half")
        if G >= 4 and c["ids"][i, 1] < 0 and c["ids"][i, 0] > 0 and num >= 2:
            assert 1 not in pos_c and 1 not in neg_c  # on a crowd box, best IoU below 0.5: neither
            seen.add("on_crowd")
        if G >= 4 and c["ids"][i, 2] > 0 and num >= 3:
            assert arg[2] == 2 and 2 in pos_c        # two identical GTs: the first one's class
            slot = np.nonzero(ref.sel[i] == 2)[0]
            assert len(slot) == 1 and ref.class_ids[i, slot[0]] == 21      # (it holds the largest positive key)
            seen.add("dup_gt_selected")
    if c["keys"] != "unique" and P >= 1023:
        assert "tie" in seen                         # a selection boundary fell inside a run of equal keys
    return seen


# ---------------------------------------------------------------------------------------------------------------
# past the kernels' limits: the wrappers run the tensor formulation, whose torch.max / argmax / topk leave ties open --
# so these inputs have unique keys and no IoU ties among GTs or anchors (asserted)
# ---------------------------------------------------------------------------------------------------------------
def _no_gt_ties(vv, rows):
    top = np.sort(vv[rows], 1)[:, -2:]
    return vv.shape[1] < 2 or bool((top[:, 1] > top[:, 0]).all())


def rpn_fallback_case():
    A, G, n_total = 2000, 257, 256
    rs = np.random.RandomState(31)
    anchors = synth_anchors(A, seed=1)
    ids, gts = np.zeros((2, G), np.int64), np.zeros((2, G, 4), np.float32)
    for i, n in enumerate((G, 40)):
        got = []
        while len(got) < n:
            for bx in np.concatenate([_draw_gt(rs, anchors, 8, True), _draw_gt(rs, anchors, 8, False)]):
                col = TR.iou_f32(anchors, bx[None])[:, 0]
                if col.max() > 0 and (col == col.max()).sum() == 1:        # one best anchor
                    got.append(bx)
        ids[i, :n], gts[i, :n] = rs.randint(1, 81, n), np.array(got[:n])
    c = dict(anchors=anchors, ids=ids, gts=gts, n_total=n_total, kp=rpn_keys("unique", 2, A, 1), kn=rpn_keys("unique", 2, A, 2))
    for i in range(2):
        cand, _, vv = TR.rpn_candidates(anchors, ids[i], gts[i], NEG_THRES, POS_THRES)
        assert _no_gt_ties(vv, cand == 1)                                  # one best GT for every positive candidate
    rpn_margins_hold(c)
    return c


def det_fallback_case(name):
    P, R, G = {"G257": (300, 64, 257), "P2049": (2049, 512, 8)}[name]
    rs = np.random.RandomState(37)
    num = np.array([P, P - 17, P], np.int64)
    imgs = [det_image(k, rs, P, G) for k in ("rich", "rich", "none")]
    ids, gts = np.stack([i[0] for i in imgs]), np.stack([i[1] for i in imgs])
    ids[:, 3], gts[:, 3] = 0, 0                                            # (no identical GT boxes here)
    for i in imgs:
        i[2][0] = (62 / 64, 1 / 64, 63 / 64, 3 / 64)                       # (and no pair on a threshold: DESIGNED_DET is the kernels')
    c = dict(name=name, keys="unique", kinds=["rich", "rich", "none"], P=P, R=R, ratio=0.33, G=G, mini=True, num=num, ids=ids,
             gts=gts, props=np.stack([i[2] for i in imgs]), kp=det_keys("unique", 3, P, 3), kn=det_keys("unique", 3, P, 4),
             pos_cap=int(R * 0.33), npp=1.0 / 0.33)
    for i in range(3):
        vv = np.where((ids[i] > 0)[None, :], TR.iou_f32(c["props"][i], gts[i]), np.float32(0))
        top = np.sort(vv, 1)[:, -2:]
        c["props"][i][(top[:, 1] >= np.float32(0.5)) & (top[:, 1] == top[:, 0])] = (62 / 64, 1 / 64, 63 / 64, 3 / 64)
        pos_c = TR.det_candidates(c["props"][i], int(num[i]), ids[i], gts[i])[0]
        vv = np.where((ids[i] > 0)[None, :], TR.iou_f32(c["props"][i], gts[i]), np.float32(0))
        assert _no_gt_ties(vv, pos_c)                                      # (those with two best GTs became background)
    for i in range(3):
        if (ids[i] > 0).any():
            assert _far_from(TR.iou_f64(gts[i][ids[i] > 0], c["props"][i]), (0.5,)).all()
        if (ids[i] < 0).any():
            assert _far_from(TR.iou_f64(gts[i][ids[i] < 0], c["props"][i]), (0.001,)).all()
    return c
