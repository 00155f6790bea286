"""GPU: the non-convolution entries of the core library -- csrc/glue.hip, fi_bn_act_backward and
fi_weight_transpose_batch (csrc/conv_igemm.hip), fi_proposal_gather (csrc/proposal.hip) and the clip + SGD step
(csrc/sgd.hip) -- at the shapes where their code takes another path than in a train step.

tests/test_gpu_step_glue_replay.py replays these entries at the shapes three real steps produce; the branches named in
each record's `why` below are ones those shapes never (or hardly ever) reach.  The records go through that file's
HANDLERS unchanged: the handlers hold the references (fp32 expressions compared bit for bit, tests/fp64_ref.py with
check_bar / check_increment) and the bars, and no tolerance is introduced here.  Every operand sits between guard zones
that the replay's _call checks after the launch.

A record is (ints, NULL pattern, address modulo 16 of the pointers, extra) as the recorder of tests/step_record.py keeps
it, plus `why`.  Offsets are bytes past a 16-byte boundary and only ones the entry's header accepts."""
import collections
import itertools

import numpy as np
import pytest
import torch

import test_gpu_step_glue_replay as G
from step_record import DEV

EPS = float(np.float32(1e-5))           # eps arguments are C floats: the records hold the value the entry sees
EPS2 = float(np.float32(1e-3))


def _rec(name, why, nulls=(), al=None, ex=(), **ints):
    args = G.SPECS[name][1]
    bad = [k for k in nulls if k not in args] + [k for k in (al or {}) if k not in args]
    assert not bad, (name, bad)
    nul = {k: k in nulls for k in args if k in G._PTRS and k != "stream"}
    return dict(I=ints, nul=nul, al=dict(al or {}), ex=ex, why=why)


# ---- the table -------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [((1, 3, 4), "H == 3: one window row of full height; W == 4: one thread column, no neighbour loads"),
               ((3, 4, 4), "even H, last window clipped to 2 rows; W == 4"),
               ((2, 5, 8), "odd H: a thread's second row is skipped (h >= H), last window of full height"),
               ((5, 7, 12), "odd H, three thread columns (left and right neighbour loads), 5 planes"),
               ((1, 9, 4), "odd H, W == 4: a single thread column over five row pairs"),
               ((2, 6, 20), "even H, five thread columns, odd OW pair count")]


def _pool_records():
    fwd, bwd = [], []
    for k, ((P, H, W), why) in enumerate(POOL_SHAPES):
        fwd.append(_rec("fi_maxpool3x3s2_forward", "glue.hip maxpool3s2_fwd_kernel: " + why, al={"y": 4 * (k % 2)},
                        planes=P, height=H, width=W))
        for pos, off in itertools.product((0, 1), (0, 4)):
            bwd.append(_rec("fi_maxpool3x3s2_backward", "glue.hip maxpool3s2_bwd_kernel: %s; positive_only %d, dy + %d" % (
                why, pos, off), al={"dy": off}, planes=P, height=H, width=W, positive_only=pos))
    fwd.append(_rec("fi_maxpool3x3s2_forward", "pool_better on signed inputs: ties, all-negative windows (no 0 start value)",
                    ex={"signed": True}, planes=3, height=7, width=12))
    fwd.append(_rec("fi_maxpool3x3s2_forward", "pool_better: v != v, the framework's NaN rule", ex={"nan": 6},
                    planes=3, height=7, width=12))
    for pos in (0, 1):
        bwd.append(_rec("fi_maxpool3x3s2_backward", "arg-max recomputed on signed inputs with ties, all-negative windows; "
                        "positive_only %d" % pos, ex={"signed": True}, planes=3, height=7, width=12, positive_only=pos))
        bwd.append(_rec("fi_maxpool3x3s2_backward", "arg-max recomputed with NaN in the windows; positive_only %d" % pos,
                        ex={"nan": 6}, planes=3, height=7, width=12, positive_only=pos))
    return fwd, bwd


def _sum2x2_records():
    out = []
    for (P, H, W), why in (((1, 1, 2), "one output pair"), ((1, 3, 4), "two pairs per row"),
                           ((3, 5, 6), "odd pair count per row, rows of dy 48 bytes apart"),
                           ((2, 7, 10), "odd H, odd pair count, two planes")):
        for off in (0, 8):
            out.append(_rec("fi_sum2x2", "glue.hip sum2x2_kernel: %s; out + %d (8-byte stores)" % (why, off),
                            al={"out": off}, planes=P, height=H, width=W))
    return out


def _interleave_records(name):
    gated = name.endswith("_gated")
    out = []

    def classes(H, W, only00):
        have = [k for k, (a, b) in (("c00", (0, 0)), ("c01", (0, 1)), ("c10", (1, 0)), ("c11", (1, 1)))
                if (H - a + 1) // 2 > 0 and (W - b + 1) // 2 > 0]
        return ["c00"] if only00 else have

    def add(P, H, W, why, only00=False, with_add=True, with_gate=True, al=None):
        have = classes(H, W, only00)
        nulls = [k for k in ("c00", "c01", "c10", "c11") if k not in have]
        if not with_add:
            nulls.append("add")
        if gated and not with_gate:
            nulls.append("gate")
        out.append(_rec(name, "glue.hip stride2_interleave_kernel: %s; classes %s, add %d, gate %d" % (
            why, "+".join(have), with_add, gated and with_gate), nulls=nulls, al=al, planes=P, height=H, width=W))

    scalar = [((1, 1, 1), "<false> one element, only c00 exists"), ((2, 5, 7), "<false> odd H and W: qw0 != qw1, qh0 != qh1"),
              ((3, 6, 6), "<false> W % 4 == 2, equal class sizes"), ((2, 7, 1), "<false> W == 1: the odd-column classes are empty")]
    vector = [((2, 4, 4), "<true> one 16-byte group per row"), ((2, 5, 8), "<true> odd H: qh0 != qh1"),
              ((1, 2, 12), "<true> three groups per row"), ((2, 1, 4), "<true> H == 1: only c00 and c01 exist")]
    for (P, H, W), why in scalar + vector:
        for only00, with_add, with_gate in itertools.product((False, True), (True, False), (True, False) if gated else (True,)):
            add(P, H, W, why, only00, with_add, with_gate)
    add(2, 1, 4, "<false> H == 1 with dx + 4", al={"dx": 4})
    for key in ("add", "dx") + (("gate",) if gated else ()):
        add(2, 5, 8, "<false> chosen for a W %% 4 == 0 shape because %s + 4" % key, al={key: 4})
        add(2, 4, 4, "<false> chosen for a W %% 4 == 0 shape because %s + 8" % key, al={key: 8})
    add(2, 5, 8, "<true> kept with c01 + 8 and c10 + 8 (8-byte class loads)", al={"c01": 8, "c10": 8})
    add(2, 5, 8, "<false> chosen because c11 + 4", al={"c11": 4})
    return out


def _relu_mask_records():
    out = []
    for n, off, aliased in itertools.product((1, 3, 4, 5, 1023, 1025, 2051), (0, 4), (False, True)):
        why = "glue.hip relu_mask_kernel: n = %d, %s, out %s" % (
            n, "vector groups + %d tail elements" % (n % 4) if off == 0 else "y + 4: n4 = 0, the whole call in the tail loop",
            "aliased to dy" if aliased else "separate")
        out.append(_rec("fi_relu_mask", why, al={"y": off}, ex={"aliased": aliased}, n=n))
    return out


ROW_SHAPES = [((1, 4), "one row of one 16-byte group"), ((7, 12), "three groups per row"),
              ((3, 262152), "row_len / 4 > 64 * 256: per capped at 64, a second grid-stride trip"),
              ((65535, 4), "n_index = 65535, the largest grid.y")]


def _rows_records():
    gather = [_rec("fi_rows_gather", "glue.hip rows_gather_kernel: " + why, n_index=n, row_len=L) for (n, L), why in ROW_SHAPES]
    scatter = [_rec("fi_rows_scatter_add", "glue.hip rows_scatter_add_kernel: " + why, n_index=n, row_len=L)
               for (n, L), why in ROW_SHAPES]
    comb = []
    for ((n, L), why), nf in zip(ROW_SHAPES, (1, 3, 2, 1000)):
        comb.append(_rec("fi_rows_combine", "glue.hip rows_combine_kernel: %s; n_front %d" % (why, nf), n_front=nf, rows=n,
                         row_len=L))
    comb += [_rec("fi_rows_combine", "rows_combine_kernel: n_front = 0 with front NULL (hf never true)", nulls=["front"],
                  n_front=0, rows=7, row_len=12),
             _rec("fi_rows_combine", "rows_combine_kernel: n_front = rows (hf always true)", n_front=7, rows=7, row_len=12),
             _rec("fi_rows_combine", "rows_combine_kernel: every src_row -1 (hs never true, row 0 of src only addressed)",
                  ex={"neg": 1.0}, n_front=3, rows=7, row_len=12),
             _rec("fi_rows_combine", "rows_combine_kernel: no src_row -1", ex={"neg": 0.0}, n_front=3, rows=7, row_len=12)]
    return gather, scatter, comb


def _rows_mask_records():
    name, out = "fi_rows_mask_scale", []
    for (M, N, ld), why in (((1, 4, 4), "one row, one column quad, N % 256 != 0"),
                            ((5, 4, 8), "ld_out > N with tiny M: padding columns stay put"),
                            ((33, 260, 260), "two panels, the second with one quad; two row blocks, the second with one row"),
                            ((130, 1024, 1032), "four full panels, ld_out > N, five row blocks")):
        for flags in (0, 1):
            out.append(_rec(name, "glue.hip rows_mask_scale_kernel: %s; FI_OUTPUTS_ZEROED %d" % (why, flags), M=M, N=N,
                            ld_out=ld, relu=1, flags=flags))
    out.append(_rec(name, "fi_rows_mask_scale: panels * ceil(M / 32) = 2080 > 2048, rows_per_block doubles; colsum alone",
                    nulls=["g", "gs", "scale"], M=2080, N=8192, ld_out=8192, relu=1, flags=0))
    for (M, N, ld) in ((5, 4, 8), (33, 260, 260)):
        z = dict(M=M, N=N, ld_out=ld)
        out += [_rec(name, "rows_mask_scale_kernel: scale NULL (gs = g)", nulls=["scale"], relu=1, flags=0, **z),
                _rec(name, "rows_mask_scale_kernel: y NULL with relu = 0", nulls=["y"], relu=0, flags=1, **z),
                _rec(name, "rows_mask_scale_kernel: relu = 0 with y given", relu=0, flags=0, **z),
                _rec(name, "rows_mask_scale_kernel: g alone", nulls=["gs", "colsum", "scale"], relu=1, flags=0, **z),
                _rec(name, "rows_mask_scale_kernel: gs alone", nulls=["g", "colsum"], relu=1, flags=0, **z),
                _rec(name, "rows_mask_scale_kernel: colsum alone, zero-filled by the call, colsum + 4 (scalar atomics)",
                     nulls=["g", "gs", "scale"], al={"colsum": 4}, relu=1, flags=0, **z),
                _rec(name, "rows_mask_scale_kernel: colsum alone, FI_OUTPUTS_ZEROED", nulls=["g", "gs", "scale"], relu=1,
                     flags=1, **z)]
    return out


def _rows_affine_records():
    out = []
    for (M, N), why in (((1, 4), "one 16-byte group"), ((3, 12), "c = (4 i) % N wraps every three groups"),
                        ((5, 260), "N % 256 != 0"), ((2049, 4096), "(total4 + 255) / 256 = 8196 blocks: grid capped at 8192")):
        for sc, b, relu in itertools.product((True, False), (True, False), (0, 1)):
            out.append(_rec("fi_rows_affine_act", "glue.hip rows_affine_act_kernel: %s; scale %d, bias %d, relu %d" % (
                why, sc, b, relu), nulls=([] if sc else ["scale"]) + ([] if b else ["bias"]), M=M, N=N, relu=relu))
    return out


def _fold_records():
    name = "fi_bn_fold_grad"
    geo = [((1, 1, 1, 0, 0), "K = 1: scalar loop, one element", []),
           ((2, 3, 49, 0, 0), "K = 147, K % 4 != 0: scalar loop, same order", ["conv_bias"]),
           ((3, 5, 9, 1, 0), "!same_order, dW' tap-major: index map ci * taps + tap", ["dgamma"]),
           ((3, 5, 9, 0, 1), "!same_order, W tap-major: index map tap * Cin + ci", ["dbias"]),
           ((2, 4, 9, 1, 1), "both tap-major, K = 36: vector loop", []),
           ((2, 8, 1, 1, 0), "taps == 1 counts as the same order: vector loop", ["conv_bias", "dgamma"]),
           ((2, 300, 9, 0, 0), "K = 2700 > 2048: three trips of the vector loop, the last partly filled", [])]
    out = [_rec(name, "glue.hip bn_fold_grad_kernel: %s; NULL %s" % (why, nulls or "none"), nulls=nulls, eps=EPS, Cout=g[0],
                Cin=g[1], taps=g[2], dw_tap_major=g[3], w_tap_major=g[4]) for g, why, nulls in geo]
    z = dict(Cout=2, Cin=4, taps=9, dw_tap_major=1, w_tap_major=1)
    out += [_rec(name, "fi_bn_fold_grad: a vector-eligible K with dw + 4 takes the scalar loop", al={"dw": 4}, eps=EPS, **z),
            _rec(name, "fi_bn_fold_grad: a vector-eligible K with w + 8 takes the scalar loop", al={"w": 8}, eps=EPS2, **z),
            _rec(name, "bn_fold_grad_kernel: conv_bias, dgamma and dbias all NULL (only dW is scaled)",
                 nulls=["conv_bias", "dgamma", "dbias"], eps=EPS, **z),
            _rec(name, "bn_fold_grad_kernel: conv_bias and dbias NULL on the index-mapped loop", nulls=["conv_bias", "dbias"],
                 eps=EPS2, Cout=3, Cin=5, taps=9, dw_tap_major=1, w_tap_major=0)]
    return out


def _fold_batch_records():
    name, out = "fi_bn_fold_grad_batch", []
    z = dict(eps=EPS, Cout=4, Cin=8, taps=9, dw_tap_major=1, w_tap_major=1)

    def ex(n, dws=None, cbs="all", dgammas="all", dbiases="all"):
        # a table: None = NULL, "all" = every member has the pointer, k = every k-th member's entry is NULL
        tab = lambda v: None if v is None else tuple([True] * n if v == "all" else [(j % v) != 0 for j in range(n)])
        return {"dws": tuple(dws or [0] * n), "ws": tuple([0] * n), "cbs": tab(cbs), "dgammas": tab(dgammas),
                "dbiases": tab(dbiases)}

    for n, why in ((1, "one member"), (24, "n = FI_WGRAD_BATCH_MAX: one full launch"),
                   (25, "n = 25: a second launch with one member (unused slots repeat it)"),
                   (49, "n = 49: three launches, the last with one member")):
        out.append(_rec(name, "fi_bn_fold_grad_batch: %s; vector loop" % why, ex=ex(n), n=n, **z))
    out.append(_rec(name, "fi_bn_fold_grad_batch: member 26's dw + 4 drops vec for the second launch only", n=49,
                    ex=ex(49, dws=[4 if j == 26 else 0 for j in range(49)]), **z))
    out.append(_rec(name, "bn_fold_grad_batch_kernel: NULL entries in cbs / dgammas / dbiases (every 2nd / 3rd / 5th member)",
                    n=25, ex=ex(25, cbs=2, dgammas=3, dbiases=5), **z))
    out.append(_rec(name, "fi_bn_fold_grad_batch: NULL tables for conv_bias, dgamma and dbias", nulls=["cbs", "dgammas", "dbiases"],
                    n=3, ex=ex(3, cbs=None, dgammas=None, dbiases=None), **z))
    out.append(_rec(name, "bn_fold_grad_batch_kernel: !same_order index map (dW' channel-major, W tap-major), K % 4 != 0", n=3,
                    ex=ex(3, dbiases=None), nulls=["dbiases"], eps=EPS2, Cout=3, Cin=5, taps=9, dw_tap_major=0, w_tap_major=1))
    return out


def _bn_fold_records():
    chans = ((1, EPS, False), (255, EPS, True), (256, EPS2, False), (257, EPS2, True), (700, EPS, True))
    return [_rec("fi_bn_fold_batch", "glue.hip bn_fold_kernel: channel counts 1 / 255 / 256 / 257 / 700 in one table (blocks past "
                 "a pair's channels return), mixed conv bias, two eps", ex=chans, n=len(chans), max_channels=700)]


def _tiles(descs):
    return sum(t * ((r + 31) // 32) * ((c + 31) // 32) for r, c, t, _, _ in descs)


def _transpose_records():
    name = "fi_weight_transpose_batch"
    mixed = ((1, 1, 1, 0, False), (64, 3, 49, 0, True), (32, 32, 1, 1, True), (33, 31, 9, 0, False), (64, 96, 1, 3, False),
             (81, 256, 1, 0, True), (96, 32, 1, 1, False), (70, 100, 4, 0, True))
    big = ((2048, 2048, 16, 0, False), (33, 31, 9, 0, True))
    return [_rec(name, "conv_igemm.hip weight_transpose_kernel: partly filled tiles, with and without row_scale, fragment-major "
                 "descriptors (flag 1, flag 3) between plain ones: the bisection crosses kinds", ex=mixed, n=len(mixed),
                 total_tiles=_tiles(mixed)),
            _rec(name, "fi_weight_transpose_batch: 65536 tiles in the first descriptor, total_tiles > 65536: the capped grid's "
                 "second trip", ex=big, n=len(big), total_tiles=_tiles(big))]


def _class_row_records():
    name = "fi_class_row_conv1x1_backward"
    z = lambda N, C, HW, K, g: dict(N=N, C=C, HW=HW, num_classes=K, gated=g)
    out = [_rec(name, "glue.hip class_row_conv1x1_bwd_kernel: one row, channel, pixel, class", ex={"dead": 0.0}, **z(1, 1, 1, 1, 0)),
           _rec(name, "class_row_conv1x1_bwd_kernel: HW = 3, len & 3 != 0: scalar zero fill of dead rows; C = 5: cend - c0 "
                "not a multiple of 8, wave 0 pairs (0, 4)", ex={"dead": 0.5}, **z(3, 5, 3, 2, 1)),
           _rec(name, "class_row_conv1x1_bwd_kernel: odd HW = 49, full channel block, K = 81", **z(7, 64, 49, 81, 1)),
           _rec(name, "class_row_conv1x1_bwd_kernel: C = 70: a second channel block with 6 channels (two only for waves 0, 1)",
                **z(9, 70, 196, 81, 0)),
           _rec(name, "class_row_reduce_kernel: N = 300 > 256: two row chunks; K = 240, the largest LDS table",
                **z(300, 8, 16, 240, 1)),
           _rec(name, "fi_class_row_conv1x1_backward: HW = 16384, the documented limit: 64 KB of dynamic LDS next to s_any",
                ex={"dead": 0.0}, **z(2, 4, 16384, 3, 0)),
           _rec(name, "class_row kernels: all rows dead (nothing is live in phase 2)", ex={"dead": 1.0}, **z(7, 64, 49, 81, 1)),
           _rec(name, "class_row kernels: no row dead", ex={"dead": 0.0}, **z(7, 64, 49, 81, 1)),
           _rec(name, "class_row_reduce_kernel: rows 0-255 dead: the first row chunk flushes nothing", ex={"dead_rows": 256},
                **z(300, 8, 16, 240, 1)),
           _rec(name, "class_row_reduce_kernel: class 1 of 2 has no row (its LDS sums stay 0, no atomic)", ex={"unused_class": 1,
                "dead": 0.0}, **z(3, 5, 3, 2, 1)),
           _rec(name, "class_row_reduce_kernel: class 0 of 81 has no row", ex={"unused_class": 0}, **z(9, 70, 196, 81, 1)),
           _rec(name, "class_row_conv1x1_bwd_kernel: dead rows' zero fill with dx + 4 on a len % 4 == 0 block (scalar fill); "
                "d + 4, x + 8", al={"dx": 4, "d": 4, "x": 8}, **z(9, 8, 16, 5, 1))]
    for k in ("dx", "dweight", "dbias"):
        out.append(_rec(name, "fi_class_row_conv1x1_backward: %s NULL" % k, nulls=[k], **z(9, 70, 196, 81, 0)))
    out.append(_rec(name, "fi_class_row_conv1x1_backward: dweight and dbias NULL: phase 2 is not launched",
                    nulls=["dweight", "dbias"], **z(9, 70, 196, 81, 1)))
    return out


EIGHT_H, EIGHT_W = (9, 8, 6, 5, 4, 3, 2, 1), (7, 6, 5, 4, 3, 2, 1, 1)


def _patch_records(name):
    fwd = name.endswith("_forward")
    k = "glue.hip patch_rows_%s_kernel: " % ("fwd" if fwd else "bwd")
    lv = lambda hs, ws, **more: dict(heights=tuple(hs), widths=tuple(ws), **more)
    z = lambda hs, per, rows, ch: dict(levels=len(hs), per_loc=per, rows=rows, channels=ch)
    out = [_rec(name, k + "one level of 1 x 1, per_loc 1, rows = 1, one channel: eight of nine taps outside",
                ex=lv((1,), (1,), pad=0.0), **z((1,), 1, 1, 1)),
           _rec(name, k + "one 1 x 1 level, five rows on one anchor%s; 257 channels: a second trip of one lane" % (
               "" if fwd else ": duplicates meet in the atomics"), ex=lv((1,), (1,), pad=0.0), **z((1,), 1, 5, 257)),
           _rec(name, k + "eight levels 9 x 7 .. 1 x 1, per_loc 3: level search to the last level, level starts and corners; "
                "300 channels", ex=lv(EIGHT_H, EIGHT_W), **z(EIGHT_H, 3, 40, 300)),
           _rec(name, k + "maps of width 1 and of height 1, per_loc 2", ex=lv((5, 1), (1, 6)), **z((5, 1), 2, 14, 257)),
           _rec(name, k + "all rows padding (image < 0)", ex=lv((4, 2), (3, 2), pad=1.0), **z((4, 2), 3, 9, 300)),
           _rec(name, k + "three images, more rows than anchors, the last six rows repeat row 0", ex=lv((2, 1), (2, 1), B=3,
                dup=6, pad=0.0), **z((2, 1), 1, 12, 1))]
    out.append(_rec(name, k + "%s + 4 (element accesses)" % ("out" if fwd else "d"), al={"out" if fwd else "d": 4},
                    ex=lv(EIGHT_H, EIGHT_W, dup=3), **z(EIGHT_H, 3, 24, 257)))
    return out


def _gather_records():
    name = "fi_proposal_gather"
    z = lambda B, pre, st, ks, cnt: dict(batch=B, pre_nms=pre, det_stride=st, keep_stride=ks, proposal_count=cnt, norm_h=1024.0,
                                         norm_w=1344.0)
    return [_rec(name, "proposal.hip proposal_gather_kernel: one image, one detection, det_stride 4", **z(1, 1, 4, 1, 1)),
            _rec(name, "proposal_gather_kernel: proposal_count 300 > keep_stride 10: two blocks, rows past num are zeros",
                 **z(2, 10, 5, 10, 300)),
            _rec(name, "proposal_gather_kernel: proposal_count 257: a second block with one live thread", **z(3, 6000, 5, 6000, 257)),
            _rec(name, "proposal_gather_kernel: det_stride 7, keep_stride 20 < pre_nms", **z(2, 50, 7, 20, 64)),
            _rec(name, "proposal_gather_kernel: num[0] = 30 > keep_stride (j < keep_stride stops the read), num[1] = 0",
                 ex={"num": (30, 0)}, **z(2, 50, 7, 20, 64)),
            _rec(name, "proposal_gather_kernel: keep entries -1 and pre_nms give rows of zeros", ex={"num": (10, 3), "bad_keep": True},
                 **z(2, 10, 5, 10, 300))]


def _bn_act_records():
    name, out = "fi_bn_act_backward", []
    z = lambda N, C, HW, relu=1, flags=0, layout=0: dict(N=N, C=C, HW=HW, relu=relu, layout=layout, flags=flags)
    base = ["residual", "g_out", "dbias"]
    k = "conv_igemm.hip bn_act_bwd_kernel: "
    for (N, C, HW), why in (((1, 1, 1), "one element (scalar loop)"), ((2, 3, 49), "HW % 4 != 0: scalar loop"),
                            ((3, 5, 4), "one 16-byte group per plane: the one-group tail alone"),
                            ((2, 2, 1024), "HW = 1024: i + 1024 < HW never true, tail for every lane"),
                            ((2, 2, 1028), "HW = 1028: lane 0 takes two groups in one trip, the others the tail"),
                            ((1, 3, 2048), "HW = 2048: one full two-group trip, no tail"),
                            ((2, 2, 2052), "HW = 2052: lane 0 two-group trip then tail at 2048"),
                            ((1, 1, 4100), "HW = 4100: two two-group trips then a tail for lane 0"),
                            ((70, 1, 8), "C = 1: chunks = N = 70, one image per block"),
                            ((5, 1000, 4), "C = 1000: chunks 3, ipb 2: the last chunk partly filled"),
                            ((3, 2050, 4), "C = 2050 > 2048: one chunk of all images")):
        ex = {"live_gamma": True} if C == 1 else ()
        out.append(_rec(name, k + why, nulls=base, ex=ex, **z(N, C, HW)))
    out.append(_rec(name, k + "C = 1 with gamma == 0: dgamma reads 0", nulls=base, **z(70, 1, 8)))
    for (N, C, HW) in ((2, 3, 49), (2, 2, 1028)):
        for res, g, relu in itertools.product((False, True), (False, True), (0, 1)):
            nulls = ["dbias"] + ([] if res else ["residual"]) + ([] if g else ["g_out"])
            out.append(_rec(name, k + "<%d, %d> relu %d on HW = %d" % (res, g, relu, HW), nulls=nulls, **z(N, C, HW, relu)))
        out += [_rec(name, "fi_bn_act_backward: gamma NULL (unit scale, no dgamma): the separate fills", nulls=base + ["gamma",
                     "beta", "dgamma"], **z(N, C, HW)),
                _rec(name, k + "beta NULL (be = 0)", nulls=base + ["beta"], **z(N, C, HW)),
                _rec(name, "fi_bn_act_backward: dbias present, adjacent sums: one fill of 3 C", nulls=["residual", "g_out"],
                     **z(N, C, HW)),
                _rec(name, "fi_bn_act_backward: dbias present, FI_OUTPUTS_ZEROED", nulls=["residual", "g_out"],
                     **z(N, C, HW, flags=1)),
                _rec(name, "fi_bn_act_backward: sum buffers not adjacent: three fills", nulls=["residual", "g_out"],
                     ex={"split_sums": True}, **z(N, C, HW)),
                _rec(name, "fi_bn_act_backward: sum buffers not adjacent, dbias NULL: two fills", nulls=base,
                     ex={"split_sums": True}, al={"dgamma": 4}, **z(N, C, HW)),
                _rec(name, "fi_bn_act_backward: sum buffers not adjacent, FI_OUTPUTS_ZEROED", nulls=["residual", "g_out"],
                     ex={"split_sums": True}, al={"dshift": 8, "dbias": 4}, **z(N, C, HW, flags=1))]
    for (N, C, HW) in ((3, 5, 4), (2, 2, 1028)):
        for key, off in (("dy", 4), ("y", 4), ("residual", 4), ("dz", 4), ("g_out", 4), ("dy", 8), ("dz", 12)):
            out.append(_rec(name, "fi_bn_act_backward: HW % 4 == 0 with " + key + " + %d: the launcher's vec is 0, scalar loop" % off,
                            nulls=["dbias"], al={key: off}, **z(N, C, HW)))
    k = "conv_igemm.hip bn_act_bwd_cl_kernel: "
    for (N, C, HW), why, relu, flags, nulls in (
            ((1, 1, 1), "one pixel, one channel", 1, 0, base), ((2, 65, 49), "C = 65: a second channel block with one channel; "
                                                                "P = 98: a partly filled second tile", 1, 0, base),
            ((3, 64, 64), "full tiles, one channel block, relu 0, FI_OUTPUTS_ZEROED", 0, 1, base),
            ((1, 130, 200), "three channel blocks, P = 200, dbias present", 1, 0, ["residual", "g_out"]),
            ((1100, 128, 64), "tiles * cblk = 2200 > 2048: tiles_per_block = 2", 1, 0, base)):
        out.append(_rec(name, k + why, nulls=nulls, ex={"live_gamma": True} if C == 1 else (), **z(N, C, HW, relu, flags, 1)))
    return out


SGD_NUMEL = (1, 3, 4, 5, 8191, 8192, 8193, 16384, 16385)
# (label, offsets of parameter / gradient / momentum buffer in bytes; the buffer's applies from the second step on)
SGD_CONFIGS = (("aligned", 0, 0, 0), ("parameter + 4", 4, 0, 0), ("gradient + 4 alone: sumsq scalar by g, update scalar by p|g|b", 0, 4, 0),
               ("momentum buffer + 4 alone, from the second step", 0, 0, 4))
SGD_CASES = [dict(numel=n, config=c[0], p=c[1], g=c[2], b=c[3], why="sgd.hip: %d elements (chunks of 8192), %s" % (n, c[0]))
             for n in SGD_NUMEL for c in SGD_CONFIGS]


def _table():
    t = collections.OrderedDict()
    t["fi_maxpool3x3s2_forward"], t["fi_maxpool3x3s2_backward"] = _pool_records()
    t["fi_sum2x2"] = _sum2x2_records()
    t["fi_stride2_interleave"] = _interleave_records("fi_stride2_interleave")
    t["fi_stride2_interleave_gated"] = _interleave_records("fi_stride2_interleave_gated")
    t["fi_relu_mask"] = _relu_mask_records()
    t["fi_rows_gather"], t["fi_rows_scatter_add"], t["fi_rows_combine"] = _rows_records()
    t["fi_rows_mask_scale"] = _rows_mask_records()
    t["fi_rows_affine_act"] = _rows_affine_records()
    t["fi_bn_fold_grad"] = _fold_records()
    t["fi_bn_fold_grad_batch"] = _fold_batch_records()
    t["fi_bn_fold_batch"] = _bn_fold_records()
    t["fi_weight_transpose_batch"] = _transpose_records()
    t["fi_class_row_conv1x1_backward"] = _class_row_records()
    t["fi_pyramid_patch_rows_forward"] = _patch_records("fi_pyramid_patch_rows_forward")
    t["fi_pyramid_patch_rows_backward"] = _patch_records("fi_pyramid_patch_rows_backward")
    t["fi_proposal_gather"] = _gather_records()
    t["fi_bn_act_backward"] = _bn_act_records()
    return t


TABLE = _table()
ENTRIES = [n for n, (fam, _) in G.SPECS.items() if fam != "sgd"]


# ---- host-only checks --------------------------------------------------------------------------------------------------
def test_every_entry_has_records_with_the_keys_of_its_spec():
    """(CPU) every entry of the replay's SPECS has records (the two SGD entries the optimizer cases); the keys of every
    record are the entry's arguments; every `why` names what the record is for."""
    assert set(TABLE) == set(ENTRIES), set(TABLE) ^ set(ENTRIES)
    assert {n for n, (fam, _) in G.SPECS.items() if fam == "sgd"} == {"fi_sgd_clip_step", "fi_sgd_clip_step_guarded"}
    assert {c["numel"] for c in SGD_CASES} == set(SGD_NUMEL) and len(SGD_CASES) == len(SGD_NUMEL) * len(SGD_CONFIGS)
    assert all(c["why"].strip() for c in SGD_CASES)
    for name, recs in TABLE.items():
        args = G.SPECS[name][1]
        assert recs, name
        for r in recs:
            assert set(r["I"]) == {a for a in args if a not in G._PTRS}, (name, r["why"], sorted(r["I"]))
            assert set(r["nul"]) == {a for a in args if a in G._PTRS and a != "stream"}, (name, r["why"])
            assert set(r["al"]) <= {a for a in r["nul"] if not r["nul"][a]}, (name, r["why"], r["al"])
            assert all(v % 4 == 0 and 0 <= v < 16 for v in r["al"].values()), (name, r["al"])
            assert isinstance(r["why"], str) and len(r["why"].strip()) >= 8, (name, r)
        assert G.SPECS[name][0] in G.HANDLERS, name


def test_glue_entries_refuse_what_their_headers_exclude_without_a_gpu():
    """(CPU) return codes only: the argument checks come before any HIP call."""
    import ctypes
    from feature_intertwiner_amd import _lib
    L = _lib.load()
    for fn in (L.fi_rows_gather, L.fi_rows_scatter_add):
        assert fn(16, 16, 16, 4, 6, None) == -1                                        # row_len % 4
        assert b"row_len" in L.fi_last_error()
        assert fn(16, 16, 16, 65536, 4, None) == -1                                    # n_index > 65535
        assert b"65535" in L.fi_last_error()
        assert fn(16, 16, 20, 4, 4, None) == -1                                        # dst off a 16-byte boundary
        assert fn(None, None, None, 0, 4, None) == 0
    assert L.fi_rows_combine(16, 1, 16, 16, 16, 4, 6, None) == -1                      # row_len % 4
    assert L.fi_rows_combine(16, 1, 16, 16, 16, 65536, 4, None) == -1                  # rows > 65535
    assert b"65535" in L.fi_last_error()
    assert L.fi_rows_combine(16, 5, 16, 16, 16, 4, 4, None) == -1                      # n_front > rows
    assert L.fi_rows_combine(None, 1, 16, 16, 16, 4, 4, None) == -1                    # front NULL with n_front > 0
    assert L.fi_rows_mask_scale(16, 16, 16, 16, 16, 16, 4, 6, 8, 1, 0, None) == -1     # N % 4
    assert L.fi_rows_mask_scale(16, 16, 16, 16, 16, 16, 4, 8, 4, 1, 0, None) == -1     # ld_out < N
    assert b"ld_out" in L.fi_last_error()
    assert L.fi_rows_mask_scale(16, None, 16, 16, 16, 16, 4, 8, 8, 1, 0, None) == -1   # relu without y
    assert L.fi_rows_mask_scale(16, 16, 16, 20, 16, 16, 4, 8, 8, 1, 0, None) == -1     # g off a 16-byte boundary
    assert L.fi_rows_affine_act(16, 16, 16, 4, 6, 1, None) == -1                       # N % 4
    assert L.fi_rows_affine_act(16, 20, 16, 4, 8, 1, None) == -1                       # scale off a 16-byte boundary
    cr = lambda HW, K: L.fi_class_row_conv1x1_backward(16, 16, 16, 16, 16, 16, 16, 4, 8, HW, K, 0, 16, None)
    assert cr(16385, 81) == -1
    assert b"16384" in L.fi_last_error()
    assert cr(16, 241) == -3                                                           # FI_ERR_UNSUPPORTED
    assert b"240" in L.fi_last_error()
    assert L.fi_class_row_conv1x1_backward(None, None, None, None, None, None, None, 0, 8, 16, 81, 0, None, None) == 0
    maps = (ctypes.c_void_p * 9)(*([16] * 9))
    ones = (ctypes.c_int * 9)(*([1] * 9))
    zero = (ctypes.c_int * 9)(1, 0, 1, 1, 1, 1, 1, 1, 1)
    assert L.fi_pyramid_patch_rows_forward(maps, ones, ones, 9, 3, 16, 16, 4, 8, 16, None) == -1       # levels > 8
    assert b"levels" in L.fi_last_error()
    assert L.fi_pyramid_patch_rows_backward(16, maps, ones, ones, 9, 3, 16, 16, 4, 8, None) == -1
    assert L.fi_pyramid_patch_rows_forward(maps, zero, ones, 2, 3, 16, 16, 4, 8, 16, None) == -1       # a zero map size
    assert b"map size" in L.fi_last_error()
    assert L.fi_pyramid_patch_rows_backward(16, maps, ones, zero, 2, 3, 16, 16, 4, 8, None) == -1
    assert L.fi_pyramid_patch_rows_forward(maps, ones, ones, 2, 0, 16, 16, 4, 8, 16, None) == -1       # per_loc < 1
    assert L.fi_proposal_gather(16, 10, 3, 16, 10, 16, 1, 10, 1.0, 1.0, 16, None) == -1                # det_stride < 4
    assert L.fi_proposal_gather(16, 10, 5, 16, 10, 16, 1, 10, 1.0, 1.0, 20, None) == -1                # proposals misaligned
    assert b"aligned" in L.fi_last_error()
    assert L.fi_proposal_gather(None, 10, 5, None, 10, None, 0, 10, 1.0, 1.0, None, None) == 0
    # layout 1 has no fused residual and no g_out (the fills before the check need FI_OUTPUTS_ZEROED to stay off the device)
    assert L.fi_bn_act_backward(16, 16, 16, 16, 16, 16, 1, 8, 16, 1, 16, None, 16, 16, None, 1, 1, None) == -1
    assert b"residual" in L.fi_last_error()
    assert L.fi_bn_act_backward(16, 16, 16, 16, 16, None, 1, 8, 16, 1, 16, 16, 16, 16, None, 1, 1, None) == -1
    assert L.fi_bn_act_backward(16, 16, 16, None, 16, None, 1, 8, 16, 1, 16, None, 16, 16, None, 0, 1, None) == -1  # dgamma, no gamma


# ---- GPU: the records through the replay's handlers ------------------------------------------------------------------------
def _synthetic_bn():
    g = torch.Generator(device=DEV).manual_seed(77)
    ga = 1.0 + 0.2 * torch.randn(96, generator=g, device=DEV)
    be = 0.3 * torch.randn(96, generator=g, device=DEV)
    return {96: (ga, be)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENTRIES)
def test_entry_matches_its_reference_at_the_edge_records(name):
    from feature_intertwiner_amd import _lib
    bn = _synthetic_bn()
    fam = G.SPECS[name][0]
    worst, failures = 0.0, []
    for i, r in enumerate(TABLE[name]):
        del G._GUARDED[:]
        try:
            # (name, I, nul, al, ex) as replay() builds them from a recorded key
            w = G.HANDLERS[fam](name, dict(r["I"]), dict(r["nul"]), dict(r["al"]), r["ex"], G._Ctx(5000 + i, bn))
            worst = max(worst, w)
        except (AssertionError, _lib.FiError) as e:
            failures.append("record %d [%s]: %s" % (i, r["why"], str(e)[:600]))
    torch.cuda.empty_cache()
    print("\n  %-40s records %4d   worst |d|/(2^-24 m) %8.2f" % (name, len(TABLE[name]), worst))
    assert not failures, "%d of %d records off:\n%s" % (len(failures), len(TABLE[name]), "\n".join(failures[:20]))


def _sgd_optimizer(momentum, ctx):
    """Two groups (weight decay 1e-4 and 0), each holding every (numel, configuration) case; parameters and gradients
    are views at the case's storage offset, between guard zones."""
    groups, cases = [], []
    for wd in (1e-4, 0.0):
        params = []
        for c in SGD_CASES:
            p = torch.nn.Parameter(G._place(ctx.randn(c["numel"]), c["p"]))
            p.grad = G._place(ctx.randn(c["numel"]), c["g"])
            assert p.data_ptr() % 16 == c["p"] and p.grad.data_ptr() % 16 == c["g"], c
            params.append(p)
            cases.append((p, c))
        groups.append(dict(params=params, weight_decay=wd))
    return torch.optim.SGD(groups, lr=0.05, momentum=momentum), cases


@pytest.mark.gpu
@pytest.mark.parametrize("momentum", [0.9, 0.0])
def test_sgd_clip_step_at_chunk_boundaries_and_misaligned_tensors(momentum):
    """optim.clip_and_step inside the replay's _SgdCheck (its bars unchanged): a step that does not clip, a step that
    clips (the scaled gradients are written back) after the momentum buffers of the last configuration moved off a
    16-byte boundary, and a guarded step with finite gradients."""
    from feature_intertwiner_amd import optim
    del G._GUARDED[:]
    ctx = G._Ctx(6000, {})
    opt, cases = _sgd_optimizer(momentum, ctx)
    zones = list(G._GUARDED)

    def guards(what):
        G._GUARDED[:] = zones
        G._check_guards(what)

    with G._SgdCheck(opt, guard_calls=(2,)) as chk:
        optim.clip_and_step(opt, 1e9)                                      # norm << max_norm: coef == 1, gradients untouched
        guards("clip_and_step, first step")
        assert float(optim._CACHE[opt]["out"][1]) == 1.0
        if momentum:
            for p, c in cases:
                if c["b"]:
                    opt.state[p]["momentum_buffer"] = G._place(opt.state[p]["momentum_buffer"], c["b"])
                    assert opt.state[p]["momentum_buffer"].data_ptr() % 16 == c["b"]
            zones += list(G._GUARDED)
        for p, c in cases:
            p.grad.copy_(ctx.randn(c["numel"]))
        optim.clip_and_step(opt, 5.0)                                      # norm ~ sqrt(459352) = 678 >> 5: clips
        guards("clip_and_step, clipping step")
        assert float(optim._CACHE[opt]["out"][1]) < 0.1
        for p, c in cases:
            p.grad.copy_(ctx.randn(c["numel"]))
        optim.clip_and_step(opt, 5.0)                                      # taken in the guarded form (guard_calls)
        guards("clip_and_step, guarded step")
    print("\n  %-40s calls %5d   worst |d|/(2^-24 m) %8.2f" % ("clip_and_step momentum %.1f (%d tensors)" % (
        momentum, len(cases)), chk.calls, chk.worst))
    assert not chk.fail, chk.fail
    assert chk.calls == 3 and chk.guarded_applied == 1, (chk.calls, chk.guarded_applied)
    assert optim.skipped_steps(opt) == 0
