"""What MODEL.ACT_SCOPE = 'pyramid' (the feature pyramid and the RPN on 16-bit channels-last tensors,
feature_intertwiner_amd/pyr16.py) costs and saves against scope 'trunk' (c2..c5 unpacked to fp32 NCHW behind the trunk), for
bf16 and fp16, ResNet-101 at 2 x 1344^2 and 4 x 1024^2.  MODEL.CONV_PRECISION and MODEL.ACT_PRECISION are the type in every arm.

In ONE process on one MI355X, the arms alternating round by round, each call timed with a HIP event pair, 5 warm-up and 20
timed rounds per arm, median / min / max.  Every comparison carries an A/A line: the 'trunk' arm runs TWICE per round under
two names, and |median - median| / median of the two is the spread a difference has to exceed to mean anything.
  (a) the segment from 16-bit c2..c5 to the RPN's outputs and the fp32 p2..p5 the Dev stage reads
        trunk:   4 unpacks (256..2048 channels), fp32 laterals with a materialised upsample, smoothing, RPN with permute copies
        pyramid: P5_conv1, 3 lateral launches, smoothing, p6 copy, RPN on 16-bit maps, 4 unpacks (256 channels)
      and the whole model's _inference both ways;
  (b) per layer and level, the old launch(es) against the new one: lateral (old: upsample2x + conv with residual),
      smoothing conv, shared conv, heads (old: stacked 1x1 conv + two permute copies), and the four unpacks before / after;
  (c) for the two new kernels the bytes they must move (x, top and y once, w in 16 bits) and the bytes/s achieved.
A layer that loses is marked; nothing falls back.

    python scripts/pyr16_probe.py [--out profiles/pyr16_probe.txt] [--types bf16,fp16] [--skip-model] [--skip-layers]
"""
import argparse
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, ROUNDS = 5, 20
SHAPES = ((2, 1344), (4, 1024))          # (images, image size)


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    del out
    return e0.elapsed_time(e1)


def _alternate(arms):
    """arms: [(name, fn)]; returns name -> list of ms, the arms taking turns inside every round."""
    for _ in range(WARMUP):
        for _, fn in arms:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in arms}
    for _ in range(ROUNDS):
        for name, fn in arms:
            times[name].append(_timed(fn))
    return times


def _row(t):
    return statistics.median(t), min(t), max(t), max(t) - min(t)


def _clocks():
    """The clocks as found (read only), or why they could not be read."""
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30).stdout
        rows = [l.strip() for l in out.splitlines() if "sclk" in l or "mclk" in l or "fclk" in l]
        return "; ".join(rows) if rows else "rocm-smi printed no clock lines"
    except Exception as e:          # the probe measures without them
        return "not read (%s)" % (e,)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pyr16_probe.txt"))
    ap.add_argument("--types", default="bf16,fp16")
    ap.add_argument("--skip-model", action="store_true", help="leave out the whole model's _inference")
    ap.add_argument("--skip-layers", action="store_true", help="leave out parts (b) and (c)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    from feature_intertwiner_amd import act16, pyr16
    from feature_intertwiner_amd import conv as Cv
    from feature_intertwiner_amd.config import make_config
    from feature_intertwiner_amd.model import MaskRCNN
    from feature_intertwiner_amd.synthetic import SyntheticProposals, synthetic_batch
    dev = "cuda:0"
    lines = []

    def emit(line=""):
        lines.append(line)
        print(line, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:          # kept current: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")

    emit("pyr16_probe: FPN and RPN on 16-bit channels-last tensors (ACT_SCOPE 'pyramid') vs fp32 NCHW behind the trunk "
         "(ACT_SCOPE 'trunk'), ResNet-101, %s" % torch.cuda.get_device_name(0))
    emit("%d timed rounds per arm after %d warm-up rounds, arms alternating in one process, HIP events; ms" % (ROUNDS, WARMUP))
    emit("clocks as found: %s" % _clocks())
    verdicts = []

    def compare(title, old, new, indent="  "):
        """old twice (A/A) and new, alternating; returns (median old, median new, A/A spread as a fraction)."""
        t = _alternate([("old", old), ("new", new), ("old again", old)])
        mo, mn, mo2 = (statistics.median(t[k]) for k in ("old", "new", "old again"))
        aa = abs(mo - mo2) / mo
        emit("%s%s" % (indent, title))
        for name in ("old", "old again", "new"):
            emit("%s  %-10s median %8.3f  min %8.3f  max %8.3f  spread %6.3f" % ((indent, name) + _row(t[name])))
        emit("%s  new / old = %.3f   A/A |old - old again| / old = %.3f%s" % (
            indent, mn / mo, aa, "" if mn <= mo * (1.0 + aa) else "   <- loses by more than the A/A spread"))
        return mo, mn, aa

    for prec in args.types.split(","):
        dtype = act16.dtype_of(prec)
        for n, size in SHAPES:
            torch.manual_seed(2000)
            cfg = make_config("resnet101", size, n, 1000, conv_precision=prec)
            cfg.MODEL.ACT_PRECISION = prec
            model = MaskRCNN(cfg).to(dev).eval()
            fpn, rpn = model.fpn, model.rpn
            hw = size // 4
            Cv.set_conv_precision(prec)
            with torch.no_grad():
                Cv.prepare_step(model)          # BatchNorm folds, channels-last weights and their 16-bit copies, as _inference does
                sides = {2: hw, 3: hw // 2, 4: hw // 4, 5: hw // 8}
                c16 = {l: act16.pack(torch.relu(torch.randn(n, 64 << l, s, s, device=dev)), dtype) for l, s in sides.items()}
                lat32 = lambda m, c, top: Cv.conv2d(c, m.weight, m.bias, m.stride, m.padding, residual=Cv.upsample2x(top))

                def seg_trunk():
                    c = {l: act16.unpack(m) for l, m in c16.items()}
                    p5 = fpn.P5_conv1(c[5])
                    p4 = lat32(fpn.P4_conv1, c[4], p5)
                    p3 = lat32(fpn.P3_conv1, c[3], p4)
                    p2 = lat32(fpn.P2_conv1, c[2], p3)
                    p5, p4, p3, p2 = fpn.P5_conv2(p5), fpn.P4_conv2(p4), fpn.P3_conv2(p3), fpn.P2_conv2(p2)
                    p6 = fpn.P6(p5)
                    return [p2, p3, p4, p5], [rpn(p) for p in (p2, p3, p4, p5, p6)]

                def seg_pyramid():
                    ps = fpn._pyramid16(c16)
                    return [act16.unpack(p) for p in ps[:4]], [rpn(p) for p in ps]

                (pa, ra), (pb, rb) = seg_trunk(), seg_pyramid()
                agree = [float((b - a).norm() / a.norm()) for a, b in zip(pa, pb)]
                agree_rpn = [float((b[2] - a[2]).norm() / a[2].norm()) for a, b in zip(ra, rb)]
                del pa, ra, pb, rb
                emit()
                emit("== %s, %d x %d^2 (c2 %d x 256 x %d x %d)" % (prec, n, size, n, hw, hw))
                emit("  |new - old| / |old|: p2..p5 %s   rpn bbox p2..p6 %s" % (
                    " ".join("%.1e" % v for v in agree), " ".join("%.1e" % v for v in agree_rpn)))
                compare("(a) segment: 16-bit c2..c5 -> RPN outputs + fp32 p2..p5", seg_trunk, seg_pyramid)

                if not args.skip_model:
                    batch = synthetic_batch(n, size, device=dev, seed=2000)
                    model.external_proposals = SyntheticProposals(batch[2], size, seed=7, cycle=1)
                    windows = torch.tensor([[0, 0, size, size]] * n, dtype=torch.float32)

                    def infer(scope):
                        cfg.MODEL.ACT_SCOPE = scope
                        return model([batch[0], windows], mode='inference')

                    mo, mn, aa = compare("(a) whole model _inference", lambda: infer("trunk"), lambda: infer("pyramid"))
                    verdicts.append(mn <= mo * (1.0 + aa))
                    del cfg.MODEL.ACT_SCOPE
                    Cv.prepare_step(model)

                if not args.skip_layers:
                    emit("  (b) per layer: level N H W Cin Cout | old ms | new ms | old / new   [(c): new MB, GB/s]")
                    tot_old = tot_new = 0.0

                    def layer(what, lvl, shape, old, new, nbytes=None):
                        nonlocal tot_old, tot_new
                        t = _alternate([("old", old), ("new", new)])
                        mo, mn = statistics.median(t["old"]), statistics.median(t["new"])
                        tot_old += mo
                        tot_new += mn
                        extra = "" if nbytes is None else "   [%7.1f MB %6.0f GB/s]" % (nbytes / 1e6, nbytes / mn / 1e6)
                        emit("    %-9s p%d %d %3d %3d %4d %3d | %7.3f | %7.3f | %5.2f%s%s" % (
                            (what, lvl) + shape + (mo, mn, mo / mn, extra, "" if mn <= mo else "   <- loses")))

                    p16 = {l: act16.pack(torch.randn(n, 256, s, s, device=dev), dtype) for l, s in sides.items()}
                    p16[6] = p16[5][:, :, ::2, ::2].contiguous(memory_format=torch.channels_last)
                    p32 = {l: act16.unpack(m) for l, m in p16.items()}
                    c32 = {l: act16.unpack(m) for l, m in c16.items()}
                    for l, m in ((4, fpn.P4_conv1), (3, fpn.P3_conv1), (2, fpn.P2_conv1)):
                        s, cin = sides[l], 64 << l
                        P = n * s * s
                        layer("lateral", l, (n, s, s, cin, 256), lambda: lat32(m, c32[l], p32[l + 1]),
                              lambda: pyr16.lateral16(c16[l], m, p16[l + 1]),
                              2.0 * (P * cin + P * 256 + P // 4 * 256 + 256 * cin))
                    for l, m in ((5, fpn.P5_conv2), (4, fpn.P4_conv2), (3, fpn.P3_conv2), (2, fpn.P2_conv2)):
                        layer("smoothing", l, (n, sides[l], sides[l], 256, 256), lambda: m(p32[l]),
                              lambda: pyr16.conv_bias_act16(p16[l], m[1]))
                    cs = rpn.conv_shared
                    for l in (2, 3, 4, 5, 6):
                        s = p16[l].shape[2]
                        layer("shared", l, (n, s, s, 256, 512),
                              lambda: Cv.conv_bias_relu(p32[l], cs.weight, cs.bias, cs.stride, cs.padding),
                              lambda: pyr16.conv_bias_act16(p16[l], cs, relu=True))
                    wh = torch.cat((rpn.conv_class.weight, rpn.conv_bbox.weight), 0)
                    bh = torch.cat((rpn.conv_class.bias, rpn.conv_bbox.bias), 0)
                    ncls = rpn.conv_class.weight.shape[0]
                    for l in (2, 3, 4, 5, 6):
                        s = p16[l].shape[2]
                        h32 = torch.relu(torch.randn(n, 512, s, s, device=dev))
                        h16 = act16.pack(h32, dtype)

                        def heads_old():
                            both = Cv.conv2d(h32, wh, bh)
                            return (both[:, :ncls].permute(0, 2, 3, 1).contiguous(), both[:, ncls:].permute(0, 2, 3, 1).contiguous())

                        P = n * s * s
                        layer("heads", l, (n, s, s, 512, wh.shape[0]), heads_old, lambda: pyr16.head1x1_16(h16, wh, bh),
                              2.0 * P * 512 + 4.0 * P * wh.shape[0] + 2.0 * wh.shape[0] * 512)
                        del h32, h16
                    t = _alternate([("old", lambda: [act16.unpack(m) for m in c16.values()]),
                                    ("new", lambda: [act16.unpack(p16[l]) for l in (2, 3, 4, 5)])])
                    mo, mn = statistics.median(t["old"]), statistics.median(t["new"])
                    tot_old += mo
                    tot_new += mn
                    emit("    4 unpacks: c2..c5 (256..2048 channels) %7.3f | p2..p5 (256 channels) %7.3f | %5.2f" % (mo, mn, mo / mn))
                    emit("    sum of the medians above: old %.3f ms, new %.3f ms" % (tot_old, tot_new))
                    del p16, p32, c32
            Cv.set_conv_precision("fp32")
            del model, fpn, rpn, c16
            torch.cuda.empty_cache()
    if verdicts:
        emit()
        emit("requirement (whole _inference with 'pyramid' not slower than 'trunk' by more than the A/A spread of the same "
             "comparison, at every shape and type): %s" % ("met" if all(verdicts) else "NOT met"))


if __name__ == "__main__":
    main()
