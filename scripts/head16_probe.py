"""What MODEL.ACT_SCOPE = 'detect' (the box and mask heads on 16-bit channels-last crops, feature_intertwiner_amd/head16.py)
costs and saves against scope 'roi' (fp32 NCHW crops, both heads and the feature extractor on fp32 tensors; unchanged by
'detect', bit for bit and launch for launch), for bf16 and fp16, ResNet-101 at 2 x 1344^2 with 1000 RoIs per image and
4 x 1024^2 with 512, 100 detections per image.  MODEL.CONV_PRECISION and MODEL.ACT_PRECISION are the type in every arm.

In ONE process on one MI355X, the arms alternating round by round, each call timed with a HIP event pair, 5 warm-up and 20
timed rounds per arm, median / min / max.  Every comparison carries an A/A line: the old arm runs TWICE per round under two
names, and |median - median| / median of the two is the spread a difference has to exceed to mean anything.
  (a) the two crop launches: fi_head16_pyramid_crop_forward (16-bit channels-last out) against fi_roi16_pyramid_crop_forward
      (fp32 NCHW out) on the same 16-bit make-up maps and boxes -- 7x7 on the proposals, 14x14 on the detections; the crops are
      compared bit for bit first;
  (b) every head launch against the layer it replaces, each on its own input: the full-window 12544 -> 1024 layer (its own
      line: 256 workgroups of 196 K blocks, about one per CU, no split over K), the 1x1 1024 -> 1024 layer, the stacked
      405-column output; the mask head's four 3x3 layers, the transposed convolution as a 1x1 layer, and conv5 + sigmoid +
      pixel shuffle (old: conv5, sigmoid, permute copy);
  (c) the segment from the 16-bit make-up maps to the three outputs: 'roi' = Dev on the proposals (7x7 and 14x14 crops, host
      read, feature extractor), box head, Dev on the detections, mask head; 'detect' = crop, box head, crop, mask head.  The
      detections are the same seeded boxes in both arms (detection_layer is not part of the segment);
  (d) the whole model's _inference under both scopes, and torch.cuda.max_memory_allocated of one call of each.
A piece that loses is marked; nothing falls back.  No rocprofv3 pass of the new kernels is taken here.

    python scripts/head16_probe.py [--out profiles/head16_probe.txt] [--types bf16,fp16] [--skip-model]
"""
import argparse
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, ROUNDS = 5, 20
SHAPES = ((2, 1344, 1000), (4, 1024, 512))          # (images, image size, RoIs per image)
DETECTIONS = 100


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


def _rois(n, per_image, seed):
    """[n, per_image, 4] normalised boxes: side log-uniform in [1/32, 1] of the image (the FPN rule then spreads them over
    p2..p5), aspect in [1/2, 2], centres uniform; clipped to the image as the proposal layer's are."""
    rs = np.random.RandomState(seed)
    m = n * per_image
    side = np.exp(rs.uniform(np.log(1.0 / 32), 0.0, m))
    aspect = np.exp(rs.uniform(np.log(0.5), np.log(2.0), m))
    h, w = side * np.sqrt(aspect), side / np.sqrt(aspect)
    cy, cx = rs.uniform(0, 1, m), rs.uniform(0, 1, m)
    b = np.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], 1).clip(0.0, 1.0).astype(np.float32)
    return torch.from_numpy(b).view(n, per_image, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head16_probe.txt"))
    ap.add_argument("--types", default="bf16,fp16")
    ap.add_argument("--skip-model", action="store_true", help="leave out the whole model's _inference")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    from feature_intertwiner_amd import act16, head16, roi16
    from feature_intertwiner_amd import conv as Cv
    from feature_intertwiner_amd.config import make_config
    from feature_intertwiner_amd.intertwiner import roi_level
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

    emit("head16_probe: box and mask heads on 16-bit channels-last crops (ACT_SCOPE 'detect') vs fp32 NCHW crops and fp32 "
         "head tensors (ACT_SCOPE 'roi'), ResNet-101, %s" % torch.cuda.get_device_name(0))
    emit("%d timed rounds per arm after %d warm-up rounds, arms alternating in one process, HIP events; ms" % (ROUNDS, WARMUP))
    emit("clocks as found: %s" % _clocks())
    losers = []
    where = [""]          # "type, shape" of the configuration being measured, for the summary line

    def compare(title, old, new, indent="  "):
        """old twice (A/A) and new, alternating; returns (median old, median new, A/A spread as a fraction)."""
        t = _alternate([("old", old), ("new", new), ("old again", old)])
        mo, mn, mo2 = (statistics.median(t[k]) for k in ("old", "new", "old again"))
        aa = abs(mo - mo2) / mo
        lost = mn > mo * (1.0 + aa)
        emit("%s%-58s old %8.3f [%7.3f, %7.3f]  new %8.3f [%7.3f, %7.3f]  new / old %.3f  A/A %.3f%s" % (
            indent, title, mo, min(t["old"]), max(t["old"]), mn, min(t["new"]), max(t["new"]), mn / mo, aa,
            "   <- loses by more than the A/A spread" if lost else ""))
        if lost:
            losers.append("%s: %s %.3f -> %.3f (%.3f)" % (where[0], title, mo, mn, mn / mo))
        return mo, mn, aa

    for prec in args.types.split(","):
        dtype = act16.dtype_of(prec)
        for n, size, per_image in SHAPES:
            torch.manual_seed(2000)
            cfg = make_config("resnet101", size, n, 1000, conv_precision=prec)
            cfg.MODEL.ACT_PRECISION = prec
            cfg.MODEL.ACT_SCOPE = "roi"
            cfg.RPN.POST_NMS_ROIS_INFERENCE = per_image
            model = MaskRCNN(cfg).to(dev).eval()
            dev_roi, box, mask = model.dev_roi, model.classifier, model.mask
            hw = size // 4
            sides = [hw, hw // 2, hw // 4, hw // 8]
            Cv.set_conv_precision(prec)
            with torch.no_grad():
                Cv.prepare_step(model)          # BatchNorm folds, channels-last weights and their 16-bit copies, as _inference does
                p16 = [act16.pack(torch.randn(n, 256, s, s, device=dev), dtype) for s in sides]
                up16 = dev_roi.make_up_maps(p16)
                rois, dets = _rois(n, per_image, 11).to(dev), _rois(n, DETECTIONS, 12).to(dev)
                area = float(size * size)

                def rows(r):
                    b = r.reshape(-1, 4).contiguous()
                    ind = torch.arange(n, device=dev, dtype=torch.int32).repeat_interleave(r.shape[1])
                    return b, ind, roi_level(b, area, cfg.ROIS.ASSIGN_ANCHOR_BASE).contiguous()

                where[0] = "%s, %d x %d^2" % (prec, n, size)
                emit()
                emit("== %s, %d x %d^2 (p2 %d x 256 x %d x %d), %d RoIs and %d detections per image" % (
                    prec, n, size, n, hw, hw, per_image, DETECTIONS))

                # (a) the crop launches
                emit("  (a) crop launches on the 16-bit make-up maps (old: fi_roi16, fp32 NCHW out; new: fi_head16, 16-bit NHWC out)")
                crops = {}
                for c, r, what in ((7, rois, "proposals"), (14, dets, "detections")):
                    b, ind, lvl = rows(r)
                    old = lambda: roi16.pyramid_crop16(up16, b, ind, lvl, c, c)
                    new = lambda: head16.pyramid_crop16_cl(up16, b, ind, lvl, c, c)
                    same = torch.equal(old().to(dtype).view(torch.int16), new().contiguous().view(torch.int16))
                    elems = b.shape[0] * 256 * c * c
                    compare("%dx%d, %d %s (%.1f -> %.1f MB written) bit-equal %s" % (
                        c, c, b.shape[0], what, elems * 4 / 1e6, elems * 2 / 1e6, same), old, new, "    ")
                    crops[c] = (old(), new())

                # (b) every head launch against the layer it replaces
                emit("  (b) head launches, each on its own input (old: the fp32-tensor layer under CONV_PRECISION = %s)" % prec)
                x32, x16 = crops[7]
                N7 = x32.shape[0]
                compare("box conv1 full-window 12544 -> 1024 + BN + ReLU, %d rows" % N7,
                        lambda: Cv.conv_bn_act(x32, box.conv1, box.bn1, relu=True),
                        lambda: head16.window_bn_act16(x16, box.conv1, box.bn1, relu=True), "    ")
                y32, y16 = Cv.conv_bn_act(x32, box.conv1, box.bn1, relu=True), head16.window_bn_act16(x16, box.conv1, box.bn1)
                compare("box conv2 1x1 1024 -> 1024 + BN + ReLU",
                        lambda: Cv.conv_bn_act(y32, box.conv2, box.bn2, relu=True),
                        lambda: head16.conv_bn_act16(y16, box.conv2, box.bn2, relu=True), "    ")
                z32 = Cv.conv_bn_act(y32, box.conv2, box.bn2, relu=True).view(-1, 1024)
                z16 = head16.conv_bn_act16(y16, box.conv2, box.bn2, relu=True)
                nc = box.linear_class.weight.shape[0]

                def out_old():
                    h = Cv.linear(z32, torch.cat((box.linear_class.weight, box.linear_bbox.weight), 0),
                                  torch.cat((box.linear_class.bias, box.linear_bbox.bias), 0))
                    return h[:, :nc].contiguous(), h[:, nc:].contiguous()

                def out_new():
                    w, bs = head16.stacked_linear16((box.linear_class, box.linear_bbox), dtype)
                    h = head16.out1x1_16(z16, w, bs)
                    return h[:, :nc].contiguous(), h[:, nc:].contiguous()

                compare("box output 1024 -> 405 (stacked class + box), slices", out_old, out_new, "    ")
                m32, m16 = crops[14]
                for i, (cv, bn) in enumerate(((mask.conv1, mask.bn1), (mask.conv2, mask.bn2), (mask.conv3, mask.bn3),
                                              (mask.conv4, mask.bn4))):
                    compare("mask conv%d 3x3 256 -> 256 + BN + ReLU on %d x 14 x 14" % (i + 1, m32.shape[0]),
                            lambda: Cv.conv_bn_act(m32, cv, bn, relu=True),
                            lambda: head16.conv_bn_act16(m16, cv, bn, relu=True), "    ")
                    m32, m16 = Cv.conv_bn_act(m32, cv, bn, relu=True), head16.conv_bn_act16(m16, cv, bn, relu=True)
                compare("mask deconv as 1x1 256 -> 1024 + bias + ReLU",
                        lambda: mask.deconv.forward_unshuffled(m32, relu=True),
                        lambda: head16.deconv2x2_act16(m16, mask.deconv, relu=True), "    ")
                u32, u16 = mask.deconv.forward_unshuffled(m32, relu=True), head16.deconv2x2_act16(m16, mask.deconv, relu=True)

                def last_old():
                    nn_, h, w = u32.shape[0], u32.shape[4], u32.shape[5]
                    y = torch.sigmoid(mask.conv5(u32.view(nn_ * 4, u32.shape[3], h, w))).view(nn_, 2, 2, -1, h, w)
                    return y.permute(0, 3, 4, 1, 5, 2).reshape(nn_, y.shape[3], 2 * h, 2 * w)

                last_new = lambda: head16.out1x1_16(u16, mask.conv5.weight, mask.conv5.bias, act=head16.SIGMOID,
                                                    layout=head16.SHUFFLE)
                emit("    |new - old| / |old| of the masks of this chain: %.1e" % float((last_new() - last_old()).norm() / last_old().norm()))
                compare("mask conv5 256 -> 81 + sigmoid + pixel shuffle", last_old, last_new, "    ")
                del x32, x16, y32, y16, z32, z16, m32, m16, u32, u16, crops

                # (c) the segment: 16-bit make-up maps -> class probabilities, boxes, masks
                def seg_roi():
                    pooled, _, feat = dev_roi(p16, rois, up_maps=up16)
                    so, sg = feat if feat else (None, None)
                    _, probs, bbox = box(pooled, so, sg)
                    _, pm, _ = dev_roi(p16, dets, up_maps=up16)
                    return probs, bbox, mask(pm)

                def seg_detect():
                    _, probs, bbox = box(dev_roi.crop16(p16, rois, 7, up_maps=up16))
                    return probs, bbox, mask(dev_roi.crop16(p16, dets, 14, up_maps=up16))

                a, b_ = seg_roi(), seg_detect()
                emit("  |new - old| / |old|: probs %.1e  bbox %.1e  masks %.1e" % tuple(
                    float((y - x).norm() / x.norm()) for x, y in zip(a, b_)))
                del a, b_
                compare("(c) segment: 16-bit make-up maps -> probs, bbox, masks", seg_roi, seg_detect)

                # (d) the whole model
                if not args.skip_model:
                    batch = synthetic_batch(n, size, device=dev, seed=2000)
                    model.external_proposals = SyntheticProposals(batch[2], size, seed=7, cycle=1)
                    windows = torch.tensor([[0, 0, size, size]] * n, dtype=torch.float32)

                    def infer(scope):
                        cfg.MODEL.ACT_SCOPE = scope
                        return model([batch[0], windows], mode='inference')

                    compare("(d) whole model _inference", lambda: infer("roi"), lambda: infer("detect"))
                    peak = {}
                    for scope in ("roi", "detect"):
                        torch.cuda.synchronize()
                        torch.cuda.empty_cache()
                        torch.cuda.reset_peak_memory_stats()
                        base = torch.cuda.memory_allocated()
                        infer(scope)
                        torch.cuda.synchronize()
                        peak[scope] = (torch.cuda.max_memory_allocated(), base)
                    emit("  max_memory_allocated of one _inference call: roi %.1f MB, detect %.1f MB (allocated before the "
                         "call: %.1f MB)" % (peak["roi"][0] / 1e6, peak["detect"][0] / 1e6, peak["detect"][1] / 1e6))
            Cv.set_conv_precision("fp32")
            del model, dev_roi, box, mask, p16, up16
            torch.cuda.empty_cache()
    emit()
    emit("launches and segments that lose by more than their A/A spread (old -> new ms, new / old):%s"
         % ("" if losers else " none"))
    for l in losers:
        emit("  " + l)


if __name__ == "__main__":
    main()
