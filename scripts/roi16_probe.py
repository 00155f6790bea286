"""What MODEL.ACT_SCOPE = 'roi' (the Dev stage's make-up layer and RoIAlign on 16-bit channels-last maps,
feature_intertwiner_amd/roi16.py) costs and saves against scope 'pyramid' (p2..p5 unpacked to fp32 NCHW behind the RPN, the
make-up pass run once per Dev call), for bf16 and fp16, ResNet-101 at 2 x 1344^2 with 1000 RoIs per image and 4 x 1024^2 with
512.  MODEL.CONV_PRECISION and MODEL.ACT_PRECISION are the type in every arm.

In ONE process on one MI355X, the arms alternating round by round, each call timed with a HIP event pair, 5 warm-up and 20
timed rounds per arm, median / min / max.  Every comparison carries an A/A line: the old arm runs TWICE per round under two
names, and |median - median| / median of the two is the spread a difference has to exceed to mean anything.
  (a) the RoIAlign launch: fi_roi16_pyramid_crop_forward on the 16-bit maps against fi_pyramid_crop_forward_nhwc on the same
      maps widened to fp32 channels-last, same boxes (a seeded generator, levels by the FPN rule), 7x7 and 14x14; the crops are
      compared bit for bit first;
  (b) the make-up layer per level: conv_bn_act of the conv precision (fp32 in, fp32 channels-last out) against conv_bn_act16;
  (c) the segment from the 16-bit p2..p5 to the mask head's input: 'pyramid' = 4 unpacks, Dev on the proposals, Dev on the
      detections (the make-up pass twice); 'roi' = the make-up pass once, Dev on the proposals, Dev on the detections;
  (d) the whole model's _inference under both scopes, and torch.cuda.max_memory_allocated of one call of each.
A piece that loses is marked; nothing falls back.  No rocprofv3 pass of the new kernel is taken here.

    python scripts/roi16_probe.py [--out profiles/roi16_probe.txt] [--types bf16,fp16] [--skip-model]
"""
import argparse
import ctypes
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roi16_probe.txt"))
    ap.add_argument("--types", default="bf16,fp16")
    ap.add_argument("--skip-model", action="store_true", help="leave out the whole model's _inference")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    from feature_intertwiner_amd import _lib, act16, roi16
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

    emit("roi16_probe: make-up layer and RoIAlign on 16-bit channels-last maps (ACT_SCOPE 'roi') vs fp32 maps behind four "
         "unpacks (ACT_SCOPE 'pyramid'), ResNet-101, %s" % torch.cuda.get_device_name(0))
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

    L32 = _lib.load()
    for prec in args.types.split(","):
        dtype = act16.dtype_of(prec)
        for n, size, per_image in SHAPES:
            torch.manual_seed(2000)
            cfg = make_config("resnet101", size, n, 1000, conv_precision=prec)
            cfg.MODEL.ACT_PRECISION = prec
            cfg.RPN.POST_NMS_ROIS_INFERENCE = per_image
            model = MaskRCNN(cfg).to(dev).eval()
            dev_roi = model.dev_roi
            hw = size // 4
            sides = [hw, hw // 2, hw // 4, hw // 8]
            Cv.set_conv_precision(prec)
            with torch.no_grad():
                Cv.prepare_step(model)          # BatchNorm folds, channels-last weights and their 16-bit copies, as _inference does
                p16 = [act16.pack(torch.randn(n, 256, s, s, device=dev), dtype) for s in sides]
                seq = dev_roi.upsample[0]
                rois = _rois(n, per_image, 11).to(dev)
                dets = _rois(n, DETECTIONS, 12).to(dev)
                boxes = rois.reshape(-1, 4).contiguous()
                box_ind = torch.arange(n, device=dev, dtype=torch.int32).repeat_interleave(per_image)
                level = dev_roi.level_info(rois)[0].contiguous()
                counts = [int((level == l).sum()) for l in (2, 3, 4, 5)]
                emit()
                emit("== %s, %d x %d^2 (p2 %d x 256 x %d x %d), %d RoIs per image, per level p2..p5 %s" % (
                    prec, n, size, n, hw, hw, per_image, counts))

                # (a) the RoIAlign launch on the make-up maps
                up16 = dev_roi.make_up_maps(p16)
                up32 = [u.float() for u in up16]                        # widened, still channels-last
                nl, N = 4, boxes.shape[0]
                hs, ws = (ctypes.c_int * nl)(*sides), (ctypes.c_int * nl)(*sides)
                t32 = (ctypes.c_void_p * nl)(*[u.data_ptr() for u in up32])
                emit("  (a) RoIAlign launch, %d boxes x 256 channels: crop | old ms | new ms | old / new | crops MB | tap MB "
                     "old -> new (4 taps per output element, before any cache)" % N)
                for c in (7, 14):
                    out32 = torch.empty((N, 256, c, c), device=dev)

                    def crop_old():
                        _lib.check(L32.fi_pyramid_crop_forward_nhwc(
                            t32, hs, ws, nl, _lib.ptr(boxes), _lib.ptr(box_ind), _lib.ptr(level), N, n, 256, c, c, 0.0,
                            _lib.ptr(out32), _lib.current_stream()), "fi_pyramid_crop_forward_nhwc")
                        return out32

                    crop_new = lambda: roi16.pyramid_crop16(up16, boxes, box_ind, level, c, c)
                    same = torch.equal(crop_old().view(torch.int32), crop_new().view(torch.int32))
                    t = _alternate([("old", crop_old), ("new", crop_new), ("old again", crop_old)])
                    mo, mn, mo2 = (statistics.median(t[k]) for k in ("old", "new", "old again"))
                    elems = N * 256 * c * c
                    emit("    %2dx%-2d | %7.3f | %7.3f | %5.2f | %7.1f | %7.1f -> %7.1f   A/A %.3f   bit-equal %s%s" % (
                        c, c, mo, mn, mo / mn, elems * 4 / 1e6, elems * 16 / 1e6, elems * 8 / 1e6, abs(mo - mo2) / mo, same,
                        "" if mn <= mo else "   <- loses"))
                    del out32

                # (b) the make-up layer per level
                p32 = [act16.unpack(p) for p in p16]
                emit("  (b) make-up layer 3x3 256 -> 256 + BatchNorm + ReLU: level N H W | old ms | new ms | old / new")
                tot_old = tot_new = 0.0
                for l, s in enumerate(sides):
                    t = _alternate([("old", lambda: Cv.conv_bn_act(p32[l], seq[0], seq[1], relu=True, channels_last_out=True)),
                                    ("new", lambda: act16.conv_bn_act16(p16[l], seq[0], seq[1], relu=True))])
                    mo, mn = statistics.median(t["old"]), statistics.median(t["new"])
                    tot_old += mo
                    tot_new += mn
                    emit("    p%d %d %3d %3d | %7.3f | %7.3f | %5.2f%s" % (l + 2, n, s, s, mo, mn, mo / mn,
                                                                         "" if mn <= mo else "   <- loses"))
                emit("    one pass over p2..p5 (sum of the medians): old %.3f ms, new %.3f ms" % (tot_old, tot_new))
                del p32, up32, up16

                # (c) the segment: 16-bit p2..p5 -> the mask head's input
                def seg_pyramid():
                    maps = [act16.unpack(p) for p in p16]
                    pooled, _, feat = dev_roi(maps, rois)
                    _, mask, _ = dev_roi(maps, dets)
                    return pooled, feat, mask

                def seg_roi():
                    up = dev_roi.make_up_maps(p16)
                    pooled, _, feat = dev_roi(p16, rois, up_maps=up)
                    _, mask, _ = dev_roi(p16, dets, up_maps=up)
                    return pooled, feat, mask

                (pa, _, ma), (pb, _, mb) = seg_pyramid(), seg_roi()
                emit("  |new - old| / |old|: 7x7 crops %.1e   14x14 crops of the detections %.1e" % (
                    float((pb - pa).norm() / pa.norm()), float((mb - ma).norm() / ma.norm())))
                del pa, ma, pb, mb
                mo, mn, aa = compare("(c) segment: 16-bit p2..p5 -> pooled 7x7, feature branch, mask head's 14x14 input",
                                     seg_pyramid, seg_roi)
                verdicts.append(mn < mo * (1.0 - aa))

                # (d) the whole model
                if not args.skip_model:
                    batch = synthetic_batch(n, size, device=dev, seed=2000)
                    model.external_proposals = SyntheticProposals(batch[2], size, seed=7, cycle=1)
                    windows = torch.tensor([[0, 0, size, size]] * n, dtype=torch.float32)

                    def infer(scope):
                        cfg.MODEL.ACT_SCOPE = scope
                        return model([batch[0], windows], mode='inference')

                    compare("(d) whole model _inference", lambda: infer("pyramid"), lambda: infer("roi"))
                    peak = {}
                    for scope in ("pyramid", "roi"):
                        torch.cuda.synchronize()
                        torch.cuda.empty_cache()
                        torch.cuda.reset_peak_memory_stats()
                        base = torch.cuda.memory_allocated()
                        infer(scope)
                        torch.cuda.synchronize()
                        peak[scope] = (torch.cuda.max_memory_allocated(), base)
                    emit("  max_memory_allocated of one _inference call: pyramid %.1f MB, roi %.1f MB (allocated before the "
                         "call: %.1f MB)" % (peak["pyramid"][0] / 1e6, peak["roi"][0] / 1e6, peak["roi"][1] / 1e6))
                    del cfg.MODEL.ACT_SCOPE
            Cv.set_conv_precision("fp32")
            del model, dev_roi, p16
            torch.cuda.empty_cache()
    emit()
    emit("requirement (the segment under 'roi' faster than under 'pyramid' by more than the A/A spread of the same "
         "comparison, at every shape and type): %s" % ("met" if all(verdicts) else "NOT met"))


if __name__ == "__main__":
    main()
