"""What MODEL.ACT_PRECISION (the ResNet trunk on 16-bit channels-last tensors, feature_intertwiner_amd/act16.py) costs and
saves against the existing 16-bit path (MODEL.CONV_PRECISION: 16-bit MFMA operands, fp32 NCHW tensors), for bf16 and fp16.

In ONE process on one MI355X, the two arms alternating round by round, each call timed with a HIP event pair, 5 warm-up and
20 timed rounds per arm, median / min / max:
  (a) CONV_PRECISION = <type>, fp32 tensors      -- the path before this switch existed
  (b) ACT_PRECISION  = <type>                    -- pack once, C2..C5 on 16-bit tensors, four unpacks
1. the ResNet-101 trunk forward from the pooled C1 map to fp32 NCHW c2..c5 (pack / unpack inside arm (b)), at 2 x 1344^2
   (pooled map 2 x 64 x 336 x 336) and 4 x 1024^2 (4 x 64 x 256 x 256);
2. per distinct trunk layer shape: fi_act16_conv_forward against fi_conv2d_forward_live_<type> on the same shape (conv +
   folded BatchNorm + ReLU, no shortcut), with the bytes each must move computed from the shapes (x + y in the tensor type,
   w in 16 bits);
3. the whole model's _inference both ways, and torch.cuda.max_memory_allocated of one call both ways.
"spread" is max - min over an arm's rounds.  Verdict per shape: (b) is not slower than (a) by more than 1.5 % (the box
noise DESIGN records).

    python scripts/act16_probe.py [--out profiles/act16_probe.txt] [--types bf16,fp16] [--skip-model]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, ROUNDS = 5, 20
SHAPES = ((2, 1344), (4, 1024))          # (images, image size)


def _timed(fn, *a):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn(*a)
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


def _layer_shapes(resnet, n, hw):
    """[(N, H, W, Cin, Cout, k, stride), count] of the trunk's convolutions on a pooled map of hw x hw, in order of first use."""
    seen, order = {}, []
    h = hw
    for stage in (resnet.C2, resnet.C3, resnet.C4, resnet.C5):
        for block in stage:
            s = block.stride
            rows = [(n, h, h, block.conv1.in_channels, block.conv1.out_channels, 1, s)]
            ho = (h - 1) // s + 1
            rows.append((n, ho, ho, block.conv2.in_channels, block.conv2.out_channels, 3, 1))
            rows.append((n, ho, ho, block.conv3.in_channels, block.conv3.out_channels, 1, 1))
            if block.downsample is not None:
                d = block.downsample[0]
                rows.append((n, h, h, d.in_channels, d.out_channels, 1, s))
            for r in rows:
                if r not in seen:
                    seen[r] = 0
                    order.append(r)
                seen[r] += 1
            h = ho
    return [(r, seen[r]) for r in order]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "act16_probe.txt"))
    ap.add_argument("--types", default="bf16,fp16")
    ap.add_argument("--skip-model", action="store_true", help="leave out part 3 (the whole model's _inference)")
    ap.add_argument("--skip-layers", action="store_true", help="leave out part 2 (the per-layer table)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    from feature_intertwiner_amd import act16
    from feature_intertwiner_amd import conv as Cv
    from feature_intertwiner_amd.config import make_config
    from feature_intertwiner_amd.model import MaskRCNN
    from feature_intertwiner_amd.sub_module import _bn
    from feature_intertwiner_amd.synthetic import SyntheticProposals, synthetic_batch
    dev = "cuda:0"
    lines = []

    def emit(line=""):
        lines.append(line)
        print(line, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:          # kept current: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")

    emit("act16_probe: ResNet-101 trunk on 16-bit channels-last tensors (ACT_PRECISION) vs 16-bit operands on fp32 tensors "
         "(CONV_PRECISION), %s" % torch.cuda.get_device_name(0))
    emit("%d timed rounds per arm after %d warm-up rounds, arms alternating in one process, HIP events; ms" % (ROUNDS, WARMUP))
    verdicts = []
    for prec in args.types.split(","):
        dtype = act16.dtype_of(prec)
        for n, size in SHAPES:
            torch.manual_seed(2000)
            cfg = make_config("resnet101", size, n, 1000, conv_precision=prec)
            model = MaskRCNN(cfg).to(dev).eval()
            fpn = model.fpn
            stages = [fpn.C2, fpn.C3, fpn.C4, fpn.C5]
            hw = size // 4
            Cv.set_conv_precision(prec)
            with torch.no_grad():
                Cv.prepare_step(model)          # BatchNorm folds, channels-last weights and their 16-bit copies, as _inference does
                x = torch.relu(torch.randn(n, 64, hw, hw, device=dev))          # a pooled C1 map: non-negative

                def arm_a():
                    out, m = [], x
                    for st in stages:
                        m = st(m)
                        out.append(m)
                    return out

                def arm_b():
                    out, m = [], act16.pack(x, dtype)
                    for st in stages:
                        m = st(m)
                        out.append(act16.unpack(m))
                    return out

                ya, yb = arm_a(), arm_b()
                agree = [float((b - a).norm() / a.norm()) for a, b in zip(ya, yb)]
                del ya, yb
                t = _alternate([("a", arm_a), ("b", arm_b)])
                emit()
                emit("== %s, %d x %d^2: trunk forward, pooled map %d x 64 x %d x %d -> fp32 NCHW c2..c5" % (prec, n, size, n, hw, hw))
                for name, label in (("a", "(a) CONV_PRECISION, fp32 tensors"), ("b", "(b) ACT_PRECISION, pack + 4 unpack in")):
                    emit("  %-38s median %8.3f  min %8.3f  max %8.3f  spread %6.3f" % ((label,) + _row(t[name])))
                ma, mb = statistics.median(t["a"]), statistics.median(t["b"])
                ok = mb <= 1.015 * ma
                verdicts.append(ok)
                emit("  (b) / (a) = %.3f  ->  %s" % (mb / ma, "not slower than (a) + 1.5 %" if ok else "SLOWER than (a) by more than 1.5 %"))
                emit("  |c_b - c_a| / |c_a| per level c2..c5: %s" % "  ".join("%.2e" % v for v in agree))

                if not args.skip_layers:
                    emit("  per distinct layer shape (conv + folded BN + ReLU): N H W Cin Cout k stride x count | new ms, MB, GB/s, "
                         "TFLOP/s | old ms, MB, GB/s | old / new")
                    tot_new = tot_old = 0.0
                    for (N, H, W, Cin, Cout, k, s), count in _layer_shapes(fpn, n, hw):
                        conv = Cv.Conv2d(Cin, Cout, kernel_size=k, stride=s, padding=(k - 1) // 2).to(dev)
                        # channels-last, as prepare_step stores a model's weights: the tap-major view is free in both arms
                        conv.weight.data = conv.weight.data.contiguous(memory_format=torch.channels_last)
                        bn = _bn(Cout).to(dev).eval()
                        x32 = torch.relu(torch.randn(N, Cin, H, W, device=dev))
                        x16 = act16.pack(x32, dtype)
                        OH = (H - 1) // s + 1
                        new = lambda: act16.conv_bn_act16(x16, conv, bn, relu=True)
                        old = lambda: Cv.conv_bn_act(x32, conv, bn, relu=True)
                        tl = _alternate([("new", new), ("old", old)])
                        mn, mo = statistics.median(tl["new"]), statistics.median(tl["old"])
                        elems = N * H * W * Cin + N * OH * OH * Cout
                        wbytes = 2.0 * Cout * Cin * k * k
                        b_new, b_old = 2.0 * elems + wbytes, 4.0 * elems + wbytes
                        flops = 2.0 * N * OH * OH * Cout * Cin * k * k
                        tot_new += count * mn
                        tot_old += count * mo
                        emit("    %d %3d %3d %4d %4d %d %d x%2d | %7.3f %7.1f %6.0f %6.1f | %7.3f %7.1f %6.0f | %5.2f%s" % (
                            N, H, W, Cin, Cout, k, s, count, mn, b_new / 1e6, b_new / mn / 1e6, flops / mn / 1e9,
                            mo, b_old / 1e6, b_old / mo / 1e6, mo / mn, "" if mn <= mo else "   <- loses"))
                        del x32, x16, conv, bn
                    emit("    sum over the trunk's layers (count x median): new %.3f ms, old %.3f ms" % (tot_new, tot_old))

                if not args.skip_model:
                    batch = synthetic_batch(n, size, device=dev, seed=2000)
                    model.external_proposals = SyntheticProposals(batch[2], size, seed=7, cycle=1)
                    windows = torch.tensor([[0, 0, size, size]] * n, dtype=torch.float32)

                    def infer(act):
                        if act:
                            cfg.MODEL.ACT_PRECISION = prec
                        elif hasattr(cfg.MODEL, "ACT_PRECISION"):
                            del cfg.MODEL.ACT_PRECISION
                        return model([batch[0], windows], mode='inference')

                    tm = _alternate([("a", lambda: infer(False)), ("b", lambda: infer(True))])
                    peak = {}
                    for name, act in (("a", False), ("b", True)):
                        torch.cuda.synchronize()
                        torch.cuda.empty_cache()
                        torch.cuda.reset_peak_memory_stats()
                        base = torch.cuda.memory_allocated()
                        infer(act)
                        torch.cuda.synchronize()
                        peak[name] = (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20
                    emit("  whole model _inference (CONV_PRECISION = %s in both arms):" % prec)
                    for name, label in (("a", "(a) fp32 trunk tensors"), ("b", "(b) ACT_PRECISION = " + prec)):
                        emit("    %-28s median %8.3f  min %8.3f  max %8.3f  spread %6.3f   peak memory above the resident "
                             "model and inputs %8.1f MiB" % ((label,) + _row(tm[name]) + (peak[name],)))
                    if hasattr(cfg.MODEL, "ACT_PRECISION"):
                        del cfg.MODEL.ACT_PRECISION
            Cv.set_conv_precision("fp32")
            del model, fpn, stages, x
            torch.cuda.empty_cache()
    emit()
    emit("requirement ((b) not slower than (a) by more than 1.5 %% on the trunk at every shape and type): %s" %
         ("met" if all(verdicts) else "NOT met"))


if __name__ == "__main__":
    main()
