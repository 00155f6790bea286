"""What the feature pyramid of a train step takes on 16-bit channels-last tensors (TRAIN.ACT_SCOPE = 'pyramid',
feature_intertwiner_amd/fpn16.py, libfi_fpn16.so) against TRAIN.ACT_SCOPE = 'trunk' (c2..c5 unpacked, the pyramid on fp32
NCHW tensors: the parent's behaviour), ResNet-101's c2..c5 at 2 x 1344^2 and 4 x 1024^2 (c2 336^2 and 256^2), bf16 and fp16.

In ONE process on one MI355X, the arms taking turns inside every round, each timed with a HIP event pair, medians:
  (a) launches  per level, through the C entry point on outputs allocated once, each launch 10 times back to back inside
                its event pair (the window / 10), 5 warm-up and 20 timed rounds:
                  new   fi_fpn16_topdown_grad (own + the 2 x 2 sums of fine, one rounding, the column sums), with its share
                        of the HBM peak (8 TB/s) from the bytes the shapes imply: 6 tensors of the coarse map's size
                  old   the composition it replaces: torch's 2 x 2 sum pool of the widened fine map, the add, one rounding
                        (.to(dtype)), and relu_grad16(relu=False) for the sums
                and for the smoothing layers' bias sums on p2..p5:
                  sums  the read-only column-sum call, against relu_grad16(relu=False), which also writes a copy
  (b) segment   forward + backward from 16-bit c2..c5 (leaves that require grad) to fp32 p2..p6, a gradient into each,
                conv.prepare_step before every forward as in a training step, MODEL.CONV_PRECISION of the type in both
                arms, 3 warm-up and 7 timed rounds:
                  trunk    train16.unpack of c2..c5, then the lines of FPN.forward: P5_conv1, the three laterals with the
                           upsampled top as their residual, the four smoothing convolutions, P6 -- the baseline
                  pyramid  FPN._pyramid_train16
                and the peak of torch's allocator over one more, untimed, round of each arm.

    python scripts/fpn16_probe.py [--out profiles/fpn16_probe.txt] [--types bf16,fp16] [--sizes 1344,1024]
Run it under a time limit (timeout -k 10 600 python scripts/fpn16_probe.py): a hung GPU step must end the command.
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from grad16_probe import SHAPES, _events, _ms      # noqa: E402  (the same batch sizes and timers)

WARMUP, ROUNDS, REPS = 5, 20, 10
T_WARMUP, T_ROUNDS = 3, 7
HBM_PEAK = 8.0e12
CIN = {2: 256, 3: 512, 4: 1024, 5: 2048}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fpn16_probe.txt"))
    ap.add_argument("--types", default="bf16,fp16")
    ap.add_argument("--sizes", default="1344,1024")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    from feature_intertwiner_amd import _lib, act16, fpn16, grad16, train16
    from feature_intertwiner_amd import conv as Cv
    from feature_intertwiner_amd.config import make_config
    from feature_intertwiner_amd.sub_module import FPN
    dev = "cuda:0"
    lines = []

    def emit(line=""):
        lines.append(line)
        print(line, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:          # kept current: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")

    emit("fpn16_probe: the feature pyramid of a train step on 16-bit channels-last tensors (TRAIN.ACT_SCOPE = 'pyramid') vs "
         "the fp32-tensor pyramid behind unpacked c2..c5 ('trunk'), %s" % torch.cuda.get_device_name(0))
    emit("arms alternating in one process, HIP event pairs, medians, ms")
    LF = fpn16.load()
    p = _lib.ptr
    cl = torch.channels_last
    for prec in args.types.split(","):
        dtype = act16.dtype_of(prec)
        Cv.set_conv_precision(prec)
        fn_top = Cv._lowp_fn(LF, "fpn16_topdown_grad", prec)
        for size in [int(s) for s in args.sizes.split(",")]:
            n = SHAPES[size]
            hw = {lvl: size // (1 << lvl) for lvl in (2, 3, 4, 5)}
            emit()
            emit("== %s, %d x %d^2 (c2 %d^2 .. c5 %d^2)" % (prec, n, size, hw[2], hw[5]))
            # ---- (a) the launches -----------------------------------------------------------------------------------
            emit("  (a) coarse level, N H W C | new ms, GB/s, share of 8 TB/s | old ms (pool + add + round | relu_grad) | "
                 "old / new")
            for lvl in (3, 4, 5):
                torch.manual_seed(2000)
                H = hw[lvl]
                own = torch.randn(n, 256, H, H, device=dev).to(dtype).contiguous(memory_format=cl)
                fine = torch.randn(n, 256, 2 * H, 2 * H, device=dev).to(dtype).contiguous(memory_format=cl)
                g = torch.empty_like(own)
                colsum = torch.empty(256, device=dev, dtype=torch.float32)
                stream = _lib.current_stream()
                k_new = lambda: fn_top(p(own), p(fine), p(g), p(colsum), n, H, H, 256, stream)

                def k_pool():
                    return (own.float() + F.avg_pool2d(fine.float(), 2, divisor_override=1)).to(dtype)

                def k_relu(t=g):
                    grad16.relu_grad16(t, None, relu=False, colsum=True)

                tk = {"new": [], "pool": [], "relu": []}
                for rnd in range(WARMUP + ROUNDS):
                    ev = _events(4)
                    ev[0].record()
                    for _ in range(REPS):
                        assert k_new() == 0
                    ev[1].record()
                    for _ in range(REPS):
                        k_pool()
                    ev[2].record()
                    for _ in range(REPS):
                        k_relu()
                    ev[3].record()
                    if rnd >= WARMUP:
                        for i, name in enumerate(("new", "pool", "relu")):
                            tk[name].append(_ms(ev[i], ev[i + 1]) / REPS)
                m = {name: statistics.median(v) for name, v in tk.items()}
                nbytes = 2.0 * 6 * n * H * H * 256 + 4.0 * 256
                old = m["pool"] + m["relu"]
                emit("      p%d  %d %3d %3d 256 | %6.3f %5.0f %4.1f %% | %6.3f (%6.3f | %6.3f) | %5.2f%s" % (
                    lvl, n, H, H, m["new"], nbytes / m["new"] / 1e6, 100.0 * nbytes / (m["new"] * 1e-3) / HBM_PEAK, old,
                    m["pool"], m["relu"], old / m["new"], "" if m["new"] <= old else "   <- loses"))
                del own, fine, g, colsum
            emit("  (a) bias sums of a smoothing layer, N H W C | read-only sums ms, GB/s, share | relu_grad16(relu=False) ms "
                 "| old / new")
            for lvl in (2, 3, 4, 5):
                torch.manual_seed(2000)
                H = hw[lvl]
                dy = torch.randn(n, 256, H, H, device=dev).to(dtype).contiguous(memory_format=cl)
                colsum = torch.empty(256, device=dev, dtype=torch.float32)
                stream = _lib.current_stream()
                k_new = lambda: fn_top(p(dy), None, p(dy), p(colsum), n, H, H, 256, stream)
                tk = {"new": [], "relu": []}
                for rnd in range(WARMUP + ROUNDS):
                    ev = _events(3)
                    ev[0].record()
                    for _ in range(REPS):
                        assert k_new() == 0
                    ev[1].record()
                    for _ in range(REPS):
                        grad16.relu_grad16(dy, None, relu=False, colsum=True)
                    ev[2].record()
                    if rnd >= WARMUP:
                        tk["new"].append(_ms(ev[0], ev[1]) / REPS)
                        tk["relu"].append(_ms(ev[1], ev[2]) / REPS)
                m = {name: statistics.median(v) for name, v in tk.items()}
                nbytes = 2.0 * n * H * H * 256 + 4.0 * 256
                emit("      p%d  %d %3d %3d 256 | %6.3f %5.0f %4.1f %% | %6.3f | %5.2f%s" % (
                    lvl, n, H, H, m["new"], nbytes / m["new"] / 1e6, 100.0 * nbytes / (m["new"] * 1e-3) / HBM_PEAK, m["relu"],
                    m["relu"] / m["new"], "" if m["new"] <= m["relu"] else "   <- loses"))
                del dy, colsum
            # ---- (b) the segment ------------------------------------------------------------------------------------
            torch.manual_seed(2000)
            cfg = make_config(backbone="resnet101", image_size=size, batch_size=n, train_rois_per_image=48,
                              conv_precision=prec)
            cfg.TRAIN.ACT_PRECISION, cfg.TRAIN.ACT_SCOPE = prec, "pyramid"
            fpn = FPN(cfg, *[torch.nn.Identity() for _ in range(5)], out_channels=256).to(dev).eval()
            c = {lvl: torch.relu(torch.randn(n, CIN[lvl], hw[lvl], hw[lvl], device=dev)).to(dtype)
                 .contiguous(memory_format=cl).requires_grad_() for lvl in (2, 3, 4, 5)}
            leaves = [c[lvl] for lvl in (2, 3, 4, 5)]
            params = [q for q in fpn.parameters()]
            dys = [torch.randn(n, 256, h, h, device=dev) for h in (hw[2], hw[3], hw[4], hw[5], (hw[5] + 1) // 2)]

            def pyramid_fp32():
                """The lines of FPN.forward behind train16.unpack under TRAIN.ACT_SCOPE = 'trunk'."""
                u = {lvl: train16.unpack(m) for lvl, m in c.items()}
                lat = lambda m, x, top: Cv.conv2d(x, m.weight, m.bias, m.stride, m.padding, residual=Cv.upsample2x(top))
                p5 = fpn.P5_conv1(u[5])
                p4 = lat(fpn.P4_conv1, u[4], p5)
                p3 = lat(fpn.P3_conv1, u[3], p4)
                p2 = lat(fpn.P2_conv1, u[2], p3)
                p5, p4, p3, p2 = fpn.P5_conv2(p5), fpn.P4_conv2(p4), fpn.P3_conv2(p3), fpn.P2_conv2(p2)
                return [p2, p3, p4, p5, fpn.P6(p5)]

            def arm(name):
                Cv.prepare_step(fpn)
                outs = pyramid_fp32() if name == "trunk" else fpn._pyramid_train16(c, {})
                torch.autograd.grad(outs, leaves + params, dys)

            arms = ("trunk", "pyramid")
            t = {a: [] for a in arms}
            for rnd in range(T_WARMUP + T_ROUNDS):
                for a in arms:
                    e0, e1 = _events(2)
                    e0.record()
                    arm(a)
                    e1.record()
                    if rnd >= T_WARMUP:
                        t[a].append(_ms(e0, e1))
            peak = {}
            for a in arms:
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                arm(a)
                torch.cuda.synchronize()
                peak[a] = (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20
            fpn16.reset_stats()
            grad16.reset_stats()
            arm("pyramid")
            sf, sg = fpn16.stats(), grad16.stats()
            m = {a: statistics.median(v) for a, v in t.items()}
            emit("  (b) c2..c5 -> p2..p6 forward + backward: trunk %.2f ms | pyramid %.2f ms | trunk / pyramid %.2f%s" % (
                m["trunk"], m["pyramid"], m["trunk"] / m["pyramid"],
                "" if m["pyramid"] <= m["trunk"] else "   <- 'pyramid' loses"))
            emit("      min .. max of the timed rounds: " + " | ".join("%s %.2f .. %.2f" % (a, min(t[a]), max(t[a])) for a in arms))
            emit("      peak memory of the segment above what was held before it (MiB): " +
                 " | ".join("%s %.0f" % (a, peak[a]) for a in arms))
            emit("      one 'pyramid' round: fpn16 %d topdown, %d sums, %d to autograd; grad16: %d relu_grad, %d dgrad, %d wgrad"
                 % (sf["topdown"], sf["sums"], sf["top_to_autograd"], sg["relu_grad"], sg["dgrad"], sg["wgrad"]))
            del fpn, c, leaves, params, dys
            torch.cuda.empty_cache()
        Cv.set_conv_precision("fp32")


if __name__ == "__main__":
    main()
