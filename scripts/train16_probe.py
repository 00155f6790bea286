"""What training the ResNet-101 trunk on 16-bit channels-last tensors (TRAIN.ACT_PRECISION, feature_intertwiner_amd/
train16.py, libfi_train16.so) takes against the existing 16-bit training path (MODEL.CONV_PRECISION: 16-bit MFMA operands,
fp32 NCHW tensors), at 2 x 1344^2 and 4 x 1024^2 (pooled maps 336^2 and 256^2), bf16 and fp16.

In ONE process on one MI355X, the arms taking turns inside every round, each timed with a HIP event pair, medians:
  layers  per distinct C2..C5 layer, through the C entry points on outputs allocated once, each launch 10 times back to back
          inside its event pair (the window / 10), 5 warm-up and 20 timed rounds:
            gated   fi_train16_conv_dgrad_gated (dx masked by the layer's input, with the column sums)
            dgrad   fi_grad16_conv_dgrad, and relu   fi_grad16_relu_grad on the dx-shaped tensor with its column sums:
                    the two launches the gated one replaces
  trunk   forward + backward of C2..C5 (sub_module.ResNet('resnet101', stage5=True), eval-mode BatchNorm, the stages
          chained, a gradient into c5), conv.prepare_step before every forward as in a training step, 3 warm-up and 7 timed
          rounds:
            old      the fp32-tensor path under CONV_PRECISION of the same type (the parent's behaviour: the baseline)
            ungated  16-bit tensors with conv.GATES = False: every layer runs relu_grad16 + dgrad16
            gated    16-bit tensors with the gates on
          and the peak of torch's allocator over one more, untimed, round of each arm.

    python scripts/train16_probe.py [--out profiles/train16_probe.txt] [--types bf16,fp16] [--sizes 1344,1024] [--no-layers]
Run it under a time limit (timeout -k 10 900 python scripts/train16_probe.py): a hung GPU step must end the command.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from grad16_probe import SHAPES, _events, _ms, layer_shapes      # noqa: E402  (the same layer table and timers)

WARMUP, ROUNDS, REPS = 5, 20, 10
T_WARMUP, T_ROUNDS = 3, 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train16_probe.txt"))
    ap.add_argument("--types", default="bf16,fp16")
    ap.add_argument("--sizes", default="1344,1024")
    ap.add_argument("--no-layers", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    from feature_intertwiner_amd import _lib, act16, grad16, train16
    from feature_intertwiner_amd import conv as Cv
    from feature_intertwiner_amd.sub_module import ResNet
    dev = "cuda:0"
    lines = []

    def emit(line=""):
        lines.append(line)
        print(line, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:          # kept current: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")

    emit("train16_probe: the ResNet-101 trunk on 16-bit channels-last tensors (TRAIN.ACT_PRECISION) vs the fp32-tensor path "
         "under CONV_PRECISION, %s" % torch.cuda.get_device_name(0))
    emit("arms alternating in one process, HIP event pairs, medians, ms")
    LG, LT = grad16.load(), train16.load()
    p = _lib.ptr
    for prec in args.types.split(","):
        dtype = act16.dtype_of(prec)
        Cv.set_conv_precision(prec)
        fn_relu, fn_dgrad = (Cv._lowp_fn(LG, "grad16_" + stem, prec) for stem in ("relu_grad", "conv_dgrad"))
        fn_gated = Cv._lowp_fn(LT, "train16_conv_dgrad_gated", prec)
        for size in [int(s) for s in args.sizes.split(",")]:
            n = SHAPES[size]
            emit()
            emit("== %s, %d x %d^2 (pooled map %d^2)" % (prec, n, size, size // 4))
            # ---- the trunk ------------------------------------------------------------------------------------------
            torch.manual_seed(2000)
            net = ResNet("resnet101", stage5=True).to(dev).eval()
            stages = torch.nn.Sequential(net.C2, net.C3, net.C4, net.C5)
            hw = size // 4
            x32 = torch.relu(torch.randn(n, 64, hw, hw, device=dev)).requires_grad_()
            x16 = act16.pack(x32.detach(), dtype).requires_grad_()
            with torch.no_grad():
                out_shape = stages(x16.detach()).shape
            dy32 = torch.randn(out_shape, device=dev)
            dy16 = act16.pack(dy32, dtype)
            params = [q for q in stages.parameters()]

            def arm(name):
                Cv.GATES = name != "ungated"
                Cv.prepare_step(stages)
                x, dy = (x32, dy32) if name == "old" else (x16, dy16)
                y = stages(x)
                torch.autograd.grad(y, [x] + params, dy)

            arms = ("old", "ungated", "gated")
            t = {a: [] for a in arms}
            try:
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
                train16.reset_stats()
                grad16.reset_stats()
                arm("gated")
                st, sg = train16.stats(), grad16.stats()
            finally:
                Cv.GATES = True
            m = {a: statistics.median(v) for a, v in t.items()}
            emit("  trunk forward + backward: old %.2f ms | ungated %.2f ms | gated %.2f ms | old / gated %.2f | "
                 "ungated / gated %.3f%s" % (m["old"], m["ungated"], m["gated"], m["old"] / m["gated"],
                                             m["ungated"] / m["gated"],
                                             "" if m["gated"] <= m["ungated"] else "   <- the gated form loses"))
            emit("  min .. max of the timed rounds: " + " | ".join("%s %.2f .. %.2f" % (a, min(t[a]), max(t[a])) for a in arms))
            emit("  peak memory of the trunk step above what was held before it (MiB): " +
                 " | ".join("%s %.0f" % (a, peak[a]) for a in arms))
            emit("  one gated backward: %d gated, %d premasked, %d fallback; grad16: %d relu_grad, %d dgrad, %d wgrad" % (
                st["gated"], st["premasked"], st["fallback"], sg["relu_grad"], sg["dgrad"], sg["wgrad"]))
            del net, stages, x32, x16, dy32, dy16, params
            torch.cuda.empty_cache()
            if args.no_layers:
                continue
            # ---- the layer classes ----------------------------------------------------------------------------------
            emit("   N   H   W  Cin Cout k s  xN | gated ms GB/s | dgrad ms | relu ms | dgrad + relu | two / gated")
            tot = {"gated": 0.0, "two": 0.0}
            for (N, H, W, Cin, Cout, k, s), count in layer_shapes(n, size // 4):
                torch.manual_seed(2000)
                pad = (k - 1) // 2
                OH = (H - 1) // s + 1
                gate = act16.pack(torch.relu(torch.randn(N, Cin, H, W, device=dev)), dtype)
                g = act16.pack(torch.randn(N, Cout, OH, OH, device=dev), dtype)
                wt = (torch.randn(Cin, k, k, Cout, device=dev) / (Cout * k * k) ** 0.5).to(dtype)
                dx, dxm = torch.empty_like(gate), torch.empty_like(gate)
                colsum = torch.empty(Cin, device=dev, dtype=torch.float32)
                geom = (N, H, W, Cin, Cout, k, k, s, pad)
                stream = _lib.current_stream()
                k_gated = lambda: fn_gated(p(g), p(wt), None, p(gate), p(dxm), p(colsum), *geom, stream)
                k_dgrad = lambda: fn_dgrad(p(g), p(wt), None, p(dx), *geom, stream)
                k_relu = lambda: fn_relu(p(dx), p(gate), p(dxm), p(colsum), N, H, W, Cin, 1, stream)
                tk = {"gated": [], "dgrad": [], "relu": []}
                for rnd in range(WARMUP + ROUNDS):
                    ev = _events(4)
                    for i, kern in enumerate((k_gated, k_dgrad, k_relu)):
                        ev[i].record()
                        for _ in range(REPS):
                            assert kern() == 0
                    ev[3].record()
                    if rnd >= WARMUP:
                        for name, a in (("gated", 0), ("dgrad", 1), ("relu", 2)):
                            tk[name].append(_ms(ev[a], ev[a + 1]) / REPS)
                mk = {name: statistics.median(v) for name, v in tk.items()}
                two = mk["dgrad"] + mk["relu"]
                b_gated = 2.0 * (N * OH * OH * Cout + 2 * N * H * W * Cin + Cout * Cin * k * k)
                tot["gated"] += count * mk["gated"]
                tot["two"] += count * two
                emit("  %2d %3d %3d %4d %4d %d %d x%2d | %6.3f %5.0f | %6.3f | %6.3f | %6.3f | %5.2f%s" % (
                    N, H, W, Cin, Cout, k, s, count, mk["gated"], b_gated / mk["gated"] / 1e6, mk["dgrad"], mk["relu"], two,
                    two / mk["gated"], "" if mk["gated"] <= two else "   <- loses"))
                del gate, g, wt, dx, dxm, colsum
            emit("  sum over the trunk's layers (count x median): gated %.3f ms, dgrad + relu_grad %.3f ms" % (
                tot["gated"], tot["two"]))
        Cv.set_conv_precision("fp32")


if __name__ == "__main__":
    main()
