"""What the 2x make-up layer (ConvTranspose2d 256 -> 256, 3x3, stride 2, padding 1, output_padding 1, + eval BatchNorm +
ReLU, channels-last for RoIAlign) costs on its shapes at the headline image size: N = 4, H = W in {256, 128, 64, 32}.

In ONE process, interleaved round by round, each call timed with a HIP event pair, median / min / max over the rounds:
  (a) stock        nn.ConvTranspose2d + eval nn.BatchNorm2d + ReLU (the vendor convolution library), then the
                   .contiguous(memory_format=channels_last) RoIAlign wants -- what ran before conv.ConvTranspose3x3
  (b) composition  the four-class composition of existing library kernels (four stride-1 convolutions with the folded
                   BatchNorm and ReLU in their epilogues + fi_stride2_interleave) and the channels-last copy
  (c) fused        fi_conv_transpose3x3s2_forward: one launch, channels-last written by the kernel
TFLOP/s on the 2.25-taps-per-output-pixel count (2 * 9 * Cin * Cout * N * H * W flops); bytes: x + w + y once.
"spread" of a path is max - min over its rounds; (c) beats (b) when median(b) - median(c) exceeds the larger spread.

    python scripts/convt_probe.py [--rounds 20] [--out profiles/convt_probe.txt]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, C = 4, 256
SIZES = (256, 128, 64, 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convt_probe.txt"))
    args = ap.parse_args()
    from feature_intertwiner_amd import conv as Cv
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    assert args.rounds >= 20, "at least 20 timed launches per path"
    Cv.load_convt()
    dev = "cuda:0"
    torch.manual_seed(2000)
    ours = Cv.ConvTranspose3x3(C, C, kernel_size=3, stride=2, padding=1, output_padding=1)
    bn = nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_()
        bn.running_mean.normal_()
        bn.running_var.uniform_(0.5, 2.0)
    stock = nn.ConvTranspose2d(C, C, kernel_size=3, stride=2, padding=1, output_padding=1)
    stock.load_state_dict(ours.state_dict())
    ours, bn, stock = ours.to(dev), bn.to(dev).eval(), stock.to(dev)

    def path_a(x):
        return torch.relu(bn(stock(x))).contiguous(memory_format=torch.channels_last)

    def path_b(x):
        Cv.CONVT_COMPOSE_ONLY = True
        try:
            return Cv.convt_bn_act(x, ours, bn, relu=True, channels_last_out=True)
        finally:
            Cv.CONVT_COMPOSE_ONLY = False

    def path_c(x):
        return Cv.convt_bn_act(x, ours, bn, relu=True, channels_last_out=True)

    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    paths = (("a stock", path_a), ("b composition", path_b), ("c fused", path_c))
    emit("convt_probe: ConvTranspose2d(%d, %d, 3, stride 2, padding 1, output_padding 1) + eval BN + ReLU -> channels-last, "
         "N = %d, fp32, %s" % (C, C, N, torch.cuda.get_device_name(0)))
    emit("%d timed rounds per path (after %d warm-up rounds), the three paths interleaved in one process, HIP events; ms" %
         (args.rounds, args.warmup))
    verdicts = []
    with torch.no_grad():
        for hw in SIZES:
            x = torch.randn(N, C, hw, hw, device=dev)
            flops = 2.0 * 9 * C * C * N * hw * hw
            nbytes = 4.0 * (N * C * hw * hw + 9 * C * C + N * C * 4 * hw * hw)
            outs = {}
            for _ in range(args.warmup):
                for name, fn in paths:
                    outs[name] = fn(x)
            torch.cuda.synchronize()
            ref = outs["a stock"]
            scale = ref.abs().max().item()
            agree = {name: (outs[name] - ref).abs().max().item() / scale for name in ("b composition", "c fused")}
            del outs, ref
            times = {name: [] for name, _ in paths}
            for _ in range(args.rounds):
                for name, fn in paths:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    y = fn(x)
                    e1.record()
                    e1.synchronize()
                    times[name].append(e0.elapsed_time(e1))
                    del y
            emit("")
            emit("H = W = %d: %.2f GFLOP (2.25 taps per output pixel), %.1f MB moved once (x + w + y)" %
                 (hw, flops / 1e9, nbytes / 1e6))
            med = {}
            spread = {}
            for name, _ in paths:
                t = times[name]
                med[name], spread[name] = statistics.median(t), max(t) - min(t)
                emit("  (%-13s) median %8.3f  min %8.3f  max %8.3f  spread %7.3f   %6.1f TFLOP/s  %7.1f GB/s" %
                     (name, med[name], min(t), max(t), spread[name], flops / med[name] / 1e9, nbytes / med[name] / 1e6))
            gain = med["b composition"] - med["c fused"]
            noise = max(spread["b composition"], spread["c fused"])
            ok = gain > noise
            verdicts.append(ok)
            emit("  (c) vs (b): %.2fx, %.3f ms saved, larger spread %.3f ms -> %s" %
                 (med["b composition"] / med["c fused"], gain, noise,
                  "faster by more than the spread" if ok else "NOT faster by more than the spread"))
            emit("  (c) vs (a): %.2fx   (b) vs (a): %.2fx" % (med["a stock"] / med["c fused"],
                                                              med["a stock"] / med["b composition"]))
            emit("  max|y - y_stock| / max|y_stock|: composition %.2e, fused %.2e" %
                 (agree["b composition"], agree["c fused"]))
            del x
    emit("")
    emit("condition ((c) faster than (b) by more than the spread on every shape): %s" %
         ("met" if all(verdicts) else "NOT met"))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
