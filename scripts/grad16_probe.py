"""What the backward of a convolution layer on 16-bit channels-last tensors (libfi_grad16.so, feature_intertwiner_amd/
grad16.py) takes against the existing 16-bit training path (MODEL.CONV_PRECISION: 16-bit MFMA operands, fp32 NCHW tensors),
for every distinct C2..C5 layer of ResNet-101 at 2 x 1344^2 and 4 x 1024^2 (pooled maps 336^2 and 256^2), bf16 and fp16.

In ONE process on one MI355X, the arms taking turns inside every round, each timed with a HIP event pair, 5 warm-up and 20
timed rounds, medians:
  new 3   the three launches on their own through the C entry points, outputs allocated once: fi_grad16_relu_grad (g and
          the column sums), fi_grad16_conv_wgrad (with its zero fill), fi_grad16_conv_dgrad -- each 10 times back to back
          inside its event pair (the window / 10), and their sum: kernel time, no host glue
  new L   the backward of grad16.conv_bn_act16 through autograd: the three launches + fi_bn_fold_grad + the host glue
  old L   the backward of conv.conv_bn_act under CONV_PRECISION of the same type on fp32 NCHW tensors, after prepare_step
          (W^T and 16-bit weight copies made, gradient arena armed) as in a training step: ReLU mask, weight gradient,
          fi_bn_fold_grad, data gradient
Only the backward is inside the event pair; both layers' forwards run untimed before it in every round.
Per kernel the bytes it must move (operands once, in their types) and its multiply-adds give GB/s and TFLOP/s.

    python scripts/grad16_probe.py [--out profiles/grad16_probe.txt] [--types bf16,fp16] [--sizes 1344,1024]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, ROUNDS = 5, 20
REPS = 10                                 # launches of one kernel inside its event pair
SHAPES = {1344: 2, 1024: 4}               # image size -> images
# ResNet-101: (planes, blocks, stride of the stage's first block); a block is 1x1 (stride) -> 3x3 -> 1x1 x4, the first of a
# stage with a 1x1 (stride) projection (sub_module.Bottleneck)
STAGES = ((64, 3, 1), (128, 4, 2), (256, 23, 2), (512, 3, 2))


def layer_shapes(n, hw):
    """[((N, H, W, Cin, Cout, k, stride), count)] of the trunk's convolutions on a pooled map of hw x hw, in order of use."""
    seen, order = {}, []
    h, cin = hw, 64
    for planes, blocks, stride in STAGES:
        for b in range(blocks):
            s = stride if b == 0 else 1
            ho = (h - 1) // s + 1
            rows = [(n, h, h, cin, planes, 1, s), (n, ho, ho, planes, planes, 3, 1), (n, ho, ho, planes, 4 * planes, 1, 1)]
            if b == 0:
                rows.append((n, h, h, cin, 4 * planes, 1, s))
            for r in rows:
                if r not in seen:
                    seen[r] = 0
                    order.append(r)
                seen[r] += 1
            h, cin = ho, 4 * planes
    return [(r, seen[r]) for r in order]


def _ms(e0, e1):
    e1.synchronize()
    return e0.elapsed_time(e1)


def _events(n):
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad16_probe.txt"))
    ap.add_argument("--types", default="bf16,fp16")
    ap.add_argument("--sizes", default="1344,1024")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    from feature_intertwiner_amd import _lib, act16, grad16
    from feature_intertwiner_amd import conv as Cv
    from feature_intertwiner_amd.sub_module import _bn
    dev = "cuda:0"
    lines = []

    def emit(line=""):
        lines.append(line)
        print(line, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:          # kept current: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")

    emit("grad16_probe: backward of the ResNet-101 trunk's layers on 16-bit channels-last tensors (libfi_grad16.so) vs the "
         "backward of conv.conv_bn_act under CONV_PRECISION on fp32 NCHW tensors, %s" % torch.cuda.get_device_name(0))
    emit("%d timed rounds after %d warm-up rounds, arms alternating in one process, HIP events around the backward only; "
         "medians, ms" % (ROUNDS, WARMUP))
    L = grad16.load()
    warmed = False
    for prec in args.types.split(","):
        dtype = act16.dtype_of(prec)
        Cv.set_conv_precision(prec)
        fn_relu, fn_wgrad, fn_dgrad = (Cv._lowp_fn(L, "grad16_" + stem, prec) for stem in ("relu_grad", "conv_wgrad", "conv_dgrad"))
        for size in [int(s) for s in args.sizes.split(",")]:
            n = SHAPES[size]
            emit()
            emit("== %s, %d x %d^2 (pooled map %d^2)" % (prec, n, size, size // 4))
            emit("   N   H   W  Cin Cout k s  xN | relu_grad ms GB/s | wgrad ms GB/s TF/s | dgrad ms GB/s TF/s | new 3 | new L | "
                 "old L | old L / new L")
            tot = {"new3": 0.0, "newL": 0.0, "oldL": 0.0}
            for (N, H, W, Cin, Cout, k, s), count in layer_shapes(n, size // 4):
                torch.manual_seed(2000)
                pad = (k - 1) // 2
                conv = Cv.Conv2d(Cin, Cout, kernel_size=k, stride=s, padding=pad).to(dev)
                bn = _bn(Cout).to(dev).eval()
                layer = torch.nn.Sequential(conv, bn)
                x32 = torch.relu(torch.randn(N, Cin, H, W, device=dev)).requires_grad_()
                x16 = act16.pack(x32.detach(), dtype).requires_grad_()
                OH = (H - 1) // s + 1
                dy32 = torch.randn(N, Cout, OH, OH, device=dev)
                dy16 = act16.pack(dy32, dtype)
                params = [conv.weight, conv.bias, bn.weight, bn.bias]
                Cv.prepare_step(layer)
                with torch.no_grad():
                    y16 = act16.conv_bn_act16(x16.detach(), conv, bn, relu=True)
                    wt = grad16.weight_t16(conv, bn, bn._fi_fold[0], dtype)
                # the three launches through the C entry points on outputs allocated once, REPS back to back inside an
                # event pair: the host's enqueue stays ahead of the GPU and the window is not one launch long
                g = torch.empty_like(y16)
                colsum = torch.empty(Cout, device=dev, dtype=torch.float32)
                dw = torch.empty((Cout, k, k, Cin), device=dev, dtype=torch.float32)
                dx = torch.empty_like(x16.detach())
                geom = (N, H, W, Cin, Cout, k, k, s, pad)
                st = _lib.current_stream()
                p = _lib.ptr
                k_relu = lambda: fn_relu(p(dy16), p(y16), p(g), p(colsum), N, OH, OH, Cout, 1, st)
                k_wgrad = lambda: fn_wgrad(p(g), p(x16), p(dw), *geom, st)
                k_dgrad = lambda: fn_dgrad(p(g), p(wt), None, p(dx), *geom, st)
                t = {"relu": [], "wgrad": [], "dgrad": [], "newL": [], "oldL": []}
                warm = WARMUP + (40 if not warmed else 0)      # the process's first layer: a longer warm-up
                warmed = True
                for rnd in range(warm + ROUNDS):
                    ev = _events(8)
                    for i, kern in enumerate((k_relu, k_wgrad, k_dgrad)):
                        ev[i].record()
                        for _ in range(REPS):
                            assert kern() == 0
                    ev[3].record()
                    Cv.prepare_step(layer)
                    y = grad16.conv_bn_act16(x16, conv, bn, relu=True)
                    ev[4].record()
                    torch.autograd.grad(y, [x16] + params, dy16)
                    ev[5].record()
                    Cv.prepare_step(layer)
                    y = Cv.conv_bn_act(x32, conv, bn, relu=True)
                    ev[6].record()
                    torch.autograd.grad(y, [x32] + params, dy32)
                    ev[7].record()
                    del y
                    if rnd >= warm:
                        for name, a, b, reps in (("relu", 0, 1, REPS), ("wgrad", 1, 2, REPS), ("dgrad", 2, 3, REPS),
                                                 ("newL", 4, 5, 1), ("oldL", 6, 7, 1)):
                            t[name].append(_ms(ev[a], ev[b]) / reps)
                m = {name: statistics.median(v) for name, v in t.items()}
                P, Pin = N * OH * OH, N * H * W
                b_relu = 2.0 * 3 * P * Cout + 4.0 * Cout
                b_wg = 2.0 * (P * Cout + Pin * Cin) + 4.0 * Cout * Cin * k * k
                b_dg = 2.0 * (P * Cout + Pin * Cin + Cout * Cin * k * k)
                flops = 2.0 * P * Cout * Cin * k * k
                new3 = m["relu"] + m["wgrad"] + m["dgrad"]
                tot["new3"] += count * new3
                tot["newL"] += count * m["newL"]
                tot["oldL"] += count * m["oldL"]
                emit("  %2d %3d %3d %4d %4d %d %d x%2d | %6.3f %5.0f | %6.3f %5.0f %6.1f | %6.3f %5.0f %6.1f | %6.3f | %6.3f | %6.3f | "
                     "%5.2f%s" % (N, H, W, Cin, Cout, k, s, count, m["relu"], b_relu / m["relu"] / 1e6, m["wgrad"],
                                  b_wg / m["wgrad"] / 1e6, flops / m["wgrad"] / 1e9, m["dgrad"], b_dg / m["dgrad"] / 1e6,
                                  flops / m["dgrad"] / 1e9, new3, m["newL"], m["oldL"], m["oldL"] / m["newL"],
                                  "" if m["newL"] <= m["oldL"] else "   <- loses"))
                del x32, x16, dy32, dy16, y16, wt, conv, bn, layer, g, colsum, dw, dx
                torch.cuda.empty_cache()
            emit("  sum over the trunk's layers (count x median): new 3 %.3f ms, new L %.3f ms, old L %.3f ms" % (
                tot["new3"], tot["newL"], tot["oldL"]))
        Cv.set_conv_precision("fp32")


if __name__ == "__main__":
    main()
