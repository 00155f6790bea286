"""What the readers of p2..p5 take on 16-bit channels-last pyramid maps in a train step (TRAIN.ACT_SCOPE = 'crops',
feature_intertwiner_amd/crops16.py, libfi_crops16.so) against TRAIN.ACT_SCOPE = 'pyramid' (the four smoothed maps unpacked,
the RPN, the make-up layer and RoIAlign on fp32 tensors: the parent's behaviour), ResNet-101's pyramid at 2 x 1344^2 with
1000 RoIs per image and 4 x 1024^2 with 512, bf16 and fp16.

In ONE process on one MI355X, the arms taking turns inside every round, each timed with a HIP event pair, medians:
  (a) launches  per level p2..p5, each launch 10 times back to back inside its event pair (the window / 10), 5 warm-up and
                20 timed rounds:
                  gate-pack   fi_crops16_gate_pack (mask, one rounding, column sums) on an fp32 channels-last gradient, with
                              its share of the HBM peak (8 TB/s) from the bytes the shapes imply (4 + 2 + 2 per element),
                              against act16.pack of the NCHW gradient + relu_grad16
                  make-up     the layer's forward + backward on one level: train16.conv_bn_act16 with the premasked backward
                              the crops leave it, against conv.conv_bn_act (channels-last output) on the fp32 map
                and once for all five levels, 256 sampled anchors per image:
                  patch rows  fi_crops16_patch_rows_forward / _backward against fi_pyramid_patch_rows_forward / _backward
                              (the backward of the fp32 arm adds into maps that exist; its zero fill is not timed)
  (b) segment   forward + backward from the smoothed 16-bit p2..p5 (leaves that require grad) to the RPN's row outputs and
                the 7 x 7 and 14 x 14 crops, a gradient into each, the dense RPN under no_grad in both arms,
                conv.prepare_step before every forward, MODEL.CONV_PRECISION of the type in both arms, 3 warm-up and 7
                timed rounds, and the peak of torch's allocator over one more, untimed, round of each arm.

    python scripts/crops16_probe.py [--out profiles/crops16_probe.txt] [--types bf16,fp16] [--sizes 1344,1024]
Run it under a time limit (timeout -k 10 600 python scripts/crops16_probe.py): a hung GPU step must end the command.
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from grad16_probe import SHAPES, _events, _ms      # noqa: E402  (the same batch sizes and timers)

WARMUP, ROUNDS, REPS = 5, 20, 10
T_WARMUP, T_ROUNDS = 3, 7
HBM_PEAK = 8.0e12
ROIS = {1344: 1000, 1024: 512}
PER_LOC = 3


def _timed(arms, warmup, rounds, reps=1):
    """{name: median ms per call}: the arms take turns inside every round."""
    t = {a: [] for a in arms}
    for rnd in range(warmup + rounds):
        for a, fn in arms.items():
            e0, e1 = _events(2)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            if rnd >= warmup:
                t[a].append(_ms(e0, e1) / reps)
    return {a: statistics.median(v) for a, v in t.items()}, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crops16_probe.txt"))
    ap.add_argument("--types", default="bf16,fp16")
    ap.add_argument("--sizes", default="1344,1024")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    from feature_intertwiner_amd import _lib, act16, crops16, grad16, train16
    from feature_intertwiner_amd import conv as Cv
    from feature_intertwiner_amd.config import make_config
    from feature_intertwiner_amd.intertwiner import roi_level
    from feature_intertwiner_amd.roi_align.crop_and_resize import CropGradGroup
    from feature_intertwiner_amd.sub_module import RPN, Dev
    dev = "cuda:0"
    lines = []

    def emit(line=""):
        lines.append(line)
        print(line, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:          # kept current: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")

    emit("crops16_probe: the readers of p2..p5 in a train step on 16-bit channels-last maps (TRAIN.ACT_SCOPE = 'crops') vs on "
         "the unpacked fp32 maps ('pyramid'), %s" % torch.cuda.get_device_name(0))
    emit("arms alternating in one process, HIP event pairs, medians, ms")
    LC, LH = crops16.load(), _lib.load()
    p = _lib.ptr
    cl = torch.channels_last
    for prec in args.types.split(","):
        dtype = act16.dtype_of(prec)
        Cv.set_conv_precision(prec)
        for size in [int(s) for s in args.sizes.split(",")]:
            n, R = SHAPES[size], ROIS[size]
            hw = [size // (1 << lvl) for lvl in (2, 3, 4, 5)]
            emit()
            emit("== %s, %d x %d^2 (p2 %d^2 .. p5 %d^2), %d RoIs per image" % (prec, n, size, hw[0], hw[3], R))
            torch.manual_seed(2000)
            cfg = make_config(backbone="resnet101", image_size=size, batch_size=n, train_rois_per_image=R,
                              conv_precision=prec)
            cfg.TRAIN.ACT_PRECISION, cfg.TRAIN.ACT_SCOPE = prec, "crops"
            rpn = RPN(PER_LOC, 1, 256).to(dev).eval()
            stage = Dev(cfg, 256).to(dev).eval()
            conv, bn = stage.upsample[0][0], stage.upsample[0][1]
            with torch.no_grad():
                bn.running_mean.normal_(0.0, 0.5)
                bn.running_var.uniform_(0.25, 1.25)
            Cv.prepare_step(stage)
            Cv.prepare_step(rpn)
            ps = [torch.randn(n, 256, h, h, device=dev).to(dtype).contiguous(memory_format=cl).requires_grad_() for h in hw]
            # ---- (a) the launches -----------------------------------------------------------------------------------
            emit("  (a) level, N H W C | gate-pack ms, GB/s, share of 8 TB/s | pack + relu_grad16 ms (pack | relu_grad) | "
                 "old / new || make-up fwd + bwd: 16-bit ms | fp32 tensors ms | old / new")
            for lvl, (h, m16) in enumerate(zip(hw, ps)):
                d_cl = torch.randn(n, 256, h, h, device=dev).contiguous(memory_format=cl)
                d_nchw = d_cl.contiguous()
                y = torch.randn(n, 256, h, h, device=dev).to(dtype).contiguous(memory_format=cl)
                g = torch.empty_like(y)
                sums = torch.empty(256, device=dev)
                fn = Cv._lowp_fn(LC, "crops16_gate_pack", prec)
                stream = _lib.current_stream()
                state = {}

                def k_new():
                    assert fn(p(d_cl), p(y), p(g), p(sums), n, h, h, 256, stream) == 0

                def k_pack():
                    state["g"] = act16.pack(d_nchw, dtype)

                def k_relu():
                    grad16.relu_grad16(state["g"], y)

                k_pack()
                m, _ = _timed({"new": k_new, "pack": k_pack, "relu": k_relu}, WARMUP, ROUNDS, REPS)
                nbytes = 8.0 * n * h * h * 256 + 4.0 * 256
                old = m["pack"] + m["relu"]
                # the make-up layer on this level
                x32 = act16.unpack(m16.detach()).requires_grad_()
                dy32 = torch.randn(n, 256, h, h, device=dev).contiguous(memory_format=cl)
                dy16 = dy32.to(dtype)
                s16 = torch.zeros(256, device=dev)
                wts = [conv.weight, conv.bias, bn.weight, bn.bias]

                def mk_new():
                    u = train16.conv_bn_act16(m16, conv, bn, relu=True)
                    gate = train16._claim_gate16(u, True)
                    gate.leave(dy16, s16)
                    torch.autograd.grad([u], [m16] + wts, [dy16])

                def mk_old():
                    u = Cv.conv_bn_act(x32, conv, bn, relu=True, channels_last_out=True)
                    torch.autograd.grad([u], [x32] + wts, [dy32])

                mm, _ = _timed({"new": mk_new, "old": mk_old}, T_WARMUP, T_ROUNDS)
                emit("      p%d  %d %3d %3d 256 | %6.3f %5.0f %4.1f %% | %6.3f (%6.3f | %6.3f) | %5.2f%s || %6.3f | %6.3f | %5.2f%s" % (
                    lvl + 2, n, h, h, m["new"], nbytes / m["new"] / 1e6, 100.0 * nbytes / (m["new"] * 1e-3) / HBM_PEAK, old,
                    m["pack"], m["relu"], old / m["new"], "" if m["new"] <= old else "   <- loses",
                    mm["new"], mm["old"], mm["old"] / mm["new"], "" if mm["new"] <= mm["old"] else "   <- loses"))
                del d_cl, d_nchw, y, g, x32, dy32, dy16, state
            # the patch rows: 256 sampled anchors per image over the five levels
            rows = 256 * n
            sizes5 = hw + [(hw[3] + 1) // 2]
            total = sum(h * h * PER_LOC for h in sizes5)
            image = torch.arange(n, device=dev).repeat_interleave(256)
            anchor = torch.randint(0, total, (rows,), device=dev)
            anchor[: rows // 4] = anchor[rows // 4: rows // 2]          # sampled anchors cluster: repeated pixels
            maps32 = [act16.unpack(m.detach()) for m in ps]
            maps32.append(maps32[3][:, :, ::2, ::2].contiguous())
            out = torch.empty(rows, 9 * 256, device=dev)
            d_rows = torch.randn(rows, 9 * 256, device=dev)
            g16 = [torch.zeros_like(m.detach()) for m in ps]
            g32 = [torch.zeros_like(m) for m in maps32]
            lv16 = [m.detach() for m in ps] + [ps[3].detach()]
            arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
            ints = lambda v: (ctypes.c_int * len(v))(*v)
            h16, st16 = ints([t.shape[2] for t in lv16]), ints([1, 1, 1, 1, 2])
            h32 = ints([t.shape[2] for t in maps32])
            f_new = Cv._lowp_fn(LC, "crops16_patch_rows_forward", prec)
            b_new = Cv._lowp_fn(LC, "crops16_patch_rows_backward", prec)
            a16, a32, ag16, ag32 = arr(lv16), arr(maps32), arr(g16 + [g16[3]]), arr(g32)
            stream = _lib.current_stream()
            arms = {
                "fwd16": lambda: f_new(a16, h16, h16, st16, 5, PER_LOC, p(image), p(anchor), rows, n, 256, p(out), stream),
                "fwd32": lambda: LH.fi_pyramid_patch_rows_forward(a32, h32, h32, 5, PER_LOC, p(image), p(anchor), rows, 256,
                                                                  p(out), stream),
                "bwd16": lambda: b_new(p(d_rows), ag16, h16, h16, st16, 5, PER_LOC, p(image), p(anchor), rows, n, 256, stream),
                "bwd32": lambda: LH.fi_pyramid_patch_rows_backward(p(d_rows), ag32, h32, h32, 5, PER_LOC, p(image), p(anchor),
                                                                   rows, 256, stream),
            }
            m, _ = _timed(arms, WARMUP, ROUNDS, REPS)
            emit("  (a) patch rows, %d rows: forward 16-bit %.4f | fp32 %.4f | old / new %.2f%s || backward 16-bit %.4f | fp32 "
                 "%.4f | old / new %.2f%s" % (rows, m["fwd16"], m["fwd32"], m["fwd32"] / m["fwd16"],
                                             "" if m["fwd16"] <= m["fwd32"] else "   <- loses", m["bwd16"], m["bwd32"],
                                             m["bwd32"] / m["bwd16"], "" if m["bwd16"] <= m["bwd32"] else "   <- loses"))
            del maps32, g32, g16, out, d_rows
            # ---- (b) the segment ------------------------------------------------------------------------------------
            torch.manual_seed(2001)
            ctr = torch.rand(n * R, 2, device=dev)
            ext = 0.02 + 0.5 * torch.rand(n * R, 2, device=dev) ** 2
            boxes = torch.cat(((ctr - ext / 2).clamp(0, 1), (ctr + ext / 2).clamp(0, 1)), 1)
            ind = torch.arange(n, device=dev, dtype=torch.int32).repeat_interleave(R)
            level = roi_level(boxes, float(size * size), cfg.ROIS.ASSIGN_ANCHOR_BASE)
            valid = torch.ones(rows, dtype=torch.bool, device=dev)
            params = list(rpn.parameters()) + [conv.weight, conv.bias, bn.weight, bn.bias]
            d_out = [torch.randn(rows, 2, device=dev), torch.randn(rows, 4, device=dev),
                     torch.randn(n * R, 256, 7, 7, device=dev), torch.randn(n * R, 256, 14, 14, device=dev)]

            def boxes4():
                b = [Cv.GradBox() for _ in range(4)]
                for t in b:
                    t.taker = True
                return b

            def arm_pyramid():
                u = [train16.unpack(m) for m in ps]
                maps = u + [u[3][:, :, ::2, ::2]]
                with torch.no_grad():
                    for m in maps:
                        rpn(m)
                to_rpn = boxes4()
                rl, rb = rpn.forward_rows(maps, image, anchor, valid, grad_boxes=to_rpn + [None])
                up = stage.make_up_maps(u, give_to=to_rpn)
                group = CropGradGroup()
                c7 = stage._crop(up, boxes, ind, level, 7, group)
                c14 = stage._crop(up, boxes, ind, level, 14, group)
                return [rl, rb, c7, c14]

            def arm_crops():
                p6 = ps[3].detach()[:, :, ::2, ::2].contiguous(memory_format=cl)
                with torch.no_grad():
                    for m in ps + [p6]:
                        rpn(m)
                to_rpn = boxes4()
                rl, rb = rpn.forward_rows(ps + [ps[3]], image, anchor, valid, grad_boxes=to_rpn + [None],
                                          steps=[1, 1, 1, 1, 2])
                up = stage.make_up_maps(ps, give_to=to_rpn)
                c7, c14 = crops16.pyramid_crops16(up, [(boxes, ind, level, 7), (boxes, ind, level, 14)])
                return [rl, rb, c7, c14]

            def arm(name):
                Cv.prepare_step(stage)
                Cv.prepare_step(rpn)
                outs = arm_pyramid() if name == "pyramid" else arm_crops()
                torch.autograd.grad(outs, ps + params, d_out)

            names = ("pyramid", "crops")
            m, t = _timed({a: (lambda a=a: arm(a)) for a in names}, T_WARMUP, T_ROUNDS)
            peak = {}
            for a in names:
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                arm(a)
                torch.cuda.synchronize()
                peak[a] = (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20
            emit("  (b) p2..p5 -> RPN rows + crops, forward + backward: pyramid %.2f ms | crops %.2f ms | pyramid / crops %.2f%s"
                 % (m["pyramid"], m["crops"], m["pyramid"] / m["crops"],
                    "" if m["crops"] <= m["pyramid"] else "   <- 'crops' loses"))
            emit("      min .. max of the timed rounds: " + " | ".join("%s %.2f .. %.2f" % (a, min(t[a]), max(t[a])) for a in names))
            emit("      peak memory of the segment above what was held before it (MiB): " +
                 " | ".join("%s %.0f" % (a, peak[a]) for a in names))
            del ps, params, d_out, boxes, rpn, stage
            torch.cuda.empty_cache()
        Cv.set_conv_precision("fp32")


if __name__ == "__main__":
    main()
