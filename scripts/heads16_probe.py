"""The box and mask heads of a train step on 16-bit channels-last crops (TRAIN.ACT_SCOPE = 'heads',
feature_intertwiner_amd/heads16.py, libfi_heads16.so) against 'crops' (fp32 NCHW crops, the heads on fp32 tensors), at the
shapes of ResNet-101's heads: 2 x 1344^2 with 1000 RoIs per image and 4 x 1024^2 with 512, bf16 and fp16.

In ONE process on one MI355X, the arms taking turns inside every round, each launch 10 times back to back inside a HIP event
pair (the window / 10), 5 warm-up and 20 timed rounds, medians:
  crop backward   fi_heads16_pyramid_crop_backward on a 16-bit channels-last crop gradient, clearing the four fp32
                  channels-last maps first, for the 7 x 7 crops of every RoI and for the 14 x 14 crops of the mask head's
                  graph batch (a third of the slots), against what a step does with such a gradient today: widen and
                  transpose it to fp32 NCHW (one torch copy) and run fi_pyramid_crop_backward_nhwc.  The share of the
                  atomic rate is (boxes x bins x channels x 4 taps x 4 bytes) / time over 1.3 TB/s of added bytes (the
                  chip-wide rate of global fp32 atomics): an upper bound of the adds, since invalid taps add nothing.
  class rows      fi_heads16_class_rows_backward on the graph batch (u [n, 14, 14, 4 x 256], 81 classes), with its share of
                  the HBM peak (8 TB/s) from the bytes the shapes imply (2 + 2 per element of u and du, 4 per element of d),
                  against fi_class_row_conv1x1_backward (gated, with d weight and d bias) on the WIDENED fp32 tensor
                  [4 n, 256, 14, 14]; the widening itself is not timed.
  full window     the box head's 7 x 7 layer forward + backward on the crops of every RoI, 3 warm-up and 7 timed rounds:
                  heads16.window_bn_act16 on a 16-bit channels-last crop against conv.conv_bn_act on the fp32 crop.
  segment         forward + backward from the smoothed 16-bit p2..p5 (leaves that require grad) through the make-up layer,
                  the crops of both heads and of the feature extractor's rows, Classifier and Mask (graph batch with a
                  graph, rest batch without) to the class logits, the boxes, the selected mask logits and the feature
                  extractor's rows, a gradient into each, and back to the gate-packed map gradients and the make-up layer's
                  data gradients: heads16.pyramid_crops_heads16 and the heads' 16-bit branches against
                  crops16.pyramid_crops16, conv.take_rows with its GradBox and the heads on fp32 crops; conv.prepare_step
                  before every forward, MODEL.CONV_PRECISION of the type in both arms, 3 warm-up and 7 timed rounds, and the
                  peak of torch's allocator over one more, untimed, round of each arm.

    python scripts/heads16_probe.py [--out profiles/heads16_probe.txt] [--types bf16,fp16] [--sizes 1344,1024]
Run it under a time limit (timeout -k 10 600 python scripts/heads16_probe.py): a hung GPU step must end the command.
"""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from crops16_probe import HBM_PEAK, REPS, ROIS, ROUNDS, WARMUP, _timed      # noqa: E402  (the same timers and RoI counts)
from grad16_probe import SHAPES                                             # noqa: E402  (the same batch sizes)

ATOMIC_RATE = 1.3e12
CLASSES = 81


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heads16_probe.txt"))
    ap.add_argument("--types", default="bf16,fp16")
    ap.add_argument("--sizes", default="1344,1024")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    from feature_intertwiner_amd import _lib, act16, crops16, heads16
    from feature_intertwiner_amd.sub_module import Classifier, Dev, Mask
    from feature_intertwiner_amd import conv as Cv
    from feature_intertwiner_amd.config import make_config
    from feature_intertwiner_amd.intertwiner import roi_level
    dev = "cuda:0"
    lines = []

    def emit(line=""):
        lines.append(line)
        print(line, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:          # kept current: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")

    props = torch.cuda.get_device_properties(0)
    emit("heads16_probe: the heads of a train step on 16-bit crops vs on fp32 crops, %s (%s: the runtime's name for the "
         "MI355X), %d CUs" % (props.name, getattr(props, "gcnArchName", "?"), props.multi_processor_count))
    emit("arms alternating in one process, HIP event pairs, %d launches per window, medians, ms" % REPS)
    LN, LH = heads16.load(), _lib.load()
    p = _lib.ptr
    cl = torch.channels_last
    for prec in args.types.split(","):
        dtype = act16.dtype_of(prec)
        for size in [int(s) for s in args.sizes.split(",")]:
            n, R = SHAPES[size], ROIS[size]
            hw = [size // (1 << lvl) for lvl in (2, 3, 4, 5)]
            cfg = make_config(backbone="resnet101", image_size=size, batch_size=n, train_rois_per_image=R)
            emit()
            emit("== %s, %d x %d^2 (maps %d^2 .. %d^2, 256 channels), %d RoIs per image" % (prec, n, size, hw[0], hw[3], R))
            torch.manual_seed(2001)
            ctr = torch.rand(n * R, 2, device=dev)
            ext = 0.02 + 0.5 * torch.rand(n * R, 2, device=dev) ** 2
            boxes = torch.cat(((ctr - ext / 2).clamp(0, 1), (ctr + ext / 2).clamp(0, 1)), 1)
            ind = torch.arange(n, device=dev, dtype=torch.int32).repeat_interleave(R)
            level = roi_level(boxes, float(size * size), cfg.ROIS.ASSIGN_ANCHOR_BASE).to(torch.int32)
            bufs = [torch.empty(n, 256, h, h, device=dev).contiguous(memory_format=cl) for h in hw]
            ptrs = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in bufs])
            hs = (ctypes.c_int * 4)(*hw)
            stream = _lib.current_stream()
            f_new = Cv._lowp_fn(LN, "heads16_pyramid_crop_backward", prec)
            emit("  crop backward: crop, boxes | 16-bit channels-last ms, share of the 1.3 TB/s atomic rate | cast + transpose + "
                 "fp32 launch ms (copy | launch) | old / new")
            front = torch.arange(n * R, device=dev).view(n, R)[:, : R // 3].reshape(-1)
            for crop, sel in ((7, None), (14, front)):
                b, i, l = (boxes, ind, level) if sel is None else (boxes[sel].contiguous(), ind[sel].contiguous(),
                                                                  level[sel].contiguous())
                nb = b.shape[0]
                d16 = torch.randn(nb, crop, crop, 256, device=dev).to(dtype)
                state = {}

                def k_new():
                    assert f_new(p(d16), ptrs, hs, hs, 4, p(b), p(i), p(l), nb, n, 256, crop, crop, 0, stream) == 0

                def k_copy():
                    state["d"] = d16.permute(0, 3, 1, 2).float().contiguous()

                def k_old():
                    assert LH.fi_pyramid_crop_backward_nhwc(p(state["d"]), ptrs, hs, hs, 4, p(b), p(i), p(l), nb, n, 256, crop,
                                                            crop, stream) == 0

                k_copy()
                m, _ = _timed({"new": k_new, "copy": k_copy, "old": k_old}, WARMUP, ROUNDS, REPS)
                added = 16.0 * nb * crop * crop * 256
                old = m["copy"] + m["old"]
                emit("      %2d x %2d  %5d | %6.3f %5.1f %% | %6.3f (%6.3f | %6.3f) | %5.2f%s" % (
                    crop, crop, nb, m["new"], 100.0 * added / (m["new"] * 1e-3) / ATOMIC_RATE, old, m["copy"], m["old"],
                    old / m["new"], "" if m["new"] <= old else "   <- loses"))
                del d16, state
            # the class rows of the graph batch
            nf, C, H = front.numel(), 256, 14
            u16 = torch.relu(torch.randn(nf, 4 * C, H, H, device=dev)).to(dtype).contiguous(memory_format=cl)
            d = torch.randn(nf, 2, 2, H, H, device=dev)
            w32 = torch.randn(CLASSES, C, device=dev) / 16.0
            w16 = w32.to(dtype)
            cls = torch.randint(1, CLASSES, (nf,), device=dev)
            du = torch.empty_like(u16)
            colsum = torch.empty(4 * C, device=dev)
            dw, db = torch.zeros(CLASSES, C, device=dev), torch.zeros(CLASSES, device=dev)
            r_new = Cv._lowp_fn(LN, "heads16_class_rows_backward", prec)
            # the fp32 form reads rows (RoI, a, b) of [C, H, W]: u widened and re-laid-out (not timed)
            x32 = u16.float().contiguous().view(nf * 4, C, H * H)
            d4 = d.reshape(nf * 4, H * H).contiguous()
            cls4 = cls.view(-1, 1).expand(-1, 4).reshape(-1).contiguous()
            dx32 = torch.empty_like(x32)
            ws = torch.empty(LH.fi_class_row_conv1x1_workspace_bytes(nf * 4, C) // 4 + 1, device=dev)

            def c_new():
                assert r_new(p(d), p(u16), p(w16), p(cls), p(du), p(colsum), p(dw), p(db), nf, H, H, C, CLASSES, stream) == 0

            def c_old():
                assert LH.fi_class_row_conv1x1_backward(p(d4), p(x32), p(w32), p(cls4), p(dx32), p(dw), p(db), nf * 4, C, H * H,
                                                        CLASSES, 1, p(ws), stream) == 0

            m, _ = _timed({"new": c_new, "old": c_old}, WARMUP, ROUNDS, REPS)
            nbytes = 4.0 * u16.numel() + 4.0 * d.numel()
            emit("  class rows: n %d, 14 x 14, C 256, K %d | 16-bit ms %6.3f, %5.0f GB/s, %4.1f %% of 8 TB/s | fp32 on the widened "
                 "tensor ms %6.3f | old / new %5.2f%s" % (nf, CLASSES, m["new"], nbytes / m["new"] / 1e6,
                                                        100.0 * nbytes / (m["new"] * 1e-3) / HBM_PEAK, m["old"],
                                                        m["old"] / m["new"], "" if m["new"] <= m["old"] else "   <- loses"))
            del u16, du, x32, dx32, d, d4, bufs
            torch.cuda.empty_cache()
            # ---- the layers and the segment: real modules ---------------------------------------------------------------
            Cv.set_conv_precision(prec)
            cfg.TRAIN.ACT_PRECISION, cfg.TRAIN.ACT_SCOPE = prec, "heads"
            net = torch.nn.ModuleDict(dict(stage=Dev(cfg, 256), box=Classifier(256, CLASSES, 7, cfg), mask=Mask(256, CLASSES)))
            net = net.to(dev).eval()
            stage, box_head, mask_head = net["stage"], net["box"], net["mask"]
            with torch.no_grad():
                for m in net.modules():
                    if isinstance(m, torch.nn.BatchNorm2d):
                        m.running_mean.normal_(0.0, 0.5)
                        m.running_var.uniform_(0.25, 1.25)
            Cv.prepare_step(net)
            nR = n * R
            conv1, bn1 = box_head.conv1, box_head.bn1
            wts = [conv1.weight, conv1.bias, bn1.weight, bn1.bias]
            x32 = torch.randn(nR, 256, 7, 7, device=dev).requires_grad_()
            x16 = x32.detach().to(dtype).contiguous(memory_format=cl).requires_grad_()
            dy32 = torch.randn(nR, 1024, 1, 1, device=dev)
            dy16 = dy32.to(dtype).contiguous(memory_format=cl)

            def w_new():
                torch.autograd.grad([heads16.window_bn_act16(x16, conv1, bn1)], [x16] + wts, [dy16])

            def w_old():
                torch.autograd.grad([Cv.conv_bn_act(x32, conv1, bn1, relu=True)], [x32] + wts, [dy32])

            mw, _ = _timed({"new": w_new, "old": w_old}, 3, 7)
            emit("  full window, %d x 256 x 7 x 7 -> 1024, forward + backward: 16-bit %.3f ms | fp32 tensors %.3f ms | old / new "
                 "%.2f%s" % (nR, mw["new"], mw["old"], mw["old"] / mw["new"], "" if mw["new"] <= mw["old"] else "   <- loses"))
            del x32, x16, dy32, dy16
            # the segment
            ps = [torch.randn(n, 256, h, h, device=dev).to(dtype).contiguous(memory_format=cl).requires_grad_() for h in hw]
            P = R // 3
            slot = torch.arange(nR, device=dev).view(n, R)
            perm = torch.cat((slot[:, :P].reshape(-1), slot[:, P:].reshape(-1)))
            inv = torch.empty_like(perm)
            inv[perm] = torch.arange(nR, device=dev)
            order = torch.sort(level, stable=True)[1]
            sel_cls = torch.randint(1, CLASSES, (n * P,), device=dev)
            spec = lambda i, s: (boxes[i].contiguous(), ind[i].contiguous(), level[i].contiguous(), s)
            params = [q for q in net.parameters() if q.requires_grad]
            d_out = [torch.randn(nR, CLASSES, device=dev), torch.randn(nR, CLASSES, 4, device=dev),
                     torch.randn(n * P, 2, 2, 14, 14, device=dev), torch.randn(nR, 256, 14, 14, device=dev)]

            def arm(name):
                Cv.prepare_step(net)
                up = stage.make_up_maps(ps)
                if name == "crops":
                    c7, c14 = crops16.pyramid_crops16(up, [(boxes, ind, level, 7), spec(perm, 14)])
                    box = Cv.GradBox()
                    feat = Cv.take_rows(c14, inv[order], box)
                    logits, _, bbox = box_head(c7)
                    with torch.no_grad():
                        mask_head(c14[n * P:], shuffled=False, activate=False)
                    sel = mask_head(c14[:n * P], shuffled=False, activate=False, input_grad_box=box, select_class=sel_cls)
                else:
                    c7, graph, rest, feat = heads16.pyramid_crops_heads16(up, (boxes, ind, level, 7), spec(perm[:n * P], 14),
                                                                          spec(perm[n * P:], 14), spec(order, 14))
                    logits, _, bbox = box_head(c7)
                    with torch.no_grad():
                        mask_head(rest)
                    sel = mask_head(graph, shuffled=False, activate=False, select_class=sel_cls)
                torch.autograd.grad([logits, bbox, sel, feat], ps + params, d_out, allow_unused=True)

            names = ("crops", "heads")
            ms, ts = _timed({a: (lambda a=a: arm(a)) for a in names}, 3, 7)
            peak = {}
            for a in names:
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                arm(a)
                torch.cuda.synchronize()
                peak[a] = (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20
            emit("  segment p2..p5 -> make-up -> crops -> both heads + feature rows, forward + backward: crops %.2f ms | heads "
                 "%.2f ms | crops / heads %.2f%s" % (ms["crops"], ms["heads"], ms["crops"] / ms["heads"],
                                                    "" if ms["heads"] <= ms["crops"] else "   <- 'heads' loses"))
            emit("      min .. max of the timed rounds: " + " | ".join("%s %.2f .. %.2f" % (a, min(ts[a]), max(ts[a]))
                                                                       for a in names))
            emit("      peak memory of the segment above what was held before it (MiB): " +
                 " | ".join("%s %.0f" % (a, peak[a]) for a in names))
            del ps, params, d_out, net, stage, box_head, mask_head
            torch.cuda.empty_cache()
            Cv.set_conv_precision("fp32")


if __name__ == "__main__":
    main()
