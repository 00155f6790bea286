"""The 3x3 / stride 1 weight-gradient slot per step shape: its Winograd form (csrc/conv3x3_wino_wgrad.hip) against the
direct kernel (FI_NO_WINOGRAD_WGRAD=1; the library reads the switch per call), rounds of the two interleaved in this process
on the same random data (in-library HIP events).  Medians of 5 rounds of 8 launches as us, the spread of the rounds, the
ratio and TFLOP/s in direct-form flops (the Winograd form issues 16/36 of the MFMAs, so its figure may read above the MFMA
peak).  On a shape the planner keeps on the direct kernel the two variants are the same launch and the ratio reads 1.
The BATCHES rows are the bottleneck blocks of C4 and C5 as fi_conv2d_weight_grad_batch launches them: n problems with
operands of their own in ONE launch of either kernel; us is the launch, us_per_problem its n-th.
winograd_scalar_staging is the Winograd form with FI_WINO_WGRAD_SCALAR_STAGING=1 (4-byte loads only, the staging before the
paired centre columns), in the same rounds.

    python scripts/wino_wgrad_probe.py [OUT.txt]        (default: profiles/wino_wgrad_probe.txt)"""
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from feature_intertwiner_amd import _lib  # noqa: E402

DEV = "cuda:0"
SWITCH = "FI_NO_WINOGRAD_WGRAD"
STAGING = "FI_WINO_WGRAD_SCALAR_STAGING"
# a batch-4 step at 1024 x 1024 with 512 RoIs per image (672 mask-head rows): every single-problem 3x3 / stride 1 launch
# with Cin >= 256 (the C4 / C5 blocks go through the batch entry: BATCHES below)
SHAPES = (("mask head 14x14 256->256 N672", 672, 256, 14, 14, 256, False),
          ("FPN P2 256x256 256->256 N4", 4, 256, 256, 256, 256, False),
          ("FPN P3 128x128 256->256 N4", 4, 256, 128, 128, 256, False),
          ("FPN P4 64x64 256->256 N4", 4, 256, 64, 64, 256, False),
          ("FPN P5 32x32 256->256 N4", 4, 256, 32, 32, 256, False),
          ("RPN P2 256x256 256->512 N4", 4, 256, 256, 256, 512, True),
          ("RPN P3 128x128 256->512 N4", 4, 256, 128, 128, 512, True),
          ("RPN P4 64x64 256->512 N4", 4, 256, 64, 64, 512, True),
          ("RPN P5 32x32 256->512 N4", 4, 256, 32, 32, 512, True),
          ("RPN P6 16x16 256->512 N4", 4, 256, 16, 16, 512, True),
          ("C5 32x32 512->512 N4 (one problem)", 4, 512, 32, 32, 512, False))
# the batched launches of that step: ResNet-101's 23 C4 blocks travel as 11 + 12 (conv's queue), the 3 C5 blocks as one
BATCHES = (("C4 64x64 256->256 N4 x11", 11, 4, 256, 64, 64, 256),
           ("C4 64x64 256->256 N4 x12", 12, 4, 256, 64, 64, 256),
           ("C5 32x32 512->512 N4 x3", 3, 4, 512, 32, 32, 512))


def run(name, N, Cin, H, W, Cout, bias, rounds=5, iters=8, nb=1):
    L = _lib.load()
    xs = [torch.randn(N, Cin, H, W, device=DEV) for _ in range(nb)]
    dys = [torch.randn(N, Cout, H, W, device=DEV) for _ in range(nb)]
    dws = [torch.zeros(Cout, 3, 3, Cin, device=DEV) for _ in range(nb)]
    x, dy, dw = xs[0], dys[0], dws[0]
    db = torch.zeros(Cout, device=DEV) if bias else None
    geom = (N, Cin, H, W, Cout, 3, 3, 1, 1, 1, 1, 1)
    args = (_lib.ptr(x), _lib.ptr(dy), _lib.ptr(dw)) + geom + (_lib.ptr(db), _lib.OUTPUTS_ZEROED)
    arr = lambda ts: (ctypes.c_void_p * nb)(*[t.data_ptr() for t in ts])
    bargs = (arr(xs), arr(dys), arr(dws), None, nb) + geom + (_lib.OUTPUTS_ZEROED,)
    us = {"winograd": [], "winograd_scalar_staging": [], "direct": []}
    plan = {}
    for r in range(rounds + 1):
        for variant in us:
            os.environ.pop(SWITCH, None)
            os.environ.pop(STAGING, None)
            if variant == "direct":
                os.environ[SWITCH] = "1"
            elif variant == "winograd_scalar_staging":
                os.environ[STAGING] = "1"
            (p,) = _lib.planned_launches(L.fi_conv2d_weight_grad_launch, *args, nb)
            key = _lib.KERNEL_KEYS[p.kernel_id]
            assert p.per_launch == nb, (p.per_launch, nb)
            plan[variant] = {"winograd": bool(p.flags & _lib.LAUNCH_FLAGS["winograd"]), "key": key,
                             "grid": [p.grid_x, p.grid_y, p.splits]}
            torch.cuda.synchronize()
            _lib.prof_reset()
            _lib.prof_enable(True)
            for _ in range(iters):
                if nb > 1:
                    _lib.check(L.fi_conv2d_weight_grad_batch(*bargs, _lib.current_stream()), "fi_conv2d_weight_grad_batch")
                else:
                    _lib.check(L.fi_conv2d_weight_grad(*args, _lib.current_stream()), "fi_conv2d_weight_grad")
            torch.cuda.synchronize()
            _lib.prof_enable(False)
            n, ms = _lib.prof_get(key)
            assert n == iters, (n, iters)
            if r:                                                      # round 0 warms up
                us[variant].append(ms / n * 1e3)
    os.environ.pop(SWITCH, None)
    os.environ.pop(STAGING, None)
    fl = 2.0 * N * H * W * Cin * Cout * 9 * nb
    out = {"layer": name}
    for variant, v in us.items():
        v.sort()
        med = v[len(v) // 2]
        out[variant] = dict(plan[variant], us_median=round(med, 1), us_min=round(v[0], 1), us_max=round(v[-1], 1),
                            TFLOPs_direct_form=round(fl / med / 1e6, 1))
        if nb > 1:
            out[variant]["us_per_problem"] = round(med / nb, 1)
    out["ratio_direct_over_winograd"] = round(out["direct"]["us_median"] / out["winograd"]["us_median"], 3)
    out["ratio_scalar_staging_over_winograd"] = round(out["winograd_scalar_staging"]["us_median"] / out["winograd"]["us_median"], 3)
    out["spread"] = round(max((v[-1] - v[0]) / v[len(v) // 2] for v in us.values()), 3)
    return json.dumps(out)


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "wino_wgrad_probe.txt")
    lines = [run(*s) for s in SHAPES] + [run(b[0], *b[2:], False, nb=b[1]) for b in BATCHES]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
