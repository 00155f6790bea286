"""conv3x3_patch_kernel alone on the chip: TFLOP/s by shape (in-library HIP events)."""
import os, sys, json, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from feature_intertwiner_amd import _lib
from feature_intertwiner_amd.conv import _conv_fwd
DEV = "cuda:0"
def run(name, N, Cin, H, W, Cout, key, iters=20):
    x = torch.randn(N, Cin, H, W, device=DEV)
    w = (torch.randn(Cout, Cin, 3, 3, device=DEV) * 0.05).contiguous(memory_format=torch.channels_last)
    sc = torch.rand(Cout, device=DEV) + 0.5; b = torch.randn(Cout, device=DEV)
    for _ in range(3): _conv_fwd(x, w, b, (1, 1), (1, 1), relu=True, scale=sc)
    torch.cuda.synchronize(); _lib.prof_reset(); _lib.prof_enable(True)
    for _ in range(iters): _conv_fwd(x, w, b, (1, 1), (1, 1), relu=True, scale=sc)
    torch.cuda.synchronize(); _lib.prof_enable(False)
    n, ms = _lib.prof_get(key); us = ms / max(n, 1) * 1e3 or float("nan"); fl = 2.0 * N * H * W * Cin * Cout * 9
    print(json.dumps({"layer": name, "us": round(us, 1), "TFLOPs": round(fl / us / 1e6, 1), "n": n,
                      "tiles": ((N * H * W + 127) // 128) * ((Cout + 127) // 128)}))
run("C4 3x3 256 N4 (256 tiles)", 4, 256, 64, 64, 256, "conv3x3_patch")
run("C4 3x3 256 N8 (512 tiles)", 8, 256, 64, 64, 256, "conv3x3_patch")
run("C4 3x3 256 N12 (768 tiles)", 12, 256, 64, 64, 256, "conv3x3_patch")
run("C4 3x3 256 N16 (1024 tiles)", 16, 256, 64, 64, 256, "conv3x3_patch")
run("C5 3x3 512 N4 (128 tiles)", 4, 512, 32, 32, 512, "conv3x3_patch")
run("C3 3x3 128 N4 (512 tiles)", 4, 128, 128, 128, 128, "conv3x3_patch")
run("FPN P2 3x3 256", 4, 256, 256, 256, 256, "conv3x3_patch")
run("mask 14x14 256 N1376", 1376, 256, 14, 14, 256, "conv3x3_patch_flat")
run("mask 14x14 256 N672", 672, 256, 14, 14, 256, "conv3x3_patch_flat")


def run_flat(name, N, Cin, Cout=256, H=14, W=14, key="conv3x3_patch_flat", rounds=5, iters=8, flip=False):
    """A patch slot (flat or 2-D) three ways -- its Winograd form with the planned input staging, the same with
    FI_WINO_SCALAR_STAGING=1 (4-byte loads only) and the direct kernel (FI_NO_WINOGRAD=1); the library reads both switches per
    call -- in rounds of the three interleaved in this process on the same random data: median, min and spread (max - min) in
    us per variant, TFLOP/s in direct-form flops (the Winograd form issues 16/36 of the MFMAs, so its figure may read above
    the MFMA peak).  flip: the data gradient (tap-major weights applied in reverse order).  On a shape the planner keeps on
    the direct kernel the variants are the same launch and the ratios read 1."""
    x = torch.randn(N, Cin, H, W, device=DEV)
    w = (torch.randn(Cout, Cin, 3, 3, device=DEV) * 0.05).contiguous(memory_format=torch.channels_last)
    if flip: w = w.permute(0, 2, 3, 1).contiguous()
    sc = torch.rand(Cout, device=DEV) + 0.5; b = torch.randn(Cout, device=DEV)
    kw = dict(w_tap_major=True, flip_taps=True) if flip else {}
    switch = {"winograd": None, "winograd_scalar_staging": "FI_WINO_SCALAR_STAGING", "direct": "FI_NO_WINOGRAD"}
    us = {v: [] for v in switch}
    for r in range(rounds + 1):
        for variant, env in switch.items():
            for e in switch.values():
                if e: os.environ.pop(e, None)
            if env: os.environ[env] = "1"
            torch.cuda.synchronize(); _lib.prof_reset(); _lib.prof_enable(True)
            for _ in range(iters): _conv_fwd(x, w, b, (1, 1), (1, 1), relu=True, scale=sc, **kw)
            torch.cuda.synchronize(); _lib.prof_enable(False)
            n, ms = _lib.prof_get(key); assert n == iters, (n, iters)
            if r: us[variant].append(ms / n * 1e3)                 # round 0 warms up
    for e in switch.values():
        if e: os.environ.pop(e, None)
    fl = 2.0 * N * H * W * Cin * Cout * 9; out = {"layer": name}
    for variant, v in us.items():
        v.sort(); med = v[len(v) // 2]
        out[variant] = {"us_median": round(med, 1), "us_min": round(v[0], 1), "us_spread": round(v[-1] - v[0], 1),
                        "TFLOPs_direct_form": round(fl / med / 1e6, 1)}
    out["speedup_median"] = round(out["direct"]["us_median"] / out["winograd"]["us_median"], 3)
    out["ratio_scalar_staging_over_winograd"] = round(out["winograd_scalar_staging"]["us_median"] / out["winograd"]["us_median"], 3)
    print(json.dumps(out), flush=True)


for n_img in (1376, 672):
    for cin in (256, 128, 64):
        run_flat("mask 14x14 %d->256 N%d" % (cin, n_img), n_img, cin)
# the 2-D slot, one line per grid size of a batch-4 step at 1024 x 1024 (workgroups of the direct kernel in brackets)
for name, N, Cin, H, W, Cout in (("C4 / P4 64x64 256->256 N4 (256)", 4, 256, 64, 64, 256),
                                 ("C3 128x128 128->128 N4 (512)", 4, 128, 128, 128, 128),
                                 ("P3 128x128 256->256 N4 (1024)", 4, 256, 128, 128, 256),
                                 ("RPN P3 128x128 256->512 N4 (2048)", 4, 256, 128, 128, 512),
                                 ("FPN P2 256x256 256->256 N4 (4096)", 4, 256, 256, 256, 256),
                                 ("RPN P2 256x256 256->512 N4 (8192)", 4, 256, 256, 256, 512)):
    run_flat(name, N, Cin, Cout, H, W, key="conv3x3_patch")
# the data gradient (taps reversed) of one layer of each slot
run_flat("mask 14x14 256->256 N1376 dgrad", 1376, 256, flip=True)
run_flat("FPN P2 256x256 256->256 N4 (4096) dgrad", 4, 256, 256, 256, 256, key="conv3x3_patch", flip=True)
