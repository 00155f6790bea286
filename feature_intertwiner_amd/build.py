"""Build libfi_hip.so (hand-written HIP kernels + C ABI) for gfx950 with hipcc.

In-tree build: the shared object is written next to this file so that it travels
to the GPU box with the repository snapshot.  Usage:

    python -m feature_intertwiner_amd.build [--force]
"""
import os
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.path.join(_HERE, "libfi_hip.so")
SOURCES = ["fi_core.hip", "crop_and_resize.hip", "roi_pool.hip", "nms.hip", "sinkhorn.hip",
           "class_mean.hip", "conv_igemm.hip", "conv1x1_ring.hip", "conv3x3_wino.hip", "conv3x3_wino_wgrad.hip", "conv_bf16.hip", "conv_f16.hip", "sgd.hip", "glue.hip", "proposal.hip", "targets.hip", "losses.hip", "dev_stage.hip", "meta_stats.hip"]
HEADERS = ["fi_common.h", os.path.join("..", "..", "include", "fi_capi.h")]
# device code that crop_and_resize.hip (libfi_hip.so), crop_roi16.hip (libfi_roi16.so) and head16_crop.hip
# (libfi_head16.so) share
CROP_DEV_HEADERS = ["crop_dev.h"]
# device code that sinkhorn.hip (libfi_hip.so) and sinkhorn_bp.hip (libfi_ot.so) share
SINKHORN_HEADERS = ["sinkhorn_dev.h"]
# the evaluation path (inference post-processing, include/fi_eval.h): its own library, linked against libfi_hip.so
EVAL_LIB_PATH = os.path.join(_HERE, "libfi_eval.so")
EVAL_SOURCES = ["unmold.hip"]
EVAL_HEADERS = [os.path.join("..", "..", "include", "fi_eval.h")]
# COCO evaluation of the result dicts (include/fi_cocoeval.h): a third library, built the same way
COCOEVAL_LIB_PATH = os.path.join(_HERE, "libfi_cocoeval.so")
COCOEVAL_SOURCES = ["cocoeval.hip"]
COCOEVAL_HEADERS = [os.path.join("..", "..", "include", "fi_cocoeval.h")]
# COCO polygon ground truth -> RLE (include/fi_cocomask.h): a fourth library, built the same way
COCOMASK_LIB_PATH = os.path.join(_HERE, "libfi_cocomask.so")
COCOMASK_SOURCES = ["cocomask.hip"]
COCOMASK_HEADERS = [os.path.join("..", "..", "include", "fi_cocomask.h")]
# the Sinkhorn term differentiated through its iterations (include/fi_ot.h): a fifth library, built the same way
OT_LIB_PATH = os.path.join(_HERE, "libfi_ot.so")
OT_SOURCES = ["sinkhorn_bp.hip"]
OT_HEADERS = SINKHORN_HEADERS + [os.path.join("..", "..", "include", "fi_ot.h")]
# the transposed 3x3 / stride 2 convolution of the 2x make-up layer (include/fi_convt.h): a sixth library, built the same way
CONVT_LIB_PATH = os.path.join(_HERE, "libfi_convt.so")
CONVT_SOURCES = ["conv_transpose.hip"]
CONVT_HEADERS = [os.path.join("..", "..", "include", "fi_convt.h")]
# convolutions on 16-bit channels-last activation tensors and the casts at their boundary (include/fi_act16.h): a seventh
# library, built the same way
ACT16_LIB_PATH = os.path.join(_HERE, "libfi_act16.so")
ACT16_SOURCES = ["conv_act16.hip", "conv_act16_f16.hip"]
# device code that conv_act16.hip (libfi_act16.so), conv_pyr16.hip (libfi_pyr16.so) and head16_out.hip (libfi_head16.so)
# share
ACT16_DEV_HEADERS = ["conv_act16_dev.h"]
ACT16_HEADERS = ACT16_DEV_HEADERS + [os.path.join("..", "..", "include", "fi_act16.h")]
# the pyramid's lateral step and the RPN's stacked heads on 16-bit channels-last tensors (include/fi_pyr16.h): an eighth
# library, built the same way
PYR16_LIB_PATH = os.path.join(_HERE, "libfi_pyr16.so")
PYR16_SOURCES = ["conv_pyr16.hip", "conv_pyr16_f16.hip"]
PYR16_HEADERS = ACT16_DEV_HEADERS + [os.path.join("..", "..", "include", "fi_pyr16.h")]
# RoIAlign that reads 16-bit channels-last pyramid maps (include/fi_roi16.h): a ninth library, built the same way
ROI16_LIB_PATH = os.path.join(_HERE, "libfi_roi16.so")
ROI16_SOURCES = ["crop_roi16.hip", "crop_roi16_f16.hip"]
ROI16_HEADERS = CROP_DEV_HEADERS + [os.path.join("..", "..", "include", "fi_roi16.h")]
# the box and mask heads on 16-bit channels-last crops -- RoIAlign that writes them, the fp32 output layer behind them
# (include/fi_head16.h): a tenth library, built the same way
HEAD16_LIB_PATH = os.path.join(_HERE, "libfi_head16.so")
HEAD16_SOURCES = ["head16_crop.hip", "head16_crop_f16.hip", "head16_out.hip", "head16_out_f16.hip"]
HEAD16_HEADERS = CROP_DEV_HEADERS + ACT16_DEV_HEADERS + [os.path.join("..", "..", "include", "fi_head16.h")]
# the backward operators of a convolution on 16-bit channels-last tensors -- ReLU mask + column sums, data gradient,
# weight gradient (include/fi_grad16.h): an eleventh library, built the same way
GRAD16_LIB_PATH = os.path.join(_HERE, "libfi_grad16.so")
GRAD16_SOURCES = ["conv_grad16.hip", "conv_grad16_f16.hip"]
GRAD16_HEADERS = ACT16_DEV_HEADERS + [os.path.join("..", "..", "include", "fi_grad16.h")]
# the data gradient with the producing layer's ReLU mask and column sums in its epilogue, for training on 16-bit
# channels-last tensors (include/fi_train16.h): a twelfth library, built the same way
TRAIN16_LIB_PATH = os.path.join(_HERE, "libfi_train16.so")
TRAIN16_SOURCES = ["conv_train16.hip", "conv_train16_f16.hip"]
TRAIN16_HEADERS = ACT16_DEV_HEADERS + [os.path.join("..", "..", "include", "fi_train16.h")]
# the backward of the feature pyramid's top-down step on 16-bit channels-last tensors -- the 2 x 2 sum of the finer level's
# gradient, the add and the column sums in one launch (include/fi_fpn16.h): a thirteenth library, built the same way
FPN16_LIB_PATH = os.path.join(_HERE, "libfi_fpn16.so")
FPN16_SOURCES = ["fpn16.hip", "fpn16_f16.hip"]
FPN16_HEADERS = ACT16_DEV_HEADERS + [os.path.join("..", "..", "include", "fi_fpn16.h")]
# what keeps a train step's pyramid 16-bit up to the RoI crops -- the RPN's patch rows gathered from and scattered into
# 16-bit maps, the masked pack of RoIAlign's fp32 gradient with column sums (include/fi_crops16.h): a fourteenth library,
# built the same way
CROPS16_LIB_PATH = os.path.join(_HERE, "libfi_crops16.so")
CROPS16_SOURCES = ["crops16.hip", "crops16_f16.hip"]
CROPS16_HEADERS = ACT16_DEV_HEADERS + [os.path.join("..", "..", "include", "fi_crops16.h")]
# what lets a train step run its box and mask heads on 16-bit channels-last crops -- RoIAlign's backward from 16-bit crop
# gradients, the backward of the mask head's class-selected output layer (include/fi_heads16.h): a fifteenth library, built
# the same way
HEADS16_LIB_PATH = os.path.join(_HERE, "libfi_heads16.so")
HEADS16_SOURCES = ["heads16.hip", "heads16_f16.hip"]
HEADS16_HEADERS = CROP_DEV_HEADERS + ACT16_DEV_HEADERS + [os.path.join("..", "..", "include", "fi_heads16.h")]

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = [
    "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
    # bit-exact coordinate / IoU arithmetic: no fused multiply-add contraction
    "-ffp-contract=off",
    # hardware fp32 atomic add (global_atomic_add_f32) for the scatter kernels
    "-munsafe-fp-atomics",
    "-Wall", "-Wno-unused-function",
    # the ring kernel's LDS-DMA asm names m0 as clobbered (a reserved register: clang warns per use)
    "-Wno-inline-asm",
] + os.environ.get("FI_EXTRA_HIPCC_FLAGS", "").split()          # e.g. -DFI_PROBE_1X1 (scripts/c4_probe.sh)


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _compile(sources, headers, force, verbose):
    srcs = [os.path.join(CSRC, s) for s in sources if os.path.exists(os.path.join(CSRC, s))]
    hdrs = [os.path.normpath(os.path.join(CSRC, h)) for h in headers]
    objs = []
    for s in srcs:
        o = s[:-4] + ".o"
        deps = [s] + hdrs + ([os.path.join(CSRC, "conv_bf16.hip")] if s.endswith("conv_f16.hip") else [])
        deps += [os.path.join(CSRC, h) for h in SINKHORN_HEADERS] if s.endswith("sinkhorn.hip") else []
        deps += [os.path.join(CSRC, "conv_act16.hip")] if s.endswith("conv_act16_f16.hip") else []
        deps += [os.path.join(CSRC, "conv_pyr16.hip")] if s.endswith("conv_pyr16_f16.hip") else []
        deps += [os.path.join(CSRC, h) for h in CROP_DEV_HEADERS] if s.endswith("crop_and_resize.hip") else []
        deps += [os.path.join(CSRC, "crop_roi16.hip")] if s.endswith("crop_roi16_f16.hip") else []
        deps += [os.path.join(CSRC, "head16_crop.hip")] if s.endswith("head16_crop_f16.hip") else []
        deps += [os.path.join(CSRC, "head16_out.hip")] if s.endswith("head16_out_f16.hip") else []
        deps += [os.path.join(CSRC, "conv_grad16.hip")] if s.endswith("conv_grad16_f16.hip") else []
        deps += [os.path.join(CSRC, "conv_train16.hip")] if s.endswith("conv_train16_f16.hip") else []
        deps += [os.path.join(CSRC, "fpn16.hip")] if s.endswith("fpn16_f16.hip") else []
        deps += [os.path.join(CSRC, "crops16.hip")] if s.endswith("crops16_f16.hip") else []
        deps += [os.path.join(CSRC, "heads16.hip")] if s.endswith("heads16_f16.hip") else []
        if force or _stale(o, deps):
            cmd = [HIPCC] + FLAGS + ["-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd)
        objs.append(o)
    return objs


def build_hip(force=False, verbose=False):
    """Builds libfi_hip.so, libfi_eval.so, libfi_cocoeval.so, libfi_cocomask.so, libfi_ot.so, libfi_convt.so,
    libfi_act16.so, libfi_pyr16.so, libfi_roi16.so, libfi_head16.so, libfi_grad16.so, libfi_train16.so,
    libfi_fpn16.so, libfi_crops16.so and libfi_heads16.so; returns the path of the first."""
    objs = _compile(SOURCES, HEADERS, force, verbose)
    if force or _stale(LIB_PATH, objs):
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_PATH] + objs
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    for lib, sources, headers in ((EVAL_LIB_PATH, EVAL_SOURCES, EVAL_HEADERS),
                                  (COCOEVAL_LIB_PATH, COCOEVAL_SOURCES, COCOEVAL_HEADERS),
                                  (COCOMASK_LIB_PATH, COCOMASK_SOURCES, COCOMASK_HEADERS),
                                  (OT_LIB_PATH, OT_SOURCES, OT_HEADERS),
                                  (CONVT_LIB_PATH, CONVT_SOURCES, CONVT_HEADERS),
                                  (ACT16_LIB_PATH, ACT16_SOURCES, ACT16_HEADERS),
                                  (PYR16_LIB_PATH, PYR16_SOURCES, PYR16_HEADERS),
                                  (ROI16_LIB_PATH, ROI16_SOURCES, ROI16_HEADERS),
                                  (HEAD16_LIB_PATH, HEAD16_SOURCES, HEAD16_HEADERS),
                                  (GRAD16_LIB_PATH, GRAD16_SOURCES, GRAD16_HEADERS),
                                  (TRAIN16_LIB_PATH, TRAIN16_SOURCES, TRAIN16_HEADERS),
                                  (FPN16_LIB_PATH, FPN16_SOURCES, FPN16_HEADERS),
                                  (CROPS16_LIB_PATH, CROPS16_SOURCES, CROPS16_HEADERS),
                                  (HEADS16_LIB_PATH, HEADS16_SOURCES, HEADS16_HEADERS)):
        objs = _compile(sources, HEADERS + headers, force, verbose)
        if force or _stale(lib, objs + [LIB_PATH]):
            cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs + [
                "-L" + _HERE, "-lfi_hip", "-Wl,-rpath,$ORIGIN"]
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd)
    return LIB_PATH


if __name__ == "__main__":
    print(build_hip(force="--force" in sys.argv, verbose=True))
