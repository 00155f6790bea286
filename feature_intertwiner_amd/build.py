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


def _api(name):
    return os.path.join("..", "..", "include", name)


# every object depends on these
HEADERS = ["fi_common.h", _api("fi_capi.h")]
# device code that several libraries share, each stated here once
CROP_DEV_HEADERS = ["crop_dev.h"]              # crop_and_resize.hip, crop_roi16.hip, head16_crop.hip, heads16.hip
ACT16_DEV_HEADERS = ["conv_act16_dev.h"]       # the 16-bit conv libraries
SINKHORN_HEADERS = ["sinkhorn_dev.h"]          # sinkhorn.hip, sinkhorn_bp.hip
# stem -> (sources, headers of the library besides HEADERS), in build and link order: libfi_<stem>.so.  The first is the
# core library; every other one is linked against it.
LIBRARIES = {
    "hip": (["fi_core.hip", "crop_and_resize.hip", "roi_pool.hip", "nms.hip", "sinkhorn.hip", "class_mean.hip",
             "conv_igemm.hip", "conv1x1_ring.hip", "conv3x3_wino.hip", "conv3x3_wino_wgrad.hip", "conv_bf16.hip",
             "conv_f16.hip", "sgd.hip", "glue.hip", "proposal.hip", "targets.hip", "losses.hip", "dev_stage.hip",
             "meta_stats.hip"], []),
    # the evaluation path: inference post-processing, COCO evaluation of the result dicts, COCO polygons -> RLE
    "eval": (["unmold.hip"], [_api("fi_eval.h")]),
    "cocoeval": (["cocoeval.hip"], [_api("fi_cocoeval.h")]),
    "cocomask": (["cocomask.hip"], [_api("fi_cocomask.h")]),
    # the Sinkhorn term differentiated through its iterations
    "ot": (["sinkhorn_bp.hip"], SINKHORN_HEADERS + [_api("fi_ot.h")]),
    # the transposed 3x3 / stride 2 convolution of the 2x make-up layer
    "convt": (["conv_transpose.hip"], [_api("fi_convt.h")]),
    # 16-bit channels-last inference: trunk convolutions and boundary casts, pyramid laterals and RPN heads, RoIAlign from
    # 16-bit maps, the box and mask heads on 16-bit crops
    "act16": (["conv_act16.hip", "conv_act16_f16.hip"], ACT16_DEV_HEADERS + [_api("fi_act16.h")]),
    "pyr16": (["conv_pyr16.hip", "conv_pyr16_f16.hip"], ACT16_DEV_HEADERS + [_api("fi_pyr16.h")]),
    "roi16": (["crop_roi16.hip", "crop_roi16_f16.hip"], CROP_DEV_HEADERS + [_api("fi_roi16.h")]),
    "head16": (["head16_crop.hip", "head16_crop_f16.hip", "head16_out.hip", "head16_out_f16.hip"],
               CROP_DEV_HEADERS + ACT16_DEV_HEADERS + [_api("fi_head16.h")]),
    # 16-bit channels-last training: ReLU mask / data / weight gradient, the gated data gradient, the pyramid's top-down
    # backward, patch rows and the gate-pack of RoIAlign's gradient, RoIAlign's and the class-selected layer's backward
    "grad16": (["conv_grad16.hip", "conv_grad16_f16.hip"], ACT16_DEV_HEADERS + [_api("fi_grad16.h")]),
    "train16": (["conv_train16.hip", "conv_train16_f16.hip"], ACT16_DEV_HEADERS + [_api("fi_train16.h")]),
    "fpn16": (["fpn16.hip", "fpn16_f16.hip"], ACT16_DEV_HEADERS + [_api("fi_fpn16.h")]),
    "crops16": (["crops16.hip", "crops16_f16.hip"], ACT16_DEV_HEADERS + [_api("fi_crops16.h")]),
    "heads16": (["heads16.hip", "heads16_f16.hip"], CROP_DEV_HEADERS + ACT16_DEV_HEADERS + [_api("fi_heads16.h")]),
}
# what one source depends on besides its library's headers.  X_f16.hip is `#define FI_E16_HALF 1` + `#include "X.hip"`: that
# dependency is a rule (source_deps); conv_f16.hip, which includes conv_bf16.hip, is the one twin the rule does not name.
_TWIN = "_f16.hip"
SOURCE_DEPS = {
    "crop_and_resize.hip": CROP_DEV_HEADERS,
    "sinkhorn.hip": SINKHORN_HEADERS,
    "conv_f16.hip": ["conv_bf16.hip"],
}


def lib_path(stem):
    return os.path.join(_HERE, "libfi_%s.so" % stem)


# the names tests and tools read
(LIB_PATH, EVAL_LIB_PATH, COCOEVAL_LIB_PATH, COCOMASK_LIB_PATH, OT_LIB_PATH, CONVT_LIB_PATH, ACT16_LIB_PATH, PYR16_LIB_PATH,
 ROI16_LIB_PATH, HEAD16_LIB_PATH, GRAD16_LIB_PATH, TRAIN16_LIB_PATH, FPN16_LIB_PATH, CROPS16_LIB_PATH,
 HEADS16_LIB_PATH) = (lib_path(stem) for stem in LIBRARIES)
SOURCES = LIBRARIES["hip"][0]
ROI16_HEADERS, HEAD16_HEADERS = LIBRARIES["roi16"][1], LIBRARIES["head16"][1]

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


def source_deps(stem, source):
    """The files whose change makes the object of `source`, a source of libfi_<stem>.so, stale."""
    names = [source] + HEADERS + LIBRARIES[stem][1] + SOURCE_DEPS.get(source, [])
    if source.endswith(_TWIN):
        twin_of = source[:-len(_TWIN)] + ".hip"
        if os.path.exists(os.path.join(CSRC, twin_of)):
            names.append(twin_of)
    return [os.path.normpath(os.path.join(CSRC, n)) for n in names]


def _compile(stem, force, verbose):
    objs = []
    for source in LIBRARIES[stem][0]:
        s = os.path.join(CSRC, source)
        if not os.path.exists(s):
            continue
        o = s[:-4] + ".o"
        if force or _stale(o, source_deps(stem, source)):
            cmd = [HIPCC] + FLAGS + ["-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd)
        objs.append(o)
    return objs


def build_hip(force=False, verbose=False):
    """Builds libfi_<stem>.so for every stem of LIBRARIES, in its order; returns the path of the first (libfi_hip.so)."""
    for stem in LIBRARIES:
        lib, objs = lib_path(stem), _compile(stem, force, verbose)
        core = stem == "hip"
        if force or _stale(lib, objs + ([] if core else [LIB_PATH])):
            cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs + (
                [] if core else ["-L" + _HERE, "-lfi_hip", "-Wl,-rpath,$ORIGIN"])
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd)
    return LIB_PATH


if __name__ == "__main__":
    print(build_hip(force="--force" in sys.argv, verbose=True))
