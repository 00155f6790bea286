"""CPU: the one loader of the sub-libraries (_lib.load_sublibrary) and the one build table (build.LIBRARIES).  Nothing is
compiled and no kernel is launched here."""
import importlib
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "feature_intertwiner_amd", "csrc")
STEMS = ["hip", "eval", "cocoeval", "cocomask", "ot", "convt", "act16", "pyr16", "roi16", "head16", "grad16", "train16",
         "fpn16", "crops16", "heads16"]
# module, the name of its signature table, of its loader and of its path, its library, one entry point
MODULES = [("act16", "SIGNATURES", "load", "LIB_PATH", "act16", "fi_act16_conv_eligible"),
           ("pyr16", "SIGNATURES", "load", "LIB_PATH", "pyr16", "fi_pyr16_lateral_bf16"),
           ("roi16", "SIGNATURES", "load", "LIB_PATH", "roi16", "fi_roi16_pyramid_crop_forward_f16"),
           ("head16", "SIGNATURES", "load", "LIB_PATH", "head16", "fi_head16_out1x1_bf16"),
           ("grad16", "SIGNATURES", "load", "LIB_PATH", "grad16", "fi_grad16_conv_wgrad_f16"),
           ("train16", "SIGNATURES", "load", "LIB_PATH", "train16", "fi_train16_conv_dgrad_gated_bf16"),
           ("fpn16", "SIGNATURES", "load", "LIB_PATH", "fpn16", "fi_fpn16_topdown_grad_f16"),
           ("crops16", "SIGNATURES", "load", "LIB_PATH", "crops16", "fi_crops16_gate_pack_bf16"),
           ("heads16", "SIGNATURES", "load", "LIB_PATH", "heads16", "fi_heads16_class_rows_backward_f16"),
           ("cocoeval", "SIGNATURES", "load", "LIB_PATH", "cocoeval", "fi_coco_match_workspace_bytes"),
           ("cocomask", "SIGNATURES", "load", "LIB_PATH", "cocomask", "fi_cocomask_merge"),
           ("postprocess", "SIGNATURES", "load", "LIB_PATH", "eval", "fi_unmold_workspace_bytes"),
           ("OT_module", "OT_SIGNATURES", "load_ot", "OT_LIB_PATH", "ot", "fi_ot_sinkhorn_backprop"),
           ("conv", "CONVT_SIGNATURES", "load_convt", "CONVT_LIB_PATH", "convt", "fi_conv_transpose3x3s2_forward")]


# ---- the loader -------------------------------------------------------------------------------------------------------
def test_a_missing_library_names_the_file_and_the_build_command():
    from feature_intertwiner_amd import _lib, build
    build.build_hip()                            # the helper loads libfi_hip.so first
    with pytest.raises(_lib.FiError) as e:
        _lib.load_sublibrary("no_such_stem", {})
    msg = str(e.value)
    assert "libfi_no_such_stem.so" in msg and _lib.sublibrary_path("no_such_stem") in msg
    assert "python -m feature_intertwiner_amd.build" in msg and "no CPU/PyTorch fallback" in msg
    with pytest.raises(_lib.FiError):            # nothing was cached for the stem
        _lib.load_sublibrary("no_such_stem", {})


@pytest.mark.parametrize("mod,table,loader,path,stem,entry", MODULES, ids=[m[0] for m in MODULES])
def test_every_module_loads_once_through_the_helper_with_its_signatures_attached(mod, table, loader, path, stem, entry):
    from feature_intertwiner_amd import _lib, build
    build.build_hip()
    m = importlib.import_module("feature_intertwiner_amd." + mod)
    sigs = getattr(m, table)
    assert getattr(m, path) == _lib.sublibrary_path(stem) == build.lib_path(stem)
    L = getattr(m, loader)()
    assert getattr(m, loader)() is L and _lib.load_sublibrary(stem, sigs) is L          # a second load: the same object
    assert os.path.samefile(L._name, getattr(m, path))
    res, args = sigs[entry]
    fn = getattr(L, entry)
    assert fn.restype is res and list(fn.argtypes) == list(args) and len(args) > 0
    for name, (res, args) in sigs.items():
        assert getattr(L, name).restype is res and list(getattr(L, name).argtypes) == list(args), name


def test_the_modules_of_one_library_do_not_share_a_stem():
    assert sorted(m[4] for m in MODULES) == sorted(s for s in STEMS if s != "hip")


# ---- the build table --------------------------------------------------------------------------------------------------
def test_the_table_has_the_fifteen_libraries_and_the_path_names_resolve_to_them():
    from feature_intertwiner_amd import build
    assert list(build.LIBRARIES) == STEMS
    names = ["LIB_PATH"] + [s.upper() + "_LIB_PATH" for s in STEMS[1:]]
    paths = [getattr(build, n) for n in names]
    pkg = os.path.join(ROOT, "feature_intertwiner_amd")
    assert paths == [os.path.join(pkg, "libfi_%s.so" % s) for s in STEMS] == [build.lib_path(s) for s in STEMS]
    assert build.SOURCES is build.LIBRARIES["hip"][0] and build.CSRC == CSRC
    assert build.ROI16_HEADERS is build.LIBRARIES["roi16"][1] and build.HEAD16_HEADERS is build.LIBRARIES["head16"][1]
    sources = [s for srcs, _ in build.LIBRARIES.values() for s in srcs]
    assert len(sources) == len(set(sources))                                     # one object, one library
    assert sorted(sources) == sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))      # and no source left out


def _includes(path):
    return re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), flags=re.M)


def _all_sources():
    from feature_intertwiner_amd import build
    return [(stem, s) for stem, (srcs, _) in build.LIBRARIES.items() for s in srcs]


def test_every_quoted_include_of_a_source_is_among_its_dependencies():
    """... and those of what it includes, down to the last header: a file that is compiled into an object makes it stale."""
    from feature_intertwiner_amd import build
    checked = 0
    for stem, source in _all_sources():
        deps = build.source_deps(stem, source)
        assert deps[0] == os.path.join(CSRC, source) and all(os.path.isabs(d) and os.path.exists(d) for d in deps), source
        todo, seen = [os.path.join(CSRC, source)], set()
        while todo:
            f = todo.pop()
            for inc in _includes(f):
                p = os.path.normpath(os.path.join(os.path.dirname(f), inc))
                assert p.startswith(ROOT + os.sep) and os.path.exists(p), (f, inc)
                assert p in deps, "%s includes %s (through %s): not a dependency of its object" % (source, inc, f)
                checked += 1
                if p not in seen:
                    seen.add(p)
                    todo.append(p)
    assert checked > 60


def test_every_16_bit_twin_depends_on_the_file_it_includes():
    """X_f16.hip is `#define FI_E16_HALF 1` + `#include "X.hip"`: read the include from the twin itself, so that a new twin
    without a rule is caught."""
    from feature_intertwiner_amd import build
    twins = [(stem, s) for stem, s in _all_sources() if s.endswith("_f16.hip")]
    assert len(twins) == 11
    for stem, twin in twins:
        text = open(os.path.join(CSRC, twin)).read()
        hips = [i for i in _includes(os.path.join(CSRC, twin)) if i.endswith(".hip")]
        assert len(hips) == 1 and "FI_E16_HALF" in text, twin
        assert os.path.join(CSRC, hips[0]) in build.source_deps(stem, twin), twin
        if twin != "conv_f16.hip":                                               # the one the naming rule does not cover
            assert hips[0] == twin[:-len("_f16.hip")] + ".hip" and twin not in build.SOURCE_DEPS
    assert build.SOURCE_DEPS["conv_f16.hip"] == ["conv_bf16.hip"]


def test_the_shared_device_headers_are_stated_once_and_reach_their_sources():
    from feature_intertwiner_amd import build
    text = open(os.path.join(ROOT, "feature_intertwiner_amd", "build.py")).read()
    for header in ("crop_dev.h", "conv_act16_dev.h", "sinkhorn_dev.h"):
        assert len(re.findall(r'"%s"' % re.escape(header), text)) == 1, header
    users = {"crop_dev.h": {"crop_and_resize.hip", "crop_roi16.hip", "head16_crop.hip", "heads16.hip"},
             "sinkhorn_dev.h": {"sinkhorn.hip", "sinkhorn_bp.hip"}}
    for header, want in users.items():
        got = {s for stem, s in _all_sources() if header in _includes(os.path.join(CSRC, s))}
        assert got == want, header
        for stem, s in _all_sources():
            if s in want:
                assert os.path.join(CSRC, header) in build.source_deps(stem, s)
    assert not re.search(r'endswith\("[a-z0-9_]+_f16\.hip"\)', text)
