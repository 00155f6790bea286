"""CPU: the Sinkhorn term differentiated through its iterations (OptTrans(no_bp_P_L=False), include/fi_ot.h).
  * the module constructs with the flag and keeps the reference's state-dict keys;
  * the reverse recurrence the kernel implements (tests/ot_backprop_ref.py, in the kernel's order) equals float64
    autograd of the non-detached formula of tests/fp64_ref.py to 1e-12 of max|dC|;
  * header, binding table and library exports of libfi_ot.so agree;
  * csrc/sinkhorn_bp.hip compiled for gfx950 has no private segment (no scratch) and a register count that fits the
    wavefronts per SIMD its 1024-thread workgroup needs."""
import os
import re
import subprocess
import tempfile
import types

import pytest
import torch

import ot_backprop_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _cfg():
    return types.SimpleNamespace(DEV=types.SimpleNamespace(OT_ONE_DIM_FORM="conv"))


def test_opttrans_constructs_with_the_differentiable_form():
    from feature_intertwiner_amd.OT_module import OptTrans
    ref = OptTrans(_cfg(), 1024)
    m = OptTrans(_cfg(), 1024, no_bp_P_L=False)
    assert m.no_bp_P_L is False and ref.no_bp_P_L is True
    assert sorted(m.state_dict().keys()) == sorted(ref.state_dict().keys()) == [
        "G_net.0.bias", "G_net.0.weight", "critic.0.bias", "critic.0.weight"]
    m2 = OptTrans(_cfg(), ch_x=32, spatial_x=8, spatial_y=16, no_bp_P_L=False)
    assert m2.two_dim and m2.no_bp_P_L is False


def test_model_reads_the_switch_from_the_config():
    import inspect
    from feature_intertwiner_amd import model
    from feature_intertwiner_amd.OT_module import sinkhorn_loss
    src = inspect.getsource(model)
    assert 'no_bp_P_L=getattr(config.DEV, "OT_NO_BP_P_L", True)' in src
    sig = inspect.signature(sinkhorn_loss)
    assert list(sig.parameters) == ["x", "y", "epsilon_inv", "L", "C_form", "detach_plan"]
    assert sig.parameters["detach_plan"].default is True


@pytest.mark.parametrize("S,D,L,mode", B.CPU_SHAPES)
def test_reverse_recurrence_equals_autograd(S, D, L, mode):
    x, y = B.inputs(S, D)
    C = B.cost(x[0], y[0], mode)
    loss, dC, P = B.recurrence_dcost(C, 1.0, L)
    ref = B.autograd_dcost(C, 1.0, L)
    scale = float(ref.abs().max())
    err = float((dC - ref).abs().max()) / scale
    print("S=%d D=%d L=%d mode=%d: |recurrence - autograd| / max|dC| = %.3g, |dC - P| / max|dC| = %.3g" % (
        S, D, L, mode, err, float((ref - P).abs().max()) / scale))
    assert err <= 1e-12
    if mode == 1 and L > 1:
        assert bool((dC < 0).any())                      # not a plan: the l2 cases have entries of either sign
    from fp64_ref import _ot_plan
    assert torch.equal(P, _ot_plan(C, 1.0, L)) or float((P - _ot_plan(C, 1.0, L)).abs().max()) <= 1e-15
    assert abs(float(loss) - float((P * C).sum())) <= 1e-15


def _declared():
    src = open(os.path.join(ROOT, "include", "fi_ot.h")).read()
    return src, sorted(set(re.findall(r"\b(fi_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))


def test_header_and_binding_table_agree():
    from feature_intertwiner_amd import OT_module
    src, declared = _declared()
    assert declared == sorted(OT_module.OT_SIGNATURES) and len(declared) == 2
    blocks = re.findall(r"/\* -{20,}.*?-{20,} \*/", src, flags=re.S)
    assert len(blocks) == 2 and all("Replaces:" in b and "lib/OT_module.py:104-135" in b for b in blocks)
    # the fifth library adds nothing to libfi_hip.so's interface
    from feature_intertwiner_amd import _lib
    assert not any(k.startswith("fi_ot_") for k in _lib.SIGNATURES)
    assert "fi_ot_" not in open(os.path.join(ROOT, "include", "fi_capi.h")).read()


def test_library_exports_match_the_header():
    from feature_intertwiner_amd import build
    if not os.path.exists(build.OT_LIB_PATH):
        pytest.skip("libfi_ot.so is not built")
    _, declared = _declared()
    nm = subprocess.check_output(["nm", "-D", "--defined-only", build.OT_LIB_PATH], text=True)
    assert sorted(set(re.findall(r" T (fi_[a-z0-9_]+)", nm))) == declared
    assert b"gfx950" in open(build.OT_LIB_PATH, "rb").read()
    needed = subprocess.check_output(["readelf", "-d", build.OT_LIB_PATH], text=True)
    assert "[libfi_hip.so]" in needed and "$ORIGIN" in needed
    assert not re.search(r"(RPATH|RUNPATH).*\[/", needed)                  # no absolute path of the build tree


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_backprop_kernel_has_no_scratch_and_fits_its_wavefronts():
    """Resource metadata of the compiled code object only.  A 1024-thread workgroup is 16 wavefronts on 4 SIMDs: 4 per
    SIMD, which 512 registers per lane allow up to an allocation of 128 (granule 8)."""
    from feature_intertwiner_amd import build
    src = os.path.join(build.CSRC, "sinkhorn_bp.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "bp.s")
        subprocess.check_call([HIPCC] + [f for f in build.FLAGS if f != "-fPIC"] + ["-S", "--cuda-device-only", src, "-o", out])
        text = open(out).read()
    meta = re.findall(r"\.agpr_count:\s+(\d+)(.*?)\.name:\s+(\S*sinkhorn_bp_kernel\S*)(.*?)\.vgpr_spill_count:\s+(\d+)", text, re.S)
    assert len(meta) == 1
    agpr, before, name, after, vspill = meta[0]
    field = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, before + after).group(1))
    assert field("private_segment_fixed_size") == 0, "the kernel uses scratch"
    assert int(vspill) == 0
    threads = field("max_flat_workgroup_size")
    assert threads == 1024
    waves_per_simd = threads // 64 // 4
    alloc = -(-(field("vgpr_count") + int(agpr)) // 8) * 8
    print("sinkhorn_bp_kernel: vgpr %d, agpr %s, LDS %d B, scratch %d" % (
        field("vgpr_count"), agpr, field("group_segment_fixed_size"), field("private_segment_fixed_size")))
    assert 512 // alloc >= waves_per_simd, (alloc, waves_per_simd)
    assert field("group_segment_fixed_size") <= 160 * 1024
