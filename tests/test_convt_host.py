"""CPU: libfi_convt.so (the transposed 3x3 / stride 2 convolution, include/fi_convt.h) builds for gfx950, exports exactly
what its header declares, validates its arguments on the host before any HIP call, and the models hold
conv.ConvTranspose3x3 with the state-dict keys and shapes of the stock nn.ConvTranspose2d.  No kernel is launched here."""
import os
import re
import subprocess

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "fi_convt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fi_[a-z0-9_]+)\s*\(", src)))


def test_library_builds_and_exports_every_declared_symbol():
    from feature_intertwiner_amd import build
    build.build_hip()
    path = build.CONVT_LIB_PATH
    assert os.path.exists(path)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    exported = set(re.findall(r" T (fi_[a-z0-9_]+)", nm))
    declared = _declared()
    assert declared == ["fi_conv_transpose3x3s2_eligible", "fi_conv_transpose3x3s2_forward"]
    assert exported == set(declared), (sorted(exported), declared)
    assert b"gfx950" in open(path, "rb").read()


def test_ctypes_table_matches_the_header():
    from feature_intertwiner_amd import conv
    assert sorted(conv.CONVT_SIGNATURES.keys()) == _declared()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fi_convt.h")).read(), flags=re.S)
    for name, (res, args) in conv.CONVT_SIGNATURES.items():
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1).split(",")
        assert len(params) == len(args), name
        for p, a in zip(params, args):
            is_ptr = "*" in p or "fi_stream_t" in p
            assert (a is conv.ctypes.c_void_p) == is_ptr, (name, p.strip())
    L = conv.load_convt()
    assert L.fi_conv_transpose3x3s2_eligible.restype is conv.ctypes.c_int


def test_eligibility_query():
    from feature_intertwiner_amd.conv import load_convt
    el = load_convt().fi_conv_transpose3x3s2_eligible
    #          N, Cin,  H,   W, Cout, nhwc, x, y
    assert el(4, 256, 256, 256, 256, 1, 64, 128) == 1        # the make-up layer on P2 of the headline image
    assert el(1, 16, 1, 1, 1, 0, None, None) == 1            # smallest: any Cout, H, W >= 1
    assert el(2, 32, 5, 7, 24, 0, 4, 16) == 1                # x only needs its 4 bytes
    assert el(2, 12, 6, 5, 20, 0, None, None) == 0           # Cin % 16
    assert el(2, 0, 6, 5, 20, 0, None, None) == 0
    assert el(2, 16, 6, 5, 20, 0, None, 8) == 0              # y not 16-byte aligned
    assert el(2, 16, 6, 5, 20, 0, 2, 16) == 0                # x not a float address
    assert el(2, 16, 6, 5, 22, 1, None, None) == 0           # channels-last needs Cout % 4 == 0
    assert el(2, 16, 6, 5, 22, 0, None, None) == 1
    assert el(0, 16, 6, 5, 20, 0, None, None) == 0 and el(2, 16, 0, 5, 20, 0, None, None) == 0
    assert el(1, 16, 1 << 14, 1 << 13, 8, 0, None, None) == 0     # 16 channels of an image no longer index with an int


def test_argument_validation_without_a_gpu():
    """Invalid calls are rejected on the host before any HIP call."""
    from feature_intertwiner_amd import _lib
    from feature_intertwiner_amd.conv import load_convt
    fwd = load_convt().fi_conv_transpose3x3s2_forward
    last = _lib.load().fi_last_error
    #   x, w, bias, scale, y, N, Cin, H, W, Cout, relu, nhwc, stream
    assert fwd(None, 64, None, None, 128, 1, 16, 4, 4, 8, 0, 0, None) == -1 and b"null" in last()
    assert fwd(64, None, None, None, 128, 1, 16, 4, 4, 8, 0, 0, None) == -1
    assert fwd(64, 64, None, None, None, 1, 16, 4, 4, 8, 0, 0, None) == -1
    assert fwd(64, 64, None, None, 128, 1, 16, 0, 4, 8, 0, 0, None) == -1          # H < 1
    assert fwd(64, 64, None, None, 128, -1, 16, 4, 4, 8, 0, 0, None) == -1
    assert fwd(64, 64, None, None, 128, 1, 16, 4, 4, 8, 0, 2, None) == -1          # out_nhwc outside {0, 1}
    assert fwd(64, 64, None, None, 128, 1, 12, 4, 4, 8, 0, 0, None) == -3 and b"Cin % 16" in last()
    assert fwd(64, 64, None, None, 136, 1, 16, 4, 4, 8, 0, 0, None) == -3          # misaligned y
    assert fwd(64, 64, None, None, 128, 1, 16, 4, 4, 6, 0, 1, None) == -3          # channels-last, Cout % 4
    assert fwd(None, None, None, None, None, 0, 16, 4, 4, 8, 0, 0, None) == 0      # empty batch: nothing to launch


def _same_keys_and_shapes(ours, stock):
    a, b = ours.state_dict(), stock.state_dict()
    assert list(a.keys()) == list(b.keys())
    assert [tuple(v.shape) for v in a.values()] == [tuple(v.shape) for v in b.values()]


def test_models_hold_the_module_with_the_stock_state_dict():
    from feature_intertwiner_amd.OT_module import OptTrans
    from feature_intertwiner_amd.config import make_config
    from feature_intertwiner_amd.conv import ConvTranspose3x3
    from feature_intertwiner_amd.sub_module import Dev
    cfg = make_config(backbone="resnet50", image_size=256, batch_size=2, train_rois_per_image=48)
    cfg.DEV.UPSAMPLE_FAC = 2.0
    dev = Dev(cfg, 256)
    up = dev.upsample[0][0]
    assert type(up) is ConvTranspose3x3 and up.geometry() == 2
    _same_keys_and_shapes(up, nn.ConvTranspose2d(256, 256, kernel_size=3, stride=2, padding=1, output_padding=1))
    for spatial_y, stride in ((16, 2), (8, 1)):
        ot = OptTrans(cfg, 32, spatial_x=8, ch_y=48, spatial_y=spatial_y)
        g = ot.G_net[0]
        assert type(g) is ConvTranspose3x3 and g.geometry() == stride
        stock = nn.ConvTranspose2d(32, 48, kernel_size=3, padding=1, stride=stride, output_padding=stride - 1)
        _same_keys_and_shapes(g, stock)
        assert [k for k in ot.state_dict() if k.startswith("G_net.0.")] == ["G_net.0.weight", "G_net.0.bias"]


def test_stock_state_dict_loads_and_cpu_forward_is_the_stock_one():
    from feature_intertwiner_amd.conv import ConvTranspose3x3
    torch.manual_seed(0)
    stock = nn.ConvTranspose2d(16, 24, kernel_size=3, stride=2, padding=1, output_padding=1)
    ours = ConvTranspose3x3(16, 24, kernel_size=3, stride=2, padding=1, output_padding=1)
    ours.load_state_dict(stock.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(ours.state_dict().values(), stock.state_dict().values()))
    x = torch.randn(2, 16, 5, 7)
    assert torch.equal(ours(x), stock(x))              # not on the GPU: super().forward, as Conv1d does
    import pytest
    with pytest.raises(NotImplementedError):
        ConvTranspose3x3(16, 24, kernel_size=3, stride=2, padding=1, output_padding=0).geometry()
    with pytest.raises(NotImplementedError):
        ConvTranspose3x3(16, 24, kernel_size=3, stride=1, padding=0).geometry()
