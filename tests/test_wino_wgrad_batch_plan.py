"""The rule that sends a BATCH of weight gradients (fi_conv2d_weight_grad_batch) to the Winograd F(2x2,3x3) form of the
3x3 slot (plan_wgrad in csrc/conv_igemm.hip, WINOGRAD in include/fi_capi.h): the single-problem conditions of
tests/test_wino_wgrad_plan.py plus a floor on the tiles of a problem, fi::WINO_WG_BATCH_MIN_TILES, which is found here
through the query and not written down.  Host-only queries with aligned fake pointers, no GPU;
tests/test_gpu_wino_wgrad_batch.py holds launches at the floor to float64."""
import os

X, DY, DW = 0x10000, 0x40000, 0x20000
ZEROED = 1
N, W = 4, 64                      # the scanned maps: 4 x H x 64, H even: 64 H tiles of 2 x 2 pixels


def _launch(N, Cin, H, W, Cout, flags=ZEROED, n=2, x=X, dy=DY):
    from feature_intertwiner_amd import _lib
    (p,) = _lib.planned_launches(_lib.load().fi_conv2d_weight_grad_launch, x, dy, DW, N, Cin, H, W, Cout, 3, 3, 1, 1, 1, 1, 1,
                                 None, flags, n)
    return p


def _wino(p):
    from feature_intertwiner_amd import _lib
    return bool(p.flags & _lib.LAUNCH_FLAGS["winograd"])


def _with_env(name, fn):
    assert name not in os.environ
    os.environ[name] = "1"
    try:
        return fn()
    finally:
        del os.environ[name]


def floor_height(n=2, Cin=256, Cout=256):
    """The smallest even H at which a batch of n problems on 4 x H x 64 maps plans the Winograd form (None: none to 256)."""
    for H in range(2, 258, 2):
        if _wino(_launch(N, Cin, H, W, Cout, n=n)):
            return H
    return None


def test_the_floor_and_one_tile_row_below_it():
    H = floor_height()
    assert H is not None and H > 2
    tiles = N * (H // 2) * (W // 2)
    # the floor is a tile count, not below 64, and the same for every batch size and for wider layers
    assert tiles >= 64
    for n in (2, 3, 12, 24):
        assert floor_height(n) == H
    assert floor_height(3, 512, 512) == H
    for n in (2, 3, 11, 12):
        p = _launch(N, 256, H, W, 256, n=n)
        assert _wino(p) and p.per_launch == n
        d = _launch(N, 256, H - 2, W, 256, n=n)                    # one tile row of every image less
        assert not _wino(d) and d.per_launch == n
    # the same tiles in another shape of map: 1 image, W = 32
    assert _wino(_launch(1, 256, 2 * tiles // 16, 32, 256, n=2)) and not _wino(_launch(1, 256, 2 * tiles // 16 - 2, 32, 256, n=2))


def test_what_stays_on_the_direct_batch():
    H = floor_height()
    # the pinned small batches (32 tiles a problem)
    for n in (3, 5):
        p = _launch(2, 256, 8, 8, 256, n=n)
        assert p.per_launch == n and not _wino(p)
    # narrower layers, whatever the map
    for shape in ((N, 128, H, W, 256), (N, 128, 4 * H, W, 128), (N, 64, H, W, 64)):
        assert not _wino(_launch(*shape, n=3)), shape
    assert _launch(N, 128, H, W, 256, n=3).per_launch == 3
    # Cout in whole blocks, even H and W, aligned operands: the single-problem conditions
    assert not _wino(_launch(N, 256, H, W, 288, n=3))
    assert not _wino(_launch(N, 256, 4 * H + 1, W, 256, n=3))
    assert _launch(N, 256, H, W, 256, n=3, x=X + 4).per_launch == 1
    # both switches, read per call
    for name in ("FI_NO_WINOGRAD", "FI_NO_WINOGRAD_WGRAD"):
        p = _with_env(name, lambda: _launch(N, 256, H, W, 256, n=3))
        assert not _wino(p) and p.per_launch == 3, name
    assert _wino(_launch(N, 256, H, W, 256, n=3))
    # outputs not zeroed: the entry loops over single launches, each of which is a Winograd launch
    p = _launch(N, 256, H, W, 256, flags=0, n=3)
    assert p.per_launch == 1 and _wino(p)


def test_the_batched_launch_reports_what_the_kernel_does():
    from feature_intertwiner_amd import _lib
    L = _lib.load()
    H = floor_height()
    f = _lib.LAUNCH_FLAGS
    shapes = [(N, 256, H, W, 256), (N, 256, H + 2, W, 256), (N, 512, H, W, 512), (N, 256, 4 * H, W, 320),
              (4, 256, 64, 64, 256), (4, 512, 32, 32, 512)]                # ... and the step's C4 and C5 blocks
    for shape in shapes:
        n_, Cin, h, w, Cout = shape
        tiles = n_ * (h // 2) * (w // 2)
        for n in (2, 3, 11, 12, 24):
            p = _launch(*shape, n=n)
            if not _wino(p):                                           # (C5 may be under the floor)
                assert tiles < N * (H // 2) * (W // 2)
                continue
            d = _with_env("FI_NO_WINOGRAD_WGRAD", lambda: _launch(*shape, n=n))
            assert p.kernel_id == d.kernel_id and d.per_launch == n == p.per_launch
            assert _lib.KERNEL_KEYS[p.kernel_id] in ("conv_wgrad_bm64_3x3", "conv_wgrad_bm128_3x3")
            assert p.flags == f["tap_major"] | f["swizzled"] | f["winograd"]
            assert _lib.WGRAD_FORMS[p.form] == "VEC" and p.window == 1 and p.tile_rows == 64
            assert (p.grid_x, p.grid_y, p.grid_z) == (Cin // 64, Cout // 64, p.splits)
            blocks = p.grid_x * p.grid_y
            workgroups = n * blocks * p.splits                          # (problem, split, block)
            assert workgroups == p.per_launch * p.grid_x * p.grid_y * p.grid_z
            # whole stages of 4 tiles, no split under 32 tiles, every split but the last full, the last not empty
            assert p.pixels_per_split % 16 == 0 and p.pixels == n_ * h * w
            tps = p.pixels_per_split // 4
            assert tps % 4 == 0 and (p.splits == 1 or tps >= 32)
            assert (p.splits - 1) * tps < tiles <= p.splits * tps
            # a problem of a batch never has more splits than it has alone
            assert p.splits <= _launch(*shape, n=1).splits
            a = (X, DY, DW, n_, Cin, h, w, Cout, 3, 3, 1, 1, 1, 1, 1, None, ZEROED, n)
            assert _lib.wgrad_plan(L.fi_conv2d_weight_grad_split_plan, *a) == (p.splits, p.pixels_per_split)
            assert _lib.wgrad_plan(L.fi_conv2d_weight_grad_plan, *a) == (p.kernel_id, n)
