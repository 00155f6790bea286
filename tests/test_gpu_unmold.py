"""GPU: the inference unmolding kernels (csrc/unmold.hip, feature_intertwiner_amd/postprocess.py) are bit-exact
against the golden made from the reference's own `_unmold_detections` and maskApi.c (tests/golden/unmold.npz), and
`workflow.test_step` after a real inference forward equals the NumPy restatement fed the same tensors."""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch

import unmold_ref as R
from unmold_cases import unmold_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = {c[0]: c for c in unmold_cases()}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "unmold.npz"))


def _split(flat, lens):
    return np.split(flat, np.cumsum(lens)[:-1]) if len(lens) else []


def _run(case, **kw):
    from feature_intertwiner_amd.postprocess import unmold_detections
    name, det, masks, hw, win = CASES[case]
    out = unmold_detections(torch.from_numpy(det).to(DEV), torch.from_numpy(masks).to(DEV), hw,
                            torch.from_numpy(win).to(DEV), **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_unmold_bit_exact_vs_golden(golden, case):
    out = _run(case, rle=True, dense=True)
    hw = CASES[case][3]
    for b, img in enumerate(out):
        k = "%s/%d/" % (case, b)
        H, W = (int(v) for v in hw[b])
        assert np.array_equal(img["boxes"].cpu().numpy(), golden[k + "boxes"])
        assert np.array_equal(img["class_ids"].cpu().numpy(), golden[k + "class_ids"])
        assert np.array_equal(img["scores"].cpu().numpy().view(np.uint32), golden[k + "scores"].view(np.uint32))
        n = golden[k + "boxes"].shape[0]
        cnts = _split(golden[k + "counts"], golden[k + "rle_len"])
        strs = _split(golden[k + "strings"], golden[k + "str_len"])
        assert len(img["rle"]) == len(img["rle_counts"]) == n
        masks = img["masks"]
        assert tuple(masks.shape) == (H, W, n)
        dense = masks.permute(2, 0, 1).contiguous().cpu().numpy()
        assert hashlib.sha256(dense.tobytes()).hexdigest() == str(golden[k + "dense_sha256"])
        if k + "dense" in golden:
            assert np.array_equal(np.packbits(dense, axis=-1), golden[k + "dense"])
        for j in range(n):
            assert np.array_equal(img["rle_counts"][j], cnts[j]), (case, b, j)
            assert img["rle"][j] == {"size": [H, W], "counts": strs[j].tobytes()}, (case, b, j)
            assert np.array_equal(R.rle_decode(img["rle_counts"][j], (H, W)), dense[j])


def test_rle_without_dense_and_dense_without_rle(golden):
    a = _run("mixed", rle=True, dense=False)
    b = _run("mixed", rle=False, dense=True)
    for x, y in zip(a, b):
        assert "masks" not in x and "rle" not in y
        assert torch.equal(x["boxes"], y["boxes"])
        for j, c in enumerate(x["rle_counts"]):
            assert np.array_equal(R.rle_decode(c, x["image_shape"]), y["masks"][:, :, j].cpu().numpy())


def test_raw_c_entry_points(golden):
    """fi_unmold_prepare / _encode / _paste called directly, with the device scan of the sizes."""
    from feature_intertwiner_amd import _lib, postprocess
    L = postprocess.load()
    name, det, masks, hw, win = CASES["mixed"]
    bs, D, K, mh, mw = masks.shape
    d, m, w = (torch.from_numpy(a).to(DEV) for a in (det, masks, win))
    hw_d = torch.from_numpy(hw).to(DEV)
    hw_h = np.ascontiguousarray(hw, np.int32)
    hp = hw_h.ctypes.data_as(ctypes.c_void_p)
    boxes = torch.full((bs * D, 4), -7, dtype=torch.int32, device=DEV)
    cls = torch.empty(bs * D, dtype=torch.int32, device=DEV)
    sc = torch.empty(bs * D, dtype=torch.float32, device=DEV)
    nv = torch.empty(bs, dtype=torch.int32, device=DEV)
    sizes = torch.empty(bs * D, 2, dtype=torch.int64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = torch.empty(L.fi_unmold_workspace_bytes(bs, D, mh, mw), dtype=torch.uint8, device=DEV)
    P = _lib.ptr
    st = _lib.current_stream()
    assert L.fi_unmold_prepare(P(d), P(m), P(hw_d), hp, P(w), bs, D, K, mh, mw, P(boxes), P(cls), P(sc), P(nv),
                               P(sizes), P(status), P(ws), st) == 0
    offsets = sizes.cumsum(0) - sizes
    n = nv.cpu().numpy()
    sz = sizes.cpu().numpy()
    assert int(status.item()) == 0
    for b in range(bs):
        k = "%s/%d/" % (name, b)
        assert n[b] == golden[k + "boxes"].shape[0]
        assert np.array_equal(sz[b * D:b * D + n[b], 0], golden[k + "rle_len"])
        assert np.array_equal(sz[b * D:b * D + n[b], 1], golden[k + "str_len"])
        assert not sz[b * D + n[b]:(b + 1) * D].any()
        assert (boxes.view(bs, D, 4)[b, n[b]:] == -7).all()           # unused slots are not written
    counts = torch.zeros(int(sz[:, 0].sum()), dtype=torch.int32, device=DEV)
    strings = torch.zeros(int(sz[:, 1].sum()), dtype=torch.uint8, device=DEV)
    assert L.fi_unmold_encode(P(hw_d), hp, P(boxes), P(nv), bs, D, mh, mw, P(ws), P(offsets), P(counts), P(strings),
                              st) == 0
    exp_c = np.concatenate([golden["mixed/%d/counts" % b] for b in range(bs)])
    exp_s = np.concatenate([golden["mixed/%d/strings" % b] for b in range(bs)])
    assert np.array_equal(counts.cpu().numpy().view(np.uint32), exp_c)
    assert np.array_equal(strings.cpu().numpy(), exp_s)
    total = int((n.astype(np.int64) * hw[:, 0] * hw[:, 1]).sum())
    dense = torch.full((total + 16,), 0xAB, dtype=torch.uint8, device=DEV)
    assert L.fi_unmold_paste(P(hw_d), hp, P(boxes), P(nv), bs, D, mh, mw, P(ws), total, P(dense), st) == 0
    host = dense.cpu().numpy()
    assert (host[total:] == 0xAB).all()                                 # nothing past total_bytes
    exp = b"".join(bytes(np.unpackbits(golden["mixed/%d/dense" % b], axis=-1)[..., :hw[b, 1]].tobytes())
                   for b in range(bs))
    assert host[:total].tobytes() == exp


def test_coco_results_equal_golden_dicts(golden):
    from feature_intertwiner_amd.postprocess import coco_results
    out = _run("mixed")
    cmap = list(range(100, 200))
    got = coco_results(out, [11, 22], cmap)
    exp = []
    for b, image_id in enumerate([11, 22]):
        k = "mixed/%d/" % b
        H, W = (int(v) for v in CASES["mixed"][3][b])
        strs = _split(golden[k + "strings"], golden[k + "str_len"])
        exp += R.coco_results(image_id, golden[k + "boxes"], golden[k + "class_ids"], golden[k + "scores"],
                              [{"size": [H, W], "counts": s.tobytes()} for s in strs], cmap)
    assert len(got) == len(exp) > 0
    for g, e in zip(got, exp):
        assert g.keys() == e.keys()
        assert g["score"].dtype == np.float32 and g["score"].view(np.uint32) == e["score"].view(np.uint32)
        assert all(g[key] == e[key] for key in ("image_id", "category_id", "bbox", "segmentation"))
    got_fn = coco_results(out, [11, 22], lambda c: c + 100)
    assert [r["category_id"] for r in got_fn] == [r["category_id"] for r in got]


def test_test_step_after_inference_equals_restatement():
    """The synthetic inference of test_gpu_detector.py::test_inference_path_runs, then workflow.test_step."""
    from feature_intertwiner_amd import workflow
    from feature_intertwiner_amd.config import make_config
    from feature_intertwiner_amd.model import MaskRCNN
    from feature_intertwiner_amd.synthetic import SyntheticProposals, synthetic_batch
    torch.manual_seed(1)
    cfg = make_config("resnet50", 256, 2)
    model = MaskRCNN(cfg).to(DEV)
    batch = synthetic_batch(2, 256, device=DEV)
    model.external_proposals = SyntheticProposals(batch[2], 256)
    K = cfg.DATASET.NUM_CLASSES
    meta = np.zeros((2, 8 + K + 1), np.float32)
    meta[:, 0] = [0, 1]
    meta[:, 1:4] = [[240, 240, 3], [300, 280, 3]]
    meta[:, 4:8] = [[0, 0, 256, 256], [0, 16, 256, 240]]
    meta[:, -1] = [501, 502]

    seen = {}

    def recording_model(inputs, mode):
        seen["out"] = model(inputs, mode=mode)
        return seen["out"]

    results, unmolded = workflow.test_step(recording_model, batch[0], torch.from_numpy(meta),
                                           category_map=lambda c: 7 * c, dense=True)
    det, masks = (t.cpu().numpy() for t in seen["out"])
    total = 0
    for b in range(2):
        H, W = int(meta[b, 1]), int(meta[b, 2])
        boxes, cls, scores, full, _ = R.unmold_detections(det[b], masks[b], (H, W), meta[b, 4:8])
        img = unmolded[b]
        assert boxes.shape[0] > 0
        assert np.array_equal(img["boxes"].cpu().numpy(), boxes)
        assert np.array_equal(img["class_ids"].cpu().numpy(), cls)
        assert np.array_equal(img["scores"].cpu().numpy(), scores)
        assert np.array_equal(img["masks"].permute(2, 0, 1).cpu().numpy(), full)
        for j in range(boxes.shape[0]):
            c = R.rle_counts(full[j])
            assert np.array_equal(img["rle_counts"][j], c)
            assert img["rle"][j]["counts"] == R.rle_string(c)
        exp = R.coco_results(int(meta[b, -1]), boxes, cls, scores, img["rle"], lambda c: 7 * c)
        for g, e in zip(results[total:total + len(exp)], exp):
            assert g["image_id"] == e["image_id"] and g["category_id"] == e["category_id"]
            assert g["bbox"] == e["bbox"] and g["score"] == e["score"] and g["segmentation"] == e["segmentation"]
        total += len(exp)
    assert len(results) == total


def test_bad_inputs_return_a_status():
    from feature_intertwiner_amd import _lib
    from feature_intertwiner_amd.postprocess import unmold_detections
    det = torch.zeros(1, 4, 6, device=DEV)
    det[0, 0] = torch.tensor([1, 1, 9, 9, 3, 0.9])
    masks = torch.rand(1, 4, 3, 28, 28, device=DEV)
    win = torch.tensor([[0.0, 0.0, 10.0, 10.0]], device=DEV)
    with pytest.raises(_lib.FiError, match="outside"):
        unmold_detections(det, masks, [[10, 10]], win)                        # class 3 with K = 3
    with pytest.raises(_lib.FiError, match="window"):
        unmold_detections(det, torch.rand(1, 4, 4, 28, 28, device=DEV), [[10, 10]], torch.zeros(1, 4, device=DEV))
    with pytest.raises(_lib.FiError, match="4096"):
        unmold_detections(det, masks, [[5000, 10]], win)
    with pytest.raises(_lib.FiError, match="1..64"):
        unmold_detections(det, torch.rand(1, 4, 4, 65, 28, device=DEV), [[10, 10]], win)
    # the device is still fine afterwards
    out = unmold_detections(det, torch.rand(1, 4, 4, 28, 28, device=DEV), [[10, 10]], win, dense=True)
    torch.cuda.synchronize()
    assert out[0]["boxes"].shape == (1, 4)
