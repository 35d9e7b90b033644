"""GPU: lt_undistort_crop_resize_u8 (csrc/img_prep.hip) against the CPU definition of an undistorted view,
torch.from_numpy(normalize_image(resize_image(undistort_crop_u8(frame, maps, bbox), shape))).float() in CHW, bitwise; against
lt_crop_resize_u8 when there is no distortion; and prepare_batch_frames on undistort_on_the_fly=True deferred items against
prepare_batch on the CPU-prepared items (fixture: tests/golden/h36m_dataset.npz)."""
import os
import pickle

import numpy as np
import pytest
import torch

from gpu_util import record
from mvn.utils import img

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# H36M-like intrinsics and distortion (made-up values of the size of the real calibration); a second camera for a second map
CAMS = [(np.array([[1146.0, 0.0, 508.5], [0.0, 1145.0, 514.0], [0.0, 0.0, 1.0]], np.float32),
         np.array([-0.21, 0.25, -0.0011, -0.0016, -0.0042], np.float32)),
        (np.array([[1150.0, 0.0, 500.0], [0.0, 1148.5, 507.0], [0.0, 0.0, 1.0]], np.float32),
         np.array([-0.19, 0.21, 0.0012, 0.0009, -0.0021], np.float32))]
_maps = {}


def maps_of(cam, hw):
    if (cam, hw) not in _maps:
        _maps[(cam, hw)] = img.undistort_maps(*CAMS[cam], *hw)
    return _maps[(cam, hw)]


def cpu_view(frame, maps, bbox, shape, norm=True):
    r = img.resize_image(img.undistort_crop_u8(frame, maps, tuple(int(x) for x in bbox)), shape)
    if norm:
        return torch.from_numpy(img.normalize_image(r)).float().permute(2, 0, 1)
    return torch.from_numpy(r.astype(np.float32)).permute(2, 0, 1)


def realistic_views(rng, S, n):
    """n views of 1000 x 1000 and 1000 x 1002 frames, two cameras, into S x S: bbox sides 300..900 with the integer factors and the
    identity among them, bboxes at the frame corners (taps leave the frame), partly outside it, and one wholly outside."""
    frames = {hw: [rng.integers(0, 256, hw + (3,), dtype=np.uint8) for _ in range(2)] for hw in ((1000, 1000), (1000, 1002))}
    fixed = [S, 2 * S, 3 * S if 3 * S <= 900 else 2 * S, S, 2 * S]
    views, maps, boxes = [], [], []
    for i in range(n):
        hw = (1000, 1000) if i % 2 == 0 else (1000, 1002)
        f = frames[hw][(i // 2) % 2]
        cam = (i // 3) % 2
        s = fixed[i] if i < len(fixed) else int(rng.integers(max(300, S), 901))
        kind = i % 5
        if kind == 0:                                           # top-left corner, partly outside
            l, u = -int(rng.integers(0, s // 3)), -int(rng.integers(0, s // 3))
        elif kind == 1:                                         # bottom-right corner, partly outside
            l, u = hw[1] - s + int(rng.integers(0, s // 3)), hw[0] - s + int(rng.integers(0, s // 3))
        elif kind == 2 and i % 10 == 2:                         # wholly outside
            l, u = hw[1] + 3, -s - 7
        else:
            l, u = int(rng.integers(-50, hw[1] - s + 50)), int(rng.integers(-50, hw[0] - s + 50))
        views.append(f); maps.append(maps_of(cam, hw)); boxes.append((l, u, l + s, u + s))
    return views, maps, np.array(boxes, np.int64)


@pytest.mark.parametrize("S", [384, 256])
def test_downscale_views_bitwise(S):
    rng = np.random.default_rng(S)
    views, maps, boxes = realistic_views(rng, S, 40)
    modes = {img.area_mode((b[3] - b[1], b[2] - b[0]), (S, S)) for b in boxes}
    assert {"identity", "fast2x2", "area"} <= modes, modes
    if S == 256:
        assert "fast" in modes
    got = img.undistort_crop_resize_normalize(views, maps, boxes, (S, S), device=DEV)
    torch.cuda.synchronize()
    got = got.cpu()
    bad = [i for i in range(len(views)) if not torch.equal(got[i], cpu_view(views[i], maps[i], boxes[i], (S, S)))]
    record("undistort/%d downscale views bitwise mismatches" % S, len(bad))
    assert not bad, bad[:10]
    again = img.undistort_crop_resize_normalize(views, maps, boxes, (S, S), device=DEV)
    assert torch.equal(again.cpu(), got)


def test_upscale_views_within_one_level():
    rng = np.random.default_rng(9)
    S = 384
    f = rng.integers(0, 256, (1000, 1002, 3), dtype=np.uint8)
    m = maps_of(0, (1000, 1002))
    boxes = []
    for i in range(16):
        sh = int(rng.integers(60, S)) if i % 3 != 2 else int(rng.integers(S + 1, 700))
        sw = int(rng.integers(60, S)) if i % 3 != 1 else int(rng.integers(S + 1, 700))
        l, u = int(rng.integers(-sw // 3, 1002 - sw // 2)), int(rng.integers(-sh // 3, 1000 - sh // 2))
        boxes.append((l, u, l + sw, u + sh))
    boxes = np.array(boxes)
    assert all(img.area_mode((b[3] - b[1], b[2] - b[0]), (S, S)) == "linear" for b in boxes)
    got = img.undistort_crop_resize_normalize([f] * 16, [m] * 16, boxes, (S, S), norm_image=False, device=DEV).cpu()
    ref = torch.stack([cpu_view(f, m, b, (S, S), norm=False) for b in boxes])
    d = (got - ref).abs()
    frac = float((d > 0).double().mean())
    record("undistort/upscale max level diff", float(d.max()))
    assert float(d.max()) <= 1.0
    if img.cv2 is None:
        assert frac == 0.0


def test_zero_distortion_equals_crop_resize():
    rng = np.random.default_rng(13)
    frames = [rng.integers(0, 256, (1000, 1002, 3), dtype=np.uint8) for _ in range(3)]
    m = img.undistort_maps(CAMS[0][0], np.zeros(5, np.float32), 1000, 1002)
    boxes = []
    for i in range(24):
        s = int(rng.integers(100, 901))
        l, u = int(rng.integers(-s // 2, 1002 - s // 2)), int(rng.integers(-s // 2, 1000 - s // 2))
        boxes.append((l, u, l + s, u + s + (i % 3) * 7))
    boxes = np.array(boxes)
    views = [frames[i % 3] for i in range(24)]
    for S in (384, 256):
        a = img.undistort_crop_resize_normalize(views, [m] * 24, boxes, (S, S), device=DEV)
        b = img.crop_resize_normalize(views, boxes, (S, S), device=DEV)
        torch.cuda.synchronize()
        assert torch.equal(a, b), S


def test_256_views_one_launch():
    rng = np.random.default_rng(11)
    frames = [rng.integers(0, 256, (1000, 1000, 3), dtype=np.uint8) for _ in range(4)]
    m = [maps_of(0, (1000, 1000)), maps_of(1, (1000, 1000))]
    views, maps, boxes = [], [], []
    for i in range(256):
        s = int(rng.integers(300, 901))
        l, u = int(rng.integers(-50, 1050 - s)), int(rng.integers(-50, 1050 - s))
        views.append(frames[i % 4]); maps.append(m[i % 2]); boxes.append((l, u, l + s, u + s))
    boxes = np.array(boxes)
    out = img.undistort_crop_resize_normalize(views, maps, boxes, (384, 384), device=DEV)
    torch.cuda.synchronize()
    assert out.shape == (256, 3, 384, 384) and torch.isfinite(out).all()
    for i in (0, 101, 255):
        assert torch.equal(out[i].cpu(), cpu_view(views[i], maps[i], boxes[i], (384, 384)))


def test_empty_bbox_is_an_error():
    f = np.zeros((50, 60, 3), np.uint8)
    m = img.undistort_maps(CAMS[0][0] * np.float32(0.05), CAMS[0][1], 50, 60)
    with pytest.raises(RuntimeError, match="empty bbox"):
        img.undistort_crop_resize_normalize([f, f], [m, m], np.array([(0, 0, 50, 50), (10, 10, 10, 30)]), (64, 64), device=DEV)


def _dataset_tree(tmp_path):
    g = np.load(os.path.join(GOLD, "h36m_dataset.npz"))
    labels = pickle.loads(g["labels"].tobytes())
    lp = str(tmp_path / "labels.npy")
    np.save(lp, labels, allow_pickle=True)
    off = g["png_offsets"]
    for i, name in enumerate(g["png_names"]):
        p = tmp_path / str(name)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(g["png_bytes"][off[i]:off[i + 1]].tobytes())
    return str(tmp_path), lp


def test_prepare_batch_frames_undistort_matches_prepare_batch_and_model(tmp_path):
    from mvn.datasets import utils as du
    from mvn.datasets.human36m import Human36MMultiViewDataset
    from mvn.models.triangulation import AlgebraicTriangulationNet
    from oracle import spec, synth
    root, lp = _dataset_tree(tmp_path)
    collate = du.make_collate_fn(randomize_n_views=False)
    for shape in ((256, 256), (24, 20)):
        kw = dict(h36m_root=root, labels_path=lp, image_shape=shape, test=True, scale_bbox=1.5, undistort_images=True,
                  undistort_on_the_fly=True)
        bc = collate([Human36MMultiViewDataset(**kw)[i] for i in range(3)])
        bg = collate([Human36MMultiViewDataset(defer_image_ops=True, **kw)[i] for i in range(3)])
        assert "undistort" in bg
        a = du.prepare_batch(bc, DEV)
        b = du.prepare_batch_frames(bg, DEV, shape)
        torch.cuda.synchronize()
        if img.cv2 is None:
            assert torch.equal(a[0], b[0]), shape
        else:                       # one level after normalisation is at most 1 / (255 * 0.224)
            assert float((a[0] - b[0]).abs().max()) <= 1.0 / (255 * 0.224) + 1e-6
        for x, y in zip(a[1:], b[1:]):
            assert torch.equal(x, y)
    cfg = synth.alg_config(50, True)
    m = AlgebraicTriangulationNet(cfg, device=DEV)
    m.load_state_dict(synth.make_state_dict(spec.alg_net_spec(50, 17, True), seed=50), strict=True)
    m.eval()
    kw = dict(h36m_root=root, labels_path=lp, image_shape=(256, 256), test=True, scale_bbox=1.5, undistort_images=True,
              undistort_on_the_fly=True)
    bc = collate([Human36MMultiViewDataset(**kw)[i] for i in range(2)])
    bg = collate([Human36MMultiViewDataset(defer_image_ops=True, **kw)[i] for i in range(2)])
    a = du.prepare_batch(bc, DEV)
    b = du.prepare_batch_frames(bg, DEV, (256, 256))
    with torch.no_grad():
        ra = m(a[0], a[3], {})
        rb = m(b[0], b[3], {})
    torch.cuda.synchronize()
    if img.cv2 is None:
        for x, y in zip(ra, rb):
            assert torch.equal(x, y)
