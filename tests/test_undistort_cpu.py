"""CPU: on-the-fly lens undistortion (mvn/utils/img.py: undistort_maps, cubic_tab, remap_cubic_u8, undistort_crop_u8,
source_window) against independent fp64 evaluations, the dataset's undistort_on_the_fly items against the undistort_images=True
file path, and the argument checks of lt_undistort_crop_resize_u8 (no device work)."""
import ctypes
import os
import pickle

import numpy as np
import pytest
from PIL import Image

import lt_hip as H
from mvn.datasets import utils as du
from mvn.datasets.human36m import Human36MMultiViewDataset
from mvn.utils import img

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# H36M-like intrinsics and distortion for a 1000 x 1000 frame (made-up values of the same size as the real calibration)
K_H36M = np.array([[1146.0, 0.0, 508.5], [0.0, 1145.0, 514.0], [0.0, 0.0, 1.0]], np.float32)
DIST_H36M = np.array([-0.21, 0.25, -0.0011, -0.0016, -0.0042], np.float32)


def grid_fp64(K, dist, h, w):
    """The reference script's distortion model (undistort-h36m.py:56-73) in float64.  Its tangential terms are p1*x*y + p2*(x^2 + r^2)
    for x and p2*x*y + p1*(y^2 + r^2) for y (the script's own expressions, which the undistorted files were made with)."""
    K, d = np.asarray(K, np.float64), np.asarray(dist, np.float64)
    k1, k2, p1, p2, k3 = d
    x, y = np.meshgrid((np.arange(w) - K[0, 2]) / K[0, 0], (np.arange(h) - K[1, 2]) / K[1, 1])
    r2 = x * x + y * y
    rad = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    xd = x * rad + p1 * x * y + p2 * (x * x + r2)
    yd = y * rad + p2 * x * y + p1 * (y * y + r2)
    return np.stack([xd * K[0, 0] + K[0, 2], yd * K[1, 1] + K[1, 2]], axis=2)


def keys(t, A=-0.75):
    t = np.abs(t)
    return np.where(t <= 1, ((A + 2) * t - (A + 3)) * t * t + 1, np.where(t < 2, ((A * t - 5 * A) * t + 8 * A) * t - 4 * A, 0.0))


def coords(maps):
    map1, map2 = maps
    m2 = map2.astype(np.int64)
    return map1[..., 0] + (m2 & 31) / 32.0, map1[..., 1] + (m2 >> 5) / 32.0


def test_maps_quantise_the_reference_model():
    for K, d, (h, w) in ((K_H36M, DIST_H36M, (1000, 1000)), (K_H36M, DIST_H36M, (1000, 1002)), (K_H36M, -2 * DIST_H36M, (300, 500))):
        map1, map2 = img.undistort_maps(K, d, h, w)
        assert map1.dtype == np.int16 and map1.shape == (h, w, 2) and map2.dtype == np.uint16 and map2.shape == (h, w)
        assert int(map2.max()) < 1024
        ref = grid_fp64(K, d, h, w)
        x, y = coords((map1, map2))
        err = max(np.abs(x - ref[..., 0]).max(), np.abs(y - ref[..., 1]).max())
        assert err <= 1 / 64 + 2e-3, err
        assert 0.3 < np.abs(ref[..., 0] - np.arange(w)[None, :]).max()          # the distortion is not negligible
    # no distortion: exactly the integer grid
    map1, map2 = img.undistort_maps(K_H36M, np.zeros(5, np.float32), 1000, 1002)
    assert (map2 == 0).all()
    assert np.array_equal(map1[..., 0], np.broadcast_to(np.arange(1002), (1000, 1002)))
    assert np.array_equal(map1[..., 1], np.broadcast_to(np.arange(1000)[:, None], (1000, 1002)))


def test_maps_follow_the_reference_float32_expressions():
    """distortion_grid is the reference script's expressions verbatim in float32; the quantisation is rint(32 x) (half to even)."""
    grid = img.distortion_grid(K_H36M, DIST_H36M, 40, 50)
    assert grid.dtype == np.float32
    map1, map2 = img.undistort_maps(K_H36M, DIST_H36M, 40, 50)
    ix, iy = np.rint(grid[..., 0] * 32).astype(np.int64), np.rint(grid[..., 1] * 32).astype(np.int64)
    assert np.array_equal(map1[..., 0], ix >> 5) and np.array_equal(map1[..., 1], iy >> 5)
    assert np.array_equal(map2, (iy & 31) * 32 + (ix & 31))


def test_cubic_table():
    t = img.cubic_tab().astype(np.int64)
    assert t.shape == (1024, 16) and (t.sum(1) == 32768).all()
    f = np.arange(32) / 32.0
    w1 = np.stack([keys(f + 1), keys(f), keys(1 - f), keys(2 - f)], 1)             # taps x - 1 .. x + 2 for fraction f
    w = np.einsum("ik,jl->ijkl", w1, w1).reshape(1024, 16)                         # row i: y fraction, column j: x fraction
    d = np.abs(t - np.round(32768 * w))
    # every weight is within one step of the exact one, except the one entry per block that OpenCV's sum correction moves (it
    # lies in the block's lower-right 2 x 2, entries 10, 11, 14, 15, and absorbs the rounding of the other 15)
    assert (d > 1).sum(1).max() <= 1
    assert set(np.nonzero(d > 1)[1]) <= {10, 11, 14, 15}
    assert d.max() <= 8


def remap_fp64(src, maps):
    """Keys bicubic (A = -0.75) at the quantised coordinates in float64, taps outside the frame 0, rounded and saturated."""
    h, w = src.shape[:2]
    x, y = coords(maps)
    xi, yi = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    acc = np.zeros(x.shape + (3,))
    for a in range(-1, 3):
        for b in range(-1, 3):
            yy, xx = yi + a, xi + b
            ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            px = src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)] * ok[..., None]
            acc += px * (keys(y - yy) * keys(x - xx))[..., None]
    return np.clip(np.rint(acc), 0, 255)


def small_camera(h, w, scale=1.0):
    K = K_H36M.copy()
    K[0, 0] *= w / 1000.0; K[1, 1] *= h / 1000.0; K[0, 2] *= w / 1000.0; K[1, 2] *= h / 1000.0
    return K, (DIST_H36M * scale).astype(np.float32)


def test_remap_cubic_against_fp64_and_identity():
    rng = np.random.default_rng(0)
    h, w = 90, 120
    src = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    for scale in (1.0, 3.0, -4.0):                       # strong distortion: taps leave the frame along the border
        maps = img.undistort_maps(*small_camera(h, w, scale), h, w)
        got = img.remap_cubic_u8(src, *maps)
        assert got.shape == (h, w, 3) and got.dtype == np.uint8
        assert np.abs(got.astype(np.int64) - remap_fp64(src, maps)).max() <= 1
        # a sub-rectangle is that rectangle of the whole remap
        assert np.array_equal(img.remap_cubic_u8(src, *maps, slice(10, 47), slice(3, 90)), got[10:47, 3:90])
    # map coordinates wholly outside the frame read the constant border
    map1 = np.full((4, 5, 2), -10, np.int16); map2 = np.zeros((4, 5), np.uint16)
    assert (img.remap_cubic_u8(src, map1, map2) == 0).all()
    # no distortion: the input, bitwise
    maps = img.undistort_maps(K_H36M, np.zeros(5, np.float32), h, w)
    assert np.array_equal(img.remap_cubic_u8(src, *maps), src)
    full = rng.integers(0, 256, (1000, 1002, 3), dtype=np.uint8)
    maps = img.undistort_maps(K_H36M, np.zeros(5, np.float32), 1000, 1002)
    assert np.array_equal(img.undistort_crop_u8(full, maps, (-20, 950, 300, 1040)), img.crop_image(full, (-20, 950, 300, 1040)))


def test_undistort_crop_is_crop_of_the_remap():
    rng = np.random.default_rng(1)
    h, w = 80, 110
    src = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    maps = img.undistort_maps(*small_camera(h, w, 2.0), h, w)
    whole = img.remap_cubic_u8(src, *maps)
    for bbox in ((10, 5, 60, 70), (-15, -8, 40, 30), (90, 60, 140, 100), (-30, -30, 150, 120), (200, 10, 240, 40), (0, 0, w, h),
                 (-50, 90, -10, 130)):
        got = img.undistort_crop_u8(src, maps, bbox)
        assert np.array_equal(got, img.crop_image(whole, bbox)), bbox


def test_source_window():
    rng = np.random.default_rng(2)
    h, w = 1000, 1002
    frame = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    maps = img.undistort_maps(K_H36M, DIST_H36M, h, w)
    assert img.map_is_monotone(maps[0])
    for bbox in ((100, 120, 700, 720), (-80, -60, 420, 440), (600, 650, 1150, 1200), (0, 0, w, h), (1100, 0, 1300, 200)):
        per = img.source_window(maps[0], bbox, (h, w))
        full = img.source_window(maps[0], bbox, (h, w), monotone=False)
        assert per == full, bbox
        x0, y0, x1, y1 = per
        if x1 == 0:
            assert img._clip_box(bbox, (h, w))[2] == img._clip_box(bbox, (h, w))[0]
            continue
        assert 0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h
        # every tap of bbox & frame that lies inside the frame lies inside the window: zeroing the rest changes nothing
        cut = np.zeros_like(frame)
        cut[y0:y1, x0:x1] = frame[y0:y1, x0:x1]
        assert np.array_equal(img.undistort_crop_u8(cut, maps, bbox), img.undistort_crop_u8(frame, maps, bbox)), bbox
    # a map that is not monotone takes the full-slice bound
    map1 = np.zeros((40, 50, 2), np.int16)
    map1[..., 0] = np.arange(50)[None, :]
    map1[..., 1] = np.arange(40)[:, None]
    map1[20, 25] = (45, 2)                                    # an inner pixel that reads far away
    assert not img.map_is_monotone(map1)
    assert img.source_window(map1, (10, 10, 30, 30), (40, 50)) == (9, 1, 48, 32)
    assert img.source_window(map1, (10, 10, 30, 30), (40, 50), monotone=False) == (9, 1, 48, 32)
    assert img.source_window(map1, (10, 10, 30, 30), (40, 50), monotone=True) == (9, 9, 32, 32)     # what the perimeter alone sees


def _tree(tmp_path):
    g = np.load(os.path.join(GOLD, "h36m_dataset.npz"))
    labels = pickle.loads(g["labels"].tobytes())
    lp = str(tmp_path / "labels.npy")
    np.save(lp, labels, allow_pickle=True)
    off = g["png_offsets"]
    for i, name in enumerate(g["png_names"]):
        p = tmp_path / str(name)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(g["png_bytes"][off[i]:off[i + 1]].tobytes())
    return str(tmp_path), lp, labels, [str(n) for n in g["png_names"]]


def test_dataset_undistort_on_the_fly(tmp_path):
    from mvn.datasets.human36m import imread_bgr
    root, lp, labels, names = _tree(tmp_path)
    # the offline pass's output, losslessly stored: the remap of every raw frame with its camera's maps
    cams = labels["cameras"]
    for name in names:
        subject, action, _, camera_name, fn = name.split("/")
        s, c = labels["subject_names"].index(subject), labels["camera_names"].index(camera_name)
        raw = imread_bgr(os.path.join(root, name))
        und = img.remap_cubic_u8(raw, *img.undistort_maps(cams[s, c]["K"], cams[s, c]["dist"], *raw.shape[:2]))
        out = os.path.join(root, subject, action, "imageSequence-undistorted", camera_name, fn)
        os.makedirs(os.path.dirname(out), exist_ok=True)
        Image.fromarray(np.ascontiguousarray(und[:, :, ::-1])).save(out, format="PNG")
    with pytest.raises(ValueError):
        Human36MMultiViewDataset(h36m_root=root, labels_path=lp, test=True, undistort_on_the_fly=True)
    for shape in ((64, 64), (24, 20)):
        kw = dict(h36m_root=root, labels_path=lp, image_shape=shape, test=True, scale_bbox=1.5, undistort_images=True)
        files, fly = Human36MMultiViewDataset(**kw), Human36MMultiViewDataset(undistort_on_the_fly=True, **kw)
        dfr = Human36MMultiViewDataset(undistort_on_the_fly=True, defer_image_ops=True, **kw)
        plain = Human36MMultiViewDataset(**dict(kw, undistort_images=False))
        for idx in range(3):
            a, b, d, p = files[idx], fly[idx], dfr[idx], plain[idx]
            assert len(a["images"]) == len(b["images"]) == len(d["frames"]) == len(d["undistort"])
            for ia, ib in zip(a["images"], b["images"]):
                assert ia.dtype == ib.dtype and np.array_equal(ia, ib)
            assert any(not np.array_equal(ib, ip) for ib, ip in zip(b["images"], p["images"]))    # the distortion is visible
            # crop -> resize -> normalise of the undistorted frame
            for v, (f, bb, (K, dist, hw)) in enumerate(zip(d["frames"], d["bboxes"], d["undistort"])):
                assert K.dtype == np.float32 and dist.dtype == np.float32 and hw == f.shape[:2]
                want = img.normalize_image(img.resize_image(img.crop_image(img.remap_cubic_u8(f, *img.undistort_maps(K, dist, *hw)), bb), shape))
                assert np.array_equal(b["images"][v], want)
            for x in (b, d):
                assert [tuple(s) for s in a["image_shapes_before_resize"]] == [tuple(s) for s in x["image_shapes_before_resize"]]
                for ca, cb in zip(a["cameras"], x["cameras"]):
                    for attr in ("K", "R", "t", "dist"):
                        assert np.array_equal(getattr(ca, attr), getattr(cb, attr))
                for pa, pb in zip(a["proj_matrices"], x["proj_matrices"]):
                    assert np.array_equal(pa, pb)
                assert a["detections"] == x["detections"]
                assert np.array_equal(a["keypoints_3d"], x["keypoints_3d"]) and a["indexes"] == x["indexes"]
    collate = du.make_collate_fn(randomize_n_views=False)
    bd = collate([dfr[i] for i in range(3)])
    nv = len(bd["frames"])
    assert len(bd["undistort"]) == nv and all(len(u) == 3 for u in bd["undistort"])
    assert bd["undistort"][1][2] is dfr[2]["undistort"][1] or bd["undistort"][1][2][2] == dfr[2]["undistort"][1][2]
    kw.pop("undistort_images")
    assert "undistort" not in collate([Human36MMultiViewDataset(defer_image_ops=True, **kw)[i] for i in range(3)])


def test_c_entry_point_validates_before_device_work():
    lib = ctypes.CDLL(H.LIB_PATH)
    assert hasattr(lib, "lt_undistort_crop_resize_u8") and "lt_undistort_crop_resize_u8" in H.SIGNATURES
    l = H.lib()
    fake = 4096                          # never dereferenced: every call below fails its host-side checks
    f = l.lt_undistort_crop_resize_u8
    # window 10 x 10 at (5, 5) of a 50 x 60 frame, bbox (0, 0, 20, 20), map at 0 with pitch 60 (50 * 60 * 8 bytes)
    good = [0, 10, 10, 30, 5, 5, 50, 60, 0, 0, 20, 20, 0, 60]
    mb = 50 * 60 * 8
    dh = lambda d: np.ascontiguousarray(np.array([d], np.int64))
    call = lambda d, src_bytes=300, maps_bytes=mb, n=1, hh=8, ww=8, maps=fake: f(fake, src_bytes, fake, dh(d).ctypes.data_as(ctypes.c_void_p),
                                                                                 maps, maps_bytes, n, hh, ww, None, fake, None)
    assert call(good, n=0) == -1 and call(good, hh=0) == -1
    assert call(good, ww=4096) == -2
    assert call(good, maps=None) == -1
    assert call(good, maps=fake + 2) == -1 and b"aligned" in l.lt_last_error()

    def bad(i, v, msg):
        d = list(good); d[i] = v
        assert call(d) == -1, (i, v)
        assert msg in l.lt_last_error(), (i, v, l.lt_last_error())

    bad(10, 0, b"empty bbox")                     # zero width
    bad(11, -3, b"empty bbox")                    # negative height
    bad(6, 0, b"frame size")
    bad(7, 40000, b"frame size")
    bad(4, 55, b"leaves")                         # window past the frame's right edge
    bad(5, -1, b"leaves")
    bad(1, 46, b"leaves")
    bad(3, 20, b"source window")                  # pitch < 3 * width
    bad(0, 280, b"past src")
    bad(12, 4, b"bad map")                        # unaligned map offset
    bad(13, 59, b"bad map")                       # pitch < frame width
    bad(12, 8, b"past maps")
    assert call(good, maps_bytes=mb - 1) == -1 and b"past maps" in l.lt_last_error()
    assert call(good, src_bytes=299) == -1 and b"past src" in l.lt_last_error()


def test_descriptors_and_device_map():
    rng = np.random.default_rng(4)
    frames = [rng.integers(0, 256, (60, 80, 3), dtype=np.uint8) for _ in range(3)]
    maps = img.undistort_maps(*small_camera(60, 80, 2.0), 60, 80)
    dm = img.device_map(maps)
    assert dm.dtype == np.int16 and dm.shape == (60, 80, 4)
    assert np.array_equal(dm[..., :2], maps[0]) and np.array_equal(dm[..., 2].astype(np.uint16), maps[1]) and (dm[..., 3] == 0).all()
    boxes = np.array([(5, 5, 40, 50), (-20, -20, 10, 10), (200, 0, 230, 30)])
    mono = img.map_is_monotone(maps[0])
    desc, wins, total = img.undistort_descriptors(frames, boxes, [(maps[0], mono, 64, 80)] * 3)
    assert desc.shape == (3, img.UNDIST_DESC_FIELDS) and total == sum(w.size for w in wins)
    for i in range(3):
        x0, y0, x1, y1 = img.source_window(maps[0], boxes[i], (60, 80))
        assert list(desc[i]) == [sum(w.size for w in wins[:i]), y1 - y0, x1 - x0, 3 * (x1 - x0), x0, y0, 60, 80, *boxes[i], 64, 80]
    assert wins[2].size == 0


def test_cv2_cross_check():
    cv2 = pytest.importorskip("cv2")
    rng = np.random.default_rng(5)
    h, w = 200, 260
    K, d = small_camera(h, w, 2.0)
    grid = img.distortion_grid(K, d, h, w)
    m1, m2 = cv2.convertMaps(grid, None, cv2.CV_16SC2)
    ix, iy = np.rint(grid[..., 0] * 32).astype(np.int64), np.rint(grid[..., 1] * 32).astype(np.int64)
    assert np.array_equal(m1[..., 0], ix >> 5) and np.array_equal(m1[..., 1], iy >> 5)
    assert np.array_equal(m2, (iy & 31) * 32 + (ix & 31))
    src = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    ref = cv2.remap(src, m1, m2, cv2.INTER_CUBIC)
    assert np.array_equal(img.remap_cubic_u8(src, m1, m2), ref)
