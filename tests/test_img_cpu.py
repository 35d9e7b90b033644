"""CPU: mvn.utils.img against the reference's own functions (tests/golden/img_ops.npz, tools/make_golden_img.py), the numpy
restatement of cv::resize(INTER_AREA) (resize_area_u8, the definition lt_crop_resize_u8 is tested against on the GPU), the
normalisation LUT, the region packing, and the new C entry point's argument checks (no device work)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import lt_hip as H
from mvn.utils import img

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLD, "img_ops.npz"))


def test_img_matches_reference_golden(g):
    for i, (f, b) in enumerate(zip(g["crop_frames"], g["crop_bboxes"])):
        c = img.crop_image(f, tuple(int(x) for x in b))
        assert c.dtype == np.uint8 and np.array_equal(c, g["crop_%d" % i]), i
    sb = np.array([img.scale_bbox(tuple(int(x) for x in b), s) for b, s in zip(g["bbox_in"], g["bbox_scales"])])
    assert np.array_equal(sb, g["scale_bbox"])
    sq = np.array([img.get_square_bbox(tuple(int(x) for x in b)) for b in g["bbox_in"]])
    assert np.array_equal(sq, g["square_bbox"])
    n = img.normalize_image(g["norm_in"])
    assert n.dtype == np.float64 and np.array_equal(n, g["norm_out"])
    assert np.array_equal(img.denormalize_image(g["denorm_in"]), g["denorm_out"])
    assert np.array_equal(img.image_batch_to_numpy(torch.from_numpy(g["batch_chw"])), g["batch_to_numpy"])
    t = img.image_batch_to_torch(g["batch_hwc"])
    assert t.dtype == torch.float32 and np.array_equal(t.numpy(), g["batch_to_torch"])
    assert np.array_equal(img.to_numpy(torch.arange(3)), np.arange(3)) and torch.equal(img.to_torch(np.arange(3)), torch.arange(3))
    with pytest.raises(ValueError):
        img.to_numpy([1, 2])
    with pytest.raises(ValueError):
        img.to_torch([1, 2])
    assert img.IMAGENET_MEAN.tolist() == [0.485, 0.456, 0.406] and img.IMAGENET_STD.tolist() == [0.229, 0.224, 0.225]


def area_integral(src, H, W):
    """fp64 INTER_AREA as an integral: the piecewise-constant source integrated over each output cell / the cell area."""
    def weights(s, d):
        sc = s / d
        M = np.zeros((d, s))
        for o in range(d):
            a, b = o * sc, min((o + 1) * sc, s)
            for k in range(int(np.floor(a)), int(np.ceil(b))):
                M[o, k] = max(0.0, min(b, k + 1) - max(a, k))
            M[o] /= (b - a)
        return M
    My, Mx = weights(src.shape[0], H), weights(src.shape[1], W)
    t = np.tensordot(My, src.astype(np.float64), axes=(1, 0))          # (H, w, 3)
    return np.einsum("yxc,Xx->yXc", t, Mx, optimize=True)


@pytest.mark.parametrize("src_hw,dst_hw", [((700, 510), (384, 384)), ((97, 61), (40, 33)), ((300, 451), (256, 256)), ((385, 900), (384, 384))])
def test_general_area_branch_against_fp64_integral(src_hw, dst_hw):
    rng = np.random.default_rng(src_hw[0] * 7 + dst_hw[1])
    src = rng.integers(0, 256, src_hw + (3,), dtype=np.uint8)
    assert img.area_mode(src_hw, dst_hw) == "area"
    pre = img._resize_area_f32(src, *dst_hw).astype(np.float64)
    ref = area_integral(src, *dst_hw)
    assert np.abs(pre - ref).max() < 1e-3
    out = img.resize_area_u8(src, dst_hw)
    assert out.dtype == np.uint8 and out.shape == dst_hw + (3,)
    diff = out.astype(np.int64) != np.clip(np.rint(ref), 0, 255).astype(np.int64)
    near_tie = np.abs(ref - np.floor(ref) - 0.5) < 1e-3
    assert not (diff & ~near_tie).any()


def test_branch_rounding_hand_cases():
    # 2x2: (a+b+c+d+2)>>2 rounds half up: 10/4 = 2.5 -> 3 (round-half-even would give 2)
    s = np.zeros((2, 2, 3), np.uint8); s[:, :, 0] = [[1, 2], [3, 4]]; s[:, :, 1] = [[0, 0], [0, 2]]; s[:, :, 2] = [[255, 255], [255, 254]]
    assert img.area_mode((2, 2), (1, 1)) == "fast2x2"
    assert img.resize_area_u8(s, (1, 1))[0, 0].tolist() == [3, 1, 255]          # 10/4 -> 3, 2/4 -> 1 (half up), 1019/4 -> 255
    # 1x2 (kx=1, ky=2) non-square integer factor: cvRound(sum * 0.5f) rounds half to even
    s = np.array([[[1, 2, 5]], [[2, 3, 6]]], np.uint8)                          # sums 3, 5, 11 -> 1.5, 2.5, 5.5
    assert img.area_mode((2, 1), (1, 1)) == "fast"
    assert img.resize_area_u8(s, (1, 1))[0, 0].tolist() == [2, 2, 6]
    # 4x4: sum / 16 at a tie (sum 40 -> 2.5 -> 2; sum 56 -> 3.5 -> 4)
    s = np.zeros((4, 4, 3), np.uint8); s[0, :3, 0] = [13, 13, 14]; s[0, :4, 1] = [14, 14, 14, 14]
    assert img.resize_area_u8(s, (1, 1))[0, 0].tolist() == [2, 4, 0]
    # 3x3: 1.f/9 in fp32 then cvRound: sum 9k + 4 -> k, 9k + 5 -> k + 1
    s = np.zeros((3, 3, 3), np.uint8); s[0, 0, 0] = 4; s[0, 0, 1] = 5; s[0, 0, 2] = 95
    assert img.area_mode((3, 3), (1, 1)) == "fast"
    assert img.resize_area_u8(s, (1, 1))[0, 0].tolist() == [0, 1, 11]
    # identity is a copy
    s = np.random.default_rng(0).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    assert img.area_mode((5, 7), (5, 7)) == "identity"
    r = img.resize_area_u8(s, (5, 7))
    assert np.array_equal(r, s) and r is not s
    # x3 downscale is the block mean rounded half to even
    s = np.random.default_rng(1).integers(0, 256, (12, 9, 3), dtype=np.uint8)
    m = s.astype(np.int64).reshape(4, 3, 3, 3, 3).sum(axis=(1, 3))
    assert np.array_equal(img.resize_area_u8(s, (4, 3)), np.rint(m.astype(np.float32) * np.float32(1 / np.float32(9))).astype(np.uint8))
    # scale just below an integer is the general branch, not the integer one
    assert img.area_mode((767, 767), (384, 384)) == "area"
    assert img.area_mode((768, 1152), (384, 384)) == "fast"


def test_linear_branch_properties():
    """Any upscaled axis: INTER_AREA's fixed-point bilinear.  Constants stay constant, and a ramp stays within one level of the
    fp64 bilinear with the same sample positions."""
    c = np.full((50, 200, 3), 77, np.uint8)
    for dst in ((384, 384), (384, 100), (30, 384)):
        assert img.area_mode(c.shape[:2], dst) == "linear"
        assert (img.resize_area_u8(c, dst) == 77).all()
    ramp = np.tile(np.linspace(0, 255, 97).round().astype(np.uint8)[None, :, None], (10, 1, 3))
    out = img.resize_area_u8(ramp, (10, 384)).astype(np.int64)
    s0, s1, w0, w1 = img.linear_tab(97, 384)
    ref = (ramp[0, s0, 0] * w0 + ramp[0, s1, 0] * w1) / 2048.0
    assert np.abs(out[0, :, 0] - ref).max() <= 1 and (np.diff(out[0, :, 0]) >= 0).all()


def test_resize_image_without_cv2_is_resize_area_u8():
    s = np.random.default_rng(2).integers(0, 256, (123, 77, 3), dtype=np.uint8)
    if img.cv2 is None:
        assert np.array_equal(img.resize_image(s, (64, 48)), img.resize_area_u8(s, (64, 48)))


def test_resize_area_u8_equals_cv2():
    """Where OpenCV is importable: bit-exact on every downscale branch, within one level (OpenCV's SIMD vertical pass rounds
    differently) when an axis is upscaled."""
    cv2 = pytest.importorskip("cv2")
    rng = np.random.default_rng(3)
    for src_hw, dst_hw in [((700, 510), (384, 384)), ((768, 768), (384, 384)), ((1152, 384), (384, 384)), ((384, 384), (384, 384)),
                           ((500, 999), (256, 256)), ((300, 200), (384, 384)), ((200, 900), (384, 384))]:
        s = rng.integers(0, 256, src_hw + (3,), dtype=np.uint8)
        ref = cv2.resize(s, (dst_hw[1], dst_hw[0]), interpolation=cv2.INTER_AREA)
        d = np.abs(img.resize_area_u8(s, dst_hw).astype(np.int64) - ref)
        assert d.max() <= (1 if img.area_mode(src_hw, dst_hw) == "linear" else 0), (src_hw, dst_hw)


def test_normalize_lut_is_normalize_image_in_fp32():
    v = np.arange(256, dtype=np.uint8)
    img_ = np.stack([v, v, v], axis=-1)[None]
    ref = torch.from_numpy(img.normalize_image(img_)).float().numpy()[0]       # (256, 3)
    lut = img.normalize_lut("cpu").numpy()                                     # (3, 256)
    assert lut.dtype == np.float32 and np.array_equal(lut.T, ref)


def test_pack_regions_layout():
    a = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3)
    b = torch.arange(4 * 1 * 3, dtype=torch.uint8).reshape(4, 1, 3)
    block, desc = img.pack_regions([a, b], [(0, 0, 3, 2), (-1, -2, 5, 6)])
    assert desc.dtype == np.int64 and desc.shape == (2, img.DESC_FIELDS)
    assert desc.tolist() == [[0, 2, 3, 9, 0, 0, 3, 2], [18, 4, 1, 3, -1, -2, 5, 6]]
    assert np.array_equal(block[:18], a.reshape(-1)) and np.array_equal(block[18:], b.numpy().reshape(-1))


def test_c_entry_point_exported_and_validates_before_device_work():
    lib = ctypes.CDLL(H.LIB_PATH)
    assert hasattr(lib, "lt_crop_resize_u8") and "lt_crop_resize_u8" in H.SIGNATURES
    l = H.lib()
    fake = 4096                                     # never dereferenced: every call below fails its host-side checks
    good = np.array([[0, 10, 10, 30, 0, 0, 5, 5]], np.int64)
    dh = lambda d: d.ctypes.data_as(ctypes.c_void_p)
    assert l.lt_crop_resize_u8(fake, 300, fake, dh(good), 0, 8, 8, None, fake, None) == -1
    assert l.lt_crop_resize_u8(fake, 300, fake, dh(good), 1, 0, 8, None, fake, None) == -1
    assert l.lt_crop_resize_u8(fake, 300, fake, dh(good), 1, 8, -3, None, fake, None) == -1
    for bad in ([0, 10, 10, 30, 5, 0, 5, 5], [0, 10, 10, 30, 0, 7, 5, 3]):          # zero width, negative height
        d = np.array([bad], np.int64)
        assert l.lt_crop_resize_u8(fake, 300, fake, dh(d), 1, 8, 8, None, fake, None) == -1
        assert b"empty bbox" in l.lt_last_error()
    d = np.array([[0, 11, 10, 30, 0, 0, 5, 5]], np.int64)                            # region ends past src
    assert l.lt_crop_resize_u8(fake, 300, fake, dh(d), 1, 8, 8, None, fake, None) == -1
    assert l.lt_crop_resize_u8(fake, 300, fake, dh(good), 1, 8, 4096, None, fake, None) == -2
