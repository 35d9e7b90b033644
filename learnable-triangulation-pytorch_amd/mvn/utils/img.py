"""Image helpers with the reference's names (mvn/utils/img.py of the reference), plus the GPU view preparation.

``crop_image`` / ``get_square_bbox`` / ``scale_bbox`` / ``normalize_image`` / ... are the reference's functions.  ``resize_image``
calls ``cv2.resize(INTER_AREA)`` when cv2 is importable and otherwise ``resize_area_u8``, a numpy restatement of OpenCV 4.x
INTER_AREA on 8-bit 3-channel images: the CPU definition the HIP kernel ``lt_crop_resize_u8`` is tested against.

``crop_resize_normalize`` runs crop (zero fill outside the frame) + INTER_AREA resize + ImageNet normalisation for a ragged list of
uint8 HWC views in ONE kernel launch and returns (N, 3, H, W) fp32 on the GPU: bitwise what
``torch.from_numpy(normalize_image(resize_image(crop_image(f, b), shape))).float()`` (transposed to CHW) gives.  Channel order is
kept as given (the reference normalises cv2's BGR pixels with RGB-ordered ImageNet constants).
"""
import ctypes as C

import numpy as np
import torch
from PIL import Image

try:
    import cv2
except ImportError:       # the build machine has no OpenCV: resize_image then uses resize_area_u8
    cv2 = None

IMAGENET_MEAN, IMAGENET_STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])


def crop_image(image, bbox):
    """The (lower - upper, right - left, 3) area of ``image`` inside ``bbox`` = (left, upper, right, lower), zeros where the bbox
    leaves the image (PIL's crop)."""
    return np.asarray(Image.fromarray(image).crop(bbox))


def resize_image(image, shape):
    """INTER_AREA resize to shape = (H, W): OpenCV when it is importable, else its numpy restatement resize_area_u8."""
    if cv2 is None:
        return resize_area_u8(image, shape)
    return cv2.resize(image, (shape[1], shape[0]), interpolation=cv2.INTER_AREA)


def get_square_bbox(bbox):
    """Square bbox: the shorter side is stretched to the longer one about its (floor) centre."""
    left, upper, right, lower = bbox
    w, h = right - left, lower - upper
    if w > h:
        upper = (upper + lower) // 2 - w // 2
        return left, upper, right, upper + w
    left = (left + right) // 2 - h // 2
    return left, upper, left + h, lower


def scale_bbox(bbox, scale):
    """bbox scaled about its (floor) centre; the new sides are int(scale * side)."""
    left, upper, right, lower = bbox
    cx, cy = (right + left) // 2, (lower + upper) // 2
    nw, nh = int(scale * (right - left)), int(scale * (lower - upper))
    left, upper = cx - nw // 2, cy - nh // 2
    return left, upper, left + nw, upper + nh


def to_numpy(tensor):
    if torch.is_tensor(tensor):
        return tensor.cpu().detach().numpy()
    if type(tensor).__module__ == "numpy":
        return tensor
    raise ValueError("Cannot convert {} to numpy array".format(type(tensor)))


def to_torch(ndarray):
    if type(ndarray).__module__ == "numpy":
        return torch.from_numpy(ndarray)
    if torch.is_tensor(ndarray):
        return ndarray
    raise ValueError("Cannot convert {} to torch tensor".format(type(ndarray)))


def image_batch_to_numpy(image_batch):
    """B,C,H,W -> B,H,W,C numpy."""
    return np.transpose(to_numpy(image_batch), (0, 2, 3, 1))


def image_batch_to_torch(image_batch):
    """B,H,W,C numpy -> B,C,H,W fp32 tensor."""
    return to_torch(np.transpose(image_batch, (0, 3, 1, 2))).float()


def normalize_image(image):
    """ImageNet normalisation of an (h, w, 3) image with levels 0..255, in float64."""
    return (image / 255.0 - IMAGENET_MEAN) / IMAGENET_STD


def denormalize_image(image):
    """Inverse of normalize_image, clipped to 0..255."""
    return np.clip((image * IMAGENET_STD + IMAGENET_MEAN) * 255.0, 0, 255)


# ---- OpenCV 4.x cv::resize(INTER_AREA) on 8UC3, restated in numpy ------------------------------------------------------------------
# Branches (modules/imgproc/src/resize.cpp): identity copy; integer factors on both axes (resizeAreaFast_: 2x2 with the SIMD rule
# (a+b+c+d+2)>>2, any other factor cvRound(sum * (1.f/area))); both scales >= 1 (resizeArea_ with computeResizeAreaTab tables, fp32
# accumulation in table order); otherwise bilinear in "area mode" with 11-bit fixed-point weights.  scale = 1 / (dsize / ssize) in
# double, as OpenCV computes it.  The kernel (csrc/img_prep.hip) evaluates the same expressions in the same order.

def _area_scale(ssize, dsize):
    return 1.0 / (float(dsize) / float(ssize))


def area_mode(src_hw, dst_hw):
    """'identity' | 'fast2x2' | 'fast' | 'area' | 'linear': the cv::resize INTER_AREA branch a (h, w) -> (H, W) resize takes."""
    (sh, sw), (H, W) = src_hw, dst_hw
    if (sh, sw) == (H, W):
        return "identity"
    sx, sy = _area_scale(sw, W), _area_scale(sh, H)
    ix, iy = int(np.rint(sx)), int(np.rint(sy))
    fast = abs(sx - ix) < np.finfo(np.float64).eps and abs(sy - iy) < np.finfo(np.float64).eps
    if sx >= 1 and sy >= 1:
        if fast:
            return "fast2x2" if (ix, iy) == (2, 2) else "fast"
        return "area"
    return "linear"


def area_tab(ssize, dsize):
    """computeResizeAreaTab for one axis -> (first source index (D,), taps (D,), alpha of every tap (D, maxtaps) fp32, 0 past the
    last tap).  The taps of one output cell are consecutive source indices."""
    scale = _area_scale(ssize, dsize)
    first = np.zeros(dsize, np.int64); n = np.zeros(dsize, np.int64); alphas = []
    for dx in range(dsize):
        fsx1 = dx * scale
        fsx2 = fsx1 + scale
        cell = min(scale, ssize - fsx1)
        sx1, sx2 = int(np.ceil(fsx1)), int(np.floor(fsx2))
        sx2 = min(sx2, ssize - 1)
        sx1 = min(sx1, sx2)
        a = []
        first[dx] = sx1
        if sx1 - fsx1 > 1e-3:
            first[dx] = sx1 - 1
            a.append(np.float32((sx1 - fsx1) / cell))
        a += [np.float32(1.0 / cell)] * (sx2 - sx1)
        if fsx2 - sx2 > 1e-3:
            a.append(np.float32(min(min(fsx2 - sx2, 1.0), cell) / cell))
        n[dx] = len(a)
        alphas.append(a)
    A = np.zeros((dsize, int(n.max())), np.float32)
    for dx, a in enumerate(alphas):
        A[dx, :len(a)] = a
    return first, n, A


def linear_tab(ssize, dsize):
    """INTER_AREA's bilinear fallback for one axis (area_mode branch of resize.cpp) -> (s0, s1, w0, w1), weights in 1/2048."""
    scale = _area_scale(ssize, dsize)
    inv = float(dsize) / float(ssize)
    d = np.arange(dsize)
    s = np.floor(d * scale).astype(np.int64)
    f = ((d + 1) - (s + 1) * inv).astype(np.float32)
    f = np.where(f <= 0, np.float32(0), f - np.floor(f).astype(np.float32)).astype(np.float32)
    edge = s >= ssize - 1
    f = np.where(edge, np.float32(0), f).astype(np.float32)
    s = np.where(edge, ssize - 1, s)
    w0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)
    w1 = np.rint(f * np.float32(2048)).astype(np.int64)
    return s, np.minimum(s + 1, ssize - 1), w0, w1


def _resize_area_f32(src, H, W):
    """General INTER_AREA downscale, the pre-rounding fp32 result (H, W, 3): buf = sum_x S*alpha per source row, then
    sum = sum_y beta*buf, both in increasing source index, one rounding per operation."""
    sh, sw = src.shape[:2]
    fx, nx, ax = area_tab(sw, W)
    fy, ny, ay = area_tab(sh, H)
    S = src.astype(np.float32)
    buf = None
    for i in range(ax.shape[1]):                                      # (sh, W, 3)
        cols = np.minimum(fx + i, sw - 1)
        t = S[:, cols, :] * ax[:, i][None, :, None]
        t = np.where((i < nx)[None, :, None], t, np.float32(0))
        buf = t if buf is None else buf + t
    out = None
    for j in range(ay.shape[1]):
        rows = np.minimum(fy + j, sh - 1)
        t = ay[:, j][:, None, None] * buf[rows]
        t = np.where((j < ny)[:, None, None], t, np.float32(0))
        out = t if out is None else out + t
    return out


def resize_area_u8(image, shape):
    """cv2.resize(image, (W, H), interpolation=cv2.INTER_AREA) for a uint8 (h, w, 3) image, in numpy."""
    src = np.ascontiguousarray(image, dtype=np.uint8)
    assert src.ndim == 3 and src.shape[2] == 3, src.shape
    H, W = int(shape[0]), int(shape[1])
    sh, sw = src.shape[:2]
    mode = area_mode((sh, sw), (H, W))
    if mode == "identity":
        return src.copy()
    if mode in ("fast2x2", "fast"):
        kx, ky = sw // W, sh // H
        s = src.astype(np.int64).reshape(H, ky, W, kx, 3).sum(axis=(1, 3))
        if mode == "fast2x2":
            return ((s + 2) >> 2).astype(np.uint8)
        v = np.rint(s.astype(np.float32) * (np.float32(1) / np.float32(kx * ky)))
        return np.clip(v, 0, 255).astype(np.uint8)
    if mode == "area":
        return np.clip(np.rint(_resize_area_f32(src, H, W)), 0, 255).astype(np.uint8)
    xs0, xs1, xw0, xw1 = linear_tab(sw, W)
    ys0, ys1, yw0, yw1 = linear_tab(sh, H)
    S = src.astype(np.int64)
    hrow = S[:, xs0, :] * xw0[None, :, None] + S[:, xs1, :] * xw1[None, :, None]          # (sh, W, 3)
    v = (hrow[ys0] * yw0[:, None, None] + hrow[ys1] * yw1[:, None, None] + (1 << 21)) >> 22
    return np.clip(v, 0, 255).astype(np.uint8)


# ---- Lens undistortion: the reference's offline pass (human36m_preprocessing/undistort-h36m.py), per view -------------------------
# The distortion maps come from the reference script's float32 expressions (:56-73), quantised as cv2.convertMaps(..., CV_16SC2)
# does (1/32 px: map1 = integer part, map2 = iy_frac * 32 + ix_frac).  cv2.remap(frame, map1, map2, INTER_CUBIC) on 8UC3 is restated
# from OpenCV 4.x (modules/imgproc/src/imgwarp.cpp: interpolateCubic, initInterTab2D, remapBicubic with a constant border of 0):
# 4 x 4 taps from (x - 1, y - 1), 15-bit fixed-point weights, taps outside the frame read 0, saturate_u8((sum + (1 << 14)) >> 15).
# The maps are built once per camera on the host (as the reference does) and never on the device, where powf and FMA contraction
# could move a coordinate across a 1/32 px rounding boundary.  The HIP kernel lt_undistort_crop_resize_u8 reads these maps and
# evaluates the same integer arithmetic.

INTER_BITS, INTER_TAB_SIZE, INTER_REMAP_COEF_BITS = 5, 32, 15
_cubic_tab = None


def _interpolate_cubic(x):
    """OpenCV's interpolateCubic(float x, float* coeffs), A = -0.75, every operation in float32."""
    f = np.float32
    A, x = f(-0.75), f(x)
    x1 = x + f(1)
    c0 = ((A * x1 - f(5) * A) * x1 + f(8) * A) * x1 - f(4) * A
    c1 = ((A + f(2)) * x - (A + f(3))) * x * x + f(1)
    y = f(1) - x
    c2 = ((A + f(2)) * y - (A + f(3))) * y * y + f(1)
    c3 = f(1) - c0 - c1 - c2
    return [c0, c1, c2, c3]


def cubic_tab():
    """initInterTab2D(INTER_CUBIC, fixpt=true): int16 (1024, 16); row i * 32 + j holds the 4 x 4 weights (row k1, column k2) for the
    y fraction i / 32 and x fraction j / 32, cvRound(wy[k1] * wx[k2] * 32768) with the one-entry correction that makes each block
    sum to 32768 (OpenCV adjusts the largest (sum too small) or smallest (sum too large) of the central 2 x 2)."""
    global _cubic_tab
    if _cubic_tab is None:
        tab1 = [_interpolate_cubic(np.float32(i) * np.float32(1.0 / INTER_TAB_SIZE)) for i in range(INTER_TAB_SIZE)]
        tab = np.zeros((INTER_TAB_SIZE * INTER_TAB_SIZE, 16), np.int16)
        for i in range(INTER_TAB_SIZE):
            for j in range(INTER_TAB_SIZE):
                it = [0] * 16
                for k1 in range(4):
                    for k2 in range(4):
                        v = tab1[i][k1] * tab1[j][k2]
                        it[k1 * 4 + k2] = int(np.clip(np.rint(v * np.float32(1 << INTER_REMAP_COEF_BITS)), -32768, 32767))
                diff = sum(it) - (1 << INTER_REMAP_COEF_BITS)
                if diff:
                    mk, Mk = (2, 2), (2, 2)
                    for k1 in (2, 3):
                        for k2 in (2, 3):
                            if it[k1 * 4 + k2] < it[mk[0] * 4 + mk[1]]:
                                mk = (k1, k2)
                            elif it[k1 * 4 + k2] > it[Mk[0] * 4 + Mk[1]]:
                                Mk = (k1, k2)
                    k = Mk if diff < 0 else mk
                    it[k[0] * 4 + k[1]] -= diff
                tab[i * INTER_TAB_SIZE + j] = it
        _cubic_tab = tab
    return _cubic_tab


def distortion_grid(K, dist, h, w):
    """float32 (h, w, 2): the distorted source position of every undistorted pixel, the reference script's expressions in its order
    (undistort-h36m.py:56-73).  K (3, 3) and dist (5,) are taken as float32, the dtype of the labels file."""
    K = np.asarray(K, dtype=np.float32)
    dist = np.asarray(dist, dtype=np.float32).reshape(-1)
    fx, fy = K[0, 0], K[1, 1]
    cx, cy = K[0, 2], K[1, 2]
    grid_x = (np.arange(w, dtype=np.float32) - cx) / fx
    grid_y = (np.arange(h, dtype=np.float32) - cy) / fy
    meshgrid = np.stack(np.meshgrid(grid_x, grid_y), axis=2).reshape(-1, 2)
    k = dist[:3].copy(); k[2] = dist[-1]
    p = dist[2:4].copy()
    r2 = meshgrid[:, 0] ** 2 + meshgrid[:, 1] ** 2
    radial = meshgrid * (1 + k[0] * r2 + k[1] * r2**2 + k[2] * r2**3).reshape(-1, 1)
    tangential_1 = p.reshape(1, 2) * np.broadcast_to(meshgrid[:, 0:1] * meshgrid[:, 1:2], (len(meshgrid), 2))
    tangential_2 = p[::-1].reshape(1, 2) * (meshgrid**2 + np.broadcast_to(r2.reshape(-1, 1), (len(meshgrid), 2)))
    meshgrid = radial + tangential_1 + tangential_2
    meshgrid *= np.array([fx, fy]).reshape(1, 2)
    meshgrid += np.array([cx, cy]).reshape(1, 2)
    return meshgrid.reshape(h, w, 2)


def undistort_maps(K, dist, h, w):
    """(map1 int16 (h, w, 2) = integer (x, y), map2 uint16 (h, w) = (iy & 31) * 32 + (ix & 31)) for an h x w frame:
    cv2.convertMaps(distortion_grid(K, dist, h, w), None, cv2.CV_16SC2), with cv2 when it is importable, else restated
    (ix = cvRound(x * 32), half to even)."""
    grid = distortion_grid(K, dist, h, w)
    if cv2 is not None:
        map1, map2 = cv2.convertMaps(grid, None, cv2.CV_16SC2)
        return map1, map2
    i = np.clip(np.rint(grid * np.float32(INTER_TAB_SIZE)), -2.0**31, 2.0**31 - 128).astype(np.int64)
    map1 = np.clip(i >> INTER_BITS, -32768, 32767).astype(np.int16)
    m = INTER_TAB_SIZE - 1
    map2 = ((i[..., 1] & m) * INTER_TAB_SIZE + (i[..., 0] & m)).astype(np.uint16)
    return map1, map2


def remap_cubic_u8(src, map1, map2, rows=slice(None), cols=slice(None)):
    """cv2.remap(src, map1, map2, INTER_CUBIC) of a uint8 (h, w, 3) frame (constant border 0), restricted to the output rectangle
    map1[rows, cols]: taps (x - 1 .. x + 2, y - 1 .. y + 2) of map1, weights cubic_tab()[map2], taps outside src read 0,
    saturate_u8((sum + (1 << 14)) >> 15)."""
    src = np.ascontiguousarray(src, dtype=np.uint8)
    assert src.ndim == 3 and src.shape[2] == 3, src.shape
    h, w = src.shape[:2]
    m1, m2 = map1[rows, cols], map2[rows, cols]
    sx = m1[..., 0].astype(np.int64) - 1
    sy = m1[..., 1].astype(np.int64) - 1
    wt = cubic_tab().astype(np.int64)[m2.astype(np.int64)]            # (r, c, 16)
    acc = np.zeros(m2.shape + (3,), np.int64)
    for k1 in range(4):
        yy = sy + k1
        vy = (yy >= 0) & (yy < h)
        yc = np.clip(yy, 0, h - 1)
        for k2 in range(4):
            xx = sx + k2
            ok = vy & (xx >= 0) & (xx < w)
            px = src[yc, np.clip(xx, 0, w - 1)].astype(np.int64) * ok[..., None]
            acc += px * wt[..., k1 * 4 + k2, None]
    return np.clip((acc + (1 << (INTER_REMAP_COEF_BITS - 1))) >> INTER_REMAP_COEF_BITS, 0, 255).astype(np.uint8)


def _clip_box(bbox, frame_hw):
    """bbox & frame as (x0, y0, x1, y1), empty (x1 <= x0 or y1 <= y0) when they do not meet."""
    l, u, r, lo = (int(x) for x in bbox)
    fh, fw = frame_hw
    x0, x1 = min(max(l, 0), fw), min(max(r, 0), fw)
    y0, y1 = min(max(u, 0), fh), min(max(lo, 0), fh)
    return x0, y0, max(x1, x0), max(y1, y0)


def undistort_crop_u8(frame, maps, bbox):
    """crop_image(cv2.remap(frame, *maps, INTER_CUBIC), bbox) -- the undistorted frame cropped to bbox = (left, upper, right, lower),
    zeros outside the frame -- computing only the pixels of bbox & frame.  maps: undistort_maps of the frame's camera and size."""
    map1, map2 = maps
    fh, fw = frame.shape[:2]
    assert map1.shape[:2] == (fh, fw), (map1.shape, frame.shape)
    l, u, r, lo = (int(x) for x in bbox)
    out = np.zeros((lo - u, r - l, 3), np.uint8)
    x0, y0, x1, y1 = _clip_box(bbox, (fh, fw))
    if x1 > x0 and y1 > y0:
        if cv2 is not None:
            part = cv2.remap(frame, np.ascontiguousarray(map1[y0:y1, x0:x1]), np.ascontiguousarray(map2[y0:y1, x0:x1]), cv2.INTER_CUBIC)
        else:
            part = remap_cubic_u8(frame, map1, map2, slice(y0, y1), slice(x0, x1))
        out[y0 - u:y1 - u, x0 - l:x1 - l] = part
    return out


def map_is_monotone(map1):
    """True when map1's x is non-decreasing along every row and its y along every column: then the range of the map over a rectangle
    is read off the rectangle's perimeter (source_window)."""
    return bool((np.diff(map1[..., 0], axis=1) >= 0).all() and (np.diff(map1[..., 1], axis=0) >= 0).all())


def source_window(map1, bbox, frame_hw, monotone=None):
    """(x0, y0, x1, y1): the rectangle of the distorted frame that the remap taps of bbox & frame read -- the range of map1 over
    bbox & frame widened by -1 / +2 (the 4 x 4 taps) and clipped to the frame; (0, 0, 0, 0) when nothing is read.  monotone: the
    cached map_is_monotone(map1) (computed here when None); a monotone map is read on the perimeter, any other over the whole slice."""
    fh, fw = frame_hw
    x0, y0, x1, y1 = _clip_box(bbox, frame_hw)
    if x1 <= x0 or y1 <= y0:
        return 0, 0, 0, 0
    if monotone is None:
        monotone = map_is_monotone(map1)
    if monotone:
        mx0, mx1 = int(map1[y0:y1, x0, 0].min()), int(map1[y0:y1, x1 - 1, 0].max())
        my0, my1 = int(map1[y0, x0:x1, 1].min()), int(map1[y1 - 1, x0:x1, 1].max())
    else:
        s = map1[y0:y1, x0:x1]
        mx0, mx1 = int(s[..., 0].min()), int(s[..., 0].max())
        my0, my1 = int(s[..., 1].min()), int(s[..., 1].max())
    wx0, wx1 = min(max(mx0 - 1, 0), fw), min(max(mx1 + 3, 0), fw)
    wy0, wy1 = min(max(my0 - 1, 0), fh), min(max(my1 + 3, 0), fh)
    if wx1 <= wx0 or wy1 <= wy0:
        return 0, 0, 0, 0
    return wx0, wy0, wx1, wy1


# ---- GPU: crop + resize + normalise of a ragged batch of views ---------------------------------------------------------------------
DESC_FIELDS = 8          # int64 per view: byte offset, region h, w, row pitch (bytes), bbox left, upper, right, lower (region coords)
_lut = {}


def normalize_lut(device):
    """3 x 256 fp32: float32((v / 255.0 - IMAGENET_MEAN[c]) / IMAGENET_STD[c]) -- normalize_image(...).float() of every level."""
    device = torch.device(device)
    if device not in _lut:
        v = np.arange(256, dtype=np.float64)
        t = np.stack([(v / 255.0 - IMAGENET_MEAN[c]) / IMAGENET_STD[c] for c in range(3)]).astype(np.float32)
        _lut[device] = torch.from_numpy(t).to(device)
    return _lut[device]


def pack_regions(src_regions, bboxes):
    """list of uint8 (h, w, 3) arrays / tensors + (N, 4) int bboxes (region coordinates) -> (flat uint8 numpy block, (N, 8) int64
    descriptors).  Rows are packed densely (pitch = 3 w)."""
    bboxes = np.asarray(bboxes).reshape(-1, 4)
    assert len(src_regions) == len(bboxes), (len(src_regions), len(bboxes))
    arrs = [np.ascontiguousarray(to_numpy(r), dtype=np.uint8) for r in src_regions]
    desc = np.zeros((len(arrs), DESC_FIELDS), np.int64)
    off = 0
    for i, a in enumerate(arrs):
        assert a.ndim == 3 and a.shape[2] == 3, a.shape
        desc[i, :4] = (off, a.shape[0], a.shape[1], 3 * a.shape[1])
        desc[i, 4:] = bboxes[i]
        off += a.nbytes
    block = np.empty(off, np.uint8)
    for i, a in enumerate(arrs):
        block[desc[i, 0]:desc[i, 0] + a.nbytes] = a.reshape(-1)
    return block, desc


def launch_crop_resize(src, desc, desc_host, image_shape, lut, out):
    """lt_crop_resize_u8 on the current stream.  src: flat uint8 device tensor; desc: (N, 8) int64 device tensor; desc_host: the same
    records on the host (validated before the launch) or None; out: (N, 3, H, W) fp32 device tensor."""
    import lt_hip as H
    H.require_gpu(src, "src"); H.require_gpu(desc, "desc"); H.require_gpu(out, "out")
    assert src.dtype == torch.uint8 and desc.dtype == torch.int64 and out.dtype == torch.float32 and out.is_contiguous()
    n = desc.shape[0]
    assert tuple(out.shape) == (n, 3, int(image_shape[0]), int(image_shape[1])), out.shape
    dh = None
    if desc_host is not None:
        desc_host = np.ascontiguousarray(desc_host, dtype=np.int64)
        dh = desc_host.ctypes.data_as(C.c_void_p)
    H.check(H.lib().lt_crop_resize_u8(H.ptr(src), src.numel(), H.ptr(desc), dh, n, int(image_shape[0]), int(image_shape[1]),
                                      H.ptr(lut), H.ptr(out), H.cur_stream()), "lt_crop_resize_u8")
    return out


def crop_resize_normalize(src_regions, bboxes, image_shape, norm_image=True, out=None, device="cuda:0"):
    """Crop every region to its bbox (zero fill outside), resize it to ``image_shape`` with INTER_AREA and (norm_image) normalise
    it, in one kernel launch.  src_regions: list of uint8 (h, w, 3) arrays or tensors (sizes may differ); bboxes: (N, 4) ints
    (left, upper, right, lower) relative to each region.  Returns (N, 3, H, W) fp32 on ``device``."""
    device = torch.device(out.device if out is not None else device)
    block, desc = pack_regions(src_regions, bboxes)
    src = torch.from_numpy(block).to(device, non_blocking=False)
    desc_dev = torch.from_numpy(desc).to(device)
    if out is None:
        out = torch.empty((len(desc), 3, int(image_shape[0]), int(image_shape[1])), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        return launch_crop_resize(src, desc_dev, desc, image_shape, normalize_lut(device) if norm_image else None, out)


# ---- GPU: lens undistortion + crop + resize + normalise of a ragged batch of views -------------------------------------------------
# int64 per view: source window byte offset into src, window height, width, row pitch (bytes), window x0, y0 (frame coordinates),
# frame height, width, bbox left, upper, right, lower (frame coordinates), map byte offset into maps, map row pitch (entries)
UNDIST_DESC_FIELDS = 14


def device_map(maps):
    """undistort_maps' (map1, map2) -> int16 (h, w, 4) = (x, y, map2, 0): the 8-byte-per-pixel map lt_undistort_crop_resize_u8 reads."""
    map1, map2 = maps
    h, w = map2.shape
    m = np.zeros((h, w, 4), np.int16)
    m[..., :2] = map1
    m[..., 2] = map2.astype(np.int16)          # 0 .. 1023
    return m


def undistort_descriptors(frames, bboxes, views_maps):
    """Descriptors and source windows of a ragged batch.  frames: list of uint8 (h, w, 3) frames; bboxes: (N, 4) frame coordinates;
    views_maps: per view (map1, monotone, map byte offset, map row pitch in entries).  Returns ((N, 14) int64 descriptors with
    window offsets counted from 0 in view order, list of the window arrays (views of the frames, not copies), total window bytes)."""
    bboxes = np.asarray(bboxes, dtype=np.int64).reshape(-1, 4)
    desc = np.zeros((len(frames), UNDIST_DESC_FIELDS), np.int64)
    wins = []
    off = 0
    for i, f in enumerate(frames):
        fh, fw = f.shape[:2]
        map1, mono, moff, mpitch = views_maps[i]
        x0, y0, x1, y1 = source_window(map1, bboxes[i], (fh, fw), mono)
        win = f[y0:y1, x0:x1]
        desc[i] = (off, y1 - y0, x1 - x0, 3 * (x1 - x0), x0, y0, fh, fw, *bboxes[i], moff, mpitch)
        wins.append(win)
        off += win.size
    return desc, wins, off


def launch_undistort_crop_resize(src, desc, desc_host, maps, image_shape, lut, out):
    """lt_undistort_crop_resize_u8 on the current stream.  src: flat uint8 device tensor of the source windows; desc: (N, 14) int64
    device tensor (UNDIST_DESC_FIELDS); desc_host: the same records on the host (validated before the launch) or None; maps: int16
    device tensor of device_map() blocks; out: (N, 3, H, W) fp32 device tensor."""
    import lt_hip as H
    H.require_gpu(src, "src"); H.require_gpu(desc, "desc"); H.require_gpu(maps, "maps"); H.require_gpu(out, "out")
    assert src.dtype == torch.uint8 and desc.dtype == torch.int64 and maps.dtype == torch.int16 and out.dtype == torch.float32
    assert out.is_contiguous() and maps.is_contiguous()
    n = desc.shape[0]
    assert tuple(out.shape) == (n, 3, int(image_shape[0]), int(image_shape[1])), out.shape
    dh = None
    if desc_host is not None:
        desc_host = np.ascontiguousarray(desc_host, dtype=np.int64)
        dh = desc_host.ctypes.data_as(C.c_void_p)
    H.check(H.lib().lt_undistort_crop_resize_u8(H.ptr(src), src.numel(), H.ptr(desc), dh, H.ptr(maps), maps.numel() * 2, n,
                                                int(image_shape[0]), int(image_shape[1]), H.ptr(lut), H.ptr(out), H.cur_stream()),
            "lt_undistort_crop_resize_u8")
    return out


def undistort_crop_resize_normalize(frames, maps, bboxes, image_shape, norm_image=True, out=None, device="cuda:0"):
    """Per view: undistort (cv2.remap INTER_CUBIC with that view's maps), crop to the bbox (zero fill outside the frame), INTER_AREA
    resize to ``image_shape`` and (norm_image) normalise, in one kernel launch -- bitwise
    normalize_image(resize_image(undistort_crop_u8(frame, maps, bbox), image_shape)).float() in CHW.  frames: list of uint8 (h, w, 3);
    maps: per view undistort_maps(...) of its camera (views sharing a camera may pass the same tuple: it is uploaded once); bboxes:
    (N, 4) frame coordinates.  Returns (N, 3, H, W) fp32 on ``device``."""
    device = torch.device(out.device if out is not None else device)
    blocks, at, views_maps, moff = [], {}, [], 0
    for m in maps:
        if id(m) not in at:
            dm = device_map(m)
            at[id(m)] = (map_is_monotone(m[0]), moff, dm.shape[1])
            blocks.append(dm.reshape(-1))
            moff += dm.nbytes
        mono, o, pitch = at[id(m)]
        views_maps.append((m[0], mono, o, pitch))
    desc, wins, total = undistort_descriptors(frames, bboxes, views_maps)
    block = np.empty(max(total, 1), np.uint8)
    for i, wn in enumerate(wins):
        if wn.size:
            block[desc[i, 0]:desc[i, 0] + wn.size].reshape(wn.shape)[...] = wn
    src = torch.from_numpy(block).to(device)
    dmaps = torch.from_numpy(np.concatenate(blocks)).to(device)
    desc_dev = torch.from_numpy(desc).to(device)
    if out is None:
        out = torch.empty((len(desc), 3, int(image_shape[0]), int(image_shape[1])), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        return launch_undistort_crop_resize(src, desc_dev, desc, dmaps, image_shape, normalize_lut(device) if norm_image else None, out)
