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
