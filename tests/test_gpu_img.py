"""GPU: lt_crop_resize_u8 (csrc/img_prep.hip) against the CPU view preparation of the reference dataset,
torch.from_numpy(normalize_image(resize_image(crop_image(frame, bbox), shape))).float() in CHW, bitwise; and prepare_batch_frames
on deferred Human36MMultiViewDataset items against prepare_batch on the CPU-prepared items (fixture: tests/golden/h36m_dataset.npz,
tools/make_golden_img.py)."""
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


def cpu_view(frame, bbox, shape, norm=True):
    r = img.resize_image(img.crop_image(frame, tuple(int(x) for x in bbox)), shape)
    if norm:
        return torch.from_numpy(img.normalize_image(r)).float().permute(2, 0, 1)
    return torch.from_numpy(r.astype(np.float32)).permute(2, 0, 1)


def downscale_views(rng, S, n):
    """n views into S x S covering every downscale branch: non-integer factors, x2, x3, non-square integer factors, identity, bboxes
    partly or wholly outside the frame, frames of different sizes."""
    frames, boxes = [], []
    fixed = [(2 * S, 2 * S), (3 * S, 3 * S), (S, 2 * S), (2 * S, S), (3 * S, S), (S, S), (S, S), (2 * S, 3 * S)]
    for i in range(n):
        sh, sw = fixed[i] if i < len(fixed) else (S + 1 + int(rng.integers(0, int(1.6 * S))), S + 1 + int(rng.integers(0, int(1.6 * S))))
        fh, fw = int(rng.integers(200, 900)), int(rng.integers(200, 900))
        f = rng.integers(0, 256, (fh, fw, 3), dtype=np.uint8)
        kind = i % 4
        if kind == 0:                                                    # straddles the top-left corner
            l, u = -int(rng.integers(1, sw)), -int(rng.integers(1, sh))
        elif kind == 1:                                                  # anywhere, mostly partly outside
            l, u = int(rng.integers(-sw // 2, fw)), int(rng.integers(-sh // 2, fh))
        elif kind == 2 and i % 8 == 2:                                   # wholly outside
            l, u = fw + 5, -sh - 3
        else:
            l, u = int(rng.integers(0, max(1, fw - sw))), int(rng.integers(0, max(1, fh - sh)))
        frames.append(f)
        boxes.append((l, u, l + sw, u + sh))
    return frames, np.array(boxes, np.int64)


@pytest.mark.parametrize("S", [384, 256])
def test_downscale_views_bitwise(S):
    rng = np.random.default_rng(S)
    frames, boxes = downscale_views(rng, S, 110)
    modes = {img.area_mode((b[3] - b[1], b[2] - b[0]), (S, S)) for b in boxes}
    assert modes == {"identity", "fast2x2", "fast", "area"}, modes
    out = img.crop_resize_normalize(frames, boxes, (S, S), device=DEV)
    torch.cuda.synchronize()
    got = out.cpu()
    bad = [i for i in range(len(frames)) if not torch.equal(got[i], cpu_view(frames[i], boxes[i], (S, S)))]
    record("img_prep/%d downscale views bitwise mismatches" % S, len(bad))
    assert not bad, bad[:10]
    # the same views shipped as bbox & frame only, the bbox shifted: same bits
    regs, shifted = [], []
    for f, (l, u, r, lo) in zip(frames, boxes):
        x0, x1 = min(max(l, 0), f.shape[1]), min(max(r, 0), f.shape[1])
        y0, y1 = min(max(u, 0), f.shape[0]), min(max(lo, 0), f.shape[0])
        regs.append(f[y0:max(y1, y0), x0:max(x1, x0)])
        shifted.append((l - x0, u - y0, r - x0, lo - y0))
    out2 = img.crop_resize_normalize(regs, np.array(shifted), (S, S), device=DEV)
    assert torch.equal(out2.cpu(), got)
    # deterministic
    out3 = img.crop_resize_normalize(frames, boxes, (S, S), device=DEV)
    assert torch.equal(out3.cpu(), got)


def test_upscale_and_mixed_views_within_one_level():
    rng = np.random.default_rng(7)
    S = 384
    frames, boxes = [], []
    for i in range(48):
        sh = int(rng.integers(40, S)) if i % 3 != 2 else int(rng.integers(S + 1, 900))
        sw = int(rng.integers(40, S)) if i % 3 != 1 else int(rng.integers(S + 1, 900))
        f = rng.integers(0, 256, (int(rng.integers(100, 700)), int(rng.integers(100, 700)), 3), dtype=np.uint8)
        l, u = int(rng.integers(-sw // 3, f.shape[1])), int(rng.integers(-sh // 3, f.shape[0]))
        frames.append(f); boxes.append((l, u, l + sw, u + sh))
    boxes = np.array(boxes)
    assert all(img.area_mode((b[3] - b[1], b[2] - b[0]), (S, S)) == "linear" for b in boxes)
    got = img.crop_resize_normalize(frames, boxes, (S, S), norm_image=False, device=DEV).cpu()
    ref = torch.stack([cpu_view(f, b, (S, S), norm=False) for f, b in zip(frames, boxes)])
    d = (got - ref).abs()
    frac = float((d > 0).double().mean())
    record("img_prep/upscale+mixed max level diff", float(d.max()))
    record("img_prep/upscale+mixed mismatch fraction", frac)
    assert float(d.max()) <= 1.0
    if img.cv2 is None:                 # resize_image is resize_area_u8, whose scalar rounding the kernel follows exactly
        assert frac == 0.0


def test_norm_image_false_and_lut():
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, (500, 600, 3), dtype=np.uint8) for _ in range(4)]
    boxes = np.array([(10, 20, 710, 620), (-50, 0, 450, 300), (0, 0, 256, 256), (100, 100, 612, 612)])
    raw = img.crop_resize_normalize(frames, boxes, (256, 256), norm_image=False, device=DEV).cpu()
    nrm = img.crop_resize_normalize(frames, boxes, (256, 256), device=DEV).cpu()
    for i in range(4):
        assert torch.equal(raw[i], cpu_view(frames[i], boxes[i], (256, 256), norm=False))
    lut = img.normalize_lut(DEV).cpu()
    assert torch.equal(nrm, torch.stack([lut[c][raw[:, c].long()] for c in range(3)], 1))


def test_empty_bbox_is_an_error_and_never_faults():
    f = np.zeros((50, 50, 3), np.uint8)
    for b in ((10, 10, 10, 30), (10, 30, 20, 10)):
        with pytest.raises(RuntimeError, match="empty bbox"):
            img.crop_resize_normalize([f, f], np.array([(0, 0, 50, 50), b]), (64, 64), device=DEV)
    # without the host copy of the descriptors the device cannot refuse: the view comes out as zeros
    block, desc = img.pack_regions([f + 7, f + 7], np.array([(0, 0, 50, 50), (10, 10, 10, 30)]))
    src, dd = torch.from_numpy(block).to(DEV), torch.from_numpy(desc).to(DEV)
    out = torch.full((2, 3, 64, 64), 5.0, device=DEV)
    img.launch_crop_resize(src, dd, None, (64, 64), None, out)
    torch.cuda.synchronize()
    assert (out[0] == 7).all() and (out[1] == 0).all()


def test_256_views_384():
    rng = np.random.default_rng(11)
    frames = [rng.integers(0, 256, (1000, 1000, 3), dtype=np.uint8) for _ in range(8)]
    views, boxes = [], []
    for i in range(256):
        s = int(rng.integers(300, 900))
        l, u = int(rng.integers(-100, 1000 - s // 2)), int(rng.integers(-100, 1000 - s // 2))
        views.append(frames[i % 8]); boxes.append((l, u, l + s, u + s))
    boxes = np.array(boxes)
    out = img.crop_resize_normalize(views, boxes, (384, 384), device=DEV)
    torch.cuda.synchronize()
    assert out.shape == (256, 3, 384, 384) and torch.isfinite(out).all()
    for i in (0, 77, 255):
        assert torch.equal(out[i].cpu(), cpu_view(views[i], boxes[i], (384, 384)))


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


def test_prepare_batch_frames_matches_prepare_batch_and_model(tmp_path):
    from mvn.datasets import utils as du
    from mvn.datasets.human36m import Human36MMultiViewDataset
    from mvn.models.triangulation import AlgebraicTriangulationNet
    from oracle import spec, synth
    root, lp = _dataset_tree(tmp_path)
    collate = du.make_collate_fn(randomize_n_views=False)
    for shape in ((256, 256), (24, 20)):
        kw = dict(h36m_root=root, labels_path=lp, image_shape=shape, test=True, scale_bbox=1.5)
        cpu = Human36MMultiViewDataset(**kw)
        gpu = Human36MMultiViewDataset(defer_image_ops=True, **kw)
        bc = collate([cpu[i] for i in range(3)])
        bg = collate([gpu[i] for i in range(3)])
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
    kw = dict(h36m_root=root, labels_path=lp, image_shape=(256, 256), test=True, scale_bbox=1.5)
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
