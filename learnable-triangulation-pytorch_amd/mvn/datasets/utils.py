"""Batch plumbing either side of the hot path, with the reference's names and contracts
(mvn/datasets/utils.py of the reference): ``make_collate_fn`` builds the ``batch`` dict the models consume
(SURVEY.md section 8b), ``prepare_batch`` turns it into device tensors.

MI355X-side difference: the reference uploads the images view by view (B small H2D copies plus a device-side stack,
datasets/utils.py:47-53); here the whole (B, NV, H, W, 3) block goes through ONE pinned staging buffer and one asynchronous
copy, and the HWC -> CHW permutation happens on the device."""
import numpy as np
import torch

from lt_staging import PinnedRing


def make_collate_fn(randomize_n_views=True, min_n_views=10, max_n_views=31, mask_views=False):
    """Reference datasets/utils.py:6-39: drops ``None`` items, optionally sub-samples the views (np.random, like the
    reference), and stacks per-view lists into the batch dict.

    mask_views (with randomize_n_views): every batch has the SAME view count, ``min(total_n_views, max_n_views)`` views (a random choice of
    that many, in ascending index order), and the drawn view count becomes ``batch["view_mask"]`` instead of the batch's shape: ``n_views`` is
    drawn once per batch as the reference draws it, and every sample gets its own random subset of ``n_views`` valid views ((B, NV) uint8,
    1 = valid).  One training plan then serves every draw (``masked_training`` on the model).  False: the function and its sequence of
    np.random calls are the reference's."""

    def collate_fn(items):
        items = [x for x in items if x is not None]
        if len(items) == 0:
            print("All items in batch are None")
            return None
        batch = dict()
        key = "images" if "images" in items[0] else "frames"        # "frames" + "bboxes": deferred pixel work (prepare_batch_frames)
        total_n_views = min(len(item[key]) for item in items)
        indexes = np.arange(total_n_views)
        if randomize_n_views and mask_views:
            kept = min(total_n_views, max_n_views)
            n_views = np.random.randint(min_n_views, kept + 1)
            indexes = np.sort(np.random.choice(np.arange(total_n_views), size=kept, replace=False))
            view_mask = np.zeros((len(items), kept), dtype=np.uint8)
            for row in view_mask:          # every sample its own subset of n_views valid views
                row[np.random.choice(kept, size=n_views, replace=False)] = 1
            batch["view_mask"] = view_mask
        elif randomize_n_views:
            n_views = np.random.randint(min_n_views, min(total_n_views, max_n_views) + 1)
            indexes = np.random.choice(np.arange(total_n_views), size=n_views, replace=False)
        if key == "images":
            batch["images"] = np.stack([np.stack([item["images"][i] for item in items], axis=0) for i in indexes], axis=0).swapaxes(0, 1)
        else:
            batch["frames"] = [[item["frames"][i] for item in items] for i in indexes]       # list[NV] of list[B] of uint8 (h, w, 3)
            batch["bboxes"] = np.array([[item["bboxes"][i] for item in items] for i in indexes]).swapaxes(0, 1)   # (B, NV, 4)
            if "undistort" in items[0]:      # undistort_on_the_fly: per view (K, dist, frame (h, w)), the key of its camera's maps
                batch["undistort"] = [[item["undistort"][i] for item in items] for i in indexes]
        batch["detections"] = np.array([[item["detections"][i] for item in items] for i in indexes]).swapaxes(0, 1)
        batch["cameras"] = [[item["cameras"][i] for item in items] for i in indexes]
        batch["keypoints_3d"] = [item["keypoints_3d"] for item in items]
        batch["indexes"] = [item["indexes"] for item in items]
        try:
            batch["pred_keypoints_3d"] = np.array([item["pred_keypoints_3d"] for item in items])
        except Exception:       # the reference swallows a missing key the same way (:33-36)
            pass
        return batch

    return collate_fn


def worker_init_fn(worker_id):
    np.random.seed(np.random.get_state()[1][0] + worker_id)


STAGE_RING = 3          # pinned staging blocks per shape: prepare_batch of batch i+1, i+2 may fill while batch i's H2D copy is still queued
_staging = {}


def _ring(shape, dtype):
    """The staging ring (lt_staging.PinnedRing) for blocks of this shape."""
    key = (tuple(shape), dtype)
    ring = _staging.get(key)
    if ring is None:
        if len(_staging) > 4:
            _staging.clear()
        ring = _staging[key] = PinnedRing(shape, dtype, STAGE_RING, pin=torch.cuda.is_available())
    return ring


def prepare_batch(batch, device, config=None, is_train=True):
    """batch dict -> (images (B,NV,3,H,W) fp32, keypoints_3d_gt (B,J,3), keypoints_3d_validity_gt (B,J,1),
    proj_matricies (B,NV,3,4) fp32), all on ``device`` -- reference datasets/utils.py:45-65."""
    device = torch.device(device)
    images = np.asarray(batch["images"])                     # (B, NV, H, W, 3), any real dtype
    if device.type == "cuda":
        ring = _ring(images.shape, torch.float32)
        stage = ring.acquire()
        stage.copy_(torch.from_numpy(np.ascontiguousarray(images)))   # dtype conversion on the way into the pinned block
        dev = stage.to(device, non_blocking=True)
        ring.commit(torch.cuda.current_stream(device))
    else:
        dev = torch.from_numpy(np.ascontiguousarray(images)).float()
    images_batch = dev.permute(0, 1, 4, 2, 3).contiguous()   # BxNVxHxWxC -> BxNVxCxHxW (reference img.py:95-98 per view)
    return (images_batch,) + _targets(batch, device)


def _targets(batch, device):
    kp = np.stack(batch["keypoints_3d"], axis=0)
    keypoints_3d_batch_gt = torch.from_numpy(kp[:, :, :3]).float().to(device)
    keypoints_3d_validity_batch_gt = torch.from_numpy(kp[:, :, 3:]).float().to(device)
    proj = np.stack([np.stack([camera.projection for camera in camera_batch], axis=0) for camera_batch in batch["cameras"]], axis=0)
    proj_matricies_batch = torch.from_numpy(np.ascontiguousarray(proj.swapaxes(0, 1))).float().to(device)   # (B, NV, 3, 4)
    return keypoints_3d_batch_gt, keypoints_3d_validity_batch_gt, proj_matricies_batch


def prepare_batch_frames(batch, device, image_shape, norm_image=True):
    """prepare_batch for a batch of deferred items (Human36MMultiViewDataset(defer_image_ops=True) collated by make_collate_fn):
    batch["frames"] list[NV] of list[B] uint8 (h, w, 3) frames of any sizes, batch["bboxes"] (B, NV, 4) crop boxes in frame
    coordinates.  Only the bytes of bbox & frame travel: the host packs them, with the view descriptors in front, into one pinned
    block of the staging ring, one asynchronous H2D copy moves it, and one lt_crop_resize_u8 launch crops,
    resizes (INTER_AREA) and normalises every view.  Returns the same 4-tuple as prepare_batch; the images are bitwise what
    prepare_batch gives for the CPU-prepared items (normalize_image(resize_image(crop_image(...))) cast to fp32).

    A batch that carries "undistort" (undistort_on_the_fly=True items: per view the (K, dist, frame (h, w)) of its camera) is
    undistorted on the way: each camera's maps are built once and kept on the device (DeviceMapCache), only the source window of
    every view travels (mvn/utils/img.py:source_window), and one lt_undistort_crop_resize_u8 launch remaps, crops, resizes and
    normalises every view -- bitwise what prepare_batch gives for the CPU-prepared undistort_on_the_fly=True items."""
    from mvn.utils import img
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("prepare_batch_frames runs the crop / resize / normalise kernel: device must be a GPU (got %s)" % device)
    frames, bboxes = batch["frames"], np.asarray(batch["bboxes"], dtype=np.int64)
    nv, bs = len(frames), len(frames[0])
    n = bs * nv
    H, W = int(image_shape[0]), int(image_shape[1])
    out = torch.empty((bs, nv, 3, H, W), dtype=torch.float32, device=device)
    if batch.get("undistort") is not None:
        und = batch["undistort"]
        cache = _map_cache(device)
        views = [frames[v][b] for b in range(bs) for v in range(nv)]        # view n = b * NV + v: the (B, NV) order of the output
        views_maps = [cache.get(und[v][b]) for b in range(bs) for v in range(nv)]
        desc, regions, off = img.undistort_descriptors(views, bboxes.reshape(n, 4), views_maps)
        dev, head = _upload(desc, regions, off, device)
        with torch.cuda.device(device):
            lut = img.normalize_lut(device) if norm_image else None
            img.launch_undistort_crop_resize(dev[head:], dev[:head].view(torch.int64).view(n, img.UNDIST_DESC_FIELDS), desc, cache.arena,
                                             (H, W), lut, out.view(n, 3, H, W))
        return (out,) + _targets(batch, device)
    desc = np.zeros((n, img.DESC_FIELDS), np.int64)
    regions = []
    off = 0
    for b in range(bs):                      # view n = b * NV + v: the (B, NV) order of the output
        for v in range(nv):
            f = frames[v][b]
            h, w = f.shape[:2]
            l, u, r, lo = (int(x) for x in bboxes[b, v])
            x0, x1, y0, y1 = min(max(l, 0), w), min(max(r, 0), w), min(max(u, 0), h), min(max(lo, 0), h)
            x1, y1 = max(x1, x0), max(y1, y0)
            reg = f[y0:y1, x0:x1]
            desc[b * nv + v] = (off, y1 - y0, x1 - x0, 3 * (x1 - x0), l - x0, u - y0, r - x0, lo - y0)
            regions.append(reg)
            off += reg.size
    dev, head = _upload(desc, regions, off, device)
    with torch.cuda.device(device):
        lut = img.normalize_lut(device) if norm_image else None
        img.launch_crop_resize(dev[head:], dev[:head].view(torch.int64).view(n, img.DESC_FIELDS), desc, (H, W), lut, out.view(n, 3, H, W))
    return (out,) + _targets(batch, device)


def ragged_batch(images, proj_matricies, batch):
    """A padded (B, NV, ...) batch with batch["view_mask"] -> its ragged form (images_r, proj_r, batch_r): the valid views of every sample, sample 0's first.
    images (B,NV,3,H,W) -> (T,3,H,W); proj_matricies (B,NV,3,4) or None -> (T,3,4) or None; batch["cameras"] (cameras[v][b], as the models take them)
    -> a flat list of T cameras in the same order; batch_r["view_counts"] holds the B counts and has no "view_mask"; every other key is passed on.
    Pure indexing: it works on CPU tensors and on device tensors alike, and copies nothing but the gathered rows.  Without a view_mask every view is
    valid (the padded batch reshaped)."""
    from mvn.utils import op
    B, NV = images.shape[:2]
    mask = batch.get("view_mask")
    m = np.ones((B, NV), np.uint8) if mask is None else op.view_mask_host(mask, B, NV, min_valid=1)
    rows = np.flatnonzero(m.reshape(-1))
    idx = torch.from_numpy(rows.astype(np.int64)).to(images.device)
    out = {k: v for k, v in batch.items() if k != "view_mask"}
    out["view_counts"] = [int(n) for n in m.sum(axis=1)]
    if batch.get("cameras") is not None:
        cams = batch["cameras"]
        out["cameras"] = [cams[int(r) % NV][int(r) // NV] for r in rows]
    images_r = images.reshape((B * NV,) + tuple(images.shape[2:])).index_select(0, idx)
    proj_r = None
    if proj_matricies is not None:
        proj_r = proj_matricies.reshape(B * NV, 3, 4).index_select(0, idx.to(proj_matricies.device))
    return images_r, proj_r, out


def _upload(desc, regions, off, device):
    """descriptors + the pixel regions they point at (desc[:, 0] = byte offset of each region after the descriptors) -> one pinned
    block of the staging ring and one asynchronous H2D copy.  Returns (device uint8 tensor, byte length of the descriptors)."""
    head = desc.nbytes
    total = head + off
    cap = 1 << max(20, (total - 1).bit_length())          # power-of-two blocks: one ring serves batches of similar byte counts
    ring = _ring((cap,), torch.uint8)
    stage = ring.acquire()
    host = stage.numpy()
    host[:head] = desc.view(np.uint8).reshape(-1)
    for i, reg in enumerate(regions):
        if reg.size:
            o = head + int(desc[i, 0])
            host[o:o + reg.size].reshape(reg.shape)[...] = reg
    dev = stage[:total].to(device, non_blocking=True)
    ring.commit(torch.cuda.current_stream(device))
    return dev, head


class DeviceMapCache:
    """Undistortion maps of every camera seen so far, resident on one device: one int16 arena of mvn/utils/img.py:device_map blocks
    (8 bytes per frame pixel, about 8 MB for a 1000 x 1000 camera), keyed by (K, dist, frame h, w).  A new camera builds its maps on
    the host (img.undistort_maps), appends them to the arena (a reallocation on the current stream, so launches already queued keep
    reading the old arena) and keeps map1 and its monotonicity for the source windows."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.arena = None
        self.entries = {}

    def get(self, key):
        """key (K, dist, (h, w)) -> (map1, monotone, byte offset in the arena, row pitch in entries)."""
        from mvn.utils import img
        K, dist, (h, w) = key
        K, dist = np.asarray(K, dtype=np.float32), np.asarray(dist, dtype=np.float32).reshape(-1)
        k = (K.tobytes(), dist.tobytes(), int(h), int(w))
        if k not in self.entries:
            maps = img.undistort_maps(K, dist, int(h), int(w))
            block = torch.from_numpy(img.device_map(maps).reshape(-1)).to(self.device)
            off = 0 if self.arena is None else self.arena.numel() * 2
            self.arena = block if self.arena is None else torch.cat([self.arena, block])
            self.entries[k] = (maps[0], img.map_is_monotone(maps[0]), off, int(w))
        return self.entries[k]


_map_caches = {}


def _map_cache(device):
    device = torch.device(device)
    if device not in _map_caches:
        _map_caches[device] = DeviceMapCache(device)
    return _map_caches[device]
