"""Functional ops of the volumetric path with the reference's names and signatures
(mvn/utils/op.py of the reference), executed by liblt_hip.so.

Public tensors keep the reference's layouts (heatmaps B,NV,C,h,w; volumes B,C,V,V,V); internally the
kernels are channels-last, so a channels-last-strided input (what our own networks produce) is consumed
without a copy, and outputs are returned as permuted views of channels-last storage."""
import ctypes

import numpy as np
import torch

import lt_hip as H
from mvn.utils.volumetric import AlgKeypointStats, KeypointStats

# workspace of lt_unproject_bwd's deterministic gather: at most this much (or one sample's share, if that is more); with less than the whole
# batch's worth the entry point walks the batch in chunks.  One constant for the autograd path here and the recorded training step.
UNPROJECT_BWD_WORKSPACE_CAP = 2 << 30

_METHODS = ("sum", "max", "softmax", "conf", "conf_norm")


def _as_channels_last(x, n_lead):
    """x: (*lead, C, *spatial) -> contiguous (*lead, *spatial, C) tensor (zero-copy when x already is a
    permuted view of such storage)."""
    nd = x.dim()
    perm = list(range(n_lead)) + list(range(n_lead + 1, nd)) + [n_lead]
    return x.permute(*perm).contiguous()


def build_coord_volumes(base_points, cuboid_side, volume_size, thetas=None, axis=(0, 0, 1), cmu_transfer=False, device="cuda:0"):
    """Per-sample voxel-centre grids (B,V,V,V,3) fp32 -- the loop body of
    VolumetricTriangulationNet.forward (reference mvn/models/triangulation.py:298-339) as one launch.

    base_points: (B,3) array-like (mm), fp64 on the host like the reference; thetas: per-sample rotation
    about ``axis`` through the base point (None = 0).
    """
    from mvn.utils import volumetric
    base = np.asarray(base_points, dtype=np.float64).reshape(-1, 3)
    B = base.shape[0]
    pos = (base - cuboid_side / 2.0).astype(np.float32)
    rot = np.stack([volumetric.get_rotation_matrix(axis, 0.0 if thetas is None else float(thetas[b])) for b in range(B)]).astype(np.float32)
    host = torch.from_numpy(np.concatenate([pos.reshape(-1), base.astype(np.float32).reshape(-1), rot.reshape(-1)]))
    dev = host.to(device)
    out = torch.empty(B, volume_size, volume_size, volume_size, 3, dtype=torch.float32, device=device)
    step = float(np.float32(cuboid_side / (volume_size - 1)))
    H.check(H.lib().lt_coord_volumes(dev.data_ptr(), dev.data_ptr() + 12 * B, dev.data_ptr() + 24 * B, step, B, volume_size,
                                     int(bool(cmu_transfer)), out.data_ptr(), H.cur_stream()), "lt_coord_volumes")
    return out


def view_mask_host(view_mask, B, NV, min_valid=0, what="view_mask"):
    """A (B, NV) validity mask (bool / uint8 / any integer tensor or array, non-zero = valid) as a C-contiguous host uint8 array of 0 / 1.
    ValueError on another shape, or when a sample has fewer than ``min_valid`` valid views (the message names the first such sample)."""
    m = view_mask.detach().cpu().numpy() if torch.is_tensor(view_mask) else np.asarray(view_mask)
    if m.dtype.kind not in "biu":
        raise TypeError("%s must be a bool or integer (B, NV) mask, got dtype %s" % (what, m.dtype))
    if m.shape != (B, NV):
        raise ValueError("%s must have shape (B, NV) = (%d, %d), got %s" % (what, B, NV, tuple(m.shape)))
    m = np.ascontiguousarray((m != 0).astype(np.uint8))
    valid = m.sum(axis=1)
    if (valid < min_valid).any():
        b = int(np.argmax(valid < min_valid))
        raise ValueError("%s: sample %d has %d valid view%s, at least %d needed" % (what, b, int(valid[b]), "" if valid[b] == 1 else "s", min_valid))
    return m


def frame_index_host(frame_index, F, what="frame_index"):
    """The frame of every cuboid (a sequence, an array or a tensor of P >= 1 integers in [0, F), any order) as a C-contiguous host int32 array.
    ValueError for an empty or non-flat list or an index outside [0, F) (the message names the first such entry), TypeError for a non-integer dtype."""
    a = frame_index.detach().cpu().numpy() if torch.is_tensor(frame_index) else np.asarray(frame_index)
    if a.ndim != 1 or a.size == 0:
        raise ValueError("%s must be a flat list of at least one frame index, got shape %s" % (what, tuple(a.shape)))
    if a.dtype.kind not in "iu":
        raise TypeError("%s must hold integers, got dtype %s" % (what, a.dtype))
    bad = (a < 0) | (a >= F)
    if bad.any():
        p = int(np.argmax(bad))
        raise ValueError("%s[%d] = %d is outside the %d frame%s [0, %d)" % (what, p, int(a[p]), F, "" if F == 1 else "s", F))
    return np.ascontiguousarray(a.astype(np.int32))


def view_counts_host(view_counts, T=None, min_views=1, what="view_counts"):
    """The views of every sample of a ragged batch (a sequence, an array or a tensor of B >= 1 integers) -> (counts, view_base, NVcap): the counts as a host
    int32 array, their exclusive prefix sum (B + 1 int32, what the ragged kernels read) and the smallest of 4, 8, 32 that holds the largest count (the
    kernel instantiation).  ValueError for an empty or non-flat list, a count below ``min_views`` or above 32 (the message names the first such sample)
    or counts that do not sum to ``T``; TypeError for a non-integer dtype."""
    a = view_counts.detach().cpu().numpy() if torch.is_tensor(view_counts) else np.asarray(view_counts)
    if a.ndim != 1 or a.size == 0:
        raise ValueError("%s must be a flat list of at least one view count, got shape %s" % (what, tuple(a.shape)))
    if a.dtype.kind not in "iu":
        raise TypeError("%s must hold integers, got dtype %s" % (what, a.dtype))
    bad = (a < min_views) | (a > 32)
    if bad.any():
        b = int(np.argmax(bad))
        raise ValueError("%s: sample %d has %d view%s, %d to 32 allowed" % (what, b, int(a[b]), "" if a[b] == 1 else "s", min_views))
    total = int(a.sum())
    if T is not None and total != T:
        raise ValueError("%s sums to %d views over %d samples, the batch holds %d" % (what, total, a.size, T))
    counts = np.ascontiguousarray(a.astype(np.int32))
    base = np.zeros(counts.size + 1, np.int32)
    np.cumsum(counts, out=base[1:])
    top = int(counts.max())
    return counts, base, (4 if top <= 4 else 8 if top <= 8 else 32)


def _view_mask_device(view_mask, B, NV, device):
    """The mask as a (B, NV) uint8 device tensor for the masked entry points (a device tensor of the right form is used as it is)."""
    if torch.is_tensor(view_mask) and view_mask.is_cuda:
        if tuple(view_mask.shape) != (B, NV):
            raise ValueError("view_mask must have shape (B, NV) = (%d, %d), got %s" % (B, NV, tuple(view_mask.shape)))
        if view_mask.dtype == torch.uint8:
            return view_mask.to(device).contiguous()
        if view_mask.dtype == torch.bool or not view_mask.dtype.is_floating_point:
            return (view_mask != 0).to(device, torch.uint8).contiguous()
        raise TypeError("view_mask must be a bool or integer (B, NV) mask, got dtype %s" % view_mask.dtype)
    return torch.from_numpy(view_mask_host(view_mask, B, NV)).to(device)


def _unproject_desc(feats_cl, P, cv, conf, method, mask=None, frame_of=None, view_base=None, nvcap=None):
    """The coordinate-form lt_unproject_desc of feats_cl (B,NV,h,w,C) contiguous channels-last over cv (B,v0,v1,v2,3); the variant is which of the rest is
    given.  mask: (B,NV) uint8 device tensor.  frame_of: (P,) int32 device tensor -- cv holds P cuboids, each over the views of its frame of the B; the mask,
    if any, is per frame.  view_base: (B + 1,) int32 device tensor -- feats_cl is (T,h,w,C) over the views of all samples, ``nvcap`` the most a sample has."""
    h, w, Cc = feats_cl.shape[-3:]
    v0, v1, v2 = cv.shape[1:4]
    return H.UnprojectDesc(dtype=H.dtype_code(feats_cl.dtype), feats=feats_cl.data_ptr(), proj=P.data_ptr(), coords=cv.data_ptr(), conf=H.ptr(conf),
                           view_mask=H.ptr(mask), frame_of=H.ptr(frame_of), F=feats_cl.shape[0], view_base=H.ptr(view_base), T=feats_cl.shape[0],
                           B=cv.shape[0], NV=feats_cl.shape[1] if view_base is None else nvcap, C=Cc, h=h, w=w, v0=v0, v1=v1, v2=v2,
                           agg=H.AGG["conf"] if conf is not None else H.AGG[method])


def _unproject_launch(feats_cl, P, cv, conf, method, mask=None, frame_of=None, view_base=None, nvcap=None):
    """_unproject_desc's arguments -> (B,v0,v1,v2,C) channels-last, same dtype (lt_unproject_desc_fwd)."""
    d = _unproject_desc(feats_cl, P, cv, conf, method, mask, frame_of, view_base, nvcap)
    out = torch.empty(tuple(cv.shape[:4]) + (d.C,), dtype=feats_cl.dtype, device=feats_cl.device)
    H.check(H.lib().lt_unproject_desc_fwd(ctypes.byref(d), out.data_ptr(), H.cur_stream()), H.unproject_entry(d))
    return out


def unproject_bwd_workspace(desc, chunk=None, cap=None):
    """Bytes of lt_unproject_desc_bwd's workspace for the desc.B samples (cuboids) walked ``chunk`` at a time (None: all at once; 1: the least the entry
    takes), as lt_unproject_desc_bwd_workspace states them.  cap: the largest chunk whose workspace stays within ``cap`` bytes instead (at least one).
    0 where the gather does not take C."""
    query = lambda items: H.lib().lt_unproject_desc_bwd_workspace(ctypes.byref(desc), items)
    n, one = desc.B, query(1)
    if one == 0:
        return 0
    if cap is not None:
        share = query(2) - one if n > 1 else one          # what every further item adds; the rest is there once
        chunk = max(1, min(n, (cap - (one - share)) // share))
    return query(n if chunk is None else min(n, int(chunk)))


_ANY_FRAME = (H.i32 * 1)()          # indexed_bwd_workspace: a host-only query reads no pointer, it only asks whether frame_of is set


def indexed_bwd_workspace(P, NV, C, v0, v1, v2, chunk=None, cap=None):
    """Bytes of lt_unproject_indexed_bwd's workspace for P cuboids walked ``chunk`` cuboids at a time (None: all at once, lt_unproject_indexed_bwd_workspace
    itself; 1: the least the entry takes): the fp64 confidence partials of ALL P cuboids plus ``chunk`` cuboids' shares of the rest (include/lt_hip.h).
    cap: the largest chunk whose workspace stays within ``cap`` bytes instead (at least one cuboid).  0 where the gather does not take C."""
    return unproject_bwd_workspace(H.UnprojectDesc(frame_of=ctypes.addressof(_ANY_FRAME), B=P, NV=NV, C=C, v0=v0, v1=v1, v2=v2), chunk, cap)


class _UnprojectFn(torch.autograd.Function):
    """lt_unproject_desc_fwd / lt_unproject_desc_bwd as one autograd node: what autograd builds in the reference from grid_sample, the in-place depth
    mask and the view aggregation (op.py:113-162).  Gradients reach the heatmaps and (conf modes) the confidences; projections and coordinates get none,
    exactly as in the reference (they do not require grad there).  mask: a (B,NV) uint8 device tensor makes it the node over every sample's valid views
    alone (masked views get zero gradients).  fof: a (P,) int32 device tensor of frames makes it the node of several cuboids per frame -- what autograd
    derives on heatmaps[fof], proj[fof], conf[fof] without the gathered copies: every frame's heatmaps and confidences get the sum of its cuboids'
    gradients, a frame without a cuboid zeros; the mask is then (F,NV), per frame."""

    @staticmethod
    def forward(ctx, heatmaps, P, cv, conf, method, mask=None, fof=None):
        feats = _as_channels_last(heatmaps, 2)
        out = _unproject_launch(feats, P, cv, conf, method, mask, fof)
        ctx.save_for_backward(feats, P, cv, conf if conf is not None else torch.empty(0, device=feats.device))
        ctx.method, ctx.has_conf, ctx.mask, ctx.fof = method, conf is not None, mask, fof
        return out.permute(0, 4, 1, 2, 3)

    @staticmethod
    def backward(ctx, grad_out):
        feats, P, cv, conf = ctx.saved_tensors
        conf = conf if ctx.has_conf else None
        g = grad_out.permute(0, 2, 3, 4, 1).float().contiguous()               # (B, v0, v1, v2, C) channels-last fp32
        gfeats = torch.empty(feats.shape, dtype=torch.float32, device=feats.device)      # written completely by the gather, empty frames included
        gconf = torch.empty_like(conf) if conf is not None else None
        d = _unproject_desc(feats, P, cv, conf, ctx.method, ctx.mask, ctx.fof)
        # deterministic gather: workspace for as many samples (cuboids) as fit 2 GiB at a time (the entry walks them in chunks, same bits)
        ws = torch.empty(max(16, unproject_bwd_workspace(d, cap=UNPROJECT_BWD_WORKSPACE_CAP)), dtype=torch.uint8, device=feats.device)
        H.check(H.lib().lt_unproject_desc_bwd(ctypes.byref(d), g.data_ptr(), gfeats.data_ptr(), H.ptr(gconf), ws.data_ptr(), ws.numel(), H.cur_stream()),
                H.unproject_entry(d, bwd=True))
        return gfeats.permute(0, 1, 4, 2, 3).to(feats.dtype), None, None, gconf, None, None, None


def unproject_heatmaps(heatmaps, proj_matricies, coord_volumes, volume_aggregation_method="sum", vol_confidences=None, view_mask=None,
                       masked_backward=False, frame_index=None, indexed_backward=False, view_counts=None):
    """heatmaps (B,NV,C,h,w), proj_matricies (B,NV,3,4), coord_volumes (B,V0,V1,V2,3),
    vol_confidences (B,NV,C) for 'conf*' -> volumes (B,C,V0,V1,V2).  Reference: op.py:99-166.  Differentiable with respect to the
    heatmaps and the confidences (lt_unproject_bwd) whenever one of them requires grad.

    view_mask: optional (B,NV) bool / uint8 tensor or array, non-zero = the view is there.  Sample b then gets what this function gives for its
    valid views alone (lt_unproject_masked_fwd: masked views are never read; a sample without a valid view gets zeros).  Inference only by
    default: with inputs that require grad it raises NotImplementedError.  None takes exactly the unmasked path.

    masked_backward=True opts into the differentiable masked op (lt_unproject_masked_bwd): what autograd derives for this function called on each
    sample's valid views alone -- a masked view's heatmaps and confidences get exactly zero gradient, conf_norm's normaliser is differentiated
    over the valid views.  Gather path only (C a power of two <= 64); ignored without a view_mask.

    frame_index: several cuboids per frame (lt_unproject_indexed_fwd).  heatmaps (F,NV,C,h,w), proj_matricies (F,NV,3,4), vol_confidences (F,NV,C) and
    view_mask (F,NV) are per FRAME, coord_volumes (P,V0,V1,V2,3) per cuboid; frame_index holds the P frames of the cuboids (a sequence, an array or a
    tensor of integers in [0, F), any order; checked on the host when it lives there -- a device tensor is used as it is, and the kernel clamps what
    it reads) -> volumes (P,C,V0,V1,V2), bit-identical to this function on the inputs gathered by frame_index, without the copies.  Inference only
    by default: NotImplementedError when an input requires grad.  None takes exactly the path without it.

    indexed_backward=True opts into the differentiable indexed op (lt_unproject_indexed_bwd): what autograd derives for this function on the inputs
    gathered by frame_index -- a frame's heatmaps and confidences get the sum of its cuboids' gradients, a frame without a cuboid zeros.  Gather path
    only (C a power of two <= 64); ignored without a frame_index.  A view_mask then needs masked_backward=True as well.

    view_counts: a ragged batch (lt_unproject_ragged_fwd), samples with different numbers of views and no padding.  heatmaps (T,C,h,w), proj_matricies
    (T,3,4) and vol_confidences (T,C) hold the views of all samples, sample 0's first; view_counts the B counts (1..32 each, summing to T; a sequence, an
    array or a tensor); coord_volumes (B,V0,V1,V2,3) -> volumes (B,C,V0,V1,V2): sample b is this function on its own views alone.  Inference only:
    NotImplementedError when an input requires grad, and together with view_mask (drop the view from the batch instead) or frame_index."""
    if volume_aggregation_method not in _METHODS:
        raise ValueError("Unknown volume_aggregation_method: {}".format(volume_aggregation_method))
    if view_counts is not None:
        if view_mask is not None:
            raise NotImplementedError("unproject_heatmaps: view_counts with view_mask; drop the missing views from the ragged batch instead of masking them")
        if frame_index is not None:
            raise NotImplementedError("unproject_heatmaps: view_counts with frame_index; gather each cuboid's views into the ragged batch instead")
        if torch.is_grad_enabled() and (heatmaps.requires_grad or (torch.is_tensor(vol_confidences) and vol_confidences.requires_grad)):
            raise NotImplementedError("unproject_heatmaps: view_counts is inference only (no ragged backward); call it under torch.no_grad(), or pad the "
                                      "batch and train with view_mask and masked_backward=True")
        if heatmaps.dim() != 4:
            raise ValueError("unproject_heatmaps: with view_counts the heatmaps are (T, C, h, w), got %s" % (tuple(heatmaps.shape),))
        counts, base, nvcap = view_counts_host(view_counts, heatmaps.shape[0])
        if coord_volumes.shape[0] != counts.size:
            raise ValueError("view_counts has %d entries, coord_volumes holds %d samples" % (counts.size, coord_volumes.shape[0]))
        if tuple(proj_matricies.shape) != (heatmaps.shape[0], 3, 4):
            raise ValueError("unproject_heatmaps: with view_counts proj_matricies are (T, 3, 4) = (%d, 3, 4), got %s" % (heatmaps.shape[0], tuple(proj_matricies.shape)))
        H.require_gpu(heatmaps, "heatmaps")
        H.dtype_code(heatmaps.dtype)
        P = proj_matricies.to(heatmaps.device, torch.float32).contiguous()
        cv = coord_volumes.to(heatmaps.device, torch.float32).contiguous()
        conf = vol_confidences.to(heatmaps.device, torch.float32).contiguous() if volume_aggregation_method.startswith("conf") else None
        vb = torch.from_numpy(base).to(heatmaps.device)
        return _unproject_launch(_as_channels_last(heatmaps, 1), P, cv, conf, volume_aggregation_method, view_base=vb, nvcap=nvcap).permute(0, 4, 1, 2, 3)
    indexed_grad = frame_index is not None and torch.is_grad_enabled() and (heatmaps.requires_grad or
                                                                              (torch.is_tensor(vol_confidences) and vol_confidences.requires_grad))
    if indexed_grad and not indexed_backward:
        raise NotImplementedError("unproject_heatmaps: frame_index is inference only (no indexed backward); call it under torch.no_grad()")
    if indexed_grad and view_mask is not None and not masked_backward:
        raise NotImplementedError("unproject_heatmaps: view_mask is inference only (no masked backward); call it under torch.no_grad()")
    H.require_gpu(heatmaps, "heatmaps")
    H.dtype_code(heatmaps.dtype)
    P = proj_matricies.to(heatmaps.device, torch.float32).contiguous()
    cv = coord_volumes.to(heatmaps.device, torch.float32).contiguous()
    conf = None
    if volume_aggregation_method.startswith("conf"):
        conf = vol_confidences.to(heatmaps.device, torch.float32).contiguous()
    if frame_index is not None:
        F, NV = heatmaps.shape[:2]
        if torch.is_tensor(frame_index) and frame_index.is_cuda:
            if frame_index.dim() != 1 or frame_index.numel() == 0 or frame_index.dtype.is_floating_point or frame_index.dtype == torch.bool:
                raise ValueError("frame_index must be a flat list of at least one integer frame index, got %s %s" % (frame_index.dtype, tuple(frame_index.shape)))
            fof = frame_index.to(heatmaps.device, torch.int32).contiguous()
        else:
            fof = torch.from_numpy(frame_index_host(frame_index, F)).to(heatmaps.device)
        if cv.shape[0] != fof.numel():
            raise ValueError("frame_index has %d entries, coord_volumes holds %d cuboids" % (fof.numel(), cv.shape[0]))
        mask = None if view_mask is None else _view_mask_device(view_mask, F, NV, heatmaps.device)
        if indexed_grad and (heatmaps.requires_grad or (conf is not None and vol_confidences.requires_grad)):
            return _UnprojectFn.apply(heatmaps, P, cv, conf, volume_aggregation_method, mask, fof)
        return _unproject_launch(_as_channels_last(heatmaps, 2), P, cv, conf, volume_aggregation_method, mask, fof).permute(0, 4, 1, 2, 3)
    if view_mask is not None:
        needs_grad = torch.is_grad_enabled() and (heatmaps.requires_grad or (conf is not None and vol_confidences.requires_grad))
        if needs_grad and not masked_backward:
            raise NotImplementedError("unproject_heatmaps: view_mask is inference only (no masked backward); call it under torch.no_grad()")
        mask = _view_mask_device(view_mask, heatmaps.shape[0], heatmaps.shape[1], heatmaps.device)
        if needs_grad:
            return _UnprojectFn.apply(heatmaps, P, cv, conf, volume_aggregation_method, mask)
        return _unproject_launch(_as_channels_last(heatmaps, 2), P, cv, conf, volume_aggregation_method, mask).permute(0, 4, 1, 2, 3)
    if torch.is_grad_enabled() and (heatmaps.requires_grad or (conf is not None and vol_confidences.requires_grad)):
        return _UnprojectFn.apply(heatmaps, P, cv, conf, volume_aggregation_method)
    return _unproject_launch(_as_channels_last(heatmaps, 2), P, cv, conf, volume_aggregation_method).permute(0, 4, 1, 2, 3)


def keypoint_stats_from_records(records, peak_index):
    """The (B,J,8) records {peak, mass, cxx, cxy, cxz, cyy, cyz, czz} and (B,J) peak voxels of lt_softargmax3d_stats_fwd as a KeypointStats."""
    cov = records[..., [2, 3, 4, 3, 5, 6, 4, 6, 7]].reshape(records.shape[:-1] + (3, 3))
    return KeypointStats(records[..., 0], peak_index, records[..., 1], cov)


def _softargmax3d_launch(volumes, cv, softmax, with_stats=False):
    B, J = volumes.shape[:2]
    nvox = int(np.prod(volumes.shape[2:]))
    cl = volumes.permute(0, 2, 3, 4, 1).is_contiguous() and not volumes.is_contiguous()
    lg = (volumes.permute(0, 2, 3, 4, 1) if cl else volumes).float().contiguous()
    kp = torch.empty(B, J, 3, dtype=torch.float32, device=volumes.device)
    probs = torch.empty((B, J) + tuple(volumes.shape[2:]), dtype=torch.float32, device=volumes.device)
    lib = H.lib()
    if with_stats:          # the same launches with the statistics out of the probabilities pass: kp and probs keep their bits
        rec = torch.empty(B, J, 8, dtype=torch.float32, device=volumes.device)
        idx = torch.empty(B, J, dtype=torch.int32, device=volumes.device)
        ws = torch.empty(max(1, lib.lt_softargmax3d_stats_workspace(B, J, nvox)), dtype=torch.uint8, device=volumes.device)
        H.check(lib.lt_softargmax3d_stats_fwd(lg.data_ptr(), cv.data_ptr(), 1.0, int(bool(softmax)), int(cl), J, kp.data_ptr(), probs.data_ptr(), rec.data_ptr(),
                                              idx.data_ptr(), B, J, nvox, ws.data_ptr(), H.cur_stream()), "lt_softargmax3d_stats_fwd")
        return kp, probs, keypoint_stats_from_records(rec, idx)
    ws = torch.empty(max(1, lib.lt_softargmax3d_workspace(B, J, nvox)), dtype=torch.uint8, device=volumes.device)
    H.check(lib.lt_softargmax3d_fwd(lg.data_ptr(), cv.data_ptr(), 1.0, int(bool(softmax)), int(cl), J, kp.data_ptr(), probs.data_ptr(),
                                    B, J, nvox, ws.data_ptr(), H.cur_stream()), "lt_softargmax3d_fwd")
    return kp, probs


class _SoftArgmax3dFn(torch.autograd.Function):
    """lt_softargmax3d_fwd / _bwd as one node with TWO outputs (coordinates, probabilities): a dense gradient on the
    probabilities goes into the same kernel (lt_softargmax3d_bwd_dense); VolumetricCELoss (mvn/models/loss.py) instead hands over its
    one-voxel-per-joint gradient in sparse form (``sparse_prob_grad``), so no (B,J,V^3) gradient tensor is ever materialised."""

    @staticmethod
    def forward(ctx, volumes, cv, softmax, stats_out=None):
        # stats_out (integrate_tensor_3d_with_stats): a list that receives the KeypointStats of this forward; they are no outputs of the node (no gradient)
        if stats_out is None:
            kp, probs = _softargmax3d_launch(volumes, cv, softmax)
        else:
            kp, probs, st = _softargmax3d_launch(volumes, cv, softmax, with_stats=True)
            stats_out.append(st)
        ctx.save_for_backward(probs, cv, kp)
        ctx.softmax, ctx.in_dtype = bool(softmax), volumes.dtype
        return kp, probs

    @staticmethod
    def backward(ctx, g_kp, g_probs):
        probs, cv, kp = ctx.saved_tensors
        B, J = probs.shape[:2]
        nvox = probs[0, 0].numel()
        g_kp = torch.zeros_like(kp) if g_kp is None else g_kp.float().contiguous()
        # sparse gradients on the probabilities left here by consumers that ran before us (VolumetricCELoss: one voxel per (b, j))
        sparse = getattr(ctx, "_lt_sparse_prob_grads", [])
        idx = val = None
        if len(sparse) == 1:
            idx, val = sparse[0]
        dense = None
        if len(sparse) > 1:       # several sparse consumers: scatter them into one dense gradient (rare)
            dense = torch.zeros(B, J, nvox, dtype=torch.float32, device=probs.device)
            for i2, v2 in sparse:
                dense.scatter_add_(2, i2.long()[..., None], v2[..., None])
            dense = dense.reshape(probs.shape)
        if g_probs is not None and not is_sparse_placeholder(ctx, g_probs):   # a real dense gradient on the returned volumes (a uniform one -- volumes.sum() -- included)
            dense = g_probs.float() if dense is None else dense + g_probs.float()
        ws = None
        if dense is not None:     # a_i += gp_i inside the kernel (softmax: minus <p, gp>, reduced per joint into the workspace first)
            dense = dense.contiguous()
            ws = torch.empty(B * J, dtype=torch.float32, device=probs.device)
        gl = torch.empty_like(probs)
        H.check(H.lib().lt_softargmax3d_bwd_dense(probs.data_ptr(), cv.data_ptr(), kp.data_ptr(), g_kp.data_ptr(), H.ptr(idx), H.ptr(val), H.ptr(dense), H.ptr(ws), 1.0,
                                                  int(ctx.softmax), 0, gl.data_ptr(), B, J, nvox, H.cur_stream()), "lt_softargmax3d_bwd")
        return gl.to(ctx.in_dtype), None, None, None


def is_sparse_placeholder(node, g):
    """True when ``g`` is the all-zero stride-0 tensor ``sparse_prob_grad`` returned for a gradient it left on ``node`` in sparse form.  Recognised by the
    STORAGE of the placeholder: any other zero-stride tensor -- the expanded ones of ``volumes.sum()``, a uniform ``volumes.mean()`` -- is a real dense
    gradient (with ``volume_softmax=False`` a uniform gradient on the ReLU volumes is not zero after the backward)."""
    if g.stride() != (0,) * g.dim():
        return False
    return any(z.data_ptr() == g.data_ptr() for z in getattr(node, "_lt_placeholders", []))


def sparse_prob_grad(volumes, idx, val):
    """Hands a one-voxel-per-(sample, joint) gradient on ``volumes`` -- the probabilities returned by
    integrate_tensor_3d_with_coordinates -- to the node that produced them.  Returns the tensor the consumer's backward
    should return for ``volumes``: an all-zero stride-0 view when the producer is our soft-argmax node (which then applies the sparse
    part itself inside lt_softargmax3d_bwd), else the dense scatter."""
    node = volumes.grad_fn
    if isinstance(node, _SoftArgmax3dFn._backward_cls) or getattr(node, "_lt_accepts_sparse_prob_grads", False):
        if not hasattr(node, "_lt_sparse_prob_grads"):
            node._lt_sparse_prob_grads = []
        node._lt_sparse_prob_grads.append((idx, val))
        zero = torch.zeros((), dtype=volumes.dtype, device=volumes.device)
        if not hasattr(node, "_lt_placeholders"):
            node._lt_placeholders = []
        node._lt_placeholders.append(zero)          # kept alive on the node: the placeholder is recognised by its storage, not by its strides
        return zero.expand(volumes.shape)
    B, J = volumes.shape[:2]
    dense = torch.zeros(B, J, volumes[0, 0].numel(), dtype=torch.float32, device=volumes.device)
    dense.scatter_(2, idx.long()[..., None], val[..., None])
    return dense.reshape(volumes.shape).to(volumes.dtype)


def integrate_tensor_3d_with_coordinates(volumes, coord_volumes, softmax=True):
    """volumes (B,J,V0,V1,V2) logits, coord_volumes (B,V0,V1,V2,3) -> (coordinates (B,J,3), volumes after
    softmax / ReLU).  Reference: op.py:84-96.  Differentiable with respect to the logits (lt_softargmax3d_bwd)."""
    H.require_gpu(volumes, "volumes")
    cv = coord_volumes.to(volumes.device, torch.float32).contiguous()
    if torch.is_grad_enabled() and volumes.requires_grad:
        return _SoftArgmax3dFn.apply(volumes, cv, softmax)
    return _softargmax3d_launch(volumes, cv, softmax)


def integrate_tensor_3d_with_stats(volumes, coord_volumes, softmax=True):
    """integrate_tensor_3d_with_coordinates plus the per-joint statistics of the 3D heatmaps, out of the same pass that writes the probabilities
    (lt_softargmax3d_stats_fwd).  Returns (coordinates, volumes, stats): the first two are bit for bit what integrate_tensor_3d_with_coordinates returns
    and differentiable in the same way; ``stats`` is a KeypointStats (peak, peak_index, mass, covariance about the returned joint) without a gradient.
    The definitions in numpy fp64: mvn.utils.volumetric.keypoint_stats."""
    H.require_gpu(volumes, "volumes")
    cv = coord_volumes.to(volumes.device, torch.float32).contiguous()
    if torch.is_grad_enabled() and volumes.requires_grad:
        out = []
        kp, probs = _SoftArgmax3dFn.apply(volumes, cv, softmax, out)
        return kp, probs, out[0]
    return _softargmax3d_launch(volumes, cv, softmax, with_stats=True)


def batchnorm_batch_stats(x, running_mean=None, running_var=None, momentum=0.1):
    """Training-mode BatchNorm statistics of x (N,C,*spatial; fp32 or bf16): per-channel batch mean and BIASED variance (what
    F.batch_norm normalises with when training=True), fp64 accumulation (lt_bn_stats_fwd); running_mean / running_var (fp32, on the
    GPU) are updated in place the way torch does (momentum, unbiased variance).  Channels-last inputs are consumed without a copy."""
    H.require_gpu(x, "x")
    xc = _as_channels_last(x, 1)
    Cc = xc.shape[-1]
    rows = xc.numel() // Cc
    mean = torch.empty(Cc, dtype=torch.float32, device=x.device)
    var = torch.empty(Cc, dtype=torch.float32, device=x.device)
    lib = H.lib()
    ws = torch.empty(max(16, lib.lt_bn_stats_workspace(rows, Cc)), dtype=torch.uint8, device=x.device)
    if running_mean is not None:
        assert running_mean.is_cuda and running_mean.dtype == torch.float32 and running_mean.is_contiguous()
        assert running_var.is_cuda and running_var.dtype == torch.float32 and running_var.is_contiguous()
    H.check(lib.lt_bn_stats_fwd(H.dtype_code(xc.dtype), xc.data_ptr(), rows, Cc, mean.data_ptr(), var.data_ptr(), H.ptr(running_mean),
                                H.ptr(running_var), float(momentum), ws.data_ptr(), H.cur_stream()), "lt_bn_stats_fwd")
    return mean, var


def heatmap_stats_from_records(records, peak_index):
    """The (..., 5) records {peak, mass, cxx, cxy, cyy} and (...) peak indices of lt_softargmax2d_stats_fwd as (peak, peak_index, mass, covariance (..., 2, 2))."""
    cov = records[..., [2, 3, 3, 4]].reshape(records.shape[:-1] + (2, 2))
    return records[..., 0], peak_index, records[..., 1], cov


def alg_keypoint_stats_from_records(records, peak_index, cov2d_img, reproj_err, cov3d):
    """The buffers of lt_softargmax2d_stats_fwd (records (B,NV,J,5), peak_index (B,NV,J)) and lt_alg_tail_stats_fwd (cov2d_img (B,NV,J,3), reproj_err
    (B,NV,J), cov3d (B,J,6)) as an AlgKeypointStats."""
    c2 = cov2d_img[..., [0, 1, 1, 2]].reshape(cov2d_img.shape[:-1] + (2, 2))
    c3 = cov3d[..., [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(cov3d.shape[:-1] + (3, 3))
    return AlgKeypointStats(records[..., 0], peak_index, records[..., 1], c2, reproj_err, c3)


def _softargmax2d_launch(heatmaps, softmax, with_stats=False):
    N, J, h, w = heatmaps.shape
    hm = heatmaps.float().contiguous()
    coords = torch.empty(N, J, 2, dtype=torch.float32, device=hm.device)
    probs = torch.empty_like(hm)
    if with_stats:          # the same kernel with the statistics out of its third pass: coords and probs keep their bits
        rec = torch.empty(N, J, 5, dtype=torch.float32, device=hm.device)
        idx = torch.empty(N, J, dtype=torch.int32, device=hm.device)
        H.check(H.lib().lt_softargmax2d_stats_fwd(hm.data_ptr(), 1.0, int(bool(softmax)), coords.data_ptr(), probs.data_ptr(), rec.data_ptr(), idx.data_ptr(), N * J,
                                                  h, w, H.cur_stream()), "lt_softargmax2d_stats_fwd")
        return coords, probs, heatmap_stats_from_records(rec, idx)
    H.check(H.lib().lt_softargmax2d_fwd(hm.data_ptr(), 1.0, int(bool(softmax)), coords.data_ptr(), probs.data_ptr(), N * J, h, w, H.cur_stream()),
            "lt_softargmax2d_fwd")
    return coords, probs


class _SoftArgmax2dFn(torch.autograd.Function):
    """lt_softargmax2d_fwd / _bwd as one node with TWO differentiable outputs (coordinates, heatmaps after softmax / ReLU).  A step whose loss touches
    the coordinates alone (the algebraic model's training, train.py:189-236) takes lt_softargmax2d_bwd as it always did -- the same launch, the same
    bits; a gradient on the returned heatmaps (an auxiliary 2D heatmap loss) goes through lt_softargmax2d_bwd_full, with or without one on the
    coordinates."""

    @staticmethod
    def forward(ctx, heatmaps, softmax, stats_out=None):
        ctx.set_materialize_grads(False)              # an unused output arrives as None in backward: that is how the old entry is chosen
        # stats_out (integrate_tensor_2d_with_stats): a list that receives the statistics of this forward; they are no outputs of the node (no gradient)
        if stats_out is None:
            coords, probs = _softargmax2d_launch(heatmaps, softmax)
        else:
            coords, probs, st = _softargmax2d_launch(heatmaps, softmax, with_stats=True)
            stats_out.append(st)
        ctx.save_for_backward(coords, probs)
        ctx.softmax, ctx.in_dtype = bool(softmax), heatmaps.dtype
        return coords, probs

    @staticmethod
    def backward(ctx, g_coords, g_probs):
        coords, probs = ctx.saved_tensors
        if g_coords is None and g_probs is None:
            return None, None, None
        N, J, h, w = probs.shape
        g = None if g_coords is None else g_coords.float().contiguous()
        ghm = torch.empty_like(probs)
        if g_probs is None:          # no gradient on the heatmaps: the entry and the launch of every step recorded before they were differentiable
            H.check(H.lib().lt_softargmax2d_bwd(probs.data_ptr(), coords.data_ptr(), g.data_ptr(), 1.0, int(ctx.softmax), ghm.data_ptr(), N * J, h, w,
                                                H.cur_stream()), "lt_softargmax2d_bwd")
        else:
            gp = g_probs.float().contiguous()
            H.check(H.lib().lt_softargmax2d_bwd_full(probs.data_ptr(), coords.data_ptr(), H.ptr(g), gp.data_ptr(), 1.0, int(ctx.softmax), ghm.data_ptr(),
                                                     N * J, h, w, H.cur_stream()), "lt_softargmax2d_bwd_full")
        return ghm.to(ctx.in_dtype), None, None


def gaussian_2d_pdf(coords, means, sigmas, normalize=True):
    """coords, means, sigmas (n, 2) as (x, y) -> (n,) values of the axis-aligned Gaussian.  Reference: op.py:169-175, a plain tensor expression on
    whatever device the inputs live on (the parity shim; the rendering kernel is behind render_points_as_2d_gaussians).  The normaliser is
    2 pi sigma_x sigma_x -- sigma_x twice, as in the reference."""
    normalization = 1.0
    if normalize:
        normalization = 2 * np.pi * sigmas[:, 0] * sigmas[:, 0]
    exp = torch.exp(-((coords[:, 0] - means[:, 0]) ** 2 / sigmas[:, 0] ** 2 + (coords[:, 1] - means[:, 1]) ** 2 / sigmas[:, 1] ** 2) / 2)
    return exp / normalization


def render_points_as_2d_gaussians(points, sigmas, image_shape, normalize=True):
    """points (n, 2) as (x, y) in pixels of the rendered map, sigmas (n, 2), image_shape (h, w) -> (n, h, w) fp32 Gaussians.  Reference: op.py:178-196.
    GPU tensors: one lt_render_gaussians_2d launch (the reference materialises an (n, h, w, 2) grid and two repeats); CPU tensors (dataset-side code):
    the broadcast tensor expression.  No gradient flows to points or sigmas through the GPU path.  numpy fp64: mvn.utils.multiview.render_gaussians_2d."""
    h, w = int(image_shape[0]), int(image_shape[1])
    n = points.shape[0]
    if not points.is_cuda:
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
        grid = torch.stack([xx, yy], dim=-1).reshape(1, h * w, 2).expand(n, h * w, 2).reshape(-1, 2)
        rep = lambda t: t.float()[:, None, :].expand(n, h * w, 2).reshape(-1, 2)
        return gaussian_2d_pdf(grid, rep(points), rep(sigmas), normalize=normalize).reshape(n, h, w)
    pts = points.detach().float().contiguous()
    sg = sigmas.detach().to(points.device, torch.float32).contiguous()
    if pts.shape != (n, 2) or sg.shape != (n, 2):
        raise ValueError("render_points_as_2d_gaussians: points and sigmas must be (n, 2), got %s and %s" % (tuple(points.shape), tuple(sigmas.shape)))
    out = torch.empty(n, h, w, dtype=torch.float32, device=points.device)
    if n:
        with torch.cuda.device(points.device):
            H.check(H.lib().lt_render_gaussians_2d(pts.data_ptr(), sg.data_ptr(), out.data_ptr(), n, h, w, int(bool(normalize)), H.cur_stream()),
                    "lt_render_gaussians_2d")
    return out


def integrate_tensor_2d(heatmaps, softmax=True):
    """heatmaps (N,J,h,w) -> (coordinates (N,J,2) as (x,y), heatmaps after softmax / ReLU).  Reference: op.py:11-47.  When the input requires grad both
    outputs are differentiable with respect to it: a loss on the coordinates alone takes lt_softargmax2d_bwd (as before the heatmaps were differentiable:
    same launch, same bits), a gradient on the returned heatmaps lt_softargmax2d_bwd_full."""
    H.require_gpu(heatmaps, "heatmaps")
    if torch.is_grad_enabled() and heatmaps.requires_grad:
        return _SoftArgmax2dFn.apply(heatmaps, softmax)
    return _softargmax2d_launch(heatmaps, softmax)

def integrate_tensor_2d_with_stats(heatmaps, softmax=True):
    """integrate_tensor_2d plus the per-heatmap statistics, out of the same pass that writes the normalised heatmaps (lt_softargmax2d_stats_fwd).  Returns
    (coordinates, heatmaps, (peak (N,J), peak_index (N,J) int32, mass (N,J), covariance (N,J,2,2) in heatmap px^2 about the returned coordinates)): the first
    two are bit for bit what integrate_tensor_2d returns and differentiable in the same way (coordinates and heatmaps both); the statistics carry no
    gradient.  The definitions in numpy fp64: mvn.utils.multiview.heatmap_stats_2d."""
    H.require_gpu(heatmaps, "heatmaps")
    if torch.is_grad_enabled() and heatmaps.requires_grad:
        out = []
        coords, probs = _SoftArgmax2dFn.apply(heatmaps, softmax, out)
        return coords, probs, out[0]
    return _softargmax2d_launch(heatmaps, softmax, with_stats=True)
