"""Losses with the reference's names and signatures (mvn/models/loss.py of the reference).

The four keypoint losses act on (B, J, 3) tensors -- a few hundred floats -- and stay the reference's plain tensor expressions
("pure torch, reusable as is"; there is nothing for a kernel to win).  ``VolumetricCELoss`` is the one
that costs the reference real time -- a Python loop over samples with a ``.cpu()`` synchronisation each and a loop over joints
(loss.py:61-77) over a (B, V^3) distance volume it materialises per sample -- and is ONE liblt_hip launch here
(lt_volumetric_ce_fwd: nearest voxel, -log p and the sparse gradient, one workgroup per (sample, joint), no host round trip)."""
import torch
from torch import nn

import lt_hip as H
from mvn.utils import op


class KeypointsMSELoss(nn.Module):
    def forward(self, keypoints_pred, keypoints_gt, keypoints_binary_validity):
        dimension = keypoints_pred.shape[-1]
        loss = torch.sum((keypoints_gt - keypoints_pred) ** 2 * keypoints_binary_validity)
        return loss / (dimension * torch.clamp(torch.sum(keypoints_binary_validity), min=1))


class KeypointsMSESmoothLoss(nn.Module):
    def __init__(self, threshold=400):
        super().__init__()
        self.threshold = threshold

    def forward(self, keypoints_pred, keypoints_gt, keypoints_binary_validity):
        dimension = keypoints_pred.shape[-1]
        diff = (keypoints_gt - keypoints_pred) ** 2 * keypoints_binary_validity
        diff = torch.where(diff > self.threshold, torch.pow(diff.clamp(min=1e-30), 0.1) * (self.threshold ** 0.9), diff)
        return torch.sum(diff) / (dimension * torch.clamp(torch.sum(keypoints_binary_validity), min=1))


class KeypointsMAELoss(nn.Module):
    def forward(self, keypoints_pred, keypoints_gt, keypoints_binary_validity):
        dimension = keypoints_pred.shape[-1]
        loss = torch.sum(torch.abs(keypoints_gt - keypoints_pred) * keypoints_binary_validity)
        return loss / (dimension * torch.clamp(torch.sum(keypoints_binary_validity), min=1))


class KeypointsL2Loss(nn.Module):
    def forward(self, keypoints_pred, keypoints_gt, keypoints_binary_validity):
        loss = torch.sum(torch.sqrt(torch.sum((keypoints_gt - keypoints_pred) ** 2 * keypoints_binary_validity, dim=2)))
        return loss / torch.clamp(torch.sum(keypoints_binary_validity), min=1)


class _VolumetricCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, coord_volumes, volumes, keypoints_gt, validity):
        B, J = volumes.shape[:2]
        nvox = volumes[0, 0].numel()
        dev = volumes.device
        cv = coord_volumes.float().contiguous()
        pr = volumes.float().contiguous()
        terms = torch.empty(B, J, dtype=torch.float32, device=dev)
        idx = torch.empty(B, J, dtype=torch.int32, device=dev)
        gval = torch.empty(B, J, dtype=torch.float32, device=dev)
        gt = keypoints_gt.float().contiguous()
        val = validity.float().reshape(B, J).contiguous()
        H.check(H.lib().lt_volumetric_ce_fwd(cv.data_ptr(), pr.data_ptr(), gt.data_ptr(), val.data_ptr(), terms.data_ptr(), idx.data_ptr(),
                                             gval.data_ptr(), B, J, nvox, H.cur_stream()), "lt_volumetric_ce_fwd")
        ctx.save_for_backward(idx, gval)
        ctx.volumes = volumes if volumes.requires_grad else None     # only its grad_fn / shape are used in backward
        return terms.sum() / (B * J)

    @staticmethod
    def backward(ctx, g):
        idx, gval = ctx.saved_tensors
        if ctx.volumes is None:
            return None, None, None, None
        # the gradient on the probabilities is one voxel per (sample, joint): it goes to lt_softargmax3d_bwd in sparse form
        # (a dense (B,J,V^3) gradient would be 570 MB at 32 samples)
        return None, op.sparse_prob_grad(ctx.volumes, idx, (gval * g).contiguous()), None, None


class _HeatmapMSEFn(torch.autograd.Function):
    """lt_heatmap_mse_fwd as one autograd node: loss terms and d loss / d heatmaps out of ONE pass over the prediction (the Gaussian targets are never
    written to memory); backward scales the stored gradient by the upstream scalar on the device.  Keypoints, sigmas and validity get no gradient."""

    @staticmethod
    def forward(ctx, pred, points, sigmas, validity, normalize):
        h, w = pred.shape[-2:]
        pr = pred.float().contiguous()
        NJ = pr.numel() // (h * w)
        terms = torch.empty(NJ, dtype=torch.float32, device=pr.device)
        need = ctx.needs_input_grad[0]
        grad = torch.empty_like(pr) if need else None
        with torch.cuda.device(pr.device):
            H.check(H.lib().lt_heatmap_mse_fwd(pr.data_ptr(), points.data_ptr(), sigmas.data_ptr(), validity.data_ptr(), int(bool(normalize)), terms.data_ptr(),
                                               H.ptr(grad), NJ, h, w, H.cur_stream()), "lt_heatmap_mse_fwd")
        if need:
            ctx.save_for_backward(grad)
        ctx.in_dtype = pred.dtype
        return terms.sum() / (h * w * torch.clamp(validity.sum(), min=1))

    @staticmethod
    def backward(ctx, g):
        if not ctx.saved_tensors:
            return None, None, None, None, None
        (grad,) = ctx.saved_tensors
        return (grad * g).to(ctx.in_dtype), None, None, None, None


class HeatmapMSELoss(nn.Module):
    """The 2D heatmap loss the reference's backbone was trained with: mean squared error between the predicted heatmaps and Gaussians rendered at the
    ground-truth keypoints (op.render_points_as_2d_gaussians), over the annotated joints:

        sum_ij validity_ij * sum_xy (pred_ij - G_ij)^2 / (h * w * max(1, sum validity))

    forward(heatmaps_pred (..., J, h, w), keypoints_2d_gt (..., J, 2), keypoints_binary_validity (..., J, 1) or (..., J), sigmas=None (..., J, 2)).
    keypoints_2d_gt are (x, y) IN HEATMAP PIXELS: from image pixels of an (H, W) input, x_hm = x * w / W and y_hm = y * h / H (the inverse of the
    scaling AlgebraicTriangulationNet applies to its 2D keypoints, triangulation.py:181-184 of the reference).  ``sigma`` (heatmap pixels) is used for
    both axes of every joint unless ``sigmas`` gives them per joint; ``normalize`` divides the targets by 2 pi sigma_x sigma_x as gaussian_2d_pdf does.
    A joint with validity 0 contributes exactly nothing and its keypoint is never read -- it may be NaN (a missing annotation).  One liblt_hip launch
    (lt_heatmap_mse_fwd); the gradient reaches ``heatmaps_pred`` only.  numpy fp64: mvn.utils.multiview.heatmap_mse_2d."""

    def __init__(self, sigma=2.0, normalize=False):
        super().__init__()
        self.sigma, self.normalize = float(sigma), bool(normalize)

    def forward(self, heatmaps_pred, keypoints_2d_gt, keypoints_binary_validity, sigmas=None):
        H.require_gpu(heatmaps_pred, "heatmaps_pred")
        dev = heatmaps_pred.device
        if heatmaps_pred.dim() < 3:
            raise ValueError("heatmaps_pred must be (..., J, h, w), got %s" % (tuple(heatmaps_pred.shape),))
        lead = tuple(heatmaps_pred.shape[:-2])
        NJ = int(torch.Size(lead).numel())
        if tuple(keypoints_2d_gt.shape) != lead + (2,):
            raise ValueError("keypoints_2d_gt must be %s, got %s" % (lead + (2,), tuple(keypoints_2d_gt.shape)))
        if tuple(keypoints_binary_validity.shape) not in (lead, lead + (1,)):
            raise ValueError("keypoints_binary_validity must be %s or %s, got %s" % (lead + (1,), lead, tuple(keypoints_binary_validity.shape)))
        pts = keypoints_2d_gt.detach().to(dev, torch.float32).reshape(NJ, 2).contiguous()
        val = keypoints_binary_validity.detach().to(dev, torch.float32).reshape(NJ).contiguous()
        if sigmas is None:
            sg = torch.full((NJ, 2), self.sigma, dtype=torch.float32, device=dev)
        else:
            if tuple(sigmas.shape) != lead + (2,):
                raise ValueError("sigmas must be %s, got %s" % (lead + (2,), tuple(sigmas.shape)))
            sg = sigmas.detach().to(dev, torch.float32).reshape(NJ, 2).contiguous()
        return _HeatmapMSEFn.apply(heatmaps_pred, pts, sg, val, self.normalize)


class VolumetricCELoss(nn.Module):
    """loss.py:52-80: mean over ALL (sample, joint) pairs of validity * -log(p[nearest voxel to the ground truth] + 1e-6)."""

    def forward(self, coord_volumes_batch, volumes_batch_pred, keypoints_gt, keypoints_binary_validity):
        H.require_gpu(volumes_batch_pred, "volumes_batch_pred")
        return _VolumetricCEFn.apply(coord_volumes_batch, volumes_batch_pred, keypoints_gt, keypoints_binary_validity)
