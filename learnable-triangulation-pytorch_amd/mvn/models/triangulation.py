"""Triangulation networks with the reference's surface (mvn/models/triangulation.py of the reference):

    VolumetricTriangulationNet(config, device).forward(images, proj_matricies, batch)
    AlgebraicTriangulationNet(config, device).forward(images, proj_matricies, batch)
    RANSACTriangulationNet(config, device).forward(images, proj_matricies, batch)

and, beyond the reference, ``CascadeTriangulationNet(alg_net, vol_net)``: its two-stage evaluation route (the algebraic model's pelvis centres the
volumetric cuboid) as one forward with the pelvis kept on the GPU.

Same constructor side effects on ``config``, same ``state_dict()`` keys, same return tuples.  The whole
forward is ONE recorded plan of liblt_hip launches per input shape, captured into a hipGraph:

    images --lt_nchw_to_nhwc--> [graph: PoseResNet convs -> process_features 1x1 -> lt_coord_volumes ->
    lt_unproject_fwd -> V2V convs -> lt_softargmax3d_fwd] --> outputs

The RANSAC net's plan ends in lt_heatmap_argmax_nchw_f32; lt_triangulate_ransac follows it on the same stream (inference only).

Host work per call is numpy fp64 camera algebra for B*NV 3x4 matrices (vectorised; the reference
deep-copies B*NV Camera objects) and one small H2D copy of the geometry block.
"""
import ctypes as C

from collections import OrderedDict

import os

import numpy as np
import torch
import torch.nn as nn

import lt_engine as E
import lt_hip as H
from lt_staging import PinnedRing
from mvn.models import pose_resnet
from mvn.models.v2v import V2VModel
from mvn.utils import multiview, op, volumetric


GEO_RING = 4          # pinned geometry staging slots per plan (forwards the host may run ahead of the GPU)
MAX_LAUNCH_ELEMS = 2 ** 31   # ONE SAMPLE's largest activation: liblt_hip's convolution kernels index a launch with 32-bit element offsets; batches beyond that
                             # are walked in sample chunks INSIDE lt_conv_fwd (64-bit base pointers, round 6), the other kernels of the path index in 64 bits


def _bn_in_train_mode(m):
    return any(isinstance(c, nn.modules.batchnorm._BatchNorm) and c.training for c in m.modules())


def _sync_buffers_before_eval(model):
    """DistributedDataParallel(broadcast_buffers=True) hands rank 0's buffers to every rank at EVERY forward, evaluation included (the reference
    validates through the wrapped model, train.py:450-460).  The training forward does it through its reducer; here the first evaluation forward
    after a training step does (the BatchNorm statistics of the ranks differ by their last momentum update until then; buffers do not change in
    eval(), so once is enough).  A COLLECTIVE: like under DDP, every rank has to run that evaluation forward -- a rank-0-only forward (master-only
    visualisation, checkpoint evaluation) on a model with an attached reducer would wait for the other ranks forever.  For that use set
    ``model.sync_buffers_on_eval = False`` (or LT_NO_EVAL_BUFFER_SYNC=1): the forward then runs on this rank's own statistics and no collective is issued
    (ADVICE r4)."""
    if not getattr(model, "sync_buffers_on_eval", True) or os.environ.get("LT_NO_EVAL_BUFFER_SYNC") == "1":
        return
    red = getattr(model, "grad_reducer", None)
    if red is not None and red.attached and model.__dict__.get("_buffers_stale"):
        red.sync_buffers()
        model.__dict__["_buffers_stale"] = False


def _batch_view_mask(batch, B, NV, min_valid, who):
    """``batch["view_mask"]`` as a checked host (B, NV) uint8 array, or None when the batch has none.  ValueError for another shape or a sample with
    fewer than ``min_valid`` valid views -- raised before anything is launched."""
    vm = batch.get("view_mask") if isinstance(batch, dict) else None
    if vm is None:
        return None
    return op.view_mask_host(vm, B, NV, min_valid=min_valid, what="%s: batch['view_mask']" % who)


def _batch_cuboid_frame(batch, F, who):
    """``batch["cuboid_frame"]`` -- the frame of every cuboid of a multi-cuboid forward -- as a checked host (P,) int32 array, or None when the batch has
    none.  ValueError for an empty list, an index outside [0, F) or a non-integer entry -- raised before anything is launched."""
    cf = batch.get("cuboid_frame") if isinstance(batch, dict) else None
    if cf is None:
        return None
    return op.frame_index_host(cf, F, what="%s: batch['cuboid_frame']" % who)


def _refuse_view_counts(batch, who):
    """``batch["view_counts"]`` (a ragged batch, mvn.datasets.utils.ragged_batch) on a model without a ragged plan is refused before anything is launched
    (VolumetricTriangulationNet and AlgebraicTriangulationNet take it in eval())."""
    if isinstance(batch, dict) and batch.get("view_counts") is not None:
        raise NotImplementedError("%s: batch['view_counts'] (a ragged batch) is not taken by this model; pad the batch to (B, NV) and pass "
                                  "batch['view_mask'] instead, or run VolumetricTriangulationNet / AlgebraicTriangulationNet on the ragged batch" % who)


class _VolTrainPlan:
    """The training step of VolumetricTriangulationNet for one input shape, recorded once and replayed (lt_train.TrainTape): the first
    forward / backward run the layers while recording them; later steps re-launch the recorded closures over the same buffers.  What
    changes from step to step enters through fixed buffers: the images (layout change into ``x_in``), the geometry block (one pinned
    H2D copy, as in inference), the parameters (gathered live into the GEMM layouts), the loss gradient (``lt_softargmax3d_bwd`` into
    ``gl``).

    masked (``masked_training`` steps with ``batch["view_mask"]``): the tape records lt_unproject_grid_masked_fwd / lt_unproject_masked_bwd in the
    unmasked pair's place; the (B, NV) uint8 mask rides at the end of the geometry block as in the inference plan, so another mask is just
    another step of the same tape.

    cuboids (``multi_cuboid_training`` steps with ``batch["cuboid_frame"]``): P = ``cuboids`` cuboids over the B frames.  The backbone and process_features
    (the frozen backbone's inference plan included) are recorded at B * NV images; the volume, V2V, the soft-argmax and their buffers at P; the tape
    records lt_unproject_grid_indexed_fwd / lt_unproject_indexed_bwd (with the mask, if ``masked``) in the pair's place.  The P int32 frame indices
    ride in the geometry block behind the rotations, at the inference plan's offset, and are read inside the kernels only: another assignment of the
    cuboids to the frames is just another step of the same tape."""

    def __init__(self, model, B, NV, Hh, W, device, masked=False, cuboids=None):
        self.model, self.B, self.NV, self.Hh, self.W, self.device = model, B, NV, Hh, W, device
        self.masked = bool(masked)
        self.cuboids = None if cuboids is None else int(cuboids)
        self.tape = None
        self.step_id = 0

    def forward(self, images, batch):
        import lt_train
        model, B, NV, Hh, W, device = self.model, self.B, self.NV, self.Hh, self.W, self.device
        V, J = model.volume_size, model.num_joints
        multi = self.cuboids is not None
        nc = self.cuboids if multi else B          # B frames carry the images, the features and the confidences; everything from the gather on is per cuboid
        lib = H.lib()
        st = torch.cuda.current_stream(device).cuda_stream
        x = images.reshape(B * NV, 3, Hh, W)
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.float().contiguous()
        first = self.tape is None
        if first:
            prec = getattr(model, "train_precision", "fp32")
            mixed, act16 = prec != "fp32", prec in ("act16", "fp8v2v")
            self.tape = tape = lt_train.TrainTape(device, params=list(model.parameters()), reducer=getattr(model, "grad_reducer", None), mixed=mixed, act16=act16,
                                                  fp8_3d=prec == "fp8v2v")
            # a FULLY FROZEN backbone in eval() (no trainable parameter, no BatchNorm module in train()) is exactly the inference backbone: its feature map
            # (and the vol_confidences head's output) come from an inference plan -- fused launches, folded BatchNorm, no activation kept -- and the tape
            # starts at process_features.  LT_TRAIN_NO_FROZEN_PLAN=1 (read here, when the training plan is built) keeps it on the tape, backward pruned.
            bb = model.backbone
            self.frozen_plan = (os.environ.get("LT_TRAIN_NO_FROZEN_PLAN") != "1" and not any(p.requires_grad for p in bb.parameters()) and
                                not any(c.training for c in bb.modules() if isinstance(c, nn.modules.batchnorm._BatchNorm)))
            # the plan's element type is the tape's activation type (bf16 for act16 / fp8v2v, fp32 for fp32); 'bf16' stores fp32, so the fp32 plan it is:
            # the one conversion left is the tape's own cast of process_features' input to the bf16 MFMA operand
            self.bb_dtype = torch.bfloat16 if act16 else torch.float32
            if not self.frozen_plan:
                self.x_in = tape.alloc((B * NV, 1, Hh, W, E.min_cin_of(torch.bfloat16 if mixed else torch.float32)))
                tape.no_grad(self.x_in)
        tape = self.tape
        ac = tape.acode          # element type of the activations: fp32, or bf16 in the 16-bit-activation step
        if self.frozen_plan:
            bb_feats, bb_volc = self._frozen_backbone(x, st)
            if first:          # the tape's gradient-free inputs: buffers of its own, so that a rebuilt plan (changed backbone weights) leaves the recorded pointers valid
                self.f_in = tape.no_grad(tape.alloc(bb_feats.shape))
                self.c_in = None if bb_volc is None else tape.no_grad(tape.alloc(bb_volc.shape, torch.float32))
            f_in, c_in = self.f_in, self.c_in
            assert f_in.t.dtype == bb_feats.t.dtype and f_in.shape == bb_feats.shape
            cf = f_in.shape[-1]
            H.check(lib.lt_convert_pad(ac, bb_feats.t.data_ptr(), ac, f_in.t.data_ptr(), f_in.t.numel() // cf, cf, cf, st), "lt_convert_pad")
            if c_in is not None:
                cc = c_in.shape[-1]
                H.check(lib.lt_convert_pad(H.LT_F32, bb_volc.t.data_ptr(), H.LT_F32, c_in.t.data_ptr(), c_in.t.numel() // cc, cc, cc, st), "lt_convert_pad")
        else:
            E.stage_images(x, self.x_in, st)
        if first:
            # layers in front of the unprojection (its launch needs the map size, the geometry block the launch reads needs the maps' size too)
            if self.frozen_plan:
                feats256, volc = self.f_in, self.c_in
            else:
                _, feats256, _, volc = model.backbone.record(tape, self.x_in, want_heatmaps=False)
            self.volc = volc          # conf / conf_norm: the vol_confidences head's sigmoid output, Act [1,1,1,B*NV,32] (pose_resnet.py:140-174)
            pf = model.process_features[0]
            self.feats = feats = tape.conv(feats256, pf.weight, pf.bias, None)
            h, w = feats.shape[2], feats.shape[3]
            # proj B*NV*12 | pos nc*3 | center nc*3 | rot nc*9 | [frame_of nc int32] | [mask B*NV bytes], the inference plan's block (_build_plan)
            o_fof = B * NV * 12 + nc * 15          # multi-cuboid plans: the frame of every cuboid
            o_mask = o_fof + (nc if multi else 0)          # masked plans: B*NV mask bytes behind the words (whole words)
            n_geo = o_mask + ((B * NV + 3) // 4 if self.masked else 0)
            self.G = {"hw": (h, w), "offs": (B * NV * 12, B * NV * 12 + 3 * nc, B * NV * 12 + 6 * nc), "geo_ring": PinnedRing(n_geo, torch.float32, GEO_RING),
                      "masked": self.masked, "o_mask": o_mask, "o_fof": o_fof, "cuboids": nc if multi else None}
            self.geo = torch.zeros(n_geo, dtype=torch.float32, device=device)
            self.n_front = len(tape.fwd_ops)
        else:
            tape.stream = st
            tape._gather_all("fwd", tape.fwd_jobs)          # every layer's weights into its GEMM layout, one launch
            tape.replay(tape.fwd_ops, 0, self.n_front)
        G = self.G
        h, w = G["hw"]
        o_pos, o_cen, o_rot = G["offs"]
        # host geometry exactly as in inference (numpy fp64; theta ~ U(0, 2 pi) because self.training), one pinned H2D copy
        position, base, sides = model._host_geometry(batch, B, (Hh, W), G)
        self.geo.copy_(G["geo_host"], non_blocking=True)
        G["geo_ring"].commit(torch.cuda.current_stream(device))
        if first:
            feats, gp = self.feats, self.geo.data_ptr()
            self.coords = coords = torch.empty(nc, V, V, V, 3, dtype=torch.float32, device=device)
            vol = tape.alloc((nc, V, V, V, 32))
            step = float(np.float32(model.cuboid_side / (V - 1)))
            agg = H.AGG[model.volume_aggregation_method]
            cmu = int(bool(model.transfer_cmu_to_human36m))
            volc = self.volc
            conf_p = None if volc is None else volc.t.data_ptr()          # (B, NV, 32) raw confidences; 'conf_norm' is normalised inside the kernels
            mask_p = gp + 4 * G["o_mask"]          # masked plans: the step's (B, NV) mask, behind the geometry in the same block
            fof_p = gp + 4 * G.get("o_fof", 0)          # multi-cuboid plans: the step's (nc,) int32 frame indices, in the same block
            # one descriptor for the forward and the backward closure: the grid form (the backward reads the coords_out the forward wrote), the
            # variant by the pointers that are set
            desc = H.UnprojectDesc(dtype=ac, feats=feats.t.data_ptr(), proj=gp, pos=gp + 4 * o_pos, center=gp + 4 * o_cen, rot=gp + 4 * o_rot, step=step,
                                   cmu_transfer=cmu, coords_out=coords.data_ptr(), conf=conf_p, view_mask=mask_p if self.masked else None,
                                   frame_of=fof_p if multi else None, F=B, B=nc, NV=NV, C=32, h=h, w=w, v0=V, v1=V, v2=V, agg=agg)
            fwd_entry, bwd_entry = H.unproject_entry(desc), H.unproject_entry(desc, bwd=True)
            tape.do(lambda s_: H.check(lib.lt_unproject_desc_fwd(C.byref(desc), vol.t.data_ptr(), s_), fwd_entry), "unproject")
            tape._derive(vol, (feats, volc))
            need_f, need_c = tape.carries(feats), tape.carries(volc)

            def unproject_bwd():
                dvol = tape.grad_of(vol)
                if dvol is None or not (need_f or need_c):          # nothing trainable in front of the volume: no unprojection backward
                    return
                gfe32 = torch.empty(feats.t.shape, dtype=torch.float32, device=device)                    # written completely by the gather (no zero fill)
                gconf = None if volc is None else torch.empty_like(volc.t)
                if tape.act16:
                    # lt_unproject_bwd takes and gives fp32 gradients: the volume's bf16 gradient is widened in front of it, the maps' gradient rounded behind it
                    dvol16 = dvol
                    dvol32 = torch.empty(dvol16.shape, dtype=torch.float32, device=device)
                    nvol = dvol16.numel()
                    tape.do(lambda s_: H.check(lib.lt_convert_pad(H.LT_BF16, dvol16.data_ptr(), H.LT_F32, dvol32.data_ptr(), nvol // 32, 32, 32, s_), "lt_convert_pad"), "cast")
                else:
                    dvol32 = dvol
                # the gather's workspace comes out of the tape's shared main-stream scratch (it is only live during this one op; a private buffer per
                # cached plan was up to 4 GiB each), capped like op.unproject_heatmaps' autograd path: below the whole batch's worth the
                # entry point walks the batch in chunks (multi-cuboid: the confidence partials of all cuboids and as many cuboids' shares as fit the cap)
                nws = int(max(16, op.unproject_bwd_workspace(desc, cap=op.UNPROJECT_BWD_WORKSPACE_CAP)))
                tape._ws_need(nws)
                tape.do(lambda s_: H.check(lib.lt_unproject_desc_bwd(C.byref(desc), dvol32.data_ptr(), gfe32.data_ptr(), H.ptr(gconf), tape._ws.data_ptr(), nws,
                                                                     s_), bwd_entry), "unproject_bwd")
                gfe = gfe32
                if tape.act16:
                    gfe = torch.empty(feats.t.shape, dtype=torch.bfloat16, device=device)
                    nfe = gfe.numel()
                    tape.do(lambda s_: H.check(lib.lt_convert_pad(H.LT_F32, gfe32.data_ptr(), H.LT_BF16, gfe.data_ptr(), nfe // 32, 32, 32, s_), "lt_convert_pad"), "cast")
                if need_f:          # (the kernel computes both gradients; one that nothing in front needs is dropped here)
                    tape.seed(feats, gfe)
                if need_c:
                    tape.seed(volc, gconf)            # the head's backward (recorded earlier, so replayed later) starts from here
            tape.add_backward(unproject_bwd)
            self.logits = logits = model.volume_net.record(tape, vol)          # channels-last (B,V,V,V,J) fp32
            self.kp = kp = torch.empty(nc, J, 3, dtype=torch.float32, device=device)
            self.probs = probs = torch.empty(nc, J, V, V, V, dtype=torch.float32, device=device)
            ws = torch.empty(max(1, lib.lt_softargmax3d_workspace(nc, J, V ** 3)), dtype=torch.uint8, device=device)
            self.mult, self.sm = float(model.volume_multiplier), int(bool(model.volume_softmax))
            mult, sm = self.mult, self.sm
            tape.do(lambda s_: H.check(lib.lt_softargmax3d_fwd(logits.t.data_ptr(), coords.data_ptr(), mult, sm, 1, J, kp.data_ptr(), probs.data_ptr(), nc, J, V ** 3,
                                                               ws.data_ptr(), s_), "lt_softargmax3d_fwd"))
            self.gl = torch.empty(nc, V ** 3, J, dtype=torch.float32, device=device)         # d loss / d logits, channels-last like the logits (fp32 in every
            tape.seed(logits, self.gl.view(logits.t.shape))                                  # precision: the logits layer stores fp32, TrainTape._act_grad rounds its dY once)
        else:
            tape.replay(tape.fwd_ops, self.n_front)
        self.step_id += 1
        conf_out = None
        if self.volc is not None:          # the returned vol_confidences (reference :266-269, :355): (B, NV, 32), normalised over the views for conf_norm
            conf_out = self.volc.t.reshape(B, NV, 32).clone()
            if model.volume_aggregation_method == "conf_norm":
                if self.masked:          # the inference rule: normalised over the valid views, a masked view's entries 0 (an all-ones mask: the same bits)
                    on = torch.from_numpy(batch["view_mask"]).to(device, non_blocking=True).bool()[:, :, None]
                    conf_out = torch.where(on, conf_out, torch.zeros((), dtype=conf_out.dtype, device=device))
                conf_out = conf_out / conf_out.sum(dim=1, keepdim=True)
        self.conf_out = conf_out
        feats_out = torch.empty(B, NV, 32, h, w, dtype=torch.float32, device=device)          # the returned features, contiguous like the reference's
        H.check(lib.lt_nhwc_to_nchw_f32(ac, self.feats.t.data_ptr(), feats_out.data_ptr(), B * NV, 32, h * w, 32, st), "lt_nhwc_to_nchw_f32")
        base_points = self.geo[o_cen:o_rot].reshape(nc, 3).clone()
        return self.kp.clone(), self.probs.clone(), feats_out, self.coords.clone(), base_points, position, sides

    def _frozen_backbone(self, x, st):
        """The frozen, eval-mode backbone of this step on the inference kernel set, on the step's stream: (features Act, vol_confidences Act | None) of an
        inference plan recorded by PoseResNet.record on a PlanBuilder, kept in the backbone's own plan cache -- whose weights fingerprint (data_ptr and
        version counter of every parameter and buffer of the backbone) rebuilds it after an in-place change or a load_state_dict."""
        bb, N, dt = self.model.backbone, self.B * self.NV, self.bb_dtype

        def build():
            b = E.PlanBuilder(self.device, dt)
            inp = b.alloc((N, 1, self.Hh, self.W, E.min_cin_of(dt)))
            _, feats, _, volc = bb.record(b, inp, want_heatmaps=False)
            return {"plan": b.finish(), "inp": inp, "outs": (feats, volc)}

        P = bb._plan_for(("train-frozen", N, self.Hh, self.W, dt, self.device), build)
        E.stage_images(x, P["inp"], st)
        P["plan"].run_eager(st)
        return P["outs"]

    def backward(self, g_kp, idx, val, g_dense=None):
        B, J = self.probs.shape[:2]
        nvox = self.probs[0, 0].numel()
        st = torch.cuda.current_stream(self.device).cuda_stream
        ws = None
        if g_dense is not None:          # a dense gradient on the returned volumes (any loss on them, as the reference's autograd accepts)
            ws = self.__dict__.setdefault("_pg_ws", torch.empty(B * J, dtype=torch.float32, device=self.device))
        H.check(H.lib().lt_softargmax3d_bwd_dense(self.probs.data_ptr(), self.coords.data_ptr(), self.kp.data_ptr(), g_kp.data_ptr(), H.ptr(idx), H.ptr(val), H.ptr(g_dense),
                                                  H.ptr(ws), self.mult, self.sm, 1, self.gl.data_ptr(), B, J, nvox, st), "lt_softargmax3d_bwd")
        pg = self.tape.run_backward()
        flat = self.tape.arena.clone()          # autograd gets its own copy: the arena is overwritten by the next step
        off = self.tape.arena.data_ptr()
        return {p: flat[(v.data_ptr() - off) // 4:(v.data_ptr() - off) // 4 + v.numel()].view(v.shape) for p, v in pg.items()}


class _VolTrainFn(torch.autograd.Function):
    """The whole training-mode forward of VolumetricTriangulationNet as ONE autograd node: forward runs (the first time: records) the
    layers through the plan's lt_train.TrainTape (liblt_hip, fp32, BatchNorm on batch statistics), backward replays the tape's backward
    and hands the parameter gradients back to autograd -- so ``loss.backward()``, ``torch.optim`` / ``lt_train.Adam`` work as with the
    reference (train.py:233-243).  Inputs: (plan, images, batch, *parameters)."""

    @staticmethod
    def forward(ctx, plan, images, batch, *params):
        ctx.set_materialize_grads(False)              # an unused output arrives as None in backward, not as a dense zero tensor
        ctx._lt_accepts_sparse_prob_grads = True      # VolumetricCELoss's one-voxel gradients are applied inside lt_softargmax3d_bwd
        with torch.cuda.device(images.device):
            kp, probs, feats_out, coords, base_points, position, sides = plan.forward(images, batch)
        ctx.plan, ctx.step_id, ctx.params = plan, plan.step_id, params
        ctx.mark_non_differentiable(feats_out, coords, base_points)
        plan.model._train_extra = (position, sides)
        return kp, probs, feats_out, coords, base_points

    @staticmethod
    def backward(ctx, g_kp, g_probs, *unused):
        plan = ctx.plan
        if ctx.step_id != plan.step_id:
            raise RuntimeError("only the LATEST training forward of a shape can be backpropagated (its activations live in the plan's buffers, "
                               "which a newer forward has overwritten)")
        with torch.cuda.device(plan.device):
            g_kp = torch.zeros_like(plan.kp) if g_kp is None else g_kp.float().contiguous()
            sparse = getattr(ctx, "_lt_sparse_prob_grads", [])
            idx = val = g_dense = None
            if len(sparse) == 1:
                idx, val = sparse[0]
            elif len(sparse) > 1:
                raise NotImplementedError("more than one sparse (VolumetricCELoss) gradient on the returned volumes of one forward")
            if g_probs is not None and not op.is_sparse_placeholder(ctx, g_probs):
                # any other loss on the volumes: a dense (B, J, V, V, V) gradient, added to the soft-argmax backward's a_i (round 4; VolumetricCELoss's
                # placeholder next to its sparse gradient is recognised by its storage -- a uniform gradient, volumes.sum(), is a real one)
                g_dense = g_probs.float().contiguous()
            pg = plan.backward(g_kp, idx, val, g_dense)
        grads = tuple(pg.get(p) if p.requires_grad else None for p in ctx.params)
        return (None, None, None) + grads


# the backbone's recorded training step (one plan class for this module's AlgebraicTriangulationNet and for PoseResNet's own train() forward)
_AlgTrainPlan, _AlgTrainFn = pose_resnet.BackboneTrainPlan, pose_resnet.BackboneTrainFn


class _PlannedNet(E.PlanCache):
    """A whole triangulation net behind one plan cache (lt_engine.PlanCache: LRU + weights fingerprint)."""

    def __init__(self):
        super().__init__()
        self.compute_dtype = torch.float32   # the reference's precision; torch.bfloat16 = throughput mode
        self.use_graph = True
        self.copy_outputs = True             # False: return views of plan-owned buffers (valid until the next forward)
        self.tile_override = 0
        self._stream = None
        self._init_plan_cache()

    def set_compute_dtype(self, dtype):
        H.dtype_code(dtype)
        self.compute_dtype = dtype
        return self

    def _open_plan(self, N, Hh, W, device, dry_run=False):
        """(builder, input Act): every plan starts with its builder and the channels-last map [N,1,H,W,c_pad] that forward() stages the caller's N images into
        (E.stage_images); the map is never handed back to the builder's pool."""
        b = E.PlanBuilder(device, self.compute_dtype, self.tile_override, dry_run=dry_run)
        x_in = b.alloc((N, 1, Hh, W, E.min_cin_of(self.compute_dtype)))
        x_in.pooled = False
        return b, x_in

    def _side_stream(self, device):
        if self._stream is None or self._stream.device != device:
            self._stream = torch.cuda.Stream(device=device)
        return self._stream


class VolumetricTriangulationNet(_PlannedNet):
    def __init__(self, config, device="cuda:0"):
        super().__init__()
        m = config.model
        self.num_joints = m.backbone.num_joints
        self.volume_aggregation_method = m.volume_aggregation_method
        self.volume_softmax = m.volume_softmax
        self.volume_multiplier = m.volume_multiplier
        self.volume_size = m.volume_size
        self.cuboid_side = m.cuboid_side
        self.kind = m.kind
        self.use_gt_pelvis = m.use_gt_pelvis
        self.heatmap_softmax = m.heatmap_softmax
        self.heatmap_multiplier = m.heatmap_multiplier
        self.transfer_cmu_to_human36m = m.transfer_cmu_to_human36m if hasattr(m, "transfer_cmu_to_human36m") else False
        # True: an eval forward also leaves the per-joint statistics of its 3D heatmaps (op.KeypointStats: peak, peak voxel, mass, covariance about the
        # returned joint) in last_keypoint_stats; the 7-tuple keeps its bits.  Ignored in train(), where last_keypoint_stats is None.
        self.keypoint_stats = False
        self.last_keypoint_stats = None
        # True: a train() forward takes batch["view_mask"] -- the masked training step (lt_unproject_grid_masked_fwd / lt_unproject_masked_bwd: every
        # sample's volume and its gradient over its valid views alone; the backbone still runs on every image).  False: a mask in train() is refused.
        self.masked_training = False
        # True: a train() forward takes batch["cuboid_frame"] -- the multi-cuboid training step (lt_unproject_grid_indexed_fwd / lt_unproject_indexed_bwd:
        # the backbone runs, forward and backward, on the F frames once; every frame's features get the sum of its cuboids' gradients).  False: refused.
        self.multi_cuboid_training = False
        if self.volume_aggregation_method not in H.AGG:
            raise ValueError("Unknown volume_aggregation_method: {}".format(self.volume_aggregation_method))
        # same config mutation as the reference (:228-231)
        m.backbone.alg_confidences = False
        m.backbone.vol_confidences = self.volume_aggregation_method.startswith("conf")
        self.backbone = pose_resnet.get_pose_net(m.backbone, device=device)
        for p in self.backbone.final_layer.parameters():
            p.requires_grad = False
        self.process_features = nn.Sequential(nn.Conv2d(256, 32, 1))
        self.volume_net = V2VModel(32, self.num_joints)
        if hasattr(m, "compute_dtype"):
            self.compute_dtype = {"fp32": torch.float32, "float32": torch.float32, "bf16": torch.bfloat16,
                                  "bfloat16": torch.bfloat16}[str(m.compute_dtype)]

    # ---------------------------------------------------------------------------------------
    def _build_plan(self, B, NV, Hh, W, device, dry_run=False, masked=False, stats=False, cuboids=None, ragged=None):
        """ragged: the plan of forwards with ``batch["view_counts"]`` -- B samples over ``ragged`` = T images in all, NV = NVcap: the backbone and
        process_features are recorded at T images, the gather is lt_unproject_grid_ragged_fwd, everything behind it is the plain plan's; the B + 1 int32
        offsets ride in the geometry block behind the rotations, outside the captured graph: other counts with the same (B, T, NVcap) are just another
        forward.  None: NV views per sample, the plan it always was.
        cuboids: the plan of forwards with ``batch["cuboid_frame"]`` -- P = ``cuboids`` cuboids over the B frames: the backbone and process_features
        are recorded at B * NV images, the gather (lt_unproject_grid_indexed_fwd), V2V, the soft-argmax and their buffers at P; the P int32 frame indices
        ride in the geometry block behind the rotations (in front of the mask), outside the captured graph like the rest of it: a new assignment of
        cuboids to frames on a captured plan is just another forward.  None: one cuboid per sample, the plan it always was.
        masked: the plan of forwards with ``batch["view_mask"]`` -- the same launch list with lt_unproject_grid_masked_fwd in the gather's place; the
        (B, NV) uint8 mask rides at the end of the geometry block (same pinned ring, same copy), outside the captured graph's baked pointers like the
        rest of the block, so a new mask on a captured plan is just another forward.
        stats: the plan of forwards with ``keypoint_stats`` -- the same launch list with lt_softargmax3d_stats_fwd in the tail op's place (same op kind)."""
        V, J = self.volume_size, self.num_joints
        F, multi = B, cuboids is not None          # F frames carry the images, the features and the confidences ...
        assert ragged is None or not (multi or masked), "a ragged plan has neither a mask nor several cuboids per frame"
        nimg = F * NV if ragged is None else int(ragged)          # images of the backbone pass
        b, x_in = self._open_plan(nimg, Hh, W, device, dry_run)
        B = int(cuboids) if multi else F           # ... everything from the gather on is per cuboid
        lib = b.lib
        # the 1x1 heatmap head is dead in the volumetric path: only its SHAPE is used (reference :264)
        # bf16 plans: the fused stem reads the caller's fp32 images (pointer handed over per forward through this cell)
        image_cell = {"ptr": None, "ref": None}
        _, feats256, _, volc = self.backbone.record(b, x_in, want_heatmaps=False, image_cell=image_cell)
        if not b.npre:
            image_cell = None
        pf = self.process_features[0]
        feats = b.conv(feats256, pf.weight, pf.bias, None)
        b.release(feats256)
        feats.pooled = False
        h, w = feats.shape[2], feats.shape[3]
        # geometry block (fp32, one H2D copy per forward): proj nimg*12 | pos B*3 | center B*3 | rot B*9 | [frame_of B int32] | [mask F*NV bytes]
        # (ragged plans: | view_base (B + 1) int32 behind the rotations)
        o_fof = nimg * 12 + B * 15             # multi-cuboid plans: the frame of every cuboid
        o_mask = o_fof + (B if multi else 0)   # masked plans: F*NV mask bytes behind the words (whole words)
        o_vb = o_fof                           # ragged plans: the B + 1 offsets (the exclusive prefix sum of the counts; the last one is T)
        n_geo = o_mask + ((F * NV + 3) // 4 if masked else 0) + (B + 1 if ragged is not None else 0)
        geo = torch.zeros(n_geo, dtype=torch.float32, device=device)
        # pinned staging ring: forward N+1 fills the next slot while forward N's copy may still be queued (forward never blocks on the GPU otherwise)
        geo_ring = PinnedRing(n_geo, torch.float32, 1 if dry_run else GEO_RING, pin=not dry_run)
        o_pos, o_cen, o_rot = nimg * 12, nimg * 12 + 3 * B, nimg * 12 + 6 * B
        coords = torch.empty(B, V, V, V, 3, dtype=torch.float32, device=device)
        step = float(np.float32(self.cuboid_side / (V - 1)))
        gp = geo.data_ptr()
        cmu = int(bool(self.transfer_cmu_to_human36m))
        conf = None
        if volc is not None:
            conf = volc.t.reshape(F, NV, 32) if ragged is None else volc.t.reshape(nimg, 32)   # 'conf_norm' is normalised inside the kernel (LT_AGG_CONF_NORM)
        vol = b.alloc((B, V, V, V, 32))
        esz = E.esize(self.compute_dtype)
        agg = H.AGG[self.volume_aggregation_method]
        # ONE launch: the voxel centres are computed in registers from (position, centre, rotation, step) and written to the returned
        # coordinate tensor on the way (reference :298-339 + op.py:99-166); configurations without a fused kernel run
        # lt_coord_volumes + the generic gather inside the same call
        # the variant is which pointers of the descriptor are set (include/lt_hip.h); `entry` names it by its shorthand entry
        desc = H.UnprojectDesc(dtype=b.code, feats=feats.t.data_ptr(), proj=gp, pos=gp + 4 * o_pos, center=gp + 4 * o_cen, rot=gp + 4 * o_rot, step=step,
                               cmu_transfer=cmu, coords_out=coords.data_ptr(), conf=H.ptr(conf), view_mask=gp + 4 * o_mask if masked else None,
                               frame_of=gp + 4 * o_fof if multi else None, F=F, view_base=gp + 4 * o_vb if ragged is not None else None, T=nimg,
                               B=B, NV=NV, C=32, h=h, w=w, v0=V, v1=V, v2=V, agg=agg)
        entry = H.unproject_entry(desc)
        b.custom(lambda st: H.check(lib.lt_unproject_desc_fwd(C.byref(desc), vol.t.data_ptr(), st), entry),
                 "unproject", nbytes=(nimg * h * w * 32 + B * V ** 3 * 32) * esz + B * V ** 3 * 12,   # feats once + volume once + the returned coords
                 info={"feats": feats, "geo": geo, "coords": coords, "conf": conf, "vol": vol, "agg": self.volume_aggregation_method, "NV": NV,
                       "offs": (o_pos, o_cen, o_rot), "step": step, "cmu": cmu, "masked": masked, "entry": entry, "frames": F, "cuboids": B})
        logits = self.volume_net.record(b, vol)
        kp = torch.empty(B, J, 3, dtype=torch.float32, device=device)
        probs = torch.empty(B, J, V, V, V, dtype=torch.float32, device=device)
        ws = torch.empty(1 if dry_run else max(1, lib.lt_softargmax3d_workspace(B, J, V ** 3)), dtype=torch.uint8, device=device)
        mult, sm = float(self.volume_multiplier), int(bool(self.volume_softmax))
        cl = int(logits.t.is_contiguous())   # channels-last rows of J floats, or planar (N, J, V, V, V) storage (bf16 pwchain tail)
        assert cl or logits.t.permute(0, 4, 1, 2, 3).is_contiguous()
        # tail op: the RETURNED features (B, NV, 32, h, w) fp32, contiguous like the reference's (triangulation.py:346,355) -- one liblt_hip layout
        # launch from the plan's channels-last map straight into the tensor forward() hands out (it was a permuted view + an ATen cast copy);
        # skipped when the caller asked for views of the plan's buffers (copy_outputs = False)
        b.custom(lambda st, outs=None: None if not outs or len(outs) < 3 or outs[2] is None else H.check(lib.lt_nhwc_to_nchw_f32(
                     b.code, feats.t.data_ptr(), outs[2].data_ptr(), nimg, 32, h * w, 32, st), "lt_nhwc_to_nchw_f32"),
                 "features_out", nbytes=nimg * h * w * 32 * (esz + 4), info={"feats": feats}, tail=True)
        # tail op (outside the captured graph): forward() points it at the tensors it returns, so the 17 x 64^3 probabilities
        # are written once, where the caller gets them, instead of being cloned out of a plan buffer (0.45 ms of copies per step)
        kstats = kindex = None
        if stats:          # the same tail with the per-joint statistics out of its probabilities pass: records (B, J, 8) and peak voxels (B, J)
            kstats = torch.empty(B, J, 8, dtype=torch.float32, device=device)
            kindex = torch.empty(B, J, dtype=torch.int32, device=device)
            ws = torch.empty(1 if dry_run else max(1, lib.lt_softargmax3d_stats_workspace(B, J, V ** 3)), dtype=torch.uint8, device=device)
            b.custom(lambda st, outs=None: H.check(lib.lt_softargmax3d_stats_fwd(
                         logits.t.data_ptr(), coords.data_ptr(), mult, sm, cl, J, (outs[0] if outs else kp).data_ptr(),
                         (outs[1] if outs else probs).data_ptr(), (outs[3] if outs else kstats).data_ptr(), (outs[4] if outs else kindex).data_ptr(),
                         B, J, V ** 3, ws.data_ptr(), st), "lt_softargmax3d_stats_fwd"),
                     "softargmax3d", nbytes=2 * B * J * V ** 3 * 4 + B * V ** 3 * 12,  # ... + the coordinates once more
                     info={"logits": logits, "coords": coords, "mult": mult, "softmax": sm, "kp": kp, "probs": probs, "entry": "lt_softargmax3d_stats_fwd",
                           "stats": kstats, "peak_index": kindex}, tail=True)
        else:
            b.custom(lambda st, outs=None: H.check(lib.lt_softargmax3d_fwd(
                         logits.t.data_ptr(), coords.data_ptr(), mult, sm, cl, J, (outs[0] if outs else kp).data_ptr(),
                         (outs[1] if outs else probs).data_ptr(), B, J, V ** 3, ws.data_ptr(), st), "lt_softargmax3d_fwd"),
                     "softargmax3d", nbytes=2 * B * J * V ** 3 * 4,  # read logits + write probabilities
                     info={"logits": logits, "coords": coords, "mult": mult, "softmax": sm, "kp": kp, "probs": probs}, tail=True)
        plan = b.finish()
        plan.keep += [geo, geo_ring, coords, kp, probs, ws] + ([kstats, kindex] if stats else [])
        if image_cell is not None and not dry_run:
            x_in.t.untyped_storage().resize_(0)   # the fused stem reads the caller's images: x_in is only a shape (150 MB at B = 32)
        return {"plan": plan, "x_in": x_in, "image_cell": image_cell, "feats": feats, "geo": geo, "geo_host": geo_ring.blocks[0], "geo_ring": geo_ring,
                "coords": coords, "kp": kp, "probs": probs, "conf": conf, "logits": logits, "vol": vol, "hw": (h, w), "offs": (o_pos, o_cen, o_rot),
                "captured": False, "masked": masked, "o_mask": o_mask, "kstats": kstats, "kindex": kindex, "frames": F, "cuboids": B if multi else None,
                "o_fof": o_fof, "ragged": None if ragged is None else nimg, "o_vb": o_vb}

    def _host_cameras(self, batch, B, image_shape, P):
        """The camera half of the host geometry (reference :272-279, :318-328): fills the projections and rotations of the next slot of the plan's
        pinned geometry ring and makes it ``P["geo_host"]``; the slot's cuboid origins and centres are the caller's to fill (``_host_geometry``)
        or to leave to ``lt_cuboid_from_keypoints`` behind the copy (``CascadeTriangulationNet``)."""
        h, w = P["hw"]
        K, R, t = multiview.stack_cameras(batch["cameras"])
        proj = multiview.resized_projections(K, R, t, image_shape, (h, w))
        axis = [0, 1, 0] if self.kind == "coco" else [0, 0, 1]
        nc = P.get("cuboids") or B          # one rotation per cuboid (multi-cuboid plans: B counts the frames)
        rot = np.empty((nc, 9))
        for i in range(nc):
            theta = np.random.uniform(0.0, 2 * np.pi) if self.training else 0.0
            rot[i] = volumetric.get_rotation_matrix(axis, theta).reshape(-1)
        o_pos, o_cen, o_rot = P["offs"]
        gh = P["geo_host"] = P["geo_ring"].acquire()
        gh[:o_pos] = torch.from_numpy(proj.astype(np.float32).reshape(-1))
        gh[o_rot:o_rot + 9 * nc] = torch.from_numpy(rot.astype(np.float32).reshape(-1))
        if P.get("cuboids"):
            gh.view(torch.int32)[P["o_fof"]:P["o_fof"] + nc] = torch.from_numpy(batch["cuboid_frame"])
        if P.get("ragged"):
            gh.view(torch.int32)[P["o_vb"]:P["o_vb"] + B + 1] = torch.from_numpy(batch["view_base"])
        if P.get("masked"):
            gh.view(torch.uint8)[4 * P["o_mask"]:4 * P["o_mask"] + B * len(batch["cameras"])] = torch.from_numpy(batch["view_mask"].reshape(-1))
        return gh

    def _host_geometry(self, batch, B, image_shape, P):
        """numpy fp64 camera / cuboid algebra of the reference (:272-296, :318-328), vectorised; fills the plan's pinned
        geometry block (fp32: projections, cuboid origins, centres, rotations).  Returns (position, base, sides)."""
        kp3d = batch["keypoints_3d"] if self.use_gt_pelvis else batch["pred_keypoints_3d"]
        nc = P.get("cuboids") or B          # multi-cuboid plans: one base point per cuboid
        base = np.empty((nc, 3), dtype=np.float64)
        for i in range(nc):
            k3 = np.asarray(kp3d[i])
            base[i] = (k3[11, :3] + k3[12, :3]) / 2 if self.kind == "coco" else k3[6, :3]
        sides = np.array([self.cuboid_side] * 3)
        position = base - sides / 2
        gh = self._host_cameras(batch, B, image_shape, P)
        o_pos, o_cen, o_rot = P["offs"]
        gh[o_pos:o_cen] = torch.from_numpy(position.astype(np.float32).reshape(-1))
        gh[o_cen:o_rot] = torch.from_numpy(base.astype(np.float32).reshape(-1))
        return position, base, sides

    # ---------------------------------------------------------------------------------------
    def max_samples_per_launch(self, NV, Hh, W):
        """Largest batch of ONE plan.  Since round 6 a plan covers any batch: tensors beyond 2^31 elements (BASELINE config 4 at 32 samples: 32 x 128^3 voxels x
        32 channels = 2^31) are walked in sample chunks inside the convolution entry points (lt_conv_chunk_samples, 64-bit base pointers; the gather, pooling,
        pointwise-chain and soft-argmax kernels index in 64 bits), so the only remaining bound is a single SAMPLE whose widest activation exceeds 32-bit
        offsets -- then 1, and liblt_hip refuses the launch loudly."""
        V = self.volume_size
        per_sample = max(32 * V ** 3, NV * 64 * ((Hh + 1) // 2) * ((W + 1) // 2), NV * 256 * ((Hh + 3) // 4) * ((W + 3) // 4))
        return (1 << 30) if per_sample < MAX_LAUNCH_ELEMS else 1

    def forward(self, images, proj_matricies, batch):
        """images (B,NV,3,H,W) fp32 on the GPU; ``proj_matricies`` is ignored exactly as in the reference
        (overwritten at :277); ``batch`` as built by datasets/utils.py:14-37 (``cameras``, and
        ``pred_keypoints_3d`` or ``keypoints_3d``).  Returns the reference's 7-tuple (:355).

        ``batch["cuboid_frame"]`` (eval(); train() with ``multi_cuboid_training``): several cuboids per frame.  P >= 1 integers in [0, B), any order -- the frame of every cuboid; the joints in
        the batch then have P entries, one base point per cuboid.  The backbone runs on the B frames once; keypoints_3d, volumes, cuboids, coord_volumes and
        base_points come back with P entries, features and vol_confidences with B.  One plan per (B, P); another assignment is another forward of it.

        Asynchronous like the reference's CUDA forward: nothing here waits for the GPU (results are ordered on the current
        stream).  One plan per batch shape whatever its size: BASELINE config 4 at 32 samples (2^31 elements per 32-channel volume) is ONE plan and one
        captured graph -- the convolution entry points walk such tensors in sample chunks (``max_samples_per_launch``)."""
        if isinstance(batch, dict) and batch.get("view_counts") is not None:
            return self._forward_ragged(images, batch)
        B, NV = images.shape[:2]
        cf = _batch_cuboid_frame(batch, B, "VolumetricTriangulationNet")          # optional: several cuboids per frame, refused before any launch
        if cf is not None:
            if _bn_in_train_mode(self) and not self.multi_cuboid_training:
                raise NotImplementedError("VolumetricTriangulationNet: batch['cuboid_frame'] is inference only (there is no indexed unprojection backward); "
                                          "call eval() first")
            key = "keypoints_3d" if self.use_gt_pelvis else "pred_keypoints_3d"
            if len(batch[key]) != len(cf):
                raise ValueError("VolumetricTriangulationNet: batch['cuboid_frame'] names %d cuboids, batch[%r] has %d entries (one base point per cuboid)" %
                                 (len(cf), key, len(batch[key])))
            if max(B, len(cf)) > self.max_samples_per_launch(NV, images.shape[3], images.shape[4]):
                raise ValueError("VolumetricTriangulationNet: a multi-cuboid forward is one plan, and %d frames with %d cuboids would need sub-batches at this "
                                 "shape (max_samples_per_launch); split the call" % (B, len(cf)))
            batch = dict(batch, cuboid_frame=cf)
        vm = _batch_view_mask(batch, B, NV, 1, "VolumetricTriangulationNet")          # optional (B, NV) validity mask: refused before any launch
        if vm is not None:
            if _bn_in_train_mode(self) and not self.masked_training:
                raise NotImplementedError("VolumetricTriangulationNet: batch['view_mask'] is inference only (there is no masked backward); call eval() first")
            batch = dict(batch, view_mask=vm)
        H.require_gpu(images, "images")
        self.last_keypoint_stats = None
        self.__dict__.pop("_chunk_stats", None)
        if _bn_in_train_mode(self):          # any BatchNorm module in train(): the training step (modules left in eval() keep frozen statistics)
            return self._forward_train(images, batch)          # keypoint_stats is ignored there: the training tape is not touched
        _sync_buffers_before_eval(self)
        cap = self.max_samples_per_launch(NV, images.shape[3], images.shape[4])
        if B <= cap or cf is not None:
            with torch.cuda.device(images.device):
                out = self._forward_chunk(images, batch, 0, B)
            self.last_keypoint_stats = self._take_keypoint_stats()
            return out
        n = -(-B // cap)
        size = -(-B // n)            # equal-sized chunks (one plan), a shorter last one only if B does not divide
        if not self.__dict__.get("_warned_sub_batches"):
            import warnings
            warnings.warn("VolumetricTriangulationNet.forward: %d samples exceed the %d per launch that liblt_hip's 32-bit element offsets allow at this "
                          "shape (%d views, %d^3 voxels); running %d consecutive sub-batches of %d (results identical, one plan)" %
                          (B, cap, NV, self.volume_size, n, size), stacklevel=2)
            self.__dict__["_warned_sub_batches"] = True
        parts = []
        with torch.cuda.device(images.device):
            for lo in range(0, B, size):
                parts.append(self._forward_chunk(images, batch, lo, min(B, lo + size)))
        cat = lambda i: torch.cat([p[i] for p in parts], dim=0)
        self.last_keypoint_stats = self._take_keypoint_stats()
        conf = None if parts[0][3] is None else cat(3)
        return cat(0), cat(1), cat(2), conf, [c for p in parts for c in p[4]], cat(5), cat(6)

    def _forward_ragged(self, images, batch):
        """``batch["view_counts"]`` (eval() only): a ragged batch, as mvn.datasets.utils.ragged_batch builds it.  images (T,3,H,W), the views of all samples
        with sample 0's first; ``batch["cameras"]`` a flat list of the T cameras in that order; view_counts the B counts (1..32 each, summing to T); one
        base point per sample.  The backbone runs on the T images and nothing else; sample b gets what the forward gives for that sample on its own views
        alone.  Returns the 7-tuple with features (T,32,h,w) and vol_confidences (T,32) ('conf_norm': normalised over each sample's views), everything
        else per sample.  One plan per (B, T, NVcap), NVcap the smallest of 4, 8, 32 that holds the largest count; other counts are another forward of it."""
        who = "VolumetricTriangulationNet"
        if batch.get("view_mask") is not None:
            raise NotImplementedError("%s: batch['view_counts'] with batch['view_mask']; drop the missing views from the ragged batch instead of masking them" % who)
        if batch.get("cuboid_frame") is not None:
            raise NotImplementedError("%s: batch['view_counts'] with batch['cuboid_frame']; run the multi-cuboid forward on a padded batch with "
                                      "batch['view_mask'] instead" % who)
        if _bn_in_train_mode(self):
            raise NotImplementedError("%s: batch['view_counts'] is inference only (a training tape is recorded per tensor shape); call eval() first, or pad "
                                      "the batch and train with batch['view_mask'] and masked_training" % who)
        if images.dim() != 4:
            raise ValueError("%s: with batch['view_counts'] the images are (T, 3, H, W), got %s" % (who, tuple(images.shape)))
        T, Hh, W = images.shape[0], images.shape[2], images.shape[3]
        counts, base, nvcap = op.view_counts_host(batch["view_counts"], T, what="%s: batch['view_counts']" % who)
        B = counts.size
        key = "keypoints_3d" if self.use_gt_pelvis else "pred_keypoints_3d"
        for k in ("cameras", key):
            if batch.get(k) is None:
                raise ValueError("%s: with batch['view_counts'] the batch needs %r (%s)" %
                                 (who, k, "a flat list of the T cameras" if k == "cameras" else "one base point per sample"))
        cams = batch["cameras"]
        if len(cams) != T or any(isinstance(c, (list, tuple)) for c in cams):
            raise ValueError("%s: with batch['view_counts'] batch['cameras'] is a flat list of the T = %d cameras, got %d entries%s" %
                             (who, T, len(cams), " of lists" if len(cams) and isinstance(cams[0], (list, tuple)) else ""))
        if len(batch[key]) != B:
            raise ValueError("%s: batch['view_counts'] names %d samples, batch[%r] has %d entries (one base point per sample)" % (who, B, key, len(batch[key])))
        if B > self.max_samples_per_launch(nvcap, Hh, W):
            raise ValueError("%s: a ragged forward is one plan, and %d samples would need sub-batches at this shape (max_samples_per_launch); split the call" % (who, B))
        H.require_gpu(images, "images")
        self.last_keypoint_stats = None
        self.__dict__.pop("_chunk_stats", None)
        _sync_buffers_before_eval(self)
        device = images.device
        stats = bool(self.keypoint_stats)
        with torch.cuda.device(device):
            P = self._plan_for(self._plan_key(B, nvcap, Hh, W, device, False, stats, None, T),
                               lambda: self._build_plan(B, nvcap, Hh, W, device, stats=stats, ragged=T))
            # cameras[v][b] with one "sample" of T views: stack_cameras gives the T projections in the batch's order
            position, _, sides = self._host_geometry(dict(batch, cameras=[[c] for c in cams], view_base=base), B, (Hh, W), P)
            cur = torch.cuda.current_stream(device)
            side = self._side_stream(device)
            side.wait_stream(cur)
            x = images if images.dtype == torch.float32 and images.is_contiguous() else images.float().contiguous()
            with torch.cuda.stream(side):
                self._copy_geometry(P, side)
                kp, feats, probs, conf, coords, base_points = self._replay(P, x, B, nvcap, side, cur, view_counts=counts)
            x.record_stream(side)
            cur.wait_stream(side)
        self.last_keypoint_stats = self._take_keypoint_stats()
        return kp, feats, probs, conf, [volumetric.Cuboid3D(position[i], sides) for i in range(B)], coords, base_points

    def _take_keypoint_stats(self):
        """The op.KeypointStats of the forward whose chunks just ran (``_replay`` left each chunk's records behind), chunks concatenated; None for a
        forward without ``keypoint_stats``."""
        recs = self.__dict__.pop("_chunk_stats", None)
        if not recs:
            return None
        one = len(recs) == 2
        return op.keypoint_stats_from_records(recs[0] if one else torch.cat(recs[0::2], dim=0), recs[1] if one else torch.cat(recs[1::2], dim=0))

    def _forward_train(self, images, batch):
        """Training mode (any BatchNorm in train()): fp32, batch statistics, running statistics updated, random cuboid rotation; the
        result carries the autograd node whose backward is liblt_hip's (lt_train.py).  Same 7-tuple as the inference forward.  Every
        ``volume_aggregation_method`` trains: for conf / conf_norm the gradient reaches the backbone through the vol_confidences head as
        well (GlobalAveragePoolingHead, pose_resnet.py:140-174)."""
        # BatchNorm modules in train() use batch statistics (and update the running ones); modules left in eval() normalise with their frozen
        # RUNNING STATISTICS (round 3; lt_train.TrainTape.conv) -- that alone freezes no parameter.  Frozen PARAMETERS are requires_grad_(False): the tape
        # records no gradient for them and no backward in front of the first trainable layer (both are in the plan key below)
        bns = [c for c in self.modules() if isinstance(c, nn.modules.batchnorm._BatchNorm) and c.training]
        if any(c.momentum is None or abs(c.momentum - 0.1) > 1e-12 or not c.track_running_stats or not c.affine for c in bns):
            raise NotImplementedError("BatchNorm with a momentum other than 0.1, without running statistics or without affine parameters")
        params = tuple(self.parameters())
        off = [n for n, t in list(self.named_parameters()) + list(self.named_buffers()) if t.device != images.device]
        if off:
            raise RuntimeError("training updates the parameters where they live: move the model to %s first (model.to(device), as "
                               "train.py:424 does); %d tensors are elsewhere, e.g. %s" % (images.device, len(off), off[0]))
        B, NV = images.shape[:2]
        masked = batch.get("view_mask") is not None          # (forward() let it through: masked_training)
        cf = batch.get("cuboid_frame")                       # (forward() let it through: multi_cuboid_training; checked, one base point per cuboid)
        nc = None if cf is None else len(cf)
        key = self._train_plan_key(B, NV, images.shape[3], images.shape[4], images.device, params, masked, nc)
        if getattr(self, "train_precision", "fp32") not in ("fp32", "bf16", "act16", "fp8v2v"):
            raise ValueError("train_precision must be 'fp32' (the reference's precision), 'bf16' (bf16 MFMA convolutions, fp32 storage), 'act16' (bf16 MFMA "
                             "convolutions AND bf16 activations / activation gradients) or 'fp8v2v' (act16 with V2V's 3x3x3 convolutions on the fp8 MFMA)")
        red = getattr(self, "grad_reducer", None)
        if red is not None:
            # DistributedDataParallel's semantics (reference train.py:453): rank 0's parameters and buffers at "construction" (here: the
            # first training forward with this reducer, unless the caller has attached it already), rank 0's buffers at every forward
            if not red.attached:
                red.attach(self)
            else:
                red.sync_buffers()
            self.__dict__["_buffers_stale"] = True          # this step updates the running statistics per rank: the next eval forward re-syncs
        plans = self.__dict__.setdefault("_train_plans", OrderedDict())
        plan = plans.get(key)
        if plan is None:
            while len(plans) >= 2:
                plans.popitem(last=False)          # frees its activations and gradient buffers
            plan = plans[key] = _VolTrainPlan(self, B, NV, images.shape[3], images.shape[4], images.device, masked=masked, cuboids=nc)
        plans.move_to_end(key)
        kp, probs, feats, coords, base_points = _VolTrainFn.apply(plan, images, batch, *params)
        # every BatchNorm's num_batches_tracked += 1 (what nn.BatchNorm does in train()): ONE liblt_hip launch over a table of the counters'
        # addresses (209 one-element torch kernels per step before); the table is rebuilt only when a buffer has moved
        nbt = [c.num_batches_tracked for c in bns]
        tab_key = tuple(t.data_ptr() for t in nbt)
        tab = self.__dict__.get("_nbt_table")
        if tab is None or tab[0] != tab_key:
            tab = self.__dict__["_nbt_table"] = (tab_key, torch.tensor(tab_key, dtype=torch.int64).to(images.device))
        H.check(H.lib().lt_add_i64_multi(tab[1].data_ptr(), len(nbt), 1, torch.cuda.current_stream(images.device).cuda_stream), "lt_add_i64_multi")
        position, sides = self.__dict__.pop("_train_extra")
        cuboids = [volumetric.Cuboid3D(position[i], sides) for i in range(len(position))]          # (one per cuboid: the frames, or batch["cuboid_frame"]'s P)
        return kp, feats, probs, plan.conf_out, cuboids, coords, base_points

    def _train_plan_key(self, B, NV, Hh, W, device, params, masked=False, cuboids=None):
        """Everything a training plan bakes in.  ``masked``: its tape records the masked unprojection pair (steps with ``batch["view_mask"]`` under
        ``masked_training``); steps without a mask keep their plan: an unmasked key is the tuple it always was.  ``cuboids``: the P of a multi-cuboid step
        over B frames (``batch["cuboid_frame"]`` under ``multi_cuboid_training``); a step without it keeps its key and its tape."""
        key = (B, NV, Hh, W, device, self.volume_size, float(self.cuboid_side), float(self.volume_multiplier),
               bool(self.volume_softmax), self.volume_aggregation_method, bool(self.transfer_cmu_to_human36m), self.num_joints,
               tuple(p.requires_grad for p in params), id(getattr(self, "grad_reducer", None)), getattr(self, "train_precision", "fp32"),
               tuple(c.training for c in self.modules() if isinstance(c, nn.modules.batchnorm._BatchNorm)))
        key = key + ("view_mask",) if masked else key
        return key if cuboids is None else key + ("cuboids", int(cuboids))

    def _chunk_plan(self, images, batch, lo, hi):
        """Samples lo .. hi of the call and the plan of that shape: (images, batch, B, P)."""
        device = images.device
        NV = images.shape[1]
        Hh, W = images.shape[3:]
        if lo != 0 or hi != images.shape[0]:
            images = images[lo:hi]
            batch = dict(batch, cameras=[cams[lo:hi] for cams in batch["cameras"]])
            for k in ("keypoints_3d", "pred_keypoints_3d"):
                if k in batch:
                    batch[k] = batch[k][lo:hi]
            if batch.get("view_mask") is not None:
                batch["view_mask"] = np.ascontiguousarray(batch["view_mask"][lo:hi])
        B = hi - lo
        masked = batch.get("view_mask") is not None
        stats = bool(self.keypoint_stats)
        cf = batch.get("cuboid_frame")          # multi-cuboid forwards are never chunked (forward()): B frames, len(cf) cuboids
        nc = None if cf is None else len(cf)
        # the key: everything a plan bakes in besides the weights (those: the fingerprint inside _plan_for)
        P = self._plan_for(self._plan_key(B, NV, Hh, W, device, masked, stats, nc),
                           lambda: self._build_plan(B, NV, Hh, W, device, masked=masked, stats=stats, cuboids=nc))
        return images, batch, B, P

    def _plan_key(self, B, NV, Hh, W, device, masked=False, stats=False, cuboids=None, ragged=None):
        """``ragged``: the T of a ragged plan of B samples, NV = NVcap (forwards without ``batch["view_counts"]`` keep their key).
        Everything a plan bakes in besides the weights; ``masked``: the plan records the masked gather (forwards without a mask keep their plan);
        ``stats``: its tail is lt_softargmax3d_stats_fwd (``keypoint_stats``; forwards without the flag keep their plan); ``cuboids``: the P of a
        multi-cuboid plan over B frames (forwards without ``batch["cuboid_frame"]`` keep their plan: their key is the tuple it always was)."""
        key = (B, NV, Hh, W, self.compute_dtype, device, self.use_graph, self.volume_size, float(self.cuboid_side),
               float(self.volume_multiplier), bool(self.volume_softmax), self.volume_aggregation_method,
               bool(self.transfer_cmu_to_human36m), self.tile_override, self.num_joints, masked, stats)
        key = key if cuboids is None else key + ("cuboids", int(cuboids))
        return key if ragged is None else key + ("ragged", int(ragged))

    @staticmethod
    def _plan_images(images, B, NV):
        x = images.reshape(B * NV, 3, images.shape[3], images.shape[4])
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.float().contiguous()
        return x

    @staticmethod
    def _copy_geometry(P, side):
        """On the side stream: the filled ring slot to the plan's device block, and the event that frees the slot."""
        P["geo"].copy_(P["geo_host"], non_blocking=True)
        P["geo_ring"].commit(side)

    def _replay(self, P, x, B, NV, side, cur, view_mask=None, view_counts=None):
        """view_counts (ragged plans): the host counts of this forward -- features come back as (T,32,h,w), confidences as (T,32).
        On the side stream, behind the geometry: the plan's launches.  Returns (kp, feats, probs, conf, coords, base_points).  view_mask (masked
        plans): the host mask of this forward, for the returned conf_norm confidences."""
        device = x.device
        h, w = P["hw"]
        st = side.cuda_stream
        if P["image_cell"] is not None:     # the plan's first op reads the images where they are
            P["image_cell"]["ptr"], P["image_cell"]["ref"] = x.data_ptr(), x
        else:
            E.stage_images(x, P["x_in"], st)
        plan = P["plan"]
        if self.use_graph and not P["captured"]:
            plan.run_eager(st)          # warm-up launch outside capture (sets func attributes, loads code objects)
            side.synchronize()
            plan.capture(st)
            P["captured"] = True
        kp, probs, coords = P["kp"], P["probs"], P["coords"]
        kstats, kindex = P.get("kstats"), P.get("kindex")          # plans with keypoint_stats: the records of lt_softargmax3d_stats_fwd
        if self.copy_outputs:       # fresh result tensors like the reference's: the tail ops write them directly
            kp, probs = torch.empty_like(kp), torch.empty_like(probs)
            feats = torch.empty((P["ragged"], 32, h, w) if P.get("ragged") else (B, NV, 32, h, w), dtype=torch.float32, device=device)
            if kstats is not None:
                kstats, kindex = torch.empty_like(kstats), torch.empty_like(kindex)
            plan.run(st, (kp, probs, feats, kstats, kindex))
        else:
            plan.run(st)
            feats = P["feats"].t.reshape(B, NV, h, w, 32).permute(0, 1, 4, 2, 3) if not P.get("ragged") else P["feats"].t.permute(0, 3, 1, 2)
        if kstats is not None:          # left for forward(), which hands them out as last_keypoint_stats (one pair per chunk of the call)
            kstats.record_stream(cur); kindex.record_stream(cur)
            self.__dict__.setdefault("_chunk_stats", []).extend([kstats, kindex])
        conf = P["conf"]
        o_pos, o_cen, o_rot = P["offs"]
        base_points = P["geo"][o_cen:o_rot].reshape(-1, 3).clone()    # fp32(base), from the block that was just copied in
        if self.copy_outputs:
            coords = coords.clone()
            conf = None if conf is None else conf.clone()
        if conf is not None and self.volume_aggregation_method == "conf_norm" and view_counts is not None:
            # normalised over each sample's views: the rows scattered into a zero-filled (B, largest count) batch and summed as the plain forward sums
            # its (B, NV) -- with equal counts that IS the plain forward's tensor, so the same bits
            # (the two index tensors are kept per plan and counts: a forward with the counts of the last one builds and uploads nothing)
            top = int(view_counts.max())
            ck = tuple(int(n) for n in view_counts)
            if P.get("conf_index", (None,))[0] != ck:
                P["conf_index"] = (ck, torch.from_numpy(np.repeat(np.arange(B), view_counts)).to(device),
                                   torch.from_numpy(np.concatenate([i * top + np.arange(n) for i, n in enumerate(view_counts)])).to(device))
            _, seg, slot = P["conf_index"]
            sums = torch.zeros(B * top, conf.shape[-1], dtype=conf.dtype, device=device).index_copy_(0, slot, conf).reshape(B, top, -1).sum(dim=1, keepdim=True)
            conf = conf / sums[:, 0].index_select(0, seg)
        elif conf is not None and self.volume_aggregation_method == "conf_norm":
            if view_mask is not None:          # normalised over the valid views, a masked view's entries 0 (an all-ones mask: the same bits)
                on = torch.from_numpy(view_mask).to(device, non_blocking=True).bool()[:, :, None]
                conf = torch.where(on, conf, torch.zeros((), dtype=conf.dtype, device=device))
            conf = conf / conf.sum(dim=1, keepdim=True)   # the RETURNED confidences are the normalised ones (reference :268-269, :355)
        for t in (kp, probs, coords, feats, base_points, conf):
            if t is not None:
                t.record_stream(cur)     # allocated on the side stream, handed to the caller's stream
        return kp, feats, probs, conf, coords, base_points

    def _forward_chunk(self, images, batch, lo, hi):
        device = images.device
        NV = images.shape[1]
        Hh, W = images.shape[3:]
        images, batch, B, P = self._chunk_plan(images, batch, lo, hi)
        position, base, sides = self._host_geometry(batch, B, (Hh, W), P)
        # ---- device side ----
        cur = torch.cuda.current_stream(device)
        side = self._side_stream(device)
        side.wait_stream(cur)
        x = self._plan_images(images, B, NV)
        with torch.cuda.stream(side):
            self._copy_geometry(P, side)
            kp, feats, probs, conf, coords, base_points = self._replay(P, x, B, NV, side, cur, batch.get("view_mask"))
        x.record_stream(side)
        cur.wait_stream(side)
        cuboids = [volumetric.Cuboid3D(position[i], sides) for i in range(len(position))]
        return kp, feats, probs, conf, cuboids, coords, base_points


class AlgebraicTriangulationNet(_PlannedNet):
    def __init__(self, config, device="cuda:0"):
        super().__init__()
        m = config.model
        self.use_confidences = m.use_confidences
        m.backbone.alg_confidences = bool(self.use_confidences)   # reference :137-141
        m.backbone.vol_confidences = False
        self.backbone = pose_resnet.get_pose_net(m.backbone, device=device)
        self.heatmap_softmax = m.heatmap_softmax
        self.heatmap_multiplier = m.heatmap_multiplier
        # True: an eval forward also leaves the statistics of its joints (op.AlgKeypointStats: per view the 2D heatmap's peak, peak pixel, mass, covariance
        # in image px^2 and the reprojection error; per joint the 3D covariance, the 2D ones pushed through the DLT) in last_keypoint_stats; the 4-tuple
        # keeps its bits.  Ignored in train(), where last_keypoint_stats is None.
        self.keypoint_stats = False
        self.last_keypoint_stats = None
        # True: a train() forward takes batch["view_mask"] -- confidences normalised over each sample's valid views, the DLT of the valid views alone, zero
        # gradient into a masked view's keypoints and confidences (the backbone still runs on every image).  False: a mask in train() is refused.
        self.masked_training = False

    def _build_plan(self, B, NV, Hh, W, device, dry_run=False, masked=False, stats=False, ragged=None):
        """ragged: the plan of forwards with ``batch["view_counts"]`` -- B samples over ``ragged`` = T images in all, NV = NVcap: the launches of T images,
        plus the device block of the B + 1 int32 view offsets and its pinned staging ring (the tail after the plan is then lt_alg_tail_ragged_fwd; other
        counts with the same (B, T, NVcap) are another forward of the plan).
        masked: the plan of forwards with ``batch["view_mask"]`` -- the same launches, plus the mask's device block and its pinned staging ring (the
        tail after the plan is then lt_alg_tail_masked_fwd).
        stats: the plan of forwards with ``keypoint_stats`` -- the same launch list with lt_softargmax2d_stats_fwd in the soft-argmax op's place (the tail
        after the plan is then lt_alg_tail_stats_fwd)."""
        assert ragged is None or not (masked or stats), "a ragged plan has neither a mask nor the statistics"
        N = B * NV if ragged is None else int(ragged)          # images of the backbone pass
        b, x_in = self._open_plan(N, Hh, W, device, dry_run)
        lib = b.lib
        hm, feats, algc, _ = self.backbone.record(b, x_in, want_heatmaps=True)
        b.release(feats)
        J, h, w = hm.shape[4], hm.shape[2], hm.shape[3]
        hm_nchw = torch.empty(N, J, h, w, dtype=torch.float32, device=device)
        b.custom(lambda st: H.check(lib.lt_nhwc_to_nchw_f32(H.LT_F32, hm.t.data_ptr(), hm_nchw.data_ptr(), N, J, h * w, J, st), "lt_nhwc_to_nchw_f32"))
        kp2d = torch.empty(N, J, 2, dtype=torch.float32, device=device)
        probs = torch.empty_like(hm_nchw)
        mult, sm = float(self.heatmap_multiplier), int(bool(self.heatmap_softmax))
        kstats = kindex = None
        if stats:          # the records (N, J, 5) {peak, mass, cxx, cxy, cyy} and peak pixels (N, J) out of the pass that writes the probabilities
            kstats = torch.empty(N, J, 5, dtype=torch.float32, device=device)
            kindex = torch.empty(N, J, dtype=torch.int32, device=device)
            b.custom(lambda st: H.check(lib.lt_softargmax2d_stats_fwd(hm_nchw.data_ptr(), mult, sm, kp2d.data_ptr(), probs.data_ptr(), kstats.data_ptr(),
                                                                      kindex.data_ptr(), N * J, h, w, st), "lt_softargmax2d_stats_fwd"),
                     info={"entry": "lt_softargmax2d_stats_fwd", "stats": kstats, "peak_index": kindex})
        else:
            b.custom(lambda st: H.check(lib.lt_softargmax2d_fwd(hm_nchw.data_ptr(), mult, sm, kp2d.data_ptr(), probs.data_ptr(), N * J, h, w, st),
                                        "lt_softargmax2d_fwd"))
        plan = b.finish()
        plan.keep += [hm_nchw, kp2d, probs] + ([kstats, kindex] if stats else [])
        P = {"plan": plan, "x_in": x_in, "kp2d": kp2d, "probs": probs, "algc": algc, "hw": (h, w), "J": J, "masked": masked, "hm_nchw": hm_nchw,
             "kstats": kstats, "kindex": kindex, "ragged": None if ragged is None else N}
        if ragged is not None:
            P.update({"view_base": torch.zeros(B + 1, dtype=torch.int32, device=device),
                      "view_base_ring": PinnedRing(B + 1, torch.int32, 1 if dry_run else GEO_RING, pin=not dry_run)})
        if masked:
            P.update({"mask": torch.zeros(N, dtype=torch.uint8, device=device),
                      "mask_ring": PinnedRing(N, torch.uint8, 1 if dry_run else GEO_RING, pin=not dry_run)})
        return P

    def forward(self, images, proj_matricies, batch):
        """Returns (keypoints_3d (B,J,3), keypoints_2d (B,NV,J,2) in image pixels, heatmaps (B,NV,J,h,w) after
        softmax, alg_confidences (B,NV,J)) -- reference :149-200."""
        if isinstance(batch, dict) and batch.get("view_counts") is not None:
            return self._forward_ragged(images, proj_matricies, batch)
        device = images.device
        B, NV = images.shape[:2]
        Hh, W = images.shape[3:]
        vm = _batch_view_mask(batch, B, NV, 2, "AlgebraicTriangulationNet")          # optional (B, NV) validity mask: refused before any launch
        if vm is not None and _bn_in_train_mode(self) and not self.masked_training:
            raise NotImplementedError("AlgebraicTriangulationNet: batch['view_mask'] is inference only (there is no masked backward); call eval() first")
        H.require_gpu(images, "images")
        self.last_keypoint_stats = None
        if _bn_in_train_mode(self):
            return self._forward_train(images, proj_matricies, vm)          # keypoint_stats is ignored there
        _sync_buffers_before_eval(self)
        masked, stats = vm is not None, bool(self.keypoint_stats)
        with torch.cuda.device(device):
            P = self._plan_for(self._plan_key(B, NV, Hh, W, device, masked, stats), lambda: self._build_plan(B, NV, Hh, W, device, masked=masked, stats=stats))
            return self._run(P, images, proj_matricies, B, NV, Hh, W, device, vm)

    def _forward_ragged(self, images, proj_matricies, batch):
        """``batch["view_counts"]`` (eval() only): a ragged batch, as mvn.datasets.utils.ragged_batch builds it.  images (T,3,H,W) and proj_matricies
        (T,3,4), the views of all samples with sample 0's first; view_counts the B counts (2..32 each, summing to T).  The backbone runs on the T images and
        nothing else; sample b gets what the forward gives for that sample on its own views alone (lt_alg_tail_ragged_fwd: confidences normalised over the
        sample's views + 1e-5, the DLT over its rows).  Returns keypoints_3d (B,J,3), keypoints_2d (T,J,2), heatmaps (T,J,h,w), alg_confidences (T,J)."""
        who = "AlgebraicTriangulationNet"
        if batch.get("view_mask") is not None:
            raise NotImplementedError("%s: batch['view_counts'] with batch['view_mask']; drop the missing views from the ragged batch instead of masking them" % who)
        if _bn_in_train_mode(self):
            raise NotImplementedError("%s: batch['view_counts'] is inference only (a training tape is recorded per tensor shape); call eval() first, or pad "
                                      "the batch and train with batch['view_mask'] and masked_training" % who)
        if self.keypoint_stats:
            raise NotImplementedError("%s: keypoint_stats with batch['view_counts'] (there is no ragged statistics tail); pad the batch and pass "
                                      "batch['view_mask'] instead, or set keypoint_stats = False" % who)
        if images.dim() != 4:
            raise ValueError("%s: with batch['view_counts'] the images are (T, 3, H, W), got %s" % (who, tuple(images.shape)))
        T, Hh, W = images.shape[0], images.shape[2], images.shape[3]
        counts, base, nvcap = op.view_counts_host(batch["view_counts"], T, min_views=2, what="%s: batch['view_counts']" % who)
        B = counts.size
        if tuple(proj_matricies.shape) != (T, 3, 4):
            raise ValueError("%s: with batch['view_counts'] proj_matricies are (T, 3, 4) = (%d, 3, 4), got %s" % (who, T, tuple(proj_matricies.shape)))
        device = images.device
        H.require_gpu(images, "images")
        self.last_keypoint_stats = None
        _sync_buffers_before_eval(self)
        with torch.cuda.device(device):
            P = self._plan_for(self._plan_key(B, nvcap, Hh, W, device, ragged=T), lambda: self._build_plan(B, nvcap, Hh, W, device, ragged=T))
            h, w = P["hw"]; J = P["J"]
            cur = torch.cuda.current_stream(device)
            st = cur.cuda_stream
            host = P["view_base_ring"].acquire()          # the offsets to their device block through the plan's pinned ring
            host.copy_(torch.from_numpy(base))
            P["view_base"].copy_(host, non_blocking=True)
            P["view_base_ring"].commit(cur)
            E.stage_images(images.float().contiguous(), P["x_in"], st)
            P["plan"].run_eager(st)
            heatmaps = P["probs"].clone()
            algc = P["algc"]
            proj = proj_matricies.to(device, torch.float32).contiguous()
            kp2d = torch.empty(T, J, 2, dtype=torch.float32, device=device)
            conf = torch.empty(T, J, dtype=torch.float32, device=device)
            kp3d = torch.empty(B, J, 3, dtype=torch.float32, device=device)
            H.check(H.lib().lt_alg_tail_ragged_fwd(P["kp2d"].data_ptr(), None if algc is None else algc.t.data_ptr(), J if algc is None else algc.t.shape[-1],
                                                   proj.data_ptr(), W / w, Hh / h, P["view_base"].data_ptr(), kp2d.data_ptr(), conf.data_ptr(), kp3d.data_ptr(),
                                                   B, T, nvcap, J, st), "lt_alg_tail_ragged_fwd")
        return kp3d, kp2d, heatmaps, conf

    def _plan_key(self, B, NV, Hh, W, device, masked=False, stats=False, ragged=None):
        """``ragged``: the T of a ragged plan of B samples, NV = NVcap (forwards without ``batch["view_counts"]`` keep their key).
        ``masked``: the plan carries the mask's block; ``stats``: its soft-argmax op is lt_softargmax2d_stats_fwd (``keypoint_stats``).  Forwards without
        a mask or without the flag keep their plans: an unflagged key is the tuple it always was."""
        key = (B, NV, Hh, W, self.compute_dtype, device, float(self.heatmap_multiplier), bool(self.heatmap_softmax), self.tile_override, masked)
        key = key + ("keypoint_stats",) if stats else key
        return key if ragged is None else key + ("ragged", int(ragged))

    def _forward_train(self, images, proj_matricies, view_mask=None):
        """view_mask (``masked_training``): the checked host (B, NV) mask -- the tape is the unmasked step's (the backbone runs on every image); the tail
        normalises the confidences over each sample's valid views (+ 1e-5 for a valid view, exactly 0 for a masked one, as lt_alg_tail_masked_fwd
        defines) and triangulates the valid views alone; a masked view's 2D keypoints and confidences get zero gradient.

        Training mode (round 3; the reference's loop for model_type "alg", train.py:189-236): the backbone -- heatmap head and, with
        ``use_confidences``, the alg_confidences head included -- runs its recorded training step (lt_train.TrainTape: batch-statistics
        BatchNorm, liblt_hip backward); 2D soft-argmax, confidence normalisation and the DLT are autograd nodes over liblt_hip kernels
        (lt_softargmax2d_bwd, lt_triangulate_dlt_bwd: what autograd derives through torch.svd in the reference).  Same 4-tuple as inference; the returned
        heatmaps (after softmax / ReLU) are differentiable too -- an auxiliary loss.HeatmapMSELoss on them trains through lt_softargmax2d_bwd_full, a
        loss that leaves them alone backpropagates through lt_softargmax2d_bwd exactly as before."""
        # BatchNorm modules in train() use batch statistics (and update the running ones); modules left in eval() normalise with their frozen
        # RUNNING STATISTICS (round 3; lt_train.TrainTape.conv) -- that alone freezes no parameter.  Frozen PARAMETERS are requires_grad_(False): the tape
        # records no gradient for them and no backward in front of the first trainable layer (both are in the plan key below)
        # (the plan cache, the reducer, the num_batches_tracked bump: pose_resnet.backbone_train_step, shared with PoseResNet's own train() forward)
        device = images.device
        B, NV = images.shape[:2]
        Hh, W = images.shape[3:]
        x = images.reshape(B * NV, 3, Hh, W)
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.float().contiguous()
        _, hm, conf_raw = pose_resnet.backbone_train_step(self, x)
        N, J, h, w = hm.shape
        kp2d, heatmaps = op.integrate_tensor_2d(hm * self.heatmap_multiplier, self.heatmap_softmax)      # reference :158
        conf = conf_raw.reshape(B, NV, J) if conf_raw.numel() else torch.ones(B, NV, J, dtype=torch.float32, device=device)
        if view_mask is not None:
            on = torch.from_numpy(view_mask).to(device).bool()[:, :, None]
            zero = torch.zeros((), dtype=torch.float32, device=device)
            conf = torch.where(on, conf, zero)
            conf = torch.where(on, conf / conf.sum(dim=1, keepdim=True) + 1e-5, zero)
            kp2d = kp2d.reshape(B, NV, J, 2) * torch.tensor([W / w, Hh / h], dtype=torch.float32, device=device)
            kp3d = multiview.triangulate_batch_of_points(proj_matricies.to(device), kp2d, confidences_batch=conf, view_mask=view_mask, masked_backward=True)
            return kp3d, kp2d, heatmaps.reshape(B, NV, J, h, w), conf
        conf = conf / conf.sum(dim=1, keepdim=True) + 1e-5                                                 # reference :173-174
        scale = torch.tensor([W / w, Hh / h], dtype=torch.float32, device=device)
        kp2d = kp2d.reshape(B, NV, J, 2) * scale                                                          # reference :181-184
        kp3d = multiview.triangulate_batch_of_points(proj_matricies.to(device), kp2d, confidences_batch=conf)
        return kp3d, kp2d, heatmaps.reshape(B, NV, J, h, w), conf

    def _run(self, P, images, proj_matricies, B, NV, Hh, W, device, view_mask=None):
        h, w = P["hw"]; J = P["J"]
        st = torch.cuda.current_stream(device).cuda_stream
        if view_mask is not None:          # the mask to its device block through the plan's pinned ring
            host = P["mask_ring"].acquire()
            host.copy_(torch.from_numpy(view_mask.reshape(-1)))
            P["mask"].copy_(host, non_blocking=True)
            P["mask_ring"].commit(torch.cuda.current_stream(device))
        E.stage_images(images.reshape(B * NV, 3, Hh, W).float().contiguous(), P["x_in"], st)
        P["plan"].run_eager(st)
        heatmaps = P["probs"].reshape(B, NV, J, h, w).clone()
        # reference :173-193 in one lt_alg_tail_fwd launch: confidences normalised over the views + 1e-5, keypoints to image pixels, the DLT --
        # bit-identical to conf / conf.sum(1) + 1e-5, kp2d * scale, triangulate_batch_of_points (the training path keeps those autograd ops)
        algc = P["algc"]
        proj = proj_matricies.to(device, torch.float32).contiguous()
        kp2d = torch.empty(B, NV, J, 2, dtype=torch.float32, device=device)
        conf = torch.empty(B, NV, J, dtype=torch.float32, device=device)
        kp3d = torch.empty(B, J, 3, dtype=torch.float32, device=device)
        if P.get("kstats") is not None:          # keypoint_stats: the same tail (masked or not) with the reprojection errors and the propagated covariance
            rec, idx = P["kstats"].reshape(B, NV, J, 5).clone(), P["kindex"].reshape(B, NV, J).clone()
            cov2d = torch.empty(B, NV, J, 3, dtype=torch.float32, device=device)
            err = torch.empty(B, NV, J, dtype=torch.float32, device=device)
            cov3d = torch.empty(B, J, 6, dtype=torch.float32, device=device)
            H.check(H.lib().lt_alg_tail_stats_fwd(P["kp2d"].data_ptr(), None if algc is None else algc.t.data_ptr(), J if algc is None else algc.t.shape[-1],
                                                  proj.data_ptr(), W / w, Hh / h, None if view_mask is None else P["mask"].data_ptr(), P["kstats"].data_ptr(),
                                                  kp2d.data_ptr(), conf.data_ptr(), kp3d.data_ptr(), cov2d.data_ptr(), err.data_ptr(), cov3d.data_ptr(),
                                                  B, NV, J, st), "lt_alg_tail_stats_fwd")
            self.last_keypoint_stats = op.alg_keypoint_stats_from_records(rec, idx, cov2d, err, cov3d)
            return kp3d, kp2d, heatmaps, conf
        if view_mask is not None:          # the same tail over the valid views of each sample; masked confidences are 0
            H.check(H.lib().lt_alg_tail_masked_fwd(P["kp2d"].data_ptr(), None if algc is None else algc.t.data_ptr(), J if algc is None else algc.t.shape[-1],
                                                   proj.data_ptr(), W / w, Hh / h, P["mask"].data_ptr(), kp2d.data_ptr(), conf.data_ptr(), kp3d.data_ptr(),
                                                   B, NV, J, st), "lt_alg_tail_masked_fwd")
            return kp3d, kp2d, heatmaps, conf
        H.check(H.lib().lt_alg_tail_fwd(P["kp2d"].data_ptr(), None if algc is None else algc.t.data_ptr(), J if algc is None else algc.t.shape[-1],
                                        proj.data_ptr(), W / w, Hh / h, kp2d.data_ptr(), conf.data_ptr(), kp3d.data_ptr(), B, NV, J, st),
                "lt_alg_tail_fwd")
        return kp3d, kp2d, heatmaps, conf


class RANSACTriangulationNet(_PlannedNet):
    """Reference :17-128.  The backbone and lt_heatmap_argmax_nchw_f32 (raw NCHW heatmaps + argmax keypoints in one pass) are one
    recorded plan; lt_triangulate_ransac then triangulates every (sample, joint) on the same stream (the reference loops over them in
    Python with numpy SVDs and a scipy Huber fit each).  The 2-view hypotheses are every pair in lexicographic order instead of
    n_iters random draws: deterministic, and the inlier set found is at least as large as any the draws can find.  Inference only:
    the reference's RANSAC output carries no gradient."""

    def __init__(self, config, device="cuda:0"):
        super().__init__()
        m = config.model
        m.backbone.alg_confidences = False        # reference :21-22
        m.backbone.vol_confidences = False
        self.backbone = pose_resnet.get_pose_net(m.backbone, device=device)
        self.direct_optimization = m.direct_optimization
        self.reprojection_error_epsilon = 15

    def _build_plan(self, B, NV, Hh, W, device):
        b, x_in = self._open_plan(B * NV, Hh, W, device)
        lib = b.lib
        hm, feats, _, _ = self.backbone.record(b, x_in, want_heatmaps=True)
        b.release(feats)
        N = B * NV
        J, h, w = hm.shape[4], hm.shape[2], hm.shape[3]
        assert hm.t.dtype == torch.float32, hm.t.dtype     # the heatmap head stores fp32 in every compute dtype
        ld = hm.t.shape[-1]
        hm_nchw = torch.empty(N, J, h, w, dtype=torch.float32, device=device)
        kp2d = torch.empty(N, J, 2, dtype=torch.int64, device=device)
        b.custom(lambda st: H.check(lib.lt_heatmap_argmax_nchw_f32(hm.t.data_ptr(), ld, hm_nchw.data_ptr(), None, kp2d.data_ptr(), N, J, h, w,
                                                                   Hh, W, st), "lt_heatmap_argmax_nchw_f32"),
                 "heatmap_argmax", nbytes=2 * N * J * h * w * 4)
        plan = b.finish()
        plan.keep += [hm_nchw, kp2d]
        return {"plan": plan, "x_in": x_in, "hm": hm_nchw, "kp2d": kp2d, "hw": (h, w), "J": J}

    def forward(self, images, proj_matricies, batch):
        """Returns (keypoints_3d (B,J,3) fp32, keypoints_2d (B,NV,J,2) int64 image pixels, raw heatmaps (B,NV,J,h,w), confidences
        (B,NV,J) zeros) -- reference :27-73."""
        _refuse_view_counts(batch, "RANSACTriangulationNet")
        if isinstance(batch, dict) and batch.get("view_mask") is not None:
            raise NotImplementedError("RANSACTriangulationNet takes no batch['view_mask']: its inlier search already drops views per joint")
        H.require_gpu(images, "images")
        if _bn_in_train_mode(self):
            raise NotImplementedError("RANSACTriangulationNet runs in eval() only: its triangulation carries no gradient (the reference "
                                      "ships only an evaluation config for it)")
        _sync_buffers_before_eval(self)
        device = images.device
        B, NV = images.shape[:2]
        Hh, W = images.shape[3:]
        key = (B, NV, Hh, W, self.compute_dtype, device, self.tile_override)
        with torch.cuda.device(device):
            P = self._plan_for(key, lambda: self._build_plan(B, NV, Hh, W, device))
            h, w = P["hw"]; J = P["J"]
            st = torch.cuda.current_stream(device).cuda_stream
            E.stage_images(images.reshape(B * NV, 3, Hh, W).float().contiguous(), P["x_in"], st)
            P["plan"].run_eager(st)
            heatmaps = P["hm"].reshape(B, NV, J, h, w).clone()
            kp2d = P["kp2d"].reshape(B, NV, J, 2).clone()
            kp3d = multiview.triangulate_ransac_batch(proj_matricies.to(device), kp2d, None, self.reprojection_error_epsilon,
                                                      self.direct_optimization)
            conf = torch.zeros(B, NV, J, dtype=torch.float32, device=device)
        return kp3d, kp2d, heatmaps, conf

    def triangulate_ransac(self, proj_matricies, points, n_iters=10, reprojection_error_epsilon=15, direct_optimization=True, device=None):
        """Reference :75-128 for one point: numpy proj_matricies (NV, 3, 4) and points (NV, 2) -> (point (3,) fp64 of the fp32 result,
        sorted inlier view indices).  Runs lt_triangulate_ransac on a 1 x 1 batch; ``n_iters`` is accepted for compatibility -- every
        pair is tried."""
        assert len(proj_matricies) == len(points)
        assert len(points) >= 2
        dev = torch.device(device) if device is not None else next(self.parameters()).device
        if dev.type != "cuda":
            dev = torch.device("cuda", torch.cuda.current_device())
        P = torch.as_tensor(np.asarray(proj_matricies, dtype=np.float32)).to(dev)[None]
        pts = torch.as_tensor(np.asarray(points).astype(np.int64)).to(dev)[None, :, None, :]
        kp, inl = multiview.triangulate_ransac_batch(P, pts, None, reprojection_error_epsilon, direct_optimization, return_inliers=True)
        return kp[0, 0].double().cpu().numpy(), np.nonzero(inl[0, 0].cpu().numpy())[0]


class _LazyCuboids:
    """The ``cuboids`` of a cascade forward: a sequence of ``Cuboid3D(position, sides)`` whose positions are on the GPU until somebody looks.  The
    first access copies the (B, 3) centres to the host -- THAT access waits for the GPU -- and builds the items as ``VolumetricTriangulationNet``
    does: position = fp64(centre) - sides / 2."""

    def __init__(self, base_points, cuboid_side):
        self._base, self._side, self._items = base_points, cuboid_side, None

    def _build(self):
        if self._items is None:
            base = self._base.detach().cpu().numpy().astype(np.float64)
            sides = np.array([self._side] * 3)
            position = base - sides / 2
            self._items = [volumetric.Cuboid3D(position[i], sides) for i in range(len(position))]
            self._base = None
        return self._items

    def __len__(self):
        return len(self._base) if self._items is None else len(self._items)

    def __getitem__(self, i):
        return self._build()[i]

    def __iter__(self):
        return iter(self._build())


class CascadeTriangulationNet(nn.Module):
    """The reference's two-stage evaluation route as ONE forward: its published volumetric numbers centre the cuboid on the pelvis an earlier run
    of the algebraic model wrote to disk (``pred_results_path``, ``use_gt_pelvis: false`` in eval/human36m_vol_softmax.yaml).  Here the algebraic
    stage's joints stay on the GPU: ``lt_cuboid_from_keypoints`` turns them into the volumetric plan's cuboid origins behind the geometry copy, so
    nothing between the two stages waits for the GPU or copies to the host.  Bit-identical to running ``alg``, copying its joints to the host and
    running ``vol`` with them as ``batch["pred_keypoints_3d"]``.

    ``alg`` / ``vol`` are the two existing modules (state-dict keys ``alg.*`` / ``vol.*``; each loads a reference checkpoint as it does alone), with
    their own ``compute_dtype`` / ``use_graph`` / ``copy_outputs``.  Inference only."""

    def __init__(self, alg_net, vol_net):
        super().__init__()
        if not isinstance(alg_net, AlgebraicTriangulationNet) or not isinstance(vol_net, VolumetricTriangulationNet):
            raise TypeError("CascadeTriangulationNet(alg_net, vol_net) takes an AlgebraicTriangulationNet and a VolumetricTriangulationNet")
        if vol_net.kind not in H.KIND:
            raise ValueError("CascadeTriangulationNet: vol_net.kind %r ('mpii' | 'coco')" % (vol_net.kind,))
        need = 13 if vol_net.kind == "coco" else 7
        J = alg_net.backbone.final_layer.out_channels
        if J < need:
            raise ValueError("CascadeTriangulationNet: the algebraic model has %d joints, kind '%s' reads joint %d" % (J, vol_net.kind, need - 1))
        self.alg, self.vol = alg_net, vol_net
        self.last_keypoint_stats = None          # with vol.keypoint_stats: the op.KeypointStats of the last forward's volumetric stage
        self.last_alg_keypoint_stats = None      # with alg.keypoint_stats: the op.AlgKeypointStats of the last forward's algebraic stage

    def forward(self, images, proj_matricies, batch):
        """images (B,NV,3,H,W) fp32 on the GPU; ``proj_matricies`` (B,NV,3,4) at image resolution for the algebraic stage; ``batch`` needs only
        ``cameras`` (``pred_keypoints_3d`` / ``keypoints_3d`` are ignored).  Returns ``(vol_outputs, alg_outputs)``: the 7-tuple of
        ``VolumetricTriangulationNet.forward`` and the 4-tuple of ``AlgebraicTriangulationNet.forward``, same shapes and dtypes.  ``base_points``
        is read from the device block; ``cuboids`` is a sequence that builds its ``Cuboid3D`` items on first access, and that access
        synchronises with the GPU (the forward itself never does, beyond what the two models' forwards do at their first call of a shape)."""
        _refuse_view_counts(batch, "CascadeTriangulationNet")
        B, NV = images.shape[:2]
        if isinstance(batch, dict) and batch.get("cuboid_frame") is not None:
            raise NotImplementedError("CascadeTriangulationNet: batch['cuboid_frame'] is not supported -- the algebraic stage gives ONE pelvis per frame, which "
                                      "cannot centre several cuboids (that needs an association of people across the views); run VolumetricTriangulationNet "
                                      "with one base point per cuboid")
        vm = _batch_view_mask(batch, B, NV, 2, "CascadeTriangulationNet")          # the one mask for both stages, refused before any launch
        if vm is not None:
            batch = dict(batch, view_mask=vm)
        if not _bn_in_train_mode(self):
            H.require_gpu(images, "images")
        else:
            raise NotImplementedError("CascadeTriangulationNet runs in eval() only: train the two stages on their own (the reference trains the "
                                      "volumetric model on pelvises read from a results file)")
        vol = self.vol
        self.last_keypoint_stats = vol.last_keypoint_stats = None
        vol.__dict__.pop("_chunk_stats", None)
        self.last_alg_keypoint_stats = None
        alg_out = self.alg(images, proj_matricies, batch)
        self.last_alg_keypoint_stats = self.alg.last_keypoint_stats
        kp_alg = alg_out[0]
        _sync_buffers_before_eval(vol)
        cap = vol.max_samples_per_launch(NV, images.shape[3], images.shape[4])
        n = -(-B // cap)
        size = -(-B // n)            # the sub-batches of VolumetricTriangulationNet.forward
        parts = []
        with torch.cuda.device(images.device):
            for lo in range(0, B, size):
                parts.append(self._vol_chunk(images, batch, kp_alg, lo, min(B, lo + size)))
        self.last_keypoint_stats = vol.last_keypoint_stats = vol._take_keypoint_stats()
        if len(parts) == 1:
            kp, feats, probs, conf, coords, base_points = parts[0]
        else:
            cat = lambda i: torch.cat([p[i] for p in parts], dim=0)
            kp, feats, probs, conf, coords, base_points = cat(0), cat(1), cat(2), None if parts[0][3] is None else cat(3), cat(4), cat(5)
        cuboids = _LazyCuboids(base_points, vol.cuboid_side)
        return (kp, feats, probs, conf, cuboids, coords, base_points), alg_out

    def _vol_chunk(self, images, batch, kp_alg, lo, hi):
        """VolumetricTriangulationNet._forward_chunk with the pelvis taken on the device: the camera half of the geometry block from the host, its
        cuboid origins and centres from ``lt_cuboid_from_keypoints`` on the side stream behind the block's copy."""
        vol = self.vol
        device = images.device
        NV = images.shape[1]
        Hh, W = images.shape[3:]
        images, batch, B, P = vol._chunk_plan(images, batch, lo, hi)
        vol._host_cameras(batch, B, (Hh, W), P)
        kp_alg = kp_alg[lo:hi]
        if kp_alg.dtype != torch.float32 or not kp_alg.is_contiguous():
            kp_alg = kp_alg.float().contiguous()
        cur = torch.cuda.current_stream(device)
        side = vol._side_stream(device)
        side.wait_stream(cur)          # behind the algebraic stage: its joints are complete when the seam kernel starts
        x = vol._plan_images(images, B, NV)
        o_pos, o_cen, _ = P["offs"]
        gp = P["geo"].data_ptr()
        with torch.cuda.stream(side):
            vol._copy_geometry(P, side)
            H.check(H.lib().lt_cuboid_from_keypoints(kp_alg.data_ptr(), B, kp_alg.shape[1], H.KIND[vol.kind], float(vol.cuboid_side), gp + 4 * o_pos, gp + 4 * o_cen,
                                                     side.cuda_stream), "lt_cuboid_from_keypoints")
            out = vol._replay(P, x, B, NV, side, cur, batch.get("view_mask"))
        kp_alg.record_stream(side)
        x.record_stream(side)
        cur.wait_stream(side)
        return out
