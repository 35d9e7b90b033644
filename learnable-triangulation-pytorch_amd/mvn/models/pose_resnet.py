"""2D backbone with the reference's surface (mvn/models/pose_resnet.py of the reference):
``get_pose_net(config, device)`` -> ``PoseResNet`` whose ``state_dict()`` keys/shapes equal the
reference's, so its checkpoints load with ``strict=True``.

The nn.Conv2d / nn.BatchNorm2d children are PARAMETER CONTAINERS ONLY: ``record()`` walks them once and
emits liblt_hip launches (implicit-GEMM convolutions on MFMA with BatchNorm, bias, residual and ReLU folded
into the epilogue, channels-last activations); ``forward`` replays the recorded plan.
"""
from collections import OrderedDict

import torch
import torch.nn as nn

import lt_engine as E
import lt_hip as H

BN_MOMENTUM = 0.1

# depth -> (block kind, blocks per stage)            (reference :177-181)
resnet_spec = {18: ("basic", [2, 2, 2, 2]), 34: ("basic", [3, 4, 6, 3]), 50: ("bottleneck", [3, 4, 6, 3]),
               101: ("bottleneck", [3, 4, 23, 3]), 152: ("bottleneck", [3, 8, 36, 3])}


def _bn(c):
    return nn.BatchNorm2d(c, momentum=BN_MOMENTUM)


def bn_tuple(bn):
    return E.BnParams(bn)


class ResidualBlock(nn.Module):
    """Bottleneck (1x1, 3x3, 1x1; expansion 4) or BasicBlock (3x3, 3x3) parameter container.
    'simple' style strides the 3x3, 'caffe' style strides the first 1x1 (reference :57-137)."""

    def __init__(self, kind, inplanes, planes, stride=1, downsample=None, caffe=False):
        super().__init__()
        self.kind, self.stride = kind, stride
        if kind == "bottleneck":
            s1, s2 = (stride, 1) if caffe else (1, stride)
            shapes = [(inplanes, planes, 1, s1), (planes, planes, 3, s2), (planes, planes * 4, 1, 1)]
        else:
            shapes = [(inplanes, planes, 3, stride), (planes, planes, 3, 1)]
        self.strides = [s for _, _, _, s in shapes]
        for i, (ci, co, k, s) in enumerate(shapes, 1):
            setattr(self, "conv%d" % i, nn.Conv2d(ci, co, k, s, k // 2, bias=False))
            setattr(self, "bn%d" % i, _bn(co))
        self.downsample = downsample

    expansion = property(lambda self: 4 if self.kind == "bottleneck" else 1)

    def is_identity_bottleneck(self):
        return self.kind == "bottleneck" and self.downsample is None and all(s == 1 for s in self.strides)

    def record(self, b, x, t1=None, next_block=None):
        """Records the block over input ``x``.  ``t1``: this block's first activation relu(bn1(conv1(x))) when the PREVIOUS block's seam launch has already
        produced it (lt_expand_reduce_fwd); ``next_block``: fuse this block's expand with that block's reduce when the plan supports the shape -- the
        return value is then (y, t1 of the next block) instead of y (ResNet layer3's identity blocks: the 4 P-channel tensor is written once and not read
        back by the next block's first convolution)."""
        n = len(self.strides)
        if self.kind == "bottleneck" and self.downsample is None and t1 is None and next_block is None:
            # identity blocks of layer1 / layer2 in bf16 plans: the whole block in one launch, the two bottleneck-width tensors stay in LDS
            convs = [self.conv1.weight, self.conv2.weight, self.conv3.weight]
            if b.can_bottleneck(x, convs, self.strides):
                return b.bottleneck(x, convs, [bn_tuple(self.bn1), bn_tuple(self.bn2), bn_tuple(self.bn3)])
        if self.kind == "bottleneck" and self.downsample is not None and t1 is None and next_block is None:
            # the first block of layer1 (downsample branch, stride 1) in bf16 plans: one launch, the residual branch computed from the tile of x in LDS
            convs = [self.conv1.weight, self.conv2.weight, self.conv3.weight]
            if b.can_bottleneck_ds(x, convs, self.strides, self.downsample[0].weight, self.downsample[0].stride[0]):
                return b.bottleneck_ds(x, convs, [bn_tuple(self.bn1), bn_tuple(self.bn2), bn_tuple(self.bn3)], self.downsample[0].weight,
                                       bn_tuple(self.downsample[1]))
        if t1 is not None or next_block is not None:
            assert self.is_identity_bottleneck()
            if t1 is None:
                t1 = b.conv(x, self.conv1.weight, None, bn_tuple(self.bn1), stride=1, pad=0, relu=True)
            t2 = b.conv(t1, self.conv2.weight, None, bn_tuple(self.bn2), stride=1, pad=1, relu=True)
            b.release(t1)
            if next_block is not None and b.can_expand_reduce(t2, x, self.conv3.weight, next_block.conv1.weight):
                y, t1n = b.expand_reduce(t2, x, self.conv3.weight, bn_tuple(self.bn3), next_block.conv1.weight, bn_tuple(next_block.bn1))
                b.release(t2)
                return y, t1n
            y = b.conv(t2, self.conv3.weight, None, bn_tuple(self.bn3), stride=1, pad=0, relu=True, residual=x)
            b.release(t2)
            return (y, None) if next_block is not None else y
        if self.kind == "bottleneck" and self.downsample is not None:
            # first block of layer2-4 in bf16 plans: the expand and the (strided) downsample branch are ONE pointwise convolution over [t2 | x] (lt_conv_cat2_fwd)
            ds, sds = self.downsample[0], self.downsample[0].stride[0]
            Ho, Wo = (x.shape[2] - 1) // sds + 1, (x.shape[3] - 1) // sds + 1
            if b.can_conv_cat2((x.shape[0], 1, Ho, Wo, self.conv3.weight.shape[1]), self.conv3.weight, x.shape, ds.weight, sds):
                t1 = b.conv(x, self.conv1.weight, None, bn_tuple(self.bn1), stride=self.conv1.stride[0], pad=0, relu=True)
                t2 = b.conv(t1, self.conv2.weight, None, bn_tuple(self.bn2), stride=self.conv2.stride[0], pad=1, relu=True)
                b.release(t1)
                y = b.conv_cat2(t2, self.conv3.weight, bn_tuple(self.bn3), x, ds.weight, bn_tuple(self.downsample[1]), sds)
                b.release(t2)
                return y
        res = x
        if self.downsample is not None:
            res = b.conv(x, self.downsample[0].weight, None, bn_tuple(self.downsample[1]), stride=self.downsample[0].stride[0], pad=0)
        y = x
        for i in range(1, n + 1):
            conv, bn = getattr(self, "conv%d" % i), getattr(self, "bn%d" % i)
            last = i == n
            z = b.conv(y, conv.weight, None, bn_tuple(bn), stride=conv.stride[0], pad=conv.padding[0], relu=True,
                       residual=res if last else None)
            if y is not x:
                b.release(y)
            y = z
        if res is not x:
            b.release(res)
        return y


class GlobalAveragePoolingHead(nn.Module):
    """Confidence head container (reference :140-174); see SURVEY.md section 8f row 3."""

    def __init__(self, in_channels, n_classes):
        super().__init__()
        self.features = nn.Sequential(
            nn.Conv2d(in_channels, 512, 3, stride=1, padding=1), _bn(512), nn.MaxPool2d(2), nn.ReLU(inplace=True),
            nn.Conv2d(512, 256, 3, stride=1, padding=1), _bn(256), nn.MaxPool2d(2), nn.ReLU(inplace=True))
        self.head = nn.Sequential(nn.Linear(256, 512), nn.ReLU(inplace=True), nn.Linear(512, 256), nn.ReLU(inplace=True),
                                  nn.Linear(256, n_classes), nn.Sigmoid())

    def record(self, b, x):
        """x: layer4 output Act.  conv+BN (+ReLU, which commutes with the max pool) -> pool, twice; global
        average; three linears as 1x1 convolutions over an N-pixel map; sigmoid.  Returns Act [1,1,1,N,n]."""
        f = self.features
        y = b.conv(x, f[0].weight, f[0].bias, bn_tuple(f[1]), stride=1, pad=1, relu=True)
        p = b.maxpool(y, 2, 2, 0, nd=2); b.release(y)
        y = b.conv(p, f[4].weight, f[4].bias, bn_tuple(f[5]), stride=1, pad=1, relu=True); b.release(p)
        p = b.maxpool(y, 2, 2, 0, nd=2); b.release(y)
        g = b.global_avgpool(p); b.release(p)           # [1,1,1,N,256]
        h = self.head
        y = b.conv(g, h[0].weight[:, :, None, None], h[0].bias, None, relu=True); b.release(g)
        z = b.conv(y, h[2].weight[:, :, None, None], h[2].bias, None, relu=True); b.release(y)
        o = b.conv(z, h[4].weight[:, :, None, None], h[4].bias, None, sigmoid=True, out_f32=True); b.release(z)
        return o


class BackboneTrainPlan:
    """The training step of a PoseResNet backbone for one input shape (lt_train.TrainTape, recorded once / replayed): images -> heatmap logits
    (N, J, h, w) and, with the ``alg_confidences`` head, its sigmoid output (N, J).  ``model`` owns the step -- its parameters, ``train_precision``
    and ``grad_reducer`` are the tape's -- and ``backbone`` is the PoseResNet it runs: ``model.backbone`` for AlgebraicTriangulationNet (whose tail --
    2D soft-argmax, confidence normalisation, DLT -- runs on the two small outputs as ordinary autograd nodes, mvn.utils.op / multiview), the module
    itself for PoseResNet's own train() forward.  The two outputs are the seeded ones; the feature map and the ``vol_confidences`` head are computed on
    the way and handed out without a gradient (``extras``): a layer whose output nobody seeds records no backward and leaves its parameters without one."""

    def __init__(self, model, N, Hh, W, device, backbone=None):
        self.model, self.N, self.Hh, self.W, self.device = model, N, Hh, W, device
        self.backbone = model.backbone if backbone is None else backbone
        self.tape = None
        self.step_id = 0

    def forward(self, x):
        import lt_train
        model, N, Hh, W, device = self.model, self.N, self.Hh, self.W, self.device
        lib = H.lib()
        st = torch.cuda.current_stream(device).cuda_stream
        first = self.tape is None
        if first:
            prec = getattr(model, "train_precision", "fp32")
            if prec not in ("fp32", "bf16", "act16"):
                raise ValueError("%s.train_precision must be 'fp32', 'bf16' or 'act16' (there is no 3D convolution for 'fp8v2v')" % type(model).__name__)
            mixed = prec != "fp32"
            self.tape = tape = lt_train.TrainTape(device, params=list(model.parameters()), reducer=getattr(model, "grad_reducer", None), mixed=mixed, act16=prec == "act16")
            self.x_in = tape.alloc((N, 1, Hh, W, E.min_cin_of(torch.bfloat16 if mixed else torch.float32)))
            tape.no_grad(self.x_in)
        tape = self.tape
        E.stage_images(x, self.x_in, st)
        if first:
            hm, feats, algc, volc = self.backbone.record(tape, self.x_in, want_heatmaps=True)
            self.hm, self.algc, self.feats, self.volc = hm, algc, feats, volc
            self.g_hm = torch.empty_like(hm.t)
            tape.seed(hm, self.g_hm)
            self.g_conf = None
            if algc is not None:
                self.g_conf = torch.empty_like(algc.t)
                tape.seed(algc, self.g_conf)
        else:
            tape.stream = st
            tape._gather_all("fwd", tape.fwd_jobs)
            tape.replay(tape.fwd_ops)
        self.step_id += 1
        _, _, h, w, J = self.hm.shape
        hm_out = torch.empty(N, J, h, w, dtype=torch.float32, device=device)
        H.check(lib.lt_nhwc_to_nchw_f32(H.LT_F32, self.hm.t.data_ptr(), hm_out.data_ptr(), N, J, h * w, J, st), "lt_nhwc_to_nchw_f32")
        conf_out = self.algc.t.reshape(N, J).clone() if self.algc is not None else torch.empty(0, device=device)
        return hm_out, conf_out

    def extras(self):
        """The outputs of the latest forward that carry no gradient: (features (N, C, h, w) fp32, contiguous like the reference's; vol_confidences
        (N, 32) or None)."""
        N, _, h, w, Cf = self.feats.shape
        st = torch.cuda.current_stream(self.device).cuda_stream
        feats_out = torch.empty(N, Cf, h, w, dtype=torch.float32, device=self.device)
        H.check(H.lib().lt_nhwc_to_nchw_f32(self.tape.acode, self.feats.t.data_ptr(), feats_out.data_ptr(), N, Cf, h * w, Cf, st), "lt_nhwc_to_nchw_f32")
        return feats_out, None if self.volc is None else self.volc.t.reshape(N, -1).float().clone()

    def backward(self, g_hm, g_conf):
        N = self.N
        _, _, h, w, J = self.hm.shape
        lib = H.lib()
        st = torch.cuda.current_stream(self.device).cuda_stream
        if g_hm is None:
            H.check(lib.lt_zero(self.g_hm.data_ptr(), self.g_hm.numel() * 4, st), "lt_zero")
        else:
            g = g_hm.float().contiguous()
            H.check(lib.lt_nchw_to_nhwc(H.LT_F32, g.data_ptr(), self.g_hm.data_ptr(), N, J, h * w, J, st), "lt_nchw_to_nhwc")
        if self.g_conf is not None:
            if g_conf is None:
                H.check(lib.lt_zero(self.g_conf.data_ptr(), self.g_conf.numel() * 4, st), "lt_zero")
            else:
                self.g_conf.view(N, J).copy_(g_conf.float())
        pg = self.tape.run_backward()
        flat = self.tape.arena.clone()          # autograd gets its own copy: the arena is overwritten by the next step
        off = self.tape.arena.data_ptr()
        return {p: flat[(v.data_ptr() - off) // 4:(v.data_ptr() - off) // 4 + v.numel()].view(v.shape) for p, v in pg.items()}


class BackboneTrainFn(torch.autograd.Function):
    """The training-mode backbone as ONE autograd node (the counterpart of triangulation._VolTrainFn).  Inputs: (plan, images (N,3,H,W),
    *parameters); outputs: heatmap logits (N,J,h,w), raw confidences (N,J) (empty without the head)."""

    @staticmethod
    def forward(ctx, plan, x, *params):
        ctx.set_materialize_grads(False)
        with torch.cuda.device(x.device):
            hm, conf = plan.forward(x)
        ctx.plan, ctx.step_id, ctx.params = plan, plan.step_id, params
        if conf.numel() == 0:
            ctx.mark_non_differentiable(conf)
        return hm, conf

    @staticmethod
    def backward(ctx, g_hm, g_conf):
        plan = ctx.plan
        if ctx.step_id != plan.step_id:
            raise RuntimeError("only the LATEST training forward of a shape can be backpropagated (its activations live in the plan's buffers, "
                               "which a newer forward has overwritten)")
        with torch.cuda.device(plan.device):
            pg = plan.backward(g_hm, g_conf)
        return (None, None) + tuple(pg.get(p) if p.requires_grad else None for p in ctx.params)


def backbone_train_step(model, x, backbone=None):
    """One recorded training forward of ``model``'s backbone on x (N,3,H,W) fp32 contiguous: (plan, heatmap logits (N,J,h,w), raw alg_confidences (N,J)
    or an empty tensor), both outputs differentiable with respect to ``model``'s parameters.  Everything around the tape that both users share:

    BatchNorm modules in train() use batch statistics (and update the running ones, ``num_batches_tracked`` included); modules left in eval() normalise
    with their frozen RUNNING STATISTICS (lt_train.TrainTape.conv) -- that alone freezes no parameter.  Frozen PARAMETERS are requires_grad_(False): the
    tape records no gradient for them and no backward in front of the first trainable layer (both are in the plan key).  ``model.grad_reducer`` gets
    DistributedDataParallel's semantics; ``model.train_precision`` picks the tape's precision; at most two plans per model are kept (LRU)."""
    bns = [c for c in model.modules() if isinstance(c, nn.modules.batchnorm._BatchNorm) and c.training]
    if any(c.momentum is None or abs(c.momentum - 0.1) > 1e-12 or not c.track_running_stats or not c.affine for c in bns):
        raise NotImplementedError("BatchNorm with a momentum other than 0.1, without running statistics or without affine parameters")
    params = tuple(model.parameters())
    device = x.device
    off = [n for n, t in list(model.named_parameters()) + list(model.named_buffers()) if t.device != device]
    if off:
        raise RuntimeError("training updates the parameters where they live: move the model to %s first (model.to(device), as "
                           "train.py:424 does); %d tensors are elsewhere, e.g. %s" % (device, len(off), off[0]))
    N, _, Hh, W = x.shape
    red = getattr(model, "grad_reducer", None)
    if red is not None:          # DistributedDataParallel's semantics, as in the volumetric model
        if not red.attached:
            red.attach(model)
        else:
            red.sync_buffers()
        model.__dict__["_buffers_stale"] = True          # this step updates the running statistics per rank: the next eval forward re-syncs
    key = (N, Hh, W, device, tuple(p.requires_grad for p in params), id(red), getattr(model, "train_precision", "fp32"),
           tuple(c.training for c in model.modules() if isinstance(c, nn.modules.batchnorm._BatchNorm)))
    plans = model.__dict__.setdefault("_train_plans", OrderedDict())
    plan = plans.get(key)
    if plan is None:
        while len(plans) >= 2:
            plans.popitem(last=False)
        plan = plans[key] = BackboneTrainPlan(model, N, Hh, W, device, backbone=backbone)
    plans.move_to_end(key)
    hm, conf_raw = BackboneTrainFn.apply(plan, x, *params)
    nbt = [c.num_batches_tracked for c in bns]
    tab_key = tuple(t.data_ptr() for t in nbt)
    tab = model.__dict__.get("_nbt_table")
    if tab is None or tab[0] != tab_key:
        tab = model.__dict__["_nbt_table"] = (tab_key, torch.tensor(tab_key, dtype=torch.int64).to(device))
    H.check(H.lib().lt_add_i64_multi(tab[1].data_ptr(), len(nbt), 1, torch.cuda.current_stream(device).cuda_stream), "lt_add_i64_multi")
    return plan, hm, conf_raw


class PoseResNet(E.PlanCache):
    def __init__(self, block_kind, layers, num_joints, num_input_channels=3, deconv_with_bias=False, num_deconv_layers=3,
                 num_deconv_filters=(256, 256, 256), num_deconv_kernels=(4, 4, 4), final_conv_kernel=1,
                 alg_confidences=False, vol_confidences=False, caffe=False):
        super().__init__()
        assert all(k == 4 for k in num_deconv_kernels), "only the 4x4 stride-2 deconvolution of the reference configs"
        self.num_joints, self.num_input_channels = num_joints, num_input_channels
        self.block_kind, self.caffe = block_kind, caffe
        exp = 4 if block_kind == "bottleneck" else 1
        self.conv1 = nn.Conv2d(num_input_channels, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = _bn(64)
        inplanes = 64
        for li, (planes, nb) in enumerate(zip((64, 128, 256, 512), layers), 1):
            stride = 1 if li == 1 else 2
            blocks = []
            for bi in range(nb):
                st = stride if bi == 0 else 1
                ds = None
                if bi == 0 and (st != 1 or inplanes != planes * exp):
                    ds = nn.Sequential(nn.Conv2d(inplanes, planes * exp, kernel_size=1, stride=st, bias=False), _bn(planes * exp))
                blocks.append(ResidualBlock(block_kind, inplanes, planes, st, ds, caffe))
                inplanes = planes * exp
            setattr(self, "layer%d" % li, nn.Sequential(*blocks))
        if alg_confidences:
            self.alg_confidences = GlobalAveragePoolingHead(inplanes, num_joints)
        if vol_confidences:
            self.vol_confidences = GlobalAveragePoolingHead(inplanes, 32)
        dl = []
        for i in range(num_deconv_layers):
            dl += [nn.ConvTranspose2d(inplanes, num_deconv_filters[i], kernel_size=4, stride=2, padding=1, output_padding=0,
                                      bias=deconv_with_bias), _bn(num_deconv_filters[i]), nn.ReLU(inplace=True)]
            inplanes = num_deconv_filters[i]
        self.deconv_layers = nn.Sequential(*dl)
        self.final_layer = nn.Conv2d(inplanes, num_joints, kernel_size=final_conv_kernel, stride=1,
                                     padding=1 if final_conv_kernel == 3 else 0)
        self.compute_dtype = torch.float32
        self._init_plan_cache()

    # ---- plan recording -------------------------------------------------------------------
    def record(self, b, x, want_heatmaps=True, image_cell=None):
        """x: Act [N,1,H,W,Cpad] (zero-padded input channels).  Returns (heatmaps Act fp32 | None,
        features Act, alg_conf Act | None, vol_conf Act | None).  image_cell: see PlanBuilder.stem_pool (the fused stem reads
        the caller's fp32 images directly; x is then only a shape)."""
        if b.can_stem_pool(x, self.conv1.weight, 2, 3, (3, 2, 1)):   # bf16: conv1 + bn1 + relu + maxpool in one pass
            y = b.stem_pool(x, self.conv1.weight, bn_tuple(self.bn1), image_cell=image_cell)
        else:
            y = b.conv(x, self.conv1.weight, None, bn_tuple(self.bn1), stride=2, pad=3, relu=True)
            p = b.maxpool(y, 3, 2, 1, nd=2); b.release(y)
            y = p
        for li in range(1, 5):
            blocks = list(getattr(self, "layer%d" % li))
            t1 = None                                         # the next block's first activation, when the seam launch in front of it produced it
            for bi, blk in enumerate(blocks):
                nxt = blocks[bi + 1] if bi + 1 < len(blocks) else None
                # a run of identity bottleneck blocks whose seams lt_expand_reduce_fwd covers (ResNet layer3, bf16 plans): expand(i) + reduce(i + 1) in one launch
                chain = (nxt is not None and blk.is_identity_bottleneck() and nxt.is_identity_bottleneck() and
                         tuple(blk.conv3.weight.shape[:2]) == (1024, 256) and tuple(nxt.conv1.weight.shape[:2]) == (256, 1024) and b.dtype == torch.bfloat16 and
                         not b.live_weights)
                if chain:
                    z, t1n = blk.record(b, y, t1=t1, next_block=nxt)
                elif t1 is not None:
                    z, t1n = blk.record(b, y, t1=t1), None
                else:
                    z, t1n = blk.record(b, y), None
                b.release(y)
                y, t1 = z, t1n
        alg = self.alg_confidences.record(b, y) if hasattr(self, "alg_confidences") else None
        vol = self.vol_confidences.record(b, y) if hasattr(self, "vol_confidences") else None
        for i in range(0, len(self.deconv_layers), 3):
            dc, bn = self.deconv_layers[i], self.deconv_layers[i + 1]
            z = b.conv(y, dc.weight, dc.bias, bn_tuple(bn), stride=2, pad=1, transposed=True, relu=True)
            b.release(y)
            y = z
        feats = y
        hm = None
        if want_heatmaps:
            fl = self.final_layer
            hm = b.conv(feats, fl.weight, fl.bias, None, stride=1, pad=fl.padding[0], out_f32=True)
        return hm, feats, alg, vol

    def heatmap_shape(self, h, w):
        def down(v, k, s, p):
            return (v + 2 * p - k) // s + 1
        for k, s, p in ((7, 2, 3), (3, 2, 1), (3, 2, 1), (3, 2, 1), (3, 2, 1)):
            h, w = down(h, k, s, p), down(w, k, s, p)
        return h * 8, w * 8

    # ---- stand-alone forward (reference :293-318) --------------------------------------------
    def forward(self, x):
        """x: (N,3,H,W) fp32 on the GPU -> (heatmaps (N,J,h,w), features (N,256,h,w), alg_confidences, vol_confidences).

        In train() the module runs its recorded training step (BackboneTrainPlan: batch-statistics BatchNorm, running statistics updated, liblt_hip
        backward) and returns the same 4-tuple: ``heatmaps`` are the raw logits and differentiable -- train them with loss.HeatmapMSELoss -- and so are
        the ``alg_confidences`` when the head exists.  ``features`` and ``vol_confidences`` are returned WITHOUT a grad_fn: nothing in the 2D training of
        the reference puts a loss on them, and parameters that feed only them (the vol_confidences head) end the step with ``grad is None``, as autograd
        leaves parameters no loss depends on.  Only the latest forward of a shape can be backpropagated.  ``train_precision`` ('fp32' / 'bf16' / 'act16'),
        ``grad_reducer`` and requires_grad_(False) work as on AlgebraicTriangulationNet (backbone_train_step)."""
        H.require_gpu(x, "images")
        if self.training:
            xs = x if x.dtype == torch.float32 and x.is_contiguous() else x.float().contiguous()
            plan, hm, conf_raw = backbone_train_step(self, xs, backbone=self)
            with torch.cuda.device(x.device):
                feats, volc = plan.extras()
            return hm, feats, (conf_raw if conf_raw.numel() else None), volc
        key =(tuple(x.shape), self.compute_dtype, x.device)
        N, _, Hh, W = x.shape

        def build():
            b = E.PlanBuilder(x.device, self.compute_dtype)
            inp = b.alloc((N, 1, Hh, W, E.min_cin_of(self.compute_dtype)))
            outs = self.record(b, inp, True)
            return {"plan": b.finish(), "inp": inp, "outs": outs}

        with torch.cuda.device(x.device):    # launches go to x's device whatever the caller's current device is
            P = self._plan_for(key, build)
            plan, inp, (hm, feats, alg, vol) = P["plan"], P["inp"], P["outs"]
            st = torch.cuda.current_stream(x.device).cuda_stream
            E.stage_images(x.float().contiguous(), inp, st)
            plan.run_eager(st)
            to_nchw = lambda a: a.t[:, 0].permute(0, 3, 1, 2).to(torch.float32, copy=True)
            conf = lambda a: None if a is None else a.t.reshape(N, -1).clone()
            return to_nchw(hm), to_nchw(feats), conf(alg), conf(vol)


def get_pose_net(config, device="cuda:0"):
    """Same contract as the reference's get_pose_net (:321-377): builds the network for
    ``config.num_layers`` / ``config.style`` and optionally loads a pretrained checkpoint, keeping only
    shape-compatible tensors, stripping ``module.`` and partially copying the final layer."""
    kind, layers = resnet_spec[config.num_layers]
    if config.style == "caffe":
        kind = "bottleneck"   # the reference swaps in Bottleneck_CAFFE (expansion 4) at EVERY depth, 18 and 34 included (:322-324)
    model = PoseResNet(kind, layers, config.num_joints, num_input_channels=3, deconv_with_bias=False, num_deconv_layers=3,
                       num_deconv_filters=(256, 256, 256), num_deconv_kernels=(4, 4, 4), final_conv_kernel=1,
                       alg_confidences=config.alg_confidences, vol_confidences=config.vol_confidences,
                       caffe=(config.style == "caffe"))
    if config.init_weights:
        print("Loading pretrained weights from: {}".format(config.checkpoint))
        own = model.state_dict()
        loaded = torch.load(config.checkpoint, map_location="cpu")
        loaded = loaded.get("state_dict", loaded)
        picked = {}
        for k, v in loaded.items():
            name = k.replace("module.", "")
            if name in own and v.shape == own[name].shape:
                picked[name] = v
            elif name in ("final_layer.weight", "final_layer.bias"):
                print("Reiniting final layer:", k)
                o = torch.zeros_like(own[name])
                if name.endswith("weight"):
                    nn.init.xavier_uniform_(o)
                n = min(o.shape[0], v.shape[0])
                o[:n] = v[:n]
                picked[name] = o
        missing = {k.replace("module.", "") for k in loaded} - set(picked)
        if missing:
            print("Parameters [{}] were not inited".format(missing))
        model.load_state_dict(picked, strict=False)
        print("Successfully loaded pretrained weights for backbone")
    return model
