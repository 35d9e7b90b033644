"""lt_unproject_bwd with 9 to 32 camera views on the GPU: the many-view K1 (views in passes for softmax / max, in groups of eight for sum / conf /
conf_norm), the many-view confidence finalizer and the many-view scatter.  Reference: torch autograd through oracle.vol_oracle.unproject_heatmaps in fp64;
gate max|d| <= 1e-4 * max|ref| (the gate of tests/test_gpu_backward.py).  The same oracle in fp32 stays within 1.5e-5 of fp64 on every case and aggregation
here, every view receives a gradient and no 'max' winner flips between fp32 and fp64, so the gate leaves room for an fp32 kernel and hides nothing."""
import pytest
import torch

import lt_hip as H
from gpu_util import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
O = __import__("oracle.vol_oracle", fromlist=["x"])
synth = __import__("oracle.synth", fromlist=["x"])

AGGS = ("sum", "max", "softmax", "conf", "conf_norm")
OP_AGGS = ("sum", "max", "softmax", "conf")
B = 2
CASES = [  # (NV, C, (h, w), vshape)
    (9, 32, (12, 12), (6, 6, 6)),          # the first count past the limit; a partial brick
    (12, 4, (20, 37), (5, 6, 7)),          # one lane per voxel; ragged tiles and bricks
    (17, 16, (33, 16), (8, 8, 8)),         # an odd count across three groups of eight
    (32, 64, (17, 40), (9, 4, 6)),         # the upper limit; the one-hit-at-a-time gather
    (31, 32, (24, 24), (16, 16, 16)),      # CMU's camera count at the model's channel width
]
SCATTER_ONLY = (9, 12, (12, 12), (6, 6, 6))          # C not a power of two: the scatter serves it
IDS = ["NV%d_C%d" % c[:2] for c in CASES]
_REF, _INPUTS = {}, {}


def case(B, NV, C, hw, vshape, seed):
    g = torch.Generator().manual_seed(seed); h, w = hw
    K, R, t = synth.ring_cameras(NV, 96, inside=True)          # camera 0 inside the grid: depth <= 0 voxels
    P = torch.from_numpy(O.resized_projection(K, R, t, (96, 96), (h, w))).float()[None].repeat(B, 1, 1, 1).contiguous()
    hm = torch.randn(B, NV, C, h, w, generator=g); conf = torch.rand(B, NV, C, generator=g) + 0.1
    ax = [torch.linspace(-900.0, 900.0, n) for n in vshape]
    cv = torch.stack(torch.meshgrid(*ax, indexing="ij"), dim=-1)[None].repeat(B, 1, 1, 1, 1).contiguous(); cv[1] += 37.0
    G = torch.randn(B, C, *vshape, generator=g)
    return hm, P, cv, conf, G


def _inputs(c):
    """The case's host tensors, made once and never written to."""
    if c not in _INPUTS:
        _INPUTS[c] = case(B, c[0], c[1], c[2], c[3], seed=500 + c[0])
    return _INPUTS[c]


def _reference(c, agg, bf16=False):
    """d/d features and d/d confidences by fp64 autograd through the oracle (computed once per case / aggregation and shared).  conf_norm: method conf
    on the confidences divided by their sum over the views."""
    key = (c, agg, bf16)
    if key not in _REF:
        hm, P, cv, conf, G = _inputs(c)
        h64 = (hm.bfloat16() if bf16 else hm).double().requires_grad_(True)
        c64 = conf.double().requires_grad_(True) if agg.startswith("conf") else None
        cin = c64 / c64.sum(dim=1, keepdim=True) if agg == "conf_norm" else c64
        vol = O.unproject_heatmaps(h64, P.double(), cv.double(), "conf" if agg == "conf_norm" else agg, cin, dtype=torch.float64)
        (vol * G.double()).sum().backward()
        _REF[key] = (h64.grad, None if c64 is None else c64.grad)
    return _REF[key]


def _entry(hm, P, cv, conf, G, agg, ws_samples=None, expect=0):
    """lt_unproject_bwd itself (every aggregation code, LT_AGG_CONF_NORM included): device tensors in the public layouts in, (grad_feats (B,NV,C,h,w),
    grad_conf or None) out.  ws_samples: workspace of exactly that many samples' share (None: the whole batch's)."""
    Bn, NV, C, h, w = hm.shape
    feats = hm.permute(0, 1, 3, 4, 2).contiguous()
    g = G.permute(0, 2, 3, 4, 1).float().contiguous()
    v0, v1, v2 = cv.shape[1:4]
    gf = torch.full((Bn, NV, h, w, C), float("nan"), dtype=torch.float32, device=hm.device)
    is_conf = agg.startswith("conf")
    gc = torch.full((Bn, NV, C), float("nan"), dtype=torch.float32, device=hm.device) if is_conf else None
    lib = H.lib()
    per_sample = lib.lt_unproject_bwd_workspace(1, NV, C, v0, v1, v2)
    nws = per_sample * (Bn if ws_samples is None else ws_samples)
    ws = torch.empty(max(16, nws), dtype=torch.uint8, device=hm.device)
    rc = lib.lt_unproject_bwd(H.dtype_code(hm.dtype), feats.data_ptr(), P.data_ptr(), cv.data_ptr(), conf.data_ptr() if is_conf else None, g.data_ptr(),
                              gf.data_ptr(), H.ptr(gc), Bn, NV, C, h, w, v0, v1, v2, H.AGG[agg], ws.data_ptr(), nws, torch.cuda.current_stream().cuda_stream)
    if expect != 0:
        assert rc == expect, (rc, lib.lt_last_error())
        return None, None
    H.check(rc, "lt_unproject_bwd")
    torch.cuda.synchronize()
    return gf.permute(0, 1, 4, 2, 3), gc


def _op(hm, P, cv, conf, G, agg):
    """The autograd path of op.unproject_heatmaps."""
    from mvn.utils import op
    f = hm.clone().requires_grad_(True)
    c = conf.clone().requires_grad_(True) if agg == "conf" else None
    (op.unproject_heatmaps(f, P, cv, agg, c) * G).sum().backward()
    return f.grad.clone(), (None if c is None else c.grad.clone())


def _run(dev, agg):
    return _entry(*dev, agg) if agg == "conf_norm" else _op(*dev, agg)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_many_view_backward_vs_fp64_autograd_and_bitwise_repeatable(c):
    hm, P, cv, conf, G = _inputs(c)
    NV = c[0]
    # the facts the gate rests on: camera 0 sees part of the grid at depth <= 0, and every view receives a gradient
    z0 = [torch.cat([cv[b].reshape(-1, 3).double(), torch.ones(cv[b][..., 0].numel(), 1, dtype=torch.float64)], 1) @ P[0, 0, 2].double() for b in range(B)]
    n_behind = [int((z <= 0).sum()) for z in z0]
    print("NV=%d: voxels at depth <= 0 in view 0, per sample: %s" % (NV, n_behind))
    assert 60 <= n_behind[0] <= 1108 and 0 < n_behind[1] < z0[1].numel(), n_behind
    dev = [t.to(DEV) for t in (hm, P, cv, conf, G)]
    for agg in AGGS:
        rf, rc = _reference(c, agg)
        assert all(float(rf[:, v].abs().max()) > 0 for v in range(NV)), agg
        gf, gc = _run(dev, agg)
        e = check("bwd/unproject many views NV=%d C=%d %s: d/d features" % (NV, c[1], agg), gf.cpu(), rf, 1e-4)
        print("NV=%d C=%d %s: d/d features max|d|/max|ref| = %.3e" % (NV, c[1], agg, e))
        if agg.startswith("conf"):
            e = check("bwd/unproject many views NV=%d C=%d %s: d/d confidences" % (NV, c[1], agg), gc.cpu(), rc, 1e-4)
            print("NV=%d C=%d %s: d/d confidences max|d|/max|ref| = %.3e" % (NV, c[1], agg, e))
        else:
            assert gc is None
        gf2, gc2 = _run(dev, agg)
        assert torch.equal(gf, gf2), "%s NV=%d: d/d features not bitwise repeatable" % (agg, NV)
        assert gc is None or torch.equal(gc, gc2), "%s NV=%d: d/d confidences not bitwise repeatable" % (agg, NV)


@pytest.mark.parametrize("c,groups", [(CASES[1], (4, 4, 4)), (CASES[2], (8, 8, 1))], ids=["NV12_as_4+4+4", "NV17_as_8+8+1"])
def test_separable_aggregations_equal_the_register_kernels_bit_for_bit(c, groups):
    """sum and conf: a view's dx, its gather and its confidence gradient do not depend on the other views, so the one many-view call gives each view the
    bits that the 4- and 8-view kernels give when the same views are run as separate calls.  grad_conf is torch.equal as well: the many-view K1 keeps the
    8-view kernel's workgroup count, lane mapping and fp64 partial order."""
    hm, P, cv, conf, G = [t.to(DEV) for t in _inputs(c)]
    for agg in ("sum", "conf"):
        gf, gc = _op(hm, P, cv, conf, G, agg)
        v0 = 0
        for n in groups:
            sl = slice(v0, v0 + n)
            pf, pc = _op(hm[:, sl].contiguous(), P[:, sl].contiguous(), cv, conf[:, sl].contiguous(), G, agg)
            assert torch.equal(gf[:, sl], pf), "%s views %d..%d: d/d features differ from the %d-view call" % (agg, v0, v0 + n - 1, n)
            if agg == "conf":
                assert torch.equal(gc[:, sl], pc), "conf views %d..%d: d/d confidences differ from the %d-view call" % (v0, v0 + n - 1, n)
            v0 += n
        assert v0 == c[0]


def test_chunked_batch_equals_the_whole_batch_bit_for_bit():
    """A workspace of exactly one sample's share: the entry walks the batch sample by sample, and nothing changes."""
    dev = [t.to(DEV) for t in _inputs(CASES[0])]
    for agg in AGGS:
        gf, gc = _entry(*dev, agg)
        cf, cc = _entry(*dev, agg, ws_samples=1)
        assert torch.isfinite(cf).all()
        assert torch.equal(gf, cf), agg
        assert gc is None or torch.equal(gc, cc), agg


@pytest.mark.parametrize("c", [CASES[0], CASES[4]], ids=[IDS[0], IDS[4]])
def test_bf16_feature_maps(c):
    """dtype = LT_BF16 (the gradients stay fp32) against the fp64 oracle on the bf16-rounded maps, same gate."""
    hm, P, cv, conf, G = _inputs(c)
    dev = [hm.bfloat16().to(DEV)] + [t.to(DEV) for t in (P, cv, conf, G)]
    for agg in AGGS:
        rf, rc = _reference(c, agg, bf16=True)
        gf, gc = _entry(*dev, agg)
        assert gf.dtype == torch.float32
        e = check("bwd/unproject many views bf16 NV=%d %s: d/d features" % (c[0], agg), gf.cpu(), rf, 1e-4)
        print("bf16 NV=%d %s: d/d features max|d|/max|ref| = %.3e" % (c[0], agg, e))
        if agg.startswith("conf"):
            e = check("bwd/unproject many views bf16 NV=%d %s: d/d confidences" % (c[0], agg), gc.cpu(), rc, 1e-4)
            print("bf16 NV=%d %s: d/d confidences max|d|/max|ref| = %.3e" % (c[0], agg, e))


@pytest.mark.parametrize("c", [SCATTER_ONLY, CASES[0]], ids=["NV9_C12", "NV9_C32_atomics"])
def test_scatter_path(c, monkeypatch):
    """The float-atomics fallback at 9 views: C = 12 goes there by itself, C = 32 under LT_UNPROJ_BWD_ATOMICS=1 (also against the gather at 2e-5, the
    existing gate between the two); conf_norm stays unsupported there."""
    dev = [t.to(DEV) for t in _inputs(c)]
    gather = {agg: _op(*dev, agg) for agg in OP_AGGS} if c[1] == 32 else None
    monkeypatch.setenv("LT_UNPROJ_BWD_ATOMICS", "1")
    for agg in OP_AGGS:
        rf, rc = _reference(c, agg)
        gf, gc = _op(*dev, agg)
        check("bwd/unproject many views scatter C=%d %s: d/d features" % (c[1], agg), gf.cpu(), rf, 1e-4)
        if agg == "conf":
            check("bwd/unproject many views scatter C=%d conf: d/d confidences" % c[1], gc.cpu(), rc, 1e-4)
        if gather is not None:
            check("bwd/unproject many views gather vs scatter %s: d/d features" % agg, gather[agg][0].cpu(), gf.cpu(), 2e-5)
            if agg == "conf":
                check("bwd/unproject many views gather vs scatter conf: d/d confidences", gather[agg][1].cpu(), gc.cpu(), 2e-5)
    _entry(*dev, "conf_norm", expect=-2)          # LT_ERR_UNSUPPORTED
    assert b"conf_norm" in H.lib().lt_last_error()
