"""GPU (-m gpu): lt_unproject_masked_bwd (csrc/unproject_bwd.hip) -- the MASKED forms of the tap / bounding-box kernel K0, of the per-view gradient kernels K1
(unproj_dx_kernel<T, 4 | 8>, the passes and groups forms for more than 8 views) and of both confidence finalizers, in front of the unchanged gather K2 --
through the entry itself.  What a mask means is stated by tests/unproject_bwd_masked_ref.py (the unmasked reference on every sample's valid views alone,
zeros for the masked ones), itself pinned to fp64 autograd by tests/test_unproject_bwd_masked_ref_cpu.py.

grad_feats and grad_conf are NaN before every call and must be finite after it: every pixel of every map is written, the masked views' included, and those
must be exactly zero.  Every case asserts from masked_bwd_plan() that it enters the K1 form and the finalizer its id names.

Gates: bit for bit on the lattice (sum / max / conf, every K1 form); for NV <= 8 bit for bit the unmasked entry run per sample on the compacted valid views,
all five aggregations, realistic geometry (the masked and the compacted run take the same K1 instantiation); one softmax case across the 4-view form within
eight fp32 yardsticks; NV > 8 softmax / conf_norm at 1e-4 max|ref| against fp64; an all-ones mask gives lt_unproject_bwd's bits in every form; the chunked
batch equals the whole batch; two runs are equal; NaN in a masked view changes nothing; the refusals; the autograd wrapper."""
import pytest
import torch

import lt_hip as H
import test_gpu_unproject_bwd_kernels as K
import unproject_bwd_masked_ref as M
import unproject_bwd_ref as R
from gpu_util import check, record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


@pytest.fixture(autouse=True)
def _gather_path(monkeypatch):
    monkeypatch.delenv("LT_UNPROJ_BWD_ATOMICS", raising=False)


def _dev(case, dtype):
    return (case.hm.to(DEV).to(dtype), case.P.to(DEV), case.cv.to(DEV), case.conf.to(DEV), case.G.to(DEV))


def _masked(dev, mask, agg, ws_samples=None, expect=0, null_mask=False):
    """lt_unproject_masked_bwd itself: device tensors in the public layouts in, (grad_feats (B,NV,C,h,w), grad_conf or None) out, both NaN before the call,
    finite after it and exactly +0.0 in the masked views.  ws_samples: a workspace of exactly that many samples' shares (None: the whole batch's)."""
    hm, P, cv, conf, G = dev
    Bn, NV, C, h, w = hm.shape
    feats = hm.permute(0, 1, 3, 4, 2).contiguous()
    g = G.permute(0, 2, 3, 4, 1).float().contiguous()
    v0, v1, v2 = cv.shape[1:4]
    gf = torch.full((Bn, NV, h, w, C), NAN, dtype=torch.float32, device=DEV)
    is_conf = agg.startswith("conf")
    gc = torch.full((Bn, NV, C), NAN, dtype=torch.float32, device=DEV) if is_conf else None
    lib = H.lib()
    nws = max(lib.lt_unproject_bwd_workspace(1, NV, min(C, 64), v0, v1, v2), 16) * (Bn if ws_samples is None else ws_samples)
    ws = torch.empty(max(16, nws), dtype=torch.uint8, device=DEV)
    m = mask.to(DEV).contiguous()
    assert m.dtype == torch.uint8 and tuple(m.shape) == (Bn, NV)
    rc = lib.lt_unproject_masked_bwd(H.dtype_code(hm.dtype), feats.data_ptr(), P.data_ptr(), cv.data_ptr(), conf.data_ptr() if is_conf else None,
                                     None if null_mask else m.data_ptr(), g.data_ptr(), gf.data_ptr(), H.ptr(gc), Bn, NV, C, h, w, v0, v1, v2, H.AGG[agg],
                                     ws.data_ptr(), nws, H.cur_stream())
    if expect != 0:
        assert rc == expect, (rc, lib.lt_last_error())
        return None, None
    H.check(rc, "lt_unproject_masked_bwd")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(gf).all()), "%s: a pixel of grad_feats was not written, or is not finite" % agg
    assert gc is None or bool(torch.isfinite(gc).all()), "%s: grad_conf was not written, or is not finite" % agg
    off = (m == 0)
    z = gf[off]
    assert bool((z == 0).all()) and not bool(torch.signbit(z).any()), "%s: a masked view's grad_feats is not +0.0 everywhere" % agg
    if gc is not None:
        assert bool((gc[off] == 0).all()) and not bool(torch.signbit(gc[off]).any()), "%s: a masked view's grad_conf is not +0.0" % agg
    return gf.permute(0, 1, 4, 2, 3).cpu(), (None if gc is None else gc.cpu())


def _twice(dev, mask, agg, name, ws_samples=None):
    gf, gc = _masked(dev, mask, agg, ws_samples)
    gf2, gc2 = _masked(dev, mask, agg, ws_samples)
    assert torch.equal(gf, gf2), "%s: d/d features differ between two runs" % name
    assert gc is None or torch.equal(gc, gc2), "%s: d/d confidences differ between two runs" % name
    return gf, gc


def _plan(dev, agg, ws_samples=None, **expect):
    hm = dev[0]
    B, NV, C, h, w = hm.shape
    plan = M.masked_bwd_plan(hm.dtype, B, NV, C, h, w, tuple(dev[2].shape[1:4]), agg, ws_samples=ws_samples)
    R.plan_is(plan, **dict(expect, k1=M._k1(NV, agg), finalizer=None if not agg.startswith("conf") else ("many" if NV > 8 else "small"), masked=True))
    assert expect.get("k1", plan["k1"]) == plan["k1"]
    return plan


def _compacted(dev, mask, agg):
    """lt_unproject_bwd per sample on the sample's valid views alone, scattered back; zeros for the masked views."""
    hm, P, cv, conf, G = dev
    B, NV, C, h, w = hm.shape
    gf = torch.zeros(B, NV, C, h, w, dtype=torch.float32)
    gc = torch.zeros(B, NV, C, dtype=torch.float32) if agg.startswith("conf") else None
    for b in range(B):
        idx = M.valid_views(mask, b)
        f, c = K._entry((hm[b:b + 1, idx].contiguous(), P[b:b + 1, idx].contiguous(), cv[b:b + 1], conf[b:b + 1, idx].contiguous(), G[b:b + 1]), agg)
        gf[b, idx] = f[0]
        if gc is not None:
            gc[b, idx] = c[0]
    return gf, gc


def _same(name, got, want, failed):
    K._equal("masked/" + name, got, want, failed)


# ---- the lattice: bit for bit ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sorted(M.EXACT))
def test_masked_backward_bit_exact_on_the_lattice(cid):
    """sum / max / conf against the fp64 reference of the valid views cast to fp32, torch.equal, twice.  NV 2, 4: unproj_dx_kernel<T, 4>; 7, 8: <T, 8>; 9, 17,
    32: the passes (max) and groups (sum, conf) forms and the many-view finalizer; fp32 and bf16 maps; 33 x 17 and 16 x 16 maps; whole and ragged brick grids.
    Row 0 of every mask is fully valid, row 1 has one view masked (view 0 for even NV: max and the passes start at a later view), row 2 a single valid view
    (the last: beyond 8 views whole groups have none).  *_nan: NaN in the masked views' maps, matrices and confidences -- the same bits, all finite."""
    spec, case = M.EXACT[cid], M.make(M.EXACT, cid)
    mask = spec["mask"]
    dev = _dev(case, spec["dtype"])
    N = case.vs[0] * case.vs[1] * case.vs[2]
    failed = []
    for agg in spec["aggs"]:
        plan = _plan(dev, agg, **spec["plan"])
        want_f, want_c = M.lattice_reference(cid, case, mask, agg, R.conf_terms(plan, N))          # asserts the exactness condition
        gf, gc = _twice(dev, mask, agg, "%s/%s" % (cid, agg))
        _same("%s/%s: d/d features" % (cid, agg), gf, want_f, failed)
        if want_c is not None:
            _same("%s/%s: d/d confidences" % (cid, agg), gc, want_c, failed)
        if spec["nan"]:          # unchanged: the clean case's reference is this case's reference on the valid views
            clean_f, clean_c = M.lattice_reference(cid[:-4], M.make(M.EXACT, cid[:-4]), mask, agg, R.conf_terms(plan, N))
            assert torch.equal(want_f, clean_f) and (want_c is None or torch.equal(want_c, clean_c))
    assert not failed, "%d mismatching comparisons:\n%s" % (len(failed), "\n".join(failed))


def test_chunked_batch_equals_the_whole_batch():
    """B = 3 with three different mask rows and a workspace of one sample's share: three chunks, the mask pointer advancing with them; the whole-batch call's bits."""
    spec, case = M.EXACT[M.CHUNKS], M.make(M.EXACT, M.CHUNKS)
    dev = _dev(case, spec["dtype"])
    for agg in M.AGGS:
        R.plan_is(_plan(dev, agg), chunk=3, nchunks=1)
        R.plan_is(_plan(dev, agg, ws_samples=1), chunk=1, nchunks=3)
        whole = _masked(dev, spec["mask"], agg)
        part = _masked(dev, spec["mask"], agg, ws_samples=1)
        assert torch.equal(part[0], whole[0]) and (whole[1] is None or torch.equal(part[1], whole[1])), agg


# ---- realistic geometry ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sorted(M.REAL_SMALL))
def test_up_to_8_views_bit_identical_to_the_compacted_unmasked_run(cid):
    """All five aggregations, fp32 and bf16 maps: on its valid views lt_unproject_masked_bwd gives lt_unproject_bwd's bits for the sample's compacted valid
    views (the same K1 instantiation: the masks keep the valid count on NV's side of 4), and zeros on the masked ones; two runs are equal."""
    NV, C, mask = M.REAL_SMALL[cid]
    c = R.realistic_case(NV, C)
    failed = []
    for ty, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        dev = _dev(c, dtype)
        for agg in M.AGGS:
            _plan(dev, agg, path="gather", CW=C // 4)
            for b in range(2):
                n = len(M.valid_views(mask, b))
                R.plan_is(R.bwd_plan(dtype, 1, n, C, c.h, c.w, c.vs, agg), k1=M._k1(NV, agg))          # the compacted run's K1 form is the masked run's
            gf, gc = _twice(dev, mask, agg, "%s/%s/%s" % (cid, ty, agg))
            want_f, want_c = _compacted(dev, mask, agg)
            _same("%s/%s/%s: d/d features vs compacted" % (cid, ty, agg), gf, want_f, failed)
            if want_c is not None:
                _same("%s/%s/%s: d/d confidences vs compacted" % (cid, ty, agg), gc, want_c, failed)
    assert not failed, "%d mismatching comparisons:\n%s" % (len(failed), "\n".join(failed))


def test_softmax_across_the_4_view_form_within_eight_fp32_yardsticks():
    """NV = 5 with three valid views: the masked run takes unproj_dx_kernel<T, 8>, the compacted run of three views <T, 4>.  The two instantiations state the
    same arithmetic, but nothing holds the compiler to the same expf / division sequence in both, so this one case is not gated bit for bit: it takes the
    suite's softmax gate on lattice inputs, |got - ref| <= 8 yardsticks x magnitude per element, the yardstick being the fp32 statement's own distance from
    fp64 (test_gpu_unproject_bwd_kernels._gate_magnitude), against the fp64 reference of the valid views."""
    spec, case, mask = M.CROSS, M.CROSS["make"](), M.CROSS["mask"]
    for ty, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        dev = _dev(case, dtype)
        _plan(dev, "softmax", **spec["plan"])
        for b in range(2):
            R.plan_is(R.bwd_plan(dtype, 1, 3, 8, case.h, case.w, case.vs, "softmax"), k1="mv4")
        ref_f, _, mag, _ = M.masked_ref_backward(case.hm, case.P, case.cv, case.G, "softmax", mask)
        f32, _, _, _ = M.masked_ref_backward(case.hm, case.P, case.cv, case.G, "softmax", mask, dtype=torch.float32)
        gf, _ = _twice(dev, mask, "softmax", "cross/" + ty)
        K._gate_magnitude("masked/cross_NV5_%s/softmax: d/d features" % ty, gf, ref_f, mag.feats, K._yard(f32, ref_f, mag.feats))


@pytest.mark.parametrize("cid", sorted(M.REAL_MANY))
def test_more_than_8_views_softmax_and_conf_norm_against_fp64(cid):
    """NV = 9, 17, 32, fp32 and bf16 maps (the reference on the bf16-rounded maps): max|d| <= 1e-4 max|ref| against the fp64 reference of the valid views (the
    suite's gate for this kernel).  Sample 0 lacks view 0 and a middle view, sample 1 the whole first group of 8 views."""
    NV, C, mask = M.REAL_MANY[cid]
    c = R.realistic_case(NV, C)
    for ty, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        hm = c.hm if ty == "fp32" else c.hm.bfloat16().float()
        dev = _dev(c._replace(hm=hm), dtype)
        for agg in ("softmax", "conf_norm"):
            _plan(dev, agg, path="gather", CW=C // 4, many=True)
            ref_f, ref_c, _, _ = M.masked_ref_backward(hm, c.P, c.cv, c.G, agg, mask, c.conf)
            name = "unproject_masked_bwd_kernels/many/%s_%s/%s" % (cid, ty, agg)
            gf, gc = _twice(dev, mask, agg, name)
            e = check(name + ": d/d features", gf, ref_f, 1e-4)
            print("%s: d/d features max|d|/max|ref| = %.3e" % (name, e))
            if ref_c is not None:
                e = check(name + ": d/d confidences", gc, ref_c, 1e-4)
                print("%s: d/d confidences max|d|/max|ref| = %.3e" % (name, e))


@pytest.mark.parametrize("NV,C", M.ALL_ONES)
def test_all_ones_mask_gives_the_unmasked_entrys_bits(NV, C):
    """Every K1 form (<T, 4>, <T, 8>, passes, groups) and both finalizers, all five aggregations, fp32 and bf16 maps."""
    c = R.realistic_case(NV, C)
    mask = torch.ones(2, NV, dtype=torch.uint8)
    failed = []
    for ty, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        dev = _dev(c, dtype)
        for agg in M.AGGS:
            _plan(dev, agg)
            gf, gc = _masked(dev, mask, agg)
            want_f, want_c = K._entry(dev, agg)
            _same("ones_NV%d_C%d_%s/%s: d/d features" % (NV, C, ty, agg), gf, want_f, failed)
            if want_c is not None:
                _same("ones_NV%d_C%d_%s/%s: d/d confidences" % (NV, C, ty, agg), gc, want_c, failed)
    assert not failed, "%d mismatching comparisons:\n%s" % (len(failed), "\n".join(failed))


# ---- refusals and the wrapper ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    """A null mask (LT_ERR_INVALID); C = 96 and LT_UNPROJ_BWD_ATOMICS=1 (LT_ERR_UNSUPPORTED, with a message that says why: there is no masked scatter)."""
    c = R.realistic_case(4, 32)
    dev = _dev(c, torch.float32)
    mask = M.REAL_SMALL["NV4_C32"][2]
    lib = H.lib()
    _masked(dev, mask, "sum", expect=-1, null_mask=True)
    assert b"lt_unproject_masked_bwd: null view_mask" in lib.lt_last_error()
    g = torch.Generator().manual_seed(5)
    wide = (torch.randn(2, 4, 96, c.h, c.w, generator=g).to(DEV), dev[1], dev[2], torch.rand(2, 4, 96, generator=g).to(DEV), torch.randn(2, 96, *c.vs, generator=g).to(DEV))
    assert M.masked_bwd_plan(torch.float32, 2, 4, 96, c.h, c.w, c.vs, "sum")["refused"][0] == -2
    _masked(wide, mask, "sum", expect=-2)
    assert b"only the gather path takes a view mask" in lib.lt_last_error()
    monkeypatch.setenv("LT_UNPROJ_BWD_ATOMICS", "1")
    assert M.masked_bwd_plan(torch.float32, 2, 4, 32, c.h, c.w, c.vs, "sum")["refused"] == (-2, "LT_UNPROJ_BWD_ATOMICS")
    _masked(dev, mask, "sum", expect=-2)
    assert b"LT_UNPROJ_BWD_ATOMICS" in lib.lt_last_error() and b"no masked form" in lib.lt_last_error()
    monkeypatch.delenv("LT_UNPROJ_BWD_ATOMICS")
    _masked(dev, mask, "sum")          # and the same call goes through without it


def test_autograd_wrapper_equals_the_entry_point():
    """mvn.utils.op.unproject_heatmaps(..., view_mask=, masked_backward=True).backward(): the wrapper's layouts, mask conversion and workspace handling -- the
    entry point's bits, for a bool host mask and a uint8 device mask; its forward is the masked forward; without the flag it refuses as it always did."""
    from mvn.utils import op
    NV, C, mask = M.REAL_SMALL["NV4_C32"]
    c = R.realistic_case(NV, C)
    dev = _dev(c, torch.float32)
    hm, P, cv, conf, G = dev
    for agg in M.AGGS:
        # (the functional op takes NORMALISED confidences for 'conf_norm', as the reference's does: both conf methods are the kernel's 'conf')
        want_f, want_c = _masked(dev, mask, "conf" if agg.startswith("conf") else agg)
        for vm in (mask.bool(), mask.to(DEV)):
            f = hm.clone().requires_grad_(True)
            cf = conf.clone().requires_grad_(True) if agg.startswith("conf") else None
            out = op.unproject_heatmaps(f, P, cv, agg, cf, view_mask=vm, masked_backward=True)
            with torch.no_grad():
                assert torch.equal(out, op.unproject_heatmaps(hm, P, cv, agg, cf, view_mask=vm))
            (out * G).sum().backward()
            assert torch.equal(f.grad.cpu(), want_f), agg
            assert cf is None or torch.equal(cf.grad.cpu(), want_c), agg
    f = hm.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="inference only"):
        op.unproject_heatmaps(f, P, cv, "sum", view_mask=mask)
