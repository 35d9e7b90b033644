"""GPU (-m gpu): every branch of the unprojection backward (csrc/unproject_bwd.hip) -- the tap / bounding-box kernel K0, the per-view gradient kernels K1
(unproj_dx_kernel<T, 4 | 8>, the passes and groups forms for more than 8 views), both confidence finalizers, the LDS gather K2
(unproj_gather_kernel<CW>, CW = 1, 2, 4, 8, 16) and both atomic scatter kernels -- through lt_unproject_bwd itself, against the backward written out in
fp64 (tests/unproject_bwd_ref.py, itself pinned to fp64 autograd by tests/test_unproject_bwd_ref_cpu.py).

Every case ASSERTS from bwd_plan() that it enters the branch its id names, before it compares numbers.  grad_feats and grad_conf are NaN before every call and
must be finite after it: every pixel of every map is written.  B = 2 with different points per sample unless the case says otherwise.

EXACT layer: inputs on a dyadic lattice (unproject_bwd_ref.lattice_case), where every weight, sample, dx and partial sum is exact in fp32 in any order.  The
gate is torch.equal with the fp64 reference cast to fp32 -- no tolerance anywhere -- for sum, max, conf, and conf_norm where the confidences make it exact;
every run is done twice and the two results must be torch.equal as well.  The exactness condition (exact.assert_exact) is asserted for every case before
anything is launched.

TOLERANCED layer: what cannot be exact.  softmax, and conf_norm with confidences in eighths, on lattice inputs: weights and taps are exact there, only expf and
the divisions round; per element |got - ref| <= tol * magnitude (exactly 0 where the magnitude is 0), tol = 8 x the largest |ref32 - ref64| / magnitude of the
case, ref32 being the same statement in fp32 on the CPU -- 8 for expf / __fdiv_rn against torch's exp and division and for another order of up to about 16
additions per pixel.  Realistic geometry (ring cameras, camera 0 inside a rotated cuboid, randn maps), all five aggregations, fp32 and bf16 maps: the project's
gate for this kernel, max|d| <= 1e-4 max|ref| against fp64.  The yardstick, tol and the achieved fraction of every gate go to the parity report."""
import pytest
import torch

import lt_hip as H
import unproject_bwd_ref as R
from gpu_util import check, record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
_DEVT = {}


def _dev(table, cid, dtype):
    """The case's tensors on the device (maps in the kernel's type), made once per case."""
    key = (id(table), cid, dtype)
    if key not in _DEVT:
        c = R.make(table, cid)
        _DEVT[key] = (c.hm.to(DEV).to(dtype), c.P.to(DEV), c.cv.to(DEV), c.conf.to(DEV), c.G.to(DEV))
    return _DEVT[key]


def _entry(dev, agg, ws_samples=None, expect=0):
    """lt_unproject_bwd itself: device tensors in the public layouts in, (grad_feats (B,NV,C,h,w), grad_conf or None) out, both NaN before the call and finite
    after it.  ws_samples: a workspace of exactly that many samples' shares (None: the whole batch's)."""
    hm, P, cv, conf, G = dev
    Bn, NV, C, h, w = hm.shape
    feats = hm.permute(0, 1, 3, 4, 2).contiguous()
    g = G.permute(0, 2, 3, 4, 1).float().contiguous()
    v0, v1, v2 = cv.shape[1:4]
    gf = torch.full((Bn, NV, h, w, C), NAN, dtype=torch.float32, device=DEV)
    is_conf = agg.startswith("conf")
    gc = torch.full((Bn, NV, C), NAN, dtype=torch.float32, device=DEV) if is_conf else None
    lib = H.lib()
    nws = lib.lt_unproject_bwd_workspace(1, NV, C, v0, v1, v2) * (Bn if ws_samples is None else ws_samples)
    ws = torch.empty(max(16, nws), dtype=torch.uint8, device=DEV)
    rc = lib.lt_unproject_bwd(H.dtype_code(hm.dtype), feats.data_ptr(), P.data_ptr(), cv.data_ptr(), conf.data_ptr() if is_conf else None, g.data_ptr(),
                              gf.data_ptr(), H.ptr(gc), Bn, NV, C, h, w, v0, v1, v2, H.AGG[agg], ws.data_ptr(), nws, H.cur_stream())
    if expect != 0:
        assert rc == expect, (rc, lib.lt_last_error())
        return None, None
    H.check(rc, "lt_unproject_bwd")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(gf).all()), "%s: a pixel of grad_feats was not written, or is not finite" % agg
    assert gc is None or bool(torch.isfinite(gc).all()), "%s: grad_conf was not written, or is not finite" % agg
    return gf.permute(0, 1, 4, 2, 3).cpu(), (None if gc is None else gc.cpu())


def _twice(dev, agg, name, ws_samples=None):
    gf, gc = _entry(dev, agg, ws_samples)
    gf2, gc2 = _entry(dev, agg, ws_samples)
    assert torch.equal(gf, gf2), "%s: d/d features differ between two runs" % name
    assert gc is None or torch.equal(gc, gc2), "%s: d/d confidences differ between two runs" % name
    return gf, gc


def _equal(name, got, want, failed):
    """The slack-free gate: torch.equal; the mismatch count goes to the parity report, and every comparison of a case runs before the case fails."""
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, (name, got.shape, want.shape)
    ok = torch.equal(got, want)
    bad = got != want
    n = int(bad.sum())
    record("unproject_bwd_kernels/exact/" + name, {"mismatching_words": n, "words": got.numel()})
    if not ok:
        i = tuple(int(t) for t in bad.nonzero()[0]) if n else ()
        failed.append("%s: %d of %d words differ, first at %s: got %r want %r, largest |d| %.3e" %
                      (name, n, got.numel(), i, float(got[i]) if n else None, float(want[i]) if n else None, float((got - want).abs().max())))


def _setenv(monkeypatch, env):
    monkeypatch.delenv("LT_UNPROJ_BWD_ATOMICS", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _plan(spec, dev, agg, ws_samples=None):
    """bwd_plan of the call as it is made (the environment as it is now), held to the branch the id names."""
    hm = dev[0]
    B, NV, C, h, w = hm.shape
    plan = R.bwd_plan(hm.dtype, B, NV, C, h, w, tuple(dev[2].shape[1:4]), agg, ws_samples=ws_samples)
    R.plan_is(plan, **spec["plan"])
    return plan


def _exact_case(cid, monkeypatch, run=None, ws_samples=None):
    spec, case = R.EXACT[cid], R.make(R.EXACT, cid)
    _setenv(monkeypatch, spec["env"])
    R.check_structure(cid, case)
    dev = _dev(R.EXACT, cid, spec["dtype"])
    N = case.vs[0] * case.vs[1] * case.vs[2]
    failed, out = [], {}
    for agg in spec["aggs"]:
        plan = _plan(spec, dev, agg, ws_samples)
        want_f, want_c, _ = R.lattice_reference(cid, case, agg, R.conf_terms(plan, N), key=cid)          # asserts the exactness condition
        gf, gc = run(dev, agg) if run is not None else _twice(dev, agg, "%s/%s" % (cid, agg), ws_samples)
        _equal("%s/%s: d/d features" % (cid, agg), gf, want_f, failed)
        if want_c is not None:
            _equal("%s/%s: d/d confidences" % (cid, agg), gc, want_c, failed)
        else:
            assert gc is None
        out[agg] = (gf, gc, plan)
    assert not failed, "%d mismatching comparisons:\n%s" % (len(failed), "\n".join(failed))
    return out


# ---- exact layer ---------------------------------------------------------------------------------------------------------------------------------------------
GATHER_IDS = [c for c in sorted(R.EXACT) if not c.startswith(("scatter", "chunks", "op_"))]


@pytest.mark.parametrize("cid", GATHER_IDS)
def test_gather_path_bit_exact_on_the_lattice(cid, monkeypatch):
    """cw*: every instantiation of the gather at NV = 3 (conf_norm at NV = 4), maps 20 x 37 (ragged tiles), grid 5 x 6 x 7 (ragged bricks), HALVES 2 and 1.
    classes: all 12 padding / depth classes in every view, ix == -1, ix == w - 1 and z == 0 among them.  tiny: 2 x 2 maps, one voxel and one brick.  seams:
    patches across the half-wave split, across tile edges and in one-pixel last tiles.  pile / alternate: 4, 3, 2 hits of a round in one cell and
    off[2] == off[0] != off[1].  refill: a second fill of the candidate list, empty bounding boxes in the walk.  empty_view: a map that is all zeros and
    still written.  k1_stride: K1's grid-stride loop past 2048 workgroups and the confidence partials of it.  bf16_*: ld4<bf16_t> in both register forms.
    views_*: MV = 4, MV = 8, passes, groups, both finalizers, the tie rule of max across view 8."""
    out = _exact_case(cid, monkeypatch)
    if cid == "empty_view":
        for agg, (gf, gc, _) in out.items():
            assert float(gf[:, 1].abs().max()) == 0 and float(gf[:, 0].abs().max()) > 0, agg
    if cid.startswith("views_"):
        NV = int(cid.split("NV")[1])
        for agg, (_, _, plan) in out.items():
            R.plan_is(plan, k1=R.VIEWS_K1[NV][0 if agg == "max" else 1], finalizer=None if not agg.startswith("conf") else ("many" if NV > 8 else "small"))


def test_chunked_batch_bit_exact_and_equal_to_the_whole_batch(monkeypatch):
    """B = 3 with a workspace of one and of two samples' shares (the second chunk of the latter holds one sample): the reference's bits, i.e. the whole-batch call's."""
    whole = _exact_case("chunks", monkeypatch)
    for n, chunks in ((1, 3), (2, 2)):
        part = _exact_case("chunks", monkeypatch, ws_samples=n)
        for agg in whole:
            R.plan_is(part[agg][2], chunk=n, nchunks=chunks)
            R.plan_is(whole[agg][2], chunk=3, nchunks=1)
            assert torch.equal(part[agg][0], whole[agg][0]) and (whole[agg][1] is None or torch.equal(part[agg][1], whole[agg][1])), (agg, n)


@pytest.mark.parametrize("cid", [c for c in sorted(R.EXACT) if c.startswith("scatter")])
def test_scatter_path_bit_exact_on_the_lattice(cid, monkeypatch):
    """Both atomic scatter kernels: C = 12 and C = 128 go there by themselves, C = 32 under LT_UNPROJ_BWD_ATOMICS=1.  On lattice inputs float atomics are exact in
    any order: scatter == reference == gather bit for bit.  conf_norm is refused with its message."""
    out = _exact_case(cid, monkeypatch)
    spec = R.EXACT[cid]
    dev = _dev(R.EXACT, cid, spec["dtype"])
    _entry(dev, "conf_norm", expect=-2)          # LT_ERR_UNSUPPORTED
    assert b"conf_norm needs the gather path" in H.lib().lt_last_error()
    if spec["env"]:
        monkeypatch.delenv("LT_UNPROJ_BWD_ATOMICS")
        for agg in spec["aggs"]:
            R.plan_is(_plan(dict(plan={}), dev, agg), path="gather", CW=8)
            gf, gc = _entry(dev, agg)
            assert torch.equal(gf, out[agg][0]) and (gc is None or torch.equal(gc, out[agg][1])), "%s: gather and scatter differ" % agg


def test_autograd_wrapper_bit_exact_on_the_lattice(monkeypatch):
    """mvn.utils.op.unproject_heatmaps(...).backward(): the wrapper's layouts and workspace handling."""
    from mvn.utils import op

    def run(dev, agg):
        hm, P, cv, conf, G = dev
        res = []
        for _ in range(2):
            f = hm.clone().requires_grad_(True)
            c = conf.clone().requires_grad_(True) if agg == "conf" else None
            (op.unproject_heatmaps(f, P, cv, agg, c) * G).sum().backward()
            res.append((f.grad.cpu(), None if c is None else c.grad.cpu()))
        assert torch.equal(res[0][0], res[1][0]) and (res[0][1] is None or torch.equal(res[0][1], res[1][1])), agg
        return res[0]
    _exact_case("op_cw8", monkeypatch, run=run)


# ---- toleranced layer ----------------------------------------------------------------------------------------------------------------------------------------
_TREF = {}


def _yard(r32, r64, mag):
    nz = mag > 0
    return float(((r32.double() - r64).abs()[nz] / mag[nz]).max())


def _toleranced_reference(cid, agg):
    """(ref64 features, ref64 confidences, Mag, yardstick of the features, of the confidences); fp32 and bf16 share it: the maps are integers."""
    key = (cid.rsplit("_", 1)[0], agg)
    if key not in _TREF:
        c = R.make(R.TOLERANCED, cid)
        gf, gc, mag, _ = R.ref_backward(c.hm, c.P, c.cv, c.G, agg, c.conf)
        f32, c32, _, _ = R.ref_backward(c.hm, c.P, c.cv, c.G, agg, c.conf, dtype=torch.float32)
        yf = _yard(f32, gf, mag.feats)
        yc = None if gc is None else _yard(c32, gc, mag.conf)
        _TREF[key] = (gf, gc, mag, yf, yc)
    return _TREF[key]


def _gate_magnitude(name, got, ref, mag, yard):
    tol = 8 * yard
    got = got.double()
    nz = mag > 0
    assert bool((got[~nz] == 0).all()), "%s: non-zero where nothing contributes" % name
    d = (got - ref).abs()
    rel = float((d[nz] / mag[nz]).max())
    frac = rel / tol if tol > 0 else (0.0 if rel == 0 else float("inf"))
    record("unproject_bwd_kernels/toleranced/" + name, {"yardstick": yard, "tol": tol, "err": rel, "fraction_of_tol": frac})
    print("%s: yardstick %.3e, tol %.3e, achieved %.3e = %.3f of tol" % (name, yard, tol, rel, frac))
    assert bool((d <= tol * mag).all()), "%s: |got - ref| reaches %.3e of the magnitude, tol %.3e (8 x the fp32 reference's %.3e)" % (name, rel, tol, yard)


@pytest.mark.parametrize("cid", sorted(R.TOLERANCED))
def test_softmax_and_conf_norm_on_the_lattice_within_eight_fp32_yardsticks(cid, monkeypatch):
    spec = R.TOLERANCED[cid]
    _setenv(monkeypatch, spec["env"])
    dev = _dev(R.TOLERANCED, cid, spec["dtype"])
    for agg in spec["aggs"]:
        _plan(spec, dev, agg)
        ref_f, ref_c, mag, yf, yc = _toleranced_reference(cid, agg)
        gf, gc = _twice(dev, agg, "%s/%s" % (cid, agg))
        _gate_magnitude("%s/%s: d/d features" % (cid, agg), gf, ref_f, mag.feats, yf)
        if ref_c is not None:
            _gate_magnitude("%s/%s: d/d confidences" % (cid, agg), gc, ref_c, mag.conf, yc)


@pytest.mark.parametrize("C", R.REAL_C)
@pytest.mark.parametrize("NV", R.REAL_NV)
def test_realistic_geometry_against_fp64(NV, C, monkeypatch):
    """Ring cameras with camera 0 inside a rotated cuboid grid, randn maps; fp32 maps, and bf16 maps against the reference on the bf16-rounded maps; all five
    aggregations; max|d| <= 1e-4 max|ref| (the gate of tests/test_gpu_backward.py).  tests/test_unproject_bwd_ref_cpu.py holds every case to: no 'max'
    winner and no depth sign differs between fp32 and fp64, every view receives a gradient."""
    _setenv(monkeypatch, {})
    c = R.realistic_case(NV, C)
    for ty, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        hm = c.hm if ty == "fp32" else c.hm.bfloat16().float()
        dev = (hm.to(DEV).to(dtype), c.P.to(DEV), c.cv.to(DEV), c.conf.to(DEV), c.G.to(DEV))
        for agg in R.AGGS:
            R.plan_is(R.bwd_plan(dtype, 2, NV, C, c.h, c.w, c.vs, agg), path="gather", CW=C // 4, k1="mv4" if NV <= 4 else "mv8")
            ref_f, ref_c, mag, _ = R.ref_backward(hm, c.P, c.cv, c.G, agg, c.conf)
            name = "unproject_bwd_kernels/realistic/NV%d_C%d_%s/%s" % (NV, C, ty, agg)
            gf, gc = _twice(dev, agg, name)
            e = check(name + ": d/d features", gf, ref_f, 1e-4)
            print("%s: d/d features max|d|/max|ref| = %.3e" % (name, e))
            if NV == 1 and agg == "conf_norm":
                # one view: n = c / c = 1 whatever c is, so d/dc = (s - s c / S) / S vanishes identically and the reference's own value is the rounding noise
                # of fp64 -- nothing to take 1e-4 of.  The finalizer works in fp64: s c / S is two roundings, s (1 + 2 eps) at worst with eps = 2^-53, so
                # what is left of s - s c / S is at most 2^-52 |s|, i.e. 2^-53 of the magnitude (>= 2 |s| / S); 2^-50 leaves room for another order of
                # the same three operations and for the rounding of the result to fp32
                e = float((gc.double().abs() / mag.conf).max())
                record(name + ": d/d confidences (identically zero)", {"err": e, "tol": 2.0 ** -50})
                assert e <= 2.0 ** -50, "%s: d/d confidences of a single view must vanish, got %.3e of the magnitude" % (name, e)
            elif ref_c is not None:
                e = check(name + ": d/d confidences", gc, ref_c, 1e-4)
                print("%s: d/d confidences max|d|/max|ref| = %.3e" % (name, e))
