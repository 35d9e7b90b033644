"""GPU (-m gpu): lt_unproject_desc_fwd / lt_unproject_desc_bwd against the shorthand entry of the same variant on the same inputs, bit for bit.

Both kernel paths that run here are deterministic (the forward, and the gather backward) and both calls go through one host body, so torch.equal is the
gate: what it proves is the mapping from the pointers that are set to the variant, and the struct's layout as ctypes fills it -- not numerics, which the
kernels' own suites hold (test_gpu_unproject_kernels.py and its kin, through the shorthands).  Every output is NaN before a call and finite after it.

Shapes: the smallest that reach each instantiation.  "bf16": B = 2, NV = 4, C = 32, maps 12 x 16, V = 16 -- the fused quad kernel.  "fp32": B = 2, NV = 3,
C = 4, volume (5, 6, 7) -- the generic kernel, odd sizes, more than one workgroup; the grid form needs a cube and takes V = 5 there.  Masks: rows 1011 / 0110
(their first three columns at NV = 3).  Indexed: F = 2 frames, P = 3 cuboids, frame_of = [1, 0, 1].  Ragged: B = 2 samples of (2, 4) views, T = 6,
NVcap = 4.  Every case asserts from the host-dispatch models (unproject_ref.unproject_plan, unproject_bwd_ref.bwd_plan) that it enters the branch its id
names before it compares.  Every pointer handed to a call is a live allocation of the size the call states."""
import ctypes as C

import numpy as np
import pytest
import torch

import lt_hip as H
import unproject_bwd_ref as R
import unproject_ref as U
from oracle import synth
from oracle import vol_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
F, P, FRAME_OF = 2, 3, (1, 0, 1)
COUNTS, T, NVCAP = (2, 4), 6, 4
HW = (12, 16)
SHAPES = {"bf16": dict(dt=torch.bfloat16, NV=4, C=32, vs=(16, 16, 16), V=16, kernel="quad"),
          "fp32": dict(dt=torch.float32, NV=3, C=4, vs=(5, 6, 7), V=5, kernel="generic")}
VARIANTS = ("plain", "masked", "indexed", "indexed+mask", "ragged")
_MADE = {}


def _inputs(ty):
    """Everything a case of shape ``ty`` reads, made once and left unchanged: by frame (F = B = 2), by cuboid (P = 3; the unindexed variants take the first
    two) and by view of the ragged batch (T = 6)."""
    if ty not in _MADE:
        s = SHAPES[ty]
        NV, Cc, vs, V, dt = s["NV"], s["C"], s["vs"], s["V"], s["dt"]
        h, w = HW
        g = torch.Generator().manual_seed(4100 + Cc)

        def cameras(n):
            K, Rm, t = synth.ring_cameras(n, 96, inside=True)
            return torch.from_numpy(O.resized_projection(K, Rm, t, (96, 96), (h, w))).float()
        base = torch.randn(P, 3, generator=g).numpy().astype(np.float64) * 100
        side = 2500.0
        rot = np.stack([O.rotation_matrix((0, 0, 1), 0.3 * p + 0.1) for p in range(P)]).astype(np.float32)
        d = dict(s, h=h, w=w,
                 feats=torch.randn(F, NV, h, w, Cc, generator=g).to(DEV, dt), proj=cameras(NV)[None].repeat(F, 1, 1, 1).contiguous().to(DEV),
                 conf=(torch.rand(F, NV, Cc, generator=g) + 0.1).to(DEV),
                 coords=torch.stack([U.box_coords(base[p], side, vs, 0.3 * p + 0.1) for p in range(P)]).to(DEV),
                 pos=torch.from_numpy((base - side / 2).astype(np.float32)).to(DEV), center=torch.from_numpy(base.astype(np.float32)).to(DEV),
                 rot=torch.from_numpy(rot).reshape(P, 9).contiguous().to(DEV), step=float(np.float32(side / (V - 1))),
                 mask=torch.tensor([[1, 0, 1, 1][:NV], [0, 1, 1, 0][:NV]], dtype=torch.uint8).to(DEV),
                 frame_of=torch.tensor(FRAME_OF, dtype=torch.int32).to(DEV),
                 rfeats=torch.randn(T, h, w, Cc, generator=g).to(DEV, dt), rproj=torch.cat([cameras(n) for n in COUNTS]).contiguous().to(DEV),
                 rconf=(torch.rand(T, Cc, generator=g) + 0.1).to(DEV), view_base=torch.tensor([0, COUNTS[0], T], dtype=torch.int32).to(DEV),
                 gout=torch.randn(P, *vs, Cc, generator=g).to(DEV))
        assert d["proj"].shape == (F, NV, 3, 4) and d["rproj"].shape == (T, 3, 4) and d["coords"].shape == (P,) + vs + (3,)
        _MADE[ty] = d
    return _MADE[ty]


def _variant(d, variant):
    """-> (feats, proj, conf, view_mask, frame_of, view_base, items, NV) of a variant: the tensors its calls take and the samples / cuboids it walks."""
    if variant == "ragged":
        return d["rfeats"], d["rproj"], d["rconf"], None, None, d["view_base"], len(COUNTS), NVCAP
    mask = d["mask"] if "mask" in variant else None
    fof = d["frame_of"] if variant.startswith("indexed") else None
    return d["feats"], d["proj"], d["conf"], mask, fof, None, P if fof is not None else F, d["NV"]


def _desc(d, variant, grid, agg, coords_out=None):
    feats, proj, conf, mask, fof, vb, n, NV = _variant(d, variant)
    vs = (d["V"],) * 3 if grid else d["vs"]
    kw = dict(pos=d["pos"].data_ptr(), center=d["center"].data_ptr(), rot=d["rot"].data_ptr(), step=d["step"], cmu_transfer=0,
              coords_out=coords_out.data_ptr()) if grid else dict(coords=d["coords"].data_ptr())
    return H.UnprojectDesc(dtype=H.dtype_code(d["dt"]), feats=feats.data_ptr(), proj=proj.data_ptr(), conf=conf.data_ptr() if agg.startswith("conf") else None,
                           view_mask=H.ptr(mask), frame_of=H.ptr(fof), F=F, view_base=H.ptr(vb), T=T, B=n, NV=NV, C=d["C"], h=d["h"], w=d["w"],
                           v0=vs[0], v1=vs[1], v2=vs[2], agg=H.AGG[agg], **kw)


def _legacy_fwd(d, variant, grid, agg, out, coords_out):
    """The shorthand entry of the variant, called as its own signature states."""
    feats, proj, conf, mask, fof, vb, n, NV = _variant(d, variant)
    lib, dt, Cc, h, w, st = H.lib(), H.dtype_code(d["dt"]), d["C"], d["h"], d["w"], H.cur_stream()
    cp = conf.data_ptr() if agg.startswith("conf") else None
    a = H.AGG[agg]
    head = (dt, feats.data_ptr(), proj.data_ptr())
    if grid:
        head += (d["pos"].data_ptr(), d["center"].data_ptr(), d["rot"].data_ptr(), d["step"], 0, coords_out.data_ptr(), cp)
        tail, name = (Cc, h, w, d["V"], a, st), "lt_unproject_grid%s_fwd"
    else:
        head += (d["coords"].data_ptr(), cp)
        tail, name = (Cc, h, w) + d["vs"] + (a, st), "lt_unproject%s_fwd"
    if variant == "ragged":
        args, name = head + (vb.data_ptr(), out.data_ptr(), n, T, NVCAP) + tail, name % "_ragged"
    elif fof is not None:
        args, name = head + (H.ptr(mask), fof.data_ptr(), out.data_ptr(), F, n, NV) + tail, name % "_indexed"
    elif mask is not None:
        args, name = head + (mask.data_ptr(), out.data_ptr(), n, NV) + tail, name % "_masked"
    else:
        args, name = head + (out.data_ptr(), n, NV) + tail, name % ""
    H.check(getattr(lib, name)(*args), name)
    return name


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("form", ["coord", "grid"])
@pytest.mark.parametrize("ty", sorted(SHAPES))
def test_forward_descriptor_is_the_shorthand_entry_bit_for_bit(ty, form, variant):
    d, grid, agg = _inputs(ty), form == "grid", "softmax"
    n, NV = _variant(d, variant)[6:8]
    vs = (d["V"],) * 3 if grid else d["vs"]
    plan = U.unproject_plan(d["dt"], n, NV, d["C"], d["h"], d["w"], *vs, agg)
    assert plan["supported"] and plan["kernel"] == d["kernel"], "the case does not enter the kernel its shape names: %r" % (plan,)
    got, ref = [], []
    for res, call in ((ref, "legacy"), (got, "desc")):
        out = torch.full((n,) + vs + (d["C"],), NAN, dtype=d["dt"], device=DEV)
        co = torch.full((n,) + vs + (3,), NAN, dtype=torch.float32, device=DEV) if grid else None
        if call == "legacy":
            name = _legacy_fwd(d, variant, grid, agg, out, co)
        else:
            desc = _desc(d, variant, grid, agg, co)
            assert H.unproject_entry(desc) == name, "the descriptor's pointers name another entry than the shorthand it is compared with"
            H.check(H.lib().lt_unproject_desc_fwd(C.byref(desc), out.data_ptr(), H.cur_stream()), "lt_unproject_desc_fwd as " + name)
        torch.cuda.synchronize()
        res += [out] + ([co] if grid else [])
    for a, b in zip(got, ref):
        assert bool(torch.isfinite(a.float()).all()) and bool(torch.isfinite(b.float()).all()), "a voxel (or a coordinate) was not written"
        assert torch.equal(a, b)


def _legacy_bwd(d, variant, agg, gout, gfeats, gconf, ws):
    feats, proj, conf, mask, fof, _, n, NV = _variant(d, variant)
    lib, st = H.lib(), H.cur_stream()
    head = (H.dtype_code(d["dt"]), feats.data_ptr(), proj.data_ptr(), d["coords"].data_ptr(), conf.data_ptr() if agg.startswith("conf") else None)
    grads = (gout.data_ptr(), gfeats.data_ptr(), H.ptr(gconf))
    tail = (NV, d["C"], d["h"], d["w"]) + d["vs"] + (H.AGG[agg], ws.data_ptr(), ws.numel(), st)
    if fof is not None:
        args, name = head + (H.ptr(mask), fof.data_ptr()) + grads + (F, n) + tail, "lt_unproject_indexed_bwd"
    elif mask is not None:
        args, name = head + (mask.data_ptr(),) + grads + (n,) + tail, "lt_unproject_masked_bwd"
    else:
        args, name = head + grads + (n,) + tail, "lt_unproject_bwd"
    H.check(getattr(lib, name)(*args), name)
    return name


@pytest.mark.parametrize("ws_items", ["whole", "min"])
@pytest.mark.parametrize("agg", ["softmax", "conf_norm"])
@pytest.mark.parametrize("variant", VARIANTS[:4])
@pytest.mark.parametrize("ty", sorted(SHAPES))
def test_backward_descriptor_is_the_shorthand_entry_bit_for_bit(ty, variant, agg, ws_items):
    """whole: the workspace of all samples (cuboids) at once, one chunk.  min: lt_unproject_desc_bwd_workspace(desc, 1), the least the entry takes, so the
    chunk loop of the one body runs once per sample (cuboid) -- and advances what its variant advances."""
    d = _inputs(ty)
    n, NV = _variant(d, variant)[6:8]
    indexed = variant.startswith("indexed")
    lib = H.lib()
    probe = _desc(d, variant, False, agg)
    nws = lib.lt_unproject_desc_bwd_workspace(C.byref(probe), n if ws_items == "whole" else 1)
    legacy_q = lib.lt_unproject_indexed_bwd_workspace if indexed else lib.lt_unproject_bwd_workspace
    assert nws > 0 and lib.lt_unproject_desc_bwd_workspace(C.byref(probe), n) == legacy_q(n, NV, d["C"], *d["vs"])
    plan = R.bwd_plan(d["dt"], n, NV, d["C"], d["h"], d["w"], d["vs"], agg, ws_samples=None if ws_items == "whole" else 1)
    R.plan_is(plan, path="gather", k1="mv4", CW=d["C"] // 4, finalizer="small" if agg == "conf_norm" else None)
    if not indexed:          # (the indexed layout's chunking: as many cuboids' shares as fit behind the partials of all -- one, by the query above)
        R.plan_is(plan, workspace=nws, nchunks=1 if ws_items == "whole" else n)
    gout = d["gout"][:n].contiguous()
    got, ref = [], []
    for res, call in ((ref, "legacy"), (got, "desc")):
        gfeats = torch.full(tuple(d["feats"].shape), NAN, dtype=torch.float32, device=DEV)
        gconf = torch.full(tuple(d["conf"].shape), NAN, dtype=torch.float32, device=DEV) if agg == "conf_norm" else None
        ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
        if call == "legacy":
            name = _legacy_bwd(d, variant, agg, gout, gfeats, gconf, ws)
        else:
            desc = _desc(d, variant, False, agg)
            assert H.unproject_entry(desc, bwd=True) == name
            H.check(lib.lt_unproject_desc_bwd(C.byref(desc), gout.data_ptr(), gfeats.data_ptr(), H.ptr(gconf), ws.data_ptr(), ws.numel(), H.cur_stream()),
                    "lt_unproject_desc_bwd as " + name)
        torch.cuda.synchronize()
        res += [gfeats] + ([gconf] if gconf is not None else [])
    assert len(got) == (2 if agg == "conf_norm" else 1)
    for a, b in zip(got, ref):
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), "a gradient was not written"
        assert torch.equal(a, b)
    assert bool((got[0] != 0).any())
