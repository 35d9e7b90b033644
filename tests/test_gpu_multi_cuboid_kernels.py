"""GPU (-m gpu): the indexed gather of csrc/unproject.hip -- several cuboids per frame -- through lt_unproject_indexed_fwd and
lt_unproject_grid_indexed_fwd, at the smallest shapes that reach every branch of unproject_kernel<T, CH, SMALL_NV, true, true> and
unproject_qn_kernel<NVL, GRID, true, true>.

Expected value, bit for bit (torch.equal): the EXISTING entry (lt_unproject_fwd, lt_unproject_grid_fwd or their masked forms) run on the inputs gathered by
the index -- feats.index_select(0, frame_of), and likewise proj, conf and mask; for the grid entries the written coordinates are compared too.  Every
indexed call runs under both settings of the workgroup-mapping switch (LT_UNPROJ_PIN=cuboid | frame): the mapping must not change a bit.  The output is NaN
before every call and must be finite after it.  The kernels are never handed an out-of-range index here: the hosts refuse those
(tests/test_multi_cuboid_cpu.py), the clamp in the kernel is only the second line of defence."""
import numpy as np
import pytest
import torch

import lt_hip as H
from oracle import synth
from oracle import vol_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
AGGS = ("sum", "max", "softmax", "conf", "conf_norm")
# (F, frame_of): frame 1 without a cuboid; P = 8 (the XCD-pinned mapping); the identity over 8 frames; one frame
PATTERNS = {"F3P5": (3, [2, 0, 2, 2, 0]), "F3P8": (3, [1, 0, 2, 2, 0, 1, 1, 2]), "F8P8id": (8, list(range(8))), "F1P3": (1, [0, 0, 0])}
VOLUMES = {"5x3x7": (5, 3, 7), "4x4x16": (4, 4, 16), "16": (16, 16, 16), "32": (32, 32, 32)}


def _inputs(F, NV, C, h, w, dtype, seed):
    """Per-frame maps, confidences and projections: every frame has its own (a wrong frame cannot give the right bits)."""
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(F, NV, h, w, C, generator=g).to(DEV, dtype).contiguous()
    conf = (torch.rand(F, NV, C, generator=g) + 0.1).to(DEV).contiguous()
    K, R, t = synth.ring_cameras(NV, 96, inside=True)
    P = torch.from_numpy(O.resized_projection(K, R, t, (96, 96), (h, w))).float()[None].repeat(F, 1, 1, 1)
    P = (P * (1.0 + 0.02 * torch.randn(F, NV, 3, 4, generator=g))).to(DEV).contiguous()
    return feats, conf, P


def _coords(P, vs, seed):
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(P, 1, 1, 1, 3, generator=g) * 100
    ax = [torch.linspace(-1250.0, 1250.0, max(v, 2))[:v] for v in vs]
    grid = torch.stack(torch.meshgrid(*ax, indexing="ij"), dim=-1)[None]
    return (grid + base).to(DEV).contiguous()


def _cuboids(P, V, seed):
    g = torch.Generator().manual_seed(seed)
    base = (torch.randn(P, 3, generator=g) * 100).numpy().astype(np.float64)
    pos = torch.from_numpy((base - 1250.0).astype(np.float32)).to(DEV)
    cen = torch.from_numpy(base.astype(np.float32)).to(DEV)
    rot = torch.from_numpy(np.stack([O.rotation_matrix((0, 0, 1), 0.3 * p + 0.1) for p in range(P)]).astype(np.float32)).reshape(P, 9).to(DEV).contiguous()
    return pos, cen, rot, float(np.float32(2500.0 / (V - 1)))


def _plain(feats, P, cv, conf, agg, mask=None):
    """lt_unproject_fwd / lt_unproject_masked_fwd: the expected value's entry."""
    B, NV, h, w, C = feats.shape
    v0, v1, v2 = cv.shape[1:4]
    out = torch.full((B, v0, v1, v2, C), NAN, dtype=feats.dtype, device=DEV)
    cp = conf.data_ptr() if agg.startswith("conf") else None
    if mask is None:
        H.check(H.lib().lt_unproject_fwd(H.dtype_code(feats.dtype), feats.data_ptr(), P.data_ptr(), cv.data_ptr(), cp, out.data_ptr(), B, NV, C, h, w, v0, v1, v2,
                                         H.AGG[agg], H.cur_stream()), "lt_unproject_fwd")
    else:
        H.check(H.lib().lt_unproject_masked_fwd(H.dtype_code(feats.dtype), feats.data_ptr(), P.data_ptr(), cv.data_ptr(), cp, mask.data_ptr(), out.data_ptr(), B, NV,
                                                C, h, w, v0, v1, v2, H.AGG[agg], H.cur_stream()), "lt_unproject_masked_fwd")
    torch.cuda.synchronize()
    return out


def _plain_grid(feats, P, cub, V, cmu, conf, agg, mask=None):
    B, NV, h, w, C = feats.shape
    pos, cen, rot, step = cub
    out = torch.full((B, V, V, V, C), NAN, dtype=feats.dtype, device=DEV)
    coords = torch.full((B, V, V, V, 3), NAN, dtype=torch.float32, device=DEV)
    cp = conf.data_ptr() if agg.startswith("conf") else None
    if mask is None:
        H.check(H.lib().lt_unproject_grid_fwd(H.dtype_code(feats.dtype), feats.data_ptr(), P.data_ptr(), pos.data_ptr(), cen.data_ptr(), rot.data_ptr(), step, int(cmu),
                                              coords.data_ptr(), cp, out.data_ptr(), B, NV, C, h, w, V, H.AGG[agg], H.cur_stream()), "lt_unproject_grid_fwd")
    else:
        H.check(H.lib().lt_unproject_grid_masked_fwd(H.dtype_code(feats.dtype), feats.data_ptr(), P.data_ptr(), pos.data_ptr(), cen.data_ptr(), rot.data_ptr(), step,
                                                     int(cmu), coords.data_ptr(), cp, mask.data_ptr(), out.data_ptr(), B, NV, C, h, w, V, H.AGG[agg],
                                                     H.cur_stream()), "lt_unproject_grid_masked_fwd")
    torch.cuda.synchronize()
    return out, coords


def _indexed(monkeypatch, pin, feats, P, cv, conf, agg, fof, mask=None):
    F, NV, h, w, C = feats.shape
    n, v0, v1, v2 = cv.shape[:4]
    monkeypatch.setenv("LT_UNPROJ_PIN", pin)
    out = torch.full((n, v0, v1, v2, C), NAN, dtype=feats.dtype, device=DEV)
    H.check(H.lib().lt_unproject_indexed_fwd(H.dtype_code(feats.dtype), feats.data_ptr(), P.data_ptr(), cv.data_ptr(), conf.data_ptr() if agg.startswith("conf") else None,
                                             H.ptr(mask), fof.data_ptr(), out.data_ptr(), F, n, NV, C, h, w, v0, v1, v2, H.AGG[agg], H.cur_stream()),
            "lt_unproject_indexed_fwd")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()), "a voxel was not written, or not finite"
    return out


def _indexed_grid(monkeypatch, pin, feats, P, cub, V, cmu, conf, agg, fof, mask=None):
    F, NV, h, w, C = feats.shape
    pos, cen, rot, step = cub
    n = pos.shape[0]
    monkeypatch.setenv("LT_UNPROJ_PIN", pin)
    out = torch.full((n, V, V, V, C), NAN, dtype=feats.dtype, device=DEV)
    coords = torch.full((n, V, V, V, 3), NAN, dtype=torch.float32, device=DEV)
    H.check(H.lib().lt_unproject_grid_indexed_fwd(H.dtype_code(feats.dtype), feats.data_ptr(), P.data_ptr(), pos.data_ptr(), cen.data_ptr(), rot.data_ptr(), step,
                                                  int(cmu), coords.data_ptr(), conf.data_ptr() if agg.startswith("conf") else None, H.ptr(mask), fof.data_ptr(),
                                                  out.data_ptr(), F, n, NV, C, h, w, V, H.AGG[agg], H.cur_stream()), "lt_unproject_grid_indexed_fwd")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(coords).all()), "a voxel or a coordinate was not written"
    return out, coords


def _fof(frame_of):
    return torch.tensor(frame_of, dtype=torch.int32, device=DEV), torch.tensor(frame_of, dtype=torch.int64, device=DEV)


def _gather(idx, *ts):
    return [None if t is None else t.index_select(0, idx).contiguous() for t in ts]


# ---- the generic kernel: coordinates entry -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vol", list(VOLUMES))
@pytest.mark.parametrize("NV", [3, 9], ids=["smallNV3", "manyNV9"])
@pytest.mark.parametrize("dt,C", [("fp32", 4), ("fp32", 3), ("bf16", 8), ("bf16", 3)], ids=["fp32-CH4", "fp32-CH1", "bf16-CH8", "bf16-CH1"])
def test_generic_indexed_equals_the_gathered_call(monkeypatch, dt, C, NV, vol):
    """unproject_kernel<T, CH, SMALL_NV, true, true> with a null mask, every aggregation mode and every index pattern: linear chunks (5x3x7), one brick
    (4x4x16), bricks in raster order (16^3) and in blocked order (32^3)."""
    dtype = torch.float32 if dt == "fp32" else torch.bfloat16
    vs = VOLUMES[vol]
    for pname, (F, frame_of) in PATTERNS.items():
        feats, conf, P = _inputs(F, NV, C, 8, 8, dtype, seed=11 + F)
        cv = _coords(len(frame_of), vs, seed=5)
        fof, idx = _fof(frame_of)
        gf, gc, gP = _gather(idx, feats, conf, P)
        for agg in AGGS if vol in ("4x4x16", "16") else ("softmax", "conf_norm"):
            want = _plain(gf, gP, cv, gc, agg)
            for pin in ("cuboid", "frame"):
                got = _indexed(monkeypatch, pin, feats, P, cv, conf, agg, fof)
                assert torch.equal(got, want), "%s %s LT_UNPROJ_PIN=%s: %d elements differ" % (pname, agg, pin, int((got != want).sum()))


def test_generic_grid_indexed_runs_coord_volumes_over_the_cuboids(monkeypatch):
    """A grid call without a fused kernel (fp32): lt_coord_volumes over the P cuboids, then the indexed gather; volume and written coordinates."""
    for pname, (F, frame_of) in PATTERNS.items():
        feats, conf, P = _inputs(F, 3, 4, 8, 8, torch.float32, seed=21 + F)
        cub = _cuboids(len(frame_of), 16, seed=3)
        fof, idx = _fof(frame_of)
        gf, gc, gP = _gather(idx, feats, conf, P)
        for cmu in (0, 1):
            want, want_cv = _plain_grid(gf, gP, cub, 16, cmu, gc, "conf_norm")
            for pin in ("cuboid", "frame"):
                got, got_cv = _indexed_grid(monkeypatch, pin, feats, P, cub, 16, cmu, conf, "conf_norm", fof)
                assert torch.equal(got, want) and torch.equal(got_cv, want_cv), (pname, cmu, pin)


# ---- the quad kernel: bf16, 32 channels, 4 or 8 views, softmax, bricked ------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [16, 32], ids=["raster16", "blocked32"])
@pytest.mark.parametrize("NV", [4, 8], ids=["NVL1", "NVL2"])
def test_quad_indexed_equals_the_gathered_call(monkeypatch, NV, V):
    """unproject_qn_kernel<NVL, GRID, true, true> with a null mask: the coordinates entry and the grid entry with cmu 0 and 1, every index pattern."""
    for pname, (F, frame_of) in PATTERNS.items():
        feats, conf, P = _inputs(F, NV, 32, 8, 8, torch.bfloat16, seed=31 + F)
        n = len(frame_of)
        fof, idx = _fof(frame_of)
        gf, gP = _gather(idx, feats, P)
        cv = _coords(n, (V, V, V), seed=7)
        want = _plain(gf, gP, cv, None, "softmax")
        cub = _cuboids(n, V, seed=9)
        want_grid = [_plain_grid(gf, gP, cub, V, cmu, None, "softmax") for cmu in (0, 1)]
        for pin in ("cuboid", "frame"):
            got = _indexed(monkeypatch, pin, feats, P, cv, conf, "softmax", fof)
            assert torch.equal(got, want), (pname, pin, int((got != want).sum()))
            for cmu in (0, 1):
                got, got_cv = _indexed_grid(monkeypatch, pin, feats, P, cub, V, cmu, conf, "softmax", fof)
                assert torch.equal(got, want_grid[cmu][0]) and torch.equal(got_cv, want_grid[cmu][1]), (pname, pin, cmu)


# ---- with a view mask per frame ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["generic-fp32-NV3", "generic-fp32-NV9", "quad-NV4", "quad-NV8"])
def test_indexed_with_a_view_mask_equals_the_gathered_masked_call(monkeypatch, kernel):
    """One masked view per frame on top of the first index pattern; a masked view's map is NaN: it may not be read."""
    F, frame_of = PATTERNS["F3P5"]
    quad = kernel.startswith("quad")
    NV = int(kernel.rsplit("NV", 1)[1])
    C, dtype, V = (32, torch.bfloat16, 16) if quad else (4, torch.float32, 16)
    feats, conf, P = _inputs(F, NV, C, 8, 8, dtype, seed=41)
    mask = torch.ones(F, NV, dtype=torch.uint8)
    for f in range(F):
        mask[f, (f + 1) % NV] = 0
    feats[(mask == 0).to(DEV)] = NAN
    mask = mask.to(DEV)
    fof, idx = _fof(frame_of)
    gf, gc, gP, gm = _gather(idx, feats, conf, P, mask)
    cv = _coords(len(frame_of), (V, V, V), seed=13)
    cub = _cuboids(len(frame_of), V, seed=15)
    for agg in ("softmax",) if quad else AGGS:
        want = _plain(gf, gP, cv, gc, agg, gm)
        want_grid = _plain_grid(gf, gP, cub, V, 1, gc, agg, gm)
        assert bool(torch.isfinite(want).all())
        for pin in ("cuboid", "frame"):
            got = _indexed(monkeypatch, pin, feats, P, cv, conf, agg, fof, mask)
            assert torch.equal(got, want), (agg, pin)
            got, got_cv = _indexed_grid(monkeypatch, pin, feats, P, cub, V, 1, conf, agg, fof, mask)
            assert torch.equal(got, want_grid[0]) and torch.equal(got_cv, want_grid[1]), (agg, pin)


def test_entries_refuse_bad_arguments():
    lib = H.lib()
    feats, conf, P = _inputs(2, 3, 4, 8, 8, torch.float32, seed=1)
    cv = _coords(2, (4, 4, 16), seed=1)
    out = torch.empty(2, 4, 4, 16, 4, device=DEV)
    fof = torch.zeros(2, dtype=torch.int32, device=DEV)
    call = lambda fo, F, n: lib.lt_unproject_indexed_fwd(H.LT_F32, feats.data_ptr(), P.data_ptr(), cv.data_ptr(), None, None, fo, out.data_ptr(), F, n, 3, 4, 8, 8, 4, 4, 16,
                                                         H.AGG["sum"], H.cur_stream())
    assert call(None, 2, 2) != 0 and b"frame_of" in lib.lt_last_error()
    assert call(fof.data_ptr(), 0, 2) != 0 and b"F 0" in lib.lt_last_error()
    assert call(fof.data_ptr(), 2, 0) != 0 and b"P 0" in lib.lt_last_error()
    assert call(fof.data_ptr(), 2, 2) == 0
    torch.cuda.synchronize()
