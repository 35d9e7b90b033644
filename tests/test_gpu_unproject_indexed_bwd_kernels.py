"""GPU (-m gpu): lt_unproject_indexed_bwd (csrc/unproject_bwd.hip) -- the INDEXED forms of K0, of every K1 form and of the gather K2, and the indexed
confidence finalizer, through the entry itself.  What a frame index means is stated by tests/unproject_bwd_indexed_ref.py (the per-cuboid reference on the
cuboid's frame, index_add over frame_of); tests/test_unproject_bwd_indexed_ref_cpu.py holds that statement and the cases below to their conditions.

* one cuboid per frame: the bits of lt_unproject_bwd (NULL mask) and lt_unproject_masked_bwd, every aggregation, fp32 and bf16 maps, NV = 2, 4, 7, 10
* lattice inputs (every product and sum exact in fp32): several cuboids per frame, an empty frame, unsorted -- the bits of the sum of the unindexed results
* the same bits for every workspace size (chunks of 1, 2 and all cuboids), conf_norm on Gaussian data included; repeatable; masked views never read
* Gaussian data against the fp64 statement at 1e-4 of max|ref| (the gate of tests/test_gpu_unproject_bwd_many_views.py); the refusals."""
import pytest
import torch

import lt_hip as H
import unproject_bwd_indexed_ref as X
import unproject_bwd_masked_ref as M
import unproject_bwd_ref as R
from gpu_util import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(autouse=True)
def _gather_path(monkeypatch):
    monkeypatch.delenv("LT_UNPROJ_BWD_ATOMICS", raising=False)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _indexed(hm, P, conf, cv, G, agg, frame_of, mask=None, chunk=None, expect=0, **over):
    """lt_unproject_indexed_bwd itself: device tensors in the public layouts (hm (F,NV,C,h,w), cv (P,v0,v1,v2,3), G (P,C,v0,v1,v2)) -> (grad_feats
    (F,NV,C,h,w), grad_conf (F,NV,C) or None); both buffers start as NaN.  chunk: workspace for that many cuboids at a time (None: all)."""
    Fn, NV, C, h, w = hm.shape
    Pn = cv.shape[0]
    vs = tuple(cv.shape[1:4])
    feats = hm.permute(0, 1, 3, 4, 2).contiguous()
    g = G.permute(0, 2, 3, 4, 1).float().contiguous()
    gf = torch.full((Fn, NV, h, w, C), float("nan"), dtype=torch.float32, device=hm.device)
    is_conf = agg.startswith("conf")
    gc = torch.full((Fn, NV, C), float("nan"), dtype=torch.float32, device=hm.device) if is_conf else None
    lib = H.lib()
    fof = None if frame_of is None else torch.tensor(list(frame_of), dtype=torch.int32, device=hm.device)
    nws = X.ws_bytes(lib, Pn, NV, C, vs, chunk) if expect == 0 else 1 << 20
    ws = torch.empty(max(16, nws), dtype=torch.uint8, device=hm.device)
    rc = lib.lt_unproject_indexed_bwd(H.dtype_code(hm.dtype), feats.data_ptr(), P.data_ptr(), cv.data_ptr(), conf.data_ptr() if is_conf else None, H.ptr(mask),
                                      H.ptr(fof), g.data_ptr(), gf.data_ptr(), H.ptr(gc), over.get("nF", Fn), over.get("nP", Pn), NV, C, h, w, *vs, H.AGG[agg],
                                      ws.data_ptr(), nws, _stream())
    if expect != 0:
        assert rc == expect, (rc, lib.lt_last_error())
        return None, None
    H.check(rc, "lt_unproject_indexed_bwd")
    torch.cuda.synchronize()
    return gf.permute(0, 1, 4, 2, 3), gc


def _unindexed(hm, P, conf, cv, G, agg, mask=None):
    """lt_unproject_bwd (mask None) / lt_unproject_masked_bwd on B samples, whole-batch workspace."""
    B, NV, C, h, w = hm.shape
    vs = tuple(cv.shape[1:4])
    feats = hm.permute(0, 1, 3, 4, 2).contiguous()
    g = G.permute(0, 2, 3, 4, 1).float().contiguous()
    gf = torch.full((B, NV, h, w, C), float("nan"), dtype=torch.float32, device=hm.device)
    is_conf = agg.startswith("conf")
    gc = torch.full((B, NV, C), float("nan"), dtype=torch.float32, device=hm.device) if is_conf else None
    lib = H.lib()
    nws = lib.lt_unproject_bwd_workspace(B, NV, C, *vs)
    ws = torch.empty(max(16, nws), dtype=torch.uint8, device=hm.device)
    head = (H.dtype_code(hm.dtype), feats.data_ptr(), P.data_ptr(), cv.data_ptr(), conf.data_ptr() if is_conf else None)
    tail = (g.data_ptr(), gf.data_ptr(), H.ptr(gc), B, NV, C, h, w, *vs, H.AGG[agg], ws.data_ptr(), nws, _stream())
    if mask is None:
        H.check(lib.lt_unproject_bwd(*head, *tail), "lt_unproject_bwd")
    else:
        H.check(lib.lt_unproject_masked_bwd(*head, mask.data_ptr(), *tail), "lt_unproject_masked_bwd")
    torch.cuda.synchronize()
    return gf.permute(0, 1, 4, 2, 3), gc


def _dev(ts, dtype=F32):
    hm, P, conf, cv, G = ts
    return [hm.to(dtype).to(DEV)] + [t.to(DEV) for t in (P, conf, cv, G)]


SMALL = dict(C=8, hw=(20, 37), vs=(5, 6, 7), F=3, P=3)          # ragged tiles and bricks, more than one tile, more than one K1 workgroup


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("NV", [2, 4, 7, 10])
def test_one_cuboid_per_frame_gives_the_unindexed_entries_bits(NV, dtype):
    """frame_of = 0 .. F-1: lt_unproject_bwd's bits with a NULL mask, lt_unproject_masked_bwd's with a mask -- the <= 4, <= 8, passes and groups forms of K1,
    both finalizers' arithmetic, every aggregation.  A permuted frame_of gives every frame the unindexed result of the cuboid that names it."""
    host = X.gaussian_case(NV, seed=7200 + NV, **SMALL)
    hm, P, conf, cv, G = _dev(host, dtype)
    mask = M.mask_rows(NV, B=3).to(DEV)
    perm = [2, 0, 1]
    pi = torch.tensor(perm, device=DEV)
    for agg in X.AGGS:
        for mk in (None, mask):
            rf, rc = _unindexed(hm, P, conf, cv, G, agg, mk)
            gf, gc = _indexed(hm, P, conf, cv, G, agg, [0, 1, 2], mk)
            assert torch.isfinite(gf).all() and float(rf.abs().max()) > 0
            assert torch.equal(gf, rf), (agg, mk is not None)
            assert gc is None or torch.equal(gc, rc), (agg, mk is not None)
            # cuboid p on frame perm[p]: the unindexed run on the frames gathered by perm, scattered back to the frames
            uf, uc = _unindexed(hm[pi].contiguous(), P[pi].contiguous(), conf[pi].contiguous(), cv, G, agg, None if mk is None else mk[pi].contiguous())
            gf, gc = _indexed(hm, P, conf, cv, G, agg, perm, mk)
            assert torch.equal(gf[pi], uf), (agg, mk is not None)
            assert gc is None or torch.equal(gc[pi], uc), (agg, mk is not None)


@pytest.mark.parametrize("vs", [(8, 4, 12), (5, 6, 7)], ids=["8x4x12", "ragged"])
@pytest.mark.parametrize("C", [4, 8, 32])
def test_lattice_several_cuboids_per_frame_bit_for_bit(C, vs):
    """F = 3, frame_of = [2, 0, 2, 2, 0] on the lattice (exact whatever the addition order): grad_feats[f] and grad_conf[f] are the bits of the sum of the
    five unindexed per-cuboid results over frame_of -- and of the fp64 statement --, frame 1 is all zeros."""
    frames, cv, G = X.lattice_frames_case(4, C, vs, 900 + C)
    fof = list(X.LATTICE_FRAME_OF)
    hm, P, conf, cvd, Gd = _dev((frames.hm, frames.P, frames.conf, cv, G))
    idx = torch.tensor(fof, device=DEV)
    for agg in X.EXACT_AGGS:
        uf, uc = _unindexed(hm[idx].contiguous(), P[idx].contiguous(), conf[idx].contiguous(), cvd, Gd, agg)
        sf = torch.zeros_like(uf[:X.LATTICE_F]).index_add_(0, idx, uf)
        gf, gc = _indexed(hm, P, conf, cvd, Gd, agg, fof)
        assert torch.equal(gf, sf), agg
        assert float(gf[1].abs().max()) == 0 and float(gf[2].abs().max()) > 0
        ef, ec = X.indexed_ref_backward(frames.hm, frames.P, cv, G, agg, fof, frames.conf)
        assert torch.equal(gf.cpu().double(), ef), agg
        if agg == "conf":
            assert torch.equal(gc, torch.zeros_like(uc[:X.LATTICE_F]).index_add_(0, idx, uc))
            assert torch.equal(gc.cpu().double(), ec) and float(gc[1].abs().max()) == 0


@pytest.mark.parametrize("kind", ["lattice", "gaussian"])
def test_every_workspace_size_gives_the_same_bits(kind):
    """Workspace for 1, 2 and all 5 cuboids at a time: with 2, a chunk boundary falls between frame 2's cuboids (p = 2 | 3), and K2 goes on from the stored
    tile.  Both gradients bit-equal, conf_norm on Gaussian data included."""
    if kind == "lattice":
        frames, cv, G = X.lattice_frames_case(4, 8, (5, 6, 7), 908)
        dev, fof, aggs = _dev((frames.hm, frames.P, frames.conf, cv, G)), list(X.LATTICE_FRAME_OF), X.EXACT_AGGS
    else:
        dev = _dev(X.gaussian_case(4, seed=7301, C=8, hw=(20, 37), vs=(5, 6, 7), F=3, P=5))
        fof, aggs = list(X.LATTICE_FRAME_OF), X.AGGS
    for agg in aggs:
        gf, gc = _indexed(*dev, agg, fof)
        for chunk in (1, 2):
            cf, cc = _indexed(*dev, agg, fof, chunk=chunk)
            assert torch.equal(gf, cf), (agg, chunk)
            assert gc is None or torch.equal(gc, cc), (agg, chunk)


@pytest.mark.parametrize("NV", [4, 10])
def test_repeatable_and_masked_views_are_never_read(NV):
    host = X.gaussian_case(NV, seed=7400 + NV, C=8, hw=(20, 37), vs=(5, 6, 7), F=3, P=5)
    fof = list(X.LATTICE_FRAME_OF)
    mask = M.mask_rows(NV, B=3)
    hm, P, conf, cv, G = host
    off = mask == 0
    hm_n, P_n, conf_n = hm.clone(), P.clone(), conf.clone()
    hm_n[off], P_n[off], conf_n[off] = float("nan"), float("nan"), float("nan")
    clean, dirty, mk = _dev(host), _dev((hm_n, P_n, conf_n, cv, G)), mask.to(DEV)
    for agg in X.AGGS:
        a = _indexed(*clean, agg, fof)
        b = _indexed(*clean, agg, fof)
        assert torch.equal(a[0], b[0]) and (a[1] is None or torch.equal(a[1], b[1])), agg
        m = _indexed(*clean, agg, fof, mk)
        n = _indexed(*dirty, agg, fof, mk)
        assert torch.isfinite(n[0]).all() and torch.equal(m[0], n[0]), agg
        assert float(n[0][off.to(DEV)].abs().max()) == 0 and float(n[0][1].abs().max()) == 0          # masked views and the empty frame: exactly zero
        if n[1] is not None:
            assert torch.isfinite(n[1]).all() and torch.equal(m[1], n[1]) and float(n[1][off.to(DEV)].abs().max()) == 0


@pytest.mark.parametrize("NV", [4, 10])
def test_gaussian_data_against_the_fp64_statement(NV):
    """F = 2, P = 5, C = 32, 24 x 24 maps, 16^3 voxels, all five aggregations: max|d| <= 1e-4 max|ref|, features and confidences."""
    host = X.gaussian_case(NV)
    hm, P, conf, cv, G = host
    fof = list(X.GATE_FRAME_OF)
    dev = _dev(host)
    for agg in X.AGGS:
        rf, rc = X.indexed_ref_backward(hm, P, cv, G, agg, fof, conf)
        gf, gc = _indexed(*dev, agg, fof)
        e = check("bwd/unproject indexed NV=%d %s: d/d features" % (NV, agg), gf.cpu(), rf, 1e-4)
        print("indexed NV=%d %s: d/d features max|d|/max|ref| = %.3e" % (NV, agg, e))
        if agg.startswith("conf"):
            e = check("bwd/unproject indexed NV=%d %s: d/d confidences" % (NV, agg), gc.cpu(), rc, 1e-4)
            print("indexed NV=%d %s: d/d confidences max|d|/max|ref| = %.3e" % (NV, agg, e))


def test_refusals_launch_nothing(monkeypatch):
    dev = _dev(X.gaussian_case(4, seed=7501, C=8, hw=(12, 14), vs=(4, 4, 4), F=2, P=3))
    fof = [0, 1, 1]
    _indexed(*dev, "sum", None, expect=-1)
    assert b"frame_of" in H.lib().lt_last_error()
    _indexed(*dev, "sum", fof, expect=-1, nP=0)
    _indexed(*dev, "sum", fof, expect=-1, nF=0)
    hm, P, conf, cv, G = X.gaussian_case(4, seed=7502, C=12, hw=(12, 14), vs=(4, 4, 4), F=2, P=3)
    _indexed(*_dev((hm, P, conf, cv, G)), "sum", fof, expect=-2)
    assert b"power of two" in H.lib().lt_last_error()
    monkeypatch.setenv("LT_UNPROJ_BWD_ATOMICS", "1")
    _indexed(*dev, "sum", fof, expect=-2)
    assert b"LT_UNPROJ_BWD_ATOMICS" in H.lib().lt_last_error()
    torch.cuda.synchronize()
