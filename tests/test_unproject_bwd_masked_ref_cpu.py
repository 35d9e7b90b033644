"""The test infrastructure of the masked unprojection backward (tests/unproject_bwd_masked_ref.py), checked without a GPU -- here the reference alone is on
trial: masked_ref_backward against fp64 autograd through the restated forward (unproject_ref.ref_unproject) on every sample's valid views; for every lattice
case of tests/test_gpu_unproject_masked_bwd_kernels.py the conditions its slack-free gate rests on; the no-flip condition of every 'max' case; the masks the
cases promise; masked_bwd_plan's branches and refusals, and the refusals of lt_unproject_masked_bwd that need no device."""
import pytest
import torch

import lt_hip as H
import unproject_bwd_masked_ref as M
import unproject_bwd_ref as R
import unproject_ref as U


@pytest.fixture(autouse=True)
def _gather_path(monkeypatch):
    monkeypatch.delenv("LT_UNPROJ_BWD_ATOMICS", raising=False)


def _autograd_on_valid_views(c, mask, agg):
    """fp64 autograd of the restated forward, sample by sample on the valid views; zeros elsewhere."""
    B, NV, C, h, w = c.hm.shape
    gf, gc = torch.zeros(B, NV, C, h, w, dtype=torch.float64), torch.zeros(B, NV, C, dtype=torch.float64)
    for b in range(B):
        idx = M.valid_views(mask, b)
        h64 = c.hm[b:b + 1, idx].double().requires_grad_(True)
        c64 = c.conf[b:b + 1, idx].double().requires_grad_(True) if agg.startswith("conf") else None
        out, _ = U.ref_unproject(h64, c.P[b:b + 1, idx], c.cv[b:b + 1], agg, c64)
        (out.reshape(1, -1, C) * c.G[b:b + 1].double().reshape(1, C, -1).permute(0, 2, 1)).sum().backward()
        gf[b, idx] = h64.grad[0]
        if c64 is not None:
            gc[b, idx] = c64.grad[0]
    return gf, gc


@pytest.mark.parametrize("cid", ["NV4_C8", "NV7_C8"])
def test_masked_reference_equals_fp64_autograd_on_the_valid_views(cid):
    """Realistic geometry, all five aggregations, 1e-12 of max|ref|; masked views exactly zero; the same through the forward reference's own mask argument."""
    NV, C, mask = M.REAL_SMALL[cid]
    c = R.realistic_case(NV, C)
    for agg in M.AGGS:
        gf, gc, mag, _ = M.masked_ref_backward(c.hm, c.P, c.cv, c.G, agg, mask, c.conf)
        af, ac = _autograd_on_valid_views(c, mask, agg)
        assert float(af.abs().max()) > 0
        assert float((gf - af).abs().max()) <= 1e-12 * float(af.abs().max()), agg
        off = mask == 0
        assert float(gf[off].abs().max()) == 0 and float(mag.feats[off].abs().max()) == 0
        assert bool((gf.abs() <= mag.feats * (1 + 1e-12)).all())
        if agg.startswith("conf"):
            assert float((gc - ac).abs().max()) <= 1e-12 * float(ac.abs().max()), agg
            assert float(gc[off].abs().max()) == 0
        else:
            assert gc is None
        # the restated forward with its mask argument is the same function: its autograd gives the same gradients, zeros for the masked views
        h64 = c.hm.double().requires_grad_(True)
        c64 = c.conf.double().requires_grad_(True) if agg.startswith("conf") else None
        out, _ = U.ref_unproject(h64, c.P, c.cv, agg, c64, mask=mask.bool())
        (out.reshape(2, -1, C) * c.G.double().reshape(2, C, -1).permute(0, 2, 1)).sum().backward()
        assert float((h64.grad - gf).abs().max()) <= 1e-12 * float(af.abs().max()), agg
        assert float(h64.grad[off].abs().max()) == 0


@pytest.mark.parametrize("cid", sorted(M.EXACT))
def test_masked_lattice_case_is_exact_in_fp32_and_enters_its_branch(cid):
    """exact.assert_exact holds for every sample's compacted views (inside lattice_reference); the fp32 statement equals the fp64 one bit for bit; the maps are
    bf16 numbers; masked_bwd_plan names the K1 form and the finalizer the id promises; every valid view receives a gradient and every masked one none."""
    spec, case = M.EXACT[cid], M.make(M.EXACT, cid)
    mask = spec["mask"]
    B, NV, C, h, w = case.hm.shape
    on = mask != 0
    assert torch.equal(case.hm[on], case.hm[on].bfloat16().float())
    assert bool(torch.isnan(case.hm[~on]).all()) == spec["nan"] and bool(torch.isnan(case.P[~on]).all()) == spec["nan"]
    N = case.vs[0] * case.vs[1] * case.vs[2]
    for agg in spec["aggs"]:
        plan = M.masked_bwd_plan(spec["dtype"], B, NV, C, h, w, case.vs, agg, env={})
        R.plan_is(plan, k1=M._k1(NV, agg), finalizer=None if agg != "conf" else ("many" if NV > 8 else "small"), masked=True, **spec["plan"])
        gf, gc = M.lattice_reference(cid, case, mask, agg, R.conf_terms(plan, N))
        f32, c32, _, _ = M.masked_ref_backward(case.hm, case.P, case.cv, case.G, agg, mask, case.conf, dtype=torch.float32)
        assert f32.dtype == torch.float32 and torch.equal(f32, gf), "%s %s: fp32 and fp64 statements differ" % (cid, agg)
        assert gc is None or torch.equal(c32, gc), "%s %s: confidence gradient" % (cid, agg)
        assert bool(torch.isfinite(gf).all())
        if agg == "sum":
            for b in range(B):
                for v in range(NV):
                    assert (float(gf[b, v].abs().max()) > 0) == bool(on[b, v]), (cid, b, v)


def _all_max_cases():
    for cid in sorted(M.EXACT):
        yield "exact/" + cid, M.make(M.EXACT, cid), M.EXACT[cid]["mask"]
    for cid, (NV, C, mask) in sorted(M.REAL_SMALL.items()):
        yield "real/" + cid, R.realistic_case(NV, C), mask


@pytest.mark.parametrize("name,case,mask", list(_all_max_cases()), ids=[n for n, _, _ in _all_max_cases()])
def test_no_max_winner_differs_between_fp32_and_fp64_among_the_valid_views(name, case, mask):
    """The condition of every gate on 'max': the winning view is the same in the fp32 and in the fp64 statement, and it is a valid view.  bf16 maps as well."""
    for hm in (case.hm, case.hm.bfloat16().float()):
        _, _, _, w64 = M.masked_ref_backward(hm, case.P, case.cv, case.G, "max", mask)
        _, _, _, w32 = M.masked_ref_backward(hm, case.P, case.cv, case.G, "max", mask, dtype=torch.float32)
        for b, (a, c) in enumerate(zip(w64, w32)):
            assert torch.equal(a, c), "%s: sample %d has a 'max' winner that differs between fp32 and fp64" % (name, b)
            assert bool((mask[b][a] != 0).all()), "a masked view wins"


def test_masks_cover_what_the_cases_promise():
    """Per lattice case: a fully valid sample, a sample with exactly one view masked, a sample with a single valid view, rows that differ; beyond 8 views a
    whole group of 8 without a valid view and a first valid view other than view 0.  The realistic masks keep the valid count on NV's side of 4; the
    crossing case does not."""
    for cid, spec in M.EXACT.items():
        m = spec["mask"]
        NV = m.shape[1]
        n = m.sum(1).tolist()
        assert n[0] == NV and n[1] == NV - 1 and n[2] == 1 and m.dtype == torch.uint8, (cid, n)
        assert len({tuple(r.tolist()) for r in m}) >= 2
        if NV > 8:
            assert int(m[2, :8].sum()) == 0 and any(int(r[0]) == 0 for r in m)
    for cid, (NV, C, m) in M.REAL_SMALL.items():
        assert all((int(k) <= 4) == (NV <= 4) and int(k) >= 1 for k in m.sum(1)), cid
        assert not torch.equal(m[0], m[1])
    for cid, (NV, C, m) in M.REAL_MANY.items():
        assert int(m[1, :8].sum()) == 0 and int(m[0, 0]) == 0 and all(int(k) >= 1 for k in m.sum(1)), cid
    k = M.CROSS["mask"].sum(1).tolist()
    assert M.CROSS["mask"].shape[1] == 5 and k == [3, 3]
    assert {M._k1(NV, a) for NV, _ in M.ALL_ONES for a in M.AGGS} == {"mv4", "mv8", "passes", "groups"}


def test_masked_plan_restates_the_dispatch_and_the_refusals():
    p = M.masked_bwd_plan(M.F32, 2, 4, 32, 24, 28, (6, 5, 9), "softmax", env={})
    u = R.bwd_plan(M.F32, 2, 4, 32, 24, 28, (6, 5, 9), "softmax", env={})
    assert p["masked"] and {k: v for k, v in p.items() if k != "masked"} == u, "the masked entry takes the unmasked entry's workspace, chunks and kernels"
    assert M.masked_bwd_plan(M.F32, 2, 4, 32, 24, 28, (6, 5, 9), "sum", mask_given=False, env={})["refused"] == (-1, "null view_mask")
    assert M.masked_bwd_plan(M.F32, 2, 4, 96, 24, 28, (6, 5, 9), "sum", env={})["refused"] == (-2, "only the gather path takes a view mask")
    assert M.masked_bwd_plan(M.F32, 2, 4, 12, 24, 28, (6, 5, 9), "conf_norm", env={})["refused"] == (-2, "only the gather path takes a view mask")
    assert M.masked_bwd_plan(M.F32, 2, 4, 32, 24, 28, (6, 5, 9), "sum", env={"LT_UNPROJ_BWD_ATOMICS": "1"})["refused"] == (-2, "LT_UNPROJ_BWD_ATOMICS")
    assert M.masked_bwd_plan(M.F32, 2, 33, 32, 24, 28, (6, 5, 9), "sum", env={})["refused"] == (-2, "NV <= 32")
    assert M.masked_bwd_plan(M.F32, 3, 4, 8, 24, 28, (6, 5, 9), "sum", env={}, ws_samples=1)["nchunks"] == 3


def test_entry_refuses_without_a_device(monkeypatch):
    """The refusals of lt_unproject_masked_bwd come before any launch: a null mask, a C the gather does not take, LT_UNPROJ_BWD_ATOMICS; return code and message
    as masked_bwd_plan states them.  (Pointers are never dereferenced on the host.)"""
    lib = H.lib()
    d = 256          # any non-null address

    def call(C, agg="sum", mask=d, NV=4):
        return lib.lt_unproject_masked_bwd(H.LT_F32, d, d, d, d, mask, d, d, d, 2, NV, C, 24, 28, 6, 5, 9, H.AGG[agg], d, 1 << 40, None)
    for kw, env in ((dict(C=32, mask=None), {}), (dict(C=96), {}), (dict(C=12, agg="conf_norm"), {}), (dict(C=32), {"LT_UNPROJ_BWD_ATOMICS": "1"}), (dict(C=32, NV=33), {})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        want = M.masked_bwd_plan(M.F32, 2, kw.get("NV", 4), kw["C"], 24, 28, (6, 5, 9), kw.get("agg", "sum"), mask_given=kw.get("mask", d) is not None, env=env)["refused"]
        assert call(**kw) == want[0], (kw, lib.lt_last_error())
        msg = lib.lt_last_error().decode()
        assert msg.startswith("lt_unproject_masked_bwd:") and want[1] in msg, (want, msg)
        monkeypatch.delenv("LT_UNPROJ_BWD_ATOMICS", raising=False)
