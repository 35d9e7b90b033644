"""TEST INFRASTRUCTURE for the masked unprojection backward (lt_unproject_masked_bwd, csrc/unproject_bwd.hip): importable without a GPU.

* masked_ref_backward(): what a view mask MEANS in the backward, stated through the unmasked reference -- unproject_bwd_ref.ref_backward called per sample on
  the sample's valid views alone (compacted, in index order), the result scattered back with zeros for the masked views; fp64, or fp32 as the kernels state it.
  A masked view's maps, matrix and confidences are never touched, so NaN there cannot reach the result.
* masked_bwd_plan(): the dispatch and the refusals of the masked entry restated on top of unproject_bwd_ref.bwd_plan (the gather path only).
* the case tables of tests/test_gpu_unproject_masked_bwd_kernels.py: EXACT (lattice inputs, sum / max / conf bit for bit, every K1 form), REAL (ring cameras,
  randn maps), CROSS (the softmax case whose valid count crosses the 4-view register form), each with its mask -- a fully valid sample, a sample with one view
  masked, a sample with a single valid view, rows that differ between the samples -- here so that tests/test_unproject_bwd_masked_ref_cpu.py can hold every
  case to the conditions its gate rests on."""
import os

import torch

import unproject_bwd_ref as R
import unproject_ref as U

AGGS, EXACT_AGGS = R.AGGS, R.EXACT_AGGS
F32, BF16 = torch.float32, torch.bfloat16


def _sub(case, b, idx):
    """Sample b of a case on the views idx alone, as a one-sample Case."""
    return R.Case(case.hm[b:b + 1, idx], case.P[b:b + 1, idx], case.cv[b:b + 1], case.conf[b:b + 1, idx], case.G[b:b + 1], case.h, case.w, case.vs, None, None, None)


def valid_views(mask, b):
    return [v for v in range(mask.shape[1]) if int(mask[b, v]) != 0]


def masked_ref_backward(hm, proj, coords, G, agg, mask, conf=None, dtype=torch.float64):
    """hm (B,NV,C,h,w), proj (B,NV,3,4), coords (B,v0,v1,v2,3), G (B,C,v0,v1,v2), mask (B,NV) non-zero = valid, conf (B,NV,C)
    -> (grad_feats (B,NV,C,h,w), grad_conf (B,NV,C) or None, Mag, winners): ref_backward of every sample on its valid views alone, zeros (and zero
    magnitudes) for the masked views; a sample without a valid view is all zeros.  winners: per sample the 'max' winner (N, C) as an ORIGINAL view
    index (None for the other aggregations)."""
    B, NV, C, h, w = hm.shape
    is_conf = agg in ("conf", "conf_norm")
    gf, mf = torch.zeros(B, NV, C, h, w, dtype=dtype), torch.zeros(B, NV, C, h, w, dtype=dtype)
    gc = torch.zeros(B, NV, C, dtype=dtype) if is_conf else None
    mc = torch.zeros(B, NV, C, dtype=torch.float64) if is_conf else None
    winners = []
    for b in range(B):
        idx = valid_views(mask, b)
        if not idx:
            winners.append(None)
            continue
        f, c, mag, rec = R.ref_backward(hm[b:b + 1, idx], proj[b:b + 1, idx], coords[b:b + 1], G[b:b + 1], agg, None if conf is None else conf[b:b + 1, idx], dtype=dtype)
        gf[b, idx], mf[b, idx] = f[0], mag.feats[0]
        if is_conf:
            gc[b, idx], mc[b, idx] = c[0], mag.conf[0]
        winners.append(None if rec.winner is None else torch.tensor(idx)[rec.winner[0]])
    return gf, gc, R.Mag(mf, mc), winners


def masked_bwd_plan(dtype, B, NV, C, h, w, v, agg, mask_given=True, env=None, ws_samples=None, has_conf=None):
    """lt_unproject_masked_bwd's checks and dispatch: lt_unproject_bwd's argument checks (with the null mask behind the null arguments), then the two
    refusals of its own -- LT_UNPROJ_BWD_ATOMICS set, a C the gather does not take -- then the gather's plan, K1 and finalizers in their MASKED forms."""
    env = os.environ if env is None else env
    if not mask_given:
        return dict(refused=(-1, "null view_mask"), path=None, agg=agg)
    p = R.bwd_plan(dtype, B, NV, C, h, w, v, agg, env={}, ws_samples=ws_samples, has_conf=has_conf)
    if p["refused"] and p["path"] is None and p["refused"][1] != "conf_norm needs the gather path":
        return p                                                       # an argument check
    if U._env_on(env, "LT_UNPROJ_BWD_ATOMICS"):
        return dict(p, refused=(-2, "LT_UNPROJ_BWD_ATOMICS"), path=None)
    if p["path"] != "gather":
        return dict(p, refused=(-2, "only the gather path takes a view mask"), path=None)
    return dict(p, masked=True)


# ---- masks -----------------------------------------------------------------------------------------------------------------------------------------
def mask_rows(NV, B=3):
    """Row 0 fully valid; row 1 with one view masked (view 0 for even NV -- the first valid view is then not view 0 -- a middle view for odd NV); row 2
    with a single valid view (the last one: for NV > 8 every group of 8 views but the last has no valid view, and the passes start at a late view)."""
    m = torch.ones(B, NV, dtype=torch.uint8)
    if B > 1:
        m[1, 0 if NV % 2 == 0 else NV // 2] = 0
    if B > 2:
        m[2] = 0
        m[2, NV - 1] = 1
    return m


def with_nan(case, mask):
    """The case with NaN in everything a masked view owns: its maps, its projection matrix, its confidences."""
    hm, P, conf = case.hm.clone(), case.P.clone(), case.conf.clone()
    off = mask == 0
    hm[off], P[off], conf[off] = float("nan"), float("nan"), float("nan")
    return case._replace(hm=hm, P=P, conf=conf)


# ---- the case tables ---------------------------------------------------------------------------------------------------------------------------------
MAPS, GRIDS = {"seam": R.SEAM_HW, "sq": (16, 16)}, {"cube": (8, 8, 8), "ragged": (5, 6, 7)}


def _case(make, mask, aggs, dtype=F32, nan=False, **plan):
    return dict(make=make, mask=mask, aggs=tuple(aggs), dtype=dtype, nan=nan, plan=plan)


def _k1(NV, agg):
    if NV > R.UB_MAXV:
        return "passes" if agg in ("softmax", "max") else "groups"
    return "mv4" if NV <= 4 else "mv8"


def _lattice(NV, C, maps, grid, seed, B=3):
    h, w = MAPS[maps]
    dup = {8: 0} if NV == 9 else ({8: 0, 16: 1, 12: 0} if NV >= 17 else None)          # exact 'max' ties across the groups of 8 views
    return R.lattice_case(B, NV, C, h, w, GRIDS[grid], seed, dup=dup)


# id -> NV, C, maps, grid, dtype: every K1 form (mv4: NV 2, 4; mv8: NV 7, 8; passes / groups and the many-view finalizer: NV 9, 17, 32), both map types,
# C = 4 (CW 1), 8, 32, both map sizes (33 x 17: ragged tiles, 16 x 16: one tile), a whole and a ragged brick grid
_EXACT_SHAPES = {"NV2_C4_f32": (2, 4, "sq", "cube", F32), "NV4_C8_bf16": (4, 8, "seam", "ragged", BF16), "NV7_C32_f32": (7, 32, "seam", "ragged", F32),
                 "NV8_C8_f32": (8, 8, "sq", "cube", F32), "NV8_C4_bf16": (8, 4, "seam", "cube", BF16), "NV9_C8_f32": (9, 8, "seam", "ragged", F32),
                 "NV17_C32_bf16": (17, 32, "sq", "ragged", BF16), "NV32_C4_f32": (32, 4, "seam", "cube", F32)}
EXACT = {}
for _i, (_id, (_NV, _C, _m, _g, _dt)) in enumerate(sorted(_EXACT_SHAPES.items())):
    EXACT[_id] = _case(lambda a=(_NV, _C, _m, _g, 400 + _i): _lattice(*a), mask_rows(_NV), EXACT_AGGS, dtype=_dt, path="gather", CW=_C // 4, many=_NV > 8)
# NaN in the masked views' maps, matrices and confidences: the bits of the clean case
for _id in ("NV4_C8_bf16", "NV9_C8_f32"):
    EXACT[_id + "_nan"] = dict(EXACT[_id], nan=True)
CHUNKS = "NV4_C8_bf16"          # B = 3, three different mask rows: the chunked walk of the batch

# softmax across the 4-view register form: 5 views (unproj_dx_kernel<T, 8>), three valid (the compacted run takes <T, 4>)
CROSS = _case(lambda: _lattice(5, 8, "seam", "ragged", 450, B=2), torch.tensor([[1, 0, 1, 0, 1], [0, 1, 1, 1, 0]], dtype=torch.uint8), ("softmax",),
              path="gather", CW=2, k1="mv8")

# realistic geometry (unproject_bwd_ref.realistic_case: B = 2): NV <= 8 against the compacted unmasked run, bit for bit -- the masks keep the valid count on
# NV's side of 4, so that both runs take the same K1 instantiation --; NV > 8 against fp64
REAL_MASKS = {2: [[1, 1], [0, 1]], 4: [[1, 0, 1, 1], [0, 0, 1, 0]], 7: [[1, 1, 0, 1, 1, 1, 1], [0, 1, 1, 1, 0, 1, 1]], 8: [[0, 1, 1, 1, 1, 1, 1, 1], [1, 1, 0, 1, 0, 1, 1, 0]]}
REAL_SMALL = {"NV%d_C%d" % (NV, C): (NV, C, torch.tensor(REAL_MASKS[NV], dtype=torch.uint8)) for NV in (2, 4, 7, 8) for C in (8, 32)}


def _many_mask(NV):
    m = torch.ones(2, NV, dtype=torch.uint8)
    m[0, 0] = m[0, NV // 2] = 0
    m[1, :8] = 0                      # the first group of 8 views has no valid view
    m[1, NV - 1] = 0 if NV > 9 else 1
    return m


REAL_MANY = {"NV%d_C%d" % (NV, C): (NV, C, _many_mask(NV)) for NV, C in ((9, 8), (17, 32), (32, 8))}
ALL_ONES = ((2, 8), (4, 32), (7, 8), (8, 32), (9, 8), (17, 8), (32, 32))          # (NV, C) on realistic geometry: every K1 form and both finalizers

_MADE = {}


def make(table, cid):
    """The case's host tensors (with NaN in the masked views where the case says so), made once and never written to."""
    key = (id(table), cid)
    if key not in _MADE:
        spec = table[cid]
        c = spec["make"]()
        _MADE[key] = with_nan(c, spec["mask"]) if spec["nan"] else c
    return _MADE[key]


_LREF = {}


def lattice_reference(cid, case, mask, agg, conf_terms=None):
    """The fp32 words a correct masked kernel writes on a lattice case: per sample unproject_bwd_ref.lattice_reference (which asserts the exactness
    condition, exact.assert_exact) on the compacted valid views, zeros for the masked ones.  -> (grad_feats (B,NV,C,h,w) fp32, grad_conf or None)."""
    key = (cid, agg)
    if key not in _LREF:
        B, NV, C, h, w = case.hm.shape
        gf = torch.zeros(B, NV, C, h, w, dtype=torch.float32)
        gc = torch.zeros(B, NV, C, dtype=torch.float32) if agg.startswith("conf") else None
        for b in range(B):
            idx = valid_views(mask, b)
            f, c, _ = R.lattice_reference("%s[sample %d]" % (cid, b), _sub(case, b, idx), agg, conf_terms)
            gf[b, idx] = f[0]
            if gc is not None:
                gc[b, idx] = c[0]
        _LREF[key] = (gf, gc)
    return _LREF[key]
