"""TEST INFRASTRUCTURE for the unprojection forward (csrc/unproject.hip): importable without a GPU.

* unproject_plan(): unproject_dispatch() restated -- which kernel and which chunk layout a call gets.  Every GPU case asserts from it
  that the branch its id names is really entered before it compares numbers.
* brick_of() / chunk_voxels(): the (workgroup, lane) -> voxel maps of both brick orders and of the linear 256-voxel chunks.
* ref_samples() / aggregate() / ref_unproject(): the operation in fp64 torch, written out without grid_sample, with a class per voxel and view.
* probe_cameras() / probe_points(): points built to land on every zero-padding class in every view.
"""
import itertools
import os
from collections import namedtuple

import numpy as np
import torch

AGGS = ("sum", "max", "softmax", "conf", "conf_norm")
CLASSES = ("interior", "west", "east", "north", "south", "nw", "ne", "sw", "se", "outside", "z<0", "z==0")
CLS = {n: i for i, n in enumerate(CLASSES)}


def _cdiv(a, b):
    return -(-a // b)


def _env_on(env, name):
    """env_on() of csrc/lt_common.h: set, not empty and not exactly "0"."""
    e = env.get(name)
    return bool(e) and e != "0"


def unproject_plan(dtype, B, NV, C, h, w, v0, v1, v2, agg, env=None):
    """unproject_dispatch() and the entry points' size guards.  dtype: torch.float32 | torch.bfloat16; agg: one of AGGS; env: the mapping the A/B
    switches are read from (os.environ when None)."""
    env = os.environ if env is None else env
    bf16 = dtype == torch.bfloat16
    assert bf16 or dtype == torch.float32, dtype
    nvox = v0 * v1 * v2
    bricked = v0 % 4 == 0 and v1 % 4 == 0 and v2 % 16 == 0
    blocked = bricked and v0 % 32 == 0 and v1 % 32 == 0 and v2 % 32 == 0 and not _env_on(env, "LT_UNPROJ_RASTER")
    chunks = _cdiv(nvox, 256)
    supported = NV * h * w * C < (1 << 31) and B * chunks < (1 << 31)
    quad = (bf16 and C == 32 and NV in (4, 8) and bricked and agg == "softmax" and not _env_on(env, "LT_UNPROJ_NO_Q4")
            and NV * h * w * C < (1 << 30))
    if bf16:
        ch = 8 if C % 8 == 0 else 1
    else:
        ch = 4 if C % 4 == 0 else 1
    return dict(supported=supported, bricked=bricked, blocked=blocked, chunks=chunks, xcd_pin=B % 8 == 0, quad=quad,
                kernel="quad" if quad else "generic", ch=None if quad else ch, small_nv=None if quad else NV <= 8,
                nvl=NV // 4 if quad else None, v=(v0, v1, v2), B=B)


def sample_of_block(plan, block):
    """(sample, chunk) of workgroup ``block``: the head of both kernels."""
    if plan["xcd_pin"]:
        xcd, j = block & 7, block >> 3
        return xcd + 8 * (j // plan["chunks"]), j % plan["chunks"]
    return block // plan["chunks"], block % plan["chunks"]


def brick_of(plan, chunk):
    """Origin (bi, bj, bk) of the 4 x 4 x 16 brick of chunk ``chunk`` of a bricked volume, in the plan's order."""
    assert plan["bricked"]
    v0, v1, v2 = plan["v"]
    nk, nj = v2 >> 4, v1 >> 2
    if plan["blocked"]:
        g, l = chunk >> 7, chunk & 127
        ngk, ngj = nk >> 1, nj >> 3
        gk, gj, gi = g % ngk, (g // ngk) % ngj, g // (ngk * ngj)
        return (gi * 8 + (l >> 4)) << 2, (gj * 8 + ((l >> 1) & 7)) << 2, (gk * 2 + (l & 1)) << 4
    return (chunk // (nk * nj)) << 2, ((chunk // nk) % nj) << 2, (chunk % nk) << 4


def chunk_voxels(plan):
    """(chunks, 256) int64: the linear voxel index of lane-slot vb of every chunk; -1 where a linear chunk runs past the volume."""
    v0, v1, v2 = plan["v"]
    nvox = v0 * v1 * v2
    out = np.full((plan["chunks"], 256), -1, dtype=np.int64)
    vb = np.arange(256)
    for c in range(plan["chunks"]):
        if plan["bricked"]:
            bi, bj, bk = brick_of(plan, c)
            out[c] = ((bi + (vb >> 6)) * v1 + bj + ((vb >> 4) & 3)) * v2 + bk + (vb & 15)
        else:
            vox = c * 256 + vb
            out[c] = np.where(vox < nvox, vox, -1)
    return out


# ---- the operation in fp64 ---------------------------------------------------------------------------------------------------------------
Samples = namedtuple("Samples", "vals cls ix iy z")     # vals (B,NV,N,C) fp64; cls (B,NV,N) int64; ix, iy, z (B,NV,N) fp64 (z before the 0 -> 1 patch)


def _axis_class(p, n):
    """0 interior (0 <= p <= n-1), 1 low border cell (-1 < p < 0), 2 high border cell (n-1 < p < n), 3 outside."""
    c = torch.full(p.shape, 3, dtype=torch.int64)
    c[(p >= 0) & (p <= n - 1)] = 0
    c[(p > -1) & (p < 0)] = 1
    c[(p > n - 1) & (p < n)] = 2
    return c


_XY_CLASS = torch.tensor([[CLS["interior"], CLS["west"], CLS["east"], CLS["outside"]],       # [y class][x class]
                          [CLS["north"], CLS["nw"], CLS["ne"], CLS["outside"]],
                          [CLS["south"], CLS["sw"], CLS["se"], CLS["outside"]],
                          [CLS["outside"]] * 4])


def ref_samples(hm, proj, coords):
    """hm (B,NV,C,h,w), proj (B,NV,3,4), coords (B,...,3) -> the per-view bilinear samples, fp64, inputs promoted as they are.
    op.py:113-141 of the reference: [X,1] P^T; invalid = z <= 0; z == 0 -> 1; x normalised by h and y by w; align_corners=True pixel =
    (g + 1) / 2 * (size - 1); four taps, a tap outside the map counts zero; the sample of an invalid point is zero."""
    hm, proj = hm.double(), proj.double()
    B, NV, C, h, w = hm.shape
    X = coords.double().reshape(B, -1, 3)
    N = X.shape[1]
    vals = torch.zeros(B, NV, N, C, dtype=torch.float64)
    cls = torch.zeros(B, NV, N, dtype=torch.int64)
    ixs, iys, zs = (torch.zeros(B, NV, N, dtype=torch.float64) for _ in range(3))
    Xh = torch.cat([X, torch.ones(B, N, 1, dtype=torch.float64)], dim=2)
    for b in range(B):
        for v in range(NV):
            p = Xh[b] @ proj[b, v].t()
            z0 = p[:, 2]
            invalid = z0 <= 0.0
            z = torch.where(z0 == 0.0, torch.ones_like(z0), z0)
            gx = 2 * (p[:, 0] / z / h - 0.5)
            gy = 2 * (p[:, 1] / z / w - 0.5)
            ix = (gx + 1) / 2 * (w - 1)
            iy = (gy + 1) / 2 * (h - 1)
            x0, y0 = torch.floor(ix), torch.floor(iy)
            fx, fy = ix - x0, iy - y0
            fm = hm[b, v].permute(1, 2, 0)                   # h, w, C
            s = torch.zeros(N, C, dtype=torch.float64)
            for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
                xt, yt = x0 + dx, y0 + dy
                ok = (xt >= 0) & (xt <= w - 1) & (yt >= 0) & (yt <= h - 1)
                wt = (fx if dx else 1 - fx) * (fy if dy else 1 - fy)
                wt = torch.where(ok, wt, torch.zeros_like(wt))
                xi, yi = xt.clamp(0, w - 1).long(), yt.clamp(0, h - 1).long()
                s = s + fm[yi, xi] * wt[:, None]
            s[invalid] = 0.0
            c = _XY_CLASS[_axis_class(iy, h), _axis_class(ix, w)]
            c[z0 < 0] = CLS["z<0"]
            c[z0 == 0] = CLS["z==0"]
            vals[b, v], cls[b, v], ixs[b, v], iys[b, v], zs[b, v] = s, c, ix, iy, z0
    return Samples(vals, cls, ixs, iys, zs)


def aggregate(vals, agg, conf=None, mask=None):
    """vals (B,NV,N,C) fp64 -> (B,N,C): the five aggregations over the valid views of every sample (all of them without a mask; none: zeros).
    conf (B,NV,C): 'conf' takes it as it is, 'conf_norm' divides it by its sum over the valid views first (the kernel gets the raw head output)."""
    B, NV, N, C = vals.shape
    out = torch.zeros(B, N, C, dtype=torch.float64)
    for b in range(B):
        idx = torch.arange(NV) if mask is None else torch.nonzero(torch.as_tensor(mask)[b]).flatten()
        if idx.numel() == 0:
            continue
        x = vals[b, idx]
        if agg == "sum":
            out[b] = x.sum(0)
        elif agg == "max":
            out[b] = x.max(0)[0]
        elif agg == "softmax":
            out[b] = (x * torch.softmax(x, dim=0)).sum(0)
        elif agg in ("conf", "conf_norm"):
            c = conf[b, idx].double()
            if agg == "conf_norm":
                c = c / c.sum(0, keepdim=True)
            out[b] = (x * c[:, None, :]).sum(0)
        else:
            raise ValueError(agg)
    return out


def ref_unproject(hm, proj, coords, agg, conf=None, mask=None):
    """-> (out, samples): out in the kernels' layout, coords.shape[:-1] + (C,), fp64."""
    s = ref_samples(hm, proj, coords)
    out = aggregate(s.vals, agg, conf, mask)
    return out.reshape(tuple(coords.shape[:-1]) + (hm.shape[2],)), s


# ---- probe: points that land on every padding class of every view ------------------------------------------------------------------------
FLAT_F, FLAT_C = 32.0, 8.0          # the flat view: P = [[f,0,c,0],[0,f,c,0],[0,0,1,0]], powers of two: pz = X2 exactly, in fp32 and in fp64


def probe_cameras(NV, h, w, flat):
    """fp64 (NV,3,4): ring cameras at map resolution, view ``flat`` replaced by the flat view."""
    from oracle import synth
    from oracle import vol_oracle as O
    K, R, t = synth.ring_cameras(NV, 96)
    P = O.resized_projection(K, R, t, (96, 96), (h, w))
    P[flat] = np.array([[FLAT_F, 0, FLAT_C, 0], [0, FLAT_F, FLAT_C, 0], [0, 0, 1, 0]], dtype=np.float64)
    return P


def is_flat(P):
    return bool(np.all(P[2] == np.array([0.0, 0.0, 1.0, 0.0])))


def probe_table(h, w):
    xs = [-1.5, -1.0, -0.5, 0.0, 0.5, w - 1.5, w - 1.0, w - 0.5, w + 0.5]
    ys = [-1.5, -1.0, -0.5, 0.0, 0.5, h - 1.5, h - 1.0, h - 0.5, h + 0.5]
    return list(itertools.product(xs, ys, (3500.0, -3500.0)))


Probe = namedtuple("Probe", "X view kind ix iy depth")      # X (n,3) fp32; per point: target view, kind 0 table / 1 tiny depth / 2 pz == 0, the row aimed at
TABLE, TINY, ZERO = 0, 1, 2


def probe_rows(P, h, w):
    """The rows (kind, ix, iy, depth) that one view is probed with: the 162 of the table; 8 at depth 1e-4 whose (ix, iy) are px, py themselves, about
    +-1000 (u, v ~ 1e7: huge and finite.  In a ring view the fp32 depth of such a point is cancellation noise of either sign: zero by the depth test or
    zero by the padding, the value does not depend on which); and -- in a flat view, where it can be exact -- 16 with pz == 0 whose px, py would sample
    the middle of the map if the depth test let them through."""
    rows = [(TABLE, ix, iy, d) for ix, iy, d in probe_table(h, w)]
    rows += [(TINY, sx * (1000.0 + 100 * k), sy * (700.0 + 50 * k), 1e-4) for k in range(2) for sx in (1, -1) for sy in (1, -1)]
    if is_flat(P):
        rows += [(ZERO, 2.25 + k, 3.5 + 0.75 * k, 0.0) for k in range(16)]
    return rows


def probe_points(P64, h, w, n):
    """Point i aims at view i % NV, row (i // NV) % len(rows of that view): X = M^-1 (d [u, v, 1] - p4) with u = ix h / (w - 1), v = iy w / (h - 1),
    solved in fp64 and rounded to fp32.  A pz == 0 row is (u, v, 0) / f in the flat view: X2 = 0 exactly, pz' = 1 would give the pixel (ix, iy)."""
    NV = P64.shape[0]
    rows = [probe_rows(P64[v], h, w) for v in range(NV)]
    X = np.zeros((n, 3))
    meta = np.zeros((n, 5))
    for i in range(n):
        v = i % NV
        kind, ix, iy, d = rows[v][(i // NV) % len(rows[v])]
        u, vv = ix * h / (w - 1), iy * w / (h - 1)
        if kind == ZERO:
            X[i] = (u / FLAT_F, vv / FLAT_F, 0.0)
        elif kind == TINY:
            X[i] = np.linalg.solve(P64[v][:, :3], np.array([ix, iy, d]) - P64[v][:, 3])
        else:
            X[i] = np.linalg.solve(P64[v][:, :3], d * np.array([u, vv, 1.0]) - P64[v][:, 3])
        meta[i] = (v, kind, ix, iy, d)
    return Probe(torch.from_numpy(X).float(), meta[:, 0].astype(np.int64), meta[:, 1].astype(np.int64), meta[:, 2], meta[:, 3], meta[:, 4])


def probe_size(P64, h, w, times=8):
    """The smallest 4 x 4 x 16k point count that walks every view's rows ``times`` times."""
    NV = P64.shape[0]
    need = times * NV * max(len(probe_rows(P64[v], h, w)) for v in range(NV))
    return _cdiv(need, 256) * 256


# ---- the shapes of tests/test_gpu_unproject_kernels.py (here so that the CPU file can check the maps and the coverage of the same tables) -----------
VOLUMES = {"7x7x7": (7, 7, 7), "1x1x300": (1, 1, 300), "4x8x32": (4, 8, 32), "8x4x16": (8, 4, 16), "16^3": (16, 16, 16), "12^3": (12, 12, 12),
           "64x64x96": (64, 64, 96), "32x64x96": (32, 64, 96)}
GENERIC_TC = (("fp32", 32), ("fp32", 5), ("bf16", 32), ("bf16", 16), ("bf16", 12), ("bf16", 5))      # ChVec<float,4>, <float,1>, <bf16,8>, <bf16,8>, <bf16,1>, <bf16,1>
GENERIC_NV = (1, 3, 8, 9, 12)
_GV, _GHW, _GB = ("7x7x7", "1x1x300", "4x8x32", "8x4x16"), ((20, 28), (28, 20)), (1, 3, 8, 16)


def generic_cases():
    """Every (type, C) with every NV; volume, map shape and batch walk their lists at different strides, so that every pair of values of two
    different factors occurs (test_unproject_ref_cpu.py checks that); B = 16 at 7^3 and at 4x8x32, in both types, is added by name."""
    cases = {}
    for i, (ty, C) in enumerate(GENERIC_TC):
        for j, NV in enumerate(GENERIC_NV):
            n = i * len(GENERIC_NV) + j
            vol, hw, B = _GV[(i + j) % 4], _GHW[(n // 2 + i) % 2], _GB[(n + n // 4) % 4]
            cases["%s_C%d_NV%d_%s_%dx%d_B%d" % (ty, C, NV, vol, hw[0], hw[1], B)] = dict(ty=ty, C=C, NV=NV, vol=vol, hw=hw, B=B)
    extra = (("pin2", "fp32", 32, 9, "7x7x7", (20, 28), 16), ("pin2", "fp32", 5, 3, "4x8x32", (28, 20), 16), ("pin2", "bf16", 32, 3, "7x7x7", (28, 20), 16),
             ("pin2", "bf16", 12, 9, "4x8x32", (20, 28), 16),
             # the pairs (type and C, B) and (NV, B) that the walk above leaves out
             ("pair", "fp32", 5, 9, "8x4x16", (20, 28), 3), ("pair", "bf16", 5, 8, "1x1x300", (28, 20), 8), ("pair", "bf16", 32, 12, "8x4x16", (20, 28), 8))
    for tag, ty, C, NV, vol, hw, B in extra:
        cases["%s_%s_C%d_NV%d_%s_%dx%d_B%d" % (tag, ty, C, NV, vol, hw[0], hw[1], B)] = dict(ty=ty, C=C, NV=NV, vol=vol, hw=hw, B=B)
    return cases


def box_coords(base, side, vs, theta):
    """(v0,v1,v2,3) fp32: the middle v0 x v1 x v2 voxels of the rotated max(vs)^3 cuboid grid of the model (a non-cubic grid around the same centre)."""
    from oracle import vol_oracle as O
    V = max(max(vs), 2)
    o = [(V - v) // 2 for v in vs]
    return O.coord_volume(base, side, V, theta)[o[0]:o[0] + vs[0], o[1]:o[1] + vs[1], o[2]:o[2] + vs[2]].contiguous()
