"""TEST INFRASTRUCTURE for the unprojection backward (csrc/unproject_bwd.hip): importable without a GPU.

* ref_backward(): the backward WRITTEN OUT -- per view the four tap pixels and weights by the forward's rules (tests/unproject_ref.py), d out / d x_v of
  the five aggregations, index_add of weight * dx into the maps -- in fp64, or in fp32 as the kernels state it (the confidence gradient is then summed in
  fp64, as K1's partials and the finalizers do).  It also returns a cancellation-free magnitude per element, the yardstick of the toleranced gates.
* lattice_case(): inputs on a dyadic lattice.  Flat views P = s [[ax,0,h ox,0],[0,ay,w oy,0],[0,0,1,0]] (s = +-1 flips the depth sign of a view) and points
  X = (h qx z, w qy z, z) give u / h = ax qx + ox without rounding, so the pixel ix = (ax qx + ox)(w - 1), the four weights, the samples of integer maps,
  dx and every partial sum of weight * dx are exact in fp32 IN ANY ORDER: gather, scatter and reference must agree bit for bit for sum / max / conf (and
  conf_norm where the confidences are powers of two with a power-of-two sum).  lattice_reference() asserts that condition (exact.assert_exact) for
  every case before anything is launched.
* builders of structured point sets (seams, pile, alternate, many bricks on one tile with empty bricks in between, an empty view) and round_stats(), the
  gather's walk restated -- (tile, brick, lane) order, half-wave split, rounds of four hit records, parity slots -- which counts what the sets claim.
* bwd_plan(): the host dispatch of lt_unproject_bwd restated; every GPU case asserts from it that it enters the branch its id names.
* EXACT / TOLERANCED / REALISTIC: the case tables of tests/test_gpu_unproject_bwd_kernels.py, here so that tests/test_unproject_bwd_ref_cpu.py can hold
  every case to the conditions its gate rests on."""
import os
from collections import Counter, namedtuple

import numpy as np
import torch

import exact
import unproject_ref as U

AGGS = U.AGGS
EXACT_AGGS = ("sum", "max", "conf")
UB_MAXV, UB_MANYV = 8, 32
G_TW = G_TH = 16
G_LIST = 256


def _cdiv(a, b):
    return -(-a // b)


def _a256(v):
    return (v + 255) // 256 * 256


# ---- the host dispatch ---------------------------------------------------------------------------------------------------------------------------
def bwd_plan(dtype, B, NV, C, h, w, v, agg, env=None, ws_samples=None, has_conf=None):
    """lt_unproject_bwd's argument checks and dispatch.  v = (v0, v1, v2); env: the mapping LT_UNPROJ_BWD_ATOMICS is read from (os.environ when None);
    ws_samples: the workspace handed over, in samples' shares (None: the whole batch's); has_conf: whether confidences are passed (None: exactly for the
    conf aggregations).  -> dict; ``refused`` is None or (return code, a word of the message)."""
    env = os.environ if env is None else env
    assert dtype in (torch.float32, torch.bfloat16), dtype
    v0, v1, v2 = v
    is_conf = agg in ("conf", "conf_norm")
    has_conf = is_conf if has_conf is None else has_conf
    p = dict(refused=None, path=None, agg=agg)
    if agg not in AGGS:
        p["refused"] = (-2, "unknown aggregation")
    elif is_conf and not has_conf:
        p["refused"] = (-1, "need confidences")
    elif not (B >= 1 and 1 <= NV <= UB_MANYV and C >= 4 and C % 4 == 0 and h >= 2 and w >= 2 and v0 >= 1 and v1 >= 1 and v2 >= 1):
        p["refused"] = (-2, "NV <= %d" % UB_MANYV)
    elif NV * h * w * C >= 1 << 31:
        p["refused"] = (-2, "feature maps too large")
    if p["refused"]:
        return p
    nvox = v0 * v1 * v2
    items = nvox * (C // 4)
    gather = 4 <= C <= 64 and C & (C - 1) == 0 and not U._env_on(env, "LT_UNPROJ_BWD_ATOMICS")
    p.update(nvox=nvox, items=items, many=NV > UB_MAXV)
    if not gather:
        if agg == "conf_norm":
            p["refused"] = (-2, "conf_norm needs the gather path")
            return p
        p.update(path="scatter", kernel="scatter_many" if NV > UB_MAXV else "scatter", grid=min(65536, _cdiv(items, 256)), per_sample=0)
        return p
    nbricks = _cdiv(v0, 4) * _cdiv(v1, 4) * _cdiv(v2, 4)
    nblk1 = min(2048, _cdiv(items, 256))
    per_sample = (_a256(NV * nvox * C * 4) + _a256(NV * nbricks * 16) + _a256(nblk1 * NV * C * 8) + _a256(NV * nvox * 4) + _a256(NV * nvox * 16))
    ws = per_sample * (B if ws_samples is None else ws_samples)
    p.update(path="gather", per_sample=per_sample, workspace=ws, nbricks=nbricks, nblk1=nblk1)
    if ws < per_sample:
        p["refused"] = (-1, "workspace of at least %d bytes" % per_sample)
        return p
    chunk = min(ws // per_sample, B)
    if NV > UB_MAXV:
        k1 = "passes" if agg in ("softmax", "max") else "groups"
    else:
        k1 = "mv4" if NV <= 4 else "mv8"
    p.update(chunk=chunk, nchunks=_cdiv(B, chunk), tiles=_cdiv(w, G_TW) * _cdiv(h, G_TH), CW=C // 4, HALVES=2 if C <= 32 else 1, k1=k1,
             groups=_cdiv(NV, UB_MAXV) if k1 == "groups" else None, finalizer=None if not is_conf else ("many" if NV > UB_MAXV else "small"),
             k1_strided=items > nblk1 * 256, k1_items_per_lane=_cdiv(items, nblk1 * 256))
    return p


def plan_is(plan, **expect):
    assert plan["refused"] is None, plan
    for k, val in expect.items():
        assert plan[k] == val, "the case does not enter the branch its id names: %s is %r, not %r" % (k, plan[k], val)


# ---- the operation -------------------------------------------------------------------------------------------------------------------------------
Taps = namedtuple("Taps", "x0 y0 wt idx invalid z ix iy")      # per (B,NV,N): origin of the 2x2 patch (floor, unclamped), weights (..,4; 0 = padding or
#                                                                depth <= 0), clamped pixel index y w + x (..,4), depth <= 0, depth, pixel position
Rec = namedtuple("Rec", "taps vals dx winner")                 # vals, dx (B,NV,N,C); winner (B,N,C) for 'max', else None
Mag = namedtuple("Mag", "feats conf")


def ref_taps(proj, coords, h, w, dtype=torch.float64):
    """unproject_ref.ref_samples' geometry (op.py:113-141 of the reference), every view at once, in ``dtype``."""
    P = proj.to(dtype)
    B, NV = P.shape[:2]
    X = coords.to(dtype).reshape(B, -1, 3)
    N = X.shape[1]
    Xh = torch.cat([X, torch.ones(B, N, 1, dtype=dtype)], dim=2)
    p = Xh[:, None] @ P.transpose(-1, -2)                                  # B, NV, N, 3
    z0 = p[..., 2]
    invalid = z0 <= 0
    z = torch.where(z0 == 0, torch.ones_like(z0), z0)
    gx = 2 * (p[..., 0] / z / h - 0.5)
    gy = 2 * (p[..., 1] / z / w - 0.5)
    ix = (gx + 1) / 2 * (w - 1)
    iy = (gy + 1) / 2 * (h - 1)
    x0, y0 = torch.floor(ix), torch.floor(iy)
    fx, fy = ix - x0, iy - y0
    wt, idx = [], []
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        xt, yt = x0 + dx, y0 + dy
        ok = (xt >= 0) & (xt <= w - 1) & (yt >= 0) & (yt <= h - 1) & ~invalid
        k = (fx if dx else 1 - fx) * (fy if dy else 1 - fy)
        wt.append(torch.where(ok, k, torch.zeros_like(k)))
        idx.append(yt.clamp(0, h - 1).long() * w + xt.clamp(0, w - 1).long())
    big = float(1 << 40)
    return Taps(x0.clamp(-big, big).long(), y0.clamp(-big, big).long(), torch.stack(wt, -1), torch.stack(idx, -1), invalid, z0, ix, iy)


def first_max(x):
    """x (NV, ...) -> the LOWEST view index among the maxima, written as the kernels' scan: a later view wins only where it is strictly greater."""
    best, am = x[0].clone(), torch.zeros(x.shape[1:], dtype=torch.int64)
    for v in range(1, x.shape[0]):
        up = x[v] > best
        best = torch.where(up, x[v], best)
        am = torch.where(up, torch.full_like(am, v), am)
    return am


def ref_backward(hm, proj, coords, G, agg, conf=None, dtype=torch.float64):
    """hm (B,NV,C,h,w), proj (B,NV,3,4), coords (B,v0,v1,v2,3), G (B,C,v0,v1,v2) = dL/d volume, conf (B,NV,C)
    -> (grad_feats (B,NV,C,h,w), grad_conf (B,NV,C) or None, Mag, Rec), in ``dtype``.

    Rules of the forward: depth <= 0 zeroes the sample (all four weights 0: nothing flows back, but the 0 takes part in max / softmax); z == 0 -> 1;
    a tap outside the map counts zero.  max: the whole gradient to the lowest view index among the maxima.  softmax: g p_v (1 + x_v - out).  conf: g c_v,
    d/dc_v = sum_n g x_v.  conf_norm: n_v = c_v / S, S = sum_u c_u; g n_v; with s_v = sum_n g x_v: d/dc_v = (s_v - sum_u s_u n_u) / S.  The sums over the
    voxels and the conf_norm chain rule run in fp64 whatever ``dtype`` is (the kernels: fp32 products, fp64 partials and finalizer); grad_conf is then
    rounded to ``dtype``.
    Mag.feats: the same scatter of weight * |dx| -- for softmax of weight * |g| p_v (1 + |x_v| + |out|), because 1 + x_v - out cancels --; Mag.conf:
    sum_n |g x_v| (conf), (that + sum_u n_u sum_n |g x_u|) / S (conf_norm)."""
    B, NV, C, h, w = hm.shape
    dt = dtype
    T = ref_taps(proj, coords, h, w, dt)
    N = T.wt.shape[2]
    g_all = G.to(dt).reshape(B, C, N).permute(0, 2, 1)
    gf = torch.zeros(B, NV, h * w, C, dtype=dt)
    mg = torch.zeros(B, NV, h * w, C, dtype=dt)
    vals = torch.zeros(B, NV, N, C, dtype=dt)
    dxs = torch.zeros(B, NV, N, C, dtype=dt)
    is_conf = agg in ("conf", "conf_norm")
    gc = torch.zeros(B, NV, C, dtype=torch.float64) if is_conf else None
    mc = torch.zeros(B, NV, C, dtype=torch.float64) if is_conf else None
    winner = torch.zeros(B, N, C, dtype=torch.int64) if agg == "max" else None
    for b in range(B):
        fm = hm[b].to(dt).permute(0, 2, 3, 1).reshape(NV, h * w, C)
        g = g_all[b]
        x = vals[b]
        for v in range(NV):
            k, i = T.wt[b, v], T.idx[b, v]
            x[v] = fm[v][i[:, 0]] * k[:, 0, None] + fm[v][i[:, 1]] * k[:, 1, None] + fm[v][i[:, 2]] * k[:, 2, None] + fm[v][i[:, 3]] * k[:, 3, None]
        if agg == "sum":
            dx = g[None].expand(NV, N, C)
            mdx = dx.abs()
        elif agg == "max":
            am = first_max(x)
            winner[b] = am
            dx = torch.stack([torch.where(am == v, g, torch.zeros_like(g)) for v in range(NV)])
            mdx = dx.abs()
        elif agg == "softmax":
            m = x.max(0)[0]
            ex = torch.exp(x - m)
            s = ex.sum(0)
            out = (x * ex).sum(0) / s
            p = ex / s
            dx = g * p * (1 + x - out)
            mdx = g.abs() * p * (1 + x.abs() + out.abs())
        elif is_conf:
            c = conf[b].to(dt)
            n = c / c.sum(0, keepdim=True) if agg == "conf_norm" else c
            dx = g[None] * n[:, None, :]
            mdx = dx.abs()
            s = (g[None] * x).double().sum(1)                                # NV, C
            ms = (g[None] * x).abs().double().sum(1)
            if agg == "conf_norm":
                c64 = conf[b].double()
                S = c64.sum(0)
                gc[b] = (s - (s * c64 / S).sum(0)) / S
                mc[b] = (ms + (ms * c64 / S).sum(0)) / S
            else:
                gc[b], mc[b] = s, ms
        else:
            raise ValueError(agg)
        dxs[b] = dx
        for v in range(NV):
            for t in range(4):
                gf[b, v].index_add_(0, T.idx[b, v, :, t], T.wt[b, v, :, t, None] * dx[v])
                mg[b, v].index_add_(0, T.idx[b, v, :, t], T.wt[b, v, :, t, None] * mdx[v])

    def maps(t):
        return t.reshape(B, NV, h, w, C).permute(0, 1, 4, 2, 3)
    return maps(gf), (gc.to(dt) if is_conf else None), Mag(maps(mg), mc), Rec(T, vals, dxs, winner)


# ---- the lattice -----------------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "hm P cv conf G h w vs q z tables")
# per view (cycled): ax, ox, ay, oy, depth sign.  ax q + ox with q in [-1/4, 5/4]: view 0 is the identity (a builder's q IS the pixel / (size - 1)),
# the others shift, shrink and stretch it, so that about half of all taps fall into the map; view 2 looks the other way (valid where z < 0)
TABLES = ((1.0, 0.0, 1.0, 0.0, 1), (0.5, 0.25, 1.0, -0.125, 1), (1.0, -0.125, 0.5, 0.375, -1), (2.0, -0.5, 1.0, 0.125, 1),
          (1.0, 0.125, 2.0, -0.75, 1), (0.5, 0.375, 0.5, 0.25, -1), (1.0, -0.25, 1.0, 0.25, 1), (2.0, -1.0, 0.5, 0.125, 1))
ZS, ZP = (1.0, 2.0, -1.0, 0.0), (0.45, 0.27, 0.2, 0.08)
POW2_CONF = {1: (0.5,), 2: (0.25, 0.25), 4: (0.5, 0.25, 0.125, 0.125), 8: (0.25, 0.25, 0.125, 0.125, 0.0625, 0.0625, 0.0625, 0.0625)}


def flat_projection(tab, h, w):
    ax, ox, ay, oy, s = tab
    return s * torch.tensor([[ax, 0, h * ox, 0], [0, ay, w * oy, 0], [0, 0, 1, 0]], dtype=torch.float64)


def lattice_case(B, NV, C, h, w, vs, seed, qden=16, conf="eighths", q=None, z=None, tables=TABLES, dup=None):
    """Exact inputs.  q (B,N,2) / z (B,N): the point lattice (qx, qy multiples of a power of two, z in ZS) when a builder sets it; otherwise qx, qy uniform
    on the 1/qden lattice of [-1/4, 5/4] and z from ZS with probabilities ZP, other points per sample.  conf: 'eighths' (1/8 .. 1) or 'pow2' (a per-channel
    permutation of POW2_CONF[NV], halved on odd channels: powers of two with a power-of-two sum).  dup: {view: source view} -- the view gets the source's
    projection and maps (exact 'max' ties between them everywhere).  Integer maps in [-3, 3] (bf16 holds them) and integer G in [-4, 4]."""
    g = exact.gen(seed)
    N = vs[0] * vs[1] * vs[2]
    if q is None:
        q = torch.randint(-qden // 4, 5 * qden // 4 + 1, (B, N, 2), generator=g).double() / qden
    if z is None:
        z = torch.tensor(ZS, dtype=torch.float64)[torch.multinomial(torch.tensor(ZP), B * N, replacement=True, generator=g).reshape(B, N)]
    q, z = q.double(), z.double()
    tabs = [tables[v % len(tables)] for v in range(NV)]
    hm = exact.ints((B, NV, C, h, w), 3, g)
    for v, src in (dup or {}).items():
        tabs[v] = tabs[src]
        hm[:, v] = hm[:, src]
    P = torch.stack([flat_projection(t, h, w) for t in tabs])[None].repeat(B, 1, 1, 1).float().contiguous()
    X = torch.stack([h * q[..., 0] * z, w * q[..., 1] * z, z], dim=-1)
    cv = exact.as_f32(X, "lattice point").reshape(B, *vs, 3).contiguous()
    G = exact.ints((B, C) + tuple(vs), 4, g)
    if conf == "pow2":
        base = torch.tensor(POW2_CONF[NV])
        cf = torch.stack([torch.stack([base[torch.randperm(NV, generator=g)] * (0.5 if c % 2 else 1.0) for c in range(C)], dim=1) for _ in range(B)])
    else:
        cf = torch.randint(1, 9, (B, NV, C), generator=g).float() / 8
    return Case(hm, P, cv, cf.contiguous(), G, h, w, tuple(vs), q, z, tabs)


_LREF = {}


def lattice_reference(name, case, agg, conf_terms=None, key=None):
    """fp64 ref_backward of a lattice case as the fp32 words a correct kernel writes, with the exactness condition asserted: the largest per-pixel
    sum of |weight * dx| on the grid of the contributions stays below 2^24, likewise the samples, and the fp32 part of the confidence gradient
    (conf_terms terms of g * x per fp32 sum: K1's per-lane accumulator, or every voxel for the atomic scatter; None: every voxel).
    -> (grad_feats fp32, grad_conf fp32 or None, Rec).  Cached under ``key``."""
    if key is not None and (key, agg) in _LREF:
        return _LREF[(key, agg)]
    gf, gc, mag, rec = ref_backward(case.hm, case.P, case.cv, case.G, agg, case.conf)
    gw, gd = exact.grid_of(rec.taps.wt), exact.grid_of(rec.dx)
    exact.assert_exact("%s/%s: per-pixel sum of |w dx|" % (name, agg), float(mag.feats.max()), gw * gd)
    exact.assert_exact("%s/%s: samples" % (name, agg), 4 * 3.0, gw)
    if gc is not None:
        gx = float(case.G.abs().max()) * float(rec.vals.abs().max())
        n = rec.vals.shape[2] if conf_terms is None else conf_terms
        exact.assert_exact("%s/%s: fp32 sums of g x" % (name, agg), min(n * gx, float(mag.conf.max())), exact.grid_of(rec.vals))
    out = (exact.as_f32(gf, name + " grad_feats").contiguous(), None if gc is None else gc.float(), rec)
    if key is not None:
        _LREF[(key, agg)] = out
    return out


# ---- the gather's walk ---------------------------------------------------------------------------------------------------------------------------------
def brick_lanes(vs):
    """(nbricks, 64) int64: brick_voxel() -- the voxel of (brick, lane) for 4 x 4 x 4 bricks in raster order, -1 past the grid's end."""
    v0, v1, v2 = vs
    nb0, nb1, nb2 = _cdiv(v0, 4), _cdiv(v1, 4), _cdiv(v2, 4)
    br = np.arange(nb0 * nb1 * nb2)[:, None]
    lane = np.arange(64)[None, :]
    i = (br // (nb2 * nb1)) * 4 + (lane >> 4)
    j = ((br // nb2) % nb1) * 4 + ((lane >> 2) & 3)
    k = (br % nb2) * 4 + (lane & 3)
    return np.where((i < v0) & (j < v1) & (k < v2), (i * v1 + j) * v2 + k, -1)


def round_stats(taps, b, v, vs, h, w, halves):
    """The walk of unproj_gather_kernel over view v of sample b, from the reference's tap records: per tile the candidate bricks (bounding box of the
    weighted taps meets the tile), per candidate brick and half the voxels with a weighted tap inside, in lane order, in rounds of four; per round and
    parity slot the cells.  -> dict: multi[m] rounds x slots where the most frequent cell occurs m = 2, 3, 4 times; alt: off[2] == off[0] != off[1];
    cand: candidate bricks per tile; empty: the bricks without a weighted tap; straddle_half / straddle_tile_x / straddle_tile_y: four-weight patches
    whose two columns lie on both sides of column 8 of a tile / in two tiles."""
    wt = taps.wt[b, v].numpy()
    x0, y0 = taps.x0[b, v].numpy(), taps.y0[b, v].numpy()
    live = wt != 0
    px = x0[:, None] + np.array([0, 1, 0, 1])
    py = y0[:, None] + np.array([0, 0, 1, 1])
    BL = brick_lanes(vs)
    st = dict(multi={2: 0, 3: 0, 4: 0}, alt=0, cand={}, empty=[], rounds=0, hits=0)
    four = live.all(1)
    st["straddle_half"] = int((four & (x0 % 16 == 7)).sum())
    st["straddle_tile_x"] = int((four & (x0 % 16 == 15)).sum())
    st["straddle_tile_y"] = int((four & (y0 % 16 == 15)).sum())
    boxes = []
    for br in range(BL.shape[0]):
        vox = BL[br][BL[br] >= 0]
        l = live[vox]
        if not l.any():
            boxes.append(None)
            st["empty"].append(br)
        else:
            boxes.append((px[vox][l].min(), px[vox][l].max(), py[vox][l].min(), py[vox][l].max()))
    for ty0 in range(0, h, G_TH):
        for tx0 in range(0, w, G_TW):
            cand = [br for br, bb in enumerate(boxes) if bb is not None and bb[1] >= tx0 and bb[0] < tx0 + G_TW and bb[3] >= ty0 and bb[2] < ty0 + G_TH]
            st["cand"][(tx0, ty0)] = len(cand)
            for br in cand:
                for hh in range(halves):
                    recs = []
                    for vx in BL[br]:
                        if vx < 0:
                            continue
                        cells = [-1, -1, -1, -1]
                        for t in range(4):
                            lx, ly = px[vx, t] - tx0, py[vx, t] - ty0
                            if live[vx, t] and 0 <= lx < G_TW and 0 <= ly < G_TH and (lx >> 3 if halves == 2 else 0) == hh:
                                cells[(px[vx, t] & 1) + 2 * (py[vx, t] & 1)] = int(ly * G_TW + lx)
                        if max(cells) >= 0:
                            recs.append(cells)
                    st["hits"] += len(recs)
                    for r0 in range(0, len(recs), 4):
                        rnd = recs[r0:r0 + 4]
                        st["rounds"] += 1
                        for s in range(4):
                            off = [r[s] for r in rnd]
                            cnt = Counter(o for o in off if o >= 0)
                            if cnt and max(cnt.values()) >= 2:
                                st["multi"][max(cnt.values())] += 1
                            if len(off) >= 3 and off[2] >= 0 and off[2] == off[0] and off[1] != off[0]:
                                st["alt"] += 1
    return st


# ---- structured point sets: q (B,N,2), z (B,N) for lattice_case, view 0 being the identity view ------------------------------------------------------------
def _background(B, N, qden, seed):
    g = exact.gen(seed)
    q = torch.randint(0, qden + 1, (B, N, 2), generator=g).double() / qden
    z = torch.tensor(ZS, dtype=torch.float64)[torch.multinomial(torch.tensor(ZP), B * N, replacement=True, generator=g).reshape(B, N)]
    return q, z, g


SEAM_X, SEAM_Y = (7, 15, 16), (15, 16, 31)
SEAM_HW = (33, 17)


def seams_points(vs, seed, B=2):
    """Maps of 33 x 17 (tiles of 16 + 1 columns, 16 + 16 + 1 rows): every origin (x, y) of SEAM_X x SEAM_Y with the fractions 1/4, 1/2, 3/4 on both axes --
    x = 7 puts the patch's columns on both sides of the half-wave split, x = 15 and y = 15, 31 put it into two tiles (the last of them one pixel wide /
    high), x = 16 is the last column, whose east taps are padding -- in front of view 0 (z in {1, 2}); the other points are background.  Sample 1 holds
    the same points in reverse order (other bricks and lanes)."""
    h, w = SEAM_HW
    N = vs[0] * vs[1] * vs[2]
    q, z, g = _background(B, N, 16, seed)
    pts = [((x + fx) / (w - 1), (y + fy) / (h - 1)) for x in SEAM_X for y in SEAM_Y for fx in (0.25, 0.5, 0.75) for fy in (0.25, 0.5, 0.75)]
    assert len(pts) <= N
    where = torch.randperm(N, generator=g)[:len(pts)]
    for b in range(B):
        idx = where if b % 2 == 0 else N - 1 - where
        q[b, idx] = torch.tensor(pts, dtype=torch.float64)
        z[b, idx] = torch.tensor([1.0, 2.0], dtype=torch.float64)[torch.arange(len(pts)) % 2]
    return q, z, dict(per_origin=9, origins=[(x, y) for x in SEAM_X for y in SEAM_Y])


ROUND_HW, ROUND_VS = (17, 17), (4, 4, 8)
# per row of four lanes (k = 0..3 of one (i, j) of a brick) the pixels of the four voxels, as indices into _ROUND_PIX
_PILE_ROWS = ((0, 0, 0, 0), (1, 1, 1, 2), (3, 2, 2, 2), (4, 4, 5, 6), (5, 6, 6, 4), (7, 7, 7, 7), (0, 1, 1, 1), (2, 2, 3, 3))
_ALT_ROWS = ((0, 2, 0, 2), (1, 3, 1, 5), (4, 6, 4, 0), (7, 5, 7, 5), (2, 0, 2, 4), (3, 1, 3, 1), (6, 4, 6, 2), (5, 7, 5, 3))
_ROUND_PIX = ((2, 3), (5, 1), (1, 6), (4, 4), (6, 2), (3, 5), (0, 0), (5, 5))          # pairwise at least 2 apart on one axis: their patches share no pixel


def round_points(kind, seed, B=2):
    """4 x 4 x 8 voxels = two bricks; maps 17 x 17; every voxel in front of view 0, inside columns 0..7 of tile (0, 0) with four weights, so that every
    lane of a brick is a hit of half 0 and a row of four lanes (k = 0..3) is one round.  'pile': rows whose voxels share the patch origin 4, 3 and 2 at a
    time (fractions differ); 'alternate': rows A B A B / A B A C with disjoint patches A, B, C.  Sample 1 has the rows in another order."""
    rows = _PILE_ROWS if kind == "pile" else _ALT_ROWS
    h, w = ROUND_HW
    g = exact.gen(seed)
    BL = brick_lanes(ROUND_VS)
    N = 128
    q, z = torch.zeros(B, N, 2, dtype=torch.float64), torch.ones(B, N, dtype=torch.float64)
    for b in range(B):
        for br in range(2):
            for r in range(16):
                row = rows[(r + 3 * br + 5 * b) % len(rows)]
                for k in range(4):
                    x, y = _ROUND_PIX[row[k]]
                    fx, fy = (torch.randint(1, 4, (2,), generator=g).double() / 4).tolist()
                    vx = BL[br, r * 4 + k]
                    q[b, vx] = torch.tensor([(x + fx) / (w - 1), (y + fy) / (h - 1)], dtype=torch.float64)
                    z[b, vx] = 1.0 + (r + k) % 2
    return q, z, dict(rounds=32)


REFILL_HW, REFILL_VS = (16, 16), (28, 28, 28)


def refill_points(seed, B=2):
    """28^3 voxels = 343 bricks in front of one 16 x 16 map (one tile): every brick whose index is 2 (sample 0) or 0 (sample 1) modulo 5 lies at z = -1
    (no weighted tap: an empty bounding box), every other brick projects into the map -- more than G_LIST - 64 = 192 candidates on the tile, so that the
    candidate list is filled a second time, with empty bricks between the candidates."""
    N = 28 ** 3
    g = exact.gen(seed)
    q = torch.randint(0, 17, (B, N, 2), generator=g).double() / 16
    z = torch.tensor([1.0, 2.0], dtype=torch.float64)[torch.randint(0, 2, (B, N), generator=g)]
    BL = brick_lanes(REFILL_VS)
    for b in range(B):
        for br in range(BL.shape[0]):
            if br % 5 == (2, 0)[b % 2]:
                z[b, BL[br][BL[br] >= 0]] = -1.0
    return q, z, dict(bricks=343, empty=(69, 69))


def empty_view_z(B, N, seed):
    """Every point in front of view 0 (z in {1, 2}): a view of depth sign -1 sees none of them."""
    g = exact.gen(seed)
    return torch.tensor([1.0, 2.0], dtype=torch.float64)[torch.randint(0, 2, (B, N), generator=g)]


CLASSES_HW, CLASSES_VS = (17, 33), (8, 8, 8)


def classes_points(NV, tables=TABLES):
    """The forward's probe table (unproject_ref.probe_table: -1.5, -1, -0.5, 0, 0.5, size - 1.5, size - 1, size - 0.5, size + 0.5 on both axes, in front of and
    behind the camera) on the lattice: maps of 17 x 33, so that ix = 32 (ax qx + ox) and iy = 16 (ay qy + oy) take every table value exactly.  Point i aims
    at view i % NV; the rest of the 8 x 8 x 8 grid lies at z == 0 (pz == 0 in every view).  One sample, used for both."""
    h, w = CLASSES_HW
    rows = U.probe_table(h, w)
    N = CLASSES_VS[0] * CLASSES_VS[1] * CLASSES_VS[2]
    assert len(rows) * NV <= N - 8
    q, z = torch.zeros(1, N, 2, dtype=torch.float64), torch.zeros(1, N, dtype=torch.float64)
    for i in range(len(rows) * NV):
        v = i % NV
        ix, iy, d = rows[i // NV]
        ax, ox, ay, oy, s = tables[v % len(tables)]
        q[0, i] = torch.tensor([(ix / (w - 1) - ox) / ax, (iy / (h - 1) - oy) / ay], dtype=torch.float64)
        z[0, i] = s * (1.0 if d > 0 else -1.0) * (1 + i % 2)
    return q.repeat(2, 1, 1), z.repeat(2, 1), dict(rows=len(rows))


# ---- the case tables ---------------------------------------------------------------------------------------------------------------------------------------
STD_HW, STD_VS = (20, 37), (5, 6, 7)
F32, BF16 = torch.float32, torch.bfloat16


def _std(C, NV, seed, conf="eighths", dup=None, B=2):
    return lattice_case(B, NV, C, STD_HW[0], STD_HW[1], STD_VS, seed, conf=conf, dup=dup)


def _seams(C, seed):
    q, z, _ = seams_points((4, 6, 9), seed)
    return lattice_case(2, 3, C, SEAM_HW[0], SEAM_HW[1], (4, 6, 9), seed, q=q, z=z)


def _rounds(kind, C, seed):
    q, z, _ = round_points(kind, seed)
    return lattice_case(2, 2, C, ROUND_HW[0], ROUND_HW[1], ROUND_VS, seed, q=q, z=z)


def _refill():
    q, z, _ = refill_points(71)
    return lattice_case(2, 1, 4, REFILL_HW[0], REFILL_HW[1], REFILL_VS, 71, q=q, z=z)


def _empty_view():
    tabs = (TABLES[0], TABLES[1][:4] + (-1,))
    return lattice_case(2, 2, 16, STD_HW[0], STD_HW[1], STD_VS, 72, z=empty_view_z(2, 210, 72), tables=tabs)


def _classes():
    q, z, _ = classes_points(3)
    return lattice_case(2, 3, 8, CLASSES_HW[0], CLASSES_HW[1], CLASSES_VS, 73, q=q, z=z)


def _k1_stride():
    return lattice_case(2, 2, 64, STD_HW[0], STD_HW[1], (36, 32, 32), 74, qden=8)


def _views(NV, seed=80):
    dup = {8: 0} if NV == 9 else ({8: 0, 16: 1, 12: 0} if NV == 17 else None)
    return _std(16, NV, seed + NV, conf="pow2" if NV in POW2_CONF else "eighths", dup=dup)


def _case(make, aggs, dtype=F32, env=None, **plan):
    return dict(make=make, aggs=tuple(aggs), dtype=dtype, env=env or {}, plan=plan)


def _views_aggs(NV):
    return EXACT_AGGS + (("conf_norm",) if NV in POW2_CONF else ())


def _k1_of(NV):
    return "mv4" if NV <= 4 else ("mv8" if NV <= 8 else None)


EXACT = {}
for _i, _C in enumerate((4, 8, 16, 32, 64)):
    EXACT["cw%d" % (_C // 4)] = _case(lambda C=_C: _std(C, 3, 10 + C), EXACT_AGGS, path="gather", CW=_C // 4, HALVES=2 if _C <= 32 else 1, k1="mv4", tiles=6)
    EXACT["cw%d_conf_norm" % (_C // 4)] = _case(lambda C=_C: _std(C, 4, 20 + C, conf="pow2"), ("conf_norm",), path="gather", CW=_C // 4, k1="mv4", finalizer="small")
EXACT["classes"] = _case(_classes, EXACT_AGGS, path="gather", CW=2, k1="mv4")
EXACT["tiny_1x1x1"] = _case(lambda: lattice_case(2, 1, 4, 2, 2, (1, 1, 1), 30, qden=8), EXACT_AGGS, path="gather", CW=1, tiles=1, nbricks=1, nblk1=1)
EXACT["tiny_4x4x4"] = _case(lambda: lattice_case(2, 1, 4, 2, 2, (4, 4, 4), 31, qden=8), EXACT_AGGS, path="gather", CW=1, tiles=1, nbricks=1, nblk1=1)
EXACT["seams_C16"] = _case(lambda: _seams(16, 40), EXACT_AGGS, path="gather", CW=4, HALVES=2, tiles=6)
EXACT["seams_C64"] = _case(lambda: _seams(64, 41), EXACT_AGGS, path="gather", CW=16, HALVES=1, tiles=6)
for _kind in ("pile", "alternate"):
    EXACT[_kind + "_C4"] = _case(lambda k=_kind: _rounds(k, 4, 50), EXACT_AGGS, path="gather", CW=1, HALVES=2, nbricks=2, tiles=4)
    EXACT[_kind + "_C64"] = _case(lambda k=_kind: _rounds(k, 64, 51), EXACT_AGGS, path="gather", CW=16, HALVES=1, nbricks=2, tiles=4)
EXACT["refill"] = _case(_refill, EXACT_AGGS, path="gather", CW=1, tiles=1, nbricks=343)
EXACT["empty_view"] = _case(_empty_view, EXACT_AGGS, path="gather", CW=4, k1="mv4")
EXACT["k1_stride"] = _case(_k1_stride, ("conf",), path="gather", CW=16, k1="mv4", nblk1=2048, k1_strided=True, k1_items_per_lane=2, finalizer="small")
for _C in (8, 32):
    for _NV in (3, 8):
        EXACT["bf16_cw%d_NV%d" % (_C // 4, _NV)] = _case(lambda C=_C, NV=_NV: _std(C, NV, 60 + C + NV, conf="pow2" if NV == 8 else "eighths"), _views_aggs(_NV),
                                                         dtype=BF16, path="gather", CW=_C // 4, k1=_k1_of(_NV))
VIEWS_K1 = {1: ("mv4", "mv4"), 2: ("mv4", "mv4"), 4: ("mv4", "mv4"), 5: ("mv8", "mv8"), 8: ("mv8", "mv8"), 9: ("passes", "groups"), 17: ("passes", "groups")}
for _NV in VIEWS_K1:
    EXACT["views_NV%d" % _NV] = _case(lambda NV=_NV: _views(NV), _views_aggs(_NV), path="gather", CW=4, many=_NV > 8)
for _C in (12, 128):
    for _NV in (3, 9):
        EXACT["scatter_C%d_NV%d" % (_C, _NV)] = _case(lambda C=_C, NV=_NV: _std(C, NV, 90 + C + NV, dup={8: 0} if NV == 9 else None), EXACT_AGGS,
                                                      path="scatter", kernel="scatter_many" if _NV > 8 else "scatter")
for _NV in (3, 9):
    EXACT["scatter_C32_atomics_NV%d" % _NV] = _case(lambda NV=_NV: _std(32, NV, 95 + NV, dup={8: 0} if NV == 9 else None), EXACT_AGGS,
                                                    env={"LT_UNPROJ_BWD_ATOMICS": "1"}, path="scatter", kernel="scatter_many" if _NV > 8 else "scatter")
CHUNKS = _case(lambda: _std(8, 3, 96, B=3), EXACT_AGGS, path="gather", CW=2)
EXACT["chunks"] = CHUNKS
EXACT["op_cw8"] = _case(lambda: _std(32, 3, 97), EXACT_AGGS, path="gather", CW=8)

# softmax everywhere, and conf_norm where the confidences cannot make it exact; fp32 and bf16 maps
TOLERANCED = {}
for _ty, _dt in (("fp32", F32), ("bf16", BF16)):
    for _C in (8, 32):
        TOLERANCED["cw%d_%s" % (_C // 4, _ty)] = _case(lambda C=_C: _std(C, 3, 110 + C), ("softmax", "conf_norm"), dtype=_dt, path="gather", CW=_C // 4, k1="mv4")
    TOLERANCED["seams_C16_%s" % _ty] = _case(lambda: _seams(16, 40), ("softmax", "conf_norm"), dtype=_dt, path="gather", CW=4)
    for _NV in (1, 4, 5, 8, 9, 17):
        TOLERANCED["views_NV%d_%s" % (_NV, _ty)] = _case(lambda NV=_NV: _views(NV), ("softmax",) + (() if _NV in POW2_CONF else ("conf_norm",)), dtype=_dt,
                                                          path="gather", CW=4, many=_NV > 8)


_MADE = {}


def make(table, cid):
    """The case's host tensors, made once and never written to."""
    key = (id(table), cid)
    if key not in _MADE:
        _MADE[key] = table[cid]["make"]()
    return _MADE[key]


def conf_terms(plan, N):
    """fp32 terms per sum of the confidence gradient: K1's per-lane accumulator on the gather path, every voxel through the scatter's atomics."""
    return plan["k1_items_per_lane"] if plan["path"] == "gather" else N


# ---- realistic geometry --------------------------------------------------------------------------------------------------------------------------------
REAL_NV, REAL_C, REAL_HW, REAL_VS = (1, 2, 4, 5, 7, 8), (8, 32), (24, 28), (6, 5, 9)
REAL_SEED = {(4, 32): 300}          # (the default seed of (4, 32) has a 'max' winner that differs between fp32 and fp64)
# (NV, C) -> seed, where the default violates a condition of the gate (tests/test_unproject_bwd_ref_cpu.py)
_REAL = {}


def realistic_case(NV, C):
    """Ring cameras at map resolution with camera 0 inside a rotated cuboid grid (its middle 6 x 5 x 9 voxels), randn maps, B = 2."""
    if (NV, C) not in _REAL:
        from oracle import synth
        from oracle import vol_oracle as O
        g = torch.Generator().manual_seed(REAL_SEED.get((NV, C), 200 + 10 * NV + C))
        h, w = REAL_HW
        K, R, t = synth.ring_cameras(NV, 96, inside=True)
        P = torch.from_numpy(O.resized_projection(K, R, t, (96, 96), (h, w))).float()[None].repeat(2, 1, 1, 1).contiguous()
        hm = torch.randn(2, NV, C, h, w, generator=g)
        conf = torch.rand(2, NV, C, generator=g) + 0.1
        base = torch.randn(2, 3, generator=g).numpy() * 100
        cv = torch.stack([U.box_coords(base[b], 2500.0, REAL_VS, 0.3 * b + 0.1) for b in range(2)])
        G = torch.randn(2, C, *REAL_VS, generator=g)
        _REAL[(NV, C)] = Case(hm, P, cv, conf, G, h, w, REAL_VS, None, None, None)
    return _REAL[(NV, C)]


def check_structure(cid, case):
    """What the structured point sets are built for, counted by round_stats on the case as it is launched (tests/test_unproject_bwd_ref_cpu.py holds the
    builders to more detail)."""
    kind = cid.split("_")[0]
    if kind not in ("pile", "alternate", "refill", "seams", "empty"):
        return None
    halves = 2 if case.hm.shape[2] <= 32 else 1
    taps = ref_taps(case.P, case.cv, case.h, case.w)
    st = None
    for b in range(case.hm.shape[0]):
        st = round_stats(taps, b, 1 if kind == "empty" else 0, case.vs, case.h, case.w, halves)
        if kind == "pile":
            assert min(st["multi"].values()) > 0, "pile: no round with 2, 3 and 4 hits in one cell: %r" % st["multi"]
        elif kind == "alternate":
            assert st["alt"] >= 32, "alternate: the pattern off[2] == off[0] != off[1] is missing"
        elif kind == "refill":
            assert st["cand"][(0, 0)] > G_LIST - 64 and len(st["empty"]) == 69, "refill: %d candidates, %d empty bricks" % (st["cand"][(0, 0)], len(st["empty"]))
        elif kind == "seams":
            assert st["straddle_half"] >= 27 and st["straddle_tile_x"] >= 27 and st["straddle_tile_y"] >= 36 and min(st["cand"].values()) > 0
        else:
            assert bool(taps.invalid[:, 1].all()) and set(st["cand"].values()) == {0}, "empty_view: view 1 has a weighted tap"
    return st
