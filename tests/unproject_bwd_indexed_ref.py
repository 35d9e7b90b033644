"""TEST INFRASTRUCTURE for the indexed unprojection backward (lt_unproject_indexed_bwd, csrc/unproject_bwd.hip): importable without a GPU.

* indexed_ref_backward(): what a frame index MEANS in the backward, stated through the unindexed reference -- unproject_bwd_ref.ref_backward (with a mask:
  unproject_bwd_masked_ref.masked_ref_backward) of every cuboid on its frame's maps, projections and confidences, added into the frame with index_add over
  frame_of; conf_norm's chain rule is applied once, on the per-frame sum of the raw confidence sums.  A frame without a cuboid stays zero.  fp64.
* ws_bytes(): the workspace that makes the entry walk the cuboids ``chunk`` at a time (include/lt_hip.h states the layout).
* the cases of tests/test_gpu_unproject_indexed_bwd_kernels.py, here so that tests/test_unproject_bwd_indexed_ref_cpu.py can hold them to the conditions
  their gates rest on (the fp32 and fp64 'max' winners agree on the Gaussian cases)."""
import torch

import unproject_bwd_masked_ref as M
import unproject_bwd_ref as R

AGGS, EXACT_AGGS = R.AGGS, R.EXACT_AGGS
LATTICE_FRAME_OF = (2, 0, 2, 2, 0)          # F = 3: frame 1 is empty, frame 2 has three cuboids, unsorted
LATTICE_F = 3
GATE_FRAME_OF = (1, 0, 1, 1, 0)             # F = 2, P = 5
GATE_HW, GATE_VS, GATE_C = (24, 24), (16, 16, 16), 32
GATE_SEED = {4: 7102, 10: 7100}             # seeds at which no 'max' winner differs between fp32 and fp64 (tests/test_unproject_bwd_indexed_ref_cpu.py)


def conf_norm_chain(s, conf, on=None):
    """s (NV, C) = d loss / d NORMALISED confidence n_v = c_v / S -> d loss / d c_v = (s_v - sum_u s_u n_u) / S, over the views ``on`` (bool (NV,); None: all);
    a masked view gets 0.  fp64."""
    s, c = s.double(), conf.double()
    on = torch.ones(s.shape[0], dtype=torch.bool) if on is None else on
    out = torch.zeros_like(s)
    if not bool(on.any()):
        return out
    S = c[on].sum(0)
    out[on] = (s[on] - (s[on] * c[on] / S).sum(0)) / S
    return out


def indexed_ref_backward(hm, proj, coords, G, agg, frame_of, conf=None, mask=None, dtype=torch.float64):
    """hm (F,NV,C,h,w), proj (F,NV,3,4), conf (F,NV,C), mask (F,NV) or None by FRAME; coords (P,v0,v1,v2,3), G (P,C,v0,v1,v2) by CUBOID; frame_of: P frames
    -> (grad_feats (F,NV,C,h,w), grad_conf (F,NV,C) or None): the per-cuboid reference on the cuboid's frame, index_add over frame_of."""
    F, NV, C, h, w = hm.shape
    fof = [int(f) for f in frame_of]
    is_conf = agg in ("conf", "conf_norm")
    gf = torch.zeros(F, NV, C, h, w, dtype=dtype)
    s = torch.zeros(F, NV, C, dtype=torch.float64) if is_conf else None          # per frame: sum over its cuboids and their voxels of g * x_v
    for p, f in enumerate(fof):
        args = (hm[f:f + 1], proj[f:f + 1], coords[p:p + 1], G[p:p + 1])
        cf = None if conf is None else conf[f:f + 1]
        one = (lambda a: R.ref_backward(*args, a, cf, dtype=dtype)[:2]) if mask is None else (lambda a: M.masked_ref_backward(*args, a, mask[f:f + 1], cf, dtype=dtype)[:2])
        gf.index_add_(0, torch.tensor([f]), one(agg)[0])
        if is_conf:          # the raw sums are the 'conf' gradient of the confidences (a masked view: zero)
            s.index_add_(0, torch.tensor([f]), one("conf")[1].double())
    if agg == "conf_norm":
        s = torch.stack([conf_norm_chain(s[f], conf[f], None if mask is None else mask[f] != 0) for f in range(F)])
    return gf, (s.to(dtype) if is_conf else None)


def gather_by_frame(case, frame_of):
    """The frame-side tensors of a Case gathered by frame_of (what the unindexed entries are handed instead): hm, P, conf with P entries."""
    idx = torch.tensor([int(f) for f in frame_of])
    return case.hm[idx].contiguous(), case.P[idx].contiguous(), case.conf[idx].contiguous()


def ws_bytes(lib, P, NV, C, vs, chunk=None):
    """Workspace bytes with which lt_unproject_indexed_bwd walks the P cuboids ``chunk`` at a time (None: all at once): the fp64 confidence partials of all P
    cuboids (min(2048, ceil(nvox C / 1024)) NV C 8 bytes each, rounded up to 256 in all) plus ``chunk`` cuboids' shares of the rest."""
    whole = lib.lt_unproject_indexed_bwd_workspace(P, NV, C, *vs)
    if chunk is None or whole == 0:
        return whole
    nvox = vs[0] * vs[1] * vs[2]
    partials = (min(2048, -(-nvox * (C // 4) // 256)) * NV * C * 8 * P + 255) // 256 * 256
    share = (whole - partials) // P
    assert share * P == whole - partials and share % 256 == 0
    return partials + share * chunk


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------------
_MADE = {}


def lattice_frames_case(NV, C, vs, seed, dtype=torch.float32):
    """A lattice case (exact in fp32 whatever the addition order) as frames and cuboids: unproject_bwd_ref.lattice_case with B = 5 gives the five cuboids'
    coordinates and upstream gradients (cv, G) and, in its first three samples, the three frames' maps and confidences (the projections are the same in
    every sample).  -> (frames Case with B = 3, cv (5,...), G (5,...))."""
    key = ("lattice", NV, C, vs, seed)
    if key not in _MADE:
        h, w = R.SEAM_HW
        c = R.lattice_case(len(LATTICE_FRAME_OF), NV, C, h, w, vs, seed)
        F = LATTICE_F
        _MADE[key] = (c._replace(hm=c.hm[:F].contiguous(), P=c.P[:F].contiguous(), conf=c.conf[:F].contiguous()), c.cv, c.G)
    return _MADE[key]


def gaussian_case(NV, C=GATE_C, hw=GATE_HW, vs=GATE_VS, F=2, P=5, seed=None):
    """Ring cameras (camera 0 inside the grid: voxels at depth <= 0), randn maps per frame, a shifted coordinate grid and a randn upstream gradient per
    cuboid.  -> (hm (F,NV,C,h,w), proj (F,NV,3,4), conf (F,NV,C), cv (P,*vs,3), G (P,C,*vs))."""
    seed = GATE_SEED.get(NV, 7100 + NV) if seed is None else seed
    key = ("gauss", NV, C, hw, vs, F, P, seed)
    if key not in _MADE:
        from oracle import synth
        from oracle import vol_oracle as O
        g = torch.Generator().manual_seed(seed)
        h, w = hw
        K, Rm, t = synth.ring_cameras(NV, 96, inside=True)
        proj = torch.from_numpy(O.resized_projection(K, Rm, t, (96, 96), (h, w))).float()[None].repeat(F, 1, 1, 1).contiguous()
        proj[1:, :, :, 3] += 3.0 * torch.arange(1, F, dtype=torch.float32)[:, None, None]          # the frames' cameras differ a little
        hm = torch.randn(F, NV, C, h, w, generator=g)
        conf = torch.rand(F, NV, C, generator=g) + 0.1
        ax = [torch.linspace(-900.0, 900.0, n) for n in vs]
        cv = torch.stack(torch.meshgrid(*ax, indexing="ij"), dim=-1)[None].repeat(P, 1, 1, 1, 1).contiguous()
        cv += 37.0 * torch.arange(P, dtype=torch.float32)[:, None, None, None, None]
        G = torch.randn(P, C, *vs, generator=g)
        _MADE[key] = (hm, proj, conf, cv, G)
    return _MADE[key]


def max_winners_agree(hm, proj, conf, cv, G, frame_of):
    """True when, for every cuboid, the 'max' winner of every (voxel, channel) is the same view in fp32 and in fp64 arithmetic."""
    for p, f in enumerate(frame_of):
        w32 = R.ref_backward(hm[f:f + 1], proj[f:f + 1], cv[p:p + 1], G[p:p + 1], "max", dtype=torch.float32)[3].winner
        w64 = R.ref_backward(hm[f:f + 1], proj[f:f + 1], cv[p:p + 1], G[p:p + 1], "max", dtype=torch.float64)[3].winner
        if not torch.equal(w32, w64):
            return False
    return True
