// Backward of the unprojection (what torch.autograd derives for the reference from op.unproject_heatmaps, mvn/utils/op.py:99-166):
//   no gradient flows to the grid / projection / coordinates (none requires grad there); grid_sample's backward spreads wt_tap * g over
//   the four taps of feat[b, v, c]; a sample with depth <= 0 is zeroed IN PLACE after sampling (op.py:141), so it passes no gradient
//   back but its 0 still enters the view softmax; softmax aggregation out = sum_v w_v x_v, w = softmax_v(x):
//   d out / d x_v = w_v (1 + x_v - out); 'conf': d out / d x_v = c_v, d out / d c_v = x_v (summed over the voxels).
//
// Round 3: a GATHER, deterministic, no atomics at all (the round-2 scatter issued NV x 4 taps x C global float atomics per voxel: 134 M
// per sample at config 2, 1.8 ms per sample, and was not bitwise repeatable).  Three launches over a workspace:
//   K0  unproj_taps_kernel   one wave per 4x4x4 voxel brick: every voxel projected into every view ONCE: its tap record (the 2x2 patch's
//                            origin pixel and the four bilinear weights, 0 = padding / depth <= 0) -> txy / tw[b][v][voxel], and the
//                            pixel bounding box of the brick's weighted taps -> bbox[b][v][brick] (empty bricks: x0 > x1)
//   K1  unproj_dx_kernel     one lane per (voxel, 4-channel vector), the forward's sampling redone: d out / d x_v times the upstream
//                            gradient -> dxs[b][v][voxel][C] fp32 (the per-view gradient of the SAMPLED value); the confidence gradient
//                            as per-workgroup partial sums, added in a fixed order by unproj_gconf_finalize_kernel
//   K2  unproj_gather_kernel one workgroup per (16 x 16 pixel tile, view, sample), the tile's gradient in LDS: walks the bricks whose
//                            bbox meets the tile in index order (next brick's tap records and dx values in flight), and adds every tap
//                            that falls INSIDE the tile in (brick, voxel) order -- each wave owns a quarter of the channels, each
//                            half-wave half of the tile's pixel columns, lane = pixel parity class x channel (the four taps of a
//                            voxel have four different parities, and a cell is only ever updated by the lane of its parity); plain
//                            LDS read-add-write in rounds of four hits, the sums forwarded in registers when hits of a round meet in
//                            one cell.  The tile is
//                            stored once with plain stores (no pre-zeroed output: every pixel of the map belongs to exactly one tile).
// A tap is processed by exactly one workgroup (the one whose tile holds its pixel), every cell's additions have a fixed order: results
// are bitwise repeatable.  Measured on the way (B = 8, config-2 shape, profiles/r03_unproject_bwd.md): the same gather with ds_add_f32
// (LDS float atomics) took 9.0 ms, 3.1 ms with the atomic replaced by a plain store -- LDS float atomics run at a small fraction of the
// LDS rate -- and 0.8 ms without the hit loop.  The round-2 scatter kernel stays reachable (LT_UNPROJ_BWD_ATOMICS=1) as the A/B
// reference and for configurations the gather does not take (C > 64 or not a power of two).
// More than 8 views (up to UB_MANYV = 32): K0 and K2 as they are; K1, the confidence finalizer and the scatter have many-view forms below that
// hold no per-view register array (the host entry dispatches on NV > UB_MAXV; nothing changes for NV <= 8).
// lt_unproject_masked_bwd (training with per-sample view masks): MASKED instantiations of K0, of every K1 form and of both finalizers -- a masked view gets
// empty bounding boxes from K0 and is skipped by K1, so the unchanged K2 stores zeros for it; the valid views are walked in index order.  Gather path only.
// lt_unproject_indexed_bwd (training with several cuboids per frame): INDEXED instantiations, on the masked forms, of K0 and of every K1 form -- the grid
// by cuboid, the frame-side reads through f = frame_of[p], a scalar per workgroup -- and of K2, one workgroup per (tile, view, FRAME) that keeps its tile
// across the frame's cuboids (additions in (cuboid, brick, voxel) order); the confidence partials of all cuboids are finalized once, per frame.  Gather
// path only; the cuboids may be walked in chunks (a later chunk's tile starts from the stored sums), with the same bits for every workspace size.
#include <stdlib.h>

#include <type_traits>

#include "unproj_geom.h"

using namespace lt;

namespace {

struct UnprojBwdArgs {
    const void* feats;       // (B, NV, h, w, C) T
    const float* proj;       // (B, NV, 3, 4)
    const float* coords;     // (B, nvox, 3)
    const float* conf;       // (B, NV, C) or null
    const float* gout;       // (B, nvox, C) fp32: dL/d volume, channels-last
    float* gfeats;           // (B, NV, h, w, C) fp32
    float* gconf;            // (B, NV, C) fp32, or null
    float* dxs;              // workspace: (B, NV, nvox, C) fp32
    int* bbox;               // workspace: (B, NV, nbricks, 4) = x0, x1, y0, y1 of the taps with weight (x0 > x1: none)
    int* txy;                // workspace: (B, NV, nvox) origin pixel of the 2x2 tap patch, (x0 + 1) | (y0 + 1) << 16  (x0, y0 >= -1)
    float4* tw;              // workspace: (B, NV, nvox) weights of the taps (x0,y0) (x0+1,y0) (x0,y0+1) (x0+1,y0+1); 0 = padding / masked
    double* gcpart;          // workspace: (B, nblk1, NV, C) partial confidence gradients
    int B, NV, C, h, w, agg;
    int v0, v1, v2, nb0, nb1, nb2;
    long long nvox;
};

// lt_unproject_masked_bwd's K0, K1 and finalizers get the mask behind the same arguments; the unmasked kernels (and K2, which needs no mask: a
// masked view has only empty bounding boxes) keep UnprojBwdArgs as their whole argument block
struct UnprojBwdMaskedArgs : UnprojBwdArgs {
    const uint8_t* mask;     // (B, NV), non-zero = the view is valid
};
// lt_unproject_indexed_bwd (several cuboids per frame): B counts the CUBOIDS of one chunk; coords, gout and the whole workspace are indexed by the
// chunk's cuboid b, feats, proj, conf and mask by its frame frame_of[p0 + b] < F, gfeats and gconf by the frame.  Built on the masked form: a null
// mask there means every view is valid.
struct UnprojBwdIndexedArgs : UnprojBwdMaskedArgs {
    const int32_t* frame_of; // (P) the frame of every cuboid
    int F, P;                // frames; cuboids of the whole call (the confidence finalizer walks all of them)
    int p0;                  // first cuboid of this chunk (the chunk holds cuboids p0 .. p0 + B - 1)
};
template <bool MASKED, bool INDEXED = false>
using UnprojBwdArgsOf = std::conditional_t<INDEXED, UnprojBwdIndexedArgs, std::conditional_t<MASKED, UnprojBwdMaskedArgs, UnprojBwdArgs>>;

constexpr int UB_MAXV = 8;   // views kept in registers

// the frame of cuboid p: uniform over the workgroup (p comes from the block index or from a scalar loop), read once as a scalar and clamped into
// [0, F-1] as the forward does -- a bad index reads a wrong frame, never outside the frame-side buffers
__device__ __forceinline__ int frame_of_cuboid(const UnprojBwdIndexedArgs& a, int p) {
    const int f = __builtin_amdgcn_readfirstlane(a.frame_of[p]);
    return min(max(f, 0), a.F - 1);
}
// the frame-side index of the workgroup's sample b: b itself, or the frame of the chunk's cuboid b
template <bool MASKED, bool INDEXED>
__device__ __forceinline__ int frame_side(const UnprojBwdArgsOf<MASKED, INDEXED>& a, int b) {
    if constexpr (INDEXED) return frame_of_cuboid(a, a.p0 + b);
    else return b;
}

// Sample b's mask row as bits (NV <= 32).  b comes from the block index in K0 and K1: the row is read with scalar loads into one scalar
// register, and every test of a view below is a scalar branch.
__device__ __forceinline__ unsigned mask_bits(const uint8_t* __restrict__ mask, int b, int NV) {
    const uint8_t* mk = mask + (long long)b * NV;
    unsigned bits = 0;
    for (int v = 0; v < NV; ++v) bits |= (mk[v] ? 1u : 0u) << v;
    return bits;
}
// the bits of frame-side row f as the kernels below take them: all ones without a mask (INDEXED: a null mask means every view is valid)
template <bool MASKED, bool INDEXED>
__device__ __forceinline__ unsigned mask_bits_of(const UnprojBwdArgsOf<MASKED, INDEXED>& a, int f) {
    if constexpr (INDEXED) return a.mask ? mask_bits(a.mask, f, a.NV) : ~0u;
    else if constexpr (MASKED) return mask_bits(a.mask, f, a.NV);
    else return ~0u;
}
// does view v take part?  Without a mask: constant true, so the unmasked instantiations compile to what they did before the mask existed
template <bool MASKED> __device__ __forceinline__ bool view_on(unsigned mbits, int v) {
    if constexpr (MASKED) return ((mbits >> v) & 1u) != 0;
    else return true;
}

// one view's sample of one voxel / channel vector: all four clamped corners, blended with the zeroed weights (the second load discipline of unproj_geom.h)
template <typename T>
__device__ __forceinline__ void sample_one_view(const T* fm, const Tap& t, int w, int C, float (&x)[4]) {
    float t0[4], t1[4], t2[4], t3[4];
    ChVec<T, 4>::ld(fm + (long long)(t.y[0] * w + t.x[0]) * C, t0); ChVec<T, 4>::ld(fm + (long long)(t.y[1] * w + t.x[1]) * C, t1);
    ChVec<T, 4>::ld(fm + (long long)(t.y[2] * w + t.x[2]) * C, t2); ChVec<T, 4>::ld(fm + (long long)(t.y[3] * w + t.x[3]) * C, t3);
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = t0[e] * t.k[0] + t1[e] * t.k[1] + t2[e] * t.k[2] + t3[e] * t.k[3];
}

// sampled values x[v][4] of one voxel / channel vector in every view (the forward's bilinear sampling with its padding / depth rules)
// MASKED: a masked view is neither projected nor sampled (its matrix and its map are never read); its tp[v] and x[v] stay unset
template <typename T, int MV, bool MASKED = false>
__device__ __forceinline__ void sample_views(const UnprojBwdArgs& a, const T* feats, const float* P, float X0, float X1, float X2, int c0,
                                             Tap (&tp)[MV], float (&x)[MV][4], unsigned mbits = ~0u) {
    const long long hw = (long long)a.h * a.w;
#pragma unroll
    for (int v = 0; v < MV; ++v) {
        if (v < a.NV && view_on<MASKED>(mbits, v)) {
            tp[v] = project_taps<false>(P + v * 12, X0, X1, X2, a.h, a.w);
            sample_one_view<T>(feats + v * hw * a.C + c0, tp[v], a.w, a.C, x[v]);
        }
    }
}

// d out / d x_v times the upstream gradient, per channel of the vector; gc[v][e] = g * x_v (the confidence gradient's summand).
// MASKED: the valid views alone, in index order -- the first valid view starts the max as view 0 does without a mask, so on the valid views
// this is the unmasked arithmetic on the compacted views, operation for operation; dx[v] of a masked view stays unset (nothing reads it)
template <int MV, bool MASKED = false>
__device__ __forceinline__ void view_gradients(const UnprojBwdArgs& a, int b, int c0, const float (&g)[4], const float (&x)[MV][4],
                                               float (&dx)[MV][4], unsigned mbits = ~0u) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (a.agg == LT_AGG_SOFTMAX) {
            float m = x[0][e];
            if constexpr (MASKED) {
                bool have = false;
#pragma unroll
                for (int v = 0; v < MV; ++v) if (v < a.NV && view_on<MASKED>(mbits, v)) { m = have ? fmaxf(m, x[v][e]) : x[v][e]; have = true; }
            } else {
#pragma unroll
                for (int v = 1; v < MV; ++v) if (v < a.NV) m = fmaxf(m, x[v][e]);
            }
            float s = 0.f, tt = 0.f, ex[MV];
#pragma unroll
            for (int v = 0; v < MV; ++v) if (v < a.NV && view_on<MASKED>(mbits, v)) { ex[v] = expf(x[v][e] - m); s += ex[v]; tt += x[v][e] * ex[v]; }
            const float out = __fdiv_rn(tt, s);
#pragma unroll
            for (int v = 0; v < MV; ++v) if (v < a.NV && view_on<MASKED>(mbits, v)) dx[v][e] = g[e] * __fdiv_rn(ex[v], s) * (1.0f + x[v][e] - out);
        } else if (a.agg == LT_AGG_MAX) {               // torch.max(dim): gradient to the FIRST maximal (valid) view
            int am = 0;
            float best = x[0][e];
            if constexpr (MASKED) {
                bool have = false;
#pragma unroll
                for (int v = 0; v < MV; ++v)
                    if (v < a.NV && view_on<MASKED>(mbits, v) && (!have || x[v][e] > best)) { best = x[v][e]; am = v; have = true; }
            } else {
#pragma unroll
                for (int v = 1; v < MV; ++v) if (v < a.NV && x[v][e] > best) { best = x[v][e]; am = v; }
            }
#pragma unroll
            for (int v = 0; v < MV; ++v) if (v < a.NV && view_on<MASKED>(mbits, v)) dx[v][e] = v == am ? g[e] : 0.f;
        } else if (a.agg == LT_AGG_CONF || a.agg == LT_AGG_CONF_NORM) {
            float cs = 1.f;
            if (a.agg == LT_AGG_CONF_NORM) {            // the forward normalises the confidences over the (valid) views (triangulation.py:268-269)
                cs = 0.f;
#pragma unroll
                for (int v = 0; v < MV; ++v) if (v < a.NV && view_on<MASKED>(mbits, v)) cs += a.conf[((long long)b * a.NV + v) * a.C + c0 + e];
            }
#pragma unroll
            for (int v = 0; v < MV; ++v)
                if (v < a.NV && view_on<MASKED>(mbits, v)) {
                    const float cv = a.conf[((long long)b * a.NV + v) * a.C + c0 + e];
                    dx[v][e] = g[e] * (a.agg == LT_AGG_CONF_NORM ? __fdiv_rn(cv, cs) : cv);
                }
        } else {
#pragma unroll
            for (int v = 0; v < MV; ++v) if (v < a.NV && view_on<MASKED>(mbits, v)) dx[v][e] = g[e];
        }
    }
}

// ---- round-2 scatter (LT_UNPROJ_BWD_ATOMICS=1; gfeats / gconf zeroed by the host entry) ------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void unproject_bwd_kernel(const UnprojBwdArgs a) {
    const int tpv = a.C >> 2;                              // lanes per voxel (4 channels each)
    const long long items = a.nvox * tpv;
    const int b = blockIdx.y;
    const T* feats = (const T*)a.feats + (long long)b * a.NV * a.h * a.w * a.C;
    float* gfeats = a.gfeats + (long long)b * a.NV * a.h * a.w * a.C;
    const float* P = a.proj + (long long)b * a.NV * 12;
    const float* coords = a.coords + (long long)b * a.nvox * 3;
    const float* gout = a.gout + (long long)b * a.nvox * a.C;
    const long long hw = (long long)a.h * a.w;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < items; q += (long long)gridDim.x * 256) {
        const long long vox = q / tpv;
        const int c0 = (int)(q - vox * tpv) * 4;
        const float X0 = coords[vox * 3], X1 = coords[vox * 3 + 1], X2 = coords[vox * 3 + 2];
        float g[4];
        ChVec<float, 4>::ld(gout + vox * a.C + c0, g);
        Tap tp[UB_MAXV];
        float x[UB_MAXV][4], dx[UB_MAXV][4];
        sample_views<T, UB_MAXV>(a, feats, P, X0, X1, X2, c0, tp, x);
        view_gradients<UB_MAXV>(a, b, c0, g, x, dx);
        if (a.gconf && a.agg == LT_AGG_CONF) {
#pragma unroll
            for (int v = 0; v < UB_MAXV; ++v)
                if (v < a.NV)
#pragma unroll
                    for (int e = 0; e < 4; ++e) atomicAdd(a.gconf + ((long long)b * a.NV + v) * a.C + c0 + e, g[e] * x[v][e]);
        }
#pragma unroll
        for (int v = 0; v < UB_MAXV; ++v) {
            if (v < a.NV) {
                float* gm = gfeats + v * hw * a.C + c0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float wk = tp[v].k[k];
                    if (wk != 0.f) {
                        float* dst = gm + (long long)(tp[v].y[k] * a.w + tp[v].x[k]) * a.C;
#pragma unroll
                        for (int e = 0; e < 4; ++e) atomicAdd(dst + e, wk * dx[v][e]);
                    }
                }
            }
        }
    }
}

// ---- gather: bricks ---------------------------------------------------------------------------------------------------------------------
// voxel of (brick, lane): bricks are 4 x 4 x 4 voxels of the (v0, v1, v2) grid; -1 past the grid's end
__device__ __forceinline__ long long brick_voxel(const UnprojBwdArgs& a, int brick, int lane) {
    const int b2 = brick % a.nb2, b1 = (brick / a.nb2) % a.nb1, b0 = brick / (a.nb2 * a.nb1);
    const int i = b0 * 4 + (lane >> 4), j = b1 * 4 + ((lane >> 2) & 3), k = b2 * 4 + (lane & 3);
    if (i >= a.v0 || j >= a.v1 || k >= a.v2) return -1;
    return ((long long)i * a.v1 + j) * a.v2 + k;
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// K0: grid (ceil(nbricks / 4), B), 4 waves, one brick per wave.  MASKED: a masked view gets the empty bounding box for every brick and nothing
// else -- it is not projected, its matrix is not read, its tap records stay unwritten: K2 then finds no brick for any tile of that view and
// stores zeros without reading its tap records or its dxs, and K1 never looks at a masked view.
// INDEXED (on the masked form, here and in every K1 form): sample b is the chunk's cuboid b -- its coordinates, upstream gradient and workspace rows by
// b, the projections, maps, confidences and mask of its frame f = frame_of[p0 + b].
template <bool MASKED = false, bool INDEXED = false>
__global__ __launch_bounds__(256) void unproj_taps_kernel(const UnprojBwdArgsOf<MASKED, INDEXED> a) {
    static_assert(MASKED || !INDEXED, "the indexed kernels are built on the masked form");
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int nbricks = a.nb0 * a.nb1 * a.nb2;
    const int brick = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (brick >= nbricks) return;
    const int f = frame_side<MASKED, INDEXED>(a, b);
    const float* P = a.proj + (long long)f * a.NV * 12;
    const float* coords = a.coords + (long long)b * a.nvox * 3;
    const long long vox = brick_voxel(a, brick, lane);
    float X0 = 0.f, X1 = 0.f, X2 = 0.f;
    if (vox >= 0) { X0 = coords[vox * 3]; X1 = coords[vox * 3 + 1]; X2 = coords[vox * 3 + 2]; }
    const unsigned mbits = mask_bits_of<MASKED, INDEXED>(a, f);
    for (int v = 0; v < a.NV; ++v) {
        int x0 = 1 << 30, x1 = -1, y0 = 1 << 30, y1 = -1;
        if constexpr (MASKED) {
            if (!view_on<MASKED>(mbits, v)) {
                if (lane == 0) *(int4*)(a.bbox + (((long long)b * a.NV + v) * nbricks + brick) * 4) = make_int4(x0, x1, y0, y1);
                continue;
            }
        }
        if (vox >= 0) {
            const Tap t = project_taps<false>(P + v * 12, X0, X1, X2, a.h, a.w);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (t.k[k] != 0.f) { x0 = min(x0, t.x[k]); x1 = max(x1, t.x[k]); y0 = min(y0, t.y[k]); y1 = max(y1, t.y[k]); }
            const long long ti = ((long long)b * a.NV + v) * a.nvox + vox;
            a.txy[ti] = (t.x0 + 1) | ((t.y0 + 1) << 16);
            a.tw[ti] = make_float4(t.k[0], t.k[1], t.k[2], t.k[3]);
        }
        x0 = wave_min(x0); x1 = wave_max(x1); y0 = wave_min(y0); y1 = wave_max(y1);
        if (lane == 0) *(int4*)(a.bbox + (((long long)b * a.NV + v) * nbricks + brick) * 4) = make_int4(x0, x1, y0, y1);
    }
}

// K1: grid (nblk1, B): one lane per (voxel, 4-channel vector), grid-stride (stride a multiple of C/4: a lane keeps its channel vector).
// MV = view capacity of the register arrays (4 or 8): at 4 views the kernel fits 128 VGPRs and two waves share a SIMD
// MASKED: masked views are skipped in the sampling, in every cross-view reduction and in the stores (K2 never reads their dxs); their
// confidence partials are written as the zeros their accumulators still hold.  A sample without a valid view walks no voxel.
// gfx950 resource usage, fp32 / bf16 maps: see DESIGN.md ("Masked unprojection backward")
template <typename T, int MV, bool MASKED = false, bool INDEXED = false>
__global__ __launch_bounds__(256) void unproj_dx_kernel(const UnprojBwdArgsOf<MASKED, INDEXED> a) {
    static_assert(MASKED || !INDEXED, "the indexed kernels are built on the masked form");
    __shared__ float red[256][4];
    const int tpv = a.C >> 2;
    const int b = blockIdx.y;
    const int f = frame_side<MASKED, INDEXED>(a, b);
    const unsigned mbits = mask_bits_of<MASKED, INDEXED>(a, f);
    const long long items = (MASKED && mbits == 0) ? 0 : a.nvox * tpv;
    const T* feats = (const T*)a.feats + (long long)f * a.NV * a.h * a.w * a.C;
    const float* P = a.proj + (long long)f * a.NV * 12;
    const float* coords = a.coords + (long long)b * a.nvox * 3;
    const float* gout = a.gout + (long long)b * a.nvox * a.C;
    float* dxs = a.dxs + (long long)b * a.NV * a.nvox * a.C;
    const bool want_gc = a.gconf != nullptr;
    float gc[MV][4];
#pragma unroll
    for (int v = 0; v < MV; ++v)
#pragma unroll
        for (int e = 0; e < 4; ++e) gc[v][e] = 0.f;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < items; q += (long long)gridDim.x * 256) {
        const long long vox = q / tpv;
        const int c0 = (int)(q - vox * tpv) * 4;
        const float X0 = coords[vox * 3], X1 = coords[vox * 3 + 1], X2 = coords[vox * 3 + 2];
        float g[4];
        ChVec<float, 4>::ld(gout + vox * a.C + c0, g);
        float x[MV][4], dx[MV][4];
        {
            Tap tp[MV];
            sample_views<T, MV, MASKED>(a, feats, P, X0, X1, X2, c0, tp, x, mbits);
        }
        view_gradients<MV, MASKED>(a, f, c0, g, x, dx, mbits);
#pragma unroll
        for (int v = 0; v < MV; ++v)
            if (v < a.NV && view_on<MASKED>(mbits, v)) {
                *(float4*)(dxs + ((long long)v * a.nvox + vox) * a.C + c0) = make_float4(dx[v][0], dx[v][1], dx[v][2], dx[v][3]);
                if (want_gc)
#pragma unroll
                    for (int e = 0; e < 4; ++e) gc[v][e] += g[e] * x[v][e];
            }
    }
    if (!want_gc) return;
    // per-workgroup partial of the confidence gradient: the 256 / tpv threads that share a channel vector, added in thread order
    const int cl = threadIdx.x % tpv;            // the stride (gridDim.x * 256) and 256 are multiples of tpv (C / 4 a power of two <= 64)
    for (int v = 0; v < a.NV; ++v) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) red[threadIdx.x][e] = gc[v][e];
        __syncthreads();
        if (threadIdx.x < tpv) {
            double s[4] = {0.0, 0.0, 0.0, 0.0};
            for (int t = threadIdx.x; t < 256; t += tpv)
#pragma unroll
                for (int e = 0; e < 4; ++e) s[e] += (double)red[t][e];
            double* dst = a.gcpart + (((long long)b * gridDim.x + blockIdx.x) * a.NV + v) * a.C + cl * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[e] = s[e];
        }
    }
}

// one thread per (b, c): the partials of every workgroup in index order; conf_norm: chain rule through c_v / sum_u c_u
// MASKED: the normaliser and the dot product run over the valid views (a masked view's confidence is never read); a masked view gets +0.0
template <bool MASKED = false>
__global__ void unproj_gconf_finalize_kernel(const UnprojBwdArgsOf<MASKED> a, int nblk1) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.B * a.C) return;
    const int b = i / a.C, c = i - b * a.C;
    unsigned mbits = ~0u;
    if constexpr (MASKED) mbits = mask_bits(a.mask, b, a.NV);
    double s[UB_MAXV];
    for (int v = 0; v < a.NV; ++v) {
        double t = 0.0;
        if (view_on<MASKED>(mbits, v))
            for (int k = 0; k < nblk1; ++k) t += a.gcpart[(((long long)b * nblk1 + k) * a.NV + v) * a.C + c];
        s[v] = t;
    }
    if (a.agg == LT_AGG_CONF_NORM) {      // s[v] is the gradient of the NORMALISED confidence n_v = c_v / S: d/dc_v = (s_v - sum_u s_u n_u) / S
        double S = 0.0, dot = 0.0;
        for (int v = 0; v < a.NV; ++v) if (view_on<MASKED>(mbits, v)) S += (double)a.conf[((long long)b * a.NV + v) * a.C + c];
        for (int v = 0; v < a.NV; ++v) if (view_on<MASKED>(mbits, v)) dot += s[v] * (double)a.conf[((long long)b * a.NV + v) * a.C + c] / S;
        for (int v = 0; v < a.NV; ++v) s[v] = view_on<MASKED>(mbits, v) ? (s[v] - dot) / S : 0.0;
    }
    for (int v = 0; v < a.NV; ++v) a.gconf[((long long)b * a.NV + v) * a.C + c] = (float)s[v];
}

// ---- more than UB_MAXV views ----------------------------------------------------------------------------------------------------------------
// Nothing below keeps a per-view register array sized by NV.  The three aggregations that are separable over the views once the confidence
// sum is known (sum, conf, conf_norm) run in GROUPS of up to UB_MAXV views, one group per workgroup (grid z), with the 8-view kernel's
// confidence-gradient accumulators and partial sums; softmax and max, which need statistics over all views (and have no confidence
// gradient), walk the views in passes and sample again in each, as the forward's any-NV branch does.  The gather-path kernels read K0's tap
// records (project_taps' own output) instead of projecting again, so they never touch the projection rows; the confidences are read once
// per workgroup into LDS.  The arithmetic is that of sample_views / view_gradients, expression for expression.
constexpr int UB_MANYV = 32;     // view limit of the many-view kernels: their LDS copies and the finalizer's workgroup shape are sized by it

// softmax / max over any number of views: view_gradients' arithmetic with the samples recomputed per pass.  sample(v, x) gives view v's
// sampled vector, emit(v, dx, sampled) takes d out / d x_v times the upstream gradient in view order (sampled: sample(v) was the last
// call of sample).  Pass 1: the max as an fmaxf chain / the first maximal view; pass 2: s and tt in view order; pass 3: dx_v.
// MASKED: the valid views (bits of mbits, at least one set) alone, in index order: the first valid view takes view 0's part, masked views
// are neither sampled nor emitted.
template <bool MASKED = false, class Sample, class Emit>
__device__ __forceinline__ void cross_view_gradients(int agg, int NV, const float (&g)[4], Sample sample, Emit emit, unsigned mbits = ~0u) {
    float x[4], dx[4];
    const int vf = MASKED ? __ffs((int)mbits) - 1 : 0;  // the view that starts the max
    if (agg == LT_AGG_SOFTMAX) {
        float m[4], s[4] = {0.f, 0.f, 0.f, 0.f}, tt[4] = {0.f, 0.f, 0.f, 0.f}, out[4];
        sample(vf, m);
        for (int v = vf + 1; v < NV; ++v) {
            if (!view_on<MASKED>(mbits, v)) continue;
            sample(v, x);
#pragma unroll
            for (int e = 0; e < 4; ++e) m[e] = fmaxf(m[e], x[e]);
        }
        for (int v = vf; v < NV; ++v) {
            if (!view_on<MASKED>(mbits, v)) continue;
            sample(v, x);
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float ex = expf(x[e] - m[e]); s[e] += ex; tt[e] += x[e] * ex; }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = __fdiv_rn(tt[e], s[e]);
        for (int v = vf; v < NV; ++v) {
            if (!view_on<MASKED>(mbits, v)) continue;
            sample(v, x);
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float ex = expf(x[e] - m[e]); dx[e] = g[e] * __fdiv_rn(ex, s[e]) * (1.0f + x[e] - out[e]); }
            emit(v, dx, true);
        }
    } else {                                            // LT_AGG_MAX: torch.max(dim), gradient to the FIRST maximal (valid) view
        float best[4];
        int am[4] = {vf, vf, vf, vf};
        sample(vf, best);
        for (int v = vf + 1; v < NV; ++v) {
            if (!view_on<MASKED>(mbits, v)) continue;
            sample(v, x);
#pragma unroll
            for (int e = 0; e < 4; ++e) if (x[e] > best[e]) { best[e] = x[e]; am[e] = v; }
        }
        for (int v = vf; v < NV; ++v) {
            if (!view_on<MASKED>(mbits, v)) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) dx[e] = v == am[e] ? g[e] : 0.f;
            emit(v, dx, false);
        }
    }
}

// K1 for NV > UB_MAXV, softmax / max: grid (nblk1, B), one lane per (voxel, 4-channel vector) as in unproj_dx_kernel; per view and pass one
// tap record (20 bytes, the same for the C / 4 lanes of a voxel) and four 16-byte taps.
// gfx950 resource usage: fp32 maps 64 VGPRs and 8 waves per SIMD, bf16 maps 68 VGPRs and 7 waves; no LDS, no scratch
// MASKED: every pass walks the valid views only (a masked view has no tap records: K0 wrote none); a sample without a valid view does nothing
template <typename T, bool MASKED = false, bool INDEXED = false>
__global__ __launch_bounds__(256) void unproj_dx_passes_kernel(const UnprojBwdArgsOf<MASKED, INDEXED> a) {
    static_assert(MASKED || !INDEXED, "the indexed kernels are built on the masked form");
    const int tpv = a.C >> 2;
    const long long items = a.nvox * tpv;
    const int b = blockIdx.y;
    const int f = frame_side<MASKED, INDEXED>(a, b);
    const unsigned mbits = mask_bits_of<MASKED, INDEXED>(a, f);
    if constexpr (MASKED) {
        if (mbits == 0) return;
    }
    const long long hw = (long long)a.h * a.w;
    const T* feats = (const T*)a.feats + (long long)f * a.NV * hw * a.C;
    const float* gout = a.gout + (long long)b * a.nvox * a.C;
    float* dxs = a.dxs + (long long)b * a.NV * a.nvox * a.C;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < items; q += (long long)gridDim.x * 256) {
        const long long vox = q / tpv;
        const int c0 = (int)(q - vox * tpv) * 4;
        float g[4];
        ChVec<float, 4>::ld(gout + vox * a.C + c0, g);
        const int* txy = a.txy + (long long)b * a.NV * a.nvox + vox;
        const float4* tw = a.tw + (long long)b * a.NV * a.nvox + vox;
        auto sample = [&](int v, float (&x)[4]) {
            const Tap t = tap_of_record(txy[(long long)v * a.nvox], tw[(long long)v * a.nvox], a.h, a.w);
            sample_one_view<T>(feats + v * hw * a.C + c0, t, a.w, a.C, x);
        };
        auto emit = [&](int v, const float (&dx)[4], bool) {
            *(float4*)(dxs + ((long long)v * a.nvox + vox) * a.C + c0) = make_float4(dx[0], dx[1], dx[2], dx[3]);
        };
        cross_view_gradients<MASKED>(a.agg, a.NV, g, sample, emit, mbits);
    }
}

// K1 for NV > UB_MAXV, sum / conf / conf_norm: grid (nblk1, B, ceil(NV / UB_MAXV)), workgroup z works on views [z * UB_MAXV, ...) with
// unproj_dx_kernel's lane mapping, accumulators and fp64 workgroup partials (same nblk1, same order: the partials of a view are the bits
// the 8-view kernel gives for it).  d out / d x_v per channel (c_v, or c_v / sum over ALL views for conf_norm) is computed once per
// workgroup into LDS; the maps are sampled only where a confidence gradient is asked for.
// gfx950 resource usage: fp32 maps 79 VGPRs and 6 waves per SIMD, bf16 maps 81 VGPRs and 5 waves; 6 KB LDS, no scratch
// MASKED: conf_norm's sum runs over the valid views; a masked view of the group is neither stored nor sampled (K0 wrote no tap records for
// it, K2 never reads its dxs) and its confidence partials are the zeros of its accumulators; a group without a valid view walks no voxel.
template <typename T, bool MASKED = false, bool INDEXED = false>
__global__ __launch_bounds__(256) void unproj_dx_groups_kernel(const UnprojBwdArgsOf<MASKED, INDEXED> a) {
    static_assert(MASKED || !INDEXED, "the indexed kernels are built on the masked form");
    __shared__ float red[256][4];
    __shared__ float coef[UB_MAXV][64];
    const int tpv = a.C >> 2;
    const int b = blockIdx.y;
    int f = b;                                            // (written out, like the mask word below: through the helpers the unindexed forms' instructions moved)
    if constexpr (INDEXED) f = frame_of_cuboid(a, a.p0 + b);
    const int vg = blockIdx.z * UB_MAXV, nv = min(UB_MAXV, a.NV - vg);
    unsigned mbits = ~0u, gbits = ~0u;                    // the sample's mask, and the group's share of it (bit v = view vg + v)
    if constexpr (MASKED) {
        if constexpr (INDEXED) mbits = a.mask ? mask_bits(a.mask, f, a.NV) : ~0u;          // (a null mask: every view valid)
        else mbits = mask_bits(a.mask, b, a.NV);
        gbits = mbits >> vg;
    }
    const long long items = (MASKED && (gbits & 0xffu) == 0) ? 0 : a.nvox * tpv;
    const long long hw = (long long)a.h * a.w;
    const T* feats = (const T*)a.feats + ((long long)f * a.NV + vg) * hw * a.C;
    const float* gout = a.gout + (long long)b * a.nvox * a.C;
    float* dxs = a.dxs + ((long long)b * a.NV + vg) * a.nvox * a.C;
    const bool is_conf = a.agg == LT_AGG_CONF || a.agg == LT_AGG_CONF_NORM;
    const bool want_gc = a.gconf != nullptr;
    if (is_conf) {
        for (int i = threadIdx.x; i < nv * a.C; i += 256) {
            const int v = i / a.C, c = i - v * a.C;
            const float* cf = a.conf + (long long)f * a.NV * a.C + c;
            if (!view_on<MASKED>(gbits, v)) continue;
            float cv = cf[(vg + v) * a.C];
            if (a.agg == LT_AGG_CONF_NORM) {
                float cs = 0.f;
                for (int u = 0; u < a.NV; ++u) if (view_on<MASKED>(mbits, u)) cs += cf[u * a.C];
                cv = __fdiv_rn(cv, cs);
            }
            coef[v][c] = cv;
        }
        __syncthreads();
    }
    float gc[UB_MAXV][4];
#pragma unroll
    for (int v = 0; v < UB_MAXV; ++v)
#pragma unroll
        for (int e = 0; e < 4; ++e) gc[v][e] = 0.f;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < items; q += (long long)gridDim.x * 256) {
        const long long vox = q / tpv;
        const int c0 = (int)(q - vox * tpv) * 4;
        float g[4];
        ChVec<float, 4>::ld(gout + vox * a.C + c0, g);
        const int* txy = a.txy + ((long long)b * a.NV + vg) * a.nvox + vox;
        const float4* tw = a.tw + ((long long)b * a.NV + vg) * a.nvox + vox;
#pragma unroll
        for (int v = 0; v < UB_MAXV; ++v)
            if (v < nv && view_on<MASKED>(gbits, v)) {
                float4 d = make_float4(g[0], g[1], g[2], g[3]);
                if (is_conf) {
                    const float4 k = *(const float4*)&coef[v][c0];
                    d = make_float4(g[0] * k.x, g[1] * k.y, g[2] * k.z, g[3] * k.w);
                }
                *(float4*)(dxs + ((long long)v * a.nvox + vox) * a.C + c0) = d;
                if (want_gc) {
                    float x[4];
                    const Tap t = tap_of_record(txy[(long long)v * a.nvox], tw[(long long)v * a.nvox], a.h, a.w);
                    sample_one_view<T>(feats + v * hw * a.C + c0, t, a.w, a.C, x);
#pragma unroll
                    for (int e = 0; e < 4; ++e) gc[v][e] += g[e] * x[e];
                }
            }
    }
    if (!want_gc) return;
    const int cl = threadIdx.x % tpv;
    for (int v = 0; v < nv; ++v) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) red[threadIdx.x][e] = gc[v][e];
        __syncthreads();
        if (threadIdx.x < tpv) {
            double s[4] = {0.0, 0.0, 0.0, 0.0};
            for (int t = threadIdx.x; t < 256; t += tpv)
#pragma unroll
                for (int e = 0; e < 4; ++e) s[e] += (double)red[t][e];
            double* dst = a.gcpart + (((long long)b * gridDim.x + blockIdx.x) * a.NV + vg + v) * a.C + cl * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[e] = s[e];
        }
    }
}

// unproj_gconf_finalize_kernel for NV > UB_MAXV: one workgroup per (sample, 8 channels) of 32 x 8 threads, thread (v, c) adds view v's
// partials in workgroup order; the conf_norm chain rule then reads every view's sum from LDS, in view order and in fp64 as the 8-view
// finalizer does (each thread for itself: the same S and dot in every thread of a channel).
// gfx950 resource usage: 54 VGPRs, 2 KB LDS, no scratch; 8 waves per SIMD
constexpr int UB_FIN_C = 8;
// MASKED: S and dot over the valid views; the thread of a masked view writes +0.0
template <bool MASKED = false>
__global__ __launch_bounds__(UB_MANYV * UB_FIN_C) void unproj_gconf_finalize_many_kernel(const UnprojBwdArgsOf<MASKED> a, int nblk1) {
    __shared__ double sv[UB_MANYV][UB_FIN_C];
    const int cc = a.C < UB_FIN_C ? a.C : UB_FIN_C;                       // channels per workgroup (C = 4: half of the threads idle)
    const int chunks = a.C / cc;
    const int b = blockIdx.x / chunks, ci = threadIdx.x % UB_FIN_C, v = threadIdx.x / UB_FIN_C;
    const int c = (blockIdx.x - b * chunks) * cc + ci;
    const bool mine = ci < cc && v < a.NV;
    unsigned mbits = ~0u;
    if constexpr (MASKED) mbits = mask_bits(a.mask, b, a.NV);
    const bool on = view_on<MASKED>(mbits, v);
    double t = 0.0;
    if (mine && on)
        for (int k = 0; k < nblk1; ++k) t += a.gcpart[(((long long)b * nblk1 + k) * a.NV + v) * a.C + c];
    sv[v][ci] = t;
    __syncthreads();
    if (!mine) return;
    if (a.agg == LT_AGG_CONF_NORM) {
        const float* cf = a.conf + (long long)b * a.NV * a.C + c;
        double S = 0.0, dot = 0.0;
        for (int u = 0; u < a.NV; ++u) if (view_on<MASKED>(mbits, u)) S += (double)cf[u * a.C];
        for (int u = 0; u < a.NV; ++u) if (view_on<MASKED>(mbits, u)) dot += sv[u][ci] * (double)cf[u * a.C] / S;
        t = on ? (t - dot) / S : 0.0;
    }
    a.gconf[((long long)b * a.NV + v) * a.C + c] = (float)t;
}

// lt_unproject_indexed_bwd's finalizer, for every NV: unproj_gconf_finalize_many_kernel's shape with one workgroup per (FRAME, 8 channels).  a.gcpart
// holds the partials of all a.P cuboids, (P, nblk1, NV, C), whatever the chunking of K0 - K2 was; thread (v, c) adds those of its frame's cuboids in
// (cuboid, workgroup) order -- frame_of is scanned in ascending p, a scalar per step -- and rounds once, so with one cuboid per frame these are the
// unindexed finalizers' bits.  conf_norm's chain rule is applied once, on that sum; a frame without a cuboid gets +0.0.
// gfx950 resource usage: DESIGN.md ("Indexed unprojection backward")
__global__ __launch_bounds__(UB_MANYV * UB_FIN_C) void unproj_gconf_finalize_indexed_kernel(const UnprojBwdIndexedArgs a, int nblk1) {
    __shared__ double sv[UB_MANYV][UB_FIN_C];
    const int cc = a.C < UB_FIN_C ? a.C : UB_FIN_C;
    const int chunks = a.C / cc;
    const int f = blockIdx.x / chunks, ci = threadIdx.x % UB_FIN_C, v = threadIdx.x / UB_FIN_C;
    const int c = (blockIdx.x - f * chunks) * cc + ci;
    const bool mine = ci < cc && v < a.NV;
    const unsigned mbits = mask_bits_of<true, true>(a, f);
    const bool on = view_on<true>(mbits, v);
    double t = 0.0;
    for (int p = 0; p < a.P; ++p) {
        if (frame_of_cuboid(a, p) != f) continue;
        if (mine && on)
            for (int k = 0; k < nblk1; ++k) t += a.gcpart[(((long long)p * nblk1 + k) * a.NV + v) * a.C + c];
    }
    sv[v][ci] = t;
    __syncthreads();
    if (!mine) return;
    if (a.agg == LT_AGG_CONF_NORM) {
        const float* cf = a.conf + (long long)f * a.NV * a.C + c;
        double S = 0.0, dot = 0.0;
        for (int u = 0; u < a.NV; ++u) if (view_on<true>(mbits, u)) S += (double)cf[u * a.C];
        for (int u = 0; u < a.NV; ++u) if (view_on<true>(mbits, u)) dot += sv[u][ci] * (double)cf[u * a.C] / S;
        t = on ? (t - dot) / S : 0.0;
    }
    a.gconf[((long long)f * a.NV + v) * a.C + c] = (float)t;
}

// round-2 scatter for NV > UB_MAXV (same semantics as unproject_bwd_kernel: zeroed outputs, float atomics): one view at a time, softmax /
// max in the passes of cross_view_gradients with the projection redone in each; the sample's projection rows in LDS.
// gfx950 resource usage: fp32 maps 90 VGPRs, bf16 maps 85 VGPRs; 1.5 KB LDS, no scratch; 5 waves per SIMD
template <typename T>
__global__ __launch_bounds__(256) void unproject_bwd_many_kernel(const UnprojBwdArgs a) {
    __shared__ float Ps[UB_MANYV * 12];
    const int tpv = a.C >> 2;
    const long long items = a.nvox * tpv;
    const int b = blockIdx.y;
    const long long hw = (long long)a.h * a.w;
    const T* feats = (const T*)a.feats + (long long)b * a.NV * hw * a.C;
    float* gfeats = a.gfeats + (long long)b * a.NV * hw * a.C;
    const float* coords = a.coords + (long long)b * a.nvox * 3;
    const float* gout = a.gout + (long long)b * a.nvox * a.C;
    for (int i = threadIdx.x; i < a.NV * 12; i += 256) Ps[i] = a.proj[(long long)b * a.NV * 12 + i];
    __syncthreads();
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < items; q += (long long)gridDim.x * 256) {
        const long long vox = q / tpv;
        const int c0 = (int)(q - vox * tpv) * 4;
        const float X0 = coords[vox * 3], X1 = coords[vox * 3 + 1], X2 = coords[vox * 3 + 2];
        float g[4];
        ChVec<float, 4>::ld(gout + vox * a.C + c0, g);
        Tap cur;
        auto scatter = [&](int v, const float (&dx)[4]) {
            float* gm = gfeats + v * hw * a.C + c0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float wk = cur.k[k];
                if (wk != 0.f) {
                    float* dst = gm + (long long)(cur.y[k] * a.w + cur.x[k]) * a.C;
#pragma unroll
                    for (int e = 0; e < 4; ++e) atomicAdd(dst + e, wk * dx[e]);
                }
            }
        };
        if (a.agg == LT_AGG_SOFTMAX || a.agg == LT_AGG_MAX) {
            auto sample = [&](int v, float (&x)[4]) {
                cur = project_taps<false>(Ps + v * 12, X0, X1, X2, a.h, a.w);
                sample_one_view<T>(feats + v * hw * a.C + c0, cur, a.w, a.C, x);
            };
            auto emit = [&](int v, const float (&dx)[4], bool sampled) {
                if (!sampled) {
                    if (dx[0] == 0.f && dx[1] == 0.f && dx[2] == 0.f && dx[3] == 0.f) return;      // max: a view that wins no channel
                    cur = project_taps<false>(Ps + v * 12, X0, X1, X2, a.h, a.w);
                }
                scatter(v, dx);
            };
            cross_view_gradients(a.agg, a.NV, g, sample, emit);
        } else {
            for (int v = 0; v < a.NV; ++v) {
                cur = project_taps<false>(Ps + v * 12, X0, X1, X2, a.h, a.w);
                float dx[4] = {g[0], g[1], g[2], g[3]};
                if (a.agg == LT_AGG_CONF) {
                    const float* cf = a.conf + ((long long)b * a.NV + v) * a.C + c0;
#pragma unroll
                    for (int e = 0; e < 4; ++e) dx[e] = g[e] * cf[e];
                    if (a.gconf) {
                        float x[4];
                        sample_one_view<T>(feats + v * hw * a.C + c0, cur, a.w, a.C, x);
#pragma unroll
                        for (int e = 0; e < 4; ++e) atomicAdd(a.gconf + ((long long)b * a.NV + v) * a.C + c0 + e, g[e] * x[e]);
                    }
                }
                scatter(v, dx);
            }
        }
    }
}

// K2: grid (tiles_x * tiles_y, NV, B), 4 waves; wave wv owns channels [wv * CW, (wv + 1) * CW) of the tile, CW = C / 4.
// LDS tile: HALVES half tiles of G_TW / HALVES pixel columns, [half][row][column][C + 8 floats] (+16 per row, +32 per half: the four taps
// of a voxel land in different banks).  With 4 * CW <= 32 lanes per hit (C <= 32) the two half-waves work on DIFFERENT hits at the same
// time -- half-wave 0 adds only taps in pixel columns 0-7, half-wave 1 only columns 8-15, each walking its own compact list of the
// brick's voxels that touch its half -- so no cell is ever addressed by both, and the per-cell order stays (brick, voxel).
constexpr int G_TW = 16, G_TH = 16;
constexpr int G_LIST = 256;      // candidate bricks per refill of the list

template <int CW>
struct GatherCfg {
    static constexpr int C = 4 * CW;
    static constexpr int HALVES = (4 * CW <= 32) ? 2 : 1;
    static constexpr int HPX = G_TW / HALVES;            // pixel columns per half
    static constexpr int PS = C + 8;                     // floats per pixel
    static constexpr int RSH = HPX * PS + 16;            // floats per row of a half
    static constexpr int HALF_SZ = G_TH * RSH + 32;
    static constexpr int TILE = HALVES * HALF_SZ;        // + 4 * 64 dummy cells (one per thread: where the adds of absent taps go)
    static constexpr int DW = CW < 4 ? 4 : CW;           // floats of dx per record (16-byte granules)
    static constexpr int REC = 4 + 4 + DW;               // ints per hit record: 4 cell byte offsets, 4 weights, the wave's dx channels
    static constexpr int WAVE_INTS = HALVES * 68 * REC;  // per half 64 records + one round of padding
    static constexpr size_t LDS = (size_t)(TILE + 256 + 4 * WAVE_INTS + G_LIST + 4) * 4;
};

// INDEXED (lt_unproject_indexed_bwd): grid (tiles, NV, F), a.B the cuboids of the chunk.  The workgroup of (tile, v, f) keeps its LDS tile across
// cuboids: it scans frame_of over the chunk in ascending p (a scalar per step, uniform over the workgroup) and runs the brick walk below over the
// tap records, bounding boxes and dxs of every cuboid of frame f, so a cell's additions are in (cuboid, brick, voxel) order; the tile is stored once
// at the end.  The first chunk (p0 == 0) starts from the zero fill, a later one from what the chunks before it stored in gfeats -- the same additions
// in the same order as one chunk over all cuboids, hence the same bits.  A frame without a cuboid stores zeros.  No LDS beyond the unindexed form's.
template <int CW, bool INDEXED = false>
__global__ __launch_bounds__(256) void unproj_gather_kernel(const std::conditional_t<INDEXED, UnprojBwdIndexedArgs, UnprojBwdArgs> a) {
    typedef GatherCfg<CW> G;
    constexpr int C = G::C, HALVES = G::HALVES, REC = G::REC;
    extern __shared__ float smem[];
    float* tile = smem;
    float* dummy = smem + G::TILE;                             // [256]
    int* wbase = (int*)(dummy + 256);
    int* list = wbase + 4 * G::WAVE_INTS;                      // [G_LIST] candidate bricks of this tile, ascending
    int* meta = list + G_LIST;                                 // count, next brick group
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int* myR = wbase + wv * G::WAVE_INTS;                      // [HALVES][68] hit records
    const int tiles_x = (a.w + G_TW - 1) / G_TW;
    const int tx0 = (blockIdx.x % tiles_x) * G_TW, ty0 = (blockIdx.x / tiles_x) * G_TH;
    const int v = blockIdx.y, b = blockIdx.z;                  // b: the sample whose tile this is (INDEXED: the frame)
    const int nbricks = a.nb0 * a.nb1 * a.nb2;
    const long long vbase = ((long long)b * a.NV + v) * a.nvox; // the workspace rows that are walked: sample b's (INDEXED: set per cuboid of the frame, below)
    const int* txy = a.txy + vbase;
    const float4* tw = a.tw + vbase;
    const float* dxs = a.dxs + vbase * C + wv * CW;
    const int* bbox = a.bbox + ((long long)b * a.NV + v) * nbricks * 4;
    for (int i = threadIdx.x; i < G::TILE; i += 256) tile[i] = 0.f;
    if constexpr (INDEXED) {
        if (a.p0 > 0) {                                        // a later chunk goes on from the sums of the chunks before it (the store loop, backwards)
            __syncthreads();
            const float* gsrc = a.gfeats + ((long long)b * a.NV + v) * a.h * a.w * C;
            for (int i = threadIdx.x; i < G_TH * G_TW * (C / 4); i += 256) {
                const int cv = i % (C / 4), px = (i / (C / 4)) % G_TW, py = i / ((C / 4) * G_TW);
                if (tx0 + px < a.w && ty0 + py < a.h) {
                    const int hh = px / G::HPX;
                    *(float4*)(tile + hh * G::HALF_SZ + py * G::RSH + (px - hh * G::HPX) * G::PS + cv * 4) =
                        *(const float4*)(gsrc + ((long long)(ty0 + py) * a.w + tx0 + px) * C + cv * 4);
                }
            }
        }
    }
    // this lane's role in the hit loop: half-wave `half`, pixel-parity class t_of (see the records), channel c_of (lanes past 4 * CW of a
    // half idle: they work on a dummy cell)
    const int half = HALVES == 2 ? lane >> 5 : 0, hl_lane = HALVES == 2 ? lane & 31 : lane;
    const int t_of = hl_lane / CW, c_of = hl_lane - t_of * CW;
    const bool adder = hl_lane < 4 * CW;
    // byte addresses (LDS) this lane works with: its channel inside a pixel's cell run, its dummy cell, its fields of record 0 of its half
    char* const cell_base = (char*)(tile + wv * CW + c_of);
    const int dummy_off = (int)((char*)(dummy + threadIdx.x) - cell_base);
    const char* const rec_c = (const char*)(myR + half * 68 * REC + (adder ? t_of : 0));
    const char* const rec_w = rec_c + 16;
    const char* const rec_d = (const char*)(myR + half * 68 * REC + 8 + (adder ? c_of : 0));
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    struct Req { long long vox; int xy; float4 w; float4 d[G::DW / 4]; };
    auto request = [&](int brick) {                            // this lane's voxel of `brick`: its tap record and this wave's dx channels
        Req r;
        r.vox = brick_voxel(a, brick, lane);
        const long long vx = r.vox >= 0 ? r.vox : 0;           // a lane past the grid's end reads voxel 0 and is masked later
        r.xy = txy[vx];
        r.w = tw[vx];
        const float* src = dxs + vx * C;
        if (CW >= 4) {
#pragma unroll
            for (int e = 0; e < CW / 4; ++e) r.d[e] = *(const float4*)(src + e * 4);
        } else {
            r.d[0] = make_float4(src[0], CW > 1 ? src[CW > 1 ? 1 : 0] : 0.f, 0.f, 0.f);
        }
        return r;
    };
    int q = -1;                                                // INDEXED: the chunk's cuboid that is walked; those of frame b, in ascending order
    do {
    if constexpr (INDEXED) {
        do ++q; while (q < a.B && frame_of_cuboid(a, a.p0 + q) != b);
        if (q >= a.B) break;
        const long long vb = ((long long)q * a.NV + v) * a.nvox;
        txy = a.txy + vb;
        tw = a.tw + vb;
        dxs = a.dxs + vb * C + wv * CW;
        bbox = a.bbox + ((long long)q * a.NV + v) * nbricks * 4;
    }
    int g_next = 0;
    while (g_next < nbricks) {
        // ---- wave 0 lists the next (up to G_LIST) bricks whose tap bounding box meets the tile, in brick order
        if (wv == 0) {
            int cnt = 0, g0 = g_next;
            while (g0 < nbricks && cnt <= G_LIST - 64) {
                bool cand = false;
                if (g0 + lane < nbricks) {
                    const int4 bb = *(const int4*)(bbox + (long long)(g0 + lane) * 4);
                    cand = bb.x <= bb.y && bb.y >= tx0 && bb.x < tx0 + G_TW && bb.w >= ty0 && bb.z < ty0 + G_TH;
                }
                const unsigned long long m = __ballot(cand);
                if (cand) list[cnt + __popcll(m & lt_mask)] = g0 + lane;
                cnt += __popcll(m);
                g0 += 64;
            }
            if (lane == 0) { meta[0] = cnt; meta[1] = g0; }
        }
        __syncthreads();                                       // (also orders the tile's zero fill in front of the first additions)
        const int cnt = meta[0];
        g_next = meta[1];
        // ---- every wave walks the list (its own channels): brick i + 1's tap records and dx values are in flight while brick i is added
        Req nxt;
        if (cnt > 0) nxt = request(list[0]);
        for (int i = 0; i < cnt; ++i) {
            const Req cur = nxt;
            if (i + 1 < cnt) nxt = request(list[i + 1]);
            // the voxel's taps that fall into this tile: byte offset of the pixel's cell run (relative to the tile), per half
            int L[2][4] = {{-1, -1, -1, -1}, {-1, -1, -1, -1}};
            bool hit[2] = {false, false};
            const float Wt[4] = {cur.w.x, cur.w.y, cur.w.z, cur.w.w};
            if (cur.vox >= 0) {
                const int lx0 = (cur.xy & 0xffff) - 1 - tx0, ly0 = (cur.xy >> 16) - 1 - ty0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int lx = lx0 + (k & 1), ly = ly0 + (k >> 1);
                    if (Wt[k] != 0.f && lx >= 0 && lx < G_TW && ly >= 0 && ly < G_TH) {
                        const int hh = HALVES == 2 ? lx >> 3 : 0;
                        const int off = (hh * G::HALF_SZ + ly * G::RSH + (lx - hh * G::HPX) * G::PS) * 4;
                        if (hh == 0) { L[0][k] = off; hit[0] = true; } else { L[1][k] = off; hit[1] = true; }
                    }
                }
            }
            const unsigned long long m0 = __ballot(hit[0]), m1 = HALVES == 2 ? __ballot(hit[1]) : 0ull;
            if (!(m0 | m1)) continue;
            const int n0 = __popcll(m0), n1 = __popcll(m1);
            // record slots are PIXEL PARITY classes, not tap numbers: slot s holds the tap whose pixel has (x & 1) + 2 (y & 1) == s, i.e.
            // tap k = s ^ parity(origin).  The four taps of a voxel always have four different parities, and lane group s of the hit loop
            // then owns every cell of parity s -- a pixel reached as tap 0 of one voxel and tap 1 of the next is updated by the SAME lane,
            // so the read-add-write below needs no atomics (the tile origin is a multiple of 16: tile-relative parity = map parity)
            float Ws[4];
            {
                const int lx0 = (cur.xy & 0xffff) - 1, ly0 = (cur.xy >> 16) - 1;
                const bool p1 = lx0 & 1, p2 = ly0 & 1;
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    const int t0 = p1 ? L[hh][1] : L[hh][0], t1 = p1 ? L[hh][0] : L[hh][1], t2 = p1 ? L[hh][3] : L[hh][2], t3 = p1 ? L[hh][2] : L[hh][3];
                    L[hh][0] = p2 ? t2 : t0; L[hh][1] = p2 ? t3 : t1; L[hh][2] = p2 ? t0 : t2; L[hh][3] = p2 ? t1 : t3;
                }
                const float t0 = p1 ? Wt[1] : Wt[0], t1 = p1 ? Wt[0] : Wt[1], t2 = p1 ? Wt[3] : Wt[2], t3 = p1 ? Wt[2] : Wt[3];
                Ws[0] = p2 ? t2 : t0; Ws[1] = p2 ? t3 : t1; Ws[2] = p2 ? t0 : t2; Ws[3] = p2 ? t1 : t3;
            }
            // compact hit records per half, in voxel order: [4 cell offsets | 4 weights | dx of this wave's channels].  Same-wave LDS traffic: a wave's LDS queue is in order, the fences stop the compiler
#pragma unroll
            for (int hh = 0; hh < HALVES; ++hh) {
                const unsigned long long m = hh == 0 ? m0 : m1;
                int* rb = myR + hh * 68 * REC;
                if (hit[hh]) {
                    int* r = rb + __popcll(m & lt_mask) * REC;
                    *(int4*)r = make_int4(L[hh][0], L[hh][1], L[hh][2], L[hh][3]);
                    *(float4*)(r + 4) = make_float4(Ws[0], Ws[1], Ws[2], Ws[3]);
#pragma unroll
                    for (int e = 0; e < G::DW / 4; ++e) *(float4*)(r + 8 + e * 4) = cur.d[e];
                }
            }
            const int nmax = HALVES == 2 ? max(n0, n1) : n0;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // rounds of four hits: twelve independent record reads, four cell reads, the sums (forwarded in registers where two hits of
            // the round meet in one cell), four cell writes in hit order.  A half with fewer hits re-reads stale / empty records into its
            // dummy cell (records past its count are never trusted: the count test below)
            const int my_n = half == 0 ? n0 : n1;
            for (int r0 = 0; r0 < nmax; r0 += 4) {
                int off[4];
                float x[4], cv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int ro = (r0 + j) * REC * 4;
                    const int cell = *(const int*)(rec_c + ro);
                    const float wt = *(const float*)(rec_w + ro), dv = *(const float*)(rec_d + ro);
                    const bool ok = adder && cell >= 0 && r0 + j < my_n;
                    off[j] = ok ? cell : dummy_off;
                    x[j] = wt * dv;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) cv[j] = *(const float*)(cell_base + off[j]);
                const float a0 = cv[0] + x[0];
                const float a1 = (off[1] == off[0] ? a0 : cv[1]) + x[1];
                const float a2 = (off[2] == off[1] ? a1 : (off[2] == off[0] ? a0 : cv[2])) + x[2];
                const float a3 = (off[3] == off[2] ? a2 : (off[3] == off[1] ? a1 : (off[3] == off[0] ? a0 : cv[3]))) + x[3];
                *(float*)(cell_base + off[0]) = a0;
                *(float*)(cell_base + off[1]) = a1;
                *(float*)(cell_base + off[2]) = a2;
                *(float*)(cell_base + off[3]) = a3;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        __syncthreads();                                       // the list is free to be rewritten; after the last round: the tile is complete
    }
    } while (INDEXED);
    if constexpr (INDEXED) __syncthreads();                    // a frame without a cuboid in this chunk walked nothing: its fill is ordered here
    // the tile's pixels inside the map, every channel: plain stores, each cell of gfeats written exactly once
    float* gm = a.gfeats + ((long long)b * a.NV + v) * a.h * a.w * C;
    constexpr int c4 = C / 4;
    for (int i = threadIdx.x; i < G_TH * G_TW * c4; i += 256) {
        const int cv = i % c4, px = (i / c4) % G_TW, py = i / (c4 * G_TW);
        if (tx0 + px < a.w && ty0 + py < a.h) {
            const int hh = px / G::HPX;
            *(float4*)(gm + ((long long)(ty0 + py) * a.w + tx0 + px) * C + cv * 4) =
                *(const float4*)(tile + hh * G::HALF_SZ + py * G::RSH + (px - hh * G::HPX) * G::PS + cv * 4);
        }
    }
}

// K2 of one chunk: one workgroup per (tile, view, sample of the chunk); INDEXED: per (tile, view, FRAME), over the m.B cuboids of the chunk.  The
// unindexed kernel receives a plain UnprojBwdArgs by value (the base of m), as in launch_taps_dx.
template <int CW, bool INDEXED>
int launch_gather(const UnprojBwdIndexedArgs& m, int tiles, hipStream_t st) {
    const std::conditional_t<INDEXED, UnprojBwdIndexedArgs, UnprojBwdArgs>& c = m;
    LT_OPT_IN_LDS((unproj_gather_kernel<CW, INDEXED>), 160 * 1024);
    hipLaunchKernelGGL((unproj_gather_kernel<CW, INDEXED>), dim3((unsigned)tiles, (unsigned)m.NV, (unsigned)(INDEXED ? m.F : m.B)), dim3(256), GatherCfg<CW>::LDS, st, c);
    LT_CHECK_LAUNCH(INDEXED ? "lt_unproject_indexed_bwd(gather)" : "lt_unproject_bwd(gather)");
    return LT_OK;
}
template <bool INDEXED>
int launch_gather_c(const UnprojBwdIndexedArgs& m, int tiles, hipStream_t st) {
    switch (m.C / 4) {                                            // K2 as it is: a masked view has no brick to walk and stores zeros
        case 1: return launch_gather<1, INDEXED>(m, tiles, st);
        case 2: return launch_gather<2, INDEXED>(m, tiles, st);
        case 4: return launch_gather<4, INDEXED>(m, tiles, st);
        case 8: return launch_gather<8, INDEXED>(m, tiles, st);
        default: return launch_gather<16, INDEXED>(m, tiles, st);
    }
}

int blocks_k1(long long nvox, int C) {
    const long long blocks = cdiv(nvox * (C / 4), 256);
    return (int)(blocks < 2048 ? blocks : 2048);
}

bool gather_takes(int C) { return C >= 4 && C <= 64 && (C & (C - 1)) == 0 && !env_on("LT_UNPROJ_BWD_ATOMICS"); }

size_t align256(size_t v) { return (v + 255) / 256 * 256; }

// K0, K1 and the confidence finalizers of one chunk of the batch.  An unmasked kernel receives a plain UnprojBwdArgs by value (the base of m)
// and a masked one its masked base: the unmasked kernels keep their argument block, and with it their code.  INDEXED: all of m, c.B cuboids of one
// chunk, and no finalizer -- the indexed entry runs its own once, after the last chunk.
template <bool MASKED, bool INDEXED = false>
int launch_taps_dx(const char* who, const UnprojBwdIndexedArgs& m, int dtype, int nbricks, int nblk1, hipStream_t st) {
    const UnprojBwdArgsOf<MASKED, INDEXED>& c = m;
    const int nb = c.B, NV = c.NV, C = c.C, agg = c.agg;
    hipLaunchKernelGGL((unproj_taps_kernel<MASKED, INDEXED>), dim3((unsigned)cdiv(nbricks, 4), (unsigned)nb), dim3(256), 0, st, c);
    LT_CHECK_LAUNCH(who);
    const dim3 g1((unsigned)nblk1, (unsigned)nb);
    if (NV > UB_MAXV) {                                       // views in passes (softmax, max) or in groups of UB_MAXV (grid z)
        const dim3 gz((unsigned)nblk1, (unsigned)nb, (unsigned)cdiv(NV, UB_MAXV));
        if (agg == LT_AGG_SOFTMAX || agg == LT_AGG_MAX) {
            if (dtype == LT_F32) hipLaunchKernelGGL((unproj_dx_passes_kernel<float, MASKED, INDEXED>), g1, dim3(256), 0, st, c);
            else hipLaunchKernelGGL((unproj_dx_passes_kernel<bf16_t, MASKED, INDEXED>), g1, dim3(256), 0, st, c);
        } else if (dtype == LT_F32) hipLaunchKernelGGL((unproj_dx_groups_kernel<float, MASKED, INDEXED>), gz, dim3(256), 0, st, c);
        else hipLaunchKernelGGL((unproj_dx_groups_kernel<bf16_t, MASKED, INDEXED>), gz, dim3(256), 0, st, c);
    } else if (dtype == LT_F32) {
        if (NV <= 4) hipLaunchKernelGGL((unproj_dx_kernel<float, 4, MASKED, INDEXED>), g1, dim3(256), 0, st, c);
        else hipLaunchKernelGGL((unproj_dx_kernel<float, UB_MAXV, MASKED, INDEXED>), g1, dim3(256), 0, st, c);
    } else {
        if (NV <= 4) hipLaunchKernelGGL((unproj_dx_kernel<bf16_t, 4, MASKED, INDEXED>), g1, dim3(256), 0, st, c);
        else hipLaunchKernelGGL((unproj_dx_kernel<bf16_t, UB_MAXV, MASKED, INDEXED>), g1, dim3(256), 0, st, c);
    }
    LT_CHECK_LAUNCH(who);
    if constexpr (!INDEXED) {
        if (c.gconf && NV > UB_MAXV) {
            hipLaunchKernelGGL(unproj_gconf_finalize_many_kernel<MASKED>, dim3((unsigned)(nb * (C / (C < UB_FIN_C ? C : UB_FIN_C)))), dim3(UB_MANYV * UB_FIN_C), 0, st, c, nblk1);
            LT_CHECK_LAUNCH(who);
        } else if (c.gconf) {
            hipLaunchKernelGGL(unproj_gconf_finalize_kernel<MASKED>, dim3((unsigned)cdiv((long long)nb * C, 64)), dim3(64), 0, st, c, nblk1);
            LT_CHECK_LAUNCH(who);
        }
    }
    return LT_OK;
}

// The gather's workspace, both layouts (their byte counts: include/lt_hip.h); bytes = fixed + per_item * the items walked at once:
//   plain, masked  [dxs | bbox | gcpart | tw | txy], each block one chunk of samples long: a sample's share includes its fp64 confidence partials,
//                  which are finalized per chunk
//   indexed        [gcpart of ALL P cuboids, dense (P, nblk1, NV, C), rounded up to 256 in all][dxs | bbox | tw | txy], each block one chunk of cuboids
//                  long: the finalizer runs once, over every chunk's partials
struct BwdWs {
    size_t s_dx, s_bb, s_gc, s_xy, s_tw;                          // one item's blocks, each rounded up to 256
    size_t fixed, per_item;
    int nblk1;
};
BwdWs bwd_ws(bool indexed, int P, int NV, int C, int v0, int v1, int v2) {
    const long long nvox = (long long)v0 * v1 * v2;
    const long long nbricks = cdiv(v0, 4) * cdiv(v1, 4) * cdiv(v2, 4);
    BwdWs s;
    s.nblk1 = blocks_k1(nvox, C);
    const size_t gc = (size_t)s.nblk1 * NV * C * 8;              // one item's partials
    s.s_dx = align256((size_t)NV * nvox * C * 4); s.s_bb = align256((size_t)NV * nbricks * 16); s.s_gc = align256(gc);
    s.s_xy = align256((size_t)NV * nvox * 4); s.s_tw = align256((size_t)NV * nvox * 16);
    s.fixed = indexed ? align256(gc * (size_t)P) : 0;
    s.per_item = s.s_dx + s.s_bb + s.s_xy + s.s_tw + (indexed ? 0 : s.s_gc);
    return s;
}
// the three workspace queries: 0 where there is nothing to walk or the gather does not take C
size_t bwd_ws_bytes(bool indexed, int P, int items, int NV, int C, int v0, int v1, int v2) {
    if (P < 1 || items < 1 || NV < 1 || C < 4 || v0 < 1 || v1 < 1 || v2 < 1 || !gather_takes(C)) return 0;
    const BwdWs s = bwd_ws(indexed, P, NV, C, v0, v1, v2);
    return s.fixed + s.per_item * (size_t)(items < P ? items : P);
}

// The one body behind lt_unproject_desc_bwd and its three shorthands: `who` is the entry that was called.  d.frame_of set: the indexed walk (d.B cuboids
// over d.F frames, on the nullable-mask instantiations); else d.view_mask set: the masked instantiations; else the plain ones, on their own argument block.
int unproject_backward(const char* who, const lt_unproject_desc& d, const float* grad_out, float* grad_feats, float* grad_conf, void* workspace,
                       size_t workspace_bytes, void* stream) {
    const bool indexed = d.frame_of != nullptr, masked = !indexed && d.view_mask;
    const char* const form = indexed ? "indexed" : "masked";      // the variants the scatter does not have, and what each takes
    const char* const takes = indexed ? "frame index" : "view mask";
    const float* coords = d.coords ? d.coords : d.coords_out;     // grid form: the voxel centres its forward wrote
    const int dtype = d.dtype, B = d.B, NV = d.NV, C = d.C, h = d.h, w = d.w, agg = d.agg;
    LT_REQUIRE(!d.view_base, LT_ERR_UNSUPPORTED, "%s: view_base has no backward (a ragged batch is inference only)", who);
    LT_REQUIRE(!(d.coords && (d.pos || d.center || d.rot || d.coords_out)), LT_ERR_INVALID, "%s: both coords and the cuboid (pos, center, rot, coords_out) are set", who);
    LT_REQUIRE(d.feats && d.proj && coords && grad_out && grad_feats, LT_ERR_INVALID, "%s: null argument", who);
    LT_REQUIRE(!indexed || (d.F >= 1 && B >= 1), LT_ERR_INVALID, "%s: needs F >= 1 frames and P >= 1 cuboids (got F=%d P=%d)", who, d.F, B);
    LT_REQUIRE(dtype == LT_F32 || dtype == LT_BF16, LT_ERR_INVALID, "%s: bad dtype %d", who, dtype);
    LT_REQUIRE(agg == LT_AGG_SUM || agg == LT_AGG_MAX || agg == LT_AGG_SOFTMAX || agg == LT_AGG_CONF || agg == LT_AGG_CONF_NORM, LT_ERR_UNSUPPORTED,
               "%s: unknown aggregation %d", who, agg);
    const bool is_conf = agg == LT_AGG_CONF || agg == LT_AGG_CONF_NORM;
    LT_REQUIRE(!is_conf || d.conf, LT_ERR_INVALID, "%s: the conf aggregations need confidences", who);
    LT_REQUIRE(B >= 1 && NV >= 1 && NV <= UB_MANYV && C >= 4 && C % 4 == 0 && h >= 2 && w >= 2 && d.v0 >= 1 && d.v1 >= 1 && d.v2 >= 1, LT_ERR_UNSUPPORTED,
               "%s: needs 1 <= NV <= %d and C %% 4 == 0 (got NV=%d C=%d)", who, UB_MANYV, NV, C);
    LT_REQUIRE((long long)NV * h * w * C < (1ll << 31), LT_ERR_UNSUPPORTED, "%s: feature maps too large", who);
    LT_REQUIRE(!indexed || d.F <= 65535, LT_ERR_UNSUPPORTED, "%s: at most 65535 frames (the gather's grid), got %d", who, d.F);
    if (indexed || masked) {                                      // there is no masked and no indexed scatter
        LT_REQUIRE(!env_on("LT_UNPROJ_BWD_ATOMICS"), LT_ERR_UNSUPPORTED,
                   "%s: LT_UNPROJ_BWD_ATOMICS selects the scatter path, which has no %s form (only the gather takes a %s)", who, form, takes);
        LT_REQUIRE(gather_takes(C), LT_ERR_UNSUPPORTED,
                   "%s: only the gather path takes a %s, and it needs C a power of two <= 64 (got C=%d; the scatter has no %s form)", who, takes, C, form);
    }
    hipStream_t st = (hipStream_t)stream;
    UnprojBwdIndexedArgs a;
    a.frame_of = d.frame_of; a.F = indexed ? d.F : B; a.P = B; a.p0 = 0;
    a.mask = d.view_mask;
    a.feats = d.feats; a.proj = d.proj; a.coords = coords; a.conf = d.conf; a.gout = grad_out; a.gfeats = grad_feats; a.gconf = is_conf ? grad_conf : nullptr;
    a.dxs = nullptr; a.bbox = nullptr; a.gcpart = nullptr; a.txy = nullptr; a.tw = nullptr;
    a.B = B; a.NV = NV; a.C = C; a.h = h; a.w = w; a.agg = agg;
    a.v0 = d.v0; a.v1 = d.v1; a.v2 = d.v2; a.nb0 = (int)cdiv(d.v0, 4); a.nb1 = (int)cdiv(d.v1, 4); a.nb2 = (int)cdiv(d.v2, 4);
    a.nvox = (long long)d.v0 * d.v1 * d.v2;
    if (!gather_takes(C)) {
        // round-2 scatter: global float atomics into zeroed buffers (not bitwise repeatable); the plain variant only (refused above otherwise)
        const UnprojBwdArgs& u = a;
        LT_REQUIRE(agg != LT_AGG_CONF_NORM, LT_ERR_UNSUPPORTED, "%s: conf_norm needs the gather path (C a power of two <= 64)", who);
        LT_REQUIRE(hipMemsetAsync(grad_feats, 0, (size_t)B * NV * h * w * C * 4, st) == hipSuccess, LT_ERR_LAUNCH, "%s: hipMemsetAsync failed", who);
        if (a.gconf) LT_REQUIRE(hipMemsetAsync(a.gconf, 0, (size_t)B * NV * C * 4, st) == hipSuccess, LT_ERR_LAUNCH, "%s: hipMemsetAsync failed", who);
        const long long blocks = cdiv(a.nvox * (C / 4), 256);
        dim3 grid((unsigned)(blocks < 65536 ? blocks : 65536), (unsigned)B);
        if (NV > UB_MAXV) {
            if (dtype == LT_F32) hipLaunchKernelGGL(unproject_bwd_many_kernel<float>, grid, dim3(256), 0, st, u);
            else hipLaunchKernelGGL(unproject_bwd_many_kernel<bf16_t>, grid, dim3(256), 0, st, u);
        } else if (dtype == LT_F32) hipLaunchKernelGGL(unproject_bwd_kernel<float>, grid, dim3(256), 0, st, u);
        else hipLaunchKernelGGL(unproject_bwd_kernel<bf16_t>, grid, dim3(256), 0, st, u);
        LT_CHECK_LAUNCH("lt_unproject_bwd(scatter)");
        return LT_OK;
    }
    const int nbricks = a.nb0 * a.nb1 * a.nb2;
    const BwdWs s = bwd_ws(indexed, B, NV, C, d.v0, d.v1, d.v2);
    const bool ws_ok = workspace && workspace_bytes >= s.fixed + s.per_item && ((size_t)workspace % 16) == 0;
    if (indexed)
        LT_REQUIRE(ws_ok, LT_ERR_INVALID,
                   "%s: workspace of at least %zu bytes (the confidence partials of all %d cuboids and one cuboid's share of the rest; "
                   "lt_unproject_indexed_bwd_workspace for all cuboids at once), 16-byte aligned", who, s.fixed + s.per_item, B);
    LT_REQUIRE(ws_ok, LT_ERR_INVALID, "%s: workspace of at least %zu bytes (one sample; lt_unproject_bwd_workspace for the whole batch), 16-byte aligned", who,
               s.per_item);
    const size_t fit = (workspace_bytes - s.fixed) / s.per_item;
    const size_t cap = indexed && B > 65535 ? 65535 : (size_t)B;  // indexed: K0 and K1 take the chunk's cuboids as grid y
    const int chunk = (int)(fit < cap ? fit : cap);
    const int tiles = (int)(cdiv(w, G_TW) * cdiv(h, G_TH));
    const size_t in_elt = dtype == LT_F32 ? 4 : 2;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = B - b0 < chunk ? B - b0 : chunk;
        UnprojBwdIndexedArgs c = a;
        c.B = nb;
        c.coords = coords + (size_t)b0 * a.nvox * 3;
        c.gout = grad_out + (size_t)b0 * a.nvox * C;
        char* wsp = (char*)workspace + s.fixed;
        c.dxs = (float*)wsp; wsp += s.s_dx * nb;
        c.bbox = (int*)wsp; wsp += s.s_bb * nb;
        if (indexed) {                                            // the frame side stays whole: the kernels reach it through frame_of[p0 + b]
            c.p0 = b0;
            c.gcpart = (double*)workspace + (size_t)b0 * s.nblk1 * NV * C;
        } else {
            c.feats = (const char*)d.feats + (size_t)b0 * NV * h * w * C * in_elt;
            c.proj = d.proj + (size_t)b0 * NV * 12;
            c.conf = d.conf ? d.conf + (size_t)b0 * NV * C : nullptr;
            c.mask = a.mask ? a.mask + (size_t)b0 * NV : nullptr;
            c.gfeats = grad_feats + (size_t)b0 * NV * h * w * C;
            c.gconf = a.gconf ? a.gconf + (size_t)b0 * NV * C : nullptr;
            c.gcpart = (double*)wsp; wsp += s.s_gc * nb;
        }
        c.tw = (float4*)wsp; wsp += s.s_tw * nb;
        c.txy = (int*)wsp;
        int rc = indexed  ? launch_taps_dx<true, true>(who, c, dtype, nbricks, s.nblk1, st)
                 : masked ? launch_taps_dx<true>(who, c, dtype, nbricks, s.nblk1, st)
                          : launch_taps_dx<false>(who, c, dtype, nbricks, s.nblk1, st);
        if (rc != LT_OK) return rc;
        rc = indexed ? launch_gather_c<true>(c, tiles, st) : launch_gather_c<false>(c, tiles, st);
        if (rc != LT_OK) return rc;
    }
    if (indexed && a.gconf) {
        UnprojBwdIndexedArgs c = a;
        c.gcpart = (double*)workspace;
        hipLaunchKernelGGL(unproj_gconf_finalize_indexed_kernel, dim3((unsigned)(d.F * (C / (C < UB_FIN_C ? C : UB_FIN_C)))), dim3(UB_MANYV * UB_FIN_C), 0, st, c, s.nblk1);
        LT_CHECK_LAUNCH(who);
    }
    return LT_OK;
}

}  // namespace

extern "C" size_t lt_unproject_desc_bwd_workspace(const lt_unproject_desc* d, int32_t items) {
    if (!d || d->view_base) return 0;
    return bwd_ws_bytes(d->frame_of != nullptr, d->B, items, d->NV, d->C, d->v0, d->v1, d->v2);
}

extern "C" int lt_unproject_desc_bwd(const lt_unproject_desc* desc, const float* grad_out, float* grad_feats, float* grad_conf, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    LT_REQUIRE(desc, LT_ERR_INVALID, "lt_unproject_desc_bwd: null descriptor");
    return unproject_backward("lt_unproject_desc_bwd", *desc, grad_out, grad_feats, grad_conf, workspace, workspace_bytes, stream);
}

// bytes for ALL B samples at once; lt_unproject_bwd walks the batch in chunks when it is handed less (at least one sample's worth)
extern "C" size_t lt_unproject_bwd_workspace(int32_t B, int32_t NV, int32_t C, int32_t v0, int32_t v1, int32_t v2) {
    return bwd_ws_bytes(false, B, B, NV, C, v0, v1, v2);
}

extern "C" size_t lt_unproject_indexed_bwd_workspace(int32_t P, int32_t NV, int32_t C, int32_t v0, int32_t v1, int32_t v2) {
    return bwd_ws_bytes(true, P, P, NV, C, v0, v1, v2);
}

extern "C" int lt_unproject_bwd(int32_t dtype, const void* feats, const float* proj, const float* coords, const float* conf, const float* grad_out,
                                float* grad_feats, float* grad_conf, int32_t B, int32_t NV, int32_t C, int32_t h, int32_t w, int32_t v0, int32_t v1,
                                int32_t v2, int32_t agg, void* workspace, size_t workspace_bytes, void* stream) {
    return unproject_backward("lt_unproject_bwd", unproject_coord_desc(dtype, feats, proj, coords, conf, B, NV, C, h, w, v0, v1, v2, agg), grad_out, grad_feats, grad_conf,
                              workspace, workspace_bytes, stream);
}

extern "C" int lt_unproject_masked_bwd(int32_t dtype, const void* feats, const float* proj, const float* coords, const float* conf, const uint8_t* view_mask,
                                       const float* grad_out, float* grad_feats, float* grad_conf, int32_t B, int32_t NV, int32_t C, int32_t h, int32_t w,
                                       int32_t v0, int32_t v1, int32_t v2, int32_t agg, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "lt_unproject_masked_bwd";
    LT_REQUIRE(view_mask, LT_ERR_INVALID, "%s: null view_mask", who);
    lt_unproject_desc d = unproject_coord_desc(dtype, feats, proj, coords, conf, B, NV, C, h, w, v0, v1, v2, agg);
    d.view_mask = view_mask;
    return unproject_backward(who, d, grad_out, grad_feats, grad_conf, workspace, workspace_bytes, stream);
}

extern "C" int lt_unproject_indexed_bwd(int32_t dtype, const void* feats, const float* proj, const float* coords, const float* conf, const uint8_t* view_mask,
                                        const int32_t* frame_of, const float* grad_out, float* grad_feats, float* grad_conf, int32_t F, int32_t P, int32_t NV,
                                        int32_t C, int32_t h, int32_t w, int32_t v0, int32_t v1, int32_t v2, int32_t agg, void* workspace, size_t workspace_bytes,
                                        void* stream) {
    const char* who = "lt_unproject_indexed_bwd";
    LT_REQUIRE(frame_of, LT_ERR_INVALID, "%s: null frame_of", who);
    lt_unproject_desc d = unproject_coord_desc(dtype, feats, proj, coords, conf, P, NV, C, h, w, v0, v1, v2, agg);
    d.view_mask = view_mask; d.frame_of = frame_of; d.F = F;
    return unproject_backward(who, d, grad_out, grad_feats, grad_conf, workspace, workspace_bytes, stream);
}
