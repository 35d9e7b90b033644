// Voxel-grid construction and the fused unprojection (projective bilinear gather + view aggregation).
//
// Unprojection is HBM/L2-bound: per sample it must read the NV feature maps once and write the
// C x V^3 volume once (38.27 MB fp32 at config 2); everything else (projection,
// 4-tap weights, view softmax) lives in registers.  Layout choices that make it stream:
//   * feature maps are channels-last, so ONE bilinear tap of ONE voxel is a contiguous C-vector
//     (128 B fp32 / 64 B bf16 at C=32): the C/CH lanes of a voxel issue one coalesced 16-byte load each;
//   * the volume is written channels-last too (what the V2V implicit GEMM wants): 16 B per lane, a
//     brick's 16 consecutive voxels form one 2 KiB run;
//   * a workgroup owns a 4x4x16 voxel brick: its projection into every view is a ~10-px patch that
//     stays L1/L2 resident across the brick's 1024 taps per view (8x reuse);
//   * with B % 8 == 0, sample b is processed only by workgroups dispatched to XCD b % 8, so a sample's
//     feature maps occupy one private L2 instead of being replicated into all eight.
#include <stdlib.h>

#include <type_traits>

#include "unproj_geom.h"
#include "wave_prims.h"

using namespace lt;

namespace {

// One voxel centre of the (rotated, optionally CMU-permuted) cuboid grid: the loop body of triangulation.py:298-339, fp32 in the
// reference's operation order (bit-exact in eval mode).  Shared by coord_volumes_kernel and the fused unprojection below.
__device__ __forceinline__ void voxel_coord(const float* __restrict__ p, const float* __restrict__ c, const float* __restrict__ R, float step,
                                            int i, int j, int k, int V, int cmu, float& o0, float& o1, float& o2) {
    // triangulation.py:336-339: permute(0,2,1,3) then flip axis 1  ==> out[i][j][k] = cv[i][k][V-1-j]
    const int a0 = i, a1 = cmu ? k : j, a2 = cmu ? (V - 1 - j) : k;
    // f32(position) + f32(step) * idx, two roundings as in triangulation.py:311-313 (no FMA contraction)
    const float x0 = __fadd_rn(p[0], __fmul_rn(step, (float)a0));
    const float x1 = __fadd_rn(p[1], __fmul_rn(step, (float)a1));
    const float x2 = __fadd_rn(p[2], __fmul_rn(step, (float)a2));
    const float d0 = __fsub_rn(x0, c[0]), d1 = __fsub_rn(x1, c[1]), d2 = __fsub_rn(x2, c[2]);
    // rot.mm(d): k-ordered multiply-adds (exact for theta = 0, where R is the identity)
    const float r0 = fmaf(R[2], d2, fmaf(R[1], d1, __fmul_rn(R[0], d0)));
    const float r1 = fmaf(R[5], d2, fmaf(R[4], d1, __fmul_rn(R[3], d0)));
    const float r2 = fmaf(R[8], d2, fmaf(R[7], d1, __fmul_rn(R[6], d0)));
    o0 = __fadd_rn(r0, c[0]);
    o1 = __fadd_rn(r1, c[1]);
    o2 = __fadd_rn(r2, c[2]);
}

__global__ void coord_volumes_kernel(const float* __restrict__ pos, const float* __restrict__ center,
                                     const float* __restrict__ rot, float step, int B, int V, int cmu, float* __restrict__ out) {
    const long long total = (long long)B * V * V * V;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
        long long r = g;
        const int k = (int)(r % V); r /= V;
        const int j = (int)(r % V); r /= V;
        const int i = (int)(r % V);
        const int b = (int)(r / V);
        float* o = out + g * 3;
        voxel_coord(pos + 3 * b, center + 3 * b, rot + 9 * b, step, i, j, k, V, cmu, o[0], o[1], o[2]);
    }
}

struct UnprojArgs {
    const void* feats;
    const float* proj;
    const float* coords;
    const float* conf;
    void* out;
    int B, NV, C, h, w, v0, v1, v2, agg;
    int bricked;        // 4x4x16 bricks (v0%4 == v1%4 == v2%16 == 0) or linear 256-voxel chunks
    int blocked;        // bricks walked in 32^3-voxel super-blocks (8 x 8 x 2 bricks) instead of in raster order -- see brick_of()
    int chunks;         // workgroups per sample
    int xcd_pin;        // B % 8 == 0
    // lt_unproject_grid_fwd: the voxel centres are COMPUTED (voxel_coord) from the cuboid description instead of read, and written to
    // coords_out when that is not null (the coordinate volume is a returned tensor of the forward: written once, never read back)
    const float* g_pos; const float* g_center; const float* g_rot;
    float g_step; int g_cmu; float* coords_out;
};
// the masked entries' kernels get the mask behind the same arguments; the unmasked kernels keep UnprojArgs as their whole argument block
struct UnprojMaskedArgs : UnprojArgs {
    const uint8_t* mask;  // (B, NV), non-zero = the view is valid
};
// the indexed entries' kernels (several cuboids per frame): B counts the CUBOIDS; coords, coords_out, out and g_* are indexed by the cuboid p,
// feats, proj, conf and mask by its frame frame_of[p] < F.  Built on the masked form: a null mask there means every view is valid.
struct UnprojIndexedArgs : UnprojMaskedArgs {
    const int32_t* frame_of;  // (B) the frame of every cuboid
    int F;                    // frames
};
// the ragged entries' kernels (samples with different view counts): feats, proj and conf are (T, ...) over all views, sample-major; sample b's NV is
// view_base[b + 1] - view_base[b] <= the NV of the arguments (NVcap) and its rows start at view_base[b].  Built on the masked form: the valid views are
// the prefix.  It is also the host's whole argument record (mask, frame_of and view_base are exclusive), which every kernel gets its base of.
struct UnprojRaggedArgs : UnprojIndexedArgs {
    const int32_t* view_base;  // (B + 1) exclusive prefix sum of the view counts
    int T;                     // rows of feats, proj and conf
};
template <bool MASKED, bool INDEXED = false, bool RAGGED = false>
using UnprojArgsOf = std::conditional_t<RAGGED, UnprojRaggedArgs, std::conditional_t<INDEXED, UnprojIndexedArgs, std::conditional_t<MASKED, UnprojMaskedArgs, UnprojArgs>>>;

// Brick (bi, bj, bk) of chunk c of a sample.  Raster order (k fastest) makes every 4-voxel i-slab of bricks sweep the WHOLE projected cube in every view:
// at 8 views the per-slab working set (2.7 MB of feature rows) plus the output stream does not fit the 4 MB L2 of the XCD the sample is pinned to, and the
// next slab -- which projects 2 pixels next to this one -- finds its rows evicted: PMC traffic 1.33 x the algorithmic bytes at BASELINE config 4 (rounds 4-5,
// unexplained there).  Blocked order (round 6): consecutive chunks fill one 32^3-voxel super-block (8 x 8 x 2 bricks = 128 workgroups, about what one XCD
// runs at a time), whose footprint is ~20 x 20 pixels per view; a pixel row is re-read once per super-block along the view's depth direction instead of
// once per slab.  Per-voxel arithmetic is untouched: results are bit-identical.  Measured at config 4, 16 samples (live PMC, profiles/r06_ab_unproject_brick_order.log):
// 3.48 -> 2.80 GB per launch = 1.33 -> 1.07 x the algorithmic 2.63 GB; the kernel's TIME does not move (3.62-3.67 ms either way: it is issue-bound, not
// traffic-bound); config 2 (4 views: 2.4 MB of maps, they fit): 1.10 -> 1.07 ms.
__device__ __forceinline__ void brick_of(const UnprojArgs& a, int chunk, int& bi, int& bj, int& bk) {
    const int nk = a.v2 >> 4, nj = a.v1 >> 2;
    if (a.blocked) {
        const int g = chunk >> 7, l = chunk & 127;
        const int ngk = nk >> 1, ngj = nj >> 3;
        const int gk = g % ngk, gj = (g / ngk) % ngj, gi = g / (ngk * ngj);
        bk = (gk * 2 + (l & 1)) << 4;
        bj = (gj * 8 + ((l >> 1) & 7)) << 2;
        bi = (gi * 8 + (l >> 4)) << 2;
    } else {
        bk = (chunk % nk) << 4;
        bj = ((chunk / nk) % nj) << 2;
        bi = (chunk / (nk * nj)) << 2;
    }
}

// workgroup -> (sample, chunk); XCD-pinned when B % 8 == 0 (block b runs on XCD b % 8)
__device__ __forceinline__ void sample_chunk_of(const UnprojArgs& a, int& b, int& chunk) {
    if (a.xcd_pin) {
        const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
        b = xcd + 8 * (j / a.chunks);
        chunk = j % a.chunks;
    } else {
        b = blockIdx.x / a.chunks;
        chunk = blockIdx.x % a.chunks;
    }
}

// The frame of cuboid p: uniform over the workgroup, so it is read into a scalar register; clamped into [0, F-1] (one scalar max, one scalar min), so
// that no index value can send a load outside the frames' tensors -- the hosts refuse such an index before any launch, this is the second line of defence.
__device__ __forceinline__ int frame_of_cuboid(const UnprojIndexedArgs& a, int p) {
    const int f = __builtin_amdgcn_readfirstlane(a.frame_of[p]);
    return min(max(f, 0), a.F - 1);
}

// workgroup -> (cuboid, chunk, frame) of the indexed kernels.  xcd_pin 0 / 1: sample_chunk_of's mapping over the cuboids.  xcd_pin 2 (by frame): all cuboids
// of a frame read the same maps, so cuboid p runs on XCD frame_of[p] % 8 -- the workgroups of XCD x walk the cuboids whose frame is x modulo 8, in increasing
// p; the assignment lives on the device (it changes from forward to forward of a captured graph), so the grid is sized for the worst case (every cuboid on
// one XCD) and a workgroup whose slot is past its XCD's last cuboid returns false and leaves.  Which workgroup computes a voxel does not touch its arithmetic.
__device__ __forceinline__ bool cuboid_chunk_of(const UnprojIndexedArgs& a, int& p, int& chunk, int& f) {
    if (a.xcd_pin != 2) {
        sample_chunk_of(a, p, chunk);
        f = frame_of_cuboid(a, p);
        return true;
    }
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
    int slot = j / a.chunks;
    chunk = j % a.chunks;
    for (int q = 0; q < a.B; ++q) {
        f = frame_of_cuboid(a, q);
        if ((f & 7) != xcd) continue;
        if (slot-- == 0) { p = q; return true; }
    }
    return false;
}

// The views of sample b of the ragged kernels: its first row and its count, uniform over the workgroup, so both are scalar.  The count is clamped into
// [0, min(NVcap, T)] and the row into [0, T - count]: no table value can send a load outside the T rows -- the hosts refuse such a table before any launch,
// this is the second line of defence, as frame_of_cuboid is.
__device__ __forceinline__ void views_of_sample(const UnprojRaggedArgs& a, int b, int cap, int& row, int& nb) {
    const int lo = __builtin_amdgcn_readfirstlane(a.view_base[b]), hi = __builtin_amdgcn_readfirstlane(a.view_base[b + 1]);
    nb = min(max(hi - lo, 0), min(cap, a.T));
    row = min(max(lo, 0), a.T - nb);
}

// Bilinear sample of CH channels for one voxel in one view (project_taps' geometry): only the corners inside the map are loaded, and
// blended with the raw weights -- the first of the two load disciplines of unproj_geom.h.
template <typename T, int CH>
__device__ __forceinline__ void sample_view(const T* __restrict__ fmap, const float* __restrict__ P, float X0, float X1,
                                            float X2, int h, int w, int C, int c0, float (&val)[CH]) {
    const FullTap t = project_taps<sizeof(T) == 2>(P, X0, X1, X2, h, w);
#pragma unroll
    for (int e = 0; e < CH; ++e) val[e] = 0.f;
    if (!t.act) return;
    float t00[CH], t01[CH], t10[CH], t11[CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) t00[e] = t01[e] = t10[e] = t11[e] = 0.f;
    const T* base = fmap + ((long long)t.y0 * w + t.x0) * C + c0;
    if (t.yn_ok && t.xw_ok) ChVec<T, CH>::ld(base, t00);
    if (t.yn_ok && t.xe_ok) ChVec<T, CH>::ld(base + C, t01);
    if (t.ys_ok && t.xw_ok) ChVec<T, CH>::ld(base + (long long)w * C, t10);
    if (t.ys_ok && t.xe_ok) ChVec<T, CH>::ld(base + (long long)w * C + C, t11);
#pragma unroll
    for (int e = 0; e < CH; ++e) val[e] = t00[e] * t.wt[0] + t01[e] * t.wt[1] + t10[e] * t.wt[2] + t11[e] * t.wt[3];
}

// does view v take part?  Without a mask: constant true, so the unmasked instantiations compile to what they did before the mask existed
// (NULLABLE, the indexed kernels: a null mask means every view is valid; as bits that is all ones)
template <bool MASKED, bool BITS, bool NULLABLE = false>
__device__ __forceinline__ bool view_on(unsigned mbits, const uint8_t* __restrict__ mk, int v) {
    if constexpr (!MASKED) return true;
    else if constexpr (BITS) return ((mbits >> v) & 1u) != 0;
    else if constexpr (NULLABLE) return !mk || mk[v] != 0;
    else return mk[v] != 0;
}

// MASKED: the views {v : mask[b][v]} of sample b alone, visited in increasing v -- exactly the unmasked arithmetic on the compacted views (a
// masked view is never sampled; no valid view at all: zeros).  The mask of a sample is uniform over its workgroups: SMALL_NV keeps it as bits.
// INDEXED (on the masked form): sample b is cuboid b, which reads the maps, projections, confidences and mask of its frame f = frame_of[b].
// RAGGED (on the masked form): sample b's views are the rows view_base[b] + v, v < n_b, of feats, proj and conf; its mask is the prefix of n_b bits (kept
// as bits whatever NV is: NVcap <= 32), n_b = 0: zeros.
template <typename T, int CH, bool SMALL_NV, bool MASKED = false, bool INDEXED = false, bool RAGGED = false>
__global__ __launch_bounds__(256) void unproject_kernel(const UnprojArgsOf<MASKED, INDEXED, RAGGED> a) {
    static_assert(MASKED || !INDEXED, "the indexed kernels are built on the masked form");
    static_assert(!RAGGED || (MASKED && !INDEXED), "the ragged kernels are built on the masked form");
    constexpr bool FAST = sizeof(T) == 2;
    constexpr bool BITS = SMALL_NV || RAGGED;
    const int tpv = a.C / CH;  // lanes per voxel
    int b, chunk, f;           // f: the sample whose views are read
    if constexpr (INDEXED) {
        if (!cuboid_chunk_of(a, b, chunk, f)) return;
    } else {
        sample_chunk_of(a, b, chunk);
        f = b;
    }
    const long long nvox = (long long)a.v0 * a.v1 * a.v2;
    long long vrow;            // the row of the sample's first view
    unsigned mbits = ~0u;
    if constexpr (RAGGED) {
        int row, nb;
        views_of_sample(a, b, a.NV, row, nb);
        vrow = row;
        mbits = nb >= 32 ? ~0u : (1u << nb) - 1u;
    } else {
        vrow = (long long)f * a.NV;
    }
    const T* feats = (const T*)a.feats + vrow * a.h * a.w * a.C;
    const float* P = a.proj + vrow * 12;
    const float* coords = a.coords + (long long)b * nvox * 3;
    T* out = (T*)a.out + (long long)b * nvox * a.C;
    int bi = 0, bj = 0, bk = 0;
    if (a.bricked) brick_of(a, chunk, bi, bj, bk);
    const uint8_t* mk = nullptr;
    if constexpr (MASKED && !RAGGED) {
        mk = a.mask + (long long)f * a.NV;
        if constexpr (INDEXED) if (!a.mask) mk = nullptr;
        if (SMALL_NV && (!INDEXED || mk)) {
            mbits = 0;
            for (int v = 0; v < a.NV; ++v) mbits |= (mk[v] ? 1u : 0u) << v;
        }
    }
    const int items = 256 * tpv;
    for (int q = threadIdx.x; q < items; q += 256) {
        const int vb = q / tpv;            // voxel within the chunk, 0..255
        const int c0 = (q - vb * tpv) * CH;
        long long vox;
        if (a.bricked) vox = ((long long)(bi + (vb >> 6)) * a.v1 + bj + ((vb >> 4) & 3)) * a.v2 + bk + (vb & 15);
        else vox = (long long)chunk * 256 + vb;
        if (vox >= nvox) continue;
        const float X0 = coords[vox * 3], X1 = coords[vox * 3 + 1], X2 = coords[vox * 3 + 2];
        float res[CH];
        if (SMALL_NV) {  // NV <= 8: keep every view's sample in registers (two-pass softmax like torch)
            float vals[8][CH];
#pragma unroll
            for (int v = 0; v < 8; ++v)
                if (v < a.NV && view_on<MASKED, BITS, INDEXED>(mbits, mk, v)) sample_view<T, CH>(feats + (long long)v * a.h * a.w * a.C, P + v * 12, X0, X1, X2, a.h, a.w, a.C, c0, vals[v]);
#pragma unroll
            for (int e = 0; e < CH; ++e) {
                float r;
                if (a.agg == LT_AGG_SOFTMAX) {
                    float m;
                    if constexpr (MASKED) {          // the first valid view starts the max, as view 0 does below
                        bool have = false;
                        m = 0.f;
#pragma unroll
                        for (int v = 0; v < 8; ++v) if (v < a.NV && view_on<MASKED, BITS, INDEXED>(mbits, mk, v)) { m = have ? fmaxf(m, vals[v][e]) : vals[v][e]; have = true; }
                    } else {
                        m = vals[0][e];
#pragma unroll
                        for (int v = 1; v < 8; ++v) if (v < a.NV) m = fmaxf(m, vals[v][e]);
                    }
                    // sum_v x_v softmax_v(x) = (sum_v x_v e_v) / (sum_v e_v): one division per channel
                    float s = 0.f, tt = 0.f;
#pragma unroll
                    for (int v = 0; v < 8; ++v) if (v < a.NV && view_on<MASKED, BITS, INDEXED>(mbits, mk, v)) { const float ex = exp_<FAST>(vals[v][e] - m); s += ex; tt += vals[v][e] * ex; }
                    r = div_<FAST>(tt, s);
                } else if (a.agg == LT_AGG_MAX) {
                    if constexpr (MASKED) {
                        bool have = false;
                        r = 0.f;
#pragma unroll
                        for (int v = 0; v < 8; ++v) if (v < a.NV && view_on<MASKED, BITS, INDEXED>(mbits, mk, v)) { r = have ? fmaxf(r, vals[v][e]) : vals[v][e]; have = true; }
                    } else {
                        r = vals[0][e];
#pragma unroll
                        for (int v = 1; v < 8; ++v) if (v < a.NV) r = fmaxf(r, vals[v][e]);
                    }
                } else if (a.agg == LT_AGG_CONF || a.agg == LT_AGG_CONF_NORM) {
                    float cs = 1.f;
                    if (a.agg == LT_AGG_CONF_NORM) {
                        cs = 0.f;
#pragma unroll
                        for (int v = 0; v < 8; ++v) if (v < a.NV && view_on<MASKED, BITS, INDEXED>(mbits, mk, v)) cs += a.conf[(vrow + v) * a.C + c0 + e];
                    }
                    r = 0.f;
#pragma unroll
                    for (int v = 0; v < 8; ++v) if (v < a.NV && view_on<MASKED, BITS, INDEXED>(mbits, mk, v)) r += vals[v][e] * __fdiv_rn(a.conf[(vrow + v) * a.C + c0 + e], cs);
                } else {
                    r = 0.f;
#pragma unroll
                    for (int v = 0; v < 8; ++v) if (v < a.NV && view_on<MASKED, BITS, INDEXED>(mbits, mk, v)) r += vals[v][e];
                }
                if constexpr (MASKED) if (mbits == 0) r = 0.f;   // no valid view
                res[e] = r;
            }
        } else {  // any NV: recompute the samples instead of storing them (softmax needs the max first)
            float m[CH], s[CH], acc[CH], val[CH], cs[CH];
#pragma unroll
            for (int e = 0; e < CH; ++e) {
                m[e] = -INFINITY; s[e] = 0.f; acc[e] = 0.f; cs[e] = 1.f;
                if (a.agg == LT_AGG_CONF_NORM) {
                    cs[e] = 0.f;
                    for (int v = 0; v < a.NV; ++v) if (view_on<MASKED, BITS, INDEXED>(mbits, mk, v)) cs[e] += a.conf[(vrow + v) * a.C + c0 + e];
                }
            }
            bool any = !MASKED;
            if constexpr (MASKED)
                for (int v = 0; v < a.NV; ++v) any = any || view_on<MASKED, BITS, INDEXED>(mbits, mk, v);
            if (a.agg == LT_AGG_SOFTMAX || a.agg == LT_AGG_MAX)
                for (int v = 0; v < a.NV; ++v) {
                    if (!view_on<MASKED, BITS, INDEXED>(mbits, mk, v)) continue;
                    sample_view<T, CH>(feats + (long long)v * a.h * a.w * a.C, P + v * 12, X0, X1, X2, a.h, a.w, a.C, c0, val);
#pragma unroll
                    for (int e = 0; e < CH; ++e) m[e] = fmaxf(m[e], val[e]);
                }
            if (a.agg != LT_AGG_MAX)
                for (int v = 0; v < a.NV; ++v) {
                    if (!view_on<MASKED, BITS, INDEXED>(mbits, mk, v)) continue;
                    sample_view<T, CH>(feats + (long long)v * a.h * a.w * a.C, P + v * 12, X0, X1, X2, a.h, a.w, a.C, c0, val);
#pragma unroll
                    for (int e = 0; e < CH; ++e) {
                        if (a.agg == LT_AGG_SOFTMAX) { const float ex = exp_<FAST>(val[e] - m[e]); s[e] += ex; acc[e] += val[e] * ex; }
                        else if (a.agg == LT_AGG_CONF || a.agg == LT_AGG_CONF_NORM)
                            acc[e] += val[e] * __fdiv_rn(a.conf[(vrow + v) * a.C + c0 + e], cs[e]);
                        else acc[e] += val[e];
                    }
                }
#pragma unroll
            for (int e = 0; e < CH; ++e)
                res[e] = !any ? 0.f : (a.agg == LT_AGG_MAX ? m[e] : (a.agg == LT_AGG_SOFTMAX ? __fdiv_rn(acc[e], s[e]) : acc[e]));
        }
        ChVec<T, CH>::st(out + vox * a.C + c0, res);
    }
}

// (unproject_lds_kernel, an LDS-staged variant of the gather -- opt-in with LT_UNPROJ_LDS=1 -- measured 0.90 ms against 0.57 ms for the
// gathering kernel at the BASELINE shape and was removed in round 2: the 37 MB of feature maps are L2-resident and the gather keeps 16
// independent loads in flight per lane, while the staged copy exposes one load round trip per workgroup between its two barriers.)

// ---- quad kernel: bf16, C = 32, 4 or 8 views, softmax aggregation, bricked volumes (BASELINE configurations 2 and 4) ------------------
// The generic kernel above is VALU-bound (~700 instructions per lane-item at 4 views; PMC: 40 % of the cycles waiting on instruction
// issue): every one of the four lanes of a voxel (one per 8-channel vector) redoes the projection of the voxel into all views.
// Here the four lanes of a voxel's quad split the VIEWS for the projection (lane j projects into views j, j+4, ... and keeps those
// 3x4 matrices in registers for the whole kernel), fold the zero-padding rules into the four bilinear weights (an invalid corner
// gets weight 0 and a clamped, readable address), and hand the four tap offsets + four weights of their views to the other three
// lanes with DPP quad broadcasts; the bilinear blend and the view softmax run on packed fp32 pairs with EXPLICIT fused
// multiply-adds (the library is built with -ffp-contract=off for the bit-exact coordinate grid, which left this kernel with 109
// v_pk_mul + 102 v_pk_add per voxel where 125 v_pk_fma do).  NVL = views per lane (1: 4 views, 2: 8 views).  GRID: the voxel centre
// is computed in registers from the cuboid description (bit-identical to coord_volumes_kernel) instead of read from the 12-byte-
// per-voxel coordinate volume, and lanes 0-2 of the quad write its three components to the returned tensor on the way.
typedef float f32x2_t __attribute__((ext_vector_type(2)));

template <int Q>
__device__ __forceinline__ int quad_bcast_i(int v) {   // value of lane Q of this lane's quad
    return __builtin_amdgcn_mov_dpp(v, Q | (Q << 2) | (Q << 4) | (Q << 6), 0xf, 0xf, true);
}
template <int Q>
__device__ __forceinline__ float quad_bcast_f(float v) { return __int_as_float(quad_bcast_i<Q>(__float_as_int(v))); }
__device__ __forceinline__ f32x2_t pk_fma(f32x2_t a, f32x2_t b, f32x2_t c) { return __builtin_elementwise_fma(a, b, c); }

// (round 6, measured and not kept: the 8-view instantiation takes 152 VGPRs = 3 waves per SIMD; capped at 128 = 4 waves with __launch_bounds__(256, 4) --
//  4 registers of loop invariants in scratch -- it ran 3.72-3.75 ms against 3.62-3.67 ms at BASELINE config 4, and with MORE memory traffic (3.09 vs 2.80 GB):
//  the kernel is bound by VALU issue + the gather path together (valu_issue_frac 0.44-0.45), and a fourth wave adds neither.)
// MASKED: a sample's mask is the same in every lane of its workgroups, so it is read once, into a scalar register as bits, and every view is one
// scalar branch: a masked view issues no loads, no blend and no exp2, and leaves its val[] registers untouched.  The softmax walks the views
// outermost there (one branch per view instead of one per view and channel pair); per channel the operations and their order are those of
// the unmasked kernel on the valid views, so an all-ones mask gives its bits (the max starts from -inf where the unmasked kernel starts from view 0:
// the same value unless EVERY valid view's sample is NaN, and then both write NaN).  (The lanes still project into their masked views: which
// lane owns a view varies over the quad, and the 30 instructions are not worth a divergent branch.)
// INDEXED (on the masked form): as in unproject_kernel -- the maps, projections and mask of frame f = frame_of[b], everything of the cuboid by b.
// RAGGED (on the masked form): as in unproject_kernel -- rows view_base[b] + v, the prefix mask of n_b bits.  The rows behind a sample's last view are
// the next sample's, and behind row T - 1 nobody's: a lane whose view slot is not one of the sample's loads the projection of the sample's LAST view
// in its place (row clamped below T), so no address outside the T rows is formed for a load; what it projects is never sampled (the slot is masked).
template <int NVL, bool GRID, bool MASKED = false, bool INDEXED = false, bool RAGGED = false>
__global__ __launch_bounds__(256) void unproject_qn_kernel(const UnprojArgsOf<MASKED, INDEXED, RAGGED> a) {
    static_assert(MASKED || !INDEXED, "the indexed kernels are built on the masked form");
    static_assert(!RAGGED || (MASKED && !INDEXED), "the ragged kernels are built on the masked form");
    typedef bf16_t T;
    constexpr int C = 32, NV = 4 * NVL;
    int b, chunk, f;
    if constexpr (INDEXED) {
        if (!cuboid_chunk_of(a, b, chunk, f)) return;
    } else {
        sample_chunk_of(a, b, chunk);
        f = b;
    }
    const long long nvox = (long long)a.v0 * a.v1 * a.v2;
    long long vrow;            // the row of the sample's first view
    int nb = NV;
    if constexpr (RAGGED) {
        int row;
        views_of_sample(a, b, NV, row, nb);
        vrow = row;
    } else {
        vrow = (long long)f * NV;
    }
    const T* feats = (const T*)a.feats + vrow * a.h * a.w * C;
    const float* coords = GRID ? nullptr : a.coords + (long long)b * nvox * 3;
    float* coords_out = (GRID && a.coords_out) ? a.coords_out + (long long)b * nvox * 3 : nullptr;
    T* out = (T*)a.out + (long long)b * nvox * C;
    int bi, bj, bk;
    brick_of(a, chunk, bi, bj, bk);
    const int t = threadIdx.x, qv = t & 3;               // qv: the views this lane projects into (qv, qv + 4) AND its 8-channel vector
    const int h = a.h, w = a.w;
    float P[NVL][12];
#pragma unroll
    for (int s = 0; s < NVL; ++s) {
        long long prow = vrow + qv + 4 * s;
        if constexpr (RAGGED) prow = min(vrow + min(qv + 4 * s, max(nb - 1, 0)), (long long)a.T - 1);
#pragma unroll
        for (int i = 0; i < 12; ++i) P[s][i] = a.proj[prow * 12 + i];
    }
    float gp[3], gc[3], gR[9];
    if (GRID) {
#pragma unroll
        for (int i = 0; i < 3; ++i) { gp[i] = a.g_pos[3 * b + i]; gc[i] = a.g_center[3 * b + i]; }
#pragma unroll
        for (int i = 0; i < 9; ++i) gR[i] = a.g_rot[9 * b + i];
    }
    const float inv_h = __builtin_amdgcn_rcpf((float)h), inv_w = __builtin_amdgcn_rcpf((float)w);
    unsigned mbits = (1u << NV) - 1u;
    if constexpr (RAGGED) {
        mbits = (1u << nb) - 1u;
    } else if constexpr (MASKED) {
        if (!INDEXED || a.mask) {
            mbits = 0;
#pragma unroll
            for (int v = 0; v < NV; ++v) mbits |= (a.mask[(long long)f * NV + v] ? 1u : 0u) << v;
        }
        mbits = __builtin_amdgcn_readfirstlane(mbits);
    }

#pragma unroll 1
    for (int it = 0; it < 4; ++it) {
        const int vb = it * 64 + (t >> 2);
        const int vi = bi + (vb >> 6), vj = bj + ((vb >> 4) & 3), vk = bk + (vb & 15);
        const long long vox = ((long long)vi * a.v1 + vj) * a.v2 + vk;
        float X0, X1, X2;
        if (GRID) {
            voxel_coord(gp, gc, gR, a.g_step, vi, vj, vk, a.v0, a.g_cmu, X0, X1, X2);
            if (coords_out && qv < 3) coords_out[vox * 3 + qv] = qv == 0 ? X0 : (qv == 1 ? X1 : X2);
        } else {
            X0 = coords[vox * 3]; X1 = coords[vox * 3 + 1]; X2 = coords[vox * 3 + 2];
        }
        int o00[NVL], o01[NVL], o10[NVL], o11[NVL];
        float k00[NVL], k01[NVL], k10[NVL], k11[NVL];
#pragma unroll
        for (int s = 0; s < NVL; ++s) {
            // view qv + 4 s: its four corners as element offsets (clamped into the map) and weights (0 where the corner is padding)
            const FullTap tp = project_taps<true>(P[s], X0, X1, X2, h, w, inv_h, inv_w, C, (qv + 4 * s) * h * w * C);
            o00[s] = tp.off[0]; o01[s] = tp.off[1]; o10[s] = tp.off[2]; o11[s] = tp.off[3];
            k00[s] = tp.k[0]; k01[s] = tp.k[1]; k10[s] = tp.k[2]; k11[s] = tp.k[3];
        }

        f32x2_t val[NV][4];                               // [view][channel pair] of this lane's 8 channels
        auto view = [&](auto vc) {
            constexpr int V = decltype(vc)::value, Q = V & 3, S = V >> 2;
            if constexpr (MASKED) if (!((mbits >> V) & 1u)) return;
            const int p00 = quad_bcast_i<Q>(o00[S]), p01 = quad_bcast_i<Q>(o01[S]), p10 = quad_bcast_i<Q>(o10[S]), p11 = quad_bcast_i<Q>(o11[S]);
            const float w00 = quad_bcast_f<Q>(k00[S]), w01 = quad_bcast_f<Q>(k01[S]), w10 = quad_bcast_f<Q>(k10[S]), w11 = quad_bcast_f<Q>(k11[S]);
            const uint4 t00 = *(const uint4*)(feats + p00 + qv * 8), t01 = *(const uint4*)(feats + p01 + qv * 8);
            const uint4 t10 = *(const uint4*)(feats + p10 + qv * 8), t11 = *(const uint4*)(feats + p11 + qv * 8);
            const unsigned u00[4] = {t00.x, t00.y, t00.z, t00.w}, u01[4] = {t01.x, t01.y, t01.z, t01.w};
            const unsigned u10[4] = {t10.x, t10.y, t10.z, t10.w}, u11[4] = {t11.x, t11.y, t11.z, t11.w};
            const f32x2_t W00 = {w00, w00}, W01 = {w01, w01}, W10 = {w10, w10}, W11 = {w11, w11};
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const f32x2_t f00 = {__uint_as_float(u00[d] << 16), __uint_as_float(u00[d] & 0xffff0000u)};
                const f32x2_t f01 = {__uint_as_float(u01[d] << 16), __uint_as_float(u01[d] & 0xffff0000u)};
                const f32x2_t f10 = {__uint_as_float(u10[d] << 16), __uint_as_float(u10[d] & 0xffff0000u)};
                const f32x2_t f11 = {__uint_as_float(u11[d] << 16), __uint_as_float(u11[d] & 0xffff0000u)};
                val[V][d] = pk_fma(f11, W11, pk_fma(f10, W10, pk_fma(f01, W01, f00 * W00)));
            }
        };
        static_for<0, NV>(view);

        // ---- softmax over the views per channel: sum_v x_v softmax_v(x) = (sum_v x_v e_v) / (sum_v e_v) ----
        unsigned o[4];
        if constexpr (MASKED) {
            if (mbits == 0) {                             // no valid view: zeros
                *(uint4*)(out + vox * C + qv * 8) = make_uint4(0u, 0u, 0u, 0u);
                continue;
            }
            const f32x2_t L2E = {1.4426950408889634f, 1.4426950408889634f};
            f32x2_t m[4], s[4], tt[4];
#pragma unroll
            for (int d = 0; d < 4; ++d) { m[d] = f32x2_t{-INFINITY, -INFINITY}; s[d] = f32x2_t{0.f, 0.f}; tt[d] = f32x2_t{0.f, 0.f}; }
            static_for<0, NV>([&](auto vc) {       // fmaxf(-inf, x) = x: the first valid view starts the max, as view 0 does below
                constexpr int V = decltype(vc)::value;
                if (!((mbits >> V) & 1u)) return;
#pragma unroll
                for (int d = 0; d < 4; ++d) { m[d][0] = fmaxf(m[d][0], val[V][d][0]); m[d][1] = fmaxf(m[d][1], val[V][d][1]); }
            });
            static_for<0, NV>([&](auto vc) {
                constexpr int V = decltype(vc)::value;
                if (!((mbits >> V) & 1u)) return;
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const f32x2_t dl = pk_fma(val[V][d], L2E, -(m[d] * L2E));   // (x - m) log2(e)
                    const f32x2_t ex = {__builtin_amdgcn_exp2f(dl[0]), __builtin_amdgcn_exp2f(dl[1])};
                    s[d] += ex;
                    tt[d] = pk_fma(val[V][d], ex, tt[d]);
                }
            });
#pragma unroll
            for (int d = 0; d < 4; ++d) o[d] = pack_bf16x2(tt[d][0] * __builtin_amdgcn_rcpf(s[d][0]), tt[d][1] * __builtin_amdgcn_rcpf(s[d][1]));
        } else {
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            f32x2_t m = val[0][d];
#pragma unroll
            for (int v = 1; v < NV; ++v) { m[0] = fmaxf(m[0], val[v][d][0]); m[1] = fmaxf(m[1], val[v][d][1]); }
            f32x2_t s = {0.f, 0.f}, tt = {0.f, 0.f};
            const f32x2_t L2E = {1.4426950408889634f, 1.4426950408889634f}, mL = m * L2E;
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const f32x2_t dl = pk_fma(val[v][d], L2E, -mL);                 // (x - m) log2(e)
                const f32x2_t ex = {__builtin_amdgcn_exp2f(dl[0]), __builtin_amdgcn_exp2f(dl[1])};
                s += ex;
                tt = pk_fma(val[v][d], ex, tt);
            }
            o[d] = pack_bf16x2(tt[0] * __builtin_amdgcn_rcpf(s[0]), tt[1] * __builtin_amdgcn_rcpf(s[1]));
        }
        }
        *(uint4*)(out + vox * C + qv * 8) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// LT_UNPROJ_PIN unset: the indexed kernels pin by cuboid (false) or by frame (true) -- the faster of the two in tools/multi_cuboid_bench.py.  Measured at
// BASELINE config 2's gather shape, bf16, 8 frames x 4 cuboids (profiles/multi_cuboid_bench.json): by cuboid 0.590 ms per launch, level with the unindexed
// gather on 32 gathered samples (0.564 ms); by frame 1.541 ms (2.241 ms with 11, 7, 5, 3, 2, 2, 1, 1 cuboids per frame): its grid is sized for the worst case
// and the XCD with the most cuboids sets the time, which costs more than the shared L2 saves (2.4 MB of maps per frame).
constexpr bool PIN_DEFAULT_FRAME = false;

// One workgroup of 256 threads per (sample, chunk).  An unmasked kernel receives a plain UnprojArgs by value (the base of m) and a masked one all of
// m: that is what keeps the unmasked kernels' argument block, and with it their code, what it was before the mask existed.
// An indexed kernel receives all of m (by frame, xcd_pin 2: eight times the workgroups, see cuboid_chunk_of).
template <bool MASKED, bool INDEXED, bool RAGGED = false>
void launch_chunks(void (*kern)(UnprojArgsOf<MASKED, INDEXED, RAGGED>), const UnprojRaggedArgs& m, hipStream_t st) {
    const UnprojArgsOf<MASKED, INDEXED, RAGGED>& a = m;
    hipLaunchKernelGGL(kern, dim3((unsigned)((long long)m.B * m.chunks * (INDEXED && m.xcd_pin == 2 ? 8 : 1))), dim3(256), 0, st, a);
}
template <bool MASKED, bool INDEXED, bool RAGGED = false>
void launch_quad(const UnprojRaggedArgs& m, bool grid, hipStream_t st) {
    launch_chunks<MASKED, INDEXED, RAGGED>(m.NV == 4 ? (grid ? unproject_qn_kernel<1, true, MASKED, INDEXED, RAGGED> : unproject_qn_kernel<1, false, MASKED, INDEXED, RAGGED>)
                                                     : (grid ? unproject_qn_kernel<2, true, MASKED, INDEXED, RAGGED> : unproject_qn_kernel<2, false, MASKED, INDEXED, RAGGED>), m, st);
}
template <typename T, int CH, bool MASKED, bool INDEXED, bool RAGGED = false>
void launch_generic(const UnprojRaggedArgs& m, hipStream_t st) {
    launch_chunks<MASKED, INDEXED, RAGGED>(m.NV <= 8 ? unproject_kernel<T, CH, true, MASKED, INDEXED, RAGGED> : unproject_kernel<T, CH, false, MASKED, INDEXED, RAGGED>, m, st);
}
template <typename T, int CH>
int launch_unproject(const UnprojRaggedArgs& m, hipStream_t st) {
    if (m.view_base) launch_generic<T, CH, true, false, true>(m, st);
    else if (m.frame_of) launch_generic<T, CH, true, true>(m, st);
    else if (m.mask) launch_generic<T, CH, true, false>(m, st);
    else launch_generic<T, CH, false, false>(m, st);
    LT_CHECK_LAUNCH(m.view_base ? "lt_unproject_ragged_fwd" : m.frame_of ? "lt_unproject_indexed_fwd" : m.mask ? "lt_unproject_masked_fwd" : "lt_unproject_fwd");
    return LT_OK;
}

int launch_coord_volumes(const char* what, const float* pos, const float* center, const float* rot, float step, int B, int V, int cmu, float* coords,
                         hipStream_t st) {
    const long long blocks = cdiv((long long)B * V * V * V, 256);
    hipLaunchKernelGGL(coord_volumes_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, st, pos, center, rot, step, B, V, cmu, coords);
    LT_CHECK_LAUNCH(what);
    return LT_OK;
}

// fills the launch geometry and picks the kernel; a.coords (read) or the a.g_* grid description must be set by the caller.  a.mask set: the masked
// instantiation of the SAME kernel the unmasked call takes (a masked plan never leaves the quad kernel for the generic one).  a.frame_of set: the
// indexed instantiation of that kernel, a.B cuboids over a.F frames.  a.view_base set: the ragged instantiation, a.NV = NVcap.
int unproject_dispatch(UnprojRaggedArgs& a, int dtype, bool grid, hipStream_t st) {
    const long long nvox = (long long)a.v0 * a.v1 * a.v2;
    a.bricked = (a.v0 % 4 == 0 && a.v1 % 4 == 0 && a.v2 % 16 == 0) ? 1 : 0;
    a.blocked = (a.bricked && a.v0 % 32 == 0 && a.v1 % 32 == 0 && a.v2 % 32 == 0 && !env_on("LT_UNPROJ_RASTER")) ? 1 : 0;          // LT_UNPROJ_RASTER=1: the old order (A/B)
    a.chunks = (int)cdiv(nvox, 256);
    a.xcd_pin = (a.B % 8 == 0) ? 1 : 0;
    LT_REQUIRE((long long)a.B * a.chunks < (1ll << 31), LT_ERR_UNSUPPORTED, "lt_unproject_fwd: grid too large");
    if (a.frame_of) {
        // LT_UNPROJ_PIN=frame | cuboid (A/B, read per call): which XCD a cuboid's workgroups run on -- see cuboid_chunk_of; unset: PIN_DEFAULT_FRAME
        const char* pin = getenv("LT_UNPROJ_PIN");
        const bool by_frame = pin && pin[0] ? pin[0] == 'f' : PIN_DEFAULT_FRAME;
        if (by_frame && a.F > 1 && 8ll * a.B * a.chunks < (1ll << 31)) a.xcd_pin = 2;
    }
    // quad kernel: bf16, 32 channels, 4 or 8 views, view softmax, bricked volume (BASELINE configurations 2 and 4)
    const bool no_q4 = env_on("LT_UNPROJ_NO_Q4");       // A/B, read per call
    const bool quad = dtype == LT_BF16 && a.C == 32 && (a.NV == 4 || a.NV == 8) && a.bricked && a.agg == LT_AGG_SOFTMAX && !no_q4 &&
                      (long long)a.NV * a.h * a.w * a.C < (1ll << 30);
    if (quad) {
        if (a.view_base) launch_quad<true, false, true>(a, grid, st);
        else if (a.frame_of) launch_quad<true, true>(a, grid, st);
        else if (a.mask) launch_quad<true, false>(a, grid, st);
        else launch_quad<false, false>(a, grid, st);
        LT_CHECK_LAUNCH(a.view_base ? "lt_unproject_ragged_fwd(quad)" : a.frame_of ? "lt_unproject_indexed_fwd(quad)" : a.mask ? "lt_unproject_masked_fwd(quad)" : "lt_unproject_fwd(quad)");
        return LT_OK;
    }
    if (grid) {      // no fused kernel for this configuration: materialise the grid (it is a returned tensor anyway), then gather
        const int rc = launch_coord_volumes("lt_unproject_grid_fwd(coords)", a.g_pos, a.g_center, a.g_rot, a.g_step, a.B, a.v0, a.g_cmu, a.coords_out, st);
        if (rc != LT_OK) return rc;
        a.coords = a.coords_out;
    }
    if (dtype == LT_F32) {
        if (a.C % 4 == 0) return launch_unproject<float, 4>(a, st);
        return launch_unproject<float, 1>(a, st);
    }
    if (a.C % 8 == 0) return launch_unproject<bf16_t, 8>(a, st);
    return launch_unproject<bf16_t, 1>(a, st);
}

// The one body behind lt_unproject_desc_fwd and its eight shorthands: `who` is the entry that was called.  The variant is which pointers of d are set
// (include/lt_hip.h); unproject_dispatch picks the instantiation from the same pointers.
int unproject_forward(const char* who, const lt_unproject_desc& d, void* out, void* stream) {
    const bool cuboid_any = d.pos || d.center || d.rot || d.coords_out, grid = !d.coords;
    LT_REQUIRE(!d.view_base || !(d.view_mask || d.frame_of), LT_ERR_UNSUPPORTED, "%s: view_base with %s has no kernel (a ragged batch takes neither a view mask nor a frame index)",
               who, d.view_mask ? "view_mask" : "frame_of");
    LT_REQUIRE(!d.view_base || d.B >= 1, LT_ERR_INVALID, "%s: B %d samples", who, d.B);
    LT_REQUIRE(!d.view_base || d.T >= 1, LT_ERR_INVALID, "%s: T %d images", who, d.T);
    LT_REQUIRE(!d.view_base || (d.NV >= 1 && d.NV <= 32), LT_ERR_INVALID, "%s: NVcap %d (1..32)", who, d.NV);
    LT_REQUIRE(!d.frame_of || d.F >= 1, LT_ERR_INVALID, "%s: F %d frames", who, d.F);
    LT_REQUIRE(!d.frame_of || d.B >= 1, LT_ERR_INVALID, "%s: P %d cuboids", who, d.B);
    LT_REQUIRE(!(d.coords && cuboid_any), LT_ERR_INVALID, "%s: both coords and the cuboid (pos, center, rot, coords_out) are set", who);
    LT_REQUIRE(d.coords || cuboid_any, LT_ERR_INVALID, "%s: null argument (neither coords nor the cuboid pos, center, rot, coords_out is set)", who);
    LT_REQUIRE(d.feats && d.proj && out && (!grid || (d.pos && d.center && d.rot && d.coords_out)), LT_ERR_INVALID, "%s: null argument", who);
    LT_REQUIRE(d.dtype == LT_F32 || d.dtype == LT_BF16, LT_ERR_INVALID, "%s: bad dtype %d", who, d.dtype);
    LT_REQUIRE(d.agg >= LT_AGG_SUM && d.agg <= LT_AGG_CONF_NORM, LT_ERR_INVALID, "%s: unknown aggregation %d", who, d.agg);
    LT_REQUIRE((d.agg != LT_AGG_CONF && d.agg != LT_AGG_CONF_NORM) || d.conf, LT_ERR_INVALID, "%s: LT_AGG_CONF* needs confidences", who);
    LT_REQUIRE(d.B >= 1 && d.NV >= 1 && d.C >= 1 && d.h >= 2 && d.w >= 2 && (grid ? d.v0 >= 2 && d.v1 == d.v0 && d.v2 == d.v0 : d.v0 >= 1 && d.v1 >= 1 && d.v2 >= 1),
               LT_ERR_INVALID, "%s: bad shape", who);
    LT_REQUIRE((long long)d.NV * d.h * d.w * d.C < (1ll << 31), LT_ERR_UNSUPPORTED, "%s: feature maps too large", who);
    UnprojRaggedArgs a = {};
    a.frame_of = d.frame_of; a.F = d.frame_of ? d.F : 0;
    a.view_base = d.view_base; a.T = d.view_base ? d.T : 0;
    a.feats = d.feats; a.proj = d.proj; a.coords = d.coords; a.conf = d.conf; a.out = out; a.mask = d.view_mask;
    a.B = d.B; a.NV = d.NV; a.C = d.C; a.h = d.h; a.w = d.w; a.v0 = d.v0; a.v1 = d.v1; a.v2 = d.v2; a.agg = d.agg;
    if (grid) { a.g_pos = d.pos; a.g_center = d.center; a.g_rot = d.rot; a.g_step = d.step; a.g_cmu = d.cmu_transfer; a.coords_out = d.coords_out; }
    return unproject_dispatch(a, d.dtype, grid, (hipStream_t)stream);
}

// the grid shorthands' descriptor (V cubed), plain; unproject_coord_desc (unproj_geom.h) is the coordinate shorthands'
lt_unproject_desc grid_desc(int dtype, const void* feats, const float* proj, const float* pos, const float* center, const float* rot, float step, int cmu,
                            float* coords_out, const float* conf, int B, int NV, int C, int h, int w, int V, int agg) {
    lt_unproject_desc d = unproject_coord_desc(dtype, feats, proj, nullptr, conf, B, NV, C, h, w, V, V, V, agg);
    d.pos = pos; d.center = center; d.rot = rot; d.step = step; d.cmu_transfer = cmu; d.coords_out = coords_out;
    return d;
}
// what is an error for a shorthand but a variant for the descriptor: the null pointer of the shorthand's own variant
int masked_forward(const char* who, lt_unproject_desc d, const uint8_t* view_mask, void* out, void* stream) {
    LT_REQUIRE(view_mask, LT_ERR_INVALID, "%s: null view_mask", who);
    d.view_mask = view_mask;
    return unproject_forward(who, d, out, stream);
}
int indexed_forward(const char* who, lt_unproject_desc d, const uint8_t* view_mask, const int32_t* frame_of, int F, void* out, void* stream) {
    LT_REQUIRE(frame_of, LT_ERR_INVALID, "%s: null frame_of", who);
    d.view_mask = view_mask; d.frame_of = frame_of; d.F = F;
    return unproject_forward(who, d, out, stream);
}
int ragged_forward(const char* who, lt_unproject_desc d, const int32_t* view_base, int T, void* out, void* stream) {
    LT_REQUIRE(view_base, LT_ERR_INVALID, "%s: null view_base", who);
    d.view_base = view_base; d.T = T;
    return unproject_forward(who, d, out, stream);
}

}  // namespace

extern "C" int lt_coord_volumes(const float* pos, const float* center, const float* rot, float step, int32_t B, int32_t V,
                                int32_t cmu_transfer, float* coords, void* stream) {
    LT_REQUIRE(pos && center && rot && coords && B >= 1 && V >= 2, LT_ERR_INVALID, "lt_coord_volumes: bad argument");
    return launch_coord_volumes("lt_coord_volumes", pos, center, rot, step, B, V, cmu_transfer, coords, (hipStream_t)stream);
}

extern "C" int lt_unproject_desc_fwd(const lt_unproject_desc* desc, void* out, void* stream) {
    LT_REQUIRE(desc, LT_ERR_INVALID, "lt_unproject_desc_fwd: null descriptor");
    return unproject_forward("lt_unproject_desc_fwd", *desc, out, stream);
}

extern "C" int lt_unproject_fwd(int32_t dtype, const void* feats, const float* proj, const float* coords, const float* conf,
                                void* out, int32_t B, int32_t NV, int32_t C, int32_t h, int32_t w, int32_t v0, int32_t v1,
                                int32_t v2, int32_t agg, void* stream) {
    return unproject_forward("lt_unproject_fwd", unproject_coord_desc(dtype, feats, proj, coords, conf, B, NV, C, h, w, v0, v1, v2, agg), out, stream);
}

extern "C" int lt_unproject_masked_fwd(int32_t dtype, const void* feats, const float* proj, const float* coords, const float* conf, const uint8_t* view_mask,
                                       void* out, int32_t B, int32_t NV, int32_t C, int32_t h, int32_t w, int32_t v0, int32_t v1, int32_t v2, int32_t agg,
                                       void* stream) {
    return masked_forward("lt_unproject_masked_fwd", unproject_coord_desc(dtype, feats, proj, coords, conf, B, NV, C, h, w, v0, v1, v2, agg), view_mask, out, stream);
}

extern "C" int lt_unproject_grid_fwd(int32_t dtype, const void* feats, const float* proj, const float* pos, const float* center, const float* rot,
                                     float step, int32_t cmu_transfer, float* coords_out, const float* conf, void* out, int32_t B, int32_t NV,
                                     int32_t C, int32_t h, int32_t w, int32_t V, int32_t agg, void* stream) {
    return unproject_forward("lt_unproject_grid_fwd", grid_desc(dtype, feats, proj, pos, center, rot, step, cmu_transfer, coords_out, conf, B, NV, C, h, w, V, agg),
                             out, stream);
}

extern "C" int lt_unproject_grid_masked_fwd(int32_t dtype, const void* feats, const float* proj, const float* pos, const float* center, const float* rot,
                                            float step, int32_t cmu_transfer, float* coords_out, const float* conf, const uint8_t* view_mask, void* out,
                                            int32_t B, int32_t NV, int32_t C, int32_t h, int32_t w, int32_t V, int32_t agg, void* stream) {
    return masked_forward("lt_unproject_grid_masked_fwd", grid_desc(dtype, feats, proj, pos, center, rot, step, cmu_transfer, coords_out, conf, B, NV, C, h, w, V, agg),
                          view_mask, out, stream);
}

extern "C" int lt_unproject_indexed_fwd(int32_t dtype, const void* feats, const float* proj, const float* coords, const float* conf, const uint8_t* view_mask,
                                        const int32_t* frame_of, void* out, int32_t F, int32_t P, int32_t NV, int32_t C, int32_t h, int32_t w, int32_t v0,
                                        int32_t v1, int32_t v2, int32_t agg, void* stream) {
    return indexed_forward("lt_unproject_indexed_fwd", unproject_coord_desc(dtype, feats, proj, coords, conf, P, NV, C, h, w, v0, v1, v2, agg), view_mask, frame_of, F, out,
                           stream);
}

extern "C" int lt_unproject_grid_indexed_fwd(int32_t dtype, const void* feats, const float* proj, const float* pos, const float* center, const float* rot,
                                             float step, int32_t cmu_transfer, float* coords_out, const float* conf, const uint8_t* view_mask,
                                             const int32_t* frame_of, void* out, int32_t F, int32_t P, int32_t NV, int32_t C, int32_t h, int32_t w, int32_t V,
                                             int32_t agg, void* stream) {
    return indexed_forward("lt_unproject_grid_indexed_fwd", grid_desc(dtype, feats, proj, pos, center, rot, step, cmu_transfer, coords_out, conf, P, NV, C, h, w, V, agg),
                           view_mask, frame_of, F, out, stream);
}

extern "C" int lt_unproject_ragged_fwd(int32_t dtype, const void* feats, const float* proj, const float* coords, const float* conf, const int32_t* view_base,
                                       void* out, int32_t B, int32_t T, int32_t NVcap, int32_t C, int32_t h, int32_t w, int32_t v0, int32_t v1, int32_t v2,
                                       int32_t agg, void* stream) {
    return ragged_forward("lt_unproject_ragged_fwd", unproject_coord_desc(dtype, feats, proj, coords, conf, B, NVcap, C, h, w, v0, v1, v2, agg), view_base, T, out, stream);
}

extern "C" int lt_unproject_grid_ragged_fwd(int32_t dtype, const void* feats, const float* proj, const float* pos, const float* center, const float* rot,
                                            float step, int32_t cmu_transfer, float* coords_out, const float* conf, const int32_t* view_base, void* out,
                                            int32_t B, int32_t T, int32_t NVcap, int32_t C, int32_t h, int32_t w, int32_t V, int32_t agg, void* stream) {
    return ragged_forward("lt_unproject_grid_ragged_fwd", grid_desc(dtype, feats, proj, pos, center, rot, step, cmu_transfer, coords_out, conf, B, NVcap, C, h, w, V, agg),
                          view_base, T, out, stream);
}

namespace {
__global__ void rotate_points_kernel(const float* __restrict__ x, const float* __restrict__ R, float* __restrict__ y, long long n) {
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (long long)gridDim.x * blockDim.x) {
        const float a = x[g * 3], b = x[g * 3 + 1], c = x[g * 3 + 2];
        y[g * 3] = fmaf(R[2], c, fmaf(R[1], b, __fmul_rn(R[0], a)));
        y[g * 3 + 1] = fmaf(R[5], c, fmaf(R[4], b, __fmul_rn(R[3], a)));
        y[g * 3 + 2] = fmaf(R[8], c, fmaf(R[7], b, __fmul_rn(R[6], a)));
    }
}
}  // namespace

extern "C" int lt_rotate_points(const float* x, const float* rot, float* y, int64_t n, void* stream) {
    LT_REQUIRE(x && rot && y && n >= 1, LT_ERR_INVALID, "lt_rotate_points: bad argument");
    const long long blocks = cdiv(n, 256);
    hipLaunchKernelGGL(rotate_points_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, (hipStream_t)stream, x, rot, y, (long long)n);
    LT_CHECK_LAUNCH("lt_rotate_points");
    return LT_OK;
}

// ---- the seam of the cascade: the algebraic model's joints -> the volumetric cuboid, on the device ----------------------------------------
namespace {
// VolumetricTriangulationNet._host_geometry's pelvis and cuboid algebra (triangulation.py:284-296 of the reference), step for step and type for type:
// base in fp32 (joint 6, or the fp32 mean of joints 11 and 12), promoted to fp64; position = base - side / 2 in fp64; both rounded to fp32.
// One lane per (sample, axis).
__global__ void cuboid_from_keypoints_kernel(const float* __restrict__ kp, int n, int J, int coco, double half, float* __restrict__ pos,
                                             float* __restrict__ center) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const int b = g / 3, k = g - 3 * b;
    const float* s = kp + (size_t)b * J * 3 + k;
    float base32;
    if (coco) base32 = __fdiv_rn(__fadd_rn(s[11 * 3], s[12 * 3]), 2.0f);
    else base32 = s[6 * 3];
    const double base = (double)base32;
    center[g] = (float)base;
    pos[g] = (float)__dsub_rn(base, half);
}
}  // namespace

extern "C" int lt_cuboid_from_keypoints(const float* keypoints_3d, int32_t B, int32_t J, int32_t kind, double cuboid_side, float* pos, float* center,
                                        void* stream) {
    LT_REQUIRE(keypoints_3d && pos && center, LT_ERR_INVALID, "lt_cuboid_from_keypoints: null argument (keypoints_3d, pos and center are required)");
    LT_REQUIRE(kind == LT_KIND_MPII || kind == LT_KIND_COCO, LT_ERR_INVALID, "lt_cuboid_from_keypoints: kind %d (LT_KIND_MPII | LT_KIND_COCO)", kind);
    LT_REQUIRE(B >= 1 && (long long)B * 3 < (1ll << 31), LT_ERR_INVALID, "lt_cuboid_from_keypoints: B %d", B);
    const int need = kind == LT_KIND_COCO ? 13 : 7;
    LT_REQUIRE(J >= need, LT_ERR_INVALID, "lt_cuboid_from_keypoints: J %d joints, kind '%s' reads joint %d", J, kind == LT_KIND_COCO ? "coco" : "mpii", need - 1);
    const int n = B * 3;
    hipLaunchKernelGGL(cuboid_from_keypoints_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, keypoints_3d, n, J,
                       kind == LT_KIND_COCO ? 1 : 0, cuboid_side / 2.0, pos, center);
    LT_CHECK_LAUNCH("lt_cuboid_from_keypoints");
    return LT_OK;
}
