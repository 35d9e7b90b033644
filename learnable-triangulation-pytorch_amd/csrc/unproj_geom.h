// The one statement of the unprojection's geometry: the projection of a voxel centre into a view and the bilinear tap set that follows
// from it -- op.py:116-141, multiview.py:105 and ATen's grid_sampler_2d (bilinear, zeros padding, align_corners=True), every step a single
// IEEE rounding in the reference's order.  The forward (unproject.hip) and the backward (unproject_bwd.hip), which redoes the forward's
// sampling, both take their taps from project_taps() below, so the two cannot drift apart.
//
// Two division flavours (FAST): false = IEEE divisions (__fdiv_rn), the fp32 parity path; true = a * v_rcp_f32(b), the bf16 throughput
// path of the forward (generic and quad kernel).  The backward uses FAST == false for bf16 maps too: its taps are those of the fp32
// forward whatever the maps' type.
//
// Two load disciplines, both fed by the same project_taps() result:
//   * the generic forward (sample_view) loads only the corners that are inside the map (FullTap::xw_ok .. ys_ok) and multiplies by the raw
//     weights (FullTap::wt); a corner that is padding contributes an exact 0;
//   * the quad kernel and the backward load all four corners at addresses clamped into the map (Tap::x, Tap::y, FullTap::off) and multiply
//     by weights that are 0 where the corner is padding or the depth is <= 0 (Tap::k).
// On finite feature maps the two agree bit for bit (0 * finite = 0).  They differ by design where a padding corner's clamped neighbour is
// Inf or NaN: the first never reads it, the second multiplies it by 0.
//
// The result is a struct of scalars and everything here is inlined: a field its user does not read is dead code and costs nothing.  The
// shape of this header is held to the kernels' machine code ("One voxel-projection routine"): the backward's kernels compile to
// the instruction streams they had with their own copy, the quad kernels to the same instructions in another order.  Three things keep it
// so, and look arbitrary otherwise: the fields the backward keeps per view are the base struct Tap, of its old size and field order;
// tap_pixels takes the patch's columns and rows by value (a `+ 1` inside it, or a Tap& argument, is simplified differently before it is
// inlined); FullTap::off is formed between the clamps and the weights, where the quad kernel formed its addresses.
#pragma once
#include "lt_common.h"

namespace lt {

// fp32 (parity) mode keeps IEEE divisions / expf; bf16 (throughput) mode uses v_rcp_f32 / v_exp_f32: the forward was
// issue-bound (PMC: SQ_WAIT_INST_ANY 40 %, ~50 IEEE divisions + 32 expf per lane-item), not memory-bound.
template <bool FAST> __device__ __forceinline__ float div_(float a, float b) { return FAST ? a * __builtin_amdgcn_rcpf(b) : __fdiv_rn(a, b); }
template <bool FAST> __device__ __forceinline__ float exp_(float x) { return FAST ? __expf(x) : expf(x); }

template <typename T, int CH> struct ChVec;  // CH channels of one pixel <-> CH floats
template <> struct ChVec<float, 4> {
    static __device__ __forceinline__ void ld(const float* p, float (&f)[4]) {
        const float4 v = *(const float4*)p;
        f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
    }
    static __device__ __forceinline__ void st(float* p, const float (&f)[4]) { *(float4*)p = make_float4(f[0], f[1], f[2], f[3]); }
};
template <> struct ChVec<float, 1> {
    static __device__ __forceinline__ void ld(const float* p, float (&f)[1]) { f[0] = *p; }
    static __device__ __forceinline__ void st(float* p, const float (&f)[1]) { *p = f[0]; }
};
template <> struct ChVec<bf16_t, 8> {
    static __device__ __forceinline__ void ld(const bf16_t* p, float (&f)[8]) {
        const uint4 v = *(const uint4*)p;
        const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f[2 * i] = __uint_as_float(u[i] << 16);
            f[2 * i + 1] = __uint_as_float(u[i] & 0xffff0000u);
        }
    }
    static __device__ __forceinline__ void st(bf16_t* p, const float (&f)[8]) {
        *(uint4*)p = make_uint4(pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]), pack_bf16x2(f[4], f[5]), pack_bf16x2(f[6], f[7]));
    }
};
template <> struct ChVec<bf16_t, 4> {        // the backward's channel vector (it reads bf16 maps and writes fp32 gradients: no st)
    static __device__ __forceinline__ void ld(const bf16_t* p, float (&f)[4]) {
        const uint2 v = *(const uint2*)p;
        f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
        f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
    }
};
template <> struct ChVec<bf16_t, 1> {
    static __device__ __forceinline__ void ld(const bf16_t* p, float (&f)[1]) { f[0] = bf16_to_f32(*p); }
    static __device__ __forceinline__ void st(bf16_t* p, const float (&f)[1]) { *p = f32_to_bf16(f[0]); }
};

// One view's projection of one voxel.  Corner order everywhere: (x0, y0) (x0+1, y0) (x0, y0+1) (x0+1, y0+1).
struct Tap {                 // what the second discipline reads, what the backward keeps per view and what its K0 records
    int x[4], y[4];          // the corners' pixels, clamped into the map
    float k[4];              // wt where the corner is inside the map and act, else 0
    int x0, y0;              // unclamped origin of the 2x2 patch (>= -1; 0 when !act)
};
struct FullTap : Tap {       // project_taps' whole result; the backward slices it to Tap
    bool act;                // depth > 0 and at least one corner inside the map; otherwise the sample is 0
    bool xw_ok, xe_ok, yn_ok, ys_ok;   // column x0 / column x0+1 / row y0 / row y0+1 is inside the map (says nothing about the depth)
    float wt[4];             // raw bilinear weights
    int off[4];              // base + (y * w + x) * pitch of the clamped corners: element offsets in channels-last maps of `pitch` channels
};

// the corners' pixels from the patch's two columns and two rows, clamped into the map: project_taps and tap_of_record, its inverse, share them
__device__ __forceinline__ void tap_pixels(int xw, int xe, int yn, int ys, int h, int w, int (&x)[4], int (&y)[4]) {
    const int xwc = min(max(xw, 0), w - 1), xec = min(max(xe, 0), w - 1);
    const int ync = min(max(yn, 0), h - 1), ysc = min(max(ys, 0), h - 1);
    x[0] = xwc; x[1] = xec; x[2] = xwc; x[3] = xec;
    y[0] = ync; y[1] = ync; y[2] = ysc; y[3] = ysc;
}

// rcp_h, rcp_w: v_rcp_f32 of (float)h, (float)w, read by the FAST form only (u * rcp(h) is div_<true>(u, (float)h): a caller may hoist them);
// pitch, base: see FullTap::off
template <bool FAST>
__device__ __forceinline__ FullTap project_taps(const float* __restrict__ P, float X0, float X1, float X2, int h, int w, float rcp_h, float rcp_w,
                                                int pitch = 0, int base = 0) {
    // multiview.py:105: [X,1] @ P^T, k-ordered
    const float px = __fadd_rn(fmaf(X2, P[2], fmaf(X1, P[1], __fmul_rn(X0, P[0]))), P[3]);
    const float py = __fadd_rn(fmaf(X2, P[6], fmaf(X1, P[5], __fmul_rn(X0, P[4]))), P[7]);
    float pz = __fadd_rn(fmaf(X2, P[10], fmaf(X1, P[9], __fmul_rn(X0, P[8]))), P[11]);
    const bool invalid = pz <= 0.0f;  // op.py:123; op.py:141: the sample is computed, then zeroed
    if (pz == 0.0f) pz = 1.0f;        // op.py:125
    const float u = div_<FAST>(px, pz), v = div_<FAST>(py, pz);
    // op.py:128-129: x normalised by heatmap_shape[0] (= h), y by heatmap_shape[1] (= w)
    const float gx = __fmul_rn(2.0f, __fsub_rn(FAST ? u * rcp_h : __fdiv_rn(u, (float)h), 0.5f));
    const float gy = __fmul_rn(2.0f, __fsub_rn(FAST ? v * rcp_w : __fdiv_rn(v, (float)w), 0.5f));
    // grid_sample, align_corners=True: pixel = (g + 1) * (size - 1) / 2
    const float ix = __fmul_rn(__fadd_rn(gx, 1.0f), 0.5f * (float)(w - 1));
    const float iy = __fmul_rn(__fadd_rn(gy, 1.0f), 0.5f * (float)(h - 1));
    const float xw = floorf(ix), yn = floorf(iy);
    const float we = __fsub_rn(ix, xw), ww = __fsub_rn(1.0f, we);
    const float ws = __fsub_rn(iy, yn), wn = __fsub_rn(1.0f, ws);
    // in-range tests in float (huge / NaN coordinates never convert to int)
    const bool xw_ok = xw >= 0.f && xw <= (float)(w - 1), xe_ok = xw >= -1.f && xw <= (float)(w - 2);
    const bool yn_ok = yn >= 0.f && yn <= (float)(h - 1), ys_ok = yn >= -1.f && yn <= (float)(h - 2);
    const bool act = !invalid && (xw_ok || xe_ok) && (yn_ok || ys_ok);
    const int x0 = act ? (int)xw : 0, y0 = act ? (int)yn : 0;
    FullTap t;
    t.x0 = x0; t.y0 = y0;
    tap_pixels(x0, x0 + 1, y0, y0 + 1, h, w, t.x, t.y);
    t.off[0] = base + (t.y[0] * w + t.x[0]) * pitch; t.off[1] = base + (t.y[1] * w + t.x[1]) * pitch;
    t.off[2] = base + (t.y[2] * w + t.x[2]) * pitch; t.off[3] = base + (t.y[3] * w + t.x[3]) * pitch;
    t.k[0] = (act && yn_ok && xw_ok) ? __fmul_rn(wn, ww) : 0.f;
    t.k[1] = (act && yn_ok && xe_ok) ? __fmul_rn(wn, we) : 0.f;
    t.k[2] = (act && ys_ok && xw_ok) ? __fmul_rn(ws, ww) : 0.f;
    t.k[3] = (act && ys_ok && xe_ok) ? __fmul_rn(ws, we) : 0.f;
    t.act = act; t.xw_ok = xw_ok; t.xe_ok = xe_ok; t.yn_ok = yn_ok; t.ys_ok = ys_ok;
    t.wt[0] = __fmul_rn(wn, ww); t.wt[1] = __fmul_rn(wn, we); t.wt[2] = __fmul_rn(ws, ww); t.wt[3] = __fmul_rn(ws, we);
    return t;
}
template <bool FAST>
__device__ __forceinline__ FullTap project_taps(const float* __restrict__ P, float X0, float X1, float X2, int h, int w) {
    return project_taps<FAST>(P, X0, X1, X2, h, w, FAST ? __builtin_amdgcn_rcpf((float)h) : 0.f, FAST ? __builtin_amdgcn_rcpf((float)w) : 0.f);
}

// The backward's K0 packs a Tap as txy = (x0 + 1) | (y0 + 1) << 16 and tw = k[0..3]; this is the inverse: the x0, y0, x, y and k that
// project_taps returned (act, the in-range flags and wt are not recorded: the record's users read clamped pixels and zeroed weights only)
__device__ __forceinline__ Tap tap_of_record(int xy, const float4 k, int h, int w) {
    Tap t;
    t.x0 = (xy & 0xffff) - 1; t.y0 = (xy >> 16) - 1;
    tap_pixels(t.x0, t.x0 + 1, t.y0, t.y0 + 1, h, w, t.x, t.y);
    t.k[0] = k.x; t.k[1] = k.y; t.k[2] = k.z; t.k[3] = k.w;
    return t;
}

// Host side: the descriptor of the shorthand entries (lt_unproject_fwd, lt_unproject_bwd and their kin) -- the coordinate form, plain; a shorthand
// then sets the pointers of its variant
inline lt_unproject_desc unproject_coord_desc(int dtype, const void* feats, const float* proj, const float* coords, const float* conf, int B, int NV, int C,
                                              int h, int w, int v0, int v1, int v2, int agg) {
    lt_unproject_desc d = {};
    d.dtype = dtype; d.feats = feats; d.proj = proj; d.coords = coords; d.conf = conf;
    d.B = B; d.NV = NV; d.C = C; d.h = h; d.w = w; d.v0 = v0; d.v1 = v1; d.v2 = v2; d.agg = agg;
    return d;
}

}  // namespace lt
