// RANSACTriangulationNet (reference mvn/models/triangulation.py:17-128): the heatmap argmax and the batched RANSAC triangulation.
//
// lt_heatmap_argmax_nchw_f32: ONE pass over the backbone's fp32 NHWC heatmaps writes the raw NCHW heatmaps the model returns and
// the per-(image, joint) argmax of torch.max(hm.view(N, J, -1), -1) (a NaN wins, the first NaN's index; among equal values the
// smallest index), plus the reference's int64 keypoints (:45-52).  One workgroup per image walks it in 256-pixel chunks staged
// through an LDS tile with an odd row stride (coalesced NHWC reads, coalesced NCHW rows, conflict-free per-joint column reads);
// the running (value, index) per joint and lane stays in LDS and is reduced across the wave at the end: no atomics, no workspace.
//
// lt_triangulate_ransac: one lane per (sample, joint) problem, fp64 throughout (the reference's numpy fp64 on fp32 projection
// matrices and integer points).  Every DLT (multiview.py:113-138) streams the rows of A (2n x 4) through Givens rotations into a
// 4x4 upper-triangular R (A = QR, same right singular vectors and the same condition number: A^T A would square it), then runs a
// one-sided Jacobi SVD on R: the routine of csrc/dlt.h, shared with lt_triangulate_dlt and the algebraic tails.
// Hypotheses are 2-view DLTs; the inlier set is the pair plus every view whose reprojection error
// r_v = 1/2 |p_v - pi_v(X)| (multiview.py:186-193) is < eps, kept only when strictly larger than the best so far (:84-97).
// The final DLT uses the inlier views; with direct_opt, Levenberg-Marquardt minimises scipy's least_squares(loss='huber')
// objective 0.5 sum_v rho(r_v^2) over them, with IRLS weights rho'(r_v^2) on both 2D components of view v (exact for this
// objective and smooth at r_v = 0) and analytic Jacobians, started from the inlier DLT point and from one DLT per inlier view with
// that view pinned (the objective is multimodal when residuals sit in Huber's linear regime); the lowest cost wins.
#include "lt_common.h"
#include "dlt.h"

using namespace lt;

namespace {

// ---- heatmap argmax fused with the NHWC -> NCHW layout change --------------------------------------------------------------------
constexpr int AM_TP = 256;     // pixels per chunk (= threads per workgroup)
constexpr int AM_JMAX = 32;    // LDS: 256 x 33 tile + 2 x 32 x 64 running states = 50 KB

// a beats b: a NaN beats every number (the smaller index among NaNs); otherwise the larger value, the smaller index on a tie.
// A total preorder, so the combine below is associative and commutative: any reduction order gives torch's answer.
__device__ __forceinline__ bool am_beats(float a, int ia, float b, int ib) {
    const bool na = a != a, nb = b != b;
    if (na || nb) return na && (!nb || ia < ib);
    return a > b || (a == b && ia < ib);
}

__global__ __launch_bounds__(AM_TP) void hm_argmax_kernel(const float* __restrict__ x, int ld, float* __restrict__ y, int64_t* __restrict__ idx_out,
                                                          int64_t* __restrict__ kp, int J, int HW, int w, float sx, float sy) {
    extern __shared__ float smem[];
    const int ts = J | 1;
    float* tile = smem;                                   // [AM_TP][ts]
    float* bv = smem + AM_TP * ts;                        // [J][64] running best value per (joint, lane)
    int* bi = (int*)(bv + J * 64);                        // [J][64] its flat index
    const int n = blockIdx.x, t = threadIdx.x, wv = t >> 6, lane = t & 63;
    for (int c = wv; c < J; c += AM_TP / 64) { bv[c * 64 + lane] = -INFINITY; bi[c * 64 + lane] = 0x7fffffff; }
    const float* xn = x + (long long)n * HW * ld;
    float* yn = y + (long long)n * J * HW;
    for (int p0 = 0; p0 < HW; p0 += AM_TP) {
        const int np = min(AM_TP, HW - p0);
        __syncthreads();
        for (int i = t; i < np * J; i += AM_TP) {
            const int p = i / J, c = i - p * J;
            tile[p * ts + c] = xn[(long long)(p0 + p) * ld + c];
        }
        __syncthreads();
        if (t < np)
            for (int c = 0; c < J; ++c) yn[(long long)c * HW + p0 + t] = tile[t * ts + c];
        for (int c = wv; c < J; c += AM_TP / 64) {       // each (joint, lane) state belongs to one wave: no race across waves
            float v = bv[c * 64 + lane];
            int id = bi[c * 64 + lane];
#pragma unroll
            for (int k = 0; k < AM_TP / 64; ++k) {
                const int p = lane + 64 * k;
                if (p < np) {
                    const float cv = tile[p * ts + c];
                    if (am_beats(cv, p0 + p, v, id)) { v = cv; id = p0 + p; }
                }
            }
            bv[c * 64 + lane] = v;
            bi[c * 64 + lane] = id;
        }
    }
    for (int c = wv; c < J; c += AM_TP / 64) {
        float v = bv[c * 64 + lane];
        int id = bi[c * 64 + lane];
        for (int off = 32; off >= 1; off >>= 1) {
            const float ov = __shfl_xor(v, off, 64);
            const int oi = __shfl_xor(id, off, 64);
            if (am_beats(ov, oi, v, id)) { v = ov; id = oi; }
        }
        if (lane == 0) {
            const long long o = (long long)n * J + c;
            if (idx_out) idx_out[o] = id;
            if (kp) {
                // reference :49-51: float32 products (int64 tensor * Python float) stored into an int64 tensor (truncation)
                const int xx = id % w, yy = id / w;
                kp[o * 2] = (int64_t)((float)xx * sx);
                kp[o * 2 + 1] = (int64_t)((float)yy * sy);
            }
        }
    }
}

// ---- RANSAC triangulation ----------------------------------------------------------------------------------------------------
constexpr int RS_MAX_NV = 32;    // inlier sets are 32-bit masks
constexpr int RS_LM_ITERS = 200; // Levenberg-Marquardt iteration cap per start (accepted + rejected steps)
constexpr double RS_PIN = 1e3;   // row weight of the pinned view in the extra starts' DLT

struct RansacArgs {
    const float* proj;      // [B][NV][3][4]
    const int64_t* pts;     // [B][NV][J][2]
    const int32_t* pairs;   // [B][J][n_iters][2] or null (every pair, lexicographic)
    float* kp3d;            // [B][J][3]
    uint8_t* inliers;       // [B][J][NV] or null
    double eps;
    int n_iters, direct, B, NV, J;
};

struct Problem {
    const float* P;         // this sample's NV matrices
    const int64_t* pts;     // this sample's points, joint j: pts[(v * J + j) * 2]
    int J, j, NV;
    __device__ __forceinline__ double px(int v) const { return (double)pts[((long long)v * J + j) * 2]; }
    __device__ __forceinline__ double py(int v) const { return (double)pts[((long long)v * J + j) * 2 + 1]; }
};

// DLT of the views in mask (the routine of dlt.h on the integer points); view `pin` (or -1) has its rows weighted by RS_PIN: a point close to that view's ray
__device__ __forceinline__ void dlt(const Problem& pb, unsigned mask, double (&X)[3], int pin = -1) {
    double R[4][4] = {};
    for (int v = 0; v < pb.NV; ++v)
        if ((mask >> v) & 1u) dlt_add_view(R, pb.P + v * 12, pb.px(v), pb.py(v), v == pin ? RS_PIN : 1.0);
    dlt_point(R, X);
}

// projection of X by view v (numpy: homogeneous X @ P.T, then divide), the residual e = p - pi(X) and q = P [X; 1]
__device__ __forceinline__ void project(const float* P, const double X[3], double q[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
        q[r] = X[0] * (double)P[4 * r] + X[1] * (double)P[4 * r + 1] + X[2] * (double)P[4 * r + 2] + (double)P[4 * r + 3];
}

__device__ __forceinline__ double reproj_err(const Problem& pb, int v, const double X[3]) {
    double q[3];
    project(pb.P + v * 12, X, q);
    const double dx = pb.px(v) - q[0] / q[2], dy = pb.py(v) - q[1] / q[2];
    return 0.5 * sqrt(dx * dx + dy * dy);
}

// scipy's objective: 0.5 sum_v rho(r_v^2), rho(z) = z (z <= 1), 2 sqrt(z) - 1 (z > 1).  front: bit v set = X must stay in front of
// camera v's principal plane (sign of q_2 as at the start): +inf otherwise, so that no step jumps through infinity
__device__ __forceinline__ double huber_cost(const Problem& pb, unsigned mask, const double X[3], unsigned front) {
    double c = 0;
    for (int v = 0; v < pb.NV; ++v) {
        if (!((mask >> v) & 1u)) continue;
        double q[3];
        project(pb.P + v * 12, X, q);
        if ((q[2] > 0.0) != (bool)((front >> v) & 1u)) return INFINITY;
        const double dx = pb.px(v) - q[0] / q[2], dy = pb.py(v) - q[1] / q[2];
        const double z = 0.25 * (dx * dx + dy * dy), r = sqrt(z);
        c += z <= 1.0 ? z : 2.0 * r - 1.0;
    }
    return 0.5 * c;
}

// Levenberg-Marquardt from X; returns the cost reached
__device__ double huber_lm(const Problem& pb, unsigned mask, double X[3]) {
    unsigned front = 0;
    for (int v = 0; v < pb.NV; ++v) {
        double q[3];
        project(pb.P + v * 12, X, q);
        front |= (q[2] > 0.0 ? 1u : 0u) << v;
    }
    double cost = huber_cost(pb, mask, X, front);
    double lam = 1e-3;
    for (int it = 0; it < RS_LM_ITERS; ++it) {
        // IRLS normal equations at X: sum_v w_v J_v^T J_v delta = -sum_v w_v J_v^T e_v, J_v = d e_v / d X = -d pi_v / d X
        double Hm[3][3] = {}, g[3] = {};
        for (int v = 0; v < pb.NV; ++v) {
            if (!((mask >> v) & 1u)) continue;
            const float* P = pb.P + v * 12;
            double q[3];
            project(P, X, q);
            const double u = q[0] / q[2], w = q[1] / q[2];
            const double ex = pb.px(v) - u, ey = pb.py(v) - w;
            const double z = 0.25 * (ex * ex + ey * ey);
            const double wt = z <= 1.0 ? 1.0 : 1.0 / sqrt(z);            // rho'(r^2)
            double jx[3], jy[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                jx[k] = -((double)P[k] - u * (double)P[8 + k]) / q[2];
                jy[k] = -((double)P[4 + k] - w * (double)P[8 + k]) / q[2];
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                g[a] += wt * (jx[a] * ex + jy[a] * ey);
#pragma unroll
                for (int b = 0; b < 3; ++b) Hm[a][b] += wt * (jx[a] * jx[b] + jy[a] * jy[b]);
            }
        }
        // (Hm + lam diag(Hm)) delta = -g by Cramer's rule (3x3, symmetric positive definite for lam > 0 unless Hm is singular)
        const double a00 = Hm[0][0] * (1 + lam), a11 = Hm[1][1] * (1 + lam), a22 = Hm[2][2] * (1 + lam);
        const double a01 = Hm[0][1], a02 = Hm[0][2], a12 = Hm[1][2];
        const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
        const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
        const double det = a00 * c00 + a01 * c01 + a02 * c02;
        if (!(det > 0.0)) break;
        const double d0 = -(c00 * g[0] + c01 * g[1] + c02 * g[2]) / det;
        const double d1 = -(c01 * g[0] + c11 * g[1] + c12 * g[2]) / det;
        const double d2 = -(c02 * g[0] + c12 * g[1] + c22 * g[2]) / det;
        const double Xn[3] = {X[0] + d0, X[1] + d1, X[2] + d2};
        const double cn = huber_cost(pb, mask, Xn, front);
        const double step = sqrt(d0 * d0 + d1 * d1 + d2 * d2), xn = sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
        if (cn < cost) {
            const double dec = cost - cn;
            X[0] = Xn[0]; X[1] = Xn[1]; X[2] = Xn[2];
            cost = cn;
            lam = fmax(lam * 0.1, 1e-12);
            if (dec <= 1e-15 * cost || step <= 1e-14 * (xn + 1e-14)) break;
        } else {
            if (step <= 1e-14 * (xn + 1e-14)) break;      // no smaller step can decrease the cost measurably
            lam *= 10.0;
            if (lam > 1e16) break;
        }
    }
    return cost;
}

// With views in Huber's linear regime (r_v > 1: a sum of distances) the objective has a local minimum near each view's ray, and
// the one scipy's trust region reaches from the DLT point need not be the one LM reaches.  So LM also starts from a DLT with each
// inlier view pinned (its rows weighted by RS_PIN); the lowest cost wins.
__device__ void huber_refine(const Problem& pb, unsigned mask, double X[3]) {
    double best[3] = {X[0], X[1], X[2]};
    double cbest = huber_lm(pb, mask, best);
    for (int v = 0; v < pb.NV; ++v) {
        if (!((mask >> v) & 1u)) continue;
        double Y[3];
        dlt(pb, mask, Y, v);
        const double c = huber_lm(pb, mask, Y);
        if (c < cbest) { cbest = c; best[0] = Y[0]; best[1] = Y[1]; best[2] = Y[2]; }
    }
    X[0] = best[0]; X[1] = best[1]; X[2] = best[2];
}

__global__ __launch_bounds__(64) void ransac_kernel(const RansacArgs a) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.B * a.J) return;
    const int b = g / a.J, j = g - b * a.J;
    Problem pb;
    pb.P = a.proj + (long long)b * a.NV * 12;
    pb.pts = a.pts + (long long)b * a.NV * a.J * 2;
    pb.J = a.J; pb.j = j; pb.NV = a.NV;
    unsigned best = 0;
    int nbest = 0;
    const int niters = a.pairs ? a.n_iters : a.NV * (a.NV - 1) / 2;
    int p0 = 0, p1 = 1;                 // exhaustive mode: (0,1), (0,2), ..., (0,NV-1), (1,2), ...
    for (int it = 0; it < niters; ++it) {
        int s0 = p0, s1 = p1;
        if (a.pairs) {
            const int32_t* pr = a.pairs + ((long long)g * a.n_iters + it) * 2;
            s0 = pr[0]; s1 = pr[1];
            if (s0 < 0 || s1 < 0 || s0 >= a.NV || s1 >= a.NV || s0 == s1) continue;   // never read outside the problem
        } else if (++p1 == a.NV) {
            ++p0; p1 = p0 + 1;
        }
        const unsigned pair = (1u << s0) | (1u << s1);
        double X[3];
        dlt(pb, pair, X);
        unsigned set = pair;
        for (int v = 0; v < a.NV; ++v)
            if (reproj_err(pb, v, X) < a.eps) set |= 1u << v;
        const int ns = __popc(set);
        if (ns > nbest) { nbest = ns; best = set; }
    }
    if (nbest == 0) best = a.NV == 32 ? 0xffffffffu : (1u << a.NV) - 1u;   // reference :100-101 (only when no draw was valid)
    double X[3];
    dlt(pb, best, X);
    if (a.direct) huber_refine(pb, best, X);
    float* o = a.kp3d + (long long)g * 3;
    o[0] = (float)X[0]; o[1] = (float)X[1]; o[2] = (float)X[2];
    if (a.inliers)
        for (int v = 0; v < a.NV; ++v) a.inliers[(long long)g * a.NV + v] = (uint8_t)((best >> v) & 1u);
}

}  // namespace

extern "C" int lt_heatmap_argmax_nchw_f32(const float* heatmaps, int32_t ld, float* heatmaps_nchw, int64_t* indices, int64_t* keypoints,
                                          int32_t N, int32_t J, int32_t h, int32_t w, int32_t image_h, int32_t image_w, void* stream) {
    LT_REQUIRE(heatmaps && heatmaps_nchw, LT_ERR_INVALID, "lt_heatmap_argmax_nchw_f32: null argument");
    LT_REQUIRE(N >= 1 && J >= 1 && h >= 1 && w >= 1 && ld >= J, LT_ERR_INVALID, "lt_heatmap_argmax_nchw_f32: bad shape");
    LT_REQUIRE(!keypoints || (image_h >= 1 && image_w >= 1), LT_ERR_INVALID, "lt_heatmap_argmax_nchw_f32: bad image size");
    LT_REQUIRE(J <= AM_JMAX, LT_ERR_UNSUPPORTED, "lt_heatmap_argmax_nchw_f32: J=%d > %d", J, AM_JMAX);
    LT_REQUIRE((long long)h * w < (1ll << 31) && (long long)h * w * ld < (1ll << 40), LT_ERR_UNSUPPORTED, "lt_heatmap_argmax_nchw_f32: heatmap too large");
    const size_t lds = ((size_t)AM_TP * (J | 1) + (size_t)J * 64 * 2) * sizeof(float);
    const float sx = (float)((double)image_w / (double)w), sy = (float)((double)image_h / (double)h);
    hipLaunchKernelGGL(hm_argmax_kernel, dim3(N), dim3(AM_TP), lds, (hipStream_t)stream, heatmaps, ld, heatmaps_nchw, indices, keypoints, J, h * w, w, sx, sy);
    LT_CHECK_LAUNCH("lt_heatmap_argmax_nchw_f32");
    return LT_OK;
}

extern "C" int lt_triangulate_ransac(const float* proj, const int64_t* points, const int32_t* pairs, int32_t n_iters, double eps, int32_t direct_opt,
                                     float* out_kp3d, uint8_t* out_inliers, int32_t B, int32_t NV, int32_t J, void* stream) {
    LT_REQUIRE(proj && points && out_kp3d, LT_ERR_INVALID, "lt_triangulate_ransac: null argument");
    LT_REQUIRE(B >= 1 && J >= 1, LT_ERR_INVALID, "lt_triangulate_ransac: bad shape");
    LT_REQUIRE(NV >= 2 && NV <= RS_MAX_NV, LT_ERR_UNSUPPORTED, "lt_triangulate_ransac: NV=%d views (2 <= NV <= %d)", NV, RS_MAX_NV);
    LT_REQUIRE(!pairs || n_iters >= 1, LT_ERR_INVALID, "lt_triangulate_ransac: n_iters=%d with a pair schedule", n_iters);
    LT_REQUIRE((long long)B * J < (1ll << 31), LT_ERR_UNSUPPORTED, "lt_triangulate_ransac: too many problems");
    RansacArgs a;
    a.proj = proj; a.pts = points; a.pairs = pairs; a.kp3d = out_kp3d; a.inliers = out_inliers;
    a.eps = eps; a.n_iters = n_iters; a.direct = direct_opt; a.B = B; a.NV = NV; a.J = J;
    hipLaunchKernelGGL(ransac_kernel, dim3((unsigned)((B * J + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
    LT_CHECK_LAUNCH("lt_triangulate_ransac");
    return LT_OK;
}
