// Soft-argmax reductions (3D: op.integrate_tensor_3d_with_coordinates, 2D: op.integrate_tensor_2d),
// the confidence-weighted DLT (multiview.triangulate_batch_of_points) and the algebraic model's tail after the 2D soft-argmax.
//
// 3D soft-argmax is HBM-bound: read J x V^3 logits (twice: statistics, then normalise) and write the
// J x V^3 probabilities the API returns.  One lane owns one voxel and walks the J joints with an online
// (max, sum, sum*coord) state per joint in registers, so the voxel's coordinates are read once for all
// joints; channels-last logits are staged through an LDS tile with an odd row stride, which turns the
// strided per-joint walk into conflict-free LDS reads while global loads stay fully coalesced.
// Planar logits ((B, J, V^3), what lt_pwchain_fwd writes for the bf16 V2V tail) need no staging: a lane owns FOUR consecutive
// voxels, every joint is one 16-byte load per lane (all J of them in flight at once) and the probabilities are written by a
// plain vectorised elementwise pass.
#include "lt_common.h"
#include "dlt.h"

using namespace lt;

namespace {

constexpr int SA_ITERS = 8;                  // voxels per lane
constexpr int SA_CHUNK = 256 * SA_ITERS;     // voxels per workgroup
constexpr int SA_REC = 5;                    // partial record: m, s, sx, sy, sz
typedef float sa_f32x4 __attribute__((ext_vector_type(4)));

struct SA3Args {
    const float* logits;
    const float* coords;
    float* partial;   // [B][J][nchunks][5]
    float* stats;     // [B][J][2] = max, sum
    float* kp;        // [B][J][3]
    float* probs;     // [B][J][nvox] or null
    float mult;
    int softmax, J, ld, nchunks;
    long long nvox;
};

// stage a [nv][J] tile of channels-last logits into LDS (row stride J|1 -> odd)
__device__ __forceinline__ void stage_cl(const SA3Args& a, const float* src_b, long long vox0, int nv, float* tile, int ts) {
    if (a.ld == a.J) {
        const float* src = src_b + vox0 * a.J;
        for (int i = threadIdx.x; i < nv * a.J; i += 256) {
            const int v = i / a.J;
            tile[v * ts + (i - v * a.J)] = src[i];
        }
    } else {
        for (int i = threadIdx.x; i < nv * a.J; i += 256) {
            const int v = i / a.J, j = i - v * a.J;
            tile[v * ts + j] = src_b[(vox0 + v) * a.ld + j];
        }
    }
}

template <int JP, bool CL>
__global__ __launch_bounds__(256, (JP <= 17 ? 3 : 2)) void sa3_partial_kernel(const SA3Args a) {   // 3 workgroups per SIMD-quad fit at <= 17 joints (152 VGPRs)
    extern __shared__ float smem[];
    const int ts = a.J | 1;
    float* tile = smem;                       // CL only: [256][ts]
    float* red = smem + (CL ? 256 * ts : 0);  // [4][JP][5]
    const int b = blockIdx.y, chunk = blockIdx.x;
    const float* lg = a.logits + (long long)b * a.J * a.nvox;
    const float* cd = a.coords + (long long)b * a.nvox * 3;
    float m[JP], s[JP], sx[JP], sy[JP], sz[JP];
#pragma unroll
    for (int j = 0; j < JP; ++j) { m[j] = -INFINITY; s[j] = sx[j] = sy[j] = sz[j] = 0.f; }
    for (int it = 0; it < SA_ITERS; ++it) {
        const long long vox0 = (long long)chunk * SA_CHUNK + it * 256;
        if (vox0 >= a.nvox) break;
        const int nv = (int)min((long long)256, a.nvox - vox0);
        if (CL) {
            __syncthreads();
            stage_cl(a, lg, vox0, nv, tile, ts);
            __syncthreads();
        }
        const int t = threadIdx.x;
        if (t < nv) {
            const long long vox = vox0 + t;
            const float cx = cd[vox * 3], cy = cd[vox * 3 + 1], cz = cd[vox * 3 + 2];
#pragma unroll
            for (int j = 0; j < JP; ++j) {
                if (j < a.J) {
                    const float x = a.mult * (CL ? tile[t * ts + j] : lg[(long long)j * a.nvox + vox]);
                    if (a.softmax) {
                        const float mn = fmaxf(m[j], x);
                        const float sc = expf(m[j] - mn), e = expf(x - mn);  // m = -inf -> sc = 0
                        s[j] = s[j] * sc + e;
                        sx[j] = sx[j] * sc + e * cx;
                        sy[j] = sy[j] * sc + e * cy;
                        sz[j] = sz[j] * sc + e * cz;
                        m[j] = mn;
                    } else {
                        const float p = fmaxf(x, 0.f);
                        s[j] += p; sx[j] += p * cx; sy[j] += p * cy; sz[j] += p * cz;
                        m[j] = 0.f;
                    }
                }
            }
        }
    }
    // wave reduction (64 lanes), then the 4 waves through LDS
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < JP; ++j) {
        if (j < a.J) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const float m2 = __shfl_xor(m[j], off), s2 = __shfl_xor(s[j], off);
                const float x2 = __shfl_xor(sx[j], off), y2 = __shfl_xor(sy[j], off), z2 = __shfl_xor(sz[j], off);
                const float mn = fmaxf(m[j], m2);
                const float c1 = (m[j] == -INFINITY) ? 0.f : expf(m[j] - mn), c2 = (m2 == -INFINITY) ? 0.f : expf(m2 - mn);
                s[j] = s[j] * c1 + s2 * c2; sx[j] = sx[j] * c1 + x2 * c2; sy[j] = sy[j] * c1 + y2 * c2; sz[j] = sz[j] * c1 + z2 * c2;
                m[j] = mn;
            }
            if (lane == 0) {
                float* r = red + (wave * JP + j) * SA_REC;
                r[0] = m[j]; r[1] = s[j]; r[2] = sx[j]; r[3] = sy[j]; r[4] = sz[j];
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < a.J) {
        const int j = threadIdx.x;
        float M = -INFINITY;
        for (int w = 0; w < 4; ++w) M = fmaxf(M, red[(w * JP + j) * SA_REC]);
        float S = 0.f, X = 0.f, Y = 0.f, Z = 0.f;
        for (int w = 0; w < 4; ++w) {
            const float* r = red + (w * JP + j) * SA_REC;
            const float c = (r[0] == -INFINITY) ? 0.f : expf(r[0] - M);
            S += r[1] * c; X += r[2] * c; Y += r[3] * c; Z += r[4] * c;
        }
        float* o = a.partial + (((long long)b * a.J + j) * a.nchunks + chunk) * SA_REC;
        o[0] = M; o[1] = S; o[2] = X; o[3] = Y; o[4] = Z;
    }
}

// Planar logits, nvox % 4 == 0: a lane owns SAP_V groups of four consecutive voxels (their coordinates stay in registers for
// all joints), the workgroup walks the joints: per joint one 16-byte load per group (the next joint's loads are in flight
// under this joint's arithmetic), an exact two-step softmax over the lane's 16 values, then one wave reduction
// (max -> rescale -> sums).  Register state is independent of J, so this kernel runs at 3+ waves per SIMD.
constexpr int SAP_V = 4;
constexpr int SAP_CHUNK = 256 * 4 * SAP_V;   // voxels per workgroup

__global__ __launch_bounds__(256, 3) void sa3_partial_planar_kernel(const SA3Args a) {
    __shared__ float red[32 * 4 * SA_REC];    // [J][wave][5]
    const int b = blockIdx.y, chunk = blockIdx.x;
    const float* lg = a.logits + (long long)b * a.J * a.nvox;
    const float* cd = a.coords + (long long)b * a.nvox * 3;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long vox[SAP_V];
    float wgt[SAP_V];
    sa_f32x4 ca[SAP_V], cb[SAP_V], cc[SAP_V];   // x0 y0 z0 x1 | y1 z1 x2 y2 | z2 x3 y3 z3
#pragma unroll
    for (int k = 0; k < SAP_V; ++k) {
        const long long v = (long long)chunk * SAP_CHUNK + k * 1024 + threadIdx.x * 4;
        const bool ok = v < a.nvox;          // nvox % 4 == 0: a group is inside or outside as a whole
        wgt[k] = ok ? 1.f : 0.f;             // outside: re-read group 0 (finite values of the same volume) with weight 0
        vox[k] = ok ? v : 0;
        const sa_f32x4* c4 = (const sa_f32x4*)(cd + vox[k] * 3);
        ca[k] = c4[0]; cb[k] = c4[1]; cc[k] = c4[2];
    }
    sa_f32x4 cur[SAP_V], nxt[SAP_V];
#pragma unroll
    for (int k = 0; k < SAP_V; ++k) cur[k] = *(const sa_f32x4*)(lg + vox[k]);
#pragma unroll 1
    for (int j = 0; j < a.J; ++j) {
        const float* nl = lg + (long long)min(j + 1, a.J - 1) * a.nvox;
#pragma unroll
        for (int k = 0; k < SAP_V; ++k) nxt[k] = *(const sa_f32x4*)(nl + vox[k]);
        float m = 0.f;
        if (a.softmax) {
            m = -INFINITY;
#pragma unroll
            for (int k = 0; k < SAP_V; ++k) {
                cur[k] *= a.mult;
                m = fmaxf(fmaxf(m, fmaxf(cur[k][0], cur[k][1])), fmaxf(cur[k][2], cur[k][3]));
            }
        }
        float s = 0.f, sx = 0.f, sy = 0.f, sz = 0.f;
#pragma unroll
        for (int k = 0; k < SAP_V; ++k) {
            float e0, e1, e2, e3;
            if (a.softmax) {
                e0 = expf(cur[k][0] - m); e1 = expf(cur[k][1] - m); e2 = expf(cur[k][2] - m); e3 = expf(cur[k][3] - m);
            } else {
                e0 = fmaxf(a.mult * cur[k][0], 0.f); e1 = fmaxf(a.mult * cur[k][1], 0.f);
                e2 = fmaxf(a.mult * cur[k][2], 0.f); e3 = fmaxf(a.mult * cur[k][3], 0.f);
            }
            e0 *= wgt[k]; e1 *= wgt[k]; e2 *= wgt[k]; e3 *= wgt[k];
            s += (e0 + e1) + (e2 + e3);
            sx += (e0 * ca[k][0] + e1 * ca[k][3]) + (e2 * cb[k][2] + e3 * cc[k][1]);
            sy += (e0 * ca[k][1] + e1 * cb[k][0]) + (e2 * cb[k][3] + e3 * cc[k][2]);
            sz += (e0 * ca[k][2] + e1 * cb[k][1]) + (e2 * cc[k][0] + e3 * cc[k][3]);
        }
        float M = m;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) M = fmaxf(M, __shfl_xor(M, off));
        if (a.softmax) {
            const float c = expf(m - M);
            s *= c; sx *= c; sy *= c; sz *= c;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            s += __shfl_xor(s, off); sx += __shfl_xor(sx, off); sy += __shfl_xor(sy, off); sz += __shfl_xor(sz, off);
        }
        if (lane == 0) {
            float* r = red + (j * 4 + wave) * SA_REC;
            r[0] = M; r[1] = s; r[2] = sx; r[3] = sy; r[4] = sz;
        }
#pragma unroll
        for (int k = 0; k < SAP_V; ++k) cur[k] = nxt[k];
    }
    __syncthreads();
    if (threadIdx.x < a.J) {
        const int j = threadIdx.x;
        float M = -INFINITY;
        for (int w = 0; w < 4; ++w) M = fmaxf(M, red[(j * 4 + w) * SA_REC]);
        float S = 0.f, X = 0.f, Y = 0.f, Z = 0.f;
        for (int w = 0; w < 4; ++w) {
            const float* r = red + (j * 4 + w) * SA_REC;
            const float c = expf(r[0] - M);
            S += r[1] * c; X += r[2] * c; Y += r[3] * c; Z += r[4] * c;
        }
        float* o = a.partial + (((long long)b * a.J + j) * a.nchunks + chunk) * SA_REC;
        o[0] = M; o[1] = S; o[2] = X; o[3] = Y; o[4] = Z;
    }
}

// planar logits -> planar probabilities: elementwise with per-(b, joint) statistics, four 16-byte vectors per lane in flight
__global__ __launch_bounds__(256) void sa3_probs_planar_kernel(const SA3Args a) {
    const long long plane = blockIdx.y;       // b * J + joint
    const float M = a.stats[plane * 2], S = a.stats[plane * 2 + 1];
    const float4* src = (const float4*)(a.logits + plane * a.nvox);
    float4* dst = (float4*)(a.probs + plane * a.nvox);
    const long long n4 = a.nvox / 4, i0 = (long long)blockIdx.x * 1024 + threadIdx.x;
    float4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (i0 + k * 256 < n4) v[k] = src[i0 + k * 256];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (i0 + k * 256 < n4) {
            float4 p;
            if (a.softmax) {
                p.x = __fdiv_rn(expf(a.mult * v[k].x - M), S); p.y = __fdiv_rn(expf(a.mult * v[k].y - M), S);
                p.z = __fdiv_rn(expf(a.mult * v[k].z - M), S); p.w = __fdiv_rn(expf(a.mult * v[k].w - M), S);
            } else {
                p.x = fmaxf(a.mult * v[k].x, 0.f); p.y = fmaxf(a.mult * v[k].y, 0.f);
                p.z = fmaxf(a.mult * v[k].z, 0.f); p.w = fmaxf(a.mult * v[k].w, 0.f);
            }
            dst[i0 + k * 256] = p;
        }
    }
}

// one wave per (b, joint): combine the chunk partials in fp64
__global__ void sa3_finalize_kernel(const SA3Args a, int B) {
    const int bj = blockIdx.x;
    const float* p = a.partial + (long long)bj * a.nchunks * SA_REC;
    const int lane = threadIdx.x;
    float M = -INFINITY;
    for (int c = lane; c < a.nchunks; c += 64) M = fmaxf(M, p[c * SA_REC]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) M = fmaxf(M, __shfl_xor(M, off));
    double S = 0, X = 0, Y = 0, Z = 0;
    for (int c = lane; c < a.nchunks; c += 64) {
        const float* r = p + c * SA_REC;
        const double w = (r[0] == -INFINITY) ? 0.0 : (double)expf(r[0] - M);
        S += r[1] * w; X += r[2] * w; Y += r[3] * w; Z += r[4] * w;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        S += __shfl_xor(S, off); X += __shfl_xor(X, off); Y += __shfl_xor(Y, off); Z += __shfl_xor(Z, off);
    }
    if (lane == 0) {
        a.stats[bj * 2] = M;
        a.stats[bj * 2 + 1] = (float)S;
        const double d = a.softmax ? S : 1.0;  // op.py:90-94: the ReLU variant is NOT normalised
        a.kp[bj * 3] = (float)(X / d); a.kp[bj * 3 + 1] = (float)(Y / d); a.kp[bj * 3 + 2] = (float)(Z / d);
    }
}

template <bool CL>
__global__ __launch_bounds__(256) void sa3_probs_kernel(const SA3Args a) {
    extern __shared__ float smem[];
    const int ts = a.J | 1;
    float* tile = smem;
    const int b = blockIdx.y, chunk = blockIdx.x;
    const float* lg = a.logits + (long long)b * a.J * a.nvox;
    const float* st = a.stats + (long long)b * a.J * 2;
    float* pr = a.probs + (long long)b * a.J * a.nvox;
    for (int it = 0; it < SA_ITERS; ++it) {
        const long long vox0 = (long long)chunk * SA_CHUNK + it * 256;
        if (vox0 >= a.nvox) break;
        const int nv = (int)min((long long)256, a.nvox - vox0);
        if (CL) {
            __syncthreads();
            stage_cl(a, lg, vox0, nv, tile, ts);
            __syncthreads();
        }
        const int t = threadIdx.x;
        if (t < nv) {
            const long long vox = vox0 + t;
            for (int j = 0; j < a.J; ++j) {
                const float x = a.mult * (CL ? tile[t * ts + j] : lg[(long long)j * a.nvox + vox]);
                const float p = a.softmax ? __fdiv_rn(expf(x - st[j * 2]), st[j * 2 + 1]) : fmaxf(x, 0.f);
                pr[(long long)j * a.nvox + vox] = p;
            }
        }
    }
}

// ---- per-joint statistics of the 3D heatmap (lt_softargmax3d_stats_fwd): the probabilities pass, which knows M, S and the joint, also reduces the six
// second moments of the heatmap ABOUT the returned joint (never E[xx^T] - mu mu^T: at world coordinates of 1e5 mm that difference has no digits left
// in fp32) and the lexicographic (largest x, smallest voxel index) pair.  Lanes and workgroups add in fp32 in a fixed order, the chunk records are
// combined in fp64 by one wave per (b, joint) as in sa3_finalize_kernel: no atomics, the same bits on every call.
constexpr int SS_REC = 8;                    // chunk record: cxx cxy cxz cyy cyz czz, x at the peak, the peak's voxel index (int bits)

struct SA3StatArgs {
    SA3Args a;
    float* spart;      // [B][J][snchunks][8]
    float* out;        // [B][J][8] = peak, mass, cxx, cxy, cxz, cyy, cyz, czz
    int* peak_index;   // [B][J]
    int snchunks;
};

struct SSAcc { float xx, xy, xz, yy, yz, zz, px; int pi; };
struct SSNorm { float M, S, cx, cy, cz; };

__device__ __forceinline__ void ss_init(SSAcc& s) {
    s.xx = s.xy = s.xz = s.yy = s.yz = s.zz = 0.f;
    s.px = -INFINITY; s.pi = 0x7fffffff;
}

// M, S and the centre of one (b, joint): the returned joint, divided by the mass in ReLU mode (whose joints are not normalised); no mass: no weights
__device__ __forceinline__ SSNorm ss_norm(const SA3Args& a, long long bj) {
    SSNorm n;
    n.M = a.stats[bj * 2]; n.S = a.stats[bj * 2 + 1];
    const float kx = a.kp[bj * 3], ky = a.kp[bj * 3 + 1], kz = a.kp[bj * 3 + 2];
    if (a.softmax) { n.cx = kx; n.cy = ky; n.cz = kz; }
    else if (n.S > 0.f) { n.cx = __fdiv_rn(kx, n.S); n.cy = __fdiv_rn(ky, n.S); n.cz = __fdiv_rn(kz, n.S); }
    else n.cx = n.cy = n.cz = 0.f;
    return n;
}

// the value the probabilities pass writes for x = mult * logit (the expressions of sa3_probs_kernel / sa3_probs_planar_kernel) ...
__device__ __forceinline__ float ss_prob(const SA3Args& a, const SSNorm& n, float x) {
    return a.softmax ? __fdiv_rn(expf(x - n.M), n.S) : fmaxf(x, 0.f);
}

// ... and the normalised weight of that voxel in the moments
__device__ __forceinline__ float ss_weight(const SA3Args& a, const SSNorm& n, float p) {
    return a.softmax ? p : (n.S > 0.f ? __fdiv_rn(p, n.S) : 0.f);
}

__device__ __forceinline__ void ss_peak(float& px, int& pi, float x2, int i2) {
    if (x2 > px || (x2 == px && i2 < pi)) { px = x2; pi = i2; }
}

// one voxel of a lane's run; a lane visits its voxels in increasing index order, so the strict comparison keeps the first of equal maxima
__device__ __forceinline__ void ss_add(SSAcc& s, float x, float w, float dx, float dy, float dz, int idx) {
    const float wx = w * dx, wy = w * dy, wz = w * dz;
    s.xx += wx * dx; s.xy += wx * dy; s.xz += wx * dz; s.yy += wy * dy; s.yz += wy * dz; s.zz += wz * dz;
    if (x > s.px) { s.px = x; s.pi = idx; }
}

__device__ __forceinline__ void ss_wave_reduce(SSAcc& s) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        s.xx += __shfl_xor(s.xx, off); s.xy += __shfl_xor(s.xy, off); s.xz += __shfl_xor(s.xz, off);
        s.yy += __shfl_xor(s.yy, off); s.yz += __shfl_xor(s.yz, off); s.zz += __shfl_xor(s.zz, off);
        const float x2 = __shfl_xor(s.px, off);
        const int i2 = __shfl_xor(s.pi, off);
        ss_peak(s.px, s.pi, x2, i2);
    }
}

__device__ __forceinline__ void ss_store(float* o, const SSAcc& s) {
    o[0] = s.xx; o[1] = s.xy; o[2] = s.xz; o[3] = s.yy; o[4] = s.yz; o[5] = s.zz; o[6] = s.px; o[7] = __int_as_float(s.pi);
}

// Generic planar and channels-last logits, the chunks of sa3_probs_kernel.  Here a WAVE owns joints (wave, wave + 4, ... : at most SS_JW of the 32) and its
// lanes walk the 256 voxels of an iteration 64 at a time, so the state is SS_JW accumulators however many joints there are, a joint's record needs one
// wave reduction per chunk and no LDS, and the probabilities leave as 256-byte rows.  Channels-last logits come through the staged tile of the other
// kernels (row stride odd: lanes on consecutive voxels read distinct banks).
constexpr int SS_JW = 8;

template <bool CL>
__global__ __launch_bounds__(256) void sa3_probs_stats_kernel(const SA3StatArgs sa) {
    extern __shared__ float smem[];
    const SA3Args& a = sa.a;
    const int ts = a.J | 1;
    float* tile = smem;                       // CL only: [256][ts]
    const int b = blockIdx.y, chunk = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* lg = a.logits + (long long)b * a.J * a.nvox;
    const float* cd = a.coords + (long long)b * a.nvox * 3;
    float* pr = a.probs ? a.probs + (long long)b * a.J * a.nvox : nullptr;
    SSAcc acc[SS_JW];
    SSNorm nm[SS_JW];
#pragma unroll
    for (int q = 0; q < SS_JW; ++q) {
        ss_init(acc[q]);
        nm[q] = ss_norm(a, (long long)b * a.J + min(wave + 4 * q, a.J - 1));
    }
    for (int it = 0; it < SA_ITERS; ++it) {
        const long long vox0 = (long long)chunk * SA_CHUNK + it * 256;
        if (vox0 >= a.nvox) break;
        const int nv = (int)min((long long)256, a.nvox - vox0);
        if (CL) {
            __syncthreads();
            stage_cl(a, lg, vox0, nv, tile, ts);
            __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int v = k * 64 + lane;
            if (v < nv) {
                const long long vox = vox0 + v;
                const float cx = cd[vox * 3], cy = cd[vox * 3 + 1], cz = cd[vox * 3 + 2];
#pragma unroll
                for (int q = 0; q < SS_JW; ++q) {
                    const int j = wave + 4 * q;
                    if (j < a.J) {
                        const float x = a.mult * (CL ? tile[v * ts + j] : lg[(long long)j * a.nvox + vox]);
                        const float p = ss_prob(a, nm[q], x);
                        if (pr) pr[(long long)j * a.nvox + vox] = p;
                        ss_add(acc[q], x, ss_weight(a, nm[q], p), cx - nm[q].cx, cy - nm[q].cy, cz - nm[q].cz, (int)vox);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < SS_JW; ++q) {
        const int j = wave + 4 * q;
        if (j < a.J) {
            ss_wave_reduce(acc[q]);
            if (lane == 0) ss_store(sa.spart + (((long long)b * a.J + j) * sa.snchunks + chunk) * SS_REC, acc[q]);
        }
    }
}

// Vectorised planar logits: the chunks and the lane-to-voxel map of sa3_partial_planar_kernel (a lane keeps the coordinates of its SAP_V groups of four
// voxels in registers and the workgroup walks the joints, the next joint's loads in flight), so the coordinates are read once per sample, not once per
// joint as a per-plane grid like sa3_probs_planar_kernel's would.  Per joint one wave reduction, the four waves through LDS.
__global__ __launch_bounds__(256) void sa3_probs_stats_planar_kernel(const SA3StatArgs sa) {
    __shared__ float red[32 * 4 * SS_REC];    // [J][wave][8]
    const SA3Args& a = sa.a;
    const int b = blockIdx.y, chunk = blockIdx.x;
    const float* lg = a.logits + (long long)b * a.J * a.nvox;
    const float* cd = a.coords + (long long)b * a.nvox * 3;
    float* pr = a.probs ? a.probs + (long long)b * a.J * a.nvox : nullptr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long vox[SAP_V];
    bool ok[SAP_V];
    sa_f32x4 ca[SAP_V], cb[SAP_V], cc[SAP_V];   // x0 y0 z0 x1 | y1 z1 x2 y2 | z2 x3 y3 z3
#pragma unroll
    for (int k = 0; k < SAP_V; ++k) {
        const long long v = (long long)chunk * SAP_CHUNK + k * 1024 + threadIdx.x * 4;
        ok[k] = v < a.nvox;                  // nvox % 4 == 0: a group is inside or outside as a whole
        vox[k] = ok[k] ? v : 0;              // outside: group 0 is loaded in its place and never used
        const sa_f32x4* c4 = (const sa_f32x4*)(cd + vox[k] * 3);
        ca[k] = c4[0]; cb[k] = c4[1]; cc[k] = c4[2];
    }
    sa_f32x4 cur[SAP_V], nxt[SAP_V];
#pragma unroll
    for (int k = 0; k < SAP_V; ++k) cur[k] = *(const sa_f32x4*)(lg + vox[k]);
#pragma unroll 1
    for (int j = 0; j < a.J; ++j) {
        const float* nl = lg + (long long)min(j + 1, a.J - 1) * a.nvox;
#pragma unroll
        for (int k = 0; k < SAP_V; ++k) nxt[k] = *(const sa_f32x4*)(nl + vox[k]);
        const SSNorm n = ss_norm(a, (long long)b * a.J + j);
        SSAcc s;
        ss_init(s);
#pragma unroll
        for (int k = 0; k < SAP_V; ++k) {
            if (ok[k]) {
                const float x0 = a.mult * cur[k][0], x1 = a.mult * cur[k][1], x2 = a.mult * cur[k][2], x3 = a.mult * cur[k][3];
                sa_f32x4 p;
                p[0] = ss_prob(a, n, x0); p[1] = ss_prob(a, n, x1); p[2] = ss_prob(a, n, x2); p[3] = ss_prob(a, n, x3);
                if (pr) *(sa_f32x4*)(pr + (long long)j * a.nvox + vox[k]) = p;
                const int i0 = (int)vox[k];
                ss_add(s, x0, ss_weight(a, n, p[0]), ca[k][0] - n.cx, ca[k][1] - n.cy, ca[k][2] - n.cz, i0);
                ss_add(s, x1, ss_weight(a, n, p[1]), ca[k][3] - n.cx, cb[k][0] - n.cy, cb[k][1] - n.cz, i0 + 1);
                ss_add(s, x2, ss_weight(a, n, p[2]), cb[k][2] - n.cx, cb[k][3] - n.cy, cc[k][0] - n.cz, i0 + 2);
                ss_add(s, x3, ss_weight(a, n, p[3]), cc[k][1] - n.cx, cc[k][2] - n.cy, cc[k][3] - n.cz, i0 + 3);
            }
        }
        ss_wave_reduce(s);
        if (lane == 0) ss_store(red + (j * 4 + wave) * SS_REC, s);
#pragma unroll
        for (int k = 0; k < SAP_V; ++k) cur[k] = nxt[k];
    }
    __syncthreads();
    if (threadIdx.x < a.J) {
        const int j = threadIdx.x;
        SSAcc s;
        ss_init(s);
        for (int w = 0; w < 4; ++w) {
            const float* r = red + (j * 4 + w) * SS_REC;
            s.xx += r[0]; s.xy += r[1]; s.xz += r[2]; s.yy += r[3]; s.yz += r[4]; s.zz += r[5];
            ss_peak(s.px, s.pi, r[6], __float_as_int(r[7]));
        }
        ss_store(sa.spart + (((long long)b * a.J + j) * sa.snchunks + chunk) * SS_REC, s);
    }
}

// one wave per (b, joint): the chunk records in fp64, then the record the caller reads
__global__ void sa3_stats_finalize_kernel(const SA3StatArgs sa) {
    const SA3Args& a = sa.a;
    const int bj = blockIdx.x, lane = threadIdx.x;
    const float* p = sa.spart + (long long)bj * sa.snchunks * SS_REC;
    double m[6] = {0, 0, 0, 0, 0, 0};
    float px = -INFINITY;
    int pi = 0x7fffffff;
    for (int c = lane; c < sa.snchunks; c += 64) {
        const float* r = p + c * SS_REC;
#pragma unroll
        for (int i = 0; i < 6; ++i) m[i] += (double)r[i];
        ss_peak(px, pi, r[6], __float_as_int(r[7]));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int i = 0; i < 6; ++i) m[i] += __shfl_xor(m[i], off);
        const float x2 = __shfl_xor(px, off);
        const int i2 = __shfl_xor(pi, off);
        ss_peak(px, pi, x2, i2);
    }
    if (lane == 0) {
        const float M = a.stats[bj * 2], S = a.stats[bj * 2 + 1];
        float* o = sa.out + (long long)bj * 8;
        // softmax: the expression of the probabilities pass at the peak voxel (x == M there, so 1 / S); ReLU: relu(x) / mass, nothing over no mass
        o[0] = a.softmax ? __fdiv_rn(expf(px - M), S) : (S > 0.f ? __fdiv_rn(fmaxf(px, 0.f), S) : 0.f);
        o[1] = a.softmax ? 1.f : S;
#pragma unroll
        for (int i = 0; i < 6; ++i) o[2 + i] = (float)m[i];
        sa.peak_index[bj] = pi;
    }
}

// planar logits whose volumes are float4-addressable take the vectorised kernels
bool sa3_planar_vec(const SA3Args& a) {
    static const bool off = env_on("LT_SA3_NO_VEC");
    return !off && a.nvox % 4 == 0 && ((uintptr_t)a.logits & 15) == 0 && ((uintptr_t)a.coords & 15) == 0 &&
           (!a.probs || ((uintptr_t)a.probs & 15) == 0);
}

template <bool CL>
int sa3_launch_partial(const SA3Args& a, int B, hipStream_t st) {
    const int J = a.J;
    // 17 joints (COCO / Human3.6M skeletons) get an exact instantiation: 35 fewer state registers than the 24-wide one
    const int JP = J == 17 ? 17 : (J <= 8 ? 8 : (J <= 16 ? 16 : (J <= 24 ? 24 : 32)));
    const size_t lds = ((CL ? 256 * (J | 1) : 0) + 4 * JP * SA_REC) * sizeof(float);
    const dim3 grid(a.nchunks, B), blk(256);
    switch (JP) {
        case 8: hipLaunchKernelGGL((sa3_partial_kernel<8, CL>), grid, blk, lds, st, a); break;
        case 16: hipLaunchKernelGGL((sa3_partial_kernel<16, CL>), grid, blk, lds, st, a); break;
        case 17: hipLaunchKernelGGL((sa3_partial_kernel<17, CL>), grid, blk, lds, st, a); break;
        case 24: hipLaunchKernelGGL((sa3_partial_kernel<24, CL>), grid, blk, lds, st, a); break;
        default: hipLaunchKernelGGL((sa3_partial_kernel<32, CL>), grid, blk, lds, st, a); break;
    }
    LT_CHECK_LAUNCH("lt_softargmax3d_fwd(partial)");
    return LT_OK;
}

// ---- 2D soft-argmax: one workgroup per heatmap ------------------------------------------------
__device__ __forceinline__ float block_reduce(float v, float* red, bool is_max) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float o = __shfl_xor(v, off);
        v = is_max ? fmaxf(v, o) : v + o;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
    for (int w = 1; w < 4; ++w) r = is_max ? fmaxf(r, red[w]) : r + red[w];
    return r;
}

// STATS (sa2_stats_kernel, lt_softargmax2d_stats_fwd): the third pass, which holds M, S and the returned coordinates, also reduces the heatmap's second
// moments ABOUT those coordinates and the (largest x, smallest index) pair together with the value it writes there, so that peak is probs[peak_index] by construction.  Lanes
// add in fp32 in index order, the wave butterfly and the four waves are combined in a fixed order (the waves in fp64): no atomics, equal bits every call.
// The first two passes and the plain third pass are the same text for both instantiations: coords and probs keep their bits.
template <bool STATS>
__device__ __forceinline__ void sa2_body(const float* __restrict__ hm, float mult, int softmax, float* __restrict__ coords, float* __restrict__ probs,
                                         float* __restrict__ stats, int* __restrict__ peak_index, int h, int w) {
    __shared__ float red[4];
    const long long base = (long long)blockIdx.x * h * w;
    const int n = h * w;
    float M = 0.f;
    if (softmax) {
        float m = -INFINITY;
        for (int i = threadIdx.x; i < n; i += 256) m = fmaxf(m, mult * hm[base + i]);
        M = block_reduce(m, red, true);
    }
    float s = 0.f, sx = 0.f, sy = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float x = mult * hm[base + i];
        const float e = softmax ? expf(x - M) : fmaxf(x, 0.f);
        const int yy = i / w, xx = i - yy * w;
        s += e; sx += e * (float)xx; sy += e * (float)yy;
    }
    const float S = block_reduce(s, red, false);
    const float X = block_reduce(sx, red, false);
    const float Y = block_reduce(sy, red, false);
    if (threadIdx.x == 0) {
        // softmax: sum p*x with p = e/S; relu: (sum e*x) / (sum e)  (op.py:39-44) -- the same quotient
        coords[blockIdx.x * 2] = X / S;
        coords[blockIdx.x * 2 + 1] = Y / S;
    }
    if (!STATS) {
        if (probs)
            for (int i = threadIdx.x; i < n; i += 256) {
                const float x = mult * hm[base + i];
                probs[base + i] = softmax ? __fdiv_rn(expf(x - M), S) : fmaxf(x, 0.f);
            }
        return;
    }
    __shared__ float sred[4][5];     // per wave: cxx, cxy, cyy, x at the peak, the value written at the peak
    __shared__ int sidx[4];
    const bool some = softmax || S > 0.f;          // ReLU without mass: no weights, the centre is never used (the coordinates are NaN as in the plain kernel)
    const float cx = some ? X / S : 0.f, cy = some ? Y / S : 0.f;
    float cxx = 0.f, cxy = 0.f, cyy = 0.f, px = -INFINITY, pp = 0.f;
    int pi = 0x7fffffff;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float x = mult * hm[base + i];
        const float p = softmax ? __fdiv_rn(expf(x - M), S) : fmaxf(x, 0.f);
        if (probs) probs[base + i] = p;
        const float wgt = softmax ? p : (some ? __fdiv_rn(p, S) : 0.f);
        const int yy = i / w, xx = i - yy * w;
        const float dx = (float)xx - cx, dy = (float)yy - cy;
        const float wx = wgt * dx, wy = wgt * dy;
        cxx += wx * dx; cxy += wx * dy; cyy += wy * dy;
        if (x > px) { px = x; pi = i; pp = p; }          // increasing i: the strict comparison keeps the first of equal maxima
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        cxx += __shfl_xor(cxx, off); cxy += __shfl_xor(cxy, off); cyy += __shfl_xor(cyy, off);
        const float x2 = __shfl_xor(px, off), p2 = __shfl_xor(pp, off);
        const int i2 = __shfl_xor(pi, off);
        if (x2 > px || (x2 == px && i2 < pi)) { px = x2; pi = i2; pp = p2; }
    }
    if ((threadIdx.x & 63) == 0) {
        float* r = sred[threadIdx.x >> 6];
        r[0] = cxx; r[1] = cxy; r[2] = cyy; r[3] = px; r[4] = pp;
        sidx[threadIdx.x >> 6] = pi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double m[3] = {0, 0, 0};
        for (int wv = 0; wv < 4; ++wv) {
            m[0] += (double)sred[wv][0]; m[1] += (double)sred[wv][1]; m[2] += (double)sred[wv][2];
            if (wv && (sred[wv][3] > px || (sred[wv][3] == px && sidx[wv] < pi))) { px = sred[wv][3]; pi = sidx[wv]; pp = sred[wv][4]; }
        }
        float* o = stats + (long long)blockIdx.x * 5;
        o[0] = softmax ? pp : (some ? __fdiv_rn(pp, S) : 0.f);          // softmax: the value written at the peak; ReLU: relu(x_peak) / mass
        o[1] = softmax ? 1.f : S;
        o[2] = (float)m[0]; o[3] = (float)m[1]; o[4] = (float)m[2];
        peak_index[blockIdx.x] = pi;
    }
}

// the plain kernel keeps its arguments; the statistics are a kernel of their own over the same body
__global__ __launch_bounds__(256) void sa2_kernel(const float* __restrict__ hm, float mult, int softmax, float* __restrict__ coords,
                                                   float* __restrict__ probs, int h, int w) {
    sa2_body<false>(hm, mult, softmax, coords, probs, nullptr, nullptr, h, w);
}

__global__ __launch_bounds__(256) void sa2_stats_kernel(const float* __restrict__ hm, float mult, int softmax, float* __restrict__ coords,
                                                         float* __restrict__ probs, float* __restrict__ stats, int* __restrict__ peak_index, int h, int w) {
    sa2_body<true>(hm, mult, softmax, coords, probs, stats, peak_index, h, w);
}

// ---- DLT: one lane per (sample, joint), the routine of dlt.h ------------------------------------------------------------------------------------
// the DLT point of one (sample, joint) from its R, rounded to fp32
__device__ __forceinline__ void dlt_solve(double (&R)[4][4], float* __restrict__ o) {
    double X[3];
    dlt_point(R, X);
    o[0] = (float)X[0]; o[1] = (float)X[1]; o[2] = (float)X[2];
}

__global__ void dlt_kernel(const float* __restrict__ proj, const float* __restrict__ pts, const float* __restrict__ conf,
                           float* __restrict__ out, int B, int NV, int J) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= B * J) return;
    const int b = g / J, j = g - b * J;
    double R[4][4] = {};  // R of A = QR, grown one view at a time
    for (int v = 0; v < NV; ++v) {
        const float* p = pts + (((long long)b * NV + v) * J + j) * 2;
        const float c = conf ? conf[((long long)b * NV + v) * J + j] : 1.f;
        dlt_add_view(R, proj + ((long long)b * NV + v) * 12, (double)p[0], (double)p[1], (double)c);
    }
    dlt_solve(R, out + (long long)g * 3);
}

// ---- what the DLT's backward and the forward-mode statistics share --------------------------------------------------------------------------------
// triangulate_point_from_multiple_views_linear_torch (multiview.py:141-168): X = v[:3] / v[3], v = right singular vector of A for its smallest
// singular value = eigenvector of M = A^T A for its smallest eigenvalue lambda; rows of A: c_v (x_{v,r} P_v[2,:] - P_v[r,:]).  What autograd derives
// through torch.svd there, written out:  g_v = (g_X / v3, -(g_X . v[:3]) / v3^2) (orthogonal to v: X does not depend on |v|),
//   w = (lambda I - M)^+ g_v = sum_{i != min} e_i (e_i . g_v) / (lambda - lambda_i),   dL/dM = (w v^T + v w^T) / 2,   dL/dA = A (w v^T + v w^T),
//   dL/dc_v = sum_r dL/dA[v,r,:] . (x P2 - Pr),   dL/dx_{v,r} = c_v dL/dA[v,r,:] . P_v[2,:].   fp64.
// dlt_grad_w: v and w for one g_X off the forward's SVD (V: eigenvectors of A^T A in its columns, ev: the eigenvalues, best: the smallest one's column)
__device__ __forceinline__ void dlt_grad_w(const double (&V)[4][4], const double (&ev)[4], const int best, const double (&gX)[3], double (&vv)[4],
                                           double (&wv)[4]) {
    const double lam = ev[best];
    double gv[4];
    for (int k = 0; k < 4; ++k) { vv[k] = V[k][best]; wv[k] = 0; }
    gv[0] = gX[0] / vv[3]; gv[1] = gX[1] / vv[3]; gv[2] = gX[2] / vv[3];
    gv[3] = -(gX[0] * vv[0] + gX[1] * vv[1] + gX[2] * vv[2]) / (vv[3] * vv[3]);
    for (int i = 0; i < 4; ++i) {
        if (i == best) continue;
        double dot = 0;
        for (int k = 0; k < 4; ++k) dot += V[k][i] * gv[k];
        const double f = dot / (lam - ev[i]);
        for (int k = 0; k < 4; ++k) wv[k] += V[k][i] * f;
    }
}

// dlt_grad_row: row r of one view (point coordinate pr, confidence c, matrix P): returns dL/dA[v,r,:] . P[2,:] -- dL/dx_{v,r} is c times that -- and
// adds the row's share of dL/dc_v to gc
__device__ __forceinline__ double dlt_grad_row(const float* __restrict__ P, const double pr, const int r, const double c, const double (&vv)[4],
                                               const double (&wv)[4], double& gc) {
    double raw[4], arow[4], av = 0, aw = 0;
    for (int k = 0; k < 4; ++k) { raw[k] = (double)P[8 + k] * pr - (double)P[4 * r + k]; arow[k] = raw[k] * c; av += arow[k] * vv[k]; aw += arow[k] * wv[k]; }
    double gp = 0;
    for (int k = 0; k < 4; ++k) {
        const double ga = aw * vv[k] + av * wv[k];          // dL/dA[v,r,k] = (A (w v^T + v w^T))[row][k]
        gc += ga * raw[k];
        gp += ga * (double)P[8 + k];
    }
    return gp;
}

// ---- statistics of a triangulated joint (lt_alg_tail_stats_fwd, lt_triangulate_dlt_stats): after the forward's dlt_svd of R ------------------------
// The joint as dlt_point gives it (same divisions, so the same bits), then per valid view the reprojection error of the RETURNED fp32 joint and the
// first-order covariance sum_v J_v Sigma_v J_v^T, J_v = dX / d(2D point of view v) (3 x 2, confidences fixed): dlt_grad_w for g_X = e_0, e_1, e_2 off the
// one SVD, dlt_grad_row per view and coordinate.  view(v, x, y, c, s) -> bool: is view v valid, and if so its fp32 2D point, its confidence and its 2D
// covariance {xx, xy, yy} (image px^2), all as fp64.  Masked views get a quiet NaN as their reprojection error and are never read.
// reproj: element v * J of it belongs to view v.  solvable == false (fewer than two valid views): NaN everywhere.
template <class View>
__device__ __forceinline__ void dlt_stats_finish(double (&R)[4][4], const bool solvable, const float* __restrict__ proj_b, const int NV, const int J, View view,
                                                 float* __restrict__ o, float* __restrict__ reproj, float* __restrict__ cov3d) {
    const float qnan = __int_as_float(0x7fc00000);
    if (!solvable) {
        o[0] = o[1] = o[2] = qnan;
        for (int k = 0; k < 6; ++k) cov3d[k] = qnan;
        for (int v = 0; v < NV; ++v) reproj[(long long)v * J] = qnan;
        return;
    }
    double V[4][4], ev[4];
    const int best = dlt_svd(R, V, ev);
    const double wh = V[3][best];
    double X[3];
    X[0] = V[0][best] / wh; X[1] = V[1][best] / wh; X[2] = V[2][best] / wh;          // dlt_point
    o[0] = (float)X[0]; o[1] = (float)X[1]; o[2] = (float)X[2];
    const double X32[3] = {(double)o[0], (double)o[1], (double)o[2]};                  // the reprojection error is that of the joint the caller gets
    double vv[4], wj[3][4];
    for (int e = 0; e < 3; ++e) {
        const double gX[3] = {e == 0 ? 1.0 : 0.0, e == 1 ? 1.0 : 0.0, e == 2 ? 1.0 : 0.0};
        dlt_grad_w(V, ev, best, gX, vv, wj[e]);
    }
    double C[6] = {0, 0, 0, 0, 0, 0};          // xx, xy, xz, yy, yz, zz
    for (int v = 0; v < NV; ++v) {
        double x, y, c, s[3];
        if (!view(v, x, y, c, s)) { reproj[(long long)v * J] = qnan; continue; }
        const float* P = proj_b + (long long)v * 12;
        double hh[3];
        for (int r = 0; r < 3; ++r) hh[r] = (double)P[4 * r] * X32[0] + (double)P[4 * r + 1] * X32[1] + (double)P[4 * r + 2] * X32[2] + (double)P[4 * r + 3];
        const double du = hh[0] / hh[2] - x, dv = hh[1] / hh[2] - y;
        reproj[(long long)v * J] = (float)sqrt(du * du + dv * dv);
        double Jm[3][2], unused = 0;
        for (int e = 0; e < 3; ++e) {
            Jm[e][0] = dlt_grad_row(P, x, 0, c, vv, wj[e], unused) * c;
            Jm[e][1] = dlt_grad_row(P, y, 1, c, vv, wj[e], unused) * c;
        }
        int q = 0;
        for (int e = 0; e < 3; ++e) {
            const double t0 = Jm[e][0] * s[0] + Jm[e][1] * s[1], t1 = Jm[e][0] * s[1] + Jm[e][1] * s[2];
            for (int f = e; f < 3; ++f) C[q++] += t0 * Jm[f][0] + t1 * Jm[f][1];
        }
    }
    for (int k = 0; k < 6; ++k) cov3d[k] = (float)C[k];
}

// what alg_tail_stats_kernel adds to the tail's arguments
struct AlgTailStats {
    const float* stats2d;   // B*NV*J,5 of lt_softargmax2d_stats_fwd
    float* cov2d;           // B,NV,J,3
    float* reproj;          // B,NV,J
    float* cov3d;           // B,J,6
};

// ---- algebraic tail (AlgebraicTriangulationNet, triangulation.py:166-193 after the 2D soft-argmax): one lane per (sample, joint) ------------
// conf = raw / (sum over views) + 1e-5 (uniform raw = 1 without the confidence head), kp2d = soft-argmax * (W / w, H / h), then the DLT of
// dlt_kernel on (kp2d, conf).  Every step is one IEEE rounding in the order of the Python host's torch ops (conf / conf.sum(1) + 1e-5,
// kp2d * scale, lt_triangulate_dlt), with the explicit _rn intrinsics so that no contraction can merge two of them.  The sum over views
// is torch's GPU reduction order: four interleaved partial sums (view v into sum v % 4), combined ((s0 + s1) + s2) + s3 -- plain view
// order for up to four views.
// MASKED: the same over the valid views of each sample (mask: (B, NV), non-zero = valid; never read otherwise), i.e. the unmasked tail on
// the compacted views, step for step -- the k-th VALID view goes into partial k % 4, the rows of the valid views enter R in view order.  A
// masked view gets confidence 0 and its 2D keypoint is passed through to kp2d only (never into the system, so NaN there stays there);
// fewer than two valid views: NaN joints.
// STATS (alg_tail_stats_kernel, lt_alg_tail_stats_fwd): the same loops, which also write every view's 2D covariance in image pixels (S Sigma_hm S in
// fp64, rounded once), then dlt_stats_finish in dlt_solve's place.  Sigma_v in the propagation is that ROUNDED value read back, like the joint in the
// reprojection error: both statistics can be reproduced from the outputs alone.
// RAGGED (alg_tail_ragged_kernel, lt_alg_tail_ragged_fwd): the unmasked tail over the rows view_base[b] .. view_base[b + 1] of sample b -- kp_hm, conf_raw,
// proj, kp2d and conf_out are (T, ...) over all views, sample-major; NV is NVcap.  The count is clamped into [0, min(NVcap, T)] and the first row into
// [0, T - count] (the hosts refuse such tables before launching; the second line of defence); fewer than two views: NaN joints.
template <bool MASKED, bool STATS, bool RAGGED = false>
__device__ __forceinline__ void alg_tail_body(const float* __restrict__ kp_hm, const float* __restrict__ conf_raw, int ld_conf, const float* __restrict__ proj,
                                              float sx, float sy, const uint8_t* __restrict__ mask, float* __restrict__ kp2d, float* __restrict__ conf_out,
                                              float* __restrict__ kp3d, int B, int NV, int J, const AlgTailStats& so, const int32_t* __restrict__ view_base = nullptr,
                                              int T = 0) {
    static_assert(!RAGGED || (!MASKED && !STATS), "the ragged tail is the plain tail over a sample's rows");
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= B * J) return;
    const int b = g / J, j = g - b * J;
    const uint8_t* mk = MASKED ? mask + (long long)b * NV : nullptr;
    long long r0 = (long long)b * NV;   // the row of the sample's first view
    if constexpr (RAGGED) {
        const int lo = view_base[b], nb = min(max(view_base[b + 1] - lo, 0), min(NV, T));
        r0 = min(max(lo, 0), T - nb);
        NV = nb;
    }
    float part[4] = {0.f, 0.f, 0.f, 0.f};
    int nvalid = 0;
    for (int v = 0; v < NV; ++v) {
        if (MASKED && !mk[v]) continue;
        const float c = conf_raw ? conf_raw[(r0 + v) * ld_conf + j] : 1.f;
        part[nvalid & 3] = __fadd_rn(part[nvalid & 3], c);
        ++nvalid;
    }
    const float sum = __fadd_rn(__fadd_rn(__fadd_rn(part[0], part[1]), part[2]), part[3]);
    double R[4][4] = {};  // R of A = QR, grown one (valid) view at a time
    for (int v = 0; v < NV; ++v) {
        const long long i = (r0 + v) * J + j;
        const float x = __fmul_rn(kp_hm[i * 2], sx), y = __fmul_rn(kp_hm[i * 2 + 1], sy);
        if (kp2d) { kp2d[i * 2] = x; kp2d[i * 2 + 1] = y; }
        if (STATS) {
            const float* s2 = so.stats2d + i * 5;
            so.cov2d[i * 3] = (float)((double)sx * (double)sx * (double)s2[2]);
            so.cov2d[i * 3 + 1] = (float)((double)sx * (double)sy * (double)s2[3]);
            so.cov2d[i * 3 + 2] = (float)((double)sy * (double)sy * (double)s2[4]);
        }
        if (MASKED && !mk[v]) {
            if (conf_out) conf_out[i] = 0.f;
            continue;
        }
        const float c = __fadd_rn(__fdiv_rn(conf_raw ? conf_raw[(r0 + v) * ld_conf + j] : 1.f, sum), 1e-5f);
        if (conf_out) conf_out[i] = c;
        dlt_add_view(R, proj + (r0 + v) * 12, (double)x, (double)y, (double)c);
    }
    float* o = kp3d + (long long)g * 3;
    if (STATS) {
        const long long i0 = r0 * J + j;
        // a view's values again, by the expressions of the loop above (each one IEEE rounding, so the same bits)
        auto view = [&](const int v, double& x, double& y, double& c, double (&s)[3]) -> bool {
            if (MASKED && !mk[v]) return false;
            const long long i = i0 + (long long)v * J;
            x = (double)__fmul_rn(kp_hm[i * 2], sx); y = (double)__fmul_rn(kp_hm[i * 2 + 1], sy);
            c = (double)__fadd_rn(__fdiv_rn(conf_raw ? conf_raw[(r0 + v) * ld_conf + j] : 1.f, sum), 1e-5f);
            const float* s2 = so.stats2d + i * 5;
            s[0] = (double)(float)((double)sx * (double)sx * (double)s2[2]);
            s[1] = (double)(float)((double)sx * (double)sy * (double)s2[3]);
            s[2] = (double)(float)((double)sy * (double)sy * (double)s2[4]);
            return true;
        };
        dlt_stats_finish(R, !(MASKED && nvalid < 2), proj + r0 * 12, NV, J, view, o, so.reproj + i0, so.cov3d + (long long)g * 6);
        return;
    }
    if ((MASKED || RAGGED) && nvalid < 2) { o[0] = o[1] = o[2] = __int_as_float(0x7fc00000); return; }
    dlt_solve(R, o);
}

// the plain tails keep their arguments; the statistics are kernels of their own over the same body
template <bool MASKED>
__global__ void alg_tail_kernel(const float* __restrict__ kp_hm, const float* __restrict__ conf_raw, int ld_conf, const float* __restrict__ proj,
                                float sx, float sy, const uint8_t* __restrict__ mask, float* __restrict__ kp2d, float* __restrict__ conf_out,
                                float* __restrict__ kp3d, int B, int NV, int J) {
    alg_tail_body<MASKED, false>(kp_hm, conf_raw, ld_conf, proj, sx, sy, mask, kp2d, conf_out, kp3d, B, NV, J, AlgTailStats());
}

__global__ void alg_tail_ragged_kernel(const float* __restrict__ kp_hm, const float* __restrict__ conf_raw, int ld_conf, const float* __restrict__ proj,
                                       float sx, float sy, const int32_t* __restrict__ view_base, float* __restrict__ kp2d, float* __restrict__ conf_out,
                                       float* __restrict__ kp3d, int B, int T, int NVcap, int J) {
    alg_tail_body<false, false, true>(kp_hm, conf_raw, ld_conf, proj, sx, sy, nullptr, kp2d, conf_out, kp3d, B, NVcap, J, AlgTailStats(), view_base, T);
}

template <bool MASKED>
__global__ void alg_tail_stats_kernel(const float* __restrict__ kp_hm, const float* __restrict__ conf_raw, int ld_conf, const float* __restrict__ proj,
                                      float sx, float sy, const uint8_t* __restrict__ mask, float* __restrict__ kp2d, float* __restrict__ conf_out,
                                      float* __restrict__ kp3d, int B, int NV, int J, const AlgTailStats so) {
    alg_tail_body<MASKED, true>(kp_hm, conf_raw, ld_conf, proj, sx, sy, mask, kp2d, conf_out, kp3d, B, NV, J, so);
}

// lt_triangulate_dlt_stats: dlt_kernel over the valid views (mask NULL: all of them) with the statistics; cov2d B,NV,J,3 {xx, xy, yy}
__global__ void dlt_stats_kernel(const float* __restrict__ proj, const float* __restrict__ pts, const float* __restrict__ conf, const float* __restrict__ cov2d,
                                 const uint8_t* __restrict__ mask, float* __restrict__ out, float* __restrict__ reproj, float* __restrict__ cov3d, int B, int NV,
                                 int J) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= B * J) return;
    const int b = g / J, j = g - b * J;
    const uint8_t* mk = mask ? mask + (long long)b * NV : nullptr;
    const long long i0 = (long long)b * NV * J + j;
    auto view = [&](const int v, double& x, double& y, double& c, double (&s)[3]) -> bool {
        if (mk && !mk[v]) return false;
        const long long i = i0 + (long long)v * J;
        x = (double)pts[i * 2]; y = (double)pts[i * 2 + 1];
        c = conf ? (double)conf[i] : 1.0;
        s[0] = (double)cov2d[i * 3]; s[1] = (double)cov2d[i * 3 + 1]; s[2] = (double)cov2d[i * 3 + 2];
        return true;
    };
    double R[4][4] = {};  // R of A = QR, grown one valid view at a time
    int nvalid = 0;
    for (int v = 0; v < NV; ++v) {
        double x, y, c, s[3];
        if (!view(v, x, y, c, s)) continue;
        dlt_add_view(R, proj + ((long long)b * NV + v) * 12, x, y, c);
        ++nvalid;
    }
    dlt_stats_finish(R, nvalid >= 2, proj + (long long)b * NV * 12, NV, J, view, out + (long long)g * 3, reproj + i0, cov3d + (long long)g * 6);
}

// ---- backward of the 2D soft-argmax and of the DLT (training of the algebraic model, train.py:189-236) ---------------------------------------
// integrate_tensor_2d (op.py:11-47), softmax mode: p = softmax_i(mult * h_i), (X, Y) = sum_i p_i (x_i, y_i):
//   d L / d h_i = mult * p_i * ((x_i - X) g_x + (y_i - Y) g_y).  One elementwise pass over the returned heatmaps p.
// ReLU mode (heatmap_softmax: false): e_i = relu(mult h_i) (the returned heatmaps), (X, Y) = sum_i e_i (x_i, y_i) / S, S = sum_i e_i:
//   d L / d h_i = mult [e_i > 0] ((x_i - X) g_x + (y_i - Y) g_y) / S   (every workgroup re-adds S: h x w is a few thousand values).
__global__ __launch_bounds__(256) void sa2_bwd_kernel(const float* __restrict__ probs, const float* __restrict__ coords, const float* __restrict__ gcoords,
                                                       float mult, int softmax, float* __restrict__ ghm, int h, int w) {
    __shared__ float red[4];
    const long long base = (long long)blockIdx.y * h * w;
    const float X = coords[blockIdx.y * 2], Y = coords[blockIdx.y * 2 + 1];
    const float gx = gcoords[blockIdx.y * 2], gy = gcoords[blockIdx.y * 2 + 1];
    const int n = h * w;
    float invS = 1.f;
    if (!softmax) {
        float s = 0.f;
        for (int i = threadIdx.x; i < n; i += 256) s += probs[base + i];
        invS = 1.f / block_reduce(s, red, false);
    }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int yy = i / w, xx = i - yy * w;
        const float pi = probs[base + i];
        const float wgt = softmax ? pi : (pi > 0.f ? invS : 0.f);
        ghm[base + i] = mult * wgt * (((float)xx - X) * gx + ((float)yy - Y) * gy);
    }
}

// The same backward with a gradient on BOTH outputs of integrate_tensor_2d (lt_softargmax2d_bwd_full): gp is the gradient on the returned heatmaps.
//   softmax: the returned heatmaps are p:  d L / d h_i = [coordinate term] + mult p_i (gp_i - sum_k p_k gp_k)
//   ReLU:    the returned heatmaps are e = relu(mult h), un-normalised (op.py:27):  d L / d h_i = [coordinate term] + mult [e_i > 0] gp_i
// Same grid as sa2_bwd_kernel; every workgroup re-adds sum_k p_k gp_k, as it re-adds S in ReLU mode.  The coordinate term is sa2_bwd_kernel's expression
// character for character (the build keeps a * b + c unfused), so gp == NULL gives that kernel's bits; gcoords == NULL is a zero coordinate gradient.
__global__ __launch_bounds__(256) void sa2_bwd_full_kernel(const float* __restrict__ probs, const float* __restrict__ coords, const float* __restrict__ gcoords,
                                                            const float* __restrict__ gprobs, float mult, int softmax, float* __restrict__ ghm, int h, int w) {
    __shared__ float red[4];
    const long long base = (long long)blockIdx.y * h * w;
    const float X = coords[blockIdx.y * 2], Y = coords[blockIdx.y * 2 + 1];
    const float gx = gcoords ? gcoords[blockIdx.y * 2] : 0.f, gy = gcoords ? gcoords[blockIdx.y * 2 + 1] : 0.f;
    const int n = h * w;
    float invS = 1.f;
    if (!softmax) {
        float s = 0.f;
        for (int i = threadIdx.x; i < n; i += 256) s += probs[base + i];
        invS = 1.f / block_reduce(s, red, false);
    }
    float D = 0.f;
    if (gprobs && softmax) {
        float d = 0.f;
        for (int i = threadIdx.x; i < n; i += 256) d += probs[base + i] * gprobs[base + i];
        D = block_reduce(d, red, false);
    }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int yy = i / w, xx = i - yy * w;
        const float pi = probs[base + i];
        const float wgt = softmax ? pi : (pi > 0.f ? invS : 0.f);
        float g = mult * wgt * (((float)xx - X) * gx + ((float)yy - Y) * gy);
        if (gprobs) {
            const float gp = gprobs[base + i];
            g += softmax ? mult * pi * (gp - D) : (pi > 0.f ? mult * gp : 0.f);
        }
        ghm[base + i] = g;
    }
}

// the DLT's backward by the formulas above dlt_grad_w / dlt_grad_row: fp64, one lane per (sample, joint)
__global__ void dlt_bwd_kernel(const float* __restrict__ proj, const float* __restrict__ pts, const float* __restrict__ conf,
                               const float* __restrict__ gout, float* __restrict__ gpts, float* __restrict__ gconf, int B, int NV, int J) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= B * J) return;
    const int b = g / J, j = g - b * J;
    double R[4][4] = {};  // R of A = QR, grown one view at a time
    for (int v = 0; v < NV; ++v) {
        const float* p = pts + (((long long)b * NV + v) * J + j) * 2;
        const float c = conf ? conf[((long long)b * NV + v) * J + j] : 1.f;
        dlt_add_view(R, proj + ((long long)b * NV + v) * 12, (double)p[0], (double)p[1], (double)c);
    }
    double V[4][4], ev[4];
    const int best = dlt_svd(R, V, ev);         // the forward's solve: eigenvectors of A^T A = right singular vectors, eigenvalues = sigma^2
    double vv[4], wv[4];
    const double gX[3] = {(double)gout[g * 3], (double)gout[g * 3 + 1], (double)gout[g * 3 + 2]};
    dlt_grad_w(V, ev, best, gX, vv, wv);
    for (int v = 0; v < NV; ++v) {
        const float* P = proj + ((long long)b * NV + v) * 12;
        const long long pi = ((long long)b * NV + v) * J + j;
        const float* p = pts + pi * 2;
        const double c = conf ? (double)conf[pi] : 1.0;
        double gc = 0;
        for (int r = 0; r < 2; ++r) gpts[pi * 2 + r] = (float)(dlt_grad_row(P, (double)p[r], r, c, vv, wv, gc) * c);
        if (gconf) gconf[pi] = (float)gc;
    }
}

}  // namespace

extern "C" int lt_softargmax2d_bwd(const float* probs, const float* coords, const float* grad_coords, float mult, int32_t softmax, float* grad_heatmaps,
                                   int32_t NJ, int32_t h, int32_t w, void* stream) {
    LT_REQUIRE(probs && coords && grad_coords && grad_heatmaps && NJ >= 1 && h >= 1 && w >= 1, LT_ERR_INVALID, "lt_softargmax2d_bwd: bad argument");
    const int bx = (int)((h * w + 255) / 256);
    hipLaunchKernelGGL(sa2_bwd_kernel, dim3(bx < 64 ? bx : 64, NJ), dim3(256), 0, (hipStream_t)stream, probs, coords, grad_coords, mult, softmax, grad_heatmaps, h, w);
    LT_CHECK_LAUNCH("lt_softargmax2d_bwd");
    return LT_OK;
}

extern "C" int lt_softargmax2d_bwd_full(const float* probs, const float* coords, const float* grad_coords, const float* grad_probs, float mult, int32_t softmax,
                                        float* grad_heatmaps, int32_t NJ, int32_t h, int32_t w, void* stream) {
    LT_REQUIRE(probs && coords && grad_heatmaps, LT_ERR_INVALID, "lt_softargmax2d_bwd_full: null probs, coords or grad_heatmaps");
    LT_REQUIRE(grad_coords || grad_probs, LT_ERR_INVALID, "lt_softargmax2d_bwd_full: grad_coords and grad_probs are both null (nothing to backpropagate)");
    LT_REQUIRE(NJ >= 1 && h >= 1 && w >= 1, LT_ERR_INVALID, "lt_softargmax2d_bwd_full: bad shape (NJ %d, h %d, w %d)", NJ, h, w);
    LT_REQUIRE((int64_t)h * w < 0x80000000LL, LT_ERR_INVALID, "lt_softargmax2d_bwd_full: h * w = %lld does not fit the int32 index of a heatmap", (long long)h * w);
    const int bx = (int)(((int64_t)h * w + 255) / 256);
    hipLaunchKernelGGL(sa2_bwd_full_kernel, dim3(bx < 64 ? bx : 64, NJ), dim3(256), 0, (hipStream_t)stream, probs, coords, grad_coords, grad_probs, mult, softmax,
                       grad_heatmaps, h, w);
    LT_CHECK_LAUNCH("lt_softargmax2d_bwd_full");
    return LT_OK;
}

extern "C" int lt_triangulate_dlt_bwd(const float* proj, const float* points, const float* conf, const float* grad_out, float* grad_points, float* grad_conf,
                                      int32_t B, int32_t NV, int32_t J, void* stream) {
    LT_REQUIRE(proj && points && grad_out && grad_points && B >= 1 && NV >= 2 && J >= 1, LT_ERR_INVALID, "lt_triangulate_dlt_bwd: bad argument");
    hipLaunchKernelGGL(dlt_bwd_kernel, dim3((B * J + 63) / 64), dim3(64), 0, (hipStream_t)stream, proj, points, conf, grad_out, grad_points, grad_conf, B, NV, J);
    LT_CHECK_LAUNCH("lt_triangulate_dlt_bwd");
    return LT_OK;
}

extern "C" size_t lt_softargmax3d_workspace(int32_t B, int32_t J, int64_t nvox) {
    const int64_t nchunks = (nvox + SA_CHUNK - 1) / SA_CHUNK;
    return (size_t)((int64_t)B * J * nchunks * SA_REC + (int64_t)B * J * 2) * sizeof(float);
}

// the one body of lt_softargmax3d_fwd and lt_softargmax3d_stats_fwd: partial and finalize kernels, then the probabilities pass -- the plain one, or
// (stats != NULL) the one that also reduces the statistics, followed by their finalize
static int sa3_forward(const char* who, const float* logits, const float* coords, float mult, int32_t softmax, int32_t channels_last, int32_t ld, float* kp,
                       float* probs, float* stats, int32_t* peak_index, bool with_stats, int32_t B, int32_t J, int64_t nvox, void* workspace, void* stream) {
    LT_REQUIRE(logits && coords && kp && workspace, LT_ERR_INVALID, "%s: null argument", who);
    LT_REQUIRE(!with_stats || (stats && peak_index), LT_ERR_INVALID, "%s: null stats or peak_index", who);
    LT_REQUIRE(B >= 1 && J >= 1 && nvox >= 1, LT_ERR_INVALID, "%s: bad shape", who);
    LT_REQUIRE(!with_stats || nvox <= 0x7fffffff, LT_ERR_UNSUPPORTED, "%s: nvox %lld does not fit the int32 peak index", who, (long long)nvox);
    LT_REQUIRE(J <= 32, LT_ERR_UNSUPPORTED, "%s: J=%d > 32 (split the joints into groups of <= 32)", who, J);
    LT_REQUIRE(!channels_last || ld >= J, LT_ERR_INVALID, "%s: ld < J", who);
    LT_REQUIRE(!channels_last || ld == J, LT_ERR_UNSUPPORTED, "%s: channels-last logits must be dense (ld == J)", who);
    SA3Args a;
    a.logits = logits; a.coords = coords; a.kp = kp; a.probs = probs; a.mult = mult; a.softmax = softmax; a.J = J; a.ld = ld; a.nvox = nvox;
    a.nchunks = (int)((nvox + SA_CHUNK - 1) / SA_CHUNK);
    a.partial = (float*)workspace;
    a.stats = a.partial + (long long)B * J * a.nchunks * SA_REC;   // the workspace layout is sized for SA_CHUNK chunks
    hipStream_t st = (hipStream_t)stream;
    const bool vec = !channels_last && sa3_planar_vec(a);
    int rc = LT_OK;
    if (vec) {
        a.nchunks = (int)((nvox + SAP_CHUNK - 1) / SAP_CHUNK);    // fewer, larger chunks: the records fit a fortiori
        hipLaunchKernelGGL(sa3_partial_planar_kernel, dim3(a.nchunks, B), dim3(256), 0, st, a);
        LT_CHECK_LAUNCH("lt_softargmax3d_fwd(partial, planar)");
    } else {
        rc = channels_last ? sa3_launch_partial<true>(a, B, st) : sa3_launch_partial<false>(a, B, st);
    }
    if (rc != LT_OK) return rc;
    hipLaunchKernelGGL(sa3_finalize_kernel, dim3(B * J), dim3(64), 0, st, a, B);
    LT_CHECK_LAUNCH("lt_softargmax3d_fwd(finalize)");
    if (with_stats) {
        SA3StatArgs sa;
        sa.a = a; sa.out = stats; sa.peak_index = peak_index; sa.snchunks = a.nchunks;
        sa.spart = (float*)((char*)workspace + lt_softargmax3d_workspace(B, J, nvox));   // behind the plain call's workspace, sized for SA_CHUNK chunks as well
        const dim3 grid(sa.snchunks, B);
        if (channels_last) hipLaunchKernelGGL(sa3_probs_stats_kernel<true>, grid, dim3(256), 256 * (J | 1) * sizeof(float), st, sa);
        else if (vec) hipLaunchKernelGGL(sa3_probs_stats_planar_kernel, grid, dim3(256), 0, st, sa);
        else hipLaunchKernelGGL(sa3_probs_stats_kernel<false>, grid, dim3(256), 0, st, sa);
        LT_CHECK_LAUNCH("lt_softargmax3d_stats_fwd(probs + statistics)");
        hipLaunchKernelGGL(sa3_stats_finalize_kernel, dim3(B * J), dim3(64), 0, st, sa);
        LT_CHECK_LAUNCH("lt_softargmax3d_stats_fwd(finalize)");
    } else if (probs) {
        const dim3 grid(a.nchunks, B);
        if (channels_last) hipLaunchKernelGGL(sa3_probs_kernel<true>, grid, dim3(256), 256 * (J | 1) * sizeof(float), st, a);
        else if (vec)
            hipLaunchKernelGGL(sa3_probs_planar_kernel, dim3((unsigned)((nvox / 4 + 1023) / 1024), B * J), dim3(256), 0, st, a);
        else hipLaunchKernelGGL(sa3_probs_kernel<false>, grid, dim3(256), 0, st, a);
        LT_CHECK_LAUNCH("lt_softargmax3d_fwd(probs)");
    }
    return LT_OK;
}

extern "C" int lt_softargmax3d_fwd(const float* logits, const float* coords, float mult, int32_t softmax, int32_t channels_last,
                                   int32_t ld, float* kp, float* probs, int32_t B, int32_t J, int64_t nvox, void* workspace,
                                   void* stream) {
    return sa3_forward("lt_softargmax3d_fwd", logits, coords, mult, softmax, channels_last, ld, kp, probs, nullptr, nullptr, false, B, J, nvox, workspace, stream);
}

extern "C" size_t lt_softargmax3d_stats_workspace(int32_t B, int32_t J, int64_t nvox) {
    const int64_t nchunks = (nvox + SA_CHUNK - 1) / SA_CHUNK;
    return lt_softargmax3d_workspace(B, J, nvox) + (size_t)((int64_t)B * J * nchunks * SS_REC) * sizeof(float);
}

extern "C" int lt_softargmax3d_stats_fwd(const float* logits, const float* coords, float mult, int32_t softmax, int32_t channels_last, int32_t ld, float* kp,
                                         float* probs, float* stats, int32_t* peak_index, int32_t B, int32_t J, int64_t nvox, void* workspace, void* stream) {
    return sa3_forward("lt_softargmax3d_stats_fwd", logits, coords, mult, softmax, channels_last, ld, kp, probs, stats, peak_index, true, B, J, nvox, workspace,
                       stream);
}

extern "C" int lt_softargmax2d_fwd(const float* heatmaps, float mult, int32_t softmax, float* coords, float* probs, int32_t NJ,
                                   int32_t h, int32_t w, void* stream) {
    LT_REQUIRE(heatmaps && coords && NJ >= 1 && h >= 1 && w >= 1, LT_ERR_INVALID, "lt_softargmax2d_fwd: bad argument");
    hipLaunchKernelGGL(sa2_kernel, dim3(NJ), dim3(256), 0, (hipStream_t)stream, heatmaps, mult, softmax, coords, probs, h, w);
    LT_CHECK_LAUNCH("lt_softargmax2d_fwd");
    return LT_OK;
}

extern "C" int lt_triangulate_dlt(const float* proj, const float* points, const float* conf, float* out, int32_t B, int32_t NV,
                                  int32_t J, void* stream) {
    LT_REQUIRE(proj && points && out && B >= 1 && NV >= 2 && J >= 1, LT_ERR_INVALID, "lt_triangulate_dlt: bad argument");
    hipLaunchKernelGGL(dlt_kernel, dim3((B * J + 63) / 64), dim3(64), 0, (hipStream_t)stream, proj, points, conf, out, B, NV, J);
    LT_CHECK_LAUNCH("lt_triangulate_dlt");
    return LT_OK;
}

extern "C" int lt_softargmax2d_stats_fwd(const float* heatmaps, float mult, int32_t softmax, float* coords, float* probs, float* stats, int32_t* peak_index,
                                         int32_t NJ, int32_t h, int32_t w, void* stream) {
    const char* who = "lt_softargmax2d_stats_fwd";
    LT_REQUIRE(heatmaps && coords, LT_ERR_INVALID, "%s: null heatmaps or coords", who);
    LT_REQUIRE(stats, LT_ERR_INVALID, "%s: null stats", who);
    LT_REQUIRE(peak_index, LT_ERR_INVALID, "%s: null peak_index", who);
    LT_REQUIRE(NJ >= 1 && h >= 1 && w >= 1, LT_ERR_INVALID, "%s: bad shape (NJ %d, h %d, w %d)", who, NJ, h, w);
    LT_REQUIRE((int64_t)h * w <= 0x7fffffff, LT_ERR_UNSUPPORTED, "%s: h * w = %lld does not fit the int32 index of a heatmap", who, (long long)h * w);
    hipLaunchKernelGGL(sa2_stats_kernel, dim3(NJ), dim3(256), 0, (hipStream_t)stream, heatmaps, mult, softmax, coords, probs, stats, peak_index, h, w);
    LT_CHECK_LAUNCH(who);
    return LT_OK;
}

extern "C" int lt_triangulate_dlt_stats(const float* proj, const float* points, const float* conf, const float* cov2d, const uint8_t* view_mask, float* out,
                                        float* reproj_err, float* cov3d, int32_t B, int32_t NV, int32_t J, void* stream) {
    const char* who = "lt_triangulate_dlt_stats";
    LT_REQUIRE(proj && points && out, LT_ERR_INVALID, "%s: null proj, points or out", who);
    LT_REQUIRE(cov2d, LT_ERR_INVALID, "%s: null cov2d", who);
    LT_REQUIRE(reproj_err, LT_ERR_INVALID, "%s: null reproj_err", who);
    LT_REQUIRE(cov3d, LT_ERR_INVALID, "%s: null cov3d", who);
    LT_REQUIRE(B >= 1 && NV >= 2 && J >= 1, LT_ERR_INVALID, "%s: bad shape (B %d, NV %d, J %d)", who, B, NV, J);
    hipLaunchKernelGGL(dlt_stats_kernel, dim3((B * J + 63) / 64), dim3(64), 0, (hipStream_t)stream, proj, points, conf, cov2d, view_mask, out, reproj_err, cov3d, B,
                       NV, J);
    LT_CHECK_LAUNCH(who);
    return LT_OK;
}

// the one checked launch behind lt_alg_tail_fwd, lt_alg_tail_masked_fwd and lt_alg_tail_stats_fwd
template <bool MASKED, bool STATS>
static int alg_tail_launch(const char* name, const float* keypoints_hm, const float* conf_raw, int32_t ld_conf, const float* proj, float scale_x, float scale_y,
                           const uint8_t* view_mask, float* keypoints_2d, float* confidences, float* keypoints_3d, int32_t B, int32_t NV, int32_t J, void* stream,
                           const AlgTailStats so = AlgTailStats()) {
    LT_REQUIRE(keypoints_hm && proj && keypoints_3d, LT_ERR_INVALID, "%s: null argument", name);
    LT_REQUIRE(!MASKED || view_mask, LT_ERR_INVALID, "%s: null view_mask", name);
    LT_REQUIRE(!STATS || so.stats2d, LT_ERR_INVALID, "%s: null stats2d", name);
    LT_REQUIRE(!STATS || so.cov2d, LT_ERR_INVALID, "%s: null cov2d_img", name);
    LT_REQUIRE(!STATS || so.reproj, LT_ERR_INVALID, "%s: null reproj_err", name);
    LT_REQUIRE(!STATS || so.cov3d, LT_ERR_INVALID, "%s: null cov3d", name);
    LT_REQUIRE(B >= 1 && NV >= 2 && J >= 1, LT_ERR_INVALID, "%s: bad shape (B %d, NV %d, J %d)", name, B, NV, J);
    LT_REQUIRE(!conf_raw || ld_conf >= J, LT_ERR_INVALID, "%s: ld_conf %d < J %d", name, ld_conf, J);
    if (STATS)
        hipLaunchKernelGGL(alg_tail_stats_kernel<MASKED>, dim3((B * J + 63) / 64), dim3(64), 0, (hipStream_t)stream, keypoints_hm, conf_raw, ld_conf, proj, scale_x,
                           scale_y, view_mask, keypoints_2d, confidences, keypoints_3d, B, NV, J, so);
    else
        hipLaunchKernelGGL(alg_tail_kernel<MASKED>, dim3((B * J + 63) / 64), dim3(64), 0, (hipStream_t)stream, keypoints_hm, conf_raw, ld_conf, proj, scale_x,
                           scale_y, view_mask, keypoints_2d, confidences, keypoints_3d, B, NV, J);
    LT_CHECK_LAUNCH(name);
    return LT_OK;
}

extern "C" int lt_alg_tail_stats_fwd(const float* keypoints_hm, const float* conf_raw, int32_t ld_conf, const float* proj, float scale_x, float scale_y,
                                     const uint8_t* view_mask, const float* stats2d, float* keypoints_2d, float* confidences, float* keypoints_3d,
                                     float* cov2d_img, float* reproj_err, float* cov3d, int32_t B, int32_t NV, int32_t J, void* stream) {
    AlgTailStats so = {};
    so.stats2d = stats2d; so.cov2d = cov2d_img; so.reproj = reproj_err; so.cov3d = cov3d;
    if (view_mask)
        return alg_tail_launch<true, true>("lt_alg_tail_stats_fwd", keypoints_hm, conf_raw, ld_conf, proj, scale_x, scale_y, view_mask, keypoints_2d, confidences,
                                           keypoints_3d, B, NV, J, stream, so);
    return alg_tail_launch<false, true>("lt_alg_tail_stats_fwd", keypoints_hm, conf_raw, ld_conf, proj, scale_x, scale_y, nullptr, keypoints_2d, confidences,
                                        keypoints_3d, B, NV, J, stream, so);
}

extern "C" int lt_alg_tail_fwd(const float* keypoints_hm, const float* conf_raw, int32_t ld_conf, const float* proj, float scale_x, float scale_y,
                               float* keypoints_2d, float* confidences, float* keypoints_3d, int32_t B, int32_t NV, int32_t J, void* stream) {
    return alg_tail_launch<false, false>("lt_alg_tail_fwd", keypoints_hm, conf_raw, ld_conf, proj, scale_x, scale_y, nullptr, keypoints_2d, confidences, keypoints_3d,
                                  B, NV, J, stream);
}

extern "C" int lt_alg_tail_masked_fwd(const float* keypoints_hm, const float* conf_raw, int32_t ld_conf, const float* proj, float scale_x, float scale_y,
                                      const uint8_t* view_mask, float* keypoints_2d, float* confidences, float* keypoints_3d, int32_t B, int32_t NV,
                                      int32_t J, void* stream) {
    return alg_tail_launch<true, false>("lt_alg_tail_masked_fwd", keypoints_hm, conf_raw, ld_conf, proj, scale_x, scale_y, view_mask, keypoints_2d, confidences,
                                 keypoints_3d, B, NV, J, stream);
}

extern "C" int lt_alg_tail_ragged_fwd(const float* keypoints_hm, const float* conf_raw, int32_t ld_conf, const float* proj, float scale_x, float scale_y,
                                      const int32_t* view_base, float* keypoints_2d, float* confidences, float* keypoints_3d, int32_t B, int32_t T,
                                      int32_t NVcap, int32_t J, void* stream) {
    const char* name = "lt_alg_tail_ragged_fwd";
    LT_REQUIRE(keypoints_hm && proj && keypoints_3d, LT_ERR_INVALID, "%s: null argument", name);
    LT_REQUIRE(view_base, LT_ERR_INVALID, "%s: null view_base", name);
    LT_REQUIRE(B >= 1 && T >= 1 && J >= 1, LT_ERR_INVALID, "%s: bad shape (B %d, T %d, J %d)", name, B, T, J);
    LT_REQUIRE(NVcap >= 1 && NVcap <= 32, LT_ERR_INVALID, "%s: NVcap %d (1..32)", name, NVcap);
    LT_REQUIRE((long long)B * J < (1ll << 31), LT_ERR_INVALID, "%s: B %d x J %d", name, B, J);
    LT_REQUIRE(!conf_raw || ld_conf >= J, LT_ERR_INVALID, "%s: ld_conf %d < J %d", name, ld_conf, J);
    hipLaunchKernelGGL(alg_tail_ragged_kernel, dim3((B * J + 63) / 64), dim3(64), 0, (hipStream_t)stream, keypoints_hm, conf_raw, ld_conf, proj, scale_x, scale_y,
                       view_base, keypoints_2d, confidences, keypoints_3d, B, T, NVcap, J);
    LT_CHECK_LAUNCH(name);
    return LT_OK;
}
