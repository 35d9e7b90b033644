// 2D heatmap targets and the heatmap loss of the backbone's own training step (the reference's op.py:169-196, gaussian_2d_pdf /
// render_points_as_2d_gaussians, and the MSE between predicted heatmaps and those targets).
//
// Both kernels are streams over a few MB (17 joints x 96 x 96 floats per image): one 256-thread workgroup (four wave64) per heatmap.  The target is
// separable, G[y][x] = ex[x] * ey[y], so the w + h one-dimensional factors go into LDS once per heatmap (w + h expf calls instead of w * h) and the
// body is one product per pixel.  The loss reads the prediction once and, when asked, writes the gradient in the same pass; the target itself never
// reaches memory.  Rows move as float4 when w % 4 == 0 and the tensors are 16-byte aligned (every row base is then), one float at a time otherwise.
// Sums: lanes add in index order, the wave butterfly and the four waves in a fixed order (the block_reduce pattern of softargmax.hip) -- no atomics,
// equal bits every call.
#include "lt_common.h"

using namespace lt;

namespace {

constexpr int HM_MAX_HW = 8192;          // h + w floats of LDS (32 KB): far beyond any heatmap of the networks here

__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
    for (int w = 1; w < 4; ++w) r += red[w];
    return r;
}

// ex[0..w) = exp(-(x - px)^2 / (2 sx^2)), ey[0..h) = exp(-(y - py)^2 / (2 sy^2)) / norm.  The exponent's argument is formed in fp64 (w + h values per
// heatmap) so that expf sees it rounded once; norm = 2 pi sx SX -- sigma_x TWICE, as gaussian_2d_pdf of the reference has it (op.py:172), kept on purpose.
__device__ __forceinline__ void gauss_factors(const float* __restrict__ pt, const float* __restrict__ sg, int normalize, int h, int w, float* ex, float* ey) {
    const double px = (double)pt[0], py = (double)pt[1], sx = (double)sg[0], sy = (double)sg[1];
    const float inv_norm = normalize ? (float)(1.0 / (6.283185307179586476925286766559 * sx * sx)) : 1.f;
    for (int i = threadIdx.x; i < w + h; i += 256) {
        const bool isx = i < w;
        const double d = isx ? (double)i - px : (double)(i - w) - py;
        const double s = isx ? sx : sy;
        const float e = expf((float)(-0.5 * (d * d) / (s * s)));
        ex[i] = isx ? e : e * inv_norm;          // (ey lives behind ex in the same array)
    }
    __syncthreads();
}

template <bool VEC>
__global__ __launch_bounds__(256) void render_gaussians_kernel(const float* __restrict__ points, const float* __restrict__ sigmas, float* __restrict__ out,
                                                                int h, int w, int normalize) {
    extern __shared__ float fac[];          // ex[w] | ey[h]
    const long long base = (long long)blockIdx.x * h * w;
    gauss_factors(points + (long long)blockIdx.x * 2, sigmas + (long long)blockIdx.x * 2, normalize, h, w, fac, fac + w);
    const float* ex = fac;
    const float* ey = fac + w;
    if (VEC) {
        const int w4 = w >> 2, n4 = h * w4;
        for (int q = threadIdx.x; q < n4; q += 256) {
            const int yy = q / w4, x0 = (q - yy * w4) << 2;
            const float gy = ey[yy];
            *(float4*)(out + base + (long long)yy * w + x0) = make_float4(ex[x0] * gy, ex[x0 + 1] * gy, ex[x0 + 2] * gy, ex[x0 + 3] * gy);
        }
    } else {
        const int n = h * w;
        for (int i = threadIdx.x; i < n; i += 256) {
            const int yy = i / w, xx = i - yy * w;
            out[base + i] = ex[xx] * ey[yy];
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void heatmap_mse_kernel(const float* __restrict__ pred, const float* __restrict__ points, const float* __restrict__ sigmas,
                                                           const float* __restrict__ validity, int normalize, float* __restrict__ terms,
                                                           float* __restrict__ gpred, int NJ, int h, int w) {
    extern __shared__ float fac[];          // ex[w] | ey[h]
    __shared__ float red[4];
    const long long base = (long long)blockIdx.x * h * w;
    const int n = h * w;
    const float v = validity ? validity[blockIdx.x] : 1.f;          // uniform over the workgroup: the branches below are taken by all 256 lanes
    if (v == 0.f) {
        // an unannotated joint: its keypoint and sigmas are NEVER read (they may be NaN), its term and its gradient row are exact zeros
        if (threadIdx.x == 0) terms[blockIdx.x] = 0.f;
        if (gpred) {
            if (VEC) {
                for (int q = threadIdx.x; q < (n >> 2); q += 256) *(float4*)(gpred + base + ((long long)q << 2)) = make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                for (int i = threadIdx.x; i < n; i += 256) gpred[base + i] = 0.f;
            }
        }
        return;
    }
    float gs = 0.f;
    if (gpred) {
        // sum of the validities, re-added by every workgroup in the same fixed order (NJ is a few hundred): no pre-pass, no host round trip, no atomics
        float s = 0.f;
        if (validity)
            for (int i = threadIdx.x; i < NJ; i += 256) s += validity[i];
        const float nv = validity ? block_sum(s, red) : (float)NJ;
        gs = 2.f * v / ((float)h * (float)w * fmaxf(1.f, nv));
    }
    gauss_factors(points + (long long)blockIdx.x * 2, sigmas + (long long)blockIdx.x * 2, normalize, h, w, fac, fac + w);
    const float* ex = fac;
    const float* ey = fac + w;
    float acc = 0.f;
    if (VEC) {
        const int w4 = w >> 2, n4 = h * w4;
        for (int q = threadIdx.x; q < n4; q += 256) {
            const int yy = q / w4, x0 = (q - yy * w4) << 2;
            const long long o = base + (long long)yy * w + x0;
            const float gy = ey[yy];
            const float4 p = *(const float4*)(pred + o);
            const float d0 = p.x - ex[x0] * gy, d1 = p.y - ex[x0 + 1] * gy, d2 = p.z - ex[x0 + 2] * gy, d3 = p.w - ex[x0 + 3] * gy;
            acc += d0 * d0; acc += d1 * d1; acc += d2 * d2; acc += d3 * d3;
            if (gpred) *(float4*)(gpred + o) = make_float4(gs * d0, gs * d1, gs * d2, gs * d3);
        }
    } else {
        for (int i = threadIdx.x; i < n; i += 256) {
            const int yy = i / w, xx = i - yy * w;
            const float d = pred[base + i] - ex[xx] * ey[yy];
            acc += d * d;
            if (gpred) gpred[base + i] = gs * d;
        }
    }
    const float total = block_sum(acc, red);
    if (threadIdx.x == 0) terms[blockIdx.x] = v * total;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int lt_render_gaussians_2d(const float* points, const float* sigmas, float* out, int32_t n, int32_t h, int32_t w, int32_t normalize, void* stream) {
    LT_REQUIRE(points && sigmas && out, LT_ERR_INVALID, "lt_render_gaussians_2d: null points, sigmas or out");
    LT_REQUIRE(n >= 1 && h >= 1 && w >= 1, LT_ERR_INVALID, "lt_render_gaussians_2d: bad shape (n %d, h %d, w %d)", n, h, w);
    LT_REQUIRE((int64_t)h * w < 0x80000000LL, LT_ERR_INVALID, "lt_render_gaussians_2d: h * w = %lld does not fit the int32 index of a heatmap", (long long)h * w);
    LT_REQUIRE((int64_t)h + w <= HM_MAX_HW, LT_ERR_UNSUPPORTED, "lt_render_gaussians_2d: h + w = %lld > %d (the row and column factors live in LDS)", (long long)h + w, HM_MAX_HW);
    const size_t lds = (size_t)(h + w) * sizeof(float);
    if ((w & 3) == 0 && aligned16(out))
        hipLaunchKernelGGL(render_gaussians_kernel<true>, dim3(n), dim3(256), lds, (hipStream_t)stream, points, sigmas, out, h, w, normalize);
    else
        hipLaunchKernelGGL(render_gaussians_kernel<false>, dim3(n), dim3(256), lds, (hipStream_t)stream, points, sigmas, out, h, w, normalize);
    LT_CHECK_LAUNCH("lt_render_gaussians_2d");
    return LT_OK;
}

extern "C" int lt_heatmap_mse_fwd(const float* pred, const float* points, const float* sigmas, const float* validity, int32_t normalize, float* terms,
                                  float* grad_pred, int32_t NJ, int32_t h, int32_t w, void* stream) {
    LT_REQUIRE(pred && points && sigmas && terms, LT_ERR_INVALID, "lt_heatmap_mse_fwd: null pred, points, sigmas or terms");
    LT_REQUIRE(NJ >= 1 && h >= 1 && w >= 1, LT_ERR_INVALID, "lt_heatmap_mse_fwd: bad shape (NJ %d, h %d, w %d)", NJ, h, w);
    LT_REQUIRE((int64_t)h * w < 0x80000000LL, LT_ERR_INVALID, "lt_heatmap_mse_fwd: h * w = %lld does not fit the int32 index of a heatmap", (long long)h * w);
    LT_REQUIRE((int64_t)h + w <= HM_MAX_HW, LT_ERR_UNSUPPORTED, "lt_heatmap_mse_fwd: h + w = %lld > %d (the row and column factors live in LDS)", (long long)h + w, HM_MAX_HW);
    const size_t lds = (size_t)(h + w) * sizeof(float);
    if ((w & 3) == 0 && aligned16(pred) && aligned16(grad_pred))
        hipLaunchKernelGGL(heatmap_mse_kernel<true>, dim3(NJ), dim3(256), lds, (hipStream_t)stream, pred, points, sigmas, validity, normalize, terms, grad_pred, NJ, h, w);
    else
        hipLaunchKernelGGL(heatmap_mse_kernel<false>, dim3(NJ), dim3(256), lds, (hipStream_t)stream, pred, points, sigmas, validity, normalize, terms, grad_pred, NJ, h, w);
    LT_CHECK_LAUNCH("lt_heatmap_mse_fwd");
    return LT_OK;
}
