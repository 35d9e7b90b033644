// Per-view image preparation of the reference dataset (mvn/datasets/human36m.py:116-189, mvn/utils/img.py): crop to the bbox with
// zero fill outside the frame (PIL), cv2.resize(INTER_AREA) of the uint8 BGR crop, normalize_image + .float() -- for a ragged batch
// of views in one launch, uint8 HWC in, fp32 N,3,H,W out.
//
// The resize reproduces OpenCV 4.x cv::resize(INTER_AREA) on 8UC3 (modules/imgproc/src/resize.cpp), branch by branch, with the
// scales OpenCV uses (scale = 1 / (double)(dsize / ssize)):
//   identity   crop size == output size: a copy;
//   fast       integer factor on both axes: 2x2 -> (a+b+c+d+2)>>2 (the SIMD rule, ResizeAreaFastVec), any other kx x ky ->
//              cvRound(int sum * (1.f / (kx*ky))) (ResizeAreaFastInvoker);
//   area       both scales >= 1: computeResizeAreaTab's taps, buf = sum_x S*alpha per source row and sum = sum_y beta*buf, each in
//              increasing source index, fp32 with one rounding per operation (the library builds with -ffp-contract=off), cvRound;
//   linear     any axis upscaled: INTER_AREA's bilinear "area mode" with 11-bit weights, a horizontal int pass, then
//              (v0*b0 + v1*b1 + (1 << 21)) >> 22 (OpenCV's scalar vertical pass; its SIMD pass can differ by one level).
// mvn/utils/img.py:resize_area_u8 states the same arithmetic in numpy.
//
// One workgroup = IP_ROWS output rows of one view.  It builds the x taps of every output column and the y taps of its rows in LDS,
// computed in fp64 once per workgroup (not per lane); then each lane produces whole output pixels (three channels) and stores
// them as coalesced fp32 rows of the planar output, through the 3x256 normalisation LUT when one is given.
#include "lt_common.h"

using namespace lt;

namespace {

constexpr int IP_THREADS = 256;
constexpr int IP_ROWS = 8;
constexpr int IP_MAX_W = 2048;       // x tables: 5 x 4 B per output column in dynamic LDS (<= 40 KB)
enum { M_IDENT = 0, M_FAST2 = 1, M_FAST = 2, M_AREA = 3, M_LINEAR = 4 };

struct View {
    const uint8_t* base;
    long long pitch;
    int rh, rw, left, upper;
};

// crop pixel (y, x), 3 channels; zero outside the region (PIL's crop fill)
__device__ __forceinline__ void pix(const View& v, int y, int x, int p[3]) {
    const int ry = v.upper + y, rx = v.left + x;
    if ((unsigned)ry >= (unsigned)v.rh || (unsigned)rx >= (unsigned)v.rw) {
        p[0] = p[1] = p[2] = 0;
        return;
    }
    const uint8_t* q = v.base + (long long)ry * v.pitch + 3LL * rx;
    p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
}

// computeResizeAreaTab for output index d: taps first .. first + n - 1, alpha a0 for tap 0, al for tap n - 1, am in between
__device__ void area_entry(int ssize, double scale, int d, int& first, int& n, float& a0, float& am, float& al) {
    const double f1 = d * scale, f2 = f1 + scale;
    const double cell = fmin(scale, ssize - f1);
    int s1 = (int)ceil(f1), s2 = (int)floor(f2);
    s2 = min(s2, ssize - 1);
    s1 = min(s1, s2);
    const bool hf = s1 - f1 > 1e-3, hl = f2 - s2 > 1e-3;
    am = (float)(1.0 / cell);
    const float pf = (float)((s1 - f1) / cell);
    const float pl = (float)(fmin(fmin(f2 - s2, 1.0), cell) / cell);
    first = hf ? s1 - 1 : s1;
    n = (s2 - s1) + (int)hf + (int)hl;
    a0 = hf ? pf : (n == 1 && hl ? pl : am);
    al = hl ? pl : (n == 1 && hf ? pf : am);
}

// INTER_AREA's bilinear fallback for output index d: source s0, s1 and weights w0, w1 in 1/2048
__device__ void linear_entry(int ssize, int dsize, int d, int& s0, int& s1, float& w0, float& w1) {
    const double inv = (double)dsize / ssize, scale = 1.0 / inv;
    int s = (int)floor(d * scale);
    float f = (float)((d + 1) - (s + 1) * inv);
    f = f <= 0.f ? 0.f : f - (float)(int)floorf(f);
    if (s >= ssize - 1) { f = 0.f; s = ssize - 1; }
    s0 = s;
    s1 = min(s + 1, ssize - 1);
    w0 = rintf((1.f - f) * 2048.f);
    w1 = rintf(f * 2048.f);
}

__device__ __forceinline__ float tap_alpha(int i, int n, float a0, float am, float al) { return i == 0 ? a0 : (i == n - 1 ? al : am); }

__device__ __forceinline__ int sat_u8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
__device__ __forceinline__ int round_u8(float v) { return sat_u8(__float2int_rn(v)); }   // saturate_cast<uchar>(float): cvRound, half to even

__global__ __launch_bounds__(IP_THREADS) void crop_resize_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ desc, int H, int W,
                                                                 const float* __restrict__ lut, float* __restrict__ out) {
    extern __shared__ float ip_smem[];
    int* xi0 = (int*)ip_smem;             // area: first tap; linear: s0
    int* xi1 = xi0 + W;                   // area: taps;      linear: s1
    float* xa0 = (float*)(xi1 + W);       // area: alpha of the first tap; linear: w0
    float* xa1 = xa0 + W;                 // area: alpha of a whole tap;   linear: w1
    float* xa2 = xa1 + W;                 // area: alpha of the last tap
    __shared__ int yi0[IP_ROWS], yi1[IP_ROWS];
    __shared__ float ya0[IP_ROWS], ya1[IP_ROWS], ya2[IP_ROWS];

    const int n = blockIdx.y, t = threadIdx.x, dy0 = blockIdx.x * IP_ROWS;
    const int64_t* d = desc + (long long)n * 8;
    View v;
    v.base = src + d[0];
    v.rh = (int)d[1];
    v.rw = (int)d[2];
    v.pitch = d[3];
    v.left = (int)d[4];
    v.upper = (int)d[5];
    const int sw = (int)(d[6] - d[4]), sh = (int)(d[7] - d[5]);
    float* o = out + (long long)n * 3 * H * W;
    const int rows = min(IP_ROWS, H - dy0);
    const long long plane = (long long)H * W;

    if (sw <= 0 || sh <= 0) {            // refused on the host when the caller passes desc_host; never read from
        for (int r = 0; r < rows; ++r)
            for (int dx = t; dx < W; dx += IP_THREADS)
                for (int c = 0; c < 3; ++c) o[c * plane + (long long)(dy0 + r) * W + dx] = 0.f;
        return;
    }

    int mode, kx = 1, ky = 1;
    const double scx = 1.0 / ((double)W / sw), scy = 1.0 / ((double)H / sh);
    if (sw == W && sh == H) {
        mode = M_IDENT;
    } else {
        kx = __double2int_rn(scx);
        ky = __double2int_rn(scy);
        const bool fast = fabs(scx - kx) < 2.220446049250313e-16 && fabs(scy - ky) < 2.220446049250313e-16;
        if (scx >= 1.0 && scy >= 1.0)
            mode = fast ? ((kx == 2 && ky == 2) ? M_FAST2 : M_FAST) : M_AREA;
        else
            mode = M_LINEAR;
    }

    if (mode == M_AREA) {
        for (int dx = t; dx < W; dx += IP_THREADS) area_entry(sw, scx, dx, xi0[dx], xi1[dx], xa0[dx], xa1[dx], xa2[dx]);
        if (t < rows) area_entry(sh, scy, dy0 + t, yi0[t], yi1[t], ya0[t], ya1[t], ya2[t]);
    } else if (mode == M_LINEAR) {
        for (int dx = t; dx < W; dx += IP_THREADS) linear_entry(sw, W, dx, xi0[dx], xi1[dx], xa0[dx], xa1[dx]);
        if (t < rows) linear_entry(sh, H, dy0 + t, yi0[t], yi1[t], ya0[t], ya1[t]);
    }
    __syncthreads();

    const float rcp_area = 1.f / (float)(kx * ky);
    for (int r = 0; r < rows; ++r) {
        const int dy = dy0 + r;
        for (int dx = t; dx < W; dx += IP_THREADS) {
            int q[3];
            if (mode == M_IDENT) {
                pix(v, dy, dx, q);
            } else if (mode == M_FAST2 || mode == M_FAST) {
                int s[3] = {0, 0, 0};
                for (int j = 0; j < ky; ++j)
                    for (int i = 0; i < kx; ++i) {
                        int p[3];
                        pix(v, dy * ky + j, dx * kx + i, p);
                        s[0] += p[0]; s[1] += p[1]; s[2] += p[2];
                    }
                for (int c = 0; c < 3; ++c) q[c] = mode == M_FAST2 ? (s[c] + 2) >> 2 : round_u8((float)s[c] * rcp_area);
            } else if (mode == M_AREA) {
                const int fx = xi0[dx], nx = xi1[dx], fy = yi0[r], ny = yi1[r];
                const float a0 = xa0[dx], am = xa1[dx], al = xa2[dx];
                float sum[3] = {0.f, 0.f, 0.f};
                for (int j = 0; j < ny; ++j) {
                    const float beta = tap_alpha(j, ny, ya0[r], ya1[r], ya2[r]);
                    float b[3] = {0.f, 0.f, 0.f};
                    for (int i = 0; i < nx; ++i) {
                        const float alpha = tap_alpha(i, nx, a0, am, al);
                        int p[3];
                        pix(v, fy + j, fx + i, p);
                        for (int c = 0; c < 3; ++c) b[c] = b[c] + (float)p[c] * alpha;
                    }
                    for (int c = 0; c < 3; ++c) sum[c] = sum[c] + beta * b[c];
                }
                for (int c = 0; c < 3; ++c) q[c] = round_u8(sum[c]);
            } else {
                const int x0 = xi0[dx], x1 = xi1[dx], wx0 = (int)xa0[dx], wx1 = (int)xa1[dx];
                const int y0 = yi0[r], y1 = yi1[r], wy0 = (int)ya0[r], wy1 = (int)ya1[r];
                int p00[3], p01[3], p10[3], p11[3];
                pix(v, y0, x0, p00); pix(v, y0, x1, p01);
                pix(v, y1, x0, p10); pix(v, y1, x1, p11);
                for (int c = 0; c < 3; ++c) {
                    const int h0 = p00[c] * wx0 + p01[c] * wx1, h1 = p10[c] * wx0 + p11[c] * wx1;
                    q[c] = sat_u8((h0 * wy0 + h1 * wy1 + (1 << 21)) >> 22);
                }
            }
            float* od = o + (long long)dy * W + dx;
            for (int c = 0; c < 3; ++c) od[c * plane] = lut ? lut[c * 256 + q[c]] : (float)q[c];
        }
    }
}

}  // namespace

extern "C" int lt_crop_resize_u8(const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int64_t* desc_host, int32_t N, int32_t H,
                                 int32_t W, const float* lut, float* out, void* stream) {
    LT_REQUIRE(N > 0 && H > 0 && W > 0, LT_ERR_INVALID, "lt_crop_resize_u8: N, H, W must be > 0 (N=%d H=%d W=%d)", N, H, W);
    LT_REQUIRE(N <= 65535, LT_ERR_UNSUPPORTED, "lt_crop_resize_u8: at most 65535 views per call (N=%d)", N);
    LT_REQUIRE(W <= IP_MAX_W, LT_ERR_UNSUPPORTED, "lt_crop_resize_u8: W <= %d (W=%d)", IP_MAX_W, W);
    LT_REQUIRE(src && desc && out && src_bytes >= 0, LT_ERR_INVALID, "lt_crop_resize_u8: NULL src / desc / out");
    if (desc_host) {
        const long long lim = 1LL << 30;
        for (int i = 0; i < N; ++i) {
            const int64_t* d = desc_host + (long long)i * 8;
            const long long off = d[0], rh = d[1], rw = d[2], pitch = d[3];
            LT_REQUIRE(d[6] > d[4] && d[7] > d[5], LT_ERR_INVALID, "lt_crop_resize_u8: view %d has an empty bbox (%lld, %lld, %lld, %lld)", i,
                       (long long)d[4], (long long)d[5], (long long)d[6], (long long)d[7]);
            for (int k = 4; k < 8; ++k)
                LT_REQUIRE(d[k] > -lim && d[k] < lim, LT_ERR_INVALID, "lt_crop_resize_u8: view %d: bbox coordinate out of range", i);
            LT_REQUIRE(d[6] - d[4] < lim && d[7] - d[5] < lim, LT_ERR_INVALID, "lt_crop_resize_u8: view %d: bbox too large", i);
            LT_REQUIRE(rh >= 0 && rw >= 0 && rh < lim && rw < lim && off >= 0 && pitch >= 3 * rw, LT_ERR_INVALID,
                       "lt_crop_resize_u8: view %d: bad region (offset %lld, %lld x %lld, pitch %lld)", i, off, rh, rw, pitch);
            LT_REQUIRE(rh == 0 || rw == 0 || off + (rh - 1) * pitch + 3 * rw <= src_bytes, LT_ERR_INVALID,
                       "lt_crop_resize_u8: view %d: region ends past src (%lld bytes)", i, (long long)src_bytes);
        }
    }
    const size_t lds = (size_t)W * 5 * 4;
    dim3 grid((H + IP_ROWS - 1) / IP_ROWS, N);
    hipLaunchKernelGGL(crop_resize_kernel, grid, dim3(IP_THREADS), lds, (hipStream_t)stream, src, desc, H, W, lut, out);
    LT_CHECK_LAUNCH("lt_crop_resize_u8");
    return LT_OK;
}
