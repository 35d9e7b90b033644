// Per-view image preparation of the reference dataset (mvn/datasets/human36m.py:116-189, mvn/utils/img.py): crop to the bbox with
// zero fill outside the frame (PIL), cv2.resize(INTER_AREA) of the uint8 BGR crop, normalize_image + .float() -- for a ragged batch
// of views in one launch, uint8 HWC in, fp32 N,3,H,W out.
// lt_undistort_crop_resize_u8 puts the reference's offline lens undistortion (cv2.remap INTER_CUBIC, see RemapView) in front of the
// crop: the same kernel template with a different pixel fetch.
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

__device__ __forceinline__ int sat_u8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
__device__ __forceinline__ int round_u8(float v) { return sat_u8(__float2int_rn(v)); }   // saturate_cast<uchar>(float): cvRound, half to even

struct View {
    static constexpr int FIELDS = 8;
    const uint8_t* base;
    long long pitch;
    int rh, rw, left, upper, sw, sh;

    __device__ View(const uint8_t* src, const uint8_t*, const int64_t* d) {
        base = src + d[0];
        rh = (int)d[1];
        rw = (int)d[2];
        pitch = d[3];
        left = (int)d[4];
        upper = (int)d[5];
        sw = (int)(d[6] - d[4]);
        sh = (int)(d[7] - d[5]);
    }

    // crop pixel (y, x), 3 channels; zero outside the region (PIL's crop fill)
    __device__ __forceinline__ void pix(int y, int x, int p[3]) const {
        const int ry = upper + y, rx = left + x;
        if ((unsigned)ry >= (unsigned)rh || (unsigned)rx >= (unsigned)rw) {
            p[0] = p[1] = p[2] = 0;
            return;
        }
        const uint8_t* q = base + (long long)ry * pitch + 3LL * rx;
        p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
    }
};

// ---- lens undistortion: cv2.remap(frame, map1, map2, INTER_CUBIC) of OpenCV 4.x (modules/imgproc/src/imgwarp.cpp) on 8UC3 ----
// initInterTab2D(INTER_CUBIC, fixpt = true), evaluated by the compiler in IEEE fp32 (interpolateCubic, A = -0.75), cvRound(v * 32768)
// half to even, then the one-entry correction that makes every 4 x 4 block sum to 32768.  mvn/utils/img.py:cubic_tab states the
// same table in numpy.
constexpr int IT_SIZE = 32, IT_COEF_BITS = 15;

struct CubicTab {
    short w[IT_SIZE * IT_SIZE * 16];
};

constexpr int cv_round(float v) {     // |v| < 2^23: v - trunc(v) is exact
    const int t = (int)v;
    const float d = v - (float)t;
    if (d > 0.5f || (d == 0.5f && (t & 1))) return t + 1;
    if (d < -0.5f || (d == -0.5f && (t & 1))) return t - 1;
    return t;
}

constexpr void interpolate_cubic(float x, float* c) {
    const float A = -0.75f;
    c[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
    c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
    c[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
    c[3] = 1.f - c[0] - c[1] - c[2];
}

constexpr CubicTab make_cubic_tab() {
    CubicTab t{};
    float tab1[IT_SIZE * 4] = {};
    const float scale = 1.f / IT_SIZE;
    for (int i = 0; i < IT_SIZE; ++i) interpolate_cubic(i * scale, tab1 + 4 * i);
    for (int i = 0; i < IT_SIZE; ++i)
        for (int j = 0; j < IT_SIZE; ++j) {
            short* it = t.w + (i * IT_SIZE + j) * 16;
            int isum = 0;
            for (int k1 = 0; k1 < 4; ++k1)
                for (int k2 = 0; k2 < 4; ++k2) {
                    const int q = cv_round(tab1[i * 4 + k1] * tab1[j * 4 + k2] * (float)(1 << IT_COEF_BITS));
                    it[k1 * 4 + k2] = (short)(q < -32768 ? -32768 : (q > 32767 ? 32767 : q));
                    isum += it[k1 * 4 + k2];
                }
            const int diff = isum - (1 << IT_COEF_BITS);
            if (diff != 0) {
                int mk = 2 * 4 + 2, Mk = 2 * 4 + 2;
                for (int k1 = 2; k1 < 4; ++k1)
                    for (int k2 = 2; k2 < 4; ++k2) {
                        if (it[k1 * 4 + k2] < it[mk]) mk = k1 * 4 + k2;
                        else if (it[k1 * 4 + k2] > it[Mk]) Mk = k1 * 4 + k2;
                    }
                if (diff < 0) it[Mk] = (short)(it[Mk] - diff);
                else it[mk] = (short)(it[mk] - diff);
            }
        }
    return t;
}

__constant__ CubicTab c_cubic = make_cubic_tab();

// One view of lt_undistort_crop_resize_u8: crop pixel (y, x) is the remap of frame pixel (upper + y, left + x), zero outside the frame
// (PIL's crop fill).  The map entry of a frame pixel is int16 (x, y, map2, 0); its 4 x 4 taps start at (x - 1, y - 1) and read the
// shipped source window, which holds every tap inside the frame (mvn/utils/img.py:source_window): a tap outside the window is outside
// the frame and reads 0 (BORDER_CONSTANT, value 0).
struct RemapView {
    static constexpr int FIELDS = 14;
    const uint8_t* win;
    const uint2* map;
    long long pitch, mpitch;
    int wh, ww, wx0, wy0, fh, fw, left, upper, sw, sh;

    __device__ RemapView(const uint8_t* src, const uint8_t* maps, const int64_t* d) {
        win = src + d[0];
        wh = (int)d[1];
        ww = (int)d[2];
        pitch = d[3];
        wx0 = (int)d[4];
        wy0 = (int)d[5];
        fh = (int)d[6];
        fw = (int)d[7];
        left = (int)d[8];
        upper = (int)d[9];
        sw = (int)(d[10] - d[8]);
        sh = (int)(d[11] - d[9]);
        map = (const uint2*)(maps + d[12]);
        mpitch = d[13];
    }

    __device__ __forceinline__ void pix(int y, int x, int p[3]) const {
        const int fy = upper + y, fx = left + x;
        if ((unsigned)fy >= (unsigned)fh || (unsigned)fx >= (unsigned)fw) {
            p[0] = p[1] = p[2] = 0;
            return;
        }
        const uint2 m = map[(long long)fy * mpitch + fx];
        const int sx = (int)(short)(m.x & 0xffffu) - 1 - wx0, sy = (int)(short)(m.x >> 16) - 1 - wy0;
        const short* w = c_cubic.w + (m.y & (IT_SIZE * IT_SIZE - 1)) * 16;
        int s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
        for (int k1 = 0; k1 < 4; ++k1) {
            const int ry = sy + k1;
            if ((unsigned)ry >= (unsigned)wh) continue;
            const uint8_t* row = win + (long long)ry * pitch;
#pragma unroll
            for (int k2 = 0; k2 < 4; ++k2) {
                const int rx = sx + k2;
                if ((unsigned)rx >= (unsigned)ww) continue;
                const int wt = w[k1 * 4 + k2];
                const uint8_t* q = row + 3 * rx;
                s0 += q[0] * wt;
                s1 += q[1] * wt;
                s2 += q[2] * wt;
            }
        }
        constexpr int half = 1 << (IT_COEF_BITS - 1);
        p[0] = sat_u8((s0 + half) >> IT_COEF_BITS);
        p[1] = sat_u8((s1 + half) >> IT_COEF_BITS);
        p[2] = sat_u8((s2 + half) >> IT_COEF_BITS);
    }
};

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

template <class V>
__global__ __launch_bounds__(IP_THREADS) void crop_resize_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ desc,
                                                                 const uint8_t* __restrict__ maps, int H, int W, const float* __restrict__ lut,
                                                                 float* __restrict__ out) {
    extern __shared__ float ip_smem[];
    int* xi0 = (int*)ip_smem;             // area: first tap; linear: s0
    int* xi1 = xi0 + W;                   // area: taps;      linear: s1
    float* xa0 = (float*)(xi1 + W);       // area: alpha of the first tap; linear: w0
    float* xa1 = xa0 + W;                 // area: alpha of a whole tap;   linear: w1
    float* xa2 = xa1 + W;                 // area: alpha of the last tap
    __shared__ int yi0[IP_ROWS], yi1[IP_ROWS];
    __shared__ float ya0[IP_ROWS], ya1[IP_ROWS], ya2[IP_ROWS];

    const int n = blockIdx.y, t = threadIdx.x, dy0 = blockIdx.x * IP_ROWS;
    const V v(src, maps, desc + (long long)n * V::FIELDS);
    const int sw = v.sw, sh = v.sh;
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
                v.pix(dy, dx, q);
            } else if (mode == M_FAST2 || mode == M_FAST) {
                int s[3] = {0, 0, 0};
                for (int j = 0; j < ky; ++j)
                    for (int i = 0; i < kx; ++i) {
                        int p[3];
                        v.pix(dy * ky + j, dx * kx + i, p);
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
                        v.pix(fy + j, fx + i, p);
                        for (int c = 0; c < 3; ++c) b[c] = b[c] + (float)p[c] * alpha;
                    }
                    for (int c = 0; c < 3; ++c) sum[c] = sum[c] + beta * b[c];
                }
                for (int c = 0; c < 3; ++c) q[c] = round_u8(sum[c]);
            } else {
                const int x0 = xi0[dx], x1 = xi1[dx], wx0 = (int)xa0[dx], wx1 = (int)xa1[dx];
                const int y0 = yi0[r], y1 = yi1[r], wy0 = (int)ya0[r], wy1 = (int)ya1[r];
                int p00[3], p01[3], p10[3], p11[3];
                v.pix(y0, x0, p00); v.pix(y0, x1, p01);
                v.pix(y1, x0, p10); v.pix(y1, x1, p11);
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
    hipLaunchKernelGGL(crop_resize_kernel<View>, grid, dim3(IP_THREADS), lds, (hipStream_t)stream, src, desc, nullptr, H, W, lut, out);
    LT_CHECK_LAUNCH("lt_crop_resize_u8");
    return LT_OK;
}

extern "C" int lt_undistort_crop_resize_u8(const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int64_t* desc_host, const int16_t* maps,
                                           int64_t maps_bytes, int32_t N, int32_t H, int32_t W, const float* lut, float* out, void* stream) {
    LT_REQUIRE(N > 0 && H > 0 && W > 0, LT_ERR_INVALID, "lt_undistort_crop_resize_u8: N, H, W must be > 0 (N=%d H=%d W=%d)", N, H, W);
    LT_REQUIRE(N <= 65535, LT_ERR_UNSUPPORTED, "lt_undistort_crop_resize_u8: at most 65535 views per call (N=%d)", N);
    LT_REQUIRE(W <= IP_MAX_W, LT_ERR_UNSUPPORTED, "lt_undistort_crop_resize_u8: W <= %d (W=%d)", IP_MAX_W, W);
    LT_REQUIRE(src && desc && maps && out && src_bytes >= 0 && maps_bytes >= 0, LT_ERR_INVALID,
               "lt_undistort_crop_resize_u8: NULL src / desc / maps / out");
    LT_REQUIRE(((uintptr_t)maps & 7) == 0, LT_ERR_INVALID, "lt_undistort_crop_resize_u8: maps must be 8-byte aligned");
    if (desc_host) {
        const long long lim = 1LL << 30;
        for (int i = 0; i < N; ++i) {
            const int64_t* d = desc_host + (long long)i * RemapView::FIELDS;
            const long long off = d[0], wh = d[1], ww = d[2], pitch = d[3], wx0 = d[4], wy0 = d[5], fh = d[6], fw = d[7];
            const long long moff = d[12], mpitch = d[13];
            LT_REQUIRE(d[10] > d[8] && d[11] > d[9], LT_ERR_INVALID, "lt_undistort_crop_resize_u8: view %d has an empty bbox (%lld, %lld, %lld, %lld)",
                       i, (long long)d[8], (long long)d[9], (long long)d[10], (long long)d[11]);
            for (int k = 8; k < 12; ++k)
                LT_REQUIRE(d[k] > -lim && d[k] < lim, LT_ERR_INVALID, "lt_undistort_crop_resize_u8: view %d: bbox coordinate out of range", i);
            LT_REQUIRE(d[10] - d[8] < lim && d[11] - d[9] < lim, LT_ERR_INVALID, "lt_undistort_crop_resize_u8: view %d: bbox too large", i);
            LT_REQUIRE(fh > 0 && fw > 0 && fh <= 32767 && fw <= 32767, LT_ERR_INVALID,
                       "lt_undistort_crop_resize_u8: view %d: bad frame size %lld x %lld", i, fh, fw);
            LT_REQUIRE(wh >= 0 && ww >= 0 && wx0 >= 0 && wy0 >= 0 && wx0 + ww <= fw && wy0 + wh <= fh, LT_ERR_INVALID,
                       "lt_undistort_crop_resize_u8: view %d: source window (%lld, %lld) + %lld x %lld leaves the %lld x %lld frame", i, wx0, wy0,
                       wh, ww, fh, fw);
            LT_REQUIRE(off >= 0 && pitch >= 3 * ww && pitch < lim, LT_ERR_INVALID,
                       "lt_undistort_crop_resize_u8: view %d: bad source window (offset %lld, pitch %lld)", i, off, pitch);
            LT_REQUIRE(wh == 0 || ww == 0 || off + (wh - 1) * pitch + 3 * ww <= src_bytes, LT_ERR_INVALID,
                       "lt_undistort_crop_resize_u8: view %d: source window ends past src (%lld bytes)", i, (long long)src_bytes);
            LT_REQUIRE(moff >= 0 && (moff & 7) == 0 && mpitch >= fw && mpitch < lim, LT_ERR_INVALID,
                       "lt_undistort_crop_resize_u8: view %d: bad map (offset %lld, pitch %lld)", i, moff, mpitch);
            LT_REQUIRE(moff + ((fh - 1) * mpitch + fw) * 8 <= maps_bytes, LT_ERR_INVALID,
                       "lt_undistort_crop_resize_u8: view %d: map ends past maps (%lld bytes)", i, (long long)maps_bytes);
        }
    }
    const size_t lds = (size_t)W * 5 * 4;
    dim3 grid((H + IP_ROWS - 1) / IP_ROWS, N);
    hipLaunchKernelGGL(crop_resize_kernel<RemapView>, grid, dim3(IP_THREADS), lds, (hipStream_t)stream, src, desc, (const uint8_t*)maps, H, W, lut,
                       out);
    LT_CHECK_LAUNCH("lt_undistort_crop_resize_u8");
    return LT_OK;
}
