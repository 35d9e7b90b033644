// bneck_kernel: a whole ResNet bottleneck block in ONE launch (identity blocks of layer1 / layer2 of the pose backbone,
// reference mvn/models/pose_resnet.py:57-95: conv1x1 -> bn -> relu -> conv3x3 -> bn -> relu -> conv1x1 -> bn -> += x -> relu).
//
// Why (VERDICT r3 "next" 1): at 96^2 / 48^2 the three launches move 16 channel-units per pixel through HBM (reduce reads 4 C' and
// writes C', the 3x3 reads and writes C', the expand reads C' + the residual 4 C' and writes 4 C'; C' = the bottleneck width P) and
// run at 0.07-0.27 of the MFMA roof because of it.  Here a workgroup owns an 8 x 16 pixel tile, reads x once (10 x 18 halo) and writes
// y once: 8 units per pixel; the two intermediate tensors never leave LDS.
//
//   phase 1  t1[hp][P]  = relu(bn1(W1 . x[hp][C]))   for the 180 halo pixels (6 blocks of 32; out-of-image pixels = 0: conv2's padding)
//            x streams through an LDS-DMA ring of 32-channel stages (180 rows x 64 B, the conv_igemm7 swizzle), W1 fragments come from
//            global memory in fragment order; transposed product D[channel][pixel]: a lane ends up with two runs of 8 consecutive
//            channels of ONE pixel, which is a 16-byte LDS store into t1 (row = halo pixel, slot XOR-swizzled by the pixel index).
//   phase 2  t2[px][P]  = relu(bn2(W2 * t1))         3x3, 128 output pixels (4 blocks of 2 rows x 16 columns); the tap offset is a
//            compile-time LDS immediate, the K block an XOR on the lane's address (one v_xor per fragment), W2 fragments from global
//            memory (each used for 4 / 2 MFMAs).  Odd rows of a pixel block are rotated by two columns so that the 16 lanes of a
//            ds_read_b128 group always hit 16 different halo pixels mod 16 = 16 different swizzle classes (conflict free for every tap).
//   phase 3  y[px][C]   = relu(bn3(W3 . t2) + x)     a wave owns C / 128 output-channel blocks x all 4 pixel blocks (every W3
//            fragment feeds 4 MFMAs); residual and result move as 16-byte channel runs straight from / to global memory.
// Four waves, <= 80 KB of LDS: two workgroups per CU overlap each other's DMA / MFMA / store phases (DESIGN rule 2).
// Weights: lt_conv_pack_weights_t32 order for all three GEMMs ([tap][K / 16][Cout / 32][lane] x 16 B, rows permuted so that MFMA row
// r carries channel 16 (r >> 4) + 8 ((r >> 2) & 1) + 4 ((r >> 3) & 1) + (r & 3)).
#include <stdlib.h>

#include <type_traits>

#include "wave_prims.h"

using namespace lt;

namespace {

__device__ uint4 g_zero_page_b[2];

// -DLT_BNECK_TRACE: shader-clock stamps at the phase boundaries of every wave of the first LT_BNECK_TRACE_WG workgroups (profiling builds only,
// read back with lt_bneck_trace_read; tools/bneck_bench.py --trace)
#ifdef LT_BNECK_TRACE
#define LT_BNECK_TRACE_WG 4096
__device__ unsigned long long g_bneck_trace[LT_BNECK_TRACE_WG * 4 * 8];
#define BN_STAMP(k)                                                                                                  \
    do {                                                                                                             \
        if (blockIdx.x < LT_BNECK_TRACE_WG && lane == 0) g_bneck_trace[(blockIdx.x * 4 + wave) * 8 + (k)] = clock64(); \
    } while (0)
#else
#define BN_STAMP(k)
#endif

struct BneckArgs {
    const bf16_t* x;
    bf16_t* y;
    const bf16_t* w1;
    const bf16_t* w2;
    const bf16_t* w3;
    const float* bias[3];    // may be null (ResNet convolutions carry no bias)
    const float* scale[3];
    const float* shift[3];
    int N, H, W, tiles_x, tiles_y;
};

// Phase 1 issue order of a wave (all of it inline asm, so the waits are counted by hand; loads return in order): prologue W1 fragments A(0 .. D-1)
// [2 loads each], ring stages DMA(0 .. AHEAD-1) [3 pieces each]; K step s issues A(s + D) and then DMA(s + AHEAD) while they exist.  Returns
// how many operations may still be outstanding at the top of step ks so that A(ks) and this wave's pieces of stage ks have landed.
template <int NK1, int AHEAD, int D>
constexpr int bneck_after(int ks) {
    int total = 0, last = 0;
    for (int k = 0; k < D && k < NK1; ++k) { total += 2; if (k == ks) last = total; }
    for (int k = 0; k < AHEAD && k < NK1; ++k) { total += 3; if (k == ks && total > last) last = total; }
    for (int s = 0; s < ks; ++s) {
        if (s + D < NK1) { total += 2; if (s + D == ks && total > last) last = total; }
        if (s + AHEAD < NK1) { total += 3; if (s + AHEAD == ks && total > last) last = total; }
    }
    return total - last;
}

template <int C, int P, int NSTR, int NHELD>
__global__ __launch_bounds__(256, 2) void bneck_kernel(const BneckArgs a) {
    typedef bf16_t T;
    constexpr int TH = 8, TW = 16, HPI = TW + 2, HROWS = (TH + 2) * HPI;   // 10 x 18 = 180 halo pixels
    constexpr int NPB = 4;                                                  // output pixel blocks of 32 (2 rows x 16 columns)
    constexpr int NCB = P / 32, NOB = C / 32, G2 = P / 16, NK1 = C / 32;
    constexpr int RB = 2 * P, NSL = P / 8;                                  // bytes / 16-byte slots per t1 / t2 row
    constexpr int T1_BYTES = HROWS * RB;
    constexpr int STAGE = HROWS * 64;                                       // a ring stage: 180 rows x 32 channels
    // the x ring of phase 1 covers the WHOLE allocation: t1 is only written when the K loop is over, so its bytes are NT1 more stages
    // (bytes in flight are what the L2 / HBM -> LDS stream is bound by: 2 x 11.5 KB per workgroup gave 2.7k cycles per K step)
    constexpr int NT1 = T1_BYTES / STAGE, NST = NT1 + NSTR;
    constexpr int T2_OFF = T1_BYTES;                                        // t2 takes the place of the ring stages behind t1 once phase 1 is over
    constexpr int AHEAD = NST - 1 < NK1 ? NST - 1 : NK1;
    constexpr int NPB1 = NCB == 4 ? 6 : 3, NPB2 = NCB == 4 ? 4 : 2, NOBW = NOB / 4;
    static_assert(NCB == 2 || NCB == 4, "bottleneck width 64 or 128");
    static_assert(T1_BYTES % STAGE == 0, "t1 is a whole number of ring stages");
    static_assert(NPB * 32 * RB <= (NSTR - 1) * STAGE + 192 * 64, "t2 fits behind t1");
    static_assert(NK1 % 2 == 0 && NHELD <= NOBW && NHELD <= 2, "K steps / held residual blocks");
    static_assert(T1_BYTES % 256 == 0 && STAGE % 256 == 0, "the XOR / bank arguments assume 256-byte aligned regions");
    auto fsw = [](int hp) -> int { return NSL == 16 ? (hp & 15) : ((hp >> 1) & 7); };

    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
    const unsigned lds0 = (unsigned)(size_t)(lptr_t)smem;
    unsigned long long zp_bits = (unsigned long long)(size_t)g_zero_page_b;
    asm volatile("" : "+s"(zp_bits));
    const void* const zero_page = (const void*)(size_t)zp_bits;

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    int lin = blockIdx.x;
    {   // XCD-aware order: XCD b % 8 walks one contiguous run of tiles (neighbouring halos and the weights meet in one L2)
        const int nb = gridDim.x, q = nb >> 3, r = nb & 7, xcd = lin & 7, j = lin >> 3;
        lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
    }
    const int tpi = a.tiles_x * a.tiles_y;
    const int img = lin / tpi, rem = lin - img * tpi;
    const int ty = rem / a.tiles_x, tx = rem - ty * a.tiles_x;
    const int y0 = ty * TH - 1, x0 = tx * TW - 1;          // image coordinates of halo pixel (0, 0)
    const T* __restrict__ x = a.x;

    const int n31 = lane & 31, hk = lane >> 5;
    const int cb = NCB == 4 ? wave : (wave & 1);           // this wave's 32-channel block of the bottleneck width (phases 1 and 2)
    const int whalf = NCB == 4 ? 0 : (wave >> 1);
    // output pixel of (block pb, lane n31): tile row 2 pb + r, column c with the odd row rotated by two columns (bank argument above)
    const int prr = n31 >> 4, pcc = ((n31 & 15) - 2 * prr) & 15;

    // the residual of this wave's first NHELD output-channel blocks (ob = wave + 4 q): K step ks of phase 1 streams channels 32 ks .. + 31 of
    // every halo pixel through the ring, i.e. exactly the residual of block ob = ks for the 128 centre pixels -- taken from LDS into registers
    // there, x is then read from memory ONCE for those channels (the blocks that are not held are read a second time in phase 3)
    uint4 held[NHELD > 0 ? NHELD : 1][NPB][2];

    // the folded BatchNorm constants of this wave's channels, requested FIRST (the oldest entries of the in-order load queue) and kept in
    // 8 registers, one float4 per lane and table; an epilogue fetches value f of a table with v_readlane (lane f / 4, component f % 4) and
    // picks the lane's half by h.  As per-element loads in front of each epilogue they were short-latency loads queued behind the residual
    // requests of the next block -- every epilogue waited for an HBM round trip.
    //   cst12: [scale1 | shift1 | scale2 | shift2][32 channels of block cb]     (lanes 0..31, mirrored in 32..63)
    //   cst3 : [q][scale3 | shift3][32 channels of block wave + 4 q]            (NOBW * 64 floats)
    float4 cst12, cst3;
    {
        const int l = lane & 31, arr = l >> 3, i4 = l & 7;
        const float* t12 = arr == 0 ? a.scale[0] : arr == 1 ? a.shift[0] : arr == 2 ? a.scale[1] : a.shift[1];
        cst12 = *(const float4*)(t12 + 32 * cb + 4 * i4);
        const int f = (4 * lane) % (NOBW * 64), q = f >> 6, which = (f >> 5) & 1, c = f & 31;
        cst3 = *(const float4*)((which ? a.shift[2] : a.scale[2]) + 32 * (wave + 4 * q) + c);
    }
    auto cget = [&](const float4& tb, int f) -> float {      // f is a compile-time constant at every call site
        const float v = (f & 3) == 0 ? tb.x : (f & 3) == 1 ? tb.y : (f & 3) == 2 ? tb.z : tb.w;
        return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), f >> 2));
    };
    // constant e (0..15) of a 32-channel table starting at float `base`: channel 16 (e >> 3) + 8 h + (e & 7)
    auto csel = [&](const float4& tb, int base, int e) -> float {
        const float lo = cget(tb, base + 16 * (e >> 3) + (e & 7)), hi = cget(tb, base + 16 * (e >> 3) + 8 + (e & 7));
        return hk ? hi : lo;
    };

    BN_STAMP(0);
    // ================================================ phase 1: t1 = relu(bn1(W1 x)) on the halo =======================================
    {
#ifndef LT_BNECK_ABL_SEG128
        const int prow = lane >> 2;
#endif
#ifdef LT_BNECK_ABL_SEG128  /* timing only: eight lanes read 128 contiguous bytes of a row (8 rows per piece) instead of four lanes 64 bytes */
        const int prow = lane >> 3;
        const int kvlog = lane & 7;
#elif defined(LT_BNECK_ABL_NOSWZ)   /* timing only: is the permuted 16-byte order inside a row's 64 bytes what the address path pays for? */
        const int kvlog = lane & 3;
#else
        const int kvlog = (lane & 3) ^ swz64(prow);
#endif
        int dbase[3];
        bool dact[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int hp = 16 * (wave + 4 * i) + prow;
            const int hr = hp / HPI, hc = hp - hr * HPI;
            const int iy = y0 + hr, ix = x0 + hc;
            const bool ok = (hp < HROWS) & ((unsigned)iy < (unsigned)a.H) & ((unsigned)ix < (unsigned)a.W);
            dbase[i] = ok ? ((img * a.H + iy) * a.W + ix) * C + kvlog * 8 : -1;
            dact[i] = hp < HROWS;
        }
        auto issue_piece = [&](int ks, unsigned stage_base, auto ic) {
            constexpr int I = decltype(ic)::value;
            if (dact[I]) {
#ifdef LT_BNECK_ABL_NODMA   /* timing only: every piece reads the zero page (L2 hit) */
                const void* src = zero_page;
#else
#ifdef LT_BNECK_ABL_SEG128
                const void* src = dbase[I] >= 0 ? (const void*)(x + (dbase[I] + (ks * 32 < C - 64 ? ks * 32 : C - 64))) : zero_page;
#else
                const void* src = dbase[I] >= 0 ? (const void*)(x + (dbase[I] + ks * 32)) : zero_page;
#endif
#endif
                dma16(src, lds0 + stage_base + (wave + 4 * I) * 1024);
            }
        };
        const int hb0 = NCB == 4 ? 0 : 3 * whalf;          // first halo pixel block of this wave
        const T* w1l = a.w1 + (size_t)cb * 512;            // fragment (g, cb): + g * NCB * 512 elements; lane offset in bytes below
        const unsigned wlane = lane * 16;
        // W1 fragments are requested DA K steps ahead: a fragment load is queued behind the ring pieces issued before it and loads return in
        // order, so at distance 1 every K step lasted as long as a ring piece's round trip to HBM (2.7k cycles per step whatever the ring depth)
        constexpr int DA = 3, NFA = DA + 1;
        static_assert(AHEAD > DA && NK1 >= DA, "W1 prefetch distance");
        V16 fa[NFA][2];
        auto loadA = [&](int ks, V16 (&dst)[2]) {
            const T* p = w1l + (size_t)(2 * ks) * NCB * 512;
            gload16(dst[0], p, wlane);
            gload16(dst[1], p + NCB * 512, wlane);
        };
        const unsigned fo0 = n31 * 64 + (((0 + hk) ^ swz64(n31)) << 4);
        const unsigned fo1 = n31 * 64 + (((2 + hk) ^ swz64(n31)) << 4);
        auto capture = [&](unsigned stage_base, uint4 (&dst)[NPB][2]) {
#pragma unroll
            for (int pb = 0; pb < NPB; ++pb) {
                const int hpc = (2 * pb + prr + 1) * HPI + pcc + 1;
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    dst[pb][j] = *(const uint4*)((lptr_t)(size_t)(lds0 + stage_base + hpc * 64 + (((2 * j + hk) ^ swz64(hpc)) << 4)));
            }
        };

        f32x16 acc[NPB1];
#pragma unroll
        for (int i = 0; i < NPB1; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;

        static_for<0, DA>([&](auto kc) { loadA(decltype(kc)::value, fa[decltype(kc)::value]); });
#pragma unroll
        for (int s = 0; s < AHEAD; ++s)
            static_for<0, 3>([&](auto ic) { issue_piece(s, s * STAGE, ic); });

        // fully unrolled: every K step's wait count, ring stage and fragment register set are compile-time (and every asm load's result is used:
        // hipcc may give the registers of a dead one to something live, and the data landing later overwrites it)
        static_for<0, NK1>([&](auto kc) {
            constexpr int ks = decltype(kc)::value, R = ks % NFA;
            constexpr unsigned rbuf = (ks % NST) * STAGE, wbuf = ((ks + AHEAD) % NST) * STAGE;
            wait_vmcnt<bneck_after<NK1, AHEAD, DA>(ks)>();    // A(ks) and this wave's pieces of stage ks
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            frag_ready(fa[R][0]);
            frag_ready(fa[R][1]);
            if constexpr (ks + DA < NK1) loadA(ks + DA, fa[(ks + DA) % NFA]);
            if constexpr (ks + AHEAD < NK1) static_for<0, 3>([&](auto ic) { issue_piece(ks + AHEAD, wbuf, ic); });
            if constexpr (NHELD > 0 && ks < 4) { if (ks == wave) capture(rbuf, held[0]); }
            if constexpr (NHELD > 1 && ks >= 4 && ks < 8) { if (ks == wave + 4) capture(rbuf, held[NHELD > 1 ? 1 : 0]); }
            const unsigned rb = lds0 + rbuf + hb0 * 2048;
            // all fragments of one K half are requested before its MFMAs, the second half's under the first half's MFMAs (left to itself
            // hipcc reads every fragment into the same four registers: ds_read -> lgkmcnt(0) -> MFMA, one LDS round trip per MFMA)
#ifndef LT_BNECK_ABL_NOMMA1   /* timing only: phase 1 without fragment reads and MFMAs */
            V16 b0[NPB1], b1[NPB1];
#pragma unroll
            for (int i = 0; i < NPB1; ++i) b0[i].u = *(const uint4*)((lptr_t)(size_t)(rb + fo0 + i * 2048));
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < NPB1; ++i) b1[i].u = *(const uint4*)((lptr_t)(size_t)(rb + fo1 + i * 2048));
#pragma unroll
            for (int i = 0; i < NPB1; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[R][0].h, b0[i].h, acc[i], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < NPB1; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[R][1].h, b1[i].h, acc[i], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
#else
            acc[0][0] += fa[R][0].f[0] + fa[R][1].f[0];
#endif
        });
        // the last stages of the ring lie in t1's bytes: every wave is done reading them before t1 is written
        asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        BN_STAMP(1);

        // epilogue: lane (pixel n31, h) holds channels 32 cb + 8 h + e (e < 8) and 32 cb + 16 + 8 h + (e - 8) of halo pixel 32 hb + n31
        float esc[16], esf[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            esc[e] = csel(cst12, 0, e);
            esf[e] = csel(cst12, 32, e);
        }
        if (a.bias[0]) {                                     // (acc + b) s + f == acc s + (b s + f) up to one rounding; ResNet has no bias
#pragma unroll
            for (int e = 0; e < 16; ++e) esf[e] = a.bias[0][32 * cb + 16 * (e >> 3) + 8 * hk + (e & 7)] * esc[e] + esf[e];
        }
#pragma unroll
        for (int i = 0; i < NPB1; ++i) {
            const int hp = 32 * (hb0 + i) + n31;
            const int hr = hp / HPI, hc = hp - hr * HPI;
            const int iy = y0 + hr, ix = x0 + hc;
            const bool inimg = ((unsigned)iy < (unsigned)a.H) & ((unsigned)ix < (unsigned)a.W);
            if (hp < HROWS) {
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    unsigned o[4];
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        const int e = 8 * q + 2 * d;
                        const float v0 = fmaxf(acc[i][e] * esc[e] + esf[e], 0.f), v1 = fmaxf(acc[i][e + 1] * esc[e + 1] + esf[e + 1], 0.f);
                        o[d] = inimg ? pack_bf16x2(v0, v1) : 0u;
                    }
                    const int slot = (4 * cb + 2 * q + hk) ^ fsw(hp);
                    *(uint4*)((lptr_t)(size_t)(lds0 + hp * RB + slot * 16)) = make_uint4(o[0], o[1], o[2], o[3]);
                }
            }
        }
    }
    __syncthreads();
    BN_STAMP(2);

    // ---- phase 3's operands that are requested early: W3 fragments one output-channel block (G2 units) ahead, and the residual of the
    // blocks that were not held one block ahead of its use (vector-memory loads return in order: a short-latency weight load queued behind a
    // long-latency residual load waits for it, so the distance between the two has to cover the residual's latency)
    constexpr int NU3 = NOBW * G2, WD3 = G2 < 6 ? G2 : 6;
    int poff[NPB];                                           // element offset of this lane's pixel in block pb, channel 8 h
#pragma unroll
    for (int pb = 0; pb < NPB; ++pb)
        poff[pb] = ((img * a.H + ty * TH + 2 * pb + prr) * a.W + tx * TW + pcc) * C + 8 * hk;
    const T* wl3 = a.w3 + (size_t)lane * 8;
    auto load_w3 = [&](int u) -> V16 {                       // unit u = q * G2 + g -> fragment (g, ob = wave + 4 q)
        const int q = u / G2, g = u - q * G2;
        V16 v;
        v.u = *(const uint4*)(wl3 + ((size_t)g * NOB + wave + 4 * q) * 512);
        return v;
    };
    V16 wf3[WD3 + 1];
    uint4 rq[2][NPB][2];
    auto load_res = [&](int q, uint4 (&dst)[NPB][2]) {
        const int ob = wave + 4 * q;
#pragma unroll
        for (int pb = 0; pb < NPB; ++pb)
#pragma unroll
            for (int j = 0; j < 2; ++j) dst[pb][j] = *(const uint4*)(x + poff[pb] + 32 * ob + 16 * j);
    };

    // ================================================ phase 2: t2 = relu(bn2(W2 * t1)) ================================================
    {
        const int pb0 = NCB == 4 ? 0 : 2 * whalf;
        const int bn = prr * HPI + pcc + 2 * HPI * pb0;      // halo pixel of tap (0, 0) of this lane's pixel in block pb0
        unsigned am[16];                                     // lane address for the tap-offset classes m = T & 15
#pragma unroll
        for (int m = 0; m < 16; ++m) am[m] = lds0 + bn * RB + ((hk ^ fsw(bn + m)) << 4);
        const T* wl = a.w2 + ((size_t)cb * 64 + lane) * 8;
        auto load_w = [&](int u) -> V16 {
            V16 v;
            v.u = *(const uint4*)(wl + (size_t)u * NCB * 512);
            return v;
        };
        constexpr int NU = 9 * G2, WD = 6;
        V16 wf[WD + 1];
#pragma unroll
        for (int u = 0; u < WD; ++u) wf[u] = load_w(u);
        f32x16 acc[NPB2];
#pragma unroll
        for (int i = 0; i < NPB2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
        V16 xa[2][NPB2];
        auto load_x = [&](auto uc, V16 (&dst)[NPB2]) {
            constexpr int u = decltype(uc)::value;
            constexpr int tap = u / G2, g = u % G2, dy = tap / 3, dx = tap % 3;
            static_for<0, NPB2>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                constexpr int TT = dy * HPI + dx + 2 * HPI * i;
                const unsigned ad = am[TT & 15] ^ (g << 5);
                dst[i].u = *(const uint4*)((lptr_t)(size_t)(ad + TT * RB));
            });
        };
        load_x(std::integral_constant<int, 0>{}, xa[0]);
        static_for<0, NU>([&](auto uc) {
            constexpr int u = decltype(uc)::value;
            if constexpr (u + WD < NU) wf[(u + WD) % (WD + 1)] = load_w(u + WD);
            if constexpr (u + 1 < NU) load_x(std::integral_constant<int, u + 1>{}, xa[(u + 1) & 1]);
#pragma unroll
            for (int i = 0; i < NPB2; ++i)
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[u % (WD + 1)].h, xa[u & 1][i].h, acc[i], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        });
        BN_STAMP(3);
        // phase 3's first requests go out here, in front of this phase's epilogue and the barrier: weights, then (younger) the residual
#pragma unroll
        for (int u = 0; u < WD3; ++u) wf3[u] = load_w3(u);
        if constexpr (NHELD < NOBW) load_res(NHELD, rq[0]);
        __builtin_amdgcn_sched_barrier(0);

        float esc[16], esf[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            esc[e] = csel(cst12, 64, e);
            esf[e] = csel(cst12, 96, e);
        }
        if (a.bias[1]) {
#pragma unroll
            for (int e = 0; e < 16; ++e) esf[e] = a.bias[1][32 * cb + 16 * (e >> 3) + 8 * hk + (e & 7)] * esc[e] + esf[e];
        }
#pragma unroll
        for (int i = 0; i < NPB2; ++i) {
            const int px = 32 * (pb0 + i) + n31;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                unsigned o[4];
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const int e = 8 * q + 2 * d;
                    o[d] = pack_bf16x2(fmaxf(acc[i][e] * esc[e] + esf[e], 0.f), fmaxf(acc[i][e + 1] * esc[e + 1] + esf[e + 1], 0.f));
                }
                const int slot = (4 * cb + 2 * q + hk) ^ fsw(n31);
                *(uint4*)((lptr_t)(size_t)(lds0 + T2_OFF + px * RB + slot * 16)) = make_uint4(o[0], o[1], o[2], o[3]);
            }
        }
    }
    __syncthreads();
    BN_STAMP(4);

    // ================================================ phase 3: y = relu(bn3(W3 t2) + x) ==============================================
    {
        const unsigned a2 = lds0 + T2_OFF + n31 * RB + ((hk ^ fsw(n31)) << 4);   // K block g: ^ (g << 5), pixel block pb: + pb * 32 * RB
        f32x16 acc[NPB];
        static_for<0, NU3>([&](auto uc) {
            constexpr int u = decltype(uc)::value;
            constexpr int q = u / G2, g = u % G2;
            const int ob = wave + 4 * q;
            if constexpr (g == 0) {
#pragma unroll
                for (int pb = 0; pb < NPB; ++pb)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[pb][e] = 0.f;
            }
            // the residual of the NEXT block (the first one that is read again went out in front of phase 2's epilogue), placed so that every
            // weight fragment this block still needs is older than it: the fragments requested from here on belong to the next block
            if constexpr (g == G2 - WD3 && q + 1 < NOBW && q + 1 > NHELD) load_res(q + 1, rq[(q + 1 - NHELD) & 1]);
            if constexpr (u + WD3 < NU3) wf3[(u + WD3) % (WD3 + 1)] = load_w3(u + WD3);
            V16 xb[NPB];
#pragma unroll
            for (int pb = 0; pb < NPB; ++pb) xb[pb].u = *(const uint4*)((lptr_t)(size_t)((a2 ^ (g << 5)) + pb * 32 * RB));
#pragma unroll
            for (int pb = 0; pb < NPB; ++pb)
                acc[pb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf3[u % (WD3 + 1)].h, xb[pb].h, acc[pb], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (g == G2 - 1) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {                // one 8-channel run at a time: 16 constants live instead of 32
                    float esc[8], esf[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        esc[e] = csel(cst3, 64 * q, 8 * j + e);
                        esf[e] = csel(cst3, 64 * q + 32, 8 * j + e);
                    }
                    if (a.bias[2]) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) esf[e] = a.bias[2][32 * ob + 16 * j + 8 * hk + e] * esc[e] + esf[e];
                    }
#pragma unroll
                    for (int pb = 0; pb < NPB; ++pb) {
                        uint4 rv;
                        if constexpr (q < NHELD) rv = held[q < NHELD ? q : 0][pb][j];
                        else rv = rq[(q - NHELD) & 1][pb][j];
                        const unsigned rr[4] = {rv.x, rv.y, rv.z, rv.w};
                        unsigned o[4];
#pragma unroll
                        for (int d = 0; d < 4; ++d) {
                            const int e = 2 * d;
                            const float v0 = fmaxf(acc[pb][8 * j + e] * esc[e] + esf[e] + __uint_as_float(rr[d] << 16), 0.f);
                            const float v1 = fmaxf(acc[pb][8 * j + e + 1] * esc[e + 1] + esf[e + 1] + __uint_as_float(rr[d] & 0xffff0000u), 0.f);
                            o[d] = pack_bf16x2(v0, v1);
                        }
                        *(uint4*)(a.y + poff[pb] + 32 * ob + 16 * j) = make_uint4(o[0], o[1], o[2], o[3]);
                    }
                }
            }
        });
    }
    BN_STAMP(5);
}

template <int C, int P, int NSTR, int NHELD>
int launch_bneck(const BneckArgs& a, hipStream_t s) {
    constexpr int RB = 2 * P;
    constexpr int lds = 180 * RB + (NSTR - 1) * 180 * 64 + 192 * 64;
    static_assert(lds <= 80 * 1024, "two workgroups per CU");
    auto kern = bneck_kernel<C, P, NSTR, NHELD>;
    LT_OPT_IN_LDS(kern, lds);
    const long long nblk = (long long)a.N * a.tiles_x * a.tiles_y;
    hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(256), lds, s, a);
    LT_CHECK_LAUNCH("lt_bottleneck_fwd");
    return LT_OK;
}


// ---- the FIRST Bottleneck of ResNet layer1 in one launch: 64 -> 64 -> 64 -> 256 with the 1x1 64 -> 256 downsample branch, stride 1 ----------------
// (reference pose_resnet.py:75-95 with `downsample` = conv1x1 + bn, :196-206).  Same tile, same three phases as bneck_kernel; what differs:
//   * x has 64 channels: its 10 x 18 halo is TWO 32-channel stages (23 KB) that stay in LDS for the whole kernel (no ring) -- phase 1 reads them as
//     the reduce's operand, phase 3 reads the 128 centre pixels again as the operand of the downsample GEMM (K = 64);
//   * the residual is not read from memory but computed: y = relu(bn3(W3 t2) + bnd(Wd x)), two accumulator sets per output block (the two branches
//     have their own BatchNorm scale), combined in fp32 -- the separate launches round the downsample branch to bf16 before the add;
//   * t1 has its own bytes, so phase 1's epilogue needs no barrier in front of it.
// The four launches it replaces move 64 (x) + 256 + 64 + 64 + 64 + 64 + 256 (residual) + 256 channel-units per pixel, this one 64 + 256.
struct BneckDsArgs {
    const bf16_t* x;
    bf16_t* y;
    const bf16_t* w1;
    const bf16_t* w2;
    const bf16_t* w3;
    const bf16_t* wd;
    const float* scale[4];   // conv1, conv2, conv3, downsample
    const float* shift[4];
    int N, H, W, tiles_x, tiles_y;
};

template <int CIN, int P, int C>
__global__ __launch_bounds__(256, 2) void bneck_ds_kernel(const BneckDsArgs a) {
    typedef bf16_t T;
    constexpr int TH = 8, TW = 16, HPI = TW + 2, HROWS = (TH + 2) * HPI;
    constexpr int NPB = 4;
    constexpr int NCB = P / 32, NOB = C / 32, G2 = P / 16, GD = CIN / 16, NK1 = CIN / 32;
    constexpr int RB = 2 * P, NSL = P / 8;
    constexpr int T1_BYTES = HROWS * RB, STAGE = HROWS * 64;
    constexpr int XS_OFF = T1_BYTES, T2_OFF = XS_OFF + NK1 * STAGE;
    constexpr int NPB1 = 3, NPB2 = 2, NOBW = NOB / 4;
    static_assert(CIN == 64 && P == 64 && C == 256, "the first block of ResNet layer1");
    static_assert(NCB == 2 && NSL == 8 && NOBW == 2, "wave roles below");
    static_assert(XS_OFF % 256 == 0 && T2_OFF % 256 == 0, "the XOR / bank arguments assume 256-byte aligned regions");
    auto fsw = [](int hp) -> int { return (hp >> 1) & 7; };

    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
    const unsigned lds0 = (unsigned)(size_t)(lptr_t)smem;
    unsigned long long zp_bits = (unsigned long long)(size_t)g_zero_page_b;
    asm volatile("" : "+s"(zp_bits));
    const void* const zero_page = (const void*)(size_t)zp_bits;

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    int lin = blockIdx.x;
    {
        const int nb = gridDim.x, q = nb >> 3, r = nb & 7, xcd = lin & 7, j = lin >> 3;
        lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
    }
    const int tpi = a.tiles_x * a.tiles_y;
    const int img = lin / tpi, rem = lin - img * tpi;
    const int ty = rem / a.tiles_x, tx = rem - ty * a.tiles_x;
    const int y0 = ty * TH - 1, x0 = tx * TW - 1;
    const T* __restrict__ x = a.x;

    const int n31 = lane & 31, hk = lane >> 5;
    const int cb = wave & 1, whalf = wave >> 1;
    const int prr = n31 >> 4, pcc = ((n31 & 15) - 2 * prr) & 15;

    // folded BatchNorm constants in 8 registers (see bneck_kernel): cst12 = [scale1 | shift1 | scale2 | shift2][32 channels of block cb],
    // cst3 = [q][scale3 | shift3 | scale_d | shift_d][32 channels of block wave + 4 q] = 256 floats = one float4 per lane
    float4 cst12, cst3;
    {
        const int l = lane & 31, arr = l >> 3, i4 = l & 7;
        const float* t12 = arr == 0 ? a.scale[0] : arr == 1 ? a.shift[0] : arr == 2 ? a.scale[1] : a.shift[1];
        cst12 = *(const float4*)(t12 + 32 * cb + 4 * i4);
        const int f = 4 * lane, q = f >> 7, which = (f >> 5) & 3, c = f & 31;
        const float* t3 = which == 0 ? a.scale[2] : which == 1 ? a.shift[2] : which == 2 ? a.scale[3] : a.shift[3];
        cst3 = *(const float4*)(t3 + 32 * (wave + 4 * q) + c);
    }
    auto cget = [&](const float4& tb, int f) -> float {
        const float v = (f & 3) == 0 ? tb.x : (f & 3) == 1 ? tb.y : (f & 3) == 2 ? tb.z : tb.w;
        return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), f >> 2));
    };
    auto csel = [&](const float4& tb, int base, int e) -> float {
        const float lo = cget(tb, base + 16 * (e >> 3) + (e & 7)), hi = cget(tb, base + 16 * (e >> 3) + 8 + (e & 7));
        return hk ? hi : lo;
    };

    // ================================================ phase 1: t1 = relu(bn1(W1 x)) on the halo =======================================
    {
        const int prow = lane >> 2;
        const int kvlog = (lane & 3) ^ swz64(prow);
        const T* w1l = a.w1 + (size_t)cb * 512;
        const unsigned wlane = lane * 16;
        V16 fa[NK1][2];
#pragma unroll
        for (int ks = 0; ks < NK1; ++ks) {
            const T* p = w1l + (size_t)(2 * ks) * NCB * 512;
            gload16(fa[ks][0], p, wlane);
            gload16(fa[ks][1], p + NCB * 512, wlane);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int hp = 16 * (wave + 4 * i) + prow;
            const int hr = hp / HPI, hc = hp - hr * HPI;
            const int iy = y0 + hr, ix = x0 + hc;
            const bool ok = (hp < HROWS) & ((unsigned)iy < (unsigned)a.H) & ((unsigned)ix < (unsigned)a.W);
            const int dbase = ok ? ((img * a.H + iy) * a.W + ix) * CIN + kvlog * 8 : -1;
            if (hp < HROWS) {
#pragma unroll
                for (int ks = 0; ks < NK1; ++ks) {
                    const void* src = dbase >= 0 ? (const void*)(x + (dbase + ks * 32)) : zero_page;
                    dma16(src, lds0 + XS_OFF + ks * STAGE + (wave + 4 * i) * 1024);
                }
            }
        }
        const int hb0 = 3 * whalf;
        const unsigned fo0 = n31 * 64 + (((0 + hk) ^ swz64(n31)) << 4);
        const unsigned fo1 = n31 * 64 + (((2 + hk) ^ swz64(n31)) << 4);
        f32x16 acc[NPB1];
#pragma unroll
        for (int i = 0; i < NPB1; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
        asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // both stages of x (all four waves' pieces), W1, the constants
#pragma unroll
        for (int ks = 0; ks < NK1; ++ks) {
            frag_ready(fa[ks][0]);
            frag_ready(fa[ks][1]);
            const unsigned rb = lds0 + XS_OFF + ks * STAGE + hb0 * 2048;
            V16 b0[NPB1], b1[NPB1];
#pragma unroll
            for (int i = 0; i < NPB1; ++i) b0[i].u = *(const uint4*)((lptr_t)(size_t)(rb + fo0 + i * 2048));
#pragma unroll
            for (int i = 0; i < NPB1; ++i) b1[i].u = *(const uint4*)((lptr_t)(size_t)(rb + fo1 + i * 2048));
#pragma unroll
            for (int i = 0; i < NPB1; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][0].h, b0[i].h, acc[i], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < NPB1; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][1].h, b1[i].h, acc[i], 0, 0, 0);
        }
        float esc[16], esf[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            esc[e] = csel(cst12, 0, e);
            esf[e] = csel(cst12, 32, e);
        }
#pragma unroll
        for (int i = 0; i < NPB1; ++i) {
            const int hp = 32 * (hb0 + i) + n31;
            const int hr = hp / HPI, hc = hp - hr * HPI;
            const int iy = y0 + hr, ix = x0 + hc;
            const bool inimg = ((unsigned)iy < (unsigned)a.H) & ((unsigned)ix < (unsigned)a.W);
            if (hp < HROWS) {
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    unsigned o[4];
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        const int e = 8 * q + 2 * d;
                        const float v0 = fmaxf(acc[i][e] * esc[e] + esf[e], 0.f), v1 = fmaxf(acc[i][e + 1] * esc[e + 1] + esf[e + 1], 0.f);
                        o[d] = inimg ? pack_bf16x2(v0, v1) : 0u;
                    }
                    const int slot = (4 * cb + 2 * q + hk) ^ fsw(hp);
                    *(uint4*)((lptr_t)(size_t)(lds0 + hp * RB + slot * 16)) = make_uint4(o[0], o[1], o[2], o[3]);
                }
            }
        }
    }
    __syncthreads();

    // phase 3's weight stream: per output block q (ob = wave + 4 q) GD units of the downsample (K blocks of x) and then G2 units of the expand
    constexpr int NUQ = GD + G2, NU3 = NOBW * NUQ, WD3 = 6;
    int poff[NPB];
#pragma unroll
    for (int pb = 0; pb < NPB; ++pb)
        poff[pb] = ((img * a.H + ty * TH + 2 * pb + prr) * a.W + tx * TW + pcc) * C + 8 * hk;
    const T* wl3 = a.w3 + (size_t)lane * 8;
    const T* wld = a.wd + (size_t)lane * 8;
    auto load_w3 = [&](int u) -> V16 {
        const int q = u / NUQ, k = u - q * NUQ;
        V16 v;
        if (k < GD) v.u = *(const uint4*)(wld + ((size_t)k * NOB + wave + 4 * q) * 512);
        else v.u = *(const uint4*)(wl3 + ((size_t)(k - GD) * NOB + wave + 4 * q) * 512);
        return v;
    };
    V16 wf3[WD3 + 1];

    // ================================================ phase 2: t2 = relu(bn2(W2 * t1)) ================================================
    {
        const int pb0 = 2 * whalf;
        const int bn = prr * HPI + pcc + 2 * HPI * pb0;
        unsigned am[16];
#pragma unroll
        for (int m = 0; m < 16; ++m) am[m] = lds0 + bn * RB + ((hk ^ fsw(bn + m)) << 4);
        const T* wl = a.w2 + ((size_t)cb * 64 + lane) * 8;
        auto load_w = [&](int u) -> V16 {
            V16 v;
            v.u = *(const uint4*)(wl + (size_t)u * NCB * 512);
            return v;
        };
        constexpr int NU = 9 * G2, WD = 6;
        V16 wf[WD + 1];
#pragma unroll
        for (int u = 0; u < WD; ++u) wf[u] = load_w(u);
        f32x16 acc[NPB2];
#pragma unroll
        for (int i = 0; i < NPB2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
        V16 xa[2][NPB2];
        auto load_x = [&](auto uc, V16 (&dst)[NPB2]) {
            constexpr int u = decltype(uc)::value;
            constexpr int tap = u / G2, g = u % G2, dy = tap / 3, dx = tap % 3;
            static_for<0, NPB2>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                constexpr int TT = dy * HPI + dx + 2 * HPI * i;
                const unsigned ad = am[TT & 15] ^ (g << 5);
                dst[i].u = *(const uint4*)((lptr_t)(size_t)(ad + TT * RB));
            });
        };
        load_x(std::integral_constant<int, 0>{}, xa[0]);
        static_for<0, NU>([&](auto uc) {
            constexpr int u = decltype(uc)::value;
            if constexpr (u + WD < NU) wf[(u + WD) % (WD + 1)] = load_w(u + WD);
            if constexpr (u + 1 < NU) load_x(std::integral_constant<int, u + 1>{}, xa[(u + 1) & 1]);
#pragma unroll
            for (int i = 0; i < NPB2; ++i)
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[u % (WD + 1)].h, xa[u & 1][i].h, acc[i], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        });
#pragma unroll
        for (int u = 0; u < WD3; ++u) wf3[u] = load_w3(u);
        __builtin_amdgcn_sched_barrier(0);

        float esc[16], esf[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            esc[e] = csel(cst12, 64, e);
            esf[e] = csel(cst12, 96, e);
        }
#pragma unroll
        for (int i = 0; i < NPB2; ++i) {
            const int px = 32 * (pb0 + i) + n31;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                unsigned o[4];
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const int e = 8 * q + 2 * d;
                    o[d] = pack_bf16x2(fmaxf(acc[i][e] * esc[e] + esf[e], 0.f), fmaxf(acc[i][e + 1] * esc[e + 1] + esf[e + 1], 0.f));
                }
                const int slot = (4 * cb + 2 * q + hk) ^ fsw(n31);
                *(uint4*)((lptr_t)(size_t)(lds0 + T2_OFF + px * RB + slot * 16)) = make_uint4(o[0], o[1], o[2], o[3]);
            }
        }
    }
    __syncthreads();

    // ================================================ phase 3: y = relu(bn3(W3 t2) + bnd(Wd x)) =======================================
    {
        const unsigned a2 = lds0 + T2_OFF + n31 * RB + ((hk ^ fsw(n31)) << 4);
        unsigned xd[NPB][2];                                  // this lane's centre pixel of block pb in a stage of x: 16-byte slot 2 s + h, s = K block & 1
#pragma unroll
        for (int pb = 0; pb < NPB; ++pb) {
            const int hpc = (2 * pb + prr + 1) * HPI + pcc + 1;
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) xd[pb][s2] = lds0 + XS_OFF + hpc * 64 + (((2 * s2 + hk) ^ swz64(hpc)) << 4);
        }
        f32x16 acc[NPB], accd[NPB];
        static_for<0, NU3>([&](auto uc) {
            constexpr int u = decltype(uc)::value;
            constexpr int q = u / NUQ, k = u % NUQ;
            const int ob = wave + 4 * q;
            if constexpr (k == 0) {
#pragma unroll
                for (int pb = 0; pb < NPB; ++pb)
#pragma unroll
                    for (int e = 0; e < 16; ++e) { acc[pb][e] = 0.f; accd[pb][e] = 0.f; }
            }
            if constexpr (u + WD3 < NU3) wf3[(u + WD3) % (WD3 + 1)] = load_w3(u + WD3);
            V16 xb[NPB];
            if constexpr (k < GD) {
#pragma unroll
                for (int pb = 0; pb < NPB; ++pb) xb[pb].u = *(const uint4*)((lptr_t)(size_t)(xd[pb][k & 1] + (k >> 1) * STAGE));
#pragma unroll
                for (int pb = 0; pb < NPB; ++pb)
                    accd[pb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf3[u % (WD3 + 1)].h, xb[pb].h, accd[pb], 0, 0, 0);
            } else {
                constexpr int g = k - GD;
#pragma unroll
                for (int pb = 0; pb < NPB; ++pb) xb[pb].u = *(const uint4*)((lptr_t)(size_t)((a2 ^ (g << 5)) + pb * 32 * RB));
#pragma unroll
                for (int pb = 0; pb < NPB; ++pb)
                    acc[pb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf3[u % (WD3 + 1)].h, xb[pb].h, acc[pb], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (k == NUQ - 1) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    float esc[8], esf[8], dsc[8], dsf[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        esc[e] = csel(cst3, 128 * q, 8 * j + e);
                        esf[e] = csel(cst3, 128 * q + 32, 8 * j + e);
                        dsc[e] = csel(cst3, 128 * q + 64, 8 * j + e);
                        dsf[e] = csel(cst3, 128 * q + 96, 8 * j + e);
                    }
#pragma unroll
                    for (int pb = 0; pb < NPB; ++pb) {
                        unsigned o[4];
#pragma unroll
                        for (int d = 0; d < 4; ++d) {
                            const int e = 2 * d;
                            const float r0 = accd[pb][8 * j + e] * dsc[e] + dsf[e], r1 = accd[pb][8 * j + e + 1] * dsc[e + 1] + dsf[e + 1];
                            const float v0 = fmaxf(acc[pb][8 * j + e] * esc[e] + esf[e] + r0, 0.f);
                            const float v1 = fmaxf(acc[pb][8 * j + e + 1] * esc[e + 1] + esf[e + 1] + r1, 0.f);
                            o[d] = pack_bf16x2(v0, v1);
                        }
                        *(uint4*)(a.y + poff[pb] + 32 * ob + 16 * j) = make_uint4(o[0], o[1], o[2], o[3]);
                    }
                }
            }
        });
    }
}

int launch_bneck_ds(const BneckDsArgs& a, hipStream_t s) {
    constexpr int lds = 180 * 128 + 2 * 180 * 64 + 128 * 128;   // t1 + the two stages of x + t2 = 62464 B
    static_assert(lds <= 80 * 1024, "two workgroups per CU");
    auto kern = bneck_ds_kernel<64, 64, 256>;
    LT_OPT_IN_LDS(kern, lds);
    const long long nblk = (long long)a.N * a.tiles_x * a.tiles_y;
    hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(256), lds, s, a);
    LT_CHECK_LAUNCH("lt_bottleneck_ds_fwd");
    return LT_OK;
}

}  // namespace

#ifdef LT_BNECK_TRACE
extern "C" int lt_bneck_trace_read(void* host, int nbytes) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_bneck_trace), nbytes, 0, hipMemcpyDeviceToHost);
}
#endif

extern "C" int lt_bottleneck_fwd(const lt_bneck_desc* d, const void* x, void* y, void* stream) {
    LT_REQUIRE(d && x && y, LT_ERR_INVALID, "lt_bottleneck_fwd: null argument");
    LT_REQUIRE(x != y, LT_ERR_INVALID, "lt_bottleneck_fwd: in-place is not possible (neighbouring tiles read each other's halo)");
    LT_REQUIRE(d->dtype == LT_BF16, LT_ERR_UNSUPPORTED, "lt_bottleneck_fwd: bf16 only");
    LT_REQUIRE((d->C == 256 && d->P == 64) || (d->C == 512 && d->P == 128), LT_ERR_UNSUPPORTED,
               "lt_bottleneck_fwd: widths %d / %d (256 / 64 and 512 / 128: the identity blocks of ResNet layer1 / layer2)", d->C, d->P);
    LT_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->H % 8 == 0 && d->W % 16 == 0, LT_ERR_UNSUPPORTED,
               "lt_bottleneck_fwd: map %d x %d (8 x 16 pixel tiles)", d->H, d->W);
    LT_REQUIRE((long long)d->N * d->H * d->W * d->C < (1ll << 31), LT_ERR_UNSUPPORTED, "lt_bottleneck_fwd: 32-bit element offsets");
    BneckArgs a;
    a.x = (const bf16_t*)x;
    a.y = (bf16_t*)y;
    a.w1 = (const bf16_t*)d->weight[0];
    a.w2 = (const bf16_t*)d->weight[1];
    a.w3 = (const bf16_t*)d->weight[2];
    for (int i = 0; i < 3; ++i) {
        LT_REQUIRE(d->weight[i] && d->scale[i] && d->shift[i], LT_ERR_INVALID, "lt_bottleneck_fwd: layer %d: null weight / scale / shift", i);
        a.bias[i] = d->bias[i];
        a.scale[i] = d->scale[i];
        a.shift[i] = d->shift[i];
    }
    a.N = d->N; a.H = d->H; a.W = d->W;
    a.tiles_x = d->W / 16; a.tiles_y = d->H / 8;
    hipStream_t s = (hipStream_t)stream;
#ifndef LT_BNECK_HELD64
#define LT_BNECK_HELD64 2
#endif
#ifndef LT_BNECK_HELD128
#define LT_BNECK_HELD128 1
#endif
    if (d->P == 64) return launch_bneck<256, 64, 4, LT_BNECK_HELD64>(a, s);
    return launch_bneck<512, 128, 3, LT_BNECK_HELD128>(a, s);
}

extern "C" int lt_bottleneck_ds_fwd(const lt_bneck_ds_desc* d, const void* x, void* y, void* stream) {
    LT_REQUIRE(d && x && y, LT_ERR_INVALID, "lt_bottleneck_ds_fwd: null argument");
    LT_REQUIRE(x != y, LT_ERR_INVALID, "lt_bottleneck_ds_fwd: in-place is not possible");
    LT_REQUIRE(d->dtype == LT_BF16, LT_ERR_UNSUPPORTED, "lt_bottleneck_ds_fwd: bf16 only");
    LT_REQUIRE(d->Cin == 64 && d->P == 64 && d->C == 256, LT_ERR_UNSUPPORTED,
               "lt_bottleneck_ds_fwd: widths %d -> %d -> %d (64 -> 64 -> 256: the first block of ResNet layer1)", d->Cin, d->P, d->C);
    LT_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->H % 8 == 0 && d->W % 16 == 0, LT_ERR_UNSUPPORTED,
               "lt_bottleneck_ds_fwd: map %d x %d (8 x 16 pixel tiles)", d->H, d->W);
    LT_REQUIRE((long long)d->N * d->H * d->W * d->C < (1ll << 31), LT_ERR_UNSUPPORTED, "lt_bottleneck_ds_fwd: 32-bit element offsets");
    BneckDsArgs a;
    a.x = (const bf16_t*)x;
    a.y = (bf16_t*)y;
    for (int i = 0; i < 4; ++i) {
        LT_REQUIRE(d->weight[i] && d->scale[i] && d->shift[i], LT_ERR_INVALID, "lt_bottleneck_ds_fwd: layer %d: null weight / scale / shift", i);
        a.scale[i] = d->scale[i];
        a.shift[i] = d->shift[i];
    }
    a.w1 = (const bf16_t*)d->weight[0];
    a.w2 = (const bf16_t*)d->weight[1];
    a.w3 = (const bf16_t*)d->weight[2];
    a.wd = (const bf16_t*)d->weight[3];
    a.N = d->N; a.H = d->H; a.W = d->W;
    a.tiles_x = d->W / 16; a.tiles_y = d->H / 8;
    return launch_bneck_ds(a, (hipStream_t)stream);
}
