// Plan-level entry points of the C ABI ("whole-network plan entry points that own pre-packed weights and a hipGraph"):
//   lt_plan_create_vol / lt_plan_forward_vol          VolumetricTriangulationNet
//   lt_plan_create_alg / lt_plan_forward_alg          AlgebraicTriangulationNet (LT_MODEL_ALG) and RANSACTriangulationNet (LT_MODEL_RANSAC)
//   lt_plan_create_cascade / lt_plan_forward_cascade  the algebraic plan's pelvis -> the volumetric plan's cuboid, on the device (CascadeTriangulationNet)
//   lt_plan_info / lt_plan_destroy                    any plan
// A non-Python host hands over the reference's state_dict (names + host fp32 arrays) and the model configuration once, and then calls the forward with
// device images and host camera parameters: layer -> kernel selection, every batch threshold, the eval-BatchNorm fold, weight packing (GEMM layout,
// MFMA fragment orders, parity phases of the transposed convolutions, split-K tap groups), buffer reuse and the captured hipGraph all live behind this
// file -- the same recording lt_engine.py / mvn/models/*.py do when the Python modules record their plan, by the same kernel-selection rules (lt_sel_*,
// select.hip: both hosts call them); tests/test_gpu_plan_abi.py holds the two against each other and against the reference's golden outputs.
//
// What it replaces in the reference (file:line): VolumetricTriangulationNet.__init__ / forward (mvn/models/triangulation.py:204-355),
// AlgebraicTriangulationNet (:131-200) and RANSACTriangulationNet (:17-128) in eval mode, PoseResNet (mvn/models/pose_resnet.py:57-318: Bottleneck /
// BasicBlock / Bottleneck_CAFFE, _make_layer, _make_deconv_layer, final_layer, GlobalAveragePoolingHead), V2VModel (mvn/models/v2v.py:7-180),
// Camera.update_after_resize / projection (mvn/utils/multiview.py:33-52), the cuboid of triangulation.py:281-341.  All three models record their backbone
// through the one record_backbone below.
//
// Host-only code (no kernel here): every launch goes through the kernel-level entry points of include/lt_hip.h.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <array>
#include <deque>
#include <functional>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "lt_common.h"

using namespace lt;

namespace {

#define PL_TRY(call)                   \
    do {                               \
        const int rc_ = (call);        \
        if (rc_ != LT_OK) return rc_;  \
    } while (0)
#define PL_HIP(call)                                                        \
    do {                                                                    \
        hipError_t e_ = (call);                                             \
        if (e_ != hipSuccess) {                                             \
            set_error("%s failed: %s", #call, hipGetErrorString(e_));       \
            return LT_ERR_LAUNCH;                                           \
        }                                                                   \
    } while (0)

constexpr float BN_EPS = 1e-5f;
constexpr int GEO_RING = 4;          // slots of a StagingRing: forwards the host may run ahead of the GPU
constexpr int MODEL_CASCADE = 3;          // lt_plan::model of a cascade plan (not a value of lt_alg_plan_config.model)

// The one staging ring of the plans: GEO_RING pinned host blocks behind asynchronous H2D copies.  acquire() advances to the next slot, waits for the event
// recorded behind that slot's last copy (GEO_RING uses ago) and hands out its block; the caller fills it, enqueues its copy and calls commit(), which records
// the slot's event behind it -- this order is what keeps forward i+1's bytes out of forward i's queued copy.  Events are created at a slot's first commit:
// the first GEO_RING uses never wait.  Owns its blocks and events.
struct StagingRing {
    void* host[GEO_RING] = {nullptr, nullptr, nullptr, nullptr}; hipEvent_t ev[GEO_RING] = {nullptr, nullptr, nullptr, nullptr};
    int slot = 0;
    StagingRing() = default;
    StagingRing(const StagingRing&) = delete;
    StagingRing& operator=(const StagingRing&) = delete;
    ~StagingRing() {
        for (int i = 0; i < GEO_RING; ++i) { if (host[i]) (void)hipHostFree(host[i]); if (ev[i]) (void)hipEventDestroy(ev[i]); }
    }
    // the blocks that are not there yet, zeroed (a retry after a failure keeps what it has)
    int alloc(size_t bytes) {
        for (int i = 0; i < GEO_RING; ++i)
            if (!host[i]) { PL_HIP(hipHostMalloc(&host[i], bytes, hipHostMallocDefault)); memset(host[i], 0, bytes); }
        return LT_OK;
    }
    int acquire(void** block) {
        slot = (slot + 1) % GEO_RING;
        if (ev[slot]) PL_HIP(hipEventSynchronize(ev[slot]));          // the copy that last read this slot has completed
        *block = host[slot];
        return LT_OK;
    }
    int commit(hipStream_t st) {
        if (!ev[slot]) PL_HIP(hipEventCreateWithFlags(&ev[slot], hipEventDisableTiming));
        PL_HIP(hipEventRecord(ev[slot], st));
        return LT_OK;
    }
    void swap(StagingRing& o) {
        for (int i = 0; i < GEO_RING; ++i) { std::swap(host[i], o.host[i]); std::swap(ev[i], o.ev[i]); }
        std::swap(slot, o.slot);
    }
};

unsigned short bf16_rne(float f) {          // torch's float -> bfloat16 (round to nearest even, NaN kept quiet)
    unsigned u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}

int cout_pad_of(int cout) { return cout <= 16 ? 16 : cout <= 32 ? 32 : cout <= 64 ? 64 : (cout + 127) / 128 * 128; }

// ---- host views of the caller's tensors --------------------------------------------------------------------------------------------
struct WT {                                   // a weight tensor of the state dict, or a host-made one (own)
    const float* d = nullptr;
    int nd = 0;
    int64_t s[5] = {0, 0, 0, 0, 0};
    std::vector<float> own;
    int64_t numel() const { int64_t n = 1; for (int i = 0; i < nd; ++i) n *= s[i]; return n; }
};
struct BN { const float* g = nullptr; const float* b = nullptr; const float* m = nullptr; const float* v = nullptr; };

// a channels-last activation on the device: [n][d][h][w][c], element size es
struct Act {
    char* p = nullptr;
    int n = 0, d = 0, h = 0, w = 0, c = 0, es = 0;
    bool pooled = true, planar = false;
    size_t bytes() const { return (size_t)n * d * h * w * c * es; }
    long long numel() const { return (long long)n * d * h * w * c; }
    bool null() const { return p == nullptr; }
};

// the selection rules' (select.hip) view of shapes
lt_wshape wshape(const WT& w) {
    lt_wshape r = {};
    r.nd = w.nd;
    for (int i = 0; i < 5; ++i) r.s[i] = w.s[i];
    return r;
}
std::array<int32_t, 5> dims(const Act& a) { return {a.n, a.d, a.h, a.w, a.c}; }

struct PhaseSpec { std::vector<float> w; std::vector<int32_t> taps; int ntaps = 0; int off[3] = {0, 0, 0}; };
struct ConvSpec {
    int N, D, H, W, Cin, Do, Ho, Wo, st[3], pd[3], OD, OH, OW, ostr[3], Cout, cout_pad, k_pad, flags;
    std::vector<float> bias, scale, shift;
    std::vector<PhaseSpec> ph;
};

// Epilogue constants of y = (acc + bias) * scale + shift: eval-mode BatchNorm folded exactly the way ATen evaluates it (fp32: invstd = 1 / sqrt(var + eps),
// scale = invstd * weight, shift = bias_bn - mean * scale) -- lt_engine.fold_bn.  (The library is built with -ffp-contract=off: every step rounds like torch's.)
void fold_bn(int cout, const float* bias, const BN* bn, int cp, std::vector<float>& bi, std::vector<float>& sc, std::vector<float>& sh) {
    bi.assign(cp, 0.f); sc.assign(cp, 1.f); sh.assign(cp, 0.f);
    if (bias) for (int i = 0; i < cout; ++i) bi[i] = bias[i];
    if (bn)
        for (int i = 0; i < cout; ++i) {
            const float ve = bn->v[i] + BN_EPS;
            const float invstd = 1.0f / sqrtf(ve);
            const float alpha = invstd * bn->g[i];
            const float ma = bn->m[i] * alpha;
            sc[i] = alpha;
            sh[i] = bn->b[i] - ma;
        }
}

int floordiv(int a, int b) { int q = a / b, r = a % b; return (r != 0 && ((r < 0) != (b < 0))) ? q - 1 : q; }
int floormod(int a, int b) { return a - floordiv(a, b) * b; }

// lt_engine.make_conv_spec: the lt_conv_fwd description of one (transposed) convolution layer.  w: Conv{2,3}d [Cout][Cin][k..] or ConvTranspose{2,3}d
// [Cin][Cout][k..] (stride 2 only); in: (N, D, H, W, Cin_buffer) of the channels-last input (Cin_buffer >= Cin: extra input channels get zero weights).
int make_conv_spec(const WT& w, const float* bias, const BN* bn, const int in[5], int stride, int pad, int es, bool transposed, int flags, int output_padding, ConvSpec& sp) {
    const bool nd3 = w.nd == 5;
    LT_REQUIRE(w.nd == 4 || w.nd == 5, LT_ERR_INVALID, "plan: convolution weight with %d dimensions", w.nd);
    const int kd = nd3 ? (int)w.s[2] : 1, kh = (int)w.s[nd3 ? 3 : 2], kw = (int)w.s[nd3 ? 4 : 3];
    const int N = in[0], D = in[1], Hh = in[2], W = in[3], cin_buf = in[4];
    int st[3] = {stride, stride, stride}, pd[3] = {pad, pad, pad};
    if (!nd3) { st[0] = 1; pd[0] = 0; }
    const int kstep = 128 / es;
    sp.N = N; sp.D = D; sp.H = Hh; sp.W = W; sp.flags = flags;
    if (!transposed) {
        const int cout = (int)w.s[0], cin = (int)w.s[1];
        LT_REQUIRE(cin <= cin_buf, LT_ERR_INVALID, "plan: weight has %d input channels, the activation %d", cin, cin_buf);
        const int Do = (D + 2 * pd[0] - kd) / st[0] + 1, Ho = (Hh + 2 * pd[1] - kh) / st[1] + 1, Wo = (W + 2 * pd[2] - kw) / st[2] + 1;
        const int cp = cout_pad_of(cout), K = kd * kh * kw * cin_buf, k_pad = (K + kstep - 1) / kstep * kstep;
        sp.Cin = cin_buf; sp.Do = Do; sp.Ho = Ho; sp.Wo = Wo; sp.OD = Do; sp.OH = Ho; sp.OW = Wo;
        for (int i = 0; i < 3; ++i) { sp.st[i] = st[i]; sp.pd[i] = pd[i]; sp.ostr[i] = 1; }
        sp.Cout = cout; sp.cout_pad = cp; sp.k_pad = k_pad;
        fold_bn(cout, bias, bn, cp, sp.bias, sp.scale, sp.shift);
        sp.ph.resize(1);
        PhaseSpec& ph = sp.ph[0];
        ph.w.assign((size_t)cp * k_pad, 0.f);
        ph.ntaps = kd * kh * kw;
        const int64_t ktot = (int64_t)kd * kh * kw;
        for (int co = 0; co < cout; ++co)
            for (int ci = 0; ci < cin; ++ci) {
                const float* src = w.d + ((int64_t)co * cin + ci) * ktot;
                for (int t = 0; t < ktot; ++t) ph.w[(size_t)co * k_pad + (size_t)t * cin_buf + ci] = src[t];
            }
        for (int a = 0; a < kd; ++a)
            for (int b = 0; b < kh; ++b)
                for (int c = 0; c < kw; ++c) { ph.taps.push_back(a); ph.taps.push_back(b); ph.taps.push_back(c); ph.taps.push_back(((a * Hh + b) * W + c) * cin_buf); }
        return LT_OK;
    }
    // ---- stride-2 transposed convolution: one phase per output parity
    const int cin = (int)w.s[0], cout = (int)w.s[1];
    LT_REQUIRE(cin == cin_buf, LT_ERR_INVALID, "plan: the input of a transposed convolution may not be channel padded");
    LT_REQUIRE(stride == 2, LT_ERR_UNSUPPORTED, "plan: only stride-2 transposed convolutions");
    const int ks[3] = {kd, kh, kw}, dims[3] = {D, Hh, W};
    int outs[3];
    for (int i = 0; i < 3; ++i) {
        if (!nd3 && i == 0) { outs[i] = 1; continue; }
        const int o = (dims[i] - 1) * 2 - 2 * pd[i] + ks[i] + output_padding;
        LT_REQUIRE(o == 2 * dims[i], LT_ERR_UNSUPPORTED, "plan: a transposed convolution must exactly double the size (k = 4, p = 1 / k = 2, p = 0)");
        outs[i] = o;
    }
    const int cp = cout_pad_of(cout);
    struct DimPhase { int phi; std::vector<std::pair<int, int>> taps; };
    auto dim_phases = [&](int i) {
        std::vector<DimPhase> res;
        if (!nd3 && i == 0) { res.push_back({0, {{0, 0}}}); return res; }
        for (int phi = 0; phi < 2; ++phi) {          // o = 2 q + phi = 2 i_in - p + kk  ->  kk = phi + p (mod 2), i_in = q + (phi + p - kk) / 2
            DimPhase dp; dp.phi = phi;
            for (int kk = 0; kk < ks[i]; ++kk)
                if (floormod(phi + pd[i] - kk, 2) == 0) dp.taps.push_back({kk, floordiv(phi + pd[i] - kk, 2)});
            res.push_back(dp);
        }
        return res;
    };
    const int64_t ktot = (int64_t)kd * kh * kw;
    struct Raw { std::vector<std::pair<std::vector<float>, int>> dummy; };
    std::vector<PhaseSpec> phases;
    std::vector<std::vector<int>> phase_k;          // per phase: the filter tap index (ka, kb, kc flattened) of each recorded tap, -1 = zero tap
    int ntaps_max = 0;
    for (const DimPhase& A : dim_phases(0))
        for (const DimPhase& Bp : dim_phases(1))
            for (const DimPhase& Cp : dim_phases(2)) {
                PhaseSpec ph; std::vector<int> kidx;
                for (auto& ta : A.taps)
                    for (auto& tb : Bp.taps)
                        for (auto& tc : Cp.taps) {
                            const int da = ta.second, db = tb.second, dc = tc.second;
                            ph.taps.push_back(da); ph.taps.push_back(db); ph.taps.push_back(dc); ph.taps.push_back(((da * Hh + db) * W + dc) * cin);
                            kidx.push_back((ta.first * kh + tb.first) * kw + tc.first);
                        }
                if (kidx.empty()) { ph.taps = {0, 0, 0, 0}; kidx.push_back(-1); }          // an output parity no tap reaches: one tap with zero weights writes the zeros
                ph.ntaps = (int)kidx.size();
                ph.off[0] = A.phi; ph.off[1] = Bp.phi; ph.off[2] = Cp.phi;
                if (ph.ntaps > ntaps_max) ntaps_max = ph.ntaps;
                phases.push_back(ph); phase_k.push_back(kidx);
            }
    const int K = ntaps_max * cin, k_pad = (K + kstep - 1) / kstep * kstep;
    for (size_t p = 0; p < phases.size(); ++p) {
        PhaseSpec& ph = phases[p];
        ph.w.assign((size_t)cp * k_pad, 0.f);
        for (int t = 0; t < ph.ntaps; ++t) {
            const int kt = phase_k[p][t];
            if (kt < 0) continue;
            for (int ci = 0; ci < cin; ++ci)
                for (int co = 0; co < cout; ++co) ph.w[(size_t)co * k_pad + (size_t)t * cin + ci] = w.d[((int64_t)ci * cout + co) * ktot + kt];
        }
    }
    LT_REQUIRE((int)phases.size() <= LT_CONV_MAX_PHASES, LT_ERR_UNSUPPORTED, "plan: %d phases", (int)phases.size());
    sp.Cin = cin; sp.Do = D; sp.Ho = Hh; sp.Wo = W; sp.OD = outs[0]; sp.OH = outs[1]; sp.OW = outs[2];
    for (int i = 0; i < 3; ++i) { sp.st[i] = 1; sp.pd[i] = 0; }
    sp.ostr[0] = nd3 ? 2 : 1; sp.ostr[1] = 2; sp.ostr[2] = 2;
    sp.Cout = cout; sp.cout_pad = cp; sp.k_pad = k_pad;
    fold_bn(cout, bias, bn, cp, sp.bias, sp.scale, sp.shift);
    sp.ph = std::move(phases);
    return LT_OK;
}

}  // namespace

// =====================================================================================================================================
struct lt_plan {
    lt_vol_plan_config cfg;                     // volumetric plans; the algebraic / RANSAC plans fill the fields they share (shape, dtype, use_graph)
    int model = 0;                              // 0: volumetric plan, LT_MODEL_ALG | LT_MODEL_RANSAC (acfg), or MODEL_CASCADE (sub_alg + sub_vol)
    lt_alg_plan_config acfg = {};
    const char* who = "lt_plan_create_vol";     // the entry point that builds the plan, for error messages
    int dtype = LT_F32, es = 4;                 // element type / size of activations and weights
    std::unordered_map<std::string, const lt_named_tensor*> sd;
    std::vector<void*> allocs;                  // every hipMalloc of the plan
    std::map<std::pair<size_t, int>, std::vector<char*>> pool;          // released activations by (bytes, element size)
    size_t bytes_alloc = 0;
    double flops = 0;
    typedef std::function<int(hipStream_t)> Op;
    std::vector<Op> ops;                        // ops[0 .. npre) read the caller's images, ops[npre .. nops - ntail) are captured, the tail writes the caller's outputs
    int npre = 0, ntail = 0;
    std::deque<lt_conv_desc> conv_descs;        // descriptor storage with stable addresses (the launch closures hold pointers)
    std::deque<lt_conv_skip> skip_descs;
    std::deque<lt_conv_cat2> cat2_descs;
    std::deque<lt_pwchain_desc> pw_descs;
    std::deque<lt_stem_desc> stem_descs;
    std::deque<lt_bneck_desc> bneck_descs;
    std::deque<lt_bneck_ds_desc> bneck_ds_descs;
    std::deque<lt_xr_desc> xr_descs;
    hipGraphExec_t graph = nullptr;
    bool captured = false;
    hipStream_t own_stream = nullptr; hipEvent_t own_ev[2] = {nullptr, nullptr};          // stream == NULL with use_graph: the legacy default stream cannot be captured
    // per-call pointers the pre / tail ops read
    const float* cur_images = nullptr;
    float* out_kp = nullptr; float* out_probs = nullptr; float* out_feats = nullptr;
    const float* cur_proj = nullptr; void* out_kp2d = nullptr; float* out_hm = nullptr; float* out_conf = nullptr;          // algebraic / RANSAC plans
    // geometry block (fp32): proj B*NV*12 | pos B*3 | center B*3 | rot B*9 -- one H2D copy per forward from a ring of pinned blocks
    float* geo_dev = nullptr; StagingRing geo; size_t n_geo = 0, o_pos = 0, o_cen = 0, o_rot = 0;
    // several cuboids per frame (lt_plan_create_vol_multi): P > 0 cuboids over the cfg.B frames -- the backbone is recorded at B * NV images, the gather, V2V and
    // the tail at P; the block is proj B*NV*12 | pos P*3 | center P*3 | rot P*9 | frame_of P int32 (o_fof, in floats).  P == 0: one cuboid per sample.
    int P = 0; size_t o_fof = 0;
    // ragged view batches (lt_plan_create_vol_ragged / lt_plan_create_alg_ragged): T > 0 images over the cfg.B samples, cfg.NV = NVcap -- the backbone is recorded
    // at T images, the gather (lt_unproject_grid_ragged_fwd) or the algebraic tail (lt_alg_tail_ragged_fwd) finds a sample's views through the B + 1 int32
    // offsets.  Volumetric plans carry them in the geometry block behind the rotations (o_vb, in floats), algebraic plans in a block of their own (vb_dev)
    // behind its pinned ring.  T == 0: NV views per sample.
    int T = 0; size_t o_vb = 0;
    int32_t* vb_dev = nullptr; StagingRing avb;
    int images() const { return T ? T : cfg.B * cfg.NV; }
    int cuboids() const { return P ? P : cfg.B; }
    // results
    Act feats, vol, logits, volc;
    float* coords = nullptr; float* kp = nullptr; float* probs = nullptr; void* sa_ws = nullptr;
    // per-joint statistics (lt_plan_set_keypoint_stats): the caller's device buffers, read by the eager tail op when it runs, and the larger workspace of
    // lt_softargmax3d_stats_fwd, allocated by the first call that asks for them
    float* ks_stats = nullptr; int32_t* ks_index = nullptr; void* ks_ws = nullptr;
    // per-joint statistics of the algebraic joints (lt_plan_set_alg_keypoint_stats): the caller's five device buffers, all set or all NULL, read by the
    // two eager tail ops when they run
    float* aks_stats2d = nullptr; int32_t* aks_index = nullptr; float* aks_cov2d = nullptr; float* aks_reproj = nullptr; float* aks_cov3d = nullptr;
    Act algc;                                   // alg_confidences head output [1,1,1,N,J] fp32 (algebraic plans with use_confidences)
    float* hm_nchw = nullptr; float* kp_hm = nullptr; int64_t* kp_i64 = nullptr;          // heatmaps N,J,h,w; soft-argmax N,J,2 (heatmap px); argmax N,J,2
    int hm_h = 0, hm_w = 0;
    // cascade plans: the two stages, the algebraic stage's image-resolution projections (pinned ring + device copy; the ring turns with sub_vol's geometry
    // ring and is guarded by that ring's events, re-recorded behind this copy: it is never committed itself, so it never waits) and its joints when the
    // caller does not ask for them
    lt_plan* sub_alg = nullptr; lt_plan* sub_vol = nullptr; int kind = 0;
    float* cproj_dev = nullptr; StagingRing cproj; float* ckp_alg = nullptr;
    // per-sample view masks (lt_plan_set_view_mask).  masked: the gather / the algebraic tail run their masked entry points, chosen before the first forward
    // (what the graph captures).  mask_cur: the host (B, NV) mask, kept until replaced.  Volumetric plans carry it at the end of the geometry block (o_mask:
    // offset in floats; same ring slot, same copy); algebraic plans have no such block: a ring of their own, copied when the mask has changed; the algebraic
    // stage of a cascade reads the volumetric stage's block.
    bool masked = false, ran = false, mask_dirty = false;
    std::vector<uint8_t> mask_cur;
    const uint8_t* mask_dev = nullptr; size_t o_mask = 0;
    uint8_t* amask_dev = nullptr; StagingRing amask;
    int n_xr = 0, n_bneck = 0, n_bneck_ds = 0, n_cat2 = 0, n_halo2d = 0, n_pwchain = 0, n_stem = 0, n_splitk = 0, n_conv_skip = 0;

    ~lt_plan() {
        if (graph) (void)hipGraphExecDestroy(graph);
        if (own_stream) (void)hipStreamDestroy(own_stream);
        for (int i = 0; i < 2; ++i) if (own_ev[i]) (void)hipEventDestroy(own_ev[i]);
        for (void* p : allocs) (void)hipFree(p);
        delete sub_alg;
        delete sub_vol;
    }

    // ---- memory ------------------------------------------------------------------------------------------------------------------
    int dev_alloc(size_t bytes, void** out) {
        void* p = nullptr;
        PL_HIP(hipMalloc(&p, bytes ? bytes : 16));
        allocs.push_back(p);
        bytes_alloc += bytes;
        *out = p;
        return LT_OK;
    }
    int alloc(int n, int d, int h, int w, int c, int esz, Act& a) {          // PlanBuilder.alloc: size-keyed reuse of released activations
        a = Act(); a.n = n; a.d = d; a.h = h; a.w = w; a.c = c; a.es = esz;
        auto it = pool.find({a.bytes(), esz});
        if (it != pool.end() && !it->second.empty()) { a.p = it->second.back(); it->second.pop_back(); return LT_OK; }
        void* p; PL_TRY(dev_alloc(a.bytes(), &p)); a.p = (char*)p;
        return LT_OK;
    }
    void release(const Act& a) { if (a.p && a.pooled) pool[{a.bytes(), a.es}].push_back(a.p); }          // stream order makes the reuse safe
    int upload(const void* host, size_t bytes, void** out) {
        PL_TRY(dev_alloc(bytes, out));
        PL_HIP(hipMemcpy(*out, host, bytes, hipMemcpyHostToDevice));
        return LT_OK;
    }
    int upload_f32(const std::vector<float>& v, const float** out) { void* p; PL_TRY(upload(v.data(), v.size() * 4, &p)); *out = (const float*)p; return LT_OK; }
    int upload_w(const std::vector<float>& v, const void** out) {          // weights in the plan's element type (bf16: round to nearest even like torch's .to(bfloat16))
        if (es == 4) { void* p; PL_TRY(upload(v.data(), v.size() * 4, &p)); *out = p; return LT_OK; }
        std::vector<unsigned short> h(v.size());
        for (size_t i = 0; i < v.size(); ++i) h[i] = bf16_rne(v[i]);
        void* p; PL_TRY(upload(h.data(), h.size() * 2, &p)); *out = p;
        return LT_OK;
    }
    int upload_i32(const std::vector<int32_t>& v, const int32_t** out) { void* p; PL_TRY(upload(v.data(), v.size() * 4, &p)); *out = (const int32_t*)p; return LT_OK; }

    // ---- state dict ----------------------------------------------------------------------------------------------------------------
    int get(const std::string& name, WT& w, int nd_expect = 0) {
        auto it = sd.find(name);
        LT_REQUIRE(it != sd.end(), LT_ERR_INVALID, "%s: state dict has no '%s'", who, name.c_str());
        const lt_named_tensor* t = it->second;
        LT_REQUIRE(t->data && t->ndim >= 1 && t->ndim <= 5 && (!nd_expect || t->ndim == nd_expect), LT_ERR_INVALID, "%s: '%s' has %d dimensions", who, name.c_str(), t->ndim);
        w.d = t->data; w.nd = t->ndim;
        for (int i = 0; i < t->ndim; ++i) w.s[i] = t->shape[i];
        return LT_OK;
    }
    bool has(const std::string& name) const { return sd.find(name) != sd.end(); }
    int get_vec(const std::string& name, int n, const float** out) {
        WT w; PL_TRY(get(name, w));
        LT_REQUIRE(w.numel() == n, LT_ERR_INVALID, "%s: '%s' has %lld elements, expected %d", who, name.c_str(), (long long)w.numel(), n);
        *out = w.d;
        return LT_OK;
    }
    int get_bn(const std::string& prefix, int c, BN& bn) {
        PL_TRY(get_vec(prefix + ".weight", c, &bn.g)); PL_TRY(get_vec(prefix + ".bias", c, &bn.b));
        PL_TRY(get_vec(prefix + ".running_mean", c, &bn.m)); PL_TRY(get_vec(prefix + ".running_var", c, &bn.v));
        return LT_OK;
    }

    // ---- ops ------------------------------------------------------------------------------------------------------------------------
    struct ConvOpt {
        const float* bias = nullptr; const BN* bn = nullptr;
        int stride = 1, pad = 0; bool transposed = false, relu = false, relu_pre = false, out_f32 = false, sigmoid = false;
        const Act* residual = nullptr;
        // lt_conv_skip_fwd: the residual is a 1x1x1 convolution + BatchNorm of this 16-channel tensor, computed inside the launch
        const Act* skip_x = nullptr; const WT* skip_w = nullptr; const float* skip_bias = nullptr; const BN* skip_bn = nullptr;
    };

    void fill_desc(lt_conv_desc& d, const ConvSpec& sp) {
        memset(&d, 0, sizeof(d));
        d.dtype = dtype;
        d.N = sp.N; d.D = sp.D; d.H = sp.H; d.W = sp.W; d.Cin = sp.Cin; d.Do = sp.Do; d.Ho = sp.Ho; d.Wo = sp.Wo;
        for (int i = 0; i < 3; ++i) { d.stride[i] = sp.st[i]; d.pad[i] = sp.pd[i]; d.out_stride[i] = sp.ostr[i]; }
        d.OD = sp.OD; d.OH = sp.OH; d.OW = sp.OW;
        d.Cout = sp.Cout; d.ldc = sp.Cout; d.cout_pad = sp.cout_pad; d.k_pad = sp.k_pad;
        d.nphase = (int)sp.ph.size(); d.flags = sp.flags; d.tile = 0; d.stages = 0;
        for (size_t i = 0; i < sp.ph.size(); ++i) {
            d.phase[i].ntaps = sp.ph[i].ntaps;
            for (int k = 0; k < 3; ++k) d.phase[i].out_off[k] = sp.ph[i].off[k];
        }
    }

    int pack_frag(const void* wdev, size_t elems, int which, int cout_pad, int k_pad, int cin, int ntaps, const void** out) {
        void* p; PL_TRY(dev_alloc(elems * 2, &p));
        int rc;
        if (which == 2) rc = lt_conv_pack_weights_t32(wdev, cout_pad, k_pad, cin, ntaps, p, nullptr);
        else if (which == 3) rc = lt_conv_pack_weights32(wdev, cout_pad, k_pad, p, nullptr);
        else rc = lt_conv_pack_weights(wdev, cout_pad, k_pad, p, nullptr);
        PL_TRY(rc);
        PL_HIP(hipStreamSynchronize(nullptr));
        *out = p;
        return LT_OK;
    }

    // PlanBuilder.conv
    int conv(const Act& x, const WT& w, const ConvOpt& o, Act& y) {
        const int flags = (o.relu ? LT_EPI_RELU_POST : 0) | (o.relu_pre ? LT_EPI_RELU_PRE : 0) | (o.out_f32 ? LT_EPI_STORE_F32 : 0) | (o.sigmoid ? LT_EPI_SIGMOID : 0);
        const int in[5] = {x.n, x.d, x.h, x.w, x.c};
        ConvSpec sp;
        PL_TRY(make_conv_spec(w, o.bias, o.bn, in, o.stride, o.pad, es, o.transposed, flags, 0, sp));
        const lt_wshape ws = wshape(w);
        lt_conv_skip* sk = nullptr;
        if (o.skip_x) {
            const lt_wshape sws = wshape(*o.skip_w);
            LT_REQUIRE(!o.residual && !o.relu_pre && !o.out_f32 && lt_sel_conv_skip(dtype, in, &ws, dims(*o.skip_x).data(), &sws), LT_ERR_INVALID, "plan: conv_skip on an unsupported shape");
            const int sin[5] = {o.skip_x->n, o.skip_x->d, o.skip_x->h, o.skip_x->w, o.skip_x->c};
            ConvSpec ss;
            PL_TRY(make_conv_spec(*o.skip_w, o.skip_bias, o.skip_bn, sin, 1, 0, es, false, 0, 0, ss));
            LT_REQUIRE(ss.cout_pad == 32 && sp.cout_pad == 32, LT_ERR_INVALID, "plan: conv_skip widths");
            // the skip branch's BatchNorm: scale into its weights (fp32 product, ONE bf16 rounding), (bias * scale + shift) into this convolution's shift
            std::vector<float> wf((size_t)32 * ss.k_pad);
            for (int co = 0; co < 32; ++co) for (int k = 0; k < ss.k_pad; ++k) wf[(size_t)co * ss.k_pad + k] = ss.ph[0].w[(size_t)co * ss.k_pad + k] * ss.scale[co];
            for (int co = 0; co < 32; ++co) { const float bs = ss.bias[co] * ss.scale[co]; const float t = sp.shift[co] + bs; sp.shift[co] = t + ss.shift[co]; }          // Python's order: (shift + bias * scale) + shift_skip
            const void* wsk; PL_TRY(upload_w(wf, &wsk));
            const void* wfr; PL_TRY(pack_frag(wsk, 32 * 16, 2, 32, ss.k_pad, 16, 1, &wfr));
            skip_descs.emplace_back();
            sk = &skip_descs.back();
            sk->x = o.skip_x->p; sk->cin = 16; sk->weight_frag = wfr;
            ++n_conv_skip;
        }
        lt_conv_desc d0;
        fill_desc(d0, sp);
        const int S = lt_sel_splitk_slices(&d0, &ws, o.transposed);
        if (S > 1) return conv_splitk(x, w, sp, S, o.residual, y);
        PL_TRY(alloc(sp.N, sp.OD, sp.OH, sp.OW, sp.Cout, o.out_f32 ? 4 : es, y));
        if (o.residual) LT_REQUIRE(o.residual->n == y.n && o.residual->d == y.d && o.residual->h == y.h && o.residual->w == y.w && o.residual->c == y.c && o.residual->es == es,
                                   LT_ERR_INVALID, "plan: residual shape");
        conv_descs.push_back(d0);
        lt_conv_desc& d = conv_descs.back();
        // the weights ALSO in the MFMA fragment order of the kernel that will run the layer (bf16 plans)
        const int layout = lt_sel_frag_layout(&d, &ws, o.transposed, o.residual != nullptr);
        if (layout == 2 && w.nd == 4) ++n_halo2d;
        for (size_t i = 0; i < sp.ph.size(); ++i) {
            const PhaseSpec& ph = sp.ph[i];
            const void* wdev; PL_TRY(upload_w(ph.w, &wdev));
            const int32_t* tdev; PL_TRY(upload_i32(ph.taps, &tdev));
            d.phase[i].weight = wdev; d.phase[i].taps = tdev;
            if (layout) {
                const void* wfr; PL_TRY(pack_frag(wdev, (size_t)sp.cout_pad * sp.k_pad, layout, sp.cout_pad, sp.k_pad, sp.Cin, ph.ntaps, &wfr));
                d.phase[i].weight_frag = wfr; d.phase[i].weight_frag_layout = layout;
            }
        }
        const float *bi, *sc, *sh;
        PL_TRY(upload_f32(sp.bias, &bi)); PL_TRY(upload_f32(sp.scale, &sc)); PL_TRY(upload_f32(sp.shift, &sh));
        long long taps = 0;
        for (auto& q : sp.ph) taps += q.ntaps;
        flops += 2.0 * sp.N * sp.Do * sp.Ho * sp.Wo * sp.Cout * taps * (o.transposed ? w.s[0] : w.s[1]);
        const lt_conv_desc* dp = &d;
        const void* xp = x.p; void* yp = y.p; const void* rp = o.residual ? o.residual->p : nullptr;
        if (sk) {
            flops += 2.0 * sp.N * sp.Do * sp.Ho * sp.Wo * sp.Cout * 16;
            ops.push_back([=](hipStream_t s) { return lt_conv_skip_fwd(dp, xp, bi, sc, sh, sk, yp, s); });
        } else
            ops.push_back([=](hipStream_t s) { return lt_conv_fwd(dp, xp, bi, sc, sh, rp, yp, s); });
        return LT_OK;
    }

    // PlanBuilder._conv_splitk
    int conv_splitk(const Act& x, const WT& w, const ConvSpec& sp, int S, const Act* residual, Act& y) {
        const PhaseSpec& ph0 = sp.ph[0];
        const int ntaps = ph0.ntaps, Cin = sp.Cin, kstep = 128 / es;
        std::vector<int> bounds(S + 1);
        int maxg = 0;
        for (int i = 0; i <= S; ++i) bounds[i] = ntaps * i / S;
        for (int i = 0; i < S; ++i) if (bounds[i + 1] - bounds[i] > maxg) maxg = bounds[i + 1] - bounds[i];
        const int kp = (maxg * Cin + kstep - 1) / kstep * kstep;
        Act part; PL_TRY(alloc(sp.N, S * sp.Do, sp.Ho, sp.Wo, sp.Cout, 4, part));
        PL_TRY(alloc(sp.N, sp.Do, sp.Ho, sp.Wo, sp.Cout, es, y));
        const long long rows = (long long)sp.N * sp.Do * sp.Ho * sp.Wo;
        conv_descs.emplace_back();
        lt_conv_desc& d = conv_descs.back();
        fill_desc(d, sp);
        d.OD = S * sp.Do; d.k_pad = kp; d.nphase = S; d.flags = LT_EPI_STORE_F32;
        d.tile = rows >= 8192 ? LT_TILE2_128x128 : LT_TILE2_64x64;
        for (int i = 0; i < S; ++i) {
            const int t0 = bounds[i], t1 = bounds[i + 1];
            std::vector<float> wk((size_t)sp.cout_pad * kp, 0.f);
            for (int co = 0; co < sp.cout_pad; ++co)
                for (int k = t0 * Cin; k < t1 * Cin; ++k) wk[(size_t)co * kp + (k - t0 * Cin)] = ph0.w[(size_t)co * sp.k_pad + k];
            std::vector<int32_t> tp(ph0.taps.begin() + 4 * t0, ph0.taps.begin() + 4 * t1);
            const void* wdev; PL_TRY(upload_w(wk, &wdev));
            const int32_t* tdev; PL_TRY(upload_i32(tp, &tdev));
            d.phase[i].weight = wdev; d.phase[i].taps = tdev; d.phase[i].ntaps = t1 - t0;
            d.phase[i].out_off[0] = i * sp.Do; d.phase[i].out_off[1] = 0; d.phase[i].out_off[2] = 0;
        }
        std::vector<float> zero(sp.cout_pad, 0.f), one(sp.cout_pad, 1.f);
        const float *ibi, *isc, *ish, *bi, *sc, *sh;
        PL_TRY(upload_f32(zero, &ibi)); PL_TRY(upload_f32(one, &isc)); PL_TRY(upload_f32(zero, &ish));
        PL_TRY(upload_f32(sp.bias, &bi)); PL_TRY(upload_f32(sp.scale, &sc)); PL_TRY(upload_f32(sp.shift, &sh));
        flops += 2.0 * rows * sp.Cout * ntaps * w.s[1];
        const lt_conv_desc* dp = &d;
        const void* xp = x.p; float* pp = (float*)part.p; void* yp = y.p; const void* rp = residual ? residual->p : nullptr;
        ops.push_back([=](hipStream_t s) { return lt_conv_fwd(dp, xp, ibi, isc, ish, nullptr, pp, s); });
        const int dt = dtype, N = sp.N, C = sp.Cout, fl = sp.flags;
        const long long R = (long long)sp.Do * sp.Ho * sp.Wo;
        ops.push_back([=](hipStream_t s) { return lt_splitk_reduce(dt, pp, S, N, R, C, bi, sc, sh, rp, yp, fl, s); });
        release(part);
        ++n_splitk;
        return LT_OK;
    }

    // PlanBuilder.conv_cat2: expand + (strided) downsample branch of a Bottleneck's first block as ONE pointwise convolution over [t2 | x]
    int conv_cat2(const Act& t2, const WT& we, const BN& bne, const Act& x, const WT& wd, const BN& bnd, int sds, Act& y) {
        const int N = t2.n, Ho = t2.h, Wo = t2.w, P = t2.c, Cc = (int)we.s[0], Cin2 = (int)wd.s[1];
        const int t2s[5] = {t2.n, t2.d, t2.h, t2.w, t2.c}, xs[5] = {x.n, x.d, x.h, x.w, x.c};
        ConvSpec s3, sd_;
        PL_TRY(make_conv_spec(we, nullptr, &bne, t2s, 1, 0, es, false, LT_EPI_RELU_POST, 0, s3));
        PL_TRY(make_conv_spec(wd, nullptr, &bnd, xs, sds, 0, es, false, 0, 0, sd_));
        LT_REQUIRE(s3.cout_pad == Cc && sd_.cout_pad == Cc, LT_ERR_INVALID, "plan: conv_cat2 widths");
        const int kp = P + Cin2;
        std::vector<float> wcat((size_t)Cc * kp), shift(Cc), zero(Cc, 0.f);
        for (int co = 0; co < Cc; ++co) {
            for (int k = 0; k < P; ++k) wcat[(size_t)co * kp + k] = s3.ph[0].w[(size_t)co * s3.k_pad + k] * s3.scale[co];
            for (int k = 0; k < Cin2; ++k) wcat[(size_t)co * kp + P + k] = sd_.ph[0].w[(size_t)co * sd_.k_pad + k] * sd_.scale[co];
            const float a = s3.bias[co] * s3.scale[co], a2 = a + s3.shift[co], b = sd_.bias[co] * sd_.scale[co], b2 = b + sd_.shift[co];
            shift[co] = a2 + b2;
        }
        PL_TRY(alloc(N, 1, Ho, Wo, Cc, es, y));
        conv_descs.emplace_back();
        lt_conv_desc& d = conv_descs.back();
        memset(&d, 0, sizeof(d));
        d.dtype = dtype; d.N = N; d.D = 1; d.H = Ho; d.W = Wo; d.Cin = P; d.Do = 1; d.Ho = Ho; d.Wo = Wo;
        for (int i = 0; i < 3; ++i) { d.stride[i] = 1; d.pad[i] = 0; d.out_stride[i] = 1; }
        d.OD = 1; d.OH = Ho; d.OW = Wo; d.Cout = Cc; d.ldc = Cc; d.cout_pad = Cc; d.k_pad = kp; d.nphase = 1; d.flags = LT_EPI_RELU_POST;
        const void* wdev; PL_TRY(upload_w(wcat, &wdev));
        const int32_t* tdev; PL_TRY(upload_i32(s3.ph[0].taps, &tdev));
        const void* wfr; PL_TRY(pack_frag(wdev, (size_t)Cc * kp, 3, Cc, kp, 0, 0, &wfr));
        d.phase[0].weight = wdev; d.phase[0].taps = tdev; d.phase[0].ntaps = 1; d.phase[0].weight_frag = wfr; d.phase[0].weight_frag_layout = 3;
        cat2_descs.emplace_back();
        lt_conv_cat2& c2 = cat2_descs.back();
        c2.x = x.p; c2.cin = Cin2; c2.H = x.h; c2.W = x.w; c2.stride = sds;
        const float *bi, *sh;
        PL_TRY(upload_f32(zero, &bi)); PL_TRY(upload_f32(shift, &sh));
        flops += 2.0 * N * Ho * Wo * Cc * kp;
        const lt_conv_desc* dp = &d; const lt_conv_cat2* cp = &c2;
        const void* xp = t2.p; void* yp = y.p;
        ops.push_back([=](hipStream_t s) { return lt_conv_cat2_fwd(dp, xp, cp, bi, nullptr, sh, nullptr, yp, s); });
        ++n_cat2;
        return LT_OK;
    }

    // PlanBuilder.pwchain: V2V's pointwise tail in one pass, planar fp32 logits
    struct PwLayer { WT w; const float* bias; const BN* bn; bool relu; };
    int pwchain(const Act& x, const std::vector<PwLayer>& L, Act& y) {
        pw_descs.emplace_back();
        lt_pwchain_desc& d = pw_descs.back();
        memset(&d, 0, sizeof(d));
        d.dtype = dtype; d.nlayers = (int)L.size(); d.rows = (long long)x.n * x.d * x.h * x.w; d.cin = 32;
        int shape[5] = {x.n, x.d, x.h, x.w, x.c};
        int cout_last = 0;
        for (size_t i = 0; i < L.size(); ++i) {
            const bool last = i + 1 == L.size();
            const int fl = (L[i].relu ? LT_EPI_RELU_POST : 0) | (last ? LT_EPI_STORE_F32 : 0);
            ConvSpec sp; PL_TRY(make_conv_spec(L[i].w, L[i].bias, L[i].bn, shape, 1, 0, es, false, fl, 0, sp));
            // lt_pwchain_fwd reads [32][k_pad] weights and 32 epilogue constants per layer: a last layer of <= 16 channels is packed with 16 rows, pad it
            if (sp.cout_pad < 32) { sp.ph[0].w.resize((size_t)32 * sp.k_pad, 0.f); sp.bias.resize(32, 0.f); sp.scale.resize(32, 0.f); sp.shift.resize(32, 0.f); }
            const void* wdev; PL_TRY(upload_w(sp.ph[0].w, &wdev));
            const float *bi, *sc, *sh;
            PL_TRY(upload_f32(sp.bias, &bi)); PL_TRY(upload_f32(sp.scale, &sc)); PL_TRY(upload_f32(sp.shift, &sh));
            d.cout[i] = sp.Cout; d.k_pad[i] = sp.k_pad; d.flags[i] = fl; d.weight[i] = wdev; d.bias[i] = bi; d.scale[i] = sc; d.shift[i] = sh;
            flops += 2.0 * d.rows * sp.Cout * L[i].w.s[1];
            shape[4] = sp.Cout; cout_last = sp.Cout;
        }
        d.ldy = cout_last;
        const long long vox = (long long)x.d * x.h * x.w;
        const bool planar = vox % 64 == 0;
        if (planar) d.plane = vox;
        PL_TRY(alloc(x.n, x.d, x.h, x.w, cout_last, 4, y));
        y.planar = planar; y.pooled = !planar;
        const lt_pwchain_desc* dp = &d; const void* xp = x.p; void* yp = y.p;
        ops.push_back([=](hipStream_t s) { return lt_pwchain_fwd(dp, xp, yp, s); });
        ++n_pwchain;
        return LT_OK;
    }

    int maxpool(const Act& x, int k, int s, int p, int nd, Act& y) {
        int32_t kk[3] = {nd == 2 ? 1 : k, k, k}, ss[3] = {nd == 2 ? 1 : s, s, s}, pp[3] = {nd == 2 ? 0 : p, p, p};
        const int od = (x.d + 2 * pp[0] - kk[0]) / ss[0] + 1, oh = (x.h + 2 * pp[1] - kk[1]) / ss[1] + 1, ow = (x.w + 2 * pp[2] - kk[2]) / ss[2] + 1;
        PL_TRY(alloc(x.n, od, oh, ow, x.c, x.es, y));
        const int dt = dtype; const Act xa = x; void* yp = y.p;
        std::vector<int32_t> a = {kk[0], kk[1], kk[2], ss[0], ss[1], ss[2], pp[0], pp[1], pp[2]};
        ops.push_back([=](hipStream_t st) { return lt_maxpool_fwd(dt, xa.p, yp, xa.n, xa.d, xa.h, xa.w, xa.c, a.data(), a.data() + 3, a.data() + 6, st); });
        return LT_OK;
    }

    int global_avgpool(const Act& x, Act& y) {          // [N,1,H,W,C] -> [1,1,1,N,C]: a one-row "image" of N pixels, feeds 1x1 convolutions = linears
        PL_TRY(alloc(1, 1, 1, x.n, x.c, x.es, y));
        const int dt = dtype; const Act xa = x; void* yp = y.p;
        ops.push_back([=](hipStream_t st) { return lt_global_avgpool(dt, xa.p, yp, xa.n, xa.d * xa.h * xa.w, xa.c, st); });
        return LT_OK;
    }

    // ---- whole-block launches of the bf16 plan (lt_engine.PlanBuilder.bottleneck / bottleneck_ds / expand_reduce / stem_pool) ------------------------
    int pack_block_layer(const WT& w, const BN& bn, const int in[5], int pad, int fl, const void** wfr, const float** sc, const float** sh, ConvSpec& sp) {
        PL_TRY(make_conv_spec(w, nullptr, &bn, in, 1, pad, es, false, fl, 0, sp));
        LT_REQUIRE(sp.cout_pad == sp.Cout && sp.k_pad == sp.ph[0].ntaps * sp.Cin, LT_ERR_INVALID, "plan: fused block layer padding (%d / %d)", sp.cout_pad, sp.k_pad);
        const void* wdev; PL_TRY(upload_w(sp.ph[0].w, &wdev));
        PL_TRY(pack_frag(wdev, (size_t)sp.cout_pad * sp.k_pad, 2, sp.cout_pad, sp.k_pad, sp.Cin, sp.ph[0].ntaps, wfr));
        PL_TRY(upload_f32(sp.scale, sc)); PL_TRY(upload_f32(sp.shift, sh));
        flops += 2.0 * in[0] * in[2] * in[3] * sp.Cout * sp.ph[0].ntaps * sp.Cin;
        return LT_OK;
    }
    int bottleneck(const Act& x, const WT w[3], const BN bn[3], Act& y) {
        PL_TRY(alloc(x.n, 1, x.h, x.w, x.c, es, y));
        bneck_descs.emplace_back();
        lt_bneck_desc& d = bneck_descs.back();
        memset(&d, 0, sizeof(d));
        d.dtype = dtype; d.N = x.n; d.H = x.h; d.W = x.w; d.C = x.c; d.P = (int)w[0].s[0];
        int shape[5] = {x.n, 1, x.h, x.w, x.c};
        for (int i = 0; i < 3; ++i) {
            ConvSpec sp;
            PL_TRY(pack_block_layer(w[i], bn[i], shape, i == 1 ? 1 : 0, LT_EPI_RELU_POST, &d.weight[i], &d.scale[i], &d.shift[i], sp));
            shape[4] = sp.Cout;
        }
        const lt_bneck_desc* dp = &d; const void* xp = x.p; void* yp = y.p;
        ops.push_back([=](hipStream_t s) { return lt_bottleneck_fwd(dp, xp, yp, s); });
        ++n_bneck;
        return LT_OK;
    }
    int bottleneck_ds(const Act& x, const WT w[3], const BN bn[3], const WT& wd, const BN& bnd, Act& y) {
        const int Cc = (int)w[2].s[0];
        PL_TRY(alloc(x.n, 1, x.h, x.w, Cc, es, y));
        bneck_ds_descs.emplace_back();
        lt_bneck_ds_desc& d = bneck_ds_descs.back();
        memset(&d, 0, sizeof(d));
        d.dtype = dtype; d.N = x.n; d.H = x.h; d.W = x.w; d.Cin = x.c; d.P = (int)w[0].s[0]; d.C = Cc;
        int shape[5] = {x.n, 1, x.h, x.w, x.c};
        for (int i = 0; i < 3; ++i) {
            ConvSpec sp;
            PL_TRY(pack_block_layer(w[i], bn[i], shape, i == 1 ? 1 : 0, LT_EPI_RELU_POST, &d.weight[i], &d.scale[i], &d.shift[i], sp));
            shape[4] = sp.Cout;
        }
        const int xs[5] = {x.n, 1, x.h, x.w, x.c};
        ConvSpec sp;
        PL_TRY(pack_block_layer(wd, bnd, xs, 0, 0, &d.weight[3], &d.scale[3], &d.shift[3], sp));
        const lt_bneck_ds_desc* dp = &d; const void* xp = x.p; void* yp = y.p;
        ops.push_back([=](hipStream_t s) { return lt_bottleneck_ds_fwd(dp, xp, yp, s); });
        ++n_bneck_ds;
        return LT_OK;
    }
    int expand_reduce(const Act& t2, const Act& res, const WT& we, const BN& bne, const WT& wr, const BN& bnr, Act& y, Act& t1) {
        const int N = t2.n, Hh = t2.h, W = t2.w, P = t2.c, Cc = res.c;
        PL_TRY(alloc(N, 1, Hh, W, Cc, es, y));
        PL_TRY(alloc(N, 1, Hh, W, P, es, t1));
        xr_descs.emplace_back();
        lt_xr_desc& d = xr_descs.back();
        memset(&d, 0, sizeof(d));
        d.dtype = dtype; d.C = Cc; d.P = P; d.M = (long long)N * Hh * W;
        const int s2[5] = {t2.n, 1, Hh, W, P}, sr[5] = {res.n, 1, Hh, W, Cc};
        ConvSpec s3, s1;
        PL_TRY(pack_block_layer(we, bne, s2, 0, LT_EPI_RELU_POST, &d.weight[0], &d.scale[0], &d.shift[0], s3));
        PL_TRY(pack_block_layer(wr, bnr, sr, 0, LT_EPI_RELU_POST, &d.weight[1], &d.scale[1], &d.shift[1], s1));
        std::vector<float> packed;          // the four tables back to back: one LDS-DMA in the kernel's prologue
        packed.insert(packed.end(), s3.scale.begin(), s3.scale.end()); packed.insert(packed.end(), s3.shift.begin(), s3.shift.end());
        packed.insert(packed.end(), s1.scale.begin(), s1.scale.end()); packed.insert(packed.end(), s1.shift.begin(), s1.shift.end());
        PL_TRY(upload_f32(packed, &d.consts));
        const lt_xr_desc* dp = &d; const void* a = t2.p; const void* r = res.p; void* yp = y.p; void* tp = t1.p;
        ops.push_back([=](hipStream_t s) { return lt_expand_reduce_fwd(dp, a, r, yp, tp, s); });
        ++n_xr;
        return LT_OK;
    }
    // conv1 + bn1 + relu + maxpool in one pass, reading the caller's fp32 (N,3,H,W) images: the first op of the plan, outside the captured graph
    int stem_pool(int N, int Hh, int W, const WT& w, const BN& bn, Act& y) {
        const int in[5] = {N, 1, Hh, W, 8};
        ConvSpec sp;
        PL_TRY(make_conv_spec(w, nullptr, &bn, in, 2, 3, es, false, LT_EPI_RELU_POST, 0, sp));
        const int Hp = (sp.Ho - 1) / 2 + 1, Wp = (sp.Wo - 1) / 2 + 1;
        PL_TRY(alloc(N, 1, Hp, Wp, 64, es, y));
        const void* wdev; PL_TRY(upload_w(sp.ph[0].w, &wdev));
        void* wpk; PL_TRY(dev_alloc(lt_stem_packed_bytes(), &wpk));
        PL_TRY(lt_stem_pack_weights(wdev, sp.k_pad, wpk, nullptr));
        PL_HIP(hipStreamSynchronize(nullptr));
        stem_descs.emplace_back();
        lt_stem_desc& d = stem_descs.back();
        memset(&d, 0, sizeof(d));
        d.dtype = dtype; d.N = N; d.H = Hh; d.W = W; d.Cin = 3; d.Cout = 64; d.weight = wpk; d.x_layout = 1;
        PL_TRY(upload_f32(sp.bias, &d.bias)); PL_TRY(upload_f32(sp.scale, &d.scale)); PL_TRY(upload_f32(sp.shift, &d.shift));
        flops += 2.0 * N * sp.Ho * sp.Wo * 64 * 49 * w.s[1];
        const lt_stem_desc* dp = &d; void* yp = y.p; lt_plan* self = this;
        LT_REQUIRE(ops.empty(), LT_ERR_INVALID, "plan: an op reading the caller's tensor must be the first of the plan");
        ops.push_back([=](hipStream_t s) { return lt_stem_pool_fwd(dp, self->cur_images, yp, s); });
        npre = 1;
        ++n_stem;
        return LT_OK;
    }

    // ---- the networks ---------------------------------------------------------------------------------------------------------------
    struct Block {          // one residual block of the backbone (pose_resnet.py:57-137)
        bool bottleneck; int nconv; WT w[3]; BN bn[3]; int strides[3]; bool has_ds; WT wd; BN bnd; int sds;
        bool identity_bottleneck() const { return bottleneck && !has_ds && strides[0] == 1 && strides[1] == 1 && strides[2] == 1; }
    };
    int load_block(const std::string& pre, bool bott, bool caffe, int stride, bool ds, Block& b) {
        b.bottleneck = bott; b.nconv = bott ? 3 : 2; b.has_ds = ds; b.sds = stride;
        if (bott) { b.strides[0] = caffe ? stride : 1; b.strides[1] = caffe ? 1 : stride; b.strides[2] = 1; }
        else { b.strides[0] = stride; b.strides[1] = 1; b.strides[2] = 1; }
        for (int i = 0; i < b.nconv; ++i) {
            PL_TRY(get(pre + ".conv" + std::to_string(i + 1) + ".weight", b.w[i], 4));
            PL_TRY(get_bn(pre + ".bn" + std::to_string(i + 1), (int)b.w[i].s[0], b.bn[i]));
        }
        if (ds) { PL_TRY(get(pre + ".downsample.0.weight", b.wd, 4)); PL_TRY(get_bn(pre + ".downsample.1", (int)b.wd.s[0], b.bnd)); }
        return LT_OK;
    }
    // ResidualBlock.record.  t1: this block's first activation when the previous block's seam launch produced it; nxt: fuse this block's expand with that
    // block's reduce where the plan supports the shape (t1n is then the next block's first activation, null otherwise).
    int record_block(const Block& b, const Act& x, const Act* t1_in, const Block* nxt, Act& y, Act& t1n) {
        t1n = Act();
        const lt_wshape w3[3] = {wshape(b.w[0]), wshape(b.w[1]), wshape(b.w[2])}, wd = wshape(b.wd);
        if (b.bottleneck && !b.has_ds && !t1_in && !nxt && lt_sel_bottleneck(dtype, dims(x).data(), w3, b.strides)) return bottleneck(x, b.w, b.bn, y);
        if (b.bottleneck && b.has_ds && !t1_in && !nxt && lt_sel_bottleneck_ds(dtype, dims(x).data(), w3, b.strides, &wd, b.sds))
            return bottleneck_ds(x, b.w, b.bn, b.wd, b.bnd, y);
        if (t1_in || nxt) {
            Act t1, t2;
            ConvOpt o;
            if (t1_in) t1 = *t1_in;
            else { o = ConvOpt(); o.bn = &b.bn[0]; o.relu = true; PL_TRY(conv(x, b.w[0], o, t1)); }
            o = ConvOpt(); o.bn = &b.bn[1]; o.relu = true; o.pad = 1; PL_TRY(conv(t1, b.w[1], o, t2));
            release(t1);
            const lt_wshape wr = nxt ? wshape(nxt->w[0]) : lt_wshape{};
            if (nxt && lt_sel_expand_reduce(dtype, dims(t2).data(), dims(x).data(), &w3[2], &wr)) {
                PL_TRY(expand_reduce(t2, x, b.w[2], b.bn[2], nxt->w[0], nxt->bn[0], y, t1n));
                release(t2);
                return LT_OK;
            }
            o = ConvOpt(); o.bn = &b.bn[2]; o.relu = true; o.residual = &x; PL_TRY(conv(t2, b.w[2], o, y));
            release(t2);
            return LT_OK;
        }
        if (b.bottleneck && b.has_ds) {
            const int Ho = (x.h - 1) / b.sds + 1, Wo = (x.w - 1) / b.sds + 1;
            const int t2s[5] = {x.n, 1, Ho, Wo, (int)b.w[2].s[1]};
            if (lt_sel_conv_cat2(dtype, t2s, &w3[2], dims(x).data(), &wd, b.sds)) {
                Act t1, t2; ConvOpt o;
                o.bn = &b.bn[0]; o.relu = true; o.stride = b.strides[0]; PL_TRY(conv(x, b.w[0], o, t1));
                o = ConvOpt(); o.bn = &b.bn[1]; o.relu = true; o.stride = b.strides[1]; o.pad = 1; PL_TRY(conv(t1, b.w[1], o, t2));
                release(t1);
                PL_TRY(conv_cat2(t2, b.w[2], b.bn[2], x, b.wd, b.bnd, b.sds, y));
                release(t2);
                return LT_OK;
            }
        }
        Act res = x; bool own_res = false;
        if (b.has_ds) { ConvOpt o; o.bn = &b.bnd; o.stride = b.sds; PL_TRY(conv(x, b.wd, o, res)); own_res = true; }
        Act cur = x;
        for (int i = 0; i < b.nconv; ++i) {
            const bool last = i + 1 == b.nconv;
            ConvOpt o; o.bn = &b.bn[i]; o.relu = true; o.stride = b.strides[i]; o.pad = (int)b.w[i].s[2] / 2; o.residual = last ? &res : nullptr;
            Act z; PL_TRY(conv(cur, b.w[i], o, z));
            if (cur.p != x.p) release(cur);
            cur = z;
        }
        if (own_res) release(res);
        y = cur;
        return LT_OK;
    }

    // GlobalAveragePoolingHead.record (pose_resnet.py:140-174): conv + BN (+ ReLU, which commutes with the max pool) -> pool, twice; global average; three linears
    // as 1x1 convolutions over an N-pixel map; sigmoid.  Returns Act [1,1,1,N,n] fp32
    int record_gap_head(const std::string& pre, const Act& x, Act& out) {
        WT w0, w4; const float *b0, *b4; BN bn1, bn5;
        PL_TRY(get(pre + ".features.0.weight", w0, 4)); PL_TRY(get_vec(pre + ".features.0.bias", (int)w0.s[0], &b0)); PL_TRY(get_bn(pre + ".features.1", (int)w0.s[0], bn1));
        PL_TRY(get(pre + ".features.4.weight", w4, 4)); PL_TRY(get_vec(pre + ".features.4.bias", (int)w4.s[0], &b4)); PL_TRY(get_bn(pre + ".features.5", (int)w4.s[0], bn5));
        Act y, p, g;
        ConvOpt o; o.bias = b0; o.bn = &bn1; o.pad = 1; o.relu = true; PL_TRY(conv(x, w0, o, y));
        PL_TRY(maxpool(y, 2, 2, 0, 2, p)); release(y);
        o = ConvOpt(); o.bias = b4; o.bn = &bn5; o.pad = 1; o.relu = true; PL_TRY(conv(p, w4, o, y)); release(p);
        PL_TRY(maxpool(y, 2, 2, 0, 2, p)); release(y);
        PL_TRY(global_avgpool(p, g)); release(p);
        Act cur = g;
        for (int i = 0; i < 3; ++i) {
            WT lw; const float* lb;
            PL_TRY(get(pre + ".head." + std::to_string(2 * i) + ".weight", lw, 2));
            PL_TRY(get_vec(pre + ".head." + std::to_string(2 * i) + ".bias", (int)lw.s[0], &lb));
            lw.nd = 4; lw.s[2] = 1; lw.s[3] = 1;          // Linear [out][in] read as a 1x1 convolution
            ConvOpt lo; lo.bias = lb; lo.relu = i < 2; lo.sigmoid = i == 2; lo.out_f32 = i == 2;
            Act z; PL_TRY(conv(cur, lw, lo, z)); release(cur);
            cur = z;
        }
        out = cur;
        return LT_OK;
    }

    // PoseResNet.record: stem, four stages, the optional confidence head conf_head ("backbone.alg_confidences" / "backbone.vol_confidences", or null), three
    // 4x4 / stride-2 deconvolutions (feats256) and, with want_heatmaps, final_layer (1x1 to J channels, fp32 output; dead in the volumetric path)
    int record_backbone(int N, int Hh, int W, int num_layers, bool caffe, const char* conf_head, bool want_heatmaps, Act& feats256, Act& conf, Act& heatmaps) {
        int nb[4]; bool bott;
        switch (num_layers) {
            case 18: bott = false; nb[0] = 2; nb[1] = 2; nb[2] = 2; nb[3] = 2; break;
            case 34: bott = false; nb[0] = 3; nb[1] = 4; nb[2] = 6; nb[3] = 3; break;
            case 50: bott = true; nb[0] = 3; nb[1] = 4; nb[2] = 6; nb[3] = 3; break;
            case 101: bott = true; nb[0] = 3; nb[1] = 4; nb[2] = 23; nb[3] = 3; break;
            case 152: bott = true; nb[0] = 3; nb[1] = 8; nb[2] = 36; nb[3] = 3; break;
            default: set_error("%s: num_layers %d (18 / 34 / 50 / 101 / 152)", who, num_layers); return LT_ERR_INVALID;
        }
        if (caffe) bott = true;          // the reference swaps in Bottleneck_CAFFE (expansion 4) at EVERY depth (pose_resnet.py:322-324)
        const int exp = bott ? 4 : 1;
        WT w1; BN bn1;
        PL_TRY(get("backbone.conv1.weight", w1, 4)); PL_TRY(get_bn("backbone.bn1", 64, bn1));
        Act y;
        const int32_t stem_in[5] = {N, 1, Hh, W, 8}, pool[3] = {3, 2, 1};
        const lt_wshape ws1 = wshape(w1);
        if (w1.s[1] == 3 && lt_sel_stem_pool(dtype, stem_in, &ws1, 2, 3, pool)) PL_TRY(stem_pool(N, Hh, W, w1, bn1, y));          // reads the 3-channel images
        else {
            // fp32 plans: the images go through lt_nchw_to_nhwc (pre op) into a 4-channel map, then conv1 + max pool
            const int cpad = 16 / es;
            Act xin; PL_TRY(alloc(N, 1, Hh, W, cpad, es, xin)); xin.pooled = false;
            const int dt = dtype; lt_plan* self = this; void* xp = xin.p;
            ops.push_back([=](hipStream_t s) { return lt_nchw_to_nhwc(dt, self->cur_images, xp, N, 3, Hh * W, cpad, s); });
            npre = 1;
            ConvOpt o; o.bn = &bn1; o.stride = 2; o.pad = 3; o.relu = true;
            Act c1; PL_TRY(conv(xin, w1, o, c1));
            PL_TRY(maxpool(c1, 3, 2, 1, 2, y)); release(c1);
        }
        int inplanes = 64;
        const int planes_of[4] = {64, 128, 256, 512};
        for (int li = 0; li < 4; ++li) {
            const int planes = planes_of[li], stride = li == 0 ? 1 : 2;
            std::vector<Block> blocks(nb[li]);
            for (int bi = 0; bi < nb[li]; ++bi) {
                const int st = bi == 0 ? stride : 1;
                const bool ds = bi == 0 && (st != 1 || inplanes != planes * exp);
                PL_TRY(load_block("backbone.layer" + std::to_string(li + 1) + "." + std::to_string(bi), bott, caffe, st, ds, blocks[bi]));
                inplanes = planes * exp;
            }
            Act t1; bool have_t1 = false;
            for (int bi = 0; bi < nb[li]; ++bi) {
                const Block& blk = blocks[bi];
                const Block* nxt = bi + 1 < nb[li] ? &blocks[bi + 1] : nullptr;
                // a run of identity bottleneck blocks whose seams lt_expand_reduce_fwd covers (ResNet layer3, bf16 plans): expand(i) + reduce(i + 1) in one launch
                const bool chain = nxt && blk.identity_bottleneck() && nxt->identity_bottleneck() && dtype == LT_BF16 && blk.w[2].s[0] == 1024 && blk.w[2].s[1] == 256 &&
                                   nxt->w[0].s[0] == 256 && nxt->w[0].s[1] == 1024;
                Act z, t1n;
                if (chain) PL_TRY(record_block(blk, y, have_t1 ? &t1 : nullptr, nxt, z, t1n));
                else if (have_t1) PL_TRY(record_block(blk, y, &t1, nullptr, z, t1n));
                else PL_TRY(record_block(blk, y, nullptr, nullptr, z, t1n));
                release(y);
                y = z; t1 = t1n; have_t1 = !t1n.null();
            }
        }
        conf = Act();
        if (conf_head) PL_TRY(record_gap_head(conf_head, y, conf));
        for (int i = 0; i < 3; ++i) {
            WT dw; BN dbn;
            PL_TRY(get("backbone.deconv_layers." + std::to_string(3 * i) + ".weight", dw, 4));
            PL_TRY(get_bn("backbone.deconv_layers." + std::to_string(3 * i + 1), (int)dw.s[1], dbn));
            const float* db = nullptr;
            if (has("backbone.deconv_layers." + std::to_string(3 * i) + ".bias")) PL_TRY(get_vec("backbone.deconv_layers." + std::to_string(3 * i) + ".bias", (int)dw.s[1], &db));
            LT_REQUIRE(dw.s[2] == 4 && dw.s[3] == 4, LT_ERR_UNSUPPORTED, "%s: only the 4x4 stride-2 deconvolution of the reference configs", who);
            ConvOpt o; o.bias = db; o.bn = &dbn; o.stride = 2; o.pad = 1; o.transposed = true; o.relu = true;
            Act z; PL_TRY(conv(y, dw, o, z)); release(y);
            y = z;
        }
        feats256 = y;
        heatmaps = Act();
        if (want_heatmaps) {
            WT fw; const float* fb;
            PL_TRY(get("backbone.final_layer.weight", fw, 4)); PL_TRY(get_vec("backbone.final_layer.bias", (int)fw.s[0], &fb));
            ConvOpt o; o.bias = fb; o.pad = fw.s[2] == 3 ? 1 : 0; o.out_f32 = true;          // pose_resnet.py: padding 1 for final_conv_kernel 3, else 0
            PL_TRY(conv(y, fw, o, heatmaps));
        }
        return LT_OK;
    }

    // V2V (mvn/models/v2v.py): Res3DBlock / Basic3DBlock / Pool3DBlock / Upsample3DBlock / EncoderDecorder / V2VModel.record
    struct C3 { WT w; const float* b = nullptr; BN bn; bool has_bn = false; };
    int load_c3(const std::string& conv, const std::string& bnname, bool transposed, C3& c) {
        PL_TRY(get(conv + ".weight", c.w, 5));
        const int cout = (int)(transposed ? c.w.s[1] : c.w.s[0]);
        PL_TRY(get_vec(conv + ".bias", cout, &c.b));
        if (!bnname.empty()) { PL_TRY(get_bn(bnname, cout, c.bn)); c.has_bn = true; }
        return LT_OK;
    }
    int res3d(const std::string& pre, const Act& x, Act& out) {
        C3 c0, c3, sk;
        PL_TRY(load_c3(pre + ".res_branch.0", pre + ".res_branch.1", false, c0));
        PL_TRY(load_c3(pre + ".res_branch.3", pre + ".res_branch.4", false, c3));
        const bool has_skip = has(pre + ".skip_con.0.weight");
        if (has_skip) PL_TRY(load_c3(pre + ".skip_con.0", pre + ".skip_con.1", false, sk));
        const int mid[5] = {x.n, x.d, x.h, x.w, (int)c0.w.s[0]};
        Act y, z;
        const lt_wshape w3 = wshape(c3.w), wsk = has_skip ? wshape(sk.w) : lt_wshape{};
        if (has_skip && lt_sel_conv_skip(dtype, mid, &w3, dims(x).data(), &wsk)) {
            ConvOpt o; o.bias = c0.b; o.bn = &c0.bn; o.pad = 1; o.relu = true; PL_TRY(conv(x, c0.w, o, y));
            o = ConvOpt(); o.bias = c3.b; o.bn = &c3.bn; o.pad = 1; o.relu = true; o.skip_x = &x; o.skip_w = &sk.w; o.skip_bias = sk.b; o.skip_bn = &sk.bn;
            PL_TRY(conv(y, c3.w, o, z)); release(y);
            out = z;
            return LT_OK;
        }
        Act skip = x; bool own = false;
        if (has_skip) { ConvOpt o; o.bias = sk.b; o.bn = &sk.bn; PL_TRY(conv(x, sk.w, o, skip)); own = true; }
        ConvOpt o; o.bias = c0.b; o.bn = &c0.bn; o.pad = 1; o.relu = true; PL_TRY(conv(x, c0.w, o, y));
        o = ConvOpt(); o.bias = c3.b; o.bn = &c3.bn; o.pad = 1; o.relu = true; o.residual = &skip; PL_TRY(conv(y, c3.w, o, z));
        release(y);
        if (own) release(skip);
        out = z;
        return LT_OK;
    }
    int record_v2v(const Act& vol_in, Act& logits_out) {
        const std::string V = "volume_net.";
        Act x = vol_in, y;
        {   // front_layers: Basic3DBlock(32, 16, 7), Res3DBlock(16, 32), Res3DBlock(32, 32) x 2
            C3 c; PL_TRY(load_c3(V + "front_layers.0.block.0", V + "front_layers.0.block.1", false, c));
            ConvOpt o; o.bias = c.b; o.bn = &c.bn; o.pad = (int)(c.w.s[2] - 1) / 2; o.relu = true;
            PL_TRY(conv(x, c.w, o, y)); release(x); x = y;
            for (int i = 1; i <= 3; ++i) { PL_TRY(res3d(V + "front_layers." + std::to_string(i), x, y)); release(x); x = y; }
        }
        {   // EncoderDecorder.record
            const std::string E = V + "encoder_decoder.";
            Act skips[5];
            for (int lvl = 1; lvl <= 5; ++lvl) {
                PL_TRY(res3d(E + "skip_res" + std::to_string(lvl), x, skips[lvl - 1]));
                Act p; PL_TRY(maxpool(x, 2, 2, 0, 3, p)); release(x);
                PL_TRY(res3d(E + "encoder_res" + std::to_string(lvl), p, x)); release(p);
            }
            PL_TRY(res3d(E + "mid_res", x, y)); release(x); x = y;
            for (int lvl = 5; lvl >= 1; --lvl) {
                PL_TRY(res3d(E + "decoder_res" + std::to_string(lvl), x, y)); release(x);
                C3 u; PL_TRY(load_c3(E + "decoder_upsample" + std::to_string(lvl) + ".block.0", E + "decoder_upsample" + std::to_string(lvl) + ".block.1", true, u));
                ConvOpt o; o.bias = u.b; o.bn = &u.bn; o.stride = 2; o.pad = 0; o.transposed = true; o.relu_pre = true; o.residual = &skips[lvl - 1];
                PL_TRY(conv(y, u.w, o, x));          // relu(BN(deconv y)) + skip: the decoder's skip add rides in the same epilogue (v2v.py:121-136)
                release(y); release(skips[lvl - 1]);
            }
        }
        PL_TRY(res3d(V + "back_layers.0", x, y)); release(x); x = y;
        C3 t1, t2, ol;
        PL_TRY(load_c3(V + "back_layers.1.block.0", V + "back_layers.1.block.1", false, t1));
        PL_TRY(load_c3(V + "back_layers.2.block.0", V + "back_layers.2.block.1", false, t2));
        PL_TRY(load_c3(V + "output_layer", "", false, ol));
        std::vector<PwLayer> chain = {{t1.w, t1.b, &t1.bn, true}, {t2.w, t2.b, &t2.bn, true}, {ol.w, ol.b, nullptr, false}};
        const lt_wshape wchain[3] = {wshape(t1.w), wshape(t2.w), wshape(ol.w)};
        if (lt_sel_pwchain(dtype, dims(x).data(), 3, wchain)) {          // the pointwise tail (back_layers[1:] + output_layer) as ONE pass, (N, J, V, V, V) planar fp32 logits
            PL_TRY(pwchain(x, chain, logits_out)); release(x);
            return LT_OK;
        }
        for (C3* c : {&t1, &t2}) { ConvOpt o; o.bias = c->b; o.bn = &c->bn; o.relu = true; PL_TRY(conv(x, c->w, o, y)); release(x); x = y; }
        ConvOpt o; o.bias = ol.b; o.out_f32 = true;
        PL_TRY(conv(x, ol.w, o, logits_out)); release(x);
        return LT_OK;
    }

    // VolumetricTriangulationNet._build_plan
    int build() {
        const int F = cfg.B, NV = cfg.NV, V = cfg.volume_size, J = cfg.num_joints;
        const int B = cuboids();          // the gather, V2V and the tail: per cuboid; the backbone and the features: per frame
        Act f256, no_hm;
        const bool conf_head = cfg.aggregation == LT_AGG_CONF || cfg.aggregation == LT_AGG_CONF_NORM;
        const int NI = images();
        PL_TRY(record_backbone(NI, cfg.H, cfg.W, cfg.num_layers, cfg.style_caffe != 0, conf_head ? "backbone.vol_confidences" : nullptr, false, f256, volc, no_hm));
        WT pw; const float* pb;
        PL_TRY(get("process_features.0.weight", pw, 4)); PL_TRY(get_vec("process_features.0.bias", (int)pw.s[0], &pb));
        LT_REQUIRE(pw.s[0] == 32, LT_ERR_UNSUPPORTED, "lt_plan_create_vol: process_features has %d output channels (32)", (int)pw.s[0]);
        ConvOpt o; o.bias = pb;
        PL_TRY(conv(f256, pw, o, feats)); release(f256);
        feats.pooled = false;
        hm_h = feats.h; hm_w = feats.w;
        // geometry block + its pinned staging ring
        o_pos = (size_t)NI * 12; o_cen = o_pos + 3 * B; o_rot = o_pos + 6 * B; o_fof = o_pos + 15 * (size_t)B;
        o_vb = o_fof;          // ragged plans (never multi): the B + 1 offsets behind the rotations
        n_geo = o_fof + (P ? (size_t)P : 0) + (T ? (size_t)B + 1 : 0);
        void* g; PL_TRY(dev_alloc(n_geo * 4, &g)); geo_dev = (float*)g;
        PL_TRY(geo.alloc(n_geo * 4));
        void* c; PL_TRY(dev_alloc((size_t)B * V * V * V * 3 * 4, &c)); coords = (float*)c;
        PL_TRY(alloc(B, V, V, V, 32, es, vol));
        const float step = (float)(cfg.cuboid_side / (double)(V - 1));          // float(np.float32(side / (V - 1))): the fp64 quotient rounded once
        {
            // everything of the descriptor that is fixed when the plan is built; the grid form, the variant by the pointers set when the op runs
            lt_unproject_desc d0 = {};
            d0.dtype = dtype; d0.feats = feats.p; d0.step = step; d0.cmu_transfer = cfg.transfer_cmu_to_human36m ? 1 : 0; d0.coords_out = coords;
            d0.conf = volc.null() ? nullptr : (const float*)volc.p;
            d0.F = F; d0.T = T; d0.B = B; d0.NV = NV; d0.C = 32; d0.h = hm_h; d0.w = hm_w; d0.v0 = d0.v1 = d0.v2 = V; d0.agg = cfg.aggregation;
            const size_t op = o_pos, oc = o_cen, orr = o_rot, of = o_fof; lt_plan* self = this; const bool multi = P > 0; void* vp = vol.p;
            // the block's address is read when the op runs: a masked plan (lt_plan_set_view_mask, before the first forward) has moved it to a block with the mask behind
            ops.push_back([=](hipStream_t s) {
                const float* gp = self->geo_dev;
                lt_unproject_desc d = d0;
                d.proj = gp; d.pos = gp + op; d.center = gp + oc; d.rot = gp + orr;
                d.view_mask = self->masked ? self->mask_dev : nullptr;
                if (d.T) d.view_base = (const int32_t*)(gp + of);
                else if (multi) d.frame_of = (const int32_t*)(gp + of);
                return lt_unproject_desc_fwd(&d, vp, s);
            });
        }
        PL_TRY(record_v2v(vol, logits));
        void* k; PL_TRY(dev_alloc((size_t)B * J * 3 * 4, &k)); kp = (float*)k;
        PL_TRY(dev_alloc((size_t)B * J * V * V * V * 4, &k)); probs = (float*)k;
        const long long nvox = (long long)V * V * V;
        const size_t wsb = lt_softargmax3d_workspace(B, J, nvox);
        PL_TRY(dev_alloc(wsb ? wsb : 16, &sa_ws));
        {   // tail op 1: the RETURNED features (B, NV, 32, h, w) fp32, skipped when the caller did not ask for them
            const int dt = dtype, h = hm_h, w = hm_w; const void* fp = feats.p; lt_plan* self = this;
            ops.push_back([=](hipStream_t s) { return self->out_feats ? lt_nhwc_to_nchw_f32(dt, fp, self->out_feats, NI, 32, h * w, 32, s) : LT_OK; });
        }
        {   // tail op 2: soft-argmax straight into the caller's tensors
            const float mult = (float)cfg.volume_multiplier; const int sm = cfg.volume_softmax ? 1 : 0, cl = logits.planar ? 0 : 1;
            const float* lp = (const float*)logits.p; const float* cp = coords; void* ws = sa_ws; lt_plan* self = this;
            float* kpd = kp; float* prd = probs;
            ops.push_back([=](hipStream_t s) {
                if (self->ks_stats)
                    return lt_softargmax3d_stats_fwd(lp, cp, mult, sm, cl, J, self->out_kp ? self->out_kp : kpd, self->out_probs ? self->out_probs : prd, self->ks_stats,
                                                     self->ks_index, B, J, nvox, self->ks_ws, s);
                return lt_softargmax3d_fwd(lp, cp, mult, sm, cl, J, self->out_kp ? self->out_kp : kpd, self->out_probs ? self->out_probs : prd, B, J, nvox, ws, s);
            });
        }
        ntail = 2;
        return LT_OK;
    }

    // AlgebraicTriangulationNet._build_plan / RANSACTriangulationNet._build_plan.  Captured: the backbone with final_layer (and the alg_confidences head),
    // then the heatmaps to NCHW (ALG: lt_nhwc_to_nchw_f32; RANSAC: lt_heatmap_argmax_nchw_f32, which also writes the int64 argmax keypoints).  Tail, eager on
    // every call because it reads the caller's proj and writes the caller's outputs: ALG lt_softargmax2d_fwd + lt_alg_tail_fwd, RANSAC lt_triangulate_ransac.
    int build_alg() {
        const lt_alg_plan_config& c = acfg;
        const int B = c.B, NV = c.NV, N = images(), J = c.num_joints, Hh = c.H, W = c.W;
        const bool ransac = c.model == LT_MODEL_RANSAC;
        Act f256, hm;
        PL_TRY(record_backbone(N, Hh, W, c.num_layers, c.style_caffe != 0, !ransac && c.use_confidences ? "backbone.alg_confidences" : nullptr, true, f256, algc, hm));
        release(f256);
        LT_REQUIRE(hm.c == J, LT_ERR_INVALID, "%s: backbone.final_layer has %d output channels, num_joints is %d", who, hm.c, J);
        hm_h = hm.h; hm_w = hm.w;
        const int h = hm_h, w = hm_w;
        void* q;
        PL_TRY(dev_alloc((size_t)N * J * h * w * 4, &q)); hm_nchw = (float*)q;
        const float* hp = (const float*)hm.p; float* hn = hm_nchw; lt_plan* self = this;
        if (ransac) {
            PL_TRY(dev_alloc((size_t)N * J * 2 * 8, &q)); kp_i64 = (int64_t*)q;
            const int ld = hm.c; int64_t* kpp = kp_i64;
            ops.push_back([=](hipStream_t s) { return lt_heatmap_argmax_nchw_f32(hp, ld, hn, nullptr, kpp, N, J, h, w, Hh, W, s); });
            // tail: every view pair as a hypothesis (pairs = NULL), as RANSACTriangulationNet.forward
            const double eps = c.reprojection_error_epsilon; const int direct = c.direct_optimization ? 1 : 0;
            ops.push_back([=](hipStream_t s) { return lt_triangulate_ransac(self->cur_proj, kpp, nullptr, 0, eps, direct, self->out_kp, nullptr, B, NV, J, s); });
            ntail = 1;
            return LT_OK;
        }
        ops.push_back([=](hipStream_t s) { return lt_nhwc_to_nchw_f32(LT_F32, hp, hn, N, J, h * w, J, s); });
        PL_TRY(dev_alloc((size_t)N * J * 2 * 4, &q)); kp_hm = (float*)q;
        PL_TRY(dev_alloc((size_t)N * J * h * w * 4, &q)); probs = (float*)q;
        {   // tail op 1: integrate_tensor_2d, the normalised heatmaps straight into the caller's tensor
            const float mult = (float)c.heatmap_multiplier; const int sm = c.heatmap_softmax ? 1 : 0; float* kh = kp_hm; float* pr = probs;
            ops.push_back([=](hipStream_t s) {
                if (self->aks_stats2d)
                    return lt_softargmax2d_stats_fwd(hn, mult, sm, kh, self->out_hm ? self->out_hm : pr, self->aks_stats2d, self->aks_index, N * J, h, w, s);
                return lt_softargmax2d_fwd(hn, mult, sm, kh, self->out_hm ? self->out_hm : pr, N * J, h, w, s);
            });
        }
        {   // tail op 2: confidences normalised over the views, keypoints to image pixels, the DLT (triangulation.py:166-193)
            const float sx = (float)((double)W / (double)w), sy = (float)((double)Hh / (double)h);          // torch.tensor([W / w, H / h], float32)
            const float* kh = kp_hm; const float* cp = algc.null() ? nullptr : (const float*)algc.p; const int ldc = algc.null() ? J : algc.c;
            const int rT = T;
            if (rT) {          // the offsets' device block and its pinned ring (stage_view_base)
                PL_TRY(avb.alloc(((size_t)B + 1) * 4));
                PL_TRY(dev_alloc(((size_t)B + 1) * 4, &q)); vb_dev = (int32_t*)q;
            }
            ops.push_back([=](hipStream_t s) {
                if (rT)
                    return lt_alg_tail_ragged_fwd(kh, cp, ldc, self->cur_proj, sx, sy, self->vb_dev, (float*)self->out_kp2d, self->out_conf, self->out_kp, B, rT, NV, J, s);
                if (self->aks_stats2d)
                    return lt_alg_tail_stats_fwd(kh, cp, ldc, self->cur_proj, sx, sy, self->masked ? self->mask_dev : nullptr, self->aks_stats2d, (float*)self->out_kp2d,
                                                 self->out_conf, self->out_kp, self->aks_cov2d, self->aks_reproj, self->aks_cov3d, B, NV, J, s);
                if (self->masked)
                    return lt_alg_tail_masked_fwd(kh, cp, ldc, self->cur_proj, sx, sy, self->mask_dev, (float*)self->out_kp2d, self->out_conf, self->out_kp, B, NV, J, s);
                return lt_alg_tail_fwd(kh, cp, ldc, self->cur_proj, sx, sy, (float*)self->out_kp2d, self->out_conf, self->out_kp, B, NV, J, s);
            });
        }
        ntail = 2;
        return LT_OK;
    }

    // stream == NULL with use_graph: the plan's own stream, ordered behind what the default stream has queued so far (enter) and in front of what it gets next (leave)
    int enter(hipStream_t& st, bool& detour) {
        detour = st == nullptr && cfg.use_graph;
        if (!detour) return LT_OK;
        if (!own_stream) {
            PL_HIP(hipStreamCreateWithFlags(&own_stream, hipStreamNonBlocking));
            for (int i = 0; i < 2; ++i) PL_HIP(hipEventCreateWithFlags(&own_ev[i], hipEventDisableTiming));
        }
        PL_HIP(hipEventRecord(own_ev[0], nullptr));
        PL_HIP(hipStreamWaitEvent(own_stream, own_ev[0], 0));
        st = own_stream;
        return LT_OK;
    }
    int leave(hipStream_t st, bool detour) {
        if (!detour) return LT_OK;
        PL_HIP(hipEventRecord(own_ev[1], st));
        PL_HIP(hipStreamWaitEvent(nullptr, own_ev[1], 0));
        return LT_OK;
    }

    // ---- host geometry in fp64 like the reference (triangulation.py:272-296): Camera.update_after_resize to the heatmap resolution, projection = K [R | t];
    // cuboid position = base - side / 2; rotation about the vertical axis (identity in eval mode); one pinned block, one H2D copy.  base_points_host NULL
    // (cascade plans): the pos / center ranges are left for lt_cuboid_from_keypoints, which the caller enqueues behind the copy.  proj_img (cascade plans,
    // its block of this forward): K [R | t] at IMAGE resolution rounded to fp32, the algebraic stage's proj_matricies_batch.
    // cuboid_frame (multi plans, checked by the caller): the P frame indices behind the rotations; base_points_host and rot_host are per cuboid there.
    int stage_geometry(const double* K_host, const double* R_host, const double* t_host, const double* base_points_host, const double* rot_host, hipStream_t st,
                       float* pi = nullptr, const int32_t* cuboid_frame = nullptr, const int32_t* view_counts = nullptr) {
        const int B = cfg.B, NV = cfg.NV, NC = cuboids(), NI = images();
        void* blk; PL_TRY(geo.acquire(&blk));
        float* gh = (float*)blk;
        const double sx = (double)hm_w / (double)cfg.W, sy = (double)hm_h / (double)cfg.H;
        for (int i = 0; i < NI; ++i) {
            double K[9];
            for (int k = 0; k < 9; ++k) K[k] = K_host[(size_t)i * 9 + k];
            const double* R = R_host + (size_t)i * 9; const double* t = t_host + (size_t)i * 3;
            if (pi)
                for (int r = 0; r < 3; ++r)
                    for (int c = 0; c < 4; ++c) {
                        double acc = 0.0;
                        for (int k = 0; k < 3; ++k) acc += K[r * 3 + k] * (c < 3 ? R[k * 3 + c] : t[k]);
                        pi[(size_t)i * 12 + r * 4 + c] = (float)acc;
                    }
            K[0] *= sx; K[4] *= sy; K[2] *= sx; K[5] *= sy;
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 4; ++c) {
                    double acc = 0.0;
                    for (int k = 0; k < 3; ++k) acc += K[r * 3 + k] * (c < 3 ? R[k * 3 + c] : t[k]);
                    gh[(size_t)i * 12 + r * 4 + c] = (float)acc;
                }
        }
        const double half = (double)cfg.cuboid_side / 2.0;
        for (int b = 0; b < NC; ++b) {
            for (int k = 0; k < 3 && base_points_host; ++k) {
                gh[o_pos + 3 * b + k] = (float)(base_points_host[3 * b + k] - half);
                gh[o_cen + 3 * b + k] = (float)base_points_host[3 * b + k];
            }
            for (int k = 0; k < 9; ++k) gh[o_rot + 9 * b + k] = rot_host ? (float)rot_host[9 * b + k] : ((k == 0 || k == 4 || k == 8) ? 1.f : 0.f);
        }
        if (cuboid_frame) memcpy(gh + o_fof, cuboid_frame, (size_t)NC * 4);
        if (view_counts) {          // ragged plans (counts checked by the caller): the exclusive prefix sum, B + 1 int32
            int32_t* vb = (int32_t*)(gh + o_vb);
            vb[0] = 0;
            for (int b = 0; b < B; ++b) vb[b + 1] = vb[b] + view_counts[b];
        }
        if (masked) memcpy((uint8_t*)(gh + o_mask), mask_cur.data(), (size_t)B * NV);          // rides in the same block: one copy
        PL_HIP(hipMemcpyAsync(geo_dev, gh, n_geo * 4, hipMemcpyHostToDevice, st));
        return geo.commit(st);
    }

    // volumetric plans, first lt_plan_set_view_mask: the geometry block and its pinned ring again, with B*NV mask bytes (whole words) behind the floats.
    // Everything new is allocated first and the plan is changed only when all of it exists: a failure leaves the plan as it was (unmasked, usable).  The
    // old block and ring are freed -- no forward has run, nothing is queued on them -- so lt_plan_info reports what the plan holds.
    int grow_geometry_for_mask() {
        const size_t n_new = n_geo + ((size_t)cfg.B * cfg.NV + 3) / 4;
        void* g = nullptr; StagingRing ring;          // frees what it got on a failure, the old ring after the swap
        auto acquire = [&]() -> int {
            PL_HIP(hipMalloc(&g, n_new * 4));
            PL_HIP(hipMemset(g, 0, n_new * 4));
            return ring.alloc(n_new * 4);
        };
        const int rc = acquire();
        if (rc != LT_OK) {
            if (g) (void)hipFree(g);
            return rc;
        }
        for (size_t i = 0; i < allocs.size(); ++i)
            if (allocs[i] == (void*)geo_dev) { allocs.erase(allocs.begin() + (long)i); break; }
        (void)hipFree(geo_dev);
        bytes_alloc += (n_new - n_geo) * 4;
        allocs.push_back(g);
        geo.swap(ring);
        geo_dev = (float*)g; o_mask = n_geo; n_geo = n_new;
        mask_dev = (const uint8_t*)(geo_dev + o_mask);
        return LT_OK;
    }
    // algebraic plans, first lt_plan_set_view_mask: the mask's device block and its pinned ring
    int alloc_alg_mask() {
        const size_t n = (size_t)cfg.B * cfg.NV;
        PL_TRY(amask.alloc(n));
        void* q; PL_TRY(dev_alloc(n, &q)); amask_dev = (uint8_t*)q; mask_dev = amask_dev;
        return LT_OK;
    }
    // ragged algebraic plans, per forward: the offsets of the counts (checked by the caller) to the device through their ring
    int stage_view_base(const int32_t* view_counts, hipStream_t st) {
        void* blk; PL_TRY(avb.acquire(&blk));
        int32_t* vb = (int32_t*)blk;
        vb[0] = 0;
        for (int b = 0; b < cfg.B; ++b) vb[b + 1] = vb[b] + view_counts[b];
        PL_HIP(hipMemcpyAsync(vb_dev, vb, ((size_t)cfg.B + 1) * 4, hipMemcpyHostToDevice, st));
        return avb.commit(st);
    }
    // algebraic plans, per forward: a changed mask to the device through the ring
    int stage_alg_mask(hipStream_t st) {
        if (!masked || !amask_dev || !mask_dirty) return LT_OK;
        void* blk; PL_TRY(amask.acquire(&blk));
        memcpy(blk, mask_cur.data(), mask_cur.size());
        PL_HIP(hipMemcpyAsync(amask_dev, blk, mask_cur.size(), hipMemcpyHostToDevice, st));
        PL_TRY(amask.commit(st));
        mask_dirty = false;
        return LT_OK;
    }

    int run(hipStream_t st) {
        const int nops = (int)ops.size();
        for (int i = 0; i < npre; ++i) PL_TRY(ops[i](st));
        if (cfg.use_graph && !captured) {
            // warm-up launch outside capture (sets function attributes, loads code objects), then capture the middle section once
            for (int i = npre; i < nops - ntail; ++i) PL_TRY(ops[i](st));
            PL_HIP(hipStreamSynchronize(st));
            PL_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
            int rc = LT_OK;
            for (int i = npre; i < nops - ntail && rc == LT_OK; ++i) rc = ops[i](st);
            hipGraph_t g = nullptr;
            const hipError_t e = hipStreamEndCapture(st, &g);
            if (rc != LT_OK) { if (g) (void)hipGraphDestroy(g); return rc; }
            if (e != hipSuccess) { set_error("hipStreamEndCapture: %s", hipGetErrorString(e)); return LT_ERR_LAUNCH; }
            const hipError_t e2 = hipGraphInstantiate(&graph, g, nullptr, nullptr, 0);
            (void)hipGraphDestroy(g);
            if (e2 != hipSuccess) { set_error("hipGraphInstantiate: %s", hipGetErrorString(e2)); return LT_ERR_LAUNCH; }
            captured = true;
        } else if (cfg.use_graph) {
            PL_HIP(hipGraphLaunch(graph, st));
        } else {
            for (int i = npre; i < nops - ntail; ++i) PL_TRY(ops[i](st));
        }
        for (int i = nops - ntail; i < nops; ++i) PL_TRY(ops[i](st));
        return LT_OK;
    }
};

namespace {
// the caller's state dict by name, "module." stripped (DataParallel checkpoints, train.py:408-410); false (and the error set) for an unnamed entry
bool load_state_dict(lt_plan* p, const lt_named_tensor* weights, int32_t nweights) {
    for (int i = 0; i < nweights; ++i) {
        if (!weights[i].name) { set_error("%s: weight %d has no name", p->who, i); return false; }
        std::string n = weights[i].name;
        if (n.rfind("module.", 0) == 0) n = n.substr(7);
        p->sd[n] = &weights[i];
    }
    return true;
}
}  // namespace

namespace {
// the configuration checks of the create calls, before any device call; who: the entry point, for the message
int check_vol_config(const lt_vol_plan_config* cfg, const char* who) {
    LT_REQUIRE(cfg->dtype == LT_F32 || cfg->dtype == LT_BF16, LT_ERR_INVALID, "%s: dtype %d", who, cfg->dtype);
    LT_REQUIRE(cfg->B >= 1 && cfg->NV >= 1 && cfg->H >= 32 && cfg->W >= 32 && cfg->volume_size >= 2 && cfg->num_joints >= 1, LT_ERR_INVALID, "%s: bad shape", who);
    LT_REQUIRE(cfg->aggregation >= LT_AGG_SUM && cfg->aggregation <= LT_AGG_CONF_NORM, LT_ERR_INVALID, "%s: aggregation %d", who, cfg->aggregation);
    return LT_OK;
}
int check_alg_config(const lt_alg_plan_config& c, const char* who) {
    LT_REQUIRE(c.model == LT_MODEL_ALG || c.model == LT_MODEL_RANSAC, LT_ERR_INVALID, "%s: model %d (LT_MODEL_ALG | LT_MODEL_RANSAC)", who, c.model);
    LT_REQUIRE(c.dtype == LT_F32 || c.dtype == LT_BF16, LT_ERR_INVALID, "%s: dtype %d", who, c.dtype);
    LT_REQUIRE(c.B >= 1 && c.NV >= 2 && c.H >= 32 && c.W >= 32 && c.num_joints >= 1, LT_ERR_INVALID,
               "%s: bad shape (B %d, NV %d, H %d, W %d, num_joints %d; at least 2 views to triangulate, 32 x 32 images)", who, c.B, c.NV, c.H, c.W, c.num_joints);
    if (c.model == LT_MODEL_RANSAC) {
        LT_REQUIRE(c.num_joints <= 32, LT_ERR_INVALID, "%s: num_joints %d > 32 (RANSAC's heatmap argmax)", who, c.num_joints);
        LT_REQUIRE(c.NV <= 32, LT_ERR_INVALID, "%s: NV %d views (RANSAC: 2 <= NV <= 32)", who, c.NV);
    }
    return LT_OK;
}

// a checked configuration + a state dict -> a recorded plan
int make_vol_plan(const lt_vol_plan_config* cfg, const lt_named_tensor* weights, int32_t nweights, const char* who, lt_plan** plan_out, int P = 0, int T = 0) {
    lt_plan* p = new lt_plan();
    p->who = who; p->P = P; p->T = T;
    p->cfg = *cfg;
    p->dtype = cfg->dtype; p->es = cfg->dtype == LT_F32 ? 4 : 2;
    if (!load_state_dict(p, weights, nweights)) { delete p; return LT_ERR_INVALID; }
    const int rc = p->build();
    if (rc != LT_OK) { delete p; return rc; }
    p->sd.clear();          // the caller's host arrays are not referenced after this call
    *plan_out = p;
    return LT_OK;
}
// the heads an algebraic / RANSAC model reads besides the backbone, named before any device work
int check_alg_heads(const lt_alg_plan_config& c, const lt_named_tensor* weights, int32_t nweights, const char* who) {
    lt_plan probe;
    probe.who = who;
    if (!load_state_dict(&probe, weights, nweights)) return LT_ERR_INVALID;
    std::vector<std::string> heads = {"backbone.final_layer.weight", "backbone.final_layer.bias"};
    if (c.model == LT_MODEL_ALG && c.use_confidences) heads.push_back("backbone.alg_confidences.head.4.weight");
    for (const std::string& k : heads) LT_REQUIRE(probe.has(k), LT_ERR_INVALID, "%s: state dict has no '%s'", who, k.c_str());
    return LT_OK;
}
int make_alg_plan(const lt_alg_plan_config& c, const lt_named_tensor* weights, int32_t nweights, const char* who, lt_plan** plan_out, int T = 0) {
    PL_TRY(check_alg_heads(c, weights, nweights, who));
    lt_plan* p = new lt_plan();
    p->who = who; p->T = T;
    p->model = c.model; p->acfg = c;
    memset(&p->cfg, 0, sizeof(p->cfg));
    p->cfg.dtype = c.dtype; p->cfg.num_layers = c.num_layers; p->cfg.style_caffe = c.style_caffe; p->cfg.num_joints = c.num_joints;
    p->cfg.B = c.B; p->cfg.NV = c.NV; p->cfg.H = c.H; p->cfg.W = c.W; p->cfg.use_graph = c.use_graph;
    p->dtype = c.dtype; p->es = c.dtype == LT_F32 ? 4 : 2;
    if (!load_state_dict(p, weights, nweights)) { delete p; return LT_ERR_INVALID; }
    const int rc = p->build_alg();
    if (rc != LT_OK) { delete p; return rc; }
    p->sd.clear();          // the caller's host arrays are not referenced after this call
    *plan_out = p;
    return LT_OK;
}
const char* plan_kind_name(const lt_plan* p) {
    if (p->T) return p->model == 0 ? "a ragged volumetric plan of lt_plan_create_vol_ragged" : "a ragged algebraic plan of lt_plan_create_alg_ragged";
    return p->model == 0 ? (p->P ? "a multi-cuboid plan of lt_plan_create_vol_multi" : "a volumetric plan of lt_plan_create_vol") : p->model == MODEL_CASCADE ? "a cascade plan of lt_plan_create_cascade"
           : p->model == LT_MODEL_RANSAC ? "an LT_MODEL_RANSAC plan of lt_plan_create_alg" : "an LT_MODEL_ALG plan of lt_plan_create_alg";
}
}  // namespace

namespace {
// the checked forward of a volumetric plan; cuboid_frame: the multi plans' assignment (base_points_host and rot_host per cuboid there), else null
int forward_vol_any(lt_plan* p, const char* who, const float* images, const double* K_host, const double* R_host, const double* t_host, const int32_t* cuboid_frame,
                    const double* base_points_host, const double* rot_host, float* keypoints_3d, float* volumes, float* features, float* coord_volumes,
                    float* vol_confidences, void* stream, const int32_t* view_counts = nullptr) {
    hipStream_t st = (hipStream_t)stream;
    bool detour;
    PL_TRY(p->enter(st, detour));
    const int V = p->cfg.volume_size;
    p->ran = true;
    PL_TRY(p->stage_geometry(K_host, R_host, t_host, base_points_host, rot_host, st, nullptr, cuboid_frame, view_counts));
    p->cur_images = images; p->out_kp = keypoints_3d; p->out_probs = volumes; p->out_feats = features;
    PL_TRY(p->run(st));
    if (coord_volumes) PL_HIP(hipMemcpyAsync(coord_volumes, p->coords, (size_t)p->cuboids() * V * V * V * 3 * 4, hipMemcpyDeviceToDevice, st));
    if (vol_confidences) {
        LT_REQUIRE(!p->volc.null(), LT_ERR_INVALID, "%s: vol_confidences asked of a plan without the confidence head (aggregation %d)", who, p->cfg.aggregation);
        PL_HIP(hipMemcpyAsync(vol_confidences, p->volc.p, (size_t)p->images() * 32 * 4, hipMemcpyDeviceToDevice, st));          // RAW sigmoid outputs; 'conf_norm' divides by their sum over views
    }
    PL_TRY(p->leave(st, detour));
    return LT_OK;
}
}  // namespace

extern "C" int lt_plan_create_vol(const lt_vol_plan_config* cfg, const lt_named_tensor* weights, int32_t nweights, lt_plan** plan_out) {
    LT_REQUIRE(cfg && weights && plan_out && nweights > 0, LT_ERR_INVALID, "lt_plan_create_vol: null argument");
    PL_TRY(check_vol_config(cfg, "lt_plan_create_vol"));
    *plan_out = nullptr;
    return make_vol_plan(cfg, weights, nweights, "lt_plan_create_vol", plan_out);
}

extern "C" int lt_plan_forward_vol(lt_plan* p, const float* images, const double* K_host, const double* R_host, const double* t_host, const double* base_points_host,
                                   const double* rot_host, float* keypoints_3d, float* volumes, float* features, float* coord_volumes, float* vol_confidences,
                                   void* stream) {
    LT_REQUIRE(p, LT_ERR_INVALID, "lt_plan_forward_vol: null argument");
    LT_REQUIRE(p->model == 0, LT_ERR_INVALID, "lt_plan_forward_vol: the plan is %s; run it with %s", plan_kind_name(p),
               p->model == MODEL_CASCADE ? "lt_plan_forward_cascade" : "lt_plan_forward_alg");
    LT_REQUIRE(!p->P, LT_ERR_INVALID, "lt_plan_forward_vol: the plan is %s; run it with lt_plan_forward_vol_multi", plan_kind_name(p));
    LT_REQUIRE(!p->T, LT_ERR_INVALID, "lt_plan_forward_vol: the plan is %s; run it with lt_plan_forward_vol_ragged", plan_kind_name(p));
    LT_REQUIRE(images && K_host && R_host && t_host && base_points_host && keypoints_3d, LT_ERR_INVALID, "lt_plan_forward_vol: null argument");
    return forward_vol_any(p, "lt_plan_forward_vol", images, K_host, R_host, t_host, nullptr, base_points_host, rot_host, keypoints_3d, volumes, features,
                           coord_volumes, vol_confidences, stream);
}

extern "C" int lt_plan_create_vol_multi(const lt_vol_plan_config* cfg, int32_t P, const lt_named_tensor* weights, int32_t nweights, lt_plan** plan_out) {
    const char* who = "lt_plan_create_vol_multi";
    LT_REQUIRE(cfg && weights && plan_out && nweights > 0, LT_ERR_INVALID, "%s: null argument", who);
    PL_TRY(check_vol_config(cfg, who));
    LT_REQUIRE(P >= 1, LT_ERR_INVALID, "%s: P %d cuboids (at least 1)", who, P);
    *plan_out = nullptr;
    return make_vol_plan(cfg, weights, nweights, who, plan_out, P);
}

extern "C" int lt_plan_forward_vol_multi(lt_plan* p, const float* images, const double* K_host, const double* R_host, const double* t_host,
                                         const int32_t* cuboid_frame_host, const double* base_points_host, const double* rot_host, float* keypoints_3d,
                                         float* volumes, float* features, float* coord_volumes, float* vol_confidences, void* stream) {
    const char* who = "lt_plan_forward_vol_multi";
    LT_REQUIRE(p, LT_ERR_INVALID, "%s: null argument", who);
    LT_REQUIRE(p->model == 0 && p->P, LT_ERR_INVALID, "%s: the plan is %s; run it with %s", who, plan_kind_name(p),
               p->model == 0 ? (p->T ? "lt_plan_forward_vol_ragged" : "lt_plan_forward_vol") : p->model == MODEL_CASCADE ? "lt_plan_forward_cascade" : "lt_plan_forward_alg");
    LT_REQUIRE(images && K_host && R_host && t_host && cuboid_frame_host && base_points_host && keypoints_3d, LT_ERR_INVALID,
               "%s: null argument (images, K, R, t, cuboid_frame, base_points and keypoints_3d are required)", who);
    for (int i = 0; i < p->P; ++i)
        LT_REQUIRE(cuboid_frame_host[i] >= 0 && cuboid_frame_host[i] < p->cfg.B, LT_ERR_INVALID, "%s: cuboid_frame[%d] = %d, the plan has frames 0 .. %d", who, i,
                   cuboid_frame_host[i], p->cfg.B - 1);
    return forward_vol_any(p, who, images, K_host, R_host, t_host, cuboid_frame_host, base_points_host, rot_host, keypoints_3d, volumes, features, coord_volumes,
                           vol_confidences, stream);
}

namespace {
// the counts of a ragged forward against the plan: each in [min_views, NVcap], summing to T; the message names the first bad sample
int check_view_counts(const lt_plan* p, const char* who, const int32_t* view_counts, int min_views) {
    long long sum = 0;
    for (int b = 0; b < p->cfg.B; ++b) {
        LT_REQUIRE(view_counts[b] >= min_views && view_counts[b] <= p->cfg.NV, LT_ERR_INVALID, "%s: sample %d has %d view%s, the plan takes %d to %d (NVcap)", who, b,
                   view_counts[b], view_counts[b] == 1 ? "" : "s", min_views, p->cfg.NV);
        sum += view_counts[b];
    }
    LT_REQUIRE(sum == p->T, LT_ERR_INVALID, "%s: view_counts sums to %lld views over %d samples, the plan holds %d images", who, sum, p->cfg.B, p->T);
    return LT_OK;
}
// T images over B samples of at most NVcap (and at least min_views) views each
int check_ragged_shape(const char* who, int B, int NVcap, int T, int min_views) {
    LT_REQUIRE(NVcap >= 1 && NVcap <= 32, LT_ERR_INVALID, "%s: NV %d (NVcap of a ragged plan: 1 .. 32)", who, NVcap);
    LT_REQUIRE(T >= 1 && (long long)T >= (long long)min_views * B && (long long)T <= (long long)B * NVcap, LT_ERR_INVALID,
               "%s: T %d images over B %d samples of %d to %d views", who, T, B, min_views, NVcap);
    return LT_OK;
}
}  // namespace

extern "C" int lt_plan_create_vol_ragged(const lt_vol_plan_config* cfg, int32_t T, const lt_named_tensor* weights, int32_t nweights, lt_plan** plan_out) {
    const char* who = "lt_plan_create_vol_ragged";
    LT_REQUIRE(cfg && weights && plan_out && nweights > 0, LT_ERR_INVALID, "%s: null argument", who);
    PL_TRY(check_vol_config(cfg, who));
    PL_TRY(check_ragged_shape(who, cfg->B, cfg->NV, T, 1));
    *plan_out = nullptr;
    return make_vol_plan(cfg, weights, nweights, who, plan_out, 0, T);
}

extern "C" int lt_plan_forward_vol_ragged(lt_plan* p, const float* images, const double* K_host, const double* R_host, const double* t_host,
                                          const int32_t* view_counts_host, const double* base_points_host, const double* rot_host, float* keypoints_3d,
                                          float* volumes, float* features, float* coord_volumes, float* vol_confidences, void* stream) {
    const char* who = "lt_plan_forward_vol_ragged";
    LT_REQUIRE(p, LT_ERR_INVALID, "%s: null argument", who);
    LT_REQUIRE(p->model == 0 && p->T, LT_ERR_INVALID, "%s: the plan is %s; run it with %s", who, plan_kind_name(p),
               p->model == 0 ? (p->P ? "lt_plan_forward_vol_multi" : "lt_plan_forward_vol") : p->model == MODEL_CASCADE ? "lt_plan_forward_cascade" : "lt_plan_forward_alg");
    LT_REQUIRE(images && K_host && R_host && t_host && view_counts_host && base_points_host && keypoints_3d, LT_ERR_INVALID,
               "%s: null argument (images, K, R, t, view_counts, base_points and keypoints_3d are required)", who);
    PL_TRY(check_view_counts(p, who, view_counts_host, 1));
    return forward_vol_any(p, who, images, K_host, R_host, t_host, nullptr, base_points_host, rot_host, keypoints_3d, volumes, features, coord_volumes,
                           vol_confidences, stream, view_counts_host);
}

extern "C" int lt_plan_create_alg_ragged(const lt_alg_plan_config* cfg, int32_t T, const lt_named_tensor* weights, int32_t nweights, lt_plan** plan_out) {
    const char* who = "lt_plan_create_alg_ragged";
    LT_REQUIRE(cfg && weights && plan_out && nweights > 0, LT_ERR_INVALID, "%s: null argument", who);
    LT_REQUIRE(cfg->model == LT_MODEL_ALG, LT_ERR_INVALID, "%s: model %d (LT_MODEL_ALG only: RANSAC has no ragged plan)", who, cfg->model);
    PL_TRY(check_alg_config(*cfg, who));
    PL_TRY(check_ragged_shape(who, cfg->B, cfg->NV, T, 2));
    *plan_out = nullptr;
    return make_alg_plan(*cfg, weights, nweights, who, plan_out, T);
}

extern "C" int lt_plan_forward_alg_ragged(lt_plan* p, const float* images, const float* proj, const int32_t* view_counts_host, float* keypoints_3d,
                                          void* keypoints_2d, float* heatmaps, float* confidences, void* stream) {
    const char* who = "lt_plan_forward_alg_ragged";
    LT_REQUIRE(p, LT_ERR_INVALID, "%s: null argument", who);
    LT_REQUIRE(p->model == LT_MODEL_ALG && p->T, LT_ERR_INVALID, "%s: the plan is %s; run it with %s", who, plan_kind_name(p),
               p->model == 0 ? (p->T ? "lt_plan_forward_vol_ragged" : p->P ? "lt_plan_forward_vol_multi" : "lt_plan_forward_vol")
                             : p->model == MODEL_CASCADE ? "lt_plan_forward_cascade" : "lt_plan_forward_alg");
    LT_REQUIRE(images && proj && view_counts_host && keypoints_3d, LT_ERR_INVALID, "%s: null argument (images, proj, view_counts and keypoints_3d are required)", who);
    PL_TRY(check_view_counts(p, who, view_counts_host, 2));
    hipStream_t st = (hipStream_t)stream;
    bool detour;
    PL_TRY(p->enter(st, detour));
    p->ran = true;
    PL_TRY(p->stage_view_base(view_counts_host, st));
    p->cur_images = images; p->cur_proj = proj; p->out_kp = keypoints_3d;
    p->out_kp2d = keypoints_2d; p->out_hm = heatmaps; p->out_conf = confidences;
    PL_TRY(p->run(st));
    PL_TRY(p->leave(st, detour));
    return LT_OK;
}

extern "C" int lt_plan_create_alg(const lt_alg_plan_config* cfg, const lt_named_tensor* weights, int32_t nweights, lt_plan** plan_out) {
    LT_REQUIRE(cfg && weights && plan_out && nweights > 0, LT_ERR_INVALID, "lt_plan_create_alg: null argument");
    PL_TRY(check_alg_config(*cfg, "lt_plan_create_alg"));
    *plan_out = nullptr;
    return make_alg_plan(*cfg, weights, nweights, "lt_plan_create_alg", plan_out);
}

extern "C" int lt_plan_forward_alg(lt_plan* p, const float* images, const float* proj, float* keypoints_3d, void* keypoints_2d, float* heatmaps,
                                   float* confidences, void* stream) {
    LT_REQUIRE(p, LT_ERR_INVALID, "lt_plan_forward_alg: null argument");
    LT_REQUIRE(p->model == LT_MODEL_ALG || p->model == LT_MODEL_RANSAC, LT_ERR_INVALID, "lt_plan_forward_alg: the plan is %s; run it with %s", plan_kind_name(p),
               p->model == MODEL_CASCADE ? "lt_plan_forward_cascade" : "lt_plan_forward_vol");
    LT_REQUIRE(!p->T, LT_ERR_INVALID, "lt_plan_forward_alg: the plan is %s; run it with lt_plan_forward_alg_ragged", plan_kind_name(p));
    LT_REQUIRE(images && proj && keypoints_3d, LT_ERR_INVALID, "lt_plan_forward_alg: null argument (images, proj and keypoints_3d are required)");
    hipStream_t st = (hipStream_t)stream;
    bool detour;
    PL_TRY(p->enter(st, detour));
    p->ran = true;
    PL_TRY(p->stage_alg_mask(st));
    p->cur_images = images; p->cur_proj = proj; p->out_kp = keypoints_3d;
    p->out_kp2d = keypoints_2d; p->out_hm = heatmaps; p->out_conf = confidences;
    PL_TRY(p->run(st));
    if (p->model == LT_MODEL_RANSAC) {          // the raw heatmaps and int64 keypoints the plan wrote, and the reference's zero confidences
        const size_t nj = (size_t)p->acfg.B * p->acfg.NV * p->acfg.num_joints;
        if (heatmaps) PL_HIP(hipMemcpyAsync(heatmaps, p->hm_nchw, nj * p->hm_h * p->hm_w * 4, hipMemcpyDeviceToDevice, st));
        if (keypoints_2d) PL_HIP(hipMemcpyAsync(keypoints_2d, p->kp_i64, nj * 2 * 8, hipMemcpyDeviceToDevice, st));
        if (confidences) PL_HIP(hipMemsetAsync(confidences, 0, nj * 4, st));
    }
    PL_TRY(p->leave(st, detour));
    return LT_OK;
}

extern "C" int lt_plan_create_cascade(const lt_cascade_plan_config* cfg, const lt_named_tensor* alg_weights, int32_t n_alg, const lt_named_tensor* vol_weights,
                                      int32_t n_vol, lt_plan** plan_out) {
    const char* who = "lt_plan_create_cascade";
    LT_REQUIRE(cfg && alg_weights && vol_weights && plan_out && n_alg > 0 && n_vol > 0, LT_ERR_INVALID, "%s: null argument", who);
    const lt_alg_plan_config& a = cfg->alg; const lt_vol_plan_config& v = cfg->vol;
    PL_TRY(check_alg_config(a, who));
    LT_REQUIRE(a.model == LT_MODEL_ALG, LT_ERR_INVALID, "%s: alg.model %d (the pelvis comes from LT_MODEL_ALG; LT_MODEL_RANSAC is not a stage of the cascade)", who, a.model);
    PL_TRY(check_vol_config(&v, who));
    LT_REQUIRE(v.B == a.B && v.NV == a.NV && v.H == a.H && v.W == a.W, LT_ERR_INVALID,
               "%s: vol.B %d, vol.NV %d, vol.H %d, vol.W %d differ from alg.B %d, alg.NV %d, alg.H %d, alg.W %d (both stages read the same images)", who, v.B, v.NV, v.H,
               v.W, a.B, a.NV, a.H, a.W);
    LT_REQUIRE(cfg->kind == LT_KIND_MPII || cfg->kind == LT_KIND_COCO, LT_ERR_INVALID, "%s: kind %d (LT_KIND_MPII | LT_KIND_COCO)", who, cfg->kind);
    const int need = cfg->kind == LT_KIND_COCO ? 13 : 7;
    LT_REQUIRE(a.num_joints >= need, LT_ERR_INVALID, "%s: alg.num_joints %d, kind '%s' reads joint %d", who, a.num_joints, cfg->kind == LT_KIND_COCO ? "coco" : "mpii", need - 1);
    PL_TRY(check_alg_heads(a, alg_weights, n_alg, who));
    *plan_out = nullptr;
    lt_plan* p = new lt_plan();
    p->who = who; p->model = MODEL_CASCADE; p->kind = cfg->kind;
    p->cfg = v; p->acfg = a;
    p->cfg.use_graph = (a.use_graph || v.use_graph) ? 1 : 0;          // enter(): a stage that captures cannot run on the legacy default stream
    p->dtype = v.dtype; p->es = v.dtype == LT_F32 ? 4 : 2;
    int rc = make_alg_plan(a, alg_weights, n_alg, who, &p->sub_alg);
    if (rc == LT_OK) rc = make_vol_plan(&v, vol_weights, n_vol, who, &p->sub_vol);
    auto finish = [&]() -> int {
        const size_t nproj = (size_t)a.B * a.NV * 12 * 4;
        void* q;
        PL_TRY(p->dev_alloc(nproj, &q)); p->cproj_dev = (float*)q;
        PL_TRY(p->dev_alloc((size_t)a.B * a.num_joints * 3 * 4, &q)); p->ckp_alg = (float*)q;
        return p->cproj.alloc(nproj);
    };
    if (rc == LT_OK) rc = finish();
    if (rc != LT_OK) { delete p; return rc; }
    *plan_out = p;
    return LT_OK;
}

extern "C" int lt_plan_forward_cascade(lt_plan* p, const float* images, const double* K_host, const double* R_host, const double* t_host, const double* rot_host,
                                       float* keypoints_3d, float* alg_keypoints_3d, float* base_points, float* volumes, float* features, float* coord_volumes,
                                       float* vol_confidences, void* stream) {
    LT_REQUIRE(p, LT_ERR_INVALID, "lt_plan_forward_cascade: null argument");
    LT_REQUIRE(p->model == MODEL_CASCADE, LT_ERR_INVALID, "lt_plan_forward_cascade: the plan is %s; run it with %s", plan_kind_name(p),
               p->model == 0 ? "lt_plan_forward_vol" : "lt_plan_forward_alg");
    LT_REQUIRE(images && K_host && R_host && t_host && keypoints_3d, LT_ERR_INVALID, "lt_plan_forward_cascade: null argument (images, K, R, t and keypoints_3d are required)");
    lt_plan* A = p->sub_alg; lt_plan* Vp = p->sub_vol;
    LT_REQUIRE(!vol_confidences || !Vp->volc.null(), LT_ERR_INVALID,
               "lt_plan_forward_cascade: vol_confidences asked of a plan without the confidence head (aggregation %d)", Vp->cfg.aggregation);
    hipStream_t st = (hipStream_t)stream;
    bool detour;
    PL_TRY(p->enter(st, detour));
    const int B = Vp->cfg.B, NV = Vp->cfg.NV, V = Vp->cfg.volume_size;
    p->ran = true;
    // cameras once: the volumetric stage's block (projections at heatmap resolution, rotations; pos / center are the seam kernel's) and the algebraic
    // stage's projections at image resolution: two H2D copies, the geometry slot's event re-recorded behind the second.  The wait in stage_geometry covers
    // both blocks: this cproj block was last read one turn of the rings ago, by the copy in front of that event.
    void* cproj_blk; PL_TRY(p->cproj.acquire(&cproj_blk));
    PL_TRY(Vp->stage_geometry(K_host, R_host, t_host, nullptr, rot_host, st, (float*)cproj_blk));
    PL_HIP(hipMemcpyAsync(p->cproj_dev, cproj_blk, (size_t)B * NV * 12 * 4, hipMemcpyHostToDevice, st));
    PL_TRY(Vp->geo.commit(st));
    // stage 1: lt_plan_forward_alg's launches
    float* kp_alg = alg_keypoints_3d ? alg_keypoints_3d : p->ckp_alg;
    A->cur_images = images; A->cur_proj = p->cproj_dev; A->out_kp = kp_alg; A->out_kp2d = nullptr; A->out_hm = nullptr; A->out_conf = nullptr;
    PL_TRY(A->run(st));
    // the seam: joints -> cuboid origin and centre, straight into the block lt_unproject_grid_fwd reads
    PL_TRY(lt_cuboid_from_keypoints(kp_alg, B, p->acfg.num_joints, p->kind, Vp->cfg.cuboid_side, Vp->geo_dev + Vp->o_pos, Vp->geo_dev + Vp->o_cen, st));
    if (base_points) PL_HIP(hipMemcpyAsync(base_points, Vp->geo_dev + Vp->o_cen, (size_t)B * 3 * 4, hipMemcpyDeviceToDevice, st));
    // stage 2: lt_plan_forward_vol's launches
    Vp->cur_images = images; Vp->out_kp = keypoints_3d; Vp->out_probs = volumes; Vp->out_feats = features;
    PL_TRY(Vp->run(st));
    if (coord_volumes) PL_HIP(hipMemcpyAsync(coord_volumes, Vp->coords, (size_t)B * V * V * V * 3 * 4, hipMemcpyDeviceToDevice, st));
    if (vol_confidences) PL_HIP(hipMemcpyAsync(vol_confidences, Vp->volc.p, (size_t)B * NV * 32 * 4, hipMemcpyDeviceToDevice, st));
    PL_TRY(p->leave(st, detour));
    return LT_OK;
}

extern "C" int lt_plan_set_view_mask(lt_plan* p, const uint8_t* mask_host) {
    const char* who = "lt_plan_set_view_mask";
    LT_REQUIRE(p, LT_ERR_INVALID, "%s: null plan", who);
    LT_REQUIRE(!p->T, LT_ERR_INVALID, "%s: the plan is %s; a ragged plan takes no view mask (drop the view from the batch instead)", who, plan_kind_name(p));
    LT_REQUIRE(p->model != LT_MODEL_RANSAC, LT_ERR_UNSUPPORTED, "%s: the plan is %s; RANSAC takes no view mask (its inlier search drops views per joint)", who,
               plan_kind_name(p));
    const int B = p->cfg.B, NV = p->cfg.NV;
    const int need = p->model == 0 ? 1 : 2;          // the DLT of the algebraic model (and of the cascade's first stage) needs two views
    std::vector<uint8_t> m((size_t)B * NV, 1);
    for (size_t i = 0; mask_host && i < m.size(); ++i) m[i] = mask_host[i] ? 1 : 0;
    for (int b = 0; b < B; ++b) {
        int n = 0;
        for (int v = 0; v < NV; ++v) n += m[(size_t)b * NV + v];
        LT_REQUIRE(n >= need, LT_ERR_INVALID, "%s: sample %d has %d valid view%s, at least %d needed (%s)", who, b, n, n == 1 ? "" : "s", need, plan_kind_name(p));
    }
    if (!p->masked) {
        LT_REQUIRE(!p->ran, LT_ERR_INVALID, "%s: the first call must come before the plan's first forward (the recorded and captured launches are chosen "
                   "there); create a new plan for masked forwards", who);
        if (p->model == MODEL_CASCADE) {
            PL_TRY(p->sub_vol->grow_geometry_for_mask());
            p->sub_alg->mask_dev = p->sub_vol->mask_dev;          // the algebraic stage reads the volumetric stage's block: one copy for both
            p->sub_vol->masked = p->sub_alg->masked = true;
        } else if (p->model == 0) {
            PL_TRY(p->grow_geometry_for_mask());
        } else {
            PL_TRY(p->alloc_alg_mask());
        }
        p->masked = true;
    }
    lt_plan* holder = p->model == MODEL_CASCADE ? p->sub_vol : p;
    holder->mask_cur = m;
    holder->mask_dirty = true;
    return LT_OK;
}

extern "C" int lt_plan_set_keypoint_stats(lt_plan* p, float* stats_dev, int32_t* peak_index_dev) {
    const char* who = "lt_plan_set_keypoint_stats";
    LT_REQUIRE(p, LT_ERR_INVALID, "%s: null plan", who);
    LT_REQUIRE(p->model == 0 || p->model == MODEL_CASCADE, LT_ERR_UNSUPPORTED, "%s: the plan is %s; the statistics are those of the volumetric joints' 3D heatmaps", who,
               plan_kind_name(p));
    LT_REQUIRE((stats_dev == nullptr) == (peak_index_dev == nullptr), LT_ERR_INVALID, "%s: stats_dev and peak_index_dev come together (both NULL: the plain tail)", who);
    lt_plan* v = p->model == MODEL_CASCADE ? p->sub_vol : p;
    if (stats_dev && !v->ks_ws) {
        const int V = v->cfg.volume_size;
        PL_TRY(v->dev_alloc(lt_softargmax3d_stats_workspace(v->cuboids(), v->cfg.num_joints, (int64_t)V * V * V), &v->ks_ws));
    }
    v->ks_stats = stats_dev; v->ks_index = peak_index_dev;
    return LT_OK;
}

extern "C" int lt_plan_set_alg_keypoint_stats(lt_plan* p, float* stats2d_dev, int32_t* peak_index_dev, float* cov2d_img_dev, float* reproj_err_dev,
                                              float* cov3d_dev) {
    const char* who = "lt_plan_set_alg_keypoint_stats";
    LT_REQUIRE(p, LT_ERR_INVALID, "%s: null plan", who);
    LT_REQUIRE(p->model == LT_MODEL_ALG || p->model == MODEL_CASCADE, LT_ERR_UNSUPPORTED, "%s: the plan is %s; the statistics are those of the algebraic joints", who,
               plan_kind_name(p));
    LT_REQUIRE(!p->T, LT_ERR_UNSUPPORTED, "%s: the plan is %s; there is no ragged statistics tail (pad the batch and use lt_plan_set_view_mask on a plan of "
               "lt_plan_create_alg)", who, plan_kind_name(p));
    const int n = (stats2d_dev != nullptr) + (peak_index_dev != nullptr) + (cov2d_img_dev != nullptr) + (reproj_err_dev != nullptr) + (cov3d_dev != nullptr);
    LT_REQUIRE(n == 0 || n == 5, LT_ERR_INVALID,
               "%s: stats2d_dev, peak_index_dev, cov2d_img_dev, reproj_err_dev and cov3d_dev come together (all NULL: the plain tail); %d of 5 given", who, n);
    lt_plan* a = p->model == MODEL_CASCADE ? p->sub_alg : p;
    a->aks_stats2d = stats2d_dev; a->aks_index = peak_index_dev; a->aks_cov2d = cov2d_img_dev; a->aks_reproj = reproj_err_dev; a->aks_cov3d = cov3d_dev;
    return LT_OK;
}

extern "C" int lt_plan_info(const lt_plan* p, lt_plan_info_t* info) {
    LT_REQUIRE(p && info, LT_ERR_INVALID, "lt_plan_info: null argument");
    memset(info, 0, sizeof(*info));
    if (p->model == MODEL_CASCADE) {          // both stages' launches, flops, memory and census; heatmap size and logits: the volumetric stage's
        lt_plan_info_t a;
        PL_TRY(lt_plan_info(p->sub_vol, info));
        PL_TRY(lt_plan_info(p->sub_alg, &a));
        info->launches += a.launches + 1;
        info->flops += a.flops; info->bytes_allocated += a.bytes_allocated + (int64_t)p->bytes_alloc;
        info->n_expand_reduce += a.n_expand_reduce; info->n_bottleneck += a.n_bottleneck; info->n_bottleneck_ds += a.n_bottleneck_ds; info->n_conv_cat2 += a.n_conv_cat2;
        info->n_conv2d_halo += a.n_conv2d_halo; info->n_pwchain += a.n_pwchain; info->n_stem_pool += a.n_stem_pool; info->n_splitk += a.n_splitk;
        info->n_conv_skip += a.n_conv_skip;
        info->graph_captured = (!p->sub_alg->cfg.use_graph || a.graph_captured) && (!p->sub_vol->cfg.use_graph || info->graph_captured) &&
                               (p->sub_alg->cfg.use_graph || p->sub_vol->cfg.use_graph) ? 1 : 0;
        return LT_OK;
    }
    info->launches = (int32_t)p->ops.size();
    info->heatmap_h = p->hm_h; info->heatmap_w = p->hm_w;
    info->flops = p->flops; info->bytes_allocated = (int64_t)p->bytes_alloc;
    info->n_expand_reduce = p->n_xr; info->n_bottleneck = p->n_bneck; info->n_bottleneck_ds = p->n_bneck_ds; info->n_conv_cat2 = p->n_cat2;
    info->n_conv2d_halo = p->n_halo2d; info->n_pwchain = p->n_pwchain; info->n_stem_pool = p->n_stem; info->n_splitk = p->n_splitk; info->n_conv_skip = p->n_conv_skip;
    info->graph_captured = p->captured ? 1 : 0;
    info->logits = (const float*)p->logits.p; info->logits_planar = p->logits.planar ? 1 : 0;
    return LT_OK;
}

extern "C" void lt_plan_destroy(lt_plan* p) { delete p; }
