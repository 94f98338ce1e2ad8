// The launch plan of the refiner network.
//
// The plan is the MI355X-side equivalent of detectron2's build_model(cfg) for the QuBER refiner:
// it walks the same module tree as
//   maskrefiner/modeling/backbone/resnet.py:358-519   (two ResNet-DeepLab streams + concat fusion)
//   [d2] DeepLabV3PlusHead / ASPP                      (decoder)
//   maskrefiner/modeling/mask_refiner/model.py:711-764 (hierarchical boundary-error -> fg/centre/offset heads)
// but emits a flat list of kernel launches over NHWC buffers.  Design points:
//   * the rgb and depth streams run as ONE grouped launch per layer (blockIdx.z selects the stream),
//     as do the three second-level prediction heads;
//   * every torch.cat of the reference is free: producers write straight into a channel slice of
//     the concatenated buffer (stream outputs, ASPP branches, decoder skip joins, the 164-channel
//     y | feat_b | softmax(pred_b) fusion input);
//   * FrozenBN / eval-BN / bias are folded into the convolution epilogue's per-channel affine;
//   * the head-fusion stack the reference evaluates three times (model.py:760-762) is evaluated once.
#include "plan.h"

namespace quber {
namespace {

constexpr int BLOCKS50[4] = {3, 4, 6, 3}, BLOCKS101[4] = {3, 4, 23, 3}, BLOCKS152[4] = {3, 8, 36, 3};

// FrozenBN ([d2]) of the convolution with key prefix n, folded into a per-channel affine: scale = weight * rsqrt(var + eps), shift = bias - mean * scale
struct BnFold {
    const float *w, *b, *m, *v;
    bool ok() const { return w && b && m && v; }
    float scale(int o) const { return w[o] * (1.0f / sqrtf(v[o] + 1e-5f)); }
    float shift(int o, float sc) const { return b[o] - m[o] * sc; }
};
BnFold frozen_bn(Builder& b, const std::string& n, int C) {
    return {b.hw(n + ".norm.weight", C), b.hw(n + ".norm.bias", C), b.hw(n + ".norm.running_mean", C), b.hw(n + ".norm.running_var", C)};
}

// Winograd F(m x m,3x3) alternatives for the wide plain 3x3 layers.  The algorithm of a layer is fixed at plan
// time, from the layer's geometry alone (frame size, channels, dilation) - never from the batch of a launch - so
// that a frame's logits do not change class of arithmetic with the batch it arrives in (split-K, a pure
// re-association of the same fp32 sum, is the only per-launch choice left).
// Ragged frames and a dilated layer's short phases are padded to whole tiles: a variant qualifies only while it
// still executes <= tune().wino_max_ratio % of the direct multiplies.  The choice is the best of m = 4 / 2 (F(4x4) measures the
// direct kernel's error against float64, profiles/r02a_parity_report.txt).  The 6x6 variant is OPT-IN
// (quber_set_tuning key 9 = 6 / QUBER_WINOGRAD=f6): 2.5x the error at tap level, +4.5 % throughput at batch 16.
// The decision - which layers, which m - is taken from the PER-PHASE ratio of a dilated layer, whatever option key 51 says: packing the
// phases of an axis into shared tiles (winograd_xf.h: Axis) makes the layers that take the pipeline cheaper, it does not change which
// layers do, so every configuration keeps its plan.  In particular ASPP d = 18 on the 30x40 map stays on its zone-skipping direct
// launch: packed it would run 180 tiles, a ratio of 180 * 36 / (9 * 1200) = 0.60 and under key 8's 67 %, but 180 tiles cost about
// 1.1 ms at 16 frames against the 0.85 ms of that launch, which already executes only 0.42 of the direct multiplies.
// take it or not; m = the output tile edge; ratio = executed / direct multiplies of that variant on this map; one_kernel = eligible for the single-kernel
// form (wino_fused.hip): its filter order is uploaded too.  plain = every input channel is real, no residual, no PReLU
struct WinoChoice { bool take = false; int m = 0; double ratio = 0.0; bool one_kernel = false; };
WinoChoice choose_winograd(int H, int W, int k, int stride, int pad, int dil, int Cin, int Cout, bool plain, int dtype) {
    WinoChoice r;
    // (the 16-bit operand modes keep every layer on the direct kernel: the Winograd transforms amplify the operands'
    // rounding error; the bf16x3 mode is fp32-equivalent and takes the same plan as the exact fp32 MFMA mode)
    if (!winograd_eligible(k, stride, pad, dil, Cin, Cout) || !plain || tune().winograd == 1 || (dtype != 0 && dtype != 3)) return r;
    const double lim = (double)tune().wino_max_ratio / 100.0;
    const double r6 = winograd_m6_channels_ok(Cin, Cout) ? winograd_mac_ratio(H, W, dil, 6) : 1e9;
    const double r4 = winograd_mac_ratio(H, W, dil, 4), r2 = winograd_mac_ratio(H, W, dil, 2);
    double best = lim;
    int wm = 0;
    if (r2 <= best && tune().wino_variant != 4 && tune().wino_variant != 6) { best = r2; wm = 2; }
    if (r4 <= best && tune().wino_variant != 2) { best = r4; wm = 4; }
    if (r2 <= lim && wm == 0) { best = r2; wm = 2; }                     // a forced larger variant does not fit: smaller tiles
    const bool has6 = wm != 0 && tune().wino_variant == 6 && r6 <= 0.9 * best;
    r.m = has6 ? 6 : wm;
    r.ratio = has6 ? r6 : best;
    r.one_kernel = r.m == 4 && tune().wino_fused && Cout % 32 == 0 && Cin <= tune().wino_fused_max_cin;     // (dtype 0 or 3: checked above)
    // Maps of a handful of tiles stay on the direct kernel.  The 64-channel layers (res2.conv2) lose to it as three
    // kernels (below 128 channels only the opt-in 6x6 variant outweighs its transforms) but not as ONE: 0.25 against
    // 0.43 ms per layer (wino_fused.hip; profiles/r05_wino_fused_layers.md).
    r.take = wm != 0 && (tune().winograd == 2 || (Cin < 128 ? (has6 || (r.one_kernel && (long)H * W >= 1024)) : (long)H * W >= 1024));
    return r;
}

}  // namespace

// ---- host weights ----
const float* Builder::hw(const std::string& name, int64_t numel) {
    if (dry) {
        c->specs.emplace_back(name, numel);
        return nullptr;
    }
    auto it = c->hostw.find(name);
    if (it == c->hostw.end()) {
        if (err.empty()) err = "missing weight '" + name + "'";
        return nullptr;
    }
    if ((int64_t)it->second.size() != numel) {
        if (err.empty()) err = "weight '" + name + "' has " + std::to_string(it->second.size()) + " elements, expected " + std::to_string(numel);
        return nullptr;
    }
    return it->second.data();
}

// ---- device memory ----
void* Builder::dalloc_bytes(size_t bytes) {
    if (dry) return nullptr;
    void* p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) {
        if (err.empty()) err = "hipMalloc of " + std::to_string(bytes) + " bytes failed";
        return nullptr;
    }
    c->allocs.push_back(p);
    c->alloc_bytes += bytes ? bytes : 16;
    if (hipMemset(p, 0, bytes ? bytes : 16) != hipSuccess && err.empty()) err = "hipMemset of a new buffer failed";
    return p;
}
template <class T> static float* upload_vec(Builder& b, const std::vector<T>& v, const char* unit) {
    float* d = (float*)b.dalloc_bytes(v.size() * sizeof(T));
    if (d && hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess && b.err.empty())
        b.err = "upload of " + std::to_string(v.size()) + unit + " failed";
    return d;
}
float* Builder::upload16(const std::vector<_Float16>& v) { return upload_vec(*this, v, " halfs"); }
float* Builder::upload(const std::vector<float>& v) { return upload_vec(*this, v, " floats"); }
// packed filters in the element type of the data path: rounded to fp16 once, here, in the fp16 data path
const float* Builder::upload_weights(const std::vector<float>& packed) {
    if (aes != 2) return upload(packed);
    std::vector<_Float16> ph(packed.size());
    for (size_t i = 0; i < packed.size(); ++i) ph[i] = (_Float16)packed[i];
    return upload16(ph);
}
// bf16x3 mode: an uploaded fp32 weight array as three planes of bf16 terms (conv_x8.hip); on the null stream, finalize synchronises
const void* Builder::split3(const float* dev_w, size_t n) {
    if (dry || !dev_w || c->cfg.compute_dtype != 3) return nullptr;
    void* planes = dalloc_bytes(n * 3 * sizeof(unsigned short));
    if (planes && launch_split_bf16x3(dev_w, (long)n, planes, nullptr) && err.empty()) err = "bf16x3 weight split failed";
    return planes;
}
View Builder::make(int C, int h, int w, int G) {
    View v;
    v.B = Bmax; v.H = h; v.W = w; v.C = C; v.cs = C;
    v.gs = (long)Bmax * h * w * C;
    v.es = aes;
    v.p = (float*)dalloc_bytes((size_t)aes * (size_t)v.gs * G);
    return v;
}
View Builder::slice(View v, int coff, int C, long gs) {
    v.p = v.at(coff);
    v.C = C;
    if (gs >= 0) v.gs = gs;
    return v;
}

// ---- ops ----
// Emits one (grouped) convolution launch.  w[g] = OIHW host weights of group g; scale/shift/prelu are
// [G*Cout] per-channel epilogue vectors (prelu may be empty).
void Builder::emit_conv(const std::string& name, const std::vector<const float*>& w, const View& in, int cin_real, const View& out, int k, int stride, int pad, int dil, bool affine,
                        const std::vector<float>& scale, const std::vector<float>& shift, const std::vector<float>& prelu, const View* res, bool relu, const std::vector<int>& dil_g) {
    const int G = (int)w.size();
    const int Cin = in.C, Cout = out.C;
    const int KS = aes == 2 ? 64 : 32;        // K-slice of the kernel in elements (32 four-byte units: 64 halfs in the fp16 data path)
    const int K = k * k * Cin, Kpad = (K + KS - 1) / KS * KS;
    const int OH = (in.H + 2 * pad - dil * (k - 1) - 1) / stride + 1;
    const int OW = (in.W + 2 * pad - dil * (k - 1) - 1) / stride + 1;
    // dilated 3x3 whose top / bottom filter rows are padding for >= 20 % of the (row, tap) pairs and that cannot take the
    // Winograd path: tap-major K order so that blocks can skip those rows (conv_igemm.hip MODE 3 / 4)
    // (its Winograd test is a separate, weaker one than choose_winograd: no map-size, channel or dtype terms.  Kept as it is.)
    const bool skip_rows = k == 3 && stride == 1 && dil > 1 && Cin % KS == 0 && cin_real == Cin && 10 * 2 * pad >= 2 * 3 * OH &&
                           !(winograd_eligible(k, stride, pad, dil, Cin, out.C) && !res && prelu.empty() &&
                             std::min(winograd_mac_ratio(in.H, in.W, dil, 4), winograd_mac_ratio(in.H, in.W, dil, 2)) <= tune().wino_max_ratio / 100.0 && tune().winograd != 1);
    const int kmode = (k > 1 && Cin % KS == 0 && !skip_rows) ? 1 : 0;   // slice-major K order for the 3x3 layers
    if (dry) return;
    const double fl = 2.0 * OH * OW * (double)cin_real * k * k * Cout * G;
    c->flops += fl;
    if (OH != out.H || OW != out.W) { if (err.empty()) err = "internal: conv output geometry mismatch at " + name; return; }
    for (const float* p : w)
        if (!p) return;   // a missing weight was already reported
    std::vector<float> packed((size_t)G * Cout * Kpad, 0.f);
    for (int g = 0; g < G; ++g)
        for (int o = 0; o < Cout; ++o) {
            float* dst = &packed[((size_t)g * Cout + o) * Kpad];
            for (int ci = 0; ci < cin_real; ++ci)
                for (int t = 0; t < k * k; ++t) {
                    const size_t kk = kmode ? ((size_t)(ci / KS) * k * k + t) * KS + ci % KS : (size_t)t * Cin + ci;
                    dst[kk] = w[g][((size_t)o * cin_real + ci) * k * k + t];
                }
        }
    ConvP p{};
    p.in = in.p;
    p.w = upload_weights(packed);
    if (aes != 2 && k == 1) { p.w3 = split3(p.w, packed.size()); p.w3_plane = (long)packed.size(); }
    p.es = aes;
    if (in.es != aes || out.es != aes || (res && res->es != aes)) { if (err.empty()) err = "internal: element type mismatch at " + name; return; }
    // (fp16 data path, layers of >= 32 output channels without an affine - ASPP branches, decoder convolutions, heads: an identity affine, so that conv_h8.hip, whose epilogue
    //  always reads one, takes them; fma(v, 1, 0) == v)
    const bool ident = !affine && aes == 2 && Cout >= 32;
    p.scale = affine ? upload(scale) : ident ? upload(std::vector<float>((size_t)G * Cout, 1.f)) : nullptr;
    p.shift = affine ? upload(shift) : ident ? upload(std::vector<float>((size_t)G * Cout, 0.f)) : nullptr;
    for (size_t g = 0; g < dil_g.size() && g < 4; ++g) p.dil_g[g] = dil_g[g];      // per-group dilation (= padding) of a grouped launch
    p.prelu = prelu.empty() ? nullptr : upload(prelu);
    p.res = res ? res->p : nullptr;
    p.out = out.p;
    p.H = in.H; p.W = in.W; p.Cin = Cin; p.in_cs = in.cs;
    p.OH = OH; p.OW = OW; p.Cout = Cout; p.out_cs = out.cs;
    p.res_cs = res ? res->cs : 0;
    p.K = K; p.Kpad = Kpad;
    p.kh = k; p.kw = k; p.stride = stride; p.pad = pad; p.dil = dil;
    p.relu = relu; p.kmode = kmode; p.skip_rows = skip_rows;
    p.bf16 = c->cfg.compute_dtype;
    p.in_gs = in.gs; p.out_gs = out.gs; p.res_gs = res ? res->gs : 0;
    p.w_gs = (long)Cout * Kpad; p.ss_gs = Cout;
    p.ohw = OH * OW;
    quber_ctx* ctx = c;
    const WinoChoice wc = choose_winograd(in.H, in.W, k, stride, pad, dil, Cin, Cout, cin_real == Cin && !res && prelu.empty(), c->cfg.compute_dtype);
    const bool wino = wc.take;
    WinoP wq{};
    if (wino) {
        const int m = wc.m, P = (m + 2) * (m + 2);
        c->wino_flops += fl;
        std::vector<float> u((size_t)G * P * Cout * Cin);
        for (int g = 0; g < G; ++g) winograd_weights_host(w[g], Cout, Cin, m, &u[(size_t)g * P * Cout * Cin]);
        wq.in = in; wq.out = out; wq.u = upload(u);
        wq.u3 = split3(wq.u, u.size()); wq.u3_plane = (long)u.size();
        if (wc.one_kernel) {     // operand order of the single-kernel form
            std::vector<float> uf(u.size());
            for (int g = 0; g < G; ++g) winograd_fused_pack_host(&u[(size_t)g * P * Cout * Cin], Cout, Cin, &uf[(size_t)g * P * Cout * Cin]);
            wq.uf = upload(uf);
        }
        wq.scale = p.scale; wq.shift = p.shift; wq.ss_gs = Cout; wq.relu = relu; wq.dil = dil; wq.m = m;
        wq.dtype = c->cfg.compute_dtype;
        wq.pack = tune().wino_pack;
    }
    std::shared_ptr<DeferredNorm> norm, norm16;
    if (wino && pending_norm && pending_norm->out.p == in.p && pending_norm->C == Cin && pending_norm->G == G) {
        norm = pending_norm;
        norm->absorbed = true;
    }
    // fp16 data path: an undilated 3x3 layer applies the GroupNorm + ReLU in front of it to its LDS patches
    // (conv_h8.hip, key 39); whether a launch really does is decided per launch (conv_h8_patch_takes: the launch-time keys may say otherwise)
    float* coef16 = nullptr;
    if (!wino && aes == 2 && tune().h8_norm && tune().h8 && tune().h8_narrow && pending_norm && pending_norm->out.p == in.p && pending_norm->C == Cin &&
        pending_norm->G == G && k == 3 && stride == 1 && pad == 1 && dil == 1 && dil_g.empty() && Cin % 64 == 0 && Cin >= 128 && Cin <= 512 && cin_real == Cin &&
        (Cout == 128 || Cout == 64 || Cout == 32 || (Cout >= 256 && Cout % 8 == 0 && tune().h8_narrow != 2)) && !res && prelu.empty() && in.cs == pending_norm->in.cs && in.gs == pending_norm->in.gs) {
        norm16 = pending_norm;
        norm16->absorbed = true;
        coef16 = (float*)dalloc_bytes(sizeof(float) * (size_t)G * Bmax * Cin * 2);
    }
    pending_norm.reset();
    if (wino) {     // workspace: V | M of the three-kernel pipeline, or only the fused GroupNorm's coefficients of the single-kernel form
        WinoP probe = wq;
        if (norm) probe.in = norm->in;           // what the layer will read (in place -> the pipeline)
        const bool fusedk = wq.uf && winograd_fused_ok(probe, Bmax, G);
        wq.algo = fusedk ? 2 : 1;            // decided once, here, for max_batch: every smaller launch takes the same kernels
        // executed multiplies over the direct kernel's, of the tiles the layer really runs: the single kernel tiles per phase, the pipeline per key 51
        const double ratio = fusedk ? wc.ratio : winograd_mac_ratio_run(in.H, in.W, dil, wq.m, wq.pack != 0);
        c->wino_saved += fl * (1.0 - ratio);
        // exactly tiled, F(m x m) executes (m + 2)^2 / (9 m^2) of the direct multiplies: what it executes beyond that is tile padding
        c->wino_pad += fl * (ratio - (double)((wq.m + 2) * (wq.m + 2)) / (9.0 * wq.m * wq.m));
        if (wq.uf && winograd_fused_prepare() && err.empty()) err = "winograd (fused): cannot raise the kernels' LDS limit";
        const size_t need = fusedk ? winograd_fused_ws_floats(Bmax, Cin, G) : winograd_ws_floats(Bmax, in.H, in.W, Cin, Cout, G, dil, wq.m);
        if (need > c->wino_floats) c->wino_floats = need;
        if (cur_lane) {
            const int lb = std::min(Bmax, LANE_BATCH);
            const size_t ln = fusedk ? winograd_fused_ws_floats(lb, Cin, G) : winograd_ws_floats(lb, in.H, in.W, Cin, Cout, G, dil, wq.m);
            if (ln > c->lane_wino_floats[cur_lane]) c->lane_wino_floats[cur_lane] = ln;
        }
    }
    auto fuse = std::make_shared<GnFuse>();
    last_conv = {fuse, out.p, G, Cout};
    const int L = cur_lane;
    c->ops.push_back({[p, G, ctx, fuse, wq, wino, norm, norm16, coef16, L](int B, hipStream_t st) mutable {
        const bool side = L && ctx->lane_now == L;             // launched on its side lane: that lane's workspaces
        float* const sk_ws = side ? ctx->lane_splitk_ws[L] : ctx->splitk_ws;
        const size_t sk_floats = side ? ctx->lane_splitk_floats : ctx->splitk_floats;
        if (wino) {
            wq.ws = side ? ctx->lane_wino_ws[L] : ctx->wino_ws; wq.ws_floats = side ? ctx->lane_wino_floats[L] : ctx->wino_floats;
            wq.splitk_ws = sk_ws; wq.splitk_floats = sk_floats;
            wq.gn_sum = fuse->sums; wq.gn_groups = fuse->groups;
            if (norm) {                      // read the producer's pre-normalisation tensor and normalise on load
                wq.in = norm->in;
                wq.norm = WinoNorm{norm->stats, norm->gamma, norm->beta, 32, 0, norm->C, 1, 0.0, 1e-5f};
            }
            return launch_conv_winograd(wq, B, G, st);
        }
        p.B = B;
        p.M = B * p.OH * p.OW;
        p.ws = sk_ws;
        p.ws_floats = sk_floats;
        p.gn_sum = fuse->sums;
        p.gn_groups = fuse->groups;
        p.gn_cpg = fuse->groups ? p.Cout / fuse->groups : 0;
        if (norm16) {
            ConvP q = p;
            q.in = norm16->in.p;              // the producer's raw output: normalised on the patch
            q.n_stats = norm16->stats; q.n_gamma = norm16->gamma; q.n_beta = norm16->beta; q.n_coef = coef16;
            q.n_groups = 32; q.n_param_gs = norm16->C; q.n_relu = 1; q.n_eps = 1e-5f;
            if (conv_h8_patch_takes(q, G, true)) return launch_conv(q, G, st);
            // this launch's keys keep it off the patch kernel: the norm as the pass it was, then the convolution on its output
            const int rc = launch_gn_apply(norm16->in, norm16->out, B, G, 32, norm16->stats, norm16->gamma, norm16->beta, norm16->C, 1e-5f, 1, st);
            if (rc) return rc;
        }
        return launch_conv(p, G, st);
    }, OP_CONV, name, fl, 1});
    c->ops.back().lane = cur_lane;
}

// refiner convolutions: `names` = one detectron2 Conv2d key prefix per group (e.g. "backbone.rgb_backbone.stem.conv1")
void Builder::conv(const std::vector<std::string>& names, const View& in, int cin_real, const View& out, int k, int stride, int pad, int dil, Affine af, const View* res, bool relu,
                   const std::vector<int>& dil_g) {
    const int G = (int)names.size(), Cout = out.C;
    std::vector<float> scale((size_t)G * Cout, 1.f), shift((size_t)G * Cout, 0.f);
    std::vector<const float*> w;
    for (int g = 0; g < G; ++g) {
        const std::string& n = names[g];
        w.push_back(hw(n + ".weight", (int64_t)Cout * cin_real * k * k));
        const bool has_bn = af == AF_FROZEN_BN || af == AF_BIAS_BN;
        const float* bias = (af == AF_BIAS || af == AF_BIAS_BN) ? hw(n + ".bias", Cout) : nullptr;
        const BnFold bn = has_bn ? frozen_bn(*this, n, Cout) : BnFold{};
        if (dry || (has_bn && !bn.ok())) continue;
        for (int o = 0; o < Cout; ++o) {
            float sc = 1.f, sh = 0.f;
            if (has_bn) {
                sc = bn.scale(o);
                sh = bn.shift(o, sc);
                if (af == AF_BIAS_BN && bias) sh = fmaf(bias[o], sc, sh);
            } else if (af == AF_BIAS && bias) {
                sh = bias[o];
            }
            scale[(size_t)g * Cout + o] = sc;
            shift[(size_t)g * Cout + o] = sh;
        }
    }
    emit_conv(names[0], w, in, cin_real, out, k, stride, pad, dil, af != AF_NONE, scale, shift, {}, res, relu, dil_g);
}

// Projection block of a stage: the two ops emitted last - `shortcut` (1x1, stride s, FrozenBN) and `conv3` (1x1, FrozenBN,
// + shortcut output, ReLU) - become ONE op that computes relu(bn3(conv3(y)) + bn_s(shortcut(x))) as a single 1x1 GEMM
// over the concatenated channels of y and x (launch_conv_dual: BN scales folded into the packed weights, shifts
// added), so that the shortcut's output never exists in HBM.  Launches the dual kernel does not cover (16-bit operand
// modes, views past 2 GiB) run the two original ops.
void Builder::fuse_shortcut(const std::vector<std::string>& n3, const std::vector<std::string>& ns, const View& y, int mid, const View& x, int cin, int stride, const View& out) {
    if (dry || !tune().fuse_shortcut || c->ops.size() < 2) return;
    const int G = (int)n3.size(), Cout = out.C, Kd = mid + cin;
    const int KS = aes == 2 ? 64 : 32;         // K-slice in elements
    if (mid % KS || cin % KS || y.C != mid || x.C != cin) return;
    std::vector<float> packed((size_t)G * Cout * Kd), ones((size_t)G * Cout, 1.f), shift((size_t)G * Cout);
    for (int g = 0; g < G; ++g) {
        const float* w3 = hw(n3[g] + ".weight", (int64_t)Cout * mid);
        const float* wsh = hw(ns[g] + ".weight", (int64_t)Cout * cin);
        const BnFold b3 = frozen_bn(*this, n3[g], Cout), bs = frozen_bn(*this, ns[g], Cout);
        if (!w3 || !wsh || !b3.ok() || !bs.ok()) return;
        for (int o = 0; o < Cout; ++o) {
            const float s3 = b3.scale(o), h3 = b3.shift(o, s3), ss = bs.scale(o), hs = bs.shift(o, ss);      // the per-channel affines of the separate launches
            float* dst = &packed[((size_t)g * Cout + o) * Kd];
            for (int ci = 0; ci < mid; ++ci) dst[ci] = s3 * w3[(size_t)o * mid + ci];
            for (int ci = 0; ci < cin; ++ci) dst[mid + ci] = ss * wsh[(size_t)o * cin + ci];
            shift[(size_t)g * Cout + o] = h3 + hs;
        }
    }
    ConvP p{};
    p.in = y.p; p.in2 = x.p; p.scale = upload(ones); p.shift = upload(shift); p.out = out.p;
    p.w = upload_weights(packed);
    if (aes != 2) { p.w3 = split3(p.w, packed.size()); p.w3_plane = (long)packed.size(); }     // bf16x3 mode: the three bf16 planes (conv_x8.hip)
    p.es = aes;
    p.H = y.H; p.W = y.W; p.Cin = mid; p.in_cs = y.cs; p.in_gs = y.gs;
    p.H2 = x.H; p.W2 = x.W; p.in2_cs = x.cs; p.in2_gs = x.gs; p.stride2 = stride; p.K1 = mid;
    p.OH = out.H; p.OW = out.W; p.Cout = Cout; p.out_cs = out.cs; p.out_gs = out.gs;
    p.K = Kd; p.Kpad = Kd; p.kh = 1; p.kw = 1; p.stride = 1; p.pad = 0; p.dil = 1; p.relu = 1;
    p.bf16 = c->cfg.compute_dtype;
    p.w_gs = (long)Cout * Kd; p.ss_gs = Cout; p.ohw = out.H * out.W;
    Op op3 = c->ops.back();
    c->ops.pop_back();
    Op ops = c->ops.back();
    c->ops.pop_back();
    quber_ctx* ctx = c;
    c->ops.push_back({[p, G, ctx, op3, ops](int B, hipStream_t st) mutable {
        p.B = B;
        p.M = B * p.OH * p.OW;
        p.ws = ctx->splitk_ws;
        p.ws_floats = ctx->splitk_floats;
        const int rc = launch_conv_dual(p, G, st);
        if (rc != 1) return rc;
        const int r1 = ops.run(B, st);
        return r1 ? r1 : op3.run(B, st);
    }, OP_CONV, op3.name + " + shortcut", op3.flops + ops.flops, 1});
}

// GroupNorm(32) + ReLU from `in` into `out` (possibly a concat slice); names = norm key prefixes per group
void Builder::gn_relu(const std::vector<std::string>& names, const View& in, const View& out, bool single_consumer) {
    const int G = (int)names.size(), C = in.C;
    std::vector<float> gamma, beta;
    for (int g = 0; g < G; ++g) {
        const float* w = hw(names[g] + ".weight", C);
        const float* b = hw(names[g] + ".bias", C);
        if (dry || !w || !b) continue;
        gamma.insert(gamma.end(), w, w + C);
        beta.insert(beta.end(), b, b + C);
    }
    if (dry) return;
    const float* dg = upload(gamma);
    const float* db = upload(beta);
    // every GroupNorm owns a slot of the sum accumulators; one launch at the start of the forward clears them all
    if (c->gn_slots >= GN_SLOTS) { if (err.empty()) err = "more GroupNorm layers than accumulator slots"; return; }
    double* stats = c->gn_stats + (size_t)c->gn_slots++ * gn_slot_doubles(c->cfg.max_batch);
    // the producer is the convolution emitted just before: it accumulates the sums while it stores its output
    const bool fused = last_conv.fuse && last_conv.out == in.p && last_conv.G == G && last_conv.C == C;
    if (fused) {
        last_conv.fuse->sums = stats;
        last_conv.fuse->groups = 32;
        last_conv.fuse.reset();
    }
    std::shared_ptr<DeferredNorm> dn;
    if (single_consumer && C % 32 == 0 && (C / 32) % 4 == 0) {
        dn = std::make_shared<DeferredNorm>();
        dn->in = in; dn->out = out; dn->stats = stats; dn->gamma = dg; dn->beta = db; dn->C = C; dn->G = G;
    }
    pending_norm = dn;
    c->ops.push_back({[=](int B, hipStream_t st) {
        if (!fused) {
            int rc = launch_gn_stats(in, B, G, 32, stats, st, false);
            if (rc) return rc;
        }
        if (dn && dn->absorbed) return 0;      // the consumer normalises while it loads
        return launch_gn_apply(in, out, B, G, 32, stats, dg, db, C, 1e-5f, 1, st);
    }, OP_NORM, names[0], 0.0, fused ? 1 : 2});
    c->ops.back().lane = cur_lane;
}

void Builder::op(std::function<int(int, hipStream_t)> f) {
    if (!dry) c->ops.push_back({std::move(f), OP_OTHER, "elementwise", 0.0, 1, cur_lane});
}
// Side lanes.  fork(L): the ops emitted until join(L) with cur_lane = L form a branch that depends on nothing emitted after
// this point and whose results nothing needs before join(L): at small batches, where a launch fills a fraction of the chip,
// quber_forward runs it on a stream of its own beside what the main stream does meanwhile (the fusion convolutions of res2
// and res3 beside the later ResNet stages).
void Builder::fork(int L) {
    if (dry) return;
    c->ops.push_back({nullptr, OP_OTHER, "fork", 0.0, 0, L, 1});
    cur_lane = L;
    c->lanes_built = true;
}
void Builder::join(int L) {
    if (dry) return;
    c->ops.push_back({nullptr, OP_OTHER, "join", 0.0, 0, L, 2});
}

// conv (no bias) -> GN -> ReLU, the [d2] Conv2d(norm=GN, activation=relu) pattern
void Builder::conv_gn(const std::string& n, const View& in, const View& tmp, const View& out, int k, int dil, bool single_consumer, int cin_real) {
    conv({n}, in, cin_real > 0 ? cin_real : in.C, tmp, k, 1, k == 3 ? dil : 0, dil, AF_NONE, nullptr, false);
    gn_relu({n + ".norm"}, tmp, out, single_consumer);
}

// a3 + stem.conv1 as one kernel (csrc/stem.hip): names = the conv's key prefix per stream; out = [NS][Bmax][h2][w2][32]
void Builder::emit_stem_fused(const std::vector<std::string>& names, const View& out) {
    const int G = (int)names.size();
    std::vector<float> packed((size_t)G * 9 * 6 * 32), scale((size_t)G * 32, 1.f), shift((size_t)G * 32, 0.f);
    bool ok = true;
    for (int g = 0; g < G; ++g) {
        const std::string& n = names[g];
        const float* w = hw(n + ".weight", (int64_t)32 * 6 * 9);
        const BnFold bn = frozen_bn(*this, n, 32);
        if (dry) continue;
        if (!w || !bn.ok()) { ok = false; continue; }
        for (int o = 0; o < 32; ++o) {
            for (int ci = 0; ci < 6; ++ci)
                for (int t = 0; t < 9; ++t) {
                    const float v = w[((size_t)o * 6 + ci) * 9 + t];
                    packed[(((size_t)g * 9 + t) * 6 + ci) * 32 + o] = out.es == 2 ? (float)(_Float16)v : v;      // fp16 data path: the operand the MFMA kernel multiplies
                }
            const float sc = bn.scale(o);
            scale[(size_t)g * 32 + o] = sc;
            shift[(size_t)g * 32 + o] = bn.shift(o, sc);
        }
    }
    if (dry || !ok) return;
    const int OH = (H + 1) / 2, OW = (W + 1) / 2;
    if (out.C != 32 || out.cs != 32 || out.H != OH || out.W != OW || (out.es != 4 && out.es != 2)) { if (err.empty()) err = "internal: fused stem output geometry"; return; }
    const double fl = 2.0 * OH * OW * 6.0 * 9.0 * 32.0 * G;
    c->flops += fl;
    const float *dw = upload(packed), *ds = upload(scale), *dh = upload(shift);
    // fp16 data path: the filters as fragments of v_mfma_f32_16x16x32_f16 (stem.hip): [stream][tile jj][k-step][lane][8 halfs], lane (fr, fq) =
    // output channel 8 (fr >> 2) + 4 jj + (fr & 3), tap 4 ks + fq, channels 0-5 (6, 7 and taps 9-11: zeros)
    const float* dwf = nullptr;
    if (out.es == 2 && tune().stem_fused != 2) {
        std::vector<_Float16> wf((size_t)G * 2 * 3 * 64 * 8, (_Float16)0.f);
        for (int g = 0; g < G; ++g)
            for (int jj = 0; jj < 2; ++jj)
                for (int ks = 0; ks < 3; ++ks)
                    for (int l = 0; l < 64; ++l) {
                        const int fr = l & 15, tap = 4 * ks + (l >> 4), n = 8 * (fr >> 2) + 4 * jj + (fr & 3);
                        if (tap < 9)
                            for (int ci = 0; ci < 6; ++ci)
                                wf[((((size_t)g * 2 + jj) * 3 + ks) * 64 + l) * 8 + ci] = (_Float16)packed[(((size_t)g * 9 + tap) * 6 + ci) * 32 + n];
                    }
        dwf = upload16(wf);
    }
    quber_ctx* ctx = c;
    const View o = out;
    c->stem_fused = true;
    c->ops.push_back({[=](int B, hipStream_t st) {
        return launch_stem_conv1(ctx->cur_bgr, ctx->cur_depth, ctx->cur_off, B, ctx->cfg.height, ctx->cfg.width, G, ctx->cfg.pixel_mean,
                                 ctx->cfg.pixel_std, dw, ds, dh, o.p, o.gs, o.es, st, dwf);
    }, OP_CONV, names[0], fl, 1});
    last_conv = {nullptr, nullptr, 0, 0};
    pending_norm.reset();
}

void Builder::build() {
    const quber_config& cf = c->cfg;
    const int* nb = cf.resnet_depth == 50 ? BLOCKS50 : cf.resnet_depth == 101 ? BLOCKS101 : BLOCKS152;
    // stride-2 stages round up (3x3/s2/p1 conv and pool: out = floor((in - 1) / 2) + 1; strided 1x1: the same)
    const int h2 = (H + 1) / 2, w2 = (W + 1) / 2, h4 = (h2 + 1) / 2, w4 = (w2 + 1) / 2;
    const int h8 = (h4 + 1) / 2, w8 = (w4 + 1) / 2, h16 = (h8 + 1) / 2, w16 = (w8 + 1) / 2;
    const std::string R = "backbone.rgb_backbone.", D = "backbone.depth_backbone.";
    const int NS = cf.streams;   // 2: rgb + depth streams with concat fusion; 1: a single ResNet (rgb-only / depth-only)
    auto two = [&](const std::string& tail, bool stage_prefix) -> std::vector<std::string> {
        if (NS == 1) return {"backbone." + tail};
        return {R + tail, D + (stage_prefix ? "depth_" : "") + tail};
    };
    if (!dry) {
        c->gn_stats = (double*)dalloc_bytes(sizeof(double) * GN_SLOTS * gn_slot_doubles(Bmax));
        quber_ctx* ctx = c;
        // (on side lane 2, joined where lane 1 is first forked - long before the first kernel that accumulates into the sums: at small
        // batches the stem starts at once instead of behind a 5 us fill)
        fork(2);
        op([ctx](int, hipStream_t st) {
            return launch_zero(ctx->gn_stats, sizeof(double) * ctx->gn_slots * gn_slot_doubles(ctx->cfg.max_batch), st);
        });
        back_to_main();
    }
    if (!dry) {
        c->splitk_floats = (size_t)40 << 20;   // 160 MiB of partial tiles: S x blocks stays near 1-2 rounds of 128x128 tiles at any batch
        c->splitk_ws = (float*)dalloc_bytes(sizeof(float) * c->splitk_floats);
    }

    // ---------------- input + stems (both streams as G = 2) ----------------
    // (fp16 data path: 16 channels - the loader steps through a filter tap in units of 8 four-byte words)
    // fp32 tensors (exact fp32 and bf16x3 modes): a3 runs inside the first convolution's kernel - the normalised 8-channel input
    // (315 MB per 16-frame step) is neither written nor read back (option key 29)
    // fp16 tensors: the same kernel on the fp16-rounded operands (no 16-channel fp16 input tensor, no zero channels multiplied)
    // (the fused kernel is exact fp32 arithmetic with one fold per K-slice - what the implicit GEMM does in the exact and bf16x3 modes and,
    //  on the fp16-rounded operands, in the fp16 data path; bf16 / fp16 OPERANDS on fp32 tensors - compute_dtype 1, or 2 without the
    //  fp16 tensors - keep the preprocess kernel + implicit GEMM, so that option 29 never changes a mode's arithmetic)
    const bool stem_one = tune().stem_fused != 0 && !(aes == 4 && (cf.compute_dtype == 1 || cf.compute_dtype == 2));
    View s1 = make(32, h2, w2, NS), s2 = make(32, h2, w2, NS), s3 = make(64, h2, w2, NS);
    if (stem_one) {
        emit_stem_fused(two("stem.conv1", false), s1);
    } else {
        View X = make(aes == 2 ? 16 : 8, H, W, NS);
        if (!dry) c->X = X;
        conv(two("stem.conv1", false), X, 6, s1, 3, 2, 1, 1, AF_FROZEN_BN, nullptr, true);
    }
    if (!dry) c->taps["stem1"] = s1;
    conv(two("stem.conv2", false), s1, 32, s2, 3, 1, 1, 1, AF_FROZEN_BN, nullptr, true);
    conv(two("stem.conv3", false), s2, 32, s3, 3, 1, 1, 1, AF_FROZEN_BN, nullptr, true);
    View x = make(64, h4, w4, NS);
    op([=](int B, hipStream_t st) { return launch_maxpool3x3s2(s3, x, B, NS, st); });

    // ---------------- res2..res5 ----------------
    View cat[4];  // concatenated [rgb | depth] stage outputs
    // ---------------- backbone fusion (resnet.py:472-485), emitted right after its stage ----------------
    View F[4];
    const int fch[4] = {256, 512, 1024, 2048};
    auto emit_fusion = [&](int s) {
        if (NS == 1) {   // build_resnet_deeplab_fusion_backbone: the stage outputs feed the head directly
            F[s] = cat[s];
            if (!dry) c->taps["res" + std::to_string(s + 2)] = F[s];
            return;
        }
        const std::string n = "backbone.fusion_res" + std::to_string(s + 2) + ".";
        const int C = fch[s], fh = cat[s].H, fw = cat[s].W;
        View t = make(C, fh, fw), a = make(C, fh, fw);
        if (cf.fusion_add) {   // FUSION_STRATEGY "add" (resnet.py:502-503): rgb + depth, no 1x1 reduction
            View ra = slice(cat[s], 0, C), rb = slice(cat[s], C, C);
            op([=](int B, hipStream_t st) { return launch_add_channels(ra, rb, a, B, st); });
        } else {
            conv({n + "conv"}, cat[s], 2 * C, t, 1, 1, 0, 1, AF_BIAS, nullptr, false);
            gn_relu({n + "gn"}, t, a, s != 3 && cf.backbone_fusion_layers > 0);   // read only by conv0 below
        }
        if (s != 3) {
            // a convolution that absorbs the GroupNorm before it reads that norm's INPUT (the previous convolution's raw
            // output): raw outputs alternate between two buffers so that no layer reads the tensor it writes (the
            // single-kernel Winograd layer reads input halos while other blocks store)
            View b2 = make(C, fh, fw), t2 = make(C, fh, fw);
            View cur = a, nxt = b2, traw = t2, tprev = t;
            for (int i = 0; i < cf.backbone_fusion_layers; ++i) {
                conv({n + "conv" + std::to_string(i)}, cur, C, traw, 3, 1, 1, 1, AF_BIAS, nullptr, false);
                gn_relu({n + "gn" + std::to_string(i)}, traw, nxt, i + 1 < cf.backbone_fusion_layers);   // read only by the next conv
                std::swap(cur, nxt);
                std::swap(traw, tprev);
            }
            a = cur;
        }
        F[s] = a;
        if (!dry) c->taps["res" + std::to_string(s + 2)] = a;
    };
    // decoder inputs that depend on ONE fused stage output only - the 1x1 projections of res3 / res2 (+ GroupNorm) into their slice of the
    // decoder's concatenated buffers - are emitted on that stage's side lane, right behind its fusion convolutions: at small batches
    // they are off the caller's stream altogether (2 x ~30 us per batch-1 forward)
    const std::string Hd = "ins_embed_head.";
    const int CD = cf.convs_dim, HC = cf.head_channels;      // INS_EMBED_HEAD.CONVS_DIM / HEAD_CHANNELS (128 / 32)
    View cat3 = make(64 + 256, h8, w8), t64 = make(64, h8, w8);
    // (fp16 data path: 160 -> 192 channels per pixel, the last 32 never written = zero, zero filters for them: whole 64-channel blocks for the patch kernel)
    View cat2 = make(aes == 2 ? (32 + CD + 63) / 64 * 64 : 32 + CD, h4, w4), t32 = make(32, h4, w4);
    int cin = 64, cout = 256, mid = 64, ch = h4, cw = w4;
    for (int s = 0; s < 4; ++s) {
        const int stage = s + 2;
        const int sdil = stage == 5 ? cf.res5_dilation : 1;
        const int first = (s == 0 || sdil > 1) ? 1 : 2;
        const int oh = first == 2 ? (ch + 1) / 2 : ch, ow = first == 2 ? (cw + 1) / 2 : cw;
        View t1 = make(mid, oh, ow, NS), t2 = make(mid, oh, ow, NS), sc = make(cout, oh, ow, NS);
        View oa = make(cout, oh, ow, NS), ob = make(cout, oh, ow, NS);
        const bool tapped = stage != 4;
        if (tapped) {
            View cb = make(NS * cout, oh, ow, 1);
            cat[s] = cb;
        }
        static const int mg[3] = {1, 2, 4};
        for (int i = 0; i < nb[s]; ++i) {
            const int stride = i == 0 ? first : 1;
            const int dil = stage == 5 ? sdil * mg[i % 3] : 1;
            const std::string tail = "res" + std::to_string(stage) + "." + std::to_string(i) + ".";
            const bool last = i == nb[s] - 1;
            View out = (last && tapped) ? slice(cat[s], 0, cout, cout) : ((i & 1) ? ob : oa);
            conv(two(tail + "conv1", true), x, cin, t1, 1, stride, 0, 1, AF_FROZEN_BN, nullptr, true);
            conv(two(tail + "conv2", true), t1, mid, t2, 3, 1, dil, dil, AF_FROZEN_BN, nullptr, true);
            View resv = x;
            if (cin != cout) {
                conv(two(tail + "shortcut", true), x, cin, sc, 1, stride, 0, 1, AF_FROZEN_BN, nullptr, false);
                resv = sc;
            }
            conv(two(tail + "conv3", true), t2, mid, out, 1, 1, 0, 1, AF_FROZEN_BN, &resv, true);
            if (cin != cout) fuse_shortcut(two(tail + "conv3", true), two(tail + "shortcut", true), t2, mid, x, cin, stride, out);
            x = out;
            cin = cout;
        }
        ch = oh; cw = ow;
        cout *= 2; mid *= 2;
        // the fusion convolutions of this stage's output: a side lane for res2 / res3 (they run beside the later stages at small
        // batches and are joined where the decoder first reads them), the main stream for res5 (the ASPP waits for it anyway)
        if (s == 0 || s == 1) {
            if (s == 0) join(2);          // the cleared GroupNorm sums: every accumulating kernel is launched behind this point
            fork(1 + s);
            emit_fusion(s);
            if (s == 1) conv_gn(Hd + "decoder.res3.project_conv", F[1], t64, slice(cat3, 0, 64), 1, 1);
            else conv_gn(Hd + "decoder.res2.project_conv", F[0], t32, slice(cat2, 0, 32), 1, 1);
            back_to_main();
        } else if (s == 3) {
            emit_fusion(3);
        }
    }

    // ---------------- decoder ([d2] DeepLabV3PlusHead.layers) ----------------
    const std::string A = Hd + "decoder.res5.project_conv.";
    View catA = make(1280, h16, w16), tA = make(256, h16, w16);
    // the image-pooling branch (global average -> 1x1 -> broadcast) on side lane 2 (idle since fusion_res3): four latency-bound launches
    // beside the other branches instead of in front of the projection
    fork(2);
    {
        View pooled = make(2048, 1, 1), pc = make(256, 1, 1);
        View f5 = F[3];
        op([=](int B, hipStream_t st) { return launch_avgpool(f5, pooled, B, st); });
        conv({A + "convs.4.1"}, pooled, 2048, pc, 1, 1, 0, 1, AF_BIAS, nullptr, true);
        View dst = slice(catA, 1024, 256);
        op([=](int B, hipStream_t st) { return launch_bilinear(pc, dst, B, st); });
    }
    back_to_main();
    conv_gn(A + "convs.0", F[3], tA, slice(catA, 0, 256), 1, 1);
    const int adil[3] = {6, 12, 18};
    // (round 2 measured the three dilated branches on lanes of their own in the bf16x3 mode: 3.92 against 3.85 ms; round 6, exact fp32, two
    // of them on the lanes that the fusion convolutions have long left: 3.74 -> 3.70 ms - key 41)
    // fp16 data path on maps large enough that no branch skips padded filter rows: the three dilated branches as ONE grouped launch
    // (they read the same tensor; per-group dilation, ConvP::dil_g) - 3 x 128 tiles at 1024x1024 batch 8 instead of three launches
    // that each leave half of conv_h8.hip's one-block-per-CU grid empty
    const int aspp_oh = F[3].H;
    const bool aspp_grouped = aes == 2 && tune().h8 && 10 * 2 * adil[2] < 2 * 3 * aspp_oh;
    if (aspp_grouped) {
        View tA3 = make(256, h16, w16, 3);
        View xin = F[3];
        xin.gs = 0;
        const std::vector<std::string> an = {A + "convs.1", A + "convs.2", A + "convs.3"};
        conv(an, xin, F[3].C, tA3, 3, 1, adil[2], adil[2], AF_NONE, nullptr, false, {adil[0], adil[1], adil[2]});
        gn_relu({an[0] + ".norm", an[1] + ".norm", an[2] + ".norm"}, tA3, slice(catA, 256, 256, 256));
    } else if (tune().aspp_lanes) {
        // key 41: the dilated branches d = 6 / 12 on the two side lanes (temporaries of their own), d = 18 on the caller's stream
        View tA1 = make(256, h16, w16), tA2 = make(256, h16, w16);
        fork(1);
        conv_gn(A + "convs.1", F[3], tA1, slice(catA, 256, 256), 3, adil[0]);
        back_to_main();
        fork(2);
        conv_gn(A + "convs.2", F[3], tA2, slice(catA, 512, 256), 3, adil[1]);
        back_to_main();
        conv_gn(A + "convs.3", F[3], tA, slice(catA, 768, 256), 3, adil[2]);
        join(1);
    } else {
        for (int i = 0; i < 3; ++i) conv_gn(A + "convs." + std::to_string(i + 1), F[3], tA, slice(catA, 256 * (i + 1), 256), 3, adil[i]);
    }
    join(2);                         // fusion_res3 + decoder.res3.project_conv + the pooling branch
    View y5 = make(256, h16, w16);
    conv_gn(A + "project", catA, tA, y5, 1, 1);

    View t128a = make(CD, F[1].H, F[1].W);
    {
        View dst = slice(cat3, 64, 256);
        op([=](int B, hipStream_t st) { return launch_bilinear(y5, dst, B, st); });
    }
    View u3 = make(CD, F[1].H, F[1].W), y3 = make(CD, F[1].H, F[1].W);
    conv_gn(Hd + "decoder.res3.fuse_conv.0", cat3, t128a, u3, 3, 1, true);    // u3 is read only by fuse_conv.1
    View t128b = make(CD, F[1].H, F[1].W);           // (not t128a: fuse_conv.1 reads it - the absorbed norm's input)
    conv_gn(Hd + "decoder.res3.fuse_conv.1", u3, t128b, y3, 3, 1);

    // ---------------- prediction heads: generic hierarchy (model.py:738-762) ----------------
    // head ids: 0 foreground, 1 center, 2 offset, 3 eee_mask, 4 eee_boundary
    static const char* HN[5] = {"foreground", "center", "offset", "eee_mask", "eee_boundary"};
    const int ncls = cf.error_classes;
    const int hch[5] = {1, 1, 2, ncls, ncls};
    const int hplane[5] = {0, 1, 2, QUBER_LOGIT_BASE + (cf.eee_boundary_on ? ncls : 0), QUBER_LOGIT_BASE};
    const bool enabled[5] = {true, true, true, cf.eee_mask_on != 0, cf.eee_boundary_on != 0};
    std::vector<std::vector<int>> levels;
    if (cf.hierarchical) {
        for (int i = 0; i < cf.n_levels; ++i) {
            std::vector<int> l;
            for (int j = 0; j < 5 && cf.level_heads[i][j] >= 0; ++j) l.push_back(cf.level_heads[i][j]);
            levels.push_back(l);
        }
    } else {
        std::vector<int> l;
        for (int k : {3, 4, 0, 1, 2})
            if (enabled[k]) l.push_back(k);
        levels.push_back(l);
    }
    const int nlev = (int)levels.size();
    // concatenated fusion inputs y | feats(prev level) | activations(prev level), one per level >= 1
    std::vector<View> YP(nlev);
    std::vector<int> ypw(nlev, 0);
    for (int i = 1; i < nlev; ++i) {
        int wd = CD;
        if (cf.fusion_feat) wd += HC * (int)levels[i - 1].size();
        if (cf.fusion_pred)
            for (int k : levels[i - 1]) wd += hch[k];
        ypw[i] = wd;
        // whole 16-byte units per pixel; fp16 data path: whole 64-channel K-tiles (164 -> 192: the zero channels meet zero filters), so that the
        // 1x1 reduction in front of the head-fusion stack runs on conv_h8.hip
        YP[i] = make(aes == 2 ? (wd + 63) / 64 * 64 : (wd + 3) / 4 * 4, h4, w4);
    }
    View t128 = make(CD, h4, w4);
    join(1);                         // fusion_res2 + decoder.res2.project_conv
    {
        View dst = slice(cat2, 32, CD);
        op([=](int B, hipStream_t st) { return launch_bilinear(y3, dst, B, st); });
    }
    View u2 = make(CD, h4, w4);
    conv_gn(Hd + "decoder.res2.fuse_conv.0", cat2, t128, u2, 3, 1, true, 32 + CD);      // u2 is read only by fuse_conv.1
    View y = nlev > 1 ? slice(YP[1], 0, CD) : make(CD, h4, w4);
    View t128c = make(CD, h4, w4);                   // (not t128: fuse_conv.1 reads it - the absorbed norm's input)
    conv_gn(Hd + "decoder.res2.fuse_conv.1", u2, t128c, y, 3, 1);
    for (int i = 2; i < nlev; ++i) {
        View dst = slice(YP[i], 0, CD);
        op([=](int B, hipStream_t st) { return launch_copy_channels(y, dst, B, st); });
    }
    if (!dry) c->taps["y"] = y;

    const int planes = QUBER_LOGIT_BASE + ncls * ((cf.eee_mask_on ? 1 : 0) + (cf.eee_boundary_on ? 1 : 0));
    if (!dry) c->q = (float*)dalloc_bytes(sizeof(float) * (size_t)Bmax * planes * h4 * w4);
    float* q = c->q;
    for (int i = 0; i < nlev; ++i) {
        const int G = (int)levels[i].size();
        View x = y;
        if (i > 0) {
            // FusionLayers_i (model.py:424-458), evaluated once (the reference re-runs it per key, model.py:760-762)
            const std::string FL = Hd + "fusion_layers_" + std::to_string(i) + ".fusion_layers.";
            View za = make(CD, h4, w4), zb = make(CD, h4, w4);
            conv({FL + "0"}, YP[i], ypw[i], za, 1, 1, 0, 1, AF_BIAS_BN, nullptr, true);
            View cur = za, nxt = zb;
            for (int j = 0; j < cf.head_fusion_layers; ++j) {
                conv({FL + std::to_string(j + 1)}, cur, CD, nxt, 3, 1, 1, 1, AF_BIAS_BN, nullptr, true);
                std::swap(cur, nxt);
            }
            x = cur;
            if (!dry) c->taps["z" + std::to_string(i)] = x;
        }
        std::vector<std::string> h0, h1, n0, n1;
        for (int k : levels[i]) {
            h0.push_back(Hd + HN[k] + "_pred_head.head.0");
            h1.push_back(Hd + HN[k] + "_pred_head.head.1");
            n0.push_back(h0.back() + ".norm");
            n1.push_back(h1.back() + ".norm");
        }
        View g128 = make(CD, h4, w4, G), g128n = make(CD, h4, w4, G), g32 = make(HC, h4, w4, G);
        const bool next = i + 1 < nlev;
        View feat = (next && cf.fusion_feat) ? slice(YP[i + 1], CD, HC, HC) : make(HC, h4, w4, G);
        View xin = x;
        xin.gs = 0;   // every head of the level reads the same features
        conv(h0, xin, CD, g128, 3, 1, 1, 1, AF_NONE, nullptr, false);
        gn_relu(n0, g128, g128n, true);          // g128n is read only by head.1
        conv(h1, g128n, CD, g32, 3, 1, 1, 1, AF_NONE, nullptr, false);
        gn_relu(n1, g32, feat);
        int act_off = CD + (cf.fusion_feat ? HC * G : 0);
        PredHeads ph{};
        int ph_act_cs = 0;
        for (int j = 0; j < G; ++j) {
            const int k = levels[i][j];
            const float* pw = hw(Hd + HN[k] + "_predictor.predictor.weight", (int64_t)hch[k] * HC);
            const float* pb = hw(Hd + HN[k] + "_predictor.predictor.bias", hch[k]);
            View in = feat;
            in.p = feat.at((long)j * feat.gs);
            if (!dry) c->taps[std::string("feat_") + HN[k]] = in;
            float* act_dst = nullptr;
            int act_cs = 0;
            if (next && cf.fusion_pred) {
                act_dst = YP[i + 1].at(act_off);
                act_cs = YP[i + 1].cs;
                act_off += hch[k];
            }
            if (dry || !pw || !pb) continue;
            const float* dw = upload(std::vector<float>(pw, pw + hch[k] * HC));
            const float* db = upload(std::vector<float>(pb, pb + hch[k]));
            ph.in[ph.n] = in.p; ph.w[ph.n] = dw; ph.bias[ph.n] = db; ph.sm[ph.n] = act_dst; ph.cout[ph.n] = hch[k];
            ph.q_ch0[ph.n] = hplane[k]; ph.act[ph.n] = act_dst ? (k >= 3 ? 1 : 2) : 0;
            if (act_dst) ph_act_cs = act_cs;
            ++ph.n;
        }
        if (!dry && ph.n == G) {         // every predictor of the level in one launch
            const int fcs = feat.cs, fes = feat.es, fh = feat.H, fw = feat.W;
            op([=](int B, hipStream_t st) { return launch_predictors(ph, HC, fcs, fes, fh, fw, q, planes, ph_act_cs, B, st); });
        }
    }
    // x4 bilinear of every plane, offsets scaled by the stride (model.py:689-708)
    quber_ctx* ctx = c;
    op([=](int B, hipStream_t st) {
        return launch_upsample_logits(q, ctx->cur_out, B, planes, h4, w4, 4, ctx->cfg.height, ctx->cfg.width, 0xCu, st);
    });
}

}  // namespace quber
