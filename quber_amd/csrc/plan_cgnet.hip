// ------------------------------------------------------------------------------------------------
// CGNet launch plan (reference foreground_segmentation/cgnet.py:275-368, classes = 2, in_channel = 4, M = 3, N = 21; keys = that
// module's state_dict keys).  Option key 52 (cgnet_fused): 1 = a context-guided block is cg_joint + cg_apply (cgnet.hip),
// 0 = 1x1 convolution + two depthwise launches + cg_sums + cg_apply, the bring-up path and the second arm of the A/B.
#include "plan.h"

namespace quber {
namespace {

struct BnP {   // folded BatchNorm(eps 1e-3) + PReLU vectors
    std::vector<float> scale, shift, slope;
};
struct DevBnP { const float *scale = nullptr, *shift = nullptr, *slope = nullptr; };

struct CgBuilder {
    Builder& b;
    quber_ctx* c;
    bool dry;
    double* partials = nullptr;       // tile sums, shared by every block (the stream orders them): [Bmax][tiles of the 1/4 map][128]
    explicit CgBuilder(Builder& bb) : b(bb), c(bb.c), dry(bb.dry) {}

    // a named intermediate (quber_debug_tensor).  `buf`: the wide buffer a channel slice lives in, registered as <name>.buf
    void tap(const std::string& n, const View& v, const View* buf = nullptr) {
        if (dry) return;
        c->taps[n] = v;
        if (buf) c->taps[n + ".buf"] = *buf;
    }
    void op(const std::string& n, std::function<int(int, hipStream_t)> f) {
        b.op(std::move(f));
        if (!dry) c->ops.back().name = n;
    }
    View array_view(float* p, int C) {     // [Bmax][1][1][C]
        View v;
        v.p = p; v.B = b.Bmax; v.H = 1; v.W = 1; v.C = C; v.cs = C; v.gs = (long)b.Bmax * C;
        return v;
    }

    // BN under `bn`.{weight, bias, running_mean, running_var}, PReLU under `act`.weight
    BnP bnp(const std::string& bn, const std::string& act, int C) {
        BnP r;
        const float* w = b.hw(bn + ".weight", C);
        const float* bi = b.hw(bn + ".bias", C);
        const float* m = b.hw(bn + ".running_mean", C);
        const float* v = b.hw(bn + ".running_var", C);
        const float* a = b.hw(act + ".weight", C);
        r.scale.assign(C, 1.f); r.shift.assign(C, 0.f); r.slope.assign(C, 0.f);
        if (dry || !w || !bi || !m || !v || !a) return r;
        for (int i = 0; i < C; ++i) {
            r.scale[i] = w[i] * (1.0f / sqrtf(v[i] + 1e-3f));
            r.shift[i] = bi[i] - m[i] * r.scale[i];
            r.slope[i] = a[i];
        }
        return r;
    }
    static BnP cut(const BnP& e, int lo, int n) {      // channels lo .. lo + n: the slice a depthwise launch folds into its epilogue
        auto part = [lo, n](const std::vector<float>& v) { return std::vector<float>(v.begin() + lo, v.begin() + lo + n); };
        return BnP{part(e.scale), part(e.shift), part(e.slope)};
    }
    DevBnP up(const BnP& e) { return dry ? DevBnP() : DevBnP{b.upload(e.scale), b.upload(e.shift), b.upload(e.slope)}; }
    const float* up(const float* w, size_t n) { return (dry || !w) ? nullptr : b.upload(std::vector<float>(w, w + n)); }

    // dense convolution n.conv.weight [+ BN + PReLU n.bn.*, n.act.weight]
    void conv(const std::string& n, const View& in, int cin_real, const View& out, int k, int stride, bool act, const View* buf = nullptr) {
        const float* w = b.hw(n + ".conv.weight", (int64_t)out.C * cin_real * k * k);
        BnP e;
        if (act) e = bnp(n + ".bn", n + ".act", out.C);
        b.emit_conv(n, {w}, in, cin_real, out, k, stride, k == 3 ? 1 : 0, 1, act, e.scale, e.shift, act ? e.slope : std::vector<float>(), nullptr, false);
        tap(n, out, buf);
    }
    // depthwise 3x3 n.conv.weight with channels lo.. of a concatenation's BN + PReLU folded into its epilogue
    void dwconv(const std::string& n, const View& in, const View& out, int dil, const BnP& e) {
        const float* w = b.hw(n + ".conv.weight", (int64_t)in.C * 9);
        const float* dw = up(w, (size_t)in.C * 9);
        const DevBnP d = up(e);
        if (dry || !w) return;
        op(n, [=](int B, hipStream_t st) { return launch_dwconv3x3(in, out, B, dil, dw, d.scale, d.shift, d.slope, st); });
        tap(n, out);
    }
    void affine(const std::string& n, const View& a, const View& out, const View* buf) {
        const DevBnP d = up(bnp(n + ".bn", n + ".act", a.C));
        if (dry) return;
        op(n, [=](int B, hipStream_t st) { return launch_affine_prelu(a, nullptr, out, B, d.scale, d.shift, d.slope, st); });
        tap(n, out, buf);
    }
    void pool(const std::string& n, const View& in, const View& out, const View* buf = nullptr) {
        op(n, [=](int B, hipStream_t st) { return launch_pool_s2(in, out, B, 0, st); });
        tap(n, out, buf);
    }
    // FGlo (cgnet.py:174-192) of `feat` [+ residual x] -> out: the apply launch over tile sums that `tiles` describes
    void glo(const std::string& n, const View& feat, const View* x, const View& out, int r, int tiles) {
        const int C = feat.C, R = C / r;
        const float* f0 = up(b.hw(n + ".F_glo.fc.0.weight", (int64_t)R * C), (size_t)R * C);
        const float* b0 = up(b.hw(n + ".F_glo.fc.0.bias", R), R);
        const float* f2 = up(b.hw(n + ".F_glo.fc.2.weight", (int64_t)C * R), (size_t)C * R);
        const float* b2 = up(b.hw(n + ".F_glo.fc.2.bias", C), C);
        if (dry || !f0 || !b0 || !f2 || !b2) return;
        float* mean = (float*)b.dalloc_bytes(sizeof(float) * (size_t)b.Bmax * C);
        float* y = (float*)b.dalloc_bytes(sizeof(float) * (size_t)b.Bmax * C);
        double* pp = partials;
        const bool has = x != nullptr;
        const View xv = has ? *x : View();
        op(n, [=](int B, hipStream_t st) { return launch_cg_apply(feat, has ? &xv : nullptr, out, B, R, pp, tiles, f0, b0, f2, b2, mean, y, st); });
        tap(n + ".F_glo.mean", array_view(mean, C));
        tap(n + ".F_glo.y", array_view(y, C));
        tap(n, out);
    }
    void sums(const std::string& n, const View& feat) {
        if (dry) return;
        double* pp = partials;
        const int tiles = cg_sums_tiles(feat.H, feat.W);
        op(n + ".F_glo.sums", [=](int B, hipStream_t st) { return launch_cg_sums(feat, B, pp, tiles, st); });
    }
    // ContextGuidedBlock_Down (cgnet.py:194-228): 3x3 stride 2 + BN + PReLU, both depthwise 3x3 into one buffer with the block's BN + PReLU
    // folded by channel slice, 1x1 reduce, FGlo over the output of reduce
    void down(const std::string& n, const View& in, int cin_real, const View& out, int dil, int r) {
        const int C = out.C, h = out.H, w = out.W;
        View t = b.make(C, h, w), cat = b.make(2 * C, h, w), red = b.make(C, h, w);
        conv(n + ".conv1x1", in, cin_real, t, 3, 2, true);
        const BnP e = bnp(n + ".bn", n + ".act", 2 * C);
        dwconv(n + ".F_loc", t, Builder::slice(cat, 0, C), 1, cut(e, 0, C));
        dwconv(n + ".F_sur", t, Builder::slice(cat, C, C), dil, cut(e, C, C));
        conv(n + ".reduce", cat, 2 * C, red, 1, 1, false);
        sums(n, red);
        glo(n, red, nullptr, out, r, cg_sums_tiles(h, w));
    }
    // ContextGuidedBlock (cgnet.py:231-261)
    void block(const std::string& n, const View& x, const View& out, int dil, int r, bool fused) {
        const int C = x.C, CH = C / 2, h = x.H, w = x.W;
        View joi = b.make(C, h, w);
        const BnP e2 = bnp(n + ".bn_prelu.bn", n + ".bn_prelu.act", C);
        if (fused) {
            const float* w1h = b.hw(n + ".conv1x1.conv.weight", (int64_t)CH * C);
            const DevBnP d1 = up(bnp(n + ".conv1x1.bn", n + ".conv1x1.act", CH));
            const float* wl = up(b.hw(n + ".F_loc.conv.weight", (int64_t)CH * 9), (size_t)CH * 9);
            const float* ws = up(b.hw(n + ".F_sur.conv.weight", (int64_t)CH * 9), (size_t)CH * 9);
            const DevBnP d2 = up(e2);
            const float* w1 = up(w1h, (size_t)CH * C);
            const int tiles = cg_joint_tiles(h, w);
            if (!dry && w1 && wl && ws) {
                double* pp = partials;
                c->flops += 2.0 * h * w * (double)C * CH;
                op(n + ".joi", [=](int B, hipStream_t st) {
                    return launch_cg_joint(x, joi, B, dil, w1, d1.scale, d1.shift, d1.slope, wl, ws, d2.scale, d2.shift, d2.slope, pp, tiles, st);
                });
                tap(n + ".joi", joi);
            }
            glo(n, joi, &x, out, r, tiles);
        } else {
            View t = b.make(CH, h, w);
            conv(n + ".conv1x1", x, C, t, 1, 1, true);
            dwconv(n + ".F_loc", t, Builder::slice(joi, 0, CH), 1, cut(e2, 0, CH));
            dwconv(n + ".F_sur", t, Builder::slice(joi, CH, CH), dil, cut(e2, CH, CH));
            tap(n + ".joi", joi);
            sums(n, joi);
            glo(n, joi, &x, out, r, cg_sums_tiles(h, w));
        }
    }

    void build() {
        const int H = b.H, W = b.W, h2 = H / 2, w2 = W / 2, h4 = H / 4, w4 = W / 4, h8 = H / 8, w8 = W / 8;
        const int ncls = 2, cin = 4, M = 3, N = 21;
        const bool fused = tune().cgnet_fused != 0;
        if (!dry) partials = (double*)b.dalloc_bytes(sizeof(double) * (size_t)b.Bmax * cg_joint_tiles(h4, w4) * 128);
        View X = b.make(8, H, W);          // [b, g, r standardised | depth / 255 | four pad zeros]
        if (!dry) c->X = X;
        tap("X", X);
        View x4 = Builder::slice(X, 0, cin);
        // stage 1
        View l0 = b.make(32, h2, w2), l1 = b.make(32, h2, w2);
        View A = b.make(40, h2, w2), An = b.make(40, h2, w2);          // [level1_2 (32) | inp1 (4) | pad]
        conv("level1_0", X, cin, l0, 3, 2, true);
        conv("level1_1", l0, 32, l1, 3, 1, true);
        conv("level1_2", l1, 32, Builder::slice(A, 0, 32), 3, 1, true);
        pool("inject_1", x4, Builder::slice(A, 32, cin));
        affine("b1", Builder::slice(A, 0, 32 + cin), Builder::slice(An, 0, 32 + cin), &An);
        // stage 2: [level2.1 (64) | level2_0 (64) | inp2 (4) | pad]
        View Bc = b.make(136, h4, w4), Bn = b.make(136, h4, w4);
        View o10 = Builder::slice(Bc, 64, 64);
        down("level2_0", An, 32 + cin, o10, 2, 8);
        View cur = o10;
        for (int i = 0; i < M - 1; ++i) {
            View out = i == M - 2 ? Builder::slice(Bc, 0, 64) : b.make(64, h4, w4);
            block("level2." + std::to_string(i), cur, out, 2, 8, fused);
            cur = out;
        }
        {
            View tmp = b.make(8, h2, w2);
            View t4 = Builder::slice(tmp, 0, cin);
            pool("inject_2.0", x4, t4, &tmp);
            pool("inject_2", t4, Builder::slice(Bc, 128, cin));
        }
        affine("bn_prelu_2", Builder::slice(Bc, 0, 128 + cin), Builder::slice(Bn, 0, 128 + cin), &Bn);
        // stage 3: [level3_0 (128) | level3.19 (128)]
        View Cc = b.make(256, h8, w8), Cn = b.make(256, h8, w8);
        View o20 = Builder::slice(Cc, 0, 128);
        down("level3_0", Bn, 128 + cin, o20, 4, 16);
        cur = o20;
        for (int i = 0; i < N - 1; ++i) {
            View out = i == N - 2 ? Builder::slice(Cc, 128, 128) : b.make(128, h8, w8);
            block("level3." + std::to_string(i), cur, out, 4, 16, fused);
            cur = out;
        }
        affine("bn_prelu_3", Cc, Cn, nullptr);
        View o8 = b.make(4, h8, w8);
        conv("classifier.0", Cn, 256, Builder::slice(o8, 0, ncls), 1, 1, false, &o8);
        if (!dry) c->q = (float*)b.dalloc_bytes(sizeof(float) * (size_t)b.Bmax * ncls * h8 * w8);
        float* q = c->q;
        quber_ctx* ctx = c;
        op("logits", [=](int B, hipStream_t st) {
            int rc = launch_cg_planes(o8, ncls, B, q, st);
            if (rc) return rc;
            return launch_upsample_logits(q, ctx->cur_out, B, ncls, h8, w8, 8, ctx->cfg.height, ctx->cfg.width, 0u, st);
        });
        if (!dry) c->ops.back().launches = 2;
        tap("A", A); tap("Bc", Bc); tap("Cc", Cc);
    }
};

}  // namespace

void build_cgnet(Builder& b) { CgBuilder(b).build(); }

}  // namespace quber
