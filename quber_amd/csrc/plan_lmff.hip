// ------------------------------------------------------------------------------------------------
// LMFFNet launch plan (reference foreground_segmentation/lmffnet.py:283-341; keys = that module's state_dict keys)
#include "plan.h"

namespace quber {
namespace {

struct BnP {   // folded BatchNorm(eps 1e-3) + PReLU vectors, padded with identity / zero slope
    std::vector<float> scale, shift, slope;
};

struct LmffBuilder {
    Builder& b;
    quber_ctx* c;
    bool dry;
    explicit LmffBuilder(Builder& bb) : b(bb), c(bb.c), dry(bb.dry) {}

    // a named intermediate (quber_debug_tensor): every buffer of the plan is an allocation of its own that stays valid after the
    // forward, so a tap is one map entry.  `buf`: the wide buffer a channel slice lives in, registered as <name>.buf (its pad channels)
    void tap(const std::string& n, const View& v, const View* buf = nullptr) {
        if (dry) return;
        c->taps[n] = v;
        if (buf) c->taps[n + ".buf"] = *buf;
    }
    // an op of lmff.hip / elementwise.hip, named after the tap it writes (quber_op_info)
    void op(const std::string& n, std::function<int(int, hipStream_t)> f) {
        b.op(std::move(f));
        if (!dry) c->ops.back().name = n;
    }
    // a plain fp32 array as a view: [Bmax][h][w][C]
    View array_view(float* p, int h, int w, int C) {
        View v;
        v.p = p; v.B = b.Bmax; v.H = h; v.W = w; v.C = C; v.cs = C; v.gs = (long)b.Bmax * h * w * C;
        return v;
    }

    BnP bnp(const std::string& n, int C, int Cpad = 0) {
        BnP r;
        const float* w = b.hw(n + ".bn.weight", C);
        const float* bi = b.hw(n + ".bn.bias", C);
        const float* m = b.hw(n + ".bn.running_mean", C);
        const float* v = b.hw(n + ".bn.running_var", C);
        const float* a = b.hw(n + ".acti.weight", C);
        if (Cpad < C) Cpad = C;
        r.scale.assign(Cpad, 1.f); r.shift.assign(Cpad, 0.f); r.slope.assign(Cpad, 0.f);
        if (dry || !w || !bi || !m || !v || !a) return r;
        for (int i = 0; i < C; ++i) {
            r.scale[i] = w[i] * (1.0f / sqrtf(v[i] + 1e-3f));
            r.shift[i] = bi[i] - m[i] * r.scale[i];
            r.slope[i] = a[i];
        }
        return r;
    }
    // dense conv (+ optional fused BN+PReLU): key prefix n -> n.conv.weight, n.bn_prelu.*
    void conv(const std::string& n, const View& in, int cin_real, const View& out, int k, int stride, bool fused, const View* buf = nullptr) {
        const int Cout = out.C;
        const float* w = b.hw(n + ".conv.weight", (int64_t)Cout * cin_real * k * k);
        BnP e;
        if (fused) e = bnp(n + ".bn_prelu", Cout);
        b.emit_conv(n, {w}, in, cin_real, out, k, stride, k == 3 ? 1 : 0, 1, fused, e.scale, e.shift, fused ? e.slope : std::vector<float>(), nullptr, false);
        tap(n, out, buf);
    }
    void dwconv(const std::string& n, const View& in, const View& out, int dil, const View* buf = nullptr) {
        const int C = in.C;
        const float* w = b.hw(n + ".conv.weight", (int64_t)C * 9);
        BnP e = bnp(n + ".bn_prelu", C);
        if (dry || !w) return;
        const float* dw = b.upload(std::vector<float>(w, w + (size_t)C * 9));
        const float *ds = b.upload(e.scale), *dh = b.upload(e.shift), *dl = b.upload(e.slope);
        op(n, [=](int B, hipStream_t st) { return launch_dwconv3x3(in, out, B, dil, dw, ds, dh, dl, st); });
        tap(n, out, buf);
    }
    void affine(const std::string& n, const View& a, const View* add, const View& out, const View* buf = nullptr) {
        BnP e = bnp(n, a.C);
        if (dry) return;
        const float *ds = b.upload(e.scale), *dh = b.upload(e.shift), *dl = b.upload(e.slope);
        const bool has = add != nullptr;
        const View addv = has ? *add : View();
        op(n, [=](int B, hipStream_t st) { return launch_affine_prelu(a, has ? &addv : nullptr, out, B, ds, dh, dl, st); });
        tap(n, out, buf);
    }
    void pool(const std::string& n, const View& in, const View& out, int mode, const View* buf = nullptr) {
        op(n, [=](int B, hipStream_t st) { return launch_pool_s2(in, out, B, mode, st); });
        tap(n, out, buf);
    }
    // SEM_B (lmffnet.py:80-113)
    View sem(const std::string& n, const View& x, int dil, const View& out) {
        const int C = x.C, h = x.H, w = x.W;
        View t = b.make(C / 2, h, w), u = b.make(C / 2, h, w), v = b.make(C / 2, h, w), r = b.make(C, h, w);
        conv(n + ".conv3x3", x, C, t, 3, 1, true);
        dwconv(n + ".dconv_left", Builder::slice(t, 0, C / 4), Builder::slice(u, 0, C / 4), 1);
        dwconv(n + ".dconv_right", Builder::slice(t, C / 4, C / 4), Builder::slice(u, C / 4, C / 4), dil);
        conv(n + ".conv3x3_resume.conv3x3", u, C / 2, v, 3, 1, true);
        conv(n + ".conv3x3_resume.conv1x1_resume", v, C / 2, r, 1, 1, false);
        affine(n + ".bn_relu_1", r, &x, out);
        return out;
    }
    // PMCA (lmffnet.py:172-191): channel attention of `x`, written scaled into `out`
    void pmca(const std::string& n, const View& x, const View& out) {
        const int C = x.C;
        const float* w2 = b.hw(n + ".conv2x2.conv.weight", (int64_t)C * 4);
        const float* f0 = b.hw(n + ".SE_Block.fc.0.weight", (int64_t)(C / 8) * C);
        const float* al = b.hw(n + ".SE_Block.fc.1.weight", 1);
        const float* f2 = b.hw(n + ".SE_Block.fc.2.weight", (int64_t)C * (C / 8));
        if (dry || !w2 || !f0 || !al || !f2) return;
        const float* dw2 = b.upload(std::vector<float>(w2, w2 + C * 4));
        const float* df0 = b.upload(std::vector<float>(f0, f0 + (C / 8) * C));
        const float* dal = b.upload(std::vector<float>(al, al + 1));
        const float* df2 = b.upload(std::vector<float>(f2, f2 + C * (C / 8)));
        float* wts = (float*)b.dalloc_bytes(sizeof(float) * (size_t)b.Bmax * C);
        double* sums = (double*)b.dalloc_bytes(sizeof(double) * (size_t)b.Bmax * C * 5);
        op(n, [=](int B, hipStream_t st) {
            int rc = launch_pmca(x, B, dw2, df0, dal, df2, wts, sums, st);
            if (rc) return rc;
            return launch_scale_channels(x, wts, out, B, st);
        });
        tap(n + ".weights", array_view(wts, 1, 1, C));
        tap(n, out);
    }

    void build() {
        const int H = b.H, W = b.W, h2 = H / 2, w2 = W / 2, h4 = H / 4, w4 = W / 4, h8 = H / 8, w8 = W / 8;
        const int ncls = 3;
        View X = b.make(8, H, W);
        if (!dry) c->X = X;
        tap("X", X);
        View x6 = Builder::slice(X, 0, 6);
        // Init block
        View i0 = b.make(32, h2, w2), i1 = b.make(32, h2, w2);
        View A = b.make(40, h2, w2);                       // [init(32) | down_1(6) | pad]
        conv("Init_Block.init_conv.0", X, 6, i0, 3, 2, true);
        conv("Init_Block.init_conv.1", i0, 32, i1, 3, 1, true);
        conv("Init_Block.init_conv.2", i1, 32, Builder::slice(A, 0, 32), 3, 1, true);
        View dn1 = Builder::slice(A, 32, 6);
        pool("inject_1", x6, dn1, 0);
        // FFM-A
        View An = b.make(40, h2, w2), ffa = b.make(40, h2, w2);
        affine("FFM_A.bn_prelu", Builder::slice(A, 0, 38), nullptr, Builder::slice(An, 0, 38), &An);
        conv("FFM_A.conv1x1", An, 38, Builder::slice(ffa, 0, 38), 1, 1, false, &ffa);
        // downsample 1: conv(38 -> 26) | maxpool(38) -> 64
        View D = b.make(64, h4, w4), d1 = b.make(64, h4, w4);
        conv("downsample_1.conv3x3", ffa, 38, Builder::slice(D, 0, 26), 3, 2, false);
        pool("downsample_1.maxpool", Builder::slice(ffa, 0, 38), Builder::slice(D, 26, 38), 1);
        affine("downsample_1.bn_prelu", D, nullptr, d1);
        // SEM-B block 1 -> FFM-B1 input [sem(64) | pmca(d1)(64) | down_2(6) | pad]
        View Bc = b.make(136, h4, w4);
        View cur = d1;
        static const int dil1[3] = {2, 2, 2};
        for (int i = 0; i < 3; ++i) {
            View out = i == 2 ? Builder::slice(Bc, 0, 64) : b.make(64, h4, w4);
            cur = sem("SEM_B_Block1.SEM_B_Block.SEM_Block_1" + std::to_string(i), cur, dil1[i], out);
        }
        pmca("FFM_B1.PMCA", d1, Builder::slice(Bc, 64, 64));
        View dn2 = Builder::slice(Bc, 128, 6);
        {
            View tmp = b.make(8, h2, w2);
            View t6 = Builder::slice(tmp, 0, 6);
            pool("inject_2.0", x6, t6, 0, &tmp);
            pool("inject_2", t6, dn2, 0);
        }
        View Bn = b.make(136, h4, w4), fb1 = b.make(136, h4, w4);
        affine("FFM_B1.bn_prelu", Builder::slice(Bc, 0, 134), nullptr, Builder::slice(Bn, 0, 134), &Bn);
        conv("FFM_B1.conv1x1", Bn, 134, Builder::slice(fb1, 0, 134), 1, 1, false, &fb1);
        // downsample 2 (134 -> 128, no concat) + BN/PReLU fused
        View d2 = b.make(128, h8, w8);
        {
            const float* w = b.hw("downsample_2.conv3x3.conv.weight", (int64_t)128 * 134 * 9);
            BnP e = bnp("downsample_2.bn_prelu", 128);
            b.emit_conv("downsample_2.conv3x3", {w}, fb1, 134, d2, 3, 2, 1, 1, true, e.scale, e.shift, e.slope, nullptr, false);
            tap("downsample_2.conv3x3", d2);
        }
        View Cc = b.make(264, h8, w8);
        cur = d2;
        static const int dil2[8] = {4, 4, 8, 8, 16, 16, 32, 32};
        for (int i = 0; i < 8; ++i) {
            View out = i == 7 ? Builder::slice(Cc, 0, 128) : b.make(128, h8, w8);
            cur = sem("SEM_B_Block2.SEM_B_Block.SEM_Block_2" + std::to_string(i), cur, dil2[i], out);
        }
        pmca("FFM_B2.PMCA", d2, Builder::slice(Cc, 128, 128));
        {
            View t1 = b.make(8, h2, w2), t2 = b.make(8, h4, w4);
            View a6 = Builder::slice(t1, 0, 6), b6 = Builder::slice(t2, 0, 6);
            pool("inject_3.0", x6, a6, 0, &t1);
            pool("inject_3.1", a6, b6, 0, &t2);
            pool("inject_3", b6, Builder::slice(Cc, 256, 6), 0);
        }
        View Cn = b.make(264, h8, w8), fb2 = b.make(264, h8, w8);
        affine("FFM_B2.bn_prelu", Builder::slice(Cc, 0, 262), nullptr, Builder::slice(Cn, 0, 262), &Cn);
        conv("FFM_B2.conv1x1", Cn, 262, Builder::slice(fb2, 0, 262), 1, 1, false, &fb2);
        // MAD (lmffnet.py:232-280)
        View cat48 = b.make(48, h4, w4), dl = b.make(32, h8, w8), dwa = b.make(48, h4, w4), att = b.make(4, h4, w4);
        conv("MAD.mid_layer_1x1", fb1, 134, Builder::slice(cat48, 0, 16), 1, 1, false);
        conv("MAD.deep_layer_1x1", fb2, 262, dl, 1, 1, false);
        {
            View dst = Builder::slice(cat48, 16, 32);
            op("MAD.up_deep", [=](int B, hipStream_t st) { return launch_bilinear(dl, dst, B, st); });
            tap("MAD.up_deep", dst);
        }
        dwconv("MAD.DwConv1", cat48, dwa, 1);
        conv("MAD.PwConv1", dwa, 48, Builder::slice(att, 0, ncls), 1, 1, false, &att);
        View dwb = b.make(264, h8, w8), o8 = b.make(4, h8, w8), o4 = b.make(4, h4, w4);
        dwconv("MAD.DwConv2", Builder::slice(fb2, 0, 262), Builder::slice(dwb, 0, 262), 1, &dwb);
        conv("MAD.PwConv2", dwb, 262, Builder::slice(o8, 0, ncls), 1, 1, false, &o8);
        op("MAD.up_out", [=](int B, hipStream_t st) { return launch_bilinear(o8, o4, B, st); });
        tap("MAD.up_out", Builder::slice(o4, 0, ncls), &o4);
        if (!dry) c->q = (float*)b.dalloc_bytes(sizeof(float) * (size_t)b.Bmax * ncls * h4 * w4);
        float* q = c->q;
        quber_ctx* ctx = c;
        op("MAD.gate", [=](int B, hipStream_t st) {
            int rc = launch_mad_gate(o4, att, q, B, ncls, st);
            if (rc) return rc;
            return launch_upsample_logits(q, ctx->cur_out, B, ncls, h4, w4, 4, ctx->cfg.height, ctx->cfg.width, 0u, st);
        });
        tap("MAD.gate", array_view(q, ncls * h4, w4, 1));
        // the concatenation buffers, whole (every other wide buffer with pad channels is the .buf tap of the op that writes into it)
        tap("A", A); tap("Bc", Bc); tap("Cc", Cc);
        if (!dry) {
            c->taps["ffm_a"] = Builder::slice(ffa, 0, 38);
            c->taps["d1"] = d1;
            c->taps["ffm_b1"] = Builder::slice(fb1, 0, 134);
            c->taps["ffm_b2"] = Builder::slice(fb2, 0, 262);
        }
    }
};

}  // namespace

void build_lmff(Builder& b) { LmffBuilder(b).build(); }

}  // namespace quber
