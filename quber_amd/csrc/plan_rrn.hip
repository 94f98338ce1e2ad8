// ------------------------------------------------------------------------------------------------
// Launch plan of the Region Refinement Network of UOIS-Net-3D (reference uois/src/segmentation.py:248-266 RegionRefinementNetwork over
// uois/src/networks.py:191-278 UNet_Encoder(4, fd) / UNet_Decoder(1, fd) and a bias-free 1x1 fg_module; keys = that module's state_dict
// keys).  A plain U-Net: the Depth Seeding Network without its ESP modules, built from the same helpers (plan_unet.h).  feature_dim is read
// off the first convolution's weight; the input is NHWC-8 [c0, c1, c2, mask | four zeros] of S x S crops, S a multiple of 16.
// Option key 54 (rrn_head): nothing non-linear lies between decoder.last_conv and fg_module, so 1 = they are one 3x3 fd -> 1 filter,
// w'[c][ky][kx] = sum_o wfg[o] W[o][c][ky][kx], b' = sum_o wfg[o] bias[o] (float64 on the host, rounded once), run by rrn_head3 (rrn.hip)
// on decoder.layer5's output; 0 = the convolution with its bias, then the 1x1 head kernel.
#include "plan_unet.h"

namespace quber {
namespace {

struct RrnBuilder : UNetBuilder {
    explicit RrnBuilder(Builder& bb) : UNetBuilder(bb) {}

    // Conv2d_GN_ReLUx2 (networks.py:35-56): n.layer1, n.layer2
    void conv_gn2(const std::string& n, const View& in, const View& out, const View* buf) {
        View mid = b.make(out.C, out.H, out.W);
        conv_gn(n + ".layer1", in, mid);
        conv_gn(n + ".layer2", mid, out, 3, buf);
    }

    void build() {
        const int H = b.H, W = b.W;
        if (!dry) {
            auto it = c->hostw.find("encoder.layer1.layer1.conv1.weight");
            if (it == c->hostw.end() || it->second.size() % 36) { b.err = "missing or misshapen weight 'encoder.layer1.layer1.conv1.weight'"; return; }
            fd = (int)(it->second.size() / 36);
            if (fd < 8 || fd > 64 || fd % 4) { b.err = "RRN: feature_dim must be a multiple of 4 in 8..64"; return; }
        }
        const bool collapsed = tune().rrn_head != 0;
        const int f = fd;
        const int h2 = H / 2, w2 = W / 2, h4 = H / 4, w4 = W / 4, h8 = H / 8, w8 = W / 8, h16 = H / 16, w16 = W / 16;
        if (!dry) alloc_stats(19);
        View X = b.make(8, H, W);            // [c0, c1, c2, mask | four pad zeros]
        if (!dry) c->X = X;
        quber_ctx* ctx = c;
        op("pack", OP_OTHER, 2, [=](int B, hipStream_t st) {
            int rc = launch_zero(ctx->dsn_stats, ctx->dsn_stats_bytes, st);
            if (rc) return rc;
            return launch_rrn_pack(ctx->rrn_rgb, ctx->rrn_mask, B, ctx->cfg.height, ctx->cfg.width, ctx->X.p, st);
        });
        tap("X", X);
        // the four concatenation buffers of the decoder: [upsampled (C/2) | encoder output (C/2)]
        View cat4 = b.make(2 * f, H, W), cat3 = b.make(4 * f, h2, w2), cat2 = b.make(8 * f, h4, w4), cat1 = b.make(16 * f, h8, w8);
        const View x1 = Builder::slice(cat4, f, f), x2 = Builder::slice(cat3, 2 * f, 2 * f), x3 = Builder::slice(cat2, 4 * f, 4 * f), x4 = Builder::slice(cat1, 8 * f, 8 * f);
        // ---- encoder ----
        View a1 = b.make(f, H, W);
        {
            View tmp = b.make(f, H, W);
            const std::string n = "encoder.layer1.layer1";
            conv(n + ".conv1", X, 4, tmp, 3, 1, false);
            gn(n + ".gn1", tmp, a1, nullptr);
        }
        conv_gn("encoder.layer1.layer2", a1, x1, 3, &cat4);
        View p1 = b.make(f, h2, w2), p2 = b.make(2 * f, h4, w4), p3 = b.make(4 * f, h8, w8), p4 = b.make(8 * f, h16, w16), x5 = b.make(16 * f, h16, w16);
        pool("pool1", x1, p1);
        conv_gn2("encoder.layer2", p1, x2, &cat3);
        pool("pool2", x2, p2);
        conv_gn2("encoder.layer3", p2, x3, &cat2);
        pool("pool3", x3, p3);
        conv_gn2("encoder.layer4", p3, x4, &cat1);
        pool("pool4", x4, p4);
        conv_gn("encoder.last_layer", p4, x5);
        // ---- decoder ----
        View fu = b.make(16 * f, h16, w16);
        conv_gn("decoder.fuse_layer", x5, fu, 1);
        View o1 = b.make(8 * f, h8, w8), o2 = b.make(4 * f, h4, w4), o3 = b.make(2 * f, h2, w2), o4 = b.make(f, H, W), o5 = b.make(f, H, W);
        up("decoder.layer1", fu, cat1, o1);
        up("decoder.layer2", o1, cat2, o2);
        up("decoder.layer3", o2, cat3, o3);
        up("decoder.layer4", o3, cat4, o4);
        conv_gn("decoder.layer5", o4, o5);
        // ---- head ----
        if (!collapsed) {
            View feat = b.make(f, H, W);
            conv("decoder.last_conv", o5, f, feat, 3, 1, true);
            const float* wf = b.hw("fg_module.weight", f);
            if (dry || !wf) return;
            const float* dwf = b.upload(std::vector<float>(wf, wf + f));
            c->flops += 2.0 * H * W * f;
            op("head", OP_OTHER, 1, [=](int B, hipStream_t st) { return launch_rrn_head(feat, B, dwf, ctx->rrn_thr, ctx->rrn_logits, ctx->rrn_refined, st); });
        } else {
            const float* wl = b.hw("decoder.last_conv.weight", (int64_t)f * f * 9);
            const float* bl = b.hw("decoder.last_conv.bias", f);
            const float* wf = b.hw("fg_module.weight", f);
            if (dry || !wl || !bl || !wf) return;
            std::vector<float> w9((size_t)9 * f);              // [tap][c]
            for (int ci = 0; ci < f; ++ci)
                for (int tp = 0; tp < 9; ++tp) {
                    double s = 0.0;
                    for (int o = 0; o < f; ++o) s += (double)wf[o] * (double)wl[((size_t)o * f + ci) * 9 + tp];
                    w9[(size_t)tp * f + ci] = (float)s;
                }
            double sb = 0.0;
            for (int o = 0; o < f; ++o) sb += (double)wf[o] * (double)bl[o];
            const float bias = (float)sb;
            const float* dw9 = b.upload(w9);
            c->flops += 2.0 * H * W * 9.0 * f;
            op("head3", OP_OTHER, 1, [=](int B, hipStream_t st) { return launch_rrn_head3(o5, B, dw9, bias, ctx->rrn_thr, ctx->rrn_logits, ctx->rrn_refined, st); });
        }
        tap("cat1", cat1); tap("cat2", cat2); tap("cat3", cat3); tap("cat4", cat4);
        check_stats();
    }
};

}  // namespace

void build_rrn(Builder& b) { RrnBuilder(b).build(); }

}  // namespace quber
