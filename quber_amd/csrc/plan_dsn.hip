// ------------------------------------------------------------------------------------------------
// Launch plan of the Depth Seeding Network of UOIS-Net-3D (reference uois/src/networks.py: UNetESP_Encoder, UNetESP_Decoder;
// uois/src/segmentation.py:72-127 DepthSeedingNetwork; keys = that module's state_dict keys).  feature_dim is read off the first
// convolution's weight; GroupNorm has feature_dim groups everywhere.  Option key 53 (dsn_fused): 1 = the five dilated convolutions of
// an ESP module, their running sums, the residual and the GroupNorm sums are one kernel (esp_branches, dsn.hip), 0 = five convolution
// launches + esp_merge, the bring-up path and the second arm of the A/B.
// A concatenation is never copied: the encoder's x1..x4 are normalised into the upper channel slice of the buffer whose lower slice
// the decoder's upsampling fills.
#include "plan_unet.h"

namespace quber {
namespace {

struct DsnBuilder : UNetBuilder {
    double* partials = nullptr;       // tile sums of the ESP modules (the stream orders them): [Bmax][tiles of the 1/4 map][fd][2]
    explicit DsnBuilder(Builder& bb) : UNetBuilder(bb) {}

    // ESPModule (networks.py:58-129), add = True: x [C] -> out [C] (possibly a slice of `buf`)
    void esp(const std::string& n, const View& x, const View& out, int k, bool fused, const View* buf = nullptr) {
        const int C = x.C, h = x.H, w = x.W;
        const int nn = C / 5, n1 = C - 4 * nn;
        const int n4 = (nn + 3) / 4 * 4, n16 = esp_nt(n1) * 16;
        View tb = b.make(n16, h, w);                            // t: nn channels on a stride of 16 ceil(n1 / 16); the rest stays zero
        View t = Builder::slice(tb, 0, nn), t4 = Builder::slice(tb, 0, n4);
        conv(n + ".conv1", x, C, t, k, 1, false, &tb);
        View sum = b.make(C, h, w);
        const int tiles = esp_tiles(h, w);
        double* pp = partials;
        const int G = fd;
        static const char* names[5] = {".dilated1", ".dilated2", ".dilated4", ".dilated8", ".dilated16"};
        if (fused) {
            // a split launch_esp_branches has no kernel for is refused here, at finalize, not at the first forward
            if (!dry && !esp_kernel(n1) && b.err.empty()) b.err = "DSN: esp_branches has no kernel for the " + std::to_string(n1) + " + 4 * " + std::to_string(nn) + " channels of " + n;
            const float* hwp[5];
            bool ok = !dry;
            for (int i = 0; i < 5; ++i) {
                hwp[i] = b.hw(n + names[i] + ".weight", (int64_t)(i == 0 ? n1 : nn) * nn * 9);
                ok = ok && hwp[i];
            }
            float* packed = ok ? (float*)b.dalloc_bytes(sizeof(float) * esp_packed_floats(n1)) : nullptr;
            if (packed) {                                       // (a missing weight or a failed allocation was already reported)
                const float* dw[5];
                for (int i = 0; i < 5; ++i) dw[i] = b.upload(std::vector<float>(hwp[i], hwp[i] + (size_t)(i == 0 ? n1 : nn) * nn * 9));
                if (launch_esp_pack(dw, nn, n1, packed, nullptr) && b.err.empty()) b.err = "esp_pack failed at " + n;      // the null stream: finalize synchronises
                const double fl = 2.0 * h * w * 9.0 * nn * (n1 + 4.0 * nn);
                c->flops += fl;
                op(n + ".branches", OP_CONV, 1, [=](int B, hipStream_t st) { return launch_esp_branches(tb, &x, sum, B, nn, n1, G, packed, pp, tiles, st); });
                c->ops.back().flops = fl;
                tap(n + ".sum", sum);
            }
        } else {
            View d[5];
            for (int i = 0; i < 5; ++i) {
                const int co = i == 0 ? n1 : nn;
                View db = b.make((co + 3) / 4 * 4, h, w);
                d[i] = Builder::slice(db, 0, co);
                conv(n + names[i], t4, nn, d[i], 3, 1 << i, false, &db);
            }
            const View d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3], d4 = d[4];
            op(n + ".merge", OP_OTHER, 1, [=](int B, hipStream_t st) {
                const View dd[5] = {d0, d1, d2, d3, d4};
                return launch_esp_merge(dd, &x, sum, B, nn, n1, G, pp, tiles, st);
            });
            tap(n + ".sum", sum);
        }
        gn(n + ".gn", sum, out, buf, pp, tiles);
    }
    void build() {
        const int H = b.H, W = b.W;
        if (!dry) {
            auto it = c->hostw.find("encoder.layer1.layer1.conv1.weight");
            if (it == c->hostw.end() || it->second.size() % 27) { b.err = "missing or misshapen weight 'encoder.layer1.layer1.conv1.weight'"; return; }
            fd = (int)(it->second.size() / 27);
            if (fd < 8 || fd > 64 || fd % 4) { b.err = "DSN: feature_dim must be a multiple of 4 in 8..64"; return; }
        }
        const bool fused = tune().dsn_fused != 0;
        const int f = fd;
        const int h2 = H / 2, w2 = W / 2, h4 = H / 4, w4 = W / 4, h8 = H / 8, w8 = W / 8, h16 = H / 16, w16 = W / 16;
        if (!dry) {
            alloc_stats(19);
            partials = (double*)b.dalloc_bytes(sizeof(double) * (size_t)b.Bmax * esp_tiles(h4, w4) * f * 2);
            c->dsn_clean = (float*)b.dalloc_bytes(sizeof(float) * (size_t)b.Bmax * 3 * H * W);
        }
        View X = b.make(8, H, W);            // [x, y, z | five pad zeros]
        if (!dry) c->X = X;
        quber_ctx* ctx = c;
        op("pack", OP_OTHER, 2, [=](int B, hipStream_t st) {
            int rc = launch_zero(ctx->dsn_stats, ctx->dsn_stats_bytes, st);
            if (rc) return rc;
            if (ctx->dsn_z)             // the point cloud exists only as the packed input and the cleaned planes
                return launch_xyz_from_depth(ctx->dsn_z, B, ctx->cfg.height, ctx->cfg.width, ctx->dsn_cam, ctx->dsn_convention, ctx->dsn_flags, nullptr, ctx->X.p, ctx->dsn_clean, st);
            return launch_dsn_pack(ctx->dsn_xyz, B, ctx->cfg.height, ctx->cfg.width, ctx->dsn_flags, ctx->X.p, ctx->dsn_clean, st);
        });
        tap("X", X);
        {
            View cl;
            cl.p = c->dsn_clean; cl.B = b.Bmax; cl.H = 3 * H; cl.W = W; cl.C = 1; cl.cs = 1; cl.gs = (long)b.Bmax * 3 * H * W;
            tap("xyz", cl);
        }
        // the four concatenation buffers of the decoder: [upsampled (C/2) | encoder output (C/2)]
        View cat4 = b.make(2 * f, H, W), cat3 = b.make(4 * f, h2, w2), cat2 = b.make(8 * f, h4, w4), cat1 = b.make(16 * f, h8, w8);
        const View x1 = Builder::slice(cat4, f, f), x2 = Builder::slice(cat3, 2 * f, 2 * f), x3 = Builder::slice(cat2, 4 * f, 4 * f), x4 = Builder::slice(cat1, 8 * f, 8 * f);
        // ---- encoder ----
        View a1 = b.make(f, H, W);
        {
            View tmp = b.make(f, H, W);
            const std::string n = "encoder.layer1.layer1";
            const float* w = b.hw(n + ".conv1.weight", (int64_t)f * 27);
            b.emit_conv(n + ".conv1", {w}, X, 3, tmp, 3, 1, 1, 1, false, {}, {}, {}, nullptr, false);
            tap(n + ".conv1", tmp);
            gn(n + ".gn1", tmp, a1, nullptr);
        }
        conv_gn("encoder.layer1.layer2", a1, x1, 3, &cat4);
        View p1 = b.make(f, h2, w2), a2 = b.make(2 * f, h2, w2);
        pool("pool1", x1, p1);
        conv_gn("encoder.layer2.layer1", p1, a2);
        conv_gn("encoder.layer2.layer2", a2, x2, 3, &cat3);
        View p2 = b.make(2 * f, h4, w4), a3 = b.make(4 * f, h4, w4);
        pool("pool2", x2, p2);
        conv_gn("encoder.layer3a", p2, a3);
        esp("encoder.layer3b", a3, x3, 3, fused, &cat2);
        View p3 = b.make(4 * f, h8, w8), a4 = b.make(8 * f, h8, w8);
        pool("pool3", x3, p3);
        conv_gn("encoder.layer4a", p3, a4);
        esp("encoder.layer4b", a4, x4, 3, fused, &cat1);
        View p4 = b.make(8 * f, h16, w16), x5 = b.make(16 * f, h16, w16);
        pool("pool4", x4, p4);
        conv_gn("encoder.last_layer", p4, x5);
        // ---- decoder ----
        View fu = b.make(16 * f, h16, w16);
        esp("decoder.fuse_layer", x5, fu, 1, fused);
        View o1 = b.make(8 * f, h8, w8), o2 = b.make(4 * f, h4, w4), o3 = b.make(2 * f, h2, w2), o4 = b.make(f, H, W), o5 = b.make(f, H, W), feat = b.make(f, H, W);
        up("decoder.layer1", fu, cat1, o1);
        up("decoder.layer2", o1, cat2, o2);
        up("decoder.layer3", o2, cat3, o3);
        up("decoder.layer4", o3, cat4, o4);
        conv_gn("decoder.layer5", o4, o5);
        conv("decoder.last_conv", o5, f, feat, 3, 1, true);
        // ---- heads ----
        const float* wf = b.hw("fg_module.weight", (int64_t)3 * f);
        const float* wc = b.hw("cd_module.weight", (int64_t)3 * f);
        if (dry || !wf || !wc) return;
        const float* dwf = b.upload(std::vector<float>(wf, wf + 3 * f));
        const float* dwc = b.upload(std::vector<float>(wc, wc + 3 * f));
        c->flops += 2.0 * H * W * 6.0 * f;
        op("head", OP_OTHER, 1, [=](int B, hipStream_t st) {
            return launch_dsn_head(feat, B, ctx->dsn_clean, dwf, dwc, ctx->dsn_logits, ctx->dsn_offsets, ctx->dsn_votes, ctx->dsn_classes, ctx->dsn_fg, st);
        });
        tap("cat1", cat1); tap("cat2", cat2); tap("cat3", cat3); tap("cat4", cat4);
        check_stats();
    }
};

}  // namespace

void build_dsn(Builder& b) { DsnBuilder(b).build(); }

}  // namespace quber
