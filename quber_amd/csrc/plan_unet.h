// What the launch plans of the two U-Nets of UOIS-Net-3D share (plan_dsn.hip: the Depth Seeding Network, plan_rrn.hip: the Region Refinement
// Network; reference uois/src/networks.py:12-56, 131-184): named taps and ops, the convolution and GroupNorm + ReLU of a Conv2d_GN_ReLU, the 2x2
// max pool, the upsample-concatenate-convolve block of the decoder.  GroupNorm has feature_dim groups everywhere; a concatenation is never
// copied: the encoder's outputs are normalised into the upper channel slice of the buffer whose lower slice the decoder's upsampling fills.
#pragma once
#include "plan.h"

namespace quber {

struct UNetBuilder {
    Builder& b;
    quber_ctx* c;
    bool dry;
    int fd = 64;
    std::vector<double*> stats;       // one [Bmax][fd][2] block of c->dsn_stats per GroupNorm, in plan order
    size_t n_stats = 0;
    explicit UNetBuilder(Builder& bb) : b(bb), c(bb.c), dry(bb.dry) {}

    void tap(const std::string& n, const View& v, const View* buf = nullptr) {
        if (dry) return;
        c->taps[n] = v;
        if (buf) c->taps[n + ".buf"] = *buf;
    }
    void op(const std::string& n, int kind, int launches, std::function<int(int, hipStream_t)> f) {
        if (dry) return;
        b.op(std::move(f));
        c->ops.back().name = n;
        c->ops.back().kind = kind;
        c->ops.back().launches = launches;
    }
    // the statistics blocks of `norms` GroupNorm layers: c->dsn_stats, cleared by the plan's first op
    void alloc_stats(int norms) {
        const size_t block = (size_t)2 * fd * b.Bmax;
        c->dsn_stats_bytes = sizeof(double) * block * norms;
        c->dsn_stats = (double*)b.dalloc_bytes(c->dsn_stats_bytes);
        for (int i = 0; i < norms; ++i) stats.push_back(c->dsn_stats ? c->dsn_stats + block * i : nullptr);
    }
    double* next_stats() {
        if (dry) return nullptr;
        if (n_stats >= stats.size()) { if (b.err.empty()) b.err = "internal: more GroupNorm layers than statistics blocks"; return nullptr; }
        return stats[n_stats++];
    }
    void check_stats() {
        if (!dry && n_stats != stats.size() && b.err.empty()) b.err = "internal: the plan has another number of GroupNorm layers than statistics blocks";
    }

    // n.weight [+ n.bias], no activation
    void conv(const std::string& n, const View& in, int cin_real, const View& out, int k, int dil, bool bias, const View* buf = nullptr) {
        const float* w = b.hw(n + ".weight", (int64_t)out.C * cin_real * k * k);
        const float* bi = bias ? b.hw(n + ".bias", out.C) : nullptr;
        std::vector<float> scale, shift;
        if (bias && bi) { scale.assign(out.C, 1.f); shift.assign(bi, bi + out.C); }
        b.emit_conv(n, {w}, in, cin_real, out, k, 1, k == 3 ? dil : 0, dil, bias, scale, shift, {}, nullptr, false);
        tap(n, out, buf);
    }
    // GroupNorm(fd groups, eps 1e-5) + ReLU under n.{weight, bias}; sums: null = a statistics pass over `in`, else tile sums that an ESP kernel left
    void gn(const std::string& n, const View& in, const View& out, const View* buf, const double* sums = nullptr, int tiles = 0) {
        const int C = in.C, G = fd;
        const float* g = b.hw(n + ".weight", C);
        const float* be = b.hw(n + ".bias", C);
        if (dry || !g || !be) return;
        const float* dg = b.upload(std::vector<float>(g, g + C));
        const float* db = b.upload(std::vector<float>(be, be + C));
        double* st8 = next_stats();
        if (!st8) return;
        op(n, OP_NORM, 2, [=](int B, hipStream_t st) {
            int rc = sums ? launch_esp_stats(sums, B, tiles, G, st8, st) : launch_gn_stats(in, B, 1, G, st8, st, false);
            if (rc) return rc;
            return launch_gn_apply(in, out, B, 1, G, st8, dg, db, C, 1e-5f, 1, st);
        });
        tap(n, out, buf);
    }
    // Conv2d_GN_ReLU (networks.py:12-33): n.conv1, n.gn1
    void conv_gn(const std::string& n, const View& in, const View& out, int k = 3, const View* buf = nullptr) {
        View tmp = b.make(out.C, out.H, out.W);
        conv(n + ".conv1", in, in.C, tmp, k, 1, false);
        gn(n + ".gn1", tmp, out, buf);
    }
    void pool(const std::string& n, const View& in, const View& out) {
        op(n, OP_OTHER, 1, [=](int B, hipStream_t st) { return launch_pool_s2(in, out, B, 1, st); });
        tap(n, out);
    }
    // Upsample_Concat_Conv2d_GN_ReLU (networks.py:131-154; one encoder: the _Multi_Branch form of :156-184 is the same module): x1 [C] at half
    // the size of cat [C/2 from x1 | C/2 from the encoder] -> out
    void up(const std::string& n, const View& x1, const View& cat, const View& out) {
        const int C = x1.C;
        View red = b.make(C / 2, x1.H, x1.W);
        conv_gn(n + ".channel_reduction_layer", x1, red);
        const View lo = Builder::slice(cat, 0, C / 2);
        op(n + ".upsample", OP_OTHER, 1, [=](int B, hipStream_t st) { return launch_bilinear(red, lo, B, st); });
        tap(n + ".upsample", lo, &cat);
        conv_gn(n + ".conv_gn_relu", cat, out);
    }
};

}  // namespace quber
