// Stand-alone ops of the C ABI (tests / micro-benchmarks): single launches without a context, on the process defaults of the options.
#include "plan.h"

using namespace quber;

static float* g_op_ws = nullptr;
static int g_op_skip_rows = 0;
static int g_op_bf16 = 0;
static const size_t g_op_ws_floats = (size_t)256 << 20;   // 1 GiB, test harness only
static int g_op_wino_reuse = 0;   // key 26

bool quber::op_set_tuning(int key, int value) {
    if (key == 2) {   // stand-alone conv op: allocate (value != 0) or drop the split-K workspace
        if (value && !g_op_ws) {
            if (hipMalloc((void**)&g_op_ws, sizeof(float) * g_op_ws_floats) != hipSuccess) g_op_ws = nullptr;
        } else if (!value && g_op_ws) {
            (void)hipFree(g_op_ws);
            g_op_ws = nullptr;
        }
        return true;
    }
    if (key == 26) { g_op_wino_reuse = value; return true; }   // timing harness: quber_op_conv3x3_winograd reuses the transformed filters its previous call left in u / ws
    if (key == 12) { g_op_bf16 = value; return true; }         // stand-alone conv ops: 1 = bf16, 2 = fp16 operands, 3 = fp32 as 3 bf16 terms; fp32 accumulation
    if (key == 11) { g_op_skip_rows = value; return true; }    // stand-alone conv op: tap-major K order with padded filter rows skipped (dilated 3x3)
    return false;
}

// the geometry fields of a dense single-group launch on unsliced tensors (K = k * k * cin; the callers pad it)
static void conv_geometry(ConvP& p, int B, int h, int w, int cin, int cout, int k, int stride, int pad, int dil) {
    p.B = B; p.H = h; p.W = w; p.Cin = cin; p.in_cs = cin;
    p.OH = (h + 2 * pad - dil * (k - 1) - 1) / stride + 1;
    p.OW = (w + 2 * pad - dil * (k - 1) - 1) / stride + 1;
    p.Cout = cout; p.out_cs = cout; p.K = k * k * cin;
    p.kh = k; p.kw = k; p.stride = stride; p.pad = pad; p.dil = dil;
    p.M = B * p.OH * p.OW; p.ohw = p.OH * p.OW;
}

// bf16x3 mode: the pre-split weight planes conv_x8.hip reads - a grow-only scratch of the process (test harness), one per op
struct PlaneScratch {
    void* planes = nullptr;
    size_t cap = 0;
    int split(const float* w, long n, ConvP& p, const char* who, hipStream_t st) {
        const size_t need = (size_t)n * 3 * sizeof(unsigned short);
        if (need > cap) {
            if (planes) (void)hipFree(planes);
            planes = nullptr; cap = 0;
            if (hipMalloc(&planes, need) != hipSuccess) return fail(std::string(who) + ": cannot allocate the bf16x3 weight planes");
            cap = need;
        }
        const int rc = launch_split_bf16x3(w, n, planes, st);
        if (rc) return rc;
        p.w3 = planes; p.w3_plane = n;
        return 0;
    }
};

static View mkview(const float* p, int B, int h, int w, int c) {
    View v;
    v.p = const_cast<float*>(p); v.B = B; v.H = h; v.W = w; v.C = c; v.cs = c; v.gs = 0;
    return v;
}

// the single-kernel form where it applies and the workspace also holds its filter order (36 * cout * cin floats per group) in front of the
// launch's own workspace: q.uf / q.ws / q.ws_floats set accordingly (q.ws, q.ws_floats: the whole workspace on entry)
static bool op_wino_single(WinoP& q, int B, int G) {
    const size_t order = (size_t)G * 36 * q.out.C * q.in.C;
    if (q.m != 4 || !tune().wino_fused || q.out.C % 32 || q.ws_floats < order) return false;
    q.uf = q.ws;
    if (!winograd_fused_ok(q, B, G)) { q.uf = nullptr; return false; }
    q.ws += order; q.ws_floats -= order;
    return true;
}

extern "C" {

__global__ void pack_oihw_kernel(const float* __restrict__ w, int O, int I, int k, int Kpad, int kmode, float* __restrict__ out) {
    const long total = (long)O * Kpad;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int o = i / Kpad, kk = i % Kpad;
        float v = 0.f;
        if (kk < k * k * I) {
            int tap, ci;
            if (kmode) {
                const int cb = kk / (k * k * 32), rem = kk % (k * k * 32);
                tap = rem / 32;
                ci = cb * 32 + rem % 32;
            } else {
                tap = kk / I;
                ci = kk % I;
            }
            v = w[((long)o * I + ci) * k * k + tap];
        }
        out[i] = v;
    }
}

int quber_op_conv2d(const float* x, int32_t B, int32_t h, int32_t w, int32_t cin, const float* w_oihw, int32_t cout, int32_t k, int32_t stride, int32_t pad, int32_t dil,
                    const float* scale, const float* shift, const float* residual, int32_t relu, float* packed, float* y, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int Kpad = (k * k * cin + 31) / 32 * 32;
    const bool skip_rows = g_op_skip_rows && k == 3 && stride == 1 && dil > 1 && cin % 32 == 0;
    const int kmode = (k > 1 && cin % 32 == 0 && !skip_rows) ? 1 : 0;
    hipLaunchKernelGGL(pack_oihw_kernel, dim3(256), dim3(256), 0, st, w_oihw, cout, cin, k, Kpad, kmode, packed);
    ConvP p{};
    p.in = x; p.w = packed; p.scale = scale; p.shift = shift; p.res = residual; p.out = y;
    conv_geometry(p, B, h, w, cin, cout, k, stride, pad, dil);
    p.res_cs = cout; p.Kpad = Kpad; p.relu = relu;
    p.kmode = kmode; p.skip_rows = skip_rows;
    p.bf16 = g_op_bf16; p.w_gs = 0; p.ss_gs = 0;
    // the stand-alone op splits K only when the test harness asked for a workspace (tuning key 2)
    p.ws = g_op_ws; p.ws_floats = g_op_ws ? g_op_ws_floats : 0;
    if (g_op_bf16 == 3 && k == 1 && tune().x8) {
        static PlaneScratch scratch;
        const int rc = scratch.split(packed, (long)cout * Kpad, p, "conv2d", st);
        if (rc) return rc;
    }
    return launch_conv(p, 1, st);
}

// the fp16 data path's 1x1 convolution on fp16 tensors (x, w [cout][cin], residual, y: fp16 in HBM; scale / shift fp32)
int quber_op_conv1x1_f16(const void* x, int32_t B, int32_t h, int32_t w, int32_t cin, const void* w_oi, int32_t cout,
                         const float* scale, const float* shift, const void* residual, int32_t relu, void* y, void* stream) {
    if (cin % 64) return fail("conv1x1_f16: cin must be a multiple of 64");
    ConvP p{};
    p.in = (const float*)x; p.w = (const float*)w_oi; p.scale = scale; p.shift = shift; p.res = (const float*)residual; p.out = (float*)y;
    conv_geometry(p, B, h, w, cin, cout, 1, 1, 0, 1);
    p.res_cs = cout; p.Kpad = cin; p.relu = relu;
    p.bf16 = 2; p.es = 2;
    return launch_conv(p, 1, (hipStream_t)stream);
}

int quber_op_conv2d_f16(const void* x, int32_t B, int32_t h, int32_t w, int32_t cin, const void* w_packed, int32_t cout, int32_t ksize, int32_t stride, int32_t pad, int32_t dil,
                        int32_t kmode, const float* scale, const float* shift, const void* residual, int32_t relu, double* gn_sums, int32_t gn_groups, void* y, void* stream) {
    if (cin % 8 || (kmode && cin % 64)) return fail("conv2d_f16: cin must be a multiple of 8 (slice-major K order: of 64)");
    if (ksize < 1 || stride < 1 || dil < 1 || pad < 0) return fail("conv2d_f16: bad geometry");
    ConvP p{};
    p.in = (const float*)x; p.w = (const float*)w_packed; p.scale = scale; p.shift = shift; p.res = (const float*)residual; p.out = (float*)y;
    conv_geometry(p, B, h, w, cin, cout, ksize, stride, pad, dil);
    if (p.OH < 1 || p.OW < 1) return fail("conv2d_f16: empty output");
    p.res_cs = cout; p.Kpad = (p.K + 63) / 64 * 64; p.relu = relu;      // (filter rows zero-filled up to Kpad)
    p.kmode = kmode; p.bf16 = 2; p.es = 2;
    p.w_gs = (long)cout * p.Kpad; p.ss_gs = cout;
    if (gn_sums) {
        if (gn_groups < 1 || cout % gn_groups) return fail("conv2d_f16: channels must divide into the norm groups");
        p.gn_sum = gn_sums; p.gn_groups = gn_groups; p.gn_cpg = cout / gn_groups;
    }
    return launch_conv(p, 1, (hipStream_t)stream);
}

// y: [B][oh][ow][mid], x: [B][h2][w2][cin] (sampled at `stride`), w: [cout][mid + cin] (BN scales already folded in),
// out = relu?(y . w[:, :mid] + x[::stride, ::stride] . w[:, mid:] + shift)
int quber_op_conv1x1_dual(const float* y, const float* x, int32_t B, int32_t oh, int32_t ow, int32_t mid, int32_t h2, int32_t w2, int32_t cin, int32_t stride,
                          const float* w, const float* shift, const float* ones, int32_t cout, int32_t relu, float* out, void* stream) {
    ConvP p{};
    p.in = y; p.in2 = x; p.w = w; p.scale = ones; p.shift = shift; p.out = out;
    conv_geometry(p, B, oh, ow, mid, cout, 1, 1, 0, 1);
    p.H2 = h2; p.W2 = w2; p.in2_cs = cin; p.stride2 = stride; p.K1 = mid;
    p.K = mid + cin; p.Kpad = mid + cin; p.relu = relu;
    p.bf16 = g_op_bf16; p.ss_gs = 0;
    p.ws = g_op_ws; p.ws_floats = g_op_ws ? g_op_ws_floats : 0;
    if (g_op_bf16 == 3 && tune().x8) {
        static PlaneScratch scratch;
        const int rs = scratch.split(w, (long)cout * p.Kpad, p, "conv1x1_dual", (hipStream_t)stream);
        if (rs) return rs;
    }
    const int rc = launch_conv_dual(p, 1, (hipStream_t)stream);
    if (rc == 1) return fail("conv1x1_dual: launch not covered by the dual kernel (workspace: tuning key 2)");
    return rc;
}

int quber_op_conv3x3_winograd(const float* x, int32_t B, int32_t h, int32_t w, int32_t cin, const float* w_oihw, int32_t cout, int32_t dil, int32_t m,
                              const float* scale, const float* shift, int32_t relu, float* u, float* ws, int64_t ws_floats, float* y, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!winograd_eligible(3, 1, dil, dil, cin, cout)) return fail("winograd: unsupported channel counts");
    if ((scale == nullptr) != (shift == nullptr)) return fail("winograd: scale and shift go together");
    if (m != 2 && m != 4 && m != 6) return fail("winograd: the output tile edge is 2, 4 or 6");
    int rc = g_op_wino_reuse ? 0 : launch_winograd_weights(w_oihw, cout, cin, m, u, st);
    if (rc) return rc;
    WinoP q{};
    q.in = mkview(x, B, h, w, cin); q.out = mkview(y, B, h, w, cout);
    q.u = u; q.scale = scale; q.shift = shift; q.ss_gs = 0; q.relu = relu; q.dil = dil; q.m = m;
    q.dtype = g_op_bf16;
    q.pack = tune().wino_pack;           // key 51, read per call
    q.ws = ws; q.ws_floats = (size_t)ws_floats;
    if (op_wino_single(q, B, 1)) {
        rc = winograd_fused_prepare();
        if (rc) return rc;
        rc = g_op_wino_reuse ? 0 : launch_winograd_fused_pack(u, cout, cin, ws, st);
        if (rc) return rc;
    }
    q.splitk_ws = g_op_ws; q.splitk_floats = g_op_ws ? g_op_ws_floats : 0;
    return launch_conv_winograd(q, B, 1, st);
}

// ---- the convolution launchers on explicit views, groups and GroupNorm sums (tests): arguments -> ConvP / WinoP -> launcher, nothing else ----
// the ConvP of quber_op_conv2d_view (and of quber_debug_conv_route, whose pointers are stand-ins that nothing dereferences)
static void conv_view_p(ConvP& p, const float* x, int x_cs, long x_gs, const float* packed, const float* scale, const float* shift, const float* res, int res_cs,
                        long res_gs, float* y, int y_cs, long y_gs, int B, int h, int w, int cin, int cout, int k, int stride, int pad, int dil, int relu,
                        double* gn_sums, int gn_groups, float* ws) {
    const int Kpad = (k * k * cin + 31) / 32 * 32;
    const bool skip_rows = g_op_skip_rows && k == 3 && stride == 1 && dil > 1 && cin % 32 == 0;
    p.in = x; p.w = packed; p.scale = scale; p.shift = shift; p.res = res; p.out = y;
    conv_geometry(p, B, h, w, cin, cout, k, stride, pad, dil);
    p.in_cs = x_cs; p.out_cs = y_cs; p.res_cs = res_cs; p.Kpad = Kpad; p.relu = relu;
    p.in_gs = x_gs; p.out_gs = y_gs; p.res_gs = res ? res_gs : 0; p.w_gs = (long)cout * Kpad; p.ss_gs = cout;
    p.kmode = (k > 1 && cin % 32 == 0 && !skip_rows) ? 1 : 0; p.skip_rows = skip_rows;
    p.bf16 = g_op_bf16;
    p.ws = ws; p.ws_floats = ws ? g_op_ws_floats : 0;
    if (gn_sums) { p.gn_sum = gn_sums; p.gn_groups = gn_groups; p.gn_cpg = cout / gn_groups; }
}

int quber_op_conv2d_view(const float* x, int32_t x_cs, int64_t x_gs, const float* w_oihw, const float* scale, const float* shift, const float* residual,
                         int32_t res_cs, int64_t res_gs, float* y, int32_t y_cs, int64_t y_gs, int32_t G, int32_t B, int32_t h, int32_t w, int32_t cin,
                         int32_t cout, int32_t k, int32_t stride, int32_t pad, int32_t dil, int32_t relu, double* gn_sums, int32_t gn_groups, float* packed,
                         void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (G < 1 || k < 1 || stride < 1 || dil < 1 || pad < 0 || cin < 1 || cout < 1) return fail("conv2d_view: bad geometry");
    if (gn_sums && (gn_groups < 1 || cout % gn_groups)) return fail("conv2d_view: channels must divide into the norm groups");
    ConvP p{};
    conv_view_p(p, x, x_cs, (long)x_gs, packed, scale, shift, residual, res_cs, (long)res_gs, y, y_cs, (long)y_gs, B, h, w, cin, cout, k, stride, pad, dil, relu,
                gn_sums, gn_groups, g_op_ws);
    if (p.OH < 1 || p.OW < 1) return fail("conv2d_view: empty output");
    for (int g = 0; g < G; ++g)
        hipLaunchKernelGGL(pack_oihw_kernel, dim3(256), dim3(256), 0, st, w_oihw + (size_t)g * cout * cin * k * k, cout, cin, k, p.Kpad, p.kmode, packed + (size_t)g * p.w_gs);
    if (g_op_bf16 == 3 && k == 1 && tune().x8) {
        static PlaneScratch scratch;
        const int rc = scratch.split(packed, (long)G * cout * p.Kpad, p, "conv2d_view", st);
        if (rc) return rc;
    }
    return launch_conv(p, G, st);
}

static void route_out(const ConvRoute& r, int32_t* out) {
    const int v[12] = {r.kernel, r.sums, r.BM, r.BN, r.S, r.tail_shift, r.tiles, r.blocks, r.nk, r.min_share, r.packed, r.shared_v};
    for (int i = 0; i < 12; ++i) out[i] = v[i];
}
static float* const kDryBase = reinterpret_cast<float*>((uintptr_t)1 << 20);      // never dereferenced

// the route launch_conv takes for the launch quber_op_conv2d_view would make of these arguments on the process keys (host only: nothing is launched, no
// device is queried).  x_off / y_off / res_off: element offsets of the views in 16-byte-aligned buffers (res_off < 0: no residual); workspace != 0: as
// with key 2 set; cus: the compute units to assume.  out[12]: kernel, sums, BM, BN, S, tail_shift, tiles, blocks, nk, min_share, packed, shared_v (ConvRoute)

int quber_debug_conv_route(int32_t x_off, int32_t x_cs, int64_t x_gs, int32_t affine, int32_t res_off, int32_t res_cs, int64_t res_gs, int32_t y_off, int32_t y_cs,
                           int64_t y_gs, int32_t G, int32_t B, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t k, int32_t stride, int32_t pad, int32_t dil,
                           int32_t gn_groups, int32_t workspace, int32_t cus, int32_t* out) {
    if (G < 1 || k < 1 || stride < 1 || dil < 1 || pad < 0 || cin < 1 || cout < 1 || !out) return fail("conv_route: bad geometry");
    if (gn_groups && (gn_groups < 1 || cout % gn_groups)) return fail("conv_route: channels must divide into the norm groups");
    ConvP p{};
    float* const b = kDryBase;
    conv_view_p(p, b + x_off, x_cs, (long)x_gs, b, affine ? b : nullptr, affine ? b : nullptr, res_off >= 0 ? b + res_off : nullptr, res_cs, (long)res_gs, b + y_off, y_cs,
                (long)y_gs, B, h, w, cin, cout, k, stride, pad, dil, 0, gn_groups ? reinterpret_cast<double*>(b) : nullptr, gn_groups, workspace ? b : nullptr);
    if (p.OH < 1 || p.OW < 1) return fail("conv_route: empty output");
    if (g_op_bf16 == 3 && k == 1 && tune().x8) { p.w3 = b; p.w3_plane = (long)G * cout * p.Kpad; }
    ConvRoute r{};
    r.cus = cus;
    const int rc = launch_conv(p, G, nullptr, &r);
    if (rc) return rc;
    route_out(r, out);
    return 0;
}

// the WinoP of quber_op_conv3x3_winograd_view
static void wino_view_q(WinoP& q, const float* x, int x_cs, long x_gs, float* y, int y_cs, long y_gs, int B, int h, int w, int cin, int cout, int dil, int m,
                        const float* scale, const float* shift, int relu, const float* u, float* ws, size_t ws_floats, double* gn_sums, int gn_groups,
                        const double* n_stats, const float* n_gamma, const float* n_beta, int n_param_gs, int n_groups, int n_relu, float n_eps, float* splitk_ws) {
    q.in = mkview(x, B, h, w, cin); q.in.cs = x_cs; q.in.gs = x_gs;
    q.out = mkview(y, B, h, w, cout); q.out.cs = y_cs; q.out.gs = y_gs;
    q.u = u; q.scale = scale; q.shift = shift; q.ss_gs = cout; q.relu = relu; q.dil = dil; q.m = m;
    q.dtype = g_op_bf16;
    q.pack = tune().wino_pack;
    q.ws = ws; q.ws_floats = ws_floats;
    q.gn_sum = gn_sums; q.gn_groups = gn_sums ? gn_groups : 0;
    if (n_stats) q.norm = WinoNorm{n_stats, n_gamma, n_beta, n_groups, 0, n_param_gs, n_relu, 0.0, n_eps};
    q.splitk_ws = splitk_ws; q.splitk_floats = splitk_ws ? g_op_ws_floats : 0;
}

int quber_op_conv3x3_winograd_view(const float* x, int32_t x_cs, int64_t x_gs, const float* w_oihw, const float* scale, const float* shift, float* y, int32_t y_cs,
                                   int64_t y_gs, int32_t G, int32_t B, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t dil, int32_t m, int32_t relu,
                                   double* gn_sums, int32_t gn_groups, const double* n_stats, const float* n_gamma, const float* n_beta, int32_t n_param_gs,
                                   int32_t n_groups, int32_t n_relu, float n_eps, float* u, float* ws, int64_t ws_floats, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (G < 1 || !winograd_eligible(3, 1, dil, dil, cin, cout)) return fail("winograd_view: unsupported channel counts");
    if ((scale == nullptr) != (shift == nullptr)) return fail("winograd_view: scale and shift go together");
    if (m != 2 && m != 4 && m != 6) return fail("winograd_view: the output tile edge is 2, 4 or 6");
    if (gn_sums && (gn_groups < 1 || cout % gn_groups)) return fail("winograd_view: channels must divide into the norm groups");
    const size_t P = (size_t)(m + 2) * (m + 2);
    for (int g = 0; g < G; ++g) {
        const int rc = launch_winograd_weights(w_oihw + (size_t)g * cout * cin * 9, cout, cin, m, u + g * P * cout * cin, st);
        if (rc) return rc;
    }
    WinoP q{};
    wino_view_q(q, x, x_cs, (long)x_gs, y, y_cs, (long)y_gs, B, h, w, cin, cout, dil, m, scale, shift, relu, u, ws, (size_t)ws_floats, gn_sums, gn_groups, n_stats,
                n_gamma, n_beta, n_param_gs, n_groups, n_relu, n_eps, g_op_ws);
    if (op_wino_single(q, B, G)) {
        int rc = winograd_fused_prepare();
        if (rc) return rc;
        for (int g = 0; g < G; ++g) {
            rc = launch_winograd_fused_pack(u + g * P * cout * cin, cout, cin, const_cast<float*>(q.uf) + g * P * cout * cin, st);
            if (rc) return rc;
        }
    }
    return launch_conv_winograd(q, B, G, st);
}

// ... and its route (host only); in_place: y is x; norm / gn_groups != 0: an input norm / sums are requested; out[12] as quber_debug_conv_route
int quber_debug_winograd_route(int32_t x_cs, int64_t x_gs, int32_t y_cs, int64_t y_gs, int32_t in_place, int32_t G, int32_t B, int32_t h, int32_t w, int32_t cin,
                               int32_t cout, int32_t dil, int32_t m, int32_t gn_groups, int32_t norm_groups, int64_t ws_floats, int32_t* out) {
    if (G < 1 || !out || !winograd_eligible(3, 1, dil, dil, cin, cout)) return fail("winograd_route: unsupported channel counts");
    if (m != 2 && m != 4 && m != 6) return fail("winograd_route: the output tile edge is 2, 4 or 6");
    if (gn_groups && cout % gn_groups) return fail("winograd_route: channels must divide into the norm groups");
    float* const b = kDryBase;
    WinoP q{};
    wino_view_q(q, b, x_cs, (long)x_gs, in_place ? b : b + (1 << 20), y_cs, (long)y_gs, B, h, w, cin, cout, dil, m, nullptr, nullptr, 0, b, b, (size_t)ws_floats,
                gn_groups ? reinterpret_cast<double*>(b) : nullptr, gn_groups, norm_groups ? reinterpret_cast<const double*>(b) : nullptr, b, b, cin, norm_groups, 1,
                1e-5f, nullptr);
    (void)op_wino_single(q, B, G);
    ConvRoute r{};
    const int rc = launch_conv_winograd(q, B, G, nullptr, &r);
    if (rc) return rc;
    route_out(r, out);
    return 0;
}

// the ConvP of the dual op: y [G][B][oh][ow][mid] (gs y_gs), x [G][B][h2][w2][cin] (x_gs), w [G][cout][mid + cin] (w_gs), shift / ones [G][cout] (ss_gs), out (out_gs)
static void dual_view_p(ConvP& p, const float* y, long y_gs, const float* x, long x_gs, const float* w, long w_gs, const float* shift, const float* ones, int ss_gs,
                        float* out, long out_gs, int B, int oh, int ow, int mid, int h2, int w2, int cin, int stride, int cout, int relu, float* ws) {
    p.in = y; p.in2 = x; p.w = w; p.scale = ones; p.shift = shift; p.out = out;
    conv_geometry(p, B, oh, ow, mid, cout, 1, 1, 0, 1);
    p.H2 = h2; p.W2 = w2; p.in2_cs = cin; p.stride2 = stride; p.K1 = mid;
    p.K = mid + cin; p.Kpad = mid + cin; p.relu = relu;
    p.in_gs = y_gs; p.in2_gs = x_gs; p.w_gs = w_gs; p.ss_gs = ss_gs; p.out_gs = out_gs;
    p.bf16 = g_op_bf16;
    p.ws = ws; p.ws_floats = ws ? g_op_ws_floats : 0;
}

int quber_op_conv1x1_dual_view(const float* y, int64_t y_gs, const float* x, int64_t x_gs, const float* w, int64_t w_gs, const float* shift, const float* ones,
                               int32_t ss_gs, float* out, int64_t out_gs, int32_t G, int32_t B, int32_t oh, int32_t ow, int32_t mid, int32_t h2, int32_t w2, int32_t cin,
                               int32_t stride, int32_t cout, int32_t relu, void* stream) {
    if (G < 1) return fail("conv1x1_dual_view: bad geometry");
    ConvP p{};
    dual_view_p(p, y, (long)y_gs, x, (long)x_gs, w, (long)w_gs, shift, ones, ss_gs, out, (long)out_gs, B, oh, ow, mid, h2, w2, cin, stride, cout, relu, g_op_ws);
    if (g_op_bf16 == 3 && tune().x8) {
        static PlaneScratch scratch;
        const int rs = scratch.split(w, (long)(G - 1) * w_gs + (long)cout * p.Kpad, p, "conv1x1_dual_view", (hipStream_t)stream);
        if (rs) return rs;
    }
    const int rc = launch_conv_dual(p, G, (hipStream_t)stream);
    if (rc == 1) return fail("conv1x1_dual_view: launch not covered by the dual kernel (workspace: tuning key 2)");
    return rc;
}

int quber_debug_dual_route(int64_t y_gs, int64_t x_gs, int64_t w_gs, int32_t ss_gs, int64_t out_gs, int32_t G, int32_t B, int32_t oh, int32_t ow, int32_t mid, int32_t h2,
                           int32_t w2, int32_t cin, int32_t stride, int32_t cout, int32_t workspace, int32_t cus, int32_t* out) {
    if (G < 1 || !out) return fail("dual_route: bad geometry");
    float* const b = kDryBase;
    ConvP p{};
    dual_view_p(p, b, (long)y_gs, b, (long)x_gs, b, (long)w_gs, b, b, ss_gs, b, (long)out_gs, B, oh, ow, mid, h2, w2, cin, stride, cout, 0, workspace ? b : nullptr);
    if (g_op_bf16 == 3 && tune().x8) { p.w3 = b; p.w3_plane = (long)(G - 1) * w_gs + (long)cout * p.Kpad; }
    ConvRoute r{};
    r.cus = cus;
    const int rc = launch_conv_dual(p, G, nullptr, &r);
    if (rc == 1) return fail("dual_route: launch not covered by the dual kernel");
    if (rc) return rc;
    route_out(r, out);
    return 0;
}

int quber_op_groupnorm(const float* x, int32_t B, int32_t h, int32_t w, int32_t c, int32_t groups, const float* gamma,
                       const float* beta, float eps, int32_t relu, double* stats, float* y, void* stream) {
    View in = mkview(x, B, h, w, c), out = mkview(y, B, h, w, c);
    int rc = launch_gn_stats(in, B, 1, groups, stats, (hipStream_t)stream);
    if (rc) return rc;
    return launch_gn_apply(in, out, B, 1, groups, stats, gamma, beta, 0, eps, relu, (hipStream_t)stream);
}

int quber_op_bilinear(const float* x, int32_t B, int32_t h, int32_t w, int32_t c, int32_t oh, int32_t ow, float* y,
                      void* stream) {
    if (c % 4) return fail("bilinear: channels must be a multiple of 4");
    return launch_bilinear(mkview(x, B, h, w, c), mkview(y, B, oh, ow, c), B, (hipStream_t)stream);
}

// ---- the glue kernels of elementwise.hip on explicit views (tests): arguments -> View -> launcher, nothing else ----
static View opview(const void* p, int B, int h, int w, int c, int cs, long gs, int es) {
    View v;
    v.p = reinterpret_cast<float*>(const_cast<void*>(p)); v.B = B; v.H = h; v.W = w; v.C = c; v.cs = cs; v.gs = gs; v.es = es;
    return v;
}

int32_t quber_debug_gn_pixels_per_block(int32_t hw, int32_t c, int32_t batch, int32_t groups_of_launch, int32_t stats_pass) {
    return gn_pixels_per_block(hw, c, batch, groups_of_launch, stats_pass != 0);
}

int quber_op_gn_stats(const void* x, int32_t x_cs, int64_t x_gs, int32_t es, int32_t B, int32_t h, int32_t w, int32_t c, int32_t G, int32_t groups,
                      double* stats, int32_t zero, void* stream) {
    return launch_gn_stats(opview(x, B, h, w, c, x_cs, x_gs, es), B, G, groups, stats, (hipStream_t)stream, zero != 0);
}

int quber_op_gn_apply(const void* x, int32_t x_cs, int64_t x_gs, int32_t x_es, void* y, int32_t y_cs, int64_t y_gs, int32_t y_es, int32_t B, int32_t h,
                      int32_t w, int32_t c, int32_t G, int32_t groups, const double* stats, const float* gamma, const float* beta, int32_t param_gs,
                      float eps, int32_t relu, void* stream) {
    return launch_gn_apply(opview(x, B, h, w, c, x_cs, x_gs, x_es), opview(y, B, h, w, c, y_cs, y_gs, y_es), B, G, groups, stats, gamma, beta,
                           param_gs, eps, relu, (hipStream_t)stream);
}

int quber_op_maxpool_view(const void* x, int32_t x_cs, int64_t x_gs, int32_t x_es, void* y, int32_t y_cs, int64_t y_gs, int32_t y_es, int32_t B,
                          int32_t h, int32_t w, int32_t c, int32_t G, void* stream) {
    return launch_maxpool3x3s2(opview(x, B, h, w, c, x_cs, x_gs, x_es), opview(y, B, (h + 1) / 2, (w + 1) / 2, c, y_cs, y_gs, y_es), B, G,
                               (hipStream_t)stream);
}

int quber_op_bilinear_view(const void* x, int32_t x_cs, int32_t x_es, void* y, int32_t y_cs, int32_t y_es, int32_t B, int32_t h, int32_t w, int32_t c,
                           int32_t oh, int32_t ow, void* stream) {
    return launch_bilinear(opview(x, B, h, w, c, x_cs, 0, x_es), opview(y, B, oh, ow, c, y_cs, 0, y_es), B, (hipStream_t)stream);
}

int quber_op_avgpool(const void* x, int32_t x_cs, int32_t x_es, void* y, int32_t y_cs, int32_t y_es, int32_t B, int32_t h, int32_t w, int32_t c,
                     void* stream) {
    return launch_avgpool(opview(x, B, h, w, c, x_cs, 0, x_es), opview(y, B, 1, 1, c, y_cs, 0, y_es), B, (hipStream_t)stream);
}

int quber_op_add_channels(const void* a, int32_t a_cs, int32_t a_es, const void* b, int32_t b_cs, int32_t b_es, void* y, int32_t y_cs, int32_t y_es,
                          int32_t B, int32_t h, int32_t w, int32_t c, void* stream) {
    return launch_add_channels(opview(a, B, h, w, c, a_cs, 0, a_es), opview(b, B, h, w, c, b_cs, 0, b_es), opview(y, B, h, w, c, y_cs, 0, y_es), B,
                               (hipStream_t)stream);
}

int quber_op_copy_channels(const void* x, int32_t x_cs, int32_t x_es, void* y, int32_t y_cs, int32_t y_es, int32_t B, int32_t h, int32_t w, int32_t c,
                           void* stream) {
    return launch_copy_channels(opview(x, B, h, w, c, x_cs, 0, x_es), opview(y, B, h, w, c, y_cs, 0, y_es), B, (hipStream_t)stream);
}

// the per-head arrays are HOST arrays of n entries (device pointers / integers); a head without an activation destination passes null there
int quber_op_predictors(int32_t n, const void* const* feat, const float* const* w, const float* const* bias, void* const* act_dst, const int32_t* cout,
                        const int32_t* q_ch0, const int32_t* act, int32_t c, int32_t feat_cs, int32_t es, int32_t B, int32_t h, int32_t wd, float* q,
                        int32_t q_nch, int32_t act_cs, void* stream) {
    PredHeads hs{};
    hs.n = n;
    for (int j = 0; j < n && j < 5; ++j) {
        hs.in[j] = feat[j]; hs.w[j] = w[j]; hs.bias[j] = bias[j]; hs.sm[j] = act_dst[j];
        hs.cout[j] = cout[j]; hs.q_ch0[j] = q_ch0[j]; hs.act[j] = act[j];
    }
    return launch_predictors(hs, c, feat_cs, es, h, wd, q, q_nch, act_cs, B, (hipStream_t)stream);
}

int quber_op_upsample_logits(const float* q, float* out, int32_t B, int32_t nch, int32_t h, int32_t w, int32_t scale, int32_t oh, int32_t ow,
                             uint32_t mul_mask, void* stream) {
    return launch_upsample_logits(q, out, B, nch, h, w, scale, oh, ow, mul_mask, (hipStream_t)stream);
}

// mean6 / std6: HOST arrays; x: [streams][batch_cap][h][w][x_c]
int quber_op_preprocess(const uint8_t* rgb, const uint8_t* depth, const float* offs, void* x, int32_t x_c, int32_t es, int32_t B, int32_t batch_cap,
                        int32_t h, int32_t w, const float* mean6, const float* std6, int32_t streams, void* stream) {
    return launch_preprocess(rgb, depth, offs, opview(x, batch_cap, h, w, x_c, x_c, (long)batch_cap * h * w * x_c, es), B, batch_cap, h, w, mean6,
                             std6, streams, (hipStream_t)stream);
}

int quber_op_group_pixels(const float* logits, int32_t n_planes, int32_t batch, int32_t h, int32_t w, int32_t cap,
                          const int32_t* centers, const int32_t* ncenters, uint8_t* ids, uint32_t* area, void* stream) {
    if (!logits || !centers || !ncenters || !ids || !area || batch < 1 || h < 1 || w < 1) return fail("bad argument to quber_op_group_pixels");
    return launch_group_pixels(logits, n_planes, batch, h, w, cap, centers, ncenters, ids, area, (hipStream_t)stream);
}

// ---- the LMFFNet kernels of lmff.hip on explicit fp32 views (tests): arguments -> View -> launcher, nothing else ----
static View lview(const void* p, int B, int h, int w, int c, int cs) { return opview(p, B, h, w, c, cs, 0, 4); }

int quber_op_lmff_preprocess(const uint8_t* bgr, const uint8_t* depth, int64_t pixels, float* x, void* stream) {
    return launch_lmff_preprocess(bgr, depth, (long)pixels, x, (hipStream_t)stream);
}

int quber_op_lmff_dwconv(const float* x, int32_t x_cs, float* y, int32_t y_cs, int32_t B, int32_t h, int32_t w, int32_t c, int32_t dil, const float* w9,
                         const float* scale, const float* shift, const float* slope, void* stream) {
    return launch_dwconv3x3(lview(x, B, h, w, c, x_cs), lview(y, B, h, w, c, y_cs), B, dil, w9, scale, shift, slope, (hipStream_t)stream);
}

int quber_op_lmff_pool(const float* x, int32_t x_cs, float* y, int32_t y_cs, int32_t B, int32_t h, int32_t w, int32_t c, int32_t oh, int32_t ow, int32_t mode,
                       void* stream) {
    return launch_pool_s2(lview(x, B, h, w, c, x_cs), lview(y, B, oh, ow, c, y_cs), B, mode, (hipStream_t)stream);
}

int quber_op_lmff_affine(const float* a, int32_t a_cs, const float* b, int32_t b_cs, float* y, int32_t y_cs, int32_t B, int32_t h, int32_t w, int32_t c,
                         const float* scale, const float* shift, const float* slope, void* stream) {
    const View bv = lview(b, B, h, w, c, b_cs);
    return launch_affine_prelu(lview(a, B, h, w, c, a_cs), b ? &bv : nullptr, lview(y, B, h, w, c, y_cs), B, scale, shift, slope, (hipStream_t)stream);
}

int quber_op_lmff_pmca(const float* x, int32_t x_cs, int32_t B, int32_t h, int32_t w, int32_t c, const float* w2x2, const float* fc0, const float* alpha,
                       const float* fc2, float* wts, double* sums, void* stream) {
    return launch_pmca(lview(x, B, h, w, c, x_cs), B, w2x2, fc0, alpha, fc2, wts, sums, (hipStream_t)stream);
}

int quber_op_lmff_scale(const float* x, int32_t x_cs, const float* wts, float* y, int32_t y_cs, int32_t B, int32_t h, int32_t w, int32_t c, void* stream) {
    return launch_scale_channels(lview(x, B, h, w, c, x_cs), wts, lview(y, B, h, w, c, y_cs), B, (hipStream_t)stream);
}

int quber_op_lmff_gate(const float* o, int32_t o_cs, const float* att, int32_t att_cs, float* q, int32_t B, int32_t h, int32_t w, int32_t c, void* stream) {
    return launch_mad_gate(lview(o, B, h, w, c, o_cs), lview(att, B, h, w, c, att_cs), q, B, c, (hipStream_t)stream);
}

// ---- the CGNet kernels of cgnet.hip on explicit fp32 views (tests): arguments -> View -> launcher, nothing else ----
int32_t quber_op_cgnet_tiles(int32_t h, int32_t w, int32_t joint) {
    if (h < 1 || w < 1) return 0;
    return joint ? cg_joint_tiles(h, w) : cg_sums_tiles(h, w);
}

int quber_op_cgnet_joint(const float* x, int32_t x_cs, float* joi, int32_t joi_cs, int32_t B, int32_t h, int32_t w, int32_t c, int32_t dil, const float* w1,
                         const float* scale1, const float* shift1, const float* slope1, const float* wloc, const float* wsur, const float* scale2,
                         const float* shift2, const float* slope2, double* partials, int32_t tiles, void* stream) {
    return launch_cg_joint(lview(x, B, h, w, c, x_cs), lview(joi, B, h, w, c, joi_cs), B, dil, w1, scale1, shift1, slope1, wloc, wsur, scale2, shift2, slope2, partials,
                           tiles, (hipStream_t)stream);
}

int quber_op_cgnet_sums(const float* x, int32_t x_cs, int32_t B, int32_t h, int32_t w, int32_t c, double* partials, int32_t tiles, void* stream) {
    return launch_cg_sums(lview(x, B, h, w, c, x_cs), B, partials, tiles, (hipStream_t)stream);
}

int quber_op_cgnet_apply(const float* joi, int32_t joi_cs, const float* x, int32_t x_cs, float* out, int32_t out_cs, int32_t B, int32_t h, int32_t w, int32_t c,
                         int32_t hidden, const double* partials, int32_t tiles, const float* fc0, const float* b0, const float* fc2, const float* b2, float* mean,
                         float* y, void* stream) {
    const View xv = lview(x, B, h, w, c, x_cs);
    return launch_cg_apply(lview(joi, B, h, w, c, joi_cs), x ? &xv : nullptr, lview(out, B, h, w, c, out_cs), B, hidden, partials, tiles, fc0, b0, fc2, b2, mean, y,
                           (hipStream_t)stream);
}

// ---- the Depth Seeding Network kernels of dsn.hip on explicit fp32 views (tests): arguments -> View -> launcher, nothing else ----
int32_t quber_op_esp_tiles(int32_t h, int32_t w) { return (h < 1 || w < 1) ? 0 : esp_tiles(h, w); }
int quber_op_esp_kernel(int n1) { return esp_kernel(n1); }
int64_t quber_op_esp_packed_floats(int32_t n1) { return esp_kernel(n1) ? (int64_t)esp_packed_floats(n1) : 0; }

int quber_op_dsn_pack(const float* xyz, int32_t B, int32_t h, int32_t w, int32_t flags, float* x8, float* clean, void* stream) {
    return launch_dsn_pack(xyz, B, h, w, flags, x8, clean, (hipStream_t)stream);
}
int quber_op_xyz_from_depth(const float* z, int32_t B, int32_t h, int32_t w, const double* cam, int32_t convention, int32_t flags, float* xyz_raw, float* x8, float* clean,
                            void* stream) {
    return launch_xyz_from_depth(z, B, h, w, cam, convention, flags, xyz_raw, x8, clean, (hipStream_t)stream);
}

int quber_op_esp_pack(const float* w1, const float* w2, const float* w4, const float* w8, const float* w16, int32_t n, int32_t n1, float* packed, void* stream) {
    const float* const w[5] = {w1, w2, w4, w8, w16};
    return launch_esp_pack(w, n, n1, packed, (hipStream_t)stream);
}

int quber_op_esp_branches(const float* t, int32_t t_cs, const float* x, int32_t x_cs, float* out, int32_t out_cs, int32_t B, int32_t h, int32_t w, int32_t c,
                          int32_t groups, const float* packed, double* partials, int32_t tiles, void* stream) {
    const int n = c / 5, n1 = c - 4 * n;
    const View xv = lview(x, B, h, w, c, x_cs);
    return launch_esp_branches(lview(t, B, h, w, n, t_cs), x ? &xv : nullptr, lview(out, B, h, w, c, out_cs), B, n, n1, groups, packed, partials, tiles,
                               (hipStream_t)stream);
}

int quber_op_esp_merge(const float* d1, int32_t d1_cs, const float* d2, const float* d4, const float* d8, const float* d16, int32_t d_cs, const float* x,
                       int32_t x_cs, float* out, int32_t out_cs, int32_t B, int32_t h, int32_t w, int32_t c, int32_t groups, double* partials, int32_t tiles,
                       void* stream) {
    const int n = c / 5, n1 = c - 4 * n;
    const View d[5] = {lview(d1, B, h, w, n1, d1_cs), lview(d2, B, h, w, n, d_cs), lview(d4, B, h, w, n, d_cs), lview(d8, B, h, w, n, d_cs),
                       lview(d16, B, h, w, n, d_cs)};
    const View xv = lview(x, B, h, w, c, x_cs);
    return launch_esp_merge(d, x ? &xv : nullptr, lview(out, B, h, w, c, out_cs), B, n, n1, groups, partials, tiles, (hipStream_t)stream);
}

int quber_op_esp_stats(const double* partials, int32_t B, int32_t tiles, int32_t groups, double* stats, void* stream) {
    return launch_esp_stats(partials, B, tiles, groups, stats, (hipStream_t)stream);
}

int quber_op_dsn_head(const float* f, int32_t f_cs, int32_t B, int32_t h, int32_t w, int32_t c, const float* clean, const float* wfg, const float* wcd,
                      float* logits, float* offsets, float* votes, uint8_t* classes, uint8_t* fg, void* stream) {
    return launch_dsn_head(lview(f, B, h, w, c, f_cs), B, clean, wfg, wcd, logits, offsets, votes, classes, fg, (hipStream_t)stream);
}

// ---- the Region Refinement Network kernels of rrn.hip on explicit fp32 views (tests): arguments -> View -> launcher, nothing else ----
int quber_op_rrn_pack(const float* rgb, const uint8_t* mask, int32_t B, int32_t h, int32_t w, float* x8, void* stream) {
    return launch_rrn_pack(rgb, mask, B, h, w, x8, (hipStream_t)stream);
}

int quber_op_rrn_head(const float* f, int32_t f_cs, int32_t B, int32_t h, int32_t w, int32_t c, const float* wfg, float thr, float* logits, uint8_t* refined,
                      void* stream) {
    return launch_rrn_head(lview(f, B, h, w, c, f_cs), B, wfg, thr, logits, refined, (hipStream_t)stream);
}

int quber_op_rrn_head3(const float* f, int32_t f_cs, int32_t B, int32_t h, int32_t w, int32_t c, const float* w9, float bias, float thr, float* logits,
                       uint8_t* refined, void* stream) {
    return launch_rrn_head3(lview(f, B, h, w, c, f_cs), B, w9, bias, thr, logits, refined, (hipStream_t)stream);
}

int quber_op_maxpool3x3s2(const float* x, int32_t B, int32_t h, int32_t w, int32_t c, float* y, void* stream) {
    if (c % 4) return fail("maxpool: channels must be a multiple of 4");
    return launch_maxpool3x3s2(mkview(x, B, h, w, c), mkview(y, B, (h + 1) / 2, (w + 1) / 2, c), B, 1, (hipStream_t)stream);
}

}  // extern "C"
