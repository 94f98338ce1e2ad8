// Kernels of CGNet, the foreground network of the UOAIS base model (reference foreground_segmentation/cgnet.py), and of the
// filter built on it (eval/base_model.py:210-216, foreground_segmentation/predictor.py:43-50).
//
// A context-guided block (cgnet.py:231-261) is   t = prelu(bn(W1 x))  (1x1, C -> C/2)
//                                               joi = prelu(bn([dw3x3(t) | dw3x3 dilated(t)]))
//                                               out = x + joi * sigmoid(fc2(relu(fc0(mean(joi)) + b0)) + b2)
// on maps of 1/4 and 1/8 of a 320 x 240 frame, 22 times: from separate launchers that is a 1x1 GEMM, two depthwise passes, a pooling pass
// and a scale pass per block, all of them far below one round of the chip.  Here a block is two kernels:
//   cg_joint_kernel   one workgroup per (frame, 8 x 8 output tile).  t of the tile plus a halo of `dil` pixels is computed into LDS with
//                     v_mfma_f32_16x16x4_f32 (exact fp32: an fmaf chain over K), rows = patch pixels, columns = the C/2 channels; the
//                     pixel operand goes from global memory into registers sixteen channels at a time, the weights stay in
//                     registers, so LDS holds only the result: 256 pixels x 64 channels x 4 B = 64 KB at C = 128, dil = 4.  The zero
//                     padding of the depthwise convolutions is a padding of t: patch positions outside the image are stored as 0,
//                     not as prelu(shift).  Both depthwise 3x3 then read LDS, the folded BN + PReLU of the concatenation is
//                     applied, joi goes to global memory and the tile's per-channel sums (float64) to partials[frame][tile][C].
//   cg_apply_kernel   every workgroup adds the partials of its frame in tile order (float64, no atomics: two runs give the same bits),
//                     divides by h w, evaluates the two fully connected layers (C / r <= 8 hidden units) and writes
//                     out = [x +] joi * y for its share of the pixels, into a view that may be a channel slice of a wider buffer.
// cg_sums_kernel writes the same partials for a tensor that another launcher produced (the down blocks' `reduce` output; the
// blocks of the unfused plan, option key 52 = 0).  No kernel waits for another workgroup.
#include "common.h"

namespace quber {

namespace {

constexpr int CG_TILE = 8;            // output tile edge of cg_joint_kernel
constexpr int CG_MAX_DIL = 4;         // largest halo: (8 + 2 * 4)^2 = 256 patch pixels
constexpr int CG_CHUNK = 64;          // pixels per tile of cg_sums_kernel

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct CgJoint {
    const float* x; int x_cs;
    float* joi; int joi_cs;
    int H, W, dil, tiles_x, tiles;
    const float *w1, *s1, *h1, *a1;           // 1x1 weights [C/2][C], its folded BN + PReLU [C/2]
    const float *wloc, *wsur;                 // depthwise filters [C/2][9]
    const float *s2, *h2, *a2;                // folded BN + PReLU of the concatenation [C]
    double* partials;                         // [B][tiles][C]
};

// LDS column of channel c of patch pixel q.  64-channel rows are exactly 64 banks wide: the rows a wave writes at once (q = 4 g + r,
// g = 0..3) are rotated against each other by 16 columns; 32-channel rows are padded to 36 instead.
template <int CH> __device__ __forceinline__ int cg_col(int q, int c) {
    if constexpr (CH == 64) return (c + 16 * ((q >> 2) & 3)) & 63;
    else return c;
}

template <int C>
__global__ __launch_bounds__(256) void cg_joint_kernel(const CgJoint a) {
    constexpr int CH = C / 2, NT = CH / 16, KJ = C / 16;
    constexpr int S = CH == 64 ? 64 : CH + 4;                 // LDS row stride in floats
    __shared__ __attribute__((aligned(16))) float lds[256 * S];     // 64 KB (C = 128) or 36 KB
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int b = blockIdx.y, tile = blockIdx.x;
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int dil = a.dil, P = CG_TILE + 2 * dil, NP = P * P;
    const int y0 = ty * CG_TILE - dil, x0 = tx * CG_TILE - dil;
    const int n = lane & 15, g = lane >> 4;
    const long frame = (long)b * a.H * a.W;

    // ---- t = prelu(bn(W1 x)) on the patch.  MFMA 16x16x4: A[i = lane & 15][k = lane >> 4] = pixel i, B[k][j = lane & 15] = W1[j][k],
    //      D[4 (lane >> 4) + r][lane & 15].  K runs over the channels in the order (16 j + 4 g + e: j, e) so that a lane's four
    //      consecutive channels are one 16-byte load; A and B use the same order.
    f32x4 wb[NT][KJ];
    float sc[NT], sh[NT], sl[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
        for (int j = 0; j < KJ; ++j) wb[nt][j] = *reinterpret_cast<const f32x4*>(a.w1 + (long)(nt * 16 + n) * C + 16 * j + 4 * g);
        sc[nt] = a.s1[nt * 16 + n]; sh[nt] = a.h1[nt * 16 + n]; sl[nt] = a.a1[nt * 16 + n];
    }
    const int mtiles = (NP + 15) >> 4;
    for (int mt = wave; mt < mtiles; mt += 4) {
        const int p = mt * 16 + n;
        const int py = p / P, px = p - py * P;
        const int y = y0 + py, x = x0 + px;
        const bool ok = p < NP && (unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W;
        f32x4 av[KJ];
        const float* src = a.x + (frame + (long)y * a.W + x) * a.x_cs + 4 * g;
#pragma unroll
        for (int j = 0; j < KJ; ++j) av[j] = ok ? *reinterpret_cast<const f32x4*>(src + 16 * j) : f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < KJ; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j][e], wb[nt][j][e], acc[nt], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q = mt * 16 + 4 * g + r;
            if (q >= NP) continue;
            const int qy = q / P, qx = q - qy * P;
            const bool in = (unsigned)(y0 + qy) < (unsigned)a.H && (unsigned)(x0 + qx) < (unsigned)a.W;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                float v = fmaf(acc[nt][r], sc[nt], sh[nt]);
                v = v > 0.f ? v : v * sl[nt];
                lds[q * S + cg_col<CH>(q, nt * 16 + n)] = in ? v : 0.f;        // the depthwise padding: zeros of t
            }
        }
    }
    __syncthreads();

    // ---- both depthwise 3x3 from LDS, BN + PReLU of the concatenation, joi and the tile's sums
    constexpr int G = 256 / CH;                                // pixel groups: a thread owns one channel pair (c, CH + c) of every G-th pixel
    const int c = t % CH, grp = t / CH;
    float wl[9], ws[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) { wl[k] = a.wloc[c * 9 + k]; ws[k] = a.wsur[c * 9 + k]; }
    const float s2l = a.s2[c], h2l = a.h2[c], a2l = a.a2[c], s2s = a.s2[CH + c], h2s = a.h2[CH + c], a2s = a.a2[CH + c];
    double suml = 0.0, sums = 0.0;
    for (int o = grp; o < CG_TILE * CG_TILE; o += G) {
        const int oy = o >> 3, ox = o & 7;
        const int y = ty * CG_TILE + oy, x = tx * CG_TILE + ox;
        if (y >= a.H || x >= a.W) continue;
        float al = 0.f, as = 0.f;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int pl = (oy + dil + ky - 1) * P + ox + dil + kx - 1;
                const int ps = (oy + dil + (ky - 1) * dil) * P + ox + dil + (kx - 1) * dil;
                al = fmaf(lds[pl * S + cg_col<CH>(pl, c)], wl[ky * 3 + kx], al);
                as = fmaf(lds[ps * S + cg_col<CH>(ps, c)], ws[ky * 3 + kx], as);
            }
        float vl = fmaf(al, s2l, h2l), vs = fmaf(as, s2s, h2s);
        vl = vl > 0.f ? vl : vl * a2l;
        vs = vs > 0.f ? vs : vs * a2s;
        float* dst = a.joi + (frame + (long)y * a.W + x) * a.joi_cs;
        dst[c] = vl;
        dst[CH + c] = vs;
        suml += (double)vl;
        sums += (double)vs;
    }
    __syncthreads();                                           // every read of t is done: the sums reuse its memory
    double* red = reinterpret_cast<double*>(lds);              // [G][C]
    red[grp * C + c] = suml;
    red[grp * C + CH + c] = sums;
    __syncthreads();
    if (t < C) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < G; ++k) s += red[k * C + t];
        a.partials[((long)b * a.tiles + tile) * C + t] = s;
    }
}

// per-channel sums of CG_CHUNK consecutive pixels of a frame -> partials[frame][tile][C], C in {64, 128}
__global__ __launch_bounds__(256) void cg_sums_kernel(const float* __restrict__ in, int cs, int C, int HW, int tiles, double* __restrict__ partials) {
    __shared__ double red[256];                                // [256 / C][C]
    const int t = threadIdx.x, b = blockIdx.y, tile = blockIdx.x;
    const int G = 256 / C, c = t % C, grp = t / C;
    const int p0 = tile * CG_CHUNK, p1 = min(HW, p0 + CG_CHUNK);
    double s = 0.0;
    for (int p = p0 + grp; p < p1; p += G) s += (double)in[((long)b * HW + p) * cs + c];
    red[grp * C + c] = s;
    __syncthreads();
    if (t < C) {
        double r = 0.0;
        for (int k = 0; k < G; ++k) r += red[k * C + t];
        partials[((long)b * tiles + tile) * C + t] = r;
    }
}

struct CgApply {
    const float* joi; int joi_cs;
    const float* x; int x_cs;                 // residual input or null
    float* out; int out_cs;
    int HW, C, R, tiles, ppb;                 // R hidden units; ppb pixels per workgroup
    const double* partials;
    const float *fc0, *b0, *fc2, *b2;         // [R][C], [R], [C][R], [C]
    float *mean, *y;                          // [B][C] each, or null: what workgroup 0 of a frame computed (taps)
};

__global__ __launch_bounds__(256) void cg_apply_kernel(const CgApply a) {
    __shared__ float s_mean[128], s_hid[8];
    __shared__ __attribute__((aligned(16))) float s_y[128];
    const int t = threadIdx.x, b = blockIdx.y, C = a.C, R = a.R;
    if (t < C) {
        const double* p = a.partials + (long)b * a.tiles * C + t;
        double s = 0.0;
        for (int i = 0; i < a.tiles; ++i) s += p[(long)i * C];
        const float m = (float)(s / (double)a.HW);
        s_mean[t] = m;
        if (blockIdx.x == 0 && a.mean) a.mean[(long)b * C + t] = m;
    }
    __syncthreads();
    if (t < 64) {                                              // eight lanes per hidden unit, then a butterfly: the same sum in all eight
        const int unit = t >> 3, part = t & 7;
        float h = 0.f;
        if (unit < R)
            for (int k = part; k < C; k += 8) h = fmaf(s_mean[k], a.fc0[unit * C + k], h);
        h += __shfl_xor(h, 4);
        h += __shfl_xor(h, 2);
        h += __shfl_xor(h, 1);
        if (part == 0 && unit < R) {
            const float v = h + a.b0[unit];
            s_hid[unit] = v > 0.f ? v : 0.f;
        }
    }
    __syncthreads();
    if (t < C) {
        float o = 0.f;
        for (int k = 0; k < R; ++k) o = fmaf(s_hid[k], a.fc2[t * R + k], o);
        o += a.b2[t];
        const float y = (float)(1.0 / (1.0 + exp(-(double)o)));     // the sigmoid in float64: correctly rounded from o
        s_y[t] = y;
        if (blockIdx.x == 0 && a.y) a.y[(long)b * C + t] = y;
    }
    __syncthreads();
    const int C4 = C >> 2;
    const int p0 = blockIdx.x * a.ppb, np = min(a.HW, p0 + a.ppb) - p0;
    for (int i = t; i < np * C4; i += 256) {
        const int pix = i / C4, c = (i - pix * C4) * 4;
        const long px = (long)b * a.HW + p0 + pix;
        const float4 j = *reinterpret_cast<const float4*>(a.joi + px * a.joi_cs + c);
        const float4 y = *reinterpret_cast<const float4*>(s_y + c);
        float4 o = make_float4(j.x * y.x, j.y * y.y, j.z * y.z, j.w * y.w);
        if (a.x) {
            const float4 r = *reinterpret_cast<const float4*>(a.x + px * a.x_cs + c);
            o = make_float4(r.x + o.x, r.y + o.y, r.z + o.z, r.w + o.w);
        }
        *reinterpret_cast<float4*>(a.out + px * a.out_cs + c) = o;
    }
}

// NHWC class maps -> planes [B][nc][HW] (the layout launch_upsample_logits reads)
__global__ void cg_planes_kernel(const float* __restrict__ in, int cs, int nc, long HW, int B, float* __restrict__ q) {
    const long total = (long)B * nc * HW;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long p = i % HW, bc = i / HW;
        const int c = (int)(bc % nc);
        const long b = bc / nc;
        q[i] = in[(b * HW + p) * cs + c];
    }
}

// predictor.py:43-46: BGR channel i standardised with entry i of the RGB statistics in float64, depth channel 0 / 255; four pad zeros
__global__ void cg_preprocess_kernel(const uint8_t* __restrict__ bgr, const uint8_t* __restrict__ depth, long pixels, float* __restrict__ x) {
    const double mean[3] = {0.485, 0.456, 0.406}, sd[3] = {0.229, 0.224, 0.225};
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < pixels; i += (long)gridDim.x * blockDim.x) {
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (float)(((double)bgr[3 * i + c] / 255.0 - mean[c]) / sd[c]);
        float4* dst = reinterpret_cast<float4*>(x + i * 8);
        dst[0] = make_float4(v[0], v[1], v[2], (float)depth[3 * i] / 255.f);
        dst[1] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// eval/base_model.py:210-216 with the cv2.resize(fg, (W, H), INTER_NEAREST) of predictor.py:50 folded into the read:
// counts[b][k] = (|mask & fg'|, |mask|), fg'(y, x) = fg(floor(y ify), floor(x ifx)) with OpenCV's float64 factors ify = 1 / (H / fh),
// ifx = 1 / (W / fw), clipped to the map.  One workgroup per (row band, mask, frame); the two integer atomics per wave are exact in any order.
__global__ __launch_bounds__(256) void fg_overlap_kernel(const uint8_t* __restrict__ fg, int fh, int fw, const uint8_t* __restrict__ masks, int K, int H, int W,
                                                         int rows, double ify, double ifx, unsigned long long* __restrict__ counts) {
    const int k = blockIdx.y, b = blockIdx.z;
    const uint8_t* m = masks + ((long)b * K + k) * H * W;
    const uint8_t* f = fg + (long)b * fh * fw;
    const int r0 = blockIdx.x * rows, r1 = min(H, r0 + rows);
    unsigned inter = 0, area = 0;
    for (int y = r0; y < r1; ++y) {
        const int sy = min((int)floor(y * ify), fh - 1);
        for (int x = threadIdx.x; x < W; x += 256) {
            const bool on = m[(long)y * W + x] != 0;
            const int sx = min((int)floor(x * ifx), fw - 1);
            area += on;
            inter += on && f[(long)sy * fw + sx] != 0;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        inter += __shfl_down(inter, o);
        area += __shfl_down(area, o);
    }
    if ((threadIdx.x & 63) == 0 && area) {
        atomicAdd(&counts[((long)b * K + k) * 2], (unsigned long long)inter);
        atomicAdd(&counts[((long)b * K + k) * 2 + 1], (unsigned long long)area);
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int cg_joint_tiles(int H, int W) { return ((H + CG_TILE - 1) / CG_TILE) * ((W + CG_TILE - 1) / CG_TILE); }
int cg_sums_tiles(int H, int W) { return (int)(((long)H * W + CG_CHUNK - 1) / CG_CHUNK); }

int launch_cg_preprocess(const uint8_t* bgr, const uint8_t* depth, long pixels, float* x, hipStream_t st) {
    long g = (pixels + 255) / 256;
    g = g < 1 ? 1 : g > 4096 ? 4096 : g;
    hipLaunchKernelGGL(cg_preprocess_kernel, dim3((int)g), dim3(256), 0, st, bgr, depth, pixels, x);
    QB_CHECK(hipGetLastError());
    return 0;
}

static int cg_check_frame(const char* who, int B, int H, int W, int C) {
    if (C != 64 && C != 128) return fail(std::string(who) + ": expects 64 or 128 channels");
    if (B < 1 || B > 65535 || H < 1 || W < 1) return fail(std::string(who) + ": batch outside 1..65535 or an empty map");
    if ((long)B * H * W * C >= (1L << 31)) return fail(std::string(who) + ": tensor too large");
    return 0;
}

int launch_cg_joint(const View& x, const View& joi, int B, int dil, const float* w1, const float* s1, const float* h1, const float* a1, const float* wloc,
                    const float* wsur, const float* s2, const float* h2, const float* a2, double* partials, int tiles, hipStream_t st) {
    const int C = x.C;
    if (cg_check_frame("cg_joint", B, x.H, x.W, C)) return -1;
    if (joi.C != C || joi.H != x.H || joi.W != x.W) return fail("cg_joint: input and output geometry differ");
    if (dil < 1 || dil > CG_MAX_DIL) return fail("cg_joint: dilation outside 1..4");
    if (x.cs < C || x.cs % 4 || !aligned16(x.p) || !aligned16(w1)) return fail("cg_joint: the input and the 1x1 weights must come in aligned groups of 4 channels");
    if (joi.cs < C) return fail("cg_joint: output channel stride below the channel count");
    if ((long)B * x.H * x.W * std::max(x.cs, joi.cs) >= (1L << 31)) return fail("cg_joint: view too large");
    if (!x.p || !joi.p || !w1 || !s1 || !h1 || !a1 || !wloc || !wsur || !s2 || !h2 || !a2 || !partials) return fail("cg_joint: null argument");
    if (tiles != cg_joint_tiles(x.H, x.W)) return fail("cg_joint: the partials buffer is laid out for another tile count");
    CgJoint a{x.p, x.cs, joi.p, joi.cs, x.H, x.W, dil, (x.W + CG_TILE - 1) / CG_TILE, tiles, w1, s1, h1, a1, wloc, wsur, s2, h2, a2, partials};
    ProfScope prof("cg_joint", 4.0 * B * x.H * x.W * C * 2, 2.0 * B * x.H * x.W * (C / 2) * (C + 18), st);
    if (C == 128) hipLaunchKernelGGL(cg_joint_kernel<128>, dim3(tiles, B), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(cg_joint_kernel<64>, dim3(tiles, B), dim3(256), 0, st, a);
    QB_CHECK(hipGetLastError());
    return 0;
}

int launch_cg_sums(const View& in, int B, double* partials, int tiles, hipStream_t st) {
    if (cg_check_frame("cg_sums", B, in.H, in.W, in.C)) return -1;
    if (!in.p || !partials) return fail("cg_sums: null argument");
    if (in.cs < in.C || (long)B * in.H * in.W * in.cs >= (1L << 31)) return fail("cg_sums: bad channel stride or view too large");
    if (tiles != cg_sums_tiles(in.H, in.W)) return fail("cg_sums: the partials buffer is laid out for another tile count");
    ProfScope prof("cg_sums", 4.0 * B * in.H * in.W * in.C, 0.0, st);
    hipLaunchKernelGGL(cg_sums_kernel, dim3(tiles, B), dim3(256), 0, st, in.p, in.cs, in.C, in.H * in.W, tiles, partials);
    QB_CHECK(hipGetLastError());
    return 0;
}

int launch_cg_apply(const View& joi, const View* x, const View& out, int B, int hidden, const double* partials, int tiles, const float* fc0, const float* b0,
                    const float* fc2, const float* b2, float* mean, float* y, hipStream_t st) {
    const int C = joi.C;
    if (cg_check_frame("cg_apply", B, joi.H, joi.W, C)) return -1;
    if (hidden < 1 || hidden > 8) return fail("cg_apply: hidden units outside 1..8");
    if (tiles < 1 || !joi.p || !out.p || !partials || !fc0 || !b0 || !fc2 || !b2) return fail("cg_apply: null argument or no tiles");
    if (out.C != C || out.H != joi.H || out.W != joi.W || (x && (x->C != C || x->H != joi.H || x->W != joi.W || !x->p))) return fail("cg_apply: views of different geometry");
    auto ok = [C](const View& v) { return v.cs >= C && v.cs % 4 == 0 && aligned16(v.p); };
    if (!ok(joi) || !ok(out) || (x && !ok(*x))) return fail("cg_apply: channels must come in aligned groups of 4");
    const int HW = joi.H * joi.W;
    const int cs_max = std::max(std::max(joi.cs, out.cs), x ? x->cs : 0);
    if ((long)B * HW * cs_max >= (1L << 31)) return fail("cg_apply: view too large");
    // a workgroup re-reads the frame's partials: give it at least 1024 channel quads of work, at most 4096 workgroups per frame
    int ppb = (1024 * 4 + C - 1) / C;
    if ((HW + ppb - 1) / ppb > 4096) ppb = (HW + 4095) / 4096;
    CgApply a{joi.p, joi.cs, x ? x->p : nullptr, x ? x->cs : 0, out.p, out.cs, HW, C, hidden, tiles, ppb, partials, fc0, b0, fc2, b2, mean, y};
    ProfScope prof("cg_apply", 4.0 * B * HW * C * (x ? 3 : 2), 0.0, st);
    hipLaunchKernelGGL(cg_apply_kernel, dim3((HW + ppb - 1) / ppb, B), dim3(256), 0, st, a);
    QB_CHECK(hipGetLastError());
    return 0;
}

int launch_cg_planes(const View& in, int nc, int B, float* q, hipStream_t st) {
    const long HW = (long)in.H * in.W, total = HW * nc * B;
    long g = (total + 255) / 256;
    g = g < 1 ? 1 : g > 4096 ? 4096 : g;
    hipLaunchKernelGGL(cg_planes_kernel, dim3((int)g), dim3(256), 0, st, in.p, in.cs, nc, HW, B, q);
    QB_CHECK(hipGetLastError());
    return 0;
}

int launch_fg_overlap(const uint8_t* fg, int fh, int fw, const uint8_t* masks, int B, int K, int H, int W, unsigned long long* counts, hipStream_t st) {
    if (B < 1 || B > 65535 || K < 0 || K > 65535 || fh < 1 || fw < 1 || H < 1 || W < 1) return fail("foreground_overlap: batch or mask count outside 0..65535, or an empty map");
    if ((long)H * W >= (1L << 31) || (long)fh * fw >= (1L << 31)) return fail("foreground_overlap: frame too large");
    if (!counts || !fg || (K > 0 && !masks)) return fail("foreground_overlap: null argument");
    if (K == 0) return 0;
    if (int rc = launch_zero(counts, sizeof(unsigned long long) * 2 * B * K, st)) return rc;
    const int rows = 16;
    hipLaunchKernelGGL(fg_overlap_kernel, dim3((H + rows - 1) / rows, K, B), dim3(256), 0, st, fg, fh, fw, masks, K, H, W, rows, 1.0 / ((double)H / fh), 1.0 / ((double)W / fw),
                       counts);
    QB_CHECK(hipGetLastError());
    return 0;
}

}  // namespace quber
