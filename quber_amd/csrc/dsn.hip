// Kernels of the Depth Seeding Network of UOIS-Net-3D (reference uois/src/networks.py: UNetESP_Encoder / UNetESP_Decoder,
// uois/src/segmentation.py:72-127, 207-243).  The dense layers, GroupNorm, max pool and bilinear upsampling of the network run on the
// launchers the project already has (plan_dsn.hip); here are its ends and the one block it is named for.
//
//   dsn_pack_kernel       planar f32 xyz [B][3][H][W] -> NHWC with 8 channels (x, y, z, five zeros) for the first 3x3 convolution and a cleaned
//                         planar copy for the head: NaN -> 0, then y negated when bit 0 of `flags` is set (eval/base_model.py:496-498).
//   An ESP module (networks.py:58-129) after its reduce convolution has produced t (n channels):
//                             combine = [d1 | d2 | d2 + d4 | (d2 + d4) + d8 | ((d2 + d4) + d8) + d16],  dK = 3x3 of t, dilation = padding = K
//                             out = [x +] combine, followed by GroupNorm(groups) + ReLU of out
//   esp_branches_kernel   one workgroup per (frame, 64 consecutive pixels), a wave per 16 of them.  The five convolutions run on
//                         v_mfma_f32_16x16x4_f32 (exact fp32: an fmaf chain over K), rows = the 16 pixels, columns = 16 output channels, K = the
//                         channels of t at one filter tap.  The pixel operand comes from global memory sixteen channels at a time (zeros outside
//                         the map: the padding is that of t), the filters from a packed copy in the lanes' operand order (esp_pack_kernel).
//                         The accumulators of d2 go on to take d4, d8 and d16: after each branch they ARE the running sum, which is stored
//                         [plus the module's input]; none of the five convolutions exists in memory.  A tap no pixel of the wave can reach
//                         (dilation 16 on the 1/16 map) is skipped.
//   esp_merge_kernel      the same running sums, residual and store from five tensors that separate convolution launches wrote (option key 53 = 0).
//   Both leave per-tile GroupNorm sums (sum, sum of squares per norm group, float64) of what they stored in partials[frame][tile][group][2];
//   esp_stats_kernel adds them in tile order into the [frame][group][2] layout launch_gn_apply reads: no atomics, two runs give the same bits.
//   dsn_head_kernel       the two 1x1 heads on the 64-channel full-resolution feature map, read once: logits, centre offsets,
//                         votes = cleaned xyz + offsets, class = first maximal logit, fg = (class == 2).
// No kernel waits for another workgroup.
#include "common.h"
#include <cmath>

namespace quber {

namespace {

constexpr int ESP_CHUNK = 64;         // pixels per tile: four waves of sixteen
constexpr int ESP_NT_MAX = 13;        // widest esp_branches_kernel instance: 208 channels of d1

typedef float f32x4 __attribute__((ext_vector_type(4)));

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline int grid1d(long items) {
    long g = (items + 255) / 256;
    return (int)(g < 1 ? 1 : g > 8192 ? 8192 : g);
}

__global__ void dsn_pack_kernel(const float* __restrict__ xyz, long HW, int B, int flags, float* __restrict__ x8, float* __restrict__ clean) {
    const long total = (long)B * HW;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long b = i / HW, p = i - b * HW;
        const float* src = xyz + b * 3 * HW + p;
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float q = src[c * HW];
            v[c] = q != q ? 0.f : q;
        }
        if (flags & 1) v[1] = -v[1];
        if (x8) {
            float4* dst = reinterpret_cast<float4*>(x8 + i * 8);
            dst[0] = make_float4(v[0], v[1], v[2], 0.f);
            dst[1] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (clean) {
            float* d = clean + b * 3 * HW + p;
#pragma unroll
            for (int c = 0; c < 3; ++c) d[c * HW] = v[c];
        }
    }
}

// depth -> organised point cloud, the contract of quber_amd/camera.py xyz_np: every operation of the two pinned expressions is one
// round-to-nearest intrinsic, so no contraction or reassociation can touch them
//   convention 0 "pinhole" (eval/base_model.py:489-495): float64, ((col - cx) / fx) * z and ((row - cy) / fy) * z, rounded to float32 once
//   convention 1 "uois" (compute_xyz): float32, ((col - cx) * z) / fx and (((H - 1 - row) - cy) * z) / fy, the camera rounded to float32 first
// raw (NaN kept), x8 and clean (dsn_pack_kernel's outputs: NaN -> 0 per component, then y negated with bit 0 of flags): any may be null
struct XyzCam { double fx, fy, cx, cy; };

template <int CONV>
__global__ void xyz_from_depth_kernel(const float* __restrict__ z, int H, int W, int B, int flags, const XyzCam cam, float* __restrict__ raw,
                                      float* __restrict__ x8, float* __restrict__ clean) {
    const long HW = (long)H * W, total = (long)B * HW;
    const float fxf = (float)cam.fx, fyf = (float)cam.fy, cxf = (float)cam.cx, cyf = (float)cam.cy;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long b = i / HW, p = i - b * HW;
        const int row = (int)(p / W), col = (int)(p - (long)row * W);
        const float zz = z[i];
        float v[3];
        if (CONV == 0) {
            const double zd = (double)zz;
            v[0] = __double2float_rn(__dmul_rn(__ddiv_rn(__dsub_rn((double)col, cam.cx), cam.fx), zd));
            v[1] = __double2float_rn(__dmul_rn(__ddiv_rn(__dsub_rn((double)row, cam.cy), cam.fy), zd));
        } else {
            v[0] = __fdiv_rn(__fmul_rn(__fsub_rn((float)col, cxf), zz), fxf);
            v[1] = __fdiv_rn(__fmul_rn(__fsub_rn((float)(H - 1 - row), cyf), zz), fyf);
        }
        v[2] = zz;
        const long base = b * 3 * HW + p;
        if (raw) {
#pragma unroll
            for (int c = 0; c < 3; ++c) raw[base + c * HW] = v[c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = v[c] != v[c] ? 0.f : v[c];
        if (flags & 1) v[1] = -v[1];
        if (x8) {
            float4* dst = reinterpret_cast<float4*>(x8 + i * 8);
            dst[0] = make_float4(v[0], v[1], v[2], 0.f);
            dst[1] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (clean) {
#pragma unroll
            for (int c = 0; c < 3; ++c) clean[base + c * HW] = v[c];
        }
    }
}

// filters of the five branches, OIHW [n1 | n][n][3][3] -> [branch][tap][nt][j][lane][4]: lane (col = lane & 15, g = lane >> 4) finds
// W[out = 16 nt + col][cin = 16 j + 4 g + e][tap], e = 0..3, as one 16-byte load; zeros beyond the real channels
__global__ void esp_pack_kernel(const float* __restrict__ w1, const float* __restrict__ w2, const float* __restrict__ w4, const float* __restrict__ w8,
                                const float* __restrict__ w16, int n, int n1, int NT, float* __restrict__ packed) {
    const long total = 5L * 9 * NT * NT * 256;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        long r = i;
        const int e = (int)(r & 3); r >>= 2;
        const int lane = (int)(r & 63); r >>= 6;
        const int j = (int)(r % NT); r /= NT;
        const int nt = (int)(r % NT); r /= NT;
        const int tap = (int)(r % 9);
        const int br = (int)(r / 9);
        const float* w = br == 0 ? w1 : br == 1 ? w2 : br == 2 ? w4 : br == 3 ? w8 : w16;
        const int o = 16 * nt + (lane & 15), ci = 16 * j + 4 * (lane >> 4) + e;
        const int no = br == 0 ? n1 : n;
        packed[i] = (o < no && ci < n) ? w[((long)o * n + ci) * 9 + tap] : 0.f;
    }
}

struct EspP {
    const float* t; int t_cs;                 // reduce output, n channels (fused form)
    const float* d[5]; int d_cs[5];           // the five convolutions (merge form)
    const float* x; int x_cs;                 // the module's input or null
    float* out; int out_cs;
    int H, W, HW, n, n1, C, groups, tiles;
    const float* wp;                          // packed filters (fused form)
    double* partials;                         // [B][tiles][groups][2]
};

// the tile's channel sums in LDS (red[C][2]) -> norm-group sums of the tile
__device__ __forceinline__ void esp_group_sums(const EspP& a, const double* red, int b, int tile) {
    const int t = threadIdx.x;
    if (t < a.groups) {
        const int cpg = a.C / a.groups;
        double s = 0.0, ss = 0.0;
        for (int k = 0; k < cpg; ++k) {
            s += red[2 * (t * cpg + k)];
            ss += red[2 * (t * cpg + k) + 1];
        }
        double* dst = a.partials + (((long)b * a.tiles + tile) * a.groups + t) * 2;
        dst[0] = s;
        dst[1] = ss;
    }
}

template <int NT>
__global__ __launch_bounds__(256) void esp_branches_kernel(const EspP a) {
    __shared__ double red[1024 * 2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y, tile = blockIdx.x;
    const int col = lane & 15, g = lane >> 4;
    const int p0 = tile * ESP_CHUNK + wave * 16;
    const long frame = (long)b * a.HW;
    // A operand: this lane's pixel
    const int pa = p0 + col;
    const bool va = pa < a.HW;
    const int ya = va ? pa / a.W : 0, xa = va ? pa - ya * a.W : 0;
    f32x4 acc[NT];
    for (int br = 0; br < 5; ++br) {
        const int dil = 1 << br;
        if (br < 2) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap - ky * 3;
            const int yy = ya + (ky - 1) * dil, xx = xa + (kx - 1) * dil;
            const bool ok = va && (unsigned)yy < (unsigned)a.H && (unsigned)xx < (unsigned)a.W;
            if (!__any(ok)) continue;                           // wave-uniform: the tap lies in the padding for all sixteen pixels
            f32x4 av[NT];
            const float* src = a.t + (frame + (long)yy * a.W + xx) * a.t_cs + 4 * g;
#pragma unroll
            for (int j = 0; j < NT; ++j) av[j] = ok ? *reinterpret_cast<const f32x4*>(src + 16 * j) : f32x4{0.f, 0.f, 0.f, 0.f};
            const f32x4* wq = reinterpret_cast<const f32x4*>(a.wp) + (long)(br * 9 + tap) * NT * NT * 64 + lane;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const f32x4 wv = wq[(nt * NT + j) * 64];
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j][e], wv[e], acc[nt], 0, 0, 0);
                }
            }
        }
        // D[4 g + r][col]: pixel p0 + 4 g + r, channel 16 nt + col of this branch's slot
        const int cnt = br == 0 ? a.n1 : a.n, off = br == 0 ? 0 : a.n1 + (br - 1) * a.n;
        double s[NT], ss[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            s[nt] = 0.0; ss[nt] = 0.0;
            const int ch = 16 * nt + col;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = p0 + 4 * g + r;
                if (q < a.HW && ch < cnt) {
                    float v = acc[nt][r];
                    if (a.x) v = a.x[(frame + q) * a.x_cs + off + ch] + v;
                    a.out[(frame + q) * a.out_cs + off + ch] = v;
                    s[nt] += (double)v;
                    ss[nt] += (double)v * (double)v;
                }
            }
            s[nt] += __shfl_xor(s[nt], 16); ss[nt] += __shfl_xor(ss[nt], 16);
            s[nt] += __shfl_xor(s[nt], 32); ss[nt] += __shfl_xor(ss[nt], 32);
        }
        for (int w = 0; w < 4; ++w) {                            // the four waves in order: the same sum every run
            if (wave == w && g == 0) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const int ch = 16 * nt + col;
                    if (ch < cnt) {
                        double* dst = red + 2 * (off + ch);
                        if (w == 0) { dst[0] = s[nt]; dst[1] = ss[nt]; }
                        else { dst[0] += s[nt]; dst[1] += ss[nt]; }
                    }
                }
            }
            __syncthreads();
        }
    }
    esp_group_sums(a, red, b, tile);
}

__global__ __launch_bounds__(256) void esp_merge_kernel(const EspP a) {
    __shared__ double red[1024 * 2];
    const int t = threadIdx.x, b = blockIdx.y, tile = blockIdx.x;
    const long frame = (long)b * a.HW;
    const int p0 = tile * ESP_CHUNK, p1 = min(a.HW, p0 + ESP_CHUNK);
    for (int c = t; c < a.C; c += 256) {
        const int k = c < a.n1 ? -1 : (c - a.n1) / a.n;          // -1: d1; 0..3: sums of 1..4 convolutions
        const int j = c < a.n1 ? c : (c - a.n1) - k * a.n;
        double s = 0.0, ss = 0.0;
        for (int p = p0; p < p1; ++p) {
            const long px = frame + p;
            float v;
            if (k < 0) v = a.d[0][px * a.d_cs[0] + j];
            else {
                v = a.d[1][px * a.d_cs[1] + j];
                for (int i = 1; i <= k; ++i) v = v + a.d[1 + i][px * a.d_cs[1 + i] + j];
            }
            if (a.x) v = a.x[px * a.x_cs + c] + v;
            a.out[px * a.out_cs + c] = v;
            s += (double)v;
            ss += (double)v * (double)v;
        }
        red[2 * c] = s;
        red[2 * c + 1] = ss;
    }
    __syncthreads();
    esp_group_sums(a, red, b, tile);
}

// partials [B][tiles][groups][2] -> stats [B][groups][2], added in tile order
__global__ void esp_stats_kernel(const double* __restrict__ partials, int tiles, int G2, double* __restrict__ stats) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (t >= G2) return;
    const double* p = partials + (long)b * tiles * G2 + t;
    double s = 0.0;
    for (int i = 0; i < tiles; ++i) s += p[(long)i * G2];
    stats[(long)b * G2 + t] = s;
}

struct HeadP {
    const float* f; int f_cs, C;              // features NHWC
    const float* clean;                       // cleaned xyz, planar, or null
    const float *wfg, *wcd;                   // [3][C] each
    float *logits, *offsets, *votes;          // planar [B][3][HW], any may be null
    uint8_t *classes, *fg;                    // [B][HW], any may be null
    long HW; int B;
};

__global__ __launch_bounds__(256) void dsn_head_kernel(const HeadP a) {
    extern __shared__ float w[];              // [6][C]
    for (int i = threadIdx.x; i < 6 * a.C; i += blockDim.x) w[i] = i < 3 * a.C ? a.wfg[i] : a.wcd[i - 3 * a.C];
    __syncthreads();
    const long total = (long)a.B * a.HW;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long b = i / a.HW, p = i - b * a.HW;
        const float* src = a.f + i * a.f_cs;
        float o[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < a.C; c += 4) {
            const float4 v = *reinterpret_cast<const float4*>(src + c);
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const float* wk = w + k * a.C + c;
                o[k] = fmaf(v.x, wk[0], o[k]);
                o[k] = fmaf(v.y, wk[1], o[k]);
                o[k] = fmaf(v.z, wk[2], o[k]);
                o[k] = fmaf(v.w, wk[3], o[k]);
            }
        }
        const long base = b * 3 * a.HW + p;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (a.logits) a.logits[base + k * a.HW] = o[k];
            if (a.offsets) a.offsets[base + k * a.HW] = o[3 + k];
            if (a.votes) a.votes[base + k * a.HW] = a.clean[base + k * a.HW] + o[3 + k];
        }
        int cls = 0;                                             // the first maximal logit
        if (o[1] > o[cls]) cls = 1;
        if (o[2] > o[cls]) cls = 2;
        if (a.classes) a.classes[i] = (uint8_t)cls;
        if (a.fg) a.fg[i] = (uint8_t)(cls == 2);
    }
}

int esp_check(const char* who, const View& x, const View& out, bool has_x, int B, int n, int n1, int groups, double* partials, int tiles) {
    const std::string w(who);
    const int C = out.C;
    if (B < 1 || B > 65535 || out.H < 1 || out.W < 1) return fail(w + ": batch outside 1..65535 or an empty map");
    if (n < 1 || n1 < n || n1 + 4 * n != C || C > 1024) return fail(w + ": channels must split as n1 + 4 n with n1 >= n >= 1, at most 1024");
    if (groups < 1 || groups > 64 || C % groups) return fail(w + ": 1..64 norm groups that divide the channels");
    if (!out.p || !partials || (has_x && !x.p)) return fail(w + ": null argument");
    if (out.cs < C || (has_x && (x.cs < C || x.C != C || x.H != out.H || x.W != out.W))) return fail(w + ": views of different geometry or a channel stride below the channel count");
    if ((long)B * out.H * out.W * std::max(out.cs, has_x ? x.cs : 0) >= (1L << 31)) return fail(w + ": view too large");
    if (tiles != esp_tiles(out.H, out.W)) return fail(w + ": the partials buffer is laid out for another tile count");
    return 0;
}

}  // namespace

int esp_tiles(int H, int W) { return (int)(((long)H * W + ESP_CHUNK - 1) / ESP_CHUNK); }
int esp_nt(int n1) { return (n1 + 15) / 16; }
// the NT of the esp_branches_kernel<NT> instance that takes n1 channels (launch_esp_branches dispatches on 1..13), 0 where there is none
int esp_kernel(int n1) { return (n1 < 1 || n1 > 16 * ESP_NT_MAX) ? 0 : esp_nt(n1); }
size_t esp_packed_floats(int n1) { return (size_t)5 * 9 * esp_nt(n1) * esp_nt(n1) * 256; }

int launch_dsn_pack(const float* xyz, int B, int H, int W, int flags, float* x8, float* clean, hipStream_t st) {
    if (!xyz || (!x8 && !clean)) return fail("dsn_pack: null argument");
    if (B < 1 || H < 1 || W < 1 || (long)B * H * W * 8 >= (1L << 31)) return fail("dsn_pack: empty or too large");
    if (x8 && !aligned16(x8)) return fail("dsn_pack: the packed output must be 16-byte aligned");
    ProfScope prof("dsn_pack", 4.0 * B * H * W * (3 + 8 + 3), 0.0, st);
    hipLaunchKernelGGL(dsn_pack_kernel, dim3(grid1d((long)B * H * W)), dim3(256), 0, st, xyz, (long)H * W, B, flags, x8, clean);
    QB_CHECK(hipGetLastError());
    return 0;
}

int launch_xyz_from_depth(const float* z, int B, int H, int W, const double cam[4], int convention, int flags, float* raw, float* x8, float* clean, hipStream_t st) {
    if (!z || !cam || (!raw && !x8 && !clean)) return fail("xyz_from_depth: null argument");
    if (B < 1 || H < 1 || W < 1 || (long)B * H * W * 8 >= (1L << 31)) return fail("xyz_from_depth: empty or too large");
    if (convention != 0 && convention != 1) return fail("xyz_from_depth: convention 0 (pinhole, float64) or 1 (uois, float32)");
    if (flags & ~1) return fail("xyz_from_depth: unknown flag bits");
    if (x8 && !aligned16(x8)) return fail("xyz_from_depth: the packed output must be 16-byte aligned");
    for (int i = 0; i < 4; ++i)
        if (!std::isfinite(cam[i])) return fail("xyz_from_depth: the camera (fx, fy, cx, cy) must be finite");
    if (cam[0] == 0.0 || cam[1] == 0.0) return fail("xyz_from_depth: a focal length of zero");
    const XyzCam c{cam[0], cam[1], cam[2], cam[3]};
    ProfScope prof("xyz_from_depth", 4.0 * B * H * W * (1 + (raw ? 3 : 0) + (x8 ? 8 : 0) + (clean ? 3 : 0)), 0.0, st);
    const dim3 grid(grid1d((long)B * H * W));
    if (convention == 0) hipLaunchKernelGGL(xyz_from_depth_kernel<0>, grid, dim3(256), 0, st, z, H, W, B, flags, c, raw, x8, clean);
    else hipLaunchKernelGGL(xyz_from_depth_kernel<1>, grid, dim3(256), 0, st, z, H, W, B, flags, c, raw, x8, clean);
    QB_CHECK(hipGetLastError());
    return 0;
}

int launch_esp_pack(const float* const w[5], int n, int n1, float* packed, hipStream_t st) {
    if (n < 1 || n1 < n || !esp_kernel(n1)) return fail("esp_pack: n1 >= n >= 1, n1 at most 208");
    if (!packed || !aligned16(packed)) return fail("esp_pack: null or unaligned destination");
    for (int i = 0; i < 5; ++i)
        if (!w[i]) return fail("esp_pack: null filter");
    hipLaunchKernelGGL(esp_pack_kernel, dim3(grid1d((long)esp_packed_floats(n1))), dim3(256), 0, st, w[0], w[1], w[2], w[3], w[4], n, n1, esp_nt(n1), packed);
    QB_CHECK(hipGetLastError());
    return 0;
}

int launch_esp_branches(const View& t, const View* x, const View& out, int B, int n, int n1, int groups, const float* packed, double* partials, int tiles, hipStream_t st) {
    if (esp_check("esp_branches", x ? *x : View(), out, x != nullptr, B, n, n1, groups, partials, tiles)) return -1;
    const int NT = esp_kernel(n1);
    if (!NT) return fail("esp_branches: no kernel for this channel count (n1 in 1..208)");
    if (!t.p || !packed || t.H != out.H || t.W != out.W) return fail("esp_branches: null argument or views of different geometry");
    if (t.cs < 16 * NT || t.cs % 4 || !aligned16(t.p) || !aligned16(packed)) return fail("esp_branches: t needs a channel stride of at least 16 ceil(n1 / 16), in aligned groups of 4");
    if ((long)B * t.H * t.W * t.cs >= (1L << 31)) return fail("esp_branches: view too large");
    EspP a{};
    a.t = t.p; a.t_cs = t.cs; a.x = x ? x->p : nullptr; a.x_cs = x ? x->cs : 0; a.out = out.p; a.out_cs = out.cs;
    a.H = out.H; a.W = out.W; a.HW = out.H * out.W; a.n = n; a.n1 = n1; a.C = out.C; a.groups = groups; a.tiles = tiles; a.wp = packed; a.partials = partials;
    ProfScope prof("esp_branches", 4.0 * B * a.HW * (n + (x ? 2 : 1) * out.C), 2.0 * B * a.HW * 9.0 * n * (n1 + 4 * n), st);
    const dim3 grid(tiles, B);
#define ESP_CASE(N) case N: hipLaunchKernelGGL(esp_branches_kernel<N>, grid, dim3(256), 0, st, a); break;
    switch (NT) {                              // every instance esp_kernel names
        ESP_CASE(1) ESP_CASE(2) ESP_CASE(3) ESP_CASE(4) ESP_CASE(5) ESP_CASE(6) ESP_CASE(7) ESP_CASE(8) ESP_CASE(9) ESP_CASE(10) ESP_CASE(11) ESP_CASE(12) ESP_CASE(13)
        default: return fail("esp_branches: no kernel for this channel count (n1 in 1..208)");
    }
#undef ESP_CASE
    QB_CHECK(hipGetLastError());
    return 0;
}

int launch_esp_merge(const View d[5], const View* x, const View& out, int B, int n, int n1, int groups, double* partials, int tiles, hipStream_t st) {
    if (esp_check("esp_merge", x ? *x : View(), out, x != nullptr, B, n, n1, groups, partials, tiles)) return -1;
    EspP a{};
    long cs_max = 0;
    for (int i = 0; i < 5; ++i) {
        const int c = i == 0 ? n1 : n;
        if (!d[i].p || d[i].cs < c || d[i].H != out.H || d[i].W != out.W) return fail("esp_merge: null branch, a channel stride below the channel count or another geometry");
        a.d[i] = d[i].p; a.d_cs[i] = d[i].cs;
        cs_max = std::max<long>(cs_max, d[i].cs);
    }
    if ((long)B * out.H * out.W * cs_max >= (1L << 31)) return fail("esp_merge: view too large");
    a.x = x ? x->p : nullptr; a.x_cs = x ? x->cs : 0; a.out = out.p; a.out_cs = out.cs;
    a.H = out.H; a.W = out.W; a.HW = out.H * out.W; a.n = n; a.n1 = n1; a.C = out.C; a.groups = groups; a.tiles = tiles; a.partials = partials;
    ProfScope prof("esp_merge", 4.0 * B * a.HW * out.C * (x ? 4.0 : 3.0), 0.0, st);
    hipLaunchKernelGGL(esp_merge_kernel, dim3(tiles, B), dim3(256), 0, st, a);
    QB_CHECK(hipGetLastError());
    return 0;
}

int launch_esp_stats(const double* partials, int B, int tiles, int groups, double* stats, hipStream_t st) {
    if (!partials || !stats || B < 1 || tiles < 1 || groups < 1 || groups > 64) return fail("esp_stats: null argument, no tiles or more than 64 groups");
    hipLaunchKernelGGL(esp_stats_kernel, dim3(B), dim3(128), 0, st, partials, tiles, 2 * groups, stats);
    QB_CHECK(hipGetLastError());
    return 0;
}

int launch_dsn_head(const View& f, int B, const float* clean, const float* wfg, const float* wcd, float* logits, float* offsets, float* votes, uint8_t* classes,
                    uint8_t* fg, hipStream_t st) {
    if (!f.p || !wfg || !wcd) return fail("dsn_head: null argument");
    if (votes && !clean) return fail("dsn_head: votes need the cleaned xyz");
    if (B < 1 || f.H < 1 || f.W < 1 || f.C < 4 || f.C % 4 || f.C > 1024 || f.cs < f.C || f.cs % 4 || !aligned16(f.p)) return fail("dsn_head: features in aligned groups of 4 channels, at most 1024");
    if ((long)B * f.H * f.W * f.cs >= (1L << 31)) return fail("dsn_head: view too large");
    HeadP a{f.p, f.cs, f.C, clean, wfg, wcd, logits, offsets, votes, classes, fg, (long)f.H * f.W, B};
    ProfScope prof("dsn_head", (double)B * f.H * f.W * (4.0 * f.C + 4.0 * 12 + 2), 2.0 * B * f.H * f.W * 6.0 * f.C, st);
    hipLaunchKernelGGL(dsn_head_kernel, dim3(grid1d((long)B * f.H * f.W)), dim3(256), sizeof(float) * 6 * f.C, st, a);
    QB_CHECK(hipGetLastError());
    return 0;
}

}  // namespace quber
