// Kernels of the Region Refinement Network of UOIS-Net-3D (reference uois/src/segmentation.py:248-266 RegionRefinementNetwork,
// :329-423 rrn_preprocess / rrn_postprocess; uois/src/networks.py:191-278 UNet_Encoder / UNet_Decoder).  The dense layers, GroupNorm, max pool
// and bilinear upsampling of the network run on the launchers the project already has (plan_rrn.hip); here are its ends and the gather /
// scatter around it.  The definition is in INTEGRATION.md "Refined initial masks of the third family" and, as numpy, in
// tests/test_rrn_cpu.py: rrn_crop_np, rrn_paste_np.
//
//   rr_crop_kernel    rrn_preprocess without the host: per slot (frame, id) the frame's bytes under the id's ROI, standardised through a
//                     3 x 256 table and resized bilinearly (align_corners) to S x S planar f32, and `ids == id` by the nearest rule as 0 / 1.
//                     One block per (slot, output row).  The bilinear expression is float32 with every operation rounded on its own.
//   rr_pack_kernel    planar crops f32 [n][3][S][S] + mask u8 [n][S][S] -> NHWC with 8 channels (c0, c1, c2, mask != 0, four zeros).
//   rr_head_kernel    decoder.last_conv's output -> logit = fg_module . f (a chain of C fused multiply-adds) [-> refined = logit > threshold].
//   rr_head3_kernel   the same logit from decoder.layer5's output through the collapsed 3x3 filter w' = fg_module * last_conv: a workgroup
//                     owns a 16 x 16 tile, stages it with a one-pixel halo in LDS sixteen channels at a time (zeros outside the crop; the
//                     frame index is part of the address, so frames do not leak) and each lane runs the 9 C multiply-adds of its pixel.
//   rrn_postprocess:  key (per slot the float64 sum and the count of z under its mask resized back to the ROI, as block partials in
//                     row-major order) -> keyfin (partials added in block order, key = float32(sum / count)) -> order (one workgroup per
//                     frame: descending key, equal keys in slot order) -> gather (per frame pixel the LAST slot in paint order that covers
//                     it: deterministic, no scatter) -> compact (one workgroup per frame: surviving ids in ascending order, source, report)
//                     -> write (id map and the 0 / 255 planes).  No floating-point atomics; two runs give the same bits.
// No kernel waits for another workgroup.
#include "zoom_dev.h"

namespace quber {

namespace {

constexpr int RR_KEY_PIX = 2048;            // ROI pixels per block of the key pass: 256 lanes x 8 consecutive pixels
constexpr int RR_TILE = 16;                 // rr_head3: tile edge
constexpr int RR_CH = 16;                   // ... channels staged at a time
constexpr int RR_PS = 20;                   // ... floats between two staged pixels (16 + 4: consecutive pixels fall into different banks)

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline int grid1d(long items) {
    long g = (items + 255) / 256;
    return (int)(g < 1 ? 1 : g > 8192 ? 8192 : g);
}

// ---- crop -----------------------------------------------------------------------------------------------------------------------------
// F.upsample_bilinear (align_corners): source position of destination index `dst` for a resize from n to S samples
__device__ __forceinline__ void rr_axis(int dst, int n, int S, int& i0, int& i1, float& l0, float& l1) {
    const float sc = __fdiv_rn((float)(n - 1), (float)(S - 1));
    const float src = __fmul_rn((float)dst, sc);
    i0 = min((int)src, n - 1);
    i1 = min(i0 + 1, n - 1);
    l1 = __fsub_rn(src, (float)i0);
    l0 = __fsub_rn(1.f, l1);
}

// grid (S rows, T slots)
__global__ __launch_bounds__(ZM_T) void rr_crop_kernel(const uint8_t* __restrict__ img, const int* __restrict__ ids, const int* __restrict__ slots,
                                                       const int* __restrict__ rois, const float* __restrict__ table, int B, int n_ids, int H, int W,
                                                       int S, float* __restrict__ rgb_crop, uint8_t* __restrict__ mask_crop) {
    __shared__ float s_tab[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += ZM_T) s_tab[i] = table[i];
    __syncthreads();
    const int dy = blockIdx.x, t = blockIdx.y;
    const ZmSlot s = zm_slot(slots, rois, t, B, n_ids, H, W);
    int ya = 0, yb = 0, my = 0;
    float ly0 = 0.f, ly1 = 0.f;
    if (s.ok) {
        rr_axis(dy, s.h, S, ya, yb, ly0, ly1);
        my = zm_near(dy, s.h, S);
    }
    const size_t HW = (size_t)H * W, SS = (size_t)S * S;
    const size_t org = s.ok ? (size_t)s.b * HW + (size_t)s.y0 * W + s.x0 : 0;
    for (int dx = threadIdx.x; dx < S; dx += ZM_T) {
        float v[3] = {0.f, 0.f, 0.f};
        unsigned m = 0;
        if (s.ok) {
            int xa, xb;
            float lx0, lx1;
            rr_axis(dx, s.w, S, xa, xb, lx0, lx1);
            const uint8_t* pa = img + (org + (size_t)ya * W) * 3;
            const uint8_t* pb = img + (org + (size_t)yb * W) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float* tb = s_tab + c * 256;
                const float a = tb[pa[xa * 3 + c]], b = tb[pa[xb * 3 + c]], cc = tb[pb[xa * 3 + c]], d = tb[pb[xb * 3 + c]];
                const float top = __fadd_rn(__fmul_rn(lx0, a), __fmul_rn(lx1, b));
                const float bot = __fadd_rn(__fmul_rn(lx0, cc), __fmul_rn(lx1, d));
                v[c] = __fadd_rn(__fmul_rn(ly0, top), __fmul_rn(ly1, bot));
            }
            const int mx = zm_near(dx, s.w, S);
            m = ids[org + (size_t)my * W + mx] == s.id ? 1u : 0u;
        }
        const size_t o = (size_t)dy * S + dx;
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb_crop[((size_t)t * 3 + c) * SS + o] = v[c];
        mask_crop[(size_t)t * SS + o] = (uint8_t)m;
    }
}

// ---- pack -----------------------------------------------------------------------------------------------------------------------------
__global__ void rr_pack_kernel(const float* __restrict__ rgb, const uint8_t* __restrict__ mask, long HW, int B, float* __restrict__ x8) {
    const long total = (long)B * HW;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long b = i / HW, p = i - b * HW;
        const float* src = rgb + b * 3 * HW + p;
        float4* dst = reinterpret_cast<float4*>(x8 + i * 8);
        dst[0] = make_float4(src[0], src[HW], src[2 * HW], mask[i] ? 1.f : 0.f);
        dst[1] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// ---- heads ----------------------------------------------------------------------------------------------------------------------------
struct RrHeadP {
    const float* f; int f_cs, C;              // features NHWC
    const float* w;                           // head: [C]; head3: [9][C], tap-major
    float bias, thr;
    float* logits; uint8_t* refined;          // [B][H][W], either may be null
    int H, W, B;
};

__global__ __launch_bounds__(256) void rr_head_kernel(const RrHeadP a) {
    extern __shared__ float w[];              // [C]
    for (int i = threadIdx.x; i < a.C; i += blockDim.x) w[i] = a.w[i];
    __syncthreads();
    const long total = (long)a.B * a.H * a.W;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const float* src = a.f + i * a.f_cs;
        float o = 0.f;
        for (int c = 0; c < a.C; c += 4) {
            const float4 v = *reinterpret_cast<const float4*>(src + c);
            o = fmaf(v.x, w[c], o);
            o = fmaf(v.y, w[c + 1], o);
            o = fmaf(v.z, w[c + 2], o);
            o = fmaf(v.w, w[c + 3], o);
        }
        if (a.logits) a.logits[i] = o;
        if (a.refined) a.refined[i] = (uint8_t)(o > a.thr);
    }
}

// grid (ceil(W / 16), ceil(H / 16), B), 256 lanes: lane (ty, tx) owns pixel (16 by + ty, 16 bx + tx)
__global__ __launch_bounds__(256) void rr_head3_kernel(const RrHeadP a) {
    __shared__ float s_x[(RR_TILE + 2) * (RR_TILE + 2) * RR_PS];
    extern __shared__ float s_w[];            // [9][C]
    const int tid = threadIdx.x, tx = tid & (RR_TILE - 1), ty = tid >> 4;
    const int x0 = blockIdx.x * RR_TILE, y0 = blockIdx.y * RR_TILE, b = blockIdx.z;
    for (int i = tid; i < 9 * a.C; i += 256) s_w[i] = a.w[i];
    const long frame = (long)b * a.H * a.W;
    constexpr int E = RR_TILE + 2;
    float acc = a.bias;
    for (int c0 = 0; c0 < a.C; c0 += RR_CH) {
        const int q = min(RR_CH, a.C - c0) / 4;                 // quads of this chunk (C is a multiple of 4)
        __syncthreads();                                         // the previous chunk has been read (first round: the weights are in place)
        for (int i = tid; i < E * E * q; i += 256) {
            const int px = i / q, j = i - px * q;
            const int yy = y0 - 1 + px / E, xx = x0 - 1 + px % E;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((unsigned)yy < (unsigned)a.H && (unsigned)xx < (unsigned)a.W)
                v = *reinterpret_cast<const float4*>(a.f + (frame + (long)yy * a.W + xx) * a.f_cs + c0 + 4 * j);
            *reinterpret_cast<float4*>(s_x + px * RR_PS + 4 * j) = v;
        }
        __syncthreads();
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const float* xp = s_x + ((ty + tap / 3) * E + tx + tap % 3) * RR_PS;
            const float* wp = s_w + tap * a.C + c0;
            for (int j = 0; j < q; ++j) {
                const float4 v = *reinterpret_cast<const float4*>(xp + 4 * j);
                acc = fmaf(v.x, wp[4 * j], acc);
                acc = fmaf(v.y, wp[4 * j + 1], acc);
                acc = fmaf(v.z, wp[4 * j + 2], acc);
                acc = fmaf(v.w, wp[4 * j + 3], acc);
            }
        }
    }
    const int y = y0 + ty, x = x0 + tx;
    if (y < a.H && x < a.W) {
        const long i = frame + (long)y * a.W + x;
        if (a.logits) a.logits[i] = acc;
        if (a.refined) a.refined[i] = (uint8_t)(acc > a.thr);
    }
}

// ---- paste ----------------------------------------------------------------------------------------------------------------------------
// whether refined crop t covers pixel (y, x) of its slot's ROI (relative coordinates) under the nearest resize from S x S back to h x w
__device__ __forceinline__ bool rr_covers(const uint8_t* __restrict__ refined, int t, int S, const ZmSlot& s, int y, int x) {
    return refined[((size_t)t * S + zm_near(y, S, s.h)) * S + zm_near(x, S, s.w)] != 0;
}

// grid (nblk, T): block k of slot t takes ROI pixels [2048 k, 2048 (k + 1)) in row-major order, lane j the eight from 2048 k + 8 j on; the
// lanes' sums are added in lane order.  psum f64 [T][nblk], pcnt u32 [T][nblk]: every entry written
__global__ __launch_bounds__(ZM_T) void rr_key_kernel(const uint8_t* __restrict__ refined, const int* __restrict__ slots, const int* __restrict__ rois,
                                                      const float* __restrict__ z, int B, int n_ids, int H, int W, int S, int nblk,
                                                      double* __restrict__ psum, unsigned* __restrict__ pcnt) {
    __shared__ double s_sum[ZM_T];
    __shared__ unsigned s_cnt[ZM_T];
    const int t = blockIdx.y, j = threadIdx.x;
    const ZmSlot s = zm_slot(slots, rois, t, B, n_ids, H, W);
    double sum = 0.0;
    unsigned cnt = 0;
    if (s.ok) {
        const long area = (long)s.w * s.h;
        const float* zf = z + (size_t)s.b * H * W;
        const long p0 = (long)blockIdx.x * RR_KEY_PIX + (long)j * 8;
        for (int k = 0; k < 8; ++k) {
            const long p = p0 + k;
            if (p < area) {
                const int y = (int)(p / s.w), x = (int)(p - (long)y * s.w);
                if (rr_covers(refined, t, S, s, y, x)) {
                    const float v = zf[(size_t)(s.y0 + y) * W + s.x0 + x];
                    sum += v != v ? 0.0 : (double)v;
                    ++cnt;
                }
            }
        }
    }
    s_sum[j] = sum;
    s_cnt[j] = cnt;
    __syncthreads();
    if (j == 0) {
        double a = 0.0;
        unsigned n = 0;
        for (int i = 0; i < ZM_T; ++i) { a += s_sum[i]; n += s_cnt[i]; }
        psum[(size_t)t * nblk + blockIdx.x] = a;
        pcnt[(size_t)t * nblk + blockIdx.x] = n;
    }
}

// one lane per slot: cnt u32 [T], keys f32 [T] = float32(sum / count), 0 for a slot without a refined pixel or without a mean
__global__ __launch_bounds__(ZM_T) void rr_keyfin_kernel(const double* __restrict__ psum, const unsigned* __restrict__ pcnt, int T, int nblk,
                                                         unsigned* __restrict__ cnt, float* __restrict__ keys) {
    const int t = blockIdx.x * ZM_T + threadIdx.x;
    if (t >= T) return;
    double a = 0.0;
    unsigned n = 0;
    for (int k = 0; k < nblk; ++k) { a += psum[(size_t)t * nblk + k]; n += pcnt[(size_t)t * nblk + k]; }
    cnt[t] = n;
    const float k = n ? (float)(a / (double)n) : 0.f;
    keys[t] = k == k ? k : 0.f;                              // (+inf and -inf under one mask: no mean - the key reads 0 and the order stays total)
}

// grid (B), 256 lanes.  The slots of frame b are slots [start, start + n) (the list ascends by frame), n <= 254.  -> order i32 [B][254]
// (the slot painted r-th), ncrop i32 [B]; descending key, equal keys in slot order
__global__ __launch_bounds__(ZM_T) void rr_order_kernel(const int* __restrict__ slots, int T, const float* __restrict__ keys, int* __restrict__ order,
                                                        int* __restrict__ ncrop) {
    __shared__ int s_start, s_n;
    __shared__ float s_key[ZM_MAXID];
    const int j = threadIdx.x, b = blockIdx.x;
    if (j == 0) { s_start = 0; s_n = 0; }
    __syncthreads();
    int below = 0, mine = 0;
    for (int t = j; t < T; t += ZM_T) {
        const int f = slots[2 * t];
        below += f < b;
        mine += f == b;
    }
    if (below) atomicAdd(&s_start, below);
    if (mine) atomicAdd(&s_n, mine);
    __syncthreads();
    const int start = s_start, n = min(s_n, ZM_MAXID);
    if (j < n) s_key[j] = keys[min(start + j, T - 1)];
    __syncthreads();
    if (j < n) {
        const float ka = s_key[j];
        int rank = 0;
        for (int q = 0; q < n; ++q) {
            const float kq = s_key[q];
            rank += kq > ka || (kq == ka && q < j);
        }
        order[b * ZM_MAXID + rank] = min(start + j, T - 1);
    }
    if (j == 0) ncrop[b] = n;
}

// grid (ceil(HW / 256), B).  owner i32 [B][HW]: 0 or the initial id of the last slot in paint order that covers the pixel; vis i32
// [B][n_ids + 1], zero on entry: 1 for owners (every writer stores the same value); painted u32 [B], zero on entry
__global__ __launch_bounds__(ZM_T) void rr_gather_kernel(const uint8_t* __restrict__ refined, const int* __restrict__ slots, const int* __restrict__ rois,
                                                         const unsigned* __restrict__ cnt, const int* __restrict__ order, const int* __restrict__ ncrop,
                                                         int B, int n_ids, int H, int W, int S, int* __restrict__ owner, int* __restrict__ vis,
                                                         unsigned* __restrict__ painted) {
    __shared__ ZmSlot s_slot[ZM_MAXID];
    __shared__ int s_t[ZM_MAXID];
    __shared__ unsigned s_painted;
    const int j = threadIdx.x, b = blockIdx.y;
    const int n = ncrop[b];
    if (j == 0) s_painted = 0;
    if (j < n) {
        const int t = order[b * ZM_MAXID + j];
        ZmSlot s = zm_slot(slots, rois, t, B, n_ids, H, W);
        s.ok = s.ok && s.b == b && cnt[t] > 0;
        s_slot[j] = s;
        s_t[j] = t;
    }
    __syncthreads();
    const long HW = (long)H * W, p = (long)blockIdx.x * ZM_T + j;
    if (p < HW) {
        const int y = (int)(p / W), x = (int)(p - (long)y * W);
        int id = 0;
        for (int r = n - 1; r >= 0; --r) {
            const ZmSlot& s = s_slot[r];
            if (!s.ok || x < s.x0 || y < s.y0 || x >= s.x0 + s.w || y >= s.y0 + s.h) continue;
            if (rr_covers(refined, s_t[r], S, s, y - s.y0, x - s.x0)) { id = s.id; break; }
        }
        owner[(size_t)b * HW + p] = id;
        if (id) {
            vis[b * (n_ids + 1) + id] = 1;
            atomicAdd(&s_painted, 1u);
        }
    }
    __syncthreads();
    if (j == 0 && s_painted) atomicAdd(painted + b, s_painted);
}

// grid (B), 256 lanes: lut i32 [B][n_ids + 1] (initial id -> final id, ascending in the initial id), source i32 [B][N], report i32 [B][4]
__global__ __launch_bounds__(ZM_T) void rr_compact_kernel(const int* __restrict__ slots, const int* __restrict__ rois, const unsigned* __restrict__ cnt,
                                                          const int* __restrict__ order, const int* __restrict__ ncrop, const int* __restrict__ vis,
                                                          const unsigned* __restrict__ painted, int B, int n_ids, int N, int H, int W,
                                                          int* __restrict__ lut, int* __restrict__ source, int* __restrict__ report) {
    __shared__ int s_vis[ZM_MAXID + 1];
    __shared__ unsigned s_writes;
    __shared__ int s_gone;
    const int j = threadIdx.x, b = blockIdx.x;
    if (j == 0) { s_writes = 0; s_gone = 0; }
    for (int i = j; i <= n_ids; i += ZM_T) s_vis[i] = i ? vis[b * (n_ids + 1) + i] : 0;
    for (int k = j; k < N; k += ZM_T) source[b * N + k] = 0;
    __syncthreads();
    const int n = ncrop[b];
    if (j < n) {                                             // the frame's initial masks: pixels they painted, and whether they survive
        const int t = order[b * ZM_MAXID + j];
        const ZmSlot s = zm_slot(slots, rois, t, B, n_ids, H, W);
        if (s.ok && s.b == b) {
            if (cnt[t]) atomicAdd(&s_writes, cnt[t]);
            if (!s_vis[s.id]) atomicAdd(&s_gone, 1);
        }
    }
    int fin = 0;
    if (j >= 1 && j <= n_ids && s_vis[j]) {
        for (int i = 1; i <= j; ++i) fin += s_vis[i] != 0;
        if (fin <= N) source[b * N + fin - 1] = j;
    }
    if (j <= n_ids) lut[b * (n_ids + 1) + j] = fin;
    __syncthreads();
    if (j == 0) {
        int total = 0;
        for (int i = 1; i <= n_ids; ++i) total += s_vis[i] != 0;
        report[4 * b + 0] = total;
        report[4 * b + 1] = s_gone;
        report[4 * b + 2] = (int)painted[b];
        report[4 * b + 3] = (int)(s_writes - painted[b]);
    }
}

// grid (ceil(HW / 256), max(N, 1), B): plane k of the masks; the blocks of plane 0 write the id map as well
__global__ __launch_bounds__(ZM_T) void rr_write_kernel(const int* __restrict__ owner, const int* __restrict__ lut, int n_ids, int N, long HW,
                                                        int* __restrict__ out_ids, uint8_t* __restrict__ out_masks) {
    const int b = blockIdx.z, k = blockIdx.y;
    const long p = (long)blockIdx.x * ZM_T + threadIdx.x;
    if (p >= HW) return;
    const int fin = lut[b * (n_ids + 1) + owner[(size_t)b * HW + p]];
    if (k == 0) out_ids[(size_t)b * HW + p] = fin;
    if (k < N) out_masks[((size_t)b * N + k) * HW + p] = fin == k + 1 ? 255 : 0;
}

struct RrWs {
    double* psum; unsigned* pcnt; unsigned* cnt; int* order; int* ncrop; int* owner; int* lut;
    int* vis; unsigned* painted; size_t zero_bytes;          // vis | painted: one zero fill
    size_t bytes;
};
inline int rr_key_blocks(int H, int W) { return (int)(((long)H * W + RR_KEY_PIX - 1) / RR_KEY_PIX); }
RrWs rr_ws(void* base, int cap_b, int H, int W) {
    const size_t T = (size_t)cap_b * ZM_MAXID, nblk = rr_key_blocks(H, W), HW = (size_t)H * W;
    char* p = (char*)base;
    size_t o = 0;
    auto take = [&](size_t n) { char* q = p + o; o += (n + 15) / 16 * 16; return q; };
    RrWs w;
    w.psum = (double*)take(sizeof(double) * T * nblk);
    w.pcnt = (unsigned*)take(sizeof(unsigned) * T * nblk);
    w.cnt = (unsigned*)take(sizeof(unsigned) * T);
    w.order = (int*)take(sizeof(int) * cap_b * ZM_MAXID);
    w.ncrop = (int*)take(sizeof(int) * cap_b);
    w.owner = (int*)take(sizeof(int) * cap_b * HW);
    w.lut = (int*)take(sizeof(int) * cap_b * (ZM_MAXID + 1));
    const size_t z0 = o;
    w.vis = (int*)take(sizeof(int) * cap_b * (ZM_MAXID + 1));
    w.painted = (unsigned*)take(sizeof(unsigned) * cap_b);
    w.zero_bytes = o - z0;
    w.bytes = o;
    return w;
}

}  // namespace

size_t rrn_paste_ws_bytes(int cap_b, int H, int W) { return rr_ws(nullptr, cap_b, H, W).bytes; }

int launch_rrn_crop(const uint8_t* img, const int* ids, const int* slots, const int* rois, const float* table, int B, int n_ids, int T, int S, int H, int W,
                    float* rgb_crop, uint8_t* mask_crop, hipStream_t st) {
    if (!img || !ids || !slots || !rois || !table || !rgb_crop || !mask_crop) return fail("rrn_crop: null argument");
    if (B < 1 || n_ids < 0 || n_ids > ZM_MAXID || T < 1 || T > 65535 || S < 2 || S > 512 || H < 1 || W < 1) return fail("rrn_crop: argument out of range");
    if ((long)B * H * W * 3 >= (1L << 31)) return fail("rrn_crop: frames too large");
    ProfScope prof("rrn_crop", (double)T * S * S * (13.0 + 16.0), 0.0, st);
    hipLaunchKernelGGL(rr_crop_kernel, dim3(S, T), dim3(ZM_T), 0, st, img, ids, slots, rois, table, B, n_ids, H, W, S, rgb_crop, mask_crop);
    QB_CHECK(hipGetLastError());
    return 0;
}

int launch_rrn_pack(const float* rgb, const uint8_t* mask, int B, int H, int W, float* x8, hipStream_t st) {
    if (!rgb || !mask || !x8) return fail("rrn_pack: null argument");
    if (B < 1 || H < 1 || W < 1 || (long)B * H * W * 8 >= (1L << 31)) return fail("rrn_pack: empty or too large");
    if (!aligned16(x8)) return fail("rrn_pack: the packed output must be 16-byte aligned");
    ProfScope prof("rrn_pack", (double)B * H * W * (12 + 1 + 32), 0.0, st);
    hipLaunchKernelGGL(rr_pack_kernel, dim3(grid1d((long)B * H * W)), dim3(256), 0, st, rgb, mask, (long)H * W, B, x8);
    QB_CHECK(hipGetLastError());
    return 0;
}

static int rr_head_check(const char* who, const View& f, int B, const float* w, float* logits, uint8_t* refined) {
    const std::string n(who);
    if (!f.p || !w) return fail(n + ": null argument");
    if (!logits && !refined) return fail(n + ": neither logits nor refined mask requested");
    if (B < 1 || B > 65535 || f.H < 1 || f.W < 1 || f.C < 4 || f.C % 4 || f.C > 1024 || f.cs < f.C || f.cs % 4 || !aligned16(f.p))
        return fail(n + ": features in aligned groups of 4 channels, at most 1024; batch 1..65535");
    if ((long)B * f.H * f.W * f.cs >= (1L << 31)) return fail(n + ": view too large");
    return 0;
}

int launch_rrn_head(const View& f, int B, const float* wfg, float thr, float* logits, uint8_t* refined, hipStream_t st) {
    if (rr_head_check("rrn_head", f, B, wfg, logits, refined)) return -1;
    RrHeadP a{f.p, f.cs, f.C, wfg, 0.f, thr, logits, refined, f.H, f.W, B};
    ProfScope prof("rrn_head", (double)B * f.H * f.W * (4.0 * f.C + 5), 2.0 * B * f.H * f.W * f.C, st);
    hipLaunchKernelGGL(rr_head_kernel, dim3(grid1d((long)B * f.H * f.W)), dim3(256), sizeof(float) * f.C, st, a);
    QB_CHECK(hipGetLastError());
    return 0;
}

int launch_rrn_head3(const View& f, int B, const float* w9, float bias, float thr, float* logits, uint8_t* refined, hipStream_t st) {
    if (rr_head_check("rrn_head3", f, B, w9, logits, refined)) return -1;
    RrHeadP a{f.p, f.cs, f.C, w9, bias, thr, logits, refined, f.H, f.W, B};
    ProfScope prof("rrn_head3", (double)B * f.H * f.W * (4.0 * f.C + 5), 2.0 * B * f.H * f.W * 9.0 * f.C, st);
    const dim3 grid((f.W + RR_TILE - 1) / RR_TILE, (f.H + RR_TILE - 1) / RR_TILE, B);
    hipLaunchKernelGGL(rr_head3_kernel, grid, dim3(256), sizeof(float) * 9 * f.C, st, a);
    QB_CHECK(hipGetLastError());
    return 0;
}

int launch_rrn_paste(const uint8_t* refined, const int* slots, const int* rois, const float* z, int B, int n_ids, int T, int S, int N, int H, int W,
                     int* out_ids, uint8_t* out_masks, int* source, float* keys, int* report, void* ws, int cap_b, hipStream_t st) {
    if (B < 1 || B > cap_b || B > 65535 || n_ids < 0 || n_ids > ZM_MAXID || T < 0 || T > cap_b * ZM_MAXID || T > 65535 || S < 2 || S > 512 || N < 1 || N > ZM_MAXID)
        return fail("rrn_paste: argument out of range");
    if (!z || !out_ids || !out_masks || !source || !report || !ws || (T > 0 && (!refined || !slots || !rois || !keys))) return fail("rrn_paste: null argument");
    const RrWs w = rr_ws(ws, cap_b, H, W);
    const int nblk = rr_key_blocks(H, W);
    const long HW = (long)H * W;
    ProfScope prof("rrn_paste", (double)B * HW * (8.0 + N) + (double)T * S * S, 0.0, st);
    if (launch_zero(w.vis, w.zero_bytes, st)) return -1;
    if (T > 0) {
        hipLaunchKernelGGL(rr_key_kernel, dim3(nblk, T), dim3(ZM_T), 0, st, refined, slots, rois, z, B, n_ids, H, W, S, nblk, w.psum, w.pcnt);
        QB_CHECK(hipGetLastError());
        hipLaunchKernelGGL(rr_keyfin_kernel, dim3((T + ZM_T - 1) / ZM_T), dim3(ZM_T), 0, st, w.psum, w.pcnt, T, nblk, w.cnt, keys);
        QB_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(rr_order_kernel, dim3(B), dim3(ZM_T), 0, st, slots, T, keys, w.order, w.ncrop);
    QB_CHECK(hipGetLastError());
    hipLaunchKernelGGL(rr_gather_kernel, dim3((unsigned)((HW + ZM_T - 1) / ZM_T), B), dim3(ZM_T), 0, st, refined, slots, rois, w.cnt, w.order, w.ncrop, B,
                       n_ids, H, W, S, w.owner, w.vis, w.painted);
    QB_CHECK(hipGetLastError());
    hipLaunchKernelGGL(rr_compact_kernel, dim3(B), dim3(ZM_T), 0, st, slots, rois, w.cnt, w.order, w.ncrop, w.vis, w.painted, B, n_ids, N, H, W, w.lut,
                       source, report);
    QB_CHECK(hipGetLastError());
    hipLaunchKernelGGL(rr_write_kernel, dim3((unsigned)((HW + ZM_T - 1) / ZM_T), N, B), dim3(ZM_T), 0, st, w.owner, w.lut, n_ids, N, HW, out_ids, out_masks);
    QB_CHECK(hipGetLastError());
    return 0;
}

}  // namespace quber
