// Mean-shift clustering of a pixel-embedding map into initial masks on the device (include/quber_hip.h: quber_meanshift_*; the
// definition is in INTEGRATION.md "Initial masks from pixel embeddings" and, as numpy, in tests/test_meanshift_cpu.py: meanshift_np,
// filter_depth_np).  Restates the UCN base model's clustering_features -> mean_shift_smart_init (select_smart_seeds,
// seed_hill_climbing_ball, connected_components) and filter_labels_depth of the reference (eval/base_model.py:622-840, :34-47), cosine
// metric, on X = f32 [B][64][n], n = H W: the layout the UCN network emits, so that a pixel's channels are n floats apart and every
// kernel below reads consecutive pixels in consecutive lanes.
//
// Stream-ordered steps, no host copy, no memset node, no grid-wide barrier:
//   seeds   one launch per seed: dist[p] = 0.5 (1 - dot(X[p], X[j])) against the seed j the previous launch published, the running
//           minimum per pixel, (value, index) reduced per block and published with ONE 64-bit atomicMax per block: the key orders floats
//           of either sign and, among equal values, prefers the lowest index (torch.argmax).  The slots are cleared by launch_zero.
//   climb   iters x (ms_climb_kernel, ms_mode_kernel).  A persistent block of four waves walks tiles of MS_TP pixels; wave w owns seeds
//           32 w .. 32 w + 31.  Per 32 pixels of a tile: S^T = X Z^T by 32 v_mfma_f32_32x32x2_f32 (K = 64 channels), W = exp(kappa S^T)
//           on the 16 accumulator registers, acc += W^T X by 2 x 16 MFMAs whose K index runs over the 32 pixels IN THE ORDER THE
//           ACCUMULATOR LAYOUT HOLDS THEM (lane half h, register r <-> pixel (r & 3) + 8 (r >> 2) + 4 h: A and B only have to agree on
//           it), so W never leaves the registers and the S x n weight matrix never exists.  The 128 x 64 accumulator (2 x 16 registers
//           per lane) lives through the block's whole walk.  Block partials go to the workspace; ms_mode_kernel adds them in block order
//           in float64 and normalises: no floating-point atomics, two runs are bit-equal.  Padded seed rows (>= S) are computed on
//           zeros by a wave that also owns real seeds, skipped by a wave that owns none, and never stored.
//   link    one workgroup per frame: S x S distances <= epsilon as bit rows in LDS, then the reference's sequential labelling by one
//           thread (bounded loops, every thread reaches every barrier).
//   assign  per pixel the first index of the minimum distance over the climbed seeds -> raw label; label histogram (and, with a depth
//           plane, the histogram of pixels with z > 0) through LDS into integer tables.
//   finish  one block per frame: the largest of the labels 0 .. num - 1 swaps with 0, the depth filter (__fdiv_rn), compaction by
//           counting -> raw label -> output id; then one pass writes the id map and all N planes.
// Every dot product that decides something is accumulated in float32 in channel order with __fmul_rn / __fadd_rn (the contract's
// pinned dot).  Every output is overwritten by every call.
#include "common.h"
#include <algorithm>
#include <initializer_list>

namespace quber {

constexpr int MS_C = 64;                     // embedding channels
constexpr int MS_SMAX = 128;                 // seeds per frame: four row tiles of the 32x32 MFMA
constexpr int MS_TP = 64;                    // pixels of a climb tile
constexpr int MS_PITCH = MS_TP + 1;          // LDS row pitch of a tile (floats): odd, the 32 channels a wave half reads lie in 32 banks
constexpr int MS_G = 256;                    // climb blocks per frame at most (independent of the batch: a frame's modes are too)
constexpr int MS_NMAX = 254;                 // output planes at most
constexpr float MS_KAPPA_MAX = 64.f;         // exp(64) = 6.2e27 summed over 2^24 pixels stays below float32's 3.4e38 in the accumulator
using f32x16 = __attribute__((ext_vector_type(16))) float;

// a float as an unsigned that orders like the float (negative values included), above the index complement: max = largest value, lowest index
__device__ __forceinline__ unsigned long long ms_key(float v, unsigned p) {
    unsigned u = __float_as_uint(v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | (0xffffffffu - p);
}

__device__ __forceinline__ float ms_dist(float dot) { return __fmul_rn(0.5f, __fsub_rn(1.f, dot)); }

// grid (ceil(n / 256), B).  Step k of S: slots u64 [B][S], slot k holds the key of the k-th seed (k >= 1; zero on entry of step 0).
__global__ __launch_bounds__(256) void ms_seed_kernel(const float* __restrict__ X, const int* __restrict__ first, unsigned long long* __restrict__ slots,
                                                      float* __restrict__ mind, int* __restrict__ idx, int n, int S, int k) {
    __shared__ float s_x[MS_C];
    __shared__ unsigned long long s_best[4];
    const int t = threadIdx.x, b = blockIdx.y;
    const float* Xb = X + (size_t)b * MS_C * n;
    int j = k == 0 ? first[b] : (int)(0xffffffffu - (unsigned)(slots[(size_t)b * S + k] & 0xffffffffull));
    j = min(max(j, 0), n - 1);
    if (t < MS_C) s_x[t] = Xb[(size_t)t * n + j];
    if (blockIdx.x == 0 && t == 0) idx[(size_t)b * S + k] = j;
    __syncthreads();
    const int p = blockIdx.x * 256 + t;
    unsigned long long key = 0;
    if (p < n) {
        float acc = 0.f;
#pragma unroll 16
        for (int c = 0; c < MS_C; ++c) acc = __fadd_rn(acc, __fmul_rn(Xb[(size_t)c * n + p], s_x[c]));
        float d = ms_dist(acc);
        if (k > 0) d = fminf(mind[(size_t)b * n + p], d);
        mind[(size_t)b * n + p] = d;
        key = ms_key(d, (unsigned)p);
    }
    if (k + 1 >= S) return;                                  // (uniform) the last seed has no successor
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o, 64);
        key = other > key ? other : key;
    }
    if ((t & 63) == 0) s_best[t >> 6] = key;
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < 4; ++w) key = s_best[w] > key ? s_best[w] : key;
        atomicMax(slots + (size_t)b * S + k + 1, key);
    }
}

// grid (S, B), 64 lanes: Z[b][s][c] = X[b][c][idx[b][s]]
__global__ __launch_bounds__(64) void ms_gather_kernel(const float* __restrict__ X, const int* __restrict__ idx, float* __restrict__ Z, int n, int S) {
    const int s = blockIdx.x, b = blockIdx.y, c = threadIdx.x;
    const int j = min(max(idx[(size_t)b * S + s], 0), n - 1);
    Z[((size_t)b * S + s) * MS_C + c] = X[((size_t)b * MS_C + c) * n + j];
}

// grid (G <= min(ntiles, MS_G), B), 256 lanes.  part f32 [B][G][MS_SMAX][64]: rows < S of the waves that own a real seed are written.
__global__ __launch_bounds__(256) void ms_climb_kernel(const float* __restrict__ X, const float* __restrict__ Z, float* __restrict__ part, int n, int S,
                                                       int ntiles, float kappa) {
    __shared__ float s_x[MS_C * MS_PITCH];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, half = lane >> 5, col = lane & 31;
    const int b = blockIdx.y, G = gridDim.x;
    const float* Xb = X + (size_t)b * MS_C * n;
    const int seed0 = wave * 32;
    const bool active = seed0 < S;                           // wave-uniform
    // B operand of S^T = X Z^T: lane holds Z[seed0 + col][2 kk + half]
    float zr[32];
    {
        const int s = seed0 + col;
        const float* zp = Z + ((size_t)b * S + min(s, S - 1)) * MS_C + half;
#pragma unroll
        for (int kk = 0; kk < 32; ++kk) zr[kk] = s < S ? zp[2 * kk] : 0.f;
    }
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
    // staging: lane loads pixel t & 63 of channels (t >> 6) + 4 i
    const int lp = t & (MS_TP - 1), lc = t >> 6;
    float pre[16];
    int tile = blockIdx.x;
    if (tile < ntiles) {
        const long p = (long)tile * MS_TP + lp;
#pragma unroll
        for (int i = 0; i < 16; ++i) pre[i] = p < n ? Xb[(size_t)(lc + 4 * i) * n + p] : 0.f;
    }
    for (; tile < ntiles; tile += G) {                       // (bounded by ntiles; uniform over the block)
        __syncthreads();                                     // the previous tile's reads are done
#pragma unroll
        for (int i = 0; i < 16; ++i) s_x[(lc + 4 * i) * MS_PITCH + lp] = pre[i];
        __syncthreads();
        if (tile + G < ntiles) {
            const long p = (long)(tile + G) * MS_TP + lp;
#pragma unroll
            for (int i = 0; i < 16; ++i) pre[i] = p < n ? Xb[(size_t)(lc + 4 * i) * n + p] : 0.f;
        }
        if (active) {
#pragma unroll
            for (int sub = 0; sub < MS_TP / 32; ++sub) {
                const int p0 = sub * 32;
                f32x16 s;
#pragma unroll
                for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
                for (int kk = 0; kk < 32; ++kk)              // A[pixel col][channel 2 kk + half], B[channel][seed col]
                    s = __builtin_amdgcn_mfma_f32_32x32x2f32(s_x[(2 * kk + half) * MS_PITCH + p0 + col], zr[kk], s, 0, 0, 0);
                // s[r] = dot(X[pixel p0 + (r & 3) + 8 (r >> 2) + 4 half], Z[seed0 + col]); a pixel behind n is a zero row: weight 1 on zeros
#pragma unroll
                for (int r = 0; r < 16; ++r) s[r] = expf(kappa * s[r]);
#pragma unroll
                for (int r = 0; r < 16; ++r) {               // A[seed col][k = half] = W of the pixel this half holds in register r
                    const float* xr = s_x + p0 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(s[r], xr[col * MS_PITCH], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(s[r], xr[(32 + col) * MS_PITCH], acc1, 0, 0, 0);
                }
            }
        }
    }
    if (!active) return;
    float* out = part + ((size_t)b * G + blockIdx.x) * MS_SMAX * MS_C;
#pragma unroll
    for (int r = 0; r < 16; ++r) {                           // acc[r] = [seed seed0 + (r & 3) + 8 (r >> 2) + 4 half][channel col (+ 32)]
        const int s = seed0 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (s < S) {
            out[(size_t)s * MS_C + col] = acc0[r];
            out[(size_t)s * MS_C + 32 + col] = acc1[r];
        }
    }
}

// grid (S, B), 64 lanes: Z[b][s] = normalize(sum over the G block partials in block order), float64 (F.normalize: x / max(|x|, 1e-12))
__global__ __launch_bounds__(64) void ms_mode_kernel(const float* __restrict__ part, float* __restrict__ Z, int S, int G) {
    __shared__ double s_v[MS_C];
    const int s = blockIdx.x, b = blockIdx.y, c = threadIdx.x;
    double a = 0.0;
    for (int g = 0; g < G; ++g) a += (double)part[(((size_t)b * G + g) * MS_SMAX + s) * MS_C + c];
    s_v[c] = a * a;
    __syncthreads();
    double ss = 0.0;
    for (int q = 0; q < MS_C; ++q) ss += s_v[q];
    Z[((size_t)b * S + s) * MS_C + c] = (float)(a / fmax(sqrt(ss), 1e-12));
}

// grid (B), 256 lanes.  labels i32 [B][S]
__global__ __launch_bounds__(256) void ms_link_kernel(const float* __restrict__ Z, int S, float eps, int* __restrict__ labels) {
    __shared__ float s_z[MS_SMAX * MS_PITCH];
    __shared__ unsigned s_adj[MS_SMAX * 4];
    __shared__ int s_lab[MS_SMAX];
    __shared__ int s_cnt[MS_SMAX];
    const int t = threadIdx.x, b = blockIdx.x;
    for (int i = t; i < S * MS_C; i += 256) s_z[(i >> 6) * MS_PITCH + (i & 63)] = Z[(size_t)b * S * MS_C + i];
    for (int i = t; i < MS_SMAX * 4; i += 256) s_adj[i] = 0;
    __syncthreads();
    for (int pair = t; pair < S * S; pair += 256) {
        const int i = pair / S, j = pair - i * S;
        float acc = 0.f;
#pragma unroll 16
        for (int c = 0; c < MS_C; ++c) acc = __fadd_rn(acc, __fmul_rn(s_z[i * MS_PITCH + c], s_z[j * MS_PITCH + c]));
        if (ms_dist(acc) <= eps) atomicOr(&s_adj[i * 4 + (j >> 5)], 1u << (j & 31));
    }
    __syncthreads();
    if (t == 0) {                                            // connected_components, as written (base_model.py:737-770)
        for (int i = 0; i < S; ++i) s_lab[i] = -1;
        int K = 0;
        for (int i = 0; i < S; ++i) {
            if (s_lab[i] != -1) continue;
            const unsigned* row = s_adj + i * 4;             // (the pinned dot is symmetric: column i = row i)
            for (int l = 0; l < S; ++l) s_cnt[l] = 0;
            int distinct = 0, unlabelled = 0;
            for (int j = 0; j < S; ++j) {
                if (!(row[j >> 5] >> (j & 31) & 1u)) continue;
                const int l = s_lab[j];
                if (l < 0) unlabelled = 1;
                else if (s_cnt[l]++ == 0) ++distinct;
            }
            int label;
            if (distinct + unlabelled > 1) {                 // the mode of the labels present, the smallest among equal counts
                label = 0;
                int best = -1;
                for (int l = 0; l < S; ++l)
                    if (s_cnt[l] > best) { best = s_cnt[l]; label = l; }
            } else {
                label = K++;
            }
            for (int j = 0; j < S; ++j)
                if (row[j >> 5] >> (j & 31) & 1u) s_lab[j] = label;
        }
    }
    __syncthreads();
    if (t < S) labels[(size_t)b * S + t] = s_lab[t];
}

// grid (ceil(n / 256), B).  raw i32 [B][n]: the seed label of the nearest seed; hist / pos u32 [B][MS_SMAX], zero on entry
__global__ __launch_bounds__(256) void ms_assign_kernel(const float* __restrict__ X, const float* __restrict__ Z, const int* __restrict__ seed_labels,
                                                        const float* __restrict__ depth_z, int n, int S, int* __restrict__ raw,
                                                        unsigned* __restrict__ hist, unsigned* __restrict__ pos) {
    __shared__ float s_z[MS_SMAX * MS_C];
    __shared__ int s_lab[MS_SMAX];
    __shared__ unsigned s_hist[MS_SMAX], s_pos[MS_SMAX];
    const int t = threadIdx.x, b = blockIdx.y;
    for (int i = t; i < S * MS_C; i += 256) s_z[i] = Z[(size_t)b * S * MS_C + i];
    if (t < MS_SMAX) { s_lab[t] = t < S ? seed_labels[(size_t)b * S + t] : -1; s_hist[t] = 0; s_pos[t] = 0; }
    __syncthreads();
    const int p = blockIdx.x * 256 + t;
    if (p < n) {
        float x[MS_C];
#pragma unroll
        for (int c = 0; c < MS_C; ++c) x[c] = X[((size_t)b * MS_C + c) * n + p];
        float best = 0.f;
        int bi = 0;
        for (int s = 0; s < S; ++s) {
            float acc = 0.f;
#pragma unroll
            for (int c = 0; c < MS_C; ++c) acc = __fadd_rn(acc, __fmul_rn(x[c], s_z[s * MS_C + c]));
            const float d = ms_dist(acc);
            if (s == 0 || d < best) { best = d; bi = s; }    // the first index of the minimum
        }
        const int l = s_lab[bi];
        raw[(size_t)b * n + p] = l;
        if (l >= 0 && l < MS_SMAX) {
            atomicAdd(&s_hist[l], 1u);
            if (depth_z && depth_z[(size_t)b * n + p] > 0.f) atomicAdd(&s_pos[l], 1u);
        }
    }
    __syncthreads();
    if (t < MS_SMAX) {
        if (s_hist[t]) atomicAdd(hist + (size_t)b * MS_SMAX + t, s_hist[t]);
        if (s_pos[t]) atomicAdd(pos + (size_t)b * MS_SMAX + t, s_pos[t]);
    }
}

// grid (B), MS_SMAX lanes.  table i32 [B][MS_SMAX + 1]: raw label + 1 -> output id (entry 0: label -1, no mask); report i32 [B][4]
__global__ __launch_bounds__(MS_SMAX) void ms_finish_kernel(const int* __restrict__ seed_labels, const unsigned* __restrict__ hist,
                                                           const unsigned* __restrict__ pos, int S, int N, int filter, float thresh,
                                                           int* __restrict__ table, int* __restrict__ report) {
    __shared__ int s_lab[MS_SMAX];
    __shared__ int s_keep[MS_SMAX], s_cluster[MS_SMAX];
    __shared__ int s_num, s_big;
    const int t = threadIdx.x, b = blockIdx.x;
    s_lab[t] = t < S ? seed_labels[(size_t)b * S + t] : 0;
    if (t == 0) s_num = 0;
    __syncthreads();
    if (t < S) {                                             // num = distinct seed labels, -1 included (len(torch.unique))
        bool firstof = true;
        for (int j = 0; j < t; ++j) firstof = firstof && s_lab[j] != s_lab[t];
        if (firstof) atomicAdd(&s_num, 1);
    }
    __syncthreads();
    const unsigned* h = hist + (size_t)b * MS_SMAX;
    if (t == 0) {                                            // the first largest of the labels 0 .. num - 1
        int big = 0;
        for (int l = 1; l < s_num; ++l)
            if (h[l] > h[big]) big = l;
        s_big = big;
    }
    __syncthreads();
    // thread t is the label t AFTER the swap of 0 and big; src is what it was called before
    const int big = s_big, src = t == 0 ? big : t == big ? 0 : t;
    const unsigned px = h[src], ps = pos[(size_t)b * MS_SMAX + src];
    const int cluster = t > 0 && px > 0;
    s_cluster[t] = cluster;
    s_keep[t] = cluster && !(filter && __fdiv_rn((float)ps, (float)px) < thresh);
    __syncthreads();
    int rank = 0, kept = 0, clusters = 0;
    for (int q = 0; q < MS_SMAX; ++q) { rank += q < t && s_keep[q]; kept += s_keep[q]; clusters += s_cluster[q]; }
    table[(size_t)b * (MS_SMAX + 1) + src + 1] = s_keep[t] && rank < N ? rank + 1 : 0;
    if (t == 0) {
        table[(size_t)b * (MS_SMAX + 1)] = 0;
        report[b * 4] = min(kept, N); report[b * 4 + 1] = clusters; report[b * 4 + 2] = clusters - kept; report[b * 4 + 3] = kept > N;
    }
}

// grid (ceil(n / (256 * PIX)), B).  PIX = 16: n % 16 == 0 and 16-byte aligned outputs, 16 pixels per lane and store; PIX = 1: any.
template <int PIX>
__global__ __launch_bounds__(256) void ms_write_kernel(const int* __restrict__ raw, const int* __restrict__ table, int N, long n, uint8_t* __restrict__ planes,
                                                       int* __restrict__ ids) {
    __shared__ int s_id[MS_SMAX + 1];
    const int b = blockIdx.y, t = threadIdx.x;
    if (t <= MS_SMAX) s_id[t] = table[(size_t)b * (MS_SMAX + 1) + t];
    __syncthreads();
    const long p = ((long)blockIdx.x * 256 + t) * PIX;
    if (p >= n) return;
    int id[PIX];
#pragma unroll
    for (int k = 0; k < PIX; ++k) id[k] = s_id[min(max(raw[(size_t)b * n + p + k], -1), MS_SMAX - 1) + 1];
    uint8_t* dst = planes + (size_t)b * N * n + p;
    if (PIX == 16) {
        int4* q = reinterpret_cast<int4*>(ids + (size_t)b * n + p);
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = make_int4(id[4 * k], id[4 * k + 1], id[4 * k + 2], id[4 * k + 3]);
        for (int m = 0; m < N; ++m) {
            unsigned w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                w[k] = (id[4 * k] == m + 1 ? 0xffu : 0u) | (id[4 * k + 1] == m + 1 ? 0xff00u : 0u) | (id[4 * k + 2] == m + 1 ? 0xff0000u : 0u) |
                       (id[4 * k + 3] == m + 1 ? 0xff000000u : 0u);
            *reinterpret_cast<uint4*>(dst + (size_t)m * n) = make_uint4(w[0], w[1], w[2], w[3]);
        }
    } else {
        ids[(size_t)b * n + p] = id[0];
        for (int m = 0; m < N; ++m) dst[(size_t)m * n] = id[0] == m + 1 ? 255 : 0;
    }
}

// workspace, for `cap_b` frames of n pixels: slots, hist, pos (cleared by the entries that use them) | mind | raw | table | part
struct MsWs { unsigned long long* slots; unsigned* hist; unsigned* pos; float* mind; int* raw; int* table; float* part; };

static int ms_blocks(long n) { return (int)std::min<long>((n + MS_TP - 1) / MS_TP, MS_G); }

static size_t ms_layout(MsWs* out, void* ws, int cap_b, long n) {
    const size_t cb = (size_t)cap_b;
    MsWs none, &r = out ? *out : none;
    WsWalk w{static_cast<char*>(ws)};
    r.slots = w.take<unsigned long long>(cb * MS_SMAX);
    r.hist = w.take<unsigned>(cb * MS_SMAX * 2);
    r.pos = r.hist ? r.hist + cb * MS_SMAX : nullptr;
    r.mind = w.take<float>(cb * n);
    r.raw = w.take<int>(cb * n);
    r.table = w.take<int>(cb * (MS_SMAX + 1));
    r.part = w.take<float>(cb * ms_blocks(n) * MS_SMAX * MS_C);
    return w.off;
}

size_t meanshift_ws_bytes(int cap_b, int H, int W) { return ms_layout(nullptr, nullptr, cap_b, (long)H * W); }

static int ms_check(const char* what, int B, int S, int H, int W, std::initializer_list<const void*> ptrs, const void* ws) {
    if (B <= 0) return fail(std::string(what) + ": empty batch");
    if (H < 1 || W < 1) return fail(std::string(what) + ": negative or empty frame");
    if ((long)H * W > (1L << 24)) return fail(std::string(what) + ": a frame of more than 2^24 pixels (the pixel counts are compared in float32)");
    if (S < 1 || S > MS_SMAX) return fail(std::string(what) + ": num_seeds outside 1..128");
    if ((long)S > (long)H * W) return fail(std::string(what) + ": more seeds than the frame has pixels");
    if (!ws) return fail(std::string(what) + ": null tensor");
    for (const void* p : ptrs) {
        if (!p) return fail(std::string(what) + ": null tensor");
        if ((uintptr_t)p & 3) return fail(std::string(what) + ": a 32-bit tensor that is not 4-byte aligned");
    }
    return 0;
}

// X f32 [B][64][H][W], first i32 [B] -> idx i32 [B][S]
int launch_meanshift_seeds(const float* X, const int* first, int B, int S, int H, int W, int* idx, void* ws, int cap_b, hipStream_t st) {
    if (ms_check("meanshift seeds", B, S, H, W, {X, first, idx}, ws)) return -1;
    const int n = H * W;
    MsWs w;
    ms_layout(&w, ws, cap_b, n);
    if (launch_zero(w.slots, (size_t)B * S * 8, st)) return -1;
    ProfScope prof("meanshift_seeds", (double)S * B * n * (MS_C + 2) * 4.0, 2.0 * S * B * n * MS_C, st);
    for (int k = 0; k < S; ++k)
        hipLaunchKernelGGL(ms_seed_kernel, dim3((n + 255) / 256, B), dim3(256), 0, st, X, first, w.slots, w.mind, idx, n, S, k);
    QB_CHECK(hipGetLastError());
    return 0;
}

// Z f32 [B][S][64] in place: with idx (i32 [B][S]) it starts from the pixels idx names, without from its contents
int launch_meanshift_climb(const float* X, const int* idx, float* Z, int B, int S, int H, int W, float kappa, int iters, void* ws, int cap_b,
                           hipStream_t st) {
    if (ms_check("meanshift climb", B, S, H, W, {X, Z}, ws)) return -1;
    if (idx && ((uintptr_t)idx & 3)) return fail("meanshift climb: a 32-bit tensor that is not 4-byte aligned");
    if (iters < 0 || iters > 1000) return fail("meanshift climb: iters outside 0..1000");
    if (!(kappa >= 0.f) || kappa > MS_KAPPA_MAX) return fail("meanshift climb: kappa outside 0..64");
    const int n = H * W;
    MsWs w;
    ms_layout(&w, ws, cap_b, n);
    if (idx) {
        hipLaunchKernelGGL(ms_gather_kernel, dim3(S, B), dim3(64), 0, st, X, idx, Z, n, S);
        QB_CHECK(hipGetLastError());
    }
    const int ntiles = (n + MS_TP - 1) / MS_TP, G = ms_blocks(n);
    ProfScope prof("meanshift_climb", (double)iters * B * n * MS_C * 4.0, 4.0 * iters * B * (double)n * S * MS_C, st);
    for (int it = 0; it < iters; ++it) {
        hipLaunchKernelGGL(ms_climb_kernel, dim3(G, B), dim3(256), 0, st, X, Z, w.part, n, S, ntiles, kappa);
        hipLaunchKernelGGL(ms_mode_kernel, dim3(S, B), dim3(64), 0, st, w.part, Z, S, G);
    }
    QB_CHECK(hipGetLastError());
    return 0;
}

// Z f32 [B][S][64] -> labels i32 [B][S]
int launch_meanshift_link(const float* Z, int B, int S, float eps, int* labels, hipStream_t st) {
    if (B <= 0) return fail("meanshift link: empty batch");
    if (S < 1 || S > MS_SMAX) return fail("meanshift link: num_seeds outside 1..128");
    if (!Z || !labels) return fail("meanshift link: null tensor");
    if (((uintptr_t)Z & 3) || ((uintptr_t)labels & 3)) return fail("meanshift link: a 32-bit tensor that is not 4-byte aligned");
    if (!(eps >= 0.f)) return fail("meanshift link: epsilon is negative or not a number");
    ProfScope prof("meanshift_link", (double)B * S * (MS_C + 1) * 4.0, 2.0 * B * S * S * MS_C, st);
    hipLaunchKernelGGL(ms_link_kernel, dim3(B), dim3(256), 0, st, Z, S, eps, labels);
    QB_CHECK(hipGetLastError());
    return 0;
}

// depth_z f32 [B][H][W] or null (then no filter); N planes; -> ids i32 [B][H][W], planes u8 [B][N][H][W], report i32 [B][4]
int launch_meanshift_assign(const float* X, const float* Z, const int* seed_labels, const float* depth_z, float thresh, int B, int S, int N, int H,
                            int W, int* ids, uint8_t* planes, int* report, void* ws, int cap_b, hipStream_t st) {
    if (ms_check("meanshift assign", B, S, H, W, {X, Z, seed_labels, ids, report}, ws)) return -1;
    if (N < 0 || N > MS_NMAX) return fail("meanshift assign: n_masks outside 0..254");
    if (N > 0 && !planes) return fail("meanshift assign: null tensor");
    if (depth_z && ((uintptr_t)depth_z & 3)) return fail("meanshift assign: a 32-bit tensor that is not 4-byte aligned");
    if (depth_z && !(thresh >= 0.f && thresh <= 1.f)) return fail("meanshift assign: depth threshold outside 0..1");
    const long n = (long)H * W;
    MsWs w;
    ms_layout(&w, ws, cap_b, n);
    if (launch_zero(w.hist, (size_t)cap_b * MS_SMAX * 8, st)) return -1;
    {
        ProfScope prof("meanshift_assign", (double)B * n * (MS_C + 2) * 4.0, 2.0 * B * (double)n * S * MS_C, st);
        hipLaunchKernelGGL(ms_assign_kernel, dim3((unsigned)((n + 255) / 256), B), dim3(256), 0, st, X, Z, seed_labels, depth_z, (int)n, S, w.raw,
                           w.hist, w.pos);
        QB_CHECK(hipGetLastError());
    }
    ProfScope prof("meanshift_write", (double)B * n * (N + 8.0), 0.0, st);
    hipLaunchKernelGGL(ms_finish_kernel, dim3(B), dim3(MS_SMAX), 0, st, seed_labels, w.hist, w.pos, S, N, depth_z ? 1 : 0, thresh, w.table, report);
    if (n % 16 == 0 && ((uintptr_t)planes & 15) == 0 && ((uintptr_t)ids & 15) == 0)
        hipLaunchKernelGGL(ms_write_kernel<16>, dim3((unsigned)((n / 16 + 255) / 256), B), dim3(256), 0, st, w.raw, w.table, N, n, planes, ids);
    else
        hipLaunchKernelGGL(ms_write_kernel<1>, dim3((unsigned)((n + 255) / 256), B), dim3(256), 0, st, w.raw, w.table, N, n, planes, ids);
    QB_CHECK(hipGetLastError());
    return 0;
}

}  // namespace quber
