// Gaussian mean-shift clustering of 3-D centre votes into initial masks on the device, and the initial mask processing (IMP) that follows
// it (include/quber_hip.h: quber_gms_*; the definition is in INTEGRATION.md "Initial masks from centre votes" and, as numpy, in
// tests/test_gms_cpu.py: gms_np, imp_np).  Restates the UOIS-Net-3D base model's DSNWrapper.cluster -> GaussianMeanShift.
// mean_shift_smart_init (select_smart_seeds, seed_hill_climbing, connected_components; uois/src/cluster.py, segmentation.py:129-187) and
// UOISNet3D.process_initial_masks (segmentation.py:425-491), euclidean metric, on votes f32 [B][3][H][W] and fg u8 [B][H][W].
//
// dist(a, b) = sqrt((dx dx + dy dy) + dz dz) in float32, every operation rounded separately, the square root correctly rounded (the
// build has -ffp-contract=off and no fast-math; sqrtf is the correctly rounded one).
//
// Stream-ordered steps, no host copy, no memset node, no grid-wide barrier, no floating-point atomics:
//   compact one block per 1024 pixels counts its foreground pixels; a second launch adds the counts of the blocks in front (block order:
//           the rank of a pixel is its row-major rank) and writes every subsample-th foreground point to xs f32 [3][n_sub].
//   seeds   ONE workgroup of 16 waves per frame runs all S steps in one launch.  Wave w owns a contiguous range of 64-point rows; a
//           point is always handled by the same lane, so the running minimum needs no hand-over.  Per step: distance to the newest
//           seed, running minimum, q = floor(mind 2^20) summed in 64-bit integers per wave; the wave that holds the threshold
//           t = umul64hi(r << 32, total) walks its rows again and a wave scan finds the first point whose inclusive prefix exceeds t.
//   climb   thread s of a 256-thread block IS seed s; the block walks tiles of 256 points through LDS (every lane reads the same word:
//           a broadcast).  It accumulates sum w and sum w (x - z), w = exp(c |x - z|^2): the mean shift as a DELTA to the seed, so the
//           rounding errors scale with the shift and not with the coordinates.  Block partials go to the workspace; gm_mode_kernel adds
//           them in block order in float64.  The number of blocks depends on H, W and subsample only, never on the batch.
//   link    one workgroup per frame: S x S distances <= epsilon as bit rows in LDS, then the reference's sequential labelling by one
//           thread (bounded loops, every thread reaches every barrier).
//   assign  per foreground pixel the first seed at minimum dist (the square root is taken only where the squared distance improves:
//           sqrt is monotone, so the strict comparison of the roots decides exactly as the contract does); label histogram through LDS
//           into integer tables; one block per frame filters by min_pixels, renumbers and averages the centres; one pass writes the id
//           map and the planes.
//   imp     ONE workgroup per frame loops over the ids present, in ascending order, on the CURRENT map (an id that is absent is a
//           no-op of the sequential contract: the opening and closing of an empty mask is empty): source and destination bit planes in
//           LDS, erosion / dilation as word-wise shifts with OpenCV's ellipse and constant border (1 for an erosion, 0 for a
//           dilation), then ids[mask] = 0, ids[result] = o.  The largest 4-connected component is launch_cleanup_ids, unchanged; ids
//           left empty are dropped and the rest renumbered.
// Every output is overwritten by every call.
#include "common.h"
#include <algorithm>
#include <cmath>
#include <initializer_list>

namespace quber {

constexpr int GM_SMAX = 256;                 // seeds per frame at most: one thread of a climb block each
constexpr int GM_NMAX = 254;                 // output planes / ids at most (launch_cleanup_ids' limit)
constexpr int GM_G = 256;                    // climb blocks per frame at most
constexpr int GM_CHUNK = 1024;               // pixels of a compaction block
constexpr int GM_TILE = 256;                 // points of a climb tile
constexpr int GM_KMAX = 15;                  // IMP: largest structuring element
constexpr size_t GM_LDS_MAX = 152 * 1024;    // IMP: both bit planes (the CU has 160 KiB; the kernel's static tables stay below 1 KiB)

struct GmElem { int r; int hw[GM_KMAX]; };   // half widths of the ellipse's rows -r..r

__device__ __forceinline__ float gm_d2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}
__device__ __forceinline__ float gm_dist(float ax, float ay, float az, float bx, float by, float bz) { return sqrtf(gm_d2(ax, ay, az, bx, by, bz)); }

__device__ __forceinline__ unsigned long long gm_quant(float m) {       // min(floor(float64(m) 2^20), 2^31 - 1), m >= 0
    const double d = (double)m * 1048576.0;
    return d >= 2147483647.0 ? 2147483647ull : (unsigned long long)d;
}

__device__ __forceinline__ unsigned long long gm_wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// info i32 [B][4] in the workspace: n = foreground pixels, n_sub = ceil(n / sub), S = min(num_seeds, n_sub), 0
// grid (nblk, B), 1024 lanes: cnt[b][blk] = foreground pixels of the block's 1024
__global__ __launch_bounds__(GM_CHUNK) void gm_count_kernel(const uint8_t* __restrict__ fg, long HW, int nblk, int* __restrict__ cnt) {
    __shared__ int s_c[GM_CHUNK / 64];
    const int t = threadIdx.x, b = blockIdx.y;
    const long p = (long)blockIdx.x * GM_CHUNK + t;
    const bool on = p < HW && fg[(size_t)b * HW + p] != 0;
    const unsigned long long bal = __ballot(on);
    if ((t & 63) == 0) s_c[t >> 6] = __popcll(bal);
    __syncthreads();
    if (t == 0) {
        int c = 0;
        for (int w = 0; w < GM_CHUNK / 64; ++w) c += s_c[w];
        cnt[(size_t)b * nblk + blockIdx.x] = c;
    }
}

// grid (nblk, B), 1024 lanes.  xs f32 [B][3][HW] (rows of n_sub used).  out_info i32 [B][3] or null: n, n_sub, S
__global__ __launch_bounds__(GM_CHUNK) void gm_scatter_kernel(const float* __restrict__ votes, const uint8_t* __restrict__ fg, long HW, int nblk,
                                                              const int* __restrict__ cnt, int sub, int num_seeds, float* __restrict__ xs,
                                                              int* __restrict__ info, int* __restrict__ out_info) {
    __shared__ int s_c[GM_CHUNK / 64];
    __shared__ int s_red[GM_CHUNK / 64];
    const int t = threadIdx.x, b = blockIdx.y, blk = blockIdx.x;
    const int* cb = cnt + (size_t)b * nblk;
    int part = 0;
    for (int i = t; i < blk; i += GM_CHUNK) part += cb[i];       // integer sums: any order gives the same base
    part = (int)gm_wave_sum((unsigned long long)part);
    const long p = (long)blk * GM_CHUNK + t;
    const bool on = p < HW && fg[(size_t)b * HW + p] != 0;
    const unsigned long long bal = __ballot(on);
    if ((t & 63) == 0) { s_red[t >> 6] = part; s_c[t >> 6] = __popcll(bal); }
    __syncthreads();
    int base = 0;
    for (int w = 0; w < GM_CHUNK / 64; ++w) base += s_red[w];
    for (int w = 0; w < (t >> 6); ++w) base += s_c[w];
    if (on) {
        const int rank = base + __popcll(bal & ((1ull << (t & 63)) - 1ull));
        if (rank % sub == 0) {
            const int q = rank / sub;
#pragma unroll
            for (int c = 0; c < 3; ++c) xs[((size_t)b * 3 + c) * HW + q] = votes[((size_t)b * 3 + c) * HW + p];
        }
    }
    if (blk == nblk - 1 && t == GM_CHUNK - 1) {                  // base counts everything in front of the last wave of the last block
        const int n = base + __popcll(bal), nsub = (n + sub - 1) / sub, S = min(num_seeds, nsub);
        info[b * 4] = n; info[b * 4 + 1] = nsub; info[b * 4 + 2] = S; info[b * 4 + 3] = 0;
        if (out_info) { out_info[b * 3] = n; out_info[b * 3 + 1] = nsub; out_info[b * 3 + 2] = S; }
    }
}

// grid (B), 1024 lanes: all S steps of a frame.  idx i32 [B][num_seeds] (entries behind S: -1); draws u32 [B][num_seeds] (entry 0 unused)
__global__ __launch_bounds__(1024) void gm_seed_kernel(const float* __restrict__ xs, const int* __restrict__ info, const int* __restrict__ first,
                                                       const unsigned* __restrict__ draws, long HW, int num_seeds, float* __restrict__ mind,
                                                       int* __restrict__ idx) {
    __shared__ unsigned long long s_tot[16];
    __shared__ int s_j;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, b = blockIdx.x;
    const int nsub = info[b * 4 + 1], S = info[b * 4 + 2];
    for (int k = S + t; k < num_seeds; k += 1024) idx[(size_t)b * num_seeds + k] = -1;
    if (S <= 0) return;                                          // (uniform)
    const float* X0 = xs + (size_t)b * 3 * HW;
    const float *X1 = X0 + HW, *X2 = X1 + HW;
    float* md = mind + (size_t)b * HW;
    const int rows = (nsub + 63) / 64, rpw = (rows + 15) / 16;
    const int r0 = min(wave * rpw, rows), r1 = min(r0 + rpw, rows);
    int j = min(max(first[b], 0), nsub - 1);
    for (int k = 0; k < S; ++k) {                                // (bounded by S <= 256; uniform over the block)
        if (t == 0) idx[(size_t)b * num_seeds + k] = j;
        if (k + 1 >= S) break;                                   // the last seed has no successor
        const float sx = X0[j], sy = X1[j], sz = X2[j];
        unsigned long long sum = 0;
        for (int row = r0; row < r1; ++row) {
            const int p = row * 64 + lane;
            if (p < nsub) {
                float d = gm_dist(X0[p], X1[p], X2[p], sx, sy, sz);
                if (k > 0) d = fminf(md[p], d);
                md[p] = d;
                sum += gm_quant(d);
            }
        }
        sum = gm_wave_sum(sum);
        if (lane == 0) s_tot[wave] = sum;
        if (t == 0) s_j = 0;                                     // total == 0: index 0
        __syncthreads();
        unsigned long long total = 0;
        for (int w = 0; w < 16; ++w) total += s_tot[w];
        const unsigned long long thr = __umul64hi((unsigned long long)draws[(size_t)b * num_seeds + k + 1] << 32, total);
        unsigned long long base = 0;
        int owner = -1;
        for (int w = 0; w < 16; ++w) {
            if (owner < 0 && total > 0 && base + s_tot[w] > thr) owner = w;
            if (owner < 0) base += s_tot[w];
        }
        if (wave == owner) {                                     // (wave-uniform) thr < total, so the walk ends inside this wave's rows
            for (int row = r0; row < r1; ++row) {
                const int p = row * 64 + lane;
                const unsigned long long q = p < nsub ? gm_quant(md[p]) : 0ull;
                unsigned long long inc = q;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const unsigned long long up = __shfl_up(inc, o, 64);
                    if (lane >= o) inc += up;
                }
                const unsigned long long hit = __ballot(base + inc > thr);
                if (hit) {
                    if (lane == 0) s_j = row * 64 + (__ffsll((long long)hit) - 1);
                    break;
                }
                base += __shfl(inc, 63, 64);
            }
        }
        __syncthreads();
        j = min(s_j, nsub - 1);
        __syncthreads();                                         // s_j and s_tot are rewritten by the next step
    }
}

// grid (num_seeds, B), 64 lanes (3 used): Z[b][s] = Xs[idx[b][s]], zero where idx < 0
__global__ __launch_bounds__(64) void gm_gather_kernel(const float* __restrict__ xs, const int* __restrict__ info, const int* __restrict__ idx, long HW,
                                                       int num_seeds, float* __restrict__ Z) {
    const int s = blockIdx.x, b = blockIdx.y, c = threadIdx.x;
    if (c >= 3) return;
    const int j = idx[(size_t)b * num_seeds + s], nsub = info[b * 4 + 1];
    Z[((size_t)b * num_seeds + s) * 3 + c] = (j >= 0 && j < nsub) ? xs[((size_t)b * 3 + c) * HW + j] : 0.f;
}

// grid (G, B), 256 lanes: lane s is seed s.  part f32 [B][G][256][4]: sum w, sum w (x - z)
__global__ __launch_bounds__(GM_SMAX) void gm_climb_kernel(const float* __restrict__ xs, const int* __restrict__ info, const float* __restrict__ Z,
                                                           long HW, int num_seeds, float c, float* __restrict__ part) {
    __shared__ float s_p[3][GM_TILE];
    const int t = threadIdx.x, b = blockIdx.y, G = gridDim.x;
    const int nsub = info[b * 4 + 1], ntiles = (nsub + GM_TILE - 1) / GM_TILE;
    const float* Xb = xs + (size_t)b * 3 * HW;
    float zx = 0.f, zy = 0.f, zz = 0.f;
    if (t < num_seeds) {
        const float* z = Z + ((size_t)b * num_seeds + t) * 3;
        zx = z[0]; zy = z[1]; zz = z[2];
    }
    float sw = 0.f, ax = 0.f, ay = 0.f, az = 0.f;
    for (int tile = blockIdx.x; tile < ntiles; tile += G) {      // (bounded by ntiles; uniform over the block)
        __syncthreads();                                         // the previous tile's reads are done
        const int p = tile * GM_TILE + t;
#pragma unroll
        for (int k = 0; k < 3; ++k) s_p[k][t] = p < nsub ? Xb[(size_t)k * HW + p] : 0.f;
        __syncthreads();
        const int cnt = min(GM_TILE, nsub - tile * GM_TILE);
        for (int i = 0; i < cnt; ++i) {
            const float dx = s_p[0][i] - zx, dy = s_p[1][i] - zy, dz = s_p[2][i] - zz;
            const float w = expf(c * ((dx * dx + dy * dy) + dz * dz));
            sw += w; ax += w * dx; ay += w * dy; az += w * dz;
        }
    }
    reinterpret_cast<float4*>(part)[((size_t)b * G + blockIdx.x) * GM_SMAX + t] = make_float4(sw, ax, ay, az);
}

// grid (B), 256 lanes: Z[b][s] += (sum of the G partials in block order, float64) / (sum w); a seed whose weights sum to 0 stays
__global__ __launch_bounds__(GM_SMAX) void gm_mode_kernel(const float* __restrict__ part, const int* __restrict__ counts, int num_seeds, int G,
                                                          float* __restrict__ Z) {
    const int s = threadIdx.x, b = blockIdx.x;
    const int S = counts ? min(max(counts[b * 3 + 2], 0), num_seeds) : num_seeds;
    if (s >= S) return;
    double w = 0.0, x = 0.0, y = 0.0, z = 0.0;
    for (int g = 0; g < G; ++g) {
        const float4 v = reinterpret_cast<const float4*>(part)[((size_t)b * G + g) * GM_SMAX + s];
        w += (double)v.x; x += (double)v.y; y += (double)v.z; z += (double)v.w;
    }
    if (!(w > 0.0)) return;
    float* zp = Z + ((size_t)b * num_seeds + s) * 3;
    zp[0] = (float)((double)zp[0] + x / w);
    zp[1] = (float)((double)zp[1] + y / w);
    zp[2] = (float)((double)zp[2] + z / w);
}

// grid (B), 256 lanes.  labels i32 [B][num_seeds]; entries behind the frame's S: -1
__global__ __launch_bounds__(256) void gm_link_kernel(const float* __restrict__ Z, const int* __restrict__ counts, int num_seeds, float eps,
                                                      int* __restrict__ labels) {
    __shared__ float s_z[GM_SMAX * 3];
    __shared__ unsigned s_adj[GM_SMAX * 8];
    __shared__ int s_lab[GM_SMAX];
    __shared__ int s_cnt[GM_SMAX];
    const int t = threadIdx.x, b = blockIdx.x;
    const int S = counts ? min(max(counts[b * 3 + 2], 0), num_seeds) : num_seeds;
    for (int i = t; i < S * 3; i += 256) s_z[i] = Z[(size_t)b * num_seeds * 3 + i];
    for (int i = t; i < GM_SMAX * 8; i += 256) s_adj[i] = 0;
    s_lab[t] = -1;
    __syncthreads();
    for (int pair = t; pair < S * S; pair += 256) {
        const int i = pair / S, j = pair - i * S;
        if (gm_dist(s_z[j * 3], s_z[j * 3 + 1], s_z[j * 3 + 2], s_z[i * 3], s_z[i * 3 + 1], s_z[i * 3 + 2]) <= eps)
            atomicOr(&s_adj[i * 8 + (j >> 5)], 1u << (j & 31));
    }
    __syncthreads();
    if (t == 0) {                                            // connected_components, as written (cluster.py:60-90)
        int K = 0;
        for (int i = 0; i < S; ++i) {
            if (s_lab[i] != -1) continue;
            const unsigned* row = s_adj + i * 8;             // (dist is symmetric: column i = row i)
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
    if (t < num_seeds) labels[(size_t)b * num_seeds + t] = t < S ? s_lab[t] : -1;
}

// grid (ceil(HW / 256), B).  raw i32 [B][HW]: the label of the nearest seed, -1 off the foreground; hist u32 [B][GM_SMAX + 1], zero on
// entry: pixels per label, and in slot GM_SMAX the foreground pixels
__global__ __launch_bounds__(256) void gm_assign_kernel(const float* __restrict__ votes, const uint8_t* __restrict__ fg, const float* __restrict__ Z,
                                                        const int* __restrict__ seed_labels, const int* __restrict__ counts, long HW, int num_seeds,
                                                        int* __restrict__ raw, unsigned* __restrict__ hist) {
    __shared__ float s_z[GM_SMAX * 3];
    __shared__ int s_lab[GM_SMAX];
    __shared__ unsigned s_hist[GM_SMAX + 1];
    const int t = threadIdx.x, b = blockIdx.y;
    const int S = counts ? min(max(counts[b * 3 + 2], 0), num_seeds) : num_seeds;
    for (int i = t; i < S * 3; i += 256) s_z[i] = Z[(size_t)b * num_seeds * 3 + i];
    s_lab[t] = t < S ? seed_labels[(size_t)b * num_seeds + t] : -1;
    s_hist[t] = 0;
    if (t == 0) s_hist[GM_SMAX] = 0;
    __syncthreads();
    const long p = (long)blockIdx.x * 256 + t;
    if (p < HW) {
        int l = -1;
        if (fg[(size_t)b * HW + p] != 0) {
            atomicAdd(&s_hist[GM_SMAX], 1u);
            const float x = votes[((size_t)b * 3) * HW + p], y = votes[((size_t)b * 3 + 1) * HW + p], z = votes[((size_t)b * 3 + 2) * HW + p];
            float best = 0.f, best2 = 0.f;
            int bi = -1;
            for (int s = 0; s < S; ++s) {
                const float d2 = gm_d2(x, y, z, s_z[s * 3], s_z[s * 3 + 1], s_z[s * 3 + 2]);
                if (bi < 0 || d2 < best2) {                  // d2 >= best2 implies sqrt(d2) >= best: only an improvement needs the root
                    const float d = sqrtf(d2);
                    if (bi < 0 || d < best) { best = d; best2 = d2; bi = s; }
                }
            }
            if (bi >= 0) l = s_lab[bi];
            if (l >= 0 && l < GM_SMAX) atomicAdd(&s_hist[l], 1u);
            else l = -1;
        }
        raw[(size_t)b * HW + p] = l;
    }
    __syncthreads();
    if (s_hist[t]) atomicAdd(hist + (size_t)b * (GM_SMAX + 1) + t, s_hist[t]);
    if (t == 0 && s_hist[GM_SMAX]) atomicAdd(hist + (size_t)b * (GM_SMAX + 1) + GM_SMAX, s_hist[GM_SMAX]);
}

// grid (B), 256 lanes: lane l is label l.  table i32 [B][GM_SMAX + 1]: raw label + 1 -> output id; centers f32 [B][N][3]; report i32 [B][6]
__global__ __launch_bounds__(GM_SMAX) void gm_finish_kernel(const float* __restrict__ Z, const int* __restrict__ seed_labels, const int* __restrict__ counts,
                                                            const unsigned* __restrict__ hist, int num_seeds, int N, int min_pixels,
                                                            int* __restrict__ table, float* __restrict__ centers, int* __restrict__ report) {
    __shared__ int s_lab[GM_SMAX];
    __shared__ int s_keep[GM_SMAX];
    __shared__ int s_K;
    const int t = threadIdx.x, b = blockIdx.x;
    const int S = counts ? min(max(counts[b * 3 + 2], 0), num_seeds) : num_seeds;
    s_lab[t] = t < S ? seed_labels[(size_t)b * num_seeds + t] : -1;
    if (t == 0) s_K = 0;
    __syncthreads();
    if (s_lab[t] >= 0) atomicMax(&s_K, min(s_lab[t], GM_SMAX - 1) + 1);
    __syncthreads();
    const int K = s_K;
    const unsigned px = hist[(size_t)b * (GM_SMAX + 1) + t];
    s_keep[t] = t < K && px >= (unsigned)min_pixels;
    if (t < N) { float* c = centers + ((size_t)b * N + t) * 3; c[0] = 0.f; c[1] = 0.f; c[2] = 0.f; }
    __syncthreads();
    int rank = 0, kept = 0;
    for (int q = 0; q < GM_SMAX; ++q) { rank += q < t && s_keep[q]; kept += s_keep[q]; }
    const int out = s_keep[t] && rank < N ? rank + 1 : 0;
    table[(size_t)b * (GM_SMAX + 1) + t + 1] = out;
    if (out) {                                               // the mean of the climbed seeds that carry the label: float32, in seed order
        float sx = 0.f, sy = 0.f, sz = 0.f;
        int m = 0;
        for (int s = 0; s < S; ++s)
            if (s_lab[s] == t) {
                const float* z = Z + ((size_t)b * num_seeds + s) * 3;
                sx = __fadd_rn(sx, z[0]); sy = __fadd_rn(sy, z[1]); sz = __fadd_rn(sz, z[2]);
                ++m;
            }
        float* c = centers + ((size_t)b * N + out - 1) * 3;
        c[0] = __fdiv_rn(sx, (float)m); c[1] = __fdiv_rn(sy, (float)m); c[2] = __fdiv_rn(sz, (float)m);
    }
    if (t == 0) {
        table[(size_t)b * (GM_SMAX + 1)] = 0;
        int* r = report + b * 6;
        r[0] = min(kept, N); r[1] = K; r[2] = K - kept; r[3] = kept > N; r[4] = 0; r[5] = (int)hist[(size_t)b * (GM_SMAX + 1) + GM_SMAX];
    }
}

// grid (ceil(n / (256 * PIX)), B): id = table[src + 1] -> ids, and planes u8 [B][N][n] (may be null).  src may be ids (each lane reads
// its pixels before it writes them).  PIX = 16: n % 16 == 0 and 16-byte aligned tensors, 16 pixels per lane and store; PIX = 1: any.
template <int PIX>
__global__ __launch_bounds__(256) void gm_write_kernel(const int* src, const int* __restrict__ table, int N, long n, uint8_t* __restrict__ planes, int* ids) {
    __shared__ int s_id[GM_SMAX + 1];
    const int b = blockIdx.y, t = threadIdx.x;
    s_id[t] = table[(size_t)b * (GM_SMAX + 1) + t];
    if (t == 0) s_id[GM_SMAX] = table[(size_t)b * (GM_SMAX + 1) + GM_SMAX];
    __syncthreads();
    const long p = ((long)blockIdx.x * 256 + t) * PIX;
    if (p >= n) return;
    int id[PIX];
#pragma unroll
    for (int k = 0; k < PIX; ++k) id[k] = s_id[min(max(src[(size_t)b * n + p + k], -1), GM_SMAX - 1) + 1];
    uint8_t* dst = planes ? planes + (size_t)b * N * n + p : nullptr;
    if (PIX == 16) {
        int4* q = reinterpret_cast<int4*>(ids + (size_t)b * n + p);
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = make_int4(id[4 * k], id[4 * k + 1], id[4 * k + 2], id[4 * k + 3]);
        for (int m = 0; dst && m < N; ++m) {
            unsigned w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                w[k] = (id[4 * k] == m + 1 ? 0xffu : 0u) | (id[4 * k + 1] == m + 1 ? 0xff00u : 0u) | (id[4 * k + 2] == m + 1 ? 0xff0000u : 0u) |
                       (id[4 * k + 3] == m + 1 ? 0xff000000u : 0u);
            *reinterpret_cast<uint4*>(dst + (size_t)m * n) = make_uint4(w[0], w[1], w[2], w[3]);
        }
    } else {
        ids[(size_t)b * n + p] = id[0];
        for (int m = 0; dst && m < N; ++m) dst[(size_t)m * n] = id[0] == m + 1 ? 255 : 0;
    }
}

__global__ __launch_bounds__(256) void gm_copy_kernel(const int* __restrict__ src, int* __restrict__ dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// ---- IMP ----
__device__ __forceinline__ unsigned gm_word(const unsigned* pl, int y, int wx, int H, int wpr, unsigned last, unsigned border) {
    if (y < 0 || y >= H || wx < 0 || wx >= wpr) return border;
    const unsigned v = pl[y * wpr + wx];
    return wx == wpr - 1 ? (v & last) | (border & ~last) : v;
}

// src -> dst over H x wpr words; ERODE: AND with border 1, else OR with border 0
template <bool ERODE>
__device__ __forceinline__ void gm_morph(const unsigned* src, unsigned* dst, int H, int wpr, unsigned last, const GmElem& e) {
    const unsigned border = ERODE ? 0xffffffffu : 0u;
    for (int i = threadIdx.x; i < H * wpr; i += 1024) {
        const int y = i / wpr, wx = i - y * wpr;
        unsigned acc = border;
        for (int dy = -e.r; dy <= e.r; ++dy) {
            const int hw = e.hw[dy + e.r];
            const unsigned cur = gm_word(src, y + dy, wx, H, wpr, last, border);
            unsigned row = cur;
            if (hw > 0) {
                const unsigned prev = gm_word(src, y + dy, wx - 1, H, wpr, last, border), next = gm_word(src, y + dy, wx + 1, H, wpr, last, border);
                for (int s = 1; s <= hw; ++s) {              // (hw <= 7: the shifts stay inside 1..31)
                    const unsigned a = (cur >> s) | (next << (32 - s)), c = (cur << s) | (prev >> (32 - s));
                    row = ERODE ? (row & a & c) : (row | a | c);
                }
            }
            acc = ERODE ? (acc & row) : (acc | row);
        }
        dst[i] = acc;
    }
}

// grid (B), 1024 lanes, dynamic LDS: two planes of H x wpr words.  ids i32 [B][H][W] in place; before u32 [B][8]: the ids present on entry
__global__ __launch_bounds__(1024) void gm_imp_kernel(int* ids, int n_ids, int H, int W, int wpr, GmElem e, unsigned* __restrict__ before) {
    extern __shared__ unsigned gm_planes[];
    __shared__ unsigned s_present[8];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, b = blockIdx.x;
    const long HW = (long)H * W;
    int* map = ids + (size_t)b * HW;
    unsigned* A = gm_planes;
    unsigned* Bp = gm_planes + (size_t)H * wpr;
    const unsigned last = (W & 31) ? (1u << (W & 31)) - 1u : 0xffffffffu;
    if (t < 8) s_present[t] = 0;
    __syncthreads();
    int seen = 0;
    for (long p = t; p < HW; p += 1024) {                        // a value outside 0..n_ids counts as 0 and is written back as 0
        int v = map[p];
        if (v < 0 || v > n_ids) { v = 0; map[p] = 0; }
        if (v != seen && v > 0) atomicOr(&s_present[v >> 5], 1u << (v & 31));
        seen = v;
    }
    __syncthreads();
    if (t < 8) before[b * 8 + t] = s_present[t];
    const int cpr = (W + 63) / 64;
    for (int o = 1; o <= n_ids; ++o) {                           // (bounded by n_ids <= 254; uniform over the block)
        if (!(s_present[o >> 5] >> (o & 31) & 1u)) continue;
        for (int item = wave; item < H * cpr; item += 16) {      // A = (ids == o), 64 pixels per wave and ballot
            const int y = item / cpr, cx = item - y * cpr, x = cx * 64 + lane;
            const unsigned long long bal = __ballot(x < W && map[(long)y * W + x] == o);
            if (lane == 0) {
                A[y * wpr + 2 * cx] = (unsigned)bal;
                if (2 * cx + 1 < wpr) A[y * wpr + 2 * cx + 1] = (unsigned)(bal >> 32);
            }
        }
        __syncthreads();
        gm_morph<true>(A, Bp, H, wpr, last, e);  __syncthreads();    // open
        gm_morph<false>(Bp, A, H, wpr, last, e); __syncthreads();
        gm_morph<false>(A, Bp, H, wpr, last, e); __syncthreads();    // close
        gm_morph<true>(Bp, A, H, wpr, last, e);  __syncthreads();
        for (long p = t; p < HW; p += 1024) {
            const int y = (int)(p / W), x = (int)(p - (long)y * W);
            const int v = map[p];
            const int nv = (A[y * wpr + (x >> 5)] >> (x & 31) & 1u) ? o : (v == o ? 0 : v);
            if (nv != v) map[p] = nv;
        }
        __syncthreads();
    }
}

// grid (ceil(HW / 256), B): after u32 [B][8], zero on entry: the ids 1..n_ids present
__global__ __launch_bounds__(256) void gm_present_kernel(const int* __restrict__ ids, long HW, int n_ids, unsigned* __restrict__ after) {
    __shared__ unsigned s_present[8];
    const int t = threadIdx.x, b = blockIdx.y;
    if (t < 8) s_present[t] = 0;
    __syncthreads();
    const long p = (long)blockIdx.x * 256 + t;
    if (p < HW) {
        const int v = ids[(size_t)b * HW + p];
        if (v > 0 && v <= n_ids) atomicOr(&s_present[v >> 5], 1u << (v & 31));
    }
    __syncthreads();
    if (t < 8 && s_present[t]) atomicOr(after + b * 8 + t, s_present[t]);
}

// grid (B), 256 lanes: lane i is id i.  table[i + 1] = the new id of i; centers f32 [B][n_ids][3] (may be null) compacted alike;
// report i32 [B][6] (may be null): [0] = ids left, [4] = ids present before and empty now
__global__ __launch_bounds__(GM_SMAX) void gm_imp_finish_kernel(const unsigned* __restrict__ before, const unsigned* __restrict__ after, int n_ids,
                                                                int* __restrict__ table, float* centers, int* __restrict__ report) {
    __shared__ int s_on[GM_SMAX];
    __shared__ float s_c[GM_SMAX * 3];
    const int t = threadIdx.x, b = blockIdx.x;
    const int on = t >= 1 && t <= n_ids && (after[b * 8 + (t >> 5)] >> (t & 31) & 1u);
    const int was = t >= 1 && t <= n_ids && (before[b * 8 + (t >> 5)] >> (t & 31) & 1u);
    s_on[t] = on;
    if (centers && t >= 1 && t <= n_ids)
        for (int c = 0; c < 3; ++c) s_c[t * 3 + c] = centers[((size_t)b * n_ids + t - 1) * 3 + c];
    __syncthreads();
    int rank = 0, left = 0;
    for (int q = 0; q < GM_SMAX; ++q) { rank += q < t && s_on[q]; left += s_on[q]; }
    table[(size_t)b * (GM_SMAX + 1) + t + 1] = on ? rank + 1 : 0;
    if (t == 0) table[(size_t)b * (GM_SMAX + 1)] = 0;
    if (centers && t >= 1 && t <= n_ids) {
        if (t > left)
            for (int c = 0; c < 3; ++c) centers[((size_t)b * n_ids + t - 1) * 3 + c] = 0.f;
        if (on)
            for (int c = 0; c < 3; ++c) centers[((size_t)b * n_ids + rank) * 3 + c] = s_c[t * 3 + c];
    }
    __syncthreads();                                         // every lane has counted its rank
    s_on[t] = was && !on;
    __syncthreads();
    if (t == 0 && report) {
        int emptied = 0;
        for (int q = 0; q < GM_SMAX; ++q) emptied += s_on[q];
        report[b * 6] = left; report[b * 6 + 4] = emptied;
    }
}

// workspace, for `cap_b` frames of HW pixels
struct GmWs { int* info; unsigned* hist; unsigned* flags; int* table; int* cnt; float* xs; float* mind; int* raw; float* part; };

static int gm_nblk(long HW) { return (int)((HW + GM_CHUNK - 1) / GM_CHUNK); }

static size_t gm_layout(GmWs* out, void* ws, int cap_b, long HW) {
    const size_t cb = (size_t)cap_b;
    GmWs none, &r = out ? *out : none;
    WsWalk w{static_cast<char*>(ws)};
    r.info = w.take<int>(cb * 4);
    r.hist = w.take<unsigned>(cb * (GM_SMAX + 1));
    r.flags = w.take<unsigned>(cb * 16);                    // [2][cap_b][8]: before, after
    r.table = w.take<int>(cb * (GM_SMAX + 1));
    r.cnt = w.take<int>(cb * gm_nblk(HW));
    r.xs = w.take<float>(cb * 3 * HW);
    r.mind = w.take<float>(cb * HW);
    r.raw = w.take<int>(cb * HW);
    r.part = w.take<float>(cb * GM_G * GM_SMAX * 4);
    return w.off;
}

size_t gms_ws_bytes(int cap_b, int H, int W) { return gm_layout(nullptr, nullptr, cap_b, (long)H * W); }

// once per process, from the call that allocates the workspace: the IMP kernel may use more than the default 64 KiB of LDS
int gms_prepare() {
    QB_CHECK(hipFuncSetAttribute((const void*)gm_imp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GM_LDS_MAX));
    return 0;
}

static int gm_check(const char* what, int B, int cap_b, int S, int H, int W, std::initializer_list<const void*> ptrs, const void* ws) {
    if (B <= 0 || B > cap_b || B > 65535) return fail(std::string(what) + ": batch outside 1..max_batch");
    if (H < 1 || W < 1) return fail(std::string(what) + ": negative or empty frame");
    if ((long)H * W > (1L << 24)) return fail(std::string(what) + ": a frame of more than 2^24 pixels");
    if (S < 1 || S > GM_SMAX) return fail(std::string(what) + ": num_seeds outside 1..256");
    if (!ws) return fail(std::string(what) + ": null tensor");
    for (const void* p : ptrs) {
        if (!p) return fail(std::string(what) + ": null tensor");
        if ((uintptr_t)p & 3) return fail(std::string(what) + ": a 32-bit tensor that is not 4-byte aligned");
    }
    return 0;
}

static int gm_compact(const float* votes, const uint8_t* fg, int B, int S, long HW, int sub, int* out_info, const GmWs& w, hipStream_t st) {
    if (sub < 1 || sub > 64) return fail("gms: subsample outside 1..64");
    if (!fg) return fail("gms: null tensor");
    const int nblk = gm_nblk(HW);
    ProfScope prof("gms_compact", (double)B * HW * 2.0 + (double)B * HW / sub * 24.0, 0.0, st);
    hipLaunchKernelGGL(gm_count_kernel, dim3(nblk, B), dim3(GM_CHUNK), 0, st, fg, HW, nblk, w.cnt);
    hipLaunchKernelGGL(gm_scatter_kernel, dim3(nblk, B), dim3(GM_CHUNK), 0, st, votes, fg, HW, nblk, w.cnt, sub, S, w.xs, w.info, out_info);
    QB_CHECK(hipGetLastError());
    return 0;
}

// votes f32 [B][3][H][W], fg u8 [B][H][W], first i32 [B], draws u32 [B][S] -> idx i32 [B][S], info i32 [B][3] (may be null)
int launch_gms_seeds(const float* votes, const uint8_t* fg, const int* first, const unsigned* draws, int B, int S, int sub, int H, int W, int* idx,
                     int* info, void* ws, int cap_b, hipStream_t st) {
    if (gm_check("gms seeds", B, cap_b, S, H, W, {votes, first, draws, idx}, ws)) return -1;
    if (info && ((uintptr_t)info & 3)) return fail("gms seeds: a 32-bit tensor that is not 4-byte aligned");
    const long HW = (long)H * W;
    GmWs w;
    gm_layout(&w, ws, cap_b, HW);
    if (gm_compact(votes, fg, B, S, HW, sub, info, w, st)) return -1;
    ProfScope prof("gms_seeds", (double)S * B * HW / sub * 20.0, (double)S * B * HW / sub * 12.0, st);
    hipLaunchKernelGGL(gm_seed_kernel, dim3(B), dim3(1024), 0, st, w.xs, w.info, first, draws, HW, S, w.mind, idx);
    QB_CHECK(hipGetLastError());
    return 0;
}

// Z f32 [B][S][3] in place: with idx (i32 [B][S]) it starts from the subsampled points idx names; counts i32 [B][3] or null (every row)
int launch_gms_climb(const float* votes, const uint8_t* fg, const int* idx, const int* counts, float* Z, int B, int S, int sub, int H, int W,
                     float sigma, int iters, bool compact, void* ws, int cap_b, hipStream_t st) {
    if (gm_check("gms climb", B, cap_b, S, H, W, {votes, Z}, ws)) return -1;
    if (((uintptr_t)idx & 3) || ((uintptr_t)counts & 3)) return fail("gms climb: a 32-bit tensor that is not 4-byte aligned");
    if (iters < 0 || iters > 1000) return fail("gms climb: iters outside 0..1000");
    if (!(sigma > 0.f) || !std::isfinite(sigma)) return fail("gms climb: sigma must be positive");
    const long HW = (long)H * W;
    GmWs w;
    gm_layout(&w, ws, cap_b, HW);
    if (sub < 1 || sub > 64) return fail("gms: subsample outside 1..64");
    if (compact && gm_compact(votes, fg, B, S, HW, sub, nullptr, w, st)) return -1;
    if (idx) {
        hipLaunchKernelGGL(gm_gather_kernel, dim3(S, B), dim3(64), 0, st, w.xs, w.info, idx, HW, S, Z);
        QB_CHECK(hipGetLastError());
    }
    const float c = (float)(-0.5 / ((double)sigma * (double)sigma));
    const long maxsub = (HW + sub - 1) / sub;
    const int G = (int)std::min<long>((maxsub + GM_TILE - 1) / GM_TILE, GM_G);
    ProfScope prof("gms_climb", (double)iters * B * maxsub * 12.0, 14.0 * iters * B * (double)maxsub * S, st);
    for (int it = 0; it < iters; ++it) {
        hipLaunchKernelGGL(gm_climb_kernel, dim3(G, B), dim3(GM_SMAX), 0, st, w.xs, w.info, Z, HW, S, c, w.part);
        hipLaunchKernelGGL(gm_mode_kernel, dim3(B), dim3(GM_SMAX), 0, st, w.part, counts, S, G, Z);
    }
    QB_CHECK(hipGetLastError());
    return 0;
}

// Z f32 [B][S][3] -> labels i32 [B][S]
int launch_gms_link(const float* Z, const int* counts, int B, int S, float eps, int* labels, hipStream_t st) {
    if (B <= 0 || B > 65535) return fail("gms link: batch outside 1..65535");
    if (S < 1 || S > GM_SMAX) return fail("gms link: num_seeds outside 1..256");
    if (!Z || !labels) return fail("gms link: null tensor");
    if (((uintptr_t)Z & 3) || ((uintptr_t)labels & 3) || ((uintptr_t)counts & 3)) return fail("gms link: a 32-bit tensor that is not 4-byte aligned");
    if (!(eps >= 0.f)) return fail("gms link: epsilon is negative or not a number");
    ProfScope prof("gms_link", (double)B * S * 16.0, 10.0 * B * S * S, st);
    hipLaunchKernelGGL(gm_link_kernel, dim3(B), dim3(256), 0, st, Z, counts, S, eps, labels);
    QB_CHECK(hipGetLastError());
    return 0;
}

static void gm_write(const int* src, const int* table, int B, int N, long n, uint8_t* planes, int* ids, hipStream_t st) {
    if (n % 16 == 0 && ((uintptr_t)planes & 15) == 0 && ((uintptr_t)ids & 15) == 0 && ((uintptr_t)src & 15) == 0)
        hipLaunchKernelGGL(gm_write_kernel<16>, dim3((unsigned)((n / 16 + 255) / 256), B), dim3(256), 0, st, src, table, N, n, planes, ids);
    else
        hipLaunchKernelGGL(gm_write_kernel<1>, dim3((unsigned)((n + 255) / 256), B), dim3(256), 0, st, src, table, N, n, planes, ids);
}

// -> ids i32 [B][H][W], planes u8 [B][N][H][W] (may be null), centers f32 [B][N][3], report i32 [B][6]
int launch_gms_assign(const float* votes, const uint8_t* fg, const float* Z, const int* seed_labels, const int* counts, int B, int S, int N,
                      int min_pixels, int H, int W, int* ids, uint8_t* planes, float* centers, int* report, void* ws, int cap_b, hipStream_t st) {
    if (gm_check("gms assign", B, cap_b, S, H, W, {votes, Z, seed_labels, ids, centers, report}, ws)) return -1;
    if (!fg) return fail("gms assign: null tensor");
    if ((uintptr_t)counts & 3) return fail("gms assign: a 32-bit tensor that is not 4-byte aligned");
    if (N < 1 || N > GM_NMAX) return fail("gms assign: n_masks outside 1..254");
    if (min_pixels < 0) return fail("gms assign: negative min_pixels");
    const long HW = (long)H * W;
    GmWs w;
    gm_layout(&w, ws, cap_b, HW);
    if (launch_zero(w.hist, (size_t)cap_b * (GM_SMAX + 1) * 4, st)) return -1;
    {
        ProfScope prof("gms_assign", (double)B * HW * 17.0, 10.0 * B * (double)HW * S, st);
        hipLaunchKernelGGL(gm_assign_kernel, dim3((unsigned)((HW + 255) / 256), B), dim3(256), 0, st, votes, fg, Z, seed_labels, counts, HW, S, w.raw,
                           w.hist);
        QB_CHECK(hipGetLastError());
    }
    ProfScope prof("gms_write", (double)B * HW * (N + 8.0), 0.0, st);
    hipLaunchKernelGGL(gm_finish_kernel, dim3(B), dim3(GM_SMAX), 0, st, Z, seed_labels, counts, w.hist, S, N, min_pixels, w.table, centers, report);
    gm_write(w.raw, w.table, B, N, HW, planes, ids, st);
    QB_CHECK(hipGetLastError());
    return 0;
}

static GmElem gm_ellipse(int k) {            // cv2.getStructuringElement(MORPH_ELLIPSE, (k, k)): the half width of row dy
    GmElem e;
    const int r = k / 2, c = k / 2;
    const double inv = r ? 1.0 / ((double)r * r) : 0.0;
    e.r = r;
    for (int i = 0; i < GM_KMAX; ++i) e.hw[i] = 0;
    for (int dy = -r; dy <= r; ++dy) e.hw[dy + r] = (int)std::nearbyint(c * std::sqrt(((double)r * r - (double)dy * dy) * inv));
    return e;
}

size_t gms_imp_lds_bytes(int H, int W) { return 2 * (size_t)H * ((W + 31) / 32) * 4; }

// ids i32 [B][H][W] in place (0, 1..n_ids); planes u8 [B][N][H][W], centers f32 [B][n_ids][3], report i32 [B][6]: each may be null.
// cleanup_ws: the connected-component workspace of the context (launch_cleanup_ids)
int launch_gms_imp(int* ids, int B, int n_ids, int ksize, int largest, int N, int H, int W, uint8_t* planes, float* centers, int* report, void* ws,
                   int cap_b, void* cleanup_ws, hipStream_t st) {
    if (B <= 0 || B > cap_b || B > 65535) return fail("gms imp: batch outside 1..max_batch");
    if (H < 1 || W < 1 || (long)H * W > (1L << 24)) return fail("gms imp: a frame that is empty or has more than 2^24 pixels");
    if (n_ids < 0 || n_ids > GM_NMAX) return fail("gms imp: n_ids outside 0..254");
    if (N < 0 || N > GM_NMAX || (N > 0 && !planes)) return fail("gms imp: n_masks outside 0..254, or no planes to write them to");
    if (ksize < 1 || ksize > GM_KMAX || !(ksize & 1)) return fail("gms imp: ksize must be odd and lie in 1..15");
    if (largest != 0 && largest != 1) return fail("gms imp: largest must be 0 or 1");
    if (!ids || !ws) return fail("gms imp: null tensor");
    if (((uintptr_t)ids & 3) || ((uintptr_t)centers & 3) || ((uintptr_t)report & 3)) return fail("gms imp: a 32-bit tensor that is not 4-byte aligned");
    const size_t lds = gms_imp_lds_bytes(H, W);
    if (lds > GM_LDS_MAX) return fail("gms imp: the two bit planes of a frame do not fit the LDS (2 * H * ceil(W / 32) * 4 bytes > 152 KiB)");
    const long HW = (long)H * W;
    GmWs w;
    gm_layout(&w, ws, cap_b, HW);
    unsigned *before = w.flags, *after = w.flags + (size_t)cap_b * 8;
    if (launch_zero(after, (size_t)cap_b * 8 * 4, st)) return -1;
    {
        ProfScope prof("gms_imp", (double)B * HW * 8.0 * (n_ids + 1), 0.0, st);
        hipLaunchKernelGGL(gm_imp_kernel, dim3(B), dim3(1024), lds, st, ids, n_ids, H, W, (W + 31) / 32, gm_ellipse(ksize), before);
        QB_CHECK(hipGetLastError());
    }
    if (largest && launch_cleanup_ids(ids, B, H, W, n_ids, 4, 1, 0, 0, cleanup_ws, nullptr, st)) return -1;
    ProfScope prof("gms_imp_write", (double)B * HW * (N + 12.0), 0.0, st);
    hipLaunchKernelGGL(gm_present_kernel, dim3((unsigned)((HW + 255) / 256), B), dim3(256), 0, st, ids, HW, n_ids, after);
    hipLaunchKernelGGL(gm_imp_finish_kernel, dim3(B), dim3(GM_SMAX), 0, st, before, after, n_ids, w.table, centers, report);
    gm_write(ids, w.table, B, N, HW, planes, ids, st);
    QB_CHECK(hipGetLastError());
    return 0;
}

int launch_gms_copy_ids(const int* src, int* dst, size_t n, hipStream_t st) {
    hipLaunchKernelGGL(gm_copy_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, dst, n);
    QB_CHECK(hipGetLastError());
    return 0;
}

}  // namespace quber
