// Scene-level mask perturbation on the device (include/quber_hip.h: quber_scene_perturb; the definition is in INTEGRATION.md "Scene-level
// perturbation" and, as numpy, in tests/test_scene_cpu.py: scene_perturb_np).  Restates the list stage of the reference's
// tools/ours/perturbate_masks.py:101-205: false positives and over- / under-segmentations from a pool of proposals, the ground truths no
// entry covers, merging of masks within the reach of a 10 x 10 dilation, splits along an axis-aligned line, deletions.  Every random
// decision arrives as a table drawn on the host (quber_amd/scene.py: scene_draws); the device executes it.
//
// A zero-fill kernel and nine stream-ordered steps, no host copy, no memset node, no floating-point atomics:
//   pack     the N + P sources (ground truths, then proposals) -> bit planes (bitplane.h); a row behind the frame's n_gt / n_prop is
//            never read, its plane is written as zero.
//   gram     inter[b][i][j], i <= j, over the sources with bitplane.h's pair tile: a block owns a 16 x 16 tile of pairs and a chunk of
//            SC_CHUNK words and adds its counts (integer atomics) into a table that launch_zero cleared; the areas are the diagonal.
//   select   one workgroup per frame runs steps 1-3 from the table: thread q judges proposal q (float64: (I + 1e-6) / (U + 1e-6)),
//            thread g ground truth g ((I + 1e-6) / ((U - I) + 1e-6), the reference's wrapped union), positions by counting.
//   dilate   the 10 x 10 dilation (anchor (5, 5): an output pixel sees the inputs 5 before .. 4 after it) of every entry's plane: the
//            rows y - 5 .. y + 4 ORed, then the shifts by -5 .. +4 bits with carries from both neighbour words.
//   touch    touch[b][a][c] = dilate10(L_a) meets L_c, the pair tile again with a non-zero test: a block that finds a common pixel in its
//            chunk stores 1 into the cleared table.
//   merge    one workgroup per frame runs the sequential merge on 256-bit member sets in LDS: per turn the reach of the snapshot's
//            members (an OR of touch rows), every other slot tests its members against it in parallel, the LAST hit stays merged.
//   compose  per slot the union of its members' planes, its area, and the prefix sums of its row and column counts.
//   decide   one workgroup per frame: empty entries drop out, every entry with a split takes the first of its ten attempts whose halves
//            both reach the limit (two lookups per attempt), a count of the successful splits places the cut-off halves, deletions,
//            compaction -> per output mask (slot, half, cut), info, report.
//   write    every output plane as bytes, 0 / 255, zero planes behind count.
// Planes and tables live in device memory; LDS holds the pair tile and per-frame tables of at most SC_MAX entries: any frame size.
#include "bitplane.h"       // mn_plane_words, mn_pack_word, mn_gram_tile
#include "common.h"

namespace quber {

constexpr int SC_MAX = 256;                  // sources (N + P) and list capacity M: one thread of a per-frame workgroup per slot
constexpr int SC_T = 256;
constexpr int SC_TILE = 16, SC_SLAB = 64, SC_PITCH = SC_SLAB + 4;      // the pair tile of masknms.hip
constexpr int SC_CHUNK = 1024;               // words of a plane per gram / touch block: SC_CHUNK / SC_SLAB steps
constexpr int SC_ATTEMPTS = 10;
static_assert(SC_CHUNK % SC_SLAB == 0, "a chunk is whole slabs");
constexpr int SC_CNT = 8;                    // per-frame counters: L1, n_fp, n_gs, gt kept, dropped in steps 1-3, absorbed
constexpr int SC_FIN = 8;                    // per output mask: slot, mode (-1 none, 0 whole, 1 kept half, 2 cut-off half), axis, side, line

struct ScWs {
    unsigned* src;        // [B][S][pw]
    unsigned* inter;      // [B][S][S]; cleared together with touch, which follows it
    unsigned* dil;        // [B][M][pw]
    unsigned* comp;       // [B][M][pw]
    unsigned* memb;       // [B][M][8]
    unsigned* area;       // [B][M]
    uint8_t* touch;       // [B][M][M]
    size_t zero_bytes;    // inter and touch
    int* ent;             // [B][M][2]: source, kind
    int* cnt;             // [B][SC_CNT]
    int* rowpre;          // [B][M][H + 1]
    int* colpre;          // [B][M][W + 1]
    int* fin;             // [B][M][SC_FIN]
};

static size_t sc_layout(ScWs* out, void* ws, int B, int S, int M, int H, int W) {
    const size_t pw = (size_t)mn_plane_words(H, W), b = (size_t)B, s = (size_t)(S > 0 ? S : 1), m = (size_t)M;
    ScWs none, &r = out ? *out : none;
    WsWalk w{static_cast<char*>(ws)};
    r.src = w.take<unsigned>(b * s * pw);
    const size_t inter_bytes = ws_align(b * s * s * 4);             // touch starts on a boundary of its own
    r.zero_bytes = inter_bytes + ws_align(b * m * m);
    r.inter = reinterpret_cast<unsigned*>(w.take<uint8_t>(r.zero_bytes));
    r.touch = r.inter ? reinterpret_cast<uint8_t*>(r.inter) + inter_bytes : nullptr;
    r.dil = w.take<unsigned>(b * m * pw);
    r.comp = w.take<unsigned>(b * m * pw);
    r.memb = w.take<unsigned>(b * m * 8);
    r.area = w.take<unsigned>(b * m);
    r.ent = w.take<int>(b * m * 2);
    r.cnt = w.take<int>(b * SC_CNT);
    r.rowpre = w.take<int>(b * m * (size_t)(H + 1));
    r.colpre = w.take<int>(b * m * (size_t)(W + 1));
    r.fin = w.take<int>(b * m * SC_FIN);
    return w.off;
}

size_t scene_ws_bytes(int B, int S, int M, int H, int W) { return sc_layout(nullptr, nullptr, B, S, M, H, W); }
int scene_max() { return SC_MAX; }

__device__ __forceinline__ int sc_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

// grid (ceil(pw / 256), S, B).  Source s < N: ground truth s, else proposal s - N; absent rows and the plane's padding -> zero words.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void sc_pack_kernel(const uint8_t* __restrict__ gt, const uint8_t* __restrict__ props,
                                                      const int* __restrict__ n_gt, const int* __restrict__ n_prop, int N, int P, int H, int W,
                                                      int wpr, int pw, unsigned* __restrict__ planes) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= pw) return;
    const int s = blockIdx.y, b = blockIdx.z, S = N + P;
    const size_t HW = (size_t)H * W;
    const bool present = s < N ? s < sc_clamp(n_gt[b], 0, N) : s - N < sc_clamp(n_prop[b], 0, P);
    unsigned bits = 0;
    if (present && i < H * wpr) {
        const uint8_t* m = s < N ? gt + ((size_t)b * N + s) * HW : props + ((size_t)b * P + (s - N)) * HW;
        bits = mn_pack_word<ALIGNED>(m, i, W, wpr);
    }
    planes[((size_t)b * S + s) * pw + i] = bits;
}

// grid (nt (nt + 1) / 2 tile pairs, ceil(pw / SC_CHUNK), B), 256 lanes.  inter u32 [B][S][S], zero on entry; only i <= j is written.
__global__ __launch_bounds__(256) void sc_gram_kernel(const unsigned* __restrict__ planes, unsigned* __restrict__ inter, int S, int pw) {
    __shared__ uint4 sm4[2 * SC_TILE * SC_PITCH / 4];
    unsigned* sm = reinterpret_cast<unsigned*>(sm4);
    const int nt = (S + SC_TILE - 1) / SC_TILE;
    int ta = 0, rem = blockIdx.x;
    while (rem >= nt - ta) { rem -= nt - ta; ++ta; }         // (bounded: blockIdx.x < nt (nt + 1) / 2)
    const int tb = ta + rem;
    const int t = threadIdx.x, b = blockIdx.z;
    const int w0 = blockIdx.y * SC_CHUNK, w1 = min(w0 + SC_CHUNK, pw);
    const unsigned* base = planes + (size_t)b * S * pw;
    const int srow = t >> 4, ma = ta * SC_TILE + srow, mb = tb * SC_TILE + srow;
    const unsigned acc = mn_gram_tile<SC_TILE, SC_SLAB, SC_PITCH>(ma < S ? base + (size_t)ma * pw : nullptr, mb < S ? base + (size_t)mb * pw : nullptr,
                                                                  w0, w1, sm);
    const int i = ta * SC_TILE + (t >> 4), j = tb * SC_TILE + (t & 15);
    if (i <= j && j < S && acc) atomicAdd(inter + ((size_t)b * S + i) * S + j, acc);
}

// grid (B), SC_T lanes.  Steps 1-3 -> ent i32 [B][M][2] (source, kind; zero behind L1), cnt[b][0..4].
__global__ __launch_bounds__(SC_T) void sc_select_kernel(const unsigned* __restrict__ inter, const int* __restrict__ n_gt,
                                                         const int* __restrict__ n_prop, const uint8_t* __restrict__ fp_act,
                                                         const uint8_t* __restrict__ gs_act, int N, int P, int M, double lim,
                                                         int* __restrict__ ent, int* __restrict__ cnt) {
    __shared__ unsigned s_area[SC_MAX];
    __shared__ uint8_t s_fp[SC_MAX], s_gs[SC_MAX], s_in[SC_MAX], s_keep[SC_MAX];
    const int t = threadIdx.x, b = blockIdx.x, S = N + P;
    const int ng = sc_clamp(n_gt[b], 0, N), np = sc_clamp(n_prop[b], 0, P);
    const unsigned* I = inter + (size_t)b * S * S;
    if (t < S) s_area[t] = I[(size_t)t * S + t];
    s_fp[t] = s_gs[t] = s_in[t] = s_keep[t] = 0;
    __syncthreads();
    unsigned max_g = 0;
    for (int g = 0; g < ng; ++g) max_g = max(max_g, s_area[g]);
    if (t < np) {
        const unsigned aq = s_area[N + t];
        double max_iou = 0.0;
        for (int g = 0; g < ng; ++g) {
            const unsigned in = I[(size_t)g * S + N + t];
            const unsigned un = s_area[g] + aq - in;
            max_iou = fmax(max_iou, ((double)in + 1e-6) / ((double)un + 1e-6));
        }
        const bool small = (double)aq < lim, large = (double)aq > 2.0 * (double)max_g;
        s_fp[t] = fp_act[(size_t)b * P + t] && !(small || large) && max_iou < 0.3;
        s_gs[t] = gs_act[(size_t)b * P + t] && !small && max_iou > 0.3;
    }
    __syncthreads();
    int fp_all = 0, gs_all = 0, fp_before = 0, gs_before = 0;
    for (int q = 0; q < np; ++q) {
        fp_all += s_fp[q]; gs_all += s_gs[q];
        if (q < t) { fp_before += s_fp[q]; gs_before += s_gs[q]; }
    }
    int* E = ent + (size_t)b * M * 2;
    if (t < np) {
        if (s_fp[t] && fp_before < M) { E[2 * fp_before] = N + t; E[2 * fp_before + 1] = 1; s_in[t] = 1; }
        const int pos = fp_all + gs_before;
        if (s_gs[t] && pos < M) { E[2 * pos] = N + t; E[2 * pos + 1] = 2; s_in[t] = 1; }
    }
    const int n_fp = min(fp_all, M), n_gs = min(gs_all, M - n_fp), L12 = n_fp + n_gs;
    __syncthreads();
    if (t < ng) {
        const unsigned ag = s_area[t];
        double max_iou = 0.0;
        for (int q = 0; q < np; ++q) {
            if (!s_in[q]) continue;
            const long long in = I[(size_t)t * S + N + q];
            const long long sym = (long long)ag + (long long)s_area[N + q] - 2 * in;           // |G u E| - |G n E|
            max_iou = fmax(max_iou, ((double)in + 1e-6) / ((double)sym + 1e-6));
        }
        s_keep[t] = max_iou < 0.3;
    }
    __syncthreads();
    int keep_all = 0, keep_before = 0;
    for (int g = 0; g < ng; ++g) {
        keep_all += s_keep[g];
        if (g < t) keep_before += s_keep[g];
    }
    if (t < ng && s_keep[t] && L12 + keep_before < M) { E[2 * (L12 + keep_before)] = t; E[2 * (L12 + keep_before) + 1] = 0; }
    const int kept = min(keep_all, M - L12), L1 = L12 + kept;
    if (t < M && t >= L1) { E[2 * t] = 0; E[2 * t + 1] = 0; }
    if (t == 0) {
        int* c = cnt + (size_t)b * SC_CNT;
        c[0] = L1; c[1] = n_fp; c[2] = n_gs; c[3] = kept; c[4] = (fp_all + gs_all - L12) + (keep_all - kept); c[5] = 0; c[6] = 0; c[7] = 0;
    }
}

// grid (ceil(pw / 256), M, B).  dil[b][k] = dilate10 of the plane of entry k < L1 (the padding words zero).
__global__ __launch_bounds__(256) void sc_dilate_kernel(const unsigned* __restrict__ src, const int* __restrict__ ent, const int* __restrict__ cnt,
                                                        int S, int M, int H, int wpr, int pw, unsigned* __restrict__ dil) {
    const int i = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y, b = blockIdx.z;
    if (i >= pw || k >= sc_clamp(cnt[(size_t)b * SC_CNT], 0, M)) return;
    const int s = sc_clamp(ent[((size_t)b * M + k) * 2], 0, S - 1);
    const unsigned* plane = src + ((size_t)b * S + s) * pw;
    unsigned out = 0;
    if (i < H * wpr) {
        const int y = i / wpr, j = i - y * wpr;
        unsigned c = 0, l = 0, r = 0;
        for (int yy = max(y - 5, 0); yy <= min(y + 4, H - 1); ++yy) {
            const unsigned* row = plane + (size_t)yy * wpr;
            c |= row[j];
            if (j > 0) l |= row[j - 1];
            if (j + 1 < wpr) r |= row[j + 1];
        }
        out = c;
#pragma unroll
        for (int d = 1; d <= 4; ++d) out |= (c >> d) | (r << (32 - d));      // output bit x sees input bit x + d
#pragma unroll
        for (int d = 1; d <= 5; ++d) out |= (c << d) | (l >> (32 - d));      // ... and input bit x - d
    }
    dil[((size_t)b * M + k) * pw + i] = out;
}

// grid (nt * nt, ceil(pw / SC_CHUNK), B), nt = ceil(M / 16), 256 lanes.  touch u8 [B][M][M], zero on entry: 1 is stored where a, c < L1 meet.
__global__ __launch_bounds__(256) void sc_touch_kernel(const unsigned* __restrict__ dil, const unsigned* __restrict__ src, const int* __restrict__ ent,
                                                       const int* __restrict__ cnt, int S, int M, int pw, uint8_t* __restrict__ touch) {
    __shared__ uint4 sm4[2 * SC_TILE * SC_PITCH / 4];
    unsigned* sm = reinterpret_cast<unsigned*>(sm4);
    const int nt = (M + SC_TILE - 1) / SC_TILE, ta = blockIdx.x / nt, tb = blockIdx.x - ta * nt;
    const int t = threadIdx.x, b = blockIdx.z;
    const int w0 = blockIdx.y * SC_CHUNK, w1 = min(w0 + SC_CHUNK, pw);
    const int L1 = sc_clamp(cnt[(size_t)b * SC_CNT], 0, M);
    if (ta * SC_TILE >= L1 || tb * SC_TILE >= L1) return;     // (the whole block: L1 is the frame's)
    const int srow = t >> 4, a = ta * SC_TILE + srow, c = tb * SC_TILE + srow;
    const unsigned* row_a = a < L1 ? dil + ((size_t)b * M + a) * pw : nullptr;
    const unsigned* row_b = c < L1 ? src + ((size_t)b * S + sc_clamp(ent[((size_t)b * M + c) * 2], 0, S - 1)) * pw : nullptr;
    const unsigned acc = mn_gram_tile<SC_TILE, SC_SLAB, SC_PITCH>(row_a, row_b, w0, w1, sm);
    const int i = ta * SC_TILE + (t >> 4), j = tb * SC_TILE + (t & 15);
    if (i < L1 && j < L1 && acc) touch[((size_t)b * M + i) * M + j] = 1;
}

// grid (B), SC_T lanes.  The sequential merge on member sets -> memb u32 [B][M][8], cnt[b][5] = absorbed.
__global__ __launch_bounds__(SC_T) void sc_merge_kernel(const uint8_t* __restrict__ touch, const uint8_t* __restrict__ merge_act,
                                                        int* __restrict__ cnt, int M, unsigned* __restrict__ memb) {
    __shared__ unsigned s_T[SC_MAX][8];          // row a: the slots dilate10(L_a) meets
    __shared__ unsigned s_S[SC_MAX][8];          // the member set of every slot
    __shared__ unsigned s_R[8];
    __shared__ uint8_t s_act[SC_MAX];
    __shared__ int s_last, s_hits;
    const int t = threadIdx.x, b = blockIdx.x;
    const int L1 = sc_clamp(cnt[(size_t)b * SC_CNT], 0, M);
    for (int w = 0; w < 8; ++w) {
        unsigned bits = 0;
        if (t < L1)
            for (int k = 0; k < 32; ++k) {
                const int c = w * 32 + k;
                if (c < L1 && touch[((size_t)b * M + t) * M + c]) bits |= 1u << k;
            }
        s_T[t][w] = bits;
        s_S[t][w] = (t < L1 && (t >> 5) == w) ? 1u << (t & 31) : 0u;
    }
    s_act[t] = t < L1 ? merge_act[(size_t)b * M + t] : 0;
    __syncthreads();
    int absorbed = 0;
    for (int idx1 = 0; idx1 < L1; ++idx1) {
        if (!s_act[idx1]) continue;                          // (uniform: read from LDS written before a barrier)
        if (t < 8) {                                         // the reach of the snapshot A = S[idx1]
            unsigned r = 0;
            for (int w = 0; w < 8; ++w) {
                unsigned a = s_S[idx1][w];
                while (a) {
                    const int m = w * 32 + __ffs(a) - 1;
                    a &= a - 1;
                    r |= s_T[m][t];
                }
            }
            s_R[t] = r;
        }
        if (t == 0) { s_last = -1; s_hits = 0; }
        __syncthreads();
        bool hit = false;
        if (t < L1 && t != idx1) {
            unsigned any = 0;
            for (int w = 0; w < 8; ++w) any |= s_R[w] & s_S[t][w];
            hit = any != 0;
            if (hit) { atomicMax(&s_last, t); atomicAdd(&s_hits, 1); }
        }
        __syncthreads();
        const int last = s_last;
        absorbed += s_hits;
        unsigned merged = 0;
        if (last >= 0 && t < 8) merged = s_S[idx1][t] | s_S[last][t];      // replaces: only the last hit stays merged
        __syncthreads();
        if (hit)
            for (int w = 0; w < 8; ++w) s_S[t][w] = 0;
        if (last >= 0 && t < 8) s_S[idx1][t] = merged;
        __syncthreads();
    }
    if (t < M)
        for (int w = 0; w < 8; ++w) memb[((size_t)b * M + t) * 8 + w] = s_S[t][w];
    if (t == 0) cnt[(size_t)b * SC_CNT + 5] = absorbed;
}

// In-place exclusive-to-inclusive scan of the counts stored at arr[1 .. n] (arr[0] becomes 0); every lane of the block calls it.
__device__ __forceinline__ void sc_block_scan(int* arr, int n, int* s_part) {
    const int t = threadIdx.x, chunk = (n + SC_T - 1) / SC_T;
    const int i0 = min(t * chunk, n), i1 = min(i0 + chunk, n);
    int sum = 0;
    for (int i = i0; i < i1; ++i) sum += arr[1 + i];
    __syncthreads();                                         // (s_part's previous readers are done)
    s_part[t] = sum;
    __syncthreads();
    int run = 0;
    for (int q = 0; q < t; ++q) run += s_part[q];
    for (int i = i0; i < i1; ++i) { run += arr[1 + i]; arr[1 + i] = run; }
    if (t == 0) arr[0] = 0;
}

// grid (M, B), SC_T lanes.  Slot k < L1 with members: comp[b][k] = the union of their planes, area, rowpre / colpre (prefix sums of the
// row and column counts: rowpre[y] = pixels in the rows < y).  Any other slot: area 0.
__global__ __launch_bounds__(SC_T) void sc_compose_kernel(const unsigned* __restrict__ src, const int* __restrict__ ent, const int* __restrict__ cnt,
                                                          const unsigned* __restrict__ memb, int S, int M, int H, int W, int wpr, int pw,
                                                          unsigned* __restrict__ comp, unsigned* __restrict__ area, int* __restrict__ rowpre,
                                                          int* __restrict__ colpre) {
    __shared__ int s_list[SC_MAX];
    __shared__ int s_part[SC_T];
    __shared__ int s_n;
    __shared__ unsigned s_total;
    const int t = threadIdx.x, k = blockIdx.x, b = blockIdx.y;
    const int L1 = sc_clamp(cnt[(size_t)b * SC_CNT], 0, M);
    if (t == 0) {
        int n = 0;
        if (k < L1)
            for (int w = 0; w < 8; ++w) {
                unsigned a = memb[((size_t)b * M + k) * 8 + w];
                while (a) {
                    const int m = w * 32 + __ffs(a) - 1;
                    a &= a - 1;
                    if (m < L1) s_list[n++] = sc_clamp(ent[((size_t)b * M + m) * 2], 0, S - 1);
                }
            }
        s_n = n;
        s_total = 0;
    }
    __syncthreads();
    const int n = s_n;
    if (n == 0) {                                            // (the whole block)
        if (t == 0) area[(size_t)b * M + k] = 0;
        return;
    }
    unsigned* out = comp + ((size_t)b * M + k) * pw;
    const unsigned* base = src + (size_t)b * S * pw;
    unsigned total = 0;
    for (int i = t; i < pw; i += SC_T) {
        unsigned u = 0;
        for (int m = 0; m < n; ++m) u |= base[(size_t)s_list[m] * pw + i];
        out[i] = u;
        total += __popc(u);
    }
    if (total) atomicAdd(&s_total, total);
    __syncthreads();                                         // the block's writes of `out` are visible to the block
    int* rp = rowpre + ((size_t)b * M + k) * (H + 1);
    int* cp = colpre + ((size_t)b * M + k) * (W + 1);
    for (int y = t; y < H; y += SC_T) {
        int c = 0;
        for (int j = 0; j < wpr; ++j) c += __popc(out[(size_t)y * wpr + j]);
        rp[1 + y] = c;
    }
    for (int x = t; x < W; x += SC_T) {
        int c = 0;
        const unsigned* col = out + (x >> 5);
        for (int y = 0; y < H; ++y) c += (col[(size_t)y * wpr] >> (x & 31)) & 1u;
        cp[1 + x] = c;
    }
    if (t == 0) area[(size_t)b * M + k] = s_total;
    __syncthreads();
    sc_block_scan(rp, H, s_part);
    sc_block_scan(cp, W, s_part);
}

// grid (B), SC_T lanes.  Empty entries drop out, splits, deletions, compaction -> fin i32 [B][M][SC_FIN], info i32 [B][M][4], report i32 [B][8].
__global__ __launch_bounds__(SC_T) void sc_decide_kernel(const int* __restrict__ ent, const int* __restrict__ cnt, const unsigned* __restrict__ memb,
                                                         const unsigned* __restrict__ area, const int* __restrict__ rowpre,
                                                         const int* __restrict__ colpre, const uint8_t* __restrict__ split_act,
                                                         const int* __restrict__ split_try, const uint8_t* __restrict__ delete_act, int N, int M,
                                                         int H, int W, double lim, int* __restrict__ fin, int* __restrict__ info,
                                                         int* __restrict__ report) {
    __shared__ uint8_t s_alive[SC_MAX], s_valid[SC_MAX], s_del[SC_MAX];
    __shared__ int s_slot[SC_MAX], s_mode[SC_MAX], s_cut[SC_MAX];       // by position in the list after the splits
    const int t = threadIdx.x, b = blockIdx.x;
    const int* c = cnt + (size_t)b * SC_CNT;
    const int L1 = sc_clamp(c[0], 0, M);
    const unsigned my_area = t < L1 ? area[(size_t)b * M + t] : 0u;
    s_alive[t] = my_area > 0;
    s_valid[t] = 0;
    __syncthreads();
    int idx = 0, L2 = 0;
    for (int q = 0; q < L1; ++q) {
        L2 += s_alive[q];
        if (q < t) idx += s_alive[q];
    }
    int cut = 0;                                             // axis | side << 1 | line << 2
    bool valid = false;
    if (s_alive[t] && split_act[(size_t)b * M + idx]) {
        const int* rp = rowpre + ((size_t)b * M + t) * (H + 1);
        const int* cp = colpre + ((size_t)b * M + t) * (W + 1);
        for (int a = 0; a < SC_ATTEMPTS && !valid; ++a) {
            const int* tr = split_try + (((size_t)b * M + idx) * SC_ATTEMPTS + a) * 4;
            const int x1 = sc_clamp(tr[0], 0, W - 1), y1 = sc_clamp(tr[1], 0, H - 1), axis = tr[2] != 0, side = tr[3] != 0;
            const int n2 = axis == 0 ? (side == 0 ? rp[H - 1] - rp[y1] : rp[y1]) : (side == 0 ? cp[W - 1] - cp[x1] : cp[x1]);
            const int n1 = (int)my_area - n2;
            if (255.0 * (double)n1 >= lim && 255.0 * (double)n2 >= lim) {
                valid = true;
                cut = axis | side << 1 | (axis == 0 ? y1 : x1) << 2;
            }
        }
        s_valid[idx] = valid;
    }
    __syncthreads();
    int rank = 0, n_valid = 0;
    for (int q = 0; q < L2; ++q) {
        n_valid += s_valid[q];
        if (q < idx) rank += s_valid[q];
    }
    const int splits = min(n_valid, M - L2), L3 = L2 + splits;
    const bool performed = valid && rank < M - L2;
    if (s_alive[t]) {
        s_slot[idx] = t; s_mode[idx] = performed ? 1 : 0; s_cut[idx] = cut;
        if (performed) { s_slot[L2 + rank] = t; s_mode[L2 + rank] = 2; s_cut[L2 + rank] = cut; }
    }
    s_del[t] = t < L3 ? delete_act[(size_t)b * M + t] != 0 : 0;
    __syncthreads();
    int o = 0, deleted = 0;
    for (int q = 0; q < L3; ++q) {
        deleted += s_del[q];
        if (q < t) o += !s_del[q];
    }
    const int count = L3 - deleted;
    int* F = fin + (size_t)b * M * SC_FIN;
    int* R = info + (size_t)b * M * 4;
    if (t < L3 && !s_del[t]) {
        const int k = s_slot[t], src = ent[((size_t)b * M + k) * 2], kind = ent[((size_t)b * M + k) * 2 + 1];
        int members = 0;
        for (int w = 0; w < 8; ++w) members += __popc(memb[((size_t)b * M + k) * 8 + w]);
        F[o * SC_FIN] = k; F[o * SC_FIN + 1] = s_mode[t]; F[o * SC_FIN + 2] = s_cut[t] & 1; F[o * SC_FIN + 3] = (s_cut[t] >> 1) & 1;
        F[o * SC_FIN + 4] = s_cut[t] >> 2;
        R[o * 4] = kind; R[o * 4 + 1] = kind == 0 ? src : src - N; R[o * 4 + 2] = members; R[o * 4 + 3] = s_mode[t];
    }
    if (t < M && t >= count) {
        F[t * SC_FIN] = 0; F[t * SC_FIN + 1] = -1; F[t * SC_FIN + 2] = 0; F[t * SC_FIN + 3] = 0; F[t * SC_FIN + 4] = 0;
        R[t * 4] = 0; R[t * 4 + 1] = 0; R[t * 4 + 2] = 0; R[t * 4 + 3] = 0;
    }
    if (t == 0) {
        int* rep = report + (size_t)b * 8;
        rep[0] = count; rep[1] = c[1]; rep[2] = c[2]; rep[3] = c[3]; rep[4] = c[5]; rep[5] = splits; rep[6] = deleted;
        rep[7] = c[4] + (n_valid - splits);
    }
}

// grid (ceil(HW / (256 * PIX)), M, B).  PIX = 16: W % 16 == 0 and a 16-byte aligned output, 16 pixels of one row per lane and store.
template <int PIX>
__global__ __launch_bounds__(256) void sc_write_kernel(const unsigned* __restrict__ comp, const int* __restrict__ fin, int M, int H, int W, int wpr,
                                                       int pw, uint8_t* __restrict__ out) {
    const int o = blockIdx.y, b = blockIdx.z;
    const size_t HW = (size_t)H * W, p = ((size_t)blockIdx.x * 256 + threadIdx.x) * PIX;
    if (p >= HW) return;
    const int* F = fin + ((size_t)b * M + o) * SC_FIN;
    const int k = sc_clamp(F[0], 0, M - 1), mode = F[1], axis = F[2], side = F[3], line = F[4];
    const int y = (int)(p / W), x0 = (int)(p - (size_t)y * W);
    unsigned bits = 0;
    if (mode >= 0) bits = (comp[((size_t)b * M + k) * pw + (size_t)y * wpr + (x0 >> 5)] >> (x0 & 31)) & (PIX == 16 ? 0xffffu : 1u);
    if (mode > 0) {
        unsigned in_cut;                                     // per pixel: inside the cut region
        if (axis == 0)
            in_cut = (side == 0 ? (y >= line && y < H - 1) : y < line) ? 0xffffu : 0u;
        else {
            in_cut = 0;
#pragma unroll
            for (int q = 0; q < PIX; ++q) {
                const int x = x0 + q;
                in_cut |= (unsigned)(side == 0 ? (x >= line && x < W - 1) : x < line) << q;
            }
        }
        bits &= mode == 1 ? ~in_cut : in_cut;
    }
    uint8_t* dst = out + ((size_t)b * M + o) * HW + p;
    if (PIX == 16) {
        unsigned w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            w[q] = ((bits >> (4 * q)) & 1u ? 0xffu : 0u) | ((bits >> (4 * q + 1)) & 1u ? 0xff00u : 0u) | ((bits >> (4 * q + 2)) & 1u ? 0xff0000u : 0u) |
                   ((bits >> (4 * q + 3)) & 1u ? 0xff000000u : 0u);
        *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        *dst = bits & 1u ? 255 : 0;
    }
}

// ws: scene_ws_bytes(B, N + P, M, H, W) bytes.
int launch_scene_perturb(const ScenePerturbArgs& q, int B, int H, int W, void* ws_mem, hipStream_t st) {
    if (B <= 0) return 0;
    const int N = q.N, P = q.P, M = q.M, S = N + P;
    if (H < 1 || W < 1 || (long)H * W > (1L << 30)) return fail("scene perturb: an empty frame, or one of more than 2^30 pixels");
    if (N < 0 || P < 0 || S > SC_MAX) return fail("scene perturb: n_gt_rows + n_prop_rows outside 0..256");
    if (M < 1 || M > SC_MAX) return fail("scene perturb: max_masks outside 1..256");
    if (!(q.min_mask_ratio >= 0.0 && q.min_mask_ratio <= 1.0)) return fail("scene perturb: min_mask_ratio outside 0..1");
    if (!q.n_gt || !q.n_prop || !q.merge_act || !q.split_act || !q.split_try || !q.delete_act || !q.out_masks || !q.info || !q.report || !ws_mem ||
        (N > 0 && !q.gt) || (P > 0 && (!q.props || !q.fp_act || !q.gs_act)))
        return fail("scene perturb: null tensor");
    if (((uintptr_t)q.n_gt & 3) || ((uintptr_t)q.n_prop & 3) || ((uintptr_t)q.split_try & 3) || ((uintptr_t)q.info & 3) || ((uintptr_t)q.report & 3))
        return fail("scene perturb: a 32-bit tensor that is not 4-byte aligned");
    const int wpr = (W + 31) / 32, pw = (int)mn_plane_words(H, W);
    const long HW = (long)H * W;
    const double lim = (double)HW * q.min_mask_ratio;
    ScWs w;
    sc_layout(&w, ws_mem, B, S, M, H, W);
    const int Sk = S > 0 ? S : 1;                            // (S = 0: no source exists, L1 = 0 and no kernel below reads one)
    const int chunks = (pw + SC_CHUNK - 1) / SC_CHUNK;
    if (S > 0 && launch_zero(w.inter, w.zero_bytes, st)) return -1;
    if (S > 0) {
        ProfScope prof("scene_pack", (double)B * S * HW + 4.0 * B * S * pw, 0.0, st);
        const dim3 grid((pw + 255) / 256, (unsigned)S, (unsigned)B);
        const bool aligned = W % 16 == 0 && (N == 0 || ((uintptr_t)q.gt & 15) == 0) && (P == 0 || ((uintptr_t)q.props & 15) == 0);
        if (aligned)
            hipLaunchKernelGGL(sc_pack_kernel<true>, grid, dim3(256), 0, st, q.gt, q.props, q.n_gt, q.n_prop, N, P, H, W, wpr, pw, w.src);
        else
            hipLaunchKernelGGL(sc_pack_kernel<false>, grid, dim3(256), 0, st, q.gt, q.props, q.n_gt, q.n_prop, N, P, H, W, wpr, pw, w.src);
        QB_CHECK(hipGetLastError());
    }
    if (S > 0) {
        const int nt = (S + SC_TILE - 1) / SC_TILE;
        ProfScope prof("scene_gram", 4.0 * B * S * pw * (nt + 1) / 2.0, 0.0, st);
        hipLaunchKernelGGL(sc_gram_kernel, dim3(nt * (nt + 1) / 2, chunks, B), dim3(256), 0, st, w.src, w.inter, S, pw);
        QB_CHECK(hipGetLastError());
    }
    {
        ProfScope prof("scene_select", 4.0 * B * S * S, 0.0, st);
        hipLaunchKernelGGL(sc_select_kernel, dim3(B), dim3(SC_T), 0, st, w.inter, q.n_gt, q.n_prop, q.fp_act, q.gs_act, N, P, M, lim, w.ent, w.cnt);
        QB_CHECK(hipGetLastError());
    }
    const int mt = (M + SC_TILE - 1) / SC_TILE;
    if (S > 0) {
        ProfScope prof("scene_touch", 8.0 * B * M * pw + 8.0 * B * M * pw * mt, 0.0, st);
        hipLaunchKernelGGL(sc_dilate_kernel, dim3((pw + 255) / 256, M, B), dim3(256), 0, st, w.src, w.ent, w.cnt, Sk, M, H, wpr, pw, w.dil);
        hipLaunchKernelGGL(sc_touch_kernel, dim3(mt * mt, chunks, B), dim3(256), 0, st, w.dil, w.src, w.ent, w.cnt, Sk, M, pw, w.touch);
        QB_CHECK(hipGetLastError());
    }
    {
        ProfScope prof("scene_merge", 1.0 * B * M * M, 0.0, st);
        hipLaunchKernelGGL(sc_merge_kernel, dim3(B), dim3(SC_T), 0, st, w.touch, q.merge_act, w.cnt, M, w.memb);
        QB_CHECK(hipGetLastError());
    }
    {
        ProfScope prof("scene_compose", 8.0 * B * M * pw, 0.0, st);
        hipLaunchKernelGGL(sc_compose_kernel, dim3(M, B), dim3(SC_T), 0, st, w.src, w.ent, w.cnt, w.memb, Sk, M, H, W, wpr, pw, w.comp, w.area, w.rowpre,
                           w.colpre);
        QB_CHECK(hipGetLastError());
    }
    {
        ProfScope prof("scene_decide", 4.0 * B * M * 16, 0.0, st);
        hipLaunchKernelGGL(sc_decide_kernel, dim3(B), dim3(SC_T), 0, st, w.ent, w.cnt, w.memb, w.area, w.rowpre, w.colpre, q.split_act, q.split_try,
                           q.delete_act, N, M, H, W, lim, w.fin, q.info, q.report);
        QB_CHECK(hipGetLastError());
    }
    {
        ProfScope prof("scene_write", (double)B * M * HW + 4.0 * B * M * pw, 0.0, st);
        if (W % 16 == 0 && ((uintptr_t)q.out_masks & 15) == 0)
            hipLaunchKernelGGL(sc_write_kernel<16>, dim3((unsigned)((HW / 16 + 255) / 256), M, B), dim3(256), 0, st, w.comp, w.fin, M, H, W, wpr, pw,
                               q.out_masks);
        else
            hipLaunchKernelGGL(sc_write_kernel<1>, dim3((unsigned)((HW + 255) / 256), M, B), dim3(256), 0, st, w.comp, w.fin, M, H, W, wpr, pw, q.out_masks);
        QB_CHECK(hipGetLastError());
    }
    return 0;
}

}  // namespace quber
