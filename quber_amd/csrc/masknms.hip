// Mask NMS on the device (include/quber_hip.h: quber_mask_nms; the definition is in INTEGRATION.md "Overlapping initial masks" and, as
// numpy, in tests/test_masknms_cpu.py: mask_nms_np).  Restates the reference's nms + combine_masks_with_NMS (eval/refiner_model.py:
// 683-740, eval/base_model.py:1027-1086 and 1154-1190): greedy mask NMS in score order, the survivors painted into one label map in
// order of area, the masks `map == id` of the ids that are still visible.
//
// Five stream-ordered steps, no host copy, no memset node:
//   pack    masks u8 -> bit planes, 32-bit words, rows padded to whole words (bit k of word j of a row = pixel 32 j + k), every plane
//           padded with zero words to a multiple of 4 words so that the gram kernel stages it in 16-byte pieces.  One word per lane;
//           where the rows are 16-byte aligned the lane reads its 32 mask bytes as two 16-byte loads, else byte by byte.
//   gram    inter[b][i][j], i <= j: the pixels inside both masks, u32.  A block owns a MN_TILE x MN_TILE tile of mask pairs (tile row <=
//           tile column) and a chunk of MN_CHUNK words; it stages MN_SLAB words of its two groups of planes in LDS per step and every
//           lane accumulates ONE pair with popc in a register, reading 16 bytes per plane and LDS access.  LDS rows have a pitch of
//           MN_SLAB + 4 words: pitch / 4 is odd, so the 16 rows the lanes of one ds_read_b128 lane group can address start on 16
//           different 4-bank slots of the 64 banks; lanes on the same row read the same address (a broadcast).  One atomicAdd per
//           (block, pair) into a table that launch_zero cleared.  A plane word is read from memory once per tile of partners.
//   select  one workgroup per frame: visit order by counting (score descending, index descending - stable, no sort network), the
//           greedy pass with all lanes testing the partners of the current mask (float32, __fadd_rn / __fsub_rn / __fdiv_rn: the
//           contract's order of operations, no contraction, no approximate division), paint ranks by counting (area ascending, visit
//           position ascending; reversed for on_top = small).  The loop is bounded by N and has one barrier per step that every thread
//           reaches: which masks are alive is read from LDS words written before the previous barrier.
//   paint   per pixel the highest paint rank among the kept planes that cover it -> rank map (0 = none, else rank + 1), visible pixels
//           per rank counted in LDS and added once per (block, rank).
//   finish  a one-block compaction per frame of the ranks with visible pixels (by counting) -> source, scores, report, the table
//           rank -> output id; then one pass writes the id map and ALL N output planes (0 / 255; zero planes behind `count`).
// Integer and bit arithmetic except the one float32 expression; every output is overwritten by every call.
#include "bitplane.h"       // mn_plane_words, mn_pack_word, mn_gram_tile
#include "common.h"

namespace quber {

constexpr int MN_TILE = 16;                  // masks per side of a gram tile; MN_TILE * MN_TILE lanes per block
constexpr int MN_SLAB = 64;                  // words of every plane staged per step
constexpr int MN_PITCH = MN_SLAB + 4;        // LDS row pitch in words: a multiple of 4 (16-byte reads), pitch / 4 odd
constexpr int MN_CHUNK = 1024;               // words of a plane per gram block: MN_CHUNK / MN_SLAB steps
constexpr int MN_MAX = 1024;                 // masks per frame: one thread of the select / compaction workgroup per mask
constexpr int MN_T = 1024;
static_assert(MN_TILE * MN_TILE == 256 && MN_SLAB % 4 == 0 && (MN_PITCH / 4) % 2 == 1 && MN_CHUNK % MN_SLAB == 0, "gram tile layout");
static_assert(MN_TILE * (MN_SLAB / 4) == 256, "one 16-byte piece per lane stages a slab of one group");

// grid (ceil(pw / 256), B * N).  One word per lane; the words behind H * wpr (the plane's padding) are written as zero.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void mn_pack_kernel(const uint8_t* __restrict__ masks, unsigned* __restrict__ planes, int H, int W, int wpr,
                                                      int pw) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= pw) return;
    const size_t m = blockIdx.y;
    const unsigned bits = i < H * wpr ? mn_pack_word<ALIGNED>(masks + m * (size_t)H * W, i, W, wpr) : 0u;
    planes[m * (size_t)pw + i] = bits;
}

// grid (nt (nt + 1) / 2 tile pairs, ceil(pw / MN_CHUNK), B), 256 lanes.  Lane t owns the pair (row t / 16 of group A, row t % 16 of
// group B).  inter: u32 [B][N][N], zero on entry; only i <= j is written.
__global__ __launch_bounds__(256) void mn_gram_kernel(const unsigned* __restrict__ planes, unsigned* __restrict__ inter, int N, int pw) {
    __shared__ uint4 sm4[2 * MN_TILE * MN_PITCH / 4];
    unsigned* sm = reinterpret_cast<unsigned*>(sm4);
    // tile pair p -> (ta <= tb): row ta of the upper triangle holds nt - ta pairs
    const int nt = (N + MN_TILE - 1) / MN_TILE;
    int ta = 0, rem = blockIdx.x;
    while (rem >= nt - ta) { rem -= nt - ta; ++ta; }         // (bounded: blockIdx.x < nt (nt + 1) / 2)
    const int tb = ta + rem;
    const int t = threadIdx.x, b = blockIdx.z;
    const int w0 = blockIdx.y * MN_CHUNK, w1 = min(w0 + MN_CHUNK, pw);
    const unsigned* base = planes + (size_t)b * N * pw;
    // lane t stages row t / 16 of each group and owns the pair (row t / 16 of group A, row t % 16 of group B)
    const int srow = t >> 4, ma = ta * MN_TILE + srow, mb = tb * MN_TILE + srow;
    const int ra = t >> 4, rb = t & 15;
    const unsigned acc = mn_gram_tile<MN_TILE, MN_SLAB, MN_PITCH>(ma < N ? base + (size_t)ma * pw : nullptr, mb < N ? base + (size_t)mb * pw : nullptr,
                                                                  w0, w1, sm);
    const int i = ta * MN_TILE + ra, j = tb * MN_TILE + rb;
    if (i <= j && j < N && acc) atomicAdd(inter + ((size_t)b * N + i) * N + j, acc);
}

// grid (B), MN_T lanes, N <= MN_MAX.  -> rank_mask i32 [B][N]: the input index of paint rank r (r < kept; -1 behind), kept i32 [B]
__global__ __launch_bounds__(MN_T) void mn_select_kernel(const float* __restrict__ scores, const unsigned* __restrict__ inter, int N,
                                                         float thresh, int small_on_top, int* __restrict__ rank_mask,
                                                         int* __restrict__ kept_out) {
    __shared__ float s_score[MN_MAX];
    __shared__ unsigned s_area[MN_MAX];                      // by visit position
    __shared__ int s_order[MN_MAX];                          // visit position -> input index
    __shared__ int s_alive[MN_MAX];                          // by visit position
    __shared__ int s_kept;
    const int t = threadIdx.x, b = blockIdx.x;
    const unsigned* I = inter + (size_t)b * N * N;
    if (t < N) s_score[t] = scores[(size_t)b * N + t];
    if (t == 0) s_kept = 0;
    __syncthreads();
    // a mask whose score is NaN is absent (the padding of a frame with fewer masks than N): placed behind the others, never alive
    int pos = 0;
    bool present = false;
    if (t < N) {
        const float s = s_score[t];
        present = s == s;
        int ahead = 0, n_present = 0, absent_behind = 0;
        for (int j = 0; j < N; ++j) {
            const float q = s_score[j];
            ahead += (q > s) || (q == s && j > t);
            n_present += q == q;
            absent_behind += q != q && j > t;
        }
        pos = present ? ahead : n_present + absent_behind;
    }
    __syncthreads();
    if (t < N) { s_order[pos] = t; s_area[pos] = I[(size_t)t * N + t]; s_alive[pos] = present; }
    __syncthreads();
    // greedy pass: thread t is visit position t
    const int me = t < N ? s_order[t] : 0;
    const float my_area = t < N ? (float)s_area[t] : 0.f;
    for (int p = 0; p < N; ++p) {
        if (s_alive[p] && t > p && t < N && s_alive[t]) {
            const int i = s_order[p];
            const float inter_ij = (float)I[(size_t)min(i, me) * N + max(i, me)];
            const float ovr = __fdiv_rn(inter_ij, __fsub_rn(__fadd_rn((float)s_area[p], my_area), inter_ij));
            if (!(ovr <= thresh)) s_alive[t] = 0;            // a NaN (two empty masks) suppresses
        }
        __syncthreads();
    }
    // paint rank among the survivors: area ascending, visit position ascending
    int rank = -1;
    if (t < N && s_alive[t]) {
        rank = 0;
        const unsigned a = s_area[t];
        for (int q = 0; q < N; ++q) rank += s_alive[q] && (s_area[q] < a || (s_area[q] == a && q < t));
        atomicAdd(&s_kept, 1);
    }
    if (t < N) rank_mask[(size_t)b * N + t] = -1;
    __syncthreads();
    const int kept = s_kept;
    if (rank >= 0) rank_mask[(size_t)b * N + (small_on_top ? kept - 1 - rank : rank)] = me;
    if (t == 0) kept_out[b] = kept;
}

// grid (ceil(HW / 256), B).  rankmap i32 [B][HW]: 0 or 1 + the highest paint rank covering the pixel; vis u32 [B][N] (zero on entry).
__global__ __launch_bounds__(256) void mn_paint_kernel(const unsigned* __restrict__ planes, const int* __restrict__ rank_mask,
                                                       const int* __restrict__ kept_in, int N, int H, int W, int wpr, int pw,
                                                       int* __restrict__ rankmap, unsigned* __restrict__ vis) {
    __shared__ unsigned s_vis[MN_MAX];
    __shared__ int s_mask[MN_MAX];
    const int b = blockIdx.y, t = threadIdx.x;
    const int kept = min(max(kept_in[b], 0), N);
    for (int r = t; r < kept; r += 256) { s_vis[r] = 0; s_mask[r] = min(max(rank_mask[(size_t)b * N + r], 0), N - 1); }
    __syncthreads();
    const long HW = (long)H * W, p = (long)blockIdx.x * 256 + t;
    if (p < HW) {
        const int y = (int)(p / W), x = (int)(p - (long)y * W);
        const unsigned* col = planes + (size_t)b * N * pw + y * wpr + (x >> 5);
        const unsigned bit = 1u << (x & 31);
        int r = kept - 1;
        while (r >= 0 && !(col[(size_t)s_mask[r] * pw] & bit)) --r;
        rankmap[(size_t)b * HW + p] = r + 1;
        if (r >= 0) atomicAdd(&s_vis[r], 1u);
    }
    __syncthreads();
    for (int r = t; r < kept; r += 256)
        if (s_vis[r]) atomicAdd(vis + (size_t)b * N + r, s_vis[r]);
}

// grid (B), MN_T lanes.  The ranks with visible pixels, compacted in rank order -> out_of_rank i32 [B][N] (rank -> output id 1..count,
// 0 hidden), source, out_scores, report.
__global__ __launch_bounds__(MN_T) void mn_compact_kernel(const float* __restrict__ scores, const int* __restrict__ rank_mask,
                                                          const int* __restrict__ kept_in, const unsigned* __restrict__ vis, int N,
                                                          int* __restrict__ out_of_rank, int* __restrict__ source,
                                                          float* __restrict__ out_scores, int* __restrict__ report) {
    __shared__ int s_seen[MN_MAX];
    __shared__ int s_count;
    const int t = threadIdx.x, b = blockIdx.x;
    const int kept = min(max(kept_in[b], 0), N);
    if (t == 0) s_count = 0;
    if (t < N) {
        s_seen[t] = t < kept && vis[(size_t)b * N + t] != 0;
        source[(size_t)b * N + t] = -1;
        out_scores[(size_t)b * N + t] = 0.f;
        out_of_rank[(size_t)b * N + t] = 0;
    }
    __syncthreads();
    if (t < N && s_seen[t]) {
        int k = 0;
        for (int q = 0; q < t; ++q) k += s_seen[q];
        const int m = min(max(rank_mask[(size_t)b * N + t], 0), N - 1);
        source[(size_t)b * N + k] = m;
        out_scores[(size_t)b * N + k] = scores[(size_t)b * N + m];
        out_of_rank[(size_t)b * N + t] = k + 1;
        atomicAdd(&s_count, 1);
    }
    __syncthreads();
    if (t < 4) report[b * 4 + t] = t == 0 ? s_count : t == 1 ? kept : 0;
}

// grid (ceil(HW / (256 * PIX)), B).  PIX = 16: HW % 16 == 0 and 16-byte aligned outputs, 16 pixels per lane and store; PIX = 1: any.
template <int PIX>
__global__ __launch_bounds__(256) void mn_write_kernel(const int* __restrict__ rankmap, const int* __restrict__ out_of_rank, int N, long HW,
                                                       uint8_t* __restrict__ out_masks, int* __restrict__ ids) {
    __shared__ int s_id[MN_MAX + 1];                         // rank + 1 -> output id
    const int b = blockIdx.y, t = threadIdx.x;
    for (int r = t; r <= N; r += 256) s_id[r] = r ? out_of_rank[(size_t)b * N + r - 1] : 0;
    __syncthreads();
    const long p = ((long)blockIdx.x * 256 + t) * PIX;
    if (p >= HW) return;
    int id[PIX];
#pragma unroll
    for (int k = 0; k < PIX; ++k) id[k] = s_id[min(max(rankmap[(size_t)b * HW + p + k], 0), N)];
    uint8_t* dst = out_masks + (size_t)b * N * HW + p;
    if (PIX == 16) {
        int4* q = reinterpret_cast<int4*>(ids + (size_t)b * HW + p);
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = make_int4(id[4 * k], id[4 * k + 1], id[4 * k + 2], id[4 * k + 3]);
        for (int n = 0; n < N; ++n) {
            unsigned w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                w[k] = (id[4 * k] == n + 1 ? 0xffu : 0u) | (id[4 * k + 1] == n + 1 ? 0xff00u : 0u) | (id[4 * k + 2] == n + 1 ? 0xff0000u : 0u) |
                       (id[4 * k + 3] == n + 1 ? 0xff000000u : 0u);
            *reinterpret_cast<uint4*>(dst + (size_t)n * HW) = make_uint4(w[0], w[1], w[2], w[3]);
        }
    } else {
        ids[(size_t)b * HW + p] = id[0];
        for (int n = 0; n < N; ++n) dst[(size_t)n * HW] = id[0] == n + 1 ? 255 : 0;
    }
}

// workspace layout, for frames of `cap_b` x `cap_n` masks: planes | inter, vis (zeroed together) | rankmap | rank_mask, out_of_rank, kept
struct MnWs { unsigned* planes; unsigned* inter; unsigned* vis; int* rankmap; int* rank_mask; int* out_of_rank; int* kept; size_t zero_bytes; };

static size_t mn_layout(MnWs* out, void* ws, int B, int N, int H, int W) {
    const size_t bn = (size_t)B * N;
    MnWs none, &r = out ? *out : none;
    WsWalk w{static_cast<char*>(ws)};
    r.planes = w.take<unsigned>(bn * mn_plane_words(H, W));
    r.inter = w.take<unsigned>(bn * N + bn);
    r.vis = r.inter ? r.inter + bn * N : nullptr;
    r.zero_bytes = (bn * N + bn) * 4;
    r.rankmap = w.take<int>((size_t)B * H * W);
    r.rank_mask = w.take<int>(bn);
    r.out_of_rank = w.take<int>(bn);
    r.kept = w.take<int>((size_t)B);
    return w.off;
}

size_t mask_nms_ws_bytes(int B, int N, int H, int W) { return mn_layout(nullptr, nullptr, B, N, H, W); }

int mask_nms_max() { return MN_MAX; }

// ws: mask_nms_ws_bytes(>= B, >= N, H, W) bytes.  N = 0: the id map and the report are cleared, nothing else exists.
int launch_mask_nms(const uint8_t* masks, const float* scores, int B, int N, int H, int W, float thresh, int small_on_top, uint8_t* out_masks,
                    int* ids, int* source, float* out_scores, int* report, void* ws, hipStream_t st) {
    if (B <= 0) return 0;
    if (H < 1 || W < 1) return fail("mask nms: negative or empty frame");
    if ((long)H * W > (1L << 24)) return fail("mask nms: a frame of more than 2^24 pixels (the overlap counts are compared in float32)");
    if (N < 0 || N > MN_MAX) return fail("mask nms: n_masks outside 0..1024");
    if (!ids || !report) return fail("mask nms: null tensor");
    const long HW = (long)H * W;
    if (N == 0) {
        if (launch_zero(ids, (size_t)B * HW * 4, st)) return -1;
        return launch_zero(report, (size_t)B * 16, st);
    }
    if (!masks || !scores || !out_masks || !source || !out_scores || !ws) return fail("mask nms: null tensor");
    if (((uintptr_t)ids & 3) || ((uintptr_t)source & 3) || ((uintptr_t)out_scores & 3) || ((uintptr_t)report & 3) || ((uintptr_t)scores & 3))
        return fail("mask nms: a 32-bit tensor that is not 4-byte aligned");
    const int wpr = (W + 31) / 32, pw = (int)mn_plane_words(H, W);
    MnWs w;
    mn_layout(&w, ws, B, N, H, W);
    const double px = (double)B * N * HW;
    {
        ProfScope prof("mask_nms_pack", px + 4.0 * B * N * pw, 0.0, st);
        const dim3 grid((pw + 255) / 256, (unsigned)(B * N));
        if (W % 16 == 0 && ((uintptr_t)masks & 15) == 0)
            hipLaunchKernelGGL(mn_pack_kernel<true>, grid, dim3(256), 0, st, masks, w.planes, H, W, wpr, pw);
        else
            hipLaunchKernelGGL(mn_pack_kernel<false>, grid, dim3(256), 0, st, masks, w.planes, H, W, wpr, pw);
        QB_CHECK(hipGetLastError());
    }
    if (launch_zero(w.inter, w.zero_bytes, st)) return -1;
    const int nt = (N + MN_TILE - 1) / MN_TILE;
    {
        ProfScope prof("mask_nms_gram", 4.0 * B * N * pw * (nt + 1) / 2.0 + 4.0 * B * N * N, 0.0, st);
        hipLaunchKernelGGL(mn_gram_kernel, dim3(nt * (nt + 1) / 2, (pw + MN_CHUNK - 1) / MN_CHUNK, B), dim3(256), 0, st, w.planes, w.inter, N, pw);
        QB_CHECK(hipGetLastError());
    }
    {
        ProfScope prof("mask_nms_select", 4.0 * B * N * N, 0.0, st);
        hipLaunchKernelGGL(mn_select_kernel, dim3(B), dim3(MN_T), 0, st, scores, w.inter, N, thresh, small_on_top, w.rank_mask, w.kept);
        QB_CHECK(hipGetLastError());
    }
    {
        ProfScope prof("mask_nms_paint", 4.0 * B * N * pw + 4.0 * B * HW, 0.0, st);
        hipLaunchKernelGGL(mn_paint_kernel, dim3((unsigned)((HW + 255) / 256), B), dim3(256), 0, st, w.planes, w.rank_mask, w.kept, N, H, W, wpr, pw,
                           w.rankmap, w.vis);
        QB_CHECK(hipGetLastError());
    }
    {
        ProfScope prof("mask_nms_write", px + 8.0 * B * HW, 0.0, st);
        hipLaunchKernelGGL(mn_compact_kernel, dim3(B), dim3(MN_T), 0, st, scores, w.rank_mask, w.kept, w.vis, N, w.out_of_rank, source, out_scores,
                           report);
        if (HW % 16 == 0 && ((uintptr_t)out_masks & 15) == 0 && ((uintptr_t)ids & 15) == 0)
            hipLaunchKernelGGL(mn_write_kernel<16>, dim3((unsigned)((HW / 16 + 255) / 256), B), dim3(256), 0, st, w.rankmap, w.out_of_rank, N, HW,
                               out_masks, ids);
        else
            hipLaunchKernelGGL(mn_write_kernel<1>, dim3((unsigned)((HW + 255) / 256), B), dim3(256), 0, st, w.rankmap, w.out_of_rank, N, HW, out_masks,
                               ids);
        QB_CHECK(hipGetLastError());
    }
    return 0;
}

}  // namespace quber
