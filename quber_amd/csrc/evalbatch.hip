// Batched evaluation (eval/evaluation.py:57-274 `multilabel_metrics` for B pairs of label maps in one call): everything the host did
// between the launches of one frame - reading the label counts, building the F-measure matrix, the Munkres assignment, sizing the
// boundary grids - happens on the device, so the B frames are enqueued once and read back once.
//
//   1. labels    presence / rank / contingency of metrics.hip with the frame on a grid axis (bodies shared: evalbody.h)
//   2. boundary  pack / bmap / pair of boundary.hip, grids sized by `cap`; a block whose object index is not below the frame's own count
//                (read from the record) returns before it touches anything
//   3. score     F = 2PR / (P + R) per (gt object, predicted object) in float64, NaN -> 0, cost = max(F) - F
//   4. solver    one workgroup per frame runs quber_amd/eval/assignment.py:munkres_assign step for step (same tie-breaking)
//   5. gather    per assigned pair: indices, overlap, union, boundary true positives; the status word
//
// Every frame has one record in `out` (EbLayout); the stages write into it directly, the host copies `out` back once.  The final
// float sums stay on the host (numpy's summation order is part of the reference's numbers).
#include <limits.h>
#include <math.h>

#include "common.h"
#include "evalbody.h"

namespace quber {

constexpr int EB_T = 256;        // threads of the score / solver / gather blocks = the largest cap: thread t owns column t
constexpr int EB_CAP_MAX = EB_T;
constexpr int EB_LDS_N = 128;    // largest solver size n whose n x n float64 cost matrix lives in LDS (128 KiB + 6 KiB bookkeeping <= 160 KiB)
constexpr int EB_BATCH_MAX = 4096;

// the record of one frame, byte offsets; the 8-byte fields come first so every field is aligned for any cap
struct EbLayout {
    size_t table;        // u64 [cap][cap]   contingency table, row = gt label index, column = predicted label index (background included)
    size_t F;            // f64 [cap][cap]   F-measure, row = gt object, column = predicted object (background excluded), row stride cap
    size_t area;         // u64 [2][cap]     pixels per label index: [0] predicted, [1] gt
    size_t pair_tps;     // u64 [cap]        per assigned pair: overlap
    size_t pair_union;   // u64 [cap]        ... union
    size_t ptps;         // u32 [cap][cap]   boundary precision true positives, [gt object][predicted object]
    size_t rtps;         // u32 [cap][cap]   boundary recall true positives
    size_t hdr;          // i32 [8]          n_pred, n_gt (distinct labels, background included), out-of-range flag, status, objects pred, objects gt, pairs, solver status
    size_t labels;       // i32 [2][cap]     sorted unique labels: [0] predicted, [1] gt
    size_t bc;           // u32 [2][cap]     boundary size per object: [0] predicted, [1] gt
    size_t assign;       // i32 [cap]        per gt object the predicted object assigned to it, or -1
    size_t pairs;        // i32 [cap][2]     the assigned pairs (gt object, predicted object), in row order
    size_t pair_ptps;    // u32 [cap]        per assigned pair: boundary precision true positives
    size_t pair_rtps;    // u32 [cap]        ... recall true positives
    size_t bytes;        // of one record, a multiple of 8
};

static EbLayout eb_layout(int cap) {
    const size_t c = (size_t)cap, cc = c * c;
    EbLayout L;
    size_t o = 0;
    L.table = o; o += 8 * cc;
    L.F = o; o += 8 * cc;
    L.area = o; o += 8 * 2 * c;
    L.pair_tps = o; o += 8 * c;
    L.pair_union = o; o += 8 * c;
    L.ptps = o; o += 4 * cc;
    L.rtps = o; o += 4 * cc;
    L.hdr = o; o += 4 * 8;
    L.labels = o; o += 4 * 2 * c;
    L.bc = o; o += 4 * 2 * c;
    L.assign = o; o += 4 * c;
    L.pairs = o; o += 4 * 2 * c;
    L.pair_ptps = o; o += 4 * c;
    L.pair_rtps = o; o += 4 * c;
    L.bytes = (o + 7) & ~(size_t)7;
    return L;
}

enum { EB_BAD_LABEL = 1, EB_OVER_CAP = 2, EB_SOLVER_BOUND = 4, EB_NO_LDS = 8 };

template <typename T> __device__ inline T* eb_field(char* out, const EbLayout& L, long b, size_t off) {
    return reinterpret_cast<T*>(out + (size_t)b * L.bytes + off);
}

// a frame the label stage gave up on: a label outside 0..65535, or more than cap labels in a map.  No later stage works on it.
__device__ inline bool eb_flagged(const int* hdr, int cap) { return hdr[2] || hdr[0] > cap || hdr[1] > cap; }
// the labels are sorted and non-negative: the background label 0, if present, has index 0, and object k has label index k + eb_bg
__device__ inline int eb_bg(const int* hdr, const int* labels, int cap, int side) { return hdr[side] > 0 && labels[side * cap] == 0; }
__device__ inline int eb_nobj(const int* hdr, const int* labels, int cap, int side) {
    return eb_flagged(hdr, cap) ? 0 : hdr[side] - eb_bg(hdr, labels, cap, side);
}

// ------------------------------------------------------------------------------------------------ 1. labels
// grid (blocks, B)
__global__ void eb_presence_kernel(const int* __restrict__ pred, const int* __restrict__ gt, long n, unsigned* __restrict__ flags, char* out,
                                   EbLayout L) {
    const long b = blockIdx.y;
    label_presence_body(pred + b * n, gt + b * n, n, flags + b * 2 * LAB_MAX, eb_field<int>(out, L, b, L.hdr) + 2);
}

// grid (2, B)
__global__ __launch_bounds__(1024) void eb_rank_kernel(const unsigned* __restrict__ flags, int cap, unsigned short* __restrict__ lut, char* out,
                                                       EbLayout L) {
    const long b = blockIdx.y;
    label_rank_body(flags + b * 2 * LAB_MAX, cap, blockIdx.x, lut + b * 2 * LAB_MAX, eb_field<int>(out, L, b, L.labels),
                    eb_field<int>(out, L, b, L.hdr));
}

// grid (blocks, B); LDS: 4096 words
__global__ __launch_bounds__(256) void eb_contingency_kernel(const int* __restrict__ pred, const int* __restrict__ gt, long n,
                                                             const unsigned short* __restrict__ lut, int cap, char* out, EbLayout L) {
    const long b = blockIdx.y;
    contingency_body(pred + b * n, gt + b * n, n, lut + b * 2 * LAB_MAX, eb_field<int>(out, L, b, L.hdr), cap, eb_field<u64>(out, L, b, L.table));
}

// ------------------------------------------------------------------------------------------------ 2. boundary
// planes: [B][2 cap][H][wpr], the predicted objects of a frame in planes 0..cap-1, the gt objects in cap..2cap-1
// grid (ceil(H wpr / 4), 2 cap, B)
__global__ __launch_bounds__(256) void eb_pack_kernel(const int* __restrict__ pred, const int* __restrict__ gt, int H, int W, int wpr, int cap,
                                                      char* out, EbLayout L, u64* __restrict__ seg) {
    const int m = blockIdx.y, side = m >= cap, k = m - side * cap;
    const long b = blockIdx.z;
    const int* hdr = eb_field<int>(out, L, b, L.hdr);
    const int* labels = eb_field<int>(out, L, b, L.labels);
    if (k >= eb_nobj(hdr, labels, cap, side)) return;
    const int value = labels[side * cap + k + eb_bg(hdr, labels, cap, side)];
    bnd_pack_body((side ? gt : pred) + b * H * W, value, H, W, wpr, seg + (b * 2 * cap + m) * H * wpr);
}

// grid (2 cap, B); LDS: reach[H][wpr]
__global__ __launch_bounds__(1024) void eb_bmap_kernel(const u64* __restrict__ seg, int H, int W, int wpr, int radius, int cap, char* out,
                                                       EbLayout L, u64* __restrict__ bmap, u64* __restrict__ dil) {
    const int m = blockIdx.x, side = m >= cap, k = m - side * cap;
    const long b = blockIdx.y;
    const int* hdr = eb_field<int>(out, L, b, L.hdr);
    if (k >= eb_nobj(hdr, eb_field<int>(out, L, b, L.labels), cap, side)) return;
    const long o = (b * 2 * cap + m) * H * wpr;
    bnd_bmap_body(seg + o, H, W, wpr, radius, bmap + o, dil + o, eb_field<unsigned>(out, L, b, L.bc) + m);
}

// grid (cap, cap, B): x = predicted object, y = gt object
__global__ __launch_bounds__(256) void eb_pair_kernel(const u64* __restrict__ bmap, const u64* __restrict__ dil, int n, int cap, char* out,
                                                      EbLayout L) {
    const int j = blockIdx.x, i = blockIdx.y;
    const long b = blockIdx.z;
    const int* hdr = eb_field<int>(out, L, b, L.hdr);
    const int* labels = eb_field<int>(out, L, b, L.labels);
    if (j >= eb_nobj(hdr, labels, cap, 0) || i >= eb_nobj(hdr, labels, cap, 1)) return;
    const long op = (b * 2 * cap + j) * n, og = (b * 2 * cap + cap + i) * n;
    bnd_pair_body(bmap + op, dil + op, bmap + og, dil + og, n, eb_field<unsigned>(out, L, b, L.ptps) + i * cap + j,
                  eb_field<unsigned>(out, L, b, L.rtps) + i * cap + j);
}

// ------------------------------------------------------------------------------------------------ block reductions
// every thread of the block calls it; every thread gets the result.  red: EB_T / 64 shared elements
template <typename T, typename Op> __device__ inline T eb_reduce(T v, Op op, T* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
    __syncthreads();                                 // the previous result has been read by everyone
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    T r = red[0];
#pragma unroll
    for (int w = 1; w < EB_T / 64; ++w) r = op(r, red[w]);
    return r;
}
struct EbMin { template <typename T> __device__ T operator()(T a, T b) const { return b < a ? b : a; } };
struct EbMax { template <typename T> __device__ T operator()(T a, T b) const { return b > a ? b : a; } };
struct EbAdd { template <typename T> __device__ T operator()(T a, T b) const { return a + b; } };

// ------------------------------------------------------------------------------------------------ 3. score matrix
// multilabel_metrics lines 102-110 over the non-background labels, float64, IEEE division (no contraction: the build sets
// -ffp-contract=off).  grid (B); thread t = predicted object t.  rows / cols [B]: the shape the solver gets (0 x 0: nothing to solve)
__global__ __launch_bounds__(EB_T) void eb_score_kernel(char* out, EbLayout L, int cap, double* __restrict__ score, int* __restrict__ rows,
                                                        int* __restrict__ cols) {
    __shared__ double red[EB_T / 64];
    const long b = blockIdx.x;
    const int t = threadIdx.x;
    int* hdr = eb_field<int>(out, L, b, L.hdr);
    const int* labels = eb_field<int>(out, L, b, L.labels);
    const u64* table = eb_field<u64>(out, L, b, L.table);
    u64* area = eb_field<u64>(out, L, b, L.area);
    double* F = eb_field<double>(out, L, b, L.F);
    const int no_p = eb_nobj(hdr, labels, cap, 0), no_g = eb_nobj(hdr, labels, cap, 1);
    const bool solve = no_p > 0 && no_g > 0;
    if (t == 0) {
        hdr[4] = no_p;
        hdr[5] = no_g;
        rows[b] = solve ? no_g : 0;
        cols[b] = solve ? no_p : 0;
    }
    if (eb_flagged(hdr, cap)) return;
    const int np_ = hdr[0], ng = hdr[1];
    if (t < np_) {
        u64 s = 0;
        for (int i = 0; i < ng; ++i) s += table[(long)i * cap + t];
        area[t] = s;
    }
    if (t < ng) {
        u64 s = 0;
        for (int j = 0; j < np_; ++j) s += table[(long)t * cap + j];
        area[cap + t] = s;
    }
    __syncthreads();
    if (!solve) return;
    const int bgp = eb_bg(hdr, labels, cap, 0), bgg = eb_bg(hdr, labels, cap, 1);
    double top = -INFINITY;
    if (t < no_p) {
        const double ap = (double)area[t + bgp];
        for (int i = 0; i < no_g; ++i) {
            const double tps = (double)table[(long)(i + bgg) * cap + t + bgp], ag = (double)area[cap + i + bgg];
            const double P = tps / ap, R = tps / ag;
            double f = ((2.0 * P) * R) / (P + R);
            if (f != f) f = 0.0;                                  // 0 / 0: no overlap
            F[(long)i * cap + t] = f;
            top = f > top ? f : top;
        }
    }
    top = eb_reduce(top, EbMax(), red);
    if (t < no_p)
        for (int i = 0; i < no_g; ++i) score[(b * cap + i) * cap + t] = top - F[(long)i * cap + t];
}

// ------------------------------------------------------------------------------------------------ 4. assignment
// One workgroup per frame; quber_amd/eval/assignment.py:munkres_assign (Clapper's six steps as the reference's vendored solver orders
// them) on the rows x cols matrix zero-padded to n = max(rows, cols).  Stars and primes are index arrays (at most one star per row and
// per column; a row is primed at most once between two clears, because a primed row with a star is covered until the clear).
// Thread t owns column t of the matrix (n <= cap <= EB_T): after the row reduction every access to C[.][t] is thread t's own, so the
// barriers below order the cover / star arrays only.  Thread 0 makes the decisions and publishes them in `ctl`; every loop condition
// is computed from block-wide reductions and `ctl`, so all threads leave every loop together.
//
// Loop bounds (n = size of the padded matrix):
//   phases (step 3 -> 4 -> 5)   every phase but the last stars one more zero, step 2 stars at least one, n stars end it: at most n
//                               phases start; the (n + 1)-th is refused.
//   step 4 / 6 iterations       within a phase a covered row stays covered, so at most n iterations prime-and-cover, one primes without
//                               a star in the row (ends the phase), and every step 6 is followed by a priming iteration, because the
//                               smallest uncovered element m only gets m subtracted (m - m == 0 exactly) and so leaves an uncovered
//                               zero: at most n + 1 of those.  2n + 2 iterations in all; the next one is refused.
//   step 5 path                 alternates primed and starred zeros through distinct rows: at most n starred zeros; more is refused.
// A refused frame gets EB_SOLVER_BOUND and an empty assignment (only non-finite input gets there).
//
// mode: 0 = the LDS launch of placement "auto" (a frame with n > EB_LDS_N is left to the launch of mode 3), 1 = LDS forced (such a frame
// gets EB_NO_LDS), 2 = matrix in `mat` for every frame, 3 = the device-memory launch of "auto" (frames with n > EB_LDS_N only)
template <bool LDS>
__global__ __launch_bounds__(EB_T) void eb_munkres_kernel(const double* __restrict__ score /*[B][cap][cap]*/, const int* __restrict__ rows_,
                                                          const int* __restrict__ cols_, int cap, int mode, double* __restrict__ mat /*[B][cap][cap]*/,
                                                          int* __restrict__ assign, long assign_stride, int* __restrict__ status,
                                                          long status_stride) {
    extern __shared__ double eb_lds_mat[];
    __shared__ int star_row[EB_T], star_col[EB_T], prime_row[EB_T], row_cov[EB_T], col_cov[EB_T];
    __shared__ double red_d[EB_T / 64];
    __shared__ int red_i[EB_T / 64];
    __shared__ int ctl[2];
    const long b = blockIdx.x;
    const int t = threadIdx.x;
    int rows = rows_[b], cols = cols_[b];
    int* asg = assign + b * assign_stride;
    int* stp = status + b * status_stride;
    int st = 0;
    if (rows < 0 || cols < 0 || rows > cap || cols > cap) { st = EB_OVER_CAP; rows = cols = 0; }
    const int n = rows > cols ? rows : cols;
    const bool big = n > EB_LDS_N;
    if ((mode == 0 && big) || (mode == 3 && !big)) return;        // the other launch of "auto" has this frame
    if (mode == 1 && big) st |= EB_NO_LDS;
    if (st || n == 0) {
        if (t < cap) asg[t] = -1;
        if (t == 0) *stp = st;
        return;
    }
    double* C = LDS ? eb_lds_mat : mat + b * cap * cap;
    const double* src = score + b * cap * cap;
    for (int idx = t; idx < n * n; idx += EB_T) {
        const int i = idx / n, j = idx - i * n;
        C[idx] = (i < rows && j < cols) ? src[(long)i * cap + j] : 0.0;       // zero padding (munkres.py pad_matrix)
    }
    star_row[t] = star_col[t] = prime_row[t] = -1;
    row_cov[t] = col_cov[t] = 0;
    __syncthreads();
    if (t < n) {                                                              // step 1: thread t = row t
        double lo = C[(long)t * n];
        for (int j = 1; j < n; ++j) { const double v = C[(long)t * n + j]; lo = v < lo ? v : lo; }
        for (int j = 0; j < n; ++j) C[(long)t * n + j] -= lo;
    }
    __syncthreads();
    for (int i = 0; i < n; ++i) {                                             // step 2: first free zero of every row, rows in order
        const bool free_zero = t < n && !col_cov[t] && C[(long)i * n + t] == 0.0;
        const int j = eb_reduce(free_zero ? t : INT_MAX, EbMin(), red_i);
        if (t == 0 && j != INT_MAX) { star_row[i] = j; star_col[j] = i; col_cov[j] = 1; }
        __syncthreads();
    }
    int refused = 0;
    for (int phase = 0;; ++phase) {
        if (t < n) {                                                          // step 3
            row_cov[t] = 0;
            prime_row[t] = -1;
            col_cov[t] = star_col[t] >= 0;
        }
        const int stars = eb_reduce((int)(t < n && star_col[t] >= 0), EbAdd(), red_i);
        if (stars >= n) break;
        if (phase >= n) { refused = 1; break; }
        int zi = -1, zj = -1;
        for (int it = 0;; ++it) {                                             // steps 4 / 6
            if (it >= 2 * n + 2) { refused = 1; break; }
            const bool cc = t < n ? col_cov[t] != 0 : true;
            int r = INT_MAX;                                                  // first uncovered row with a zero in this (uncovered) column
            if (!cc)
                for (int i = 0; i < n; ++i)
                    if (!row_cov[i] && C[(long)i * n + t] == 0.0) { r = i; break; }
            const int i0 = eb_reduce(r, EbMin(), red_i);
            if (i0 == INT_MAX) {                                              // step 6: no uncovered zero
                double lo = INFINITY;
                if (!cc)
                    for (int i = 0; i < n; ++i)
                        if (!row_cov[i]) { const double v = C[(long)i * n + t]; lo = v < lo ? v : lo; }
                const double m = eb_reduce(lo, EbMin(), red_d);
                if (t < n)
                    for (int i = 0; i < n; ++i) {
                        double v = C[(long)i * n + t];
                        if (row_cov[i]) v += m;                               // add to covered rows, THEN subtract from uncovered columns:
                        if (!cc) v -= m;                                      // two roundings on a cell that gets both, as the reference
                        C[(long)i * n + t] = v;
                    }
                continue;
            }
            // the first row with an uncovered zero is i0; a column has its first zero there iff it has an uncovered zero there: the LAST one
            const int j0 = eb_reduce(r == i0 ? t : -1, EbMax(), red_i);
            if (t == 0) {
                prime_row[i0] = j0;
                const int s = star_row[i0];
                if (s < 0) ctl[0] = 1;                                        // no star in the row: augment
                else { row_cov[i0] = 1; col_cov[s] = 0; ctl[0] = 0; }
            }
            __syncthreads();
            if (ctl[0]) { zi = i0; zj = j0; break; }
        }
        if (refused) break;
        if (t == 0) {                                                         // step 5: flip the alternating path
            int r = zi, c = zj, bad = 0;
            for (int k = 0;; ++k) {
                if (k > n) { bad = 1; break; }
                const int r1 = star_col[c];                                   // the star of this column, if any, loses it
                star_row[r] = c;
                star_col[c] = r;
                if (r1 < 0) break;
                r = r1;
                c = prime_row[r1];                                            // ... and its row takes its primed zero
                if (c < 0) { bad = 1; break; }
            }
            ctl[1] = bad;
        }
        __syncthreads();
        if (ctl[1]) { refused = 1; break; }
    }
    __syncthreads();
    if (t < cap) {
        int j = -1;
        if (!refused && t < rows) { j = star_row[t]; if (j >= cols) j = -1; }    // only pairs inside the original shape
        asg[t] = j;
    }
    if (t == 0) *stp = refused ? EB_SOLVER_BOUND : 0;
}

// ------------------------------------------------------------------------------------------------ 5. gather
// grid (B)
__global__ __launch_bounds__(EB_T) void eb_gather_kernel(char* out, EbLayout L, int cap) {
    __shared__ int pos[EB_T + 1];
    const long b = blockIdx.x;
    const int t = threadIdx.x;
    int* hdr = eb_field<int>(out, L, b, L.hdr);
    const int* labels = eb_field<int>(out, L, b, L.labels);
    if (eb_flagged(hdr, cap)) {
        if (t == 0) {
            hdr[3] = (hdr[2] ? EB_BAD_LABEL : 0) | ((hdr[0] > cap || hdr[1] > cap) ? EB_OVER_CAP : 0);
            hdr[6] = 0;
        }
        return;
    }
    const int rows = hdr[5], bgp = eb_bg(hdr, labels, cap, 0), bgg = eb_bg(hdr, labels, cap, 1);
    const int* assign = eb_field<int>(out, L, b, L.assign);
    const int j = (t < rows && t < cap) ? assign[t] : -1;
    pos[t] = j >= 0;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int i = 0; i < EB_T; ++i) { const int f = pos[i]; pos[i] = run; run += f; }
        pos[EB_T] = run;
    }
    __syncthreads();
    if (j >= 0) {
        const int k = pos[t];
        const u64* table = eb_field<u64>(out, L, b, L.table);
        const u64* area = eb_field<u64>(out, L, b, L.area);
        int* pairs = eb_field<int>(out, L, b, L.pairs);
        const u64 tps = table[(long)(t + bgg) * cap + j + bgp];
        pairs[2 * k] = t;
        pairs[2 * k + 1] = j;
        eb_field<u64>(out, L, b, L.pair_tps)[k] = tps;
        eb_field<u64>(out, L, b, L.pair_union)[k] = area[cap + t + bgg] + area[j + bgp] - tps;
        eb_field<unsigned>(out, L, b, L.pair_ptps)[k] = eb_field<unsigned>(out, L, b, L.ptps)[(long)t * cap + j];
        eb_field<unsigned>(out, L, b, L.pair_rtps)[k] = eb_field<unsigned>(out, L, b, L.rtps)[(long)t * cap + j];
    }
    if (t == 0) {
        hdr[3] = hdr[7];                                                      // the solver's bits
        hdr[6] = pos[EB_T];
    }
}

// ------------------------------------------------------------------------------------------------ host
static inline int eb_wpr(int W) { return (W + 63) / 64; }

size_t eval_batch_out_bytes(int batch, int cap) { return (size_t)batch * eb_layout(cap).bytes; }

// ws: flags u32 [B][2][LAB_MAX] | score f64 [B][cap][cap] | mat f64 [B][cap][cap] | planes u64 [3][B][2 cap][H][wpr] (with_boundary) |
//     lut u16 [B][2][LAB_MAX] | rows i32 [B] | cols i32 [B]; the fields follow each other without padding
struct EbWs { unsigned* flags; double* score; double* mat; u64 *seg, *bmap, *dil; unsigned short* lut; int *rows, *cols; };
static size_t eb_ws_layout(EbWs* out, void* ws, int batch, int H, int W, int cap, int with_boundary) {
    const size_t B = (size_t)batch, cc = (size_t)cap * cap;
    const size_t planes = with_boundary ? B * 2 * cap * H * eb_wpr(W) : 0;        // words of one of the three sets
    EbWs none, &r = out ? *out : none;
    WsWalk w{static_cast<char*>(ws)};
    r.flags = w.take<unsigned>(B * 2 * LAB_MAX, false);
    r.score = w.take<double>(B * cc, false);
    r.mat = w.take<double>(B * cc, false);
    r.seg = w.take<u64>(3 * planes, false);
    r.bmap = r.seg ? r.seg + planes : nullptr;
    r.dil = r.seg ? r.seg + 2 * planes : nullptr;
    r.lut = w.take<unsigned short>(B * 2 * LAB_MAX, false);
    r.rows = w.take<int>(2 * B, false);
    r.cols = r.rows ? r.rows + B : nullptr;
    return (w.off + 7) & ~(size_t)7;
}
size_t eval_batch_ws_bytes(int batch, int H, int W, int cap, int with_boundary) { return eb_ws_layout(nullptr, nullptr, batch, H, W, cap, with_boundary); }

int launch_munkres_batch(const double* score, const int* rows, const int* cols, int batch, int cap, int placement, double* mat, int* assign,
                         long assign_stride, int* status, long status_stride, hipStream_t st) {
    if (batch < 1 || batch > EB_BATCH_MAX) return fail("munkres batch: batch outside 1..4096");
    if (cap < 1 || cap > EB_CAP_MAX) return fail("munkres batch: cap outside 1..256");
    if (placement < 0 || placement > 2) return fail("munkres batch: placement must be 0 (auto), 1 (LDS) or 2 (device memory)");
    const bool global = placement == 2 || (placement == 0 && cap > EB_LDS_N);
    if (global && !mat) return fail("munkres batch: this placement needs the workspace");
    ProfScope prof("eval_munkres", 8.0 * batch * cap * cap, 0.0, st);
    if (placement != 2) {
        const int nl = cap < EB_LDS_N ? cap : EB_LDS_N;
        // the attribute is per device (and this entry point may be called from several threads): set it on every call
        QB_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(eb_munkres_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     EB_LDS_N * EB_LDS_N * (int)sizeof(double)));
        hipLaunchKernelGGL(eb_munkres_kernel<true>, dim3(batch), dim3(EB_T), (size_t)nl * nl * sizeof(double), st, score, rows, cols, cap,
                           placement == 1 ? 1 : 0, mat, assign, assign_stride, status, status_stride);
        QB_CHECK(hipGetLastError());
    }
    if (global) {
        hipLaunchKernelGGL(eb_munkres_kernel<false>, dim3(batch), dim3(EB_T), 0, st, score, rows, cols, cap, placement == 2 ? 2 : 3, mat, assign,
                           assign_stride, status, status_stride);
        QB_CHECK(hipGetLastError());
    }
    return 0;
}

int launch_eval_batch(const int* pred, const int* gt, int batch, int H, int W, int cap, int radius, int with_boundary, int placement, void* ws,
                      void* out_, hipStream_t st) {
    if (batch < 1 || batch > EB_BATCH_MAX) return fail("eval batch: batch outside 1..4096");
    if (cap < 1 || cap > EB_CAP_MAX) return fail("eval batch: cap outside 1..256");
    if (H < 1 || W < 1 || (long)H * W > (1l << 32)) return fail("eval batch: frames of 1..2^32 pixels");
    if (placement < 0 || placement > 2) return fail("eval batch: placement must be 0 (auto), 1 (LDS) or 2 (device memory)");
    const int wpr = eb_wpr(W);
    const size_t plane = (size_t)H * wpr * sizeof(u64);
    if (with_boundary) {
        if (radius < 0 || radius > 63) return fail("boundary overlap: dilation radius must be 0..63");
        if (plane > 160 * 1024 - 64) return fail("boundary overlap: frame too large for the LDS flood fill (H * ceil(W/64) * 8 <= 160 KiB)");
    }
    const EbLayout L = eb_layout(cap);
    const size_t B = (size_t)batch, cc = (size_t)cap * cap;
    const long n = (long)H * W;
    char* out = reinterpret_cast<char*>(out_);
    EbWs w;
    eb_ws_layout(&w, ws, batch, H, W, cap, with_boundary);

    // accumulators: the records (table, out-of-range flag; and every field a stage leaves alone reads 0) and the presence flags
    if (int rc = launch_zero(out, B * L.bytes, st)) return rc;
    if (int rc = launch_zero(w.flags, B * 2 * LAB_MAX * sizeof(unsigned), st)) return rc;
    int blocks = (int)((n + 255) / 256);
    if (blocks > 1024) blocks = 1024;
    {
        ProfScope prof("eval_labels", 16.0 * batch * (double)n, 0.0, st);
        hipLaunchKernelGGL(eb_presence_kernel, dim3(blocks, batch), dim3(256), 0, st, pred, gt, n, w.flags, out, L);
        hipLaunchKernelGGL(eb_rank_kernel, dim3(2, batch), dim3(1024), 0, st, w.flags, cap, w.lut, out, L);
        hipLaunchKernelGGL(eb_contingency_kernel, dim3(blocks, batch), dim3(256), sizeof(unsigned) * 4096, st, pred, gt, n, w.lut, cap, out, L);
        QB_CHECK(hipGetLastError());
    }
    if (with_boundary) {
        ProfScope prof("eval_boundary", 8.0 * batch * (double)n, 0.0, st);
        hipLaunchKernelGGL(eb_pack_kernel, dim3((unsigned)(((long)H * wpr + 3) / 4), 2 * cap, batch), dim3(256), 0, st, pred, gt, H, W, wpr, cap,
                           out, L, w.seg);
        QB_CHECK(hipGetLastError());
        QB_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(eb_bmap_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     160 * 1024 - 64));
        hipLaunchKernelGGL(eb_bmap_kernel, dim3(2 * cap, batch), dim3(1024), plane, st, w.seg, H, W, wpr, radius, cap, out, L, w.bmap, w.dil);
        QB_CHECK(hipGetLastError());
        hipLaunchKernelGGL(eb_pair_kernel, dim3(cap, cap, batch), dim3(256), 0, st, w.bmap, w.dil, H * wpr, cap, out, L);
        QB_CHECK(hipGetLastError());
    }
    {
        ProfScope prof("eval_score", 16.0 * batch * cc, 0.0, st);
        hipLaunchKernelGGL(eb_score_kernel, dim3(batch), dim3(EB_T), 0, st, out, L, cap, w.score, w.rows, w.cols);
        QB_CHECK(hipGetLastError());
    }
    const long stride = (long)(L.bytes / sizeof(int));
    if (int rc = launch_munkres_batch(w.score, w.rows, w.cols, batch, cap, placement, w.mat, reinterpret_cast<int*>(out + L.assign), stride,
                                      reinterpret_cast<int*>(out + L.hdr) + 7, stride, st))
        return rc;
    {
        ProfScope prof("eval_gather", 64.0 * batch * cap, 0.0, st);
        hipLaunchKernelGGL(eb_gather_kernel, dim3(batch), dim3(EB_T), 0, st, out, L, cap);
        QB_CHECK(hipGetLastError());
    }
    return 0;
}

}  // namespace quber
