// Perturbed initial masks on the device (include/quber_hip.h: quber_perturb_masks; the definition is in INTEGRATION.md "Perturbed
// initial masks" and, as numpy, in tests/test_perturb_cpu.py).  Restates the reference's perturb_seg (tools/ours/perturbation_utils.py:
// 39-71): a random walk of erosions and dilations on random sub-rectangles of the mask, until the IoU with the mask it started from
// falls below a target.  The number of random draws per operation does not depend on the data, so the host draws the whole walk up
// front (quber_amd/perturb.py: perturb_program) and the kernel executes it.
//
// One workgroup per mask.  Every operation depends on the one before it, so the mask stays packed one bit per pixel (32-bit words,
// rows padded to whole words, bit k of word j = pixel 32 j + k) in three planes - seg, a scratch plane, g - for the whole walk:
//   placement 1  the planes in LDS (3 x 38 KB at 640 x 480), when they fit the 160 KB one workgroup may declare
//   placement 2  the planes in a per-mask workspace in device memory (1280 x 720, 1024 x 1024, 800 x 1333 ...)
// both instantiated from one kernel body.  An operation:
//   - every row of a structuring element is one contiguous run of columns [a, b) (a rectangle, or a row of cv::getStructuringElement's
//     ellipse), so dst word = OR over the element's rows of a horizontal run-OR of the source row: a 96-bit window (left, own, right
//     word) shifted once and folded by doubling.  An erosion is the dilation of the complement (the element is not reflected in
//     either, as in OpenCV's formula).  The source is masked to the rectangle: beyond it a dilation sees 0, an erosion 1.
//   - phase 1 writes the rectangle's words into the scratch plane, phase 2 copies them back - each word by the thread that computed
//     it - with one barrier between the phases and one after.  The cleared pixel always lies inside its rectangle, so it is applied
//     to the source words as they are read and never stored.
//   - the runs of the next operation's element are computed by 15 threads during phase 2 (float64: the ellipse's sqrt and rint).
// After every round (ops_per_round operations) a block-wide popcount gives |seg & g|, |seg | g|, |seg|; thread 0 compares
// (|seg & g| + 1e-6) / (|seg | g| + 1e-6) with the target in float64 and writes the decision into one LDS word, which ALL threads read
// after a barrier: the loop over the operations is bounded by n_ops and is left by all threads together or by none.
// A malformed program cannot write outside the mask: rectangles are clipped to the frame, sizes clamped to 1..15, stores limited to
// the rectangle's bits.  Integer and bit arithmetic throughout; masks and reports are exact.
#include "common.h"

namespace quber {

constexpr int PT_T = 1024;
constexpr int PT_WAVES = PT_T / 64;
constexpr int PT_ROWS = 15;                               // rows (and columns) of the largest structuring element
// control words in front of the planes (LDS in both placements)
constexpr int PT_STOP = 0, PT_ROUNDS = 1, PT_SUM = 2 /* 3 */, PT_PART = 8 /* 3 x PT_WAVES */, PT_TAB = 64 /* 2 x 2 x 16 */, PT_CTL = 128;
constexpr size_t PT_LDS_MAX = 160 * 1024;

struct PtOp { int lx, ly, lw, lh, clear, dilate, kw, kh, cx, cy; };

// one program row (lx, ly, lw, lh, clear, dilate, size, choice), made safe: the rectangle clipped to the frame, the size clamped
__device__ __forceinline__ PtOp pt_parse(const int* __restrict__ p, int H, int W) {
    PtOp o;
    o.lx = min(max(p[0], 0), W); o.ly = min(max(p[1], 0), H);
    o.lw = min(max(p[2], 0), W); o.lh = min(max(p[3], 0), H);
    o.clear = p[4] != 0; o.dilate = p[5] != 0;
    const int size = min(max(p[6], 1), PT_ROWS), half = max(size / 2, 1), choice = p[7];
    o.kw = choice == 4 ? half : size;
    o.kh = choice == 3 ? half : size;
    o.cx = (o.lx + o.lw) / 2; o.cy = (o.ly + o.lh) / 2;
    return o;
}

// row i of the element of program row p: the run of columns [a, b) it sets (cv::getStructuringElement; choice 1 and anything outside
// 2..4: a rectangle)
__device__ inline void pt_run(const int* __restrict__ p, int H, int W, int i, int* __restrict__ tab) {
    const PtOp o = pt_parse(p, H, W);
    int a = 0, b = 0;
    if (i < o.kh) {
        const int choice = p[7];
        if (choice < 2 || choice > 4 || (o.kw == 1 && o.kh == 1)) {
            b = o.kw;
        } else {
            const int r = o.kh / 2, c = o.kw / 2, dy = i - r;
            const double inv = r ? 1.0 / ((double)r * r) : 0.0;
            if (abs(dy) <= r) {
                const int dx = (int)rint((double)c * sqrt((double)(r * r - dy * dy) * inv));
                a = max(c - dx, 0);
                b = min(c + dx + 1, o.kw);
            }
        }
    }
    tab[2 * i] = a; tab[2 * i + 1] = b;
}

// bits of word wx that lie in the columns [lx, lw)
__device__ __forceinline__ unsigned pt_colmask(int wx, int lx, int lw) {
    const int lo = max(lx - 32 * wx, 0), hi = min(lw - 32 * wx, 32);
    if (hi <= lo) return 0u;
    return (hi == 32 ? ~0u : (1u << hi) - 1u) & ~((1u << lo) - 1u);
}

// |seg & g|, |seg | g|, |seg| of the whole mask into ctl[PT_SUM ..] (thread 0 holds them on return; not yet published by a barrier)
__device__ inline void pt_count(const unsigned* seg, const unsigned* g, int words, unsigned* ctl) {
    const int t = threadIdx.x;
    unsigned ci = 0, cu = 0, cs = 0;
    for (int i = t; i < words; i += PT_T) {
        const unsigned s = seg[i], q = g[i];
        ci += __popc(s & q); cu += __popc(s | q); cs += __popc(s);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { ci += __shfl_down(ci, o); cu += __shfl_down(cu, o); cs += __shfl_down(cs, o); }
    if ((t & 63) == 0) {
        unsigned* part = ctl + PT_PART + 3 * (t >> 6);
        part[0] = ci; part[1] = cu; part[2] = cs;
    }
    __syncthreads();
    if (t == 0) {
        ci = cu = cs = 0;
        for (int w = 0; w < PT_WAVES; ++w) { ci += ctl[PT_PART + 3 * w]; cu += ctl[PT_PART + 3 * w + 1]; cs += ctl[PT_PART + 3 * w + 2]; }
        ctl[PT_SUM] = ci; ctl[PT_SUM + 1] = cu; ctl[PT_SUM + 2] = cs;
    }
}

// grid (B * N masks).  LDS: PT_CTL control words [+ the three planes].  ws: the planes of every mask, placement 2 only.
template <bool LDS>
__global__ __launch_bounds__(PT_T) void perturb_kernel(const uint8_t* __restrict__ masks, const int* __restrict__ programs,
                                                       const double* __restrict__ targets, uint8_t* __restrict__ out,
                                                       unsigned* __restrict__ report, unsigned* __restrict__ ws, int H, int W, int wpr, int n_ops,
                                                       int opr) {
    extern __shared__ unsigned pt_smem[];
    unsigned* ctl = pt_smem;
    const int m = blockIdx.x, t = threadIdx.x, words = H * wpr;
    unsigned* seg = LDS ? pt_smem + PT_CTL : ws + (size_t)m * 3 * words;
    unsigned* tmp = seg + words;
    unsigned* g = tmp + words;
    const uint8_t* src = masks + (size_t)m * H * W;
    const int* prog = programs + (size_t)m * n_ops * 8;
    int* tab = reinterpret_cast<int*>(ctl + PT_TAB);

    // threshold and pack: seg = mask > 127, g = mask != 0; the bits beyond W stay 0 for good
    for (int i = t; i < words; i += PT_T) {
        const int y = i / wpr, x0 = (i - y * wpr) * 32, nb = min(32, W - x0);
        const uint8_t* p = src + (size_t)y * W + x0;
        unsigned s = 0, q = 0;
        for (int k = 0; k < nb; ++k) {
            const unsigned v = p[k];
            s |= (unsigned)(v > 127u) << k;
            q |= (unsigned)(v != 0u) << k;
        }
        seg[i] = s; g[i] = q;
    }
    if (t < PT_ROWS && n_ops > 0) pt_run(prog, H, W, t, tab);
    __syncthreads();
    pt_count(seg, g, words, ctl);
    const int n_rounds = n_ops / opr;
    if (t == 0) {
        unsigned stop = 0, rounds = 0;
        if (H <= 2 || W <= 2 || n_rounds == 0) {
            stop = 1;                                        // perturb_seg's "rare case": the thresholded mask, no round
        } else if (ctl[PT_SUM + 2] == 0) {                   // an empty mask stays empty: the IoU never changes
            stop = 1;
            rounds = (0.0 + 1e-6) / ((double)ctl[PT_SUM + 1] + 1e-6) < targets[m] ? 1u : (unsigned)n_rounds;
        }
        ctl[PT_STOP] = stop; ctl[PT_ROUNDS] = rounds;
    }
    __syncthreads();

    for (int op = 0; op < n_ops; ++op) {
        if (ctl[PT_STOP]) break;                             // written before the last barrier: every thread reads the same word
        const PtOp o = pt_parse(prog + (size_t)op * 8, H, W);
        const int* runs = tab + (op & 1) * 32;
        const bool some = o.lw > o.lx && o.lh > o.ly;
        const int wx0 = o.lx >> 5, nw = some ? ((o.lw - 1) >> 5) - wx0 + 1 : 0, total = nw * (o.lh - o.ly);
        const int r = o.kh / 2, c = o.kw / 2, cwx = o.cx >> 5;
        const unsigned cbit = o.clear ? 1u << (o.cx & 31) : 0u;
        for (int k = t; k < total; k += PT_T) {              // phase 1: the rectangle's words into the scratch plane
            const int yy = k / nw, wx = wx0 + k - yy * nw, y = o.ly + yy;
            const unsigned m0 = pt_colmask(wx - 1, o.lx, o.lw), m1 = pt_colmask(wx, o.lx, o.lw), m2 = pt_colmask(wx + 1, o.lx, o.lw);
            unsigned acc = 0;
            for (int i = 0; i < o.kh; ++i) {
                const int a = runs[2 * i], b = runs[2 * i + 1], ys = y + i - r;
                if (b <= a || ys < o.ly || ys >= o.lh) continue;
                const unsigned* row = seg + ys * wpr;
                unsigned v0 = m0 ? row[wx - 1] : 0u, v1 = row[wx], v2 = m2 ? row[wx + 1] : 0u;
                if (ys == o.cy) {                            // the cleared pixel, applied on the fly
                    if (cwx == wx - 1) v0 &= ~cbit;
                    if (cwx == wx) v1 &= ~cbit;
                    if (cwx == wx + 1) v2 &= ~cbit;
                }
                if (!o.dilate) { v0 = ~v0; v1 = ~v1; v2 = ~v2; }
                v0 &= m0; v1 &= m1; v2 &= m2;
                // dst bit x = OR over dx in [a - c, b - 1 - c] of source bit x + dx: bit 32 + x + dx of the window v0 | v1 << 32 | v2 << 64
                const int s0 = 32 + a - c, len = b - a;      // s0 in 25..32, len in 1..15
                unsigned long long w = (((unsigned long long)v1 << 32 | v0) >> s0) | ((unsigned long long)v2 << (64 - s0));
                int s = 1;
                while (2 * s <= len) { w |= w >> s; s *= 2; }
                if (len > s) w |= w >> (len - s);
                acc |= (unsigned)w;
            }
            const int idx = y * wpr + wx;
            tmp[idx] = (seg[idx] & ~m1) | ((o.dilate ? acc : ~acc) & m1);
        }
        __syncthreads();
        for (int k = t; k < total; k += PT_T) {              // phase 2: back, each word by the thread that wrote it
            const int yy = k / nw, idx = (o.ly + yy) * wpr + wx0 + k - yy * nw;
            seg[idx] = tmp[idx];
        }
        if (!some && cbit && t == 0 && o.cy < H && o.cx < W) seg[o.cy * wpr + cwx] &= ~cbit;       // (malformed programs only)
        if (t < PT_ROWS && op + 1 < n_ops) pt_run(prog + (size_t)(op + 1) * 8, H, W, t, tab + ((op + 1) & 1) * 32);
        __syncthreads();
        if ((op + 1) % opr == 0) {
            pt_count(seg, g, words, ctl);
            if (t == 0) {
                const double iou = ((double)ctl[PT_SUM] + 1e-6) / ((double)ctl[PT_SUM + 1] + 1e-6);
                ctl[PT_ROUNDS] = (unsigned)((op + 1) / opr);
                ctl[PT_STOP] = iou < targets[m] ? 1u : 0u;
            }
            __syncthreads();
        }
    }

    // unpack to 0 / 255; one byte per thread and store, consecutive lanes consecutive bytes (any alignment of `out`)
    uint8_t* dst = out + (size_t)m * H * W;
    for (int i = t; i < H * W; i += PT_T) {
        const int y = i / W, x = i - y * W;
        dst[i] = (seg[y * wpr + (x >> 5)] >> (x & 31)) & 1u ? 255 : 0;
    }
    if (report && t < 4) report[(size_t)m * 4 + t] = t == 0 ? ctl[PT_ROUNDS] : ctl[PT_SUM + t - 1];
}

static size_t pt_plane_words(int H, int W) { return (size_t)H * ((W + 31) / 32); }
bool perturb_fits_lds(int H, int W) { return PT_CTL * 4 + 3 * 4 * pt_plane_words(H, W) <= PT_LDS_MAX; }
size_t perturb_ws_bytes(long n_masks, int H, int W) { return (size_t)n_masks * 3 * 4 * pt_plane_words(H, W); }

// lds != 0: the planes in LDS (the caller has checked perturb_fits_lds); else in `ws`, sized by perturb_ws_bytes for >= n_masks masks
int launch_perturb(const uint8_t* masks, long n_masks, int H, int W, const int* programs, int n_ops, int ops_per_round, const double* targets,
                   uint8_t* out, unsigned* report, int lds, void* ws, hipStream_t st) {
    if (n_masks <= 0) return 0;
    if (H < 1 || W < 1 || (long)H * W > 0x7fffffffL || pt_plane_words(H, W) > 0x7fffffffUL / 3) return fail("perturb: frame out of range");
    if (n_masks > 0x7fffffffL) return fail("perturb: more than 2^31 - 1 masks");
    if (n_ops < 0 || ops_per_round < 1 || n_ops % ops_per_round) return fail("perturb: n_ops must be a multiple of ops_per_round >= 1");
    if (!masks || !out || !targets || (!programs && n_ops > 0)) return fail("perturb: null tensor");
    if (lds ? !perturb_fits_lds(H, W) : !ws) return fail("perturb: no room for the bit planes");
    const int wpr = (W + 31) / 32;
    const double px = (double)n_masks * H * W;
    ProfScope prof("perturb", 2.0 * px + 32.0 * n_masks * n_ops, 0.0, st);
    if (lds) {
        const size_t bytes = PT_CTL * 4 + 3 * 4 * pt_plane_words(H, W);
        // the attribute is per device: set it on every call
        QB_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(perturb_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)PT_LDS_MAX));
        hipLaunchKernelGGL(perturb_kernel<true>, dim3((unsigned)n_masks), dim3(PT_T), bytes, st, masks, programs, targets, out, report,
                           (unsigned*)nullptr, H, W, wpr, n_ops, ops_per_round);
    } else {
        hipLaunchKernelGGL(perturb_kernel<false>, dim3((unsigned)n_masks), dim3(PT_T), PT_CTL * 4, st, masks, programs, targets, out, report,
                           reinterpret_cast<unsigned*>(ws), H, W, wpr, n_ops, ops_per_round);
    }
    QB_CHECK(hipGetLastError());
    return 0;
}

}  // namespace quber
