// Evaluation support (boundary half): the boundary precision / recall counts of
// eval/evaluation.py:21-54 `boundary_overlap` for every (ground-truth object, predicted object) pair, and the per-object
// boundary sizes of evaluation.py:165-175, in three launches on bit planes.
//
//   reference, per pair (i, j):  fg_b = seg2bmap(pred_j); gt_b = seg2bmap(gt_i);                    (utilities.py:672-697)
//                                gt_d = cv2.dilate(gt_b, disk(r)); fg_d = cv2.dilate(fg_b, disk(r))
//                                precision_tps = |fg_b & gt_d|,  recall_tps = |gt_b & fg_d|
//   seg2bmap = cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_NONE) + drawContours(thickness 1).  OpenCV is not in the image;
//   restated from the published border-following algorithm (Suzuki & Abe): with 8-connected objects the outer border of a
//   component is the set of its pixels that are 4-adjacent to the background region surrounding it, and RETR_EXTERNAL keeps
//   only the components that are not nested inside a hole of another one - i.e. those whose surrounding background is the
//   frame-connected ("outside") background.  Hence
//       outside = 4-connected flood of the background from the image frame
//       bmap    = seg & (a 4-neighbour is outside, the frame counting as outside)
//   Parity unpinned (hand-derived cases + scipy restatement in oracle/metrics_np.py).
//
//   1. pack   label map == label  ->  one bit per pixel (one __ballot per 64 pixels)
//   2. bmap   one workgroup per object: flood fill in LDS (whole-word run fills + one-row / one-word hops per sweep, until
//             a sweep changes nothing), border bits, disk dilation as row-wise shifted ORs, popcounts
//   3. pairs  one workgroup per (gt, pred): popcount(fg_b & gt_d), popcount(gt_b & fg_d)
#include "common.h"
#include "evalbody.h"   // the kernel bodies, shared with the batched launches of evalbatch.hip

namespace quber {

static inline int bnd_wpr(int W) { return (W + 63) / 64; }

__global__ __launch_bounds__(256) void bnd_pack_kernel(const int* __restrict__ pred, const int* __restrict__ gt,
                                                       const int* __restrict__ labels, int n_pred, int H, int W, int wpr,
                                                       u64* __restrict__ seg) {
    const int m = blockIdx.y;
    bnd_pack_body(m < n_pred ? pred : gt, labels[m], H, W, wpr, seg + (long)m * H * wpr);
}

// grid (n objects); LDS: reach[H][wpr]
__global__ __launch_bounds__(1024) void bnd_bmap_kernel(const u64* __restrict__ seg, int H, int W, int wpr, int radius,
                                                        u64* __restrict__ bmap, u64* __restrict__ dil,
                                                        unsigned* __restrict__ counts) {
    const int m = blockIdx.x;
    const long n = (long)H * wpr;
    bnd_bmap_body(seg + m * n, H, W, wpr, radius, bmap + m * n, dil + m * n, counts + m);
}

// grid (n_pred, n_gt): out_fg[i][j] = |bmap_pred_j & dil_gt_i|, out_gt[i][j] = |bmap_gt_i & dil_pred_j|
__global__ __launch_bounds__(256) void bnd_pair_kernel(const u64* __restrict__ bmap, const u64* __restrict__ dil, int n,
                                                       int n_pred, unsigned* __restrict__ out_fg, unsigned* __restrict__ out_gt) {
    const int j = blockIdx.x, i = blockIdx.y;
    bnd_pair_body(bmap + (long)j * n, dil + (long)j * n, bmap + (long)(n_pred + i) * n, dil + (long)(n_pred + i) * n, n,
                  out_fg + (long)i * n_pred + j, out_gt + (long)i * n_pred + j);
}

size_t boundary_ws_bytes(int H, int W, int n_masks) { return (size_t)3 * n_masks * H * bnd_wpr(W) * sizeof(u64); }

// out: counts[n_pred + n_gt] | fg_match[n_gt][n_pred] | gt_match[n_gt][n_pred]   (u32)
int launch_boundary_overlap(const int* pred, const int* gt, int H, int W, const int* labels, int n_pred, int n_gt, int radius,
                            void* ws, unsigned* out, hipStream_t st) {
    const int wpr = bnd_wpr(W), nm = n_pred + n_gt;
    const size_t plane = (size_t)H * wpr * sizeof(u64);
    if (n_pred < 1 || n_gt < 1) return fail("boundary overlap: needs at least one object on each side");
    if (radius < 0 || radius > 63) return fail("boundary overlap: dilation radius must be 0..63");
    if (plane > 160 * 1024 - 64) return fail("boundary overlap: frame too large for the LDS flood fill (H * ceil(W/64) * 8 <= 160 KiB)");
    u64* seg = reinterpret_cast<u64*>(ws);
    u64* bmap = seg + (size_t)nm * H * wpr;
    u64* dil = bmap + (size_t)nm * H * wpr;
    hipLaunchKernelGGL(bnd_pack_kernel, dim3((unsigned)(((long)H * wpr + 3) / 4), nm), dim3(256), 0, st, pred, gt, labels, n_pred, H,
                       W, wpr, seg);
    QB_CHECK(hipGetLastError());
    // the attribute is per device (and this entry point may be called from several threads): set it on every call
    QB_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(bnd_bmap_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 160 * 1024 - 64));
    hipLaunchKernelGGL(bnd_bmap_kernel, dim3(nm), dim3(1024), plane, st, seg, H, W, wpr, radius, bmap, dil, out);
    QB_CHECK(hipGetLastError());
    hipLaunchKernelGGL(bnd_pair_kernel, dim3(n_pred, n_gt), dim3(256), 0, st, bmap, dil, H * wpr, n_pred, out + nm,
                       out + nm + (size_t)n_gt * n_pred);
    QB_CHECK(hipGetLastError());
    return 0;
}

}  // namespace quber
