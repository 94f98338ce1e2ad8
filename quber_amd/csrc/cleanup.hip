// Connected-component clean-up of a compact instance map on the device (include/quber_hip.h: quber_cleanup_ids,
// quber_cleanup_postprocess; the definition is in INTEGRATION.md "Connected-component clean-up").
//   step 1, islands: per instance, the c-connected components of {ids == i}; all but the largest (keep_largest) or all smaller than
//                    min_island_area (the largest always stays) become void
//   step 2, holes:   the c-connected components of {ids == 0} of the map step 1 left; one smaller than max_hole_area whose
//                    neighbours all carry one id takes that id
// Replaces the host loops the competing refiners of the reference run over their masks: largest_connected_component
// (eval/utilities.py:726-748) and remove_small_regions (eval/refiner_model.py:526-549).
//
// Labelling is the lock-free union-find of csrc/inpaint_dev.hip (file-local there): a link only ever goes from a larger pixel index
// to a smaller one (atomicMin), so a root is the first pixel of its component in raster order, no thread waits for another, and every
// loop is bounded by the length of a parent chain.  A phase is four launches on the caller's stream - seed, union, flatten, decide +
// apply - with nothing but the stream order between them: no grid-wide barrier, no cooperative launch.  Frames never interact: a
// pixel's neighbours are taken inside its own frame.
//   seed     parent = the start of the pixel's row run inside its wave (one ballot; a run crossing a wave border is joined by the
//            union pass), -1 for the phase's background; the per-root accumulators are cleared here, by their own pixel
//   union    the raster neighbours already visited (left, up; the two upper diagonals for c = 8) of equal id, minus the pairs another
//            pixel's links already join (cc_union_kernel) - inside an object no atomic is left
//   flatten  parent = root; area at the root (one add per wave whose lanes share it); phase 2: min / max of the neighbour ids
//   decide   phase 1: one 64-bit atomicMax of (area << 32) | (0xffffffff - root) per root and instance = the largest component, the
//            first in raster order among equals; then the pixels are rewritten
// Integer arithmetic only: ids and the report are exact and independent of the order the atomics arrive in.  The counters are cleared
// by launch_zero (memset nodes do not replay in a captured graph), so a call overwrites its outputs.
#include <limits.h>

#include "common.h"

namespace quber {

constexpr int CC_T = 256;
constexpr int CC_BINS = 256;                             // ids 0..254 per frame

__device__ __forceinline__ int cc_id(int v, int n_ids) { return (unsigned)v <= (unsigned)n_ids ? v : 0; }

__device__ inline int cc_find(const int* parent, int x) {
    int r = x;
    while (true) {
        const int p = parent[r];
        if (p == r) return r;
        r = p;
    }
}
__device__ inline void cc_union(int* parent, int x, int y) {
    for (;;) {
        x = cc_find(parent, x);
        y = cc_find(parent, y);
        if (x == y) return;
        if (x < y) { const int t = x; x = y; y = t; }        // x > y: link x under y
        const int old = atomicMin(&parent[x], y);
        if (old == x) return;
        x = old;                                             // somebody else linked x meanwhile: continue from there
    }
}

// grid (ceil(HW / CC_T), B): lane l of a wave owns pixel 64 * k + l of its frame, so the lanes of a wave are consecutive pixels.
// phase 1: the pixels with an id are labelled, equal ids connect; phase 2: the void pixels (the map is in range by then).
__global__ __launch_bounds__(CC_T) void cc_seed_kernel(const int* __restrict__ ids, int* __restrict__ parent, unsigned* __restrict__ area,
                                                       int* __restrict__ nmin, int* __restrict__ nmax, int n_ids, int HW, int W, int phase) {
    const int q = blockIdx.x * CC_T + threadIdx.x, lane = threadIdx.x & 63;
    const bool in = q < HW;
    const long g = (long)blockIdx.y * HW + q;
    const int id = in ? cc_id(ids[g], n_ids) : 0;
    const bool act = in && (phase == 1 ? id != 0 : id == 0);
    const bool cont = act && q % W != 0 && cc_id(ids[g - 1], n_ids) == id;       // continues the run of its left neighbour
    // a lane that continues a run has an active left neighbour of the same id: down to the nearest start (or lane 0) the run is unbroken
    const unsigned long long starts = __ballot(act && !cont) | 1ull;
    if (!in) return;
    int par = -1;
    if (act) par = (int)g - (lane - (63 - __clzll((long long)(starts & (~0ull >> (63 - lane))))));
    parent[g] = par;
    area[g] = 0u;
    if (phase == 2) { nmin[g] = INT_MAX; nmax[g] = 0; }
}

// With L / U / UL / UR the left, upper, upper-left and upper-right neighbour of equal id: L is always joined (by the seed inside a
// wave, here across its border).  By induction over the raster order every pixel is connected to each of its visited neighbours:
//   c = 4: U is skipped when L and UL exist (p - L by its own link, L - UL by induction, UL - U as row neighbours);
//   c = 8: U is skipped when L exists (U is L's upper-right), UL when L or U exists (L's upper / U's left neighbour), UR when U
//          exists (its row neighbour).
__global__ __launch_bounds__(CC_T) void cc_union_kernel(const int* __restrict__ ids, int* parent, int n_ids, int HW, int W,
                                                        int conn) {
    const int q = blockIdx.x * CC_T + threadIdx.x;
    if (q >= HW) return;
    const long g = (long)blockIdx.y * HW + q;
    if (parent[g] < 0) return;
    const int id = cc_id(ids[g], n_ids);
    const int y = q / W, x = q - y * W;
    const bool L = x > 0 && cc_id(ids[g - 1], n_ids) == id;
    const bool U = y > 0 && cc_id(ids[g - W], n_ids) == id;
    const bool UL = y > 0 && x > 0 && cc_id(ids[g - W - 1], n_ids) == id;
    if (L && (threadIdx.x & 63) == 0) cc_union(parent, (int)g, (int)g - 1);
    if (conn == 4) {
        if (U && !(L && UL)) cc_union(parent, (int)g, (int)g - W);
    } else {
        const bool UR = y > 0 && x + 1 < W && cc_id(ids[g - W + 1], n_ids) == id;
        if (U && !L) cc_union(parent, (int)g, (int)g - W);
        if (UL && !L && !U) cc_union(parent, (int)g, (int)g - W - 1);
        if (UR && !U) cc_union(parent, (int)g, (int)g - W + 1);
    }
}

__global__ __launch_bounds__(CC_T) void cc_flatten_kernel(const int* __restrict__ ids, int* parent, unsigned* __restrict__ area,
                                                          int* __restrict__ nmin, int* __restrict__ nmax, int H, int W, int conn, int phase) {
    const int HW = H * W;
    const int q = blockIdx.x * CC_T + threadIdx.x, lane = threadIdx.x & 63;
    const long g = (long)blockIdx.y * HW + q;
    const bool act = q < HW && parent[g] >= 0;
    int r = -1;
    if (act) {
        r = cc_find(parent, (int)g);
        parent[g] = r;                                       // (roots never change any more: every union is done)
    }
    const unsigned long long m = __ballot(act);
    if (m == 0) return;
    const int lead = __ffsll((long long)m) - 1;
    const int first = __shfl(r, lead);
    if (__all(!act || r == first)) {
        if (lane == lead) atomicAdd(&area[first], (unsigned)__popcll(m));
    } else if (act) {
        atomicAdd(&area[r], 1u);
    }
    if (phase == 2 && act) {                                 // the ids around a void pixel (never void themselves outside its component)
        const int y = q / W, x = q - y * W;
        int mn = INT_MAX, mx = 0;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                if ((dy == 0 && dx == 0) || (conn == 4 && dy != 0 && dx != 0)) continue;
                const int yy = y + dy, xx = x + dx;
                if ((unsigned)yy >= (unsigned)H || (unsigned)xx >= (unsigned)W) continue;
                const int v = ids[g + dy * W + dx];
                if (v != 0) { mn = min(mn, v); mx = max(mx, v); }
            }
        if (mx) { atomicMin(&nmin[r], mn); atomicMax(&nmax[r], mx); }
    }
}

// report rows: [B][n_ids + 1][4] = components, pixels removed, pixels gained, final area (row 0: void components examined, 0, pixels
// filled, final void area)
__device__ __forceinline__ unsigned* cc_rep(unsigned* rep, int b, int n_ids, int id, int col) { return rep + ((long)b * (n_ids + 1) + id) * 4 + col; }

__global__ __launch_bounds__(CC_T) void cc_best_kernel(const int* __restrict__ ids, const int* __restrict__ parent, const unsigned* __restrict__ area,
                                                       unsigned long long* __restrict__ best, unsigned* __restrict__ rep, int n_ids, int HW) {
    const int q = blockIdx.x * CC_T + threadIdx.x, b = blockIdx.y;
    if (q >= HW) return;
    const long g = (long)b * HW + q;
    if (parent[g] != (int)g) return;
    const int id = cc_id(ids[g], n_ids);
    atomicMax(&best[b * CC_BINS + id], (unsigned long long)area[g] << 32 | (0xffffffffu - (unsigned)q));
    atomicAdd(cc_rep(rep, b, n_ids, id, 0), 1u);
}

__global__ __launch_bounds__(CC_T) void cc_islands_kernel(int* __restrict__ ids, const int* __restrict__ parent, const unsigned* __restrict__ area,
                                                          const unsigned long long* __restrict__ best, unsigned* __restrict__ rep, int n_ids,
                                                          int HW, int keep_largest, unsigned min_island) {
    const int q = blockIdx.x * CC_T + threadIdx.x, b = blockIdx.y;
    if (q >= HW) return;
    const long g = (long)b * HW + q;
    int id = cc_id(ids[g], n_ids);
    if (id) {
        const int r = parent[g];
        const unsigned first = 0xffffffffu - (unsigned)best[b * CC_BINS + id];      // the instance's largest component, as a pixel of the frame
        const bool keep = (unsigned)(r - (int)((long)b * HW)) == first || (!keep_largest && area[r] >= min_island);
        if (!keep) {
            atomicAdd(cc_rep(rep, b, n_ids, id, 1), 1u);
            id = 0;
        }
    }
    ids[g] = id;                                             // (in range from here on)
}

__global__ __launch_bounds__(CC_T) void cc_holes_kernel(int* __restrict__ ids, const int* __restrict__ parent, const unsigned* __restrict__ area,
                                                        const int* __restrict__ nmin, const int* __restrict__ nmax, unsigned* __restrict__ rep,
                                                        int n_ids, int HW, unsigned max_hole) {
    const int q = blockIdx.x * CC_T + threadIdx.x, b = blockIdx.y;
    if (q >= HW) return;
    const long g = (long)b * HW + q;
    const int r = parent[g];
    if (r < 0) return;
    if (r == (int)g) atomicAdd(cc_rep(rep, b, n_ids, 0, 0), 1u);
    const int mn = nmin[r], mx = nmax[r];
    if (area[r] < max_hole && mx > 0 && mn == mx) {
        ids[g] = mn;
        atomicAdd(cc_rep(rep, b, n_ids, mn, 2), 1u);
        atomicAdd(cc_rep(rep, b, n_ids, 0, 2), 1u);
    }
}

// final areas: a block's pixels counted in LDS (one add per wave whose lanes agree), one global add per (block, id)
__global__ __launch_bounds__(CC_T) void cc_area_kernel(const int* __restrict__ ids, unsigned* __restrict__ rep, int n_ids, int HW) {
    __shared__ unsigned h[CC_BINS];
    const int q = blockIdx.x * CC_T + threadIdx.x, b = blockIdx.y, lane = threadIdx.x & 63;
    h[threadIdx.x] = 0;
    __syncthreads();
    const bool in = q < HW;
    const int id = in ? ids[(long)b * HW + q] : 0;
    const unsigned long long m = __ballot(in);
    if (m) {
        const int first = __shfl(id, __ffsll((long long)m) - 1);
        if (__all(!in || id == first)) {
            if (lane == 0) atomicAdd(&h[first], (unsigned)__popcll(m));
        } else if (in) {
            atomicAdd(&h[id], 1u);
        }
    }
    __syncthreads();
    if ((int)threadIdx.x <= n_ids && h[threadIdx.x]) atomicAdd(cc_rep(rep, b, n_ids, threadIdx.x, 3), h[threadIdx.x]);
}
static_assert(CC_T == CC_BINS, "cc_area_kernel: one thread per bin");

// workspace layout (bytes): ids | parent | area | nmin | nmax  i32 / u32 B*HW each | best u64 B*256 | report u32 B*255*4 | lut f32 B*256 | stats B*cap
struct CcWs {
    int *ids, *parent, *nmin, *nmax;
    unsigned* area;
    unsigned long long* best;
    unsigned* rep;
    float* lut;
    InstStat* stats;
};
static size_t cc_layout(CcWs* out, void* ws, int B, int H, int W, int cap) {
    const size_t px = (size_t)B * H * W;
    CcWs none, &c = out ? *out : none;
    WsWalk w{static_cast<char*>(ws)};
    c.ids = w.take<int>(px);
    c.parent = w.take<int>(px);
    c.area = w.take<unsigned>(px);
    c.nmin = w.take<int>(px);
    c.nmax = w.take<int>(px);
    c.best = w.take<unsigned long long>((size_t)B * CC_BINS);
    c.rep = w.take<unsigned>((size_t)B * 255 * 4);
    c.lut = w.take<float>((size_t)B * CC_BINS);
    c.stats = w.take<InstStat>((size_t)B * cap);
    return w.off;
}
size_t cleanup_ws_bytes(int B, int H, int W, int cap) { return cc_layout(nullptr, nullptr, B, H, W, cap); }

// `ws`: sized by cleanup_ws_bytes for a batch >= B of this frame size
int launch_cleanup_ids(int* ids, int B, int H, int W, int n_ids, int conn, int keep_largest, int min_island, int max_hole, void* ws,
                       unsigned* report, hipStream_t st) {
    if (B <= 0) return 0;
    if (B > 65535) return fail("cleanup: batch above 65535");
    if (n_ids < 0 || n_ids > 254) return fail("cleanup: n_ids outside 0..254");
    if (conn != 4 && conn != 8) return fail("cleanup: connectivity must be 4 or 8");
    if (keep_largest != 0 && keep_largest != 1) return fail("cleanup: keep_largest must be 0 or 1");
    if (min_island < 0 || max_hole < 0) return fail("cleanup: negative area");
    const long HW = (long)H * W;
    if (HW < 1 || (long)B * HW > 0x7fffffffL) return fail("cleanup: more than 2^31 - 1 pixels");
    if (!ids || !ws) return fail("cleanup: null tensor");
    CcWs c;
    cc_layout(&c, ws, B, H, W, 0);           // (stats is the last field and not used here: its length does not matter)
    unsigned* rep = report ? report : c.rep;
    const dim3 grid((unsigned)((HW + CC_T - 1) / CC_T), (unsigned)B), blk(CC_T);
    const double px = (double)B * (double)HW;
    if (int rc = launch_zero(c.best, (size_t)B * CC_BINS * 8, st)) return rc;
    if (int rc = launch_zero(rep, (size_t)B * (n_ids + 1) * 16, st)) return rc;
    for (int phase = 1; phase <= (max_hole > 0 ? 2 : 1); ++phase) {
        {   // id map in; parent map and the per-root tables out, parent map in and out twice more
            ProfScope prof("cleanup_label", (phase == 1 ? 28.0 : 36.0) * px, 0.0, st);
            hipLaunchKernelGGL(cc_seed_kernel, grid, blk, 0, st, ids, c.parent, c.area, c.nmin, c.nmax, n_ids, (int)HW, W, phase);
            hipLaunchKernelGGL(cc_union_kernel, grid, blk, 0, st, ids, c.parent, n_ids, (int)HW, W, conn);
            hipLaunchKernelGGL(cc_flatten_kernel, grid, blk, 0, st, ids, c.parent, c.area, c.nmin, c.nmax, H, W, conn, phase);
        }
        {
            ProfScope prof("cleanup_apply", (phase == 1 ? 24.0 : 12.0) * px, 0.0, st);
            if (phase == 1) {
                hipLaunchKernelGGL(cc_best_kernel, grid, blk, 0, st, ids, c.parent, c.area, c.best, rep, n_ids, (int)HW);
                hipLaunchKernelGGL(cc_islands_kernel, grid, blk, 0, st, ids, c.parent, c.area, c.best, rep, n_ids, (int)HW, keep_largest,
                                   (unsigned)min_island);
            } else {
                hipLaunchKernelGGL(cc_holes_kernel, grid, blk, 0, st, ids, c.parent, c.area, c.nmin, c.nmax, rep, n_ids, (int)HW,
                                   (unsigned)max_hole);
            }
        }
    }
    {
        ProfScope prof("cleanup_apply", 4.0 * px, 0.0, st);
        hipLaunchKernelGGL(cc_area_kernel, grid, blk, 0, st, ids, rep, n_ids, (int)HW);
    }
    QB_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// quber_cleanup_postprocess: the label map of quber_postprocess -> compact ids (launch_relabel_panoptic, count read on the device) ->
// clean-up -> label map, scores and boxes over the cleaned masks by the post-processor's own paint / statistics / finalize kernels
// (launch_post_paint_finalize), which read the compact ids through a table id -> label.
// one block per frame: that table (id 1 + j -> the frame's j-th label, -1 elsewhere) and the cleared statistics
__global__ void cc_lut_kernel(const float* __restrict__ labels, const int* __restrict__ count, int cap, float* __restrict__ lut,
                              InstStat* __restrict__ stats) {
    const int b = blockIdx.x;
    const int n = min(max(count[b], 0), cap);
    for (int i = threadIdx.x; i < CC_BINS; i += blockDim.x) lut[(long)b * CC_BINS + i] = (i >= 1 && i <= n) ? labels[(long)b * cap + i - 1] : -1.f;
    for (int i = threadIdx.x; i < cap; i += blockDim.x) {
        InstStat s;
        s.prob = 0.0; s.sy = 0; s.sx = 0; s.cnt = 0;
        s.xmin = 1 << 30; s.ymin = 1 << 30; s.xmax = -1; s.ymax = -1; s.pad = 0;
        stats[(long)b * cap + i] = s;
    }
}

int launch_cleanup_postprocess(const float* logits, int nch, int B, int H, int W, int cap, int label_divisor, float* pan, const float* labels, const int* count,
                               float* scores, float* boxes, int conn, int keep_largest, int min_island, int max_hole, void* ws,
                               unsigned* report, hipStream_t st) {
    if (B <= 0) return 0;
    if (cap < 1 || cap > 254) return fail("cleanup_postprocess: top_k outside 1..254");
    if (nch < 2) return fail("cleanup_postprocess: logits need the foreground and centre planes");
    if (!logits || !pan || !labels || !count || !scores || !boxes || !ws) return fail("cleanup_postprocess: null tensor");
    CcWs c;
    cc_layout(&c, ws, B, H, W, cap);
    const long HW = (long)H * W;
    if (int rc = launch_relabel_panoptic(pan, labels, count, B, cap, 0, H, W, c.ids, st)) return rc;
    if (int rc = launch_cleanup_ids(c.ids, B, H, W, cap, conn, keep_largest, min_island, max_hole, ws, report, st)) return rc;
    {   // id map + fg plane in, label map out, per-instance sums
        ProfScope prof("cleanup_apply", 12.0 * B * (double)HW, 0.0, st);
        hipLaunchKernelGGL(cc_lut_kernel, dim3(B), dim3(256), 0, st, labels, count, cap, c.lut, c.stats);
        if (int rc = launch_post_paint_finalize(logits, nch, B, H, W, cap, label_divisor, c.ids, c.lut, count, pan, c.stats, scores, boxes, st)) return rc;
    }
    return 0;
}

}  // namespace quber
