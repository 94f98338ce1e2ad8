// Zoom-in refinement on the device (include/quber_hip.h: quber_zoom_rois, quber_zoom_crop, quber_zoom_paste; the definition is in
// INTEGRATION.md "Zoom-in refinement" and, as numpy, in tests/test_zoom_cpu.py: zoom_rois_np, zoom_crop_np, zoom_paste_np).  Restates the
// gather / scatter around the reference's second, zoomed-in pass - crop_rois and match_label_crop, eval/base_model.py:843-961 (copies at
// :1088 and :1192) - which run one mask at a time on the host side of torch (unique, nonzero, a .cpu() per paste).
//
// Stream-ordered launches, no host copy, no memset node; every output is overwritten by every call:
//   rois    zero -> extents (per id the tight x / y extent of its pixels: a block of 256 consecutive pixels reduces in LDS - only the
//           first and the last pixel of a run of equal ids in a row touch LDS, so the lanes of a wave rarely meet on one address - then
//           one atomicMax per used (block, id, side) into a zero-filled table of `extent + 1` values, 0 = absent) -> pad and clamp.
//   crop    one block per (slot, output row): the u8 bilinear resize (align_corners, exact rational weights) of BGR and depth and the
//           nearest gather of `ids == id` as 0 / 255.  Where the crop rows are 16-byte aligned a lane assembles a whole 16-byte word
//           and stores it once, else a lane per byte.
//   paste   zero -> keep (float32 overlap / area >= min_overlap per crop-pass instance) -> key (per crop the u64 sum / u32 count of
//           the positive channel-2 depths under its kept instances, block partials added atomically) -> order (one workgroup per
//           frame: the frame's slots, the paint order by counting with the keys compared as exact fractions) -> gather (per frame
//           pixel the LAST crop in paint order whose kept instance covers it under the nearest resize back to the ROI: deterministic,
//           no scatter; ROIs in LDS) -> compact (one workgroup per frame: final ids in paint order over the instances that kept a
//           pixel, source, scores, report) -> write (id map and the 0 / 255 planes) -> extents of the final map -> boxes.
// Integer arithmetic except the three named float32 expressions (padding, nearest index, overlap ratio), each evaluated with the
// correctly rounded intrinsics so that no contraction changes them.
#include "zoom_dev.h"

namespace quber {

// ---- extents --------------------------------------------------------------------------------------------------------------------------
// grid (ceil(HW / 256), B).  ext u32 [B][n][4], zero on entry: max over the pixels of id j + 1 of (W - x, H - y, x + 1, y + 1).
__global__ __launch_bounds__(ZM_T) void zm_extent_kernel(const int* __restrict__ ids, int n, int H, int W, unsigned* __restrict__ ext) {
    __shared__ unsigned s_ext[ZM_MAXID * 4];
    const int t = threadIdx.x, b = blockIdx.y;
    for (int k = t; k < n * 4; k += ZM_T) s_ext[k] = 0;
    __syncthreads();
    const long HW = (long)H * W, p = (long)blockIdx.x * ZM_T + t;
    if (p < HW) {
        const int* f = ids + (size_t)b * HW;
        const int id = f[p];
        if (id >= 1 && id <= n) {
            const int y = (int)(p / W), x = (int)(p - (long)y * W);
            const bool first = t == 0 || x == 0 || f[p - 1] != id;
            const bool last = t == ZM_T - 1 || x == W - 1 || f[p + 1] != id;       // (x < W - 1: p + 1 < HW)
            unsigned* e = s_ext + (id - 1) * 4;
            if (first) { atomicMax(e + 0, (unsigned)(W - x)); atomicMax(e + 1, (unsigned)(H - y)); atomicMax(e + 3, (unsigned)(y + 1)); }
            if (last) atomicMax(e + 2, (unsigned)(x + 1));
        }
    }
    __syncthreads();
    for (int k = t; k < n * 4; k += ZM_T)
        if (s_ext[k]) atomicMax(ext + (size_t)b * n * 4 + k, s_ext[k]);
}

// one lane per (frame, id): the padded, clamped box (x0, y0, x1, y1), inclusive; (0, 0, -1, -1) for an id without a pixel
__global__ __launch_bounds__(ZM_T) void zm_pad_kernel(const unsigned* __restrict__ ext, int total, int H, int W, float padding,
                                                      int* __restrict__ rois) {
    const int k = blockIdx.x * ZM_T + threadIdx.x;
    if (k >= total) return;
    const unsigned* e = ext + (size_t)k * 4;
    int4 r = make_int4(0, 0, -1, -1);
    if (e[2]) {
        const int x0 = W - (int)e[0], y0 = H - (int)e[1], x1 = (int)e[2] - 1, y1 = (int)e[3] - 1;
        const int px = (int)rintf(__fmul_rn((float)(x1 - x0), padding)), py = (int)rintf(__fmul_rn((float)(y1 - y0), padding));
        r = make_int4(max(x0 - px, 0), max(y0 - py, 0), min(x1 + px, W - 1), min(y1 + py, H - 1));
    }
    rois[(size_t)k * 4 + 0] = r.x; rois[(size_t)k * 4 + 1] = r.y; rois[(size_t)k * 4 + 2] = r.z; rois[(size_t)k * 4 + 3] = r.w;
}

// one lane per (frame, slot of max_inst): f32 (x_min, y_min, x_max + 1, y_max + 1) of the final mask, zeros for an absent id
__global__ __launch_bounds__(ZM_T) void zm_box_kernel(const unsigned* __restrict__ ext, int total, int H, int W, float* __restrict__ boxes) {
    const int k = blockIdx.x * ZM_T + threadIdx.x;
    if (k >= total) return;
    const unsigned* e = ext + (size_t)k * 4;
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e[2]) r = make_float4((float)(W - (int)e[0]), (float)(H - (int)e[1]), (float)e[2], (float)e[3]);
    boxes[(size_t)k * 4 + 0] = r.x; boxes[(size_t)k * 4 + 1] = r.y; boxes[(size_t)k * 4 + 2] = r.z; boxes[(size_t)k * 4 + 3] = r.w;
}

// ---- crop -----------------------------------------------------------------------------------------------------------------------------
// one output byte of the u8 bilinear resize: channel c of crop pixel dx on a row whose source rows and weights are (ya, yb, ry)
__device__ __forceinline__ unsigned zm_bil(const uint8_t* __restrict__ roi, int W, int w, int dx, int c, int d, const int ya, const int yb,
                                           const int ry) {
    const int tx = dx * (w - 1), xa = tx / d, rx = tx - xa * d, xb = min(xa + 1, w - 1);
    const unsigned p00 = roi[((size_t)ya * W + xa) * 3 + c], p01 = roi[((size_t)ya * W + xb) * 3 + c];
    const unsigned p10 = roi[((size_t)yb * W + xa) * 3 + c], p11 = roi[((size_t)yb * W + xb) * 3 + c];
    const unsigned num = (unsigned)(d - ry) * ((unsigned)(d - rx) * p00 + (unsigned)rx * p01) + (unsigned)ry * ((unsigned)(d - rx) * p10 + (unsigned)rx * p11);
    const unsigned dd = (unsigned)d * (unsigned)d;
    return (num + dd / 2) / dd;
}

// grid (S rows, T slots).  WORDS: a lane per 16-byte word of the three output rows (S % 16 == 0 and 16-byte aligned bases); else a lane
// per byte.  2 <= S <= 512.
template <bool WORDS>
__global__ __launch_bounds__(ZM_T) void zm_crop_kernel(const uint8_t* __restrict__ bgr, const uint8_t* __restrict__ depth, const int* __restrict__ ids,
                                                       const int* __restrict__ slots, const int* __restrict__ rois, int B, int n_ids, int H,
                                                       int W, int S, uint8_t* __restrict__ bgr_crop, uint8_t* __restrict__ depth_crop,
                                                       uint8_t* __restrict__ mask_crop) {
    const int dy = blockIdx.x, t = blockIdx.y;
    const ZmSlot s = zm_slot(slots, rois, t, B, n_ids, H, W);
    const int d = S - 1;
    const int row = 3 * S;                                   // bytes of an image row
    const int n_img = depth ? 2 : 1;
    const int unit = WORDS ? 16 : 1;
    const int items = (n_img * row + S) / unit;
    int ya = 0, yb = 0, ry = 0, my = 0;
    if (s.ok) {
        const int ty = dy * (s.h - 1);
        ya = ty / d; ry = ty - ya * d; yb = min(ya + 1, s.h - 1);
        my = zm_near(dy, s.h, S);
    }
    const size_t HW = (size_t)H * W;
    const size_t org = s.ok ? (size_t)s.b * HW + (size_t)s.y0 * W + s.x0 : 0;
    for (int it = threadIdx.x; it < items; it += ZM_T) {
        int o = it * unit;                                   // byte offset inside (bgr row | depth row | mask row)
        uint8_t* dst;
        int img;                                             // 0 bgr, 1 depth, 2 mask
        if (o < row) { img = 0; dst = bgr_crop + ((size_t)t * S + dy) * row + o; }
        else if (o < n_img * row) { img = 1; o -= row; dst = depth_crop + ((size_t)t * S + dy) * row + o; }
        else { img = 2; o -= n_img * row; dst = mask_crop + ((size_t)t * S + dy) * S + o; }
        unsigned v[WORDS ? 16 : 1];
#pragma unroll
        for (int k = 0; k < unit; ++k) {
            unsigned r = 0;
            if (s.ok) {
                if (img == 2) {
                    const int mx = zm_near(o + k, s.w, S);
                    r = ids[org + (size_t)my * W + mx] == s.id ? 255u : 0u;
                } else {
                    const int px = (o + k) / 3, c = (o + k) - px * 3;
                    r = zm_bil((img ? depth : bgr) + org * 3, W, s.w, px, c, d, ya, yb, ry);
                }
            }
            v[k] = r;
        }
        if (WORDS) {
            unsigned w4[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) w4[k] = v[4 * k] | v[4 * k + 1] << 8 | v[4 * k + 2] << 16 | v[4 * k + 3] << 24;
            *reinterpret_cast<uint4*>(dst) = make_uint4(w4[0], w4[1], w4[2], w4[3]);
        } else {
            *dst = (uint8_t)v[0];
        }
    }
}

// ---- paste ----------------------------------------------------------------------------------------------------------------------------
// one lane per (slot, crop-pass id 0..C): keep[t][i] = instance i >= 1 of a real crop exists and float32(overlap) / float32(area) >=
// min_overlap.  (overlap, area <= S * S <= 2^18 are exact in float32 and the division is correctly rounded, so for min_overlap = 0.5
// this is 2 * overlap >= area: rounding is monotonic and 0.5 is representable - the reference's `percentage < 0.5` drops the rest.)
__global__ __launch_bounds__(ZM_T) void zm_keep_kernel(const unsigned* __restrict__ table, const unsigned* __restrict__ area,
                                                       const int* __restrict__ slots, const int* __restrict__ rois, int B, int n_ids, int T, int C,
                                                       int H, int W, float min_overlap, uint8_t* __restrict__ keep) {
    const int k = blockIdx.x * ZM_T + threadIdx.x;
    if (k >= T * (C + 1)) return;
    const int t = k / (C + 1), i = k - t * (C + 1);
    bool kp = false;
    if (i >= 1 && area[k] > 0 && zm_slot(slots, rois, t, B, n_ids, H, W).ok) kp = __fdiv_rn((float)table[k], (float)area[k]) >= min_overlap;
    keep[k] = kp ? 1 : 0;
}

// grid (ceil(S * S / (256 * 8)), T).  ksum u64 [T], kcnt u32 [T], zero on entry.
__global__ __launch_bounds__(ZM_T) void zm_key_kernel(const int* __restrict__ crop_ids, const uint8_t* __restrict__ depth_crop,
                                                      const uint8_t* __restrict__ keep, int C, int SS, unsigned long long* __restrict__ ksum,
                                                      unsigned* __restrict__ kcnt) {
    __shared__ uint8_t s_keep[ZM_MAXID + 2];
    __shared__ unsigned s_sum, s_cnt;
    const int t = blockIdx.y;
    for (int i = threadIdx.x; i <= C; i += ZM_T) s_keep[i] = keep[(size_t)t * (C + 1) + i];
    if (threadIdx.x == 0) { s_sum = 0; s_cnt = 0; }
    __syncthreads();
    unsigned sum = 0, cnt = 0;
    const int p0 = blockIdx.x * ZM_T * 8;
    for (int k = 0; k < 8; ++k) {
        const int p = p0 + k * ZM_T + threadIdx.x;
        if (p < SS) {
            const int i = min(max(crop_ids[(size_t)t * SS + p], 0), C);
            const unsigned dep = depth_crop[((size_t)t * SS + p) * 3 + 2];
            if (s_keep[i] && dep) { sum += dep; ++cnt; }
        }
    }
    for (int o = 32; o > 0; o >>= 1) { sum += __shfl_down(sum, o); cnt += __shfl_down(cnt, o); }
    if ((threadIdx.x & 63) == 0 && cnt) { atomicAdd(&s_sum, sum); atomicAdd(&s_cnt, cnt); }      // <= 2048 * 255 per block: fits u32
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) { atomicAdd(ksum + t, (unsigned long long)s_sum); atomicAdd(kcnt + t, s_cnt); }
}

// grid (B), 256 lanes.  The slots of frame b are slots [start, start + n) (the list ascends by frame), n <= 254.  -> order i32 [B][254]
// (the slot painted r-th), ncrop i32 [B].  Keys: with_depth - the mean positive depth sum / cnt as an exact fraction, a crop without one
// first; else the ROI area; descending, equal keys in slot order.
__global__ __launch_bounds__(ZM_T) void zm_order_kernel(const int* __restrict__ slots, const int* __restrict__ rois, int B, int n_ids, int T,
                                                        int H, int W, int with_depth, const unsigned long long* __restrict__ ksum,
                                                        const unsigned* __restrict__ kcnt, int* __restrict__ order, int* __restrict__ ncrop) {
    __shared__ int s_start, s_n;
    __shared__ unsigned long long s_sum[ZM_MAXID];
    __shared__ unsigned s_cnt[ZM_MAXID];
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
    if (j < n) {
        const int t = min(start + j, T - 1);
        if (with_depth) { s_sum[j] = ksum[t]; s_cnt[j] = kcnt[t]; }
        else {
            const ZmSlot s = zm_slot(slots, rois, t, B, n_ids, H, W);
            s_sum[j] = s.ok ? (unsigned long long)s.w * s.h : 0;
            s_cnt[j] = 1;
        }
    }
    __syncthreads();
    if (j < n) {
        const unsigned long long sa = s_sum[j];
        const unsigned ca = s_cnt[j];
        int rank = 0;
        for (int q = 0; q < n; ++q) {
            const unsigned long long sq = s_sum[q];
            const unsigned cq = s_cnt[q];
            bool before, equal;                              // q is painted before j / has the same key
            if (cq == 0 || ca == 0) { before = cq == 0 && ca != 0; equal = cq == 0 && ca == 0; }
            else { const unsigned long long l = sq * ca, r = sa * cq; before = l > r; equal = l == r; }
            rank += before || (equal && q < j);
        }
        order[b * ZM_MAXID + rank] = start + j;
    }
    if (j == 0) ncrop[b] = n;
}

// grid (ceil(HW / 256), B).  keymap i32 [B][HW]: 0 or 1 + t * (C + 1) + i of the instance that owns the pixel; vis[t][i] = 1 for owners.
__global__ __launch_bounds__(ZM_T) void zm_gather_kernel(const int* __restrict__ crop_ids, const uint8_t* __restrict__ keep,
                                                         const int* __restrict__ slots, const int* __restrict__ rois, const int* __restrict__ order,
                                                         const int* __restrict__ ncrop, int B, int n_ids, int T, int C, int S, int H, int W,
                                                         int* __restrict__ keymap, unsigned* __restrict__ vis) {
    __shared__ int4 s_roi[ZM_MAXID];                         // x0, y0, w, h of the crop painted r-th (w = 0: not a crop)
    __shared__ int s_t[ZM_MAXID];
    const int b = blockIdx.y;
    const int n = min(max(ncrop[b], 0), ZM_MAXID);
    for (int r = threadIdx.x; r < n; r += ZM_T) {
        const int t = min(max(order[b * ZM_MAXID + r], 0), T - 1);
        const ZmSlot s = zm_slot(slots, rois, t, B, n_ids, H, W);
        s_t[r] = t;
        s_roi[r] = s.ok && s.b == b ? make_int4(s.x0, s.y0, s.w, s.h) : make_int4(0, 0, 0, 0);
    }
    __syncthreads();
    const long HW = (long)H * W, p = (long)blockIdx.x * ZM_T + threadIdx.x;
    if (p >= HW) return;
    const int y = (int)(p / W), x = (int)(p - (long)y * W);
    int key = 0;
    for (int r = n - 1; r >= 0; --r) {                       // the last painter wins: walk backwards, stop at the first hit
        const int4 q = s_roi[r];
        const int lx = x - q.x, ly = y - q.y;
        if (lx < 0 || ly < 0 || lx >= q.z || ly >= q.w) continue;
        const int t = s_t[r];
        const int sy = zm_near(ly, S, q.w), sx = zm_near(lx, S, q.z);
        const int i = min(max(crop_ids[((size_t)t * S + sy) * S + sx], 0), C);
        if (i && keep[(size_t)t * (C + 1) + i]) { key = 1 + t * (C + 1) + i; break; }
    }
    keymap[(size_t)b * HW + p] = key;
    if (key) vis[key - 1] = 1u;
}

// grid (B), 256 lanes.  Final ids 1.. in paint order, per crop in ascending crop-pass id, over the kept instances that own a pixel; at
// most max_inst.  -> outof i32 [T][C + 1] (final id or 0) for the frame's slots, source, scores, report (crops, kept, dropped, count).
__global__ __launch_bounds__(ZM_T) void zm_compact_kernel(const uint8_t* __restrict__ keep, const unsigned* __restrict__ vis,
                                                          const float* __restrict__ crop_scores, const int* __restrict__ slots,
                                                          const int* __restrict__ rois, const int* __restrict__ order, const int* __restrict__ ncrop,
                                                          int B, int n_ids, int T, int C, int H, int W, int max_inst, int* __restrict__ outof,
                                                          int* __restrict__ source, float* __restrict__ scores, int* __restrict__ report) {
    __shared__ int s_vis[ZM_MAXID], s_kept, s_crops;
    const int r = threadIdx.x, b = blockIdx.x;
    const int n = min(max(ncrop[b], 0), ZM_MAXID);
    if (r == 0) { s_kept = 0; s_crops = 0; }
    __syncthreads();
    int t = 0, id1 = 0;
    if (r < n) {
        t = min(max(order[b * ZM_MAXID + r], 0), T - 1);
        const ZmSlot s = zm_slot(slots, rois, t, B, n_ids, H, W);
        id1 = s.id;
        int v = 0, kp = 0;
        for (int i = 1; i <= C; ++i) {
            const size_t k = (size_t)t * (C + 1) + i;
            kp += keep[k];
            v += keep[k] && vis[k];
        }
        s_vis[r] = v;
        if (kp) atomicAdd(&s_kept, kp);
        if (s.ok) atomicAdd(&s_crops, 1);
    }
    __syncthreads();
    int total = 0;
    for (int q = 0; q < n; ++q) total += s_vis[q];
    const int count = min(total, max_inst);
    if (r < n) {
        int next = 0;
        for (int q = 0; q < r; ++q) next += s_vis[q];
        outof[(size_t)t * (C + 1)] = 0;
        for (int i = 1; i <= C; ++i) {
            const size_t k = (size_t)t * (C + 1) + i;
            int fid = 0;
            if (keep[k] && vis[k]) {
                if (next < max_inst) {
                    fid = next + 1;
                    source[((size_t)b * max_inst + next) * 2] = id1;
                    source[((size_t)b * max_inst + next) * 2 + 1] = i;
                    scores[(size_t)b * max_inst + next] = crop_scores[(size_t)t * C + i - 1];
                }
                ++next;
            }
            outof[k] = fid;
        }
    }
    for (int k = count + r; k < max_inst; k += ZM_T) {
        source[((size_t)b * max_inst + k) * 2] = -1;
        source[((size_t)b * max_inst + k) * 2 + 1] = -1;
        scores[(size_t)b * max_inst + k] = 0.f;
    }
    if (r < 4) report[b * 4 + r] = r == 0 ? s_crops : r == 1 ? s_kept : r == 2 ? s_kept - count : count;
}

// grid (ceil(HW / (256 * PIX)), B).  PIX = 16: HW % 16 == 0 and 16-byte aligned outputs; PIX = 1: any.
template <int PIX>
__global__ __launch_bounds__(ZM_T) void zm_write_kernel(const int* __restrict__ keymap, const int* __restrict__ outof, long n_keys, int N, long HW,
                                                        uint8_t* __restrict__ out_masks, int* __restrict__ ids) {
    const int b = blockIdx.y;
    const long p = ((long)blockIdx.x * ZM_T + threadIdx.x) * PIX;
    if (p >= HW) return;
    int id[PIX];
#pragma unroll
    for (int k = 0; k < PIX; ++k) {
        const long key = keymap[(size_t)b * HW + p + k];
        id[k] = key >= 1 && key <= n_keys ? outof[key - 1] : 0;
    }
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

// workspace layout for `cap_b` frames: ksum | ext | kcnt | vis (zeroed together, vis only as far as a call uses it) | keep | outof | order |
// ncrop | keymap
struct ZmWs { unsigned long long* ksum; unsigned* ext; unsigned* kcnt; unsigned* vis; uint8_t* keep; int* outof; int* order; int* ncrop; int* keymap; };

static size_t zm_layout(ZmWs* out, void* ws, int cap_b, int H, int W) {
    const size_t tc = (size_t)cap_b * ZM_MAXID, keys = tc * (ZM_MAXID + 1);
    ZmWs none, &r = out ? *out : none;
    WsWalk w{static_cast<char*>(ws)};
    r.ksum = w.take<unsigned long long>(tc, false);         // ksum .. vis: one range, cleared by one launch
    r.ext = w.take<unsigned>(tc * 4, false);
    r.kcnt = w.take<unsigned>(tc, false);
    r.vis = w.take<unsigned>(keys);
    r.keep = w.take<uint8_t>(keys);
    r.outof = w.take<int>(keys);
    r.order = w.take<int>(tc);
    r.ncrop = w.take<int>((size_t)cap_b);
    r.keymap = w.take<int>((size_t)cap_b * H * W);
    return w.off;
}

size_t zoom_ws_bytes(int cap_b, int H, int W) { return zm_layout(nullptr, nullptr, cap_b, H, W); }

static int zm_extents(const int* ids, int B, int n, int H, int W, unsigned* ext, hipStream_t st) {
    const long HW = (long)H * W;
    hipLaunchKernelGGL(zm_extent_kernel, dim3((unsigned)((HW + ZM_T - 1) / ZM_T), B), dim3(ZM_T), 0, st, ids, n, H, W, ext);
    QB_CHECK(hipGetLastError());
    return 0;
}

// ws: zoom_ws_bytes(>= B, H, W) bytes
int launch_zoom_rois(const int* ids, int B, int n_ids, int H, int W, float padding, int* rois, void* ws, int cap_b, hipStream_t st) {
    if (B <= 0 || n_ids == 0) return 0;
    ZmWs w;
    zm_layout(&w, ws, cap_b, H, W);
    ProfScope prof("zoom_rois", 4.0 * B * H * W + 32.0 * B * n_ids, 0.0, st);
    if (launch_zero(w.ext, (size_t)B * n_ids * 16, st)) return -1;
    if (zm_extents(ids, B, n_ids, H, W, w.ext, st)) return -1;
    hipLaunchKernelGGL(zm_pad_kernel, dim3((B * n_ids + ZM_T - 1) / ZM_T), dim3(ZM_T), 0, st, w.ext, B * n_ids, H, W, padding, rois);
    QB_CHECK(hipGetLastError());
    return 0;
}

int launch_zoom_crop(const uint8_t* bgr, const uint8_t* depth, const int* ids, const int* slots, const int* rois, int B, int n_ids, int T, int S,
                     int H, int W, uint8_t* bgr_crop, uint8_t* depth_crop, uint8_t* mask_crop, hipStream_t st) {
    if (T <= 0) return 0;
    ProfScope prof("zoom_crop", (depth ? 7.0 : 4.0) * T * S * S, 0.0, st);
    const bool words = S % 16 == 0 && (((uintptr_t)bgr_crop | (uintptr_t)depth_crop | (uintptr_t)mask_crop) & 15) == 0;
    const dim3 grid(S, T);
    if (words)
        hipLaunchKernelGGL(zm_crop_kernel<true>, grid, dim3(ZM_T), 0, st, bgr, depth, ids, slots, rois, B, n_ids, H, W, S, bgr_crop, depth_crop, mask_crop);
    else
        hipLaunchKernelGGL(zm_crop_kernel<false>, grid, dim3(ZM_T), 0, st, bgr, depth, ids, slots, rois, B, n_ids, H, W, S, bgr_crop, depth_crop, mask_crop);
    QB_CHECK(hipGetLastError());
    return 0;
}

int launch_zoom_paste(const int* crop_ids, const float* crop_scores, const unsigned* table, const unsigned* area, const uint8_t* depth_crop,
                      const int* slots, const int* rois, int B, int n_ids, int T, int S, int C, float min_overlap, int max_inst, int H, int W,
                      int* out_ids, uint8_t* out_masks, int* source, float* out_scores, float* boxes, int* report, void* ws, int cap_b,
                      hipStream_t st) {
    if (B <= 0) return 0;
    ZmWs w;
    zm_layout(&w, ws, cap_b, H, W);
    const long HW = (long)H * W;
    const size_t tc = (size_t)cap_b * ZM_MAXID, keys = (size_t)T * (C + 1);
    const int SS = S * S;
    ProfScope prof("zoom_paste", 4.0 * T * SS + (8.0 + max_inst) * B * HW, 0.0, st);
    if (launch_zero(w.ksum, tc * 28 + keys * 4, st)) return -1;                  // ksum, ext, kcnt and the used part of vis
    if (T > 0) {
        hipLaunchKernelGGL(zm_keep_kernel, dim3((unsigned)((keys + ZM_T - 1) / ZM_T)), dim3(ZM_T), 0, st, table, area, slots, rois, B, n_ids, T, C,
                           H, W, min_overlap, w.keep);
        if (depth_crop)
            hipLaunchKernelGGL(zm_key_kernel, dim3((SS + ZM_T * 8 - 1) / (ZM_T * 8), T), dim3(ZM_T), 0, st, crop_ids, depth_crop, w.keep, C, SS, w.ksum,
                               w.kcnt);
        QB_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(zm_order_kernel, dim3(B), dim3(ZM_T), 0, st, slots, rois, B, n_ids, T, H, W, depth_crop ? 1 : 0, w.ksum, w.kcnt, w.order, w.ncrop);
    hipLaunchKernelGGL(zm_gather_kernel, dim3((unsigned)((HW + ZM_T - 1) / ZM_T), B), dim3(ZM_T), 0, st, crop_ids, w.keep, slots, rois, w.order, w.ncrop,
                       B, n_ids, T, C, S, H, W, w.keymap, w.vis);
    hipLaunchKernelGGL(zm_compact_kernel, dim3(B), dim3(ZM_T), 0, st, w.keep, w.vis, crop_scores, slots, rois, w.order, w.ncrop, B, n_ids, T, C,
                       H, W, max_inst, w.outof, source, out_scores, report);
    QB_CHECK(hipGetLastError());
    if (HW % 16 == 0 && ((uintptr_t)out_masks & 15) == 0 && ((uintptr_t)out_ids & 15) == 0)
        hipLaunchKernelGGL(zm_write_kernel<16>, dim3((unsigned)((HW / 16 + ZM_T - 1) / ZM_T), B), dim3(ZM_T), 0, st, w.keymap, w.outof, (long)keys, max_inst,
                           HW, out_masks, out_ids);
    else
        hipLaunchKernelGGL(zm_write_kernel<1>, dim3((unsigned)((HW + ZM_T - 1) / ZM_T), B), dim3(ZM_T), 0, st, w.keymap, w.outof, (long)keys, max_inst, HW,
                           out_masks, out_ids);
    QB_CHECK(hipGetLastError());
    if (zm_extents(out_ids, B, max_inst, H, W, w.ext, st)) return -1;
    hipLaunchKernelGGL(zm_box_kernel, dim3((B * max_inst + ZM_T - 1) / ZM_T), dim3(ZM_T), 0, st, w.ext, B * max_inst, H, W, boxes);
    QB_CHECK(hipGetLastError());
    return 0;
}

}  // namespace quber
