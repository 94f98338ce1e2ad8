// COCO AP on the device: the per-frame half of COCOeval (include/quber_hip.h: quber_coco_match; the definition is in DESIGN.md "COCO AP"
// and, as numpy in plain loops, in tests/test_cocoap_cpu.py: coco_eval_img_np).  Restates computeIoU + evaluateImg of the published
// pycocotools algorithm and bbIou / rleIou of its maskApi.c for ONE category; accumulate and summarize stay on the host
// (quber_amd/eval/coco_ap.py): their input is the few KB per frame this file writes.
//
// Stream-ordered steps, no host copy, no synchronisation, no memset node:
//   rank    one workgroup per frame: the CA_TOP = 100 best detections by counting (score descending, index ascending, NaN = absent; no
//           sort network) -> order, scores, n_top; the present ground truths are counted -> n_gt_present.
//   zero    the pair table and the areas.
//   pack    (segm) only the ranked detection planes and the present ground-truth planes -> bit planes as in masknms.hip (bitplane.h; 32-bit words, rows
//           padded to whole words, planes padded to a multiple of 4 words); the planes of missing ranks and absent ground truths are
//           written as zero words.  The pixels of a plane are counted here: popc per lane, one wave reduction, one integer atomicAdd per
//           (wave, plane) - so that a frame without ground truths still has its detection areas.
//   boxes   (bbox) the boxes of the ranked detections and the ground truths, given or the tight box of the mask, into one table.
//   gram    (segm) inter[b][d][g] on the rectangular CA_TOP x n_gt table with the tile of masknms.hip's gram kernel (bitplane.h: mn_gram_tile): a block owns
//           CA_TILE ranks x CA_TILE ground truths and a chunk of CA_CHUNK words, stages CA_SLAB words of its two groups of planes per step,
//           every lane accumulates ONE pair with popc in a register (16 bytes per plane and LDS access; pitch CA_SLAB + 4 words, pitch / 4
//           odd: the 16 rows of a ds_read_b128 lane group start on 16 different 4-bank slots, lanes on one row read one address), one
//           integer atomicAdd per (block, pair).
//   iou     the float64 expressions of the contract, one division (__ddiv_rn) per pair; the areas as used.
//   Boundary IoU (quber_coco_match_boundary): behind pack, boundaryap.hip writes m & ~erode_d(m) of every plane into a second set of planes with
//           their areas, gram runs a second time on those into a second pair table (cleared by the same zero fill), and iou stores
//           min(mask iou, boundary iou) - the same expression on the two sets of integers; the areas stay the mask areas.
//   gorder  per (frame, area range): gi and the stable order "not ignored first" by counting.
//   match   one wave per (frame, area range, threshold): the greedy matching, detections in rank order, the lanes scanning gorder.
// Integer and bit arithmetic except the float64 expressions of `iou`; no floating-point atomics; every output byte is written by every call.
#include "bitplane.h"       // mn_plane_words, mn_pack_word, mn_gram_tile
#include "common.h"

namespace quber {

constexpr int CA_TOP = 100;                  // maxDets[-1]: detections of a frame that can ever count
constexpr int CA_TILE = 16;                  // planes per side of a gram tile; CA_TILE * CA_TILE lanes per block
constexpr int CA_DT_TILES = (CA_TOP + CA_TILE - 1) / CA_TILE;
constexpr int CA_SLAB = 64;                  // words of every plane staged per step
constexpr int CA_PITCH = CA_SLAB + 4;        // LDS row pitch in words: a multiple of 4 (16-byte reads), pitch / 4 odd
constexpr int CA_CHUNK = 1024;               // words of a plane per gram block: CA_CHUNK / CA_SLAB steps
constexpr int CA_MAX = 1024;                 // detections / ground truths per frame: one thread of the rank / gorder workgroup each
constexpr int CA_MAX_T = 16, CA_MAX_A = 8;   // thresholds, area ranges
constexpr uint8_t CA_ABSENT = 0xFF;          // gt_flags of a ground truth that is not there
static_assert(CA_TILE * CA_TILE == 256 && CA_SLAB % 4 == 0 && (CA_PITCH / 4) % 2 == 1 && CA_CHUNK % CA_SLAB == 0, "gram tile layout");
static_assert(CA_TILE * (CA_SLAB / 4) == 256, "one 16-byte piece per lane stages a slab of one group");
static_assert(CA_TOP <= CA_MAX, "the rank workgroup writes one slot per thread");

// grid (B), CA_MAX lanes.  counts i32 [B][2] = n_top, n_gt_present; order i32 [B][CA_TOP] (-1 behind n_top); out_scores f32 [B][CA_TOP] (0 behind)
__global__ __launch_bounds__(CA_MAX) void ca_rank_kernel(const float* __restrict__ scores, const uint8_t* __restrict__ gt_flags, int n_dt, int n_gt,
                                                         int* __restrict__ counts, int* __restrict__ order, float* __restrict__ out_scores) {
    __shared__ float s_score[CA_MAX];
    __shared__ int s_n[2];
    const int t = threadIdx.x, b = blockIdx.x;
    if (t < 2) s_n[t] = 0;
    if (t < n_dt) s_score[t] = scores[(size_t)b * n_dt + t];
    if (t < CA_TOP) { order[b * CA_TOP + t] = -1; out_scores[b * CA_TOP + t] = 0.f; }
    __syncthreads();
    if (t < n_dt) {
        const float s = s_score[t];
        if (s == s) {                                        // NaN: absent
            int ahead = 0;
            for (int j = 0; j < n_dt; ++j) {
                const float q = s_score[j];
                ahead += (q > s) || (q == s && j < t);
            }
            atomicAdd(&s_n[0], 1);
            if (ahead < CA_TOP) { order[b * CA_TOP + ahead] = t; out_scores[b * CA_TOP + ahead] = s; }
        }
    }
    if (t < n_gt && gt_flags[(size_t)b * n_gt + t] != CA_ABSENT) atomicAdd(&s_n[1], 1);
    __syncthreads();
    if (t < 2) counts[b * 2 + t] = t == 0 ? min(s_n[0], CA_TOP) : s_n[1];
}

// plane m of frame b: rank m (m < CA_TOP) or ground truth m - CA_TOP -> its input plane, or null when there is none
__device__ __forceinline__ const uint8_t* ca_plane_src(const uint8_t* dt, const uint8_t* gt, const int* order, const uint8_t* gt_flags, int b,
                                                       int m, int n_dt, int n_gt, size_t HW) {
    if (m < CA_TOP) {
        const int o = order[b * CA_TOP + m];
        return o >= 0 && o < n_dt ? dt + ((size_t)b * n_dt + o) * HW : nullptr;
    }
    const int g = m - CA_TOP;
    return gt_flags[(size_t)b * n_gt + g] != CA_ABSENT ? gt + ((size_t)b * n_gt + g) * HW : nullptr;
}

// grid (ceil(pw / 256), CA_TOP + n_gt, B).  One word per lane; planes u32 [B][CA_TOP + n_gt][pw]; area u32 [B][CA_TOP + n_gt], zero on entry.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void ca_pack_kernel(const uint8_t* __restrict__ dt, const uint8_t* __restrict__ gt, const int* __restrict__ order,
                                                      const uint8_t* __restrict__ gt_flags, int n_dt, int n_gt, int H, int W, int wpr, int pw,
                                                      unsigned* __restrict__ planes, unsigned* __restrict__ area) {
    const int i = blockIdx.x * 256 + threadIdx.x, m = blockIdx.y, b = blockIdx.z, P = CA_TOP + n_gt;
    const uint8_t* src = ca_plane_src(dt, gt, order, gt_flags, b, m, n_dt, n_gt, (size_t)H * W);
    const unsigned bits = src && i < H * wpr ? mn_pack_word<ALIGNED>(src, i, W, wpr) : 0u;
    if (i < pw) planes[((size_t)b * P + m) * pw + i] = bits;
    int c = __popc(bits);                                    // (every lane of the block gets here)
    for (int off = 32; off; off >>= 1) c += __shfl_xor(c, off);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(area + (size_t)b * P + m, (unsigned)c);
}

// grid (CA_TOP + n_gt, B), 256 lanes.  boxes f64 [B][CA_TOP + n_gt][4] = x, y, w, h: the given box, else the tight box of the mask
// (x0, y0, x1 + 1 - x0, y1 + 1 - y0; an empty mask: zeros), zeros where there is no plane.
__global__ __launch_bounds__(256) void ca_box_kernel(const uint8_t* __restrict__ dt, const uint8_t* __restrict__ gt, const double* __restrict__ dt_boxes,
                                                     const double* __restrict__ gt_boxes, const int* __restrict__ order,
                                                     const uint8_t* __restrict__ gt_flags, int n_dt, int n_gt, int H, int W,
                                                     double* __restrict__ boxes) {
    __shared__ int s_box[4];
    const int m = blockIdx.x, b = blockIdx.y, t = threadIdx.x, P = CA_TOP + n_gt;
    double* out = boxes + ((size_t)b * P + m) * 4;
    int idx;                                                 // the input index of plane m, -1: none
    if (m < CA_TOP) {
        idx = order[b * CA_TOP + m];
        if (idx >= n_dt) idx = -1;
    } else {
        idx = gt_flags[(size_t)b * n_gt + m - CA_TOP] != CA_ABSENT ? m - CA_TOP : -1;
    }
    const double* given = m < CA_TOP ? dt_boxes : gt_boxes;
    if (idx < 0 || given) {                                  // (uniform over the block)
        if (t < 4) out[t] = idx < 0 ? 0.0 : given[((size_t)b * (m < CA_TOP ? n_dt : n_gt) + idx) * 4 + t];
        return;
    }
    const uint8_t* src = (m < CA_TOP ? dt + ((size_t)b * n_dt + idx) * (size_t)H * W : gt + ((size_t)b * n_gt + idx) * (size_t)H * W);
    if (t < 4) s_box[t] = t == 0 ? W : t == 1 ? H : -1;
    __syncthreads();
    int x0 = W, y0 = H, x1 = -1, y1 = -1;
    for (int y = t / 64; y < H; y += 4)                      // one wave per row: consecutive bytes per lane group
        for (int x = t & 63; x < W; x += 64)
            if (src[(size_t)y * W + x]) { x0 = min(x0, x); x1 = max(x1, x); y0 = min(y0, y); y1 = max(y1, y); }
    if (x1 >= 0) { atomicMin(&s_box[0], x0); atomicMin(&s_box[1], y0); atomicMax(&s_box[2], x1); atomicMax(&s_box[3], y1); }
    __syncthreads();
    if (t < 4) {
        const bool any = s_box[2] >= 0;
        const int v = t == 0 ? s_box[0] : t == 1 ? s_box[1] : t == 2 ? s_box[2] + 1 - s_box[0] : s_box[3] + 1 - s_box[1];
        out[t] = any ? (double)v : 0.0;
    }
}

// grid (CA_DT_TILES * ceil(n_gt / CA_TILE), ceil(pw / CA_CHUNK), B), 256 lanes.  Lane t owns the pair (rank row t / 16 of its tile, ground
// truth t % 16 of its tile).  inter u32 [B][CA_TOP][n_gt], zero on entry.
__global__ __launch_bounds__(256) void ca_gram_kernel(const unsigned* __restrict__ planes, unsigned* __restrict__ inter, int n_gt, int pw) {
    __shared__ uint4 sm4[2 * CA_TILE * CA_PITCH / 4];
    unsigned* sm = reinterpret_cast<unsigned*>(sm4);
    const int ntg = (n_gt + CA_TILE - 1) / CA_TILE;
    const int ta = blockIdx.x / ntg, tb = blockIdx.x - ta * ntg;
    const int t = threadIdx.x, b = blockIdx.z;
    const int w0 = blockIdx.y * CA_CHUNK, w1 = min(w0 + CA_CHUNK, pw);
    const unsigned* base = planes + (size_t)b * (CA_TOP + n_gt) * pw;
    const int srow = t >> 4, ma = ta * CA_TILE + srow, mb = tb * CA_TILE + srow;      // the rank and the ground truth this lane stages
    const int ra = t >> 4, rb = t & 15;
    const unsigned acc = mn_gram_tile<CA_TILE, CA_SLAB, CA_PITCH>(ma < CA_TOP ? base + (size_t)ma * pw : nullptr,
                                                                  mb < n_gt ? base + (size_t)(CA_TOP + mb) * pw : nullptr, w0, w1, sm);
    const int i = ta * CA_TILE + ra, j = tb * CA_TILE + rb;
    if (i < CA_TOP && j < n_gt && acc) atomicAdd(inter + ((size_t)b * CA_TOP + i) * n_gt + j, acc);
}

// grid (ceil((CA_TOP + n_gt + CA_TOP * n_gt) / 256), B).  Element e of a frame: a detection area, a ground-truth area, or a pair.
//   dt_area f64 [B][CA_TOP] (0 behind n_top), gt_area f64 [B][n_gt] as used (the caller's where it is given and not NaN; 0 for an absent
//   one), iou f64 [B][CA_TOP][n_gt] (0 behind n_top and for an absent ground truth)
//   BOUNDARY: inter_b, area_b = the pair table and the areas of the boundary planes; iou = min(mask iou, boundary iou), the two ratios also
//   to mask_iou / bnd_iou f64 [B][CA_TOP][n_gt] where those are not null
template <bool BOUNDARY>
__global__ __launch_bounds__(256) void ca_iou_kernel(int bbox, const unsigned* __restrict__ inter, const unsigned* __restrict__ area,
                                                     const double* __restrict__ boxes, const int* __restrict__ counts,
                                                     const uint8_t* __restrict__ gt_flags, const double* __restrict__ gt_area_in, int n_gt,
                                                     double* __restrict__ dt_area, double* __restrict__ gt_area, double* __restrict__ iou,
                                                     const unsigned* __restrict__ inter_b, const unsigned* __restrict__ area_b,
                                                     double* __restrict__ mask_iou, double* __restrict__ bnd_iou) {
    const int b = blockIdx.y, P = CA_TOP + n_gt;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)P + (long)CA_TOP * n_gt) return;
    const int n_top = min(max(counts[b * 2], 0), CA_TOP);
    const double* bx = boxes + (size_t)b * P * 4;
    const unsigned* ar = area + (size_t)b * P;
    if (e < CA_TOP) {
        const int d = (int)e;
        dt_area[b * CA_TOP + d] = d >= n_top ? 0.0 : bbox ? __dmul_rn(bx[d * 4 + 2], bx[d * 4 + 3]) : (double)ar[d];
        return;
    }
    if (e < P) {
        const int g = (int)e - CA_TOP;
        double v = 0.0;
        if (gt_flags[(size_t)b * n_gt + g] != CA_ABSENT) {
            const double given = gt_area_in ? gt_area_in[(size_t)b * n_gt + g] : 0.0;
            v = gt_area_in && given == given ? given : bbox ? __dmul_rn(bx[(CA_TOP + g) * 4 + 2], bx[(CA_TOP + g) * 4 + 3]) : (double)ar[CA_TOP + g];
        }
        gt_area[(size_t)b * n_gt + g] = v;
        return;
    }
    const long pair = e - P;
    const int d = (int)(pair / n_gt), g = (int)(pair - (long)d * n_gt);
    const uint8_t f = gt_flags[(size_t)b * n_gt + g];
    double v = 0.0;
    if (d < n_top && f != CA_ABSENT) {
        const bool crowd = f & 1;
        if (bbox) {
            const double* D = bx + d * 4;
            const double* G = bx + (CA_TOP + g) * 4;
            const double w = __dsub_rn(fmin(__dadd_rn(D[0], D[2]), __dadd_rn(G[0], G[2])), fmax(D[0], G[0]));
            const double h = __dsub_rn(fmin(__dadd_rn(D[1], D[3]), __dadd_rn(G[1], G[3])), fmax(D[1], G[1]));
            if (w > 0.0 && h > 0.0) {
                const double i = __dmul_rn(w, h), da = __dmul_rn(D[2], D[3]);
                const double u = crowd ? da : __dsub_rn(__dadd_rn(da, __dmul_rn(G[2], G[3])), i);
                v = __ddiv_rn(i, u);
            }
        } else {
            const long long i = inter[((size_t)b * CA_TOP + d) * n_gt + g], da = ar[d], ga = ar[CA_TOP + g];
            if (i) v = __ddiv_rn((double)i, (double)(crowd ? da : da + ga - i));
        }
    }
    if (BOUNDARY) {
        double vb = 0.0;
        if (d < n_top && f != CA_ABSENT) {
            const unsigned* ab = area_b + (size_t)b * P;
            const long long i = inter_b[((size_t)b * CA_TOP + d) * n_gt + g], da = ab[d], ga = ab[CA_TOP + g];
            if (i) vb = __ddiv_rn((double)i, (double)((f & 1) ? da : da + ga - i));
        }
        const size_t o = ((size_t)b * CA_TOP + d) * n_gt + g;
        if (mask_iou) mask_iou[o] = v;
        if (bnd_iou) bnd_iou[o] = vb;
        v = vb < v ? vb : v;
    }
    iou[((size_t)b * CA_TOP + d) * n_gt + g] = v;
}

// grid (A, B), CA_MAX lanes.  gi u8 [B][A][n_gt]: 0 = counts, 1 = ignored (ignore or crowd flag, or an area outside the range), 2 = absent;
// gorder i32 [B][A][n_gt]: the input indices in the stable order of gi (numpy's argsort(gi, kind='mergesort'); the absent ones behind).
__global__ __launch_bounds__(CA_MAX) void ca_gorder_kernel(const uint8_t* __restrict__ gt_flags, const double* __restrict__ gt_area,
                                                           const double* __restrict__ area_rng, int n_gt, int A, uint8_t* __restrict__ gi_out,
                                                           int* __restrict__ gorder) {
    __shared__ uint8_t s_gi[CA_MAX];
    const int t = threadIdx.x, a = blockIdx.x, b = blockIdx.y;
    const double lo = area_rng[a * 2], hi = area_rng[a * 2 + 1];
    int gi = 0;
    if (t < n_gt) {
        const uint8_t f = gt_flags[(size_t)b * n_gt + t];
        const double ar = gt_area[(size_t)b * n_gt + t];
        gi = f == CA_ABSENT ? 2 : ((f & 3) || ar < lo || ar > hi) ? 1 : 0;
        s_gi[t] = (uint8_t)gi;
    }
    __syncthreads();
    if (t < n_gt) {
        int pos = 0;
        for (int j = 0; j < n_gt; ++j) pos += s_gi[j] < gi || (s_gi[j] == gi && j < t);
        const size_t o = ((size_t)b * A + a) * n_gt;
        gi_out[o + t] = (uint8_t)gi;
        gorder[o + pos] = t;
    }
}

// grid (T, A, B), 64 lanes: one wave per (frame, area range, threshold).  dtm, dtig u8 [B][A][T][CA_TOP] (0 behind n_top).
//
// The contract's inner loop walks gorder (the ground truths that count first, then the ignored ones) with a running `best`, starting at
// best0 = min(t, 1 - 1e-10), and takes g iff it is eligible (not matched yet, or a crowd) and iou[g] >= best; taking sets best = iou[g],
// m = g.  It stops at the first ignored g once m is one that counts.  Claim: m is
//   1. the LAST position in gorder attaining M0 = max{iou[g] : g counts, eligible, iou[g] >= best0}, if that set is not empty;
//   2. else the last position attaining M1 = the same maximum over the eligible ignored g, if that set is not empty; else none.
// Proof.  `best` never decreases and always equals best0 or the iou of a taken g, so best <= M0 while the loop is among the g that count.
// Every g of set 1 with iou[g] = M0 therefore passes `iou[g] >= best` when it is reached and is taken (equal replaces); after the last of
// them best = M0 and no later g of the first part has iou >= M0 without being another attainer - so m is that last attainer when the
// first part ends, and the break keeps it.  If set 1 is empty nothing was taken, best is still best0 and m = -1 when the ignored part
// starts: there is no break, and the same argument on the ignored part gives 2.  (A crowd is always ignored, so "eligible" in the first
// part is just "not matched".)  Every lane keeps the best candidate of its positions k = lane, lane + 64, ... under the order (counts before
// ignored, higher iou, higher position), and a butterfly of shuffles leaves the wave's best in every lane: the order is total on distinct
// positions, so all lanes agree.
__global__ __launch_bounds__(64) void ca_match_kernel(const double* __restrict__ iou, const int* __restrict__ counts, const uint8_t* __restrict__ gt_flags,
                                                      const uint8_t* __restrict__ gi, const int* __restrict__ gorder,
                                                      const double* __restrict__ dt_area, const double* __restrict__ iou_thrs,
                                                      const double* __restrict__ area_rng, int n_gt, int T, int A, uint8_t* __restrict__ dtm,
                                                      uint8_t* __restrict__ dtig) {
    __shared__ int s_g[CA_MAX];                              // position in gorder -> input index
    __shared__ uint8_t s_state[CA_MAX];                      // by position: bit 0 = ignored, bit 1 = crowd, bit 2 = matched
    const int lane = threadIdx.x, ti = blockIdx.x, a = blockIdx.y, b = blockIdx.z;
    const int n_top = min(max(counts[b * 2], 0), CA_TOP), ngp = min(max(counts[b * 2 + 1], 0), n_gt);
    const size_t go = ((size_t)b * A + a) * n_gt;
    for (int k = lane; k < ngp; k += 64) {
        const int g = min(max(gorder[go + k], 0), n_gt - 1);
        s_g[k] = g;
        s_state[k] = (uint8_t)((gi[go + g] & 1) | (gt_flags[(size_t)b * n_gt + g] & 1) << 1);
    }
    __syncthreads();
    const double best0 = fmin(iou_thrs[ti], 1 - 1e-10);
    const double lo = area_rng[a * 2], hi = area_rng[a * 2 + 1];
    const size_t out = (((size_t)b * A + a) * T + ti) * CA_TOP;
    for (int d = 0; d < n_top; ++d) {
        const double* row = iou + ((size_t)b * CA_TOP + d) * n_gt;
        int pr = -1, bk = -1;                                // priority: 1 = counts, 0 = ignored, -1 = no candidate
        double bi = 0.0;
        for (int k = lane; k < ngp; k += 64) {
            const int st = s_state[k];
            if ((st & 4) && !(st & 2)) continue;
            const double v = row[s_g[k]];
            if (v < best0) continue;
            const int p = (st & 1) ? 0 : 1;
            if (p > pr || (p == pr && v >= bi)) { pr = p; bi = v; bk = k; }     // (k ascends: equal replaces)
        }
        for (int off = 32; off; off >>= 1) {
            const int opr = __shfl_xor(pr, off), obk = __shfl_xor(bk, off);
            const double obi = __shfl_xor(bi, off);
            if (opr > pr || (opr == pr && (obi > bi || (obi == bi && obk > bk)))) { pr = opr; bi = obi; bk = obk; }
        }
        if (lane == 0) {
            const double da = dt_area[b * CA_TOP + d];
            dtm[out + d] = pr >= 0;
            dtig[out + d] = pr >= 0 ? (s_state[bk] & 1) : (da < lo || da > hi);
            if (pr >= 0) s_state[bk] |= 4;
        }
        __syncthreads();                                     // (one wave: orders lane 0's LDS write before the next scan)
    }
    for (int d = n_top + lane; d < CA_TOP; d += 64) { dtm[out + d] = 0; dtig[out + d] = 0; }
}

// workspace layout: planes (segm and boundary) | inter, area [, inter_b, area_b] (zeroed together) | boxes [| boundary planes]
// mode: quber_coco_match's iou_type (0 segm, 1 bbox), 2 = Boundary IoU
struct CaWs { unsigned* planes; unsigned* inter; unsigned* area; double* boxes; size_t zero_bytes; unsigned* inter_b; unsigned* area_b; unsigned* bplanes; };

static size_t ca_layout(CaWs* out, void* ws, int B, int n_gt, int H, int W, int mode) {
    const size_t b = (size_t)B, P = CA_TOP + n_gt, pairs = b * CA_TOP * n_gt, sets = mode == 2 ? 2 : 1;
    CaWs none, &r = out ? *out : none;
    WsWalk w{static_cast<char*>(ws)};
    r.planes = mode == 1 ? nullptr : w.take<unsigned>(b * P * mn_plane_words(H, W));
    r.inter = w.take<unsigned>(sets * (pairs + b * P));
    r.area = r.inter ? r.inter + pairs : nullptr;
    r.inter_b = r.inter && mode == 2 ? r.inter + pairs + b * P : nullptr;
    r.area_b = r.inter_b ? r.inter_b + pairs : nullptr;
    r.zero_bytes = sets * (pairs + b * P) * 4;
    r.boxes = w.take<double>(b * P * 4);
    r.bplanes = mode == 2 ? w.take<unsigned>(b * P * mn_plane_words(H, W)) : nullptr;
    return w.off;
}

size_t coco_match_ws_bytes(int B, int n_gt, int H, int W, int bbox) { return ca_layout(nullptr, nullptr, B, n_gt, H, W, bbox); }

int coco_match_top() { return CA_TOP; }

// mode as in ca_layout; dilation, mask_iou, bnd_iou: mode 2 only
static int ca_launch(const CocoMatchArgs& q, int mode, int dilation, double* mask_iou, double* bnd_iou, int B, int H, int W, void* ws,
                     hipStream_t st) {
    if (B <= 0) return 0;
    if (H < 1 || W < 1) return fail("coco match: negative or empty frame");
    const int n_dt = q.n_dt, n_gt = q.n_gt, T = q.n_thrs, A = q.n_rng, bbox = mode == 1;
    if (n_dt < 0 || n_dt > CA_MAX) return fail("coco match: n_dt outside 0..1024");
    if (n_gt < 0 || n_gt > CA_MAX) return fail("coco match: n_gt outside 0..1024");
    if (T < 1 || T > CA_MAX_T) return fail("coco match: the number of IoU thresholds outside 1..16");
    if (A < 1 || A > CA_MAX_A) return fail("coco match: the number of area ranges outside 1..8");
    if (mode < 0 || mode > 2) return fail("coco match: iou_type must be 0 (segm) or 1 (bbox)");
    if (mode == 2 && (dilation < 1 || dilation > mask_boundary_max_dilation())) return fail("coco match: dilation outside 1..64");
    if (!q.iou_thrs || !q.area_rng || !q.counts || !q.order || !q.out_scores || !q.dt_area || !q.dtm || !q.dtig || !ws)
        return fail("coco match: null tensor");
    if (n_dt > 0 && (!q.scores || (!q.dt && !(bbox && q.dt_boxes)))) return fail("coco match: null detections");
    if (n_gt > 0 && (!q.gt_flags || !q.gt_area_used || !q.iou || !q.gi || !q.gorder || (!q.gt && !(bbox && q.gt_boxes))))
        return fail("coco match: null ground truth");
    const uintptr_t a8 = (uintptr_t)q.dt_boxes | (uintptr_t)q.gt_boxes | (uintptr_t)q.gt_area | (uintptr_t)q.iou_thrs | (uintptr_t)q.area_rng |
                         (uintptr_t)q.dt_area | (uintptr_t)q.gt_area_used | (uintptr_t)q.iou | (uintptr_t)mask_iou | (uintptr_t)bnd_iou;
    const uintptr_t a4 = (uintptr_t)q.scores | (uintptr_t)q.counts | (uintptr_t)q.order | (uintptr_t)q.out_scores | (uintptr_t)q.gorder;
    if ((a8 & 7) || (a4 & 3)) return fail("coco match: a 64-bit tensor that is not 8-byte aligned, or a 32-bit one that is not 4-byte aligned");
    const long HW = (long)H * W;
    const int wpr = (W + 31) / 32, pw = (int)mn_plane_words(H, W), P = CA_TOP + n_gt;
    CaWs w;
    ca_layout(&w, ws, B, n_gt, H, W, mode);
    {
        ProfScope prof("coco_rank", 4.0 * B * n_dt + 1.0 * B * n_gt, 0.0, st);
        hipLaunchKernelGGL(ca_rank_kernel, dim3(B), dim3(CA_MAX), 0, st, q.scores, q.gt_flags, n_dt, n_gt, q.counts, q.order, q.out_scores);
        QB_CHECK(hipGetLastError());
    }
    if (launch_zero(w.inter, w.zero_bytes, st)) return -1;
    if (bbox) {
        ProfScope prof("coco_boxes", 32.0 * B * P, 0.0, st);
        hipLaunchKernelGGL(ca_box_kernel, dim3(P, B), dim3(256), 0, st, q.dt, q.gt, q.dt_boxes, q.gt_boxes, q.order, q.gt_flags, n_dt, n_gt, H, W,
                           w.boxes);
        QB_CHECK(hipGetLastError());
    } else {
        {
            ProfScope prof("coco_pack", (double)B * P * HW + 4.0 * B * P * pw, 0.0, st);
            const dim3 grid((pw + 255) / 256, P, B);
            const bool aligned = W % 16 == 0 && ((uintptr_t)q.dt & 15) == 0 && ((uintptr_t)q.gt & 15) == 0;
            if (aligned)
                hipLaunchKernelGGL(ca_pack_kernel<true>, grid, dim3(256), 0, st, q.dt, q.gt, q.order, q.gt_flags, n_dt, n_gt, H, W, wpr, pw, w.planes, w.area);
            else
                hipLaunchKernelGGL(ca_pack_kernel<false>, grid, dim3(256), 0, st, q.dt, q.gt, q.order, q.gt_flags, n_dt, n_gt, H, W, wpr, pw, w.planes, w.area);
            QB_CHECK(hipGetLastError());
        }
        if (mode == 2 && launch_boundary_planes(w.planes, (long)B * P, H, W, dilation, w.bplanes, w.area_b, 1, st)) return -1;
        if (n_gt > 0) {
            const int ntg = (n_gt + CA_TILE - 1) / CA_TILE;
            ProfScope prof("coco_gram", (mode == 2 ? 2.0 : 1.0) * (4.0 * B * pw * ((double)CA_TOP * ntg + (double)n_gt * CA_DT_TILES) + 4.0 * B * CA_TOP * n_gt),
                           0.0, st);
            const dim3 grid(CA_DT_TILES * ntg, (pw + CA_CHUNK - 1) / CA_CHUNK, B);
            hipLaunchKernelGGL(ca_gram_kernel, grid, dim3(256), 0, st, w.planes, w.inter, n_gt, pw);
            if (mode == 2) hipLaunchKernelGGL(ca_gram_kernel, grid, dim3(256), 0, st, w.bplanes, w.inter_b, n_gt, pw);
            QB_CHECK(hipGetLastError());
        }
    }
    {
        ProfScope prof("coco_iou", (mode == 2 ? 36.0 : 12.0) * B * CA_TOP * n_gt, 0.0, st);
        const long n = (long)P + (long)CA_TOP * n_gt;
        const dim3 grid((unsigned)((n + 255) / 256), B);
        if (mode == 2)
            hipLaunchKernelGGL(ca_iou_kernel<true>, grid, dim3(256), 0, st, 0, w.inter, w.area, w.boxes, q.counts, q.gt_flags, q.gt_area, n_gt, q.dt_area,
                               q.gt_area_used, q.iou, w.inter_b, w.area_b, mask_iou, bnd_iou);
        else
            hipLaunchKernelGGL(ca_iou_kernel<false>, grid, dim3(256), 0, st, bbox, w.inter, w.area, w.boxes, q.counts, q.gt_flags, q.gt_area, n_gt,
                               q.dt_area, q.gt_area_used, q.iou, nullptr, nullptr, nullptr, nullptr);
        QB_CHECK(hipGetLastError());
    }
    if (n_gt > 0) {
        ProfScope prof("coco_gorder", 13.0 * B * n_gt + 5.0 * B * A * n_gt, 0.0, st);
        hipLaunchKernelGGL(ca_gorder_kernel, dim3(A, B), dim3(CA_MAX), 0, st, q.gt_flags, q.gt_area_used, q.area_rng, n_gt, A, q.gi, q.gorder);
        QB_CHECK(hipGetLastError());
    }
    {
        ProfScope prof("coco_match", 8.0 * B * CA_TOP * n_gt * A * T + 2.0 * B * A * T * CA_TOP, 0.0, st);
        hipLaunchKernelGGL(ca_match_kernel, dim3(T, A, B), dim3(64), 0, st, q.iou, q.counts, q.gt_flags, q.gi, q.gorder, q.dt_area, q.iou_thrs,
                           q.area_rng, n_gt, T, A, q.dtm, q.dtig);
        QB_CHECK(hipGetLastError());
    }
    return 0;
}

int launch_coco_match(const CocoMatchArgs& q, int B, int H, int W, void* ws, hipStream_t st) {
    if (q.iou_type != 0 && q.iou_type != 1) return fail("coco match: iou_type must be 0 (segm) or 1 (bbox)");
    return ca_launch(q, q.iou_type, 0, nullptr, nullptr, B, H, W, ws, st);
}

int launch_coco_match_boundary(const CocoMatchArgs& q, int dilation, double* mask_iou, double* boundary_iou, int B, int H, int W, void* ws,
                               hipStream_t st) {
    if (q.dt_boxes || q.gt_boxes) return fail("coco match: boxes come with iou_type 1 (bbox)");
    return ca_launch(q, 2, dilation, mask_iou, boundary_iou, B, H, W, ws, st);
}

}  // namespace quber
