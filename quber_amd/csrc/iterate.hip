// Iterative refinement without leaving the device: what lies between quber_postprocess of one pass and quber_encode_label_map of the
// next, and the bookkeeping a caller asks for once there is more than one pass.
//   relabel_panoptic: the label map of quber_postprocess (f32: -1 / 1000 / 1001 ...) + the frame's label list -> compact ids 0 | 1..count
//                     (the input of quber_encode_label_map), optionally with the W-mirror of every frame behind the batch
//   overlap_masks:    pixels of every initial mask per id of a compact label map (+ the area of every id)
//   overlap_ids:      contingency table of two compact label maps (successive passes: has the segmentation stopped changing)
// All three are pure streams on the caller's stream in the style of csrc/errhead.hip: no allocation, no synchronisation; every counter
// table is cleared by the zero-fill kernel (launch_zero: memset nodes do not replay) in front of the kernel that adds to it, so a call
// overwrites its outputs and a captured graph replays idempotently.  Integer arithmetic only: results are exact and order-independent.
//
// Counting.  The tables have up to 255 (masks) / 255 x 255 (ids) bins per frame, of which a block meets a handful: a strip of a few
// rows overlaps a few instances.  So a block counts into a small LDS hash table keyed by the cell index (open addressing, a cell
// that finds no slot within OV_PROBES steps is added to global memory directly - correct whatever the input, only slower), and adds
// every used slot to the global table once at its end.  In front of the LDS sits the aggregation of Guideline "reduce atomic
// contention": a 16-pixel group is decomposed into its (at most two, else pixel by pixel) ids and adds one popcount per id; a wave
// whose lanes all count into the same cell - the common case, masks and instances being blobs - adds one wave sum.
#include "common.h"

namespace quber {

constexpr int OV_THREADS = 256;
constexpr int OV_SLOTS = 2048;                           // LDS hash slots per block (key + count: 16 KiB)
constexpr int OV_PROBES = 8;
constexpr unsigned OV_EMPTY = 0xffffffffu;
constexpr unsigned OV_NOID = 255u;                       // byte code of an id outside 0..n_ids (n_ids <= 254): counted nowhere

typedef int ov_i4 __attribute__((ext_vector_type(4)));
typedef ov_i4 ov_i4u __attribute__((aligned(4)));        // a 16-byte load at any int address (global memory: dword alignment suffices)
typedef float ov_f4 __attribute__((ext_vector_type(4)));
typedef ov_f4 ov_f4u __attribute__((aligned(4)));

// the byte-set helpers of csrc/errhead.hip (file-local there)
__device__ __forceinline__ unsigned ov_nz(unsigned wd) { return ((((wd & 0x7f7f7f7fu) + 0x7f7f7f7fu) | wd) & 0x80808080u) >> 7; }
__device__ __forceinline__ unsigned ov_nib(unsigned m) { return (m * 0x01020408u) >> 24; }
// bit i = (byte i of the 16 bytes is non-zero)
__device__ __forceinline__ unsigned ov_nzbits(unsigned x, unsigned y, unsigned z, unsigned w) {
    return ov_nib(ov_nz(x)) | ov_nib(ov_nz(y)) << 4 | ov_nib(ov_nz(z)) << 8 | ov_nib(ov_nz(w)) << 12;
}
// bit i = (byte i of the 16 bytes equals c)
__device__ __forceinline__ unsigned ov_eqbits(const unsigned (&v)[4], unsigned c) {
    const unsigned k = c * 0x01010101u;
    return ov_nzbits(v[0] ^ k, v[1] ^ k, v[2] ^ k, v[3] ^ k) ^ 0xffffu;
}
// byte i (0..15) of the 16 bytes (shifts of two 64-bit halves: indexing the words by i >> 2 would send them to scratch memory)
__device__ __forceinline__ unsigned ov_byte(const unsigned (&v)[4], int i) {
    const unsigned long long lo = (unsigned long long)v[1] << 32 | v[0], hi = (unsigned long long)v[3] << 32 | v[2];
    return (unsigned)((i < 8 ? lo : hi) >> (8 * (i & 7))) & 0xffu;
}
// four ids -> four byte codes in one word
__device__ __forceinline__ unsigned ov_pack(const ov_i4& q, int n_ids) {
    unsigned r = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) r |= ((unsigned)q[e] <= (unsigned)n_ids ? (unsigned)q[e] : OV_NOID) << (8 * e);
    return r;
}

__device__ __forceinline__ unsigned ov_wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;                                            // complete in lane 0
}

struct OvHash {
    unsigned key[OV_SLOTS];
    unsigned cnt[OV_SLOTS];
};

__device__ __forceinline__ void ov_clear(OvHash& h) {
    for (int i = threadIdx.x; i < OV_SLOTS; i += OV_THREADS) {
        h.key[i] = OV_EMPTY;
        h.cnt[i] = 0;
    }
}

// `c` more pixels in cell `key`; DST: cell index -> address of its global counter
template <typename DST>
__device__ __forceinline__ void ov_add(OvHash& h, const DST& dst, unsigned key, unsigned c) {
    unsigned s = (key * 2654435761u) >> 21;              // 11 bits: OV_SLOTS
#pragma unroll 1
    for (int i = 0; i < OV_PROBES; ++i) {
        const unsigned prev = atomicCAS(&h.key[s], OV_EMPTY, key);
        if (prev == OV_EMPTY || prev == key) {
            atomicAdd(&h.cnt[s], c);
            return;
        }
        s = (s + 1) & (OV_SLOTS - 1);
    }
    atomicAdd(dst(key), c);
}
static_assert(OV_SLOTS == 1 << 11, "ov_add hashes to 11 bits");

// Every lane of the wave calls (wave-uniform control flow); a lane with c == 0 adds nothing.  Lanes that agree on the cell add one sum.
template <typename DST>
__device__ __forceinline__ void ov_wave_add(OvHash& h, const DST& dst, unsigned key, unsigned c) {
    const bool act = c != 0;
    const unsigned long long bal = __ballot(act);
    if (bal == 0) return;
    const unsigned k0 = __shfl(key, __ffsll((long long)bal) - 1);
    if (__ballot(act && key != k0) == 0) {
        const unsigned s = ov_wave_sum(c);
        if ((threadIdx.x & 63) == 0) ov_add(h, dst, k0, s);
    } else if (act) {
        ov_add(h, dst, key, c);
    }
}

template <typename DST>
__device__ __forceinline__ void ov_flush(OvHash& h, const DST& dst) {
    for (int i = threadIdx.x; i < OV_SLOTS; i += OV_THREADS)
        if (h.key[i] != OV_EMPTY && h.cnt[i]) atomicAdd(dst(h.key[i]), h.cnt[i]);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// relabel_panoptic.  grid (ceil(HW / 4 / 256), B).  The frame's label list (count <= top_k values, ascending) sits in LDS; a pixel's
// value is looked up by binary search (the first position that holds it), a lane remembering its previous pixel's answer.  A frame is
// split at the 16-byte boundaries of its OUTPUT as in error_decode: a head (< 4 pixels), groups of four pixels - one per lane: one
// 16-byte load, one 16-byte store -, a tail (< 4 pixels); head and tail are done one pixel per lane by the frame's first block.  The
// mirrored copy (frame B + b, x -> W - 1 - x) is written pixel by pixel: a wave's stores still cover whole lines, back to front.
__device__ __forceinline__ int rl_lookup(const float* lab, int n, float v) {
    int lo = 0, hi = n;                                  // first position with lab[pos] >= v
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (lab[mid] < v) lo = mid + 1; else hi = mid;
    }
    return (lo < n && lab[lo] == v) ? lo + 1 : 0;        // a NaN compares false everywhere: 0
}

__global__ __launch_bounds__(OV_THREADS) void relabel_panoptic_kernel(const float* __restrict__ pan, const float* __restrict__ labels,
                                                                      const int* __restrict__ count, int top_k, long HW, int W,
                                                                      int* __restrict__ ids, int* __restrict__ mirror) {
    extern __shared__ float rl_lab[];                    // [top_k]
    const int b = blockIdx.y;
    const int n = min(max(count[b], 0), top_k);
    for (int i = threadIdx.x; i < n; i += OV_THREADS) rl_lab[i] = labels[(long)b * top_k + i];
    __syncthreads();
    const float* src = pan + (long)b * HW;
    int* o = ids + (long)b * HW;
    int* om = mirror ? mirror + (long)b * HW : nullptr;
    const int head = (int)min((long)(((16 - (int)((uintptr_t)o & 15)) & 15) >> 2), HW);
    const long nbody = (HW - head) >> 2;
    const long g = (long)blockIdx.x * OV_THREADS + threadIdx.x;
    if (g < nbody) {
        const long p = head + (g << 2);
        const ov_f4u v = *reinterpret_cast<const ov_f4u*>(src + p);
        ov_i4 r;
        r[0] = rl_lookup(rl_lab, n, v[0]);
#pragma unroll
        for (int e = 1; e < 4; ++e) r[e] = v[e] == v[e - 1] ? r[e - 1] : rl_lookup(rl_lab, n, v[e]);
        *reinterpret_cast<ov_i4*>(o + p) = r;
        if (om) {
            const long y = p / W;
            int x = (int)(p - y * W);
            long row = y * W;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                om[row + (W - 1 - x)] = r[e];
                if (++x == W) { x = 0; row += W; }
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < 8) {            // the ragged ends: lanes 0..3 the head, 4..7 the tail
        const int t = threadIdx.x;
        const long tail0 = head + (nbody << 2);
        long p = -1;
        if (t < 4) {
            if (t < head) p = t;
        } else if (tail0 + (t - 4) < HW) {
            p = tail0 + (t - 4);
        }
        if (p >= 0) {
            const int r = rl_lookup(rl_lab, n, src[p]);
            o[p] = r;
            if (om) {
                const long y = p / W;
                om[y * W + (W - 1 - (int)(p - y * W))] = r;
            }
        }
    }
}

int launch_relabel_panoptic(const float* pan, const float* labels, const int* count, int B, int top_k, int mirror, int H, int W,
                            int* ids, hipStream_t st) {
    if (B <= 0) return 0;
    if (B > 65535) return fail("relabel_panoptic: batch above 65535");
    if (top_k < 1 || top_k > 8192) return fail("relabel_panoptic: top_k outside 1..8192");
    const long HW = (long)H * W;
    if (HW < 1 || ((HW >> 2) + OV_THREADS - 1) / OV_THREADS > 0x7fffffffL) return fail("relabel_panoptic: frame size");
    ProfScope prof("iterate_relabel", (mirror ? 12.0 : 8.0) * B * (double)HW, 0.0, st);
    const dim3 grid((unsigned)max(1L, ((HW >> 2) + OV_THREADS - 1) / OV_THREADS), (unsigned)B);
    hipLaunchKernelGGL(relabel_panoptic_kernel, grid, dim3(OV_THREADS), sizeof(float) * (size_t)top_k, st, pan, labels, count, top_k, HW,
                       W, ids, mirror ? ids + (long)B * HW : nullptr);
    QB_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// overlap_masks.  The reading pattern of error_mask_hist: grid (ceil(HW / (256 * 16 * OM_R)), B, mask chunks); a lane owns OM_R groups
// of 16 pixels, 1 KiB (one wave load) apart.  It loads the 16 id words of a group once (4 x 16 bytes), packs them into 16 byte codes
// and decomposes the group: id A (that of its first pixel) with the 16-bit set of the pixels that carry it, id B (that of the first
// pixel outside A) with its set, and the set of the pixels that carry neither - empty except where three instances meet within 16
// pixels.  Per mask of its chunk it issues its OM_R 16-byte loads back to back (the next mask's before this one's arithmetic), turns
// the 16 mask bytes into 16 bits and counts the intersections: one popcount per (group, id).  The lane's count for the id of its first
// group goes through the wave (ov_wave_add), anything else straight to the LDS table.  The frame's first chunk also counts the area
// of every id: the same path with every pixel "inside".
constexpr int OM_R = 2;
constexpr int OM_CHUNK = 2048;                           // most masks per block (grid z <= 65535)
constexpr long OM_SPAN = (long)OV_THREADS * 16 * OM_R;   // pixels per block
constexpr long OM_BLOCKS = 1024;                         // blocks a launch aims for (4 per CU)

struct OmDst {                                           // cell = row * bins + id; row Nc (behind the chunk's masks) = the area
    unsigned* table;                                     // [Nc][bins] of this block's chunk
    unsigned* area;                                      // [bins] of this frame, or null
    unsigned bins, Nc;
    __device__ __forceinline__ unsigned* operator()(unsigned key) const {
        const unsigned row = key / bins;
        return row < Nc ? table + key : area + (key - Nc * bins);
    }
};

struct OmGroup {
    unsigned idA, idB, bitsA, bitsB, rest;               // ids as byte codes (OV_NOID: its set is empty), sets of 16 bits
    unsigned w[4];                                       // the 16 byte codes
};

__device__ __forceinline__ void om_count(OvHash& h, const OmDst& dst, const OmGroup (&g)[OM_R], const unsigned (&m)[OM_R], unsigned row) {
    const unsigned base = row * dst.bins;
    const unsigned id0 = g[0].idA;
    unsigned c0 = 0;
#pragma unroll
    for (int r = 0; r < OM_R; ++r) {
        const unsigned cA = __popc(m[r] & g[r].bitsA), cB = __popc(m[r] & g[r].bitsB);
        if (g[r].idA == id0) c0 += cA;
        else if (cA) ov_add(h, dst, base + g[r].idA, cA);
        if (cB) ov_add(h, dst, base + g[r].idB, cB);
        unsigned left = m[r] & g[r].rest;
        while (left) {
            const int i = __ffs(left) - 1;
            left &= left - 1;
            const unsigned id = ov_byte(g[r].w, i);
            if (id != OV_NOID) ov_add(h, dst, base + id, 1u);
        }
    }
    ov_wave_add(h, dst, base + id0, c0);                 // (id0 == OV_NOID: bitsA is empty, c0 == 0)
}

__global__ __launch_bounds__(OV_THREADS) void overlap_masks_kernel(const uint8_t* __restrict__ masks, const int* __restrict__ ids, int N,
                                                                   int per, int n_ids, long HW, unsigned* __restrict__ table,
                                                                   unsigned* __restrict__ area) {
    __shared__ OvHash h;
    const int n0 = blockIdx.z * per, Nc = max(0, min(per, N - n0));
    const int b = blockIdx.y;
    const unsigned bins = (unsigned)n_ids + 1u;
    const bool with_area = area != nullptr && blockIdx.z == 0;
    const OmDst dst{table + ((long)b * N + n0) * bins, with_area ? area + (long)b * bins : nullptr, bins, (unsigned)Nc};
    ov_clear(h);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long base = ((long)blockIdx.x * 4 + wave) * OM_R * 1024 + lane * 16;
    bool act[OM_R];
    OmGroup g[OM_R];
#pragma unroll
    for (int r = 0; r < OM_R; ++r) {
        act[r] = base + (long)r * 1024 < HW;             // HW % 16 == 0: a group is inside or outside as a whole
        const int* ip = ids + (long)b * HW + base + (long)r * 1024;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            ov_i4 q4 = {-1, -1, -1, -1};
            if (act[r]) q4 = *reinterpret_cast<const ov_i4u*>(ip + 4 * q);
            g[r].w[q] = ov_pack(q4, n_ids);              // (outside the frame: four OV_NOID)
        }
        g[r].idA = g[r].w[0] & 0xffu;
        const unsigned eqA = ov_eqbits(g[r].w, g[r].idA);
        const unsigned notA = eqA ^ 0xffffu;
        g[r].idB = notA ? ov_byte(g[r].w, __ffs(notA) - 1) : OV_NOID;
        const unsigned eqB = notA ? ov_eqbits(g[r].w, g[r].idB) : 0u;
        g[r].bitsA = g[r].idA != OV_NOID ? eqA : 0u;
        g[r].bitsB = g[r].idB != OV_NOID ? eqB : 0u;
        g[r].rest = notA & ~eqB;
    }
    if (with_area) {
        unsigned all[OM_R];
#pragma unroll
        for (int r = 0; r < OM_R; ++r) all[r] = act[r] ? 0xffffu : 0u;
        om_count(h, dst, g, all, (unsigned)Nc);
    }
    if (Nc > 0) {
        const uint8_t* src = masks + ((long)b * N + n0) * HW + base;
        uint4 nxt[OM_R];
#pragma unroll
        for (int r = 0; r < OM_R; ++r) nxt[r] = act[r] ? *reinterpret_cast<const uint4*>(src + (long)r * 1024) : make_uint4(0, 0, 0, 0);
        for (int n = 0; n < Nc; ++n) {
            uint4 v[OM_R];
#pragma unroll
            for (int r = 0; r < OM_R; ++r) v[r] = nxt[r];
            if (n + 1 < Nc) {
#pragma unroll
                for (int r = 0; r < OM_R; ++r)
                    nxt[r] = act[r] ? *reinterpret_cast<const uint4*>(src + (long)(n + 1) * HW + (long)r * 1024) : make_uint4(0, 0, 0, 0);
            }
            unsigned m[OM_R];
#pragma unroll
            for (int r = 0; r < OM_R; ++r) m[r] = ov_nzbits(v[r].x, v[r].y, v[r].z, v[r].w);
            om_count(h, dst, g, m, (unsigned)n);
        }
    }
    __syncthreads();
    ov_flush(h, dst);
}

// any HW, any alignment: one pixel per lane
__global__ __launch_bounds__(OV_THREADS) void overlap_masks_generic_kernel(const uint8_t* __restrict__ masks, const int* __restrict__ ids,
                                                                           int N, int per, int n_ids, long HW,
                                                                           unsigned* __restrict__ table, unsigned* __restrict__ area) {
    __shared__ OvHash h;
    const int n0 = blockIdx.z * per, Nc = max(0, min(per, N - n0));
    const int b = blockIdx.y;
    const unsigned bins = (unsigned)n_ids + 1u;
    const bool with_area = area != nullptr && blockIdx.z == 0;
    const OmDst dst{table + ((long)b * N + n0) * bins, with_area ? area + (long)b * bins : nullptr, bins, (unsigned)Nc};
    ov_clear(h);
    __syncthreads();
    const long p = (long)blockIdx.x * OV_THREADS + threadIdx.x;
    const unsigned id = p < HW ? (unsigned)ids[(long)b * HW + p] : OV_EMPTY;
    const bool ok = id <= (unsigned)n_ids;               // (a lane outside the frame: never)
    if (with_area) ov_wave_add(h, dst, (unsigned)Nc * bins + id, ok ? 1u : 0u);
    const uint8_t* src = masks + ((long)b * N + n0) * HW + p;
    for (int n = 0; n < Nc; ++n) ov_wave_add(h, dst, (unsigned)n * bins + id, (ok && src[(long)n * HW] != 0) ? 1u : 0u);
    __syncthreads();
    ov_flush(h, dst);
}

int launch_overlap_masks(const uint8_t* masks, const int* ids, int B, int N, int n_ids, int H, int W, unsigned* table, unsigned* area,
                         hipStream_t st) {
    if (B <= 0) return 0;
    if (B > 65535) return fail("overlap_masks: batch above 65535");
    if (N < 0) return fail("overlap_masks: negative mask count");
    if (n_ids < 0 || n_ids > 254) return fail("overlap_masks: n_ids outside 0..254");
    const long HW = (long)H * W;
    if (HW < 1 || HW > 0x7fffffffL) return fail("overlap_masks: frame size");
    if (((long)N + 1) * (n_ids + 1) > 0x7fffffffL) return fail("overlap_masks: table too large");
    if (N == 0 && !area) return 0;
    const size_t bins = (size_t)n_ids + 1;
    if (N > 0)
        if (int rc = launch_zero(table, sizeof(unsigned) * (size_t)B * N * bins, st)) return rc;
    if (area)
        if (int rc = launch_zero(area, sizeof(unsigned) * (size_t)B * bins, st)) return rc;
    ProfScope prof("iterate_overlap_masks", (double)B * (double)HW * (N + 4.0) + 4.0 * B * (N + 1.0) * bins, 0.0, st);
    const bool vec = HW % 16 == 0 && ((uintptr_t)masks & 15) == 0;
    const long bx = vec ? (HW + OM_SPAN - 1) / OM_SPAN : (HW + OV_THREADS - 1) / OV_THREADS;
    // masks per block: all of them when the pixel strips alone fill the device, else split until about OM_BLOCKS blocks exist
    // (a chunk re-reads the id words, 4 / `per` of its mask bytes)
    const long nz = min((long)max(N, 1), max(1L, (OM_BLOCKS + bx * B - 1) / (bx * B)));
    const int per = (int)min((long)OM_CHUNK, (max(N, 1) + nz - 1) / nz);
    const long gz = (max(N, 1) + per - 1) / per;
    if (gz > 65535) return fail("overlap_masks: too many masks");
    const dim3 grid((unsigned)bx, (unsigned)B, (unsigned)gz);
    if (vec)
        hipLaunchKernelGGL(overlap_masks_kernel, grid, dim3(OV_THREADS), 0, st, masks, ids, N, per, n_ids, HW, table, area);
    else
        hipLaunchKernelGGL(overlap_masks_generic_kernel, grid, dim3(OV_THREADS), 0, st, masks, ids, N, per, n_ids, HW, table, area);
    QB_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// overlap_ids.  grid (ceil(HW / (256 * 16)), B); a lane owns 16 consecutive pixels: 4 + 4 loads of 16 bytes (any alignment), the pair
// (a, b) of every pixel as its cell index a * (n_b + 1) + b.  The pixels that share the first pixel's cell are counted at once and go
// through the wave (ov_wave_add); the others are folded into runs of equal cells, one LDS add per run.  The last, partial group of a
// frame is read pixel by pixel.
__global__ __launch_bounds__(OV_THREADS) void overlap_ids_kernel(const int* __restrict__ A, const int* __restrict__ Bm, int n_a, int n_b,
                                                                 long HW, unsigned* __restrict__ table) {
    __shared__ OvHash h;
    const int b = blockIdx.y;
    const unsigned nb1 = (unsigned)n_b + 1u;
    unsigned* tb = table + (long)b * ((long)n_a + 1) * nb1;
    const auto dst = [tb](unsigned key) { return tb + key; };
    ov_clear(h);
    __syncthreads();
    const long p0 = ((long)blockIdx.x * OV_THREADS + threadIdx.x) * 16;
    const int* ap = A + (long)b * HW + p0;
    const int* bp = Bm + (long)b * HW + p0;
    unsigned cell[16];
    if (p0 + 16 <= HW) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const ov_i4 va = *reinterpret_cast<const ov_i4u*>(ap + 4 * q), vb = *reinterpret_cast<const ov_i4u*>(bp + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                cell[4 * q + e] = ((unsigned)va[e] <= (unsigned)n_a && (unsigned)vb[e] <= (unsigned)n_b) ? (unsigned)va[e] * nb1 + (unsigned)vb[e] : OV_EMPTY;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            cell[i] = OV_EMPTY;
            if (p0 + i < HW) {
                const unsigned a = (unsigned)ap[i], c = (unsigned)bp[i];
                if (a <= (unsigned)n_a && c <= (unsigned)n_b) cell[i] = a * nb1 + c;
            }
        }
    }
    const unsigned k0 = cell[0];
    unsigned c0 = 0, run = OV_EMPTY, rc = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const unsigned k = cell[i];
        if (k == k0) {
            c0 += 1;
        } else if (k == run) {
            rc += 1;
        } else {
            if (run != OV_EMPTY) ov_add(h, dst, run, rc);
            run = k;
            rc = 1;
        }
    }
    if (run != OV_EMPTY) ov_add(h, dst, run, rc);
    ov_wave_add(h, dst, k0, k0 != OV_EMPTY ? c0 : 0u);
    __syncthreads();
    ov_flush(h, dst);
}

int launch_overlap_ids(const int* a, const int* b, int B, int n_a, int n_b, int H, int W, unsigned* table, hipStream_t st) {
    if (B <= 0) return 0;
    if (B > 65535) return fail("overlap_ids: batch above 65535");
    if (n_a < 0 || n_a > 254 || n_b < 0 || n_b > 254) return fail("overlap_ids: n_a / n_b outside 0..254");
    const long HW = (long)H * W;
    if (HW < 1 || HW > 0x7fffffffL) return fail("overlap_ids: frame size");
    const size_t cells = ((size_t)n_a + 1) * ((size_t)n_b + 1);
    if (int rc = launch_zero(table, sizeof(unsigned) * (size_t)B * cells, st)) return rc;
    ProfScope prof("iterate_overlap_ids", 8.0 * B * (double)HW + 4.0 * B * cells, 0.0, st);
    const long per = (long)OV_THREADS * 16;
    hipLaunchKernelGGL(overlap_ids_kernel, dim3((unsigned)((HW + per - 1) / per), (unsigned)B), dim3(OV_THREADS), 0, st, a, b, n_a, n_b, HW,
                       table);
    QB_CHECK(hipGetLastError());
    return 0;
}

}  // namespace quber
