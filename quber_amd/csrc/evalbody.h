// Bodies of the evaluation kernels, shared by the one-frame launches (metrics.hip, boundary.hip) and the batched ones (evalbatch.hip):
// each kernel there is a thin wrapper that picks the frame's (object's) pointers and calls one of these.  A body uses blockIdx.x /
// gridDim.x (and, where stated, blockIdx.y) as the one-frame kernel did; the batched kernels put the frame on a further grid axis.
#pragma once
#include "common.h"

namespace quber {

using u64 = unsigned long long;

constexpr int LAB_MAX = 65536;

// ------------------------------------------------------------------------------------------------ labels (metrics.hip)
__device__ inline void label_presence_body(const int* __restrict__ pred, const int* __restrict__ gt, long n,
                                           unsigned* __restrict__ flags /*[2][LAB_MAX]*/, int* __restrict__ bad) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int p = pred[i], g = gt[i];
        if ((unsigned)p >= LAB_MAX || (unsigned)g >= LAB_MAX) { *bad = 1; continue; }
        if (!flags[p]) flags[p] = 1;                 // benign race: every writer stores 1
        if (!flags[LAB_MAX + g]) flags[LAB_MAX + g] = 1;
    }
}

// one block of 1024 threads per map (which = 0 pred, 1 gt): ordered compaction of the set flags
__device__ inline void label_rank_body(const unsigned* __restrict__ flags, int cap, int which, unsigned short* __restrict__ lut /*[2][LAB_MAX]*/,
                                       int* __restrict__ labels /*[2][cap]*/, int* __restrict__ counts) {
    __shared__ unsigned scan[1024];
    const int t = threadIdx.x;
    const unsigned* f = flags + (long)which * LAB_MAX;
    constexpr int SEG = LAB_MAX / 1024;
    unsigned n = 0;
    for (int i = 0; i < SEG; ++i) n += f[t * SEG + i] != 0;
    scan[t] = n;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const unsigned v = t >= o ? scan[t - o] : 0;
        __syncthreads();
        scan[t] += v;
        __syncthreads();
    }
    unsigned pos = scan[t] - n;
    for (int i = 0; i < SEG; ++i) {
        const int v = t * SEG + i;
        if (f[v]) {
            if ((int)pos < cap) {
                labels[which * cap + pos] = v;
                lut[(long)which * LAB_MAX + v] = (unsigned short)pos;
            }
            ++pos;
        }
    }
    if (t == 1023) counts[which] = (int)scan[1023];
}

// 256 threads; dynamic LDS: 4096 words (the private table)
__device__ inline void contingency_body(const int* __restrict__ pred, const int* __restrict__ gt, long n, const unsigned short* __restrict__ lut,
                                        const int* __restrict__ counts, int cap, u64* __restrict__ table /*[cap][cap]*/) {
    extern __shared__ unsigned priv[];
    const int np_ = counts[0], ng = counts[1];
    // counts[2]: label_presence met a value outside 0..65535 - the LUT cannot index it, the host raises
    if (np_ > cap || ng > cap || counts[2]) return;
    const bool use_lds = (long)np_ * ng <= 4096;
    if (use_lds) {
        for (int i = threadIdx.x; i < np_ * ng; i += 256) priv[i] = 0;
        __syncthreads();
    }
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int pv = pred[i], gv = gt[i];
        if ((unsigned)pv >= LAB_MAX || (unsigned)gv >= LAB_MAX) continue;     // unreachable once counts[2] is honoured
        const int pj = lut[pv], gi = lut[LAB_MAX + gv];
        if (use_lds) atomicAdd(&priv[gi * np_ + pj], 1u);
        else atomicAdd(&table[(long)gi * cap + pj], 1ull);
    }
    if (use_lds) {
        __syncthreads();
        for (int i = threadIdx.x; i < np_ * ng; i += 256)
            if (priv[i]) atomicAdd(&table[(long)(i / np_) * cap + (i % np_)], (u64)priv[i]);
    }
}

// ------------------------------------------------------------------------------------------------ boundary (boundary.hip)
// 256 threads = 4 words of 64 pixels, blockIdx.x = group of 4 words: seg = (map == value), one bit per pixel
__device__ inline void bnd_pack_body(const int* __restrict__ map, int value, int H, int W, int wpr, u64* __restrict__ seg /*[H][wpr]*/) {
    const long word = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int y = (int)(word / wpr), wx = (int)(word - (long)y * wpr);
    const int x = wx * 64 + (threadIdx.x & 63);
    const bool on = y < H && x < W && map[(long)y * W + x] == value;
    const u64 bits = __ballot(on);
    if ((threadIdx.x & 63) == 0 && y < H) seg[(long)y * wpr + wx] = bits;
}

// all bits reachable from `gen` by moving towards higher / lower bit positions through set bits of `pro` (within the word)
__device__ inline u64 fill_up(u64 gen, u64 pro) {
    gen |= pro & (gen << 1); pro &= pro << 1;
    gen |= pro & (gen << 2); pro &= pro << 2;
    gen |= pro & (gen << 4); pro &= pro << 4;
    gen |= pro & (gen << 8); pro &= pro << 8;
    gen |= pro & (gen << 16); pro &= pro << 16;
    gen |= pro & (gen << 32);
    return gen;
}
__device__ inline u64 fill_down(u64 gen, u64 pro) {
    gen |= pro & (gen >> 1); pro &= pro >> 1;
    gen |= pro & (gen >> 2); pro &= pro >> 2;
    gen |= pro & (gen >> 4); pro &= pro >> 4;
    gen |= pro & (gen >> 8); pro &= pro >> 8;
    gen |= pro & (gen >> 16); pro &= pro >> 16;
    gen |= pro & (gen >> 32);
    return gen;
}

// one workgroup of 1024 threads per object; dynamic LDS: reach[H][wpr].  s: the object's packed plane; bm / dl: its border and dilated
// border planes; *count: its border size
__device__ inline void bnd_bmap_body(const u64* __restrict__ s, int H, int W, int wpr, int radius, u64* __restrict__ bm, u64* __restrict__ dl,
                                     unsigned* __restrict__ count) {
    extern __shared__ u64 reach[];
    __shared__ int changed;
    __shared__ unsigned total;
    const int t = threadIdx.x, n = H * wpr;
    const u64 last_mask = (W & 63) ? ((1ull << (W & 63)) - 1) : ~0ull;
    auto bgw = [&](int i) { const int wx = i % wpr; return ~s[i] & (wx == wpr - 1 ? last_mask : ~0ull); };
    // seeds: background pixels of the first / last row and column
    for (int i = t; i < n; i += 1024) {
        const int y = i / wpr, wx = i - y * wpr;
        u64 seed = (y == 0 || y == H - 1) ? ~0ull : 0ull;
        if (wx == 0) seed |= 1ull;
        if (wx == wpr - 1) seed |= 1ull << ((W - 1) & 63);
        reach[i] = seed & bgw(i);
    }
    if (t == 0) total = 0;
    __syncthreads();
    for (int sweep = 0; sweep < H * W; ++sweep) {        // monotone: every sweep but the last adds a pixel
        if (t == 0) changed = 0;
        __syncthreads();
        bool any = false;
        for (int i = t; i < n; i += 1024) {
            const int y = i / wpr, wx = i - y * wpr;
            const u64 bg = bgw(i), old = reach[i];
            u64 r = old;
            if (y > 0) r |= reach[i - wpr];
            if (y + 1 < H) r |= reach[i + wpr];
            if (wx > 0) r |= reach[i - 1] >> 63;
            if (wx + 1 < wpr) r |= reach[i + 1] << 63;
            r &= bg;
            r = fill_up(r, bg);
            r = fill_down(r, bg);
            if (r != old) { reach[i] = r; any = true; }      // racing readers see old or new: both are valid reached sets
        }
        if (any) changed = 1;
        __syncthreads();
        const int c = changed;
        __syncthreads();
        if (!c) break;
    }
    // border pixels: object pixels with an outside 4-neighbour (beyond the image counts as outside)
    unsigned cnt = 0;
    for (int i = t; i < n; i += 1024) {
        const int y = i / wpr, wx = i - y * wpr;
        const u64 r = reach[i];
        u64 nb = (r << 1) | (r >> 1);
        nb |= wx > 0 ? reach[i - 1] >> 63 : 1ull;
        nb |= wx + 1 < wpr ? reach[i + 1] << 63 : 0ull;
        if (wx == wpr - 1) nb |= 1ull << ((W - 1) & 63);                 // right of the last column: outside
        nb |= y > 0 ? reach[i - wpr] : ~0ull;
        nb |= y + 1 < H ? reach[i + wpr] : ~0ull;
        const u64 b = s[i] & nb & (wx == wpr - 1 ? last_mask : ~0ull);
        bm[i] = b;
        cnt += __popcll(b);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o);
    if ((t & 63) == 0 && cnt) atomicAdd(&total, cnt);
    __syncthreads();                                                     // bm complete (this block wrote it), total summed
    if (t == 0) *count = total;
    // dilation by skimage.morphology.disk(radius): OR of the rows dy away, each spread by floor(sqrt(r^2 - dy^2)) columns
    for (int i = t; i < n; i += 1024) {
        const int y = i / wpr, wx = i - y * wpr;
        u64 acc = 0;
        for (int dy = -radius; dy <= radius; ++dy) {
            const int yy = y + dy;
            if (yy < 0 || yy >= H) continue;
            int ext = 0;
            while ((ext + 1) * (ext + 1) + dy * dy <= radius * radius) ++ext;
            const u64* row = bm + (long)yy * wpr;
            const u64 c = row[wx], l = wx > 0 ? row[wx - 1] : 0ull, rr = wx + 1 < wpr ? row[wx + 1] : 0ull;
            u64 v = c;
            for (int sft = 1; sft <= ext; ++sft) v |= (c << sft) | (l >> (64 - sft)) | (c >> sft) | (rr << (64 - sft));
            acc |= v;
        }
        dl[i] = acc & (wx == wpr - 1 ? last_mask : ~0ull);
    }
}

// 256 threads per (gt, pred) pair: *out_fg = |bmap_pred & dil_gt|, *out_gt = |bmap_gt & dil_pred| over planes of n words
__device__ inline void bnd_pair_body(const u64* __restrict__ bp, const u64* __restrict__ dp, const u64* __restrict__ bg, const u64* __restrict__ dg,
                                     int n, unsigned* __restrict__ out_fg, unsigned* __restrict__ out_gt) {
    __shared__ unsigned acc[2];
    if (threadIdx.x < 2) acc[threadIdx.x] = 0;
    __syncthreads();
    unsigned a = 0, b = 0;
    for (int k = threadIdx.x; k < n; k += 256) {
        a += __popcll(bp[k] & dg[k]);
        b += __popcll(bg[k] & dp[k]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_down(a, o);
        b += __shfl_down(b, o);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&acc[0], a);
        atomicAdd(&acc[1], b);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        *out_fg = acc[0];
        *out_gt = acc[1];
    }
}

}  // namespace quber
