// Bit planes of u8 masks and the pair-count tile over them, shared by masknms.hip (the square table of one set of masks) and cocoap.hip
// (the rectangular table of detections x ground truths).  A plane: 32-bit words, rows padded to whole words (bit k of word j of a row =
// pixel 32 j + k), the plane padded with zero words to a multiple of 4 words so that a tile stages it in 16-byte pieces.
#pragma once
#include "common.h"

namespace quber {

// words of one padded plane
static inline long mn_plane_words(int H, int W) { return (((long)H * ((W + 31) / 32)) + 3) / 4 * 4; }

// 0x01 per non-zero byte of w -> 4 bits (the multiplier moves bits 0, 8, 16, 24 to 21, 22, 23, 24; no two products share a bit)
__device__ __forceinline__ unsigned mn_nibble(unsigned w) {
    const unsigned nz = ((((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u) >> 7;
    return ((nz * 0x00204081u) >> 21) & 0xfu;
}
__device__ __forceinline__ unsigned mn_bits16(uint4 v) {
    return mn_nibble(v.x) | mn_nibble(v.y) << 4 | mn_nibble(v.z) << 8 | mn_nibble(v.w) << 12;
}

// word i (< H * wpr) of the plane of `mask` (u8 [H][W], non-zero = inside).  ALIGNED: W % 16 == 0 and a 16-byte aligned mask, the lane
// reads its 32 mask bytes as two 16-byte loads (x0 + 16 <= W); else byte by byte.
template <bool ALIGNED>
__device__ __forceinline__ unsigned mn_pack_word(const uint8_t* __restrict__ mask, int i, int W, int wpr) {
    const int y = i / wpr, x0 = (i - y * wpr) * 32;
    const uint8_t* p = mask + (size_t)y * W + x0;
    unsigned bits = 0;
    if (ALIGNED) {
        bits = mn_bits16(*reinterpret_cast<const uint4*>(p));
        if (x0 + 16 < W) bits |= mn_bits16(*reinterpret_cast<const uint4*>(p + 16)) << 16;
    } else {
        const int nb = min(32, W - x0);
        for (int k = 0; k < nb; ++k) bits |= (unsigned)(p[k] != 0) << k;
    }
    return bits;
}

// One block of TILE * TILE = 256 lanes counts the pixels inside both planes for a TILE x TILE tile of pairs over the words [w0, w1) of
// the planes (w0 and the plane length multiples of 4).  Lane t stages piece t % 16 (4 words) of row t / 16 of each group per step of SLAB
// words - row_a / row_b: word 0 of that row's plane, or null for a row outside the table (staged as zeros) - and owns the pair (row
// t / 16 of group A, row t % 16 of group B): popc in a register, 16 bytes per plane and LDS access.  sm: 2 * TILE * PITCH words of LDS,
// 16-byte aligned.  LDS rows have a pitch of PITCH = SLAB + 4 words: pitch / 4 is odd, so the 16 rows the lanes of one ds_read_b128 lane
// group can address start on 16 different 4-bank slots of the 64 banks; lanes on the same row read the same address (a broadcast).
// Every lane of the block must call it (barriers).  -> the lane's count.
template <int TILE, int SLAB, int PITCH>
__device__ __forceinline__ unsigned mn_gram_tile(const unsigned* __restrict__ row_a, const unsigned* __restrict__ row_b, int w0, int w1,
                                                 unsigned* sm) {
    static_assert(TILE * TILE == 256 && SLAB % 4 == 0 && PITCH % 4 == 0 && (PITCH / 4) % 2 == 1 && PITCH >= SLAB, "gram tile layout");
    static_assert(TILE * (SLAB / 4) == 256, "one 16-byte piece per lane stages a slab of one group");
    const int t = threadIdx.x;
    const int srow = t >> 4, sq = (t & 15) * 4;
    const int ra = t >> 4, rb = t & 15;
    unsigned acc = 0;
    for (int w = w0; w < w1; w += SLAB) {
        const bool in = w + sq < w1;                         // the plane length and w are multiples of 4: a piece is inside or outside as a whole
        uint4 va = make_uint4(0, 0, 0, 0), vb = va;
        if (in && row_a) va = *reinterpret_cast<const uint4*>(row_a + w + sq);
        if (in && row_b) vb = *reinterpret_cast<const uint4*>(row_b + w + sq);
        __syncthreads();                                     // the previous step's reads are done
        *reinterpret_cast<uint4*>(sm + srow * PITCH + sq) = va;
        *reinterpret_cast<uint4*>(sm + (TILE + srow) * PITCH + sq) = vb;
        __syncthreads();
        const uint4* pa = reinterpret_cast<const uint4*>(sm + ra * PITCH);
        const uint4* pb = reinterpret_cast<const uint4*>(sm + (TILE + rb) * PITCH);
#pragma unroll
        for (int k = 0; k < SLAB / 4; ++k) {
            const uint4 a = pa[k], c = pb[k];
            acc += __popc(a.x & c.x) + __popc(a.y & c.y) + __popc(a.z & c.z) + __popc(a.w & c.w);
        }
    }
    return acc;
}

}  // namespace quber
