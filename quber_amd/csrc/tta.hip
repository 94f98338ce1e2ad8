// Horizontal-flip test-time augmentation (INTEGRATION.md "Test-time augmentation"): the two streaming kernels around the
// one forward of 2B frames.
//   tta_flip_u8:  the W-mirror of P planes u8 [H][W][C] (C = 3: BGR / depth, C = 1: initial masks), written right behind
//                 the source planes - the caller fills frames [0, B) of a 2B buffer, this fills [B, 2B).
//   tta_merge:    out[b,c,y,x] = (L[b,c,y,x] + s_c * L[B+b,c,y,W-1-x]) * 0.5f, s_c = -1 on the x-offset plane (plane 3),
//                 +1 on every other plane: SemanticSegmentorWithTTA's flip-back and average (reference
//                 maskrefiner/test_time_augmentation.py:72-95), one fp32 rounding for the add, then an exact halving.
// Both are pure streams on the caller's stream: no allocation, no synchronisation.
#include "common.h"

namespace quber {

constexpr int TTA_THREADS = 256;
constexpr int TTA_SPAN = 16384;         // source bytes a flip block stages in LDS (whole rows; one row if a row is longer)
constexpr int TTA_MAX_ROW = 65536 - 48; // longest row (W * C bytes) the flip takes: the LDS of one work-group

// The 16 output bytes k .. k+15 of one row (k + 16 <= W*C), gathered from the row's mirror image in LDS (row byte 0 at lds[rb]).
// C = 1: source bytes W-16-k .. W-1-k in reverse - five aligned LDS dwords and four byte permutes.
// C = 3: output byte b is pixel x0 + (p+b)/3, channel (p+b)%3 (x0 = k/3, p = k%3); its source, relative to channel 0 of the
// mirrored pixel W-1-x0, is -3*((p+b)/3) + (p+b)%3, in [-15, 2]: sixteen byte reads at constant offsets per phase p.
template <int C>
__device__ __forceinline__ uint4 tta_gather16(const uint8_t* lds, int rb, int W, int k);

template <>
__device__ __forceinline__ uint4 tta_gather16<1>(const uint8_t* lds, int rb, int W, int k) {
    const int s = rb + W - 16 - k;                                       // LDS index of the lowest source byte
    const int a = s & ~3, ph = s - a;
    const unsigned* d = reinterpret_cast<const unsigned*>(lds + a);
    const unsigned d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3], d4 = d[4];
    // byte i of an output dword = byte (ph + 3 - i) of {hi:lo}
    const unsigned sel = (unsigned)(ph + 3) | (unsigned)(ph + 2) << 8 | (unsigned)(ph + 1) << 16 | (unsigned)ph << 24;
    return make_uint4(__builtin_amdgcn_perm(d4, d3, sel), __builtin_amdgcn_perm(d3, d2, sel), __builtin_amdgcn_perm(d2, d1, sel),
                      __builtin_amdgcn_perm(d1, d0, sel));
}

template <int P>
__device__ __forceinline__ uint4 tta_gather16_c3(const uint8_t* q) {    // q = LDS address of relative offset -15
    unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int b = 0; b < 16; ++b) w[b >> 2] |= (unsigned)q[15 - 3 * ((P + b) / 3) + (P + b) % 3] << (8 * (b & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

template <>
__device__ __forceinline__ uint4 tta_gather16<3>(const uint8_t* lds, int rb, int W, int k) {
    const int x0 = k / 3, p = k - 3 * x0;
    const uint8_t* q = lds + rb + (W - 1 - x0) * 3 - 15;                 // >= the row's start: pixel x0 + 5 is in the word
    return p == 0 ? tta_gather16_c3<0>(q) : p == 1 ? tta_gather16_c3<1>(q) : tta_gather16_c3<2>(q);
}

// One block mirrors `rpb` whole rows (rows of W*C bytes, consecutive in memory): the rows' bytes go to LDS through 16-byte loads
// (bytewise at the unaligned ends of the span), then every lane assembles aligned 16-byte output words from LDS - the source
// offset of output byte (x, c) of a row is (W-1-x)*C + c, stepped incrementally - and writes them with 16-byte stores (bytewise
// at the unaligned ends of the output span).  LDS byte i holds the source byte at address align16_down(span start) + i.
template <int C>
__global__ __launch_bounds__(TTA_THREADS) void tta_flip_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                               long rows, int W, int rpb) {
    extern __shared__ uint4 tta_lds4[];
    uint8_t* lds = reinterpret_cast<uint8_t*>(tta_lds4);
    const int Rb = W * C;
    const long r0 = (long)blockIdx.x * rpb;
    const int nr = (int)min((long)rpb, rows - r0);
    const long s0 = r0 * Rb;
    const long len = (long)nr * Rb;
    const int t = threadIdx.x;

    // ---- load the span [src + s0, src + s0 + len) ----
    {
        const uintptr_t g0 = (uintptr_t)(src + s0), g1 = g0 + len;
        const uintptr_t lo = g0 & ~(uintptr_t)15;
        const uintptr_t ha = min((g0 + 15) & ~(uintptr_t)15, g1);     // end of the unaligned head
        const uintptr_t ta = max(g1 & ~(uintptr_t)15, ha);             // start of the unaligned tail
        for (int i = t; i < (int)(ha - g0); i += TTA_THREADS) lds[g0 - lo + i] = reinterpret_cast<const uint8_t*>(g0)[i];
        const int nch = (int)(ta - ha) >> 4;
        const uint4* body = reinterpret_cast<const uint4*>(ha);
        uint4* lbody = reinterpret_cast<uint4*>(lds + (ha - lo));
        for (int i = t; i < nch; i += TTA_THREADS) lbody[i] = body[i];
        for (int i = t; i < (int)(g1 - ta); i += TTA_THREADS) lds[ta - lo + i] = reinterpret_cast<const uint8_t*>(ta)[i];
    }
    __syncthreads();
    const uint8_t* ls = lds + (((uintptr_t)(src + s0)) & 15);        // LDS address of span byte 0

    // ---- write the span [dst + s0, dst + s0 + len) ----
    const uintptr_t d0 = (uintptr_t)(dst + s0), d1 = d0 + len;
    const uintptr_t ha = min((d0 + 15) & ~(uintptr_t)15, d1);
    const uintptr_t ta = max(d1 & ~(uintptr_t)15, ha);
    // unaligned ends: one byte per lane
    // (span offsets fit an int: a span is at most max(TTA_SPAN, TTA_MAX_ROW) bytes)
    const int nh = (int)(ha - d0), nt = (int)(d1 - ta);
    for (int i = t; i < nh + nt; i += TTA_THREADS) {
        const int j = i < nh ? i : (int)(ta - d0) + (i - nh);         // span offset of the byte
        const int row = j / Rb, k = j - row * Rb;
        const int x = k / C, c = k - x * C;
        reinterpret_cast<uint8_t*>(d0)[j] = ls[row * Rb + (W - 1 - x) * C + c];
    }
    // aligned body: 16 bytes per lane.  A word inside one row takes the fast form (tta_gather16); one that crosses into the next row
    // steps byte by byte.
    const int nch = (int)(ta - ha) >> 4;
    uint4* out = reinterpret_cast<uint4*>(ha);
    const int lso = (int)(((uintptr_t)(src + s0)) & 15);              // LDS index of span byte 0
    const float inv_rb = 1.0f / (float)Rb;
    for (int q = t; q < nch; q += TTA_THREADS) {
        const int j = (int)(ha - d0) + (q << 4);
        int row = (int)((float)j * inv_rb);                              // j / Rb (j < 2^17: the float estimate is off by at most one)
        if (row * Rb > j) --row;
        else if ((row + 1) * Rb <= j) ++row;
        int k = j - row * Rb;
        if (k + 16 <= Rb) {
            out[q] = tta_gather16<C>(lds, lso + row * Rb, W, k);
            continue;
        }
        int x = k / C, c = k - x * C;
        int rowbase = row * Rb;
        int off = (W - 1 - x) * C + c;                                   // source offset inside the row
        unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            w[b >> 2] |= (unsigned)ls[rowbase + off] << (8 * (b & 3));
            if (++k == Rb) {                                             // next row: its last pixel, channel 0
                k = 0;
                c = 0;
                rowbase += Rb;
                off = (W - 1) * C;
            } else if (C == 1) {
                off -= 1;
            } else if (++c == C) {                                       // (x, C-1) -> (x+1, 0): one pixel back
                c = 0;
                off -= 2 * C - 1;
            } else {
                off += 1;
            }
        }
        out[q] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// grid (ceil(H*W / (256 * V)), B * planes); plane (b, c) of the output, from planes (b, c) and (B + b, c) of the input
template <bool VEC>
__global__ __launch_bounds__(TTA_THREADS) void tta_merge_kernel(const float* __restrict__ L, float* __restrict__ out, int B,
                                                                int planes, int H, int W) {
    const int bc = blockIdx.y;
    const int b = bc / planes, c = bc - b * planes;
    const long HW = (long)H * W;
    const float* a = L + (long)bc * HW;
    const float* f = L + ((long)(B + b) * planes + c) * HW;
    float* o = out + (long)bc * HW;
    const float s = c == 3 ? -1.f : 1.f;                                 // plane 3 = off_x (csrc/postproc.hip: fg, centre, off_y, off_x)
    const long e = ((long)blockIdx.x * TTA_THREADS + threadIdx.x) * (VEC ? 4 : 1);
    if (e >= HW) return;
    const int y = (int)(e / W), x = (int)(e - (long)y * W);
    if (VEC) {                                                           // W % 4 == 0: the mirrored quad is aligned too
        const float4 va = *reinterpret_cast<const float4*>(a + e);
        const float4 vf = *reinterpret_cast<const float4*>(f + (long)y * W + (W - 4 - x));
        float4 r;
        r.x = (va.x + s * vf.w) * 0.5f;
        r.y = (va.y + s * vf.z) * 0.5f;
        r.z = (va.z + s * vf.y) * 0.5f;
        r.w = (va.w + s * vf.x) * 0.5f;
        *reinterpret_cast<float4*>(o + e) = r;
    } else {
        o[e] = (a[e] + s * f[(long)y * W + (W - 1 - x)]) * 0.5f;
    }
}

int launch_tta_flip_u8(const uint8_t* src, uint8_t* dst, long planes, int H, int W, int C, hipStream_t st) {
    if (planes <= 0) return 0;
    if (C != 1 && C != 3) return fail("tta_flip: C must be 1 or 3");
    const long Rb = (long)W * C;
    if (Rb < 1 || Rb > TTA_MAX_ROW) return fail("tta_flip: row of W * C bytes outside 1..65488");
    const long rows = planes * H;
    const int rpb = (int)max(1L, (long)TTA_SPAN / Rb);
    const long blocks = (rows + rpb - 1) / rpb;
    if (blocks > 0x7fffffffL) return fail("tta_flip: too many rows");
    const size_t lds = (((size_t)rpb * Rb + 32) + 15) & ~(size_t)15;    // + the dword reads past a span's end (tta_gather16<1>)
    ProfScope prof("tta_flip", 2.0 * (double)rows * Rb, 0.0, st);
    if (C == 1)
        hipLaunchKernelGGL(tta_flip_kernel<1>, dim3((unsigned)blocks), dim3(TTA_THREADS), lds, st, src, dst, rows, W, rpb);
    else
        hipLaunchKernelGGL(tta_flip_kernel<3>, dim3((unsigned)blocks), dim3(TTA_THREADS), lds, st, src, dst, rows, W, rpb);
    QB_CHECK(hipGetLastError());
    return 0;
}

int launch_tta_merge(const float* logits2, int planes, int B, int H, int W, float* out, hipStream_t st) {
    if (B <= 0) return 0;
    if ((long)B * planes > 65535) return fail("tta_merge: batch * planes above 65535");
    const long HW = (long)H * W;
    const bool vec = W % 4 == 0 && ((uintptr_t)logits2 & 15) == 0 && ((uintptr_t)out & 15) == 0;
    const long per = (long)TTA_THREADS * (vec ? 4 : 1);
    const dim3 grid((unsigned)((HW + per - 1) / per), (unsigned)(B * planes));
    ProfScope prof("tta_merge", 12.0 * B * planes * (double)HW, 2.0 * B * planes * (double)HW, st);
    if (vec)
        hipLaunchKernelGGL(tta_merge_kernel<true>, grid, dim3(TTA_THREADS), 0, st, logits2, out, B, planes, H, W);
    else
        hipLaunchKernelGGL(tta_merge_kernel<false>, grid, dim3(TTA_THREADS), 0, st, logits2, out, B, planes, H, W);
    QB_CHECK(hipGetLastError());
    return 0;
}

}  // namespace quber
