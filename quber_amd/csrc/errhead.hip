// The predicted error maps on the device: what a caller does with the eee_boundary / eee_mask logits of quber_forward.
//   error_decode:     per-pixel argmax of `classes` logit planes -> u8 class map + per-frame class histogram
//                     (reference eval/eval_utils.py:308-328 and explicit_error_estimation/util.py:29-31: `argmax`, one-hot, host copy)
//   error_mask_hist:  pixels of every initial mask per predicted class (which masks does the network reject)
//   error_score:      confusion table of the class map against the explicit TP/TN/FP/FN maps of csrc/errmaps.hip, the target class being
//                     the training target of maskrefiner/modeling/mask_refiner/model.py:185-227 (util.py:29-54 scores the same pair)
//   error_overlay:    the class colours painted over a BGR image (eval_utils.py:315-317)
// All four are pure streams on the caller's stream: no allocation, no synchronisation; every counter table is cleared by the
// zero-fill kernel (launch_zero: memset nodes do not replay) in front of the kernel that adds to it, so a call overwrites its
// outputs and a captured graph replays idempotently.
// Pixels are addressed flat (p = y * W + x): no kernel needs the row structure, so any width runs the 16-byte path as long as the
// plane starts are aligned; what is not aligned takes one pixel per lane.
#include "common.h"

#include <type_traits>

namespace quber {

constexpr int EH_THREADS = 256;

typedef float eh_f4 __attribute__((ext_vector_type(4)));
typedef eh_f4 eh_f4u __attribute__((aligned(4)));       // a 16-byte load at any float address (global memory: dword alignment suffices)

// 0x01 in every byte of `wd` that is non-zero
__device__ __forceinline__ unsigned eh_nz(unsigned wd) { return ((((wd & 0x7f7f7f7fu) + 0x7f7f7f7fu) | wd) & 0x80808080u) >> 7; }
// bits 0, 8, 16, 24 of `m` gathered into bits 0..3 (the partial products land on distinct bits: no carries)
__device__ __forceinline__ unsigned eh_nib(unsigned m) { return (m * 0x01020408u) >> 24; }
// bit i = (byte i of the 16 bytes is non-zero)
__device__ __forceinline__ unsigned eh_nzbits(const uint4& v) {
    return eh_nib(eh_nz(v.x)) | eh_nib(eh_nz(v.y)) << 4 | eh_nib(eh_nz(v.z)) << 8 | eh_nib(eh_nz(v.w)) << 12;
}
// bit i = (byte i of the 16 bytes equals c)
__device__ __forceinline__ unsigned eh_eqbits(const uint4& v, unsigned c) {
    const unsigned k = c * 0x01010101u;
    return eh_nzbits(make_uint4(v.x ^ k, v.y ^ k, v.z ^ k, v.w ^ k)) ^ 0xffffu;
}

template <typename T>
__device__ __forceinline__ T eh_wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;                                            // complete in lane 0
}

// torch.argmax over C values: the first index wins ties (+0.0 == -0.0), a NaN is the maximum and the first NaN wins
template <int C>
__device__ __forceinline__ unsigned eh_argmax(const float (&x)[C]) {
    float best = x[0];
    unsigned idx = 0;
#pragma unroll
    for (int c = 1; c < C; ++c) {
        const float v = x[c];
        if (v > best || (v != v && best == best)) {
            best = v;
            idx = c;
        }
    }
    return idx;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// error_decode.  grid (ceil(HW / 16 / 256), B); L points at plane `first_plane` of frame 0.  A frame's class map is split at the
// 16-byte boundaries of its OUTPUT: an unaligned head (< 16 pixels), whole 16-pixel groups - one per lane: 4 x C dwordx4 loads
// requested together, one 16-byte store -, a tail (< 16 pixels); head and tail are done one pixel per lane by the frame's first block.
// The class counts travel as 16-bit fields of one 64-bit word: wave shuffle, LDS, then C global adds per block.
template <int C, bool HIST>
__global__ __launch_bounds__(EH_THREADS) void error_decode_kernel(const float* __restrict__ L, long frame_stride, long HW,
                                                                  uint8_t* __restrict__ cls, unsigned* __restrict__ hist) {
    __shared__ unsigned sm[4];
    const int b = blockIdx.y;
    const float* Lb = L + (long)b * frame_stride;
    uint8_t* o = cls + (long)b * HW;
    const int head = (int)min((long)((16 - (int)((uintptr_t)o & 15)) & 15), HW);
    const long nbody = (HW - head) >> 4;
    if (HIST) {
        if (threadIdx.x < 4) sm[threadIdx.x] = 0;
        __syncthreads();
    }
    unsigned long long acc = 0;
    const long g = (long)blockIdx.x * EH_THREADS + threadIdx.x;
    if (g < nbody) {
        const long p = head + (g << 4);
        eh_f4u v[C][4];
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int q = 0; q < 4; ++q) v[c][q] = *reinterpret_cast<const eh_f4u*>(Lb + (long)c * HW + p + 4 * q);
        unsigned w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            w[q] = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float x[C];
#pragma unroll
                for (int c = 0; c < C; ++c) x[c] = v[c][q][e];
                const unsigned idx = eh_argmax<C>(x);
                w[q] |= idx << (8 * e);
                acc += 1ull << (16 * idx);
            }
        }
        *reinterpret_cast<uint4*>(o + p) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    if (blockIdx.x == 0 && threadIdx.x < 32) {           // the ragged ends: lanes 0..15 the head, 16..31 the tail
        const int t = threadIdx.x;
        const long tail0 = head + (nbody << 4);
        long p = -1;
        if (t < 16) {
            if (t < head) p = t;
        } else if (tail0 + (t - 16) < HW) {
            p = tail0 + (t - 16);
        }
        if (p >= 0) {
            float x[C];
#pragma unroll
            for (int c = 0; c < C; ++c) x[c] = Lb[(long)c * HW + p];
            const unsigned idx = eh_argmax<C>(x);
            o[p] = (uint8_t)idx;
            acc += 1ull << (16 * idx);
        }
    }
    if (HIST) {
        acc = eh_wave_sum(acc);                          // <= 64 * 17 per field
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const unsigned k = (unsigned)(acc >> (16 * c)) & 0xffffu;
                if (k) atomicAdd(&sm[c], k);
            }
        }
        __syncthreads();
        if (threadIdx.x < C && sm[threadIdx.x]) atomicAdd(&hist[(long)b * C + threadIdx.x], sm[threadIdx.x]);
    }
}

template <int C>
static void decode_launch(const float* L, long frame_stride, long HW, int B, uint8_t* cls, unsigned* hist, hipStream_t st) {
    const dim3 grid((unsigned)max(1L, ((HW >> 4) + EH_THREADS - 1) / EH_THREADS), (unsigned)B);
    if (hist)
        hipLaunchKernelGGL((error_decode_kernel<C, true>), grid, dim3(EH_THREADS), 0, st, L, frame_stride, HW, cls, hist);
    else
        hipLaunchKernelGGL((error_decode_kernel<C, false>), grid, dim3(EH_THREADS), 0, st, L, frame_stride, HW, cls, hist);
}

int launch_error_decode(const float* logits, int n_planes, int first_plane, int classes, int B, int H, int W, uint8_t* cls,
                        unsigned* hist, hipStream_t st) {
    if (B <= 0) return 0;
    if (B > 65535) return fail("error_decode: batch above 65535");
    if (classes < 2 || classes > 4) return fail("error_decode: classes outside 2..4");
    if (first_plane < 0 || (long)first_plane + classes > n_planes) return fail("error_decode: planes first_plane .. first_plane + classes - 1 outside the logits");
    const long HW = (long)H * W;
    if (HW < 1) return fail("error_decode: empty frame");
    if (hist)
        if (int rc = launch_zero(hist, sizeof(unsigned) * (size_t)B * classes, st)) return rc;
    ProfScope prof("error_decode", (4.0 * classes + 1.0) * B * (double)HW, 0.0, st);
    const float* L = logits + (long)first_plane * HW;
    const long fs = (long)n_planes * HW;
    if (classes == 2) decode_launch<2>(L, fs, HW, B, cls, hist, st);
    else if (classes == 3) decode_launch<3>(L, fs, HW, B, cls, hist, st);
    else decode_launch<4>(L, fs, HW, B, cls, hist, st);
    QB_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// error_mask_hist.  The reading pattern of csrc/encode.hip: grid (ceil(HW / (256 * 16 * MH_R)), B, mask chunks); a lane owns MH_R
// groups of 16 pixels, 1 KiB (one wave load) apart, and keeps, per group and class, the 16-bit set of its pixels that carry the class.
// Per mask of its chunk it issues its MH_R 16-byte loads back to back (the next mask's before this one's arithmetic), turns the 16 mask
// bytes of a group into 16 bits and counts the intersections; one wave reduction and up to C LDS adds per mask, C integer adds per
// (block, mask) at the end.  The masks are split over blockIdx.z only as far as the pixel strips alone leave the device short of blocks
// (one 1280x720 frame is 113 strips): a chunk re-reads the class map, 1 / `per` of its mask bytes.
constexpr int MH_R = 2;                                  // measured 2 < 4 < 8 (profiles/r22_error_mask_hist_ab.txt)
constexpr int MH_CHUNK = 2048;                           // most masks per block: the LDS table [masks][C] stays <= 32 KiB
constexpr long MH_SPAN = (long)EH_THREADS * 16 * MH_R;   // pixels per block
constexpr long MH_BLOCKS = 1024;                         // blocks a launch aims for (4 per CU)

template <int C>
__global__ __launch_bounds__(EH_THREADS) void error_mask_hist_kernel(const uint8_t* __restrict__ cls, const uint8_t* __restrict__ masks,
                                                                     int N, int per, long HW, unsigned* __restrict__ out) {
    extern __shared__ unsigned mh_sm[];                  // [per][C]
    const int n0 = blockIdx.z * per, Nc = min(per, N - n0);
    using acc_t = typename std::conditional<(C <= 2), unsigned, unsigned long long>::type;
    const int b = blockIdx.y;
    for (int i = threadIdx.x; i < Nc * C; i += EH_THREADS) mh_sm[i] = 0;
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long base = ((long)blockIdx.x * 4 + wave) * MH_R * 1024 + lane * 16;
    bool act[MH_R];
    unsigned eq[MH_R][C];
#pragma unroll
    for (int r = 0; r < MH_R; ++r) {
        act[r] = base + (long)r * 1024 < HW;             // HW % 16 == 0: a group is inside or outside as a whole
        const uint4 cv = act[r] ? *reinterpret_cast<const uint4*>(cls + (long)b * HW + base + (long)r * 1024) : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int c = 0; c < C; ++c) eq[r][c] = act[r] ? eh_eqbits(cv, (unsigned)c) : 0u;
    }
    const uint8_t* src = masks + ((long)b * N + n0) * HW + base;
    uint4 nxt[MH_R];
#pragma unroll
    for (int r = 0; r < MH_R; ++r) nxt[r] = act[r] ? *reinterpret_cast<const uint4*>(src + (long)r * 1024) : make_uint4(0, 0, 0, 0);
    for (int n = 0; n < Nc; ++n) {
        uint4 v[MH_R];
#pragma unroll
        for (int r = 0; r < MH_R; ++r) v[r] = nxt[r];
        if (n + 1 < Nc) {
#pragma unroll
            for (int r = 0; r < MH_R; ++r)
                nxt[r] = act[r] ? *reinterpret_cast<const uint4*>(src + (long)(n + 1) * HW + (long)r * 1024) : make_uint4(0, 0, 0, 0);
        }
        acc_t acc = 0;
#pragma unroll
        for (int r = 0; r < MH_R; ++r) {
            const unsigned m = eh_nzbits(v[r]);
#pragma unroll
            for (int c = 0; c < C; ++c) acc += (acc_t)__popc(m & eq[r][c]) << (16 * c);
        }
        acc = eh_wave_sum(acc);                          // <= 64 * 64 per field
        if (lane == 0 && acc) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const unsigned k = (unsigned)(acc >> (16 * c)) & 0xffffu;
                if (k) atomicAdd(&mh_sm[n * C + c], k);
            }
        }
    }
    __syncthreads();
    unsigned* ob = out + ((long)b * N + n0) * C;
    for (int i = threadIdx.x; i < Nc * C; i += EH_THREADS)
        if (mh_sm[i]) atomicAdd(&ob[i], mh_sm[i]);
}

// any HW, any alignment: one pixel per lane
template <int C>
__global__ __launch_bounds__(EH_THREADS) void error_mask_hist_generic_kernel(const uint8_t* __restrict__ cls, const uint8_t* __restrict__ masks,
                                                                             int N, int per, long HW, unsigned* __restrict__ out) {
    extern __shared__ unsigned mh_sm[];                  // [per][C]
    const int n0 = blockIdx.z * per, Nc = min(per, N - n0);
    const int b = blockIdx.y;
    for (int i = threadIdx.x; i < Nc * C; i += EH_THREADS) mh_sm[i] = 0;
    __syncthreads();
    const long p = (long)blockIdx.x * EH_THREADS + threadIdx.x;
    const bool active = p < HW;
    const unsigned c0 = active ? cls[(long)b * HW + p] : 255u;
    const unsigned long long one = c0 < (unsigned)C ? 1ull << (16 * c0) : 0ull;
    const uint8_t* src = masks + ((long)b * N + n0) * HW + p;
    for (int n = 0; n < Nc; ++n) {
        unsigned long long acc = (active && src[(long)n * HW] != 0) ? one : 0ull;
        acc = eh_wave_sum(acc);
        if ((threadIdx.x & 63) == 0 && acc) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const unsigned k = (unsigned)(acc >> (16 * c)) & 0xffffu;
                if (k) atomicAdd(&mh_sm[n * C + c], k);
            }
        }
    }
    __syncthreads();
    unsigned* ob = out + ((long)b * N + n0) * C;
    for (int i = threadIdx.x; i < Nc * C; i += EH_THREADS)
        if (mh_sm[i]) atomicAdd(&ob[i], mh_sm[i]);
}

template <int C>
static void mask_hist_launch(bool vec, const uint8_t* cls, const uint8_t* masks, int N, long HW, int B, unsigned* out, hipStream_t st) {
    const long bx = vec ? (HW + MH_SPAN - 1) / MH_SPAN : (HW + EH_THREADS - 1) / EH_THREADS;
    // masks per block: all of them when the pixel strips alone fill the device, else split until about MH_BLOCKS blocks exist
    const long nz = min((long)N, max(1L, (MH_BLOCKS + bx * B - 1) / (bx * B)));
    const int per = (int)min((long)MH_CHUNK, (N + nz - 1) / nz);
    const dim3 grid((unsigned)bx, (unsigned)B, (unsigned)((N + per - 1) / per));
    const size_t lds = sizeof(unsigned) * (size_t)per * C;
    if (vec)
        hipLaunchKernelGGL(error_mask_hist_kernel<C>, grid, dim3(EH_THREADS), lds, st, cls, masks, N, per, HW, out);
    else
        hipLaunchKernelGGL(error_mask_hist_generic_kernel<C>, grid, dim3(EH_THREADS), lds, st, cls, masks, N, per, HW, out);
}

int launch_error_mask_hist(const uint8_t* cls, const uint8_t* masks, int B, int N, int classes, int H, int W, unsigned* out,
                           hipStream_t st) {
    if (B <= 0 || N <= 0) return 0;
    if (B > 65535) return fail("error_mask_hist: batch above 65535");
    if (classes < 2 || classes > 4) return fail("error_mask_hist: classes outside 2..4");
    const long HW = (long)H * W;
    if (HW < 1 || (HW + EH_THREADS - 1) / EH_THREADS > 0x7fffffffL) return fail("error_mask_hist: frame size");
    const bool vec = HW % 16 == 0 && ((uintptr_t)cls & 15) == 0 && ((uintptr_t)masks & 15) == 0;
    if (int rc = launch_zero(out, sizeof(unsigned) * (size_t)B * N * classes, st)) return rc;
    ProfScope prof("error_mask_hist", (double)B * (double)HW * (N + 1.0) + 4.0 * B * N * classes, 0.0, st);
    if ((N + MH_CHUNK - 1) / MH_CHUNK > 65535) return fail("error_mask_hist: too many masks");
    if (classes == 2) mask_hist_launch<2>(vec, cls, masks, N, HW, B, out, st);
    else if (classes == 3) mask_hist_launch<3>(vec, cls, masks, N, HW, B, out, st);
    else mask_hist_launch<4>(vec, cls, masks, N, HW, B, out, st);
    QB_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// error_score.  Target class of a pixel from its four explicit bytes (TP, TN, FP, FN; the first set plane of the target stack of
// model.py:185-227, `C` = none), cell = target * C + predicted; a lane counts its pixels per cell in 5-bit fields of two 64-bit words,
// the wave sums them as 16-bit fields, the block in LDS, and (C + 1) * C 64-bit adds per block reach the table.
__device__ __forceinline__ unsigned eh_target(bool tp, bool tn, bool fp, bool fn, int et) {
    if (et == 0) return tp ? 0u : tn ? 1u : fp ? 2u : fn ? 3u : 4u;          // e3
    if (et == 1) return (tp || tn) ? 0u : (fp || fn) ? 1u : 2u;              // e2
    if (et == 2) return (tp || tn) ? 0u : fp ? 1u : fn ? 2u : 3u;            // e33
    return fp ? 0u : fn ? 1u : 2u;                                           // e32
}

// grid (ceil(HW / (256 * PIX)), B); PIX = 16: 16-byte loads (HW % 16 == 0 and aligned bases), PIX = 1: any shape
template <int PIX>
__global__ __launch_bounds__(EH_THREADS) void error_score_kernel(const uint8_t* __restrict__ cls, const uint8_t* __restrict__ expl,
                                                                 long expl_frame_stride, long HW, int C, int et,
                                                                 unsigned long long* __restrict__ table) {
    __shared__ unsigned sm[20];
    const int b = blockIdx.y;
    if (threadIdx.x < 20) sm[threadIdx.x] = 0;
    __syncthreads();
    const long p = ((long)blockIdx.x * EH_THREADS + threadIdx.x) * PIX;
    unsigned long long lo = 0, hi = 0;                   // cells 0..11, 12..19: 5 bits each (<= 16 pixels per lane)
    if (p < HW) {
        const uint8_t* e = expl + (long)b * expl_frame_stride + p;
        unsigned cw[PIX == 16 ? 4 : 1], xw[4][PIX == 16 ? 4 : 1];
        if constexpr (PIX == 16) {
            const uint4 cv = *reinterpret_cast<const uint4*>(cls + (long)b * HW + p);
            cw[0] = cv.x; cw[1] = cv.y; cw[2] = cv.z; cw[3] = cv.w;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint4 xv = *reinterpret_cast<const uint4*>(e + (long)j * HW);
                xw[j][0] = xv.x; xw[j][1] = xv.y; xw[j][2] = xv.z; xw[j][3] = xv.w;
            }
        } else {
            cw[0] = cls[(long)b * HW + p];
#pragma unroll
            for (int j = 0; j < 4; ++j) xw[j][0] = e[(long)j * HW];
        }
#pragma unroll
        for (int i = 0; i < PIX; ++i) {
            const int q = i >> 2, s = 8 * (i & 3);
            const unsigned pred = (cw[q] >> s) & 0xffu;
            const unsigned t = eh_target(((xw[0][q] >> s) & 0xffu) != 0, ((xw[1][q] >> s) & 0xffu) != 0, ((xw[2][q] >> s) & 0xffu) != 0,
                                         ((xw[3][q] >> s) & 0xffu) != 0, et);
            const unsigned cell = t * (unsigned)C + pred;            // < 20 when pred < C
            const bool ok = pred < (unsigned)C;                      // a class outside the head's range is counted nowhere
            lo += (ok && cell < 12u) ? 1ull << (5 * cell) : 0ull;
            hi += (ok && cell >= 12u) ? 1ull << (5 * (cell - 12u)) : 0ull;
        }
    }
#pragma unroll
    for (int k = 0; k < 20; k += 4) {
        unsigned long long f = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int cell = k + i;
            const unsigned long long cnt = (cell < 12 ? lo >> (5 * cell) : hi >> (5 * (cell - 12))) & 31ull;
            f |= cnt << (16 * i);
        }
        f = eh_wave_sum(f);                              // <= 64 * 16 per field
        if ((threadIdx.x & 63) == 0 && f) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const unsigned v = (unsigned)(f >> (16 * i)) & 0xffffu;
                if (v) atomicAdd(&sm[k + i], v);
            }
        }
    }
    __syncthreads();
    const int cells = (C + 1) * C;
    if ((int)threadIdx.x < cells && sm[threadIdx.x]) atomicAdd(&table[(long)b * cells + threadIdx.x], (unsigned long long)sm[threadIdx.x]);
}

int launch_error_score(const uint8_t* cls, const uint8_t* expl, int kind, int error_type, int classes, int B, int H, int W,
                       unsigned long long* table, hipStream_t st) {
    if (B <= 0) return 0;
    if (B > 65535) return fail("error_score: batch above 65535");
    if (kind != 0 && kind != 1) return fail("error_score: kind must be 0 (region) or 1 (boundary)");
    static const int want[4] = {4, 2, 3, 2};             // e3, e2, e33, e32
    if (error_type < 0 || error_type > 3) return fail("error_score: error_type outside 0..3 (e3, e2, e33, e32)");
    if (classes != want[error_type]) return fail("error_score: classes must be 4 (e3), 2 (e2), 3 (e33) or 2 (e32)");
    const long HW = (long)H * W;
    if (HW < 1 || (HW + EH_THREADS - 1) / EH_THREADS > 0x7fffffffL) return fail("error_score: frame size");
    const uint8_t* e = expl + (long)kind * 4 * HW;
    const bool vec = HW % 16 == 0 && ((uintptr_t)cls & 15) == 0 && ((uintptr_t)e & 15) == 0;
    const int cells = (classes + 1) * classes;
    if (int rc = launch_zero(table, sizeof(unsigned long long) * (size_t)B * cells, st)) return rc;
    ProfScope prof("error_score", 5.0 * B * (double)HW + 8.0 * B * cells, 0.0, st);
    if (vec) {
        const long per = (long)EH_THREADS * 16;
        hipLaunchKernelGGL(error_score_kernel<16>, dim3((unsigned)((HW + per - 1) / per), (unsigned)B), dim3(EH_THREADS), 0, st, cls, e,
                           8 * HW, HW, classes, error_type, table);
    } else {
        hipLaunchKernelGGL(error_score_kernel<1>, dim3((unsigned)((HW + EH_THREADS - 1) / EH_THREADS), (unsigned)B), dim3(EH_THREADS), 0,
                           st, cls, e, 8 * HW, HW, classes, error_type, table);
    }
    QB_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// error_overlay.  Pixels are flat over the whole batch.  A lane of the 16-byte path owns 16 pixels: three 16-byte words of BGR and one
// of classes in, three out; it reads all of them before it writes, so the output may be the input.  Buffers that are not 16-byte
// aligned, and the last P % 16 pixels, go one pixel per lane.
struct OverlayColors {
    unsigned c[4];                                       // bits 0-7 B, 8-15 G, 16-23 R, bit 24 = paint
};

__device__ __forceinline__ unsigned eh_color(const OverlayColors& k, unsigned cl) {
    return cl == 0 ? k.c[0] : cl == 1 ? k.c[1] : cl == 2 ? k.c[2] : cl == 3 ? k.c[3] : 0u;
}

__global__ __launch_bounds__(EH_THREADS) void error_overlay_kernel(const uint8_t* bgr, const uint8_t* __restrict__ cls, uint8_t* out,
                                                                   long P, OverlayColors k) {
    const long g = (long)blockIdx.x * EH_THREADS + threadIdx.x;
    if (g >= (P >> 4)) return;
    const uint4* src = reinterpret_cast<const uint4*>(bgr) + 3 * g;
    const uint4 a0 = src[0], a1 = src[1], a2 = src[2];
    const uint4 cv = reinterpret_cast<const uint4*>(cls)[g];
    unsigned w[12] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w};
    const unsigned cw[4] = {cv.x, cv.y, cv.z, cv.w};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const unsigned col = eh_color(k, (cw[i >> 2] >> (8 * (i & 3))) & 0xffu);
        const unsigned m = (col >> 24) & 1u ? 0xffffffu : 0u;
        const unsigned v = col & m;
        const int j = (3 * i) >> 2, s = 8 * ((3 * i) & 3);
        w[j] = (w[j] & ~(m << s)) | (v << s);
        if (s > 8) w[j + 1] = (w[j + 1] & ~(m >> (32 - s))) | (v >> (32 - s));     // j + 1 <= 11: pixel 15 ends word 11 exactly
    }
    uint4* dst = reinterpret_cast<uint4*>(out) + 3 * g;
    dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
    dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
    dst[2] = make_uint4(w[8], w[9], w[10], w[11]);
}

// pixels [p0, P), one per lane
__global__ __launch_bounds__(EH_THREADS) void error_overlay_scalar_kernel(const uint8_t* bgr, const uint8_t* __restrict__ cls, uint8_t* out,
                                                                          long p0, long P, OverlayColors k) {
    const long p = p0 + (long)blockIdx.x * EH_THREADS + threadIdx.x;
    if (p >= P) return;
    const unsigned col = eh_color(k, cls[p]);
    const bool paint = (col >> 24) & 1u;
    const uint8_t b0 = bgr[3 * p], b1 = bgr[3 * p + 1], b2 = bgr[3 * p + 2];
    out[3 * p] = paint ? (uint8_t)col : b0;
    out[3 * p + 1] = paint ? (uint8_t)(col >> 8) : b1;
    out[3 * p + 2] = paint ? (uint8_t)(col >> 16) : b2;
}

int launch_error_overlay(const uint8_t* bgr, const uint8_t* cls, int B, int H, int W, const unsigned* colors, uint8_t* out,
                         hipStream_t st) {
    if (B <= 0) return 0;
    const long P = (long)B * H * W;
    if (P < 1) return fail("error_overlay: empty frame");
    OverlayColors k;
    for (int i = 0; i < 4; ++i) k.c[i] = colors[i];
    const bool vec = (((uintptr_t)bgr | (uintptr_t)cls | (uintptr_t)out) & 15) == 0;
    const long body = vec ? P >> 4 : 0;                  // 16-pixel groups of the 16-byte path
    const long rest = P - (body << 4);
    if ((body + EH_THREADS - 1) / EH_THREADS > 0x7fffffffL || (rest + EH_THREADS - 1) / EH_THREADS > 0x7fffffffL)
        return fail("error_overlay: too many pixels");
    ProfScope prof("error_overlay", 7.0 * (double)P, 0.0, st);
    if (body > 0)
        hipLaunchKernelGGL(error_overlay_kernel, dim3((unsigned)((body + EH_THREADS - 1) / EH_THREADS)), dim3(EH_THREADS), 0, st, bgr, cls,
                           out, P, k);
    if (rest > 0)
        hipLaunchKernelGGL(error_overlay_scalar_kernel, dim3((unsigned)((rest + EH_THREADS - 1) / EH_THREADS)), dim3(EH_THREADS), 0, st,
                           bgr, cls, out, body << 4, P, k);
    QB_CHECK(hipGetLastError());
    return 0;
}

}  // namespace quber
