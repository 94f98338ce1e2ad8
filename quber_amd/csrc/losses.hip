// Validation losses on the device (include/quber_hip.h: quber_loss_targets, quber_losses; the definition is in INTEGRATION.md "Validation
// losses" and, as numpy / float64 torch, in tests/test_losses_cpu.py: loss_targets_np, losses_ref).  Restates the reference's training
// targets - PanopticDeepLabTargetGenerator, maskrefiner/data/dataset_mappers/target_generator.py:8-165, for datasets whose segments are all
// things and none crowd - and the five values of its loss dict (maskrefiner/modeling/mask_refiner/model.py:36-72, 672-687, 766-802), per frame.
//
// Stream-ordered launches, no host copy, no memset node; every output is overwritten by every call:
//   targets  zero -> moments (per id the pixel count, sum of y, sum of x as integers: a block of 256 consecutive pixels reduces in LDS - only
//            the first and the last pixel of a run of equal ids in a row touch LDS, each with the run's prefix sums up to its own position, so
//            the lanes of a wave rarely meet on one address - then one 64-bit integer atomicAdd per used (block, id, sum) into a zero-filled
//            table) -> centres (one lane per id: the float64 division, rint, the area test) -> paint (per pixel the offsets of its own id and
//            the centre heat as a GATHER: the maximum, over the frame's centres whose window holds the pixel, of the host's Gaussian table,
//            which sits in LDS - deterministic, no float atomics, no scatter).
//   losses   terms (one pass over every logit and target plane: the per-pixel terms in float64 from the float32 inputs, block partials in a
//            fixed layout; the weighted foreground term also as a float64 plane when top_k < 1) -> [select: the k-th largest of a frame's
//            plane by an MSB-first radix select on the bit patterns, 11 bits a pass, 6 passes whatever the data; the sum of the values above
//            it] -> finish (one block per frame adds the partials in block order and forms the ratios).
// No floating-point atomics anywhere: two runs give the same bits.
#include "common.h"
#include "../../include/quber_hip.h"

namespace quber {

constexpr int LS_T = 256;
constexpr int LS_MAXID = 254;
constexpr int LT_CHUNK = 4096;               // pixels of a paint block: the Gaussian table is loaded into LDS once per block
constexpr int LS_CHUNK = 2048;               // pixels of a terms / histogram block
constexpr int LS_NACC = 30;                  // fg, centre numerator, weight sum, offset numerator, 2 heads x (ce, inter[4], target[4], prob[4])
constexpr int LS_BINS = 2048;
constexpr int LS_PASSES = 6;

struct LtCentre { double cy, cx; int py, px, area, small; };

// ---- targets: moments -----------------------------------------------------------------------------------------------------------------
// grid (ceil(HW / 256), B).  mom u64 [B][n][3] = (count, sum y, sum x), zero on entry.  A run [xa, xb] of one id in a row adds
// (xb + 1 - xa, y (xb + 1 - xa), T(xb + 1) - T(xa)), T(k) = k (k - 1) / 2: its last pixel adds the terms in xb + 1, its first one subtracts
// the terms in xa, modulo 2^32 - a block's true sums (<= 256 max(H, W)) fit 32 bits, so the wrapped partial sums end on them.
__global__ __launch_bounds__(LS_T) void lt_moment_kernel(const int* __restrict__ labels, int n, int H, int W, unsigned long long* __restrict__ mom) {
    __shared__ unsigned s_m[LS_MAXID * 3];
    const int t = threadIdx.x, b = blockIdx.y;
    for (int k = t; k < n * 3; k += LS_T) s_m[k] = 0;
    __syncthreads();
    const long HW = (long)H * W, p = (long)blockIdx.x * LS_T + t;
    if (p < HW) {
        const int* f = labels + (size_t)b * HW;
        const int id = f[p];
        if (id >= 1 && id <= n) {
            const unsigned y = (unsigned)(p / W), x = (unsigned)(p - (long)y * W);
            const bool first = t == 0 || x == 0 || f[p - 1] != id;
            const bool last = t == LS_T - 1 || x == (unsigned)W - 1 || f[p + 1] != id;       // (x < W - 1: p + 1 < HW)
            unsigned* m = s_m + (id - 1) * 3;
            if (first && last) { atomicAdd(m, 1u); atomicAdd(m + 1, y); atomicAdd(m + 2, x); }
            else if (first) {
                atomicAdd(m, 0u - x); atomicAdd(m + 1, 0u - y * x);
                atomicAdd(m + 2, 0u - (unsigned)((unsigned long long)x * (x - 1) / 2));        // (x = 0: 0 times the wrapped x - 1 is still 0)
            } else if (last) {
                atomicAdd(m, x + 1); atomicAdd(m + 1, y * (x + 1));
                atomicAdd(m + 2, (unsigned)((unsigned long long)(x + 1) * x / 2));
            }
        }
    }
    __syncthreads();
    for (int k = t; k < n; k += LS_T)
        if (s_m[k * 3]) {
            unsigned long long* g = mom + ((size_t)b * n + k) * 3;
            atomicAdd(g, (unsigned long long)s_m[k * 3]); atomicAdd(g + 1, (unsigned long long)s_m[k * 3 + 1]);
            atomicAdd(g + 2, (unsigned long long)s_m[k * 3 + 2]);
        }
}

// one lane per (frame, id): cen [B][254], points f64 [B][n][2] = (cy, cx), area i32 [B][n]; an id without a pixel: zeros, and a peak no window reaches
__global__ __launch_bounds__(LS_T) void lt_centre_kernel(const unsigned long long* __restrict__ mom, int total, int n, int small_area,
                                                         LtCentre* __restrict__ cen, double* __restrict__ points, int* __restrict__ area) {
    const int k = blockIdx.x * LS_T + threadIdx.x;
    if (k >= total) return;
    const int b = k / n, i = k - b * n;
    const unsigned long long cnt = mom[(size_t)k * 3], sy = mom[(size_t)k * 3 + 1], sx = mom[(size_t)k * 3 + 2];
    LtCentre c;
    c.cy = 0.0; c.cx = 0.0; c.py = c.px = -(1 << 28); c.area = 0; c.small = 0;
    if (cnt) {
        c.cy = (double)sy / (double)cnt;                     // the integer sums are exact: one rounding (np.mean of the index arrays)
        c.cx = (double)sx / (double)cnt;
        c.py = (int)rint(c.cy);                              // ties to even: Python's round
        c.px = (int)rint(c.cx);
        c.area = (int)cnt;
        c.small = cnt < (unsigned long long)small_area ? 1 : 0;
    }
    cen[(size_t)b * LS_MAXID + i] = c;
    points[(size_t)k * 2] = c.cy; points[(size_t)k * 2 + 1] = c.cx;
    area[k] = c.area;
}

// grid (ceil(HW / LT_CHUNK), B); dynamic LDS: the Gaussian table f32 [size][size], size = 6 sigma + 3.  PIX = 4: HW % 4 == 0 and 16-byte
// aligned planes, a lane per 16-byte word of each of the six planes; PIX = 1: a lane per element.
template <int PIX>
__global__ __launch_bounds__(LS_T) void lt_paint_kernel(const int* __restrict__ labels, const LtCentre* __restrict__ cen, const float* __restrict__ gauss,
                                                        int n, int H, int W, int sigma, float small_weight, int legacy_f32, float* __restrict__ out) {
    extern __shared__ float lt_g[];
    __shared__ int2 s_pk[LS_MAXID];
    const int t = threadIdx.x, b = blockIdx.y;
    const int size = 6 * sigma + 3, R = 3 * sigma + 1;
    for (int k = t; k < size * size; k += LS_T) lt_g[k] = gauss[k];
    const LtCentre* fc = cen + (size_t)b * LS_MAXID;
    for (int k = t; k < n; k += LS_T) s_pk[k] = make_int2(fc[k].px, fc[k].py);
    __syncthreads();
    const long HW = (long)H * W;
    const int* f = labels + (size_t)b * HW;
    float* o = out + (size_t)b * 6 * HW;
    for (int it = 0; it < LT_CHUNK / (LS_T * PIX); ++it) {
        const long p0 = (long)blockIdx.x * LT_CHUNK + ((long)it * LS_T + t) * PIX;
        if (p0 >= HW) break;                                 // (PIX = 4: HW % 4 == 0, so p0 + 3 < HW)
        float v[6][PIX];
#pragma unroll
        for (int q = 0; q < PIX; ++q) {
            const long p = p0 + q;
            const int y = (int)(p / W), x = (int)(p - (long)y * W);
            int id = f[p];
            if (id < 1 || id > n) id = 0;
            float heat = 0.f;
            for (int j = 0; j < n; ++j) {
                const int2 pk = s_pk[j];
                const int dx = x - pk.x + R, dy = y - pk.y + R;              // inside [x - 3 sigma - 1, x + 3 sigma + 2) x [y ...)
                if ((unsigned)dx < (unsigned)size && (unsigned)dy < (unsigned)size) heat = fmaxf(heat, lt_g[dy * size + dx]);
            }
            float oy = 0.f, ox = 0.f, fg = 0.f, wt = 1.f;
            if (id) {
                const LtCentre c = fc[id - 1];
                if (legacy_f32) { oy = (float)c.cy - (float)y; ox = (float)c.cx - (float)x; }      // numpy < 2: all float32
                else { oy = (float)(c.cy - (double)y); ox = (float)(c.cx - (double)x); }           // numpy >= 2: float64, rounded once
                fg = 1.f;
                if (c.small) wt = small_weight;
            }
            v[0][q] = heat; v[1][q] = oy; v[2][q] = ox; v[3][q] = fg; v[4][q] = wt; v[5][q] = fg;
        }
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            if (PIX == 4) *reinterpret_cast<float4*>(o + (size_t)c * HW + p0) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
            else o[(size_t)c * HW + p0] = v[c][0];
        }
    }
}

// ---- losses ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double ls_wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

struct LsArgs {
    const float* logits; const float* targets; const uint8_t* expl; int P; long HW; int nblk;
    int et, ncls, plane[2], kind[2];         // head 0 = eee_mask (explicit plane 0, region), 1 = eee_boundary (plane 1); plane < 0: absent
};

// the target stack of model.py:186-226 from the four explicit bytes (sums as written there)
__device__ __forceinline__ void ls_stack(bool tp, bool tn, bool fp, bool fn, int et, double (&t)[4]) {
    const double a = tp, b = tn, c = fp, d = fn;
    t[0] = t[1] = t[2] = t[3] = 0.0;
    if (et == 0) { t[0] = a; t[1] = b; t[2] = c; t[3] = d; }
    else if (et == 1) { t[0] = a + b; t[1] = c + d; }
    else if (et == 2) { t[0] = a + b; t[1] = c; t[2] = d; }
    else { t[0] = c; t[1] = d; }
}

// grid (nblk, B).  part f64 [B][nblk][LS_NACC]; fgp f64 [B][HW] or null
__global__ __launch_bounds__(LS_T) void ls_terms_kernel(LsArgs a, double* __restrict__ part, double* __restrict__ fgp) {
    __shared__ double s_red[LS_T / 64][LS_NACC];
    const int t = threadIdx.x, b = blockIdx.y;
    const long HW = a.HW;
    const float* L = a.logits + (size_t)b * a.P * HW;
    const float* T = a.targets + (size_t)b * 6 * HW;
    double acc[LS_NACC];
#pragma unroll
    for (int i = 0; i < LS_NACC; ++i) acc[i] = 0.0;
    for (int it = 0; it < LS_CHUNK / LS_T; ++it) {
        const long p = (long)blockIdx.x * LS_CHUNK + (long)it * LS_T + t;
        if (p >= HW) break;
        const double x0 = L[p], x1 = L[HW + p], x2 = L[2 * HW + p], x3 = L[3 * HW + p];
        const double tc = T[p], ty = T[HW + p], tx = T[2 * HW + p], ts = T[3 * HW + p], tw = T[4 * HW + p], iw = T[5 * HW + p];
        const double v = (fmax(x0, 0.0) - x0 * ts + log1p(exp(-fabs(x0)))) * tw;       // BCEWithLogits, stable form, times sem_seg_weights
        acc[0] += v;
        if (fgp) fgp[(size_t)b * HW + p] = v;
        const double d = x1 - tc;
        acc[1] += d * d * iw;
        acc[2] += iw;
        acc[3] += (fabs(x2 - ty) + fabs(x3 - tx)) * iw;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (a.plane[h] < 0) continue;
            const uint8_t* e = a.expl + ((size_t)b * 2 + a.kind[h]) * 4 * HW + p;
            double tg[4], z[4], ex[4];
            ls_stack(e[0] != 0, e[HW] != 0, e[2 * HW] != 0, e[3 * HW] != 0, a.et, tg);
            double m = -INFINITY;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                z[c] = c < a.ncls ? (double)L[(size_t)(a.plane[h] + c) * HW + p] : -INFINITY;
                m = fmax(m, z[c]);
            }
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < 4; ++c) { ex[c] = c < a.ncls ? exp(z[c] - m) : 0.0; s += ex[c]; }
            const double lse = m + log(s);
            const int o = 4 + 13 * h;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (c < a.ncls) {
                    acc[o] += tg[c] * (lse - z[c]);
                    acc[o + 1 + c] += tg[c] * (ex[c] / s);
                    acc[o + 5 + c] += tg[c];
                    acc[o + 9 + c] += ex[c] / s;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < LS_NACC; ++i) {
        const double v = ls_wave_sum(acc[i]);
        if ((t & 63) == 0) s_red[t >> 6][i] = v;
    }
    __syncthreads();
    if (t < LS_NACC) part[((size_t)b * a.nblk + blockIdx.x) * LS_NACC + t] = ((s_red[0][t] + s_red[1][t]) + s_red[2][t]) + s_red[3][t];
}

// select state of a frame: u64 [4] = (the bits of T found so far, k still to take inside them, values above them, 0)
// grid (B): clears the frame's histogram and starts its state
__global__ __launch_bounds__(LS_T) void ls_select_init_kernel(unsigned* __restrict__ hist, unsigned long long* __restrict__ state, unsigned long long k) {
    const int b = blockIdx.x;
    for (int i = threadIdx.x; i < LS_BINS; i += LS_T) hist[(size_t)b * LS_BINS + i] = 0;
    if (threadIdx.x < 4) state[b * 4 + threadIdx.x] = threadIdx.x == 1 ? k : 0ull;
}

// grid (nblk, B): the histogram of digit (bits >> shift) & mask over the values whose bits above the digit equal the state's.  Non-negative
// doubles order as their bit patterns.  The lanes of a wave that hold one digit add once (the early passes see one or two digits only).
__global__ __launch_bounds__(LS_T) void ls_hist_kernel(const double* __restrict__ fgp, long HW, int shift, int width,
                                                       const unsigned long long* __restrict__ state, unsigned* __restrict__ hist) {
    __shared__ unsigned s_h[LS_BINS];
    const int t = threadIdx.x, b = blockIdx.y, lane = t & 63;
    for (int i = t; i < LS_BINS; i += LS_T) s_h[i] = 0;
    __syncthreads();
    const int hi = shift + width;                            // 64 in the first pass: every value takes part
    const unsigned long long prefix = state[b * 4];
    const unsigned mask = (1u << width) - 1u;
    for (int it = 0; it < LS_CHUNK / LS_T; ++it) {
        const long p = (long)blockIdx.x * LS_CHUNK + (long)it * LS_T + t;        // (no early exit: the whole wave votes)
        bool active = false;
        unsigned digit = 0;
        if (p < HW) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(fgp[(size_t)b * HW + p]);
            active = hi >= 64 || (bits >> hi) == (prefix >> hi);
            digit = (unsigned)(bits >> shift) & mask;
        }
        unsigned long long m = __ballot(active);
        for (int r = 0; r < 64 && m; ++r) {
            const int leader = __ffsll((long long)m) - 1;
            const unsigned d0 = __shfl(digit, leader);
            const bool mine = active && digit == d0;
            const unsigned long long same = __ballot(mine);
            if (lane == leader) atomicAdd(&s_h[d0], (unsigned)__popcll(same));
            if (mine) active = false;
            m &= ~same;
        }
    }
    __syncthreads();
    for (int i = t; i < LS_BINS; i += LS_T)
        if (s_h[i]) atomicAdd(hist + (size_t)b * LS_BINS + i, s_h[i]);
}

// grid (B): the digit in which the k-th largest falls, from the top; the histogram is cleared for the next pass
__global__ __launch_bounds__(LS_T) void ls_pick_kernel(unsigned* __restrict__ hist, unsigned long long* __restrict__ state, int shift) {
    __shared__ unsigned s_h[LS_BINS], s_sum[LS_T];
    const int t = threadIdx.x, b = blockIdx.x;
    for (int i = t; i < LS_BINS; i += LS_T) { s_h[i] = hist[(size_t)b * LS_BINS + i]; hist[(size_t)b * LS_BINS + i] = 0; }
    __syncthreads();
    unsigned s = 0;
    for (int i = 0; i < LS_BINS / LS_T; ++i) s += s_h[t * (LS_BINS / LS_T) + i];
    s_sum[t] = s;
    __syncthreads();
    if (t == 0) {
        const unsigned long long krem = state[b * 4 + 1];
        unsigned long long cum = 0;
        int chunk = 0, digit = 0;
        for (int j = LS_T - 1; j >= 0; --j) {
            if (cum + s_sum[j] >= krem) { chunk = j; break; }
            cum += s_sum[j];
        }
        for (int i = LS_BINS / LS_T - 1; i >= 0; --i) {
            const int d = chunk * (LS_BINS / LS_T) + i;
            if (cum + s_h[d] >= krem) { digit = d; break; }
            cum += s_h[d];
        }
        state[b * 4] |= (unsigned long long)digit << shift;
        state[b * 4 + 1] = krem - cum;
        state[b * 4 + 2] += cum;
    }
}

// grid (nblk, B): the sum of the values above T, per block
__global__ __launch_bounds__(LS_T) void ls_above_kernel(const double* __restrict__ fgp, long HW, int nblk, const unsigned long long* __restrict__ state,
                                                        double* __restrict__ apart) {
    __shared__ double s_red[LS_T / 64];
    const int t = threadIdx.x, b = blockIdx.y;
    const unsigned long long T = state[b * 4];
    double acc = 0.0;
    for (int it = 0; it < LS_CHUNK / LS_T; ++it) {
        const long p = (long)blockIdx.x * LS_CHUNK + (long)it * LS_T + t;
        if (p >= HW) break;
        const double v = fgp[(size_t)b * HW + p];
        if ((unsigned long long)__double_as_longlong(v) > T) acc += v;
    }
    acc = ls_wave_sum(acc);
    if ((t & 63) == 0) s_red[t >> 6] = acc;
    __syncthreads();
    if (t == 0) apart[(size_t)b * nblk + blockIdx.x] = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}

struct LsFinish { double w_fg, w_c, w_o; unsigned long long k; int select, ncls, plane[2], loss[2]; long HW; int nblk; };

// grid (B), 64 lanes: the block partials added in block order, then the ratios -> out f64 [B][QUBER_LOSS_WORDS]
__global__ __launch_bounds__(64) void ls_finish_kernel(const double* __restrict__ part, const double* __restrict__ apart,
                                                       const unsigned long long* __restrict__ state, LsFinish f, double* __restrict__ out) {
    __shared__ double s_acc[LS_NACC + 1];
    const int t = threadIdx.x, b = blockIdx.x;
    if (t < LS_NACC) {
        double s = 0.0;
        for (int j = 0; j < f.nblk; ++j) s += part[((size_t)b * f.nblk + j) * LS_NACC + t];
        s_acc[t] = s;
    } else if (t == LS_NACC) {
        double s = 0.0;
        if (f.select)
            for (int j = 0; j < f.nblk; ++j) s += apart[(size_t)b * f.nblk + j];
        s_acc[t] = s;
    }
    __syncthreads();
    if (t != 0) return;
    double* o = out + (size_t)b * QUBER_LOSS_WORDS;
    double fg_sum = s_acc[0], kth = 0.0, above = 0.0;
    if (f.select) {
        kth = __longlong_as_double((long long)state[b * 4]);
        above = (double)state[b * 4 + 2];
        fg_sum = s_acc[LS_NACC] + (double)(f.k - state[b * 4 + 2]) * kth;      // the values tied at T are equal: any of them serves
    }
    const double wsum = s_acc[2];
    o[0] = f.w_fg * fg_sum / (double)f.k;
    o[1] = wsum > 0.0 ? f.w_c * s_acc[1] / wsum : 0.0;
    o[2] = wsum > 0.0 ? f.w_o * s_acc[3] / wsum : 0.0;          // the ONE-plane weight sum under both planes' numerator: model.py:796-798
    for (int h = 0; h < 2; ++h) {
        const int a = 4 + 13 * h;
        double v = 0.0;
        if (f.plane[h] >= 0) {
            if (f.loss[h] == 1) v = s_acc[a] / (double)f.HW;
            else {
                for (int c = 0; c < f.ncls; ++c) v += 1.0 - (2.0 * s_acc[a + 1 + c] + 1e-5) / ((s_acc[a + 5 + c] + s_acc[a + 9 + c]) + 1e-5);
                v /= (double)f.ncls;
            }
        }
        o[3 + h] = v;
        for (int i = 0; i < 13; ++i) o[13 + 13 * h + i] = f.plane[h] >= 0 ? s_acc[a + i] : 0.0;
    }
    o[5] = fg_sum; o[6] = (double)f.k; o[7] = kth; o[8] = above; o[9] = s_acc[1]; o[10] = wsum; o[11] = s_acc[3]; o[12] = (double)f.HW;
    o[39] = 0.0;
}

// ---- workspace, launchers ---------------------------------------------------------------------------------------------------------------
// layout for `cap_b` frames: mom | centres | partials | above partials | histograms | select states | foreground plane
struct LsWs { unsigned long long* mom; LtCentre* cen; double* part; double* apart; unsigned* hist; unsigned long long* state; double* fgp; };

static int ls_blocks(long HW) { return (int)((HW + LS_CHUNK - 1) / LS_CHUNK); }

static size_t ls_layout(LsWs* out, void* ws, int cap_b, int H, int W) {
    const long HW = (long)H * W;
    const size_t cb = (size_t)cap_b, nblk = (size_t)ls_blocks(HW);
    LsWs none, &r = out ? *out : none;
    WsWalk w{static_cast<char*>(ws)};
    r.mom = w.take<unsigned long long>(cb * LS_MAXID * 3);
    r.cen = w.take<LtCentre>(cb * LS_MAXID);
    r.part = w.take<double>(cb * nblk * LS_NACC);
    r.apart = w.take<double>(cb * nblk);
    r.hist = w.take<unsigned>(cb * LS_BINS);
    r.state = w.take<unsigned long long>(cb * 4);
    r.fgp = w.take<double>(cb * HW);
    return w.off;
}

size_t losses_ws_bytes(int cap_b, int H, int W) { return ls_layout(nullptr, nullptr, cap_b, H, W); }

// ws: losses_ws_bytes(cap_b >= B, H, W) bytes.  1 <= sigma <= 20 (the table and the peaks fit the 64 KB of LDS a launch gets without asking), n <= 254
int launch_loss_targets(const int* labels, int B, int n, int H, int W, int sigma, int small_area, float small_weight, int legacy_f32,
                        const float* gauss, float* targets, double* points, int* area, void* ws, int cap_b, hipStream_t st) {
    if (B <= 0) return 0;
    LsWs w;
    ls_layout(&w, ws, cap_b, H, W);
    const long HW = (long)H * W;
    ProfScope prof("loss_targets", 28.0 * B * HW, 0.0, st);                       // the label map in, six f32 planes out
    if (n > 0) {
        if (launch_zero(w.mom, (size_t)B * n * 24, st)) return -1;
        hipLaunchKernelGGL(lt_moment_kernel, dim3((unsigned)((HW + LS_T - 1) / LS_T), B), dim3(LS_T), 0, st, labels, n, H, W, w.mom);
        hipLaunchKernelGGL(lt_centre_kernel, dim3((B * n + LS_T - 1) / LS_T), dim3(LS_T), 0, st, w.mom, B * n, n, small_area, w.cen, points, area);
        QB_CHECK(hipGetLastError());
    }
    const size_t lds = (size_t)(6 * sigma + 3) * (6 * sigma + 3) * sizeof(float);
    const dim3 grid((unsigned)((HW + LT_CHUNK - 1) / LT_CHUNK), B);
    if (HW % 4 == 0 && ((uintptr_t)targets & 15) == 0)
        hipLaunchKernelGGL(lt_paint_kernel<4>, grid, dim3(LS_T), lds, st, labels, w.cen, gauss, n, H, W, sigma, small_weight, legacy_f32, targets);
    else
        hipLaunchKernelGGL(lt_paint_kernel<1>, grid, dim3(LS_T), lds, st, labels, w.cen, gauss, n, H, W, sigma, small_weight, legacy_f32, targets);
    QB_CHECK(hipGetLastError());
    return 0;
}

// k: pixels the foreground term averages over (H * W for top_k == 1.0: no selection)
int launch_losses(const float* logits, int P, const float* targets, const uint8_t* expl, const ::quber_loss_spec& sp, int ncls, long k, int B, int H,
                  int W, double* out, void* ws, int cap_b, hipStream_t st) {
    if (B <= 0) return 0;
    LsWs w;
    ls_layout(&w, ws, cap_b, H, W);
    const long HW = (long)H * W;
    const int nblk = ls_blocks(HW);
    const bool select = sp.top_k != 1.0;
    const int heads = (sp.eee_mask_plane >= 0) + (sp.eee_boundary_plane >= 0);
    ProfScope prof("losses", (double)B * HW * (4.0 * (4 + 6 + heads * ncls) + 4.0 * heads + (select ? 8.0 : 0.0)), 0.0, st);
    LsArgs a;
    a.logits = logits; a.targets = targets; a.expl = expl; a.P = P; a.HW = HW; a.nblk = nblk; a.et = sp.error_type; a.ncls = ncls;
    a.plane[0] = sp.eee_mask_plane; a.plane[1] = sp.eee_boundary_plane; a.kind[0] = 0; a.kind[1] = 1;
    const dim3 grid(nblk, B);
    hipLaunchKernelGGL(ls_terms_kernel, grid, dim3(LS_T), 0, st, a, w.part, select ? w.fgp : nullptr);
    QB_CHECK(hipGetLastError());
    if (select) {
        static const int shifts[LS_PASSES] = {53, 42, 31, 20, 9, 0}, widths[LS_PASSES] = {11, 11, 11, 11, 11, 9};
        hipLaunchKernelGGL(ls_select_init_kernel, dim3(B), dim3(LS_T), 0, st, w.hist, w.state, (unsigned long long)k);
        for (int p = 0; p < LS_PASSES; ++p) {
            hipLaunchKernelGGL(ls_hist_kernel, grid, dim3(LS_T), 0, st, w.fgp, HW, shifts[p], widths[p], w.state, w.hist);
            hipLaunchKernelGGL(ls_pick_kernel, dim3(B), dim3(LS_T), 0, st, w.hist, w.state, shifts[p]);
        }
        hipLaunchKernelGGL(ls_above_kernel, grid, dim3(LS_T), 0, st, w.fgp, HW, nblk, w.state, w.apart);
        QB_CHECK(hipGetLastError());
    }
    LsFinish f;
    f.w_fg = sp.foreground_weight; f.w_c = sp.center_weight; f.w_o = sp.offset_weight; f.k = (unsigned long long)k;
    f.select = select ? 1 : 0; f.ncls = ncls; f.plane[0] = sp.eee_mask_plane; f.plane[1] = sp.eee_boundary_plane;
    f.loss[0] = sp.eee_mask_loss; f.loss[1] = sp.eee_boundary_loss; f.HW = HW; f.nblk = nblk;
    hipLaunchKernelGGL(ls_finish_kernel, dim3(B), dim3(64), 0, st, w.part, w.apart, w.state, f, out);
    QB_CHECK(hipGetLastError());
    return 0;
}

}  // namespace quber
