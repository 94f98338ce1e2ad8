// Transform arithmetic shared by the Winograd kernels (winograd.hip: the three-kernel pipeline; wino_fused.hip: the
// single-kernel F(4x4,3x3) layer): B^T / A^T in one dimension, the tile index map.
#pragma once
#include "common.h"

namespace quber {
namespace wxf {

// V consecutive channels of one pixel (V = 4: 16-byte accesses; V = 2 for the 8x8 transforms of m = 6, whose 64
// intermediate values per channel would not fit the register file four channels at a time)
template <int V>
struct Vec {
    float v[V];
    __device__ inline Vec operator+(const Vec& o) const { Vec r; for (int e = 0; e < V; ++e) r.v[e] = v[e] + o.v[e]; return r; }
    __device__ inline Vec operator-(const Vec& o) const { Vec r; for (int e = 0; e < V; ++e) r.v[e] = v[e] - o.v[e]; return r; }
};
template <int V>
__device__ inline Vec<V> operator*(float s, const Vec<V>& a) { Vec<V> r; for (int e = 0; e < V; ++e) r.v[e] = s * a.v[e]; return r; }
template <int V>
__device__ inline Vec<V> vzero() { Vec<V> r; for (int e = 0; e < V; ++e) r.v[e] = 0.f; return r; }
template <int V>
__device__ inline Vec<V> vload(const float* p) {
    Vec<V> r;
    if constexpr (V == 4) { const float4 t = *reinterpret_cast<const float4*>(p); r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w; }
    else { const float2 t = *reinterpret_cast<const float2*>(p); r.v[0] = t.x; r.v[1] = t.y; }
    return r;
}
template <int V>
__device__ inline void vstore(float* p, const Vec<V>& a) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(a.v[0], a.v[1], a.v[2], a.v[3]);
    else *reinterpret_cast<float2*>(p) = make_float2(a.v[0], a.v[1]);
}

// y = B^T x  (one dimension)
template <int O, class T>
__device__ inline void bt(const T* x, T* y) {
    if constexpr (O == 2) {
        y[0] = x[0] - x[2];
        y[1] = x[1] + x[2];
        y[2] = x[2] - x[1];
        y[3] = x[1] - x[3];
    } else if constexpr (O == 4) {
        // points 0, +-3/4, +-3/2, inf (all constants dyadic, hence exact in fp32)
        const T e1 = x[4] - 2.25f * x[2], o1 = 0.75f * x[3] - 1.6875f * x[1];
        const T e2 = x[4] - 0.5625f * x[2], o2 = 1.5f * x[3] - 0.84375f * x[1];
        y[0] = (1.265625f * x[0] - 2.8125f * x[2]) + x[4];
        y[1] = e1 + o1;
        y[2] = e1 - o1;
        y[3] = e2 + o2;
        y[4] = e2 - o2;
        y[5] = (1.265625f * x[1] - 2.8125f * x[3]) + x[5];
    } else {
        // points 0, +-1, +-2, +-1/2, inf (Lavin & Gray / wincnn)
        const T a = (x[2] + x[6]) - 4.25f * x[4], b = (x[1] + x[5]) - 4.25f * x[3];
        const T c = (0.25f * x[2] - 1.25f * x[4]) + x[6], d = (0.5f * x[1] - 2.5f * x[3]) + 2.f * x[5];
        const T e = (4.f * x[2] - 5.f * x[4]) + x[6], f = (2.f * x[1] - 2.5f * x[3]) + 0.5f * x[5];
        y[0] = (x[0] - x[6]) + 5.25f * (x[4] - x[2]);
        y[1] = a + b;
        y[2] = a - b;
        y[3] = c + d;
        y[4] = c - d;
        y[5] = e + f;
        y[6] = e - f;
        y[7] = (x[7] - x[1]) + 5.25f * (x[3] - x[5]);
    }
}

// y = A^T x  (one dimension)
template <int O, class T>
__device__ inline void at(const T* x, T* y) {
    if constexpr (O == 2) {
        y[0] = (x[0] + x[1]) + x[2];
        y[1] = (x[1] - x[2]) - x[3];
    } else if constexpr (O == 4) {
        const T a = x[1] + x[2], b = x[1] - x[2], c = x[3] + x[4], d = x[3] - x[4];
        y[0] = (x[0] + a) + c;
        y[1] = 0.75f * b + 1.5f * d;
        y[2] = 0.5625f * a + 2.25f * c;
        y[3] = (0.421875f * b + 3.375f * d) + x[5];
    } else {
        const T s1 = x[1] + x[2], d1 = x[1] - x[2], s2 = x[3] + x[4], d2 = x[3] - x[4], s3 = x[5] + x[6], d3 = x[5] - x[6];
        y[0] = ((x[0] + s1) + s2) + s3;
        y[1] = (d1 + 2.f * d2) + 0.5f * d3;
        y[2] = (s1 + 4.f * s2) + 0.25f * s3;
        y[3] = (d1 + 8.f * d2) + 0.125f * d3;
        y[4] = (s1 + 16.f * s2) + 0.0625f * s3;
        y[5] = ((d1 + 32.f * d2) + 0.03125f * d3) + x[7];
    }
}

// tile index -> image, phase and tile position
struct TileAt { int b, py, px, ty, tx; };
__device__ inline TileAt locate(long tile, int TH, int TW, int d) {
    TileAt t;
    t.tx = tile % TW;
    long r = tile / TW;
    t.ty = r % TH;
    r /= TH;
    t.px = r % d;
    r /= d;
    t.py = r % d;
    t.b = (int)(r / d);
    return t;
}


// the same on 32-bit indices (the single-kernel form checks tiles < 2^31: 64-bit divisions cost its prologue ~100 instructions)
__device__ inline TileAt locate32(unsigned tile, unsigned TH, unsigned TW, unsigned d) {
    TileAt t;
    unsigned r = tile / TW;
    t.tx = (int)(tile - r * TW);
    unsigned r2 = r / TH;
    t.ty = (int)(r - r2 * TH);
    unsigned r3 = r2 / d;
    t.px = (int)(r2 - r3 * d);
    const unsigned r4 = r3 / d;
    t.py = (int)(r3 - r4 * d);
    t.b = (int)r4;
    return t;
}

// tiles per image: d*d phases of ceil(ceil(H/d)/m) x ceil(ceil(W/d)/m) tiles
inline int tiles_1d(int n, int d, int m) { return ((n + d - 1) / d + m - 1) / m; }
inline long wino_tiles(int H, int W, int d, int m) { return (long)d * d * tiles_1d(H, d, m) * tiles_1d(W, d, m); }

// ---- the tile map of one axis (three-kernel pipeline; host and device) ----
// With dilation d (= padding) an axis of n pixels is d phases, phase p = the pixels d*r + p, r < n_p = ceil((n - p) / d); in
// phase coordinates the layer is a dense 3-tap convolution with zero padding 1.  Two tilings of the axis into tiles of m slots:
//   per phase: every phase gets ceil(ceil(n/d)/m) tiles of its own, d * that in all (what wino_fused.hip keeps);
//   packed:    the non-empty phases one after the other with ONE zero slot between neighbours - the slot both read as their
//              padding - tiled as if they were one image: L = n + (non-empty phases - 1) slots, ceil(L / m) tiles.
// An axis is packed iff that needs fewer tiles (rows and columns decide independently; d = 1 never is).
// A tile reads the slots m*t - 1 .. m*t + m and owns m*t .. m*t + m - 1; a slot is a pixel or zero (separator, slot -1, slots
// >= L / past the phase's end): a zero slot's output is computed and dropped.
struct Axis {
    int n, d, m;
    int packed;      // 1: the packed tiling
    int T;           // tiles of the axis
    int Tp;          // per phase: tiles of one phase
    int q, rem;      // n / d, n % d: phases < rem have q + 1 pixels, the others q
};
__host__ __device__ inline int axis_tiles_phase(int n, int d, int m) { return d * (((n + d - 1) / d + m - 1) / m); }
__host__ __device__ inline int axis_tiles_packed(int n, int d, int m) { return (n + (d < n ? d : n) - 1 + m - 1) / m; }
__host__ __device__ inline Axis make_axis(int n, int d, int m, bool pack) {
    Axis a;
    a.n = n; a.d = d; a.m = m;
    a.Tp = ((n + d - 1) / d + m - 1) / m;
    const int tph = d * a.Tp, tpk = axis_tiles_packed(n, d, m);
    a.packed = pack && tpk < tph;
    a.T = a.packed ? tpk : tph;
    a.q = n / d; a.rem = n % d;
    return a;
}
// a slot of the axis: element r of phase p (r == -1: the zero slot in front of the phase)
struct AxisPos { int p, r; };
// slot m*t - 1, the first one tile t reads
__host__ __device__ inline AxisPos axis_begin(const Axis& a, int t) {
    AxisPos s;
    if (!a.packed) {
        s.p = t / a.Tp;
        s.r = a.m * (t - s.p * a.Tp) - 1;
        return s;
    }
    // with a zero slot in front of phase 0 as well, slot m*t - 1 has index e = m*t >= 0 in a sequence of segments
    // [zero, the phase's pixels]: rem segments of q + 2 slots, then segments of q + 1
    const int e = a.m * t, head = a.rem * (a.q + 2);
    const bool lng = e < head;
    const int seg = lng ? a.q + 2 : a.q + 1, e2 = lng ? e : e - head, k = e2 / seg;
    s.p = (lng ? 0 : a.rem) + k;
    s.r = e2 - k * seg - 1;
    return s;
}
// the next slot
__host__ __device__ inline AxisPos axis_next(const Axis& a, AxisPos s) {
    ++s.r;
    if (a.packed && s.r == a.q + (s.p < a.rem ? 1 : 0)) { ++s.p; s.r = -1; }
    return s;
}
// the pixel coordinate of a slot, or -1: it reads zero and stores nothing
__host__ __device__ inline int axis_coord(const Axis& a, AxisPos s) {
    const int c = a.d * s.r + s.p;
    return (s.r >= 0 && s.p < a.d && c < a.n) ? c : -1;
}
// tiles per image of the pipeline: each axis packed where that needs fewer tiles (pack == false: wino_tiles)
inline long wino_tiles_run(int H, int W, int d, int m, bool pack) {
    return (long)make_axis(H, d, m, pack).T * make_axis(W, d, m, pack).T;
}

}  // namespace wxf
}  // namespace quber
