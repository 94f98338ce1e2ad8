// The boundary of a mask for Boundary AP (include/quber_hip.h: quber_coco_match_boundary, quber_op_mask_boundary; the definition is in
// DESIGN.md "Boundary AP" and, as numpy, in tests/test_boundary_ap_cpu.py: mask_boundary_np): boundary(m) = m & ~erode_d(m), erode_d = d
// iterations of a 3 x 3 erosion with zeros outside the frame = a pixel survives iff the whole (2d + 1) x (2d + 1) square around it lies
// inside the frame and inside m.  Restates mask_to_boundary of the published boundary-iou-api on the bit planes of bitplane.h.
//
//   boundary  a workgroup owns CB_BAND rows x CB_COLS words of one plane.
//             horizontal: for its rows and the d rows above and below, the run-AND of width 2d + 1 over the bits of every word, by
//               shift-and-fold doubling on the 96-bit windows (word j .. j + 2: the d pixels to the right; word j - 2 .. j: to the left;
//               d <= 64 = two words on each side).  Word -1 and the words behind the row read 0 and the bits behind W are 0 in a plane: the
//               zero border left and right.  The result goes to LDS; a row outside the frame is stored as zeros: the border above and below.
//             vertical: the AND over the rows y - d .. y + d of that result, out = m & ~that, popc per lane, one wave reduction, one
//               integer atomicAdd per (wave, plane).
//             One barrier, reached by every lane; the loop bounds depend on d and the frame only.  No floating point.
//   pack / unpack  (the stand-alone op) u8 masks -> planes, planes -> 0 / 1 bytes.
#include "bitplane.h"       // mn_plane_words, mn_pack_word
#include "common.h"

namespace quber {

constexpr int CB_BAND = 64;                  // rows of a plane per workgroup
constexpr int CB_COLS = 32;                  // words of a row per workgroup
constexpr int CB_MAX_D = 64;                 // dilation: the windows above reach two words to each side
static_assert(32 * 2 >= CB_MAX_D, "a 96-bit window holds the d pixels to one side of every bit of its word");

// bits [0, 96) as lo (64) | hi (32, in a 64-bit register); s in 0..63; zeros come in
__device__ __forceinline__ void cb_shr(unsigned long long& lo, unsigned long long& hi, int s) {
    if (s) lo = (lo >> s) | (hi << (64 - s));
    hi >>= s;
}
__device__ __forceinline__ void cb_shl(unsigned long long& lo, unsigned long long& hi, int s) {
    if (s) hi = ((hi << s) | (lo >> (64 - s))) & 0xffffffffull;
    lo <<= s;
}

// bit p of the result = AND of the bits p .. p + n - 1 of (w0 | w1 << 32 | w2 << 64), p in 0..31, n in 1..65.  A(k)(x) = AND of k bits
// from x: A(2k)(x) = A(k)(x) & A(k)(x + k), at last A(n)(x) = A(k)(x) & A(k)(x + n - k) with n - k < k.  The zeros a shift brings in reach
// only positions whose run leaves the window, and no bit of the result is built from those.
__device__ __forceinline__ unsigned cb_run_up(unsigned w0, unsigned w1, unsigned w2, int n) {
    unsigned long long lo = w0 | (unsigned long long)w1 << 32, hi = w2;
    int k = 1;
    for (; 2 * k <= n; k *= 2) {
        unsigned long long l = lo, h = hi;
        cb_shr(l, h, k);
        lo &= l; hi &= h;
    }
    unsigned long long l = lo, h = hi;
    cb_shr(l, h, n - k);
    return (unsigned)(lo & l);
}
// bit p of the result = AND of the bits 64 + p - n + 1 .. 64 + p of the same window (w2 is the word of the result)
__device__ __forceinline__ unsigned cb_run_down(unsigned w0, unsigned w1, unsigned w2, int n) {
    unsigned long long lo = w0 | (unsigned long long)w1 << 32, hi = w2;
    int k = 1;
    for (; 2 * k <= n; k *= 2) {
        unsigned long long l = lo, h = hi;
        cb_shl(l, h, k);
        lo &= l; hi &= h;
    }
    unsigned long long l = lo, h = hi;
    cb_shl(l, h, n - k);
    return (unsigned)(hi & h);
}

// grid (planes, ceil(H / CB_BAND), ceil(wpr / CB_COLS)), 256 lanes.  planes, out u32 [planes][pw]; area + plane * area_stride: += the
// pixels of the boundary (zero on entry).  Every word of `out` below H * wpr is written; the padding words behind are written as zero.
__global__ __launch_bounds__(256) void ca_boundary_kernel(const unsigned* __restrict__ planes, int H, int wpr, int pw, int d,
                                                          unsigned* __restrict__ out, unsigned* __restrict__ area, int area_stride) {
    __shared__ unsigned s_h[(CB_BAND + 2 * CB_MAX_D) * CB_COLS];
    const int t = threadIdx.x;
    const size_t m = blockIdx.x;
    const int y0 = blockIdx.y * CB_BAND, y1 = min(y0 + CB_BAND, H);
    const int j0 = blockIdx.z * CB_COLS, tw = min(CB_COLS, wpr - j0);
    const unsigned* src = planes + m * pw;
    unsigned* dst = out + m * pw;
    const int rows = y1 - y0 + 2 * d;                        // <= CB_BAND + 2 CB_MAX_D
    for (int i = t; i < rows * tw; i += 256) {
        const int r = i / tw, c = i - r * tw, y = y0 - d + r, j = j0 + c;
        unsigned h = 0;
        if (y >= 0 && y < H) {
            const unsigned* row = src + (size_t)y * wpr;
            const unsigned a0 = j >= 2 ? row[j - 2] : 0u, a1 = j >= 1 ? row[j - 1] : 0u, a2 = row[j];
            const unsigned a3 = j + 1 < wpr ? row[j + 1] : 0u, a4 = j + 2 < wpr ? row[j + 2] : 0u;
            h = cb_run_up(a2, a3, a4, d + 1) & cb_run_down(a0, a1, a2, d + 1);
        }
        s_h[r * CB_COLS + c] = h;
    }
    __syncthreads();
    int cnt = 0;
    for (int i = t; i < (y1 - y0) * tw; i += 256) {
        const int r = i / tw, c = i - r * tw;
        unsigned v = 0xffffffffu;
        for (int k = 0; k <= 2 * d; ++k) v &= s_h[(r + k) * CB_COLS + c];
        const size_t o = (size_t)(y0 + r) * wpr + j0 + c;
        const unsigned b = src[o] & ~v;
        dst[o] = b;
        cnt += __popc(b);
    }
    if (blockIdx.y == 0 && blockIdx.z == 0)                  // the padding of the plane (at most 3 words)
        for (int i = H * wpr + t; i < pw; i += 256) dst[i] = 0u;
    for (int off = 32; off; off >>= 1) cnt += __shfl_xor(cnt, off);
    if ((t & 63) == 0 && cnt) atomicAdd(area + m * area_stride, (unsigned)cnt);
}

int mask_boundary_max_dilation() { return CB_MAX_D; }
int mask_boundary_band() { return CB_BAND; }

int launch_boundary_planes(const unsigned* planes, long n_planes, int H, int W, int d, unsigned* out, unsigned* area, int area_stride,
                           hipStream_t st) {
    if (d < 1 || d > CB_MAX_D) return fail("mask boundary: dilation outside 1..64");
    if (n_planes <= 0) return 0;
    if (n_planes > 0x7fffffffL) return fail("mask boundary: more than 2^31 - 1 planes");
    const int wpr = (W + 31) / 32, pw = (int)mn_plane_words(H, W);
    const dim3 grid((unsigned)n_planes, (H + CB_BAND - 1) / CB_BAND, (wpr + CB_COLS - 1) / CB_COLS);
    if (grid.y > 65535 || grid.z > 65535) return fail("mask boundary: a frame of more than 65535 bands of rows or columns");
    ProfScope prof("mask_boundary", 8.0 * n_planes * pw, 0.0, st);
    hipLaunchKernelGGL(ca_boundary_kernel, grid, dim3(256), 0, st, planes, H, wpr, pw, d, out, area, area_stride);
    QB_CHECK(hipGetLastError());
    return 0;
}

// ---- the stand-alone op: u8 masks -> planes -> boundary planes -> 0 / 1 bytes ----
// grid (n, ceil(pw / 256)).  area i32 [n][2], zero on entry: [m][0] += the pixels of mask m
template <bool ALIGNED>
__global__ __launch_bounds__(256) void cb_pack_kernel(const uint8_t* __restrict__ masks, int H, int W, int wpr, int pw, unsigned* __restrict__ planes,
                                                      unsigned* __restrict__ area) {
    const int i = blockIdx.y * 256 + threadIdx.x;
    const size_t m = blockIdx.x;
    const unsigned bits = i < H * wpr ? mn_pack_word<ALIGNED>(masks + m * (size_t)H * W, i, W, wpr) : 0u;
    if (i < pw) planes[m * pw + i] = bits;
    int c = __popc(bits);                                    // (every lane of the block gets here)
    for (int off = 32; off; off >>= 1) c += __shfl_xor(c, off);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(area + m * 2, (unsigned)c);
}

// grid (n, ceil(H * wpr / 256)): one word per lane -> up to 32 bytes of 0 / 1
__global__ __launch_bounds__(256) void cb_unpack_kernel(const unsigned* __restrict__ planes, int H, int W, int wpr, int pw, uint8_t* __restrict__ out) {
    const int i = blockIdx.y * 256 + threadIdx.x;
    const size_t m = blockIdx.x;
    if (i >= H * wpr) return;
    const int y = i / wpr, x0 = (i - y * wpr) * 32, nb = min(32, W - x0);
    const unsigned bits = planes[m * pw + i];
    uint8_t* p = out + m * (size_t)H * W + (size_t)y * W + x0;
    for (int k = 0; k < nb; ++k) p[k] = (bits >> k) & 1u;
}

size_t mask_boundary_ws_bytes(long n, int H, int W) { return ws_align((size_t)n * mn_plane_words(H, W) * 4) * 2; }

int launch_mask_boundary(const uint8_t* masks, long n, int H, int W, int d, uint8_t* out, int* area, void* ws, hipStream_t st) {
    if (H < 1 || W < 1 || (long)H * W > (1L << 30)) return fail("mask boundary: an empty frame or one of more than 2^30 pixels");
    if (n < 0 || n > 0x7fffffffL) return fail("mask boundary: n outside 0..2^31 - 1");
    if (d < 1 || d > CB_MAX_D) return fail("mask boundary: dilation outside 1..64");
    if (n == 0) return 0;
    if (!masks || !out || !area || !ws) return fail("mask boundary: null tensor");
    if ((uintptr_t)area & 3) return fail("mask boundary: dev_area is not 4-byte aligned");
    const int wpr = (W + 31) / 32, pw = (int)mn_plane_words(H, W);
    unsigned* planes = static_cast<unsigned*>(ws);
    unsigned* bplanes = reinterpret_cast<unsigned*>(static_cast<char*>(ws) + ws_align((size_t)n * pw * 4));
    unsigned* ar = reinterpret_cast<unsigned*>(area);
    if ((pw + 255) / 256 > 65535) return fail("mask boundary: a frame of more than 65535 x 256 plane words");
    if (launch_zero(ar, (size_t)n * 8, st)) return -1;
    {
        ProfScope prof("mask_boundary_pack", (double)n * H * W + 4.0 * n * pw, 0.0, st);
        const dim3 grid((unsigned)n, (pw + 255) / 256);
        if (W % 16 == 0 && ((uintptr_t)masks & 15) == 0)
            hipLaunchKernelGGL(cb_pack_kernel<true>, grid, dim3(256), 0, st, masks, H, W, wpr, pw, planes, ar);
        else
            hipLaunchKernelGGL(cb_pack_kernel<false>, grid, dim3(256), 0, st, masks, H, W, wpr, pw, planes, ar);
        QB_CHECK(hipGetLastError());
    }
    if (launch_boundary_planes(planes, n, H, W, d, bplanes, ar + 1, 2, st)) return -1;
    {
        ProfScope prof("mask_boundary_unpack", (double)n * H * W + 4.0 * n * pw, 0.0, st);
        hipLaunchKernelGGL(cb_unpack_kernel, dim3((unsigned)n, (H * wpr + 255) / 256), dim3(256), 0, st, bplanes, H, W, wpr, pw, out);
        QB_CHECK(hipGetLastError());
    }
    return 0;
}

}  // namespace quber
