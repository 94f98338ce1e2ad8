// Device helpers that the zoom-in entries (zoom.hip) and the Region Refinement Network's crop / paste (rrn.hip) share: the legacy
// nearest-neighbour index, and what a slot (frame, id) of a crop list means.
#pragma once
#include "common.h"

namespace quber {

constexpr int ZM_MAXID = 254;                // ids of a compact map; crops per frame
constexpr int ZM_T = 256;

// F.interpolate(mode="nearest"): the source index of destination index `dst` for a resize from `in` to `out` samples
__device__ __forceinline__ int zm_near(int dst, int in, int out) {
    const float scale = __fdiv_rn((float)in, (float)out);
    return min((int)floorf(__fmul_rn((float)dst, scale)), in - 1);
}

struct ZmSlot { int b, id, x0, y0, w, h; bool ok; };

// slot t -> its frame, first-pass id and ROI; ok = 0 for a slot that is no crop (frame or id out of range, a ROI that is empty or leaves
// the frame)
__device__ __forceinline__ ZmSlot zm_slot(const int* __restrict__ slots, const int* __restrict__ rois, int t, int B, int n_ids, int H, int W) {
    ZmSlot s;
    s.b = slots[2 * t];
    s.id = slots[2 * t + 1];
    s.x0 = s.y0 = 0; s.w = s.h = 0;
    s.ok = s.b >= 0 && s.b < B && s.id >= 1 && s.id <= n_ids;
    if (s.ok) {
        const int* r = rois + ((size_t)s.b * n_ids + s.id - 1) * 4;
        s.x0 = r[0]; s.y0 = r[1]; s.w = r[2] - r[0] + 1; s.h = r[3] - r[1] + 1;
        s.ok = s.x0 >= 0 && s.y0 >= 0 && s.w >= 1 && s.h >= 1 && r[2] < W && r[3] < H;
    }
    return s;
}

}  // namespace quber
