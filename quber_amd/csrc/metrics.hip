// Evaluation support: the pairwise overlap counts behind eval/evaluation.py:57-274
// `multilabel_metrics`.  The reference loops over every (gt label, predicted label) pair and counts
// |gt_i & pred_j| with one full-frame pass each (evaluation.py:180-199); here ONE pass over the two label maps
// fills the whole contingency table, from which the host derives tp / P / R / F / IoU / union for all pairs.
//   1. presence:  which label values (0..65535) occur in each map
//   2. rank:      sorted unique labels (np.unique order) + value -> dense index LUT   (one block)
//   3. count:     table[gt index][pred index] += 1, LDS-privatised when the table fits
#include "common.h"
#include "evalbody.h"   // the kernel bodies, shared with the batched launches of evalbatch.hip

namespace quber {

__global__ void label_presence_kernel(const int* __restrict__ pred, const int* __restrict__ gt, long n,
                                      unsigned* __restrict__ flags /*[2][LAB_MAX]*/, int* __restrict__ bad) {
    label_presence_body(pred, gt, n, flags, bad);
}

// one block of 1024 threads per map (blockIdx.x = 0 pred, 1 gt): ordered compaction of the set flags
__global__ __launch_bounds__(1024) void label_rank_kernel(const unsigned* __restrict__ flags, int cap,
                                                          unsigned short* __restrict__ lut /*[2][LAB_MAX]*/,
                                                          int* __restrict__ labels /*[2][cap]*/, int* __restrict__ counts) {
    label_rank_body(flags, cap, blockIdx.x, lut, labels, counts);
}

__global__ __launch_bounds__(256) void contingency_kernel(const int* __restrict__ pred, const int* __restrict__ gt, long n,
                                                          const unsigned short* __restrict__ lut,
                                                          const int* __restrict__ counts, int cap,
                                                          unsigned long long* __restrict__ table /*[cap][cap]*/) {
    contingency_body(pred, gt, n, lut, counts, cap, table);
}

size_t contingency_ws_bytes(int cap) {
    return sizeof(unsigned) * 2 * LAB_MAX + sizeof(unsigned short) * 2 * LAB_MAX + sizeof(int) * (2 * cap + 4) +
           sizeof(unsigned long long) * (size_t)cap * cap;
}

// ws layout: flags u32[2][LAB_MAX] | table u64[cap][cap] | labels i32[2][cap] | counts i32[2] bad i32 pad | lut u16[2][LAB_MAX]
int launch_contingency(const int* pred, const int* gt, long n, int cap, void* ws, hipStream_t st) {
    char* w = reinterpret_cast<char*>(ws);
    unsigned* flags = reinterpret_cast<unsigned*>(w); w += sizeof(unsigned) * 2 * LAB_MAX;
    unsigned long long* table = reinterpret_cast<unsigned long long*>(w); w += sizeof(unsigned long long) * (size_t)cap * cap;
    int* labels = reinterpret_cast<int*>(w); w += sizeof(int) * 2 * cap;
    int* counts = reinterpret_cast<int*>(w); w += sizeof(int) * 4;
    unsigned short* lut = reinterpret_cast<unsigned short*>(w);
    if (int rc = launch_zero(ws, contingency_ws_bytes(cap), st)) return rc;
    int blocks = (int)((n + 255) / 256);
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(label_presence_kernel, dim3(blocks), dim3(256), 0, st, pred, gt, n, flags, counts + 2);
    hipLaunchKernelGGL(label_rank_kernel, dim3(2), dim3(1024), 0, st, flags, cap, lut, labels, counts);
    hipLaunchKernelGGL(contingency_kernel, dim3(blocks), dim3(256), sizeof(unsigned) * 4096, st, pred, gt, n, lut, counts, cap,
                       table);
    QB_CHECK(hipGetLastError());
    return 0;
}

}  // namespace quber
