// Process-wide runtime state of libquber_hip.so: the option table, the device-CU cache, the error string and the stage profiler.
#include <atomic>

#include "plan.h"

namespace quber {

Tuning g_tune;
thread_local const Tuning* t_tune = nullptr;

// The option keys of quber_set_option / quber_get_option / quber_set_tuning (include/quber_hip.h), in key order: THE key -> field relation.
// plan = the key shapes the plan: it acts when quber_finalize_weights builds it and is refused afterwards (31 and 38 are read at launch too and stay settable).
// Keys 2, 11, 12, 26 belong to the stand-alone ops (api_ops.hip: op_set_tuning); 33 and 34 are retired.
struct TuneKey { int key; int Tuning::*field; bool plan; };
constexpr TuneKey TUNE_KEYS[] = {
    {3, &Tuning::force_split, false},           {4, &Tuning::force_tile, false},
    {5, &Tuning::tail_split, false},            {6, &Tuning::winograd, true},
    {7, &Tuning::wino_min_cin, true},           {8, &Tuning::wino_max_ratio, true},
    {9, &Tuning::wino_variant, true},           {10, &Tuning::wino_min_cout, true},
    {13, &Tuning::persist, false},              {14, &Tuning::persist_min_nk, false},
    {15, &Tuning::persist_min_tiles, false},    {16, &Tuning::persist_debug, false},
    {17, &Tuning::wino_pairs, false},           {18, &Tuning::fuse_shortcut, true},
    {19, &Tuning::tile_128x64, false},          {20, &Tuning::wino_chunk_mb, false},
    {21, &Tuning::acc_chunk, false},            {24, &Tuning::lanes, false},
    {25, &Tuning::wino_fused, true},            {27, &Tuning::wino_fused_max_cin, true},
    {29, &Tuning::stem_fused, true},            {30, &Tuning::lean_loader, false},
    {31, &Tuning::h8, false},                   {32, &Tuning::h8_min_tiles, false},
    {35, &Tuning::x8, false},                   {36, &Tuning::x8_min_rounds, false},
    {37, &Tuning::x8_min_nk, false},            {38, &Tuning::h8_narrow, false},
    {39, &Tuning::h8_norm, true},               {41, &Tuning::aspp_lanes, true},
    {42, &Tuning::small_n_64, false},           {43, &Tuning::zone_cols, false},
    {51, &Tuning::wino_pack, true},              {52, &Tuning::cgnet_fused, true},
    {53, &Tuning::dsn_fused, true},              {54, &Tuning::rrn_head, true},
};
int* tuning_field(Tuning& t, int key) {
    for (const TuneKey& k : TUNE_KEYS)
        if (k.key == key) return &(t.*k.field);
    return nullptr;
}
bool tuning_set(Tuning& t, int key, int value) {
    int* f = tuning_field(t, key);
    if (f) *f = value;
    return f != nullptr;
}
bool tuning_plan_time(int key) {
    for (const TuneKey& k : TUNE_KEYS)
        if (k.key == key) return k.plan;
    return false;
}

// compute units of the current device, cached per device id (a process may drive several devices with different counts)
int device_cus() {
    static std::atomic<int> cache[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    const bool cached = dev >= 0 && dev < 64;
    if (cached) {
        const int v = cache[dev].load(std::memory_order_relaxed);
        if (v > 0) return v;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return -1;
    const int cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (cached) cache[dev].store(cus, std::memory_order_relaxed);
    return cus;
}

static thread_local std::string g_err;
extern "C" const char* quber_last_error(void) { return g_err.c_str(); }
void set_error(const std::string& m) { g_err = m; }
int fail(const std::string& m) { g_err = m; return -1; }

// ---- stage profiler (common.h: ProfScope; plan.h: Profiler) ----
thread_local Profiler* g_prof = nullptr;

ProfScope::ProfScope(const char* tag, double bytes, double flops, hipStream_t s) : rec(-1), st(s) {
    Profiler* p = g_prof;
    if (!p) return;
    int ti = -1;
    for (size_t i = 0; i < p->tags.size(); ++i)
        if (p->tags[i] == tag) { ti = (int)i; break; }
    if (ti < 0) { ti = (int)p->tags.size(); p->tags.emplace_back(tag); }
    ProfRec r{ti, p->get(), p->get(), bytes, flops};
    if (!r.e0 || !r.e1 || hipEventRecord(r.e0, s) != hipSuccess) return;
    rec = (int)p->recs.size();
    p->recs.push_back(r);
}
ProfScope::~ProfScope() {
    if (rec >= 0 && g_prof) (void)hipEventRecord(g_prof->recs[rec].e1, st);
}

}  // namespace quber
