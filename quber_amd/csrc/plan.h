// What the host-side units of libquber_hip.so (runtime, plan, plan_lmff, api, api_ops) share: the context, the ops of a launch plan, the plan builder.
#pragma once
#include <math.h>
#include <string.h>

#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/quber_hip.h"
#include "common.h"

namespace quber {

int* tuning_field(Tuning& t, int key);    // the member option `key` names, or null
bool tuning_plan_time(int key);           // the key shapes the plan: it acts when quber_finalize_weights builds it and is refused afterwards

// ---- stage profiler (common.h: ProfScope) ----
struct ProfRec { int tag; hipEvent_t e0, e1; double bytes, flops; };
struct StageSum { std::string name; double ms = 0.0, bytes = 0.0, flops = 0.0; int launches = 0; };
struct Profiler {
    std::vector<std::string> tags;
    std::vector<ProfRec> recs;
    std::vector<hipEvent_t> pool;
    size_t used = 0;
    std::vector<StageSum> sums;
    hipEvent_t get() {
        if (used == pool.size()) {
            hipEvent_t e = nullptr;
            if (hipEventCreate(&e) != hipSuccess) return nullptr;
            pool.push_back(e);
        }
        return pool[used++];
    }
    ~Profiler() { for (hipEvent_t e : pool) (void)hipEventDestroy(e); }
};
extern thread_local Profiler* g_prof;     // the profiler of the open quber_profile_begin / _end window of this thread, or null

// a device buffer of the context that its entry allocates on first use and keeps (ws_reserve, api.hip)
struct LazyWs { void* p = nullptr; size_t bytes = 0; };
enum LazyId {
    WS_PERTURB,     // bit planes of quber_perturb_masks in its device-memory placement: grown on demand
    WS_MASKNMS,     // bit planes, pair table, rank map and per-frame tables of quber_mask_nms: for max_batch frames
    WS_COCOAP,      // bit planes, pair table(s), areas and boxes of quber_coco_match / _boundary, the planes of quber_op_mask_boundary: grown on demand
    WS_SCENE,       // bit planes, pair and touch tables, member sets, prefix sums of quber_scene_perturb: grown on demand
    WS_MEANSHIFT,   // seed slots, histograms, running minimum, raw labels, block partials of the mean-shift entries (meanshift.hip): for max_batch frames
    WS_GMS,         // counts, compacted points, running minimum, raw labels, tables, block partials of the Gaussian mean-shift entries (gms.hip): for max_batch frames
    WS_ZOOM,        // extents, keep flags, depth keys, paint order, key map of the zoom-in entries (zoom.hip): for max_batch frames
    WS_RRN,         // block partials, counts, paint order, owner map, id tables of quber_rrn_paste (rrn.hip): for max_batch frames
    WS_LOSSES,      // moments, centres, block partials, histograms, foreground plane of the loss entries (losses.hip): for max_batch frames
    WS_COUNT
};

constexpr int GN_SLOTS = 64;
inline size_t gn_slot_doubles(int max_batch) { return (size_t)2 * 32 * max_batch * 4; }

enum OpKind { OP_CONV = 0, OP_NORM = 1, OP_OTHER = 2, OP_KINDS = 3 };
struct Op {
    std::function<int(int, hipStream_t)> run;
    int kind;
    std::string name;   // first weight key (convs / norms) or a short tag
    double flops;       // algorithmic FLOPs at batch 1 (convolutions only)
    int launches;       // kernel launches per run (memsets not counted)
    int lane = 0;       // 0 = the caller's stream; 1.. = a side stream of the context (small batches only, see quber_forward)
    int ctl = 0;        // 1 = fork `lane` here (it may start once the main stream has reached this point), 2 = join it
};
constexpr int LANES = 3;            // side lanes 1, 2: the fusion convolutions of res2 and of res3
constexpr int LANE_BATCH = 16;      // side lanes are used up to this batch (their workspaces are sized for it) ...
constexpr int LANE_BATCH_F32 = 12;  // ... in the fp32-class modes (exact fp32, bf16x3) up to this one.  Same-box A/B of the step with the lanes against one
                                    // stream (profiles/r20_lanes.md): exact fp32 -5 % at 1 frame, -4.3 % at 4, -3 % at 6, -1.5 ... -2.3 % at 8, -0.8 ... -1.3 % at 12,
                                    // 0 ... +0.5 % at 16 (the headline stays on one stream); bf16x3 -3.4 ... -4 % at 8, -2.4 % / +1 % at 16 on two boxes (one stream);
                                    // fp16 data path -11 % at 8, -5.8 ... -6.7 % at 16 (640x480), -1 ... -1.8 % at 1024x1024 x 8.  (Batches <= 2 until round 6's last pass.)

}  // namespace quber

struct quber_ctx {
    quber_config cfg;
    quber::Tuning tune;           // this context's knobs (quber_set_option); starts as a copy of the process defaults
    std::map<std::string, std::vector<float>> hostw;
    std::vector<std::pair<std::string, int64_t>> specs;
    std::vector<void*> allocs;
    size_t alloc_bytes = 0;       // device bytes owned by the context (quber_workspace_bytes)
    int* enc_bad = nullptr;       // out-of-range flag of the label-map encoder
    std::vector<quber::Op> ops;
    std::map<std::string, quber::View> taps;
    float* gauss = nullptr;
    void* enc_ws = nullptr;
    uint8_t* err_ws = nullptr;
    void* post_ws = nullptr;
    void* cleanup_ws = nullptr;   // parent map, per-root tables, per-instance keys of the connected-component clean-up (cleanup.hip)
    quber::LazyWs lazy[quber::WS_COUNT];   // the workspaces that are not part of quber_create (ws_reserve, api.hip); quber_destroy frees every one
    double* gn_stats = nullptr;   // [GN_SLOTS][launch group <= 4][max_batch][32 groups][sum, sum of squares]
    int gn_slots = 0;
    float* splitk_ws = nullptr;
    size_t splitk_floats = 0;
    float* wino_ws = nullptr;     // V | M of the Winograd layers (sized for the largest one at max_batch)
    size_t wino_floats = 0;
    // side lanes (batch <= LANE_BATCH): independent branches of the network on streams of their own, each with its own workspaces
    hipStream_t lane_stream[quber::LANES] = {};
    hipEvent_t lane_fork[quber::LANES] = {}, lane_join[quber::LANES] = {};
    float* lane_wino_ws[quber::LANES] = {};
    size_t lane_wino_floats[quber::LANES] = {};
    float* lane_splitk_ws[quber::LANES] = {};
    size_t lane_splitk_floats = 0;
    bool lanes_built = false;     // the plan contains fork / join points
    bool lanes_on = false;        // ... and this forward uses them
    int lane_now = 0;             // lane of the op being launched (0 = the caller's stream): its workspaces are the ones to use
    quber::View X;        // [2][Bmax][H][W][8] (16 channels of fp16 in the fp16 data path)
    float* q = nullptr;   // [Bmax][planes][H/4][W/4]
    const uint8_t* cur_bgr = nullptr;
    const uint8_t* cur_depth = nullptr;
    const float* cur_off = nullptr;
    float* cur_out = nullptr;
    // Depth Seeding Network contexts (with_network = 4): what the plan's first and last op read, set by quber_dsn_forward
    const float* dsn_xyz = nullptr;
    const float* dsn_z = nullptr;   // quber_dsn_forward_depth: the depth planes the first op back-projects with dsn_cam instead of reading dsn_xyz
    double dsn_cam[4] = {};         // fx, fy, cx, cy
    int dsn_convention = 0;
    int dsn_flags = 0;
    float* dsn_clean = nullptr;   // [Bmax][3][H][W]: xyz with NaN -> 0 and the y flag applied
    double* dsn_stats = nullptr;  // GroupNorm sums of every norm of the plan, cleared by its first op
    size_t dsn_stats_bytes = 0;
    float *dsn_logits = nullptr, *dsn_offsets = nullptr, *dsn_votes = nullptr;
    uint8_t *dsn_classes = nullptr, *dsn_fg = nullptr;
    // Region Refinement Network contexts (with_network = 5; their GroupNorm sums are dsn_stats): set by quber_rrn_forward
    const float* rrn_rgb = nullptr;
    const uint8_t* rrn_mask = nullptr;
    float rrn_thr = 0.f;
    float* rrn_logits = nullptr;
    uint8_t* rrn_refined = nullptr;
    double flops = 0.0;
    double wino_flops = 0.0;      // algorithmic FLOPs (batch 1) of the layers that take the Winograd path
    double wino_saved = 0.0;      // ... and the part of them the path does not execute
    double wino_pad = 0.0;        // executed FLOPs (batch 1) spent on the padding of ragged / short-phase Winograd tiles
    std::vector<hipEvent_t> prof_events;
    std::unique_ptr<quber::Profiler> prof;
    bool stem_fused = false;      // the plan's first op reads the u8 images and the encoding itself: quber_forward launches no preprocess kernel
    bool finalized = false;
    int device = 0;
};

namespace quber {

enum Affine { AF_NONE, AF_FROZEN_BN, AF_BIAS, AF_BIAS_BN };

struct GnFuse { double* sums = nullptr; int groups = 0; };
// a GroupNorm + ReLU whose output has exactly one consumer: if that consumer takes the Winograd path it normalises
// while loading and the separate apply pass is skipped
struct DeferredNorm {
    View in, out;
    const double* stats = nullptr;
    const float *gamma = nullptr, *beta = nullptr;
    int C = 0, G = 0;
    bool absorbed = false;                 // set by the consumer at plan time: it normalises while it loads
};
struct LastConv { std::shared_ptr<GnFuse> fuse; const float* out = nullptr; int G = 0, C = 0; };

// Walks a network's module tree and appends its launches to c->ops (plan.hip).  A dry builder only records the weights the walk asks for (c->specs).
struct Builder {
    quber_ctx* c;
    bool dry;
    LastConv last_conv;
    std::shared_ptr<DeferredNorm> pending_norm;
    std::string err;    // the first error of the walk; the caller reports it
    int Bmax, H, W;
    int cur_lane = 0;   // lane of the ops being emitted (0 = main)
    int aes = 4;        // element size of the activation tensors: 2 in the fp16 data path (quber_config.compute_dtype 2)

    Builder(quber_ctx* ctx, bool d) : c(ctx), dry(d), Bmax(ctx->cfg.max_batch), H(ctx->cfg.height), W(ctx->cfg.width) {
        if (ctx->cfg.compute_dtype == 2 && ctx->cfg.with_network == 1) aes = 2;
    }

    // ---- host weights, device memory ----
    const float* hw(const std::string& name, int64_t numel);
    void* dalloc_bytes(size_t bytes);
    float* upload16(const std::vector<_Float16>& v);
    float* upload(const std::vector<float>& v);
    const float* upload_weights(const std::vector<float>& packed);
    const void* split3(const float* dev_w, size_t n);
    View make(int C, int h, int w, int G = 1);
    static View slice(View v, int coff, int C, long gs = -1);

    // ---- ops ----
    void emit_conv(const std::string& name, const std::vector<const float*>& w, const View& in, int cin_real, const View& out, int k, int stride, int pad, int dil, bool affine,
                   const std::vector<float>& scale, const std::vector<float>& shift, const std::vector<float>& prelu, const View* res, bool relu, const std::vector<int>& dil_g = {});
    void conv(const std::vector<std::string>& names, const View& in, int cin_real, const View& out, int k, int stride, int pad, int dil, Affine af, const View* res, bool relu,
              const std::vector<int>& dil_g = {});
    void fuse_shortcut(const std::vector<std::string>& n3, const std::vector<std::string>& ns, const View& y, int mid, const View& x, int cin, int stride, const View& out);
    void gn_relu(const std::vector<std::string>& names, const View& in, const View& out, bool single_consumer = false);
    void op(std::function<int(int, hipStream_t)> f);
    void fork(int L);
    void back_to_main() { cur_lane = 0; }
    void join(int L);
    void conv_gn(const std::string& n, const View& in, const View& tmp, const View& out, int k, int dil, bool single_consumer = false, int cin_real = -1);
    void emit_stem_fused(const std::vector<std::string>& names, const View& out);
    void build();       // the refiner network
};
void build_lmff(Builder& b);     // LMFFNet (plan_lmff.hip)
void build_cgnet(Builder& b);    // CGNet (plan_cgnet.hip)
void build_dsn(Builder& b);      // Depth Seeding Network of UOIS-Net-3D (plan_dsn.hip)
void build_rrn(Builder& b);      // Region Refinement Network of UOIS-Net-3D (plan_rrn.hip)

int check_cfg(const quber_config& c);
bool op_set_tuning(int key, int value);      // api_ops.hip: the process-only keys 2, 11, 12, 26 of quber_set_tuning; false: not one of them

inline int check_batch(quber_ctx* c, int batch) {
    if (!c) return fail("null context");
    if (batch < 1 || batch > c->cfg.max_batch) return fail("batch outside 1..max_batch");
    return 0;
}
// 2 * batch frames on the engine: originals in [0, batch), their mirrors in [batch, 2 * batch)
inline int check_tta_batch(quber_ctx* c, int batch) {
    if (!c) return fail("null context");
    if (batch < 1 || 2L * batch > c->cfg.max_batch) return fail("test-time augmentation: 2 * batch outside 2..max_batch");
    return 0;
}

}  // namespace quber
