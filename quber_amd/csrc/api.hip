// The C ABI of libquber_hip.so: contexts, weight ingestion, the forward pass and the context-free adapter / metrics / in-painting entries.
// (The stand-alone test ops quber_op_* are in api_ops.hip.)
#include "plan.h"

#include <optional>

using namespace quber;

// the time-stamp readers of the diagnostic builds (wino_fused.hip WF_STAMPS, conv_h8.hip H8_STAMPS, conv_x8.hip X8_STAMPS)
namespace quber { int wf_read_stamps(unsigned long long* dst, int n), h8_read_stamps(unsigned long long* dst, int n), x8_read_stamps(unsigned long long* dst, int n); }

int quber::check_cfg(const quber_config& c) {
    if (c.height <= 0 || c.width <= 0) return fail("height and width must be positive");
    if (c.with_network && (c.height < 16 || c.width < 16)) return fail("frames smaller than 16 x 16 are not supported");
    if (c.with_network == 2) {
        if (c.height % 8 || c.width % 8) return fail("LMFFNet needs height and width to be multiples of 8");
        return c.max_batch >= 1 ? 0 : fail("max_batch must be >= 1");
    }
    if (c.with_network == 3) {
        if (c.height % 8 || c.width % 8) return fail("CGNet needs height and width to be multiples of 8");
        return c.max_batch >= 1 ? 0 : fail("max_batch must be >= 1");
    }
    if (c.with_network == 4) {
        if (c.height < 16 || c.width < 16 || c.height % 16 || c.width % 16) return fail("the Depth Seeding Network needs height and width to be multiples of 16");
        return c.max_batch >= 1 ? 0 : fail("max_batch must be >= 1");
    }
    if (c.with_network == 5) {
        if (c.height != c.width || c.height < 16 || c.height % 16) return fail("the Region Refinement Network needs square crops whose side is a multiple of 16");
        return c.max_batch >= 1 ? 0 : fail("max_batch must be >= 1");
    }
    if (c.max_batch < 1) return fail("max_batch must be >= 1");
    if (c.max_instances < 1) return fail("max_instances must be >= 1");
    if (c.resnet_depth != 50 && c.resnet_depth != 101 && c.resnet_depth != 152) return fail("resnet_depth must be 50, 101 or 152");
    if (c.res5_dilation != 1 && c.res5_dilation != 2 && c.res5_dilation != 4) return fail("res5_dilation must be 1, 2 or 4");
    if (c.res5_dilation == 1) return fail("res5_dilation 1 (output stride 32) is not supported by this build");
    if (c.error_classes < 2 || c.error_classes > 4) return fail("error_classes must be 2..4");
    if (c.streams != 1 && c.streams != 2) return fail("streams must be 1 or 2");
    if (c.with_network == 1 && c.convs_dim != 128 && c.convs_dim != 256) return fail("convs_dim must be 128 or 256");
    if (c.with_network == 1 && c.head_channels != 32 && c.head_channels != 64) return fail("head_channels must be 32 or 64");
    if (c.compute_dtype < 0 || c.compute_dtype > 3)
        return fail("compute_dtype must be 0 (fp32 MFMA), 1 (bf16 operands), 2 (fp16 operands) or 3 (fp32 operands as 3 bf16 terms)");
    if (c.with_network && c.hierarchical) {
        if (c.n_levels < 1 || c.n_levels > 5) return fail("n_levels must be 1..5");
        int seen[5] = {0, 0, 0, 0, 0};
        for (int i = 0; i < c.n_levels; ++i) {
            if (c.level_heads[i][0] < 0) return fail("empty hierarchy level");
            for (int j = 0; j < 5 && c.level_heads[i][j] >= 0; ++j) {
                const int k = c.level_heads[i][j];
                if (k > 4) return fail("hierarchy head id out of range");
                seen[k]++;
            }
        }
        const int want[5] = {1, 1, 1, c.eee_mask_on ? 1 : 0, c.eee_boundary_on ? 1 : 0};
        for (int k = 0; k < 5; ++k)
            if (seen[k] != want[k]) return fail("the hierarchy must list every enabled head exactly once");
    }
    if (c.top_k < 1 || c.top_k > 254) return fail("top_k must be in 1..254");
    if (c.gaussian_sigma < 1 || c.gaussian_sigma > 40) return fail("gaussian_sigma out of range");
    return 0;
}

// Makes `w` hold at least `need` bytes: nothing when it already does, else a new buffer replaces the old one and alloc_bytes stays exact.
// A buffer never shrinks; an entry that asks for the same size on every call allocates once.
static int ws_reserve(quber_ctx* c, LazyWs& w, size_t need) {
    if (need <= w.bytes) return 0;
    if (w.p) {
        QB_CHECK(hipFree(w.p));                              // (waits for the launches that may still use it)
        c->alloc_bytes -= w.bytes;
        w = LazyWs();
    }
    QB_CHECK(hipMalloc(&w.p, need));
    w.bytes = need;
    c->alloc_bytes += need;
    return 0;
}

extern "C" {

const char* quber_version(void) { return "quber-hip 0.1 (gfx950, fp32 MFMA)"; }

void quber_default_config(quber_config* c) {
    memset(c, 0, sizeof(*c));
    c->height = 480; c->width = 640; c->max_batch = 1; c->max_instances = 64;
    c->resnet_depth = 50; c->res5_dilation = 2; c->backbone_fusion_layers = 2; c->head_fusion_layers = 3;
    c->error_classes = 4; c->gaussian_sigma = 10; c->nms_kernel = 7; c->top_k = 200; c->stuff_area = 2048;
    c->min_instance_area = 512; c->label_divisor = 1000; c->with_network = 1;
    c->eee_mask_on = 0; c->eee_boundary_on = 1; c->hierarchical = 1; c->fusion_feat = 1; c->fusion_pred = 1;
    c->n_levels = 2;
    c->streams = 2;
    c->fusion_add = 0;
    c->convs_dim = 128; c->head_channels = 32;
    for (int i = 0; i < 5; ++i)
        for (int j = 0; j < 5; ++j) c->level_heads[i][j] = -1;
    c->level_heads[0][0] = 4;                                   // [[eee_boundary], [foreground, center, offset]]
    c->level_heads[1][0] = 0; c->level_heads[1][1] = 1; c->level_heads[1][2] = 2;
    c->center_threshold = 0.3f; c->boundary_ratio = 0.01f;
    const float mean[6] = {103.53f, 116.28f, 123.675f, 127.5f, 127.5f, 127.5f};
    for (int i = 0; i < 6; ++i) { c->pixel_mean[i] = mean[i]; c->pixel_std[i] = 1.f; }
}

int quber_create(const quber_config* cfg, quber_ctx** out) {
    if (!cfg || !out) return fail("null argument");
    if (check_cfg(*cfg)) return -1;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("no HIP device available");
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return fail("hipGetDevice failed");
    quber_ctx* c = new quber_ctx();
    c->cfg = *cfg;
    c->tune = quber::g_tune;          // the process defaults of this moment; quber_set_option changes this context only
    c->device = device;
    const int B = cfg->max_batch, H = cfg->height, W = cfg->width;
    // Gaussian template (predictor.py:246-251): float64 exp rounded to f32
    const int sg = cfg->gaussian_sigma, side = 6 * sg + 3, c0 = 3 * sg + 1;
    std::vector<float> g((size_t)side * side);
    for (int y = 0; y < side; ++y)
        for (int x = 0; x < side; ++x)
            g[(size_t)y * side + x] = (float)exp(-((double)((x - c0) * (x - c0)) + (double)((y - c0) * (y - c0))) / (2.0 * sg * sg));
    Builder b(c, false);
    c->gauss = b.upload(g);
    c->enc_ws = b.dalloc_bytes(encode_ws_bytes(B, cfg->max_instances, H, W));
    c->enc_bad = (int*)b.dalloc_bytes(16);
    c->err_ws = (uint8_t*)b.dalloc_bytes(errmaps_ws_bytes(B, cfg->max_instances > 0 ? cfg->max_instances : 1, H, W));
    c->post_ws = b.dalloc_bytes(postprocess_ws_bytes(B, H, W, cfg->top_k));
    c->cleanup_ws = b.dalloc_bytes(cleanup_ws_bytes(B, H, W, cfg->top_k));
    if (!b.err.empty()) {
        std::string e = b.err;
        quber_destroy(c);
        return fail(e);
    }
    if (cfg->with_network) {      // the weights the plan will ask for
        Builder dry(c, true);
        if (cfg->with_network == 2) build_lmff(dry);
        else if (cfg->with_network == 3) build_cgnet(dry);
        else if (cfg->with_network == 4) build_dsn(dry);
        else if (cfg->with_network == 5) build_rrn(dry);
        else dry.build();
    }
    *out = c;
    return 0;
}

void quber_destroy(quber_ctx* c) {
    if (!c) return;
    if (c->prof && quber::g_prof == c->prof.get()) quber::g_prof = nullptr;
    for (hipEvent_t e : c->prof_events) (void)hipEventDestroy(e);   // nothing useful to do with a failure while tearing down
    for (int l = 1; l < LANES; ++l) {
        if (c->lane_fork[l]) (void)hipEventDestroy(c->lane_fork[l]);
        if (c->lane_join[l]) (void)hipEventDestroy(c->lane_join[l]);
        if (c->lane_stream[l]) (void)hipStreamDestroy(c->lane_stream[l]);
    }
    for (void* p : c->allocs) (void)hipFree(p);
    for (LazyWs& w : c->lazy)
        if (w.p) (void)hipFree(w.p);
    delete c;
}

int quber_num_weights(quber_ctx* c) { return c ? (int)c->specs.size() : 0; }
int quber_weight_spec(quber_ctx* c, int i, const char** name, int64_t* numel) {
    if (!c || i < 0 || i >= (int)c->specs.size()) return fail("weight index out of range");
    *name = c->specs[i].first.c_str();
    *numel = c->specs[i].second;
    return 0;
}

int quber_set_weight(quber_ctx* c, const char* name, const float* host, int64_t numel) {
    if (!c || !name || !host || numel <= 0) return fail("bad argument to quber_set_weight");
    if (c->finalized) return fail("weights already finalized");
    c->hostw[name].assign(host, host + numel);
    return 0;
}

int quber_finalize_weights(quber_ctx* c) {
    if (!c) return fail("null context");
    if (!c->cfg.with_network) return fail("context was created with with_network = 0");
    if (c->finalized) return fail("weights already finalized");
    quber::TuneScope tscope(&c->tune);          // the plan is shaped by THIS context's options
    Builder b(c, false);
    c->flops = c->wino_flops = c->wino_saved = c->wino_pad = 0.0;
    if (c->cfg.with_network >= 2 && c->cfg.with_network <= 5) {
        c->splitk_floats = (size_t)4 << 20;
        c->splitk_ws = (float*)b.dalloc_bytes(sizeof(float) * c->splitk_floats);
        if (c->cfg.with_network == 2) build_lmff(b);
        else if (c->cfg.with_network == 3) build_cgnet(b);
        else if (c->cfg.with_network == 4) build_dsn(b);
        else build_rrn(b);
    } else {
        b.build();
    }
    if (c->wino_floats) c->wino_ws = (float*)b.dalloc_bytes(sizeof(float) * c->wino_floats);
    if (c->lanes_built) {          // side lanes: streams, fork / join events, workspaces sized for LANE_BATCH frames
        c->lane_splitk_floats = c->splitk_floats;       // as large as the caller's stream's (160 MiB): a launch picks the same split on a lane as off it
        for (int l = 1; l < LANES; ++l) {
            QB_CHECK(hipStreamCreateWithFlags(&c->lane_stream[l], hipStreamNonBlocking));
            QB_CHECK(hipEventCreateWithFlags(&c->lane_fork[l], hipEventDisableTiming));
            QB_CHECK(hipEventCreateWithFlags(&c->lane_join[l], hipEventDisableTiming));
            c->lane_splitk_ws[l] = (float*)b.dalloc_bytes(sizeof(float) * c->lane_splitk_floats);
            if (c->lane_wino_floats[l]) c->lane_wino_ws[l] = (float*)b.dalloc_bytes(sizeof(float) * c->lane_wino_floats[l]);
        }
    }
    if (!b.err.empty()) {
        c->ops.clear();
        return fail(b.err);
    }
    QB_CHECK(hipDeviceSynchronize());
    c->hostw.clear();
    c->finalized = true;
    return 0;
}

double quber_forward_flops(quber_ctx* c) { return c ? c->flops : 0.0; }
double quber_forward_flops_executed(quber_ctx* c) {
    if (!c) return 0.0;
    // a layer planned as Winograd F(m x m,3x3) multiplies (m+2)^2 times per m x m output tile and channel pair (padded tiles included) instead of 9 m^2
    return c->flops - c->wino_saved;
}
double quber_forward_flops_padding(quber_ctx* c) { return c ? c->wino_pad : 0.0; }
void quber_set_tuning(int32_t key, int32_t value) {
    // process defaults: copied by every context created afterwards (quber_create) and used by the stand-alone quber_op_* ops; contexts that already exist keep theirs (quber_set_option)
    if (op_set_tuning(key, value)) return;       // keys 2, 11, 12, 26: state of the stand-alone ops
    (void)quber::tuning_set(quber::g_tune, key, value);
}

int quber_set_option(quber_ctx* c, int32_t key, int32_t value) {
    if (!c) return fail("null context");
    if (quber::tuning_plan_time(key) && c->finalized) return fail("option " + std::to_string(key) + " shapes the plan: set it before quber_finalize_weights");
    if (!quber::tuning_set(c->tune, key, value)) return fail("unknown option key " + std::to_string(key));
    return 0;
}

int quber_get_option(quber_ctx* c, int32_t key, int32_t* value) {
    if (!c || !value) return fail("null argument");
    int* f = quber::tuning_field(c->tune, key);
    if (!f) return fail("unknown option key " + std::to_string(key));
    *value = *f;
    return 0;
}

#ifdef WF_STAMPS
int quber_wf_read_stamps(unsigned long long* dst, int n) { return quber::wf_read_stamps(dst, n); }
#endif
#ifdef H8_STAMPS
int quber_h8_read_stamps(unsigned long long* dst, int n) { return quber::h8_read_stamps(dst, n); }
#endif
#ifdef X8_STAMPS
int quber_x8_read_stamps(unsigned long long* dst, int n) { return quber::x8_read_stamps(dst, n); }
#endif
#ifdef PK_STAMPS
int quber_pk_read_stamps(unsigned long long* dst, int n) { return quber::pk_read_stamps(dst, n); }
int quber_pk_read_span(unsigned long long* dst, int n) { return quber::pk_read_span(dst, n); }
#endif

int32_t quber_debug_persistent_segments(int32_t tiles, int32_t blocks, int32_t k_slices, int32_t min_share, int32_t block, int32_t* out4, int32_t cap) {
    return quber::conv_persistent_segments(tiles, blocks, k_slices, min_share, block, out4, cap);
}
int32_t quber_debug_persistent_fixup(int32_t tiles, int32_t blocks, int32_t k_slices, int32_t min_share, int32_t xcd, int32_t j, int32_t* tile, int32_t* slots, int32_t cap) {
    return quber::conv_persistent_fixup(tiles, blocks, k_slices, min_share, xcd, j, tile, slots, cap);
}

int64_t quber_debug_ws_bytes(int32_t which, int32_t b, int32_t n, int32_t m, int32_t h, int32_t w, int32_t flag) {
    switch (which) {
    case 0: return (int64_t)mask_nms_ws_bytes(b, n, h, w);
    case 1: return (int64_t)coco_match_ws_bytes(b, n, h, w, flag);
    case 2: return (int64_t)scene_ws_bytes(b, n, m, h, w);
    case 3: return (int64_t)meanshift_ws_bytes(b, h, w);
    case 4: return (int64_t)gms_ws_bytes(b, h, w);
    case 5: return (int64_t)zoom_ws_bytes(b, h, w);
    case 6: return (int64_t)losses_ws_bytes(b, h, w);
    case 7: return (int64_t)cleanup_ws_bytes(b, h, w, n);
    case 8: return (int64_t)postprocess_ws_bytes(b, h, w, n);
    default: return -1;
    }
}

int quber_profile_begin(quber_ctx* c) {
    if (!c) return fail("null context");
    if (!c->prof) c->prof.reset(new quber::Profiler());
    c->prof->recs.clear(); c->prof->sums.clear(); c->prof->used = 0;
    quber::g_prof = c->prof.get();
    return 0;
}

int quber_profile_end(quber_ctx* c, void* stream) {
    if (!c || !c->prof || quber::g_prof != c->prof.get()) return fail("quber_profile_end without quber_profile_begin");
    quber::g_prof = nullptr;
    QB_CHECK(hipStreamSynchronize((hipStream_t)stream));
    quber::Profiler& p = *c->prof;
    p.sums.assign(p.tags.size(), quber::StageSum());
    for (size_t i = 0; i < p.tags.size(); ++i) p.sums[i].name = p.tags[i];
    for (const quber::ProfRec& r : p.recs) {
        float ms = 0.f;
        QB_CHECK(hipEventElapsedTime(&ms, r.e0, r.e1));
        quber::StageSum& s = p.sums[r.tag];
        s.ms += ms; s.bytes += r.bytes; s.flops += r.flops; s.launches += 1;
    }
    return 0;
}

int quber_profile_num_stages(quber_ctx* c) { return (c && c->prof) ? (int)c->prof->sums.size() : 0; }

int quber_profile_stage(quber_ctx* c, int i, const char** name, double* ms, double* bytes, double* flops, int32_t* launches) {
    if (!c || !c->prof || i < 0 || i >= (int)c->prof->sums.size()) return fail("stage index out of range");
    const quber::StageSum& s = c->prof->sums[i];
    *name = s.name.c_str(); *ms = s.ms; *bytes = s.bytes; *flops = s.flops; *launches = s.launches;
    return 0;
}

int quber_num_ops(quber_ctx* c) { return c ? (int)c->ops.size() : 0; }
int quber_op_info(quber_ctx* c, int i, const char** name, int32_t* kind, double* flops, int32_t* launches) {
    if (!c || i < 0 || i >= (int)c->ops.size()) return fail("op index out of range");
    const Op& o = c->ops[i];
    *name = o.name.c_str(); *kind = o.kind; *flops = o.flops; *launches = o.launches;
    return 0;
}

int quber_encode_initial_masks(quber_ctx* c, const uint8_t* masks, int32_t batch, int32_t n, float* out, void* stream) {
    if (check_batch(c, batch)) return -1;
    if (n > c->cfg.max_instances) return fail("more initial masks than max_instances");
    if (!masks && n > 0) return fail("null masks");
    return launch_encode(masks, batch, n, c->cfg.height, c->cfg.width, c->gauss, c->cfg.gaussian_sigma, c->cfg.encode_legacy_f32, c->enc_ws, out, (hipStream_t)stream);
}

int quber_encode_label_map(quber_ctx* c, const int32_t* labels, int32_t batch, int32_t n, float* out, void* stream) {
    if (check_batch(c, batch)) return -1;
    if (n > c->cfg.max_instances) return fail("more instances than max_instances");
    if (!labels && n > 0) return fail("null label map");
    return launch_encode_labels(labels, batch, n, c->cfg.height, c->cfg.width, c->gauss, c->cfg.gaussian_sigma, c->cfg.encode_legacy_f32, c->enc_ws, out, c->enc_bad, (hipStream_t)stream);
}

int64_t quber_workspace_bytes(quber_ctx* c) { return c ? (int64_t)c->alloc_bytes : 0; }

int quber_explicit_error_maps(quber_ctx* c, const uint8_t* init, int32_t n_init, const uint8_t* gt, int32_t n_gt, int32_t batch, uint8_t* out, void* stream) {
    if (check_batch(c, batch)) return -1;
    const int H = c->cfg.height, W = c->cfg.width;
    // util.py:80-83: dilation = max(1, int(round(ratio * diag)))   (Python round = half to even)
    int d = (int)rint((double)c->cfg.boundary_ratio * sqrt((double)H * H + (double)W * W));
    if (d < 1) d = 1;
    return launch_errmaps(init, n_init, gt, n_gt, batch, c->cfg.max_instances > 0 ? c->cfg.max_instances : 1, H, W, d, c->err_ws, out, (hipStream_t)stream);
}

// The shared preamble of quber_forward / quber_forward_profiled: checks, this context's options for every launcher (`scope`, until the caller returns), the pointers
// the plan's ops read, the preprocess kernel.  0 = go on, < 0 = error, 1 = an LMFFNet / CGNet context that the caller runs itself (lmff_own; nothing stored or launched).
static int forward_begin(quber_ctx* c, const char* who, std::optional<quber::TuneScope>& scope, const uint8_t* bgr, const uint8_t* depth,
                         const float* offs, int batch, float* logits, bool lmff_own, bool rest_ok, const char* null_msg, hipStream_t st) {
    if (check_batch(c, batch)) return -1;
    if (!c->finalized) return fail(std::string(who) + " before quber_finalize_weights");
    scope.emplace(&c->tune);
    if (c->cfg.with_network == 4) return fail(std::string(who) + ": a Depth Seeding Network context runs through quber_dsn_forward");
    if (c->cfg.with_network == 5) return fail(std::string(who) + ": a Region Refinement Network context runs through quber_rrn_forward");
    if (lmff_own && c->cfg.with_network >= 2) return 1;
    if (!bgr || (!depth && c->cfg.streams == 2) || !offs || !logits || !rest_ok) return fail(null_msg);
    c->cur_out = logits;
    c->cur_bgr = bgr; c->cur_depth = depth; c->cur_off = offs;
    return c->stem_fused ? 0 : launch_preprocess(bgr, depth, offs, c->X, batch, c->cfg.max_batch, c->cfg.height, c->cfg.width,
                                                 c->cfg.pixel_mean, c->cfg.pixel_std, c->cfg.streams, st);
}

int quber_forward(quber_ctx* c, const uint8_t* bgr, const uint8_t* depth, const float* offs, int32_t batch, float* logits, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    std::optional<quber::TuneScope> tscope;
    int rc = forward_begin(c, "quber_forward", tscope, bgr, depth, offs, batch, logits, true, true, "null tensor", st);
    if (rc == 1) {   // LMFFNet / CGNet: (bgr, depth) -> 3 / 2 class planes; `offs` is unused
        if (!bgr || !depth || !logits) return fail("null tensor");
        c->cur_out = logits;
        const long pixels = (long)batch * c->cfg.height * c->cfg.width;
        int r2 = c->cfg.with_network == 3 ? launch_cg_preprocess(bgr, depth, pixels, c->X.p, st) : launch_lmff_preprocess(bgr, depth, pixels, c->X.p, st);
        for (size_t i = 0; !r2 && i < c->ops.size(); ++i)
            if (!c->ops[i].ctl) r2 = c->ops[i].run(batch, st);
        return r2;
    }
    if (rc) return rc;
    // side lanes: at small batches the independent branches of the plan (Builder::fork / join) run on streams of the context
    c->lanes_on = c->lanes_built && tune().lanes && batch <= (c->cfg.compute_dtype == 0 || c->cfg.compute_dtype == 3 ? LANE_BATCH_F32 : LANE_BATCH) && c->lane_stream[1] != nullptr &&
                  quber::g_prof == nullptr;
    auto lane_used = [&](int l) { return c->lanes_on && l > 0; };
    for (auto& op : c->ops) {
        if (op.ctl == 1) {
            if (lane_used(op.lane)) {
                QB_CHECK(hipEventRecord(c->lane_fork[op.lane], st));
                QB_CHECK(hipStreamWaitEvent(c->lane_stream[op.lane], c->lane_fork[op.lane], 0));
            }
            continue;
        }
        if (op.ctl == 2) {
            if (lane_used(op.lane)) {
                QB_CHECK(hipEventRecord(c->lane_join[op.lane], c->lane_stream[op.lane]));
                QB_CHECK(hipStreamWaitEvent(st, c->lane_join[op.lane], 0));
            }
            continue;
        }
        c->lane_now = lane_used(op.lane) ? op.lane : 0;
        rc = op.run(batch, c->lane_now ? c->lane_stream[op.lane] : st);
        if (rc) return rc;
    }
    c->lane_now = 0;
    c->lanes_on = false;
    return 0;
}

// every op of a U-Net plan (plan_dsn.hip, plan_rrn.hip) in plan order; op_ms (the profiled forms): an event pair around every op, read after one synchronisation
static int run_ops(quber_ctx* c, int batch, hipStream_t st, double* op_ms) {
    const size_t n = c->ops.size();
    if (op_ms && c->prof_events.size() < 2 * n) {
        const size_t old = c->prof_events.size();
        c->prof_events.resize(2 * n);
        for (size_t i = old; i < 2 * n; ++i) QB_CHECK(hipEventCreate(&c->prof_events[i]));
    }
    for (size_t i = 0; i < n; ++i) {
        if (op_ms) QB_CHECK(hipEventRecord(c->prof_events[2 * i], st));
        if (!c->ops[i].ctl) {
            const int rc = c->ops[i].run(batch, st);
            if (rc) return rc;
        }
        if (op_ms) QB_CHECK(hipEventRecord(c->prof_events[2 * i + 1], st));
    }
    if (!op_ms) return 0;
    QB_CHECK(hipStreamSynchronize(st));
    for (size_t i = 0; i < n; ++i) {
        float ms = 0.f;
        QB_CHECK(hipEventElapsedTime(&ms, c->prof_events[2 * i], c->prof_events[2 * i + 1]));
        op_ms[i] = ms;
    }
    return 0;
}

// quber_dsn_forward / quber_dsn_forward_profiled: the checks, the pointers the plan's first and last op read, then run_ops
// (z + cam + convention in place of xyz: quber_dsn_forward_depth)
static int dsn_run(quber_ctx* c, const char* who, const float* xyz, int batch, int flags, float* fg_logits, float* offsets, float* votes, uint8_t* fg_classes, uint8_t* fg,
                   hipStream_t st, double* op_ms, const float* z = nullptr, const double* cam = nullptr, int convention = 0) {
    if (check_batch(c, batch)) return -1;
    if (c->cfg.with_network != 4) return fail(std::string(who) + ": the context was not created with with_network = 4");
    if (!c->finalized) return fail(std::string(who) + " before quber_finalize_weights");
    if (!xyz && !z) return fail(std::string(who) + (cam ? ": null depth" : ": null xyz"));
    if (flags & ~1) return fail(std::string(who) + ": unknown flag bits");
    if (z) {
        if (!cam) return fail(std::string(who) + ": null camera");
        if (convention != 0 && convention != 1) return fail(std::string(who) + ": convention 0 (pinhole) or 1 (uois)");
        for (int i = 0; i < 4; ++i) {
            if (!std::isfinite(cam[i]) || (i < 2 && cam[i] == 0.0)) return fail(std::string(who) + ": the camera must be finite with focal lengths other than zero");
            c->dsn_cam[i] = cam[i];
        }
        c->dsn_convention = convention;
    }
    quber::TuneScope tscope(&c->tune);
    c->dsn_xyz = xyz; c->dsn_z = z; c->dsn_flags = flags;
    c->dsn_logits = fg_logits; c->dsn_offsets = offsets; c->dsn_votes = votes; c->dsn_classes = fg_classes; c->dsn_fg = fg;
    return run_ops(c, batch, st, op_ms);
}

int quber_dsn_forward(quber_ctx* c, const float* xyz, int32_t batch, int32_t flags, float* fg_logits, float* offsets, float* votes, uint8_t* fg_classes, uint8_t* fg,
                      void* stream) {
    return dsn_run(c, "quber_dsn_forward", xyz, batch, flags, fg_logits, offsets, votes, fg_classes, fg, (hipStream_t)stream, nullptr);
}

int quber_dsn_forward_profiled(quber_ctx* c, const float* xyz, int32_t batch, int32_t flags, float* fg_logits, float* offsets, float* votes, uint8_t* fg_classes,
                               uint8_t* fg, void* stream, double* op_ms) {
    if (!op_ms) return fail("quber_dsn_forward_profiled: null op_ms");
    return dsn_run(c, "quber_dsn_forward_profiled", xyz, batch, flags, fg_logits, offsets, votes, fg_classes, fg, (hipStream_t)stream, op_ms);
}

int quber_dsn_forward_depth(quber_ctx* c, const float* z, int32_t batch, int32_t flags, const double* cam, int32_t convention, float* fg_logits, float* offsets,
                            float* votes, uint8_t* fg_classes, uint8_t* fg, void* stream) {
    if (!z || !cam) return fail("quber_dsn_forward_depth: null depth or camera");
    return dsn_run(c, "quber_dsn_forward_depth", nullptr, batch, flags, fg_logits, offsets, votes, fg_classes, fg, (hipStream_t)stream, nullptr, z, cam, convention);
}

int quber_dsn_forward_depth_profiled(quber_ctx* c, const float* z, int32_t batch, int32_t flags, const double* cam, int32_t convention, float* fg_logits,
                                     float* offsets, float* votes, uint8_t* fg_classes, uint8_t* fg, void* stream, double* op_ms) {
    if (!z || !cam || !op_ms) return fail("quber_dsn_forward_depth_profiled: null depth, camera or op_ms");
    return dsn_run(c, "quber_dsn_forward_depth_profiled", nullptr, batch, flags, fg_logits, offsets, votes, fg_classes, fg, (hipStream_t)stream, op_ms, z, cam, convention);
}

// quber_rrn_forward / quber_rrn_forward_profiled: the same for a Region Refinement Network context
static int rrn_run(quber_ctx* c, const char* who, const float* rgb_crop, const uint8_t* mask_crop, int n, float thr, float* logits, uint8_t* refined, hipStream_t st,
                   double* op_ms) {
    if (check_batch(c, n)) return -1;
    if (c->cfg.with_network != 5) return fail(std::string(who) + ": the context was not created with with_network = 5");
    if (!c->finalized) return fail(std::string(who) + " before quber_finalize_weights");
    if (!rgb_crop || !mask_crop) return fail(std::string(who) + ": null crops");
    if (!logits && !refined) return fail(std::string(who) + ": neither logits nor refined masks requested");
    if (!(thr == thr)) return fail(std::string(who) + ": logit_threshold is not a number");
    quber::TuneScope tscope(&c->tune);
    c->rrn_rgb = rgb_crop; c->rrn_mask = mask_crop; c->rrn_thr = thr; c->rrn_logits = logits; c->rrn_refined = refined;
    return run_ops(c, n, st, op_ms);
}

int quber_rrn_forward(quber_ctx* c, const float* rgb_crop, const uint8_t* mask_crop, int32_t n, float logit_threshold, float* logits, uint8_t* refined, void* stream) {
    return rrn_run(c, "quber_rrn_forward", rgb_crop, mask_crop, n, logit_threshold, logits, refined, (hipStream_t)stream, nullptr);
}

int quber_rrn_forward_profiled(quber_ctx* c, const float* rgb_crop, const uint8_t* mask_crop, int32_t n, float logit_threshold, float* logits, uint8_t* refined,
                               void* stream, double* op_ms) {
    if (!op_ms) return fail("quber_rrn_forward_profiled: null op_ms");
    return rrn_run(c, "quber_rrn_forward_profiled", rgb_crop, mask_crop, n, logit_threshold, logits, refined, (hipStream_t)stream, op_ms);
}

int quber_forward_profiled(quber_ctx* c, const uint8_t* bgr, const uint8_t* depth, const float* offs, int32_t batch,
                           float* logits, void* stream, double* kind_ms, int32_t* kind_launches) {
    hipStream_t st = (hipStream_t)stream;
    std::optional<quber::TuneScope> tscope;
    int rc = forward_begin(c, "quber_forward_profiled", tscope, bgr, depth, offs, batch, logits, false, kind_ms && kind_launches, "null argument", st);
    if (rc) return rc;
    const size_t n = c->ops.size();
    if (c->prof_events.size() < 2 * n) {
        const size_t old = c->prof_events.size();
        c->prof_events.resize(2 * n);
        for (size_t i = old; i < 2 * n; ++i) QB_CHECK(hipEventCreate(&c->prof_events[i]));
    }
    c->lanes_on = false;          // one stream: every op in plan order
    for (size_t i = 0; i < n; ++i) {
        QB_CHECK(hipEventRecord(c->prof_events[2 * i], st));
        if (!c->ops[i].ctl) {
            rc = c->ops[i].run(batch, st);
            if (rc) return rc;
        }
        QB_CHECK(hipEventRecord(c->prof_events[2 * i + 1], st));
    }
    QB_CHECK(hipStreamSynchronize(st));
    for (int k = 0; k < OP_KINDS; ++k) { kind_ms[k] = 0.0; kind_launches[k] = 0; }
    for (size_t i = 0; i < n; ++i) {
        float ms = 0.f;
        QB_CHECK(hipEventElapsedTime(&ms, c->prof_events[2 * i], c->prof_events[2 * i + 1]));
        kind_ms[c->ops[i].kind] += ms;
        kind_launches[c->ops[i].kind] += 1;
    }
    return 0;
}

int quber_postprocess(quber_ctx* c, const float* logits, int32_t n_planes, int32_t batch, float* pan, int32_t* count,
                      float* labels, float* scores, float* boxes, int32_t* centers, int32_t* ncenters, void* stream) {
    if (check_batch(c, batch)) return -1;
    PostCfg pc;
    pc.threshold = c->cfg.center_threshold; pc.nms_kernel = c->cfg.nms_kernel; pc.top_k = c->cfg.top_k;
    pc.stuff_area = c->cfg.stuff_area; pc.min_area = c->cfg.min_instance_area; pc.label_divisor = c->cfg.label_divisor;
    pc.cap = c->cfg.top_k;
    return launch_postprocess(logits, n_planes, batch, c->cfg.height, c->cfg.width, pc, c->post_ws, pan, count, labels,
                              scores, boxes, centers, ncenters, (hipStream_t)stream);
}

int quber_extract_masks(quber_ctx* c, const float* pan, const float* labels, int32_t batch, int32_t max_inst,
                        uint8_t* masks, void* stream) {
    if (check_batch(c, batch)) return -1;
    return launch_extract_masks(pan, labels, batch, c->cfg.height, c->cfg.width, c->cfg.top_k, max_inst, masks,
                                (hipStream_t)stream);
}

int quber_tta_flip_inputs(quber_ctx* c, uint8_t* bgr, uint8_t* depth, uint8_t* masks, int32_t batch, int32_t n, void* stream) {
    if (check_tta_batch(c, batch)) return -1;
    if (n < 0 || n > c->cfg.max_instances) return fail("initial masks outside 0..max_instances");
    if (!bgr || (!masks && n > 0)) return fail("null tensor");
    const int H = c->cfg.height, W = c->cfg.width;
    const long hw = (long)H * W;
    hipStream_t st = (hipStream_t)stream;
    if (launch_tta_flip_u8(bgr, bgr + batch * hw * 3, batch, H, W, 3, st)) return -1;
    if (depth && launch_tta_flip_u8(depth, depth + batch * hw * 3, batch, H, W, 3, st)) return -1;
    if (n > 0 && launch_tta_flip_u8(masks, masks + (long)batch * n * hw, (long)batch * n, H, W, 1, st)) return -1;
    return 0;
}

int quber_tta_merge(quber_ctx* c, const float* logits2, int32_t n_planes, int32_t batch, float* out, void* stream) {
    if (check_tta_batch(c, batch)) return -1;
    if (n_planes < 4) return fail("test-time augmentation: fewer than 4 logit planes");
    if (!logits2 || !out) return fail("null tensor");
    return launch_tta_merge(logits2, n_planes, batch, c->cfg.height, c->cfg.width, out, (hipStream_t)stream);
}

// ---- the predicted error maps (errhead.hip); usable on a context without a network ----
int quber_error_decode(quber_ctx* c, const float* logits, int32_t n_planes, int32_t first_plane, int32_t classes, int32_t batch,
                       uint8_t* classes_out, uint32_t* hist, void* stream) {
    if (check_batch(c, batch)) return -1;
    if (!logits || !classes_out) return fail("null tensor");
    return launch_error_decode(logits, n_planes, first_plane, classes, batch, c->cfg.height, c->cfg.width, classes_out, hist,
                               (hipStream_t)stream);
}

int quber_error_mask_hist(quber_ctx* c, const uint8_t* classes_map, const uint8_t* masks, int32_t batch, int32_t n, int32_t classes,
                          uint32_t* out, void* stream) {
    if (check_batch(c, batch)) return -1;
    if (n < 0 || n > c->cfg.max_instances) return fail("initial masks outside 0..max_instances");
    if (n == 0) return 0;
    if (!classes_map || !masks || !out) return fail("null tensor");
    return launch_error_mask_hist(classes_map, masks, batch, n, classes, c->cfg.height, c->cfg.width, out, (hipStream_t)stream);
}

int quber_error_score(quber_ctx* c, const uint8_t* classes_map, const uint8_t* explicit_maps, int32_t kind, int32_t error_type,
                      int32_t classes, int32_t batch, uint64_t* table, void* stream) {
    if (check_batch(c, batch)) return -1;
    if (!classes_map || !explicit_maps || !table) return fail("null tensor");
    return launch_error_score(classes_map, explicit_maps, kind, error_type, classes, batch, c->cfg.height, c->cfg.width,
                              (unsigned long long*)table, (hipStream_t)stream);
}

int quber_error_overlay(quber_ctx* c, const uint8_t* bgr, const uint8_t* classes_map, int32_t batch, uint32_t color0, uint32_t color1,
                        uint32_t color2, uint32_t color3, uint8_t* out, void* stream) {
    if (check_batch(c, batch)) return -1;
    if (!bgr || !classes_map || !out) return fail("null tensor");
    const unsigned colors[4] = {color0, color1, color2, color3};
    return launch_error_overlay(bgr, classes_map, batch, c->cfg.height, c->cfg.width, colors, out, (hipStream_t)stream);
}

// ---- iterative refinement (iterate.hip); usable on a context without a network ----
int quber_relabel_panoptic(quber_ctx* c, const float* panoptic, const float* labels, const int32_t* count, int32_t batch, int32_t mirror,
                           int32_t* ids, void* stream) {
    if (mirror ? check_tta_batch(c, batch) : check_batch(c, batch)) return -1;
    if (!panoptic || !labels || !count || !ids) return fail("null tensor");
    return launch_relabel_panoptic(panoptic, labels, count, batch, c->cfg.top_k, mirror != 0, c->cfg.height, c->cfg.width, ids,
                                   (hipStream_t)stream);
}

int quber_overlap_masks(quber_ctx* c, const uint8_t* masks, const int32_t* ids, int32_t batch, int32_t n_masks, int32_t n_ids,
                        uint32_t* table, uint32_t* area, void* stream) {
    if (check_batch(c, batch)) return -1;
    if (n_masks < 0 || n_masks > c->cfg.max_instances) return fail("initial masks outside 0..max_instances");
    if (n_ids < 0 || n_ids > 254) return fail("n_ids outside 0..254");
    if (!ids || (n_masks > 0 && (!masks || !table))) return fail("null tensor");
    return launch_overlap_masks(masks, ids, batch, n_masks, n_ids, c->cfg.height, c->cfg.width, table, area, (hipStream_t)stream);
}

int quber_overlap_ids(quber_ctx* c, const int32_t* a, const int32_t* b, int32_t batch, int32_t n_a, int32_t n_b, uint32_t* table,
                      void* stream) {
    if (check_batch(c, batch)) return -1;
    if (n_a < 0 || n_a > 254 || n_b < 0 || n_b > 254) return fail("n_a / n_b outside 0..254");
    if (!a || !b || !table) return fail("null tensor");
    return launch_overlap_ids(a, b, batch, n_a, n_b, c->cfg.height, c->cfg.width, table, (hipStream_t)stream);
}

// ---- connected-component clean-up (cleanup.hip); usable on a context without a network ----
int quber_cleanup_ids(quber_ctx* c, int32_t* ids, int32_t batch, int32_t n_ids, int32_t connectivity, int32_t keep_largest,
                      int32_t min_island_area, int32_t max_hole_area, uint32_t* report, void* stream) {
    if (check_batch(c, batch)) return -1;
    if (!ids) return fail("null tensor");
    return launch_cleanup_ids(ids, batch, c->cfg.height, c->cfg.width, n_ids, connectivity, keep_largest, min_island_area, max_hole_area,
                              c->cleanup_ws, report, (hipStream_t)stream);
}

int quber_cleanup_postprocess(quber_ctx* c, const float* logits, int32_t n_planes, int32_t batch, float* panoptic, const float* labels,
                              const int32_t* count, float* scores, float* boxes, int32_t connectivity, int32_t keep_largest,
                              int32_t min_island_area, int32_t max_hole_area, uint32_t* report, void* stream) {
    if (check_batch(c, batch)) return -1;
    if (!logits || !panoptic || !labels || !count || !scores || !boxes) return fail("null tensor");
    return launch_cleanup_postprocess(logits, n_planes, batch, c->cfg.height, c->cfg.width, c->cfg.top_k, c->cfg.label_divisor, panoptic, labels, count, scores,
                                      boxes, connectivity, keep_largest, min_island_area, max_hole_area, c->cleanup_ws, report,
                                      (hipStream_t)stream);
}

// ---- perturbed initial masks (perturb.hip); usable on a context without a network ----
int quber_perturb_masks(quber_ctx* c, const uint8_t* masks, int32_t batch, int32_t n_masks, const int32_t* programs, int32_t n_ops,
                        int32_t ops_per_round, const double* iou_targets, uint8_t* out, uint32_t* report, int32_t placement, void* stream) {
    if (check_batch(c, batch)) return -1;
    if (n_masks < 0) return fail("perturb: negative n_masks");
    if (placement < 0 || placement > 2) return fail("perturb: placement must be 0 (auto), 1 (LDS) or 2 (device memory)");
    if (n_masks == 0) return 0;
    if (!masks || !out || !iou_targets || (!programs && n_ops > 0)) return fail("perturb: null tensor");
    const int H = c->cfg.height, W = c->cfg.width;
    const long M = (long)batch * n_masks;
    const size_t bytes = (size_t)M * H * W;
    if (out < masks + bytes && masks < out + bytes) return fail("perturb: dev_out overlaps dev_masks");
    const bool fits = perturb_fits_lds(H, W);
    if (placement == 1 && !fits) return fail("perturb: three bit planes of this frame do not fit the 160 KB of LDS a workgroup may declare");
    const bool lds = placement == 1 || (placement == 0 && fits);
    // the only allocation of this entry: made on first use, kept, grown when a larger batch comes
    if (!lds && ws_reserve(c, c->lazy[WS_PERTURB], perturb_ws_bytes(M, H, W))) return -1;
    return launch_perturb(masks, M, H, W, programs, n_ops, ops_per_round, iou_targets, out, report, lds ? 1 : 0, c->lazy[WS_PERTURB].p, (hipStream_t)stream);
}

// ---- mask NMS of scored, overlapping initial masks (masknms.hip); usable on a context without a network ----
int quber_mask_nms(quber_ctx* c, const uint8_t* masks, const float* scores, int32_t batch, int32_t n_masks, float thresh, int32_t on_top,
                   uint8_t* out_masks, int32_t* ids, int32_t* source, float* out_scores, int32_t* report, void* stream) {
    if (check_batch(c, batch)) return -1;
    const int limit = std::min(c->cfg.max_instances, mask_nms_max());
    if (n_masks < 0 || n_masks > limit) return fail("mask nms: n_masks outside 0..min(max_instances, 1024)");
    if (on_top != 0 && on_top != 1) return fail("mask nms: on_top must be 0 (large) or 1 (small)");
    if (!(thresh == thresh)) return fail("mask nms: thresh is not a number");
    const int H = c->cfg.height, W = c->cfg.width;
    if ((long)H * W > (1L << 24)) return fail("mask nms: a frame of more than 2^24 pixels (the overlap counts are compared in float32)");
    if (!ids || !report || (n_masks > 0 && (!masks || !scores || !out_masks || !source || !out_scores))) return fail("mask nms: null tensor");
    const size_t bytes = (size_t)batch * n_masks * H * W;
    if (out_masks != masks && out_masks < masks + bytes && masks < out_masks + bytes) return fail("mask nms: dev_out_masks overlaps dev_masks partially");
    // the only allocation of this entry: made by the first call, for max_batch x limit masks, and kept
    if (n_masks > 0 && ws_reserve(c, c->lazy[WS_MASKNMS], mask_nms_ws_bytes(c->cfg.max_batch, limit, H, W))) return -1;
    return launch_mask_nms(masks, scores, batch, n_masks, H, W, thresh, on_top, out_masks, ids, source, out_scores, report, c->lazy[WS_MASKNMS].p,
                           (hipStream_t)stream);
}

// ---- scene-level perturbation of a frame's instance list (scene.hip); usable on a context without a network ----
int quber_scene_perturb(quber_ctx* c, const uint8_t* gt, const uint8_t* props, const int32_t* n_gt, const int32_t* n_prop, int32_t batch,
                        int32_t n_gt_rows, int32_t n_prop_rows, int32_t max_masks, double min_mask_ratio, const uint8_t* fp_act,
                        const uint8_t* gs_act, const uint8_t* merge_act, const uint8_t* split_act, const int32_t* split_try,
                        const uint8_t* delete_act, uint8_t* out_masks, int32_t* info, int32_t* report, void* stream) {
    if (check_batch(c, batch)) return -1;
    if (n_gt_rows < 0 || n_prop_rows < 0 || (long)n_gt_rows + n_prop_rows > scene_max())
        return fail("scene perturb: n_gt_rows + n_prop_rows outside 0..256");
    if (max_masks < 1 || max_masks > scene_max()) return fail("scene perturb: max_masks outside 1..256");
    if (!(min_mask_ratio >= 0.0 && min_mask_ratio <= 1.0)) return fail("scene perturb: min_mask_ratio outside 0..1");
    const int H = c->cfg.height, W = c->cfg.width;
    if ((long)H * W > (1L << 30)) return fail("scene perturb: a frame of more than 2^30 pixels");
    if (!n_gt || !n_prop || !merge_act || !split_act || !split_try || !delete_act || !out_masks || !info || !report || (n_gt_rows > 0 && !gt) ||
        (n_prop_rows > 0 && (!props || !fp_act || !gs_act)))
        return fail("scene perturb: null tensor");
    // the only allocation of this entry: made on first use, kept, grown when a larger call comes
    if (ws_reserve(c, c->lazy[WS_SCENE], scene_ws_bytes(batch, n_gt_rows + n_prop_rows, max_masks, H, W))) return -1;
    const ScenePerturbArgs q{gt, props, n_gt, n_prop, n_gt_rows, n_prop_rows, max_masks, min_mask_ratio, fp_act, gs_act, merge_act, split_act,
                             split_try, delete_act, out_masks, info, report};
    return launch_scene_perturb(q, batch, H, W, c->lazy[WS_SCENE].p, (hipStream_t)stream);
}

// ---- the per-frame half of COCO AP (cocoap.hip); usable on a context without a network ----
int quber_coco_match(quber_ctx* c, const uint8_t* dt, const float* scores, const double* dt_boxes, int32_t n_dt, const uint8_t* gt,
                     const uint8_t* gt_flags, const double* gt_area, const double* gt_boxes, int32_t n_gt, int32_t batch, int32_t iou_type,
                     const double* iou_thrs, int32_t n_thrs, const double* area_rng, int32_t n_rng, int32_t* counts, int32_t* order,
                     float* out_scores, double* dt_area, double* gt_area_used, double* iou, uint8_t* dtm, uint8_t* dtig, uint8_t* gi,
                     int32_t* gorder, void* stream) {
    if (check_batch(c, batch)) return -1;
    if (n_gt < 0 || n_gt > 1024) return fail("coco match: n_gt outside 0..1024");
    if (iou_type != 0 && iou_type != 1) return fail("coco match: iou_type must be 0 (segm) or 1 (bbox)");
    const int H = c->cfg.height, W = c->cfg.width;
    // the only allocation of this entry: made on first use, kept, grown when a larger call comes
    if (ws_reserve(c, c->lazy[WS_COCOAP], coco_match_ws_bytes(batch, n_gt, H, W, iou_type))) return -1;
    const CocoMatchArgs q{dt, scores, dt_boxes, n_dt, gt, gt_flags, gt_area, gt_boxes, n_gt, iou_type, iou_thrs, n_thrs, area_rng, n_rng,
                          counts, order, out_scores, dt_area, gt_area_used, iou, dtm, dtig, gi, gorder};
    return launch_coco_match(q, batch, H, W, c->lazy[WS_COCOAP].p, (hipStream_t)stream);
}

// ... under Boundary IoU (boundaryap.hip makes the boundary planes); the same lazy workspace, larger by the second set of planes, pair table and areas
int quber_coco_match_boundary(quber_ctx* c, const uint8_t* dt, const float* scores, int32_t n_dt, const uint8_t* gt, const uint8_t* gt_flags,
                              const double* gt_area, int32_t n_gt, int32_t batch, int32_t dilation, const double* iou_thrs, int32_t n_thrs,
                              const double* area_rng, int32_t n_rng, int32_t* counts, int32_t* order, float* out_scores, double* dt_area,
                              double* gt_area_used, double* iou, double* mask_iou, double* boundary_iou, uint8_t* dtm, uint8_t* dtig, uint8_t* gi,
                              int32_t* gorder, void* stream) {
    if (check_batch(c, batch)) return -1;
    if (n_gt < 0 || n_gt > 1024) return fail("coco match: n_gt outside 0..1024");
    if (dilation < 1 || dilation > mask_boundary_max_dilation()) return fail("coco match: dilation outside 1..64");
    const int H = c->cfg.height, W = c->cfg.width;
    if (ws_reserve(c, c->lazy[WS_COCOAP], coco_match_ws_bytes(batch, n_gt, H, W, 2))) return -1;
    const CocoMatchArgs q{dt, scores, nullptr, n_dt, gt, gt_flags, gt_area, nullptr, n_gt, 0, iou_thrs, n_thrs, area_rng, n_rng,
                          counts, order, out_scores, dt_area, gt_area_used, iou, dtm, dtig, gi, gorder};
    return launch_coco_match_boundary(q, dilation, mask_iou, boundary_iou, batch, H, W, c->lazy[WS_COCOAP].p, (hipStream_t)stream);
}

// ---- the boundary of masks as Boundary AP takes it (boundaryap.hip): the kernel of quber_coco_match_boundary on its own; any frame size ----
int quber_op_mask_boundary(quber_ctx* c, const uint8_t* masks, int32_t n, int32_t h, int32_t w, int32_t dilation, uint8_t* out, int32_t* area,
                           void* stream) {
    if (!c) return fail("null context");
    if (h < 1 || w < 1 || (long)h * w > (1L << 30)) return fail("mask boundary: an empty frame or one of more than 2^30 pixels");
    if (n < 0) return fail("mask boundary: negative n");
    if (dilation < 1 || dilation > mask_boundary_max_dilation()) return fail("mask boundary: dilation outside 1..64");
    if (n == 0) return 0;
    if (!masks || !out || !area) return fail("mask boundary: null tensor");
    const size_t bytes = (size_t)n * h * w;
    if (out != masks && out < masks + bytes && masks < out + bytes) return fail("mask boundary: dev_out overlaps dev_masks partially");
    // the planes live in the workspace of quber_coco_match: made on first use, kept, grown when a larger call comes
    if (ws_reserve(c, c->lazy[WS_COCOAP], mask_boundary_ws_bytes(n, h, w))) return -1;
    return launch_mask_boundary(masks, n, h, w, dilation, out, area, c->lazy[WS_COCOAP].p, (hipStream_t)stream);
}

// ---- mean-shift clustering of pixel embeddings into initial masks (meanshift.hip); usable on a context without a network ----
static int meanshift_ws(quber_ctx* c) {      // the only allocation of the five entries: made by the first call, for max_batch frames, and kept
    return ws_reserve(c, c->lazy[WS_MEANSHIFT], meanshift_ws_bytes(c->cfg.max_batch, c->cfg.height, c->cfg.width));
}

static int meanshift_args(quber_ctx* c, const char* what, int32_t batch, int32_t channels, int32_t num_seeds) {
    if (check_batch(c, batch)) return -1;
    if (channels != 64) return fail(std::string(what) + ": the embedding must have 64 channels (NUM_UNITS of every UCN config)");
    if (num_seeds < 1 || num_seeds > 128) return fail(std::string(what) + ": num_seeds outside 1..128");
    const long n = (long)c->cfg.height * c->cfg.width;
    if (n > (1L << 24)) return fail(std::string(what) + ": a frame of more than 2^24 pixels (the pixel counts are compared in float32)");
    if (num_seeds > n) return fail(std::string(what) + ": more seeds than the frame has pixels");
    return 0;
}

int quber_meanshift_seeds(quber_ctx* c, const float* emb, int32_t batch, int32_t channels, const int32_t* first, int32_t num_seeds, int32_t* indices,
                          void* stream) {
    if (meanshift_args(c, "meanshift seeds", batch, channels, num_seeds)) return -1;
    if (!emb || !first || !indices) return fail("meanshift seeds: null tensor");
    if (meanshift_ws(c)) return -1;
    return launch_meanshift_seeds(emb, first, batch, num_seeds, c->cfg.height, c->cfg.width, indices, c->lazy[WS_MEANSHIFT].p, c->cfg.max_batch,
                                  (hipStream_t)stream);
}

int quber_meanshift_climb(quber_ctx* c, const float* emb, int32_t batch, int32_t channels, const int32_t* indices, int32_t num_seeds, float kappa,
                          int32_t iters, float* seeds, void* stream) {
    if (meanshift_args(c, "meanshift climb", batch, channels, num_seeds)) return -1;
    if (!emb || !seeds) return fail("meanshift climb: null tensor");
    if (iters < 0 || iters > 1000) return fail("meanshift climb: iters outside 0..1000");
    if (!(kappa >= 0.f) || kappa > 64.f) return fail("meanshift climb: kappa outside 0..64");
    if (meanshift_ws(c)) return -1;
    return launch_meanshift_climb(emb, indices, seeds, batch, num_seeds, c->cfg.height, c->cfg.width, kappa, iters, c->lazy[WS_MEANSHIFT].p,
                                  c->cfg.max_batch, (hipStream_t)stream);
}

int quber_meanshift_link(quber_ctx* c, const float* seeds, int32_t batch, int32_t num_seeds, float epsilon, int32_t* seed_labels, void* stream) {
    if (check_batch(c, batch)) return -1;
    return launch_meanshift_link(seeds, batch, num_seeds, epsilon, seed_labels, (hipStream_t)stream);
}

static int meanshift_assign_args(const char* what, int32_t n_masks, const float* depth_z, float thresh) {
    if (n_masks < 0 || n_masks > 254) return fail(std::string(what) + ": n_masks outside 0..254");
    if (depth_z && !(thresh >= 0.f && thresh <= 1.f)) return fail(std::string(what) + ": depth threshold outside 0..1");
    return 0;
}

int quber_meanshift_assign(quber_ctx* c, const float* emb, int32_t batch, int32_t channels, const float* seeds, const int32_t* seed_labels,
                           int32_t num_seeds, const float* depth_z, float depth_threshold, int32_t n_masks, int32_t* ids, uint8_t* masks,
                           int32_t* report, void* stream) {
    if (meanshift_args(c, "meanshift assign", batch, channels, num_seeds)) return -1;
    if (meanshift_assign_args("meanshift assign", n_masks, depth_z, depth_threshold)) return -1;
    if (!emb || !seeds || !seed_labels || !ids || !report || (n_masks > 0 && !masks)) return fail("meanshift assign: null tensor");
    if (meanshift_ws(c)) return -1;
    return launch_meanshift_assign(emb, seeds, seed_labels, depth_z, depth_threshold, batch, num_seeds, n_masks, c->cfg.height, c->cfg.width, ids,
                                   masks, report, c->lazy[WS_MEANSHIFT].p, c->cfg.max_batch, (hipStream_t)stream);
}

int quber_meanshift_cluster(quber_ctx* c, const float* emb, int32_t batch, int32_t channels, const int32_t* first, int32_t num_seeds, float kappa,
                            int32_t iters, float epsilon, const float* depth_z, float depth_threshold, int32_t n_masks, int32_t* indices,
                            float* seeds, int32_t* seed_labels, int32_t* ids, uint8_t* masks, int32_t* report, void* stream) {
    if (meanshift_args(c, "meanshift", batch, channels, num_seeds)) return -1;
    if (meanshift_assign_args("meanshift", n_masks, depth_z, depth_threshold)) return -1;
    if (iters < 0 || iters > 1000) return fail("meanshift: iters outside 0..1000");
    if (!(kappa >= 0.f) || kappa > 64.f) return fail("meanshift: kappa outside 0..64");
    if (!(epsilon >= 0.f)) return fail("meanshift: epsilon is negative or not a number");
    if (!emb || !first || !indices || !seeds || !seed_labels || !ids || !report || (n_masks > 0 && !masks)) return fail("meanshift: null tensor");
    for (const void* p : {(const void*)emb, (const void*)first, (const void*)indices, (const void*)seeds, (const void*)seed_labels, (const void*)ids,
                          (const void*)report, (const void*)depth_z})
        if ((uintptr_t)p & 3) return fail("meanshift: a 32-bit tensor that is not 4-byte aligned");
    if (meanshift_ws(c)) return -1;
    const int H = c->cfg.height, W = c->cfg.width, cap = c->cfg.max_batch;
    hipStream_t st = (hipStream_t)stream;
    if (launch_meanshift_seeds(emb, first, batch, num_seeds, H, W, indices, c->lazy[WS_MEANSHIFT].p, cap, st)) return -1;
    if (launch_meanshift_climb(emb, indices, seeds, batch, num_seeds, H, W, kappa, iters, c->lazy[WS_MEANSHIFT].p, cap, st)) return -1;
    if (launch_meanshift_link(seeds, batch, num_seeds, epsilon, seed_labels, st)) return -1;
    return launch_meanshift_assign(emb, seeds, seed_labels, depth_z, depth_threshold, batch, num_seeds, n_masks, H, W, ids, masks, report,
                                   c->lazy[WS_MEANSHIFT].p, cap, st);
}

// ---- Gaussian mean shift of centre votes into initial masks, and the IMP (gms.hip); usable on a context without a network ----
static int gms_ws(quber_ctx* c) {            // the only allocation of the six entries: made by the first call, for max_batch frames, and kept
    if (c->lazy[WS_GMS].p) return 0;
    if (gms_prepare()) return -1;
    return ws_reserve(c, c->lazy[WS_GMS], gms_ws_bytes(c->cfg.max_batch, c->cfg.height, c->cfg.width));
}

static int gms_args(quber_ctx* c, const char* what, int32_t batch, int32_t num_seeds) {
    if (check_batch(c, batch)) return -1;
    if (num_seeds < 1 || num_seeds > 256) return fail(std::string(what) + ": num_seeds outside 1..256");
    if ((long)c->cfg.height * c->cfg.width > (1L << 24)) return fail(std::string(what) + ": a frame of more than 2^24 pixels");
    return 0;
}

int quber_gms_seeds(quber_ctx* c, const float* votes, const uint8_t* fg, int32_t batch, int32_t subsample, const int32_t* first,
                    const uint32_t* draws, int32_t num_seeds, int32_t* indices, int32_t* info, void* stream) {
    if (gms_args(c, "gms seeds", batch, num_seeds)) return -1;
    if (!votes || !fg || !first || !draws || !indices) return fail("gms seeds: null tensor");
    if (gms_ws(c)) return -1;
    return launch_gms_seeds(votes, fg, first, draws, batch, num_seeds, subsample, c->cfg.height, c->cfg.width, indices, info, c->lazy[WS_GMS].p,
                            c->cfg.max_batch, (hipStream_t)stream);
}

int quber_gms_climb(quber_ctx* c, const float* votes, const uint8_t* fg, int32_t batch, int32_t subsample, const int32_t* indices,
                    const int32_t* info, int32_t num_seeds, float sigma, int32_t iters, float* seeds, void* stream) {
    if (gms_args(c, "gms climb", batch, num_seeds)) return -1;
    if (!votes || !fg || !seeds) return fail("gms climb: null tensor");
    if (gms_ws(c)) return -1;
    return launch_gms_climb(votes, fg, indices, info, seeds, batch, num_seeds, subsample, c->cfg.height, c->cfg.width, sigma, iters, true,
                            c->lazy[WS_GMS].p, c->cfg.max_batch, (hipStream_t)stream);
}

int quber_gms_link(quber_ctx* c, const float* seeds, int32_t batch, int32_t num_seeds, const int32_t* info, float epsilon, int32_t* seed_labels,
                   void* stream) {
    if (check_batch(c, batch)) return -1;
    return launch_gms_link(seeds, info, batch, num_seeds, epsilon, seed_labels, (hipStream_t)stream);
}

int quber_gms_assign(quber_ctx* c, const float* votes, const uint8_t* fg, int32_t batch, const float* seeds, const int32_t* seed_labels,
                     const int32_t* info, int32_t num_seeds, int32_t min_pixels, int32_t n_masks, int32_t* ids, uint8_t* masks, float* centers,
                     int32_t* report, void* stream) {
    if (gms_args(c, "gms assign", batch, num_seeds)) return -1;
    if (!votes || !fg || !seeds || !seed_labels || !ids || !centers || !report) return fail("gms assign: null tensor");
    if (gms_ws(c)) return -1;
    return launch_gms_assign(votes, fg, seeds, seed_labels, info, batch, num_seeds, n_masks, min_pixels, c->cfg.height, c->cfg.width, ids, masks,
                             centers, report, c->lazy[WS_GMS].p, c->cfg.max_batch, (hipStream_t)stream);
}

int quber_gms_imp(quber_ctx* c, int32_t* ids, int32_t batch, int32_t n_ids, int32_t ksize, int32_t largest, int32_t n_masks, uint8_t* masks,
                  float* centers, int32_t* report, void* stream) {
    if (check_batch(c, batch)) return -1;
    if (!ids) return fail("gms imp: null tensor");
    if (gms_ws(c)) return -1;
    return launch_gms_imp(ids, batch, n_ids, ksize, largest, n_masks, c->cfg.height, c->cfg.width, masks, centers, report, c->lazy[WS_GMS].p,
                          c->cfg.max_batch, c->cleanup_ws, (hipStream_t)stream);
}

int quber_gms_cluster(quber_ctx* c, const float* votes, const uint8_t* fg, int32_t batch, const int32_t* first, const uint32_t* draws,
                      int32_t num_seeds, float sigma, int32_t iters, float epsilon, int32_t subsample, int32_t min_pixels, int32_t imp_ksize,
                      int32_t imp_largest, int32_t n_masks, int32_t* indices, float* seeds, int32_t* seed_labels, int32_t* info, int32_t* raw_ids,
                      int32_t* ids, uint8_t* masks, float* centers, int32_t* report, void* stream) {
    if (gms_args(c, "gms", batch, num_seeds)) return -1;
    if (!votes || !fg || !first || !draws || !indices || !seeds || !seed_labels || !info || !raw_ids || !ids || !masks || !centers || !report)
        return fail("gms: null tensor");
    if (!(epsilon >= 0.f)) return fail("gms: epsilon is negative or not a number");
    if (n_masks < 1 || n_masks > 254) return fail("gms: n_masks outside 1..254");
    const int H = c->cfg.height, W = c->cfg.width, cap = c->cfg.max_batch;
    if (imp_ksize != 0) {                    // refused before anything is launched
        if (imp_ksize < 1 || imp_ksize > 15 || !(imp_ksize & 1)) return fail("gms imp: ksize must be odd and lie in 1..15");
        if (gms_imp_lds_bytes(H, W) > 152 * 1024) return fail("gms imp: the two bit planes of a frame do not fit the LDS (2 * H * ceil(W / 32) * 4 bytes > 152 KiB)");
    }
    if (gms_ws(c)) return -1;
    hipStream_t st = (hipStream_t)stream;
    if (launch_gms_seeds(votes, fg, first, draws, batch, num_seeds, subsample, H, W, indices, info, c->lazy[WS_GMS].p, cap, st)) return -1;
    if (launch_gms_climb(votes, fg, indices, info, seeds, batch, num_seeds, subsample, H, W, sigma, iters, false, c->lazy[WS_GMS].p, cap, st)) return -1;
    if (launch_gms_link(seeds, info, batch, num_seeds, epsilon, seed_labels, st)) return -1;
    if (launch_gms_assign(votes, fg, seeds, seed_labels, info, batch, num_seeds, n_masks, min_pixels, H, W, raw_ids, imp_ksize ? nullptr : masks,
                          centers, report, c->lazy[WS_GMS].p, cap, st))
        return -1;
    if (launch_gms_copy_ids(raw_ids, ids, (size_t)batch * H * W, st)) return -1;
    if (!imp_ksize) return 0;
    return launch_gms_imp(ids, batch, n_masks, imp_ksize, imp_largest, n_masks, H, W, masks, centers, report, c->lazy[WS_GMS].p, cap, c->cleanup_ws, st);
}

// ---- zoom-in refinement: rois, crops, paste (zoom.hip); usable on a context without a network ----
static int zoom_ws(quber_ctx* c) {           // the only allocation of the three entries: made by the first call, for max_batch frames, and kept
    return ws_reserve(c, c->lazy[WS_ZOOM], zoom_ws_bytes(c->cfg.max_batch, c->cfg.height, c->cfg.width));
}

static int zoom_aligned4(std::initializer_list<const void*> ps, const char* who = "zoom") {
    for (const void* p : ps)
        if ((uintptr_t)p & 3) return fail(std::string(who) + ": a 32-bit tensor that is not 4-byte aligned");
    return 0;
}

int quber_zoom_rois(quber_ctx* c, const int32_t* ids, int32_t batch, int32_t n_ids, float padding, int32_t* rois, void* stream) {
    if (check_batch(c, batch)) return -1;
    if (n_ids < 0 || n_ids > 254) return fail("zoom rois: n_ids outside 0..254");
    if (!(padding >= 0.f) || padding > 16.f) return fail("zoom rois: padding outside 0..16");
    if (!ids || (n_ids > 0 && !rois)) return fail("zoom rois: null tensor");
    if (zoom_aligned4({ids, rois})) return -1;
    if (n_ids == 0) return 0;
    if (zoom_ws(c)) return -1;
    return launch_zoom_rois(ids, batch, n_ids, c->cfg.height, c->cfg.width, padding, rois, c->lazy[WS_ZOOM].p, c->cfg.max_batch, (hipStream_t)stream);
}

int quber_zoom_crop(quber_ctx* c, const uint8_t* bgr, const uint8_t* depth, const int32_t* ids, const int32_t* slots, const int32_t* rois,
                    int32_t batch, int32_t n_ids, int32_t n_slots, int32_t crop, uint8_t* bgr_crop, uint8_t* depth_crop, uint8_t* mask_crop,
                    void* stream) {
    if (check_batch(c, batch)) return -1;
    if (n_ids < 0 || n_ids > 254) return fail("zoom crop: n_ids outside 0..254");
    if (n_slots < 0 || n_slots > c->cfg.max_batch * 254) return fail("zoom crop: n_slots outside 0..254 * max_batch");
    if (crop < 2 || crop > 512) return fail("zoom crop: crop outside 2..512");
    if (n_slots == 0) return 0;
    if (!bgr || !ids || !slots || !rois || !bgr_crop || !mask_crop || (depth && !depth_crop)) return fail("zoom crop: null tensor");
    if (zoom_aligned4({ids, slots, rois})) return -1;
    return launch_zoom_crop(bgr, depth, ids, slots, rois, batch, n_ids, n_slots, crop, c->cfg.height, c->cfg.width, bgr_crop,
                            depth ? depth_crop : nullptr, mask_crop, (hipStream_t)stream);
}

int quber_zoom_paste(quber_ctx* c, const int32_t* crop_ids, const float* crop_scores, const uint32_t* table, const uint32_t* area,
                     const uint8_t* depth_crop, const int32_t* slots, const int32_t* rois, int32_t batch, int32_t n_ids, int32_t n_slots,
                     int32_t crop, int32_t n_crop_ids, float min_overlap, int32_t max_inst, int32_t* out_ids, uint8_t* out_masks,
                     int32_t* source, float* out_scores, float* boxes, int32_t* report, void* stream) {
    if (check_batch(c, batch)) return -1;
    if (n_ids < 0 || n_ids > 254) return fail("zoom paste: n_ids outside 0..254");
    if (n_slots < 0 || n_slots > c->cfg.max_batch * 254) return fail("zoom paste: n_slots outside 0..254 * max_batch");
    if (crop < 2 || crop > 512) return fail("zoom paste: crop outside 2..512");
    if (n_crop_ids < 1 || n_crop_ids > 254) return fail("zoom paste: n_crop_ids outside 1..254");
    if (max_inst < 1 || max_inst > 254) return fail("zoom paste: max_inst outside 1..254");
    if (!(min_overlap == min_overlap)) return fail("zoom paste: min_overlap is not a number");
    if (!out_ids || !out_masks || !source || !out_scores || !boxes || !report) return fail("zoom paste: null tensor");
    if (n_slots > 0 && (!crop_ids || !crop_scores || !table || !area || !slots || !rois)) return fail("zoom paste: null tensor");
    if (zoom_aligned4({crop_ids, crop_scores, table, area, slots, rois, out_ids, source, out_scores, boxes, report})) return -1;
    if (zoom_ws(c)) return -1;
    return launch_zoom_paste(crop_ids, crop_scores, table, area, depth_crop, slots, rois, batch, n_ids, n_slots, crop, n_crop_ids, min_overlap,
                             max_inst, c->cfg.height, c->cfg.width, out_ids, out_masks, source, out_scores, boxes, report, c->lazy[WS_ZOOM].p,
                             c->cfg.max_batch, (hipStream_t)stream);
}

// ---- Region Refinement Network: crops in, refined masks back (rrn.hip); usable on a context without a network ----
int quber_rrn_crop(quber_ctx* c, const uint8_t* bytes, const int32_t* ids, const int32_t* slots, const int32_t* rois, const float* table, int32_t batch,
                   int32_t n_ids, int32_t n_slots, int32_t crop, float* rgb_crop, uint8_t* mask_crop, void* stream) {
    if (check_batch(c, batch)) return -1;
    if (n_ids < 0 || n_ids > 254) return fail("rrn crop: n_ids outside 0..254");
    if (n_slots < 0 || n_slots > c->cfg.max_batch * 254) return fail("rrn crop: n_slots outside 0..254 * max_batch");
    if (crop < 2 || crop > 512) return fail("rrn crop: crop outside 2..512");
    if (n_slots == 0) return 0;
    if (!bytes || !ids || !slots || !rois || !table || !rgb_crop || !mask_crop) return fail("rrn crop: null tensor");
    if (zoom_aligned4({ids, slots, rois, table, rgb_crop}, "rrn crop")) return -1;
    return launch_rrn_crop(bytes, ids, slots, rois, table, batch, n_ids, n_slots, crop, c->cfg.height, c->cfg.width, rgb_crop, mask_crop, (hipStream_t)stream);
}

int quber_rrn_paste(quber_ctx* c, const uint8_t* refined, const int32_t* slots, const int32_t* rois, const float* z, int32_t batch, int32_t n_ids,
                    int32_t n_slots, int32_t crop, int32_t n_masks, int32_t* out_ids, uint8_t* out_masks, int32_t* source, float* keys, int32_t* report,
                    void* stream) {
    if (check_batch(c, batch)) return -1;
    if (n_ids < 0 || n_ids > 254) return fail("rrn paste: n_ids outside 0..254");
    if (n_slots < 0 || n_slots > c->cfg.max_batch * 254) return fail("rrn paste: n_slots outside 0..254 * max_batch");
    if (crop < 2 || crop > 512) return fail("rrn paste: crop outside 2..512");
    if (n_masks < 1 || n_masks > 254) return fail("rrn paste: n_masks outside 1..254");
    if (!z || !out_ids || !out_masks || !source || !report) return fail("rrn paste: null tensor");
    if (n_slots > 0 && (!refined || !slots || !rois || !keys)) return fail("rrn paste: null tensor");
    if (zoom_aligned4({slots, rois, z, out_ids, source, keys, report}, "rrn paste")) return -1;
    if (ws_reserve(c, c->lazy[WS_RRN], rrn_paste_ws_bytes(c->cfg.max_batch, c->cfg.height, c->cfg.width))) return -1;   // made by the first call, and kept
    return launch_rrn_paste(refined, slots, rois, z, batch, n_ids, n_slots, crop, n_masks, c->cfg.height, c->cfg.width, out_ids, out_masks, source, keys, report,
                            c->lazy[WS_RRN].p, c->cfg.max_batch, (hipStream_t)stream);
}

// ---- validation losses: targets, loss record (losses.hip); usable on a context without a network ----
static int losses_ws(quber_ctx* c) {         // the only allocation of the two entries: made by the first call, for max_batch frames, and kept
    return ws_reserve(c, c->lazy[WS_LOSSES], losses_ws_bytes(c->cfg.max_batch, c->cfg.height, c->cfg.width));
}

int quber_loss_targets(quber_ctx* c, const int32_t* gt, int32_t batch, int32_t n_gt, int32_t sigma, int32_t small_area, float small_weight,
                       const float* gauss, float* targets, double* points, int32_t* area, void* stream) {
    if (check_batch(c, batch)) return -1;
    if (n_gt < 0 || n_gt > 254) return fail("loss targets: n_gt outside 0..254");
    if (sigma < 1 || sigma > 20) return fail("loss targets: sigma outside 1..20");
    if (small_area < 0) return fail("loss targets: negative small_area");
    if (!(small_weight == small_weight)) return fail("loss targets: small_weight is not a number");
    if (!gt || !gauss || !targets || (n_gt > 0 && (!points || !area))) return fail("loss targets: null tensor");
    if (((uintptr_t)gt | (uintptr_t)gauss | (uintptr_t)targets | (uintptr_t)area) & 3) return fail("loss targets: a 32-bit tensor that is not 4-byte aligned");
    if ((uintptr_t)points & 7) return fail("loss targets: dev_points is not 8-byte aligned");
    if (losses_ws(c)) return -1;
    return launch_loss_targets(gt, batch, n_gt, c->cfg.height, c->cfg.width, sigma, small_area, small_weight, c->cfg.encode_legacy_f32 ? 1 : 0, gauss,
                               targets, points, area, c->lazy[WS_LOSSES].p, c->cfg.max_batch, (hipStream_t)stream);
}

int quber_losses(quber_ctx* c, const float* logits, int32_t n_planes, const float* targets, const uint8_t* explicit_maps, const quber_loss_spec* sp,
                 int32_t batch, double* out, void* stream) {
    if (check_batch(c, batch)) return -1;
    if (!sp || !logits || !targets || !out) return fail("losses: null argument");
    if (((uintptr_t)logits | (uintptr_t)targets) & 3) return fail("losses: a 32-bit tensor that is not 4-byte aligned");
    if ((uintptr_t)out & 7) return fail("losses: dev_out is not 8-byte aligned");
    if (!(sp->top_k > 0.0 && sp->top_k <= 1.0)) return fail("losses: top_k outside (0, 1]");
    if (sp->error_type < 0 || sp->error_type > 3) return fail("losses: error_type must be 0 (e3), 1 (e2), 2 (e33) or 3 (e32)");
    static const int classes[4] = {4, 2, 3, 2};
    const int ncls = classes[sp->error_type];
    if (n_planes < 4) return fail("losses: fewer than the 4 planes fg, centre, off_y, off_x");
    const int planes[2] = {sp->eee_mask_plane, sp->eee_boundary_plane}, kinds[2] = {sp->eee_mask_loss, sp->eee_boundary_loss};
    for (int h = 0; h < 2; ++h) {
        if (planes[h] < 0) continue;
        if (planes[h] < 4 || planes[h] + ncls > n_planes) return fail("losses: an error head's planes lie outside 4..n_planes");
        if (kinds[h] != 0 && kinds[h] != 1) return fail("losses: loss type must be 0 (dice) or 1 (cross_entropy)");
        if (!explicit_maps) return fail("losses: an error head needs dev_explicit");
    }
    const long HW = (long)c->cfg.height * c->cfg.width;
    const long k = sp->top_k == 1.0 ? HW : (long)(sp->top_k * (double)HW);          // int(top_k * numel): model.py:70
    if (k < 1) return fail("losses: top_k selects no pixel of this frame (the reference would return NaN)");
    if (losses_ws(c)) return -1;
    return launch_losses(logits, n_planes, targets, explicit_maps, *sp, ncls, k, batch, c->cfg.height, c->cfg.width, out, c->lazy[WS_LOSSES].p,
                         c->cfg.max_batch, (hipStream_t)stream);
}

int64_t quber_contingency_workspace_bytes(int32_t cap) { return (int64_t)contingency_ws_bytes(cap); }

int quber_label_contingency(const int32_t* pred, const int32_t* gt, int64_t n_pixels, int32_t cap, void* workspace,
                            void* stream) {
    if (!pred || !gt || !workspace || n_pixels < 1 || cap < 1 || cap > 1024) return fail("bad argument to quber_label_contingency");
    return launch_contingency(pred, gt, n_pixels, cap, workspace, (hipStream_t)stream);
}

int64_t quber_boundary_workspace_bytes(int32_t h, int32_t w, int32_t n_masks) {
    return (int64_t)boundary_ws_bytes(h, w, n_masks);
}

int quber_boundary_overlap(const int32_t* pred, const int32_t* gt, int32_t h, int32_t w, const int32_t* labels, int32_t n_pred,
                           int32_t n_gt, int32_t bound_pix, void* workspace, uint32_t* out, void* stream) {
    if (!pred || !gt || !labels || !workspace || !out || h < 1 || w < 1) return fail("bad argument to quber_boundary_overlap");
    return launch_boundary_overlap(pred, gt, h, w, labels, n_pred, n_gt, bound_pix, workspace, out, (hipStream_t)stream);
}

int64_t quber_eval_batch_workspace_bytes(int32_t batch, int32_t h, int32_t w, int32_t cap, int32_t with_boundary) {
    if (batch < 1 || h < 1 || w < 1 || cap < 1 || cap > 256) return 0;
    return (int64_t)eval_batch_ws_bytes(batch, h, w, cap, with_boundary);
}

int quber_eval_batch(const int32_t* pred, const int32_t* gt, int32_t batch, int32_t h, int32_t w, int32_t cap, int32_t bound_pix,
                     int32_t with_boundary, int32_t placement, void* workspace, void* out, void* stream) {
    if (!pred || !gt || !workspace || !out) return fail("quber_eval_batch: null pointer");
    if (((uintptr_t)pred & 3) || ((uintptr_t)gt & 3) || ((uintptr_t)workspace & 7) || ((uintptr_t)out & 7))
        return fail("quber_eval_batch: label maps must be 4-byte aligned, workspace and out 8-byte aligned");
    return launch_eval_batch(pred, gt, batch, h, w, cap, bound_pix, with_boundary, placement, workspace, out, (hipStream_t)stream);
}

int quber_munkres_batch(const double* score, const int32_t* rows, const int32_t* cols, int32_t batch, int32_t cap, int32_t placement,
                        void* workspace, int32_t* assign, int32_t* status, void* stream) {
    if (!score || !rows || !cols || !assign || !status) return fail("quber_munkres_batch: null pointer");
    if (((uintptr_t)score & 7) || ((uintptr_t)workspace & 7) || ((uintptr_t)rows & 3) || ((uintptr_t)cols & 3) || ((uintptr_t)assign & 3) ||
        ((uintptr_t)status & 3))
        return fail("quber_munkres_batch: misaligned pointer");
    return launch_munkres_batch(score, rows, cols, batch, cap, placement, reinterpret_cast<double*>(workspace), assign, cap, status, 1,
                                (hipStream_t)stream);
}

int quber_foreground_filter(const float* fg_logits, int32_t n_classes, int32_t fg_class, const uint8_t* masks,
                            int32_t batch, int32_t n_masks, int64_t hw, uint8_t* fg_mask, uint64_t* counts, void* stream) {
    if (!fg_logits || !fg_mask || batch < 1 || hw < 1 || n_classes < 2) return fail("bad argument to quber_foreground_filter");
    if (n_masks < 0 || n_masks > 65535) return fail("quber_foreground_filter: n_masks outside 0..65535");     // grid.y of the overlap kernel
    hipStream_t st = (hipStream_t)stream;
    int rc = launch_argmax_fg(fg_logits, batch, hw, n_classes, fg_class, fg_mask, st);
    if (rc || n_masks == 0) return rc;
    if (!masks || !counts) return fail("null masks / counts");
    return launch_mask_overlap(masks, fg_mask, batch, n_masks, hw, (unsigned long long*)counts, st);
}

int quber_foreground_overlap(const uint8_t* fg, int32_t fg_h, int32_t fg_w, const uint8_t* masks, int32_t batch, int32_t n_masks, int32_t h, int32_t w,
                             uint64_t* counts, void* stream) {
    return launch_fg_overlap(fg, fg_h, fg_w, masks, batch, n_masks, h, w, (unsigned long long*)counts, (hipStream_t)stream);
}

int quber_normalize_depth(const void* depth, int32_t is_float32, int64_t n_pixels, double min_val, double max_val,
                          uint8_t* out3, uint8_t* zero, void* stream) {
    if (!depth || !out3 || n_pixels <= 0) return fail("bad argument to quber_normalize_depth");
    if (!(max_val > min_val)) return fail("normalize_depth: max_val must exceed min_val");
    return launch_normalize_depth(depth, is_float32, n_pixels, min_val, max_val, out3, zero, (hipStream_t)stream);
}

int quber_inpaint_telea_u8(const uint8_t* host_img, const uint8_t* host_mask, int32_t h, int32_t w, int32_t radius,
                           uint8_t* host_out) {
    return inpaint_telea_u8_host(host_img, host_mask, h, w, radius, host_out);
}

int quber_inpaint_depth_u8(const uint8_t* host_depth3, int32_t h, int32_t w, int32_t kernel, uint8_t* host_out3) {
    return inpaint_depth_u8_host(host_depth3, h, w, kernel, host_out3);
}

int64_t quber_inpaint_depth_workspace_bytes(int32_t batch, int32_t h, int32_t w) { return (int64_t)inpaint_depth_ws_bytes(batch, h, w); }

int quber_inpaint_depth_device(const uint8_t* dev_depth3, int32_t batch, int32_t h, int32_t w, int32_t kernel, void* dev_workspace,
                               int64_t workspace_bytes, uint8_t* dev_out3, void* stream) {
    return launch_inpaint_depth(dev_depth3, batch, h, w, kernel, dev_workspace, (size_t)workspace_bytes, dev_out3, (hipStream_t)stream);
}

int quber_resize_u8(const uint8_t* src, int32_t src_h, int32_t src_w, int32_t channels, uint8_t* dst, int32_t dst_h,
                    int32_t dst_w, int32_t linear, void* stream) {
    if (!src || !dst) return fail("bad argument to quber_resize_u8");
    return launch_resize_u8(src, src_h, src_w, channels, dst, dst_h, dst_w, linear, (hipStream_t)stream);
}

int quber_debug_tensor(quber_ctx* c, const char* name, float** ptr, int32_t* dims4, int32_t* cs) {
    if (!c || !name) return fail("null argument");
    auto it = c->taps.find(name);
    if (it == c->taps.end()) return fail(std::string("no intermediate named '") + name + "'");
    *ptr = it->second.p;
    dims4[0] = it->second.B; dims4[1] = it->second.H; dims4[2] = it->second.W; dims4[3] = it->second.C;
    *cs = it->second.cs;
    return 0;
}
int32_t quber_debug_tensor_elem_size(quber_ctx* c, const char* name) {
    if (!c || !name) return 0;
    auto it = c->taps.find(name);
    return it == c->taps.end() ? 0 : it->second.es;
}

}  // extern "C"
