/* libquber_hip.so - C ABI of the MI355X (gfx950) QuBER mask-refinement hot path.
 *
 * The reference (gist-ailab/QuBER) has no native interface on this path: everything below the Python
 * predictor is stock torch ops.  The entry points therefore replace *Python call sites*; each one cites the
 * reference code it stands in for.  All `const T* dev_*` / `T* dev_*` arguments are DEVICE pointers
 * (e.g. torch.Tensor.data_ptr() of a ROCm tensor); every hot call is asynchronous on `stream`
 * (a hipStream_t passed as void*), allocates nothing, and never synchronises.  Return value: 0 on
 * success, negative on error with the text available from quber_last_error() (thread-local).
 * One context per GPU / stream; a context is not re-entrant.
 */
#ifndef QUBER_HIP_H
#define QUBER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct quber_ctx quber_ctx;

/* Architecture + post-processing constants; defaults mirror
 * configs/uoais-sim/instance-segmentation/seed77/mask-refiner-rgbd-concat-l2-gn-hf-b-fco-l3-b8.yaml on top of
 * Base-Mask-Refiner.yaml and maskrefiner/config.py:6-102 (see quber_default_config). */
typedef struct quber_config {
    int32_t height, width;           /* frame size; multiples of 16 */
    int32_t max_batch;               /* frames per call the workspace is sized for */
    int32_t max_instances;           /* initial masks per frame a call may carry (any number; > 254 are encoded in chunks) */
    int32_t resnet_depth;            /* MODEL.RESNETS.DEPTH: 50 | 101 | 152 */
    int32_t res5_dilation;           /* MODEL.RESNETS.RES5_DILATION (2) */
    int32_t backbone_fusion_layers;  /* MODEL.BACKBONE.NUM_FUSION_LAYERS (2) */
    int32_t head_fusion_layers;      /* MODEL.INS_EMBED_HEAD.NUM_FUSION_LAYERS (3) */
    int32_t error_classes;           /* ERROR_TYPE e3 -> 4 */
    int32_t gaussian_sigma;          /* predictor.py:246 (10) */
    int32_t nms_kernel;              /* PANOPTIC_DEEPLAB.NMS_KERNEL (7) */
    int32_t top_k;                   /* PANOPTIC_DEEPLAB.TOP_K_INSTANCE (200) */
    int32_t stuff_area;              /* PANOPTIC_DEEPLAB.STUFF_AREA (2048) */
    int32_t min_instance_area;       /* post_processing.py:145 (512) */
    int32_t label_divisor;           /* register_uoais_sim_panoptic.py:177-186 (1000) */
    int32_t with_network;            /* 0: only the encode / error-map / post-processing kernels are usable;
                                        1: the refiner network; 4: the Depth Seeding Network of UOIS-Net-3D (uois/src/networks.py
                                           UNetESP_Encoder / UNetESP_Decoder, uois/src/segmentation.py:72-127; feature_dim is read off the first
                                           convolution's weight; H and W multiples of 16; runs through quber_dsn_forward, not quber_forward;
                                           csrc/plan_dsn.hip, option key 53); 5: the Region Refinement Network of UOIS-Net-3D
                                           (uois/src/networks.py UNet_Encoder / UNet_Decoder, uois/src/segmentation.py:248-266; feature_dim
                                           is read off the first convolution's weight; height = width = the crop side, a multiple of 16;
                                           runs through quber_rrn_forward; csrc/plan_rrn.hip, option key 54); 3: the CGNet foreground network of the UOAIS base model
                                           (foreground_segmentation/cgnet.py, classes = 2, in_channel = 4; quber_forward then maps
                                           (bgr, depth) to [B][2][H][W] logits, H and W multiples of 8; csrc/plan_cgnet.hip, option key 52);
                                           2: the LMFFNet foreground network of the post-filter
                                           (foreground_segmentation/lmffnet.py; quber_forward then maps (bgr, depth) to
                                           3 class planes [B][3][H][W], dev_offsets is ignored) */
    float center_threshold;          /* PANOPTIC_DEEPLAB.CENTER_THRESHOLD (0.3) */
    float boundary_ratio;            /* explicit_error_estimation/util.py:92 dilation_ratio (0.01) */
    float pixel_mean[6];             /* MODEL.PIXEL_MEAN */
    float pixel_std[6];              /* MODEL.PIXEL_STD */
    /* prediction-head wiring (maskrefiner/modeling/mask_refiner/model.py:545-608, 738-762).
     * head ids: 0 foreground, 1 center, 2 offset, 3 eee_mask, 4 eee_boundary */
    int32_t eee_mask_on;             /* INS_EMBED_HEAD.EEE_MASK_ON */
    int32_t eee_boundary_on;         /* INS_EMBED_HEAD.EEE_BOUNDARY_ON */
    int32_t hierarchical;            /* INS_EMBED_HEAD.HIERARCHICAL_FUSION_ON */
    int32_t fusion_feat;             /* "feat" in INS_EMBED_HEAD.FUSION_TARGET */
    int32_t fusion_pred;             /* "pred" in INS_EMBED_HEAD.FUSION_TARGET */
    int32_t n_levels;                /* len(INS_EMBED_HEAD.HIERARCHY) */
    int32_t level_heads[5][5];       /* head ids per level, -1 padded */
    int32_t fusion_add;              /* MODEL.BACKBONE.FUSION_STRATEGY == "add" (0 = "concat") */
    int32_t streams;                 /* 2: rgb + depth streams (build_resnet_deeplab_rgbd_fusion_backbone); 1: single stream
                                        (build_resnet_deeplab_fusion_backbone: rgb-only or depth-only, pixel_mean[0..2]) */
    int32_t compute_dtype;           /* arithmetic of the convolutions: 0 = exact fp32 MFMA (default; the 1e-4 parity bar),
                                        3 = fp32-equivalent on the bf16 matrix pipe: every fp32 operand split into 3 bf16 terms,
                                        6 exact partial products per multiply, fp32 accumulation (dropped terms < 2^-26; same
                                        plan, same 1e-4 bar, 6/16 of the matrix time),
                                        2 = the fp16 data path (BASELINE.json configs[4] "fp16 MFMA path" stand-in): activations and
                                        packed weights fp16 in device memory, fp32 accumulation, fp32 norm statistics and logits;
                                        own tolerance (tests/test_gpu_loud_parity.py HALF_TOL),
                                        1 = bf16 operands on fp32 tensors (8x coarser) */
    int32_t encode_legacy_f32;       /* a1 offset arithmetic (predictor.py:345-346, `np.float64 scalar - float32 array`):
                                        0 = numpy >= 2 promotion (float64, rounded once; what the reference computes when run
                                        under this image's numpy 2.2, pinned by tests/golden/encode_*.npz);
                                        1 = numpy < 2 value-based casting (all float32; the reference's pinned numpy==1.23.1,
                                        INSTALL.md:14) - differs by 1 ulp on about a third of the mask pixels */
    int32_t convs_dim;               /* INS_EMBED_HEAD.CONVS_DIM (128): channels of the decoder's res3 / res2 stages, of the head
                                        convolutions and of the head-fusion stacks (model.py:610-651 decoder_channels); 128 | 256 */
    int32_t head_channels;           /* INS_EMBED_HEAD.HEAD_CHANNELS (32): channels in front of every 1x1 predictor
                                        (model.py:514-531, 413-422); 32 | 64 */
} quber_config;

/* logit planes produced by quber_forward: [fg, centre, off_y, off_x, eee_boundary x classes (if on), eee_mask x classes (if on)] */
#define QUBER_LOGIT_BASE 4

void quber_default_config(quber_config* cfg);
const char* quber_last_error(void);
const char* quber_version(void);

/* Build a context on the current HIP device.  Replaces MaskRefinerPredictor.__init__'s build_model(cfg)
 * (maskrefiner/predictor.py:209-229) minus its dataset / output-dir side effects. */
int quber_create(const quber_config* cfg, quber_ctx** out);
void quber_destroy(quber_ctx* ctx);

/* Weights: one call per state_dict entry, `name` being the detectron2-compatible key, `host`
 * a HOST pointer to `numel` contiguous fp32 values in torch's layout (OIHW for convs).  Replaces
 * DetectionCheckpointer.load (predictor.py:228-229).  quber_finalize_weights folds the frozen / eval
 * batch-norms into per-channel affines, re-lays the filters out for the implicit-GEMM kernel, uploads them and
 * fails (listing the first missing key) if the architecture needs a tensor that was not supplied. */
int quber_set_weight(quber_ctx* ctx, const char* name, const float* host, int64_t numel);
int quber_finalize_weights(quber_ctx* ctx);
/* number of tensors the configured architecture expects, and the i-th name / element count */
int quber_num_weights(quber_ctx* ctx);
int quber_weight_spec(quber_ctx* ctx, int index, const char** name, int64_t* numel);

/* a1 - initial masks -> (centre heat-map, off_y, off_x).  Replaces the numpy loop of
 * MaskRefinerPredictor.predict (maskrefiner/predictor.py:304-357).
 *   dev_masks u8 [B][N][H][W] (non-zero = inside)  ->  dev_out f32 [B][3][H][W] */
int quber_encode_initial_masks(quber_ctx* ctx, const uint8_t* dev_masks, int32_t batch, int32_t n_masks,
                               float* dev_out, void* stream);

/* a1 from a label map: dev_labels i32 [B][H][W] with values 0 (no instance) or 1..n_instances (<= 254), i.e. the n
 * non-overlapping masks (labels == i + 1); same output as quber_encode_initial_masks on those masks.  Values outside
 * 0..n_instances count as 0. */
int quber_encode_label_map(quber_ctx* ctx, const int32_t* dev_labels, int32_t batch, int32_t n_instances, float* dev_out,
                           void* stream);

/* device bytes the context owns (weights in kernel layout, activations, workspaces).  Everything is allocated by
 * quber_create / quber_finalize_weights; no hot call allocates. */
int64_t quber_workspace_bytes(quber_ctx* ctx);

/* a2 - explicit quadruple error maps.  Replaces masks_to_fg_mask / masks_to_boundary
 * (explicit_error_estimation/util.py:62-99) and the TP/TN/FP/FN logic of tools/ours/panoptic2eee.py:110-123.
 *   dev_init u8 [B][N][H][W], dev_gt u8 [B][Ng][H][W]  ->  dev_out u8 [B][2 (region,boundary)][4 (TP,TN,FP,FN)][H][W] */
int quber_explicit_error_maps(quber_ctx* ctx, const uint8_t* dev_init, int32_t n_init, const uint8_t* dev_gt,
                              int32_t n_gt, int32_t batch, uint8_t* dev_out, void* stream);

/* a3-a7 - the network.  Replaces MaskRefiner.forward up to the head outputs
 * (maskrefiner/modeling/mask_refiner/model.py:137-156, 244-250, 689-708).
 *   dev_bgr u8 [B][H][W][3], dev_depth u8 [B][H][W][3] (NULL when streams == 1: dev_bgr then carries the single
 *   image, rgb or depth), dev_offsets f32 [B][3][H][W]
 *   -> dev_logits f32 [B][4+classes][H][W]  (fg logit, centre, off_y px, off_x px, boundary-error logits) */
int quber_forward(quber_ctx* ctx, const uint8_t* dev_bgr, const uint8_t* dev_depth, const float* dev_offsets,
                  int32_t batch, float* dev_logits, void* stream);

/* quber_forward with a HIP-event pair around every launch group of the plan, on `stream` (synchronises it).
 *   kind_ms[3] / kind_launches[3]: summed device time and launch-group count of
 *   [0] implicit-GEMM convolutions, [1] GroupNorm (stats + apply), [2] everything else.  Benchmark use only. */
int quber_forward_profiled(quber_ctx* ctx, const uint8_t* dev_bgr, const uint8_t* dev_depth,
                           const float* dev_offsets, int32_t batch, float* dev_logits, void* stream,
                           double* kind_ms, int32_t* kind_launches);

/* Stage profile (benchmark use): every quber_* call made on `ctx` by this thread between begin and end brackets each of
 * its kernels with a HIP-event pair on the launch stream.  quber_profile_end synchronises `stream` and sums, per stage
 * name ("encode_reduce", "preprocess", "conv_gemm", "wino_input", "wino_gemm", "wino_output", "splitk_reduce",
 * "gn_apply", "upsample_logits", "post_nms", "post_group", "extract_masks", "errmaps_pack", ...): device milliseconds,
 * the stage's ALGORITHMIC bytes (every operand read / written once) and FLOPs, and the number of brackets. */
int quber_profile_begin(quber_ctx* ctx);
int quber_profile_end(quber_ctx* ctx, void* stream);
int quber_profile_num_stages(quber_ctx* ctx);
int quber_profile_stage(quber_ctx* ctx, int index, const char** name, double* ms, double* bytes, double* flops,
                        int32_t* launches);

/* a8-a11 - centre NMS/top-k, pixel grouping, 512-px merge, scores and boxes.  Replaces get_panoptic_segmentation
 * (maskrefiner/modeling/mask_refiner/post_processing.py:165-221) and the instance loop of model.py:313-356.
 *   dev_logits f32 [B][n_planes][H][W] (planes 0..3 used)
 *   -> dev_panoptic f32 [B][H][W]  labels {-1, 1000, 1001, ...}
 *      dev_count   i32 [B]         instances per frame
 *      dev_labels  f32 [B][top_k]  their labels, ascending, -1 padded
 *      dev_scores  f32 [B][top_k], dev_boxes f32 [B][top_k][4] (x0,y0,x1,y1)
 *      dev_centers i32 [B][top_k][2] (y,x) and dev_ncenters i32 [B]  (the surviving centre points) */
int quber_postprocess(quber_ctx* ctx, const float* dev_logits, int32_t n_planes, int32_t batch,
                      float* dev_panoptic, int32_t* dev_count, float* dev_labels, float* dev_scores,
                      float* dev_boxes, int32_t* dev_centers, int32_t* dev_ncenters, void* stream);

/* pred_masks of model.py:334 for the first `max_inst` labels of every frame:
 *   -> dev_masks u8 [B][max_inst][H][W] in {0,1} (all zero for slots beyond the frame's count) */
int quber_extract_masks(quber_ctx* ctx, const float* dev_panoptic, const float* dev_labels, int32_t batch,
                        int32_t max_inst, uint8_t* dev_masks, void* stream);

/* horizontal-flip test-time augmentation: one forward of 2B frames, originals in slots [0, B), their W-mirrors in [B, 2B).
 * The reference's driver builds MaskRefinerTTA for --refiner_model maskrefiner-tta (eval/un_eval_utils.py:78-81) but never
 * defines it; SemanticSegmentorWithTTA (maskrefiner/test_time_augmentation.py:72-95) runs the original and the flipped input,
 * flips the second sem_seg back and averages, and model.py:304-307 keeps a hook that hands centre and offset to that caller.
 *
 * Mirrors frames [0, batch) of each input into [batch, 2 * batch), in place; the caller fills the first half.
 *   dev_bgr u8 [2B][H][W][3], dev_depth u8 [2B][H][W][3] or null, dev_masks u8 [2B][n][H][W] (unused when n == 0).
 * The mirrored frame's initial-mask encoding is quber_encode_initial_masks on all 2B frames afterwards: a1 of the mirrored
 * masks, as predict() computes it for a mirrored frame (maskrefiner/predictor.py:304-348) - not a mirror of the
 * originals' offsets, which is not bit-equal. */
int quber_tta_flip_inputs(quber_ctx* ctx, uint8_t* dev_bgr, uint8_t* dev_depth, uint8_t* dev_masks, int32_t batch,
                          int32_t n_masks, void* stream);
/* The merge of the 2B full-resolution logits of quber_forward, plane by plane, in fp32:
 *   out[b][c][y][x] = (L[b][c][y][x] + s_c * L[B+b][c][y][W-1-x]) * 0.5f,  s_c = -1 for plane 3 (off_x), +1 otherwise
 *   dev_logits2 f32 [2B][n_planes][H][W] -> dev_out f32 [B][n_planes][H][W]; quber_postprocess then runs on dev_out. */
int quber_tta_merge(quber_ctx* ctx, const float* dev_logits2, int32_t n_planes, int32_t batch, float* dev_out,
                    void* stream);

/* The predicted error maps (the eee_boundary / eee_mask planes of quber_forward, plane order as at QUBER_LOGIT_BASE), decoded,
 * attributed and scored without leaving the device (csrc/errhead.hip).  All four work on a context created with with_network = 0;
 * every output is overwritten (the call clears what it accumulates into, on `stream`).
 *
 * Per-pixel class of one head.  Replaces the `argmax` of eval/eval_utils.py:308-328 and explicit_error_estimation/util.py:29-31;
 * exactly torch.argmax(logits[:, first_plane : first_plane + classes], dim=1): the first index wins ties, a NaN is the maximum.
 *   dev_logits f32 [B][n_planes][H][W], classes 2..4, n_planes >= first_plane + classes
 *   -> dev_classes u8 [B][H][W]; dev_hist u32 [B][classes] pixels per class (may be NULL).  Any H, W and alignment. */
int quber_error_decode(quber_ctx* ctx, const float* dev_logits, int32_t n_planes, int32_t first_plane, int32_t classes,
                       int32_t batch, uint8_t* dev_classes, uint32_t* dev_hist, void* stream);
/* Which initial masks carry which predicted class (no reference counterpart: the reference only paints the classes,
 * eval_utils.py:308-328; with the boundary head of an e3 model FP / (TP + FP) of a row is the share of the mask's own boundary
 * band the network rejects).
 *   dev_classes u8 [B][H][W], dev_masks u8 [B][n_masks][H][W] (non-zero = inside), n_masks 0..max_instances (0: no-op)
 *   -> dev_out u32 [B][n_masks][classes]: pixels of mask n with class c; overlapping masks each count their own pixels; a class
 *      value >= classes is counted nowhere */
int quber_error_mask_hist(quber_ctx* ctx, const uint8_t* dev_classes, const uint8_t* dev_masks, int32_t batch, int32_t n_masks,
                          int32_t classes, uint32_t* dev_out, void* stream);
/* Confusion table of a class map against the explicit maps.  Replaces compute_metrics' get_stats inputs
 * (explicit_error_estimation/util.py:29-54); the target class is the training target of
 * maskrefiner/modeling/mask_refiner/model.py:185-227.
 *   dev_explicit u8 [B][2][4][H][W]: the output of quber_explicit_error_maps; kind 0 = region (eee_mask), 1 = boundary (eee_boundary)
 *   error_type 0 = e3 (TP,TN,FP,FN -> 0,1,2,3), 1 = e2 (TP|TN -> 0, FP|FN -> 1), 2 = e33 (TP|TN -> 0, FP -> 1, FN -> 2),
 *              3 = e32 (FP -> 0, FN -> 1, TP / TN: no target); classes must be 4, 2, 3, 2 respectively
 *   -> dev_table u64 [B][classes + 1][classes]: row = target class (row `classes`: pixels without one), column = predicted class.
 *      Every frame's table sums to H * W provided every byte of dev_classes is < classes: a larger value is a caller error, such a
 *      pixel is counted nowhere (nothing is read or written out of bounds). */
int quber_error_score(quber_ctx* ctx, const uint8_t* dev_classes, const uint8_t* dev_explicit, int32_t kind, int32_t error_type,
                      int32_t classes, int32_t batch, uint64_t* dev_table, void* stream);
/* The picture of eval/eval_utils.py:308-328: class colours painted over the image.
 *   dev_bgr u8 [B][H][W][3], dev_classes u8 [B][H][W]; colorN: bits 0-7 B, 8-15 G, 16-23 R, bit 24 = paint class N
 *   -> dev_out u8 [B][H][W][3] (may be dev_bgr itself): the colour where the pixel's class has bit 24 set, the input elsewhere */
int quber_error_overlay(quber_ctx* ctx, const uint8_t* dev_bgr, const uint8_t* dev_classes, int32_t batch, uint32_t color0,
                        uint32_t color1, uint32_t color2, uint32_t color3, uint8_t* dev_out, void* stream);

/* Iterative refinement (csrc/iterate.hip): the refined label map of one pass fed back as the initial masks of the next without
 * leaving the device, and what the refinement did to the caller's masks.  No reference counterpart: the reference refines once
 * (maskrefiner/predictor.py:287-359).  All three work on a context created with with_network = 0, take any H, W and pointer
 * alignment (4 bytes for the 32-bit maps), use integer arithmetic only (exact, order-independent) and overwrite their outputs
 * (the call clears what it accumulates into, on `stream`).
 *
 * The label map of quber_postprocess as the input of quber_encode_label_map:
 *   dev_panoptic f32 [B][H][W], dev_labels f32 [B][top_k] (ascending), dev_count i32 [B] (read on the device; above top_k: top_k)
 *   -> dev_ids i32 [B][H][W]: 1 + j where j < count[b] is the first position of the pixel's value in labels[b][0 .. count[b]),
 *      0 when the value is not in that list (-1, or anything else).  The value is looked up, not offset: the list need not be
 *      consecutive and may hold `label_divisor` itself (the K = 0 "stuff blob" of post_processing.py:110-162).
 *   mirror != 0: dev_ids is [2B][H][W] and frame B + b receives the W-mirror, ids[B + b][y][x] = ids[b][y][W - 1 - x] (the
 *      test-time-augmentation pass: quber_encode_label_map then runs on all 2B frames); 2 * batch <= max_batch. */
int quber_relabel_panoptic(quber_ctx* ctx, const float* dev_panoptic, const float* dev_labels, const int32_t* dev_count,
                           int32_t batch, int32_t mirror, int32_t* dev_ids, void* stream);
/* Initial masks against a compact label map: which refined instance came from which initial mask, what was dropped.
 *   dev_masks u8 [B][n_masks][H][W] (non-zero = inside), n_masks 0..max_instances (0: only dev_area); dev_ids i32 [B][H][W],
 *   n_ids 0..254
 *   -> dev_table u32 [B][n_masks][n_ids + 1]: pixels of mask n whose id is j; dev_area u32 [B][n_ids + 1] (may be NULL): pixels
 *      whose id is j.  Overlapping masks each count their own pixels; a pixel whose id lies outside 0..n_ids is counted nowhere. */
int quber_overlap_masks(quber_ctx* ctx, const uint8_t* dev_masks, const int32_t* dev_ids, int32_t batch, int32_t n_masks,
                        int32_t n_ids, uint32_t* dev_table, uint32_t* dev_area, void* stream);
/* Two compact label maps against each other (successive passes):
 *   dev_a, dev_b i32 [B][H][W], n_a, n_b 0..254
 *   -> dev_table u32 [B][n_a + 1][n_b + 1]: pixels with a == i and b == j; out-of-range ids are counted nowhere.
 * The two maps describe the same segmentation iff every row and every column holds at most one non-zero cell and row 0 and
 * column 0 hold none besides [0][0].  (quber_label_contingency below is one frame per call, compacts arbitrary 16-bit labels and
 * needs a workspace; this one takes compact ids and a batch.) */
int quber_overlap_ids(quber_ctx* ctx, const int32_t* dev_a, const int32_t* dev_b, int32_t batch, int32_t n_a, int32_t n_b,
                      uint32_t* dev_table, void* stream);

/* Connected-component clean-up of the refined instances (csrc/cleanup.hip).  Nearest-centre grouping does not make an instance
 * connected: stray votes leave detached specks, a dip of the foreground logit leaves a void hole.  The competing refiners of the
 * reference clean their masks on the host - largest_connected_component(mask, connectivity=4) (eval/utilities.py:726-748, the UOIS
 * path) and remove_small_regions(mask, 300, "holes") (eval/refiner_model.py:526-549, the SAM path); these two do it on the device.
 * Both work on a context created with with_network = 0, take any H, W and 4-byte alignment, allocate nothing (the workspace is part of
 * the context, sized for max_batch), use integer arithmetic for the maps (exact, order-independent) and overwrite their outputs.
 *
 *   dev_ids i32 [B][H][W], in place: 0 = void, 1..n_ids = instance (n_ids 0..254); a value outside 0..n_ids counts as 0 and is
 *   written back as 0.  Frames never interact.  connectivity c = 4 or 8; keep_largest 0 or 1; the two areas >= 0.
 *   Step 1, islands.  For every i >= 1 the c-connected components of {ids == i}, ordered by their first pixel in raster order; the
 *     largest has the most pixels, the earlier one among equals.  keep_largest: every other component becomes 0.  Otherwise every
 *     component of fewer than min_island_area pixels becomes 0, except that the largest always stays (min_island_area = 0: nothing
 *     is removed).
 *   Step 2, holes, only if max_hole_area > 0, on the map step 1 left.  A c-connected component of {ids == 0} takes the id i iff it
 *     has fewer than max_hole_area pixels and its c-neighbours outside itself (inside the frame) all carry i.  One that touches the
 *     frame edge can be filled; one that borders two instances, or none, cannot.  A removed speck of j inside i ends up as i.
 *   Every instance keeps at least one pixel; the operation is idempotent.
 *   -> dev_report u32 [B][n_ids + 1][4] (may be NULL), row i >= 1: components found in step 1, pixels removed, pixels gained by
 *      filling, final area; row 0: void components examined in step 2, 0, pixels filled in all, final void area. */
int quber_cleanup_ids(quber_ctx* ctx, int32_t* dev_ids, int32_t batch, int32_t n_ids, int32_t connectivity, int32_t keep_largest,
                      int32_t min_island_area, int32_t max_hole_area, uint32_t* dev_report, void* stream);
/* The same on the outputs of quber_postprocess, with no host read and no synchronisation: the label map is compacted on the device
 * (the lookup of quber_relabel_panoptic, dev_count read there), cleaned with n_ids = top_k and written back - a removed pixel becomes
 * -1, a filled one takes the instance's label - and scores and boxes are recomputed over the cleaned masks exactly as quber_postprocess
 * defines them (mean of sigmoid(fg) over the mask in float64, times the centre plane at the truncated centre of mass; box = min /
 * max + 1).  Labels, count and the centre list do not change (every instance keeps a pixel); the 512-px filter is not applied again.
 *   dev_logits f32 [B][n_planes][H][W] (planes 0, 1 used); dev_panoptic f32 [B][H][W] in / out; dev_labels f32 [B][top_k], dev_count
 *   i32 [B] in; dev_scores f32 [B][top_k], dev_boxes f32 [B][top_k][4] out; dev_report u32 [B][top_k + 1][4] (may be NULL). */
int quber_cleanup_postprocess(quber_ctx* ctx, const float* dev_logits, int32_t n_planes, int32_t batch, float* dev_panoptic,
                              const float* dev_labels, const int32_t* dev_count, float* dev_scores, float* dev_boxes,
                              int32_t connectivity, int32_t keep_largest, int32_t min_island_area, int32_t max_hole_area,
                              uint32_t* dev_report, void* stream);

/* Perturbed initial masks (csrc/perturb.hip): the reference's perturb_seg (tools/ours/perturbation_utils.py:39-71) - a random walk of
 * erosions and dilations on random sub-rectangles of a mask, until its IoU with the mask it started from falls below a target - on
 * masks that are already on the device, one workgroup per mask, the mask kept on chip for the whole walk.  The number of random draws
 * per operation does not depend on the data: the host draws the walk (quber_amd/perturb.py: perturb_program, the reference's order of
 * draws) and this call executes it.  The numpy statement of what it computes is tests/test_perturb_cpu.py: perturb_np.
 *   dev_masks u8 [B][n_masks][H][W] in; seg = mask > 127 is what is perturbed, g = mask != 0 what the IoU is taken against
 *   dev_programs i32 [B][n_masks][n_ops][8], rows (lx, ly, lw, lh, clear, dilate, size, choice); n_ops a multiple of ops_per_round
 *     (the reference: 4 operations per round, 250 rounds).  An operation: if clear, pixel (int((ly + lh) / 2), int((lx + lw) / 2))
 *     becomes 0; then seg[ly:lh, lx:lw] is replaced by its dilation (dilate != 0) or erosion with the structuring element
 *     cv::getStructuringElement gives for choice 1 (rectangle size x size), 2, 3, 4 (ellipse of width x height = size x size,
 *     size x size/2, size/2 x size), computed INSIDE the rectangle: beyond it a dilation sees 0 and an erosion 1 (OpenCV's default
 *     border on an isolated sub-matrix); dst(x, y) = max / min over the set (i, j) of src(x + j - kw/2, y + i - kh/2).
 *     Rectangles are clipped to the frame, sizes clamped to 1..15 (a half size to >= 1), any other choice is a rectangle: no program
 *     can write outside its mask.
 *   dev_iou_targets f64 [B][n_masks]: after every round iou = (|seg & g| + 1e-6) / (|seg | g| + 1e-6) in float64; the walk of a mask
 *     stops after the first round with iou < target.  H <= 2 or W <= 2: no round (perturb_seg's "rare case").
 *   -> dev_out u8 [B][n_masks][H][W], 0 / 255, any alignment; must not overlap dev_masks (error)
 *   -> dev_report u32 [B][n_masks][4] (may be NULL): rounds executed, |seg & g|, |seg | g|, |seg| after the last executed round.
 * placement: where the three bit planes (seg, scratch, g; rows padded to 32-bit words) live - 1 = LDS, an error when
 * 12 * H * ceil(W / 32) + 512 bytes exceed the 160 KB a workgroup may declare (640 x 480: 113 KB); 2 = a per-mask workspace in device
 * memory, any frame size; 0 = LDS when it fits.  Both compute the same bits.  The device-memory workspace (12 * H * ceil(W / 32)
 * bytes per mask) is not part of quber_create: the first call that needs it (and one that needs a larger one) allocates it, so that
 * call is not capturable into a graph; later calls are.  No host copy, no memset node; outputs are overwritten.  Works on a context
 * created with with_network = 0; n_masks is not bounded by max_instances. */
int quber_perturb_masks(quber_ctx* ctx, const uint8_t* dev_masks, int32_t batch, int32_t n_masks, const int32_t* dev_programs,
                        int32_t n_ops, int32_t ops_per_round, const double* dev_iou_targets, uint8_t* dev_out, uint32_t* dev_report,
                        int32_t placement, void* stream);

/* Mask NMS (csrc/masknms.hip): scored, overlapping, possibly duplicated initial masks made disjoint on the device - the reference's
 * nms + combine_masks_with_NMS, which it runs on the host in numpy at eval/refiner_model.py:683-740, eval/base_model.py:1027-1086 and
 * eval/base_model.py:1154-1190 (one full-frame np.multiply + np.sum per pair of masks).  The numpy statement of what this call computes
 * is tests/test_masknms_cpu.py: mask_nms_np; INTEGRATION.md "Overlapping initial masks" has it in words.
 *   dev_masks u8 [B][n_masks][H][W] in (non-zero = inside), dev_scores f32 [B][n_masks] in; a mask whose score is NaN is absent (never
 *     visited, never kept, never a source): the padding of a frame that has fewer masks than n_masks
 *   inter[i][j] = pixels inside both masks, area[i] = inter[i][i].  Masks are visited by score, descending, among equal scores the
 *     higher index first; a visited mask that is still alive is kept and every later alive j stays alive iff
 *     inter / ((area_i + area_j) - inter) <= thresh, evaluated in float32 in that order (a NaN - two empty masks - suppresses).
 *   The survivors are painted into one map, later over earlier, in the order (area ascending, visit position ascending) for
 *     on_top = 0 ("large", the reference) or in the reverse of it for on_top = 1 ("small"); id = 1 + position in that order.
 *   -> dev_out_masks u8 [B][n_masks][H][W]: map == id for the ids still visible, in ascending id, 0 / 255, zero planes behind count.
 *      May be dev_masks itself (only the first launch reads the input); any other overlap is an error.
 *   -> dev_ids i32 [B][H][W]: 0 or the 1-based index of the output mask that owns the pixel
 *   -> dev_source i32 [B][n_masks]: the input index of each output mask, -1 behind count
 *   -> dev_out_scores f32 [B][n_masks]: the output masks' scores, 0 behind count
 *   -> dev_report i32 [B][4]: count, kept (NMS survivors, before hidden ones drop out), 0, 0
 * Every output is overwritten by every call.  n_masks <= min(max_instances, 1024); H * W <= 2^24 (counts are compared in float32).
 * Launches (pack, zero, gram, select, paint, compaction, write) on `stream`; no host copy, no synchronisation, no memset node.  The
 * workspace (bit planes, pair table, rank map, per-frame tables, sized for max_batch x min(max_instances, 1024) masks) is not part of
 * quber_create: the FIRST call with n_masks > 0 allocates it and keeps it (quber_workspace_bytes counts it from then on), so that
 * call is not capturable into a graph; later calls are.  Works on a context created with with_network = 0. */
int quber_mask_nms(quber_ctx* ctx, const uint8_t* dev_masks, const float* dev_scores, int32_t batch, int32_t n_masks, float thresh,
                   int32_t on_top, uint8_t* dev_out_masks, int32_t* dev_ids, int32_t* dev_source, float* dev_out_scores,
                   int32_t* dev_report, void* stream);

/* Scene-level perturbation (csrc/scene.hip): the instance list of a frame degraded the way the reference builds the initial masks its
 * checkpoints were trained on (tools/ours/perturbate_masks.py:101-205, run there on the host with one full-frame numpy pass per pair of
 * masks) - false positives and over- / under-segmentations from a pool of proposals, merging of masks within ten pixels, splits along
 * an axis-aligned line, deletions.  The host draws every random decision (quber_amd/scene.py: scene_draws) and this call executes
 * them.  The numpy statement of what it computes is tests/test_scene_cpu.py: scene_perturb_np; INTEGRATION.md "Scene-level
 * perturbation" has it in words.
 *   dev_gt u8 [B][n_gt_rows][H][W], dev_props u8 [B][n_prop_rows][H][W] in (non-zero = inside; NULL with zero rows);
 *   dev_n_gt, dev_n_prop i32 [B]: the rows of each frame that exist (clamped to the row counts); the rows behind them are never read
 *   dev_fp_act, dev_gs_act u8 [B][n_prop_rows]; dev_merge_act, dev_split_act, dev_delete_act u8 [B][max_masks];
 *   dev_split_try i32 [B][max_masks][10][4], rows (x1, y1, axis, side), x1 / y1 clamped to the frame
 *   lim = (double)(W * H) * min_mask_ratio; iou(A, B) = (|A n B| + 1e-6) / (|A u B| + 1e-6) in float64.  The list starts empty:
 *   1. proposal q (ascending) is appended as a false positive when fp_act[q], not (|Q| < lim or |Q| > 2.0 * the largest ground truth's
 *      area, 0 without ground truth) and max_g iou(G_g, Q) < 0.3 (the maximum starts at 0);
 *   2. ... as an over- / under-segmentation when gs_act[q], |Q| >= lim and max_g iou(G_g, Q) > 0.3;
 *   3. ground truth g (ascending) is appended when the maximum over the entries E of 1-2 of (|G n E| + 1e-6) / ((|G u E| - |G n E|) + 1e-6)
 *      is < 0.3 (the symmetric difference: the reference's uint8 sum of a 0 / 1 and a 0 / 255 mask wraps);
 *   4. touch(a, b) = dilate10(L_a) meets L_b, dilate10(E)(y, x) = OR over i, j in 0..9 of E(y + i - 5, x + j - 5); every slot starts
 *      as its own member set; for idx1 ascending with merge_act[idx1]: A = S[idx1]; for idx2 != idx1 ascending: if some a in A and b
 *      in S[idx2] touch, S[idx1] = A u S[idx2] (replaced, not accumulated) and S[idx2] = {}.  Every entry becomes the union of its
 *      members' planes; entries without a pixel are removed, the order is kept;
 *   5. for idx ascending (the entries of step 4 only) with split_act[idx]: the first of its ten attempts for which 255.0 * |E \ C| >= lim
 *      and 255.0 * |E n C| >= lim, C = rows [y1, H - 1) (axis 0, side 0), rows [0, y1) (0, 1), columns [x1, W - 1) (1, 0), columns
 *      [0, x1) (1, 1): the entry becomes E \ C and E n C is appended;
 *   6. the entries idx of the list as it stands with delete_act[idx] are dropped, the order is kept.
 *   An append that would make the list longer than max_masks is not performed (in 5: the whole split) and counted in `dropped`.
 *   -> dev_out_masks u8 [B][max_masks][H][W], 0 / 255, zero planes behind count; any alignment
 *   -> dev_info i32 [B][max_masks][4]: kind (0 ground truth, 1 false positive, 2 over- / under-segmentation), the source index of the
 *      slot's own origin, the number of members, split (0 none, 1 the kept half, 2 the cut-off half); zero rows behind count
 *   -> dev_report i32 [B][8]: count, n_fp, n_gs, ground truths kept, absorbed, splits, deleted, dropped
 * Every output is overwritten by every call.  n_gt_rows + n_prop_rows <= 256 and 1 <= max_masks <= 256 (anything else is an error);
 * any H and W up to 2^30 pixels.  Launches (zero, pack, gram, select, dilate, touch, merge, compose, decide, write) on `stream`; no host
 * copy, no synchronisation, no memset node.  The workspace (bit planes, tables, prefix sums) is not part of quber_create: the first
 * call allocates it for its batch, row counts and max_masks and keeps it, a call that needs a larger one replaces it
 * (quber_workspace_bytes counts it); such a call is not capturable into a graph, the others are.  Works on a context created with
 * with_network = 0; the row counts are not bounded by max_instances. */
int quber_scene_perturb(quber_ctx* ctx, const uint8_t* dev_gt, const uint8_t* dev_props, const int32_t* dev_n_gt, const int32_t* dev_n_prop,
                        int32_t batch, int32_t n_gt_rows, int32_t n_prop_rows, int32_t max_masks, double min_mask_ratio,
                        const uint8_t* dev_fp_act, const uint8_t* dev_gs_act, const uint8_t* dev_merge_act, const uint8_t* dev_split_act,
                        const int32_t* dev_split_try, const uint8_t* dev_delete_act, uint8_t* dev_out_masks, int32_t* dev_info,
                        int32_t* dev_report, void* stream);

/* COCO AP, the per-frame half (csrc/cocoap.hip): computeIoU + evaluateImg of the published COCOeval and bbIou / rleIou of its maskApi.c for
 * ONE category, which the reference runs on the host through pycocotools (train_net.py:57 COCOEvaluator(use_fast_impl=False),
 * maskrefiner/evaluation/instance_evaluation.py) on the masks, scores and boxes of model.py:318-356.  The numpy statement of what this call
 * computes is tests/test_cocoap_cpu.py: coco_eval_img_np; DESIGN.md "COCO AP" has it in words.  accumulate / summarize run on the host
 * (quber_amd/eval/coco_ap.py) on the records below.
 *   dev_dt u8 [B][n_dt][H][W] (non-zero = inside), dev_scores f32 [B][n_dt]; a detection whose score is NaN is absent (never ranked): the
 *     padding of a frame with fewer detections.  dev_gt u8 [B][n_gt][H][W], dev_gt_flags u8 [B][n_gt]: bit 0 = crowd, bit 1 = ignore, 0xFF =
 *     absent.  dev_gt_area f64 [B][n_gt] or NULL: the ground-truth areas to use; an entry that is NaN, like NULL, means the computed one.
 *   iou_type 0 = segm: i = pixels in both masks, da / ga = pixels in each; iou = 0 if i == 0, else i / da for a crowd, else
 *     i / (da + ga - i), integers converted to float64 and divided once.  Areas: da, ga.
 *   iou_type 1 = bbox: dev_dt_boxes f64 [B][n_dt][4], dev_gt_boxes f64 [B][n_gt][4] = x, y, w, h; either may be NULL - the tight box of
 *     each mask (x0, y0, x1 + 1 - x0, y1 + 1 - y0; zeros for an empty mask) - and with both given the mask pointers may be NULL.
 *     w = min(dx + dw, gx + gw) - max(dx, gx), h likewise, 0 if w <= 0 or h <= 0; i = w h; u = crowd ? dw dh : dw dh + gw gh - i; i / u in
 *     float64, every operation rounded on its own.  Areas: dw dh, gw gh.
 *   dev_iou_thrs f64 [n_thrs], dev_area_rng f64 [n_rng][2]: the host's constants, bit for bit.
 *   The detections are ranked by score, descending, among equal scores the lower index first; the first 100 count.  Per area range
 *     gi[g] = ignore or crowd or area_g outside [lo, hi]; gorder = the stable order of gi.  Per threshold t the ranked detections are
 *     matched in order: best = min(t, 1 - 1e-10); walking gorder, a ground truth that is matched and no crowd is skipped, the walk stops at
 *     the first ignored one once a counting one is held, iou < best is skipped, anything else replaces the held one (equal replaces: the
 *     later wins).  A match sets dtm, dtIg = gi of the match; an unmatched detection is ignored iff its area is outside [lo, hi].
 *   -> dev_counts i32 [B][2]: n_top (<= 100), n_gt_present
 *   -> dev_order i32 [B][100]: the input index of every rank, -1 behind n_top;  dev_out_scores f32 [B][100], 0 behind n_top
 *   -> dev_dt_area f64 [B][100] in rank order, 0 behind n_top;  dev_gt_area_used f64 [B][n_gt], 0 for an absent one
 *   -> dev_iou f64 [B][100][n_gt]: rank x input ground truth; 0 behind n_top and for an absent ground truth
 *   -> dev_dtm, dev_dtig u8 [B][n_rng][n_thrs][100], 0 behind n_top
 *   -> dev_gi u8 [B][n_rng][n_gt]: 0 counts, 1 ignored, 2 absent;  dev_gorder i32 [B][n_rng][n_gt]: input indices, the absent ones last
 * Every output byte is written by every call.  n_dt <= 1024, n_gt <= 1024 (neither is bounded by max_instances), n_thrs <= 16,
 * n_rng <= 8: anything beyond is an error, never truncated.  Launches (rank, zero, pack + gram | boxes, iou, gorder, match) on `stream`; no
 * host copy, no synchronisation, no memset node.  The workspace (bit planes of 100 + n_gt masks per frame, pair table, areas, boxes) is not
 * part of quber_create: the first call allocates it and a call that needs a larger one replaces it (quber_workspace_bytes counts it), so
 * such a call is not capturable into a graph; later calls are.  Works on a context created with with_network = 0. */
int quber_coco_match(quber_ctx* ctx, const uint8_t* dev_dt, const float* dev_scores, const double* dev_dt_boxes, int32_t n_dt,
                     const uint8_t* dev_gt, const uint8_t* dev_gt_flags, const double* dev_gt_area, const double* dev_gt_boxes, int32_t n_gt,
                     int32_t batch, int32_t iou_type, const double* dev_iou_thrs, int32_t n_thrs, const double* dev_area_rng, int32_t n_rng,
                     int32_t* dev_counts, int32_t* dev_order, float* dev_out_scores, double* dev_dt_area, double* dev_gt_area_used,
                     double* dev_iou, uint8_t* dev_dtm, uint8_t* dev_dtig, uint8_t* dev_gi, int32_t* dev_gorder, void* stream);

/* Boundary AP, the per-frame half (csrc/cocoap.hip, csrc/boundaryap.hip): quber_coco_match with iou_type 0 under Boundary IoU (Cheng et al.;
 * mask_to_boundary and COCOeval.computeBoundaryIoU of the published boundary-iou-api, restated - parity with that package is argued, not
 * pinned by a test, as parity with pycocotools is).  The numpy statement is tests/test_boundary_ap_cpu.py: mask_boundary_np, boundary_iou_np,
 * coco_frame_boundary_np; DESIGN.md "Boundary AP" has it in words.
 *   boundary(m) = m & ~erode_d(m), d = dilation: d iterations of a 3 x 3 erosion with zeros outside the frame - a pixel survives the
 *     erosion iff the whole (2d + 1) x (2d + 1) square around it lies inside the frame and inside m.  1 <= dilation <= 64; anything else is an
 *     error, never clamped.  The caller derives it from the frame: max(1, round(0.02 * sqrt(H H + W W))) (coco_ap.boundary_dilation).
 *   mask iou: exactly iou_type 0.  boundary iou: the same expression on the boundaries - i_b = pixels in both boundaries, db / gb = pixels of
 *     each; 0 if i_b == 0, else i_b / db for a crowd, else i_b / (db + gb - i_b).  iou = min(mask iou, boundary iou).  The areas - dev_dt_area,
 *     dev_gt_area_used and with them the area ranges - stay the MASK areas; ranking, gi / gorder, matching and the records are unchanged.
 *   The arguments and outputs are quber_coco_match's, without iou_type and the boxes; dev_iou receives the minimum;
 *   -> dev_mask_iou, dev_boundary_iou f64 [B][100][n_gt], either may be NULL (not wanted): the two ratios on their own, 0 behind n_top and for an
 *      absent ground truth.
 * Every output byte is written by every call; the limits are quber_coco_match's and are errors, never truncated.  Launches (rank, zero, pack,
 * boundary, gram, gram, iou, gorder, match) on `stream`; no host copy, no synchronisation, no memset node, no floating-point atomics.  The
 * workspace is quber_coco_match's, larger by the boundary planes, the second pair table and the boundary areas (lazy, counted by
 * quber_workspace_bytes; the call that makes or grows it is not capturable into a graph).  Works on a context created with with_network = 0. */
int quber_coco_match_boundary(quber_ctx* ctx, const uint8_t* dev_dt, const float* dev_scores, int32_t n_dt, const uint8_t* dev_gt,
                              const uint8_t* dev_gt_flags, const double* dev_gt_area, int32_t n_gt, int32_t batch, int32_t dilation,
                              const double* dev_iou_thrs, int32_t n_thrs, const double* dev_area_rng, int32_t n_rng, int32_t* dev_counts,
                              int32_t* dev_order, float* dev_out_scores, double* dev_dt_area, double* dev_gt_area_used, double* dev_iou,
                              double* dev_mask_iou, double* dev_boundary_iou, uint8_t* dev_dtm, uint8_t* dev_dtig, uint8_t* dev_gi,
                              int32_t* dev_gorder, void* stream);

/* The boundary kernel of quber_coco_match_boundary on its own (overlays, tests): dev_masks u8 [n][h][w] (non-zero = inside; any frame size,
 * not only the context's) -> dev_out u8 [n][h][w] of 0 / 1 = boundary(m) as above, dev_area i32 [n][2] = (pixels of the mask, pixels of its
 * boundary).  1 <= dilation <= 64 and h w <= 2^30, else an error that writes nothing.  dev_out may be dev_masks itself.  Launches (zero, pack,
 * boundary, unpack) on `stream`; the bit planes live in the lazy workspace of quber_coco_match (the call that makes or grows it is not
 * capturable into a graph).  Works on a context created with with_network = 0. */
int quber_op_mask_boundary(quber_ctx* ctx, const uint8_t* dev_masks, int32_t n, int32_t h, int32_t w, int32_t dilation, uint8_t* dev_out,
                           int32_t* dev_area, void* stream);

/* Mean-shift clustering of pixel embeddings into initial masks (csrc/meanshift.hip): the UCN base model's clustering_features ->
 * mean_shift_smart_init (select_smart_seeds, seed_hill_climbing_ball, connected_components) and filter_labels_depth of the reference
 * (eval/base_model.py:622-840 and :34-47, cosine metric), which it runs as torch and Python loops per frame.  The numpy statement of
 * what these calls compute is tests/test_meanshift_cpu.py: meanshift_np, filter_depth_np; INTEGRATION.md "Initial masks from pixel
 * embeddings" has it in words.  dot(a, b) below is accumulated in float32 in channel order 0..63, multiply and add rounded separately;
 * dist(a, b) = 0.5 * (1 - dot(a, b)).
 *   dev_emb f32 [B][channels][H][W], channels == 64 (anything else is an error); X[p] = the 64 values of pixel p.
 * quber_meanshift_seeds: dev_first i32 [B], the first seed of every frame (clamped to the frame)
 *   -> dev_indices i32 [B][num_seeds]: farthest-first - seed k + 1 is the FIRST index of the maximum over p of
 *      min over j <= k of dist(X[p], X[seed j]).  One launch per seed.  1 <= num_seeds <= min(128, H * W).
 * quber_meanshift_climb: dev_seeds f32 [B][num_seeds][64] in and out; with dev_indices (may be NULL) it is first set to the pixels they
 *   name.  iters times: Z = normalize(exp(kappa Z X^T) X), on the float32 matrix pipe with float32 accumulation in a fixed order; the
 *   partial sums of the blocks are added in float64 in block order (no floating-point atomics: two calls give the same bits, and a
 *   frame's result does not depend on the batch it is in).  0 <= iters <= 1000, 0 <= kappa <= 64: the weights exp(kappa cos) are summed in
 *   float32 (as in the reference), and exp(64) over a frame of 2^24 pixels is the most that stays finite.
 * quber_meanshift_link -> dev_seed_labels i32 [B][num_seeds]: connected_components as written - in seed order, an unlabelled seed i
 *   labels every seed j with dist(Z[j], Z[i]) <= epsilon: with the mode of the labels already there (the smallest among equal counts)
 *   if there is one, else with the next new label.  A seed outside its own ball (a zero vector) stays -1 and uses up a label.
 * quber_meanshift_assign: every pixel takes the label of the first seed at minimum dist; num = distinct seed labels, the first largest
 *   of the labels 0 .. num - 1 swaps with label 0; with dev_depth_z (f32 [B][H][W], may be NULL = no filter) a label > 0 is dropped
 *   when float32(its pixels with z > 0) / float32(its pixels) < depth_threshold; the survivors are numbered 1..count by ascending label,
 *   those behind n_masks are dropped.  A pixel whose label is -1 belongs to no mask.
 *   -> dev_ids i32 [B][H][W] (0, 1..count), dev_masks u8 [B][n_masks][H][W] (ids == k + 1 as 0 / 255, zero planes behind count; may be
 *      NULL when n_masks == 0), dev_report i32 [B][4]: count, clusters before the filter, dropped by depth, 1 if truncated to n_masks.
 *      n_masks <= 254.
 * quber_meanshift_cluster: seeds -> climb -> link -> assign on `stream`, with every intermediate result as an output.
 * Every output is overwritten by every call.  H * W <= 2^24.  No host copy, no synchronisation, no memset node, no cooperative launch.
 * The workspace (seed slots, histograms, running minimum, raw labels, block partials: up to 8 MB + 8 H W bytes per frame of max_batch)
 * is not part of quber_create: the FIRST call of any of these entries (quber_meanshift_link excepted, which needs none) allocates it and
 * keeps it (quber_workspace_bytes counts it from then on), so that call is not capturable into a graph; later calls are.  Works on a
 * context created with with_network = 0. */
int quber_meanshift_seeds(quber_ctx* ctx, const float* dev_emb, int32_t batch, int32_t channels, const int32_t* dev_first, int32_t num_seeds,
                          int32_t* dev_indices, void* stream);
int quber_meanshift_climb(quber_ctx* ctx, const float* dev_emb, int32_t batch, int32_t channels, const int32_t* dev_indices, int32_t num_seeds,
                          float kappa, int32_t iters, float* dev_seeds, void* stream);
int quber_meanshift_link(quber_ctx* ctx, const float* dev_seeds, int32_t batch, int32_t num_seeds, float epsilon, int32_t* dev_seed_labels,
                         void* stream);
int quber_meanshift_assign(quber_ctx* ctx, const float* dev_emb, int32_t batch, int32_t channels, const float* dev_seeds,
                           const int32_t* dev_seed_labels, int32_t num_seeds, const float* dev_depth_z, float depth_threshold, int32_t n_masks,
                           int32_t* dev_ids, uint8_t* dev_masks, int32_t* dev_report, void* stream);
int quber_meanshift_cluster(quber_ctx* ctx, const float* dev_emb, int32_t batch, int32_t channels, const int32_t* dev_first, int32_t num_seeds,
                            float kappa, int32_t iters, float epsilon, const float* dev_depth_z, float depth_threshold, int32_t n_masks,
                            int32_t* dev_indices, float* dev_seeds, int32_t* dev_seed_labels, int32_t* dev_ids, uint8_t* dev_masks,
                            int32_t* dev_report, void* stream);

/* Gaussian mean shift of 3-D centre votes into initial masks, and the initial mask processing (csrc/gms.hip): the UOIS-Net-3D base
 * model's DSNWrapper.cluster -> GaussianMeanShift.mean_shift_smart_init (uois/src/segmentation.py:129-187, uois/src/cluster.py) and
 * UOISNet3D.process_initial_masks (segmentation.py:425-491), which the reference runs as torch, numpy and OpenCV loops per frame on the
 * host.  The numpy statement of what these calls compute is tests/test_gms_cpu.py: gms_np, imp_np; INTEGRATION.md "Initial masks from
 * centre votes" has it in words.  dist(a, b) = sqrt((dx dx + dy dy) + dz dz) in float32, every operation rounded separately, the
 * square root correctly rounded.
 *   dev_votes f32 [B][3][H][W]: xyz + offsets, finite (the caller's duty: nothing on the device checks it); dev_fg u8 [B][H][W]: non-zero
 *   marks an object pixel.  P = the fg pixels in row-major order, n = |P|; Xs = P[::subsample], n_sub = ceil(n / subsample);
 *   S = min(num_seeds, n_sub): the seeds the frame really has.  1 <= num_seeds <= 256, 1 <= subsample <= 64.
 *   dev_info i32 [B][3] = n, n_sub, S: written by quber_gms_seeds; read by climb / link / assign, where NULL means S = num_seeds.
 * quber_gms_seeds: dev_first i32 [B] (clamped to 0..n_sub - 1), dev_draws u32 [B][num_seeds] (32-bit draws r_k; entry 0 is not read)
 *   -> dev_indices i32 [B][num_seeds] into Xs, -1 behind S.  Seed 0 is first.  For k >= 1, with mind[p] = min over j < k of
 *      dist(Xs[p], Xs[seed j]), q[p] = min(floor(float64(mind[p]) * 2^20), 2^31 - 1), total = sum q (exact in 64 bits) and
 *      t = floor(r_k * total / 2^32): seed k is the first p whose inclusive prefix sum of q exceeds t; index 0 when total == 0.  This is
 *      torch.multinomial(distance_to_nearest_seed, 1) quantised to about 1 um and stated in integers.  One launch, one workgroup per frame.
 * quber_gms_climb: dev_seeds f32 [B][num_seeds][3] in and out; with dev_indices (may be NULL) it is first set to the points of Xs they
 *   name (zero where the index is -1).  iters times, for the rows below S: W = exp(-0.5 / sigma^2 |Z - Xs|^2), Z = (W Xs) / sum W, in
 *   float32 as a shift of Z (sum W (Xs - Z) / sum W), with a fixed reduction order: block partials are added in float64 in block order,
 *   no floating-point atomics - two calls give the same bits, and a frame's result does not depend on the batch it is in.  A seed whose
 *   weights sum to 0 keeps its position (the reference would make it NaN).  0 <= iters <= 1000, sigma > 0.
 * quber_gms_link -> dev_seed_labels i32 [B][num_seeds] (-1 behind S): connected_components as written - in seed order, an unlabelled
 *   seed i labels every seed j with dist(Z[j], Z[i]) <= epsilon: with the mode of the labels already there (the smallest among equal
 *   counts) if there is one, else with the next new label.  A seed is inside its own ball, so the labels are 0..K-1 without gaps.
 * quber_gms_assign: every fg pixel (all of P) takes the label of the first seed at minimum dist; labels with fewer than min_pixels
 *   pixels are dropped, the survivors are numbered 1..count by ascending label, those behind n_masks (1..254) are dropped.
 *   -> dev_ids i32 [B][H][W] (0, 1..count), dev_masks u8 [B][n_masks][H][W] (ids == k + 1 as 0 / 255, zero planes behind count; may be
 *      NULL), dev_centers f32 [B][n_masks][3] (the mean of the climbed seeds that carry the label: a float32 sum in seed order, divided
 *      by their number; zero rows behind count), dev_report i32 [B][6]: count, clusters found (K), dropped by min_pixels, 1 if truncated
 *      to n_masks, 0 (ids emptied by the IMP), fg pixels.
 * quber_gms_imp, on ANY id map: dev_ids i32 [B][H][W] in place, 0 = none, 1..n_ids (<= 254; a value outside counts as 0 and is written
 *   back as 0).  For o = 1..n_ids in ascending order on the CURRENT map: mask = ids == o is opened, then closed, with
 *   cv2.getStructuringElement(MORPH_ELLIPSE, (ksize, ksize)) (ksize odd, 1..15) and OpenCV's default constant border (beyond the frame
 *   reads as 1 for an erosion, as 0 for a dilation); ids[mask] = 0, ids[result] = o.  Then, if largest, the largest 4-connected component
 *   of every id (quber_cleanup_ids with keep_largest = 1, connectivity = 4).  Ids left empty are dropped, the rest renumbered 1..count'.
 *   -> dev_masks u8 [B][n_masks][H][W] (may be NULL with n_masks = 0), dev_centers f32 [B][n_ids][3] (may be NULL) in and out: the rows
 *      of the ids that stay, moved up, zero behind them; dev_report i32 [B][6] (may be NULL): entry 0 = count', entry 4 = ids that were
 *      present and are empty now; the other entries are not touched.  One workgroup per frame with both bit planes in LDS: a frame with
 *      2 * H * ceil(W / 32) * 4 > 152 KiB is an error (no global-memory fallback).
 * quber_gms_cluster: seeds -> climb -> link -> assign -> (imp_ksize != 0: imp) on `stream`, with every intermediate result as an
 *   output: dev_raw_ids is the id map before the IMP, dev_ids the one after it (equal without); masks, centers and report describe dev_ids.
 * Every output is overwritten by every call.  H * W <= 2^24.  No host copy, no synchronisation, no memset node, no cooperative launch.
 * The workspace (block counts, compacted points, running minimum, raw labels, tables, block partials: 1 MB + 20 H W bytes per frame of
 * max_batch) is not part of quber_create: the FIRST call of any of these entries (quber_gms_link excepted, which needs none) allocates it
 * and keeps it (quber_workspace_bytes counts it from then on), so that call is not capturable into a graph; later calls are.  Works on a
 * context created with with_network = 0. */
int quber_gms_seeds(quber_ctx* ctx, const float* dev_votes, const uint8_t* dev_fg, int32_t batch, int32_t subsample, const int32_t* dev_first,
                    const uint32_t* dev_draws, int32_t num_seeds, int32_t* dev_indices, int32_t* dev_info, void* stream);
int quber_gms_climb(quber_ctx* ctx, const float* dev_votes, const uint8_t* dev_fg, int32_t batch, int32_t subsample, const int32_t* dev_indices,
                    const int32_t* dev_info, int32_t num_seeds, float sigma, int32_t iters, float* dev_seeds, void* stream);
int quber_gms_link(quber_ctx* ctx, const float* dev_seeds, int32_t batch, int32_t num_seeds, const int32_t* dev_info, float epsilon,
                   int32_t* dev_seed_labels, void* stream);
int quber_gms_assign(quber_ctx* ctx, const float* dev_votes, const uint8_t* dev_fg, int32_t batch, const float* dev_seeds,
                     const int32_t* dev_seed_labels, const int32_t* dev_info, int32_t num_seeds, int32_t min_pixels, int32_t n_masks,
                     int32_t* dev_ids, uint8_t* dev_masks, float* dev_centers, int32_t* dev_report, void* stream);
int quber_gms_imp(quber_ctx* ctx, int32_t* dev_ids, int32_t batch, int32_t n_ids, int32_t ksize, int32_t largest, int32_t n_masks,
                  uint8_t* dev_masks, float* dev_centers, int32_t* dev_report, void* stream);
int quber_gms_cluster(quber_ctx* ctx, const float* dev_votes, const uint8_t* dev_fg, int32_t batch, const int32_t* dev_first,
                      const uint32_t* dev_draws, int32_t num_seeds, float sigma, int32_t iters, float epsilon, int32_t subsample,
                      int32_t min_pixels, int32_t imp_ksize, int32_t imp_largest, int32_t n_masks, int32_t* dev_indices, float* dev_seeds,
                      int32_t* dev_seed_labels, int32_t* dev_info, int32_t* dev_raw_ids, int32_t* dev_ids, uint8_t* dev_masks,
                      float* dev_centers, int32_t* dev_report, void* stream);

/* Zoom-in refinement (csrc/zoom.hip): the gather / scatter around a second pass that shows the network every first-pass instance as
 * a padded crop resized to a fixed square - the reference's crop_rois and match_label_crop (eval/base_model.py:843-961, copies at :1088
 * and :1192), which run one mask at a time with torch.unique, nonzero and a .cpu() per paste.  The numpy statement of what the three
 * calls compute is tests/test_zoom_cpu.py: zoom_rois_np, zoom_crop_np, zoom_paste_np; INTEGRATION.md "Zoom-in refinement" has it in words.
 *
 * quber_zoom_rois: dev_ids i32 [B][H][W], a compact map (0 = none, 1..n_ids; other values are ignored), n_ids <= 254
 *   -> dev_rois i32 [B][n_ids][4] = (x0, y0, x1, y1), inclusive: the tight extent of id j + 1, each side moved out by
 *      rint(float32(x1 - x0) * padding) (y alike; round half to even, base_model.py:865) and clamped to the frame; (0, 0, -1, -1) for
 *      an id without a pixel.  0 <= padding <= 16.
 * quber_zoom_crop: dev_bgr (and dev_depth, or NULL) u8 [B][H][W][3], dev_ids as above, dev_slots i32 [n_slots][2] = (frame, id): one
 *   crop per slot, dev_rois as above; 2 <= crop = S <= 512; n_slots <= 254 * max_batch
 *   -> dev_bgr_crop (dev_depth_crop) u8 [n_slots][S][S][3]: the ROI resized bilinearly with align_corners (F.upsample_bilinear) in exact
 *      rational arithmetic on the bytes: with d = S - 1, y0 = dy (h - 1) / d, ry = dy (h - 1) % d (x alike), weights (d - r) and r, the
 *      neighbour clamped to the ROI, out = (sum + d d / 2) / (d d)
 *   -> dev_mask_crop u8 [n_slots][1][S][S]: 255 where ids == id at the source pixel of F.upsample_nearest, whose index is
 *      min(int(floorf(float32(dst) * (float32(in) / float32(out)))), in - 1), else 0
 *   A slot that is no crop (frame or id out of range, a ROI that is empty or leaves the frame) gives zero crops.
 * quber_zoom_paste: dev_crop_ids i32 [n_slots][S][S] (the crop pass's compact ids, 0..n_crop_ids), dev_crop_scores f32
 *   [n_slots][n_crop_ids], dev_table / dev_area u32 [n_slots][n_crop_ids + 1] (quber_overlap_masks of (dev_mask_crop, dev_crop_ids):
 *   pixels of id i inside the crop's own mask, pixels of id i), dev_depth_crop or NULL, dev_slots ascending by frame, dev_rois
 *   keep   crop-pass instance i >= 1 with area > 0 is kept iff float32(overlap) / float32(area) >= min_overlap (base_model.py:898-907)
 *   order  a frame's crops are painted in descending mean of the positive channel-2 depths under their kept instances, compared as
 *          exact fractions, a crop without such a pixel first, equal keys in slot order (:909-930); dev_depth_crop NULL: in descending
 *          ROI area
 *   paste  in that order, a crop's kept instances in ascending id: the crop's id plane resized back to the ROI by the nearest rule
 *          overwrites the frame where it is a kept instance (:932-959); the instances that still own a pixel get the final ids 1.. in
 *          that order, at most max_inst (1..254) of them - the surplus is dropped
 *   -> dev_out_ids i32 [B][H][W]; dev_out_masks u8 [B][max_inst][H][W] (0 / 255, zero planes behind count); dev_source i32
 *      [B][max_inst][2] (first-pass id, crop-pass id; -1 behind count); dev_out_scores f32 [B][max_inst] (0 behind); dev_boxes f32
 *      [B][max_inst][4] (x_min, y_min, x_max + 1, y_max + 1; 0 behind); dev_report i32 [B][4]: crops, kept instances, kept instances
 *      that got no final id (painted over or surplus), count
 * Every output is overwritten by every call; the inputs are not written.  All launches go to `stream`: no host copy, no
 * synchronisation, no memset node (the tables are cleared by the zero-fill kernel).  The workspace (extents, keep flags, depth keys,
 * paint order, key map, sized for max_batch frames) is not part of quber_create: the FIRST call of quber_zoom_rois or quber_zoom_paste
 * allocates it and keeps it (quber_workspace_bytes counts it from then on), so that call is not capturable into a graph; later calls
 * are.  The entries of one context share it: they run on one stream at a time.  They work on a context created with with_network = 0. */
int quber_zoom_rois(quber_ctx* ctx, const int32_t* dev_ids, int32_t batch, int32_t n_ids, float padding, int32_t* dev_rois, void* stream);
int quber_zoom_crop(quber_ctx* ctx, const uint8_t* dev_bgr, const uint8_t* dev_depth, const int32_t* dev_ids, const int32_t* dev_slots,
                    const int32_t* dev_rois, int32_t batch, int32_t n_ids, int32_t n_slots, int32_t crop, uint8_t* dev_bgr_crop,
                    uint8_t* dev_depth_crop, uint8_t* dev_mask_crop, void* stream);
int quber_zoom_paste(quber_ctx* ctx, const int32_t* dev_crop_ids, const float* dev_crop_scores, const uint32_t* dev_table,
                     const uint32_t* dev_area, const uint8_t* dev_depth_crop, const int32_t* dev_slots, const int32_t* dev_rois,
                     int32_t batch, int32_t n_ids, int32_t n_slots, int32_t crop, int32_t n_crop_ids, float min_overlap, int32_t max_inst,
                     int32_t* dev_out_ids, uint8_t* dev_out_masks, int32_t* dev_source, float* dev_out_scores, float* dev_boxes,
                     int32_t* dev_report, void* stream);

/* Validation losses (csrc/losses.hip): the reference's training targets and the five values of its loss dict, per frame, without leaving
 * the device - PanopticDeepLabTargetGenerator (maskrefiner/data/dataset_mappers/target_generator.py:8-165) and DeepLabBCE / center_losses
 * / offset_losses / the two error-head losses (maskrefiner/modeling/mask_refiner/model.py:36-72, 672-687, 766-802).  The numpy / float64
 * torch statement of what the two calls compute is tests/test_losses_cpu.py: loss_targets_np, losses_ref; INTEGRATION.md "Validation
 * losses" has it in words, with the deviations.
 *
 * quber_loss_targets: dev_gt i32 [B][H][W] (0 = none, 1..n_gt; other values count as 0), n_gt <= 254; every id a thing, none crowd
 *   sigma 1..20; dev_gauss f32 [(6 sigma + 3)^2]: exp(-((i - x0)^2 + (j - y0)^2) / (2 sigma^2)) in float64 with x0 = y0 = 3 sigma + 1,
 *     rounded to float32 BY THE CALLER (numpy), so the heat values are numpy's bits whatever the device's exp does
 *   -> dev_targets f32 [B][6][H][W]: centre heat (the maximum over the instances whose window [x - 3 sigma - 1, x + 3 sigma + 2) x
 *        [y ...) around the peak (rint(cy), rint(cx)) holds the pixel), off_y = cy - y and off_x = cx - x inside an instance (float64
 *        rounded once, or all float32 with quber_config.encode_legacy_f32), sem_seg 0 / 1, sem_seg_weights (small_weight inside an
 *        instance of fewer than small_area pixels, else 1), inst_weights 0 / 1 (the reference's center_weights == offset_weights)
 *   -> dev_points f64 [B][n_gt][2] = (cy, cx) = (sum y, sum x) / count in float64; dev_area i32 [B][n_gt]; zeros for an id without a pixel
 * quber_losses: dev_logits f32 [B][n_planes][H][W] (quber_forward's planes), dev_targets as above, dev_explicit u8 [B][2][4][H][W]
 *   (quber_explicit_error_maps; may be NULL when spec names no head)
 *   -> dev_out f64 [B][QUBER_LOSS_WORDS], per frame (the reference's value for a batch of that one frame):
 *        [0] loss_sem_seg = foreground_weight * (sum of the k largest BCEWithLogits(x, sem_seg) * sem_seg_weights) / k, k = int(top_k * H * W)
 *            (all pixels for top_k == 1.0; k == 0 is an error)   [1] loss_center = center_weight * sum((x - t)^2 w) / sum(w)
 *        [2] loss_offset = offset_weight * sum over BOTH planes(|x - t| w) / sum over ONE plane(w) (model.py:796-798); [1], [2] = 0 for sum(w) = 0
 *        [3] loss_eee_mask, [4] loss_eee_boundary (0 for an absent head): dice = mean over classes of 1 - (2 sum(t p) + 1e-5) / (sum(t) +
 *            sum(p) + 1e-5), p = softmax; cross_entropy = mean over pixels of -sum_c t_c log_softmax(x)_c.  Targets: the stack of
 *            model.py:186-226 for error_type.  Neither is multiplied by EEE_*_LOSS_WEIGHT (the reference does not either)
 *        [5] the foreground sum, [6] k, [7] the k-th largest value T and [8] the number of values above it (both 0 for top_k == 1.0),
 *        [9] centre numerator, [10] sum(w), [11] offset numerator, [12] H * W, [13..25] eee_mask: cross-entropy sum, then per class (4
 *        slots each) sum(t p), sum(t), sum(p); [26..38] eee_boundary alike; [39] 0
 *   Per-pixel terms are evaluated in float64 from the float32 inputs and added in a fixed order (no floating-point atomics: two runs give
 *   the same bits); T is exact (a radix select on the bit patterns).
 * Every output is overwritten by every call; the inputs are not written.  All launches go to `stream`: no host copy, no synchronisation,
 * no memset node.  The workspace (moments, centres, block partials, histograms, the float64 foreground plane, sized for max_batch
 * frames) is not part of quber_create: the FIRST call of either entry allocates it and keeps it (quber_workspace_bytes counts it from
 * then on), so that call is not capturable into a graph; later calls are.  Both work on a context created with with_network = 0. */
#define QUBER_LOSS_WORDS 40
typedef struct quber_loss_spec {
    double top_k;                    /* INS_EMBED_HEAD.FOREGROUND_LOSS_TOP_K, in (0, 1] */
    double foreground_weight;        /* INS_EMBED_HEAD.FOREGROUND_LOSS_WEIGHT */
    double center_weight;            /* INS_EMBED_HEAD.CENTER_LOSS_WEIGHT */
    double offset_weight;            /* INS_EMBED_HEAD.OFFSET_LOSS_WEIGHT */
    int32_t error_type;              /* INS_EMBED_HEAD.ERROR_TYPE: 0 e3 (4 classes), 1 e2 (2), 2 e33 (3), 3 e32 (2) */
    int32_t eee_mask_plane;          /* first logit plane of the region-error head, -1 = no such head */
    int32_t eee_boundary_plane;      /* ... of the boundary-error head */
    int32_t eee_mask_loss;           /* 0 dice, 1 cross_entropy */
    int32_t eee_boundary_loss;
    int32_t reserved;                /* 0 */
} quber_loss_spec;
int quber_loss_targets(quber_ctx* ctx, const int32_t* dev_gt, int32_t batch, int32_t n_gt, int32_t sigma, int32_t small_area,
                       float small_weight, const float* dev_gauss, float* dev_targets, double* dev_points, int32_t* dev_area, void* stream);
int quber_losses(quber_ctx* ctx, const float* dev_logits, int32_t n_planes, const float* dev_targets, const uint8_t* dev_explicit,
                 const quber_loss_spec* spec, int32_t batch, double* dev_out, void* stream);

/* evaluation support - all pairwise overlap counts of two label maps in one pass. Replaces the per-pair
 * np.count_nonzero loops of eval/evaluation.py:180-199 (multilabel_metrics).
 *   dev_pred, dev_gt i32 [n_pixels], label values in 0..65535, at most `cap` (<= 1024) distinct values per map
 *   workspace (quber_contingency_workspace_bytes(cap) bytes, device) receives, in this order:
 *     u32 flags[2][65536] | u64 table[cap][cap] (row = gt index, column = pred index) | i32 labels[2][cap] (sorted unique
 *     values: [0] pred, [1] gt) | i32 counts[4] = (n_pred, n_gt, out-of-range flag, 0) | u16 lut[2][65536] */
int64_t quber_contingency_workspace_bytes(int32_t cap);
int quber_label_contingency(const int32_t* dev_pred, const int32_t* dev_gt, int64_t n_pixels, int32_t cap,
                            void* dev_workspace, void* stream);

/* evaluation support - the boundary half of multilabel_metrics: for every (ground-truth object i, predicted object j) the
 * true-positive counts of eval/evaluation.py:21-54 `boundary_overlap` and the per-object boundary sizes of :165-175.
 * seg2bmap (eval/utilities.py:672-697: cv2.findContours RETR_EXTERNAL + drawContours) and the disk dilation are restated
 * from their published algorithms (no OpenCV / skimage in the build image; parity unpinned).
 *   dev_pred, dev_gt i32 [h][w] label maps; dev_labels i32 [n_pred + n_gt]: the object labels, predicted ones first
 *   bound_pix: disk radius = ceil(0.003 * hypot(h, w)) in the reference (evaluation.py:33-34)
 *   -> dev_out u32: boundary size [n_pred + n_gt] | precision_tps [n_gt][n_pred] | recall_tps [n_gt][n_pred]
 *   dev_workspace: quber_boundary_workspace_bytes(h, w, n_pred + n_gt) bytes; h * ceil(w / 64) * 8 must fit 160 KiB of LDS */
int64_t quber_boundary_workspace_bytes(int32_t h, int32_t w, int32_t n_masks);
int quber_boundary_overlap(const int32_t* dev_pred, const int32_t* dev_gt, int32_t h, int32_t w, const int32_t* dev_labels,
                           int32_t n_pred, int32_t n_gt, int32_t bound_pix, void* dev_workspace, uint32_t* dev_out,
                           void* stream);

/* evaluation support - multilabel_metrics (eval/evaluation.py:57-274) for `batch` pairs of label maps in one call, with no read-back in
 * between: the label counts, the F-measure matrix and the Munkres assignment (eval/munkres.py, with its tie-breaking) stay on the
 * device, the caller copies dev_out back once and does the final float sums (numpy's summation order is part of the reference's numbers).
 *   dev_pred, dev_gt i32 [batch][h][w] (h * w <= 2^32), batch 1..4096
 *   cap 1..256: most distinct labels per map, background included; a frame above it is flagged (status 2), never truncated
 *   bound_pix, with_boundary: as quber_boundary_overlap (same frame-size limit: h * ceil(w / 64) * 8 <= 160 KiB - 64); 0 = no boundary work
 *   placement of the solver's cost matrix: 0 = LDS for a frame of up to 128 objects a side, device memory above; 1 = LDS (a larger frame
 *     gets status 8); 2 = device memory
 *   dev_workspace: quber_eval_batch_workspace_bytes(batch, h, w, cap, with_boundary) bytes =
 *     batch * (786440 + 16 cap^2 [+ 3 * 2 cap * h * ceil(w / 64) * 8]), rounded up to 8
 *   -> dev_out: one record per frame, R = 24 cap^2 + 68 cap + 32 bytes rounded up to 8, every byte written by every call; at byte offset
 *        0                      u64 table[cap][cap]   row = gt label index, column = predicted label index (quber_label_contingency)
 *        8 cap^2                f64 F[cap][cap]       F-measure, row = gt OBJECT, column = predicted OBJECT (labels != 0), row stride cap
 *        16 cap^2               u64 area[2][cap]      pixels per label index, predicted then gt
 *        16 cap^2 + 16 cap      u64 pair_tps[cap], u64 pair_union[cap]     per assigned pair
 *        16 cap^2 + 32 cap      u32 ptps[cap][cap], u32 rtps[cap][cap]     boundary true positives [gt object][predicted object]
 *        24 cap^2 + 32 cap      i32 hdr[8] = labels in pred, labels in gt, out-of-range flag, STATUS, objects in pred, objects in gt, pairs, the solver's bits
 *        ... + 32               i32 labels[2][cap] (sorted), u32 boundary size[2][cap] (per object), i32 assign[cap] (per gt object the
 *                               predicted object or -1), i32 pairs[cap][2] (gt object, predicted object), u32 pair_ptps[cap], u32 pair_rtps[cap]
 *      STATUS bits: 1 a label outside 0..65535, 2 more than cap labels in a map, 4 the solver reached one of its iteration bounds
 *      (non-finite scores only), 8 placement 1 and the frame does not fit.  A frame with a status has no usable tables.
 * quber_munkres_batch is the solver alone: dev_score f64 [batch][cap][cap] holds a dev_rows[b] x dev_cols[b] cost matrix per frame (row
 * stride cap; zero-padded to square as the reference does), dev_assign i32 [batch][cap] receives per row the assigned column or -1,
 * dev_status i32 [batch] the bits 2 (shape outside 0..cap), 4, 8.  dev_workspace: batch * cap^2 * 8 bytes for placement 2, and for
 * placement 0 with cap > 128; may be NULL otherwise. */
int64_t quber_eval_batch_workspace_bytes(int32_t batch, int32_t h, int32_t w, int32_t cap, int32_t with_boundary);
int quber_eval_batch(const int32_t* dev_pred, const int32_t* dev_gt, int32_t batch, int32_t h, int32_t w, int32_t cap, int32_t bound_pix,
                     int32_t with_boundary, int32_t placement, void* dev_workspace, void* dev_out, void* stream);
int quber_munkres_batch(const double* dev_score, const int32_t* dev_rows, const int32_t* dev_cols, int32_t batch, int32_t cap,
                        int32_t placement, void* dev_workspace, int32_t* dev_assign, int32_t* dev_status, void* stream);

/* post-filter of eval/refiner_model.py:273-277 on LMFFNet logits (foreground_segmentation/predictor.py:85,98):
 *   dev_fg_logits f32 [B][n_classes][HW] -> dev_fg_mask u8 [B][HW] = (argmax == fg_class)
 *   dev_masks u8 [B][n_masks][HW] (may be NULL with n_masks = 0)
 *   -> dev_counts u64 [B][n_masks][2] = (|mask & fg|, |mask|); the caller keeps masks with inter / area > 0.3 */
int quber_foreground_filter(const float* dev_fg_logits, int32_t n_classes, int32_t fg_class, const uint8_t* dev_masks,
                            int32_t batch, int32_t n_masks, int64_t hw, uint8_t* dev_fg_mask, uint64_t* dev_counts,
                            void* stream);

/* the foreground filter of the UOAIS base model (eval/base_model.py:210-216) on a CGNet foreground map (quber_foreground_filter with
 * n_classes = 2, fg_class = 1 on the logits of a with_network = 3 context):
 *   dev_fg u8 [B][fg_h][fg_w], dev_masks u8 [B][n_masks][h][w] at any size (may be NULL with n_masks = 0)
 *   -> dev_counts u64 [B][n_masks][2] = (|mask & fg'|, |mask|), fg'(y, x) = fg(floor(y fg_h / h), floor(x fg_w / w)) (OpenCV's float64
 *      factors 1 / (h / fg_h), 1 / (w / fg_w)): the
 *      cv2.resize(fg, (w, h), INTER_NEAREST) of foreground_segmentation/predictor.py:50 folded into the read.  The caller skips empty
 *      masks and keeps those with inter / area > 0.5.  Integer sums: exact.  Nothing is written for n_masks = 0. */
int quber_foreground_overlap(const uint8_t* dev_fg, int32_t fg_h, int32_t fg_w, const uint8_t* dev_masks, int32_t batch, int32_t n_masks,
                             int32_t h, int32_t w, uint64_t* dev_counts, void* stream);

/* adapter pre-processing - depth normalisation.  Replaces normalize_depth (eval/preprocess_utils.py:12-28) and the
 * zero-depth bookkeeping of eval/refiner_model.py:250.
 *   dev_depth: uint16 [n] (is_float32 = 0, e.g. PNG millimetres, evaluated in float64 like numpy) or f32 [n]
 *   -> dev_out3 u8 [n][3] (the value replicated to 3 channels), dev_zero u8 [n] = (depth == 0), may be NULL */
int quber_normalize_depth(const void* dev_depth, int32_t is_float32, int64_t n_pixels, double min_val, double max_val,
                          uint8_t* dev_out3, uint8_t* dev_zero, void* stream);

/* adapter pre-processing - cv2.resize of an interleaved uint8 image (eval/refiner_model.py:229 `cv2.resize(rgb, (w, h))`,
 * :232 / :254 INTER_NEAREST on masks / depth, :246).  linear = 1: cv2.INTER_LINEAR's 8-bit path (11-bit fixed-point
 * weights; the area filter at exactly half scale), linear = 0: cv2.INTER_NEAREST.  OpenCV is absent from the build image:
 * restated from its published algorithm, parity unpinned.
 *   dev_src u8 [src_h][src_w][channels] (channels 1..4) -> dev_dst u8 [dst_h][dst_w][channels] */
int quber_resize_u8(const uint8_t* dev_src, int32_t src_h, int32_t src_w, int32_t channels, uint8_t* dev_dst,
                    int32_t dst_h, int32_t dst_w, int32_t linear, void* stream);

/* adapter pre-processing - cv2.inpaint(img, mask, radius, cv2.INPAINT_TELEA) of one 8-bit channel (inpaint_depth,
 * eval/preprocess_utils.py:44-64).  The ONE entry point that takes HOST pointers and runs on the host, like the OpenCV call
 * it replaces (the fast-marching method is sequential; it runs once per frame outside the refiner's timed region).
 * Restated from Telea's published algorithm in the form OpenCV implements it; parity unpinned, own tolerance.
 *   host_img u8 [h][w], host_mask u8 [h][w] (non-zero = to be filled)  ->  host_out u8 [h][w] */
int quber_inpaint_telea_u8(const uint8_t* host_img, const uint8_t* host_mask, int32_t h, int32_t w, int32_t radius,
                           uint8_t* host_out);
/* inpaint_depth(depth, kernel_size) of eval/preprocess_utils.py:44-64 (factor 1) in one host call: mask = pixels whose three channels
 * are 0, dilated by a kernel x kernel square; TELEA in-painting (radius = kernel) per channel; only the zero pixels are replaced.
 *   host_depth3 u8 [h][w][3]  ->  host_out3 u8 [h][w][3] */
int quber_inpaint_depth_u8(const uint8_t* host_depth3, int32_t h, int32_t w, int32_t kernel, uint8_t* host_out3);
/* The same on the DEVICE, asynchronous on `stream`, for a batch of frames, bit-equal to the host function above (csrc/inpaint_dev.hip):
 * the hole regions that can influence each other (connected components of the mask dilated by radius + 2) are marched one wave each
 * with the host's queue order; a pixel's (2 r + 1)^2 neighbours are evaluated one per lane and summed in the host's order.
 * kernel <= 3 (the reference calls it with 3: eval/refiner_model.py:255).
 *   dev_depth3 u8 [batch][h][w][3] -> dev_out3 u8 [batch][h][w][3]; dev_workspace: quber_inpaint_depth_workspace_bytes(batch, h, w) bytes */
int64_t quber_inpaint_depth_workspace_bytes(int32_t batch, int32_t h, int32_t w);
int quber_inpaint_depth_device(const uint8_t* dev_depth3, int32_t batch, int32_t h, int32_t w, int32_t kernel, void* dev_workspace,
                               int64_t workspace_bytes, uint8_t* dev_out3, void* stream);

/* ---- introspection / kernel-level entry points used by the parity tests and the benchmark ---- */
/* device pointer + NHWC geometry of a named intermediate of the last quber_forward ("res2", "res3", "res5", "y", ...) */
int quber_debug_tensor(quber_ctx* ctx, const char* name, float** dev_ptr, int32_t* dims4, int32_t* channel_stride);
/* bytes per element of that intermediate: 4 (fp32), or 2 (fp16) in the fp16 data path (compute_dtype 2); 0 = no such tensor */
int32_t quber_debug_tensor_elem_size(quber_ctx* ctx, const char* name);
/* algorithmic FLOPs of one forward at batch 1 (2 * MACs of every convolution) */
double quber_forward_flops(quber_ctx* ctx);
/* FLOPs the matrix pipe actually executes per forward at batch 1: a layer planned as Winograd F(m x m,3x3) counts
 * (m+2)^2 / (9 m^2) of its algorithmic FLOPs, padded tiles included (transform additions not counted) */
double quber_forward_flops_executed(quber_ctx* ctx);
/* ... and the part of those executed FLOPs that is tile padding (ragged maps, short phases of dilated layers): a 30x40 map under 4x4 tiles
 * carries 6.7 % of it */
double quber_forward_flops_padding(quber_ctx* ctx);
/* Options.  Every knob that shapes a plan or changes the arithmetic / work distribution of a launch belongs to a CONTEXT:
 *   quber_set_option(ctx, key, value)   this context only.  "plan" keys act when quber_finalize_weights builds the plan and
 *                                       are refused afterwards; "launch" keys may change between forwards.
 *   quber_get_option(ctx, key, &value)
 *   quber_set_tuning(key, value)        the PROCESS DEFAULTS: what a context created afterwards starts from (quber_create copies
 *                                       them) and what the stand-alone quber_op_* test ops, which have no context, use.  Contexts
 *                                       that already exist are not affected.  Keys 2, 11, 12, 26 exist only here (test harness).
 * Two engines with different options coexist in one process and may run on different threads.
 * Context keys (default; when it acts):
 * key 3  (0; launch, test harness) force the number of K partitions of convolutions that have a workspace (0 = automatic);
 * key 4  (0; launch, test harness) force the convolution tile shape (1 = 64x64, 2 = 128x128, 3 = 128x64, 4 = 256x32);
 * key 5  (1; launch) split the ragged last round of large convolution launches into K-pieces: when the cost model favours
 *         it (1), never (0), whenever feasible (2);
 * key 6  (0; plan) Winograd path of the eligible 3x3 layers: 0 = where it pays, 1 = never, 2 = always;
 * key 7  (32; plan) smallest input width (channels) routed to the Winograd path (below 128 channels a layer takes it only in the
 *         single-kernel form, key 25);
 * key 8  (67; plan) Winograd only while its multiplies are <= value % of the direct kernel's (dilated layers);
 * key 9  (0; plan) Winograd output tile edge of the eligible layers: 0 = automatic (F(4x4), or F(2x2) where its tiles fit the
 *         map better; both measure the direct kernel's error), 2, 4, or 6 = opt into F(6x6,3x3) where it executes >= 10 % fewer
 *         multiplies still (2.5x the error at tap level, +4.5 % throughput at batch 16); the algorithm of every layer is fixed at
 *         plan time from its geometry alone, never from the batch of a launch;
 * key 10 (32; plan) smallest output width routed to the Winograd path;
 * key 13 (1; launch) persistent convolution launches (csrc/conv_persist.hip): 0 = never (one tile per block everywhere),
 *         1 = the 128x128-tile launches, 2 = every tile shape;
 * key 14 (32; launch) persistent launches: shortest K, in 32-wide slices, whose remainder tiles are shared between blocks;
 * key 15 (256; launch) persistent launches: fewest tiles (all groups) of a launch that goes persistent (smaller launches - small
 *         batches - keep the one-tile-per-block kernel and its split-K model);
 * key 16 (0; diagnostics) 1 = the output stores of the persistent convolution kernel are dropped by the range check;
 * key 17 (0; launch) Winograd F(4x4) transforms on channel pairs instead of quads (measured: input transform 6 % slower);
 * key 18 (1; plan) the projection block of every ResNet stage runs conv3 and its shortcut as ONE 1x1 GEMM over the
 *         concatenated inputs (reference: detectron2 BottleneckBlock as built by maskrefiner/modeling/backbone/resnet.py:37-63)
 *         or as two convolutions (0);
 * key 19 (1; launch) 128x64 tiles for the convolutions with 33-64 output channels and no residual, or 64x64 (0);
 * key 20 (0; launch) Winograd pipeline layers in passes whose V | M intermediates stay below `value` MiB (0 = the whole batch at
 *         once; measured slower at every size: profiles/r03c_wino_subbatch_rejected.md);
 * key 21 (2; launch, ARITHMETIC) K-slices per chunk of the two-level fp32 accumulation of the GEMM kernels (the bf16x3 mode folds
 *         every `value` slices, the exact fp32 mode every slice; 0 = one sequential chain over K);
 * key 24 (1; launch) side lanes at batches <= 16 (exact fp32 and bf16x3: <= 12), or everything on the caller's stream (0);
 * key 25 (1; plan) Winograd F(4x4,3x3) layers as ONE kernel - input transform, the 36 position GEMMs and the output transform, no
 *         V | M intermediates in HBM (csrc/wino_fused.hip): the eligible layers, or never (0);
 * key 27 (160; plan, ARITHMETIC) widest input, in channels, that takes the single-kernel form.  Its two accumulation chains are
 *         Cin / 2 long - 80 channels at the default, with which the float64-anchor ratios stay 0.64-1.11; admitting 256 / 320
 *         channels (chains of 128-160) measures 1.20 / 1.21 and no speed-up inside the network (DECISIONS.md section 4,
 *         profiles/r05_fused_anchor.md, r05_wino_fused_layers.md).
 * key 29 (1; plan) the input normalisation + concatenation (a3, model.py:137-153) inside the first stem convolution's kernel
 *         (csrc/stem.hip: same fmaf chains as the implicit GEMM, no normalised input tensor in HBM; fp16 data path: the layer on the
 *         matrix pipe from 16-byte fp16 pixels staged in LDS, equal to the preprocess kernel + implicit GEMM up to fp32 summation
 *         order; 2 = the fp16 data path keeps the vector-FMA form of the kernel), or as a kernel of its own (0).
 * key 30 (1; launch) implicit GEMM loader: block-uniform filter taps in scalar registers, a tap-validity bit mask and a 32-bit byte
 *         offset per row, buffer loads whose out-of-range offset returns the zero padding (conv_igemm.hip LEAN; layers with
 *         Cin % 32 == 0 - fp16 data path: % 64 - and tensors below 2 GiB), or per-thread tap arithmetic everywhere (0).  Same bits.
 * key 31 (1; plan + launch) fp16 data path: the layers with >= 256 output channels and K a multiple of 64 on 256 x 256 tiles with the LDS-DMA
 *         operand pipeline (csrc/conv_h8.hip: resnet.py:395-449 res4 / res5 bottlenecks, :472-485 fusion convolutions, the ASPP
 *         branches of model.py:610-651), 0 = the 128-tile kernel everywhere, 2 = also narrower outputs (tests).  Same arithmetic
 *         (fp16 products, fp32 accumulation), another summation order inside a K-tile.
 *         (plan + launch, keys 31 and 38: the value at quber_finalize_weights decides the SHAPE of the plan - with 31 on, the three dilated
 *         ASPP branches are one grouped op; with 31, 38 and 39 on, a norm in front of a patch-kernel layer is planned as absorbed - so op
 *         list, GroupNorm slots and quber_op_info names differ between plans built under different values.  The value at LAUNCH only
 *         selects kernels: with a key switched off afterwards the same ops run on conv_igemm.hip and an absorbed norm as the pass it was.)
 * key 32 (224; launch) fewest tiles (all groups) of a launch that key 31 takes: its blocks own a CU each.
 * keys 33, 34: retired (the exact-fp32 256 x 128 LDS-DMA kernel was no faster in the network and was removed: profiles/r11_f8.md).
 * key 35 (1; launch) bf16x3 mode: the wide 1x1 launches and the Winograd position GEMMs on csrc/conv_x8.hip (256 x 128 tiles, LDS-DMA
 *         pipeline, the weights pre-split into three bf16 planes when the plan is built, the activations split in registers by the
 *         wave that is not multiplying); the same six partial products in the same order as conv_igemm.hip's bf16x3 kernels.
 *         0 = those kernels everywhere, 2 = every covered launch (tests).
 * key 36 (2; launch) fewest rounds of tiles (tiles / CUs), key 37 (8; launch) fewest K-slices of 32 of a launch that key 35 = 1 takes.
 * key 38 (1; plan + launch) fp16 data path: the undilated 3x3 / stride 1 layers with the pixel operand as an LDS patch - a tile is 8 x 32 output
 *         pixels, the 10 x 34-pixel patch of a 64-channel block is fetched once and the nine taps read it at shifted addresses, instead of
 *         nine DMA gathers (conv_h8.hip: conv_h8p_kernel up to 128 output channels, conv_h8w_kernel 256 and more, conv_h8s_kernel the stem's
 *         32-channel inputs with LDS-resident filters); 0 = key 31's DMA-gather kernels / conv_igemm.hip there, 2 = only up to 128 channels.
 * key 39 (1; plan) fp16 data path: a patch-kernel layer of up to 128 output channels that is the only reader of a GroupNorm + ReLU output
 *         (decoder fuse convolutions, the heads' second convolution: model.py:386-403, 610-651) applies that norm to its LDS patches - the
 *         arithmetic of the norm pass, bit for bit, without the pass over the tensor in HBM; 0 = every norm is a pass of its own.
 * key 41 (1; plan) small batches (side lanes, key 24): the dilated ASPP branches d = 6 / 12 (model.py:610-651) on the two side lanes,
 *         beside the d = 18 and 1x1 branches on the caller's stream; 0 = one after the other.  Same launches, same bits.
 * key 42 (1; launch) exact fp32 (and the bf16x3 mode's launches that conv_x8.hip does not take): 1x1 GEMMs - bottleneck / fusion / ASPP 1x1
 *         convolutions of resnet.py:395-449, 472-485 and model.py:610-651, Winograd position GEMMs - on 64 x 64 tiles, one per block, instead of
 *         the 128 x 128 split-K / persistent launch when (a) the 128 x 128 tiling has at most 1 280 tiles (small batches), or (b, exact fp32 only)
 *         K <= 1024 whatever the size; 2 = rule (a) only, 0 = neither.  The same K order per output element: a re-association at most.
 * key 43 (1; launch) the dilated 3x3 layers whose launch skips the filter rows that lie in the zero padding (ASPP d = 18, model.py:610-651, on
 *         64-row tiles) skip the padded filter COLUMNS as well: the GEMM rows of an image run through three column zones (left tap padded |
 *         both taps inside or both padded | right tap padded) as a serpentine, a tile multiplies only the filter columns its zones meet.
 *         The skipped taps multiply zeros: same bits unless the launch is split over K (then a re-association); 0 = rows only.
 * key 51 (1; plan - the stand-alone quber_op_conv3x3_winograd reads the process default per call) dilated layers of the three-kernel Winograd
 *         pipeline: the d phases of an axis share tiles, one zero slot between two phases, where that needs fewer tiles than a tiling of every
 *         phase on its own (rows and columns decide independently; 640x480: res5.1/.2 conv2 and ASPP d = 6 / 12 run 88 / 96 / 108 / 132 tiles per
 *         image instead of 96 / 128 / 144 / 144).  Which layers take Winograd, and with which tile, is not affected.  The same arithmetic per
 *         tile; a pixel falls into another tile, so the last bits move as on a ragged frame; 0 = per phase everywhere, the bits before the key.
 * key 52 (1; plan) CGNet contexts (with_network = 3): a context-guided block (foreground_segmentation/cgnet.py:231-261) as two kernels -
 *         cg_joint (1x1 + BN + PReLU into LDS with a halo, both depthwise 3x3, BN + PReLU of the concatenation, per-tile channel sums) and
 *         cg_apply (global mean, the two fully connected layers, channel scale, residual), csrc/cgnet.hip; 0 = 1x1 convolution, two depthwise
 *         launches, cg_sums and cg_apply: five launches per block, the same arithmetic but for the K order of the 1x1.
 * key 53 (0; plan) Depth Seeding Network contexts (with_network = 4): the second half of an ESP module (uois/src/networks.py:108-125) as one kernel,
 *         esp_branches (csrc/dsn.hip): the five dilated 3x3 convolutions of t on v_mfma_f32_16x16x4_f32, the running sums d2, d2 + d4, ... kept in the
 *         accumulators, the residual, the store and per-tile GroupNorm sums; 0 = five convolution launches into temporaries + esp_merge.  The same
 *         convolutions; a running sum is continued in the accumulator instead of rounded and added (profiles/dsn_ab.md decides the default).
 * key 54 (1; plan) Region Refinement Network contexts (with_network = 5): decoder.last_conv and fg_module, with nothing non-linear between them, as ONE
 *         3x3 feature_dim -> 1 filter, w'[c][ky][kx] = sum_o wfg[o] W[o][c][ky][kx], b' = sum_o wfg[o] bias[o] (float64 on the host, rounded once), run by
 *         rrn_head3 (csrc/rrn.hip) on decoder.layer5's output from LDS tiles with a halo; 0 = the convolution with its bias, then the 1x1 head kernel.
 *         The collapsed form rounds the filter once more and the features once less (profiles/rrn_ab.md decides the default).
 * Process-only keys (quber_set_tuning): key 2 = give the stand-alone conv ops a split-K workspace (value != 0) or drop it (0);
 * key 11 = stand-alone conv op: dilated 3x3 layers in tap-major K order with the zero-padding filter rows skipped;
 * key 12 = stand-alone conv ops: quber_config.compute_dtype of the launch (1 = bf16 / 2 = fp16 operands, 3 = bf16x3);
 * key 26 = timing harness: quber_op_conv3x3_winograd reuses the transformed filters of its previous call (u / ws untouched) */
int quber_set_option(quber_ctx* ctx, int32_t key, int32_t value);
int quber_get_option(quber_ctx* ctx, int32_t key, int32_t* value);
void quber_set_tuning(int32_t key, int32_t value);
/* Host view of the work distribution of a persistent convolution launch (csrc/conv_persist.hip), for the CPU tests: no GPU.
 * _segments: the work list of block `block` of a launch of `blocks` blocks over `tiles` tiles of `k_slices` K-slices each
 *   (min_share = shortest K share of the remainder, 0 = remainder tiles whole): up to cap x (tile, first slice, end slice,
 *   workspace slot or -1 for a whole tile); returns their number.
 * _fixup: for remainder tile j of XCD run xcd: its tile index and the workspace slots the fix-up pass sums, in order;
 *   returns their number, 0 when the tile is computed whole, -1 past the remainder. */
int32_t quber_debug_persistent_segments(int32_t tiles, int32_t blocks, int32_t k_slices, int32_t min_share, int32_t block,
                                        int32_t* out4, int32_t cap);
int32_t quber_debug_persistent_fixup(int32_t tiles, int32_t blocks, int32_t k_slices, int32_t min_share, int32_t xcd, int32_t j,
                                     int32_t* tile, int32_t* slots, int32_t cap);
/* Host view of a device workspace layout, for the CPU tests: no GPU.  The bytes the layout walk of entry `which` ends at:
 * 0 mask NMS (b frames, n masks), 1 COCO matching (b, n ground truths, flag = iou_type), 2 scene perturbation (b, n = N + P rows,
 * m = max_masks), 3 mean shift, 4 Gaussian mean shift, 5 zoom-in, 6 losses (b = max_batch each), 7 clean-up, 8 post-processing
 * (b, n = top_k); h x w frames; arguments an entry does not name are ignored.  -1: unknown `which`. */
int64_t quber_debug_ws_bytes(int32_t which, int32_t b, int32_t n, int32_t m, int32_t h, int32_t w, int32_t flag);
/* the launch plan of quber_forward, in execution order (after the input pre-processing kernel):
 * kind 0 = convolution, 1 = GroupNorm, 2 = other; flops = algorithmic FLOPs at batch 1 */
int quber_num_ops(quber_ctx* ctx);
int quber_op_info(quber_ctx* ctx, int index, const char** name, int32_t* kind, double* flops, int32_t* launches);
/* stand-alone convolution: y = act((conv(x, w) * scale + shift) + residual), NHWC, weights OIHW on the device */
int quber_op_conv2d(const float* dev_x, int32_t batch, int32_t h, int32_t w, int32_t cin, const float* dev_w_oihw,
                    int32_t cout, int32_t ksize, int32_t stride, int32_t pad, int32_t dil, const float* dev_scale,
                    const float* dev_shift, const float* dev_residual, int32_t relu, float* dev_packed_scratch,
                    float* dev_y, void* stream);
/* the 1x1 / stride 1 convolution of the fp16 data path (compute_dtype 2 with fp16 tensors in HBM): x [batch][h][w][cin],
 * w [cout][cin], residual and y [batch][h][w][cout] are fp16, scale / shift fp32; cin a multiple of 64 (test hook: the
 * network reaches this kernel only through quber_forward). */
int quber_op_conv1x1_f16(const void* dev_x, int32_t batch, int32_t h, int32_t w, int32_t cin, const void* dev_w_oi,
                         int32_t cout, const float* dev_scale, const float* dev_shift, const void* dev_residual,
                         int32_t relu, void* dev_y, void* stream);
/* a convolution of the fp16 data path on fp16 tensors: x [batch][h][w][cin] (cin a multiple of 8; kmode 1: of 64), w_packed [cout][Kpad]
 * (Kpad = k*k*cin rounded up to a multiple of 64, rows zero-filled) in the kernels' K order - kmode 0: k = (tap, channel); kmode 1:
 * k = (channel / 64, tap, channel % 64) - residual and y fp16, scale /
 * shift fp32; gn_sums (or null): f64 [batch][gn_groups][2], the sums and sums of squares of the stored outputs per norm group
 * are ADDED to it (the GroupNorm statistics the network's convolutions gather in their epilogue).  Test hook: the layers of
 * maskrefiner/modeling/backbone/resnet.py:395-449, 472-485 reach these kernels through quber_forward. */
int quber_op_conv2d_f16(const void* dev_x, int32_t batch, int32_t h, int32_t w, int32_t cin, const void* dev_w_packed,
                        int32_t cout, int32_t ksize, int32_t stride, int32_t pad, int32_t dil, int32_t kmode,
                        const float* dev_scale, const float* dev_shift, const void* dev_residual, int32_t relu,
                        double* dev_gn_sums, int32_t gn_groups, void* dev_y, void* stream);
/* one 1x1 GEMM over two inputs: out = relu?(y . w[:, :mid] + x[::stride, ::stride] . w[:, mid:] + shift), NHWC;
 * y [batch][oh][ow][mid], x [batch][h2][w2][cin], w [cout][mid + cin], `dev_ones` = cout ones (the kernel's affine scale).
 * Needs the op workspace (key 2) and fp32 / bf16x3 arithmetic (key 12 = 0 / 3). */
int quber_op_conv1x1_dual(const float* dev_y, const float* dev_x, int32_t batch, int32_t oh, int32_t ow, int32_t mid,
                          int32_t h2, int32_t w2, int32_t cin, int32_t stride, const float* dev_w, const float* dev_shift,
                          const float* dev_ones, int32_t cout, int32_t relu, float* dev_out, void* stream);
/* the same for a 3x3 / stride 1 / pad = dilation convolution through the Winograd F(m x m, 3x3) path, m = 2, 4 or 6
 * (cin >= 128 and a multiple of 32, cout >= 128): with P = (m+2)^2, dev_u_scratch holds P*cout*cin floats (transformed
 * weights), dev_ws at least P * batch * dil^2 * ceil(ceil(h/dil)/m) * ceil(ceil(w/dil)/m) * (cin + cout) floats.
 * m = 4 with cin <= key 27, 32 | cout and a dev_ws of at least 36 * cout * cin floats: the single-kernel form (key 25). */
int quber_op_conv3x3_winograd(const float* dev_x, int32_t batch, int32_t h, int32_t w, int32_t cin,
                              const float* dev_w_oihw, int32_t cout, int32_t dil, int32_t m, const float* dev_scale,
                              const float* dev_shift,
                              int32_t relu, float* dev_u_scratch, float* dev_ws, int64_t ws_floats, float* dev_y,
                              void* stream);
/* The three convolution ops above in the forms the plan launches them - test hooks: arguments -> launch parameters -> launcher.  A view is (pointer
 * to its first channel, cs = elements between two pixels, gs = elements between two launch groups) over batch x h x w x channels of fp32; arithmetic
 * per key 12, split-K workspace per key 2, as the dense ops.  No op allocates (but the bf16x3 weight planes) or synchronises.
 *   quber_op_conv2d_view            G groups: weights OIHW [G][cout][cin][k][k] (packed per group into dev_packed_scratch [G][cout][Kpad]), scale / shift
 *                                   [G][cout] or null, residual view or null; dev_gn_sums (or null): f64 [G][batch][gn_groups][2], the sums and sums of
 *                                   squares of the stored outputs are ADDED to it
 *   quber_op_conv3x3_winograd_view  the same through Winograd F(m x m, 3x3); x_gs may be 0 (the groups share one input); dev_n_stats (or null): the
 *                                   input is normalised on load, relu?((x - mean) * rstd * gamma + beta), from the sums f64 [G][batch][n_groups][2] of
 *                                   quber_op_gn_stats, gamma / beta of group g at g * n_param_gs; dev_y may be dev_x where the three-kernel pipeline runs;
 *                                   dev_u_scratch: G * P * cout * cin floats; the single-kernel form as in the dense op, with a dev_ws that also holds
 *                                   G * 36 * cout * cin floats
 *   quber_op_conv1x1_dual_view      G groups of the dual 1x1 GEMM: dense tensors at the group strides given, w [G][cout][mid + cin] at w_gs, shift / ones at ss_gs
 * quber_debug_*_route: host only - nothing is launched, no device queried.  The launcher itself walks its decisions for the launch the op would make
 * of these arguments on the current process keys and reports them: out[12] = kernel, sums, rows and channels of a tile, K partitions, log2 pieces of a
 * split tail, tiles, blocks, K slices, shortest share (the arguments of quber_debug_persistent_segments), packed axis, shared input transform.
 *   kernel: 1 one tile per block, 2 ... with the split-K reduce, 3 persistent, 4 Winograd pipeline, 5 single Winograd kernel, 6 conv_x8
 *   sums:   0 none requested; the kernel's number: gathered by it; 7: a separate pass over the output
 *   x_off / y_off / res_off: element offsets of the views in 16-byte-aligned buffers (res_off < 0: no residual); workspace: as with key 2 set; cus:
 *   compute units to assume; Winograd: tiles = per image, rows of a tile = tiles per block of the kernel that gathers the sums, K partitions = passes */
int quber_op_conv2d_view(const float* dev_x, int32_t x_cs, int64_t x_gs, const float* dev_w_oihw, const float* dev_scale, const float* dev_shift,
                         const float* dev_residual, int32_t res_cs, int64_t res_gs, float* dev_y, int32_t y_cs, int64_t y_gs, int32_t groups_of_launch,
                         int32_t batch, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t ksize, int32_t stride, int32_t pad, int32_t dil,
                         int32_t relu, double* dev_gn_sums, int32_t gn_groups, float* dev_packed_scratch, void* stream);
int quber_debug_conv_route(int32_t x_off, int32_t x_cs, int64_t x_gs, int32_t affine, int32_t res_off, int32_t res_cs, int64_t res_gs, int32_t y_off,
                           int32_t y_cs, int64_t y_gs, int32_t groups_of_launch, int32_t batch, int32_t h, int32_t w, int32_t cin, int32_t cout,
                           int32_t ksize, int32_t stride, int32_t pad, int32_t dil, int32_t gn_groups, int32_t workspace, int32_t cus, int32_t* out12);
int quber_op_conv3x3_winograd_view(const float* dev_x, int32_t x_cs, int64_t x_gs, const float* dev_w_oihw, const float* dev_scale,
                                   const float* dev_shift, float* dev_y, int32_t y_cs, int64_t y_gs, int32_t groups_of_launch, int32_t batch, int32_t h,
                                   int32_t w, int32_t cin, int32_t cout, int32_t dil, int32_t m, int32_t relu, double* dev_gn_sums, int32_t gn_groups,
                                   const double* dev_n_stats, const float* dev_n_gamma, const float* dev_n_beta, int32_t n_param_gs, int32_t n_groups,
                                   int32_t n_relu, float n_eps, float* dev_u_scratch, float* dev_ws, int64_t ws_floats, void* stream);
int quber_debug_winograd_route(int32_t x_cs, int64_t x_gs, int32_t y_cs, int64_t y_gs, int32_t in_place, int32_t groups_of_launch, int32_t batch,
                               int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t dil, int32_t m, int32_t gn_groups, int32_t norm_groups,
                               int64_t ws_floats, int32_t* out12);
int quber_op_conv1x1_dual_view(const float* dev_y, int64_t y_gs, const float* dev_x, int64_t x_gs, const float* dev_w, int64_t w_gs,
                               const float* dev_shift, const float* dev_ones, int32_t ss_gs, float* dev_out, int64_t out_gs, int32_t groups_of_launch,
                               int32_t batch, int32_t oh, int32_t ow, int32_t mid, int32_t h2, int32_t w2, int32_t cin, int32_t stride, int32_t cout,
                               int32_t relu, void* stream);
int quber_debug_dual_route(int64_t y_gs, int64_t x_gs, int64_t w_gs, int32_t ss_gs, int64_t out_gs, int32_t groups_of_launch, int32_t batch, int32_t oh,
                           int32_t ow, int32_t mid, int32_t h2, int32_t w2, int32_t cin, int32_t stride, int32_t cout, int32_t workspace, int32_t cus,
                           int32_t* out12);
int quber_op_groupnorm(const float* dev_x, int32_t batch, int32_t h, int32_t w, int32_t c, int32_t groups,
                       const float* dev_gamma, const float* dev_beta, float eps, int32_t relu,
                       double* dev_stats_scratch, float* dev_y, void* stream);
int quber_op_bilinear(const float* dev_x, int32_t batch, int32_t h, int32_t w, int32_t c, int32_t oh, int32_t ow,
                      float* dev_y, void* stream);
int quber_op_maxpool3x3s2(const float* dev_x, int32_t batch, int32_t h, int32_t w, int32_t c, float* dev_y,
                          void* stream);
/* The glue kernels between the convolutions (csrc/elementwise.hip), each on explicit NHWC views - test hooks: the network reaches
 * them only through quber_forward.  A view is (pointer to its first channel, cs = elements between two pixels, gs = elements between
 * two launch groups, es = element size: 4 fp32, 2 fp16) over batch x h x w x c; a view the launcher refuses (mixed element types, c or cs
 * no multiple of 4, a base address off the 4-element boundary) returns the launcher's error.  No op allocates or synchronises.
 *   quber_debug_gn_pixels_per_block   pixels per block the GroupNorm statistics (stats_pass != 0) / apply pass give a tensor (host only)
 *   quber_op_gn_stats                 dev_stats f64 [G][batch][groups][sum, sum of squares] += the sums of x; zero != 0 clears it first
 *   quber_op_gn_apply                 y = relu?((x - mean) * rstd * gamma + beta) from those sums; gamma / beta of launch group g at g * param_gs
 *   quber_op_maxpool_view             3x3 / stride 2 / pad 1 -> [batch][(h+1)/2][(w+1)/2][c]
 *   quber_op_bilinear_view            F.interpolate(mode="bilinear", align_corners=False) to oh x ow
 *   quber_op_avgpool                  mean over the pixels -> y [batch][c] at stride y_cs
 *   quber_op_add_channels / quber_op_copy_channels    y = a + b / y = x on channel slices
 *   quber_op_predictors               n <= 5 1x1 heads on c = 32 / 64 features in one launch: logits -> planar dev_q [batch][q_nch][h*w] from
 *                                     plane q_ch0[j]; act[j] 1 = softmax / 2 = sigmoid of the head's cout[j] logits -> act_dst[j] (pixel stride
 *                                     act_cs; null = none).  feat, w, bias, act_dst, cout, q_ch0, act: HOST arrays of n entries
 *   quber_op_upsample_logits          planar bilinear x scale of dev_q [batch][nch][h][w], top-left oh x ow kept; planes whose bit of mul_mask is
 *                                     set are multiplied by scale
 *   quber_op_preprocess               u8 HWC bgr (+ depth, streams = 2) + f32 planar offsets -> x [streams][batch_cap][h][w][x_c];
 *                                     mean6 / std6: HOST arrays */
int32_t quber_debug_gn_pixels_per_block(int32_t hw, int32_t c, int32_t batch, int32_t groups_of_launch, int32_t stats_pass);
int quber_op_gn_stats(const void* dev_x, int32_t x_cs, int64_t x_gs, int32_t es, int32_t batch, int32_t h, int32_t w, int32_t c,
                      int32_t groups_of_launch, int32_t groups, double* dev_stats, int32_t zero, void* stream);
int quber_op_gn_apply(const void* dev_x, int32_t x_cs, int64_t x_gs, int32_t x_es, void* dev_y, int32_t y_cs, int64_t y_gs, int32_t y_es,
                      int32_t batch, int32_t h, int32_t w, int32_t c, int32_t groups_of_launch, int32_t groups, const double* dev_stats,
                      const float* dev_gamma, const float* dev_beta, int32_t param_gs, float eps, int32_t relu, void* stream);
int quber_op_maxpool_view(const void* dev_x, int32_t x_cs, int64_t x_gs, int32_t x_es, void* dev_y, int32_t y_cs, int64_t y_gs, int32_t y_es,
                          int32_t batch, int32_t h, int32_t w, int32_t c, int32_t groups_of_launch, void* stream);
int quber_op_bilinear_view(const void* dev_x, int32_t x_cs, int32_t x_es, void* dev_y, int32_t y_cs, int32_t y_es, int32_t batch, int32_t h,
                           int32_t w, int32_t c, int32_t oh, int32_t ow, void* stream);
int quber_op_avgpool(const void* dev_x, int32_t x_cs, int32_t x_es, void* dev_y, int32_t y_cs, int32_t y_es, int32_t batch, int32_t h, int32_t w,
                     int32_t c, void* stream);
int quber_op_add_channels(const void* dev_a, int32_t a_cs, int32_t a_es, const void* dev_b, int32_t b_cs, int32_t b_es, void* dev_y, int32_t y_cs,
                          int32_t y_es, int32_t batch, int32_t h, int32_t w, int32_t c, void* stream);
int quber_op_copy_channels(const void* dev_x, int32_t x_cs, int32_t x_es, void* dev_y, int32_t y_cs, int32_t y_es, int32_t batch, int32_t h,
                           int32_t w, int32_t c, void* stream);
int quber_op_predictors(int32_t n, const void* const* dev_feat, const float* const* dev_w, const float* const* dev_bias, void* const* dev_act_dst,
                        const int32_t* cout, const int32_t* q_ch0, const int32_t* act, int32_t c, int32_t feat_cs, int32_t es, int32_t batch,
                        int32_t h, int32_t w, float* dev_q, int32_t q_nch, int32_t act_cs, void* stream);
int quber_op_upsample_logits(const float* dev_q, float* dev_out, int32_t batch, int32_t nch, int32_t h, int32_t w, int32_t scale, int32_t oh,
                             int32_t ow, uint32_t mul_mask, void* stream);
int quber_op_preprocess(const uint8_t* dev_bgr, const uint8_t* dev_depth, const float* dev_offsets, void* dev_x, int32_t x_c, int32_t es,
                        int32_t batch, int32_t batch_cap, int32_t h, int32_t w, const float* mean6, const float* std6, int32_t streams,
                        void* stream);
/* Depth Seeding Network of UOIS-Net-3D on a with_network = 4 context: xyz -> foreground logits, centre offsets, centre votes, classes.
 *   dev_xyz f32 [B][3][H][W] planar (x, y, z in metres, as compute_xyz delivers them; NaN allowed).  The network's input is xyz with NaN -> 0
 *   and, when bit 0 of flags is set, y negated (eval/base_model.py:496-498); no other flag bit is defined.
 *   -> dev_fg_logits f32 [B][3][H][W] (fg_module, classes background / table / objects), dev_offsets f32 [B][3][H][W] (cd_module),
 *      dev_votes f32 [B][3][H][W] = cleaned xyz + offsets (one float32 add: DSNWrapper.cluster's predicted centres),
 *      dev_fg_classes u8 [B][H][W] = the FIRST maximal logit (the reference takes argmax(softmax(logits)): where float32 softmax rounds two distinct
 *      logits to one probability it returns the lower index instead), dev_fg u8 [B][H][W] = (class == 2).
 *   Any output pointer may be NULL.  dev_votes / dev_fg are the layouts quber_gms_cluster reads.  Everything runs on `stream`; no host copy, no
 *   memset node, no allocation: the call can be captured into a graph. */
int quber_dsn_forward(quber_ctx* ctx, const float* dev_xyz, int32_t batch, int32_t flags, float* dev_fg_logits, float* dev_offsets, float* dev_votes,
                      uint8_t* dev_fg_classes, uint8_t* dev_fg, void* stream);
/* the same forward with a HIP-event pair around every op of the plan (benchmark use; tools/dsn_ab.py): synchronises `stream`, then writes the milliseconds
 * of op i (quber_op_info) to op_ms[i], quber_num_ops doubles on the host */
int quber_dsn_forward_profiled(quber_ctx* ctx, const float* dev_xyz, int32_t batch, int32_t flags, float* dev_fg_logits, float* dev_offsets,
                               float* dev_votes, uint8_t* dev_fg_classes, uint8_t* dev_fg, void* stream, double* op_ms);
/* quber_dsn_forward from a depth image: dev_z f32 [B][H][W] in metres (NaN / inf / 0 / negative pass through the arithmetic) and cam = (fx, fy, cx, cy)
 * on the host, read during the call.  The plan's first op back-projects and packs in one kernel; the point cloud never exists as a tensor of its own.
 *   convention 0 "pinhole" (eval/base_model.py:489-495): float64, x = ((col - cx) / fx) * z, y = ((row - cy) / fy) * z, rounded to float32 once
 *   convention 1 "uois" (compute_xyz): float32 with the camera rounded to float32 first, x = ((col - cx) * z) / fx, y = (((H - 1 - row) - cy) * z) / fy
 * every operation rounded on its own (quber_amd/camera.py xyz_np is the contract).  NaN -> 0 and bit 0 of flags apply to the result, as in
 * quber_dsn_forward; the outputs are those of quber_dsn_forward.  The camera must be finite, the focal lengths other than zero. */
int quber_dsn_forward_depth(quber_ctx* ctx, const float* dev_z, int32_t batch, int32_t flags, const double* cam, int32_t convention, float* dev_fg_logits,
                            float* dev_offsets, float* dev_votes, uint8_t* dev_fg_classes, uint8_t* dev_fg, void* stream);
int quber_dsn_forward_depth_profiled(quber_ctx* ctx, const float* dev_z, int32_t batch, int32_t flags, const double* cam, int32_t convention,
                                     float* dev_fg_logits, float* dev_offsets, float* dev_votes, uint8_t* dev_fg_classes, uint8_t* dev_fg, void* stream,
                                     double* op_ms);

/* The kernels of the Depth Seeding Network (csrc/dsn.hip), each on explicit fp32 views - test hooks: the network reaches them only through
 * quber_dsn_forward.  An NHWC view is (pointer to its first channel, cs = elements between two pixels).  An ESP module of c channels splits them as
 * n = c / 5 (integer), n1 = c - 4 n.  A refused view returns an error and launches nothing; no op allocates or synchronises.
 *   quber_op_dsn_pack      planar xyz f32 [batch][3][h][w] -> dev_x8 NHWC with 8 channels (x, y, z, five zeros) and dev_clean planar; NaN -> 0, then
 *                          y negated when bit 0 of flags is set; either destination may be NULL
 *   quber_op_xyz_from_depth  depth f32 [batch][h][w] + cam (fx, fy, cx, cy; host) -> dev_xyz_raw planar f32 [batch][3][h][w] with NaN kept, and / or the
 *                          two outputs quber_op_dsn_pack makes of it (conventions and flags: quber_dsn_forward_depth); any destination may be NULL, not all;
 *                          no multiple-of-16 rule
 *   quber_op_esp_tiles     tiles (runs of 64 pixels) per frame of the partials buffer f64 [batch][tiles][groups][2] = (sum, sum of squares)
 *   quber_op_esp_kernel    host only: ceil(n1 / 16), the instance of the one-kernel form that quber_op_esp_branches and the plan (option key 53 = 1)
 *                          launch for n1 channels of dilated1, in 1..13; 0 where there is none (n1 < 1 or n1 > 208): both then refuse
 *   quber_op_esp_packed_floats / quber_op_esp_pack  the five OIHW filters (dilated1 [n1][n][3][3], the others [n][n][3][3]) -> the operand order
 *                          of quber_op_esp_branches, a buffer of quber_op_esp_packed_floats(n1) floats
 *   quber_op_esp_branches  out = [x +] [d1 | d2 | d2 + d4 | (d2 + d4) + d8 | ((d2 + d4) + d8) + d16], dK = 3x3 of t with dilation = padding = K, zero
 *                          padding of t; t: n channels on a channel stride of at least 16 ceil(n1 / 16) in aligned groups of 4 - the channels
 *                          n .. 16 ceil(n1 / 16) are read and multiplied by zero: they must be finite; n1 in 1..208 (quber_op_esp_kernel);
 *                          dev_x may be NULL; also writes the partials of out for `groups` norm groups (1..64, dividing c)
 *   quber_op_esp_merge     the same out and partials from the five convolutions as tensors (d1: n1 channels on d1_cs; the others n channels on d_cs),
 *                          added in the reference's order
 *   quber_op_esp_stats     partials added in tile order -> dev_stats f64 [batch][groups][2], the layout quber_op_gn_apply reads
 *   quber_op_dsn_head      features NHWC (c a multiple of 4) -> logits = wfg [3][c] f, offsets = wcd [3][c] f, votes = dev_clean + offsets, classes =
 *                          the first maximal logit, fg = (class == 2); planar outputs as in quber_dsn_forward, any may be NULL */
int32_t quber_op_esp_tiles(int32_t h, int32_t w);
int quber_op_esp_kernel(int n1);
int64_t quber_op_esp_packed_floats(int32_t n1);
int quber_op_dsn_pack(const float* dev_xyz, int32_t batch, int32_t h, int32_t w, int32_t flags, float* dev_x8, float* dev_clean, void* stream);
int quber_op_xyz_from_depth(const float* dev_z, int32_t batch, int32_t h, int32_t w, const double* cam, int32_t convention, int32_t flags, float* dev_xyz_raw,
                            float* dev_x8, float* dev_clean, void* stream);
int quber_op_esp_pack(const float* dev_w1, const float* dev_w2, const float* dev_w4, const float* dev_w8, const float* dev_w16, int32_t n, int32_t n1,
                      float* dev_packed, void* stream);
int quber_op_esp_branches(const float* dev_t, int32_t t_cs, const float* dev_x, int32_t x_cs, float* dev_out, int32_t out_cs, int32_t batch, int32_t h,
                          int32_t w, int32_t c, int32_t groups, const float* dev_packed, double* dev_partials, int32_t tiles, void* stream);
int quber_op_esp_merge(const float* dev_d1, int32_t d1_cs, const float* dev_d2, const float* dev_d4, const float* dev_d8, const float* dev_d16,
                       int32_t d_cs, const float* dev_x, int32_t x_cs, float* dev_out, int32_t out_cs, int32_t batch, int32_t h, int32_t w, int32_t c,
                       int32_t groups, double* dev_partials, int32_t tiles, void* stream);
int quber_op_esp_stats(const double* dev_partials, int32_t batch, int32_t tiles, int32_t groups, double* dev_stats, void* stream);
int quber_op_dsn_head(const float* dev_f, int32_t f_cs, int32_t batch, int32_t h, int32_t w, int32_t c, const float* dev_clean, const float* dev_wfg,
                      const float* dev_wcd, float* dev_logits, float* dev_offsets, float* dev_votes, uint8_t* dev_classes, uint8_t* dev_fg, void* stream);

/* Region Refinement Network of UOIS-Net-3D on a with_network = 5 context: n crops of side S = height = width -> foreground logits, refined masks.
 *   dev_rgb_crop f32 [n][3][S][S] planar, standardised (what quber_rrn_crop writes), dev_mask_crop u8 [n][S][S] (non-zero = the initial mask); the
 *   network's input is their concatenation, the mask as 0.0 / 1.0 (segmentation.py:262-264).  n in 1..max_batch; GroupNorm is per sample, so a
 *   caller may chunk its crops in any way (the reference's step_size is only that).
 *   -> dev_logits f32 [n][S][S] (fg_module of the decoder's features), dev_refined u8 [n][S][S] = (logit > logit_threshold), 0 / 1.  Either may be
 *      NULL, not both.  logit_threshold = float32(log(t / (1 - t))) of the probability threshold t, computed by the host; exactly 0 for t = 0.5.
 *      Stated deviation: the reference compares float32 sigmoid(logit) > t, which differs for |logit| below about 1e-7 at t = 0.5.
 *   Everything runs on `stream`; no host copy, no memset node, no allocation: the call can be captured into a graph.
 *   quber_forward and quber_dsn_forward refuse such a context, and quber_rrn_forward every other. */
int quber_rrn_forward(quber_ctx* ctx, const float* dev_rgb_crop, const uint8_t* dev_mask_crop, int32_t n, float logit_threshold, float* dev_logits,
                      uint8_t* dev_refined, void* stream);
/* the same forward with a HIP-event pair around every op of the plan (benchmark use; tools/rrn_ab.py): synchronises `stream`, then writes the milliseconds
 * of op i (quber_op_info) to op_ms[i], quber_num_ops doubles on the host */
int quber_rrn_forward_profiled(quber_ctx* ctx, const float* dev_rgb_crop, const uint8_t* dev_mask_crop, int32_t n, float logit_threshold, float* dev_logits,
                               uint8_t* dev_refined, void* stream, double* op_ms);
/* rrn_preprocess / rrn_postprocess of uois/src/segmentation.py:329-423 on the device, on any context of the FRAME size (one without a network will do; these
 * two are their own test hooks).  slots i32 [n_slots][2] = (frame, id), ascending by frame, at most 254 per frame; rois i32 [batch][n_ids][4] = (x0, y0, x1, y1)
 * inclusive as quber_zoom_rois writes them (the padded box of rrn_preprocess is the same expression).  A slot whose frame or id is out of range, or whose
 * ROI is empty or leaves the frame, is no crop: zero crops, nothing painted.
 *   quber_rrn_crop    dev_bytes u8 [batch][H][W][3] (the image as the caller holds it), dev_ids i32 [batch][H][W] (compact: 0 none, 1..n_ids), dev_table f32
 *                     [3][256]: table[c][v] = float32((v / 255. - mean[c]) / std[c]) computed by the host in float64 - byte channel c takes mean[c]; the
 *                     reference standardises the BGR bytes of cv2.imread with its RGB-ordered means (eval/base_model.py:460-462), and so does a caller
 *                     that hands over BGR bytes.  -> dev_rgb_crop f32 [n_slots][3][S][S]: the standardised ROI resized bilinearly with align_corners
 *                     (F.upsample_bilinear) in float32, per axis sc = float32(n - 1) / float32(S - 1), src = float32(dst) * sc, i0 = min(int(src), n - 1),
 *                     i1 = min(i0 + 1, n - 1), l1 = src - i0, l0 = 1 - l1, out = l0y * (l0x * a + l1x * b) + l1y * (l0x * c + l1x * d), every operation
 *                     rounded on its own; dev_mask_crop u8 [n_slots][S][S] = (ids == id) at the nearest index min(int(floorf(float32(dst) *
 *                     (float32(in) / float32(out)))), in - 1) (F.upsample_nearest), 0 / 1.  2 <= crop <= 512.  No allocation.
 *   quber_rrn_paste   dev_refined u8 [n_slots][S][S] (non-zero = refined foreground), dev_z f32 [batch][H][W] (depth; NaN counts as 0) -> every crop
 *                     resized back to its ROI by the nearest index; dev_keys f32 [n_slots] = float32(sum / count) of z under the resized mask, the sum
 *                     in float64 from block partials added in a fixed order (0 for a slot without a refined pixel, which paints nothing, and for one whose z holds both infinities); a frame's slots
 *                     painted in descending key, equal keys in ascending slot order (the stable sorted(reverse=True)); the surviving initial ids compacted in
 *                     ascending order (np.unique) -> dev_out_ids i32 [batch][H][W], dev_out_masks u8 [batch][n_masks][H][W] of 0 / 255 (n_masks 1..254; a
 *                     final id above n_masks has no plane), dev_source i32 [batch][n_masks] = the initial id of each refined mask, 0 beyond the count,
 *                     dev_report i32 [batch][4] = (refined masks, initial masks that vanished, pixels painted, pixels painted over).  Every output is
 *                     overwritten by every call; no memset node, no host copy, no floating-point atomics: two runs give the same bits.  Its workspace is
 *                     allocated by the first call on a context (for max_batch frames) and kept: that call cannot be captured into a graph. */
int quber_rrn_crop(quber_ctx* ctx, const uint8_t* dev_bytes, const int32_t* dev_ids, const int32_t* dev_slots, const int32_t* dev_rois, const float* dev_table,
                   int32_t batch, int32_t n_ids, int32_t n_slots, int32_t crop, float* dev_rgb_crop, uint8_t* dev_mask_crop, void* stream);
int quber_rrn_paste(quber_ctx* ctx, const uint8_t* dev_refined, const int32_t* dev_slots, const int32_t* dev_rois, const float* dev_z, int32_t batch,
                    int32_t n_ids, int32_t n_slots, int32_t crop, int32_t n_masks, int32_t* dev_out_ids, uint8_t* dev_out_masks, int32_t* dev_source,
                    float* dev_keys, int32_t* dev_report, void* stream);
/* The network-side kernels of csrc/rrn.hip on explicit fp32 views - test hooks: the network reaches them only through quber_rrn_forward.  A refused view
 * returns an error and launches nothing; no op allocates or synchronises.
 *   quber_op_rrn_pack    planar crops f32 [batch][3][h][w] + mask u8 [batch][h][w] -> dev_x8 NHWC with 8 channels (c0, c1, c2, mask != 0, four zeros)
 *   quber_op_rrn_head    features NHWC (c a multiple of 4 on a stride f_cs) -> logit = wfg [c] . f, a chain of c fused multiply-adds; dev_logits f32 /
 *                        dev_refined u8 = (logit > thr), [batch][h][w], either may be NULL
 *   quber_op_rrn_head3   the same outputs from a 3x3 filter dev_w9 [9][c] (tap-major) + bias with zero padding: 16 x 16 tiles staged in LDS with a halo */
int quber_op_rrn_pack(const float* dev_rgb, const uint8_t* dev_mask, int32_t batch, int32_t h, int32_t w, float* dev_x8, void* stream);
int quber_op_rrn_head(const float* dev_f, int32_t f_cs, int32_t batch, int32_t h, int32_t w, int32_t c, const float* dev_wfg, float thr, float* dev_logits,
                      uint8_t* dev_refined, void* stream);
int quber_op_rrn_head3(const float* dev_f, int32_t f_cs, int32_t batch, int32_t h, int32_t w, int32_t c, const float* dev_w9, float bias, float thr,
                       float* dev_logits, uint8_t* dev_refined, void* stream);

/* The kernels of the CGNet foreground network (csrc/cgnet.hip), each on explicit fp32 NHWC views - test hooks: the network reaches them only
 * through quber_forward of a with_network = 3 context.  A view is (pointer to its first channel, cs = elements between two pixels); c = 64
 * or 128.  A refused view returns an error and launches nothing; no op allocates or synchronises.
 *   quber_op_cgnet_tiles   tiles per frame of the partials buffer f64 [batch][tiles][c]: joint != 0: the 8 x 8 tiles quber_op_cgnet_joint writes,
 *                          0: the 64-pixel runs quber_op_cgnet_sums writes
 *   quber_op_cgnet_joint   joi = prelu(bn2([dw3x3(t) | dw3x3 dilated by dil (t)])), t = prelu(bn1(W1 x)) with zero padding OF t; dil 1..4;
 *                          dev_w1 [c/2][c], scale1 / shift1 / slope1 [c/2], dev_wloc / dev_wsur [c/2][3][3], scale2 / shift2 / slope2 [c];
 *                          x in aligned groups of 4 channels; also writes this launch's partials
 *   quber_op_cgnet_sums    the partials of a tensor
 *   quber_op_cgnet_apply   y = sigmoid(fc2 relu(fc0 mean + b0) + b2) with mean = (partials added in tile order) / (h w), hidden = c / r <= 8 units;
 *                          out = [x +] joi * y (dev_x may be NULL); dev_mean / dev_y f32 [batch][c] receive the mean and y (may be NULL);
 *                          views in aligned groups of 4 channels */
int32_t quber_op_cgnet_tiles(int32_t h, int32_t w, int32_t joint);
int quber_op_cgnet_joint(const float* dev_x, int32_t x_cs, float* dev_joi, int32_t joi_cs, int32_t batch, int32_t h, int32_t w, int32_t c, int32_t dil,
                         const float* dev_w1, const float* dev_scale1, const float* dev_shift1, const float* dev_slope1, const float* dev_wloc,
                         const float* dev_wsur, const float* dev_scale2, const float* dev_shift2, const float* dev_slope2, double* dev_partials,
                         int32_t tiles, void* stream);
int quber_op_cgnet_sums(const float* dev_x, int32_t x_cs, int32_t batch, int32_t h, int32_t w, int32_t c, double* dev_partials, int32_t tiles,
                        void* stream);
int quber_op_cgnet_apply(const float* dev_joi, int32_t joi_cs, const float* dev_x, int32_t x_cs, float* dev_out, int32_t out_cs, int32_t batch,
                         int32_t h, int32_t w, int32_t c, int32_t hidden, const double* dev_partials, int32_t tiles, const float* dev_fc0,
                         const float* dev_b0, const float* dev_fc2, const float* dev_b2, float* dev_mean, float* dev_y, void* stream);

/* The kernels of the LMFFNet foreground network (csrc/lmff.hip), each on explicit fp32 NHWC views - test hooks: the network reaches them
 * only through quber_forward of a with_network = 2 context.  A view is (pointer to its first channel, cs = elements between two pixels)
 * over batch x h x w x c; scale / shift / slope are per-channel device arrays of c floats.  A view the launcher refuses returns the
 * launcher's error and launches nothing.  No op allocates or synchronises.
 *   quber_op_lmff_preprocess   u8 HWC bgr + depth [pixels][3] -> x [pixels][8]: (bgr / 255 - mean) / std in float64, depth / 255, two zeros
 *   quber_op_lmff_dwconv       y = prelu(bn(depthwise 3x3 of x, dilation = padding = dil)); dev_w9 [c][3][3].  16-byte accesses when c, both
 *                              cs and both base addresses allow it, one channel per lane otherwise
 *   quber_op_lmff_pool         mode 0: AvgPool2d(3, 2, 1) (divisor 9), mode 1: MaxPool2d(2, 2), h x w -> oh x ow; a max pool whose window
 *                              leaves the map (h < 2 oh or w < 2 ow) is refused
 *   quber_op_lmff_affine       y = prelu((a [+ b]) * scale + shift); dev_b may be NULL
 *   quber_op_lmff_pmca         dev_wts f32 [batch][c] = sigmoid(fc2(prelu(fc0(dw2x2(adaptive_avg_pool 2x2 (x)) + global_avg_pool(x))))), c = 64 or
 *                              128 in aligned groups of 4 (anything else is refused); dev_sums: f64 [batch][c][5] scratch
 *   quber_op_lmff_scale        y[b][pixel][ch] = dev_wts[b][ch] * x[b][pixel][ch]
 *   quber_op_lmff_gate         planar dev_q [batch][c][h*w] = o * sigmoid(att) of two NHWC views */
int quber_op_lmff_preprocess(const uint8_t* dev_bgr, const uint8_t* dev_depth, int64_t pixels, float* dev_x, void* stream);
int quber_op_lmff_dwconv(const float* dev_x, int32_t x_cs, float* dev_y, int32_t y_cs, int32_t batch, int32_t h, int32_t w, int32_t c, int32_t dil,
                         const float* dev_w9, const float* dev_scale, const float* dev_shift, const float* dev_slope, void* stream);
int quber_op_lmff_pool(const float* dev_x, int32_t x_cs, float* dev_y, int32_t y_cs, int32_t batch, int32_t h, int32_t w, int32_t c, int32_t oh,
                       int32_t ow, int32_t mode, void* stream);
int quber_op_lmff_affine(const float* dev_a, int32_t a_cs, const float* dev_b, int32_t b_cs, float* dev_y, int32_t y_cs, int32_t batch, int32_t h,
                         int32_t w, int32_t c, const float* dev_scale, const float* dev_shift, const float* dev_slope, void* stream);
int quber_op_lmff_pmca(const float* dev_x, int32_t x_cs, int32_t batch, int32_t h, int32_t w, int32_t c, const float* dev_w2x2, const float* dev_fc0,
                       const float* dev_alpha, const float* dev_fc2, float* dev_wts, double* dev_sums, void* stream);
int quber_op_lmff_scale(const float* dev_x, int32_t x_cs, const float* dev_wts, float* dev_y, int32_t y_cs, int32_t batch, int32_t h, int32_t w,
                        int32_t c, void* stream);
int quber_op_lmff_gate(const float* dev_o, int32_t o_cs, const float* dev_att, int32_t att_cs, float* dev_q, int32_t batch, int32_t h, int32_t w,
                       int32_t c, void* stream);
/* a9 alone, on a caller-supplied centre list in ANY order - group_pixels(ctr, offsets) of post_processing.py:44-76
 * (quber_postprocess derives its centres from the centre plane, i.e. always in raster order; the reference's function takes
 * whatever list it is handed).  The grouping kernel quber_postprocess launches, unchanged.
 *   dev_logits f32 [B][n_planes][H][W]: plane 0 foreground logit (a pixel is grouped iff sigmoid(x).round() == 1),
 *              planes 2, 3 the (y, x) offsets; dev_centers i32 [B][cap][2] (y, x), dev_ncenters i32 [B], cap <= 254
 *   -> dev_ids u8 [B][H][W]: 0 = background, 1..K = index of the nearest centre + 1 (first index wins ties), 255 = foreground
 *      of a frame without centres; dev_area u32 [B][256]: pixels per id */
int quber_op_group_pixels(const float* dev_logits, int32_t n_planes, int32_t batch, int32_t h, int32_t w, int32_t cap,
                          const int32_t* dev_centers, const int32_t* dev_ncenters, uint8_t* dev_ids, uint32_t* dev_area,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif
