/*
 * hhrnet.h -- C-ABI of the MI355X-native HigherHRNet forward + associative-embedding decode.
 *
 * The reference (thawro/pytorch-human-pose) has no FFI: its plug-in points are Python
 * classes.  Each entry point below names the reference interface it stands in for
 * (paths relative to the reference's src/); the Python shims in
 * pytorch-human-pose_amd/keypoints/ bind them with ctypes.
 *
 * Conventions: every function returning int returns 0 on success, non-zero on error with
 * a thread-local message in hh_last_error().  All *device* pointers are plain HIP device
 * addresses (e.g. torch.Tensor.data_ptr()); `stream` is a hipStream_t passed as void*
 * (NULL = the legacy default stream).  Calls are asynchronous on `stream` unless noted.
 * A handle is not re-entrant; different handles may be used from different threads.
 *
 * The `typedef struct hh_x { ... } hh_x;` blocks and the HH_* macros / enumerators below are the ONLY definition of the descriptor
 * tables, limits and flags: the kernels under csrc/ include this file and take these types, and the Python binding parses these
 * bodies into numpy dtypes (_lib.struct_dtype).  Keep a body to what that parser reads: fixed-width scalars, int, long long, float,
 * double, pointers, arrays bounded by a number or an HH_* macro defined above the struct, earlier hh_* structs by value; no
 * bit-fields, unions or function pointers.  Where the library and Python had spelled a field differently the spelling here won,
 * except for two that were changed here without moving a byte: hh_render_prim.rgb[3] (was r, g, b) and hh_jpeg_win_desc as
 * { hh_jpeg_dec_desc d; hh_jpeg_window window; } (was the ten fields of the decode descriptor written out again).
 */
#ifndef HHRNET_H
#define HHRNET_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HH_ABI_VERSION 3
#define HH_DTYPE_BF16 1 /* bf16 MFMA operands, fp32 accumulate, bf16 NHWC activations */
#define HH_DTYPE_FP8 2  /* OCP e4m3 MFMA operands (v_mfma_f32_32x32x64_f8f6f4), fp32 accumulate, e4m3 NHWC activations with one
                           scale per tensor, e4m3 weights with one scale per output channel; needs hh_calibrate (BASELINE.json
                           configs[4]; no reference precedent: the reference infers in fp32, keypoints/model.py:79-83)     */
#define HH_DTYPE_F16 3  /* fp16 MFMA operands (v_mfma_f32_32x32x16_f16), fp32 accumulate, fp16 NHWC activations, packed weights fp16,
                           outputs fp32 as for bf16: the format every GPU forward of the reference runs in (torch.autocast(float16)).
                           The plan -- ops, lanes, fusions, workspace -- is the bf16 handle's; the kernels are the same templates over
                           the element type.  Semantics, those of HH_ACT_F16 below (the same element traits):
                             - every store rounds to nearest even;
                             - a value beyond +-65504 becomes +-inf.  It is NOT saturated: an overflowing activation shows in the
                               outputs as inf / NaN instead of as a plausible wrong map (check a checkpoint's range with
                               hh_set_taps / hh_tap_read maxima against 65504);
                             - subnormals are kept by every store and every fp32 <-> fp16 conversion.  Whether the f16 MFMA keeps
                               subnormal INPUTS is what the subnormal case of tests/test_gpu_train_f16_lattice.py decides;
                             - BatchNorm-folded weights are rounded to fp16 on the host: one below 2^-14 in magnitude loses mantissa
                               bits, one below 2^-25 becomes zero, and one beyond +-65504 makes hh_finalize FAIL with the parameter's
                               name (it does not load an inf).  Biases / BN shifts stay fp32.
                           hh_calibrate on such a handle is an error.  A handle created under a debug switch that reaches a kernel
                           without an fp16 form (HH_NO_STEM_FUSED, HH_BB32=tile) is refused by hh_create.
                           (One new constant, no new symbol: HH_ABI_VERSION stays 3.)                                         */

typedef struct hh_net hh_net;
typedef struct hh_decoder hh_decoder;

int hh_abi_version(void);
const char *hh_last_error(void);

/* ------------------------------------------------------------------ network forward
 * hh_create: HigherHRNet(num_kpts, C).__init__ -- keypoints/architectures/higher_hrnet.py:47-64
 * (backbone: hrnet.py:342-376).  Parameters are addressed by the reference's state-dict
 * key names (1810 keys for W32).                                                        */
hh_net *hh_create(int num_kpts, int C, int dtype);
void hh_destroy(hh_net *net);

/* ClassificationHRNet(C, num_classes) -- classification/architectures/hrnet.py:64-74 (BASELINE.json configs[0]):
 * the same backbone with a 4-scale last fusion + ClassificationHead.  Parameters/keys as the reference's
 * state dict (hh_num_params/hh_load_weights/hh_finalize work on the handle); forward writes logits [B,num_classes]. */
hh_net *hh_create_classifier(int C, int num_classes, int dtype);
int hh_forward_classifier(hh_net *net, const float *images, int B, int H, int W, float *logits, void *stream);

/* state_dict() introspection: key names and shapes in the reference's order. */
int hh_num_params(const hh_net *net);
const char *hh_param_name(const hh_net *net, int index);
int hh_param_shape(const hh_net *net, int index, int64_t shape[4]); /* returns ndim (0 for scalars) */

/* load_state_dict(): base/model.py:155-175. `host` is fp32 (int64 counters are ignored);
 * unknown names and shape mismatches are errors (strict=True semantics).                */
int hh_load_weights(hh_net *net, const char *name, const float *host, const int64_t *shape, int ndim);
/* Folds eval-mode BatchNorm (eps 1e-5) into the preceding conv, packs kernel-layout weights in the handle's
 * element type and uploads them.  Fails if any parameter was never loaded, and on an HH_DTYPE_F16 handle if a
 * folded weight exceeds the fp16 range (the message names the parameter).  Synchronous.  */
int hh_finalize(hh_net *net);

/* fp8 handles only: sets the per-tensor activation scales from `rounds` (0 = 2) forwards over a calibration batch
 * (images [B,3,H,W] fp32 NCHW, device).  Every layer's output maximum is taken from its fp32 epilogue values and mapped to
 * 240 of e4m3's 448; maxima accumulate over calls until the next hh_finalize.  Synchronous.  hh_forward on an fp8 handle
 * fails until this has run.                                                                                              */
int hh_calibrate(hh_net *net, const float *images, int B, int H, int W, int rounds, void *stream);

/* The host-side OCP e4m3fn codec the fp8 weight packer uses (round to nearest even, saturating at +-448, NaN = 0x7f);
 * exported so that it can be checked against an independent implementation without a GPU.                                */
int hh_e4m3_encode(const float *x, int64_t n, unsigned char *out);
int hh_e4m3_decode(const unsigned char *x, int64_t n, float *out);

/* Allocates the activation workspace for inputs up to [B,3,H,W] (H, W multiples of 32).
 * Synchronous; hh_forward calls it implicitly when the shape grows.                     */
int hh_reserve(hh_net *net, int B, int H, int W);
int64_t hh_workspace_bytes(const hh_net *net);

/* HigherHRNet.forward: higher_hrnet.py:66-81.
 *   images          [B,3,H,W]        fp32 NCHW (device)
 *   init_heatmaps   [B,2K,H/4,W/4]   fp32 NCHW (device): stage-0 heatmaps = [:, :K], tags = [:, K:]
 *   deconv_heatmaps [B,K,H/2,W/2]    fp32 NCHW (device): stage-1 heatmaps
 * use_graph != 0 replays a cached hipGraph when (pointers, shape) repeat.               */
int hh_forward(hh_net *net, const float *images, int B, int H, int W, float *init_heatmaps, float *deconv_heatmaps,
               int use_graph, void *stream);

/* Multi-lane execution (default on): independent resolution branches / fusion outputs are launched on
 * internal HIP streams forked from and joined back to `stream` with events.  0 = everything on `stream`. */
int hh_set_multi_lane(hh_net *net, int enable);

/* Static check of the multi-lane schedule (no GPU needed): every read-after-write, write-after-read and write-after-write
 * pair of ops on different lanes must be ordered by a join/dependency edge.  0 = no hazard.                              */
int hh_debug_check_plan(const hh_net *net);

/* Algorithmic conv/deconv FLOPs (2*MACs) of one forward at this shape -- SURVEY.md §8d.  */
double hh_forward_flops(const hh_net *net, int B, int H, int W);

/* Live per-launch timing for bench.py's roofline line: when enabled, hh_forward runs eagerly and brackets
 * every convolution launch with HIP events recorded on `stream`.  hh_profile_get(i) returns the i-th
 * launch since hh_profile_enable: kernel instantiation index, algorithmic FLOPs (2*MACs) and bytes (input + output
 * (+ residual) + weights, each once: no halo re-reads) of that launch,
 * elapsed milliseconds, and the state-dict prefix of the layer.  hh_conv_config describes an
 * instantiation as {KS, S, KC, NT, WC, PT, TW}.  `ms` = hipEventElapsedTime of the start / stop events the launch itself
 * was given (hipExtLaunchKernelGGL): the runtime fills them from the dispatch packet's begin / end timestamps, the same
 * clock pair rocprofv3's kernel trace reports.  `kernel_ms` is first-workgroup-start to last-workgroup-end read by the
 * kernel itself from the device wall clock (hipDeviceAttributeWallClockRate): shorter, it leaves out the dispatch ramp
 * and the end-of-kernel write-back; only with hh_profile_enable(net, 2) -- the same-address atomics that stamp it lengthen
 * each launch by 3-5 us as the dispatch timestamps see it, so mode 1 (events only) is the one to quote -- else -1.     */
int hh_profile_enable(hh_net *net, int enable);
int hh_profile_count(const hh_net *net);
int hh_profile_get(hh_net *net, int index, int *cfg, double *flops, double *bytes, float *ms, float *kernel_ms, const char **layer);
/* mode 2 only, kernels that stamp it (the fused 32-channel block): the core clock workgroup 0 of launch `index` ran at, from
 * s_memtime / s_memrealtime deltas inside the kernel; 0 = not stamped.  Under load the chip holds this well below its 2.4 GHz. */
int hh_profile_clock(hh_net *net, int index, double *ghz);
int hh_conv_config(int cfg, int out[7]);
/* 1 if instantiation `cfg` runs its K loop on two LDS buffers (conv_mfma.hip, DB), 0 if not, -1 for an unknown index */
int hh_conv_config_double_buffered(int cfg);

/* Kernel micro-benchmark used by tools/conv_bench.py (not on the hot path): `iters` back-to-back launches of
 * convolution instantiation `cfg` on random bf16 data, HIP-event timed; returns ms per launch.        */
int hh_debug_conv_bench(int cfg, int B, int Hin, int Win, int cin, int cout, int with_res, int relu, int iters,
                        float *ms_per_launch, unsigned long long *stamps16, int ref_cfg, float *max_diff);

int hh_debug_bb_bench(int B, int H, int W, int iters, float *ms_per_launch, unsigned long long *stamps64);
/* the two fused 32-channel block kernels (tile form / producer-consumer form) on the same input: output difference and time */
int hh_debug_bb_compare(int B, int H, int W, int iters, float *max_diff, float *ms_classic, float *ms_pc);

/* Static check of the fused 32-channel block's tile geometry (basicblock_fused_pc.hip; no GPU needed, nothing is launched): makes
 * the launcher's tile choice for a [B,H,W,32] map (tall: 0 = per-image tiles, 1 = the batch as one tall image where that needs fewer
 * tiles, 2 = wherever the launcher allows it; num_cus: the grid limit) and walks every tile through the kernel's own row arithmetic.
 * counts[0] = row segments (one output row of one column tile) no tile stores, counts[1] = segments stored more than once,
 * counts[2] = input rows a stored row needs that its tile's patch reads as zero or from elsewhere, counts[3] = the same for the
 * rows of the intermediate (conv1) tile.  All four are 0 for a correct launch.  Non-zero return: the launcher refuses the shape.
 * (Additive diagnostic entry point: like hh_conv_config_double_buffered it leaves HH_ABI_VERSION at 3.)                       */
int hh_debug_bb_cover(int B, int H, int W, int tall, int num_cus, int64_t counts[4]);

/* The fused stem (stem_fused.hip) alone, on the handle's packed stem weights (bf16 and fp16 handles of the default plan, after
 * hh_finalize): images [B,3,H,W] fp32 NCHW (device) -> out16 [B,H/4,W/4,64] raw 16-bit words in the handle's element type (device).
 * H and W need only be multiples of 4, so the kernel's partial tiles and ragged widths can be run, which hh_forward's multiples of 32
 * never reach; a handle created under HH_POISON_LDS=1 fills every CU's LDS with NaN patterns in front of the launch.
 * (Additive diagnostic entry point: it leaves HH_ABI_VERSION at 3.)                                                              */
int hh_debug_stem_fused(hh_net *net, const float *images, int B, int H, int W, void *out16, void *stream);

/* Debug taps (parity tests): when enabled, hh_forward copies selected intermediate
 * activations; hh_tap_read converts one to fp32 NCHW on the host. Names follow the
 * reference module paths, e.g. "stages.2.blocks.3#1" = output 1 of backbone.stages[2].blocks[3]. */
int hh_set_taps(hh_net *net, int enable);
int hh_num_taps(const hh_net *net);
const char *hh_tap_name(const hh_net *net, int index);
int hh_tap_shape(const hh_net *net, int index, int64_t shape[4]); /* N,C,H,W of the last forward */
int hh_tap_read(hh_net *net, int index, float *host_nchw);        /* synchronous */

/* InferenceKeypointsModel.prepare_input on the device (keypoints/model.py:70-76; resize-align warp of
 * base/transforms/utils.py:89-97): `image_hwc` uint8 RGB [h,w,3] (device), `dst_to_src` the INVERSE of the 2x3 affine
 * that get_affine_transform returns (cv2.warpAffine maps every destination pixel back; hh_invert_affine), output fp32 NCHW [3,H,W] = Normalize(ToTensor(warpAffine(image))).
 * The warp is OpenCV 4.9's 8-bit INTER_LINEAR path restated (fixed-point coordinates and weights, see hh_warp_affine_u8);
 * parity with cv2 itself is UNPINNED (no cv2 in the build or run images): checked against oracle/transforms.py. */
int hh_preprocess_u8(const unsigned char *image_hwc, int h, int w, const double dst_to_src[6], float *out_nchw, int H, int W,
                     const float mean[3], const float stdv[3], void *stream);

/* The same for a batch of raw images of any sizes in ONE launch (the batched caller behind the reference's per-image `__call__`,
 * bin/eval.py:18-49): the images lie in one device buffer, image i at `images_base + descs[i].offset` with its own size and affine;
 * `descs_dev` is a DEVICE array (the caller ships it with the pixels in the same host->device copy); out_nchw is [n,3,H,W]. */
typedef struct hh_image_desc {
    long long offset;     /* bytes from images_base */
    int h, w;             /* raw image size */
    double dst_to_src[6]; /* as in hh_preprocess_u8 */
} hh_image_desc;
int hh_preprocess_u8_batch(const unsigned char *images_base, const hh_image_desc *descs_dev, int n, float *out_nchw, int H, int W,
                           const float mean[3], const float stdv[3], void *stream);

/* Flip test-time augmentation, keypoints/model.py:85-94 (COCO_FLIP_INDEX: keypoints/transforms.py:11).
 * hh_flip_images: out = flip(images, W axis), fp32 NCHW.
 * hh_flip_merge : hm[b,k] = (hm[b,k] + flip_w(hm_flipped[b, perm[k]])) / 2  in place for `hm`
 *                 (K channels each, batch strides in elements), and
 *                 tags_out[b,k] = flip_w(tags_flipped[b, perm[k]]).                       */
int hh_flip_images(const float *images, float *out, int B, int C, int H, int W, void *stream);
int hh_flip_merge(float *hm, int64_t hm_bstride, const float *hm_flipped, int64_t hmf_bstride, const float *tags_flipped,
                  int64_t tf_bstride, float *tags_out, int64_t to_bstride, const int32_t *perm_host, int B, int K,
                  int h, int w, void *stream);

/* ------------------------------------------------------------------ decode
 * hh_decoder_create: MPPEHeatmapParser(num_kpts, max_num_people, det_thr, tag_thr)
 * -- keypoints/grouping.py:67-78.  Thresholds are doubles because the reference compares
 * float32 scores / float64 distances against Python floats.                             */
hh_decoder *hh_decoder_create(int num_kpts, int max_people, double det_thr, double tag_thr);
void hh_decoder_destroy(hh_decoder *dec);
int hh_decoder_reserve(hh_decoder *dec, int B, int H, int W, int E); /* H, W = full (model-input) resolution */
/* By default hh_decode skips the NMS / top-k work of every 16x16-pixel block whose averaged half-resolution source values cannot
 * exceed det_thr (and only keeps peaks above it): such pixels cannot contribute a candidate that survives match_by_tag's
 * `score > det_thr` filter (grouping.py:98-102), so joints / scores / num_people are unchanged, bit for bit; the no-group
 * fallback's top-1 candidates are then recomputed from the maps for the flagged images.  What changes is the candidate list
 * itself (sub-threshold entries are missing): enable = 1 takes the exhaustive path (the stage average materialised, every
 * 60x60 tile processed), which hh_decoder_read_topk (the reference's full top_k) needs.                                    */
int hh_decoder_set_exact_topk(hh_decoder *dec, int enable);

/* InferenceKeypointsResult.from_preds aggregation + MPPEHeatmapParser.parse, batched:
 * keypoints/results.py:225-238 + keypoints/grouping.py:252-283.
 *   hm_q   [B,K,hq,wq]   fp32, batch stride hm_q_bstride elements (channel-slice views allowed)
 *   hm_h   [B,K,2hq,2wq] fp32
 *   tags_q E pointers (host array of device pointers), each [B,K,hq,wq]
 * Outputs (device): joints [B,max_people,K,3+E] (x, y, score, tag...; zero rows = no person),
 * scores [B,max_people], num_people [B], flags [B] (may be NULL).  Bit-exact with the reference on identical inputs
 * (ties between equal candidate scores are ordered by ascending pixel index).
 * flags[b] bits: HH_DECODE_FALLBACK = no group was formed and the one person returned is the best-candidate pseudo-person
 * of grouping.py:262-269 (the reference's arrays are float64 there with the score 0.01 as a double; the device arrays stay
 * float32 and the host shim widens them); HH_DECODE_SOLVER_GUARD = the assignment solver stopped at its iteration guard,
 * the image's result is invalid and the caller must raise.                                                           */
#define HH_DECODE_FALLBACK 1
#define HH_DECODE_SOLVER_GUARD 2
int hh_decode(hh_decoder *dec, const float *hm_q, int64_t hm_q_bstride, const float *hm_h, int64_t hm_h_bstride,
              const float *const *tags_q, const int64_t *tags_bstride, int E, int B, int hq, int wq, int adjust,
              int refine, float *joints, float *scores, int32_t *num_people, int32_t *flags, void *stream);

/* MPPEHeatmapParser.parse on explicit full-resolution maps (grouping.py:252-283):
 *   hm_full [B,K,H,W] fp32, tags_full [B,K,H,W,E] fp32 (both contiguous).              */
int hh_parse(hh_decoder *dec, const float *hm_full, const float *tags_full, int E, int B, int H, int W, int adjust,
             int refine, float *joints, float *scores, int32_t *num_people, int32_t *flags, void *stream);

/* Training loss of keypoints/loss.py, each fused with its gradient (all pointers device memory, fp32).
 * `scratch`: >= max(1024, 2*B) doubles.  Sums are taken in double in a fixed order (results do not depend on the launch).
 *
 * hh_loss_heatmaps = HeatmapsLoss.forward (loss.py:12-16): *loss = mean((pred - target)^2 * mask[:,None]);
 *   pred [B,K,h,w] with batch stride pred_bstride (a channel slice of a wider tensor is fine), target [B,K,h,w] and
 *   mask [B,h,w] contiguous; if grad != NULL, grad[b,k] (batch stride grad_bstride) = d loss / d pred.  h*w and both batch strides
 *   are multiples of 4 and all four pointers 16-byte aligned (the kernel moves float4); anything else is refused before the launch.
 * hh_loss_ae_grouping = AEGroupingLoss.forward (loss.py:20-61): push_pull[0] = push, [1] = pull, both / batch size
 *   (calculate_loss, loss.py:90-92, scales them by 1e-3 afterwards); tags [B,K,h,w]; joints [B,P,K,3] int32 (x, y, vis)
 *   padded to P people, num_people[b] of them valid, x in [0,w), y in [0,h) wherever vis > 0 (the caller checks);
 *   if grad != NULL, push_scale * d push + pull_scale * d pull is ADDED to grad (zero it first).                    */
int hh_loss_heatmaps(const float *pred, int64_t pred_bstride, const float *target, const float *mask, int B, int K, int h, int w,
                     float *loss, float *grad, int64_t grad_bstride, double *scratch, void *stream);
int hh_loss_ae_grouping(const float *tags, int64_t tags_bstride, const int32_t *joints, const int32_t *num_people, int B, int P, int K,
                        int h, int w, float *push_pull, float *grad, int64_t grad_bstride, float push_scale, float pull_scale,
                        double *scratch, void *stream);

/* The input of the training step built on the device: what the reference's dataset worker does per sample on the host with cv2 and
 * numpy (keypoints/transforms.py:75-172 RandomAffineTransform, :56-72 RandomHorizontalFlip, :37-53 ToTensor + Normalize;
 * keypoints/datasets/coco.py:77-121 HeatmapGenerator), batched.  The raw uint8 pixels, the crowd masks and the descriptors lie in ONE
 * device buffer that the caller ships in one host->device copy; `descs_dev` is a DEVICE array.  The random draws, the matrices and
 * the joints stay on the host (keypoints/train_input.py).  The warp is the one of hh_preprocess_u8 (cv2 parity UNPINNED).
 *
 * hh_train_desc: one sample.  Image uint8 RGB [h,w,3] at batch_base + image_offset, crowd mask uint8 [h,w] with values 0 / 255
 *   (= (mask * 255).astype(np.uint8), transforms.py:159) at batch_base + mask_offset; flip != 0 reverses the destination columns
 *   AFTER the warp (image[:, ::-1], transforms.py:66-68; not folded into the matrix: the fixed-point rounding is per destination
 *   column); the dst_to_src matrices are hh_invert_affine of RandomAffineTransform._get_affine_matrix(...)[:2] for the image
 *   (transforms.py:167-170) and for every heatmap stage (transforms.py:155-156).                                            */
#define HH_TRAIN_MAX_STAGES 4
typedef struct hh_train_desc {
    long long image_offset, mask_offset; /* bytes from batch_base */
    int h, w;                            /* raw image (and mask) size */
    int flip, reserved;
    double image_dst_to_src[6];
    double mask_dst_to_src[HH_TRAIN_MAX_STAGES][6];
} hh_train_desc;
/* out_nchw[b,:,y,x] = Normalize(ToTensor(warpAffine(image_b)))[y, flip_b ? W-1-x : x], fp32 [n,3,H,W]; one launch. */
int hh_train_images_u8_batch(const unsigned char *batch_base, const hh_train_desc *descs_dev, int n, float *out_nchw, int H, int W,
                             const float mean[3], const float stdv[3], void *stream);
/* transforms.py:155-163 + :68 for all stages in one launch: out[k] (HOST array of nstages device pointers) is fp32
 * [n, stage_hw[2k], stage_hw[2k+1]] (stage_hw: HOST ints) = (warpAffine(mask * 255) / 255 > 0.5) as 1.0 / 0.0, then the flip.
 * For a byte v, v / 255 > 0.5 is v >= 128, which is what the kernel tests.                                             */
int hh_train_masks_u8_batch(const unsigned char *batch_base, const hh_train_desc *descs_dev, int n, int nstages, const int *stage_hw,
                            float *const *out, void *stream);
/* The mosaic of the reference's training dataset (keypoints/datasets/coco.py:300-370, get_raw_mosaiced_data; applied with
 * `mosaic_probability`, coco.py:459-462) composed on the device, for all mosaic samples of a batch in ONE launch.  For sample i,
 * tile t (0 top-left, 1 top-right, 2 bottom-left, 3 bottom-right, coco.py:318-325) is resized to S x S and written at
 * (s_y, s_x) = (S * (t / 2), S * (t % 2)): the image (uint8 RGB [h,w,3] at batch_base + image_offset) into the uint8 RGB
 * [2S,2S,3] canvas at batch_base + canvas_image_offset, the crowd mask (uint8 [h,w], 0 / 255, at batch_base + mask_offset) into the
 * uint8 [2S,2S] canvas at batch_base + canvas_mask_offset, which holds 255 where the resized mask is non-zero and 0 elsewhere
 * (cv2.resize(mask * 255) > 0.5, coco.py:328, then (mask * 255).astype(np.uint8), transforms.py:159).  Every canvas byte is written
 * exactly once; deterministic.  The canvases are ordinary sources of hh_train_images_u8_batch / hh_train_masks_u8_batch (a
 * hh_train_desc with h = w = 2S pointing at them), launched afterwards on the same stream.
 *
 * The resize is cv2.resize(src, (S, S)): 8-bit INTER_LINEAR, restated from OpenCV 4.x modules/imgproc/src/resize.cpp (resize(),
 * resizeGeneric_Invoker, HResizeLinear / VResizeLinear with INTER_RESIZE_COEF_BITS = 11).  cv2 is not available where the fixtures
 * are made, so parity with cv2 itself is UNPINNED, as for the warp of hh_preprocess_u8; kernel, tests/cv_resize.py and the golden
 * implement exactly this text (an OpenCV built with IPP or another HAL may take a different 8-bit path):
 *   scale     per axis, scale = 1.0 / ((double)S / src) in double.
 *   area      if h == 2S and w == 2S (both scales exactly 2) OpenCV switches to INTER_AREA: every output byte is
 *             (a + b + c + d + 2) >> 2 of its 2 x 2 source block.  Needs BOTH axes at 2; one alone stays bilinear.
 *             (The bilinear text below gives the same bytes there: all four weights are 1024 and every shift is exact.)
 *   columns   fx = (float)((dx + 0.5) * scale_x - 0.5) (double product and difference, rounded separately, no fused multiply-add),
 *             sx = floor(fx), fx -= sx (fp32); if sx < 0: sx = 0, fx = 0; if sx >= w - 1: sx = w - 1, fx = 0; taps sx and
 *             min(sx + 1, w - 1) with the weights a0 = cvRound((1.f - fx) * 2048), a1 = cvRound(fx * 2048) as shorts (cvRound: to
 *             nearest, half to even); horizontal result H = src[sx] * a0 + src[sx + 1] * a1, an int.
 *   rows      fy, sy formed the same way from dy, scale_y and h, but fy is NOT zeroed at the borders: the two row indices sy and
 *             sy + 1 are clamped into [0, h - 1]; weights b0 = cvRound((1.f - fy) * 2048), b1 = cvRound(fy * 2048).
 *   vertical  with H0, H1 the horizontal results of the two rows:
 *             dst = (uint8)((((b0 * (H0 >> 4)) >> 16) + ((b1 * (H1 >> 4)) >> 16) + 2) >> 2).
 * Validation: `descs_dev` is the DEVICE array the kernel reads; `descs_host` is the caller's HOST copy of the same n descriptors, and
 *   it is what is checked (device memory is never read back).  Returns 1 with hh_last_error set, before any launch, for a null
 *   pointer, n outside 1..65535, S outside 4..HH_MOSAIC_MAX_S or not a multiple of 4 (a thread stores four adjacent pixels as whole
 *   dwords), a canvas offset that is negative or not a multiple of 4, a tile with h or w < 1 or h * w * 3 >= 2^31 (the kernel
 *   indexes one tile's bytes with 32 bits), a negative tile offset.  batch_base itself must be 4-byte aligned.  That tiles and
 *   canvases lie inside the caller's buffer and that no canvas overlaps a tile or another canvas cannot be checked here.
 * (Additive entry point: HH_ABI_VERSION stays 3.)                                                                          */
#define HH_MOSAIC_MAX_S 8192
typedef struct hh_mosaic_tile {
    long long image_offset, mask_offset; /* bytes from batch_base: raw uint8 RGB [h,w,3], crowd mask uint8 [h,w] 0 / 255 */
    int h, w;
} hh_mosaic_tile;
typedef struct hh_mosaic_desc {
    hh_mosaic_tile tile[4];                                /* top-left, top-right, bottom-left, bottom-right */
    long long canvas_image_offset, canvas_mask_offset;     /* bytes from batch_base: uint8 [2S,2S,3] and uint8 [2S,2S] */
} hh_mosaic_desc;
int hh_mosaic_u8_batch(unsigned char *batch_base, const hh_mosaic_desc *descs_dev, const hh_mosaic_desc *descs_host, int n, int S,
                       void *stream);
/* Crowd masks from COCO segmentations (get_crowd_mask, keypoints/datasets/coco.py:167-177, without the COCO API package): the host
 * reduces every segment to a toggle list, the device fills all masks of a batch, of mixed sizes, in ONE launch.
 *
 * The rule.  A segment is one polygon or one run-length list for an image of h x w.  Every segment reduces to a toggle list: a
 * strictly increasing list of uint32 positions in 0 .. h*w.  Pixels are numbered column-major, idx = x*h + y.  Pixel idx is covered
 * by the segment iff the number of toggles <= idx is odd.  A mask byte is 0 where at least one of the mask's segments covers the pixel
 * and 255 elsewhere ((m < 0.5) * 255 of coco.py:177 followed by transforms.py:159): segments combine as a UNION, not XOR.  A toggle
 * equal to h*w is legal and changes nothing.
 *
 * Run-length segment (COCO's {"counts": [c0, c1, ...], "size": [h, w]} of an iscrowd object): runs alternate uncovered / covered,
 *   starting with uncovered; the toggles are the cumulative sums c0, c0+c1, ... without the last; the sum must equal h*w; values that
 *   occur an even number of times (zero-length runs) drop out, values that occur an odd number of times stay once.  (Formed in Python;
 *   `counts` as a compressed string raises.)
 * Polygon segment, xy[2k] doubles, k >= 3 (hh_crowd_polygon_toggles).  This is the COCO API's polygon conversion as recalled from its
 *   C source; the package is not available where the fixtures are made, so parity with it is UNPINNED and this text is the contract:
 *   1. Snap to a grid five times finer: X[j] = (int)(5*x_j + 0.5), Y[j] = (int)(5*y_j + 0.5) (product and sum in double, the
 *      conversion truncates toward zero); X[k] = X[0], Y[k] = Y[0].
 *   2. Walk every edge j -> j+1 as a dense point list (u, v).  dx = |X[j+1]-X[j]|, dy = |Y[j+1]-Y[j]|.  The edge is flipped when
 *      (dx >= dy and X[j] > X[j+1]) or (dx < dy and Y[j] > Y[j+1]); (xs,ys) -> (xe,ye) are the endpoints after swapping if flipped.
 *      If dx >= dy: s = (double)(ye-ys)/dx; for d = 0..dx: t = flipped ? dx-d : d, u = xs+t, v = (int)(ys + s*t + 0.5).
 *      Otherwise:   s = (double)(xe-xs)/dy; for d = 0..dy: t = flipped ? dy-d : d, v = ys+t, u = (int)(xs + s*t + 0.5).
 *      The points therefore always run from vertex j to vertex j+1.  A zero-length edge (dx = dy = 0) contributes the single point
 *      (X[j], Y[j]).  No fused multiply-add.
 *   3. Over the concatenation of all edges' points, for every i >= 1 with u[i] != u[i-1]:
 *      xd = (double)(u[i] < u[i-1] ? u[i] : u[i]-1), then xd = (xd+0.5)/5 - 0.5; skip unless xd is an integer with 0 <= xd <= w-1;
 *      yd = (double)min(v[i], v[i-1]), then yd = (yd+0.5)/5 - 0.5; clamp yd to [0, h], then yd = ceil(yd);
 *      emit the position (int)xd * h + (int)yd.  (The clamp to h puts a toggle on the first position of the next column, which is
 *      why the rule is stated on the linear index and not per column.)
 *   4. Sort the positions and cancel even multiplicities.  The result is the toggle list.
 *
 * hh_crowd_polygon_toggles: host only, no GPU.  Writes the toggle list of one polygon to out[0 .. count) and returns count, or -1 with
 *   hh_last_error set: for a null pointer, k < 3, a non-finite coordinate, h or w outside 1..16384, a coordinate whose five-fold value
 *   5*x + 0.5 leaves the int range, or a list longer than `capacity` entries (nothing is written then).  The walk visits every grid
 *   step of every edge, also of the part of a polygon that lies outside the image: its time is O(5 x perimeter), not O(image).
 * hh_crowd_polygon_capacity: a capacity that always suffices, from the vertices alone in O(k), without walking: the sum over the edges
 *   of min(dx / 5 + 2, 2w) (a position is emitted only where u steps onto a column centre, every fifth grid step).  Same refusals, -1.
 *
 * hh_crowd_masks_u8_batch: mask i is uint8 [h,w] at batch_base + mask_offset (any alignment) with the segments
 *   seg_first .. seg_first + seg_count - 1 of the segment table; segment s has `count` uint32 toggles at batch_base + toggle_offset (a
 *   multiple of 4) and can cover the columns col_first .. col_last only (inclusive; used to cull).  Every mask byte is written exactly
 *   once; deterministic, no atomics; a mask without segments is all 255.  On the stream; nothing is synchronised.
 * Validation: `descs_dev` / `segs_dev` are the DEVICE tables the kernel reads; `descs_host` / `segs_host` are the caller's HOST copies
 *   of the same tables and `host_base` the HOST copy of the staged bytes (the toggles at the offsets the device sees them at): the host
 *   copies are what is checked, device memory is never read back.  Returns 1 with hh_last_error set, before any launch, for a null
 *   pointer (the segment tables may be null when num_segs is 0), n outside 1..65535, negative num_segs, batch_base not 4-byte aligned,
 *   h or w outside 1..16384, a negative mask offset, a segment range outside [0, num_segs), a toggle offset that is negative or not a
 *   multiple of 4, a negative count, toggles not strictly increasing or above h*w, a column range outside the image or one that does
 *   not hold the segment's covered columns.  That masks and toggles lie inside the caller's buffer and that masks do not overlap each
 *   other or the tables cannot be checked here.
 * hh_crowd_mask_config: out = {tile rows, tile columns, threads per workgroup, per-chunk toggle capacity (0: toggles are read in
 *   place, no chunking)}.
 * hh_debug_crowd_masks_host: the same tile walk compiled for the host, one mask into mask[h*w] (mask_offset is not applied), with the
 *   same validation.
 * (Additive entry points: HH_ABI_VERSION stays 3.)                                                                             */
typedef struct hh_crowd_mask_desc {
    long long mask_offset;         /* bytes from batch_base: uint8 [h,w] out */
    int h, w;
    int seg_first, seg_count;      /* this mask's rows of the segment table */
} hh_crowd_mask_desc;
typedef struct hh_crowd_seg_desc {
    long long toggle_offset;       /* bytes from batch_base: `count` uint32 toggles */
    int count;
    int col_first, col_last;       /* inclusive */
    int reserved;
} hh_crowd_seg_desc;
long long hh_crowd_polygon_capacity(const double *xy, int k, int h, int w);
long long hh_crowd_polygon_toggles(const double *xy, int k, int h, int w, unsigned int *out, long long capacity);
int hh_crowd_masks_u8_batch(unsigned char *batch_base, const hh_crowd_mask_desc *descs_dev, const hh_crowd_seg_desc *segs_dev,
                            const hh_crowd_mask_desc *descs_host, const hh_crowd_seg_desc *segs_host, const unsigned char *host_base, int n,
                            int num_segs, void *stream);
int hh_crowd_mask_config(int out[4]);
int hh_debug_crowd_masks_host(unsigned char *mask, const hh_crowd_mask_desc *desc_host, const hh_crowd_seg_desc *segs_host,
                              const unsigned char *host_base, int num_segs);
/* Pose overlays: plot_connections (keypoints/visualization.py:43-90, with draw_elipsis :13-40) for n frames of mixed sizes in ONE
 * launch, on the raw uint8 RGB frames that are on the device for hh_preprocess_u8 anyway.  The host forms the primitive table
 * (keypoints/visualization.py build_primitives here); the kernel does the per-pixel work; the result is bit-identical to this text
 * (tests/render_ref.py restates it in numpy).
 *
 * The drawing rule.  plot_connections(image, coords [P,K,2], scores [P,K], limbs, thr, color_mode, alpha) makes connections_image =
 * image.copy() and draws into it, a later primitive overwriting an earlier one:
 *   for person i ascending: draw size s_i = max(2, int((max_k y - min_k y) / 100)) over ALL K keypoints, drawn or not;
 *     its limbs j ascending (skipped if either end has score < thr), one filled ellipse each;
 *     then its keypoints j ascending (skipped if score < thr; a score equal to thr is drawn), each a filled disc of radius s_i in the
 *     colour followed by a black ring of radius s_i + 1.  Scores and thr are compared as float64.
 *   Coordinates are int() of the float64 value (truncated toward zero).  Colour: palette[i] in mode "person"; in mode "limb"
 *   palette[j], j the limb index for limbs and the keypoint index for keypoints.
 * Then out = addWeighted(image, 1 - alpha, connections_image, alpha, 0) over every pixel, covered or not.
 * Rasterisation (this project's rule; all centres and radii are integers; pixel (x, y), dx = x - cx, dy = y - cy):
 *   disc     radius r: inside iff dx^2 + dy^2 <= r^2 + r (radius r + 1/2).  Exact in int32.
 *   ring     the reference's circle(radius R = r + 1, thickness 1, black): inside iff R^2 - R < dx^2 + dy^2 <= R^2 + R.  Exact in int32.
 *   ellipse  draw_elipsis on the truncated ends (x1, y1), (x2, y2): centre ((x1 + x2) // 2, (y1 + y2) // 2) with Python's floor
 *            division; Dx = x2 - x1, Dy = y2 - y1; hyp = sqrt(Dx^2 + Dy^2) in float64, dist = int(hyp).  If |Dx| > |Dy|:
 *            (a, b) = (dist // 2, s_i) and (c, s) = (Dx, Dy) / hyp; otherwise (a, b) = (s_i, dist // 2) and (c, s) = (Dy, -Dx) / hyp;
 *            (c, s) = (1, 0) when hyp == 0.  (The reference's arctan2 angle without a libm call: sqrt and division are correctly
 *            rounded, so the table is the same on every machine.)  c and s are rounded once to fp32.  With A = 2a + 1, B = 2b + 1
 *            (semi-axes a + 1/2 and b + 1/2: a zero axis still draws a line one pixel wide), every operation in fp32, rounded on
 *            its own, in this order:  fx = (float)dx, fy = (float)dy;  u = fx * c + fy * s;  v = fy * c - fx * s;
 *            p = (2 * u) * B;  q = (2 * v) * A;  lhs = p * p + q * q;  ab = A * B;  rhs = ab * ab;  inside iff lhs <= rhs.
 *   blend    per channel rintf(img * w0 + conn * w1) in fp32, the two products and the sum rounded separately, clamped to 0..255;
 *            w0 = (float)(1.0 - alpha), w1 = (float)alpha, both formed in double on the host.
 *   Primitives are clipped to the frame; centres may lie outside it and may be negative.
 * Stated deviation from OpenCV: cv2.ellipse rounds the angle to whole degrees and fills a polygon approximation (ellipse2Poly),
 *   cv2.circle is a midpoint circle.  Parity of the covered pixel set with cv2 itself is therefore UNPINNED: it differs on boundary
 *   pixels only; the size of that difference is not measured, and cv2 is not available where the fixtures are made.  Everything in
 *   front of the rasteriser IS pinned to the reference by tests/golden/render.npz, written by the reference's own plot_connections
 *   with recording stand-ins for cv2.ellipse / circle / addWeighted: which primitives, in what order, where, how large, which colour,
 *   the thresholds, the truncations and the blend weights.
 *
 * The primitive table: hh_render_prim rows of 32 bytes, in draw order.  kind: HH_RENDER_DISC (A = B = r), HH_RENDER_RING (A = B = R), HH_RENDER_ELLIPSE (A, B, c, s
 *   as above).  (x0, y0)..(x1, y1) is an inclusive bounding box clipped to 0..16383 that must contain every pixel of the primitive
 *   that can lie in a frame; it is empty (x1 < x0 or y1 < y0) for a primitive wholly outside.  Pixels outside the box are not drawn.
 * The frame descriptors: one hh_render_desc of 48 bytes per frame: the RGB source [h,w,3] at batch_base + src_offset, the output [h,w,3] at batch_base +
 *   dst_offset (another place than any source), the frame's primitives table[prim_offset .. prim_offset + prim_count), the blend
 *   weights, flags bit 0 = store B,G,R instead of R,G,B.  Every output byte is written exactly once, also for prim_count == 0;
 *   deterministic.  Descriptors and table are meant to travel to the device in one copy (the binding does so).
 * Validation: the *_dev arrays are what the kernel reads, the *_host arrays the caller's HOST copies of the same data, and those are
 *   what is checked (device memory is never read back).  Returns 1 with hh_last_error set, before any launch, for a null pointer,
 *   n outside 1..65535, num_prims < 0, descs_dev not 8-byte or prims_dev not 4-byte aligned, a frame with h or w outside 1..16384, a
 *   negative offset, a primitive range outside [0, num_prims), more than HH_RENDER_MAX_PRIMS primitives in one frame (refused, never
 *   capped), a weight that is not finite, an unknown flag or kind, A or B < 1, a disc or ring radius above 32767, a centre beyond
 *   +-2^23, a box outside 0..16383 or reaching further from the centre than 32767 (disc, ring) or 65536 (ellipse): inside the box
 *   dx^2 + dy^2 stays below 2^31 and (float)dx is exact.  That frames lie inside the caller's buffer cannot be checked here.
 * hh_render_config: out[4] = tile height, tile width, primitives culled per chunk, pixels per thread (a workgroup owns one tile and
 *   walks the frame's primitives a chunk at a time, keeping the draw order within and across chunks).
 * hh_debug_render_host: one frame through the same tile walk compiled for the host (src, dst: the frame's own HOST buffers; the
 *   descriptor's offsets are ignored); same validation.  For tests and tools/render_host_check.cpp.
 * hh_resize_u8: cv2.resize(src, (W, H)) for a uint8 [h,w] (channels = 1) or [h,w,3] (channels = 3) device array, the general form of
 *   the resize stated at hh_mosaic_u8_batch above with S replaced by W on the columns and H on the rows: INTER_LINEAR with 11-bit
 *   weights and the 2 x 2 mean iff h == 2H and w == 2W.  Every side in 1..HH_RESIZE_MAX_SIDE; no alignment requirement (dword stores
 *   where a thread's four pixels are 4-byte aligned, bytes otherwise).  Every output byte is written exactly once; deterministic.
 * (Additive entry points: HH_ABI_VERSION stays 3.)                                                                           */
#define HH_RENDER_MAX_PRIMS 4096 /* per frame; 30 people x (19 limbs + 2 x 17 keypoints) = 1590 */
#define HH_RESIZE_MAX_SIDE 16384
enum { HH_RENDER_DISC = 0, HH_RENDER_RING = 1, HH_RENDER_ELLIPSE = 2 };
typedef struct hh_render_prim {
    int32_t cx, cy;
    uint16_t A, B;
    float c, s;
    uint8_t rgb[3], kind; /* the colour as drawn into the R,G,B frame (one array, as every user fills it; the bytes r, g, b of before) */
    int16_t x0, y0, x1, y1;
} hh_render_prim;
typedef struct hh_render_desc {
    long long src_offset, dst_offset;
    int32_t h, w;
    int32_t prim_offset, prim_count;
    float w0, w1;
    int32_t flags, reserved;
} hh_render_desc;
int hh_render_poses_u8_batch(unsigned char *batch_base, const hh_render_desc *descs_dev, const hh_render_desc *descs_host,
                             const hh_render_prim *prims_dev, const hh_render_prim *prims_host, int num_prims, int n, void *stream);
int hh_render_config(int out[4]);
int hh_debug_render_host(const unsigned char *src, unsigned char *dst, const hh_render_desc *desc, const hh_render_prim *prims, int num_prims);
int hh_resize_u8(const unsigned char *src, int h, int w, int channels, unsigned char *dst, int H, int W, void *stream);
/* Text labels: put_txt (utils/image.py:64-119), the one function through which the reference draws all of its text, for n uint8
 * [h,w,3] frames of mixed sizes in ONE launch, IN PLACE, on the frames where they already lie on the device (behind the render and
 * resize launches, in front of the copy back or the JPEG encode).  The host forms the primitive table (keypoints/text.py
 * layout_put_txt here, which restates put_txt's arithmetic in integers); the kernel does the per-pixel work; the result is
 * bit-identical to this text (tests/text_ref.py restates it in numpy).
 *
 * The rule.  put_txt(image, labels, vspace, font_scale, thickness = 1, loc, bg_color, txt_color, alpha) measures every label
 * (width, height) = text_size(label, font_scale), forms txt_h = vspace + sum(height + vspace), txt_w = max(width) + 2 vspace, the
 * box origin (_x, _y) from `loc` (tl tr bl br tc bc; Python's floor division), and draws, in this order:
 *   one BOX   alpha < 1: the rectangle [_x, _x + txt_w) x [_y, _y + txt_h) blended with bg_color; otherwise (alpha == 1 included) the
 *             INCLUSIVE rectangle [_x, _x + txt_w] x [_y, _y + txt_h] filled with bg_color: one pixel wider and taller, as cv2.rectangle
 *             draws it (the reference's quirk, kept);
 *   per label, top to bottom, its characters left to right from the origin (x, y + height) = baseline left, y advancing by height +
 *             vspace: one GLYPH per character that has ink, its bitmap's top-left at (pen + left bearing, baseline + top), the pen
 *             advancing by the character's integer advance.
 * Pixel arithmetic, per channel, on the stored bytes (the caller gives colours in the frame's own channel order):
 *   BOX   opaque: the colour.  Otherwise rintf(img * w0 + bg * w1) in fp32, the two products and the sum rounded separately, clamped
 *         to 0..255; w0 = (float)(1.0 - alpha), w1 = (float)alpha, both formed in double on the host: the blend of the overlays above.
 *   GLYPH with coverage c = atlas[offset + row * bitmap width + column]: (pix * (255 - c) + col * c + 127) / 255 in integers.
 *   Primitives apply to a pixel in table order; two put_txt tables concatenated compose two boxes (plot_top_preds' target box).
 * The font: text_size and the glyph bitmaps come from an atlas file that ships with the package (keypoints/data/, rasterised from
 *   DejaVu Sans by tools/make_font_atlas.py): three size classes with cap heights 7, 11 and 15 pixels for font_scale 0.3, 0.5 and 0.7;
 *   another font_scale takes the nearest class (the smaller on a tie); thickness != 1 is refused; a character outside 0x20..0x7E draws
 *   as '?'.  height = the class's cap height, width = the sum of the integer advances.
 * Stated deviations: (1) cv2's Hershey font is not available where this is built and is not guessed at: glyph shapes and, through
 *   the text metrics, box sizes differ from cv2's.  Parity with cv2.putText / getTextSize is UNPINNED.  Everything in front of the
 *   rasteriser IS pinned to the reference by tests/golden/text.npz, written by the reference's own put_txt, plot_top_preds and
 *   draw_labels with a stand-in cv2 that answers getTextSize from this atlas and records rectangle / addWeighted / putText: the box,
 *   the six locs, the alpha == 1 quirk, the weights, the colours, every label's origin and string.  (2) Primitives are clipped to the
 *   frame; the reference's negative slice start, which wraps in numpy, is not imitated.
 *
 * The table: hh_text_prim rows of 32 bytes in draw order.  They ARE hh_render_prim rows (one definition), read as follows.
 *   kind HH_TEXT_BOX:   (x0, y0)..(x1, y1) the inclusive rectangle clipped to the frame (x1 < x0 or y1 < y0: nothing), rgb the colour
 *                       as stored, c = w0, s = w1, A = 1 opaque / 0 blended; B, cx, cy = 0.
 *   kind HH_TEXT_GLYPH: (cx, cy) the bitmap's top-left in the frame (may be negative), A x B the bitmap's width x height, c = the
 *                       offset of its A * B coverage bytes in the atlas (an integer below 2^24, exact in fp32), s = 0, rgb the colour,
 *                       (x0, y0)..(x1, y1) the inclusive rectangle [cx, cx + A - 1] x [cy, cy + B - 1] clipped to the frame.
 * The frame descriptors: one hh_text_desc per frame; they ARE hh_render_desc: the frame [h,w,3], tightly packed (w * 3 bytes a row,
 *   any alignment), at batch_base + src_offset; dst_offset = src_offset (in place); its rows table[prim_offset .. prim_offset +
 *   prim_count); w0, w1, flags and reserved are 0 (there is no flag yet).
 * The tile list: int32 pairs (frame, tile), tile = ty * ceil(w / tile width) + tx, strictly ascending: the tiles that some
 *   primitive's box touches, as hh_text_tiles lists them.  A workgroup takes one pair, culls the frame's primitives to its tile a
 *   chunk at a time keeping the draw order within and across chunks, and neither reads nor writes a pixel that no primitive covers:
 *   work scales with the labelled area.  Descriptors, table and tile list are meant to travel in one copy (the binding does so);
 *   atlas_dev holds the atlas's atlas_len coverage bytes.
 * Validation: on the caller's HOST copies, before any launch; returns 1 with hh_last_error set for a null pointer, n outside
 *   1..65535, num_prims or num_tiles < 0, a misaligned device table, h or w outside 1..16384, a negative offset, dst_offset !=
 *   src_offset, a primitive range outside the table, more than HH_TEXT_MAX_PRIMS primitives in one frame (refused, never capped), a
 *   weight that is not finite, an unknown kind or flag, an empty or inverted glyph bitmap, a glyph whose coverage range leaves the
 *   atlas or whose offset is no such integer, a coordinate beyond +-2^23, a box outside the frame or (glyph) outside its bitmap, a
 *   tile pair that names no tile of its frame or does not ascend.  That frames lie inside the caller's buffer cannot be checked here.
 * hh_text_tiles: validates as above and lists the touched tiles into tiles_host (room for `capacity` pairs); *count = how many there
 *   are (call with capacity 0 to size the list).  num_tiles == 0 launches nothing.
 * hh_text_check: the validation of hh_text_labels_u8_batch alone, on the same host copies; it launches nothing (tests).
 * hh_text_config: out[4] = tile height, tile width, primitives culled per chunk, pixels per thread.
 * hh_debug_text_host: one frame (its own HOST buffer, drawn in place; the descriptor's offsets are ignored) through the same tile
 *   walk compiled for the host; `atlas` is the host copy.  Same validation.  For tests and tools/text_host_check.cpp.
 * (Additive entry points: HH_ABI_VERSION stays 3.)                                                                           */
#define HH_TEXT_MAX_PRIMS 4096 /* per frame */
enum { HH_TEXT_BOX = 0, HH_TEXT_GLYPH = 1 };
typedef hh_render_prim hh_text_prim;
typedef hh_render_desc hh_text_desc;
int hh_text_labels_u8_batch(unsigned char *batch_base, const hh_text_desc *descs_dev, const hh_text_desc *descs_host, const hh_text_prim *prims_dev,
                            const hh_text_prim *prims_host, int num_prims, int n, const unsigned char *atlas_dev, long long atlas_len,
                            const int32_t *tiles_dev, const int32_t *tiles_host, long long num_tiles, void *stream);
int hh_text_tiles(const hh_text_desc *descs_host, const hh_text_prim *prims_host, int num_prims, int n, long long atlas_len, int32_t *tiles_host,
                  long long capacity, long long *count);
int hh_text_check(const hh_text_desc *descs_host, const hh_text_prim *prims_host, int num_prims, int n, long long atlas_len, const int32_t *tiles_host,
                  long long num_tiles);
int hh_text_config(int out[4]);
int hh_debug_text_host(unsigned char *frame, const hh_text_desc *desc, const hh_text_prim *prims, int num_prims, const unsigned char *atlas,
                       long long atlas_len);
/* Segmentation overlays: the per-object cv2.fillPoly + cv2.drawContours(thickness 1) + addWeighted(overlay, 0.4, image, 0.6) of the
 * reference's plot_raw (keypoints/datasets/coco.py:383-398) for n uint8 RGB [h,w,3] frames of mixed sizes in ONE launch, on frames that
 * are on the device already.  The host forms the tables (keypoints/sample_plot.py seg_tables here); the kernel does the per-pixel
 * work; the result is bit-identical to this text (tests/seg_overlay_ref.py restates it in numpy).
 *
 * The tables.  Shapes: int32 rows of HH_SEG_SHAPE_INTS = 8, {kind, colour = r | g << 8 | b << 16, a, b, c, d, 0, 0}, in draw order.
 *   HH_SEG_FILL  a = the first toggle as an index into the toggle table, b = the toggle count, c..d = an inclusive column range that
 *                holds every covered column (used to cull).
 *   HH_SEG_LINE  (a, b) -> (c, d) = the integer endpoints (xa, ya) -> (xb, yb) as given; they may lie outside the frame and be negative.
 * Toggles: one uint32 table; a fill's toggles are strictly increasing positions in 0 .. h*w on the column-major pixel index
 *   idx = x * h + y, the toggle lists of hh_crowd_polygon_toggles above.
 * The rule.  overlay = image.  The frame's rows are walked in order and a later row overwrites an earlier one: a pixel ends up in the
 * colour of the LAST row that covers it.
 *   fill   pixel (x, y) of the h x w frame is covered iff the number of the row's toggles <= x * h + y is odd (the crowd mask's predicate).
 *   line   dx = |xb - xa|, dy = |yb - ya|; every product in int64; floor_div rounds toward minus infinity.
 *          dx == dy == 0: the single pixel (xa, ya).
 *          dx >= dy: the ends are swapped if xa > xb; for x = xa..xb: y = ya + floor_div(2 (x - xa) (yb - ya) + dx, 2 dx).
 *          otherwise: the ends are swapped if ya > yb; for y = ya..yb: x = xa + floor_div(2 (y - ya) (xb - xa) + dy, 2 dy).
 *          (The nearest pixel of the minor coordinate, an exact tie toward plus infinity AFTER the swap: a line and its reverse draw the
 *          same pixels.)  Pixels outside the frame are not drawn.
 *   blend  over EVERY pixel, covered or not, per channel out = rintf(image * w0 + overlay * w1) in fp32, the two products and the sum
 *          each rounded on their own, half to even, clamped to 0..255: the blend of hh_render_poses_u8_batch.  w0 is the image's weight,
 *          w1 the overlay's (keypoints/visualization.py blend_weights(0.4) for the reference's figure).  An uncovered pixel p is therefore
 *          rintf(p * w0 + p * w1), not p: addWeighted's behaviour, kept.
 * The frame descriptors: hh_seg_desc ARE hh_render_desc (one definition, no new struct): the source [h,w,3] at batch_base + src_offset,
 *   the output at batch_base + dst_offset, both tightly packed at any alignment; dst equals src (in place) or does not overlap it;
 *   the frame's rows shapes[prim_offset .. prim_offset + prim_count); w0, w1; flags bit 0 = store B,G,R; reserved = 0.  Every output
 *   byte is written exactly once, by one lane, also for prim_count == 0; no atomics; deterministic; nothing outside the frames, the
 *   tables and the toggles is read.  That the frames of a batch do not overlap ONE ANOTHER, and lie inside the caller's buffer,
 *   cannot be checked here.
 * Stated deviations.  cv2.fillPoly's scan conversion and cv2.drawContours' line walk are not available where this is built and are not
 *   guessed at: parity of the boundary pixels with cv2 is UNPINNED.  The fill is COCO's polygon rule on the truncated vertices shifted
 *   by +0.5 (an integer vertex is a pixel centre, cv2's convention); with the contour it leaves no pixel uncovered whose centre lies
 *   strictly inside the polygon (tests/test_sample_plot_cpu.py).  A run-length (iscrowd) object is one fill and no contour; the
 *   reference turns it into polygons with cv2.findContours first.  Everything in front of the rasteriser IS pinned to the reference by
 *   tests/golden/sample_plot.npz: which polygons, their truncation, order, colours and the blend weights.
 * Validation: on the caller's HOST copies (device memory is never read back), before any launch; returns 1 with hh_last_error set for
 *   a null pointer (the shape and toggle tables may be null when empty), n outside 1..65535, a negative count, a misaligned device
 *   table (descs_dev 8 bytes, shapes_dev and toggles_dev 4), h or w outside 1..16384, a negative offset, a dst range that partially
 *   overlaps its src, a row range outside the table, more than HH_SEG_MAX_SHAPES rows in one frame (refused, never capped), an
 *   unknown kind or flag, a weight that is not finite or above 1e6 in magnitude, a colour above 0xFFFFFF, non-zero reserved ints, a fill
 *   whose toggle range
 *   leaves the table, whose toggles are not strictly increasing or exceed h*w, or whose column range is outside the frame or does not
 *   hold its covered columns, a line endpoint beyond +-2^23.
 * hh_seg_overlay_config: out[4] = tile rows, tile columns, threads per workgroup, shapes culled per chunk (a workgroup owns one tile
 *   and walks the frame's rows a chunk at a time, keeping the draw order within and across chunks).
 * hh_debug_seg_overlay_host: one frame through the same tile walk compiled for the host (src, dst: the frame's own HOST buffers, equal
 *   or disjoint; the descriptor's offsets are ignored); same validation.  For tests and tools/seg_overlay_host_check.cpp.
 * (Additive entry points: HH_ABI_VERSION stays 3.)                                                                           */
#define HH_SEG_SHAPE_INTS 8
#define HH_SEG_MAX_SHAPES 65535 /* per frame; refused, never capped */
enum { HH_SEG_FILL = 0, HH_SEG_LINE = 1 };
typedef hh_render_desc hh_seg_desc;
int hh_seg_overlay_u8_batch(unsigned char *batch_base, const hh_seg_desc *descs_dev, const hh_seg_desc *descs_host, const int32_t *shapes_dev,
                            const int32_t *shapes_host, int num_shapes, const unsigned int *toggles_dev, const unsigned int *toggles_host,
                            long long num_toggles, int n, void *stream);
int hh_seg_overlay_config(int out[4]);
int hh_debug_seg_overlay_host(const unsigned char *src, unsigned char *dst, const hh_seg_desc *desc, const int32_t *shapes, int num_shapes,
                              const unsigned int *toggles, long long num_toggles);
/* Heatmap panels: plot_heatmaps + make_grid of the reference (keypoints/visualization.py:93-110, utils/image.py:15-38) for every grid
 * of one figure in ONE call (one min/max launch, skipped when no map asks for it, and one paint launch), from the stage outputs of the
 * net as they are: no full-resolution fp32 map is stored or copied to the host.  tests/panels_ref.py restates the rule in numpy /
 * torch-CPU; the result is bit-identical to it.
 *
 * The per-pixel rule.  A figure is a uint8 canvas [Hc, Wc, 3] with `pitch` bytes between rows.  It is zero everywhere except in its
 * cells.  Cell m is H x W pixels at origin (oy_m, ox_m) and shows map m over the same uint8 image [H, W, 3].  The value v of map m at
 * (y, x) of its cell, by the map's kind (src_index / bilerp: torch CPU's F.interpolate(bilinear, align_corners=False) in fp32, the
 * decode's own, scale = (float)in / (float)out):
 *   HH_PANEL_DIRECT   src[y][x]; src is H x W.  No arithmetic.
 *   HH_PANEL_SINGLE   one interpolate from h x w: bilerp(src, w, src_index(h, (float)h / H, y), src_index(w, (float)w / W, x)).
 *   HH_PANEL_NESTED   src is the quarter-resolution map (H == 4h, W == 4w), resized x2 and then to H x W (match_heatmaps_size, then
 *                     resize_heatmaps: stage 0 of KeypointsResult): the four half-resolution taps (r, c) of the second resize are each
 *                     bilerp(src, w, src_index(h, 0.5f, r), src_index(w, 0.5f, c)) and are combined as hh_decode combines its taps.
 *   HH_PANEL_AVERAGE  the same with every tap averaged with the half-resolution map: (tap + src2[r][c]) / 2.0f, src2 [2h, 2w]: the
 *                     stage average as InferenceKeypointsResult.from_preds decodes it.
 * From v to the pixel, in fp32, every operation rounded on its own:
 *   1. HH_PANEL_CLIP: v = np.clip(v, 0, 1); NaN stays NaN.
 *   2. HH_PANEL_MINMAX: v = (v - mx) / (mx - mn), mx and mn the np.max / np.min of this map's values after step 1 over all H W pixels:
 *      a NaN anywhere makes both NaN.  The subtraction is v - mx, the reference's expression (visualization.py:104), so v lies in
 *      [-1, 0]; a constant map gives 0 / 0.
 *   3. q = v * 255.0f; t = q truncated toward zero as int32, 0 when q is not finite or outside int32; level = t & 255: what
 *      (hm * 255).astype(np.uint8) gives with numpy on x86-64 (-1.0 -> 255, -3.7 -> 253, NaN -> 0).
 *   4. c = 255 - level; colour = lut[c], lut a uint8 [256, 3] table of the caller's, applied channel for channel next to the image's
 *      channels with no B <-> R swap (the reference blends applyColorMap's B,G,R onto an R,G,B image as it is).
 *   5. out[ch] = rintf(image[y][x][ch] * 0.25f + colour[ch] * 0.75f), half to even, clamped to 0..255.
 * Pinned to torch: the resampling.  Pinned to numpy: the quantiser and the un-normalise below.  Pinned to this text: the blend and the
 * grid layout.  UNPINNED for want of cv2 where the fixtures are made: the default table (keypoints/visualization.py jet_lut: in B,G,R
 * order X2 = clamp(765 - |8 i - 510 k|, 0, 510) for k = 1 (B), 2 (G), 3 (R), entry (X2 + 1) >> 1, a reading of COLORMAP_JET) and the
 * fx / fy form of the resize.  The table is a parameter: a user with cv2 passes applyColorMap(arange(256), COLORMAP_JET).
 *
 * hh_heatmap_panels_u8: maps_dev / maps_host are the device copy the kernels read and the caller's HOST copy of the same n rows, which
 *   is what is checked.  src / src2 are device pointers to contiguous fp32 planes.  image, lut, canvas, scratch: device.  scratch:
 *   n * HH_PANEL_PARTS * 2 floats, may be null when no map has HH_PANEL_MINMAX; every element that is read is written earlier in the
 *   same call, so it needs no clearing and carries nothing from call to call.  The Wc * 3 bytes of every canvas row are all written
 *   (cells, padding, unused cells) exactly once; bytes between Wc * 3 and pitch are left alone; no alignment requirement on canvas, pitch
 *   or origins.  Of two cells that overlap the later row of the table wins.  Deterministic.  Returns 1 with hh_last_error set, before any
 *   launch, for a null pointer (image, lut, canvas, table, a map's src, an AVERAGE map's src2), n outside 1..HH_PANEL_MAX_MAPS, a kind or
 *   flag out of range, a side outside 1..16384, pitch < Wc * 3, a DIRECT map whose size is not H x W, a NESTED / AVERAGE map whose size
 *   is not H/4 x W/4, a cell that does not lie inside the canvas.
 * hh_debug_heatmap_panels_host: the same arithmetic (csrc/panel_math.h) compiled for the host on one figure in HOST memory (every
 *   pointer, those in the table too); same validation.  For tests and tools/panels_host_check.cpp.
 * hh_unnormalize_u8: KeypointsTransform.inverse_transform (base/transforms/base.py:33-41): out[y][x][c] = the cast of step 3 applied
 *   to ((double)x[c][y][x] * std[c] + mean[c]) * 255 in float64 (product, sum, product rounded separately), fp32 [3,H,W] -> uint8
 *   [H,W,3], both on the device.  The truncation can give one less than the raw byte; that is the reference's behaviour.
 * hh_resize_u8_scaled: cv2.resize(src, (0, 0), fx=fx, fy=fy): hh_resize_u8 with the coordinate scales 1 / fx and 1 / fy (not w / W);
 *   H x W must be cvRound(h * fy) x cvRound(w * fx), half to even, or the call is refused.  The 2 x 2 mean applies iff h == 2H and
 *   w == 2W, as in hh_resize_u8.  UNPINNED against cv2 like the rest of that resize.
 * (Additive entry points: HH_ABI_VERSION stays 3.)                                                                           */
#define HH_PANEL_MAX_MAPS 256 /* per figure */
#define HH_PANEL_PARTS 32     /* (max, min) pairs per map in the scratch */
enum { HH_PANEL_DIRECT = 0, HH_PANEL_SINGLE = 1, HH_PANEL_NESTED = 2, HH_PANEL_AVERAGE = 3 };
enum { HH_PANEL_CLIP = 1, HH_PANEL_MINMAX = 2 };
typedef struct hh_panel_map {
    const float *src;    /* DIRECT [H,W]; SINGLE [h,w]; NESTED, AVERAGE: the quarter-resolution map [h,w] */
    const float *src2;   /* AVERAGE: the half-resolution map [2h,2w]; otherwise ignored */
    int32_t h, w;        /* size of src */
    int32_t kind, flags;
    int32_t oy, ox;      /* the cell's origin in the canvas */
} hh_panel_map;
int hh_heatmap_panels_u8(const hh_panel_map *maps_dev, const hh_panel_map *maps_host, int n, const unsigned char *image, int H, int W,
                         const unsigned char *lut, unsigned char *canvas, int Hc, int Wc, long long pitch, float *scratch, void *stream);
int hh_debug_heatmap_panels_host(const hh_panel_map *maps, int n, const unsigned char *image, int H, int W, const unsigned char *lut,
                                 unsigned char *canvas, int Hc, int Wc, long long pitch);
int hh_unnormalize_u8(const float *x_chw, int H, int W, const double mean[3], const double stdv[3], unsigned char *out_hwc, void *stream);
int hh_resize_u8_scaled(const unsigned char *src, int h, int w, int channels, double fx, double fy, unsigned char *dst, int H, int W,
                        void *stream);
/* Baseline JPEG on the device: the files the reference's video and directory paths end in (cv2.VideoWriter "MJPG",
 * src/base/datasets/video.py:93-106; the .jpg plots of src/base/datasets/base.py:140 and src/base/callbacks.py:234,371), for n rendered
 * frames or figures of mixed sizes, qualities and subsamplings in ONE call of three launches.  The frames leave the GPU compressed.
 * tests/jpeg_ref.py restates the rule in numpy; device, host (hh_debug_jpeg_encode_host) and numpy agree byte for byte, because
 * everything below is integer arithmetic.  `>>` is a floor shift, `/` truncates.
 *
 * Input: a uint8 image [h,w,3], `pitch` bytes between rows, R,G,B or (flags bit 0) B,G,R: the flag swaps the channels on read, the
 *   stream always holds the true colours.  1 <= h, w <= 65535.
 * Output: one baseline sequential JFIF stream (SOF0, 8 bit, 3 components, Huffman).
 * 1. Padding to a multiple of the MCU (16 x 16 for subsampling 420, 8 x 8 for 444) by repeating the last row and column.
 * 2. Colour (libjpeg's 16-bit fixed point):  Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *                                            Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
 *                                            Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
 * 3. 4:2:0 chroma: (a + b + c + d + 2) >> 2 over each 2 x 2 group (this project's rule; libjpeg alternates its bias).
 * 4. FDCT on s = sample - 128 with T[u][x] = round(2^14 c(u) cos((2x + 1) u pi / 16)), c(0) = sqrt(1/8), c(u) = 1/2 otherwise (row 0
 *    is all 5793; the other magnitudes are 8035 6811 4551 1598 for odd u, 7568 3135 for u = 2, 6, and 5793 for u = 4):
 *    rows A[y][u] = (sum_x s[y][x] T[u][x] + 1024) >> 11, columns F[v][u] = sum_y A[y][u] T[v][y] = the coefficient times 2^17.
 *    Bound: |s| <= 128 and the largest row sum of |T| is 8 * 5793 = 46344 (46344, 41990, 42812, 41990, 46344, ... for u = 0, 1, 2, ...),
 *    so |A| <= (46344 * 128 + 1024) >> 11 = 2897 and |F| <= 2897 * 46344 = 134258568 < 2^27.1: both inside int32.  (Measured over the
 *    sign-pattern inputs that maximise each coefficient: |A| <= 2896.)
 * 5. Quantisation: q = sign(F) ((|F| + (Q << 16)) / (Q << 17)): to nearest, half away from zero.  Q = clamp((base scale + 50) / 100,
 *    1, 255) with base from the Annex K luminance table (component 1) or chrominance table (components 2, 3) and libjpeg's scale =
 *    5000 / quality below quality 50, 200 - 2 quality from there on; quality 1..100.  Then AC is clamped to +-1023 and DC to
 *    -1024..1023: a guard (the sign patterns reach |AC| = 1020 and DC = -1024 at Q = 1).
 * 6. Entropy coding: zigzag order, the four Annex K Huffman tables, DC as the difference to the previous block of the same component,
 *    ZRL for zero runs above 15, EOB unless coefficient 63 is non-zero.  The restart interval is one MCU row (DRI = MCUs per row):
 *    every interval starts with DC predictions 0, is padded with 1-bits to a byte and byte-stuffed (FF -> FF 00), and each but the last
 *    is followed by RSTm, m = row & 7.  Intervals are independent and byte aligned: that is what makes the stream parallel.
 * 7. Segments: SOI; APP0 (JFIF 1.01, units 0, density 1:1, no thumbnail); DQT table 0, DQT table 1 (zigzag order); SOF0 (component 1
 *    sampling 2x2 or 1x1 with Tq 0, components 2 and 3 1x1 with Tq 1); DHT DC0, DC1, AC0, AC1; DRI; SOS (component 1 tables 0/0,
 *    components 2 and 3 tables 1/1, Ss 0, Se 63, Ah/Al 0); the intervals; EOI.  The header is 629 bytes.
 * Stated deviations from libjpeg: the chroma bias of step 3, the FDCT's own rounding (step 4), the restart intervals.  Any baseline
 *   decoder reads the stream; byte parity with libjpeg or cv2.imwrite is not a goal.
 *
 * The size bound.  One block costs at most 22 + 63 * 26 = 1660 bits: a DC code of at most 11 bits with 11 value bits, and 63 non-zero
 *   AC coefficients of at most 16 code bits and 10 value bits each (a zero never costs more: a ZRL of at most 11 bits stands for 16 of
 *   them, the EOB of at most 4 bits needs one).  An interval of nblk blocks (6 per MCU in 420, 3 in 444) therefore has at most
 *   2 * ceil(1660 nblk / 8) bytes, every byte stuffed, and hh_jpeg_bound = 629 + rows * (2 * ceil(1660 nblk / 8) + 2), the 2 being the
 *   RSTm or EOI.  Every buffer is sized by it: the LDS bit buffer of the entropy kernel holds 64 blocks at 1660 bits, the workspace one
 *   slot of the interval's bound per interval, the output hh_jpeg_bound per frame.  Nothing is sized by typical content.
 *
 * hh_jpeg_bound / hh_jpeg_workspace_bytes: the bytes of output capacity and of workspace (a multiple of 16) one h x w frame needs;
 *   -1 with hh_last_error set for a size outside 1..65535 or a subsampling other than 420 or 444.
 * hh_jpeg_quant_tables: out[2][64] = the luminance and chrominance divisors at `quality`, in zigzag order.
 * hh_jpeg_config: out[4] = blocks per pass of the entropy kernel (one wave per interval, one lane per block), the per-block bound in
 *   bits, the header's bytes, MCUs per workgroup of the transform kernel (a wave each).
 * hh_jpeg_encode_u8_batch: one hh_jpeg_desc of 64 bytes per frame.  Source and stream lie at batch_base + src_offset and batch_base +
 *   out_offset (one base for both, never dereferenced itself), the frame's scratch at workspace + ws_offset (a multiple of 16;
 *   hh_jpeg_workspace_bytes of room; no clearing needed, nothing is carried from call to call).  lengths_dev[i] receives the stream's
 *   length, at most the bound.  Bytes beyond the length are not written.  Deterministic.  descs_dev is what the kernels read, descs_host
 *   the caller's HOST copy of the same rows, and that is what is checked (device memory is never read back).  Returns 1 with
 *   hh_last_error set, before any launch, for a null pointer, n outside 1..65535, a misaligned descs_dev (8), workspace (16) or
 *   lengths_dev (4), h or w outside 1..65535, "quality outside 1..100", "subsampling must be 420 or 444", "pitch below 3 * w", an unknown
 *   flag, "output capacity below hh_jpeg_bound", a bound beyond int32, a negative offset, a frame whose scratch does not lie inside
 *   workspace_bytes.  That frames and streams lie inside the caller's buffer cannot be checked here.
 * hh_debug_jpeg_encode_host: the same rule (csrc/jpeg_math.h) in plain C++ on one frame in HOST memory (src and out are the frame's
 *   own buffers; the descriptor's offsets are not applied); same validation.  For tests, tools/jpeg_host_check.cpp, and as the
 *   yardstick of the GPU tests.
 * hh_debug_jpeg_fdct: step 4 alone on one block of samples (absolute sum at most 8192 = 64 * 128, which keeps F inside int32): rows_out = A, cols_out = F,
 *   both [8][8] in natural order.
 * (Additive entry points: HH_ABI_VERSION stays 3.)                                                                           */
typedef struct hh_jpeg_desc {
    long long src_offset, out_offset, out_capacity, ws_offset, pitch;
    int32_t h, w;
    int32_t quality, subsampling;
    int32_t flags, reserved;
} hh_jpeg_desc;
long long hh_jpeg_bound(int h, int w, int subsampling);
long long hh_jpeg_workspace_bytes(int h, int w, int subsampling);
int hh_jpeg_quant_tables(int quality, int32_t out[128]);
int hh_jpeg_config(int out[4]);
int hh_jpeg_encode_u8_batch(unsigned char *batch_base, const hh_jpeg_desc *descs_dev, const hh_jpeg_desc *descs_host, int n,
                            unsigned char *workspace, long long workspace_bytes, int32_t *lengths_dev, void *stream);
int hh_debug_jpeg_encode_host(const unsigned char *src, const hh_jpeg_desc *desc, unsigned char *out, long long *length);
int hh_debug_jpeg_fdct(const int32_t samples[64], int32_t rows_out[64], int32_t cols_out[64]);
/* Baseline JPEG decoded on the device: the reference's `np.array(Image.open(path).convert("RGB"))` (src/base/datasets/base.py:174,194,
 * src/classification/datasets/imagenet.py:49) for n streams of mixed sizes, samplings and tables in ONE call of three launches.  Only
 * the compressed bytes and a small table cross the bus.  The target is the same bytes as Pillow (libjpeg-turbo), not a tolerance:
 * tests/golden/jpeg_decode.npz holds Pillow's pixels, tests/jpeg_decode_ref.py restates the rule in numpy; device, host
 * (hh_debug_jpeg_decode_host), numpy and Pillow agree byte for byte on that corpus.  Integer arithmetic only; `>>` is arithmetic.
 *
 * Accepted: SOF0, 8 bit; 1 component (grayscale, replicated to three channels) or 3 components Y/Cb/Cr; sampling 4:4:4, 4:2:2 (h2v1),
 *   4:2:0 (h2v2); one interleaved scan of all components; up to 4 DC and 4 AC Huffman tables (standard or optimised); 8- or 16-bit
 *   quantiser tables; any DRI or none; APPn and COM are skipped.
 * Refused by name by hh_jpeg_parse, on the host, before anything is staged or launched: "progressive streams (SOF2)", any other SOF,
 *   "arithmetic coding", "12-bit precision", "4 components", "unsupported sampling" (4:4:0, 4:1:1, ...), "more than one scan", "an Adobe
 *   marker with transform 0 (RGB)", "missing tables", "a dimension of 0", "dimensions beyond what int32 offsets allow", "truncated
 *   header", restart markers that do not match the interval or are out of sequence.
 * a. Entropy decoding (ITU T.81 F.2): FF 00 is FF; DC prediction per component, 0 at the start and after each RSTm; coefficients in
 *    natural order.
 * b. IDCT: libjpeg's jidctint ("islow") on coefficient x divisor (integer multiply): CONST_BITS 13, PASS1_BITS 2, columns first,
 *    descaled by 11 with rounding, rows descaled by 18 with rounding; the constants 2446 3196 4433 6270 7373 9633 12299 15137 16069
 *    16819 20995 25172; sample = clamp(result + 128, 0, 255).  (libjpeg's C code wraps results beyond +-512 through a 1024-entry
 *    table; the SIMD code Pillow runs saturates instead, and Pillow's output decides: see tests/jpeg_decode_ref.py.)
 * c. Chroma upsampling, libjpeg's "fancy" filters, with edges at the component's true size ceil(w / 2) x ceil(h / 2):
 *    h2v2: s[c] = 3 near[c] + far[c], far = the row above for the upper output row, below for the lower, the edge row itself at the first
 *      and last row; even outputs (3 s[c] + s[c-1] + 8) >> 4, odd outputs (3 s[c] + s[c+1] + 7) >> 4, the missing neighbour = s[c].
 *    h2v1: even outputs (3 c + left + 1) >> 2, odd (3 c + right + 2) >> 2; the first and last output equal the edge sample.
 *    A chroma width <= 2 (image width <= 4): plain replication in both axes.
 * d. Colour: R = Y + ((91881 cr + 32768) >> 16), B = Y + ((116130 cb + 32768) >> 16), G = Y + ((-22554 cb - 46802 cr + 32768) >> 16)
 *    with cb = Cb - 128, cr = Cr - 128, each clamped to 0..255.  Flag bit 0 stores B,G,R.
 *
 * hh_jpeg_parse: walks the markers of one stream in HOST memory and fills the info (all refusals happen here).
 * A segment is the run of MCUs one lane decodes.  hh_jpeg_restart_segments: with DRI, one segment per restart interval from a byte scan
 *   for RSTm, no Huffman work, predictors 0.  hh_jpeg_index_host: one Huffman pass on the host (symbol lengths and DC sums only) that
 *   records an entry every mcus_per_segment MCUs (<= 0: one MCU row, our encoder's interval; a parameter, not a measured optimum),
 *   counted anew at every restart; it validates the stream ("the scan cannot be walked: <status>").  Both refuse a capacity below the
 *   number of entries.  A file's index is built once and reused.
 * hh_jpeg_decode_workspace_bytes: int16 coefficients of the MCU grid plus the block-padded component planes (a multiple of 16).
 * hh_jpeg_decode_tables_bytes: info (112) + quantiser and Huffman lookup tables (7808) + 32 nseg.  hh_jpeg_decode_tables writes that
 *   block (HOST) for a stream and its entries.  Nothing is sized by typical content.
 * hh_jpeg_decode_u8_batch: one hh_jpeg_dec_desc of 64 bytes per image; stream, table block and destination lie at batch_base + their
 *   offsets (one base, never dereferenced itself), scratch at workspace + ws_offset.  descs_host / infos_host are the caller's HOST
 *   copies of the descriptors and of the infos the table blocks start with: they are what is checked.  status_dev[i] is cleared, then
 *   raised to the largest code a lane of image i met: 1 bad Huffman code, 2 zero run past coefficient 63, 3 bytes exhausted, 4 missing
 *   or unexpected RSTm, 5 bad segment; that lane ends there.  No input makes a kernel read or write outside the image's stream,
 *   workspace and destination: every byte read is bounded by the segment's and the scan's end, every block by the segment's own extent
 *   cut to the MCU grid.  Returns 1 with hh_last_error set, before any launch or clearing, for a null pointer, n outside 1..65535,
 *   misaligned descs_dev (8) / workspace (16) / status_dev (4) / table block (16), an info hh_jpeg_parse cannot have written, "negative
 *   offset", "pitch below 3 * w", an unknown flag, nseg < 1, a scan outside stream_length, "table block below
 *   hh_jpeg_decode_tables_bytes", "workspace below hh_jpeg_decode_workspace_bytes".  It is the window decode (below) of the window
 *   (0, 0, h, w), whose MCU rectangle is the MCU grid: the same kernels, with the whole stream and all nseg segments shipped.
 * hh_debug_jpeg_decode_host: the whole rule on one stream in HOST memory into dst (entries NULL: its own segments); *status receives the
 *   code, a nonzero one also returns 1.  For tests, tools/jpeg_decode_host_check.cpp, and as the yardstick of the GPU tests.
 * (Additive entry points: HH_ABI_VERSION stays 3.)                                                                           */
typedef struct hh_jpeg_stream_info {
    long long scan_offset, scan_end;
    int32_t h, w, ncomp;
    int32_t sampling;          /* 444, 422, 420; 400: grayscale */
    int32_t restart_interval;  /* MCUs; 0: none */
    int32_t hs, vs;            /* luminance blocks per MCU across and down */
    int32_t mcols, mrows;
    int32_t bpm;               /* blocks per MCU */
    int32_t qt[3], dc[3], ac[3];
    int32_t nseg_restart;
    int32_t adobe_transform;   /* -1: none */
    int32_t reserved[3];       /* 0 from hh_jpeg_parse; the device index (below) uses [0]: its status, [1]: 1 = entries to be filled */
} hh_jpeg_stream_info;
typedef struct hh_jpeg_segment {
    int32_t first_mcu, mcu_count;
    int32_t byte_offset, bit_offset;
    int32_t pred[3];
    int32_t byte_end;          /* (end of the segment's bytes) << 1 | (an RSTm follows) */
} hh_jpeg_segment;
typedef struct hh_jpeg_dec_desc {
    long long stream_offset, tables_offset, tables_bytes, dst_offset, ws_offset, pitch;
    int32_t stream_length, nseg;
    int32_t flags, reserved;
} hh_jpeg_dec_desc;
int hh_jpeg_parse(const unsigned char *bytes, long long len, hh_jpeg_stream_info *info);
int hh_jpeg_restart_segments(const unsigned char *bytes, long long len, hh_jpeg_segment *entries, int capacity, int *n);
int hh_jpeg_index_host(const unsigned char *bytes, long long len, int mcus_per_segment, hh_jpeg_segment *entries, int capacity, int *n);
long long hh_jpeg_decode_workspace_bytes(const hh_jpeg_stream_info *info);
long long hh_jpeg_decode_tables_bytes(const hh_jpeg_stream_info *info, int nseg);
int hh_jpeg_decode_tables(const unsigned char *bytes, long long len, const hh_jpeg_segment *entries, int nseg, unsigned char *out,
                          long long out_bytes);
int hh_jpeg_decode_u8_batch(unsigned char *batch_base, const hh_jpeg_dec_desc *descs_dev, const hh_jpeg_dec_desc *descs_host,
                            const hh_jpeg_stream_info *infos_host, int n, unsigned char *workspace, long long workspace_bytes,
                            int32_t *status_dev, void *stream);
int hh_debug_jpeg_decode_host(const unsigned char *bytes, long long len, const hh_jpeg_segment *entries, int nseg, int flags,
                              unsigned char *dst, long long pitch, int *status);
/* Window decode: only a rectangle of the image is turned into pixels (the classifier's crop; classification/input.py).
 *
 * The rule.  For a window (top, left, height, width) inside the image the destination receives height x width x 3 bytes that equal,
 *   byte for byte, rows top .. top+height-1 and columns left .. left+width-1 of what hh_jpeg_decode_u8_batch writes for the whole
 *   image (so they also equal Pillow's pixels).  Steps a-d above hold as they stand: the fancy-upsampling edge rules stay tied to the
 *   component's true size and to the image's edges, never to the window's, and "chroma width <= 2: replicate" is decided by the
 *   image's width, never by the window's.
 * The MCU rectangle.  An output pixel of a subsampled axis reads its chroma sample and one neighbour on each side (rule c).  Luma rows
 *   t .. b need chroma rows max(0, (t >> 1) - 1) .. min(ch - 1, (b >> 1) + 1) when vs == 2 and rows t .. b when vs == 1; the same
 *   across with hs (h2v1 needs the +-1 column as well).  The rectangle is the MCUs that hold the window's luma samples and those
 *   chroma samples (grayscale: the luma samples).
 * Work done (derived, not measured).  Only segments with at least one MCU in the rectangle are selected (with a finer index not a
 *   contiguous set).  A lane walks its segment from the segment's first MCU, stores coefficients only for MCUs inside the rectangle and
 *   ends after the segment's last MCU inside it.  Coefficients and component planes are laid out for the rectangle
 *   (hh_jpeg_decode_window_workspace_bytes); the IDCT launch covers the rectangle's blocks, the colour launch the window's pixels; the
 *   grids are sized by the batch's largest.  Three launches per call, whatever the batch.
 * Staged bytes.  The slice [slice[0], slice[1]) of the file runs from the first selected segment's byte_offset to the last selected
 *   segment's end; nothing else of the stream is needed.  hh_jpeg_decode_window_select reports the count of selected segments and
 *   the slice; hh_jpeg_decode_window_tables (HOST) also writes the table block (hh_jpeg_decode_tables_bytes(info, *nsel)) that holds
 *   only the selected segments, their byte offsets and the info's scan_offset / scan_end rebased to the slice (scan_offset 0).  The
 *   descriptor's stream_offset / stream_length are the slice's.  The device bit reader knows no second origin; its bound is as
 *   before: every byte read lies inside the slice, cut to the segment's end.
 * Status.  status_dev[i] reports what the WALKED part of the scan met (codes as above).  "Data where the RSTm should stand" is checked
 *   only by a lane that walked its segment to the end.  Damage outside the walked part is not seen: the host index pass (or the
 *   restart scan) has validated the stream once per file, and that stays the gate.
 * Safety.  No input makes a kernel read or write outside the image's shipped slice, its window workspace and its height x pitch
 *   destination.  hh_jpeg_decode_window_u8_batch (one hh_jpeg_win_desc of 80 bytes per image: the fields of hh_jpeg_dec_desc, then
 *   the window; infos_host: the rebased infos of the table blocks) returns 1 with hh_last_error set, before any launch or clearing,
 *   for everything hh_jpeg_decode_u8_batch refuses and for "the window is empty", "the window leaves the image", "pitch below
 *   3 * width", "workspace below hh_jpeg_decode_window_workspace_bytes", "table block below hh_jpeg_decode_tables_bytes", "no selected
 *   segment"; select / tables refuse "no segment holds an MCU of the window's rectangle".
 * hh_debug_jpeg_decode_window_host: the same shared code (csrc/jpeg_dec_math.h) on one stream in HOST memory, through the same
 *   select / tables / slice steps (the slice is copied out, so nothing outside it can be read); *counts (may be NULL) receives what
 *   was done.  A window equal to the whole image gives the bytes of hh_jpeg_decode_u8_batch, which is the decode of that window.
 * (Additive entry points: HH_ABI_VERSION stays 3.)                                                                           */
typedef struct hh_jpeg_window {
    int32_t top, left, height, width;
} hh_jpeg_window;
typedef struct hh_jpeg_win_desc {
    hh_jpeg_dec_desc d;            /* stream_offset / stream_length: the shipped slice; nseg: the selected segments */
    hh_jpeg_window window;
} hh_jpeg_win_desc;                /* (the same 80 bytes as before, when the fields of `d` were written out here a second time) */
typedef struct hh_jpeg_window_counts {
    long long segments_walked, mcus_walked, mcus_stored, blocks_transformed, pixels_written, stream_bytes;
} hh_jpeg_window_counts;
long long hh_jpeg_decode_window_workspace_bytes(const hh_jpeg_stream_info *info, const hh_jpeg_window *window);
int hh_jpeg_decode_window_select(const hh_jpeg_stream_info *info, const hh_jpeg_segment *entries, int nseg, const hh_jpeg_window *window,
                                 int *nsel, long long slice[2]);
int hh_jpeg_decode_window_tables(const unsigned char *bytes, long long len, const hh_jpeg_segment *entries, int nseg,
                                 const hh_jpeg_window *window, unsigned char *out, long long out_bytes, int *nsel, long long slice[2]);
int hh_jpeg_decode_window_u8_batch(unsigned char *batch_base, const hh_jpeg_win_desc *descs_dev, const hh_jpeg_win_desc *descs_host,
                                   const hh_jpeg_stream_info *infos_host, int n, unsigned char *workspace, long long workspace_bytes,
                                   int32_t *status_dev, void *stream);
int hh_debug_jpeg_decode_window_host(const unsigned char *bytes, long long len, const hh_jpeg_segment *entries, int nseg,
                                     const hh_jpeg_window *window, int flags, unsigned char *dst, long long pitch, int *status,
                                     hh_jpeg_window_counts *counts);
/* The index of a restart-less stream built on the device: no Huffman work on the host before the bytes cross the bus, and segments as
 * fine as one likes (the entropy launch of the decode is bound by the length of one lane's walk).  Huffman codes self-synchronise: a
 * decoder started at an arbitrary bit soon falls into step with the true symbol sequence (Weissenberger & Schmidt, "Accelerating JPEG
 * decompression on GPUs", 2021).
 *
 * The rule.
 * Which streams.  For a stream without DRI that hh_jpeg_parse accepts, hh_jpeg_index_device_batch writes into the image's table block
 *   the same hh_jpeg_segment entries that hh_jpeg_index_host(bytes, len, mcus_per_segment, ...) writes, bit for bit: first_mcu,
 *   mcu_count, byte_offset, bit_offset, pred[3], byte_end.  Parity is defined against that function and nothing else.  The count is
 *   ceil(mcols mrows / mcus_per_segment), known from the header alone.
 * Algorithm (all arithmetic in csrc/jpeg_dec_math.h, shared by host and device: JpegBits, jpeg_dec_symbol, jpeg_dec_block<false>,
 *   jpeg_bits_where, jpeg_idx_walk).  The scan's bytes [scan_offset, min(scan_end, stream_length)) are cut into subsequences of
 *   subseq_bytes; one lane takes one subsequence.  Lane 0 starts at the true state: scan_offset, bit 0, block 0 of the MCU.  Every other
 *   lane starts at the first data bit of its subsequence (a 00 that follows an FF is skipped) and assumes a block boundary with
 *   block-in-MCU index 0.  A lane's state at a block boundary is the canonical bit position plus the block's index in the MCU; the
 *   canonical position is byte_offset / bit_offset exactly as hh_jpeg_index_host forms them (an FF 00 pair is one byte, the offset
 *   points at the FF).  DC predictors are not part of the state: only the differences are summed, with uint32 wrap.  Each lane decodes
 *   whole blocks up to its first boundary at or past the start of the next subsequence and records that exit state, its block count
 *   and its DC sums per component.  Then the lanes synchronise until nothing changes: a lane whose start state differs from its
 *   predecessor's exit state takes that state and decodes again.  Lane 0 is true, so after k passes lanes 0..k are true, and the loop
 *   ends after at most as many passes as there are lanes.  Exclusive scans over block counts and DC sums follow; in a last walk from
 *   the verified start states each lane writes the entries whose MCU boundary it crosses, pred = prefix + running sum.
 * Several rounds.  One workgroup owns one image.  A stream with more subsequences than the workgroup has lanes is processed in rounds
 *   of that many; the verified end state, block count and DC sums of one round are the true start of the next.
 * Status.  Speculative lanes report nothing.  Only the last walk, which is on the true chain, reports: status_dev[i] is cleared first,
 *   then set to the code hh_jpeg_index_host meets on the same stream: 0, or 1 bad Huffman code, 2 zero run past coefficient 63, 3 bytes
 *   exhausted.  A nonzero code is also written to reserved[0] of the info at the head of the image's table block on the DEVICE, and the
 *   entropy launch of hh_jpeg_decode_u8_batch skips an image whose table block carries one (its pixels are then unspecified, inside
 *   its own destination; its decode status stays 0, so the larger of the two calls' codes is the index's).
 * Invariants, held by construction.  Every loop is bounded by the subsequence count (the passes of a round: the round's lanes; the
 *   rounds: ceil(subsequences / lanes)), the block count mcols mrows bpm (a lane's walk ends after that many blocks at the latest), or
 *   the scan's length (the bit reader).  No workgroup ever waits for another: no spins, no grid-wide barriers, no cooperative launch;
 *   the only waits are the barriers of one workgroup, reached by all of its lanes.  Every byte read lies inside the image's stream
 *   ([scan_offset, min(scan_end, stream_length))).  Every write lies inside the image's table block (entries below nseg, the info's
 *   reserved[0]) or its status word.
 * Streams with DRI keep hh_jpeg_restart_segments (a byte scan with no Huffman work already); cutting restart intervals finer on the
 *   device is out of scope.  The index launch skips such images, and every image whose table block was not written by
 *   hh_jpeg_index_tables (reserved[1] of its info is not 1): host-indexed, DRI and device-indexed images mix freely in one batch.
 *
 * hh_jpeg_index_config: out[4] = lanes per workgroup (1024), the default subseq_bytes (32: the fastest of 16..512 in profiles/jpeg_index.md), the minimum subseq_bytes (4), the default
 *   mcus_per_segment (2: the finest size measured, profiles/jpeg_index.md; a parameter, not an optimum).
 * hh_jpeg_index_workspace_bytes: the global scratch of one image.  Derived, not measured: a round's states (one exit state per lane)
 *   live in LDS and what a round hands to the next is one state, one block count and three sums, so the answer is 0 for every stream
 *   and `workspace` may be NULL; -1 with hh_last_error set for an info hh_jpeg_parse cannot have written or a refused subseq_bytes.
 * hh_jpeg_index_tables (HOST): the table block of hh_jpeg_decode_tables for a stream without DRI, with every entry's first_mcu /
 *   mcu_count filled and its offsets and predictors zero, and reserved[1] of the info set to 1 (the device is to fill the entries).
 *   *nseg receives the count.  The whole block crosses the bus with the stream (32 nseg bytes of it are the blank entries).
 * hh_jpeg_index_device_batch: one launch on `stream`, in front of hh_jpeg_decode_u8_batch on the same stream with the same
 *   hh_jpeg_dec_desc rows.  Returns 1 with hh_last_error set, before any launch or clearing, for everything the decode refuses, for
 *   subseq_bytes below the minimum or not a multiple of 4, mcus_per_segment < 1, workspace_bytes < 0, and for an image to be indexed
 *   whose nseg is not the count of mcus_per_segment.
 * hh_debug_jpeg_index_sync_host: the same shared code on one stream in HOST memory with `lanes` subsequences per round; *n entries
 *   (0 with a nonzero *status, which also returns 1); counts (may be NULL) receives six numbers: rounds, passes that changed a lane in
 *   all, the same in the worst round, subsequences, blocks decoded in all, blocks decoded by the last walk (the true chain).  For tests and
 *   tools/jpeg_index_host_check.cpp, and as the yardstick of the GPU tests.
 * (Additive entry points: HH_ABI_VERSION stays 3.)                                                                           */
int hh_jpeg_index_config(int out[4]);
long long hh_jpeg_index_workspace_bytes(const hh_jpeg_stream_info *info, int subseq_bytes);
int hh_jpeg_index_tables(const unsigned char *bytes, long long len, int mcus_per_segment, unsigned char *out, long long out_bytes, int *nseg);
int hh_jpeg_index_device_batch(unsigned char *batch_base, const hh_jpeg_dec_desc *descs_dev, const hh_jpeg_dec_desc *descs_host,
                               const hh_jpeg_stream_info *infos_host, int n, int mcus_per_segment, int subseq_bytes, unsigned char *workspace,
                               long long workspace_bytes, int32_t *status_dev, void *stream);
int hh_debug_jpeg_index_sync_host(const unsigned char *bytes, long long len, int mcus_per_segment, int subseq_bytes, int lanes,
                                  hh_jpeg_segment *entries, int capacity, int *n, int *status, long long counts[6]);
/* COCO keypoint scoring on the device: computeOks + evaluateImg of pycocotools' COCOeval(iouType="keypoints") as keypoints/coco_eval.py
 * restates them (`_oks`, `_evaluate_img`; the `eval_coco` step of keypoints/bin/eval.py:52-65), for every image, area range and threshold
 * in ONE launch over packed tables.  What is pinned is "device = this repository's host evaluator"; parity with pycocotools itself stays
 * UNPINNED (the package is absent where the fixtures are made).  The arithmetic is csrc/coco_eval_math.h, shared with the host.
 *
 * The tables (keypoints.coco_eval.pack_tables builds them): I images; the detections of image i are rows dt_off[i] .. dt_off[i+1]-1 of
 * the N detection rows, in the evaluator's order (stable by descending score, cut to maxDets = 20 by the packer; the kernels accept up
 * to HH_COCO_MAX_DET); its ground truths rows gt_off[i] .. gt_off[i+1]-1 of the M ground-truth rows, in annotation order.  oks_off[i] is
 * the sum of D_j * G_j over j < i.  All floating-point tables are fp64.  gt_flags: HH_COCO_GT_IGNORE (_prepare: iscrowd or
 * num_keypoints == 0) | HH_COCO_GT_CROWD.  vars[k] = (2 sigma_k)^2, formed by the caller: the sigmas are a parameter.
 *
 * OKS of one pair, fp64, every operation rounded on its own: k1 = #{k : v_k > 0}; if k1 > 0, dx = xd - xg, dy = yd - yg, else the
 * distance to the doubled box dx = max(0, x0 - xd) + max(0, xd - x1), x0 = bx - bw, x1 = bx + 2 bw (the same in y);
 * e_k = (dx dx + dy dy) / vars[k] / (area + 2^-52) / 2; OKS = sum of exp(-e_k) over the labelled joints (all K when k1 = 0), ascending
 * k, divided by their number.  e_k is bit-identical to numpy's; exp and the order of the sum may differ from the host evaluator.
 * Matching of one (image, area range a, threshold t), no floating-point arithmetic: a ground truth is ignored iff its flag is set or its
 * area is outside [lo_a, hi_a]; they are walked not-ignored first, each half in table order; per detection, in table order, the running
 * best starts at min(t, 1 - 1e-10), a ground truth already matched is skipped unless it is a crowd, the walk stops when the best so far
 * is not ignored and the ignored ones begin, an OKS below the running best is skipped (an equal one on a later ground truth wins).
 *
 * Outputs (device): dt_match int32 [A,T,N] = the matched ground truth's row in the table + 1, 0 for none; dt_ignore uint8 [A,T,N] = the
 * matched ground truth's ignore flag, or "the detection's area is outside the range" when unmatched; gt_ignore uint8 [A,M] in table
 * order.  Every element is written exactly once (no clearing first), nothing else is; nothing is carried between calls; deterministic.
 * hh_coco_evaluate: the fused launch; the OKS values stay in LDS.  hh_coco_oks: only the OKS matrices, image i's D_i x G_i row-major at
 *   oks[oks_off[i]], oks_off[I] doubles in all.  hh_coco_match: only the matching, on such a buffer of the caller's.
 * hh_coco_evaluate_host: the same code compiled for the host over tables in HOST memory: with oks_in the matching alone on that buffer,
 *   otherwise OKS (stored to oks_out if it is not null) and matching; the three outputs may all be null to get the OKS only.
 * tables_dev / tables_host are two structs in HOST memory: the one holds the device addresses the kernel reads, the other the caller's
 *   host copy of the same tables, which is what is checked (device memory is never read back).  Returns 1 with hh_last_error set, before
 *   any launch, for a null pointer, a misaligned table, offsets that do not start at 0, decrease, or leave N / M, an image with more than
 *   HH_COCO_MAX_DET detections or HH_COCO_MAX_GT ground truths (the message names the image), K, T or A over its limit, a non-finite
 *   area, a var that is not finite and > 0, a NaN range or threshold.  (Additive entry points: HH_ABI_VERSION stays 3.)            */
#define HH_COCO_MAX_DET 32 /* per image (the evaluator uses 20) */
#define HH_COCO_MAX_GT 128 /* per image */
#define HH_COCO_MAX_K 64
#define HH_COCO_MAX_T 16
#define HH_COCO_MAX_A 4
enum { HH_COCO_GT_IGNORE = 1, HH_COCO_GT_CROWD = 2 };
typedef struct hh_coco_tables {
    const int32_t *dt_off;          /* [I+1] */
    const int32_t *gt_off;          /* [I+1] */
    const int64_t *oks_off;         /* [I+1] */
    const double *dt_xy;            /* [N,K,2] */
    const double *dt_score;         /* [N] (not read by the kernels) */
    const double *dt_area;          /* [N] */
    const double *gt_xyv;           /* [M,K,3] */
    const double *gt_area;          /* [M] */
    const double *gt_bbox;          /* [M,4] x, y, w, h */
    const unsigned char *gt_flags;  /* [M] */
    const double *vars;             /* [K] */
    const double *area_rng;         /* [A,2] */
    const double *thr;              /* [T] */
    int32_t I, N, M, K, A, T;
    int32_t reserved[2];
} hh_coco_tables;
int hh_coco_oks(const hh_coco_tables *tables_dev, const hh_coco_tables *tables_host, double *oks, void *stream);
int hh_coco_match(const hh_coco_tables *tables_dev, const hh_coco_tables *tables_host, const double *oks, int32_t *dt_match,
                  unsigned char *dt_ignore, unsigned char *gt_ignore, void *stream);
int hh_coco_evaluate(const hh_coco_tables *tables_dev, const hh_coco_tables *tables_host, int32_t *dt_match, unsigned char *dt_ignore,
                     unsigned char *gt_ignore, void *stream);
int hh_coco_evaluate_host(const hh_coco_tables *tables_host, const double *oks_in, double *oks_out, int32_t *dt_match,
                          unsigned char *dt_ignore, unsigned char *gt_ignore);
/* Pose tracking across video frames behind hh_decode (csrc/track.hip, csrc/track_math.h; keypoints/tracking.py PoseTracker): person ids
 * that persist from frame to frame and One-Euro smoothed coordinates, one launch for a whole chunk of frames, on hh_decode's device
 * outputs before they are copied anywhere.  An extension: the reference has no tracker (its video_processing_fn sorts people by mean
 * tag and colours by limb).  (Additive entry points: HH_ABI_VERSION stays 3.)
 *
 * STREAMS AND FRAMES.  A call handles S independent streams of F consecutive frames each, stream-major: frame f of stream s is row
 *   b = s * F + f of the decode's batch, B = S * F.  One workgroup per stream walks its frames in order; streams share nothing.
 * STATE.  `state`: S * hh_track_state_bytes(K, max_tracks) bytes of device memory, 8-byte aligned, owned by the caller, opaque; stream s
 *   owns the s-th block.  All zero = empty (hh_track_reset: one memset of nstreams consecutive blocks).  Per stream: the number of ids
 *   issued (next_id - 1) and a frame counter; per slot: id (0 = free), hits, misses, the last matched raw pose xy[K] and score[K] as
 *   floats, its box area, and xhat / dxhat of the filter per coordinate as doubles.  The kernel keeps the block in LDS during the frame
 *   loop when it fits there next to the max_tracks x max_people similarity matrix and the frame's staged rows, in global memory otherwise (or when params.reserved
 *   bit 0 is set: a test switch); the results are the same bits.
 * INPUTS: hh_decode's outputs joints [B,max_people,K,3+E], scores [B,max_people], num_people [B], flags [B] (may be NULL = all 0).
 *   Coordinates are model-input pixels.
 * RULE for one frame of one stream, fp64 with every operation rounded on its own (compiled with -ffp-contract=off), joint scores and
 *   thresholds compared as floats:
 *   1. Row d < min(num_people, max_people) is VALID if scores[d] >= min_person_score, at least min_joints of its joints have
 *      score > joint_thr, and neither HH_DECODE_FALLBACK nor HH_DECODE_SOLVER_GUARD is set in the frame's flags.  Every other row gets
 *      id 0.  A frame with HH_DECODE_SOLVER_GUARD has no detections at all, and out_flags carries HH_TRACK_SOLVER_GUARD.
 *   2. For each live track t (id != 0) and valid row d, over the joints k labelled in both (score > joint_thr in the track's last
 *      matched pose and in the row), k ascending:
 *        dx = (double)x_d - (double)x_t, dy likewise;  e_k = ((dx*dx + dy*dy) / vars[k]) / (area_t + 2^-52) / 2
 *        S[t][d] = (sum of exp(-e_k)) / n_common if n_common >= min_common and n_common > 0, else 0
 *      vars[k] = (2 sigma_k)^2 is the caller's.  area_t = (max x - min x) * (max y - min y) over the labelled joints of the row the
 *      track last matched, in doubles, and 1 if that is below 1.  The track's pose is the last MATCHED RAW pose, neither filtered nor
 *      predicted: matching does not depend on the smoothing.  All other entries of S are 0.
 *   3. Greedy assignment, comparisons only: among the pairs with S >= min_oks whose track and row are both still free, take the one
 *      with the largest S, then the lowest track id, then the lowest d; repeat until none is left.
 *   4. A matched track: Te = (misses + 1) / fps, hits += 1, misses = 0, area from the row; per joint labelled in the row xy and score
 *      are replaced, a joint unlabelled in the row keeps its xy with score 0.  An unmatched track: misses += 1, and it is freed when
 *      misses > max_age.  Then the valid rows nobody matched, d ascending, open tracks in the free slots, lowest first (a slot freed in
 *      this frame counts), with id = ++issued, hits 1, misses 0; ids start at 1 and are never reused within a stream.  Rows left over
 *      keep id 0 and out_flags carries HH_TRACK_POOL_FULL.
 *   5. One-Euro filter per coordinate x of every labelled joint of a matched row, pi = 3.141592653589793:
 *        alpha(c) = 1.0 / (1.0 + (1.0 / ((2.0 * pi) * c)) / Te)
 *        dx = (x - xhat) / Te;  dxhat = alpha(d_cutoff) * dx + (1.0 - alpha(d_cutoff)) * dxhat
 *        c = min_cutoff + beta * fabs(dxhat);  xhat = alpha(c) * x + (1.0 - alpha(c)) * xhat
 *      A joint labelled now that was not labelled at the track's previous match, and every joint of a track opened in this frame,
 *      starts afresh: xhat = x, dxhat = 0.
 * OUTPUTS (device): track_ids int32 [B,max_people] (0 = no track); smooth float [B,max_people,K,2] = xhat rounded once to fp32 for the
 *   labelled joints of tracked rows, the row's raw x, y everywhere else; out_flags int32 [B].  Every element is written exactly once
 *   per call; nothing but the state carries over between calls.  Deterministic.
 * hh_track_step: the fused launch.  hh_track_step_host: the same code compiled for the host over HOST memory (state included).
 * hh_track_similarity: only the S matrices, sim double [S,max_tracks,max_people], of ONE frame per stream (B = S) against the current
 *   state, which is not changed.  hh_track_assign: only step 3 on n caller's matrices sim [n,T,P] (device) with ids int32 [n,T]
 *   (0 = the row is no live track; the live ids of a matrix must be distinct) -> match int32 [n,T] = the row's d or -1;
 *   hh_track_assign_host: the same over host memory.
 * Each returns 1 with hh_last_error set, before any launch, for a null pointer (flags excepted), a state or sim pointer that is not
 *   8-byte aligned, any other pointer that is not 4-byte aligned, K, max_tracks or max_people outside 1..64, E outside 0..64, negative
 *   S, F, n, a vars entry that is not finite and > 0, a non-finite or non-positive fps, min_cutoff or d_cutoff, a negative or
 *   non-finite beta, a negative max_age, min_joints or min_common, a min_oks outside (0, 1], a negative or non-finite joint_thr, a NaN
 *   min_person_score.  */
#define HH_TRACK_MAX_TRACKS 64
#define HH_TRACK_MAX_K 64
#define HH_TRACK_MAX_PEOPLE 64
#define HH_TRACK_SOLVER_GUARD 2
#define HH_TRACK_POOL_FULL 4
typedef struct hh_track_params {
    double vars[HH_TRACK_MAX_K];  /* the first K are read */
    double fps, min_cutoff, beta, d_cutoff, min_oks;
    float joint_thr, min_person_score;
    int32_t K, E, max_people, max_tracks, max_age, min_joints, min_common;
    int32_t reserved;             /* 0 (bit 0: keep the state in global memory) */
} hh_track_params;
int64_t hh_track_state_bytes(int K, int max_tracks);
int hh_track_reset(void *state, int K, int max_tracks, int nstreams, void *stream);
int hh_track_step(const hh_track_params *params, void *state, const float *joints, const float *scores, const int32_t *num_people,
                  const int32_t *flags, int S, int F, int32_t *track_ids, float *smooth, int32_t *out_flags, void *stream);
int hh_track_step_host(const hh_track_params *params, void *state, const float *joints, const float *scores, const int32_t *num_people,
                       const int32_t *flags, int S, int F, int32_t *track_ids, float *smooth, int32_t *out_flags);
int hh_track_similarity(const hh_track_params *params, void *state, const float *joints, const float *scores, const int32_t *num_people,
                        const int32_t *flags, int S, double *sim, void *stream);
int hh_track_assign(const double *sim, const int32_t *ids, int n, int T, int P, double min_oks, int32_t *match, void *stream);
int hh_track_assign_host(const double *sim, const int32_t *ids, int n, int T, int P, double min_oks, int32_t *match);

/* Per-image OKS and PCKh against annotations, scored behind hh_decode (csrc/pose_score.hip, csrc/pose_score_math.h;
 * keypoints/pose_score.py): the reference's match_preds_to_targets (keypoints/results.py:21-43), object_OKS / image_OKS
 * (keypoints/datasets/coco.py:489-535, what InferenceKeypointsResult.calculate_OKS prints) and object_PCKh / image_PCKh
 * (keypoints/datasets/mpii.py) for every image of a batch in ONE launch, one workgroup per image, on hh_decode's device outputs
 * before they are copied anywhere.  This text is the specification.  All arithmetic is fp64, every operation rounds on its own
 * (compiled with -ffp-contract=off), every sum runs in the stated order.  (Additive entry points: HH_ABI_VERSION stays 3.)
 *
 * TABLES of image i < B.
 *   Predictions, `form`:
 *   HH_POSE_PRED_DECODE: hh_decode's outputs in place.  P_i = min(num[i], max_people), and num[i] < 0 counts as 0.  Joint k of person p
 *     is the two floats x, y at joints[i * image_stride + p * person_stride + k * joint_stride] (strides in floats); the person score is
 *     scores[i * score_stride + p]; flags may be NULL (= all 0).  inv_affine [B,6] fp64 is the image's inverse resize matrix M, formed
 *     by the host exactly as hh_transform_coords forms it (hh_get_affine_transform(..., inverse = 1, M)).  Un-warp, left to right:
 *       x' = M0*x + M1*y + M2*1.0,  y' = M3*x + M4*y + M5*1.0     with x, y widened to fp64 first.
 *     x', y' are rounded to float32 and widened again unless HH_DECODE_FALLBACK is set in flags[i]: transform_coords(...).astype(dtype)
 *     gives float32 normally and float64 for the fallback pseudo-person.  In the fallback case the person score is the fp64 mean of K
 *     values 0.01 (ascending sum divided by K), as MPPEHeatmapParser.to_lists forms it.
 *   HH_POSE_PRED_F64: P_i = p_off[i+1] - p_off[i]; p_xy fp64 [P,K,2] and p_score fp64 [P], contiguous, used as they are (results that
 *     already sit on the host; validation results, whose coordinates are model-input pixels).
 *   Targets: rows t_off[i] .. t_off[i+1]-1 of t_xyv fp64 [T,K,3] (x, y, v), t_area fp64 [T] (the packer's polygon area + 2^-52) and
 *     t_head fp64 [T] (the PCKh head size, 0 when unused).
 *   Per call: vars[K] = (2 sigma_k)^2, formed by the caller; alpha = the PCKh threshold; metric = HH_POSE_METRIC_OKS or _PCKH.
 *
 * RULE for one image with P predictions and T targets; d2(p,t,k) = dx*dx + dy*dy with dx = px - tx, dy = py - ty.
 *   0. status = HH_POSE_NONFINITE if an un-warped coordinate (DECODE) or p_xy value (F64) of a person p < P, or a person score, is not
 *      finite; | HH_POSE_NO_PRED if P = 0 and T > 0.  With status != 0: value = NaN, and obj = NaN, kpt = NaN, match = -1 for every
 *      target of the image; never a silent score.  Otherwise:
 *   1. Walk order of the predictions: ascending person score, stable (equal scores by ascending index): argsort(kind="mergesort").
 *   2. Matching.  n_t = #{k : v_tk > 0}.  D[p,t] = (sum over k with v_tk > 0, ascending k, of d2(p,t,k)) / n_t;  val = 1.0 / D (D = 0
 *      gives +inf).  Target t takes the first prediction in walk order whose val is strictly greater than every earlier one, starting
 *      from -inf.  Several targets may take the same prediction.  match[t] = that prediction's index in decode order.
 *   3. HH_POSE_METRIC_OKS, target t with p = match[t]:  e_k = d2(p,t,k) / ((2.0 * vars[k]) * area_t);  kpt[t,k] = exp(-e_k) for
 *      v_tk > 0, else -1;  obj[t] = oks_t = (sum of exp(-e_k) over the k with v_tk > 0, ascending) / n_t.
 *   4. HH_POSE_METRIC_PCKH: if head_t == 0, obj[t] = -1 and kpt[t,k] = -1 for all k.  Otherwise
 *      d_k = sqrt((px/h - tx/h)*(px/h - tx/h) + (py/h - ty/h)*(py/h - ty/h)),  hit_k = d_k < alpha;  kpt[t,k] = hit_k (1.0 or 0.0) for
 *      v_tk > 0, else -1;  obj[t] = pckh_t = (number of hits over the k with v_tk > 0) / n_t.
 *   5. Image value.  OKS: r_t = rint(oks_t * 1000.0) / 1000.0 (numpy's round(3); rint = to nearest, ties to even); value = (sum of r_t,
 *      ascending t) / T.  PCKh: value = (sum of the pckh_t that are not -1, ascending t) / their number.  value = -1 when no target counts.
 * Two stated differences from the reference: the sums run in ascending order where numpy sums pairwise from 8 elements up; the
 * matched order is returned (match) instead of reordering the predictions in place.  exp is each side's library function.
 *
 * hh_polygon_area: the reference's cv2.contourArea(np.array(poly).reshape(-1, 2).astype(np.int32)) restated as an exact int64
 *   shoelace: with (x_j, y_j) = the n points of xy [n,2] truncated toward zero, |sum over j of x_prev*y_j - y_prev*x_j| * 0.5, prev = j-1
 *   cyclically; 0 for n < 3 (cv2 returns 0 for an empty contour; a 1- or 2-point contour has no area).  Host code: packing happens on
 *   the host and polygons have variable length.  Parity with cv2 itself is UNPINNED (cv2 is absent where the fixtures are made).
 *   Returns 1 for a null xy with n > 0, negative n, or a coordinate that is not finite or outside +-2^30.
 *
 * OUTPUTS (device): value fp64 [B]; obj fp64 [T_all], unrounded; kpt fp64 [T_all,K]; match int32 [T_all]; status int32 [B], with
 *   T_all = t_off[B].  Every element is written exactly once; nothing is carried between calls; deterministic.
 * hh_pose_score_batch: the launch.  The tables are plain arguments: the set of descriptor structs of ABI version 3 is closed.  A
 *   table whose contents the host must check comes twice, as the device address the kernel reads (`*_dev`) and as the caller's host
 *   copy of the same values (`*_host`), which is what is checked: device memory is never read back.  joints, scores, num, flags, p_xy,
 *   p_score exist on the device only.  vars and alpha are host values and travel in the launch's arguments.  The arguments of the form
 *   that is not chosen are not looked at (pass NULL / 0).
 * hh_pose_score_host: the same text compiled for the host; every table lies in HOST memory (in either form) and is passed once.
 * hh_pose_score_config: out = {threads per workgroup, dynamic LDS bytes at the maxima, HH_POSE_MAX_T, HH_POSE_MAX_P}.
 * Refused with 1 before any launch, hh_last_error naming the image where there is one: a null pointer (flags excepted), an fp64 table
 *   or output that is not 8-byte aligned, another that is not 4-byte aligned, B < 0 or over 2^24, K outside 1..HH_POSE_MAX_K,
 *   max_people outside 1..HH_POSE_MAX_P or a negative stride (DECODE), offsets that do not start at 0 or that decrease, an image with
 *   more than HH_POSE_MAX_T targets or HH_POSE_MAX_P predictions (refused, never capped), a target with no labelled joint, a
 *   non-finite target value, an area or var that is not finite and > 0, a head size that is not finite and >= 0, a non-finite alpha or
 *   inverse matrix, an unknown form or metric. */
#define HH_POSE_MAX_T 128 /* targets per image */
#define HH_POSE_MAX_P 64  /* predictions per image */
#define HH_POSE_MAX_K 64
enum { HH_POSE_PRED_DECODE = 0, HH_POSE_PRED_F64 = 1 };
enum { HH_POSE_METRIC_OKS = 0, HH_POSE_METRIC_PCKH = 1 };
enum { HH_POSE_NONFINITE = 1, HH_POSE_NO_PRED = 2 };
int hh_pose_score_batch(int form, int metric, int B, int K,
                        const float *joints, int64_t image_stride, int64_t person_stride, int64_t joint_stride, const float *scores,
                        int64_t score_stride, const int32_t *num, const int32_t *flags, int max_people, const double *inv_affine_dev,
                        const double *inv_affine_host,
                        const int32_t *p_off_dev, const int32_t *p_off_host, const double *p_xy, const double *p_score,
                        const int32_t *t_off_dev, const int32_t *t_off_host, const double *t_xyv_dev, const double *t_xyv_host,
                        const double *t_area_dev, const double *t_area_host, const double *t_head_dev, const double *t_head_host,
                        const double *vars_host, double alpha,
                        double *value, double *obj, double *kpt, int32_t *match, int32_t *status, void *stream);
int hh_pose_score_host(int form, int metric, int B, int K,
                       const float *joints, int64_t image_stride, int64_t person_stride, int64_t joint_stride, const float *scores,
                       int64_t score_stride, const int32_t *num, const int32_t *flags, int max_people, const double *inv_affine,
                       const int32_t *p_off, const double *p_xy, const double *p_score,
                       const int32_t *t_off, const double *t_xyv, const double *t_area, const double *t_head,
                       const double *vars, double alpha,
                       double *value, double *obj, double *kpt, int32_t *match, int32_t *status);
int hh_polygon_area(const double *xy, int n, double *area);
int hh_pose_score_config(int out[4]);

/* HeatmapGenerator (coco.py:77-121) as a gather over the packed joints the grouping loss takes (hh_loss_ae_grouping: joints int32
 * [B,P,K,3] = x, y, vis from JointsGenerator, coco.py:124-137; num_people [B]): out fp32 [B,K,h,w], each element the maximum over
 * the image's people p < num_people[b] with vis > 0 and (x, y) inside the map of table[y - y_p + reach][x - x_p + reach] where that
 * index is inside the table, else 0.  `table` (device) is the reference's `gauss` (coco.py:89-92: float64 exp) cast to fp32,
 * [n,n] with n = 2 * reach + 1 = 6 sigma + 3.  Bit-identical to the reference's float32 maps: the cast is monotone, max is
 * order-free.  Every element is written exactly once (no memset first); deterministic.  One launch per stage.
 * hh_heatmap_table_size (host-side): n and reach for a sigma; refuses a sigma for which 3 sigma + 1 is not an integer (the
 * reference's np.round of the window corners then depends on the parity of the joint) or n > 63.                            */
int hh_heatmap_table_size(double sigma, int *n, int *reach);
int hh_render_heatmaps(const int32_t *joints, const int32_t *num_people, int B, int P, int K, const float *table, int n, int reach,
                       float *out, int h, int w, void *stream);

/* The classifier's input built on the device: classification/transforms.py:14-30 (ClassificationTransform.train: ToTensor ->
 * RandomResizedCrop(224, antialias=True) -> RandomHorizontalFlip -> Normalize; .inference: ToTensor -> Resize(256, antialias=True) ->
 * CenterCrop(224) -> Normalize) and classification/model.py:45-57 (InferenceClassificationModel: Resize + CenterCrop of input_size),
 * batched, one launch.  Raw uint8 pixels and descriptors lie in ONE device buffer that the caller ships in one host->device copy.
 * The random draws and the Resize / CenterCrop geometry stay on the host (classification/input.py).
 *
 * hh_crop_desc: one sample.  Image uint8 RGB [h,w,3] at batch_base + image_offset.  (top, left, ch, cw) is the source rectangle: the
 *   whole image for Resize, the drawn crop for RandomResizedCrop.  That rectangle is resampled to a VIRTUAL image of rh x rw, of
 *   which only the H x W window at (oy, ox) is computed (CenterCrop; the whole of it when rh x rw = H x W).  flip != 0 reverses the
 *   window's columns.  For sample b, channel c and output pixel (y, x), with xs = flip ? W-1-x : x:
 *     out[b,c,y,x] = (resample(crop_b(ToTensor(image_b)))[c, oy + y, ox + xs] - mean[c]) / stdv[c]
 * resample is torch's upsample_bilinear2d_aa with align_corners = False (what torchvision's tensor resize / resized_crop run),
 *   separable, the horizontal pass first, its result kept as fp32.  Per axis, with in = crop extent, out = virtual size,
 *   scale = in / out and support = antialias ? max(scale, 1) : 1: centre = scale (i + 0.5); taps
 *   j in [max(0, int(centre - support + 0.5)), min(in, int(centre + support + 0.5))); weight max(0, 1 - |(j - centre + 0.5) / support|),
 *   normalised to sum 1.  There is no cap on the tap count.  Tap indices are relative to the crop and never leave it (pixels of the
 *   image outside the rectangle do not contribute, as for a tensor that was cropped first).  antialias = 0 is
 *   F.interpolate(mode="bilinear", antialias=False): torchvision's T.Resize default changed between versions, so the caller says.
 * Arithmetic: all fp32; ToTensor is the division v / 255.0f, Normalize a subtraction then a division (no reciprocal), products and
 *   sums rounded separately, the taps summed in ascending order.  A crop whose extent equals the virtual size on both axes gives
 *   Normalize(ToTensor(.)) of the source pixels bit for bit.  Deterministic; every output element is written exactly once.
 * Validation: `descs_dev` is the DEVICE array the kernel reads; `descs_host` is the caller's HOST copy of the same n descriptors, and
 *   it is what is checked (device memory is never read back).  Returns 1 with hh_last_error set, before any launch, for a null
 *   pointer, a non-positive extent, a rectangle outside its image, a window outside rh x rw, a negative offset, an image of
 *   h * w * 3 >= 2^31 bytes (the kernel indexes one image's bytes with 32 bits), a side beyond 2^23 (tap positions are formed in
 *   fp32), n outside 1..65535, H or W outside 1..32768.  That the image bytes lie inside the caller's buffer cannot be checked here.
 * (Additive entry point: HH_ABI_VERSION stays 3.)                                                                          */
#define HH_CROP_MAX_SIDE (1 << 23)
#define HH_CROP_MAX_EXTENT 32768
typedef struct hh_crop_desc {
    long long image_offset;      /* bytes from batch_base: uint8 RGB [h,w,3] */
    int h, w;                    /* raw image */
    int top, left, ch, cw;       /* source rectangle (the crop), inside the image */
    int rh, rw;                  /* size of the virtual resized crop */
    int oy, ox;                  /* origin of the H x W output window inside it */
    int flip, antialias;
} hh_crop_desc;
int hh_resized_crop_u8_batch(const unsigned char *batch_base, const hh_crop_desc *descs_dev, const hh_crop_desc *descs_host, int n,
                             float *out_nchw, int H, int W, const float mean[3], const float stdv[3], void *stream);

/* Building blocks of the training step (keypoints/module.py:43-71), assembled into the net's training forward / backward
 * by keypoints/train_net.py with torch autograd as the tape.  Activations are NHWC bf16 [B,H,W,C] (= torch channels_last),
 * parameters fp32, all device pointers.
 *
 * Element type.  Every entry point below that reads or writes an activation (or a packed weight set) has a second form with the
 * suffix _dt, whose first argument `act_dtype` is HH_ACT_BF16 or HH_ACT_F16: the 16-bit format of ALL activation tensors of that
 * call, of the packed weights, and the MFMA form that multiplies them (the reference trains under fp16 autocast with a GradScaler,
 * keypoints/module.py:43-71).  The unsuffixed function is its _dt form with HH_ACT_BF16.  Any other value returns 1 with
 * hh_last_error set, before anything is launched.  Workspace, element-count and plan functions do not depend on the type.
 * fp16 semantics (HH_ACT_F16):
 *   - every store rounds to nearest even;
 *   - a value beyond +-65504 becomes +-inf.  It is NOT saturated: the loss scaler detects an oversized scale by it;
 *   - NaN / inf in a gradient tensor reach the data gradient and the fp32 weight, gamma and beta gradients as non-finite values
 *     (an exception by construction: an element the ReLU mask zeroes carries nothing, whatever it held);
 *   - subnormals are kept by every store and every fp32 <-> fp16 conversion (the kernels are compiled in the default mode).
 *     Whether the f16 MFMA honours subnormal A / B INPUTS on gfx950 is decided by the subnormal case of
 *     tests/test_gpu_train_f16_lattice.py; INTEGRATION.md records the outcome.
 * (Additive entry points: HH_ABI_VERSION stays 3.)
 *
 * hh_conv2d: y = act(conv(x, w) + bias (+ res)) with the CURRENT fp32 weights w [cout][cin][ks][ks] (packed on the device
 *   each call), ks in {1,2,3} (2x2: stride 1), stride in {1,2}; pad_y / pad_x = top / left zero padding, -1 = (ks-1)/2
 *   (the output keeps the input size at stride 1, so a 2x2 kernel with pad 0 pads bottom/right instead).  mode 1 = data gradient of the stride-1 conv with these
 *   weights: x is dL/dy [B,H,W,cout], y is dL/dx [B,H,W,cin] (the same kernel with rotated, transposed weights).
 *   mode 2 = data gradient of the 3x3 stride-2 conv: x is dL/dy [B,H,W,cout], y is dL/dx [B,2H,2W,cin] (four
 *   output-parity phases, each a 2x2 conv over dL/dy).
 *   Input channels (of the conv that runs) % 16 == 0, output channels % 8 == 0; workspace: hh_conv2d_workspace_bytes.
 * hh_bn_train_forward = nn.BatchNorm2d in training mode on [P = B*H*W, C] (+ residual, + ReLU): batch mean and biased
 *   variance, y = act(gamma * (x - mean) * invstd + beta (+ res)); mean / invstd are kept for the backward.
 *   scratch: 256 * C * 2 doubles.  (The running statistics are updated by the caller: plain torch arithmetic on C floats.)
 * hh_bn_train_backward: dx, dgamma, dbeta (and dres = the gradient after the ReLU mask, if dres != NULL).
 * hh_bn_train_backward_plain: the same for a BatchNorm that had no residual input, without its stored output y: no ReLU needs
 *   nothing of it, and with ReLU the mask y > 0 is recomputed from x (gamma * (x - mean) * invstd + beta > 0, evaluated by the
 *   function the forward evaluated) -- one tensor pass less in each of the two kernels.
 * hh_conv2d_wgrad: dw [cout][cin][ks][ks] fp32 = dL/dW of y = conv(x, W) (padding (ks-1)/2) from x [B,H,W,cin] and
 *   dy [B,Ho,Wo,cout]; 3x3 stride 1/2 and 1x1 stride 1, channel counts % 8 == 0.  A GEMM contracted over pixels on MFMA
 *   (operands read from LDS with the transposing ds_read_b64_tr_b16), partial sums reduced in a fixed order.          */
#define HH_ACT_BF16 0
#define HH_ACT_F16 1
int64_t hh_conv2d_workspace_bytes(int cin, int cout, int ks, int mode);
/* What would run, as host arithmetic alone (no device call; the selection code of the launches themselves):
 *   hh_conv2d_config: the index (see hh_conv_config) of the instantiation hh_conv2d / hh_conv2d_packed launch for these
 *     arguments on a map whose launched conv writes Wo columns (W at stride 1, W / 2 at stride 2, the W of dL/dy in mode 2,
 *     whose four phase convs each write that many); -1 where they refuse the shape.
 *   hh_conv2d_wgrad_plan: out = {kernel variant 0..5 (3x3 narrow maps, 3x3 small channel counts, 3x3, 1x1, 3x3 stride 2, 2x2),
 *     persistent workers per channel block, pixel tiles they share}; 1 where hh_conv2d_wgrad refuses the shape.
 *   (Additive diagnostic entry points: HH_ABI_VERSION stays 3.)                                                         */
int hh_conv2d_config(int cin, int cout, int ks, int stride, int mode, int Wo);
int hh_conv2d_wgrad_plan(int B, int H, int W, int cin, int cout, int ks, int stride, int out[3]);
int64_t hh_conv2d_wgrad_workspace_bytes(int B, int H, int W, int cin, int cout, int ks, int stride);
int hh_conv2d_wgrad(const void *x, const void *dy, int B, int H, int W, int cin, int cout, int ks, int stride, int pad_y, int pad_x, float *dw,
                    void *workspace, void *stream);
int hh_conv2d_wgrad_dt(int act_dtype, const void *x, const void *dy, int B, int H, int W, int cin, int cout, int ks, int stride, int pad_y,
                       int pad_x, float *dw, void *workspace, void *stream);
int hh_conv2d(const void *x, int B, int H, int W, int cin, const float *w, int cout, int ks, int stride, int mode, int pad_y, int pad_x,
              const float *bias, const void *res, int relu, void *y, void *workspace, void *stream);
int hh_conv2d_dt(int act_dtype, const void *x, int B, int H, int W, int cin, const float *w, int cout, int ks, int stride, int mode, int pad_y,
                 int pad_x, const float *bias, const void *res, int relu, void *y, void *workspace, void *stream);
/* The same convolution with weights packed ahead of it.  A training step packs ~700 weight sets (forward layout and
 * data-gradient layout of every conv); as separate launches that is ~700 tiny dependent kernels whose launch gaps cost more
 * than the packing.  hh_pack_conv_weights_batch packs n weight sets in ONE launch: w[i] fp32 [cout][cin][ks][ks] (device
 * pointers in a HOST array), packed[i] device buffers of hh_conv2d_packed_elems(cin, cout, ks, stride, mode) bf16 elements,
 * shapes host int32 [n][5] = cout, cin, ks, stride, mode (modes as in hh_conv2d), descs_dev a device scratch of
 * n * 4 * 64 bytes.  hh_conv2d_packed = hh_conv2d on such a buffer (bias NULL or a multiple of 32 long).  The packed copy
 * is valid until the fp32 weights change (the optimizer step).  hh_pack_conv_weights_batch_dt: act_dtype is the format of all n
 * packed buffers of the call (16-bit elements either way); hh_conv2d_packed_dt must be given the dtype they were packed with.    */
int64_t hh_conv2d_packed_elems(int cin, int cout, int ks, int stride, int mode);
int hh_pack_conv_weights_batch(int n, const float *const *w, void *const *packed, const int32_t *shapes, void *descs_dev, void *stream);
int hh_pack_conv_weights_batch_dt(int act_dtype, int n, const float *const *w, void *const *packed, const int32_t *shapes, void *descs_dev,
                                  void *stream);
int hh_conv2d_packed(const void *x, int B, int H, int W, int cin, const void *w_packed, int cout, int ks, int stride, int mode, int pad_y,
                     int pad_x, const float *bias, const void *res, int relu, void *y, void *stream);
int hh_conv2d_packed_dt(int act_dtype, const void *x, int B, int H, int W, int cin, const void *w_packed, int cout, int ks, int stride, int mode,
                        int pad_y, int pad_x, const float *bias, const void *res, int relu, void *y, void *stream);
int hh_bn_train_forward(const void *x, int64_t P, int C, const float *gamma, const float *beta, float eps, const void *res, int relu,
                        void *y, float *mean, float *invstd, double *scratch, void *stream);
int hh_bn_train_backward(const void *x, const void *y, const void *dy, int64_t P, int C, const float *mean, const float *invstd,
                         const float *gamma, int relu, void *dx, void *dres, float *dgamma, float *dbeta, double *scratch, void *stream);
int hh_bn_train_backward_plain(const void *x, const void *dy, int64_t P, int C, const float *mean, const float *invstd, const float *gamma,
                               const float *beta, int relu, void *dx, float *dgamma, float *dbeta, double *scratch, void *stream);
int hh_bn_train_forward_dt(int act_dtype, const void *x, int64_t P, int C, const float *gamma, const float *beta, float eps, const void *res,
                           int relu, void *y, float *mean, float *invstd, double *scratch, void *stream);
int hh_bn_train_backward_dt(int act_dtype, const void *x, const void *y, const void *dy, int64_t P, int C, const float *mean, const float *invstd,
                            const float *gamma, int relu, void *dx, void *dres, float *dgamma, float *dbeta, double *scratch, void *stream);
int hh_bn_train_backward_plain_dt(int act_dtype, const void *x, const void *dy, int64_t P, int C, const float *mean, const float *invstd,
                                  const float *gamma, const float *beta, int relu, void *dx, float *dgamma, float *dbeta, double *scratch,
                                  void *stream);

/* FusionLayer's sum in the training step (hrnet.py:214-229: `sum_j f_ij(x_j)` then ReLU, with nn.Upsample(nearest) on the
 * low-resolution terms, hrnet.py:200-205): out = act(sum_j term_j[b, y >> shift_j, x >> shift_j, :]) over 1..4 NHWC bf16
 * terms [B, H >> shift_j, W >> shift_j, C] (shift 0 first), summed in fp32 -- the upsampled tensors are never materialised.
 * Backward: g = dy * (out > 0) [B,H,W,C] is the gradient of every shift-0 term (g may be NULL when relu == 0: then it is dy
 * itself); dup[j] [B, H >> s, W >> s, C] = the 2^s x 2^s block sums of g for the nup upsampled terms.                     */
int hh_fusion_sum_forward(const void *const *terms, const int *shifts, int nterms, int B, int H, int W, int C, int relu, void *out, void *stream);
int hh_fusion_sum_backward(const void *dy, const void *out, int relu, int B, int H, int W, int C, void *g, void *const *dup, const int *up_shift,
                           int nup, void *stream);
int hh_fusion_sum_forward_dt(int act_dtype, const void *const *terms, const int *shifts, int nterms, int B, int H, int W, int C, int relu, void *out,
                             void *stream);
int hh_fusion_sum_backward_dt(int act_dtype, const void *dy, const void *out, int relu, int B, int H, int W, int C, void *g, void *const *dup,
                              const int *up_shift, int nup, void *stream);

/* SyncBatchNorm (src/base/model.py:42-44: `to_DDP(..., use_batchnorm=True)` converts every BatchNorm2d, the reference
 * trainer's default, trainer.py:44,253; experiments/keypoints/higher_hrnet_32.yaml:17 turns it off): the two passes above split around their one exchange step.
 *   hh_bn_train_stats:          sums[2c], sums[2c+1] = sum x, sum x^2 over THIS rank's P pixels (doubles).
 *   -- the caller all-reduces (SUM) sums and the pixel count over the ranks (RCCL) --
 *   hh_bn_train_normalize:      mean / invstd from the global sums and count, then the same apply pass.
 *   hh_bn_train_backward_stats: sums = sum g, sum g * xhat of this rank (g = dy after the ReLU mask); dbeta / dgamma = the
 *                               same local sums as floats (parameter gradients are averaged by DDP like all others).
 *   -- all-reduce (SUM) sums --
 *   hh_bn_train_backward_apply: dx (and dres) from the global sums and count.
 * With count == P and no exchange the results equal hh_bn_train_forward / hh_bn_train_backward.  scratch: 256*C*2 doubles. */
int hh_bn_train_stats(const void *x, int64_t P, int C, double *sums, double *scratch, void *stream);
int hh_bn_train_normalize(const void *x, int64_t P, int C, const double *sums, double count, const float *gamma, const float *beta, float eps,
                          const void *res, int relu, void *y, float *mean, float *invstd, void *stream);
int hh_bn_train_backward_stats(const void *x, const void *y, const void *dy, int64_t P, int C, const float *mean, const float *invstd, int relu,
                               double *sums, float *dgamma, float *dbeta, double *scratch, void *stream);
int hh_bn_train_backward_apply(const void *x, const void *y, const void *dy, int64_t P, int C, const float *mean, const float *invstd,
                               const float *gamma, int relu, const double *sums, double count, void *dx, void *dres, double *scratch,
                               void *stream);
int hh_bn_train_stats_dt(int act_dtype, const void *x, int64_t P, int C, double *sums, double *scratch, void *stream);
int hh_bn_train_normalize_dt(int act_dtype, const void *x, int64_t P, int C, const double *sums, double count, const float *gamma,
                             const float *beta, float eps, const void *res, int relu, void *y, float *mean, float *invstd, void *stream);
int hh_bn_train_backward_stats_dt(int act_dtype, const void *x, const void *y, const void *dy, int64_t P, int C, const float *mean,
                                  const float *invstd, int relu, double *sums, float *dgamma, float *dbeta, double *scratch, void *stream);
int hh_bn_train_backward_apply_dt(int act_dtype, const void *x, const void *y, const void *dy, int64_t P, int C, const float *mean,
                                  const float *invstd, const float *gamma, int relu, const double *sums, double count, void *dx, void *dres,
                                  double *scratch, void *stream);

/* The classification head's tail in training form (classification/architectures/hrnet.py:55-61, classification/loss.py,
 * classification/module.py:15-22); keypoints/train_net.py puts it behind the 4-scale backbone.  All device pointers.
 * (Additive entry points: HH_ABI_VERSION stays 3.)
 *   hh_global_avgpool: out fp32 [B,C] = the mean over the HW pixels of x [B,HW,C] (NHWC, 16-bit), summed in fp32 in pixel order and
 *     divided by HW; C % 8 == 0.  The kernel the inference engine runs.  hh_global_avgpool_backward: dx [B,HW,C] (16-bit) =
 *     g[b,c] / HW at every pixel, rounded to nearest even.  Both touch activations: the forms with the suffix _act take
 *     act_dtype = HH_ACT_BF16 / HH_ACT_F16 in front, with the meaning it has for the _dt forms above; the unsuffixed ones are bf16.
 *   hh_linear_forward: y [B,N] = x [B,K] W[N,K]^T + bias, fp32 throughout (nn.Linear; the engine's kernel).
 *   hh_linear_backward: dx [B,K] = dy W, dw [N,K] = dy^T x and db [N] = sum_b dy, fp32, every sum in an order that depends
 *     on the shape alone: identical bits from call to call.  dx, dw, db may each be NULL (not computed); w is read only for dx, x only for dw.
 *   hh_softmax_xent: nn.CrossEntropyLoss() (mean over the batch, no label smoothing) on logits fp32 [B,N] and targets int64 [B], its
 *     gradient and the classification metrics in ONE launch.  result (device, 16 bytes, read with one copy):
 *       loss   = (1/B) sum_b (max_b + log sum_j exp(z_bj - max_b) - z_bt), the row sums and the batch sum in double, fixed order;
 *       top1, top5 = the number of rows whose target has rank < 1 / < 5, where
 *                rank = #{j : z_j > z_t} + #{j < t : z_j == z_t}
 *              (ties go to the lower index, the project's rule; torch.topk leaves the order of equal values unspecified);
 *       flags  bit 0: some target is outside [0, N).  Such a row adds nothing to loss, top1, top5, its dlogits row is zero, and no
 *              logit is read at its index.  The caller decides what to do about it (classification/loss.py raises when it reads
 *              the record).
 *     dlogits fp32 [B,N] = (softmax(z) - onehot(t)) / B, or NULL.                                                              */
typedef struct hh_xent_result {
    float loss;
    int32_t top1, top5;
    uint32_t flags;
} hh_xent_result;
int hh_global_avgpool(const void *x, int B, int HW, int C, float *out, void *stream);
int hh_global_avgpool_act(int act_dtype, const void *x, int B, int HW, int C, float *out, void *stream);
int hh_global_avgpool_backward(const float *g, int B, int HW, int C, void *dx, void *stream);
int hh_global_avgpool_backward_act(int act_dtype, const float *g, int B, int HW, int C, void *dx, void *stream);
int hh_linear_forward(const float *x, const float *w, const float *bias, int B, int K, int N, float *y, void *stream);
int hh_linear_backward(const float *x, const float *w, const float *dy, int B, int K, int N, float *dx, float *dw, float *db, void *stream);
int hh_softmax_xent(const float *logits, const int64_t *targets, int B, int N, float *dlogits, hh_xent_result *result, void *stream);

/* Evaluation of the classifier on the device (csrc/cls_score.hip, csrc/cls_score_math.h; classification/evaluation.py ClsEvaluator,
 * evaluate_images): top-k, rank, loss and the running state of a whole evaluation from a batch of logits, nothing read back.  The
 * reference has no evaluation script (its bin/eval.py is a stub); the metric names are those of its get_metrics.
 * (Additive entry points: HH_ABI_VERSION stays 3.)
 *
 * INPUTS: logits fp32 [B,N] contiguous, targets int64 [B] or NULL, 0 <= B <= HH_CLS_MAX_B, 1 <= N <= HH_CLS_MAX_N,
 *   1 <= k <= HH_CLS_TOPK_MAX; k_eff = min(k, N).
 * RULE for one row z[0..N), target t:
 *   ORDER.  j comes before j' iff z_j > z_j', or z_j == z_j' and j < j' (ties go to the lower index, the project's rule; -0.0 == +0.0
 *     is a tie).  It is decided on the logits as given, with comparisons only.  topk_idx[0..k_eff) = the first k_eff indices in this
 *     order; entries k_eff..k-1 get index -1 and probability 0.
 *   NON-FINITE ROW.  A row that holds a NaN or a +inf (-inf entries are ordinary), or that holds nothing but -inf (max z = -inf:
 *     z - max is not a number), is a non-finite row: flag bit 1 (HH_CLS_NONFINITE); every topk_idx = -1, every topk_prob = 0,
 *     rank = -1, row_loss = 0; it adds 1 to `nonfinite` and nothing else, whatever its target.
 *   SOFTMAX.  m = max_j z_j; sum = sum_j (double)expf(z_j - m) in the per-row order of hh_softmax_xent: lane l of 64 adds its
 *     elements j = l, l + 64, ... in ascending j into a double that starts at 0, then the 64 partial sums go through the shuffle tree
 *     s_l += s_(l xor o) for o = 32, 16, 8, 4, 2, 1.  topk_prob_i = (float)((double)expf(z_i - m) / sum).
 *   TARGET.  Without targets: rank = -1, row_loss = 0.  A t outside [0, N): flag bit 0 (HH_CLS_BAD_TARGET); the row adds 1 to
 *     `bad_target` and otherwise only writes its top-k; rank = -1, row_loss = 0; no logit is read at its index.
 *   RANK AND LOSS.  rank = #{j : z_j > z_t} + #{j < t : z_j == z_t};  row_loss = (float)(((double)m + log(sum)) - (double)z_t),
 *     the double kept for the accumulator.  A top-1 hit is rank < 1, a top-k hit rank < k_eff.
 * ACCUMULATOR (device; hh_cls_eval_bytes(N, with_confusion) bytes, 8-byte aligned, owned by the caller, set up by hh_cls_eval_reset).
 *   It is passed as a plain pointer: the set of descriptor structs of ABI version 3 is closed, so its 64-byte header hh_cls_eval_acc is
 *   defined in csrc/cls_score_math.h and stated here by offset (classification/evaluation.py ACC_HEADER is the same list):
 *     int64 rows @0, top1 @8, topk @16, bad_target @24, nonfinite @32; double loss_sum @40; uint32 flags @48; int32 N @52,
 *     with_confusion @56, reserved @60.
 *   Behind the header: int32 per_class[3][N] = the scored rows, the top-1 hits and
 *   the top-k hits by target class, then with confusion int32 conf[N][N], conf[t][topk_idx[0]] += 1 per scored row, then (8-byte
 *   aligned) the call scratch: double [HH_CLS_MAX_B] and int32 [HH_CLS_MAX_B], all zero between calls.  A scored row (finite, target in
 *   range) adds 1 to rows, its hits to top1 / topk, its row to per_class and conf.  The int32 tables limit one evaluation to 2^31 - 1
 *   rows.  The accumulator is written only when both targets and acc are given; every per-row output pointer may be NULL.
 *   ORDER OF loss_sum.  loss_sum grows by the scored rows' double losses one at a time, in ascending row order, so every byte of the
 *     accumulator after an evaluation is independent of how its rows were split into calls (given the same device expf / log).
 *   If the header's N is not the call's N (or with_confusion is not 0 / 1) the call sets flag bit 2 (HH_CLS_LAYOUT) and touches
 *     nothing else of the accumulator.
 * LAUNCHES.  hh_cls_score_batch is one launch without an accumulator and two with one: cls_score_kernel, one wave per row, four rows
 *   per workgroup, which leaves each row's double loss and status in the scratch and adds to per_class / conf with vector atomics; then
 *   cls_fold_kernel, one wave, which adds the scratch to the header in row order and zeroes it.  A row of N <= HH_CLS_ROW_REGS (1024)
 *   is held in the wave's registers (16 per lane) across the passes; a longer one is read again from memory on every pass (max, sum,
 *   rank, k_eff arg-max rounds), with the same results.
 * hh_cls_score_host / hh_cls_eval_reset_host: the same text compiled for the host over HOST memory (accumulator included).
 * Each returns 1 with hh_last_error set (hh_cls_eval_bytes: -1), before any launch, for a null logits pointer, B, N or k outside its
 *   range, with_confusion not 0 / 1, an accumulator or targets pointer that is not 8-byte aligned, another that is not 4-byte aligned.  */
#define HH_CLS_TOPK_MAX 8
#define HH_CLS_MAX_B 1024
#define HH_CLS_MAX_N 65536
#define HH_CLS_ROW_REGS 1024
enum { HH_CLS_BAD_TARGET = 1, HH_CLS_NONFINITE = 2, HH_CLS_LAYOUT = 4 };
int64_t hh_cls_eval_bytes(int N, int with_confusion);
int hh_cls_eval_reset(void *acc, int N, int with_confusion, void *stream);
int hh_cls_eval_reset_host(void *acc, int N, int with_confusion);
int hh_cls_score_batch(const float *logits, const int64_t *targets, int B, int N, int k, void *acc, int32_t *topk_idx, float *topk_prob,
                       int32_t *rank, float *row_loss, void *stream);
int hh_cls_score_host(const float *logits, const int64_t *targets, int B, int N, int k, void *acc, int32_t *topk_idx, float *topk_prob,
                      int32_t *rank, float *row_loss);

/* The end of the training step on the device (csrc/optim.hip): what torch.optim.Adam / AdamW / SGD and the GradScaler's non-finite
 * check do over ~900 parameter tensors, each as ONE launch over a device-resident table (the Python classes are
 * pytorch-human-pose_amd/optim.py; the reference picks its optimizer in utils/optim.py:40-45).  Parameters, gradients and state are
 * fp32 device tensors, contiguous, at any 4-byte alignment (float4 access where all of a chunk's pointers are 16-byte aligned).
 * (Additive entry points: HH_ABI_VERSION stays 3.)
 *
 * hh_optim_tensor: one parameter.  state0 / state1 = exp_avg / exp_avg_sq (Adam, AdamW) or momentum_buffer / unused (SGD; state0 may
 *   be NULL where the group's momentum is 0).  step = the tensor's fp32 step counter on the device (torch's state[p]["step"]; Adam and
 *   AdamW only).  group indexes the hyper-parameter blocks.
 * hh_optim_group: doubles, as Python holds them; the bias corrections 1 - beta^step are formed from them in fp64 on the device.
 *   momentum / nesterov: SGD (dampening is 0); beta1 / beta2 / eps: Adam and AdamW; weight_decay: L2 for Adam and SGD, decoupled
 *   (p *= 1 - lr * weight_decay) for AdamW.
 * hh_optim_table_bytes: the size of `table_dev` for these tensors (it holds the descriptors, one entry per 4096-element chunk of
 *   every tensor, and the group blocks); -1 on a bad argument.
 * hh_optim_step: one update launch over all chunks plus, for Adam / AdamW, a one-workgroup launch that adds 1 to every step counter
 *   (no workgroup reads a counter another one of the same launch has advanced).  `upload` says which parts of the table this call
 *   copies into table_dev first (one hipMemcpyAsync on `stream`): HH_OPTIM_UPLOAD_ALL, or less where the caller knows that table_dev
 *   still holds the same part from its previous call with the same arguments.  grad_scale / found_inf (device fp32 scalars, either may be
 *   NULL) are the contract torch.amp.GradScaler.step offers an optimizer with _step_supports_amp_scaling: with *found_inf != 0 nothing
 *   is stored at all -- parameters, state and counters keep their bits; otherwise g / *grad_scale is used and written back to grad.
 * hh_grads_nonfinite: *found_inf = 1.0f if any element of any gradient is inf or NaN (the caller zeroes it first), and, unless
 *   inv_scale is NULL or holds 1, every gradient is multiplied by *inv_scale in place (_amp_foreach_non_finite_check_and_unscale_).
 *   Works on the same table; its upload may be 0 or HH_OPTIM_UPLOAD_TENSORS (it does not read the groups).
 * Non-zero (nothing launched or copied) for an unknown algorithm, null tables or table pointers, a negative numel or count, a
 * group index outside [0, ngroups), a beta outside [0, 1), a table_dev that is not 16-byte aligned or smaller than hh_optim_table_bytes. */
#define HH_OPTIM_ADAM 0
#define HH_OPTIM_ADAMW 1
#define HH_OPTIM_SGD 2
#define HH_OPTIM_UPLOAD_TENSORS 1 /* descriptors and chunk list */
#define HH_OPTIM_UPLOAD_GROUPS 2  /* hyper-parameter blocks */
#define HH_OPTIM_UPLOAD_ALL 3
typedef struct hh_optim_tensor {
    float *param, *grad, *state0, *state1, *step;
    int64_t numel;
    int32_t group, reserved;
} hh_optim_tensor;
typedef struct hh_optim_group {
    double lr, beta1, beta2, eps, weight_decay, momentum;
    int32_t nesterov, reserved;
} hh_optim_group;
int64_t hh_optim_table_bytes(const hh_optim_tensor *tensors_host, int ntensors, int ngroups);
int hh_optim_step(int algo, const hh_optim_tensor *tensors_host, int ntensors, const hh_optim_group *groups_host, int ngroups,
                  const float *grad_scale, const float *found_inf, void *table_dev, int64_t table_bytes, int upload, void *stream);
int hh_grads_nonfinite(const hh_optim_tensor *tensors_host, int ntensors, int ngroups, const float *inv_scale, float *found_inf,
                       void *table_dev, int64_t table_bytes, int upload, void *stream);

/* Gradient statistics and clipping by global norm on that table (csrc/grad_stats.hip; optim.clip_grad_norm_ and
 * optimizer.grad_stats() of pytorch-human-pose_amd/optim.py): torch.nn.utils.clip_grad_norm_ and the per-layer mean / max |grad|
 * that the reference's trainer lists as its open TODO (src/base/trainer.py:23-26), from ONE read of the gradients.
 * (Additive entry points: HH_ABI_VERSION stays 3.  hh_optim_table_bytes and the two structs are unchanged.)
 *
 * hh_grad_stats_bytes: the size of `work_dev` for these tensors; -1 on a bad argument.  work_dev (16-byte aligned) begins with
 *   float totals[4] = {total_l2, total_inf, coef, unused} and float rows[ntensors][4] = {l2, absmax, absmean, nonfinite_count} per
 *   tensor in table order; behind them the per-tensor fp64 sums of squares, one 24-byte record per 4096-element chunk (double sum of
 *   g^2, double sum of |g|, float max |g|, int non-finite count) and the index of every tensor's first chunk, all written on the device.
 * hh_grad_stats: one launch over all chunks, one per tensor, one that forms the totals.  With found_inf != NULL the first is also
 *   hh_grads_nonfinite, with the same stored bits: *found_inf = 1.0f on an inf / NaN (the caller zeroes it first), g *= *inv_scale in
 *   place unless inv_scale is NULL or holds 1.  The statistics are those of the value that is stored (the unscaled gradient).
 *   Squares and sums are formed in fp64 and added in one fixed order (no floating-point atomics): the same bits on every run.
 *   total_l2 = (float)sqrt(sum over all elements of g^2), rounded once; total_inf = max of the absmax column.
 *   NaN / inf, as g.norm(), g.abs().max() and g.abs().mean(): a NaN anywhere in a tensor makes its l2, absmax and absmean NaN, an inf
 *   (without a NaN) makes them inf, and the totals follow; a tensor with numel == 0 has the row {0, 0, 0, 0}.
 * hh_grad_clip: after hh_grad_stats on the same table_dev and work_dev.  One launch: coef = max_norm / (total + 1e-6f) in fp32, at
 *   most 1 (torch's arithmetic; total = total_l2 or total_inf by norm_type), stored to totals[2]; g = g * coef in place.  Nothing is
 *   stored to a gradient when coef >= 1 (multiplying by 1.0f is the identity), nor when found_inf != NULL and *found_inf != 0: that
 *   step is skipped by hh_optim_step anyway and the gradients stay as the unscale pass left them.  DIFFERENCE: torch would multiply
 *   them by 0 or NaN there.  Without found_inf a non-finite total gives torch's coefficient (0 or NaN) and torch's gradients.
 * Non-zero (nothing launched or copied) for what hh_grads_nonfinite refuses, a null or misaligned work_dev, a work_dev smaller than
 * hh_grad_stats_bytes, inv_scale without found_inf, a max_norm that is negative or NaN, an unknown norm type.                       */
#define HH_GRAD_NORM_L2 0
#define HH_GRAD_NORM_INF 1
int64_t hh_grad_stats_bytes(const hh_optim_tensor *tensors_host, int ntensors, int ngroups);
int hh_grad_stats(const hh_optim_tensor *tensors_host, int ntensors, int ngroups, const float *inv_scale, float *found_inf,
                  void *table_dev, int64_t table_bytes, int upload, void *work_dev, int64_t work_bytes, void *stream);
int hh_grad_clip(const hh_optim_tensor *tensors_host, int ntensors, int ngroups, float max_norm, int norm_type, const float *found_inf,
                 void *table_dev, int64_t table_bytes, void *work_dev, int64_t work_bytes, void *stream);

/* Exponential moving average (EMA) of the weights next to that table (csrc/ema.hip; optim.ModelEMA of pytorch-human-pose_amd/optim.py):
 * what torch.optim.swa_utils.AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(decay)) keeps, updated inside the optimizer's step
 * launch, with a one-launch exchange of weights and average.  (Additive entry points: HH_ABI_VERSION stays 3.  hh_optim_tensor,
 * hh_optim_group, hh_optim_table_bytes and hh_optim_step are unchanged.)
 * RULE, per element in fp32 with every operation rounded on its own, n = *n_averaged before the call:
 *   n == 0:    ema = value, the bits copied
 *   otherwise: d = warmup ? min(decay, (1 + n) / (10 + n)) : decay in fp64;  w = (float)(1.0 - d), rounded once;
 *              ema = ema + w * (value - ema)
 *   and then *n_averaged = n + 1 (a one-workgroup launch behind the update: no workgroup reads a counter that one of the same launch
 *   has advanced).  n_averaged is a device int64 scalar, like torch's.
 * DIFFERENCES from torch: (1) this one formula serves every w; torch's lerp switches to another form at w >= 0.5.  (2) With
 *   *found_inf != 0 nothing is stored at all: average and counter keep their bits, like the parameters, the optimizer state and the
 *   step counters of the skipped step; torch's AveragedModel, which cannot see the skip, would update and count.
 * hh_ema_row: one averaged fp32 tensor, `value` the live one (a parameter or a buffer) and `ema` its average, both dense with numel
 *   elements and the same memory layout.
 * hh_ema_table_bytes: the size of `ema_table_dev` for these rows next to an optimizer table of `ntensors` rows (0 for hh_ema_update /
 *   hh_ema_swap); -1 on a bad argument.  The table holds the rows, one entry per 4096-element chunk, and the row indices.
 * hh_ema_update: the stand-alone update of every row, one launch plus the counter's; found_inf may be NULL.  For any optimizer that
 *   is not hh_optim_step.  upload != 0 copies the table into table_dev first (as in hh_optim_step: 0 where table_dev still holds the
 *   same rows from the previous call of the SAME entry point; the three entry points lay the chunk list out differently).
 * hh_ema_swap: one launch that exchanges value and ema element by element; twice is the identity, bit for bit.
 * hh_optim_step_ema: hh_optim_step with its arguments, plus: the average of tensor i is rows_host[row_of_tensor[i]].ema (-1: this
 *   tensor has none and is stepped as by hh_optim_step; that row's `value` is not read, the optimizer row's param is the value), and
 *   every row that no tensor names is updated from its own `value` in the same launch (frozen parameters, floating-point buffers).
 *   Parameter, gradient, state and step-counter bits are the ones hh_optim_step stores for the same arguments.
 * Non-zero (nothing launched or copied) for: a null row table with nrows > 0, a null or misaligned (16 bytes) or too-small device
 * table, a negative numel, a null value / ema pointer, a decay outside [0, 1] or NaN, a null n_averaged, and in hh_optim_step_ema
 * whatever hh_optim_step refuses, a null row_of_tensor, a row index outside [-1, nrows), a row named by two tensors, and an optimizer
 * row whose numel differs from its EMA row's.                                                                                        */
typedef struct hh_ema_row {
    float *value, *ema;
    int64_t numel;
} hh_ema_row;
int64_t hh_ema_table_bytes(const hh_ema_row *rows_host, int nrows, int ntensors);
int hh_ema_update(const hh_ema_row *rows_host, int nrows, double decay, int warmup, int64_t *n_averaged, const float *found_inf,
                  void *table_dev, int64_t table_bytes, int upload, void *stream);
int hh_ema_swap(const hh_ema_row *rows_host, int nrows, void *table_dev, int64_t table_bytes, int upload, void *stream);
int hh_optim_step_ema(int algo, const hh_optim_tensor *tensors_host, int ntensors, const hh_optim_group *groups_host, int ngroups,
                      const float *grad_scale, const float *found_inf, void *table_dev, int64_t table_bytes, int upload,
                      const hh_ema_row *rows_host, int nrows, const int32_t *row_of_tensor, double decay, int warmup, int64_t *n_averaged,
                      void *ema_table_dev, int64_t ema_table_bytes, int ema_upload, void *stream);

/* Multi-scale test-time augmentation (BASELINE.json configs[3]; an extension: the reference only calls its resize helper
 * with scale 1, keypoints/model.py:73): dst[B,K,H,W] (+)= weight * bilinear(src[B,K,h,w] -> HxW) with the arithmetic of
 * F.interpolate(mode="bilinear", align_corners=False); init != 0 overwrites dst.  Batch strides in elements.            */
int hh_resize_accumulate(const float *src, int64_t src_bstride, int B, int K, int h, int w, float *dst, int64_t dst_bstride, int H,
                         int W, float weight, int init, void *stream);

/* The whole aggregation of that test as ONE launch (csrc/tta_aggregate.hip; the batched caller is
 * InferenceKeypointsModel.infer_images(scales=...); an extension like hh_resize_accumulate, no reference precedent).
 * For every (b,k,y,x) of dst [B,K,H,W] and the sources i = 0 .. nsrc-1 in the order given:
 *   tap_i(r,c) = hm_i[b,k,r,c]                                                     (hm_flipped NULL), or
 *              = (hm_i[b,k,r,c] + hm_flipped_i[b,perm[k],r,w_i-1-c]) / 2.0f       (hh_flip_merge's expression),
 *   v_i = weight_i * bilinear(tap_i -> HxW)(y,x)   (hh_resize_accumulate's arithmetic),  acc = v_0, then acc = acc + v_i,
 * every step rounded on its own; dst = acc is written and never read, the elements between K*H*W and dst_bstride are left alone.
 * The result equals hh_flip_merge on each flipped source followed by hh_resize_accumulate(init = (i == 0)) per source bit for
 * bit, without a merged map or a partial sum in memory.  `srcs_host` and `perm_host` are HOST arrays, copied into the launch's
 * arguments (perm_host may be NULL when no source is flipped).  Non-zero (nothing launched) for nsrc outside 1..8, K outside
 * 1..64, a NULL srcs_host / dst / hm, non-positive sizes, dst_bstride < K*H*W or a source batch stride < K*h*w.
 * (Additive entry point: HH_ABI_VERSION stays 3.)                                                                        */
#define HH_MAX_SCALE_SRCS 8
typedef struct hh_scale_src {
    const float *hm;          /* [B,K,h,w] heatmaps of one scale pass, batch stride in elements */
    long long bstride;
    const float *hm_flipped;  /* the flipped pass's maps (same h,w), or NULL: no flip merge for this source */
    long long flipped_bstride;
    int h, w;
    float weight;
} hh_scale_src;
int hh_multi_scale_aggregate(const hh_scale_src *srcs_host, int nsrc, const int32_t *perm_host, int B, int K, float *dst,
                             int64_t dst_bstride, int H, int W, void *stream);

/* Candidates of the last hh_decode/hh_parse call (MPPEHeatmapParser.top_k, grouping.py:147-170),
 * copied to host: tags_k [B,K,max_people,E], coords_k [B,K,max_people,2] (x,y), scores_k [B,K,max_people].
 * Synchronous; for parity tests.  Needs the exhaustive candidate lists: hh_decoder_set_exact_topk(dec, 1) before the decode. */
int hh_decoder_read_topk(hh_decoder *dec, float *tags_k, int32_t *coords_k, float *scores_k);

/* Test hook: the matcher's assignment solver (munkres 1.1.4's step machine, grouping.py:55-59, as one wavefront) alone on one
 * square float64 cost matrix in host memory, n <= 32: star[i] = the column assigned to row i.  Pad a rectangular problem with zeros
 * as munkres.pad_matrix does.  */
int hh_debug_munkres(const double *cost, int n, int32_t *star);

/* get_affine_transform(center, scale, rot=0, output_size, inverse) of base/transforms/utils.py:25-57 -> the 2x3 matrix
 * (row-major, 6 doubles) cv2.getAffineTransform returns for the reference's three float32 point pairs: the 6x6 system solved
 * by OpenCV's own LU in float64.  Only scale[0] enters (the reference ignores scale_h).  Host-side. */
int hh_get_affine_transform(double center_x, double center_y, double scale_w, double dst_w, double dst_h, int inverse, double out[6]);

/* The destination -> source matrix cv2.warpAffine builds from a forward 2x3 matrix (no WARP_INVERSE_MAP), same operation
 * order; what hh_preprocess_u8 / hh_warp_affine_u8 take as `dst_to_src`.  Host-side. */
int hh_invert_affine(const double m[6], double out[6]);

/* cv2.warpAffine(image, M, (W, H)) itself, uint8 HWC in and out on the device (resize_align_multi_scale,
 * base/transforms/utils.py:89-97): OpenCV's fixed-point bilinear (10-bit coordinates, 5-bit fractions, int16 weights summing to
 * 32768, (v + 2^14) >> 15), constant-0 border. */
int hh_warp_affine_u8(const unsigned char *image_hwc, int h, int w, const double dst_to_src[6], unsigned char *out_hwc, int H, int W,
                      void *stream);

/* get_final_kpts_coords / transform_coords: keypoints/results.py:158-171,189-201 with
 * get_affine_transform(inverse=True, rot=0) (hh_get_affine_transform). Host-side,
 * float64: xy_out[i] = M @ (xy_in[i], 1) as affine_transform (base/transforms/utils.py:5-8). */
int hh_transform_coords(const float *xy_in, int n, double center_x, double center_y, double scale_w, double dst_w,
                        double dst_h, double *xy_out);

#ifdef __cplusplus
}
#endif
#endif /* HHRNET_H */
