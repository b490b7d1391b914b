// extern "C" surface declared in include/hhrnet.h (network part).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hhrnet.h"
#include "engine.h"
#include "optim_math.h"
#include "grad_stats_math.h"
#include "ema_math.h"
#include "render_math.h"
#include "text_math.h"
#include "seg_overlay_math.h"
#include "panel_math.h"
#include "coco_eval_math.h"
#include "pose_score_math.h"
#include "cls_score_math.h"
#include "crowd_mask_math.h"
#include "track_math.h"
#include "jpeg_math.h"
#include "jpeg_dec_math.h"

const char *hh_get_error();
int hh_tap_read_impl(hh_net *n, int index, float *host);

// The host checks of a drawing call (render, text, seg): n in 1..65535; `call_why`, the caller's refusal of the whole call; then per
// frame a null table where rows are named (`no_table`) and frame(d) as "fn: frame b: why".  *max_tiles: the most th x tw tiles.
template <class Frame>
static int draw_check_frames(const char *fn, const hh_render_desc *descs_host, int n, const char *call_why, bool no_table, int th, int tw, int *max_tiles,
                             Frame frame)
{
    if (n <= 0 || n > 65535) { hh_set_error(std::string(fn) + ": need 0 < n <= 65535"); return 1; }
    if (call_why) { hh_set_error(std::string(fn) + ": " + call_why); return 1; }
    int tiles = 1;
    for (int b = 0; b < n; ++b) {
        const hh_render_desc &d = descs_host[b];
        if (d.prim_count > 0 && no_table) { hh_set_error(std::string(fn) + ": null primitive table"); return 1; }
        const char *why = frame(d);
        if (why) { hh_set_error(std::string(fn) + ": frame " + std::to_string(b) + ": " + why); return 1; }
        tiles = std::max(tiles, ((d.h + th - 1) / th) * ((d.w + tw - 1) / tw));
    }
    if (max_tiles) *max_tiles = tiles;
    return 0;
}

extern "C" {

int hh_abi_version(void) { return HH_ABI_VERSION; }
const char *hh_last_error(void) { return hh_get_error(); }

// stem_conv.hip and basicblock_fused.hip (the tile form) exist in bf16 only: an fp16 handle whose switches reach them would run bf16
// arithmetic on fp16 bits.  Deletes the handle and returns true when refused.
static bool f16_switch_refused(hh_net *n)
{
    if (n->dtype != HH_DTYPE_F16 || (!n->sw.no_stem_fused && !n->sw.bb32_tile)) return false;
    hh_set_error(std::string("hh_create: HH_DTYPE_F16 with ") + (n->sw.no_stem_fused ? "HH_NO_STEM_FUSED" : "HH_BB32=tile") +
                 ": that debug switch reaches a kernel that has no fp16 form");
    delete n;
    return true;
}

hh_net *hh_create(int num_kpts, int C, int dtype)
{
    if (dtype != HH_DTYPE_BF16 && dtype != HH_DTYPE_FP8 && dtype != HH_DTYPE_F16) {
        hh_set_error("hh_create: dtype must be HH_DTYPE_BF16 (1), HH_DTYPE_FP8 (2) or HH_DTYPE_F16 (3)");
        return nullptr;
    }
    if (num_kpts <= 0 || num_kpts > 64 || C <= 0 || C % 16) { hh_set_error("hh_create: need 0 < num_kpts <= 64 and C % 16 == 0"); return nullptr; }
    hh_net *n = new hh_net();
    n->K = num_kpts; n->C = C; n->dtype = dtype;
    n->sw = PlanSwitches::from_env();
    if (f16_switch_refused(n)) return nullptr;
    n->build();
    return n;
}
hh_net *hh_create_classifier(int C, int num_classes, int dtype)
{
    if (dtype != HH_DTYPE_BF16 && dtype != HH_DTYPE_F16) { hh_set_error("hh_create_classifier: dtype must be HH_DTYPE_BF16 (1) or HH_DTYPE_F16 (3)"); return nullptr; }
    if (C <= 0 || C % 16 || num_classes <= 0) { hh_set_error("hh_create_classifier: need C % 16 == 0 and num_classes > 0"); return nullptr; }
    hh_net *n = new hh_net();
    n->K = 17; n->C = C; n->dtype = dtype; n->kind = 1; n->num_classes = num_classes;
    n->sw = PlanSwitches::from_env();
    if (f16_switch_refused(n)) return nullptr;
    n->build();
    return n;
}
int hh_forward_classifier(hh_net *net, const float *images, int B, int H, int W, float *logits, void *stream)
{
    if (!net || net->kind != 1) { hh_set_error("hh_forward_classifier: not a classifier handle"); return 1; }
    if (!images || !logits) { hh_set_error("hh_forward_classifier: null buffer"); return 1; }
    if (B <= 0 || H <= 0 || W <= 0 || H % 32 || W % 32) { hh_set_error("hh_forward_classifier: H and W must be positive multiples of 32"); return 1; }
    return net->forward(images, B, H, W, logits, nullptr, 0, (hipStream_t)stream);
}
void hh_destroy(hh_net *net) { delete net; }

int hh_num_params(const hh_net *net) { return (int)net->params.size(); }
const char *hh_param_name(const hh_net *net, int i) { return (i >= 0 && i < (int)net->params.size()) ? net->params[i].name.c_str() : nullptr; }
int hh_param_shape(const hh_net *net, int i, int64_t shape[4])
{
    if (i < 0 || i >= (int)net->params.size()) return -1;
    const auto &s = net->params[i].shape;
    for (size_t d = 0; d < s.size(); ++d) shape[d] = s[d];
    return (int)s.size();
}

int hh_load_weights(hh_net *net, const char *name, const float *host, const int64_t *shape, int ndim)
{
    auto it = net->param_index.find(name);
    if (it == net->param_index.end()) { hh_set_error(std::string("hh_load_weights: unexpected key ") + name); return 1; }
    ParamSlot &p = net->params[it->second];
    if (p.counter) { p.loaded = true; return 0; }
    if (ndim != (int)p.shape.size()) { hh_set_error(std::string("hh_load_weights: rank mismatch for ") + name); return 1; }
    size_t n = 1;
    for (int d = 0; d < ndim; ++d) {
        if (shape[d] != p.shape[d]) { hh_set_error(std::string("hh_load_weights: size mismatch for ") + name); return 1; }
        n *= (size_t)shape[d];
    }
    p.data.assign(host, host + n);
    p.loaded = true;
    net->finalized = false;
    return 0;
}
int hh_e4m3_encode(const float *x, int64_t n, unsigned char *out)
{
    for (int64_t i = 0; i < n; ++i) out[i] = hh_f32_to_e4m3(x[i]);
    return 0;
}
int hh_e4m3_decode(const unsigned char *x, int64_t n, float *out)
{
    for (int64_t i = 0; i < n; ++i) out[i] = hh_e4m3_to_f32(x[i]);
    return 0;
}
int hh_finalize(hh_net *net) { return net->finalize(); }
int hh_calibrate(hh_net *net, const float *images, int B, int H, int W, int rounds, void *stream)
{
    if (!images || B <= 0 || H <= 0 || W <= 0 || H % 32 || W % 32) { hh_set_error("hh_calibrate: need images [B,3,H,W] with H, W multiples of 32"); return 1; }
    return net->calibrate(images, B, H, W, rounds > 0 ? rounds : 2, (hipStream_t)stream);
}
int hh_reserve(hh_net *net, int B, int H, int W) { return net->reserve(B, H, W); }
int64_t hh_workspace_bytes(const hh_net *net) { return net->ws_bytes; }

int hh_forward(hh_net *net, const float *images, int B, int H, int W, float *init_heatmaps, float *deconv_heatmaps,
               int use_graph, void *stream)
{
    if (net->kind != 0) { hh_set_error("hh_forward: classifier handle, use hh_forward_classifier"); return 1; }
    if (!images || !init_heatmaps || !deconv_heatmaps) { hh_set_error("hh_forward: null buffer"); return 1; }
    if (B <= 0 || H <= 0 || W <= 0 || H % 32 || W % 32) { hh_set_error("hh_forward: H and W must be positive multiples of 32"); return 1; }
    return net->forward(images, B, H, W, init_heatmaps, deconv_heatmaps, use_graph, (hipStream_t)stream);
}
double hh_forward_flops(const hh_net *net, int B, int H, int W) { return net->flops(B, H, W); }

int hh_set_multi_lane(hh_net *net, int enable)
{
    net->multi_lane = enable != 0;
    for (auto &g : net->graphs) hipGraphExecDestroy(g.exec);
    net->graphs.clear();
    return 0;
}
int hh_set_taps(hh_net *net, int enable) { net->taps_enabled = enable != 0; return 0; }
int hh_num_taps(const hh_net *net) { return (int)net->taps.size(); }
const char *hh_tap_name(const hh_net *net, int i) { return (i >= 0 && i < (int)net->taps.size()) ? net->taps[i].name.c_str() : nullptr; }
int hh_tap_shape(const hh_net *net, int i, int64_t shape[4])
{
    if (i < 0 || i >= (int)net->taps.size()) return 1;
    const TensorDesc &d = net->tensors[net->taps[i].tensor];
    shape[0] = net->lastB; shape[1] = net->taps[i].C; shape[2] = net->lastH >> d.shift; shape[3] = net->lastW >> d.shift;
    return 0;
}
int hh_tap_read(hh_net *net, int index, float *host_nchw) { return hh_tap_read_impl(net, index, host_nchw); }

int hh_debug_check_plan(const hh_net *net)
{
    std::string why;
    if (net->check_plan(&why)) { hh_set_error("schedule hazard: " + why); return 1; }
    return 0;
}

// The fused stem alone on the handle's packed stem weights: any H, W the kernel accepts, not only the forward's multiples of 32.
int hh_debug_stem_fused(hh_net *net, const float *images, int B, int H, int W, void *out16, void *stream)
{
    if (!net->finalized) { hh_set_error("hh_debug_stem_fused: call hh_finalize first"); return 1; }
    if (!images || !out16 || B <= 0 || H <= 0 || W <= 0) { hh_set_error("hh_debug_stem_fused: null buffer or empty shape"); return 1; }
    for (const Op &op : net->ops) {
        if (op.kind != OP_STEM || op.layer2 < 0) continue;
        const ConvLayer &l = net->layers[op.layer], &l2 = net->layers[op.layer2];
        StemFusedParams q{};
        q.images = images; q.w1 = l.d_w; q.b1 = l.d_bias; q.w2 = l2.d_w; q.b2 = l2.d_bias;
        q.out = (bf16_raw *)out16; q.out_cs = 64;
        q.B = B; q.H = H; q.W = W;
        if (!stem_fused_supported(q)) { hh_set_error("hh_debug_stem_fused: H, W must be multiples of 4 and an image below 2 GB"); return 1; }
        if (net->sw.poison_lds) HH_CHECK_HIP(launch_lds_poison(net->num_cus, (hipStream_t)stream));
        HH_CHECK_HIP(stem_fused_launch(q, net->num_cus, (hipStream_t)stream, net->act()));
        return 0;
    }
    hh_set_error("hh_debug_stem_fused: the handle's plan has no fused stem (HH_NO_STEM_FUSED, or an fp8 handle)");
    return 1;
}

int hh_profile_enable(hh_net *net, int enable) { net->prof_enabled = enable != 0; net->prof_clk = enable == 2; net->prof_used = 0; return 0; }
int hh_profile_count(const hh_net *net) { return (int)net->prof_used; }
int hh_profile_get(hh_net *net, int i, int *cfg, double *flops, double *bytes, float *ms, float *kernel_ms, const char **layer)
{
    if (i < 0 || i >= (int)net->prof_used) { hh_set_error("hh_profile_get: index out of range"); return 1; }
    const ProfRecord &r = net->prof[i];
    HH_CHECK_HIP(hipEventSynchronize(r.e1));
    HH_CHECK_HIP(hipEventElapsedTime(ms, r.e0, r.e1));
    *cfg = r.cfg; *flops = r.flops; *bytes = r.bytes;
    *layer = net->layers[net->ops[r.op].layer].conv.c_str();
    *kernel_ms = -1.f;
    if (r.slot >= 0 && net->prof_clk && net->d_clk && net->clk_khz > 0) {
        unsigned long long t[2];
        HH_CHECK_HIP(hipMemcpy(t, net->d_clk + 4 * r.slot, 16, hipMemcpyDeviceToHost));
        if (t[1] > t[0]) *kernel_ms = (float)((double)(t[1] - t[0]) / net->clk_khz);
    }
    return 0;
}
int hh_profile_clock(hh_net *net, int i, double *ghz)
{
    if (i < 0 || i >= (int)net->prof_used) { hh_set_error("hh_profile_clock: index out of range"); return 1; }
    const ProfRecord &r = net->prof[i];
    *ghz = 0.0;
    if (r.slot >= 0 && net->prof_clk && net->d_clk && net->clk_khz > 0) {
        unsigned long long t[2];
        HH_CHECK_HIP(hipEventSynchronize(r.e1));
        HH_CHECK_HIP(hipMemcpy(t, net->d_clk + 4 * r.slot + 2, 16, hipMemcpyDeviceToHost));
        if (t[1]) *ghz = (double)t[0] / (double)t[1] * net->clk_khz * 1e-6;  // core cycles per wall tick x wall ticks per second
    }
    return 0;
}
int hh_conv_config(int cfg, int out[7])
{
    if (cfg >= 1000 && cfg - 1000 < conv_fp8_num_configs()) {  // fp8 instantiations are reported as 1000 + index
        const Fp8ConvConfig &c = conv_fp8_config(cfg - 1000);
        out[0] = c.KS; out[1] = c.S; out[2] = c.KC; out[3] = c.NT; out[4] = 1; out[5] = c.PT; out[6] = c.TW;
        return 0;
    }
    if (cfg < 0 || cfg >= conv_num_configs()) return 1;
    const ConvConfig &c = conv_config(cfg);
    out[0] = c.KS; out[1] = c.S; out[2] = c.KC; out[3] = c.NT; out[4] = c.WC; out[5] = c.PT; out[6] = c.TW;
    return 0;
}

int hh_conv_config_double_buffered(int cfg)
{
    if (cfg >= 1000 && cfg - 1000 < conv_fp8_num_configs()) return 0;
    if (cfg < 0 || cfg >= conv_num_configs()) return -1;
    return conv_config(cfg).DB;
}

int hh_preprocess_u8(const unsigned char *image_hwc, int h, int w, const double dst_to_src[6], float *out_nchw, int H, int W,
                     const float mean[3], const float stdv[3], void *stream)
{
    if (!image_hwc || !out_nchw || h <= 0 || w <= 0 || H <= 0 || W <= 0) { hh_set_error("hh_preprocess_u8: bad argument"); return 1; }
    HH_CHECK_HIP(launch_preprocess(image_hwc, h, w, dst_to_src, out_nchw, H, W, mean, stdv, (hipStream_t)stream));
    return 0;
}

int hh_preprocess_u8_batch(const unsigned char *images_base, const hh_image_desc *descs_dev, int n, float *out_nchw, int H, int W,
                           const float mean[3], const float stdv[3], void *stream)
{
    if (!images_base || !descs_dev || !out_nchw || n <= 0 || n > 65535 || H <= 0 || W <= 0) { hh_set_error("hh_preprocess_u8_batch: bad argument"); return 1; }
    HH_CHECK_HIP(launch_preprocess_batch(images_base, descs_dev, n, out_nchw, H, W, mean, stdv,
                                         (hipStream_t)stream));
    return 0;
}

int hh_train_images_u8_batch(const unsigned char *batch_base, const hh_train_desc *descs_dev, int n, float *out_nchw, int H, int W,
                             const float mean[3], const float stdv[3], void *stream)
{
    if (!batch_base || !descs_dev || !out_nchw || !mean || !stdv) { hh_set_error("hh_train_images_u8_batch: null pointer"); return 1; }
    if (n <= 0 || n > 65535 || H <= 0 || W <= 0 || (int64_t)H * W > (1 << 30)) { hh_set_error("hh_train_images_u8_batch: need 0 < n <= 65535 and 0 < H * W <= 2^30"); return 1; }
    HH_CHECK_HIP(launch_train_images(batch_base, descs_dev, n, out_nchw, H, W, mean, stdv, (hipStream_t)stream));
    return 0;
}

int hh_train_masks_u8_batch(const unsigned char *batch_base, const hh_train_desc *descs_dev, int n, int nstages, const int *stage_hw,
                            float *const *out, void *stream)
{
    if (!batch_base || !descs_dev || !stage_hw || !out) { hh_set_error("hh_train_masks_u8_batch: null pointer"); return 1; }
    if (n <= 0 || n > 65535) { hh_set_error("hh_train_masks_u8_batch: need 0 < n <= 65535"); return 1; }
    if (nstages <= 0 || nstages > HH_TRAIN_MAX_STAGES) { hh_set_error("hh_train_masks_u8_batch: 1..HH_TRAIN_MAX_STAGES (4) stages"); return 1; }
    TrainMaskStages st = {};
    st.n = nstages;
    int64_t total = 0;
    for (int k = 0; k < nstages; ++k) {
        if (!out[k]) { hh_set_error("hh_train_masks_u8_batch: null output pointer in the table"); return 1; }
        if (stage_hw[2 * k] <= 0 || stage_hw[2 * k + 1] <= 0) { hh_set_error("hh_train_masks_u8_batch: stage sizes must be positive"); return 1; }
        st.out[k] = out[k], st.h[k] = stage_hw[2 * k], st.w[k] = stage_hw[2 * k + 1];
        total += (int64_t)st.h[k] * st.w[k];
    }
    if (total > (1 << 30)) { hh_set_error("hh_train_masks_u8_batch: the stages' pixel count exceeds 2^30"); return 1; }
    HH_CHECK_HIP(launch_train_masks(batch_base, descs_dev, n, st, (hipStream_t)stream));
    return 0;
}

int hh_resized_crop_u8_batch(const unsigned char *batch_base, const hh_crop_desc *descs_dev, const hh_crop_desc *descs_host, int n, float *out_nchw,
                             int H, int W, const float mean[3], const float stdv[3], void *stream)
{
    const char *fn = "hh_resized_crop_u8_batch";
    if (!batch_base || !descs_dev || !descs_host || !out_nchw || !mean || !stdv) { hh_set_error(std::string(fn) + ": null pointer"); return 1; }
    if (n <= 0 || n > 65535 || H <= 0 || W <= 0 || H > HH_CROP_MAX_EXTENT || W > HH_CROP_MAX_EXTENT || (int64_t)H * W > (1 << 30)) {
        hh_set_error(std::string(fn) + ": need 0 < n <= 65535, 0 < H, W <= 32768 and H * W <= 2^30");
        return 1;
    }
    for (int c = 0; c < 3; ++c)
        if (!(stdv[c] != 0.f)) { hh_set_error(std::string(fn) + ": std must not be zero"); return 1; }
    for (int b = 0; b < n; ++b) {
        const hh_crop_desc &d = descs_host[b];
        const std::string who = std::string(fn) + ": sample " + std::to_string(b) + ": ";
        if (d.h <= 0 || d.w <= 0 || d.ch <= 0 || d.cw <= 0 || d.rh <= 0 || d.rw <= 0) { hh_set_error(who + "non-positive extent (image, crop or virtual size)"); return 1; }
        if (d.image_offset < 0) { hh_set_error(who + "negative image offset"); return 1; }
        // the kernel indexes the bytes of one image with 32-bit integers and forms tap positions in fp32
        if ((int64_t)d.h * d.w * 3 > INT32_MAX) { hh_set_error(who + "image beyond 32-bit byte indexing (h * w * 3 >= 2^31)"); return 1; }
        if (d.h > HH_CROP_MAX_SIDE || d.w > HH_CROP_MAX_SIDE || d.rh > HH_CROP_MAX_SIDE || d.rw > HH_CROP_MAX_SIDE) { hh_set_error(who + "a side exceeds 2^23 pixels"); return 1; }
        if (d.top < 0 || d.left < 0 || (int64_t)d.top + d.ch > d.h || (int64_t)d.left + d.cw > d.w) { hh_set_error(who + "crop rectangle outside its image"); return 1; }
        if (d.oy < 0 || d.ox < 0 || (int64_t)d.oy + H > d.rh || (int64_t)d.ox + W > d.rw) { hh_set_error(who + "output window outside the virtual resized crop"); return 1; }
    }
    HH_CHECK_HIP(launch_resized_crop(batch_base, descs_dev, n, out_nchw, H, W, mean, stdv, (hipStream_t)stream));
    return 0;
}

int hh_mosaic_u8_batch(unsigned char *batch_base, const hh_mosaic_desc *descs_dev, const hh_mosaic_desc *descs_host, int n, int S, void *stream)
{
    const char *fn = "hh_mosaic_u8_batch";
    if (!batch_base || !descs_dev || !descs_host) { hh_set_error(std::string(fn) + ": null pointer"); return 1; }
    if (n <= 0 || n > 65535) { hh_set_error(std::string(fn) + ": need 0 < n <= 65535"); return 1; }
    if (S < 4 || S > HH_MOSAIC_MAX_S || S % 4) { hh_set_error(std::string(fn) + ": S must be a multiple of 4 in 4..8192"); return 1; }
    if ((uintptr_t)batch_base % 4) { hh_set_error(std::string(fn) + ": batch_base must be 4-byte aligned"); return 1; }
    for (int b = 0; b < n; ++b) {
        const hh_mosaic_desc &d = descs_host[b];
        const std::string who = std::string(fn) + ": sample " + std::to_string(b) + ": ";
        if (d.canvas_image_offset < 0 || d.canvas_mask_offset < 0) { hh_set_error(who + "negative canvas offset"); return 1; }
        if (d.canvas_image_offset % 4 || d.canvas_mask_offset % 4) { hh_set_error(who + "canvas offsets must be multiples of 4"); return 1; }
        for (int t = 0; t < 4; ++t) {
            const hh_mosaic_tile &q = d.tile[t];
            const std::string tile = who + "tile " + std::to_string(t) + ": ";
            if (q.h < 1 || q.w < 1) { hh_set_error(tile + "non-positive extent"); return 1; }
            if ((int64_t)q.h * q.w * 3 > INT32_MAX) { hh_set_error(tile + "beyond 32-bit byte indexing (h * w * 3 >= 2^31)"); return 1; }
            if (q.image_offset < 0 || q.mask_offset < 0) { hh_set_error(tile + "negative offset"); return 1; }
        }
    }
    HH_CHECK_HIP(launch_mosaic(batch_base, descs_dev, n, S, (hipStream_t)stream));
    return 0;
}

int hh_render_config(int out[4])
{
    if (!out) { hh_set_error("hh_render_config: null pointer"); return 1; }
    out[0] = RENDER_TH, out[1] = RENDER_TW, out[2] = RENDER_CHUNK, out[3] = RENDER_PX;
    return 0;
}

// The checks of a render call that need no device: every frame's descriptor and its primitives, on the caller's host copy.
static int render_check(const char *fn, const hh_render_desc *descs_host, const hh_render_prim *prims_host, int num_prims, int n, int *max_tiles)
{
    return draw_check_frames(fn, descs_host, n, num_prims < 0 ? "negative table length" : nullptr, !prims_host, RENDER_TH, RENDER_TW, max_tiles,
                             [&](const RenderDesc &d) { return render_check_frame(d, prims_host, num_prims, HH_RENDER_MAX_PRIMS); });
}

int hh_render_poses_u8_batch(unsigned char *batch_base, const hh_render_desc *descs_dev, const hh_render_desc *descs_host,
                             const hh_render_prim *prims_dev, const hh_render_prim *prims_host, int num_prims, int n, void *stream)
{
    const char *fn = "hh_render_poses_u8_batch";
    if (!batch_base || !descs_dev || !descs_host || (num_prims > 0 && (!prims_dev || !prims_host))) { hh_set_error(std::string(fn) + ": null pointer"); return 1; }
    if ((uintptr_t)descs_dev % 8 || (uintptr_t)prims_dev % 4) { hh_set_error(std::string(fn) + ": descs_dev must be 8-byte and prims_dev 4-byte aligned"); return 1; }
    int max_tiles = 0;
    if (render_check(fn, descs_host, prims_host, num_prims, n, &max_tiles)) return 1;
    HH_CHECK_HIP(launch_render_poses(batch_base, descs_dev, prims_dev, n,
                                     max_tiles, (hipStream_t)stream));
    return 0;
}

int hh_debug_render_host(const unsigned char *src, unsigned char *dst, const hh_render_desc *desc, const hh_render_prim *prims, int num_prims)
{
    const char *fn = "hh_debug_render_host";
    if (!src || !dst || !desc) { hh_set_error(std::string(fn) + ": null pointer"); return 1; }
    int max_tiles = 0;
    if (render_check(fn, desc, prims, num_prims, 1, &max_tiles)) return 1;
    RenderDesc d = *desc;  // src and dst are the frame's own buffers here
    d.src_offset = d.dst_offset = 0;
    render_debug_host(src, dst, d, prims);
    return 0;
}

int hh_text_config(int out[4])
{
    if (!out) { hh_set_error("hh_text_config: null pointer"); return 1; }
    out[0] = TEXT_TH, out[1] = TEXT_TW, out[2] = TEXT_CHUNK, out[3] = TEXT_PX;
    return 0;
}

// The checks of a text call that need no device: every frame's descriptor and its primitives, on the caller's host copy.
static int text_check(const char *fn, const hh_text_desc *descs_host, const hh_text_prim *prims_host, int num_prims, int n, long long atlas_len)
{
    return draw_check_frames(fn, descs_host, n, num_prims < 0 || atlas_len < 0 ? "negative table or atlas length" : nullptr, !prims_host, TEXT_TH, TEXT_TW,
                             nullptr, [&](const TextDesc &d) { return text_check_frame(d, prims_host, num_prims, atlas_len); });
}

int hh_text_tiles(const hh_text_desc *descs_host, const hh_text_prim *prims_host, int num_prims, int n, long long atlas_len, int32_t *tiles_host,
                  long long capacity, long long *count)
{
    const char *fn = "hh_text_tiles";
    if (!descs_host || !count || (capacity > 0 && !tiles_host) || (num_prims > 0 && !prims_host)) { hh_set_error(std::string(fn) + ": null pointer"); return 1; }
    if (capacity < 0) { hh_set_error(std::string(fn) + ": negative capacity"); return 1; }
    if (text_check(fn, descs_host, prims_host, num_prims, n, atlas_len)) return 1;
    std::vector<uint8_t> seen;
    long long total = 0;
    for (int b = 0; b < n; ++b) {
        const TextDesc &d = descs_host[b];
        seen.resize((size_t)text_xtiles(d.w) * text_ytiles(d.h));
        const long long room = capacity > total ? capacity - total : 0;
        total += text_list_tiles(d, prims_host, b, seen.data(), reinterpret_cast<TextTile *>(tiles_host) + (room ? total : 0), room);
    }
    *count = total;
    return 0;
}

// A tile list names tiles of its frames, each at most once (two workgroups on one tile would both read and write it): strictly ascending.
static int text_check_tiles(const char *fn, const hh_text_desc *descs_host, int n, const int32_t *tiles_host, long long num_tiles)
{
    const TextTile *t = reinterpret_cast<const TextTile *>(tiles_host);
    for (long long i = 0; i < num_tiles; ++i) {
        if (t[i].frame < 0 || t[i].frame >= n || t[i].tile < 0 || t[i].tile >= text_xtiles(descs_host[t[i].frame].w) * text_ytiles(descs_host[t[i].frame].h)) {
            hh_set_error(std::string(fn) + ": tile " + std::to_string(i) + " names no tile of its frame");
            return 1;
        }
        if (i && (t[i].frame < t[i - 1].frame || (t[i].frame == t[i - 1].frame && t[i].tile <= t[i - 1].tile))) {
            hh_set_error(std::string(fn) + ": the tile list must ascend strictly");
            return 1;
        }
    }
    return 0;
}

// Everything a text call checks on the host copies.
static int text_check_call(const char *fn, const hh_text_desc *descs_host, const hh_text_prim *prims_host, int num_prims, int n, long long atlas_len,
                           const int32_t *tiles_host, long long num_tiles)
{
    if (!descs_host || (num_prims > 0 && !prims_host) || (num_tiles > 0 && !tiles_host)) { hh_set_error(std::string(fn) + ": null pointer"); return 1; }
    if (num_tiles < 0 || num_tiles > INT32_MAX) { hh_set_error(std::string(fn) + ": need 0 <= num_tiles < 2^31"); return 1; }
    return text_check(fn, descs_host, prims_host, num_prims, n, atlas_len) || text_check_tiles(fn, descs_host, n, tiles_host, num_tiles);
}

int hh_text_check(const hh_text_desc *descs_host, const hh_text_prim *prims_host, int num_prims, int n, long long atlas_len, const int32_t *tiles_host,
                  long long num_tiles)
{
    return text_check_call("hh_text_check", descs_host, prims_host, num_prims, n, atlas_len, tiles_host, num_tiles);
}

int hh_text_labels_u8_batch(unsigned char *batch_base, const hh_text_desc *descs_dev, const hh_text_desc *descs_host, const hh_text_prim *prims_dev,
                            const hh_text_prim *prims_host, int num_prims, int n, const unsigned char *atlas_dev, long long atlas_len,
                            const int32_t *tiles_dev, const int32_t *tiles_host, long long num_tiles, void *stream)
{
    const char *fn = "hh_text_labels_u8_batch";
    if (!batch_base || !descs_dev || !descs_host || !atlas_dev || (num_prims > 0 && (!prims_dev || !prims_host)) || (num_tiles > 0 && (!tiles_dev || !tiles_host))) {
        hh_set_error(std::string(fn) + ": null pointer");
        return 1;
    }
    if ((uintptr_t)descs_dev % 8 || (uintptr_t)prims_dev % 4 || (uintptr_t)tiles_dev % 4) {
        hh_set_error(std::string(fn) + ": descs_dev must be 8-byte, prims_dev and tiles_dev 4-byte aligned");
        return 1;
    }
    if (text_check_call(fn, descs_host, prims_host, num_prims, n, atlas_len, tiles_host, num_tiles)) return 1;
    if (num_tiles == 0) return 0;
    HH_CHECK_HIP(launch_text_labels(batch_base, descs_dev, prims_dev, atlas_dev, tiles_dev, num_tiles, (hipStream_t)stream));
    return 0;
}

int hh_debug_text_host(unsigned char *frame, const hh_text_desc *desc, const hh_text_prim *prims, int num_prims, const unsigned char *atlas,
                       long long atlas_len)
{
    const char *fn = "hh_debug_text_host";
    if (!frame || !desc || !atlas) { hh_set_error(std::string(fn) + ": null pointer"); return 1; }
    if (text_check(fn, desc, prims, num_prims, 1, atlas_len)) return 1;
    TextDesc d = *desc;  // frame is the frame's own buffer here
    d.src_offset = d.dst_offset = 0;
    std::vector<uint8_t> seen((size_t)text_xtiles(d.w) * text_ytiles(d.h));
    std::vector<TextTile> tiles(seen.size());
    const long long nt = text_list_tiles(d, prims, 0, seen.data(), tiles.data(), (long long)tiles.size());
    text_debug_host(frame, d, prims, atlas, tiles.data(), nt);
    return 0;
}

// Segmentation overlays (seg_overlay.hip, seg_overlay_math.h).
int hh_seg_overlay_config(int out[4])
{
    if (!out) { hh_set_error("hh_seg_overlay_config: null pointer"); return 1; }
    out[0] = SEG_TH, out[1] = SEG_TW, out[2] = SEG_THREADS, out[3] = SEG_CHUNK;
    return 0;
}

// The checks of an overlay call that need no device: every frame's descriptor, its shape rows and their toggles, on the caller's host copies.
static int seg_check(const char *fn, const hh_seg_desc *descs_host, const int32_t *shapes_host, int num_shapes, const unsigned int *toggles_host,
                     long long num_toggles, int n, int *max_tiles)
{
    const bool null = !descs_host || (num_shapes > 0 && !shapes_host) || (num_toggles > 0 && !toggles_host);
    const char *call_why = num_shapes < 0 || num_toggles < 0 ? "negative table length" : null ? "null pointer" : nullptr;
    return draw_check_frames(fn, descs_host, n, call_why, false, SEG_TH, SEG_TW, max_tiles, [&](const SegDesc &d) {
        return seg_check_frame(d, reinterpret_cast<const SegShape *>(shapes_host), num_shapes, toggles_host, num_toggles);
    });
}

int hh_seg_overlay_u8_batch(unsigned char *batch_base, const hh_seg_desc *descs_dev, const hh_seg_desc *descs_host, const int32_t *shapes_dev,
                            const int32_t *shapes_host, int num_shapes, const unsigned int *toggles_dev, const unsigned int *toggles_host,
                            long long num_toggles, int n, void *stream)
{
    const char *fn = "hh_seg_overlay_u8_batch";
    if (!batch_base || !descs_dev || !descs_host || (num_shapes > 0 && !shapes_dev) || (num_toggles > 0 && !toggles_dev)) {
        hh_set_error(std::string(fn) + ": null pointer");
        return 1;
    }
    if ((uintptr_t)descs_dev % 8 || (uintptr_t)shapes_dev % 4 || (uintptr_t)toggles_dev % 4) {
        hh_set_error(std::string(fn) + ": descs_dev must be 8-byte, shapes_dev and toggles_dev 4-byte aligned");
        return 1;
    }
    int max_tiles = 0;
    if (seg_check(fn, descs_host, shapes_host, num_shapes, toggles_host, num_toggles, n, &max_tiles)) return 1;
    HH_CHECK_HIP(launch_seg_overlay(batch_base, descs_dev, shapes_dev, toggles_dev, n, max_tiles, (hipStream_t)stream));
    return 0;
}

int hh_debug_seg_overlay_host(const unsigned char *src, unsigned char *dst, const hh_seg_desc *desc, const int32_t *shapes, int num_shapes,
                              const unsigned int *toggles, long long num_toggles)
{
    const char *fn = "hh_debug_seg_overlay_host";
    if (!src || !dst) { hh_set_error(std::string(fn) + ": null pointer"); return 1; }
    int max_tiles = 0;
    if (seg_check(fn, desc, shapes, num_shapes, toggles, num_toggles, 1, &max_tiles)) return 1;
    const long long bytes = (long long)desc->h * desc->w * 3;
    if (src != dst && src < dst + bytes && dst < src + bytes) { hh_set_error(std::string(fn) + ": dst partially overlaps src"); return 1; }
    seg_frame_host(src, dst, *desc, reinterpret_cast<const SegShape *>(shapes), toggles);
    return 0;
}

// Baseline JPEG (jpeg.hip, jpeg_math.h).
static const char *jpeg_check_sub(int h, int w, int subsampling)
{
    if (h < 1 || w < 1 || h > 65535 || w > 65535) return "h and w must lie in 1..65535";
    if (subsampling != 420 && subsampling != 444) return "subsampling must be 420 or 444";
    return nullptr;
}

long long hh_jpeg_bound(int h, int w, int subsampling)
{
    const char *why = jpeg_check_sub(h, w, subsampling);
    if (why) { hh_set_error(std::string("hh_jpeg_bound: ") + why); return -1; }
    return jpeg_bound(jpeg_geom(h, w, subsampling));
}

long long hh_jpeg_workspace_bytes(int h, int w, int subsampling)
{
    const char *why = jpeg_check_sub(h, w, subsampling);
    if (why) { hh_set_error(std::string("hh_jpeg_workspace_bytes: ") + why); return -1; }
    return jpeg_geom(h, w, subsampling).ws_bytes;
}

int hh_jpeg_quant_tables(int quality, int32_t out[128])
{
    if (!out) { hh_set_error("hh_jpeg_quant_tables: null pointer"); return 1; }
    if (quality < 1 || quality > 100) { hh_set_error("hh_jpeg_quant_tables: quality outside 1..100"); return 1; }
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k) out[t * 64 + k] = jpeg_quant(quality, t, k);
    return 0;
}

int hh_jpeg_config(int out[4])
{
    if (!out) { hh_set_error("hh_jpeg_config: null pointer"); return 1; }
    out[0] = JPEG_ENT_LANES, out[1] = JPEG_BLOCK_BITS, out[2] = JPEG_HEADER_BYTES, out[3] = JPEG_MCUS_PER_GROUP;
    return 0;
}

int hh_jpeg_encode_u8_batch(unsigned char *batch_base, const hh_jpeg_desc *descs_dev, const hh_jpeg_desc *descs_host, int n,
                            unsigned char *workspace, long long workspace_bytes, int32_t *lengths_dev, void *stream)
{
    const std::string fn = "hh_jpeg_encode_u8_batch";
    if (!batch_base || !descs_dev || !descs_host || !workspace || !lengths_dev) { hh_set_error(fn + ": null pointer"); return 1; }
    if (n <= 0 || n > 65535) { hh_set_error(fn + ": need 0 < n <= 65535"); return 1; }
    if ((uintptr_t)descs_dev % 8 || (uintptr_t)workspace % 16 || (uintptr_t)lengths_dev % 4) {
        hh_set_error(fn + ": descs_dev must be 8-byte, workspace 16-byte and lengths_dev 4-byte aligned");
        return 1;
    }
    int max_mcus = 1, max_rows = 1;
    for (int b = 0; b < n; ++b) {
        const JpegDesc &d = descs_host[b];
        const char *why = jpeg_check_desc(d);
        if (why) { hh_set_error(fn + ": frame " + std::to_string(b) + ": " + why); return 1; }
        const JpegGeom g = jpeg_geom(d.h, d.w, d.subsampling);
        if (d.ws_offset + g.ws_bytes > workspace_bytes) { hh_set_error(fn + ": frame " + std::to_string(b) + ": workspace below hh_jpeg_workspace_bytes"); return 1; }
        max_mcus = std::max(max_mcus, g.mrows * g.mcols);
        max_rows = std::max(max_rows, g.mrows);
    }
    HH_CHECK_HIP(launch_jpeg_encode(batch_base, descs_dev, n, max_mcus, max_rows, workspace, lengths_dev,
                                    (hipStream_t)stream));
    return 0;
}

int hh_debug_jpeg_encode_host(const unsigned char *src, const hh_jpeg_desc *desc, unsigned char *out, long long *length)
{
    const std::string fn = "hh_debug_jpeg_encode_host";
    if (!src || !desc || !out || !length) { hh_set_error(fn + ": null pointer"); return 1; }
    const JpegDesc &d = *desc;
    const char *why = jpeg_check_desc(d);
    if (why) { hh_set_error(fn + ": " + why); return 1; }
    std::vector<JpegVec8> work((size_t)jpeg_geom(d.h, d.w, d.subsampling).nblk * 8);
    *length = jpeg_encode_host(src, d, out, work[0].v);
    return 0;
}

int hh_debug_jpeg_fdct(const int32_t samples[64], int32_t rows_out[64], int32_t cols_out[64])
{
    if (!samples || !rows_out || !cols_out) { hh_set_error("hh_debug_jpeg_fdct: null pointer"); return 1; }
    long long sum = 0;  // sum |s| <= 8192 (what a block of samples has at most) keeps |F| <= 8035 * (8035 * 8192 / 2048 + 8) < 2^31
    for (int i = 0; i < 64; ++i) sum += samples[i] < 0 ? -(long long)samples[i] : samples[i];
    if (sum > 8192) { hh_set_error("hh_debug_jpeg_fdct: the samples' absolute sum exceeds 8192"); return 1; }
    memcpy(rows_out, samples, 64 * sizeof(int32_t));
    for (int y = 0; y < 8; ++y) jpeg_fdct_row(rows_out + y * 8);
    for (int u = 0; u < 8; ++u) {
        int32_t F[8];
        jpeg_fdct_col(rows_out, u, F);
        for (int v = 0; v < 8; ++v) cols_out[v * 8 + u] = F[v];
    }
    return 0;
}

// Baseline JPEG decode (jpeg_decode.hip, jpeg_dec_math.h).
static const char *const JPEG_STATUS_NAME[6] = {"ok", "bad Huffman code", "zero run past coefficient 63", "bytes exhausted",
                                                "missing or unexpected RSTm", "bad segment"};

// What the kernels trust of a stream's info; nullptr if it is what hh_jpeg_parse can have written.
// rebased: the info of a window decode's table block, whose scan is the shipped slice (scan_offset 0).
static const char *jpeg_dec_check_info(const JpegStreamInfo &I, bool rebased = false)
{
    if (I.h < 1 || I.w < 1 || I.h > 65535 || I.w > 65535) return "bad stream info: h and w must lie in 1..65535";
    const bool grey = I.ncomp == 1 && I.hs == 1 && I.vs == 1 && I.bpm == 1;
    const bool colour = I.ncomp == 3 && (I.hs == 1 || I.hs == 2) && (I.vs == 1 || I.vs == I.hs) && I.bpm == I.hs * I.vs + 2;
    if (!grey && !colour) return "bad stream info: components or sampling";
    if (I.mcols != (I.w + 8 * I.hs - 1) / (8 * I.hs) || I.mrows != (I.h + 8 * I.vs - 1) / (8 * I.vs)) return "bad stream info: the MCU grid";
    if ((long long)I.mcols * I.hs * 8 * 3 * ((long long)I.mrows * I.vs * 8) > INT32_MAX || (long long)I.mcols * I.mrows * I.bpm * 128 > INT32_MAX)
        return "dimensions beyond what int32 offsets allow";
    for (int c = 0; c < 3; ++c)
        if ((I.qt[c] | I.dc[c] | I.ac[c]) & ~3) return "bad stream info: a table id outside 0..3";
    if (I.scan_offset < (rebased ? 0 : 2) || I.scan_end < I.scan_offset || I.scan_end > INT32_MAX) return "bad stream info: the scan's bytes";
    return nullptr;
}

int hh_jpeg_parse(const unsigned char *bytes, long long len, hh_jpeg_stream_info *info)
{
    if (!bytes || !info) { hh_set_error("hh_jpeg_parse: null pointer"); return 1; }
    const char *why = jpeg_dec_parse(bytes, len, info, nullptr);
    if (why) { hh_set_error(std::string("hh_jpeg_parse: ") + why); return 1; }
    return 0;
}

int hh_jpeg_restart_segments(const unsigned char *bytes, long long len, hh_jpeg_segment *entries, int capacity, int *n)
{
    const std::string fn = "hh_jpeg_restart_segments";
    if (!bytes || !entries || !n) { hh_set_error(fn + ": null pointer"); return 1; }
    JpegStreamInfo I;
    const char *why = jpeg_dec_parse(bytes, len, &I, nullptr);
    if (!why && !I.restart_interval) why = "the stream has no restart interval (use hh_jpeg_index_host)";
    if (!why && capacity < I.nseg_restart) why = "capacity below the number of segments";
    if (!why) why = jpeg_dec_restart_segments(bytes, I, entries);
    if (why) { hh_set_error(fn + ": " + why); return 1; }
    *n = I.nseg_restart;
    return 0;
}

int hh_jpeg_index_host(const unsigned char *bytes, long long len, int mcus_per_segment, hh_jpeg_segment *entries, int capacity, int *n)
{
    const std::string fn = "hh_jpeg_index_host";
    if (!bytes || !entries || !n) { hh_set_error(fn + ": null pointer"); return 1; }
    JpegStreamInfo I;
    std::vector<JpegDecTables> T(1);
    const char *why = jpeg_dec_parse(bytes, len, &I, &T[0]);
    int status = 0;
    if (!why) why = jpeg_dec_index(bytes, len, I, T[0], mcus_per_segment > 0 ? mcus_per_segment : I.mcols, entries, capacity, n, &status);
    if (why) { hh_set_error(fn + ": " + why + (status ? std::string(": ") + JPEG_STATUS_NAME[status] : std::string())); return 1; }
    return 0;
}

long long hh_jpeg_decode_workspace_bytes(const hh_jpeg_stream_info *info)
{
    const char *why = info ? jpeg_dec_check_info(*info) : "null pointer";
    if (why) { hh_set_error(std::string("hh_jpeg_decode_workspace_bytes: ") + why); return -1; }
    const JpegStreamInfo &I = *info;
    return jpeg_dec_geom(I, jpeg_full_rect(I)).ws_bytes;
}

long long hh_jpeg_decode_tables_bytes(const hh_jpeg_stream_info *info, int nseg)
{
    const char *why = info ? jpeg_dec_check_info(*info) : "null pointer";
    if (!why && nseg < 1) why = "nseg must be at least 1";
    if (why) { hh_set_error(std::string("hh_jpeg_decode_tables_bytes: ") + why); return -1; }
    return jpeg_dec_tables_bytes(nseg);
}

int hh_jpeg_decode_tables(const unsigned char *bytes, long long len, const hh_jpeg_segment *entries, int nseg, unsigned char *out, long long out_bytes)
{
    const std::string fn = "hh_jpeg_decode_tables";
    if (!bytes || !entries || !out) { hh_set_error(fn + ": null pointer"); return 1; }
    if (nseg < 1 || out_bytes < jpeg_dec_tables_bytes(nseg)) { hh_set_error(fn + ": room below hh_jpeg_decode_tables_bytes"); return 1; }
    JpegStreamInfo I;
    std::vector<JpegDecTables> T(1);
    const char *why = jpeg_dec_parse(bytes, len, &I, &T[0]);
    if (why) { hh_set_error(fn + ": " + why); return 1; }
    memcpy(out, &I, sizeof(I));
    memcpy(out + JPEG_DEC_TABLES_AT, &T[0], sizeof(JpegDecTables));
    memcpy(out + JPEG_DEC_SEGS_AT, entries, (size_t)nseg * sizeof(JpegSegment));
    return 0;
}

// One image of a batch call, `win`: its window (hh_jpeg_decode_window_u8_batch, whose info is rebased to the shipped slice:
// hh_jpeg_decode_window_tables) or null (hh_jpeg_decode_u8_batch: the whole image) -> the refusal or nullptr, and the geometry.
static const char *jpeg_dec_check_image(const unsigned char *batch_base, const JpegDecDesc &d, const JpegStreamInfo &I, const JpegWindow *win,
                                        long long workspace_bytes, JpegDecGeom *g)
{
    const char *why = jpeg_dec_check_info(I, win != nullptr);
    if (!why && win) why = jpeg_win_check(I, *win);
    if (!why && (d.stream_offset < 0 || d.tables_offset < 0 || d.dst_offset < 0 || d.ws_offset < 0)) why = "negative offset";
    if (!why && d.pitch < 3ll * (win ? win->width : I.w)) why = win ? "pitch below 3 * width" : "pitch below 3 * w";
    if (!why && (d.flags & ~1)) why = "unknown flag";
    if (!why && d.nseg < 1) why = win ? "no selected segment (nseg must be at least 1)" : "nseg must be at least 1";
    if (!why && (d.stream_length < 1 || I.scan_end > d.stream_length))
        why = win ? "the scan's bytes lie outside the slice's length" : "the scan's bytes lie outside the stream's length";
    if (!why && d.tables_bytes < jpeg_dec_tables_bytes(d.nseg)) why = "table block below hh_jpeg_decode_tables_bytes";
    if (!why && ((uintptr_t)(batch_base + d.tables_offset) % 16 || d.ws_offset % 16)) why = "the table block and ws_offset must be 16-byte aligned";
    if (why) return why;
    *g = jpeg_dec_geom(I, jpeg_win_rect(I, win ? *win : jpeg_full_window(I)));
    if (d.ws_offset + g->ws_bytes > workspace_bytes) return win ? "workspace below hh_jpeg_decode_window_workspace_bytes" : "workspace below hh_jpeg_decode_workspace_bytes";
    return nullptr;
}

// Both batch entries.  windowed: the descriptors are JpegWinDesc (a JpegDecDesc, then the window), else JpegDecDesc.
static int jpeg_decode_batch(const std::string &fn, bool windowed, unsigned char *batch_base, const void *descs_dev, const void *descs_host,
                             const hh_jpeg_stream_info *infos_host, int n, unsigned char *workspace, long long workspace_bytes, int32_t *status_dev,
                             void *stream)
{
    if (!batch_base || !descs_dev || !descs_host || !infos_host || !workspace || !status_dev) { hh_set_error(fn + ": null pointer"); return 1; }
    if (n < 1 || n > 65535) { hh_set_error(fn + ": need 1 <= n <= 65535"); return 1; }
    if ((uintptr_t)descs_dev % 8 || (uintptr_t)workspace % 16 || (uintptr_t)status_dev % 4) {
        hh_set_error(fn + ": descs_dev must be 8-byte, workspace 16-byte and status_dev 4-byte aligned");
        return 1;
    }
    int max_seg = 1, max_blk = 1, max_h = 1, max_w = 1;
    for (int b = 0; b < n; ++b) {
        const JpegWinDesc *wd = windowed ? static_cast<const JpegWinDesc *>(descs_host) + b : nullptr;
        const JpegDecDesc &d = wd ? wd->d : static_cast<const JpegDecDesc *>(descs_host)[b];
        const JpegStreamInfo &I = infos_host[b];
        const JpegWindow *win = wd ? &wd->window : nullptr;
        JpegDecGeom g;
        const char *why = jpeg_dec_check_image(batch_base, d, I, win, workspace_bytes, &g);
        if (why) { hh_set_error(fn + ": image " + std::to_string(b) + ": " + why); return 1; }
        max_seg = std::max(max_seg, d.nseg), max_blk = std::max(max_blk, g.nblk);
        max_h = std::max(max_h, win ? win->height : I.h), max_w = std::max(max_w, win ? win->width : I.w);
    }
    HH_CHECK_HIP(hipMemsetAsync(status_dev, 0, (size_t)n * 4, (hipStream_t)stream));
    HH_CHECK_HIP(windowed ? launch_jpeg_decode(batch_base, static_cast<const JpegWinDesc *>(descs_dev), n, max_seg, max_blk, max_h, max_w, workspace, status_dev,
                                               (hipStream_t)stream)
                          : launch_jpeg_decode(batch_base, static_cast<const JpegDecDesc *>(descs_dev), n, max_seg, max_blk, max_h, max_w, workspace, status_dev,
                                               (hipStream_t)stream));
    return 0;
}

int hh_jpeg_decode_u8_batch(unsigned char *batch_base, const hh_jpeg_dec_desc *descs_dev, const hh_jpeg_dec_desc *descs_host,
                            const hh_jpeg_stream_info *infos_host, int n, unsigned char *workspace, long long workspace_bytes, int32_t *status_dev,
                            void *stream)
{
    return jpeg_decode_batch("hh_jpeg_decode_u8_batch", false, batch_base, descs_dev, descs_host, infos_host, n, workspace, workspace_bytes, status_dev, stream);
}

// The index built on the device (jpeg_index.hip; the rule: hh_jpeg_index_device_batch in include/hhrnet.h).
int hh_jpeg_index_config(int out[4])
{
    if (!out) { hh_set_error("hh_jpeg_index_config: null pointer"); return 1; }
    out[0] = JPEG_IDX_LANES, out[1] = JPEG_IDX_SUBSEQ, out[2] = JPEG_IDX_SUBSEQ_MIN, out[3] = JPEG_IDX_MPS;
    return 0;
}

long long hh_jpeg_index_workspace_bytes(const hh_jpeg_stream_info *info, int subseq_bytes)
{
    const char *why = info ? jpeg_dec_check_info(*info) : "null pointer";
    if (!why) why = jpeg_idx_check_params(1, subseq_bytes);
    if (why) { hh_set_error(std::string("hh_jpeg_index_workspace_bytes: ") + why); return -1; }
    return 0;  // (a round's states live in LDS, what it hands on in registers: see the header)
}

int hh_jpeg_index_tables(const unsigned char *bytes, long long len, int mcus_per_segment, unsigned char *out, long long out_bytes, int *nseg)
{
    const std::string fn = "hh_jpeg_index_tables";
    if (!bytes || !out || !nseg) { hh_set_error(fn + ": null pointer"); return 1; }
    JpegStreamInfo I;
    std::vector<JpegDecTables> T(1);
    const char *why = jpeg_dec_parse(bytes, len, &I, &T[0]);
    if (!why && mcus_per_segment < 1) why = "mcus_per_segment must be at least 1";
    if (!why && I.restart_interval) why = "the stream has a restart interval (use hh_jpeg_restart_segments)";
    const int n = why ? 0 : jpeg_dec_index_count(I, mcus_per_segment);
    if (!why && out_bytes < jpeg_dec_tables_bytes(n)) why = "room below hh_jpeg_decode_tables_bytes";
    if (!why && (uintptr_t)(out + JPEG_DEC_SEGS_AT) % alignof(JpegSegment)) why = "the table block must be 4-byte aligned";
    if (why) { hh_set_error(fn + ": " + why); return 1; }
    I.reserved[1] = JPEG_IDX_PENDING;
    memcpy(out, &I, sizeof(I));
    memcpy(out + JPEG_DEC_TABLES_AT, &T[0], sizeof(JpegDecTables));
    jpeg_idx_blank(I, mcus_per_segment, reinterpret_cast<JpegSegment *>(out + JPEG_DEC_SEGS_AT), n);
    *nseg = n;
    return 0;
}

int hh_jpeg_index_device_batch(unsigned char *batch_base, const hh_jpeg_dec_desc *descs_dev, const hh_jpeg_dec_desc *descs_host,
                               const hh_jpeg_stream_info *infos_host, int n, int mcus_per_segment, int subseq_bytes, unsigned char *workspace,
                               long long workspace_bytes, int32_t *status_dev, void *stream)
{
    const std::string fn = "hh_jpeg_index_device_batch";
    (void)workspace;  // (no global scratch: hh_jpeg_index_workspace_bytes is 0)
    if (!batch_base || !descs_dev || !descs_host || !infos_host || !status_dev) { hh_set_error(fn + ": null pointer"); return 1; }
    if (n < 1 || n > 65535) { hh_set_error(fn + ": need 1 <= n <= 65535"); return 1; }
    if ((uintptr_t)descs_dev % 8 || (uintptr_t)status_dev % 4) { hh_set_error(fn + ": descs_dev must be 8-byte and status_dev 4-byte aligned"); return 1; }
    const char *bad = jpeg_idx_check_params(mcus_per_segment, subseq_bytes);
    if (!bad && workspace_bytes < 0) bad = "workspace_bytes is negative";
    if (bad) { hh_set_error(fn + ": " + bad); return 1; }
    bool any = false;
    for (int b = 0; b < n; ++b) {
        const JpegDecDesc &d = descs_host[b];
        const JpegStreamInfo &I = infos_host[b];
        JpegDecGeom g;
        const char *why = jpeg_dec_check_image(batch_base, d, I, nullptr, 1ll << 62, &g);  // (the decode's workspace is the decode's to check)
        const bool pending = !why && !I.restart_interval && I.reserved[1] == JPEG_IDX_PENDING;
        if (pending && d.nseg != jpeg_dec_index_count(I, mcus_per_segment)) why = "nseg is not the entry count of mcus_per_segment (hh_jpeg_index_tables)";
        if (why) { hh_set_error(fn + ": image " + std::to_string(b) + ": " + why); return 1; }
        any = any || pending;
    }
    HH_CHECK_HIP(hipMemsetAsync(status_dev, 0, (size_t)n * 4, (hipStream_t)stream));
    if (any) HH_CHECK_HIP(launch_jpeg_index(batch_base, descs_dev, n, mcus_per_segment, subseq_bytes, status_dev, (hipStream_t)stream));
    return 0;
}

int hh_debug_jpeg_index_sync_host(const unsigned char *bytes, long long len, int mcus_per_segment, int subseq_bytes, int lanes, hh_jpeg_segment *entries,
                                  int capacity, int *n, int *status, long long counts[6])
{
    const std::string fn = "hh_debug_jpeg_index_sync_host";
    if (!bytes || !entries || !n) { hh_set_error(fn + ": null pointer"); return 1; }
    JpegStreamInfo I;
    std::vector<JpegDecTables> T(1);
    const char *why = jpeg_dec_parse(bytes, len, &I, &T[0]);
    int st = 0;
    if (status) *status = 0;
    if (!why) why = jpeg_idx_sync_host(bytes, len, I, T[0], mcus_per_segment, subseq_bytes, lanes, entries, capacity, n, &st, reinterpret_cast<JpegIdxCounts *>(counts));
    if (status) *status = st;
    if (why) { hh_set_error(fn + ": " + why + (st ? std::string(": ") + JPEG_STATUS_NAME[st] : std::string())); return 1; }
    return 0;
}

// The segments of a stream when the caller gave none: its restart intervals, or the whole scan as one segment (no index is needed for
// a single lane).
static const char *jpeg_own_segments(const unsigned char *bytes, const JpegStreamInfo &I, std::vector<JpegSegment> &own)
{
    if (I.restart_interval) {
        own.resize(I.nseg_restart);
        return jpeg_dec_restart_segments(bytes, I, own.data());
    }
    own.push_back(JpegSegment{0, I.mcols * I.mrows, (int32_t)I.scan_offset, 0, {0, 0, 0}, (int32_t)(I.scan_end << 1)});
    return nullptr;
}

// Both host twins.  window: null for the whole image, which is decoded from the stream and the entries as they are given
// (hh_jpeg_decode_tables); a window from the selected segments and their slice (hh_jpeg_decode_window_tables).
static int jpeg_decode_host(const std::string &fn, const unsigned char *bytes, long long len, const hh_jpeg_segment *entries, int nseg,
                            const hh_jpeg_window *window, int flags, unsigned char *dst, long long pitch, int *status, hh_jpeg_window_counts *counts)
{
    if (status) *status = 0;
    JpegStreamInfo I;
    std::vector<JpegDecTables> T(1);
    const char *why = jpeg_dec_parse(bytes, len, &I, &T[0]);
    const JpegWindow W = why ? JpegWindow() : window ? *window : jpeg_full_window(I);
    if (!why && window) why = jpeg_win_check(I, W);
    if (!why && pitch < 3ll * W.width) why = window ? "pitch below 3 * width" : "pitch below 3 * w";
    if (!why && (flags & ~1)) why = "unknown flag";
    if (!why && entries && nseg < 1) why = "nseg must be at least 1";
    std::vector<JpegSegment> own;
    if (!why && !entries) {
        why = jpeg_own_segments(bytes, I, own);
        entries = own.data();
        nseg = (int)own.size();
    }
    const JpegSegment *seg = entries;
    const JpegWinRect R = why ? JpegWinRect() : jpeg_win_rect(I, W);
    int nsel = nseg;
    long long slice[2] = {0, len};
    if (!why && window) why = jpeg_win_select(I, R, seg, nseg, &nsel, slice);
    if (why) { hh_set_error(fn + ": " + why); return 1; }
    // what the device receives: the table block, the stream or the slice in a block of its own, the rectangle's workspace
    const std::vector<unsigned char> part(bytes + slice[0], bytes + slice[1]);
    std::vector<JpegVec8> block((size_t)jpeg_dec_tables_bytes(nsel) / 16 + 1), ws((size_t)jpeg_dec_geom(I, R).ws_bytes / 16 + 1);
    unsigned char *blk = reinterpret_cast<unsigned char *>(block.data());
    if (window) {
        jpeg_win_tables(I, T[0], R, seg, nseg, slice, blk);
    } else {
        memcpy(blk, &I, sizeof(I));
        memcpy(blk + JPEG_DEC_TABLES_AT, &T[0], sizeof(JpegDecTables));
        memcpy(blk + JPEG_DEC_SEGS_AT, seg, (size_t)nseg * sizeof(JpegSegment));
    }
    memset(ws.data(), 0, ws.size() * 16);
    JpegWinCounts local = {0, 0, 0, 0, 0, 0};
    const int st = jpeg_dec_window_host(part.data(), (int)part.size(), blk, nsel, W, flags & 1, reinterpret_cast<unsigned char *>(ws.data()), dst, pitch, &local,
                                        nullptr);
    if (counts) memcpy(counts, &local, sizeof(local));
    if (status) *status = st;
    if (st) { hh_set_error(fn + ": status " + std::to_string(st) + " (" + JPEG_STATUS_NAME[st] + ")"); return 1; }
    return 0;
}

int hh_debug_jpeg_decode_host(const unsigned char *bytes, long long len, const hh_jpeg_segment *entries, int nseg, int flags, unsigned char *dst,
                              long long pitch, int *status)
{
    if (!bytes || !dst) { hh_set_error("hh_debug_jpeg_decode_host: null pointer"); return 1; }
    return jpeg_decode_host("hh_debug_jpeg_decode_host", bytes, len, entries, nseg, nullptr, flags, dst, pitch, status, nullptr);
}

// The window decode (the rule: hh_jpeg_decode_window_u8_batch in include/hhrnet.h).

long long hh_jpeg_decode_window_workspace_bytes(const hh_jpeg_stream_info *info, const hh_jpeg_window *window)
{
    const char *why = info && window ? jpeg_dec_check_info(*info, true) : "null pointer";
    if (!why) why = jpeg_win_check(*info, *window);
    if (why) { hh_set_error(std::string("hh_jpeg_decode_window_workspace_bytes: ") + why); return -1; }
    const JpegStreamInfo &I = *info;
    return jpeg_dec_geom(I, jpeg_win_rect(I, *window)).ws_bytes;
}

int hh_jpeg_decode_window_select(const hh_jpeg_stream_info *info, const hh_jpeg_segment *entries, int nseg, const hh_jpeg_window *window, int *nsel,
                                 long long slice[2])
{
    const std::string fn = "hh_jpeg_decode_window_select";
    if (!info || !entries || !window || !nsel || !slice) { hh_set_error(fn + ": null pointer"); return 1; }
    const JpegStreamInfo &I = *info;
    const JpegWindow &W = *window;
    const char *why = jpeg_dec_check_info(I);
    if (!why && nseg < 1) why = "nseg must be at least 1";
    if (!why) why = jpeg_win_check(I, W);
    if (!why) why = jpeg_win_select(I, jpeg_win_rect(I, W), entries, nseg, nsel, slice);
    if (why) { hh_set_error(fn + ": " + why); return 1; }
    return 0;
}

int hh_jpeg_decode_window_tables(const unsigned char *bytes, long long len, const hh_jpeg_segment *entries, int nseg, const hh_jpeg_window *window,
                                 unsigned char *out, long long out_bytes, int *nsel, long long slice[2])
{
    const std::string fn = "hh_jpeg_decode_window_tables";
    if (!bytes || !entries || !window || !out || !nsel || !slice) { hh_set_error(fn + ": null pointer"); return 1; }
    JpegStreamInfo I;
    std::vector<JpegDecTables> T(1);
    const JpegWindow &W = *window;
    const char *why = nseg < 1 ? "nseg must be at least 1" : jpeg_dec_parse(bytes, len, &I, &T[0]);
    if (!why) why = jpeg_win_check(I, W);
    int n = 0;
    long long sl[2] = {0, 0};
    if (!why) why = jpeg_win_select(I, jpeg_win_rect(I, W), entries, nseg, &n, sl);
    if (!why && out_bytes < jpeg_dec_tables_bytes(n)) why = "room below hh_jpeg_decode_tables_bytes of the selected segments";
    if (why) { hh_set_error(fn + ": " + why); return 1; }
    jpeg_win_tables(I, T[0], jpeg_win_rect(I, W), entries, nseg, sl, out);
    *nsel = n, slice[0] = sl[0], slice[1] = sl[1];
    return 0;
}

int hh_jpeg_decode_window_u8_batch(unsigned char *batch_base, const hh_jpeg_win_desc *descs_dev, const hh_jpeg_win_desc *descs_host,
                                   const hh_jpeg_stream_info *infos_host, int n, unsigned char *workspace, long long workspace_bytes,
                                   int32_t *status_dev, void *stream)
{
    return jpeg_decode_batch("hh_jpeg_decode_window_u8_batch", true, batch_base, descs_dev, descs_host, infos_host, n, workspace, workspace_bytes, status_dev,
                             stream);
}

int hh_debug_jpeg_decode_window_host(const unsigned char *bytes, long long len, const hh_jpeg_segment *entries, int nseg, const hh_jpeg_window *window,
                                     int flags, unsigned char *dst, long long pitch, int *status, hh_jpeg_window_counts *counts)
{
    if (!bytes || !dst || !window) { hh_set_error("hh_debug_jpeg_decode_window_host: null pointer"); return 1; }
    return jpeg_decode_host("hh_debug_jpeg_decode_window_host", bytes, len, entries, nseg, window, flags, dst, pitch, status, counts);
}

int hh_resize_u8(const unsigned char *src, int h, int w, int channels, unsigned char *dst, int H, int W, void *stream)
{
    const char *fn = "hh_resize_u8";
    if (!src || !dst) { hh_set_error(std::string(fn) + ": null pointer"); return 1; }
    if (channels != 1 && channels != 3) { hh_set_error(std::string(fn) + ": channels must be 1 or 3"); return 1; }
    if (h < 1 || w < 1 || H < 1 || W < 1 || h > HH_RESIZE_MAX_SIDE || w > HH_RESIZE_MAX_SIDE || H > HH_RESIZE_MAX_SIDE || W > HH_RESIZE_MAX_SIDE) {
        hh_set_error(std::string(fn) + ": every side must lie in 1..16384");
        return 1;
    }
    // (with sides <= 16384 and 3 channels both images stay below 2^31 bytes: the kernel indexes the source with 32 bits)
    HH_CHECK_HIP(launch_resize_u8(src, h, w, channels, dst, H, W, (hipStream_t)stream));
    return 0;
}

int hh_resize_u8_scaled(const unsigned char *src, int h, int w, int channels, double fx, double fy, unsigned char *dst, int H, int W, void *stream)
{
    const char *fn = "hh_resize_u8_scaled";
    if (!src || !dst) { hh_set_error(std::string(fn) + ": null pointer"); return 1; }
    if (channels != 1 && channels != 3) { hh_set_error(std::string(fn) + ": channels must be 1 or 3"); return 1; }
    if (!(fx > 0.0) || !(fy > 0.0) || !std::isfinite(fx) || !std::isfinite(fy)) { hh_set_error(std::string(fn) + ": fx and fy must be positive and finite"); return 1; }
    if (h < 1 || w < 1 || H < 1 || W < 1 || h > HH_RESIZE_MAX_SIDE || w > HH_RESIZE_MAX_SIDE || H > HH_RESIZE_MAX_SIDE || W > HH_RESIZE_MAX_SIDE) {
        hh_set_error(std::string(fn) + ": every side must lie in 1..16384");
        return 1;
    }
    // cvRound of the double product: to nearest, half to even (the default rounding mode)
    if ((double)W != std::nearbyint((double)w * fx) || (double)H != std::nearbyint((double)h * fy)) {
        hh_set_error(std::string(fn) + ": H x W must be cvRound(h * fy) x cvRound(w * fx)");
        return 1;
    }
    HH_CHECK_HIP(launch_resize_u8_scaled(src, h, w, channels, dst, H, W, fx, fy, (hipStream_t)stream));
    return 0;
}

int hh_unnormalize_u8(const float *x_chw, int H, int W, const double mean[3], const double stdv[3], unsigned char *out_hwc, void *stream)
{
    const char *fn = "hh_unnormalize_u8";
    if (!x_chw || !out_hwc || !mean || !stdv) { hh_set_error(std::string(fn) + ": null pointer"); return 1; }
    if (H < 1 || W < 1 || H > HH_RESIZE_MAX_SIDE || W > HH_RESIZE_MAX_SIDE) { hh_set_error(std::string(fn) + ": every side must lie in 1..16384"); return 1; }
    HH_CHECK_HIP(launch_unnormalize_u8(x_chw, H, W, out_hwc, mean, stdv, (hipStream_t)stream));
    return 0;
}

// The checks of a panels call that need no device, on the caller's host copy of the table; *any_minmax: does any map ask for the range.
static int panels_check(const char *fn, const hh_panel_map *maps_host, int n, const void *image, int H, int W, const void *lut, const void *canvas, int Hc,
                        int Wc, long long pitch, bool *any_minmax)
{
    if (!maps_host || !image || !lut || !canvas) { hh_set_error(std::string(fn) + ": null pointer"); return 1; }
    const char *why = panel_check(maps_host, n, H, W, Hc, Wc, pitch);
    if (why) { hh_set_error(std::string(fn) + ": " + why); return 1; }
    *any_minmax = false;
    for (int i = 0; i < n; ++i) *any_minmax |= (maps_host[i].flags & HH_PANEL_MINMAX) != 0;
    return 0;
}

int hh_heatmap_panels_u8(const hh_panel_map *maps_dev, const hh_panel_map *maps_host, int n, const unsigned char *image, int H, int W,
                         const unsigned char *lut, unsigned char *canvas, int Hc, int Wc, long long pitch, float *scratch, void *stream)
{
    const char *fn = "hh_heatmap_panels_u8";
    bool any_minmax = false;
    if (!maps_dev) { hh_set_error(std::string(fn) + ": null pointer"); return 1; }
    if ((uintptr_t)maps_dev % 8) { hh_set_error(std::string(fn) + ": maps_dev must be 8-byte aligned"); return 1; }
    if (panels_check(fn, maps_host, n, image, H, W, lut, canvas, Hc, Wc, pitch, &any_minmax)) return 1;
    if (any_minmax && (!scratch || (uintptr_t)scratch % 4)) { hh_set_error(std::string(fn) + ": a map asks for min-max and scratch is null or misaligned"); return 1; }
    HH_CHECK_HIP(launch_panels(maps_dev, n, any_minmax, image, H, W, lut, canvas, Hc, Wc, pitch, scratch, (hipStream_t)stream));
    return 0;
}

int hh_debug_heatmap_panels_host(const hh_panel_map *maps, int n, const unsigned char *image, int H, int W, const unsigned char *lut, unsigned char *canvas,
                                 int Hc, int Wc, long long pitch)
{
    const char *fn = "hh_debug_heatmap_panels_host";
    bool any_minmax = false;
    if (panels_check(fn, maps, n, image, H, W, lut, canvas, Hc, Wc, pitch, &any_minmax)) return 1;
    std::vector<PanelRange> ranges(n);
    panels_debug_host(maps, n, image, H, W, lut, canvas, Hc, Wc, pitch, ranges.data());
    return 0;
}

// The checks of a COCO scoring call that need no device: the host copy's contents (coco_check), and of the device copy only that its
// pointers are there and aligned and that its counts are the host copy's.  Nothing behind a device pointer is read.
static int coco_tables_check(const char *fn, const hh_coco_tables *dev, const hh_coco_tables *host)
{
    char msg[192];
    const char *why = coco_check(host, msg, sizeof msg);
    if (why) { hh_set_error(std::string(fn) + ": " + why); return 1; }
    if (!dev) return 0;  // (the host entry point)
    const void *p8[] = {dev->oks_off, dev->dt_xy, dev->dt_score, dev->dt_area, dev->gt_xyv, dev->gt_area, dev->gt_bbox, dev->vars, dev->area_rng, dev->thr};
    for (const void *p : p8) {
        if (!p) { hh_set_error(std::string(fn) + ": null pointer"); return 1; }
        if ((uintptr_t)p % 8) { hh_set_error(std::string(fn) + ": a device table is not 8-byte aligned"); return 1; }
    }
    if (!dev->dt_off || !dev->gt_off || !dev->gt_flags) { hh_set_error(std::string(fn) + ": null pointer"); return 1; }
    if ((uintptr_t)dev->dt_off % 4 || (uintptr_t)dev->gt_off % 4) { hh_set_error(std::string(fn) + ": a device table is not 4-byte aligned"); return 1; }
    if (dev->I != host->I || dev->N != host->N || dev->M != host->M || dev->K != host->K || dev->A != host->A || dev->T != host->T) {
        hh_set_error(std::string(fn) + ": the device tables' counts differ from the host copy's");
        return 1;
    }
    return 0;
}
static int coco_outputs_check(const char *fn, const int32_t *dt_match, const uint8_t *dt_ignore, const uint8_t *gt_ignore)
{
    if (!dt_match || !dt_ignore || !gt_ignore) { hh_set_error(std::string(fn) + ": null pointer"); return 1; }
    if ((uintptr_t)dt_match % 4) { hh_set_error(std::string(fn) + ": dt_match is not 4-byte aligned"); return 1; }
    return 0;
}

int hh_coco_oks(const hh_coco_tables *tables_dev, const hh_coco_tables *tables_host, double *oks, void *stream)
{
    const char *fn = "hh_coco_oks";
    if (!tables_dev || !oks) { hh_set_error(std::string(fn) + ": null pointer"); return 1; }
    if ((uintptr_t)oks % 8) { hh_set_error(std::string(fn) + ": oks is not 8-byte aligned"); return 1; }
    if (coco_tables_check(fn, tables_dev, tables_host)) return 1;
    HH_CHECK_HIP(launch_coco_eval(1, *tables_dev, nullptr, oks, nullptr, nullptr, nullptr, (hipStream_t)stream));
    return 0;
}

int hh_coco_match(const hh_coco_tables *tables_dev, const hh_coco_tables *tables_host, const double *oks, int32_t *dt_match, unsigned char *dt_ignore,
                  unsigned char *gt_ignore, void *stream)
{
    const char *fn = "hh_coco_match";
    if (!tables_dev || !oks) { hh_set_error(std::string(fn) + ": null pointer"); return 1; }
    if ((uintptr_t)oks % 8) { hh_set_error(std::string(fn) + ": oks is not 8-byte aligned"); return 1; }
    if (coco_outputs_check(fn, dt_match, dt_ignore, gt_ignore) || coco_tables_check(fn, tables_dev, tables_host)) return 1;
    HH_CHECK_HIP(launch_coco_eval(2, *tables_dev, oks, nullptr, dt_match, dt_ignore, gt_ignore, (hipStream_t)stream));
    return 0;
}

int hh_coco_evaluate(const hh_coco_tables *tables_dev, const hh_coco_tables *tables_host, int32_t *dt_match, unsigned char *dt_ignore,
                     unsigned char *gt_ignore, void *stream)
{
    const char *fn = "hh_coco_evaluate";
    if (!tables_dev) { hh_set_error(std::string(fn) + ": null pointer"); return 1; }
    if (coco_outputs_check(fn, dt_match, dt_ignore, gt_ignore) || coco_tables_check(fn, tables_dev, tables_host)) return 1;
    HH_CHECK_HIP(launch_coco_eval(0, *tables_dev, nullptr, nullptr, dt_match, dt_ignore, gt_ignore, (hipStream_t)stream));
    return 0;
}

int hh_coco_evaluate_host(const hh_coco_tables *tables_host, const double *oks_in, double *oks_out, int32_t *dt_match, unsigned char *dt_ignore,
                          unsigned char *gt_ignore)
{
    const char *fn = "hh_coco_evaluate_host";
    const bool match = dt_match || dt_ignore || gt_ignore;
    if (match && coco_outputs_check(fn, dt_match, dt_ignore, gt_ignore)) return 1;
    if (!match && !oks_out) { hh_set_error(std::string(fn) + ": null pointer"); return 1; }
    if (coco_tables_check(fn, nullptr, tables_host)) return 1;
    coco_eval_host(*tables_host, oks_in, oks_in ? nullptr : oks_out, match, dt_match, dt_ignore, gt_ignore);
    return 0;
}

// The checks of a tracking call: the parameter block (track_check) and the pointers.  Nothing behind a device pointer is read.
static int track_args_check(const char *fn, const hh_track_params *params, const void *state, const float *joints, const float *scores,
                            const int32_t *num_people, const int32_t *flags, int S, int F)
{
    if (!params || !state || !joints || !scores || !num_people) { hh_set_error(std::string(fn) + ": null pointer"); return 1; }
    if ((uintptr_t)state % 8) { hh_set_error(std::string(fn) + ": state is not 8-byte aligned"); return 1; }
    if ((uintptr_t)joints % 4 || (uintptr_t)scores % 4 || (uintptr_t)num_people % 4 || (uintptr_t)flags % 4) { hh_set_error(std::string(fn) + ": an input is not 4-byte aligned"); return 1; }
    if (S < 0 || F < 0 || (int64_t)S * F > (1 << 24)) { hh_set_error(std::string(fn) + ": S and F must be >= 0 and S * F <= 2^24"); return 1; }
    if (const char *why = track_check(params)) { hh_set_error(std::string(fn) + ": " + why); return 1; }
    return 0;
}
static int track_outputs_check(const char *fn, const int32_t *track_ids, const float *smooth, const int32_t *out_flags)
{
    if (!track_ids || !smooth || !out_flags) { hh_set_error(std::string(fn) + ": null pointer"); return 1; }
    if ((uintptr_t)track_ids % 4 || (uintptr_t)smooth % 4 || (uintptr_t)out_flags % 4) { hh_set_error(std::string(fn) + ": an output is not 4-byte aligned"); return 1; }
    return 0;
}
static int track_assign_check(const char *fn, const double *sim, const int32_t *ids, int n, int T, int P, double min_oks, const int32_t *match)
{
    if (!sim || !ids || !match) { hh_set_error(std::string(fn) + ": null pointer"); return 1; }
    if ((uintptr_t)sim % 8 || (uintptr_t)ids % 4 || (uintptr_t)match % 4) { hh_set_error(std::string(fn) + ": sim must be 8-byte, ids and match 4-byte aligned"); return 1; }
    if (n < 0 || n > (1 << 24)) { hh_set_error(std::string(fn) + ": n outside 0..2^24"); return 1; }
    if (T < 1 || T > HH_TRACK_MAX_TRACKS || P < 1 || P > HH_TRACK_MAX_PEOPLE) { hh_set_error(std::string(fn) + ": T and P must lie in 1..64"); return 1; }
    if (!(min_oks > 0.0) || !(min_oks <= 1.0)) { hh_set_error(std::string(fn) + ": min_oks outside (0, 1]"); return 1; }
    return 0;
}

int64_t hh_track_state_bytes(int K, int max_tracks)
{
    if (K < 1 || K > HH_TRACK_MAX_K || max_tracks < 1 || max_tracks > HH_TRACK_MAX_TRACKS) { hh_set_error("hh_track_state_bytes: K and max_tracks must lie in 1..64"); return -1; }
    return track_state_bytes(K, max_tracks);
}

int hh_track_reset(void *state, int K, int max_tracks, int nstreams, void *stream)
{
    const char *fn = "hh_track_reset";
    if (!state) { hh_set_error(std::string(fn) + ": null pointer"); return 1; }
    if ((uintptr_t)state % 8) { hh_set_error(std::string(fn) + ": state is not 8-byte aligned"); return 1; }
    if (K < 1 || K > HH_TRACK_MAX_K || max_tracks < 1 || max_tracks > HH_TRACK_MAX_TRACKS || nstreams < 0 || nstreams > (1 << 24)) {
        hh_set_error(std::string(fn) + ": K and max_tracks must lie in 1..64, nstreams in 0..2^24");
        return 1;
    }
    if (nstreams) HH_CHECK_HIP(hipMemsetAsync(state, 0, (size_t)nstreams * track_state_bytes(K, max_tracks), (hipStream_t)stream));
    return 0;
}

int hh_track_step(const hh_track_params *params, void *state, const float *joints, const float *scores, const int32_t *num_people, const int32_t *flags, int S,
                  int F, int32_t *track_ids, float *smooth, int32_t *out_flags, void *stream)
{
    const char *fn = "hh_track_step";
    if (track_outputs_check(fn, track_ids, smooth, out_flags) || track_args_check(fn, params, state, joints, scores, num_people, flags, S, F)) return 1;
    HH_CHECK_HIP(launch_track_step(*params, state, joints, scores, num_people, flags, S, F, track_ids, smooth, out_flags,
                                   (hipStream_t)stream));
    return 0;
}

int hh_track_step_host(const hh_track_params *params, void *state, const float *joints, const float *scores, const int32_t *num_people, const int32_t *flags,
                       int S, int F, int32_t *track_ids, float *smooth, int32_t *out_flags)
{
    const char *fn = "hh_track_step_host";
    if (track_outputs_check(fn, track_ids, smooth, out_flags) || track_args_check(fn, params, state, joints, scores, num_people, flags, S, F)) return 1;
    track_step_host(*params, state, joints, scores, num_people, flags, S, F, track_ids, smooth, out_flags);
    return 0;
}

int hh_track_similarity(const hh_track_params *params, void *state, const float *joints, const float *scores, const int32_t *num_people, const int32_t *flags,
                        int S, double *sim, void *stream)
{
    const char *fn = "hh_track_similarity";
    if (!sim) { hh_set_error(std::string(fn) + ": null pointer"); return 1; }
    if ((uintptr_t)sim % 8) { hh_set_error(std::string(fn) + ": sim is not 8-byte aligned"); return 1; }
    if (track_args_check(fn, params, state, joints, scores, num_people, flags, S, 1)) return 1;
    HH_CHECK_HIP(launch_track_similarity(*params, state, joints, scores, num_people, flags, S, sim, (hipStream_t)stream));
    return 0;
}

int hh_track_assign(const double *sim, const int32_t *ids, int n, int T, int P, double min_oks, int32_t *match, void *stream)
{
    if (track_assign_check("hh_track_assign", sim, ids, n, T, P, min_oks, match)) return 1;
    HH_CHECK_HIP(launch_track_assign(sim, ids, n, T, P, min_oks, match, (hipStream_t)stream));
    return 0;
}

int hh_track_assign_host(const double *sim, const int32_t *ids, int n, int T, int P, double min_oks, int32_t *match)
{
    if (track_assign_check("hh_track_assign_host", sim, ids, n, T, P, min_oks, match)) return 1;
    for (int m = 0; m < n; ++m) track_assign_host(sim + (size_t)m * T * P, ids + (size_t)m * T, T, P, min_oks, match + (size_t)m * T, nullptr);
    return 0;
}

// The checks of a pose scoring call that need no device: the host copies' contents (pose_check) and the alignment of every pointer that
// will be dereferenced.  `dev`: the addresses the kernel reads (for the host entry point the same struct as `host`).
static int pose_args_check(const char *fn, const PoseTables &dev, const PoseTables &host, const double *vars, const double *value, const double *obj,
                           const double *kpt, const int32_t *match, const int32_t *status)
{
    auto fail = [&](const char *why) { hh_set_error(std::string(fn) + ": " + why); return 1; };
    if (!vars || !value || !obj || !kpt || !match || !status) return fail("null pointer");
    char msg[192];
    if (const char *why = pose_check(host, msg, sizeof msg)) return fail(why);
    const bool decode = host.form == HH_POSE_PRED_DECODE;
    const void *p8[] = {value, obj, kpt, dev.t_xyv, dev.t_area, dev.t_head, decode ? (const void *)dev.inv_affine : dev.p_xy, decode ? nullptr : dev.p_score};
    const void *p4[] = {match, status, dev.t_off, decode ? (const void *)dev.joints : dev.p_off, decode ? (const void *)dev.scores : dev.p_off,
                        decode ? (const void *)dev.num : dev.p_off};
    for (const void *p : p8)
        if ((uintptr_t)p % 8) return fail("an fp64 table or output is not 8-byte aligned");
    for (const void *p : p4)
        if ((uintptr_t)p % 4) return fail("a 4-byte table or output is not 4-byte aligned");
    if (decode ? (!dev.joints || !dev.scores || !dev.num || !dev.inv_affine) : (!dev.p_off || !dev.p_xy || !dev.p_score)) return fail("null pointer");
    if (!dev.t_off || !dev.t_xyv || !dev.t_area || !dev.t_head) return fail("null pointer");
    if (decode && (uintptr_t)dev.flags % 4) return fail("a 4-byte table or output is not 4-byte aligned");
    return 0;
}
static PoseTables pose_tables(int form, int metric, int B, int K, const float *joints, int64_t image_stride, int64_t person_stride, int64_t joint_stride,
                              const float *scores, int64_t score_stride, const int32_t *num, const int32_t *flags, int max_people, const double *inv_affine,
                              const int32_t *p_off, const double *p_xy, const double *p_score, const int32_t *t_off, const double *t_xyv, const double *t_area,
                              const double *t_head, const double *vars, double alpha)
{
    PoseTables t = {};
    t.joints = joints, t.scores = scores, t.num = num, t.flags = flags, t.inv_affine = inv_affine;
    t.p_off = p_off, t.p_xy = p_xy, t.p_score = p_score;
    t.t_off = t_off, t.t_xyv = t_xyv, t.t_area = t_area, t.t_head = t_head;
    for (int k = 0; k < HH_POSE_MAX_K; ++k) t.vars[k] = vars && k < K && K <= HH_POSE_MAX_K ? vars[k] : 1.0;
    t.alpha = alpha;
    t.image_stride = image_stride, t.person_stride = person_stride, t.joint_stride = joint_stride, t.score_stride = score_stride;
    t.B = B, t.K = K, t.form = form, t.metric = metric, t.max_people = max_people;
    return t;
}

int hh_pose_score_batch(int form, int metric, int B, int K, const float *joints, int64_t image_stride, int64_t person_stride, int64_t joint_stride,
                        const float *scores, int64_t score_stride, const int32_t *num, const int32_t *flags, int max_people, const double *inv_affine_dev,
                        const double *inv_affine_host, const int32_t *p_off_dev, const int32_t *p_off_host, const double *p_xy, const double *p_score,
                        const int32_t *t_off_dev, const int32_t *t_off_host, const double *t_xyv_dev, const double *t_xyv_host, const double *t_area_dev,
                        const double *t_area_host, const double *t_head_dev, const double *t_head_host, const double *vars_host, double alpha, double *value,
                        double *obj, double *kpt, int32_t *match, int32_t *status, void *stream)
{
    const char *fn = "hh_pose_score_batch";
    const PoseTables dev = pose_tables(form, metric, B, K, joints, image_stride, person_stride, joint_stride, scores, score_stride, num, flags, max_people,
                                       inv_affine_dev, p_off_dev, p_xy, p_score, t_off_dev, t_xyv_dev, t_area_dev, t_head_dev, vars_host, alpha);
    const PoseTables host = pose_tables(form, metric, B, K, nullptr, image_stride, person_stride, joint_stride, nullptr, score_stride, nullptr, nullptr, max_people,
                                        inv_affine_host, p_off_host, nullptr, nullptr, t_off_host, t_xyv_host, t_area_host, t_head_host, vars_host, alpha);
    if (pose_args_check(fn, dev, host, vars_host, value, obj, kpt, match, status)) return 1;
    int max_P = max_people;
    if (form == HH_POSE_PRED_F64) {
        max_P = 1;  // (an LDS array of no bytes is never indexed, but keep its address distinct from the wave slots')
        for (int i = 0; i < B; ++i) max_P = std::max(max_P, p_off_host[i + 1] - p_off_host[i]);
    }
    HH_CHECK_HIP(launch_pose_score(dev, max_P, value, obj, kpt, match, status, (hipStream_t)stream));
    return 0;
}

int hh_pose_score_host(int form, int metric, int B, int K, const float *joints, int64_t image_stride, int64_t person_stride, int64_t joint_stride,
                       const float *scores, int64_t score_stride, const int32_t *num, const int32_t *flags, int max_people, const double *inv_affine,
                       const int32_t *p_off, const double *p_xy, const double *p_score, const int32_t *t_off, const double *t_xyv, const double *t_area,
                       const double *t_head, const double *vars, double alpha, double *value, double *obj, double *kpt, int32_t *match, int32_t *status)
{
    const char *fn = "hh_pose_score_host";
    const PoseTables t = pose_tables(form, metric, B, K, joints, image_stride, person_stride, joint_stride, scores, score_stride, num, flags, max_people, inv_affine,
                                     p_off, p_xy, p_score, t_off, t_xyv, t_area, t_head, vars, alpha);
    if (pose_args_check(fn, t, t, vars, value, obj, kpt, match, status)) return 1;
    pose_score_host(t, value, obj, kpt, match, status);
    return 0;
}

int64_t hh_cls_eval_bytes(int N, int with_confusion)
{
    if (const char *why = cls_check_shape(N, with_confusion)) { hh_set_error(std::string("hh_cls_eval_bytes: ") + why); return -1; }
    return (int64_t)cls_acc_bytes(N, with_confusion);
}

static int cls_reset_check(const char *fn, const void *acc, int N, int with_confusion)
{
    if (!acc) { hh_set_error(std::string(fn) + ": null pointer"); return 1; }
    if ((uintptr_t)acc % 8) { hh_set_error(std::string(fn) + ": acc is not 8-byte aligned"); return 1; }
    if (const char *why = cls_check_shape(N, with_confusion)) { hh_set_error(std::string(fn) + ": " + why); return 1; }
    return 0;
}

int hh_cls_eval_reset(void *acc, int N, int with_confusion, void *stream)
{
    if (cls_reset_check("hh_cls_eval_reset", acc, N, with_confusion)) return 1;
    HH_CHECK_HIP(launch_cls_eval_reset(acc, N, with_confusion, (hipStream_t)stream));
    return 0;
}

int hh_cls_eval_reset_host(void *acc, int N, int with_confusion)
{
    if (cls_reset_check("hh_cls_eval_reset_host", acc, N, with_confusion)) return 1;
    cls_reset_host(acc, N, with_confusion);
    return 0;
}

int hh_cls_score_batch(const float *logits, const int64_t *targets, int B, int N, int k, void *acc, int32_t *topk_idx, float *topk_prob, int32_t *rank,
                       float *row_loss, void *stream)
{
    if (const char *why = cls_check(logits, targets, B, N, k, acc, topk_idx, topk_prob, rank, row_loss)) { hh_set_error(std::string("hh_cls_score_batch: ") + why); return 1; }
    HH_CHECK_HIP(launch_cls_score(logits, (const long long *)targets, B, N, k, acc, topk_idx, topk_prob, rank, row_loss, (hipStream_t)stream));
    return 0;
}

int hh_cls_score_host(const float *logits, const int64_t *targets, int B, int N, int k, void *acc, int32_t *topk_idx, float *topk_prob, int32_t *rank,
                      float *row_loss)
{
    if (const char *why = cls_check(logits, targets, B, N, k, acc, topk_idx, topk_prob, rank, row_loss)) { hh_set_error(std::string("hh_cls_score_host: ") + why); return 1; }
    cls_score_host(logits, (const long long *)targets, B, N, k, acc, topk_idx, topk_prob, rank, row_loss);
    return 0;
}

int hh_polygon_area(const double *xy, int n, double *area)
{
    if (!area) { hh_set_error("hh_polygon_area: null pointer"); return 1; }
    if (pose_polygon_area(xy, n, area)) { hh_set_error("hh_polygon_area: null xy, negative n, or a coordinate that is not finite or outside +-2^30"); return 1; }
    return 0;
}

int hh_pose_score_config(int out[4])
{
    if (!out) { hh_set_error("hh_pose_score_config: null pointer"); return 1; }
    out[0] = POSE_THREADS, out[1] = (int)pose_lds_bytes(HH_POSE_MAX_P, HH_POSE_MAX_K), out[2] = HH_POSE_MAX_T, out[3] = HH_POSE_MAX_P;
    return 0;
}

int hh_crowd_mask_config(int out[4])
{
    if (!out) { hh_set_error("hh_crowd_mask_config: null pointer"); return 1; }
    out[0] = CROWD_TH, out[1] = CROWD_TW, out[2] = CROWD_THREADS, out[3] = 0;  // no per-chunk toggle capacity: toggles are read in place
    return 0;
}

long long hh_crowd_polygon_capacity(const double *xy, int k, int h, int w)
{
    const char *fn = "hh_crowd_polygon_capacity";
    if (!xy) { hh_set_error(std::string(fn) + ": null pointer"); return -1; }
    if (const char *why = crowd_polygon_check(xy, k, h, w)) { hh_set_error(std::string(fn) + ": " + why); return -1; }
    return crowd_polygon_bound(xy, k, w);
}

long long hh_crowd_polygon_toggles(const double *xy, int k, int h, int w, unsigned int *out, long long capacity)
{
    const char *fn = "hh_crowd_polygon_toggles";
    if (!xy || (!out && capacity > 0)) { hh_set_error(std::string(fn) + ": null pointer"); return -1; }
    if (capacity < 0) { hh_set_error(std::string(fn) + ": negative capacity"); return -1; }
    if (const char *why = crowd_polygon_check(xy, k, h, w)) { hh_set_error(std::string(fn) + ": " + why); return -1; }
    std::vector<uint32_t> pos;
    crowd_polygon_walk(xy, k, h, w, pos);
    crowd_cancel(pos);
    if ((long long)pos.size() > capacity) {
        hh_set_error(std::string(fn) + ": " + std::to_string(pos.size()) + " toggles do not fit the capacity " + std::to_string(capacity));
        return -1;
    }
    if (!pos.empty()) memcpy(out, pos.data(), pos.size() * sizeof(uint32_t));
    return (long long)pos.size();
}

// The checks of a crowd-mask call that need no device, on the caller's host copies.
static int crowd_check(const char *fn, const hh_crowd_mask_desc *descs_host, const hh_crowd_seg_desc *segs_host, const unsigned char *host_base, int n,
                       int num_segs, int *max_tiles)
{
    if (!descs_host || !host_base || (num_segs > 0 && !segs_host)) { hh_set_error(std::string(fn) + ": null pointer"); return 1; }
    if (n <= 0 || n > 65535) { hh_set_error(std::string(fn) + ": need 0 < n <= 65535"); return 1; }
    if (num_segs < 0) { hh_set_error(std::string(fn) + ": negative table length"); return 1; }
    int tiles = 1;
    for (int b = 0; b < n; ++b) {
        const CrowdMaskDesc &d = descs_host[b];
        const char *why = crowd_check_mask(d, segs_host, num_segs, host_base);
        if (why) { hh_set_error(std::string(fn) + ": mask " + std::to_string(b) + ": " + why); return 1; }
        tiles = std::max(tiles, ((d.w + CROWD_TW - 1) / CROWD_TW) * ((d.h + CROWD_TH - 1) / CROWD_TH));
    }
    *max_tiles = tiles;
    return 0;
}

int hh_crowd_masks_u8_batch(unsigned char *batch_base, const hh_crowd_mask_desc *descs_dev, const hh_crowd_seg_desc *segs_dev,
                            const hh_crowd_mask_desc *descs_host, const hh_crowd_seg_desc *segs_host, const unsigned char *host_base, int n,
                            int num_segs, void *stream)
{
    const char *fn = "hh_crowd_masks_u8_batch";
    if (!batch_base || !descs_dev || (num_segs > 0 && !segs_dev)) { hh_set_error(std::string(fn) + ": null pointer"); return 1; }
    if ((uintptr_t)batch_base % 4) { hh_set_error(std::string(fn) + ": batch_base must be 4-byte aligned"); return 1; }
    int max_tiles = 0;
    if (crowd_check(fn, descs_host, segs_host, host_base, n, num_segs, &max_tiles)) return 1;
    HH_CHECK_HIP(launch_crowd_masks(batch_base, descs_dev, segs_dev, n,
                                    max_tiles, (hipStream_t)stream));
    return 0;
}

int hh_debug_crowd_masks_host(unsigned char *mask, const hh_crowd_mask_desc *desc_host, const hh_crowd_seg_desc *segs_host, const unsigned char *host_base,
                              int num_segs)
{
    const char *fn = "hh_debug_crowd_masks_host";
    if (!mask) { hh_set_error(std::string(fn) + ": null pointer"); return 1; }
    int max_tiles = 0;
    if (crowd_check(fn, desc_host, segs_host, host_base, 1, num_segs, &max_tiles)) return 1;
    crowd_mask_host(mask, *desc_host, segs_host, host_base);
    return 0;
}

int hh_heatmap_table_size(double sigma, int *n, int *reach)
{
    if (!n || !reach) { hh_set_error("hh_heatmap_table_size: null pointer"); return 1; }
    const double r = 3.0 * sigma + 1.0;
    if (!(sigma > 0.0) || !(r <= 1e6) || r != std::floor(r)) { hh_set_error("hh_heatmap_table_size: 3 * sigma + 1 must be a positive integer (sigma = 1, 2, 4, ...)"); return 1; }
    if (2 * (int)r + 1 > HH_RENDER_MAX_N) { hh_set_error("hh_heatmap_table_size: the bump table 6 * sigma + 3 would exceed 63 entries a side"); return 1; }
    *reach = (int)r;
    *n = 2 * (int)r + 1;
    return 0;
}

int hh_render_heatmaps(const int32_t *joints, const int32_t *num_people, int B, int P, int K, const float *table, int n, int reach,
                       float *out, int h, int w, void *stream)
{
    if (!joints || !num_people || !table || !out) { hh_set_error("hh_render_heatmaps: null pointer"); return 1; }
    if (n <= 0 || n > HH_RENDER_MAX_N || reach < 0 || n != 2 * reach + 1) { hh_set_error("hh_render_heatmaps: need a table of n = 2 * reach + 1 <= 63 entries a side"); return 1; }
    if (B <= 0 || B > 65535 || K <= 0 || K > 65535 || P <= 0 || h <= 0 || w <= 0 || w > HH_RENDER_MAX_W || (int64_t)h * w > (1 << 30)) {
        hh_set_error("hh_render_heatmaps: need 0 < B, K <= 65535, P > 0, 0 < w <= 4096, h > 0");
        return 1;
    }
    HH_CHECK_HIP(launch_render_heatmaps(joints, num_people, B, P, K, table, n, reach, out, h, w, (hipStream_t)stream));
    return 0;
}

int hh_loss_heatmaps(const float *pred, int64_t pred_bstride, const float *target, const float *mask, int B, int K, int h, int w,
                     float *loss, float *grad, int64_t grad_bstride, double *scratch, void *stream)
{
    if (!pred || !target || !mask || !loss || !scratch || B <= 0 || K <= 0 || h <= 0 || w <= 0) { hh_set_error("hh_loss_heatmaps: bad argument"); return 1; }
    if ((h * w) % 4 || pred_bstride % 4 || (grad && grad_bstride % 4)) { hh_set_error("hh_loss_heatmaps: h*w and the batch strides must be multiples of 4"); return 1; }
    // the kernel reads float4 from all three inputs and stores float4 to grad (NULL counts as aligned)
    if (((uintptr_t)pred | (uintptr_t)target | (uintptr_t)mask | (uintptr_t)grad) & 15) { hh_set_error("hh_loss_heatmaps: pred, target, mask and grad must be 16-byte aligned"); return 1; }
    HH_CHECK_HIP(launch_masked_mse(pred, pred_bstride, target, mask, B, K, h, w, loss, grad, grad_bstride, scratch, (hipStream_t)stream));
    return 0;
}

int hh_loss_ae_grouping(const float *tags, int64_t tags_bstride, const int32_t *joints, const int32_t *num_people, int B, int P, int K,
                        int h, int w, float *push_pull, float *grad, int64_t grad_bstride, float push_scale, float pull_scale,
                        double *scratch, void *stream)
{
    if (!tags || !joints || !num_people || !push_pull || !scratch || B <= 0 || P <= 0 || K <= 0 || h <= 0 || w <= 0) { hh_set_error("hh_loss_ae_grouping: bad argument"); return 1; }
    if (P > 2048) { hh_set_error("hh_loss_ae_grouping: at most 2048 people per image"); return 1; }
    HH_CHECK_HIP(launch_ae_grouping(tags, tags_bstride, joints, num_people, B, P, K, h, w, push_pull, grad, grad_bstride, push_scale,
                                    pull_scale, scratch, (hipStream_t)stream));
    return 0;
}

// ------------------------------------------------------------------ training building blocks
static int round_up_i(int a, int b) { return (a + b - 1) / b * b; }

int64_t hh_conv2d_workspace_bytes(int cin, int cout, int ks, int mode)
{
    const int ci = mode ? cout : cin, co = mode ? cin : cout;
    const int coutp = round_up_i(co, 32);
    int KC = 0, NT = 0;
    if (hh_family_pick(mode == 2 ? 2 : ks, 1, round_up_i(ci, 16), coutp, &KC, &NT)) return -1;
    const int cin_pad = round_up_i(ci, KC);
    return (int64_t)coutp * cin_pad * ks * ks * 2 + (int64_t)coutp * 4 + 512;
}

// Shape bookkeeping shared by hh_conv2d / hh_conv2d_packed / hh_pack_conv_weights_batch: the conv that actually runs for
// (cin, cout, ks, stride, mode) and the size of one packed weight set.
struct Conv2dPlan {
    int ci, co, coutp, kks, kstride, KC, NT, COUT_T, cin_pad, nsets;
    size_t wel;  // bf16 elements of ONE packed set (mode 2 has four: the output-parity phases)
};
static int conv2d_plan(int cin, int cout, int ks, int stride, int mode, Conv2dPlan *pl, const char *who)
{
    pl->ci = mode ? cout : cin; pl->co = mode ? cin : cout;  // channels of the conv that actually runs
    if (pl->ci % 16 || pl->co % 8) { hh_set_error((std::string(who) + ": input channels must be a multiple of 16 and output channels of 8").c_str()); return 1; }
    if (mode == 1 && stride != 1) { hh_set_error((std::string(who) + ": mode 1 is the data gradient of a stride-1 convolution").c_str()); return 1; }
    if (ks == 2 && stride != 1) { hh_set_error((std::string(who) + ": 2x2 kernels run at stride 1 only").c_str()); return 1; }
    if (mode == 2 && (stride != 2 || ks != 3)) { hh_set_error((std::string(who) + ": mode 2 is the data gradient of a 3x3 stride-2 convolution").c_str()); return 1; }
    pl->coutp = round_up_i(pl->co, 32);
    pl->kks = mode == 2 ? 2 : ks; pl->kstride = mode == 2 ? 1 : stride;  // kernel that actually runs
    if (hh_family_pick(pl->kks, pl->kstride, pl->ci, pl->coutp, &pl->KC, &pl->NT)) { hh_set_error((std::string(who) + ": no kernel family for this shape").c_str()); return 1; }
    pl->COUT_T = 32 * pl->NT; pl->cin_pad = round_up_i(pl->ci, pl->KC);
    pl->wel = (size_t)pl->coutp * pl->cin_pad * pl->kks * pl->kks;
    pl->nsets = mode == 2 ? 4 : 1;
    return 0;
}

// the instantiation that runs a plan on an output map Wo columns wide (of one phase in mode 2)
static int conv2d_pick(const Conv2dPlan &pl, int Wo) { return hh_pick_config(pl.kks, pl.kstride, pl.KC, pl.NT, Wo); }

int hh_conv2d_config(int cin, int cout, int ks, int stride, int mode, int Wo)
{
    Conv2dPlan pl;
    if (mode < 0 || mode > 2 || Wo <= 0 || conv2d_plan(cin, cout, ks, stride, mode, &pl, "hh_conv2d_config")) return -1;
    return conv2d_pick(pl, Wo);
}

// the element type of a training entry point: HH_ACT_BF16 / HH_ACT_F16, anything else is refused before any launch
static int act_dtype_ok(int act_dtype, const char *who)
{
    if (act_dtype == HH_ACT_BF16 || act_dtype == HH_ACT_F16) return 1;
    hh_set_error((std::string(who) + ": unknown activation dtype (HH_ACT_BF16 = 0, HH_ACT_F16 = 1)").c_str());
    return 0;
}

// w: fp32 weights (packed into `workspace` here) or, with prepacked != NULL, weight sets packed by hh_pack_conv_weights_batch
static int conv2d_impl(int act_dtype, const void *x, int B, int H, int W, int cin, const float *w, const bf16_raw *prepacked, int cout, int ks, int stride,
                       int mode, int pad_y, int pad_x, const float *bias, const void *res, int relu, void *y, void *workspace, void *stream,
                       const char *who)
{
    if (!act_dtype_ok(act_dtype, who)) return 1;
    if (pad_y < 0) pad_y = (ks - 1) / 2;
    if (pad_x < 0) pad_x = (ks - 1) / 2;
    static bool inited = false;
    if (!inited) { HH_CHECK_HIP(conv_init()); inited = true; }
    if (!x || (!w && !prepacked) || !y || (!workspace && !prepacked) || B <= 0 || H <= 0 || W <= 0) { hh_set_error((std::string(who) + ": bad argument").c_str()); return 1; }
    Conv2dPlan pl;
    if (conv2d_plan(cin, cout, ks, stride, mode, &pl, who)) return 1;
    if (mode == 1) { pad_y = ks - 1 - pad_y; pad_x = ks - 1 - pad_x; }  // the adjoint correlates with the rotated kernel
    const int co = pl.co, coutp = pl.coutp, KC = pl.KC, COUT_T = pl.COUT_T;
    const size_t wel = pl.wel;
    bf16_raw *packed = (bf16_raw *)workspace;
    float *zbias = workspace ? (float *)((char *)workspace + ((wel * 2 + 255) & ~(size_t)255)) : nullptr;
    hipStream_t s = (hipStream_t)stream;
    // the kernel reads coutp bias values: an all-zero device array serves the bias-free case (no memset per call), a bias
    // whose length is already a multiple of 32 is used in place, anything else is copied behind the packed weights
    static float *zeros_dev[64] = {};  // one per device: a process may drive several GPUs
    if (!bias && coutp <= 4096) {
        int dev = 0;
        HH_CHECK_HIP(hipGetDevice(&dev));
        float *&zeros = zeros_dev[dev & 63];
        if (!zeros) {  // (once per device; the wait: a null-stream memset is not ordered in front of launches on a non-blocking stream)
            HH_CHECK_HIP(hipMalloc((void **)&zeros, 4096 * 4));
            HH_CHECK_HIP(hipMemset(zeros, 0, 4096 * 4));
            HH_CHECK_HIP(hipDeviceSynchronize());
        }
        zbias = zeros;
    } else if (bias && co == coutp) {
        zbias = const_cast<float *>(bias);
    } else if (!workspace) {
        hh_set_error((std::string(who) + ": without a workspace the bias must be NULL or have a multiple of 32 entries").c_str());
        return 1;
    } else if (!bias) {
        HH_CHECK_HIP(hipMemsetAsync(zbias, 0, (size_t)coutp * 4, s));
    } else {
        HH_CHECK_HIP(hipMemcpyAsync(zbias, bias, (size_t)co * 4, hipMemcpyDeviceToDevice, s));
    }
    const int Ho = pl.kstride == 2 ? H / 2 : H, Wo = pl.kstride == 2 ? W / 2 : W;
    const int cfg = conv2d_pick(pl, Wo);
    if (cfg < 0) { hh_set_error((std::string(who) + ": no kernel instantiation for this shape").c_str()); return 1; }
    const ConvConfig &cc = conv_config(cfg);
    ConvParams p{};
    p.in = (const bf16_raw *)x; p.in_cs = pl.ci; p.Hin = H; p.Win = W;
    p.w = prepacked ? prepacked : packed; p.bias = zbias;
    p.res = (const bf16_raw *)res; p.res_cs = co;
    p.out = (bf16_raw *)y; p.out_cs = co;
    p.Ho = Ho; p.Wo = Wo; p.Hob = Ho; p.Wob = Wo; p.osy = p.osx = 1;
    p.cin = pl.cin_pad; p.cout_real = co; p.cout_store = co; p.relu = relu;
    p.pad_y = pad_y; p.pad_x = pad_x; p.B = B;
    p.tiles_x = (Wo + cc.TW - 1) / cc.TW; p.tiles_y = (Ho + cc.th() - 1) / cc.th(); p.ncg = coutp / cc.cout_t();
    if (mode == 2) {  // four output-parity phases, each a 2x2 conv over dL/dy scattered onto the 2H x 2W grid
        p.Hob = 2 * H; p.Wob = 2 * W; p.osy = p.osx = 2; p.pad_y = p.pad_x = 0;
        for (int ph = 0; ph < 4; ++ph) {
            if (prepacked) p.w = prepacked + (size_t)ph * wel;
            else HH_CHECK_HIP(launch_pack_weights(w, cout, cin, 2, 2, KC, COUT_T, packed, wel, s, ph >> 1, ph & 1, act_dtype));
            p.ooy = ph >> 1; p.oox = ph & 1;
            HH_CHECK_HIP(conv_launch(cfg, p, s, act_dtype));
        }
        return 0;
    }
    if (!prepacked) HH_CHECK_HIP(launch_pack_weights(w, cout, cin, ks, mode, KC, COUT_T, packed, wel, s, 0, 0, act_dtype));
    HH_CHECK_HIP(conv_launch(cfg, p, s, act_dtype));
    return 0;
}

int hh_conv2d_dt(int act_dtype, const void *x, int B, int H, int W, int cin, const float *w, int cout, int ks, int stride, int mode, int pad_y,
                 int pad_x, const float *bias, const void *res, int relu, void *y, void *workspace, void *stream)
{
    if (!w || !workspace) { hh_set_error("hh_conv2d: bad argument"); return 1; }
    return conv2d_impl(act_dtype, x, B, H, W, cin, w, nullptr, cout, ks, stride, mode, pad_y, pad_x, bias, res, relu, y, workspace, stream, "hh_conv2d");
}
int hh_conv2d(const void *x, int B, int H, int W, int cin, const float *w, int cout, int ks, int stride, int mode, int pad_y, int pad_x,
              const float *bias, const void *res, int relu, void *y, void *workspace, void *stream)
{
    return hh_conv2d_dt(HH_ACT_BF16, x, B, H, W, cin, w, cout, ks, stride, mode, pad_y, pad_x, bias, res, relu, y, workspace, stream);
}

int hh_conv2d_packed_dt(int act_dtype, const void *x, int B, int H, int W, int cin, const void *w_packed, int cout, int ks, int stride, int mode,
                        int pad_y, int pad_x, const float *bias, const void *res, int relu, void *y, void *stream)
{
    if (!w_packed) { hh_set_error("hh_conv2d_packed: bad argument"); return 1; }
    return conv2d_impl(act_dtype, x, B, H, W, cin, nullptr, (const bf16_raw *)w_packed, cout, ks, stride, mode, pad_y, pad_x, bias, res, relu, y,
                       nullptr, stream, "hh_conv2d_packed");
}
int hh_conv2d_packed(const void *x, int B, int H, int W, int cin, const void *w_packed, int cout, int ks, int stride, int mode, int pad_y,
                     int pad_x, const float *bias, const void *res, int relu, void *y, void *stream)
{
    return hh_conv2d_packed_dt(HH_ACT_BF16, x, B, H, W, cin, w_packed, cout, ks, stride, mode, pad_y, pad_x, bias, res, relu, y, stream);
}

int64_t hh_conv2d_packed_elems(int cin, int cout, int ks, int stride, int mode)
{
    Conv2dPlan pl;
    if (conv2d_plan(cin, cout, ks, stride, mode, &pl, "hh_conv2d_packed_elems")) return -1;
    return (int64_t)(pl.wel * pl.nsets);
}

int hh_pack_conv_weights_batch(int n, const float *const *w, void *const *packed, const int32_t *shapes, void *descs_dev, void *stream)
{
    return hh_pack_conv_weights_batch_dt(HH_ACT_BF16, n, w, packed, shapes, descs_dev, stream);
}
int hh_pack_conv_weights_batch_dt(int act_dtype, int n, const float *const *w, void *const *packed, const int32_t *shapes, void *descs_dev,
                                  void *stream)
{
    if (!act_dtype_ok(act_dtype, "hh_pack_conv_weights_batch")) return 1;
    if (n < 0 || (n && (!w || !packed || !shapes || !descs_dev))) { hh_set_error("hh_pack_conv_weights_batch: bad argument"); return 1; }
    std::vector<PackDesc> d;
    d.reserve((size_t)n * 4);
    for (int i = 0; i < n; ++i) {
        const int cout = shapes[5 * i], cin = shapes[5 * i + 1], ks = shapes[5 * i + 2], stride = shapes[5 * i + 3], mode = shapes[5 * i + 4];
        Conv2dPlan pl;
        if (!w[i] || !packed[i] || conv2d_plan(cin, cout, ks, stride, mode, &pl, "hh_pack_conv_weights_batch")) {
            if (w[i] && packed[i]) return 1;
            hh_set_error("hh_pack_conv_weights_batch: null pointer in the table");
            return 1;
        }
        for (int ph = 0; ph < pl.nsets; ++ph) {
            PackDesc e{};
            e.W = w[i]; e.packed = (bf16_raw *)packed[i] + (size_t)ph * pl.wel; e.total = (long long)pl.wel;
            e.cout = cout; e.cin = cin; e.ks = pl.kks; e.mode = mode; e.KC = pl.KC; e.COUT_T = pl.COUT_T; e.py = ph >> 1; e.px = ph & 1;
            d.push_back(e);
        }
    }
    if (d.empty()) return 0;
    // (pageable source: the copy is staged before hipMemcpyAsync returns, so the vector may go)
    HH_CHECK_HIP(hipMemcpyAsync(descs_dev, d.data(), d.size() * sizeof(PackDesc), hipMemcpyHostToDevice, (hipStream_t)stream));
    HH_CHECK_HIP(launch_pack_weights_batch((const PackDesc *)descs_dev, (int)d.size(), (hipStream_t)stream, act_dtype));
    return 0;
}

int64_t hh_conv2d_wgrad_workspace_bytes(int B, int H, int W, int cin, int cout, int ks, int stride)
{
    const int Ho = stride == 2 ? H / 2 : H, Wo = stride == 2 ? W / 2 : W;
    // one partial-sum set [ks*ks][cout64][cin64] per worker; the reduction combines them in LDS (no staging rows since round 3)
    return (int64_t)conv_wgrad_num_workers(B, Ho, Wo, ks, stride, cin, cout) * ks * ks * round_up_i(cout, 64) * round_up_i(cin, 64) * 4;
}

// the shape checks of hh_conv2d_wgrad; -> 0 and the output map, or 1 with the error set
static int wgrad_shape(int B, int H, int W, int cin, int cout, int ks, int stride, int *Ho, int *Wo)
{
    if (B <= 0 || H <= 0 || W <= 0) { hh_set_error("hh_conv2d_wgrad: bad argument"); return 1; }
    if (cin <= 0 || cout <= 0 || cin % 8 || cout % 8) { hh_set_error("hh_conv2d_wgrad: channel counts must be multiples of 8"); return 1; }
    *Ho = stride == 2 ? H / 2 : H; *Wo = stride == 2 ? W / 2 : W;
    if (conv_wgrad_variant(ks, stride, *Wo, cin, cout) < 0) { hh_set_error("hh_conv2d_wgrad: 3x3 (stride 1 or 2), 2x2 and 1x1 (stride 1) only"); return 1; }
    return 0;
}

int hh_conv2d_wgrad_plan(int B, int H, int W, int cin, int cout, int ks, int stride, int out[3])
{
    int Ho, Wo;
    if (!out || wgrad_shape(B, H, W, cin, cout, ks, stride, &Ho, &Wo)) return 1;
    out[0] = conv_wgrad_variant(ks, stride, Wo, cin, cout);
    out[1] = conv_wgrad_num_workers(B, Ho, Wo, ks, stride, cin, cout);
    out[2] = conv_wgrad_num_tiles(B, Ho, Wo, out[0]);
    return 0;
}

int hh_conv2d_wgrad_dt(int act_dtype, const void *x, const void *dy, int B, int H, int W, int cin, int cout, int ks, int stride, int pad_y, int pad_x,
                       float *dw, void *workspace, void *stream)
{
    if (!act_dtype_ok(act_dtype, "hh_conv2d_wgrad")) return 1;
    if (pad_y < 0) pad_y = (ks - 1) / 2;
    if (pad_x < 0) pad_x = (ks - 1) / 2;
    if (!x || !dy || !dw || !workspace) { hh_set_error("hh_conv2d_wgrad: bad argument"); return 1; }
    int Ho_, Wo_;
    if (wgrad_shape(B, H, W, cin, cout, ks, stride, &Ho_, &Wo_)) return 1;
    WgradParams p{};
    p.x = (const bf16_raw *)x; p.dy = (const bf16_raw *)dy; p.partial = (float *)workspace;
    p.B = B; p.H = H; p.W = W; p.Ho = Ho_; p.Wo = Wo_; p.cin = cin; p.cout = cout;
    p.pad_y = pad_y; p.pad_x = pad_x;
    HH_CHECK_HIP(conv_wgrad_launch(p, ks, stride, dw, (hipStream_t)stream, act_dtype));
    return 0;
}
int hh_conv2d_wgrad(const void *x, const void *dy, int B, int H, int W, int cin, int cout, int ks, int stride, int pad_y, int pad_x, float *dw,
                    void *workspace, void *stream)
{
    return hh_conv2d_wgrad_dt(HH_ACT_BF16, x, dy, B, H, W, cin, cout, ks, stride, pad_y, pad_x, dw, workspace, stream);
}

int hh_bn_train_forward_dt(int act_dtype, const void *x, int64_t P, int C, const float *gamma, const float *beta, float eps, const void *res,
                           int relu, void *y, float *mean, float *invstd, double *scratch, void *stream)
{
    if (!act_dtype_ok(act_dtype, "hh_bn_train_forward")) return 1;
    if (!x || !y || !gamma || !beta || !mean || !invstd || !scratch || P <= 0 || C <= 0 || C % 8 || C > 2048) { hh_set_error("hh_bn_train_forward: bad argument (C must be a multiple of 8, <= 2048)"); return 1; }
    HH_CHECK_HIP(launch_bn_train_forward((const bf16_raw *)x, C, (size_t)P, C, gamma, beta, eps, (const bf16_raw *)res, relu, (bf16_raw *)y,
                                         mean, invstd, scratch, (hipStream_t)stream, act_dtype));
    return 0;
}
int hh_bn_train_forward(const void *x, int64_t P, int C, const float *gamma, const float *beta, float eps, const void *res, int relu, void *y,
                        float *mean, float *invstd, double *scratch, void *stream)
{
    return hh_bn_train_forward_dt(HH_ACT_BF16, x, P, C, gamma, beta, eps, res, relu, y, mean, invstd, scratch, stream);
}

int hh_bn_train_backward_dt(int act_dtype, const void *x, const void *y, const void *dy, int64_t P, int C, const float *mean, const float *invstd,
                            const float *gamma, int relu, void *dx, void *dres, float *dgamma, float *dbeta, double *scratch, void *stream)
{
    if (!act_dtype_ok(act_dtype, "hh_bn_train_backward")) return 1;
    if (!x || !y || !dy || !dx || !mean || !invstd || !gamma || !dgamma || !dbeta || !scratch || P <= 0 || C <= 0 || C % 8 || C > 2048) { hh_set_error("hh_bn_train_backward: bad argument"); return 1; }
    HH_CHECK_HIP(launch_bn_train_backward((const bf16_raw *)x, (const bf16_raw *)y, (const bf16_raw *)dy, C, (size_t)P, C, mean, invstd, gamma,
                                          nullptr, relu, (bf16_raw *)dx, (bf16_raw *)dres, dgamma, dbeta, scratch, (hipStream_t)stream, act_dtype));
    return 0;
}
int hh_bn_train_backward(const void *x, const void *y, const void *dy, int64_t P, int C, const float *mean, const float *invstd, const float *gamma,
                         int relu, void *dx, void *dres, float *dgamma, float *dbeta, double *scratch, void *stream)
{
    return hh_bn_train_backward_dt(HH_ACT_BF16, x, y, dy, P, C, mean, invstd, gamma, relu, dx, dres, dgamma, dbeta, scratch, stream);
}

int hh_bn_train_backward_plain_dt(int act_dtype, const void *x, const void *dy, int64_t P, int C, const float *mean, const float *invstd,
                                  const float *gamma, const float *beta, int relu, void *dx, float *dgamma, float *dbeta, double *scratch, void *stream)
{
    if (!act_dtype_ok(act_dtype, "hh_bn_train_backward_plain")) return 1;
    if (!x || !dy || !dx || !mean || !invstd || !gamma || !beta || !dgamma || !dbeta || !scratch || P <= 0 || C <= 0 || C % 8 || C > 2048) { hh_set_error("hh_bn_train_backward_plain: bad argument"); return 1; }
    HH_CHECK_HIP(launch_bn_train_backward((const bf16_raw *)x, nullptr, (const bf16_raw *)dy, C, (size_t)P, C, mean, invstd, gamma, beta, relu,
                                          (bf16_raw *)dx, nullptr, dgamma, dbeta, scratch, (hipStream_t)stream, act_dtype));
    return 0;
}
int hh_bn_train_backward_plain(const void *x, const void *dy, int64_t P, int C, const float *mean, const float *invstd, const float *gamma,
                               const float *beta, int relu, void *dx, float *dgamma, float *dbeta, double *scratch, void *stream)
{
    return hh_bn_train_backward_plain_dt(HH_ACT_BF16, x, dy, P, C, mean, invstd, gamma, beta, relu, dx, dgamma, dbeta, scratch, stream);
}

int hh_fusion_sum_forward_dt(int act_dtype, const void *const *terms, const int *shifts, int nterms, int B, int H, int W, int C, int relu, void *out,
                             void *stream)
{
    if (!act_dtype_ok(act_dtype, "hh_fusion_sum_forward")) return 1;
    if (!terms || !shifts || nterms < 1 || nterms > 4 || !out || B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 || shifts[0] != 0) { hh_set_error("hh_fusion_sum_forward: 1..4 terms, the first at the output resolution, C a multiple of 8"); return 1; }
    UpAddParams p{};
    p.base = (const bf16_raw *)terms[0]; p.base_cs = C;
    p.nup = nterms - 1;
    for (int j = 1; j < nterms; ++j) {
        if (shifts[j] < 0 || shifts[j] > 5 || (H >> shifts[j]) << shifts[j] != H || (W >> shifts[j]) << shifts[j] != W) { hh_set_error("hh_fusion_sum_forward: bad shift"); return 1; }
        p.up[j - 1] = (const bf16_raw *)terms[j]; p.up_cs[j - 1] = C; p.up_shift[j - 1] = shifts[j];
    }
    p.out = (bf16_raw *)out; p.out_cs = C;
    p.B = B; p.H = H; p.W = W; p.C = C; p.relu = relu;
    HH_CHECK_HIP(launch_upadd(p, (hipStream_t)stream, act_dtype));
    return 0;
}
int hh_fusion_sum_forward(const void *const *terms, const int *shifts, int nterms, int B, int H, int W, int C, int relu, void *out, void *stream)
{
    return hh_fusion_sum_forward_dt(HH_ACT_BF16, terms, shifts, nterms, B, H, W, C, relu, out, stream);
}
int hh_fusion_sum_backward_dt(int act_dtype, const void *dy, const void *out, int relu, int B, int H, int W, int C, void *g, void *const *dup,
                              const int *up_shift, int nup, void *stream)
{
    if (!act_dtype_ok(act_dtype, "hh_fusion_sum_backward")) return 1;
    if (!dy || (relu && (!out || !g)) || nup < 0 || nup > 3 || B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8) { hh_set_error("hh_fusion_sum_backward: bad argument"); return 1; }
    HH_CHECK_HIP(launch_upadd_backward((const bf16_raw *)dy, (const bf16_raw *)out, relu, B, H, W, C, (bf16_raw *)g, (bf16_raw *const *)dup, up_shift, nup,
                                       (hipStream_t)stream, act_dtype));
    return 0;
}
int hh_fusion_sum_backward(const void *dy, const void *out, int relu, int B, int H, int W, int C, void *g, void *const *dup, const int *up_shift,
                           int nup, void *stream)
{
    return hh_fusion_sum_backward_dt(HH_ACT_BF16, dy, out, relu, B, H, W, C, g, dup, up_shift, nup, stream);
}

static bool bn_dims_ok(int64_t P, int C) { return P > 0 && C > 0 && C % 8 == 0 && C <= 2048; }

int hh_bn_train_stats_dt(int act_dtype, const void *x, int64_t P, int C, double *sums, double *scratch, void *stream)
{
    if (!act_dtype_ok(act_dtype, "hh_bn_train_stats")) return 1;
    if (!x || !sums || !scratch || !bn_dims_ok(P, C)) { hh_set_error("hh_bn_train_stats: bad argument (C must be a multiple of 8, <= 2048)"); return 1; }
    HH_CHECK_HIP(launch_bn_train_stats((const bf16_raw *)x, C, (size_t)P, C, sums, scratch, (hipStream_t)stream, act_dtype));
    return 0;
}
int hh_bn_train_stats(const void *x, int64_t P, int C, double *sums, double *scratch, void *stream)
{
    return hh_bn_train_stats_dt(HH_ACT_BF16, x, P, C, sums, scratch, stream);
}

int hh_bn_train_normalize_dt(int act_dtype, const void *x, int64_t P, int C, const double *sums, double count, const float *gamma, const float *beta,
                             float eps, const void *res, int relu, void *y, float *mean, float *invstd, void *stream)
{
    if (!act_dtype_ok(act_dtype, "hh_bn_train_normalize")) return 1;
    if (!x || !y || !sums || !gamma || !beta || !mean || !invstd || !bn_dims_ok(P, C) || !(count >= (double)P)) { hh_set_error("hh_bn_train_normalize: bad argument (count = pixels of all ranks >= P)"); return 1; }
    HH_CHECK_HIP(launch_bn_train_normalize((const bf16_raw *)x, C, (size_t)P, C, sums, count, gamma, beta, eps, (const bf16_raw *)res, relu,
                                           (bf16_raw *)y, mean, invstd, (hipStream_t)stream, act_dtype));
    return 0;
}
int hh_bn_train_normalize(const void *x, int64_t P, int C, const double *sums, double count, const float *gamma, const float *beta, float eps,
                          const void *res, int relu, void *y, float *mean, float *invstd, void *stream)
{
    return hh_bn_train_normalize_dt(HH_ACT_BF16, x, P, C, sums, count, gamma, beta, eps, res, relu, y, mean, invstd, stream);
}

int hh_bn_train_backward_stats_dt(int act_dtype, const void *x, const void *y, const void *dy, int64_t P, int C, const float *mean,
                                  const float *invstd, int relu, double *sums, float *dgamma, float *dbeta, double *scratch, void *stream)
{
    if (!act_dtype_ok(act_dtype, "hh_bn_train_backward_stats")) return 1;
    if (!x || !y || !dy || !mean || !invstd || !sums || !dgamma || !dbeta || !scratch || !bn_dims_ok(P, C)) { hh_set_error("hh_bn_train_backward_stats: bad argument"); return 1; }
    HH_CHECK_HIP(launch_bn_train_backward_stats((const bf16_raw *)x, (const bf16_raw *)y, (const bf16_raw *)dy, C, (size_t)P, C, mean, invstd,
                                                relu, sums, dgamma, dbeta, scratch, (hipStream_t)stream, act_dtype));
    return 0;
}
int hh_bn_train_backward_stats(const void *x, const void *y, const void *dy, int64_t P, int C, const float *mean, const float *invstd, int relu,
                               double *sums, float *dgamma, float *dbeta, double *scratch, void *stream)
{
    return hh_bn_train_backward_stats_dt(HH_ACT_BF16, x, y, dy, P, C, mean, invstd, relu, sums, dgamma, dbeta, scratch, stream);
}

int hh_bn_train_backward_apply_dt(int act_dtype, const void *x, const void *y, const void *dy, int64_t P, int C, const float *mean,
                                  const float *invstd, const float *gamma, int relu, const double *sums, double count, void *dx, void *dres, double *scratch,
                                  void *stream)
{
    if (!act_dtype_ok(act_dtype, "hh_bn_train_backward_apply")) return 1;
    if (!x || !y || !dy || !dx || !mean || !invstd || !gamma || !sums || !scratch || !bn_dims_ok(P, C) || !(count >= (double)P)) { hh_set_error("hh_bn_train_backward_apply: bad argument"); return 1; }
    HH_CHECK_HIP(launch_bn_train_backward_apply((const bf16_raw *)x, (const bf16_raw *)y, (const bf16_raw *)dy, C, (size_t)P, C, mean, invstd,
                                                gamma, relu, sums, count, (bf16_raw *)dx, (bf16_raw *)dres, scratch, (hipStream_t)stream, act_dtype));
    return 0;
}
int hh_bn_train_backward_apply(const void *x, const void *y, const void *dy, int64_t P, int C, const float *mean, const float *invstd,
                               const float *gamma, int relu, const double *sums, double count, void *dx, void *dres, double *scratch, void *stream)
{
    return hh_bn_train_backward_apply_dt(HH_ACT_BF16, x, y, dy, P, C, mean, invstd, gamma, relu, sums, count, dx, dres, scratch, stream);
}

// ------------------------------------------------------------------ the classifier's tail in training form (cls_tail.hip)
int hh_global_avgpool_act(int act_dtype, const void *x, int B, int HW, int C, float *out, void *stream)
{
    if (!act_dtype_ok(act_dtype, "hh_global_avgpool")) return 1;
    if (!x || !out || B <= 0 || HW <= 0 || C <= 0 || C % 8) { hh_set_error("hh_global_avgpool: bad argument (C must be a multiple of 8)"); return 1; }
    HH_CHECK_HIP(launch_avgpool((const bf16_raw *)x, C, out, B, HW, C, (hipStream_t)stream, act_dtype));
    return 0;
}
int hh_global_avgpool(const void *x, int B, int HW, int C, float *out, void *stream) { return hh_global_avgpool_act(HH_ACT_BF16, x, B, HW, C, out, stream); }

int hh_global_avgpool_backward_act(int act_dtype, const float *g, int B, int HW, int C, void *dx, void *stream)
{
    if (!act_dtype_ok(act_dtype, "hh_global_avgpool_backward")) return 1;
    if (!g || !dx || B <= 0 || HW <= 0 || C <= 0 || C % 8) { hh_set_error("hh_global_avgpool_backward: bad argument (C must be a multiple of 8)"); return 1; }
    HH_CHECK_HIP(launch_avgpool_backward(g, (bf16_raw *)dx, B, HW, C, (hipStream_t)stream, act_dtype));
    return 0;
}
int hh_global_avgpool_backward(const float *g, int B, int HW, int C, void *dx, void *stream)
{
    return hh_global_avgpool_backward_act(HH_ACT_BF16, g, B, HW, C, dx, stream);
}

int hh_linear_forward(const float *x, const float *w, const float *bias, int B, int K, int N, float *y, void *stream)
{
    if (!x || !w || !bias || !y || B <= 0 || B > 65535 || K <= 0 || N <= 0) { hh_set_error("hh_linear_forward: bad argument (0 < B <= 65535)"); return 1; }
    HH_CHECK_HIP(launch_linear(x, w, bias, y, B, K, N, (hipStream_t)stream));
    return 0;
}
int hh_linear_backward(const float *x, const float *w, const float *dy, int B, int K, int N, float *dx, float *dw, float *db, void *stream)
{
    if (!dy || (dx && !w) || (dw && !x) || B <= 0 || K <= 0 || N <= 0 || N > 65535 || (B + 7) / 8 > 65535) { hh_set_error("hh_linear_backward: bad argument (0 < N <= 65535)"); return 1; }
    HH_CHECK_HIP(launch_linear_backward(x, w, dy, B, K, N, dx, dw, db, (hipStream_t)stream));
    return 0;
}

int hh_softmax_xent(const float *logits, const int64_t *targets, int B, int N, float *dlogits, hh_xent_result *result, void *stream)
{
    static_assert(sizeof(long long) == sizeof(int64_t), "targets");
    if (!logits || !targets || !result || B <= 0 || N <= 0) { hh_set_error("hh_softmax_xent: bad argument"); return 1; }
    HH_CHECK_HIP(launch_softmax_xent(logits, (const long long *)targets, B, N, dlogits, result, (hipStream_t)stream));
    return 0;
}

// ---- device optimizer step (optim.hip).  Table layout in table_dev: [tensors][chunks][groups], each 8-byte aligned.
static_assert(sizeof(OptimChunk) == 8, "chunk list layout");

// the checks every entry point shares; -> the chunk count, or -1 with the error set
static int64_t optim_count_chunks(const hh_optim_tensor *t, int ntensors, int ngroups, const char *who)
{
    if (ntensors < 0 || ngroups <= 0) { hh_set_error(std::string(who) + ": need ntensors >= 0 and ngroups > 0"); return -1; }
    if (ntensors && !t) { hh_set_error(std::string(who) + ": null tensor table"); return -1; }
    int64_t nchunks = 0;
    for (int i = 0; i < ntensors; ++i) {
        if (t[i].numel < 0) { hh_set_error(std::string(who) + ": negative numel in the table"); return -1; }
        if (t[i].group < 0 || t[i].group >= ngroups) { hh_set_error(std::string(who) + ": group index outside [0, ngroups)"); return -1; }
        nchunks += (t[i].numel + OPTIM_CHUNK - 1) / OPTIM_CHUNK;
    }
    if (nchunks > 0x7fffffffLL) { hh_set_error(std::string(who) + ": more than 2^31 - 1 chunks"); return -1; }
    return nchunks;
}

static int64_t optim_bytes(int ntensors, int ngroups, int64_t nchunks)
{
    return (int64_t)ntensors * (int64_t)sizeof(OptimTensor) + nchunks * (int64_t)sizeof(OptimChunk) + (int64_t)ngroups * (int64_t)sizeof(OptimGroup);
}

int64_t hh_optim_table_bytes(const hh_optim_tensor *tensors_host, int ntensors, int ngroups)
{
    const int64_t nchunks = optim_count_chunks(tensors_host, ntensors, ngroups, "hh_optim_table_bytes");
    return nchunks < 0 ? -1 : optim_bytes(ntensors, ngroups, nchunks);
}

// Builds the host image of the table parts `upload` names and ships it with one async copy (the parts are adjacent in the order
// tensors, chunks, groups, so bit 0 and bit 1 together are still one copy).
static int optim_upload(const hh_optim_tensor *t, int ntensors, const hh_optim_group *groups, int ngroups, int64_t nchunks, int upload,
                        char *table_dev, hipStream_t stream)
{
    if (!upload) return 0;
    // (thread-local and reused: it outlives the call, and the next call on this thread comes after the copy has been staged)
    static thread_local std::vector<char> host;
    const size_t tb = (size_t)ntensors * sizeof(OptimTensor), cb = (size_t)nchunks * sizeof(OptimChunk), gb = (size_t)ngroups * sizeof(OptimGroup);
    host.resize(tb + cb + gb);
    size_t lo = tb + cb, hi = tb + cb;
    if (upload & HH_OPTIM_UPLOAD_TENSORS) {
        lo = 0;
        if (tb) std::memcpy(host.data(), t, tb);
        OptimChunk *c = (OptimChunk *)(host.data() + tb);
        for (int i = 0; i < ntensors; ++i) {
            const int n = (int)((t[i].numel + OPTIM_CHUNK - 1) / OPTIM_CHUNK);
            for (int k = 0; k < n; ++k) *c++ = OptimChunk{i, k};
        }
    }
    if (upload & HH_OPTIM_UPLOAD_GROUPS) {
        hi = tb + cb + gb;
        std::memcpy(host.data() + tb + cb, groups, gb);
    }
    if (hi > lo) HH_CHECK_HIP(hipMemcpyAsync(table_dev + lo, host.data() + lo, hi - lo, hipMemcpyHostToDevice, stream));
    return 0;
}

// the checks of hh_optim_step (and of hh_optim_step_ema, which steps the same table); -> the chunk count, or -1 with the error set
static int64_t optim_step_check(const char *who, int algo, const hh_optim_tensor *tensors_host, int ntensors, const hh_optim_group *groups_host,
                                int ngroups, const void *table_dev, int64_t table_bytes, int upload)
{
    const std::string w(who);
    if (algo != HH_OPTIM_ADAM && algo != HH_OPTIM_ADAMW && algo != HH_OPTIM_SGD) { hh_set_error(w + ": unknown algorithm (HH_OPTIM_ADAM = 0, HH_OPTIM_ADAMW = 1, HH_OPTIM_SGD = 2)"); return -1; }
    if (!groups_host || !table_dev) { hh_set_error(w + ": null group table or device table"); return -1; }
    if (upload < 0 || upload > HH_OPTIM_UPLOAD_ALL) { hh_set_error(w + ": upload is a mask of HH_OPTIM_UPLOAD_TENSORS | HH_OPTIM_UPLOAD_GROUPS"); return -1; }
    if ((uintptr_t)table_dev % 16) { hh_set_error(w + ": table_dev must be 16-byte aligned"); return -1; }
    const int64_t nchunks = optim_count_chunks(tensors_host, ntensors, ngroups, who);
    if (nchunks < 0) return -1;
    if (table_bytes < optim_bytes(ntensors, ngroups, nchunks)) { hh_set_error(w + ": table buffer too small (hh_optim_table_bytes)"); return -1; }
    const bool adam = algo != HH_OPTIM_SGD;
    for (int g = 0; g < ngroups; ++g) {
        const hh_optim_group &gr = groups_host[g];
        if (adam && !(gr.beta1 >= 0.0 && gr.beta1 < 1.0 && gr.beta2 >= 0.0 && gr.beta2 < 1.0)) { hh_set_error(w + ": betas must lie in [0, 1)"); return -1; }
    }
    for (int i = 0; i < ntensors; ++i) {
        const hh_optim_tensor &t = tensors_host[i];
        const bool need_s0 = adam || groups_host[t.group].momentum != 0.0;
        if (!t.param || !t.grad || (need_s0 && !t.state0) || (adam && (!t.state1 || !t.step))) { hh_set_error(w + ": null pointer in the tensor table"); return -1; }
    }
    return nchunks;
}

int hh_optim_step(int algo, const hh_optim_tensor *tensors_host, int ntensors, const hh_optim_group *groups_host, int ngroups,
                  const float *grad_scale, const float *found_inf, void *table_dev, int64_t table_bytes, int upload, void *stream)
{
    const int64_t nchunks = optim_step_check("hh_optim_step", algo, tensors_host, ntensors, groups_host, ngroups, table_dev, table_bytes, upload);
    if (nchunks < 0) return 1;
    if (!nchunks) return 0;
    if (optim_upload(tensors_host, ntensors, groups_host, ngroups, nchunks, upload, (char *)table_dev, (hipStream_t)stream)) return 1;
    const OptimTensor *td = (const OptimTensor *)table_dev;
    const OptimChunk *cd = (const OptimChunk *)(td + ntensors);
    const OptimGroup *gd = (const OptimGroup *)(cd + nchunks);
    HH_CHECK_HIP(launch_optim_step(algo, td, ntensors, gd, cd, (int)nchunks, grad_scale, found_inf, algo != HH_OPTIM_SGD ? 1 : 0, (hipStream_t)stream));
    return 0;
}

// ---- weight EMA (ema.hip).  Table layout in the EMA table: [rows][chunks][row_of: one int per optimizer tensor].  The chunk list is of
// all rows (hh_ema_update, hh_ema_swap) or of the rows no optimizer tensor names (hh_optim_step_ema); the buffer is sized for all.

// -> the chunk count of all rows, or -1 with the error set
static int64_t ema_count_chunks(const char *who, const hh_ema_row *rows, int nrows)
{
    const std::string w(who);
    if (nrows < 0) { hh_set_error(w + ": need nrows >= 0"); return -1; }
    if (nrows && !rows) { hh_set_error(w + ": null row table"); return -1; }
    int64_t nchunks = 0;
    for (int i = 0; i < nrows; ++i) {
        if (rows[i].numel < 0) { hh_set_error(w + ": negative numel in the row table"); return -1; }
        if (!rows[i].value || !rows[i].ema) { hh_set_error(w + ": null pointer in the row table"); return -1; }
        nchunks += (rows[i].numel + OPTIM_CHUNK - 1) / OPTIM_CHUNK;
    }
    if (nchunks > 0x7fffffffLL) { hh_set_error(w + ": more than 2^31 - 1 chunks"); return -1; }
    return nchunks;
}

static int64_t ema_bytes(int nrows, int64_t nchunks, int ntensors)
{
    return (int64_t)nrows * (int64_t)sizeof(EmaRow) + nchunks * (int64_t)sizeof(OptimChunk) + (int64_t)ntensors * (int64_t)sizeof(int);
}

// the checks the three entry points share; -> the chunk count of all rows, or -1 with the error set
static int64_t ema_check(const char *who, const hh_ema_row *rows, int nrows, int ntensors, const void *table_dev, int64_t table_bytes)
{
    const std::string w(who);
    if (!table_dev) { hh_set_error(w + ": null EMA device table"); return -1; }
    if ((uintptr_t)table_dev % 16) { hh_set_error(w + ": the EMA device table must be 16-byte aligned"); return -1; }
    const int64_t nchunks = ema_count_chunks(who, rows, nrows);
    if (nchunks < 0) return -1;
    if (table_bytes < ema_bytes(nrows, nchunks, ntensors)) { hh_set_error(w + ": EMA table buffer too small (hh_ema_table_bytes)"); return -1; }
    return nchunks;
}

static bool ema_decay_ok(const char *who, double decay, const int64_t *n_averaged)
{
    if (!(decay >= 0.0 && decay <= 1.0)) { hh_set_error(std::string(who) + ": decay must lie in [0, 1]"); return false; }
    if (!n_averaged) { hh_set_error(std::string(who) + ": null n_averaged"); return false; }
    return true;
}

// Ships [rows][chunks of the rows with skip[row] == 0][row_of] with one async copy; -> the number of chunks listed, -1 on a HIP error.
// `nall` is the chunk count of all rows: row_of sits behind room for that many, whatever is listed.
static int64_t ema_upload(const hh_ema_row *rows, int nrows, const char *skip, const int32_t *row_of, int ntensors, int64_t nall, int upload,
                          char *table_dev, hipStream_t stream)
{
    int64_t listed = 0;
    for (int i = 0; i < nrows; ++i)
        if (!skip || !skip[i]) listed += (rows[i].numel + OPTIM_CHUNK - 1) / OPTIM_CHUNK;
    if (!upload) return listed;
    static thread_local std::vector<char> host;
    const size_t rb = (size_t)nrows * sizeof(EmaRow), cb = (size_t)nall * sizeof(OptimChunk), ib = (size_t)ntensors * sizeof(int);
    host.assign(rb + cb + ib, 0);
    if (rb) std::memcpy(host.data(), rows, rb);
    OptimChunk *c = (OptimChunk *)(host.data() + rb);
    for (int i = 0; i < nrows; ++i) {
        if (skip && skip[i]) continue;
        const int n = (int)((rows[i].numel + OPTIM_CHUNK - 1) / OPTIM_CHUNK);
        for (int k = 0; k < n; ++k) *c++ = OptimChunk{i, k};
    }
    if (ib) std::memcpy(host.data() + rb + cb, row_of, ib);
    if (!host.empty() && hipMemcpyAsync(table_dev, host.data(), host.size(), hipMemcpyHostToDevice, stream) != hipSuccess) {
        hh_set_error("hipMemcpyAsync of the EMA table failed");
        return -1;
    }
    return listed;
}

int64_t hh_ema_table_bytes(const hh_ema_row *rows_host, int nrows, int ntensors)
{
    if (ntensors < 0) { hh_set_error("hh_ema_table_bytes: need ntensors >= 0"); return -1; }
    const int64_t nchunks = ema_count_chunks("hh_ema_table_bytes", rows_host, nrows);
    return nchunks < 0 ? -1 : ema_bytes(nrows, nchunks, ntensors);
}

int hh_ema_update(const hh_ema_row *rows_host, int nrows, double decay, int warmup, int64_t *n_averaged, const float *found_inf, void *table_dev,
                  int64_t table_bytes, int upload, void *stream)
{
    if (!ema_decay_ok("hh_ema_update", decay, n_averaged)) return 1;
    const int64_t nall = ema_check("hh_ema_update", rows_host, nrows, 0, table_dev, table_bytes);
    if (nall < 0) return 1;
    if (ema_upload(rows_host, nrows, nullptr, nullptr, 0, nall, upload, (char *)table_dev, (hipStream_t)stream) < 0) return 1;
    const EmaRow *rd = (const EmaRow *)table_dev;
    HH_CHECK_HIP(launch_ema_update(rd, (const OptimChunk *)(rd + nrows), (int)nall, decay, warmup != 0, (long long *)n_averaged, found_inf,
                                   (hipStream_t)stream));
    return 0;
}

int hh_ema_swap(const hh_ema_row *rows_host, int nrows, void *table_dev, int64_t table_bytes, int upload, void *stream)
{
    const int64_t nall = ema_check("hh_ema_swap", rows_host, nrows, 0, table_dev, table_bytes);
    if (nall < 0) return 1;
    if (ema_upload(rows_host, nrows, nullptr, nullptr, 0, nall, upload, (char *)table_dev, (hipStream_t)stream) < 0) return 1;
    const EmaRow *rd = (const EmaRow *)table_dev;
    HH_CHECK_HIP(launch_ema_swap(rd, (const OptimChunk *)(rd + nrows), (int)nall, (hipStream_t)stream));
    return 0;
}

int hh_optim_step_ema(int algo, const hh_optim_tensor *tensors_host, int ntensors, const hh_optim_group *groups_host, int ngroups,
                      const float *grad_scale, const float *found_inf, void *table_dev, int64_t table_bytes, int upload,
                      const hh_ema_row *rows_host, int nrows, const int32_t *row_of_tensor, double decay, int warmup, int64_t *n_averaged,
                      void *ema_table_dev, int64_t ema_table_bytes, int ema_upload_flag, void *stream)
{
    const char *who = "hh_optim_step_ema";
    const int64_t nchunks = optim_step_check(who, algo, tensors_host, ntensors, groups_host, ngroups, table_dev, table_bytes, upload);
    if (nchunks < 0) return 1;
    if (!ema_decay_ok(who, decay, n_averaged)) return 1;
    const int64_t nall = ema_check(who, rows_host, nrows, ntensors, ema_table_dev, ema_table_bytes);
    if (nall < 0) return 1;
    if (ntensors && !row_of_tensor) { hh_set_error("hh_optim_step_ema: null row_of_tensor"); return 1; }
    std::vector<char> named((size_t)nrows, 0);
    for (int i = 0; i < ntensors; ++i) {
        const int32_t r = row_of_tensor[i];
        if (r < -1 || r >= nrows) { hh_set_error("hh_optim_step_ema: row index outside [-1, nrows)"); return 1; }
        if (r < 0) continue;
        if (named[r]) { hh_set_error("hh_optim_step_ema: an EMA row is named by two tensors"); return 1; }
        named[r] = 1;
        if (rows_host[r].numel != tensors_host[i].numel) { hh_set_error("hh_optim_step_ema: an optimizer row and its EMA row differ in numel"); return 1; }
    }
    if (nchunks && optim_upload(tensors_host, ntensors, groups_host, ngroups, nchunks, upload, (char *)table_dev, (hipStream_t)stream)) return 1;
    const int64_t nonly = ema_upload(rows_host, nrows, named.data(), row_of_tensor, ntensors, nall, ema_upload_flag, (char *)ema_table_dev, (hipStream_t)stream);
    if (nonly < 0) return 1;
    const OptimTensor *td = (const OptimTensor *)table_dev;
    const OptimChunk *cd = (const OptimChunk *)(td + ntensors);
    const OptimGroup *gd = (const OptimGroup *)(cd + nchunks);
    const EmaRow *rd = (const EmaRow *)ema_table_dev;
    const OptimChunk *od = (const OptimChunk *)(rd + nrows);
    const int *row_of = (const int *)(od + nall);
    if (nchunks + nonly > 0x7fffffffLL) { hh_set_error("hh_optim_step_ema: more than 2^31 - 1 chunks"); return 1; }
    HH_CHECK_HIP(launch_optim_step_ema(algo, td, ntensors, gd, cd, (int)nchunks, grad_scale, found_inf, algo != HH_OPTIM_SGD ? 1 : 0, rd, row_of, od,
                                       (int)nonly, decay, warmup != 0, (long long *)n_averaged, (hipStream_t)stream));
    return 0;
}

int hh_grads_nonfinite(const hh_optim_tensor *tensors_host, int ntensors, int ngroups, const float *inv_scale, float *found_inf, void *table_dev,
                       int64_t table_bytes, int upload, void *stream)
{
    if (!found_inf || !table_dev) { hh_set_error("hh_grads_nonfinite: null found_inf or device table"); return 1; }
    if (upload != 0 && upload != HH_OPTIM_UPLOAD_TENSORS) { hh_set_error("hh_grads_nonfinite: upload is 0 or HH_OPTIM_UPLOAD_TENSORS"); return 1; }
    if ((uintptr_t)table_dev % 16) { hh_set_error("hh_grads_nonfinite: table_dev must be 16-byte aligned"); return 1; }
    const int64_t nchunks = optim_count_chunks(tensors_host, ntensors, ngroups, "hh_grads_nonfinite");
    if (nchunks < 0) return 1;
    if (table_bytes < optim_bytes(ntensors, ngroups, nchunks)) { hh_set_error("hh_grads_nonfinite: table buffer too small (hh_optim_table_bytes)"); return 1; }
    for (int i = 0; i < ntensors; ++i)
        if (!tensors_host[i].grad) { hh_set_error("hh_grads_nonfinite: null gradient pointer in the tensor table"); return 1; }
    if (!nchunks) return 0;
    if (optim_upload(tensors_host, ntensors, nullptr, ngroups, nchunks, upload, (char *)table_dev, (hipStream_t)stream)) return 1;
    const OptimTensor *td = (const OptimTensor *)table_dev;
    HH_CHECK_HIP(launch_grads_nonfinite(td, (const OptimChunk *)(td + ntensors), (int)nchunks, inv_scale, found_inf, (hipStream_t)stream));
    return 0;
}

// ---- gradient statistics and clipping by global norm (grad_stats.hip) on the same table; the workspace's layout is grad_work's.
static_assert(sizeof(GradPartial) == 24 && sizeof(GradTotals) == 16 && sizeof(GradRow) == 16, "grad_stats workspace layout");

// the checks hh_grad_stats and hh_grad_clip share, in hh_grads_nonfinite's order; -> the chunk count, or -1 with the error set
static int64_t grad_check(const char *who, const hh_optim_tensor *t, int ntensors, int ngroups, const void *table_dev, int64_t table_bytes,
                          const void *work_dev, int64_t work_bytes)
{
    const std::string w(who);
    if (!table_dev || !work_dev) { hh_set_error(w + ": null device table or workspace"); return -1; }
    if ((uintptr_t)table_dev % 16 || (uintptr_t)work_dev % 16) { hh_set_error(w + ": table_dev and work_dev must be 16-byte aligned"); return -1; }
    const int64_t nchunks = optim_count_chunks(t, ntensors, ngroups, who);
    if (nchunks < 0) return -1;
    if (table_bytes < optim_bytes(ntensors, ngroups, nchunks)) { hh_set_error(w + ": table buffer too small (hh_optim_table_bytes)"); return -1; }
    if (work_bytes < grad_work_bytes(ntensors, nchunks)) { hh_set_error(w + ": workspace too small (hh_grad_stats_bytes)"); return -1; }
    for (int i = 0; i < ntensors; ++i)
        if (!t[i].grad) { hh_set_error(w + ": null gradient pointer in the tensor table"); return -1; }
    return nchunks;
}

int64_t hh_grad_stats_bytes(const hh_optim_tensor *tensors_host, int ntensors, int ngroups)
{
    const int64_t nchunks = optim_count_chunks(tensors_host, ntensors, ngroups, "hh_grad_stats_bytes");
    return nchunks < 0 ? -1 : (int64_t)grad_work_bytes(ntensors, nchunks);
}

int hh_grad_stats(const hh_optim_tensor *tensors_host, int ntensors, int ngroups, const float *inv_scale, float *found_inf, void *table_dev,
                  int64_t table_bytes, int upload, void *work_dev, int64_t work_bytes, void *stream)
{
    if (inv_scale && !found_inf) { hh_set_error("hh_grad_stats: inv_scale needs found_inf (the unscale pass is the non-finite check)"); return 1; }
    if (upload != 0 && upload != HH_OPTIM_UPLOAD_TENSORS) { hh_set_error("hh_grad_stats: upload is 0 or HH_OPTIM_UPLOAD_TENSORS"); return 1; }
    const int64_t nchunks = grad_check("hh_grad_stats", tensors_host, ntensors, ngroups, table_dev, table_bytes, work_dev, work_bytes);
    if (nchunks < 0) return 1;
    if (nchunks && optim_upload(tensors_host, ntensors, nullptr, ngroups, nchunks, upload, (char *)table_dev, (hipStream_t)stream)) return 1;
    const OptimTensor *td = (const OptimTensor *)table_dev;
    HH_CHECK_HIP(launch_grad_stats(td, ntensors, (const OptimChunk *)(td + ntensors), (int)nchunks, inv_scale, found_inf, work_dev, (hipStream_t)stream));
    return 0;
}

int hh_grad_clip(const hh_optim_tensor *tensors_host, int ntensors, int ngroups, float max_norm, int norm_type, const float *found_inf,
                 void *table_dev, int64_t table_bytes, void *work_dev, int64_t work_bytes, void *stream)
{
    if (!(max_norm >= 0.0f)) { hh_set_error("hh_grad_clip: max_norm must be a number >= 0"); return 1; }
    if (norm_type != HH_GRAD_NORM_L2 && norm_type != HH_GRAD_NORM_INF) { hh_set_error("hh_grad_clip: unknown norm type (HH_GRAD_NORM_L2 = 0, HH_GRAD_NORM_INF = 1)"); return 1; }
    const int64_t nchunks = grad_check("hh_grad_clip", tensors_host, ntensors, ngroups, table_dev, table_bytes, work_dev, work_bytes);
    if (nchunks < 0) return 1;
    const OptimTensor *td = (const OptimTensor *)table_dev;
    HH_CHECK_HIP(launch_grad_clip(td, ntensors, (const OptimChunk *)(td + ntensors), (int)nchunks, max_norm, norm_type, found_inf, work_dev,
                                  (hipStream_t)stream));
    return 0;
}

int hh_flip_images(const float *images, float *out, int B, int C, int H, int W, void *stream)
{
    HH_CHECK_HIP(launch_flip_images(images, out, B, C, H, W, (hipStream_t)stream));
    return 0;
}

int hh_flip_merge(float *hm, int64_t hm_bstride, const float *hm_flipped, int64_t hmf_bstride, const float *tags_flipped,
                  int64_t tf_bstride, float *tags_out, int64_t to_bstride, const int32_t *perm_host, int B, int K, int h,
                  int w, void *stream)
{
    if (K > 64) { hh_set_error("hh_flip_merge: K > 64"); return 1; }
    for (int k = 0; k < K; ++k)
        if (perm_host[k] < 0 || perm_host[k] >= K) { hh_set_error("hh_flip_merge: perm is not a permutation of 0..K-1"); return 1; }
    HH_CHECK_HIP(launch_flip_merge(hm, hm_bstride, hm_flipped, hmf_bstride, tags_flipped, tf_bstride, tags_out, to_bstride,
                                   perm_host, B, K, h, w, (hipStream_t)stream));
    return 0;
}

// cv::solve(A, b, DECOMP_LU) for the 6x6 system of cv::getAffineTransform: OpenCV's own LU (matrix_decomp.cpp LUImpl: partial
// pivoting on the largest magnitude, first one wins; eliminate with alpha = A[j][i] * (-1 / A[i][i]); back-substitute), which is
// what hal::LU64f runs for matrices this small.  Every product and sum rounded on its own.
#pragma clang fp contract(off)
static int lu_solve6(double A[6][6], double b[6])
{
    const int m = 6;
    const double eps = 2.220446049250313e-16 * 100;
    for (int i = 0; i < m; ++i) {
        int k = i;
        for (int j = i + 1; j < m; ++j)
            if (std::fabs(A[j][i]) > std::fabs(A[k][i])) k = j;
        if (std::fabs(A[k][i]) < eps) return 1;
        if (k != i) {
            for (int j = i; j < m; ++j) std::swap(A[i][j], A[k][j]);
            std::swap(b[i], b[k]);
        }
        const double d = -1 / A[i][i];
        for (int j = i + 1; j < m; ++j) {
            const double alpha = A[j][i] * d;
            for (int c = i + 1; c < m; ++c) A[j][c] += alpha * A[i][c];
            b[j] += alpha * b[i];
        }
    }
    for (int i = m - 1; i >= 0; --i) {
        double sres = b[i];
        for (int k = i + 1; k < m; ++k) sres -= A[i][k] * b[k];
        b[i] = sres / A[i][i];
    }
    return 0;
}

int hh_get_affine_transform(double cx, double cy, double scale_w, double dst_w, double dst_h, int inverse, double out[6])
{
#pragma clang fp contract(off)
    // the three point pairs of get_affine_transform(center, scale, rot=0, output_size) as the reference's numpy code leaves them
    // in its float32 arrays (base/transforms/utils.py:37-53): [center, center + (0, -scale_w/2), third], [dst centre, dst centre +
    // (0, -dst_w/2), third]; third = b + (-(a-b).y, (a-b).x) in float32
    float src[3][2], dst[3][2];
    src[0][0] = (float)cx; src[0][1] = (float)cy;
    src[1][0] = (float)(cx + 0.0); src[1][1] = (float)(cy + (-scale_w / 2));
    const float dst_dir_y = (float)(-dst_w / 2);
    dst[0][0] = (float)(dst_w * 0.5); dst[0][1] = (float)(dst_h * 0.5);
    dst[1][0] = (float)(dst_w * 0.5 + 0.0); dst[1][1] = (float)(dst_h * 0.5 + (double)dst_dir_y);
    auto third = [](float p[3][2]) {
        const float dx = p[0][0] - p[1][0], dy = p[0][1] - p[1][1];
        p[2][0] = p[1][0] + (-dy);
        p[2][1] = p[1][1] + dx;
    };
    third(src); third(dst);
    float (*from)[2] = inverse ? dst : src, (*to)[2] = inverse ? src : dst;
    double A[6][6] = {}, b[6];
    for (int i = 0; i < 3; ++i) {  // cv::getAffineTransform (imgwarp.cpp): rows (x y 1 0 0 0), (0 0 0 x y 1)
        A[2 * i][0] = A[2 * i + 1][3] = from[i][0];
        A[2 * i][1] = A[2 * i + 1][4] = from[i][1];
        A[2 * i][2] = A[2 * i + 1][5] = 1;
        b[2 * i] = to[i][0];
        b[2 * i + 1] = to[i][1];
    }
    if (lu_solve6(A, b)) { hh_set_error("hh_get_affine_transform: degenerate point set (scale_w or dst_w is 0)"); return 1; }
    for (int i = 0; i < 6; ++i) out[i] = b[i];
    return 0;
}

int hh_invert_affine(const double m[6], double out[6])
{
#pragma clang fp contract(off)
    // cv::warpAffine without WARP_INVERSE_MAP (imgwarp.cpp), same order of operations
    double M[6];
    for (int i = 0; i < 6; ++i) M[i] = m[i];
    double D = M[0] * M[4] - M[1] * M[3];
    D = D != 0 ? 1. / D : 0;
    const double A11 = M[4] * D, A22 = M[0] * D;
    M[0] = A11; M[1] *= -D;
    M[3] *= -D; M[4] = A22;
    const double b1 = -M[0] * M[2] - M[1] * M[5];
    const double b2 = -M[3] * M[2] - M[4] * M[5];
    M[2] = b1; M[5] = b2;
    for (int i = 0; i < 6; ++i) out[i] = M[i];
    return 0;
}

int hh_warp_affine_u8(const unsigned char *image_hwc, int h, int w, const double dst_to_src[6], unsigned char *out_hwc, int H, int W, void *stream)
{
    if (!image_hwc || !out_hwc || h <= 0 || w <= 0 || H <= 0 || W <= 0) { hh_set_error("hh_warp_affine_u8: bad argument"); return 1; }
    HH_CHECK_HIP(launch_warp_affine_u8(image_hwc, h, w, dst_to_src, out_hwc, H, W, (hipStream_t)stream));
    return 0;
}

int hh_transform_coords(const float *xy_in, int n, double cx, double cy, double scale_w, double dst_w, double dst_h,
                        double *xy_out)
{
#pragma clang fp contract(off)
    double M[6];
    if (hh_get_affine_transform(cx, cy, scale_w, dst_w, dst_h, 1, M)) return 1;
    for (int i = 0; i < n; ++i) {  // affine_transform (base/transforms/utils.py:5-8): M @ (x, y, 1) in float64
        const double x = (double)xy_in[2 * i + 0], y = (double)xy_in[2 * i + 1];
        xy_out[2 * i + 0] = M[0] * x + M[1] * y + M[2] * 1.0;
        xy_out[2 * i + 1] = M[3] * x + M[4] * y + M[5] * 1.0;
    }
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------
// Kernel micro-benchmark (tools/conv_bench.py): one convolution shape, random bf16 data, `iters` back-to-back
// launches of instantiation `cfg` timed with HIP events.  If `max_diff`
// is given, the output is also compared with generic instantiation `ref_cfg` on the same data.  Not on the hot path.
extern "C" int hh_debug_conv_bench(int cfg, int B, int Hin, int Win, int cin, int cout, int with_res, int relu, int iters,
                                   float *ms_per_launch, unsigned long long *stamps16, int ref_cfg, float *max_diff)
{
    HH_CHECK_HIP(conv_init());
    if (cfg < 0 || cfg >= conv_num_configs()) { hh_set_error("bad cfg"); return 1; }
    ConvConfig c = conv_config(cfg);
    if (cin % c.KC) { hh_set_error("cin must be a multiple of the config's KC"); return 1; }
    const int coutp = (cout + c.cout_t() - 1) / c.cout_t() * c.cout_t();
    const int Ho = c.S == 2 ? Hin / 2 : Hin, Wo = c.S == 2 ? Win / 2 : Win;
    const size_t n_in = (size_t)B * Hin * Win * cin, n_out = (size_t)B * Ho * Wo * coutp;
    std::vector<bf16_raw> h_in(n_in), h_res(n_out);
    std::vector<float> W((size_t)cout * cin * c.KS * c.KS), scale(coutp, 1.f);
    uint32_t s = 12345u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (bf16_raw)(0x3c00u + ((s >> 16) & 0x1ffu) + ((s >> 30) << 15)); };
    auto rndf = [&]() { s = s * 1664525u + 1013904223u; return ((int)(s >> 20) - 2048) / 16384.0f; };
    for (auto &v : h_in) v = rnd();
    for (auto &v : h_res) v = rnd();
    for (auto &v : W) v = rndf();
    bf16_raw *d_in, *d_out, *d_out2, *d_res, *d_zero;
    float *d_bias;
    HH_CHECK_HIP(hipMalloc((void **)&d_in, n_in * 2));
    HH_CHECK_HIP(hipMalloc((void **)&d_out, n_out * 2));
    HH_CHECK_HIP(hipMalloc((void **)&d_out2, n_out * 2));
    HH_CHECK_HIP(hipMalloc((void **)&d_res, n_out * 2));
    HH_CHECK_HIP(hipMalloc((void **)&d_bias, (size_t)coutp * 4));
    HH_CHECK_HIP(hipMalloc((void **)&d_zero, 256));
    HH_CHECK_HIP(hipMemcpy(d_in, h_in.data(), n_in * 2, hipMemcpyHostToDevice));
    HH_CHECK_HIP(hipMemcpy(d_res, h_res.data(), n_out * 2, hipMemcpyHostToDevice));
    HH_CHECK_HIP(hipMemset(d_bias, 0, (size_t)coutp * 4));
    HH_CHECK_HIP(hipMemset(d_zero, 0, 256));
    HH_CHECK_HIP(hipMemset(d_out, 0, n_out * 2));
    HH_CHECK_HIP(hipMemset(d_out2, 0, n_out * 2));
    unsigned long long *d_st = nullptr;
    HH_CHECK_HIP(hipMalloc((void **)&d_st, 16 * 8));
    HH_CHECK_HIP(hipMemset(d_st, 0, 16 * 8));
    hipStream_t st;
    HH_CHECK_HIP(hipStreamCreate(&st));
    auto run = [&](int k, bf16_raw *out, int n, float *ms_out) -> int {
        const ConvConfig cc = conv_config(k);
        std::vector<bf16_raw> packed;
        hh_pack_weights(W.data(), scale.data(), cc.KS, cin, cout, cc.KC, cc.cout_t(), false, 0, 0, packed);
        bf16_raw *d_w;
        HH_CHECK_HIP(hipMalloc((void **)&d_w, packed.size() * 2));
        HH_CHECK_HIP(hipMemcpy(d_w, packed.data(), packed.size() * 2, hipMemcpyHostToDevice));
        ConvParams p{};
        p.in = d_in; p.in_cs = cin; p.Hin = Hin; p.Win = Win; p.w = d_w; p.bias = d_bias;
        p.res = with_res ? d_res : nullptr; p.res_cs = coutp;
        p.out = out; p.out_cs = coutp; p.Hob = Ho; p.Wob = Wo; p.osy = p.osx = 1;
        p.Ho = Ho; p.Wo = Wo; p.cin = cin; p.cout_real = cout; p.cout_store = coutp; p.relu = relu;
        p.pad_y = p.pad_x = (cc.KS - 1) / 2; p.B = B; p.stamps = d_st;
        p.tiles_x = (Wo + cc.TW - 1) / cc.TW; p.tiles_y = (Ho + cc.th() - 1) / cc.th(); p.ncg = coutp / cc.cout_t();
        auto launch = [&]() { return conv_launch(k, p, st); };
        hipEvent_t e0, e1;
        HH_CHECK_HIP(hipEventCreate(&e0));
        HH_CHECK_HIP(hipEventCreate(&e1));
        for (int i = 0; i < 3; ++i) HH_CHECK_HIP(launch());
        HH_CHECK_HIP(hipEventRecord(e0, st));
        for (int i = 0; i < n; ++i) HH_CHECK_HIP(launch());
        HH_CHECK_HIP(hipEventRecord(e1, st));
        HH_CHECK_HIP(hipEventSynchronize(e1));
        float ms = 0;
        HH_CHECK_HIP(hipEventElapsedTime(&ms, e0, e1));
        if (ms_out) *ms_out = ms / n;
        hipEventDestroy(e0); hipEventDestroy(e1); hipFree(d_w);
        return 0;
    };
    if (run(cfg, d_out, iters, ms_per_launch)) return 1;
    if (stamps16) HH_CHECK_HIP(hipMemcpy(stamps16, d_st, 16 * 8, hipMemcpyDeviceToHost));
    if (max_diff) {
        if (run(ref_cfg, d_out2, 1, nullptr)) return 1;
        std::vector<bf16_raw> a(n_out), b2(n_out);
        HH_CHECK_HIP(hipMemcpy(a.data(), d_out, n_out * 2, hipMemcpyDeviceToHost));
        HH_CHECK_HIP(hipMemcpy(b2.data(), d_out2, n_out * 2, hipMemcpyDeviceToHost));
        float md = 0.f;
        for (size_t i = 0; i < n_out; ++i) {
            uint32_t ua = (uint32_t)a[i] << 16, ub = (uint32_t)b2[i] << 16;
            float fa, fb;
            memcpy(&fa, &ua, 4); memcpy(&fb, &ub, 4);
            const float d = fa > fb ? fa - fb : fb - fa;
            if (d > md || d != d) md = d;
        }
        *max_diff = md;
    }
    hipStreamDestroy(st);
    hipFree(d_in); hipFree(d_out); hipFree(d_out2); hipFree(d_res); hipFree(d_bias); hipFree(d_st); hipFree(d_zero);
    return 0;
}

// Host-only walk of the producer / consumer block's tiles (bbpc_cover, basicblock_fused_pc.hip): see hhrnet.h
extern "C" int hh_debug_bb_cover(int B, int H, int W, int tall, int num_cus, int64_t counts[4])
{
    long long c[4];
    if (!counts) { hh_set_error("hh_debug_bb_cover: counts is NULL"); return 1; }
    if (!bbpc_cover(B, H, W, tall, num_cus, c)) { hh_set_error("hh_debug_bb_cover: the launcher does not take this shape"); return 1; }
    for (int i = 0; i < 4; ++i) counts[i] = c[i];
    return 0;
}

// A/B of the two fused 32-channel blocks on the same random input (H, W need not be tile multiples): the largest absolute
// difference of the outputs (both round to bf16, the accumulation orders differ: expect a few bf16 ulps) and the time per launch.
extern "C" int hh_debug_bb_compare(int B, int H, int W, int iters, float *max_diff, float *ms_classic, float *ms_pc)
{
    HH_CHECK_HIP(conv_init());
    HH_CHECK_HIP(bb_fused_init());
    HH_CHECK_HIP(bbpc_init());
    const size_t n = (size_t)B * H * W * 32;
    std::vector<bf16_raw> h_in(n), h_w(2 * 9 * 32 * 32), h_o1(n), h_o2(n);
    std::vector<float> h_b(64);
    uint32_t s = 4242u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (bf16_raw)(0x3c00u + ((s >> 16) & 0x1ffu) + ((s >> 30) << 15)); };  // +-[0.0078, 0.031)
    for (auto &v : h_in) v = (bf16_raw)(rnd() + 0x0300u);
    for (auto &v : h_w) v = rnd();
    for (auto &v : h_b) { s = s * 1664525u + 1013904223u; v = ((int)(s >> 20) - 2048) * 1e-4f; }
    bf16_raw *d_in, *d_o1, *d_o2, *d_w;
    float *d_b;
    HH_CHECK_HIP(hipMalloc((void **)&d_in, n * 2));
    HH_CHECK_HIP(hipMalloc((void **)&d_o1, n * 2));
    HH_CHECK_HIP(hipMalloc((void **)&d_o2, n * 2));
    HH_CHECK_HIP(hipMalloc((void **)&d_w, h_w.size() * 2));
    HH_CHECK_HIP(hipMalloc((void **)&d_b, 64 * 4));
    HH_CHECK_HIP(hipMemcpy(d_in, h_in.data(), n * 2, hipMemcpyHostToDevice));
    HH_CHECK_HIP(hipMemcpy(d_w, h_w.data(), h_w.size() * 2, hipMemcpyHostToDevice));
    HH_CHECK_HIP(hipMemcpy(d_b, h_b.data(), 64 * 4, hipMemcpyHostToDevice));
    HH_CHECK_HIP(hipMemset(d_o1, 0xff, n * 2));
    HH_CHECK_HIP(hipMemset(d_o2, 0xff, n * 2));
    BBParams p{};
    p.in = d_in; p.in_cs = 32; p.out_cs = 32; p.w1 = d_w; p.w2 = d_w + 9 * 32 * 32; p.b1 = d_b; p.b2 = d_b + 32;
    p.B = B; p.H = H; p.W = W;
    unsigned long long *d_st = nullptr;
    HH_CHECK_HIP(hipMalloc((void **)&d_st, 72 * 8));
    HH_CHECK_HIP(hipMemset(d_st, 0, 72 * 8));
    p.stamps = d_st;
    int dev = 0;
    hipDeviceProp_t prop;
    HH_CHECK_HIP(hipGetDevice(&dev));
    HH_CHECK_HIP(hipGetDeviceProperties(&prop, dev));
    hipStream_t st;
    HH_CHECK_HIP(hipStreamCreate(&st));
    hipEvent_t e0, e1;
    HH_CHECK_HIP(hipEventCreate(&e0));
    HH_CHECK_HIP(hipEventCreate(&e1));
    float ms[2] = {0, 0};
    for (int v = 0; v < 2; ++v) {
        p.out = v ? d_o2 : d_o1;
        auto go = [&]() { return v ? bbpc_launch(p, prop.multiProcessorCount, st) : bb_fused_launch(p, prop.multiProcessorCount, st); };
        for (int i = 0; i < 3; ++i) HH_CHECK_HIP(go());
        HH_CHECK_HIP(hipEventRecord(e0, st));
        for (int i = 0; i < iters; ++i) HH_CHECK_HIP(go());
        HH_CHECK_HIP(hipEventRecord(e1, st));
        HH_CHECK_HIP(hipEventSynchronize(e1));
        HH_CHECK_HIP(hipEventElapsedTime(&ms[v], e0, e1));
#ifdef HH_STAMP
        {
            unsigned long long c[4];
            HH_CHECK_HIP(hipMemcpy(c, d_st + 64, sizeof(c), hipMemcpyDeviceToHost));
            if (c[3] > c[1]) fprintf(stderr, "  %s: in-kernel clock of the last launch %.3f GHz (%lld core cycles in %.2f us)\n", v ? "producer/consumer" : "tile form",
                                     (double)(c[2] - c[0]) / (double)(c[3] - c[1]) * 0.1, (long long)(c[2] - c[0]), (double)(c[3] - c[1]) * 0.01);
        }
#endif
    }
    HH_CHECK_HIP(hipMemcpy(h_o1.data(), d_o1, n * 2, hipMemcpyDeviceToHost));
    HH_CHECK_HIP(hipMemcpy(h_o2.data(), d_o2, n * 2, hipMemcpyDeviceToHost));
    float md = 0.f;
    for (size_t i = 0; i < n; ++i) {
        uint32_t a = (uint32_t)h_o1[i] << 16, b = (uint32_t)h_o2[i] << 16;
        float fa, fb;
        memcpy(&fa, &a, 4); memcpy(&fb, &b, 4);
        const float d = fabsf(fa - fb);
        if (!(d <= md)) md = d;  // NaN sticks
    }
    *max_diff = md; *ms_classic = ms[0] / iters; *ms_pc = ms[1] / iters;
#ifdef HH_STAMP
    {
        unsigned long long stv[72];
        HH_CHECK_HIP(hipMemcpy(stv, d_st, sizeof(stv), hipMemcpyDeviceToHost));
        for (int w = 0; w < 8; ++w) {
            fprintf(stderr, "  wave %d (100 MHz ticks from its iteration start):", w);
            for (int i = 1; i < 8; ++i) fprintf(stderr, " %lld", stv[w * 8 + i] ? (long long)(stv[w * 8 + i] - stv[w * 8]) : -1ll);
            fprintf(stderr, "   start %+lld vs wave 0\n", (long long)(stv[w * 8] - stv[0]));
        }
    }
#endif
    hipFree(d_st);
    hipEventDestroy(e0); hipEventDestroy(e1); hipStreamDestroy(st);
    hipFree(d_in); hipFree(d_o1); hipFree(d_o2); hipFree(d_w); hipFree(d_b);
    return 0;
}

// Fused BasicBlock micro-benchmark; with a -DHH_STAMP build also returns s_memtime stamps of workgroup 0.
extern "C" int hh_debug_bb_bench(int B, int H, int W, int iters, float *ms_per_launch, unsigned long long *stamps64)
{
    HH_CHECK_HIP(conv_init());
    HH_CHECK_HIP(bb_fused_init());
    const size_t n = (size_t)B * H * W * 32;
    std::vector<bf16_raw> h_in(n), h_w(9 * 32 * 32);
    uint32_t s = 777u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (bf16_raw)(0x3c00u + ((s >> 16) & 0x1ffu) + ((s >> 30) << 15)); };
    for (auto &v : h_in) v = rnd();
    for (auto &v : h_w) v = (bf16_raw)(rnd() - 0x0400u);
    bf16_raw *d_in, *d_out, *d_w;
    float *d_b;
    unsigned long long *d_st;
    HH_CHECK_HIP(hipMalloc((void **)&d_in, n * 2));
    HH_CHECK_HIP(hipMalloc((void **)&d_out, n * 2));
    HH_CHECK_HIP(hipMalloc((void **)&d_w, h_w.size() * 2));
    HH_CHECK_HIP(hipMalloc((void **)&d_b, 32 * 4));
    HH_CHECK_HIP(hipMalloc((void **)&d_st, 72 * 8));
    HH_CHECK_HIP(hipMemcpy(d_in, h_in.data(), n * 2, hipMemcpyHostToDevice));
    HH_CHECK_HIP(hipMemcpy(d_w, h_w.data(), h_w.size() * 2, hipMemcpyHostToDevice));
    HH_CHECK_HIP(hipMemset(d_b, 0, 32 * 4));
    HH_CHECK_HIP(hipMemset(d_st, 0, 64 * 8));
    BBParams p{};
    p.in = d_in; p.in_cs = 32; p.out = d_out; p.out_cs = 32; p.w1 = d_w; p.w2 = d_w; p.b1 = d_b; p.b2 = d_b;
    p.B = B; p.H = H; p.W = W; p.stamps = d_st;
    int dev = 0;
    hipDeviceProp_t prop;
    HH_CHECK_HIP(hipGetDevice(&dev));
    HH_CHECK_HIP(hipGetDeviceProperties(&prop, dev));
    hipStream_t st;
    HH_CHECK_HIP(hipStreamCreate(&st));
    hipEvent_t e0, e1;
    HH_CHECK_HIP(hipEventCreate(&e0));
    HH_CHECK_HIP(hipEventCreate(&e1));
    for (int i = 0; i < 3; ++i) HH_CHECK_HIP(bb_fused_launch(p, prop.multiProcessorCount, st));
    HH_CHECK_HIP(hipEventRecord(e0, st));
    for (int i = 0; i < iters; ++i) HH_CHECK_HIP(bb_fused_launch(p, prop.multiProcessorCount, st));
    HH_CHECK_HIP(hipEventRecord(e1, st));
    HH_CHECK_HIP(hipEventSynchronize(e1));
    float ms = 0;
    HH_CHECK_HIP(hipEventElapsedTime(&ms, e0, e1));
    *ms_per_launch = ms / iters;
    if (stamps64) HH_CHECK_HIP(hipMemcpy(stamps64, d_st, 64 * 8, hipMemcpyDeviceToHost));
    hipEventDestroy(e0); hipEventDestroy(e1); hipStreamDestroy(st);
    hipFree(d_in); hipFree(d_out); hipFree(d_w); hipFree(d_b); hipFree(d_st);
    return 0;
}
