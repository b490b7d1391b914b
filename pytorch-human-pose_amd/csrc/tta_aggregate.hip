// Multi-scale (+ flip) heatmap aggregation as ONE launch (hh_multi_scale_aggregate; BASELINE.json configs[3], an extension: the
// reference has no aggregation code).  What InferenceKeypointsModel.multi_scale_maps composes per image out of hh_flip_merge and
// one read-modify-write hh_resize_accumulate per scale happens here in registers: every output value takes its four taps of every
// source (each tap flip-merged on the fly where the source brings a flipped pass), resizes, weights and sums them in the order of
// the source table, and is stored once.  No merged map and no partial accumulator reaches HBM.
// Built with -ffp-contract=off like the decode files: the result must equal that composition bit for bit, so the tap expression is
// flip_merge_kernel's (misc_kernels.hip), the interpolation is src_index / bilerp's fmaf pattern (decode_dev.h), and weight * value
// and acc + value are rounded one by one as resize_accumulate_kernel (decode_kernels.hip) rounds them.
#include "kernels.h"
#include "decode_dev.h"
#include "engine.h"
#include "../../include/hhrnet.h"

static_assert(sizeof(hh_scale_src) == 48, "ABI 3");
struct AggSrc {
    const float *hm, *hmf;  // hmf null: plain source
    long long bs, fbs;      // batch strides in elements
    int h, w;
    float sy, sx;           // torch's area_pixel_compute_scale, (float)in / (float)out, divided once on the host
    float weight;
    int pad_;
};
// K <= 64 joints, <= 8 sources: table and permutation travel in the kernel arguments (as FlipPerm does), no device buffer to share
// between streams
struct AggTable {
    AggSrc s[HH_MAX_SCALE_SRCS];
    FlipPerm perm;
};

// one thread = 4 consecutive x of one (b, k, y) row: the row's y interpolation is formed once per source, the four values leave in
// one 16-byte store where the row address allows it.  Taps of upsampled sources are re-read through the cache (neighbouring
// outputs share them); there is nothing to stage in LDS.
__global__ __launch_bounds__(256) void multi_scale_aggregate_kernel(const AggTable t, int nsrc, int K, float *__restrict__ dst,
                                                                    long long dst_bs, int H, int W, int W4, long long total)
{
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= total) return;
    const int xq = (int)(id % W4), row = (int)(id / W4);
    const int y = row % H, bk = row / H, k = bk % K, b = bk / K;
    const int x0 = xq * 4;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < nsrc; ++i) {
        const AggSrc &s = t.s[i];
        const int w = s.w;
        const size_t plane = (size_t)s.h * w;
        const Lin ly = src_index(s.h, s.sy, y);
        const float *p = s.hm + (size_t)b * s.bs + (size_t)k * plane;
        const float *p0 = p + (size_t)ly.i0 * w, *p1 = p + (size_t)ly.i1 * w;
        // the flipped pass's rows, addressed from their last column: tap column c of the merged map reads column w-1-c
        const float *f0 = nullptr, *f1 = nullptr;
        if (s.hmf) {
            const float *f = s.hmf + (size_t)b * s.fbs + (size_t)t.perm.v[k] * plane + (w - 1);
            f0 = f + (size_t)ly.i0 * w;
            f1 = f + (size_t)ly.i1 * w;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = x0 + j < W ? x0 + j : W - 1;  // (past the row's end: a value that is formed and not stored)
            const Lin lx = src_index(w, s.sx, x);
            float t00 = p0[lx.i0], t01 = p0[lx.i1], t10 = p1[lx.i0], t11 = p1[lx.i1];
            if (f0) {
                t00 = (t00 + f0[-lx.i0]) / 2.0f; t01 = (t01 + f0[-lx.i1]) / 2.0f;
                t10 = (t10 + f1[-lx.i0]) / 2.0f; t11 = (t11 + f1[-lx.i1]) / 2.0f;
            }
            const float a = __builtin_fmaf(t00, lx.w0, t01 * lx.w1);
            const float c = __builtin_fmaf(t10, lx.w0, t11 * lx.w1);
            const float v = s.weight * __builtin_fmaf(a, ly.w0, c * ly.w1);
            acc[j] = i == 0 ? v : acc[j] + v;
        }
    }
    float *o = dst + (size_t)b * dst_bs + ((size_t)k * H + y) * W + x0;
    if (x0 + 3 < W && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
        *reinterpret_cast<float4 *>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x0 + j < W) o[j] = acc[j];
    }
}

int hh_multi_scale_aggregate(const hh_scale_src *srcs_host, int nsrc, const int32_t *perm_host, int B, int K, float *dst,
                             int64_t dst_bstride, int H, int W, void *stream)
{
    // every refusal comes before the first HIP call
    if (nsrc < 1 || nsrc > HH_MAX_SCALE_SRCS) { hh_set_error("hh_multi_scale_aggregate: need 1 <= nsrc <= 8"); return 1; }
    if (!srcs_host || !dst) { hh_set_error("hh_multi_scale_aggregate: null srcs_host or dst"); return 1; }
    if (K < 1 || K > 64) { hh_set_error("hh_multi_scale_aggregate: need 1 <= K <= 64"); return 1; }
    if (B <= 0 || H <= 0 || W <= 0) { hh_set_error("hh_multi_scale_aggregate: B, H and W must be positive"); return 1; }
    if (dst_bstride < (int64_t)K * H * W) { hh_set_error("hh_multi_scale_aggregate: dst_bstride < K*H*W"); return 1; }
    const int W4 = (W + 3) / 4;
    const long long rows = (long long)B * K * H, total = rows * W4;
    if (rows >= (1ll << 31) || (total + 255) / 256 >= (1ll << 31)) { hh_set_error("hh_multi_scale_aggregate: dst too large for one launch"); return 1; }
    AggTable t{};
    bool any_flipped = false;
    for (int i = 0; i < nsrc; ++i) {
        const hh_scale_src &s = srcs_host[i];
        if (!s.hm) { hh_set_error("hh_multi_scale_aggregate: null hm in source " + std::to_string(i)); return 1; }
        if (s.h <= 0 || s.w <= 0) { hh_set_error("hh_multi_scale_aggregate: h and w must be positive in source " + std::to_string(i)); return 1; }
        const long long need = (long long)K * s.h * s.w;
        if (s.bstride < need || (s.hm_flipped && s.flipped_bstride < need)) {
            hh_set_error("hh_multi_scale_aggregate: batch stride < K*h*w in source " + std::to_string(i));
            return 1;
        }
        any_flipped |= s.hm_flipped != nullptr;
        t.s[i] = AggSrc{s.hm, s.hm_flipped, s.bstride, s.flipped_bstride, s.h, s.w, (float)s.h / (float)H, (float)s.w / (float)W, s.weight, 0};
    }
    if (any_flipped) {
        if (!perm_host) { hh_set_error("hh_multi_scale_aggregate: null perm_host with a flipped source"); return 1; }
        for (int k = 0; k < K; ++k) {
            if (perm_host[k] < 0 || perm_host[k] >= K) { hh_set_error("hh_multi_scale_aggregate: perm is not a permutation of 0..K-1"); return 1; }
            t.perm.v[k] = (unsigned char)perm_host[k];
        }
    }
    hipLaunchKernelGGL(multi_scale_aggregate_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, t, nsrc, K,
                       dst, (long long)dst_bstride, H, W, W4, total);
    HH_CHECK_HIP(hipGetLastError());
    return 0;
}
