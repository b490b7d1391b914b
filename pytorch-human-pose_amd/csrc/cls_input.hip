// The classifier's input built on the GPU: classification/transforms.py:14-30 (train: ToTensor -> RandomResizedCrop(antialias) ->
// RandomHorizontalFlip -> Normalize; inference: ToTensor -> Resize(antialias) -> CenterCrop -> Normalize) and
// classification/model.py:45-57 as ONE launch per batch over raw uint8 images of mixed sizes (hh_crop_desc of include/hhrnet.h).
//
// The resample is torch's upsample_bilinear2d_aa (align_corners = False), which torchvision's tensor resize / resized_crop call: a
// separable triangle filter whose support grows with the down-scale, horizontal pass first, the intermediate kept as fp32.  Per
// axis, with in = crop extent, out = virtual size, scale = in / out, support = antialias ? max(scale, 1) : 1:
//   centre = scale (i + 0.5); taps j in [max(0, int(centre - support + 0.5)), min(in, int(centre + support + 0.5)));
//   weight = tri((j - centre + 0.5) / support) / (sum of the taps' tri), tri(x) = max(0, 1 - |x|),
// all in fp32 in torch's operation order (the division by the support is torch's multiplication by 1 / scale), the sum over the taps
// sequential from the first tap, product and sum rounded separately (the file is compiled with -ffp-contract=off).  Tap indices
// count from the crop's corner and never leave the crop: what lies outside the crop rectangle does not exist, as for a tensor that
// was cropped first.  A crop whose extent equals the virtual size has the weights 1 and 0 and gives ToTensor's value bit for bit.
//
// One workgroup owns a TH x TW tile of one sample's output.  It walks the source rows its TH rows touch in chunks of CHUNK rows:
// the horizontal pass of a chunk goes to LDS as fp32 [row][channel][column] (a thread keeps ONE tile column for the whole kernel, so
// its column's tap range and weight sum are formed once), then every thread adds the chunk's rows to its output pixel's three
// channel sums in ascending row order.  There is no cap on the tap count on either axis: both tap loops are loops, the chunks bound
// the LDS.  Weights are recomputed per tap from the descriptor (a handful of fp32 operations; the kernel moves ~1 byte per 4
// operations either way and is bound by the source bytes and the output stores).  ToTensor's v / 255.0f is a 256-entry table of the
// very quotients.  Every output element is written exactly once; nothing depends on the launch.
#include "kernels.h"

#define CROP_TH 8
#define CROP_TW 32
#define CROP_THREADS (CROP_TH * CROP_TW)
#define CROP_CHUNK 32  // source rows per LDS chunk: 32 * 3 * 32 floats = 12 KB

struct AxisTaps {
    int lo, n;  // taps lo .. lo + n - 1, relative to the crop
    float centre, invscale, total;
};

__device__ __forceinline__ float tri_filter(float x)
{
    x = fabsf(x);
    return x < 1.f ? 1.f - x : 0.f;
}
__device__ __forceinline__ float tap_raw(const AxisTaps &t, int j) { return tri_filter(((float)(j + t.lo) - t.centre + 0.5f) * t.invscale); }
__device__ __forceinline__ float tap_weight(const AxisTaps &t, int j)
{
    const float w = tap_raw(t, j);
    return t.total != 0.f ? w / t.total : w;
}
// tap range of output index i (with_total: also the sum that normalises the weights)
__device__ __forceinline__ AxisTaps axis_taps(int i, int in, int out, int antialias, bool with_total)
{
    AxisTaps t;
    const float scale = (float)in / (float)out;
    const bool wide = antialias && scale >= 1.f;
    const float support = wide ? scale : 1.f;
    t.invscale = wide ? 1.f / scale : 1.f;
    t.centre = scale * ((float)i + 0.5f);
    t.lo = max((int)(t.centre - support + 0.5f), 0);
    t.n = min((int)(t.centre + support + 0.5f), in) - t.lo;  // lo >= 0 and lo + n <= in: no tap leaves the crop
    t.total = 0.f;
    if (with_total)
        for (int j = 0; j < t.n; ++j) t.total += tap_raw(t, j);
    return t;
}

__global__ __launch_bounds__(CROP_THREADS) void resized_crop_kernel(const unsigned char *__restrict__ base, const hh_crop_desc *__restrict__ descs,
                                                                    float *__restrict__ out, int H, int W, float m0, float m1, float m2,
                                                                    float s0, float s1, float s2)
{
    __shared__ float to_tensor[256];
    __shared__ float rows[CROP_CHUNK][3][CROP_TW];
    const int tid = threadIdx.x, xi = tid % CROP_TW, yi = tid / CROP_TW;
    const hh_crop_desc d = descs[blockIdx.z];
    to_tensor[tid] = (float)tid / 255.0f;  // CROP_THREADS == 256

    const int x = blockIdx.x * CROP_TW + xi, y = blockIdx.y * CROP_TH + yi;
    const bool col_live = x < W, live = col_live && y < H;
    // this thread's column of the virtual image (the flip reverses the window's columns) and its row
    const AxisTaps tx = axis_taps(d.ox + (d.flip ? W - 1 - min(x, W - 1) : min(x, W - 1)), d.cw, d.rw, d.antialias, true);
    const AxisTaps ty = axis_taps(d.oy + min(y, H - 1), d.ch, d.rh, d.antialias, true);
    // the source rows of the whole tile (the tap ranges are monotone in the row): the same in every thread
    const int y_first = blockIdx.y * CROP_TH, y_last = min(y_first + CROP_TH, H) - 1;
    const AxisTaps t_first = axis_taps(d.oy + y_first, d.ch, d.rh, d.antialias, false), t_last = axis_taps(d.oy + y_last, d.ch, d.rh, d.antialias, false);
    const int r_begin = t_first.lo, r_end = t_last.lo + t_last.n;

    const unsigned char *img = base + d.image_offset;
    float acc[3] = {0.f, 0.f, 0.f};
    __syncthreads();  // the table
    for (int r0 = r_begin; r0 < r_end; r0 += CROP_CHUNK) {
        const int r1 = min(r0 + CROP_CHUNK, r_end);
        // horizontal pass: source rows r0 .. r1 - 1 of the crop at this thread's column
        for (int r = r0 + yi; r < r1; r += CROP_TH) {
            float h[3] = {0.f, 0.f, 0.f};
            if (col_live) {
                const unsigned char *p = img + ((d.top + r) * d.w + d.left + tx.lo) * 3;  // < h * w * 3 <= INT_MAX (checked by the caller)
                for (int j = 0; j < tx.n; ++j, p += 3) {
                    const float wgt = tap_weight(tx, j);
#pragma unroll
                    for (int c = 0; c < 3; ++c) h[c] += to_tensor[p[c]] * wgt;
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) rows[r - r0][c][xi] = h[c];
        }
        __syncthreads();
        // vertical pass: the chunk's share of this thread's rows, ascending
        const int a = max(r0, ty.lo), b = min(r1, ty.lo + ty.n);
        for (int r = a; r < b; ++r) {
            const float wgt = tap_weight(ty, r - ty.lo);
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += rows[r - r0][c][xi] * wgt;
        }
        __syncthreads();  // everyone has read the chunk before the next one overwrites it
    }
    if (!live) return;
    const float mean[3] = {m0, m1, m2}, stdv[3] = {s0, s1, s2};
    float *o = out + (size_t)blockIdx.z * 3 * H * W + (size_t)y * W + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[(size_t)c * H * W] = (acc[c] - mean[c]) / stdv[c];
}

hipError_t launch_resized_crop(const unsigned char *base, const hh_crop_desc *descs, int n, float *out, int H, int W, const float mean[3],
                               const float stdv[3], hipStream_t s)
{
    hipLaunchKernelGGL(resized_crop_kernel, dim3((W + CROP_TW - 1) / CROP_TW, (H + CROP_TH - 1) / CROP_TH, n), dim3(CROP_THREADS), 0, s, base, descs,
                       out, H, W, mean[0], mean[1], mean[2], stdv[0], stdv[1], stdv[2]);
    return hipGetLastError();
}
