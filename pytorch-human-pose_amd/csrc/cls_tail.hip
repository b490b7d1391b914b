// The classification head's tail in training form (classification/architectures/hrnet.py:55-61, classification/loss.py,
// classification/module.py:15-22): the backward of the global average pool, the three gradients of the fp32 Linear, and softmax
// cross-entropy fused with its gradient and the top-1 / top-5 hit counts.  The pool's forward is avgpool_kernel and the Linear's
// forward linear_kernel (misc_kernels.hip), the ones the inference engine runs.
// ~1 GFLOP per step at B = 80 beside the backbone's 4.3 TFLOP: plain fp32 FMA, no matrix cores.  Every sum is taken by one thread, one
// wave's shuffle tree, or per-wave partial sums added in wave order: an order that depends on the shape alone, so results are identical
// from call to call.
#include "mfma_dev.h"

// dx[b, p, c] = g[b, c] / HW, rounded to E: one thread = 8 channels of one pixel (C % 8 == 0)
template <typename E>
__global__ __launch_bounds__(256) void avgpool_backward_kernel(const float *__restrict__ g, bf16_raw *__restrict__ dx, int B, int HW, int C)
{
    const int c8n = C / 8;
    const size_t total = (size_t)B * HW * c8n;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c8 = (int)(i % c8n);
        const size_t bp = i / c8n;  // b * HW + p
        const int b = (int)(bp / HW);
        const float4 lo = *reinterpret_cast<const float4 *>(g + (size_t)b * C + c8 * 8);
        const float4 hi = *reinterpret_cast<const float4 *>(g + (size_t)b * C + c8 * 8 + 4);
        const float n = (float)HW;
        uint4 v;
        v.x = E::round2(lo.x / n, lo.y / n); v.y = E::round2(lo.z / n, lo.w / n);
        v.z = E::round2(hi.x / n, hi.y / n); v.w = E::round2(hi.z / n, hi.w / n);
        *reinterpret_cast<uint4 *>(dx + bp * C + c8 * 8) = v;
    }
}
hipError_t launch_avgpool_backward(const float *g, bf16_raw *dx, int B, int HW, int C, hipStream_t s, int act_dtype)
{
    const size_t total = (size_t)B * HW * (C / 8);
    unsigned grid = (unsigned)((total + 255) / 256);
    if (grid > 8192) grid = 8192;
    if (act_dtype == 0) hipLaunchKernelGGL(avgpool_backward_kernel<ElemBF16>, dim3(grid), dim3(256), 0, s, g, dx, B, HW, C);
    else if (act_dtype == 1) hipLaunchKernelGGL(avgpool_backward_kernel<ElemF16>, dim3(grid), dim3(256), 0, s, g, dx, B, HW, C);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// ------------------------------------------------------------------ nn.Linear backward, fp32: y = x W^T + b with x [B,K], W [N,K]
// dX[b, k] = sum_n dY[b, n] W[n, k].  One workgroup = LIN_TB batch rows of 64 k (lane = k: W is read coalesced along k, once per LIN_TB
// rows; the dY values are the same for a whole wave).  Its LIN_NW waves split the sum over n: wave w adds n = w, w + LIN_NW, ... in
// ascending order into one accumulator per (row, k), and wave 0 adds the LIN_NW partial sums from LDS in wave order -- an order that
// depends on the shape alone.  (One wave per workgroup walking all N was a chain of N dependent load + FMA steps: 0.48 ms at B = 80.)
#define LIN_TB 8
#define LIN_NW 16
__global__ __launch_bounds__(64 * LIN_NW) void linear_dx_kernel(const float *__restrict__ dy, const float *__restrict__ w, float *__restrict__ dx,
                                                                int B, int K, int N)
{
    __shared__ float part[LIN_NW][LIN_TB][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = blockIdx.x * 64 + lane, b0 = blockIdx.y * LIN_TB;
    const int nb = min(LIN_TB, B - b0);
    float acc[LIN_TB] = {};
    if (k < K) {
        for (int n = wave; n < N; n += LIN_NW) {
            const float wv = w[(size_t)n * K + k];
#pragma unroll
            for (int i = 0; i < LIN_TB; ++i)
                if (i < nb) acc[i] += dy[(size_t)(b0 + i) * N + n] * wv;
        }
    }
#pragma unroll
    for (int i = 0; i < LIN_TB; ++i) part[wave][i][lane] = acc[i];
    __syncthreads();
    if (wave == 0 && k < K) {
#pragma unroll
        for (int i = 0; i < LIN_TB; ++i) {
            if (i >= nb) break;
            float s = part[0][i][lane];
            for (int v = 1; v < LIN_NW; ++v) s += part[v][i][lane];
            dx[(size_t)(b0 + i) * K + k] = s;
        }
    }
}
// dW[n, k] = sum_b dY[b, n] X[b, k] and db[n] = sum_b dY[b, n], b ascending.  One workgroup = 256 k of one n.
__global__ __launch_bounds__(256) void linear_dw_kernel(const float *__restrict__ dy, const float *__restrict__ x, float *__restrict__ dw,
                                                        float *__restrict__ db, int B, int K, int N)
{
    const int k = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
    if (db && k == 0) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += dy[(size_t)b * N + n];
        db[n] = s;
    }
    if (!dw || k >= K) return;
    float acc = 0.f;
    for (int b = 0; b < B; ++b) acc += dy[(size_t)b * N + n] * x[(size_t)b * K + k];
    dw[(size_t)n * K + k] = acc;
}
hipError_t launch_linear_backward(const float *x, const float *w, const float *dy, int B, int K, int N, float *dx, float *dw, float *db,
                                  hipStream_t s)
{
    if (dx) hipLaunchKernelGGL(linear_dx_kernel, dim3((K + 63) / 64, (B + LIN_TB - 1) / LIN_TB), dim3(64 * LIN_NW), 0, s, dy, w, dx, B, K, N);
    // (db alone needs the workgroups that hold k = 0 only)
    if (dw || db) hipLaunchKernelGGL(linear_dw_kernel, dim3(dw ? (K + 255) / 256 : 1, N), dim3(256), 0, s, dy, x, dw, db, B, K, N);
    return hipGetLastError();
}

// ------------------------------------------------------------------ softmax cross-entropy + gradient + top-k hits, one launch
// nn.CrossEntropyLoss() (mean over the batch, no smoothing) on fp32 logits [B,N] and int64 targets [B]; one workgroup of 16 waves,
// wave w takes rows w, w + 16, ...  Per row: m = max z; e_j = expf(z_j - m) summed in double (lane-strided, then the shuffle tree);
// loss_b = m + log(sum) - z_t in double; dlogits = (e_j / sum - [j == t]) / B; rank = #{z_j > z_t} + #{j < t : z_j == z_t}.
// A target outside [0, N) sets bit 0 of the flag word; its row adds nothing to the loss or the counts, its gradient row is zero and
// no logit is read at the target's index.  The row losses are added wave by wave in row order, then the 16 waves in order.
#define XENT_WAVES 16
__global__ __launch_bounds__(64 * XENT_WAVES) void softmax_xent_kernel(const float *__restrict__ z, const long long *__restrict__ targets, int B,
                                                                        int N, float *__restrict__ dz, hh_xent_result *__restrict__ result)
{
    __shared__ double sh_loss[XENT_WAVES];
    __shared__ int sh_cnt[XENT_WAVES][3];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float invB = 1.0f / (float)B;
    double loss = 0.0;
    int top1 = 0, top5 = 0, bad = 0;
    for (int b = wave; b < B; b += XENT_WAVES) {
        const float *row = z + (size_t)b * N;
        float *drow = dz ? dz + (size_t)b * N : nullptr;
        const long long t = targets[b];
        if (t < 0 || t >= N) {
            bad = 1;
            if (drow) for (int j = lane; j < N; j += 64) drow[j] = 0.f;
            continue;
        }
        const float zt = row[t];
        float m = -INFINITY;
        int above = 0;
        for (int j = lane; j < N; j += 64) {
            const float v = row[j];
            m = fmaxf(m, v);
            above += (v > zt) || (v == zt && j < (int)t);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { m = fmaxf(m, __shfl_xor(m, o, 64)); above += __shfl_xor(above, o, 64); }
        double sum = 0.0;
        for (int j = lane; j < N; j += 64) sum += (double)expf(row[j] - m);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);  // (a + b is commutative: every lane ends with the same bits)
        loss += ((double)m + log(sum)) - (double)zt;
        top1 += above < 1;
        top5 += above < 5;
        if (drow) {
            const float inv = (float)(1.0 / sum);
            for (int j = lane; j < N; j += 64) {
                const float p = expf(row[j] - m) * inv;
                drow[j] = (p - (j == (int)t ? 1.0f : 0.0f)) * invB;
            }
        }
    }
    if (lane == 0) { sh_loss[wave] = loss; sh_cnt[wave][0] = top1; sh_cnt[wave][1] = top5; sh_cnt[wave][2] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        int c1 = 0, c5 = 0, f = 0;
        for (int w = 0; w < XENT_WAVES; ++w) { s += sh_loss[w]; c1 += sh_cnt[w][0]; c5 += sh_cnt[w][1]; f |= sh_cnt[w][2]; }
        hh_xent_result r;
        r.loss = (float)(s / (double)B); r.top1 = c1; r.top5 = c5; r.flags = (unsigned)f;
        *result = r;
    }
}
hipError_t launch_softmax_xent(const float *logits, const long long *targets, int B, int N, float *dlogits, hh_xent_result *result, hipStream_t s)
{
    hipLaunchKernelGGL(softmax_xent_kernel, dim3(1), dim3(64 * XENT_WAVES), 0, s, logits, targets, B, N, dlogits, result);
    return hipGetLastError();
}
