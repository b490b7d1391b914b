// Target heatmaps of the training step rendered on the GPU: the HeatmapGenerator of keypoints/datasets/coco.py:77-121 as a gather.
//
// The reference scatters: per person and joint it takes np.maximum of a (6 sigma + 3)^2 window of the map with a float64 bump
// table and stores the result as float32.  With integer joint positions (JointsGenerator, coco.py:124-137, runs first) and an
// integer reach R = 3 sigma + 1 the window of a joint at (xp, yp) is [xp - R, xp + R] x [yp - R, yp + R] clipped to the map, and
// pixel (x, y) reads table[y - yp + R][x - xp + R].  Rounding to float32 is monotone and max does not depend on the order, so the
// maximum over the float32 table entries equals the reference's map bit for bit.  Every output element is written exactly once
// (pixels no bump reaches get 0): no memset, no atomics, the result does not depend on the launch.
//
// The work is a write stream (178 MB per step at B = 32, K = 17, 128^2 + 256^2), so one workgroup owns a band of rows of one
// (image, joint type) plane: it culls that plane's visible joints to the band into LDS next to the table, then every thread
// walks the survivors (a wave-uniform loop: the LDS reads of a survivor are broadcasts) for its groups of four consecutive
// pixels and stores them as one 16-byte store.  Measured (profiles/train_input.md): both stages of a B = 32 batch in 0.043 ms, 1.63x
// the hipMemsetAsync of the same buffers.  The table reads t[e] are 16 bytes apart from lane to lane and conflict on LDS banks;
// not tuned, the kernel is 0.07 % of the training step.
#include "kernels.h"

#define RENDER_THREADS 256
#define RENDER_ITEMS 4  // groups of four pixels per thread: a band holds at most RENDER_THREADS * RENDER_ITEMS groups

static int render_band_rows(int w)
{
    const int gpr = (w + 3) / 4, fit = RENDER_THREADS * RENDER_ITEMS / gpr;
    return fit < 1 ? 1 : fit > 16 ? 16 : fit;
}

__global__ __launch_bounds__(RENDER_THREADS) void render_heatmaps_kernel(const int32_t *__restrict__ joints, const int32_t *__restrict__ num_people,
                                                                         const float *__restrict__ table, int n, int R, float *__restrict__ out,
                                                                         int P, int K, int h, int w, int band_rows, int vec)
{
    __shared__ float tab[HH_RENDER_MAX_N * HH_RENDER_MAX_N];
    __shared__ int lx[RENDER_THREADS], ly[RENDER_THREADS];
    __shared__ int count;
    const int tid = threadIdx.x, k = blockIdx.y, b = blockIdx.z;
    const int y0 = blockIdx.x * band_rows, y1 = min(h, y0 + band_rows);
    const int gpr = (w + 3) / 4, items = (y1 - y0) * gpr;
    for (int i = tid; i < n * n; i += RENDER_THREADS) tab[i] = table[i];

    int row[RENDER_ITEMS], x4[RENDER_ITEMS];
    float acc[RENDER_ITEMS][4];
#pragma unroll
    for (int it = 0; it < RENDER_ITEMS; ++it) {
        const int item = tid + it * RENDER_THREADS;
        row[it] = y0 + item / gpr;
        x4[it] = (item % gpr) * 4;
        acc[it][0] = acc[it][1] = acc[it][2] = acc[it][3] = 0.f;
    }

    const int np = min(max(num_people[b], 0), P);  // rows beyond num_people[b] are padding
    for (int base = 0; base < np; base += RENDER_THREADS) {
        if (tid == 0) count = 0;
        __syncthreads();  // (also orders the table stores before the first reads)
        const int p = base + tid;
        if (p < np) {
            const int32_t *j = joints + (((size_t)b * P + p) * K + k) * 3;
            const int x = j[0], y = j[1], vis = j[2];
            if (vis > 0 && x >= 0 && x < w && y >= 0 && y < h && y + R >= y0 && y - R < y1) {
                const int s = atomicAdd(&count, 1);  // the order of the list is free: max commutes
                lx[s] = x;
                ly[s] = y;
            }
        }
        __syncthreads();
        const int cnt = count;
        for (int s = 0; s < cnt; ++s) {
            const int px = lx[s] - R, py = ly[s] - R;
#pragma unroll
            for (int it = 0; it < RENDER_ITEMS; ++it) {
                const int dy = row[it] - py, dx = x4[it] - px;
                if (tid + it * RENDER_THREADS < items && (unsigned)dy < (unsigned)n && dx > -4 && dx < n) {
                    const float *t = tab + dy * n + dx;
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if ((unsigned)(dx + e) < (unsigned)n) acc[it][e] = fmaxf(acc[it][e], t[e]);
                }
            }
        }
        __syncthreads();  // everyone has read `count` and the list before the next round resets them
    }

    float *plane = out + ((size_t)b * K + k) * h * w;
#pragma unroll
    for (int it = 0; it < RENDER_ITEMS; ++it) {
        if (tid + it * RENDER_THREADS >= items) continue;
        float *dst = plane + (size_t)row[it] * w + x4[it];
        if (vec) {
            *reinterpret_cast<float4 *>(dst) = make_float4(acc[it][0], acc[it][1], acc[it][2], acc[it][3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (x4[it] + e < w) dst[e] = acc[it][e];
        }
    }
}

hipError_t launch_render_heatmaps(const int32_t *joints, const int32_t *num_people, int B, int P, int K, const float *table, int n, int reach,
                                  float *out, int h, int w, hipStream_t s)
{
    const int band_rows = render_band_rows(w);
    const int vec = w % 4 == 0 && (uintptr_t)out % 16 == 0;  // every group of four pixels is then a 16-byte aligned store
    hipLaunchKernelGGL(render_heatmaps_kernel, dim3((h + band_rows - 1) / band_rows, K, B), dim3(RENDER_THREADS), 0, s, joints, num_people, table, n,
                       reach, out, P, K, h, w, band_rows, vec);
    return hipGetLastError();
}
