// COCO keypoint scoring on the GPU: computeOks + evaluateImg of keypoints/coco_eval.py for every image, area range and threshold in ONE
// launch over the packed tables (CocoTables; the arithmetic and the matching walk are coco_eval_math.h, shared with the host).
//
// coco_eval_kernel<MODE>: grid (I), one workgroup of COCO_THREADS = 256 threads per image.
//   Phase 1: the threads compute the image's D x G OKS values into LDS, one pair per thread per step (D <= 32, G <= 128: at most 16 steps,
//            32 KB of fp64); the ground truths' areas and flags and the detections' areas are staged next to them.  Barrier.
//   Phase 2: lane a * T + t < A * T <= 64 of the first wave runs the serial walk of (area range a, threshold t) with its taken-set in two
//            64-bit registers and writes its D rows of dt_match / dt_ignore; lane t = 0 of each area also writes that area's gt_ignore.
// MODE 0 (hh_coco_evaluate) does both and the OKS matrix never reaches HBM; MODE 1 (hh_coco_oks) stores phase 1 to the caller's buffer and
// stops; MODE 2 (hh_coco_match) loads the caller's matrix instead of phase 1.  Every output element in range is written exactly once by
// exactly one thread, unconditionally: no atomics, no counters, nothing to clear and nothing carried between calls.  The launch is a few
// million fp64 exp for a val2017-sized set; occupancy is not tuned, the point is to remove the interpreter loops.
#include "kernels.h"
#include "coco_eval_math.h"

enum { COCO_FUSED = 0, COCO_OKS_ONLY = 1, COCO_MATCH_ONLY = 2 };

template <int MODE>
__global__ __launch_bounds__(COCO_THREADS) void coco_eval_kernel(const CocoTables t, const double *__restrict__ oks_in, double *__restrict__ oks_out,
                                                                 int32_t *__restrict__ dt_match, uint8_t *__restrict__ dt_ignore,
                                                                 uint8_t *__restrict__ gt_ignore)
{
    __shared__ double s_oks[HH_COCO_MAX_DET * HH_COCO_MAX_GT];
    __shared__ double s_gt_area[HH_COCO_MAX_GT], s_dt_area[HH_COCO_MAX_DET];
    __shared__ uint8_t s_gt_flags[HH_COCO_MAX_GT];
    const int i = blockIdx.x, tid = threadIdx.x;  // i < I = the grid's size
    const int d0 = t.dt_off[i], D = t.dt_off[i + 1] - d0, g0 = t.gt_off[i], G = t.gt_off[i + 1] - g0;  // D <= 32, G <= 128 (checked by the caller)
    const int pairs = D * G;                                                                               // <= 4096 = the LDS array
    for (int p = tid; p < pairs; p += COCO_THREADS) {
        double v;
        if (MODE == COCO_MATCH_ONLY) {
            v = oks_in[t.oks_off[i] + p];  // p < D * G = oks_off[i + 1] - oks_off[i]
        } else {
            const int d = p / G, g = p % G;  // d0 + d < N, g0 + g < M
            v = coco_oks_pair(t.dt_xy + (size_t)(d0 + d) * t.K * 2, t.gt_xyv + (size_t)(g0 + g) * t.K * 3, t.gt_bbox + (size_t)(g0 + g) * 4, t.gt_area[g0 + g],
                              t.vars, t.K);
        }
        if (MODE == COCO_OKS_ONLY) oks_out[t.oks_off[i] + p] = v;
        else s_oks[p] = v;
    }
    if (MODE == COCO_OKS_ONLY) return;
    if (tid < G) s_gt_area[tid] = t.gt_area[g0 + tid], s_gt_flags[tid] = t.gt_flags[g0 + tid];  // G <= 128 < COCO_THREADS
    if (tid < D) s_dt_area[tid] = t.dt_area[d0 + tid];
    __syncthreads();
    if (tid >= t.A * t.T) return;  // A * T <= 64: the first wave
    const int a = tid / t.T, k = tid % t.T;
    const double lo = t.area_rng[2 * a], hi = t.area_rng[2 * a + 1];
    const CocoGtSets s = coco_gt_sets(s_gt_area, s_gt_flags, G, lo, hi);
    if (k == 0) coco_store_gt_ignore(s, G, gt_ignore + (size_t)a * t.M + g0);  // a < A, g0 + G <= M
    const size_t o = ((size_t)a * t.T + k) * t.N + d0;  // rows o .. o + D - 1 of [A, T, N]: d0 + D <= N
    coco_match_walk(s_oks, D, G, s, t.thr[k], s_dt_area, lo, hi, g0, dt_match + o, dt_ignore + o);
}

hipError_t launch_coco_eval(int mode, const CocoTables &dev, const double *oks_in, double *oks_out, int32_t *dt_match, uint8_t *dt_ignore, uint8_t *gt_ignore,
                            hipStream_t s)
{
    if (dev.I == 0) return hipSuccess;
    const dim3 grid(dev.I), block(COCO_THREADS);
    if (mode == COCO_FUSED) hipLaunchKernelGGL(coco_eval_kernel<COCO_FUSED>, grid, block, 0, s, dev, oks_in, oks_out, dt_match, dt_ignore, gt_ignore);
    else if (mode == COCO_OKS_ONLY) hipLaunchKernelGGL(coco_eval_kernel<COCO_OKS_ONLY>, grid, block, 0, s, dev, oks_in, oks_out, dt_match, dt_ignore, gt_ignore);
    else hipLaunchKernelGGL(coco_eval_kernel<COCO_MATCH_ONLY>, grid, block, 0, s, dev, oks_in, oks_out, dt_match, dt_ignore, gt_ignore);
    return hipGetLastError();
}

void coco_eval_host(const CocoTables &t, const double *oks_in, double *oks_out, bool match, int32_t *dt_match, uint8_t *dt_ignore, uint8_t *gt_ignore)
{
    double *scratch = new double[HH_COCO_MAX_DET * HH_COCO_MAX_GT];
    for (int i = 0; i < t.I; ++i) coco_image_host(t, i, oks_in, oks_out, scratch, match, dt_match, dt_ignore, gt_ignore);
    delete[] scratch;
}
