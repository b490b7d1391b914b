// Per-image OKS / PCKh against annotations on the GPU, behind hh_decode: match_preds_to_targets + object_OKS / image_OKS (or object_PCKh /
// image_PCKh) of the reference for every image of a batch in ONE launch (the rule is written at hh_pose_score_batch in include/hhrnet.h;
// the arithmetic is pose_score_math.h, shared with the host).
//
// pose_score_kernel: grid (B), one workgroup of POSE_THREADS = 256 threads (4 waves) per image.
//   Phase 1: the threads un-warp the image's P x K x 2 prediction coordinates into LDS (dynamic, sized by the launch for the largest P the
//            call can meet) and the P person scores next to them; a non-finite one raises the image's status bit.  Barrier.
//   Phase 2: wave w takes targets w, w + 4, ...: the target's row [K,3] is staged in the wave's LDS slot, lane p computes val = 1 / D[p,t]
//            serially over k (ascending, so the sum's order is the rule's), a 6-step butterfly over (val, walk rank) finds the prediction the
//            strict-greater walk ends on, lane k computes joint k's term against it, lane 0 sums the terms in ascending k.
//   Phase 3: thread 0 forms the image value from the T object values kept in LDS, ascending t.
// Every output element in range is written exactly once by exactly one thread: no atomics on global memory, nothing to clear, nothing
// carried between calls.  The work per image is a few thousand fp64 operations: the launch is latency-bound and nothing here is tuned for
// throughput; the point is that the score needs no host round trip and no second copy.
#include "kernels.h"
#include "pose_score_math.h"

__global__ __launch_bounds__(POSE_THREADS) void pose_score_kernel(const PoseTables t, int lds_P, double *__restrict__ value, double *__restrict__ obj,
                                                                  double *__restrict__ kpt, int32_t *__restrict__ match, int32_t *__restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ double s_score[HH_POSE_MAX_P], s_obj[HH_POSE_MAX_T];
    __shared__ int s_status;
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;  // i < B = the grid's size
    const int K = t.K, P = pose_num_preds(t, i), t0 = t.t_off[i], T = t.t_off[i + 1] - t0;
    if (P < 0 || P > lds_P || T < 0 || T > HH_POSE_MAX_T) {  // the device tables are not the host copy that was checked: touch nothing they index
        if (tid == 0) status[i] = -1, value[i] = pose_nan();
        return;
    }
    double *s_pxy = reinterpret_cast<double *>(smem);                      // [P, K, 2], P <= lds_P
    double *s_row = s_pxy + (size_t)lds_P * K * 2 + (size_t)wave * K * 4;  // [K, 3] of the wave's target, then its [K] terms
    double *s_term = s_row + (size_t)K * 3;
    const bool fb = pose_fallback(t, i);
    if (tid == 0) s_status = P == 0 && T > 0 ? HH_POSE_NO_PRED : 0;
    __syncthreads();
    bool bad = false;
    for (int e = tid; e < P * K * 2; e += POSE_THREADS) {  // e / (2 K) < P
        const double v = pose_pred_coord(t, i, e / (2 * K), (e / 2) % K, e % 2, fb);
        s_pxy[e] = v;
        bad |= !pose_finite(v);
    }
    if (tid < P) {  // P <= 64
        const double v = pose_pred_score(t, i, tid, fb);
        s_score[tid] = v;
        bad |= !pose_finite(v);
    }
    if (bad) atomicOr(&s_status, HH_POSE_NONFINITE);
    __syncthreads();
    const int st = s_status;  // (the same on every thread: the branches below are uniform)
    if (tid == 0) status[i] = st;
    if (st) {
        for (int j = tid; j < T; j += POSE_THREADS) obj[t0 + j] = pose_nan(), match[t0 + j] = -1;
        for (int e = tid; e < T * K; e += POSE_THREADS) kpt[(size_t)t0 * K + e] = pose_nan();
        if (tid == 0) value[i] = pose_nan();
        return;
    }
    const int rank = lane < P ? pose_rank(s_score, P, lane) : 0;
    for (int j0 = 0; j0 < T; j0 += POSE_WAVES) {  // (the same trip count on every wave: the barriers inside are legal)
        const int j = j0 + wave;
        const bool act = j < T;
        if (act)
            for (int e = lane; e < K * 3; e += 64) s_row[e] = t.t_xyv[(size_t)(t0 + j) * K * 3 + e];
        __syncthreads();
        int n = 0, m = -1;
        bool scored = false;
        if (act) {
            n = pose_visible(s_row, K);  // > 0 (checked by the caller)
            double v = lane < P ? pose_match_val(s_pxy + (size_t)lane * K * 2, s_row, K, n) : 0.0;
            int r = rank;
            m = lane < P ? lane : -1;
            for (int step = 1; step < 64; step <<= 1) {
                const double ov = __shfl_xor(v, step, 64);
                const int orank = __shfl_xor(r, step, 64), om = __shfl_xor(m, step, 64);
                if (om >= 0 && (m < 0 || pose_better(ov, orank, v, r))) v = ov, r = orank, m = om;
            }  // (ranks are distinct, so (val, rank) is a total order and every lane ends on the same holder; m >= 0 as P > 0)
            const double head = t.t_head[t0 + j];
            scored = !(t.metric == HH_POSE_METRIC_PCKH && head == 0.0);
            if (lane < K) {
                const double term = scored ? pose_term(t, s_pxy + (size_t)m * K * 2, s_row, t.t_area[t0 + j], head, lane) : -1.0;
                s_term[lane] = term;
                kpt[(size_t)(t0 + j) * K + lane] = term;
            }
        }
        __syncthreads();
        if (act && lane == 0) {
            const double o = scored ? pose_object(s_term, K, n) : -1.0;
            obj[t0 + j] = o;
            s_obj[j] = o;
            match[t0 + j] = m;
        }
    }
    __syncthreads();
    if (tid == 0) value[i] = pose_image_value(s_obj, T, t.metric);
}

hipError_t launch_pose_score(const PoseTables &t, int max_P, double *value, double *obj, double *kpt, int32_t *match, int32_t *status, hipStream_t s)
{
    if (t.B == 0) return hipSuccess;
    static bool attr_set[64] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (!attr_set[dev & 63]) {
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(pose_score_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)pose_lds_bytes(HH_POSE_MAX_P, HH_POSE_MAX_K));
        if (e != hipSuccess) return e;
        attr_set[dev & 63] = true;
    }
    hipLaunchKernelGGL(pose_score_kernel, dim3(t.B), dim3(POSE_THREADS), pose_lds_bytes(max_P, t.K), s, t, max_P, value, obj, kpt, match, status);
    return hipGetLastError();
}

void pose_score_host(const PoseTables &t, double *value, double *obj, double *kpt, int32_t *match, int32_t *status)
{
    double *pxy = new double[(size_t)HH_POSE_MAX_P * HH_POSE_MAX_K * 2], score[HH_POSE_MAX_P], term[HH_POSE_MAX_K];
    for (int i = 0; i < t.B; ++i) pose_image_host(t, i, pxy, score, term, value, obj, kpt, match, status);
    delete[] pxy;
}
