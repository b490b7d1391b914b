// Evaluation of the classifier on the GPU: top-k, rank and loss of every row of a batch of logits, and the running state of a whole
// evaluation (the rule is written at hh_cls_score_batch in include/hhrnet.h; the layout, the order and the host twin are
// cls_score_math.h).
//
// cls_score_kernel<REG>: one wave per row, CLS_WAVES = 4 rows per workgroup, grid ceil(B / 4): B x N is small (32 x 1000 fp32 is 128 KB),
//   the launch is latency-bound, so the rows run side by side instead of queueing in one workgroup as the training tail's do.  Lane l
//   owns the elements j = l, l + 64, ...  REG: N <= HH_CLS_ROW_REGS, the row is loaded once into CLS_REG = 16 registers per lane and
//   every pass runs on them; otherwise every pass reads the row again (it stays in L2: a row of 65536 is 256 KB).
//   Passes: max + non-finite test; the double sum of expf(z - m), lane-strided then the xor tree (softmax_xent_kernel's order); the rank
//   count; k_eff arg-max rounds.  Round r takes the first element in the rule's order that comes AFTER round r - 1's winner, so no
//   "taken" mask is kept: per lane a scan in ascending j, then a 6-step butterfly over (z, j), a total order, so every lane ends on the
//   same winner; lane r keeps it and writes entry r.
//   There is no barrier and no LDS.  With an accumulator lane 0 leaves the row's double loss and status word in the call scratch and adds
//   the row to per_class / conf with vector atomics (integer: order-free).
// cls_fold_kernel: one wave, launched behind it on the same stream: the counters by a lane-strided sum, loss_sum by adding the scratch
//   losses one at a time in ascending row order (64 at a time through the wave, read lane by lane), then the scratch is zeroed again.
#include "kernels.h"
#include "cls_score_math.h"

// f(z_j, j) for the lane's elements in ascending j
template <bool REG, class F> __device__ __forceinline__ void cls_each(const float (&v)[CLS_REG], const float *__restrict__ row, int N, int lane, F f)
{
    if (REG) {
#pragma unroll
        for (int i = 0; i < CLS_REG; ++i) {
            const int j = lane + 64 * i;
            if (j < N) f(v[i], j);
        }
    } else {
        for (int j = lane; j < N; j += 64) f(row[j], j);
    }
}

template <bool REG>
__global__ __launch_bounds__(CLS_THREADS) void cls_score_kernel(const float *__restrict__ z, const long long *__restrict__ targets, int B, int N, int k,
                                                                void *acc, int32_t *__restrict__ topk_idx, float *__restrict__ topk_prob,
                                                                int32_t *__restrict__ rank, float *__restrict__ row_loss)
{
    const int lane = threadIdx.x & 63, b = blockIdx.x * CLS_WAVES + (threadIdx.x >> 6);
    if (b >= B) return;  // (whole waves leave: nothing below synchronises across waves)
    const float *row = z + (size_t)b * N;
    const int keff = k < N ? k : N;
    float v[CLS_REG];
    if (REG) {
#pragma unroll
        for (int i = 0; i < CLS_REG; ++i) {
            const int j = lane + 64 * i;
            v[i] = j < N ? row[j] : cls_neg_inf();  // j < N: inside the row
        }
    }
    float m = cls_neg_inf();
    bool bad = false;
    cls_each<REG>(v, row, N, lane, [&](float zj, int) { bad |= cls_bad_value(zj); m = fmaxf(m, zj); });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    bad |= !(m > cls_neg_inf());
    const bool nonfinite = __ballot(bad) != 0ull;  // (wave-uniform from here on)

    const bool has_t = targets != nullptr;
    const long long t = has_t ? targets[b] : -1;
    const bool t_ok = has_t && t >= 0 && t < N;
    int st = 0, rk = -1, my_idx = -1;
    float my_prob = 0.f;
    double loss = 0.0;
    int top0 = -1;
    if (nonfinite) {
        st = CLS_ST_NONFINITE;
    } else {
        double sum = 0.0;
        cls_each<REG>(v, row, N, lane, [&](float zj, int) { sum += (double)expf(zj - m); });
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);  // (a + b is commutative: every lane ends with the same bits)
        float pz = 0.f, my_z = 0.f;
        int pj = -1;
        for (int r = 0; r < keff; ++r) {
            float bz = 0.f;
            int bj = -1;
            cls_each<REG>(v, row, N, lane, [&](float zj, int j) {
                const bool cand = pj < 0 || cls_before(pz, pj, zj, j);
                if (cand && (bj < 0 || zj > bz)) bz = zj, bj = j;  // (ascending j: an equal later one does not replace)
            });
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float oz = __shfl_xor(bz, o, 64);
                const int oj = __shfl_xor(bj, o, 64);
                if (oj >= 0 && (bj < 0 || cls_before(oz, oj, bz, bj))) bz = oz, bj = oj;
            }  // (r < k_eff <= N: some lane had a candidate, so bj >= 0 on every lane)
            pz = bz, pj = bj;
            if (r == 0) top0 = bj;
            if (lane == r) my_idx = bj, my_z = bz;
        }
        if (lane < keff) my_prob = (float)((double)expf(my_z - m) / sum);
        if (has_t && !t_ok) {
            st = CLS_ST_BAD_TARGET;
        } else if (t_ok) {
            const float zt = row[t];  // 0 <= t < N
            int above = 0;
            cls_each<REG>(v, row, N, lane, [&](float zj, int j) { above += cls_before(zj, j, zt, (int)t); });
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) above += __shfl_xor(above, o, 64);
            rk = above;
            loss = ((double)m + log(sum)) - (double)zt;
            st = CLS_ST_SCORED | (rk < 1 ? CLS_ST_TOP1 : 0) | (rk < keff ? CLS_ST_TOPK : 0);
        }
    }
    if (lane < k) {  // k <= HH_CLS_TOPK_MAX < 64; entry b * k + lane < B * k
        if (topk_idx) topk_idx[(size_t)b * k + lane] = my_idx;
        if (topk_prob) topk_prob[(size_t)b * k + lane] = my_prob;
    }
    if (lane == 0) {
        if (rank) rank[b] = rk;
        if (row_loss) row_loss[b] = (float)loss;
        if (acc && has_t) {
            const ClsAcc a = cls_acc_view(acc, N);
            if (a.ok) {  // the header describes the layout this call assumes: b < B <= HH_CLS_MAX_B, t < N, top0 < N
                a.status[b] = st, a.loss[b] = loss;
                if (st & CLS_ST_SCORED) {
                    atomicAdd(a.per_class + t, 1);
                    if (st & CLS_ST_TOP1) atomicAdd(a.per_class + (size_t)N + t, 1);
                    if (st & CLS_ST_TOPK) atomicAdd(a.per_class + (size_t)2 * N + t, 1);
                    if (a.conf) atomicAdd(a.conf + (size_t)t * N + top0, 1);
                }
            }
        }
    }
}

__global__ __launch_bounds__(64) void cls_fold_kernel(void *acc, int B, int N)
{
    const int lane = threadIdx.x;
    const ClsAcc a = cls_acc_view(acc, N);
    if (!a.ok) {
        if (lane == 0) a.hdr->flags |= HH_CLS_LAYOUT;
        return;
    }
    int rows = 0, top1 = 0, topk = 0, badt = 0, nonf = 0;
    double s = a.hdr->loss_sum;
    for (int b0 = 0; b0 < B; b0 += 64) {  // (the same trip count on every lane)
        const int b = b0 + lane;
        const int st = b < B ? a.status[b] : 0;  // B <= HH_CLS_MAX_B = the scratch's length
        const double l = st & CLS_ST_SCORED ? a.loss[b] : 0.0;
        rows += (st & CLS_ST_SCORED) != 0, top1 += (st & CLS_ST_TOP1) != 0, topk += (st & CLS_ST_TOPK) != 0;
        badt += (st & CLS_ST_BAD_TARGET) != 0, nonf += (st & CLS_ST_NONFINITE) != 0;
#pragma unroll
        for (int i = 0; i < 64; ++i) {  // every lane forms the same sum: rows b0 .. b0 + 63 in order, the unscored ones skipped
            const int si = __builtin_amdgcn_readlane(st, i);  // (a constant lane: one scalar read each, no LDS crossbar round trip)
            const double li = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(l), i), __builtin_amdgcn_readlane(__double2loint(l), i));
            if (si & CLS_ST_SCORED) s += li;
        }
        if (b < B) a.status[b] = 0, a.loss[b] = 0.0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        rows += __shfl_xor(rows, o, 64), top1 += __shfl_xor(top1, o, 64), topk += __shfl_xor(topk, o, 64);
        badt += __shfl_xor(badt, o, 64), nonf += __shfl_xor(nonf, o, 64);
    }
    if (lane == 0) {
        hh_cls_eval_acc *h = a.hdr;
        h->rows += rows, h->top1 += top1, h->topk += topk, h->bad_target += badt, h->nonfinite += nonf;
        h->loss_sum = s;
        h->flags |= (badt ? HH_CLS_BAD_TARGET : 0) | (nonf ? HH_CLS_NONFINITE : 0);
    }
}

__global__ void cls_reset_kernel(hh_cls_eval_acc *h, int N, int with_confusion)
{
    if (threadIdx.x == 0) h->N = N, h->with_confusion = with_confusion;
}

hipError_t launch_cls_eval_reset(void *acc, int N, int with_confusion, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(acc, 0, cls_acc_bytes(N, with_confusion), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cls_reset_kernel, dim3(1), dim3(64), 0, s, static_cast<hh_cls_eval_acc *>(acc), N, with_confusion);
    return hipGetLastError();
}

hipError_t launch_cls_score(const float *logits, const long long *targets, int B, int N, int k, void *acc, int32_t *topk_idx, float *topk_prob,
                            int32_t *rank, float *row_loss, hipStream_t s)
{
    if (B == 0) return hipSuccess;
    const dim3 grid((B + CLS_WAVES - 1) / CLS_WAVES), block(CLS_THREADS);
    if (N <= HH_CLS_ROW_REGS)
        hipLaunchKernelGGL(cls_score_kernel<true>, grid, block, 0, s, logits, targets, B, N, k, acc, topk_idx, topk_prob, rank, row_loss);
    else
        hipLaunchKernelGGL(cls_score_kernel<false>, grid, block, 0, s, logits, targets, B, N, k, acc, topk_idx, topk_prob, rank, row_loss);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !acc || !targets) return e;
    hipLaunchKernelGGL(cls_fold_kernel, dim3(1), dim3(64), 0, s, acc, B, N);
    return hipGetLastError();
}

void cls_score_host(const float *logits, const long long *targets, int B, int N, int k, void *acc, int32_t *topk_idx, float *topk_prob,
                    int32_t *rank, float *row_loss)
{
    cls_batch_host(logits, targets, B, N, k, acc, topk_idx, topk_prob, rank, row_loss);
}
