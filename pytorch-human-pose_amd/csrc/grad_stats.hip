// Gradient statistics and clipping by global norm over the optimizer's device-resident table (optim.hip): what
// torch.nn.utils.clip_grad_norm_ and a per-layer gradient logger do over ~900 tensors, as one read of the gradients.  The
// arithmetic, its fixed summation order and the NaN / inf rule are in grad_stats_math.h (shared with a host build); this file is built
// with -ffp-contract=off.
//
// grad_stats_kernel   one workgroup per entry of the chunk list.  One read of the chunk's gradients; optionally g *= *inv_scale in
//                     place and *found_inf = 1 (grads_nonfinite_kernel's stores, bit for bit); one GradPartial per chunk, of the
//                     value that is stored.  The workgroup of a tensor's chunk 0 also records its own index as the tensor's first.
// grad_tensor_kernel  one workgroup per tensor: its chunks' records in a fixed order -> the tensor's fp32 row and its fp64 sum of
//                     squares.  A tensor of 1152 chunks takes five rounds of the workgroup.
// grad_totals_kernel  one workgroup: total_l2 and total_inf from the per-tensor figures.
// grad_clip_kernel    one workgroup per chunk: coef = min(max_norm / (total + 1e-6f), 1) from the totals (every workgroup forms the
//                     same fp32 value; workgroup 0 also stores it), g = g * coef.  Every workgroup returns before its first gradient
//                     store when coef >= 1 (multiplying by 1.0f is the identity) or when *found_inf != 0 (that step is skipped).
//
// Hand-over between the four is the launch boundary on one stream: no workgroup reads what a workgroup of its own launch wrote, so
// there is no ticket, no flag and no fence, and no floating-point atomic anywhere.
#include "kernels.h"
#include "grad_stats_math.h"

// lane 0 of every wave ends with the wave's record (grad_wave_tree's pairs), then thread 0 with the block's (grad_block_combine)
__device__ __forceinline__ GradPartial grad_block_reduce(GradPartial a, GradPartial *sh)
{
#pragma unroll
    for (int off = GRAD_WAVE / 2; off > 0; off >>= 1) {
        GradPartial b;
        b.sumsq = __shfl_down(a.sumsq, off, GRAD_WAVE);
        b.abssum = __shfl_down(a.abssum, off, GRAD_WAVE);
        b.absmax = __shfl_down(a.absmax, off, GRAD_WAVE);
        b.nonfinite = __shfl_down(a.nonfinite, off, GRAD_WAVE);
        a = grad_combine(a, b);
    }
    if ((threadIdx.x & (GRAD_WAVE - 1)) == 0) sh[threadIdx.x / GRAD_WAVE] = a;
    __syncthreads();
    return grad_block_combine(sh[0], sh[1], sh[2], sh[3]);  // (every thread forms it; thread 0's copy is the one that is stored)
}

__global__ __launch_bounds__(OPTIM_THREADS) void grad_stats_kernel(const OptimTensor *__restrict__ tensors, const OptimChunk *__restrict__ chunks,
                                                                   const float *__restrict__ inv_scale, float *__restrict__ found_inf,
                                                                   GradPartial *__restrict__ parts, int *__restrict__ first)
{
    __shared__ GradPartial sh[GRAD_WAVES];
    const OptimChunk ck = chunks[blockIdx.x];
    const OptimTensor t = tensors[ck.tensor];
    const float s = inv_scale ? *inv_scale : 1.0f;
    bool bad;
    const GradPartial mine = grad_chunk_stats(t, ck.chunk, s != 1.0f, s, (int)threadIdx.x, &bad);
    if (bad && found_inf) *found_inf = 1.0f;
    const GradPartial all = grad_block_reduce(mine, sh);
    if (threadIdx.x == 0) {
        parts[blockIdx.x] = all;
        if (ck.chunk == 0) first[ck.tensor] = (int)blockIdx.x;
    }
}

__global__ __launch_bounds__(OPTIM_THREADS) void grad_tensor_kernel(const OptimTensor *__restrict__ tensors, const GradPartial *__restrict__ parts,
                                                                    const int *__restrict__ first, GradRow *__restrict__ rows,
                                                                    double *__restrict__ tensor_sumsq)
{
    __shared__ GradPartial sh[GRAD_WAVES];
    const long long numel = tensors[blockIdx.x].numel;
    const int nparts = (int)((numel + OPTIM_CHUNK - 1) / OPTIM_CHUNK);
    // (a tensor without elements has no chunk and no `first` entry: nothing is read for it)
    const GradPartial mine = grad_tensor_share(nparts ? parts + first[blockIdx.x] : parts, nparts, (int)threadIdx.x);
    const GradPartial all = grad_block_reduce(mine, sh);
    if (threadIdx.x == 0) {
        rows[blockIdx.x] = grad_row(all, numel);
        tensor_sumsq[blockIdx.x] = all.sumsq;
    }
}

__global__ __launch_bounds__(OPTIM_THREADS) void grad_totals_kernel(const GradRow *__restrict__ rows, const double *__restrict__ tensor_sumsq,
                                                                    int ntensors, GradTotals *__restrict__ totals)
{
    __shared__ GradPartial sh[GRAD_WAVES];
    GradPartial mine = grad_partial_zero();
    for (int i = threadIdx.x; i < ntensors; i += OPTIM_THREADS)
        mine = grad_combine(mine, GradPartial{tensor_sumsq[i], 0.0, rows[i].absmax, 0});
    const GradPartial all = grad_block_reduce(mine, sh);
    if (threadIdx.x == 0) {
        float l2, inf;
        grad_totals(all, &l2, &inf);
        totals->l2 = l2;
        totals->inf = inf;
    }
}

__global__ __launch_bounds__(OPTIM_THREADS) void grad_clip_kernel(const OptimTensor *__restrict__ tensors, const OptimChunk *__restrict__ chunks,
                                                                  int nchunks, GradTotals *totals, float max_norm, int norm_type,
                                                                  const float *__restrict__ found_inf)
{
    // (totals->coef is only ever stored here and never loaded by a kernel, so workgroup 0's store races with nothing)
    const float coef = grad_clip_coef(max_norm, norm_type == GRAD_NORM_INF ? totals->inf : totals->l2);
    if (blockIdx.x == 0 && threadIdx.x == 0) totals->coef = coef;
    if (found_inf && *found_inf != 0.0f) return;  // a skipped step: the gradients stay as the unscale pass left them
    if (coef >= 1.0f || (int)blockIdx.x >= nchunks) return;  // (a table without elements still gets its coefficient: one workgroup)
    const OptimChunk ck = chunks[blockIdx.x];
    grad_chunk_scale(tensors[ck.tensor], ck.chunk, coef, (int)threadIdx.x);
}

hipError_t launch_grad_stats(const OptimTensor *tensors, int ntensors, const OptimChunk *chunks, int nchunks, const float *inv_scale,
                             float *found_inf, void *work, hipStream_t s)
{
    const GradWork w = grad_work(work, ntensors, nchunks);
    const dim3 block(OPTIM_THREADS);
    hipError_t e = hipSuccess;
    if (nchunks > 0) {
        hipLaunchKernelGGL(grad_stats_kernel, dim3(nchunks), block, 0, s, tensors, chunks, inv_scale, found_inf, w.parts, w.first);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (ntensors > 0) {
        hipLaunchKernelGGL(grad_tensor_kernel, dim3(ntensors), block, 0, s, tensors, (const GradPartial *)w.parts, (const int *)w.first, w.rows,
                           w.tensor_sumsq);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    // (an empty table has the totals 0, 0)
    hipLaunchKernelGGL(grad_totals_kernel, dim3(1), block, 0, s, (const GradRow *)w.rows, (const double *)w.tensor_sumsq, ntensors, w.totals);
    return hipGetLastError();
}

hipError_t launch_grad_clip(const OptimTensor *tensors, int ntensors, const OptimChunk *chunks, int nchunks, float max_norm, int norm_type,
                            const float *found_inf, void *work, hipStream_t s)
{
    const GradWork w = grad_work(work, ntensors, nchunks);
    hipLaunchKernelGGL(grad_clip_kernel, dim3(nchunks > 0 ? nchunks : 1), dim3(OPTIM_THREADS), 0, s, tensors, chunks, nchunks, w.totals, max_norm,
                       norm_type, found_inf);
    return hipGetLastError();
}
