// Exponential moving average of the weights on the optimizer table: fused into the step launch, a stand-alone update for any other
// optimizer, and a one-launch swap of weights and average.  The rule is ema_math.h's (this file is built with -ffp-contract=off).
//
// Fused step: optim_step_kernel's walk (optim_math.h) with a fifth stream.  The new p is still in registers when it is stored, so the
// average costs one read and one write of itself and no further read of p.  The same chunk list, the same 16-byte / scalar split with
// the average's address in the alignment test; rows without an average (row_of < 0) are stepped as by optim_step_kernel.  Tensors the
// optimizer does not step (frozen parameters, floating-point buffers) are (value, ema) rows in a second chunk list behind the first,
// walked by the workgroups blockIdx.x >= nchunks of the same launch.  p, gradient, state and counter bits are optim_step_kernel's.
//
// Skip: *found_inf != 0 -> every workgroup of every kernel here returns before its first store; average and counter keep their bits.
//
// Counter (int64 device scalar, torch's n_averaged): optim.hip's RULE for step counters -- no workgroup reads a counter that a
// workgroup of the same launch has advanced.  The update kernels only read it; the one-workgroup tail launch behind them
// (optim_ema_advance_kernel: the step counters as optim_advance_steps_kernel, then the EMA counter) adds 1.
#include "kernels.h"
#include "ema_math.h"

template <int ALGO>
__global__ __launch_bounds__(OPTIM_THREADS) void optim_step_ema_kernel(const OptimTensor *__restrict__ tensors, const OptimGroup *__restrict__ groups,
                                                                       const OptimChunk *__restrict__ chunks, int nchunks,
                                                                       const float *__restrict__ grad_scale, const float *__restrict__ found_inf,
                                                                       const EmaRow *__restrict__ rows, const int *__restrict__ row_of,
                                                                       const OptimChunk *__restrict__ only_chunks, double decay, int warmup,
                                                                       const long long *__restrict__ n_averaged)
{
    if (found_inf && *found_inf != 0.0f) return;  // a skipped step: before any store
    __shared__ OptimCoefs sh;
    __shared__ EmaCoef she;
    const bool only = (int)blockIdx.x >= nchunks;  // (uniform over the workgroup)
    const OptimChunk ck = only ? only_chunks[blockIdx.x - nchunks] : chunks[blockIdx.x];
    OptimTensor t = {};
    if (!only) t = tensors[ck.tensor];
    if (threadIdx.x == 0) {
        she = ema_coef(decay, warmup, *n_averaged);
        if (!only) {
            const OptimGroup gr = groups[t.group];
            const double step = t.step ? (double)*t.step + 1.0 : 1.0;
            sh = optim_coefs(ALGO, gr.lr, gr.beta1, gr.beta2, gr.eps, gr.weight_decay, gr.momentum, gr.nesterov, step);
        }
    }
    __syncthreads();
    const EmaCoef ec = she;
    if (only) {
        ema_chunk_walk<false>(rows[ck.tensor], ck.chunk, ec, (int)threadIdx.x);
        return;
    }
    const OptimCoefs c = sh;
    const bool unscale = grad_scale != nullptr;
    const int row = row_of[ck.tensor];
    const EmaFifth fifth = {row >= 0 ? rows[row].ema : nullptr, ec};
    optim_chunk_update<ALGO, EmaFifth>(t, ck.chunk, c, unscale, unscale ? *grad_scale : 1.0f, (int)threadIdx.x, fifth);
}

// the stand-alone update: one launch over the rows' chunks
__global__ __launch_bounds__(OPTIM_THREADS) void ema_update_kernel(const EmaRow *__restrict__ rows, const OptimChunk *__restrict__ chunks, double decay,
                                                                   int warmup, const long long *__restrict__ n_averaged,
                                                                   const float *__restrict__ found_inf)
{
    if (found_inf && *found_inf != 0.0f) return;
    const OptimChunk ck = chunks[blockIdx.x];
    ema_chunk_walk<false>(rows[ck.tensor], ck.chunk, ema_coef(decay, warmup, *n_averaged), (int)threadIdx.x);
}

__global__ __launch_bounds__(OPTIM_THREADS) void ema_swap_kernel(const EmaRow *__restrict__ rows, const OptimChunk *__restrict__ chunks)
{
    const OptimChunk ck = chunks[blockIdx.x];
    ema_chunk_walk<true>(rows[ck.tensor], ck.chunk, EmaCoef{0.f, 0}, (int)threadIdx.x);
}

// the tail launch of the header comment: one workgroup, after every read of the counters
__global__ __launch_bounds__(OPTIM_THREADS) void optim_ema_advance_kernel(const OptimTensor *__restrict__ tensors, int ntensors,
                                                                        long long *__restrict__ n_averaged, const float *__restrict__ found_inf)
{
    if (found_inf && *found_inf != 0.0f) return;
    for (int i = threadIdx.x; i < ntensors; i += OPTIM_THREADS) {
        float *step = tensors[i].step;
        if (step) *step = *step + 1.0f;
    }
    if (threadIdx.x == 0) *n_averaged = *n_averaged + 1;
}

hipError_t launch_optim_step_ema(int algo, const OptimTensor *tensors, int ntensors, const OptimGroup *groups, const OptimChunk *chunks, int nchunks,
                                 const float *grad_scale, const float *found_inf, int advance_steps, const EmaRow *rows, const int *row_of,
                                 const OptimChunk *only_chunks, int nonly, double decay, int warmup, long long *n_averaged, hipStream_t s)
{
    const dim3 grid(nchunks + nonly), block(OPTIM_THREADS);
    if (algo != HH_OPTIM_ADAM && algo != HH_OPTIM_ADAMW && algo != HH_OPTIM_SGD) return hipErrorInvalidValue;
    if (nchunks + nonly > 0) {
        if (algo == HH_OPTIM_ADAM)
            hipLaunchKernelGGL(optim_step_ema_kernel<HH_OPTIM_ADAM>, grid, block, 0, s, tensors, groups, chunks, nchunks, grad_scale, found_inf, rows, row_of,
                               only_chunks, decay, warmup, n_averaged);
        else if (algo == HH_OPTIM_ADAMW)
            hipLaunchKernelGGL(optim_step_ema_kernel<HH_OPTIM_ADAMW>, grid, block, 0, s, tensors, groups, chunks, nchunks, grad_scale, found_inf, rows, row_of,
                               only_chunks, decay, warmup, n_averaged);
        else
            hipLaunchKernelGGL(optim_step_ema_kernel<HH_OPTIM_SGD>, grid, block, 0, s, tensors, groups, chunks, nchunks, grad_scale, found_inf, rows, row_of,
                               only_chunks, decay, warmup, n_averaged);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(optim_ema_advance_kernel, dim3(1), block, 0, s, tensors, advance_steps ? ntensors : 0, n_averaged, found_inf);
    return hipGetLastError();
}

hipError_t launch_ema_update(const EmaRow *rows, const OptimChunk *chunks, int nchunks, double decay, int warmup, long long *n_averaged,
                             const float *found_inf, hipStream_t s)
{
    if (nchunks > 0) {
        hipLaunchKernelGGL(ema_update_kernel, dim3(nchunks), dim3(OPTIM_THREADS), 0, s, rows, chunks, decay, warmup, n_averaged, found_inf);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(optim_ema_advance_kernel, dim3(1), dim3(OPTIM_THREADS), 0, s, (const OptimTensor *)nullptr, 0, n_averaged, found_inf);
    return hipGetLastError();
}

hipError_t launch_ema_swap(const EmaRow *rows, const OptimChunk *chunks, int nchunks, hipStream_t s)
{
    if (nchunks <= 0) return hipSuccess;
    hipLaunchKernelGGL(ema_swap_kernel, dim3(nchunks), dim3(OPTIM_THREADS), 0, s, rows, chunks);
    return hipGetLastError();
}
