// Device optimizer step: Adam / AdamW / SGD over every parameter of every param group in ONE launch, with the loss-scale contract
// of torch.amp.GradScaler (grad_scale, found_inf), and the non-finite check over all gradients in one launch.
//
// Semantics: the installed torch's single-tensor implementations (torch/optim/adam.py _single_tensor_adam, sgd.py
// _single_tensor_sgd) with maximize=False, amsgrad=False, dampening=0, restated per element in fp32 (optim_math.h; this file is
// built with -ffp-contract=off, every operation rounds on its own):
//   Adam   g += wd * p                        (L2, only when wd != 0)
//          m += (1 - beta1) * (g - m)         (exp_avg.lerp_)
//          v  = beta2 * v + (1 - beta2) * g*g
//          p -= (lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps)),   bc1 = 1 - beta1^step, bc2 = 1 - beta2^step
//   AdamW  p *= 1 - lr * wd  first (only when wd != 0), no L2 term, then as Adam
//   SGD    g += wd * p;  buf = momentum * buf + g  (buf starts at zero, which gives torch's first step buf = g exactly at
//          dampening 0);  g = nesterov ? g + momentum * buf : buf  (only when momentum != 0);  p -= lr * g
// The hyper-parameters are doubles in the per-group blocks.  1 - beta1, 1 - beta2, 1 - lr * wd, lr / bc1, sqrt(bc2) and the bias
// corrections themselves are computed in fp64 from them and the tensor's step counter, once per workgroup (thread 0, handed over
// in LDS), and only the results are rounded to fp32: a beta2 rounded to fp32 first is off by 5e-5 of 1 - beta2 at step 1.
//
// Grid: blockIdx.x indexes a host-built chunk list; entry = (tensor, chunk of OPTIM_CHUNK = 4096 elements).  A 4.7 M element
// weight gets 1152 workgroups, a 17-element bias one.  A chunk whose four pointers are 16-byte aligned moves float4 (a chunk
// starts 16 KiB into its tensor, so only the tensors' own addresses decide); any other chunk, e.g. a gradient that is a view into a
// DDP bucket at an odd offset, takes the scalar path.  Pure streaming: Adam reads 16 B and writes 12 B per element.
//
// Loss scale: found_inf != 0 -> every workgroup returns before its first store (parameters, state, counters keep their bits).
// Otherwise g / *grad_scale is used and written back to the gradient (as torch's fused optimizers leave it).
//
// Step counters (one fp32 scalar per tensor, torch's state[p]["step"]): RULE -- no workgroup reads a counter that a workgroup of
// the same launch has advanced.  CHOICE -- the update kernel only reads them (this step = counter + 1); a second, one-workgroup
// launch behind it (optim_advance_steps_kernel) adds 1 to each, and returns early on found_inf like the first.
#include "kernels.h"
#include "optim_math.h"

template <int ALGO>
__global__ __launch_bounds__(OPTIM_THREADS) void optim_step_kernel(const OptimTensor *__restrict__ tensors, const OptimGroup *__restrict__ groups,
                                                                   const OptimChunk *__restrict__ chunks, const float *__restrict__ grad_scale,
                                                                   const float *__restrict__ found_inf)
{
    if (found_inf && *found_inf != 0.0f) return;  // a skipped step: before any store
    __shared__ OptimCoefs sh;
    const OptimChunk ck = chunks[blockIdx.x];
    const OptimTensor t = tensors[ck.tensor];
    if (threadIdx.x == 0) {
        const OptimGroup gr = groups[t.group];
        const double step = t.step ? (double)*t.step + 1.0 : 1.0;
        sh = optim_coefs(ALGO, gr.lr, gr.beta1, gr.beta2, gr.eps, gr.weight_decay, gr.momentum, gr.nesterov, step);
    }
    __syncthreads();
    const OptimCoefs c = sh;
    const bool unscale = grad_scale != nullptr;
    optim_chunk_update<ALGO>(t, ck.chunk, c, unscale, unscale ? *grad_scale : 1.0f, (int)threadIdx.x);
}

// the tail launch of the header comment: one workgroup, after every read of the counters
__global__ __launch_bounds__(OPTIM_THREADS) void optim_advance_steps_kernel(const OptimTensor *__restrict__ tensors, int ntensors,
                                                                          const float *__restrict__ found_inf)
{
    if (found_inf && *found_inf != 0.0f) return;
    for (int i = threadIdx.x; i < ntensors; i += OPTIM_THREADS) {
        float *step = tensors[i].step;
        if (step) *step = *step + 1.0f;
    }
}

// _amp_foreach_non_finite_check_and_unscale_ over the table: *found_inf = 1 if any gradient element is inf / NaN (the caller zeroes
// it first; every thread that sees one stores the same 1.0f), and g *= *inv_scale in place unless inv_scale is NULL or holds 1.
__global__ __launch_bounds__(OPTIM_THREADS) void grads_nonfinite_kernel(const OptimTensor *__restrict__ tensors, const OptimChunk *__restrict__ chunks,
                                                                        const float *__restrict__ inv_scale, float *__restrict__ found_inf)
{
    const OptimChunk ck = chunks[blockIdx.x];
    const OptimTensor t = tensors[ck.tensor];
    const float s = inv_scale ? *inv_scale : 1.0f;
    if (optim_chunk_nonfinite(t, ck.chunk, s != 1.0f, s, (int)threadIdx.x)) *found_inf = 1.0f;
}

hipError_t launch_optim_step(int algo, const OptimTensor *tensors, int ntensors, const OptimGroup *groups, const OptimChunk *chunks, int nchunks,
                             const float *grad_scale, const float *found_inf, int advance_steps, hipStream_t s)
{
    if (nchunks <= 0) return hipSuccess;
    const dim3 grid(nchunks), block(OPTIM_THREADS);
    if (algo == HH_OPTIM_ADAM) hipLaunchKernelGGL(optim_step_kernel<HH_OPTIM_ADAM>, grid, block, 0, s, tensors, groups, chunks, grad_scale, found_inf);
    else if (algo == HH_OPTIM_ADAMW) hipLaunchKernelGGL(optim_step_kernel<HH_OPTIM_ADAMW>, grid, block, 0, s, tensors, groups, chunks, grad_scale, found_inf);
    else if (algo == HH_OPTIM_SGD) hipLaunchKernelGGL(optim_step_kernel<HH_OPTIM_SGD>, grid, block, 0, s, tensors, groups, chunks, grad_scale, found_inf);
    else return hipErrorInvalidValue;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !advance_steps) return e;
    hipLaunchKernelGGL(optim_advance_steps_kernel, dim3(1), block, 0, s, tensors, ntensors, found_inf);
    return hipGetLastError();
}

hipError_t launch_grads_nonfinite(const OptimTensor *tensors, const OptimChunk *chunks, int nchunks, const float *inv_scale, float *found_inf,
                                  hipStream_t s)
{
    if (nchunks <= 0) return hipSuccess;
    hipLaunchKernelGGL(grads_nonfinite_kernel, dim3(nchunks), dim3(OPTIM_THREADS), 0, s, tensors, chunks, inv_scale, found_inf);
    return hipGetLastError();
}
