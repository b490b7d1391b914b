// The arithmetic of the gradient statistics and of clipping by global norm (grad_stats.hip), kept apart from the kernels so that the
// same text also compiles for the host (tools/grad_stats_host_check.cpp runs it under the sanitizers): the partial record, one
// thread's walk over one chunk of the optimizer table (optim_math.h), the fixed-order combination of records, the per-tensor row, the
// totals and the clip coefficient.  Compile with -ffp-contract=off: every operation below rounds on its own.
//
// Precision.  Squares and sums are formed in fp64: the product of two fp32 values is exact there, and a sum of n of them is off by at
// most n 2^-53 of itself, so the one rounding that shows is the final one to fp32.  No floating-point atomics: every sum has ONE order.
//   thread   its elements in the order of the walk (16-byte rounds x, y, z, w; then the scalar tail)
//   wave     lane i += lane i + off for off = 32, 16, 8, 4, 2, 1 (grad_wave_tree; lane 0 holds the wave's record)
//   block    (wave 0 + wave 1) + (wave 2 + wave 3)   (grad_block_combine)
//   tensor   thread t of the reduction takes the tensor's chunks t, t + 256, ... in that order, then wave and block as above
//   total    thread t takes tensors t, t + 256, ..., then wave and block as above
//
// NaN / inf rule (that of g.norm(), g.abs().max(), g.abs().mean()): a NaN anywhere in a tensor makes its three figures NaN, an inf
// (and no NaN) makes them inf.  The fp64 sums carry both by themselves; the maximum does not (fmaxf drops a NaN), so grad_max_nan
// keeps one explicitly, and the row writes one canonical quiet NaN.  numel == 0: the row is [0, 0, 0, 0].
#ifndef HH_GRAD_STATS_MATH_H
#define HH_GRAD_STATS_MATH_H
#include "optim_math.h"

enum { GRAD_NORM_L2 = 0, GRAD_NORM_INF = 1 };  // HH_GRAD_NORM_* of include/hhrnet.h
enum { GRAD_WAVE = 64, GRAD_WAVES = OPTIM_THREADS / GRAD_WAVE };
static_assert(GRAD_WAVES == 4, "grad_block_combine adds four waves");

// One chunk's (one thread's, one wave's) statistics.  24 bytes; the workspace holds one per chunk.
struct GradPartial { double sumsq, abssum; float absmax; int nonfinite; };
// The head of the workspace: total_l2, total_inf, the coefficient of the last clip, unused.
struct GradTotals { float l2, inf, coef, reserved; };
// One fp32 row per tensor.
struct GradRow { float l2, absmax, absmean, nonfinite; };

HH_HD float grad_max_nan(float a, float b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

HH_HD GradPartial grad_partial_zero() { return GradPartial{0.0, 0.0, 0.0f, 0}; }

HH_HD void grad_accumulate(GradPartial &a, float v)
{
    const double d = (double)v;
    a.sumsq = a.sumsq + d * d;
    a.abssum = a.abssum + fabs(d);
    a.absmax = grad_max_nan(a.absmax, fabsf(v));
    a.nonfinite += optim_nonfinite(v) ? 1 : 0;
}

HH_HD GradPartial grad_combine(const GradPartial &a, const GradPartial &b)
{
    return GradPartial{a.sumsq + b.sumsq, a.abssum + b.abssum, grad_max_nan(a.absmax, b.absmax), a.nonfinite + b.nonfinite};
}

HH_HD GradPartial grad_block_combine(const GradPartial &w0, const GradPartial &w1, const GradPartial &w2, const GradPartial &w3)
{
    return grad_combine(grad_combine(w0, w1), grad_combine(w2, w3));
}

// The wave's tree on an array of GRAD_WAVE records (the host's form of it; the kernel runs the same pairs through lane shuffles).
inline void grad_wave_tree(GradPartial *lane)
{
    for (int off = GRAD_WAVE / 2; off > 0; off >>= 1)
        for (int i = 0; i < off; ++i) lane[i] = grad_combine(lane[i], lane[i + off]);
}

// Thread `tid`'s share of one chunk: optim_chunk_nonfinite's walk (the same addresses, the same stored bits: g * s where `scale`),
// with the statistics of the value that is stored.  *bad: the thread saw an inf / NaN (the gradient as read: a finite value times a
// finite scale that overflows is not flagged by optim_chunk_nonfinite either).
HH_HD GradPartial grad_chunk_stats(const OptimTensor &t, int chunk, bool scale, float s, int tid, bool *bad)
{
    const long long base = (long long)chunk * OPTIM_CHUNK;
    const long long left = t.numel - base;
    const int n = left < OPTIM_CHUNK ? (int)left : (int)OPTIM_CHUNK;
    const OptimPtr g = (OptimPtr)(t.grad + base);
    GradPartial a = grad_partial_zero();
    bool seen = false;
    int done = 0;
    if (optim_aligned16(g, nullptr, nullptr, nullptr)) {
        const int n4 = n >> 2;
        done = n4 << 2;
#pragma unroll
        for (int it = 0; it < OPTIM_ROUNDS; ++it) {
            const int i = it * OPTIM_THREADS + tid;
            if (i < n4) {
                OptimF4 v = ((OptimPtr4)g)[i];
                seen = seen || optim_nonfinite(v.x) || optim_nonfinite(v.y) || optim_nonfinite(v.z) || optim_nonfinite(v.w);
                if (scale) {
                    v.x = v.x * s; v.y = v.y * s; v.z = v.z * s; v.w = v.w * s;
                    ((OptimPtr4)g)[i] = v;
                }
                grad_accumulate(a, v.x);
                grad_accumulate(a, v.y);
                grad_accumulate(a, v.z);
                grad_accumulate(a, v.w);
            }
        }
    }
    for (int i = done + tid; i < n; i += OPTIM_THREADS) {
        float v = g[i];
        seen = seen || optim_nonfinite(v);
        if (scale) {
            v = v * s;
            g[i] = v;
        }
        grad_accumulate(a, v);
    }
    *bad = seen;
    return a;
}

// Thread `tid` of the per-tensor reduction: the tensor's chunk records tid, tid + OPTIM_THREADS, ... in that order.
HH_HD GradPartial grad_tensor_share(const GradPartial *parts, int nparts, int tid)
{
    GradPartial a = grad_partial_zero();
    for (int i = tid; i < nparts; i += OPTIM_THREADS) a = grad_combine(a, parts[i]);
    return a;
}

HH_HD float grad_quiet_nan()
{
    return __builtin_nanf("");
}

// The tensor's row from its combined record.
HH_HD GradRow grad_row(const GradPartial &a, long long numel)
{
    if (numel <= 0) return GradRow{0.0f, 0.0f, 0.0f, 0.0f};
    if (a.absmax != a.absmax) {
        const float q = grad_quiet_nan();
        return GradRow{q, q, q, (float)a.nonfinite};
    }
    return GradRow{(float)sqrt(a.sumsq), a.absmax, (float)(a.abssum / (double)numel), (float)a.nonfinite};
}

// total_l2 = (float)sqrt(sum over the tensors of their fp64 sums of squares), rounded once; total_inf = max of the rows' absmax.
HH_HD void grad_totals(const GradPartial &a, float *l2, float *inf)
{
    const bool nan = a.absmax != a.absmax;
    *l2 = nan ? grad_quiet_nan() : (float)sqrt(a.sumsq);
    *inf = nan ? grad_quiet_nan() : a.absmax;
}

// torch.nn.utils.clip_grad_norm_'s coefficient in its own fp32 arithmetic: max_norm / (total + 1e-6), clamped to at most 1
// (torch.clamp(max=1) keeps a NaN, and so does the comparison here).
HH_HD float grad_clip_coef(float max_norm, float total)
{
    const float c = max_norm / (total + 1e-6f);
    return c > 1.0f ? 1.0f : c;
}

// Thread `tid`'s share of one chunk of the scale pass: g = g * coef, over optim_chunk_nonfinite's walk.
HH_HD void grad_chunk_scale(const OptimTensor &t, int chunk, float coef, int tid)
{
    const long long base = (long long)chunk * OPTIM_CHUNK;
    const long long left = t.numel - base;
    const int n = left < OPTIM_CHUNK ? (int)left : (int)OPTIM_CHUNK;
    const OptimPtr g = (OptimPtr)(t.grad + base);
    int done = 0;
    if (optim_aligned16(g, nullptr, nullptr, nullptr)) {
        const int n4 = n >> 2;
        done = n4 << 2;
#pragma unroll
        for (int it = 0; it < OPTIM_ROUNDS; ++it) {
            const int i = it * OPTIM_THREADS + tid;
            if (i < n4) {
                OptimF4 v = ((OptimPtr4)g)[i];
                v.x = v.x * coef; v.y = v.y * coef; v.z = v.z * coef; v.w = v.w * coef;
                ((OptimPtr4)g)[i] = v;
            }
        }
    }
    for (int i = done + tid; i < n; i += OPTIM_THREADS) g[i] = g[i] * coef;
}

// The workspace (hh_grad_stats_bytes): [GradTotals][GradRow x ntensors][double sumsq x ntensors][GradPartial x nchunks]
// [int first_chunk x ntensors], every part 8-byte aligned when the workspace is 16-byte aligned.
struct GradWork { GradTotals *totals; GradRow *rows; double *tensor_sumsq; GradPartial *parts; int *first; };

HH_HD long long grad_work_bytes(long long ntensors, long long nchunks)
{
    return (long long)sizeof(GradTotals) + ntensors * (long long)(sizeof(GradRow) + sizeof(double)) + nchunks * (long long)sizeof(GradPartial) +
           (ntensors + (ntensors & 1)) * (long long)sizeof(int);
}

HH_HD GradWork grad_work(void *base, long long ntensors, long long nchunks)
{
    GradWork w;
    w.totals = (GradTotals *)base;
    w.rows = (GradRow *)(w.totals + 1);
    w.tensor_sumsq = (double *)(w.rows + ntensors);
    w.parts = (GradPartial *)(w.tensor_sumsq + ntensors);
    w.first = (int *)(w.parts + nchunks);
    return w;
}

#endif
