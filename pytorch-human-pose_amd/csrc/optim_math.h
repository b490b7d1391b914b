// The arithmetic of the device optimizer step (optim.hip), kept apart from the kernel so that the same text also compiles for the
// host (tools/optim_host_check.cpp runs it under the sanitizers): the table's structs, the per-workgroup coefficients, the per-element
// update, and one thread's walk over one chunk.  Compile with -ffp-contract=off: every operation below rounds on its own.
#ifndef HH_OPTIM_MATH_H
#define HH_OPTIM_MATH_H
#include <math.h>

#include "../../include/hhrnet.h"
#include "host_dev.h"

// The device table: hh_optim_tensor / hh_optim_group of include/hhrnet.h, and the chunk list hh_optim_step builds.
using OptimTensor = hh_optim_tensor;
using OptimGroup = hh_optim_group;
static_assert(sizeof(hh_optim_tensor) == 56 && sizeof(hh_optim_group) == 56, "ABI 3");
struct OptimChunk { int tensor, chunk; };  // elements [chunk * OPTIM_CHUNK, + OPTIM_CHUNK) of tensors[tensor]
enum { OPTIM_CHUNK = 4096, OPTIM_THREADS = 256, OPTIM_ROUNDS = OPTIM_CHUNK / (OPTIM_THREADS * 4) };
static_assert(OPTIM_ROUNDS * OPTIM_THREADS * 4 == OPTIM_CHUNK, "a chunk is a whole number of 4-element rounds of the workgroup");
struct alignas(16) OptimF4 { float x, y, z, w; };  // one 16-byte access
// The table's pointers are loaded from memory, so the compiler cannot know that they are device-global addresses and would emit
// flat_ accesses; the walkers say so (nothing on the host).
#if defined(__HIP_DEVICE_COMPILE__)
#define HH_GLOBAL __attribute__((address_space(1)))
#else
#define HH_GLOBAL
#endif
typedef HH_GLOBAL float *OptimPtr;
typedef HH_GLOBAL OptimF4 *OptimPtr4;

// What one workgroup needs of its tensor's hyper-parameter block, derived in fp64 and rounded to fp32 once.
struct OptimCoefs {
    float wd;         // Adam (L2) / SGD: g += wd * p; 0 = no such term
    float decay;      // AdamW: p *= 1 - lr * wd
    float om_b1;      // 1 - beta1
    float b2, om_b2;  // beta2, 1 - beta2
    float bc2_sqrt;   // sqrt(1 - beta2^step)
    float eps;
    float step_size;  // Adam: lr / (1 - beta1^step);  SGD: lr
    float momentum;
    int has_wd, has_momentum, nesterov;
};

// `step` is the number of THIS step: the tensor's counter before the launch, plus one.
HH_HD OptimCoefs optim_coefs(int algo, double lr, double beta1, double beta2, double eps, double weight_decay, double momentum, int nesterov,
                             double step)
{
    OptimCoefs c;
    c.has_wd = weight_decay != 0.0;
    c.wd = (float)weight_decay;
    c.decay = (float)(1.0 - lr * weight_decay);
    c.om_b1 = (float)(1.0 - beta1);
    c.b2 = (float)beta2;
    c.om_b2 = (float)(1.0 - beta2);
    c.eps = (float)eps;
    c.momentum = (float)momentum;
    c.has_momentum = momentum != 0.0;
    c.nesterov = nesterov;
    if (algo == HH_OPTIM_SGD) {
        c.bc2_sqrt = 1.0f;
        c.step_size = (float)lr;
    } else {
        const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);
        c.bc2_sqrt = (float)sqrt(bc2);
        c.step_size = (float)(lr / bc1);
    }
    return c;
}

// One element.  g is the unscaled gradient; s0 / s1 are exp_avg / exp_avg_sq (Adam, AdamW) or momentum_buffer / unused (SGD).
template <int ALGO> HH_HD void optim_update(float &p, float g, float &s0, float &s1, const OptimCoefs &c)
{
    if (ALGO == HH_OPTIM_SGD) {
        if (c.has_wd) g = g + c.wd * p;
        if (c.has_momentum) {
            const float buf = c.momentum * s0 + g;
            s0 = buf;
            g = c.nesterov ? g + c.momentum * buf : buf;
        }
        p = p - c.step_size * g;
    } else {
        if (c.has_wd) {
            if (ALGO == HH_OPTIM_ADAMW) p = p * c.decay;
            else g = g + c.wd * p;
        }
        const float m = s0 + c.om_b1 * (g - s0);
        const float v = c.b2 * s1 + c.om_b2 * (g * g);
        s0 = m;
        s1 = v;
        const float denom = sqrtf(v) / c.bc2_sqrt + c.eps;
        p = p - c.step_size * (m / denom);
    }
}

HH_HD bool optim_nonfinite(float x) { return !(fabsf(x) <= 3.402823466e+38f); }  // inf or NaN

HH_HD bool optim_aligned16(OptimPtr a, OptimPtr b, OptimPtr c, OptimPtr d)
{
    return (((unsigned long long)a | (unsigned long long)b | (unsigned long long)c | (unsigned long long)d) & 15ull) == 0;
}

// An optional fifth stream of the walk below: `ptr` is its address for this tensor (NULL: this tensor has none), apply() its new value
// from its old one and the stepped parameter.  OptimNoFifth is none at all, the walk of optim_step_kernel; ema_math.h has the other.
struct OptimNoFifth {
    enum { ON = 0 };
    float *ptr;
    HH_HD float apply(float old, float) const { return old; }
};

// Thread `tid` of OPTIM_THREADS's share of one chunk: the whole memory walk of optim_step_kernel.  16-byte accesses where the chunk's
// four addresses allow them (a chunk starts 16 KiB into its tensor, so the tensors' own addresses decide), scalar ones for any other
// chunk and for the last numel % 4 elements.  unscale: g / scale is used and written back.  A fifth stream joins the alignment test
// (it alone misaligned: the scalar path for all five) and is read and written next to p.
template <int ALGO, class Fifth = OptimNoFifth>
HH_HD void optim_chunk_update(const OptimTensor &t, int chunk, const OptimCoefs &c, bool unscale, float scale, int tid, const Fifth fifth = Fifth{nullptr})
{
    const long long base = (long long)chunk * OPTIM_CHUNK;
    const long long left = t.numel - base;
    const int n = left < OPTIM_CHUNK ? (int)left : (int)OPTIM_CHUNK;
    // SGD: s1 is unused, and s0 only with momentum (hh_optim_step checks that it is there then)
    const bool use_s0 = ALGO != HH_OPTIM_SGD || c.has_momentum, use_s1 = ALGO != HH_OPTIM_SGD;
    const OptimPtr p = (OptimPtr)(t.param + base), g = (OptimPtr)(t.grad + base), s0 = use_s0 ? (OptimPtr)(t.state0 + base) : nullptr,
                   s1 = use_s1 ? (OptimPtr)(t.state1 + base) : nullptr;
    const bool use_e = Fifth::ON && fifth.ptr != nullptr;
    const OptimPtr e = use_e ? (OptimPtr)(fifth.ptr + base) : nullptr;
    int done = 0;  // elements the 16-byte path covers
    if (optim_aligned16(p, g, s0, s1) && (!Fifth::ON || ((unsigned long long)e & 15ull) == 0)) {
        const int n4 = n >> 2;
        done = n4 << 2;
#pragma unroll
        for (int it = 0; it < OPTIM_ROUNDS; ++it) {
            const int i = it * OPTIM_THREADS + tid;
            if (i < n4) {
                OptimF4 pv = ((OptimPtr4)p)[i], gv = ((OptimPtr4)g)[i];
                OptimF4 av = use_s0 ? ((OptimPtr4)s0)[i] : OptimF4{0.f, 0.f, 0.f, 0.f};
                OptimF4 bv = use_s1 ? ((OptimPtr4)s1)[i] : OptimF4{0.f, 0.f, 0.f, 0.f};
                OptimF4 ev = use_e ? ((OptimPtr4)e)[i] : OptimF4{0.f, 0.f, 0.f, 0.f};
                if (unscale) {
                    gv.x = gv.x / scale; gv.y = gv.y / scale; gv.z = gv.z / scale; gv.w = gv.w / scale;
                    ((OptimPtr4)g)[i] = gv;
                }
                optim_update<ALGO>(pv.x, gv.x, av.x, bv.x, c);
                optim_update<ALGO>(pv.y, gv.y, av.y, bv.y, c);
                optim_update<ALGO>(pv.z, gv.z, av.z, bv.z, c);
                optim_update<ALGO>(pv.w, gv.w, av.w, bv.w, c);
                ((OptimPtr4)p)[i] = pv;
                if (use_s0) ((OptimPtr4)s0)[i] = av;
                if (use_s1) ((OptimPtr4)s1)[i] = bv;
                if (use_e) {
                    ev.x = fifth.apply(ev.x, pv.x); ev.y = fifth.apply(ev.y, pv.y); ev.z = fifth.apply(ev.z, pv.z); ev.w = fifth.apply(ev.w, pv.w);
                    ((OptimPtr4)e)[i] = ev;
                }
            }
        }
    }
    for (int i = done + tid; i < n; i += OPTIM_THREADS) {
        float pv = p[i], gv = g[i], av = use_s0 ? s0[i] : 0.f, bv = use_s1 ? s1[i] : 0.f;
        if (unscale) {
            gv = gv / scale;
            g[i] = gv;
        }
        optim_update<ALGO>(pv, gv, av, bv, c);
        p[i] = pv;
        if (use_s0) s0[i] = av;
        if (use_s1) s1[i] = bv;
        if (use_e) e[i] = fifth.apply(e[i], pv);
    }
}

// The same walk over the gradient alone (grads_nonfinite_kernel): -> true if this thread saw an inf / NaN; scale: g *= s in place.
HH_HD bool optim_chunk_nonfinite(const OptimTensor &t, int chunk, bool scale, float s, int tid)
{
    const long long base = (long long)chunk * OPTIM_CHUNK;
    const long long left = t.numel - base;
    const int n = left < OPTIM_CHUNK ? (int)left : (int)OPTIM_CHUNK;
    const OptimPtr g = (OptimPtr)(t.grad + base);
    bool bad = false;
    int done = 0;
    if (optim_aligned16(g, nullptr, nullptr, nullptr)) {
        const int n4 = n >> 2;
        done = n4 << 2;
#pragma unroll
        for (int it = 0; it < OPTIM_ROUNDS; ++it) {
            const int i = it * OPTIM_THREADS + tid;
            if (i < n4) {
                OptimF4 v = ((OptimPtr4)g)[i];
                bad = bad || optim_nonfinite(v.x) || optim_nonfinite(v.y) || optim_nonfinite(v.z) || optim_nonfinite(v.w);
                if (scale) {
                    v.x = v.x * s; v.y = v.y * s; v.z = v.z * s; v.w = v.w * s;
                    ((OptimPtr4)g)[i] = v;
                }
            }
        }
    }
    for (int i = done + tid; i < n; i += OPTIM_THREADS) {
        const float v = g[i];
        bad = bad || optim_nonfinite(v);
        if (scale) g[i] = v * s;
    }
    return bad;
}

#endif
