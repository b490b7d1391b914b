// The arithmetic of the weight EMA (ema.hip), host/device like optim_math.h so that the same text compiles for the host
// (tools/ema_host_check.cpp runs it under the sanitizers): the row struct, the per-launch coefficient, the per-element update, and one
// thread's walk over one chunk for the stand-alone update and the swap.  The fused form is optim_math.h's walk with EmaFifth as its
// fifth stream.  Compile with -ffp-contract=off: every operation below rounds on its own.
//
// RULE, for one element, n = the update counter before this launch:
//   n == 0:    ema = value, the bits copied
//   otherwise: d = warmup ? min(decay, (1 + n) / (10 + n)) : decay       in fp64, decay in [0, 1]
//              w = (float)(1.0 - d)                                      rounded once (a decay rounded to fp32 first is off by
//                                                                        about 1e-4 of w at decay 0.9998)
//              ema = ema + w * (value - ema)                             in fp32, this one form for every w
#ifndef HH_EMA_MATH_H
#define HH_EMA_MATH_H
#include "optim_math.h"

using EmaRow = hh_ema_row;
static_assert(sizeof(hh_ema_row) == 24, "ABI 3");

struct EmaCoef {
    float w;   // 1 - d
    int copy;  // n == 0
};

HH_HD EmaCoef ema_coef(double decay, int warmup, long long n)
{
    EmaCoef c;
    c.copy = n == 0;
    double d = decay;
    if (warmup) {
        const double ramp = (1.0 + (double)n) / (10.0 + (double)n);
        if (ramp < d) d = ramp;
    }
    c.w = (float)(1.0 - d);
    return c;
}

HH_HD float ema_update(float ema, float value, const EmaCoef &c) { return c.copy ? value : ema + c.w * (value - ema); }

// The fifth stream of optim_chunk_update: the average of the parameter that walk has just stepped.
struct EmaFifth {
    enum { ON = 1 };
    float *ptr;
    EmaCoef c;
    HH_HD float apply(float old, float p) const { return ema_update(old, p, c); }
};

typedef float EmaV4 __attribute__((vector_size(16)));  // one 16-byte access moved as a value (the swap computes nothing)

// the elements of `chunk` in a row of `numel`
HH_HD int ema_chunk_len(long long numel, int chunk)
{
    const long long left = numel - (long long)chunk * OPTIM_CHUNK;
    return left < OPTIM_CHUNK ? (int)left : (int)OPTIM_CHUNK;
}

// Thread `tid` of OPTIM_THREADS's share of one chunk of a (value, ema) row: 16-byte accesses where both addresses allow them, scalar
// ones for any other chunk and for the last numel % 4 elements.  SWAP: exchange the two instead of updating the average.
template <bool SWAP> HH_HD void ema_chunk_walk(const EmaRow &r, int chunk, const EmaCoef &c, int tid)
{
    const long long base = (long long)chunk * OPTIM_CHUNK;
    const int n = ema_chunk_len(r.numel, chunk);
    const OptimPtr v = (OptimPtr)(r.value + base), e = (OptimPtr)(r.ema + base);
    int done = 0;
    if (optim_aligned16(v, e, nullptr, nullptr)) {
        const int n4 = n >> 2;
        done = n4 << 2;
#pragma unroll
        for (int it = 0; it < OPTIM_ROUNDS; ++it) {
            const int i = it * OPTIM_THREADS + tid;
            if (i < n4) {
                if (SWAP) {
                    const EmaV4 a = ((HH_GLOBAL EmaV4 *)v)[i], b = ((HH_GLOBAL EmaV4 *)e)[i];
                    ((HH_GLOBAL EmaV4 *)v)[i] = b;
                    ((HH_GLOBAL EmaV4 *)e)[i] = a;
                } else {
                    const OptimF4 vv = ((OptimPtr4)v)[i];
                    OptimF4 ev = ((OptimPtr4)e)[i];
                    ev.x = ema_update(ev.x, vv.x, c); ev.y = ema_update(ev.y, vv.y, c); ev.z = ema_update(ev.z, vv.z, c); ev.w = ema_update(ev.w, vv.w, c);
                    ((OptimPtr4)e)[i] = ev;
                }
            }
        }
    }
    for (int i = done + tid; i < n; i += OPTIM_THREADS) {
        const float vv = v[i], ev = e[i];
        if (SWAP) {
            v[i] = ev;
            e[i] = vv;
        } else {
            e[i] = ema_update(ev, vv, c);
        }
    }
}

#endif
