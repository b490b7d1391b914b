// The weight EMA's code (pytorch-human-pose_amd/csrc/ema_math.h: coefficient, per-element update, the chunk walk of the stand-alone
// update and the swap; and optim_math.h's optimizer walk with the average as its fifth stream) compiled for the HOST and run over the
// lattice of tests/test_gpu_ema.py, so that the address arithmetic can be put under the sanitizers without a GPU:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I pytorch-human-pose_amd/csrc tools/ema_host_check.cpp -o /tmp/ema_host_check && /tmp/ema_host_check
//
// Every buffer is its own heap block that ends with the tensor's last element (one that starts one float into its block included), so
// a read or write one element past a tensor is an AddressSanitizer report.  The "grid" is two loops: chunk list x 256 thread ids.
// Checked against a plain per-element loop, bit for bit: the fused walk's p / state / gradient equal the walk without the fifth stream
// and its average equals the rule applied to that p; the stand-alone walk over the stepped p gives the same average; two swaps restore
// both sides and one exchanges them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ema_math.h"

static const long long SIZES[] = {1, 3, 4, 5, 255, 4095, 4096, 4097, 8195, 65539};
static const int NT = sizeof(SIZES) / sizeof(SIZES[0]);
enum { ALIGNED = 0, EMA_OFF = 1, PARAM_OFF = 2 };

static unsigned long long rng_state = 88172645463325252ull;
static float frand()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (float)((double)(rng_state >> 11) / 9007199254740992.0 * 2.0 - 1.0);
}

struct Buf {  // n floats whose first element sits `off` floats into a 16-byte aligned block that ends with the last element
    void *block = nullptr;
    float *ptr = nullptr;
    long long n;
    Buf(long long n_, int off) : n(n_)
    {
        const size_t bytes = (size_t)(n + off) * 4;
        if (posix_memalign(&block, 16, bytes ? bytes : 16)) abort();
        ptr = (float *)block + off;
        for (long long i = 0; i < n; ++i) ptr[i] = frand();
    }
    Buf(const Buf &o, int off) : Buf(o.n, off) { memcpy(ptr, o.ptr, (size_t)n * 4); }
    ~Buf() { free(block); }
};

static int differ(const float *a, const float *b, long long n) { return memcmp(a, b, (size_t)n * 4) != 0; }

template <int ALGO> static int run(int align, long long n_averaged, double decay, int warmup)
{
    const OptimGroup gr = {ALGO == HH_OPTIM_SGD ? 0.05 : 1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.9, 1, 0};
    const OptimCoefs c = optim_coefs(ALGO, gr.lr, gr.beta1, gr.beta2, gr.eps, gr.weight_decay, gr.momentum, gr.nesterov, 8.0);
    const EmaCoef ec = ema_coef(decay, warmup, n_averaged);
    int bad = 0;
    for (int k = 0; k < NT; ++k) {
        const long long n = SIZES[k];
        const int poff = align == PARAM_OFF, eoff = align == EMA_OFF;
        // two copies of the same operands: A walks with the fifth stream, B without and then the stand-alone walk
        Buf pA(n, poff), g0(n, 0), s0A(n, 0), s1A(n, 0), eA(n, eoff);
        for (long long i = 0; i < n; ++i) s1A.ptr[i] *= s1A.ptr[i];
        if (n > 2) { pA.ptr[0] = -0.0f; eA.ptr[1] = 1e-41f; }
        Buf gA(g0, 0), pB(pA, poff), gB(g0, 0), s0B(s0A, 0), s1B(s1A, 0), eB(eA, eoff), e0(eA, 0);
        const OptimTensor tA = {pA.ptr, gA.ptr, s0A.ptr, ALGO != HH_OPTIM_SGD ? s1A.ptr : nullptr, nullptr, n, 0, 0};
        const OptimTensor tB = {pB.ptr, gB.ptr, s0B.ptr, ALGO != HH_OPTIM_SGD ? s1B.ptr : nullptr, nullptr, n, 0, 0};
        const EmaRow rB = {pB.ptr, eB.ptr, n};
        const int nchunks = (int)((n + OPTIM_CHUNK - 1) / OPTIM_CHUNK);
        for (int ch = 0; ch < nchunks; ++ch)
            for (int tid = 0; tid < OPTIM_THREADS; ++tid) {
                optim_chunk_update<ALGO, EmaFifth>(tA, ch, c, true, 4.0f, tid, EmaFifth{eA.ptr, ec});
                optim_chunk_update<ALGO>(tB, ch, c, true, 4.0f, tid);
            }
        for (int ch = 0; ch < nchunks; ++ch)
            for (int tid = 0; tid < OPTIM_THREADS; ++tid) ema_chunk_walk<false>(rB, ch, ec, tid);
        bad += differ(pA.ptr, pB.ptr, n) + differ(gA.ptr, gB.ptr, n) + differ(s0A.ptr, s0B.ptr, n) + differ(s1A.ptr, s1B.ptr, n);
        bad += differ(eA.ptr, eB.ptr, n);
        for (long long i = 0; i < n; ++i) {  // the plain loop
            const float want = n_averaged == 0 ? pB.ptr[i] : e0.ptr[i] + (float)(1.0 - (warmup && (1.0 + n_averaged) / (10.0 + n_averaged) < decay
                                                                                                ? (1.0 + n_averaged) / (10.0 + n_averaged) : decay)) *
                                                                                 (pB.ptr[i] - e0.ptr[i]);
            bad += memcmp(&want, &eA.ptr[i], 4) != 0;
        }
        // a NULL fifth stream is the plain walk
        Buf pC(pB, poff), gC(gB, 0), s0C(s0B, 0), s1C(s1B, 0);
        const OptimTensor tC = {pC.ptr, gC.ptr, s0C.ptr, ALGO != HH_OPTIM_SGD ? s1C.ptr : nullptr, nullptr, n, 0, 0};
        for (int ch = 0; ch < nchunks; ++ch)
            for (int tid = 0; tid < OPTIM_THREADS; ++tid) {
                optim_chunk_update<ALGO, EmaFifth>(tC, ch, c, false, 1.0f, tid, EmaFifth{nullptr, ec});
                optim_chunk_update<ALGO>(tB, ch, c, false, 1.0f, tid);
            }
        bad += differ(pC.ptr, pB.ptr, n) + differ(s0C.ptr, s0B.ptr, n);
        // swap: once exchanges, twice restores
        Buf pS(pB, 0), eS(eB, 0);
        for (int round = 0; round < 2; ++round) {
            for (int ch = 0; ch < nchunks; ++ch)
                for (int tid = 0; tid < OPTIM_THREADS; ++tid) ema_chunk_walk<true>(rB, ch, ec, tid);
            bad += differ(pB.ptr, round ? pS.ptr : eS.ptr, n) + differ(eB.ptr, round ? eS.ptr : pS.ptr, n);
        }
    }
    return bad;
}

int main()
{
    int bad = 0, cases = 0;
    for (int align : {ALIGNED, EMA_OFF, PARAM_OFF})
        for (long long n : {0LL, 1LL, 7LL, 1000000LL})
            for (double decay : {0.9998, 0.5, 0.0, 1.0})
                for (int warmup : {0, 1}) {
                    const int b = run<HH_OPTIM_ADAM>(align, n, decay, warmup) + run<HH_OPTIM_ADAMW>(align, n, decay, warmup) + run<HH_OPTIM_SGD>(align, n, decay, warmup);
                    if (b) printf("align %d  n_averaged %lld  decay %g  warmup %d: %d mismatches\n", align, n, decay, warmup, b);
                    bad += b;
                    ++cases;
                }
    printf("%d cases x 3 algorithms x %d tensors: %s\n", cases, NT, bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
