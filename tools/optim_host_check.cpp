// The device optimizer step's code (pytorch-human-pose_amd/csrc/optim_math.h: coefficients, per-element update, one thread's walk over
// one chunk) compiled for the HOST and run over the table of tests/test_gpu_optim.py, so that the address arithmetic can be put under
// the sanitizers without a GPU:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I pytorch-human-pose_amd/csrc tools/optim_host_check.cpp -o /tmp/optim_host_check && /tmp/optim_host_check
//
// Every buffer is its own heap block of exactly the tensor's size (a gradient at an odd offset ends exactly at its block's end), so a
// read or write one element past a tensor is an AddressSanitizer report.  The "grid" is two loops: chunk list x 256 thread ids, as
// hh_optim_step builds and launches it.  Checked besides: every element was updated exactly once (it equals the scalar update of its
// original, bit for bit), a skipped chunk walk stores nothing, and the non-finite walk finds a planted inf / NaN.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "optim_math.h"

static const long long SIZES[] = {1, 7, 8, 17, 255, 256, 257, 4096, 4097, 65539, 589824};
static const int NT = sizeof(SIZES) / sizeof(SIZES[0]);

static unsigned long long rng_state = 88172645463325252ull;
static float frand()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (float)((double)(rng_state >> 11) / 9007199254740992.0 * 2.0 - 1.0);
}

struct Buf {  // n floats whose first element sits `off` floats into a 16-byte aligned block that ends with the last element
    void *block = nullptr;
    float *ptr = nullptr;
    Buf(long long n, int off)
    {
        const size_t bytes = (size_t)(n + off) * 4;
        if (posix_memalign(&block, 16, bytes ? bytes : 16)) abort();
        ptr = (float *)block + off;
    }
    ~Buf() { free(block); }
};

template <int ALGO> static int run(int step0, bool unscale)
{
    std::vector<Buf *> bufs;
    std::vector<OptimTensor> tensors;
    std::vector<std::vector<float>> orig;  // p, g, s0, s1 per tensor
    const OptimGroup groups[2] = {{ALGO == HH_OPTIM_SGD ? 0.05 : 1e-3, 0.9, 0.999, 1e-8, ALGO == HH_OPTIM_SGD ? 1e-4 : 0.0, 0.9, 1, 0},
                                  {ALGO == HH_OPTIM_SGD ? 0.01 : 3e-3, 0.9, 0.999, 1e-8, ALGO == HH_OPTIM_SGD ? 0.0 : 1e-2, 0.0, 0, 0}};
    const float scale = unscale ? 65536.0f : 1.0f;
    float step_counter[NT];
    for (int k = 0; k < NT; ++k) {
        const long long n = SIZES[k];
        const int goff = k % 3 == 0 ? 0 : (k % 3 == 1 ? 1 : 3);
        Buf *p = new Buf(n, 0), *g = new Buf(n, goff), *s0 = new Buf(n, 0), *s1 = new Buf(n, 0);
        bufs.insert(bufs.end(), {p, g, s0, s1});
        for (long long i = 0; i < n; ++i) {
            p->ptr[i] = frand();
            g->ptr[i] = frand() * 1e-2f * scale;
            s0->ptr[i] = step0 ? frand() * 1e-2f : 0.f;
            const float r = frand() * 1e-2f;
            s1->ptr[i] = step0 ? r * r : 0.f;
        }
        for (Buf *b : {p, g, s0, s1}) orig.emplace_back(b->ptr, b->ptr + n);
        step_counter[k] = (float)step0;
        const bool need_s0 = ALGO != HH_OPTIM_SGD || groups[k % 2].momentum != 0.0;
        tensors.push_back(OptimTensor{p->ptr, g->ptr, need_s0 ? s0->ptr : nullptr, ALGO != HH_OPTIM_SGD ? s1->ptr : nullptr,
                                      ALGO != HH_OPTIM_SGD ? &step_counter[k] : nullptr, n, k % 2, 0});
    }
    std::vector<OptimChunk> chunks;
    for (int k = 0; k < NT; ++k)
        for (int c = 0; c < (int)((SIZES[k] + OPTIM_CHUNK - 1) / OPTIM_CHUNK); ++c) chunks.push_back(OptimChunk{k, c});
    int bad = 0;
    // the non-finite walk on clean gradients, then the update
    for (const OptimChunk &ck : chunks)
        for (int tid = 0; tid < OPTIM_THREADS; ++tid) bad += optim_chunk_nonfinite(tensors[ck.tensor], ck.chunk, false, 1.0f, tid);
    if (bad) { printf("clean gradients flagged\n"); return 1; }
    for (const OptimChunk &ck : chunks) {
        const OptimTensor &t = tensors[ck.tensor];
        const OptimGroup &gr = groups[t.group];
        const OptimCoefs c = optim_coefs(ALGO, gr.lr, gr.beta1, gr.beta2, gr.eps, gr.weight_decay, gr.momentum, gr.nesterov,
                                         t.step ? (double)*t.step + 1.0 : 1.0);
        for (int tid = 0; tid < OPTIM_THREADS; ++tid) optim_chunk_update<ALGO>(t, ck.chunk, c, unscale, scale, tid);
    }
    // every element: the scalar update of its original
    for (int k = 0; k < NT; ++k) {
        const OptimTensor &t = tensors[k];
        const OptimGroup &gr = groups[t.group];
        const OptimCoefs c = optim_coefs(ALGO, gr.lr, gr.beta1, gr.beta2, gr.eps, gr.weight_decay, gr.momentum, gr.nesterov, step0 + 1.0);
        for (long long i = 0; i < SIZES[k]; ++i) {
            float p = orig[4 * k][i], g = orig[4 * k + 1][i] / scale, a = orig[4 * k + 2][i], b = orig[4 * k + 3][i];
            optim_update<ALGO>(p, g, a, b, c);
            bad += memcmp(&p, &t.param[i], 4) != 0;
            if (t.state0) bad += memcmp(&a, &t.state0[i], 4) != 0;
            if (t.state1) bad += memcmp(&b, &t.state1[i], 4) != 0;
            if (unscale) bad += memcmp(&g, &t.grad[i], 4) != 0;
        }
    }
    // a planted inf in the last element of the last tensor, a NaN in the first of the first
    tensors[NT - 1].grad[SIZES[NT - 1] - 1] = INFINITY;
    int hits = 0;
    for (const OptimChunk &ck : chunks)
        for (int tid = 0; tid < OPTIM_THREADS; ++tid) hits += optim_chunk_nonfinite(tensors[ck.tensor], ck.chunk, false, 1.0f, tid);
    bad += hits != 1;
    tensors[0].grad[0] = NAN;
    hits = 0;
    for (const OptimChunk &ck : chunks)
        for (int tid = 0; tid < OPTIM_THREADS; ++tid) hits += optim_chunk_nonfinite(tensors[ck.tensor], ck.chunk, true, 0.5f, tid);
    bad += hits != 2;
    for (Buf *b : bufs) delete b;
    printf("algo %d  step counter %d  %s: %zu chunks, %d mismatches\n", ALGO, step0, unscale ? "grad_scale 65536" : "no grad_scale", chunks.size(), bad);
    return bad;
}

int main()
{
    int bad = 0;
    for (int step0 : {0, 1, 999, 99999})
        for (bool unscale : {false, true}) bad += run<HH_OPTIM_ADAM>(step0, unscale) + run<HH_OPTIM_ADAMW>(step0, unscale);
    for (int step0 : {0, 1})
        for (bool unscale : {false, true}) bad += run<HH_OPTIM_SGD>(step0, unscale);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
