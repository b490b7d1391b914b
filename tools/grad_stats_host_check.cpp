// The gradient statistics' and the clip's code (pytorch-human-pose_amd/csrc/grad_stats_math.h: one thread's walk over one chunk, the
// fixed-order combination, the per-tensor row, the totals, the coefficient, the scale walk) compiled for the HOST and run over the
// lattice of tests/test_gpu_grad_clip.py, so that the address arithmetic can be put under the sanitizers without a GPU:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I pytorch-human-pose_amd/csrc tools/grad_stats_host_check.cpp -o /tmp/grad_stats_host_check && /tmp/grad_stats_host_check
//
// Every buffer -- each gradient, and each part of the workspace -- is its own heap block of exactly its size (a gradient at an odd
// offset ends exactly at its block's end), so a read or write one element past it is an AddressSanitizer report.  The "grid" is loops:
// chunk list x 256 thread ids, then the wave tree and the block's combination as the kernels run them.  Checked besides: every row and
// both totals against a long double reference (printed in units of the budgets of tests/grad_clip_budget.py), the fused unscale pass
// (stored bits, flag, statistics of the stored value), the exact-arithmetic case, a planted inf / NaN, the scale walk (g0 * coef bit
// for bit, nothing stored at coef >= 1) and the workspace's parts lying inside grad_work_bytes.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "grad_stats_math.h"

static const long long SIZES[] = {1, 7, 8, 17, 255, 256, 257, 4096, 4097, 65539, 589824, 4096 * 257 + 3};
static const int NT = sizeof(SIZES) / sizeof(SIZES[0]);
static const float SCALES[] = {1e-6f, 1e-3f, 1.0f, 30.0f};
static const double U = 1.0 / 16777216.0;  // 2^-24

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

struct Table {
    std::vector<Buf *> bufs;
    std::vector<OptimTensor> tensors;
    std::vector<OptimChunk> chunks;
    // the workspace's parts, each a block of exactly its size
    std::vector<GradPartial> parts;
    std::vector<int> first;
    std::vector<GradRow> rows;
    std::vector<double> tensor_sumsq;
    GradTotals totals{};
    Table()
    {
        for (int k = 0; k < NT; ++k) {
            const int goff = k % 3 == 0 ? 0 : (k % 3 == 1 ? 1 : 3);
            bufs.push_back(new Buf(SIZES[k], goff));
            tensors.push_back(OptimTensor{nullptr, bufs[k]->ptr, nullptr, nullptr, nullptr, SIZES[k], 0, 0});
            for (int c = 0; c < (int)((SIZES[k] + OPTIM_CHUNK - 1) / OPTIM_CHUNK); ++c) chunks.push_back(OptimChunk{k, c});
        }
        parts.resize(chunks.size());
        first.assign(NT, -1);
        rows.resize(NT);
        tensor_sumsq.resize(NT);
    }
    ~Table() { for (Buf *b : bufs) delete b; }
    float *g(int k) { return tensors[k].grad; }
};

static GradPartial block_reduce(GradPartial *thread)  // OPTIM_THREADS records -> the block's, as grad_block_reduce of grad_stats.hip
{
    for (int w = 0; w < GRAD_WAVES; ++w) grad_wave_tree(thread + w * GRAD_WAVE);
    return grad_block_combine(thread[0], thread[GRAD_WAVE], thread[2 * GRAD_WAVE], thread[3 * GRAD_WAVE]);
}

// hh_grad_stats as the three launches run it; -> found_inf
static float run_stats(Table &T, bool fused, float inv_scale)
{
    float found = 0.0f;
    std::vector<GradPartial> thread(OPTIM_THREADS);
    for (size_t b = 0; b < T.chunks.size(); ++b) {
        const OptimChunk ck = T.chunks[b];
        for (int tid = 0; tid < OPTIM_THREADS; ++tid) {
            bool bad;
            thread[tid] = grad_chunk_stats(T.tensors[ck.tensor], ck.chunk, fused && inv_scale != 1.0f, inv_scale, tid, &bad);
            if (bad && fused) found = 1.0f;
        }
        T.parts[b] = block_reduce(thread.data());
        if (ck.chunk == 0) T.first[ck.tensor] = (int)b;
    }
    for (int k = 0; k < NT; ++k) {
        const int nparts = (int)((SIZES[k] + OPTIM_CHUNK - 1) / OPTIM_CHUNK);
        for (int tid = 0; tid < OPTIM_THREADS; ++tid) thread[tid] = grad_tensor_share(T.parts.data() + T.first[k], nparts, tid);
        const GradPartial all = block_reduce(thread.data());
        T.rows[k] = grad_row(all, SIZES[k]);
        T.tensor_sumsq[k] = all.sumsq;
    }
    for (int tid = 0; tid < OPTIM_THREADS; ++tid) {
        GradPartial a = grad_partial_zero();
        for (int i = tid; i < NT; i += OPTIM_THREADS) a = grad_combine(a, GradPartial{T.tensor_sumsq[i], 0.0, T.rows[i].absmax, 0});
        thread[tid] = a;
    }
    grad_totals(block_reduce(thread.data()), &T.totals.l2, &T.totals.inf);
    return found;
}

static void run_clip(Table &T, float max_norm, int norm_type, float found)
{
    const float coef = grad_clip_coef(max_norm, norm_type == GRAD_NORM_INF ? T.totals.inf : T.totals.l2);
    T.totals.coef = coef;
    if (found != 0.0f || coef >= 1.0f) return;
    for (const OptimChunk &ck : T.chunks)
        for (int tid = 0; tid < OPTIM_THREADS; ++tid) grad_chunk_scale(T.tensors[ck.tensor], ck.chunk, coef, tid);
}

static bool same(float a, float b) { return memcmp(&a, &b, 4) == 0; }

static void fill_random(Table &T, float mul)
{
    for (int k = 0; k < NT; ++k)
        for (long long i = 0; i < SIZES[k]; ++i) T.g(k)[i] = frand() * SCALES[k % 4] * mul;
}

static int lattice()
{
    Table T;
    fill_random(T, 1.0f);
    std::vector<std::vector<float>> g0;
    for (int k = 0; k < NT; ++k) g0.emplace_back(T.g(k), T.g(k) + SIZES[k]);
    int bad = run_stats(T, false, 1.0f) != 0.0f;
    long double total = 0;
    float total_inf = 0;
    double worst_l2 = 0, worst_mean = 0;
    for (int k = 0; k < NT; ++k) {
        long double ss = 0, as = 0;
        float mx = 0;
        for (float v : g0[k]) { ss += (long double)v * v; as += fabsl((long double)v); mx = fmaxf(mx, fabsf(v)); }
        total += ss;
        total_inf = fmaxf(total_inf, mx);
        const double l2 = (double)sqrtl(ss), mean = (double)(as / SIZES[k]), nu = 2.0 * (double)SIZES[k] * 0x1p-53;
        worst_l2 = fmax(worst_l2, fabs((double)T.rows[k].l2 - l2) / ((U + nu) * l2 + 0x1p-150));
        worst_mean = fmax(worst_mean, fabs((double)T.rows[k].absmean - mean) / ((U + nu) * mean + 0x1p-150));
        bad += !same(T.rows[k].absmax, mx) || T.rows[k].nonfinite != 0.0f;
        bad += memcmp(g0[k].data(), T.g(k), (size_t)SIZES[k] * 4) != 0;  // the statistics pass alone stores nothing
    }
    const double tl2 = (double)sqrtl(total);
    const double worst_total = fabs((double)T.totals.l2 - tl2) / ((U + 2.0 * 1.8e6 * 0x1p-53) * tl2 + 0x1p-150);
    printf("lattice: worst error / budget  l2 %.3f  absmean %.3f  total_l2 %.3f  (total %.9g, inf %.9g)\n", worst_l2, worst_mean, worst_total,
           (double)T.totals.l2, (double)T.totals.inf);
    bad += !(worst_l2 < 1 && worst_mean < 1 && worst_total < 1) || !same(T.totals.inf, total_inf);
    // clip far above the norm: nothing stored; then below it, both norm types: g0 * coef bit for bit
    run_clip(T, 1e6f, GRAD_NORM_L2, 0.0f);
    bad += !same(T.totals.coef, 1.0f);
    for (int k = 0; k < NT; ++k) bad += memcmp(g0[k].data(), T.g(k), (size_t)SIZES[k] * 4) != 0;
    for (int norm_type : {GRAD_NORM_L2, GRAD_NORM_INF}) {
        for (int k = 0; k < NT; ++k) memcpy(T.g(k), g0[k].data(), (size_t)SIZES[k] * 4);
        const float maxn = 0.25f * (norm_type == GRAD_NORM_INF ? T.totals.inf : T.totals.l2);
        run_clip(T, maxn, norm_type, 0.0f);
        const float coef = T.totals.coef;
        bad += !(coef < 1.0f);
        for (int k = 0; k < NT; ++k)
            for (long long i = 0; i < SIZES[k]; ++i) bad += !same(T.g(k)[i], g0[k][i] * coef);
        // with the flag set the scale walk stores nothing
        for (int k = 0; k < NT; ++k) memcpy(T.g(k), g0[k].data(), (size_t)SIZES[k] * 4);
        run_clip(T, maxn, norm_type, 1.0f);
        for (int k = 0; k < NT; ++k) bad += memcmp(g0[k].data(), T.g(k), (size_t)SIZES[k] * 4) != 0;
    }
    printf("lattice: %zu chunks, %d mismatches\n", T.chunks.size(), bad);
    return bad;
}

static int fused()
{
    // gradients x 65536, unscaled in the statistics pass: the stored bits and the flag are optim_chunk_nonfinite's, the statistics
    // those of a separate pass over the stored values
    Table A, B;
    const unsigned long long seed = rng_state;
    fill_random(A, 65536.0f);
    rng_state = seed;
    fill_random(B, 65536.0f);
    int bad = run_stats(A, true, 1.0f / 65536.0f) != 0.0f;
    for (const OptimChunk &ck : B.chunks)
        for (int tid = 0; tid < OPTIM_THREADS; ++tid) bad += optim_chunk_nonfinite(B.tensors[ck.tensor], ck.chunk, true, 1.0f / 65536.0f, tid);
    for (int k = 0; k < NT; ++k) bad += memcmp(A.g(k), B.g(k), (size_t)SIZES[k] * 4) != 0;
    run_stats(B, false, 1.0f);
    bad += memcmp(A.rows.data(), B.rows.data(), NT * sizeof(GradRow)) != 0 || !same(A.totals.l2, B.totals.l2) || !same(A.totals.inf, B.totals.inf);
    // a planted inf in the last element of the last chunk, a NaN in the first element
    A.g(NT - 1)[SIZES[NT - 1] - 1] = INFINITY;
    A.g(0)[0] = NAN;
    A.g(3)[2] = -INFINITY;
    A.g(3)[5] = INFINITY;
    bad += run_stats(A, true, 0.5f) != 1.0f;
    const GradRow rn = A.rows[0], ri = A.rows[NT - 1], r2 = A.rows[3];
    bad += !(std::isnan(rn.l2) && std::isnan(rn.absmax) && std::isnan(rn.absmean) && rn.nonfinite == 1.0f);
    bad += !(std::isinf(ri.l2) && std::isinf(ri.absmax) && std::isinf(ri.absmean) && ri.nonfinite == 1.0f);
    bad += !(std::isinf(r2.l2) && std::isinf(r2.absmax) && std::isinf(r2.absmean) && r2.nonfinite == 2.0f);
    bad += !(std::isnan(A.totals.l2) && std::isnan(A.totals.inf));
    printf("fused unscale at 65536, planted inf / NaN: %d mismatches\n", bad);
    return bad;
}

static int exact()
{
    // 0 / +-1 with 4^j non-zeros per tensor, one of them the last element: every summation order is exact
    Table T;
    long long total = 0;
    for (int k = 0; k < NT; ++k) {
        long long nz = 1;
        while (nz * 4 <= SIZES[k]) nz *= 4;
        memset(T.g(k), 0, (size_t)SIZES[k] * 4);
        const long long stride = nz > 1 ? (SIZES[k] - 1) / (nz - 1) : 1;
        for (long long j = 0; j < nz - 1; ++j) T.g(k)[j * stride] = j % 2 ? -1.0f : 1.0f;
        T.g(k)[SIZES[k] - 1] = 1.0f;
        total += nz;
    }
    run_stats(T, false, 1.0f);
    int bad = 0;
    for (int k = 0; k < NT; ++k) bad += T.tensor_sumsq[k] != floor(T.tensor_sumsq[k]) || !same(T.rows[k].absmax, 1.0f);
    bad += total != 1385049 || !same(T.totals.l2, (float)sqrt((double)total)) || !same(T.totals.l2, 1176.881103515625f);
    run_clip(T, 3.0f, GRAD_NORM_L2, 0.0f);
    const float coef = 3.0f / (1176.881103515625f + 1e-6f);
    bad += !same(T.totals.coef, coef);
    for (int k = 0; k < NT; ++k)
        for (long long i = 0; i < SIZES[k]; ++i) bad += T.g(k)[i] != 0.0f && !same(fabsf(T.g(k)[i]), coef);
    printf("exact case: sum of squares %lld, total %.12f, %d mismatches\n", total, (double)T.totals.l2, bad);
    return bad;
}

static int workspace()
{
    // grad_work's parts lie inside grad_work_bytes, in order, without overlap, for odd and even tensor counts
    int bad = 0;
    for (long long nt : {0LL, 1LL, 2LL, 11LL, 900LL})
        for (long long nc : {0LL, 1LL, 7001LL}) {
            char *base = (char *)0x1000;
            const GradWork w = grad_work(base, nt, nc);
            const long long bytes = grad_work_bytes(nt, nc);
            bad += (char *)w.rows != base + 16 || (char *)w.tensor_sumsq != (char *)(w.rows + nt) || (char *)w.parts != (char *)(w.tensor_sumsq + nt) ||
                   (char *)w.first != (char *)(w.parts + nc) || (char *)(w.first + nt) > base + bytes || bytes % 8 != 0;
        }
    printf("workspace layout: %d mismatches\n", bad);
    return bad;
}

int main()
{
    const int bad = lattice() + fused() + exact() + workspace();
    printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
