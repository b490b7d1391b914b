// The classifier scoring code (pytorch-human-pose_amd/csrc/cls_score_math.h: the accumulator's layout, the order, one row in plain loops
// with the kernel's summation order, the fold, the validation) compiled for the HOST and run over generated batches, so that its address
// arithmetic can be put under the sanitizers without a GPU:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I pytorch-human-pose_amd/csrc tools/cls_score_host_check.cpp -o /tmp/cls_score_host_check && /tmp/cls_score_host_check
//
// Shapes (B, N, k): (1,1,1), (1,5,5), (3,3,5), (7,64,5), (5,65,5), (33,1000,5), (4,1001,8), (3,1024,5), (3,1025,5), (2,65536,8), and
// (1024,10,5), the largest batch; each with and without the confusion matrix, with targets (two of them out of range where B >= 3, one
// row NaN, one +inf where B >= 5), without targets, without an accumulator, and with every per-row output NULL.  Every buffer is a heap
// block of exactly its size, so a read or write one element past any of them is an AddressSanitizer report.  Checked besides: run from
// two different fills (0xA5, 0x5A) the per-row outputs come out equal, so every element was written; indices lie in [-1, N) and are
// distinct, probabilities in [0, 1] and descending, entries from min(k, N) on are -1 / 0; the counters add up to B; the scratch is zero
// after every call; one call and calls of 1, 2 and the rest leave identical accumulator bytes; an accumulator reset for another N gets
// the layout flag and nothing else; the validation refuses, each by its own message, B = 1025, N = 0, N = 65537, k = 0, k = 9, null
// logits, misaligned pointers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cls_score_math.h"

static unsigned long long rng_state = 88172645463325252ull;
static double rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (double)(rng_state >> 11) / 9007199254740992.0;
}

template <class T> static T *block(size_t n) { return (T *)malloc(n * sizeof(T) + (n ? 0 : 1)); }

struct Out {
    int32_t *idx, *rank;
    float *prob, *loss;
    Out(int B, int k, int fill) : idx(block<int32_t>((size_t)B * k)), rank(block<int32_t>(B)), prob(block<float>((size_t)B * k)), loss(block<float>(B))
    {
        memset(idx, fill, (size_t)B * k * 4), memset(prob, fill, (size_t)B * k * 4), memset(rank, fill, (size_t)B * 4), memset(loss, fill, (size_t)B * 4);
    }
    ~Out() { free(idx), free(rank), free(prob), free(loss); }
};

static int check_shape(int B, int N, int k, int wc)
{
    int bad = 0;
    float *z = block<float>((size_t)B * N);
    int64_t *t = block<int64_t>(B);
    for (size_t i = 0; i < (size_t)B * N; ++i) z[i] = (float)(rnd() * 12 - 6);
    for (int b = 0; b < B; ++b) t[b] = (int64_t)(rnd() * N) % N;
    for (int j = 0; j + 1 < N && j < 3; ++j) z[j + 1] = z[0];  // ties in row 0
    int want_bad = 0, want_nf = 0;
    if (B >= 3) t[1] = -1, t[2] = N, want_bad = 2;
    if (B >= 5) z[(size_t)3 * N + N - 1] = NAN, z[(size_t)4 * N] = INFINITY, want_nf = 2;
    const int keff = k < N ? k : N;
    const size_t bytes = cls_acc_bytes(N, wc);
    unsigned char *acc = block<unsigned char>(bytes), *acc2 = block<unsigned char>(bytes);
    memset(acc, 0xEE, bytes), memset(acc2, 0x11, bytes);
    cls_reset_host(acc, N, wc), cls_reset_host(acc2, N, wc);
    Out a(B, k, 0xA5), c(B, k, 0x5A);
    if (cls_check(z, t, B, N, k, acc, a.idx, a.prob, a.rank, a.loss)) { printf("  the validation refuses a good call\n"); return 1; }
    cls_batch_host(z, (const long long *)t, B, N, k, acc, a.idx, a.prob, a.rank, a.loss);
    // the same rows as calls of 1, 2 and the rest, from the other fill
    for (int b0 = 0, step = 1; b0 < B; b0 += step, step = step == 1 ? 2 : B) {
        const int n = step < B - b0 ? step : B - b0;
        cls_batch_host(z + (size_t)b0 * N, (const long long *)t + b0, n, N, k, acc2, c.idx + (size_t)b0 * k, c.prob + (size_t)b0 * k, c.rank + b0, c.loss + b0);
    }
    if (memcmp(acc, acc2, bytes)) printf("  accumulator bytes depend on the split\n"), ++bad;
    if (memcmp(a.idx, c.idx, (size_t)B * k * 4) || memcmp(a.prob, c.prob, (size_t)B * k * 4) || memcmp(a.rank, c.rank, (size_t)B * 4) ||
        memcmp(a.loss, c.loss, (size_t)B * 4))
        printf("  per-row outputs depend on the fill or the split\n"), ++bad;
    for (size_t i = cls_off_loss(N, wc); i < bytes; ++i)
        if (acc[i]) { printf("  scratch byte %zu not zero after the call\n", i); ++bad; break; }
    const hh_cls_eval_acc *h = (const hh_cls_eval_acc *)acc;
    if (h->rows + h->bad_target + h->nonfinite != B || h->bad_target != want_bad || h->nonfinite != want_nf || h->top1 > h->topk || h->topk > h->rows)
        printf("  counters: rows %lld bad %lld nonfinite %lld top1 %lld topk %lld of B = %d\n", (long long)h->rows, (long long)h->bad_target,
               (long long)h->nonfinite, (long long)h->top1, (long long)h->topk, B), ++bad;
    if (h->flags != (unsigned)((want_bad ? HH_CLS_BAD_TARGET : 0) | (want_nf ? HH_CLS_NONFINITE : 0))) printf("  flags %u\n", h->flags), ++bad;
    const int32_t *pc = (const int32_t *)(acc + cls_off_per_class());
    long long n0 = 0, n1 = 0, nk = 0, nc = 0;
    for (int j = 0; j < N; ++j) n0 += pc[j], n1 += pc[N + j], nk += pc[2 * (size_t)N + j];
    if (wc) {
        const int32_t *cf = (const int32_t *)(acc + cls_off_conf(N));
        for (size_t i = 0; i < (size_t)N * N; ++i) nc += cf[i];
    }
    if (n0 != h->rows || n1 != h->top1 || nk != h->topk || (wc && nc != h->rows)) printf("  the tables do not add up to the counters\n"), ++bad;
    for (int b = 0; b < B; ++b) {
        const bool nf = B >= 5 && (b == 3 || b == 4);
        for (int r = 0; r < k; ++r) {
            const int j = a.idx[(size_t)b * k + r];
            const float p = a.prob[(size_t)b * k + r];
            const bool empty = nf || r >= keff;
            if (empty ? (j != -1 || p != 0.f) : (j < 0 || j >= N || !(p >= 0.f && p <= 1.f))) { printf("  row %d entry %d: index %d prob %g\n", b, r, j, p); ++bad; }
            for (int q = 0; q < r && !empty; ++q)
                if (a.idx[(size_t)b * k + q] == j || a.prob[(size_t)b * k + q] < p) { printf("  row %d: entries %d and %d out of order\n", b, q, r); ++bad; }
        }
        const bool scored = !nf && t[b] >= 0 && t[b] < N;
        if (scored ? (a.rank[b] < 0 || a.rank[b] >= N || !(a.loss[b] >= 0.f)) : (a.rank[b] != -1 || a.loss[b] != 0.f)) { printf("  row %d: rank %d loss %g\n", b, a.rank[b], a.loss[b]); ++bad; }
    }
    if (N >= 4 && (a.idx[0] > 3 && z[0] >= z[a.idx[0]])) printf("  row 0: a tie went to the higher index\n"), ++bad;
    // without targets, without an accumulator, with no outputs: the accumulator does not move
    memcpy(acc2, acc, bytes);
    Out d(B, k, 0xA5);
    cls_batch_host(z, nullptr, B, N, k, acc, d.idx, d.prob, d.rank, d.loss);
    cls_batch_host(z, (const long long *)t, B, N, k, nullptr, d.idx, d.prob, d.rank, d.loss);
    if (memcmp(acc, acc2, bytes)) printf("  a call without targets changed the accumulator\n"), ++bad;
    if (memcmp(a.idx, d.idx, (size_t)B * k * 4) || memcmp(a.rank, d.rank, (size_t)B * 4)) printf("  outputs without an accumulator differ\n"), ++bad;
    cls_batch_host(z, (const long long *)t, B, N, k, acc, nullptr, nullptr, nullptr, nullptr);
    if (((const hh_cls_eval_acc *)acc)->rows != 2 * ((const hh_cls_eval_acc *)acc2)->rows)
        printf("  a second call did not double the rows\n"), ++bad;
    // an accumulator reset for another N: the layout flag and nothing else
    cls_reset_host(acc2, N, wc);
    ((hh_cls_eval_acc *)acc2)->N = N + 1;
    memcpy(acc, acc2, bytes);
    cls_batch_host(z, (const long long *)t, B, N, k, acc2, nullptr, nullptr, nullptr, nullptr);
    if (((hh_cls_eval_acc *)acc2)->flags != HH_CLS_LAYOUT) printf("  no layout flag\n"), ++bad;
    ((hh_cls_eval_acc *)acc2)->flags = 0;
    if (memcmp(acc, acc2, bytes)) printf("  a call on a foreign accumulator wrote more than the flag\n"), ++bad;
    free(z), free(t), free(acc), free(acc2);
    return bad;
}

static int expect_refused(const char *why, const char *needle, const char *what)
{
    if (!why || !strstr(why, needle)) { printf("  %s: %s\n", what, why ? why : "accepted"); return 1; }
    return 0;
}

int main()
{
    const int shapes[][3] = {{1, 1, 1}, {1, 5, 5}, {3, 3, 5}, {7, 64, 5}, {5, 65, 5}, {33, 1000, 5}, {4, 1001, 8}, {3, 1024, 5}, {3, 1025, 5},
                             {2, 65536, 8}, {1024, 10, 5}};
    int bad = 0;
    for (const auto &s : shapes)
        for (int wc = 0; wc < 2; ++wc) {
            if (wc && s[1] > 2048) continue;  // (a 65536 x 65536 confusion matrix is 16 GB)
            const int n = check_shape(s[0], s[1], s[2], wc);
            printf("B %d N %d k %d confusion %d: %s\n", s[0], s[1], s[2], wc, n ? "FAILED" : "ok");
            bad += n;
        }
    float z[8] = {};
    bad += expect_refused(cls_check(z, nullptr, 1025, 4, 1, nullptr, nullptr, nullptr, nullptr, nullptr), "B must", "B = 1025");
    bad += expect_refused(cls_check(z, nullptr, 2, 0, 1, nullptr, nullptr, nullptr, nullptr, nullptr), "N must", "N = 0");
    bad += expect_refused(cls_check(z, nullptr, 2, 65537, 1, nullptr, nullptr, nullptr, nullptr, nullptr), "N must", "N = 65537");
    bad += expect_refused(cls_check(z, nullptr, 2, 4, 0, nullptr, nullptr, nullptr, nullptr, nullptr), "k must", "k = 0");
    bad += expect_refused(cls_check(z, nullptr, 2, 4, 9, nullptr, nullptr, nullptr, nullptr, nullptr), "k must", "k = 9");
    bad += expect_refused(cls_check(nullptr, nullptr, 2, 4, 1, nullptr, nullptr, nullptr, nullptr, nullptr), "null logits", "null logits");
    bad += expect_refused(cls_check(z, (const int64_t *)((char *)z + 4), 2, 4, 1, nullptr, nullptr, nullptr, nullptr, nullptr), "8-byte", "misaligned targets");
    bad += expect_refused(cls_check(z, nullptr, 2, 4, 1, nullptr, nullptr, (const float *)((char *)z + 2), nullptr, nullptr), "4-byte", "misaligned output");
    bad += expect_refused(cls_check_shape(4, 2), "with_confusion", "with_confusion = 2");
    printf(bad ? "FAILED (%d)\n" : "all ok\n", bad);
    return bad ? 1 : 0;
}
