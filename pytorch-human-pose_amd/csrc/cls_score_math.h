// Scoring of classifier logits (hh_cls_score_batch of include/hhrnet.h, whose text is the specification), kept apart from the kernel so
// that the same text also compiles for the host (hh_cls_score_host, tools/cls_score_host_check.cpp): the accumulator's layout, the
// order, the non-finite test, the per-row status word, the validation, one row in plain loops with the kernel's summation order, the
// fold.  Compile with -ffp-contract=off: every operation rounds on its own, so everything but expf() and log() is bit-identical on both
// sides.
#ifndef HH_CLS_SCORE_MATH_H
#define HH_CLS_SCORE_MATH_H
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/hhrnet.h"
#include "host_dev.h"

// The accumulator's header (include/hhrnet.h states it by offset: it is not one of the ABI's descriptor structs).
struct hh_cls_eval_acc {
    int64_t rows, top1, topk, bad_target, nonfinite;
    double loss_sum;
    uint32_t flags;
    int32_t N, with_confusion, reserved;
};
static_assert(offsetof(hh_cls_eval_acc, loss_sum) == 40 && offsetof(hh_cls_eval_acc, flags) == 48 && offsetof(hh_cls_eval_acc, N) == 52 &&
                  offsetof(hh_cls_eval_acc, with_confusion) == 56,
              "the offsets written in include/hhrnet.h");

// One wave owns one row: lane l holds the elements j = l, l + 64, ...; CLS_REG of them fit in its registers (N <= HH_CLS_ROW_REGS).
enum { CLS_WAVES = 4, CLS_THREADS = 64 * CLS_WAVES, CLS_REG = HH_CLS_ROW_REGS / 64 };
static_assert(HH_CLS_TOPK_MAX <= 64, "lane r keeps the r-th winner");
static_assert(sizeof(hh_cls_eval_acc) == 64, "the tables behind the header start 8-byte aligned");

// the status word a row leaves in the call scratch for the fold
enum { CLS_ST_SCORED = 1, CLS_ST_TOP1 = 2, CLS_ST_TOPK = 4, CLS_ST_BAD_TARGET = 8, CLS_ST_NONFINITE = 16 };

// The blocks behind the header, as byte offsets from the accumulator's start (N and with_confusion checked by the caller).
HH_HD size_t cls_off_per_class() { return sizeof(hh_cls_eval_acc); }
HH_HD size_t cls_off_conf(int N) { return cls_off_per_class() + (size_t)3 * N * sizeof(int32_t); }
HH_HD size_t cls_off_loss(int N, int with_confusion)
{
    const size_t end = cls_off_conf(N) + (with_confusion ? (size_t)N * N * sizeof(int32_t) : 0);
    return (end + 7) & ~(size_t)7;
}
HH_HD size_t cls_off_status(int N, int with_confusion) { return cls_off_loss(N, with_confusion) + (size_t)HH_CLS_MAX_B * sizeof(double); }
HH_HD size_t cls_acc_bytes(int N, int with_confusion) { return cls_off_status(N, with_confusion) + (size_t)HH_CLS_MAX_B * sizeof(int32_t); }

// the accumulator's blocks as pointers; ok = the header describes the layout the call assumes
struct ClsAcc {
    hh_cls_eval_acc *hdr;
    int32_t *per_class, *conf, *status;
    double *loss;
    bool ok;
};
HH_HD ClsAcc cls_acc_view(void *acc, int N)
{
    ClsAcc a;
    unsigned char *p = static_cast<unsigned char *>(acc);
    a.hdr = static_cast<hh_cls_eval_acc *>(acc);
    const int wc = a.hdr->with_confusion;
    a.ok = a.hdr->N == N && (wc == 0 || wc == 1);
    a.per_class = reinterpret_cast<int32_t *>(p + cls_off_per_class());
    a.conf = a.ok && wc ? reinterpret_cast<int32_t *>(p + cls_off_conf(N)) : nullptr;
    a.loss = reinterpret_cast<double *>(p + cls_off_loss(N, a.ok ? wc : 0));      // (not touched unless ok)
    a.status = reinterpret_cast<int32_t *>(p + cls_off_status(N, a.ok ? wc : 0));
    return a;
}

// j before j' in the order of the rule
HH_HD bool cls_before(float za, int ja, float zb, int jb) { return za > zb || (za == zb && ja < jb); }
// NaN or +inf
HH_HD bool cls_bad_value(float v) { return !(v < INFINITY); }
HH_HD float cls_neg_inf() { return -INFINITY; }

inline const char *cls_check_shape(int N, int with_confusion)
{
    if (N < 1 || N > HH_CLS_MAX_N) return "N must lie in 1..HH_CLS_MAX_N (65536)";
    if (with_confusion != 0 && with_confusion != 1) return "with_confusion must be 0 or 1";
    return nullptr;
}
inline const char *cls_check(const float *logits, const int64_t *targets, int B, int N, int k, const void *acc, const int32_t *topk_idx,
                             const float *topk_prob, const int32_t *rank, const float *row_loss)
{
    if (B < 0 || B > HH_CLS_MAX_B) return "B must lie in 0..HH_CLS_MAX_B (1024)";
    if (const char *why = cls_check_shape(N, 0)) return why;
    if (k < 1 || k > HH_CLS_TOPK_MAX) return "k must lie in 1..HH_CLS_TOPK_MAX (8)";
    if (!logits && B > 0) return "null logits";
    if ((uintptr_t)targets % 8 || (uintptr_t)acc % 8) return "targets and acc must be 8-byte aligned";
    if ((uintptr_t)logits % 4 || (uintptr_t)topk_idx % 4 || (uintptr_t)topk_prob % 4 || (uintptr_t)rank % 4 || (uintptr_t)row_loss % 4)
        return "logits and the per-row outputs must be 4-byte aligned";
    return nullptr;
}

inline void cls_reset_host(void *acc, int N, int with_confusion)
{
    memset(acc, 0, cls_acc_bytes(N, with_confusion));
    hh_cls_eval_acc *h = static_cast<hh_cls_eval_acc *>(acc);
    h->N = N, h->with_confusion = with_confusion;
}

// The fold of one call on the host: the header grows by the B status words and losses of the scratch, losses in ascending row order.
inline void cls_fold_host(const ClsAcc &a, int B)
{
    if (!a.ok) { a.hdr->flags |= HH_CLS_LAYOUT; return; }
    double s = a.hdr->loss_sum;
    for (int b = 0; b < B; ++b) {
        const int st = a.status[b];
        if (st & CLS_ST_SCORED) s += a.loss[b];
        a.hdr->rows += (st & CLS_ST_SCORED) != 0, a.hdr->top1 += (st & CLS_ST_TOP1) != 0, a.hdr->topk += (st & CLS_ST_TOPK) != 0;
        a.hdr->bad_target += (st & CLS_ST_BAD_TARGET) != 0, a.hdr->nonfinite += (st & CLS_ST_NONFINITE) != 0;
        if (st & CLS_ST_BAD_TARGET) a.hdr->flags |= HH_CLS_BAD_TARGET;
        if (st & CLS_ST_NONFINITE) a.hdr->flags |= HH_CLS_NONFINITE;
        a.status[b] = 0, a.loss[b] = 0.0;
    }
    a.hdr->loss_sum = s;
}

// One row on the host, in the kernel's order: 64 lanes' strided partial sums, then the shuffle tree.  a: the accumulator's view or null.
inline void cls_row_host(const float *row, bool has_t, long long t, int b, int N, int k, const ClsAcc *a, int32_t *topk_idx, float *topk_prob,
                         int32_t *rank, float *row_loss)
{
    const int keff = k < N ? k : N;
    float m = cls_neg_inf();
    bool bad = false;
    for (int j = 0; j < N; ++j) {
        bad |= cls_bad_value(row[j]);
        m = fmaxf(m, row[j]);
    }
    bad |= !(m > cls_neg_inf());
    int idx[HH_CLS_TOPK_MAX];
    float prob[HH_CLS_TOPK_MAX];
    for (int r = 0; r < k; ++r) idx[r] = -1, prob[r] = 0.f;
    int st = 0, rk = -1;
    double loss = 0.0;
    if (bad) {
        st = CLS_ST_NONFINITE;
    } else {
        double part[64];
        for (int l = 0; l < 64; ++l) {
            double s = 0.0;
            for (int j = l; j < N; j += 64) s += (double)expf(row[j] - m);
            part[l] = s;
        }
        for (int o = 32; o > 0; o >>= 1) {
            double next[64];
            for (int l = 0; l < 64; ++l) next[l] = part[l] + part[l ^ o];
            memcpy(part, next, sizeof part);
        }
        const double sum = part[0];
        float pz = 0.f;
        int pj = -1;
        for (int r = 0; r < keff; ++r) {
            float bz = 0.f;
            int bj = -1;
            for (int j = 0; j < N; ++j) {
                const bool cand = pj < 0 || cls_before(pz, pj, row[j], j);
                if (cand && (bj < 0 || cls_before(row[j], j, bz, bj))) bz = row[j], bj = j;
            }
            idx[r] = bj, prob[r] = (float)((double)expf(bz - m) / sum);
            pz = bz, pj = bj;
        }
        if (has_t && (t < 0 || t >= N)) {
            st = CLS_ST_BAD_TARGET;
        } else if (has_t) {
            const float zt = row[t];
            rk = 0;
            for (int j = 0; j < N; ++j) rk += cls_before(row[j], j, zt, (int)t);
            loss = ((double)m + log(sum)) - (double)zt;
            st = CLS_ST_SCORED | (rk < 1 ? CLS_ST_TOP1 : 0) | (rk < keff ? CLS_ST_TOPK : 0);
        }
    }
    for (int r = 0; r < k; ++r) {
        if (topk_idx) topk_idx[(size_t)b * k + r] = idx[r];
        if (topk_prob) topk_prob[(size_t)b * k + r] = prob[r];
    }
    if (rank) rank[b] = rk;
    if (row_loss) row_loss[b] = (float)loss;
    if (a && a->ok) {
        a->status[b] = st, a->loss[b] = loss;
        if (st & CLS_ST_SCORED) {
            a->per_class[t] += 1;
            if (st & CLS_ST_TOP1) a->per_class[(size_t)N + t] += 1;
            if (st & CLS_ST_TOPK) a->per_class[(size_t)2 * N + t] += 1;
            if (a->conf) a->conf[(size_t)t * N + idx[0]] += 1;
        }
    }
}

// One call on the host: the rows in order, then the fold.  Without targets or without an accumulator only the per-row outputs are written.
inline void cls_batch_host(const float *logits, const long long *targets, int B, int N, int k, void *acc, int32_t *topk_idx, float *topk_prob,
                           int32_t *rank, float *row_loss)
{
    ClsAcc a = {};
    const bool use = acc && targets;
    if (use) a = cls_acc_view(acc, N);
    for (int b = 0; b < B; ++b)
        cls_row_host(logits + (size_t)b * N, targets != nullptr, targets ? targets[b] : -1, b, N, k, use ? &a : nullptr, topk_idx, topk_prob, rank,
                     row_loss);
    if (use && B > 0) cls_fold_host(a, B);
}
#endif
