// The COCO keypoint scoring code (pytorch-human-pose_amd/csrc/coco_eval_math.h: the OKS of a pair, the matching walk, one image in plain
// loops, the validation) compiled for the HOST and run over generated images, so that its address arithmetic can be put under the
// sanitizers without a GPU:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I pytorch-human-pose_amd/csrc tools/coco_eval_host_check.cpp -o /tmp/coco_eval_host_check && /tmp/coco_eval_host_check
//
// For K in {1, 17, 64} one dataset holds an image for every D in {0, 1, 20, 32} x G in {0, 1, 63, 64, 65, 128}.  Every table and every
// output is a heap block of exactly its size, so a read or write one element past any of them is an AddressSanitizer report.  Checked
// besides: run over all images from two different fills (0xA5, 0x5A) the outputs come out equal, so every element was written; run
// for ONE image at a time exactly that image's rows of dt_match / dt_ignore (for every area and threshold) and of gt_ignore (for every
// area) change and no other element does, so, the images' rows being disjoint, every element is written by exactly one image and
// nothing outside the outputs is; the values are in range; the validation accepts the dataset and refuses one detection or one ground
// truth too many, offsets that decrease, and a non-positive var.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "coco_eval_math.h"

static unsigned long long rng_state = 88172645463325252ull;
static double rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (double)(rng_state >> 11) / 9007199254740992.0;
}

template <class T> static T *block(size_t n) { return (T *)malloc(n * sizeof(T)); }

static int run(int K)
{
    const int Ds[] = {0, 1, 20, 32}, Gs[] = {0, 1, 63, 64, 65, 128};
    const int I = 24, A = 3, T = 10;
    int32_t *dt_off = block<int32_t>(I + 1), *gt_off = block<int32_t>(I + 1);
    int64_t *oks_off = block<int64_t>(I + 1);
    dt_off[0] = gt_off[0] = 0; oks_off[0] = 0;
    for (int i = 0; i < I; ++i) {
        const int D = Ds[i / 6], G = Gs[i % 6];
        dt_off[i + 1] = dt_off[i] + D; gt_off[i + 1] = gt_off[i] + G; oks_off[i + 1] = oks_off[i] + (int64_t)D * G;
    }
    const int N = dt_off[I], M = gt_off[I];
    double *dt_xy = block<double>((size_t)N * K * 2), *dt_score = block<double>(N), *dt_area = block<double>(N);
    double *gt_xyv = block<double>((size_t)M * K * 3), *gt_area = block<double>(M), *gt_bbox = block<double>((size_t)M * 4);
    uint8_t *gt_flags = block<uint8_t>(M);
    double *vars = block<double>(K), *area_rng = block<double>(A * 2), *thr = block<double>(T);
    for (int k = 0; k < K; ++k) vars[k] = 1.0 + rnd();
    const double rng[6] = {0, 1e10, 1024, 9216, 9216, 1e10};
    memcpy(area_rng, rng, sizeof rng);
    for (int k = 0; k < T; ++k) thr[k] = 0.5 + 0.05 * k;
    for (int m = 0; m < M; ++m) {
        const int kind = (int)(rnd() * 8);  // 0: no labelled joint (doubled-box branch), 1: crowd
        for (int k = 0; k < K; ++k) {
            gt_xyv[((size_t)m * K + k) * 3] = 1000 + 40 * rnd();
            gt_xyv[((size_t)m * K + k) * 3 + 1] = 1000 + 40 * rnd();
            gt_xyv[((size_t)m * K + k) * 3 + 2] = kind == 0 ? 0 : (int)(rnd() * 3);
        }
        gt_area[m] = rnd() < 0.3 ? 1024.0 : 500 + 20000 * rnd();
        gt_bbox[4 * m] = 1000; gt_bbox[4 * m + 1] = 1000; gt_bbox[4 * m + 2] = 10 + 20 * rnd(); gt_bbox[4 * m + 3] = 10 + 20 * rnd();
        gt_flags[m] = (uint8_t)((kind <= 1 ? HH_COCO_GT_IGNORE : 0) | (kind == 1 ? HH_COCO_GT_CROWD : 0));
    }
    for (int n = 0; n < N; ++n) {
        for (int k = 0; k < K * 2; ++k) dt_xy[(size_t)n * K * 2 + k] = 1000 + 40 * rnd();
        dt_score[n] = rnd();
        dt_area[n] = 20000 * rnd();
    }
    CocoTables t;
    memset(&t, 0, sizeof t);
    t.dt_off = dt_off; t.gt_off = gt_off; t.oks_off = oks_off; t.dt_xy = dt_xy; t.dt_score = dt_score; t.dt_area = dt_area; t.gt_xyv = gt_xyv;
    t.gt_area = gt_area; t.gt_bbox = gt_bbox; t.gt_flags = gt_flags; t.vars = vars; t.area_rng = area_rng; t.thr = thr;
    t.I = I; t.N = N; t.M = M; t.K = K; t.A = A; t.T = T;

    int bad = 0;
    char msg[192];
    const char *why = coco_check(&t, msg, sizeof msg);
    if (why) { printf("  refused: %s\n", why); ++bad; }
    dt_off[1] += 33;  // (image 0 has no detection)
    if (!coco_check(&t, msg, sizeof msg)) { printf("  33 detections in one image were accepted\n"); ++bad; }
    dt_off[1] -= 33;
    gt_off[6] += 1;   // (image 5 has 128 ground truths)
    if (!coco_check(&t, msg, sizeof msg)) { printf("  129 ground truths in one image were accepted\n"); ++bad; }
    gt_off[6] -= 1;
    dt_off[8] -= 2;
    if (!coco_check(&t, msg, sizeof msg)) { printf("  decreasing offsets were accepted\n"); ++bad; }
    dt_off[8] += 2;
    const double keep = vars[K - 1];
    vars[K - 1] = 0;
    if (!coco_check(&t, msg, sizeof msg)) { printf("  a zero var was accepted\n"); ++bad; }
    vars[K - 1] = keep;

    const size_t n_match = (size_t)A * T * N, n_gt = (size_t)A * M, n_oks = (size_t)oks_off[I];
    double *scratch = block<double>(HH_COCO_MAX_DET * HH_COCO_MAX_GT);
    int32_t *m1 = block<int32_t>(n_match), *m2 = block<int32_t>(n_match);
    uint8_t *i1 = block<uint8_t>(n_match), *i2 = block<uint8_t>(n_match), *g1 = block<uint8_t>(n_gt), *g2 = block<uint8_t>(n_gt);
    double *o1 = block<double>(n_oks), *o2 = block<double>(n_oks);
    if (!bad) {
        memset(m1, 0xA5, n_match * 4); memset(i1, 0xA5, n_match); memset(g1, 0xA5, n_gt); memset(o1, 0xA5, n_oks * 8);
        memset(m2, 0x5A, n_match * 4); memset(i2, 0x5A, n_match); memset(g2, 0x5A, n_gt); memset(o2, 0x5A, n_oks * 8);
        for (int i = 0; i < I; ++i) coco_image_host(t, i, nullptr, o1, scratch, true, m1, i1, g1);
        for (int i = 0; i < I; ++i) coco_image_host(t, i, nullptr, o2, scratch, true, m2, i2, g2);
        if (memcmp(m1, m2, n_match * 4) || memcmp(i1, i2, n_match) || memcmp(g1, g2, n_gt) || memcmp(o1, o2, n_oks * 8)) { printf("  an element was not written\n"); ++bad; }
        for (size_t e = 0; e < n_match; ++e)
            if (m1[e] < 0 || m1[e] > M || i1[e] > 1) ++bad;
        for (size_t e = 0; e < n_gt; ++e)
            if (g1[e] > 1) ++bad;
        for (size_t e = 0; e < n_oks; ++e)
            if (!(o1[e] >= 0.0 && o1[e] <= 1.0)) ++bad;
        // matching alone on the stored matrix gives the same tables
        memset(m2, 0x5A, n_match * 4); memset(i2, 0x5A, n_match); memset(g2, 0x5A, n_gt);
        for (int i = 0; i < I; ++i) coco_image_host(t, i, o1, nullptr, scratch, true, m2, i2, g2);
        if (memcmp(m1, m2, n_match * 4) || memcmp(i1, i2, n_match) || memcmp(g1, g2, n_gt)) { printf("  matching on the stored matrix differs\n"); ++bad; }
        // one image at a time: exactly its rows change
        for (int i = 0; i < I && !bad; ++i) {
            memset(m2, 0x5A, n_match * 4); memset(i2, 0x5A, n_match); memset(g2, 0x5A, n_gt); memset(o2, 0x5A, n_oks * 8);
            coco_image_host(t, i, nullptr, o2, scratch, true, m2, i2, g2);
            for (int a = 0; a < A; ++a) {
                for (int k = 0; k < T; ++k)
                    for (int n = 0; n < N; ++n) {
                        const size_t e = ((size_t)a * T + k) * N + n;
                        const bool mine = n >= dt_off[i] && n < dt_off[i + 1];
                        if (mine ? (m2[e] != m1[e] || i2[e] != i1[e]) : (m2[e] != 0x5A5A5A5A || i2[e] != 0x5A)) ++bad;
                    }
                for (int m = 0; m < M; ++m) {
                    const bool mine = m >= gt_off[i] && m < gt_off[i + 1];
                    if (mine ? g2[(size_t)a * M + m] != g1[(size_t)a * M + m] : g2[(size_t)a * M + m] != 0x5A) ++bad;
                }
            }
            for (size_t e = 0; e < n_oks; ++e) {
                const bool mine = (int64_t)e >= oks_off[i] && (int64_t)e < oks_off[i + 1];
                uint64_t bits;
                memcpy(&bits, &o2[e], 8);
                if (mine ? memcmp(&o2[e], &o1[e], 8) != 0 : bits != 0x5A5A5A5A5A5A5A5Aull) ++bad;
            }
            if (bad) printf("  image %d wrote outside its rows or not all of them\n", i);
        }
    }
    size_t matched = 0;
    for (size_t e = 0; e < n_match; ++e) matched += m1[e] > 0;
    printf("K %2d: %d images, %d detections, %d ground truths, %zu OKS values, %zu of %zu matched%s\n", K, I, N, M, n_oks, matched, n_match, bad ? "  FAILED" : "");
    free(dt_off); free(gt_off); free(oks_off); free(dt_xy); free(dt_score); free(dt_area); free(gt_xyv); free(gt_area); free(gt_bbox); free(gt_flags);
    free(vars); free(area_rng); free(thr); free(scratch); free(m1); free(m2); free(i1); free(i2); free(g1); free(g2); free(o1); free(o2);
    return bad;
}

int main()
{
    int bad = 0;
    for (int K : {1, 17, 64}) bad += run(K);
    printf(bad ? "FAILED\n" : "coco_eval_host_check: clean\n");
    return bad ? 1 : 0;
}
