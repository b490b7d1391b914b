// The pose scoring code (pytorch-human-pose_amd/csrc/pose_score_math.h: the un-warp, the walk rank, D of a pair, the terms, one image
// in plain loops, the validation, the polygon area) compiled for the HOST and run over generated batches, so that its address
// arithmetic can be put under the sanitizers without a GPU:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I pytorch-human-pose_amd/csrc tools/pose_score_host_check.cpp -o /tmp/pose_score_host_check && /tmp/pose_score_host_check
//
// For K in {1, 3, 17, 64}, both metrics and both prediction forms, one batch holds an image for every P in {0, 1, 2, 30, 64} x T in
// {0, 1, 7, 8, 9, 128} (the maxima and the empty images included).  Every table and every output is a heap block of exactly its size,
// so a read or write one element past any of them is an AddressSanitizer report; the decode rows at and behind num[i] are NaN and must
// never count.  Checked besides: run over all images from two different fills (0xA5, 0x5A) the outputs come out equal, so every element
// was written; run for ONE image at a time exactly that image's elements change; the values are in range (match < P, terms in [0, 1] or
// -1, P = 0 with targets gives the NO_PRED bit and NaN); the validation accepts the batch and refuses, each by its own message: T = 129,
// P = 65, K = 65, max_people = 65, offsets that do not start at 0 or decrease, a target without a labelled joint, a non-finite target
// value, a zero / negative / infinite / NaN area, a zero var, a negative head size, a NaN alpha, a non-finite inverse matrix, an
// unknown form or metric, a null table; the polygon area on hand-made polygons, degenerate and out-of-range ones.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pose_score_math.h"

static unsigned long long rng_state = 88172645463325252ull;
static double rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (double)(rng_state >> 11) / 9007199254740992.0;
}

template <class T> static T *block(size_t n) { return (T *)malloc(n * sizeof(T) + (n ? 0 : 1)); }

static int expect_refused(const PoseTables &t, const char *needle, const char *what)
{
    char msg[192];
    const char *why = pose_check(t, msg, sizeof msg);
    if (!why || !strstr(why, needle)) { printf("  %s: %s\n", what, why ? why : "accepted"); return 1; }
    return 0;
}

static int run(int K, int form, int metric)
{
    const int Ps[] = {0, 1, 2, 30, 64}, Ts[] = {0, 1, 7, 8, 9, 128};
    const int B = 30, MP = 64, W = 4;
    int32_t *p_off = block<int32_t>(B + 1), *t_off = block<int32_t>(B + 1), *num = block<int32_t>(B), *flags = block<int32_t>(B);
    p_off[0] = t_off[0] = 0;
    for (int i = 0; i < B; ++i) {
        num[i] = Ps[i / 6];
        flags[i] = num[i] == 1 && (i & 1) ? HH_DECODE_FALLBACK : 0;
        p_off[i + 1] = p_off[i] + num[i];
        t_off[i + 1] = t_off[i] + Ts[i % 6];
    }
    const int NP = p_off[B], NT = t_off[B];
    float *joints = block<float>((size_t)B * MP * K * W), *scores = block<float>((size_t)B * MP);
    double *inv = block<double>((size_t)B * 6), *p_xy = block<double>((size_t)NP * K * 2), *p_score = block<double>(NP);
    double *t_xyv = block<double>((size_t)NT * K * 3), *t_area = block<double>(NT), *t_head = block<double>(NT);
    for (int i = 0; i < B; ++i) {
        const double m[6] = {1.7, 0, -3.25, 0, 1.7, 5.5}, id[6] = {1, 0, 0, 0, 1, 0};
        memcpy(inv + (size_t)i * 6, i % 2 ? m : id, sizeof m);
        for (int p = 0; p < MP; ++p) {
            scores[(size_t)i * MP + p] = p < num[i] ? (float)((int)(rnd() * 4) / 4.0) : NAN;  // (equal scores happen)
            for (int e = 0; e < K * W; ++e) joints[((size_t)i * MP + p) * K * W + e] = p < num[i] ? (float)(300 * rnd()) : NAN;
        }
    }
    for (int n = 0; n < NP; ++n) {
        p_score[n] = (int)(rnd() * 4) / 4.0;
        for (int e = 0; e < K * 2; ++e) p_xy[(size_t)n * K * 2 + e] = 300 * rnd();
    }
    for (int j = 0; j < NT; ++j) {
        for (int k = 0; k < K; ++k) {
            t_xyv[((size_t)j * K + k) * 3] = (int)(300 * rnd());
            t_xyv[((size_t)j * K + k) * 3 + 1] = (int)(300 * rnd());
            t_xyv[((size_t)j * K + k) * 3 + 2] = (int)(rnd() * 3);
        }
        t_xyv[((size_t)j * K + (int)(rnd() * K)) * 3 + 2] = 2;  // at least one labelled joint
        t_area[j] = rnd() < 0.2 ? 2.220446049250313e-16 : 500 + 20000 * rnd();
        t_head[j] = rnd() < 0.2 ? 0.0 : 10 + 40 * rnd();
    }
    PoseTables t;
    memset(&t, 0, sizeof t);
    if (form == HH_POSE_PRED_DECODE) t.joints = joints, t.scores = scores, t.num = num, t.flags = flags, t.inv_affine = inv;
    else t.p_off = p_off, t.p_xy = p_xy, t.p_score = p_score;
    t.t_off = t_off; t.t_xyv = t_xyv; t.t_area = t_area; t.t_head = t_head;
    for (int k = 0; k < HH_POSE_MAX_K; ++k) t.vars[k] = 0.002 + 0.04 * rnd();
    t.alpha = 0.5;
    t.image_stride = (int64_t)MP * K * W; t.person_stride = (int64_t)K * W; t.joint_stride = W; t.score_stride = MP;
    t.B = B; t.K = K; t.form = form; t.metric = metric; t.max_people = MP;

    int bad = 0;
    char msg[192];
    if (const char *why = pose_check(t, msg, sizeof msg)) { printf("  refused: %s\n", why); ++bad; }
    // the refusals, each undone again
    t_off[6] += 1;  // (image 5 has 128 targets; the later offsets stay ahead of it)
    bad += expect_refused(t, "over HH_POSE_MAX_T", "129 targets");
    t_off[6] -= 1;
    if (form == HH_POSE_PRED_F64) {
        p_off[B] += 1;  // (the last image has 64 predictions)
        bad += expect_refused(t, "over HH_POSE_MAX_P", "65 predictions");
        p_off[B] -= 1;
        p_off[0] = 1;
        bad += expect_refused(t, "p_off does not start at 0", "p_off[0] = 1");
        p_off[0] = 0;
        p_off[8] -= 3;
        bad += expect_refused(t, "p_off decreases", "decreasing p_off");
        p_off[8] += 3;
        t.p_off = nullptr;
        bad += expect_refused(t, "null pointer", "null p_off");
        t.p_off = p_off;
    } else {
        t.max_people = 65;
        bad += expect_refused(t, "max_people outside", "max_people 65");
        t.max_people = MP;
        inv[(size_t)3 * 6 + 2] = INFINITY;
        bad += expect_refused(t, "image 3: non-finite inverse matrix", "infinite matrix");
        inv[(size_t)3 * 6 + 2] = 0;
        t.person_stride = -1;
        bad += expect_refused(t, "negative stride", "negative stride");
        t.person_stride = (int64_t)K * W;
        t.inv_affine = nullptr;
        bad += expect_refused(t, "null pointer", "null inv_affine");
        t.inv_affine = inv;
    }
    t.K = 65;
    bad += expect_refused(t, "K outside", "K 65");
    t.K = 0;
    bad += expect_refused(t, "K outside", "K 0");
    t.K = K;
    t_off[0] = 1;
    bad += expect_refused(t, "t_off does not start at 0", "t_off[0] = 1");
    t_off[0] = 0;
    t_off[3] -= 8;  // (image 2 has 7 targets)
    bad += expect_refused(t, "image 2: t_off decreases", "decreasing t_off");
    t_off[3] += 8;
    {
        std::vector<double> keep(t_xyv, t_xyv + (size_t)K * 3);  // target 0 = image 1's only one
        for (int k = 0; k < K; ++k) t_xyv[(size_t)k * 3 + 2] = 0;
        bad += expect_refused(t, "image 1: target 0 has no labelled joint", "no labelled joint");
        memcpy(t_xyv, keep.data(), keep.size() * 8);
        t_xyv[1] = NAN;
        bad += expect_refused(t, "image 1: target 0 has a non-finite value", "NaN target");
        memcpy(t_xyv, keep.data(), keep.size() * 8);
    }
    for (double a : {0.0, -1.0, (double)INFINITY, (double)NAN}) {
        const double keep = t_area[1];
        t_area[1] = a;
        bad += expect_refused(t, "image 2: target 0: area must be finite and > 0", "bad area");
        t_area[1] = keep;
    }
    for (double h : {-1.0, (double)INFINITY, (double)NAN}) {
        const double keep = t_head[NT - 1];
        t_head[NT - 1] = h;
        bad += expect_refused(t, "head size must be finite and >= 0", "bad head");
        t_head[NT - 1] = keep;
    }
    for (double v : {0.0, -1.0, (double)INFINITY, (double)NAN}) {
        const double keep = t.vars[K - 1];
        t.vars[K - 1] = v;
        bad += expect_refused(t, "vars must be finite and > 0", "bad var");
        t.vars[K - 1] = keep;
    }
    t.alpha = NAN;
    bad += expect_refused(t, "alpha is not finite", "NaN alpha");
    t.alpha = 0.5;
    t.form = 2;
    bad += expect_refused(t, "form is neither", "form 2");
    t.form = form;
    t.metric = -1;
    bad += expect_refused(t, "metric is neither", "metric -1");
    t.metric = metric;
    t.t_area = nullptr;
    bad += expect_refused(t, "null pointer", "null t_area");
    t.t_area = t_area;
    t.B = -1;
    bad += expect_refused(t, "B outside", "B -1");
    t.B = B;
    if (pose_check(t, msg, sizeof msg)) { printf("  the tables were not restored\n"); ++bad; }

    double *pxy = block<double>((size_t)HH_POSE_MAX_P * K * 2), *score = block<double>(HH_POSE_MAX_P), *term = block<double>(K);
    double *v1 = block<double>(B), *v2 = block<double>(B), *o1 = block<double>(NT), *o2 = block<double>(NT);
    double *k1 = block<double>((size_t)NT * K), *k2 = block<double>((size_t)NT * K);
    int32_t *m1 = block<int32_t>(NT), *m2 = block<int32_t>(NT), *s1 = block<int32_t>(B), *s2 = block<int32_t>(B);
    auto fill = [&](int c, double *v, double *o, double *k, int32_t *m, int32_t *s) {
        memset(v, c, (size_t)B * 8); memset(o, c, (size_t)NT * 8); memset(k, c, (size_t)NT * K * 8); memset(m, c, (size_t)NT * 4); memset(s, c, (size_t)B * 4);
    };
    auto same = [&](const void *a, const void *b, size_t n) { return n == 0 || memcmp(a, b, n) == 0; };
    size_t hits = 0, nopred = 0;
    if (!bad) {
        fill(0xA5, v1, o1, k1, m1, s1);
        fill(0x5A, v2, o2, k2, m2, s2);
        for (int i = 0; i < B; ++i) pose_image_host(t, i, pxy, score, term, v1, o1, k1, m1, s1);
        for (int i = 0; i < B; ++i) pose_image_host(t, i, pxy, score, term, v2, o2, k2, m2, s2);
        if (!same(v1, v2, (size_t)B * 8) || !same(o1, o2, (size_t)NT * 8) || !same(k1, k2, (size_t)NT * K * 8) || !same(m1, m2, (size_t)NT * 4) ||
            !same(s1, s2, (size_t)B * 4)) { printf("  an element was not written\n"); ++bad; }
        for (int i = 0; i < B; ++i) {
            const int P = Ps[i / 6], T = Ts[i % 6];
            const int want = P == 0 && T > 0 ? HH_POSE_NO_PRED : 0;
            if (s1[i] != want) { printf("  image %d: status %d\n", i, s1[i]); ++bad; }
            nopred += want != 0;
            if (want ? v1[i] == v1[i] : T == 0 ? v1[i] != -1.0 : !(v1[i] >= -1.0 && v1[i] <= 1.0)) { printf("  image %d: value %g\n", i, v1[i]); ++bad; }
            for (int j = t_off[i]; j < t_off[i + 1]; ++j) {
                if (want) { bad += m1[j] != -1 || o1[j] == o1[j]; continue; }
                if (m1[j] < 0 || m1[j] >= P) ++bad;
                if (!(o1[j] == -1.0 || (o1[j] >= 0.0 && o1[j] <= 1.0))) ++bad;
                for (int k = 0; k < K; ++k) {
                    const double x = k1[(size_t)j * K + k];
                    if (!(x == -1.0 || (x >= 0.0 && x <= 1.0))) ++bad;
                    hits += x == 1.0;
                }
            }
        }
        for (int i = 0; i < B && !bad; ++i) {  // one image at a time: exactly its elements change
            fill(0x5A, v2, o2, k2, m2, s2);
            pose_image_host(t, i, pxy, score, term, v2, o2, k2, m2, s2);
            for (int b = 0; b < B; ++b) {
                uint64_t bits;
                memcpy(&bits, &v2[b], 8);
                if (b == i ? (memcmp(&v2[b], &v1[b], 8) || s2[b] != s1[b]) : (bits != 0x5A5A5A5A5A5A5A5Aull || s2[b] != 0x5A5A5A5A)) ++bad;
            }
            for (int j = 0; j < NT; ++j) {
                const bool mine = j >= t_off[i] && j < t_off[i + 1];
                uint64_t bits;
                memcpy(&bits, &o2[j], 8);
                if (mine ? (memcmp(&o2[j], &o1[j], 8) || m2[j] != m1[j]) : (bits != 0x5A5A5A5A5A5A5A5Aull || m2[j] != 0x5A5A5A5A)) ++bad;
                for (int k = 0; k < K; ++k) {
                    memcpy(&bits, &k2[(size_t)j * K + k], 8);
                    if (mine ? memcmp(&k2[(size_t)j * K + k], &k1[(size_t)j * K + k], 8) != 0 : bits != 0x5A5A5A5A5A5A5A5Aull) ++bad;
                }
            }
            if (bad) printf("  image %d wrote outside its elements or not all of them\n", i);
        }
    }
    printf("K %2d %s %s: %d images, %d predictions, %d targets, %zu terms of exactly 1, %zu images without a prediction%s\n", K,
           form == HH_POSE_PRED_DECODE ? "decode" : "f64   ", metric == HH_POSE_METRIC_OKS ? "oks " : "pckh", B, form == HH_POSE_PRED_DECODE ? p_off[B] : NP, NT,
           hits, nopred, bad ? "  FAILED" : "");
    free(p_off); free(t_off); free(num); free(flags); free(joints); free(scores); free(inv); free(p_xy); free(p_score); free(t_xyv); free(t_area); free(t_head);
    free(pxy); free(score); free(term); free(v1); free(v2); free(o1); free(o2); free(k1); free(k2); free(m1); free(m2); free(s1); free(s2);
    return bad;
}

static int polygons()
{
    int bad = 0;
    double a = -1;
    const double square[] = {0, 0, 10.9, 0, 10, 10.5, -0.9, 10}, tri[] = {0, 0, 3, 0, 0, 3}, tie[] = {0, 0, 2, 2, 2, 0, 0, 2};
    const double big[] = {-1073741824.0, -1073741824.0, 1073741824.0, -1073741824.0, 1073741824.0, 1073741824.0, -1073741824.0, 1073741824.0};
    const double far[] = {0, 0, 2147483648.0, 0, 1, 1}, nan[] = {0, 0, NAN, 0, 1, 1};
    bad += pose_polygon_area(square, 4, &a) != 0 || a != 100.0;
    bad += pose_polygon_area(tri, 3, &a) != 0 || a != 4.5;
    bad += pose_polygon_area(tie, 4, &a) != 0 || a != 0.0;
    bad += pose_polygon_area(big, 4, &a) != 0 || a != 4611686018427387904.0;
    bad += pose_polygon_area(tri, 2, &a) != 0 || a != 0.0;
    bad += pose_polygon_area(nullptr, 0, &a) != 0 || a != 0.0;
    double *one = block<double>(2);
    one[0] = 1, one[1] = 2;
    bad += pose_polygon_area(one, 1, &a) != 0 || a != 0.0;
    free(one);
    bad += pose_polygon_area(far, 3, &a) != 1;
    bad += pose_polygon_area(nan, 3, &a) != 1;
    bad += pose_polygon_area(nullptr, 3, &a) != 1;
    bad += pose_polygon_area(tri, -1, &a) != 1;
    bad += pose_polygon_area(tri, 3, nullptr) != 1;
    printf("polygon area: %s\n", bad ? "FAILED" : "ok");
    return bad;
}

int main()
{
    int bad = polygons();
    for (int K : {1, 3, 17, 64})
        for (int form : {HH_POSE_PRED_DECODE, HH_POSE_PRED_F64})
            for (int metric : {HH_POSE_METRIC_OKS, HH_POSE_METRIC_PCKH}) bad += run(K, form, metric);
    printf(bad ? "FAILED\n" : "pose_score_host_check: clean\n");
    return bad ? 1 : 0;
}
