// The crowd mask's host code (pytorch-human-pose_amd/csrc/crowd_mask_math.h: polygon walk, cancel step, upper-bound predicate, column
// bits, one mask walked tile by tile, the validation) compiled for the HOST and run over the stated fixtures, random polygons and
// random toggle lists aimed at the tile boundaries, so that the address arithmetic can be put under the sanitizers without a GPU:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I pytorch-human-pose_amd/csrc tools/crowd_mask_host_check.cpp -o /tmp/crowd_mask_host_check && /tmp/crowd_mask_host_check
//
// The mask is a heap block of exactly h * w bytes and the toggles a block of exactly their count, so a read or write one element past
// either is an AddressSanitizer report.  Checked besides: the fixtures' pixel counts, the tile walk against the per-pixel predicate
// (every byte, union over the segments), the toggle lists strictly increasing and <= h * w, the capacity bound never below the count,
// and that the validation accepts what is drawn here and refuses a broken list.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "crowd_mask_math.h"

static unsigned long long rng_state = 88172645463325252ull;
static unsigned rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (unsigned)(rng_state >> 33);
}
static double uniform(double lo, double hi) { return lo + (hi - lo) * (rnd() / 2147483648.0); }

static int fail(const char *what, int h, int w)
{
    printf("FAILED: %s (h = %d, w = %d)\n", what, h, w);
    return 1;
}

static std::vector<uint32_t> polygon(const std::vector<double> &xy, int h, int w)
{
    std::vector<uint32_t> t;
    const int k = (int)xy.size() / 2;
    if (crowd_polygon_check(xy.data(), k, h, w)) { printf("FAILED: a polygon of this program was refused\n"); exit(1); }
    crowd_polygon_walk(xy.data(), k, h, w, t);
    crowd_cancel(t);
    if ((long long)t.size() > crowd_polygon_bound(xy.data(), k, w)) { printf("FAILED: more toggles than the capacity bound\n"); exit(1); }
    return t;
}

// One mask from `lists` through the tile walk, in exactly sized heap blocks, against the per-pixel predicate.  -> covered pixels, or -1.
static long long run(int h, int w, const std::vector<std::vector<uint32_t>> &lists)
{
    size_t words = 0;
    for (const auto &t : lists) words += t.size();
    uint32_t *toggles = (uint32_t *)malloc(words ? words * 4 : 1);
    CrowdSegDesc *segs = (CrowdSegDesc *)malloc(lists.empty() ? 1 : sizeof(CrowdSegDesc) * lists.size());
    unsigned char *mask = (unsigned char *)malloc((size_t)h * w);
    memset(mask, 0x5b, (size_t)h * w);
    size_t at = 0;
    for (size_t s = 0; s < lists.size(); ++s) {
        const auto &t = lists[s];
        for (size_t i = 0; i < t.size(); ++i) {
            if (t[i] > (uint32_t)h * w || (i && t[i] <= t[i - 1])) return fail("toggle list not strictly increasing in 0 .. h*w", h, w), -1;
            toggles[at + i] = t[i];
        }
        int first = 0, last = 0;
        if (!t.empty()) {
            first = (int)(t[0] / h) < w - 1 ? (int)(t[0] / h) : w - 1;
            last = (t.size() & 1) ? w - 1 : (int)((t.back() - 1) / h);
            if (last < first) last = first;
        }
        segs[s] = CrowdSegDesc{(long long)(at * 4), (int32_t)t.size(), first, last, 0};
        at += t.size();
    }
    const CrowdMaskDesc d{0, h, w, 0, (int32_t)lists.size()};
    const unsigned char *base = reinterpret_cast<const unsigned char *>(toggles);
    if (const char *why = crowd_check_mask(d, segs, (long long)lists.size(), base)) return fail(why, h, w), -1;
    crowd_mask_host(mask, d, segs, base);
    long long covered = 0;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            bool c = false;
            size_t off = 0;
            for (const auto &t : lists) {
                c = c || crowd_covered(toggles + off, (uint32_t)t.size(), (uint32_t)x * h + y);
                off += t.size();
            }
            if (mask[(size_t)y * w + x] != (c ? 0 : 255)) return fail("tile walk differs from the per-pixel predicate", h, w), -1;
            covered += c;
        }
    free(toggles); free(segs); free(mask);
    return covered;
}

int main()
{
    // the fixtures stated with the rule: h = 8, w = 9
    struct { std::vector<double> xy; int h, w; long long pixels; } fixtures[] = {
        {{0, 0, 0, 4, 4, 4, 4, 0}, 8, 9, 16},       {{1.5, 1.2, 7.3, 2.0, 4.1, 9.7}, 8, 9, 22}, {{1, 1, 7, 7, 7, 1, 1, 7}, 8, 9, 18},
        {{5, 2, 15, 2, 15, 6, 5, 6}, 8, 9, 16},     {{2, 5, 6, 5, 6, 12, 2, 12}, 8, 9, 12},     {{-5, 2, 3, 2, 3, 6, -5, 6}, 8, 9, 12},
        {{20, 20, 30, 20, 30, 30}, 8, 9, 0},        {{1, 3, 7, 3, 4, 3}, 8, 9, 0},              {{0, 0, 0, 1, 1, 1, 1, 0}, 1, 1, 1},
    };
    for (auto &f : fixtures)
        if (run(f.h, f.w, {polygon(f.xy, f.h, f.w)}) != f.pixels) return fail("a fixture's pixel count", f.h, f.w);

    // random polygons, three to a mask, on sizes around the tile shape and small ones
    const int sides_h[] = {1, 2, 7, CROWD_TH - 1, CROWD_TH, CROWD_TH + 1, 2 * CROWD_TH + 3, 71};
    const int sides_w[] = {1, 3, 9, CROWD_TW - 1, CROWD_TW, CROWD_TW + 1, 2 * CROWD_TW + 5, 71};
    int masks = 0;
    for (int h : sides_h)
        for (int w : sides_w)
            for (int rep = 0; rep < 3; ++rep) {
                std::vector<std::vector<uint32_t>> lists;
                for (int s = 0; s < 3; ++s) {
                    const int k = 3 + (int)(rnd() % 6);
                    std::vector<double> xy;
                    for (int j = 0; j < k; ++j) { xy.push_back(uniform(-4, w + 4)); xy.push_back(uniform(-4, h + 4)); }
                    lists.push_back(polygon(xy, h, w));
                }
                if (rep == 2) lists.push_back({(uint32_t)h * w});  // a toggle at h*w changes nothing
                if (rep == 1) lists.push_back({});                 // an empty segment
                if (run(h, w, lists) < 0) return 1;
                ++masks;
            }
    // random toggle lists, dense ones included (every position toggles)
    for (int h : sides_h)
        for (int w : sides_w) {
            std::vector<uint32_t> every, some;
            for (uint32_t i = 0; i <= (uint32_t)h * w; ++i) {
                every.push_back(i);
                if (rnd() % 5 == 0) some.push_back(i);
            }
            if (run(h, w, {every}) < 0 || run(h, w, {some, every}) < 0 || run(h, w, {}) != 0) return 1;
            masks += 3;
        }
    // the cancel step: even multiplicities drop out, odd ones stay once
    std::vector<uint32_t> c = {9, 3, 3, 7, 9, 9, 1, 7};
    crowd_cancel(c);
    if (c != std::vector<uint32_t>({1, 9})) return fail("cancel step", 0, 0);
    // the validation refuses a list that is not strictly increasing, and one above h*w
    {
        uint32_t bad[2] = {5, 5}, high[1] = {73};
        CrowdSegDesc sg{0, 2, 0, 8, 0};
        const CrowdMaskDesc d{0, 8, 9, 0, 1};
        if (!crowd_check_mask(d, &sg, 1, reinterpret_cast<const unsigned char *>(bad))) return fail("a repeated toggle was accepted", 8, 9);
        sg.count = 1;
        if (!crowd_check_mask(d, &sg, 1, reinterpret_cast<const unsigned char *>(high))) return fail("a toggle above h*w was accepted", 8, 9);
        const double nan_xy[6] = {0, 0, 1, NAN, 2, 2};
        if (!crowd_polygon_check(nan_xy, 3, 8, 9) || !crowd_polygon_check(nan_xy, 2, 8, 9)) return fail("a bad polygon was accepted", 8, 9);
    }
    printf("crowd_mask_host_check: %d masks, all equal to the per-pixel predicate\n", masks);
    return 0;
}
