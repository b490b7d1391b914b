// The heatmap panels' code (pytorch-human-pose_amd/csrc/panel_math.h: the four value paths, the range, quantise / colour / blend, one
// figure in plain loops, the validation) compiled for the HOST and run over figures of a few sizes, so that the address arithmetic can be
// put under the sanitizers without a GPU:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I pytorch-human-pose_amd/csrc tools/panels_host_check.cpp -o /tmp/panels_host_check && /tmp/panels_host_check
//
// Every source plane, the image, the colour table and the canvas are heap blocks of exactly their size (the canvas exactly
// (Hc - 1) * pitch + Wc * 3 bytes), so a read or write one element past any of them is an AddressSanitizer report.  Checked besides:
// every byte of every canvas row was written (the block starts as 0xA5; padding and unused cells must come out 0, cells are compared
// with a second run), the bytes between a row's end and the pitch were not, the validation accepts what is painted here and refuses a
// cell one pixel outside the canvas, a wrong DIRECT size and a kind out of range.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "panel_math.h"

static unsigned long long rng_state = 88172645463325252ull;
static unsigned rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (unsigned)(rng_state >> 33);
}

static float *plane(int h, int w, int special)
{
    float *p = (float *)malloc(sizeof(float) * h * w);
    for (int i = 0; i < h * w; ++i) p[i] = (float)(rnd() % 4001) / 1000.f - 1.5f;
    if (special == 0) for (int i = 0; i < h * w; ++i) p[i] = 0.37f;
    if (special == 1) p[(h / 2) * w + w / 3] = NAN;
    if (special == 2) p[0] = INFINITY, p[h * w - 1] = -INFINITY;
    return p;
}

static int run(int hq, int wq, int K, int nrows, int pad, int slack)
{
    const int H = 4 * hq, W = 4 * wq, n = 4 * K;
    const int ncols = (K + nrows - 1) / nrows, gh = (H + pad) * nrows + pad, gw = (W + pad) * ncols + pad;
    const int Hc = 4 * gh, Wc = gw;
    const long long pitch = (long long)Wc * 3 + slack;
    std::vector<PanelMap> maps(n);
    std::vector<float *> blocks;
    for (int kind = 0; kind < 4; ++kind)
        for (int k = 0; k < K; ++k) {
            PanelMap &m = maps[kind * K + k];
            memset(&m, 0, sizeof(m));
            m.kind = kind;
            m.flags = (k + kind) % 4;
            m.h = kind == HH_PANEL_DIRECT ? H : (kind == HH_PANEL_SINGLE && (k & 1) ? 2 * hq : hq);
            m.w = kind == HH_PANEL_DIRECT ? W : (kind == HH_PANEL_SINGLE && (k & 1) ? 2 * wq : wq);
            float *a = plane(m.h, m.w, k), *b = kind == HH_PANEL_AVERAGE ? plane(2 * hq, 2 * wq, -1) : nullptr;
            blocks.push_back(a);
            if (b) blocks.push_back(b);
            m.src = a; m.src2 = b;
            m.oy = kind * gh + pad + (k / ncols) * (H + pad);
            m.ox = pad + (k % ncols) * (W + pad);
        }
    uint8_t *image = (uint8_t *)malloc((size_t)H * W * 3), *lut = (uint8_t *)malloc(768);
    for (size_t i = 0; i < (size_t)H * W * 3; ++i) image[i] = (uint8_t)rnd();
    for (int i = 0; i < 768; ++i) lut[i] = (uint8_t)rnd();
    const size_t bytes = (size_t)(Hc - 1) * pitch + (size_t)Wc * 3;
    uint8_t *canvas = (uint8_t *)malloc(bytes), *again = (uint8_t *)malloc(bytes);
    memset(canvas, 0xA5, bytes);
    memset(again, 0x5A, bytes);
    std::vector<PanelRange> ranges(n);

    int bad = 0;
    const char *why = panel_check(maps.data(), n, H, W, Hc, Wc, pitch);
    if (why) { printf("  refused: %s\n", why); ++bad; }
    PanelMap keep = maps[n - 1];
    maps[n - 1].ox = Wc - W + 1;
    if (!panel_check(maps.data(), n, H, W, Hc, Wc, pitch)) { printf("  a cell one pixel outside the canvas was accepted\n"); ++bad; }
    maps[n - 1] = keep;
    maps[n - 1].kind = 4;
    if (!panel_check(maps.data(), n, H, W, Hc, Wc, pitch)) { printf("  a kind out of range was accepted\n"); ++bad; }
    maps[n - 1] = keep;
    keep = maps[0];
    maps[0].h = H - 1;
    if (!panel_check(maps.data(), n, H, W, Hc, Wc, pitch)) { printf("  a DIRECT map of the wrong size was accepted\n"); ++bad; }
    maps[0] = keep;

    if (!bad) {
        panel_figure_host(maps.data(), n, image, H, W, lut, canvas, Hc, Wc, pitch, ranges.data());
        panel_figure_host(maps.data(), n, image, H, W, lut, again, Hc, Wc, pitch, ranges.data());
        std::vector<char> in_cell((size_t)Hc * Wc, 0);
        for (const PanelMap &m : maps)
            for (int y = 0; y < H; ++y) memset(&in_cell[(size_t)(m.oy + y) * Wc + m.ox], 1, W);
        size_t zero_outside = 0, outside = 0;
        for (int y = 0; y < Hc && !bad; ++y) {
            for (int b = 0; b < Wc * 3; ++b) {
                const uint8_t v = canvas[(size_t)y * pitch + b];
                if (v != again[(size_t)y * pitch + b]) { ++bad; break; }  // 0xA5 vs 0x5A: a byte neither run wrote
                if (!in_cell[(size_t)y * Wc + b / 3]) { ++outside; zero_outside += v == 0; }
            }
            if (y < Hc - 1)
                for (long long b = (long long)Wc * 3; b < pitch; ++b)
                    if (canvas[(size_t)y * pitch + b] != 0xA5) ++bad;  // the slack of a row is not touched
        }
        if (zero_outside != outside) ++bad;
    }
    printf("%3d x %3d quarter, K %2d, %d rows, pad %d, pitch + %d: %d maps on %d x %d%s\n", hq, wq, K, nrows, pad, slack, n, Hc, Wc, bad ? "  FAILED" : "");
    for (float *b : blocks) free(b);
    free(image); free(lut); free(canvas); free(again);
    return bad;
}

int main()
{
    int bad = 0;
    const int sizes[][2] = {{1, 1}, {5, 7}, {8, 12}, {16, 16}, {3, 33}};
    for (const auto &s : sizes)
        for (int K : {1, 3, 17})
            for (int nrows : {1, 2}) bad += run(s[0], s[1], K, nrows, 5, (K + nrows) % 4);
    bad += run(5, 7, 3, 2, 0, 0);
    // the un-normalise and the quantiser on values around and beyond their ranges
    const float xs[] = {-3.f, -2.1179f, 0.f, 2.64f, 3.f, 1e30f, -1e30f, NAN, INFINITY, -INFINITY};
    unsigned sum = 0;
    for (float x : xs) sum += panel_unnormalize(x, 0.229, 0.485) + panel_level(x * 255.0f);
    printf(bad ? "FAILED\n" : "panels_host_check: clean (%u)\n", sum);
    return bad ? 1 : 0;
}
