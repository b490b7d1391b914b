// The segmentation overlay's host code (pytorch-human-pose_amd/csrc/seg_overlay_math.h: the tile cull, the column bitmasks of fills and
// lines, the blend, one frame walked tile by tile, the validation) compiled for the HOST and run over random tables, shapes partly and
// wholly outside the frame, empty frames, in-place and out-of-place frames and every refusal, so that the address arithmetic can be
// put under the sanitizers without a GPU:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I pytorch-human-pose_amd/csrc tools/seg_overlay_host_check.cpp -o /tmp/seg_overlay_host_check && /tmp/seg_overlay_host_check
//
// Frames, shape rows and toggles are heap blocks of exactly their size, so a read or write one element past any of them is an
// AddressSanitizer report.  Checked besides: the tile walk against a per-pixel restatement of the rule written here (toggle parity, the
// line rule walked along its major axis, the last covering row wins, the blend over every pixel), and that the validation accepts what
// is drawn here and refuses each broken table.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "seg_overlay_math.h"

static unsigned long long rng_state = 88172645463325252ull;
static unsigned rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (unsigned)(rng_state >> 33);
}
static int between(int lo, int hi) { return lo + (int)(rnd() % (unsigned)(hi - lo + 1)); }

static int fail(const char *what, int h, int w)
{
    printf("FAILED: %s (h = %d, w = %d)\n", what, h, w);
    return 1;
}

struct Tables {
    std::vector<SegShape> shapes;
    std::vector<uint32_t> toggles;
};

static void add_line(Tables &t, int colour, int xa, int ya, int xb, int yb) { t.shapes.push_back(SegShape{{HH_SEG_LINE, colour, xa, ya, xb, yb, 0, 0}}); }

// A random strictly increasing toggle list in 0 .. h*w as one fill row with the tightest column range.
static void add_fill(Tables &t, int colour, int h, int w, int every)
{
    const int first = (int)t.toggles.size();
    for (uint32_t i = 0; i <= (uint32_t)h * w; ++i)
        if (every <= 1 || rnd() % (unsigned)every == 0) t.toggles.push_back(i);
    const int n = (int)t.toggles.size() - first;
    int c = 0, d = 0;
    if (n > 0) {
        const uint32_t t0 = t.toggles[first], tl = t.toggles.back();
        c = (int)(t0 / (uint32_t)h) < w - 1 ? (int)(t0 / (uint32_t)h) : w - 1;
        d = (n & 1) ? w - 1 : (int)((tl - 1) / (uint32_t)h);
        if (d < c) d = c;
    }
    t.shapes.push_back(SegShape{{HH_SEG_FILL, colour, first, n, c, d, 0, 0}});
}

// The rule, pixel by pixel, written apart from the header's column-wise forms.
static void rule(const uint8_t *src, uint8_t *dst, const SegDesc &d, const Tables &t)
{
    const int h = d.h, w = d.w;
    std::vector<uint32_t> own((size_t)h * w, 0u);
    for (int i = 0; i < d.prim_count; ++i) {
        const int32_t *v = t.shapes[d.prim_offset + i].v;
        const uint32_t col = SEG_COVERED | (uint32_t)v[1];
        if (v[0] == HH_SEG_FILL) {
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) {
                    const auto first = t.toggles.begin() + v[2];
                    const long long below = std::upper_bound(first, first + v[3], (uint32_t)x * h + y) - first;  // toggles <= x * h + y
                    if (below & 1) own[(size_t)y * w + x] = col;
                }
            continue;
        }
        long long xa = v[2], ya = v[3], xb = v[4], yb = v[5];
        const long long dx = llabs(xb - xa), dy = llabs(yb - ya);
        auto put = [&](long long x, long long y) { if (x >= 0 && x < w && y >= 0 && y < h) own[(size_t)y * w + x] = col; };
        if (dx == 0 && dy == 0) { put(xa, ya); continue; }
        if (dx >= dy) {
            if (xa > xb) { std::swap(xa, xb); std::swap(ya, yb); }
            // clipped to the frame's columns: the endpoints may be 2^23 away
            for (long long x = std::max(xa, 0LL); x <= std::min(xb, (long long)w - 1); ++x) put(x, ya + seg_floor_div(2 * (x - xa) * (yb - ya) + dx, 2 * dx));
        } else {
            if (ya > yb) { std::swap(xa, xb); std::swap(ya, yb); }
            for (long long y = std::max(ya, 0LL); y <= std::min(yb, (long long)h - 1); ++y) put(xa + seg_floor_div(2 * (y - ya) * (xb - xa) + dy, 2 * dy), y);
        }
    }
    for (size_t p = 0; p < (size_t)h * w; ++p) {
        const uint32_t px = seg_pixel(src[3 * p] | src[3 * p + 1] << 8 | src[3 * p + 2] << 16, own[p], d.w0, d.w1, d.flags);
        dst[3 * p] = px & 255, dst[3 * p + 1] = px >> 8 & 255, dst[3 * p + 2] = px >> 16 & 255;
    }
}

// One frame through the tile walk in exactly sized heap blocks, out of place and in place, against the rule.
static int run(int h, int w, const Tables &t, float w0, float w1, int flags)
{
    const size_t bytes = (size_t)h * w * 3;
    SegShape *shapes = (SegShape *)malloc(t.shapes.empty() ? 1 : sizeof(SegShape) * t.shapes.size());
    uint32_t *toggles = (uint32_t *)malloc(t.toggles.empty() ? 1 : 4 * t.toggles.size());
    if (!t.shapes.empty()) memcpy(shapes, t.shapes.data(), sizeof(SegShape) * t.shapes.size());
    if (!t.toggles.empty()) memcpy(toggles, t.toggles.data(), 4 * t.toggles.size());
    uint8_t *src = (uint8_t *)malloc(bytes), *dst = (uint8_t *)malloc(bytes), *want = (uint8_t *)malloc(bytes);
    for (size_t i = 0; i < bytes; ++i) src[i] = (uint8_t)rnd();
    memset(dst, 0x5b, bytes);
    const SegDesc d{0, (long long)bytes, h, w, 0, (int32_t)t.shapes.size(), w0, w1, flags, 0};
    int bad = 0;
    if (const char *why = seg_check_frame(d, shapes, (long long)t.shapes.size(), toggles, (long long)t.toggles.size())) bad = fail(why, h, w);
    if (!bad) {
        rule(src, want, d, t);
        seg_frame_host(src, dst, d, shapes, toggles);
        if (memcmp(dst, want, bytes)) bad = fail("tile walk differs from the per-pixel rule", h, w);
        seg_frame_host(src, src, d, shapes, toggles);  // in place
        if (!bad && memcmp(src, want, bytes)) bad = fail("in place differs from out of place", h, w);
    }
    free(shapes); free(toggles); free(src); free(dst); free(want);
    return bad;
}

static int refused(const char *what, const SegDesc &d, const Tables &t, const char *word)
{
    const char *why = seg_check_frame(d, t.shapes.data(), (long long)t.shapes.size(), t.toggles.data(), (long long)t.toggles.size());
    if (why && strstr(why, word)) return 0;
    printf("FAILED: %s was %s%s\n", what, why ? "refused for another reason: " : "accepted", why ? why : "");
    return 1;
}

int main()
{
    const int sides_h[] = {1, 2, 7, SEG_ROWS - 1, SEG_ROWS + 1, SEG_TH - 1, SEG_TH, SEG_TH + 1, 2 * SEG_TH + 3, 45};
    const int sides_w[] = {1, 3, 37, SEG_TW - 1, SEG_TW, SEG_TW + 1, 2 * SEG_TW + 5, 300};
    int frames = 0;
    for (int h : sides_h)
        for (int w : sides_w)
            for (int rep = 0; rep < 3; ++rep) {
                Tables t;
                const int n = rep == 0 ? 0 : between(1, 12);  // rep 0: an empty frame, the pure blend
                for (int i = 0; i < n; ++i) {
                    const int colour = (int)(rnd() & 0xFFFFFF);
                    switch (rnd() % 6) {
                    case 0: add_fill(t, colour, h, w, between(2, 40)); break;
                    case 1: add_line(t, colour, between(-20, w + 20), between(-20, h + 20), between(-20, w + 20), between(-20, h + 20)); break;
                    case 2: add_line(t, colour, between(0, w - 1), between(0, h - 1), between(0, w - 1), between(0, h - 1)); break;
                    case 3: add_line(t, colour, w + between(5, 900), h + between(5, 900), w + between(5, 900), h + between(5, 900)); break;  // wholly outside
                    case 4: add_line(t, colour, -between(0, 1 << 23), between(-50, h + 50), between(0, 1 << 23), between(-50, h + 50)); break;  // far ends
                    default: add_line(t, colour, between(-9, w + 9), -between(0, 1 << 23), between(-9, w + 9), between(0, 1 << 23)); break;
                    }
                }
                if (rep == 2) {
                    add_fill(t, 0x123456, h, w, 1);               // every position toggles
                    t.shapes.push_back(SegShape{{HH_SEG_FILL, 1, (int)t.toggles.size(), 0, 0, 0, 0, 0}});  // an empty fill
                }
                if (run(h, w, t, rep == 1 ? 0.6f : 0.35f, rep == 1 ? 0.4f : 0.65f, rep == 2)) return 1;
                ++frames;
            }
    {   // more rows than one chunk: the draw order holds across chunks
        Tables t;
        add_fill(t, 0x0000FF, 40, 150, 7);
        for (int i = 0; i < SEG_CHUNK + 77; ++i) add_line(t, (int)(rnd() & 0xFFFFFF), between(-5, 155), between(-5, 45), between(-5, 155), between(-5, 45));
        add_fill(t, 0x00FF00, 40, 150, 300);
        if (run(40, 150, t, 0.6f, 0.4f, 0)) return 1;
        ++frames;
    }
    // every refusal of one frame (the call's own checks -- null pointers, n, counts, alignment -- need no table and are in capi.cpp)
    {
        Tables t;
        t.toggles = {9, 20};
        t.shapes.push_back(SegShape{{HH_SEG_FILL, 0x010203, 0, 2, 1, 2, 0, 0}});
        t.shapes.push_back(SegShape{{HH_SEG_LINE, 0x040506, -3, 2, 11, 5, 0, 0}});
        const SegDesc ok{0, 4096, 8, 8, 0, 2, 0.6f, 0.4f, 0, 0};
        if (seg_check_frame(ok, t.shapes.data(), 2, t.toggles.data(), 2)) return fail("a good frame was refused", 8, 8);
        SegDesc d = ok;
        int bad = 0;
        d = ok; d.h = 0; bad |= refused("h = 0", d, t, "size");
        d = ok; d.w = 16385; bad |= refused("w = 16385", d, t, "size");
        d = ok; d.src_offset = -1; bad |= refused("a negative src offset", d, t, "negative offset");
        d = ok; d.dst_offset = -4; bad |= refused("a negative dst offset", d, t, "negative offset");
        d = ok; d.dst_offset = 191; bad |= refused("a dst inside its src", d, t, "overlaps");
        d = ok; d.src_offset = 4096 + 100; bad |= refused("a src inside its dst", d, t, "overlaps");
        d = ok; d.dst_offset = 0; if (seg_check_frame(d, t.shapes.data(), 2, t.toggles.data(), 2)) bad |= fail("in place was refused", 8, 8);
        d = ok; d.prim_offset = 1; bad |= refused("a row range past the table", d, t, "outside the table");
        d = ok; d.prim_count = -1; bad |= refused("a negative row count", d, t, "outside the table");
        d = ok; d.w0 = NAN; bad |= refused("a NaN weight", d, t, "finite");
        d = ok; d.w1 = INFINITY; bad |= refused("an infinite weight", d, t, "finite");
        d = ok; d.flags = 2; bad |= refused("an unknown flag", d, t, "flag");
        d = ok; d.reserved = 7; bad |= refused("a reserved descriptor field", d, t, "reserved");
        struct { int row, col, value; const char *word; } edits[] = {
            {1, 0, 2, "kind"}, {1, 0, -1, "kind"}, {1, 1, 0x1000000, "colour"}, {0, 1, -1, "colour"}, {1, 6, 1, "reserved"}, {0, 7, 1, "reserved"},
            {1, 2, SEG_MAX_COORD + 1, "2^23"}, {1, 5, -SEG_MAX_COORD - 1, "2^23"}, {0, 2, 1, "toggle range"}, {0, 2, -1, "toggle range"}, {0, 3, 3, "toggle range"},
            {0, 3, -1, "toggle range"}, {0, 4, 2, "does not hold"}, {0, 5, 1, "does not hold"}, {0, 4, -1, "column range"}, {0, 5, 8, "column range"},
        };
        for (auto &e : edits) {
            Tables u = t;
            u.shapes[e.row].v[e.col] = e.value;
            bad |= refused("an edited row", ok, u, e.word);
        }
        { Tables u = t; u.toggles = {20, 9}; bad |= refused("descending toggles", ok, u, "increasing"); }
        { Tables u = t; u.toggles = {9, 9}; bad |= refused("a repeated toggle", ok, u, "increasing"); }
        { Tables u = t; u.toggles = {9, 65}; bad |= refused("a toggle above h*w", ok, u, "h*w"); }
        {
            std::vector<SegShape> many((size_t)HH_SEG_MAX_SHAPES + 1, SegShape{{HH_SEG_LINE, 0, 0, 0, 0, 0, 0, 0}});
            SegDesc m = ok;
            m.prim_count = (int32_t)many.size();
            const char *why = seg_check_frame(m, many.data(), (long long)many.size(), nullptr, 0);
            if (!why || !strstr(why, "HH_SEG_MAX_SHAPES")) bad |= fail("more than HH_SEG_MAX_SHAPES rows were accepted", 8, 8);
            m.prim_count = HH_SEG_MAX_SHAPES;
            if (seg_check_frame(m, many.data(), (long long)many.size(), nullptr, 0)) bad |= fail("exactly HH_SEG_MAX_SHAPES rows were refused", 8, 8);
        }
        if (bad) return 1;
    }
    printf("seg_overlay_host_check: %d frames, all equal to the per-pixel rule out of place and in place; every refusal refused\n", frames);
    return 0;
}
