// The text labels' code (pytorch-human-pose_amd/csrc/text_math.h: the two primitive kinds on a pixel, the tile list, one tile walked
// chunk by chunk, the validation) compiled for the HOST and run over adversarial tables, so that the address arithmetic can be put
// under the sanitizers without a GPU:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I pytorch-human-pose_amd/csrc tools/text_host_check.cpp -o /tmp/text_host_check && /tmp/text_host_check
//
// Frame, table, tile list and atlas are heap blocks of exactly their sizes, so a read or write one byte past any of them is an
// AddressSanitizer report.  The tables: glyphs and boxes hanging off every edge, negative origins, boxes larger than the frame,
// primitives wholly outside, 1 x 1 frames, empty tables, maximal tables, counts around the chunk.  Checked besides: the tile walk
// equals a plain walk of the table over the whole frame, a byte outside every box keeps its value, the validation accepts what is
// drawn here and refuses one broken row of each kind.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "text_math.h"

static unsigned long long rng_state = 88172645463325252ull;
static unsigned rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (unsigned)(rng_state >> 33);
}
static int between(int lo, int hi) { return lo + (int)(rnd() % (unsigned)(hi - lo + 1)); }

static void clip(TextPrim &p, long long x0, long long y0, long long x1, long long y1, int h, int w)
{
    x0 = x0 < 0 ? 0 : x0; y0 = y0 < 0 ? 0 : y0; x1 = x1 > w - 1 ? w - 1 : x1; y1 = y1 > h - 1 ? h - 1 : y1;
    if (x0 > x1 || y0 > y1) x0 = y0 = 0, x1 = y1 = -1;
    p.x0 = (int16_t)x0; p.y0 = (int16_t)y0; p.x1 = (int16_t)x1; p.y1 = (int16_t)y1;
}

static const int ATLAS_LEN = 4099;  // (a prime: no glyph size divides it)

static TextPrim random_prim(int i, int h, int w)
{
    TextPrim p;
    memset(&p, 0, sizeof(p));
    for (uint8_t &v : p.rgb) v = (uint8_t)rnd();
    if (i % 4 == 0) {
        p.kind = HH_TEXT_BOX;
        p.A = (uint16_t)(i % 8 == 0);
        p.c = (float)(1.0 - 0.6); p.s = (float)0.6;
        const int x0 = between(-20, w + 5), y0 = between(-20, h + 5);
        clip(p, x0, y0, i % 12 == 0 ? x0 + w + 40 : x0 + between(0, 30), i % 12 == 0 ? y0 + h + 40 : y0 + between(0, 12), h, w);
    } else {
        p.kind = HH_TEXT_GLYPH;
        p.A = (uint16_t)between(1, 23); p.B = (uint16_t)between(1, 21);
        p.cx = between(-30, w + 5); p.cy = between(-25, h + 5);
        if (i % 31 == 7) p.cx = -(1 << 23);  // far outside: the box is empty
        if (i % 31 == 9) p.cy = 1 << 23;
        // the last glyph's coverage ends on the atlas's last byte
        p.c = (float)(i % 7 == 1 ? ATLAS_LEN - p.A * p.B : between(0, ATLAS_LEN - p.A * p.B));
        clip(p, p.cx, p.cy, (long long)p.cx + p.A - 1, (long long)p.cy + p.B - 1, h, w);
    }
    return p;
}

static int run(int h, int w, int count)
{
    const size_t bytes = (size_t)h * w * 3;
    uint8_t *frame = (uint8_t *)malloc(bytes), *plain = (uint8_t *)malloc(bytes), *src = (uint8_t *)malloc(bytes), *atlas = (uint8_t *)malloc(ATLAS_LEN);
    TextPrim *table = (TextPrim *)malloc(count ? sizeof(TextPrim) * count : 1);
    for (size_t i = 0; i < bytes; ++i) src[i] = (uint8_t)rnd();
    for (int i = 0; i < ATLAS_LEN; ++i) atlas[i] = (uint8_t)(rnd() % 3 ? rnd() : (rnd() & 1 ? 255 : 0));
    for (int i = 0; i < count; ++i) table[i] = random_prim(i, h, w);
    TextDesc d;
    memset(&d, 0, sizeof(d));
    d.h = h; d.w = w; d.prim_count = count;
    int bad = 0;
    const char *why = text_check_frame(d, table, count, ATLAS_LEN);
    if (why) { printf("  refused: %s\n", why); ++bad; }
    d.prim_count = count + 1;
    if (!text_check_frame(d, table, count, ATLAS_LEN)) { printf("  a range past the table was accepted\n"); ++bad; }
    d.prim_count = count;
    if (count > 1) {  // one broken row of each kind is refused
        TextPrim keep = table[1];
        table[1].c = (float)(ATLAS_LEN - table[1].A * table[1].B + 1);
        if (!text_check_frame(d, table, count, ATLAS_LEN)) { printf("  a coverage range past the atlas was accepted\n"); ++bad; }
        table[1] = keep; table[1].x0 = table[1].y0 = table[1].y1 = 0; table[1].x1 = (int16_t)w;
        if (!text_check_frame(d, table, count, ATLAS_LEN)) { printf("  a box past the frame was accepted\n"); ++bad; }
        table[1] = keep;
    }
    if (bad) {
        free(frame); free(plain); free(src); free(atlas); free(table);
        return bad;
    }

    // the tile walk, over exactly the listed tiles
    const size_t ntiles = (size_t)text_xtiles(w) * text_ytiles(h);
    uint8_t *seen = (uint8_t *)malloc(ntiles);
    const long long nt = text_list_tiles(d, table, 0, seen, nullptr, 0);
    TextTile *tiles = (TextTile *)malloc(nt ? sizeof(TextTile) * nt : 1);
    if (text_list_tiles(d, table, 0, seen, tiles, nt) != nt) ++bad;
    TextPrim *list = (TextPrim *)malloc(sizeof(TextPrim) * TEXT_CHUNK);
    memcpy(frame, src, bytes);
    for (long long i = 0; i < nt; ++i) text_tile_host(frame, d, table, atlas, tiles[i].tile, list);
    // a plain walk of the table over the whole frame
    memcpy(plain, src, bytes);
    std::vector<uint8_t> covered((size_t)h * w, 0);
    for (int i = 0; i < count; ++i)
        for (int y = table[i].y0; y <= table[i].y1; ++y)
            for (int x = table[i].x0; x <= table[i].x1; ++x) {
                uint8_t *q = plain + ((size_t)y * w + x) * 3;
                const uint32_t v = text_apply(table[i], atlas, x, y, q[0] | q[1] << 8 | q[2] << 16);
                q[0] = v & 255, q[1] = (v >> 8) & 255, q[2] = (v >> 16) & 255;
                covered[(size_t)y * w + x] = 1;
            }
    size_t changed = 0, cover = 0;
    for (size_t i = 0; i < bytes; ++i) {
        if (frame[i] != plain[i]) { ++bad; break; }
        if (!covered[i / 3] && frame[i] != src[i]) { ++bad; break; }
        changed += frame[i] != src[i];
    }
    for (uint8_t c : covered) cover += c;
    printf("%5d x %5d, %4d primitives, %3lld of %3zu tiles: %zu pixels covered, %zu bytes changed%s\n", h, w, count, nt, ntiles, cover, changed, bad ? "  FAILED" : "");
    free(frame); free(plain); free(src); free(atlas); free(table); free(seen); free(tiles); free(list);
    return bad;
}

int main()
{
    int bad = 0;
    const int sizes[][2] = {{1, 1}, {5, 7}, {TEXT_TH, TEXT_TW}, {TEXT_TH - 1, TEXT_TW + 1}, {TEXT_TH + 1, TEXT_TW - 1}, {2 * TEXT_TH + 3, 3 * TEXT_TW - 1},
                            {3, 2 * TEXT_TW + 2}, {200, 1}};
    const int counts[] = {0, 1, 2, TEXT_CHUNK - 1, TEXT_CHUNK, TEXT_CHUNK + 1, HH_TEXT_MAX_PRIMS};
    for (const auto &s : sizes)
        for (int c : counts) bad += run(s[0], s[1], c);
    printf(bad ? "FAILED\n" : "text_host_check: clean\n");
    return bad ? 1 : 0;
}
