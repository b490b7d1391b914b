// The window decode's shared code (pytorch-human-pose_amd/csrc/jpeg_dec_math.h: the MCU rectangle, the selection of segments, the
// rebased table block, the windowed segment walk, the rectangle's IDCT and planes, the colour step) compiled for the HOST and fed
// malformed streams, so that its address arithmetic can be put under the sanitizers without a GPU:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I pytorch-human-pose_amd/csrc tools/jpeg_window_host_check.cpp -o /tmp/jpeg_window_host_check && /tmp/jpeg_window_host_check
//
// This is a stand-alone program for a CPU: it is not run on a GPU machine and not loaded into Python.
//
// Three small streams are made with this project's own encoder (33 x 50 and 20 x 37 at 4:2:0, 17 x 23 at 4:4:4, the samplings it writes; one
// restart interval per MCU row; h2v1 addresses are covered by tests/test_jpeg_window_cpu.py, without the sanitizers).  Each is decoded through a handful of windows (the whole image, 1 x 1 at a corner, a window that starts at an MCU
// edge, one that ends one before an MCU edge, one that touches the right and bottom edge, a one-pixel-high and a one-pixel-wide one)
//   * cut at every length from its scan's start to its own (every truncation),
//   * with single bytes of its scan substituted: every 3rd position, by the fixed values 00 FF D0 D9 7F FE,
// through the restart segments of the cut or substituted stream and through an index of one MCU per segment taken from the intact
// stream.  Every buffer is its own heap block of exactly the size the rule promises: the shipped slice ends with its last byte,
// the table block is jpeg_dec_tables_bytes(selected segments), the workspace is the rectangle's ws_bytes, the destination is
// height x 3 * width.  A read or write one byte outside any of them is an AddressSanitizer report.  Besides: the extents the
// segment walk reports must lie inside the slice and the rectangle's coefficients; every case ends in a refusal by name, a status
// or a clean decode; and no status-0 result differs from the same rows and columns of the whole-image decode of the same bytes
// through the same segments (jpeg_dec_segment + jpeg_dec_window_pixels_host over the MCU grid, whatever status that decode has: damage outside the walked part
// is not the window's).  Exit status 0: all of that held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_math.h"
#include "jpeg_dec_math.h"

static long long n_refused, n_status[6], n_clean, n_cases, n_compared;

static std::vector<unsigned char> make_stream(int h, int w, int sub, int quality)
{
    JpegDesc d;
    memset(&d, 0, sizeof(d));
    d.h = h, d.w = w, d.quality = quality, d.subsampling = sub, d.pitch = 3ll * w;
    const JpegGeom g = jpeg_geom(h, w, sub);
    d.out_capacity = jpeg_bound(g);
    std::vector<unsigned char> src((size_t)h * w * 3), out((size_t)d.out_capacity);
    unsigned long long s = 88172645463325252ull;
    for (size_t i = 0; i < src.size(); ++i) {
        s ^= s << 13, s ^= s >> 7, s ^= s << 17;
        const size_t y = i / (3 * w), x = i % (3 * w) / 3;
        src[i] = (unsigned char)((x * 5 + y * 3 + ((s >> 33) & 63)) & 255);  // a gradient with noise on it
    }
    void *work = nullptr;
    if (posix_memalign(&work, 16, (size_t)g.nblk * 128)) abort();
    out.resize((size_t)jpeg_encode_host(src.data(), d, out.data(), (int16_t *)work));
    free(work);
    return out;
}

// The whole image of `len` bytes through `seg`, whatever the status -> its pixels [h][w][3].
static std::vector<unsigned char> whole(const unsigned char *stream, long long len, const JpegStreamInfo &I, const JpegDecTables &T, const std::vector<JpegSegment> &seg)
{
    const JpegWinRect R = jpeg_full_rect(I);
    const JpegDecGeom g = jpeg_dec_geom(I, R);
    void *ws = nullptr;
    if (posix_memalign(&ws, 16, (size_t)g.ws_bytes)) abort();
    memset(ws, 0, (size_t)g.ws_bytes);
    for (size_t s = 0; s < seg.size(); ++s) jpeg_dec_segment(stream, (int)len, I, T.huff, seg[s], R, (int16_t *)ws, nullptr, nullptr);
    std::vector<unsigned char> px((size_t)I.h * I.w * 3);
    jpeg_dec_window_pixels_host((unsigned char *)ws, I, T, jpeg_full_window(I), false, px.data(), 3ll * I.w);
    free(ws);
    return px;
}

// One window decode of `len` bytes at `bytes` (an exact heap copy is made) through the given segments (nullptr: the stream's restart
// segments) -> 0 fine, 1 a check of this program failed.
static int decode(const unsigned char *bytes, long long len, const std::vector<JpegSegment> *index, const JpegWindow &W)
{
    ++n_cases;
    unsigned char *stream = (unsigned char *)malloc(len ? (size_t)len : 1);
    memcpy(stream, bytes, (size_t)len);
    JpegStreamInfo I;
    JpegDecTables *T = (JpegDecTables *)malloc(sizeof(JpegDecTables));
    int bad = 0;
    const char *why = jpeg_dec_parse(stream, len, &I, T);
    std::vector<JpegSegment> seg;
    if (!why) {
        if (index) seg = *index;
        else {
            seg.resize(I.nseg_restart ? I.nseg_restart : 1);
            if (I.nseg_restart) why = jpeg_dec_restart_segments(stream, I, seg.data());
            else seg[0] = JpegSegment{0, I.mcols * I.mrows, (int32_t)I.scan_offset, 0, {0, 0, 0}, (int32_t)(I.scan_end << 1)};
        }
    }
    if (!why) why = jpeg_win_check(I, W);
    int nsel = 0;
    long long slice[2] = {0, 0};
    JpegWinRect R;
    memset(&R, 0, sizeof(R));
    if (!why) {
        R = jpeg_win_rect(I, W);
        if (R.mx0 < 0 || R.my0 < 0 || R.mx1 >= I.mcols || R.my1 >= I.mrows || R.cols < 1 || R.rows < 1) bad = 1, fprintf(stderr, "FAILED: the rectangle leaves the grid\n");
        why = jpeg_win_select(I, R, seg.data(), (int)seg.size(), &nsel, slice);
    }
    if (why) {
        ++n_refused;
    } else {
        if (slice[0] < I.scan_offset || slice[1] > I.scan_end || slice[1] > len || slice[0] >= slice[1]) bad = 1, fprintf(stderr, "FAILED: the slice leaves the scan\n");
        const long long part_len = slice[1] - slice[0];
        unsigned char *part = (unsigned char *)malloc((size_t)part_len);
        memcpy(part, stream + slice[0], (size_t)part_len);
        void *block = nullptr, *ws = nullptr;
        const JpegDecGeom g = jpeg_dec_geom(I, R);
        if (posix_memalign(&block, 16, (size_t)jpeg_dec_tables_bytes(nsel)) || posix_memalign(&ws, 16, (size_t)g.ws_bytes)) abort();
        jpeg_win_tables(I, *T, R, seg.data(), (int)seg.size(), slice, (unsigned char *)block);
        memset(ws, 0x5a, (size_t)g.ws_bytes);
        unsigned char *dst = (unsigned char *)malloc((size_t)W.height * W.width * 3);
        JpegExtent ext = {0, 0};
        JpegWinCounts counts = {0, 0, 0, 0, 0, 0};
        const int status = jpeg_dec_window_host(part, (int)part_len, (const unsigned char *)block, nsel, W, false, (unsigned char *)ws, dst, 3ll * W.width, &counts, &ext);
        if (status < 0 || status > 5) bad = 1, fprintf(stderr, "FAILED: status %d\n", status);
        if (ext.max_byte > part_len || ext.max_coef > (long long)g.nblk * 64) {
            bad = 1;
            fprintf(stderr, "FAILED: extents: byte %lld of %lld, coefficient %lld of %lld\n", ext.max_byte, part_len, ext.max_coef, (long long)g.nblk * 64);
        }
        if (counts.mcus_stored > (long long)R.cols * R.rows || counts.segments_walked > nsel) bad = 1, fprintf(stderr, "FAILED: counts\n");
        if (status >= 0 && status <= 5) ++n_status[status];
        if (!status) {
            ++n_clean;
            if (counts.mcus_stored != (long long)R.cols * R.rows) bad = 1, fprintf(stderr, "FAILED: a clean decode stored %lld of %d MCUs\n", counts.mcus_stored, R.cols * R.rows);
            const std::vector<unsigned char> full = whole(stream, len, I, *T, seg);
            for (int y = 0; y < W.height && !bad; ++y)
                if (memcmp(dst + (size_t)y * W.width * 3, full.data() + ((size_t)(W.top + y) * I.w + W.left) * 3, (size_t)W.width * 3)) {
                    bad = 1;
                    fprintf(stderr, "FAILED: a status-0 window (%d,%d,%d,%d) differs from the whole decode in row %d (length %lld)\n", W.top, W.left, W.height, W.width, y, len);
                }
            ++n_compared;
        }
        free(dst), free(ws), free(block), free(part);
    }
    free(T), free(stream);
    return bad;
}

static int run(int h, int w, int sub, int quality)
{
    const std::vector<unsigned char> good = make_stream(h, w, sub, quality);
    JpegStreamInfo I;
    std::vector<JpegDecTables> T(1);
    if (jpeg_dec_parse(good.data(), (long long)good.size(), &I, &T[0])) return fprintf(stderr, "FAILED: the intact stream is refused\n"), 1;
    std::vector<JpegSegment> index((size_t)jpeg_dec_index_count(I, 1));
    int n = 0, st = 0;
    if (jpeg_dec_index(good.data(), (long long)good.size(), I, T[0], 1, index.data(), (int)index.size(), &n, &st) || n != (int)index.size())
        return fprintf(stderr, "FAILED: the intact stream could not be indexed\n"), 1;
    const int Mh = 8 * I.vs, Mw = 8 * I.hs;
    const JpegWindow windows[] = {{0, 0, h, w}, {h - 1, w - 1, 1, 1}, {Mh, Mw, h - Mh, 5}, {1, 1, Mh - 1, Mw - 1}, {h - 3, w - 9, 3, 9}, {Mh - 1, 0, 1, w}, {0, Mw, h, 1}};
    int bad = 0;
    const long long clean_before = n_clean;
    for (const JpegWindow &W : windows) {
        bad |= decode(good.data(), (long long)good.size(), nullptr, W);
        bad |= decode(good.data(), (long long)good.size(), &index, W);
    }
    if (n_clean - clean_before != 2 * (long long)(sizeof(windows) / sizeof(windows[0]))) return fprintf(stderr, "FAILED: the intact stream did not decode\n"), 1;
    for (long long len = I.scan_offset; len < (long long)good.size(); ++len)  // every truncation (the header's are hh_jpeg_parse's refusals)
        for (const JpegWindow &W : windows) {
            bad |= decode(good.data(), len, nullptr, W);
            bad |= decode(good.data(), len, &index, W);
        }
    static const unsigned char VALUES[] = {0x00, 0xff, 0xd0, 0xd9, 0x7f, 0xfe};
    std::vector<unsigned char> trial = good;
    for (long long at = I.scan_offset; at < I.scan_end; at += 3)
        for (unsigned char v : VALUES) {
            if (good[at] == v) continue;
            trial[at] = v;
            for (const JpegWindow &W : windows) {
                bad |= decode(trial.data(), (long long)trial.size(), nullptr, W);
                bad |= decode(trial.data(), (long long)trial.size(), &index, W);
            }
            trial[at] = good[at];
        }
    return bad;
}

int main()
{
    int bad = run(33, 50, 420, 90);
    bad |= run(17, 23, 444, 75);
    bad |= run(20, 37, 420, 60);
    printf("%lld window decodes: %lld refused by name, %lld clean (%lld compared with the whole decode), status 1..5: %lld %lld %lld %lld %lld; %s\n", n_cases,
           n_refused, n_clean, n_compared, n_status[1], n_status[2], n_status[3], n_status[4], n_status[5], bad ? "FAILED" : "all checks passed");
    return bad;
}
