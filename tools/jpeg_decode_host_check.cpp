// The JPEG decoder's shared code (pytorch-human-pose_amd/csrc/jpeg_dec_math.h: marker walk, restart scan, index pass, the segment
// decoder the entropy kernel compiles, IDCT, upsampling, colour) compiled for the HOST and fed malformed streams, so that its address
// arithmetic can be put under the sanitizers without a GPU:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I pytorch-human-pose_amd/csrc tools/jpeg_decode_host_check.cpp -o /tmp/jpeg_decode_host_check && /tmp/jpeg_decode_host_check
//
// Two small streams are made with this project's own encoder (jpeg_math.h: 33 x 50 at 4:2:0 and 17 x 23 at 4:4:4, the "own" entries of
// tests/golden/jpeg_decode.npz; one restart interval per MCU row).  Each is decoded whole, then
//   * cut at every length from 0 to its own (every truncation),
//   * with single bytes of its scan substituted: every 3rd position, by the fixed values 00 FF D0 D9 7F FE,
// through the restart segments and through an index of one MCU per segment taken from the intact stream (bit offsets inside
// intervals).  Every buffer is its own heap block of exactly the size the rule promises: the stream ends with its last byte, the
// workspace is hh_jpeg_decode_workspace_bytes, the destination ends with the last pixel.  A read or write one byte past any of them
// is an AddressSanitizer report, a signed overflow or oversized shift an UndefinedBehaviorSanitizer report.  Besides, the extents the
// segment decoder reports (last stream byte read, last coefficient written) must lie inside the stream and the coefficient area, and
// every case must end in a refusal by name, a status, or a clean decode; decoding the intact streams through the index must give
// the same pixels.  Exit status 0: all of that held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_math.h"
#include "jpeg_dec_math.h"

static long long n_refused, n_status[6], n_clean, n_cases;

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

// One decode of `len` bytes at `bytes` (an exact heap copy is made) through the given segments (nullptr: the stream's restart segments).
// -> 0 fine, 1 a check of this program failed.  pixels_out: receives the pixels of a clean decode.
static int decode(const unsigned char *bytes, long long len, const std::vector<JpegSegment> *index, std::vector<unsigned char> *pixels_out, int *status_out)
{
    ++n_cases;
    unsigned char *stream = (unsigned char *)malloc(len ? (size_t)len : 1);
    memcpy(stream, bytes, (size_t)len);
    JpegStreamInfo I;
    JpegDecTables *T = (JpegDecTables *)malloc(sizeof(JpegDecTables));
    int bad = 0, status = 0;
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
    if (why) {
        ++n_refused;
        status = -1;
    } else {
        const JpegWinRect R = jpeg_full_rect(I);  // the whole image: the rectangle is the MCU grid
        const JpegDecGeom g = jpeg_dec_geom(I, R);
        void *ws = nullptr;
        if (posix_memalign(&ws, 16, (size_t)g.ws_bytes)) abort();
        memset(ws, 0x5a, (size_t)g.ws_bytes);
        JpegExtent ext = {0, 0};
        for (size_t s = 0; s < seg.size(); ++s) {
            const int st = jpeg_dec_segment(stream, (int)len, I, T->huff, seg[s], R, (int16_t *)ws, nullptr, &ext);
            if (st < 0 || st > 5) bad = 1, fprintf(stderr, "FAILED: status %d\n", st);
            else if (st > status) status = st;
        }
        if (ext.max_byte > len || ext.max_byte > I.scan_end || ext.max_coef > (long long)g.nblk * 64) {
            bad = 1;
            fprintf(stderr, "FAILED: extents: byte %lld of %lld, coefficient %lld of %lld\n", ext.max_byte, len, ext.max_coef, (long long)g.nblk * 64);
        }
        // steps b to d run whatever the status, as the kernels do: the planes and the destination stay inside their blocks
        unsigned char *dst = (unsigned char *)malloc((size_t)I.h * I.w * 3);
        jpeg_dec_window_pixels_host((unsigned char *)ws, I, *T, jpeg_full_window(I), false, dst, 3ll * I.w);
        if (!status && pixels_out) pixels_out->assign(dst, dst + (size_t)I.h * I.w * 3);
        ++n_status[status];
        if (!status) ++n_clean;
        free(dst), free(ws);
    }
    if (status_out) *status_out = status;
    free(T), free(stream);
    return bad;
}

static int run(int h, int w, int sub, int quality)
{
    const std::vector<unsigned char> good = make_stream(h, w, sub, quality);
    std::vector<unsigned char> want, got;
    int status = 0, bad = decode(good.data(), (long long)good.size(), nullptr, &want, &status);
    if (status || want.empty()) return fprintf(stderr, "FAILED: the intact stream did not decode (status %d)\n", status), 1;
    // the index of the intact stream: one MCU per segment, and the same pixels through it
    JpegStreamInfo I;
    std::vector<JpegDecTables> T(1);
    if (jpeg_dec_parse(good.data(), (long long)good.size(), &I, &T[0])) return 1;
    std::vector<JpegSegment> index((size_t)jpeg_dec_index_count(I, 1));
    int n = 0, st = 0;
    if (jpeg_dec_index(good.data(), (long long)good.size(), I, T[0], 1, index.data(), (int)index.size(), &n, &st) || n != (int)index.size())
        return fprintf(stderr, "FAILED: the intact stream could not be indexed\n"), 1;
    bad |= decode(good.data(), (long long)good.size(), &index, &got, &status);
    if (status || got != want) return fprintf(stderr, "FAILED: decoding through the index differs\n"), 1;

    for (long long len = 0; len < (long long)good.size(); ++len) {  // every truncation
        bad |= decode(good.data(), len, nullptr, nullptr, nullptr);
        if (len > I.scan_offset) bad |= decode(good.data(), len, &index, nullptr, nullptr);
        // the index pass itself on the cut stream
        JpegStreamInfo Ic;
        std::vector<unsigned char> cut(good.begin(), good.begin() + len);
        if (!jpeg_dec_parse(cut.data(), len, &Ic, &T[0])) {
            std::vector<JpegSegment> e((size_t)jpeg_dec_index_count(Ic, 1));
            jpeg_dec_index(cut.data(), len, Ic, T[0], 1, e.data(), (int)e.size(), &n, &st);
        }
    }
    static const unsigned char VALUES[] = {0x00, 0xff, 0xd0, 0xd9, 0x7f, 0xfe};
    std::vector<unsigned char> trial = good;
    for (long long at = I.scan_offset; at < I.scan_end; at += 3)
        for (unsigned char v : VALUES) {
            if (good[at] == v) continue;
            trial[at] = v;
            got.clear();
            bad |= decode(trial.data(), (long long)trial.size(), nullptr, nullptr, nullptr);
            bad |= decode(trial.data(), (long long)trial.size(), &index, nullptr, nullptr);
            JpegStreamInfo Ic;
            if (!jpeg_dec_parse(trial.data(), (long long)trial.size(), &Ic, &T[0])) {
                std::vector<JpegSegment> e((size_t)jpeg_dec_index_count(Ic, 1));
                jpeg_dec_index(trial.data(), (long long)trial.size(), Ic, T[0], 1, e.data(), (int)e.size(), &n, &st);
            }
            trial[at] = good[at];
        }
    return bad;
}

int main()
{
    int bad = run(33, 50, 420, 90);
    bad |= run(17, 23, 444, 75);
    printf("%lld decodes: %lld refused by name, %lld clean, status 1..5: %lld %lld %lld %lld %lld; %s\n", n_cases, n_refused, n_clean, n_status[1],
           n_status[2], n_status[3], n_status[4], n_status[5], bad ? "FAILED" : "all checks passed");
    return bad;
}
