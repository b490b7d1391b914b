// The shared code of the device JPEG index (pytorch-human-pose_amd/csrc/jpeg_dec_math.h: jpeg_bits_where, jpeg_idx_guess, jpeg_idx_walk,
// and the kernel's procedure in plain loops, jpeg_idx_sync_host) compiled for the HOST and fed malformed streams, so that its address
// arithmetic can be put under the sanitizers without a GPU:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I pytorch-human-pose_amd/csrc tools/jpeg_index_host_check.cpp -o /tmp/jpeg_index_host_check && /tmp/jpeg_index_host_check
//
// Three small restart-less streams are made with this project's own encoder (jpeg_math.h).  It writes one restart interval per MCU row,
// so each stream is ONE MCU row, which has no RSTm in its scan, with its DRI segment taken out: 16 x 200 at 4:2:0 and quality 90, 8 x 93
// at 4:4:4 and quality 75, 16 x 160 at 4:2:0 and quality 5 (blocks of a few bits).  Each is indexed whole, then
//   * cut at every length from 0 to its own (every truncation),
//   * with single bytes of its scan substituted: every position, by the fixed values 00 FF D0 D9 7F FE FD (those of the tests and more),
// at subsequences of 4, 16 and 128 bytes with 3, 64 and 1024 lanes per round and 1 and 3 MCUs per segment.  Every buffer is its own heap
// block of exactly its size: the stream ends with its last byte, the entries with the last entry.  A read or write one byte past either
// is an AddressSanitizer report, a signed overflow or oversized shift an UndefinedBehaviorSanitizer report.  Besides, every case must
// end as hh_jpeg_index_host ends on the same bytes: the same refusal, the same status, or the same entries byte for byte; and the
// passes must stay within the subsequence count.  Exit status 0: all of that held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_math.h"
#include "jpeg_dec_math.h"

static long long n_cases, n_refused, n_status[6], n_clean;

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

// A restart-less stream: one MCU row of width w (the encoder's one interval, so no RSTm in the scan) without its DRI segment.
static std::vector<unsigned char> restartless(int w, int sub, int quality)
{
    std::vector<unsigned char> s = make_stream(sub == 420 ? 16 : 8, w, sub, quality);
    // take out the DRI segment (FF DD 00 04 n n): with one interval there is no RSTm in the scan
    for (size_t at = 2; at + 6 <= s.size(); ++at)
        if (s[at] == 0xff && s[at + 1] == 0xdd) {
            s.erase(s.begin() + (long)at, s.begin() + (long)at + 6);
            break;
        }
    return s;
}

// One stream of exactly `len` bytes through both index passes -> 0 fine, 1 a check of this program failed.
static int check(const unsigned char *bytes, long long len, int mps, int B, int lanes)
{
    ++n_cases;
    unsigned char *stream = (unsigned char *)malloc(len ? (size_t)len : 1);
    memcpy(stream, bytes, (size_t)len);
    JpegStreamInfo I;
    JpegDecTables *T = (JpegDecTables *)malloc(sizeof(JpegDecTables));
    int bad = 0;
    const char *why = jpeg_dec_parse(stream, len, &I, T);
    if (why || I.restart_interval) {
        ++n_refused;
    } else {
        const int n = jpeg_dec_index_count(I, mps);
        JpegSegment *want = (JpegSegment *)malloc((size_t)n * sizeof(JpegSegment)), *got = (JpegSegment *)malloc((size_t)n * sizeof(JpegSegment));
        int nw = 0, sw = 0, ng = 0, sg = 0;
        JpegIdxCounts counts;
        const char *a = jpeg_dec_index(stream, len, I, *T, mps, want, n, &nw, &sw);
        const char *b = jpeg_idx_sync_host(stream, len, I, *T, mps, B, lanes, got, n, &ng, &sg, &counts);
        if ((a == nullptr) != (b == nullptr) || sw != sg || nw != ng) {
            bad = 1;
            fprintf(stderr, "FAILED: len %lld mps %d B %d lanes %d: host '%s' status %d n %d, lanes '%s' status %d n %d\n", len, mps, B, lanes, a ? a : "ok", sw, nw,
                    b ? b : "ok", sg, ng);
        } else if (!a && memcmp(want, got, (size_t)n * sizeof(JpegSegment))) {
            bad = 1;
            fprintf(stderr, "FAILED: len %lld mps %d B %d lanes %d: entries differ\n", len, mps, B, lanes);
        }
        if (counts.iterations > counts.subsequences || counts.iterations_worst > lanes || counts.rounds > (counts.subsequences + lanes - 1) / lanes) {
            bad = 1;
            fprintf(stderr, "FAILED: len %lld: %lld passes for %lld subsequences in %lld rounds\n", len, counts.iterations, counts.subsequences, counts.rounds);
        }
        if (sg < 0 || sg > 3) bad = 1, fprintf(stderr, "FAILED: status %d\n", sg);
        else ++n_status[sg];
        if (!sg) ++n_clean;
        free(want), free(got);
    }
    free(T), free(stream);
    return bad;
}

static int run(int w, int sub, int quality)
{
    const std::vector<unsigned char> good = restartless(w, sub, quality);
    JpegStreamInfo I;
    if (jpeg_dec_parse(good.data(), (long long)good.size(), &I, nullptr) || I.restart_interval)
        return fprintf(stderr, "FAILED: the intact stream is refused or has restarts\n"), 1;
    static const int PARAMS[][3] = {{1, 4, 3}, {1, 4, 64}, {3, 16, 64}, {1, 128, 1024}, {3, 16, 3}};
    int bad = 0;
    const long long before = n_clean;
    for (const auto &p : PARAMS) bad |= check(good.data(), (long long)good.size(), p[0], p[1], p[2]);
    if (n_clean - before != 5) return fprintf(stderr, "FAILED: the intact stream did not index\n"), 1;
    for (long long len = 0; len < (long long)good.size(); ++len)  // every truncation
        for (const auto &p : PARAMS) bad |= check(good.data(), len, p[0], p[1], p[2]);
    static const unsigned char VALUES[] = {0x00, 0xff, 0xd0, 0xd9, 0x7f, 0xfe, 0xfd};
    std::vector<unsigned char> trial = good;
    for (long long at = I.scan_offset; at < I.scan_end; ++at)
        for (unsigned char v : VALUES) {
            if (good[at] == v) continue;
            trial[at] = v;
            for (const auto &p : PARAMS) bad |= check(trial.data(), (long long)trial.size(), p[0], p[1], p[2]);
            trial[at] = good[at];
        }
    return bad;
}

int main()
{
    int bad = run(200, 420, 90);
    bad |= run(93, 444, 75);
    bad |= run(160, 420, 5);
    printf("%lld index passes: %lld refused by name, %lld clean, status 1..3: %lld %lld %lld; %s\n", n_cases, n_refused, n_clean, n_status[1], n_status[2],
           n_status[3], bad ? "FAILED" : "all checks passed");
    return bad;
}
