// The arithmetic of the baseline JPEG encoder (jpeg.hip; the rule is stated at hh_jpeg_encode_u8_batch in include/hhrnet.h), kept apart
// from the kernels so that the same text also compiles for the host (hh_debug_jpeg_encode_host, tools/jpeg_host_check.cpp): the frame
// descriptor and its geometry, the worst-case size bound, colour, 4:2:0 subsampling, the two FDCT passes, the quantiser, the Huffman
// code tables, one block's walk over its zigzag coefficients (templated on where the codes go), the header writer, and a whole frame
// encoded in plain loops.  Integer arithmetic only.
#ifndef HH_JPEG_MATH_H
#define HH_JPEG_MATH_H
#include <stdint.h>
#include <string.h>

#include "../../include/hhrnet.h"
#include "host_dev.h"

using JpegDesc = hh_jpeg_desc;
static_assert(sizeof(hh_jpeg_desc) == 64, "ABI 3");

// The worst case of one block: a DC code of at most 11 bits (chrominance, category 11) with 11 value bits, and 63 coefficients that
// are all non-zero, each an AC code of at most 16 bits with at most 10 value bits (|AC| <= 1023).  A zero coefficient never costs more:
// a ZRL (at most 11 bits) stands for 16 of them and the EOB (at most 4 bits) needs one.
enum { JPEG_BLOCK_BITS = 22 + 63 * 26 };
static_assert(JPEG_BLOCK_BITS == 1660, "stated in include/hhrnet.h");
// SOI 2, APP0 18, DQT 2 x 69, SOF0 19, DHT 2 x 33 + 2 x 183, DRI 6, SOS 14
enum { JPEG_HEADER_BYTES = 2 + 18 + 2 * 69 + 19 + 2 * 33 + 2 * 183 + 6 + 14 };
static_assert(JPEG_HEADER_BYTES == 629, "stated in include/hhrnet.h");
// The entropy kernel: one wave per restart interval, a lane per block, JPEG_ENT_LANES blocks per pass through an LDS bit buffer that
// holds their worst case plus the 7 bits carried over from the pass before.
enum { JPEG_ENT_LANES = 64, JPEG_ENT_WORDS = (JPEG_ENT_LANES * JPEG_BLOCK_BITS + 7 + 31) / 32 + 1 };
enum { JPEG_MCUS_PER_GROUP = 4 };  // the transform kernel: a wave per MCU, four to a workgroup

struct JpegGeom {
    int mcu;               // 16 (420) or 8 (444)
    int bpm;               // blocks per MCU: 6 (Y Y Y Y Cb Cr) or 3 (Y Cb Cr)
    int mcols, mrows;      // MCUs per row (= the restart interval), MCU rows (= the number of intervals)
    int nblk;              // blocks per interval
    long long slot;        // bytes of workspace per interval: its worst case, rounded up to 16
    long long coef_bytes;  // int16 zigzag coefficients of the whole frame
    long long ws_bytes;    // coefficients | slots | int32 interval lengths, a multiple of 16
};
// the worst-case bytes of one interval of nblk blocks: every bit used, padded to a byte, every byte stuffed
HH_HD long long jpeg_interval_bound(long long nblk) { return 2 * ((nblk * JPEG_BLOCK_BITS + 7) / 8); }
HH_HD JpegGeom jpeg_geom(int h, int w, int subsampling)
{
    JpegGeom g;
    g.mcu = subsampling == 420 ? 16 : 8;
    g.bpm = subsampling == 420 ? 6 : 3;
    g.mcols = (w + g.mcu - 1) / g.mcu;
    g.mrows = (h + g.mcu - 1) / g.mcu;
    g.nblk = g.mcols * g.bpm;
    g.slot = (jpeg_interval_bound(g.nblk) + 15) / 16 * 16;
    g.coef_bytes = (long long)g.mrows * g.nblk * 128;
    g.ws_bytes = g.coef_bytes + g.mrows * g.slot + ((long long)g.mrows * 4 + 15) / 16 * 16;
    return g;
}
// the worst-case bytes of the stream: header, every interval at its bound followed by a marker (RSTm, or EOI after the last)
HH_HD long long jpeg_bound(const JpegGeom &g) { return JPEG_HEADER_BYTES + g.mrows * (jpeg_interval_bound(g.nblk) + 2); }

// T[u][x] = round(2^14 c(u) cos((2x + 1) u pi / 16)), c(0) = sqrt(1/8), c(u) = 1/2
static constexpr int16_t JPEG_T[64] = {
    5793,  5793,  5793,  5793,  5793,  5793,  5793,  5793,
    8035,  6811,  4551,  1598, -1598, -4551, -6811, -8035,
    7568,  3135, -3135, -7568, -7568, -3135,  3135,  7568,
    6811, -1598, -8035, -4551,  4551,  8035,  1598, -6811,
    5793, -5793, -5793,  5793,  5793, -5793, -5793,  5793,
    4551, -8035,  1598,  6811, -6811, -1598,  8035, -4551,
    3135, -7568,  7568, -3135, -3135,  7568, -7568,  3135,
    1598, -4551,  6811, -8035,  8035, -6811,  4551, -1598};
// the zigzag position of natural index v * 8 + u
static constexpr uint8_t JPEG_INVZZ[64] = {
     0,  1,  5,  6, 14, 15, 27, 28,
     2,  4,  7, 13, 16, 26, 29, 42,
     3,  8, 12, 17, 25, 30, 41, 43,
     9, 11, 18, 24, 31, 40, 44, 53,
    10, 19, 23, 32, 39, 45, 52, 54,
    20, 22, 33, 38, 46, 51, 55, 60,
    21, 34, 37, 47, 50, 56, 59, 61,
    35, 36, 48, 49, 57, 58, 62, 63};
// Annex K quantisation tables (luminance, chrominance), in zigzag order
static constexpr uint8_t JPEG_QBASE[2][64] = {
    {16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37, 29, 40, 58, 51, 61, 60, 57, 51,
     56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101, 103, 99},
    {17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// Annex K Huffman tables: BITS (codes of length 1..16) and HUFFVAL, for DC luminance, DC chrominance, AC luminance, AC chrominance
static constexpr uint8_t JPEG_DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
static constexpr uint8_t JPEG_DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};  // (both tables)
static constexpr uint8_t JPEG_AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
static constexpr uint8_t JPEG_AC_VALS[2][162] = {
    {1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51, 98, 114,
     130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89,
     90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148,
     149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197,
     198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244,
     245, 246, 247, 248, 249, 250},
    {0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98, 114, 209, 10,
     22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89,
     90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147,
     148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196,
     197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245,
     246, 247, 248, 249, 250}};

// Q of zigzag position k in table `tbl` (0 luminance, 1 chrominance) at `quality` 1..100: libjpeg's jpeg_quality_scaling
HH_HD int jpeg_quant(int quality, int tbl, int k)
{
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int q = (JPEG_QBASE[tbl][k] * scale + 50) / 100;
    return q < 1 ? 1 : q > 255 ? 255 : q;
}

// One pixel -> Y, Cb, Cr (libjpeg's 16-bit fixed point; every numerator is positive, so >> is a plain division).
HH_HD void jpeg_ycc(int r, int g, int b, int &y, int &cb, int &cr)
{
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// The share of lane 0..63 in the samples (value - 128) of MCU (my, mx): smp holds the MCU's blocks, 64 values each in natural order.
// 444: the lane's one pixel into blocks 0 (Y), 1 (Cb), 2 (Cr).  420: the lane's 2 x 2 pixels into the Y blocks 0..3 (left to right, top
// to bottom) and their rounded mean chroma into blocks 4 (Cb) and 5 (Cr).  Pixels beyond the frame repeat its last row and column:
// every source index is y * pitch + x * 3 + c with y < h, x < w, c < 3.
HH_HD void jpeg_mcu_samples(const unsigned char *src, const JpegDesc &d, int my, int mx, int lane, int32_t *smp)
{
    const int swap = d.flags & 1;
    if (d.subsampling == 420) {
        const int gy = lane >> 3, gx = lane & 7;
        int scb = 0, scr = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int py = 2 * gy + (e >> 1), px = 2 * gx + (e & 1);
            const int y = my * 16 + py < d.h ? my * 16 + py : d.h - 1, x = mx * 16 + px < d.w ? mx * 16 + px : d.w - 1;
            const unsigned char *p = src + (size_t)y * (size_t)d.pitch + (size_t)x * 3;
            int Y, cb, cr;
            jpeg_ycc(p[swap ? 2 : 0], p[1], p[swap ? 0 : 2], Y, cb, cr);
            smp[((py >> 3) * 2 + (px >> 3)) * 64 + (py & 7) * 8 + (px & 7)] = Y - 128;
            scb += cb, scr += cr;
        }
        smp[4 * 64 + lane] = ((scb + 2) >> 2) - 128;
        smp[5 * 64 + lane] = ((scr + 2) >> 2) - 128;
    } else {
        const int py = lane >> 3, px = lane & 7;
        const int y = my * 8 + py < d.h ? my * 8 + py : d.h - 1, x = mx * 8 + px < d.w ? mx * 8 + px : d.w - 1;
        const unsigned char *p = src + (size_t)y * (size_t)d.pitch + (size_t)x * 3;
        int Y, cb, cr;
        jpeg_ycc(p[swap ? 2 : 0], p[1], p[swap ? 0 : 2], Y, cb, cr);
        smp[lane] = Y - 128, smp[64 + lane] = cb - 128, smp[128 + lane] = cr - 128;
    }
}

// Row pass, in place on one row of 8 samples: A[u] = (sum_x s[x] T[u][x] + 1024) >> 11.  |s| <= 128 and the largest row sum of |T| is
// 8 * 5793 = 46344, so |A| <= (46344 * 128 + 1024) >> 11 = 2897.
HH_HD void jpeg_fdct_row(int32_t *row)
{
    int32_t s[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) s[x] = row[x];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        int32_t acc = 0;
#pragma unroll
        for (int x = 0; x < 8; ++x) acc += s[x] * JPEG_T[u * 8 + x];
        row[u] = (acc + 1024) >> 11;
    }
}

// Column pass of column u of one block: F[v] = sum_y A[y][u] T[v][y] = 2^17 x the coefficient; |F| <= 2897 * 46344 < 2^27.1.
HH_HD void jpeg_fdct_col(const int32_t *A, int u, int32_t F[8])
{
    int32_t a[8];
#pragma unroll
    for (int y = 0; y < 8; ++y) a[y] = A[y * 8 + u];
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        int32_t acc = 0;
#pragma unroll
        for (int y = 0; y < 8; ++y) acc += a[y] * JPEG_T[v * 8 + y];
        F[v] = acc;
    }
}

// q = sign(F) ((|F| + (Q << 16)) / (Q << 17)), clamped to -1024..1023 (DC) or +-1023 (AC).  |F| + (Q << 16) < 2^27.1 + 2^24 < 2^32.
HH_HD int jpeg_quantise(int32_t F, int Q, bool dc)
{
    const uint32_t a = F < 0 ? 0u - (uint32_t)F : (uint32_t)F;
    int q = (int)((a + ((uint32_t)Q << 16)) / ((uint32_t)Q << 17));
    if (q > 1023) q = F < 0 && dc ? (q > 1024 ? 1024 : q) : 1023;
    return F < 0 ? -q : q;
}

// Column u of one block through the column pass and the quantiser, into the block's zigzag order.  Qzz: this component's 64 divisors.
HH_HD void jpeg_fdct_col_quant(const int32_t *A, int u, const uint16_t *Qzz, int16_t *zz)
{
    int32_t F[8];
    jpeg_fdct_col(A, u, F);
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        const int k = JPEG_INVZZ[v * 8 + u];
        zz[k] = (int16_t)jpeg_quantise(F[v], Qzz[k], k == 0);
    }
}

// Block j of an interval (MCU j / bpm, block j % bpm of it): is it luminance, and which block holds its DC prediction (-1: none, 0).
HH_HD bool jpeg_block_is_luma(int j, int bpm) { return bpm == 6 ? j % 6 < 4 : j % 3 == 0; }
HH_HD int jpeg_pred_block(int j, int bpm)
{
    if (bpm == 3) return j - 3;  // (negative in the first MCU)
    const int k = j % 6;
    if (k >= 1 && k <= 3) return j - 1;
    return j < 6 ? -1 : k == 0 ? j - 3 : j - 6;
}

// Canonical codes from BITS / HUFFVAL: table[symbol] = length << 16 | code.  The table must be zero before.
HH_HD void jpeg_build_codes(const uint8_t *bits, const uint8_t *vals, uint32_t *table)
{
    uint32_t code = 0;
    int p = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) table[vals[p++]] = (uint32_t)len << 16 | code++;
        code <<= 1;
    }
}
struct JpegCodes {
    uint32_t dc[2][16], ac[2][256];
};
HH_HD void jpeg_build_table(JpegCodes *c, int t)  // t = 0..3: DC luminance, DC chrominance, AC luminance, AC chrominance
{
    if (t < 2) jpeg_build_codes(JPEG_DC_BITS[t], JPEG_DC_VALS, c->dc[t]);
    else jpeg_build_codes(JPEG_AC_BITS[t - 2], JPEG_AC_VALS[t - 2], c->ac[t - 2]);
}

// size category of v: the number of bits of |v|
HH_HD int jpeg_category(int v)
{
    uint32_t a = v < 0 ? -v : v;
    int s = 0;
    while (a) ++s, a >>= 1;
    return s;
}
// Huffman code of `symbol` followed by the s value bits of v (v itself if positive, v - 1 in s bits if negative) -> sink.put(bits, count)
template <class Sink>
HH_HD void jpeg_put_value(const uint32_t *table, int symbol, int v, int s, Sink &sink)
{
    const uint32_t e = table[symbol];
    const uint32_t value = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1u);
    sink.put((e & 0xffffu) << s | value, (int)(e >> 16) + s);  // at most 16 + 10 bits (AC), 11 + 11 (DC)
}
struct alignas(16) JpegVec8 {
    int16_t v[8];
};
// One block: its DC difference to `pred`, then the run-length coded AC coefficients, ZRL for runs above 15, EOB unless coefficient 63
// is non-zero.  zz: 64 zigzag coefficients, 16-byte aligned, read as eight 16-byte vectors.
template <class Sink>
HH_HD void jpeg_code_block(const int16_t *zz, int pred, const uint32_t *dc, const uint32_t *ac, Sink &sink)
{
    int run = 0;
#pragma unroll 1
    for (int g = 0; g < 8; ++g) {
        const JpegVec8 q = *reinterpret_cast<const JpegVec8 *>(zz + g * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int v = q.v[e];
            if (g == 0 && e == 0) {
                const int diff = v - pred;
                const int s = jpeg_category(diff);
                jpeg_put_value(dc, s, diff, s, sink);
                continue;
            }
            if (v == 0) {
                ++run;
                continue;
            }
            while (run > 15) {
                sink.put(ac[0xf0] & 0xffffu, (int)(ac[0xf0] >> 16));
                run -= 16;
            }
            const int s = jpeg_category(v);
            jpeg_put_value(ac, run << 4 | s, v, s, sink);
            run = 0;
        }
    }
    if (run > 0) sink.put(ac[0] & 0xffffu, (int)(ac[0] >> 16));
}
struct JpegCountSink {
    int bits;
    HH_HD void put(uint32_t, int count) { bits += count; }
};

// The JPEG_HEADER_BYTES bytes in front of the first interval: SOI, APP0, DQT 0, DQT 1, SOF0, DHT DC0 DC1 AC0 AC1, DRI, SOS.
HH_HD int jpeg_write_header(unsigned char *o, int h, int w, int subsampling, int quality, int mcols)
{
    int n = 0;
#define JPEG_B(x) o[n++] = (unsigned char)(x)
#define JPEG_W(x) JPEG_B((x) >> 8), JPEG_B((x) & 255)
    JPEG_W(0xffd8);
    JPEG_W(0xffe0), JPEG_W(16), JPEG_B('J'), JPEG_B('F'), JPEG_B('I'), JPEG_B('F'), JPEG_B(0), JPEG_W(0x0101), JPEG_B(0), JPEG_W(1), JPEG_W(1), JPEG_W(0);
    for (int t = 0; t < 2; ++t) {
        JPEG_W(0xffdb), JPEG_W(67), JPEG_B(t);
        for (int k = 0; k < 64; ++k) JPEG_B(jpeg_quant(quality, t, k));
    }
    JPEG_W(0xffc0), JPEG_W(17), JPEG_B(8), JPEG_W(h), JPEG_W(w), JPEG_B(3);
    JPEG_B(1), JPEG_B(subsampling == 420 ? 0x22 : 0x11), JPEG_B(0);
    JPEG_B(2), JPEG_B(0x11), JPEG_B(1);
    JPEG_B(3), JPEG_B(0x11), JPEG_B(1);
    for (int t = 0; t < 4; ++t) {
        const bool isdc = t < 2;
        const uint8_t *bits = isdc ? JPEG_DC_BITS[t] : JPEG_AC_BITS[t - 2];
        const uint8_t *vals = isdc ? JPEG_DC_VALS : JPEG_AC_VALS[t - 2];
        const int count = isdc ? 12 : 162;
        JPEG_W(0xffc4), JPEG_W(2 + 1 + 16 + count), JPEG_B(isdc ? t : 0x10 | (t - 2));
        for (int i = 0; i < 16; ++i) JPEG_B(bits[i]);
        for (int i = 0; i < count; ++i) JPEG_B(vals[i]);
    }
    JPEG_W(0xffdd), JPEG_W(4), JPEG_W(mcols);
    JPEG_W(0xffda), JPEG_W(12), JPEG_B(3), JPEG_B(1), JPEG_B(0x00), JPEG_B(2), JPEG_B(0x11), JPEG_B(3), JPEG_B(0x11), JPEG_B(0), JPEG_B(63), JPEG_B(0);
#undef JPEG_W
#undef JPEG_B
    return n;
}

// What a frame's descriptor must satisfy before anything is launched or encoded; nullptr if it does.
inline const char *jpeg_check_desc(const JpegDesc &d)
{
    if (d.h < 1 || d.w < 1 || d.h > 65535 || d.w > 65535) return "h and w must lie in 1..65535";
    if (d.quality < 1 || d.quality > 100) return "quality outside 1..100";
    if (d.subsampling != 420 && d.subsampling != 444) return "subsampling must be 420 or 444";
    if (d.pitch < 3ll * d.w) return "pitch below 3 * w";
    if (d.flags & ~1) return "unknown flag";
    const long long bound = jpeg_bound(jpeg_geom(d.h, d.w, d.subsampling));
    if (bound > INT32_MAX) return "the frame's bound exceeds the int32 of its length";
    if (d.out_capacity < bound) return "output capacity below hh_jpeg_bound";
    if (d.src_offset < 0 || d.out_offset < 0 || d.ws_offset < 0) return "negative offset";
    if (d.ws_offset % 16) return "ws_offset must be a multiple of 16";
    return nullptr;
}

// Bits to bytes on the host: most significant bit first, FF followed by 00.
struct JpegHostSink {
    unsigned char *out;
    long long pos;
    uint64_t acc;
    int nacc;
    HH_HD void put(uint32_t bits, int count)
    {
        acc = acc << count | bits;
        nacc += count;
        while (nacc >= 8) {
            const unsigned char b = (unsigned char)(acc >> (nacc - 8));
            out[pos++] = b;
            if (b == 0xff) out[pos++] = 0;
            nacc -= 8;
        }
    }
};

// The whole rule on the host: src is the frame's own buffer (src_offset, out_offset and ws_offset are not applied), out holds at least
// jpeg_bound bytes, work holds jpeg_geom().nblk * 64 coefficients (16-byte aligned).  -> the stream's length.
inline long long jpeg_encode_host(const unsigned char *src, const JpegDesc &d, unsigned char *out, int16_t *work)
{
    const JpegGeom g = jpeg_geom(d.h, d.w, d.subsampling);
    JpegCodes codes;
    memset(&codes, 0, sizeof(codes));
    for (int t = 0; t < 4; ++t) jpeg_build_table(&codes, t);
    uint16_t Q[2][64];
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k) Q[t][k] = (uint16_t)jpeg_quant(d.quality, t, k);
    long long pos = jpeg_write_header(out, d.h, d.w, d.subsampling, d.quality, g.mcols);
    for (int my = 0; my < g.mrows; ++my) {
        for (int mx = 0; mx < g.mcols; ++mx) {
            int32_t smp[6 * 64];
            for (int lane = 0; lane < 64; ++lane) jpeg_mcu_samples(src, d, my, mx, lane, smp);
            for (int t = 0; t < g.bpm * 8; ++t) jpeg_fdct_row(smp + t * 8);
            for (int t = 0; t < g.bpm * 8; ++t)
                jpeg_fdct_col_quant(smp + (t >> 3) * 64, t & 7, Q[jpeg_block_is_luma(t >> 3, g.bpm) ? 0 : 1], work + ((size_t)mx * g.bpm + (t >> 3)) * 64);
        }
        JpegHostSink sink = {out, pos, 0, 0};
        for (int j = 0; j < g.nblk; ++j) {
            const int pj = jpeg_pred_block(j, g.bpm), t = jpeg_block_is_luma(j, g.bpm) ? 0 : 1;
            jpeg_code_block(work + (size_t)j * 64, pj < 0 ? 0 : work[(size_t)pj * 64], codes.dc[t], codes.ac[t], sink);
        }
        if (sink.nacc) sink.put((1u << (8 - sink.nacc)) - 1u, 8 - sink.nacc);
        pos = sink.pos;
        out[pos++] = 0xff;
        out[pos++] = (unsigned char)(my + 1 < g.mrows ? 0xd0 + (my & 7) : 0xd9);
    }
    return pos;
}
#endif
