// The baseline JPEG decoder (jpeg_decode.hip; the rule is stated at hh_jpeg_decode_u8_batch in include/hhrnet.h), kept apart from the
// kernels so that the same text compiles for the host (hh_jpeg_parse, hh_jpeg_index_host, hh_debug_jpeg_decode_host,
// hh_debug_jpeg_decode_window_host, tools/jpeg_decode_host_check.cpp, tools/jpeg_window_host_check.cpp): the marker walk with its
// refusals, the Huffman lookup tables, the bit reader, one segment's entropy decode, libjpeg's islow IDCT, its fancy upsampling, the
// colour step, and a decode in plain loops.  A decode is always the decode of a window's MCU rectangle (hh_jpeg_decode_window_u8_batch);
// the whole image is the window that covers it, whose rectangle is the MCU grid.  What only a true window needs comes last: the
// selection of segments and the rebased table block.  Integer arithmetic only; `>>` is an arithmetic shift.
#ifndef HH_JPEG_DEC_MATH_H
#define HH_JPEG_DEC_MATH_H
#include <stdint.h>
#include <string.h>
#include <vector>  // (the host twin of the index, jpeg_idx_sync_host)

#include "../../include/hhrnet.h"
#include "host_dev.h"

// The tables of the decode are the public structs.  hh_jpeg_dec_desc.tables_offset leads to JpegStreamInfo | JpegDecTables | nseg
// JpegSegment at a multiple of 16; a hh_jpeg_win_desc is a hh_jpeg_dec_desc, whose stream is the shipped slice, and the window.
using JpegStreamInfo = hh_jpeg_stream_info;
using JpegSegment = hh_jpeg_segment;
using JpegDecDesc = hh_jpeg_dec_desc;
using JpegWindow = hh_jpeg_window;
using JpegWinDesc = hh_jpeg_win_desc;
using JpegWinCounts = hh_jpeg_window_counts;
static_assert(sizeof(hh_jpeg_stream_info) == 112 && sizeof(hh_jpeg_segment) == 32 && sizeof(hh_jpeg_dec_desc) == 64 && sizeof(hh_jpeg_window) == 16 &&
              sizeof(hh_jpeg_win_desc) == 80 && sizeof(hh_jpeg_window_counts) == 48, "ABI 3");

// One Huffman table as the decoder reads it: the 8-bit first level (length << 8 | symbol, 0: longer than 8 bits or no code), and for the
// lengths 9..16 libjpeg's maxcode / valptr pair (valoff = valptr - mincode; maxcode -1: no code of that length).
struct JpegHuff {
    uint16_t look[256];
    int32_t maxcode[18];
    int32_t valoff[18];
    uint8_t vals[256];
};
static_assert(sizeof(JpegHuff) == 912, "table layout");
struct JpegDecTables {
    uint16_t q[4][64];  // natural order
    JpegHuff huff[8];   // DC 0..3, AC 0..3
};
static_assert(sizeof(JpegDecTables) == 7808 && sizeof(JpegDecTables) % 16 == 0, "table layout");
enum { JPEG_DEC_TABLES_AT = sizeof(JpegStreamInfo), JPEG_DEC_SEGS_AT = sizeof(JpegStreamInfo) + sizeof(JpegDecTables) };
HH_HD long long jpeg_dec_tables_bytes(long long nseg) { return JPEG_DEC_SEGS_AT + nseg * (long long)sizeof(JpegSegment); }

// status_dev codes
enum { JPEG_ST_OK = 0, JPEG_ST_BAD_CODE = 1, JPEG_ST_RUN = 2, JPEG_ST_EXHAUSTED = 3, JPEG_ST_RESTART = 4, JPEG_ST_SEGMENT = 5 };
enum { JPEG_DEC_IDCT_BLOCKS = 32, JPEG_DEC_LDS_STRIDE = 72 };  // the IDCT kernel: 8 lanes per block, 32 blocks per workgroup

// the natural index v * 8 + u of zigzag position k
static constexpr uint8_t JPEG_ZZ[64] = {
     0,  1,  8, 16,  9,  2,  3, 10, 17, 24, 32, 25, 18, 11,  4,  5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13,  6,  7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// The MCU rectangle of a window inside the image: an output pixel of a subsampled axis reads its chroma sample and one neighbour on
// each side (rule c), clamped to the component's true size, so luma rows t..b need chroma rows max(0, (t >> 1) - 1) ..
// min(ch - 1, (b >> 1) + 1) when vs == 2, and likewise across with hs (also for h2v1).  The rectangle is the MCUs that hold the
// window's luma samples and those chroma samples.
struct JpegWinRect {
    int mx0, mx1, my0, my1;  // inclusive
    int cols, rows;
};
HH_HD JpegWinRect jpeg_win_rect(const JpegStreamInfo &I, const JpegWindow &W)
{
    const int t = W.top, b = W.top + W.height - 1, l = W.left, r = W.left + W.width - 1;
    JpegWinRect R;
    R.mx0 = l / (8 * I.hs), R.mx1 = r / (8 * I.hs), R.my0 = t / (8 * I.vs), R.my1 = b / (8 * I.vs);
    if (I.ncomp == 3 && I.hs == 2) {
        const int cw = (I.w + 1) / 2, c0 = (l >> 1) - 1 < 0 ? 0 : (l >> 1) - 1, c1 = (r >> 1) + 1 > cw - 1 ? cw - 1 : (r >> 1) + 1;
        R.mx0 = c0 / 8 < R.mx0 ? c0 / 8 : R.mx0, R.mx1 = c1 / 8 > R.mx1 ? c1 / 8 : R.mx1;
    }
    if (I.ncomp == 3 && I.vs == 2) {
        const int ch = (I.h + 1) / 2, c0 = (t >> 1) - 1 < 0 ? 0 : (t >> 1) - 1, c1 = (b >> 1) + 1 > ch - 1 ? ch - 1 : (b >> 1) + 1;
        R.my0 = c0 / 8 < R.my0 ? c0 / 8 : R.my0, R.my1 = c1 / 8 > R.my1 ? c1 / 8 : R.my1;
    }
    R.cols = R.mx1 - R.mx0 + 1, R.rows = R.my1 - R.my0 + 1;
    return R;
}
// The whole image as a window, and its rectangle: the MCU grid (mx1 = (w - 1) / (8 hs) = mcols - 1, and likewise down).
HH_HD JpegWindow jpeg_full_window(const JpegStreamInfo &I) { return JpegWindow{0, 0, I.h, I.w}; }
HH_HD JpegWinRect jpeg_full_rect(const JpegStreamInfo &I) { return jpeg_win_rect(I, jpeg_full_window(I)); }

// The workspace of a rectangle's decode: its coefficients, then its component planes (cw / ch stay the image's).
struct JpegDecGeom {
    int nmcu, nblk;            // MCUs and blocks of the rectangle
    int pw[3], ph[3];          // the padded component planes: whole blocks
    int cw[3], ch[3];          // the components' true sizes
    long long coef_bytes;      // int16 [nblk][64], natural order, not yet dequantised
    long long plane_at[3];     // from the image's workspace
    long long ws_bytes;        // a multiple of 16
};
HH_HD JpegDecGeom jpeg_dec_geom(const JpegStreamInfo &I, const JpegWinRect &R)
{
    JpegDecGeom g;
    g.nmcu = R.cols * R.rows;
    g.nblk = g.nmcu * I.bpm;
    g.coef_bytes = (long long)g.nblk * 128;
    long long at = g.coef_bytes;
    for (int c = 0; c < 3; ++c) {
        const int hs = c == 0 ? I.hs : 1, vs = c == 0 ? I.vs : 1;
        const bool have = c < I.ncomp;
        g.pw[c] = have ? R.cols * hs * 8 : 0;
        g.ph[c] = have ? R.rows * vs * 8 : 0;
        g.cw[c] = c == 0 ? I.w : (I.w + I.hs - 1) / I.hs;
        g.ch[c] = c == 0 ? I.h : (I.h + I.vs - 1) / I.vs;
        g.plane_at[c] = at;
        at += ((long long)g.pw[c] * g.ph[c] + 15) / 16 * 16;
    }
    g.ws_bytes = at;
    return g;
}

// ---------------------------------------------------------------------------------------------------------------- the bit reader
// A 64-bit buffer refilled bytewise (four bytes at once where none of them is FF): FF 00 gives FF, any other FF xx (a marker) and the end of the segment's bytes end the data; what is
// read beyond is zero bits, counted in `fake`.  Every byte read lies in [0, end).
struct JpegBits {
    const unsigned char *p;
    int pos, end;
    uint64_t acc;  // the low n bits are unread
    int n, fake;
    bool stop;
    HH_HD void init(const unsigned char *bytes, int at, int limit)
    {
        p = bytes, pos = at, end = limit, acc = 0, n = 0, fake = 0, stop = false;
    }
    HH_HD void refill()
    {
        // four bytes at once while they lie inside the segment and none of them is FF (no stuffing, no marker) ...
        while (n <= 32 && !stop && pos + 4 <= end) {
            uint32_t w;
            memcpy(&w, p + pos, 4);
            if (((w & 0x7f7f7f7fu) + 0x01010101u) & w & 0x80808080u) break;  // (exact: a byte is FF iff its low 7 bits carry into a set top bit)
            w = w << 24 | (w & 0xff00u) << 8 | (w >> 8 & 0xff00u) | w >> 24;  // the first byte is the most significant
            acc = acc << 32 | w;
            n += 32, pos += 4;
        }
        if (n > 32) return;  // (at least 33 bits: a code and its value take at most 31)
        // ... bytewise otherwise
        while (n <= 56) {
            uint32_t b = 0;
            if (!stop && pos < end) {
                b = p[pos];
                if (b == 0xff) {
                    if (pos + 1 < end && p[pos + 1] == 0) pos += 2;
                    else stop = true, b = 0;
                } else {
                    pos += 1;
                }
            } else {
                stop = true;
            }
            if (stop) fake += 8;
            acc = acc << 8 | b;
            n += 8;
        }
    }
    HH_HD uint32_t peek(int k) const { return (uint32_t)(acc >> (n - k)) & ((1u << k) - 1u); }  // 1 <= k <= 16 <= n
    HH_HD void drop(int k) { n -= k; }
    HH_HD bool starved() const { return n < fake; }  // bits that are not there were consumed
    HH_HD int real() const { return n - fake; }      // unread bits of the stream in the buffer
};

// The canonical position of a reader that is not starved: the byte that holds the next unread bit and that bit's index in it, found by
// going back from the reader's position over the unread bits.  An FF 00 pair is one byte and the position points at its FF.  `floor`:
// where the reader began (no byte before it is looked at).
HH_HD void jpeg_bits_where(const JpegBits &br, int floor, int &p, int &bit)
{
    int unread = br.real();
    p = br.pos;
    while (unread >= 8) {  // a whole data byte back: FF 00 is one
        --p;
        if (br.p[p] == 0 && p > floor && br.p[p - 1] == 0xff) --p;
        unread -= 8;
    }
    if (unread) {
        --p;
        if (br.p[p] == 0 && p > floor && br.p[p - 1] == 0xff) --p;
    }
    bit = unread ? 8 - unread : 0;
}

// -> the symbol, or -1 for a code no table entry has.  Needs 16 bits in the buffer.
HH_HD int jpeg_dec_symbol(JpegBits &br, const JpegHuff &H)
{
    const uint32_t e = H.look[br.peek(8)];
    if (e) {
        br.drop((int)(e >> 8));
        return (int)(e & 255u);
    }
#pragma unroll 1
    for (int l = 9; l <= 16; ++l) {
        const int code = (int)br.peek(l);
        if (code <= H.maxcode[l]) {  // (maxcode -1: no code of this length)
            br.drop(l);
            return H.vals[(code + H.valoff[l]) & 255];
        }
    }
    return -1;
}
HH_HD int jpeg_dec_extend(uint32_t v, int s) { return (int)v < (1 << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

// One block.  STORE: blk receives the 64 coefficients (natural order; zero first).  pred: the component's DC predictor.
template <bool STORE>
HH_HD int jpeg_dec_block(JpegBits &br, const JpegHuff &dc, const JpegHuff &ac, int &pred, int16_t *blk)
{
    if (STORE) {
        struct alignas(16) Z { int16_t v[8]; };
        Z z = {};
#pragma unroll
        for (int i = 0; i < 8; ++i) reinterpret_cast<Z *>(blk)[i] = z;
    }
    br.refill();
    int s = jpeg_dec_symbol(br, dc);
    if (br.starved()) return JPEG_ST_EXHAUSTED;
    if (s < 0 || s > 15) return JPEG_ST_BAD_CODE;
    if (s) {
        pred = (int)((uint32_t)pred + (uint32_t)jpeg_dec_extend(br.peek(s), s));  // (wraps in a malformed stream)
        br.drop(s);
    }
    if (br.starved()) return JPEG_ST_EXHAUSTED;
    if (STORE) blk[0] = (int16_t)pred;
#pragma unroll 1
    for (int k = 1; k < 64; ++k) {
        br.refill();
        const int rs = jpeg_dec_symbol(br, ac);
        if (br.starved()) return JPEG_ST_EXHAUSTED;  // (before the code is judged: it was read from bits that are not there)
        if (rs < 0) return JPEG_ST_BAD_CODE;
        const int r = rs >> 4;
        s = rs & 15;
        if (s) {
            k += r;
            if (k > 63) return JPEG_ST_RUN;
            const int v = jpeg_dec_extend(br.peek(s), s);
            br.drop(s);
            if (STORE) blk[JPEG_ZZ[k]] = (int16_t)v;  // k <= 63
        } else if (r == 15) {
            k += 15;
            if (k > 63) return JPEG_ST_RUN;
        } else {
            if (br.starved()) return JPEG_ST_EXHAUSTED;
            break;
        }
        if (br.starved()) return JPEG_ST_EXHAUSTED;
    }
    return JPEG_ST_OK;
}

struct JpegExtent {
    long long max_byte, max_coef;  // one past the last stream byte read, one past the last coefficient written
};
// The component of block j of an MCU.
HH_HD int jpeg_dec_block_comp(const JpegStreamInfo &I, int j) { return j < I.hs * I.vs ? 0 : j - I.hs * I.vs + 1; }

// The last MCU of [first, first + count) that lies inside the rectangle, or -1: where a lane's walk ends, and whether it has one.
// With the whole grid as the rectangle no clause applies (ly <= mrows - 1 = my1, lx >= 0 = mx0, ly >= 0 = my0, lx <= mcols - 1 = mx1):
// the result is the segment's last MCU.
HH_HD int jpeg_win_last(const JpegStreamInfo &I, const JpegWinRect &R, int first, int count)
{
    const int last = first + count - 1;
    int ly = last / I.mcols, lx = last % I.mcols;
    if (ly > R.my1) ly = R.my1, lx = I.mcols - 1;
    if (lx < R.mx0) ly -= 1, lx = I.mcols - 1;  // (this row's part lies left of the rectangle: the row before, whole)
    if (ly < R.my0) return -1;
    const int cand = ly * I.mcols + (lx < R.mx1 ? lx : R.mx1);  // the largest MCU of the rectangle <= last
    return cand >= first ? cand : -1;
}

// One segment: walked from its first MCU to its last MCU inside the rectangle; coefficients are stored for the MCUs inside (coefs: the
// rectangle's [rows * cols * bpm][64]), the others are walked without storing.  Every stream byte read lies in [scan_offset,
// min(byte_end, length)) of the stream (a window's: the shipped slice); every coefficient written in a block of the rectangle, after
// the segment's MCU range was cut to the image's grid.  The RSTm check applies only to a walk that reached the segment's end.
// With the whole grid as the rectangle (jpeg_full_rect) `stop` is the segment's last MCU (see jpeg_win_last) and `inside` is always
// true, since 0 <= mx < mcols and 0 <= my < mrows for every MCU of the grid: every MCU is stored at (first_mcu + m) * bpm, the walk
// always reaches the segment's end, and ext->max_coef is one past the last MCU begun.
HH_HD int jpeg_dec_segment(const unsigned char *stream, int length, const JpegStreamInfo &I, const JpegHuff *huff, const JpegSegment &sg,
                             const JpegWinRect &R, int16_t *coefs, JpegWinCounts *counts, JpegExtent *ext)
{
    const int nmcu = I.mcols * I.mrows;
    const long long lim = I.scan_end < length ? I.scan_end : length;
    const int end = (sg.byte_end >> 1) < lim ? (sg.byte_end >> 1) : (int)lim;
    if (sg.first_mcu < 0 || sg.first_mcu >= nmcu || sg.mcu_count < 1 || sg.mcu_count > nmcu - sg.first_mcu || sg.byte_offset < I.scan_offset ||
        sg.byte_offset > end || (sg.bit_offset & ~7))
        return JPEG_ST_SEGMENT;
    const int stop = jpeg_win_last(I, R, sg.first_mcu, sg.mcu_count);
    if (stop < 0) return JPEG_ST_OK;  // (no MCU of the rectangle: the host does not select such a segment)
    JpegBits br;
    br.init(stream, sg.byte_offset, end);
    br.refill();
    br.drop(sg.bit_offset);
    int pred[3] = {sg.pred[0], sg.pred[1], sg.pred[2]};
    int status = JPEG_ST_OK;
    int my = sg.first_mcu / I.mcols, mx = sg.first_mcu % I.mcols;
    long long stored = 0, top = 0;
    int m = sg.first_mcu;
#pragma unroll 1
    for (; m <= stop && !status; ++m) {
        const bool inside = mx >= R.mx0 && mx <= R.mx1 && my >= R.my0 && my <= R.my1;
        const size_t at = ((size_t)(my - R.my0) * R.cols + (size_t)(mx - R.mx0)) * I.bpm;  // (read only when inside)
#pragma unroll 1
        for (int j = 0; j < I.bpm && !status; ++j) {
            const int c = jpeg_dec_block_comp(I, j);
            const JpegHuff &dc = huff[I.dc[c] & 3], &ac = huff[4 + (I.ac[c] & 3)];
            status = inside ? jpeg_dec_block<true>(br, dc, ac, pred[c], coefs + (at + j) * 64) : jpeg_dec_block<false>(br, dc, ac, pred[c], nullptr);
        }
        if (inside) {
            ++stored;
            if ((long long)(at + I.bpm) * 64 > top) top = (long long)(at + I.bpm) * 64;
        }
        if (++mx == I.mcols) mx = 0, ++my;
    }
    // data where the RSTm should stand
    if (!status && stop == sg.first_mcu + sg.mcu_count - 1 && (sg.byte_end & 1) && (br.real() >= 8 || br.pos < end)) status = JPEG_ST_RESTART;
    if (counts) counts->segments_walked += 1, counts->mcus_walked += m - sg.first_mcu, counts->mcus_stored += stored;
    if (ext) {
        if (br.pos > ext->max_byte) ext->max_byte = br.pos;
        if (top > ext->max_coef) ext->max_coef = top;
    }
    return status;
}

// ---------------------------------------------------------------------------------------------------------------- the IDCT
// libjpeg's jidctint ("islow"): CONST_BITS 13, PASS1_BITS 2.  v[8] holds a column of dequantised coefficients (pass 1: descale by 11)
// or a row of pass-1 results (pass 2: descale by 18); the results replace them.
template <int SHIFT>
HH_HD void jpeg_idct_1d(int32_t v[8])
{
    // (modular uint32 arithmetic: what a stream within the rule gives fits int32 and is the same; a malformed one wraps instead of
    // overflowing a signed type)
    typedef uint32_t U;
    U z2 = (U)v[2], z3 = (U)v[6];
    U z1 = (z2 + z3) * 4433u;
    U tmp2 = z1 + z3 * (U)-15137;
    U tmp3 = z1 + z2 * 6270u;
    z2 = (U)v[0], z3 = (U)v[4];
    U tmp0 = (z2 + z3) << 13;
    U tmp1 = (z2 - z3) << 13;
    const U tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = (U)v[7], tmp1 = (U)v[5], tmp2 = (U)v[3], tmp3 = (U)v[1];
    z1 = tmp0 + tmp3, z2 = tmp1 + tmp2, z3 = tmp0 + tmp2;
    U z4 = tmp1 + tmp3;
    const U z5 = (z3 + z4) * 9633u;
    tmp0 *= 2446u, tmp1 *= 16819u, tmp2 *= 25172u, tmp3 *= 12299u;
    z1 *= (U)-7373, z2 *= (U)-20995, z3 *= (U)-16069, z4 *= (U)-3196;
    z3 += z5, z4 += z5;
    tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
    const U half = 1u << (SHIFT - 1);
    v[0] = (int32_t)(tmp10 + tmp3 + half) >> SHIFT, v[7] = (int32_t)(tmp10 - tmp3 + half) >> SHIFT;
    v[1] = (int32_t)(tmp11 + tmp2 + half) >> SHIFT, v[6] = (int32_t)(tmp11 - tmp2 + half) >> SHIFT;
    v[2] = (int32_t)(tmp12 + tmp1 + half) >> SHIFT, v[5] = (int32_t)(tmp12 - tmp1 + half) >> SHIFT;
    v[3] = (int32_t)(tmp13 + tmp0 + half) >> SHIFT, v[4] = (int32_t)(tmp13 - tmp0 + half) >> SHIFT;
}
// The sample of a pass-2 result.
HH_HD int jpeg_idct_sample(int32_t x)
{
    return x < -128 ? 0 : x > 127 ? 255 : x + 128;
}
// Column u of a block: dequantise (int16 coefficient x divisor, natural order) and pass 1, into ws (row stride 8).
HH_HD void jpeg_idct_col(const int16_t *coef, const uint16_t *q, int u, int32_t *ws)
{
    int32_t v[8];
#pragma unroll
    for (int y = 0; y < 8; ++y) v[y] = (int32_t)((uint32_t)(int32_t)coef[y * 8 + u] * (uint32_t)q[y * 8 + u]);
    jpeg_idct_1d<11>(v);
#pragma unroll
    for (int y = 0; y < 8; ++y) ws[y * 8 + u] = v[y];
}
struct alignas(8) JpegRow8 {
    unsigned char v[8];
};
HH_HD JpegRow8 jpeg_idct_row(const int32_t *ws_row)
{
    int32_t v[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) v[x] = ws_row[x];
    jpeg_idct_1d<18>(v);
    JpegRow8 r;
#pragma unroll
    for (int x = 0; x < 8; ++x) r.v[x] = (unsigned char)jpeg_idct_sample(v[x]);
    return r;
}
// Where block `blk` of the rectangle lies: its component, and its first sample in that component's plane (g = jpeg_dec_geom(I, R)).
HH_HD void jpeg_dec_block_place(const JpegStreamInfo &I, const JpegWinRect &R, const JpegDecGeom &g, int blk, int &c, long long &at)
{
    const int mcu = blk / I.bpm, j = blk % I.bpm;
    const int ry = mcu / R.cols, rx = mcu % R.cols;
    c = jpeg_dec_block_comp(I, j);
    const int hs = c == 0 ? I.hs : 1, vs = c == 0 ? I.vs : 1;
    const int by = c == 0 ? j / I.hs : 0, bx = c == 0 ? j % I.hs : 0;
    at = g.plane_at[c] + (long long)((ry * vs + by) * 8) * g.pw[c] + (rx * hs + bx) * 8;
}

// ---------------------------------------------------------------------------------------------------------------- upsampling, colour
// The chroma sample of output pixel (y, x) of the image (libjpeg's fancy filters; plain replication when cw <= 2) from a plane that
// starts at row oy, column ox of the component (0, 0: the whole component): the taps and the edges go by the component's true size
// cw x ch, only the addresses are relative to (oy, ox).
HH_HD int jpeg_dec_chroma(const unsigned char *plane, int pitch, int oy, int ox, int cw, int ch, int hs, int vs, int y, int x)
{
    if (hs == 1) return plane[(size_t)(y - oy) * pitch + (x - ox)];
    const int c = x >> 1;
    if (cw <= 2) return plane[(size_t)((vs == 2 ? y >> 1 : y) - oy) * pitch + (c - ox)];
    if (vs == 1) {
        const unsigned char *row = plane + (size_t)(y - oy) * pitch;
        const int v = row[c - ox];
        if (x & 1) return c == cw - 1 ? v : (3 * v + row[c + 1 - ox] + 2) >> 2;
        return c == 0 ? v : (3 * v + row[c - 1 - ox] + 1) >> 2;
    }
    const int r = y >> 1;
    int far = (y & 1) ? r + 1 : r - 1;
    far = far < 0 ? 0 : far > ch - 1 ? ch - 1 : far;
    const unsigned char *near_row = plane + (size_t)(r - oy) * pitch, *far_row = plane + (size_t)(far - oy) * pitch;
    const int s = 3 * near_row[c - ox] + far_row[c - ox];
    if (x & 1) {
        const int cn = (c == cw - 1 ? c : c + 1) - ox;
        return (3 * s + 3 * near_row[cn] + far_row[cn] + 7) >> 4;
    }
    const int cp = (c == 0 ? c : c - 1) - ox;
    return (3 * s + 3 * near_row[cp] + far_row[cp] + 8) >> 4;
}
HH_HD int jpeg_dec_clamp(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
// Pixel (y, x) of the IMAGE from the rectangle's planes -> dst[0..2].
HH_HD void jpeg_dec_pixel(const unsigned char *ws, const JpegStreamInfo &I, const JpegWinRect &R, const JpegDecGeom &g, int y, int x, bool bgr,
                            unsigned char *dst)
{
    const int Y = ws[g.plane_at[0] + (size_t)(y - R.my0 * I.vs * 8) * g.pw[0] + (x - R.mx0 * I.hs * 8)];
    if (I.ncomp == 1) {
        dst[0] = dst[1] = dst[2] = (unsigned char)Y;
        return;
    }
    const int cy = R.my0 * 8, cx = R.mx0 * 8;  // the chroma planes' origin: one block per MCU, whatever the sampling
    const int cb = jpeg_dec_chroma(ws + g.plane_at[1], g.pw[1], cy, cx, g.cw[1], g.ch[1], I.hs, I.vs, y, x) - 128;
    const int cr = jpeg_dec_chroma(ws + g.plane_at[2], g.pw[2], cy, cx, g.cw[2], g.ch[2], I.hs, I.vs, y, x) - 128;
    const int Rr = jpeg_dec_clamp(Y + ((91881 * cr + 32768) >> 16));
    const int B = jpeg_dec_clamp(Y + ((116130 * cb + 32768) >> 16));
    const int G = jpeg_dec_clamp(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    dst[bgr ? 2 : 0] = (unsigned char)Rr, dst[1] = (unsigned char)G, dst[bgr ? 0 : 2] = (unsigned char)B;
}

// ---------------------------------------------------------------------------------------------------------------- host only
// BITS / HUFFVAL -> the lookup form; false for counts that are no prefix code.
inline bool jpeg_dec_build_huff(const unsigned char *bits, const unsigned char *vals, int nvals, JpegHuff *H)
{
    memset(H, 0, sizeof(*H));
    for (int l = 0; l < 18; ++l) H->maxcode[l] = -1;
    int code = 0, p = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = bits[l - 1];
        if (p + n > nvals || code + n > (1 << l)) return false;
        if (n) {
            H->valoff[l] = p - code;
            H->maxcode[l] = code + n - 1;
            for (int i = 0; i < n; ++i) {
                H->vals[p + i] = vals[p + i];
                if (l <= 8)
                    for (int f = 0; f < (1 << (8 - l)); ++f) H->look[((code + i) << (8 - l)) + f] = (uint16_t)(l << 8 | vals[p + i]);
            }
            p += n, code += n;
        }
        code <<= 1;
    }
    return true;
}

// The marker walk: every refusal of the rule, by name; nullptr when the stream is accepted.  T may be null.
inline const char *jpeg_dec_parse(const unsigned char *b, long long len, JpegStreamInfo *I, JpegDecTables *T)
{
    static const char *trunc = "truncated header";
    JpegDecTables local;
    if (!T) T = &local;
    memset(I, 0, sizeof(*I));
    memset(T, 0, sizeof(*T));
    I->adobe_transform = -1;
    if (len > INT32_MAX) return "the stream is longer than int32 offsets allow";
    if (len < 2 || b[0] != 0xff || b[1] != 0xd8) return "not a JPEG stream (no SOI)";
    bool have_q[4] = {false, false, false, false}, have_h[8] = {false, false, false, false, false, false, false, false};
    bool have_sof = false;
    int comp_id[3] = {0, 0, 0};
    long long at = 2;
    for (;;) {
        if (at + 2 > len) return trunc;
        if (b[at] != 0xff) return "a marker is expected in the header";
        while (at + 1 < len && b[at + 1] == 0xff) ++at;  // fill bytes
        if (at + 2 > len) return trunc;
        const int m = b[at + 1];
        at += 2;
        if (m == 0xd9) return "no scan before EOI";
        if (m == 0xd8 || (m >= 0xd0 && m <= 0xd7) || m == 0x01) continue;  // (no length)
        if (at + 2 > len) return trunc;
        const int L = b[at] << 8 | b[at + 1];
        if (L < 2 || at + L > len) return trunc;
        const unsigned char *s = b + at + 2;
        const int n = L - 2;
        at += L;
        if (m == 0xcc) return "arithmetic coding is not supported";
        if (m == 0xc4) {
            int k = 0;
            while (k < n) {
                if (k + 17 > n) return trunc;
                const int tc = s[k] >> 4, th = s[k] & 15;
                if (tc > 1 || th > 3) return "a Huffman table id outside 0..3";
                int count = 0;
                for (int i = 0; i < 16; ++i) count += s[k + 1 + i];
                if (count > 256 || k + 17 + count > n) return count > 256 ? "a Huffman table with more than 256 codes" : trunc;
                if (!jpeg_dec_build_huff(s + k + 1, s + k + 17, count, &T->huff[tc * 4 + th])) return "a Huffman table that is no prefix code";
                have_h[tc * 4 + th] = true;
                k += 17 + count;
            }
        } else if (m == 0xdb) {
            int k = 0;
            while (k < n) {
                const int pq = s[k] >> 4, tq = s[k] & 15;
                if (pq > 1 || tq > 3) return "a quantiser table id outside 0..3";
                if (k + 1 + 64 * (pq + 1) > n) return trunc;
                for (int i = 0; i < 64; ++i) T->q[tq][JPEG_ZZ[i]] = pq ? (uint16_t)(s[k + 1 + 2 * i] << 8 | s[k + 2 + 2 * i]) : s[k + 1 + i];
                have_q[tq] = true;
                k += 1 + 64 * (pq + 1);
            }
        } else if (m == 0xdd) {
            if (n < 2) return trunc;
            I->restart_interval = s[0] << 8 | s[1];
        } else if (m == 0xee) {
            if (n >= 12 && !memcmp(s, "Adobe", 5)) I->adobe_transform = s[11];
        } else if (m >= 0xc0 && m <= 0xcf) {  // (c4 and cc went above) a frame header
            if (n < 6) return trunc;
            if (s[0] == 12) return "12-bit precision is not supported";
            if (m == 0xc2) return "progressive streams (SOF2) are not supported";
            if (m >= 0xc9) return "arithmetic coding is not supported";
            if (m != 0xc0) return "only baseline streams (SOF0) are supported";
            if (s[0] != 8) return "only 8-bit precision is supported";
            if (have_sof) return "more than one frame header";
            I->h = s[1] << 8 | s[2], I->w = s[3] << 8 | s[4], I->ncomp = s[5];
            if (I->ncomp == 4) return "4 components are not supported";
            if (I->ncomp != 1 && I->ncomp != 3) return "only 1 or 3 components are supported";
            if (n < 6 + 3 * I->ncomp) return trunc;
            if (I->h == 0 || I->w == 0) return "a dimension of 0";
            for (int c = 0; c < I->ncomp; ++c) {
                comp_id[c] = s[6 + 3 * c];
                const int hv = s[7 + 3 * c];
                I->qt[c] = s[8 + 3 * c];
                if (I->qt[c] > 3) return "a quantiser table id outside 0..3";
                if (I->ncomp == 1) {
                    I->hs = I->vs = 1;  // (a lone component is coded block by block, whatever its factors)
                } else if (c == 0) {
                    if (hv != 0x11 && hv != 0x21 && hv != 0x22) return "unsupported sampling (only 4:4:4, 4:2:2 h2v1 and 4:2:0)";
                    I->hs = hv >> 4, I->vs = hv & 15;
                } else if (hv != 0x11) {
                    return "unsupported sampling (only 4:4:4, 4:2:2 h2v1 and 4:2:0)";
                }
            }
            I->sampling = I->ncomp == 1 ? 400 : I->hs == 1 ? 444 : I->vs == 1 ? 422 : 420;
            I->bpm = I->ncomp == 1 ? 1 : I->hs * I->vs + 2;
            I->mcols = (I->w + 8 * I->hs - 1) / (8 * I->hs);
            I->mrows = (I->h + 8 * I->vs - 1) / (8 * I->vs);
            if ((long long)I->mcols * I->hs * 8 * 3 * ((long long)I->mrows * I->vs * 8) > INT32_MAX || (long long)I->mcols * I->mrows * I->bpm * 128 > INT32_MAX)
                return "dimensions beyond what int32 offsets allow";
            have_sof = true;
        } else if (m == 0xda) {
            if (!have_sof) return "a scan before the frame header";
            if (n < 1) return trunc;
            if (s[0] != I->ncomp) return "more than one scan (the scan does not hold all components)";
            if (n < 4 + 2 * I->ncomp) return trunc;
            for (int c = 0; c < I->ncomp; ++c) {
                if (s[1 + 2 * c] != comp_id[c]) return "the scan's components are not the frame's";
                I->dc[c] = s[2 + 2 * c] >> 4, I->ac[c] = s[2 + 2 * c] & 15;
                if (I->dc[c] > 3 || I->ac[c] > 3) return "a Huffman table id outside 0..3";
                if (!have_h[I->dc[c]] || !have_h[4 + I->ac[c]]) return "missing tables (Huffman)";
                if (!have_q[I->qt[c]]) return "missing tables (quantiser)";
            }
            const unsigned char *t = s + 1 + 2 * I->ncomp;
            if (t[0] != 0 || t[1] != 63 || t[2] != 0) return "progressive scan parameters in a baseline stream";
            if (I->ncomp == 3 && I->adobe_transform == 0) return "an Adobe marker with transform 0 (RGB) is not supported";
            break;
        }
        // everything else (APPn, COM, ...) is skipped
    }
    I->scan_offset = at;
    // the scan ends at the first marker that is neither a stuffed FF nor an RSTm; it must be the EOI
    long long e = at;
    int rst = 0;
    for (;;) {
        const unsigned char *f = e < len ? (const unsigned char *)memchr(b + e, 0xff, (size_t)(len - e)) : nullptr;
        if (!f || f + 1 >= b + len) {
            e = len;
            break;
        }
        e = f - b;
        const int m = b[e + 1];
        if (m == 0 || m == 0xff) {
            e += m == 0 ? 2 : 1;
        } else if (m >= 0xd0 && m <= 0xd7) {
            ++rst;
            e += 2;
        } else if (m == 0xd9) {
            break;
        } else {
            return "more than one scan (a marker other than RSTm or EOI follows the scan's data)";
        }
    }
    I->scan_end = e;
    if (I->restart_interval) {
        I->nseg_restart = (I->mcols * I->mrows + I->restart_interval - 1) / I->restart_interval;
        if (rst != I->nseg_restart - 1) return "the restart markers do not match the restart interval";
    } else if (rst) {
        return "restart markers without a restart interval";
    }
    return nullptr;
}

// With DRI: the segments from a byte scan for the RSTm markers (no Huffman work).  seg: nseg_restart entries.
inline const char *jpeg_dec_restart_segments(const unsigned char *b, const JpegStreamInfo &I, JpegSegment *seg)
{
    const int nmcu = I.mcols * I.mrows;
    long long at = I.scan_offset;
    for (int i = 0; i < I.nseg_restart; ++i) {
        long long e = at;
        const bool last = i + 1 == I.nseg_restart;
        if (!last) {
            for (;;) {  // (the parse counted nseg_restart - 1 markers inside [scan_offset, scan_end))
                const unsigned char *f = e < I.scan_end ? (const unsigned char *)memchr(b + e, 0xff, (size_t)(I.scan_end - e)) : nullptr;
                if (!f || f + 1 >= b + I.scan_end) return "the restart markers do not match the restart interval";
                e = f - b;
                if (b[e + 1] >= 0xd0 && b[e + 1] <= 0xd7) break;
                e += b[e + 1] == 0 ? 2 : 1;
            }
            if (b[e + 1] != 0xd0 + (i & 7)) return "a restart marker out of sequence";
        } else {
            e = I.scan_end;
        }
        seg[i].first_mcu = i * I.restart_interval;
        seg[i].mcu_count = nmcu - seg[i].first_mcu < I.restart_interval ? nmcu - seg[i].first_mcu : I.restart_interval;
        seg[i].byte_offset = (int32_t)at, seg[i].bit_offset = 0;
        seg[i].pred[0] = seg[i].pred[1] = seg[i].pred[2] = 0;
        seg[i].byte_end = (int32_t)(e << 1 | (last ? 0 : 1));
        at = e + 2;
    }
    return nullptr;
}

// How many entries jpeg_dec_index writes at `mps` MCUs per segment.
inline int jpeg_dec_index_count(const JpegStreamInfo &I, int mps)
{
    const int nmcu = I.mcols * I.mrows;
    if (!I.restart_interval) return (nmcu + mps - 1) / mps;
    const int full = nmcu / I.restart_interval, rest = nmcu % I.restart_interval;
    return full * ((I.restart_interval + mps - 1) / mps) + (rest + mps - 1) / mps;
}

// One Huffman pass over the scan (symbol lengths and DC sums only): an entry every `mps` MCUs, counted anew from every restart.  The
// pass validates the stream: *status receives the code that stopped it (the refusal is then "the scan cannot be walked").
inline const char *jpeg_dec_index(const unsigned char *b, long long len, const JpegStreamInfo &I, const JpegDecTables &T, int mps, JpegSegment *seg,
                                  int capacity, int *count, int *status)
{
    const int nmcu = I.mcols * I.mrows, ri = I.restart_interval ? I.restart_interval : nmcu;
    *count = 0, *status = 0;
    if (mps < 1) return "mcus_per_segment must be at least 1";
    if (jpeg_dec_index_count(I, mps) > capacity) return "capacity below the number of segments";
    long long at = I.scan_offset;
    int n = 0;
    for (int first = 0, iv = 0; first < nmcu; first += ri, ++iv) {
        const int cnt = nmcu - first < ri ? nmcu - first : ri;
        const bool last = first + ri >= nmcu;
        // this interval's bytes end at its RSTm, or at scan_end
        long long e = I.scan_end;
        if (!last) {
            e = at;
            for (;;) {
                const unsigned char *f = e < I.scan_end ? (const unsigned char *)memchr(b + e, 0xff, (size_t)(I.scan_end - e)) : nullptr;
                if (!f || f + 1 >= b + I.scan_end) return "the restart markers do not match the restart interval";
                e = f - b;
                if (b[e + 1] >= 0xd0 && b[e + 1] <= 0xd7) break;
                e += b[e + 1] == 0 ? 2 : 1;
            }
            if (b[e + 1] != 0xd0 + (iv & 7)) return "a restart marker out of sequence";
        }
        JpegSegment walk;
        walk.first_mcu = first, walk.byte_offset = (int32_t)at, walk.bit_offset = 0;
        walk.pred[0] = walk.pred[1] = walk.pred[2] = 0;
        for (int m = 0; m < cnt; m += mps) {
            walk.mcu_count = cnt - m < mps ? cnt - m : mps;
            const bool tail = m + mps >= cnt;
            walk.byte_end = (int32_t)(e << 1 | (tail && !last ? 1 : 0));
            seg[n++] = walk;
            // walk these MCUs; where the next entry starts: back from the reader's position over the unread bits
            JpegBits br;
            {
                const long long lim = I.scan_end < len ? I.scan_end : len;
                br.init(b, walk.byte_offset, (int)(e < lim ? e : lim));
                br.refill();
                br.drop(walk.bit_offset);
            }
            int st = 0;
            for (int k = 0; k < walk.mcu_count && !st; ++k)
                for (int j = 0; j < I.bpm && !st; ++j) {
                    const int c = jpeg_dec_block_comp(I, j);
                    st = jpeg_dec_block<false>(br, T.huff[I.dc[c]], T.huff[4 + I.ac[c]], walk.pred[c], nullptr);
                }
            if (!st && tail && !last && (br.real() >= 8 || br.pos < br.end)) st = JPEG_ST_RESTART;
            if (st) {
                *status = st;
                return "the scan cannot be walked";
            }
            if (!tail) {
                int p, bit;
                jpeg_bits_where(br, walk.byte_offset, p, bit);
                walk.byte_offset = p, walk.bit_offset = bit;
                walk.first_mcu += walk.mcu_count;
            }
        }
        at = e + 2;
    }
    *count = n;
    return nullptr;
}

// Steps b to d of a window on the host: ws (jpeg_dec_geom(I, jpeg_win_rect(I, W)).ws_bytes, 16-byte aligned) holds the rectangle's
// coefficients, the planes are formed there, dst receives [height,width,3].
inline void jpeg_dec_window_pixels_host(unsigned char *ws, const JpegStreamInfo &I, const JpegDecTables &T, const JpegWindow &W, bool bgr,
                                        unsigned char *dst, long long pitch)
{
    const JpegWinRect R = jpeg_win_rect(I, W);
    const JpegDecGeom g = jpeg_dec_geom(I, R);
    for (int blk = 0; blk < g.nblk; ++blk) {
        int c;
        long long at;
        jpeg_dec_block_place(I, R, g, blk, c, at);
        int32_t tmp[64];
        const int16_t *coef = reinterpret_cast<const int16_t *>(ws) + (size_t)blk * 64;
        for (int u = 0; u < 8; ++u) jpeg_idct_col(coef, T.q[I.qt[c] & 3], u, tmp);
        for (int y = 0; y < 8; ++y) {
            const JpegRow8 r = jpeg_idct_row(tmp + y * 8);
            memcpy(ws + at + (size_t)y * g.pw[c], r.v, 8);
        }
    }
    for (int y = 0; y < W.height; ++y)
        for (int x = 0; x < W.width; ++x) jpeg_dec_pixel(ws, I, R, g, W.top + y, W.left + x, bgr, dst + (size_t)y * pitch + (size_t)x * 3);
}

// ---------------------------------------------------------------------------------------------------------------- host only, window
inline const char *jpeg_win_check(const JpegStreamInfo &I, const JpegWindow &W)
{
    if (W.height < 1 || W.width < 1) return "the window is empty";
    if (W.top < 0 || W.left < 0 || W.top > I.h - W.height || W.left > I.w - W.width) return "the window leaves the image";
    return nullptr;
}

// The segments of a window decode: those with at least one MCU in the rectangle (with a fine index not a contiguous set), and the
// slice [slice[0], slice[1]) of the stream they need: from the first selected segment's byte_offset to the last one's end.
inline const char *jpeg_win_select(const JpegStreamInfo &I, const JpegWinRect &R, const JpegSegment *entries, int nseg, int *nsel, long long slice[2])
{
    const int nmcu = I.mcols * I.mrows;
    long long lo = I.scan_end, hi = I.scan_offset;
    int n = 0;
    for (int s = 0; s < nseg; ++s) {
        const JpegSegment &e = entries[s];
        if (e.first_mcu < 0 || e.first_mcu >= nmcu || e.mcu_count < 1 || e.mcu_count > nmcu - e.first_mcu) return "a segment outside the MCU grid";
        if (jpeg_win_last(I, R, e.first_mcu, e.mcu_count) < 0) continue;
        const long long end = (e.byte_end >> 1) < I.scan_end ? (e.byte_end >> 1) : I.scan_end;
        if (e.byte_offset < I.scan_offset || e.byte_offset > end) return "a selected segment's bytes lie outside the scan";
        lo = e.byte_offset < lo ? e.byte_offset : lo, hi = end > hi ? end : hi;
        ++n;
    }
    if (!n) return "no segment holds an MCU of the window's rectangle";
    if (hi <= lo) return "the selected segments hold no bytes";
    *nsel = n, slice[0] = lo, slice[1] = hi;
    return nullptr;
}

// The table block of a window decode (jpeg_dec_tables_bytes(nsel) at `out`): the info, the tables and the selected segments, with the
// segments' byte offsets and the info's scan_offset / scan_end rebased to the slice, so that the bit reader knows one origin only.
inline void jpeg_win_tables(const JpegStreamInfo &I, const JpegDecTables &T, const JpegWinRect &R, const JpegSegment *entries, int nseg,
                            const long long slice[2], unsigned char *out)
{
    JpegStreamInfo J = I;
    J.scan_offset = 0, J.scan_end = slice[1] - slice[0];
    memcpy(out, &J, sizeof(J));
    memcpy(out + JPEG_DEC_TABLES_AT, &T, sizeof(T));
    unsigned char *at = out + JPEG_DEC_SEGS_AT;
    for (int s = 0; s < nseg; ++s) {
        JpegSegment e = entries[s];
        if (jpeg_win_last(I, R, e.first_mcu, e.mcu_count) < 0) continue;
        const long long end = (e.byte_end >> 1) < I.scan_end ? (e.byte_end >> 1) : I.scan_end;
        e.byte_offset -= (int32_t)slice[0];
        e.byte_end = (int32_t)((end - slice[0]) << 1 | (e.byte_end & 1));
        memcpy(at, &e, sizeof(e));
        at += sizeof(e);
    }
}

// A decode on the host, from what the device receives: the stream (a window's: the slice), its table block (hh_jpeg_decode_tables, or
// jpeg_win_tables), a workspace of jpeg_dec_geom().ws_bytes (16-byte aligned) and the height x pitch destination -> the largest status
// of the walked part.
inline int jpeg_dec_window_host(const unsigned char *slice, int slice_len, const unsigned char *block, int nsel, const JpegWindow &W, bool bgr,
                                unsigned char *ws, unsigned char *dst, long long pitch, JpegWinCounts *counts, JpegExtent *ext)
{
    JpegStreamInfo I;
    memcpy(&I, block, sizeof(I));
    const JpegDecTables *T = reinterpret_cast<const JpegDecTables *>(block + JPEG_DEC_TABLES_AT);
    const JpegWinRect R = jpeg_win_rect(I, W);
    int status = 0;
    for (int s = 0; s < nsel; ++s) {
        JpegSegment sg;
        memcpy(&sg, block + JPEG_DEC_SEGS_AT + (size_t)s * sizeof(sg), sizeof(sg));
        const int st = jpeg_dec_segment(slice, slice_len, I, T->huff, sg, R, reinterpret_cast<int16_t *>(ws), counts, ext);
        status = st > status ? st : status;
    }
    jpeg_dec_window_pixels_host(ws, I, *T, W, bgr, dst, pitch);
    if (counts) {
        counts->blocks_transformed += jpeg_dec_geom(I, R).nblk, counts->pixels_written += (long long)W.height * W.width;
        counts->stream_bytes += slice_len;
    }
    return status;
}

// ---------------------------------------------------------------------------------------------------------------- the device index
// The index of a restart-less stream without a sequential Huffman pass (the rule: hh_jpeg_index_device_batch in include/hhrnet.h).  The
// scan's bytes [S, E) are cut into subsequences of B bytes, one lane each.  What lanes hand to each other is a state at a block
// boundary, packed into one word: the canonical byte position (jpeg_bits_where) << 6 | the bit in that byte << 3 | the block's index
// in its MCU.  jpeg_idx_walk is one lane's walk, written once for the host and the device; how the lanes of a round wait for each
// other differs (loops in jpeg_idx_sync_host below, barriers in jpeg_index.hip).
enum { JPEG_IDX_LANES = 1024, JPEG_IDX_SUBSEQ = 32, JPEG_IDX_SUBSEQ_MIN = 4, JPEG_IDX_MPS = 2 };
enum { JPEG_IDX_PENDING = 1 };  // info.reserved[1] of a table block whose entries the device is to fill (hh_jpeg_index_tables)
typedef unsigned long long JpegIdxKey;
static constexpr JpegIdxKey JPEG_IDX_NONE = ~0ull;  // no state: the walk met an error or ran out of blocks
HH_HD JpegIdxKey jpeg_idx_key(int p, int bit, int j) { return (JpegIdxKey)(uint32_t)p << 6 | (JpegIdxKey)(uint32_t)bit << 3 | (JpegIdxKey)(uint32_t)j; }

struct JpegIdxLane {
    JpegIdxKey exit;  // the first boundary at or past `limit`, or JPEG_IDX_NONE
    uint32_t count;   // whole blocks decoded
    uint32_t dc[3];   // the sums of their DC differences per component (uint32 wrap, as jpeg_dec_block adds them)
    int status;       // what stopped the walk (reported by the last walk only)
};

// The scan's bytes as the index walks them, and how many subsequences of B bytes they make (at least one: lane 0 always walks).
HH_HD int jpeg_idx_scan_end(const JpegStreamInfo &I, long long length) { return (int)(I.scan_end < length ? I.scan_end : length); }
HH_HD long long jpeg_idx_subsequences(const JpegStreamInfo &I, long long length, int B)
{
    const long long bytes = (long long)jpeg_idx_scan_end(I, length) - I.scan_offset;
    return bytes > 0 ? (bytes + B - 1) / B : 1;
}
// Where lane k >= 1 begins before it knows better: the first data bit of its subsequence (a 00 behind an FF belongs to that FF), at a
// block boundary, block 0 of an MCU.  S + k B < E, and S + k B - 1 >= S: both bytes lie in the scan.
HH_HD JpegIdxKey jpeg_idx_guess(const unsigned char *b, const JpegStreamInfo &I, long long k, int B)
{
    int p = (int)(I.scan_offset + k * B);
    if (b[p] == 0 && b[p - 1] == 0xff) p += 1;
    return jpeg_idx_key(p, 0, 0);
}
// One past the last byte of subsequence k: the start of the next one, or no limit for the last.
HH_HD int jpeg_idx_limit(const JpegStreamInfo &I, long long nsub, long long k, int B) { return k + 1 < nsub ? (int)(I.scan_offset + (k + 1) * B) : INT32_MAX; }

// One lane: whole blocks from the state `from` up to the first boundary whose canonical byte is at or past `limit`, but no further
// than block `total` of the image, the walk's first block being block g0 (a speculative lane does not know its g0: 0, which makes
// `total` a plain bound on its loop).  EMIT (the last walk, from a verified state, with the true g0 and the DC sums `dcpre` of all
// blocks before g0): the entry of every boundary in front of a block g with g % (mps bpm) == 0 is written, if it lies below nseg.
// Every byte read lies in [from's byte, E) of the stream; every entry written below seg + nseg; the loop ends after at most
// total - g0 blocks.
template <bool EMIT>
#if defined(__HIPCC__)
__host__ __device__
#endif
inline void jpeg_idx_walk(const unsigned char *b, int E, const JpegStreamInfo &I, const JpegHuff *huff, JpegIdxKey from, int limit, long long g0, long long total,
                          int mps, const uint32_t *dcpre, JpegSegment *seg, int nseg, JpegIdxLane &out)
{
    const int start = (int)(from >> 6);
    int cp = start, cb = (int)(from >> 3) & 7, j = (int)from & 7;
    out.exit = JPEG_IDX_NONE, out.count = 0, out.dc[0] = out.dc[1] = out.dc[2] = 0, out.status = JPEG_ST_OK;
    if (j >= I.bpm) return;  // (no state a walk hands on)
    JpegBits br;
    br.init(b, start, E);
    br.refill();
    br.drop(cb);
    int pred[3] = {0, 0, 0};
    const long long period = (long long)mps * I.bpm, nmcu = (long long)I.mcols * I.mrows;
    long long phase = EMIT ? g0 % period : 0, entry = EMIT ? g0 / period : 0;
    bool known = true;  // (cp, cb) is the position of the boundary in front of the next block
#pragma unroll 1
    for (long long g = g0;; ++g) {
        const bool emit = EMIT && phase == 0 && g < total;
        if (!known && (emit || br.pos >= limit)) jpeg_bits_where(br, start, cp, cb), known = true;  // (the canonical byte is never behind br.pos)
        if (known && cp >= limit) {
            out.exit = jpeg_idx_key(cp, cb, j);
            return;
        }
        if (g >= total) return;
        if (emit && entry < nseg) {
            JpegSegment e;
            e.first_mcu = (int32_t)(entry * mps);
            e.mcu_count = (int32_t)(nmcu - entry * mps < mps ? nmcu - entry * mps : mps);
            e.byte_offset = cp, e.bit_offset = cb;
            for (int c = 0; c < 3; ++c) e.pred[c] = (int32_t)(dcpre[c] + (uint32_t)pred[c]);
            e.byte_end = (int32_t)(I.scan_end << 1);
            seg[entry] = e;
        }
        const int c = jpeg_dec_block_comp(I, j);
        const int st = jpeg_dec_block<false>(br, huff[I.dc[c] & 3], huff[4 + (I.ac[c] & 3)], pred[c], nullptr);
        if (st) {
            out.status = st;
            return;
        }
        out.count += 1, out.dc[c] = (uint32_t)pred[c];
        j = j + 1 == I.bpm ? 0 : j + 1;
        known = false;
        if (EMIT && ++phase == period) phase = 0, ++entry;
    }
}

// ---------------------------------------------------------------------------------------------------------------- host only, index
// The entries as hh_jpeg_index_tables ships them: first_mcu / mcu_count filled, offsets and predictors zero.
inline void jpeg_idx_blank(const JpegStreamInfo &I, int mps, JpegSegment *seg, int n)
{
    const long long nmcu = (long long)I.mcols * I.mrows;
    memset(seg, 0, (size_t)n * sizeof(JpegSegment));
    for (long long i = 0; i < n; ++i) seg[i].first_mcu = (int32_t)(i * mps), seg[i].mcu_count = (int32_t)(nmcu - i * mps < mps ? nmcu - i * mps : mps);
}

inline const char *jpeg_idx_check_params(int mps, int B)
{
    if (mps < 1) return "mcus_per_segment must be at least 1";
    if (B < JPEG_IDX_SUBSEQ_MIN) return "subseq_bytes below the minimum (hh_jpeg_index_config)";
    if (B % 4) return "subseq_bytes must be a multiple of 4";
    return nullptr;
}

// What hh_debug_jpeg_index_sync_host reports, in the order of its counts[6].
struct JpegIdxCounts {
    long long rounds, iterations, iterations_worst, subsequences, blocks_decoded, blocks_true;
};
static_assert(sizeof(JpegIdxCounts) == 48, "counts[6]");
// The kernel's procedure in plain loops, `lanes` subsequences per round.  A barrier of the kernel is a loop boundary here; where the
// kernel's lanes read their predecessors' exits before any of them writes its own, the loop runs from the last lane down.
inline const char *jpeg_idx_sync_host(const unsigned char *b, long long len, const JpegStreamInfo &I, const JpegDecTables &T, int mps, int B, int lanes,
                                      JpegSegment *seg, int capacity, int *count, int *status, JpegIdxCounts *counts)
{
    *count = 0, *status = 0;
    JpegIdxCounts local;
    memset(&local, 0, sizeof(local));
    if (counts) *counts = local;
    const char *why = jpeg_idx_check_params(mps, B);
    if (why) return why;
    if (lanes < 1 || lanes > (1 << 20)) return "lanes must lie in 1..1048576";
    if (I.restart_interval) return "the stream has a restart interval (use hh_jpeg_restart_segments)";
    const int nseg = jpeg_dec_index_count(I, mps);
    if (nseg > capacity) return "capacity below the number of segments";
    jpeg_idx_blank(I, mps, seg, nseg);
    const int E = jpeg_idx_scan_end(I, len);
    const long long nsub = jpeg_idx_subsequences(I, len, B), total = (long long)I.mcols * I.mrows * I.bpm;
    local.subsequences = nsub;
    JpegIdxKey carry = jpeg_idx_key((int)I.scan_offset, 0, 0);  // lane 0 of the stream starts at the true state
    long long g = 0;
    uint32_t dc[3] = {0, 0, 0};
    int st = 0;
    std::vector<JpegIdxKey> start((size_t)(nsub < lanes ? nsub : lanes));
    std::vector<JpegIdxLane> lane(start.size());
    for (long long k0 = 0; k0 < nsub && g < total && carry != JPEG_IDX_NONE; k0 += lanes) {
        const int n = (int)(nsub - k0 < lanes ? nsub - k0 : lanes);
        local.rounds += 1;
        for (int t = 0; t < n; ++t) {
            start[t] = t == 0 ? carry : jpeg_idx_guess(b, I, k0 + t, B);
            jpeg_idx_walk<false>(b, E, I, T.huff, start[t], jpeg_idx_limit(I, nsub, k0 + t, B), 0, total, mps, nullptr, nullptr, 0, lane[t]);
            local.blocks_decoded += lane[t].count;
        }
        // lane 0 is true, so after k passes lanes 0..k are: at most n passes
        long long passes = 0;
        for (int it = 0; it < n; ++it) {
            bool changed = false;
            for (int t = n - 1; t >= 1; --t) {
                const JpegIdxKey prev = lane[t - 1].exit;
                if (prev == JPEG_IDX_NONE || prev == start[t]) continue;
                start[t] = prev, changed = true;
                jpeg_idx_walk<false>(b, E, I, T.huff, start[t], jpeg_idx_limit(I, nsub, k0 + t, B), 0, total, mps, nullptr, nullptr, 0, lane[t]);
                local.blocks_decoded += lane[t].count;
            }
            if (!changed) break;
            ++passes;
        }
        local.iterations += passes;
        if (passes > local.iterations_worst) local.iterations_worst = passes;
        // the last walk: the lanes up to the first one without an exit are on the true chain
        int bad = n;
        for (int t = n - 1; t >= 0; --t)
            if (lane[t].exit == JPEG_IDX_NONE) bad = t;
        long long gt = g;
        uint32_t dct[3] = {dc[0], dc[1], dc[2]};
        for (int t = 0; t < n; ++t) {
            if (t <= bad && gt < total) {
                JpegIdxLane last;
                jpeg_idx_walk<true>(b, E, I, T.huff, start[t], jpeg_idx_limit(I, nsub, k0 + t, B), gt, total, mps, dct, seg, nseg, last);
                local.blocks_decoded += last.count, local.blocks_true += last.count;
                if (last.status > st) st = last.status;
            }
            gt += lane[t].count;
            for (int c = 0; c < 3; ++c) dct[c] += lane[t].dc[c];
        }
        g = gt, dc[0] = dct[0], dc[1] = dct[1], dc[2] = dct[2];
        carry = bad < n ? JPEG_IDX_NONE : lane[n - 1].exit;
    }
    if (counts) *counts = local;
    if (st) {
        *status = st;
        return "the scan cannot be walked";
    }
    *count = nseg;
    return nullptr;
}
#endif
