"""The baseline JPEG rule of include/hhrnet.h (hh_jpeg_encode_u8_batch) restated in numpy from its text, independently of csrc/jpeg_math.h:
padding, colour, 4:2:0 mean, the fixed-point FDCT with its table formed from the cosine formula, the quantiser, zigzag, the Annex K
Huffman tables, restart intervals per MCU row, byte stuffing, the segment order.  `encode` also reports what the entropy coder met, so
that a test can assert that its grid reached every path."""
import numpy as np

QBASE = np.array([
    [16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37, 29, 40, 58, 51, 61, 60, 57, 51,
     56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101, 103, 99],
    [17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66] + [99] * 50], dtype=np.int64)  # Annex K, zigzag order
DC_BITS = [[0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]]
DC_VALS = [list(range(12)), list(range(12))]
AC_BITS = [[0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119]]
_RUNS = [r << 4 | s for r in range(16) for s in range(1, 11)]


def _ac_vals(head: list) -> list:
    """HUFFVAL of an AC table: Annex K lists the short codes' symbols explicitly and then every remaining (run, size) symbol ascending."""
    rest = sorted(set(_RUNS + [0x00, 0xF0]) - set(head))
    return head + rest


AC_VALS = [
    _ac_vals([1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51,
              98, 114, 130]),
    _ac_vals([0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98, 114,
              209, 10, 22, 36, 52, 225, 37, 241])]
assert all(len(v) == 162 and sum(b) == 162 for v, b in zip(AC_VALS, AC_BITS))


def zigzag_order() -> np.ndarray:
    """ZZ[k] = the natural index v * 8 + u of zigzag position k: the anti-diagonals, alternating direction."""
    order = []
    for d in range(15):
        cells = [(v, d - v) for v in range(8) if 0 <= d - v < 8]
        order += cells if d % 2 else cells[::-1]
    return np.array([v * 8 + u for v, u in order])


ZZ = zigzag_order()


def fdct_table() -> np.ndarray:
    u, x = np.mgrid[:8, :8]
    c = np.where(u == 0, np.sqrt(1 / 8), 0.5)
    return np.rint(2 ** 14 * c * np.cos((2 * x + 1) * u * np.pi / 16)).astype(np.int64)


T = fdct_table()


def quant_tables(quality: int) -> np.ndarray:
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((QBASE * scale + 50) // 100, 1, 255)


def huffman_codes(bits: list, vals: list) -> dict:
    codes, code, p = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[vals[p]] = (code, length)
            code += 1
            p += 1
        code <<= 1
    return codes


def ycc(rgb: np.ndarray):
    R, G, B = (rgb[..., c].astype(np.int64) for c in range(3))
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    return Y, Cb, Cr


def fdct(samples: np.ndarray):
    """[..., 8, 8] samples (value - 128) -> (A, F)"""
    A = (samples @ T.T + 1024) >> 11          # A[y][u] = sum_x s[y][x] T[u][x]
    F = np.swapaxes(np.swapaxes(A, -1, -2) @ T.T, -1, -2)  # F[v][u] = sum_y A[y][u] T[v][y]
    return A, F


def quantise(F: np.ndarray, Qzz: np.ndarray) -> np.ndarray:
    """F [..., 8, 8] -> zigzag coefficients [..., 64]"""
    Fz = F.reshape(F.shape[:-2] + (64,))[..., ZZ]
    q = np.sign(Fz) * ((np.abs(Fz) + (Qzz << 16)) // (Qzz << 17))
    q[..., 1:] = np.clip(q[..., 1:], -1023, 1023)
    q[..., 0] = np.clip(q[..., 0], -1024, 1023)
    return q


def coefficients(image: np.ndarray, quality: int, subsampling: int, bgr: bool = False):
    """-> (luma [by, bx, 64], cb [cy, cx, 64], cr) zigzag coefficients of the padded frame"""
    img = np.asarray(image)
    if bgr:
        img = img[..., ::-1]
    h, w = img.shape[:2]
    m = 16 if subsampling == 420 else 8
    img = np.pad(img, ((0, -h % m), (0, -w % m), (0, 0)), mode="edge")
    Y, Cb, Cr = ycc(img)
    if subsampling == 420:
        Cb, Cr = ((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2 for p in (Cb, Cr))
    Q = quant_tables(quality)
    out = []
    for plane, t in ((Y, 0), (Cb, 1), (Cr, 1)):
        H, W = plane.shape
        blocks = (plane - 128).reshape(H // 8, 8, W // 8, 8).swapaxes(1, 2)
        out.append(quantise(fdct(blocks)[1], Q[t]))
    return out


def _size(v: int) -> int:
    return int(abs(v)).bit_length()


def _value_bits(v: int, s: int) -> int:
    return (v if v >= 0 else v - 1) & ((1 << s) - 1)


def header(h: int, w: int, quality: int, subsampling: int, mcols: int) -> bytes:
    def seg(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body
    Q = quant_tables(quality)
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for t in range(2):
        out += seg(0xDB, bytes([t]) + bytes(int(v) for v in Q[t]))
    out += seg(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([3, 1, 0x22 if subsampling == 420 else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for cls, bits, vals in ((0x00, DC_BITS[0], DC_VALS[0]), (0x01, DC_BITS[1], DC_VALS[1]), (0x10, AC_BITS[0], AC_VALS[0]), (0x11, AC_BITS[1], AC_VALS[1])):
        out += seg(0xC4, bytes([cls]) + bytes(bits) + bytes(vals))
    out += seg(0xDD, mcols.to_bytes(2, "big"))
    out += seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def encode(image: np.ndarray, quality: int = 90, subsampling: int = 420, bgr: bool = False):
    """-> (stream, stats).  stats: stuffed (FF 00 pairs), zrl, no_eob (blocks whose coefficient 63 is non-zero), restarts (the m of every
    RSTm written, in order), mcu_rows, nonzero_ac, nonzero_dc_diff, blocks, max_block_bits."""
    subsampling = int(subsampling)
    h, w = np.asarray(image).shape[:2]
    luma, cb, cr = coefficients(image, quality, subsampling, bgr)
    dc = [huffman_codes(DC_BITS[t], DC_VALS[t]) for t in range(2)]
    ac = [huffman_codes(AC_BITS[t], AC_VALS[t]) for t in range(2)]
    mrows, mcols = cb.shape[:2] if subsampling == 420 else luma.shape[:2]
    stats = dict(stuffed=0, zrl=0, no_eob=0, restarts=[], mcu_rows=mrows, nonzero_ac=0, nonzero_dc_diff=0, blocks=0, max_block_bits=0)
    out = bytearray(header(h, w, quality, subsampling, mcols))
    for my in range(mrows):
        acc, nbits = 0, 0
        pred = [0, 0, 0]
        for mx in range(mcols):
            if subsampling == 420:
                blocks = [(0, luma[2 * my, 2 * mx]), (0, luma[2 * my, 2 * mx + 1]), (0, luma[2 * my + 1, 2 * mx]), (0, luma[2 * my + 1, 2 * mx + 1]),
                          (1, cb[my, mx]), (2, cr[my, mx])]
            else:
                blocks = [(0, luma[my, mx]), (1, cb[my, mx]), (2, cr[my, mx])]
            for comp, zz in blocks:
                t = 0 if comp == 0 else 1
                before = nbits
                diff = int(zz[0]) - pred[comp]
                pred[comp] = int(zz[0])
                s = _size(diff)
                code, length = dc[t][s]
                acc, nbits = (acc << (length + s)) | (code << s) | _value_bits(diff, s), nbits + length + s
                stats["nonzero_dc_diff"] += diff != 0
                last = 0
                for k in np.nonzero(zz[1:])[0] + 1:
                    k, v = int(k), int(zz[k])
                    run = k - last - 1
                    while run > 15:
                        code, length = ac[t][0xF0]
                        acc, nbits = (acc << length) | code, nbits + length
                        run -= 16
                        stats["zrl"] += 1
                    s = _size(v)
                    code, length = ac[t][run << 4 | s]
                    acc, nbits = (acc << (length + s)) | (code << s) | _value_bits(v, s), nbits + length + s
                    last = k
                    stats["nonzero_ac"] += 1
                if last != 63:
                    code, length = ac[t][0x00]
                    acc, nbits = (acc << length) | code, nbits + length
                else:
                    stats["no_eob"] += 1
                stats["blocks"] += 1
                stats["max_block_bits"] = max(stats["max_block_bits"], nbits - before)
        fill = -nbits % 8
        acc, nbits = (acc << fill) | ((1 << fill) - 1), nbits + fill
        raw = acc.to_bytes(nbits // 8, "big")
        stats["stuffed"] += raw.count(0xFF)
        out += raw.replace(b"\xff", b"\xff\x00")
        if my + 1 < mrows:
            out += bytes([0xFF, 0xD0 + (my & 7)])
            stats["restarts"].append(my & 7)
    out += b"\xff\xd9"
    return bytes(out), stats
