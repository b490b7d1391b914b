"""The decoder's rule (hh_jpeg_decode_u8_batch in include/hhrnet.h) restated in plain Python and numpy, written from the rule's text:
marker walk, bit-by-bit Huffman decoding, libjpeg's islow IDCT, fancy upsampling, the colour step.  Nothing here is shared with
csrc/jpeg_dec_math.h.  Step b's overflow behaviour was settled against Pillow: results saturate (clamp(x + 128, 0, 255)); the 1024-entry
wrap of libjpeg's C code is not what Pillow's SIMD build does (checked with quantiser tables up to 8 x the quality-75 ones)."""
import numpy as np

ZZ = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
               57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


class Header:
    pass


def parse(data: bytes) -> Header:
    """Accepted streams only (the refusals are the library's business): -> tables, frame and scan parameters, the scan's bytes."""
    H = Header()
    H.q, H.huff, H.ri = {}, {}, 0
    at = 2
    assert data[:2] == b"\xff\xd8"
    while True:
        assert data[at] == 0xff
        m = data[at + 1]
        L = data[at + 2] << 8 | data[at + 3]
        s = data[at + 4:at + 2 + L]
        at += 2 + L
        if m == 0xdb:
            k = 0
            while k < len(s):
                pq, tq = s[k] >> 4, s[k] & 15
                vals = np.frombuffer(s[k + 1:k + 1 + 64 * (pq + 1)], ">u2" if pq else np.uint8).astype(np.int64)
                nat = np.zeros(64, np.int64)
                nat[ZZ] = vals
                H.q[tq] = nat
                k += 1 + 64 * (pq + 1)
        elif m == 0xc4:
            k = 0
            while k < len(s):
                bits = list(s[k + 1:k + 17])
                vals = s[k + 17:k + 17 + sum(bits)]
                codes, code, p = {}, 0, 0
                for length in range(1, 17):
                    for _ in range(bits[length - 1]):
                        codes[(length, code)] = vals[p]
                        code, p = code + 1, p + 1
                    code <<= 1
                H.huff[(s[k] >> 4, s[k] & 15)] = codes
                k += 17 + sum(bits)
        elif m == 0xdd:
            H.ri = s[0] << 8 | s[1]
        elif m == 0xc0:
            H.h, H.w, H.ncomp = s[1] << 8 | s[2], s[3] << 8 | s[4], s[5]
            H.samp = [(s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15) for c in range(H.ncomp)]
            H.qt = [s[8 + 3 * c] for c in range(H.ncomp)]
            if H.ncomp == 1:
                H.samp = [(1, 1)]
        elif m == 0xda:
            H.tabs = [(s[2 + 2 * c] >> 4, s[2 + 2 * c] & 15) for c in range(H.ncomp)]
            break
    H.scan_at = at
    H.hs, H.vs = H.samp[0]
    H.mcols, H.mrows = -(-H.w // (8 * H.hs)), -(-H.h // (8 * H.vs))
    return H


class _Bits:
    def __init__(self, data: bytes, at: int):
        """The scan from `at` on, unstuffed, as a bit array; a marker ends it and is remembered."""
        out = bytearray()
        self.after = []  # (bits before, marker) for each RSTm met
        i = at
        while i < len(data):
            b = data[i]
            if b == 0xff:
                nxt = data[i + 1] if i + 1 < len(data) else 0xd9
                if nxt == 0:
                    out.append(0xff)
                    i += 2
                    continue
                if 0xd0 <= nxt <= 0xd7:
                    self.after.append((len(out) * 8, nxt))
                    i += 2
                    continue
                break
            out.append(b)
            i += 1
        self.bits = np.unpackbits(np.frombuffer(bytes(out), np.uint8)).tolist()
        self.pos = 0

    def get(self, n: int) -> int:
        v = 0
        for b in self.bits[self.pos:self.pos + n]:
            v = v << 1 | b
        assert self.pos + n <= len(self.bits), "bytes exhausted"
        self.pos += n
        return v

    def symbol(self, codes: dict) -> int:
        code = 0
        for length in range(1, 17):
            code = code << 1 | self.get(1)
            if (length, code) in codes:
                return codes[(length, code)]
        raise AssertionError("bad code")


def _extend(v: int, s: int) -> int:
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def entropy(data: bytes, H: Header):
    """-> (coefficients int64 [nmcu, blocks per MCU, 64] in natural order, not dequantised; the DC predictors before every MCU [nmcu, 3])"""
    br = _Bits(data, H.scan_at)
    comps = [0] * (H.hs * H.vs) + [1, 2] if H.ncomp == 3 else [0]
    nmcu = H.mcols * H.mrows
    coefs = np.zeros((nmcu, len(comps), 64), np.int64)
    preds = np.zeros((nmcu, 3), np.int64)
    pred = [0, 0, 0]
    rst = 0
    for m in range(nmcu):
        if H.ri and m and m % H.ri == 0:
            br.pos = (br.pos + 7) // 8 * 8
            assert br.after[rst] == (br.pos, 0xd0 + (rst & 7)), "RSTm"
            rst += 1
            pred = [0, 0, 0]
        preds[m] = pred
        for j, c in enumerate(comps):
            dc, ac = H.huff[(0, H.tabs[c][0])], H.huff[(1, H.tabs[c][1])]
            s = br.symbol(dc)
            if s:
                pred[c] += _extend(br.get(s), s)
            coefs[m, j, 0] = pred[c]
            k = 1
            while k < 64:
                rs = br.symbol(ac)
                r, s = rs >> 4, rs & 15
                if s:
                    k += r
                    coefs[m, j, ZZ[k]] = _extend(br.get(s), s)
                elif r == 15:
                    k += 15
                else:
                    break
                k += 1
    return coefs, preds


def _idct_1d(v, shift: int):
    """v: int64 [..., 8] along the last axis."""
    z2, z3 = v[..., 2], v[..., 6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 + z3 * -15137
    tmp3 = z1 + z2 * 6270
    z2, z3 = v[..., 0], v[..., 4]
    tmp0, tmp1 = (z2 + z3) << 13, (z2 - z3) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = v[..., 7], v[..., 5], v[..., 3], v[..., 1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    half = 1 << (shift - 1)
    out = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    return np.stack([(o + half) >> shift for o in out], -1)


def idct(blocks: np.ndarray, q: np.ndarray) -> np.ndarray:
    """int64 [..., 64] coefficients, natural order -> uint8-valued samples [..., 8, 8]."""
    x = (blocks * q).reshape(blocks.shape[:-1] + (8, 8))
    x = np.swapaxes(_idct_1d(np.swapaxes(x, -1, -2), 11), -1, -2)  # columns
    x = _idct_1d(x, 18)                                             # rows
    return np.clip(x + 128, 0, 255)


def planes(coefs: np.ndarray, H: Header) -> list:
    """The block-padded component planes."""
    out = []
    nl = H.hs * H.vs
    for c in range(H.ncomp):
        q = H.q[H.qt[c]]
        if c == 0:
            s = idct(coefs[:, :nl], q).reshape(H.mrows, H.mcols, H.vs, H.hs, 8, 8)
            out.append(s.transpose(0, 2, 4, 1, 3, 5).reshape(H.mrows * H.vs * 8, H.mcols * H.hs * 8))
        else:
            s = idct(coefs[:, nl + c - 1], q).reshape(H.mrows, H.mcols, 8, 8)
            out.append(s.transpose(0, 2, 1, 3).reshape(H.mrows * 8, H.mcols * 8))
    return out


def upsample(p: np.ndarray, H: Header) -> np.ndarray:
    """A chroma plane (block padded) -> [h, w] by rule c; the edges are the component's true size."""
    cw, ch = -(-H.w // H.hs), -(-H.h // H.vs)
    p = p[:ch, :cw]
    if H.hs == 1:
        return p[:H.h, :H.w]
    if cw <= 2:
        return np.repeat(np.repeat(p, H.vs, 0), 2, 1)[:H.h, :H.w]
    if H.vs == 2:
        above, below = np.concatenate([p[:1], p[:-1]]), np.concatenate([p[1:], p[-1:]])
        rows = np.empty((2 * ch, cw), np.int64)
        rows[0::2], rows[1::2] = 3 * p + above, 3 * p + below
        bias_even, bias_odd, shift, mul = 8, 7, 4, 1
    else:
        rows, bias_even, bias_odd, shift, mul = p, 1, 2, 2, 1
    left, right = np.concatenate([rows[:, :1], rows[:, :-1]], 1), np.concatenate([rows[:, 1:], rows[:, -1:]], 1)
    out = np.empty((rows.shape[0], 2 * cw), np.int64)
    out[:, 0::2] = (3 * rows + left + bias_even) >> shift
    out[:, 1::2] = (3 * rows + right + bias_odd) >> shift
    if H.vs == 1:  # h2v1: the first and last output samples equal the edge sample
        out[:, 0], out[:, -1] = rows[:, 0], rows[:, -1]
    return out[:H.h, :H.w]


def decode(data: bytes, bgr: bool = False, with_preds: bool = False):
    H = parse(data)
    coefs, preds = entropy(data, H)
    pl = planes(coefs, H)
    Y = pl[0][:H.h, :H.w]
    if H.ncomp == 1:
        out = np.stack([Y, Y, Y], -1)
    else:
        cb, cr = upsample(pl[1], H) - 128, upsample(pl[2], H) - 128
        R = Y + ((91881 * cr + 32768) >> 16)
        B = Y + ((116130 * cb + 32768) >> 16)
        G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
        out = np.clip(np.stack([B, G, R] if bgr else [R, G, B], -1), 0, 255)
    out = out.astype(np.uint8)
    return (out, preds, H) if with_preds else out
