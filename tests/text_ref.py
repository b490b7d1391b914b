"""numpy restatement of the text labels (the rule at hh_text_labels_u8_batch in include/hhrnet.h): the layout of put_txt
(utils/image.py:64-119 of the reference) and the two pixel rules, independent of the C code and of keypoints/text.py.  Only the
atlas FILE is shared: it is data.  Also the recording stand-ins for cv2 that tools/make_text_golden.py binds."""
import json
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATLAS = os.path.join(REPO, "pytorch-human-pose_amd", "keypoints", "data", "dejavu_sans_atlas.json")
GRAY, WHITE = (128, 128, 128), (255, 255, 255)
BOX, GLYPH = 0, 1

with open(ATLAS) as _f:
    _z = json.load(_f)
CAP = [int(v) for v in _z["cap_height"]]
GLYPHS = np.array(_z["glyphs"], np.int64)  # [3,95,6]: advance, w, h, left, top, offset
COVERAGE = np.frombuffer(bytes.fromhex("".join("".join(rows) for rows in _z["coverage"])), np.uint8)


def size_class(font_scale) -> int:
    """0.3 / 0.5 / 0.7 -> 0 / 1 / 2; anything else the nearest, the smaller on a tie (in tenths of thousandths: exact for 0.4, 0.6)."""
    t = round(float(font_scale) * 10000)
    return min(range(3), key=lambda k: (abs((3000, 5000, 7000)[k] - t), k))


def codes(label):
    return [(ord(c) if 0x20 <= ord(c) <= 0x7E else ord("?")) - 0x20 for c in label]


def text_size(label, font_scale):
    k = size_class(font_scale)
    return sum(int(GLYPHS[k, c, 0]) for c in codes(label)), CAP[k]


def image(seed, h, w):
    """A seeded frame of 4 x 4 blocks."""
    blocks = np.random.default_rng(seed).integers(0, 256, ((h + 3) // 4, (w + 3) // 4, 3), dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(blocks, 4, 0), 4, 1)[:h, :w])


# ---------------------------------------------------------------- the two pixel rules, on an image in place, clipped to it
def _window(img, x0, y0, x1, y1):
    """The inclusive rectangle clipped to the image as slices, or None."""
    h, w = img.shape[:2]
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, w - 1), min(y1, h - 1)
    return (slice(y0, y1 + 1), slice(x0, x1 + 1)) if x0 <= x1 and y0 <= y1 else None


def fill_box(img, x0, y0, x1, y1, colour):
    win = _window(img, x0, y0, x1, y1)
    if win is not None:
        img[win] = np.array(colour, np.uint8)


def blend(a, w0, b, w1):
    """rintf(a * w0 + b * w1), products and sum rounded to fp32 one by one, clamped to 0..255."""
    pa, pb = np.asarray(a, np.float32) * np.float32(w0), np.asarray(b, np.float32) * np.float32(w1)
    return np.clip(np.rint((pa + pb).astype(np.float32)), 0, 255).astype(np.uint8)


def blend_box(img, x0, y0, x1, y1, colour, w0, w1):
    win = _window(img, x0, y0, x1, y1)
    if win is not None:
        img[win] = blend(img[win], w0, np.array(colour, np.uint8)[None, None, :], w1)


def draw_bitmap(img, cx, cy, bits, colour):
    """(pix * (255 - c) + col * c + 127) // 255 where the bitmap, top-left at (cx, cy), meets the image."""
    bh, bw = bits.shape
    win = _window(img, cx, cy, cx + bw - 1, cy + bh - 1)
    if win is None:
        return
    c = bits[win[0].start - cy:win[0].stop - cy, win[1].start - cx:win[1].stop - cx].astype(np.int64)[..., None]
    img[win] = ((img[win].astype(np.int64) * (255 - c) + np.array(colour, np.int64)[None, None, :] * c + 127) // 255).astype(np.uint8)


def bitmap(k, code):
    _, w, h, _, _, off = (int(v) for v in GLYPHS[k, code])
    return COVERAGE[off:off + w * h].reshape(h, w)


def draw_text(img, label, x, y, font_scale, colour):
    """The label's glyphs from the baseline-left origin (x, y)."""
    k = size_class(font_scale)
    for c in codes(label):
        adv, w, h, left, top, _ = (int(v) for v in GLYPHS[k, c])
        if w and h:
            draw_bitmap(img, x + left, y + top, bitmap(k, c), colour)
        x += adv


def put_txt(image, labels, vspace=10, font_scale=0.5, thickness=1, loc="tl", bg_color=GRAY, txt_color=WHITE, alpha=1.0):
    """The reference's put_txt with the project's metrics and rasteriser, primitives clipped to the frame -> a drawn copy."""
    assert thickness == 1
    img = image.copy()
    img_h, img_w = img.shape[:2]
    txt_h, txt_w = vspace, 0
    for label in labels:
        width, height = text_size(label, font_scale)
        txt_h += height + vspace
        txt_w = max(txt_w, width)
    txt_w += 2 * vspace
    y = vspace if loc in ("tl", "tc", "tr") else img_h - txt_h + vspace
    x = vspace if loc in ("tl", "bl") else img_w - txt_w + vspace if loc in ("tr", "br") else img_w // 2 - txt_w // 2 + vspace // 2
    _x, _y = x - vspace, y - vspace
    if alpha < 1:
        blend_box(img, _x, _y, _x + txt_w - 1, _y + txt_h - 1, bg_color, np.float32(1.0 - alpha), np.float32(alpha))
    else:
        fill_box(img, _x, _y, _x + txt_w, _y + txt_h, bg_color)
    for label in labels:
        _, height = text_size(label, font_scale)
        draw_text(img, label, x, y + height, font_scale, txt_color)
        y += height + vspace
    return img


def plot_scale(h, w):
    m = min(h, w)
    return 0.3 if 0 < m <= 224 else 0.5 if 224 < m <= 336 else 0.7


def plot_top_preds(image, probs, idx2label, k=5, target_label=None):
    """classification/visualization.py of the reference on put_txt above."""
    fs = plot_scale(*image.shape[:2])
    top = list(reversed(np.argsort(probs)[-k:]))
    out = put_txt(image, [f"{probs[i]:.3f}:  {idx2label[i]}" for i in top], alpha=0.8, font_scale=fs)
    if target_label is not None:
        out = put_txt(out, ["Target:", str(target_label)], loc="br", txt_color=(80, 255, 80), alpha=0.8, font_scale=fs)
    return out


def apply_table(image, table):
    """A primitive table (rows with the fields of hh_text_prim) on a copy of the image, row by row."""
    img = image.copy()
    for p in table:
        x0, y0, x1, y1 = int(p["x0"]), int(p["y0"]), int(p["x1"]), int(p["y1"])
        if x1 < x0 or y1 < y0:
            continue
        if int(p["kind"]) == BOX:
            if int(p["A"]):
                fill_box(img, x0, y0, x1, y1, p["rgb"])
            else:
                blend_box(img, x0, y0, x1, y1, p["rgb"], p["c"], p["s"])
        else:
            w, h, off = int(p["A"]), int(p["B"]), int(p["c"])
            bits = np.zeros((h, w), np.uint8)
            # only the part inside the box is drawn (the box lies inside the bitmap)
            cx, cy = int(p["cx"]), int(p["cy"])
            full = COVERAGE[off:off + w * h].reshape(h, w)
            bits[y0 - cy:y1 - cy + 1, x0 - cx:x1 - cx + 1] = full[y0 - cy:y1 - cy + 1, x0 - cx:x1 - cx + 1]
            draw_bitmap(img, cx, cy, bits, p["rgb"])
    return img


# ---------------------------------------------------------------- recording stand-ins for cv2 (tools/make_text_golden.py)
class Recorder:
    """getTextSize answers from the atlas; rectangle / addWeighted / putText log their arguments and draw by the rule above.
    `calls`: in order, ("box", x0, y0, x1, y1 inclusive in the frame, opaque, w0, w1, colour) and ("text", string, x, y, font_scale,
    colour, thickness)."""
    FONT = 0

    def __init__(self):
        self.calls = []

    def getTextSize(self, text, font, font_scale, thickness):
        assert font == self.FONT
        return text_size(text, font_scale), 0

    def rectangle(self, img, pt1, pt2, color, thickness):
        assert thickness == -1
        fill_box(img, pt1[0], pt1[1], pt2[0], pt2[1], color)
        self.calls.append(["box", int(pt1[0]), int(pt1[1]), int(pt2[0]), int(pt2[1]), 1, 0.0, 1.0, tuple(int(c) for c in color), img])
        return img

    def addWeighted(self, a, wa, b, wb, gamma):
        """a: a view of the frame (its place is read from its address), b: the rectangle-filled patch of the call just before."""
        assert gamma == 0.0 and a.shape == b.shape
        last = self.calls[-1]
        assert last[0] == "box" and last[-1] is b and last[1:3] == [0, 0] and last[3] >= b.shape[1] - 1 and last[4] >= b.shape[0] - 1
        assert (b == np.array(last[8], np.uint8)).all(), "the patch is not one colour"
        frame = a.base
        off = a.__array_interface__["data"][0] - frame.__array_interface__["data"][0]
        y, x = off // frame.strides[0], off % frame.strides[0] // frame.strides[1]
        assert a.strides == frame.strides and 0 <= y and y + a.shape[0] <= frame.shape[0] and 0 <= x and x + a.shape[1] <= frame.shape[1]
        self.calls[-1] = ["box", int(x), int(y), int(x + a.shape[1] - 1), int(y + a.shape[0] - 1), 0, float(wa), float(wb), last[8], frame]
        return blend(a, np.float32(wa), b, np.float32(wb))

    def putText(self, img, text, org, font, font_scale, color, thickness):
        assert font == self.FONT
        draw_text(img, text, int(org[0]), int(org[1]), font_scale, color)
        self.calls.append(["text", str(text), int(org[0]), int(org[1]), float(font_scale), tuple(int(c) for c in color), int(thickness)])
        return img

    def rows(self):
        """-> (boxes float64 [Nb,11]: x0, y0, x1, y1, opaque, w0, w1, r, g, b, position in the call order;
               texts float64 [Nt,8]: x, y, font_scale, r, g, b, thickness, position in the call order;  strings [Nt])."""
        boxes = [[*c[1:8], *c[8], i] for i, c in enumerate(self.calls) if c[0] == "box"]
        texts = [[c[2], c[3], c[4], *c[5], c[6], i] for i, c in enumerate(self.calls) if c[0] == "text"]
        return (np.array(boxes, np.float64).reshape(-1, 11), np.array(texts, np.float64).reshape(-1, 8), [c[1] for c in self.calls if c[0] == "text"])
