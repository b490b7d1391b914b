#!/usr/bin/env python3
"""Rasterise the font atlas that keypoints/text.py draws with: ASCII 0x20..0x7E of DejaVuSans.ttf in three size classes.

  python3 tools/make_font_atlas.py [path to DejaVuSans.ttf]

Without an argument the font is taken from matplotlib's mpl-data/fonts/ttf/ (DejaVu's licence, LICENSE_DEJAVU next to it, permits
this; its text is committed beside the atlas).  Needs Pillow built with FreeType; nothing at run time does.

The size classes stand for the only font_scales the reference ever passes to put_txt: 0.3, 0.5 and 0.7.  Their pixel sizes 10, 15
and 21 give cap heights (the bitmap height of "H") of 7, 11 and 15 pixels, which this tool asserts.

The file is JSON (text, so that it lives in the package as source does):
  font_scale  [3]          0.3, 0.5, 0.7
  pixel_size  [3]          10, 15, 21
  cap_height  [3]          7, 11, 15
  glyphs      [3][95][6]   per class and character 0x20 + i: advance (getlength rounded half up), bitmap width, bitmap height,
                           left bearing (bitmap column 0 relative to the pen), top (bitmap row 0 relative to the baseline,
                           negative = above), offset of its width * height coverage bytes in the coverage (row-major)
  coverage    [3][95]      per class and character its 8-bit coverage bytes as a hex string; all of them back to back, in this order,
                           are the coverage buffer the offsets count in; a glyph without ink has width = height = 0
"""
import json
import math
import os
import sys

import numpy as np
from PIL import ImageFont, features

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "pytorch-human-pose_amd", "keypoints", "data", "dejavu_sans_atlas.json")
SCALES, PIXELS, CAPS = (0.3, 0.5, 0.7), (10, 15, 21), (7, 11, 15)
FIRST, LAST = 0x20, 0x7E


def main():
    if not features.check("freetype2"):
        raise SystemExit("Pillow without FreeType")
    if len(sys.argv) > 1:
        ttf = sys.argv[1]
    else:
        import matplotlib
        ttf = os.path.join(os.path.dirname(matplotlib.__file__), "mpl-data", "fonts", "ttf", "DejaVuSans.ttf")
    glyphs = np.zeros((len(PIXELS), LAST - FIRST + 1, 6), np.int32)
    coverage, caps = [[] for _ in PIXELS], []
    at = 0
    for k, px in enumerate(PIXELS):
        font = ImageFont.truetype(ttf, px)
        caps.append(font.getmask("H", mode="L").size[1])
        for i, code in enumerate(range(FIRST, LAST + 1)):
            ch = chr(code)
            mask, (left, top) = font.getmask2(ch, mode="L", anchor="ls")
            w, h = mask.size
            bits = np.frombuffer(bytes(mask), np.uint8).reshape(h, w) if w * h else np.zeros((0, 0), np.uint8)
            if not bits.any():
                w = h = left = top = 0
                bits = bits[:0, :0]
            glyphs[k, i] = (math.floor(font.getlength(ch) + 0.5), w, h, left, top, at)
            coverage[k].append(bits.tobytes().hex())
            at += w * h
    if tuple(caps) != CAPS:
        raise SystemExit(f"cap heights {caps} at pixel sizes {PIXELS}: not {CAPS} (another FreeType or font file?)")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    rows = lambda items: "[\n" + ",\n".join(json.dumps(v, separators=(",", ":")) for v in items) + "\n]"  # noqa: E731 (one item a line)
    with open(OUT, "w") as f:
        f.write("{\n" + ",\n".join([f'"font_scale":{json.dumps(list(SCALES))}', f'"pixel_size":{json.dumps(list(PIXELS))}', f'"cap_height":{json.dumps(caps)}',
                                   '"glyphs":[' + ",".join(rows(g) for g in glyphs.tolist()) + "]",
                                   '"coverage":[' + ",".join(rows(c) for c in coverage) + "]"]) + "\n}\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", at, "coverage bytes; cap heights", caps)


if __name__ == "__main__":
    main()
